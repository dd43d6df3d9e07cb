"""The registry of tests/switch_cases.py is complete and alive, without a GPU: every GFSHIP_* variable
the sources read is either pinned by a registry switch, pinned by the test file the registry names,
or listed as not kernel-selecting; nothing in the registry is stale; every name is documented; the
families the evidence names exist; the oracle half of the cases up to 64^3 runs and is deterministic."""
import glob
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import gfship
import switch_cases as S
from conftest import ROOT

PKG = os.path.join(ROOT, "gerris-fft-particles_amd")


def _read(path):
    with open(path, errors="replace") as f:
        return f.read()


def _names_read_by_the_sources():
    names = {}
    for path in glob.glob(os.path.join(PKG, "csrc", "**", "*"), recursive=True):
        if os.path.splitext(path)[1] in (".hip", ".hpp", ".cpp", ".h"):
            for m in re.finditer(r'getenv\s*\(\s*"(GFSHIP_[A-Z0-9_]+)"', _read(path)):
                names.setdefault(m.group(1), set()).add(os.path.relpath(path, ROOT))
    for path in glob.glob(os.path.join(PKG, "gfship", "**", "*.py"), recursive=True) + [os.path.join(ROOT, "bench.py")]:
        for m in re.finditer(r'environ(?:\.get\s*\(|\s*\[)\s*"(GFSHIP_[A-Z0-9_]+)"', _read(path)):
            names.setdefault(m.group(1), set()).add(os.path.relpath(path, ROOT))
    return names


def test_every_variable_the_sources_read_is_accounted_for():
    read = _names_read_by_the_sources()
    assert len(read) >= 40, sorted(read)
    known = set(S.REGISTRY_NAMES) | set(S.NOT_KERNEL_SELECTING) | set(S.PINNED_ELSEWHERE)
    assert not set(read) - known, \
        "read by the sources but neither a registry switch nor listed: %s" % \
        {n: sorted(read[n]) for n in set(read) - known}
    assert not known - set(read), "in tests/switch_cases.py but no longer read by any source: %s" % sorted(known - set(read))
    # one home per name
    assert not set(S.REGISTRY_NAMES) & set(S.NOT_KERNEL_SELECTING)
    assert not set(S.NOT_KERNEL_SELECTING) & set(S.PINNED_ELSEWHERE)
    assert set(S.READ_ONCE) <= set(S.REGISTRY_NAMES)


def test_variables_pinned_elsewhere_are_set_by_the_file_named():
    for name, path in S.PINNED_ELSEWHERE.items():
        assert name in _read(os.path.join(ROOT, path)), (name, path)


def test_read_once_list_matches_the_sources():
    """a variable read into a function-level static must be set before the library is loaded"""
    static = set()
    for path in glob.glob(os.path.join(PKG, "csrc", "*.hip")):
        text = _read(path)
        static |= set(re.findall(r'static const bool \w+ = getenv \("(GFSHIP_[A-Z0-9_]+)"\)', text))
        # static int n = 0; if (!n) { e = getenv (...) }
        for m in re.finditer(r'static int (\w+) = 0;\s*if \(!\1\) \{\s*const char \* e = getenv \("(GFSHIP_[A-Z0-9_]+)"\)', text):
            static.add(m.group(2))
    assert static == set(S.READ_ONCE), static ^ set(S.READ_ONCE)


def test_every_variable_is_documented():
    docs = _read(os.path.join(ROOT, "README.md")) + _read(os.path.join(ROOT, "DESIGN.md"))
    readme = _read(os.path.join(ROOT, "README.md"))
    for name in _names_read_by_the_sources():
        assert name in docs, "%s is documented neither in README.md nor in DESIGN.md" % name
    for name in S.REGISTRY_NAMES:
        assert name in readme, "%s is missing from README.md's list of switches" % name
    for name in S.READ_ONCE:
        assert re.search(r"read once[^\n]*(\n[^\n]+)*%s\b" % name, readme), \
            "README.md does not say that %s is read once per process" % name


def test_design_table_matches_the_registry():
    """DESIGN.md section 5 keeps one row per registry switch: | `switch` | families | cases |"""
    text = _read(os.path.join(ROOT, "DESIGN.md"))
    rows = {m.group(1): (m.group(2), m.group(3)) for m in
            re.finditer(r"^\| `([^`|]+)` \| ([^|]*) \| ([^|]*) \|", text, flags=re.M)}
    for name, sw in S.SWITCHES.items():
        assert name in rows, "DESIGN.md section 5 has no row for the switch %r" % name
        fam, cases = rows[name]
        for case, ev in sw["cases"].items():
            assert case in cases, (name, case)
            for f in ev["on"] + tuple(ev["values"]):
                assert f in fam, (name, f)


def test_kernel_count_names_mirror_the_header():
    text = re.sub(r"/\*.*?\*/", "", _read(os.path.join(ROOT, "include", "gfship.h")), flags=re.S)
    body = text[text.index("GFSHIP_KC_PREDICT_SWEEP"):text.index("GFSHIP_KC_COUNT")]
    assert tuple(re.findall(r"GFSHIP_KC_([A-Z0-9_]+)", body)) == gfship.KERNEL_COUNT_NAMES
    assert set(gfship.KERNEL_COUNT_VALUES) <= set(gfship.KERNEL_COUNT_NAMES)


def test_evidence_names_existing_families_and_cases():
    assert "default" in S.SWITCHES and S.SWITCHES["default"]["env"] == {}
    assert set(S.SWITCHES["default"]["cases"]) == set(S.CASES)      # the control runs every case
    for name, sw in S.SWITCHES.items():
        assert sw["cases"], name
        for k in sw["env"]:
            assert k.startswith("GFSHIP_")
        for case, ev in sw["cases"].items():
            assert case in S.CASES, (name, case)
            for f in ev["on"] + ev["off"]:
                assert f in gfship.KERNEL_COUNT_NAMES and f not in gfship.KERNEL_COUNT_VALUES, (name, f)
            for f in ev["values"]:
                assert f in gfship.KERNEL_COUNT_VALUES, (name, f)
            if name != "default" and not ev["values"]:
                # a switch leaves evidence on at least one of its cases
                assert any(e["on"] or e["values"] for e in sw["cases"].values()), name


def test_worker_lists_the_registry_without_touching_the_device():
    env = {k: v for k, v in os.environ.items() if not k.startswith("GFSHIP_")}
    env["HIP_VISIBLE_DEVICES"] = ""         # would make any use of the device an error
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "switch_worker.py"), "--list"],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("SWITCHES ")][-1]
    assert json.loads(line[len("SWITCHES "):]) == {n: sw["env"] for n, sw in S.SWITCHES.items()}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "switch_worker.py"), "NO_SUCH_SWITCH", "x"],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "unknown switch" in r.stderr


@pytest.mark.timeout(900)
@pytest.mark.parametrize("case", S.CPU_CASES)
def test_oracle_half_runs_and_is_deterministic(case):
    a = S.run_case(case, "oracle")[0]
    b = S.run_case(case, "oracle")[0]
    assert set(a) == set(b) and len(a) > 10
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    full = [k for k in a if np.ndim(a[k]) > 1]
    assert full and any(k.endswith("#") for k in a), "a case keeps its last step in full and digests of the others"
    for k in full:
        assert np.isfinite(a[k]).all(), k
