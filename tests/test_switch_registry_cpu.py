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


TABLE = os.path.join(PKG, "csrc", "switches.hpp")
# read outside the table, each for a reason the source states beside the read: name -> file
OUTSIDE_THE_TABLE = {
    "GFSHIP_FAULT_DROP_HANDOFF": "csrc/relax_skew_loop.hip",
    "GFSHIP_RCCL_LIBRARY": "csrc/transport.hip",
    "GFSHIP_CC": "csrc/host/gfs_function.hpp",
}
README_RULE = "Every switch of the library is looked up when a domain or a tree is created"


def _table_lines():
    """the lines of read_switches (): [(member, [names])], one per environment variable"""
    body = _read(TABLE)
    body = body[body.index("inline Switches read_switches ()"):]
    body = body[body.index("Switches s;") + len("Switches s;"):body.index("return s;")]
    return [(line.split("=")[0].strip(), re.findall(r'"(GFSHIP_[A-Z0-9_]+)"', line))
            for line in body.splitlines() if line.strip()]


def _getenv_calls():
    """every getenv under csrc/: [(path relative to the package, its argument as written)]"""
    calls = []
    for path in glob.glob(os.path.join(PKG, "csrc", "**", "*"), recursive=True):
        if os.path.splitext(path)[1] in (".hip", ".hpp", ".cpp", ".h"):
            for m in re.finditer(r'\bgetenv\s*\(\s*([^)]*?)\s*\)', _read(path)):
                calls.append((os.path.relpath(path, PKG), m.group(1)))
    return calls


def _names_read_by_the_sources():
    names = {}
    for member, found in _table_lines():
        for name in found:
            names.setdefault(name, set()).add(os.path.relpath(TABLE, ROOT))
    for name, path in OUTSIDE_THE_TABLE.items():
        names.setdefault(name, set()).add(os.path.join("gerris-fft-particles_amd", path))
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
    assert not set(S.REGISTRY_NAMES) & set(S.PINNED_ELSEWHERE)


def test_variables_pinned_elsewhere_are_set_by_the_file_named():
    for name, path in S.PINNED_ELSEWHERE.items():
        assert name in _read(os.path.join(ROOT, path)), (name, path)


def test_read_once_list_matches_the_sources():
    """nothing is read once per process or per call any more: the table of csrc/switches.hpp, with one
    line, one member and one variable per line, and the three reads allowed outside it are every getenv
    under csrc/"""
    lines = _table_lines()
    assert len(lines) >= 35
    for member, found in lines:
        assert re.fullmatch(r"s\.\w+", member) and len(set(found)) == 1, (member, found)
    members = [m for m, _ in lines]
    names = [f[0] for _, f in lines]
    assert len(set(members)) == len(members) and len(set(names)) == len(names)
    # every member of the struct is filled by a line of the table
    struct = _read(TABLE)
    struct = struct[struct.index("struct Switches {"):struct.index("bool patch () const")]
    declared = re.findall(r"^\s*(?:bool|int) (\w+) = ", struct, flags=re.M)
    assert sorted("s." + d for d in declared) == sorted(members)
    outside = [(path, arg) for path, arg in _getenv_calls() if path != "csrc/switches.hpp"]
    assert sorted(outside) == sorted((path, '"%s"' % name) for name, path in OUTSIDE_THE_TABLE.items()), outside
    # the table itself calls getenv in its three helpers only, on their argument
    assert [arg for path, arg in _getenv_calls() if path == "csrc/switches.hpp"] == ["name"] * 3


def test_every_variable_is_documented():
    docs = _read(os.path.join(ROOT, "README.md")) + _read(os.path.join(ROOT, "DESIGN.md"))
    readme = _read(os.path.join(ROOT, "README.md"))
    for name in _names_read_by_the_sources():
        assert name in docs, "%s is documented neither in README.md nor in DESIGN.md" % name
    for name in S.REGISTRY_NAMES:
        assert name in readme, "%s is missing from README.md's list of switches" % name
    assert README_RULE in " ".join(readme.split()), "README.md does not state when the switches are looked up"
    assert "read once per process, at the first call" not in " ".join(readme.split())


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
