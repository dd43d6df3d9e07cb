"""Every kernel-selecting GFSHIP_* switch against the oracle, one process per setting.

A domain looks its switches up when it is created (csrc/switches.hpp;
test_three_domains_of_one_process_each_follow_their_own_environment).  A process per setting keeps a
fault under one switch from the others: per setting of tests/switch_cases.py:SWITCHES this file starts
ONE child (tests/switch_worker.py, a fresh interpreter with the setting in its environment before the
library is loaded; one child at a time), then compares every case the child ran with the oracle --
np.array_equal on every field of the last step, the SHA-256 of every field of the earlier steps, ==
on dt, t, niter, residual.infty, cfl, and rel = 1e-12 (RTOL_SUM of tests/test_gpu_fullsize.py) on the
summed norms -- and checks the *evidence*: the tallies of gfship_domain_kernel_counts must show
that the selected branch ran under the switch and did not in the control run ("default", the empty
environment), and the converse for the branch it replaces.  The oracle half of a case is computed
once per session and shared by all switches.

If a child ends by a signal, with exit status 134 / 139, or by its time limit, nothing more is
started: every remaining switch fails at once with that child's stderr.  No retries.

Cost: one child per setting (29), not one per setting and case, and one oracle run per case per
session.  The oracle halves take 72 s on one CPU core together (tg128 18 s, each vcycle128_* 9 s,
visc64 10 s, the others 1-4 s).  The wall time of the children on an MI355X has not been measured
yet (nobody has measured the start-up cost of a child there): put the figure here, and in DESIGN.md
section 5.1, from the first run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import switch_cases as S
from conftest import ROOT

pytestmark = pytest.mark.gpu

_STOP = {}          # set by the first child that faulted, hung or ran out of time
_ORACLE = {}        # case -> record
_RUNS = {}          # "default" -> {case: (record, tallies, extra)}


def _oracle(case):
    if case not in _ORACLE:
        _ORACLE[case] = S.run_case(case, "oracle")[0]
    return _ORACLE[case]


def _child(switch, outdir):
    """the device half of every case of `switch', from a process of its own; cached per session"""
    if switch in _RUNS:
        return _RUNS[switch]
    if _STOP:
        pytest.fail("not started: the child of %r ended with %s\n%s" %
                    (_STOP["switch"], _STOP["how"], _STOP["stderr"]), pytrace=False)
    env = {k: v for k, v in os.environ.items() if not k.startswith("GFSHIP_") or k in S.KEEP_IN_CHILD}
    cmd = [sys.executable, os.path.join(ROOT, "tests", "switch_worker.py"), switch, str(outdir)]
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=S.child_timeout(switch))
        rc, err, out = r.returncode, r.stderr, r.stdout
        how = None
        if rc < 0 or rc in (134, 139, 124, 137):
            how = "signal %d" % -rc if rc < 0 else "exit status %d" % rc
    except subprocess.TimeoutExpired as e:
        rc, out = None, ""
        err = e.stderr.decode(errors="replace") if isinstance(e.stderr, bytes) else (e.stderr or "")
        how = "its time limit of %d s" % S.child_timeout(switch)
    if how:
        _STOP.update(switch=switch, how=how, stderr=err[-4000:])
        pytest.fail("the child of %r ended with %s; no further child is started\n%s" %
                    (switch, how, err[-4000:]), pytrace=False)
    assert rc == 0, "switch_worker %s: exit status %d\n%s\n%s" % (switch, rc, out[-2000:], err[-4000:])
    line = [x for x in out.splitlines() if x.startswith("SWITCHWORKER ")][-1]
    info = json.loads(line[len("SWITCHWORKER "):])
    assert info["env"] == S.SWITCHES[switch]["env"]
    runs = {}
    for case in S.SWITCHES[switch]["cases"]:
        with np.load(os.path.join(str(outdir), case + ".npz")) as z:
            rec = {k: z[k] for k in z.files}
        with open(os.path.join(str(outdir), case + ".json")) as f:
            meta = json.load(f)
        runs[case] = (rec, meta["counts"], meta["extra"])
        os.remove(os.path.join(str(outdir), case + ".npz"))
    print("switch %s: %s" % (switch, info["seconds"]))
    if switch == "default":        # the control run is needed by every switch; the others are used once
        _RUNS[switch] = runs
    return runs


def _differences(ora, got):
    """one line per key that differs: for a field the count and the first index of the differing cells
    and the largest difference, so that a wrong tile column or z chunk can be read off the log"""
    bad = []
    if set(ora) != set(got):
        bad.append("keys differ: %s" % sorted(set(ora) ^ set(got)))
    for k in sorted(set(ora) & set(got)):
        a, b = np.asarray(ora[k]), np.asarray(got[k])
        if k.endswith("~"):
            if not (float(b) == pytest.approx(float(a), rel=S.RTOL_SUM)):
                bad.append("%s: oracle %r device %r (rel %g)" % (k, float(a), float(b), S.RTOL_SUM))
        elif a.shape != b.shape:
            bad.append("%s: shape %s against %s" % (k, a.shape, b.shape))
        elif not np.array_equal(a, b):
            if k.endswith("#"):
                bad.append("%s: differs (digest of an earlier step)" % k[:-1])
            elif a.ndim == 0:
                bad.append("%s: oracle %r device %r" % (k, a.item(), b.item()))
            else:
                ne = a != b
                idx = np.argwhere(ne)
                with np.errstate(invalid="ignore"):
                    worst = np.nanmax(np.abs(a[ne] - b[ne]))
                bad.append("%s: %d of %d cells differ, first at %s, last at %s (index order k, j, i), "
                           "largest difference %.3e; distinct i: %s" %
                           (k, idx.shape[0], a.size, tuple(idx[0].tolist()), tuple(idx[-1].tolist()), worst,
                            np.unique(idx[:, -1])[:12].tolist()))
    return bad


def _evidence(switch, case, ev, counts, control):
    bad = []
    for f in ev["on"]:
        if not counts[f] > 0:
            bad.append("%s == %d under the switch: the selected branch did not run" % (f, counts[f]))
        if control[f] != 0:
            bad.append("%s == %d in the control run: it does not tell the branches apart" % (f, control[f]))
    for f in ev["off"]:
        if counts[f] != 0:
            bad.append("%s == %d under the switch: the replaced branch still ran" % (f, counts[f]))
        if not control[f] > 0:
            bad.append("%s == %d in the control run: the default branch did not run there" % (f, control[f]))
    for f, (want, base) in ev["values"].items():
        if counts[f] != want:
            bad.append("%s == %d under the switch, expected %d" % (f, counts[f], want))
        if control[f] != base:
            bad.append("%s == %d in the control run, expected %d" % (f, control[f], base))
    return ["%s / %s: %s" % (switch, case, b) for b in bad]


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("switch", list(S.SWITCHES))
def test_switch_is_bit_identical_to_the_oracle_and_selects_its_kernels(switch, tmp_path_factory):
    runs = _child(switch, tmp_path_factory.mktemp("switch"))
    control = runs if switch == "default" else _child("default", tmp_path_factory.mktemp("control"))
    bad = []
    for case, ev in S.SWITCHES[switch]["cases"].items():
        rec, counts, extra = runs[case]
        print("%s / %s: %s" % (switch, case, {k: v for k, v in counts.items() if v}))
        bad += ["%s / %s: %s" % (switch, case, d) for d in _differences(_oracle(case), rec)]
        bad += _evidence(switch, case, ev, counts, control[case][1])
        if case == "selfmpi64":
            for axes, st in extra["selfmpi"].items():
                print("%s / selfmpi64 %s: %s" % (switch, axes, st))
                if not (st["messages"] > 100 and st["bytes"] > 8 * st["messages"]):
                    bad.append("%s / selfmpi64 %s: nothing went over the transport: %s" % (switch, axes, st))
                fast = "GFSHIP_NO_FUSED_MPI" not in S.SWITCHES[switch]["env"]
                if (st["fused_mpi"] >= 4) != fast:
                    bad.append("%s / selfmpi64 %s: fused_mpi == %d" % (switch, axes, st["fused_mpi"]))
                fast = "GFSHIP_NO_LATTICE_CYCLE" not in S.SWITCHES[switch]["env"]
                if (st["lattice_cycles"] >= 4) != fast or (not fast and st["lattice_cycles"]):
                    bad.append("%s / selfmpi64 %s: lattice_cycles == %d" % (switch, axes, st["lattice_cycles"]))
    assert not bad, "\n".join(bad)


@pytest.mark.timeout(1800)
def test_control_run_takes_the_default_branches(tmp_path_factory):
    """the empty environment really is the default path: the sweeps along z beside the one-component
    tiled kernel (tg64_tracer), four tiles along x and two z chunks (tg128), the 2 x 2 loops with
    fused prolongation and restriction (128^3)"""
    c = {case: r[1] for case, r in _child("default", tmp_path_factory.mktemp("control")).items()}
    for case in S.TG64 + ("tg128",):
        assert c[case]["PREDICT_SWEEP"] > 0 and c[case]["ADVECT3_SWEEP2"] > 0, (case, c[case])
        assert c[case]["PREDICT_TILED"] == 0 and c[case]["ADVECT3_TILED"] == 0, (case, c[case])
    assert c["tg64_tracer"]["ADVECT1_TILED_TRACER"] >= 3
    for case in S.VC128 + ("tg128",):
        assert c[case]["PROLONGATION_FUSED"] > 0 and c[case]["RESTRICTION_FUSED"] > 0, (case, c[case])
        assert c[case]["PATCH_LOOP_HOST_ARMS"] > 0 and c[case]["COARSE_CYCLES"] > 0, (case, c[case])


def test_three_domains_of_one_process_each_follow_their_own_environment(monkeypatch):
    """A domain looks its switches up when it is created, none is read once per process: three domains
    created one after another in this process -- empty environment, three of the switches that used to
    be read into a static, empty environment again -- each show the kernel families of their own
    environment, and each equal the oracle (Taylor-Green 64^3 with a mean flow, van Leer + GfsSource,
    two steps: 64^3 is the smallest size the sweeps along z and the pair kernels run at)"""
    case = S._case_tg(6, 1, -0.7, False, 2)
    oracle = case("oracle", None)
    default = ("PREDICT_SWEEP", "ADVECT3_SWEEP2", "RESIDUAL_PAIRS", "PROJECT_PAIRS")
    switched = ("PREDICT_TILED", "ADVECT3_TILED", "RESIDUAL_SCALAR", "PROJECT_SCALAR")
    for k in [k for k in os.environ if k.startswith("GFSHIP_") and k not in S.KEEP_IN_CHILD]:
        monkeypatch.delenv(k)
    bad = []
    for which, env in enumerate(({}, {"GFSHIP_NO_ADVECT_SWEEP": "1", "GFSHIP_RN_SCALAR": "1", "GFSHIP_PC_SCALAR": "1"}, {})):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        dev = S._Device()
        rec = case("device", dev)           # creates the domain: the environment counts from here on
        for k in env:
            monkeypatch.delenv(k)
        counts = S._counts(dev.domains)
        for gs in dev.sims:
            gs.destroy()
        for gd in dev.domains:
            gd.destroy()
        print("domain %d: %s" % (which + 1, {k: v for k, v in counts.items() if v}))
        on, off = (switched, default) if env else (default, switched)
        bad += ["domain %d: %s == %d, expected > 0" % (which + 1, f, counts[f]) for f in on if not counts[f] > 0]
        bad += ["domain %d: %s == %d, expected 0" % (which + 1, f, counts[f]) for f in off if counts[f] != 0]
        bad += ["domain %d: %s" % (which + 1, d) for d in _differences(oracle, rec)]
    assert not bad, "\n".join(bad)
