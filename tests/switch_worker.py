"""Worker of tests/test_gpu_switches.py: one setting of the GFSHIP_* switches in a process of its own
(a domain looks them up when it is created; here they are in the environment from the start).  Runs the device half of every case tests/switch_cases.py lists for the switch,
writes OUTDIR/<case>.npz (fields, scalars) and OUTDIR/<case>.json (the tallies of
gfship_domain_kernel_counts and what else the case reports) and prints one JSON line.  It computes
no oracle and asserts nothing about bits: the parent does.

  python tests/switch_worker.py --list
  python tests/switch_worker.py SWITCH_NAME OUTDIR
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gerris-fft-particles_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def main(argv):
    if len(argv) == 2 and argv[1] == "--list":
        import switch_cases as S          # loads the oracle's module, never the device library
        for name, sw in S.SWITCHES.items():
            env = " ".join("%s=%s" % kv for kv in sorted(sw["env"].items())) or "(empty environment)"
            print("%-40s %s" % (name, env))
            for case, ev in sw["cases"].items():
                what = ["%s > 0" % f for f in ev["on"]] + ["%s == 0" % f for f in ev["off"]] + \
                    ["%s == %d" % (f, v[0]) for f, v in ev["values"].items()]
                print("    %-22s %s" % (case, ", ".join(what)))
        print("SWITCHES " + json.dumps({n: sw["env"] for n, sw in S.SWITCHES.items()}, sort_keys=True))
        return 0
    if len(argv) != 3:
        sys.stderr.write(__doc__)
        return 2
    name, outdir = argv[1], argv[2]
    import switch_cases as S
    for k in [k for k in os.environ if k.startswith("GFSHIP_") and k not in S.KEEP_IN_CHILD]:
        del os.environ[k]
    if name not in S.SWITCHES:
        sys.stderr.write("unknown switch %r\n" % name)
        return 2
    sw = S.SWITCHES[name]
    os.environ.update(sw["env"])          # before the library is loaded
    import numpy as np
    import gfship
    gfship.lib()
    os.makedirs(outdir, exist_ok=True)
    done = {}
    for case in sw["cases"]:
        t0 = time.time()
        rec, counts, extra = S.run_case(case, "device")
        np.savez(os.path.join(outdir, case + ".npz"), **{k: np.asarray(v) for k, v in rec.items()})
        with open(os.path.join(outdir, case + ".json"), "w") as f:
            json.dump(dict(counts=counts, extra=extra, env=sw["env"]), f)
        done[case] = round(time.time() - t0, 2)
        sys.stderr.write("switch_worker: %s %s %.1f s\n" % (name, case, done[case]))
    print("SWITCHWORKER " + json.dumps(dict(switch=name, env=sw["env"], seconds=done), sort_keys=True))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
