"""GfsDropletToParticle and GfsRemoveDroplets without a device: the messages of the front end for a bad list, a bad
variable, bad keywords and a refined tree, in the style of tests/test_gfs_frontend_errors_cpu.py (through
`--check'), and the new entry points in libgfship.so."""
import ctypes
import os
import subprocess

import pytest

from test_gfs_frontend_errors_cpu import BIN, PLIST, S, TRACERS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOT_ON_DEVICE = "which is not kept on the device"

ROWS = [
    ("d2p_ok", 2, S(PLIST + "  VariableTracer T\n  DropletToParticle { istep = 1 } drops T { min = 5 reset = 0.5 density = 2 } T - 0.5*P\n"),
     0, ["event DropletToParticle line 7"]),
    ("d2p_defaults", 2, S(PLIST + "  VariableTracer T\n  DropletToParticle { istep = 1 } drops T\n"), 0,
     ["event DropletToParticle line 7"]),
    ("d2p_no_list", 2, S(PLIST + "  VariableTracer T\n  DropletToParticle { istep = 1 }\n"), 1,
     [":7: expecting a string (object name)"]),
    ("d2p_unknown_list", 2, S(PLIST + "  VariableTracer T\n  DropletToParticle { istep = 1 } drips T\n"), 1,
     [":7: unknown object 'drips'"]),
    ("d2p_not_a_list", 2, S(PLIST + "  VariableTracer T\n  DropletToParticle { istep = 1 } T T\n"), 1,
     [":7: object 'T' is not a GfsParticleList"]),
    ("d2p_tracers", 2, S(TRACERS + "  VariableTracer T\n  DropletToParticle { istep = 1 } dust T\n"), 1,
     [":7: the list `dust' holds GfsParticle objects: GfsDropletToParticle needs GfsParticulate objects"]),
    ("d2p_no_variable", 2, S(PLIST + "  DropletToParticle { istep = 1 } drops\n"), 1,
     [":6: expecting a string (variable)"]),
    ("d2p_unknown_variable", 2, S(PLIST + "  DropletToParticle { istep = 1 } drops C\n"), 1,
     [":6: unknown variable `C'"]),
    ("d2p_host_variable", 2, S(PLIST + "  Init {} { C = x }\n  DropletToParticle { istep = 1 } drops C\n"), 1,
     [":7: GfsDropletToParticle works on `C', " + NOT_ON_DEVICE]),
    ("d2p_keyword", 2, S(PLIST + "  VariableTracer T\n  DropletToParticle { istep = 1 } drops T {\n    max = 3 }\n"), 1,
     ["simulation file:8: unknown identifier `max'"]),
    ("d2p_min", 2, S(PLIST + "  VariableTracer T\n  DropletToParticle { istep = 1 } drops T { min = 2.5 }\n"), 1,
     ["simulation file:7: expecting an integer (min)"]),
    ("d2p_reset", 2, S(PLIST + "  VariableTracer T\n  DropletToParticle { istep = 1 } drops T { reset = T }\n"), 1,
     ["simulation file:7: expecting a number (reset)"]),
    ("d2p_equal", 2, S(PLIST + "  VariableTracer T\n  DropletToParticle { istep = 1 } drops T { min 3 }\n"), 1,
     ["simulation file:7: expecting `='"]),
    ("d2p_function_host_variable", 2,
     S(PLIST + "  VariableTracer T\n  Init {} { C = x }\n  DropletToParticle { istep = 1 } drops T { min = 3 } T - C\n"), 1,
     [":8: the function of GfsDropletToParticle reads `C', " + NOT_ON_DEVICE]),
    ("remove_ok", 2, S("  VariableTracer T\n  VariableTracer S\n  RemoveDroplets { istep = 1 } T -2 S 0.25\n"), 0,
     ["event RemoveDroplets line 4"]),
    ("remove_no_variable", 2, S("  RemoveDroplets { istep = 1 }\n"), 1, [":2: expecting a string (variable)"]),
    ("remove_unknown_variable", 2, S("  RemoveDroplets { istep = 1 } C 3\n"), 1, [":2: unknown variable `C'"]),
    ("remove_no_min", 2, S("  VariableTracer T\n  RemoveDroplets { istep = 1 } T\n"), 1, [":3: expecting an integer (min)"]),
    ("remove_min", 2, S("  VariableTracer T\n  RemoveDroplets { istep = 1 } T 2.5\n"), 1, [":3: expecting an integer (min)"]),
    ("remove_function", 2, S("  VariableTracer T\n  RemoveDroplets { istep = 1 } T 3 Q\n"), 1,
     [":3: the function of GfsRemoveDroplets is the name of a variable here: `Q' is none"]),
    ("remove_constant_function", 2, S("  VariableTracer T\n  RemoveDroplets { istep = 1 } T 3 0.5\n"), 1,
     [":3: the function of GfsRemoveDroplets is the name of a variable here: the constant `0.5' is not supported"]),
    ("remove_trailing", 2, S("  VariableTracer T\n  RemoveDroplets { istep = 1 } T 3 T 1 2\n"), 1,
     [":3: unexpected text after RemoveDroplets"]),
    # neither class runs on a refined tree
    ("remove_tree", 2, S("  Refine (x > 0 ? 4 : 3)\n  VariableTracer T\n  RemoveDroplets { istep = 1 } T 5\n"), 1,
     ["gfship: line 4: GfsRemoveDroplets is not supported on a refined tree"]),
    ("d2p_tree", 2, S("  Refine (x > 0 ? 4 : 3)\n" + PLIST + "  VariableTracer T\n  DropletToParticle { istep = 1 } drops T\n"), 1,
     ["gfship: line 8: GfsDropletToParticle is not supported on a refined tree"]),
]


@pytest.mark.parametrize("name,dim,text,status,fragments", ROWS, ids=[r[0] for r in ROWS])
def test_droplet_objects_of_a_file(tmp_path, name, dim, text, status, fragments):
    bad = tmp_path / "bad.gfs"
    bad.write_text(text)
    r = subprocess.run([os.path.join(BIN, "gfship%dD" % dim), "--check", str(bad)], capture_output=True, text=True,
                       timeout=60)
    print(r.stdout, r.stderr)
    assert r.returncode == status, r.stderr
    for f in fragments:
        assert f in (r.stderr if status else r.stdout), (r.stdout, r.stderr)
    if status:
        assert r.stderr.startswith("gfship: ") and r.stderr.count("\n") == 1, r.stderr


def test_the_library_exports_the_new_entry_points():
    lib = ctypes.CDLL(os.path.join(ROOT, "gerris-fft-particles_amd", "lib", "libgfship.so"))
    for name in ("gfship_tag_droplets", "gfship_remove_droplets", "gfship_droplet_to_particle_create",
                 "gfship_droplet_to_particle_event", "gfship_droplet_to_particle_destroy", "gfship_tag_droplets_time"):
        assert getattr(lib, name) is not None
    header = open(os.path.join(ROOT, "include", "gfship.h")).read()
    for name in ("gfship_tag_droplets", "gfship_remove_droplets", "gfship_droplet_to_particle_create",
                 "gfship_droplet_to_particle_event", "gfship_droplet_to_particle_destroy"):
        assert name + " (" in header
