"""The value semantics of the table of environment switches (csrc/switches.hpp), without a GPU: the
header is plain C++, so a small program that prints read_switches () is built with the host compiler
and run under a handful of environments.  What is expected here was written from the reads the table
replaced (getenv (...) != nullptr, w && w[0] == '1', e ? atoi (e) : default, ...), not from the table."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "gerris-fft-particles_amd", "csrc")

DEFAULTS = dict(
    advect_sweep=1, mpi_sweep=1, advect_sweep1=0, advect3=1, fused_mpi=1, fused_divergence=1,
    fused_correction=1, lazy_un=1, project_pairs=1, residual_pairs=1, rn_blocks=0, coarse_threads=1024,
    rows2d=1, diffusion_pipelined=1, weighted_pipelined=1, lattice_cycle=1, fused_restriction=1,
    fused_prolongation=1, old_prolong_pack=0, arm_ahead=1, kernel_arming=0, xcd_scope=0, xcd_near_mode=2,
    xcd_place=0, wave_loop=0, skew_old=0, skew_lines=0, patch_min_n=128, patch_regs=0, skew_stats=0,
    tree_residual_tape=1, tree_template_relax=0, tree_pipeline=1, tree_flow=1, tree_prefetch=1,
    flow_width=0, tree_debug=0, patch=1)


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """-> function (environment) -> {member: value}"""
    header = open(os.path.join(CSRC, "switches.hpp")).read()
    struct = header[header.index("struct Switches {"):header.index("bool patch () const")]
    members = re.findall(r"^\s*(?:bool|int) (\w+) = ", struct, flags=re.M)
    assert sorted(members + ["patch"]) == sorted(DEFAULTS)
    tmp = tmp_path_factory.mktemp("switches")
    src, exe = str(tmp / "print_switches.cpp"), str(tmp / "print_switches")
    with open(src, "w") as f:
        f.write('#include "switches.hpp"\n#include <cstdio>\nint main ()\n{\n'
                "  const gfship::Switches d, s = gfship::read_switches ();\n" +
                "".join('  printf ("%s=%%d %%d\\n", (int) s.%s, (int) d.%s);\n' % (m, m, m) for m in members) +
                '  printf ("patch=%d %d\\n", (int) s.patch (), (int) d.patch ());\n  return 0;\n}\n')
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe],
                   check=True, capture_output=True, text=True, timeout=120)

    def run(env):
        out = subprocess.run([exe], env=env, check=True, capture_output=True, text=True, timeout=30).stdout
        got = {k: tuple(int(x) for x in v.split()) for k, v in (line.split("=") for line in out.splitlines())}
        # the default member initialisers are the values of the empty environment, whatever is set
        assert {k: v[1] for k, v in got.items()} == DEFAULTS
        return {k: v[0] for k, v in got.items()}
    return run


def _changed(got):
    return {k: v for k, v in got.items() if v != DEFAULTS[k]}


def test_empty_environment_gives_the_defaults(table):
    assert table({}) == DEFAULTS


@pytest.mark.parametrize("value", ["1", "0", ""])
def test_presence_switches_are_on_with_any_value(table, value):
    """getenv (...) != nullptr: GFSHIP_NO_ADVECT_SWEEP=0 still switches the sweep off"""
    assert _changed(table({"GFSHIP_NO_ADVECT_SWEEP": value})) == {"advect_sweep": 0}
    env = {"GFSHIP_" + k: value for k in (
        "NO_MPI_SWEEP", "ADVECT_SWEEP1", "NO_ADVECT3", "NO_FUSED_MPI", "NO_FUSED_DIVERGENCE", "NO_FUSED_CORRECTION",
        "NO_LAZY_UN", "PC_SCALAR", "RN_SCALAR", "NO_ROWS2D", "DIFFUSION_HYPERPLANES", "WEIGHTED_HYPERPLANES",
        "NO_LATTICE_CYCLE", "NO_FUSED_RESTRICTION", "NO_FUSED_PROLONGATION", "OLD_PROLONG_PACK", "NO_ARM_AHEAD",
        "KERNEL_ARMING", "PATCH_REGS", "SKEW_STATS", "TREE_DEBUG")}
    assert _changed(table(env)) == dict(
        mpi_sweep=0, advect_sweep1=1, advect3=0, fused_mpi=0, fused_divergence=0, fused_correction=0, lazy_un=0,
        project_pairs=0, residual_pairs=0, rows2d=0, diffusion_pipelined=0, weighted_pipelined=0, lattice_cycle=0,
        fused_restriction=0, fused_prolongation=0, old_prolong_pack=1, arm_ahead=0, kernel_arming=1, patch_regs=1,
        skew_stats=1, tree_debug=1)


def test_xcd_place_and_wave_loop_need_a_leading_1(table):
    assert _changed(table({"GFSHIP_XCD_PLACE": "0", "GFSHIP_WAVE_LOOP": "yes"})) == {}
    assert _changed(table({"GFSHIP_XCD_PLACE": "1", "GFSHIP_WAVE_LOOP": "1x"})) == dict(xcd_place=1, wave_loop=1)


def test_tree_switches_go_through_atoi(table):
    assert _changed(table({"GFSHIP_TREE_NO_FLOW": "0"})) == {}
    env = {"GFSHIP_TREE_" + k: "0" for k in ("NO_RESIDUAL_TAPE", "TEMPLATE_RELAX", "NO_PIPELINE", "NO_PREFETCH")}
    assert _changed(table(env)) == {}
    env = {"GFSHIP_TREE_" + k: "1" for k in ("NO_FLOW", "NO_RESIDUAL_TAPE", "TEMPLATE_RELAX", "NO_PIPELINE", "NO_PREFETCH")}
    assert _changed(table(env)) == dict(tree_flow=0, tree_residual_tape=0, tree_template_relax=1, tree_pipeline=0,
                                        tree_prefetch=0)
    assert _changed(table({"GFSHIP_TREE_NO_FLOW": "yes"})) == {}       # atoi ("yes") == 0


def test_xcd_scope_leaves_the_near_mode_at_2(table):
    assert _changed(table({"GFSHIP_XCD_SCOPE": "1"})) == dict(xcd_scope=1)
    assert _changed(table({"GFSHIP_XCD_SCOPE": "1", "GFSHIP_XCD_NEAR_MODE": "0"})) == dict(xcd_scope=1, xcd_near_mode=0)
    assert _changed(table({"GFSHIP_XCD_NEAR_MODE": "-1"})) == dict(xcd_near_mode=-1)


def test_patch_is_derived_from_skew_lines_and_skew_old(table):
    assert _changed(table({"GFSHIP_SKEW_OLD": "1"})) == dict(skew_old=1, patch=0)
    assert _changed(table({"GFSHIP_SKEW_LINES": "1"})) == dict(skew_lines=1, patch=0)


def test_integer_switches(table):
    """the values as written: the clamps of GFSHIP_RN_BLOCKS and GFSHIP_COARSE_THREADS are where they are used"""
    env = {"GFSHIP_PATCH_MIN_N": "64", "GFSHIP_RN_BLOCKS": "8192", "GFSHIP_COARSE_THREADS": "256",
           "GFSHIP_FLOW_WIDTH": "200"}
    assert _changed(table(env)) == dict(patch_min_n=64, rn_blocks=8192, coarse_threads=256, flow_width=192)
    env = {"GFSHIP_PATCH_MIN_N": "x", "GFSHIP_RN_BLOCKS": "7", "GFSHIP_COARSE_THREADS": "100", "GFSHIP_FLOW_WIDTH": "0"}
    assert _changed(table(env)) == dict(patch_min_n=0, rn_blocks=7, coarse_threads=100, flow_width=64)
    # a width below 64 (or none that atoi can read) was 64 operations per level, above 512 the use site clamps
    assert _changed(table({"GFSHIP_FLOW_WIDTH": "4096"})) == dict(flow_width=4096)
