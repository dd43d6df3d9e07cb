"""The FFT outputs of the device (csrc/spectra.hip: GfsOutputEnergySpectra, GfsOutputSpectra of the box
and of a plane) against tests/dft_reference.py ONLY: a direct extended-precision DFT read with the
index expressions of the reference's modules/fft.c.  Nothing here goes through oracle/go_spectra.py or
an FFT library, so a reading of the reference shared by the kernels and their restatement does not pass.

Bounds (the project's own, tests/test_gpu_spectra.py): 1e-13 max abs on coefficients, 1e-12 Etot per bin
and on Etot.  The reference transform itself is exact to ~1e-19.

Largest device-minus-direct error seen on an MI355X, per entry point (see the figures each case prints):
  gfship_energy_spectra         bins 2.1e-16 Etot (2-D, N = 4), Etot 3.3e-15 Etot (256^2)   bound 1e-12 Etot
  gfship_output_spectra         coefficients 2.4e-16 (64^3)                                 bound 1e-13
  gfship_output_spectra_plane   coefficients 9.1e-17 (y-normal, N = 32, pos = -0.5)         bound 1e-13
  2 x 2 x 2 lattice of 16^3     coefficients 3.1e-17, bins 2.5e-17 Etot                     same bounds
None comes within a factor 10 of its bound (the closest, Etot at 256^2, is 300 times inside).
"""
import numpy as np
import pytest

import gfship
import dft_reference as R
from dft_reference import (checkerboard, cosine, checkerboard_bin_3d, cosine_bin_2d, random_field, plane_field,
                           assert_rows_match, assert_bins_match, TOL_BINS)

pytestmark = pytest.mark.gpu

PERIODIC = [gfship.SIDE_PERIODIC] * 6


def _upload(gd, a):
    f = gd.variable()
    f.upload(np.pad(a, 1, mode="wrap"))
    return f


def _energy(gd, comps):
    return gd.energy_spectra([_upload(gd, a) for a in comps])


# ---- GfsOutputEnergySpectra ----------------------------------------------------------------------

@pytest.mark.parametrize("dim,level", [(2, 1), (2, 2), (2, 3), (2, 6), (2, 8), (3, 1), (3, 2), (3, 3), (3, 5), (3, 6)])
def test_energy_spectra_of_random_fields(dim, level):
    """from N = 2 (where N/2 + 1 = N and one 256-thread block is mostly tail) to 256^2 and 64^3; every
    component has its own non-zero mean"""
    n = 1 << level
    comps = [random_field(n, dim, 1000 * dim + 10 * level + c, mean=0.3 - 0.5 * c) for c in range(dim)]
    gd = gfship.Domain(dim, level, PERIODIC)
    assert_bins_match(_energy(gd, comps), R.energy_bins(comps), label="energy_spectra %dD N=%d" % (dim, n))
    gd.destroy()


def test_energy_spectra_of_one_cell_is_refused():
    gd = gfship.Domain(3, 0, PERIODIC)
    f = gd.variable()
    with pytest.raises(gfship.GfshipError):
        gd.energy_spectra([f, f, f])
    gd.destroy()


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("level", [1, 2, 4])
def test_energy_spectra_checkerboard_3d_tells_z_from_x_and_y(axis, level):
    """A (-1)^i along z gives Ek[(N/2)^2] = A^2, along x or y A^2/2 (derivation: the docstring of
    tests/test_dft_reference_cpu.py): only the last dimension is halved, its Nyquist plane has weight 1"""
    n, A = 1 << level, 1.5
    comps = [checkerboard(n, 3, axis, A), np.zeros((n,) * 3), np.full((n,) * 3, 0.25)]
    gd = gfship.Domain(3, level, PERIODIC)
    got = _energy(gd, comps)
    assert_bins_match(got, R.energy_bins(comps), label="checkerboard 3D axis %d N=%d" % (axis, n))
    k, Ek, Etot = got
    want = checkerboard_bin_3d(axis, A)
    assert abs(Ek[(n // 2) ** 2 - 1] - want) <= TOL_BINS * want
    assert abs(Etot - want) <= TOL_BINS * want
    gd.destroy()


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("level,m", [(2, 1), (4, 3), (6, 5)])
def test_energy_spectra_cosine_2d_tells_x_from_y(axis, level, m):
    """A cos (2 pi m x) gives Ek[m^2] = 3 A^2/4, A cos (2 pi m y) gives A^2/4: the j = 0 column of the
    halved y direction is counted with 1/2 and again with 1"""
    n, A = 1 << level, 0.8
    comps = [cosine(n, 2, axis, m, A), np.zeros((n, n))]
    gd = gfship.Domain(2, level, PERIODIC)
    got = _energy(gd, comps)
    assert_bins_match(got, R.energy_bins(comps), label="cosine 2D axis %d N=%d" % (axis, n))
    k, Ek, Etot = got
    want = cosine_bin_2d(axis, A)
    # the cosines are rounded to double: (eps/2) A per point, at most 2 (eps/2)/A relative on A^2
    assert abs(Ek[m * m - 1] - want) <= TOL_BINS * want
    assert abs(Etot - want) <= TOL_BINS * want
    gd.destroy()


@pytest.mark.parametrize("dim,level", [(2, 1), (2, 5), (3, 1), (3, 2), (3, 4)])
def test_energy_spectra_with_energy_on_the_nyquist_planes_only(dim, level):
    """every combination of (-1)^i over the axes, each with its own amplitude: all the energy sits at
    indices 0 or N/2, where knx = np - i, the weight of k = N/2 and the last bins meet"""
    n = 1 << level
    comps = []
    for c in range(dim):
        a = np.zeros((n,) * dim)
        for mask in range(1, 1 << dim):
            b = np.full((n,) * dim, 0.1 * mask + 0.37 * c + 0.2)
            for axis in range(dim):
                if mask >> axis & 1:
                    b = b * checkerboard(n, dim, axis, 1.)
            a += b
        comps.append(a)
    gd = gfship.Domain(dim, level, PERIODIC)
    got = _energy(gd, comps)
    want = R.energy_bins(comps)
    assert_bins_match(got, want, label="nyquist %dD N=%d" % (dim, n))
    h2 = (n // 2) ** 2
    on = [m * h2 for m in range(1, dim + 1)]
    assert float(sum(want[0][q] for q in on)) >= (1. - 1e-15) * float(want[1])
    assert sum(got[1][q - 1] for q in on) >= (1. - TOL_BINS) * got[2]
    gd.destroy()


# ---- GfsOutputSpectra of the box -----------------------------------------------------------------

@pytest.mark.parametrize("level", [1, 2, 4, 6])
def test_output_spectra_rows_of_the_box(level):
    """all N*N*(N/2 + 1) rows in write_spectra's order, the k columns included"""
    n = 1 << level
    v = random_field(n, 3, 77 + level, mean=1.7)
    gd = gfship.Domain(3, level, PERIODIC)
    F, ks = gd.output_spectra(_upload(gd, v))
    want = R.spectra_rows_box(v)
    assert len(want) == n * n * (n // 2 + 1)
    assert_rows_match(R.rows_of_box_output(F, ks), want, label="output_spectra N=%d" % n)
    gd.destroy()


# ---- GfsOutputSpectra of a plane -----------------------------------------------------------------

def _plane_positions(n):
    c = -0.5 + (np.arange(n) + 0.5) / n
    return [("centre", c[(3 * n) // 4 - 1]),         # the only case the reference itself defines
            ("centre0", c[0]),
            ("face", -0.5 + (n // 2) / n),           # exactly on a face: the upper cell
            ("low", -0.5),
            ("inside", 0.1),
            ("top", np.nextafter(0.5, 0.))]          # in the last cell; pos + 0.5 rounds to 1


@pytest.mark.parametrize("normal", [0, 1, 2])
@pytest.mark.parametrize("level", [1, 2, 5])
def test_output_spectra_rows_of_a_plane(normal, level):
    """the full N x N transform: N*N rows, outer loop the first in-plane coordinate, inner the second,
    both with signed k, 0 along the normal.  (x- and y-normal planes: extension, parity undefined by
    the reference, compared with the coherent analogue of the z-normal case.)"""
    n = 1 << level
    v = plane_field(n, 5 + level)
    gd = gfship.Domain(3, level, PERIODIC)
    f = _upload(gd, v)
    for name, pos in _plane_positions(n):
        F, ks = gd.output_spectra_plane(f, normal, pos)
        assert F.shape == (n, n)
        want = R.spectra_rows_plane(v, normal, pos)
        assert len(want) == n * n and np.all(want[:, normal] == 0.)
        assert_rows_match(R.rows_of_plane_output(F, ks, normal), want,
                          label="output_spectra_plane normal %d N=%d %s" % (normal, n, name))
    gd.destroy()


@pytest.mark.parametrize("normal", [0, 1, 2])
@pytest.mark.parametrize("pos", [0.5, np.nextafter(0.5, 1.), 0.75, np.nextafter(-0.5, -1.), -3., float("nan")])
def test_output_spectra_of_a_plane_outside_the_box_is_refused(normal, pos):
    """a plane at 0.5 or beyond, or below -0.5, is an error: no cell of the level is read"""
    gd = gfship.Domain(3, 3, PERIODIC)
    f = _upload(gd, plane_field(8, 1))
    with pytest.raises(gfship.GfshipError):
        gd.output_spectra_plane(f, normal, pos)
    gd.destroy()


# ---- one call does not leak into the next --------------------------------------------------------

def test_results_do_not_depend_on_the_calls_before():
    """two calls in a row on one domain with different fields, and energy spectra followed by a plane
    and by the box: work buffers and plans are made per call today; a cache must keep this true"""
    level, n = 4, 16
    gd = gfship.Domain(3, level, PERIODIC)
    A = [random_field(n, 3, 300 + c, mean=0.5 * c) for c in range(3)]
    B = [plane_field(n, 400 + c) for c in range(3)]
    fa, fb = [_upload(gd, a) for a in A], [_upload(gd, b) for b in B]
    wa, wb = R.energy_bins(A), R.energy_bins(B)
    assert_bins_match(gd.energy_spectra(fa), wa, label="sequence energy A")
    assert_bins_match(gd.energy_spectra(fb), wb, label="sequence energy B")
    F, ks = gd.output_spectra_plane(fa[1], 1, 0.26)
    assert_rows_match(R.rows_of_plane_output(F, ks, 1), R.spectra_rows_plane(A[1], 1, 0.26), label="sequence plane A")
    F, ks = gd.output_spectra(fb[2])
    assert_rows_match(R.rows_of_box_output(F, ks), R.spectra_rows_box(B[2]), label="sequence box B")
    F, ks = gd.output_spectra_plane(fb[0], 2, -0.4)
    assert_rows_match(R.rows_of_plane_output(F, ks, 2), R.spectra_rows_plane(B[0], 2, -0.4), label="sequence plane B")
    F, ks = gd.output_spectra(fa[0])
    assert_rows_match(R.rows_of_box_output(F, ks), R.spectra_rows_box(A[0]), label="sequence box A")
    assert_bins_match(gd.energy_spectra(fa), wa, label="sequence energy A again")
    gd.destroy()
