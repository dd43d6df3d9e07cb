"""The direct extended-precision reference of the FFT outputs (tests/dft_reference.py): its transform
against closed forms, the reference's binning against values derived by hand from its loops, and the
numpy restatement oracle/go_spectra.py against it.

Closed forms of the binning (modules/fft.c:1405-1466), with v = A f/ntot transformed without
normalisation, so that a cosine of amplitude A has the two coefficients A/2 and a checkerboard
A (-1)^i the single coefficient A at the Nyquist index N/2:

3-D, F[i][j][k <= N/2], weight 1/2 for k = 0 and 1 for k = 1 .. N/2 (:1437-1444):
  * A (-1)^iz:  F[0][0][N/2] = A, k = N/2 has weight 1          -> Ek[(N/2)^2] = A^2
  * A (-1)^ix:  F[N/2][0][0] = A, k = 0 has weight 1/2           -> Ek[(N/2)^2] = A^2/2   (same for iy)
  only the last dimension is halved, and its Nyquist plane counts fully.
2-D, F[i][j <= N/2], the j = 0 column added with 1/2 (:1420-1422) and again with 1 (:1424-1428):
  * A cos (2 pi m x): F[m][0] = F[N - m][0] = A/2, each (1/2 + 1) A^2/4 -> Ek[m^2] = 3 A^2/4
  * A cos (2 pi m y): F[0][m] = A/2 only (F[0][N - m] is not stored): as the j = 0 column of i = 0 it
    adds 1/2 |F[0][0]|^2 = 0, then |F[0][m]|^2                           -> Ek[m^2] = A^2/4
These tell the axes apart without any oracle."""
import numpy as np
import pytest

import dft_reference as R
from dft_reference import (LD, EPS, checkerboard, cosine, checkerboard_bin_3d, cosine_bin_2d, random_field,
                           plane_field, assert_rows_match, assert_bins_match)

# direct_dft against closed forms: every twiddle is within about one eps, a coefficient is a product of
# up to three of them, and the closed forms are themselves evaluated with cos / sin of 2 pi times a
# rounded fraction (a few eps at angles up to 2 pi)
TOL_EXACT = 16 * EPS


def test_longdouble_is_extended():
    assert EPS < 2e-19


# ---- direct_dft against closed forms -------------------------------------------------------------

@pytest.mark.parametrize("shape", [(16,), (8, 12), (4, 6, 10), (2, 2, 2)])
def test_direct_dft_of_a_constant_and_of_a_delta(shape):
    ntot = int(np.prod(shape))
    F = R.direct_dft(np.full(shape, LD(3)) / LD(ntot))
    want = np.zeros(shape, dtype=R.CLD)
    want[(0,) * len(shape)] = 3
    assert np.abs(F - want).max() <= TOL_EXACT
    d = np.zeros(shape)
    at = tuple(s - 1 for s in shape)
    d[at] = 1.
    F = R.direct_dft(d)
    k = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    # exp (-2 pi i sum_a k_a (s_a - 1)/s_a) = exp (+2 pi i sum_a k_a/s_a)
    # (reduced to [0, 1) in integers, so that the closed form carries no argument-reduction error)
    ph = (sum(ka * (ntot // s) for ka, s in zip(k, shape)) % ntot).astype(LD) / LD(ntot)
    want = np.cos(2 * R._PI * ph) + 1j * np.sin(2 * R._PI * ph)
    assert np.abs(F - want).max() <= TOL_EXACT


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("n,m", [(8, 1), (16, 3), (16, 7)])
def test_direct_dft_of_single_modes_per_axis(axis, n, m):
    """cos -> n^3/2 at +-m, sin -> -+ i n^3/2: on the axis of the mode only"""
    j = np.arange(n).astype(LD)
    sh = [1, 1, 1]
    sh[axis] = n
    ph = (2 * R._PI * m * j / n).reshape(sh)
    for f, cp, cm in ((np.cos, 0.5, 0.5), (np.sin, -0.5j, 0.5j)):
        a = np.broadcast_to(f(ph), (n, n, n)) / LD(n ** 3)
        F = R.direct_dft(a)
        want = np.zeros((n, n, n), dtype=R.CLD)
        ip, im = [0, 0, 0], [0, 0, 0]
        ip[axis], im[axis] = m, n - m
        want[tuple(ip)] = cp
        want[tuple(im)] = cm
        assert np.abs(F - want).max() <= TOL_EXACT


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("n", [2, 4, 16])
def test_direct_dft_of_a_checkerboard_on_one_axis(axis, n):
    sh = [1, 1, 1]
    sh[axis] = n
    a = np.broadcast_to(((-1.) ** np.arange(n)).reshape(sh), (n, n, n)) / LD(n ** 3)
    F = R.direct_dft(a)
    want = np.zeros((n, n, n), dtype=R.CLD)
    at = [0, 0, 0]
    at[axis] = n // 2
    want[tuple(at)] = 1
    assert np.abs(F - want).max() <= TOL_EXACT


# ---- the reference's binning: closed forms that tell the axes apart ------------------------------

@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("n", [2, 4, 16])
def test_bins_of_a_checkerboard_3d_tell_z_from_x_and_y(axis, n):
    A = 1.5
    zero = np.zeros((n,) * 3)
    Ek, Etot, _ = R.energy_bins([checkerboard(n, 3, axis, A), zero, zero])
    assert len(Ek) == 4 * (n // 2 + 1) ** 2
    want = np.zeros(len(Ek))
    want[(n // 2) ** 2] = checkerboard_bin_3d(axis, A)
    assert np.abs(Ek - want).max() <= 1e-17
    assert abs(Etot - want.sum()) <= 1e-17


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("n,m", [(4, 1), (16, 3), (64, 5)])
def test_bins_of_a_cosine_2d_tell_x_from_y(axis, n, m):
    A = 0.8
    Ek, Etot, deltak = R.energy_bins([cosine(n, 2, axis, m, A, extended=True), np.zeros((n, n))])
    assert len(Ek) == 3 * (n // 2 + 1) ** 2
    want = np.zeros(len(Ek))
    want[m * m] = cosine_bin_2d(axis, A)
    assert np.abs(Ek - LD(A) ** 2 * (want / (A * A)).astype(LD)).max() <= 1e-17
    assert abs(float(deltak) - 2. * np.pi / (1. - 1. / n)) <= 1e-14 * float(deltak)


def test_rows_of_a_plane_are_the_full_signed_transform():
    """sin (2 pi x) cos (2 pi 2 y) (1 + z) on the plane z = const: four modes (+-1, +-2, 0) of size
    (1 + z_cell)/4, at the rows write_spectra's loops give them (outer x, inner y, both signed)"""
    n = 8
    c = -0.5 + (np.arange(n) + 0.5) / n
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    v = np.sin(2. * np.pi * x) * np.cos(2. * np.pi * 2. * y) * (1. + z)
    rows = R.spectra_rows_plane(v, 2, c[5])
    assert rows.shape == (n * n, 5)
    ks = 2. * np.pi / (1. - 1. / n)
    amp = np.hypot(rows[:, 3], rows[:, 4]).astype(float)
    big = np.nonzero(amp > 1e-10)[0]
    assert list(big) == [1 * n + 2, 1 * n + 6, 7 * n + 2, 7 * n + 6]
    assert np.allclose(amp[big], (1. + c[5]) / 4., rtol=1e-14)
    k = rows[big, :3].astype(float)
    assert np.allclose(k, ks * np.array([[1, 2, 0], [1, -2, 0], [-1, 2, 0], [-1, -2, 0]]), rtol=1e-14)
    # the same field seen from an x-normal plane: in-plane (y, z), no sine left, z-dependence = all kz
    rows = R.spectra_rows_plane(v, 0, c[6])
    k = rows[:, :3].astype(float)
    assert np.all(k[:, 0] == 0.) and np.isclose(k[n + 2, 1], ks) and np.isclose(k[n + 2, 2], 2 * ks)
    assert np.isclose(k[n + 7, 2], -ks)


@pytest.mark.parametrize("pos,kc", [(-0.5, 0), (0., 4), (np.nextafter(0.5, 0.), 7), (0.125, 5),
                                    (np.nextafter(0.125, 0.), 4), (0.5, None), (-0.5000001, None)])
def test_locate(pos, kc):
    assert R.locate(pos, 8) == kc


# ---- oracle/go_spectra.py against the direct reference -------------------------------------------

@pytest.mark.parametrize("dim,level", [(2, l) for l in range(1, 7)] + [(3, l) for l in range(1, 6)])
def test_oracle_energy_spectra_against_the_direct_reference(dim, level):
    from oracle.go_spectra import energy_spectra
    n = 1 << level
    comps = [random_field(n, dim, 10 * level + c, mean=0.3 - 0.5 * c) for c in range(dim)]
    assert_bins_match(energy_spectra(comps), R.energy_bins(comps))


@pytest.mark.parametrize("level", [1, 2, 4, 5])
def test_oracle_output_spectra_against_the_direct_reference(level):
    from oracle.go_spectra import output_spectra
    n = 1 << level
    v = random_field(n, 3, 77 + level, mean=1.7)
    F, ks = output_spectra(v)
    assert_rows_match(R.rows_of_box_output(F, ks), R.spectra_rows_box(v))


@pytest.mark.parametrize("normal", [0, 1, 2])
@pytest.mark.parametrize("level,pos", [(5, 0.1), (5, -0.3), (4, -0.5 + 2.5 / 16), (4, 0.25), (3, -0.5),
                                       (1, 0.)])
def test_oracle_output_spectra_plane_against_the_direct_reference(normal, level, pos):
    """the full N x N transform in write_spectra's order (fails on the half-spectrum N x (N/2 + 1))"""
    from oracle.go_spectra import output_spectra_plane
    n = 1 << level
    v = plane_field(n, 5 + level)
    F, ks = output_spectra_plane(v, normal, pos)
    assert F.shape == (n, n)
    assert_rows_match(R.rows_of_plane_output(F, ks, normal), R.spectra_rows_plane(v, normal, pos))


def test_oracle_plane_positions_outside_the_box_are_refused():
    from oracle.go_spectra import output_spectra_plane
    v = plane_field(8, 1)
    pos = np.nextafter(0.5, 0.)              # inside the last cell, though pos + 0.5 rounds to 1
    F, ks = output_spectra_plane(v, 2, pos)
    assert_rows_match(R.rows_of_plane_output(F, ks, 2), R.spectra_rows_plane(v, 2, pos))
    for pos in (0.5, 0.7, -0.50001):
        with pytest.raises(ValueError):
            output_spectra_plane(v, 2, pos)


@pytest.mark.parametrize("dim,b,level", [(3, 2, 2), (3, 2, 3), (2, 2, 4)])
def test_oracle_lattice_form_against_the_direct_reference(dim, b, level):
    """n_box: a cubic lattice of b^dim boxes of 2^level cells per side (the levels below a box do not
    exist, the cell size and the k step are those of a unit box)"""
    from oracle.go_spectra import energy_spectra, output_spectra
    nb = 1 << level
    n = b * nb
    comps = [random_field(n, dim, 31 * level + c, mean=0.2 + c) for c in range(dim)]
    assert_bins_match(energy_spectra(comps, n_box=nb), R.energy_bins(comps, n_box=nb))
    if dim == 3:
        F, ks = output_spectra(comps[0], n_box=nb)
        assert_rows_match(R.rows_of_box_output(F, ks), R.spectra_rows_box(comps[0], n_box=nb))
