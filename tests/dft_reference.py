"""A direct, extended-precision reference for the FFT outputs (GfsOutputSpectra, GfsOutputEnergySpectra),
independent of oracle/go_spectra.py and of any FFT library.

`direct_dft` is the discrete Fourier transform by its definition, over every index of every axis, in
numpy.clongdouble.  The functions below it are written from the text of the reference's modules/fft.c,
line by line and with its own index expressions; the line numbers in the comments are those of that
file.  They read the FULL transform: which part of it the reference prints, and in which order, follows
from its loops alone, not from a half-spectrum convention of some library.

Arrays of cell values are indexed [k][j][i] (3-D) or [j][i] (2-D) like everywhere in tests/: the leaf
level of the whole domain, unit box (-0.5, 0.5)^dim (physical_params.L = 1), or of a cubic lattice of
unit boxes with `n_box` cells per side and box."""
import math
from fractions import Fraction

import numpy as np

LD = np.longdouble
CLD = np.clongdouble
EPS = float(np.finfo(LD).eps)
_PI = LD(4) * np.arctan(LD(1))


def _twiddles(n):
    """exp (-2 pi i m/n) for m = 0 .. n - 1.  The angle is reduced in integers to [0, pi/4] before cos and
    sin are taken (quadrant, then complement), so every entry is within about one eps and the values on
    the axes and diagonals are exact or correctly rounded."""
    a = 4 * np.arange(n)                          # angle = (pi/2) a/n
    quad, rem = a // n, a % n
    comp = 2 * rem > n
    phi = (_PI / LD(2)) * np.where(comp, n - rem, rem).astype(LD) / LD(n)
    c, s = np.cos(phi), np.sin(phi)
    c, s = np.where(comp, s, c), np.where(comp, c, s)
    cq = np.choose(quad, [c, -s, -c, s])
    sq = np.choose(quad, [s, c, -s, -c])
    return (cq - 1j * sq).astype(CLD)


def _dft_matrix(n):
    """W[k][j] = exp (-2 pi i (j k mod n)/n): the angles are exact multiples of 2 pi/n"""
    return _twiddles(n)[(np.arange(n)[:, None] * np.arange(n)[None, :]) % n]


def direct_dft(a):
    """F[k] = sum_j a[j] exp (-2 pi i j.k/N) over every axis, all N indices on every axis (no
    half-spectrum, no normalisation: the sign and scale of FFTW's forward transform)."""
    F = np.asarray(a).astype(CLD)
    for ax in range(F.ndim):
        F = np.moveaxis(np.tensordot(_dft_matrix(F.shape[ax]), F, axes=([1], [ax])), 0, ax)
    return F


# ---- the pieces of modules/fft.c the outputs are made of -----------------------------------------

def cell_centres(n, n_box=None):
    """ftt_cell_pos along one direction: the lattice starts at -0.5, dx = 1/n_box"""
    nb = n if n_box is None else n_box
    return LD(-0.5) + (np.arange(n).astype(LD) + LD(0.5)) / LD(nb)


def all_levels_average(v, n_box=None):
    """substract_average (:897-908) / add_data (:885-890): val = sum vol*v, vol = sum vol over the cells
    of ALL levels (FTT_TRAVERSE_ALL; level 0 = one cell per box), val/vol.  The value of a cell that is
    not a leaf is the average of its children."""
    a = np.asarray(v).astype(LD)
    dim = a.ndim
    m = a.shape[0] if n_box is None else n_box      # cells per side of a box at this level
    val, vol = LD(0), LD(0)
    while True:
        cv = (LD(1) / LD(m)) ** dim                 # gfs_cell_volume
        val += cv * a.sum()
        vol += cv * LD(a.size)
        if m == 1:
            break
        sh = []
        for s in a.shape:
            sh += [s // 2, 2]
        a = a.reshape(sh).sum(axis=tuple(range(1, 2 * dim, 2))) / LD(2 ** dim)
        m //= 2
    return val / vol


def order_array(pos_min_global, pos_max_global, dx, Ndim):
    """order_array (:800-820): np = |max - min|/dx + 1 per coordinate, sorted with `b.np - a.np', that is
    in DESCENDING order of np; npaux = np except for dirdata[Ndim - 1], which gets np/2 + 1.
    The reference leaves the order of directions with equal np to g_array_sort (a qsort): here the sort
    is stable, equal np stay in coordinate order."""
    dirs = []
    for i in range(3):
        # (gint) of a quotient that is an integer up to rounding: guarded against landing just below it
        np_ = int(abs(pos_max_global[i] - pos_min_global[i]) / dx + LD(1) + LD(1e-9))
        dirs.append(dict(coord=i, np=np_, npaux=np_))
    dirdata = sorted(dirs, key=lambda d: -d["np"])
    dirdata[Ndim - 1]["npaux"] = dirdata[Ndim - 1]["np"] // 2 + 1
    return dirdata


def init_kmax(pos_min_global, pos_max_global):
    """init_kmax (:1033-1047): 2 pi/L per coordinate, L = |pos_max_global - pos_min_global|, 0 if L = 0"""
    kmax = []
    for i in range(3):
        L = abs(pos_max_global[i] - pos_min_global[i])
        kmax.append(LD(2) * _PI / L if L != 0 else LD(0))
    return kmax


def write_spectra(out, dirdata, kmax):
    """write_spectra (:1049-1085) with L = 1, as rows (kx, ky, kz, re, im).  `out' is the flat complex
    array the transform of dimensions (dirdata[0].np, dirdata[1].np, dirdata[2].np) leaves, last
    dimension of length dirdata[2].npaux.  The loop over i runs over all of dirdata[0].np (the slabs
    local_0_start .. + local_n0 of all processes together)."""
    np0, np1, npaux2 = dirdata[0]["np"], dirdata[1]["np"], dirdata[2]["npaux"]
    i, j, l = np.meshgrid(np.arange(np0), np.arange(np1), np.arange(npaux2), indexing="ij")
    i, j, l = i.ravel(), j.ravel(), l.ravel()                       # the order of the three loops
    k = np.zeros((i.size, 3), dtype=LD)
    k[:, dirdata[0]["coord"]] = kmax[dirdata[0]["coord"]] * np.where(i < np0 // 2 + 1, i, i - np0)    # :1063-1067
    k[:, dirdata[1]["coord"]] = kmax[dirdata[1]["coord"]] * np.where(j < np1 // 2 + 1, j, j - np1)    # :1069-1073
    k[:, dirdata[2]["coord"]] = kmax[dirdata[2]["coord"]] * l                                         # :1075
    o = out[l + npaux2 * (i * np1 + j)]                                                               # :1078
    return np.column_stack([k, o.real, o.imag])


def _r2c_3d(a, dirdata):
    """fftw_plan_dft_r2c_3d (dirdata[0].np, dirdata[1].np, dirdata[2].np) (:1087-1098) of a real array
    indexed in that order: the flat output, whose last dimension keeps the first np2/2 + 1 =
    dirdata[2].npaux entries of the full transform (Ndim = 3: dirdata[2] is the halved one)."""
    assert a.shape == tuple(d["np"] for d in dirdata)
    T = direct_dft(a)
    return np.ascontiguousarray(T[:, :, :dirdata[2]["npaux"]]).reshape(-1)


def spectra_rows_box(v, n_box=None):
    """GfsOutputSpectra (:1101-1166) of the whole 3-D domain at the finest level, realdim == 3: the rows
    of write_spectra.  v: [k][j][i]."""
    v = np.asarray(v)
    N = v.shape[0]
    c = cell_centres(N, n_box)
    dx = c[1] - c[0]
    # get_deep_level / get_domain_limits (:443-450, :911-928): extreme cell centres inside the box
    pos_min_global, pos_max_global = [c[0]] * 3, [c[-1]] * 3
    dirdata = order_array(pos_min_global, pos_max_global, dx, 3)
    # fill_cartesian_matrix (:966-1001): u = v - average (all levels), get_data (:403-420): the value of
    # the cell at (i, j, k) = its coordinates along dirdata[0..2].coord, divided by ntot
    u = np.transpose(v.astype(LD) - all_levels_average(v, n_box))        # [ix][iy][iz]
    ntot = dirdata[2]["np"] * dirdata[1]["np"] * dirdata[0]["np"]
    a = np.transpose(u, [d["coord"] for d in dirdata]) / LD(ntot)
    return write_spectra(_r2c_3d(a, dirdata), dirdata, init_kmax(pos_min_global, pos_max_global))


def locate(pos, N):
    """gfs_domain_locate along one direction of the unit box: the index of the cell whose extent
    [-0.5 + k/N, -0.5 + (k + 1)/N) holds pos (exact arithmetic), None outside"""
    k = math.floor((Fraction(float(pos)) + Fraction(1, 2)) * N)
    return k if 0 <= k < N else None


def spectra_rows_plane(v, normal, pos):
    """GfsOutputSpectra with a box that is flat along `normal' (0 x, 1 y, 2 z) at coordinate pos,
    realdim == 2, d.Ndim = 3 (:1121): the rows of write_spectra.  v: [k][j][i], one box.

    inside_domain (:348-362) selects cells only when pos IS a cell-centre coordinate; there the cell
    holding the plane is that cell.  For any other pos the cell holding the plane is taken (what
    gfs_domain_locate does in fill_interpolated_cartesian_matrix): an extension.  The points of the
    plane are stored in the order of dirdata, which is what get_index_matrix (:393-401) amounts to for a
    z-normal plane; for the two other normals the reference's (ix, iy, iz) indexing does not land where
    its transform reads and this is the coherent analogue."""
    v = np.asarray(v)
    N = v.shape[0]
    c = cell_centres(N)
    dx = c[1] - c[0]
    kc = locate(pos, N)
    if kc is None:
        raise ValueError("the plane lies outside the box")
    pos_min_global, pos_max_global = [c[0]] * 3, [c[-1]] * 3
    pos_min_global[normal] = pos_max_global[normal] = c[kc]
    dirdata = order_array(pos_min_global, pos_max_global, dx, 3)        # descending: the flat one is LAST
    assert [d["np"] for d in dirdata] == [N, N, 1] and dirdata[2]["coord"] == normal
    assert dirdata[2]["npaux"] == 1                                     # 1/2 + 1 (:817)
    # fill_interpolated_cartesian_matrix (:836-876): the value of the cell each point lies in, avg = their
    # sum / their number np, then v -= avg, v /= np
    val = np.take(np.transpose(v.astype(LD)), [kc], axis=normal)        # [ix][iy][iz], one entry along normal
    npts = val.size
    avg = val.sum() / LD(npts)
    val = (val - avg) / LD(npts)
    a = np.transpose(val, [d["coord"] for d in dirdata])                # (N, N, 1)
    return write_spectra(_r2c_3d(a, dirdata), dirdata, init_kmax(pos_min_global, pos_max_global))


def get_index(i, j, k, np_, dim):
    """get_index (:1350-1357)"""
    if dim == 2:
        return j + (np_ // 2 + 1) * i
    return k + (np_ // 2 + 1) * (j + np_ * i)


def energy_bins(comps, n_box=None):
    """GfsOutputEnergySpectra (:1360-1474) of the velocity components comps ([j][i] in 2-D, [k][j][i] in
    3-D): (Ek, Etot, deltak) with Ek the nk bins before printing (write_energy_spectra prints i >= 1).
    The directions are those of order_array on a cube, x, y(, z), the last one halved."""
    dim = comps[0].ndim
    np_ = comps[0].shape[0]                                             # np = d.dirdata[0].np (:1405)
    nh = np_ // 2 + 1
    nk = (dim + 1) * nh ** 2                                            # d.cgd->N = FTT_DIMENSION + 1 (:1379, :1406)
    Ek = np.zeros(nk, dtype=LD)
    for u in comps:
        a = np.transpose(np.asarray(u).astype(LD) - all_levels_average(u, n_box)) / LD(np_ ** dim)
        T = direct_dft(a)                                               # [ix][iy]([iz]), full
        out = np.ascontiguousarray(T[..., :nh]).reshape(-1)             # r2c: last dimension halved
        P = out.real ** 2 + out.imag ** 2
        i = np.arange(np_)
        knx = np.where(i < nh, i, np_ - i)                              # :1418-1419, :1432-1433
        if dim == 2:
            np.add.at(Ek, knx ** 2, LD(0.5) * P[get_index(i, 0, 0, np_, 2)])          # :1420-1422
            ii, jj = np.meshgrid(i, np.arange(nh), indexing="ij")                     # j = 0 .. np/2 (:1424)
            np.add.at(Ek, (knx[ii] ** 2 + jj ** 2).ravel(), P[get_index(ii, jj, 0, np_, 2)].ravel())
        else:
            ii, jj = np.meshgrid(i, i, indexing="ij")
            kny = knx                                                                 # :1435-1436
            np.add.at(Ek, (knx[ii] ** 2 + kny[jj] ** 2).ravel(),
                      LD(0.5) * P[get_index(ii, jj, 0, np_, 3)].ravel())              # :1437-1439
            ii, jj, kk = np.meshgrid(i, i, np.arange(1, nh), indexing="ij")           # k = 1 .. np/2 (:1440)
            np.add.at(Ek, (knx[ii] ** 2 + kny[jj] ** 2 + kk ** 2).ravel(),
                      P[get_index(ii, jj, kk, np_, 3)].ravel())                       # :1441-1443
    Etot = LD(0)
    for j in range(nk):                                                 # :1456-1460
        Etot += Ek[j]
    c = cell_centres(np_, n_box)
    deltak = LD(2) * _PI / (c[-1] - c[0])                               # :1464
    return Ek, Etot, deltak


# ---- the layouts gfship documents (include/gfship.h), turned into the same rows -------------------

def rows_of_box_output(F, kstep):
    """gfship_output_spectra: F[ix][iy][iz <= N/2], k = kstep times the signed index"""
    N = F.shape[0]
    i, j, l = [x.ravel() for x in np.meshgrid(np.arange(N), np.arange(N), np.arange(N // 2 + 1), indexing="ij")]
    sg = lambda q: np.where(q < N // 2 + 1, q, q - N)
    return np.column_stack([kstep * sg(i), kstep * sg(j), kstep * l, F.real.ravel(), F.imag.ravel()])


def rows_of_plane_output(F, kstep, normal):
    """gfship_output_spectra_plane: F[ia][ib], ia / ib the first / second in-plane coordinate, both signed;
    0 along the normal"""
    N = F.shape[0]
    assert F.shape == (N, N)
    ia, ib = [x.ravel() for x in np.meshgrid(np.arange(N), np.arange(N), indexing="ij")]
    sg = lambda q: np.where(q < N // 2 + 1, q, q - N)
    k = np.zeros((N * N, 3))
    k[:, 1 if normal == 0 else 0] = kstep * sg(ia)
    k[:, 1 if normal == 2 else 2] = kstep * sg(ib)
    return np.column_stack([k, F.real.ravel(), F.imag.ravel()])


# ---- fields and comparisons shared by the CPU and the GPU tests ----------------------------------

TOL_COEF = 1e-13            # max abs on coefficients (the project's own: tests/test_gpu_spectra.py)
TOL_BINS = 1e-12            # times Etot, per bin


def checkerboard(n, dim, axis, A):
    """A (-1)^i along coordinate `axis' (0 = x), as an array [k][j][i] / [j][i]"""
    sh = [1] * dim
    sh[dim - 1 - axis] = n
    return np.broadcast_to(A * ((-1.) ** np.arange(n)).reshape(sh), (n,) * dim).copy()


def cosine(n, dim, axis, m, A, extended=False):
    """A cos (2 pi m x_axis) at the cell centres (in double, or in long double)"""
    if extended:
        x = (np.arange(n).astype(LD) + LD(0.5)) / LD(n) - LD(0.5)
        f = LD(A) * np.cos(2 * _PI * m * x)
    else:
        x = (np.arange(n) + 0.5) / n - 0.5
        f = A * np.cos(2. * np.pi * m * x)
    sh = [1] * dim
    sh[dim - 1 - axis] = n
    return np.broadcast_to(f.reshape(sh), (n,) * dim).copy()


def checkerboard_bin_3d(axis, A):
    return A * A if axis == 2 else A * A / 2.


def cosine_bin_2d(axis, A):
    return 3. * A * A / 4. if axis == 0 else A * A / 4.


def random_field(n, dim, seed, mean=0.3):
    """amplitude ~ 1: noise, a non-zero mean and a different imposed mode along every axis"""
    rng = np.random.default_rng(seed)
    x = (np.arange(n) + 0.5) / n - 0.5
    g = np.meshgrid(*([x] * dim), indexing="ij")[::-1]               # g[0] = X
    a = mean + 0.1 * rng.standard_normal((n,) * dim)
    for c in range(dim):
        a = a + (1. - 0.2 * c) * np.sin(2. * np.pi * min(c + 1, n // 2) * g[c] + 0.3 * c)
    return a


def assert_rows_match(got, want, tol=TOL_COEF, label=None):
    """rows (kx, ky, kz, re, im): same number, same order, k to a few double eps, coefficients to tol;
    prints (with a label) and returns the largest coefficient error"""
    assert got.shape == want.shape
    kw = want[:, :3].astype(float)
    assert np.abs(got[:, :3] - kw).max() <= 4e-16 * np.abs(kw).max()
    err = float(np.abs(got[:, 3:].astype(LD) - want[:, 3:]).max())
    if label:
        print("direct-dft coefficients %s: max abs error %.3e (bound %.1e)" % (label, err, tol))
    assert err <= tol, err
    return err


def assert_bins_match(got, want, tol=TOL_BINS, label=None):
    """got: (k, Ek[1:], Etot) as gfship / the oracle return them; want: (Ek, Etot, deltak) of
    dft_reference.energy_bins; prints (with a label) and returns the largest bin error over Etot"""
    k, Ek, Etot = got
    Ek0, Etot0, deltak0 = want
    assert len(Ek) == len(Ek0) - 1
    i = np.arange(1, len(Ek0))
    k0 = (deltak0 * np.sqrt(i.astype(LD))).astype(float)
    assert np.abs(k - k0).max() <= 4e-16 * k0.max()
    et = float(Etot0)
    err = float(np.abs(Ek.astype(LD) - Ek0[1:]).max()) / et
    if label:
        print("direct-dft bins %s: max error %.3e Etot, Etot error %.3e Etot (bound %.1e)"
              % (label, err, abs(Etot - et) / et, tol))
    assert abs(Etot - et) <= tol * et
    assert err <= tol, err
    return err


def plane_field(n, seed):
    """different modes along x and y, an amplitude that depends on z, noise: a transposed plane, a wrong
    cell index along the normal or an unsigned k each change the rows"""
    rng = np.random.default_rng(seed)
    c = -0.5 + (np.arange(n) + 0.5) / n
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    mx, my = min(3, n // 2), min(2, n // 2)
    return 0.4 + np.sin(2. * np.pi * mx * x + 0.2) * np.cos(2. * np.pi * my * y) * (1. + z) + \
        0.5 * np.sin(2. * np.pi * z) + 0.1 * rng.standard_normal((n,) * 3)
