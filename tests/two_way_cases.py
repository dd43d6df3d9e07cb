"""The inputs of the two-way coupling tests (tests/test_two_way_reference_cpu.py checks their properties on
the restatement, tests/test_gpu_two_way.py runs them on the device).  Unit box, L = 1."""
import numpy as np

# kernel texts of GfsSourceParticulate and the same functions for the restatement
POLY_TEXT = "(1. - 0.04*(x*x + y*y + z*z))"
EXP_TEXT = "exp(-(x*x+y*y+z*z))"


def poly_kernel(x, y, z, t):
    return (1. - 0.04 * (x * x + y * y + z * z))


def exp_kernel(x, y, z, t):
    import math
    return math.exp(-(x * x + y * y + z * z))


# the cases of the GPU tests: 2-D level 4 and 3-D levels 3 and 4, the smallest boxes in which a kernel of
# rkernel = 2.5 h is clipped at one side and not at the other
BOXES = [(2, 4), (3, 3), (3, 4)]
RKERNEL_H = [0., 1.5, 2.5]


def void_fraction_case(dim, depth, seed=7):
    """300 particles with volumes over six decades: 40 of them four by four in ten cells, one on a cell
    face, one outside the box"""
    rng = np.random.default_rng(seed + 10 * dim + depth)
    n = 1 << depth
    h = 1. / n
    npart = 300
    pos = rng.random((npart, 3)) - 0.5
    cells = rng.integers(0, n, size=(10, 3))
    for q in range(40):
        pos[q] = -0.5 + (cells[q % 10] + 0.1 + 0.8 * rng.random(3)) * h
    pos[40] = [-0.5 + 3 * h, -0.5 + 2.25 * h, -0.5 + 1.5 * h]       # on the face between cells 2 and 3 along x
    pos[41] = [-0.5 + 3.5 * h, -0.5 + 2.25 * h, -0.5 + 1.5 * h]     # and a neighbour in cell 3
    pos[42] = [0.7, 0.1, -0.2]                                      # outside
    if dim == 2:
        pos[:, 2] = 0.
    volume = 10. ** rng.uniform(-9., -3., npart)
    return pos, np.arange(1, npart + 1, dtype=np.uint32), volume


def spreading_case(dim, depth, seed=3):
    """80 particulates for the spreading: 14 within one cell's width of each other in the middle of the box
    (their kernels overlap in every cell around), 10 within half a cell of the side x = +0.5 (periodic in
    the GPU test: no wrap), 10 within half a cell of the side y = -0.5 (a wall), the rest anywhere.
    Volumes over six decades: rb of distance_normalization runs from a seventh of a cell to several cells,
    so the polynomial kernel is positive over the whole stencil of the large particles and negative over
    that of the small ones (correction <= 1e-10: nothing deposited).  `force' is a stand-in, of the size of
    a drag force (proportional to the volume), for tests without a device."""
    rng = np.random.default_rng(seed + 10 * dim + depth)
    n = 1 << depth
    h = 1. / n
    npart = 80
    pos = rng.random((npart, 3)) - 0.5
    centre = np.array([0.5 * h, -0.5 * h, 0.5 * h])
    pos[:14] = centre + (rng.random((14, 3)) - 0.5) * h
    pos[14:24, 0] = 0.5 - 0.5 * h * rng.random(10)
    pos[24:34, 1] = -0.5 + 0.5 * h * rng.random(10)
    volume = 10. ** rng.uniform(-5.5, 0.5, npart)
    volume[:14] = 10. ** rng.uniform(-3., 0.5, 14)
    # one particle far smaller than a cell and away from the centre of its cell: the polynomial kernel is
    # negative on every leaf it reaches, whatever rkernel
    pos[40] = [-0.5 + 5.9 * h, -0.5 + 6.9 * h, -0.5 + 2.9 * h]
    volume[40] = 1e-9
    # velocities of any direction and of sizes over six decades: with the volumes, drag forces over six too
    vel = rng.standard_normal((npart, 3))
    if dim == 2:
        pos[:, 2] = 0.
        vel[:, 2] = 0.
    vel *= (10. ** rng.uniform(-3., 4., npart) / np.sqrt((vel * vel).sum(axis=1)))[:, None]
    mass = volume * (0.5 + 2.5 * rng.random(npart))
    force = volume[:, None] * 10. * rng.standard_normal((npart, 3))
    if dim == 2:
        force[:, 2] = 0.
    return pos, np.arange(1, npart + 1, dtype=np.uint32), vel, mass, volume, force


# the spreading in more than one chunk (a chunk holds 2^22 record slots): a 3-D box of level 5, or the uniform octree
# of that level, and rkernel = 16 h -- the slots of a particle are capped at the 32^3 leaves, 128 particles fill a
# chunk, and the 130 particulates of spreading_chunks_case make a second chunk of two.  The kernel is positive
# everywhere: every particle deposits
CHUNKS_DEPTH, CHUNKS_RKERNEL_H, CHUNKS_PER_CHUNK, CHUNKS_N = 5, 16., 128, 130
CHUNKS_TEXT = "(1. + 1e-6*(x*x + y*y + z*z))"


def chunks_kernel(x, y, z, t):
    return (1. + 1e-6 * (x * x + y * y + z * z))


def spreading_chunks_case(seed=11):
    """130 particulates anywhere in the 3-D box, volumes over three decades; `force' as in spreading_case"""
    rng = np.random.default_rng(seed)
    npart = CHUNKS_N
    pos = rng.random((npart, 3)) - 0.5
    volume = 10. ** rng.uniform(-4., -1., npart)
    vel = rng.standard_normal((npart, 3))
    vel *= (10. ** rng.uniform(-3., 4., npart) / np.sqrt((vel * vel).sum(axis=1)))[:, None]
    mass = volume * (0.5 + 2.5 * rng.random(npart))
    force = volume[:, None] * 10. * rng.standard_normal((npart, 3))
    return pos, np.arange(1, npart + 1, dtype=np.uint32), vel, mass, volume, force


def assert_two_chunks_are_order_sensitive(R, pos, volume, force, alpha=None):
    """spread_flat of the two-chunk case with these forces: at least 20 particles of the first chunk and both of the
    second deposit, and reversing the list changes at least one component.  Returns F of the list order"""
    rk = CHUNKS_RKERNEL_H / (1 << CHUNKS_DEPTH)
    want, corr = R.spread_flat(3, CHUNKS_DEPTH, pos, volume, force, rk, chunks_kernel, alpha_cell=alpha)
    assert len(pos) == CHUNKS_N > CHUNKS_PER_CHUNK
    assert (corr[:CHUNKS_PER_CHUNK] > 1.e-10).sum() >= 20 and (corr[CHUNKS_PER_CHUNK:] > 1.e-10).all()
    rev, _ = R.spread_flat(3, CHUNKS_DEPTH, pos[::-1], volume[::-1], force[::-1], rk, chunks_kernel, alpha_cell=alpha)
    assert any(not np.array_equal(want[c], rev[c]) for c in range(3))
    return want


def device_sim(gfship, osim, side):
    """a device simulation initialised from the current state of an oracle simulation, with its solver and
    advection parameters"""
    gd = gfship.Domain(osim.dim, osim.depth, side)
    gs = gfship.Simulation(gd)
    for c in range(osim.dim):
        gs.u[c].upload(osim.u[c].leaf())
    for name in ("projection_params", "approx_projection_params"):
        op, gp = getattr(osim, name), getattr(gs, name)
        for f in ("tolerance", "nrelax", "erelax", "minlevel", "nitermax", "nitermin", "omega"):
            setattr(gp, f, getattr(op, f))
    gs.advection_params.cfl = osim.advection_params.cfl
    gs.advection_params.gradient = osim.advection_params.gradient
    return gd, gs


def alpha_cell_case(dim, depth):
    """alpha at the cell centres: three values, two of them with an inexact 1./alpha"""
    n = 1 << depth
    idx = np.indices((n,) * dim).sum(axis=0)
    return np.choose(idx % 3, [1., 0.8, 1.3])


def smooth_velocity(dim, depth):
    """a smooth velocity on the leaf level, ghost cells included, arrays indexed [k][j][i]"""
    n = 1 << depth
    x = -0.5 + (np.arange(n + 2) - 0.5) / n
    g = np.meshgrid(*([x] * dim), indexing="ij")
    X, Y = g[-1], g[-2]
    Z = g[0] if dim == 3 else np.zeros_like(X)
    tp = 2. * np.pi
    return [np.sin(tp * X) * np.cos(tp * Y) * (1. + 0.3 * np.cos(tp * Z)),
            -np.cos(tp * X) * np.sin(tp * Y) * (1. + 0.2 * np.sin(tp * Z)),
            0.4 * np.sin(tp * (X + Y + Z))][:dim]


# runs without source fields whose launches must stay what they were before the feature: (name, dim,
# depth, sides, viscosity); sides: 0 periodic, 1 boundary (gfship.SIDE_*)
PLAIN_RUNS = [("periodic-3d", 3, 4, [0] * 6, 0.),
              ("periodic-3d-viscous", 3, 4, [0] * 6, 1e-2),
              ("channel-2d-viscous", 2, 4, [0, 0, 1, 1, 0, 0], 1e-2)]


def plain_run_kernel_counts(gfship, name):
    """gfship_domain_kernel_counts after start and two steps of one of PLAIN_RUNS"""
    _, dim, depth, sides, nu = [r for r in PLAIN_RUNS if r[0] == name][0]
    gd = gfship.Domain(dim, depth, sides)
    gs = gfship.Simulation(gd)
    try:
        for c, a in enumerate(smooth_velocity(dim, depth)):
            gs.u[c].upload(a)
            if nu:
                gs.set_viscosity(c, nu)
        gs.start()
        gs.step()
        gs.step()
        return {k: int(v) for k, v in gd.kernel_counts().items()}
    finally:
        gs.destroy()
        gd.destroy()
