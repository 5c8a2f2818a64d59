"""Shapes, inputs and the numpy float64 model of the direct cosine-transform
pressure solve (HIP_POISSON_DCT, cfd_amd/csrc/hip/transform_solve.hpp), shared by
tests/test_dct_cases.py (the model against the oracle's RB-SOR and Jacobi, on
the CPU) and tests/test_gpu_dct.py (the device against both).

The algorithm: RB-SOR and Jacobi apply the Neumann BC after every sweep, so at
their fixed point every shell cell equals its interior neighbour and the
interior operator is the cell-centred Neumann Laplacian. With n = size - 2,
    Q_n[a][b] = w_a cos(pi a (2b+1) / (2n)),  w_0 = sqrt(1/n), w_a = sqrt(2/n),
    lambda_n[a] = 4 sin^2(pi a / (2n)) / h^2
on each axis, the six steps are
    1. res0 = max |lap(x) - rhs| of x as it stands (no start BC); below
       absolute_tolerance: CONVERGED, 0 iterations, x untouched
    2. t = Qz Qy Qx (-rhs) on the interior
    3. t /= lx[i] + ly[j] + lz[k], the zero mode set to 0.0 and never divided
    4. x_interior = Qx^T Qy^T Qz^T t
    5. the Neumann shell
    6. res = max |lap(x) - rhs|; CONVERGED when res < max(tol res0, abs) or
       res < abs, else MAX_ITER; iterations = 1.
"""
from __future__ import annotations

import functools

import numpy as np

from cfd_amd import _abi as A
from oracle import oracle
from tests import dst_cases as D

# the sine solver's table (the passes' tile edges are the same) and two shapes
# that put an even and an odd n on every axis
SHAPE_LIST = list(D.SHAPE_LIST) + [(18, 17, 1), (10, 11, 12)]

# Largest deviation of the model below from the oracle's relaxation solvers run
# to TIGHT_TOL, both demeaned over the interior, relative to max |x - mean|
# (test_dct_cases.test_model_matches_tight_relaxation prints it), times 100:
# the margin of DST_BAR and the BiCGSTAB pin. Measured 1.81e-10 (Jacobi,
# 34 x 34 x 34, 27 028 iterations; RB-SOR 2.24e-11 on 67 x 35 x 18): the
# oracle's stopping point is the limit, not the model (at 1e-13 the same runs
# give 1.81e-8 and 2.26e-9). DESIGN.md, the direct cosine-transform solve.
DCT_MEASURED = 1.81e-10
DCT_BAR = 1.81e-8

# The tightest power of ten at which the oracle reports CONVERGED on every
# shape it is run on from these inputs: at 1e-16 its RB-SOR stalls on
# 67 x 35 x 1 (test_dct_cases.test_tight_tolerance_is_the_tightest_power_of_ten)
TIGHT_TOL = 1e-15
TIGHT = dict(tolerance=TIGHT_TOL, absolute_tolerance=1e-300, max_iterations=400000)
JACOBI_MAX_EXTENT = 40      # the tight Jacobi run: shapes with every extent <= this
LIMIT_MAX_EXTENT = 24       # the incompatible input's Jacobi limit: ... <= this
LIMIT_ITERATIONS = 30000    # ... at this fixed cap (MAX_ITER accepted)

sid = D.sid
spacing = D.spacing
interior = D.interior
shell_mask = D.shell_mask


def extents(shape):
    return shape if shape[2] > 1 else shape[:2]


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    nx, ny, nz = shape
    rng = np.random.default_rng(7000003 * nx + 7001 * ny + nz)
    bad = rng.standard_normal((nz, ny, nx))
    x0 = 0.1 * rng.standard_normal((nz, ny, nx))
    good = bad - np.mean(bad[interior(bad.shape)])
    for a in (good, bad, x0):
        a.setflags(write=False)
    return good, bad, x0


def inputs(shape):
    """(compatible rhs, incompatible rhs, x0) on the whole (nz, ny, nx) array,
    shell included; read-only. The compatible right-hand side is the
    incompatible one with its interior mean subtracted."""
    return _inputs(tuple(shape))


def demean(x):
    """x minus its interior mean (the whole array: the Neumann shell follows)."""
    return x - np.mean(x[interior(x.shape)])


def rel_dev(x, ref):
    """max |demean(x) - demean(ref)| relative to max |ref - mean| (absolute
    where the demeaned reference is zero: one interior cell)."""
    a, b = demean(x), demean(ref)
    scale = float(np.max(np.abs(b)))
    dev = float(np.max(np.abs(a - b)))
    return dev / scale if scale > 0.0 else dev


# ---------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------
_PI_L = np.longdouble(4) * np.arctan(np.longdouble(1))


def cos_matrix_ld(n, half_shift=True):
    """Q_n in long double, the argument reduced as an integer first."""
    a = np.arange(n, dtype=np.int64)
    b = 2 * a + 1 if half_shift else 2 * a
    m = np.outer(a, b) % (4 * n)
    w = np.full(n, np.sqrt(np.longdouble(2) / n))
    w[0] = np.sqrt(np.longdouble(1) / n)
    return w[:, None] * np.cos(_PI_L * m.astype(np.longdouble) / np.longdouble(2 * n))


@functools.lru_cache(maxsize=None)
def cos_matrix(n, half_shift=True):
    """Q_n rounded once to double."""
    return cos_matrix_ld(n, half_shift).astype(np.float64)


def eig(n, shift=0):
    """e_n[a] = 4 sin^2(pi (a + shift) / (2n)) rounded once to double."""
    a = (np.arange(n) + shift).astype(np.longdouble)
    s = np.sin(_PI_L * a / np.longdouble(2 * n))
    return (4 * s * s).astype(np.float64)


def apply_along(M, v, ax):
    """M applied along array axis ax of v."""
    return np.moveaxis(np.tensordot(M, v, axes=([1], [ax])), 0, ax)


def transform(a, axis, inverse=False):
    """The orthonormal DCT-II (inverse: its transpose) of the interior of `a`
    (nz, ny, nx) along axis 0 (x), 1 (y), 2 (z); the boundary left as it is."""
    out = a.copy()
    inn = interior(a.shape)
    ax = 2 - axis
    v = a[inn]
    Q = cos_matrix(v.shape[ax])
    out[inn] = apply_along(Q.T if inverse else Q, v, ax)
    return out


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------
class Result:
    def __init__(self, rc, status, iterations, res0, res, x):
        self.rc, self.status, self.iterations = rc, status, iterations
        self.initial_residual, self.final_residual, self.x = res0, res, x


def residual_linf(x, rhs, d):
    """max |lap(x) - rhs| over the interior in the relaxation solvers' own
    operation order (linear_solver.c:304-346, k_residual_linf)."""
    nz = x.shape[0]
    inn = interior(x.shape)
    c = x[inn]
    dx2, dy2 = d[0] * d[0], d[1] * d[1]
    if nz > 1:
        inv_dz2 = 1.0 / (d[2] * d[2])
        lap = ((x[1:-1, 1:-1, 2:] - 2.0 * c + x[1:-1, 1:-1, :-2]) / dx2 +
               (x[1:-1, 2:, 1:-1] - 2.0 * c + x[1:-1, :-2, 1:-1]) / dy2 +
               (x[2:, 1:-1, 1:-1] + x[:-2, 1:-1, 1:-1] - 2.0 * c) * inv_dz2)
    else:
        lap = ((x[:, 1:-1, 2:] - 2.0 * c + x[:, 1:-1, :-2]) / dx2 +
               (x[:, 2:, 1:-1] - 2.0 * c + x[:, :-2, 1:-1]) / dy2)
    return float(np.max(np.abs(lap - rhs[inn])))


# the planted bugs of model_solve(bug=...)
BUGS = {
    "swap_q": "Q and Q^T swapped (acts where some n >= 3: Q_1 and Q_2 are symmetric)",
    "eig_shift": "eigenvalue index a + 1",
    "no_half": "the half-sample shift dropped: cos(pi a b / n)",
    "swap_h": "1/h^2 of x and y exchanged",
    "zero_div": "the zero mode divided by 1e-30 instead of dropped (incompatible input)",
    "no_neg": "the right-hand side not negated",
}


def bug_exempt(bug, shape):
    """Shapes a planted bug cannot act on: one interior cell on every axis
    leaves only the zero mode, and the demeaned result is zero whatever is
    done; Q_1 and Q_2 are symmetric."""
    n = [v - 2 for v in extents(shape)]
    if bug == "swap_q":
        return all(v <= 2 for v in n)
    return all(v == 1 for v in n)


def model_solve(x0, rhs, d, tolerance=1e-6, absolute_tolerance=1e-10, *, bug=None):
    """The six steps of the module docstring in numpy float64."""
    assert bug is None or bug in BUGS
    x = np.ascontiguousarray(x0, dtype=np.float64).copy()
    is3d = x.shape[0] > 1
    res0 = residual_linf(x, rhs, d)
    tol = max(tolerance * res0, absolute_tolerance)
    if res0 < absolute_tolerance:
        return Result(A.CFD_SUCCESS, A.POISSON_CONVERGED, 0, res0, res0, x)
    inn = interior(x.shape)
    ih2 = [1.0 / (d[0] * d[0]), 1.0 / (d[1] * d[1]), 1.0 / (d[2] * d[2]) if is3d else 0.0]
    if bug == "swap_h":
        ih2 = [ih2[1], ih2[0], ih2[2]]
    t = rhs[inn].copy() if bug == "no_neg" else -rhs[inn]
    n = t.shape
    axes = [2, 1] + ([0] if is3d else [])  # x, y, z as array axes
    Q = {ax: cos_matrix(n[ax], bug != "no_half") for ax in axes}
    fwd = {ax: (Q[ax].T if bug == "swap_q" else Q[ax]) for ax in axes}
    inv = {ax: (Q[ax] if bug == "swap_q" else Q[ax].T) for ax in axes}
    for ax in axes:
        t = apply_along(fwd[ax], t, ax)
    sh = 1 if bug == "eig_shift" else 0
    lam = eig(n[2], sh)[None, None, :] * ih2[0] + eig(n[1], sh)[None, :, None] * ih2[1]
    if is3d:
        lam = lam + eig(n[0], sh)[:, None, None] * ih2[2]
    lam = np.broadcast_to(lam, n).copy()
    zero = t[0, 0, 0]
    lam[0, 0, 0] = 1.0
    t = t / lam
    t[0, 0, 0] = zero / 1e-30 if bug == "zero_div" else 0.0
    for ax in reversed(axes):
        t = apply_along(inv[ax], t, ax)
    x[inn] = t
    oracle.poisson_apply_bc(x)
    res = residual_linf(x, rhs, d)
    conv = res < tol or res < absolute_tolerance
    return Result(A.CFD_SUCCESS if conv else A.CFD_ERROR_MAX_ITER,
                  A.POISSON_CONVERGED if conv else A.POISSON_MAX_ITER, 1, res0, res, x)


@functools.lru_cache(maxsize=None)
def _model(shape, which):
    good, bad, x0 = inputs(shape)
    m = model_solve(x0, good if which == "compatible" else bad, spacing(shape))
    m.x.setflags(write=False)
    return m


def model(shape, which="compatible"):
    """model_solve on inputs(shape) at the default tolerances, once."""
    return _model(tuple(shape), which)


# ---------------------------------------------------------------------------
# the oracle's relaxation solvers, once per (shape, method, input)
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _relax(shape, method, which):
    good, bad, x0 = inputs(shape)
    x = x0.copy()
    if which == "compatible":
        rhs, prm = good, oracle.poisson_params(**TIGHT)
    else:
        rhs, prm = bad, oracle.poisson_params(tolerance=0.0, absolute_tolerance=0.0,
                                              max_iterations=LIMIT_ITERATIONS)
    fn = oracle.redblack_solve if method == "redblack" else oracle.jacobi_solve
    s, st = fn(x, np.ascontiguousarray(rhs), *spacing(shape), prm)
    x.setflags(write=False)
    return s, st.status, st.iterations, x


def tight_relax(shape, method="redblack"):
    """(rc, status, iterations, x) of the oracle's RB-SOR or Jacobi at TIGHT
    from inputs(shape) with the compatible right-hand side."""
    return _relax(tuple(shape), method, "compatible")


def jacobi_limit(shape):
    """... of oracle_jacobi_solve run LIMIT_ITERATIONS iterations on the
    incompatible right-hand side (it ends MAX_ITER; its demeaned iterates
    converge, their mean drifts)."""
    return _relax(tuple(shape), "jacobi", "incompatible")


def oracle_initial_residual(x0, rhs, d):
    """solve_common's initial residual of x0 (linear_solver.c:397-485): the
    oracle's RB-SOR stopped before its first iteration."""
    x = np.array(x0)
    st = oracle.redblack_solve(x, np.ascontiguousarray(rhs), *d,
                               oracle.poisson_params(max_iterations=0))[1]
    return st.initial_residual


# ---------------------------------------------------------------------------
# the whole step: fields whose pressure problem is compatible
# ---------------------------------------------------------------------------
STEP_SHAPES = [(20, 14, 11), (23, 19, 1), (35, 67, 21)]
STEP_DT, STEP_NU = 1e-4, 0.01
STEP_TOL = 1e-12
STEP_PARAMS = dict(tolerance=STEP_TOL, absolute_tolerance=1e-300, max_iterations=20000)


def step_fields(shape, fill=False):
    """u, v, w random, zero on the boundary and (unless fill) on the three
    outermost interior layers: the predictor's stencil then leaves u* zero on
    the two outermost layers, the central-difference divergence telescopes to
    zero over the interior, and the pressure problem is compatible. p random."""
    nx, ny, nz = shape
    rng = np.random.default_rng(4242 + 31 * nx + 7 * ny + nz)
    f = {k: 0.1 * rng.standard_normal((nz, ny, nx)) for k in ("u", "v", "w", "p")}
    m = 1 if fill else 4
    keep = np.zeros((nz, ny, nx), bool)
    keep[(slice(m, -m) if nz > 1 else slice(None)), m:-m, m:-m] = True
    for k in ("u", "v", "w"):
        f[k][~keep] = 0.0
    if nz == 1:
        f["w"][...] = 0.0
    return f


def grid_field(shape, fields):
    """(Grid, FlowField, params) of a step on the spacing() box."""
    from cfd_amd import api
    nx, ny, nz = shape
    g = api.Grid(nx, ny, nz, 0.0, D.BOX[0], 0.0, D.BOX[1], 0.0, D.BOX[2] if nz > 1 else 0.0)
    f = api.FlowField(nx, ny, nz)
    for k, v in fields.items():
        getattr(f, k)[...] = v
    f.rho[...] = 1.0
    f.T[...] = 300.0
    return g, f, api.validation_params(STEP_DT, STEP_NU)


# The incompatible step: the lid-driven cavity's boundary values around
# velocities that fill the interior, in 2-D.
CAVITY_SHAPE = (23, 19, 1)


def cavity_fields():
    from cfd_amd import api
    g, f, _ = grid_field(CAVITY_SHAPE, step_fields(CAVITY_SHAPE, fill=True))
    api.cavity_bc(f, 1.0)
    return {k: np.array(getattr(f, k)) for k in ("u", "v", "w", "p")}


@functools.lru_cache(maxsize=None)
def cavity_rhs():
    """The right-hand side the projection step forms from cavity_fields(),
    from the oracle alone: its RB-SOR step told to stop after one iteration
    (tolerance 1e30) still runs the corrector, so u* = u_new + (dt / rho)
    grad p_new on the interior (central differences, as the corrector) and
    rhs = (rho / dt) div u* (central differences). rho = 1."""
    g, f, prm = grid_field(CAVITY_SHAPE, cavity_fields())
    oracle.set_projection_poisson_params(
        oracle.poisson_params(tolerance=1e30, absolute_tolerance=1e-300, max_iterations=10))
    try:
        s, _, _ = oracle.projection_step(f, g, prm, A.ORACLE_POISSON_REDBLACK)
    finally:
        oracle.set_projection_poisson_params(None)
    assert s == A.CFD_SUCCESS
    res0 = oracle.last_poisson_stats().initial_residual
    dx, dy, _ = spacing(CAVITY_SHAPE)
    u, v, p = f.u[0], f.v[0], f.p[0]
    us, vs = u.copy(), v.copy()
    us[1:-1, 1:-1] += STEP_DT * (p[1:-1, 2:] - p[1:-1, :-2]) / (2 * dx)
    vs[1:-1, 1:-1] += STEP_DT * (p[2:, 1:-1] - p[:-2, 1:-1]) / (2 * dy)
    rhs = np.zeros_like(np.array(f.p))
    rhs[0, 1:-1, 1:-1] = ((us[1:-1, 2:] - us[1:-1, :-2]) / (2 * dx) +
                          (vs[2:, 1:-1] - vs[:-2, 1:-1]) / (2 * dy)) / STEP_DT
    rhs.setflags(write=False)
    return rhs, res0
