"""Shapes, inputs and the numpy float64 model of the direct sine-transform
pressure solve (HIP_POISSON_DST, cfd_amd/csrc/hip/transform_solve.hpp), shared by
tests/test_dst_cases.py (the model against the oracle's CG, on the CPU) and
tests/test_gpu_dst.py (the device against both).

The algorithm: inside a solve the reference's CG writes the boundary cells of
x only before and after its loop, so the interior system is the 7-point
Laplacian with Dirichlet data frozen from the start BC. With S_n[a][b] =
sin(pi (a+1)(b+1) / (n+1)) and lambda_n[a] = 4 sin^2(pi (a+1) / (2 (n+1))) / h^2
on each axis,
    b  = -rhs + (boundary neighbours of the frozen shell) / h^2
    x  = S_x S_y S_z [ prod 2/(n+1) / (lx[i] + ly[j] + lz[k]) * S_z S_y S_x b ].

The kernels work on 16 x 16 x 4 matrix tiles (64 output rows per wave along a
strided axis; 32 lines x 256 columns per workgroup, staged in 64-column chunks,
along x), so the interior extents n = size - 2 are chosen for those edges.
"""
from __future__ import annotations

import functools

import numpy as np

from cfd_amd import _abi as A
from oracle import oracle

# (nx, ny, nz) -> what the shape reaches (n = interior extent per axis)
SHAPES = {
    (3, 3, 1): "n = 1 on both axes, 2-D: every tile all tail",
    (3, 3, 3): "n = 1 on all three axes",
    (5, 4, 1): "n = 3, 2: below one k step of 4 (n = 3 mod 16)",
    (12, 9, 6): "n = 10, 7, 4: below one 16-row tile, n = 4 one exact k step",
    (17, 18, 1): "n = 15, 16: 15 mod 16 and the exact 16 tile (0 mod 16)",
    (23, 19, 1): "2-D, n = 21, 17: 1 mod 16 on y, a k tail of 1",
    (67, 35, 1): "2-D, row pitch 128: n = 65 along x (two 64-column chunks, two groups of "
                 "column tiles), n = 33 along y (two 32-line tiles of the x pass)",
    (261, 5, 1): "n = 259 (3 mod 16): two 256-column tiles of the x pass, the second with "
                 "one active wave; five 64-column chunks",
    (20, 14, 11): "3-D, n = 18, 12, 9",
    (67, 35, 18): "3-D, row pitch 128, n = 65, 33, 16",
    (35, 67, 21): "3-D, n = 33, 65, 19: two 64-row tiles along y, 3 mod 16 along z",
    (34, 34, 34): "n = 32 on all three axes: exact tiles, no tail anywhere",
}
SHAPE_LIST = list(SHAPES)

# Largest deviation of the model below from the oracle's CG run to 1e-13
# (test_dst_cases.test_model_matches_tight_cg prints it), relative to max |x|,
# times 100: the margin the BiCGSTAB pin used for a changed summation order.
# Measured 5.57e-12 (34 x 34 x 34, Neumann; Dirichlet hook: 2.9e-12 on
# 67 x 35 x 18); DESIGN.md, the direct sine-transform solve.
DST_BAR = 5.6e-10

BOX = (0.9, 1.3, 0.7)  # dx != dy != dz

TIGHT = dict(tolerance=1e-13, absolute_tolerance=1e-300, max_iterations=20000)
# left + right != top + bottom: with one interior cell per axis a boundary term
# scaled by the wrong axis spacing would otherwise cancel
DIRICHLET = dict(left=0.3, right=-0.2, top=0.5, bottom=-0.15, front=0.1, back=0.25)


def sid(shape):
    return "x".join(str(v) for v in shape)


def spacing(shape):
    nx, ny, nz = shape
    return (BOX[0] / (nx - 1), BOX[1] / (ny - 1), BOX[2] / (nz - 1) if nz > 1 else 0.0)


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    nx, ny, nz = shape
    rng = np.random.default_rng(1000003 * nx + 1009 * ny + nz)
    rhs = rng.standard_normal((nz, ny, nx))
    x0 = 0.1 * rng.standard_normal((nz, ny, nx))
    rhs.setflags(write=False)
    x0.setflags(write=False)
    return rhs, x0


def inputs(shape):
    """(rhs, x0) on the whole (nz, ny, nx) array, shell included; read-only."""
    return _inputs(tuple(shape))


def interior(shape3):
    nz = shape3[0]
    return (slice(1, -1) if nz > 1 else slice(None), slice(1, -1), slice(1, -1))


def shell_mask(shape3):
    m = np.ones(shape3, bool)
    m[interior(shape3)] = False
    return m


def dirichlet_values():
    return A.DirichletValues(**DIRICHLET)


def dirichlet_bc(a):
    """An apply_bc override: fixed face values (bc_apply_dirichlet_scalar_3d)."""
    oracle.bc_dirichlet(a, dirichlet_values())


def bc_hook(fn):
    """fn(array view) as an oracle_set_poisson_bc_hook callback."""
    def cb(ptr, nx, ny, nz, _ctx):
        fn(np.ctypeslib.as_array(ptr, shape=(nz * ny * nx,)).reshape(nz, ny, nx))
    return oracle.BC_HOOK(cb)


# ---------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------
_PI_L = np.longdouble(4) * np.arctan(np.longdouble(1))


def sine_matrix_ld(n):
    """S_n in long double, the argument reduced as an integer first."""
    a = np.arange(1, n + 1, dtype=np.int64)
    m = np.outer(a, a) % (2 * (n + 1))
    return np.sin(_PI_L * m.astype(np.longdouble) / np.longdouble(n + 1))


@functools.lru_cache(maxsize=None)
def sine_matrix(n):
    """S_n rounded once to double."""
    return sine_matrix_ld(n).astype(np.float64)


def eigenvalues(n, h):
    a = np.arange(1, n + 1).astype(np.longdouble)
    s = np.sin(_PI_L * a / np.longdouble(2 * (n + 1)))
    return (4 * s * s).astype(np.float64) / (h * h)


def transform(a, axis, S=None):
    """Unnormalised DST-I of the interior of `a` (nz, ny, nx) along axis
    0 (x), 1 (y), 2 (z); the boundary is left as it is."""
    out = a.copy()
    inn = interior(a.shape)
    ax = 2 - axis
    v = a[inn]
    S = sine_matrix(v.shape[ax]) if S is None else S
    out[inn] = np.moveaxis(np.tensordot(S, v, axes=([1], [ax])), 0, ax)
    return out


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------
class Result:
    def __init__(self, rc, status, iterations, res0, res, x):
        self.rc, self.status, self.iterations = rc, status, iterations
        self.initial_residual, self.final_residual, self.x = res0, res, x


def _residual(x, rhs, d):
    """r = -rhs + lap(x) on the interior (linear_solver_cg.c:134-158) and its 2-norm."""
    nz = x.shape[0]
    inn = interior(x.shape)
    c = x[inn]
    if nz > 1:
        lap = ((x[1:-1, 1:-1, 2:] - 2.0 * c + x[1:-1, 1:-1, :-2]) / (d[0] * d[0]) +
               (x[1:-1, 2:, 1:-1] - 2.0 * c + x[1:-1, :-2, 1:-1]) / (d[1] * d[1]) +
               (x[2:, 1:-1, 1:-1] + x[:-2, 1:-1, 1:-1] - 2.0 * c) / (d[2] * d[2]))
    else:
        lap = ((x[:, 1:-1, 2:] - 2.0 * c + x[:, 1:-1, :-2]) / (d[0] * d[0]) +
               (x[:, 2:, 1:-1] - 2.0 * c + x[:, :-2, 1:-1]) / (d[1] * d[1]))
    r = -rhs[inn] + lap
    return float(np.sqrt(np.sum(r * r)))


def model_solve(x0, rhs, d, tolerance=1e-6, absolute_tolerance=1e-10, bc=None, *,
                bnd_sign=1.0, swap_h=False, norm_scale=1.0):
    """The solve of the module docstring in numpy float64. bc: None = the
    default Neumann apply_bc, else a function applied to x in place at the
    start and the end (a no-op function: the boundary kept). The three
    keyword switches plant the bugs the tests must be able to see: the sign
    of the boundary term, its 1/h^2 taken from another axis, the
    normalisation."""
    apply_bc = oracle.poisson_apply_bc if bc is None else bc
    x = np.ascontiguousarray(x0, dtype=np.float64).copy()
    nz = x.shape[0]
    is3d = nz > 1
    apply_bc(x)
    res0 = _residual(x, rhs, d)
    tol = max(tolerance * res0, absolute_tolerance)
    if res0 < absolute_tolerance:
        return Result(A.CFD_SUCCESS, A.POISSON_CONVERGED, 0, res0, res0, x)
    inn = interior(x.shape)
    h2 = [d[0] * d[0], d[1] * d[1], d[2] * d[2] if is3d else 0.0]
    if swap_h:
        h2 = [h2[1], h2[0], h2[2]]
    b = -rhs[inn].copy()
    kk = slice(1, -1) if is3d else slice(None)
    b[:, :, 0] += bnd_sign * x[kk, 1:-1, 0] / h2[0]
    b[:, :, -1] += bnd_sign * x[kk, 1:-1, -1] / h2[0]
    b[:, 0, :] += bnd_sign * x[kk, 0, 1:-1] / h2[1]
    b[:, -1, :] += bnd_sign * x[kk, -1, 1:-1] / h2[1]
    if is3d:
        b[0, :, :] += bnd_sign * x[0, 1:-1, 1:-1] / h2[2]
        b[-1, :, :] += bnd_sign * x[-1, 1:-1, 1:-1] / h2[2]
    n = b.shape
    axes = [2, 1] + ([0] if is3d else [])  # x, y, z as array axes
    t = b
    for ax in axes:
        t = np.moveaxis(np.tensordot(sine_matrix(n[ax]), t, axes=([1], [ax])), 0, ax)
    lam = (eigenvalues(n[2], d[0])[None, None, :] + eigenvalues(n[1], d[1])[None, :, None])
    norm = (2.0 / (n[2] + 1)) * (2.0 / (n[1] + 1))
    if is3d:
        lam = lam + eigenvalues(n[0], d[2])[:, None, None]
        norm *= 2.0 / (n[0] + 1)
    t = t * (norm * norm_scale / lam)
    for ax in reversed(axes):
        t = np.moveaxis(np.tensordot(sine_matrix(n[ax]), t, axes=([1], [ax])), 0, ax)
    x[inn] = t
    res = _residual(x, rhs, d)
    conv = res < tol or res < absolute_tolerance
    apply_bc(x)
    return Result(A.CFD_SUCCESS if conv else A.CFD_ERROR_MAX_ITER,
                  A.POISSON_CONVERGED if conv else A.POISSON_MAX_ITER, 1, res0, res, x)


# ---------------------------------------------------------------------------
# the oracle's CG at the tight settings, once per (shape, bc)
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tight_cg(shape, bc):
    rhs, x0 = inputs(shape)
    x = x0.copy()
    hook = None
    if bc == "dirichlet":
        hook = bc_hook(dirichlet_bc)
    elif bc == "keep":
        hook = bc_hook(lambda a: None)
    if hook is not None:
        oracle.lib().oracle_set_poisson_bc_hook(hook, None)
    try:
        s, st = oracle.cg_solve(x, np.ascontiguousarray(rhs), *spacing(shape),
                                oracle.poisson_params(**TIGHT))
    finally:
        if hook is not None:
            oracle.lib().oracle_set_poisson_bc_hook(oracle.BC_HOOK(0), None)
    x.setflags(write=False)
    return s, st.status, st.iterations, x


def tight_cg(shape, bc="neumann"):
    """(rc, status, iterations, x) of oracle_cg_solve at TIGHT from inputs(shape);
    bc: "neumann" (the default apply_bc), "dirichlet" (the hook writing
    DIRICHLET) or "keep" (a hook that leaves the boundary alone)."""
    return _tight_cg(tuple(shape), bc)


def rel_dev(x, ref):
    return float(np.max(np.abs(x - ref))) / float(np.max(np.abs(ref)))
