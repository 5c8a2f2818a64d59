"""Case table and seeded inputs of the explicit Euler / RK2 fixtures
(tests/golden/euler_rk2_cases.json). tests/golden/make_rk_golden.py runs the
reference's own CPU solvers on these inputs and records the outputs; the
tests rebuild the same inputs and compare the device result with the record.

Shapes are test_gpu_rk4.py's seam list (k_euler_step tiles the grid exactly
as k_rk_stage2 does, 128 columns x 4 rows of x pairs): nx = 130 / 131 put the
pair that holds column nx - 2 on lane 0 / 1 of the second tile, ny = 3 and
nz = 3 leave one interior row / plane, (20, 18, 1) is 2-D (stride_z = 0).

The st* / it* cases repeat those shapes on a grid stretched in x and y
(stretch_grid): all three kernels read dx[i] and dy[j] per index, and on a
uniform grid a wrong index reads the right value. x clusters mid-domain and
y at the walls, so no two neighbouring entries are equal and an x / y
exchange shows; their noise amplitude follows the smallest spacing, so that
the RHS's derivative clamps do not hide the spacing. stzero17 collapses two
columns and a row onto their neighbours: the |dx[i]|, |dy[j]| < 1e-10 skip.

Call patterns: "steps" is `steps` calls of one step each (source index 0
every time: hip_*_step); "iter" is one call with max_iter = steps and
source_decay_rate = 0.5, so that the source index matters
(solve_*_method_gpu and the _iter_internal loops).
"""
from __future__ import annotations

import hashlib

import numpy as np

from cfd_amd import _abi as A
from cfd_amd import api

FIELDS = ("u", "v", "w", "p", "rho", "T")
INTEGRATORS = ("euler", "rk2", "rk4")
ITER_DECAY = 0.5


def _c(name, shape, buoy=False, energy=False, pattern="steps", dt=1e-4, steps=4, seed=5,
       guard=False, rk_dt=None, rk_steps=None, stretch=False, zero=False):
    return dict(name=name, shape=shape, buoy=buoy, energy=energy, pattern=pattern, dt=dt,
                steps=steps, seed=seed, guard=guard, rk_dt=dt if rk_dt is None else rk_dt,
                rk_steps=steps if rk_steps is None else rk_steps, stretch=stretch, zero=zero)


# dt = 5e-4 is above explicit Euler's 1e-4 cap (conservative_dt), 1e-4 is at it
CASES = [
    _c("s17", (17, 13, 11)),
    _c("s17_be", (17, 13, 11), buoy=True, energy=True, dt=5e-4),
    _c("s20_2d_b", (20, 18, 1), buoy=True),
    _c("s130", (130, 19, 9)),
    _c("s131_b", (131, 3, 7), buoy=True, dt=5e-4),
    _c("s9", (9, 17, 3)),
    _c("s257_be", (257, 21, 5), buoy=True, energy=True),
    _c("i17_be", (17, 13, 11), buoy=True, energy=True, pattern="iter", dt=5e-4, seed=6),
    _c("i20_2d", (20, 18, 1), pattern="iter", seed=6),
    _c("i130_b", (130, 19, 9), buoy=True, pattern="iter", seed=6),
    # the guards: +-1 increment clamp (large pressure gradient over rho = 1e-3)
    # and the rho <= 1e-10 skip; RK2 / RK4 run it at dt = 1e-4 for 3 steps
    _c("guard17", (17, 13, 11), dt=5e-4, seed=11, guard=True, rk_dt=1e-4, rk_steps=3),
    # stretched x / y (stretch_grid below): dx[i], dy[j] differ from index to
    # index, so which entry a cell reads shows in its result. The energy
    # equation refuses such a grid, so none of these has it on.
    _c("st17", (17, 13, 11), stretch=True),
    _c("st17_b", (17, 13, 11), buoy=True, dt=5e-4, stretch=True),
    _c("st20_2d_b", (20, 18, 1), buoy=True, stretch=True),
    _c("st130", (130, 19, 9), stretch=True),
    _c("st131_b", (131, 3, 7), buoy=True, stretch=True),
    _c("st9", (9, 17, 3), stretch=True),
    _c("st257_b", (257, 21, 5), buoy=True, stretch=True),
    _c("it17_b", (17, 13, 11), buoy=True, pattern="iter", dt=5e-4, seed=6, stretch=True),
    _c("it130", (130, 19, 9), pattern="iter", seed=6, stretch=True),
    # the |dx[i]| < 1e-10 / |dy[j]| < 1e-10 skip: dx[5] = 0 (odd column, the b
    # cell of its pair), dx[10] = 5e-11 (even column, the a cell), dy[3] = 0
    _c("stzero17", (17, 13, 11), stretch=True, zero=True),
]
BY_NAME = {c["name"]: c for c in CASES}
# full output fields are kept for these cases
NPZ_FILES = {"s17": "euler_rk2_17x13x11.npz", "st17": "euler_rk2_st17x13x11.npz"}
STRETCH_AX, STRETCH_AY = 1.2, -0.7
ZERO_COLS, ZERO_ROWS = (5, 10), (3,)  # stzero17's skipped interior columns / rows


def case_dt(case, integrator):
    return case["dt"] if integrator == "euler" else case["rk_dt"]


def case_steps(case, integrator):
    return case["steps"] if integrator == "euler" else case["rk_steps"]


def stretch_coords(n, lo, hi, a):
    """lo + (hi - lo) (xi - a xi (1 - xi) (2 xi - 1)), xi = i / (n - 1): monotone
    for -1 < a < 2, clustered mid-domain for a > 0 and at the ends for a < 0.
    Only + - * /, each correctly rounded: the same bytes on any numpy."""
    xi = np.arange(n, dtype=np.float64) / np.float64(n - 1)
    return lo + (hi - lo) * (xi - a * xi * (1.0 - xi) * (2.0 * xi - 1.0))


def set_axis(g, axis, v):
    """Write coordinates v and the n - 1 spacings v[i + 1] - v[i] of one axis
    ("x" / "y") straight into the grid's C arrays."""
    c = g.c
    arr, darr = getattr(c, axis), getattr(c, "d" + axis)
    v = np.asarray(v, dtype=np.float64)
    for i in range(len(v)):
        arr[i] = v[i]
    for i in range(len(v) - 1):
        darr[i] = v[i + 1] - v[i]


def grid_arrays(g):
    """x[nx], y[ny], dx[nx - 1], dy[ny - 1] of a grid as numpy copies."""
    c = g.c
    return {"x": np.array(c.x[:g.nx]), "y": np.array(c.y[:g.ny]),
            "dx": np.array(c.dx[:g.nx - 1]), "dy": np.array(c.dy[:g.ny - 1])}


def stretch_grid(g, zero=False):
    """Stretched x (a = 1.2) and y (a = -0.7) on a uniform grid; z stays
    uniform (the reference rejects anything else). Returns the smallest
    spacing of the stretched grid, before `zero` collapses three cells."""
    c = g.c
    x = stretch_coords(g.nx, c.xmin, c.xmax, STRETCH_AX)
    y = stretch_coords(g.ny, c.ymin, c.ymax, STRETCH_AY)
    dmin = min(float(np.min(np.diff(x))), float(np.min(np.diff(y))))
    if g.nz > 1:
        dmin = min(dmin, min(c.dz[k] for k in range(g.nz - 1)))
    if zero:
        x[6] = x[5]
        x[11] = x[10] + 5e-11
        y[4] = y[3]
    set_axis(g, "x", x)
    set_axis(g, "y", y)
    return dmin


def make_inputs(case):
    """(grid, field, params) of a case; params.dt / max_iter are set by params_for."""
    nx, ny, nz = case["shape"]
    g = api.Grid(nx, ny, nz, 0.0, 1.0, 0.0, 1.0, 0.0, 1.0 if nz > 1 else 0.0)
    f = api.FlowField(nx, ny, nz)
    rng = np.random.default_rng(case["seed"])
    # stretched grids: noise small enough for the +-100 / +-1000 derivative
    # clamps of the RHS not to mask the spacing (second differences ~ amp / d^2)
    amp = min(0.05, 50.0 * stretch_grid(g, case["zero"]) ** 2) if case["stretch"] else 0.05
    for k in ("u", "v", "w"):
        getattr(f, k)[...] = amp * rng.standard_normal(f.u.shape)
    if nz == 1:
        f.w[...] = 0.0
    if case["stretch"]:
        f.p[...] = 1.0 + 0.2 * amp * rng.standard_normal(f.u.shape)
        f.rho[...] = 1.0 + 0.1 * rng.random(f.u.shape)
    elif case["guard"]:
        f.p[...] = 1.0 + 10.0 * rng.standard_normal(f.u.shape)
        f.rho[...] = 1.0 + 0.1 * rng.random(f.u.shape)
        pick = rng.random(f.u.shape)
        f.rho[pick < 0.10] = 1e-3
        f.rho[pick < 0.03] = 0.0
    else:
        f.p[...] = 1.0 + 0.01 * rng.standard_normal(f.u.shape)
        f.rho[...] = 1.0 + 0.1 * rng.random(f.u.shape)
    f.T[...] = 300.0 + rng.standard_normal(f.u.shape)
    p = api.params_default()  # default source term on (amp 0.1 / 0.05)
    if case["buoy"]:
        p.beta = 3.3e-3
        p.T_ref = 300.0
        p.gravity[1] = -9.81
    if case["energy"]:
        set_energy(p)
    return g, f, p


def set_energy(p):
    """The energy equation of the *_be cases: alpha and their thermal BCs."""
    p.alpha = 1e-3
    tb = p.thermal_bc
    tb.left = tb.right = A.BC_TYPE_DIRICHLET
    tb.bottom = tb.top = A.BC_TYPE_NEUMANN
    tb.back = tb.front = A.BC_TYPE_PERIODIC
    tb.dirichlet_values.left = 301.0
    tb.dirichlet_values.right = 299.0


REFUSALS = ("stretched_xy_with_energy", "nonuniform_dz")


def refusal_inputs(which):
    """Inputs every solver of the reference refuses (the `refusals` record of
    the fixture holds the statuses): "stretched_xy_with_energy" is st17 with
    s17_be's energy equation on, "nonuniform_dz" is s17 with dz[3] *= 1.5."""
    if which == "stretched_xy_with_energy":
        g, f, p = make_inputs(BY_NAME["st17"])
        set_energy(p)
    else:
        assert which == "nonuniform_dz"
        g, f, p = make_inputs(BY_NAME["s17"])
        g.c.dz[3] *= 1.5
    p.dt = 1e-4
    p.max_iter = 1
    return g, f, p


def params_for(case, integrator, params, pattern=None):
    """Set dt, max_iter and the decay rate of one call; returns the number of calls."""
    pattern = pattern or case["pattern"]
    params.dt = case_dt(case, integrator)
    n = case_steps(case, integrator)
    if pattern == "iter":
        params.max_iter = n
        params.source_decay_rate = ITER_DECAY
        return 1
    params.max_iter = 1
    return n


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def digest(a) -> dict:
    a = np.asarray(a, dtype=np.float64)
    return {"sha256": sha(a), "sum": float(np.sum(a)), "l2": float(np.sqrt(np.sum(a * a))),
            "max": float(np.max(np.abs(a)))}
