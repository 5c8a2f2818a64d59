"""Case table and seeded inputs of the explicit Euler / RK2 fixtures
(tests/golden/euler_rk2_cases.json). tests/golden/make_rk_golden.py runs the
reference's own CPU solvers on these inputs and records the outputs; the
tests rebuild the same inputs and compare the device result with the record.

Shapes are test_gpu_rk4.py's seam list (k_euler_step tiles the grid exactly
as k_rk_stage2 does, 128 columns x 4 rows of x pairs): nx = 130 / 131 put the
pair that holds column nx - 2 on lane 0 / 1 of the second tile, ny = 3 and
nz = 3 leave one interior row / plane, (20, 18, 1) is 2-D (stride_z = 0).

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
       guard=False, rk_dt=None, rk_steps=None):
    return dict(name=name, shape=shape, buoy=buoy, energy=energy, pattern=pattern, dt=dt,
                steps=steps, seed=seed, guard=guard, rk_dt=dt if rk_dt is None else rk_dt,
                rk_steps=steps if rk_steps is None else rk_steps)


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
]
BY_NAME = {c["name"]: c for c in CASES}
NPZ_CASE = "s17"  # full output fields are kept for this case


def case_dt(case, integrator):
    return case["dt"] if integrator == "euler" else case["rk_dt"]


def case_steps(case, integrator):
    return case["steps"] if integrator == "euler" else case["rk_steps"]


def make_inputs(case):
    """(grid, field, params) of a case; params.dt / max_iter are set by params_for."""
    nx, ny, nz = case["shape"]
    g = api.Grid(nx, ny, nz, 0.0, 1.0, 0.0, 1.0, 0.0, 1.0 if nz > 1 else 0.0)
    f = api.FlowField(nx, ny, nz)
    rng = np.random.default_rng(case["seed"])
    for k in ("u", "v", "w"):
        getattr(f, k)[...] = 0.05 * rng.standard_normal(f.u.shape)
    if nz == 1:
        f.w[...] = 0.0
    if case["guard"]:
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
        p.alpha = 1e-3
        tb = p.thermal_bc
        tb.left = tb.right = A.BC_TYPE_DIRICHLET
        tb.bottom = tb.top = A.BC_TYPE_NEUMANN
        tb.back = tb.front = A.BC_TYPE_PERIODIC
        tb.dirichlet_values.left = 301.0
        tb.dirichlet_values.right = 299.0
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
