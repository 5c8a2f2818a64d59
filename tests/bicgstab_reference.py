"""TEST INFRASTRUCTURE ONLY -- the reference's BiCGSTAB loop
(linear_solver_bicgstab.c:265-495) restated in numpy long double, the
high-precision reference of test_bicgstab_reference.py (CPU, against the
fixtures the reference's own C solver produced) and test_gpu_bicgstab.py.

The problem is cg_reference.py's: A = -(7-point Laplacian) on the interior
(5-point when nz = 1) with the spacing factors 1 / (dx dx), 1 / (dy dy),
1 / (dz dz) each rounded to double once, zero walls for r, r^, p, v, s, t,
r_0 = -rhs + lap(x_0), r^ = r_0, rho = alpha = omega = 1, p = v = 0,
tolerance = max(rel ||r_0||, abs). `shell` is "neumann" (the default boundary
copy on x at solve start and, on the exits that reach it, at the end) or
"keep" (leave the caller's boundary: an apply_bc override that writes nothing).

The seven exits, numbered as the loop meets them:
  1 converged at start   ||r_0|| < abs: CONVERGED, 0 iterations, no closing copy
  2 rho / (r^, v) breakdown   STAGNATED, iter + 1, the previous res_norm, no copy
  3 converged on s       tested every iteration; x += alpha p only; closing copy
  4 (t, t) breakdown     x += alpha p; STAGNATED, ||s||, no copy
  5 converged on r       tested when iter % check_interval == 0; closing copy
  6 omega breakdown      STAGNATED after the full update, no copy
  7 loop exhausted       one last test of res_norm; iterations = max_iterations
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from tests.cg_reference import LD, _require_extended, interior, laplacian, neumann_shell

CFD_SUCCESS = 0
CFD_ERROR_MAX_ITER = -7
ST_CONVERGED, ST_MAX_ITER, ST_STAGNATED = 0, 1, 3
BREAKDOWN = 1e-30

EXIT_START, EXIT_RHO, EXIT_S, EXIT_TT, EXIT_R, EXIT_OMEGA, EXIT_EXHAUSTED = range(1, 8)


class BcgResult(NamedTuple):
    x: np.ndarray            # the solver's x, shell included, in the run's dtype
    tested: list             # [("s" | "r" | "end", iteration counted from 1, norm)], in order
    exit: int                # 1 .. 7, see the module docstring
    status: int              # poisson_solver_status_t
    rc: int                  # CFD_SUCCESS or CFD_ERROR_MAX_ITER
    iterations: int
    initial_residual: float
    final_residual: float
    moved: float             # max |x - x_0| (x_0 after the opening shell), the scale of the bar


def bicgstab_reference(x0, rhs, dx, dy, dz, tolerance=1e-6, absolute_tolerance=1e-10,
                       max_iterations=5000, check_interval=1, shell="neumann",
                       dtype=LD) -> BcgResult:
    if dtype is LD:
        _require_extended()
    assert shell in ("neumann", "keep")
    x = np.array(x0, dtype=dtype)
    b = np.array(rhs, dtype=dtype)

    def bc(a):
        if shell == "neumann":
            neumann_shell(a)

    bc(x)
    xs = x.copy()
    inn = interior(x.shape)

    def A(f):  # zero walls: f is a full array, the product lives on the interior
        return -laplacian(f, dx, dy, dz)

    def full(v):
        f = np.zeros_like(x)
        f[inn] = v
        return f

    r = -b[inn] + laplacian(x, dx, dy, dz)
    rh = r.copy()
    rho = alpha = omega = dtype(1.0)
    p = np.zeros_like(r)
    v = np.zeros_like(r)
    res0 = np.sqrt(np.sum(r * r))
    tol = dtype(tolerance) * res0
    if tol < absolute_tolerance:
        tol = dtype(absolute_tolerance)
    tested = []

    def done(exit_, status, iters, res, closing):
        if closing:
            bc(x)
        rc = CFD_SUCCESS if status == ST_CONVERGED else CFD_ERROR_MAX_ITER
        return BcgResult(x, tested, exit_, status, rc, iters, float(res0), float(res),
                         float(np.max(np.abs(x - xs))))

    def met(n):
        return bool(n < tol or n < absolute_tolerance)

    if res0 < absolute_tolerance:
        return done(EXIT_START, ST_CONVERGED, 0, res0, False)
    res = res0
    converged = False
    exit_ = EXIT_EXHAUSTED
    it = 0
    while it < max_iterations:
        rho_new = np.sum(rh * r)
        if abs(rho_new) < BREAKDOWN:
            return done(EXIT_RHO, ST_STAGNATED, it + 1, res, False)
        beta = (rho_new / rho) * (alpha / omega)
        p = r + beta * (p - omega * v)
        v = A(full(p))
        rhv = np.sum(rh * v)
        if abs(rhv) < BREAKDOWN:
            return done(EXIT_RHO, ST_STAGNATED, it + 1, res, False)
        alpha = rho_new / rhv
        s = r - alpha * v
        s_norm = np.sqrt(np.sum(s * s))
        tested.append(("s", it + 1, float(s_norm)))
        if met(s_norm):
            x[inn] += alpha * p
            res = s_norm
            converged, exit_ = True, EXIT_S
            break
        t = A(full(s))
        ts = np.sum(t * s)
        tt = np.sum(t * t)
        if abs(tt) < BREAKDOWN:
            x[inn] += alpha * p
            return done(EXIT_TT, ST_STAGNATED, it + 1, s_norm, False)
        omega = ts / tt
        x[inn] += alpha * p + omega * s
        r = s - omega * t
        rho = rho_new
        res = np.sqrt(np.sum(r * r))
        if it % check_interval == 0:
            tested.append(("r", it + 1, float(res)))
            if met(res):
                converged, exit_ = True, EXIT_R
                break
        if abs(omega) < BREAKDOWN:
            return done(EXIT_OMEGA, ST_STAGNATED, it + 1, res, False)
        it += 1
    if not converged:
        tested.append(("end", it, float(res)))
        converged = met(res)
    iters = it + 1 if it < max_iterations else it
    return done(exit_, ST_CONVERGED if converged else ST_MAX_ITER, iters, res, True)


def stop_margin(res: BcgResult):
    """(norm that stopped the solve, smallest norm tested before it), or None
    for a solve that met no tolerance."""
    if res.status != ST_CONVERGED or res.exit == EXIT_START or len(res.tested) < 2:
        return None
    norms = [n for _, _, n in res.tested]
    return norms[-1], min(norms[:-1])
