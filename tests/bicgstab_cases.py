"""TEST INFRASTRUCTURE ONLY -- the BiCGSTAB case table shared by
tests/golden/make_bicgstab_golden.py (the reference's own C solver),
test_bicgstab_reference.py (CPU) and test_gpu_bicgstab.py.

Problems come from cg_seam_shapes.problem(shape) on the 1.0 x 0.7 x 1.3 box
(rhs ~ N(0, 1), x0 = 0.1 N(0, 1)); the degenerate cases take rhs = 0 and a
constant x0 instead.

Converged cases: at tolerance 1e-6 these problems need 60-110 iterations, and
fp64 and long double then stop one iteration apart. So every converged case
stops within three iterations, on a tolerance chosen from the long-double
run: the relative tolerance is the geometric mean of the norm that stops the
solve and the smallest norm tested before it, which differ by a factor of at
least 1.5 (test_bicgstab_reference.py asserts both).
"""
from __future__ import annotations

import functools

import numpy as np

from tests import bicgstab_reference as B
from tests import cg_seam_shapes as T

CAP_ITERS = (1, 2, 5)   # the rho = alpha = omega = 1 start, the first real beta and
#                         omega, both parities of the p / v double buffer
MIN_FACTOR = 1.5
# max |x - x_ref| <= BAR * max |x_ref - x0|, and each residual norm relative:
# 100 x the largest deviation of the reference's own fp64 results (the
# fixtures) from the long-double restatement, rounded up to a power of ten
# (test_bicgstab_reference.test_the_bar holds it to that rule)
BAR = 1e-11
DEFAULT_MAX_ITER = 5000
DEFAULT_ABS = 1e-10
CONST_X0 = 0.75
DEGENERATE_SHAPE = (17, 13, 11)


def cap_iters_for(shape):
    """CAP_ITERS under cg_seam_shapes.iters_for's rule: below the number of
    interior cells (2 x 2 x 1 on the smallest grid)."""
    nx, ny, nz = shape
    n = (nx - 2) * (ny - 2) * max(nz - 2, 1)
    return tuple(it for it in CAP_ITERS if it < n)


def _case(name, shape, kind, tolerance, absolute_tolerance=DEFAULT_ABS,
          max_iterations=DEFAULT_MAX_ITER, check_interval=1, kchunk=0, expect=None):
    return dict(name=name, shape=tuple(shape), kind=kind, tolerance=tolerance,
                absolute_tolerance=absolute_tolerance, max_iterations=max_iterations,
                check_interval=check_interval, kchunk=kchunk, expect=expect)


def _capped():
    out = []
    shapes = [(s, 0) for s, _ in T.TEXTBOOK] + [(s, k) for s, k, _ in T.TEXTBOOK_KCHUNK]
    shapes += [((4, 4, 3), 0), ((5, 4, 3), 0)]
    for shape, kchunk in shapes:
        for it in cap_iters_for(shape):
            tag = f"cap-{T.sid(shape)}" + (f"-kc{kchunk}" if kchunk else "") + f"-it{it}"
            # capped_params: no tolerance a residual could meet
            out.append(_case(tag, shape, "capped", 1e-30, 0.0, it, 1, kchunk,
                             expect=(B.EXIT_EXHAUSTED, it)))
    return out


# (shape, relative tolerance, exit, iteration): the issue's table
CONVERGED = [
    ((62, 30, 27), 2.730e-2, B.EXIT_S, 3),
    ((130, 18, 7), 3.057e-2, B.EXIT_S, 3),
    ((17, 13, 11), 3.980e-2, B.EXIT_R, 2),
    ((61, 29, 51), 4.058e-2, B.EXIT_R, 2),
    ((130, 18, 7), 1.513e-1, B.EXIT_R, 1),
]
CI_SHAPE, CI_TOL = (17, 13, 11), 3.980e-2

CASES = _capped()
CASES += [_case(f"conv-{T.sid(s)}-{tol:.3e}", s, "converged", tol, expect=(ex, it))
          for s, tol, ex, it in CONVERGED]
CASES += [
    _case("ci1", CI_SHAPE, "check_interval", CI_TOL, check_interval=1, expect=(B.EXIT_R, 2)),
    # r_2 is not tested; s_3 / tolerance = 0.47
    _case("ci4", CI_SHAPE, "check_interval", CI_TOL, check_interval=4, expect=(B.EXIT_S, 3)),
    # the loop-exhausted check: CONVERGED with 2 iterations
    _case("ci4-max2", CI_SHAPE, "check_interval", CI_TOL, check_interval=4, max_iterations=2,
          expect=(B.EXIT_EXHAUSTED, 2)),
    # rhs = 0, constant x0: r_0 = 0
    _case("degen-start", DEGENERATE_SHAPE, "degenerate", 1e-6, expect=(B.EXIT_START, 0)),
    _case("degen-rho", DEGENERATE_SHAPE, "degenerate", 1e-6, absolute_tolerance=0.0,
          expect=(B.EXIT_RHO, 1)),
]
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)

NPZ_MAX_CELLS = 10_000
JSON_FILE = "bicgstab_cases.json"
NPZ_FILE = "bicgstab_x.npz"


def inputs(case):
    """(rhs, x0), read-only, of a case."""
    if case["kind"] == "degenerate":
        nx, ny, nz = case["shape"]
        rhs = np.zeros((nz, ny, nx))
        x0 = np.full((nz, ny, nx), CONST_X0)
        rhs.setflags(write=False)
        x0.setflags(write=False)
        return rhs, x0
    return T.problem(case["shape"])


def solver_params(case):
    return dict(tolerance=case["tolerance"], absolute_tolerance=case["absolute_tolerance"],
                max_iterations=case["max_iterations"], check_interval=case["check_interval"])


@functools.lru_cache(maxsize=None)
def reference(name, shell="neumann"):
    """The long-double restatement of a case, computed once per process."""
    case = BY_NAME[name]
    rhs, x0 = inputs(case)
    res = B.bicgstab_reference(x0, rhs, *T.spacing(case["shape"]), shell=shell,
                               **solver_params(case))
    res.x.setflags(write=False)
    return res


def in_npz(case):
    nx, ny, nz = case["shape"]
    return nx * ny * nz <= NPZ_MAX_CELLS


def deviation(x, initial_residual, final_residual, ref):
    """(x, initial residual, final residual) deviations of a result from the
    long-double reference `ref`, in the units of the bar: max |x - x_ref| /
    max |x_ref - x0| and the norms' relative differences (absolute where the
    reference norm or the movement is 0: the degenerate cases)."""
    dx = float(np.max(np.abs(np.asarray(x, dtype=B.LD) - ref.x)))
    if ref.moved > 0.0:
        dx /= ref.moved
    out = [dx]
    for got, want in ((initial_residual, ref.initial_residual),
                      (final_residual, ref.final_residual)):
        out.append(abs(got - want) / want if want > 0.0 else abs(got - want))
    return tuple(out)
