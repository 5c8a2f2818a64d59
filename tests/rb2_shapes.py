"""TEST INFRASTRUCTURE ONLY -- the shapes of the k_rb2 interior-tile tests, the
layout each one gives the kernel, and the random problems the tests share
(test_rb2_shapes.py on the CPU, test_gpu_rb2_interior.py on the GPU).

What is restated here (cfd_amd/csrc/hip), as the independent model the GPU
tests compare the launch log with; tests/test_tile_plan.py holds layout() and
is_interior() to the product's planner without a GPU:
  tile_plan.hpp, plan_rb2 (the r2geo tiling)
      tiles of 56 x 24 written cells (RB2_OX x RB2_OY) from cell 0,
      tiles_x = (nx - 1 + 55) / 56; z runs of kc planes from plane 1: 128
      (or (nint_k + 2) / 3 on deep, wide grids), CFD_HIP_RB2_KC in its place,
      halved while kc > 4 and there are fewer than 512 workgroups unless
      CFD_HIP_RB2_KC_FIXED is set, then clamped to [1, nz - 2]
  tile_plan.hpp, rb2_tile_interior (k_rb2 spells the same test out)
      a tile loads 64 x 32 cells from (56 tx - 4, 24 ty - 4) and is interior
      (rb2_march<BND = false>) when those are columns 1 .. nx - 3 and rows
      2 .. ny - 3 at most
  rb2.hpp, rb2_march
      a run [kb, ke) takes nsteps = ke - kb + 6 steps from plane q0 = kb - 4;
      groups of four with the per-plane tests (ZB) up to step n_s, steady
      groups of four (ZB = false) while n + 3 < n_e, ZB groups of four to the
      end and up to three single steps
  poisson_solve.hpp, relax_solve_rb2 (poll_loop)
      the chunked launch loop (8 iterates, doubling to poll_interval, the
      decision read one chunk behind)
The box is 1.0 x 0.7 x 1.3: dx, dy and dz all differ and all are below 1, so
the certified fast division (1 <= 1 / d^2) stays eligible.
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

BOX = (1.0, 0.7, 1.3)
OX, OY = 56, 24          # cells written per tile (RB2_OX, RB2_OY)
LX, LY = 64, 32          # cells loaded per tile (2 RB2_TC, RB2_TR)
GRID_CAP = 2048          # 8 workgroups x 256 CUs (hip_proj_ctx::grid_cap on an MI355X)
POLL_INTERVAL = 64       # hip_proj_config_default
CAPS = (6, 7)            # an even and an odd cap: the loop ends on a sweep's
                         # middle iterate (recomputed by the host) and on its input


class Run(NamedTuple):
    kb: int            # first plane of the run
    ke: int            # one past its last plane
    n_s: int           # first step that may be steady
    n_e: int           # steady groups of four start while n + 3 < n_e
    steady_fours: int  # groups of four ZB = false steps
    tail_steps: int    # single steps after the last group of four (0 .. 3)


class Layout(NamedTuple):
    tiles_x: int
    tiles_y: int
    kc: int
    interior: list     # (tx, ty) of the tiles marched with BND = false
    runs: list         # Run per z run


def is_interior(tx, ty, nx, ny):
    """rb2_tile_interior (k_rb2's `!bnd`)."""
    ilo, jlo = tx * OX - 4, ty * OY - 4
    return ilo >= 1 and ilo + LX - 1 <= nx - 3 and jlo >= 2 and jlo + LY - 1 <= ny - 3


def march(kb, ke):
    """rb2_march's step schedule for the run [kb, ke)."""
    q0 = kb - 4
    nsteps = ke - kb + 6
    n_s = min((max(kb + 2, 4) - q0 + 3) & ~3, nsteps)
    n_e = ke - 2 - q0 + 1
    n = 0
    while n + 3 < n_s:
        n += 4
    steady = 0
    while n + 3 < n_e:
        n += 4
        steady += 1
    while n + 3 < nsteps:
        n += 4
    return Run(kb, ke, n_s, n_e, steady, nsteps - n)


def layout(shape, kc_request=None, fixed=True, grid_cap=GRID_CAP) -> Layout:
    """The r2geo block for one device: kc_request is CFD_HIP_RB2_KC, fixed is
    CFD_HIP_RB2_KC_FIXED."""
    nx, ny, nz = shape
    assert nz > 1 and nx >= 8 and ny >= 8, shape  # else k_rb2 is not used
    nint_k = nz - 2
    tiles_x = (nx - 1 + OX - 1) // OX
    tiles_y = (ny - 1 + OY - 1) // OY
    kc = 128
    if nint_k >= 384 and 3 * tiles_x * tiles_y >= 8 * max(1, grid_cap // 8):
        kc = (nint_k + 2) // 3
    if kc_request is not None:
        kc = max(1, int(kc_request))
    while not fixed and kc > 4 and tiles_x * tiles_y * ((nint_k + kc - 1) // kc) < 512:
        kc //= 2
    kc = max(1, min(kc, nint_k))
    tiles_z = (nint_k + kc - 1) // kc
    runs = [march(1 + tz * kc, min(1 + tz * kc + kc, nz - 1)) for tz in range(tiles_z)]
    interior = [(tx, ty) for ty in range(tiles_y) for tx in range(tiles_x)
                if is_interior(tx, ty, nx, ny)]
    return Layout(tiles_x, tiles_y, kc, interior, runs)


def host_launches(stop_it, max_iter, poll_interval=POLL_INTERVAL):
    """(k_rb1, k_rb2) launches relax_solve_rb2 logs for a solve the device
    decides at iterate stop_it (max_iter when capped) with no ambiguous and no
    uncertified stop: one k_rb1 sweep (iterate 0 -> 1), then k_rb2 sweeps
    s = 1, 3, 5, ... in chunks, the state read one chunk behind."""
    cur, n1, n2, chunk = 0, 0, 0, 8
    prev_done = None
    while cur <= max_iter:
        target = cur + chunk
        while cur <= max_iter and cur < target:
            if cur == 0:
                n1 += 1
                cur += 1
            else:
                n2 += 1
                cur += 2
        done = stop_it < cur  # every iterate below cur has been decided on
        if prev_done:
            break
        prev_done = done
        chunk = min(chunk * 2, max(1, poll_interval))
    return n1, n2


class Case(NamedTuple):
    shape: tuple
    kc: int | None     # CFD_HIP_RB2_KC (None: the default), with CFD_HIP_RB2_KC_FIXED
    what: str

    @property
    def id(self):
        return sid(self.shape) + (f"-kc{self.kc}" if self.kc else "")


# The conditions in `what` govern; test_rb2_shapes.py checks each with layout().
CASES = [
    Case((118, 54, 20), None, "the smallest grid with an interior tile (3 x 3 tiles, the centre "
                              "one interior); one 18-plane run"),
    Case((117, 53, 20), None, "CONTROL: one short in x and y, the same tiling, no interior tile "
                              "(the edge of the bnd predicate)"),
    Case((122, 58, 30), None, "one 28-plane run: five steady groups, two tail steps"),
    Case((123, 59, 30), None, "odd nx, the same tiling"),
    Case((122, 58, 40), 9, "the shortest run with a steady group, tail 3; remainder run of 2"),
    Case((122, 58, 40), 10, "tail 0; remainder run of 8 planes (no steady group)"),
    Case((122, 58, 40), 11, "tail 1; remainder run of 5"),
    Case((122, 58, 40), 12, "tail 2; remainder run of 2"),
    Case((178, 82, 30), 13, "4 x 4 tiles, four mutually adjacent interior tiles (interior to "
                            "interior seams in x and y); runs 13 + 13 + 2"),
    Case((122, 58, 132), None, "the product's 128-plane run plus a 2-plane run"),
]
CONTROL = CASES[1]
XMAP_CASE = CASES[8]
STEP_SHAPE = (122, 58, 30)
STEP_RELAX = dict(tolerance=1e-2, max_iterations=5000)

# Relative tolerances whose oracle iteration counts are one odd, one even
# (chosen on the CPU; test_rb2_shapes.py holds them to it), and a cap well
# above both.
TOL_CAP = 400
TOL_CASES = [
    (CASES[2], (0.5, 0.3)),    # the oracle stops after 8 and 13 iterations
    (CASES[8], (0.55, 0.45)),  # 9 and 12
]
# The interior-peak problem at PEAK_CASE: the random problem x 8 on the cells
# the centre tile owns (columns 56 .. 111, rows 24 .. 47), in the planes whose
# residuals only steady steps form (the residual of X at planes 6 .. 25, of the
# middle iterate at 4 .. 23). The L-inf residual of every iterate up to the
# stop then lies in cells only the interior tile's unmasked maxima see.
# Both rhs and x0 are scaled: the residual of these problems is lap(x0)'s
# (~ 0.1 / dx^2, four decades above rhs), so a gain on rhs alone moves nothing.
PEAK_CASE = CASES[2]
PEAK_BLOCK = (slice(6, 24), slice(24, 48), slice(56, 112))  # planes, rows, columns
PEAK_GAIN = 8.0
PEAK_TOLS = (0.6, 0.35)  # the oracle stops after 6 and 11 iterations


def sid(shape):
    return "x".join(str(v) for v in shape)


def spacing(shape):
    nx, ny, nz = shape
    return (BOX[0] / (nx - 1), BOX[1] / (ny - 1), BOX[2] / (nz - 1))


@functools.lru_cache(maxsize=3)
def problem(shape, peak=False):
    """(rhs ~ N(0, 1), x0 = 0.1 N(0, 1)) on the whole (nz, ny, nx) array, shell
    included, seeded from the shape; peak: the interior-peak right-hand side.
    Read-only: every test copies x0."""
    nx, ny, nz = shape
    rng = np.random.default_rng(nx * 7 + nz * 3 + ny)
    rhs = rng.standard_normal((nz, ny, nx))
    x0 = 0.1 * rng.standard_normal((nz, ny, nx))
    if peak:
        rhs[PEAK_BLOCK] *= PEAK_GAIN
        x0[PEAK_BLOCK] *= PEAK_GAIN
    rhs.setflags(write=False)
    x0.setflags(write=False)
    return rhs, x0


def capped_params(iters):
    """A solve that can only stop at its cap."""
    from oracle import oracle
    return oracle.poisson_params(max_iterations=iters, tolerance=0.0, absolute_tolerance=0.0)


def tol_params(tol):
    from oracle import oracle
    return oracle.poisson_params(max_iterations=TOL_CAP, tolerance=tol)


@functools.lru_cache(maxsize=None)
def oracle_solve(shape, peak, key):
    """(status, stats, x) of the oracle's RB-SOR solve, computed once and
    read-only; key = ("cap", iters) or ("tol", tolerance)."""
    from oracle import oracle
    rhs, x0 = problem(shape, peak)
    prm = capped_params(key[1]) if key[0] == "cap" else tol_params(key[1])
    x = x0.copy()
    s, st = oracle.redblack_solve(x, rhs, *spacing(shape), prm)
    x.setflags(write=False)
    return s, st, x


def residual_abs(x, rhs, shape):
    """|lap(x) - rhs| on the interior cells, plain double numpy (positions,
    not bits): the 7-point form of linear_solver.c's residual."""
    dx, dy, dz = spacing(shape)
    c = x[1:-1, 1:-1, 1:-1]
    lap = ((x[1:-1, 1:-1, 2:] - 2 * c + x[1:-1, 1:-1, :-2]) / (dx * dx) +
           (x[1:-1, 2:, 1:-1] - 2 * c + x[1:-1, :-2, 1:-1]) / (dy * dy) +
           (x[2:, 1:-1, 1:-1] - 2 * c + x[:-2, 1:-1, 1:-1]) / (dz * dz))
    return np.abs(lap - rhs[1:-1, 1:-1, 1:-1])


def locate(cell, case: Case):
    """Which workgroup and step of the march writes cell (k, j, i): a shell
    cell is written with the interior cell it copies."""
    nx, ny, nz = case.shape
    lay = layout(case.shape, case.kc)
    k, j, i = cell
    kk, jj, ii = min(max(k, 1), nz - 2), min(max(j, 1), ny - 2), min(max(i, 1), nx - 2)
    tx, ty = ii // OX, jj // OY
    tz = (kk - 1) // lay.kc
    run = lay.runs[tz]
    n = kk + 2 - (run.kb - 4)  # Y2 of plane q - 2 is stored in step q
    first = (run.n_s + 3) // 4 * 4 if run.steady_fours else 0
    steady = run.steady_fours > 0 and first <= n < first + 4 * run.steady_fours
    return (f"tile (tx, ty) = ({tx}, {ty}) "
            f"{'interior' if (tx, ty) in lay.interior else 'boundary'}, "
            f"run {tz} [{run.kb}, {run.ke}) step {n} of {run.ke - run.kb + 6} "
            f"({'steady' if steady else 'ZB'})")


def first_diff(got, want, case: Case):
    """None if the arrays are bitwise equal, else the first differing cell
    with its tile, run and step, and how many cells differ."""
    ne = got.view(np.uint64) != want.view(np.uint64)
    if not ne.any():
        return None
    cell = tuple(int(v) for v in np.argwhere(ne)[0])
    return (f"{case.id}: {int(ne.sum())} cells differ, first (k, j, i) = {cell}: got "
            f"{float(got[cell])!r}, want {float(want[cell])!r}; " + locate(cell, case))
