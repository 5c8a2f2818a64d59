"""TEST INFRASTRUCTURE ONLY -- the shapes of the CG seam tests, one line each
saying which tile seam the shape sits on, and the random problem every test
of a shape shares (test_cg_reference.py, test_gpu_cg_seams.py).

Tilings (cfd_amd/csrc/hip/tile_plan.hpp, plan_tiles; tests/test_tile_plan.py
holds the claims below to what that planner gives, without a GPU):
  k_ccf          one device: 60 x 29 cells written per tile (CCF_OX x
                 CCF_OY_EDGE, the edge-sum form), tile tx writes columns
                 60 tx .. 60 tx + 59, ty rows 29 ty .. 29 ty + 28; on Z-slabs
                 and with CFD_HIP_CCF_EDGE_DOT=0 (the cell form) 60 x 28
                 (CCF_OY), rows 28 ty .. 28 ty + 27; tiles_x = (nx - 1 + 59) /
                 60; z runs of kc planes from plane 1 (kc = 24 on one device,
                 halved down to 3 on small grids unless CFD_HIP_CCF_KC_FIXED
                 is set)
  k_cgA / k_cgB  128 columns x sweep_rows (8 or 16) rows, z runs of kchunk
  k_cg_small     a flat index over the interior, 256 threads per workgroup
  k_pred3/corr3  128 columns x 16 rows
The box is 1.0 x 0.7 x 1.3, so dx, dy and dz all differ.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import cg_reference

BOX = (1.0, 0.7, 1.3)
ITERS = (1, 3, 4, 5, 8)  # every residue of the CG_XFOLD = 4 fold period + the first fold
# max |x - x_ref| <= BAR * max |x_ref - x0| (and the residual norms relative):
# 250 x the oracle's largest deviation from the reference (3.9e-14, measured
# on the CPU at 1..13 capped iterations on four of these shapes); the GPU
# differs from the oracle only in how its dot products are grouped
BAR = 1e-11
MAX_CELLS = 340_000
CG_SMALL_CELLS = 300_000  # kernels.hpp
CELL_FORM = " | 28-row tiles: "  # splits a description, see CCF_FIXED

# cg_variant 1, 3-D, CFD_HIP_CCF_KC_FIXED=1: 24-plane runs. The y seams of this
# table are those of the cell form's 28-row tiles only: it was chosen when
# every context ran that form. test_gpu_cg_seams.py creates one-device contexts
# with the default switches, which now run the edge-sum form on 29-row tiles, so
# there these shapes sit on the x seams and the z runs named before CELL_FORM,
# and what follows it holds on the 28-row tiles (CFD_HIP_CCF_EDGE_DOT=0, and
# the slabs' march). The 29-row seams are test_gpu_ccf_edge_dot.EDGE_FIXED's.
# "n-column" / "n-row": the last tile's interior columns / rows.
CCF_FIXED = [
    ((60, 28, 26), "wall column 59 closes tile 0; 24 planes: exactly one run" + CELL_FORM +
                   "wall row 27 closes tile 0"),
    ((61, 29, 26), "last interior column 59 closes tile 0, the wall has no tile" + CELL_FORM +
                   "last interior row 27 closes tile 0"),
    ((62, 30, 26), "one-column last x tile (interior 60 + wall 61)" + CELL_FORM +
                   "one-row last y tile (interior 28 + wall 29)"),
    ((63, 31, 26), "last x tile: interior 60-61 + wall 62" + CELL_FORM +
                   "last y tile likewise (interior 28-29 + wall 30)"),
    ((121, 57, 26), "second seam: last interior column 119 closes tile 1" + CELL_FORM +
                    "last interior row 55 closes tile 1"),
    ((122, 58, 27), "one-column third x tile; runs 24 + 1" + CELL_FORM + "one-row third y tile"),
    ((60, 29, 27), "even nx clamp with the wall on the seam; runs 24 + 1"),
    ((61, 28, 27), "odd nx clamp; runs 24 + 1" + CELL_FORM + "wall row on the y seam"),
    ((62, 31, 28), "one-column last x tile; runs 24 + 2"),
    ((63, 30, 28), "two-column last x tile; runs 24 + 2" + CELL_FORM + "one-row last y tile"),
    ((61, 29, 51), "49 planes: two runs + one plane"),
    ((62, 30, 51), "one-column last x tile over two runs + one plane" + CELL_FORM +
                   "one-row last y tile"),
    ((60, 58, 28), "x wall on the seam, two y tiles; runs 24 + 2" + CELL_FORM + "three y tiles"),
    ((121, 28, 27), "x interior ends on the second seam" + CELL_FORM + "y wall on the first"),
    ((122, 31, 28), "three x tiles (one column), two y tiles; runs 24 + 2"),
    ((63, 57, 27), "runs 24 + 1" + CELL_FORM + "y interior ends on the second seam"),
    ((62, 58, 27), "one-column last x tile (also a step shape)" + CELL_FORM +
                   "one-row third y tile"),
    ((61, 30, 27), "x interior ends on the seam (also a step shape)" + CELL_FORM +
                   "one-row last y tile"),
    ((121, 30, 51), "two full x tiles over two runs + one plane"),
]
# cg_variant 1 under the default kc (halved to 3 at these sizes, then clamped
# to the planes there are)
CCF_DEFAULT = [
    ((4, 4, 3), "the smallest legal grid: 2 x 2 x 1 interior cells"),
    ((5, 4, 3), "odd nx at the smallest ny, nz"),
    ((4, 5, 4), "even nx, two interior planes"),
    ((62, 30, 27), "the product's short runs (kc = 3) on the one-column last x tile" + CELL_FORM +
                   "one-row last y tile"),
]
# textbook CG: the sweeps (CFD_HIP_CG_SMALL=0, sweep_rows 8 and 16) and, by
# default, k_cg_small
TEXTBOOK = [
    ((127, 15, 1), "2-D, odd nx one short of the 128 seam, ny one short of 16"),
    ((128, 16, 1), "2-D, wall column 127 / wall row 15 close tile 0"),
    ((129, 17, 1), "2-D, the second x tile holds the wall column alone"),
    ((130, 18, 1), "2-D, second x tile: interior 128 + wall 129; rows 16-17"),
    ((129, 33, 1), "2-D, third 16-row tile holds the wall row alone"),
    ((127, 16, 7), "odd nx, wall row on the 16 seam, 5 planes"),
    ((128, 17, 7), "wall column on the seam, last interior row 15 on the seam"),
    ((129, 18, 7), "wall-only x tile, one interior row in the last 16-row tile"),
    ((130, 15, 7), "one interior column in the last x tile, ny below one 16-row tile"),
    ((128, 33, 7), "wall-only third 16-row tile (fifth 8-row tile)"),
    ((130, 17, 7), "one-column x tile and the last interior row on the seam"),
    ((129, 17, 5), "a step shape: wall-only x and y tiles"),
]
# (shape, kchunk): 5 interior planes in runs of 2 + 2 + 1 and 3 + 2
TEXTBOOK_KCHUNK = [
    ((130, 18, 7), 2, "kchunk 2 leaves a one-plane remainder run"),
    ((129, 17, 7), 3, "kchunk 3 leaves a two-plane remainder run"),
]
# k_cg_small only
SMALL_ONLY = [
    ((41, 37, 5), "39 x 35 x 3 = 4095 interior cells: one short of 16 workgroups of 256"),
    ((101, 102, 32), "297 000 interior cells, just under CG_SMALL_CELLS"),
]
# cg_variant 1, 2-D: k_cc1 / k_cc2
CC_2D = [
    ((129, 17, 1), "wall-only x tile, wall-only 16-row tile"),
    ((62, 30, 1), "a k_ccf seam shape taken 2-D"),
]
# whole projection steps from random fields (k_pred3 / k_corr3: 128 x 16)
STEP_SHAPES = [
    ((130, 18, 7), "one interior column / two rows past the 128 x 16 tile"),
    ((129, 17, 5), "wall-only x and y tiles"),
    ((127, 33, 6), "odd nx short of the seam, wall-only third y tile"),
    ((61, 30, 27), "k_ccf: x interior ends on the seam" + CELL_FORM + "one-row last y tile"),
    ((62, 58, 27), "k_ccf: one-column last x tile" + CELL_FORM + "one-row third y tile"),
]
# Z-slabs (in-process groups): (shape, ranks, interior planes per rank)
SLAB_CASES = [
    ((62, 30, 27), 2, (13, 12), "edge launch + interior march on every rank"),
    ((62, 30, 27), 3, (9, 8, 8), "edge launch + interior march on every rank"),
    ((61, 29, 7), 3, (2, 2, 1), "whole-march slabs of < 3 planes side by side"),
    ((61, 29, 10), 3, (3, 3, 2), "a whole-march slab of 2 planes beside two that split"),
]


def all_poisson_shapes():
    """Every shape a capped Poisson solve runs at, once each, in table order."""
    seen = []
    for tab in (CCF_FIXED, CCF_DEFAULT, TEXTBOOK, SMALL_ONLY, CC_2D):
        seen += [s for s, _ in tab]
    seen += [s for s, _, _ in TEXTBOOK_KCHUNK] + [c[0] for c in SLAB_CASES]
    return list(dict.fromkeys(seen))


def iters_for(shape):
    """The capped iteration counts run at `shape`: ITERS below the number of
    interior cells. In exact arithmetic CG ends after at most as many
    iterations as there are unknowns (4, 6 and 12 on the three smallest
    grids); from there on the residual is rounding noise, the next (p, A p)
    a breakdown, and no relative bar means anything."""
    nx, ny, nz = shape
    n = (nx - 2) * (ny - 2) * max(nz - 2, 1)
    return tuple(it for it in ITERS if it < n)


def sid(shape):
    return "x".join(str(v) for v in shape)


def spacing(shape):
    nx, ny, nz = shape
    return (BOX[0] / (nx - 1), BOX[1] / (ny - 1), BOX[2] / (nz - 1) if nz > 1 else 0.0)


def _rng(shape):
    nx, ny, nz = shape
    return np.random.default_rng(nx * 7 + nz * 3 + ny)


@functools.lru_cache(maxsize=4)
def problem(shape):
    """(rhs ~ N(0, 1), x0 = 0.1 N(0, 1)) on the whole (nz, ny, nx) array, shell
    included, seeded from the shape; read-only: every test copies x0."""
    nx, ny, nz = shape
    rng = _rng(shape)
    rhs = rng.standard_normal((nz, ny, nx))
    x0 = 0.1 * rng.standard_normal((nz, ny, nx))
    rhs.setflags(write=False)
    x0.setflags(write=False)
    return rhs, x0


@functools.lru_cache(maxsize=4)
def reference(shape):
    """{iters: CgReference} for every iters of ITERS, computed once per shape."""
    rhs, x0 = problem(shape)
    return cg_reference.cg_reference_at(x0, rhs, *spacing(shape), ITERS)


def capped_params(iters):
    """Parameters of a solve that can only stop at its cap: no tolerance a
    residual could meet."""
    from oracle import oracle
    return oracle.poisson_params(max_iterations=iters, tolerance=1e-30, absolute_tolerance=0.0)


def check_capped_solve(shape, iters, status, st, x, tile, kc=None, what=""):
    """The gates of a solve capped at `iters` against the long-double
    reference: status, iteration count, both residual norms and x (shell
    included) within BAR. Returns max |x - x_ref| / max |x_ref - x0|."""
    from cfd_amd import _abi as A
    ref = reference(shape)[iters]
    tag = f"{what} {sid(shape)} iters {iters}"
    where = cg_reference.worst_cell(x, ref.x, tile, kc)  # every message names the tile
    assert status == A.CFD_ERROR_MAX_ITER and st.status == A.POISSON_MAX_ITER, \
        f"{tag}: status {status} / {st.status}; {where}"
    assert st.iterations == iters, f"{tag}: {st.iterations} iterations; {where}"
    assert np.isfinite(x).all(), f"{tag}: x not finite; {where}"
    r0, rn = float(ref.residuals[0]), float(ref.residuals[iters])
    dev = float(np.max(np.abs(x.astype(cg_reference.LD) - ref.x))) / ref.moved
    d0, dn = abs(st.initial_residual - r0) / r0, abs(st.final_residual - rn) / rn
    print(f"SEAM {tag}: x {dev:.3e} res0 {d0:.3e} res {dn:.3e}")  # before the gates
    assert d0 <= BAR, f"{tag}: initial residual {st.initial_residual!r}, want {r0!r}; {where}"
    assert dn <= BAR, f"{tag}: final residual {st.final_residual!r}, want {rn!r}; {where}"
    assert dev <= BAR, f"{tag}: x off by {dev:.3e} > {BAR:.0e}; {where}"
    return dev


def step_case(shape, dt=1e-4, nu=0.01):
    """(grid, field, params) of a whole projection step from random fields:
    u, v, w, p = 0.1 N(0, 1) seeded from the shape, rho = 1, on the BOX."""
    from cfd_amd import api
    nx, ny, nz = shape
    g = api.Grid(nx, ny, nz, 0.0, BOX[0], 0.0, BOX[1], 0.0, BOX[2] if nz > 1 else 0.0)
    f = api.FlowField(nx, ny, nz)
    rng = np.random.default_rng(nx * 7 + nz * 3 + ny + 1)
    for k in ("u", "v", "w", "p"):
        getattr(f, k)[...] = 0.1 * rng.standard_normal((nz, ny, nx))
    f.rho[...] = 1.0
    f.T[...] = 300.0
    return g, f, api.validation_params(dt, nu)


JACOBI = dict(tolerance=1e-2, max_iterations=5000)
