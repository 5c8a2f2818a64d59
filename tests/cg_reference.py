"""TEST INFRASTRUCTURE ONLY -- a plain textbook CG in numpy long double, the
high-precision reference of the CG seam tests (test_cg_reference.py on the CPU,
test_gpu_cg_seams.py on the GPU).

The problem is the one linear_solver_cg.c solves and ccf.hpp:5-17 restates:
A = -(7-point Laplacian) on the interior cells with the reference's spacing
factors (1 / (dx dx), 1 / (dy dy), 1 / (dz dz), each rounded to double once,
as the solvers hold them), zero walls for the residual and the search
direction, the Neumann shell copy on x before and after the solve, r_0 =
-rhs + lap(x_0), then `iters` iterations of
    alpha = (r, r) / (p, A p);  x += alpha p;  r -= alpha A p;
    beta = (r', r') / (r, r);   p = r' + beta p
with no convergence test. Everything is array arithmetic in np.longdouble
(64-bit mantissa), so its own rounding sits three decimal digits below any
double-precision CG's.

worst_cell() names the worst cell of a mismatch with its tile and in-tile
offset, so a failing seam case says which tile edge it sits on.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

LD = np.longdouble

# the k_ccf tiles (tile_plan.hpp; z runs of kc planes): CCF_OX x CCF_OY_EDGE on
# one device (the edge-sum form), CCF_OX x CCF_OY on Z-slabs and with
# CFD_HIP_CCF_EDGE_DOT=0 (the cell form); the textbook sweeps' (128 columns x
# sweep_rows) and k_pred3 / k_corr3's (128 x 16)
CCF_EDGE_TILE = (60, 29)
CCF_TILE = (60, 28)
SWEEP_TILE = (128,)
PC3_TILE = (128, 16)


def _require_extended():
    if np.finfo(LD).eps >= 2e-16:
        raise RuntimeError("np.longdouble is no wider than double on this platform: "
                           "the CG reference needs an extended-precision long double")


def neumann_shell(x: np.ndarray) -> None:
    """The solvers' default boundary copy, in place: the z faces from their
    neighbour planes, then in every plane the x faces, then the y faces."""
    if x.shape[0] > 1:
        x[0] = x[1]
        x[-1] = x[-2]
    x[:, :, 0] = x[:, :, 1]
    x[:, :, -1] = x[:, :, -2]
    x[:, 0, :] = x[:, 1, :]
    x[:, -1, :] = x[:, -2, :]


def interior(shape):
    """Index of the interior cells of an (nz, ny, nx) array (all of z if nz = 1)."""
    kk = slice(1, -1) if shape[0] > 1 else slice(None)
    return (kk, slice(1, -1), slice(1, -1))


def laplacian(a: np.ndarray, dx, dy, dz) -> np.ndarray:
    """7-point Laplacian of `a` on its interior cells (5-point if nz = 1)."""
    cx = LD(1.0 / (dx * dx))
    cy = LD(1.0 / (dy * dy))
    kk = interior(a.shape)[0]
    c = a[kk, 1:-1, 1:-1]
    out = (a[kk, 1:-1, 2:] - 2 * c + a[kk, 1:-1, :-2]) * cx
    out = out + (a[kk, 2:, 1:-1] - 2 * c + a[kk, :-2, 1:-1]) * cy
    if a.shape[0] > 1 and dz > 0.0:
        cz = LD(1.0 / (dz * dz))
        out = out + (a[2:, 1:-1, 1:-1] - 2 * c + a[:-2, 1:-1, 1:-1]) * cz
    return out


class CgReference(NamedTuple):
    x: np.ndarray            # long double, shell included
    residuals: list          # ||r_0||, ||r_1||, ..., ||r_iters|| (2-norms)
    moved: float             # max |x - x_0| (x_0 with its shell applied)
    r: np.ndarray            # the recurrence residual r_iters on the interior


def cg_reference_at(x0: np.ndarray, rhs: np.ndarray, dx, dy, dz, stops) -> dict:
    """{iters: CgReference} for every iteration count in `stops`, from one run
    (a solve capped at m iterations is the first m iterations of a longer one)."""
    _require_extended()
    x = np.array(x0, dtype=LD)
    b = np.array(rhs, dtype=LD)
    neumann_shell(x)
    xs = x.copy()
    inn = interior(x.shape)
    r = -b[inn] + laplacian(x, dx, dy, dz)
    p = np.zeros_like(x)  # zero walls: A p reads them
    p[inn] = r
    rho = np.sum(r * r)
    res = [np.sqrt(rho)]
    out = {}

    def snapshot(it):
        xo = x.copy()
        neumann_shell(xo)
        out[it] = CgReference(xo, list(res), float(np.max(np.abs(xo - xs))), r.copy())

    if 0 in stops:
        snapshot(0)
    for it in range(1, max(stops) + 1):
        ap = -laplacian(p, dx, dy, dz)
        alpha = rho / np.sum(p[inn] * ap)
        x[inn] += alpha * p[inn]
        r = r - alpha * ap
        rho_new = np.sum(r * r)
        res.append(np.sqrt(rho_new))
        p[inn] = r + (rho_new / rho) * p[inn]
        rho = rho_new
        if it in stops:
            snapshot(it)
    return out


def cg_reference(x0: np.ndarray, rhs: np.ndarray, dx, dy, dz, iters: int) -> CgReference:
    return cg_reference_at(x0, rhs, dx, dy, dz, (iters,))[iters]


def true_residual(x: np.ndarray, x0: np.ndarray, rhs: np.ndarray, dx, dy, dz) -> np.ndarray:
    """-rhs + lap(x) on the interior, from the interior of x inside the shell
    the solve ran with: that of x0 after its shell copy. (The iteration moves
    the interior only, with zero walls for p; the closing shell copy of x is
    not part of the operator.)"""
    xt = np.array(x0, dtype=LD)
    neumann_shell(xt)
    inn = interior(xt.shape)
    xt[inn] = np.asarray(x, dtype=LD)[inn]
    return -np.array(rhs, dtype=LD)[inn] + laplacian(xt, dx, dy, dz)


def worst_cell(got: np.ndarray, want: np.ndarray, tile, kc: int | None = None) -> str:
    """Where |got - want| is largest: the cell (k, j, i), the tile that writes
    it and its offset inside that tile. `tile` is (columns,) or (columns,
    rows) of a tiling that starts at cell 0 in x and y; `kc` the z-run length
    of a tiling whose first run starts at the first interior plane."""
    d = np.abs(np.asarray(got, dtype=LD) - np.asarray(want, dtype=LD))
    k, j, i = (int(v) for v in np.unravel_index(int(np.argmax(d)), d.shape))
    t = [f"x tile {i // tile[0]} + {i % tile[0]} of {tile[0]}"]
    if len(tile) > 1:
        t.append(f"y tile {j // tile[1]} + {j % tile[1]} of {tile[1]}")
    if kc and d.shape[0] > 1:
        kk = k - 1
        t.append(f"z run {kk // kc} + {kk % kc} of {kc}" if kk >= 0 else "z face")
    nz, ny, nx = d.shape
    return (f"worst cell (k, j, i) = ({k}, {j}, {i}) of ({nz}, {ny}, {nx}): "
            f"|diff| = {float(d[k, j, i]):.3e}, got {float(got[k, j, i])!r}, "
            f"want {float(want[k, j, i])!r}; " + ", ".join(t))
