"""Shape table, seeded inputs and the numpy model of the flow-diagnostics tests
(tests/test_flow_diag_cases.py, tests/test_gpu_flow_diag.py) and of the script
that records the reference helpers' results for them
(tests/golden/make_flow_diag_golden.py -> tests/golden/flow_diag_cases.json).

Shapes (nx, ny, nz), none above 42 210 cells (67x35x18):
  3x3x3, 3x3x1        one interior cell: every sum is a single term
  5x4x3, 4x5x1        smallest grids with more than one interior cell per axis
  17x13x11            odd extents on every axis
  34x19x1, 67x35x18   the direct solves' shapes
  130x18x5, 131x66x4  x past 128, y past 16 and 64, odd nx so the last 16-B
                      pair straddles the pad
  258x5x6             third x trip
  18x130x3            y past 128
  5x70x61             more than 4096 rows
  9x9x140             z past every run length in use
  129x5x4             the row walk's own seam: a wavefront walks a row 64 pairs
                      (128 cells) a trip, so at nx = 129 the second trip holds
                      one lane whose pair is half pad
The device pass (flow_diag.hip) walks rows: its only seams are the x trips
every 128 cells (130, 131, 129, 258) and the capped grid's second round of
rows past 4 x 1024 (5x70x61).

Inputs: u, v, w uniform in [-0.5, 0.5), rho uniform in [0.75, 1.25) per cell,
dx = 0.1, dy = 0.07, dz = 0.13. 2-D shapes are also recorded with w = 0
("name_w0"): there ke_rho, ke and ke_rho_cells have the terms of the 2-D
helpers test_compute_kinetic_energy, _simple and the cavity drivers'
compute_kinetic_energy.

model() forms the per-cell terms in float64 in the reference's expression
order (numpy: one IEEE operation per operator, no contraction) and sums them
exactly with math.fsum.
"""
import functools
import hashlib
import math

import numpy as np

JSON_FILE = "flow_diag_cases.json"
SPACING = (0.1, 0.07, 0.13)
RHO0 = 1.25  # density of a context without a per-cell rho
SHAPES = [(3, 3, 3), (3, 3, 1), (5, 4, 3), (4, 5, 1), (17, 13, 11), (34, 19, 1), (67, 35, 18),
          (130, 18, 5), (131, 66, 4), (258, 5, 6), (18, 130, 3), (5, 70, 61), (9, 9, 140),
          (129, 5, 4)]
X_SEAMS = (128, 256)   # a trip of the row walk ends before these columns
ROW_SEAM = 4096        # rows of one round of the capped grid
FIELDS = ("u", "v", "w", "rho")
SUMS = ("div_sumsq", "ke", "ke_rho", "ke_rho_cells")
U = 2.0 ** -53

BUGS = ("dvdy_x_stride", "no_dwdz", "dz_for_2dz", "i_lo", "i_hi", "j_lo", "j_hi", "k_lo", "k_hi",
        "ke_all_cells", "rho0_for_rho", "no_2d_dz_rule")


def name_of(shape, w0=False):
    return "s%dx%dx%d" % tuple(shape) + ("_w0" if w0 else "")


def cases():
    """[(name, shape, w0)]: every shape, and the 2-D ones again with w = 0."""
    out = [(name_of(s), s, False) for s in SHAPES]
    out += [(name_of(s, True), s, True) for s in SHAPES if s[2] == 1]
    return out


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def inputs(shape, w0=False):
    """{u, v, w, rho: read-only (nz, ny, nx) float64 arrays}, seeded from the shape."""
    nx, ny, nz = shape
    rng = np.random.default_rng([nx, ny, nz, 2024])
    out = {k: rng.random((nz, ny, nx)) - 0.5 for k in ("u", "v", "w")}
    out["rho"] = 0.75 + 0.5 * rng.random((nz, ny, nx))
    if w0:
        out["w"] = np.zeros((nz, ny, nx))
    for a in out.values():
        a.setflags(write=False)
    return out


def interior_cells(shape):
    nx, ny, nz = shape
    return max(nx - 2, 0) * max(ny - 2, 0) * (nz - 2 if nz > 1 else 1)


def exact_sum(terms):
    """math.fsum of the terms with the classes the entries state: any NaN term
    gives NaN, +inf terms only +inf (also when the exact sum overflows)."""
    t = np.asarray(terms, dtype=np.float64).reshape(-1)
    if np.isnan(t).any() or (np.isposinf(t).any() and np.isneginf(t).any()):
        return math.nan
    if np.isinf(t).any():
        return math.inf if np.isposinf(t).any() else -math.inf
    try:
        return math.fsum(t.tolist())
    except OverflowError:
        return math.inf


def model(shape, f, spacing=SPACING, rho0=None, bug=None):
    """The definitions of include/cfd_hip/flow_diagnostics.h on the arrays
    f = {u, v, w, rho} (rho0 given: that constant instead of f["rho"]).
    Returns the cfd_flow_diag_t numbers (sums exact), the per-cell term arrays
    ("terms": div, and the four sums' terms), "div_abs_parts" = max over the
    interior of |du_dx| + |dv_dy| + |dw_dz|, and the term counts "n".
    bug: one of BUGS, a planted defect (tests/test_flow_diag_cases.py)."""
    assert bug is None or bug in BUGS
    nx, ny, nz = shape
    dx, dy, dz = spacing
    three = nz > 1
    n = nx * ny * nz
    u, v, w = (np.ascontiguousarray(f[k], dtype=np.float64).reshape(-1) for k in ("u", "v", "w"))
    rho = (np.ascontiguousarray(f["rho"], dtype=np.float64).reshape(-1) if rho0 is None
           else np.full(n, float(rho0)))
    lo = {"i": 1, "j": 1, "k": 1 if three else 0}
    hi = {"i": nx - 1, "j": ny - 1, "k": nz - 1 if three else 1}
    if bug and bug[1:] == "_lo" and (three or bug[0] != "k"):
        lo[bug[0]] += 1
    if bug and bug[1:] == "_hi" and (three or bug[0] != "k"):
        hi[bug[0]] -= 1
    kk, jj, ii = np.meshgrid(np.arange(lo["k"], hi["k"]), np.arange(lo["j"], hi["j"]),
                             np.arange(lo["i"], hi["i"]), indexing="ij")
    sz = nx * ny if three else 0
    idx = (kk * (nx * ny) + jj * nx + ii).reshape(-1)
    sy = 1 if bug == "dvdy_x_stride" else nx
    inv_2dz = 1.0 / (2.0 * dz) if three else 0.0
    if bug == "dz_for_2dz" and three:
        inv_2dz = 1.0 / dz
    with np.errstate(all="ignore"):
        du_dx = (u[idx + 1] - u[idx - 1]) / (2.0 * dx)
        dv_dy = (v[idx + sy] - v[idx - sy]) / (2.0 * dy)
        dw_dz = (w[idx + sz] - w[idx - sz]) * inv_2dz
        if bug == "no_dwdz":
            dw_dz = np.zeros_like(dw_dz)
        div = du_dx + dv_dy + dw_dz
        s = u * u + v * v + w * w
        dzv = dz if (three or bug == "no_2d_dz_rule") else 1.0
        e = np.arange(n) if bug == "ke_all_cells" else idx
        re = np.full(n, RHO0) if bug == "rho0_for_rho" else rho
        terms = {"div": div, "div_sumsq": div * div,
                 "ke": 0.5 * s[e] * dx * dy * dzv,
                 "ke_rho": 0.5 * re[e] * s[e] * dx * dy * dzv,
                 "ke_rho_cells": 0.5 * rho * s}
        ad = np.abs(div)
        parts = np.abs(du_dx) + np.abs(dv_dy) + np.abs(dw_dz)
    finite = ad[~np.isnan(ad)]
    out = {"div_linf": float(finite.max()) if finite.size else 0.0,
           "div_cells": int(div.size), "div_nan_cells": int(np.isnan(div).sum()),
           "terms": terms, "n": {k: int(terms[k].size) for k in SUMS},
           "div_abs_parts": float(np.nanmax(parts)) if parts.size and not np.isnan(parts).all()
           else 0.0}
    for k in SUMS:
        out[k] = exact_sum(terms[k])
    out["div_l2"] = (math.sqrt(out["div_sumsq"] / div.size)
                     if div.size and not math.isnan(out["div_sumsq"]) else
                     (math.nan if div.size else 0.0))
    return out


def sum_close(got, want, nterms, factor):
    """|got - want| <= factor * nterms-ish bar: the bound factor * 2^-53 * |want|
    for sums of non-negative terms (every term of every sum here is one); NaN
    and inf by class."""
    if math.isnan(want):
        return math.isnan(got)
    if math.isinf(want):
        return got == want
    return abs(got - want) <= factor * U * abs(want)


def plant_positions(shape):
    """[(k, j, i)]: the first and last interior cells, each neighbour of them
    across the boundary, and the cells on either side of every seam of the
    device pass (the x trips, the second round of rows); distinct, in range."""
    nx, ny, nz = shape
    three = nz > 1
    k0, k1 = (1, nz - 2) if three else (0, 0)
    first, last = (k0, 1, 1), (k1, ny - 2, nx - 2)
    out = [first, last]
    for (k, j, i) in (first, last):
        out += [(k, j, i - 1), (k, j, i + 1), (k, j - 1, i), (k, j + 1, i)]
        if three:
            out += [(k - 1, j, i), (k + 1, j, i)]
    jm, km = ny // 2, nz // 2
    for s in X_SEAMS:
        out += [(km, jm, i) for i in (s - 2, s - 1, s, s + 1)]
    for r in (ROW_SEAM - 1, ROW_SEAM):
        out.append((r // ny, r % ny, nx // 2))
    ok = []
    for p in out:
        k, j, i = p
        if 0 <= k < nz and 0 <= j < ny and 0 <= i < nx and p not in ok:
            ok.append(p)
    return ok
