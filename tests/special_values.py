"""TEST INFRASTRUCTURE ONLY -- inputs that drive the fast-division fallbacks
(device_util.hpp divc / divz / DivFastZ + DivExact, rb2.hpp) and the bitwise
comparison that sees signed zeros and NaNs (test_special_values.py proves on
the oracle alone that the inputs reach both sides of the thresholds;
test_gpu_special_values.py runs the kernels on them).

A division a / d by a constant spacing takes the reciprocal-multiply form
only while |RN(a RN(1/d))| lies in [2^-900, 2^900] (or is a zero, for divz).
The builders below put a field's quotients on both sides of that range:

  tiny         u, v, w, p = N(0, 1) 2^e, e uniform per cell in TINY_E
  subnormal    the same with e in SUBNORMAL_E: every quotient below the range
  huge         u, v, w with e in HUGE_E, p as step_case gives it. The
               convective products u du/dx of such values overflow by
               necessity (2^890 x 2^896); the reference's +-100 clamp absorbs
               the infinities and the NaNs of inf - inf, so the outputs are
               finite. No difference, quotient or pressure value overflows.
  signed_zero  70 % of the cells +-0.0 with a random sign
  nonfinite    1 % of the interior cells of u, v, w NaN / +inf / -inf (the
               shell stays finite, as does p)
  planted      step_case's field with single cells of 2^-950, a subnormal,
               2^905 and -0.0 at the lane-0 / lane-63 columns, the LDS halo
               rows and the first and last plane (a wave that holds exactly
               one dropped lane), plus, away from those rows, rows that hold
               N(0, 1) 2^905 in every third cell so that each predictor
               division class has a tenth of the interior on either side.
               2^905 stays out of the shell and out of p: the shell's
               velocities enter the Poisson right-hand side unclamped, and a
               pressure of that size would push every corrected velocity
               into the clamp, where nothing could be told apart

Relaxation problems: x0 = N(0, 1) 2^e, rhs = N(0, 1) 2^(e + 12) with e a ramp
plus +-1 of jitter. Per-cell random exponents do not survive one sweep (the
update averages the neighbours), a ramp does: one sweep moves a magnitude by
at most the neighbour weight, 2^-1.06 per column in x and 2^-5.6 per row in
y at these spacings, so a ramp no steeper than that keeps its shape.
  axis "x"     e = E + s (93 - |i - 155|): the threshold column is 62 (the
               middle of the first 124-column k_rb1 tile, lanes 30 / 31 of its
               wave) and, at nx = 250, column 248 (the remainder strip)
  axis "jk"    e = E + s (j + k - mid): the threshold runs through every tile
               (the subnormal variant falls at 12 bits per step below the
               threshold, to reach the subnormals within 11 steps, and rises
               at 4 above it, so that no larger value bleeds down)
"""
from __future__ import annotations

import functools

import numpy as np

from tests import cg_seam_shapes as T

LO, HI = 2.0 ** -900, 2.0 ** 900
TINY_E = (-940, -900)
SUBNORMAL_E = (-1074, -1000)
HUGE_E = (865, 900)
STEP_SHAPES = [(130, 18, 7), (127, 33, 6), (129, 17, 1)]
REGIMES = ("tiny", "subnormal", "huge", "signed_zero", "nonfinite", "planted")
FIELDS = ("u", "v", "w", "p")
PC_TILE = (128, 16)

RELAX_SHAPES = [(130, 20, 9), (250, 21, 10), (249, 21, 10), (130, 20, 1)]
RELAX_CAPS = (6, 7)
# (kind, axis): the ramp's E is the exponent of x at which the x class's
# quotient sits on the threshold, 2^-900 dx^2 or 2^900 dx^2 (-914 and 886 at
# nx = 130; the y class's is 4 to 6 higher); slopes in bits per column / per
# j + k step
RELAX_PROBLEMS = [(kind, axis) for kind in ("tiny", "subnormal", "huge") for axis in ("x", "jk")]
_RELAX_T = {"tiny": -900, "subnormal": -900, "huge": 900}
_RELAX_SLOPE = {("tiny", "x"): 1.0, ("tiny", "jk"): 4.0,
                ("subnormal", "x"): 2.4, ("subnormal", "jk"): (12.0, 4.0),
                ("huge", "x"): -0.75, ("huge", "jk"): -3.0}


def _rng(shape, salt):
    nx, ny, nz = shape
    return np.random.default_rng([nx, ny, nz, salt])


def _scaled(rng, dims, window):
    e = rng.integers(window[0], window[1] + 1, size=dims)
    return np.ldexp(rng.standard_normal(dims), e)


def _interior(a):
    return a[1:-1, 1:-1, 1:-1] if a.shape[0] > 1 else a[:, 1:-1, 1:-1]


def planted_rows(ny):
    """Rows that hold 2^905 in every third cell: clear of rows 13 .. 19 and of
    the last six rows, where the single cells sit."""
    return [j for j in range(2, ny - 6, 3) if not 13 <= j <= 19]


def planted_cells(shape):
    """[(k, j, i, kind)]: the single cells, kinds in turn."""
    nx, ny, nz = shape
    cols = sorted({c for c in (0, 1, 127, 128, nx - 2) if c < nx})
    rows = [r for r in (15, 16, 17) if r < ny]
    planes = [0] if nz == 1 else [1, nz - 2]
    out, n = [], 0
    for k in planes:
        for j in rows:
            for i in cols:
                out.append((k, j, i, n % 4))
                n += 1
    return out


_KINDS = (2.0 ** -950, 2.0 ** -1060, 2.0 ** 905, -0.0)


def step_fields(regime, shape):
    """(grid, field, params) of a Jacobi-route step of `regime` at `shape`,
    seeded from the shape (a fresh field: callers may advance it)."""
    g, f, p = T.step_case(shape)
    nx, ny, nz = shape
    dims = (nz, ny, nx)
    rng = _rng(shape, REGIMES.index(regime))
    if regime in ("tiny", "subnormal"):
        win = TINY_E if regime == "tiny" else SUBNORMAL_E
        for k in FIELDS:
            getattr(f, k)[...] = _scaled(rng, dims, win)
    elif regime == "huge":
        for k in ("u", "v", "w"):
            getattr(f, k)[...] = _scaled(rng, dims, HUGE_E)
    elif regime == "signed_zero":
        for k in FIELDS:
            a = getattr(f, k)
            z = rng.random(dims) < 0.7
            sign = np.where(rng.random(dims) < 0.5, -0.0, 0.0)
            a[z] = sign[z]
    elif regime == "nonfinite":
        for k in ("u", "v", "w"):
            a = getattr(f, k)
            pick = rng.random(dims) < 0.01
            what = rng.integers(0, 3, size=dims)
            vals = np.array([np.nan, np.inf, -np.inf])[what]
            inner = np.zeros(dims, dtype=bool)
            _interior(inner)[...] = True
            pick &= inner
            a[pick] = vals[pick]
    elif regime == "planted":
        for n, k in enumerate(("u", "v", "w")):
            a = getattr(f, k)
            for j in planted_rows(ny):
                cells = _interior(a[:, j - 1:j + 2, :])[:, 0, (j + n) % 3::3]
                cells[...] = np.ldexp(rng.standard_normal(cells.shape), 905)
        for n, k in enumerate(FIELDS):
            a = getattr(f, k)
            for kk, j, i, kind in planted_cells(shape):
                kind = (kind + n) % 4
                shell = i in (0, nx - 1) or j in (0, ny - 1)
                if kind == 2 and (shell or k == "p"):
                    kind = 0
                a[kk, j, i] = _KINDS[kind]
    else:
        raise ValueError(regime)
    return g, f, p


# ---- relaxation problems -----------------------------------------------------

def _ramp(kind, axis, shape):
    nx, ny, nz = shape
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    s = _RELAX_SLOPE[kind, axis]
    if axis == "x":
        t = 93 - np.abs(i - 155)
    else:
        t = j + k - (2 + (ny - 2) + max(nz - 2, 0)) / 2.0
    if isinstance(s, tuple):  # (below, above) the threshold
        s = np.where(t < 0, s[0], s[1])
    dx = T.spacing(shape)[0]
    return _RELAX_T[kind] + np.floor(np.log2(dx * dx)) + s * t


@functools.lru_cache(maxsize=8)
def relax_problem(kind, axis, shape):
    """(x0, rhs) on the whole (nz, ny, nx) array, read-only: tests copy x0."""
    nx, ny, nz = shape
    dims = (nz, ny, nx)
    rng = _rng(shape, 100 + RELAX_PROBLEMS.index((kind, axis)))
    e = np.rint(_ramp(kind, axis, shape)).astype(np.int64) + rng.integers(-1, 2, size=dims)
    x0 = np.ldexp(rng.standard_normal(dims), e)
    rhs = np.ldexp(rng.standard_normal(dims), e + 12)
    x0.setflags(write=False)
    rhs.setflags(write=False)
    return x0, rhs


def relax_params(cap, **kw):
    from oracle import oracle
    return oracle.poisson_params(max_iterations=cap, tolerance=0.0, absolute_tolerance=0.0, **kw)


@functools.lru_cache(maxsize=64)
def relax_oracle(method, kind, axis, shape, cap, check_interval=1):
    """(status, stats, x) of the oracle's capped solve, computed once and
    shared (x read-only). method: "rb" or "jacobi"."""
    from oracle import oracle
    x0, rhs = relax_problem(kind, axis, shape)
    x = x0.copy()
    prm = relax_params(cap, check_interval=check_interval)
    fn = oracle.redblack_solve if method == "rb" else oracle.jacobi_solve
    s, st = fn(x, rhs, *T.spacing(shape), prm)
    x.setflags(write=False)
    return s, st, x


# ---- census -----------------------------------------------------------------

def shares(a, d):
    """Shares of the quotients a / d as the kernels classify them (|a RN(1/d)|):
    {"zero", "below", "in", "above"}; non-finite quotients count as above."""
    with np.errstate(all="ignore"):
        q = np.abs(np.asarray(a, dtype=np.float64).ravel() * (1.0 / d))
    n = float(q.size)
    zero = q == 0.0
    below = (q < LO) & ~zero
    inr = (q >= LO) & (q <= HI)
    return {"zero": zero.sum() / n, "below": below.sum() / n, "in": inr.sum() / n,
            "above": 1.0 - (zero.sum() + below.sum() + inr.sum()) / n}


def _c(a):  # interior centre and its x / y neighbours
    three = a.shape[0] > 1
    ks = slice(1, -1) if three else slice(None)
    return (a[ks, 1:-1, 1:-1], a[ks, 1:-1, :-2], a[ks, 1:-1, 2:], a[ks, :-2, 1:-1], a[ks, 2:, 1:-1])


def predictor_census(shape, u, v, w):
    """Shares per division class of the predictor (solver_projection.c:121-
    182) over the interior cells of the three input fields together."""
    dx, dy, _ = T.spacing(shape)
    num = {"d/dx": [], "d/dy": [], "d2/dx2": [], "d2/dy2": []}
    with np.errstate(all="ignore"):
        for a in (u, v, w):
            c, xm, xp, ym, yp = _c(a)
            num["d/dx"].append((xp - xm).ravel())
            num["d/dy"].append((yp - ym).ravel())
            num["d2/dx2"].append((xp - 2.0 * c + xm).ravel())
            num["d2/dy2"].append((yp - 2.0 * c + ym).ravel())
    div = {"d/dx": 2.0 * dx, "d/dy": 2.0 * dy, "d2/dx2": dx * dx, "d2/dy2": dy * dy}
    return {k: shares(np.concatenate(v_), div[k]) for k, v_ in num.items()}


def corrector_census(shape, p):
    """Shares of dp/dx and dp/dy (solver_projection.c:243-262) from the
    pressure the solve returned, which is the step's output p."""
    dx, dy, _ = T.spacing(shape)
    with np.errstate(all="ignore"):
        c, xm, xp, ym, yp = _c(p)
        return {"dp/dx": shares(xp - xm, 2.0 * dx), "dp/dy": shares(yp - ym, 2.0 * dy)}


def relax_census(shape, x):
    """Shares of the sweep's (xl + xr) / dx^2, (ys + yn) / dy^2 and of the
    residual's second differences at the iterate x."""
    dx, dy, _ = T.spacing(shape)
    with np.errstate(all="ignore"):
        c, xm, xp, ym, yp = _c(x)
        return {"x": shares(xp + xm, dx * dx), "y": shares(yp + ym, dy * dy),
                "res x": shares(xp - 2.0 * c + xm, dx * dx),
                "res y": shares(yp - 2.0 * c + ym, dy * dy)}


def outside(s):
    return s["below"] + s["above"]


def fmt(census):
    return "; ".join(f"{k}: zero {s['zero']:.1%} below {s['below']:.1%} in {s['in']:.1%} "
                     f"above {s['above']:.1%}" for k, s in census.items())


# ---- comparison -------------------------------------------------------------

def bits_differ(got, want):
    """Boolean array: cells whose uint64 patterns differ, every NaN one class."""
    got = np.ascontiguousarray(got, dtype=np.float64)
    want = np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    return (gn != wn) | ((got.view(np.uint64) != want.view(np.uint64)) & ~(gn & wn))


def assert_bits_equal(got, want, tile=None, what=""):
    """got == want bit for bit: -0.0 differs from +0.0 and a NaN equals only a
    NaN (same positions, payload ignored). On failure names the number of
    differing cells and the worst one with the tile that writes it (`tile` as
    for cg_reference.worst_cell; None: no tile named)."""
    bad = bits_differ(got, want)
    if not bad.any():
        return
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    with np.errstate(all="ignore"):
        d = np.abs(got.astype(np.longdouble) - want.astype(np.longdouble))
    d = np.where(np.isfinite(d), d, np.inf)  # a NaN / inf mismatch is the worst
    d = np.where(bad, d, -1.0)
    idx = tuple(int(v) for v in np.unravel_index(int(np.argmax(d)), d.shape))
    g, w = float(got[idx]), float(want[idx])
    where = []
    if tile is not None and len(idx) == 3:
        k, j, i = idx
        where.append(f"x tile {i // tile[0]} + {i % tile[0]} of {tile[0]}")
        if len(tile) > 1:
            where.append(f"y tile {j // tile[1]} + {j % tile[1]} of {tile[1]}")
    raise AssertionError(
        f"{what}: {int(bad.sum())} of {bad.size} cells differ in bits; worst cell (k, j, i) = "
        f"{idx} of {got.shape}: got {g!r} ({g.hex() if np.isfinite(g) else g}), want {w!r} "
        f"({w.hex() if np.isfinite(w) else w})" + ("; " + ", ".join(where) if where else ""))
