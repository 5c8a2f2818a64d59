"""Seeded inputs and the shape table of the field-statistics / velocity-magnitude
/ CSV-output tests (tests/test_derived_fixtures.py, tests/test_gpu_derived.py)
and of the script that records the reference's results for them
(tests/golden/make_derived_golden.py -> tests/golden/derived_cases.json).

Shapes: the smallest at which the device pass's row walk can go wrong.
  3x3x1      smaller than a wavefront, one workgroup, 2-D
  17x13x11   nx not a multiple of 8: pad columns exist, an odd nx (the last
             16-B pair of a row is half pad)
  67x9x5     crosses the 64-wide tile (a lane's second pair of a row), tail
  130x34x3   crosses the 128-wide tile, even nx with pad columns
  129x66x1   2-D, more than 64 pairs a row and an odd nx
  96x96x48   4608 rows: more than 4 x 1024, so the capped grid's second round
             of rows and the ticket over 1024 workgroups both run
The pass has no other seam: a wavefront owns a row whatever its width, and a
row holds at most ceil(nx / 2) pairs walked 64 at a time.

Kinds: "real" fields are seeded doubles; "int" fields hold integers with
|x| <= 2^20 (at most 442368 cells, so every partial sum is an exact integer
below 2^53 and every summation order gives the same bits).

Every field carries planted, unique extremes so that a dropped cell, a pad
value or a wrong plane shows: u's max at index 0 and its min in the last cell
(last column, last plane), v's max in the first plane's last column, w's min
at index 0 and its max in the last plane, the others at seeded cells.
"""
import hashlib
import math

import numpy as np

FIELDS = ("u", "v", "w", "p", "rho", "T")
STATS = FIELDS + ("vel_mag",)
JSON_FILE = "derived_cases.json"
NPZ_FILE = "derived_vel_mag_17x13x11.npz"
NPZ_CASE = "s17_real"

SHAPES = {"s3": (3, 3, 1), "s17": (17, 13, 11), "s67": (67, 9, 5), "s130": (130, 34, 3),
          "s129": (129, 66, 1), "s96": (96, 96, 48)}
# seeds for which every real-valued average (all CSV steps included) lies at
# least 1e-9 relative away from a %.6e rounding boundary (boundary_clear below)
_SEEDS = {"s3": 11, "s17": 22, "s67": 13, "s130": 14, "s129": 15, "s96": 16}

CASES = [{"name": f"{s}_{kind}", "shape": SHAPES[s], "kind": kind,
          "seed": _SEEDS[s] + (100 if kind == "int" else 0)}
         for s in SHAPES for kind in ("real", "int")]
BY_NAME = {c["name"]: c for c in CASES}

# CSV files are recorded for one 2-D and one 3-D case, three steps each
CSV_CASES = ("s129_real", "s17_real")
CSV_STEPS = 3
RHO0 = 1.25  # density of a context without a per-cell rho


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def _plant(a, rng, lo_cell, hi_cell, lo, hi):
    flat = a.reshape(-1)
    n = flat.size
    if lo_cell is None or hi_cell is None:
        cells = rng.choice(n, size=2, replace=False) if n > 2 else np.array([0, n - 1])
        lo_cell = int(cells[0]) if lo_cell is None else lo_cell
        hi_cell = int(cells[1]) if hi_cell is None else hi_cell
        if lo_cell == hi_cell:
            hi_cell = (lo_cell + 1) % n
    flat[lo_cell] = lo
    flat[hi_cell] = hi


def inputs(case, step=0):
    """{name: (nz, ny, nx) float64 array} of u, v, w, p, rho, T. `step` varies
    the seed (the CSV files hold three steps)."""
    nx, ny, nz = case["shape"]
    n = nx * ny * nz
    rng = np.random.default_rng([case["seed"], step])
    integer = case["kind"] == "int"
    out = {}
    # (centre, half width) of the bulk, and the planted (min, max)
    spec = {"u": (0.0, 1.0, -3.5, 4.25), "v": (0.25, 0.5, -2.75, 3.125),
            "w": (-0.5, 0.75, -5.5, 2.5), "p": (10.0, 4.0, 1.5, 20.75),
            "rho": (1.0, 0.25, 0.5, 1.75), "T": (300.0, 15.0, 270.25, 333.5)}
    last = n - 1
    first_plane_last_col = (ny // 2) * nx + nx - 1
    last_plane = (nz - 1) * nx * ny
    # (min cell, max cell); None: a seeded cell
    cells = {"u": (last, 0), "v": (None, first_plane_last_col), "w": (0, last_plane + nx // 2),
             "p": (None, None), "rho": (None, None), "T": (None, None)}
    for name in FIELDS:
        c, h, lo, hi = spec[name]
        if integer:
            a = rng.integers(-1000, 1001, size=(nz, ny, nx)).astype(np.float64)
            a += float(round(c)) * 8.0
            lo, hi = float(round(c)) * 8.0 - 2000.0 - 7.0, float(round(c)) * 8.0 + 2000.0 + 9.0
        else:
            a = c + h * rng.uniform(-1.0, 1.0, size=(nz, ny, nx))
            lo, hi = lo + 1e-3 * rng.uniform(), hi + 1e-3 * rng.uniform()
        lo_cell, hi_cell = cells[name]
        if lo_cell is not None and lo_cell == hi_cell:  # degenerate shapes only
            hi_cell = (lo_cell + 1) % n
        _plant(a, rng, lo_cell, hi_cell, lo, hi)
        out[name] = a
    return out


def csv_step_args(step):
    """(time, dt, iterations, residual, elapsed_time_ms) of CSV step `step`."""
    return (0.0125 * step, 1.25e-3, 17 + 3 * step, 3.7e-7 / (step + 1), 12.345 + 100.0 * step)


def grid_extent(case):
    nx, ny, nz = case["shape"]
    return dict(xmin=0.0, xmax=2.0, ymin=-0.5, ymax=1.0, zmin=0.0, zmax=1.0 if nz > 1 else 0.0)


def csv_keys():
    """Names of the recorded CSV texts of one CSV case."""
    keys = []
    for mag in (0, 1):
        keys += [f"timeseries_mag{mag}", f"statistics_mag{mag}", f"centerline_h_mag{mag}",
                 f"centerline_v_mag{mag}"]
    return keys


def boundary_clear(x: float, rel: float = 1e-9) -> bool:
    """True when x is at least rel * |x| away from every value at which its
    %.6e text changes (the midpoints between neighbouring 7-digit decimals)."""
    if x == 0.0 or not math.isfinite(x):
        return True
    from decimal import Decimal
    d = Decimal(abs(x))
    e = d.adjusted()
    unit = Decimal(10) ** (e - 6)
    frac = (d / unit) % 1  # position between two 7-digit neighbours
    return abs(frac - Decimal("0.5")) * unit >= Decimal(rel) * d
