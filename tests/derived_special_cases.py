"""Blown-up, signed-zero and extreme fields for the field statistics and the
velocity magnitude (tests/test_derived_special_fixtures.py, tests/
test_gpu_derived.py) and for the script that records the reference on them
(tests/golden/make_derived_golden.py --special ->
tests/golden/derived_special_cases.json). Pure numpy.

The contract (`contract` below) is the reference's sequential loop
(derived_fields.c:107-120; cfd_amd/csrc/host/derived_host.c): min and max start
at data[0] and move on strict `<` / `>`, so
  min, max   cell 0 is NaN: that NaN's 64 bits. Otherwise the least / greatest
             non-NaN value; where it is a zero, the sign of the zero with the
             lowest packed index k nx ny + j nx + i.
  sum, avg   NaN if any cell is NaN or both infinities occur (isnan only: sign
             and payload are not part of the contract); +-inf for infinities of
             one sign; otherwise within n 2^-53 sum|x| of the exact sum.

Shapes: the smallest that reach each part of the device reduction that carries
the cell-0 value and the first-zero index.
  3x3x1     one workgroup, 2-D
  17x13x4   884 cells: pad columns, odd nx
  67x14x1   938 cells in 14 rows: a lane's second pair (a device context
            takes nz = 1 or nz >= 3, so the 14 rows lie in one plane)
  261x5x3   a lane's third pair, odd nx
  130x34x3  several workgroups
  96x96x48  the capped grid's second round of rows, the ticket over 1024
            workgroups
The first three stay under 1000 cells, where the reference runs its sequential
loop; from 1000 cells on it runs an OpenMP min / max reduction whose result
with a NaN operand is the compiler's choice (recorded as `openmp_path`,
informative only).

Classes (the probed field rotates over u, p, T; every other field is a regular
seeded field of tests/derived_cases.py):
  nan_first      NaN at cell 0 only: the positive quiet NaN, and on 3x3x1 and
                 17x13x4 also 0xFFF8000000000001
  nan_all        every cell the positive quiet NaN
  nan_but_first  every cell but cell 0
  nan_edges      NaN in the last cell, in the last column of a middle row (the
                 pair half next to the pad) and next to a planted extreme
  zeros          allneg / allpos: an all-zero field with -0 (+0) at cell 0 and
                 the other sign elsewhere; nonneg / nonpos: a field >= 0 (<= 0)
                 whose only zeros are a +0 (-0) and a later -0 (+0), placed
                 where index order and processing order disagree:
                   seam   last column of row 0, then column 0 of row 1
                   pair   the two halves of one 16-byte pair
                   round  (96x96x48) a row of the last workgroup's first round,
                          then a row workgroup 0 takes in its second round
  inf            a single +inf, a single -inf, both
  mag_extreme    u, v, w scaled per cell by 2^-600, 2^-530, 2^-512, 1, 2^511 or
                 2^520 (squares that vanish, are subnormal, normal, overflow),
                 with exact +-0 components, one NaN and one inf component; on
                 3x3x1 w is absent (w_i = 0.0; a device context holds zeros)
"""
import hashlib
import math

import numpy as np

from tests import derived_cases as K

FIELDS = K.FIELDS
STATS = K.STATS
RHO0 = K.RHO0
JSON_FILE = "derived_special_cases.json"
NPZ_FILE = "derived_special_vel_mag_17x13x4.npz"
NPZ_CASE = "s17_mag_extreme"
OMP_THRESHOLD = 1000  # cells from which the reference takes its OpenMP path

SHAPES = {"s3": (3, 3, 1), "s17": (17, 13, 4), "s67": (67, 14, 1), "s261": (261, 5, 3),
          "s130": (130, 34, 3), "s96": (96, 96, 48)}
_SEEDS = {"s3": 31, "s17": 32, "s67": 33, "s261": 34, "s130": 35, "s96": 36}
PROBED = ("u", "p", "T")
QNAN = np.uint64(0x7FF8000000000000)
NAN_VARIANTS = {"pos": np.uint64(0x7FF8000000000000), "neg1": np.uint64(0xFFF8000000000001)}
SCALES = (-600, -530, -512, 0, 511, 520)
DS_WAVES, DS_MAX_WG = 4, 1024  # rows per workgroup and the grid cap of k_derived_stats

BUG_CLASSES = ("nan_first", "nan_all", "zeros")      # the parent's rule disagrees
PIN_CLASSES = ("nan_but_first", "nan_edges", "inf")  # it agrees; the tests pin


def from_bits(b):
    return np.array([b], dtype=np.uint64).view(np.float64)[0]


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def hexbits(x) -> str:
    return f"{int(bits(np.float64(x)).reshape(-1)[0]):016x}"


def sha_nan_canonical(a) -> str:
    """sha256 of the array's bytes with every NaN replaced by the positive
    quiet NaN."""
    b = bits(a).copy()
    b[np.isnan(np.asarray(a, dtype=np.float64))] = QNAN
    return hashlib.sha256(b.tobytes()).hexdigest()


def _cases():
    out = []
    for s, shape in SHAPES.items():
        variants = [("nan_first", v) for v in (("pos", "neg1") if s in ("s3", "s17") else ("pos",))]
        variants += [("nan_all", None), ("nan_but_first", None), ("nan_edges", None)]
        variants += [("zeros", "allneg"), ("zeros", "allpos")]
        places = ("seam", "pair") + (("round",) if s == "s96" else ())
        variants += [("zeros", f"{sub}_{pl}") for sub in ("nonneg", "nonpos") for pl in places]
        variants += [("inf", v) for v in ("pinf", "ninf", "both")]
        variants += [("mag_extreme", None)]
        for n, (cls, var) in enumerate(variants):
            out.append({"name": f"{s}_{cls}" + (f"_{var}" if var else ""), "shape": shape,
                        "cls": cls, "variant": var, "seed": _SEEDS[s] * 100 + n,
                        "probe": "uvw" if cls == "mag_extreme" else PROBED[len(out) % 3],
                        "w_absent": cls == "mag_extreme" and s == "s3"})
    return out


CASES = _cases()
BY_NAME = {c["name"]: c for c in CASES}


def with_probe(case, probe, seed):
    return dict(case, probe=probe, seed=seed)


# CSV: three appended steps each, 17x13x4; (case, step) per row. No NaN is
# generated in them, only propagated from the positive quiet NaN.
CSV_STEPS = 3
CSV_CASES = {
    "nan_all_p": [with_probe(BY_NAME["s17_nan_all"], "p", 3250)] * 3,
    "zeros_u": [with_probe(BY_NAME["s17_zeros_nonneg_seam"], "u", 3260),
                with_probe(BY_NAME["s17_zeros_allneg"], "u", 3260),
                with_probe(BY_NAME["s17_zeros_nonpos_pair"], "u", 3260)],
}


def _cell(shape, k, j, i):
    nx, ny, _ = shape
    return (k * ny + j) * nx + i


def zero_pair(shape, place):
    """Packed indices (first, later) of the two zeros of a nonneg / nonpos case."""
    nx, ny, nz = shape
    if place == "seam":
        return _cell(shape, 0, 0, nx - 1), _cell(shape, 0, 1, 0)
    if place == "pair":
        i0 = 2 * ((nx // 2) // 2)
        return _cell(shape, nz // 2, ny // 2, i0), _cell(shape, nz // 2, ny // 2, i0 + 1)
    assert place == "round"
    nrows = ny * nz
    grid = min((nrows + DS_WAVES - 1) // DS_WAVES, DS_MAX_WG)
    assert nrows > DS_WAVES * grid, "no second round of rows at this shape"
    r_first = DS_WAVES * (grid - 1) + 1  # wave 1 of the last workgroup, first round
    r_later = DS_WAVES * grid + 1        # wave 1 of workgroup 0, second round
    return r_first * nx + nx // 3, r_later * nx + nx // 5


def nan_edge_cells(a):
    """The three NaN cells of a nan_edges case on the finite field a."""
    nz, ny, nx = a.shape
    n = a.size
    cells = [n - 1, (nz // 2 * ny + ny // 2) * nx + nx - 1]
    flat = a.reshape(-1).copy()
    flat[cells] = np.nan
    hi, lo = int(np.nanargmax(flat)), int(np.nanargmin(flat))
    for c in (hi + 1, hi - 1, lo + 1, lo - 1):
        if 0 < c < n and c not in cells and c not in (hi, lo):
            return cells + [c]
    raise AssertionError("no free neighbour of an extreme")


def _mag_extreme(case, base, rng):
    nx, ny, nz = case["shape"]
    n = nx * ny * nz
    perm = rng.permutation(n)
    common = np.empty(n, dtype=np.int64)
    common[perm] = np.arange(n) % len(SCALES)  # every scale occurs on >= 1 cell
    out = {}
    for q, name in enumerate(("u", "v", "w")):
        own = rng.integers(0, len(SCALES), size=n)
        idx = np.where(rng.random(n) < 0.25, own, common)
        idx[perm[:9]] = common[perm[:9]]
        a = np.ldexp(base[name].reshape(-1), np.array(SCALES)[idx])
        z = rng.random(n) < 0.02
        z[perm[:6]] = False
        a[z] = np.where(rng.random(n) < 0.5, -0.0, 0.0)[z]
        out[name] = a
    # cells perm[6 .. 8] repeat the scales of perm[0 .. 2]
    out["u"][perm[6]] = from_bits(NAN_VARIANTS["pos"])
    out["v"][perm[7]] = np.inf
    out["u"][perm[8]] = 0.0
    out["v"][perm[8]] = -0.0
    if case["w_absent"]:
        out["w"][:] = 0.0
    return {k: v.reshape(nz, ny, nx) for k, v in out.items()}


def inputs(case, step=0):
    """{name: (nz, ny, nx) float64 array} of u, v, w, p, rho, T."""
    nx, ny, nz = case["shape"]
    n = nx * ny * nz
    out = K.inputs({"shape": case["shape"], "kind": "real", "seed": case["seed"]}, step)
    rng = np.random.default_rng([case["seed"], step, 7])
    cls, var = case["cls"], case["variant"]
    if cls == "mag_extreme":
        out.update(_mag_extreme(case, out, rng))
        return out
    a = out[case["probe"]]
    flat = a.reshape(-1)
    nan = from_bits(NAN_VARIANTS["pos"])
    if cls == "nan_first":
        flat[0] = from_bits(NAN_VARIANTS[var])
    elif cls == "nan_all":
        flat[:] = nan
    elif cls == "nan_but_first":
        flat[1:] = nan
    elif cls == "nan_edges":
        flat[nan_edge_cells(a)] = nan
    elif cls == "inf":
        hi, lo = int(np.argmax(flat)), int(np.argmin(flat))
        free = [int(c) for c in rng.permutation(n)[:5] if c not in (0, hi, lo)]
        free += [c for c in range(1, 9) if c not in free][:2]  # 3x3x1 may run short
        if var in ("pinf", "both"):
            flat[free[0]] = np.inf
        if var in ("ninf", "both"):
            flat[free[1]] = -np.inf
    elif cls == "zeros":
        if var in ("allneg", "allpos"):
            flat[:] = 0.0 if var == "allneg" else -0.0
            flat[0] = -0.0 if var == "allneg" else 0.0
        else:
            sub, place = var.split("_")
            first, later = zero_pair(case["shape"], place)
            assert first < later
            np.abs(flat, out=flat)
            flat[flat == 0.0] = 1.0
            if sub == "nonpos":
                np.negative(flat, out=flat)
            flat[first] = 0.0 if sub == "nonneg" else -0.0
            flat[later] = -0.0 if sub == "nonneg" else 0.0
    else:
        raise ValueError(cls)
    return out


def magnitude(arrs):
    """The reference's expression (derived_fields.c:175) in numpy."""
    u, v, w = arrs["u"], arrs["v"], arrs["w"]
    with np.errstate(all="ignore"):
        return np.sqrt((u * u) + (v * v) + (w * w))


def _zero_sign(flat, value):
    if value != 0.0:
        return value
    return flat[int(np.flatnonzero(flat == 0.0)[0])]


def contract(a):
    """(min, max, sum class) of the contract; sum class: "nan", "+inf", "-inf"
    or "finite"."""
    flat = np.asarray(a, dtype=np.float64).reshape(-1)
    isn = np.isnan(flat)
    if isn[0]:
        mn = mx = flat[0]
    else:
        vals = flat[~isn]
        mn, mx = _zero_sign(flat, vals.min()), _zero_sign(flat, vals.max())
    pinf, ninf = bool(np.any(flat == np.inf)), bool(np.any(flat == -np.inf))
    if isn.any() or (pinf and ninf):
        cls = "nan"
    elif pinf or ninf:
        cls = "+inf" if pinf else "-inf"
    else:
        cls = "finite"
    return mn, mx, cls


def parent_rule(a):
    """(min, max) of the rule this contract replaced: a NaN-ignoring fold from
    +inf / -inf identities in which -0 orders below +0."""
    flat = np.asarray(a, dtype=np.float64).reshape(-1)
    vals = flat[~np.isnan(flat)]
    if vals.size == 0:
        return np.float64(np.inf), np.float64(-np.inf)
    mn, mx = vals.min(), vals.max()
    zeros = vals[vals == 0.0]
    if mn == 0.0:
        mn = np.float64(-0.0) if np.signbit(zeros).any() else np.float64(0.0)
    if mx == 0.0:
        mx = np.float64(0.0) if (~np.signbit(zeros)).any() else np.float64(-0.0)
    return mn, mx


def check_sum(sum_val, avg_val, data, what=""):
    """sum and avg of one quantity against the contract."""
    flat = np.asarray(data, dtype=np.float64).reshape(-1)
    n = flat.size
    cls = contract(flat)[2]
    if cls == "nan":
        assert math.isnan(sum_val) and math.isnan(avg_val), (what, sum_val, avg_val)
    elif cls != "finite":
        want = math.inf if cls == "+inf" else -math.inf
        assert sum_val == want and avg_val == want, (what, sum_val, avg_val)
    else:
        assert avg_val == sum_val / float(n), what
        exact = math.fsum(flat.tolist())
        bound = n * 2.0 ** -53 * math.fsum(np.abs(flat).tolist())
        assert abs(sum_val - exact) <= bound, (what, sum_val, exact, bound)


def mag_census(arrs):
    """Cells of a mag_extreme case by what their squares do."""
    comps = np.stack([arrs[k].reshape(-1) for k in ("u", "v", "w")])
    with np.errstate(all="ignore"):
        sq = comps * comps
    tiny = np.finfo(np.float64).tiny
    mag = magnitude(arrs).reshape(-1)
    finite = np.all(np.isfinite(comps), axis=0)
    return {"subnormal_square": int(np.any((sq > 0.0) & (sq < tiny), axis=0).sum()),
            "flushed_square": int(np.any((comps != 0.0) & (sq == 0.0), axis=0).sum()),
            "overflow_magnitude": int((np.isinf(mag) & finite).sum()),
            "inf_magnitude": int(np.isinf(mag).sum()),
            "nan_magnitude": int(np.isnan(mag).sum()),
            "zero_components": int((comps == 0.0).sum()),
            "negative_zero_components": int(((comps == 0.0) & np.signbit(comps)).sum())}
