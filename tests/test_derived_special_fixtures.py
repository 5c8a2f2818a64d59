"""The NaN / signed-zero / inf / extreme cases of tests/derived_special_cases.py
on the CPU: the host mirror (libcfd_host.so) against the reference's record
(tests/golden/derived_special_cases.json, written by tests/golden/
make_derived_golden.py --special), a numpy statement of the contract against
the host mirror on every case (which pins the asserted values of the shapes
from 1000 cells on, where the reference takes its OpenMP path), and a numpy
model of the rule the device pass used before (a NaN-ignoring fold from +-inf
identities with -0 < +0) against the record: it must miss the record on every
nan_first, nan_all and zeros case and meet it on every nan_but_first,
nan_edges and inf case, so the GPU tests see the former and pin the latter.
"""
import json
import math
from pathlib import Path

import numpy as np
import pytest

from cfd_amd import _abi as A
from cfd_amd import api
from tests import derived_cases as K
from tests import derived_special_cases as S
from tests.special_values import assert_bits_equal

GOLDEN = Path(__file__).resolve().parent / "golden"
IDS = [c["name"] for c in S.CASES]
SMALL = [c for c in S.CASES if np.prod(c["shape"]) < S.OMP_THRESHOLD]


@pytest.fixture(scope="module")
def record():
    return json.loads((GOLDEN / S.JSON_FILE).read_text())


def host_derived(case, arrs, with_mag=True):
    """(DerivedFields of the host mirror, its FlowField); w = NULL while the
    mirror reads a case whose w is absent."""
    f = api.FlowField(*case["shape"])
    for k in S.FIELDS:
        getattr(f, k)[...] = arrs[k]
    d = api.DerivedFields(*case["shape"])
    c = f.ptr.contents
    keep = c.w
    if case["w_absent"]:
        c.w = None
    try:
        if with_mag:
            d.compute_velocity_magnitude(f)
        d.compute_statistics(f)
    finally:
        c.w = keep
    return d, f


def stats_hex(dc):
    return {k: {m: S.hexbits(getattr(getattr(dc, k + "_stats"), m + "_val"))
                for m in ("min", "max", "sum", "avg")} for k in S.STATS}


def test_case_table():
    assert len(IDS) == len(set(IDS))
    for s in S.SHAPES:
        classes = {c["cls"] for c in S.CASES if c["name"].startswith(s + "_")}
        assert classes == set(S.BUG_CLASSES + S.PIN_CLASSES + ("mag_extreme",)), s
    for cls in S.BUG_CLASSES + S.PIN_CLASSES:
        assert {c["probe"] for c in S.CASES if c["cls"] == cls} == set(S.PROBED), cls
    assert sum(np.prod(s) < S.OMP_THRESHOLD for s in S.SHAPES.values()) == 3
    assert [c["name"] for c in S.CASES if c["w_absent"]] == ["s3_mag_extreme"]
    # the "round" pair: the first zero in the last workgroup's first round of
    # rows, the later one in workgroup 0's second round
    nx, ny, nz = S.SHAPES["s96"]
    first, later = S.zero_pair((nx, ny, nz), "round")
    grid = min((ny * nz + S.DS_WAVES - 1) // S.DS_WAVES, S.DS_MAX_WG)
    r0, r1 = first // nx, later // nx
    assert r0 < S.DS_WAVES * grid and r0 // S.DS_WAVES == grid - 1
    assert r1 >= S.DS_WAVES * grid and (r1 // S.DS_WAVES) % grid == 0
    for shape in S.SHAPES.values():
        a, b = S.zero_pair(shape, "pair")
        # one 16-byte pair: columns 2 q and 2 q + 1 of one row
        assert (a % shape[0]) % 2 == 0 and b == a + 1 and a // shape[0] == b // shape[0]
        a, b = S.zero_pair(shape, "seam")
        assert a == shape[0] - 1 and b == shape[0]


@pytest.mark.parametrize("case", S.CASES, ids=IDS)
def test_inputs_match_the_record_and_their_class(record, case):
    rec = record["cases"][case["name"]]
    arrs = S.inputs(case)
    assert rec["shape"] == list(case["shape"]) and rec["cls"] == case["cls"]
    assert rec["probe"] == case["probe"]
    for k in S.FIELDS:
        assert K.sha(arrs[k]) == rec["inputs"][k], f"{k}: the seeded input changed"
    if case["cls"] == "mag_extreme":
        return
    for k in S.FIELDS:
        if k != case["probe"]:
            assert np.all(np.isfinite(arrs[k])) and not np.any(arrs[k] == 0.0), k
    flat = arrs[case["probe"]].reshape(-1)
    nx, ny, nz = case["shape"]
    cls, var = case["cls"], case["variant"]
    isn = np.isnan(flat)
    if cls == "nan_first":
        assert isn[0] and isn.sum() == 1 and int(S.bits(flat)[0]) == int(S.NAN_VARIANTS[var])
    elif cls == "nan_all":
        assert isn.all() and np.all(S.bits(flat) == S.QNAN)
    elif cls == "nan_but_first":
        assert not isn[0] and isn[1:].all()
    elif cls == "nan_edges":
        cells = np.flatnonzero(isn).tolist()
        assert len(cells) == 3 and flat.size - 1 in cells and 0 not in cells
        assert (nz // 2 * ny + ny // 2) * nx + nx - 1 in cells
        third = [c for c in cells if c not in (flat.size - 1, (nz // 2 * ny + ny // 2) * nx + nx - 1)]
        ext = (int(np.nanargmax(flat)), int(np.nanargmin(flat)))
        assert len(third) == 1 and min(abs(third[0] - e) for e in ext) == 1
    elif cls == "inf":
        assert not isn.any()
        assert int((flat == np.inf).sum()) == (var in ("pinf", "both"))
        assert int((flat == -np.inf).sum()) == (var in ("ninf", "both"))
    elif var in ("allneg", "allpos"):
        assert np.all(flat == 0.0) and np.signbit(flat[0]) == (var == "allneg")
        assert np.all(np.signbit(flat[1:]) == (var == "allpos"))
    else:
        zeros = np.flatnonzero(flat == 0.0).tolist()
        assert zeros == list(S.zero_pair(case["shape"], var.split("_")[1]))
        neg = var.startswith("nonpos")
        assert np.all(flat <= 0.0) if neg else np.all(flat >= 0.0)
        assert bool(np.signbit(flat[zeros[0]])) == neg and bool(np.signbit(flat[zeros[1]])) != neg


@pytest.mark.parametrize("case", [c for c in S.CASES if c["cls"] == "mag_extreme"],
                         ids=lambda c: c["name"])
def test_mag_extreme_inputs_reach_every_regime(case):
    arrs = S.inputs(case)
    census = S.mag_census(arrs)
    print(case["name"], census)
    for key in ("subnormal_square", "flushed_square", "overflow_magnitude", "inf_magnitude",
                "nan_magnitude", "zero_components", "negative_zero_components"):
        assert census[key] >= 1, (key, census)
    comps = np.stack([arrs[k].reshape(-1) for k in ("u", "v", "w")])
    assert np.isnan(comps).sum() == 1 and np.isinf(comps).sum() == 1
    assert np.all(arrs["w"] == 0.0) == case["w_absent"]
    if case["w_absent"]:
        assert not np.signbit(arrs["w"]).any()


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c["name"])
def test_host_mirror_reproduces_the_reference_record(record, case):
    """Under 1000 cells the record is the reference's own sequential loop."""
    rec = record["cases"][case["name"]]
    assert "openmp_path" not in rec
    arrs = S.inputs(case)
    d, _ = host_derived(case, arrs)
    assert S.sha_nan_canonical(d.velocity_magnitude) == rec["vel_mag_sha256"]
    got = stats_hex(d.c)
    for k in S.STATS:
        for m in ("min", "max"):
            assert got[k][m] == rec["stats"][k][m], (k, m)
        for m in ("sum", "avg"):
            g, w = (S.from_bits(int(v, 16)) for v in (got[k][m], rec["stats"][k][m]))
            # a sum's NaN: isnan only (the contract); anything else, the bits
            assert (math.isnan(g) and math.isnan(w)) or got[k][m] == rec["stats"][k][m], (k, m)
    if case["name"] == S.NPZ_CASE:
        assert_bits_equal(d.velocity_magnitude, np.load(GOLDEN / S.NPZ_FILE)["vel_mag"],
                          what="host velocity magnitude")


@pytest.mark.parametrize("case", S.CASES, ids=IDS)
def test_numpy_contract_equals_the_host_mirror_and_the_record(record, case):
    """Every shape: the asserted record (`stats`) is the sequential loop."""
    rec = record["cases"][case["name"]]
    assert ("openmp_path" in rec) == (int(np.prod(case["shape"])) >= S.OMP_THRESHOLD)
    arrs = S.inputs(case)
    d, _ = host_derived(case, arrs)
    mag = S.magnitude(arrs)
    assert_bits_equal(d.velocity_magnitude, mag, what="host magnitude against numpy")
    assert S.sha_nan_canonical(mag) == rec["vel_mag_sha256"]
    got = stats_hex(d.c)
    data = dict(arrs, vel_mag=d.velocity_magnitude)
    for k in S.STATS:
        mn, mx, _ = S.contract(data[k])
        assert got[k]["min"] == S.hexbits(mn) == rec["stats"][k]["min"], k
        assert got[k]["max"] == S.hexbits(mx) == rec["stats"][k]["max"], k
        s = getattr(d.c, k + "_stats")
        S.check_sum(s.sum_val, s.avg_val, data[k], f"{case['name']} {k} (host)")
        r = rec["stats"][k]
        S.check_sum(S.from_bits(int(r["sum"], 16)), S.from_bits(int(r["avg"], 16)), data[k],
                    f"{case['name']} {k} (record)")


@pytest.mark.parametrize("case", [c for c in S.CASES if c["cls"] != "mag_extreme"],
                         ids=lambda c: c["name"])
def test_the_former_device_rule_misses_exactly_the_bug_classes(record, case):
    rec = record["cases"][case["name"]]["stats"]
    arrs = S.inputs(case)
    k = case["probe"]
    mn, mx = S.parent_rule(arrs[k])
    meets = S.hexbits(mn) == rec[k]["min"] and S.hexbits(mx) == rec[k]["max"]
    assert meets == (case["cls"] in S.PIN_CLASSES), (case["name"], mn, mx, rec[k])
    # the unprobed fields are regular: both rules agree on them
    for o in S.FIELDS:
        if o != k:
            mn, mx = S.parent_rule(arrs[o])
            assert (S.hexbits(mn), S.hexbits(mx)) == (rec[o]["min"], rec[o]["max"]), o
    # the magnitude follows the same rules (u enters it; p and T do not)
    mag = S.magnitude(arrs)
    mn, mx = S.parent_rule(mag)
    meets = S.hexbits(mn) == rec["vel_mag"]["min"] and S.hexbits(mx) == rec["vel_mag"]["max"]
    nan0 = k == "u" and case["cls"] in ("nan_first", "nan_all")
    assert meets == (not nan0), (case["name"], "vel_mag")


def test_openmp_path_as_recorded(record):
    """Informative: where the reference's OpenMP reduction (1000 cells and
    more, one thread) was recorded to differ from its own sequential loop."""
    differs = {n: r["openmp_path_differs"] for n, r in record["cases"].items()
               if r.get("openmp_path_differs")}
    print("openmp_path differs on:", differs or "no case")
    for n, r in record["cases"].items():
        if "openmp_path" in r:
            assert sorted(r["openmp_path"]) == sorted(S.STATS)


@pytest.mark.parametrize("name", list(S.CSV_CASES))
@pytest.mark.parametrize("mag", [0, 1])
def test_host_csv_files_match_byte_for_byte(record, tmp_path, name, mag):
    steps = S.CSV_CASES[name]
    want = record["csv"][name]
    nx, ny, nz = steps[0]["shape"]
    g = api.Grid(nx, ny, nz, **K.grid_extent(steps[0]))
    ts, st = tmp_path / "ts.csv", tmp_path / "st.csv"
    for step, case in enumerate(steps):
        d, f = host_derived(case, S.inputs(case, step), bool(mag))
        t, dt, its, res, ms = K.csv_step_args(step)
        prm = A.SolverParams()
        prm.dt = dt
        stats = A.SolverStats()
        stats.iterations, stats.residual, stats.elapsed_time_ms = its, res, ms
        api.write_csv_timeseries(str(ts), step, t, f, d, prm, stats, step == 0)
        api.write_csv_statistics(str(st), step, t, f, d, step == 0)
        if step == 0:
            for tag, direction in (("h", A.PROFILE_HORIZONTAL), ("v", A.PROFILE_VERTICAL)):
                cl = tmp_path / f"cl{tag}.csv"
                api.write_csv_centerline(str(cl), f, d, g, direction)
                assert cl.read_bytes() == want[f"centerline_{tag}_mag{mag}"].encode(), tag
    assert ts.read_bytes() == want[f"timeseries_mag{mag}"].encode()
    assert st.read_bytes() == want[f"statistics_mag{mag}"].encode()
    text = st.read_text()
    assert ("nan" in text) == (name == "nan_all_p") and "inf" not in text
    assert ("-0.000000e+00" in text) == (name == "zeros_u")


@pytest.mark.parametrize("name", list(S.CSV_CASES))
def test_csv_averages_are_clear_of_rounding_boundaries(name):
    """The device sums in another order: a finite average must not sit where
    the last bits of the sum decide its %.6e text."""
    for step, case in enumerate(S.CSV_CASES[name]):
        arrs = dict(S.inputs(case, step))
        arrs["vel_mag"] = S.magnitude(arrs)
        for k, a in arrs.items():
            avg = math.fsum(a.reshape(-1).tolist()) / a.size
            assert K.boundary_clear(avg, 1e-9), (name, step, k, avg)
