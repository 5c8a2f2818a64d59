"""Device-side field statistics, velocity magnitude and CSV outputs
(hip_proj_field_statistics / _derived_statistics / _velocity_magnitude /
_write_csv_*, cfd_amd/csrc/hip/derived_stats.hip) against the reference's
recorded results (tests/golden/derived_cases.json) on the shapes of
tests/derived_cases.py.

min and max are exact. Sums: on integer-valued fields every order is exact, so
sum and avg are the reference's bits; on real-valued fields
|sum_dev - fsum(x)| <= n * 2^-53 * sum|x|, the worst-case bound of any
summation order (derived, not measured; one dropped or doubled cell is orders
of magnitude above it on these fields).

The second half holds the entries to the contract of
tests/derived_special_cases.py on NaN, signed-zero, inf and extreme fields
(tests/golden/derived_special_cases.json): min and max as 64-bit patterns,
sum and avg by their class, the magnitude cell by cell, the CSV files byte
for byte.
"""
import ctypes as C
import json
import math
from pathlib import Path

import numpy as np
import pytest

from cfd_amd import _abi as A
from cfd_amd import api
from tests import cases
from tests import derived_cases as K
from tests import derived_special_cases as S
from tests.special_values import assert_bits_equal

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
FID = {"u": A.HIP_FIELD_U, "v": A.HIP_FIELD_V, "w": A.HIP_FIELD_W, "p": A.HIP_FIELD_P,
       "rho": A.HIP_FIELD_RHO, "T": A.HIP_FIELD_T}


ENTRIES = ("field_statistics", "derived_statistics", "velocity_magnitude",
           "write_csv_timeseries", "write_csv_statistics", "write_csv_centerline")


@pytest.fixture(scope="session", autouse=True)
def monitoring_entries_present():
    """Every test here needs the monitoring entries: without them in the
    bindings each test fails at once, before any device or context is set up."""
    missing = [e for e in ENTRIES if not hasattr(api.HipProjection, e)]
    missing += [n for n in ("FieldStats", "DerivedFields") if not hasattr(A, n)]
    assert not missing, f"the bindings lack the monitoring entries: {missing}"


@pytest.fixture(scope="module")
def record():
    return json.loads((GOLDEN / K.JSON_FILE).read_text())


@pytest.fixture(scope="module")
def loaded(hip_lib):
    """name -> (context holding the case's six fields, the host arrays); built
    once, never modified by a test (tests that change fields make their own)."""
    cache = {}

    def get(name):
        if name not in cache:
            case = K.BY_NAME[name]
            ctx = api.HipProjection(*case["shape"])
            arrs = K.inputs(case)
            for k in K.FIELDS:
                ctx.set_field(FID[k], arrs[k])
            cache[name] = (ctx, arrs)
        return cache[name]

    yield get
    for ctx, _ in cache.values():
        ctx.close()


def stats_tuple(s):
    return (s.min_val, s.max_val, s.avg_val, s.sum_val)


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def check_sum(s, data, kind, rec, what):
    flat = np.asarray(data, dtype=np.float64).reshape(-1)
    n = flat.size
    assert s.avg_val == s.sum_val / float(n), what
    if kind == "int":
        assert float(s.sum_val).hex() == rec["sum"] and float(s.avg_val).hex() == rec["avg"], what
        return
    exact = math.fsum(flat.tolist())
    bound = n * 2.0 ** -53 * math.fsum(np.abs(flat).tolist())
    err = abs(s.sum_val - exact)
    print(f"{what}: |sum_dev - fsum| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (what, s.sum_val, exact, bound)


@pytest.mark.parametrize("case", K.CASES, ids=lambda c: c["name"])
def test_against_the_record(record, loaded, case):
    rec = record["cases"][case["name"]]
    ctx, arrs = loaded(case["name"])
    d = ctx.derived_statistics(True, K.RHO0)
    assert d.stats_computed == 1 and not d.velocity_magnitude
    mag = ctx.velocity_magnitude()
    assert K.sha(mag) == rec["vel_mag_sha256"]
    if case["name"] == K.NPZ_CASE:
        assert_bits_equal(mag, np.load(GOLDEN / K.NPZ_FILE)["vel_mag"], what="velocity magnitude")
    data = dict(arrs, vel_mag=mag)
    for k in K.STATS:
        s = getattr(d, k + "_stats")
        r = rec["stats"][k]
        assert s.min_val == float.fromhex(r["min"]), (k, s.min_val, r["min"])
        assert s.max_val == float.fromhex(r["max"]), (k, s.max_val, r["max"])
        # the magnitude of integer-valued fields is not integer-valued
        kind = "real" if k == "vel_mag" else case["kind"]
        check_sum(s, data[k], kind, r, f"{case['name']} {k}")
    # the single-field pass walks the same rows in the same order
    for k in K.FIELDS:
        one = ctx.field_statistics(FID[k])
        assert bits(stats_tuple(one)).tolist() == bits(stats_tuple(getattr(d, k + "_stats"))).tolist()
    # without the magnitude: the other six unchanged, vel_mag_stats left alone
    d0 = ctx.derived_statistics(False, K.RHO0)
    assert stats_tuple(d0.vel_mag_stats) == (0.0, 0.0, 0.0, 0.0)
    for k in K.FIELDS:
        assert bits(stats_tuple(getattr(d0, k + "_stats"))).tolist() == \
            bits(stats_tuple(getattr(d, k + "_stats"))).tolist()


@pytest.mark.parametrize("shape", list(K.SHAPES.values()), ids=list(K.SHAPES))
def test_padding_and_coverage(hip_lib, shape):
    nx, ny, nz = shape
    n = nx * ny * nz
    rng = np.random.default_rng([7, nx, ny, nz])
    ctx = api.HipProjection(nx, ny, nz)
    try:
        # a pad value (the pad columns hold zeros) must not lower a positive
        # min nor raise a negative max
        pos = rng.uniform(1.0, 2.0, size=(nz, ny, nx))
        for fid, a in ((A.HIP_FIELD_U, pos), (A.HIP_FIELD_V, -pos), (A.HIP_FIELD_W, pos),
                       (A.HIP_FIELD_P, -pos)):
            ctx.set_field(fid, a)
        d = ctx.derived_statistics(True, 1.0)
        for s, a in ((d.u_stats, pos), (d.v_stats, -pos), (d.w_stats, pos), (d.p_stats, -pos)):
            assert s.min_val == a.min() and s.max_val == a.max()
        m = np.sqrt((pos * pos) + (pos * pos) + (pos * pos))
        assert d.vel_mag_stats.min_val == m.min() and d.vel_mag_stats.max_val == m.max()
        # all ones: the sum counts every cell once
        ctx.set_field(A.HIP_FIELD_U, np.ones((nz, ny, nx)))
        s = ctx.field_statistics(A.HIP_FIELD_U)
        assert stats_tuple(s) == (1.0, 1.0, 1.0, float(n))
        # a single 1.0 in a zero field: the corners, the last column, seeded cells
        cells = {(k, j, i) for k in (0, nz - 1) for j in (0, ny - 1) for i in (0, nx - 1)}
        cells.add((nz // 2, ny // 2, nx - 1))
        for flat in rng.choice(n, size=min(8, n), replace=False):
            cells.add(tuple(int(v) for v in np.unravel_index(int(flat), (nz, ny, nx))))
        for cell in sorted(cells):
            a = np.zeros((nz, ny, nx))
            a[cell] = 1.0
            ctx.set_field(A.HIP_FIELD_U, a)
            s = ctx.field_statistics(A.HIP_FIELD_U)
            assert (s.min_val, s.max_val, s.sum_val) == (0.0, 1.0, 1.0), cell
            assert s.avg_val == 1.0 / n
    finally:
        ctx.close()


def test_nan_convention(record, hip_lib):
    case = K.BY_NAME["s17_real"]
    rec = record["cases"][case["name"]]["stats"]
    arrs = K.inputs(case)
    u = arrs["u"].copy()
    cell = (5, 6, 7)  # away from index 0 and from the planted extremes
    assert u[cell] not in (u.min(), u.max())
    u[cell] = np.nan
    ctx = api.HipProjection(*case["shape"])
    try:
        for k in K.FIELDS:
            ctx.set_field(FID[k], u if k == "u" else arrs[k])
        d = ctx.derived_statistics(True, K.RHO0)
        assert d.u_stats.min_val == float.fromhex(rec["u"]["min"])
        assert d.u_stats.max_val == float.fromhex(rec["u"]["max"])
        assert math.isnan(d.u_stats.sum_val) and math.isnan(d.u_stats.avg_val)
        assert math.isnan(d.vel_mag_stats.sum_val)
        for k in ("v", "w", "p", "rho", "T"):
            s = getattr(d, k + "_stats")
            assert s.min_val == float.fromhex(rec[k]["min"]) and math.isfinite(s.sum_val)
        one = ctx.field_statistics(A.HIP_FIELD_U)
        assert one.max_val == d.u_stats.max_val and math.isnan(one.sum_val)
    finally:
        ctx.close()


def test_absent_fields_and_invalid_ids(hip_lib):
    case = K.BY_NAME["s67_real"]
    nx, ny, nz = case["shape"]
    n = nx * ny * nz
    arrs = K.inputs(case)
    ctx = api.HipProjection(nx, ny, nz)
    try:
        for k in ("u", "v", "w", "p"):
            ctx.set_field(FID[k], arrs[k])
        d = ctx.derived_statistics(False, K.RHO0)
        assert stats_tuple(d.rho_stats) == (K.RHO0, K.RHO0, (K.RHO0 * n) / n, K.RHO0 * n)
        assert d.rho_stats.avg_val == K.RHO0
        assert stats_tuple(d.T_stats) == (0.0, 0.0, 0.0, 0.0)
        s = A.FieldStats()
        for fid in (A.HIP_FIELD_T, A.HIP_FIELD_RHO, 17, -1):
            assert hip_lib.hip_proj_field_statistics(ctx.ctx, fid, C.byref(s)) == \
                A.CFD_ERROR_INVALID
        assert hip_lib.hip_proj_field_statistics(ctx.ctx, A.HIP_FIELD_U, None) == \
            A.CFD_ERROR_INVALID
        assert hip_lib.hip_proj_derived_statistics(None, 1, 1.0, C.byref(A.DerivedFields())) == \
            A.CFD_ERROR_INVALID
    finally:
        ctx.close()


def test_slab_contexts_are_unsupported(hip_lib, tmp_path):
    group = api.LocalGroup(2)
    ctxs = [api.HipProjection(17, 13, 12, comm=group.comm(r, 0)) for r in range(2)]
    try:
        c = ctxs[0]
        g = api.Grid(17, 13, 12)
        assert hip_lib.hip_proj_field_statistics(c.ctx, A.HIP_FIELD_U, C.byref(A.FieldStats())) == \
            A.CFD_ERROR_UNSUPPORTED
        assert hip_lib.hip_proj_derived_statistics(c.ctx, 1, 1.0, C.byref(A.DerivedFields())) == \
            A.CFD_ERROR_UNSUPPORTED
        buf = np.zeros(c.shape)
        assert hip_lib.hip_proj_velocity_magnitude(c.ctx, buf.ctypes.data_as(A.c_double_p)) == \
            A.CFD_ERROR_UNSUPPORTED
        prm, st = A.SolverParams(), A.SolverStats()
        assert c.write_csv_timeseries(str(tmp_path / "t.csv"), 0, 0.0, prm, st, True, True) == \
            A.CFD_ERROR_UNSUPPORTED
        assert c.write_csv_statistics(str(tmp_path / "s.csv"), 0, 0.0, 1.0, True, True) == \
            A.CFD_ERROR_UNSUPPORTED
        assert c.write_csv_centerline(str(tmp_path / "c.csv"), g, A.PROFILE_VERTICAL, 1.0, True) == \
            A.CFD_ERROR_UNSUPPORTED
        assert not list(tmp_path.iterdir())
    finally:
        for c in ctxs:
            c.close()
        group.close()


def test_ten_calls_are_bit_identical(loaded):
    ctx, _ = loaded("s96_real")
    first = bytes(ctx.derived_statistics(True, K.RHO0))
    m0 = ctx.velocity_magnitude()
    for _ in range(9):
        assert bytes(ctx.derived_statistics(True, K.RHO0)) == first
    assert_bits_equal(ctx.velocity_magnitude(), m0, what="velocity magnitude, second call")


def _monitor(ctx, g, tmp_path, tag):
    """Every monitoring entry once."""
    ctx.derived_statistics(True, 1.0)
    ctx.field_statistics(A.HIP_FIELD_P)
    ctx.velocity_magnitude()
    prm, st = A.SolverParams(), A.SolverStats()
    assert ctx.write_csv_timeseries(str(tmp_path / f"{tag}_t.csv"), 0, 0.0, prm, st, True,
                                    False) == A.CFD_SUCCESS
    assert ctx.write_csv_statistics(str(tmp_path / f"{tag}_s.csv"), 0, 0.0, 1.0, False,
                                    False) == A.CFD_SUCCESS
    for direction in (A.PROFILE_HORIZONTAL, A.PROFILE_VERTICAL):
        assert ctx.write_csv_centerline(str(tmp_path / f"{tag}_c.csv"), g, direction, 1.0,
                                        True) == A.CFD_SUCCESS


def test_device_steps_are_unchanged_by_the_calls(hip_lib, tmp_path):
    def run(monitor):
        g, f, p = cases.cavity(33, 29, 21, Re=100.0, dt=5e-4)
        api.cavity_bc(f, 1.0)
        ctx = api.HipProjection(g.nx, g.ny, g.nz)
        ctx.upload(f)
        out = []
        for step in range(3):
            st = A.SolverStats()
            assert ctx.step_device(g, p, st) == A.CFD_SUCCESS
            if monitor:
                _monitor(ctx, g, tmp_path, f"dev{step}")
            out.append((st.iterations, st.residual, st.max_velocity, st.max_pressure))
        fields = {k: ctx.get_field(FID[k]) for k in ("u", "v", "w", "p")}
        ctx.close()
        return out, fields

    plain, fp = run(False)
    watched, fw = run(True)
    assert plain == watched
    for k in fp:
        assert_bits_equal(fw[k], fp[k], what=f"{k} after 3 device steps with monitoring calls")


def test_resident_run_is_unchanged_by_the_calls(hip_lib, tmp_path):
    def run(monitor):
        g, f, p = cases.cavity(33, 29, 21, Re=100.0, dt=5e-4)
        ctx = api.HipProjection(g.nx, g.ny, g.nz, dirty_faces=1)
        out = []
        for step in range(4):
            api.cavity_bc(f, 1.0)
            st = A.SolverStats()
            assert ctx.step(f, g, p, st) == A.CFD_SUCCESS
            if monitor:
                _monitor(ctx, g, tmp_path, f"res{step}")
            out.append((st.iterations, st.residual, st.max_velocity, st.max_pressure))
        # were the run no longer resident, the next step would have uploaded
        # the stale host interior and the results below would differ
        ctx.sync_host(f)
        fields = {k: getattr(f, k).copy() for k in ("u", "v", "w", "p")}
        ctx.close()
        return out, fields

    plain, fp = run(False)
    watched, fw = run(True)
    assert plain == watched
    for k in fp:
        assert_bits_equal(fw[k], fp[k], what=f"{k} after a resident run with monitoring calls")


@pytest.mark.parametrize("name", K.CSV_CASES)
@pytest.mark.parametrize("mag", [0, 1])
def test_device_csv_files_match_byte_for_byte(record, hip_lib, tmp_path, name, mag):
    case = K.BY_NAME[name]
    want = record["csv"][name]
    nx, ny, nz = case["shape"]
    g = api.Grid(nx, ny, nz, **K.grid_extent(case))
    ctx = api.HipProjection(nx, ny, nz)
    ts, st = tmp_path / "ts.csv", tmp_path / "st.csv"
    try:
        for step in range(K.CSV_STEPS):
            arrs = K.inputs(case, step)
            for k in K.FIELDS:
                ctx.set_field(FID[k], arrs[k])
            t, dt, its, res, ms = K.csv_step_args(step)
            prm = A.SolverParams()
            prm.dt = dt
            stats = A.SolverStats()
            stats.iterations, stats.residual, stats.elapsed_time_ms = its, res, ms
            assert ctx.write_csv_timeseries(str(ts), step, t, prm, stats, bool(mag),
                                            step == 0) == A.CFD_SUCCESS
            assert ctx.write_csv_statistics(str(st), step, t, K.RHO0, bool(mag),
                                            step == 0) == A.CFD_SUCCESS
            if step == 0:
                # both directions read the k = 0 plane (IDX_2D), on the 3-D case too
                for tag, direction in (("h", A.PROFILE_HORIZONTAL), ("v", A.PROFILE_VERTICAL)):
                    cl = tmp_path / f"cl{tag}.csv"
                    assert ctx.write_csv_centerline(str(cl), g, direction, K.RHO0,
                                                    bool(mag)) == A.CFD_SUCCESS
                    assert cl.read_bytes() == want[f"centerline_{tag}_mag{mag}"].encode(), tag
        assert ts.read_bytes() == want[f"timeseries_mag{mag}"].encode()
        assert st.read_bytes() == want[f"statistics_mag{mag}"].encode()
    finally:
        ctx.close()


# ---- NaN, signed zeros, infinities, extreme magnitudes -------------------------

@pytest.fixture(scope="module")
def special_record():
    return json.loads((GOLDEN / S.JSON_FILE).read_text())


@pytest.fixture(scope="module")
def special_ctx(hip_lib):
    """shape -> one context; a test loads all six fields of its case."""
    cache = {}

    def get(case, step=0):
        shape = tuple(case["shape"])
        if shape not in cache:
            cache[shape] = api.HipProjection(*shape)
        arrs = S.inputs(case, step)
        for k in S.FIELDS:
            cache[shape].set_field(FID[k], arrs[k])
        return cache[shape], arrs

    yield get
    for ctx in cache.values():
        ctx.close()


def raw(s):
    """{min, max, avg, sum} of a field_stats as uint64 patterns."""
    names = [n.replace("_val", "") for n, _ in A.FieldStats._fields_]
    assert sorted(names) == ["avg", "max", "min", "sum"]
    return dict(zip(names, np.frombuffer(bytes(s), dtype=np.uint64).tolist()))


def rec_bits(r, m):
    return int(r[m], 16)


def same_sum(x, y):
    """Two sums / averages as patterns: both NaN, or the same bits."""
    fx, fy = S.from_bits(x), S.from_bits(y)
    return (math.isnan(fx) and math.isnan(fy)) or x == y


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: c["name"])
def test_special_fields_against_the_record(special_record, special_ctx, case):
    rec = special_record["cases"][case["name"]]
    ctx, arrs = special_ctx(case)
    d = ctx.derived_statistics(True, S.RHO0)
    mag = ctx.velocity_magnitude()
    assert_bits_equal(mag, S.magnitude(arrs), what=f"{case['name']}: velocity magnitude")
    assert S.sha_nan_canonical(mag) == rec["vel_mag_sha256"]
    if case["name"] == S.NPZ_CASE:
        assert_bits_equal(mag, np.load(GOLDEN / S.NPZ_FILE)["vel_mag"], what="velocity magnitude")
    data = dict(arrs, vel_mag=mag)
    for k in S.STATS:
        s = getattr(d, k + "_stats")
        got, r = raw(s), rec["stats"][k]
        want = np.array([rec_bits(r, "min"), rec_bits(r, "max")], dtype=np.uint64)
        have = np.array([got["min"], got["max"]], dtype=np.uint64)
        print(f"{case['name']} {k}: min {got['min']:016x} max {got['max']:016x} "
              f"(record {r['min']} {r['max']}) sum {s.sum_val!r}")
        assert_bits_equal(have.view(np.float64), want.view(np.float64),
                          what=f"{case['name']} {k} (min, max)")
        first = data[k].reshape(-1)[0]
        if k != "vel_mag":
            # a NaN in cell 0 included: the cell's own 64 bits
            assert have.tolist() == want.tolist(), (case["name"], k)
        elif np.isnan(first):
            # the magnitude's NaN is computed: the bits of the device's own cell 0
            assert have.tolist() == [int(S.bits(first).reshape(-1)[0])] * 2, (case["name"], k)
        S.check_sum(s.sum_val, s.avg_val, data[k], f"{case['name']} {k}")
    for k in S.FIELDS:
        one, fused = raw(ctx.field_statistics(FID[k])), raw(getattr(d, k + "_stats"))
        assert (one["min"], one["max"]) == (fused["min"], fused["max"]), k
        assert same_sum(one["sum"], fused["sum"]) and same_sum(one["avg"], fused["avg"]), k
    d0 = ctx.derived_statistics(False, S.RHO0)
    assert stats_tuple(d0.vel_mag_stats) == (0.0, 0.0, 0.0, 0.0)
    for k in S.FIELDS:
        a, b = raw(getattr(d0, k + "_stats")), raw(getattr(d, k + "_stats"))
        assert (a["min"], a["max"]) == (b["min"], b["max"]), k
        assert same_sum(a["sum"], b["sum"]) and same_sum(a["avg"], b["avg"]), k


def test_special_cases_are_deterministic(special_ctx):
    """The same case twice, and again after an unrelated case on the context."""
    case = S.BY_NAME["s96_zeros_nonneg_round"]

    def run():
        ctx, _ = special_ctx(case)
        return bytes(ctx.derived_statistics(True, S.RHO0)), ctx.velocity_magnitude(), \
            [bytes(ctx.field_statistics(FID[k])) for k in S.FIELDS]

    first = run()
    ctx, _ = special_ctx(case)
    assert bytes(ctx.derived_statistics(True, S.RHO0)) == first[0]
    for other in ("s96_nan_all", "s96_mag_extreme"):
        ctx, _ = special_ctx(S.BY_NAME[other])
        ctx.derived_statistics(True, S.RHO0)
        ctx.velocity_magnitude()
    again = run()
    assert again[0] == first[0] and again[2] == first[2]
    assert_bits_equal(again[1], first[1], what="velocity magnitude after an unrelated case")
    # a case with NaNs: the same bits too, NaN payloads included
    nan_case = S.BY_NAME["s96_nan_first_pos"]
    ctx, _ = special_ctx(nan_case)
    a = bytes(ctx.derived_statistics(True, S.RHO0))
    special_ctx(case)
    ctx, _ = special_ctx(nan_case)
    assert bytes(ctx.derived_statistics(True, S.RHO0)) == a


def csv_equal_up_to_nan_sign_of_averages(got: bytes, want: bytes, what: str):
    """Byte for byte; failing that, the only difference allowed is the sign of
    a NaN in an avg_ / sum_ column (a propagated NaN's sign is not part of the
    contract), which is printed."""
    if got == want:
        return
    g, w = got.decode().splitlines(), want.decode().splitlines()
    assert len(g) == len(w) and g[0] == w[0], what
    head = g[0].split(",")
    for n, (gl, wl) in enumerate(zip(g[1:], w[1:]), start=1):
        gc, wc = gl.split(","), wl.split(",")
        assert len(gc) == len(wc) == len(head), (what, n)
        for name, x, y in zip(head, gc, wc):
            if x == y:
                continue
            assert name.startswith(("avg_", "sum_")) and {x, y} == {"nan", "-nan"}, \
                (what, n, name, x, y)
            print(f"{what}: row {n} column {name}: {x} for the record's {y}")


@pytest.mark.parametrize("name", list(S.CSV_CASES))
@pytest.mark.parametrize("mag", [0, 1])
def test_special_csv_files_match_byte_for_byte(special_record, special_ctx, tmp_path, name, mag):
    steps = S.CSV_CASES[name]
    want = special_record["csv"][name]
    nx, ny, nz = steps[0]["shape"]
    g = api.Grid(nx, ny, nz, **K.grid_extent(steps[0]))
    ts, st = tmp_path / "ts.csv", tmp_path / "st.csv"
    for step, case in enumerate(steps):
        ctx, _ = special_ctx(case, step)
        t, dt, its, res, ms = K.csv_step_args(step)
        prm = A.SolverParams()
        prm.dt = dt
        stats = A.SolverStats()
        stats.iterations, stats.residual, stats.elapsed_time_ms = its, res, ms
        assert ctx.write_csv_timeseries(str(ts), step, t, prm, stats, bool(mag),
                                        step == 0) == A.CFD_SUCCESS
        assert ctx.write_csv_statistics(str(st), step, t, S.RHO0, bool(mag),
                                        step == 0) == A.CFD_SUCCESS
        if step == 0:
            for tag, direction in (("h", A.PROFILE_HORIZONTAL), ("v", A.PROFILE_VERTICAL)):
                cl = tmp_path / f"cl{tag}.csv"
                assert ctx.write_csv_centerline(str(cl), g, direction, S.RHO0,
                                                bool(mag)) == A.CFD_SUCCESS
                assert cl.read_bytes() == want[f"centerline_{tag}_mag{mag}"].encode(), tag
    csv_equal_up_to_nan_sign_of_averages(ts.read_bytes(), want[f"timeseries_mag{mag}"].encode(),
                                         f"{name} timeseries")
    csv_equal_up_to_nan_sign_of_averages(st.read_bytes(), want[f"statistics_mag{mag}"].encode(),
                                         f"{name} statistics")
