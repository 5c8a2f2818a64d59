"""The host mirror of the reference's monitoring layer (libcfd_host.so:
calculate_field_statistics, derived_fields_*, write_csv_*) against the
reference's own recorded results (tests/golden/derived_cases.json, written by
tests/golden/make_derived_golden.py with one OpenMP thread), and the
conditions the seeded inputs of tests/derived_cases.py must meet so that the
record can tell errors apart.

Sum bound on real-valued fields: any summation order of n doubles, the
reference's sequential one included, errs by at most (n - 1) u sum|x| to first
order, u = 2^-53; the tests use n * 2^-53 * sum|x| against math.fsum. The
mirror sums in the reference's order, so it is also compared bit for bit.
"""
import ctypes as C
import json
import math
import os
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from cfd_amd import _abi as A
from cfd_amd import api
from tests import derived_cases as K

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"
HOST = ROOT / "cfd_amd" / "csrc" / "host"


@pytest.fixture(scope="module")
def record():
    return json.loads((GOLDEN / K.JSON_FILE).read_text())


def load_field(case, step=0):
    nx, ny, nz = case["shape"]
    f = api.FlowField(nx, ny, nz)
    arrs = K.inputs(case, step)
    for k in K.FIELDS:
        getattr(f, k)[...] = arrs[k]
    return f, arrs


def host_derived(case, f, with_mag=True):
    d = api.DerivedFields(*case["shape"])
    if with_mag:
        d.compute_velocity_magnitude(f)
    d.compute_statistics(f)
    return d


def check_sum(got_sum, got_avg, data, kind, rec):
    flat = np.asarray(data, dtype=np.float64).reshape(-1)
    n = flat.size
    if kind == "int":
        assert got_sum.hex() == rec["sum"] and got_avg.hex() == rec["avg"]
        return
    exact = math.fsum(flat.tolist())
    bound = n * 2.0 ** -53 * math.fsum(np.abs(flat).tolist())
    assert abs(got_sum - exact) <= bound, (got_sum, exact, bound)
    assert got_avg == got_sum / float(n)


@pytest.mark.parametrize("case", K.CASES, ids=lambda c: c["name"])
def test_inputs_match_the_record_and_tell_errors_apart(record, case):
    rec = record["cases"][case["name"]]
    arrs = K.inputs(case)
    nx, ny, nz = case["shape"]
    assert rec["shape"] == [nx, ny, nz] and rec["kind"] == case["kind"]
    where = {"last_col": False, "first_plane": False, "last_plane": False, "index0": False}
    for k in K.FIELDS:
        a = arrs[k]
        assert K.sha(a) == rec["inputs"][k], f"{k}: the seeded input changed"
        assert np.all(np.isfinite(a))
        if case["kind"] == "int":
            assert np.all(a == np.rint(a)) and np.max(np.abs(a)) <= 2.0 ** 20
        for ext in (a.min(), a.max()):
            cells = np.argwhere(a == ext)
            assert len(cells) == 1, f"{k}: extreme {ext} at {len(cells)} cells"
            kk, jj, ii = (int(v) for v in cells[0])
            where["last_col"] |= ii == nx - 1
            where["first_plane"] |= kk == 0
            where["last_plane"] |= kk == nz - 1
            where["index0"] |= (kk, jj, ii) == (0, 0, 0)
        assert int(np.argmin(a)) != int(np.argmax(a))
    assert all(where.values()), where


@pytest.mark.parametrize("case", [c for c in K.CASES if c["kind"] == "real"],
                         ids=lambda c: c["name"])
def test_real_averages_are_clear_of_rounding_boundaries(case):
    steps = range(K.CSV_STEPS) if case["name"] in K.CSV_CASES else (0,)
    for step in steps:
        arrs = dict(K.inputs(case, step))
        arrs["vel_mag"] = np.sqrt((arrs["u"] * arrs["u"]) + (arrs["v"] * arrs["v"])
                                  + (arrs["w"] * arrs["w"]))
        for k, a in arrs.items():
            avg = math.fsum(a.reshape(-1).tolist()) / a.size
            assert K.boundary_clear(avg, 1e-9), (case["name"], step, k, avg)


def test_boundary_rule_itself():
    assert not K.boundary_clear(1.2345675)          # the midpoint itself
    assert not K.boundary_clear(1.2345675 * (1 + 5e-10))
    assert K.boundary_clear(1.2345675 * (1 + 2e-9))
    assert K.boundary_clear(1.234567) and K.boundary_clear(0.0)


@pytest.mark.parametrize("case", K.CASES, ids=lambda c: c["name"])
def test_host_mirror_reproduces_the_reference(record, case):
    rec = record["cases"][case["name"]]
    f, arrs = load_field(case)
    d = host_derived(case, f)
    mag = d.velocity_magnitude
    assert K.sha(mag) == rec["vel_mag_sha256"]
    if case["name"] == K.NPZ_CASE:
        want = np.load(GOLDEN / K.NPZ_FILE)["vel_mag"]
        assert np.array_equal(mag.view(np.uint64), want.view(np.uint64))
    assert d.c.stats_computed == 1
    data = dict(arrs, vel_mag=mag)
    for k in K.STATS:
        s = getattr(d.c, k + "_stats")
        r = rec["stats"][k]
        assert float(s.min_val).hex() == r["min"] and float(s.max_val).hex() == r["max"], k
        # the magnitude of integer-valued fields is not integer-valued
        check_sum(s.sum_val, s.avg_val, data[k], "real" if k == "vel_mag" else case["kind"], r)
        # the mirror sums in the reference's order
        assert float(s.sum_val).hex() == r["sum"] and float(s.avg_val).hex() == r["avg"], k
        one = api.calculate_field_statistics(data[k])
        assert (one.min_val, one.max_val, one.sum_val, one.avg_val) == (
            s.min_val, s.max_val, s.sum_val, s.avg_val)


def test_host_conventions():
    a = np.array([3.0, np.nan, -2.0, 7.0, 1.0])
    s = api.calculate_field_statistics(a)
    assert s.min_val == -2.0 and s.max_val == 7.0 and math.isnan(s.sum_val)
    s = api.calculate_field_statistics(np.array([np.nan, 1.0, 2.0]))  # data[0] is the seed
    assert math.isnan(s.min_val) and math.isnan(s.max_val)
    # an absent w is w_i = 0.0; clear() frees the magnitude and resets the flag
    f = api.FlowField(4, 3, 1)
    f.u[...] = 3.0
    f.v[...] = 4.0
    f.w[...] = 100.0
    keep = f.ptr.contents.w
    f.ptr.contents.w = None
    d = api.DerivedFields(4, 3, 1)
    d.compute_velocity_magnitude(f)
    d.compute_statistics(f)
    f.ptr.contents.w = keep
    assert np.all(d.velocity_magnitude == 5.0)
    assert d.c.w_stats.max_val == 0.0 and d.c.vel_mag_stats.sum_val == 60.0
    d.clear()
    assert d.velocity_magnitude is None and d.c.stats_computed == 0


@pytest.mark.parametrize("name", K.CSV_CASES)
@pytest.mark.parametrize("mag", [0, 1])
def test_host_csv_files_match_byte_for_byte(record, tmp_path, name, mag):
    case = K.BY_NAME[name]
    want = record["csv"][name]
    nx, ny, nz = case["shape"]
    g = api.Grid(nx, ny, nz, **K.grid_extent(case))
    ts, st = tmp_path / "ts.csv", tmp_path / "st.csv"
    for step in range(K.CSV_STEPS):
        f, _ = load_field(case, step)
        d = host_derived(case, f, bool(mag))
        t, dt, its, res, ms = K.csv_step_args(step)
        prm = A.SolverParams()
        prm.dt = dt
        stats = A.SolverStats()
        stats.iterations, stats.residual, stats.elapsed_time_ms = its, res, ms
        # step 0 by create_new, then the append path
        api.write_csv_timeseries(str(ts), step, t, f, d, prm, stats, step == 0)
        api.write_csv_statistics(str(st), step, t, f, d, step == 0)
        if step == 0:
            for tag, direction in (("h", A.PROFILE_HORIZONTAL), ("v", A.PROFILE_VERTICAL)):
                cl = tmp_path / f"cl{tag}.csv"
                api.write_csv_centerline(str(cl), f, d, g, direction)
                assert cl.read_bytes() == want[f"centerline_{tag}_mag{mag}"].encode(), tag
    assert ts.read_bytes() == want[f"timeseries_mag{mag}"].encode()
    assert st.read_bytes() == want[f"statistics_mag{mag}"].encode()
    assert ts.read_text().count("\n") == K.CSV_STEPS + 1


def test_csv_header_rule(tmp_path):
    """create_new || !file_exists: an absent file gets a header without
    create_new; an existing one is appended to; create_new truncates."""
    case = K.BY_NAME["s3_real"]
    f, _ = load_field(case)
    d = host_derived(case, f)
    p = tmp_path / "s.csv"
    api.write_csv_statistics(str(p), 0, 0.0, f, d, False)
    api.write_csv_statistics(str(p), 1, 0.1, f, d, False)
    lines = p.read_text().splitlines()
    assert len(lines) == 3 and lines[0].startswith("step,time,min_u") and lines[2][0] == "1"
    api.write_csv_statistics(str(p), 2, 0.2, f, d, True)
    assert len(p.read_text().splitlines()) == 2


def _struct_members(text, name):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    m = re.search(r"typedef (?:struct|enum) \{([^{}]*)\} " + name + r";", text)
    assert m, name
    sep = ";" if "struct" in m.group(0)[:16] else ","
    return [re.sub(r"\s+", " ", x).strip() for x in m.group(1).split(sep) if x.strip()]


def test_struct_layouts_equal_the_reference_header_text():
    ref = Path(os.environ.get("CFD_REFERENCE_DIR") or ROOT.parent / "reference")
    hdr = ref / "lib" / "include" / "cfd" / "core" / "derived_fields.h"
    csv = ref / "lib" / "include" / "cfd" / "io" / "csv_output.h"
    if not (hdr.is_file() and csv.is_file()):
        pytest.skip("the reference checkout is not present")
    ours = (ROOT / "include" / "cfd_hip" / "cfd_abi.h").read_text()
    for name, path in (("field_stats", hdr), ("derived_fields", hdr),
                       ("profile_direction", csv)):
        assert _struct_members(ours, name) == _struct_members(path.read_text(), name), name


def test_ctypes_mirrors_match_the_c_layout():
    assert C.sizeof(A.FieldStats) == 32
    assert A.DerivedFields.u_stats.offset == 32 and A.DerivedFields.vel_mag_stats.offset == 224
    assert A.DerivedFields.stats_computed.offset == 256 and C.sizeof(A.DerivedFields) == 264


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not present")
def test_host_monitoring_code_under_asan_ubsan(tmp_path):
    """csv_format.h, the host statistics and the writers in a stand-alone
    program (tests/native/derived_host_main.c) built with ASan + UBSan."""
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(["gcc", *flags, str(probe), "-o", str(tmp_path / "probe")],
                       capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("the sanitizer runtime cannot be linked: " + r.stderr[-200:])
    exe = tmp_path / "derived_host_main"
    cmd = ["gcc", "-std=c11", "-g", "-O1", "-fno-omit-frame-pointer", "-ffp-contract=off", *flags,
           "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", f"-I{HOST}",
           str(ROOT / "tests" / "native" / "derived_host_main.c"), str(HOST / "derived_host.c"),
           "-o", str(exe), "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True, env=env,
                         timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout + out.stderr)[-4000:]
