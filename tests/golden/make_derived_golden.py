#!/usr/bin/env python3
"""Writes the field-statistics / velocity-magnitude / CSV fixtures from the
reference's own functions (calculate_field_statistics via
derived_fields_compute_statistics, derived_fields_compute_velocity_magnitude,
write_csv_timeseries / _statistics / _centerline) on every case of
tests/derived_cases.py:

  tests/golden/derived_cases.json   per case: shape, kind, seed, sha256 of the
                                    inputs, min / max / avg / sum of u, v, w,
                                    p, rho, T and the magnitude as hex floats,
                                    sha256 of the magnitude array; `csv`: the
                                    text of the three CSV files of the two
                                    CSV cases, with and without the magnitude,
                                    timeseries and statistics as three
                                    appended steps, the centerline in both
                                    directions
  tests/golden/derived_vel_mag_17x13x11.npz  the full magnitude of "s17_real"

The reference is built unmodified by make_rk_golden.build_reference (copied
to a work directory, its own CMake, CPU only, -ffp-contract=off); the
archives it links hold derived_fields.c and csv_output.c. The script runs the
reference with ONE OpenMP thread, so its sum is the sequential one. Nothing
built from the reference and none of its text is written into this
repository: only the numbers and the CSV rows its functions produce.

With --special it writes instead, for the NaN / signed-zero / inf / extreme
cases of tests/derived_special_cases.py:

  tests/golden/derived_special_cases.json  per case: min / max / sum / avg of
                                    the seven quantities as 64-bit patterns
                                    (hex, so a NaN's bits survive), sha256 of
                                    the magnitude with its NaNs canonicalised;
                                    `csv`: the text of the three writers for
                                    the two CSV cases. Under 1000 cells
                                    `stats` is the reference's answer (its
                                    sequential loop). From 1000 cells on the
                                    reference takes its OpenMP min / max
                                    reduction, whose result with a NaN operand
                                    is the compiler's choice: its answer goes
                                    under `openmp_path` (informative only,
                                    with `openmp_path_differs` naming the
                                    entries whose bits differ) and `stats` is
                                    the sequential loop as the host mirror
                                    (libcfd_host.so) computes it, which
                                    tests/test_derived_special_fixtures.py
                                    ties to the reference below 1000 cells.
  tests/golden/derived_special_vel_mag_17x13x4.npz  the full magnitude of
                                    "s17_mag_extreme"

usage: make_derived_golden.py [--special] [--work DIR] [--jobs N] [--so BUILT_LIBRARY]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import tempfile
from pathlib import Path

os.environ["OMP_NUM_THREADS"] = "1"

import numpy as np  # noqa: E402

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))
OUT = Path(__file__).resolve().parent


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--work", default="/tmp/cfd_rk_golden")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--so", default=None, help="a library build_reference already linked")
    ap.add_argument("--special", action="store_true",
                    help="record tests/derived_special_cases.py instead")
    a = ap.parse_args()
    if a.so:
        so = Path(a.so)
    else:
        from make_rk_golden import build_reference
        work = Path(a.work)
        work.mkdir(parents=True, exist_ok=True)
        so = build_reference(work, a.jobs)
    ref = C.CDLL(str(so))

    from cfd_amd import _abi as A
    from cfd_amd import api
    from tests import derived_cases as K

    P = C.POINTER
    ref.derived_fields_create.restype = P(A.DerivedFields)
    ref.derived_fields_create.argtypes = [C.c_size_t] * 3
    ref.derived_fields_destroy.restype = None
    ref.derived_fields_destroy.argtypes = [P(A.DerivedFields)]
    for fn in ("derived_fields_compute_velocity_magnitude", "derived_fields_compute_statistics"):
        getattr(ref, fn).restype = None
        getattr(ref, fn).argtypes = [P(A.DerivedFields), P(A.FlowField)]
    ref.write_csv_timeseries.restype = None
    ref.write_csv_timeseries.argtypes = [C.c_char_p, C.c_int, C.c_double, P(A.FlowField),
                                         P(A.DerivedFields), P(A.SolverParams), P(A.SolverStats),
                                         C.c_size_t, C.c_size_t, C.c_int]
    ref.write_csv_statistics.restype = None
    ref.write_csv_statistics.argtypes = [C.c_char_p, C.c_int, C.c_double, P(A.FlowField),
                                         P(A.DerivedFields), C.c_size_t, C.c_size_t, C.c_int]
    ref.write_csv_centerline.restype = None
    ref.write_csv_centerline.argtypes = [C.c_char_p, P(A.FlowField), P(A.DerivedFields),
                                         A.c_double_p, A.c_double_p, C.c_size_t, C.c_size_t,
                                         C.c_int]

    if a.special:
        return record_special(ref, A, api)

    def load(case, step=0):
        nx, ny, nz = case["shape"]
        f = api.FlowField(nx, ny, nz)
        arrs = K.inputs(case, step)
        for k in K.FIELDS:
            getattr(f, k)[...] = arrs[k]
        return f, arrs

    def derive(case, f, with_mag):
        d = ref.derived_fields_create(*case["shape"])
        if with_mag:
            ref.derived_fields_compute_velocity_magnitude(d, f.ptr)
        ref.derived_fields_compute_statistics(d, f.ptr)
        return d

    doc = {"reference": "shaia/CFD v0.3.0, derived_fields.c / csv_output.c, one OpenMP thread",
           "build_flags": "-DCMAKE_BUILD_TYPE=Release -DCMAKE_C_FLAGS=-ffp-contract=off",
           "cases": {}, "csv": {}}
    npz = {}
    for case in K.CASES:
        nx, ny, nz = case["shape"]
        n = nx * ny * nz
        f, arrs = load(case)
        d = derive(case, f, True)
        dc = d.contents
        mag = np.ctypeslib.as_array(dc.velocity_magnitude, shape=(nz, ny, nx)).copy()
        rec = {"shape": list(case["shape"]), "kind": case["kind"], "seed": case["seed"],
               "inputs": {k: K.sha(arrs[k]) for k in K.FIELDS}, "stats": {},
               "vel_mag_sha256": K.sha(mag)}
        for k in K.STATS:
            s = getattr(dc, k + "_stats")
            rec["stats"][k] = {"min": float(s.min_val).hex(), "max": float(s.max_val).hex(),
                               "avg": float(s.avg_val).hex(), "sum": float(s.sum_val).hex()}
            # a real-valued average must not sit on a %.6e rounding boundary
            data = mag if k == "vel_mag" else arrs[k]
            exact = math.fsum(data.reshape(-1).tolist()) / n
            if case["kind"] == "real" and not K.boundary_clear(exact):
                raise SystemExit(f"make_derived_golden: {case['name']} {k}: avg {exact!r} is "
                                 "within 1e-9 of a %.6e rounding boundary; pick another seed")
        assert dc.stats_computed == 1
        doc["cases"][case["name"]] = rec
        if case["name"] == K.NPZ_CASE:
            npz["vel_mag"] = mag
        ref.derived_fields_destroy(d)

    with tempfile.TemporaryDirectory() as tmp:
        for name in K.CSV_CASES:
            case = K.BY_NAME[name]
            nx, ny, nz = case["shape"]
            g = api.Grid(nx, ny, nz, **K.grid_extent(case))
            texts = {}
            for mag in (0, 1):
                ts, stt = Path(tmp) / f"{name}_ts{mag}.csv", Path(tmp) / f"{name}_st{mag}.csv"
                for step in range(K.CSV_STEPS):
                    f, arrs = load(case, step)
                    d = derive(case, f, bool(mag))
                    if case["kind"] == "real":
                        dm = d.contents.velocity_magnitude
                        data = dict(arrs)
                        if mag:
                            data["vel_mag"] = np.ctypeslib.as_array(dm, shape=(nz, ny, nx))
                        for k in data:
                            exact = math.fsum(data[k].reshape(-1).tolist()) / (nx * ny * nz)
                            if not K.boundary_clear(exact):
                                raise SystemExit(f"make_derived_golden: {name} step {step} {k}: "
                                                 "avg on a rounding boundary; pick another seed")
                    t, dt, its, res, ms = K.csv_step_args(step)
                    prm = A.SolverParams()
                    prm.dt = dt
                    st = A.SolverStats()
                    st.iterations, st.residual, st.elapsed_time_ms = its, res, ms
                    ref.write_csv_timeseries(str(ts).encode(), step, t, f.ptr, d, C.byref(prm),
                                             C.byref(st), nx, ny, int(step == 0))
                    ref.write_csv_statistics(str(stt).encode(), step, t, f.ptr, d, nx, ny,
                                             int(step == 0))
                    if step == 0:
                        for tag, direction in (("h", A.PROFILE_HORIZONTAL),
                                               ("v", A.PROFILE_VERTICAL)):
                            cl = Path(tmp) / f"{name}_cl{tag}{mag}.csv"
                            ref.write_csv_centerline(str(cl).encode(), f.ptr, d, g.c.x, g.c.y, nx,
                                                     ny, direction)
                            texts[f"centerline_{tag}_mag{mag}"] = cl.read_text()
                    ref.derived_fields_destroy(d)
                texts[f"timeseries_mag{mag}"] = ts.read_text()
                texts[f"statistics_mag{mag}"] = stt.read_text()
            assert sorted(texts) == sorted(K.csv_keys())
            doc["csv"][name] = texts
    (OUT / K.JSON_FILE).write_text(json.dumps(doc, indent=1) + "\n")
    np.savez_compressed(OUT / K.NPZ_FILE, **npz)
    print(json.dumps({"cases": len(doc["cases"]), "csv": list(doc["csv"])}))


def record_special(ref, A, api):
    from tests import derived_cases as K
    from tests import derived_special_cases as S

    def load(case, step=0):
        f = api.FlowField(*case["shape"])
        arrs = S.inputs(case, step)
        for k in S.FIELDS:
            getattr(f, k)[...] = arrs[k]
        return f, arrs

    class without_w:
        """The case's flow_field with w = NULL while a function reads it."""

        def __init__(self, case, f):
            self.c, self.absent = f.ptr.contents, case["w_absent"]

        def __enter__(self):
            self.keep = self.c.w
            if self.absent:
                self.c.w = None

        def __exit__(self, *exc):
            self.c.w = self.keep

    def derive(case, f, with_mag):
        d = ref.derived_fields_create(*case["shape"])
        with without_w(case, f):
            if with_mag:
                ref.derived_fields_compute_velocity_magnitude(d, f.ptr)
            ref.derived_fields_compute_statistics(d, f.ptr)
        return d

    def stats_of(dc):
        return {k: {m: S.hexbits(getattr(getattr(dc, k + "_stats"), m + "_val"))
                    for m in ("min", "max", "sum", "avg")} for k in S.STATS}

    def same(x, y, m):
        fx, fy = (S.from_bits(int(v, 16)) for v in (x, y))
        if m in ("sum", "avg") and math.isnan(fx) and math.isnan(fy):
            return True  # a sum's NaN: sign and payload are not part of the contract
        return x == y

    doc = {"reference": "shaia/CFD v0.3.0, derived_fields.c / csv_output.c, one OpenMP thread",
           "build_flags": "-DCMAKE_BUILD_TYPE=Release -DCMAKE_C_FLAGS=-ffp-contract=off",
           "cases": {}, "csv": {}}
    npz = {}
    for case in S.CASES:
        nx, ny, nz = case["shape"]
        f, arrs = load(case)
        d = derive(case, f, True)
        dc = d.contents
        assert dc.stats_computed == 1
        mag = np.ctypeslib.as_array(dc.velocity_magnitude, shape=(nz, ny, nx)).copy()
        rec = {"shape": list(case["shape"]), "cls": case["cls"], "variant": case["variant"],
               "probe": case["probe"], "seed": case["seed"],
               "inputs": {k: K.sha(arrs[k]) for k in S.FIELDS},
               "vel_mag_sha256": S.sha_nan_canonical(mag)}
        if nx * ny * nz < S.OMP_THRESHOLD:
            rec["stats"] = stats_of(dc)
        else:
            h = api.DerivedFields(nx, ny, nz)
            with without_w(case, f):
                h.compute_velocity_magnitude(f)
                h.compute_statistics(f)
            rec["stats"] = stats_of(h.c)
            rec["openmp_path"] = stats_of(dc)
            rec["openmp_path_differs"] = [
                f"{k}.{m}" for k in S.STATS for m in ("min", "max", "sum", "avg")
                if not same(rec["stats"][k][m], rec["openmp_path"][k][m], m)]
        doc["cases"][case["name"]] = rec
        if case["name"] == S.NPZ_CASE:
            npz["vel_mag"] = mag
        ref.derived_fields_destroy(d)

    with tempfile.TemporaryDirectory() as tmp:
        for name, steps in S.CSV_CASES.items():
            nx, ny, nz = steps[0]["shape"]
            g = api.Grid(nx, ny, nz, **K.grid_extent(steps[0]))
            texts = {}
            for mag in (0, 1):
                ts, stt = Path(tmp) / f"{name}_ts{mag}.csv", Path(tmp) / f"{name}_st{mag}.csv"
                for step, case in enumerate(steps):
                    f, arrs = load(case, step)
                    d = derive(case, f, bool(mag))
                    data = dict(arrs)
                    if mag:
                        data["vel_mag"] = np.ctypeslib.as_array(d.contents.velocity_magnitude,
                                                                shape=(nz, ny, nx))
                    for k in data:
                        exact = math.fsum(data[k].reshape(-1).tolist()) / (nx * ny * nz)
                        if not K.boundary_clear(exact):
                            raise SystemExit(f"make_derived_golden: {name} step {step} {k}: "
                                             "avg on a rounding boundary; pick another seed")
                    t, dt, its, res, ms = K.csv_step_args(step)
                    prm = A.SolverParams()
                    prm.dt = dt
                    st = A.SolverStats()
                    st.iterations, st.residual, st.elapsed_time_ms = its, res, ms
                    ref.write_csv_timeseries(str(ts).encode(), step, t, f.ptr, d, C.byref(prm),
                                             C.byref(st), nx, ny, int(step == 0))
                    ref.write_csv_statistics(str(stt).encode(), step, t, f.ptr, d, nx, ny,
                                             int(step == 0))
                    if step == 0:
                        for tag, direction in (("h", A.PROFILE_HORIZONTAL),
                                               ("v", A.PROFILE_VERTICAL)):
                            cl = Path(tmp) / f"{name}_cl{tag}{mag}.csv"
                            ref.write_csv_centerline(str(cl).encode(), f.ptr, d, g.c.x, g.c.y, nx,
                                                     ny, direction)
                            texts[f"centerline_{tag}_mag{mag}"] = cl.read_text()
                    ref.derived_fields_destroy(d)
                texts[f"timeseries_mag{mag}"] = ts.read_text()
                texts[f"statistics_mag{mag}"] = stt.read_text()
            assert sorted(texts) == sorted(K.csv_keys())
            doc["csv"][name] = texts
    (OUT / S.JSON_FILE).write_text(json.dumps(doc, indent=1) + "\n")
    np.savez_compressed(OUT / S.NPZ_FILE, **npz)
    differs = {n: r["openmp_path_differs"] for n, r in doc["cases"].items()
               if r.get("openmp_path_differs")}
    print(json.dumps({"cases": len(doc["cases"]), "csv": list(doc["csv"]),
                      "openmp_path_differs": differs}))


if __name__ == "__main__":
    sys.exit(main())
