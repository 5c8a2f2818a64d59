#!/usr/bin/env python3
"""Device-side field statistics at n^3 (default 512) on one context, interleaved
on the same box with the only route to the same numbers without them:
hip_proj_get_field x 4 followed by the host mirror's
derived_fields_compute_velocity_magnitude / _compute_statistics.
usage: derived_bench.py [out.json]      (env: N, REPS, ROUNDS; default
out: profiles/derived_stats_<N>.json)
ROUNDS rounds of: REPS fused passes with the magnitude, REPS without, REPS
single-field passes, one hip_proj_velocity_magnitude (pass + store + download),
one download-and-host-statistics. Each timing starts after
hip_proj_synchronize; every entry ends with its own stream synchronisation, so
the wall time per call is the call's whole cost. Prints and writes one JSON
record: ms per call (median over the rounds), each pass's algorithmic-byte
rate (8 B per resident field and cell; the context holds u, v, w, p, rho, T:
48 B/cell fused, 8 B/cell single) beside cfd_hip_stream_bench's copy rate."""
import ctypes as C
import json
import os
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401

from cfd_amd import _abi as A  # noqa: E402
from cfd_amd import _native, api  # noqa: E402


def main():
    n = int(os.environ.get("N", "512"))
    root = Path(__file__).resolve().parent.parent
    out = sys.argv[1] if len(sys.argv) > 1 else root / "profiles" / f"derived_stats_{n}.json"
    reps = int(os.environ.get("REPS", "20"))
    rounds = int(os.environ.get("ROUNDS", "3"))
    cells = n ** 3
    lib = _native.hip()
    copy, triad = C.c_double(0.0), C.c_double(0.0)
    assert lib.cfd_hip_stream_bench(0, cells, 5, C.byref(copy), C.byref(triad)) == A.CFD_SUCCESS

    rng = np.random.default_rng(n)
    f = api.FlowField(n, n, n)
    f.u[...] = rng.standard_normal((n, n, n))
    f.v[...] = f.u[::-1]
    f.w[...] = 0.5 * f.u + 0.25
    f.p[...] = 3.0 - f.u
    ctx = api.HipProjection(n, n, n)
    ctx.upload(f)
    ctx.fill(A.HIP_FIELD_T, 300.0)
    ctx.fill(A.HIP_FIELD_RHO, 1.0)
    host = api.DerivedFields(n, n, n)

    def timed(fn, count):
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(count):
            fn()
        return (time.perf_counter() - t0) * 1e3 / count

    ms = {k: [] for k in ("fused_mag", "fused", "single", "velocity_magnitude",
                          "download4", "host_compute")}
    ctx.derived_statistics(True, 1.0)  # warm-up: first launches, lazy buffers
    ctx.field_statistics(A.HIP_FIELD_U)
    ctx.velocity_magnitude()
    dev = None
    for _ in range(rounds):
        ms["fused_mag"].append(timed(lambda: ctx.derived_statistics(True, 1.0), reps))
        ms["fused"].append(timed(lambda: ctx.derived_statistics(False, 1.0), reps))
        ms["single"].append(timed(lambda: ctx.field_statistics(A.HIP_FIELD_U), reps))
        ms["velocity_magnitude"].append(timed(ctx.velocity_magnitude, 1))

        def download():
            for fid, a in ((A.HIP_FIELD_U, f.u), (A.HIP_FIELD_V, f.v), (A.HIP_FIELD_W, f.w),
                           (A.HIP_FIELD_P, f.p)):
                assert lib.hip_proj_get_field(ctx.ctx, fid, a.ctypes.data_as(A.c_double_p)) == 0

        def compute():
            host.compute_velocity_magnitude(f)
            host.compute_statistics(f)

        ms["download4"].append(timed(download, 1))
        ms["host_compute"].append(timed(compute, 1))
        dev = ctx.derived_statistics(True, 1.0)
    # the two routes agree: min / max exactly, sums to the summation-order bound
    hs = host.stats()
    for k in ("u", "v", "w", "p", "vel_mag"):
        d = api.stats_dict(getattr(dev, k + "_stats"))
        assert d["min"] == hs[k]["min"] and d["max"] == hs[k]["max"], (k, d, hs[k])
        assert abs(d["sum"] - hs[k]["sum"]) <= 2.0 * cells * 2.0 ** -53 * 8.0 * cells, k
    ctx.close()
    med = {k: statistics.median(v) for k, v in ms.items()}
    gb = lambda b, t: round(b * cells / (t * 1e-3) / 1e9, 1)  # noqa: E731
    rec = {"n": n, "reps": reps, "rounds": rounds,
           "ms_per_call": {k: round(v, 4) for k, v in med.items()},
           "host_route_ms": round(med["download4"] + med["host_compute"], 1),
           "bytes_per_cell": {"fused_mag": 48, "fused": 48, "single": 8},
           "GBps": {"fused_mag": gb(48, med["fused_mag"]), "fused": gb(48, med["fused"]),
                    "single": gb(8, med["single"])},
           "stream_copy_GBps": round(copy.value, 1), "stream_triad_GBps": round(triad.value, 1),
           "speedup_vs_host_route": round((med["download4"] + med["host_compute"])
                                          / med["fused_mag"], 1),
           "all_rounds_ms": {k: [round(t, 4) for t in v] for k, v in ms.items()}}
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        Path(out).write_text(line + "\n")


if __name__ == "__main__":
    main()
