#!/usr/bin/env python3
"""hip_proj_flow_diagnostics at n^3 (default 512) on the lid-driven cavity state
after WARM direct-solve steps, interleaved in one process with its yardsticks.
usage: flow_diag_bench.py [out.json]   (env: N, WARM, REPS, ROUNDS; default
                                        out: profiles/flow_diag_<N>.json)
       flow_diag_bench.py --passes     (the traced child)

Phase A, the context as the steps leave it (no resident rho: 24 B/cell), ROUNDS
rounds of: REPS full passes (what = 3), REPS energy-only passes (what = 2).
Phase B, after HIP_FIELD_RHO and HIP_FIELD_T are filled (32 B/cell for the
diagnostics, 48 B/cell for the statistics), ROUNDS rounds of: REPS full, REPS
energy-only, REPS hip_proj_derived_statistics with the magnitude (the
streaming yardstick: same reduction scheme). Once: today's route to the same
numbers, hip_proj_get_field of u, v, w plus the host twin
cfd_flow_diagnostics; the two routes must agree (div_linf bitwise, sums to
the summation-order bound). Each timing starts after hip_proj_synchronize and
every entry ends with its own stream synchronisation and a 48-B readback, so
ms_per_call is a call's whole cost on the host clock. The kernels' own
durations come from the dispatch timestamps of `rocprofv3 --kernel-trace` on
a child process (--passes: the same state, each entry five times).
Algorithmic bytes: 8 B per cell and field read (u, v, w, and rho when
resident) over all nx*ny*nz cells. Prints and writes one JSON record."""
import csv
import ctypes as C
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402,F401
import torch  # noqa: E402,F401

from cfd_amd import _abi as A  # noqa: E402
from cfd_amd import _native, api  # noqa: E402

KERNELS = {"k_flow_diag<true>": ("k_flow_diag", "Lb1"), "k_flow_diag<false>": ("k_flow_diag", "Lb0"),
           "k_derived_stats<true>": ("k_derived_stats", "Lb1")}


def cavity_state(n, warm):
    c = api.HipProjection(n, n, n, cg_variant=1, poisson_method=A.HIP_POISSON_DST)
    for fid in (A.HIP_FIELD_U, A.HIP_FIELD_V, A.HIP_FIELD_W, A.HIP_FIELD_P):
        c.fill(fid, 0.0)
    c.set_density(1.0)
    g = api.Grid(n, n, n, 0.0, 1.0, 0.0, 1.0, 0.0, 1.0)
    prm = api.validation_params(1e-4, 1.0 / 1000.0)
    for _ in range(warm):
        c.apply_dirichlet(A.HIP_FIELD_U, api.dirichlet(top=1.0))
        c.apply_dirichlet(A.HIP_FIELD_V, api.dirichlet())
        c.apply_dirichlet(A.HIP_FIELD_W, api.dirichlet())
        c.apply_scalar_bc(A.HIP_FIELD_P, A.BC_TYPE_NEUMANN)
        s = c.step_device(g, prm)
        if s != A.CFD_SUCCESS:
            raise RuntimeError(f"step failed {s}: {_native.last_error()}")
    c.synchronize()
    return c, g


def passes_child():
    n = int(os.environ.get("N", "512"))
    ctx, g = cavity_state(n, 2)
    ctx.fill(A.HIP_FIELD_RHO, 1.0)
    ctx.fill(A.HIP_FIELD_T, 300.0)
    for _ in range(5):
        ctx.flow_diagnostics(g, 1.0, 3)
        ctx.flow_diagnostics(g, 1.0, 2)
        ctx.derived_statistics(True, 1.0)
    ctx.close()


def traced_kernels(n):
    """{kernel: median ms over its dispatches but the first} from the trace."""
    with tempfile.TemporaryDirectory() as tmp:
        prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
        cmd = [prof, "--kernel-trace", "--output-format", "csv", "-d", tmp,
               "--", sys.executable, str(Path(__file__).resolve()), "--passes"]
        r = subprocess.run(cmd, env=dict(os.environ, N=str(n)), capture_output=True, text=True,
                           timeout=600)
        if r.returncode != 0:
            return {"error": (r.stdout + r.stderr)[-800:]}
        ms = {k: [] for k in KERNELS}
        for f in Path(tmp).rglob("*kernel_trace.csv"):
            with open(f, newline="") as fh:
                for row in csv.DictReader(fh):
                    name = row.get("Kernel_Name", "")
                    for k, (stem, arg) in KERNELS.items():
                        if stem in name and (arg in name or k.split("<")[1] in name):
                            ms[k].append((int(row["Start_Timestamp"]),
                                          (int(row["End_Timestamp"]) -
                                           int(row["Start_Timestamp"])) * 1e-6))
    out = {}
    for k, v in ms.items():
        v.sort()
        if len(v) > 1:
            out[k] = {"ms": round(statistics.median(t for _, t in v[1:]), 4),
                      "dispatches": len(v)}
    return out or {"error": "no dispatch of the kernels in the trace"}


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--passes":
        return passes_child()
    n = int(os.environ.get("N", "512"))
    out = sys.argv[1] if len(sys.argv) > 1 else ROOT / "profiles" / f"flow_diag_{n}.json"
    warm = int(os.environ.get("WARM", "3"))
    reps = int(os.environ.get("REPS", "20"))
    rounds = int(os.environ.get("ROUNDS", "5"))
    cells = n ** 3
    lib = _native.hip()
    copy, triad = C.c_double(0.0), C.c_double(0.0)
    assert lib.cfd_hip_stream_bench(0, cells, 5, C.byref(copy), C.byref(triad)) == A.CFD_SUCCESS
    ctx, g = cavity_state(n, warm)

    def timed(fn, count):
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(count):
            fn()
        return (time.perf_counter() - t0) * 1e3 / count

    full = lambda: ctx.flow_diagnostics(g, 1.0, 3)  # noqa: E731
    energy = lambda: ctx.flow_diagnostics(g, 1.0, 2)  # noqa: E731
    derived = lambda: ctx.derived_statistics(True, 1.0)  # noqa: E731
    ms = {k: [] for k in ("full_24B", "energy_24B", "full_32B", "energy_32B", "derived_48B",
                          "download3", "host_twin")}
    full(), energy()  # warm-up: first launches, the lazy buffer
    for _ in range(rounds):
        ms["full_24B"].append(timed(full, reps))
        ms["energy_24B"].append(timed(energy, reps))
    dev = full()
    # today's route, once: three field downloads and the host loops
    f = api.FlowField(n, n, n)
    f.rho[...] = 1.0

    def download():
        for fid, a in ((A.HIP_FIELD_U, f.u), (A.HIP_FIELD_V, f.v), (A.HIP_FIELD_W, f.w)):
            assert lib.hip_proj_get_field(ctx.ctx, fid, a.ctypes.data_as(A.c_double_p)) == 0

    host = {}
    ms["download3"].append(timed(download, 1))
    ms["host_twin"].append(timed(lambda: host.update(d=api.flow_diagnostics(f, g, 1.0, 3)), 1))
    h = host["d"]
    assert dev.div_linf == h.div_linf and dev.div_cells == h.div_cells, (dev.div_linf, h.div_linf)
    agree = {}
    for k in ("div_sumsq", "ke", "ke_rho", "ke_rho_cells"):
        a, b = getattr(dev, k), getattr(h, k)
        agree[k] = abs(a - b) / abs(b) if b else abs(a)
        assert agree[k] <= 2.0 * cells * 2.0 ** -53, (k, a, b)
    del f

    ctx.fill(A.HIP_FIELD_RHO, 1.0)
    ctx.fill(A.HIP_FIELD_T, 300.0)
    full(), energy(), derived()
    for _ in range(rounds):
        ms["full_32B"].append(timed(full, reps))
        ms["energy_32B"].append(timed(energy, reps))
        ms["derived_48B"].append(timed(derived, reps))
    ctx.close()

    med = {k: statistics.median(v) for k, v in ms.items()}
    bpc = {"full_24B": 24, "energy_24B": 24, "full_32B": 32, "energy_32B": 32, "derived_48B": 48}
    gb = lambda b, t: round(b * cells / (t * 1e-3) / 1e9, 1)  # noqa: E731
    rec = {"n": n, "warm_steps": warm, "reps": reps, "rounds": rounds,
           "ms_per_call": {k: round(v, 4) for k, v in med.items()},
           "bytes_per_cell": bpc,
           "GBps_per_call": {k: gb(b, med[k]) for k, b in bpc.items()},
           "host_route_ms": round(med["download3"] + med["host_twin"], 1),
           "speedup_vs_host_route": round((med["download3"] + med["host_twin"])
                                          / med["full_24B"], 1),
           "stream_copy_GBps": round(copy.value, 1), "stream_triad_GBps": round(triad.value, 1),
           "device": {"div_linf": dev.div_linf, "div_l2": dev.div_l2, "ke": dev.ke,
                      "ke_rho_cells": dev.ke_rho_cells},
           "device_vs_host_rel": agree,
           "all_rounds_ms": {k: [round(t, 4) for t in v] for k, v in ms.items()}}
    traced = traced_kernels(n)
    if "error" in traced:
        rec["kernel_trace_error"] = traced["error"]
    else:
        kb = {"k_flow_diag<true>": 32, "k_flow_diag<false>": 32, "k_derived_stats<true>": 48}
        rec["kernel_ms"] = {k: dict(v, bytes_per_cell=kb[k], GBps=gb(kb[k], v["ms"]))
                            for k, v in traced.items()}
        d = rec["kernel_ms"].get("k_derived_stats<true>")
        for k in ("k_flow_diag<true>", "k_flow_diag<false>"):
            if d and k in rec["kernel_ms"]:
                rec["kernel_ms"][k]["rate_over_derived"] = round(
                    rec["kernel_ms"][k]["GBps"] / d["GBps"], 3)
    line = json.dumps(rec)
    print(line, flush=True)
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    Path(out).write_text(line + "\n")


if __name__ == "__main__":
    main()
