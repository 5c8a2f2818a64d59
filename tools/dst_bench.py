#!/usr/bin/env python3
"""The direct sine-transform pressure solve (HIP_POISSON_DST) against the
single-reduction CG (cg_variant 1) at n^3, on the lid-driven cavity step's own
pressure problem.
usage: dst_bench.py [out.json]            (N=512 WARM=3 ROUNDS=3 in the environment)
       dst_bench.py --passes              (the traced child: two DST solves)

One context (cg_variant 1, poisson_method DST) runs WARM cavity steps
(Re 1000, dt 1e-4; each timed). The last step's pressure problem is rebuilt on
the host: x0 = p before the step, rhs = lap(p after it), which is the step's
right-hand side to the direct solve's residual (1e-15 of it). Then ROUNDS
rounds of: one DST solve of it (device ms from the solve's own two events,
stats.elapsed_time_ms), one CG solve of it to the default tolerance (device ms
= the sum of its kernels' dispatch-packet times). A second context
(poisson_method CG) times the same steps with CG. The transform passes are
timed by `rocprofv3 --kernel-trace --stats` on a child process of its own
(--passes: random right-hand side; a pass's time does not depend on the data).
Prints and writes one JSON record."""
import csv
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

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401

from cfd_amd import _abi as A  # noqa: E402
from cfd_amd import _native, api  # noqa: E402

DST = A.HIP_POISSON_DST


def cavity_ctx(n, **cfg):
    c = api.HipProjection(n, n, n, **cfg)
    for fid in (A.HIP_FIELD_U, A.HIP_FIELD_V, A.HIP_FIELD_W, A.HIP_FIELD_P):
        c.fill(fid, 0.0)
    c.set_density(1.0)
    c.apply_dirichlet(A.HIP_FIELD_U, api.dirichlet(top=1.0))
    c.apply_dirichlet(A.HIP_FIELD_V, api.dirichlet())
    c.apply_dirichlet(A.HIP_FIELD_W, api.dirichlet())
    c.apply_scalar_bc(A.HIP_FIELD_P, A.BC_TYPE_NEUMANN)
    c.synchronize()
    return c


def timed_steps(ctx, g, prm, nsteps, before_last=None):
    ms, stats = [], []
    for i in range(nsteps):
        if before_last and i == nsteps - 1:
            before_last()
        ctx.synchronize()
        t0 = time.perf_counter()
        s = ctx.step_device(g, prm)
        ctx.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        if s != A.CFD_SUCCESS:
            raise RuntimeError(f"step failed {s}: {_native.last_error()}")
        st = ctx.poisson_stats()
        stats.append((st.iterations, st.initial_residual, st.final_residual))
    return ms, stats


def host_laplacian(p, h):
    out = np.zeros_like(p)
    c = p[1:-1, 1:-1, 1:-1]
    acc = p[1:-1, 1:-1, 2:] + p[1:-1, 1:-1, :-2]
    acc += p[1:-1, 2:, 1:-1]
    acc += p[1:-1, :-2, 1:-1]
    acc += p[2:, 1:-1, 1:-1]
    acc += p[:-2, 1:-1, 1:-1]
    acc -= 6.0 * c
    acc /= h * h
    out[1:-1, 1:-1, 1:-1] = acc
    return out


def passes_child():
    n = int(os.environ.get("N", "512"))
    rng = np.random.default_rng(n)
    rhs = rng.standard_normal((n, n, n))
    d = 1.0 / (n - 1)
    ctx = api.HipProjection(n, n, n)
    for _ in range(2):
        x = np.zeros((n, n, n))
        ctx.poisson_solve(DST, x, rhs, d, d, d)
    ctx.close()


def traced_passes(n):
    """[(kernel, ms)] of the last solve's transform passes, in launch order."""
    with tempfile.TemporaryDirectory() as tmp:
        prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp,
               "--", sys.executable, str(Path(__file__).resolve()), "--passes"]
        r = subprocess.run(cmd, env=dict(os.environ, N=str(n)), capture_output=True, text=True,
                           timeout=900)
        if r.returncode != 0:
            return {"error": (r.stdout + r.stderr)[-800:]}
        rows = []
        for f in Path(tmp).rglob("*kernel_trace.csv"):
            with open(f, newline="") as fh:
                for row in csv.DictReader(fh):
                    if "k_dst" in row.get("Kernel_Name", ""):
                        rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]),
                                     row["Kernel_Name"]))
    rows.sort()
    if not rows:
        return {"error": "no k_dst dispatch in the kernel trace"}
    per = len(rows) // 2  # two solves
    out = []
    for t0, t1, name in rows[-per:]:
        short = "k_dst_x" if "k_dst_x" in name else "k_dst_strided"
        if "Lb1" in name or "<true>" in name:
            short += "<fused>"
        out.append((short, (t1 - t0) * 1e-6))
    return {"passes": out}


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--passes":
        return passes_child()
    out = sys.argv[1] if len(sys.argv) > 1 else None
    n = int(os.environ.get("N", "512"))
    warm = max(2, int(os.environ.get("WARM", "3")))
    rounds = int(os.environ.get("ROUNDS", "3"))
    h = 1.0 / (n - 1)
    g = api.Grid(n, n, n, 0.0, 1.0, 0.0, 1.0, 0.0, 1.0)
    prm = api.validation_params(1e-4, 1.0 / 1000.0)
    keep = {}
    ctx = cavity_ctx(n, cg_variant=1, poisson_method=DST)
    try:
        dst_step_ms, dst_step_stats = timed_steps(
            ctx, g, prm, warm, lambda: keep.update(x0=ctx.get_field(A.HIP_FIELD_P)))
        p1 = ctx.get_field(A.HIP_FIELD_P)
        rhs = host_laplacian(p1, h)
        del p1
        x0 = keep["x0"]
        dst_ms, cg_ms, cg_its, res = [], [], [], {}
        for _ in range(rounds):
            x = x0.copy()
            s, st = ctx.poisson_solve(DST, x, rhs, h, h, h)
            assert s == A.CFD_SUCCESS and st.iterations == 1, (s, st.iterations)
            dst_ms.append(st.elapsed_time_ms)
            res["dst"] = (st.initial_residual, st.final_residual)
            x = x0.copy()
            ctx.reset_timing()
            ctx.enable_timing(True)
            s, st = ctx.poisson_solve(A.HIP_POISSON_CG, x, rhs, h, h, h)
            kt = ctx.timing()
            ctx.enable_timing(False)
            assert s == A.CFD_SUCCESS, (s, _native.last_error())
            cg_ms.append(sum(v[0] for v in kt.values()))
            cg_its.append(st.iterations)
            res["cg"] = (st.initial_residual, st.final_residual)
    finally:
        ctx.close()
    del rhs, x0, x, keep
    ctx = cavity_ctx(n, cg_variant=1)
    try:
        cg_step_ms, cg_step_stats = timed_steps(ctx, g, prm, warm)
    finally:
        ctx.close()
    traced = traced_passes(n)
    cells = float(n - 2) ** 3
    flop_pass = 2.0 * (n - 2) * cells  # one dense product with S_n per line
    rec = {"n": n, "rounds": rounds, "warm_steps": warm,
           "dst_solve_ms": [round(v, 3) for v in dst_ms],
           "cg_solve_ms": [round(v, 2) for v in cg_ms], "cg_iterations": cg_its,
           "dst_solve_ms_median": round(statistics.median(dst_ms), 3),
           "cg_solve_ms_median": round(statistics.median(cg_ms), 2),
           "cg_over_dst": round(statistics.median(cg_ms) / statistics.median(dst_ms), 2),
           "residuals": res,
           "dst_step_ms": [round(v, 2) for v in dst_step_ms],
           "cg_step_ms": [round(v, 2) for v in cg_step_ms],
           "dst_step_stats": dst_step_stats, "cg_step_stats": cg_step_stats,
           "flop_per_pass": flop_pass}
    if "passes" in traced:
        rec["passes"] = [{"kernel": k, "ms": round(ms, 3),
                          "fp64_tflops": round(flop_pass / (ms * 1e-3) / 1e12, 2)}
                         for k, ms in traced["passes"]]
    else:
        rec["passes_error"] = traced["error"]
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        Path(out).write_text(line + "\n")


if __name__ == "__main__":
    main()
