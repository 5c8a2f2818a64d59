#!/usr/bin/env python3
"""The direct cosine-transform pressure solve (HIP_POISSON_DCT) against the
Red-Black SOR solve at the reference tolerance, on the pressure problem of the
natural-convection step (configs[4] of bench.py, its own convection_setup).
usage: dct_bench.py [out.json]     (NX=512 NY=512 NZ=256 WARM=2 ROUNDS=3 in the environment;
                                    the flagship grid is NX=1024 NY=1024 NZ=512)
       dct_bench.py --passes       (the traced child: two DCT solves)

One context (poisson_method REDBLACK, bench.py's settings) runs WARM convection
steps, each timed. The last step's pressure problem is rebuilt on the host:
x0 = p before the step, rhs = lap(p after it) with p's Neumann shell, which is
a compatible right-hand side by construction and the step's own to the RB-SOR
tolerance. Then ROUNDS rounds on that context of: one DCT solve of it (device
ms from the solve's own two events, stats.elapsed_time_ms), one RB-SOR solve of
it at the reference tolerance 1e-6 (device ms = the sum of its kernels'
dispatch-packet times). A second context (poisson_method DCT) times the same
steps with the direct solve. The transform passes are timed by
`rocprofv3 --kernel-trace --stats` on a child process of its own (--passes:
random right-hand side; a pass's time does not depend on the data).
Prints and writes one JSON record; the speedup is reported, not gated."""
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

import bench  # noqa: E402
from cfd_amd import _abi as A  # noqa: E402
from cfd_amd import _native, api  # noqa: E402

DCT = A.HIP_POISSON_DCT
RB = A.HIP_POISSON_REDBLACK
RELAX_TOL, RELAX_MAX_ITER = 1e-6, 20000  # bench.py's --relax-tol / --relax-max-iter defaults


def progress(msg):
    print(f"[dct_bench] {msg}", file=sys.stderr, flush=True)


def shape_env():
    return (int(os.environ.get("NX", "512")), int(os.environ.get("NY", "512")),
            int(os.environ.get("NZ", "256")))


def convection_ctx(nx, ny, nz, T0, method):
    c = api.HipProjection(nx, ny, nz, poisson_method=method, poisson_max_iter=RELAX_MAX_ITER,
                          poisson_tolerance=RELAX_TOL, relax_two_pass=0)
    for fid in (A.HIP_FIELD_U, A.HIP_FIELD_V, A.HIP_FIELD_W, A.HIP_FIELD_P):
        c.fill(fid, 0.0)
    c.set_field(A.HIP_FIELD_T, np.broadcast_to(T0[None, None, :], c.shape))
    c.set_density(1.0)
    for fid in (A.HIP_FIELD_U, A.HIP_FIELD_V, A.HIP_FIELD_W):
        c.apply_dirichlet(fid, api.dirichlet())
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
        stats.append((st.status, st.iterations, st.initial_residual, st.final_residual))
    return ms, stats


def host_laplacian(p, d):
    out = np.zeros_like(p)
    c = p[1:-1, 1:-1, 1:-1]
    acc = (p[1:-1, 1:-1, 2:] + p[1:-1, 1:-1, :-2] - 2.0 * c) / (d[0] * d[0])
    acc += (p[1:-1, 2:, 1:-1] + p[1:-1, :-2, 1:-1] - 2.0 * c) / (d[1] * d[1])
    acc += (p[2:, 1:-1, 1:-1] + p[:-2, 1:-1, 1:-1] - 2.0 * c) / (d[2] * d[2])
    out[1:-1, 1:-1, 1:-1] = acc
    return out


def demeaned_dev(a, b):
    ia, ib = a[1:-1, 1:-1, 1:-1], b[1:-1, 1:-1, 1:-1]
    da, db = ia - ia.mean(), ib - ib.mean()
    return float(np.max(np.abs(da - db)) / np.max(np.abs(db)))


def passes_child():
    nx, ny, nz = shape_env()
    rng = np.random.default_rng(nx + ny + nz)
    rhs = rng.standard_normal((nz, ny, nx))
    rhs[1:-1, 1:-1, 1:-1] -= rhs[1:-1, 1:-1, 1:-1].mean()
    d = (1.0 / (nx - 1), 1.0 / (ny - 1), 0.5 / (nz - 1))
    ctx = api.HipProjection(nx, ny, nz)
    for _ in range(2):
        x = np.zeros((nz, ny, nx))
        ctx.poisson_solve(DCT, x, rhs, *d)
    ctx.close()


def traced_passes(shape):
    """[(kernel, axis length, ms)] of the last solve's transform passes, in launch order."""
    nx, ny, nz = shape
    with tempfile.TemporaryDirectory() as tmp:
        prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp,
               "--", sys.executable, str(Path(__file__).resolve()), "--passes"]
        r = subprocess.run(cmd, env=dict(os.environ, NX=str(nx), NY=str(ny), NZ=str(nz)),
                           capture_output=True, text=True, timeout=900)
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
    if len(rows) != 12:
        return {"error": f"{len(rows)} k_dst dispatches in the kernel trace, not 12"}
    # the solve's order: x, y, z forward; z, y, x inverse
    order = [("x", nx - 2), ("y", ny - 2), ("z", nz - 2), ("z", nz - 2), ("y", ny - 2),
             ("x", nx - 2)]
    out = []
    for (t0, t1, name), (axis, n), q in zip(rows[-6:], order, range(6)):
        short = "k_dst_x" if "k_dst_x" in name else "k_dst_strided"
        out.append((f"{short} {axis} {'forward' if q < 3 else 'inverse'}", n, (t1 - t0) * 1e-6))
    return {"passes": out}


def relax_params():
    """The reference's solver defaults with bench.py's tolerance and cap."""
    p = _native.host().poisson_solver_params_default()
    p.tolerance = RELAX_TOL
    p.max_iterations = RELAX_MAX_ITER
    return p


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--passes":
        return passes_child()
    out = sys.argv[1] if len(sys.argv) > 1 else None
    nx, ny, nz = shape_env()
    warm = max(2, int(os.environ.get("WARM", "2")))
    rounds = int(os.environ.get("ROUNDS", "3"))
    g, prm, T0 = bench.convection_setup(nx, ny, nz)
    d = (1.0 / (nx - 1), 1.0 / (ny - 1), 0.5 / (nz - 1))
    keep = {}
    ctx = convection_ctx(nx, ny, nz, T0, RB)
    try:
        rb_step_ms, rb_step_stats = timed_steps(
            ctx, g, prm, warm, lambda: keep.update(x0=ctx.get_field(A.HIP_FIELD_P)))
        progress(f"RB-SOR steps {[round(v) for v in rb_step_ms]} ms")
        p1 = ctx.get_field(A.HIP_FIELD_P)
        rhs = host_laplacian(p1, d)
        del p1
        x0 = keep["x0"]
        dct_ms, rb_ms, rb_its, res, dev = [], [], [], {}, None
        for _ in range(rounds):
            xd = x0.copy()
            s, st = ctx.poisson_solve(DCT, xd, rhs, *d)
            assert st.iterations == 1, (s, st.iterations, _native.last_error())
            dct_ms.append(st.elapsed_time_ms)
            res["dct"] = (st.status, st.initial_residual, st.final_residual)
            xr = x0.copy()
            ctx.reset_timing()
            ctx.enable_timing(True)
            s, st = ctx.poisson_solve(RB, xr, rhs, *d, relax_params())
            kt = ctx.timing()
            ctx.enable_timing(False)
            assert s == A.CFD_SUCCESS, (s, _native.last_error())
            rb_ms.append(sum(v[0] for v in kt.values()))
            rb_its.append(st.iterations)
            res["rbsor"] = (st.status, st.initial_residual, st.final_residual)
            progress(f"round: DCT {dct_ms[-1]:.3f} ms, RB-SOR {rb_ms[-1]:.1f} ms")
        dev = demeaned_dev(xd, xr)
    finally:
        ctx.close()
    del rhs, x0, xd, xr, keep
    ctx = convection_ctx(nx, ny, nz, T0, DCT)
    try:
        dct_step_ms, dct_step_stats = timed_steps(ctx, g, prm, warm)
        progress(f"DCT steps {[round(v, 1) for v in dct_step_ms]} ms")
    finally:
        ctx.close()
    traced = traced_passes((nx, ny, nz))
    cells = float(nx - 2) * float(ny - 2) * float(nz - 2)
    rec = {"grid": [nx, ny, nz], "flagship_grid": [1024, 1024, 512],
           "rounds": rounds, "warm_steps": warm, "relax_tol": RELAX_TOL,
           "dct_solve_ms": [round(v, 3) for v in dct_ms],
           "rbsor_solve_ms": [round(v, 2) for v in rb_ms], "rbsor_iterations": rb_its,
           "dct_solve_ms_median": round(statistics.median(dct_ms), 3),
           "rbsor_solve_ms_median": round(statistics.median(rb_ms), 2),
           "rbsor_over_dct": round(statistics.median(rb_ms) / statistics.median(dct_ms), 2),
           "residuals": res, "x_demeaned_dct_minus_rbsor_rel": dev,
           "rbsor_step_ms": [round(v, 2) for v in rb_step_ms],
           "dct_step_ms": [round(v, 2) for v in dct_step_ms],
           "rbsor_step_stats": rb_step_stats, "dct_step_stats": dct_step_stats}
    if "passes" in traced:
        rec["passes"] = [{"kernel": k, "n": n, "ms": round(ms, 3),
                          "fp64_tflops": round(2.0 * n * cells / (ms * 1e-3) / 1e12, 2)}
                         for k, n, ms in traced["passes"]]
    else:
        rec["passes_error"] = traced["error"]
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        Path(out).write_text(line + "\n")


if __name__ == "__main__":
    main()
