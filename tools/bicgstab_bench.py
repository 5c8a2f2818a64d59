#!/usr/bin/env python3
"""BiCGSTAB launch timing at n^3, interleaved with textbook CG on one context.
usage: bicgstab_bench.py [out.json] ["sweep_rows=16,sweep_variant=15"]
ROUNDS rounds of: ITERS capped BiCGSTAB iterations (tolerance 0), then ITERS
fixed CG iterations, both with dispatch-packet timing, same box, same process.
Prints and writes one JSON record: per-launch microseconds (median over the
rounds), ms per iteration, and each launch's algorithmic-byte rate
(k_bcg_v 48, k_bcg_t 32, k_bcg_x 56 B/cell; CG sweeps 24 / 24 / 64 B/cell)."""
import json
import os
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401

from cfd_amd import _abi as A  # noqa: E402
from cfd_amd import api  # noqa: E402
from oracle import oracle  # noqa: E402

BCG_BYTES = {"bcg_v": 48, "bcg_t": 32, "bcg_x": 56}
CG_BYTES = {"cg_sweep_a": 24, "cg_sweep_b": 24, "cg_sweep_bx": 64}


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    spec = sys.argv[2] if len(sys.argv) > 2 else "sweep_rows=16,sweep_variant=15"
    n = int(os.environ.get("N", "512"))
    iters = int(os.environ.get("ITERS", "50"))
    rounds = int(os.environ.get("ROUNDS", "3"))
    kw = {k: int(v) for k, v in (item.split("=") for item in filter(None, spec.split(",")))}
    rng = np.random.default_rng(n)
    rhs = rng.standard_normal((n, n, n))
    d = 1.0 / (n - 1)
    cells = (n - 2) ** 3
    prm = oracle.poisson_params(max_iterations=iters, tolerance=0.0, absolute_tolerance=0.0)
    ctx = api.HipProjection(n, n, n, **kw)
    us = {k: [] for k in list(BCG_BYTES) + list(CG_BYTES)}
    x = np.zeros((n, n, n))
    s, st = ctx.poisson_solve(A.HIP_POISSON_BICGSTAB, x, rhs, d, d, d, prm)  # warm-up
    ctx.cg_fixed_iters(rhs, d, d, d, 10)
    stats = None
    for _ in range(rounds):
        x[...] = 0.0
        ctx.reset_timing()
        ctx.enable_timing(True)
        s, st = ctx.poisson_solve(A.HIP_POISSON_BICGSTAB, x, rhs, d, d, d, prm)
        kt = ctx.timing()
        assert s == A.CFD_ERROR_MAX_ITER and st.iterations == iters, (s, st.iterations)
        for k in BCG_BYTES:
            assert kt[k][1] == iters, (k, kt[k])
            us[k].append(kt[k][0] / kt[k][1] * 1e3)
        stats = (st.initial_residual, st.final_residual)
        ctx.reset_timing()
        ctx.cg_fixed_iters(rhs, d, d, d, iters)
        kt = ctx.timing()
        ctx.enable_timing(False)
        for k in CG_BYTES:
            if kt[k][1]:
                us[k].append(kt[k][0] / kt[k][1] * 1e3)
    ctx.close()
    med = {k: statistics.median(v) for k, v in us.items() if v}
    rec = {"n": n, "iters": iters, "rounds": rounds, "cfg": spec,
           "launch_us": {k: round(v, 1) for k, v in med.items()},
           "GBps": {k: round({**BCG_BYTES, **CG_BYTES}[k] * cells / (v * 1e-6) / 1e9, 1)
                    for k, v in med.items()},
           "bicgstab_ms_per_iter": round(sum(med[k] for k in BCG_BYTES) / 1e3, 4),
           # a CG iteration: sweep A (every 4th: the x-fold form) + sweep B
           "cg_ms_per_iter": round((0.75 * med["cg_sweep_a"] + 0.25 * med["cg_sweep_bx"] +
                                    med["cg_sweep_b"]) / 1e3, 4),
           "bicgstab_bytes_per_cell": sum(BCG_BYTES.values()),
           "residual_after": {"initial": stats[0], "final": stats[1]},
           "all_rounds_us": {k: [round(t, 1) for t in v] for k, v in us.items()}}
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        Path(out).write_text(line + "\n")


if __name__ == "__main__":
    main()
