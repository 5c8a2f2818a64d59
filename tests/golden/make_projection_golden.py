#!/usr/bin/env python3
"""Writes the buoyant / sourced / energy-coupled projection fixtures from the
reference's own CPU solver, solve_projection_method (the oracle restates it;
tests/test_projection_fixtures.py holds the restatement to this record):

  tests/golden/projection_buoyant_cases.json   per case of tests/buoyant_cases.py
                                               (every table entry under "all" and
                                               with exactly one of buoyancy, sources
                                               and energy on): sha256 of the inputs,
                                               and per call pattern the status and
                                               sha256 + sum / L2 / max of u, v, w, p, T
  tests/golden/projection_buoyant_17x13x11.npz full u, v, w, p, T of the 17 x 13 x 11
                                               "all" case, both call patterns

Call patterns: "steps" is three calls with max_iter = 1 (step index 0 in the
source terms every time), "iter" one call with max_iter = 3 (step index 0, 1,
2: the sources decay by exp(-0.2) per step).

The reference is built exactly as for tests/golden/make_rk_golden.py (its
build_reference: an unmodified copy, its own CMake, CPU only,
-ffp-contract=off, the static archives linked into one shared object in the
work directory and loaded with ctypes). Nothing built from the reference and
none of its text is written into this repository: only the numbers its
solver produces. The .npz is written with fixed zip timestamps, so a rerun
reproduces both files byte for byte.

usage: make_projection_golden.py [--work DIR] [--jobs N] [--out DIR]
"""
import argparse
import ctypes as C
import io
import json
import sys
import zipfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(HERE))

from make_rk_golden import build_reference  # noqa: E402


def write_npz(path: Path, arrays: dict) -> None:
    """np.savez_compressed with a fixed timestamp on every member."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--work", default="/tmp/cfd_projection_golden")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--out", default=str(HERE))
    a = ap.parse_args()
    work, out = Path(a.work), Path(a.out)
    work.mkdir(parents=True, exist_ok=True)
    ref = C.CDLL(str(build_reference(work, a.jobs)))

    from cfd_amd import _abi as A
    from cfd_amd import api
    from tests import buoyant_cases as B
    from tests import rk_cases as R

    solve = ref.solve_projection_method
    solve.restype = C.c_int
    solve.argtypes = [C.POINTER(A.FlowField), C.POINTER(A.Grid), C.POINTER(A.SolverParams)]

    doc = {"reference": "shaia/CFD v0.3.0, solve_projection_method (CPU scalar, CG)",
           "build_flags": "-DCMAKE_BUILD_TYPE=Release -DCMAKE_C_FLAGS=-ffp-contract=off",
           "fields": list(B.FIELDS), "steps": B.STEPS, "cases": {}}
    npz = {}
    for name, shape, thermal, terms in B.all_cases():
        g, f0, p0 = B.case(shape, thermal, terms)
        rec = {"shape": list(shape), "thermal": thermal, "terms": terms,
               "inputs": {k: R.sha(getattr(f0, k)) for k in B.INPUTS}, "runs": {}}
        for pattern in B.PATTERNS:
            f = api.FlowField(*shape)
            f.copy_from(f0)
            p = A.SolverParams.from_buffer_copy(p0)
            p.max_iter = B.STEPS if pattern == "iter" else 1
            status = A.CFD_SUCCESS
            for _ in range(1 if pattern == "iter" else B.STEPS):
                status = int(solve(f.ptr, g.ptr, C.byref(p)))
                if status != A.CFD_SUCCESS:
                    raise SystemExit(f"make_projection_golden: {name} {pattern}: status {status}")
            for k in B.FIELDS:
                if not np.all(np.isfinite(getattr(f, k))):
                    raise SystemExit(f"make_projection_golden: {name} {pattern}: {k} not finite")
            rec["runs"][pattern] = {"max_iter": int(p.max_iter), "status": status,
                                    "outputs": {k: R.digest(getattr(f, k)) for k in B.FIELDS}}
            if (shape, thermal, terms) == B.NPZ_CASE:
                for k in B.FIELDS:
                    npz[f"{pattern}_{k}"] = getattr(f, k).copy()
        doc["cases"][name] = rec
    (out / B.JSON_FILE).write_text(json.dumps(doc, indent=1) + "\n")
    write_npz(out / B.NPZ_FILE, npz)
    print(json.dumps({"cases": len(doc["cases"]), "work": str(work), "out": str(out)}))


if __name__ == "__main__":
    sys.exit(main())
