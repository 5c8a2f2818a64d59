#!/usr/bin/env python3
"""Writes the BiCGSTAB fixtures from the reference's own CPU solver
(poisson_solver_create(POISSON_METHOD_BICGSTAB, POISSON_BACKEND_SCALAR), then
poisson_solver_init and poisson_solver_solve) on every case of
tests/bicgstab_cases.py:

  tests/golden/bicgstab_cases.json  per case: shape, parameters, status,
                                    return code, iterations, both residuals
                                    as hex floats, sha256 + sum / L2 / max of x
  tests/golden/bicgstab_x.npz       full x of the cases of <= 10 000 cells

The reference is built unmodified by make_rk_golden.build_reference (copied
to a work directory, its own CMake, CPU only, -ffp-contract=off). Nothing
built from the reference and none of its text is written into this
repository: only the numbers its solver produces.

usage: make_bicgstab_golden.py [--work DIR] [--jobs N]
"""
import argparse
import ctypes as C
import hashlib
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))
OUT = Path(__file__).resolve().parent


def digest(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return {"sha256": hashlib.sha256(a.tobytes()).hexdigest(), "sum": float(a.sum()).hex(),
            "l2": float(np.sqrt(np.sum(a * a))).hex(), "max": float(np.max(np.abs(a))).hex()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--work", default="/tmp/cfd_rk_golden")
    ap.add_argument("--jobs", type=int, default=8)
    a = ap.parse_args()
    work = Path(a.work)
    work.mkdir(parents=True, exist_ok=True)
    from make_rk_golden import build_reference
    ref = C.CDLL(str(build_reference(work, a.jobs)))

    from cfd_amd import _abi as A
    from tests import bicgstab_cases as K
    from tests import cg_seam_shapes as T

    P = C.POINTER
    ref.poisson_solver_create.restype = P(A.PoissonSolver)
    ref.poisson_solver_create.argtypes = [C.c_int, C.c_int]
    ref.poisson_solver_params_default.restype = A.PoissonParams
    ref.poisson_solver_init.restype = C.c_int
    ref.poisson_solver_init.argtypes = [P(A.PoissonSolver), C.c_size_t, C.c_size_t, C.c_size_t,
                                        C.c_double, C.c_double, C.c_double, P(A.PoissonParams)]
    ref.poisson_solver_solve.restype = C.c_int
    ref.poisson_solver_solve.argtypes = [P(A.PoissonSolver), A.c_double_p, A.c_double_p,
                                         A.c_double_p, P(A.PoissonStats)]
    ref.poisson_solver_destroy.restype = None
    ref.poisson_solver_destroy.argtypes = [P(A.PoissonSolver)]

    doc = {"reference": "shaia/CFD v0.3.0, create_bicgstab_scalar_solver",
           "build_flags": "-DCMAKE_BUILD_TYPE=Release -DCMAKE_C_FLAGS=-ffp-contract=off",
           "cases": {}}
    npz = {}
    for case in K.CASES:
        rhs, x0 = K.inputs(case)
        nx, ny, nz = case["shape"]
        dx, dy, dz = T.spacing(case["shape"])
        s = ref.poisson_solver_create(A.POISSON_METHOD_BICGSTAB, A.POISSON_BACKEND_SCALAR)
        if not s:
            raise SystemExit("make_bicgstab_golden: poisson_solver_create returned NULL")
        prm = ref.poisson_solver_params_default()
        for k, v in K.solver_params(case).items():
            setattr(prm, k, v)
        if ref.poisson_solver_init(s, nx, ny, nz, dx, dy, dz, C.byref(prm)) != A.CFD_SUCCESS:
            raise SystemExit(f"make_bicgstab_golden: {case['name']}: init failed")
        x = np.array(x0, dtype=np.float64)
        b = np.array(rhs, dtype=np.float64)
        xt = np.zeros_like(x)
        st = A.PoissonStats()
        rc = ref.poisson_solver_solve(s, x.ctypes.data_as(A.c_double_p),
                                      xt.ctypes.data_as(A.c_double_p),
                                      b.ctypes.data_as(A.c_double_p), C.byref(st))
        ref.poisson_solver_destroy(s)
        if not np.all(np.isfinite(x)):
            raise SystemExit(f"make_bicgstab_golden: {case['name']}: x not finite")
        doc["cases"][case["name"]] = {
            "shape": list(case["shape"]), "kind": case["kind"], "params": K.solver_params(case),
            "inputs": {"rhs": hashlib.sha256(b.tobytes()).hexdigest(),
                       "x0": hashlib.sha256(np.ascontiguousarray(x0).tobytes()).hexdigest()},
            "status": int(st.status), "rc": int(rc), "iterations": int(st.iterations),
            "initial_residual": float(st.initial_residual).hex(),
            "final_residual": float(st.final_residual).hex(), "x": digest(x)}
        if K.in_npz(case):
            npz[case["name"]] = x
    (OUT / K.JSON_FILE).write_text(json.dumps(doc, indent=1) + "\n")
    np.savez_compressed(OUT / K.NPZ_FILE, **npz)
    print(json.dumps({"cases": len(doc["cases"]), "npz": len(npz), "work": str(work)}))


if __name__ == "__main__":
    sys.exit(main())
