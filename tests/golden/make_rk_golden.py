#!/usr/bin/env python3
"""Writes the explicit Euler / RK2 fixtures from the reference's own CPU
solvers (the oracle restates neither integrator):

  tests/golden/euler_rk2_cases.json     per case and integrator: sha256 of the
                                        inputs, sha256 + sum / L2 / max of every
                                        output field, shape, flags, dt, steps,
                                        call pattern; for stretched grids sha256 of
                                        x, y, dx, dy; `refusals`: the status of
                                        each solver on two inputs it refuses
  tests/golden/euler_rk2_17x13x11.npz   full output fields of case "s17"
  tests/golden/euler_rk2_st17x13x11.npz full output fields of case "st17"

The reference checkout (CFD_REFERENCE_DIR, else `reference` beside this
repository) is copied to a work directory and built there unmodified with its
own CMake (CPU only, -DCMAKE_POSITION_INDEPENDENT_CODE=ON
-DCMAKE_C_FLAGS=-ffp-contract=off), target cfd_api; the five static archives
are linked into one shared object (--whole-archive), loaded with ctypes, and
explicit_euler_impl / rk2_impl / rk4_impl are called on the struct mirrors of
cfd_amd/_abi.py. Nothing built from the reference and none of its text is
written into this repository: only the numbers its solvers produce.

rk4_impl runs on every case too, always as single steps (the oracle's
rk4_step takes source index 0), so that tests/test_rk_fixtures.py can tie
this build's arithmetic to the oracle's bit for bit.

usage: make_rk_golden.py [--work DIR] [--jobs N]
"""
import argparse
import ctypes as C
import json
import os
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
REF = Path(os.environ.get("CFD_REFERENCE_DIR") or ROOT.parent / "reference")
OUT = Path(__file__).resolve().parent
ARCHIVES = ["libcfd_api.a", "libcfd_core.a", "libcfd_scalar.a", "libcfd_simd.a", "libcfd_omp.a"]
IMPL = {"euler": "explicit_euler_impl", "rk2": "rk2_impl", "rk4": "rk4_impl"}


def run(cmd):
    r = subprocess.run(list(map(str, cmd)), capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"make_rk_golden: {' '.join(map(str, cmd))} failed ({r.returncode}):\n"
                         + (r.stdout + r.stderr)[-4000:])
    return r.stdout


def build_reference(work: Path, jobs: int) -> Path:
    if not REF.is_dir():
        raise SystemExit(f"make_rk_golden: {REF} is absent")
    src, bld = work / "src", work / "build"
    for d in (src, bld):
        if d.exists():
            shutil.rmtree(d)
    shutil.copytree(REF, src, ignore=shutil.ignore_patterns(".git", "build*", "*.so", "*.a",
                                                           "ext_bin"))
    gen = ["-G", "Ninja"] if shutil.which("ninja") else []
    run(["cmake", "-S", src, "-B", bld, *gen, "-DCMAKE_BUILD_TYPE=Release", "-DBUILD_TESTS=OFF",
         "-DBUILD_EXAMPLES=OFF", "-DBUILD_SHARED_LIBS=OFF",
         "-DCMAKE_POSITION_INDEPENDENT_CODE=ON", "-DCMAKE_C_FLAGS=-ffp-contract=off"])
    run(["cmake", "--build", bld, "--target", "cfd_api", "-j", jobs])
    libs = {p.name: p for p in bld.rglob("libcfd_*.a")}
    missing = [n for n in ARCHIVES if n not in libs]
    if missing:
        raise SystemExit(f"make_rk_golden: archives not built: {missing}")
    so = work / "libcfd_reference.so"
    run(["gcc", "-shared", "-o", so, "-Wl,--whole-archive", *[libs[n] for n in ARCHIVES],
         "-Wl,--no-whole-archive", "-fopenmp", "-lm", "-ldl"])
    return so


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--work", default="/tmp/cfd_rk_golden")
    ap.add_argument("--jobs", type=int, default=8)
    a = ap.parse_args()
    work = Path(a.work)
    work.mkdir(parents=True, exist_ok=True)
    ref = C.CDLL(str(build_reference(work, a.jobs)))

    from cfd_amd import _abi as A
    from cfd_amd import api
    from tests import rk_cases as R

    for fn in IMPL.values():
        f = getattr(ref, fn)
        f.restype = C.c_int
        f.argtypes = [C.POINTER(A.FlowField), C.POINTER(A.Grid), C.POINTER(A.SolverParams)]

    doc = {"reference": "shaia/CFD v0.3.0, CPU scalar solvers",
           "build_flags": "-DCMAKE_BUILD_TYPE=Release -DCMAKE_C_FLAGS=-ffp-contract=off",
           "fields": list(R.FIELDS), "iter_decay_rate": R.ITER_DECAY, "cases": {}}
    npz = {}
    for case in R.CASES:
        g, f0, p0 = R.make_inputs(case)
        rec = {"shape": list(case["shape"]), "buoy": case["buoy"], "energy": case["energy"],
               "seed": case["seed"], "inputs": {k: R.sha(getattr(f0, k)) for k in R.FIELDS},
               "runs": {}}
        if case["stretch"]:
            rec["grid"] = {k: R.sha(v) for k, v in R.grid_arrays(g).items()}
        for integ in R.INTEGRATORS:
            f = api.FlowField(*case["shape"])
            f.copy_from(f0)
            p = A.SolverParams.from_buffer_copy(p0)
            # RK4 is the tie to the oracle, which only steps with source index 0
            pattern = "steps" if integ == "rk4" else case["pattern"]
            calls = R.params_for(case, integ, p, pattern)
            first = None
            for _ in range(calls):
                s = getattr(ref, IMPL[integ])(f.ptr, g.ptr, C.byref(p))
                if s != A.CFD_SUCCESS:
                    raise SystemExit(f"make_rk_golden: {case['name']} {integ}: status {s}")
                if first is None:
                    first = f.arrays()
            for k in R.FIELDS:
                if not np.all(np.isfinite(getattr(f, k))):
                    raise SystemExit(f"make_rk_golden: {case['name']} {integ}: {k} not finite")
            run_rec = {"dt": R.case_dt(case, integ), "steps": R.case_steps(case, integ),
                       "pattern": pattern,
                       "outputs": {k: R.digest(getattr(f, k)) for k in R.FIELDS}}
            if case["guard"] and integ == "euler":
                # both guards must act on the committed case: in the first step
                # some interior cell's u increment is exactly +-1 (the clamp),
                # and the rho = 0 cells keep their u through every step
                inner = (slice(1, -1),) * 3
                u0, u1, rho0 = f0.u[inner], first["u"][inner], f0.rho[inner]
                clamped = int(np.sum((u1 == u0 + 1.0) | (u1 == u0 - 1.0)))
                kept = int(np.sum(rho0 == 0.0))
                assert clamped > 0, "guard case: no increment reached the +-1 clamp"
                assert kept > 0, "guard case: no rho = 0 interior cell"
                assert np.array_equal(f.u[inner][rho0 == 0.0], f0.u[inner][rho0 == 0.0])
                run_rec["guard"] = {"u_increments_clamped_step1": clamped,
                                    "rho0_interior_cells_kept": kept}
            rec["runs"][integ] = run_rec
            if case["name"] in R.NPZ_FILES and integ != "rk4":
                for k in R.FIELDS:
                    npz.setdefault(case["name"], {})[f"{integ}_{k}"] = getattr(f, k).copy()
        doc["cases"][case["name"]] = rec
    # inputs the reference refuses: the status of each solver, one call
    doc["refusals"] = {}
    for which in R.REFUSALS:
        doc["refusals"][which] = {}
        for integ in R.INTEGRATORS:
            g, f, p = R.refusal_inputs(which)
            doc["refusals"][which][integ] = int(getattr(ref, IMPL[integ])(f.ptr, g.ptr,
                                                                          C.byref(p)))
    (OUT / "euler_rk2_cases.json").write_text(json.dumps(doc, indent=1) + "\n")
    for name, arrays in npz.items():
        np.savez_compressed(OUT / R.NPZ_FILES[name], **arrays)
    print(json.dumps({"cases": len(doc["cases"]), "work": str(work)}))


if __name__ == "__main__":
    sys.exit(main())
