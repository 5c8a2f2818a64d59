#!/usr/bin/env python3
"""Writes tests/golden/flow_diag_cases.json from the reference's own
validation helpers:

  test_compute_divergence_linf_3d, test_compute_divergence_l2_3d,
  test_compute_kinetic_energy_3d, test_compute_kinetic_energy,
  test_compute_kinetic_energy_simple   tests/solvers/navier_stokes/test_solver_helpers.h
  tg3_compute_kinetic_energy, tg3_compute_max_divergence
                                       tests/validation/taylor_green_3d_reference.h
  compute_kinetic_energy               tests/validation/lid_driven_cavity_common.h

The reference checkout (CFD_REFERENCE_DIR, else `reference` beside this
repository) is copied to a work directory and built there unmodified, CPU only,
with -ffp-contract=off (make_rk_golden.build_reference). The small driver of
this repository, tests/native/flow_diag_ref_driver.c, is compiled against that
copy's include directories and the three headers above, with the same flag and
an empty unity.h stand-in in the work directory (the two validation headers
include it and use none of its macros outside functions the driver never
calls), linked against the reference build, and run on the seeded inputs of
tests/flow_diag_cases.py. Nothing built from the reference and none of its text
is written into this repository: only the numbers its helpers return, as hex
floats, with the sha256 of each input, the shape and the spacings.

usage: make_flow_diag_golden.py [--work DIR] [--jobs N] [--reuse]
"""
import argparse
import importlib.util
import json
import os
import struct
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
OUT = Path(__file__).resolve().parent


def _rk():
    spec = importlib.util.spec_from_file_location("make_rk_golden", OUT / "make_rk_golden.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build_driver(work: Path, ref_so: Path) -> Path:
    src = work / "src"
    stub = work / "unity_stub"
    stub.mkdir(exist_ok=True)
    (stub / "unity.h").write_text("/* stand-in: the driver calls no Unity macro */\n")
    exe = work / "flow_diag_ref_driver"
    cmd = ["gcc", "-std=gnu11", "-O2", "-ffp-contract=off", "-fno-fast-math",
           f"-I{src / 'lib' / 'include'}", f"-I{work / 'build' / 'lib' / 'include'}",
           f"-I{src / 'tests' / 'solvers' / 'navier_stokes'}",
           f"-I{src / 'tests' / 'validation'}", f"-I{stub}",
           str(ROOT / "tests" / "native" / "flow_diag_ref_driver.c"), "-o", str(exe),
           str(ref_so), f"-Wl,-rpath,{ref_so.parent}", "-fopenmp", "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit("make_flow_diag_golden: driver build failed:\n" + r.stderr[-4000:])
    return exe


def run_driver(exe: Path, work: Path, shape, spacing, arrays) -> dict:
    path = work / "flow_diag_input.bin"
    with open(path, "wb") as fp:
        fp.write(struct.pack("<3Q3d", *shape, *spacing))
        for k in ("u", "v", "w", "rho"):
            fp.write(np.ascontiguousarray(arrays[k], dtype="<f8").tobytes())
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True,
                       env=dict(os.environ, OMP_NUM_THREADS="1"))
    if r.returncode != 0:
        raise SystemExit(f"make_flow_diag_golden: driver failed on {shape}: {r.stderr[-2000:]}")
    out = {}
    for line in r.stdout.split("\n"):
        if line.strip():
            name, val = line.split()
            out[name] = float.fromhex(val).hex()  # %a text -> Python's canonical form
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--work", default="/tmp/cfd_flow_diag_golden")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--reuse", action="store_true",
                    help="keep a reference build already in the work directory")
    a = ap.parse_args()
    work = Path(a.work)
    work.mkdir(parents=True, exist_ok=True)
    rk = _rk()
    ref_so = work / "libcfd_reference.so"
    if not (a.reuse and ref_so.exists()):
        ref_so = rk.build_reference(work, a.jobs)
    exe = build_driver(work, ref_so)

    from tests import flow_diag_cases as K

    doc = {"reference": "shaia/CFD v0.3.0, validation helpers (test_solver_helpers.h, "
                        "taylor_green_3d_reference.h, lid_driven_cavity_common.h)",
           "build_flags": "-O2 -ffp-contract=off", "spacing": [x.hex() for x in K.SPACING],
           "cases": {}}
    for name, shape, w0 in K.cases():
        arrays = K.inputs(shape, w0)
        doc["cases"][name] = {"shape": list(shape), "w0": w0,
                              "inputs": {k: K.sha(arrays[k]) for k in K.FIELDS},
                              "ref": run_driver(exe, work, shape, K.SPACING, arrays)}
    (OUT / K.JSON_FILE).write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps({"cases": len(doc["cases"]), "work": str(work)}))


if __name__ == "__main__":
    sys.exit(main())
