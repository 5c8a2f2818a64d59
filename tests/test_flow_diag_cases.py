"""The flow diagnostics on the CPU: the numpy model of tests/flow_diag_cases.py
and the host twin cfd_flow_diagnostics (libcfd_host.so) against the reference
helpers' recorded results (tests/golden/flow_diag_cases.json, written by
tests/golden/make_flow_diag_golden.py), the host twin under ASan + UBSan, and
planted defects that the bars must see.

Bars. div_linf is a maximum: bitwise. A sum of N non-negative terms: the exact
sum (math.fsum, correctly rounded) and the reference's sequential sum each lie
within N 2^-53 relative of the exact value, so they differ by at most
2 N 2^-53 relative. tg3_compute_max_divergence divides by 2.0*dz where the
helper multiplies by the reciprocal: one rounding of dw_dz, at most 2^-53
|dw_dz|, carried through one more addition; held within
2^-50 max(|du_dx| + |dv_dy| + |dw_dz|) of div_linf.
"""
import ctypes as C
import json
import math
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from cfd_amd import _abi as A
from cfd_amd import api
from tests import flow_diag_cases as K

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"
HOST = ROOT / "cfd_amd" / "csrc" / "host"
CASES = K.cases()
IDS = [c[0] for c in CASES]


@pytest.fixture(scope="module")
def record():
    return json.loads((GOLDEN / K.JSON_FILE).read_text())


def ref_of(record, name):
    return {k: float.fromhex(v) for k, v in record["cases"][name]["ref"].items()}


def make_grid(shape, spacing=K.SPACING):
    """api.Grid of `shape` whose spacing arrays hold dx, dy, dz (the helpers
    and the diagnostics read element 0)."""
    nx, ny, nz = shape
    g = api.Grid(nx, ny, nz, 0.0, 1.0, 0.0, 1.0, 0.0, 1.0 if nz > 1 else 0.0)
    np.ctypeslib.as_array(g.c.dx, shape=(nx - 1,))[...] = spacing[0]
    np.ctypeslib.as_array(g.c.dy, shape=(ny - 1,))[...] = spacing[1]
    if nz > 1:
        np.ctypeslib.as_array(g.c.dz, shape=(nz - 1,))[...] = spacing[2]
    return g


def make_field(shape, arrays):
    f = api.FlowField(*shape)
    for k in K.FIELDS:
        getattr(f, k)[...] = arrays[k]
    return f


def test_record_is_of_these_inputs(record):
    assert [float.fromhex(x) for x in record["spacing"]] == list(K.SPACING)
    assert sorted(record["cases"]) == sorted(IDS)
    for name, shape, w0 in CASES:
        rec = record["cases"][name]
        assert tuple(rec["shape"]) == shape and rec["w0"] == w0
        assert shape[0] * shape[1] * shape[2] <= 42210  # the largest: 67x35x18
        arrays = K.inputs(shape, w0)
        assert {k: K.sha(arrays[k]) for k in K.FIELDS} == rec["inputs"], name
        assert np.all(arrays["rho"] > 0.0)  # every term of every sum is non-negative


def test_ctypes_mirror_matches_the_c_layout():
    assert C.sizeof(A.FlowDiag) == 64
    assert A.FlowDiag.div_cells.offset == 24 and A.FlowDiag.ke.offset == 40
    assert (A.HIP_DIAG_DIVERGENCE, A.HIP_DIAG_ENERGY) == (1, 2)


@pytest.mark.parametrize("name,shape,w0", CASES, ids=IDS)
def test_model_against_reference(record, name, shape, w0):
    ref = ref_of(record, name)
    m = K.model(shape, K.inputs(shape, w0))
    n_int = K.interior_cells(shape)
    assert m["div_cells"] == n_int and m["div_nan_cells"] == 0
    assert m["div_linf"].hex() == ref["test_compute_divergence_linf_3d"].hex()
    # sqrt is monotone and correctly rounded: 2 N u on the sum is at most N u + u on the root
    want_l2 = ref["test_compute_divergence_l2_3d"]
    assert abs(m["div_l2"] - want_l2) <= (n_int + 2) * K.U * want_l2
    assert K.sum_close(ref["test_compute_kinetic_energy_3d"], m["ke"], n_int, 2 * n_int)
    if shape[2] > 1:
        assert K.sum_close(ref["tg3_compute_kinetic_energy"], m["ke"], n_int, 2 * n_int)
        assert abs(ref["tg3_compute_max_divergence"] - m["div_linf"]) <= \
            2.0 ** -50 * m["div_abs_parts"]
    else:
        # 2-D helpers: no w in their expressions, so only the w = 0 inputs have their terms
        if w0:
            assert K.sum_close(ref["test_compute_kinetic_energy"], m["ke_rho"], n_int, 2 * n_int)
            assert K.sum_close(ref["test_compute_kinetic_energy_simple"], m["ke"], n_int,
                               2 * n_int)
            n_all = shape[0] * shape[1]
            assert K.sum_close(ref["compute_kinetic_energy"], m["ke_rho_cells"], n_all, 2 * n_all)
        else:
            assert not K.sum_close(ref["test_compute_kinetic_energy_simple"], m["ke"], n_int,
                                   2 * n_int)


@pytest.mark.parametrize("name,shape,w0", CASES, ids=IDS)
def test_host_twin_is_bitwise_the_reference(record, name, shape, w0):
    ref = ref_of(record, name)
    arrays = K.inputs(shape, w0)
    f, g = make_field(shape, arrays), make_grid(shape)
    d = api.flow_diagnostics(f, g, K.RHO0, 3)
    m = K.model(shape, arrays)
    n_int = K.interior_cells(shape)
    assert d.div_cells == n_int and d.div_nan_cells == 0
    assert d.div_linf.hex() == ref["test_compute_divergence_linf_3d"].hex()
    assert d.div_l2.hex() == ref["test_compute_divergence_l2_3d"].hex()
    assert d.div_l2.hex() == math.sqrt(d.div_sumsq / n_int).hex()
    assert K.sum_close(d.div_sumsq, m["div_sumsq"], n_int, n_int + 1)
    assert d.ke.hex() == ref["test_compute_kinetic_energy_3d"].hex()
    assert K.sum_close(d.ke_rho, m["ke_rho"], n_int, n_int + 1)
    assert K.sum_close(d.ke_rho_cells, m["ke_rho_cells"], m["n"]["ke_rho_cells"],
                       m["n"]["ke_rho_cells"] + 1)
    if shape[2] > 1:
        assert d.ke.hex() == ref["tg3_compute_kinetic_energy"].hex()
    elif w0:
        assert d.ke_rho.hex() == ref["test_compute_kinetic_energy"].hex()
        assert d.ke.hex() == ref["test_compute_kinetic_energy_simple"].hex()
        assert d.ke_rho_cells.hex() == ref["compute_kinetic_energy"].hex()
    # what = 1 and 2: the same numbers, the other half zero
    d1 = api.flow_diagnostics(f, g, K.RHO0, A.HIP_DIAG_DIVERGENCE)
    d2 = api.flow_diagnostics(f, g, K.RHO0, A.HIP_DIAG_ENERGY)
    assert (d1.div_linf, d1.div_sumsq, d1.div_l2, d1.div_cells) == \
        (d.div_linf, d.div_sumsq, d.div_l2, d.div_cells)
    assert (d1.ke, d1.ke_rho, d1.ke_rho_cells) == (0.0, 0.0, 0.0)
    assert (d2.ke, d2.ke_rho, d2.ke_rho_cells) == (d.ke, d.ke_rho, d.ke_rho_cells)
    assert (d2.div_linf, d2.div_sumsq, d2.div_l2, d2.div_cells, d2.div_nan_cells) == \
        (0.0, 0.0, 0.0, 0, 0)


def test_host_twin_refusals():
    shape = (5, 4, 3)
    f, g = make_field(shape, K.inputs(shape)), make_grid(shape)
    lib = api._native.host()
    d = A.FlowDiag()
    for what in (0, 4, -1):
        assert lib.cfd_flow_diagnostics(f.ptr, g.ptr, 1.0, what, C.byref(d)) == \
            A.CFD_ERROR_INVALID
    assert lib.cfd_flow_diagnostics(None, g.ptr, 1.0, 3, C.byref(d)) == A.CFD_ERROR_INVALID
    assert lib.cfd_flow_diagnostics(f.ptr, None, 1.0, 3, C.byref(d)) == A.CFD_ERROR_INVALID
    assert lib.cfd_flow_diagnostics(f.ptr, g.ptr, 1.0, 3, None) == A.CFD_ERROR_INVALID
    g2 = make_grid((5, 4, 4))
    assert lib.cfd_flow_diagnostics(f.ptr, g2.ptr, 1.0, 3, C.byref(d)) == A.CFD_ERROR_INVALID


# what each planted defect must move, and where it can
def _applies(bug, shape):
    nx, ny, nz = shape
    three = nz > 1
    if bug in ("no_dwdz", "dz_for_2dz", "k_lo", "k_hi"):
        return three
    if bug == "no_2d_dz_rule":
        return not three
    return True


_MOVES = {"dvdy_x_stride": ("div_sumsq",), "no_dwdz": ("div_sumsq",), "dz_for_2dz": ("div_sumsq",),
          "ke_all_cells": ("ke", "ke_rho"), "rho0_for_rho": ("ke_rho",),
          "no_2d_dz_rule": ("ke", "ke_rho")}


@pytest.mark.parametrize("shape", K.SHAPES, ids=[K.name_of(s) for s in K.SHAPES])
def test_planted_bugs_move_the_numbers(shape):
    arrays = K.inputs(shape)
    good = K.model(shape, arrays)
    for bug in K.BUGS:
        if not _applies(bug, shape):
            continue
        bad = K.model(shape, arrays, bug=bug)
        keys = _MOVES.get(bug, ("div_sumsq", "ke", "ke_rho"))  # the bounds defects: every interior sum
        for k in keys:
            n = max(good["n"][k], bad["n"][k])
            assert not K.sum_close(bad[k], good[k], n, 2 * n + 2), (bug, k, bad[k], good[k])
        if bug[1:] in ("_lo", "_hi"):
            assert bad["div_cells"] != good["div_cells"], bug


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not present")
def test_host_twin_under_asan_ubsan(tmp_path):
    """cfd_flow_diagnostics in a stand-alone program (tests/native/
    flow_diag_check.c) built with ASan + UBSan, on the whole shape table."""
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(["gcc", *flags, str(probe), "-o", str(tmp_path / "probe")],
                       capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("the sanitizer runtime cannot be linked: " + r.stderr[-200:])
    exe = tmp_path / "flow_diag_check"
    cmd = ["gcc", "-std=c11", "-g", "-O1", "-fno-omit-frame-pointer", "-ffp-contract=off", *flags,
           "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}",
           str(ROOT / "tests" / "native" / "flow_diag_check.c"), str(HOST / "flow_diag_host.c"),
           "-o", str(exe), "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    args = [str(v) for s in K.SHAPES for v in s]
    out = subprocess.run([str(exe), *args], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout + out.stderr)[-4000:]
