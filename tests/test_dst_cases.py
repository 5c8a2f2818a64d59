"""The direct sine-transform pressure solve on the CPU: the numpy float64 model
of tests/dst_cases.py (the algorithm of cfd_amd/csrc/hip/transform_solve.hpp) against
the oracle's CG run to 1e-13, on every shape of the table, with the default
Neumann apply_bc and with a Dirichlet hook; the model's stats rules; planted
bugs; the public surface; the host table builder under ASan + UBSan.

The largest deviation printed by test_model_matches_tight_cg, times 100, is
dst_cases.DST_BAR, the bar of the device tests (tests/test_gpu_dst.py).
"""
import ctypes as C
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from cfd_amd import _abi as A
from cfd_amd import _native, api
from oracle import oracle
from tests import dst_cases as K

ROOT = Path(__file__).resolve().parents[1]
HOST = ROOT / "cfd_amd" / "csrc" / "host"

BCS = {"neumann": None, "dirichlet": K.dirichlet_bc}


@pytest.mark.parametrize("bc", list(BCS))
def test_model_matches_tight_cg(bc):
    worst = 0.0
    for shape in K.SHAPE_LIST:
        rc, status, its, ref = K.tight_cg(shape, bc)
        assert (rc, status) == (A.CFD_SUCCESS, A.POISSON_CONVERGED), (shape, rc, status, its)
        rhs, x0 = K.inputs(shape)
        m = K.model_solve(x0, rhs, K.spacing(shape), bc=BCS[bc])
        dev = K.rel_dev(m.x, ref)
        worst = max(worst, dev)
        print(f"DST model {bc} {K.sid(shape)}: deviation {dev:.3e} (CG iterations {its})")
        assert dev <= K.DST_BAR, (shape, dev)
        # the boundary: what the end BC gives from the model's own interior
        # (Dirichlet: the oracle's values)
        again = m.x.copy()
        (BCS[bc] or oracle.poisson_apply_bc)(again)
        assert np.array_equal(again, m.x), shape
        if bc == "dirichlet":
            sh = K.shell_mask(ref.shape)
            assert np.array_equal(m.x[sh], ref[sh]), shape
    print(f"DST model {bc}: largest deviation {worst:.3e}, x 100 = {100 * worst:.3e}")


@pytest.mark.parametrize("shape", K.SHAPE_LIST, ids=K.sid)
def test_model_stats(shape):
    rhs, x0 = K.inputs(shape)
    d = K.spacing(shape)
    m = K.model_solve(x0, rhs, d)
    assert (m.rc, m.status, m.iterations) == (A.CFD_SUCCESS, A.POISSON_CONVERGED, 1)
    # the initial residual is CG's
    want = np.array(x0)
    st = oracle.cg_solve(want, np.ascontiguousarray(rhs), *d,
                         oracle.poisson_params(max_iterations=0))[1]
    assert abs(m.initial_residual - st.initial_residual) <= 1e-12 * st.initial_residual
    assert m.final_residual < 1e-6 * m.initial_residual
    # an unreachable tolerance: MAX_ITER and the CG return code, x the same
    u = K.model_solve(x0, rhs, d, tolerance=1e-30, absolute_tolerance=1e-300)
    assert (u.rc, u.status, u.iterations) == (A.CFD_ERROR_MAX_ITER, A.POISSON_MAX_ITER, 1)
    assert np.array_equal(u.x, m.x) and u.final_residual == m.final_residual
    # zero right-hand side from a constant field: the early exit, no iteration
    z = K.model_solve(np.full_like(x0, 0.25), np.zeros_like(rhs), d)
    assert (z.rc, z.status, z.iterations) == (A.CFD_SUCCESS, A.POISSON_CONVERGED, 0)
    assert z.final_residual == z.initial_residual < 1e-10
    assert np.array_equal(z.x, np.full_like(x0, 0.25))


@pytest.mark.parametrize("shape", K.SHAPE_LIST, ids=K.sid)
def test_planted_bugs_show(shape):
    """Under the Dirichlet hook: with the Neumann shell of a grid of one
    interior cell per axis every face holds the same value, and a 1/h^2 taken
    from the other axis cancels in b."""
    rhs, x0 = K.inputs(shape)
    d = K.spacing(shape)
    good = K.model_solve(x0, rhs, d, bc=K.dirichlet_bc).x
    for what, kw in (("boundary sign", dict(bnd_sign=-1.0)), ("1/h^2 axis", dict(swap_h=True)),
                     ("normalisation", dict(norm_scale=0.5))):
        bad = K.model_solve(x0, rhs, d, bc=K.dirichlet_bc, **kw).x
        assert K.rel_dev(bad, good) > K.DST_BAR, (what, shape)


def test_transform_model_is_an_involution():
    for shape in K.SHAPE_LIST:
        _, x0 = K.inputs(shape)
        for axis in range(3 if shape[2] > 1 else 2):
            n = shape[axis] - 2
            back = K.transform(K.transform(np.array(x0), axis), axis)
            inn = K.interior(x0.shape)
            assert np.allclose(back[inn], (n + 1) / 2.0 * x0[inn], rtol=0, atol=1e-12 * (n + 1))
            sh = K.shell_mask(x0.shape)
            assert np.array_equal(back[sh], x0[sh])


def test_surface():
    """The method value, the entry point and the bindings; ABI version and the
    timer count stay."""
    hdr = (ROOT / "include" / "cfd_hip" / "projection_hip.h").read_text()
    assert A.HIP_POISSON_DST == 4 and "HIP_POISSON_DST = 4" in hdr
    assert "cfd_status_t hip_proj_dst_transform(hip_proj_ctx_t* ctx, double* field_host," in hdr
    assert "#define HIP_PROJ_ABI_VERSION 4" in hdr and "HIP_KT_COUNT = 21" in hdr
    hip = _native.hip()
    assert hip.hip_proj_abi_version() == 4 and A.HIP_KT_COUNT == 21
    assert hip.hip_proj_dst_transform.argtypes == [C.c_void_p, A.c_double_p, C.c_int]
    assert callable(api.HipProjection.dst_transform)
    assert hip.hip_proj_dst_transform(None, None, 0) == A.CFD_ERROR_INVALID


def test_shape_table_covers_the_tile_edges():
    n = sorted({v - 2 for s in K.SHAPE_LIST for v in (s if s[2] > 1 else s[:2])})
    assert 1 in n and any(v < 4 for v in n) and any(4 <= v < 16 for v in n)
    assert {1, 15, 0, 3} <= {v % 16 for v in n if v > 4}
    assert any(v > 64 for v in n) and any(v > 256 for v in n) and 32 in n
    assert all(d[0] != d[1] and (s[2] == 1 or d[1] != d[2])
               for s in K.SHAPE_LIST for d in [K.spacing(s)])


SAN_DRIVER = r"""
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include "dst_tables.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main(void) {
    const size_t ns[] = {1, 2, 3, 15, 16, 17, 63, 64, 65, 259};
    for (size_t q = 0; q < sizeof ns / sizeof ns[0]; q++) {
        const size_t n = ns[q], np = dst_table_pitch(n);
        CHECK(np >= n && np % 64 == 0 && np < n + 64);
        /* heap blocks of exactly the documented sizes */
        double* S = (double*)malloc(np * np * sizeof(double));
        double* e = (double*)malloc(n * sizeof(double));
        CHECK(S && e);
        dst_fill_sine_table(n, S);
        dst_fill_eigenvalues(n, e);
        for (size_t a = 0; a < np; a++)
            for (size_t b = 0; b < np; b++) {
                const double v = S[a * np + b];
                if (a >= n || b >= n) CHECK(v == 0.0);
                else {
                    CHECK(v == S[b * np + a]);
                    CHECK(fabs(v - sin(M_PI * (double)((a + 1) * (b + 1) % (2 * (n + 1))) /
                                       (double)(n + 1))) < 1e-14);
                }
            }
        /* S S = (n + 1) / 2 I, first row */
        for (size_t b = 0; b < n; b++) {
            double s = 0.0;
            for (size_t k = 0; k < n; k++) s += S[k] * S[k * np + b];
            CHECK(fabs(s - (b == 0 ? (double)(n + 1) / 2.0 : 0.0)) < 1e-12 * (double)(n + 1));
        }
        for (size_t a = 0; a < n; a++) {
            CHECK(e[a] > 0.0 && e[a] < 4.0);
            if (a) CHECK(e[a] > e[a - 1]);
        }
        free(S);
        free(e);
    }
    printf("ok\n");
    return 0;
}
"""


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not present")
def test_table_builder_under_asan_ubsan(tmp_path):
    src = tmp_path / "dst_drv.c"
    src.write_text(SAN_DRIVER)
    exe = tmp_path / "dst_drv"
    cmd = ["gcc", "-std=gnu11", "-g", "-O1", "-fno-omit-frame-pointer",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", f"-I{HOST}",
           str(src), "-o", str(exe), "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout + out.stderr)[-4000:]
