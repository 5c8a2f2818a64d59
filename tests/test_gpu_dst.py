"""The direct sine-transform pressure solve on the device (HIP_POISSON_DST,
transform_solve.hpp: k_dst_x and k_dst_strided on the fp64 matrix cores) on the shape
table of tests/dst_cases.py.

- each transform pass alone (hip_proj_dst_transform) against the long-double
  product S X, to the derived bound (n + 2) 2^-53 sum_b |S_ab| |x_b| per element;
- the solve with all three bc_modes against the oracle's CG run to 1e-13, to
  dst_cases.DST_BAR, and its stats against the numpy model's;
- determinism, a CG solve on the same context unaffected;
- three projection steps with poisson_method = DST (step_device, and the
  plugin's `step` under CFD_HIP_POISSON=dst in a child process) against the
  oracle's step with its CG at the tight settings;
- the refusals.

The final residual of a direct solve is rounding noise (1e-16 .. 1e-14 of the
initial one), which two summation orders do not reproduce digit by digit: it
is compared with the model's to 1e-9 of the INITIAL residual, the initial
residual to 1e-9 of itself.

Measured on an MI355X: x within 5.6e-12 of the tight CG on every shape and
bc_mode (bar 5.6e-10), the initial residual within 2.1e-16, every transform
element within 0.37 of its bound, the step's u, v, w within 3.5e-14 and p
within 2.5e-13.
"""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from cfd_amd import _abi as A
from cfd_amd import _native, api
from oracle import oracle
from tests import dst_cases as K

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
DST = A.HIP_POISSON_DST
U = 2.0 ** -53
SHAPE_IDS = [K.sid(s) for s in K.SHAPE_LIST]


def _axes(shape):
    return range(3 if shape[2] > 1 else 2)


# ---------------------------------------------------------------------------
# the transform alone
# ---------------------------------------------------------------------------
def _ld_product(M, a, axis):
    """M applied along `axis` (0 x, 1 y, 2 z) of the interior of a, in long double."""
    inn = K.interior(a.shape)
    ax = 2 - axis
    v = a[inn].astype(np.longdouble)
    return np.moveaxis(np.tensordot(M, v, axes=([1], [ax])), 0, ax)


@pytest.mark.parametrize("shape", K.SHAPE_LIST, ids=SHAPE_IDS)
def test_transform_alone(hip_lib, shape):
    _, x0 = K.inputs(shape)
    inn = K.interior(x0.shape)
    sh = K.shell_mask(x0.shape)
    ctx = api.HipProjection(*shape)
    try:
        first = {}
        for axis in _axes(shape):
            n = shape[axis] - 2
            S = K.sine_matrix(n).astype(np.longdouble)  # the table's doubles
            y = np.array(x0)
            assert ctx.dst_transform(y, axis) == A.CFD_SUCCESS, _native.last_error()
            first[axis] = y
            want = _ld_product(K.sine_matrix_ld(n), x0, axis)
            absx = np.abs(np.array(x0))
            absx[sh] = 0.0
            bound = (n + 2) * U * _ld_product(np.abs(S), absx, axis)
            err = np.abs(y[inn].astype(np.longdouble) - want)
            worst = float(np.max(err / np.maximum(bound, np.longdouble(1e-300))))
            print(f"DST transform {K.sid(shape)} axis {axis}: error / bound {worst:.3f}")
            assert np.all(err <= bound), (axis, worst)
            assert np.array_equal(y[sh], x0[sh]), f"axis {axis}: boundary cells written"
            # twice: (n + 1) / 2 X. The first pass's error goes through |S| once
            # more and the second adds its own on |S| |y| <= |S| |S| |x|
            z = y.copy()
            assert ctx.dst_transform(z, axis) == A.CFD_SUCCESS
            absy = np.zeros_like(absx)
            absy[inn] = _ld_product(np.abs(S), absx, axis).astype(np.float64)
            bound2 = 2 * (n + 2) * U * _ld_product(np.abs(S), absy, axis) * (1 + 1e-12)
            err2 = np.abs(z[inn].astype(np.longdouble) -
                          np.longdouble(n + 1) / 2 * x0[inn].astype(np.longdouble))
            assert np.all(err2 <= bound2), (axis, float(np.max(err2 / bound2)))
            assert np.array_equal(z[sh], x0[sh])
        # a NaN-filled field through every work field of the context, then the
        # same transforms: no pass may read a cell it does not own
        nan = np.full(x0.shape, np.nan)
        ctx.poisson_solve(DST, nan.copy(), nan.copy(), *K.spacing(shape))
        for axis in _axes(shape):
            junk = nan.copy()
            ctx.dst_transform(junk, axis)
        for axis in _axes(shape):
            y = np.array(x0)
            assert ctx.dst_transform(y, axis) == A.CFD_SUCCESS
            assert np.array_equal(y, first[axis]), f"axis {axis}: differs after NaN fields"
    finally:
        ctx.close()


# ---------------------------------------------------------------------------
# the solve
# ---------------------------------------------------------------------------
def _mode_inputs(shape, mode):
    """(x0, bc_values, oracle bc name, model bc) of a bc_mode."""
    _, x0 = K.inputs(shape)
    x0 = np.array(x0)
    if mode == A.HIP_POISSON_BC_NEUMANN:
        return x0, None, "neumann", None
    if mode == A.HIP_POISSON_BC_NONE:
        return x0, None, "keep", (lambda a: None)
    # FIXED: an apply_bc that writes x-independent values. The solve's start
    # BC is CG's (which leaves the caller's boundary in place), so the caller
    # hands x over with those values on its shell
    K.dirichlet_bc(x0)
    return x0, x0.copy(), "dirichlet", K.dirichlet_bc


MODES = [A.HIP_POISSON_BC_NEUMANN, A.HIP_POISSON_BC_NONE, A.HIP_POISSON_BC_FIXED]


@pytest.mark.parametrize("shape", K.SHAPE_LIST, ids=SHAPE_IDS)
def test_solve(hip_lib, shape):
    rhs, _ = K.inputs(shape)
    d = K.spacing(shape)
    ctx = api.HipProjection(*shape)
    fails = []
    try:
        for mode in MODES:
            x0, vals, oname, mbc = _mode_inputs(shape, mode)
            rc, status, _, ref = K.tight_cg(shape, oname)
            assert (rc, status) == (A.CFD_SUCCESS, A.POISSON_CONVERGED)
            m = K.model_solve(x0, rhs, d, bc=mbc)
            x = x0.copy()
            # max_iterations, check_interval and omega are ignored
            prm = oracle.poisson_params(max_iterations=0, check_interval=7, omega=1.9)
            s, st = ctx.poisson_solve(DST, x, rhs, *d, prm, bc_mode=mode, bc_values=vals)
            dev = K.rel_dev(x, ref)
            r0 = abs(st.initial_residual - m.initial_residual) / m.initial_residual
            r1 = abs(st.final_residual - m.final_residual) / m.initial_residual
            print(f"DST solve {K.sid(shape)} bc {mode}: x {dev:.3e} res0 {r0:.3e} "
                  f"res {st.final_residual:.3e} (model {m.final_residual:.3e}) "
                  f"{st.elapsed_time_ms:.3f} ms")
            try:
                assert (s, st.status, st.iterations) == (m.rc, m.status, m.iterations) == \
                    (A.CFD_SUCCESS, A.POISSON_CONVERGED, 1), (s, st.status, st.iterations)
                assert np.isfinite(x).all()
                assert dev <= K.DST_BAR, f"x off by {dev:.3e}"
                assert r0 <= 1e-9 and r1 <= 1e-9, (r0, r1)
                assert st.elapsed_time_ms > 0.0
                sh = K.shell_mask(x.shape)
                if mode == A.HIP_POISSON_BC_NEUMANN:
                    again = x.copy()
                    oracle.poisson_apply_bc(again)
                    assert np.array_equal(again, x), "the end BC's shell"
                else:
                    assert np.array_equal(x[sh], x0[sh]), "boundary cells written"
                ps = ctx.poisson_stats()
                assert (ps.status, ps.iterations, ps.initial_residual, ps.final_residual) == \
                    (st.status, st.iterations, st.initial_residual, st.final_residual)
            except AssertionError as e:
                fails.append(f"bc {mode}: {e}")
    finally:
        ctx.close()
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("shape", [(3, 3, 3), (23, 19, 1), (20, 14, 11)], ids=K.sid)
def test_solve_exits(hip_lib, shape):
    rhs, x0 = K.inputs(shape)
    d = K.spacing(shape)
    ctx = api.HipProjection(*shape)
    try:
        good = np.array(x0)
        s, st = ctx.poisson_solve(DST, good, rhs, *d)
        assert s == A.CFD_SUCCESS
        # an unreachable tolerance: MAX_ITER, CG's return code, the same x
        x = np.array(x0)
        prm = oracle.poisson_params(tolerance=1e-30, absolute_tolerance=1e-300)
        s, u = ctx.poisson_solve(DST, x, rhs, *d, prm)
        assert (s, u.status, u.iterations) == (A.CFD_ERROR_MAX_ITER, A.POISSON_MAX_ITER, 1)
        assert np.array_equal(x, good) and u.final_residual == st.final_residual
        # nothing to solve: converged at the start, no iteration, no end BC
        x = np.full(x0.shape, 0.25)
        s, z = ctx.poisson_solve(DST, x, np.zeros_like(x), *d)
        assert (s, z.status, z.iterations) == (A.CFD_SUCCESS, A.POISSON_CONVERGED, 0)
        assert z.initial_residual == z.final_residual < 1e-10
        assert np.array_equal(x, np.full(x0.shape, 0.25))
    finally:
        ctx.close()


def test_determinism_and_cg_unaffected(hip_lib, monkeypatch):
    monkeypatch.setenv("CFD_HIP_CG_SMALL", "0")  # CG on the sweeps: the whole p ring
    shape = (67, 35, 18)
    rhs, x0 = K.inputs(shape)
    d = K.spacing(shape)
    prm = oracle.poisson_params(max_iterations=40)

    def solve(ctx, method):
        x = np.array(x0)
        s, st = ctx.poisson_solve(method, x, rhs, *d, prm)
        return s, st.iterations, st.initial_residual, st.final_residual, x

    ctx = api.HipProjection(*shape)
    try:
        fresh_cg = solve(ctx, A.HIP_POISSON_CG)
    finally:
        ctx.close()
    ctx = api.HipProjection(*shape)
    try:
        a = solve(ctx, DST)
        cg = solve(ctx, A.HIP_POISSON_CG)
        b = solve(ctx, DST)
    finally:
        ctx.close()
    assert a[:4] == b[:4] and np.array_equal(a[4], b[4])
    assert cg[:4] == fresh_cg[:4] and np.array_equal(cg[4], fresh_cg[4])


# ---------------------------------------------------------------------------
# the projection step
# ---------------------------------------------------------------------------
STEP_SHAPES = [(20, 14, 11), (67, 35, 1)]
STEP_DT, STEP_NU, STEPS = 1e-4, 0.01, 3


def _step_fields(shape):
    nx, ny, nz = shape
    rng = np.random.default_rng(77 + nx + ny + nz)
    f = {k: 0.1 * rng.standard_normal((nz, ny, nx)) for k in ("u", "v", "w", "p")}
    if nz == 1:
        f["w"][...] = 0.0
    return f


def _grid_field(shape, fields):
    nx, ny, nz = shape
    g = api.Grid(nx, ny, nz, 0.0, K.BOX[0], 0.0, K.BOX[1], 0.0, K.BOX[2] if nz > 1 else 0.0)
    f = api.FlowField(nx, ny, nz)
    for k, v in fields.items():
        getattr(f, k)[...] = v
    f.rho[...] = 1.0
    f.T[...] = 300.0
    return g, f, api.validation_params(STEP_DT, STEP_NU)


_STEP_REF = {}


def _step_reference(shape):
    """Three oracle steps with its CG at the tight settings, once per shape."""
    if shape not in _STEP_REF:
        g, f, prm = _grid_field(shape, _step_fields(shape))
        oracle.set_projection_poisson_params(oracle.poisson_params(**K.TIGHT))
        try:
            for _ in range(STEPS):
                s, _, _ = oracle.projection_step(f, g, prm)
                assert s == A.CFD_SUCCESS
                assert oracle.last_poisson_stats().status == A.POISSON_CONVERGED
        finally:
            oracle.set_projection_poisson_params(None)
        _STEP_REF[shape] = {k: np.array(getattr(f, k)) for k in ("u", "v", "w", "p")}
    return _STEP_REF[shape]


def _check_fields(got, ref, what):
    fails = []
    for k in ("u", "v", "w", "p"):
        scale = float(np.max(np.abs(ref[k])))
        dev = float(np.max(np.abs(got[k] - ref[k]))) / scale if scale > 0.0 else \
            float(np.max(np.abs(got[k])))
        print(f"DST step {what} {k}: {dev:.3e}")
        if not dev <= K.DST_BAR:
            fails.append(f"{what} {k}: {dev:.3e}")
    assert not fails, fails


@pytest.mark.parametrize("shape", STEP_SHAPES, ids=K.sid)
def test_step_device(hip_lib, shape):
    ref = _step_reference(shape)
    g, f, prm = _grid_field(shape, _step_fields(shape))
    ctx = api.HipProjection(*shape, poisson_method=DST)
    try:
        ctx.upload(f)
        for _ in range(STEPS):
            assert ctx.step_device(g, prm) == A.CFD_SUCCESS, _native.last_error()
            st = ctx.poisson_stats()
            assert (st.status, st.iterations) == (A.POISSON_CONVERGED, 1)
            assert st.final_residual < 1e-9 * st.initial_residual
        ctx.download(f)
    finally:
        ctx.close()
    _check_fields({k: getattr(f, k) for k in ref}, ref, f"step_device {K.sid(shape)}")


def test_step_fail_fatal_keeps_its_meaning(hip_lib):
    shape = STEP_SHAPES[0]
    for fatal, want in ((1, A.CFD_ERROR_MAX_ITER), (0, A.CFD_SUCCESS)):
        g, f, prm = _grid_field(shape, _step_fields(shape))
        ctx = api.HipProjection(*shape, poisson_method=DST, poisson_tolerance=1e-30,
                                poisson_abs_tolerance=1e-300, poisson_fail_fatal=fatal)
        try:
            ctx.upload(f)
            assert ctx.step_device(g, prm) == want
            assert ctx.poisson_stats().status == A.POISSON_MAX_ITER
        finally:
            ctx.close()


@pytest.mark.parametrize("shape", STEP_SHAPES, ids=K.sid)
def test_plugin_step_in_a_child(hip_lib, shape, tmp_path):
    ref = _step_reference(shape)
    src, dst = tmp_path / "in.npz", tmp_path / "out.npz"
    nz = shape[2]
    np.savez(src, shape=np.array(shape), box=np.array([K.BOX[0], K.BOX[1],
                                                       K.BOX[2] if nz > 1 else 0.0]),
             dt=STEP_DT, nu=STEP_NU, steps=STEPS, **_step_fields(shape))
    env = dict(os.environ, CFD_HIP_POISSON="dst")
    env["PYTHONPATH"] = str(ROOT) + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "dst_plugin_worker.py"), str(src),
                        str(dst)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DST_PLUGIN_OK" in r.stdout, (r.stdout + r.stderr)[-4000:]
    got = np.load(dst)
    _check_fields(got, ref, f"plugin {K.sid(shape)}")
    # ... and it was the direct solve: the CG path's p differs from the tight
    # reference by its own 1e-6 tolerance
    if shape == STEP_SHAPES[0]:
        env.pop("CFD_HIP_POISSON")
        r = subprocess.run([sys.executable, str(ROOT / "tests" / "dst_plugin_worker.py"),
                            str(src), str(dst)], cwd=ROOT, env=env, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
        cg = np.load(dst)
        scale = float(np.max(np.abs(ref["p"])))
        assert float(np.max(np.abs(cg["p"] - ref["p"]))) / scale > K.DST_BAR


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------
def test_refusals(hip_lib):
    shape = (20, 14, 11)
    rhs, x0 = K.inputs(shape)
    d = K.spacing(shape)
    sentinel = np.array(x0) + 3.0
    ctx = api.HipProjection(*shape)
    try:
        good = np.array(x0)
        assert ctx.poisson_solve(DST, good, rhs, *d)[0] == A.CFD_SUCCESS
        p_before = ctx.get_field(A.HIP_FIELD_P)
        stats_before = ctx.poisson_stats()
        # a preconditioner
        x = sentinel.copy()
        prm = oracle.poisson_params(preconditioner=1)  # POISSON_PRECOND_JACOBI
        s, _ = ctx.poisson_solve(DST, x, rhs, *d, prm)
        assert s == A.CFD_ERROR_UNSUPPORTED and "preconditioner" in _native.last_error()
        assert np.array_equal(x, sentinel)
        # an unknown axis
        for axis in (-1, 3):
            y = sentinel.copy()
            assert ctx.dst_transform(y, axis) == A.CFD_ERROR_INVALID
            assert "axis" in _native.last_error() and np.array_equal(y, sentinel)
        assert np.array_equal(ctx.get_field(A.HIP_FIELD_P), p_before)
        assert ctx.poisson_stats().final_residual == stats_before.final_residual
        # the context still solves, to the same bits
        x = np.array(x0)
        assert ctx.poisson_solve(DST, x, rhs, *d)[0] == A.CFD_SUCCESS
        assert np.array_equal(x, good)
    finally:
        ctx.close()
    # axis 2 on a 2-D context
    shape2 = (23, 19, 1)
    ctx = api.HipProjection(*shape2)
    try:
        y = np.array(K.inputs(shape2)[1]) + 3.0
        keep = y.copy()
        assert ctx.dst_transform(y, 2) == A.CFD_ERROR_INVALID
        assert "2-D" in _native.last_error() and np.array_equal(y, keep)
        assert ctx.dst_transform(y, 1) == A.CFD_SUCCESS
    finally:
        ctx.close()


def test_z_slab_contexts_are_refused(hip_lib):
    """Refused before anything is uploaded or launched: one rank's calls
    return at once, without its neighbour taking part."""
    shape = (20, 14, 11)
    nx, ny, nz = shape
    d = K.spacing(shape)
    group = api.LocalGroup(2)
    ctxs = []
    try:
        ctxs = [api.HipProjection(nx, ny, nz, comm=group.comm(r, 0), poisson_method=DST)
                for r in range(2)]
        c = ctxs[0]
        rng = np.random.default_rng(5)
        local = rng.standard_normal(c.shape)
        c.set_field(A.HIP_FIELD_P, local)
        x = local + 3.0
        keep = x.copy()
        s, _ = c.poisson_solve(DST, x, np.zeros(c.shape), *d)
        assert s == A.CFD_ERROR_UNSUPPORTED and "Z-slab" in _native.last_error()
        assert np.array_equal(x, keep)
        assert c.dst_transform(x, 0) == A.CFD_ERROR_UNSUPPORTED
        assert "Z-slab" in _native.last_error() and np.array_equal(x, keep)
        g = api.Grid(nx, ny, nz, 0.0, K.BOX[0], 0.0, K.BOX[1], 0.0, K.BOX[2])
        prm = api.validation_params(STEP_DT, STEP_NU)
        assert c.step_device(g, prm) == A.CFD_ERROR_UNSUPPORTED
        assert "Z-slab" in _native.last_error()
        assert np.array_equal(c.get_field(A.HIP_FIELD_P), local)
    finally:
        for c in ctxs:
            c.close()
        group.close()
