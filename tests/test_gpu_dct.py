"""The direct cosine-transform pressure solve on the device (HIP_POISSON_DCT,
transform_solve.hpp: the passes k_dst_x and k_dst_strided with cosine tables, the
negating load and the cosine eigenvalue division) on the shape table of
tests/dct_cases.py.

- each transform pass alone (hip_proj_dct_transform), forward and inverse,
  against the long-double product, to the derived bound
  (n + 2) 2^-53 sum_b |T_ab| |x_b| per element;
- the solve on a compatible and an incompatible right-hand side against the
  oracle's RB-SOR run to 1e-15 and the numpy model, to dct_cases.DCT_BAR, both
  demeaned over the interior; its stats against the model's;
- determinism; CG, RB-SOR and DST solves on the same context unaffected;
- a projection step with poisson_method = DCT (step_device, and the plugin's
  `step` under CFD_HIP_POISSON=dct in a child process) against the oracle's
  step with its RB-SOR at 1e-12; the incompatible cavity step;
- the refusals.

The final residual of a direct solve on a compatible right-hand side is
rounding noise, which two summation orders do not reproduce digit by digit:
it is compared with the model's to 1e-9 of the INITIAL residual. The initial
residual is compared bit for bit.

Measured on an MI355X: demeaned x within 7.4e-16 of the model and 2.24e-11 of
the tight RB-SOR on every shape (bar 1.81e-8), every transform element within
0.41 of its bound, the step's p within 1.0e-10 of the oracle's and u, v, w
within 9.1e-13 (bound 2.2e-9 .. 4.4e-9), the cavity step's (dt / rho) grad p
within 1.1e-16 of the model's.

The refusals read the context's kernel timers as the launch log: with timing
enabled every timed launch counts, and a DCT solve that does run shows its
two residual launches there.
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
from tests import dct_cases as K

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
DCT = A.HIP_POISSON_DCT
U = 2.0 ** -53
SHAPE_IDS = [K.sid(s) for s in K.SHAPE_LIST]


def _axes(shape):
    return range(len(K.extents(shape)))


def _launches(ctx):
    """The launch log: timed launches per kernel timer since reset_timing."""
    return {k: n for k, (_, n) in ctx.timing().items() if n}


# ---------------------------------------------------------------------------
# one pass alone
# ---------------------------------------------------------------------------
def _ld_product(M, a, axis):
    """M applied along `axis` (0 x, 1 y, 2 z) of the interior of a, in long double."""
    inn = K.interior(a.shape)
    ax = 2 - axis
    return K.apply_along(M, a[inn].astype(np.longdouble), ax)


@pytest.mark.parametrize("shape", K.SHAPE_LIST, ids=SHAPE_IDS)
def test_transform_alone(hip_lib, shape):
    _, _, x0 = K.inputs(shape)
    x0 = np.array(x0)
    inn = K.interior(x0.shape)
    sh = K.shell_mask(x0.shape)
    absx = np.abs(x0)
    absx[sh] = 0.0
    ctx = api.HipProjection(*shape)
    try:
        first = {}
        for axis in _axes(shape):
            n = shape[axis] - 2
            Qld = K.cos_matrix_ld(n)
            Qd = K.cos_matrix(n).astype(np.longdouble)  # the table's doubles
            for inverse in (False, True):
                T, Td = (Qld.T, Qd.T) if inverse else (Qld, Qd)
                y = x0.copy()
                assert ctx.dct_transform(y, axis, inverse) == A.CFD_SUCCESS, _native.last_error()
                first[axis, inverse] = y
                want = _ld_product(T, x0, axis)
                bound = (n + 2) * U * _ld_product(np.abs(Td), absx, axis)
                err = np.abs(y[inn].astype(np.longdouble) - want)
                worst = float(np.max(err / np.maximum(bound, np.longdouble(1e-300))))
                print(f"DCT transform {K.sid(shape)} axis {axis} inverse {int(inverse)}: "
                      f"error / bound {worst:.3f}")
                assert np.all(err <= bound), (axis, inverse, worst)
                assert np.array_equal(y[sh], x0[sh]), f"axis {axis}: boundary cells written"
            # forward then inverse: the input. The first pass's error goes
            # through |Q^T| and the second adds its own on |Q^T| |y|
            z = first[axis, False].copy()
            assert ctx.dct_transform(z, axis, True) == A.CFD_SUCCESS
            absy = np.zeros_like(absx)
            absy[inn] = _ld_product(np.abs(Qd), absx, axis).astype(np.float64)
            bound2 = 2 * (n + 2) * U * _ld_product(np.abs(Qd.T), absy, axis) * (1 + 1e-12)
            err2 = np.abs(z[inn].astype(np.longdouble) - x0[inn].astype(np.longdouble))
            assert np.all(err2 <= bound2), (axis, float(np.max(err2 / bound2)))
            assert np.array_equal(z[sh], x0[sh])
        # NaN through every work field of the context (a solve on NaN fields,
        # then NaN transforms), and NaN on the input's shell: no pass may read
        # a cell it does not own
        nan = np.full(x0.shape, np.nan)
        ctx.poisson_solve(DCT, nan.copy(), nan.copy(), *K.spacing(shape))
        for axis in _axes(shape):
            for inverse in (False, True):
                ctx.dct_transform(nan.copy(), axis, inverse)
        holed = x0.copy()
        holed[sh] = np.nan
        for axis in _axes(shape):
            for inverse in (False, True):
                y = holed.copy()
                assert ctx.dct_transform(y, axis, inverse) == A.CFD_SUCCESS
                assert np.array_equal(y[inn], first[axis, inverse][inn]), \
                    f"axis {axis} inverse {inverse}: differs after NaN fields"
                assert np.isnan(y[sh]).all()
    finally:
        ctx.close()


# ---------------------------------------------------------------------------
# the solve
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", K.SHAPE_LIST, ids=SHAPE_IDS)
def test_solve(hip_lib, shape):
    good, bad, x0 = K.inputs(shape)
    d = K.spacing(shape)
    inn = K.interior(x0.shape)
    ctx = api.HipProjection(*shape)
    fails = []
    try:
        for which, rhs in (("compatible", good), ("incompatible", bad)):
            m = K.model(shape, which)
            x = np.array(x0)
            # max_iterations, check_interval and omega are ignored
            prm = oracle.poisson_params(max_iterations=0, check_interval=7, omega=1.9)
            s, st = ctx.poisson_solve(DCT, x, rhs, *d, prm)
            dev_m = K.rel_dev(x, m.x)
            r1 = abs(st.final_residual - m.final_residual) / m.initial_residual
            line = (f"DCT solve {K.sid(shape)} {which}: model {dev_m:.3e} res0 "
                    f"{st.initial_residual:.6e} res {st.final_residual:.3e} "
                    f"(model {m.final_residual:.3e}) {st.elapsed_time_ms:.3f} ms")
            try:
                assert np.isfinite(x).all()
                assert dev_m <= K.DCT_BAR, f"x off the model by {dev_m:.3e}"
                if which == "compatible":
                    rc, status, _, ref = K.tight_relax(shape)
                    assert (rc, status) == (A.CFD_SUCCESS, A.POISSON_CONVERGED)
                    dev = K.rel_dev(x, ref)
                    line += f" tight RB-SOR {dev:.3e}"
                    assert dev <= K.DCT_BAR, f"x off the tight RB-SOR by {dev:.3e}"
                # the shell is the Neumann BC of the device's own interior
                again = x.copy()
                oracle.poisson_apply_bc(again)
                assert np.array_equal(again, x), "the end BC's shell"
                # the zero mode is dropped
                assert abs(np.mean(x[inn])) <= 1e-13 * np.max(np.abs(x))
                # k_residual_linf's value of x0 as it stands = the oracle's
                assert st.initial_residual == m.initial_residual == \
                    K.oracle_initial_residual(x0, rhs, d)
                assert r1 <= 1e-9, r1
                assert (s, st.status, st.iterations) == (m.rc, m.status, m.iterations), \
                    (s, st.status, st.iterations)
                assert st.iterations == 1 and st.elapsed_time_ms > 0.0
                ps = ctx.poisson_stats()
                assert (ps.status, ps.iterations, ps.initial_residual, ps.final_residual) == \
                    (st.status, st.iterations, st.initial_residual, st.final_residual)
            except AssertionError as e:
                fails.append(f"{which}: {e}")
            print(line)
    finally:
        ctx.close()
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("shape", [(3, 3, 3), (23, 19, 1), (10, 11, 12)], ids=K.sid)
def test_solve_exits(hip_lib, shape):
    good, _, x0 = K.inputs(shape)
    d = K.spacing(shape)
    ctx = api.HipProjection(*shape)
    try:
        ok = np.array(x0)
        s, st = ctx.poisson_solve(DCT, ok, good, *d)
        assert s == A.CFD_SUCCESS
        # an unreachable tolerance: MAX_ITER, the same x
        m = K.model_solve(x0, good, d, tolerance=1e-30, absolute_tolerance=1e-300)
        x = np.array(x0)
        prm = oracle.poisson_params(tolerance=1e-30, absolute_tolerance=1e-300)
        s, u = ctx.poisson_solve(DCT, x, good, *d, prm)
        if st.final_residual > 0.0:
            assert (s, u.status, u.iterations) == (A.CFD_ERROR_MAX_ITER, A.POISSON_MAX_ITER, 1)
        assert (s, u.status) == (m.rc, m.status) or m.final_residual == 0.0
        assert np.array_equal(x, ok) and u.final_residual == st.final_residual
        # nothing to solve: converged at the start, no iteration, x untouched
        # (shell included: no end BC)
        x = np.full(x0.shape, 0.25)
        x[0, 0, 0] = 7.0  # a corner no stencil reads
        keep = x.copy()
        s, z = ctx.poisson_solve(DCT, x, np.zeros_like(x), *d)
        assert (s, z.status, z.iterations) == (A.CFD_SUCCESS, A.POISSON_CONVERGED, 0)
        assert z.initial_residual == z.final_residual < 1e-10
        assert np.array_equal(x, keep)
    finally:
        ctx.close()


def test_determinism_and_other_solvers_unaffected(hip_lib, monkeypatch):
    monkeypatch.setenv("CFD_HIP_CG_SMALL", "0")  # CG on the sweeps: the whole p ring
    shape = (67, 35, 18)
    good, _, x0 = K.inputs(shape)
    d = K.spacing(shape)
    prm = oracle.poisson_params(max_iterations=40)
    others = (A.HIP_POISSON_CG, A.HIP_POISSON_REDBLACK, A.HIP_POISSON_DST)

    def solve(ctx, method):
        x = np.array(x0)
        s, st = ctx.poisson_solve(method, x, good, *d, prm)
        return s, st.iterations, st.initial_residual, st.final_residual, x

    fresh = {}
    for method in others:
        ctx = api.HipProjection(*shape)
        try:
            fresh[method] = solve(ctx, method)
        finally:
            ctx.close()
    ctx = api.HipProjection(*shape)
    try:
        a = solve(ctx, DCT)
        after = {}
        for method in others:
            after[method] = solve(ctx, method)
            b = solve(ctx, DCT)
            assert a[:4] == b[:4] and np.array_equal(a[4], b[4]), method
    finally:
        ctx.close()
    for method in others:
        assert after[method][:4] == fresh[method][:4], method
        assert np.array_equal(after[method][4], fresh[method][4]), method


# ---------------------------------------------------------------------------
# the projection step
# ---------------------------------------------------------------------------
_STEP_REF = {}


def _step_reference(shape):
    """One oracle step with its RB-SOR at STEP_TOL, once per shape."""
    if shape not in _STEP_REF:
        g, f, prm = K.grid_field(shape, K.step_fields(shape))
        oracle.set_projection_poisson_params(oracle.poisson_params(**K.STEP_PARAMS))
        try:
            s, ost, _ = oracle.projection_step(f, g, prm, A.ORACLE_POISSON_REDBLACK)
        finally:
            oracle.set_projection_poisson_params(None)
        assert s == A.CFD_SUCCESS
        assert oracle.last_poisson_stats().status == A.POISSON_CONVERGED
        _STEP_REF[shape] = {k: np.array(getattr(f, k)) for k in ("u", "v", "w", "p", "T")}
        _STEP_REF[shape]["stats"] = ost
    return _STEP_REF[shape]


def _velocity_bound(shape, p_ref, field_ref):
    """The corrector is linear in p: u = u* - (dt / rho) grad p by central
    differences, so a p within DCT_BAR max |p - mean| moves a velocity by at
    most (dt / rho) DCT_BAR max |p - mean| / h; plus 4 ulp of the field."""
    h = min(v for v in K.spacing(shape) if v > 0.0)
    pmax = float(np.max(np.abs(K.demean(p_ref))))
    return K.STEP_DT * K.DCT_BAR * pmax / h + 4 * np.spacing(float(np.max(np.abs(field_ref))))


def _check_step(got, ref, shape, what):
    fails = []
    dev = K.rel_dev(got["p"], ref["p"])
    print(f"DCT step {what} p: {dev:.3e}")
    if not dev <= K.DCT_BAR:
        fails.append(f"p {dev:.3e}")
    for k in ("u", "v", "w"):
        bound = _velocity_bound(shape, ref["p"], ref[k])
        err = float(np.max(np.abs(got[k] - ref[k])))
        print(f"DCT step {what} {k}: {err:.3e} (bound {bound:.3e})")
        if not err <= bound:
            fails.append(f"{k} {err:.3e} > {bound:.3e}")
    assert not fails, (what, fails)


@pytest.mark.parametrize("shape", K.STEP_SHAPES, ids=K.sid)
def test_step_device(hip_lib, shape):
    ref = _step_reference(shape)
    g, f, prm = K.grid_field(shape, K.step_fields(shape))
    ctx = api.HipProjection(*shape, poisson_method=DCT)
    try:
        ctx.upload(f)
        stats = A.SolverStats()
        assert ctx.step_device(g, prm, stats) == A.CFD_SUCCESS, _native.last_error()
        st = ctx.poisson_stats()
        assert (st.status, st.iterations) == (A.POISSON_CONVERGED, 1)
        assert st.final_residual < 1e-9 * st.initial_residual
        # the step's own statistics: the oracle's, but for the pressure
        # constant (max_pressure follows it)
        ost = ref["stats"]
        assert (stats.iterations, stats.status) == (ost.iterations, ost.status)
        assert stats.max_temperature == ost.max_temperature
        assert abs(stats.max_velocity - ost.max_velocity) <= \
            2 * _velocity_bound(shape, ref["p"], ref["u"])
        ctx.download(f)
        T = ctx.get_field(A.HIP_FIELD_T)
    finally:
        ctx.close()
    got = {k: np.array(getattr(f, k)) for k in ("u", "v", "w", "p")}
    _check_step(got, ref, shape, f"step_device {K.sid(shape)}")
    assert np.array_equal(T, ref["T"])
    inn = K.interior(got["p"].shape)
    assert abs(np.mean(got["p"][inn])) <= 1e-13 * np.max(np.abs(got["p"]))


@pytest.mark.parametrize("shape", K.STEP_SHAPES, ids=K.sid)
def test_plugin_step_in_a_child(hip_lib, shape, tmp_path):
    ref = _step_reference(shape)
    src, dst = tmp_path / "in.npz", tmp_path / "out.npz"
    nz = shape[2]
    np.savez(src, shape=np.array(shape),
             box=np.array([K.D.BOX[0], K.D.BOX[1], K.D.BOX[2] if nz > 1 else 0.0]),
             dt=K.STEP_DT, nu=K.STEP_NU, steps=1, **K.step_fields(shape))
    env = dict(os.environ, CFD_HIP_POISSON="dct")
    env["PYTHONPATH"] = str(ROOT) + os.pathsep + env.get("PYTHONPATH", "")
    worker = str(ROOT / "tests" / "dst_plugin_worker.py")  # steps of the plugin, any method
    r = subprocess.run([sys.executable, worker, str(src), str(dst)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DST_PLUGIN_OK" in r.stdout, (r.stdout + r.stderr)[-4000:]
    got = np.load(dst)
    _check_step(got, ref, shape, f"plugin {K.sid(shape)}")
    # ... and it was the cosine solve: the interior mean of p is zero, which
    # no other method of the plugin leaves behind from a random p
    inn = K.interior(got["p"].shape)
    assert abs(np.mean(got["p"][inn])) <= 1e-13 * np.max(np.abs(got["p"]))


def _grad(p, d):
    """Central differences of p on the interior (the corrector's)."""
    nz = p.shape[0]
    kk = slice(1, -1) if nz > 1 else slice(None)
    gx = (p[kk, 1:-1, 2:] - p[kk, 1:-1, :-2]) / (2 * d[0])
    gy = (p[kk, 2:, 1:-1] - p[kk, :-2, 1:-1]) / (2 * d[1])
    return gx, gy


def test_incompatible_step(hip_lib):
    """A lid-driven cavity step whose right-hand side has a non-zero interior
    mean: the status is the model's, and with poisson_fail_fatal = 0 the step
    goes on with the least-squares pressure, whose gradient is the model's."""
    shape = K.CAVITY_SHAPE
    d = K.spacing(shape)
    rhs, res0 = K.cavity_rhs()
    fields = K.cavity_fields()
    m = K.model_solve(fields["p"], rhs, d)
    mean = abs(float(np.mean(rhs[K.interior(rhs.shape)])))
    print(f"DCT cavity step: |mean rhs| {mean:.3e}, threshold "
          f"{max(1e-6 * m.initial_residual, 1e-10):.3e}, model status {m.status}")
    assert m.status == A.POISSON_MAX_ITER  # the case this test is about
    assert abs(m.initial_residual - res0) <= 1e-12 * res0
    for fatal in (1, 0):
        g, f, prm = K.grid_field(shape, fields)
        ctx = api.HipProjection(*shape, poisson_method=DCT, poisson_fail_fatal=fatal)
        try:
            ctx.upload(f)
            s = ctx.step_device(g, prm)
            st = ctx.poisson_stats()
            assert s == (m.rc if fatal else A.CFD_SUCCESS), (fatal, s, _native.last_error())
            assert (st.status, st.iterations) == (m.status, 1)
            assert abs(st.initial_residual - m.initial_residual) <= 1e-12 * m.initial_residual
            assert abs(st.final_residual - m.final_residual) <= 1e-9 * m.initial_residual
            if fatal:
                continue
            ctx.download(f)
        finally:
            ctx.close()
        p = np.array(f.p)
        bound = _velocity_bound(shape, m.x, fields["u"])
        for name, a, b in zip("xy", _grad(p, d), _grad(m.x, d)):
            err = K.STEP_DT * float(np.max(np.abs(a - b)))
            print(f"DCT cavity step: (dt / rho) dp/d{name} off the model's by {err:.3e} "
                  f"(bound {bound:.3e})")
            assert err <= bound, (name, err, bound)


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------
def test_refusals(hip_lib):
    shape = (20, 14, 11)
    good, _, x0 = K.inputs(shape)
    d = K.spacing(shape)
    sentinel = np.array(x0) + 3.0
    ctx = api.HipProjection(*shape)
    try:
        ctx.enable_timing(True)
        ok = np.array(x0)
        assert ctx.poisson_solve(DCT, ok, good, *d)[0] == A.CFD_SUCCESS
        assert _launches(ctx).get("residual") == 2  # the log sees a solve that runs
        p_before = ctx.get_field(A.HIP_FIELD_P)
        stats_before = ctx.poisson_stats()
        ctx.reset_timing()
        # a preconditioner
        x = sentinel.copy()
        prm = oracle.poisson_params(preconditioner=1)  # POISSON_PRECOND_JACOBI
        s, _ = ctx.poisson_solve(DCT, x, good, *d, prm)
        assert s == A.CFD_ERROR_UNSUPPORTED and "preconditioner" in _native.last_error()
        assert np.array_equal(x, sentinel)
        # a caller boundary mode
        for mode in (A.HIP_POISSON_BC_NONE, A.HIP_POISSON_BC_FIXED):
            x = sentinel.copy()
            s, _ = ctx.poisson_solve(DCT, x, good, *d, bc_mode=mode, bc_values=sentinel.copy())
            assert s == A.CFD_ERROR_UNSUPPORTED and "BC_NEUMANN" in _native.last_error(), mode
            assert np.array_equal(x, sentinel)
        # an unknown axis
        for axis in (-1, 3):
            for inverse in (False, True):
                y = sentinel.copy()
                assert ctx.dct_transform(y, axis, inverse) == A.CFD_ERROR_INVALID
                assert "axis" in _native.last_error() and np.array_equal(y, sentinel)
        assert _launches(ctx) == {}, "a refused call launched"
        assert np.array_equal(ctx.get_field(A.HIP_FIELD_P), p_before)
        assert ctx.poisson_stats().final_residual == stats_before.final_residual
        # the context still solves, to the same bits
        x = np.array(x0)
        assert ctx.poisson_solve(DCT, x, good, *d)[0] == A.CFD_SUCCESS
        assert np.array_equal(x, ok)
    finally:
        ctx.close()
    # axis 2 on a 2-D context
    shape2 = (23, 19, 1)
    ctx = api.HipProjection(*shape2)
    try:
        ctx.enable_timing(True)
        y = np.array(K.inputs(shape2)[2]) + 3.0
        keep = y.copy()
        assert ctx.dct_transform(y, 2) == A.CFD_ERROR_INVALID
        assert "2-D" in _native.last_error() and np.array_equal(y, keep)
        assert _launches(ctx) == {}
        assert ctx.dct_transform(y, 1) == A.CFD_SUCCESS
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
        ctxs = [api.HipProjection(nx, ny, nz, comm=group.comm(r, 0), poisson_method=DCT)
                for r in range(2)]
        c = ctxs[0]
        c.enable_timing(True)
        rng = np.random.default_rng(5)
        local = rng.standard_normal(c.shape)
        c.set_field(A.HIP_FIELD_P, local)
        c.reset_timing()
        x = local + 3.0
        keep = x.copy()
        s, _ = c.poisson_solve(DCT, x, np.zeros(c.shape), *d)
        assert s == A.CFD_ERROR_UNSUPPORTED and "Z-slab" in _native.last_error()
        assert "DCT" in _native.last_error() and np.array_equal(x, keep)
        for inverse in (False, True):
            assert c.dct_transform(x, 0, inverse) == A.CFD_ERROR_UNSUPPORTED
            assert "Z-slab" in _native.last_error() and np.array_equal(x, keep)
        g = api.Grid(nx, ny, nz, 0.0, K.D.BOX[0], 0.0, K.D.BOX[1], 0.0, K.D.BOX[2])
        prm = api.validation_params(K.STEP_DT, K.STEP_NU)
        assert c.step_device(g, prm) == A.CFD_ERROR_UNSUPPORTED
        assert "Z-slab" in _native.last_error()
        assert _launches(c) == {}, "a refused call launched"
        assert np.array_equal(c.get_field(A.HIP_FIELD_P), local)
    finally:
        for c in ctxs:
            c.close()
        group.close()
