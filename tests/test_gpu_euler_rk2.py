"""Explicit Euler and RK2 on the device against fixtures from the reference's
own CPU solvers (tests/golden/euler_rk2_cases.json, make_rk_golden.py): neither
integrator has a reduction, so every field is bitwise explicit_euler_impl's /
rk2_impl's. Step-wise cases drive hip_*_step, the max_iter = 4 cases the
device API's solve_*_method_gpu (source index 0..3, decay rate 0.5)."""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest

from cfd_amd import _abi as A
from cfd_amd import _native, api
from tests import cases
from tests import rk_cases as R

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
DOC = json.loads((GOLDEN / "euler_rk2_cases.json").read_text())
STEP_CASES = [c["name"] for c in R.CASES if c["pattern"] == "steps"]
ITER_CASES = [c["name"] for c in R.CASES if c["pattern"] == "iter"]
NEW = ("euler", "rk2")
SOLVE = {"euler": "solve_explicit_euler_method_gpu", "rk2": "solve_rk2_method_gpu"}
IDS = {"u": A.HIP_FIELD_U, "v": A.HIP_FIELD_V, "w": A.HIP_FIELD_W, "p": A.HIP_FIELD_P,
       "rho": A.HIP_FIELD_RHO, "T": A.HIP_FIELD_T}


def _step(ctx, integ, f, g, p, st=None):
    return getattr(ctx, f"{integ}_step")(f, g, p, st)


def _step_device(ctx, integ, g, p):
    return getattr(ctx, f"{integ}_step_device")(g, p)


def _check_fields(name, integ, f):
    want = DOC["cases"][name]["runs"][integ]["outputs"]
    for k in R.FIELDS:
        got = R.digest(getattr(f, k))
        assert got["sha256"] == want[k]["sha256"], (name, integ, k, got, want[k])
    if name in R.NPZ_FILES:
        z = np.load(GOLDEN / R.NPZ_FILES[name])
        for k in R.FIELDS:
            np.testing.assert_array_equal(getattr(f, k), z[f"{integ}_{k}"], err_msg=k)


@pytest.mark.parametrize("integ", NEW)
@pytest.mark.parametrize("name", STEP_CASES)
def test_steps_bitwise(hip_lib, name, integ):
    case = R.BY_NAME[name]
    g, f, p = R.make_inputs(case)
    ctx = api.HipProjection(*case["shape"])
    for _ in range(R.params_for(case, integ, p)):
        st = A.SolverStats()
        assert _step(ctx, integ, f, g, p, st) == A.CFD_SUCCESS, _native.last_error()
        # the stats of the step just made, from the fields it returned
        assert st.iterations == 1
        assert st.max_velocity == float(np.sqrt(np.max(f.u * f.u + f.v * f.v + f.w * f.w)))
        assert st.max_pressure == float(np.max(np.abs(f.p)))
        assert st.max_temperature == float(np.max(f.T))
    ctx.close()
    _check_fields(name, integ, f)


@pytest.mark.parametrize("integ", NEW)
@pytest.mark.parametrize("name", ITER_CASES)
def test_solve_method_gpu_bitwise(hip_lib, name, integ):
    case = R.BY_NAME[name]
    g, f, p = R.make_inputs(case)
    assert R.params_for(case, integ, p) == 1 and p.max_iter == 4
    cfg = hip_lib.gpu_config_default()
    # below the default gate (grid size / step count): CFD_ERROR, field untouched
    before = f.arrays()
    assert getattr(hip_lib, SOLVE[integ])(f.ptr, g.ptr, C.byref(p), C.byref(cfg)) == A.CFD_ERROR
    for k in R.FIELDS:
        np.testing.assert_array_equal(getattr(f, k), before[k])
    cfg.min_grid_size = 1  # what the reference's registry wrappers pass
    cfg.min_steps = 1
    assert getattr(hip_lib, SOLVE[integ])(f.ptr, g.ptr, C.byref(p),
                                          C.byref(cfg)) == A.CFD_SUCCESS, _native.last_error()
    _check_fields(name, integ, f)


@pytest.mark.parametrize("integ", NEW)
def test_device_resident_matches_host_path(hip_lib, integ):
    _device_resident_matches_host_path(integ, "s17_be")


@pytest.mark.parametrize("integ", NEW)
def test_device_resident_matches_host_path_stretched(hip_lib, integ):
    _device_resident_matches_host_path(integ, "st17_b")


def _device_resident_matches_host_path(integ, name):
    case = R.BY_NAME[name]
    g, f, p = R.make_inputs(case)
    n = R.params_for(case, integ, p)
    ctx = api.HipProjection(*case["shape"])
    for k, i in IDS.items():
        ctx.set_field(i, getattr(f, k))
    for _ in range(n):
        assert _step_device(ctx, integ, g, p) == A.CFD_SUCCESS, _native.last_error()
    dev = {k: ctx.get_field(i) for k, i in IDS.items()}
    ctx.close()
    ctx2 = api.HipProjection(*case["shape"])
    for _ in range(n):
        assert _step(ctx2, integ, f, g, p) == A.CFD_SUCCESS
    ctx2.close()
    for k in IDS:
        np.testing.assert_array_equal(dev[k], getattr(f, k), err_msg=k)
    _check_fields(name, integ, f)


@pytest.mark.parametrize("integ", NEW)
def test_projection_after_integrator_on_one_context(hip_lib, integ):
    """Euler swaps u, v, w, p with u*, v*, w*, p_new and RK2 leaves its
    predictor there: a projection step on the same context afterwards equals
    the step of a fresh context on the same state, bitwise."""
    n = 17
    g, f, p = cases.tg3(n)
    ids = {k: IDS[k] for k in ("u", "v", "w", "p", "rho")}
    a = api.HipProjection(n, n, n)
    for k, i in ids.items():
        a.set_field(i, getattr(f, k))
    for _ in range(2):
        assert _step_device(a, integ, g, p) == A.CFD_SUCCESS, _native.last_error()
    state = {k: a.get_field(i) for k, i in ids.items()}
    assert not np.array_equal(state["u"], f.u)
    for fid in (A.HIP_FIELD_U, A.HIP_FIELD_V, A.HIP_FIELD_W, A.HIP_FIELD_P):
        a.apply_scalar_bc(fid, A.BC_TYPE_PERIODIC)
    assert a.step_device(g, p) == A.CFD_SUCCESS, _native.last_error()
    it_a = a.poisson_stats().iterations
    got = {k: a.get_field(ids[k]) for k in ("u", "v", "w", "p")}
    a.close()

    b = api.HipProjection(n, n, n)
    for k in ("u", "v", "w", "p"):
        b.set_field(ids[k], state[k])
    b.set_density(1.0)
    for fid in (A.HIP_FIELD_U, A.HIP_FIELD_V, A.HIP_FIELD_W, A.HIP_FIELD_P):
        b.apply_scalar_bc(fid, A.BC_TYPE_PERIODIC)
    assert b.step_device(g, p) == A.CFD_SUCCESS
    assert b.poisson_stats().iterations == it_a
    want = {k: b.get_field(ids[k]) for k in ("u", "v", "w", "p")}
    b.close()
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


_NOOP_SOURCE = A.SourceFunc(lambda x, y, z, t, ctx, su, sv, sw: None)


@pytest.mark.parametrize("integ", NEW)
def test_refusals(hip_lib, integ):
    case = R.BY_NAME["s17"]
    g, f, p = R.make_inputs(case)
    R.params_for(case, integ, p)
    ctx = api.HipProjection(*case["shape"])
    # a source callback cannot run on the device
    ps = A.SolverParams.from_buffer_copy(p)
    ps.source_func = C.cast(_NOOP_SOURCE, C.c_void_p)
    assert _step(ctx, integ, f, g, ps) == A.CFD_ERROR_UNSUPPORTED
    # grid of another shape
    g2 = api.Grid(16, 13, 11, 0.0, 1.0, 0.0, 1.0, 0.0, 1.0)
    assert _step_device(ctx, integ, g2, p) == A.CFD_ERROR_INVALID
    # buoyancy without a temperature field on the context
    for k in ("u", "v", "w", "p", "rho"):
        ctx.set_field(IDS[k], getattr(f, k))
    pb = A.SolverParams.from_buffer_copy(p)
    pb.beta = 3.3e-3
    pb.gravity[1] = -9.81
    assert _step_device(ctx, integ, g, pb) == A.CFD_ERROR_INVALID
    ctx.close()


@pytest.mark.parametrize("integ", NEW)
def test_zslab_context_is_refused(hip_lib, integ):
    shape = (17, 13, 11)
    g, _, p = R.make_inputs(R.BY_NAME["s17"])
    p.dt = 1e-4
    grp = api.LocalGroup(2)
    ctxs = [api.HipProjection(*shape, comm=grp.comm(r, 0)) for r in range(2)]
    try:
        # refused on the host before any device or group work: no rank threads needed
        assert [_step_device(c, integ, g, p) for c in ctxs] == [A.CFD_ERROR_UNSUPPORTED] * 2
    finally:
        for c in ctxs:
            c.close()
        grp.close()
