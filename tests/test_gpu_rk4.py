"""rk4_hip: the RK4 integrator on the device against the
oracle restatement of rk4_impl. RK4 has no reductions, so every field is
bitwise the oracle's; the reference's own golden L2 triple
(test_ns_solver_3d.c:363-366) is checked through the plugin.

The stretched cases of tests/rk_cases.py (dx[i], dy[j] differ from index to
index; tests/test_rk_fixtures.py shows that a wrong index changes every cell)
run through both stage kernels, the x-pair one and the per-cell one
(CFD_HIP_RK_PAIR=0). The tests at the end hold for all three explicit
integrators: the zero-spacing skip, the spacing of the grid of the call, and
the refusals the reference's solvers make (the fixture's `refusals` record)."""
import json
from pathlib import Path

import numpy as np
import pytest

from cfd_amd import _abi as A
from cfd_amd import api
from oracle import oracle
from tests import cases
from tests import rk_cases as R

pytestmark = pytest.mark.gpu

F = ("u", "v", "w", "p", "rho", "T")
DOC = json.loads((Path(__file__).resolve().parent / "golden" / "euler_rk2_cases.json").read_text())
IDS = {"u": A.HIP_FIELD_U, "v": A.HIP_FIELD_V, "w": A.HIP_FIELD_W, "p": A.HIP_FIELD_P,
       "rho": A.HIP_FIELD_RHO, "T": A.HIP_FIELD_T}


def test_rk4_plugin_kat(hip_lib):
    g, f, p = cases.kat_2d()
    reg = api.Registry()
    assert reg.has("rk4_hip")
    s = reg.create("rk4_hip")
    assert s.init(g, p) == A.CFD_SUCCESS
    p.max_iter = 3  # the reference helper; the step wrapper does one step
    st = A.SolverStats()
    assert s.step(f, g, p, st) == A.CFD_SUCCESS, api._native.last_error()
    s.close()
    l2 = (cases.l2_rms(f.u), cases.l2_rms(f.v), cases.l2_rms(f.p))
    for got, want in zip(l2, cases.KAT_RK4_L2):
        assert abs(got - want) <= 1e-12
    assert l2 == cases.KAT_RK4_L2  # no reductions: bit for bit
    assert np.all(f.w == 0.0)


def _case(nx, ny, nz, buoy=False, energy=False):
    zmax = 1.0 if nz > 1 else 0.0
    g = api.Grid(nx, ny, nz, 0.0, 1.0, 0.0, 1.0, 0.0, zmax)
    f = api.FlowField(nx, ny, nz)
    rng = np.random.default_rng(5)
    for k in ("u", "v", "w"):
        getattr(f, k)[...] = 0.05 * rng.standard_normal(f.u.shape)
    if nz == 1:
        f.w[...] = 0.0
    f.p[...] = 1.0 + 0.01 * rng.standard_normal(f.u.shape)
    f.rho[...] = 1.0 + 0.1 * rng.random(f.u.shape)
    f.T[...] = 300.0 + rng.standard_normal(f.u.shape)
    p = api.params_default()  # default source term on (amp 0.1 / 0.05)
    p.dt = 1e-4
    if buoy:
        p.beta = 3.3e-3
        p.T_ref = 300.0
        p.gravity[1] = -9.81
    if energy:
        p.alpha = 1e-3
        tb = p.thermal_bc
        tb.left = tb.right = A.BC_TYPE_DIRICHLET
        tb.bottom = tb.top = A.BC_TYPE_NEUMANN
        tb.back = tb.front = A.BC_TYPE_PERIODIC
        tb.dirichlet_values.left = 301.0
        tb.dirichlet_values.right = 299.0
    return g, f, p


# 3-D shapes also cover k_rk_stage3's tiling (r03): nx = 130 / 131 put the
# wrapped x neighbour (i0 = nx - 2 / i0 + 1 = nx - 2) on lane 0 of the second
# 128-column tile, ny = 3 makes row 1 both wrapped rows, nz = 3 plane 1 both
# wrapped planes, and 11 / 9 planes split the z-march into several runs
SEAMS = [((17, 13, 11), False, False),
         ((17, 13, 11), True, True),
         ((20, 18, 1), True, False),
         ((130, 19, 9), False, False),
         ((131, 3, 7), True, False),
         ((9, 17, 3), False, False),
         ((257, 21, 5), True, True)]


@pytest.mark.parametrize("shape,buoy,energy", SEAMS)
def test_rk4_steps_bitwise(hip_lib, shape, buoy, energy):
    _steps_vs_oracle(*_case(*shape, buoy=buoy, energy=energy))


@pytest.mark.parametrize("shape,buoy,energy", SEAMS)
def test_rk4_steps_bitwise_per_cell_kernel(hip_lib, monkeypatch, shape, buoy, energy):
    """k_rk_stage, one cell per lane in 64 x 4 tiles (the context reads the
    switch when it is created)."""
    monkeypatch.setenv("CFD_HIP_RK_PAIR", "0")
    _steps_vs_oracle(*_case(*shape, buoy=buoy, energy=energy))


RK4_STRETCHED = [c["name"] for c in R.CASES
                 if c["stretch"] and (c["pattern"] == "steps" or c["zero"])]


@pytest.mark.parametrize("pair", ["1", "0"])
@pytest.mark.parametrize("name", RK4_STRETCHED)
def test_rk4_stretched_steps_bitwise(hip_lib, monkeypatch, name, pair):
    monkeypatch.setenv("CFD_HIP_RK_PAIR", pair)
    case = R.BY_NAME[name]
    g, f, p = R.make_inputs(case)
    R.params_for(case, "rk4", p, "steps")
    _steps_vs_oracle(g, f, p)


def _steps_vs_oracle(g, f, p):
    shape = (g.nx, g.ny, g.nz)
    fo = api.FlowField(*shape)
    fo.copy_from(f)
    ctx = api.HipProjection(*shape)
    for _ in range(4):
        sh = A.SolverStats()
        assert ctx._lib().hip_rk4_step(ctx.ctx, f.ptr, g.ptr, api.C.byref(p),
                                       api.C.byref(sh)) == A.CFD_SUCCESS, api._native.last_error()
        so, sto = oracle.rk4_step(fo, g, p)
        assert so == A.CFD_SUCCESS
        assert sh.max_velocity == sto.max_velocity
        assert sh.max_pressure == sto.max_pressure
        assert sh.max_temperature == sto.max_temperature
    ctx.close()
    for k in F:
        np.testing.assert_array_equal(getattr(f, k), getattr(fo, k), err_msg=k)


def test_rk4_device_resident_matches_host_path(hip_lib):
    g, f, p = _case(17, 13, 11, buoy=True)
    fh = api.FlowField(17, 13, 11)
    fh.copy_from(f)
    ctx = api.HipProjection(17, 13, 11)
    ids = {"u": A.HIP_FIELD_U, "v": A.HIP_FIELD_V, "w": A.HIP_FIELD_W, "p": A.HIP_FIELD_P,
           "rho": A.HIP_FIELD_RHO, "T": A.HIP_FIELD_T}
    for k, i in ids.items():
        ctx.set_field(i, getattr(f, k))
    for _ in range(3):
        assert ctx._lib().hip_rk4_step_device(ctx.ctx, g.ptr, api.C.byref(p),
                                              api.C.byref(A.SolverStats())) == A.CFD_SUCCESS
    dev = {k: ctx.get_field(i) for k, i in ids.items()}
    ctx.close()
    ctx2 = api.HipProjection(17, 13, 11)
    for _ in range(3):
        assert ctx2._lib().hip_rk4_step(ctx2.ctx, fh.ptr, g.ptr, api.C.byref(p),
                                        api.C.byref(A.SolverStats())) == A.CFD_SUCCESS
    ctx2.close()
    for k in ids:
        np.testing.assert_array_equal(dev[k], getattr(fh, k), err_msg=k)


# --- all three explicit integrators on stretched grids -----------------------
def _fresh_step(integ, case, g, f, p):
    """One step of a fresh context on a copy of f; returns the copy."""
    fc = api.FlowField(*case["shape"])
    fc.copy_from(f)
    ctx = api.HipProjection(*case["shape"])
    assert getattr(ctx, f"{integ}_step")(fc, g, p) == A.CFD_SUCCESS, api._native.last_error()
    ctx.close()
    return fc


@pytest.mark.parametrize("integ", R.INTEGRATORS)
def test_zero_spacing_cells_keep_their_inputs(hip_lib, integ):
    """stzero17: |dx[5]|, |dx[10]| < 1e-10 and dy[3] = 0. The RHS skips those
    cells (column 5 is the b cell of its x pair, column 10 the a cell), so
    their u, v, w, p are bitwise the inputs after a step; column 4 moves."""
    case = R.BY_NAME["stzero17"]
    g, f, p = R.make_inputs(case)
    R.params_for(case, integ, p)
    got = _fresh_step(integ, case, g, f, p)
    for k in ("u", "v", "w", "p"):
        a, b = getattr(got, k), getattr(f, k)
        for i in R.ZERO_COLS:
            np.testing.assert_array_equal(a[1:-1, 1:-1, i], b[1:-1, 1:-1, i], err_msg=f"{k} col {i}")
        for j in R.ZERO_ROWS:
            np.testing.assert_array_equal(a[1:-1, j, 1:-1], b[1:-1, j, 1:-1], err_msg=f"{k} row {j}")
    keep = [j for j in range(1, case["shape"][1] - 1) if j not in R.ZERO_ROWS]
    for k in ("u", "v", "p"):
        assert np.all(getattr(got, k)[1:-1, keep, 4] != getattr(f, k)[1:-1, keep, 4]), k


@pytest.mark.parametrize("integ", R.INTEGRATORS)
def test_spacing_follows_the_grid_of_the_call(hip_lib, integ):
    """One context stepped with the uniform grid, the stretched grid and the
    uniform grid again (fields reset each time): each result is bitwise that
    of a fresh context on the same grid, so no spacing or source table of an
    earlier call survives."""
    cu, cs = R.BY_NAME["s17"], R.BY_NAME["st17"]
    gu, fu, p = R.make_inputs(cu)
    gs, fs, _ = R.make_inputs(cs)
    R.params_for(cu, integ, p)
    want_u = _fresh_step(integ, cu, gu, fu, p)
    want_s = _fresh_step(integ, cs, gs, fu, p)  # the same fields on the other grid
    assert not np.array_equal(want_u.u, want_s.u)
    ctx = api.HipProjection(*cu["shape"])
    for g, want in ((gu, want_u), (gs, want_s), (gu, want_u)):
        f = api.FlowField(*cu["shape"])
        f.copy_from(fu)
        assert getattr(ctx, f"{integ}_step")(f, g, p) == A.CFD_SUCCESS, api._native.last_error()
        for k in F:
            np.testing.assert_array_equal(getattr(f, k), getattr(want, k), err_msg=k)
    ctx.close()


def _entry_points(ctx):
    """Every way into a step: (name, call on a host field, call on the context's fields)."""
    out = [("projection", ctx.step, ctx.step_device)]
    for integ in R.INTEGRATORS:
        out.append((integ, getattr(ctx, f"{integ}_step"), getattr(ctx, f"{integ}_step_device")))
    return out


@pytest.mark.parametrize("which", R.REFUSALS)
def test_refusals_of_the_reference(hip_lib, which):
    """The energy equation on a stretched x / y grid (the reference returns
    CFD_ERROR_UNSUPPORTED from energy_step_explicit, its field half advanced)
    and a non-uniform dz (CFD_ERROR_INVALID) are refused with the reference's
    status before anything is uploaded or computed: the caller's arrays and
    the context's fields stay as they were."""
    rec = DOC["refusals"][which]
    g, f, p = R.refusal_inputs(which)
    shape = tuple(f.u.shape[::-1])
    ctx = api.HipProjection(*shape)
    on_ctx = {k: getattr(f, k) + 1.0 for k in F}  # not what the host field holds
    for k, i in IDS.items():
        ctx.set_field(i, on_ctx[k])
    before = f.arrays()
    for name, host_call, device_call in _entry_points(ctx):
        # the projection solver of the reference refuses both inputs as its
        # integrators do (it shares the energy step and has its own dz check)
        want = rec["rk4" if name == "projection" else name]
        assert host_call(f, g, p) == want, (name, api._native.last_error())
        assert device_call(g, p) == want, (name, api._native.last_error())
        for k in F:
            np.testing.assert_array_equal(getattr(f, k), before[k], err_msg=f"{name} host {k}")
            np.testing.assert_array_equal(ctx.get_field(IDS[k]), on_ctx[k],
                                          err_msg=f"{name} context {k}")
    ctx.close()
    assert rec["rk4"] == (A.CFD_ERROR_UNSUPPORTED if which == "stretched_xy_with_energy"
                          else A.CFD_ERROR_INVALID)
