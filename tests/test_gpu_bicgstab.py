"""BiCGSTAB on the device (k_bcg_v / k_bcg_t / k_bcg_x, bicgstab.hpp) against the
long-double restatement of the reference's loop (tests/bicgstab_reference.py),
on the case table of tests/bicgstab_cases.py.

Capped solves at the textbook sweeps' seam shapes (128 columns x 8 and 16
rows, kchunk remainder runs, the smallest legal grids) at 1, 2 and 5
iterations: status MAX_ITER, the exact count, both residual norms and x within
BAR = 1e-11 (bicgstab_cases.BAR: 100 x the reference's own fp64 deviation from
the restatement; the kernels differ from the reference only in how the dot
products are grouped). Then every exit with its exact status, return code and
iteration count, the create_bicgstab_gpu_solver path, the refusals,
determinism, scratch shared with CG, and the three timers. The Z-slab refusal
is by code reading (the dist(c) check of hip_proj_poisson_solve_ex).

Measured on an MI355X over every case (bar 1e-11): x within 2.2e-15, the
residual norms within 2.0e-15 relative, except the final residual of the
5 x 4 x 3 grid after 5 iterations (6 unknowns, ||r|| down to 3e-7 ||r_0||),
1.5e-13; the reference's own fp64 solver is 9.8e-14 off there.
"""
import ctypes as C

import numpy as np
import pytest

from cfd_amd import _abi as A
from cfd_amd import _native, api
from oracle import oracle
from tests import bicgstab_cases as K
from tests import bicgstab_reference as B
from tests import cg_reference as R
from tests import cg_seam_shapes as T

pytestmark = pytest.mark.gpu

BCG = A.HIP_POISSON_BICGSTAB
HOST_BC = C.CFUNCTYPE(None, C.c_void_p, A.c_double_p)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    # CG runs beside BiCGSTAB in the scratch test: keep it on the sweeps, which
    # use the whole p ring
    monkeypatch.setenv("CFD_HIP_CG_SMALL", "0")


def _params(case):
    return oracle.poisson_params(**K.solver_params(case))


def _solve(ctx, case, method=BCG, **kw):
    rhs, x0 = K.inputs(case)
    x = x0.copy()
    s, st = ctx.poisson_solve(method, x, rhs, *T.spacing(case["shape"]), _params(case), **kw)
    return s, st, x


def _check(case, s, st, x, ref, tile, kc=None, what=""):
    """Exact status, return code and iterations; residuals and x within BAR.
    Every message names the worst cell's tile."""
    tag = f"{what} {case['name']}"
    where = R.worst_cell(x, ref.x, tile, kc)
    assert (s, st.status, st.iterations) == (ref.rc, ref.status, ref.iterations), \
        f"{tag}: rc {s} status {st.status} iterations {st.iterations}, want " \
        f"{(ref.rc, ref.status, ref.iterations)}; {where}"
    assert np.isfinite(x).all(), f"{tag}: x not finite; {where}"
    dev = K.deviation(x, st.initial_residual, st.final_residual, ref)
    print(f"BCG {tag}: x {dev[0]:.3e} res0 {dev[1]:.3e} res {dev[2]:.3e}")  # before the gates
    assert dev[1] <= K.BAR, f"{tag}: initial residual {st.initial_residual!r}; {where}"
    assert dev[2] <= K.BAR, f"{tag}: final residual {st.final_residual!r}, want " \
                            f"{ref.final_residual!r}; {where}"
    assert dev[0] <= K.BAR, f"{tag}: x off by {dev[0]:.3e} > {K.BAR:.0e}; {where}"


def _capped_groups():
    groups = {}
    for c in K.CASES:
        if c["kind"] == "capped":
            groups.setdefault((c["shape"], c["kchunk"]), []).append(c)
    return groups


CAPPED = _capped_groups()


@pytest.mark.parametrize("rows", [8, 16])
@pytest.mark.parametrize("key", list(CAPPED),
                         ids=[T.sid(s) + (f"-kc{k}" if k else "") for s, k in CAPPED])
def test_capped_seam_solves(hip_lib, key, rows):
    shape, kchunk = key
    cfg = dict(sweep_rows=rows, **({"kchunk": kchunk} if kchunk else {}))
    fails = []
    ctx = api.HipProjection(*shape, **cfg)
    try:
        for case in CAPPED[key]:
            s, st, x = _solve(ctx, case)
            ref = K.reference(case["name"])
            assert ref.status == B.ST_MAX_ITER and ref.iterations == case["max_iterations"]
            try:
                _check(case, s, st, x, ref, (128, rows), kchunk or None, f"rows {rows}")
            except AssertionError as e:
                fails.append(str(e))
    finally:
        ctx.close()
    assert not fails, "\n".join(fails)


EXITS = [c for c in K.CASES if c["kind"] != "capped"]


@pytest.mark.parametrize("case", EXITS, ids=[c["name"] for c in EXITS])
def test_exits_and_stats(hip_lib, case):
    ref = K.reference(case["name"])
    assert (ref.exit, ref.iterations) == case["expect"]
    ctx = api.HipProjection(*case["shape"])
    try:
        s, st, x = _solve(ctx, case)
    finally:
        ctx.close()
    _check(case, s, st, x, ref, (128, 8))
    if ref.exit in (B.EXIT_START, B.EXIT_RHO):
        # x with the opening shell copy only
        want = K.inputs(case)[1].copy()
        R.neumann_shell(want)
        assert np.array_equal(x, want)
        assert st.final_residual == 0.0 and st.initial_residual == 0.0


def _plugin_solve(case, bc=None):
    """create_bicgstab_gpu_solver, then the host mirror's init and solve."""
    host = _native.host()
    rhs, x0 = K.inputs(case)
    nx, ny, nz = case["shape"]
    s = api.bicgstab_gpu_solver()
    cb = None
    if bc is not None:
        cb = HOST_BC(lambda _s, ptr: bc(np.ctypeslib.as_array(ptr, shape=(nz * ny * nx,))
                                        .reshape(nz, ny, nx)))
        s.contents.apply_bc = C.cast(cb, C.c_void_p).value
    prm = _params(case)
    try:
        assert host.poisson_solver_init(s, nx, ny, nz, *T.spacing(case["shape"]),
                                        C.byref(prm)) == A.CFD_SUCCESS, _native.last_error()
        x = x0.copy()
        st = host.poisson_solver_stats_default()
        rc = host.poisson_solver_solve(s, x.ctypes.data_as(A.c_double_p), None,
                                       np.ascontiguousarray(rhs).ctypes.data_as(A.c_double_p),
                                       C.byref(st))
    finally:
        host.poisson_solver_destroy(s)
    return rc, st, x


def test_plugin_path(hip_lib):
    case = K.BY_NAME["conv-17x13x11-3.980e-02"]
    ctx = api.HipProjection(*case["shape"])
    try:
        s, st, x = _solve(ctx, case)
    finally:
        ctx.close()
    rc, pst, px = _plugin_solve(case)
    assert (rc, pst.status, pst.iterations) == (s, st.status, st.iterations)
    assert (pst.initial_residual, pst.final_residual) == (st.initial_residual, st.final_residual)
    assert np.array_equal(px, x)
    _check(case, rc, pst, px, K.reference(case["name"]), (128, 8), what="plugin")
    # an override that leaves the boundary alone: the restatement's "keep" form
    calls = []
    rc, kst, kx = _plugin_solve(case, bc=lambda a: calls.append(1))
    assert len(calls) == 2  # solve start and end
    _check(case, rc, kst, kx, K.reference(case["name"], "keep"), (128, 8), what="plugin keep")
    x0 = K.inputs(case)[1]
    inn = R.interior(x0.shape)
    shell = np.ones(x0.shape, bool)
    shell[inn] = False
    assert np.array_equal(kx[shell], x0[shell])


def test_refusals(hip_lib):
    case = K.BY_NAME["ci4-max2"]
    rhs, x0 = K.inputs(case)
    d = T.spacing(case["shape"])
    sentinel = x0 + 3.0
    ctx = api.HipProjection(*case["shape"])
    try:
        x = sentinel.copy()
        s, _ = ctx.poisson_solve(BCG, x, rhs, *d, _params(case),
                                 bc_mode=A.HIP_POISSON_BC_FIXED, bc_values=x0)
        assert s == A.CFD_ERROR_UNSUPPORTED and "BC_FIXED" in _native.last_error()
        assert np.array_equal(x, sentinel)
        # the context still solves
        s, st, x = _solve(ctx, case)
        _check(case, s, st, x, K.reference(case["name"]), (128, 8), what="after refusal")
    finally:
        ctx.close()
    ctx = api.HipProjection(*case["shape"], cg_variant=1)
    try:
        x = sentinel.copy()
        s, _ = ctx.poisson_solve(BCG, x, rhs, *d, _params(case))
        assert s == A.CFD_ERROR_UNSUPPORTED and "cg_variant" in _native.last_error()
        assert np.array_equal(x, sentinel)
    finally:
        ctx.close()


def test_determinism(hip_lib):
    case = K.BY_NAME["cap-130x17x7-it5"]
    ctx = api.HipProjection(*case["shape"])
    try:
        s1, st1, x1 = _solve(ctx, case)
        s2, st2, x2 = _solve(ctx, case)
    finally:
        ctx.close()
    assert s1 == s2 and st1.iterations == st2.iterations
    assert (st1.initial_residual, st1.final_residual) == (st2.initial_residual,
                                                           st2.final_residual)
    assert np.array_equal(x1, x2)


def test_scratch_shared_with_cg(hip_lib):
    """CG, BiCGSTAB, CG on one context: each result bitwise a fresh context's."""
    case = K.BY_NAME["cap-130x17x7-it5"]

    def fresh(method):
        ctx = api.HipProjection(*case["shape"])
        try:
            return _solve(ctx, case, method)
        finally:
            ctx.close()

    s_cg, st_cg, x_cg = fresh(A.HIP_POISSON_CG)
    s_b, st_b, x_b = fresh(BCG)
    ctx = api.HipProjection(*case["shape"])
    try:
        runs = [_solve(ctx, case, m) for m in (A.HIP_POISSON_CG, BCG, A.HIP_POISSON_CG)]
    finally:
        ctx.close()
    for (s, st, x), (ws, wst, wx) in zip(runs, [(s_cg, st_cg, x_cg), (s_b, st_b, x_b),
                                                (s_cg, st_cg, x_cg)]):
        assert (s, st.iterations, st.final_residual) == (ws, wst.iterations, wst.final_residual)
        assert np.array_equal(x, wx)


def test_timers(hip_lib):
    case = K.BY_NAME["cap-130x17x7-it5"]
    ctx = api.HipProjection(*case["shape"])
    try:
        ctx.reset_timing()
        ctx.enable_timing(True)
        s, st, x = _solve(ctx, case)
        kt = ctx.timing()
    finally:
        ctx.close()
    _check(case, s, st, x, K.reference(case["name"]), (128, 8), what="timed")
    n = case["max_iterations"]
    assert [kt[k][1] for k in ("bcg_v", "bcg_t", "bcg_x")] == [n, n, n], kt
    assert kt["cg_sweep_a"][1] == 0 and kt["cg_sweep_b"][1] == 0
