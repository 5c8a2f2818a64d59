"""hip_proj_flow_diagnostics (cfd_amd/csrc/hip/flow_diag.hip) on the shapes of
tests/flow_diag_cases.py: against the reference helpers' recorded results
(tests/golden/flow_diag_cases.json), the numpy model and the host twin.

Bars. div_linf, div_cells, div_nan_cells: exact. A device sum of N
non-negative terms, whatever its (fixed) order, lies within N 2^-53 relative
of the exact sum and math.fsum within 2^-53 of it: (N + 1) 2^-53 relative.
With one non-zero cell in otherwise zero fields every other term is +0.0 and
adding +0.0 is exact, so each sum is the bits of the reference term (or of the
two equal terms a planted u, v or w cell gives the divergence of its two
neighbours, whose sum is exact in any order), and exactly 0.0 where the cell
is outside the quantity's domain.
"""
import ctypes as C
import json
import math
from pathlib import Path

import numpy as np
import pytest

from cfd_amd import _abi as A
from cfd_amd import _native, api
from tests import cases
from tests import flow_diag_cases as K
from tests import special_values as S
from tests.test_flow_diag_cases import make_field, make_grid

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
FID = {"u": A.HIP_FIELD_U, "v": A.HIP_FIELD_V, "w": A.HIP_FIELD_W, "rho": A.HIP_FIELD_RHO}
CASES = K.cases()
IDS = [c[0] for c in CASES]
SHAPE_IDS = [K.name_of(s) for s in K.SHAPES]
NUMBERS = ("div_linf", "div_sumsq", "div_l2", "div_cells", "div_nan_cells", "ke", "ke_rho",
           "ke_rho_cells")


@pytest.fixture(scope="session", autouse=True)
def diagnostics_entry_present():
    """Without the entry in the bindings every test here fails at once."""
    assert hasattr(api.HipProjection, "flow_diagnostics") and hasattr(A, "FlowDiag"), \
        "the bindings lack hip_proj_flow_diagnostics"


@pytest.fixture(scope="module")
def record():
    return json.loads((GOLDEN / K.JSON_FILE).read_text())


def context(shape, arrays, rho=True):
    ctx = api.HipProjection(*shape)
    for k in ("u", "v", "w") + (("rho",) if rho else ()):
        ctx.set_field(FID[k], arrays[k])
    return ctx


@pytest.fixture(scope="module")
def loaded(hip_lib):
    """(shape, w0) -> (context with u, v, w, rho resident, grid, arrays); built
    once, never modified by a test."""
    cache = {}

    def get(shape, w0=False):
        if (shape, w0) not in cache:
            arrays = K.inputs(shape, w0)
            cache[shape, w0] = (context(shape, arrays), make_grid(shape), arrays)
        return cache[shape, w0]

    yield get
    for ctx, _, _ in cache.values():
        ctx.close()


def numbers(d):
    return tuple(getattr(d, k) for k in NUMBERS)


def bits(x):
    return np.float64(x).view(np.uint64)


def same_bits(a, b):
    return (math.isnan(a) and math.isnan(b)) or bits(a) == bits(b)


def check_against_model(d, m, what=""):
    assert d.div_cells == m["div_cells"], what
    assert d.div_nan_cells == m["div_nan_cells"], what
    assert same_bits(d.div_linf, m["div_linf"]), (what, d.div_linf, m["div_linf"])
    for k in K.SUMS:
        got, want, n = getattr(d, k), m[k], m["n"][k]
        if math.isfinite(want) and want != 0.0:
            print(f"{what} {k}: |dev - fsum| / fsum = {abs(got - want) / abs(want):.3e}, "
                  f"bar {(n + 1) * K.U:.3e}")
        assert K.sum_close(got, want, n, n + 1), (what, k, got, want)
    if d.div_cells:
        assert same_bits(d.div_l2, math.sqrt(d.div_sumsq / float(d.div_cells))
                         if not math.isnan(d.div_sumsq) else math.nan), what


@pytest.mark.parametrize("name,shape,w0", CASES, ids=IDS)
def test_fixture_shapes(record, loaded, name, shape, w0):
    ctx, g, arrays = loaded(shape, w0)
    ref = {k: float.fromhex(v) for k, v in record["cases"][name]["ref"].items()}
    d = ctx.flow_diagnostics(g, K.RHO0, 3)
    assert bits(d.div_linf) == bits(ref["test_compute_divergence_linf_3d"])
    assert d.div_cells == K.interior_cells(shape) and d.div_nan_cells == 0
    check_against_model(d, K.model(shape, arrays), name)
    # the reference's sequential sums: 2 N 2^-53 from the device's, by the same argument
    n = d.div_cells
    assert K.sum_close(d.ke, ref["test_compute_kinetic_energy_3d"], n, 2 * n)
    assert abs(d.div_l2 - ref["test_compute_divergence_l2_3d"]) <= \
        (n + 2) * K.U * ref["test_compute_divergence_l2_3d"]
    if w0:
        assert K.sum_close(d.ke_rho, ref["test_compute_kinetic_energy"], n, 2 * n)
        na = shape[0] * shape[1]
        assert K.sum_close(d.ke_rho_cells, ref["compute_kinetic_energy"], na, 2 * na)


@pytest.mark.parametrize("shape", K.SHAPES, ids=SHAPE_IDS)
def test_planted_cells(hip_lib, shape):
    nx, ny, nz = shape
    g = make_grid(shape)
    base = K.inputs(shape)
    zeros = np.zeros((nz, ny, nx))
    ctx = context(shape, {"u": zeros, "v": zeros, "w": zeros, "rho": base["rho"]})
    try:
        values = {"u": 0.375, "v": -1.5, "w": 2.75}
        for pos in K.plant_positions(shape):
            for k, val in values.items():
                a = np.zeros((nz, ny, nx))
                a[pos] = val
                ctx.set_field(FID[k], a)
                arrays = {"u": zeros, "v": zeros, "w": zeros, "rho": base["rho"]}
                arrays[k] = a
                m = K.model(shape, arrays)
                d = ctx.flow_diagnostics(g, K.RHO0, 3)
                what = f"{K.name_of(shape)} {k} at {pos}"
                assert d.div_nan_cells == 0 and d.div_cells == K.interior_cells(shape), what
                assert bits(d.div_linf) == bits(m["div_linf"]), (what, d.div_linf, m["div_linf"])
                for q in K.SUMS:
                    t = m["terms"][q]
                    nz_terms = t[t != 0.0]
                    # one term, or the two equal terms of a planted cell's two neighbours
                    assert nz_terms.size <= 2 and np.all(nz_terms == nz_terms[:1]), (what, q)
                    assert bits(getattr(d, q)) == bits(m[q]), (what, q, getattr(d, q), m[q])
                ctx.set_field(FID[k], zeros)
        # the table is not vacuous: the first interior cell is in every domain,
        # its neighbour across the boundary only in ke_rho_cells'
        first = (1 if nz > 1 else 0, 1, 1)
        a = np.zeros((nz, ny, nx))
        a[first] = 0.375
        ctx.set_field(FID["u"], a)
        d = ctx.flow_diagnostics(g, K.RHO0, 3)
        assert d.ke > 0.0 and d.ke_rho > 0.0 and d.ke_rho_cells > 0.0
        a[first] = 0.0
        a[first[0], first[1], 0] = 0.375
        ctx.set_field(FID["u"], a)
        d = ctx.flow_diagnostics(g, K.RHO0, 3)
        assert (d.ke, d.ke_rho) == (0.0, 0.0) and d.ke_rho_cells > 0.0
        assert d.div_sumsq > 0.0  # u(0) is the west neighbour of the first interior cell
    finally:
        ctx.close()


@pytest.mark.parametrize("shape", [(17, 13, 11), (131, 66, 4), (34, 19, 1), (5, 70, 61)],
                         ids=lambda s: K.name_of(s))
def test_paths_agree(loaded, shape):
    ctx, g, arrays = loaded(shape)
    d3 = ctx.flow_diagnostics(g, K.RHO0, 3)
    d1 = ctx.flow_diagnostics(g, K.RHO0, A.HIP_DIAG_DIVERGENCE)
    d2 = ctx.flow_diagnostics(g, K.RHO0, A.HIP_DIAG_ENERGY)
    assert numbers(d1) == numbers(d3)[:5] + (0.0, 0.0, 0.0)
    assert numbers(d2) == (0.0, 0.0, 0.0, 0, 0) + numbers(d3)[5:]
    # run to run, and on a second context
    assert numbers(ctx.flow_diagnostics(g, K.RHO0, 3)) == numbers(d3)
    twin = context(shape, arrays)
    norho = context(shape, arrays, rho=False)
    try:
        assert numbers(twin.flow_diagnostics(g, K.RHO0, 3)) == numbers(d3)
        # without a resident rho: the constant rho0, as the model says
        dn = norho.flow_diagnostics(g, K.RHO0, 3)
        check_against_model(dn, K.model(shape, arrays, rho0=K.RHO0), "rho0")
        assert numbers(dn)[:6] == numbers(d3)[:6]
        assert dn.ke_rho != d3.ke_rho and dn.ke_rho_cells != d3.ke_rho_cells
        # rho0 is ignored where rho is resident
        assert numbers(ctx.flow_diagnostics(g, 7.0, 3)) == numbers(d3)
    finally:
        twin.close()
        norho.close()


@pytest.mark.parametrize("shape", S.STEP_SHAPES, ids=lambda s: K.name_of(s))
@pytest.mark.parametrize("regime", S.REGIMES)
def test_special_values(hip_lib, regime, shape):
    g, f, _ = S.step_fields(regime, shape)
    arrays = {k: getattr(f, k).copy() for k in K.FIELDS}
    spacing = (g.dx, g.dy, g.dz)
    ctx = context(shape, arrays)
    try:
        d = ctx.flow_diagnostics(g, K.RHO0, 3)
    finally:
        ctx.close()
    h = api.flow_diagnostics(f, g, K.RHO0, 3)
    what = f"{regime} {K.name_of(shape)}"
    assert same_bits(d.div_linf, h.div_linf), (what, d.div_linf, h.div_linf)
    assert (d.div_cells, d.div_nan_cells) == (h.div_cells, h.div_nan_cells), what
    m = K.model(shape, arrays, spacing=spacing)
    check_against_model(d, m, what)
    for k in K.SUMS:  # the host twin's sequential sums have the same class
        want, got = getattr(h, k), getattr(d, k)
        assert math.isnan(want) == math.isnan(got) and math.isinf(want) == math.isinf(got), \
            (what, k, got, want)
    if regime == "nonfinite":
        assert d.div_nan_cells > 0 and math.isnan(d.div_sumsq) and math.isnan(d.ke)


def test_special_values_reach_both_division_paths():
    """The inputs above put du/dx and dv/dy quotients on either side of the
    fast division's range, so a fallback that misrounds would show."""
    seen = {"below": 0.0, "in": 0.0, "above": 0.0}
    for regime in ("tiny", "subnormal", "huge", "planted"):
        g, f, _ = S.step_fields(regime, S.STEP_SHAPES[0])
        with np.errstate(all="ignore"):
            num = (f.u[1:-1, 1:-1, 2:] - f.u[1:-1, 1:-1, :-2]).ravel()
        sh = S.shares(num, 2.0 * g.dx)
        for k in seen:
            seen[k] = max(seen[k], sh[k])
    assert seen["below"] > 0.05 and seen["in"] > 0.05 and seen["above"] > 0.01, seen


def test_nan_in_w_alone_2d(hip_lib):
    """2-D: dw_dz = (w - w) * 0.0 is NaN for a NaN w, so every divergence is
    NaN, div_linf stays 0.0 and div_nan_cells says why."""
    shape = (34, 19, 1)
    arrays = dict(K.inputs(shape))
    arrays["w"] = np.full((1, 19, 34), np.nan)
    g = make_grid(shape)
    ctx = context(shape, arrays)
    try:
        d = ctx.flow_diagnostics(g, K.RHO0, 3)
    finally:
        ctx.close()
    h = api.flow_diagnostics(make_field(shape, arrays), g, K.RHO0, 3)
    n = K.interior_cells(shape)
    for r in (d, h):
        assert bits(r.div_linf) == bits(0.0) and r.div_nan_cells == n == r.div_cells
        assert math.isnan(r.div_sumsq) and math.isnan(r.div_l2)
        assert math.isnan(r.ke) and math.isnan(r.ke_rho) and math.isnan(r.ke_rho_cells)
    # +inf in u only: the energies are +inf, the divergence of its neighbours inf
    arrays["w"] = np.zeros((1, 19, 34))
    u = arrays["u"].copy()
    u[0, 9, 17] = np.inf
    arrays["u"] = u
    ctx = context(shape, arrays)
    try:
        d = ctx.flow_diagnostics(g, K.RHO0, 3)
    finally:
        ctx.close()
    assert d.div_linf == math.inf and d.div_sumsq == math.inf and d.div_nan_cells == 0
    assert d.ke == math.inf and d.ke_rho == math.inf and d.ke_rho_cells == math.inf


@pytest.mark.parametrize("shape", [(17, 13, 11), (131, 66, 4), (129, 5, 4), (3, 3, 1)],
                         ids=lambda s: K.name_of(s))
def test_pad_columns_never_reach_a_result(loaded, shape):
    """hip_proj_fill_field writes the whole padded array, pad columns included;
    hip_proj_set_field then writes the cells only. NaN pads must change nothing."""
    ctx, g, arrays = loaded(shape)
    want = numbers(ctx.flow_diagnostics(g, K.RHO0, 3))
    dirty = api.HipProjection(*shape)
    try:
        for k in K.FIELDS:
            dirty.fill(FID[k], math.nan)
            dirty.set_field(FID[k], arrays[k])
        assert numbers(dirty.flow_diagnostics(g, K.RHO0, 3)) == want
        assert numbers(dirty.flow_diagnostics(g, K.RHO0, 2))[5:] == want[5:]
    finally:
        dirty.close()


def test_no_side_effects(hip_lib):
    n = 17
    g, f, p = cases.tg3(n)
    ctxs = [api.HipProjection(n, n, n) for _ in range(2)]
    try:
        for c in ctxs:
            c.upload(f)
            c.set_field(A.HIP_FIELD_RHO, np.asarray(f.rho))
        a, b = ctxs
        fids = (A.HIP_FIELD_U, A.HIP_FIELD_V, A.HIP_FIELD_W, A.HIP_FIELD_P, A.HIP_FIELD_RHO)
        before = [a.field_crc32(i) for i in fids]
        for what in (1, 2, 3):
            a.flow_diagnostics(g, 1.0, what)
        assert [a.field_crc32(i) for i in fids] == before
        assert a.step_device(g, p) == A.CFD_SUCCESS and b.step_device(g, p) == A.CFD_SUCCESS
        a.flow_diagnostics(g, 1.0, 3)
        for i in fids[:4]:
            S.assert_bits_equal(a.get_field(i), b.get_field(i), what=f"field {i} after a step")
    finally:
        for c in ctxs:
            c.close()


def _launches(ctx):
    return sum(n for _, n in ctx.timing().values())


def test_refusals_launch_nothing(loaded):
    shape = (17, 13, 11)
    ctx, g, _ = loaded(shape)
    lib = _native.hip()
    fids = (A.HIP_FIELD_U, A.HIP_FIELD_V, A.HIP_FIELD_W, A.HIP_FIELD_RHO)
    before = [ctx.field_crc32(i) for i in fids]
    ctx.enable_timing(True)
    ctx.reset_timing()
    try:
        d = A.FlowDiag()
        d.ke = -7.0
        for what in (0, 4, -1, 7):
            assert lib.hip_proj_flow_diagnostics(ctx.ctx, g.ptr, 1.0, what, C.byref(d)) == \
                A.CFD_ERROR_INVALID
        assert lib.hip_proj_flow_diagnostics(None, g.ptr, 1.0, 3, C.byref(d)) == A.CFD_ERROR_INVALID
        assert lib.hip_proj_flow_diagnostics(ctx.ctx, None, 1.0, 3, C.byref(d)) == \
            A.CFD_ERROR_INVALID
        assert lib.hip_proj_flow_diagnostics(ctx.ctx, g.ptr, 1.0, 3, None) == A.CFD_ERROR_INVALID
        for other in ((18, 13, 11), (17, 14, 11), (17, 13, 12), (17, 13, 1)):
            g2 = make_grid(other)
            assert lib.hip_proj_flow_diagnostics(ctx.ctx, g2.ptr, 1.0, 3, C.byref(d)) == \
                A.CFD_ERROR_INVALID
            assert "mismatch" in _native.last_error()
        assert d.ke == -7.0  # a refusal leaves the output alone
        ctx.synchronize()
        assert _launches(ctx) == 0
    finally:
        ctx.enable_timing(False)
    assert [ctx.field_crc32(i) for i in fids] == before


def test_z_slab_contexts_are_refused(hip_lib):
    """Refused on the host before anything is launched: one rank's call
    returns at once, without its neighbour taking part."""
    nx, ny, nz = 20, 14, 11
    group = api.LocalGroup(2)
    ctxs = []
    try:
        ctxs = [api.HipProjection(nx, ny, nz, comm=group.comm(r, 0),
                                  poisson_method=A.HIP_POISSON_DST) for r in range(2)]
        c = ctxs[0]
        g = make_grid((nx, ny, nz))
        c.enable_timing(True)
        c.reset_timing()
        d = A.FlowDiag()
        for what in (1, 2, 3):
            assert _native.hip().hip_proj_flow_diagnostics(c.ctx, g.ptr, 1.0, what,
                                                           C.byref(d)) == A.CFD_ERROR_UNSUPPORTED
            assert "Z-slab" in _native.last_error()
        assert _launches(c) == 0
    finally:
        for c in ctxs:
            c.close()
        group.close()
