"""k_ccf's edge-sum form on one device (ccf.hpp, EDGE): delta = (r, A r) summed
over grid edges, 60 x 29 cells written per tile (tile ty writes rows 29 ty ..
29 ty + 28), z runs that load planes kb - 1 .. ke + 1.

Capped solves on random data (tests/cg_seam_shapes.py: problem, capped_params,
check_capped_solve, BAR = 1e-11 against the long-double textbook CG) at the
seams of the new tiling. An edge or a wall term dropped from delta moves alpha
by about 1e-6, a row or plane that feeds the sum without having been formed
by more, so the bar of the other seam tests sees either.

The cell form (CFD_HIP_CCF_EDGE_DOT=0: w = A r at every cell, 60 x 28 tiles,
today's Z-slab interior march) against the edge form on the same problems:
equal iteration counts, x within BAR x the distance moved, and whole steps of
both through the single-reduction gates against the oracle's textbook CG.
"""
import numpy as np
import pytest

from cfd_amd import _abi as A
from cfd_amd import api
from oracle import oracle
from tests import cg_reference as R
from tests import cg_seam_shapes as T

pytestmark = pytest.mark.gpu

CC = dict(cg_variant=1)
EDGE_TILE = (60, 29)   # ccf.hpp CCF_OX x CCF_OY_EDGE
CELL_TILE = R.CCF_TILE

# CFD_HIP_CCF_KC_FIXED=1: 24-plane runs. y seams after rows 28 and 57.
EDGE_FIXED = [
    ((60, 29, 26), "wall column 59 and wall row 28 close tile 0; 24 planes: exactly one run"),
    ((61, 30, 26), "last interior column 59 / row 28 close tile 0, the walls have no tile"),
    ((62, 31, 26), "one-column last x tile, one-row last y tile (interior 29 + wall 30)"),
    ((63, 32, 26), "last x tile: interior 60-61 + wall 62; last y tile: interior 29-30 + wall"),
    ((121, 59, 26), "second seams: last interior column 119 / row 57 close tile 1"),
    ((122, 60, 27), "one-column third x tile, one-row third y tile; runs 24 + 1"),
    ((60, 30, 27), "even nx clamp with the x wall on the seam; runs 24 + 1"),
    ((61, 29, 27), "odd nx clamp, wall row on the y seam; runs 24 + 1"),
    ((62, 32, 28), "one-column last x tile, two-row last y tile; runs 24 + 2"),
    ((63, 31, 28), "two-column last x tile, one-row last y tile; runs 24 + 2"),
    ((61, 30, 51), "49 planes: two runs + one plane (its +z edge is the top wall's)"),
    ((62, 31, 51), "one-column / one-row last tiles over two runs + one plane"),
    ((60, 59, 28), "x wall on the seam, two full y tiles; runs 24 + 2"),
    ((121, 29, 27), "x interior ends on the second seam, y wall on the first"),
    ((122, 32, 28), "three x tiles (one column), two y tiles (two rows); runs 24 + 2"),
    ((63, 60, 27), "one interior row in the third y tile; runs 24 + 1"),
    ((62, 59, 27), "one-column x tile, y interior ends on the second seam"),
    ((61, 31, 27), "x interior ends on the seam, one-row last y tile"),
    ((121, 31, 51), "two full x tiles over two runs + one plane"),
]
# the default kc (halved to 3 at these sizes)
EDGE_DEFAULT = [
    ((4, 4, 3), "the smallest legal grid: 2 x 2 x 1 interior cells, every edge a wall edge"),
    ((5, 4, 3), "odd nx at the smallest ny, nz"),
    ((4, 5, 4), "even nx, two interior planes"),
]
AB_SHAPES = [(62, 31, 28), (121, 59, 51)]


def test_shapes_cover_the_seams():
    fixed = [s for s, _ in EDGE_FIXED]
    assert {60, 61, 62, 63, 121, 122} == {s[0] for s in fixed}
    assert {29, 30, 31, 32, 59, 60} == {s[1] for s in fixed}
    assert {26, 27, 28, 51} == {s[2] for s in fixed}
    assert all(s[0] * s[1] * s[2] < T.MAX_CELLS for s in fixed)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ("CFD_HIP_CG_SMALL", "CFD_HIP_CCF_KC", "CFD_HIP_CCF_KC_FIXED", "CFD_HIP_CCF_TAIL",
              "CFD_HIP_CCF_KC2", "CFD_HIP_CCF", "CFD_HIP_CCF_EDGE_DOT", "CFD_HIP_CCF_XMAP"):
        monkeypatch.delenv(k, raising=False)


def _capped_solves(shape, what, tile, kc, iters_list=None, timed=False):
    """Every capped solve of `shape` on one context; all failures reported
    together. Returns {iters: (x, stats)}."""
    rhs, x0 = T.problem(shape)
    d = T.spacing(shape)
    fails, out = [], {}
    ctx = api.HipProjection(*shape, **CC)
    try:
        if timed:
            ctx.reset_timing()
            ctx.enable_timing(True)
        for iters in iters_list or T.iters_for(shape):
            x = x0.copy()
            s, st = ctx.poisson_solve(A.HIP_POISSON_CG, x, rhs, *d, T.capped_params(iters))
            out[iters] = (x, st)
            try:
                T.check_capped_solve(shape, iters, s, st, x, tile, kc, what)
            except AssertionError as e:
                fails.append(str(e))
        if timed:
            kt = ctx.timing()
            # the march ran (plain and fold launches), not k_cc1 / k_cg_small
            assert kt["cc_fused"][1] > 0 and kt["cc_fold"][1] > 0, (what, kt)
            assert kt["cc_update"][1] == 0 and kt["cg_small"][1] == 0, (what, kt)
    finally:
        ctx.close()
    assert not fails, "\n".join(fails)
    return out


@pytest.mark.parametrize("shape", [s for s, _ in EDGE_FIXED], ids=T.sid)
def test_edge_dot_24_plane_runs(hip_lib, monkeypatch, shape):
    monkeypatch.setenv("CFD_HIP_CCF_KC_FIXED", "1")
    _capped_solves(shape, "k_ccf edge sum kc 24", EDGE_TILE, 24)


@pytest.mark.parametrize("shape", [s for s, _ in EDGE_DEFAULT], ids=T.sid)
def test_edge_dot_default_runs(hip_lib, shape):
    _capped_solves(shape, "k_ccf edge sum default kc", EDGE_TILE, 3)


def test_edge_dot_path_taken(hip_lib, monkeypatch):
    """The default context runs the march (cc_fused and cc_fold launches) and
    its results hold with the timers on."""
    monkeypatch.setenv("CFD_HIP_CCF_KC_FIXED", "1")
    _capped_solves((62, 31, 28), "k_ccf edge sum timed", EDGE_TILE, 24, timed=True)


@pytest.mark.parametrize("shape", AB_SHAPES, ids=T.sid)
def test_cell_form_against_edge_form_capped(hip_lib, monkeypatch, shape):
    """8 capped iterations, 24-plane runs: both forms pass the reference's
    gates, count the same iterations and agree in x within BAR x moved."""
    monkeypatch.setenv("CFD_HIP_CCF_KC_FIXED", "1")
    got = {}
    for form, tile in (("0", CELL_TILE), ("1", EDGE_TILE)):
        monkeypatch.setenv("CFD_HIP_CCF_EDGE_DOT", form)
        got[form] = _capped_solves(shape, f"k_ccf EDGE_DOT={form}", tile, 24, iters_list=(8,),
                                   timed=True)[8]
    (x0_, st0), (x1_, st1) = got["0"], got["1"]
    assert st0.iterations == st1.iterations == 8
    moved = T.reference(shape)[8].moved
    dev = float(np.max(np.abs(x1_ - x0_))) / float(moved)
    print(f"EDGE_DOT 0 vs 1 {T.sid(shape)}: x {dev:.3e}")
    assert dev <= T.BAR, R.worst_cell(x1_, x0_, EDGE_TILE, 24)


@pytest.mark.parametrize("shape", AB_SHAPES, ids=T.sid)
def test_cell_form_against_edge_form_steps(hip_lib, monkeypatch, shape):
    """Two whole steps from random fields in both forms, each through the
    single-reduction gates against the oracle's textbook CG (iterations +-2,
    u, v, w within 1e-6, demeaned p within 1e-5); the two forms stop after the
    same iteration counts."""
    g, f0, p = T.step_case(shape)
    fo = api.FlowField(g.nx, g.ny, g.nz)
    fo.copy_from(f0)
    want = []
    for step in range(2):
        so, _, io = oracle.projection_step(fo, g, p)
        assert so == A.CFD_SUCCESS
        want.append(io)
    counts = {}
    for form in ("0", "1"):
        monkeypatch.setenv("CFD_HIP_CCF_EDGE_DOT", form)
        f = api.FlowField(g.nx, g.ny, g.nz)
        f.copy_from(f0)
        ctx = api.HipProjection(g.nx, g.ny, g.nz, **CC)
        its = []
        try:
            for step in range(2):
                assert ctx.step(f, g, p) == A.CFD_SUCCESS, api._native.last_error()
                its.append(ctx.poisson_stats().iterations)
                assert abs(its[-1] - want[step]) <= 2, (form, step, its, want)
        finally:
            ctx.close()
        counts[form] = its
        for k in ("u", "v", "w"):
            a, b = getattr(f, k), getattr(fo, k)
            assert float(np.max(np.abs(a - b))) / float(np.max(np.abs(b))) <= 1e-6, \
                (form, k, R.worst_cell(a, b, EDGE_TILE))
        dp = (f.p - f.p.mean()) - (fo.p - fo.p.mean())
        assert float(np.max(np.abs(dp))) / float(np.max(np.abs(fo.p))) <= 1e-5, (form, "p")
    print(f"EDGE_DOT steps {T.sid(shape)}: iterations {counts} oracle {want}")
    assert counts["0"] == counts["1"], counts
