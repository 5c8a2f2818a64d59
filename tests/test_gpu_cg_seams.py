"""The CG kernels on random data at tile-seam shapes (tests/cg_seam_shapes.py),
against a long-double textbook CG (tests/cg_reference.py).

Every other CG test solves smooth, mirror-symmetric data from x0 = 0 at
shapes that keep walls and last columns away from the tile seams. Here the
right-hand side is N(0, 1), the initial iterate 0.1 N(0, 1) with its own
Neumann shell, dx != dy != dz, and the shapes put the wall, the last interior
column / row / plane and one-cell last tiles on the seams of

  k_ccf (cg_variant 1)     60 x 29 x kc tiles on one device, 60 x 28 x kc on
                           slabs (cg_seam_shapes.CCF_FIXED says which seams
                           that leaves here), 24-plane runs + short remainder
                           runs, the smallest legal grids
  k_cgA / k_cgB            128 x 8 and 128 x 16 tiles, a kchunk remainder run
  k_cg_small               the same shapes, a ragged last workgroup, the
                           largest grid that takes it
  k_cc1 / k_cc2            2-D single-reduction CG
  k_cg_setup               a nonzero x0 and its shell in r_0 (all of the above)
  k_pred3 / k_corr3        whole steps from random fields, 128 x 16 tiles

Capped solves (1, 3, 4, 5, 8 iterations: every residue of the fold period of
4): status MAX_ITER, the exact count, both residual norms within 1e-11
relative and max |x - x_ref| <= 1e-11 max |x_ref - x0|, shell included. The
oracle's textbook CG stays within 3.9e-14 of the reference on these problems
(test_cg_reference.py); the kernels differ from it only in how the dot
products are grouped (and, for cg_variant 1, in the recurrence for alpha and
beta), so rounding does not force a looser bar. One interior cell dropped
from a dot product moves alpha by about 1e-6.

Largest max |x - x_ref| / max |x_ref - x0| measured on an MI355X over every
shape and count, per kernel family (bar 1e-11):
  k_ccf, 24-plane runs 1.2e-15, default runs 5.7e-16; k_cgA / k_cgB 2.8e-15
  (8 and 16 rows; kchunk remainder 1.4e-15); k_cg_small 2.6e-15; k_cc1 / k_cc2
  2-D 1.1e-15; Z-slabs 7.9e-16 (textbook) and 8.2e-16 (single reduction);
  residual norms at most 6.5e-15 relative. Steps: textbook CG fields within
  3.6e-15 (bar 1e-10), cg_variant 1's r_0 within 5.8e-15 on both steps.

Whole steps from random u, v, w, p: the Jacobi route bitwise the oracle's
(k_pred3, k_corr3, the relaxation right-hand side, the shell kernels), the
textbook CG route through test_gpu_parity's gates, cg_variant 1 through the
single-reduction gates plus the Poisson initial residual (k_cg_setup's fused
right-hand side) within 1e-12 of the oracle's.

Z-slabs (in-process groups of 2 and 3 ranks): the same capped gates for both
CG forms against the one long-double reference, and the side-stream edge
launch of k_ccf (CFD_HIP_CCF_EDGE_SIDE) bitwise against the in-order form.
"""
import numpy as np
import pytest

from cfd_amd import _abi as A
from cfd_amd import api
from oracle import oracle
from tests import cg_reference as R
from tests import cg_seam_shapes as T
from tests.test_gpu_parity import CG_FIELD_RTOL, _rel_maxdiff, _step_both
from tests.test_gpu_slabs import FIELDS, Slabs, _run_steps, _slab_poisson

pytestmark = pytest.mark.gpu

CC = dict(cg_variant=1)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ("CFD_HIP_CG_SMALL", "CFD_HIP_CCF_KC", "CFD_HIP_CCF_KC_FIXED", "CFD_HIP_CCF_TAIL",
              "CFD_HIP_CCF_KC2", "CFD_HIP_CCF_EDGE_SIDE", "CFD_HIP_CCF"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("CFD_HIP_GROUP_TIMEOUT_S", "60")


def _capped_solves(shape, what, tile, kc=None, timers=None, **cfg):
    """Every capped solve of `shape` on one context; all failures reported
    together. timers: {name: wanted} launch counts > 0 (True) or == 0."""
    rhs, x0 = T.problem(shape)
    d = T.spacing(shape)
    fails = []
    ctx = api.HipProjection(*shape, **cfg)
    try:
        if timers:
            ctx.reset_timing()
            ctx.enable_timing(True)
        for iters in T.iters_for(shape):
            x = x0.copy()
            s, st = ctx.poisson_solve(A.HIP_POISSON_CG, x, rhs, *d, T.capped_params(iters))
            try:
                T.check_capped_solve(shape, iters, s, st, x, tile, kc, what)
            except AssertionError as e:
                fails.append(str(e))
        if timers:
            kt = ctx.timing()
            for name, want in timers.items():
                assert (kt[name][1] > 0) == want, (what, name, kt[name])
    finally:
        ctx.close()
    assert not fails, "\n".join(fails)


# ---- item 3: the operator at the seams --------------------------------------

@pytest.mark.parametrize("shape", [s for s, _ in T.CCF_FIXED], ids=T.sid)
def test_ccf_24_plane_runs(hip_lib, monkeypatch, shape):
    monkeypatch.setenv("CFD_HIP_CCF_KC_FIXED", "1")
    _capped_solves(shape, "k_ccf kc 24", R.CCF_EDGE_TILE, 24, **CC)


@pytest.mark.parametrize("shape", [s for s, _ in T.CCF_DEFAULT], ids=T.sid)
def test_ccf_default_runs(hip_lib, shape):
    _capped_solves(shape, "k_ccf default kc", R.CCF_EDGE_TILE, 3, **CC)


@pytest.mark.parametrize("rows", [8, 16])
@pytest.mark.parametrize("shape", [s for s, _ in T.TEXTBOOK], ids=T.sid)
def test_textbook_sweeps(hip_lib, monkeypatch, shape, rows):
    monkeypatch.setenv("CFD_HIP_CG_SMALL", "0")
    _capped_solves(shape, f"k_cgA/B rows {rows}", (128, rows), sweep_rows=rows)


@pytest.mark.parametrize("rows", [8, 16])
@pytest.mark.parametrize("shape,kchunk", [(s, k) for s, k, _ in T.TEXTBOOK_KCHUNK])
def test_textbook_sweeps_kchunk_remainder(hip_lib, monkeypatch, shape, kchunk, rows):
    monkeypatch.setenv("CFD_HIP_CG_SMALL", "0")
    _capped_solves(shape, f"k_cgA/B rows {rows} kchunk {kchunk}", (128, rows), kchunk,
                   sweep_rows=rows, kchunk=kchunk)


@pytest.mark.parametrize("shape", [s for s, _ in T.TEXTBOOK + T.SMALL_ONLY], ids=T.sid)
def test_cg_small(hip_lib, shape):
    _capped_solves(shape, "k_cg_small", (128,))


@pytest.mark.parametrize("shape", [s for s, _ in T.CC_2D], ids=T.sid)
def test_single_reduction_2d(hip_lib, shape):
    _capped_solves(shape, "k_cc1/k_cc2", (128, 16), **CC)


def test_paths_taken(hip_lib, monkeypatch):
    """The cases above run the kernels they name: launch counts of one timed
    context per family (timing changes no result; the gates hold here too)."""
    _capped_solves((62, 30, 27), "k_ccf timed", R.CCF_EDGE_TILE, 3,
                   timers={"cc_fused": True, "cc_fold": True, "cc_update": False,
                           "cg_sweep_a": False, "cg_small": False}, **CC)
    _capped_solves((62, 30, 1), "k_cc1/k_cc2 timed", (128, 16),
                   timers={"cc_update": True, "cc_spmv": True, "cc_fused": False,
                           "cg_small": False}, **CC)
    _capped_solves((101, 102, 32), "k_cg_small timed", (128,),
                   timers={"cg_small": True, "cg_sweep_a": False, "cg_sweep_b": False})
    _capped_solves((41, 37, 5), "k_cg_small timed", (128,),
                   timers={"cg_small": True, "cg_sweep_a": False})
    monkeypatch.setenv("CFD_HIP_CG_SMALL", "0")
    _capped_solves((130, 18, 7), "k_cgA/B timed", (128, 16),
                   timers={"cg_small": False, "cg_sweep_a": True, "cg_sweep_b": True,
                           "cg_sweep_bx": True}, sweep_rows=16)


# ---- item 4: whole steps from random fields ---------------------------------

STEP_IDS = [T.sid(s) for s, _ in T.STEP_SHAPES]


def _fields_msg(fh, fo, k):
    return k + ": " + R.worst_cell(getattr(fh, k), getattr(fo, k), R.PC3_TILE)


@pytest.mark.parametrize("shape", [s for s, _ in T.STEP_SHAPES], ids=STEP_IDS)
def test_steps_jacobi_bitwise(hip_lib, shape):
    """No summation anywhere on the Jacobi route: u, v, w, p and the iteration
    counts (asserted equal in _step_both) are the oracle's, bit for bit."""
    g, f, p = T.step_case(shape)
    oracle.set_projection_poisson_params(oracle.poisson_params(**T.JACOBI))
    try:
        fo, fh = _step_both(g, f, p, 2, method=A.HIP_POISSON_JACOBI,
                            poisson_tolerance=T.JACOBI["tolerance"],
                            poisson_max_iter=T.JACOBI["max_iterations"])
    finally:
        oracle.set_projection_poisson_params(None)
    for k in ("u", "v", "w", "p"):
        a, b = getattr(fh, k), getattr(fo, k)
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), _fields_msg(fh, fo, k)


@pytest.mark.parametrize("small", [None, "0"], ids=["cg_small", "sweeps"])
@pytest.mark.parametrize("shape", [s for s, _ in T.STEP_SHAPES], ids=STEP_IDS)
def test_steps_textbook_cg(hip_lib, monkeypatch, shape, small):
    if small is not None:
        monkeypatch.setenv("CFD_HIP_CG_SMALL", small)
    g, f, p = T.step_case(shape)
    fo, fh = _step_both(g, f, p, 2)
    for k in ("u", "v", "w", "p"):
        rel = _rel_maxdiff(getattr(fh, k), getattr(fo, k))
        print(f"SEAM step textbook {T.sid(shape)} {k}: {rel:.3e}")
        assert rel <= CG_FIELD_RTOL, _fields_msg(fh, fo, k)


@pytest.mark.parametrize("shape", [s for s, _ in T.STEP_SHAPES], ids=STEP_IDS)
def test_steps_single_reduction(hip_lib, shape):
    """cg_variant 1 against the oracle's textbook CG: the single-reduction
    gates (iterations +-2, u, v, w within 1e-6, demeaned p within 1e-5) and
    the Poisson initial residual within 1e-12 relative: k_cg_setup's fused
    right-hand side and r_0 from a random p with its shell. The first step's
    inputs are identical; the second step's are the same Krylov iterate to
    rounding as long as both solvers stopped after the same count (measured:
    they do at every shape, r_0 within 5.8e-15 on both steps). Had they
    stopped one iteration apart, the fields would differ by what the 1e-6
    stopping tolerance allows and r_0 with them: then it is only printed."""
    g, f, p = T.step_case(shape)
    fo = api.FlowField(g.nx, g.ny, g.nz)
    fo.copy_from(f)
    ctx = api.HipProjection(g.nx, g.ny, g.nz, **CC)
    same = True
    try:
        for step in range(2):
            assert ctx.step(f, g, p) == A.CFD_SUCCESS, api._native.last_error()
            sth = ctx.poisson_stats()
            so, _, io = oracle.projection_step(fo, g, p)
            assert so == A.CFD_SUCCESS
            sto = oracle.last_poisson_stats()
            assert abs(sth.iterations - io) <= 2, (step, sth.iterations, io)
            rel = abs(sth.initial_residual - sto.initial_residual) / sto.initial_residual
            print(f"SEAM step cc {T.sid(shape)} step {step}: res0 {rel:.3e} "
                  f"iterations {sth.iterations} / {io}")
            if same:
                assert rel <= 1e-12, (step, sth.initial_residual, sto.initial_residual)
            same = same and sth.iterations == io
    finally:
        ctx.close()
    for k in ("u", "v", "w"):
        a, b = getattr(f, k), getattr(fo, k)
        assert float(np.max(np.abs(a - b))) / float(np.max(np.abs(b))) <= 1e-6, _fields_msg(f, fo, k)
    dp = (f.p - f.p.mean()) - (fo.p - fo.p.mean())
    assert float(np.max(np.abs(dp))) / float(np.max(np.abs(fo.p))) <= 1e-5, _fields_msg(f, fo, "p")


# ---- item 5: Z-slabs ---------------------------------------------------------

class _Spacing:
    """What _slab_poisson and Slabs read of a grid."""

    def __init__(self, shape):
        self.nx, self.ny, self.nz = shape
        self.dx, self.dy, self.dz = T.spacing(shape)


@pytest.mark.parametrize("cgv", [0, 1], ids=["textbook", "single_reduction"])
@pytest.mark.parametrize("shape,nranks,spans", [c[:3] for c in T.SLAB_CASES])
def test_slab_capped_solves(hip_lib, shape, nranks, spans, cgv):
    """Slabs of >= 3 planes split into the edge launch and the interior march;
    shorter ones run the whole march, then a blocking r halo."""
    assert tuple(api.slab_layout(shape[2], r, nranks)[1] - 2 for r in range(nranks)) == spans
    rhs, x0 = T.problem(shape)
    fails = []
    for iters in T.iters_for(shape):
        stats = []
        stat, its, x = _slab_poisson(_Spacing(shape), rhs, nranks, A.HIP_POISSON_CG,
                                     T.capped_params(iters), x0=x0, stats=stats, cg_variant=cgv)
        for r in range(nranks):
            try:
                T.check_capped_solve(shape, iters, stat[r], stats[r], x,
                                     R.CCF_TILE if cgv else (128, 16), None,
                                     f"slabs {nranks} rank {r} cg_variant {cgv}")
            except AssertionError as e:
                fails.append(str(e))
    assert not fails, "\n".join(fails)


def test_ccf_edge_side_stream_is_bitwise_neutral(hip_lib, monkeypatch):
    """The edge planes' march of k_ccf on the side stream, beside the interior
    march (CFD_HIP_CCF_EDGE_SIDE, default 1), against the in-order form (0):
    the two launches write disjoint planes, so 8 capped iterations from
    random data and three steps from random fields are bitwise equal."""
    shape, nranks = (62, 30, 27), 3
    rhs, x0 = T.problem(shape)
    out = {}
    for side in ("0", "1"):
        monkeypatch.setenv("CFD_HIP_CCF_EDGE_SIDE", side)
        stat, its, x = _slab_poisson(_Spacing(shape), rhs, nranks, A.HIP_POISSON_CG,
                                     T.capped_params(8), x0=x0, **CC)
        assert its == [8] * nranks and all(s == A.CFD_ERROR_MAX_ITER for s in stat)
        g, f, p = T.step_case(shape)
        S = Slabs(g, nranks, **CC)
        try:
            S.scatter(f)
            hist = _run_steps(S, g, p, 3, lambda c: None)
            got = {k: S.gather(k) for k in FIELDS}
        finally:
            S.close()
        out[side] = (x, hist, got)
    assert np.array_equal(out["0"][0].view(np.uint64), out["1"][0].view(np.uint64)), \
        R.worst_cell(out["1"][0], out["0"][0], R.CCF_TILE)
    assert out["0"][1] == out["1"][1]
    for k in FIELDS:
        a, b = out["0"][2][k], out["1"][2][k]
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), \
            k + ": " + R.worst_cell(b, a, R.CCF_TILE)
