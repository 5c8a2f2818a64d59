"""The case table of the k_rb2 interior-tile tests (tests/rb2_shapes.py) and
its reference side, proved without a GPU:

  - the gap: under the product's run-length rule every shape of
    test_gpu_rb2.SHAPES marches runs of at most 4 planes, with no steady
    (ZB = false) step and no interior (BND = false) tile;
  - the table: every case has an interior tile (the control has none) and a
    run with a steady group of four; over the table the tail takes all four
    residues and the runs start at plane 1, end at plane nz - 2, and do neither;
  - the tolerance cases stop converged in the oracle below their cap, at one
    odd and one even count each;
  - the interior-peak problem: the L-inf residual of every iterate up to the
    stop sits inside the amplified block, which only the interior tile's
    steady steps see.
"""
import ast
from pathlib import Path

import numpy as np
import pytest

from cfd_amd import _abi as A
from oracle import oracle
from tests import cg_reference
from tests import cg_seam_shapes
from tests import rb2_shapes as T


def _old_shapes():
    """test_gpu_rb2.SHAPES, read from the source (importing the module needs
    nothing of the GPU, but keeps this file independent of its fixtures)."""
    src = (Path(__file__).parent / "test_gpu_rb2.py").read_text()
    for node in ast.parse(src).body:
        if isinstance(node, ast.Assign) and node.targets[0].id == "SHAPES":
            return sorted({tuple(e.value for e in item.elts[0].elts) for item in node.value.elts})
    raise AssertionError("test_gpu_rb2.SHAPES not found")


def test_the_gap_in_the_existing_shapes():
    shapes = _old_shapes() + [(96, 80, 70), (70, 66, 40), (96, 96, 48)]
    assert len(shapes) >= 10
    for shape in shapes:
        lay = T.layout(shape, fixed=False)
        assert lay.kc <= 4, (shape, lay.kc)
        assert all(r.steady_fours == 0 for r in lay.runs), shape
        assert lay.interior == [], shape


def test_layout_restates_the_march():
    # the shortest run with a steady group has 9 planes
    assert T.march(1, 9).steady_fours == 0 and T.march(1, 10).steady_fours == 1
    assert T.march(5, 13).steady_fours == 0 and T.march(5, 14).steady_fours == 1
    # 118 x 54 is the smallest grid with an interior tile
    assert T.layout((118, 54, 20)).interior == [(1, 1)]
    assert T.layout((117, 54, 20)).interior == [] and T.layout((118, 53, 20)).interior == []
    # the halving loop: the product's layout of two shapes the suite runs
    assert T.layout((250, 30, 40), fixed=False).kc == 4
    assert T.layout((1024, 1024, 512), fixed=False).kc == 170
    # the steps of every run add up
    for c in T.CASES:
        for r in T.layout(c.shape, c.kc).runs:
            assert 0 <= r.tail_steps <= 3 and (r.ke - r.kb + 6 - r.tail_steps) % 4 == 0


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.id)
def test_case_reaches_the_steady_interior_path(case):
    lay = T.layout(case.shape, case.kc)
    assert (lay.tiles_x, lay.tiles_y) == ((4, 4) if case.shape[0] == 178 else (3, 3))
    if case is T.CONTROL:
        assert lay.interior == []
        assert lay[:3] == T.layout(T.CASES[0].shape)[:3]  # the same tiling
    else:
        assert len(lay.interior) >= 1
    assert any(r.steady_fours > 0 for r in lay.runs)
    assert sum(r.ke - r.kb for r in lay.runs) == case.shape[2] - 2
    assert case.shape[0] * case.shape[1] * case.shape[2] <= 940_000


def test_table_covers_tails_run_positions_and_seams():
    lays = {c.id: T.layout(c.shape, c.kc) for c in T.CASES}
    steady = [r for lay in lays.values() for r in lay.runs if r.steady_fours]
    assert {r.tail_steps for r in steady} == {0, 1, 2, 3}
    nz_of = {c.id: c.shape[2] for c in T.CASES}
    pos = {(r.kb == 1, r.ke == nz_of[cid] - 1) for cid, lay in lays.items() for r in lay.runs
           if r.steady_fours}
    assert pos >= {(True, True), (True, False), (False, False)}
    # the four shortest steady runs, with their remainder runs
    for kc, tail, rem in ((9, 3, 2), (10, 0, 8), (11, 1, 5), (12, 2, 2)):
        runs = lays[f"122x58x40-kc{kc}"].runs
        assert [r.ke - r.kb for r in runs[:-1]] == [kc] * (len(runs) - 1)
        assert all(r.steady_fours == 1 and r.tail_steps == tail for r in runs[:-1])
        assert runs[-1].ke - runs[-1].kb == rem and runs[-1].steady_fours == 0
    assert [r.steady_fours for r in lays["122x58x30"].runs] == [5]
    assert lays["122x58x30"].runs[0].tail_steps == 2
    assert [(r.ke - r.kb, r.steady_fours) for r in lays["178x82x30-kc13"].runs] == \
        [(13, 2), (13, 2), (2, 0)]
    assert lays["178x82x30-kc13"].interior == [(1, 1), (2, 1), (1, 2), (2, 2)]
    assert [r.ke - r.kb for r in lays["122x58x132"].runs] == [128, 2]
    assert lays["123x59x30"][:4] == lays["122x58x30"][:4]


def test_host_launches_restates_the_loop():
    # capped: sweeps s = 1, 3, ... <= cap
    assert T.host_launches(6, 6) == (1, 3) and T.host_launches(7, 7) == (1, 4)
    # the first chunk launches iterates 0 .. 8, the second 9 .. 24; a stop is
    # seen one chunk late
    assert T.host_launches(8, 400) == (1, 4 + 8)
    assert T.host_launches(9, 400) == (1, 4 + 8 + 16)
    assert T.host_launches(2, 3) == (1, 2)


def test_spacings_keep_the_fast_division_eligible():
    for c in T.CASES:
        dx, dy, dz = T.spacing(c.shape)
        assert len({dx, dy, dz}) == 3 and max(dx, dy, dz) < 1.0
        assert 1.0 <= 1.0 / (dx * dx) <= 2.0 ** 60 and 1.0 <= 1.0 / (dy * dy) <= 2.0 ** 60


@pytest.mark.parametrize("case,tols", T.TOL_CASES, ids=lambda v: getattr(v, "id", None))
def test_tolerance_cases_stop_on_both_parities(case, tols):
    counts = []
    for tol in tols:
        s, st, x = T.oracle_solve(case.shape, False, ("tol", tol))
        assert s == A.CFD_SUCCESS and st.status == A.POISSON_CONVERGED
        assert 2 <= st.iterations < 40 < T.TOL_CAP
        counts.append(st.iterations)
    assert {n % 2 for n in counts} == {0, 1}, counts


def test_capped_solves_stop_at_their_cap():
    shape = T.CASES[0].shape
    for cap in T.CAPS:
        s, st, x = T.oracle_solve(shape, False, ("cap", cap))
        assert s == A.CFD_ERROR_MAX_ITER and st.status == A.POISSON_MAX_ITER
        assert st.iterations == cap + 1
        assert st.final_residual > 1.0  # nowhere near a bound of order 1e-9


def test_interior_peak_residual_lies_in_the_steady_block():
    shape = T.PEAK_CASE.shape
    rhs, x0 = T.problem(shape, True)
    plain_rhs, plain_x0 = T.problem(shape, False)
    outside = np.ones(rhs.shape, bool)
    outside[T.PEAK_BLOCK] = False
    assert np.array_equal(rhs[outside], plain_rhs[outside])
    assert np.array_equal(rhs[T.PEAK_BLOCK], T.PEAK_GAIN * plain_rhs[T.PEAK_BLOCK])
    assert np.array_equal(x0[T.PEAK_BLOCK], T.PEAK_GAIN * plain_x0[T.PEAK_BLOCK])
    # the block is the centre tile's owned cells, and its planes those whose
    # residuals both iterates of a sweep form in steady steps
    (tx, ty), = T.layout(shape).interior
    kk, jj, ii = T.PEAK_BLOCK
    assert (ii.start, ii.stop) == (tx * T.OX, tx * T.OX + T.OX)
    assert (jj.start, jj.stop) == (ty * T.OY, ty * T.OY + T.OY)
    run, = T.layout(shape).runs
    q_lo, q_hi = run.kb - 4 + 8, run.kb - 4 + 8 + 4 * run.steady_fours - 1  # steady steps
    assert (kk.start, kk.stop - 1) == (q_lo + 1, q_hi - 1)
    stops = []
    for tol in T.PEAK_TOLS:
        s, st, _ = T.oracle_solve(shape, True, ("tol", tol))
        assert s == A.CFD_SUCCESS and st.status == A.POISSON_CONVERGED
        stops.append(st.iterations)
    assert {n % 2 for n in stops} == {0, 1}, stops
    inner = tuple(slice(s.start - 1, s.stop - 1) for s in T.PEAK_BLOCK)  # interior indexing
    for it in range(0, max(stops) + 1):
        if it == 0:
            x = x0.copy()
            cg_reference.neumann_shell(x)
        else:
            _, st, x = T.oracle_solve(shape, True, ("cap", it))
        r = T.residual_abs(x, rhs, shape)
        if it:
            assert float(r.max()) == pytest.approx(st.final_residual, rel=1e-9)
        am = np.unravel_index(int(np.argmax(r)), r.shape)
        assert all(s.start <= v < s.stop for s, v in zip(inner, am)), (it, am)
        masked = r.copy()
        masked[inner] = 0.0
        assert float(r.max()) > 1.05 * float(masked.max()), it  # not a near tie


def test_locate_names_tile_run_and_step():
    case = T.CASES[5]  # 122 x 58 x 40, 10-plane runs
    msg = T.locate((17, 30, 60), case)
    # plane 17 is in run 1 = [11, 21): stored in step q = 19, n = 19 - 7 = 12
    assert "(tx, ty) = (1, 1) interior" in msg and "run 1 [11, 21) step 12 of 16 (ZB)" in msg
    assert "step 9 of 16 (steady)" in T.locate((14, 30, 60), case)
    assert "(tx, ty) = (0, 2) boundary" in T.locate((0, 57, 0), case)
    a = np.zeros(case.shape[::-1])
    b = a.copy()
    assert T.first_diff(a, b, case) is None
    b[14, 30, 60] = 1.0
    b[20, 5, 5] = 1.0
    assert "2 cells differ, first (k, j, i) = (14, 30, 60)" in T.first_diff(a, b, case)


def test_rb_sor_steps_converge_in_oracle():
    g, f, p = cg_seam_shapes.step_case(T.STEP_SHAPE)
    oracle.set_projection_poisson_params(oracle.poisson_params(**T.STEP_RELAX))
    try:
        for _ in range(2):
            s, _, it = oracle.projection_step(f, g, p, A.ORACLE_POISSON_REDBLACK)
            assert s == A.CFD_SUCCESS
            assert oracle.last_poisson_stats().status == A.POISSON_CONVERGED
            assert 10 < it < 2000, it
    finally:
        oracle.set_projection_poisson_params(None)
    for k in ("u", "v", "w", "p"):
        assert np.isfinite(getattr(f, k)).all()
