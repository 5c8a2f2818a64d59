"""The long-double CG reference (tests/cg_reference.py), the seam shape table
(tests/cg_seam_shapes.py) and the 1e-11 bar of the GPU seam tests
(test_gpu_cg_seams.py), proved sound without a GPU:

  - at every shape of the table and every capped iteration count the oracle's
    textbook cg_solve (plain double, sequential dot products) passes the very
    gates the HIP kernels must pass: status, count, both residual norms and x
    with its shell within 1e-11 of the reference;
  - the reference's recurrence residual is the residual of its own x (inside
    the shell the solve ran with);
  - the Jacobi projection steps the GPU test pins bitwise converge in the
    oracle at every step shape.
"""
import numpy as np
import pytest

from cfd_amd import _abi as A
from oracle import oracle
from tests import cg_reference
from tests import cg_seam_shapes as T


def test_long_double_is_extended():
    assert np.finfo(np.longdouble).eps < 2e-16


def test_table_covers_the_seams():
    """The values the tiles' geometry asks for are all in the table, no grid
    is large, and the k_cg_small extras are what their lines say."""
    ccf = [s for s, _ in T.CCF_FIXED]
    assert {60, 61, 62, 63, 121, 122} <= {s[0] for s in ccf}
    assert {28, 29, 30, 31, 57, 58} <= {s[1] for s in ccf}
    assert {26, 27, 28, 51} == {s[2] for s in ccf}
    assert {(4, 4, 3), (5, 4, 3), (4, 5, 4)} <= {s for s, _ in T.CCF_DEFAULT}
    tb = [s for s, _ in T.TEXTBOOK]
    assert {127, 128, 129, 130} == {s[0] for s in tb}
    assert {15, 16, 17, 18, 33} == {s[1] for s in tb}
    assert {1, 7} <= {s[2] for s in tb}
    for s, kchunk, _ in T.TEXTBOOK_KCHUNK:
        assert (s[2] - 2) % kchunk != 0
    inner = [(s[0] - 2) * (s[1] - 2) * (s[2] - 2) for s, _ in T.SMALL_ONLY]
    assert inner[0] % 256 != 0
    assert 0.98 * T.CG_SMALL_CELLS <= inner[1] < T.CG_SMALL_CELLS
    for s in T.all_poisson_shapes() + [s for s, _ in T.STEP_SHAPES]:
        assert s[0] * s[1] * s[2] <= T.MAX_CELLS, s
    assert {s for s, _ in T.STEP_SHAPES} == {(130, 18, 7), (129, 17, 5), (127, 33, 6),
                                             (61, 30, 27), (62, 58, 27)}


@pytest.mark.parametrize("shape", T.all_poisson_shapes(), ids=T.sid)
def test_oracle_cg_within_bar_of_reference(shape):
    rhs, x0 = T.problem(shape)
    worst = 0.0
    for iters in T.iters_for(shape):
        x = x0.copy()
        s, st = oracle.cg_solve(x, rhs, *T.spacing(shape), T.capped_params(iters))
        worst = max(worst, T.check_capped_solve(shape, iters, s, st, x, (1 << 30,),
                                                what="oracle"))
    print(f"oracle vs long double {T.sid(shape)}: {worst:.3e}")
    # the bar keeps a decade above the oracle's own deviation for the GPU's
    # regrouped dot products
    assert worst <= 1e-12


@pytest.mark.parametrize("shape", [(122, 58, 27), (63, 31, 26), (130, 18, 7), (129, 17, 1),
                                   (4, 4, 3)], ids=T.sid)
def test_reference_residual_is_its_own(shape):
    rhs, x0 = T.problem(shape)
    d = T.spacing(shape)
    for iters in T.iters_for(shape):
        ref = T.reference(shape)[iters]
        true = cg_reference.true_residual(ref.x, x0, rhs, *d)
        assert float(np.max(np.abs(ref.r - true))) <= 1e-15 * float(np.max(np.abs(true))), \
            (shape, iters)
        assert float(ref.residuals[iters]) == pytest.approx(
            float(np.sqrt(np.sum(true * true))), rel=1e-13)


def test_reference_one_run_equals_capped_runs():
    shape = (61, 29, 7)
    rhs, x0 = T.problem(shape)
    many = T.reference(shape)
    one = cg_reference.cg_reference(x0, rhs, *T.spacing(shape), 4)
    assert np.array_equal(one.x, many[4].x) and one.residuals == many[4].residuals


def test_worst_cell_names_the_tile():
    a = np.zeros((9, 60, 130))
    b = a.copy()
    b[5, 29, 121] = 1.0
    msg = cg_reference.worst_cell(a, b, cg_reference.CCF_TILE, kc=3)
    assert "(5, 29, 121)" in msg and "x tile 2 + 1 of 60" in msg
    assert "y tile 1 + 1 of 28" in msg and "z run 1 + 1 of 3" in msg


@pytest.mark.parametrize("shape", [s for s, _ in T.STEP_SHAPES], ids=T.sid)
def test_jacobi_steps_converge_in_oracle(shape):
    g, f, p = T.step_case(shape)
    oracle.set_projection_poisson_params(oracle.poisson_params(**T.JACOBI))
    try:
        for _ in range(2):
            s, _, it = oracle.projection_step(f, g, p, A.ORACLE_POISSON_JACOBI)
            assert s == A.CFD_SUCCESS
            assert oracle.last_poisson_stats().status == A.POISSON_CONVERGED
            assert 10 < it < 1000, it
    finally:
        oracle.set_projection_poisson_params(None)
    for k in ("u", "v", "w", "p"):
        assert np.isfinite(getattr(f, k)).all()
