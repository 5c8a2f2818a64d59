"""The inputs of tests/special_values.py have teeth: on the oracle alone (no
GPU), every regime runs a whole Jacobi-route step to CFD_SUCCESS with finite
outputs, and its quotients lie on the sides of the fast-division range
[2^-900, 2^900] that the GPU tests need (at least a tenth of the interior
cells on either side, per division class). These shares are conditions the
exponent windows were tuned to, not measurements of the code under test.

Observed (percent of the interior cells: below / in range / above; the three
velocity fields together; 130x18x7, 127x33x6, 129x17x1 differ by 1-8 points):
  tiny       d/dx 75/25/0   d/dy 85/15/0   d2/dx2 29/71/0  d2/dy2 47/53/0
             dp/dx 75/25/0  dp/dy 85/15/0  (the solve stops at 0 iterations)
  subnormal  every class 100/0/0
  huge       d/dx 0/72/28   d/dy 0/83/17   d2/dx2 0/23/77  d2/dy2 0/42/58
             dp/dx 0/11/89  dp/dy 0/9/91   (118-203 Jacobi iterations, max |p|
             1e273)
  planted    d/dx 0/83/17   d/dy 0/83/17   d2/dx2 0/75/25  d2/dy2 0/75/25
  signed_zero  49 % of the first and 34 % of the second differences are zeros;
             the output holds 2092-2214 (130x18x7), 3340-3406 (127x33x6) cells
             of each zero sign per velocity field, all of them in the shell
             (no interior cell of the output is a zero: the pressure gradient
             is nowhere zero). The 2-D shape's shell has only 288 cells, of
             which 88-108 come out as each zero.
  nonfinite  2-3 % of the quotients non-finite; no non-finite output
Relaxation problems, share of the interior outside the range (below it for
tiny and subnormal, above it for huge) over the sweep's x and y classes and
the residual's, the four shapes and both caps:
             at x0     RB-SOR's last iterate   Jacobi's last iterate
  tiny x     25-53 %   19-44 %                 24-52 %
  tiny jk    51-56 %   35-47 %                 50-56 %
  subn. x    25-50 %   19-41 %                 23-47 %
  subn. jk   51-56 %   34-47 %                 50-55 %
  huge x     21-47 %   26-57 %                 21-48 %
  huge jk    43-50 %   49-66 %                 42-51 %
(the low ends are the 250- and 249-wide grids, whose ramp is in range between
its two crossings, columns 62 and 248)
"""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from cfd_amd import _abi as A
from oracle import oracle
from tests import cg_seam_shapes as T
from tests import special_values as S

ROOT = Path(__file__).resolve().parent.parent
SIDE = 0.10  # the issue's condition: a tenth of the interior cells on either side


def _oracle_step(regime, shape):
    g, f, p = S.step_fields(regime, shape)
    before = {k: getattr(f, k).copy() for k in S.FIELDS}
    oracle.set_projection_poisson_params(oracle.poisson_params(**T.JACOBI))
    try:
        s, st, it = oracle.projection_step(f, g, p, A.ORACLE_POISSON_JACOBI)
    finally:
        oracle.set_projection_poisson_params(None)
    return s, it, before, f


@pytest.mark.parametrize("shape", S.STEP_SHAPES, ids=T.sid)
@pytest.mark.parametrize("regime", S.REGIMES)
def test_step_inputs_reach_both_sides(regime, shape):
    s, it, before, f = _oracle_step(regime, shape)
    assert s == A.CFD_SUCCESS
    for k in S.FIELDS:
        assert np.isfinite(getattr(f, k)).all(), k
    pred = S.predictor_census(shape, before["u"], before["v"], before["w"])
    corr = S.corrector_census(shape, f.p)
    print(f"CENSUS {regime} {T.sid(shape)} iterations {it}: {S.fmt(pred)}; {S.fmt(corr)}")
    if regime in ("tiny", "huge", "planted"):
        for k, c in pred.items():
            assert S.outside(c) >= SIDE and c["in"] >= SIDE, (k, c)
    if regime == "tiny":
        for k, c in corr.items():
            assert S.outside(c) >= SIDE and c["in"] >= SIDE, (k, c)
    if regime == "huge":
        for k, c in corr.items():
            assert S.outside(c) >= SIDE, (k, c)
    if regime == "subnormal":
        for k, c in {**pred, **corr}.items():
            assert c["below"] >= 0.99, (k, c)
    if regime == "signed_zero":
        # 500 of each sign where the shell is large enough to hold them (3-D:
        # 6140 and 6511 shell cells, 35 % of them each zero). The 2-D shell
        # has 288 cells: 101 expected of each sign, standard deviation 8.
        need = 500 if shape[2] > 1 else 60
        for k in ("u", "v", "w")[:3 if shape[2] > 1 else 2]:
            a = getattr(f, k)
            neg = int(((a == 0.0) & np.signbit(a)).sum())
            pos = int(((a == 0.0) & ~np.signbit(a)).sum())
            print(f"CENSUS signed_zero {T.sid(shape)} {k}: {neg} x -0.0, {pos} x +0.0")
            assert neg >= need and pos >= need, (k, neg, pos)
        for k, c in pred.items():
            assert c["zero"] >= SIDE and c["in"] >= SIDE, (k, c)
    if regime == "nonfinite":
        for k in ("u", "v", "w"):
            a = before[k]
            assert not np.isfinite(S._interior(a)).all() and np.isfinite(before["p"]).all()
            shell = a.copy()
            S._interior(shell)[...] = 0.0
            assert np.isfinite(shell).all()
        for k, c in pred.items():
            assert c["above"] >= 0.01, (k, c)  # the non-finite quotients


@pytest.mark.parametrize("shape", S.STEP_SHAPES, ids=T.sid)
def test_planted_cells_sit_on_the_seams(shape):
    """The single cells are where the builder says, in waves (one row of one
    128-column tile) that hold nothing else out of the ordinary; one of them,
    at least, gives a wave exactly one lane (column pair) out of the range."""
    nx, ny, nz = shape
    g, f, p = S.step_fields("planted", shape)
    cells = S.planted_cells(shape)
    assert {c[2] for c in cells} == {c for c in (0, 1, 127, 128, nx - 2) if c < nx}
    assert {c[1] for c in cells} == {r for r in (15, 16, 17) if r < ny}
    assert not set(S.planted_rows(ny)) & {j + d for _, j, _, _ in cells for d in (-1, 0, 1)}
    dx = T.spacing(shape)[0]
    lone = 0
    for kk, j, i, _ in cells:
        if not (1 <= j <= ny - 2 and abs(f.u[kk, j, i]) == 2.0 ** 905):
            continue
        row = f.u[kk, j]
        with np.errstate(all="ignore"):
            q = np.abs((row[2:] - row[:-2]) * (1.0 / (2.0 * dx)))  # cells 1 .. nx - 2
        bad = np.flatnonzero(~((q >= S.LO) & (q <= S.HI))) + 1
        tile = i // 128
        lanes = {int(c) // 2 for c in bad if c // 128 == tile}
        lone += len(lanes) == 1
    assert lone >= 1


@pytest.mark.parametrize("shape", S.RELAX_SHAPES, ids=T.sid)
@pytest.mark.parametrize("kind,axis", S.RELAX_PROBLEMS)
def test_relax_inputs_keep_both_sides(kind, axis, shape):
    x0, rhs = S.relax_problem(kind, axis, shape)
    first = S.relax_census(shape, x0)
    for method in ("rb", "jacobi"):
        for cap in S.RELAX_CAPS:
            s, st, x = S.relax_oracle(method, kind, axis, shape, cap)
            assert s == A.CFD_ERROR_MAX_ITER and st.status == A.POISSON_MAX_ITER
            assert st.iterations == cap + 1  # linear_solver.c:472
            assert np.isfinite(x).all()
            assert np.isfinite(st.initial_residual) and np.isfinite(st.final_residual)
            last = S.relax_census(shape, x)
            print(f"CENSUS relax {kind} {axis} {T.sid(shape)} {method} cap {cap}: "
                  f"x0 {S.fmt(first)} | end {S.fmt(last)}")
            for census in (first, last):
                for k, c in census.items():
                    assert S.outside(c) >= SIDE and c["in"] >= SIDE, (method, cap, k, c)
            if kind == "huge":  # k_rb2 must refuse these (|v| > 2^800)
                assert float(np.max(np.abs(x0))) > 2.0 ** 800


def test_x_ramp_threshold_columns():
    """The x ramp crosses the range's lower end inside column pairs 30 .. 32
    of the first 124-column k_rb1 tile and, at nx = 250, again within two
    columns of the remainder strip (columns 248, 249)."""
    for kind in ("tiny", "subnormal"):
        for shape in ((130, 20, 9), (250, 21, 10)):
            x0, _ = S.relax_problem(kind, "x", shape)
            dx = T.spacing(shape)[0]
            q = np.abs((x0[1:-1, 1:-1, 2:] + x0[1:-1, 1:-1, :-2]) * (1.0 / (dx * dx)))
            low = (q < S.LO).mean(axis=(0, 1))  # per column 1 .. nx - 2
            cols = np.flatnonzero((low > 0.05) & (low < 0.95)) + 1
            assert cols.size and (np.abs(cols - 62) <= 4).any(), cols
            if shape[0] == 250:
                assert (cols >= 244).any(), cols
            else:
                assert (np.abs(cols - 62) <= 4).all(), cols


def test_assert_bits_equal_sees_zero_signs_and_nans():
    a = np.array([[[0.0, -0.0, np.nan, 1.0, np.inf]]])
    S.assert_bits_equal(a, a.copy(), (128, 16), "same")
    nan2 = a.copy()
    nan2.view(np.uint64)[0, 0, 2] ^= 1  # another NaN payload: the same class
    S.assert_bits_equal(nan2, a, (128, 16), "payload")
    np.testing.assert_array_equal(np.array([0.0]), np.array([-0.0]))  # what the old tests saw
    for idx, val in ((0, -0.0), (1, 0.0), (2, 1.0), (3, np.nan), (3, np.nextafter(1.0, 2.0))):
        b = a.copy()
        b[0, 0, idx] = val
        with pytest.raises(AssertionError, match=rf"worst cell \(k, j, i\) = \(0, 0, {idx}\)"):
            S.assert_bits_equal(b, a, (128, 16), "diff")


def test_divz_and_deferred_division_match_division(tmp_path):
    """tools/divc_check.c, second mode: divz, the deferred DivFastZ + DivExact
    selection and divc against `/` for every test divisor, with the threshold
    claims (the full run is recorded in DESIGN.md; here 20 000 per family)."""
    exe = tmp_path / "divc_check"
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-o", str(exe),
                    str(ROOT / "tools" / "divc_check.c"), "-lm"], check=True)
    out = subprocess.run([str(exe), "divz", "20000"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout
    assert "192 divisors, 0 mismatches" in out.stdout, out.stdout
