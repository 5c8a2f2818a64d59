"""k_rb2's interior-tile steady march (rb2.hpp: rb2_march<BND = false>, the
ZB = false steps) against the oracle, bit for bit, on the shapes of
tests/rb2_shapes.py: grids with interior tiles, z runs long enough for steady
groups of four (CFD_HIP_RB2_KC_FIXED keeps them from being halved away), every
tail residue, interior-to-interior seams, and the product's 128-plane run.
test_rb2_shapes.py proves on the CPU that the table reaches that code and that
the shapes of test_gpu_rb2.py never do.

Besides the bits (status, iteration count, both residuals, x with its shell),
the launch log (CFD_HIP_RB2_LOG) must show the path taken: the layout of
rb2_shapes.layout, the k_rb2 launches the iteration count implies, and in the
product form no uncertified sweep (a silent rerun with k_rb1 gives the same
bits) and no ambiguous decision on solves whose residuals are nowhere near
their threshold."""
import re

import numpy as np
import pytest

from cfd_amd import _abi as A
from cfd_amd import api
from oracle import oracle
from tests import cg_seam_shapes
from tests import rb2_shapes as T
from tests.test_gpu_rb2 import MODES
from tests.special_values import assert_bits_equal

pytestmark = pytest.mark.gpu

LOG = re.compile(r"rb2: iterations (\d+) status (\d+), k_rb1 (\d+) k_rb2 (\d+) launches, "
                 r"(\d+) ambiguous, (\d+) uncertified, res_it (\d+), kc (\d+) tiles (\d+) x (\d+) "
                 r"x (\d+) interior (\d+)")
FIELDS = ("iterations", "status", "k_rb1", "k_rb2", "ambiguous", "uncertified", "res_it", "kc",
          "tiles_x", "tiles_y", "tiles_z", "interior")
CAPPED = [(c, cap) for c in T.CASES for cap in T.CAPS]
TOLS = [(c, tol) for c, tols in T.TOL_CASES for tol in tols]


def _id(v):
    return getattr(v, "id", None) or str(v)


def _env(monkeypatch, case, mode="1", knob="0", xmap=None):
    for k in ("CFD_HIP_RB2_KC", "CFD_HIP_RB2_XMAP", "CFD_HIP_RB1_FOLD", "CFD_HIP_RB1_TC"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("CFD_HIP_RB2", mode)
    monkeypatch.setenv("CFD_HIP_RB2_TEST", knob)
    monkeypatch.setenv("CFD_HIP_RB2_KC_FIXED", "1")
    monkeypatch.setenv("CFD_HIP_RB2_LOG", "1")
    if case.kc:
        monkeypatch.setenv("CFD_HIP_RB2_KC", str(case.kc))
    if xmap:
        monkeypatch.setenv("CFD_HIP_RB2_XMAP", xmap)


def _logs(capfd):
    err = capfd.readouterr().err
    return [dict(zip(FIELDS, (int(v) for v in m.groups()))) for m in LOG.finditer(err)]


def _solve(case, peak, key, capfd):
    """The device solve of rb2_shapes.oracle_solve(case.shape, peak, key) and
    its log line."""
    nx, ny, nz = case.shape
    rhs, x0 = T.problem(case.shape, peak)
    prm = T.capped_params(key[1]) if key[0] == "cap" else T.tol_params(key[1])
    capfd.readouterr()
    ctx = api.HipProjection(nx, ny, nz)
    x = x0.copy()
    s, st = ctx.poisson_solve(A.HIP_POISSON_REDBLACK, x, rhs, *T.spacing(case.shape), prm)
    ctx.close()
    logs = _logs(capfd)
    assert len(logs) == 1, logs
    return s, st, x, logs[0]


def _check_bitwise(case, peak, key, got):
    so, sto, xo = T.oracle_solve(case.shape, peak, key)
    s, st, x, log = got
    where = T.first_diff(x, xo, case) or "x is bitwise the oracle's"
    tag = f"{case.id} {key} log {log}; {where}"
    assert s == so, tag
    assert (st.iterations, st.status) == (sto.iterations, sto.status), \
        f"{st.iterations} iterations, status {st.status}, want {sto.iterations}, {sto.status}; {tag}"
    assert st.initial_residual == sto.initial_residual, \
        f"initial residual {st.initial_residual!r}, want {sto.initial_residual!r}; {tag}"
    assert st.final_residual == sto.final_residual, \
        f"final residual {st.final_residual!r}, want {sto.final_residual!r}; {tag}"
    assert T.first_diff(x, xo, case) is None, tag


def _check_layout(case, log):
    """The context marched the runs and tiles the table says."""
    lay = T.layout(case.shape, case.kc)
    assert (log["kc"], log["tiles_x"], log["tiles_y"], log["tiles_z"], log["interior"]) == \
        (lay.kc, lay.tiles_x, lay.tiles_y, len(lay.runs), len(lay.interior)), log


def _check_path(case, key, st, log, mode, knob):
    """The launches and host stops of the solve, by mode."""
    _check_layout(case, log)
    cap = key[1] if key[0] == "cap" else T.TOL_CAP
    stop = st.iterations if st.status == A.POISSON_CONVERGED else cap
    assert log["res_it"] == stop, log
    n1, n2 = T.host_launches(stop, cap)
    if knob == "2":  # forced: the first sweep fails its range test, k_rb1 from there on
        assert (log["uncertified"], log["k_rb2"]) == (1, 0), log
        assert log["k_rb1"] >= stop, log
        return
    assert log["uncertified"] == 0, log  # no silent rerun with k_rb1
    if knob == "1":  # forced: every approximate decision goes to the host
        assert log["ambiguous"] >= 1 and log["k_rb1"] == 1, log
        return
    if key[0] == "cap":
        # residuals of order 1e4 against a bound of order 1e-9 and thresholds of 0
        assert log["ambiguous"] == 0, log
    else:
        assert log["ambiguous"] <= 1, log
    assert log["k_rb1"] == 1, log
    if log["ambiguous"] == 0:
        assert log["k_rb2"] == n2, (log, n2)
    assert log["k_rb2"] >= (stop + 1) // 2, log


@pytest.mark.parametrize("mode,knob", MODES)
@pytest.mark.parametrize("case,cap", CAPPED, ids=_id)
def test_capped_bitwise_and_path(hip_lib, monkeypatch, capfd, case, cap, mode, knob):
    """Every table case, capped at an even and an odd count, in every mode of
    test_gpu_rb2.MODES."""
    _env(monkeypatch, case, mode, knob)
    got = _solve(case, False, ("cap", cap), capfd)
    _check_bitwise(case, False, ("cap", cap), got)
    _check_path(case, ("cap", cap), got[1], got[3], mode, knob)


@pytest.mark.parametrize("mode,knob", MODES)
@pytest.mark.parametrize("case,tol", TOLS, ids=_id)
def test_tolerance_bitwise_and_path(hip_lib, monkeypatch, capfd, case, tol, mode, knob):
    """Converged stops on a sweep's input and on its middle iterate (odd and
    even counts, test_rb2_shapes.py)."""
    _env(monkeypatch, case, mode, knob)
    got = _solve(case, False, ("tol", tol), capfd)
    _check_bitwise(case, False, ("tol", tol), got)
    assert got[1].status == A.POISSON_CONVERGED
    _check_path(case, ("tol", tol), got[1], got[3], mode, knob)


@pytest.mark.parametrize("mode,knob", MODES)
@pytest.mark.parametrize("tol", T.PEAK_TOLS)
def test_interior_peak_bitwise_and_path(hip_lib, monkeypatch, capfd, tol, mode, knob):
    """The L-inf residual of every iterate lies in cells whose residual only
    the interior tile's steady steps form (unmasked maxima, the `own` mask
    applied after the march): the decisions, the stopping iterate and the
    reported residuals are the oracle's."""
    case = T.PEAK_CASE
    _env(monkeypatch, case, mode, knob)
    got = _solve(case, True, ("tol", tol), capfd)
    _check_bitwise(case, True, ("tol", tol), got)
    assert got[1].status == A.POISSON_CONVERGED
    _check_path(case, ("tol", tol), got[1], got[3], mode, knob)


def test_xcd_tile_order_bitwise(hip_lib, monkeypatch, capfd):
    """CFD_HIP_RB2_XMAP=1 changes which workgroup marches which tile, nothing
    else: the default order's bits and launches."""
    case, key = T.XMAP_CASE, ("cap", 7)
    _env(monkeypatch, case)
    base = _solve(case, False, key, capfd)
    _env(monkeypatch, case, xmap="1")
    got = _solve(case, False, key, capfd)
    _check_bitwise(case, False, key, got)
    _check_path(case, key, got[1], got[3], "1", "0")
    assert T.first_diff(got[2], base[2], case) is None
    assert got[3] == base[3]


@pytest.mark.parametrize("shape", [(250, 30, 40), (131, 27, 70)], ids=T.sid)
def test_default_layout_is_the_halved_one(hip_lib, monkeypatch, capfd, shape):
    """Without CFD_HIP_RB2_KC_FIXED the context keeps the product's rule (runs
    halved down to 4 planes at these sizes), on two shapes of test_gpu_rb2."""
    case = T.Case(shape, None, "default layout")
    _env(monkeypatch, case)
    monkeypatch.delenv("CFD_HIP_RB2_KC_FIXED")
    s, st, x, log = _solve(case, False, ("cap", 6), capfd)
    lay = T.layout(shape, fixed=False)
    assert lay.kc == 4 and lay.interior == []
    assert (log["kc"], log["tiles_x"], log["tiles_y"], log["tiles_z"], log["interior"]) == \
        (lay.kc, lay.tiles_x, lay.tiles_y, len(lay.runs), 0), log
    so, sto, xo = T.oracle_solve(shape, False, ("cap", 6))
    assert (s, st.iterations, st.final_residual) == (so, sto.iterations, sto.final_residual)
    assert_bits_equal(x, xo)


def test_whole_step_bitwise(hip_lib, monkeypatch, capfd):
    """Two projection steps with RB-SOR on a grid with an interior tile and a
    28-plane run: u, v, w, p and the iteration counts are the oracle's."""
    case = T.CASES[2]
    assert case.shape == T.STEP_SHAPE
    _env(monkeypatch, case)
    g, f, p = cg_seam_shapes.step_case(T.STEP_SHAPE)
    fo = api.FlowField(g.nx, g.ny, g.nz)
    fo.copy_from(f)
    oracle.set_projection_poisson_params(oracle.poisson_params(**T.STEP_RELAX))
    capfd.readouterr()
    ctx = api.HipProjection(g.nx, g.ny, g.nz, poisson_method=A.HIP_POISSON_REDBLACK,
                            poisson_tolerance=T.STEP_RELAX["tolerance"],
                            poisson_max_iter=T.STEP_RELAX["max_iterations"])
    try:
        for step in range(2):
            so, _, io = oracle.projection_step(fo, g, p, A.ORACLE_POISSON_REDBLACK)
            sh = ctx.step(f, g, p, A.SolverStats())
            assert so == A.CFD_SUCCESS
            assert sh == A.CFD_SUCCESS, (sh, api._native.last_error())
            assert ctx.poisson_stats().iterations == io, step
            for k in ("u", "v", "w", "p"):
                where = T.first_diff(getattr(f, k), getattr(fo, k), case)
                assert where is None, f"step {step} field {k}: {where}"
    finally:
        oracle.set_projection_poisson_params(None)
        ctx.close()
    logs = _logs(capfd)
    assert len(logs) == 2, logs
    for log in logs:
        _check_layout(case, log)
        assert log["uncertified"] == 0 and log["ambiguous"] <= 1 and log["k_rb1"] == 1, log
