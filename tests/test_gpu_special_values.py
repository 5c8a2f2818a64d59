"""The fast-division fallbacks of every kernel on tiny, subnormal, huge,
signed-zero, non-finite and planted fields (tests/special_values.py), bit for
bit against the oracle: sign of zero and NaN positions included
(special_values.assert_bits_equal). test_special_values.py proves on the CPU
that these inputs put at least a tenth of the interior cells on either side
of the range [2^-900, 2^900] in every division class, so each wave mixes
lanes that keep the reciprocal-multiply value with lanes that must take
`/`:

  k_pred3 / k_corr3 (CFD_HIP_PC3 unset), k_pred2 / k_corr2 (0) and the
  variants 2 and 4     DivFastZ's lane flag, then DivExact on the flagged lanes
                       behind wave_any_bad: whole Jacobi-route steps (no
                       summation anywhere), two of them (huge: one), with exact
                       max_velocity / max_pressure and iteration counts
  k_rb1 at every tile width, k_rb1 by check_interval = 2, k_rb2 in both
  modes (its exact recompute on the tiny problems, its uncertified stop on the
  huge ones), k_rx at 8 and 16 rows, k_rb_pass / k_jacobi (relax_two_pass = 1),
  k_rb_edge_r + k_rb1 on Z-slabs with and without the split launch
                       divc's a / d branch: solves capped at 6 and 7
                       iterations with both tolerances 0, from the ramp
                       problems whose threshold surface survives the sweeps

No number here is a tolerance: every comparison is on bits or exact counts.

What these steps cannot see. (1) A quotient just below 2^-900 that skipped
its fallback: the range is conservative, the reciprocal-multiply value stays
`/`'s until the inner residual (2^-53 of the operand) loses bits that matter,
at operands near 2^-1020. A lane flag that never drops therefore fails only
the subnormal and the non-finite regimes (measured), not tiny, huge or
planted. (2) The sign of a zero quotient. A predicted velocity
is fc + dt (-conv + visc + src) with src = +0.0 or, where fc = -0.0 could keep
the sum's sign, a second difference xp - 2 fc + xm that is then +0.0; so an
interior u*, v*, w* is never -0.0 and u* - (dt / rho) dp/dx takes neither
sign of a zero dp/dx into its result. DivFastZ returning divc's form (+0 for
a = -0) passes every test here; divz's promise of `/`'s zero is pinned on the
formula alone, by tools/divc_check.c's second mode (test_special_values.py).
"""
import functools

import numpy as np
import pytest

from cfd_amd import _abi as A
from cfd_amd import api
from oracle import oracle
from tests import cg_seam_shapes as T
from tests import special_values as S
from tests.test_gpu_slabs import Slabs

pytestmark = pytest.mark.gpu

KNOBS = ("CFD_HIP_PC3", "CFD_HIP_RB2", "CFD_HIP_RB2_TEST", "CFD_HIP_RB2_LOG", "CFD_HIP_RB1_TC",
         "CFD_HIP_RB_SPLIT")
# steps per regime: the huge shell keeps the second step's Jacobi solve from
# converging within its 5000 iterations (the oracle returns MAX_ITER), so
# that regime runs one
STEPS = {"huge": 1}
RB1_TILE = (124,)
SHAPES_3D = [s for s in S.RELAX_SHAPES if s[2] > 1]


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in KNOBS:  # read once, when a context is created
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("CFD_HIP_GROUP_TIMEOUT_S", "60")


# ---- whole steps on the Jacobi route ----------------------------------------

@functools.lru_cache(maxsize=None)
def _oracle_steps(regime, shape):
    """Per step: ({field: array}, max_velocity, max_pressure, iterations) of
    the oracle, computed once per (regime, shape) and left unchanged."""
    g, f, p = S.step_fields(regime, shape)
    out = []
    oracle.set_projection_poisson_params(oracle.poisson_params(**T.JACOBI))
    try:
        for _ in range(STEPS.get(regime, 2)):
            s, st, it = oracle.projection_step(f, g, p, A.ORACLE_POISSON_JACOBI)
            assert s == A.CFD_SUCCESS, (regime, shape, s)
            fields = {k: getattr(f, k).copy() for k in S.FIELDS}
            for a in fields.values():
                a.setflags(write=False)
            out.append((fields, st.max_velocity, st.max_pressure, it))
    finally:
        oracle.set_projection_poisson_params(None)
    return out


@pytest.mark.parametrize("pc3", [None, "0", "2", "4"], ids=["pc3_default", "pc3_0", "pc3_2", "pc3_4"])
@pytest.mark.parametrize("shape", S.STEP_SHAPES, ids=T.sid)
@pytest.mark.parametrize("regime", S.REGIMES)
def test_steps_jacobi_special_values(hip_lib, monkeypatch, regime, shape, pc3):
    if pc3 is not None:
        monkeypatch.setenv("CFD_HIP_PC3", pc3)
    want = _oracle_steps(regime, shape)
    g, f, p = S.step_fields(regime, shape)
    ctx = api.HipProjection(g.nx, g.ny, g.nz, poisson_method=A.HIP_POISSON_JACOBI,
                            poisson_tolerance=T.JACOBI["tolerance"],
                            poisson_max_iter=T.JACOBI["max_iterations"])
    try:
        for step, (fields, maxv, maxp, it) in enumerate(want):
            st = A.SolverStats()
            s = ctx.step(f, g, p, st)
            assert s == A.CFD_SUCCESS, (step, s, api._native.last_error())
            tag = f"{regime} {T.sid(shape)} pc3 {pc3} step {step}"
            for k in S.FIELDS:
                S.assert_bits_equal(getattr(f, k), fields[k], S.PC_TILE, f"{tag} {k}")
            assert ctx.poisson_stats().iterations == it, tag
            assert st.iterations == 1
            assert (st.max_velocity, st.max_pressure) == (maxv, maxp), tag
    finally:
        ctx.close()


# ---- capped relaxation solves -----------------------------------------------

METHOD = {"rb": A.HIP_POISSON_REDBLACK, "jacobi": A.HIP_POISSON_JACOBI}


def _check(tag, method, kind, axis, shape, cap, s, st, x, check_interval=1):
    so, sto, xo = S.relax_oracle(method, kind, axis, shape, cap, check_interval)
    assert s == so, f"{tag}: status {s}, want {so}"
    assert (st.iterations, st.status) == (sto.iterations, sto.status), tag
    assert st.initial_residual == sto.initial_residual, tag
    assert st.final_residual == sto.final_residual, tag
    S.assert_bits_equal(x, xo, RB1_TILE if method == "rb" else S.PC_TILE, tag)


def _capped_solves(what, method, shape, problems=S.RELAX_PROBLEMS, check_interval=1, **cfg):
    """Every problem at both caps on one context; all failures reported
    together."""
    fails = []
    ctx = api.HipProjection(*shape, **cfg)
    try:
        for kind, axis in problems:
            x0, rhs = S.relax_problem(kind, axis, shape)
            for cap in S.RELAX_CAPS:
                x = x0.copy()
                s, st = ctx.poisson_solve(METHOD[method], x, rhs, *T.spacing(shape),
                                          S.relax_params(cap, check_interval=check_interval))
                try:
                    _check(f"{what} {method} {kind} {axis} {T.sid(shape)} cap {cap}", method, kind,
                           axis, shape, cap, s, st, x, check_interval)
                except AssertionError as e:
                    fails.append(str(e))
    finally:
        ctx.close()
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("tc", ["64", "32", "16"])
@pytest.mark.parametrize("shape", SHAPES_3D, ids=T.sid)
def test_rb1_tile_widths(hip_lib, monkeypatch, shape, tc):
    monkeypatch.setenv("CFD_HIP_RB2", "0")
    monkeypatch.setenv("CFD_HIP_RB1_TC", tc)
    _capped_solves(f"k_rb1 tc {tc}", "rb", shape)


@pytest.mark.parametrize("shape", S.RELAX_SHAPES, ids=T.sid)
def test_rb1_by_check_interval(hip_lib, shape):
    """check_interval = 2 routes every sweep past k_rb2 (2-D: k_rx's sweeps)."""
    _capped_solves("check_interval 2", "rb", shape, check_interval=2)


@pytest.mark.parametrize("mode", ["1", "2"])
@pytest.mark.parametrize("shape", S.RELAX_SHAPES, ids=T.sid)
def test_rb2_tiny_and_subnormal(hip_lib, monkeypatch, shape, mode):
    monkeypatch.setenv("CFD_HIP_RB2", mode)
    _capped_solves(f"k_rb2 mode {mode}", "rb", shape,
                   [p for p in S.RELAX_PROBLEMS if p[0] != "huge"])


@pytest.mark.parametrize("shape", SHAPES_3D, ids=T.sid)
def test_rb2_huge_is_uncertified(hip_lib, monkeypatch, capfd, shape):
    """|x0| > 2^800: the first sweep's input is not certified, the host reruns
    with one iteration per sweep, and the launch log says so."""
    monkeypatch.setenv("CFD_HIP_RB2", "1")
    monkeypatch.setenv("CFD_HIP_RB2_LOG", "1")
    problems = [p for p in S.RELAX_PROBLEMS if p[0] == "huge"]
    capfd.readouterr()
    _capped_solves("k_rb2 huge", "rb", shape, problems)
    lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("rb2:")]
    assert len(lines) == len(problems) * len(S.RELAX_CAPS), lines
    for ln in lines:
        assert "1 uncertified" in ln, ln


@pytest.mark.parametrize("rows", [8, 16])
@pytest.mark.parametrize("shape", S.RELAX_SHAPES, ids=T.sid)
def test_jacobi_fused_loop(hip_lib, shape, rows):
    _capped_solves(f"k_rx rows {rows}", "jacobi", shape, sweep_rows=rows)


@pytest.mark.parametrize("method", ["rb", "jacobi"])
@pytest.mark.parametrize("shape", S.RELAX_SHAPES, ids=T.sid)
def test_two_pass(hip_lib, shape, method):
    _capped_solves("relax_two_pass 1", method, shape, relax_two_pass=1)


class _Spacing:
    def __init__(self, shape):
        self.nx, self.ny, self.nz = shape
        self.dx, self.dy, self.dz = T.spacing(shape)


@pytest.mark.parametrize("split", [None, "0"], ids=["split", "no_split"])
@pytest.mark.parametrize("shape", [(130, 20, 9), (250, 21, 10)], ids=T.sid)
def test_slabs_two_ranks(hip_lib, monkeypatch, shape, split):
    """test_gpu_slabs._slab_poisson's solve on one group of 2 ranks (4 + 3 and
    4 + 4 interior planes), every problem and cap: k_rb_edge_r, the R halo and
    k_rb1 as three launches or (CFD_HIP_RB_SPLIT=0) one; Jacobi beside it."""
    if split is not None:
        monkeypatch.setenv("CFD_HIP_RB_SPLIT", split)
    g = _Spacing(shape)
    fails = []
    grp = Slabs(g, 2)
    try:
        for method in ("rb", "jacobi") if split is None else ("rb",):
            for kind, axis in S.RELAX_PROBLEMS:
                x0, rhs = S.relax_problem(kind, axis, shape)
                for cap in S.RELAX_CAPS:
                    prm = S.relax_params(cap)

                    def body(r, c):
                        sl = slice(c.k_offset, c.k_offset + c.nz_local)
                        x = np.array(x0[sl])
                        s, st = c.poisson_solve(METHOD[method], x, np.array(rhs[sl]), g.dx, g.dy,
                                                g.dz, prm)
                        return s, st, x
                    res = grp.run(body)
                    x = np.full(x0.shape, np.nan)
                    for c, (s, st, xl) in zip(grp.ctx, res):
                        loc, glob = c.owned()
                        x[glob] = xl[loc]
                    for r, (s, st, xl) in enumerate(res):
                        try:
                            _check(f"slabs rank {r} split {split} {method} {kind} {axis} "
                                   f"{T.sid(shape)} cap {cap}", method, kind, axis, shape, cap, s,
                                   st, x)
                        except AssertionError as e:
                            fails.append(str(e))
    finally:
        grp.close()
    assert not fails, "\n".join(fails[:6])
