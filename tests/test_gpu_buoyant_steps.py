"""Whole projection steps with buoyancy, a non-zero momentum source and the
energy equation on, from random fields at tile-seam shapes
(tests/buoyant_cases.py), against the oracle -- which
tests/test_projection_fixtures.py ties bit for bit to the reference's own
solve_projection_method on exactly these inputs, and whose inputs it shows to
make every term visible in at least 0.9 of the interior cells.

Every other bitwise step test runs with beta = 0, alpha = 0 and zero source
amplitudes. Here:

  k_pred3<true, FL> (CFD_HIP_PC3 unset, 2, 4) and k_pred2<true, 0> (0)
                 the T load and the three -beta dT g_q terms, with three
                 distinct gravity components, across a second x tile
  src_u_row[jc], src_v_col[c.i0], src_v_col[c.i0 + 1]
                 non-zero tables on both cells of a lane pair at the x seam
  k_energy       advection by an O(0.1) random velocity, thermal faces of all
                 three kinds, 64 x 4 blocks crossed in x and y
  the plugin's solve
                 plugin_solve -> host_steps(n_steps = max_iter) ->
                 step_device_impl(..., iter): the step index in
                 exp(-source_decay_rate iter dt), which scales the sources by
                 exp(-0.2) per step here
  Z-slabs        the T halo (and its periodic wrap) under buoyancy + energy

Jacobi-route steps (tolerance 1e-2, cap 5000, never reached) have no
summation anywhere: u, v, w, p, T, the iteration count and max_velocity /
max_pressure / max_temperature are the oracle's bit for bit. No number there
is a tolerance. The only tolerance of this file is test_gpu_parity's
CG_FIELD_RTOL (1e-10 of the field's scale) in the plugin's CG solve, whose dot
products the device sums in another order.

Measured on an MI355X, the plugin's solve against the oracle's, largest
|a - b| / max(1, max |b|) over the three shapes (bar 1e-10): u 2.9e-16, v
1.1e-16, w 5.6e-17, p 2.5e-15, T 0; CG iterations identical on every step
(215 / 218 / 215, 196 / 203 / 200, 46 / 47 / 47); three `step` calls end
1.6e-5 (u) and 9.8e-6 (v) away from the solve.

The cases fail on deliberately wrong builds (none kept): the sign of one
buoyancy component reversed in k_pred3 fails the all-terms cases under
CFD_HIP_PC3 unset / 2 / 4, the buoyancy-alone, device-resident, slab and
plugin cases; src_v_col[c.i0] read for both cells of a pair fails the same
with the sources-alone case instead; 0 passed for iter in host_steps fails
exactly test_plugin_solve_step_index.
"""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from cfd_amd import _abi as A
from cfd_amd import api
from tests import buoyant_cases as B
from tests import cg_seam_shapes as T
from tests.special_values import PC_TILE, assert_bits_equal
from tests.test_gpu_parity import CG_FIELD_RTOL, _rel_maxdiff
from tests.test_gpu_slabs import Slabs

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
FID = {"u": A.HIP_FIELD_U, "v": A.HIP_FIELD_V, "w": A.HIP_FIELD_W, "p": A.HIP_FIELD_P,
       "T": A.HIP_FIELD_T}
JACOBI_CFG = dict(poisson_method=A.HIP_POISSON_JACOBI, poisson_tolerance=T.JACOBI["tolerance"],
                  poisson_max_iter=T.JACOBI["max_iterations"])
KNOBS = ("CFD_HIP_PC3", "CFD_HIP_DIRTY_FACES", "CFD_HIP_CG_SMALL", "CFD_HIP_RB_SPLIT")


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in KNOBS:  # read once, when a context is created
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("CFD_HIP_GROUP_TIMEOUT_S", "60")


def _host_steps(shape, thermal="dn", terms="all"):
    """STEPS host-buffer Jacobi-route steps, each held to the oracle's."""
    want = B.oracle_jacobi_steps(shape, thermal, terms)
    g, f, p = B.case(shape, thermal, terms)
    ctx = api.HipProjection(g.nx, g.ny, g.nz, **JACOBI_CFG)
    try:
        for step, (fields, maxv, maxp, maxt, it) in enumerate(want):
            st = A.SolverStats()
            s = ctx.step(f, g, p, st)
            assert s == A.CFD_SUCCESS, (step, s, api._native.last_error())
            tag = f"{T.sid(shape)} {thermal} {terms} step {step}"
            for k in B.FIELDS:
                assert_bits_equal(getattr(f, k), fields[k], PC_TILE, f"{tag} {k}")
            assert ctx.poisson_stats().iterations == it, tag
            assert 0 < it < T.JACOBI["max_iterations"], tag
            assert st.iterations == 1
            assert (st.max_velocity, st.max_pressure, st.max_temperature) == (maxv, maxp, maxt), tag
    finally:
        ctx.close()
    return f


@pytest.mark.parametrize("pc3", [None, "0", "2", "4"],
                         ids=["pc3_default", "pc3_0", "pc3_2", "pc3_4"])
@pytest.mark.parametrize("shape", B.SEAM_SHAPES, ids=T.sid)
def test_steps_jacobi_all_terms(hip_lib, monkeypatch, shape, pc3):
    """Buoyancy, sources and energy together under every predictor / corrector
    form: k_pred3<true, 0 / NT_STORE / NT_STORE | NT_LOAD>, k_pred2<true, 0>."""
    if pc3 is not None:
        monkeypatch.setenv("CFD_HIP_PC3", pc3)
    _host_steps(shape)


@pytest.mark.parametrize("terms", B.TERMS[1:])
def test_steps_jacobi_one_term(hip_lib, terms):
    """One term at a time: a term that is wrong only when alone fails (BUOY =
    true reading an unset source table, k_energy without the T upload that
    buoyancy otherwise forces, ...)."""
    _host_steps((130, 18, 7), "dn", terms)


def test_device_resident_equals_host_buffer(hip_lib):
    """set_field / step_device / get_field against hip_proj_step on host
    buffers: the same bits, both the oracle's."""
    shape = (130, 18, 7)
    fh = _host_steps(shape)
    g, f, p = B.case(shape)
    want = B.oracle_jacobi_steps(shape)
    ctx = api.HipProjection(*shape, **JACOBI_CFG)
    try:
        for k, fid in FID.items():
            ctx.set_field(fid, getattr(f, k))
        ctx.set_density(float(f.rho.flat[0]))
        for step, (_, maxv, maxp, maxt, it) in enumerate(want):
            st = A.SolverStats()
            assert ctx.step_device(g, p, st) == A.CFD_SUCCESS, api._native.last_error()
            assert ctx.poisson_stats().iterations == it, step
            assert (st.max_velocity, st.max_pressure, st.max_temperature) == (maxv, maxp, maxt), step
        got = {k: ctx.get_field(fid) for k, fid in FID.items()}
    finally:
        ctx.close()
    for k in B.FIELDS:
        assert_bits_equal(got[k], getattr(fh, k), PC_TILE, f"device-resident vs host-buffer {k}")
        assert_bits_equal(got[k], want[-1][0][k], PC_TILE, f"device-resident vs oracle {k}")


# ---- the plugin's solve: the step index -----------------------------------------

def _plugin_ctx(solver):
    """The hip_proj context the plugin keeps as the first member of its own."""
    ctx = solver._ptr.contents.context
    assert ctx
    return C.cast(ctx, C.POINTER(C.c_void_p))[0]


def _last_cg_iterations(solver):
    ps = A.PoissonStats()
    assert api._native.hip().hip_proj_get_poisson_stats(_plugin_ctx(solver), C.byref(ps)) == 0
    return ps.iterations


@pytest.mark.parametrize("shape", [(130, 18, 7), (129, 17, 1), B.SMALL_SHAPE], ids=T.sid)
def test_plugin_solve_step_index(hip_lib, shape):
    """projection_hip through the registry with params.max_iter = 3 against
    oracle_projection_solve(CG, 3), i.e. the reference's loop with iter = 0,
    1, 2 in the source terms: u, v, w, p, T within CG_FIELD_RTOL, the CG
    iteration count of every step within 1 of the oracle's (test_gpu_parity.
    _step_both's gate for CG; the count of step n is read after a solve of
    n + 1 steps from the same inputs), stats.iterations == 3. At 17 x 13 x 11
    the result is held to the reference's own fields as well.

    Three `step` calls take index 0 each time. With amplitudes 0.3 / 0.2, dt
    1e-4 and exp(-0.2) per step they leave u and v about 0.3 1e-4 ((1 -
    e^-0.2) + (1 - e^-0.4)) = 1.5e-5 away from the solve's, 1e5 times the
    bar: asserted below at 1e3 times the bar, so a solve that passed index 0
    cannot pass.

    The Jacobi and RB-SOR plugins cannot serve here: their fixed 1e-6
    tolerance is not reachable from random, Neumann-incompatible fields within
    their caps (2000 / 5000), and loosening it is not the plugin's to do.

    Measured on an MI355X (bar 1e-10): fields within 2.5e-15 (p; u 2.9e-16),
    identical CG iteration counts; the figures are printed before the gates."""
    want, sto, its_o = B.oracle_cg_solve(shape, "dn", "all", "iter")
    reg = api.Registry()
    solver = reg.create("projection_hip")
    try:
        g, f, p = B.case(shape)
        assert solver.init(g, p) == A.CFD_SUCCESS, api._native.last_error()
        its_h = []
        for n in range(1, B.STEPS + 1):
            g, f, p = B.case(shape)
            p.max_iter = n
            st = A.SolverStats()
            s = solver.solve(f, g, p, st)
            assert s == A.CFD_SUCCESS, (n, s, api._native.last_error())
            assert st.iterations == n
            its_h.append(_last_cg_iterations(solver))
        print(f"BUOY solve {T.sid(shape)}: CG iterations {its_h} / oracle {its_o}")
        for ih, io in zip(its_h, its_o):
            assert abs(ih - io) <= 1, (its_h, its_o)
        assert st.max_velocity == pytest.approx(sto.max_velocity, rel=1e-9)
        assert st.max_pressure == pytest.approx(sto.max_pressure, rel=1e-9)
        assert st.max_temperature == pytest.approx(sto.max_temperature, rel=1e-12)
        devs = {k: _rel_maxdiff(getattr(f, k), want[k]) for k in B.FIELDS}
        print(f"BUOY solve {T.sid(shape)}: " + " ".join(f"{k} {v:.3e}" for k, v in devs.items()))
        for k in B.FIELDS:
            assert devs[k] <= CG_FIELD_RTOL, (k, devs[k])
        if shape == B.SMALL_SHAPE:
            z = np.load(GOLDEN / B.NPZ_FILE)
            rdev = {k: _rel_maxdiff(getattr(f, k), z[f"iter_{k}"]) for k in B.FIELDS}
            print(f"BUOY solve {T.sid(shape)} vs the reference's fields: " +
                  " ".join(f"{k} {v:.3e}" for k, v in rdev.items()))
            for k in B.FIELDS:
                assert rdev[k] <= CG_FIELD_RTOL, (k, rdev[k])
        # three `step` calls: index 0 every time
        g, f3, p = B.case(shape)
        for _ in range(B.STEPS):
            assert solver.step(f3, g, p, A.SolverStats()) == A.CFD_SUCCESS
    finally:
        solver.close()
    steps_o = B.oracle_cg_solve(shape, "dn", "all", "steps")[0]
    for k in ("u", "v"):
        assert _rel_maxdiff(getattr(f3, k), steps_o[k]) <= CG_FIELD_RTOL, k
        apart = _rel_maxdiff(getattr(f3, k), getattr(f, k))
        print(f"BUOY solve {T.sid(shape)}: three steps vs one solve, {k} {apart:.3e}")
        assert apart >= 1e3 * CG_FIELD_RTOL, (k, apart)


# ---- Z-slabs -----------------------------------------------------------------------

@pytest.mark.parametrize("thermal", B.THERMALS, ids=["z_neumann_dirichlet", "z_periodic"])
@pytest.mark.parametrize("nranks", [2, 3])
def test_slab_steps_jacobi_bitwise(hip_lib, nranks, thermal):
    """Three Jacobi-route step_device steps on in-process Z-slabs of (62, 30,
    27): the T halo under buoyancy and energy, with Neumann / Dirichlet
    thermal z faces and with periodic ones (the halo wrap between the first
    and the last rank). All five fields bitwise the single-domain oracle's,
    every rank's iteration counts and maxima the oracle's."""
    shape = B.SLAB_SHAPE
    want = B.oracle_jacobi_steps(shape, thermal)
    g, f, p = B.case(shape, thermal)
    S = Slabs(g, nranks, **JACOBI_CFG)
    try:
        S.scatter(f)
        for c in S.ctx:
            c.set_field(A.HIP_FIELD_T, f.T[c.k_offset:c.k_offset + c.nz_local])

        def body(r, c):
            out = []
            for _ in range(B.STEPS):
                st = A.SolverStats()
                s = c.step_device(g, p, st)
                assert s == A.CFD_SUCCESS, (r, s, api._native.last_error())
                out.append((st.max_velocity, st.max_pressure, st.max_temperature,
                            c.poisson_stats().iterations))
            return out
        hist = S.run(body)
        got = {}
        for k, fid in FID.items():
            out = np.full(f.u.shape, np.nan)
            for c in S.ctx:
                loc, glob = c.owned()
                out[glob] = c.get_field(fid)[loc]
            got[k] = out
    finally:
        S.close()
    for r in range(nranks):
        assert hist[r] == [w[1:] for w in want], (r, hist[r])
    for k in B.FIELDS:
        assert_bits_equal(got[k], want[-1][0][k], PC_TILE, f"slabs {nranks} {thermal} {k}")
