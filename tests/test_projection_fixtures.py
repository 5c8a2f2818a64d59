"""The buoyant / sourced / energy-coupled projection fixtures on the CPU
(tests/golden/projection_buoyant_cases.json, written by
tests/golden/make_projection_golden.py from the reference's own
solve_projection_method; cases of tests/buoyant_cases.py).

1. Integrity: the case table is the fixture's, the inputs regenerate, the
   .npz holds the fields the digests describe.
2. The oracle's projection (oracle_projection_solve, CG) reproduces the
   reference's record bit for bit: every case, with all three terms on and
   with each alone, as three max_iter = 1 calls and as one max_iter = 3 call.
   Every bitwise claim about the device step rests on this restatement. The
   two call patterns differ wherever the sources are on (the step index
   scales them by exp(-0.2) per step) and are the same bits where they are
   off (the energy step's time feeds only a heat-source callback).
3. Census, with the oracle alone on the Jacobi route: after one step a fault a
   kernel could have in any term changes the bits of at least 0.9 of the
   interior cells of every field the term reaches, so a bitwise comparison
   cannot miss it. Measured shares of the asserted fields: 1.0 for every
   buoyancy mutation, for alpha and for u under source_amplitude_u = 0; v
   under source_amplitude_v = 0 from 0.958 (17 x 13 x 11) and 0.994 (127 x 33
   x 6) to 1.0; step index 1: u 1.0, v from 0.961 (17 x 13 x 11). Fields a
   term reaches only through the pressure are printed, not asserted (u under
   source_amplitude_v = 0: 0.935 at 17 x 13 x 11, 0.961 at 129 x 17 x 5). 0.9
   is a condition the inputs meet with room, not a tuned bar.
"""
import json
from pathlib import Path

import numpy as np
import pytest

from cfd_amd import _abi as A
from oracle import oracle
from tests import buoyant_cases as B
from tests import cg_seam_shapes as T
from tests import rk_cases as R

GOLDEN = Path(__file__).resolve().parent / "golden"
DOC = json.loads((GOLDEN / B.JSON_FILE).read_text())
CASES = B.all_cases()
NAMES = [c[0] for c in CASES]
BY_NAME = {c[0]: c[1:] for c in CASES}
SHARE = 0.9


# ---- 1. integrity -------------------------------------------------------------

def test_case_table_matches_fixture():
    assert sorted(DOC["cases"]) == sorted(NAMES) and len(set(NAMES)) == len(NAMES)
    assert DOC["fields"] == list(B.FIELDS) and DOC["steps"] == B.STEPS
    for name, shape, thermal, terms in CASES:
        rec = DOC["cases"][name]
        assert (tuple(rec["shape"]), rec["thermal"], rec["terms"]) == (shape, thermal, terms)
        assert sorted(rec["runs"]) == sorted(B.PATTERNS)
        assert rec["runs"]["steps"]["max_iter"] == 1
        assert rec["runs"]["iter"]["max_iter"] == B.STEPS
        for run in rec["runs"].values():
            assert run["status"] == A.CFD_SUCCESS
    shapes = {s for s, _ in B.TABLE}
    assert shapes == set(B.SEAM_SHAPES) | {B.SLAB_SHAPE, B.SMALL_SHAPE}
    assert (B.SLAB_SHAPE, "pz") in B.TABLE  # the Z-slab halo wrap


def test_case_parameters():
    """What the table promises of a case's parameters."""
    g, f, p = B.case((130, 18, 7))
    assert (p.dt, p.mu, p.max_iter) == (1e-4, 0.01, 1)
    assert (p.beta, p.T_ref, p.alpha) == (B.BETA, 300.0, B.ALPHA)
    assert tuple(p.gravity) == B.GRAVITY and len(set(B.GRAVITY)) == 3 and all(B.GRAVITY)
    assert (p.source_amplitude_u, p.source_amplitude_v, p.source_decay_rate) == (0.3, 0.2, 2000.0)
    assert np.exp(-p.source_decay_rate * p.dt) == pytest.approx(np.exp(-0.2))
    assert np.all(f.rho == 1.25)
    tb = p.thermal_bc
    P, N, D = A.BC_TYPE_PERIODIC, A.BC_TYPE_NEUMANN, A.BC_TYPE_DIRICHLET
    assert (tb.left, tb.right, tb.bottom, tb.top, tb.back, tb.front) == (D, N, P, P, N, D)
    dv = tb.dirichlet_values
    assert (dv.left, dv.right, dv.bottom, dv.top, dv.back, dv.front) == B.THERMAL_VALUES
    tb = B.case(B.SLAB_SHAPE, "pz")[2].thermal_bc
    assert (tb.left, tb.right, tb.bottom, tb.top, tb.back, tb.front) == (D, N, P, P, P, P)
    assert B.case((129, 17, 1))[2].gravity[2] == 0.0
    for terms, want in (("buoyancy", (B.BETA, 0.0, 0.0, 0.0)), ("sources", (0.0, 0.3, 0.2, 0.0)),
                        ("energy", (0.0, 0.0, 0.0, B.ALPHA))):
        q = B.case((17, 13, 11), "dn", terms)[2]
        assert (q.beta, q.source_amplitude_u, q.source_amplitude_v, q.alpha) == want, terms


@pytest.mark.parametrize("shape,thermal", B.TABLE, ids=[B.name(s, th, "")[:-1] for s, th in B.TABLE])
def test_inputs_regenerate(shape, thermal):
    """A drifted builder reads as an input mismatch, not as a kernel failure."""
    for terms in B.TERMS:
        _, f, _ = B.case(shape, thermal, terms)
        for k in B.INPUTS:
            assert R.sha(getattr(f, k)) == DOC["cases"][B.name(shape, thermal, terms)]["inputs"][k], \
                (terms, k)
    nx, ny, nz = shape
    want = 300.0 + 5.0 * np.random.default_rng(nx * 7 + nz * 3 + ny + 2).standard_normal((nz, ny, nx))
    assert np.array_equal(f.T, want)
    assert 2.0 < float(np.std(f.T)) < 8.0


def test_npz_matches_digests():
    z = np.load(GOLDEN / B.NPZ_FILE)
    shape, thermal, terms = B.NPZ_CASE
    rec = DOC["cases"][B.name(shape, thermal, terms)]
    assert sorted(z.files) == sorted(f"{pt}_{k}" for pt in B.PATTERNS for k in B.FIELDS)
    for pattern in B.PATTERNS:
        for k in B.FIELDS:
            assert R.digest(z[f"{pattern}_{k}"]) == rec["runs"][pattern]["outputs"][k], (pattern, k)


# ---- 2. the oracle against the reference's record -----------------------------

def _oracle_run(shape, thermal, terms, pattern):
    g, f, p = B.case(shape, thermal, terms)
    if pattern == "iter":
        s, st, its = oracle.projection_solve(f, g, p, B.STEPS)
        assert st.iterations == B.STEPS
    else:
        its = []
        for _ in range(B.STEPS):
            s, st, it = oracle.projection_step(f, g, p)
            assert s == A.CFD_SUCCESS and st.iterations == 1
            its.append(it)
    assert s == A.CFD_SUCCESS
    assert len(its) == B.STEPS and all(0 < it < 5000 for it in its), its
    return f, its


@pytest.mark.parametrize("name", NAMES)
def test_oracle_reproduces_reference_projection(name):
    """Bit for bit: the oracle restates the scalar path operation for
    operation, CG's sequential dot products included."""
    shape, thermal, terms = BY_NAME[name]
    got = {}
    for pattern in B.PATTERNS:
        f, its = _oracle_run(shape, thermal, terms, pattern)
        want = DOC["cases"][name]["runs"][pattern]["outputs"]
        for k in B.FIELDS:
            d = R.digest(getattr(f, k))
            assert d["sha256"] == want[k]["sha256"], \
                (name, pattern, k, "max |.|", d["max"], want[k]["max"], "sum", d["sum"], want[k]["sum"])
        got[pattern] = f
        print(f"PROJ {name} {pattern}: CG iterations {its}, bitwise the reference's")
    # the step index: visible exactly where the sources are on
    for k in ("u", "v", "w", "p"):
        a, b = getattr(got["steps"], k), getattr(got["iter"], k)
        if terms in ("all", "sources"):
            assert B.changed_share(a, b) >= SHARE, (name, k)
        else:
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (name, k)


def test_record_tells_the_call_patterns_apart():
    """The reference's own record: max_iter = 3 differs from three max_iter =
    1 calls in u, v, w, p wherever the sources are on, and only there."""
    for name, _, _, terms in CASES:
        runs = DOC["cases"][name]["runs"]
        for k in ("u", "v", "w", "p"):
            same = runs["steps"]["outputs"][k]["sha256"] == runs["iter"]["outputs"][k]["sha256"]
            assert same == (terms not in ("all", "sources")), (name, k)


def test_solve_of_one_step_is_the_step():
    """oracle_projection_step stays the n_steps = 1 case."""
    for shape in ((17, 13, 11), (129, 17, 1)):
        g, f, p = B.case(shape)
        g2, f2, p2 = B.case(shape)
        s, st, it = oracle.projection_step(f, g, p)
        s2, st2, its2 = oracle.projection_solve(f2, g2, p2, 1)
        assert (s, s2) == (A.CFD_SUCCESS, A.CFD_SUCCESS) and its2 == [it]
        assert (st.iterations, st.max_velocity, st.max_pressure, st.max_temperature) == \
            (st2.iterations, st2.max_velocity, st2.max_pressure, st2.max_temperature)
        for k in B.FIELDS:
            assert np.array_equal(getattr(f, k).view(np.uint64), getattr(f2, k).view(np.uint64)), k


# ---- 3. census ------------------------------------------------------------------

def _jacobi(shape, thermal, mutate=None, n_steps=1, solve=False):
    """The fields after n Jacobi-route oracle steps of the (mutated) case."""
    g, f, p = B.case(shape, thermal)
    if mutate:
        mutate(f, p)
    oracle.set_projection_poisson_params(oracle.poisson_params(**T.JACOBI))
    try:
        if solve:
            s, _, its = oracle.projection_solve(f, g, p, n_steps, A.ORACLE_POISSON_JACOBI)
            assert s == A.CFD_SUCCESS
        else:
            its = []
            for _ in range(n_steps):
                s, _, it = oracle.projection_step(f, g, p, A.ORACLE_POISSON_JACOBI)
                assert s == A.CFD_SUCCESS
                its.append(it)
    finally:
        oracle.set_projection_poisson_params(None)
    assert all(it < T.JACOBI["max_iterations"] for it in its), its
    return f


def _swap_gravity(f, p):
    p.gravity[0], p.gravity[1] = p.gravity[1], p.gravity[0]


def _roll_T(f, p):
    f.T[...] = np.roll(f.T, 1, axis=2)


@pytest.mark.parametrize("shape,thermal", B.TABLE, ids=[B.name(s, th, "")[:-1] for s, th in B.TABLE])
def test_every_term_is_visible_after_one_step(shape, thermal):
    three = shape[2] > 1
    true = _jacobi(shape, thermal)
    lines = []

    def shares(what, mutate, fields, **kw):
        base = true if not kw else _jacobi(shape, thermal, None, **{**kw, "solve": False})
        got = _jacobi(shape, thermal, mutate, **kw)
        out = {k: B.changed_share(getattr(got, k), getattr(base, k)) for k in B.FIELDS}
        lines.append(f"CENSUS {T.sid(shape)} {thermal} {what}: " +
                     " ".join(f"{k} {v:.3f}" for k, v in out.items()))
        print(lines[-1])
        for k in fields:
            assert out[k] >= SHARE, (what, k, out[k])
        return out

    buoyant = ("u", "v") + (("w",) if three else ()) + ("p", "T")
    shares("beta = 0", lambda f, p: setattr(p, "beta", 0.0), buoyant)
    shares("gravity 0 <-> 1", _swap_gravity, buoyant)
    shares("T rolled in x", _roll_T, buoyant)
    shares("T_ref = 0", lambda f, p: setattr(p, "T_ref", 0.0), buoyant)
    shares("source_amplitude_u = 0", lambda f, p: setattr(p, "source_amplitude_u", 0.0), ("u",))
    shares("source_amplitude_v = 0", lambda f, p: setattr(p, "source_amplitude_v", 0.0), ("v",))
    out = shares("alpha = 0", lambda f, p: setattr(p, "alpha", 0.0), ("T",))
    assert [out[k] for k in ("u", "v", "w", "p")] == [0.0] * 4, out
    # step index 1 instead of 0 in the second step: one solve of two steps
    # against two single steps
    shares("step index 1", None, ("u", "v"), n_steps=2, solve=True)
