"""The context's tile planning (cfd_amd/csrc/hip/tile_plan.hpp: plan_tiles,
read_knobs, slab_layout) pinned without a GPU. tests/native/tile_plan_dump.cpp
is compiled with g++ under ASan + UBSan and run on the whole case table
(tests/tile_plan_cases.py):

  a. every plan's digest, and the whole plan of a few readable cases, equal
     those in tests/golden/tile_plans.json, which was recorded from the
     arithmetic init_ctx carried before the planner was split out of it;
  b. the Python model of k_rb2's tiling (tests/rb2_shapes.py), which the GPU
     tests compare the launch log with, agrees with the planner;
  c. the one-line descriptions of the seam tables (tests/cg_seam_shapes.py,
     test_gpu_ccf_edge_dot.EDGE_FIXED) claim the tile counts and z runs the
     planner gives under the switches their GPU tests set.
"""
import json
import re
import shutil

import pytest

from tests import cg_seam_shapes as S
from tests import rb2_shapes as RB2
from tests import tile_plan_cases as C

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not present")


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """plans(lines) -> {line: plan}; the table's own cases are planned once."""
    exe = C.build_dump(tmp_path_factory.mktemp("tile_plan"))
    known = C.run_dump(exe, C.cases())

    def plans(lines):
        new = [ln for ln in dict.fromkeys(lines) if ln not in known]
        if new:
            known.update(C.run_dump(exe, new))
        return {ln: known[ln] for ln in lines}

    plans.table = known
    return plans


# ---- a. the recorded plans ---------------------------------------------------

def test_plans_equal_the_recorded_ones(dump):
    fixture = json.loads(C.FIXTURE.read_text())
    # the readable plans, field by field: {case: {field: (planned now, recorded)}}
    assert list(fixture["plans"]) == C.readable()
    moved = {c: {k: (dump.table[c].get(k), v) for k, v in p.items() if dump.table[c].get(k) != v}
             for c, p in fixture["plans"].items() if dump.table[c] != p}
    assert not moved, moved
    want = fixture["digests"]
    assert list(want) == C.cases()  # the table and the fixture list the same cases
    bad = {c: dump.table[c] for c in want if C.plan_digest(dump.table[c]) != want[c]}
    assert not bad, (f"{len(bad)} plans differ from the recorded ones; the first, as planned "
                     f"now: {list(bad.items())[:1]}")


def test_table_covers_what_it_names(dump):
    t = dump.table
    full = [p for p in t.values() if "geo" in p]
    assert sum(1 for p in full if p["rg_strip"]) >= 3 and sum(1 for p in full if p["split_rb"]) > 20
    assert {p["rb1_tc"] for p in full} == {64, 32, 16}
    assert {p["pc3"] for p in full} == {0, 1, 2, 4}
    assert {p["sweep_ty"] for p in full} == {4, 8, 16}
    norm = {r: t[C.line((96, 96, 96), sweep_rows=r, only="sweep_variants")]["sweep_variants"]
            for r in (8, 16)}
    assert set(norm[16]) == {0, 1, 2, 3, 4, 7, 15, 23, 31} and set(norm[8]) == set(norm[16]) - {23, 31}
    assert all(len(v) == 64 for v in norm.values())
    # the slab thresholds: ranks of 2, 3 and 4 interior planes
    by_planes = {}
    for c, p in t.items():
        if "ranks=2" in c and "shape=62x30x" in c:
            by_planes.setdefault(p["nz_local"] - 2, set()).add((p["split_b"], p["split_rb"]))
    assert by_planes[2] == {(0, 0)} and by_planes[3] == {(1, 0)} and by_planes[4] == {(1, 1)}
    # a fused and an unfused slab march, a tail layout, both forms of delta
    assert any(p["cc_int"] and p["cc_int_red"] for p in full)
    assert any(p["cc_int"] and not p["cc_int_red"] for p in full)
    assert any(p["ccgeo"] and C.sgeo(p, "ccgeo")["kc2"] != C.sgeo(p, "ccgeo")["kc"] for p in full)
    assert {p["ccf_edge_dot"] for p in full} == {0, 1}


# ---- b. rb2_shapes against the planner ---------------------------------------

def _rb2_pairs():
    out = [(C.rb2_line(c), RB2.layout(c.shape, c.kc)) for c in RB2.CASES]
    out += [(C.line(s), RB2.layout(s, fixed=False))
            for s in C.RB2_DEFAULT_SHAPES + [(1024, 1024, 512)]]
    return out


def test_rb2_shapes_model_agrees_with_the_planner(dump):
    pairs = _rb2_pairs()
    plans = dump([ln for ln, _ in pairs])
    for ln, lay in pairs:
        g = C.sgeo(plans[ln], "r2geo")
        assert (g["kc"], g["tiles_x"], g["tiles_y"], g["tiles_z"]) == \
            (lay.kc, lay.tiles_x, lay.tiles_y, len(lay.runs)), ln
        assert plans[ln]["rb2_interior"] == len(lay.interior), ln
    assert RB2.GRID_CAP == 2048 and "grid_cap" not in pairs[0][0]  # the dump's default


# ---- c. the seam tables' descriptions ------------------------------------------

NUM = {"one": 1, "two": 2, "three": 3, "second": 2, "third": 3, "fifth": 5}


def claims(what):
    """The checkable claims of a one-line description: (kind, value) pairs.
    Tile counts, the interior cells of the last tile, z runs."""
    out = []
    if m := re.search(r"runs (\d+(?: \+ \d+)+)", what):
        out.append(("runs", [int(v) for v in m.group(1).split(" + ")]))
    if "exactly one run" in what:
        out.append(("runs", [24]))
    if "two runs + one plane" in what:
        out.append(("runs", [24, 24, 1]))
    if re.search(r"halved to 3|kc = 3", what):
        out.append(("kc", 3))
    for n, ax in re.findall(r"\b(one|two|three) (?:full )?(x|y) tiles?\b", what):
        out.append((f"tiles_{ax}", NUM[n]))
    for n, ax in re.findall(r"\b(second|third) (x|y) tile\b", what):
        out.append((f"tiles_{ax}", NUM[n]))
    for n, rows in re.findall(r"\b(second|third|fifth) (16|8)-row tile\b", what):
        out.append((f"tiles_y@{rows}", NUM[n]))
    for n in re.findall(r"\b(one|two)-column\b", what):
        out.append(("last_x", NUM[n]))
    for n in re.findall(r"\b(one|two)-row\b", what):
        out.append(("last_y", NUM[n]))
    if m := re.search(r"\b(one|two)-plane remainder run", what):
        out.append(("remainder", NUM[m.group(1)]))
    return out


def holds(claim, g, tile, shape):
    """Does the SGeo dict g (tiles of tile[0] x tile[1] cells from cell 0) give
    what the claim says? last_x / last_y: interior cells of the last tile."""
    kind, want = claim
    if kind == "runs":
        return C.z_runs(g) == want
    if kind == "kc":
        return g["kc"] == want
    if kind == "remainder":
        planes = g["k1"] - g["k0"]
        return g["tiles_z"] > 1 and planes - (g["tiles_z"] - 1) * g["kc"] == want
    if kind in ("tiles_x", "tiles_y"):
        return g[kind] == want
    if kind == "last_x":
        return shape[0] - 1 - tile[0] * (g["tiles_x"] - 1) == want
    if kind == "last_y":
        return shape[1] - 1 - tile[1] * (g["tiles_y"] - 1) == want
    raise AssertionError(kind)


def _check(table_name, rows, geo_of, n_claims):
    """Every claim of every row against geo_of(shape) -> (SGeo dict, tile).
    n_claims is how many the table makes today, exactly: a description
    reworded so that claims() no longer reads it fails here, not silently."""
    fails, n = [], 0
    for shape, what in rows:
        for part, form in zip(what.split(S.CELL_FORM), ("today", "cell")):
            for claim in claims(part):
                g, tile = geo_of(shape, form, claim)
                if claim[0].startswith("tiles_y@"):
                    claim = ("tiles_y", claim[1])
                n += 1
                if not holds(claim, g, tile, shape):
                    fails.append(f"{table_name} {S.sid(shape)} ({form}): {claim} but "
                                 f"tiles {g['tiles_x']} x {g['tiles_y']}, runs {C.z_runs(g)}")
    assert not fails, "\n".join(fails)
    assert n == n_claims, f"{table_name}: {n} claims read, {n_claims} when this test was written"


def test_ccf_fixed_tables_say_what_the_planner_says(dump):
    """CCF_FIXED and EDGE_FIXED as test_gpu_cg_seams.py / test_gpu_ccf_edge_dot.py
    create them: cg_variant 1, CFD_HIP_CCF_KC_FIXED=1, one device, so the
    edge-sum form on 60 x 29 tiles. What CCF_FIXED says after S.CELL_FORM
    holds on the cell form's 60 x 28 tiles (CFD_HIP_CCF_EDGE_DOT=0)."""
    def geo_of(shape, form, claim):
        ln = C.ccf_fixed_line(shape, 0 if form == "cell" else None)
        plan = dump([ln])[ln]
        assert plan["ccf_edge_dot"] == (0 if form == "cell" else 1)
        return C.sgeo(plan, "ccgeo"), ((60, 28) if form == "cell" else (60, 29))

    _check("CCF_FIXED", S.CCF_FIXED, geo_of, 32)
    _check("EDGE_FIXED", C.edge_table("EDGE_FIXED"), geo_of, 31)
    # every 24-plane table shape gets 24-plane runs in both forms
    for shape in [s for s, _ in S.CCF_FIXED + C.edge_table("EDGE_FIXED")]:
        for form in ("today", "cell"):
            g, _ = geo_of(shape, form, None)
            assert g["kc"] == min(24, shape[2] - 2) and g["kc2"] == g["kc"], shape


def test_ccf_default_tables_say_what_the_planner_says(dump):
    def geo_of(shape, form, claim):
        cell = form == "cell"
        ln = C.line(shape, cg_variant=1, **({"CCF_EDGE_DOT": 0} if cell else {}))
        return C.sgeo(dump([ln])[ln], "ccgeo"), ((60, 28) if cell else (60, 29))

    rows = S.CCF_DEFAULT + C.edge_table("EDGE_DEFAULT")
    _check("CCF_DEFAULT", rows, geo_of, 3)
    _check("STEP_SHAPES", S.STEP_SHAPES[3:], geo_of, 4)  # the k_ccf step shapes
    for shape, _ in rows:  # "halved to 3", then clamped to the planes there are
        g, _ = geo_of(shape, "today", None)
        assert g["kc"] == min(3, shape[2] - 2), shape
    # the timed and the slab cases name kc = 3 at 62 x 30 x 27 too
    assert geo_of((62, 30, 27), "today", None)[0]["kc"] == 3


def test_textbook_tables_say_what_the_planner_says(dump):
    """The 128-column tilings: the CG sweeps at sweep_rows 8 and 16 (row
    counts named in the claim, else 16), k_pred3 / k_corr3's 128 x 16."""
    def sweeps(kchunk=0):
        def geo_of(shape, form, claim):
            rows = int(claim[0].split("@")[1]) if claim and "@" in claim[0] else 16
            ln = C.line(shape, sweep_rows=rows, **({"kchunk": kchunk} if kchunk else {}))
            return C.sgeo(dump([ln])[ln], "sgeo"), (128, rows)
        return geo_of

    def pc3_geo(shape, form, claim):
        ln = C.line(shape)
        return C.sgeo(dump([ln])[ln], "pgeo16"), (128, 16)

    _check("TEXTBOOK", S.TEXTBOOK, sweeps(), 6)
    for shape, kchunk, what in S.TEXTBOOK_KCHUNK:
        _check("TEXTBOOK_KCHUNK", [(shape, what)], sweeps(kchunk), 1)
    _check("STEP_SHAPES", S.STEP_SHAPES[:3], pc3_geo, 1)
    for shape, _ in S.CC_2D:  # 2-D: no k_ccf tiling, k_cc1 / k_cc2 run
        ln = C.line(shape, cg_variant=1)
        assert dump([ln])[ln]["ccgeo"] is None or C.sgeo(dump([ln])[ln], "ccgeo")["tiles_x"] == 0


def test_slab_cases_say_what_the_planner_says(dump):
    for shape, ranks, planes, what in S.SLAB_CASES:
        plans = list(dump(C.slab_lines(shape, ranks, cg_variant=1)).values())
        assert tuple(p["nz_local"] - 2 for p in plans) == planes, (shape, ranks)
        split = [C.sgeo(p, "cc_int")["tiles_x"] > 0 for p in plans]
        assert split == [n >= 3 for n in planes], (shape, ranks)
        assert [p["split_b"] for p in plans] == [int(s) for s in split]
        if "on every rank" in what:
            assert all(split)
        if "whole-march slabs of < 3 planes side by side" in what:
            assert not any(split)
        if "beside two that split" in what:
            assert sorted(split) == [False, True, True]
