"""TEST INFRASTRUCTURE ONLY -- the case table of tests/test_tile_plan.py and
of `make_golden.py tile_plans`, and the helpers that build and run
tests/native/tile_plan_dump.cpp (the product's planner,
cfd_amd/csrc/hip/tile_plan.hpp, behind a stdin / JSON-lines front end).

A case is the line the dump program reads (its header explains the tokens;
sweep_rows and sweep_variant default to hip_proj_config_default's 16 and 15).
The fixture holds one digest per case, plan_digest() of everything the dump
program prints for it, so any field of any plan that moves changes it; and
the whole plans (integers, in the dump's layout) of the few READABLE cases,
which a reader can check by eye and a failure can show field by field.
"""
from __future__ import annotations

import ast
import hashlib
import json
import os
import shutil
import subprocess
from pathlib import Path

from tests import cg_seam_shapes as S
from tests import rb2_shapes as RB2

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "native" / "tile_plan_dump.cpp"
HIP_DIR = ROOT / "cfd_amd" / "csrc" / "hip"
FIXTURE = ROOT / "tests" / "golden" / "tile_plans.json"

GEO_FIELDS = ("nx ny nz px ps sz k0 k1 kc tiles_x tiles_y tiles_z lo_face hi_face kofs").split()
SGEO_FIELDS = ("nx ny nz px ps sz k0 k1 kc tiles_x tiles_y tiles_z kmode part_ofs part_total "
               "kofs kt0 kt1 xofs kc2 nz1").split()
SGEOS = ("sgeo sg_edge sg_int rgeo rg_in1 rg_edge rg_in2 rg_main rg_strip r2geo ccgeo cc_edge "
         "cc_int cc_int_red cc2_edge pgeo pgeo16").split()

BENCH_SHAPES = [(512, 512, 512), (1024, 1024, 512), (256, 256, 256), (128, 128, 128),
                (96, 96, 96)]
RB2_DEFAULT_SHAPES = [(96, 80, 70), (70, 66, 40), (96, 96, 48)]  # test_rb2_shapes.py


def _assigned(test_file, name):
    """The expression assigned to `name` at the top of tests/<test_file>, read
    from the source: the GPU test modules are not imported here."""
    for node in ast.parse((ROOT / "tests" / test_file).read_text()).body:
        if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", None) == name:
            return node.value
    raise AssertionError(f"{test_file}: {name} not found")


def edge_table(name):
    """EDGE_FIXED / EDGE_DEFAULT of test_gpu_ccf_edge_dot.py: [(shape, what)]."""
    return ast.literal_eval(_assigned("test_gpu_ccf_edge_dot.py", name))


def rb2_suite_shapes():
    """The shapes of test_gpu_rb2.SHAPES."""
    return sorted({ast.literal_eval(item.elts[0])
                   for item in _assigned("test_gpu_rb2.py", "SHAPES").elts})


def line(shape, **kw):
    """One case line; lower-case keywords are inputs, upper-case ones switches."""
    return " ".join([f"shape={S.sid(shape)}"] + [f"{k}={v}" for k, v in kw.items()])


def slab_lines(shape, ranks, **kw):
    return [line(shape, ranks=ranks, rank=r, **kw) for r in range(ranks)]


def rb2_line(case: RB2.Case):
    kc = {"RB2_KC": case.kc} if case.kc else {}
    return line(case.shape, **kc, RB2_KC_FIXED=1)


def ccf_fixed_line(shape, edge_dot=None):
    """A shape of CCF_FIXED / EDGE_FIXED as its GPU test creates it
    (edge_dot None: CFD_HIP_CCF_EDGE_DOT unset, the default)."""
    kw = {} if edge_dot is None else {"CCF_EDGE_DOT": edge_dot}
    return line(shape, cg_variant=1, CCF_KC_FIXED=1, **kw)


def readable():
    """The cases whose whole plans the fixture holds: the flagship shapes, an
    8-rank slab, a seam shape under the default run length, a k_rb2 case."""
    return [line((512, 512, 512), cg_variant=1), line((1024, 1024, 512)),
            line((512, 512, 512), ranks=8, rank=0, cg_variant=1),
            line((62, 30, 27), cg_variant=1), rb2_line(RB2.CASES[5])]


def cases():
    """Every case line of the fixture, in order, without duplicates."""
    out = []
    # the benchmark shapes
    out += [line((512, 512, 512), cg_variant=v) for v in (0, 1)]
    out += [line(s) for s in BENCH_SHAPES[1:]]
    # the legal minimum and 2-D
    out += [line(s, cg_variant=v) for s in ((3, 3, 1), (4, 4, 3), (129, 17, 1)) for v in (0, 1)]
    # k_rb1's remainder strip at its edges (R = nx mod 124 = 0, 1, 2, 28, 29), on and off
    strip = [(nx, 30, 40) for nx in (248, 249, 250, 276, 277)]
    out += [line(s) for s in strip] + [line(s, RB1_STRIP=0) for s in strip]
    out += [line((250, 30, 40), RB1_TC=tc) for tc in (32, 16)]
    out += [line((250, 30, 40), RB1_KC=32), line((512, 512, 512), RB1_KC=32)]
    # k_rb2: the interior-tile cases as their GPU tests create them, and the
    # product's own run lengths
    out += [rb2_line(c) for c in RB2.CASES]
    out += [line(s) for s in RB2_DEFAULT_SHAPES + [(250, 30, 40)] + rb2_suite_shapes()]
    # k_ccf: the seam tables in both forms of delta
    fixed = [s for s, _ in S.CCF_FIXED] + [s for s, _ in edge_table("EDGE_FIXED")]
    out += [ccf_fixed_line(s, e) for s in fixed for e in (None, 1, 0)]
    default = [s for s, _ in S.CCF_DEFAULT] + [s for s, _ in edge_table("EDGE_DEFAULT")]
    out += [line(s, cg_variant=1, **kw) for s in default
            for kw in ({}, {"CCF_EDGE_DOT": 1}, {"CCF_EDGE_DOT": 0})]
    # test_gpu_cg_single_reduction.py's tail layers at 65^3
    n65 = (65, 65, 65)
    out += [line(n65, cg_variant=1, CCF_KC=24, CCF_KC_FIXED=1)]
    out += [line(n65, cg_variant=1, CCF_TAIL=t, CCF_KC2=k, CCF_KC=24, CCF_KC_FIXED=1)
            for t, k in ((1, 12), (2, 5))]
    # Z-slabs, every rank, both CG forms
    for v in (0, 1):
        for ranks in (2, 4, 8):
            out += slab_lines((512, 512, 512), ranks, cg_variant=v)
        out += slab_lines((130, 130, 130), 8, cg_variant=v)
        for shape, ranks, _, _ in S.SLAB_CASES:
            out += slab_lines(shape, ranks, cg_variant=v)
        # 2, 3 and 4 interior planes per rank, and 4 beside 3: the thresholds
        # of split_b / the k_ccf split (3) and split_rb (4)
        for nz in (6, 8, 10, 9):
            out += slab_lines((62, 30, nz), 2, cg_variant=v)
    for kw in ({"RB_SPLIT": 0}, {"CCF_SLAB_FUSED": 0}):
        out += slab_lines((62, 30, 27), 3, cg_variant=1, **kw)
        out += [line((512, 512, 512), ranks=8, rank=r, cg_variant=1, **kw) for r in (0, 3, 7)]
    # the configuration
    out += [line(s, sweep_rows=r) for s in ((512, 512, 512), (129, 17, 1)) for r in (4, 5, 8, 16)]
    out += [line((96, 96, 96), sweep_rows=r, only="sweep_variants") for r in (8, 16)]
    out += [line(s, kchunk=k) for s in ((512, 512, 512), (130, 18, 7), (129, 17, 7))
            for k in (2, 3, 1000)]
    out += [line(s, sweep_rows=r, kchunk=k) for s, k, _ in S.TEXTBOOK_KCHUNK for r in (8, 16)]
    # other switches that enter the plan
    out += [line((512, 512, 512), cg_variant=1, ROW_PAD=8), line((62, 30, 27), ROW_PAD=8)]
    out += [line((96, 96, 96), cg_variant=1, FIELD_STAGGER=v) for v in (0, 1000)]
    out += [line((96, 96, 96), PC3=v) for v in (0, 2, 3, 4)]
    # thresholds inside the rules: k_ccf's slab run length at 100 / 101 planes,
    # k_rb2's three-run rule at 383 / 384 planes, the smallest grids k_rb2 and
    # k_ccf take and the ones just below
    out += [line((62, 30, nz), ranks=2, rank=0, cg_variant=1) for nz in (202, 204)]
    out += [line((1024, 1024, nz)) for nz in (385, 386)]
    out += [line(s, cg_variant=1) for s in ((7, 8, 5), (8, 7, 5), (8, 8, 5), (3, 4, 3), (4, 3, 3))]
    # another grid_cap (104 CUs)
    out += [line((512, 512, 512), cg_variant=v, grid_cap=832) for v in (0, 1)]
    out += [line((96, 96, 96), grid_cap=832)]
    return list(dict.fromkeys(out))


def build_dump(outdir, include_dir=HIP_DIR):
    """Compiles the dump program under ASan + UBSan, their runtimes linked
    statically (the program then needs them nowhere in the order of its shared
    objects, whatever else the environment loads); returns the executable."""
    exe = Path(outdir) / "tile_plan_dump"
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan",
           f"-I{include_dir}", str(SRC), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_dump(exe, lines):
    """{case line: plan} of the given lines. The program runs in the caller's
    environment less its CFD_HIP_* switches: a case sets its own."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("CFD_HIP_")}
    env.update(ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True,
                         text=True, env=env, timeout=300)
    assert out.returncode == 0 and not out.stderr, (out.stdout[-1000:] + out.stderr)[-4000:]
    plans = [json.loads(s) for s in out.stdout.splitlines()]
    assert [p["case"] for p in plans] == list(lines)
    return {p.pop("case"): p for p in plans}


def sgeo(plan, name):
    """The named SGeo of a plan as a dict (all zeros for an unused one)."""
    v = plan[name] or [0] * len(SGEO_FIELDS)
    return dict(zip(SGEO_FIELDS, v))


def z_runs(g):
    """The z-run lengths of a k_ccf tiling (ccf_layout: nz1 layers of kc
    planes, then layers of kc2) over its planes."""
    lo, hi = (g["kt0"], g["kt1"]) if g["kmode"] == 2 else (g["k0"], g["k1"])
    runs, k = [], lo
    for tz in range(g["tiles_z"]):
        n = g["kc"] if tz < g["nz1"] else g["kc2"]
        runs.append(min(n, hi - k))
        k += n
    return runs


def plan_digest(plan):
    """sha256[:16] of a plan's canonical JSON (sorted keys, no spaces)."""
    return hashlib.sha256(json.dumps(plan, sort_keys=True, separators=(",", ":"))
                          .encode()).hexdigest()[:16]


def write_fixture(path=FIXTURE, include_dir=HIP_DIR, tmpdir=None):
    """Regenerates the fixture from the dump program (make_golden.py tile_plans)."""
    import tempfile
    assert shutil.which("g++"), "g++ not present"
    with tempfile.TemporaryDirectory(dir=tmpdir) as d:
        plans = run_dump(build_dump(d, include_dir), cases())
    one = lambda v: json.dumps(v, separators=(",", ":"))  # noqa: E731
    full = ",\n".join(f"{one(c)}:{one(plans[c])}" for c in readable())
    dig = ",\n".join(f"{one(c)}:{one(plan_digest(p))}" for c, p in plans.items())
    Path(path).write_text('{"plans":{\n' + full + '\n},\n"digests":{\n' + dig + "\n}}\n")
    return len(plans)
