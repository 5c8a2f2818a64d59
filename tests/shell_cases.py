"""TEST INFRASTRUCTURE ONLY -- the resident mode's boundary-shell transfers
(cfd_amd/csrc/hip/shell_io.hip, shell_map.hpp): the shape table of
tests/test_shell_cases.py and tests/test_gpu_shell_transfers.py, a numpy
statement of the packed layout, the random inputs, and the helpers that build
and run tests/native/shell_map_check.cpp.

Shapes are (nx, ny, nz); arrays are (nz, ny, nx), cells are (k, j, i). The
layout is written here from its description ("for each z plane k, for each
row j, the row's shell cells in x order"; a row is whole when its plane or the
row itself is within `depth` of a face, otherwise it holds its first and last
`depth` cells), not from the product's offset arithmetic.
"""
from __future__ import annotations

import os
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "native" / "shell_map_check.cpp"
HIP_DIR = ROOT / "cfd_amd" / "csrc" / "hip"

FIELDS = ("u", "v", "w", "p", "T")

# (shape, what it reaches). k_shell_io runs one wavefront per row: a whole
# row takes one trip of its x loop per 64 cells; its grid is capped at 8192
# workgroups of 4 waves, so more than 32768 rows x fields take a grid-stride
# trip; host_rows splits over threads from 2^18 staged cells.
SHAPES_2D = [
    ((5, 5, 1), "the minimum in x and y: one partial row, one deep cell"),
    ((6, 5, 1), "even nx at the minimum ny: two deep cells in one row"),
    ((64, 7, 1), "a whole row of exactly one trip of the x loop"),
    ((65, 9, 1), "one cell into the second trip of the x loop"),
    ((130, 5, 1), "a third trip of the x loop, one partial row"),
    ((7, 130, 1), "mostly partial rows: 126 of 130 at depth 2"),
]
SHAPES_3D = [
    ((5, 5, 5), "the minimum on every axis: one partial plane, one deep cell"),
    ((6, 7, 5), "three different extents, one partial plane"),
    ((65, 6, 7), "second trip of the x loop, partial planes with two partial rows"),
    ((130, 9, 6), "third trip of the x loop, two partial planes at depth 2"),
    ((5, 96, 96), "36864 rows at four fields: the grid-stride trip"),
    ((258, 130, 6), "280672 staged cells at depth 1, four fields: the threaded host path"),
]
SHAPES = SHAPES_2D + SHAPES_3D
# an extent of 4: the depth-2 shell does not fit, every step transfers in full
NO_FIT = [(4, 9, 9), (9, 4, 1), (9, 9, 4)]
# small enough to flip every cell in turn under the guard's hashes
SMALL_CELLS = 5000


def sid(shape):
    return "x".join(str(int(v)) for v in shape)


def np_shape(shape):
    nx, ny, nz = shape
    return (nz, ny, nx)


def shell_mask(shape, depth):
    """True on the cells within `depth` of a face (2-D: of an x or y face)."""
    nx, ny, nz = shape
    m = np.zeros((nz, ny, nx), bool)
    m[:, :, :depth] = m[:, :, nx - depth:] = True
    m[:, :depth, :] = m[:, ny - depth:, :] = True
    if nz > 1:
        m[:depth] = m[nz - depth:] = True
    return m


def packed_cells(shape, depth):
    """The (k, j, i) of every staged cell of one field in packed order, an
    (n, 3) int64 array, row by row as the layout's description has it."""
    nx, ny, nz = shape
    whole_i = np.arange(nx)
    part_i = np.concatenate([np.arange(depth), np.arange(nx - depth, nx)])
    out = []
    for k in range(nz):
        plane_whole = nz > 1 and (k < depth or k >= nz - depth)
        for j in range(ny):
            whole = plane_whole or j < depth or j >= ny - depth
            i = whole_i if whole else part_i
            out.append(np.stack([np.full(i.size, k), np.full(i.size, j), i], axis=1))
    return np.concatenate(out).astype(np.int64)


def packed_linear(shape, depth):
    """packed_cells as linear indices (k ny + j) nx + i."""
    nx, ny, _ = shape
    c = packed_cells(shape, depth)
    return (c[:, 0] * ny + c[:, 1]) * nx + c[:, 2]


def hash_parts(shape):
    """(deep, layer1) masks of the guard's two hashes: the cells with every
    index in [2, n-3], and the cells off the outer layer that are not deep
    (2-D: x and y only)."""
    outer = shell_mask(shape, 1)
    deep = ~shell_mask(shape, 2)
    return deep, ~outer & ~deep


SPECIALS = np.array([-0.0, 0.0, 5e-324, -5e-324, 2.2250738585072009e-308, -1.5e-310])


def random_fields(shape, seed, amp=0.1):
    """{name: (nz, ny, nx) array}: u, v, w, p uniform in (-amp, amp), T in
    300 +- 10 amp; every value finite."""
    rng = np.random.default_rng(seed)
    out = {}
    for name in FIELDS:
        a = amp * rng.uniform(-1.0, 1.0, np_shape(shape))
        out[name] = 300.0 + 10.0 * a if name == "T" else a
    return out


def plant_specials(fields, shape, seed):
    """Writes -0.0, +0.0 and subnormals into random depth-1 shell cells of
    u, v, w and p (in place); T keeps its values (a zero temperature is not a
    state a step is given)."""
    rng = np.random.default_rng(seed)
    cells = np.argwhere(shell_mask(shape, 1))
    for name in FIELDS[:4]:
        pick = cells[rng.choice(len(cells), size=min(len(cells), 2 * len(SPECIALS)), replace=False)]
        for n, (k, j, i) in enumerate(pick):
            fields[name][k, j, i] = SPECIALS[n % len(SPECIALS)]
    return fields


def sentinels(shape, field_index, step=0):
    """Distinct finite values no step produces, different in every cell,
    field and step: -(1e7 + cell + 1e6 field + step / 8)."""
    n = int(np.prod(shape))
    return -(1.0e7 + np.arange(n, dtype=np.float64) + 1.0e6 * field_index
             + step / 8.0).reshape(np_shape(shape))


# ---- the stand-alone host program ---------------------------------------------

SANITIZERS = {
    "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                   "-static-libasan", "-static-libubsan"],
    "tsan": ["-fsanitize=thread", "-static-libtsan"],
}


def build_check(outdir, sanitizer, include_dir=HIP_DIR):
    """Compiles shell_map_check.cpp with g++ under the named sanitizers, their
    runtimes linked statically; returns the executable."""
    exe = Path(outdir) / f"shell_map_check_{sanitizer}"
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
           "-pthread", *SANITIZERS[sanitizer], f"-I{include_dir}", str(SRC), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_check(exe, outdir, shapes):
    """Runs the program on the shapes; it checks what it can itself and leaves
    the rest as files in `outdir` (see its header). Returns its stdout lines."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("CFD_HIP_")}
    env.update(ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1",
               TSAN_OPTIONS="halt_on_error=1")
    out = subprocess.run([str(exe), str(outdir), str(SMALL_CELLS)] + [sid(s) for s in shapes],
                         capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0 and not out.stderr, (out.stdout[-1500:] + out.stderr)[-5000:]
    lines = out.stdout.splitlines()
    assert lines and lines[-1] == "SHELL_MAP_OK", lines[-5:]
    return lines


# ---- the GPU runs of tests/test_gpu_shell_transfers.py ------------------------

STEP_AMP, STEP_DT, STEP_NU = 0.1, 1e-4, 1e-2
FIELD_IDS = dict(u=0, v=1, w=2, p=3, T=4)  # HIP_FIELD_*


def step_case(shape, energy, seed=11):
    """(grid, flow_field, params) on the unit box with random_fields(shape,
    seed); energy: the energy equation and buoyancy on."""
    from cfd_amd import api
    nx, ny, nz = shape
    g = api.Grid(nx, ny, nz, 0.0, 1.0, 0.0, 1.0, 0.0, 1.0 if nz > 1 else 0.0)
    f = api.FlowField(nx, ny, nz)
    for name, a in random_fields(shape, seed, STEP_AMP).items():
        getattr(f, name)[...] = a
    f.rho[...] = 1.0
    p = api.validation_params(STEP_DT, STEP_NU)
    if energy:
        p.alpha = 2e-3
        p.beta = 3.333e-3
        p.T_ref = 300.0
        p.gravity[1] = -9.81
    return g, f, p


def fresh_shell(shape, step):
    """The values a caller's BC routine writes before step `step`: random on
    the whole array (only the depth-1 shell of it is used), with signed zeros
    and subnormals planted before step 2."""
    a = random_fields(shape, 100 + step, STEP_AMP)
    return plant_specials(a, shape, 200 + step) if step == 2 else a


def download_run(shape, resident, energy, steps=4, **config):
    """`steps` host-buffer steps of one context (dirty_faces = resident). Before
    every step the depth-1 shell of u, v, w, p, T takes fresh_shell's values;
    from the second step on (the resident ones) a resident run also sets every
    other host cell to sentinels(shape, field, step). Returns one record per
    step -- status, stats, `before` and `host` (copies of the host arrays
    before and after the step), `dev` (get_field of every field, resident
    runs) -- and the host arrays after a final hip_proj_sync_host (resident
    runs)."""
    from cfd_amd import _abi as A
    from cfd_amd import api
    g, f, p = step_case(shape, energy)
    ctx = api.HipProjection(*shape, dirty_faces=1 if resident else 0, **config)
    m1 = shell_mask(shape, 1)
    out = []
    try:
        for step in range(steps):
            fresh = fresh_shell(shape, step)
            sent = None
            if resident and step > 0:
                sent = {n: sentinels(shape, q, step) for q, n in enumerate(FIELDS)}
            for name in FIELDS:
                a = getattr(f, name)
                a[...] = np.where(m1, fresh[name], a if sent is None else sent[name])
            before = {n: getattr(f, n).copy() for n in FIELDS}
            st = A.SolverStats()
            s = ctx.step(f, g, p, st)
            rec = dict(status=s, stats=(st.max_velocity, st.max_pressure, st.max_temperature),
                       before=before, host={n: getattr(f, n).copy() for n in FIELDS}, dev=None)
            if resident:
                rec["dev"] = {n: ctx.get_field(FIELD_IDS[n]) for n in FIELDS}
            out.append(rec)
        synced = None
        if resident:
            ctx.sync_host(f)
            synced = {n: getattr(f, n).copy() for n in FIELDS}
    finally:
        ctx.close()
    return out, synced
