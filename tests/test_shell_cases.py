"""The resident mode's packed shell layout and its host code
(cfd_amd/csrc/hip/shell_map.hpp: ShellMap, host_rows, host_max, host_hash,
shell_thread_count) pinned without a GPU. tests/native/shell_map_check.cpp is
compiled with g++ once under ASan + UBSan and once under TSan and run
directly on every shape of tests/shell_cases.py, depths 1 and 2:

  a. the packed order host_rows gathers in equals the numpy model's, which is
     written from the layout's description: every shell cell once, offsets
     0 .. total() - 1;
  b. (in the program) gather and scatter on 1, 2, 3, 7 and 16 threads with 1,
     4 and 5 fields against that order, sentinels outside the shell kept bit
     for bit; host_max against the sequential loop on NaNs, signed zeros and
     chunk edges; the guard's hashes independent of the thread count and
     changed by swaps;
  c. the guard's two hashes cover exactly the cells off the outer layer, each
     once, shown by flipping every cell of the small shapes in turn;
  d. shell_thread_count at its boundaries;
  e. the table reaches what its descriptions name.
"""
import shutil

import numpy as np
import pytest

from tests import shell_cases as S

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not present")

ALL = [s for s, _ in S.SHAPES]


@pytest.fixture(scope="module", params=list(S.SANITIZERS))
def checked(request, tmp_path_factory):
    """(directory of the program's files, its stdout lines) under one sanitizer
    build; the program's own checks (b) have passed when this returns."""
    d = tmp_path_factory.mktemp("shell_map_" + request.param)
    exe = S.build_check(d, request.param)
    return d, S.run_check(exe, d, ALL)


# ---- a. the packed order --------------------------------------------------------

@pytest.mark.parametrize("depth", [1, 2])
def test_packed_order_equals_the_model(checked, depth):
    d, _ = checked
    for shape in ALL:
        got = np.fromfile(d / f"order_{S.sid(shape)}_{depth}.bin", dtype=np.int64)
        want = S.packed_linear(shape, depth)
        assert got.size == want.size, (shape, got.size, want.size)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (shape, depth, int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))


@pytest.mark.parametrize("depth", [1, 2])
def test_model_holds_every_shell_cell_once(depth):
    """The model against the mask, two statements of the same shell: the
    packed cells are the mask's cells, each once, in (k, j, i) order."""
    for shape in ALL + [(5, 6, 1), (9, 5, 6)]:
        cells = S.packed_cells(shape, depth)
        mask = S.shell_mask(shape, depth)
        assert np.array_equal(cells, np.argwhere(mask)), shape
        nx, ny, nz = shape
        inner = (nx - 2 * depth) * (ny - 2 * depth) * (nz - 2 * depth if nz > 1 else 1)
        assert len(cells) == nx * ny * nz - inner


# ---- c. the guard's hashes ------------------------------------------------------

def test_hash_parts_cover_the_inner_cells_once(checked):
    d, _ = checked
    small = [s for s in ALL if np.prod(s) <= S.SMALL_CELLS]
    assert {s[2] == 1 for s in small} == {True, False} and len(small) >= 8
    for shape in small:
        cover = np.fromfile(d / f"cover_{S.sid(shape)}.bin", dtype=np.uint8).reshape(S.np_shape(shape))
        deep, layer1 = S.hash_parts(shape)
        assert np.array_equal(cover == 1, deep), shape      # the deep part alone
        assert np.array_equal(cover == 2, layer1), shape    # layer 1 alone
        assert not (cover == 3).any()                       # no cell in both
        assert np.array_equal(cover == 0, S.shell_mask(shape, 1)), shape  # no outer-layer cell
    for shape in [(5, 5, 1), (5, 5, 5)]:  # the minimum extents: one deep cell
        cover = np.fromfile(d / f"cover_{S.sid(shape)}.bin", dtype=np.uint8)
        assert int((cover == 1).sum()) == 1


# ---- d. the thread count ---------------------------------------------------------

def test_shell_thread_count_boundaries(checked):
    _, lines = checked
    got = {tuple(int(v) for v in ln.split()[1:4]): int(ln.split()[4])
           for ln in lines if ln.startswith("threads ")}
    edge = 1 << 18
    assert len(got) == 4 * 4 * 6
    for (cells, env, hw), n in got.items():
        if cells < edge:
            want = 1                    # below 2^18 cells one thread, whatever the override
        elif env > 0:
            want = env                  # the override replaces the count
        else:
            want = min(max(hw, 1), 16)  # at most 16 of the machine's threads
        assert n == want, (cells, env, hw, n)
    # the three boundaries, spelt out
    assert got[(edge - 1, 40, 256)] == 1 and got[(edge, 40, 256)] == 40
    assert got[(edge, 0, 16)] == 16 and got[(edge, 0, 17)] == 16 and got[(edge, 0, 8)] == 8
    assert got[(edge, 0, 0)] == 1 and got[(edge, 1, 256)] == 1 and got[(edge, 3, 1)] == 3


# ---- e. the table ----------------------------------------------------------------

def test_table_reaches_what_it_names():
    rows4 = {s: s[1] * s[2] * 4 for s in ALL}
    assert rows4[(5, 96, 96)] == 36864 and max(rows4.values()) > 32768  # the grid-stride trip
    staged1 = {s: 4 * int(S.shell_mask(s, 1).sum()) for s in ALL}
    assert staged1[(258, 130, 6)] == 280672 and max(staged1.values()) >= 1 << 18  # threaded host path
    # ... and only that one: every other shape stays on one thread, both depths
    assert sum(5 * int(S.shell_mask(s, 2).sum()) >= 1 << 18 for s in ALL) == 1
    for dim in (True, False):
        nxs = [s[0] for s in ALL if (s[2] == 1) == dim]
        assert any(n <= 64 for n in nxs) and any(64 < n <= 128 for n in nxs) and any(n > 128 for n in nxs)
    assert 64 in [s[0] for s in ALL] and 65 in [s[0] for s in ALL]
    for axis in range(3):  # the minimum extent on every axis, and none below it
        assert min(s[axis] for s in ALL if s[2] > 1) == 5
    assert min(s[0] for s, _ in S.SHAPES_2D) == 5 and min(s[1] for s, _ in S.SHAPES_2D) == 5
    assert all(s[2] == 1 for s, _ in S.SHAPES_2D) and all(s[2] > 1 for s, _ in S.SHAPES_3D)
    assert all(min(s[0], s[1], s[2] if s[2] > 1 else 9) == 4 for s in S.NO_FIT)
    # the GPU cases stay small
    assert max(int(np.prod(s)) for s in ALL) <= 202000


def test_inputs_are_finite_and_specials_land_in_the_shell():
    shape = (6, 7, 5)
    a = S.random_fields(shape, 1)
    b = S.plant_specials(S.random_fields(shape, 1), shape, 2)
    m = S.shell_mask(shape, 1)
    for name in S.FIELDS:
        assert np.isfinite(b[name]).all()
        changed = a[name].view(np.uint64) != b[name].view(np.uint64)
        assert not (changed & ~m).any()
        assert changed.any() == (name != "T")
    assert np.signbit(b["u"][b["u"] == 0.0]).any() and (~np.signbit(b["u"][b["u"] == 0.0])).any()
    assert ((np.abs(b["p"]) > 0) & (np.abs(b["p"]) < 2.3e-308)).any()
    s0, s1 = S.sentinels(shape, 0), S.sentinels(shape, 1, step=2)
    assert np.unique(np.concatenate([s0.ravel(), s1.ravel()])).size == 2 * s0.size
