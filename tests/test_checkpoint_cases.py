"""The tables of tests/checkpoint_cases.py against their own claims, and the
CRC kernel's decomposition (lane registers 64 values apart, moved to the chunk
end, to the field end, XORed) against zlib. CPU only: what the device tests
of tests/test_gpu_checkpoint.py run is decided here."""
import re
import zlib
from pathlib import Path

import numpy as np
import pytest

from cfd_amd import api
from oracle import checkpoint_format as fmt
from tests import checkpoint_cases as K
from tests.test_checkpoint import grid_dict, nondefault_params, params_dict

HIP = Path(__file__).resolve().parents[1] / "cfd_amd" / "csrc" / "hip" / "checkpoint_hip.hip"


def raw0(b):
    """The zero-register CRC of b; test_checkpoint.py::
    test_crc_join_arithmetic_matches_zlib joins it into zlib.crc32."""
    return zlib.crc32(b, 0xFFFFFFFF) ^ 0xFFFFFFFF


def test_constants_match_the_kernel_source():
    src = HIP.read_text()
    chunk = re.search(r"constexpr long long CRC_CHUNK = (\d+);", src)
    waves = re.search(r"constexpr int CRC_WAVES = (\d+);", src)
    assert chunk and waves, "checkpoint_hip.hip no longer declares CRC_CHUNK / CRC_WAVES"
    assert int(chunk.group(1)) == K.CRC_CHUNK
    assert int(waves.group(1)) == K.CRC_WAVES
    # the wavefront width: the launch bound, the lane mask, the stride, the shuffle width
    assert re.search(r"__launch_bounds__\((\d+) \* CRC_WAVES\)", src).group(1) == str(K.LANES)
    assert f"threadIdx.x & {K.LANES - 1}" in src
    assert f"s += {K.LANES})" in src and f"i += {K.LANES};" in src
    assert f"off, {K.LANES})" in src
    # the skip between two values of a lane, and the default staging size
    assert f"chk_xpow_bytes({8 * K.LANES - 8})" in src
    assert "cap = 64u << 20" in src and K.STAGE_DEFAULT == 64 << 20
    assert f'getenv("{K.STAGE_KNOB}")' in src


@pytest.mark.parametrize("shape", K.CRC_SHAPE_LIST, ids=K.sid)
def test_shape_has_the_property_it_claims(shape):
    plan = K.crc_plan(shape)
    claim = K.CLAIMS[shape]
    assert claim, shape
    for key, want in claim.items():
        assert plan[key] == want, (shape, key, plan[key], want)
    # the text names n: it is the product
    m = re.search(r"n = (\d+)", K.CRC_SHAPES[shape])
    if m:
        assert int(m.group(1)) == plan["n"] == shape[0] * shape[1] * shape[2]


def test_every_shape_has_claims_and_the_issue_shapes_are_there():
    assert set(K.CLAIMS) == set(K.CRC_SHAPES)
    for shape in [(3, 3, 1), (5, 4, 3), (8, 8, 1), (13, 5, 1), (3, 3, 20), (63, 5, 3), (65, 7, 3),
                  (91, 90, 1), (128, 64, 1), (3, 2731, 1), (2731, 3, 1), (181, 181, 1),
                  (17, 41, 47), (32, 32, 32), (9, 3641, 1), (67, 35, 18), (33, 33, 33),
                  (17, 9, 5), (130, 70, 3), (64, 64, 1)]:
        assert shape in K.CRC_SHAPES, shape
    assert set(K.ROW_PAD_SHAPES) <= set(K.CRC_SHAPES) and len(K.ROW_PAD_SHAPES) == 3


def test_table_covers_every_property_class():
    plans = [K.crc_plan(s) for s in K.CRC_SHAPES]

    def some(pred):
        return any(pred(p) for p in plans)

    assert some(lambda p: p["n"] < K.LANES and p["idle_lanes"] > 0)
    assert some(lambda p: p["n"] == K.LANES)
    assert some(lambda p: p["n"] == K.LANES + 1)
    assert some(lambda p: p["plane_wrap"] and p["planes_per_stride"] >= 2)
    for last in (1, K.CRC_CHUNK - 2, K.CRC_CHUNK):
        assert some(lambda p: p["last_chunk_values"] == last), last
    for chunks in (K.CRC_WAVES, K.CRC_WAVES + 1):
        assert some(lambda p: p["chunks"] == chunks), chunks
    assert some(lambda p: p["chunks"] == K.CRC_WAVES and p["last_chunk_values"] < K.CRC_CHUNK)
    assert some(lambda p: p["workgroups"] == 2 and p["last_group_waves"] == 1
                and p["last_chunk_values"] == 1)
    assert some(lambda p: p["padded_rows"]) and some(lambda p: not p["padded_rows"])
    assert some(lambda p: p["row_wrap"] and not p["plane_wrap"])
    assert some(lambda p: not p["row_wrap"])


def test_patterns_are_what_they_say():
    shape = (3, 2731, 1)  # n = 8193: both chunk-edge indices exist
    P = K.patterns(shape, 3)
    assert tuple(P) == K.PATTERNS
    bits = {k: v.view(np.uint64).ravel() for k, v in P.items()}
    n = bits["zeros"].size
    assert all(v.shape == (1, 2731, 3) and v.dtype == np.float64 for v in P.values())
    assert not bits["zeros"].any()
    assert np.flatnonzero(bits["only_first"]).tolist() == [0]
    assert np.flatnonzero(bits["only_last"]).tolist() == [n - 1]
    assert np.flatnonzero(bits["only_chunk_edges"]).tolist() == [K.CRC_CHUNK - 1, K.CRC_CHUNK]
    assert np.all(P["constant"] == 1.25)
    # a field below the chunk edge has no edge value: the pattern is all zero
    assert not K.patterns((5, 4, 3))["only_chunk_edges"].view(np.uint64).any()
    # the random patterns reach the classes a float comparison would miss
    r = K.random_bits((67, 35, 18), 0)
    rb = r.view(np.uint64)
    expo = (rb >> np.uint64(52)) & np.uint64(0x7FF)
    assert np.isnan(r).any() and (expo == 0).any()
    assert len({int(v) for v in rb[np.isnan(r)] & np.uint64((1 << 52) - 1)}) > 1  # NaN payloads
    assert not np.array_equal(K.random_bits((5, 4, 3), 0).view(np.uint64),
                              K.random_bits((5, 4, 3), 1).view(np.uint64))
    # -0.0, the infinities, a subnormal and both kinds of NaN are in every
    # field, the smallest included, and the packed bytes carry their bits
    for s in K.CRC_SHAPES:
        a = K.random_bits(s, 0)
        got = a.view(np.uint64).ravel()[K.special_positions(a.size)]
        assert got.tolist() == list(K.SPECIAL_BITS), s
        assert np.frombuffer(K.packed_bytes(a), "<u8")[K.special_positions(a.size)].tolist() == \
            list(K.SPECIAL_BITS), s
    flat = K.random_bits((3, 3, 1), 0).ravel()
    assert np.signbit(flat[1]) and flat[1] == 0.0 and np.isinf(flat[2]) and np.isnan(flat[-1])


@pytest.mark.parametrize("shape", K.CRC_SHAPE_LIST, ids=K.sid)
def test_lane_crc_matches_zlib(shape):
    P = K.patterns(shape, 1)
    blobs = [K.packed_bytes(a) for a in P.values()]
    assert dict(zip(P, K.lane_crcs(blobs, shape))) == dict(zip(P, map(raw0, blobs)))
    assert K.lane_crc(blobs[0], shape) == raw0(blobs[0])  # the one-field form


def test_lane_crc_sees_a_lane_shift_off_by_one_value():
    """The planted bug: every lane moved one value too far towards the chunk
    end. The comparison above must not be blind to it."""
    for shape in [(3, 3, 1), (13, 5, 1), (3, 2731, 1), (33, 33, 33)]:
        b = K.packed_bytes(K.random_bits(shape, 2))
        assert K.lane_crc(b, shape, lane_bias=1) != raw0(b), shape
        crc, lanes, chunks = K.lane_crc(b, shape, detail=True)
        plan = K.crc_plan(shape)
        assert crc == raw0(b) and lanes.shape == (plan["chunks"], K.LANES)
        assert chunks.shape == (plan["chunks"],)
        # a lane with nothing contributes nothing
        if plan["idle_lanes"]:
            assert not lanes[-1, K.LANES - plan["idle_lanes"]:].any()


@pytest.mark.parametrize("case", K.STAGE_CASES, ids=K.stage_id)
def test_stage_case_matches_the_formula(case):
    shape, nbytes, kp, nchunk = case
    nx, ny, nz = shape
    assert kp == max(1, min(nz, nbytes // (nx * ny * 8))) == K.stage_planes(shape, nbytes)
    assert nchunk == -(-nz // kp) == len(K.stage_chunks(shape, nbytes))
    chunks = K.stage_chunks(shape, nbytes)
    assert sum(nk for _, nk in chunks) == nz and chunks[0][0] == 0
    if nchunk > 1:
        assert any(k0 > 0 for k0, _ in chunks)
        if nz % kp:
            k0, nk = chunks[-1]
            assert k0 > 0 and nk == nz % kp < kp


def test_stage_cases_cover_the_pipeline():
    cases = K.STAGE_CASES
    shapes = {c[0] for c in cases}
    assert shapes == {(20, 14, 11), (67, 35, 18), (23, 19, 1)}
    plane = lambda s: s[0] * s[1] * 8  # noqa: E731
    tails = [K.stage_chunks(c[0], c[1])[-1] for c in cases if c[3] > 1]
    assert any(c[2] == 1 and c[3] > 1 and c[1] >= plane(c[0]) for c in cases)  # plane per chunk
    assert any(c[3] > 1 and c[3] % 2 == 1 and c[2] > 1 for c in cases)  # odd: buffers alternate
    assert any(c[3] > 1 and c[3] % 2 == 0 for c in cases)
    assert any(k0 > 0 and nk == 1 and c[2] > 1 for c, (k0, nk) in
               zip([c for c in cases if c[3] > 1], tails))              # a tail of one plane
    assert any(k0 > 0 and 1 < nk < c[2] for c, (k0, nk) in
               zip([c for c in cases if c[3] > 1], tails))              # a longer short tail
    assert any(c[1] < plane(c[0]) and c[0][2] > 1 for c in cases)        # clamps to one plane
    assert any(c[1] < plane(c[0]) and c[0][2] == 1 for c in cases)       # ... in 2-D
    # the default: unset and non-positive values are 64 MiB
    assert K.stage_planes((1024, 1024, 9)) == K.stage_planes((1024, 1024, 9), 0) == \
        K.stage_planes((1024, 1024, 9), -5) == 8
    assert K.stage_chunks((1024, 1024, 9)) == [(0, 8), (8, 1)]
    assert len(K.stage_chunks((512, 512, 512))) == 16


@pytest.mark.parametrize("shape", [(20, 14, 11), (23, 19, 1)], ids=K.sid)
def test_format_oracle_round_trips_random_bits(shape):
    """oracle.checkpoint_format carries every bit pattern: the expected files
    of the device tests are built with it from random_bits fields."""
    nx, ny, nz = shape
    g = api.Grid(nx, ny, nz, 0.0, 1.0, 0.0, 2.0, 0.0, 0.5 if nz > 1 else 0.0)
    fields = {k: K.random_bits(shape, q) for q, k in enumerate(fmt.FIELDS)}
    blob = fmt.encode(grid_dict(g), fields, params_dict(nondefault_params()), 0.75, b"projection_hip",
                      b"run", None)
    d = fmt.decode(blob)
    assert d["crc_ok"] is True
    for k in fmt.FIELDS:
        assert np.array_equal(d["fields"][k].view(np.uint64), fields[k].view(np.uint64)), k
    off = fmt.field_offsets(blob)
    for k in fmt.FIELDS:
        assert blob[off[k]:off[k] + 8 * nx * ny * nz] == K.packed_bytes(fields[k]), k
