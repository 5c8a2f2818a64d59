"""Shapes, field contents and staging sizes that pin the device restart files
(cfd_amd/csrc/hip/checkpoint_hip.hip), shared by tests/test_checkpoint_cases.py
(the tables against their own claims and the kernel's CRC decomposition
against zlib, on the CPU) and tests/test_gpu_checkpoint.py (the device against
zlib, the format oracle and the host writer). Pure Python + numpy.

k_crc_raw: one wavefront (LANES lanes) per chunk of CRC_CHUNK consecutive
values of the packed field, CRC_WAVES chunks per workgroup. Lane l folds the
values l, l + 64, l + 128, ... of its chunk into one register (504 zero bytes
skipped between two of them), the registers are moved to the chunk end and
XORed, the chunk to the field end and XORed. lane_crc() below restates that
without tables.

The staging pipeline moves max(1, min(nz, bytes // (nx ny 8))) planes per
chunk through two pinned buffers, chunk m of the six-field stream through
buffer m & 1; bytes is CFD_HIP_CHK_STAGE_BYTES, 64 MiB by default.
"""
from __future__ import annotations

import numpy as np

CRC_CHUNK = 8192  # values per wavefront
LANES = 64
CRC_WAVES = 4     # wavefronts (chunks) per workgroup
POLY = 0xEDB88320
STAGE_DEFAULT = 64 << 20
STAGE_KNOB = "CFD_HIP_CHK_STAGE_BYTES"


def sid(shape):
    return "x".join(str(v) for v in shape)


def crc_plan(shape):
    """What k_crc_raw makes of a packed (nx, ny, nz) field."""
    nx, ny, nz = shape
    n = nx * ny * nz
    chunks = -(-n // CRC_CHUNK)
    groups = -(-chunks // CRC_WAVES)
    last = n - (chunks - 1) * CRC_CHUNK
    return {
        "n": n,
        "chunks": chunks,
        "workgroups": groups,
        "last_chunk_values": last,
        # lanes of the last chunk whose first index is already past the end
        "idle_lanes": max(0, LANES - last),
        # wavefronts of the last workgroup that own a chunk at all
        "last_group_waves": chunks - (groups - 1) * CRC_WAVES,
        # one lane stride of 64 values crosses a row end more than once ...
        "row_wrap": nx < LANES,
        # ... and a plane end more than once
        "plane_wrap": nx * ny < LANES,
        "planes_per_stride": LANES // (nx * ny),
        # the device row pitch is nx rounded up to 8 doubles
        "padded_rows": (nx + 7) // 8 * 8 > nx,
    }


# (nx, ny, nz) -> what the shape reaches; tests/test_checkpoint_cases.py holds
# every entry to the properties its text claims (CLAIMS below)
CRC_SHAPES = {
    (3, 3, 1): "n = 9 < 64: 55 lanes with nothing",
    (5, 4, 3): "n = 60: four lanes with nothing, a stride crosses all three planes",
    (8, 8, 1): "n = 64: one value per lane, pitch = nx",
    (13, 5, 1): "n = 65: lane 0 alone holds two values",
    (3, 3, 20): "n = 180: one lane stride crosses 7 planes",
    (63, 5, 3): "nx one below the wavefront width",
    (65, 7, 3): "nx one above the wavefront width",
    (91, 90, 1): "n = 8190: two short of the chunk",
    (128, 64, 1): "n = 8192: the exact chunk, pitch = nx",
    (3, 2731, 1): "n = 8193: a second chunk that holds one value, rows of 3",
    (2731, 3, 1): "n = 8193: a second chunk that holds one value, long rows",
    (181, 181, 1): "n = 32761: seven short of four chunks",
    (17, 41, 47): "n = 32759: nine short of four chunks, 3-D with short rows",
    (32, 32, 32): "n = 32768: exactly one workgroup of four chunks, pitch = nx",
    (9, 3641, 1): "n = 32769: a second workgroup whose only active wave holds one value",
    (67, 35, 18): "n = 42210: six chunks, row pitch 72 (128 in the DST table)",
    (33, 33, 33): "n = 35937: five chunks",
    (17, 9, 5): "n = 765: one chunk, rows shorter than a wavefront",
    (130, 70, 3): "n = 27300: four chunks, rows longer than two wavefronts",
    (64, 64, 1): "n = 4096: rows of exactly one wavefront, pitch = nx",
}
CRC_SHAPE_LIST = list(CRC_SHAPES)

# shape -> the crc_plan entries its text stands for
CLAIMS = {
    (3, 3, 1): dict(n=9, chunks=1, idle_lanes=55, plane_wrap=True),
    (5, 4, 3): dict(n=60, idle_lanes=4, plane_wrap=True, planes_per_stride=3),
    (8, 8, 1): dict(n=64, idle_lanes=0, chunks=1, padded_rows=False),
    (13, 5, 1): dict(n=65, idle_lanes=0, chunks=1, row_wrap=True),
    (3, 3, 20): dict(n=180, plane_wrap=True, planes_per_stride=7),
    (63, 5, 3): dict(row_wrap=True, plane_wrap=False, padded_rows=True),
    (65, 7, 3): dict(row_wrap=False, padded_rows=True),
    (91, 90, 1): dict(n=8190, chunks=1, last_chunk_values=8190),
    (128, 64, 1): dict(n=8192, chunks=1, last_chunk_values=8192, padded_rows=False),
    (3, 2731, 1): dict(n=8193, chunks=2, last_chunk_values=1, idle_lanes=63, row_wrap=True),
    (2731, 3, 1): dict(n=8193, chunks=2, last_chunk_values=1, idle_lanes=63, row_wrap=False),
    (181, 181, 1): dict(n=32761, chunks=4, workgroups=1, last_chunk_values=8185),
    (17, 41, 47): dict(n=32759, chunks=4, workgroups=1, last_chunk_values=8183, row_wrap=True),
    (32, 32, 32): dict(n=32768, chunks=4, workgroups=1, last_chunk_values=8192,
                       padded_rows=False),
    (9, 3641, 1): dict(n=32769, chunks=5, workgroups=2, last_group_waves=1,
                       last_chunk_values=1),
    (67, 35, 18): dict(n=42210, chunks=6, workgroups=2, padded_rows=True),
    (33, 33, 33): dict(n=35937, chunks=5, workgroups=2, last_group_waves=1),
    (17, 9, 5): dict(n=765, chunks=1, row_wrap=True, plane_wrap=False),
    (130, 70, 3): dict(n=27300, chunks=4, row_wrap=False, padded_rows=True),
    (64, 64, 1): dict(n=4096, chunks=1, row_wrap=False, padded_rows=False),
}

# the shapes that run once more under CFD_HIP_ROW_PAD=8: short rows in 3-D, a
# pitch that was nx before the pad, several chunks in 3-D
ROW_PAD_SHAPES = [(5, 4, 3), (32, 32, 32), (67, 35, 18)]

PATTERNS = ("random_bits", "zeros", "only_first", "only_last", "only_chunk_edges", "constant")


def _from_bits(bits, shape):
    nx, ny, nz = shape
    a = np.ascontiguousarray(bits, dtype=np.uint64).view(np.float64).reshape(nz, ny, nx)
    a.setflags(write=False)
    return a


# -0.0, +inf, -inf, the smallest subnormal, a signalling and a quiet NaN with payloads
SPECIAL_BITS = (0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000, 0x0000000000000001,
                0x7FF0000000000001, 0xFFF8000000000ABC)


def special_positions(n):
    """Where random_bits plants SPECIAL_BITS (n >= 9), spread over the field."""
    return [(q * n) // len(SPECIAL_BITS) + 1 for q in range(len(SPECIAL_BITS))]


def random_bits(shape, seed):
    """Uniform 64-bit patterns as float64 (NaN payloads and subnormals come by
    themselves) with SPECIAL_BITS planted, so that -0.0 and the infinities
    occur in every field; read-only."""
    nx, ny, nz = shape
    n = nx * ny * nz
    rng = np.random.default_rng([nx, ny, nz, seed])
    bits = rng.integers(0, 2 ** 64, size=n, dtype=np.uint64)
    bits[special_positions(n)] = np.array(SPECIAL_BITS, dtype=np.uint64)
    return _from_bits(bits, shape)


def patterns(shape, seed=0):
    """name -> float64 array (nz, ny, nx), built from its bits, read-only."""
    nx, ny, nz = shape
    n = nx * ny * nz
    one = np.float64(1.0).view(np.uint64)
    out = {"random_bits": random_bits(shape, seed), "zeros": _from_bits(np.zeros(n, np.uint64), shape)}
    for name, idx in (("only_first", [0]), ("only_last", [n - 1]),
                      ("only_chunk_edges", [i for i in (CRC_CHUNK - 1, CRC_CHUNK) if i < n])):
        b = np.zeros(n, np.uint64)
        b[idx] = one + np.uint64(seed + 1)
        out[name] = _from_bits(b, shape)
    out["constant"] = _from_bits(np.full(n, np.float64(1.25).view(np.uint64)), shape)
    assert tuple(out) == PATTERNS
    return out


def packed_bytes(a):
    return np.ascontiguousarray(a, dtype="<f8").tobytes()


# ---------------------------------------------------------------------------
# the kernel's decomposition, without tables
# ---------------------------------------------------------------------------
def gf_mul(a, b):
    """a * b mod the CRC polynomial, reflected bit order (chk_gf_mul); a and b
    uint32 arrays of one shape, or scalars."""
    a = np.array(a, dtype=np.uint32)
    b = np.broadcast_to(np.array(b, dtype=np.uint32), a.shape).copy()
    r = np.zeros_like(a)
    top, one, poly = np.uint32(0x80000000), np.uint32(1), np.uint32(POLY)
    for _ in range(32):
        r ^= np.where(a & top, b, np.uint32(0))
        a = a << one
        b = np.where(b & one, (b >> one) ^ poly, b >> one)
    return r


def xpow_bytes(n):
    """x^(8 n): the multiplier that moves a register past n zero bytes."""
    r, sq = np.uint32(0x80000000), np.uint32(0x00800000)
    while n:
        if n & 1:
            r = gf_mul(r, sq)
        sq = gf_mul(sq, sq)
        n >>= 1
    return int(r)


def _fold_bytes(acc, words):
    """The zero-register CRC step over one little-endian 8-byte value per
    register, bit by bit."""
    one, poly = np.uint32(1), np.uint32(POLY)
    for half in (words & np.uint64(0xFFFFFFFF), words >> np.uint64(32)):
        acc = acc ^ half.astype(np.uint32)  # four bytes at once: the 32 bit steps follow
        for _ in range(32):
            acc = np.where(acc & one, (acc >> one) ^ poly, acc >> one)
    return acc


def _lane_parts(blobs, shape, lane_bias):
    """The per-lane registers at their chunk's end (B, chunks, 64) and the
    per-chunk registers at the field end (B, chunks) of B packed fields of
    one shape: a chunk depends on nothing outside it, so the fields march
    side by side."""
    nx, ny, nz = shape
    n = nx * ny * nz
    chunks = -(-n // CRC_CHUNK)
    steps = CRC_CHUNK // LANES
    words = np.zeros((len(blobs), chunks * CRC_CHUNK), np.uint64)
    for q, b in enumerate(blobs):
        assert len(b) == 8 * n
        words[q, :n] = np.frombuffer(b, dtype="<u8")
    words = words.reshape(len(blobs), chunks, steps, LANES)
    index = np.arange(chunks * CRC_CHUNK, dtype=np.int64).reshape(1, chunks, steps, LANES)
    x504 = np.uint32(xpow_bytes(8 * LANES - 8))
    acc = np.zeros((len(blobs), chunks, LANES), np.uint32)
    last = np.full((1, chunks, LANES), -1, np.int64)
    for t in range(steps):
        live = index[:, :, t, :] < n
        if not live.any():
            break
        new = _fold_bytes(gf_mul(acc, x504), words[:, :, t, :])
        acc = np.where(live, new, acc)
        last = np.where(live, index[:, :, t, :], last)
    end = np.minimum((np.arange(chunks, dtype=np.int64) + 1) * CRC_CHUNK, n)[None, :, None]
    gap = np.where(last >= 0, end - 1 - last + lane_bias, 0)
    assert gap.min() >= 0
    mult = {int(q): xpow_bytes(8 * int(q)) for q in np.unique(gap)}
    shift = np.vectorize(mult.get, otypes=[np.uint32])(gap)
    lanes = gf_mul(acc, np.broadcast_to(shift, acc.shape))
    lanes = np.where(last >= 0, lanes, np.uint32(0))
    per_chunk = np.bitwise_xor.reduce(lanes, axis=2)
    to_end = np.array([xpow_bytes(8 * int(n - e)) for e in end[0, :, 0]], dtype=np.uint32)
    return lanes, gf_mul(per_chunk, np.broadcast_to(to_end[None, :], per_chunk.shape))


def lane_crc(bytes_, shape, *, lane_bias=0, detail=False):
    """The zero-register CRC of the packed field as k_crc_raw forms it: per
    (chunk, lane) registers over values 64 apart, moved to the chunk end and
    XORed, the chunk moved to the field end and XORed. Equals
    zlib.crc32(b, 0xFFFFFFFF) ^ 0xFFFFFFFF. lane_bias plants the bug the test
    must see: the lanes' move to the chunk end off by that many values.
    detail: also the per-lane registers at the chunk end (chunks, 64) and the
    per-chunk registers at the field end, to find a failing lane or chunk."""
    lanes, at_end = _lane_parts([bytes_], shape, lane_bias)
    crc = int(np.bitwise_xor.reduce(at_end[0]))
    return (crc, lanes[0], at_end[0]) if detail else crc


def lane_crcs(blobs, shape):
    """lane_crc of several fields of one shape at once."""
    return [int(v) for v in np.bitwise_xor.reduce(_lane_parts(list(blobs), shape, 0)[1], axis=1)]


# ---------------------------------------------------------------------------
# staging
# ---------------------------------------------------------------------------
def stage_planes(shape, stage_bytes=None):
    """Planes per staging buffer: the documented formula."""
    nx, ny, nz = shape
    b = STAGE_DEFAULT if stage_bytes is None or stage_bytes <= 0 else stage_bytes
    return max(1, min(nz, b // (nx * ny * 8)))


def stage_chunks(shape, stage_bytes=None):
    """[(k0, nk)] of one field's chunks."""
    nz = shape[2]
    kp = stage_planes(shape, stage_bytes)
    return [(k0, min(kp, nz - k0)) for k0 in range(0, nz, kp)]


_P3, _P18, _P2 = 20 * 14 * 8, 67 * 35 * 8, 23 * 19 * 8  # one plane, bytes

# (shape, stage_bytes, planes per chunk, chunks per field)
STAGE_CASES = [
    ((20, 14, 11), _P3, 1, 11),            # one plane per chunk; 11 chunks: odd
    ((20, 14, 11), 4 * _P3 + 8, 4, 3),     # odd count: successive fields start on alternating
                                           # buffers; a tail of 3
    ((20, 14, 11), 5 * _P3 + 100, 5, 3),   # a tail of one plane
    ((67, 35, 18), 5 * _P18, 5, 4),        # even count: every field starts on buffer 0
    ((67, 35, 18), 17 * _P18 + 1, 17, 2),  # two chunks, the second of one plane
    ((20, 14, 11), 100, 1, 11),            # a cap below one plane clamps to 1
    ((23, 19, 1), 100, 1, 1),              # the same cap in 2-D
    ((23, 19, 1), _P2, 1, 1),              # 2-D, exactly the plane
    ((20, 14, 11), 1 << 20, 11, 1),        # a cap above the field: one chunk
]


def stage_id(case):
    return f"{sid(case[0])}-{case[1]}B"
