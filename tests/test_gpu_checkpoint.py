"""Restart files of the device-resident state (hip_proj_checkpoint_write/read,
hip_proj_field_crc32) against the format oracle
(oracle/checkpoint_format.py: struct + zlib) and the reference's restart
contract (tests/io/test_checkpoint.c:169-233: N steps + checkpoint + M steps
equals N + M steps bit for bit). Runs on an MI355X.

The second half pins what the first leaves open, from the tables of
tests/checkpoint_cases.py: the CRC kernel at its lane, chunk and workgroup
edges on bit patterns and near-empty fields; the staging pipeline with many
chunks per field (CFD_HIP_CHK_STAGE_BYTES) and once at its natural 64 MiB;
2-D, padded-pitch and own-rho / own-T contexts; the scratch a write or read
borrowed; the refusals. Every check is an equality of bytes, bits or
integers."""
import ctypes as C
import os
import shutil
import struct
import time
import zlib

import numpy as np
import pytest

from cfd_amd import _abi as A
from cfd_amd import _native, api
from oracle import checkpoint_format as fmt
from oracle import oracle
from tests import cases
from tests import checkpoint_cases as K
from tests.special_values import assert_bits_equal
from tests.test_checkpoint import grid_dict, nondefault_params, params_dict

pytestmark = pytest.mark.gpu

F = {"u": A.HIP_FIELD_U, "v": A.HIP_FIELD_V, "w": A.HIP_FIELD_W, "p": A.HIP_FIELD_P,
     "T": A.HIP_FIELD_T}


def _loaded(g, f, **cfg):
    ctx = api.HipProjection(g.nx, g.ny, g.nz, **cfg)
    for k, fid in F.items():
        ctx.set_field(fid, getattr(f, k))
    ctx.set_density(float(f.rho.flat[0]))
    return ctx


@pytest.mark.parametrize("shape", [(33, 33, 33), (17, 9, 5), (130, 70, 3), (64, 64, 1)])
def test_device_crc32_matches_zlib(hip_lib, shape):
    """GPU CRC of the packed field (wave-strided registers, lane/chunk shifts,
    XOR combine) equals zlib.crc32 of the same bytes, for rows shorter and
    longer than a wavefront and chunk tails."""
    nx, ny, nz = shape
    rng = np.random.default_rng(nx * ny * nz)
    ctx = api.HipProjection(nx, ny, nz)
    a = rng.standard_normal((nz, ny, nx))
    ctx.set_field(A.HIP_FIELD_U, a)
    assert ctx.field_crc32(A.HIP_FIELD_U) == zlib.crc32(np.ascontiguousarray(a).tobytes())
    ctx.close()


def test_device_crc32_large_multichunk(hip_lib):
    """256^3: 2048 chunks of 8192 values joined by x^(8d) shifts and an XOR."""
    n = 256
    ctx = api.HipProjection(n, n, n)
    a = np.random.default_rng(1).standard_normal((n, n, n))
    ctx.set_field(A.HIP_FIELD_P, a)
    assert ctx.field_crc32(A.HIP_FIELD_P) == zlib.crc32(a.tobytes())
    ctx.close()


def test_device_write_matches_format_and_host_writer(hip_lib, tmp_path):
    g, f, _ = cases.tg3(17)
    f.T[...] = np.random.default_rng(3).standard_normal(f.T.shape) + 300.0
    ctx = _loaded(g, f)
    p = nondefault_params()
    dev = str(tmp_path / "dev.cfdchk")
    host = str(tmp_path / "host.cfdchk")
    assert ctx.checkpoint_write(dev, g, p, 3.5, "projection_hip", "run7", "/out") == A.CFD_SUCCESS
    data = open(dev, "rb").read()
    d = fmt.decode(data)
    assert d["crc_ok"] is True
    for k, fid in F.items():
        assert np.array_equal(d["fields"][k], ctx.get_field(fid)), k
    assert np.all(d["fields"]["rho"] == 1.0)
    assert (d["solver"], d["prefix"], d["base"], d["time"]) == (b"projection_hip", b"run7", b"/out", 3.5)
    # the host writer, given the same arrays, produces the identical file
    assert api.checkpoint_write(host, g, f, p, 3.5, "projection_hip", "run7", "/out") == 0
    assert open(host, "rb").read() == data
    ctx.close()


def test_device_read_and_reject_corruption(hip_lib, tmp_path):
    g, f, _ = cases.tg3(17)
    f.T[...] = 290.0 + np.arange(f.T.size).reshape(f.T.shape) * 1e-3
    p = nondefault_params()
    path = str(tmp_path / "h.cfdchk")
    assert api.checkpoint_write(path, g, f, p, 9.0, "projection_hip", None, "/b") == 0
    ctx = api.HipProjection(17, 17, 17)
    st, g2, p2, t2, name, prefix, base = ctx.checkpoint_read(path)
    assert st == A.CFD_SUCCESS and (t2, name, prefix, base) == (9.0, "projection_hip", "", "/b")
    for k, fid in F.items():
        assert np.array_equal(ctx.get_field(fid), getattr(f, k)), k
    for k, v in grid_dict(g).items():
        assert np.array_equal(np.asarray(grid_dict(g2)[k]), np.asarray(v)), k
    assert params_dict(p2) == params_dict(p)
    before = {k: ctx.get_field(fid) for k, fid in F.items()}
    data = open(path, "rb").read()
    for name, off in fmt.field_offsets(data).items():
        bad = bytearray(data)
        bad[off + 8 * 100 + 3] ^= 0x10
        open(path, "wb").write(bytes(bad))
        assert ctx.checkpoint_read(path)[0] == A.CFD_ERROR_IO, name
        for k, fid in F.items():  # a rejected file leaves the device state alone
            assert np.array_equal(ctx.get_field(fid), before[k]), (name, k)
    open(path, "wb").write(data[: len(data) // 3])
    assert ctx.checkpoint_read(path)[0] == A.CFD_ERROR_IO
    other = str(tmp_path / "o.cfdchk")
    g9, f9, _ = cases.tg3(9)
    assert api.checkpoint_write(other, g9, f9, p, 0.0, "projection_hip") == 0
    assert ctx.checkpoint_read(other)[0] == A.CFD_ERROR_INVALID  # dimensions are the context's
    ctx.close()


@pytest.mark.parametrize("case", ["tg", "cavity"])
def test_restart_continuity_device(hip_lib, tmp_path, case):
    """test_checkpoint.c:169-222 on the device path: N steps, checkpoint, M
    steps in a fresh context from the file == N + M steps, bit for bit."""
    if case == "tg":
        g, f, p = cases.tg3(17)
        bc = lambda c: [c.apply_scalar_bc(fid, A.BC_TYPE_PERIODIC) for fid in  # noqa: E731
                        (A.HIP_FIELD_U, A.HIP_FIELD_V, A.HIP_FIELD_W, A.HIP_FIELD_P)]
    else:
        g, f, p = cases.cavity(17, 17, 17, Re=100.0, dt=5e-4)

        def bc(c):
            c.apply_dirichlet(A.HIP_FIELD_U, api.dirichlet(top=1.0))
            c.apply_dirichlet(A.HIP_FIELD_V, api.dirichlet())
            c.apply_dirichlet(A.HIP_FIELD_W, api.dirichlet())
            c.apply_scalar_bc(A.HIP_FIELD_P, A.BC_TYPE_NEUMANN)
    N, M = 3, 4
    path = str(tmp_path / "r.cfdchk")
    a = _loaded(g, f)
    for i in range(N + M):
        if i == N:
            assert a.checkpoint_write(path, g, p, N * p.dt, "projection_hip") == A.CFD_SUCCESS
        bc(a)
        assert a.step_device(g, p) == A.CFD_SUCCESS
    b = api.HipProjection(g.nx, g.ny, g.nz)
    st, _, p2, t2, *_ = b.checkpoint_read(path)
    assert st == A.CFD_SUCCESS and t2 == N * p.dt
    for _ in range(M):
        bc(b)
        assert b.step_device(g, p2) == A.CFD_SUCCESS
    for k, fid in F.items():
        if k == "T":
            continue
        assert np.array_equal(a.get_field(fid), b.get_field(fid)), k
    a.close()
    b.close()


def test_simulation_save_load_restart_projection_hip(hip_lib, tmp_path):
    """save_simulation_checkpoint / load_simulation_from_checkpoint /
    restore_simulation_checkpoint (simulation_api.c:257-440) with the
    projection_hip plugin driving run_simulation_step: bitwise continuation."""
    h = _native.host()
    _native.hip()
    path = str(tmp_path / "sim.cfdchk").encode()

    def new_sim():
        s = h.init_simulation_with_solver(17, 17, 17, 0.0, 1.0, 0.0, 1.0, 0.0, 1.0,
                                          b"projection_hip")
        assert s, _native.last_error()
        return s

    def arrays(s):
        c = s.contents.field.contents
        n = c.nx * c.ny * c.nz
        return {k: np.ctypeslib.as_array(getattr(c, k), (n,)).copy() for k in ("u", "v", "w", "p")}

    a = new_sim()
    for _ in range(2):
        assert h.run_simulation_step(a) == A.CFD_SUCCESS
    assert h.save_simulation_checkpoint(a, path) == A.CFD_SUCCESS
    for _ in range(3):
        assert h.run_simulation_step(a) == A.CFD_SUCCESS
    b = h.load_simulation_from_checkpoint(path)
    assert b, _native.last_error()
    assert b.contents.solver.contents.name == b"projection_hip"
    assert b.contents.current_time == pytest.approx(2 * 0.005)
    for _ in range(3):
        assert h.run_simulation_step(b) == A.CFD_SUCCESS
    fa, fb = arrays(a), arrays(b)
    for k in fa:
        assert np.array_equal(fa[k], fb[k]), k
    c = new_sim()
    assert h.restore_simulation_checkpoint(c, path) == A.CFD_SUCCESS
    for _ in range(3):
        assert h.run_simulation_step(c) == A.CFD_SUCCESS
    fc = arrays(c)
    for k in fa:
        assert np.array_equal(fa[k], fc[k]), k
    for s in (a, b, c):
        h.free_simulation(s)


# ---------------------------------------------------------------------------
# helpers of the tests below
# ---------------------------------------------------------------------------
ALL = dict(F, rho=A.HIP_FIELD_RHO)  # the six fields of the file
UVWP = ("u", "v", "w", "p")
RHO0 = 1.25
TAIL = (3.5, "projection_hip", "run7", "/out")  # time and the three strings


def _grid(shape):
    nx, ny, nz = shape
    return api.Grid(nx, ny, nz, 0.0, 0.9, 0.0, 1.3, 0.0, 0.7 if nz > 1 else 0.0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(got, want, what):
    """Bit for bit, NaN payloads included (assert_bits_equal names the cell
    and treats every NaN as one class; the view compares the payloads)."""
    assert_bits_equal(got, want, what=what)
    assert np.array_equal(_bits(got), _bits(want)), f"{what}: NaN payloads differ"


def _six(shape, seed=0):
    """u, v, w, p, rho, T as random bit patterns, seeded per field."""
    return {k: K.random_bits(shape, 10 * seed + q) for q, k in enumerate(fmt.FIELDS)}


def _bits_ctx(shape, fields, own_rho=True, own_T=True, **cfg):
    """A context that holds `fields`; without its own rho it has rho0 = RHO0,
    without its own T it has none."""
    ctx = api.HipProjection(*shape, **cfg)
    for k in UVWP:
        ctx.set_field(ALL[k], fields[k])
    ctx.set_density(RHO0)
    if own_rho:
        ctx.set_field(A.HIP_FIELD_RHO, fields["rho"])
    if own_T:
        ctx.set_field(A.HIP_FIELD_T, fields["T"])
    return ctx


def _held(shape, fields, own_rho=True, own_T=True):
    """What such a context writes: rho0 everywhere / T = 0 where it has no
    field of its own."""
    nx, ny, nz = shape
    out = dict(fields)
    if not own_rho:
        out["rho"] = np.full((nz, ny, nx), RHO0)
    if not own_T:
        out["T"] = np.zeros((nz, ny, nx))
    return out


def _encode(g, fields, p, **kw):
    t, name, prefix, base = TAIL
    return fmt.encode(grid_dict(g), fields, params_dict(p), t, name.encode(), prefix.encode(),
                      base.encode(), **kw)


def _dev_write(ctx, path, g, p):
    return ctx.checkpoint_write(str(path), g, p, *TAIL)


def _host_write(path, g, fields, p):
    nx, ny, nz = g.nx, g.ny, g.nz
    f = api.FlowField(nx, ny, nz)
    for k in fmt.FIELDS:
        getattr(f, k)[...] = fields[k]
    return api.checkpoint_write(str(path), g, f, p, *TAIL)


def _state(ctx, names=tuple(ALL)):
    """name -> the field, or None where the context has none."""
    out = {}
    for k in names:
        try:
            out[k] = ctx.get_field(ALL[k])
        except api.CfdError as e:
            assert e.status == A.CFD_ERROR_INVALID and k in ("rho", "T"), (k, e)
            out[k] = None
    return out


def _assert_state(ctx, before, what):
    now = _state(ctx, tuple(before))
    for k, want in before.items():
        assert (now[k] is None) == (want is None), (what, k)
        if want is not None:
            _same_bits(now[k], want, f"{what}: {k}")


def _crc_failure(shape, name, a, got):
    """Which lane or chunk of the decomposition accounts for a wrong CRC."""
    b = K.packed_bytes(a)
    want = zlib.crc32(b)
    _, lanes, chunks = K.lane_crc(b, shape, detail=True)
    diff = got ^ want  # the join is linear: the registers differ by the same word
    plan = K.crc_plan(shape)
    to_end = [K.xpow_bytes(8 * (plan["n"] - min((c + 1) * K.CRC_CHUNK, plan["n"])))
              for c in range(plan["chunks"])]
    lane_hits = [(c, l) for c in range(plan["chunks"]) for l in range(K.LANES)
                 if lanes[c, l] and int(K.gf_mul(lanes[c, l], to_end[c])) == diff]
    chunk_hits = [c for c in range(plan["chunks"]) if chunks[c] and int(chunks[c]) == diff]
    return (f"{K.sid(shape)} {name}: device {got:#010x}, zlib {want:#010x}, xor {diff:#010x}; "
            f"a dropped chunk would be {chunk_hits}, a dropped (chunk, lane) {lane_hits}; "
            f"plan {plan}")


# ---------------------------------------------------------------------------
# the CRC kernel
# ---------------------------------------------------------------------------
def _check_crcs(ctx, shape, fid=A.HIP_FIELD_U, seed=0):
    fails = []
    for name, a in K.patterns(shape, seed).items():
        ctx.set_field(fid, a)
        got = ctx.field_crc32(fid)
        if got != zlib.crc32(K.packed_bytes(a)):
            fails.append(_crc_failure(shape, name, a, got))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("shape", K.CRC_SHAPE_LIST, ids=K.sid)
def test_device_crc32_at_lane_chunk_and_workgroup_edges(hip_lib, shape):
    """k_crc_raw == zlib on every pattern of checkpoint_cases.patterns: bit
    patterns no float comparison sees, and the all-zero, one-value and
    constant fields that reach the kernel's short-circuits (a zero register
    skips its shifts, a zero chunk skips its atomic)."""
    ctx = api.HipProjection(*shape)
    try:
        assert hip_lib.hip_proj_row_pitch(ctx.ctx) == (shape[0] + 7) // 8 * 8
        _check_crcs(ctx, shape)
    finally:
        ctx.close()


@pytest.mark.parametrize("shape", K.ROW_PAD_SHAPES, ids=K.sid)
def test_device_crc32_on_a_padded_row_pitch(hip_lib, monkeypatch, shape):
    monkeypatch.setenv("CFD_HIP_ROW_PAD", "8")
    ctx = api.HipProjection(*shape)
    try:
        # the pitch really grew: the round-up to 8 and eight more
        assert hip_lib.hip_proj_row_pitch(ctx.ctx) == (shape[0] + 7) // 8 * 8 + 8
        _check_crcs(ctx, shape, seed=1)
    finally:
        ctx.close()


@pytest.mark.parametrize("shape", [(5, 4, 3), (67, 35, 18)], ids=K.sid)
def test_device_crc32_of_T_and_rho(hip_lib, shape):
    ctx = api.HipProjection(*shape)
    try:
        v = C.c_uint32(77)
        for fid in (A.HIP_FIELD_T, A.HIP_FIELD_RHO):  # a context that has neither
            assert hip_lib.hip_proj_field_crc32(ctx.ctx, fid, C.byref(v)) == A.CFD_ERROR_INVALID
            assert v.value == 77
        for seed, fid in ((2, A.HIP_FIELD_T), (3, A.HIP_FIELD_RHO)):  # set_field creates them
            _check_crcs(ctx, shape, fid, seed)
        # ... and the other fields' CRCs are their own
        a = K.random_bits(shape, 4)
        ctx.set_field(A.HIP_FIELD_W, a)
        assert ctx.field_crc32(A.HIP_FIELD_W) == zlib.crc32(K.packed_bytes(a))
        assert ctx.field_crc32(A.HIP_FIELD_T) == \
            zlib.crc32(K.packed_bytes(K.patterns(shape, 2)["constant"]))
    finally:
        ctx.close()


# ---------------------------------------------------------------------------
# write
# ---------------------------------------------------------------------------
def _check_write(monkeypatch, tmp_path, shape, nbytes, own_rho, own_T):
    g = _grid(shape)
    p = nondefault_params()
    fields = _six(shape, seed=1)
    held = _held(shape, fields, own_rho, own_T)
    want = _encode(g, held, p)
    ctx = _bits_ctx(shape, fields, own_rho, own_T)
    try:
        before = _state(ctx)
        monkeypatch.setenv(K.STAGE_KNOB, str(nbytes))
        dev = tmp_path / "dev.cfdchk"
        assert _dev_write(ctx, dev, g, p) == A.CFD_SUCCESS, _native.last_error()
        data = dev.read_bytes()
        if data != want:
            off = fmt.field_offsets(want)
            n8 = 8 * shape[0] * shape[1] * shape[2]
            plane = 8 * shape[0] * shape[1]
            bad = {k: sorted({(i // plane) for i in range(0, n8, 8)
                              if data[o + i:o + i + 8] != want[o + i:o + i + 8]})
                   for k, o in off.items() if data[o:o + n8] != want[o:o + n8]}
            raise AssertionError(f"device file differs from the format oracle's; planes that "
                                 f"differ per field {bad}; chunks (k0, nk) "
                                 f"{K.stage_chunks(shape, nbytes)}; lengths {len(data)}, {len(want)}")
        # the host writer, given the same arrays, writes the same file
        host = tmp_path / "host.cfdchk"
        assert _host_write(host, g, held, p) == A.CFD_SUCCESS
        assert host.read_bytes() == data
        # the staging size changes how the bytes travel, not the bytes
        monkeypatch.delenv(K.STAGE_KNOB)
        again = tmp_path / "again.cfdchk"
        assert _dev_write(ctx, again, g, p) == A.CFD_SUCCESS
        assert again.read_bytes() == data
        # a write changes nothing the context holds, and creates no rho / T
        _assert_state(ctx, before, "after the writes")
    finally:
        ctx.close()


@pytest.mark.parametrize("case", K.STAGE_CASES, ids=K.stage_id)
def test_device_write_multi_chunk(hip_lib, monkeypatch, tmp_path, case):
    """The file of a context with its own rho and T under each staging size of
    STAGE_CASES (k0 > 0 offsets, short tails, buffers reused and alternating
    between fields) is the format oracle's and the host writer's, byte for
    byte, and the same as with the default size."""
    shape, nbytes, kp, nchunk = case
    assert (K.stage_planes(shape, nbytes), len(K.stage_chunks(shape, nbytes))) == (kp, nchunk)
    _check_write(monkeypatch, tmp_path, shape, nbytes, True, True)


@pytest.mark.parametrize("own_T", [False, True], ids=["noT", "ownT"])
@pytest.mark.parametrize("own_rho", [False, True], ids=["rho0", "ownrho"])
@pytest.mark.parametrize("case", [K.STAGE_CASES[2], K.STAGE_CASES[6]], ids=K.stage_id)
def test_device_write_with_and_without_own_rho_and_T(hip_lib, monkeypatch, tmp_path, case,
                                                     own_rho, own_T):
    """The k_fill_const substitutes (rho0 into us, 0 into vs) in every
    combination, chunked in 3-D and in 2-D."""
    _check_write(monkeypatch, tmp_path, case[0], case[1], own_rho, own_T)


# ---------------------------------------------------------------------------
# read
# ---------------------------------------------------------------------------
def _check_read(ctx, path, g, p, fields, what):
    st, g2, p2, t2, name, prefix, base = ctx.checkpoint_read(str(path))
    assert st == A.CFD_SUCCESS, (what, _native.last_error())
    assert (t2, name, prefix, base) == TAIL
    for k, v in grid_dict(g).items():
        assert np.array_equal(np.asarray(grid_dict(g2)[k]), np.asarray(v)), (what, k)
    assert params_dict(p2) == params_dict(p)
    for k in fmt.FIELDS:
        _same_bits(ctx.get_field(ALL[k]), fields[k], f"{what}: {k}")
    return g2, p2


@pytest.mark.parametrize("case", K.STAGE_CASES, ids=K.stage_id)
def test_device_read_multi_chunk(hip_lib, monkeypatch, tmp_path, case):
    """A file the format oracle built restores u, v, w, p, rho, T bit for bit
    into a fresh context (no rho, no T of its own) under each staging size."""
    shape, nbytes, _, _ = case
    g = _grid(shape)
    p = nondefault_params()
    fields = _six(shape, seed=2)
    path = tmp_path / "o.cfdchk"
    path.write_bytes(_encode(g, fields, p))
    monkeypatch.setenv(K.STAGE_KNOB, str(nbytes))
    ctx = api.HipProjection(*shape)
    try:
        _check_read(ctx, path, g, p, fields, K.stage_id(case))
        # once more into the now populated context, other contents
        fields = _six(shape, seed=3)
        path.write_bytes(_encode(g, fields, p))
        _check_read(ctx, path, g, p, fields, K.stage_id(case) + " again")
    finally:
        ctx.close()


@pytest.mark.parametrize("sizes", [(K.STAGE_CASES[1], K.STAGE_CASES[2][1], K.STAGE_CASES[0][1]),
                                   (K.STAGE_CASES[3], K.STAGE_CASES[4][1], None),
                                   (K.STAGE_CASES[6], None, K.STAGE_CASES[7][1])],
                         ids=lambda s: K.stage_id(s[0]))
def test_device_round_trip_under_different_staging_sizes(hip_lib, monkeypatch, tmp_path, sizes):
    """write -> read -> write with another staging size on each side (None:
    the default) reproduces the file."""
    (shape, first, _, _), second, third = sizes

    def knob(v):
        if v is None:
            monkeypatch.delenv(K.STAGE_KNOB, raising=False)
        else:
            monkeypatch.setenv(K.STAGE_KNOB, str(v))

    g = _grid(shape)
    p = nondefault_params()
    fields = _six(shape, seed=4)
    a = _bits_ctx(shape, fields)
    b = api.HipProjection(*shape)
    try:
        knob(first)
        one = tmp_path / "one.cfdchk"
        assert _dev_write(a, one, g, p) == A.CFD_SUCCESS
        knob(second)
        g2, p2 = _check_read(b, one, g, p, fields, "round trip")
        knob(third)
        two = tmp_path / "two.cfdchk"
        assert _dev_write(b, two, g2, p2) == A.CFD_SUCCESS
        assert two.read_bytes() == one.read_bytes() == _encode(g, fields, p)
    finally:
        a.close()
        b.close()


def test_device_write_and_read_on_a_padded_row_pitch(hip_lib, monkeypatch, tmp_path):
    """Row pitch 88 for nx = 67: the 2-D copies' device pitch is not the
    round-up of the row."""
    shape, nbytes = K.STAGE_CASES[3][:2]
    monkeypatch.setenv("CFD_HIP_ROW_PAD", "16")
    monkeypatch.setenv(K.STAGE_KNOB, str(nbytes))
    g = _grid(shape)
    p = nondefault_params()
    fields = _six(shape, seed=5)
    a = _bits_ctx(shape, fields)
    b = api.HipProjection(*shape)
    try:
        assert hip_lib.hip_proj_row_pitch(a.ctx) == hip_lib.hip_proj_row_pitch(b.ctx) == 88
        path = tmp_path / "pad.cfdchk"
        assert _dev_write(a, path, g, p) == A.CFD_SUCCESS
        assert path.read_bytes() == _encode(g, fields, p)
        _check_read(b, path, g, p, fields, "padded pitch")
    finally:
        a.close()
        b.close()


def test_device_checkpoint_at_the_natural_staging_size(hip_lib, monkeypatch, tmp_path):
    """1024 x 1024 x 9 with the knob unset: planes of 8 MiB, 8 per 64 MiB
    buffer, so two chunks per field with a tail of one plane -- the pipeline
    as the product's 512^3 runs it, at its own buffer size. The device
    writes, a second context reads, all six fields are equal in every bit and
    the trailer is zlib's CRC of the streamed body.
    Measured on the MI355X: 0.78 s wall (the test prints its own time),
    against 0.24 s for test_device_crc32_large_multichunk in the same run."""
    shape = (1024, 1024, 9)
    free = shutil.disk_usage(tmp_path).free
    if free < 2 << 30:
        pytest.skip(f"{free >> 20} MiB free under {tmp_path}: the 450 MB file needs room")
    monkeypatch.delenv(K.STAGE_KNOB, raising=False)
    assert K.stage_chunks(shape) == [(0, 8), (8, 1)]
    t0 = time.perf_counter()
    g = _grid(shape)
    p = nondefault_params()
    fields = _six(shape, seed=6)
    path = tmp_path / "natural.cfdchk"
    a = _bits_ctx(shape, fields)
    try:
        assert _dev_write(a, path, g, p) == A.CFD_SUCCESS, _native.last_error()
    finally:
        a.close()
    n8 = 8 * shape[0] * shape[1] * shape[2]
    size = os.path.getsize(path)
    crc, left = 0, size - 4
    with open(path, "rb") as fh:
        head = fh.read(4096)
        off = fmt.field_offsets(head)
        fh.seek(0)
        while left:
            blk = fh.read(min(left, 32 << 20))
            assert blk
            crc = zlib.crc32(blk, crc)
            left -= len(blk)
        (stored,) = struct.unpack("<I", fh.read(4))
        assert fh.read(1) == b""
    assert stored == crc
    assert off["T"] + n8 < size
    b = api.HipProjection(*shape)
    try:
        st, _, p2, t2, name, *_ = b.checkpoint_read(str(path))
        assert st == A.CFD_SUCCESS, _native.last_error()
        assert (t2, name) == TAIL[:2] and params_dict(p2) == params_dict(p)
        for k in fmt.FIELDS:
            _same_bits(b.get_field(ALL[k]), fields[k], f"natural size: {k}")
    finally:
        b.close()
    path.unlink()
    print(f"natural-size checkpoint test: {time.perf_counter() - t0:.2f} s")


# ---------------------------------------------------------------------------
# scratch hygiene
# ---------------------------------------------------------------------------
HYGIENE_SHAPES = [(20, 14, 11), (67, 35, 1)]
CAP = dict(poisson_max_iter=60, poisson_fail_fatal=0)  # every step completes, converged or not
# route -> (context configuration, CFD_HIP_CG_SMALL)
ROUTES = {
    "cg": (dict(cg_variant=0), None),                    # the one-launch small-grid CG
    "cg_sweeps": (dict(cg_variant=0), "0"),              # textbook CG on the sweeps
    "cg_single_reduction": (dict(cg_variant=1), None),
    "redblack": (dict(poisson_method=A.HIP_POISSON_REDBLACK), None),
    "jacobi": (dict(poisson_method=A.HIP_POISSON_JACOBI), None),
    "dst": (dict(poisson_method=A.HIP_POISSON_DST), None),
    "dct": (dict(poisson_method=A.HIP_POISSON_DCT), None),  # the step's pressure BC is Neumann
    "bicgstab": (dict(cg_variant=0), "0"),               # poisson_solve(BICGSTAB) + CG steps
}


def _flow_fields(shape):
    nx, ny, nz = shape
    rng = np.random.default_rng([nx, ny, nz, 99])
    f = {k: 0.05 * rng.standard_normal((nz, ny, nx)) for k in UVWP}
    f["T"] = 300.0 + rng.standard_normal((nz, ny, nx))
    f["rhs"] = rng.standard_normal((nz, ny, nx))
    f["x0"] = 0.1 * rng.standard_normal((nz, ny, nx))
    return f


def _flow_ctx(shape, f, cfg):
    ctx = api.HipProjection(*shape, **CAP, **cfg)
    for k in UVWP + ("T",):
        ctx.set_field(ALL[k], f[k])
    ctx.set_density(RHO0)
    return ctx


def _pstats(ctx):
    s = ctx.poisson_stats()
    return (s.status, s.iterations, s.initial_residual, s.final_residual)


def _advance(ctx, g, p, f, route):
    """Two device steps (and BiCGSTAB's own solve first): every status,
    iteration count, residual and field they leave."""
    out = {}
    if route == "bicgstab":
        x = np.array(f["x0"])
        d = (g.dx, g.dy, g.dz)
        s, st = ctx.poisson_solve(A.HIP_POISSON_BICGSTAB, x, f["rhs"], *d,
                                  oracle.poisson_params(max_iterations=40))
        out["bicgstab"] = (s, st.status, st.iterations, st.initial_residual, st.final_residual)
        out["bicgstab x"] = x
    for n in range(2):
        st = A.SolverStats()
        out[f"step {n}"] = (ctx.step_device(g, p, st), st.iterations, st.residual, st.status,
                            st.max_velocity, st.max_pressure) + _pstats(ctx)
    for k in UVWP:
        out[k] = ctx.get_field(ALL[k])
    return out


def _assert_same_run(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], tuple):
            assert np.array_equal(np.array(a[k][1:]).view(np.uint64),
                                  np.array(b[k][1:]).view(np.uint64)) and a[k][0] == b[k][0], \
                (what, k, a[k], b[k])
        else:
            _same_bits(a[k], b[k], f"{what}: {k}")


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("shape", HYGIENE_SHAPES, ids=K.sid)
def test_checkpoint_leaves_the_scratch_as_the_solvers_need_it(hip_lib, monkeypatch, tmp_path,
                                                              shape, route):
    """A context that writes, fails to write, reads and has reads rejected
    (for a flipped byte, for a solver-name buffer that is too small -- after
    all six uploads -- and for a bad magic) between its steps computes what a
    twin that never touches a checkpoint computes, bit for bit: two device
    steps after each event, on every Poisson route, then one RK4 step (which
    borrows r, pa, pb). A rejected read also leaves the Poisson statistics,
    rho and T alone."""
    cfg, small = ROUTES[route]
    if small is not None:
        monkeypatch.setenv("CFD_HIP_CG_SMALL", small)
    # three chunks per field in 3-D, so the scratch is written at k0 > 0 too
    monkeypatch.setenv(K.STAGE_KNOB, str(4 * shape[0] * shape[1] * 8))
    g = _grid(shape)
    p = api.validation_params(1e-4, 0.01)
    f = _flow_fields(shape)
    a, b = _flow_ctx(shape, f, cfg), _flow_ctx(shape, f, cfg)
    path = tmp_path / "h.cfdchk"
    other = _six(shape, seed=7)  # what a rejected file holds: nothing of it may arrive

    def current_file(ctx):
        s = _state(ctx)
        nx, ny, nz = shape
        if s["rho"] is None:
            s["rho"] = np.full((nz, ny, nx), RHO0)
        return _encode(g, s, p)

    def good_write():
        assert _dev_write(a, path, g, p) == A.CFD_SUCCESS
        assert path.read_bytes() == current_file(a)

    def failed_write():
        missing = tmp_path / "no_such_dir" / "x.cfdchk"
        assert _dev_write(a, missing, g, p) == A.CFD_ERROR_IO
        assert not missing.parent.exists()

    def good_read():
        path.write_bytes(current_file(a))
        assert a.checkpoint_read(str(path))[0] == A.CFD_SUCCESS, _native.last_error()

    def rejected(blob, status, caps=(128, 256, 512)):
        path.write_bytes(blob)
        before, stats = _state(a), _pstats(a)
        assert a.checkpoint_read(str(path), caps=caps)[0] == status
        _assert_state(a, before, "rejected read")
        assert _pstats(a) == stats

    def flipped_byte():
        blob = bytearray(_encode(g, other, p))
        blob[fmt.field_offsets(bytes(blob))["T"] + 8 * 37 + 2] ^= 0x04
        rejected(bytes(blob), A.CFD_ERROR_IO)

    def small_name_buffer():
        rejected(_encode(g, other, p), A.CFD_ERROR_INVALID, caps=(4, 256, 512))

    def bad_magic():
        rejected(b"X" + _encode(g, other, p)[1:], A.CFD_ERROR_INVALID)

    try:
        _assert_same_run(_advance(a, g, p, f, route), _advance(b, g, p, f, route), "before")
        for event in (good_write, failed_write, flipped_byte, good_read, small_name_buffer,
                      bad_magic):
            event()
            _assert_same_run(_advance(a, g, p, f, route), _advance(b, g, p, f, route),
                             f"{route} after {event.__name__}")
        # RK4 straight after a rejected read and a write, nothing in between
        # that would clear the CG scratch for it
        flipped_byte()
        good_write()
        sa, sb = a.rk4_step_device(g, p), b.rk4_step_device(g, p)
        assert sa == sb == A.CFD_SUCCESS, (sa, sb, _native.last_error())
        for k in UVWP:
            _same_bits(a.get_field(ALL[k]), b.get_field(ALL[k]), f"{route} rk4: {k}")
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------
def test_device_checkpoint_refusals(hip_lib, monkeypatch, tmp_path):
    """Every refusal leaves the device fields as they were."""
    shape = (20, 14, 11)
    nbytes = K.STAGE_CASES[1][1]  # chunks of 4, 4 and 3 planes
    monkeypatch.setenv(K.STAGE_KNOB, str(nbytes))
    g = _grid(shape)
    p = nondefault_params()
    fields = _six(shape, seed=8)
    ctx = _bits_ctx(shape, fields)
    try:
        before = _state(ctx)
        path = tmp_path / "r.cfdchk"
        # write: a grid of other dimensions, a NULL solver name, a path that cannot be opened
        for dims in ((21, 14, 11), (20, 15, 11), (20, 14, 12), (20, 14, 1)):
            assert ctx.checkpoint_write(str(path), _grid(dims), p, *TAIL) == A.CFD_ERROR_INVALID
            assert not path.exists(), dims
        assert ctx.checkpoint_write(str(path), g, p, 1.0, None) == A.CFD_ERROR_INVALID
        assert not path.exists()
        missing = tmp_path / "nowhere" / "r.cfdchk"
        assert _dev_write(ctx, missing, g, p) == A.CFD_ERROR_IO and not missing.parent.exists()
        _assert_state(ctx, before, "refused writes")
        # read: version, endian marker, magic
        blob = _encode(g, _six(shape, seed=9), p)
        for kw, status in ((dict(version=2), A.CFD_ERROR_UNSUPPORTED),
                           (dict(endian=0x04030201), A.CFD_ERROR_UNSUPPORTED)):
            path.write_bytes(_encode(g, _six(shape, seed=9), p, **kw))
            assert ctx.checkpoint_read(str(path))[0] == status, kw
            _assert_state(ctx, before, f"read refused for {kw}")
        path.write_bytes(b"cfdchk\0\0" + blob[8:])
        assert ctx.checkpoint_read(str(path))[0] == A.CFD_ERROR_INVALID
        _assert_state(ctx, before, "bad magic")
        # truncated inside the second chunk of w: u and v are in the scratch
        # already, w's first chunk too
        k0, nk = K.stage_chunks(shape, nbytes)[1]
        assert k0 > 0 and nk > 1
        cut = fmt.field_offsets(blob)["w"] + (k0 * shape[0] * shape[1] + 50) * 8
        path.write_bytes(blob[:cut])
        assert ctx.checkpoint_read(str(path))[0] == A.CFD_ERROR_IO
        _assert_state(ctx, before, "truncated")
        # a file of other dimensions, a missing file
        g2 = _grid((20, 14, 12))
        path.write_bytes(_encode(g2, _six((20, 14, 12)), p))
        assert ctx.checkpoint_read(str(path))[0] == A.CFD_ERROR_INVALID
        assert ctx.checkpoint_read(str(tmp_path / "none.cfdchk"))[0] == A.CFD_ERROR_IO
        _assert_state(ctx, before, "other dimensions")
        # ... and the context still writes what it holds
        assert _dev_write(ctx, path, g, p) == A.CFD_SUCCESS
        assert path.read_bytes() == _encode(g, fields, p)
    finally:
        ctx.close()


def test_z_slab_contexts_refuse_checkpoints(hip_lib, tmp_path):
    """One rank's write and read return CFD_ERROR_UNSUPPORTED at once, without
    its neighbour taking part; nothing appears at the path."""
    shape = (20, 14, 11)
    g = _grid(shape)
    p = nondefault_params()
    group = api.LocalGroup(2)
    ctxs = []
    try:
        ctxs = [api.HipProjection(*shape, comm=group.comm(r, 0)) for r in range(2)]
        c = ctxs[0]
        rng = np.random.default_rng(5)
        local = {k: rng.standard_normal(c.shape) for k in UVWP}
        for k, a in local.items():
            c.set_field(ALL[k], a)
        path = tmp_path / "slab.cfdchk"
        assert _dev_write(c, path, g, p) == A.CFD_ERROR_UNSUPPORTED
        assert "Z-slab" in _native.last_error() and not path.exists()
        path.write_bytes(_encode(g, _six(shape), p))
        assert c.checkpoint_read(str(path))[0] == A.CFD_ERROR_UNSUPPORTED
        assert "Z-slab" in _native.last_error()
        for k, a in local.items():
            _same_bits(c.get_field(ALL[k]), a, f"slab rank 0: {k}")
    finally:
        for c in ctxs:
            c.close()
        group.close()
