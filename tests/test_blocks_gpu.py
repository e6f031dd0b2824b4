"""The blocks library's batched calls on the GPU (snappy.jl_amd/blocks.py over
libsnappy_mi355x_blocks.so): smb_uncompress_streams_device and smb_compress_streams_device in both
formats over mixed batches laid back to back at odd alignments, isolation between the chunks of a
stream, the capacity and slot bounds, workgroup and scan-tile edges, chunks of more than 64 KiB with
and without the fragment index, and the host-buffer and Python calls.  Every expected value comes
from the plain-Python reference (tests/blocks_ref.py) and the CPU oracle."""
import functools
import importlib

import numpy as np
import pytest

import blocks_ref as R
from conftest import load_package, read_testfile

pytestmark = pytest.mark.gpu

BLOCK = 65536
GUARD = 0xA5
ARG = R.SM_ERR_ARGUMENT
ROOM = 300000  # a stream that declares more gets no room here (structure only: SM_BUFFER_TOO_SMALL)


@pytest.fixture(scope="module")
def bl(gpu_available):
    load_package()
    return importlib.import_module("snappy_jl_amd.blocks")


def _torch():
    import torch
    return torch


def _dev():
    return _torch().device("cuda", 0)


def _i64(values):
    return _torch().from_numpy(np.array(values, dtype=np.uint64).view(np.int64)).to(_dev())


def _oracle():
    import oracle as O
    O.lib()
    return O


@functools.lru_cache(maxsize=None)
def text(n):
    t = read_testfile("alice29.txt")
    return (t * (n // len(t) + 1))[:n]


@functools.lru_cache(maxsize=None)
def rand(n, seed=17):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def encoded(fmt, kind, n):
    """(input, its reference-mode stream by the Python writer)"""
    data = text(n) if kind == "text" else rand(n)
    return data, R.encode(data, fmt, _oracle().compress)


def lay(buffers, lead=1, gap=0):
    """The buffers in one device tensor, the first at an address that is `lead` mod 16, `gap` bytes
    between them (0: directly behind one another): (tensor, offsets, lengths)."""
    offs, pos = [], lead
    for b in buffers:
        offs.append(pos)
        pos += len(b) + gap
    host = np.full(pos + 16, 0x5A, np.uint8)
    for o, b in zip(offs, buffers):
        host[o:o + len(b)] = np.frombuffer(bytes(b), np.uint8)
    d = _torch().from_numpy(host).to(_dev())
    assert d.data_ptr() % 16 == 0
    return d, offs, [len(b) for b in buffers]


# ---- decode -----------------------------------------------------------------------------------------

def run_decode(bl, fmt, streams, caps, max_chunks, max_fragments=0, with_chunks=True):
    """One smb_uncompress_streams_device call over the streams laid back to back; every output has
    its cap bytes in a guard-filled buffer with at least 16 guard bytes on both sides, at odd places."""
    torch = _torch()
    d_in, in_off, in_len = lay(streams)
    offs, pos = [], 33
    for c in caps:
        offs.append(pos)
        pos += c + 16 + (c % 3)
    d_out = torch.full((pos + 32,), GUARD, dtype=torch.uint8, device=_dev())
    k = len(streams)
    d_ol = torch.full((k,), -1, dtype=torch.int64, device=_dev())
    d_st = torch.full((k,), 77, dtype=torch.int32, device=_dev())
    d_cf = torch.full((k + 1,), -1, dtype=torch.int32, device=_dev()) if with_chunks else None
    d_cs = torch.full((max(max_chunks, 1),), 77, dtype=torch.int32, device=_dev()) if with_chunks else None
    bl.uncompress_block_streams_device(fmt, d_in, _i64(in_off), _i64(in_len), max_chunks, max_fragments, d_out, _i64(offs),
                                       _i64(caps), d_ol, d_st, d_cf, d_cs)
    torch.cuda.synchronize()
    return dict(status=d_st.cpu().tolist(), length=d_ol.cpu().tolist(), out=d_out.cpu().numpy(), offs=offs,
                first=d_cf.cpu().tolist() if with_chunks else None,
                chunk_status=d_cs.cpu().tolist()[:max_chunks] if with_chunks else None)


def check_decode(fmt, streams, caps, models, res, max_chunks):
    """Per stream the status, the length and every good chunk's bytes against the model; the chunk
    statuses; and every byte outside the decoded streams' own content is still the guard's."""
    out, offs = res["out"], res["offs"]
    outside = np.ones(out.size, bool)
    wrong, first, want_cs = [], [0], []
    for s, (stream, m) in enumerate(zip(streams, models)):
        ok = (res["status"][s], res["length"][s]) == (m.status, m.length)
        if m.slots:
            assert m.length <= caps[s]
            outside[offs[s]:offs[s] + m.length] = False
            for piece, c in zip(m.pieces, R.walk(stream, fmt)[1]):
                if piece is not None:
                    ok = ok and out[offs[s] + c.out:offs[s] + c.out + c.ulen].tobytes() == piece
        first.append(first[-1] + m.slots)
        want_cs += m.chunk_status
        if not ok:
            wrong.append((s, res["status"][s], res["length"][s], m.status, m.length))
    assert not wrong, wrong[:8]
    assert (out[outside] == GUARD).all()
    if res["first"] is not None:
        assert res["first"] == first
        assert res["chunk_status"] == want_cs + [0] * (max_chunks - len(want_cs))


def models_of(fmt, streams, caps):
    return [R.model(s, fmt, c, _oracle()) for s, c in zip(streams, caps)]


def room_for(fmt, streams):
    totals = [R.walk(s, fmt)[2] for s in streams]
    return [t if t <= ROOM else 0 for t in totals]


@functools.lru_cache(maxsize=None)
def mixed_batch(fmt):
    streams = [c[2] for c in R.cases_of(fmt)]
    for kind in ("text", "random"):
        streams += [encoded(fmt, kind, n)[1] for n in (0, 1, 65535, 65536, 65537, 131073)]
    caps = room_for(fmt, streams)
    return streams, caps, models_of(fmt, streams, caps)


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_decode_mixed_batch(bl, fmt):
    streams, caps, models = mixed_batch(fmt)
    cases = R.cases_of(fmt)
    assert all(m.status == c[3] for m, c in zip(models, cases) if c[3] != 0)
    assert all(m.status == 0 for m in models[len(cases):])
    assert b"".join(models[-1].pieces) == rand(131073) and b"".join(models[-7].pieces) == text(131073)
    total = sum(m.slots for m in models)
    res = run_decode(bl, fmt, streams, caps, total)
    check_decode(fmt, streams, caps, models, res, total)
    # the host plan says the same before any decode, and its fragment bound changes nothing
    rc, first, out_len, status, chunks, frags = bl.streams_plan(streams, fmt, out_cap=caps)
    assert (rc, chunks, first.tolist()) == (0, total, res["first"])
    assert [st for st, m in zip(status.tolist(), models) if m.slots == 0] == [m.status for m in models if m.slots == 0]
    again = run_decode(bl, fmt, streams, caps, total, max_fragments=frags)
    assert (again["status"], again["length"]) == (res["status"], res["length"]) and (again["out"] == res["out"]).all()


def three_chunks(fmt, seed, middle=None):
    """(stream, content): three small chunks in one HADOOP block or behind one XERIAL header;
    `middle` replaces the second chunk's payload."""
    O = _oracle()
    parts = [text(9000)[seed:seed + 5000], rand(300, seed), text(9000)[5000 + seed:9000]]
    pays = [O.compress(p) for p in parts]
    declared = [len(p) for p in parts]
    if middle is not None:
        pays[1], declared[1] = middle, R.parse_varint(middle)[0]
    body = b"".join(R.chunk(p) for p in pays)
    stream = (R.be(sum(declared)) if fmt == R.HADOOP else R.HEADER) + body
    return stream, parts


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_a_corrupt_chunk_fails_alone(bl, fmt):
    good = [three_chunks(fmt, seed)[0] for seed in (0, 11, 22, 33)]
    # the middle chunk: 10 bytes declared, the literal "ab", then a copy with offset 0
    bad, parts = three_chunks(fmt, 11, middle=b"\x0a\x04ab\x11\x00")
    streams = [good[0], bad, good[2], good[3]]
    caps = room_for(fmt, streams)
    models = models_of(fmt, streams, caps)
    assert [m.status for m in models] == [0, R.SM_ERR_COPY_OFFSET, 0, 0]
    assert models[1].chunk_status == [0, R.SM_ERR_COPY_OFFSET, 0] and models[1].pieces[0] == parts[0] and models[1].pieces[2] == parts[2]
    res = run_decode(bl, fmt, streams, caps, 12)
    check_decode(fmt, streams, caps, models, res, 12)
    assert res["chunk_status"] == [0] * 4 + [R.SM_ERR_COPY_OFFSET] + [0] * 7


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_capacity_one_byte_short(bl, fmt):
    streams = [three_chunks(fmt, seed)[0] for seed in (0, 11, 22)]
    caps = room_for(fmt, streams)
    caps[1] -= 1
    models = models_of(fmt, streams, caps)
    assert [m.status for m in models] == [0, R.SM_BUFFER_TOO_SMALL, 0] and models[1].length == caps[1] + 1
    res = run_decode(bl, fmt, streams, caps, 6)
    check_decode(fmt, streams, caps, models, res, 6)  # (the guard check covers the short stream's whole range)


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_slot_bound(bl, fmt):
    streams, caps, models = mixed_batch(fmt)
    keep = [i for i, m in enumerate(models) if m.length <= 70000]  # (the small ones: the bound is the point)
    streams, caps, models = [streams[i] for i in keep], [caps[i] for i in keep], [models[i] for i in keep]
    total = sum(m.slots for m in models)
    res = run_decode(bl, fmt, streams, caps, total)
    check_decode(fmt, streams, caps, models, res, total)
    res = run_decode(bl, fmt, streams, caps, total + 3, with_chunks=False)  # (spare slots decode nothing)
    check_decode(fmt, streams, caps, models, res, total + 3)
    res = run_decode(bl, fmt, streams, caps, total - 1)
    k = len(streams)
    assert res["status"] == [ARG] * k and res["length"] == [0] * k and (res["out"] == GUARD).all()
    assert res["chunk_status"] == [0] * (total - 1)


@pytest.mark.parametrize("nstreams", [1, 4, 5, 257])
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_one_chunk_streams(bl, fmt, nstreams):
    O = _oracle()
    want = [bytes([65 + s % 26]) * (1 + s % 40) + b"%d" % s for s in range(nstreams)]
    streams = [R.encode(w, fmt, O.compress) for w in want]
    caps = [len(w) for w in want]
    models = models_of(fmt, streams, caps)
    assert [b"".join(m.pieces) for m in models] == want
    res = run_decode(bl, fmt, streams, caps, nstreams)
    check_decode(fmt, streams, caps, models, res, nstreams)


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_many_chunks_in_one_stream(bl, fmt):
    content = bytes((7 * i + i // 256) & 0xFF for i in range(1025))
    body = b"".join(R.chunk(R.lit(content[i:i + 1])) for i in range(1025))  # 1,025 one-byte chunks: the scan's tile edge
    long_stream = (R.be(1025) if fmt == R.HADOOP else R.HEADER) + body
    streams = [R.encode(b"", fmt, _oracle().compress), long_stream, b"", R.encode(b"tail", fmt, _oracle().compress)]
    caps = [0, 1025, 0, 4]
    models = models_of(fmt, streams, caps)
    assert [m.slots for m in models] == [0, 1025, 0, 1] and b"".join(models[1].pieces) == content
    assert models[2].status == (0 if fmt == R.HADOOP else R.NO_HEADER)
    for slots in (1026, 1100):
        res = run_decode(bl, fmt, streams, caps, slots)
        check_decode(fmt, streams, caps, models, res, slots)


def literal(data):
    """one literal element of any length up to 2^24"""
    n = len(data) - 1
    if n < 60:
        return bytes([n << 2]) + data
    if n < 1 << 16:
        return bytes([61 << 2]) + n.to_bytes(2, "little") + data
    return bytes([62 << 2]) + n.to_bytes(3, "little") + data


def test_large_hadoop_chunk_by_fragments(bl):
    """A block of 200,000 bytes as one chunk, the payload written by a 64 KiB-block compressor: with
    the plan's fragment bound it decodes by fragments, with 0 in stream order, to the same bytes."""
    data = text(200000)
    stream = R.be(200000) + R.chunk(_oracle().compress(data))
    small = R.encode(b"abc", R.HADOOP, _oracle().compress)
    streams, caps = [small, stream, small], [3, 200000, 3]
    models = models_of(R.HADOOP, streams, caps)
    assert [m.status for m in models] == [0, 0, 0] and models[1].pieces == [data]
    rc, _, _, _, chunks, frags = bl.streams_plan(streams, "hadoop", out_cap=caps)
    assert (rc, chunks, frags) == (0, 3, 6)
    res = run_decode(bl, R.HADOOP, streams, caps, 3, max_fragments=frags)
    assert bl.last_indexed(0) == 1
    check_decode(R.HADOOP, streams, caps, models, res, 3)
    res0 = run_decode(bl, R.HADOOP, streams, caps, 3, max_fragments=0)
    assert bl.last_indexed(0) == 0
    check_decode(R.HADOOP, streams, caps, models, res0, 3)
    assert (res0["out"] == res["out"]).all()
    res1 = run_decode(bl, R.HADOOP, streams, caps, 3, max_fragments=frags - 1)  # a bound too small: stream order
    assert bl.last_indexed(0) == 0 and (res1["out"] == res["out"]).all() and res1["status"] == [0, 0, 0]


def test_large_chunk_with_a_copy_across_64k(bl):
    """The same size, hand-made: a copy that crosses the 64 KiB multiple, which no block compressor
    writes.  The index builder gives it up and the chunk decodes in stream order."""
    data = bytearray(rand(200000, 5))
    data[65532:65540] = data[65432:65440]  # 8 bytes from 100 back, across 65536
    data = bytes(data)
    payload = (R.varint(200000) + literal(data[:65532]) + bytes([(7 << 2) | 2]) + (100).to_bytes(2, "little") +
               literal(data[65540:]))
    assert _oracle().uncompress(payload) == data
    for fmt in R.FORMATS:
        stream = (R.be(200000) if fmt == R.HADOOP else R.HEADER) + R.chunk(payload)
        models = models_of(fmt, [stream], [200000])
        assert models[0].pieces == [data]
        res = run_decode(bl, fmt, [stream], [200000], 1, max_fragments=4)
        assert bl.last_indexed(0) == 0
        check_decode(fmt, [stream], [200000], models, res, 1)


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_libsnappy_payloads(bl, fmt, libsnappy):
    datas = [text(70000), rand(3000), b"", text(1), text(218000)]
    streams = [R.encode(d, fmt, libsnappy.compress) for d in datas[:4]]
    # libsnappy's own blocks: one chunk of 218,000 bytes (the size Hadoop's default buffer gives)
    streams.append((R.be(218000) if fmt == R.HADOOP else R.HEADER) + R.chunk(libsnappy.compress(datas[4])))
    caps = [len(d) for d in datas]
    models = models_of(fmt, streams, caps)
    assert [b"".join(m.pieces) for m in models] == datas
    rc, _, _, _, chunks, frags = bl.streams_plan(streams, fmt, out_cap=caps)
    res = run_decode(bl, fmt, streams, caps, chunks, max_fragments=frags)
    assert bl.last_indexed(0) == 1
    check_decode(fmt, streams, caps, models, res, chunks)


# ---- compress ---------------------------------------------------------------------------------------

LENGTHS = (0, 1, 65535, 65536, 65537, 131073)


def run_compress(bl, fmt, datas, mode, max_blocks=None):
    """One smb_compress_streams_device call over misaligned inputs; every stream has its max_length in
    a guard-filled buffer, at least 16 guard bytes between.  Returns (statuses, lengths, the buffer,
    the offsets)."""
    torch = _torch()
    d_in, in_off, in_len = lay(datas, lead=3, gap=5)
    offs, pos = [], 35
    for d in datas:
        offs.append(pos)
        pos += R.max_length(len(d), fmt) + 16 + len(d) % 5
    d_out = torch.full((pos + 32,), GUARD, dtype=torch.uint8, device=_dev())
    k = len(datas)
    d_ol = torch.full((k,), -1, dtype=torch.int64, device=_dev())
    d_st = torch.full((k,), 77, dtype=torch.int32, device=_dev())
    blocks = sum(-(-len(d) // BLOCK) for d in datas)
    bl.compress_block_streams_device(fmt, d_in, _i64(in_off), _i64(in_len), blocks if max_blocks is None else max_blocks,
                                     d_out, _i64(offs), d_ol, d_st, mode=mode)
    torch.cuda.synchronize()
    return d_st.cpu().tolist(), d_ol.cpu().tolist(), d_out.cpu().numpy(), offs


def written(fmt, datas, st, lens, out, offs):
    """The streams, after checking that nothing but them was written."""
    assert st == [0] * len(datas)
    outside = np.ones(out.size, bool)
    res = []
    for d, n, o in zip(datas, lens, offs):
        assert 0 < n <= R.max_length(len(d), fmt)
        outside[o:o + n] = False
        res.append(out[o:o + n].tobytes())
    assert (out[outside] == GUARD).all()
    return res


def batch_inputs():
    return [text(n) for n in LENGTHS] + [rand(n) for n in LENGTHS]


@pytest.mark.parametrize("mode", ["reference", "fast", "dense"])
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_compress(bl, fmt, mode):
    datas = batch_inputs()
    got = written(fmt, datas, *run_compress(bl, fmt, datas, mode))
    if mode == "reference":
        want = [R.encode(d, fmt, _oracle().compress) for d in datas]
        wrong = [s for s, (g, w) in enumerate(zip(got, want)) if g != w]
        assert not wrong, wrong
    for s, (d, g) in enumerate(zip(datas, got)):
        assert R.decode(g, fmt, _oracle()) == d, s
        chunks = R.walk(g, fmt)[1]
        assert [c.ulen for c in chunks] == [min(BLOCK, len(d) - o) for o in range(0, len(d), BLOCK)], s
    # the host-buffer call and the Python calls give the device call's bytes
    assert bl.compress_block_streams(datas, fmt, mode=mode) == got
    one = {R.HADOOP: bl.compress_hadoop, R.XERIAL: bl.compress_xerial}[fmt]
    assert [one(datas[i], mode=mode) for i in (0, 1, 5)] == [got[i] for i in (0, 1, 5)]
    blocks = sum(-(-len(d) // BLOCK) for d in datas)
    st, lens, out, offs = run_compress(bl, fmt, datas, mode, max_blocks=blocks - 1)
    assert st == [ARG] * len(datas) and lens == [0] * len(datas) and (out == GUARD).all()


@pytest.mark.parametrize("nstreams", [1, 257])
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_compress_many_small_streams(bl, fmt, nstreams):
    datas = [text(300)[s:s + s % 23] for s in range(nstreams)]  # (empty ones among them)
    got = written(fmt, datas, *run_compress(bl, fmt, datas, "reference"))
    assert got == [R.encode(d, fmt, _oracle().compress) for d in datas]


# ---- the host-buffer calls and Python ---------------------------------------------------------------

@pytest.mark.parametrize("fmt", R.FORMATS)
def test_python_round_trip(bl, fmt):
    assert bl.compress_block_streams([], fmt) == [] and bl.uncompress_block_streams([], fmt) == []
    assert bl.uncompress_block_streams([], fmt, statuses=True) == ([], [])
    datas = [b"", text(1), rand(70000), text(200000), b"", rand(5), np.frombuffer(text(1000), np.uint8)]
    streams = bl.compress_block_streams(datas, fmt)
    empty = R.be(0) if fmt == R.HADOOP else R.HEADER
    assert streams[0] == streams[4] == empty
    assert bl.compress_block_streams([datas[3]], fmt, mode="reference")[0] == R.encode(datas[3], fmt, _oracle().compress)
    assert bl.uncompress_block_streams(streams, fmt) == [bytes(d) for d in datas]
    one = {R.HADOOP: bl.uncompress_hadoop, R.XERIAL: bl.uncompress_xerial}[fmt]
    assert [one(s) for s in streams[:3]] == [bytes(d) for d in datas[:3]]
    # one bad stream: the raising form names it, the other form hands out the rest
    cut = streams[2][:-1]  # (its last payload a byte short)
    batch = streams[:2] + [cut] + streams[3:]
    with pytest.raises(bl.BlocksError) as e:
        bl.uncompress_block_streams(batch, fmt)
    assert (e.value.code, e.value.stream) == (R.TRUNCATED, 2)
    with pytest.raises(bl.BlocksError) as e:
        one(cut)
    assert (e.value.code, e.value.stream) == (R.TRUNCATED, None)
    out, st = bl.uncompress_block_streams(batch, fmt, statuses=True)
    assert st == [0, 0, R.TRUNCATED, 0, 0, 0, 0]
    assert out == [bytes(d) if i != 2 else None for i, d in enumerate(datas)]
    # a foreign stream with a chunk of more than 64 KiB, through the host-buffer call: by fragments
    big = (R.be(200000) if fmt == R.HADOOP else R.HEADER) + R.chunk(_oracle().compress(text(200000)))
    assert bl.uncompress_block_streams([big, streams[1]], fmt) == [text(200000), text(1)] and bl.last_indexed(0) == 1


def test_host_buffer_call_keeps_to_each_streams_own_bytes(bl):
    fmt = R.HADOOP
    streams = [encoded(fmt, "text", 65537)[1], R.be(2) + R.chunk(R.ABC), encoded(fmt, "random", 1)[1]]
    buf = np.frombuffer(b"".join(streams), np.uint8)
    in_len = np.array([len(s) for s in streams], np.uint64)
    in_off = np.array([0, len(streams[0]), len(streams[0]) + len(streams[1])], np.uint64)
    out = np.full(65537 + 100, GUARD, np.uint8)
    out_off = np.array([20, 7, 3], np.uint64)
    out_cap = np.array([65537, 9, 0], np.uint64)  # (the last one: a byte short)
    out_len, status = np.zeros(3, np.uint64), np.full(3, 77, np.int32)
    rc = bl.lib().smb_uncompress_streams(bl.context(0), 0, buf.ctypes.data, in_off.ctypes.data, in_len.ctypes.data, 3,
                                         out.ctypes.data, out_off.ctypes.data, out_cap.ctypes.data, out_len.ctypes.data,
                                         status.ctypes.data)
    assert (rc, status.tolist(), out_len.tolist()) == (0, [0, R.BLOCK_LENGTH, R.SM_BUFFER_TOO_SMALL], [65537, 3, 1])
    assert out[20:20 + 65537].tobytes() == text(65537) and (out[:20] == GUARD).all() and (out[20 + 65537:] == GUARD).all()
