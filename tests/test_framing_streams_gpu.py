"""The framing library's batched stream calls on the GPU (snappy.jl_amd/framing.py over
libsnappy_mi355x_framing.so): smf_uncompress_streams_device and smf_compress_streams_device over
mixed batches laid back to back, isolation between the streams of a batch, the capacity and slot
bounds, workgroup and scan-tile edges, and the host-buffer and Python calls.  Every expected value
comes from the plain-Python references (tests/framing_ref.py, tests/framing_streams_ref.py) and the
CPU oracle; the single-stream calls are run beside the batch as a second witness."""
import ctypes
import functools
import importlib

import numpy as np
import pytest

import framing_ref as R
import framing_streams_ref as SR
from conftest import load_package, read_testfile

pytestmark = pytest.mark.gpu

BLOCK = 65536
GUARD = 0xA5
ARG = SR.SM_ERR_ARGUMENT
SM_ERR_COPY_OFFSET = 19


@pytest.fixture(scope="module")
def fr(gpu_available):
    load_package()
    return importlib.import_module("snappy_jl_amd.framing")


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
def encoded(kind, n):
    """(input, its reference-mode framed stream by the Python encoder)"""
    data = text(n) if kind == "text" else rand(n)
    return data, R.encode(data, _oracle())


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

def run_decode(fr, streams, caps, max_chunks, with_chunks=True):
    """One smf_uncompress_streams_device call over the streams laid back to back; every output has
    its cap bytes in a guard-filled buffer with 16 guard bytes on both sides, at odd places."""
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
    fr.uncompress_framed_streams_device(d_in, _i64(in_off), _i64(in_len), max_chunks, d_out, _i64(offs), _i64(caps), d_ol,
                                        d_st, d_cf, d_cs)
    torch.cuda.synchronize()
    return dict(status=d_st.cpu().tolist(), length=d_ol.cpu().tolist(), out=d_out.cpu().numpy(), offs=offs,
                first=d_cf.cpu().tolist() if with_chunks else None,
                chunk_status=d_cs.cpu().tolist()[:max_chunks] if with_chunks else None)


def check_decode(streams, caps, models, res, max_chunks):
    """Per stream the status, the length and every good chunk's bytes against the model; the chunk
    statuses; and every byte outside the decoded streams' own content is still the guard's."""
    out, offs = res["out"], res["offs"]
    outside = np.ones(out.size, bool)
    wrong, first, want_cs = [], [0], []
    for s, (stream, m) in enumerate(zip(streams, models)):
        ok = (res["status"][s], res["length"][s]) == (m.status, m.length)
        if m.slots:
            at = offs[s]
            assert m.length <= caps[s]
            outside[at:at + m.length] = False
            for piece, chunk in zip(m.pieces, R.walk(stream)):
                if piece is not None:
                    ok = ok and out[at:at + chunk[4]].tobytes() == piece
                at += chunk[4]
        first.append(first[-1] + m.slots)
        want_cs += m.chunk_status
        if not ok:
            wrong.append((s, res["status"][s], res["length"][s], m.status, m.length))
    assert not wrong, wrong[:8]
    assert (out[outside] == GUARD).all()
    if res["first"] is not None:
        assert res["first"] == first
        assert res["chunk_status"] == want_cs + [0] * (max_chunks - len(want_cs))


def single_stream(fr, stream, cap):
    """smf_uncompress_device on the stream alone with out_capacity = cap: (status, length, bytes)."""
    torch = _torch()
    d_in, off, _ = lay([stream])
    d_out = torch.full((cap + 64,), GUARD, dtype=torch.uint8, device=_dev())
    d_ol = torch.full((1,), -1, dtype=torch.int64, device=_dev())
    d_st = torch.full((1,), 77, dtype=torch.int32, device=_dev())
    stream_handle = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = fr.lib().smf_uncompress_device(fr.context(0), ctypes.c_void_p(d_in.data_ptr() + off[0]), len(stream),
                                        ctypes.c_void_p(d_out.data_ptr()), cap, ctypes.c_void_p(d_ol.data_ptr()),
                                        ctypes.c_void_p(d_st.data_ptr()), stream_handle)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert (out[cap:] == GUARD).all() and rc in (0, int(d_st.item()))
    return int(d_st.item()), int(d_ol.item()), out[:cap]


@functools.lru_cache(maxsize=None)
def mixed_batch():
    streams = [c[1] for c in R.structural_cases()]
    for kind in ("text", "random"):
        streams += [encoded(kind, n)[1] for n in (0, 1, 65535, 65536, 65537, 131073)]
    caps = [sum(c[4] for c in SR.walk_prefix(s)[0]) for s in streams]
    models = [SR.model(s, c, _oracle()) for s, c in zip(streams, caps)]
    return streams, caps, models


def test_decode_mixed_batch(fr):
    streams, caps, models = mixed_batch()
    nstruct = len(R.structural_cases())
    # (a well-formed case may still fail its decode or its CRC: the model says)
    assert all(m.status == c[2] for m, c in zip(models, R.structural_cases()) if c[2] != 0)
    assert {m.status for m in models[:nstruct]} > {0, R.CRC, R.TRUNCATED} and all(m.status == 0 for m in models[nstruct:])
    assert b"".join(models[-1].pieces) == rand(131073) and b"".join(models[-7].pieces) == text(131073)
    total = sum(m.slots for m in models)
    res = run_decode(fr, streams, caps, total)
    check_decode(streams, caps, models, res, total)
    # the same from the single-stream call, stream by stream
    for s, (stream, cap, m) in enumerate(zip(streams, caps, models)):
        st, length, out = single_stream(fr, stream, cap)
        assert (st, length) == (res["status"][s], res["length"][s]) == (m.status, m.length), s
        if m.status == 0:
            assert out.tobytes() == res["out"][res["offs"][s]:res["offs"][s] + cap].tobytes() == b"".join(m.pieces), s


def three_chunks(seed):
    """(stream, content): a compressed, an uncompressed and a compressed chunk, all small."""
    a, b, c = text(9000)[seed:seed + 5000], rand(300, seed), text(9000)[5000 + seed:9000]
    O = _oracle()
    stream = R.IDENTIFIER + R.compressed_chunk(a, O) + R.raw_chunk(b) + R.compressed_chunk(c, O)
    assert [ch[0] for ch in R.walk(stream)] == [0, 1, 0]
    return stream, a + b + c


def test_isolation(fr):
    good = [three_chunks(seed)[0] for seed in (0, 11, 22, 33)]
    caps = [sum(c[4] for c in R.walk(s)) for s in good]
    victim = 1
    chunks = R.walk(good[victim])
    flipped = bytearray(good[victim])
    flipped[chunks[1][1] - 3] ^= 0x01  # the second chunk's stored CRC
    # the third chunk's payload: 10 bytes declared, the literal "ab", then a copy from offset 5
    bad_copy = good[victim][:chunks[2][1] - 8] + R.chunk(0x00, R.crc_field(b"") + b"\x0a\x04ab\x11\x05")
    cut = good[victim][:-7]  # in the middle of its last chunk; the next stream follows directly
    damages = [(bytes(flipped), R.CRC, [0, R.CRC, 0]), (bad_copy, SM_ERR_COPY_OFFSET, [0, 0, SM_ERR_COPY_OFFSET]),
               (cut, R.TRUNCATED, [])]
    clean = [SR.model(s, c, _oracle()) for s, c in zip(good, caps)]
    assert all(m.status == 0 and m.slots == 3 for m in clean)
    for damaged, status, chunk_status in damages:
        streams = list(good)
        streams[victim] = damaged
        these = list(caps)
        if status == SM_ERR_COPY_OFFSET:
            these[victim] = caps[victim] - chunks[2][4] + 10  # (its third chunk now declares 10 bytes)
        models = [SR.model(s, c, _oracle()) for s, c in zip(streams, these)]
        assert models[victim].status == status and models[victim].chunk_status == chunk_status
        assert [m for i, m in enumerate(models) if i != victim] == [m for i, m in enumerate(clean) if i != victim]
        total = sum(m.slots for m in models)
        assert total == (9 if status == R.TRUNCATED else 12)
        res = run_decode(fr, streams, these, total)
        check_decode(streams, these, models, res, total)
        assert [st for i, st in enumerate(res["status"]) if i != victim] == [0, 0, 0]


def test_capacity_one_byte_short(fr):
    good = [three_chunks(seed)[0] for seed in (0, 11, 22)]
    caps = [sum(c[4] for c in R.walk(s)) for s in good]
    caps[1] -= 1
    models = [SR.model(s, c, _oracle()) for s, c in zip(good, caps)]
    assert [m.status for m in models] == [0, R.SM_BUFFER_TOO_SMALL, 0] and models[1].length == caps[1] + 1
    res = run_decode(fr, good, caps, 6)
    check_decode(good, caps, models, res, 6)  # (the guard check covers the short stream's whole range)


def test_slot_bound(fr):
    streams, caps, models = mixed_batch()
    keep = [i for i, m in enumerate(models) if m.length <= 70000]  # (the small ones: the bound is the point)
    streams, caps, models = [streams[i] for i in keep], [caps[i] for i in keep], [models[i] for i in keep]
    total = sum(m.slots for m in models)
    res = run_decode(fr, streams, caps, total)
    check_decode(streams, caps, models, res, total)
    res = run_decode(fr, streams, caps, total - 1)
    k = len(streams)
    assert res["status"] == [ARG] * k and res["length"] == [0] * k and (res["out"] == GUARD).all()
    assert res["chunk_status"] == [0] * (total - 1)


@pytest.mark.parametrize("nstreams", [1, 3, 4, 5, 64, 65, 256, 257])
def test_one_chunk_streams(fr, nstreams):
    O = _oracle()
    streams, want = [], []
    for s in range(nstreams):
        data = bytes([65 + s % 26]) * (1 + s % 40) + b"%d" % s
        c = R.compressed_chunk(data, O) if s % 3 == 0 else R.raw_chunk(data)
        streams.append(R.IDENTIFIER + c)
        want.append(data)
    caps = [len(w) for w in want]
    models = [SR.model(s, c, O) for s, c in zip(streams, caps)]
    assert [b"".join(m.pieces) for m in models] == want
    res = run_decode(fr, streams, caps, nstreams)
    check_decode(streams, caps, models, res, nstreams)


def test_many_chunks_in_one_stream(fr):
    long_stream, content = SR.long_foreign_stream(300)
    assert len(R.walk(long_stream)) == 300 and R.decode(long_stream, _oracle()) == content
    streams = [R.IDENTIFIER, long_stream, b"", R.IDENTIFIER + R.raw_chunk(b"tail")]
    caps = [0, 300, 0, 4]
    models = [SR.model(s, c, _oracle()) for s, c in zip(streams, caps)]
    assert [m.status for m in models] == [0, 0, R.NO_IDENTIFIER, 0] and [m.slots for m in models] == [0, 300, 0, 1]
    for slots in (301, 400):
        res = run_decode(fr, streams, caps, slots)
        check_decode(streams, caps, models, res, slots)
    res = run_decode(fr, streams, caps, 301, with_chunks=False)
    check_decode(streams, caps, models, res, 301)


# ---- compress ---------------------------------------------------------------------------------------

LENGTHS = (0, 1, 65535, 65536, 65537, 196608, 196609)


def run_compress(fr, datas, mode, max_blocks=None):
    """One smf_compress_streams_device call over misaligned inputs; every stream has its
    max_framed_length in a guard-filled buffer, 16 guard bytes between.  Returns (statuses,
    lengths, the buffer, the offsets)."""
    torch = _torch()
    d_in, in_off, in_len = lay(datas, lead=3, gap=5)
    offs, pos = [], 35
    for d in datas:
        offs.append(pos)
        pos += R.max_framed_length(len(d)) + 16 + len(d) % 5
    d_out = torch.full((pos + 32,), GUARD, dtype=torch.uint8, device=_dev())
    k = len(datas)
    d_ol = torch.full((k,), -1, dtype=torch.int64, device=_dev())
    d_st = torch.full((k,), 77, dtype=torch.int32, device=_dev())
    blocks = sum(-(-len(d) // BLOCK) for d in datas)
    fr.compress_framed_streams_device(d_in, _i64(in_off), _i64(in_len), blocks if max_blocks is None else max_blocks, d_out,
                                      _i64(offs), d_ol, d_st, mode=mode)
    torch.cuda.synchronize()
    return d_st.cpu().tolist(), d_ol.cpu().tolist(), d_out.cpu().numpy(), offs


def framed_outputs(datas, st, lens, out, offs):
    """The framed streams, after checking that nothing but them was written."""
    assert st == [0] * len(datas)
    outside = np.ones(out.size, bool)
    res = []
    for d, n, o in zip(datas, lens, offs):
        assert 10 <= n <= R.max_framed_length(len(d))
        outside[o:o + n] = False
        res.append(out[o:o + n].tobytes())
    assert (out[outside] == GUARD).all()
    return res


def compress_batches():
    every = [encoded(kind, n) for kind in ("text", "random") for n in LENGTHS]
    tiny = [(text(300)[s:s + s % 23], None) for s in range(257)]
    return {1: [encoded("text", 196609)], 5: [every[i] for i in (0, 8, 2, 10, 4)], 14: every, 257: tiny}


@pytest.mark.parametrize("nstreams", [1, 5, 14, 257])
def test_compress_reference_mode(fr, nstreams):
    batch = compress_batches()[nstreams]
    datas = [b[0] for b in batch]
    want = [b[1] if b[1] is not None else R.encode(b[0], _oracle()) for b in batch]
    got = framed_outputs(datas, *run_compress(fr, datas, "reference"))
    wrong = [s for s, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not wrong, wrong[:8]
    if nstreams == 14:
        assert {c[0] for w in want for c in R.walk(w)} == {0, 1} and want[0] == R.IDENTIFIER


def compress_alone(fr, data, mode):
    torch = _torch()
    d_in, off, _ = lay([data], lead=3)
    d_out = torch.full((R.max_framed_length(len(data)),), GUARD, dtype=torch.uint8, device=_dev())
    d_len = torch.full((1,), -1, dtype=torch.int64, device=_dev())
    d_st = torch.full((1,), 77, dtype=torch.int32, device=_dev())
    fr.compress_framed_device(d_in[off[0]:off[0] + len(data)], d_out, d_len, d_st, mode=mode)
    torch.cuda.synchronize()
    assert int(d_st.item()) == 0
    return d_out.cpu().numpy()[:int(d_len.item())].tobytes()


@pytest.mark.parametrize("mode", ["fast", "dense"])
def test_compress_fast_modes(fr, mode):
    datas = [encoded(kind, n)[0] for kind in ("text", "random") for n in (0, 1, 65535, 65537, 196609)]
    got = framed_outputs(datas, *run_compress(fr, datas, mode))
    for s, (d, g) in enumerate(zip(datas, got)):
        assert R.decode(g, _oracle()) == d, s
        assert g == compress_alone(fr, d, mode), s
    blocks = sum(-(-len(d) // BLOCK) for d in datas)
    st, lens, out, offs = run_compress(fr, datas, mode, max_blocks=blocks - 1)
    assert st == [ARG] * len(datas) and lens == [0] * len(datas) and (out == GUARD).all()


# ---- the host-buffer calls and Python ---------------------------------------------------------------

def test_python_round_trip(fr):
    assert fr.compress_framed_streams([]) == [] and fr.uncompress_framed_streams([]) == []
    assert fr.uncompress_framed_streams([], return_status=True) == ([], [])
    datas = [b"", text(1), rand(70000), text(131073), b"", rand(5), np.frombuffer(text(1000), np.uint8)]
    framed = fr.compress_framed_streams(datas)
    assert framed[0] == framed[4] == R.IDENTIFIER
    assert framed == [fr.compress_framed(bytes(d)) for d in datas]
    assert fr.compress_framed_streams([datas[3]], mode="reference")[0] == encoded("text", 131073)[1]
    assert fr.uncompress_framed_streams(framed) == [bytes(d) for d in datas]
    assert fr.uncompress_framed_streams([R.IDENTIFIER, b"", R.IDENTIFIER], return_status=True) == (
        [b"", None, b""], [0, R.NO_IDENTIFIER, 0])
    # one bad stream: the raising form names it, the other form hands out the rest
    bad = bytearray(framed[2])
    bad[-1] ^= 0x10
    batch = framed[:2] + [bytes(bad)] + framed[3:]
    with pytest.raises(fr.FramingError) as e:
        fr.uncompress_framed_streams(batch)
    want = SR.model(bytes(bad), 70000, _oracle()).status
    assert (e.value.code, e.value.stream) == (want, 2) and want != 0
    out, st = fr.uncompress_framed_streams(batch, return_status=True)
    assert st == [0, 0, want, 0, 0, 0, 0]
    assert out == [bytes(d) if i != 2 else None for i, d in enumerate(datas)]
    rc, first, out_len, status, total = fr.streams_plan(batch)
    assert (rc, status.tolist(), out_len.tolist()) == (0, [0] * 7, [len(d) for d in datas])
    assert first.tolist() == [0, 0, 1, 3, 6, 6, 7, 8] and total == 8


def test_host_buffer_call_keeps_to_each_streams_own_bytes(fr):
    streams = [encoded("text", 65537)[1], R.IDENTIFIER + R.chunk(0x02, b"abcd"), encoded("random", 1)[1]]
    buf = np.frombuffer(b"".join(streams), np.uint8)
    in_len = np.array([len(s) for s in streams], np.uint64)
    in_off = np.array([0, len(streams[0]), len(streams[0]) + len(streams[1])], np.uint64)
    out = np.full(65537 + 100, GUARD, np.uint8)
    out_off = np.array([20, 7, 3], np.uint64)
    out_cap = np.array([65537, 9, 0], np.uint64)  # (the last one: a byte short)
    out_len, status = np.zeros(3, np.uint64), np.full(3, 77, np.int32)
    rc = fr.lib().smf_uncompress_streams(fr.context(0), buf.ctypes.data, in_off.ctypes.data, in_len.ctypes.data, 3,
                                         out.ctypes.data, out_off.ctypes.data, out_cap.ctypes.data, out_len.ctypes.data,
                                         status.ctypes.data)
    assert (rc, status.tolist(), out_len.tolist()) == (0, [0, R.RESERVED_CHUNK, R.SM_BUFFER_TOO_SMALL], [65537, 0, 1])
    assert out[20:20 + 65537].tobytes() == text(65537) and (out[:20] == GUARD).all() and (out[20 + 65537:] == GUARD).all()
