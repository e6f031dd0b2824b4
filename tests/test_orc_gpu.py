"""The ORC library's batched calls on the GPU (snappy.jl_amd/orc.py over libsnappy_mi355x_orc.so):
the two files an independent writer made, the encoder's compressed-or-stored choice against the
plain-Python reference built on this project's own raw compressor, the stored chunks' copy at every
source and destination alignment, mixed streams with a corrupt chunk and every structural error,
the two bounds, and the tensor wrappers on a side stream.  Every expected value comes from
tests/orc_ref.py, the CPU oracle and the committed fixture record."""
import functools
import hashlib
import importlib
import json
import os

import numpy as np
import pytest

import orc_ref as R
from conftest import ROOT, load_package, read_testfile

pytestmark = pytest.mark.gpu

GUARD = 0xA5
ARG = R.SM_ERR_ARGUMENT
GOLDEN = os.path.join(ROOT, "tests", "golden", "orc")
MODES = ("reference", "fast", "dense")


@pytest.fixture(scope="module")
def orc(gpu_available):
    load_package()
    return importlib.import_module("snappy_jl_amd.orc")


@pytest.fixture(scope="module")
def sm(gpu_available):
    return load_package()


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


def _status():
    return R.oracle_status(_oracle())


@functools.lru_cache(maxsize=None)
def content(kind, n):
    """n bytes of zeros, of html or of random1.bin (repeated where the file is shorter), or from a
    seeded generator"""
    if kind == "zeros":
        return bytes(n)
    if kind == "rng":
        return np.random.default_rng(9).integers(0, 256, n, dtype=np.uint8).tobytes()
    t = read_testfile("html" if kind == "html" else "random1.bin")
    return (t * (n // len(t) + 1))[:n]


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

def run_decode(orc, block_size, streams, caps, max_chunks, max_fragments=0, with_chunks=True):
    """One smo_uncompress_streams_device call over the streams laid back to back; every output has
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
    orc.uncompress_orc_streams_device(block_size, d_in, _i64(in_off), _i64(in_len), max_chunks, max_fragments, d_out,
                                      _i64(offs), _i64(caps), d_ol, d_st, d_cf, d_cs)
    torch.cuda.synchronize()
    return dict(status=d_st.cpu().tolist(), length=d_ol.cpu().tolist(), out=d_out.cpu().numpy(), offs=offs,
                first=d_cf.cpu().tolist() if with_chunks else None,
                chunk_status=d_cs.cpu().tolist()[:max_chunks] if with_chunks else None)


def check_decode(block_size, streams, caps, models, res, max_chunks):
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
            for piece, c in zip(m.pieces, R.walk(stream, block_size)[1]):
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


def models_of(block_size, streams, caps):
    return [R.model(s, block_size, c, _status()) for s, c in zip(streams, caps)]


# ---- an independent writer's files -------------------------------------------------------------------

@pytest.mark.parametrize("name", ["snappy_64k.orc", "snappy_256k.orc"])
def test_fixture_files(orc, name):
    with open(os.path.join(GOLDEN, "orc_fixture.json")) as f:
        rec = json.load(f)["files"][name]
    with open(os.path.join(GOLDEN, name), "rb") as f:
        body = R.file_streams(f.read())
    bs, total = rec["block_size"], rec["decoded_bytes"]
    rc, first, out_len, status, chunks, frags = orc.streams_plan([body], bs, out_cap=[total])
    assert (rc, status.tolist(), out_len.tolist(), chunks) == (0, [0], [total], rec["chunks"])
    for max_fragments in (frags, 0):
        res = run_decode(orc, bs, [body], [total], chunks, max_fragments=max_fragments)
        assert (res["status"], res["length"], res["first"]) == ([0], [total], [0, chunks])
        assert res["chunk_status"] == [0] * chunks
        got = res["out"][res["offs"][0]:res["offs"][0] + total]
        assert hashlib.sha256(got.tobytes()).hexdigest() == rec["sha256"]
        outside = np.ones(res["out"].size, bool)
        outside[res["offs"][0]:res["offs"][0] + total] = False
        assert (res["out"][outside] == GUARD).all()
        if name == "snappy_256k.orc" and max_fragments:
            assert orc.last_indexed(0) >= 1  # the 164,000-byte chunk went by fragments
        if not max_fragments:
            assert orc.last_indexed(0) == 0
    # the host-buffer call and the Python call give the same bytes
    assert hashlib.sha256(orc.uncompress_orc(body, bs)).hexdigest() == rec["sha256"]


# ---- the encoder ------------------------------------------------------------------------------------

def run_compress(orc, block_size, datas, mode, max_pieces=None):
    """One smo_compress_streams_device call over misaligned inputs; every stream has its max_length in
    a guard-filled buffer, at least 16 guard bytes between.  Returns (statuses, lengths, the buffer,
    the offsets)."""
    torch = _torch()
    d_in, in_off, in_len = lay(datas, lead=3, gap=5)
    offs, pos = [], 35
    for d in datas:
        offs.append(pos)
        pos += R.max_length(len(d), block_size) + 16 + len(d) % 5
    d_out = torch.full((pos + 32,), GUARD, dtype=torch.uint8, device=_dev())
    k = len(datas)
    d_ol = torch.full((k,), -1, dtype=torch.int64, device=_dev())
    d_st = torch.full((k,), 77, dtype=torch.int32, device=_dev())
    pieces = sum(-(-len(d) // block_size) for d in datas)
    orc.compress_orc_streams_device(block_size, d_in, _i64(in_off), _i64(in_len), pieces if max_pieces is None else max_pieces,
                                    d_out, _i64(offs), d_ol, d_st, mode=mode)
    torch.cuda.synchronize()
    return d_st.cpu().tolist(), d_ol.cpu().tolist(), d_out.cpu().numpy(), offs


def written(block_size, datas, st, lens, out, offs):
    """The streams, after checking that nothing but them was written (a sentinel fill)."""
    assert st == [0] * len(datas)
    outside = np.ones(out.size, bool)
    res = []
    for d, n, o in zip(datas, lens, offs):
        assert 0 <= n <= R.max_length(len(d), block_size) and (n > 0) == (len(d) > 0)
        outside[o:o + n] = False
        res.append(out[o:o + n].tobytes())
    assert (out[outside] == GUARD).all()
    return res


def encoder_lengths(block_size):
    return (0, 1, block_size - 1, block_size, block_size + 1, 3 * block_size + 7)


def no_copy_can_pay(piece):
    """No 4-byte sequence occurs twice in the piece.  A copy element needs a match of 4 bytes, so
    such a piece's raw stream is its varint and one literal per fragment -- longer than the piece,
    whatever the compressor: the chunk must be a stored one."""
    if len(piece) < 8:
        return True
    b = np.frombuffer(piece, np.uint8).astype(np.uint32)
    words = b[:-3] | (b[1:-2] << 8) | (b[2:-1] << 16) | (b[3:] << 24)
    return np.unique(words).size == words.size


@pytest.mark.parametrize("block_size", [1, 64, 1000, 65536, 65537, 262144])
def test_encoder(orc, sm, block_size):
    """The three contents of the corpus and a fourth from a seeded generator.  random1.bin is not
    free of repeats (its five bytes at 27 recur at 32, its nine at 156 recur at 183), so a small piece of it can
    compress by a byte or two: its pieces must be stored wherever no copy can pay.  Of the
    generator's bytes every piece must be: a repeat of 4 bytes is too rare and too short there to
    win back a literal's tag (a 4-byte copy saves at most 2 bytes and splits a literal, which costs
    1 to 3), let alone the varint and the tags a raw stream starts with."""
    kinds = ("zeros", "html", "random", "rng")
    datas = [content(kind, n) for kind in kinds for n in encoder_lengths(block_size)]
    for mode in MODES:
        raw = functools.lru_cache(maxsize=None)(lambda piece: sm.compress(piece, mode=mode, device=0))
        got = written(block_size, datas, *run_compress(orc, block_size, datas, mode))
        want = [R.encode(d, block_size, raw) for d in datas]
        wrong = [(s, len(g), len(w)) for s, (g, w) in enumerate(zip(got, want)) if g != w]
        assert not wrong, (mode, wrong)
        for s, (d, g) in enumerate(zip(datas, got)):
            assert R.decode(g, block_size, _status()) == d, (mode, s)
            chunks = R.walk(g, block_size)[1]
            assert [c.ulen for c in chunks] == [len(p) for p in R.pieces(d, block_size)], (mode, s)
            kind = kinds[s // len(encoder_lengths(block_size))]
            if kind == "random":
                assert all(c.original for c, p in zip(chunks, R.pieces(d, block_size)) if no_copy_can_pay(p)), (mode, s)
            if kind == "rng":
                assert all(c.original for c in chunks), (mode, s)
            if kind == "zeros":  # (a run of zeros too short for a copy to pay is stored like anything else)
                assert all(not c.original for c in chunks if c.ulen >= 64), (mode, s)
        if mode == "fast":  # the host-buffer call and the Python calls give the device call's bytes
            fast = got
            assert orc.compress_orc_streams(datas, block_size, mode=mode) == got
            assert [orc.compress_orc(datas[i], block_size, mode=mode) for i in (0, 1, 5)] == [got[i] for i in (0, 1, 5)]
            assert orc.uncompress_orc_streams(got, block_size) == datas
    pieces = sum(-(-len(d) // block_size) for d in datas)
    st, lens, out, offs = run_compress(orc, block_size, datas, "fast", max_pieces=pieces - 1)
    assert st == [ARG] * len(datas) and lens == [0] * len(datas) and (out == GUARD).all()
    st, lens, out, offs = run_compress(orc, block_size, datas, "fast", max_pieces=pieces + 3)  # (spare slots pack nothing)
    assert written(block_size, datas, st, lens, out, offs) == fast


def test_encoder_many_pieces(orc):
    """More pieces than the pack's grid holds workgroups: 17,001 pieces of one byte, every one stored
    (a byte's raw stream has three), beside empty inputs; the scan's tile edges."""
    data = bytes((7 * i + i // 256) & 0xFF for i in range(17001))
    datas = [b"", data, b"", b"xy"]
    got = written(1, datas, *run_compress(orc, 1, datas, "fast"))
    assert got[1] == b"".join(b"\x03\x00\x00" + data[i:i + 1] for i in range(len(data)))
    assert got[0] == got[2] == b"" and got[3] == b"\x03\x00\x00x\x03\x00\x00y"


# ---- the stored chunks' copy ------------------------------------------------------------------------

def copy_case(orc, length, pairs, max_chunks=None):
    """One batch of single-chunk stored streams of `length` bytes, stream i's payload at an address
    that is pairs[i][0] mod 16 and its output at one that is pairs[i][1] mod 16.  The input tensor
    ends with the last payload byte and the output tensor with the last stream's capacity; every
    output has at least 16 sentinel bytes before it."""
    torch = _torch()
    rng = np.random.default_rng(length)
    payloads = [rng.integers(0, 256, length, dtype=np.uint8) for _ in pairs]
    in_off, out_off, pos, opos = [], [], 0, 16
    for (src, dst), p in zip(pairs, payloads):
        pos += (src - (pos + R.HEADER)) % 16  # the payload behind its 3-byte header, at src mod 16
        in_off.append(pos)
        pos += R.HEADER + length
        opos += (dst - opos) % 16
        out_off.append(opos)
        opos += length + 16
    host = np.full(pos, 0x5A, np.uint8)  # (ends with the last payload byte)
    for o, p in zip(in_off, payloads):
        host[o:o + R.HEADER] = np.frombuffer(R.header(length, True), np.uint8)
        host[o + R.HEADER:o + R.HEADER + length] = p
    d_in = torch.from_numpy(host).to(_dev())
    d_out = torch.full((opos - 16,), GUARD, dtype=torch.uint8, device=_dev())  # (ends with the last capacity)
    assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    k = len(pairs)
    d_ol = torch.full((k,), -1, dtype=torch.int64, device=_dev())
    d_st = torch.full((k,), 77, dtype=torch.int32, device=_dev())
    block_size = max(length, 1)
    orc.uncompress_orc_streams_device(block_size, d_in, _i64(in_off), _i64([R.HEADER + length] * k),
                                      k if max_chunks is None else max_chunks, 0, d_out, _i64(out_off), _i64([length] * k),
                                      d_ol, d_st)
    torch.cuda.synchronize()
    assert d_st.cpu().tolist() == [0] * k and d_ol.cpu().tolist() == [length] * k
    out = d_out.cpu().numpy()
    outside = np.ones(out.size, bool)
    wrong = []
    for i, (o, p) in enumerate(zip(out_off, payloads)):
        outside[o:o + length] = False
        if not (out[o:o + length] == p).all():
            wrong.append(pairs[i])
    assert not wrong, wrong[:8]
    assert (out[outside] == GUARD).all()


ALL_PAIRS = [(src, dst) for src in range(16) for dst in range(16)]


@pytest.mark.parametrize("length", [0, 1, 15, 16, 17, 255, 256, 257, 4095, 65537])
def test_stored_copy_every_alignment(orc, length):
    copy_case(orc, length, ALL_PAIRS)
    if length == 65537:  # spare slots: fewer rows than a slot has tiles, so a row strides them
        copy_case(orc, length, ALL_PAIRS[::17], max_chunks=1024)


def test_stored_copy_tiled(orc):
    """A chunk of 1 MiB + 1: 65 tiles over as many workgroups, every source and every destination
    alignment once; and alone, so that one slot is the whole grid."""
    copy_case(orc, 1048577, [(s, (5 * s + 3) % 16) for s in range(16)])
    copy_case(orc, 1048577, [(13, 6)])


# ---- mixed streams ----------------------------------------------------------------------------------

BAD_COPY = b"\x0a\x04ab\x11\x00"  # 10 bytes declared, the literal "ab", then a copy with offset 0


@functools.lru_cache(maxsize=None)
def alternating(seed, corrupt=None):
    """(stream, the chunks' contents): 100 chunks of 1..300 bytes, compressed and stored in turn
    (chunk 0 compressed); `corrupt` names a compressed chunk whose payload becomes BAD_COPY."""
    O = _oracle()
    rng = np.random.default_rng(seed)
    text = read_testfile("alice29.txt")
    parts, stream = [], bytearray()
    for k in range(100):
        n = int(rng.integers(1, 301))
        at = int(rng.integers(0, len(text) - 300))
        part = text[at:at + n]
        parts.append(part)
        if k % 2:
            stream += R.stored(part)
        else:
            stream += R.compressed(BAD_COPY if k == corrupt else O.compress(part))
    return bytes(stream), parts


def test_mixed_streams(orc):
    B = R.CASE_BLOCK
    good, parts = alternating(1)
    bad, bad_parts = alternating(2, corrupt=36)  # its 37th chunk
    cases = R.structural_cases()
    streams = [good, bad] + [c[1] for c in cases] + [alternating(3)[0], R.encode(b"tail", B, _oracle().compress)]
    caps = [R.walk(s, B)[2] for s in streams]
    models = models_of(B, streams, caps)
    # the reference's own expectations, before the device is asked
    assert models[0].status == 0 and models[0].pieces == parts and models[0].slots == 100
    assert models[1].status == R.SM_ERR_COPY_OFFSET and models[1].chunk_status == [0] * 36 + [R.SM_ERR_COPY_OFFSET] + [0] * 63
    assert [p for k, p in enumerate(models[1].pieces) if k != 36] == [p for k, p in enumerate(bad_parts) if k != 36]
    assert [m.status for m, c in zip(models[2:], cases) if c[2]] == [c[2] for c in cases if c[2]]
    total = sum(m.slots for m in models)
    res = run_decode(orc, B, streams, caps, total)
    check_decode(B, streams, caps, models, res, total)
    # statuses and lengths of the streams that are not decoded are the host plan's, and so is the scan
    rc, first, out_len, status, chunks, frags = orc.streams_plan(streams, B, out_cap=caps)
    assert (rc, chunks, first.tolist()) == (0, total, res["first"])
    undecoded = [s for s, m in enumerate(models) if m.slots == 0 and m.status]
    assert [res["status"][s] for s in undecoded] == [int(status[s]) for s in undecoded] and len(undecoded) >= 15
    assert res["length"] == out_len.tolist()
    again = run_decode(orc, B, streams, caps, total + 5, max_fragments=frags, with_chunks=False)  # spare slots, an index
    check_decode(B, streams, caps, models, again, total + 5)
    assert (again["out"] == res["out"]).all()
    # one slot too few: nothing is decoded, copied or written
    res = run_decode(orc, B, streams, caps, total - 1)
    k = len(streams)
    assert res["status"] == [ARG] * k and res["length"] == [0] * k and (res["out"] == GUARD).all()
    assert res["chunk_status"] == [0] * (total - 1) and res["first"][-1] == total
    # a byte of room too few: that stream alone, with the size it needs
    short = list(caps)
    short[0] -= 1
    models_short = models_of(B, streams, short)
    assert models_short[0].status == R.SM_BUFFER_TOO_SMALL and models_short[0].length == caps[0]
    res = run_decode(orc, B, streams, short, total)
    check_decode(B, streams, short, models_short, res, total)
    assert res["status"][0] == R.SM_BUFFER_TOO_SMALL and res["length"][0] == caps[0] and res["status"][1:] == [m.status for m in models[1:]]
    # the Python call: the corrupt stream is named, or handed out as None
    with pytest.raises(orc.OrcError) as e:
        orc.uncompress_orc_streams([good, bad], B)
    assert (e.value.code, e.value.stream) == (R.SM_ERR_COPY_OFFSET, 1)
    out, st = orc.uncompress_orc_streams([good, bad, b"\x07"], B, statuses=True)
    assert st == [0, R.SM_ERR_COPY_OFFSET, R.TRUNCATED] and out == [b"".join(parts), None, None]


def test_many_chunks_in_one_stream(orc):
    """17,001 one-byte chunks, stored and compressed in turn: more slots than the copy's grid holds
    workgroups, and the scan's tile edges; beside empty streams."""
    content_ = bytes((7 * i + i // 256) & 0xFF for i in range(17001))
    body = b"".join(R.stored(content_[i:i + 1]) if i % 2 else R.compressed(R.lit(content_[i:i + 1])) for i in range(17001))
    streams, caps = [b"", body, b"", R.stored(b"tail")], [0, 17001, 0, 4]
    models = models_of(4, streams, caps)
    assert [m.slots for m in models] == [0, 17001, 0, 1] and b"".join(models[1].pieces) == content_
    for slots in (17002, 17100):
        res = run_decode(orc, 4, streams, caps, slots)
        check_decode(4, streams, caps, models, res, slots)


# ---- the tensor wrappers ----------------------------------------------------------------------------

def test_wrappers_on_a_side_stream_and_scratch_growth(orc):
    """compress and decode through the tensor wrappers on a non-default torch stream, twice on one
    ctx of its own: the second call's shape is larger, so the ctx's scratch grows between them."""
    torch = _torch()
    side = torch.cuda.Stream(device=_dev())
    ctx = ("wrappers", 0, 0)  # a further context of device 0
    for block_size, datas, slots in ((1000, [content("html", 2500), content("random", 999), b""], 5),
                                     (65537, [content("html", 300000), content("random", 70000), content("zeros", 5)] * 3, 400)):
        want = [R.encode(d, block_size, _oracle().compress) for d in datas]
        d_in, in_off, in_len = lay(datas, lead=7, gap=3)
        offs, pos = [], 5
        for d in datas:
            offs.append(pos)
            pos += R.max_length(len(d), block_size) + 16
        k = len(datas)
        d_out = torch.full((pos,), GUARD, dtype=torch.uint8, device=_dev())
        d_ol = torch.full((k,), -1, dtype=torch.int64, device=_dev())
        d_st = torch.full((k,), 77, dtype=torch.int32, device=_dev())
        d_back = torch.full((sum(len(d) + 16 for d in datas) + 16,), GUARD, dtype=torch.uint8, device=_dev())
        back_off = list(np.cumsum([16] + [len(d) + 16 for d in datas[:-1]]))
        d_bl = torch.full((k,), -1, dtype=torch.int64, device=_dev())
        d_bs = torch.full((k,), 77, dtype=torch.int32, device=_dev())
        args = [_i64(in_off), _i64(in_len), _i64(offs), _i64(back_off), _i64([len(d) for d in datas])]
        torch.cuda.synchronize()  # (the inputs were made on the default stream)
        orc.compress_orc_streams_device(block_size, d_in, args[0], args[1], slots, d_out, args[2], d_ol, d_st, mode="reference",
                                        stream=side, device=ctx)
        # the encoder's output is the decoder's input on the same stream: no synchronisation between
        orc.uncompress_orc_streams_device(block_size, d_out, args[2], d_ol, slots, 4 * slots, d_back, args[3], args[4], d_bl,
                                          d_bs, stream=side, device=ctx)
        side.synchronize()
        assert d_st.cpu().tolist() == [0] * k and d_ol.cpu().tolist() == [len(w) for w in want]
        out = d_out.cpu().numpy()
        assert [out[o:o + len(w)].tobytes() for o, w in zip(offs, want)] == want
        assert d_bs.cpu().tolist() == [0] * k and d_bl.cpu().tolist() == [len(d) for d in datas]
        back = d_back.cpu().numpy()
        assert [back[o:o + len(d)].tobytes() for o, d in zip(back_off, datas)] == datas
        outside = np.ones(back.size, bool)
        for o, d in zip(back_off, datas):
            outside[o:o + len(d)] = False
        assert (back[outside] == GUARD).all()
    assert orc._ctx[ctx] != orc.context(0)
