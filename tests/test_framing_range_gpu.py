"""The framing library's seek index and ranged decode on the GPU (snappy.jl_amd/framing.py over
libsnappy_mi355x_framing.so): the encoder's own index, batched ranges with direct and edge chunks,
the trim copy at every alignment, foreign streams, local corruption, hostile indexes, the chunk
bound, and the host-buffer and Python calls.  Every expected value comes from the plain-Python
references (tests/framing_ref.py, tests/framing_range_ref.py) and the CPU oracle."""
import ctypes
import functools
import importlib

import numpy as np
import pytest

import framing_range_ref as RR
import framing_ref as R
from conftest import load_package, read_testfile

pytestmark = pytest.mark.gpu

BLOCK = 65536
GUARD = 0xA5
ARG = RR.SM_ERR_ARGUMENT
KEYS = ("type", "pay_off", "pay_len", "crc", "ulen")
SIGNED = {"type": np.uint8, "pay_off": np.int64, "pay_len": np.int32, "crc": np.int32, "ulen": np.int32}
UNSIGNED = {"type": np.uint8, "pay_off": np.uint64, "pay_len": np.uint32, "crc": np.uint32, "ulen": np.uint32}


@pytest.fixture(scope="module")
def fr(gpu_available):
    load_package()
    return importlib.import_module("snappy_jl_amd.framing")


def _torch():
    import torch
    return torch


def _dev():
    return _torch().device("cuda", 0)


def _u8(data):
    return _torch().from_numpy(np.frombuffer(bytes(data), np.uint8).copy()).to(_dev())


def _i64(values):
    return _torch().from_numpy(np.array(values, dtype=np.uint64).view(np.int64)).to(_dev())


@functools.lru_cache(maxsize=None)
def blocks(n):
    """n bytes of alternating text and random 64 KiB blocks: both chunk types occur."""
    text = read_testfile("alice29.txt")
    rnd = np.random.default_rng(17).integers(0, 256, 2 * BLOCK, dtype=np.uint8).tobytes()
    parts = [text[:BLOCK], rnd[:BLOCK], text[BLOCK:2 * BLOCK], rnd[BLOCK:]]
    return b"".join(parts[i % 4] for i in range(-(-n // BLOCK)))[:n]


@functools.lru_cache(maxsize=None)
def five_chunks():
    """text, random, text, random, 5 bytes; framed by the Python encoder (fixture `oracle`'s module)."""
    import oracle as O
    O.lib()
    data = blocks(4 * BLOCK) + b"tail!"
    stream = R.encode(data, O)
    assert [c[0] for c in R.walk(stream)] == [0, 1, 0, 1, 1]
    return stream, data


def ref_index(fr, stream):
    """The stream's seek index from the Python walker alone."""
    chunks = R.walk(stream)
    arrays = {k: np.array([c[i] for c in chunks], dtype=UNSIGNED[k]) for i, k in enumerate(KEYS)}
    return fr.FramedIndex(arrays, np.array(RR.chunk_offsets(chunks), dtype=np.uint64))


def to_device(index):
    arrays = {k: _torch().from_numpy(getattr(index, k).view(SIGNED[k]).copy()).to(_dev()) for k in KEYS}
    return arrays, _torch().from_numpy(index.chunk_off.view(np.int64).copy()).to(_dev())


def run_ranges(fr, stream, index, ranges, max_range_chunks, out_mis=None):
    """One smf_uncompress_ranges_device call: every range's output sits in a guard-filled buffer with
    at least 16 guard bytes on both sides, at an address that is out_mis[i] mod 16.  Returns
    (statuses, lengths, the buffer, the outputs' offsets)."""
    torch = _torch()
    offs, pos = [], 32
    for i, (lo, n) in enumerate(ranges):
        pos = (pos + 15) // 16 * 16 + (out_mis[i] if out_mis else 0)
        offs.append(pos)
        pos += min(n, 1 << 20) + 16
    d_out = torch.full((pos + 32,), GUARD, dtype=torch.uint8, device=_dev())
    assert d_out.data_ptr() % 16 == 0
    arrays, d_off = to_device(index)
    d_ol = torch.full((len(ranges),), -1, dtype=torch.int64, device=_dev())
    d_st = torch.full((len(ranges),), 77, dtype=torch.int32, device=_dev())
    fr.uncompress_ranges_device(_u8(stream), arrays, d_off, index.nchunks, _i64([r[0] for r in ranges]),
                                _i64([r[1] for r in ranges]), max_range_chunks, d_out, _i64(offs), d_ol, d_st,
                                n=len(stream))
    torch.cuda.synchronize()
    return d_st.cpu().tolist(), d_ol.cpu().tolist(), d_out.cpu().numpy(), offs


def check_ranges(ranges, want, st, lens, out, offs, total):
    """Statuses, lengths and bytes against `want` = [(status, bytes)]; every byte outside the
    outputs of the ranges that lie inside the `total` content bytes is still the guard's (a range
    that leaves the stream writes nothing at all)."""
    outside = np.ones(out.size, bool)
    wrong = []
    for i, ((lo, n), (wst, wbytes)) in enumerate(zip(ranges, want)):
        ok = st[i] == wst and lens[i] == (n if wst == 0 else 0)
        if wst == 0:
            ok = ok and out[offs[i]:offs[i] + n].tobytes() == wbytes
        if lo + n <= total:
            outside[offs[i]:offs[i] + n] = False
        if not ok:
            wrong.append(((lo, n), st[i], lens[i], wst))
    assert not wrong, wrong[:8]
    assert (out[outside] == GUARD).all()


def total_slots(index, ranges):
    offsets = index.chunk_off.tolist()
    return sum(RR.plan(offsets, lo, n)[1] for lo, n in ranges)


# ---- the encoder's index --------------------------------------------------------------------------

def compress_indexed(fr, data, max_chunks=None, mode="fast"):
    torch = _torch()
    n = len(data)
    nblk = -(-n // BLOCK)
    mc = nblk if max_chunks is None else max_chunks
    d_out = torch.full((R.max_framed_length(n),), GUARD, dtype=torch.uint8, device=_dev())
    d_len = torch.full((1,), -1, dtype=torch.int64, device=_dev())
    d_st = torch.full((1,), 77, dtype=torch.int32, device=_dev())
    arrays = fr.device_chunks(mc)
    d_off = torch.full((mc + 1,), -1, dtype=torch.int64, device=_dev())
    d_nc = torch.full((1,), -1, dtype=torch.int32, device=_dev())
    fr.compress_framed_indexed_device(_u8(data), d_out, d_len, d_st, arrays, d_off, d_nc, mode=mode)
    return d_out, d_len, d_st, arrays, d_off, d_nc


@pytest.mark.parametrize("n", [0, 1, 65535, 65536, 65537, 3 * 65536 + 5])
def test_encoder_index(fr, n):
    torch = _torch()
    data = blocks(n)
    nblk = -(-n // BLOCK)
    d_plain = torch.full((R.max_framed_length(n),), GUARD, dtype=torch.uint8, device=_dev())
    d_len0 = torch.full((1,), -1, dtype=torch.int64, device=_dev())
    d_st0 = torch.full((1,), 77, dtype=torch.int32, device=_dev())
    fr.compress_framed_device(_u8(data), d_plain, d_len0, d_st0)
    d_out, d_len, d_st, arrays, d_off, d_nc = compress_indexed(fr, data)
    torch.cuda.synchronize()
    assert (int(d_st.item()), int(d_len.item()), int(d_nc.item())) == (0, int(d_len0.item()), nblk)
    assert torch.equal(d_out, d_plain)  # the framed bytes, and the guard behind them
    framed = d_out.cpu().numpy().tobytes()[:int(d_len.item())]
    if n >= 2 * BLOCK:
        assert {c[0] for c in R.walk(framed)} == {0, 1}
    # the walker's index of those bytes, completed by the scan
    walked = fr.device_chunks(nblk)
    d_sum = torch.zeros(16, dtype=torch.uint8, device=_dev())
    d_off2 = torch.full((nblk + 1,), -1, dtype=torch.int64, device=_dev())
    fr.index_framed_device(d_out, walked, d_sum, n=len(framed))
    fr.chunk_offsets_device(walked["ulen"], nblk, d_off2)
    s = fr.read_summary(d_sum)
    assert (s.status, s.nchunks, s.total_length) == (0, nblk, n)
    ref = R.walk(framed)
    for i, k in enumerate(KEYS):
        got = arrays[k][:nblk].cpu().numpy().view(UNSIGNED[k]).tolist()
        assert got == walked[k][:nblk].cpu().numpy().view(UNSIGNED[k]).tolist() == [c[i] for c in ref], k
    assert d_off.cpu().tolist() == d_off2.cpu().tolist() == RR.chunk_offsets(ref)
    assert d_off.cpu().tolist() == [min(BLOCK * b, n) for b in range(nblk + 1)]


def test_encoder_index_max_chunks_too_small(fr):
    with pytest.raises(fr.SnappyError) as e:
        compress_indexed(fr, blocks(BLOCK + 1), max_chunks=1)
    assert e.value.code == R.SM_BUFFER_TOO_SMALL
    torch = _torch()
    data = blocks(BLOCK + 1)
    d_out = torch.full((R.max_framed_length(len(data)),), GUARD, dtype=torch.uint8, device=_dev())
    d_len = torch.full((1,), -1, dtype=torch.int64, device=_dev())
    d_st = torch.full((1,), 77, dtype=torch.int32, device=_dev())
    arrays, d_off = fr.device_chunks(1), torch.zeros(2, dtype=torch.int64, device=_dev())
    d_nc = torch.full((1,), -1, dtype=torch.int32, device=_dev())
    with pytest.raises(fr.SnappyError):
        fr.compress_framed_indexed_device(_u8(data), d_out, d_len, d_st, arrays, d_off, d_nc)
    torch.cuda.synchronize()
    assert bool((d_out == GUARD).all()) and int(d_len.item()) == -1 and int(d_nc.item()) == -1  # nothing was launched


def test_round_trip_without_a_walk(fr):
    torch = _torch()
    data = blocks(3 * BLOCK + 5)
    d_out, d_len, d_st, arrays, d_off, d_nc = compress_indexed(fr, data)
    nblk = 4  # (known from the input's length: no result is read back before the decode)
    d_back = torch.zeros(len(data), dtype=torch.uint8, device=_dev())
    d_cs = torch.full((nblk,), 77, dtype=torch.int32, device=_dev())
    d_len2 = torch.full((1,), -1, dtype=torch.int64, device=_dev())
    d_st2 = torch.full((1,), 77, dtype=torch.int32, device=_dev())
    fr.uncompress_chunks_device(d_out, arrays, nblk, d_back, d_cs, d_len2, d_st2)
    torch.cuda.synchronize()
    assert (int(d_st2.item()), int(d_len2.item()), d_cs.cpu().tolist()) == (0, len(data), [0] * nblk)
    assert d_back.cpu().numpy().tobytes() == data


# ---- ranges ---------------------------------------------------------------------------------------

EDGE_RANGES = [(65535, 2), (65536, 1), (65535, 65538), (70000, 300)]


def test_ranges_of_a_five_chunk_stream(fr, oracle):
    stream, data = five_chunks()
    total = len(data)
    index = ref_index(fr, stream)
    whole_chunks = [(BLOCK * c, min(BLOCK, total - BLOCK * c)) for c in range(5)]
    ranges = [(0, total)] + whole_chunks + EDGE_RANGES + [(total, 0), (0, 0), (total - 1, 2)]
    want = [RR.read_range(stream, lo, n, oracle) for lo, n in ranges]
    assert want[0] == (0, data) and want[-1] == (ARG, b"") and want[8] == (0, data[65535:65535 + 65538])
    st, lens, out, offs = run_ranges(fr, stream, index, ranges, total_slots(index, ranges))
    check_ranges(ranges, want, st, lens, out, offs, total)
    # the whole stream and the whole chunks need no edge slot: the count of slots says which
    # chunks a range has, the guard bytes around each output that nothing else was written
    assert total_slots(index, ranges) == 5 + 5 + 2 + 1 + 3 + 1


def test_trim_copy_alignment_sweep(fr, oracle):
    """lo mod 16 x the output's address mod 16 x lengths around a granule, at both kinds of chunk
    boundary (0x00 | 0x01 at 65536, 0x01 | 0x00 at 131072): ranges that end before, at, and behind
    the boundary, each trimmed out of one or two edge slots."""
    stream, data = five_chunks()
    index = ref_index(fr, stream)
    for boundary in (BLOCK, 2 * BLOCK):
        ranges, mis = [], []
        for a in range(16):
            for o in range(16):
                for n in (1, 15, 16, 17, 40):
                    ranges.append((boundary - 16 + a, n))
                    mis.append(o)
        assert sum(lo + n > boundary for lo, n in ranges) > len(ranges) // 2  # most of them straddle it
        want = [RR.read_range(stream, lo, n, oracle) for lo, n in ranges]
        assert all(w == (0, data[lo:lo + n]) for w, (lo, n) in zip(want, ranges))
        st, lens, out, offs = run_ranges(fr, stream, index, ranges, total_slots(index, ranges), out_mis=mis)
        check_ranges(ranges, want, st, lens, out, offs, len(data))


def device_index(fr, stream, max_chunks=16):
    """The stream's index by the device walker and the offsets kernel, back on the host."""
    torch = _torch()
    arrays = fr.device_chunks(max_chunks)
    d_sum = torch.zeros(16, dtype=torch.uint8, device=_dev())
    d_off = torch.zeros(max_chunks + 1, dtype=torch.int64, device=_dev())
    fr.index_framed_device(_u8(stream), arrays, d_sum, n=len(stream))
    s = fr.read_summary(d_sum)
    assert s.status == 0 and s.nchunks <= max_chunks
    fr.chunk_offsets_device(arrays["ulen"], s.nchunks, d_off)
    torch.cuda.synchronize()
    return fr.FramedIndex({k: arrays[k][:s.nchunks].cpu().numpy().view(UNSIGNED[k]) for k in KEYS},
                          d_off[:s.nchunks + 1].cpu().numpy().view(np.uint64))


def test_foreign_stream_every_range(fr, oracle):
    stream, data = RR.foreign_stream(oracle)
    index = device_index(fr, stream)
    assert index.chunk_off.tolist() == RR.chunk_offsets(R.walk(stream))
    ranges = RR.all_ranges(len(data))
    want = [RR.read_range(stream, lo, n, oracle) for lo, n in ranges]
    assert all(w == ((0, data[lo:lo + n]) if lo + n <= len(data) else (ARG, b"")) for w, (lo, n) in zip(want, ranges))
    st, lens, out, offs = run_ranges(fr, stream, index, ranges, total_slots(index, ranges))
    check_ranges(ranges, want, st, lens, out, offs, len(data))


def test_structural_cases_full_range(fr, oracle):
    for name, stream, status, nchunks in R.structural_cases():
        if status != R.SM_OK:
            continue
        index = device_index(fr, stream)
        total = index.total_length
        ranges = [(0, total)]
        want = [RR.read_range(stream, 0, total, oracle)]
        try:
            assert want[0] == (0, R.decode(stream, oracle)), name
        except R.FramingRefError as e:
            assert want[0] == (e.code, b""), name
        st, lens, out, offs = run_ranges(fr, stream, index, ranges, max(total_slots(index, ranges), 1))
        check_ranges(ranges, want, st, lens, out, offs, total)


def test_corruption_is_local(fr, oracle):
    stream, data = five_chunks()
    chunks = R.walk(stream)
    total = len(data)
    payload = bytearray(stream)
    payload[chunks[2][1] + 1000] ^= 0x40  # a payload byte of chunk 2 (0x00)
    stored = bytearray(stream)
    stored[chunks[1][1] - 3] ^= 0x01      # a byte of chunk 1's stored CRC (0x01)
    both = bytearray(payload)
    both[chunks[1][1] - 3] ^= 0x01
    ranges = [(0, total), (0, BLOCK), (BLOCK, BLOCK), (2 * BLOCK, BLOCK), (3 * BLOCK, BLOCK + 5), (BLOCK - 1, 2),
              (2 * BLOCK - 1, 2), (3 * BLOCK - 1, 2), (BLOCK + 7, 100), (2 * BLOCK + 7, 100), (BLOCK + 1, 2 * BLOCK),
              (3 * BLOCK, 1), (10, 20)]
    for damaged, bad in ((bytes(payload), {2}), (bytes(stored), {1}), (bytes(both), {1, 2})):
        index = ref_index(fr, damaged)
        want = [RR.read_range(damaged, lo, n, oracle) for lo, n in ranges]
        firsts = {}
        for (lo, n), w in zip(ranges, want):
            hit = sorted(bad & set(RR.touched(index.chunk_off.tolist(), lo, n)))
            assert (w[0] != 0) == bool(hit)
            if hit:
                firsts[hit[0]] = w[0]
            else:
                assert w == (0, data[lo:lo + n])
        assert len(firsts) == len(bad) and firsts.get(1, R.CRC) == R.CRC
        if bad == {1, 2}:
            assert want[0][0] == R.CRC and want[10][0] == R.CRC  # two bad chunks: the first one's status
        st, lens, out, offs = run_ranges(fr, damaged, index, ranges, total_slots(index, ranges))
        check_ranges(ranges, want, st, lens, out, offs, total)


def test_hostile_index(fr, oracle):
    """Every case is rejected by the shared rules before any access (tests/test_framing_range_host.py
    runs the same rules on the CPU, `make host_check` under sanitizers): statuses are the host
    plan's, untouched ranges decode, and nothing is written outside the ranges' outputs."""
    stream, data = RR.foreign_stream(oracle)
    good = ref_index(fr, stream)
    ranges = RR.all_ranges(len(data))
    for name, bad, victim in RR.hostile_indexes(fr.FramedIndex, good, len(stream)):
        rc, first, count, status, total = fr.range_plan(bad, len(stream), ranges)
        assert rc == 0 and total < 4096, name
        want = []
        for (lo, n), pst in zip(ranges, status.tolist()):
            assert pst == RR.hostile_want(good, int(bad.chunk_off[-1]), victim, lo, n), (name, lo, n)
            want.append((0, data[lo:lo + n]) if pst == 0 else (ARG, b""))
        st, lens, out, offs = run_ranges(fr, stream, bad, ranges, int(total))
        check_ranges(ranges, want, st, lens, out, offs, len(data))


def test_chunk_bound_exceeded_by_one(fr, oracle):
    stream, data = five_chunks()
    index = ref_index(fr, stream)
    ranges = [(0, len(data)), (BLOCK, BLOCK)] + EDGE_RANGES + [(0, 0)]
    need = total_slots(index, ranges)
    st, lens, out, offs = run_ranges(fr, stream, index, ranges, need - 1)
    assert st == [ARG] * len(ranges) and lens == [0] * len(ranges)
    assert (out == GUARD).all()
    want = [RR.read_range(stream, lo, n, oracle) for lo, n in ranges]
    st, lens, out, offs = run_ranges(fr, stream, index, ranges, need)
    check_ranges(ranges, want, st, lens, out, offs, len(data))


# ---- the host-buffer call and Python --------------------------------------------------------------

def test_host_buffer_call_and_python(fr, oracle):
    stream, data = five_chunks()
    total = len(data)
    index = fr.seek_index_framed(stream)
    ranges = EDGE_RANGES + [(0, total), (total - 5, 5), (total, 0), (0, 0), (3 * BLOCK, BLOCK + 5)]
    for lo, n in ranges:
        assert fr.uncompress_framed_range(stream, lo, n) == data[lo:lo + n], (lo, n)
    for lo, n in EDGE_RANGES + [(total, 0)]:
        assert fr.uncompress_framed_range(stream, lo, n, index=index) == data[lo:lo + n], (lo, n)
    out, st = fr.uncompress_framed_ranges(stream, ranges + [(total - 1, 2)])
    assert st.tolist() == [0] * len(ranges) + [ARG]
    assert out == [data[lo:lo + n] for lo, n in ranges] + [b""]
    out, st = fr.uncompress_framed_ranges(stream, ranges, index=index)
    assert st.tolist() == [0] * len(ranges) and out == [data[lo:lo + n] for lo, n in ranges]
    for lo, n in ((total - 1, 2), (1 << 63, 1 << 63)):
        with pytest.raises(fr.SnappyError) as e:
            fr.uncompress_framed_range(stream, lo, n)
        assert e.value.code == ARG
    # a structural error behind the range: the walk sees it
    with pytest.raises(fr.SnappyError) as e:
        fr.uncompress_framed_range(stream + R.chunk(0x02, b""), 10, 20)
    assert e.value.code == R.RESERVED_CHUNK
    # a damaged chunk fails the ranges that touch it, and only those
    damaged = bytearray(stream)
    damaged[R.walk(stream)[2][1] + 1000] ^= 0x40
    damaged = bytes(damaged)
    assert fr.uncompress_framed_range(damaged, BLOCK - 10, 20) == data[BLOCK - 10:BLOCK + 10]
    with pytest.raises(fr.SnappyError) as e:
        fr.uncompress_framed_range(damaged, 2 * BLOCK - 1, 2)
    assert e.value.code == RR.read_range(damaged, 2 * BLOCK - 1, 2, oracle)[0] != 0
    # the C call with a short output
    src = np.frombuffer(stream, np.uint8)
    buf = np.full(64, GUARD, np.uint8)
    ol = ctypes.c_size_t(19)
    rc = fr.lib().smf_uncompress_range(fr.context(0), src.ctypes.data, src.size, 65530, 20, buf.ctypes.data, ctypes.byref(ol))
    assert (rc, ol.value) == (R.SM_BUFFER_TOO_SMALL, 20) and (buf == GUARD).all()
    ol = ctypes.c_size_t(64)
    rc = fr.lib().smf_uncompress_range(fr.context(0), src.ctypes.data, src.size, 65530, 20, buf.ctypes.data, ctypes.byref(ol))
    assert (rc, ol.value) == (0, 20) and buf[:20].tobytes() == data[65530:65550] and (buf[20:] == GUARD).all()


def test_compress_framed_returns_the_index(fr, oracle):
    data = blocks(2 * BLOCK + 77)
    framed, index = fr.compress_framed(data, return_index=True)
    assert framed == fr.compress_framed(data) and R.decode(framed, oracle) == data
    walked = fr.seek_index_framed(framed)
    for k in KEYS + ("chunk_off",):
        assert getattr(index, k).tolist() == getattr(walked, k).tolist(), k
    assert fr.uncompress_framed_range(framed, BLOCK - 3, 10, index=index) == data[BLOCK - 3:BLOCK + 7]
