"""The three decode entry points of the framing library run one slot stage (csrc/framing/
smf_slots.h): smf_uncompress_chunks_device, smf_uncompress_streams_device and
smf_uncompress_ranges_device give the same per-chunk verdicts for the same chunks, the first
failing slot decides a group's status in either order, the scan of the groups' slot counts is right
across a scan tile, and one slot short fails every group without a byte written.  Expected values
come from tests/framing_ref.py and the CPU oracle, never from the library."""
import functools
import importlib

import numpy as np
import pytest

import framing_ref as R
import framing_streams_ref as SR
from conftest import load_package, read_testfile

pytestmark = pytest.mark.gpu

GUARD = 0xA5
ARG = SR.SM_ERR_ARGUMENT
PIECE = 100


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


def _full(n, value, dtype):
    return _torch().full((max(n, 1),), value, dtype=dtype, device=_dev())


def _bytes(buf):
    return _torch().from_numpy(np.frombuffer(bytes(buf), np.uint8).copy()).to(_dev())


def _oracle():
    import oracle as O
    O.lib()
    return O


def _upload_index(arrays):
    """A host index (numpy, unsigned) as the device arrays the C ABI takes, bit for bit."""
    signed = {"type": np.uint8, "pay_off": np.int64, "pay_len": np.int32, "crc": np.int32, "ulen": np.int32}
    return {k: _torch().from_numpy(np.ascontiguousarray(arrays[k]).view(signed[k]).copy()).to(_dev()) for k in signed}


# ---- test 1: six chunks, three ways ------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def pieces():
    t = read_testfile("alice29.txt")
    return [t[1000 + PIECE * k:1000 + PIECE * (k + 1)] for k in range(6)]


def wrong(field):
    return bytes([field[0] ^ 0x40]) + field[1:]


@functools.lru_cache(maxsize=None)
def rejected_payload():
    """A raw stream the decoder rejects behind a good header: it declares PIECE bytes, then copies
    from before the start of the output.  The oracle names the status."""
    payload = bytes([PIECE]) + b"\x01\x05" + b"\x00" * 8  # copy, 1-byte offset form: 4 bytes from 5 back
    st, _ = _oracle().uncompress_status(payload)
    assert st not in (R.SM_OK, R.CRC)
    return payload, st


def make_chunk(kind, data):
    O = _oracle()
    if kind == "good00":
        return R.compressed_chunk(data, O)
    if kind == "good01":
        return R.raw_chunk(data)
    if kind == "crc00":
        return R.chunk(0x00, wrong(R.crc_field(data)) + O.compress(data))
    if kind == "crc01":
        return R.chunk(0x01, wrong(R.crc_field(data)) + data)
    assert kind == "bad00"  # the decoder rejects it, and its CRC is wrong as well
    return R.chunk(0x00, wrong(R.crc_field(data)) + rejected_payload()[0])


def want_status(kind):
    return {"good00": R.SM_OK, "good01": R.SM_OK, "crc00": R.CRC, "crc01": R.CRC, "bad00": rejected_payload()[1]}[kind]


# chunk 1..6 of the issue are entries 0..5
SCENARIOS = {
    "all": ("good00", "good01", "crc00", "crc01", "bad00", "good00"),
    "only_3": ("good00", "good01", "crc00", "good01", "good00", "good00"),
    "only_5": ("good00", "good01", "good00", "good01", "bad00", "good00"),
    "swapped": ("good00", "good01", "bad00", "crc01", "crc00", "good00"),
}


@functools.lru_cache(maxsize=None)
def scenario(name):
    """(stream, the per-chunk statuses, the stream's status) of a scenario.  The statuses are the
    table above, checked against the reference decoder's rule chunk by chunk."""
    kinds = SCENARIOS[name]
    stream = R.IDENTIFIER + b"".join(make_chunk(k, d) for k, d in zip(kinds, pieces()))
    want = [want_status(k) for k in kinds]
    O = _oracle()
    model = []
    for ctype, off, plen, stored, declared in R.walk(stream):
        assert declared == PIECE
        payload = stream[off:off + plen]
        st, data = O.uncompress_status(payload) if ctype == 0 else (0, payload)
        model.append(st if st else (R.CRC if R.mask(R.crc32c(data)) != stored else R.SM_OK))
    assert model == want
    first = next((s for s in want if s), R.SM_OK)
    try:
        R.decode(stream, O)
        assert first == R.SM_OK
    except R.FramingRefError as e:
        assert e.code == first
    return stream, want, first


def check_good_bytes(out, offs, want):
    for k, (o, st) in enumerate(zip(offs, want)):
        if st == R.SM_OK:
            assert out[o:o + PIECE].tobytes() == pieces()[k], k


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_chunks_path(fr, name):
    torch = _torch()
    stream, want, first = scenario(name)
    summary, arrays = fr.index_framed(stream)
    assert summary.status == 0 and summary.nchunks == 6 and summary.total_length == 6 * PIECE
    d_out = _full(6 * PIECE + 32, GUARD, torch.uint8)
    d_cs, d_len, d_st = _full(6, 77, torch.int32), _full(1, -1, torch.int64), _full(1, 77, torch.int32)
    fr.uncompress_chunks_device(_bytes(stream), _upload_index(arrays), 6, d_out[16:16 + 6 * PIECE], d_cs, d_len, d_st)
    torch.cuda.synchronize()
    assert d_cs.cpu().tolist() == want
    assert int(d_st.item()) == first and int(d_len.item()) == 6 * PIECE
    out = d_out.cpu().numpy()
    check_good_bytes(out, [16 + PIECE * k for k in range(6)], want)
    assert (out[:16] == GUARD).all() and (out[16 + 6 * PIECE:] == GUARD).all()


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_streams_path(fr, name):
    torch = _torch()
    stream, want, first = scenario(name)
    d_out = _full(6 * PIECE + 32, GUARD, torch.uint8)
    d_ol, d_st = _full(1, -1, torch.int64), _full(1, 77, torch.int32)
    d_cf, d_cs = _full(2, -1, torch.int32), _full(6, 77, torch.int32)
    fr.uncompress_framed_streams_device(_bytes(stream), _i64([0]), _i64([len(stream)]), 6, d_out, _i64([16]),
                                        _i64([6 * PIECE]), d_ol, d_st, d_cf, d_cs)
    torch.cuda.synchronize()
    assert d_cs.cpu().tolist() == want and d_cf.cpu().tolist() == [0, 6]
    assert d_st.cpu().tolist() == [first] and d_ol.cpu().tolist() == [6 * PIECE]
    out = d_out.cpu().numpy()
    check_good_bytes(out, [16 + PIECE * k for k in range(6)], want)
    assert (out[:16] == GUARD).all() and (out[16 + 6 * PIECE:] == GUARD).all()


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_ranges_path(fr, name):
    torch = _torch()
    stream, want, first = scenario(name)
    summary, arrays = fr.index_framed(stream)
    d_arrays, d_in = _upload_index(arrays), _bytes(stream)
    d_coff = _i64(fr.chunk_offsets(arrays["ulen"]).tolist())
    # one range per chunk, at odd places of the output
    offs = [16 + (PIECE + 7) * r for r in range(6)]
    d_out = _full(offs[-1] + PIECE + 16, GUARD, torch.uint8)
    d_ol, d_rs = _full(6, -1, torch.int64), _full(6, 77, torch.int32)
    fr.uncompress_ranges_device(d_in, d_arrays, d_coff, 6, _i64([PIECE * r for r in range(6)]), _i64([PIECE] * 6), 6, d_out,
                                _i64(offs), d_ol, d_rs)
    torch.cuda.synchronize()
    assert d_rs.cpu().tolist() == want
    assert d_ol.cpu().tolist() == [PIECE if st == R.SM_OK else 0 for st in want]
    out = d_out.cpu().numpy()
    check_good_bytes(out, offs, want)
    for r in range(6):  # between the ranges nothing is written
        assert (out[offs[r] + PIECE:offs[r] + PIECE + 7] == GUARD).all(), r
    assert (out[:16] == GUARD).all()
    # one range over the whole content: the first failing chunk's status
    d_all = _full(6 * PIECE + 32, GUARD, torch.uint8)
    d_ol, d_rs = _full(1, -1, torch.int64), _full(1, 77, torch.int32)
    fr.uncompress_ranges_device(d_in, d_arrays, d_coff, 6, _i64([0]), _i64([6 * PIECE]), 6, d_all, _i64([16]), d_ol, d_rs)
    torch.cuda.synchronize()
    assert d_rs.cpu().tolist() == [first] and d_ol.cpu().tolist() == [0 if first else 6 * PIECE]
    out = d_all.cpu().numpy()
    check_good_bytes(out, [16 + PIECE * k for k in range(6)], want)
    assert (out[:16] == GUARD).all() and (out[16 + 6 * PIECE:] == GUARD).all()


# ---- tests 2 and 3: 258 groups, empty ones at both ends and on both sides of the scan's tile -------------

GROUPS = 258
EMPTY = (0, 255, 256, 257)
SMALL = 16


@functools.lru_cache(maxsize=None)
def small_inputs():
    t = read_testfile("alice29.txt")
    return [b"" if g in EMPTY else t[5000 + SMALL * g:5000 + SMALL * (g + 1)] for g in range(GROUPS)]


def want_first():
    out, at = [], 0
    for d in small_inputs():
        out.append(at)
        at += 1 if d else 0
    return out + [at]


def decode_streams(fr, max_chunks):
    torch = _torch()
    streams = [R.IDENTIFIER + (R.raw_chunk(d) if d else b"") for d in small_inputs()]
    in_off = np.concatenate([[0], np.cumsum([len(s) for s in streams])]).tolist()
    offs = [16 + (SMALL + 5) * g for g in range(GROUPS)]
    d_out = _full(offs[-1] + SMALL + 16, GUARD, torch.uint8)
    d_ol, d_st = _full(GROUPS, -1, torch.int64), _full(GROUPS, 77, torch.int32)
    d_cf, d_cs = _full(GROUPS + 1, -1, torch.int32), _full(max_chunks, 77, torch.int32)
    fr.uncompress_framed_streams_device(_bytes(b"".join(streams)), _i64(in_off[:-1]), _i64([len(s) for s in streams]),
                                        max_chunks, d_out, _i64(offs), _i64([len(d) for d in small_inputs()]), d_ol, d_st,
                                        d_cf, d_cs)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), offs, d_ol.cpu().tolist(), d_st.cpu().tolist(), d_cf.cpu().tolist(), d_cs.cpu().tolist()


def decode_ranges(fr, max_range_chunks):
    torch = _torch()
    data = [d for d in small_inputs() if d]
    stream = R.IDENTIFIER + b"".join(R.raw_chunk(d) for d in data)
    summary, arrays = fr.index_framed(stream)
    assert summary.status == 0 and summary.nchunks == GROUPS - len(EMPTY)
    first = want_first()
    lo = [SMALL * first[g] for g in range(GROUPS)]
    ln = [len(d) for d in small_inputs()]
    offs = [16 + (SMALL + 5) * g for g in range(GROUPS)]
    d_out = _full(offs[-1] + SMALL + 16, GUARD, torch.uint8)
    d_ol, d_rs = _full(GROUPS, -1, torch.int64), _full(GROUPS, 77, torch.int32)
    fr.uncompress_ranges_device(_bytes(stream), _upload_index(arrays), _i64(fr.chunk_offsets(arrays["ulen"]).tolist()),
                                summary.nchunks, _i64(lo), _i64(ln), max_range_chunks, d_out, _i64(offs), d_ol, d_rs)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), offs, d_ol.cpu().tolist(), d_rs.cpu().tolist()


def check_small_outputs(out, offs):
    expected = np.full(out.size, GUARD, np.uint8)
    for o, d in zip(offs, small_inputs()):
        expected[o:o + len(d)] = np.frombuffer(d, np.uint8)
    assert (out == expected).all()


def test_group_scan_across_a_tile_streams(fr):
    out, offs, length, status, first, chunk_status = decode_streams(fr, GROUPS - len(EMPTY))
    assert status == [0] * GROUPS and length == [len(d) for d in small_inputs()]
    assert first == want_first() and [first[g] for g in EMPTY] == [0, 254, 254, 254] and first[GROUPS] == 254
    assert chunk_status == [0] * (GROUPS - len(EMPTY))
    check_small_outputs(out, offs)


def test_group_scan_across_a_tile_ranges(fr):
    out, offs, length, status = decode_ranges(fr, GROUPS - len(EMPTY))
    assert status == [0] * GROUPS and length == [len(d) for d in small_inputs()]
    check_small_outputs(out, offs)


def test_group_scan_across_a_tile_compress(fr):
    torch = _torch()
    inputs = small_inputs()
    in_off = np.concatenate([[0], np.cumsum([len(d) for d in inputs])]).tolist()
    d_in = _bytes(b"".join(inputs))
    room = (R.max_framed_length(SMALL) + 15) // 16 * 16
    d_out = _full(GROUPS * room, GUARD, torch.uint8)
    d_ol, d_st = _full(GROUPS, -1, torch.int64), _full(GROUPS, 77, torch.int32)
    fr.compress_framed_streams_device(d_in, _i64(in_off[:-1]), _i64([len(d) for d in inputs]), GROUPS - len(EMPTY), d_out,
                                      _i64([room * g for g in range(GROUPS)]), d_ol, d_st, mode="fast")
    # the single-stream call, input by input
    d_one = _full(GROUPS * room, GUARD, torch.uint8)
    d_ol1, d_st1 = _full(GROUPS, -1, torch.int64), _full(GROUPS, 77, torch.int32)
    for g, d in enumerate(inputs):
        fr.compress_framed_device(d_in[in_off[g]:in_off[g + 1]], d_one[room * g:room * (g + 1)], d_ol1[g:g + 1], d_st1[g:g + 1],
                                  mode="fast")
    torch.cuda.synchronize()
    assert d_st.cpu().tolist() == [0] * GROUPS and d_st1.cpu().tolist() == [0] * GROUPS
    assert d_ol.cpu().tolist() == d_ol1.cpu().tolist()
    assert bool(torch.equal(d_out, d_one))
    # and the streams are the inputs', by the reference decoder
    out, length = d_out.cpu().numpy(), d_ol.cpu().tolist()
    for g in (0, 1, 254, 255, 256, 257):
        assert R.decode(out[room * g:room * g + length[g]].tobytes(), _oracle()) == inputs[g], g


def test_bound_exceeded_by_one(fr):
    m = GROUPS - len(EMPTY) - 1
    out, offs, length, status, first, chunk_status = decode_streams(fr, m)
    assert status == [ARG] * GROUPS and length == [0] * GROUPS and (out == GUARD).all()
    out, offs, length, status = decode_ranges(fr, m)
    assert status == [ARG] * GROUPS and length == [0] * GROUPS and (out == GUARD).all()
