"""The framing format on the GPU (snappy.jl_amd/framing.py over libsnappy_mi355x_framing.so)
against the plain-Python reference of tests/framing_ref.py: the CRC-32C kernel, framed round trips,
foreign streams, the error contract and the device API.  Every expected value comes from the
Python reference or the CPU oracle."""
import ctypes
import functools
import importlib

import numpy as np
import pytest

import framing_ref as R
from conftest import load_package, read_testfile

pytestmark = pytest.mark.gpu

BLOCK = 65536
CRC_LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4097, 65535, 65536)


@pytest.fixture(scope="module")
def fr(gpu_available):
    load_package()
    return importlib.import_module("snappy_jl_amd.framing")


def _torch():
    import torch
    return torch


def _dev():
    return _torch().device("cuda", 0)


def _aligned_u8(host, mis=0):
    """host (uint8 array) on the device in a tensor whose data_ptr() is `mis` mod 16."""
    torch = _torch()
    raw = torch.empty(host.size + 32, dtype=torch.uint8, device=_dev())
    shift = (mis - raw.data_ptr()) % 16
    t = raw[shift:shift + host.size]
    t.copy_(torch.from_numpy(np.array(host, dtype=np.uint8)))
    assert host.size == 0 or t.data_ptr() % 16 == mis
    return t


def _i64(values):
    return _torch().tensor(np.asarray(values, dtype=np.uint64).astype(np.int64), device=_dev())


def _i32(values):
    return _torch().tensor(np.asarray(values, dtype=np.uint32).view(np.int32), device=_dev())


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


@functools.lru_cache(maxsize=None)
def text_block():
    return read_testfile("alice29.txt")[:BLOCK]


@functools.lru_cache(maxsize=None)
def random_bytes(n, seed=1):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def crc_blocks():
    """One random block per length of CRC_LENGTHS and its reference CRC, computed once."""
    blocks = [random_bytes(n, seed=100 + i) for i, n in enumerate(CRC_LENGTHS)]
    return blocks, [R.crc32c(b) for b in blocks]


def gpu_crcs(fr, blocks, mis, masked, exact=False):
    """CRCs of `blocks` laid out behind one another with every block's address `mis` mod 16 (exact:
    back to back from an aligned base, the tensor ending with the last block)."""
    offs, pos = [], 0
    for b in blocks:
        offs.append(pos)
        pos += len(b) if exact else (len(b) + 15) // 16 * 16 + 16
    host = np.zeros(pos if exact else max(pos, 1), np.uint8)
    for o, b in zip(offs, blocks):
        host[o:o + len(b)] = np.frombuffer(b, np.uint8)
    if exact:
        d_in = _torch().from_numpy(host).to(_dev())
        assert d_in.numel() == sum(len(b) for b in blocks)
    else:
        d_in = _aligned_u8(host, mis)
    d_crc = _i32(np.full(len(blocks), 0xDEADBEEF, np.uint32))
    fr.crc32c_batch_device(d_in, _i64(offs), _i32([len(b) for b in blocks]), d_crc, masked=masked)
    _torch().cuda.synchronize()
    return _u32(d_crc).tolist()


# ---- CRC ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("masked", [False, True])
def test_crc_known_answers(fr, masked):
    got = gpu_crcs(fr, [k[0] for k in R.KNOWN_ANSWERS], 0, masked)
    assert got == [k[2] if masked else k[1] for k in R.KNOWN_ANSWERS]


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("mis", [0, 1, 5, 15])
def test_crc_lengths_and_alignments(fr, mis, masked):
    blocks, ref = crc_blocks()
    got = gpu_crcs(fr, blocks, mis, masked)
    want = [R.mask(c) if masked else c for c in ref]
    bad = [(n, hex(g), hex(w)) for n, g, w in zip(CRC_LENGTHS, got, want) if g != w]
    assert not bad, "address %d mod 16: (length, gpu, reference) %s" % (mis, bad)


def test_crc_tensor_ends_with_its_last_block(fr):
    # back to back: the second block starts at 65536 (aligned) and ends with the tensor; the third
    # layout starts its last block at an odd address
    blocks, ref = crc_blocks()
    by_len = dict(zip(CRC_LENGTHS, zip(blocks, ref)))
    for lens in ((65536, 65535), (4097, 65535), (17, 1)):
        got = gpu_crcs(fr, [by_len[n][0] for n in lens], 0, False, exact=True)
        assert got == [by_len[n][1] for n in lens]


def test_crc_more_blocks_than_workgroups(fr):
    # 2,300 blocks: past the launch's 2,048 workgroups, so some take a second block
    data = np.frombuffer(random_bytes(2300 * 48 + 7, seed=3), np.uint8)
    lens = [(7 * i) % 49 for i in range(2300)]
    offs = [48 * i + (i % 7) for i in range(2300)]
    d_crc = _i32(np.zeros(2300, np.uint32))
    fr.crc32c_batch_device(_aligned_u8(data), _i64(offs), _i32(lens), d_crc, masked=True)
    _torch().cuda.synchronize()
    want = [R.mask(R.crc32c(data[o:o + n].tobytes())) for o, n in zip(offs, lens)]
    assert _u32(d_crc).tolist() == want


# ---- round trips ----------------------------------------------------------------------------------

def _inputs():
    text = text_block()
    html = read_testfile("html")
    return {
        "empty": b"", "one_byte": b"a", "65535": text[:65535], "65536": text, "65537": text + b"z",
        "three_blocks_and_one": (text * 3) + b"!", "html": html, "random_70000": random_bytes(70000),
        "text_random_text": text + random_bytes(BLOCK, seed=2) + text[:1000],
    }


@pytest.mark.parametrize("name", list(_inputs()))
def test_round_trip(fr, oracle, name):
    data = _inputs()[name]
    ref_stream = R.encode(data, oracle)
    for mode in ("reference", "fast", "dense"):
        framed = fr.compress_framed(data, mode=mode)
        assert len(framed) <= R.max_framed_length(len(data))
        if mode == "reference":
            assert framed == ref_stream  # byte for byte the Python encoder's stream
        else:
            assert R.decode(framed, oracle) == data
        assert fr.length_uncompressed_framed(framed) == len(data)
        assert fr.uncompress_framed(framed) == data
        assert fr.validate_framed(framed) == 0
    assert fr.uncompress_framed(ref_stream) == data


def test_golden_and_chunk_types(fr):
    assert fr.compress_framed(b"a", mode="reference") == R.GOLDEN_A
    assert fr.compress_framed(b"a", mode="fast") == R.GOLDEN_A
    assert fr.compress_framed(b"") == R.IDENTIFIER
    for mode in ("reference", "fast", "dense"):
        framed = fr.compress_framed(random_bytes(BLOCK) + text_block(), mode=mode)
        chunks = R.walk(framed)
        assert [c[0] for c in chunks] == [1, 0]
        assert framed[10] == 0x01 and int.from_bytes(framed[11:14], "little") == 65540
        assert chunks[1][2] < BLOCK and chunks[1][4] == BLOCK


# ---- foreign streams ------------------------------------------------------------------------------

def _foreign(oracle):
    text, rnd = text_block(), random_bytes(5000, seed=7)
    parts = [text[:30000], rnd, b"", text[30000:], b"x", rnd[:100]]
    stream = (R.IDENTIFIER + R.compressed_chunk(parts[0], oracle) + R.chunk(0xFE, bytes(13)) + R.raw_chunk(parts[1]) +
              R.chunk(0x80, b"skip me") + R.compressed_chunk(parts[2], oracle) + R.IDENTIFIER +
              R.compressed_chunk(parts[3], oracle) + R.chunk(0xFD, b"") + R.raw_chunk(parts[4]) +
              R.compressed_chunk(parts[5], oracle))
    return stream, b"".join(parts)


def test_foreign_stream(fr, oracle):
    stream, data = _foreign(oracle)
    assert R.decode(stream, oracle) == data
    assert fr.uncompress_framed(stream) == data
    assert fr.length_uncompressed_framed(stream) == len(data)


def test_concatenated_streams(fr, oracle):
    a, b = text_block()[:70000 - BLOCK] + random_bytes(BLOCK), _inputs()["html"]
    joined = fr.compress_framed(a, mode="fast") + fr.compress_framed(b, mode="dense")
    assert fr.uncompress_framed(joined) == a + b
    assert fr.uncompress_framed(joined + R.IDENTIFIER) == a + b


# ---- errors ---------------------------------------------------------------------------------------

def decode_chunks(fr, stream, capacity=None):
    """smf_uncompress_chunks_device over the host index of `stream`: (chunk statuses, status,
    length, output bytes)."""
    torch = _torch()
    s, arrays = fr.index_framed(stream)
    assert s.status == 0
    n = s.nchunks
    d = {k: torch.from_numpy(v.view({"uint8": np.uint8, "uint64": np.int64, "uint32": np.int32}[v.dtype.name])).to(_dev())
         for k, v in arrays.items()}
    d_in = _aligned_u8(np.frombuffer(stream, np.uint8))
    cap = s.total_length if capacity is None else capacity
    d_out = torch.zeros(cap, dtype=torch.uint8, device=_dev())  # (every caller's capacity is > 0)
    d_cs = _i32(np.full(max(n, 1), 77, np.uint32))
    d_len = torch.full((1,), -1, dtype=torch.int64, device=_dev())
    d_st = torch.full((1,), 77, dtype=torch.int32, device=_dev())
    fr.uncompress_chunks_device(d_in, d, n, d_out, d_cs, d_len, d_st)
    torch.cuda.synchronize()
    return d_cs.cpu().numpy()[:n].tolist(), int(d_st.item()), int(d_len.item()), d_out.cpu().numpy().tobytes()[:cap]


def _three_chunks(oracle):
    parts = [text_block()[:20000], text_block()[20000:45000], random_bytes(3000, seed=11)]
    chunks = [R.compressed_chunk(parts[0], oracle), R.compressed_chunk(parts[1], oracle), R.raw_chunk(parts[2])]
    return parts, chunks


def test_flipped_crc_bit_fails_that_chunk_only(fr, oracle):
    parts, chunks = _three_chunks(oracle)
    for victim in range(3):
        bad = bytearray(chunks[victim])
        bad[4 + 2] ^= 0x10  # a bit of the stored CRC
        stream = R.IDENTIFIER + b"".join(bytes(bad) if i == victim else c for i, c in enumerate(chunks))
        cs, st, length, out = decode_chunks(fr, stream)
        assert cs == [R.CRC if i == victim else 0 for i in range(3)] and st == R.CRC
        assert length == sum(map(len, parts))
        pos = 0
        for i, p in enumerate(parts):  # the neighbours decoded (and so did the victim: only its CRC field is wrong)
            assert out[pos:pos + len(p)] == p, i
            pos += len(p)
        with pytest.raises(fr.SnappyError) as e:
            fr.uncompress_framed(stream)
        assert e.value.code == R.CRC and fr.validate_framed(stream) == R.CRC


def test_flipped_payload_byte_of_uncompressed_chunk(fr, oracle):
    parts, chunks = _three_chunks(oracle)
    bad = bytearray(chunks[2])
    bad[8 + 1234] ^= 0x01
    stream = R.IDENTIFIER + chunks[0] + bytes(bad) + chunks[1]
    cs, st, _, _ = decode_chunks(fr, stream)
    assert cs == [0, R.CRC, 0] and st == R.CRC
    assert fr.validate_framed(stream) == R.CRC


def test_corrupted_compressed_payloads(fr, oracle):
    """48 seeded mutations of one compressed chunk's Snappy body (behind its varint), all in one
    stream: each chunk's status is the oracle's for the mutated payload, SMF_ERR_CRC where the
    oracle accepts it with other bytes, SM_OK where it still decodes to the same bytes."""
    data = text_block()[:6000]
    comp = oracle.compress(data)
    hv = 2  # varint(6000)
    rng = np.random.default_rng(21)
    stream, want = [R.IDENTIFIER], []
    for k in range(48):
        m = bytearray(comp)
        for _ in range(1 + k % 3):
            m[int(rng.integers(hv, len(m)))] ^= int(rng.integers(1, 256))
        st, out = oracle.uncompress_status(bytes(m))
        want.append(st if st else (0 if out == data else R.CRC))
        stream.append(R.chunk(0x00, R.crc_field(data) + bytes(m)))
    stream.append(R.raw_chunk(b"tail"))
    want.append(0)
    assert len(set(want)) >= 3  # decode errors, CRC errors and (possibly) harmless mutations all occur
    cs, st, _, _ = decode_chunks(fr, b"".join(stream))
    assert cs == want
    assert st == next(w for w in want if w)


@pytest.mark.parametrize("name,stream,status,nchunks", R.structural_cases(), ids=[c[0] for c in R.structural_cases()])
def test_index_device_matches_host(fr, name, stream, status, nchunks):
    torch = _torch()
    hs, harr = fr.index_framed(stream, max_chunks=8)
    assert hs.status == status
    d_in = _aligned_u8(np.frombuffer(stream, np.uint8), mis=3)  # exactly the stream: a walk past a cut reads outside it
    arrays = fr.device_chunks(8)
    d_sum = torch.zeros(16, dtype=torch.uint8, device=_dev())
    fr.index_framed_device(d_in, arrays, d_sum, n=len(stream))
    ds = fr.read_summary(d_sum)
    assert (ds.status, ds.nchunks, ds.total_length) == (hs.status, hs.nchunks, hs.total_length)
    for k in harr:
        got = arrays[k].cpu().numpy()[:nchunks]
        assert got.view(harr[k].dtype).tolist() == harr[k][:nchunks].tolist(), k
    d_len = torch.full((1,), -1, dtype=torch.int64, device=_dev())
    d_st = torch.full((1,), 77, dtype=torch.int32, device=_dev())
    fr.uncompressed_length_framed_device(d_in, d_len, d_st, n=len(stream))
    assert (int(d_st.item()), int(d_len.item())) == (hs.status, hs.total_length)
    d_out = torch.zeros(max(hs.total_length, 1), dtype=torch.uint8, device=_dev())
    rc = fr.uncompress_framed_device(d_in, d_out, d_len, d_st, n=len(stream))
    if status:
        assert rc == status and int(d_st.item()) == status


def test_index_device_capacity_too_small(fr):
    torch = _torch()
    a = R.raw_chunk(b"a")
    stream = R.IDENTIFIER + a + R.chunk(0xFE, b"pad") + R.raw_chunk(b"bc") + a
    d_in = _aligned_u8(np.frombuffer(stream, np.uint8))
    arrays = fr.device_chunks(2)
    d_sum = torch.zeros(16, dtype=torch.uint8, device=_dev())
    fr.index_framed_device(d_in, arrays, d_sum)
    s = fr.read_summary(d_sum)
    assert (s.status, s.nchunks, s.total_length) == (R.SM_BUFFER_TOO_SMALL, 3, 4)
    assert arrays["ulen"].cpu().tolist() == [1, 2]
    fr.index_framed_device(d_in, None, d_sum)  # count only
    s = fr.read_summary(d_sum)
    assert (s.status, s.nchunks, s.total_length) == (0, 3, 4)


def test_capacity_one_byte_short(fr, oracle):
    torch = _torch()
    data = text_block() + random_bytes(1000, seed=4)
    framed = fr.compress_framed(data, mode="fast")
    # the host call: the size needed comes back
    src = np.frombuffer(framed, np.uint8)
    out = np.zeros(len(data), np.uint8)
    ol = ctypes.c_size_t(len(data) - 1)
    assert fr.lib().smf_uncompress(fr.context(0), src.ctypes.data, src.size, out.ctypes.data, ctypes.byref(ol)) == 2
    assert ol.value == len(data)
    # the device call
    d_in = _aligned_u8(src)
    d_out = torch.zeros(len(data) - 1, dtype=torch.uint8, device=_dev())
    d_len = torch.full((1,), -1, dtype=torch.int64, device=_dev())
    d_st = torch.full((1,), 77, dtype=torch.int32, device=_dev())
    assert fr.uncompress_framed_device(d_in, d_out, d_len, d_st) == R.SM_BUFFER_TOO_SMALL
    torch.cuda.synchronize()
    assert (int(d_st.item()), int(d_len.item())) == (R.SM_BUFFER_TOO_SMALL, len(data))
    # the chunk call: the chunk that would end past the capacity is not decoded, the other is
    cs, st, length, got = decode_chunks(fr, framed, capacity=len(data) - 1)
    assert cs == [0, R.SM_BUFFER_TOO_SMALL] and st == R.SM_BUFFER_TOO_SMALL and length == len(data)
    assert got[:BLOCK] == data[:BLOCK] and got[BLOCK:] == bytes(len(data) - 1 - BLOCK)
    # compress into too small a buffer: refused before any launch
    d_small = torch.zeros(R.max_framed_length(len(data)) - 1, dtype=torch.uint8, device=_dev())
    with pytest.raises(fr.SnappyError) as e:
        fr.compress_framed_device(_aligned_u8(np.frombuffer(data, np.uint8)), d_small, d_len, d_st)
    assert e.value.code == R.SM_BUFFER_TOO_SMALL


# ---- device API -----------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["reference", "fast"])
def test_device_api_on_a_side_stream(fr, oracle, mode):
    torch = _torch()
    data = _inputs()["text_random_text"]
    side = torch.cuda.Stream(device=_dev())
    d_data = _aligned_u8(np.frombuffer(data, np.uint8), mis=5)
    cap = R.max_framed_length(len(data))
    d_framed = torch.zeros(cap, dtype=torch.uint8, device=_dev())
    d_back = torch.zeros(len(data), dtype=torch.uint8, device=_dev())
    d_len = torch.full((2,), -1, dtype=torch.int64, device=_dev())
    d_st = torch.full((2,), 77, dtype=torch.int32, device=_dev())
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        fr.compress_framed_device(d_data, d_framed, d_len[0:1], d_st[0:1], mode=mode, stream=side)
        # the framed length is still on the device: hand the decoder the whole buffer's stream by
        # synchronising once for the length, as a caller would
        side.synchronize()
        n = int(d_len[0].item())
        rc = fr.uncompress_framed_device(d_framed, d_back, d_len[1:2], d_st[1:2], n=n, stream=side)
    assert rc == 0
    side.synchronize()
    assert d_st.cpu().tolist() == [0, 0]
    assert d_len.cpu().tolist() == [n, len(data)]
    framed = d_framed.cpu().numpy().tobytes()[:n]
    if mode == "reference":
        assert framed == R.encode(data, oracle)
    else:
        assert R.decode(framed, oracle) == data
    assert d_back.cpu().numpy().tobytes() == data
    assert not d_framed[n:].any()  # nothing written past the stream
