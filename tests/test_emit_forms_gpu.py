"""Every form a compressor emits, at every writer that emits it.

The emit rules are written once (sm_format.h literal_tag, copy_piece, copy_piece_len,
block_literal_bytes / block_literal_head_byte, parts_verdict; common/smc_layout.h varint_byte), and
sm_host_check sweeps them on the CPU.  These tests pin the bytes the kernels make of them.

Literal forms.  Seeded random blocks of 1, 59, 60, 61, 256, 257, 8191, 8192, 65535 and 65536 bytes:
no tag size, screen threshold or block size is left out.  Reference mode must equal the CPU oracle
(which has the reference's two-byte tag for a 60-byte run, quirk Q3); the fast modes must give
varint(n) + the standard literal tag + the bytes, built here by hand and checked against the
oracle's decoder.  Paths: the host batch call (the whole-block writer and its fallback, the
screen), the single-buffer call (the span parse and the single-stream parts gather), the device
batch call with three blocks (all of them parsed in parts and joined by the batch gather), the
fragment call (no header), and sm_place_fragments_device's varint at both ends of its length
classes.  The multi library's pack kernel writes its header by the same varint_byte, but only
for streams of more than one 64 KiB block; tests/test_multi_gpu.py covers it there.

Copy forms.  Blocks R + R[a : a + L] + tail, R seeded random bytes, the copy inside one 1 KiB
super-chunk, for L = 4, 11, 12, 60, 64, 65, 67, 68, 69, 128, 255 and a source distance below and
above 2048.  The tail is a few random bytes, a run of one byte (so that the parse stays shorter
than one literal of the block and no writer falls back) and a few random bytes.  The seed of each
block is the first one from its row's base for which, on the CPU, the bytes around the copy differ
(so it is exactly L long), no position between the source and the copy shares the source's 13-bit
hash bucket (the fast parse keeps the latest earlier position per bucket), and the oracle's
streams (compat = 1 and the reference's own) have the copy as the reference's piece sequence for
L.  Every GPU stream must decode under the oracle and show the same piece sequence; a row the
parse does not hit fails.
Reference mode must equal the oracle for the same blocks and for a 1,000-byte run of one byte.
"""
import functools

import numpy as np
import pytest

import streams

gpu = pytest.mark.gpu

MODES = ("reference", "fast", "dense")
SIZES = (1, 59, 60, 61, 256, 257, 8191, 8192, 65535, 65536)
GROUPS = ((1, 59, 60), (61, 256, 257), (8191, 8192, 65535), (65536, 60, 1))  # the device calls' batches of three
COPY_L = (4, 11, 12, 60, 64, 65, 67, 68, 69, 128, 255)
HASH_MUL = 0x1E35A7BD
ROWS = [(L, far) for L in COPY_L for far in (False, True)]


@functools.lru_cache(maxsize=None)
def random_block(n):
    return np.random.default_rng(0xE317 + n).integers(0, 256, n, dtype=np.uint8).tobytes()


def literal_stream(block, header=True):
    """The block as one literal under the standard rule, by hand."""
    m = len(block) - 1
    if m < 60:
        tag = bytes([m << 2])
    else:
        k = 1 if m < 256 else 2 if m < 65536 else 3
        tag = bytes([(59 + k) << 2]) + m.to_bytes(k, "little")
    return (streams.varint(len(block)) if header else b"") + tag + block


def expected(oracle, mode, block, total=None):
    """The stream of a random block: with its header, or (total given) as a fragment of a stream."""
    if mode == "reference":
        return oracle.compress(block) if total is None else oracle.compress_fragment(block, total)
    return literal_stream(block, total is None)


def list_tags(stream, header=True):
    """[('lit', length) | ('copy', offset, length)] of a stream, read byte by byte."""
    p = 0
    if header:
        while stream[p] >= 0x80:
            p += 1
        p += 1
    out = []
    while p < len(stream):
        c = stream[p]
        kind, up = c & 3, c >> 2
        if kind == 0:
            extra = up - 59 if up >= 60 else 0
            ln = 1 + int.from_bytes(stream[p + 1:p + 1 + extra], "little") if extra else up + 1
            out.append(("lit", ln))
            p += 1 + extra + ln
        elif kind == 1:
            out.append(("copy", ((c >> 5) << 8) | stream[p + 1], 4 + (up & 7)))
            p += 2
        else:
            n = 2 if kind == 2 else 4
            out.append(("copy", int.from_bytes(stream[p + 1:p + 1 + n], "little"), up + 1))
            p += 1 + n
    assert p == len(stream)
    return out


def pieces(L):
    """emit_copy!'s split (internal.jl:306-329), written out."""
    out = []
    while L >= 68:
        out.append(64)
        L -= 64
    if L > 64:
        out.append(60)
        L -= 60
    return out + [L]


def has_copy(tags, d, L):
    """The copy (d, L) as the reference's piece sequence, and no further piece of offset d around it."""
    want = [("copy", d, l) for l in pieces(L)]
    for i in range(len(tags) - len(want) + 1):
        if tags[i:i + len(want)] == want:
            before = tags[i - 1] if i else ("lit", 0)
            after = tags[i + len(want)] if i + len(want) < len(tags) else ("lit", 0)
            if before[:2] != ("copy", d) and after[:2] != ("copy", d):
                return True
    return False


def copy_form(stream, d, L):
    """The tag bytes the format prescribes for the copy's pieces are in the stream."""
    raw = b"".join(streams.copy_tag(d, l) for l in pieces(L))
    return raw in stream


def buckets(block):
    b = np.frombuffer(block, np.uint8).astype(np.uint64)
    w = b[:-3] | (b[1:-2] << 8) | (b[2:-1] << 16) | (b[3:] << 24)
    return ((w * HASH_MUL) & 0xFFFFFFFF) >> 19


@functools.lru_cache(maxsize=None)
def copy_block(L, far):
    """(block, distance) of one row: see the module's docstring."""
    import oracle as O
    for seed in range(100000 * L + (50000 if far else 0), 100000 * L + 50000 + (50000 if far else 0)):
        rng = np.random.default_rng(seed)
        # the copy starts at nr, in super-chunk 2 or 0, and ends inside it (the reference probes a
        # fixed sequence of positions while it finds nothing, so nr moves with the seed)
        nr = (2100 if far else 304) + seed % 32
        R = rng.integers(0, 256, nr, dtype=np.uint8).tobytes()
        a = int(rng.integers(1, 33))
        U = rng.integers(0, 256, 40, dtype=np.uint8).tobytes()
        V = rng.integers(0, 256, 8, dtype=np.uint8).tobytes()
        block = R + R[a:a + L] + U + bytes([U[-1] ^ 0x55]) * 200 + V
        d = nr - a
        if R[a - 1] == R[nr - 1] or R[a + L] == U[0] or (d < 2048) == far:
            continue
        h = buckets(block)
        if (h[a + 1:nr] == h[a]).any():
            continue
        if has_copy(list_tags(O.compress(block, compat=True)), d, L) and has_copy(list_tags(O.compress(block)), d, L):
            return block, d
    raise AssertionError("no seed gives row (%d, %s) its copy" % (L, far))


RUN = b"\x6b" * 1000


# ---- CPU --------------------------------------------------------------------------------------------

def test_hand_built_literal_streams_decode(oracle):
    for n in SIZES:
        block = random_block(n)
        assert oracle.uncompress(literal_stream(block)) == block
    s60 = oracle.compress(random_block(60))
    assert s60 == streams.varint(60) + bytes([60 << 2, 59]) + random_block(60)  # the reference's Q3 form
    assert oracle.compress(random_block(60), compat=True) == literal_stream(random_block(60))
    assert oracle.compress(random_block(59)) == literal_stream(random_block(59))


def test_copy_blocks_hold_their_copy(oracle):
    for L, far in ROWS:
        block, d = copy_block(L, far)
        assert len(block) <= 65536 and (d >= 2048) == far
        q = block.index(block[-8:]) - 240 - L  # (the tail is 40 + 200 + 8 bytes)
        assert (2100 if far else 304) <= q < (2132 if far else 336)
        assert q // 1024 == (q + L - 1) // 1024
        s = oracle.compress(block, compat=True)
        assert oracle.uncompress(s) == block
        assert has_copy(list_tags(s), d, L) and copy_form(s, d, L), (L, far)
    assert pieces(65) == [60, 5] and pieces(68) == [64, 4] and pieces(255) == [64, 64, 64, 63]


# ---- GPU --------------------------------------------------------------------------------------------

def device_call(sm, call, mode, blocks):
    """One device batch call (call: "batch" or "frag") into slots at an odd pitch: the streams and
    sm_ctx_last_batch_parts after the call."""
    import torch
    dev = torch.device("cuda", 0)
    lens = np.array([len(b) for b in blocks], np.int64)
    n = len(blocks)
    pitch = 76490 + 5 + 8
    d_in = torch.from_numpy(np.frombuffer(b"".join(blocks) + bytes(16), np.uint8).copy()).to(dev)
    in_off = torch.from_numpy(np.cumsum(lens) - lens).to(dev)
    in_len = torch.from_numpy(lens.astype(np.int32)).to(dev)
    d_out = torch.zeros(n * pitch, dtype=torch.uint8, device=dev)
    off = np.arange(n, dtype=np.int64) * pitch
    out_off = torch.from_numpy(off).to(dev)
    out_len = torch.full((n,), 7, dtype=torch.int32, device=dev)
    if call == "batch":
        sm.compress_batch_device(d_in, in_off, in_len, d_out, out_off, out_len, mode=mode)
    else:
        sm.compress_fragments_device(d_in, in_off, in_len, d_out, out_off, out_len, int(lens.sum()), mode=mode)
    parts = sm.last_batch_parts(0)
    torch.cuda.synchronize()
    cl = out_len.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    out = d_out.cpu().numpy()
    assert (cl <= 32 + lens + lens // 6 + 5).all(), cl
    return [out[o:o + c].tobytes() for o, c in zip(off, cl)], parts


@gpu
@pytest.mark.parametrize("mode", MODES)
def test_literal_forms_host_batch(sm, oracle, gpu_available, mode):
    blocks = [random_block(n) for n in SIZES]
    got = sm.compress_batch(blocks, mode=mode)
    for n, block, s in zip(SIZES, blocks, got):
        assert s == expected(oracle, mode, block), (mode, n, s[:8].hex())


@gpu
@pytest.mark.parametrize("mode", MODES)
def test_literal_forms_single_buffer(sm, oracle, gpu_available, mode):
    for n in SIZES:
        block = random_block(n)
        s = sm.compress(block, mode=mode)
        assert s == expected(oracle, mode, block), (mode, n, s[:8].hex())
        if mode != "reference":
            assert sm.last_compress_split(0), (mode, n)  # the span parse and the parts gather


@gpu
@pytest.mark.parametrize("mode", MODES)
def test_literal_forms_device_calls(sm, oracle, gpu_available, mode):
    for group in GROUPS:
        blocks = [random_block(n) for n in group]
        total = sum(group)
        for call in ("batch", "frag"):
            got, parts = device_call(sm, call, mode, blocks)
            if mode != "reference":
                assert parts == len(blocks), (mode, call, group, parts)  # every block in parts: the batch gather
            for n, block, s in zip(group, blocks, got):
                want = expected(oracle, mode, block, total if call == "frag" else None)
                assert s == want, (mode, call, n, s[:8].hex())


@gpu
def test_placed_varint(sm, gpu_available):
    import torch
    dev = torch.device("cuda", 0)
    frag = random_block(59)
    for total in (127, 128, 16383, 16384, 1 << 21):
        hv = len(streams.varint(total))
        d_src = torch.from_numpy(np.frombuffer(frag + bytes(5), np.uint8).copy()).to(dev)
        d_dst = torch.full((96,), 0xA5, dtype=torch.uint8, device=dev)
        d_st = torch.zeros(1, dtype=torch.int32, device=dev)
        sm.place_fragments_device(d_src, torch.zeros(1, dtype=torch.int64, device=dev),
                                  torch.full((1,), len(frag), dtype=torch.int32, device=dev),
                                  torch.full((1,), hv, dtype=torch.int64, device=dev), d_dst, total, True, d_status=d_st)
        torch.cuda.synchronize()
        want = streams.varint(total) + frag
        assert d_dst.cpu().numpy().tobytes() == want + b"\xa5" * (96 - len(want)), total
        assert int(d_st.item()) == 0


@gpu
@pytest.mark.parametrize("mode", MODES)
def test_copy_forms(sm, oracle, gpu_available, mode):
    rows = [copy_block(L, far) for L, far in ROWS]
    blocks = [b for b, _ in rows] + [RUN]
    got = sm.compress_batch(blocks, mode=mode)
    missing = []
    for (L, far), (block, d), s in zip(ROWS, rows, got):
        assert oracle.uncompress(s) == block, (mode, L, far)
        if mode == "reference":
            assert s == oracle.compress(block), (mode, L, far)
        elif not (has_copy(list_tags(s), d, min(L, 255)) and copy_form(s, d, min(L, 255))):
            missing.append((L, far, list_tags(s)[:6]))
    assert not missing, (mode, missing)
    assert oracle.uncompress(got[-1]) == RUN
    if mode == "reference":
        assert got[-1] == oracle.compress(RUN)
