"""The Parquet page encoder on the GPU (snappy.jl_amd/parquet.py over libsnappy_mi355x_parquet.so,
include/snappy_mi355x_parquet_write.h): the plain column chunks of four files pyarrow wrote with
compression="none", header shapes no writer emits, every rejection, the batch rules and the three
bounds.  Every expected value comes from tests/parquet_write_ref.py over the CPU oracle's compressor,
tests/parquet_ref.py, zlib and the committed fixture record; in the fast modes, whose bytes nobody
else writes, the output is judged by this library's own decoder with CRC verification on, by the
oracle's decoder and by the decode walk."""
import functools
import importlib
import io
import json
import os
import sys
import zlib

import numpy as np
import pytest

import parquet_ref as R
import parquet_write_ref as W
from conftest import ROOT, load_package

pytestmark = pytest.mark.gpu

GUARD = 0xA5
ARG = R.SM_ERR_ARGUMENT
GOLDEN = os.path.join(ROOT, "tests", "golden", "parquet_write")
FILES = ("v1.parquet", "v2.parquet", "bigpage.parquet", "v1_nocrc.parquet")


@pytest.fixture(scope="module")
def pq(gpu_available):
    load_package()
    return importlib.import_module("snappy_jl_amd.parquet")


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
def fixture_chunks(name):
    """[(record, bytes)] of a fixture file's column chunks, in their plain form"""
    with open(os.path.join(GOLDEN, "parquet_write_fixture.json")) as f:
        rec = json.load(f)["files"][name]
    with open(os.path.join(GOLDEN, name), "rb") as f:
        data = f.read()
    return [(c, data[c["offset"]:c["offset"] + c["length"]]) for c in rec["chunks"]]


@functools.lru_cache(maxsize=None)
def reference(chunk):
    """(status, bytes or None): the reference transcoder over the CPU oracle's compressor"""
    return W.transcode(chunk, _oracle().compress)


def bodies(chunk):
    """the plain chunk's page bodies back to back: what a decoder of its SNAPPY form returns"""
    return b"".join(chunk[p.hdr_off + p.hdr_len:p.hdr_off + p.hdr_len + p.body_len] for p in W.walk(chunk)[1] if p.output)


def place(sizes, mods, start):
    """offsets of regions of `sizes` bytes, region i at the next address that is mods[i] mod 16, with at
    least 16 bytes between two of them"""
    offs, pos = [], start
    for n, m in zip(sizes, mods):
        pos += 16 + (m - pos - 16) % 16
        offs.append(pos)
        pos += n
    return offs, pos


def run_encode(pq, chunks, caps, max_pages, stage, frags, mode="reference", in_mods=None, out_mods=None, with_pages=True):
    """One smqe_compress_chunks_device call: chunk i at an address that is in_mods[i] mod 16 (default:
    odd places), its room of caps[i] bytes at out_mods[i] mod 16 in a guard-filled buffer with at least
    16 guard bytes on both sides."""
    torch = _torch()
    k = len(chunks)
    in_mods = in_mods or [(3 * i + 1) % 16 for i in range(k)]
    out_mods = out_mods or [(5 * i + 3) % 16 for i in range(k)]
    in_off, in_end = place([len(c) for c in chunks], in_mods, 0)
    host = np.full(max(in_end, 1), 0x5A, np.uint8)  # (the tensor ends with the last chunk's last byte)
    for o, c in zip(in_off, chunks):
        host[o:o + len(c)] = np.frombuffer(c, np.uint8)
    d_in = torch.from_numpy(host).to(_dev())
    offs, out_end = place(caps, out_mods, 0)
    d_out = torch.full((out_end + 32,), GUARD, dtype=torch.uint8, device=_dev())
    assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    m = max(max_pages, 1)
    d_ol = torch.full((k,), -1, dtype=torch.int64, device=_dev())
    d_st = torch.full((k,), 77, dtype=torch.int32, device=_dev())
    d_pf = d_ps = d_pages = None
    if with_pages:
        d_pf = torch.full((k + 1,), -1, dtype=torch.int32, device=_dev())
        d_ps = torch.full((m,), 77, dtype=torch.int32, device=_dev())
        d_pages = {key: torch.full((m,), -7, dtype=torch.int64 if key in ("hdr_off", "out_off") else torch.int32, device=_dev())
                   for key in pq.INDEX_KEYS}
    pq.compress_column_chunks_device(d_in, _i64(in_off), _i64([len(c) for c in chunks]), max_pages, stage, frags, d_out, _i64(offs),
                                     _i64(caps), d_ol, d_st, mode=mode, d_page_first=d_pf, d_page_status=d_ps, d_pages=d_pages)
    torch.cuda.synchronize()
    table = None
    if with_pages:
        table = {key: d_pages[key].cpu().numpy().astype(np.int64)[:max_pages] for key in pq.INDEX_KEYS}
        for key in ("flags", "crc", "hdr_len", "body_len", "usize", "levels"):
            table[key] = table[key] & 0xFFFFFFFF
    out = d_out.cpu().numpy()
    status, length = d_st.cpu().tolist(), d_ol.cpu().tolist()
    outside = np.ones(out.size, bool)
    for c in range(k):
        if status[c] == 0:
            assert 0 <= length[c] <= caps[c]
            outside[offs[c]:offs[c] + length[c]] = False
    assert (out[outside] == GUARD).all(), "bytes outside the written chunks were touched"
    return dict(status=status, length=length, offs=offs, table=table, first=d_pf.cpu().tolist() if with_pages else None,
                page_status=d_ps.cpu().tolist()[:max_pages] if with_pages else None,
                chunks=[out[o:o + n].tobytes() if s == 0 else None for o, n, s in zip(offs, length, status)])


def judge(pq, chunk, out, rows=None):
    """A written chunk against its plain form, whatever the compressor's mode: the decode walk accepts
    it, every header's crc is zlib's of the stored body, every section decodes under the oracle to the
    plain section, pages that are stepped over are the input's bytes; `rows`: the device's page table."""
    st, pages, total = R.walk(out)
    _, plain, _, plain_total = W.walk(chunk)
    assert st == 0 and len(pages) == len(plain) and total == plain_total
    s, a = pq.index_column_chunk(out)
    assert s.status == 0 and {k: a[k].tolist() for k in pq.INDEX_KEYS} == R.table(pages)
    if rows is not None:
        assert rows == R.table(pages)
    for p, q in zip(pages, plain):
        body = out[p.hdr_off + p.hdr_len:p.hdr_off + p.hdr_len + p.body_len]
        was = chunk[q.hdr_off + q.hdr_len:q.hdr_off + q.hdr_len + q.body_len]
        assert (p.type, p.usize, p.levels, p.num_values, p.encoding, p.flags & R.HAS_CRC) == \
            (q.type, q.usize, q.levels, q.num_values, q.encoding, q.flags & R.HAS_CRC)
        if not q.output:
            assert out[p.hdr_off:p.hdr_off + p.hdr_len] + body == chunk[q.hdr_off:q.hdr_off + q.hdr_len] + was
            continue
        assert p.flags & R.COMPRESSED and body[:p.levels] == was[:q.levels]
        code, values = _oracle().uncompress_status(body[p.levels:])
        assert code == 0 and values == was[q.levels:]
        if p.flags & R.HAS_CRC:
            assert p.crc == zlib.crc32(body)


def rows_of(table, first, c):
    return {k: table[k][first[c]:first[c + 1]].tolist() for k in R.TABLE_KEYS}


# ---- the fixture: what parquet-cpp writes with compression=NONE ----------------------------------------------

@pytest.mark.parametrize("name", FILES)
def test_fixture_chunks_in_reference_mode(pq, name):
    """Byte for byte the reference transcoder over the oracle -- which pyarrow read back on the CPU
    (tests/test_parquet_write_host.py); where pyarrow imports, it reads the device's bytes too."""
    chunks = [c for _, c in fixture_chunks(name)]
    want = [reference(c) for c in chunks]
    rc, first, status, bound, pages, stage, frags = pq.compress_chunks_plan(chunks)
    assert rc == 0 and not status.any() and frags == (3 if name == "bigpage.parquet" else 0)
    res = run_encode(pq, chunks, [len(w) for _, w in want], pages, stage, frags)
    assert res["status"] == [0] * len(chunks) and res["chunks"] == [w for _, w in want]
    assert res["first"] == first.tolist() and res["page_status"] == [0] * pages
    for c, chunk in enumerate(chunks):
        judge(pq, chunk, res["chunks"][c], rows_of(res["table"], res["first"], c))
    try:
        import pyarrow.parquet as pap
    except ImportError:
        return
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_parquet_fixture import FILES as RECIPES
    with open(os.path.join(GOLDEN, name), "rb") as f:
        data = f.read()
    spliced = W.splice_file(data, None, {rec["offset"]: out for (rec, _), out in zip(fixture_chunks(name), res["chunks"])})
    assert pap.read_table(io.BytesIO(spliced), page_checksum_verification=True).equals(RECIPES[name][0]())


@pytest.mark.parametrize("mode", ["fast", "dense"])
def test_fast_modes_round_trip(pq, mode):
    """All fixture chunks in one call: the output passes smq_index and this library's decoder, with
    CRC verification on, returns the input's page bodies."""
    chunks = [c for name in FILES for _, c in fixture_chunks(name)]
    rc, first, status, bound, pages, stage, frags = pq.compress_chunks_plan(chunks)
    res = run_encode(pq, chunks, bound.tolist(), pages, stage, frags, mode=mode)
    assert res["status"] == [0] * len(chunks) and res["page_status"] == [0] * pages
    for c, chunk in enumerate(chunks):
        judge(pq, chunk, res["chunks"][c], rows_of(res["table"], res["first"], c))
    decoded = pq.uncompress_column_chunks(res["chunks"], verify_crc=True)
    assert [d for d, _ in decoded] == [bodies(c) for c in chunks]
    # and the host-buffer twin gives the same bytes
    assert pq.compress_column_chunks(chunks, mode=mode) == res["chunks"]


# ---- shapes no writer emits -------------------------------------------------------------------------------------

def synthetic_chunks():
    rng = np.random.default_rng(77)
    shapes = W.shape_cases(sections=(0, 1, 40, 100, 5000))
    shapes.append(("a section whose size varint shrinks", W.plain_page_v1(b"abcdefgh" * 1125, crc=True)))  # 9,000 bytes
    for n in (70000, 1100000):  # random: they grow, the larger through the fragment path
        shapes.append(("%d random bytes" % n, W.plain_page_v2(b"\x01\x02", b"\x03" * 5, rng.integers(0, 256, n, dtype=np.uint8).tobytes(),
                                                              crc=True, is_compressed=False)))
    return shapes


def test_synthetic_shapes(pq):
    shapes = synthetic_chunks()
    chunks = [c for _, c in shapes]
    want = [reference(c) for c in chunks]
    assert all(st == 0 for st, _ in want)
    shrunk = dict(zip([n for n, _ in shapes], want))["a section whose size varint shrinks"][1]
    assert R.walk(shrunk)[1][0].body_len < 8192 <= 9000
    rc, first, status, bound, pages, stage, frags = pq.compress_chunks_plan(chunks)
    assert rc == 0 and frags == 2 + 17
    res = run_encode(pq, chunks, [len(w) for _, w in want], pages, stage, frags)
    for (name, chunk), (_, w), got, st in zip(shapes, want, res["chunks"], res["status"]):
        assert st == 0 and got == w, name
    for c, chunk in enumerate(chunks):
        judge(pq, chunk, res["chunks"][c], rows_of(res["table"], res["first"], c))
    assert res["first"] == first.tolist()


def test_every_alignment(pq):
    """every chunk start alignment 0..15 crossed with every output alignment 0..15, one call"""
    P = R.payload
    chunk = W.plain_page_v1(P(1, 130), crc=True, ptype=R.DICTIONARY_PAGE) + W.plain_page_v2(b"\x01" * 3, b"\x02" * 18, P(2, 290), crc=True,
                                                                                                  is_compressed=False) + \
        W.plain_page_v1(P(3, 77))
    want = reference(chunk)[1]
    in_mods = [a for a in range(16) for _ in range(16)]
    out_mods = [b for _ in range(16) for b in range(16)]
    chunks = [chunk] * 256
    rc, first, status, bound, pages, stage, frags = pq.compress_chunks_plan(chunks)
    res = run_encode(pq, chunks, [len(want)] * 256, pages, stage, frags, in_mods=in_mods, out_mods=out_mods, with_pages=False)
    assert res["status"] == [0] * 256 and res["chunks"] == [want] * 256
    assert sorted({(o % 16) for o in res["offs"]}) == list(range(16))


# ---- the batch rules ----------------------------------------------------------------------------------------------

def mixed_batch():
    """64 chunks: valid ones, every rejection, the empty chunk"""
    good = [c for _, c in W.shape_cases()] + [c for _, c in fixture_chunks("v2.parquet")]
    bad = [c for _, c, _ in W.rejection_cases()]
    chunks = []
    while len(chunks) < 64:
        chunks.append((good if len(chunks) % 3 else bad)[(len(chunks) // 3) % len(good if len(chunks) % 3 else bad)])
    assert {W.walk(c)[0] for c in chunks} == {0, R.HEADER, R.TRUNCATED, R.SIZE_MISMATCH}
    return chunks


def test_batch_of_64(pq):
    chunks = mixed_batch()
    want = [reference(c) for c in chunks]
    rc, first, status, bound, pages, stage, frags = pq.compress_chunks_plan(chunks)
    assert rc == 0 and status.tolist() == [st for st, _ in want]
    caps = [len(w) if st == 0 else 40 for st, w in want]
    victim = next(i for i, (st, w) in enumerate(want) if st == 0 and len(w) > 1000)
    caps[victim] -= 1
    res = run_encode(pq, chunks, caps, pages, stage, frags)
    for c, (st, w) in enumerate(want):
        if c == victim:  # the size needed, and nothing written (run_encode checked the guards)
            assert (res["status"][c], res["length"][c]) == (R.SM_BUFFER_TOO_SMALL, len(w))
        elif st:
            assert (res["status"][c], res["length"][c]) == (st, 0)
        else:
            assert res["status"][c] == 0 and res["chunks"][c] == w, c
    assert res["first"] == first.tolist() and res["page_status"] == [0] * pages
    # the host-buffer twin: the same statuses and bytes
    got, codes = pq.compress_column_chunks(chunks, mode="reference", statuses=True)
    assert codes == [st for st, _ in want] and got == [w for _, w in want]
    with pytest.raises(pq.ParquetError) as e:
        pq.compress_column_chunks(chunks, mode="reference")
    assert (e.value.code, e.value.chunk) == next((st, i) for i, (st, _) in enumerate(want) if st)
    with pytest.raises(pq.ParquetError) as e:
        pq.compress_column_chunk(chunks[0] if want[0][0] else next(c for c, (st, _) in zip(chunks, want) if st))
    assert e.value.chunk is None


@pytest.mark.parametrize("short", ["max_pages", "stage_bytes", "max_fragments"])
def test_a_bound_one_below_the_plan(pq, short):
    chunks = [c for _, c in fixture_chunks("bigpage.parquet")] + [c for _, c in fixture_chunks("v1.parquet")]
    rc, first, status, bound, pages, stage, frags = pq.compress_chunks_plan(chunks)
    args = dict(max_pages=pages, stage_bytes=stage, max_fragments=frags)
    assert frags == 3
    args[short] -= 1
    res = run_encode(pq, chunks, bound.tolist(), args["max_pages"], args["stage_bytes"], args["max_fragments"])
    assert res["status"] == [ARG] * len(chunks) and res["length"] == [0] * len(chunks)  # (run_encode: d_out is untouched)
    assert res["page_status"] == [0] * args["max_pages"]
    # at the plan's values it runs
    res = run_encode(pq, chunks, bound.tolist(), pages, stage, frags, with_pages=False)
    assert res["status"] == [0] * len(chunks) and res["chunks"] == [reference(c)[1] for c in chunks]


def test_header_mutations(pq):
    """the 200 seeded mutants of the host test in one call: reference, host and device agree"""
    chunk = fixture_chunks("v2.parquet")[4][1]
    pages = W.walk(chunk)[1]
    rng = np.random.default_rng(20250301)
    chunks = []
    for _ in range(200):
        p = pages[int(rng.integers(0, len(pages)))]
        at = p.hdr_off + int(rng.integers(0, p.hdr_len))
        mutated = bytearray(chunk)
        mutated[at] ^= int(rng.integers(1, 256))
        chunks.append(bytes(mutated))
    want = [reference(c) for c in chunks]
    accepted = sum(1 for st, _ in want if st == 0)
    assert accepted >= 20 and len(chunks) - accepted >= 20
    rc, first, status, bound, npages, stage, frags = pq.compress_chunks_plan(chunks)
    assert status.tolist() == [st for st, _ in want]
    res = run_encode(pq, chunks, [len(w) if st == 0 else 8 for st, w in want], npages, stage, frags)
    assert res["status"] == [st for st, _ in want]
    assert res["chunks"] == [w for _, w in want]
    assert res["first"] == first.tolist()


def test_no_chunks_and_no_pages(pq):
    torch = _torch()
    empty = torch.zeros(1, dtype=torch.uint8, device=_dev())
    none = torch.zeros(0, dtype=torch.int64, device=_dev())
    pq.compress_column_chunks_device(empty, none, none, 0, 0, 0, empty, none, none, none, torch.zeros(0, dtype=torch.int32, device=_dev()))
    res = run_encode(pq, [b"", b"\x15"], [0, 0], 0, 0, 0, with_pages=False)
    assert res["status"] == [0, R.TRUNCATED] and res["length"] == [0, 0]
    assert pq.compress_column_chunks([]) == [] and pq.compress_column_chunk(b"") == b""


def test_wrapper_on_a_side_stream(pq):
    """the tensor wrapper on a non-default torch stream and a ctx of its own, whose scratch grows between two calls"""
    torch = _torch()
    side = torch.cuda.Stream(device=_dev())
    ctx = ("write wrappers", 0, 0)
    for name in ("v1.parquet", "v2.parquet"):
        chunks = [c for _, c in fixture_chunks(name)] * (1 if name == "v1.parquet" else 4)
        want = [reference(c)[1] for c in chunks]
        rc, first, status, bound, pages, stage, frags = pq.compress_chunks_plan(chunks)
        caps = bound.tolist()
        in_off, in_end = place([len(c) for c in chunks], [5] * len(chunks), 0)
        host = np.zeros(in_end, np.uint8)
        for o, c in zip(in_off, chunks):
            host[o:o + len(c)] = np.frombuffer(c, np.uint8)
        d_in = torch.from_numpy(host).to(_dev())
        offs, out_end = place(caps, [0] * len(chunks), 0)
        d_out = torch.full((out_end + 16,), GUARD, dtype=torch.uint8, device=_dev())
        d_ol = torch.full((len(chunks),), -1, dtype=torch.int64, device=_dev())
        d_st = torch.full((len(chunks),), 77, dtype=torch.int32, device=_dev())
        args = [_i64(in_off), _i64([len(c) for c in chunks]), _i64(offs), _i64(caps)]
        torch.cuda.synchronize()  # (the inputs were made on the default stream)
        pq.compress_column_chunks_device(d_in, args[0], args[1], pages + 7, stage + 100, frags + 2, d_out, args[2], args[3], d_ol, d_st,
                                         mode="reference", stream=side, device=ctx)
        side.synchronize()
        assert d_st.cpu().tolist() == [0] * len(chunks) and d_ol.cpu().tolist() == [len(w) for w in want]
        out = d_out.cpu().numpy()
        assert [out[o:o + len(w)].tobytes() for o, w in zip(offs, want)] == want
    assert pq._ctx[ctx] != pq.context(0)
