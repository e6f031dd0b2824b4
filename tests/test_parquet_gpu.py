"""The Parquet page library on the GPU (snappy.jl_amd/parquet.py over libsnappy_mi355x_parquet.so):
the column chunks of four files pyarrow wrote, header shapes no writer emits from the reference's
own Thrift writer, every rejection, the batch rules and the CRC-32 pass alone.  Every expected value
comes from tests/parquet_ref.py, the CPU oracle, zlib and the committed fixture record."""
import functools
import hashlib
import importlib
import json
import os
import zlib

import numpy as np
import pytest

import parquet_ref as R
from conftest import ROOT, load_package

pytestmark = pytest.mark.gpu

GUARD = 0xA5
ARG = R.SM_ERR_ARGUMENT
GOLDEN = os.path.join(ROOT, "tests", "golden", "parquet")
FILES = ("v1.parquet", "v2.parquet", "bigpage.parquet", "v1_nocrc.parquet")
SEGMENT = 65536  # the CRC pass's segment (include/snappy_mi355x_parquet.h)
SM_ERR_COPY_OFFSET = 19
BAD_COPY = b"\x0a\x04ab\x11\x00"  # 10 bytes declared, the literal "ab", then a copy with offset 0


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


def _status():
    return R.oracle_status(_oracle())


def _compress():
    return _oracle().compress


@functools.lru_cache(maxsize=None)
def fixture_chunks(name):
    """[(record, bytes)] of a fixture file's column chunks"""
    with open(os.path.join(GOLDEN, "parquet_fixture.json")) as f:
        rec = json.load(f)["files"][name]
    with open(os.path.join(GOLDEN, name), "rb") as f:
        data = f.read()
    return [(c, data[c["offset"]:c["offset"] + c["length"]]) for c in rec["chunks"]]


def lay(buffers, lead=1, align=None):
    """The buffers in one device tensor, the first at an address that is `lead` mod 64, directly
    behind one another -- or, with align (one value per buffer), each at the next address that is
    align[i] mod 64: (tensor, offsets, lengths).  The tensor ends with the last buffer's last byte."""
    offs, pos = [], lead
    for i, b in enumerate(buffers):
        if align is not None:
            pos += (align[i] - pos) % 64
        offs.append(pos)
        pos += len(b)
    host = np.full(max(pos, 1), 0x5A, np.uint8)
    for o, b in zip(offs, buffers):
        host[o:o + len(b)] = np.frombuffer(bytes(b), np.uint8)
    d = _torch().from_numpy(host).to(_dev())
    assert d.data_ptr() % 64 == 0
    return d, offs, [len(b) for b in buffers]


def run_decode(pq, chunks, caps, max_pages, max_fragments=0, verify_crc=True, with_pages=True, lead=1, align=None):
    """One smq_uncompress_chunks_device call over the chunks laid back to back; every output has its
    cap bytes in a guard-filled buffer with at least 16 guard bytes on both sides, at odd places."""
    torch = _torch()
    d_in, in_off, in_len = lay(chunks, lead, align)
    offs, pos = [], 33
    for c in caps:
        offs.append(pos)
        pos += c + 16 + (c % 3)
    d_out = torch.full((pos + 32,), GUARD, dtype=torch.uint8, device=_dev())
    k, m = len(chunks), max(max_pages, 1)
    d_ol = torch.full((k,), -1, dtype=torch.int64, device=_dev())
    d_st = torch.full((k,), 77, dtype=torch.int32, device=_dev())
    d_pf = torch.full((k + 1,), -1, dtype=torch.int32, device=_dev()) if with_pages else None
    d_ps = torch.full((m,), 77, dtype=torch.int32, device=_dev()) if with_pages else None
    d_pages = None
    if with_pages:
        d_pages = {key: torch.full((m,), -7, dtype=torch.int64 if key in ("hdr_off", "out_off") else torch.int32, device=_dev())
                   for key in pq.INDEX_KEYS}
    pq.uncompress_column_chunks_device(d_in, _i64(in_off), _i64(in_len), max_pages, max_fragments, d_out, _i64(offs), _i64(caps),
                                       d_ol, d_st, verify_crc=verify_crc, d_page_first=d_pf, d_page_status=d_ps, d_pages=d_pages)
    torch.cuda.synchronize()
    table = None
    if with_pages:
        table = {key: d_pages[key].cpu().numpy().astype(np.int64)[:max_pages] for key in pq.INDEX_KEYS}
        for key in ("flags", "crc", "hdr_len", "body_len", "usize", "levels"):
            table[key] = table[key] & 0xFFFFFFFF
    return dict(status=d_st.cpu().tolist(), length=d_ol.cpu().tolist(), out=d_out.cpu().numpy(), offs=offs,
                first=d_pf.cpu().tolist() if with_pages else None,
                page_status=d_ps.cpu().tolist()[:max_pages] if with_pages else None, table=table)


def check_decode(chunks, caps, models, res, max_pages):
    """Per chunk the status, the length and every good page's bytes against the model; the page
    statuses and the page table; and every byte outside the decoded chunks' own content is still
    the guard's."""
    out, offs = res["out"], res["offs"]
    outside = np.ones(out.size, bool)
    wrong, first, want_ps, want_table = [], [0], [], {k: [] for k in R.TABLE_KEYS}
    for c, m in enumerate(models):
        ok = (res["status"][c], res["length"][c]) == (m.status, m.length)
        if m.slots:
            assert m.length <= caps[c]
            outside[offs[c]:offs[c] + m.length] = False
            for piece, p in zip(m.pieces, m.pages):
                if piece is not None and p.output:
                    ok = ok and out[offs[c] + p.out_off:offs[c] + p.out_off + p.usize].tobytes() == piece
            for k, v in R.table(m.pages).items():
                want_table[k] += v
        first.append(first[-1] + m.slots)
        want_ps += m.page_status
        if not ok:
            wrong.append((c, res["status"][c], res["length"][c], m.status, m.length))
    assert not wrong, wrong[:8]
    assert (out[outside] == GUARD).all()
    if res["first"] is not None:
        assert res["first"] == first
        assert res["page_status"] == want_ps + [0] * (max_pages - len(want_ps))
        for k in R.TABLE_KEYS:
            assert res["table"][k].tolist() == want_table[k] + [0] * (max_pages - len(want_ps)), k


def models_of(chunks, caps, verify_crc=True):
    return [R.model(s, c, _status(), verify_crc) for s, c in zip(chunks, caps)]


def decode_and_check(pq, chunks, caps=None, spare=0, **kw):
    caps = [R.walk(s)[2] for s in chunks] if caps is None else caps
    models = models_of(chunks, caps, kw.get("verify_crc", True))
    total = sum(m.slots for m in models)
    res = run_decode(pq, chunks, caps, total + spare, **kw)
    check_decode(chunks, caps, models, res, total + spare)
    return models, res


# ---- 1. the files pyarrow wrote ----------------------------------------------------------------------

@pytest.mark.parametrize("name", FILES)
def test_fixture_files(pq, name):
    recs = [r for r, _ in fixture_chunks(name)]
    chunks = [c for _, c in fixture_chunks(name)]
    caps = [r["decoded_bytes"] for r in recs]
    rc, first, out_len, status, pages, frags = pq.chunks_plan(chunks, out_cap=caps)
    assert (rc, status.tolist(), out_len.tolist(), pages) == (0, [0] * len(chunks), caps, sum(r["pages"] for r in recs))
    res = run_decode(pq, chunks, caps, pages, max_fragments=frags, verify_crc=True)
    assert res["status"] == [0] * len(chunks) and res["length"] == caps and res["page_status"] == [0] * pages
    assert res["first"] == first.tolist()
    got = [res["out"][o:o + n].tobytes() for o, n in zip(res["offs"], caps)]
    assert [hashlib.sha256(g).hexdigest() for g in got] == [r["sha256"] for r in recs]
    assert res["table"]["type"].tolist() == [t for r in recs for t in r["page_types"]]
    assert int((res["table"]["flags"] & R.HAS_CRC).sum()) == sum(r["with_crc"] for r in recs)
    assert int(res["table"]["levels"].sum()) == sum(r["levels"] for r in recs)
    check_decode(chunks, caps, models_of(chunks, caps), res, pages)  # the bytes page by page, the whole table, the guards
    if name == "v1.parquet":  # a required column has no level bytes: the whole stack without the reference
        assert recs[0]["column"] == "counter" and got[0] == np.arange(4000, dtype="<i8").tobytes()
    if name == "bigpage.parquet":
        assert recs[0]["largest_page"] > 131072 and frags >= 3
        assert pq.last_indexed(0) >= 1  # the page went by fragments
        again = run_decode(pq, chunks, caps, pages, max_fragments=0)
        assert again["status"] == [0] and pq.last_indexed(0) == 0 and (again["out"] == res["out"]).all()
    # the host-buffer call and the Python calls give the same bytes and the same table
    decoded = pq.uncompress_column_chunks(chunks)
    assert [d for d, _ in decoded] == got
    assert {k: v.tolist() for k, v in decoded[-1][1].items()} == R.table(R.walk(chunks[-1])[1])
    assert pq.uncompress_column_chunk(chunks[0], verify_crc=False)[0] == got[0]


# ---- 2. header shapes from the reference's writer ----------------------------------------------------

def test_header_shapes(pq):
    cases = R.shape_cases(_compress())
    chunks = [c for _, c in cases]
    models, res = decode_and_check(pq, chunks)
    assert all(m.status == 0 for m in models) and sum(m.slots for m in models) >= 16
    names = [n for n, _ in cases]
    empty = names.index("the empty chunk")
    assert (res["status"][empty], res["length"][empty], models[empty].slots) == (0, 0, 0)
    skipped = models[names.index("an index page between data pages")]
    assert skipped.pieces[1] == skipped.pieces[2] == b"" and skipped.length == 400
    # every chunk alone, at another start, with spare slots and no page table
    for lead, c in enumerate(chunks):
        decode_and_check(pq, [c], spare=3, with_pages=False, lead=17 + lead)


def test_every_start_alignment(pq):
    """The same two-page chunk at every start 0 .. 63 mod 64: a header meets every window boundary"""
    two = dict(R.shape_cases(_compress()))["two pages"]
    chunks = [two] * 64
    caps = [R.walk(two)[2]] * 64
    models = models_of(chunks[:1], caps[:1]) * 64
    res = run_decode(pq, chunks, caps, 128, align=list(range(64)))
    check_decode(chunks, caps, models, res, 128)
    assert res["status"] == [0] * 64
    # and with the unknown fields of every type, whose skip crosses windows by itself
    wide = dict(R.shape_cases(_compress()))["unknown fields of every type"]
    chunks, caps = [wide] * 64, [R.walk(wide)[2]] * 64
    res = run_decode(pq, chunks, caps, 128, align=list(range(64)))
    check_decode(chunks, caps, models_of(chunks[:1], caps[:1]) * 64, res, 128)


# ---- 3. rejections -----------------------------------------------------------------------------------

def test_every_prefix(pq):
    two = dict(R.shape_cases(_compress()))["two pages"]
    chunks = [two[:n] for n in range(len(two) + 1)]
    models, res = decode_and_check(pq, chunks)
    assert {m.status for m in models} == {0, R.TRUNCATED} and [m.status for m in models].count(0) == 3
    for c, s in enumerate(chunks):  # status, out_len and page count: device, host and reference
        summary = pq.index_column_chunk(s)[0]
        st, pages, total = R.walk(s)
        assert (summary.status, summary.total_length, summary.nchunks) == (st, total, len(pages)) == \
            (res["status"][c], res["length"][c], len(pages))
        assert res["first"][c + 1] - res["first"][c] == (len(pages) if st == 0 else 0)


def test_rejections(pq):
    cases = R.rejection_cases(_compress())
    chunks = [c for _, c in cases]
    models, res = decode_and_check(pq, chunks)
    assert [m.status for m in models] == [R.REJECTION_STATUS[n] for n, _ in cases]
    assert res["length"] == [120] * len(cases) and res["first"][-1] == 0
    for c, s in enumerate(chunks):
        summary = pq.index_column_chunk(s)[0]
        assert (summary.status, summary.total_length, summary.nchunks) == (res["status"][c], res["length"][c], 1)


def test_header_mutations(pq):
    """200 seeded one-byte mutations of header bytes of a fixture chunk: device, host and reference agree"""
    chunk = fixture_chunks("v2.parquet")[4][1]
    pages = R.walk(chunk)[1]
    rng = np.random.default_rng(4321)
    chunks = []
    for _ in range(200):
        p = pages[int(rng.integers(0, len(pages)))]
        at = p.hdr_off + int(rng.integers(0, p.hdr_len))
        mutated = bytearray(chunk)
        mutated[at] ^= int(rng.integers(1, 256))
        chunks.append(bytes(mutated))
    models, res = decode_and_check(pq, chunks)
    assert len({m.status for m in models}) >= 3
    for c, s in enumerate(chunks):
        summary = pq.index_column_chunk(s)[0]
        assert (summary.status, summary.total_length) == (R.walk(s)[0], res["length"][c])
        assert summary.status == res["status"][c] or summary.status == 0


def test_crc_verdicts(pq):
    rec, chunk = fixture_chunks("v1.parquet")[0]
    pages = R.walk(chunk)[1]
    body = pages[1].hdr_off + pages[1].hdr_len
    flipped = bytearray(chunk)
    flipped[body + 1000] ^= 0x10  # one body bit of the second page
    field = bytearray(chunk)
    assert chunk[10] == 0x8E  # the crc field's first varint byte (tests/test_parquet_host.py: the header's bytes)
    field[10] ^= 0x02
    synthetic = R.page_v1(R.payload(1, 200), _compress(), crc=True)
    wrong = R.page_header(0, 200, len(_compress()(R.payload(1, 200))), crc=zlib.crc32(_compress()(R.payload(1, 200))) ^ 1) + \
        _compress()(R.payload(1, 200))
    chunks = [chunk, bytes(flipped), bytes(field), synthetic, wrong]
    models, res = decode_and_check(pq, chunks, verify_crc=True)
    assert res["status"] == [0, R.CRC, R.CRC, 0, R.CRC]
    assert models[1].page_status == [0, R.CRC, 0, 0] and models[2].page_status == [R.CRC, 0, 0, 0]
    # without verification the raw decoder's own status is the page's
    models, res = decode_and_check(pq, chunks, verify_crc=False)
    assert res["status"][0] == res["status"][2] == res["status"][3] == res["status"][4] == 0
    assert res["status"][1] == models[1].status == _status()(bytes(flipped[body:body + pages[1].body_len]))[0]
    good = res["out"][res["offs"][0]:res["offs"][0] + rec["decoded_bytes"]].tobytes()
    assert res["out"][res["offs"][2]:res["offs"][2] + rec["decoded_bytes"]].tobytes() == good
    # a CRC mismatch outranks the decoder's status; under the right crc the decoder's status shows
    outranked = R.page_header(0, 10, len(BAD_COPY), crc=zlib.crc32(BAD_COPY) ^ 5) + BAD_COPY
    honest = R.page_header(0, 10, len(BAD_COPY), crc=zlib.crc32(BAD_COPY)) + BAD_COPY
    models, res = decode_and_check(pq, [outranked, honest, synthetic], verify_crc=True)
    assert res["status"] == [R.CRC, SM_ERR_COPY_OFFSET, 0]
    models, res = decode_and_check(pq, [outranked, honest, synthetic], verify_crc=False)
    assert res["status"] == [SM_ERR_COPY_OFFSET, SM_ERR_COPY_OFFSET, 0]
    # the Python call names the failing chunk
    with pytest.raises(pq.ParquetError) as e:
        pq.uncompress_column_chunks([chunk, bytes(flipped)])
    assert (e.value.code, e.value.chunk) == (R.CRC, 1)
    out, st = pq.uncompress_column_chunks([chunk, bytes(flipped), chunk[:50]], statuses=True)
    assert st == [0, R.CRC, R.TRUNCATED] and out[0][0] == good and out[1][0] is None and out[2][0] is None


# ---- 4. the batch rules ------------------------------------------------------------------------------

def test_batch_of_64(pq):
    """64 chunks mixing good, malformed and too-small capacity: each status is independent and is the
    plan's; the guards around every output range stay; one slot too few refuses the call."""
    good = [c for n in ("v1.parquet", "v2.parquet") for _, c in fixture_chunks(n)] + [c for _, c in R.shape_cases(_compress())]
    bad = [c for _, c in R.rejection_cases(_compress())]
    chunks, caps = [], []
    for i in range(64):
        if i % 3 == 1:
            chunks.append(bad[(i // 3) % len(bad)])
        else:
            chunks.append(good[i % len(good)])
        total = R.walk(chunks[-1])[2]
        caps.append(total - 1 if i % 3 == 2 and total else total)
    models, res = decode_and_check(pq, chunks, caps, spare=5)
    rc, first, out_len, status, pages, frags = pq.chunks_plan(chunks, out_cap=caps)
    assert (rc, first.tolist(), out_len.tolist()) == (0, res["first"], res["length"]) and status.tolist() == res["status"]
    kinds = set(res["status"])
    assert {0, R.SM_BUFFER_TOO_SMALL, R.HEADER, R.TRUNCATED, R.SIZE_MISMATCH} <= kinds
    again = run_decode(pq, chunks, caps, pages, max_fragments=frags, with_pages=False)
    assert again["status"] == res["status"] and (again["out"] == res["out"]).all()
    # one slot too few: nothing is decoded, copied or written
    res = run_decode(pq, chunks, caps, pages - 1)
    assert res["status"] == [ARG] * 64 and res["length"] == [0] * 64 and (res["out"] == GUARD).all()
    assert res["page_status"] == [0] * (pages - 1) and res["first"][-1] == pages


def test_many_pages_in_one_chunk(pq):
    """3,001 pages in one chunk, v1 and stored v2 in turn: more slots than a scan's tile, beside empty chunks"""
    comp = _compress()
    body = b"".join(R.page_v2(b"", b"\x01", bytes([i & 0xFF, 7]), None, is_compressed=False, crc=True) if i % 2 else
                    R.page_v1(bytes([i & 0xFF]) * 3, comp, crc=(i % 4 == 0)) for i in range(3001))
    models, res = decode_and_check(pq, [b"", body, b""], spare=2)
    assert [m.slots for m in models] == [0, 3001, 0] and res["status"] == [0, 0, 0]


# ---- 5. the CRC alone --------------------------------------------------------------------------------

def test_crc32_device(pq):
    torch = _torch()
    lengths = [0, 1, 15, 16, 17, SEGMENT - 1, SEGMENT, SEGMENT + 1, 2 * SEGMENT + 3, (1 << 20) + 5]
    rng = np.random.default_rng(5)
    offs, lens, pos = [], [], 0
    for n in lengths:
        for a in range(16):
            pos += (a - pos) % 16
            offs.append(pos)
            lens.append(n)
            pos += n
    host = rng.integers(0, 256, pos, dtype=np.uint8)  # (ends with the last range's last byte)
    d = torch.from_numpy(host).to(_dev())
    assert d.data_ptr() % 16 == 0
    d_crc = torch.full((len(offs),), 77, dtype=torch.int32, device=_dev())
    pq.crc32_device(d, _i64(offs), _i64(lens), d_crc)
    torch.cuda.synchronize()
    got = (d_crc.cpu().numpy().astype(np.int64) & 0xFFFFFFFF).tolist()
    want = [zlib.crc32(host[o:o + n].tobytes()) for o, n in zip(offs, lens)]
    assert [(n, o % 16) for n, o, g, w in zip(lens, offs, got, want) if g != w] == []
    check = torch.from_numpy(np.frombuffer(b"123456789", np.uint8).copy()).to(_dev())
    one = torch.zeros(1, dtype=torch.int32, device=_dev())
    pq.crc32_device(check, _i64([0]), _i64([9]), one)
    assert int(one.cpu()[0]) & 0xFFFFFFFF == 0xCBF43926


def test_wrapper_on_a_side_stream(pq):
    """the tensor wrapper on a non-default torch stream and a ctx of its own, whose scratch grows between two calls"""
    torch = _torch()
    side = torch.cuda.Stream(device=_dev())
    ctx = ("wrappers", 0, 0)
    for name in ("v1.parquet", "v2.parquet"):
        chunks = [c for _, c in fixture_chunks(name)] * (1 if name == "v1.parquet" else 4)
        caps = [R.walk(c)[2] for c in chunks]
        d_in, in_off, in_len = lay(chunks, lead=5)
        offs = list(np.cumsum([16] + [c + 16 for c in caps[:-1]]))
        d_out = torch.full((sum(c + 16 for c in caps) + 16,), GUARD, dtype=torch.uint8, device=_dev())
        d_ol = torch.full((len(chunks),), -1, dtype=torch.int64, device=_dev())
        d_st = torch.full((len(chunks),), 77, dtype=torch.int32, device=_dev())
        args = [_i64(in_off), _i64(in_len), _i64(offs), _i64(caps)]
        torch.cuda.synchronize()  # (the inputs were made on the default stream)
        frags = pq.chunks_plan(chunks)[5]
        pq.uncompress_column_chunks_device(d_in, args[0], args[1], 40 * len(chunks), frags, d_out, args[2], args[3], d_ol, d_st,
                                           stream=side, device=ctx)
        side.synchronize()
        assert d_st.cpu().tolist() == [0] * len(chunks) and d_ol.cpu().tolist() == caps
        out = d_out.cpu().numpy()
        assert [hashlib.sha256(out[o:o + n].tobytes()).hexdigest() for o, n in zip(offs, caps)] == \
            [r["sha256"] for r, _ in fixture_chunks(name)] * (len(chunks) // len(fixture_chunks(name)))
    assert pq._ctx[ctx] != pq.context(0)
