"""The Parquet page encoder's host side on the CPU (snappy.jl_amd/parquet.py over
libsnappy_mi355x_parquet.so, include/snappy_mi355x_parquet_write.h): the bindings table against the
header, smqe_rewrite_header, smqe_index and smqe_chunks_plan against the plain-Python reference of
tests/parquet_write_ref.py over every fixture chunk, every synthetic case and seeded mutations, the
reference transcoder judged by pyarrow, and the sanitizer driver."""
import ctypes
import hashlib
import importlib
import io
import json
import os
import re
import subprocess

import numpy as np
import pytest

from prototype_types import assert_device_elements

import parquet_ref as R
import parquet_write_ref as W
from conftest import ROOT

CSRC = os.path.join(ROOT, "snappy.jl_amd", "csrc", "parquet")
GOLDEN = os.path.join(ROOT, "tests", "golden", "parquet_write")
FILES = ("v1.parquet", "v2.parquet", "bigpage.parquet", "v1_nocrc.parquet")
HEADER = "snappy_mi355x_parquet_write.h"
SM_ERR_INPUT_TOO_LARGE = 16

BODY_LENGTHS = (0, 63, 64, 8191, 8192, 1048575, 1048576, 0x7FFFFFFF)  # zigzag varints of 1, 1, 2, 2, 3, 3, 4 and 5 bytes
CRCS = (0, 31, 0xFFFFFFE0, 32, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF)     # as i32: 0, 31, -32, 32, max, min, -1


@pytest.fixture(scope="module")
def pq(sm):
    return importlib.import_module("snappy_jl_amd.parquet")


def fixture_record():
    with open(os.path.join(GOLDEN, "parquet_write_fixture.json")) as f:
        return json.load(f)


def fixture_chunks(name):
    """[(record, bytes)] of a fixture file's column chunks, in their plain form"""
    with open(os.path.join(GOLDEN, name), "rb") as f:
        data = f.read()
    return [(c, data[c["offset"]:c["offset"] + c["length"]]) for c in fixture_record()["files"][name]["chunks"]]


def same_as_reference(pq, chunk):
    st, pages, sites, total = W.walk(chunk)
    s, a, got_sites = pq.index_plain_column_chunk(chunk)
    assert (s.status, s.nchunks, s.total_length) == (st, len(pages), total)
    assert {k: a[k].tolist() for k in pq.INDEX_KEYS} == R.table(pages)
    assert got_sites.tolist() == [list(x) for x in sites]
    return st, pages, sites, total


def mutants(count=200, seed=20250301):
    """seeded one-byte mutations of header bytes of a fixture chunk (v2, with levels and crcs)"""
    chunk = fixture_chunks("v2.parquet")[4][1]
    pages = W.walk(chunk)[1]
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        p = pages[int(rng.integers(0, len(pages)))]
        at = p.hdr_off + int(rng.integers(0, p.hdr_len))
        mutated = bytearray(chunk)
        mutated[at] ^= int(rng.integers(1, 256))
        out.append(bytes(mutated))
    return out


# ---- the bindings ----------------------------------------------------------------------------------------

SCALARS = {"size_t": ctypes.c_size_t, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "int": ctypes.c_int,
           "int32_t": ctypes.c_int32, "sm_status": ctypes.c_int32}


def _declarations():
    with open(os.path.join(ROOT, "include", HEADER)) as f:
        src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S))
    src = re.sub(r"^[ \t]*#[^\n]*", "", src, flags=re.M)  # (the preprocessor's lines)
    out = {}
    for m in re.finditer(r"([\w\s\*]+?)\b(smqe_\w+)\s*\(([^;{]*?)\)\s*;", src, re.S):
        params = m.group(3).strip()
        types = [] if params in ("", "void") else [re.sub(r"\w+$", "", p.strip()) for p in params.split(",")]
        assert m.group(2) not in out
        out[m.group(2)] = (m.group(1), types)
    return out


def _class(ctype):
    if ctype is None:
        return None
    if ctype in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(ctype, ctypes._Pointer):
        return ("pointer",)
    return (ctypes.sizeof(ctype), ctype(-1).value < 0)


def _c_class(decl):
    words = decl.replace("const", " ").split()
    if "*" in decl:
        return ("pointer",)
    if words == ["void"]:
        return None
    assert len(words) == 1 and words[0] in SCALARS, decl
    return _class(SCALARS[words[0]])


def test_table_matches_the_header(sm, pq):
    binding = importlib.import_module("snappy_jl_amd._binding")
    declared, table = _declarations(), binding.PARQUET_WRITE
    assert len(declared) == 8 and set(declared) == set(table)
    for name, (ret, params) in declared.items():
        restype, argtypes = binding.prototype(table[name])
        assert len(argtypes) == len(params), name
        assert _class(restype) == _c_class(ret), name
        for k, (t, p) in enumerate(zip(argtypes, params)):
            assert t is not None and _class(t) == _c_class(p), "%s: argument %d (%s)" % (name, k, p.strip())
    assert assert_device_elements(binding, declared, table) == 13  # the pointer parameters of the *_device functions, ctx and stream among them
    assert pq.PARQUET_WRITE_ABI_SYMBOLS == tuple(table)
    others = [binding.RAW, binding.FRAMING, binding.MULTI, binding.MULTI_RANGE, binding.BLOCKS, binding.ORC, binding.PARQUET]
    assert not set(table) & set().union(*others)  # a group of its own
    assert not any(re.match(r"smq_\w", name) for name in table)  # and no name the decoder's table would claim
    header = open(os.path.join(ROOT, "include", HEADER)).read()
    assert int(re.search(r"#define SMQE_SITES (\d+)", header).group(1)) == len(pq.SITE_KEYS) == len(W.SITE_KEYS)
    assert pq.SITE_KEYS == W.SITE_KEYS


def test_exported_symbols(pq):
    out = subprocess.run(["nm", "-D", "--defined-only", pq.library_path()], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.split()}
    assert {n for n in names if n.startswith("smqe_")} == set(pq.PARQUET_WRITE_ABI_SYMBOLS)
    assert {n for n in names if n.startswith("smq_")} == set(pq.PARQUET_ABI_SYMBOLS)  # the decoder's exports: unchanged
    for name in pq.PARQUET_WRITE_ABI_SYMBOLS:
        assert getattr(pq.lib(), name) is not None


# ---- the rewrite rule ----------------------------------------------------------------------------------------

def rewrite_both(pq, header, n, crc):
    st, want = W.rewrite_header(header, n, crc)
    if st:
        with pytest.raises(pq.ParquetError) as e:
            pq.rewrite_page_header(header, n, crc)
        assert e.value.code == st
        return None
    got = pq.rewrite_page_header(header, n, crc)
    assert got == want
    return got


def header_shapes():
    H = R.page_header
    unknown = [(20, (R.T_TRUE, None)), (27, (R.T_BINARY, b"some bytes")), (300, (R.T_I32, 7))]
    between = [(3, (R.T_I64, 99), True)]  # field 3 under another type, behind the real one: skipped, not patched
    shapes = [
        ("v1 with crc", H(R.DATA_PAGE, 8192, 8192, crc=0x41EE9AC7)),
        ("v1 without crc", H(R.DATA_PAGE, 8192, 8192)),
        ("dictionary", H(R.DICTIONARY_PAGE, 100, 100, crc=5)),
        ("index page", H(R.INDEX_PAGE, 10, 10, crc=1)),
        ("v2 compressed true", H(R.DATA_PAGE_V2, 300, 300, crc=7, def_len=3, rep_len=2, is_compressed=True)),
        ("v2 compressed false", H(R.DATA_PAGE_V2, 300, 300, crc=7, def_len=3, rep_len=2, is_compressed=False)),
        ("v2 compressed missing", H(R.DATA_PAGE_V2, 300, 300, crc=7, def_len=3, rep_len=2)),
        ("v2 false without crc", H(R.DATA_PAGE_V2, 300, 300, is_compressed=False)),
        ("long ids", H(R.DATA_PAGE, 100, 100, crc=0xFFFFFFFF, long_ids=True)),
        ("v2 long ids", H(R.DATA_PAGE_V2, 100, 100, crc=9, long_ids=True, is_compressed=False)),
        ("unknown fields before, between and after", H(R.DATA_PAGE, 100, 100, crc=3, extra=unknown + between + [(0, (R.T_I32, 4), True)])),
        ("unknown fields of every type", H(R.DATA_PAGE, 100, 100, crc=3, extra=R.UNKNOWN_EVERY_TYPE, sub_extra=R.UNKNOWN_EVERY_TYPE)),
        ("statistics", H(R.DATA_PAGE, 100, 100, crc=1 << 31, sub_extra=[R.STATS_300])),
        ("v2 statistics", H(R.DATA_PAGE_V2, 100, 100, crc=2, is_compressed=False, sub_extra=[(8, R.STATS_300[1])])),
        ("crc before the size", R.write_struct([(1, R.i32(0)), (2, R.i32(60)), (4, R.i32(-77), True), (3, R.i32(60), True),
                                                (5, (R.T_STRUCT, [(1, R.i32(5)), (2, R.i32(0))]))])),
        ("five-byte size", H(R.DATA_PAGE, 0x7FFFFFFF, 0x7FFFFFFF, crc=0x80000000)),
    ]
    return shapes


def test_rewrite_rule_on_every_shape(pq):
    lengths = {1: set(), 2: set()}  # the varints' lengths seen, old -> new
    for name, header in header_shapes():
        site = W.sites_of(W.read_header(R.Reader(header, 0))[1], 0)
        for n in BODY_LENGTHS:
            for crc in CRCS:
                got = rewrite_both(pq, header + b"behind the header", n, crc)
                assert got is not None, name
                # what an independent reader takes from it: the decode walk's header fields
                h = R.read_header(R.Reader(got + bytes(8), 0))
                assert h["csize"] == n and (h["crc"] & 0xFFFFFFFF == crc if site[3] else 4 not in h["seen"]), name
                assert h["is_compressed"] is True and h["usize"] == R.read_header(R.Reader(header, 0))["usize"]
                lengths[1].add((site[1], len(R.zigzag(n))))
                lengths[2].add((site[3], len(R.zigzag(W.as_i32(crc))) if site[3] else 0))
                # a byte short
                out = np.zeros(len(got) - 1, np.uint8)
                size = ctypes.c_size_t(0)
                rc = pq.lib().smqe_rewrite_header(header, len(header), n, crc, out.ctypes.data, out.size, ctypes.byref(size))
                assert (rc, size.value) == (R.SM_BUFFER_TOO_SMALL, len(got)) and not out.any(), name
    assert {new for _, new in lengths[1]} == {1, 2, 3, 4, 5} and {old for old, _ in lengths[1]} >= {1, 2, 5}
    assert {new for old, new in lengths[2] if old} == {1, 5} and {old for old, _ in lengths[2]} >= {0, 1, 5}
    # both varints of every length from 1 to 5, growing and shrinking, around three-byte ones
    header = R.page_header(R.DATA_PAGE, 100000, 100000, crc=100000)
    crcs = (0, 64, 8192, 1048576, 0xFFFFFFFF - 1048576, 0x80000000)
    assert {len(R.zigzag(W.as_i32(c))) for c in crcs} == {1, 2, 3, 4, 5}
    for n in (0, 64, 8192, 1048576, 0x7FFFFFFF):
        for crc in crcs:
            assert rewrite_both(pq, header, n, crc) is not None


def test_rewrite_rule_rejections(pq):
    good = R.page_header(R.DATA_PAGE, 100, 100, crc=1)
    assert rewrite_both(pq, good, 0x80000000, 0) is None  # SM_ERR_INPUT_TOO_LARGE
    assert W.rewrite_header(good, 0x80000000, 0)[0] == SM_ERR_INPUT_TOO_LARGE
    for name, chunk, status in W.rejection_cases():
        if "twice" in name or name in ("field 3 missing", "field 2 not an i32", "negative size", "i32 varint of 6 bytes"):
            bad = chunk[len(W.plain_page_v1(R.payload(20, 120), crc=True)):]
            assert W.rewrite_header(bad, 5, 5)[0] == status, name
            assert rewrite_both(pq, bad, 5, 5) is None, name
    for cut in range(len(good)):
        assert W.rewrite_header(good[:cut], 5, 5)[0] == R.TRUNCATED
        assert rewrite_both(pq, good[:cut], 5, 5) is None


def test_rewrite_rule_on_every_fixture_header(pq):
    count = 0
    for name in FILES:
        for rec, chunk in fixture_chunks(name):
            for k, p in enumerate(W.walk(chunk)[1]):
                header = chunk[p.hdr_off:p.hdr_off + p.hdr_len]
                for n, crc in ((0, 0), (p.body_len // 2, 0xDEADBEEF), (p.body_len, p.crc), (0x7FFFFFFF, 0xFFFFFFFF)):
                    assert rewrite_both(pq, header, n, crc) is not None
                assert pq.rewrite_page_header(header, p.body_len, p.crc) == header or p.type == R.DATA_PAGE_V2
                count += 1
    assert count == sum(c["pages"] for f in fixture_record()["files"].values() for c in f["chunks"]) == 37


# ---- smqe_index and smqe_chunks_plan against the reference ------------------------------------------------------

@pytest.mark.parametrize("name", FILES)
def test_fixture_chunks(pq, name):
    """The encode walk by the library equals the reference's, and both what the recipe recorded."""
    chunks = fixture_chunks(name)
    assert chunks
    for rec, chunk in chunks:
        st, pages, sites, total = same_as_reference(pq, chunk)
        assert (st, len(pages)) == (0, rec["pages"]) and [p.type for p in pages] == rec["page_types"], rec["column"]
        assert [p.levels for p in pages] == rec["levels"] and max(p.usize for p in pages) == rec["largest_page"]
        assert sum(1 for p in pages if p.flags & R.HAS_CRC) == rec["with_crc"] == (0 if "nocrc" in name or "big" in name else len(pages))
        assert all(p.body_len == p.usize for p in pages)
        bodies = b"".join(chunk[p.hdr_off + p.hdr_len:p.hdr_off + p.hdr_len + p.body_len] for p in pages)
        assert hashlib.sha256(bodies).hexdigest() == rec["sha256"], rec["column"]
        assert all((s[3] != 0) == bool(p.flags & R.HAS_CRC) and s[1] >= 1 for s, p in zip(sites, pages))
        assert all((s[4] != 0) == (p.type == R.DATA_PAGE_V2) for s, p in zip(sites, pages))  # parquet-cpp writes is_compressed
    assert fixture_record()["files"][name]["file_bytes"] <= 300000


def test_every_synthetic_case(pq):
    seen = set()
    two = dict(W.shape_cases())["a dictionary page"]
    cases = [(n, c, 0) for n, c in W.shape_cases()] + W.rejection_cases() + [("prefix %d" % n, two[:n], None) for n in range(len(two))]
    for name, chunk, status in cases:
        st, pages, sites, total = same_as_reference(pq, chunk)
        seen.add(st)
        if status is not None:
            assert st == status, name
        if status:
            assert (len(pages), total) == (1, 120), name
        if pages:  # one entry too few: the same walk, SM_BUFFER_TOO_SMALL unless it ended in an error
            s, a, _ = pq.index_plain_column_chunk(chunk, max_pages=len(pages) - 1)
            assert (s.status, s.nchunks, s.total_length) == (st or R.SM_BUFFER_TOO_SMALL, len(pages), total)
    assert seen == {0, R.HEADER, R.TRUNCATED, R.SIZE_MISMATCH}
    # the decode walk's "the last counts" stays what it is: a repeated field 3 decodes
    dup3 = R.write_struct([(1, R.i32(R.INDEX_PAGE)), (2, R.i32(0)), (3, R.i32(5)), (3, R.i32(0), True)])
    assert pq.index_column_chunk(dup3)[0].status == R.walk(dup3)[0] == 0 and W.walk(dup3)[0] == R.HEADER
    assert pq.index_plain_column_chunk(dup3)[0].status == R.HEADER


def test_header_mutations(pq):
    """200 seeded one-byte mutations of header bytes of a fixture chunk: status, page count and patch
    sites are the reference's; the reference alone accepts and rejects enough of them for both sides
    of the rule to be tested."""
    accepted = rejected = 0
    for m in mutants():
        st = W.walk(m)[0]
        accepted += st == 0
        rejected += st != 0
    assert accepted >= 20 and rejected >= 20, (accepted, rejected)
    statuses = {same_as_reference(pq, m)[0] for m in mutants()}
    assert len(statuses) >= 3


def test_plan(pq):
    cases = [(n, c) for n, c in W.shape_cases()] + [(n, c) for n, c, _ in W.rejection_cases()] + \
        [(rec["column"], chunk) for name in FILES for rec, chunk in fixture_chunks(name)]
    chunks = [c for _, c in cases]
    want = W.plan(chunks, 0x7FFFFFFF)
    rc, first, status, bound, pages, stage, frags = pq.compress_chunks_plan(chunks)
    assert (rc, first.tolist(), status.tolist(), bound.tolist(), pages, stage, frags) == want
    assert pages > 50 and frags == 3 and stage > sum(len(c) for c in chunks)  # (bigpage's 187,201 bytes: 3 fragments)
    assert pq.compress_chunks_plan(chunks, max_pages=pages)[0] == 0
    rc, first, status, bound, total, _, _ = pq.compress_chunks_plan(chunks, max_pages=pages - 1)
    assert (rc, total) == (R.SM_BUFFER_TOO_SMALL, pages)
    assert status.tolist() == [R.SM_ERR_ARGUMENT] * len(chunks) and bound.tolist() == [0] * len(chunks)
    assert (rc, first.tolist(), status.tolist(), bound.tolist()) == W.plan(chunks, pages - 1)[:4]
    # the bounds hold: of the reference transcoder over a compressor that only ever grows its input
    def grow(b):
        return R.varint(len(b)) + b"".join(bytes([0xFC]) + b[i:i + 60] for i in range(0, len(b), 60))
    for chunk, st, b in zip(chunks, want[2], want[3]):
        if st == 0:
            out = W.transcode(chunk, grow)[1]
            npages = len(W.walk(chunk)[1])
            assert len(out) <= b <= pq.max_compressed_chunk_length(len(chunk), npages)
    assert stage <= pq.lib().smqe_stage_bound(sum(len(c) for c in chunks), pages)


def test_scratch_bytes(pq):
    f = pq.lib().smqe_scratch_bytes
    assert f(3, 7, 1000) > f(3, 6, 1000) and f(4, 7, 1000) >= f(3, 7, 1000) and f(3, 7, 2000) >= f(3, 7, 1000) + 992 and f(0, 0, 0) > 0


# ---- the rig, judged by an independent reader -------------------------------------------------------------------

def test_reference_transcoder_reads_back_under_pyarrow(pq, oracle):
    """The reference transcoder over the CPU oracle's compressor, spliced into the files: pyarrow
    reads the recipe's tables back with page checksum verification on, and refuses a flipped byte."""
    pytest.importorskip("pyarrow")
    import pyarrow.parquet as pap
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_parquet_fixture import FILES as RECIPES
    for name in FILES:
        with open(os.path.join(GOLDEN, name), "rb") as f:
            data = f.read()
        new = W.splice_file(data, oracle.compress)
        make, args = RECIPES[name]
        assert pap.read_table(io.BytesIO(new), page_checksum_verification=True).equals(make()), name
        assert pap.ParquetFile(io.BytesIO(new)).metadata.row_group(0).column(0).compression == "SNAPPY"
        for rec, chunk in fixture_chunks(name):  # and every transcoded chunk passes this library's decode walk
            out = W.transcode(chunk, oracle.compress)[1]
            assert len(out) <= pq.compress_chunks_plan([chunk])[3][0]  # (the plan's room suffices)
            st, pages, total = R.walk(out)
            assert st == 0 and total == sum(p.usize for p in W.walk(chunk)[1])
            assert R.decode(out, R.oracle_status(oracle)) == b"".join(
                chunk[p.hdr_off + p.hdr_len:p.hdr_off + p.hdr_len + p.body_len] for p in W.walk(chunk)[1])
        if args.get("write_page_checksum"):
            first = fixture_record()["files"][name]["chunks"][0]
            bad = bytearray(new)
            bad[first["offset"] + 100] ^= 1  # a body byte of the first page
            with pytest.raises(Exception, match="CRC"):
                pap.read_table(io.BytesIO(bytes(bad)), page_checksum_verification=True)


# ---- the sanitizer driver -------------------------------------------------------------------------------------

def test_host_check_covers_the_encoder(tmp_path):
    r = subprocess.run(["make", "-C", CSRC, "host_check", "OBJ=%s" % tmp_path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "smq_host_check ok" in r.stdout
    src = open(os.path.join(CSRC, "smq_host_check.cpp")).read()
    assert "smqe_rewrite_header" in src and "smqe_index" in src and "smqe_chunks_plan" in src
