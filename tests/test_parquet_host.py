"""The Parquet page library's host side on the CPU (snappy.jl_amd/parquet.py over
libsnappy_mi355x_parquet.so): the reference of tests/parquet_ref.py against known answers that do
not come from it (a PageHeader parquet-cpp wrote, the files' own metadata as recorded in the fixture,
zlib's CRC-32), then smq_index, smq_uncompressed_length and smq_chunks_plan against the reference
over every fixture chunk and every synthetic case, the bindings table against the header, and the
sanitizer driver."""
import ctypes
import hashlib
import importlib
import json
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

from prototype_types import assert_device_elements

import parquet_ref as R
from conftest import ROOT

CSRC = os.path.join(ROOT, "snappy.jl_amd", "csrc", "parquet")
GOLDEN = os.path.join(ROOT, "tests", "golden", "parquet")
FILES = ("v1.parquet", "v2.parquet", "bigpage.parquet", "v1_nocrc.parquet")

# the counter column's first PageHeader of v1.parquet: 73 bytes, a v1 data page of 1,024 PLAIN values
PYARROW_HEADER = bytes.fromhex(
    "150015808001159440158eebf49e081c1580101500150615061c1808ff030000000000001808000000000000000016002808ff030000000000"
    "00180800000000000000001111000000")


@pytest.fixture(scope="module")
def pq(sm):
    return importlib.import_module("snappy_jl_amd.parquet")


def fixture_record():
    with open(os.path.join(GOLDEN, "parquet_fixture.json")) as f:
        return json.load(f)


def fixture_chunks(name):
    """[(record, bytes)] of a fixture file's column chunks"""
    with open(os.path.join(GOLDEN, name), "rb") as f:
        data = f.read()
    return [(c, data[c["offset"]:c["offset"] + c["length"]]) for c in fixture_record()["files"][name]["chunks"]]


def synthetic(oracle):
    shapes, rejections = R.shape_cases(oracle.compress), R.rejection_cases(oracle.compress)
    two = dict(shapes)["two pages"]
    prefixes = [("prefix %d" % n, two[:n]) for n in range(len(two))]
    return shapes + rejections + prefixes


def same_as_reference(pq, chunk):
    st, pages, total = R.walk(chunk)
    s, a = pq.index_column_chunk(chunk)
    assert (s.status, s.nchunks, s.total_length) == (st, len(pages), total)
    assert {k: a[k].tolist() for k in pq.INDEX_KEYS} == R.table(pages)
    return st, pages, total


# ---- the reference, pinned ---------------------------------------------------------------------------

def test_reference_known_answers(oracle):
    # the bytes parquet-cpp wrote: its header walks to what pyarrow's metadata says of the page
    st, pages, total = R.walk(PYARROW_HEADER + b"\x80\x40" + bytes(4104))  # (the body: its varint and zeros)
    assert (st, total, len(pages)) == (0, 8192, 1)
    assert pages[0] == R.Page(0, 73, 4106, 8192, 0, 0, 1024, 0, 0, R.HAS_CRC | R.COMPRESSED, 0x41EE9AC7, True)
    assert R.page_header(0, 8192, 4106)[:9] == PYARROW_HEADER[:9]  # the writer writes parquet-cpp's bytes
    assert R.write_struct([(1, R.i32(0)), (2, R.i32(8192)), (3, R.i32(4106)), (4, R.i32(0x41EE9AC7))]) == PYARROW_HEADER[:15] + b"\x00"
    assert zlib.crc32(b"123456789") == 0xCBF43926
    # zigzag and the long form
    assert R.zigzag(0) == b"\x00" and R.zigzag(-1) == b"\x01" and R.zigzag(1) == b"\x02" and R.zigzag(-(1 << 31)) == b"\xff\xff\xff\xff\x0f"
    assert R.write_struct([(300, R.i32(7))]) == b"\x05\xd8\x04\x0e\x00"
    assert R.walk(b"")[0] == 0


def test_reference_cases_are_consistent(oracle):
    for name, chunk in R.shape_cases(oracle.compress):
        st, pages, total = R.walk(chunk)
        assert st == 0, name
        assert all(100 <= p.usize <= 300 for p in pages if p.output) and (pages or name == "the empty chunk"), name
        assert R.decode(chunk, R.oracle_status(oracle)) is not None
    rejections = R.rejection_cases(oracle.compress)
    assert {n for n, _ in rejections} == set(R.REJECTION_STATUS)
    for name, chunk in rejections:
        st, pages, total = R.walk(chunk)
        assert (st, len(pages), total) == (R.REJECTION_STATUS[name], 1, 120), name
    shapes = dict(R.shape_cases(oracle.compress))
    kinds = [p.type for p in R.walk(shapes["an index page between data pages"])[1]]
    assert kinds == [0, 1, 9, 0]
    stored = R.walk(shapes["v2 not compressed"])[1]
    assert [p.flags & R.COMPRESSED for p in stored] == [0, 0] and stored[0].levels == 5
    empty = R.walk(shapes["v2 with an empty values section"])[1]
    assert (empty[0].levels, empty[0].usize, empty[0].flags) == (127, 127, R.HAS_CRC)


# ---- smq_index against the reference -------------------------------------------------------------------

def test_known_answers_through_the_library(pq):
    s, a = pq.index_column_chunk(PYARROW_HEADER + b"\x80\x40" + bytes(4104))
    assert (s.status, s.nchunks, s.total_length) == (0, 1, 8192)
    assert [int(a[k][0]) for k in pq.INDEX_KEYS] == [0, 73, 4106, 8192, 0, 0, 1024, 0, 0, 3, 0x41EE9AC7]
    assert pq.length_uncompressed(PYARROW_HEADER + b"\x80\x40" + bytes(4104)) == 8192
    with pytest.raises(pq.ParquetError) as e:
        pq.length_uncompressed(PYARROW_HEADER)
    assert e.value.code == R.TRUNCATED and e.value.chunk is None and "truncated" in str(e.value)
    s, a = pq.index_column_chunk(b"")
    assert (s.status, s.nchunks, s.total_length) == (0, 0, 0)


@pytest.mark.parametrize("name", FILES)
def test_fixture_chunks(pq, oracle, name):
    """The walk by the library equals the reference's, and both what pyarrow's metadata said of the
    chunk when the fixture was written; the reference's decode has the recorded hash."""
    chunks = fixture_chunks(name)
    assert chunks
    for rec, chunk in chunks:
        st, pages, total = same_as_reference(pq, chunk)
        assert (st, len(pages), total) == (0, rec["pages"], rec["decoded_bytes"]), rec["column"]
        assert [p.type for p in pages] == rec["page_types"]
        assert sum(1 for p in pages if p.flags & R.HAS_CRC) == rec["with_crc"] == (0 if "nocrc" in name or "big" in name else len(pages))
        assert sum(p.levels for p in pages) == rec["levels"] and max(p.usize for p in pages) == rec["largest_page"]
        decoded = R.decode(chunk, R.oracle_status(oracle))
        assert hashlib.sha256(decoded).hexdigest() == rec["sha256"], rec["column"]
        assert pq.length_uncompressed(chunk) == total
    rows = fixture_record()["rows"]
    if name == "v1.parquet":  # a required column has no levels: the chunk is the values themselves
        assert R.decode(chunks[0][1], R.oracle_status(oracle)) == np.arange(rows, dtype="<i8").tobytes()
        assert 2 in chunks[1][0]["page_types"]  # the dictionary page of the label column
    if name == "v2.parquet":
        assert all(t in (2, 3) for c, _ in chunks for t in c["page_types"])
        assert chunks[3][0]["levels"] > 0 and chunks[4][0]["levels"] > chunks[3][0]["levels"]  # definition, and repetition too
    if name == "bigpage.parquet":
        assert chunks[0][0]["largest_page"] > 131072 and chunks[0][0]["pages"] == 1


def test_fixture_decodes_under_libsnappy(libsnappy):
    for name in FILES:
        for rec, chunk in fixture_chunks(name):
            assert hashlib.sha256(R.decode(chunk, R.libsnappy_status(libsnappy))).hexdigest() == rec["sha256"]


def test_every_synthetic_case(pq, oracle):
    seen = set()
    for name, chunk in synthetic(oracle):
        st, pages, total = same_as_reference(pq, chunk)
        seen.add(st)
        if name in R.REJECTION_STATUS:
            assert st == R.REJECTION_STATUS[name], name
        if st == 0:
            assert pq.length_uncompressed(chunk) == total
        else:
            with pytest.raises(pq.ParquetError) as e:
                pq.length_uncompressed(chunk)
            assert e.value.code == st
        if pages:  # one entry too few: the same walk, SM_BUFFER_TOO_SMALL unless it ended in an error
            s, a = pq.index_column_chunk(chunk, max_pages=len(pages) - 1)
            assert (s.status, s.nchunks, s.total_length) == (st or R.SM_BUFFER_TOO_SMALL, len(pages), total)
    assert seen == {0, R.HEADER, R.TRUNCATED, R.SIZE_MISMATCH, R.SM_ERR_VARINT}


def test_header_mutations(pq):
    """200 seeded one-byte mutations of header bytes of a fixture chunk: the library's walk is the reference's"""
    chunk = fixture_chunks("v2.parquet")[4][1]
    pages = R.walk(chunk)[1]
    rng = np.random.default_rng(1234)
    statuses = set()
    for _ in range(200):
        p = pages[int(rng.integers(0, len(pages)))]
        at = p.hdr_off + int(rng.integers(0, p.hdr_len))
        mutated = bytearray(chunk)
        mutated[at] ^= int(rng.integers(1, 256))
        statuses.add(same_as_reference(pq, bytes(mutated))[0])
    assert len(statuses) >= 3


# ---- smq_chunks_plan -------------------------------------------------------------------------------------

def test_plan_back_to_back(pq, oracle):
    cases = synthetic(oracle) + [(rec["column"], chunk) for name in FILES for rec, chunk in fixture_chunks(name)]
    chunks = [c for _, c in cases]
    caps = [R.walk(c)[2] for c in chunks]
    want = R.plan(chunks, caps, 0x7FFFFFFF)
    rc, first, out_len, status, pages, frags = pq.chunks_plan(chunks, out_cap=caps)
    assert (rc, first.tolist(), out_len.tolist(), status.tolist(), pages, frags) == want and pages > 40 and frags >= pages - 10
    # exact, then one too few
    got = pq.chunks_plan(chunks, out_cap=caps, max_pages=pages)
    assert (got[0], got[3].tolist()) == (0, want[3])
    rc, first, out_len, status, total, _ = pq.chunks_plan(chunks, out_cap=caps, max_pages=pages - 1)
    assert (rc, total) == (R.SM_BUFFER_TOO_SMALL, pages)
    assert status.tolist() == [R.SM_ERR_ARGUMENT] * len(chunks) and out_len.tolist() == [0] * len(chunks)
    assert (rc, first.tolist(), out_len.tolist(), status.tolist()) == R.plan(chunks, caps, pages - 1)[:4]
    # a byte short gives its slots up; no cap is no limit
    victim = next(i for i, (n, _) in enumerate(cases) if n == "two pages")
    short = list(caps)
    short[victim] -= 1
    got = pq.chunks_plan(chunks, out_cap=short)
    assert (got[0], got[1].tolist(), got[2].tolist(), got[3].tolist(), got[4], got[5]) == R.plan(chunks, short, 0x7FFFFFFF)
    assert got[3][victim] == R.SM_BUFFER_TOO_SMALL and got[2][victim] == caps[victim] and got[4] == pages - 2
    free = pq.chunks_plan(chunks)
    assert free[3].tolist() == want[3] and free[4] == pages


def test_plan_counts_fragments_of_compressed_sections_only(pq):
    big = fixture_chunks("bigpage.parquet")[0][1]
    want = R.walk(big)[1][0].usize
    stored = R.page_v2(b"", b"", bytes(70000), None, is_compressed=False)
    rc, first, out_len, status, pages, frags = pq.chunks_plan([big, stored, big], out_cap=[want, 70000, want - 1])
    assert (rc, first.tolist(), status.tolist(), pages, frags) == (0, [0, 1, 2, 2], [0, 0, R.SM_BUFFER_TOO_SMALL], 2, -(-want // 65536))
    assert frags == 3


# ---- the size helpers and the texts ----------------------------------------------------------------------

def test_max_pages(pq, oracle):
    assert [pq.max_pages(n) for n in (0, 6, 7, 13, 14, 7000)] == [0, 0, 1, 1, 2, 1000]
    shortest = R.write_struct([(1, R.i32(1)), (2, R.i32(0)), (3, R.i32(0))])
    assert len(shortest) == 7 and R.walk(shortest * 3)[:1] + (len(R.walk(shortest * 3)[1]),) == (0, 3)
    for name, chunk in synthetic(oracle):  # no chunk of the cases holds more
        assert len(R.walk(chunk)[1]) <= pq.max_pages(len(chunk)), name


def test_scratch_bytes(pq):
    f = pq.lib().smq_chunks_scratch_bytes
    assert f(3, 7, 0) > f(3, 6, 0) and f(4, 7, 9) >= f(3, 7, 9) and f(3, 0, 1000) > f(3, 0, 1) and f(0, 0, 0) > 0


def test_status_texts(pq):
    texts = {code: pq.status_message(code) for code in (72, 73, 74, 75)}
    assert len(set(texts.values())) == 4 and all("Parquet column chunk" in t for t in texts.values())
    assert pq.status_message(18) == "Could not decode varint32."  # the main library's
    assert pq.status_message(71) == pq.status_message(76)  # both unused
    assert pq.version().startswith("snappy_mi355x_parquet gfx950 ")
    assert (pq.SMQ_ERR_HEADER, pq.SMQ_ERR_TRUNCATED, pq.SMQ_ERR_SIZE_MISMATCH, pq.SMQ_ERR_CRC) == \
        (R.HEADER, R.TRUNCATED, R.SIZE_MISMATCH, R.CRC) == (72, 73, 74, 75)


def test_status_codes_are_free_in_the_other_headers():
    used = {0: "SM_OK", 1: "SM_INVALID_INPUT", 2: "SM_BUFFER_TOO_SMALL"}
    for header in sorted(os.listdir(os.path.join(ROOT, "include"))):
        text = open(os.path.join(ROOT, "include", header)).read()
        for name, value in re.findall(r"\b(SM\w?_ERR_\w+)\s*=\s*(\d+)", text):
            assert int(value) not in used, (name, used[int(value)])
            used[int(value)] = name
    mine = open(os.path.join(ROOT, "include", "snappy_mi355x_parquet.h")).read()
    assert re.findall(r"(SMQ_ERR_\w+) = (\d+)", mine) == [("SMQ_ERR_HEADER", "72"), ("SMQ_ERR_TRUNCATED", "73"),
                                                         ("SMQ_ERR_SIZE_MISMATCH", "74"), ("SMQ_ERR_CRC", "75")]
    assert {used[v] for v in (72, 73, 74, 75)} == {"SMQ_ERR_HEADER", "SMQ_ERR_TRUNCATED", "SMQ_ERR_SIZE_MISMATCH", "SMQ_ERR_CRC"}


# ---- the bindings ----------------------------------------------------------------------------------------

SCALARS = {"size_t": ctypes.c_size_t, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "int": ctypes.c_int,
           "int32_t": ctypes.c_int32, "sm_status": ctypes.c_int32}


def _declarations():
    with open(os.path.join(ROOT, "include", "snappy_mi355x_parquet.h")) as f:
        src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S))
    out = {}
    for m in re.finditer(r"([\w\s\*]+?)\b(smq_\w+)\s*\(([^;{]*?)\)\s*;", src, re.S):
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
    declared, table = _declarations(), binding.PARQUET
    assert len(declared) == 13 and set(declared) == set(table)
    for name, (ret, params) in declared.items():
        restype, argtypes = binding.prototype(table[name])
        assert len(argtypes) == len(params), name
        assert _class(restype) == _c_class(ret), name
        for k, (t, p) in enumerate(zip(argtypes, params)):
            assert t is not None and _class(t) == _c_class(p), "%s: argument %d (%s)" % (name, k, p.strip())
    assert assert_device_elements(binding, declared, table) == 19  # the pointer parameters of the *_device functions, ctx and stream among them
    assert pq.PARQUET_ABI_SYMBOLS == tuple(table)
    others = [binding.RAW, binding.FRAMING, binding.MULTI, binding.MULTI_RANGE, binding.BLOCKS, binding.ORC]
    assert not set(table) & set().union(*others)  # a group of its own
    header = open(os.path.join(ROOT, "include", "snappy_mi355x_parquet.h")).read()
    struct = re.search(r"typedef struct smq_pages \{(.*?)\} smq_pages;", header, re.S).group(1)
    fields = re.findall(r"\b(u?int\d+_t)\* (\w+);", struct)
    assert [n for n, _ in binding.Pages._fields_] == list(pq.INDEX_KEYS) == [n for _, n in fields] == list(R.TABLE_KEYS)
    assert [np.dtype(pq.PAGE_DTYPES[n]).name + "_t" for _, n in fields] == [t for t, _ in fields]


def test_exported_symbols_are_the_table(pq):
    out = subprocess.run(["nm", "-D", "--defined-only", pq.library_path()], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split() and line.split()[-1].startswith("smq_")}
    assert exported == set(pq.PARQUET_ABI_SYMBOLS)
    for name in pq.PARQUET_ABI_SYMBOLS:
        assert getattr(pq.lib(), name) is not None


def test_library_links_its_companions_by_name(pq):
    out = subprocess.run(["readelf", "-d", pq.library_path()], capture_output=True, text=True).stdout
    assert "libsnappy_mi355x_multi.so" in out and "libsnappy_mi355x.so" in out and "$ORIGIN" in out


def test_importing_loads_no_library():
    import sys
    code = ("import sys; sys.path.insert(0, %r); from conftest import load_package; import importlib; "
            "load_package(); m = importlib.import_module('snappy_jl_amd.parquet'); "
            "assert m._lib is None and m._ctx == {}; "
            "assert 'libsnappy_mi355x' not in open('/proc/self/maps').read()" % os.path.join(ROOT, "tests"))
    subprocess.run([sys.executable, "-c", code], check=True)


def test_not_built_message(pq, monkeypatch, tmp_path):
    monkeypatch.setattr(pq, "_lib", None)
    monkeypatch.setattr(pq, "LIB_PATH", str(tmp_path / "libsnappy_mi355x_parquet.so"))
    with pytest.raises(OSError) as e:
        pq.lib()
    assert str(e.value) == "libsnappy_mi355x_parquet.so not built (run __graft_entry__.build())"


# ---- the sanitizer driver --------------------------------------------------------------------------------

def test_host_check_runs_clean(tmp_path):
    r = subprocess.run(["make", "-C", CSRC, "host_check", "OBJ=%s" % tmp_path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "smq_host_check ok" in r.stdout
    src = open(os.path.join(CSRC, "smq_host_check.cpp")).read()
    assert "smq_chunks_plan" in src and "smq_index" in src and "crc32_model" in src and "int main()" in src
