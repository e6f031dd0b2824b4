"""The ORC library's host side on the CPU (snappy.jl_amd/orc.py over libsnappy_mi355x_orc.so): the
reference of tests/orc_ref.py against known answers that do not come from it (the ORC
specification's example headers), then smo_index, smo_uncompressed_length and smo_streams_plan
against the reference over every structural case, the size helpers, the bindings table against the
header, the sanitizer driver, and the two files an independent writer made (tests/golden/orc/)."""
import ctypes
import hashlib
import importlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

from prototype_types import assert_device_elements

import orc_ref as R
from conftest import ROOT

CSRC = os.path.join(ROOT, "snappy.jl_amd", "csrc", "orc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "orc")
B = R.CASE_BLOCK
CASES = R.structural_cases()


@pytest.fixture(scope="module")
def orc(sm):
    return importlib.import_module("snappy_jl_amd.orc")


# ---- the reference, pinned ---------------------------------------------------------------------------

def test_reference_known_answers(oracle):
    assert R.header(100000, False) == bytes.fromhex("400d03")  # the specification's two examples
    assert R.header(5, True) == bytes.fromhex("0b0000")
    assert oracle.compress(b"abc") == bytes.fromhex("0308616263") == R.ABC
    # the raw stream of "abc" has 5 bytes, not fewer than 3: the piece is stored
    assert R.encode(b"abc", 262144, oracle.compress) == bytes.fromhex("070000616263")
    assert R.encode(b"", 262144, oracle.compress) == b""
    zeros = R.encode(bytes(100), 64, oracle.compress)
    st, chunks, total = R.walk(zeros, 64)
    assert (st, total, [(c.ulen, c.original) for c in chunks]) == (0, 100, [(64, 0), (36, 0)])
    for bs in (1, 64, 70000):
        for data in (b"", b"abc", bytes(range(256)) * 300, bytes(1000)):
            enc = R.encode(data, bs, oracle.compress)
            assert R.decode(enc, bs, R.oracle_status(oracle)) == data and len(enc) <= R.max_length(len(data), bs)
    assert R.walk(b"", 0)[0] == R.walk(b"", 0x800000)[0] == R.SM_ERR_ARGUMENT


def test_reference_cases_are_consistent():
    names = set()
    for name, stream, status, nchunks, total in CASES:
        assert name not in names
        names.add(name)
        st, chunks, tot = R.walk(stream, B)
        assert (st, len(chunks), tot) == (status, nchunks, total), name
    assert {c[2] for c in CASES} == {0, R.SM_ERR_VARINT, R.TRUNCATED, R.CHUNK_TOO_LARGE}


# ---- smo_index -------------------------------------------------------------------------------------------

def test_known_answers_through_the_library(orc):
    for text, pay_len, original in (("070000616263", 3, 1), ("0a00000308616263", 5, 0)):
        s, a = orc.index_chunks(bytes.fromhex(text), 262144)
        assert (s.status, s.nchunks, s.total_length) == (0, 1, 3)
        assert (a["pay_off"].tolist(), a["pay_len"].tolist(), a["ulen"].tolist(), a["original"].tolist()) == \
            ([3], [pay_len], [3], [original])
        rc, first, out_len, status, chunks, frags = orc.streams_plan([bytes.fromhex(text)], 262144)
        assert (rc, first.tolist(), out_len.tolist(), status.tolist(), chunks, frags) == (0, [0, 1], [3], [0], 1, 1 - original)
    s, a = orc.index_chunks(b"", 262144)
    assert (s.status, s.nchunks, s.total_length) == (0, 0, 0)
    # a chunk compressed to 100,000 bytes under the specification's header: its structure alone
    big = bytes.fromhex("400d03") + R.varint(262144) + bytes(100000 - 3)
    s, a = orc.index_chunks(big, 262144)
    assert (s.status, s.nchunks, s.total_length, a["pay_len"].tolist()) == (0, 1, 262144, [100000])
    assert orc.length_uncompressed(bytes.fromhex("0b0000") + b"hello", 5) == 5
    with pytest.raises(orc.OrcError) as e:
        orc.length_uncompressed(bytes.fromhex("0b0000") + b"hello", 4)
    assert e.value.code == R.CHUNK_TOO_LARGE and e.value.stream is None and "block size" in str(e.value)


@pytest.mark.parametrize("case", range(len(CASES)), ids=lambda i: CASES[i][0].replace(" ", "-"))
def test_every_walk_status(orc, case):
    name, stream, status, nchunks, total = CASES[case]
    s, a = orc.index_chunks(stream, B)
    assert (s.status, s.nchunks, s.total_length) == (status, nchunks, total)
    chunks = R.walk(stream, B)[1]
    assert a["pay_off"].tolist() == [c.pay_off for c in chunks]
    assert a["pay_len"].tolist() == [c.pay_len for c in chunks] and a["ulen"].tolist() == [c.ulen for c in chunks]
    assert a["original"].tolist() == [c.original for c in chunks]
    if status == 0:
        assert orc.length_uncompressed(stream, B) == total
    else:
        with pytest.raises(orc.OrcError) as e:
            orc.length_uncompressed(stream, B)
        assert e.value.code == status
    if nchunks:  # one entry too few: the same walk, SM_BUFFER_TOO_SMALL unless it ended in an error
        s, a = orc.index_chunks(stream, B, max_chunks=nchunks - 1)
        assert (s.status, s.nchunks, s.total_length) == (status or R.SM_BUFFER_TOO_SMALL, nchunks, total)


@pytest.mark.parametrize("block_size", [0, 0x800000])
def test_block_size_out_of_range(orc, block_size):
    stream = R.stored(b"abc")
    s, a = orc.index_chunks(stream, block_size)
    assert (s.status, s.nchunks) == (R.SM_ERR_ARGUMENT, 0) == (R.walk(stream, block_size)[0], 0)
    with pytest.raises(orc.OrcError) as e:
        orc.length_uncompressed(stream, block_size)
    assert e.value.code == R.SM_ERR_ARGUMENT
    assert orc.streams_plan([stream], block_size)[0] == R.SM_ERR_ARGUMENT
    assert orc.lib().smo_max_length(10, block_size) == 0
    with pytest.raises(ValueError):
        orc.max_length(10, block_size)
    with pytest.raises(ValueError):
        orc.compress_orc_streams([b"abc"], block_size)
    with pytest.raises(ValueError):
        orc.uncompress_orc_streams([stream], block_size)
    assert orc.index_chunks(stream, 0x7FFFFF)[0].status == 0 and orc.index_chunks(stream, 3)[0].status == 0
    assert orc.index_chunks(stream, 2)[0].status == R.CHUNK_TOO_LARGE


def test_status_texts(orc):
    texts = {code: orc.status_message(code) for code in (64, 65)}
    assert len(set(texts.values())) == 2 and all("ORC stream" in t for t in texts.values())
    assert orc.status_message(18) == "Could not decode varint32."  # the main library's
    assert orc.status_message(63) == orc.status_message(66)  # both unused
    assert orc.version().startswith("snappy_mi355x_orc gfx950 ")
    assert (orc.SMO_ERR_TRUNCATED, orc.SMO_ERR_CHUNK_TOO_LARGE) == (R.TRUNCATED, R.CHUNK_TOO_LARGE) == (64, 65)


def test_status_codes_are_free_in_the_other_headers():
    for header in ("snappy_mi355x.h", "snappy_mi355x_framing.h", "snappy_mi355x_multi.h", "snappy_mi355x_multi_range.h",
                   "snappy_mi355x_blocks.h"):
        text = open(os.path.join(ROOT, "include", header)).read()
        assert not re.search(r"=\s*6[3-6]\b", text), header
    mine = open(os.path.join(ROOT, "include", "snappy_mi355x_orc.h")).read()
    assert re.findall(r"(SMO_ERR_\w+) = (\d+)", mine) == [("SMO_ERR_TRUNCATED", "64"), ("SMO_ERR_CHUNK_TOO_LARGE", "65")]


# ---- smo_streams_plan ------------------------------------------------------------------------------------

def test_plan_back_to_back(orc):
    streams = [c[1] for c in CASES]
    caps = [c[4] for c in CASES]
    want = R.plan(streams, B, caps, 0x7FFFFFFF)
    rc, first, out_len, status, chunks, frags = orc.streams_plan(streams, B, out_cap=caps)
    assert (rc, first.tolist(), out_len.tolist(), status.tolist(), chunks, frags) == want and chunks > 5
    assert status.tolist() == [c[2] for c in CASES]
    # exact, then one too few
    got = orc.streams_plan(streams, B, out_cap=caps, max_chunks=chunks)
    assert (got[0], got[3].tolist()) == (0, want[3])
    rc, first, out_len, status, total, _ = orc.streams_plan(streams, B, out_cap=caps, max_chunks=chunks - 1)
    assert (rc, total) == (R.SM_BUFFER_TOO_SMALL, chunks)
    assert status.tolist() == [R.SM_ERR_ARGUMENT] * len(streams) and out_len.tolist() == [0] * len(streams)
    assert (rc, first.tolist(), out_len.tolist(), status.tolist()) == R.plan(streams, B, caps, chunks - 1)[:4]
    # a byte short gives its slots up; no cap is no limit
    victim = next(i for i, c in enumerate(CASES) if c[2] == 0 and c[3] == 3)
    short = list(caps)
    short[victim] -= 1
    got = orc.streams_plan(streams, B, out_cap=short)
    assert (got[0], got[1].tolist(), got[2].tolist(), got[3].tolist(), got[4], got[5]) == R.plan(streams, B, short, 0x7FFFFFFF)
    assert got[3][victim] == R.SM_BUFFER_TOO_SMALL and got[2][victim] == caps[victim] and got[4] == chunks - 3
    free = orc.streams_plan(streams, B)
    assert free[3].tolist() == want[3] and free[4] == chunks


def test_plan_counts_fragments_of_compressed_chunks_only(orc):
    big = R.compressed(R.varint(200000))  # (structure only)
    raw = R.stored(bytes(70000))
    rc, first, out_len, status, chunks, frags = orc.streams_plan([R.compressed(R.ABC), big, big, raw], 262144,
                                                                 out_cap=[3, 200000, 199999, 70000])
    assert (rc, first.tolist(), status.tolist(), chunks, frags) == (0, [0, 1, 2, 2, 3], [0, 0, R.SM_BUFFER_TOO_SMALL, 0], 3, 5)


# ---- the size helpers ------------------------------------------------------------------------------------

@pytest.mark.parametrize("block_size", [1, 64, 65536, 0x7FFFFF])
def test_max_length(orc, oracle, block_size):
    for n in (0, 1, block_size - 1, block_size, block_size + 1, 2 * block_size, 2 * block_size + 1):
        if n > 200000:
            assert orc.max_length(n, block_size) == R.max_length(n, block_size)
            continue
        data = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8).tobytes()
        want = R.max_length(n, block_size)
        assert orc.max_length(n, block_size) == want
        written = R.encode(data, block_size, oracle.compress)
        assert len(written) == want  # random pieces are stored: the bound is met exactly
        assert len(R.encode(bytes(n), block_size, oracle.compress)) <= want
    assert orc.max_length(0, block_size) == 0 and orc.max_length(1, block_size) == 4


def test_max_chunks(orc):
    assert [orc.max_chunks(n) for n in (0, 2, 3, 5, 6, 3000)] == [0, 0, 1, 1, 2, 1000]
    for c in CASES:  # no stream of the cases holds more
        assert c[3] <= orc.max_chunks(len(c[1])), c[0]


def test_scratch_bytes(orc):
    f = orc.lib().smo_streams_scratch_bytes
    assert f(3, 7, 0, B) > f(3, 6, 0, B) and f(4, 7, 9, B) >= f(3, 7, 9, B) and f(3, 0, 1000, B) > f(3, 0, 1, B)
    assert f(0, 0, 0, B) > 0
    assert f(1, 10, 0, 262144) >= 10 * 305920  # the compress call's slots: 32 + n + n / 6, rounded up to 256


# ---- the bindings ----------------------------------------------------------------------------------------

SCALARS = {"size_t": ctypes.c_size_t, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "int": ctypes.c_int,
           "int32_t": ctypes.c_int32, "sm_status": ctypes.c_int32}


def _declarations():
    with open(os.path.join(ROOT, "include", "snappy_mi355x_orc.h")) as f:
        src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S))
    out = {}
    for m in re.finditer(r"([\w\s\*]+?)\b(smo_\w+)\s*\(([^;{]*?)\)\s*;", src, re.S):
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


def test_table_matches_the_header(sm, orc):
    binding = importlib.import_module("snappy_jl_amd._binding")
    declared, table = _declarations(), binding.ORC
    assert len(declared) == 15 and set(declared) == set(table)
    for name, (ret, params) in declared.items():
        restype, argtypes = binding.prototype(table[name])
        assert len(argtypes) == len(params), name
        assert _class(restype) == _c_class(ret), name
        for k, (t, p) in enumerate(zip(argtypes, params)):
            assert t is not None and _class(t) == _c_class(p), "%s: argument %d (%s)" % (name, k, p.strip())
    assert assert_device_elements(binding, declared, table) == 21  # the pointer parameters of the *_device functions, ctx and stream among them
    assert orc.ORC_ABI_SYMBOLS == tuple(table)
    others = [binding.RAW, binding.FRAMING, binding.MULTI, binding.MULTI_RANGE, binding.BLOCKS]
    assert not set(table) & set().union(*others)  # a group of its own
    assert [n for n, _ in binding.OrcChunks._fields_] == list(orc.INDEX_KEYS) == ["pay_off", "pay_len", "ulen", "original"]


def test_exported_symbols_are_the_table(orc):
    out = subprocess.run(["nm", "-D", "--defined-only", orc.library_path()], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split() and line.split()[-1].startswith("smo_")}
    assert exported == set(orc.ORC_ABI_SYMBOLS)
    for name in orc.ORC_ABI_SYMBOLS:
        assert getattr(orc.lib(), name) is not None


def test_library_links_its_companions_by_name(orc):
    out = subprocess.run(["readelf", "-d", orc.library_path()], capture_output=True, text=True).stdout
    assert "libsnappy_mi355x_multi.so" in out and "libsnappy_mi355x.so" in out and "$ORIGIN" in out


def test_importing_loads_no_library():
    import sys
    code = ("import sys; sys.path.insert(0, %r); from conftest import load_package; import importlib; "
            "load_package(); m = importlib.import_module('snappy_jl_amd.orc'); "
            "assert m._lib is None and m._ctx == {}; "
            "assert 'libsnappy_mi355x' not in open('/proc/self/maps').read()" % os.path.join(ROOT, "tests"))
    subprocess.run([sys.executable, "-c", code], check=True)


def test_not_built_message(orc, monkeypatch, tmp_path):
    monkeypatch.setattr(orc, "_lib", None)
    monkeypatch.setattr(orc, "LIB_PATH", str(tmp_path / "libsnappy_mi355x_orc.so"))
    with pytest.raises(OSError) as e:
        orc.lib()
    assert str(e.value) == "libsnappy_mi355x_orc.so not built (run __graft_entry__.build())"


# ---- the sanitizer driver --------------------------------------------------------------------------------

def test_host_check_runs_clean(tmp_path):
    r = subprocess.run(["make", "-C", CSRC, "host_check", "OBJ=%s" % tmp_path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "smo_host_check ok" in r.stdout
    src = open(os.path.join(CSRC, "smo_host_check.cpp")).read()
    assert "smo_streams_plan" in src and "smo_index" in src and "int main()" in src


# ---- an independent writer's files -------------------------------------------------------------------------

def fixture_record():
    with open(os.path.join(GOLDEN, "orc_fixture.json")) as f:
        return json.load(f)


def fixture_file(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


@pytest.mark.parametrize("name", ["snappy_64k.orc", "snappy_256k.orc"])
def test_fixture_structure(orc, name):
    """What needs no raw codec: the PostScript, the walk by the reference and by the library."""
    rec, data = fixture_record()["files"][name], fixture_file(name)
    assert len(data) == rec["file_bytes"] and data[:3] == b"ORC"
    assert R.postscript(data) == (rec["postscript_length"], rec["block_size"])
    body = R.file_streams(data)
    status, chunks, total = R.walk(body, rec["block_size"])
    assert (status, len(chunks), total) == (0, rec["chunks"], rec["decoded_bytes"])
    stored = sum(c.original for c in chunks)
    assert stored == rec["stored_chunks"] and 0 < stored < len(chunks)  # both kinds occur
    assert max(c.ulen for c in chunks) == rec["largest_chunk"] <= rec["block_size"]
    s, a = orc.index_chunks(body, rec["block_size"])
    assert (s.status, s.nchunks, s.total_length) == (0, rec["chunks"], rec["decoded_bytes"])
    assert a["pay_off"].tolist() == [c.pay_off for c in chunks] and a["original"].tolist() == [c.original for c in chunks]
    assert a["ulen"].tolist() == [c.ulen for c in chunks]
    if name == "snappy_256k.orc":  # a compressed chunk above 64 KiB: the fragment path's case
        assert any(c.ulen > 65536 and not c.original for c in chunks)
        assert orc.streams_plan([body], rec["block_size"])[5] > rec["chunks"] - stored
    else:
        assert rec["largest_chunk"] == 65536
        assert R.walk(body, 65535)[0] == R.CHUNK_TOO_LARGE == orc.index_chunks(body, 65535)[0].status


@pytest.mark.parametrize("name", ["snappy_64k.orc", "snappy_256k.orc"])
def test_fixture_decodes_under_libsnappy(libsnappy, name):
    rec, data = fixture_record()["files"][name], fixture_file(name)
    body = R.file_streams(data)
    decoded = R.decode(body, rec["block_size"], R.libsnappy_status(libsnappy))
    assert len(decoded) == rec["decoded_bytes"] and hashlib.sha256(decoded).hexdigest() == rec["sha256"]
    last = R.walk(body, rec["block_size"])[1][-1]  # the file footer: the schema's field names
    tail = decoded[last.out:]
    assert all(col.encode() in tail for col in fixture_record()["columns"]) and len(fixture_record()["columns"]) == 3
