"""The blocks library's host side on the CPU (snappy.jl_amd/blocks.py over
libsnappy_mi355x_blocks.so): the reference of tests/blocks_ref.py against known answers that do not
come from it, then smb_index and smb_streams_plan against the reference over every structural case,
the size helpers, the bindings table against the header, and the sanitizer driver."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

from prototype_types import assert_device_elements

import blocks_ref as R
from conftest import ROOT

CSRC = os.path.join(ROOT, "snappy.jl_amd", "csrc", "blocks")
HEX_ABC_HADOOP = "00000003" "00000005" "0308616263"
HEX_ABC_XERIAL = "82534e4150505900" "00000001" "00000001" "00000005" "0308616263"


@pytest.fixture(scope="module")
def bl(sm):
    return importlib.import_module("snappy_jl_amd.blocks")


# ---- the reference, pinned ---------------------------------------------------------------------------

def test_reference_known_answers(oracle):
    assert oracle.compress(b"abc") == bytes.fromhex("0308616263") == R.ABC
    assert R.encode(b"abc", R.HADOOP, oracle.compress) == bytes.fromhex(HEX_ABC_HADOOP)
    assert R.encode(b"abc", R.XERIAL, oracle.compress) == bytes.fromhex(HEX_ABC_XERIAL)
    assert R.encode(b"", R.HADOOP, oracle.compress) == bytes.fromhex("00000000")
    assert R.encode(b"", R.XERIAL, oracle.compress) == bytes.fromhex("82534e41505059000000000100000001") == R.HEADER
    for fmt in R.FORMATS:
        for data in (b"", b"abc", bytes(range(256)) * 300):
            assert R.decode(R.encode(data, fmt, oracle.compress), fmt, oracle) == data
    two = R.encode(bytes(70000), R.HADOOP, oracle.compress)
    assert two[:4] == R.be(65536) and [c.ulen for c in R.walk(two, R.HADOOP)[1]] == [65536, 4464]


def test_reference_cases_are_consistent():
    names = set()
    for name, fmt, stream, status, nchunks, total in R.structural_cases():
        assert (name, fmt) not in names
        names.add((name, fmt))
        st, chunks, tot = R.walk(stream, fmt)
        assert (st, len(chunks), tot) == (status, nchunks, total), (name, fmt)
    statuses = {c[3] for c in R.structural_cases()}
    assert statuses == {0, R.SM_ERR_VARINT, R.NO_HEADER, R.BAD_HEADER, R.TRUNCATED, R.CHUNK_TOO_LARGE, R.BLOCK_LENGTH}


# ---- smb_index -------------------------------------------------------------------------------------------

def test_known_answers_through_the_library(bl):
    for fmt, text, pay_off in ((R.HADOOP, HEX_ABC_HADOOP, 8), (R.XERIAL, HEX_ABC_XERIAL, 20)):
        s, a = bl.index_blocks(bytes.fromhex(text), fmt)
        assert (s.status, s.nchunks, s.total_length) == (0, 1, 3)
        assert (a["pay_off"].tolist(), a["pay_len"].tolist(), a["ulen"].tolist()) == ([pay_off], [5], [3])
        rc, first, out_len, status, chunks, frags = bl.streams_plan([bytes.fromhex(text)], fmt)
        assert (rc, first.tolist(), out_len.tolist(), status.tolist(), chunks, frags) == (0, [0, 1], [3], [0], 1, 1)
    for fmt, text in ((R.HADOOP, "00000000"), (R.XERIAL, "82534e41505059000000000100000001")):
        s, a = bl.index_blocks(bytes.fromhex(text), fmt)
        assert (s.status, s.nchunks, s.total_length) == (0, 0, 0)
        rc, first, out_len, status, chunks, frags = bl.streams_plan([bytes.fromhex(text)], fmt)
        assert (rc, first.tolist(), out_len.tolist(), status.tolist(), chunks, frags) == (0, [0, 0], [0], [0], 0, 0)
    assert bl.length_uncompressed(bytes.fromhex(HEX_ABC_HADOOP), "hadoop") == 3
    with pytest.raises(bl.BlocksError) as e:
        bl.length_uncompressed(bytes.fromhex(HEX_ABC_HADOOP), "xerial")
    assert e.value.code == R.NO_HEADER and e.value.stream is None and "header" in str(e.value)


@pytest.mark.parametrize("case", range(len(R.structural_cases())), ids=lambda i: "%s-%s" % R.structural_cases()[i][1::-1])
def test_every_walk_status(bl, case):
    name, fmt, stream, status, nchunks, total = R.structural_cases()[case]
    s, a = bl.index_blocks(stream, fmt)
    assert (s.status, s.nchunks, s.total_length) == (status, nchunks, total)
    chunks = R.walk(stream, fmt)[1]
    assert a["pay_off"].tolist() == [c.pay_off for c in chunks]
    assert a["pay_len"].tolist() == [c.pay_len for c in chunks] and a["ulen"].tolist() == [c.ulen for c in chunks]
    if nchunks:  # one entry too few: the same walk, SM_BUFFER_TOO_SMALL unless it ended in an error
        s, a = bl.index_blocks(stream, fmt, max_chunks=nchunks - 1)
        assert (s.status, s.nchunks, s.total_length) == (status or R.SM_BUFFER_TOO_SMALL, nchunks, total)


def test_status_texts(bl):
    texts = {code: bl.status_message(code) for code in range(56, 61)}
    assert len(set(texts.values())) == 5 and all("lock stream" in t for t in texts.values())
    assert bl.status_message(18) == "Could not decode varint32."  # the main library's
    assert bl.status_message(61) == bl.status_message(55)  # both unused
    assert bl.version().startswith("snappy_mi355x_blocks gfx950 ")
    assert (bl.SMB_ERR_NO_HEADER, bl.SMB_ERR_BAD_HEADER, bl.SMB_ERR_TRUNCATED, bl.SMB_ERR_CHUNK_TOO_LARGE,
            bl.SMB_ERR_BLOCK_LENGTH) == (R.NO_HEADER, R.BAD_HEADER, R.TRUNCATED, R.CHUNK_TOO_LARGE, R.BLOCK_LENGTH)


def test_status_codes_are_free_in_the_other_headers():
    for header in ("snappy_mi355x.h", "snappy_mi355x_framing.h", "snappy_mi355x_multi.h"):
        text = open(os.path.join(ROOT, "include", header)).read()
        assert not re.search(r"=\s*(5[6-9]|6[01])\b", text), header
    mine = open(os.path.join(ROOT, "include", "snappy_mi355x_blocks.h")).read()
    assert re.findall(r"(SMB_ERR_\w+) = (\d+)", mine) == [
        ("SMB_ERR_NO_HEADER", "56"), ("SMB_ERR_BAD_HEADER", "57"), ("SMB_ERR_TRUNCATED", "58"),
        ("SMB_ERR_CHUNK_TOO_LARGE", "59"), ("SMB_ERR_BLOCK_LENGTH", "60")]


# ---- smb_streams_plan ------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", R.FORMATS)
def test_plan_back_to_back(bl, fmt):
    streams = [c[2] for c in R.cases_of(fmt)]
    caps = [c[5] for c in R.cases_of(fmt)]
    want = R.plan(streams, fmt, caps, 0x7FFFFFFF)
    rc, first, out_len, status, chunks, frags = bl.streams_plan(streams, fmt, out_cap=caps)
    assert (rc, first.tolist(), out_len.tolist(), status.tolist(), chunks, frags) == want and chunks > 5
    assert status.tolist() == [c[3] for c in R.cases_of(fmt)]
    # exact, then one too few
    got = bl.streams_plan(streams, fmt, out_cap=caps, max_chunks=chunks)
    assert (got[0], got[3].tolist()) == (0, want[3])
    rc, first, out_len, status, total, _ = bl.streams_plan(streams, fmt, out_cap=caps, max_chunks=chunks - 1)
    assert (rc, total) == (R.SM_BUFFER_TOO_SMALL, chunks)
    assert status.tolist() == [R.SM_ERR_ARGUMENT] * len(streams) and out_len.tolist() == [0] * len(streams)
    assert (rc, first.tolist(), out_len.tolist(), status.tolist()) == R.plan(streams, fmt, caps, chunks - 1)[:4]
    # a byte short gives its slots up; no cap is no limit
    victim = next(i for i, c in enumerate(R.cases_of(fmt)) if c[3] == 0 and c[4] == 2)
    short = list(caps)
    short[victim] -= 1
    got = bl.streams_plan(streams, fmt, out_cap=short)
    assert (got[0], got[1].tolist(), got[2].tolist(), got[3].tolist(), got[4], got[5]) == R.plan(streams, fmt, short, 0x7FFFFFFF)
    assert got[3][victim] == R.SM_BUFFER_TOO_SMALL and got[4] == chunks - 2
    free = bl.streams_plan(streams, fmt)
    assert free[3].tolist() == want[3] and free[4] == chunks


def test_plan_counts_fragments(bl):
    big = R.be(200000) + R.chunk(R.varint(200000))  # (structure only)
    rc, first, out_len, status, chunks, frags = bl.streams_plan([bytes.fromhex(HEX_ABC_HADOOP), big, big], "hadoop",
                                                                out_cap=[3, 200000, 199999])
    assert (rc, first.tolist(), status.tolist(), chunks, frags) == (0, [0, 1, 2, 2], [0, 0, R.SM_BUFFER_TOO_SMALL], 2, 5)


# ---- the size helpers ------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 65535, 65536, 65537, 131073])
def test_max_length(bl, oracle, n):
    rng = np.random.default_rng(n)
    data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    for fmt in R.FORMATS:
        want = R.max_length(n, fmt)
        assert bl.max_length(n, fmt) == want
        written = R.encode(data, fmt, oracle.compress)
        assert len(written) <= want
        # the writer's stream with every payload at its bound has exactly that size
        pieces = -(-n // R.BLOCK)
        assert want == len(written) + sum(R.max_compressed_length(c.ulen) - c.pay_len for c in R.walk(written, fmt)[1])
        assert len(R.walk(written, fmt)[1]) == pieces
    assert bl.max_length(0, "hadoop") == 4 and bl.max_length(0, "xerial") == 16


def test_max_chunks(bl):
    assert [bl.max_chunks(n, "hadoop") for n in (0, 4, 5, 9, 10, 5000)] == [0, 0, 1, 1, 2, 1000]
    assert [bl.max_chunks(n, "xerial") for n in (0, 15, 16, 20, 21, 5016)] == [0, 0, 0, 0, 1, 1000]
    for fmt in R.FORMATS:  # no stream of the cases holds more
        for c in R.cases_of(fmt):
            assert c[4] <= bl.max_chunks(len(c[2]), fmt), c[0]
    with pytest.raises(ValueError):
        bl.max_chunks(5, "lz4")


def test_scratch_bytes(bl):
    f = bl.lib().smb_streams_scratch_bytes
    assert f(3, 7, 0) > f(3, 6, 0) and f(4, 7, 9) >= f(3, 7, 9) and f(3, 0, 1000) > f(3, 0, 1) and f(0, 0, 0) > 0
    assert f(1, 10, 0) >= 10 * 76496  # the compress call's slots


# ---- the bindings ----------------------------------------------------------------------------------------

SCALARS = {"size_t": ctypes.c_size_t, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "int": ctypes.c_int,
           "int32_t": ctypes.c_int32, "sm_status": ctypes.c_int32}


def _declarations():
    with open(os.path.join(ROOT, "include", "snappy_mi355x_blocks.h")) as f:
        src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S))
    out = {}
    for m in re.finditer(r"([\w\s\*]+?)\b(smb_\w+)\s*\(([^;{]*?)\)\s*;", src, re.S):
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


def test_table_matches_the_header(sm, bl):
    binding = importlib.import_module("snappy_jl_amd._binding")
    declared, table = _declarations(), binding.BLOCKS
    assert len(declared) == 15 and set(declared) == set(table)
    for name, (ret, params) in declared.items():
        restype, argtypes = binding.prototype(table[name])
        assert len(argtypes) == len(params), name
        assert _class(restype) == _c_class(ret), name
        for k, (t, p) in enumerate(zip(argtypes, params)):
            assert t is not None and _class(t) == _c_class(p), "%s: argument %d (%s)" % (name, k, p.strip())
    assert assert_device_elements(binding, declared, table) == 21  # the pointer parameters of the *_device functions, ctx and stream among them
    assert bl.BLOCKS_ABI_SYMBOLS == tuple(table)
    others = [binding.RAW, binding.FRAMING, binding.MULTI]
    assert not set(table) & set().union(*others)  # a group of its own
    assert [n for n, _ in binding.BlockChunks._fields_] == list(bl.INDEX_KEYS) == ["pay_off", "pay_len", "ulen"]
    for name in table:  # every symbol is exported
        assert getattr(bl.lib(), name) is not None


def test_library_links_its_companions_by_name(bl):
    out = subprocess.run(["readelf", "-d", bl.library_path()], capture_output=True, text=True).stdout
    assert "libsnappy_mi355x_multi.so" in out and "libsnappy_mi355x.so" in out and "$ORIGIN" in out


def test_importing_loads_no_library():
    import sys
    code = ("import sys; sys.path.insert(0, %r); from conftest import load_package; import importlib; "
            "load_package(); m = importlib.import_module('snappy_jl_amd.blocks'); "
            "assert m._lib is None and m._ctx == {}; "
            "assert 'libsnappy_mi355x' not in open('/proc/self/maps').read()" % os.path.join(ROOT, "tests"))
    subprocess.run([sys.executable, "-c", code], check=True)


def test_not_built_message(bl, monkeypatch, tmp_path):
    monkeypatch.setattr(bl, "_lib", None)
    monkeypatch.setattr(bl, "LIB_PATH", str(tmp_path / "libsnappy_mi355x_blocks.so"))
    with pytest.raises(OSError) as e:
        bl.lib()
    assert str(e.value) == "libsnappy_mi355x_blocks.so not built (run __graft_entry__.build())"


# ---- the sanitizer driver --------------------------------------------------------------------------------

def test_host_check_runs_clean(tmp_path):
    r = subprocess.run(["make", "-C", CSRC, "host_check", "OBJ=%s" % tmp_path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "smb_host_check ok" in r.stdout
    src = open(os.path.join(CSRC, "smb_host_check.cpp")).read()
    assert "smb_streams_plan" in src and "smb_index" in src
