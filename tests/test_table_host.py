"""The LevelDB table library's host side on the CPU (snappy.jl_amd/table.py over
libsnappy_mi355x_table.so): the reference of tests/table_ref.py and the library against pins that
come from neither (the RFC 3720 CRC-32C vectors, the magic, a hand-assembled empty table), then
smt_footer, smt_walk_index, smt_block_head and smt_write_tail against the reference, the fixtures of
tests/golden/table/ against their recipe's record, the bindings table against the header, and the
sanitizer driver."""
import ctypes
import hashlib
import importlib
import json
import os
import re
import struct
import subprocess

import pytest

from prototype_types import assert_device_elements

import avro_ref
import table_ref as R
from conftest import ROOT

CSRC = os.path.join(ROOT, "snappy.jl_amd", "csrc", "table")
GOLDEN = os.path.join(ROOT, "tests", "golden", "table")
FILES = ("mixed.ldb", "bigblock.ldb", "bigindex.ldb", "empty.ldb")
MAGIC = bytes.fromhex("57fb808b247547db")
# a metaindex block with no entries (restart array {0}, one restart), stored, with its masked
# CRC-32C; an index block alike; the footer: handles (0, 8) and (13, 8), padding, the magic
HEX_EMPTY = ("0000000001000000" "00" "c0f2a1b0") * 2 + "00080d08" + "00" * 36 + "57fb808b247547db"
RFC3720 = [(bytes(32), 0x8A9136AA), (b"\xff" * 32, 0x62A8AB43), (bytes(range(32)), 0x46DD794E),
           (bytes(range(31, -1, -1)), 0x113FDB5C)]


@pytest.fixture(scope="module")
def tb(sm):
    return importlib.import_module("snappy_jl_amd.table")


@pytest.fixture(scope="module")
def fr(sm):
    return importlib.import_module("snappy_jl_amd.framing")


@pytest.fixture(scope="module")
def files():
    out = {}
    for name in FILES:
        with open(os.path.join(GOLDEN, name), "rb") as f:
            out[name] = f.read()
    return out


@pytest.fixture(scope="module")
def described():
    with open(os.path.join(GOLDEN, "table_fixture.json")) as f:
        return json.load(f)["files"]


def footer(moff, msize, ioff, isize, body=b""):
    foot = R.put_varint(moff) + R.put_varint(msize) + R.put_varint(ioff) + R.put_varint(isize)
    return bytes(body) + foot + bytes(40 - len(foot)) + MAGIC


def ref_footer(data):
    try:
        return 0, R.read_footer(data)
    except R.Stop as e:
        return e.status, None


# ---- the pins ------------------------------------------------------------------------------------------

def test_reference_pins():
    for data, crc in RFC3720:
        assert R.crc32c(data) == crc
    assert R.crc32c(b"") == 0 and R.mask(0) == 0xA282EAD8
    assert R.MAGIC == MAGIC == struct.pack("<Q", 0xDB4775248B80FB57)
    empty = bytes.fromhex(HEX_EMPTY)
    assert len(empty) == 74 and R.write_table([], [], None) == empty
    compress, uncompress = avro_ref.libsnappy()
    assert R.read_footer(empty) == ((0, 8), (13, 8))
    p = R.plan(empty, uncompress)
    assert (p.status, p.out_len, p.decoded, p.handles) == (0, 0, b"", [])
    assert R.put_varint(300) == b"\xac\x02" and R.get_varint64(b"\xff" * 9 + b"\x01", 0, 10) == (2**64 - 1, 10)
    assert R.get_varint64(b"\xff" * 9 + b"\x02", 0, 10) is None and R.get_varint32(b"\x80" * 4 + b"\x10", 0, 5) is None
    block = R.build_block([(b"apple", b"1"), (b"apply", b"2")])
    assert block == bytes.fromhex("000501") + b"apple1" + bytes.fromhex("040101") + b"y2" + bytes.fromhex("0000000001000000")
    assert list(R.entries(block)) == [(b"apple", b"1"), (b"apply", b"2")]
    stored, size = R.stored_block(b"abc" * 40, compress)
    assert stored[size] == 1 and size == len(compress(b"abc" * 40)) and R.read_block(stored, (0, size), uncompress) == (0, b"abc" * 40)
    stored, size = R.stored_block(b"abcdefgh", compress)  # (not 12.5 % smaller: stored)
    assert stored[size] == 0 and size == 8


def test_library_pins(tb, fr):
    for data, crc in RFC3720:
        assert fr.lib().smf_crc32c(data, len(data)) == crc
    assert fr.lib().smf_crc32c_mask(0) == 0xA282EAD8
    assert tb.MAGIC == MAGIC and tb.FOOTER_LENGTH == 48 and tb.BLOCK_TRAILER == 5
    empty = bytes.fromhex(HEX_EMPTY)
    assert tb.write_tail([], [], 0) == empty
    assert tb.read_footer(empty) == ((0, 8), (13, 8)) and tb.index_bound(empty) == 8
    assert tb.walk_index(empty[13:21], len(empty)) == (0, 0, [])
    assert tb.block_head(empty, (13, 8)) == (0, 8)


# ---- the footer ----------------------------------------------------------------------------------------

def footer_cases():
    ok = footer(0, 8, 13, 8, bytes(26))
    cases = [b"", bytes(47), bytes(48), ok, ok[1:], ok[:-1]]
    cases += [ok[:len(ok) - 8 + i] + bytes([ok[len(ok) - 8 + i] ^ 0x40]) + ok[len(ok) - 7 + i:] for i in range(8)]
    cases.append(bytes(26) + b"\x80" * 9 + b"\x01" + bytes(30) + MAGIC)  # a 10-byte varint64: 2^63
    cases.append(bytes(26) + b"\x80" * 9 + b"\x02" + bytes(30) + MAGIC)  # its tenth byte 2
    cases.append(bytes(26) + b"\x80" * 40 + MAGIC)  # leaves the 40 bytes
    cases.append(bytes(26) + b"\x00" * 3 + b"\xff" * 37 + MAGIC)  # the last varint cut by the magic
    cases.append(footer(0, 8, 13, 8, bytes(26)))  # the index block ends exactly at n - 48
    cases.append(footer(0, 8, 13, 9, bytes(26)))  # ... and a byte later
    cases.append(footer(0, 22, 13, 8, bytes(26)))  # the metaindex handle is checked too
    cases.append(footer(2**64 - 1, 8, 13, 8, bytes(26)))  # off + size overflows 64 bits
    cases.append(footer(0, 8, 9, 2**64 - 4, bytes(26)))
    cases.append(footer(0, 8, 0, 0x7FFFFFFF, bytes(26)))
    return cases


def test_footer_equals_the_reference(tb):
    seen = set()
    for data in footer_cases():
        st, handles = tb.read_footer(data, status=True)
        want, ref = ref_footer(data)
        assert st == want, data[-48:].hex()
        if want == 0:
            assert handles == ref
        seen.add(st)
    assert seen == {0, R.TRUNCATED, R.MAGIC_ERR, R.FOOTER, R.HANDLE}
    # TOO_LARGE needs a table of more than 2 GiB to pass the handle check first; the rule's order
    # shows on the index walk (below), which takes the table's length as a number
    with pytest.raises(tb.TableError) as e:
        tb.read_footer(bytes(48))
    assert e.value.code == R.MAGIC_ERR and "magic" in str(e.value)


# ---- the index walk --------------------------------------------------------------------------------------

def entry(shared, klen, value):
    return R.put_varint(shared) + R.put_varint(klen) + R.put_varint(len(value)) + b"k" * klen + value


def contents(entries, r=1):
    return entries + bytes(4 * r) + struct.pack("<I", r)


def index_cases():
    n = 1048
    h = R.put_handle
    cases = [(bytes(3), n), (bytes(4), n), (contents(b"", 1), n), (contents(b"", 0), n), (bytes(4) + struct.pack("<I", 2), n)]
    whole = entry(0, 7, h((10, 20))) + entry(7, 2, h((35, 40)))
    parts = [0, 1, 2, 3, 3 + 7, 3 + 7 + 1]  # cut at shared, non_shared, value_len, the key, the handle's two varints
    first = len(entry(0, 7, h((10, 20))))
    for cut in parts:
        cases.append((contents(whole[:first + cut]), n))
        cases.append((contents(whole[:cut]), n))
    cases.append((contents(entry(0, 7, h((10, 20))) + entry(8, 2, h((35, 40)))), n))  # shared one over
    cases.append((contents(entry(0, 7, h((10, 20))) + entry(7, 0, h((35, 40))) + entry(8, 0, h((80, 1)))), n))
    cases.append((contents(entry(0, 1, R.put_varint(5))), n))  # a value holding one varint only
    cases.append((contents(entry(0, 1, b"")), n))
    cases.append((contents(entry(0, 1, h((10, 20)) + b"\xee\xff")), n))  # trailing bytes
    cases.append((contents(entry(0, 1, b"\x80" * 9 + b"\x02" + b"\x00")), n))
    cases.append((contents(entry(0, 1, h((995, 0)))), n))  # ends exactly at n - 48
    cases.append((contents(entry(0, 1, h((996, 0)))), n))
    cases.append((contents(entry(0, 1, h((2**64 - 1, 2)))), n))
    cases.append((contents(entry(0, 1, h((0, 0x7FFFFFFF)))), 2**32))  # TOO_LARGE, behind the handle check
    cases.append((contents(entry(0, 1, h((0, 0x7FFFFFFF)))), 2**31))  # HANDLE first
    cases.append((contents(b"\x80\x80\x80\x80\x10" + bytes(8)), n))  # a varint32's fifth byte 0x10
    cases.append((contents(b"\x80\x80\x80\x80\x0f\x00\x00"), n))  # shared 0xf0000000 over the key length
    for klen in (0, 1, 63, 64, 65, 300):
        cases.append((contents(entry(0, klen, h((10, 20))) + entry(klen, 3, h((35, 40))) + entry(klen + 3, 0, h((80, 1))), 3), n))
    return cases


def test_walk_index_equals_the_reference(tb):
    seen = set()
    for data, n in index_cases():
        st, count, handles = tb.walk_index(data, n)
        want, ref = R.walk_index(data, n)
        assert (st, count, handles) == (want, len(ref), ref), data.hex()
        seen.add(st)
    assert seen == {0, R.INDEX, R.HANDLE, R.TOO_LARGE}
    three = index_cases()[-1]
    assert tb.walk_index(*three, max_entries=2) == (R.SM_BUFFER_TOO_SMALL, 3, [(10, 20), (35, 40)])


def test_block_head_equals_the_reference(tb):
    compress, _ = avro_ref.libsnappy()
    stored, size = R.stored_block(b"abc" * 40, compress)
    assert tb.block_head(stored, (0, size)) == R.block_head(stored, (0, size)) == (1, 120)
    for kind, body, want in ((0, b"abcd", (0, 0, 4)), (2, b"abcd", (R.TYPE, 2, 0)), (1, b"", (R.SM_ERR_VARINT, 1, 0)),
                             (1, b"\xff" * 5, (R.SM_ERR_VARINT, 1, 0)), (1, b"\xff\xff\xff\xff\x08", (R.TOO_LARGE, 1, 0)),
                             (1, b"\xff\xff\xff\xff\x07", (0, 1, 0x7FFFFFFF)), (1, b"\x80", (R.SM_ERR_VARINT, 1, 0))):
        data = body + bytes([kind]) + bytes(4)
        assert tb.block_head(data, (0, len(body)), status=True) == want
        try:
            ref = (0,) + R.block_head(data, (0, len(body)))
        except R.Stop as e:
            ref = (e.status,)
        assert ref == want[:len(ref)]
    assert tb.block_head(bytes(10), (0, 6), status=True)[0] == R.HANDLE


# ---- the fixtures ----------------------------------------------------------------------------------------

def test_fixtures_are_what_the_recipe_describes(tb, files, described):
    _, uncompress = avro_ref.libsnappy()
    for name in FILES:
        data, d = files[name], described[name]
        assert len(data) < 400 * 1024 and hashlib.sha256(data).hexdigest() == d["sha256_file"], name
        p = R.plan(data, uncompress)
        assert (p.status, p.out_len, len(p.handles)) == (0, d["decoded_bytes"], d["blocks"]), name
        assert hashlib.sha256(p.decoded).hexdigest() == d["sha256_decoded"], name
        assert [list(h) for h in p.handles][:64] == d["handles"], name
        assert tb.read_footer(data)[1] == tuple(d["index_handle"]) and tb.index_bound(data) == d["index_bytes"], name
        index = tuple(d["index_handle"])
        raw = data[index[0]:index[0] + index[1]]
        decoded_index = uncompress(raw) if d["index_type"] else raw
        assert tb.walk_index(decoded_index, len(data)) == (0, d["blocks"], p.handles), name
        assert tb.max_blocks(d["index_bytes"]) >= d["blocks"]
    assert set(described["mixed.ldb"]["types"]) == {0, 1} and described["mixed.ldb"]["index_type"] == 1
    assert described["bigindex.ldb"]["index_bytes"] > 65536 and described["bigindex.ldb"]["blocks"] == 4500
    assert described["bigblock.ldb"]["decoded_bytes"] > 3 * 65536 and described["empty.ldb"]["blocks"] == 0
    # a key looked up in a decoded block: the entry iterator reads what the block builder wrote
    p = R.plan(files["mixed.ldb"], uncompress)
    block = p.decoded[p.block_out_off[1]:p.block_out_off[1] + p.block_len[1]]
    pairs = list(R.entries(block))
    assert len(pairs) > 16 and all(k.startswith(b"fixture/key/") and len(k) == 24 for k, _ in pairs)
    assert [k for k, _ in pairs] == sorted(k for k, _ in pairs)


# ---- the tail writer and the size helpers ----------------------------------------------------------------

def test_write_tail_equals_the_reference(tb, files):
    _, uncompress = avro_ref.libsnappy()
    for keys, handles, base in (([], [], 0), ([b""], [(0, 0)], 5), ([b"a", b"", b"k" * 300], [(0, 100), (105, 70000), (70110, 3)], 70118),
                                ([b"x" * 127, b"y" * 128], [(2**40, 2**31 - 2), (2**63, 1)], 2**63 + 6)):
        assert tb.write_tail(keys, handles, base) == R.write_tail(keys, handles, base), keys
    p = R.plan(files["bigindex.ldb"], uncompress)
    keys = [b"fixture/key/%012d" % i for i in range(4500)]
    base = p.handles[-1][0] + p.handles[-1][1] + 5
    tail = tb.write_tail(keys, p.handles, base)
    assert tail == R.write_tail(keys, p.handles, base)
    rebuilt = files["bigindex.ldb"][:base] + tail  # the same table with a stored index
    q = R.plan(rebuilt, uncompress)
    assert (q.status, q.handles, q.decoded) == (0, p.handles, p.decoded)
    with pytest.raises(ValueError):
        tb.write_tail([b"a"], [], 0)


def test_size_helpers_and_texts(tb):
    assert [tb.max_blocks(n) for n in (0, 4, 5, 9, 10, 500)] == [0, 0, 1, 1, 2, 100]
    assert len(entry(0, 0, R.put_handle((0, 0)))) == 5  # the shortest entry there is
    assert [tb.max_block_length(n) for n in (0, 1, 4096)] == [5, 6, 4101]
    assert tb.lib().smt_stage_length(65536) == 76496
    f = tb.lib().smt_tables_scratch_bytes
    assert f(3, 7, 0, 0, 0) > f(3, 6, 0, 0, 0) and f(4, 7, 9, 0, 0) >= f(3, 7, 9, 0, 0) and f(1, 1, 0, 0, 1 << 20) > 1 << 20
    assert f(1, 1, 1 << 20, 0, 0) > 1 << 20 and f(0, 0, 0, 0, 0) > 0
    texts = {code: tb.status_message(code) for code in range(96, 104)}
    assert len(set(texts.values())) == 8 and all(t.startswith("Table file") for t in texts.values())
    assert tb.status_message(18) == "Could not decode varint32."  # the main library's
    assert tb.status_message(104) == tb.status_message(95)  # both unused
    assert tb.version().startswith("snappy_mi355x_table gfx950 ")
    assert (tb.SMT_ERR_TRUNCATED, tb.SMT_ERR_MAGIC, tb.SMT_ERR_FOOTER, tb.SMT_ERR_HANDLE, tb.SMT_ERR_TOO_LARGE, tb.SMT_ERR_TYPE,
            tb.SMT_ERR_INDEX, tb.SMT_ERR_CRC) == (R.TRUNCATED, R.MAGIC_ERR, R.FOOTER, R.HANDLE, R.TOO_LARGE, R.TYPE, R.INDEX, R.CRC)
    for header in os.listdir(os.path.join(ROOT, "include")):
        text = open(os.path.join(ROOT, "include", header)).read()
        taken = re.findall(r"_ERR_\w+ = (9[6-9]|10[0-3])\b", text)
        assert taken == ([str(c) for c in range(96, 104)] if header == "snappy_mi355x_table.h" else []), header


# ---- the bindings ----------------------------------------------------------------------------------------

SCALARS = {"size_t": ctypes.c_size_t, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "int": ctypes.c_int,
           "int32_t": ctypes.c_int32, "sm_status": ctypes.c_int32}


def _declarations():
    with open(os.path.join(ROOT, "include", "snappy_mi355x_table.h")) as f:
        src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S))
    out = {}
    for m in re.finditer(r"([\w\s\*]+?)\b(smt_\w+)\s*\(([^;{]*?)\)\s*;", src, re.S):
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


def test_table_matches_the_header(sm, tb):
    binding = importlib.import_module("snappy_jl_amd._binding")
    declared, table = _declarations(), binding.TABLE
    assert len(declared) == 21 and set(declared) == set(table)
    for name, (ret, params) in declared.items():
        restype, argtypes = binding.prototype(table[name])
        assert len(argtypes) == len(params), name
        assert _class(restype) == _c_class(ret), name
        for k, (t, p) in enumerate(zip(argtypes, params)):
            assert t is not None and _class(t) == _c_class(p), "%s: argument %d (%s)" % (name, k, p.strip())
    assert assert_device_elements(binding, declared, table) == 47  # the pointer parameters of the *_device functions, ctx and stream among them
    assert tb.TABLE_ABI_SYMBOLS == tuple(table)
    others = [binding.RAW, binding.FRAMING, binding.MULTI, binding.BLOCKS, binding.ORC, binding.PARQUET, binding.PARQUET_WRITE,
              binding.AVRO]
    assert not set(table) & set().union(*others)  # a group of its own
    assert ctypes.sizeof(binding.Summary) == 16  # smt_summary: 8 + 4 + 4
    for name in table:  # every symbol is exported
        assert getattr(tb.lib(), name) is not None


def test_library_links_its_companions_by_name(tb):
    out = subprocess.run(["readelf", "-d", tb.library_path()], capture_output=True, text=True).stdout
    assert "libsnappy_mi355x_multi.so" in out and "libsnappy_mi355x_framing.so" in out and "libsnappy_mi355x.so" in out
    assert "$ORIGIN" in out


def test_importing_loads_no_library():
    import sys
    code = ("import sys; sys.path.insert(0, %r); from conftest import load_package; import importlib; "
            "load_package(); m = importlib.import_module('snappy_jl_amd.table'); "
            "assert m._lib is None and m._ctx == {}; "
            "assert 'libsnappy_mi355x' not in open('/proc/self/maps').read()" % os.path.join(ROOT, "tests"))
    subprocess.run([sys.executable, "-c", code], check=True)


def test_not_built_message(tb, monkeypatch, tmp_path):
    monkeypatch.setattr(tb, "_lib", None)
    monkeypatch.setattr(tb, "LIB_PATH", str(tmp_path / "libsnappy_mi355x_table.so"))
    with pytest.raises(OSError) as e:
        tb.lib()
    assert str(e.value) == "libsnappy_mi355x_table.so not built (run __graft_entry__.build())"


def test_build_and_smoke_name_the_library():
    entry_text = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert '"csrc", "table")' in entry_text and "snappy_jl_amd.table" in entry_text and "_table.so" in entry_text
    assert entry_text.index('"csrc", "framing")') < entry_text.index('"csrc", "multi")') < entry_text.index('"csrc", "table")')
    assert entry_text.index('"csrc", "table")') < entry_text.index('"oracle")')


# ---- the sanitizer driver --------------------------------------------------------------------------------

def test_host_check_runs_clean(tmp_path):
    r = subprocess.run(["make", "-C", CSRC, "host_check", "OBJ=%s" % tmp_path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "smt_host_check ok" in r.stdout
    src = open(os.path.join(CSRC, "smt_host_check.cpp")).read()
    assert all(name in src for name in ("smt_footer", "smt_walk_index", "smt_block_head", "smt_write_tail", "smt_index_bound"))
