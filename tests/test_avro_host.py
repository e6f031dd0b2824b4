"""The Avro container library's host side on the CPU (snappy.jl_amd/avro.py over
libsnappy_mi355x_avro.so): the reference of tests/avro_ref.py against known answers that do not come
from it, then sma_index, sma_streams_plan and sma_find_sync against the reference on the four
fixtures of tests/golden/avro/, one input per walk status, every truncation of a file's first 200
bytes, the header writer, the bindings table against the header, and the sanitizer driver."""
import ctypes
import hashlib
import importlib
import json
import os
import re
import subprocess
import zlib

import pytest

from prototype_types import assert_device_elements

import avro_ref as R
from conftest import ROOT

CSRC = os.path.join(ROOT, "snappy.jl_amd", "csrc", "avro")
GOLDEN = os.path.join(ROOT, "tests", "golden", "avro")
FILES = ("blocks_64k.avro", "small_blocks.avro", "bigblock.avro", "meta_forms.avro")
SYNC = bytes(range(0xA0, 0xB0))
# "Obj\1"; a map of one block with two pairs, avro.schema = "bytes" (with its quotes) and avro.codec =
# snappy; the map's end; the marker; one block: count 1, size 9, compress("abc"), CRC-32("abc"), the marker
HEX_ONE_BLOCK = ("4f626a01" "04" "16" + b"avro.schema".hex() + "0e" + b'"bytes"'.hex() + "14" + b"avro.codec".hex() + "0c"
                 + b"snappy".hex() + "00" + SYNC.hex() + "02" "12" "0308616263" "352441c2" + SYNC.hex())
ZIGZAG = [(0, "00"), (-1, "01"), (1, "02"), (63, "7e"), (64, "8001"), (-64, "7f"), (-65, "8101"), (2**31, "8080808010"),
          (2**62, "80808080808080808001"), (-2**62, "ffffffffffffffff7f")]


@pytest.fixture(scope="module")
def av(sm):
    return importlib.import_module("snappy_jl_amd.avro")


@pytest.fixture(scope="module")
def files():
    out = {}
    for name in FILES:
        with open(os.path.join(GOLDEN, name), "rb") as f:
            out[name] = f.read()
    return out


@pytest.fixture(scope="module")
def described():
    with open(os.path.join(GOLDEN, "avro_fixture.json")) as f:
        return json.load(f)["files"]


# ---- the reference, pinned ---------------------------------------------------------------------------

def test_reference_known_answers():
    assert zlib.crc32(b"123456789") == 0xCBF43926 and zlib.crc32(b"abc") == 0x352441C2
    for v, text in ZIGZAG:
        assert R.encode_long(v) == bytes.fromhex(text), v
        assert R.decode_long(bytes.fromhex(text), 0) == (v, len(text) // 2), v
    compress, uncompress = R.libsnappy()
    assert compress(b"abc") == bytes.fromhex("0308616263") and uncompress(bytes.fromhex("0308616263")) == b"abc"
    one = bytes.fromhex(HEX_ONE_BLOCK)
    assert R.write([b"abc"], [1], b'"bytes"', SYNC, compress) == one
    w = R.walk(one)
    assert (w.status, w.total, w.objects, w.header_len, w.sync) == (0, 3, 1, 60, SYNC)
    assert w.blocks == [R.Block(62, 5, 3, 1, 0x352441C2, 0)]
    assert R.read(one, uncompress)[:2] == (0, b"abc")
    assert R.read(one[:-21] + b"\x00" + one[-20:], uncompress)[0] == R.CRC
    assert R.find_sync(one, SYNC, 0) == 44 and R.find_sync(one, SYNC, 45) == len(one) - 16
    assert R.find_sync(one, SYNC, len(one) - 15) == len(one)


def test_fixtures_are_what_the_recipe_describes(files, described):
    compress, uncompress = R.libsnappy()
    for name in FILES:
        status, decoded, w = R.read(files[name], uncompress)
        d = described[name]
        assert status == 0 and hashlib.sha256(decoded).hexdigest() == d["sha256"], name
        assert (len(files[name]), w.header_len, len(w.blocks), w.objects, w.total, w.sync.hex()) == (
            d["file_bytes"], d["header_length"], d["blocks"], d["objects"], d["decoded_bytes"], d["sync"]), name
        assert len(files[name]) < 200 * 1024
    assert described["small_blocks.avro"]["one_byte_counts"] > 0 < described["small_blocks.avro"]["two_byte_counts"]
    assert described["small_blocks.avro"]["blocks"] > 256 and described["bigblock.avro"]["largest_block"] > 3 * 65536
    assert files["meta_forms.avro"][4] & 1  # the first map block's count is negative


# ---- sma_index, sma_streams_plan, sma_find_sync ----------------------------------------------------------

def _same_walk(av, data, kind=R.FILE, sync=None):
    s, a = av.index_avro(data, kind, sync)
    w = R.walk(data, kind, sync)
    assert (s.status, s.nblocks, s.total_length, s.objects, s.header_length, bytes(s.sync)) == (
        w.status, len(w.blocks), w.total, w.objects, w.header_len, w.sync)
    for i, key in enumerate(av.INDEX_KEYS):
        assert a[key].tolist() == [b[i] for b in w.blocks], key
    return s, w


def test_known_answer_through_the_library(av):
    one = bytes.fromhex(HEX_ONE_BLOCK)
    s, a = av.index_avro(one)
    assert (s.status, s.nblocks, s.total_length, s.objects, s.header_length, bytes(s.sync)) == (0, 1, 3, 1, 60, SYNC)
    assert [a[k].tolist() for k in av.INDEX_KEYS] == [[62], [5], [3], [1], [0x352441C2], [0]]
    assert av.length_uncompressed(one) == 3
    rc, first, out_len, status, objects, blocks, frags = av.avro_plan([one])
    assert (rc, first.tolist(), out_len.tolist(), status.tolist(), objects.tolist(), blocks, frags) == (0, [0, 1], [3], [0], [1], 1, 1)
    s, a = av.index_avro(one[60:], "blocks", SYNC)
    assert (s.status, s.nblocks, s.total_length, a["pay_off"].tolist()) == (0, 1, 3, [2])
    with pytest.raises(av.AvroError) as e:
        av.length_uncompressed(one[60:])
    assert e.value.code == R.NO_HEADER and e.value.stream is None and "magic" in str(e.value)
    with pytest.raises(ValueError):
        av.index_avro(one, "blocks")


@pytest.mark.parametrize("name", FILES)
def test_index_equals_the_reference(av, files, name):
    s, w = _same_walk(av, files[name])
    assert s.status == 0 and bytes(s.sync) == w.sync and s.header_length == w.header_len
    # a block run behind every marker is the file's tail
    for k in (0, len(w.blocks) // 2, len(w.blocks) - 1):
        start = w.blocks[k].pay_off + w.blocks[k].pay_len + 20
        s2, w2 = _same_walk(av, files[name][start:], R.BLOCKS, w.sync)
        assert s2.status == 0 and s2.nblocks == len(w.blocks) - k - 1
    few = av.index_avro(files[name], max_blocks=len(w.blocks) - 1)[0]
    assert (few.status, few.nblocks, few.total_length) == (R.SM_BUFFER_TOO_SMALL, len(w.blocks), w.total)


def test_plan_equals_the_reference(av, files):
    streams = [files[n] for n in FILES] + [files["meta_forms.avro"][:1009], files["meta_forms.avro"][:-1], b""]
    caps = [R.walk(s).total for s in streams]
    caps[1] -= 1
    got = av.avro_plan(streams, out_cap=caps)
    want = R.plan(streams, caps=caps)
    assert (got[0], [x.tolist() for x in got[1:5]], got[5:]) == (want[0], list(want[1:5]), want[5:])
    assert got[3].tolist() == [0, R.SM_BUFFER_TOO_SMALL, 0, 0, 0, R.TRUNCATED, R.NO_HEADER] and got[5] == 4 + 1 + 4
    exact = av.avro_plan(streams, out_cap=caps, max_blocks=got[5])
    assert exact[0] == 0 and exact[3].tolist() == got[3].tolist()
    short = av.avro_plan(streams, out_cap=caps, max_blocks=got[5] - 1)
    want = R.plan(streams, caps=caps, max_blocks=got[5] - 1)
    assert (short[0], [x.tolist() for x in short[1:5]], short[5:]) == (want[0], list(want[1:5]), want[5:])
    assert short[0] == R.SM_BUFFER_TOO_SMALL and short[3].tolist() == [R.SM_ERR_ARGUMENT] * 7
    free = av.avro_plan(streams)
    assert free[3].tolist() == [0, 0, 0, 0, 0, R.TRUNCATED, R.NO_HEADER] and free[5] == 4 + 300 + 1 + 4


@pytest.mark.parametrize("name", FILES)
def test_find_sync_equals_the_reference(av, files, name):
    data = files[name]
    w = R.walk(data)
    n = len(data)
    marks = [b.pay_off + b.pay_len + 4 for b in w.blocks]
    starts = sorted({0, 1, w.header_len - 16, w.header_len - 15, n - 16, n - 15, n, n + 5}
                    | {m + d for m in marks[:40] for d in (-1, 0, 1)})
    got = av.find_sync_host([data], [w.sync], [(0, s) for s in starts])
    assert got == [R.find_sync(data, w.sync, s) for s in starts]
    assert got[0] == w.header_len - 16  # the header's own marker: a split at 0 starts at the first block
    assert av.find_sync_host([data, data], [w.sync, bytes(16)], [(1, 0), (0, marks[0])]) == [R.find_sync(data, bytes(16), 0), marks[0]]


# ---- one input per status --------------------------------------------------------------------------------

def test_every_walk_status(av, files):
    seen = set()
    for name, stream, status in R.mutations(files["small_blocks.avro"], files["meta_forms.avro"]):
        s, w = _same_walk(av, stream)
        assert s.status == w.status == status, name
        seen.add(status)
        got = av.avro_plan([stream])
        want = R.plan([stream])
        assert (got[0], [x.tolist() for x in got[1:5]], got[5:]) == (want[0], list(want[1:5]), want[5:]), name
    assert seen == {R.NO_HEADER, R.BAD_HEADER, R.TRUNCATED, R.VARLONG, R.CODEC, R.BLOCK, R.TOO_LARGE, R.SYNC, R.SM_ERR_VARINT}


def test_every_truncation_of_the_first_200_bytes(av, files):
    small = files["small_blocks.avro"]
    head = small[:658]
    for n in range(201):
        s, w = _same_walk(av, small[:n])
        assert s.status == w.status == (R.NO_HEADER if n == 0 else R.TRUNCATED), n
    # and of the bytes around the first blocks: only a cut behind a marker is a file
    w = R.walk(small)
    ends = {w.header_len} | {b.pay_off + b.pay_len + 20 for b in w.blocks}
    for n in range(len(head) - 20, len(head) + 200):
        s, w2 = _same_walk(av, small[:n])
        assert s.status == w2.status and (s.status == 0) == (n in ends), n


# ---- the header writer and the size helpers ----------------------------------------------------------------

def test_write_header_equals_the_reference(av, files):
    schema = b'{"type": "record", "name": "r", "fields": []}'
    for meta in ((), [(b"k", b"v")], [(b"", b""), (b"user.key", bytes(range(256)) * 3)]):
        got = av.write_header(schema, SYNC, meta)
        assert got == R.header(schema, SYNC, meta)
        s, _ = av.index_avro(got)
        assert (s.status, s.nblocks, s.header_length, bytes(s.sync)) == (0, 0, len(got), SYNC)
    assert av.write_header(b'"bytes"', SYNC) == bytes.fromhex(HEX_ONE_BLOCK)[:60]
    assert av.write_header(b"", SYNC) == R.header(b"", SYNC)
    big = os.urandom(70000)  # a three-byte length
    assert av.write_header(big, SYNC) == R.header(big, SYNC)
    with pytest.raises(ValueError):
        av.write_header(schema, b"short")


def test_size_helpers(av):
    assert [av.max_blocks(n) for n in (0, 22, 23, 45, 46, 2300)] == [0, 0, 1, 1, 2, 100]
    compress, _ = R.libsnappy()
    assert len(R.block(b"", 0, SYNC, compress)) == 23  # the shortest block there is
    assert [av.max_block_length(n) for n in (0, 1, 65536)] == [72, 73, 32 + 65536 + 10922 + 40]
    for data, count in ((b"", 0), (b"x" * 100, 2**62), (os.urandom(70000), 1)):  # no block is longer than its bound
        assert len(R.block(data, count, SYNC, compress)) <= av.max_block_length(len(data))
    f = av.lib().sma_streams_scratch_bytes
    assert f(3, 7, 0, 0) > f(3, 6, 0, 0) and f(4, 7, 9, 0) >= f(3, 7, 9, 0) and f(1, 1, 0, 1 << 20) > 1 << 20 and f(0, 0, 0, 0) > 0


def test_status_texts_and_codes(av):
    texts = {code: av.status_message(code) for code in range(80, 89)}
    assert len(set(texts.values())) == 9 and all(t.startswith("Avro file") for t in texts.values())
    assert av.status_message(18) == "Could not decode varint32."  # the main library's
    assert av.status_message(89) == av.status_message(79)  # both unused
    assert av.version().startswith("snappy_mi355x_avro gfx950 ")
    assert (av.SMA_ERR_NO_HEADER, av.SMA_ERR_BAD_HEADER, av.SMA_ERR_TRUNCATED, av.SMA_ERR_VARLONG, av.SMA_ERR_CODEC, av.SMA_ERR_BLOCK,
            av.SMA_ERR_TOO_LARGE, av.SMA_ERR_SYNC, av.SMA_ERR_CRC) == (R.NO_HEADER, R.BAD_HEADER, R.TRUNCATED, R.VARLONG, R.CODEC,
                                                                      R.BLOCK, R.TOO_LARGE, R.SYNC, R.CRC)
    for header in os.listdir(os.path.join(ROOT, "include")):
        text = open(os.path.join(ROOT, "include", header)).read()
        taken = re.findall(r"_ERR_\w+ = (8\d)\b", text)
        assert taken == ([str(c) for c in range(80, 89)] if header == "snappy_mi355x_avro.h" else []), header


# ---- the bindings ----------------------------------------------------------------------------------------

SCALARS = {"size_t": ctypes.c_size_t, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "int": ctypes.c_int,
           "int32_t": ctypes.c_int32, "sm_status": ctypes.c_int32}


def _declarations():
    with open(os.path.join(ROOT, "include", "snappy_mi355x_avro.h")) as f:
        src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S))
    out = {}
    for m in re.finditer(r"([\w\s\*]+?)\b(sma_\w+)\s*\(([^;{]*?)\)\s*;", src, re.S):
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


def test_table_matches_the_header(sm, av):
    binding = importlib.import_module("snappy_jl_amd._binding")
    declared, table = _declarations(), binding.AVRO
    assert len(declared) == 19 and set(declared) == set(table)
    for name, (ret, params) in declared.items():
        restype, argtypes = binding.prototype(table[name])
        assert len(argtypes) == len(params), name
        assert _class(restype) == _c_class(ret), name
        for k, (t, p) in enumerate(zip(argtypes, params)):
            assert t is not None and _class(t) == _c_class(p), "%s: argument %d (%s)" % (name, k, p.strip())
    assert assert_device_elements(binding, declared, table) == 38  # the pointer parameters of the *_device functions, ctx and stream among them
    assert av.AVRO_ABI_SYMBOLS == tuple(table)
    others = [binding.RAW, binding.FRAMING, binding.MULTI, binding.BLOCKS, binding.ORC, binding.PARQUET, binding.PARQUET_WRITE]
    assert not set(table) & set().union(*others)  # a group of its own
    assert [n for n, _ in binding.AvroBlocks._fields_] == list(av.INDEX_KEYS) == ["pay_off", "pay_len", "ulen", "count", "crc", "out_off"]
    assert ctypes.sizeof(binding.AvroSummary) == 48  # sma_summary: 8 + 4 + 4 + 8 + 8 + 16
    for name in table:  # every symbol is exported
        assert getattr(av.lib(), name) is not None


def test_library_links_its_companions_by_name(av):
    out = subprocess.run(["readelf", "-d", av.library_path()], capture_output=True, text=True).stdout
    assert "libsnappy_mi355x_multi.so" in out and "libsnappy_mi355x_parquet.so" in out and "libsnappy_mi355x.so" in out
    assert "$ORIGIN" in out


def test_importing_loads_no_library():
    import sys
    code = ("import sys; sys.path.insert(0, %r); from conftest import load_package; import importlib; "
            "load_package(); m = importlib.import_module('snappy_jl_amd.avro'); "
            "assert m._lib is None and m._ctx == {}; "
            "assert 'libsnappy_mi355x' not in open('/proc/self/maps').read()" % os.path.join(ROOT, "tests"))
    subprocess.run([sys.executable, "-c", code], check=True)


def test_not_built_message(av, monkeypatch, tmp_path):
    monkeypatch.setattr(av, "_lib", None)
    monkeypatch.setattr(av, "LIB_PATH", str(tmp_path / "libsnappy_mi355x_avro.so"))
    with pytest.raises(OSError) as e:
        av.lib()
    assert str(e.value) == "libsnappy_mi355x_avro.so not built (run __graft_entry__.build())"


def test_build_and_smoke_name_the_library():
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert '"csrc", "avro")' in entry and "snappy_jl_amd.avro" in entry and "_avro.so" in entry
    assert entry.index('"csrc", "parquet")') < entry.index('"csrc", "avro")') < entry.index('"oracle")')


# ---- the sanitizer driver --------------------------------------------------------------------------------

def test_host_check_runs_clean(tmp_path):
    r = subprocess.run(["make", "-C", CSRC, "host_check", "OBJ=%s" % tmp_path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sma_host_check ok" in r.stdout
    src = open(os.path.join(CSRC, "sma_host_check.cpp")).read()
    assert all(name in src for name in ("sma_streams_plan", "sma_index", "sma_find_sync", "sma_write_header"))
