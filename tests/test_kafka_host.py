"""The Kafka segment library's host side (snappy.jl_amd/kafka.py over include/snappy_mi355x_kafka.h):
the reference of tests/kafka_ref.py pinned by answers that are not its own, then smk_index, the two
plans and smk_write_batch against it on the fixtures and on one mutation per rule, the KAFKA table
against the header, and the two device wrappers' argument checks on CPU tensors.  No GPU."""
import ctypes
import hashlib
import importlib
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from prototype_types import assert_device_elements

import avro_ref
import kafka_ref as R
from conftest import ROOT

CSRC = os.path.join(ROOT, "snappy.jl_amd", "csrc", "kafka")
GOLDEN = os.path.join(ROOT, "tests", "golden", "kafka")
FILES = ("mixed.log", "bigbatch.log", "small_batches.log", "empty.log")
RFC3720 = [(bytes(32), 0x8A9136AA), (b"\xff" * 32, 0x62A8AB43), (bytes(range(32)), 0x46DD794E),
           (bytes(range(31, -1, -1)), 0x113FDB5C)]
# One batch by hand: baseOffset 5, batchLength 52, partitionLeaderEpoch 1, magic 2, the crc,
# attributes 0, lastOffsetDelta 0, baseTimestamp 1000, maxTimestamp 1001, producerId -1,
# producerEpoch -1, baseSequence -1, recordsCount 1, the records bytes "abc".
HEX_BODY = ("0000" "00000000" "00000000000003e8" "00000000000003e9" "ffffffffffffffff" "ffff" "ffffffff" "00000001" "616263")
HEX_HEAD = "0000000000000005" "00000034" "00000001" "02"


@pytest.fixture(scope="module")
def kf(sm):
    return importlib.import_module("snappy_jl_amd.kafka")


@pytest.fixture(scope="module")
def snappy():
    return avro_ref.libsnappy()


@pytest.fixture(scope="module")
def fixtures():
    with open(os.path.join(GOLDEN, "kafka_fixture.json")) as f:
        meta = json.load(f)["files"]
    data = {}
    for name in FILES:
        with open(os.path.join(GOLDEN, name), "rb") as f:
            data[name] = f.read()
    return data, meta


# ---- the reference, pinned ---------------------------------------------------------------------------

def test_reference_crc32c_is_rfc3720s():
    for data, want in RFC3720:
        assert R.crc32c(data) == want and R.crc32c_fast(data) == want
    assert R.crc32c(b"123456789") == 0xE3069283 and R.crc32c(b"") == 0


def test_reference_writes_the_batch_assembled_by_hand():
    body = bytes.fromhex(HEX_BODY)
    want = bytes.fromhex(HEX_HEAD) + struct.pack(">I", R.crc32c(body)) + body
    assert len(want) == 64
    got = R.write_batch(b"abc", 5, 1, 0, R.tail_fields(0, 1000, 1001, -1, -1, -1, 1))
    assert got == want
    w = R.walk(got)
    assert w == R.Walk(0, [R.Batch(0, 52, 0, R.STORED, 3, 0, 0, 0)], 64)


def test_reference_snappy_java_header_and_chunks(snappy):
    compress, uncompress = snappy
    data = bytes(range(256)) * 300
    x = R.write_xerial(data, compress, 32768)
    assert x[:16] == bytes.fromhex("82534e4150505900" "00000001" "00000001")
    st, chunks, total = R.walk_xerial(x)
    assert st == 0 and total == len(data) and [d for _, _, d in chunks] == [32768, 32768, 76800 - 65536]
    assert chunks[0][0] == 20 and struct.unpack_from(">I", x, 16)[0] == chunks[0][1]
    assert R.read_xerial(x, uncompress) == data
    y = R.write_xerial(data, compress, 32768, repeat_header=True)
    assert len(y) == len(x) + 32 and R.read_xerial(y, uncompress) == data


def test_fixtures_are_the_recipes(fixtures, snappy):
    data, meta = fixtures
    assert set(meta) == set(FILES)
    for name in FILES:
        m = meta[name]
        assert len(data[name]) == m["file_bytes"] <= 300000 and hashlib.sha256(data[name]).hexdigest() == m["sha256_file"]
        w = R.walk(data[name])
        assert w.status == 0 and len(w.batches) == len(m["batches"])
        decoded = R.uncompress_segment(data[name], snappy[1])
        assert hashlib.sha256(decoded).hexdigest() == m["sha256_decoded"]
    kinds = [b["kind"] for b in meta["mixed.log"]["batches"]]
    assert kinds == [R.STORED, R.XERIAL, R.RAW, R.STORED, R.STORED, R.STORED, R.STORED, R.STORED, R.XERIAL]
    assert [b["declared"] for b in meta["bigbatch.log"]["batches"]] == [100000, 150000]
    assert len(meta["small_batches.log"]["batches"]) == 300 and data["empty.log"] == b""


# ---- smk_index -------------------------------------------------------------------------------------------

def _agrees(kf, seg):
    """smk_index against the reference walker on `seg`; returns the summary's status."""
    s, a = kf.index_segment(seg)
    w = R.walk(seg)
    st, total = R.index_status(w)
    assert (s.status, s.nbatches, s.valid_length, s.total_length) == (st, len(w.batches), w.valid, total)
    assert a["pos"].tolist() == [b.pos for b in w.batches] and a["length"].tolist() == [b.length for b in w.batches]
    assert a["codec"].tolist() == [b.codec for b in w.batches] and a["status"].tolist() == [b.status for b in w.batches]
    assert a["declared"].tolist() == [b.declared for b in w.batches]
    return s.status


def test_index_equals_the_reference_on_the_fixtures(kf, fixtures):
    data, meta = fixtures
    for name in FILES:
        assert _agrees(kf, data[name]) == 0
        _, a = kf.index_segment(data[name])
        assert a["pos"].tolist() == [b["pos"] for b in meta[name]["batches"]]
        assert a["declared"].tolist() == [b["declared"] for b in meta[name]["batches"]]
    s, a = kf.index_segment(data["mixed.log"], max_batches=3)
    assert s.status == 2 and s.nbatches == 9 and len(a["pos"]) == 3


def _patched(seg, at, new):
    return seg[:at] + bytes(new) + seg[at + len(new):]


def test_index_equals_the_reference_on_a_mutation_per_rule(kf, fixtures, snappy):
    data, _ = fixtures
    seg = data["mixed.log"]
    w = R.walk(seg)
    second, third, last = w.batches[1], w.batches[2], w.batches[-1]
    # the walk: each error at its first possible byte
    assert _agrees(kf, seg[:16]) == R.TRUNCATED and _agrees(kf, seg[:17]) == R.TRUNCATED
    assert _agrees(kf, seg[:second.pos + 16]) == R.TRUNCATED
    cut = seg[:last.pos + 12 + last.length - 1]  # a partial last batch: a fetch response
    assert _agrees(kf, cut) == R.TRUNCATED
    s, _ = kf.index_segment(cut)
    assert s.valid_length == last.pos and s.nbatches == 8 and _agrees(kf, cut[:s.valid_length]) == 0
    for magic in (0, 1, 3):
        assert _agrees(kf, _patched(seg, second.pos + 16, [magic])) == R.MAGIC
    assert _agrees(kf, _patched(seg, 16, [1])) == R.MAGIC
    for codec in (1, 3, 4, 5, 6, 7):
        assert _agrees(kf, _patched(seg, second.pos + 22, [codec])) == R.CODEC
    assert _agrees(kf, _patched(seg, second.pos + 8, struct.pack(">I", 48))) == R.LENGTH
    assert _agrees(kf, _patched(seg, second.pos + 8, struct.pack(">I", 0x80000000))) == R.LENGTH
    assert _agrees(kf, _patched(seg, second.pos + 8, struct.pack(">I", 0xFFFFFFFF))) == R.LENGTH
    assert _agrees(kf, _patched(seg, second.pos + 8, struct.pack(">I", 0x7FFFFFFF))) == R.TRUNCATED
    assert _agrees(kf, _patched(seg, last.pos + 8, struct.pack(">I", last.length + 1))) == R.TRUNCATED
    # a length one short makes the next batch start a byte early: its magic byte is then another
    assert _agrees(kf, _patched(seg, 8, struct.pack(">I", w.batches[0].length - 1))) in (R.MAGIC, R.LENGTH, R.TRUNCATED, R.CODEC)
    # the heads
    pay = second.pos + 61
    assert _agrees(kf, _patched(seg, pay + 11, [0])) == R.SMB_BAD_HEADER            # version 0
    assert _agrees(kf, _patched(seg, pay + 16, struct.pack(">I", 0x7FFFFFF0))) == R.SMB_TRUNCATED
    assert _agrees(kf, _patched(seg, pay + 20, [0x80] * 5)) == R.SM_ERR_VARINT      # the first chunk's varint
    assert _agrees(kf, _patched(seg, pay + 7, [1])) in (0, R.SM_ERR_VARINT)          # no magic: a raw stream, 82 53 as its varint
    assert _agrees(kf, _patched(seg, third.pos + 61, [0xFF] * 5)) == R.SM_ERR_VARINT
    assert _agrees(kf, _patched(seg, third.pos + 61, bytes.fromhex("cfffffff07"))) == R.TOO_LARGE
    assert _agrees(kf, _patched(seg, third.pos + 61, bytes.fromhex("ceffffff07"))) == 0
    # a snappy batch of exactly the 8 magic bytes; of 7 of them; an uncompressed batch that starts with them
    assert _agrees(kf, R.write_batch(R.XERIAL_MAGIC, attributes=2)) == R.SMB_TRUNCATED
    assert _agrees(kf, R.write_batch(R.XERIAL_MAGIC[:7], attributes=2)) == 0
    assert _agrees(kf, R.write_batch(R.XERIAL_HEADER, attributes=0)) == 0
    assert _agrees(kf, R.write_batch(R.XERIAL_HEADER, attributes=2)) == 0            # no chunks: no records
    # the walk's error outranks a failing head in front of it; a failing head does not stop the walk
    bad = _patched(seg, third.pos + 61, [0xFF] * 5)
    assert _agrees(kf, _patched(bad, last.pos + 22, [4])) == R.CODEC
    s, a = kf.index_segment(bad)
    assert s.nbatches == 9 and s.total_length == 61 + 2000 + 61 + 100000 and a["status"].tolist().count(R.SM_ERR_VARINT) == 1


# ---- the plans -------------------------------------------------------------------------------------------

def test_segments_plan_equals_the_reference(kf, fixtures):
    data, meta = fixtures
    seg = data["mixed.log"]
    third = R.walk(seg).batches[2]
    segs = [data[n] for n in FILES] + [_patched(seg, third.pos + 61, [0xFF] * 5), seg[:-1], _patched(seg, 22, [3])]
    plans = [R.plan(s) for s in segs]
    batches, chunks, fragments = R.plan_totals(plans)
    rc, first, out_len, status, tb, tc, tf = kf.segments_plan(segs)
    assert rc == 0 and (tb, tc, tf) == (batches, chunks, fragments)
    assert status.tolist() == [p.status for p in plans] == [0, 0, 0, 0, R.SM_ERR_VARINT, R.TRUNCATED, R.CODEC]
    assert out_len.tolist() == [p.out_len for p in plans]
    assert first.tolist() == np.concatenate(([0], np.cumsum([p.batches for p in plans]))).tolist()
    for name, n in zip(FILES, out_len.tolist()):
        assert n == meta[name]["decoded_bytes"]
    assert chunks == sum(meta[n]["chunks"] for n in FILES) and fragments == sum(meta[n]["fragments"][0] for n in FILES)
    # each bound exact and exceeded by one
    assert kf.segments_plan(segs, max_batches=batches, max_chunks=chunks)[0] == 0
    for bounds in ({"max_batches": batches - 1, "max_chunks": chunks}, {"max_batches": batches, "max_chunks": chunks - 1}):
        rc, _, out_len, status, *_ = kf.segments_plan(segs, **bounds)
        assert rc == 2 and set(status.tolist()) == {R.SM_ERR_ARGUMENT} and not out_len.any()
    # capacities: exact, one short, none
    caps = [p.out_len for p in plans]
    caps[1] -= 1
    caps[2] = 0
    rc, _, out_len, status, tb, tc, tf = kf.segments_plan(segs, out_cap=caps)
    want = [R.plan(s, c) for s, c in zip(segs, caps)]
    assert rc == 0 and status.tolist() == [p.status for p in want] and status.tolist()[:3] == [0, 2, 2]
    assert out_len.tolist() == [p.out_len for p in want] and (tb, tc, tf) == R.plan_totals(want)


def test_compress_plan_equals_the_reference(kf, fixtures, snappy):
    data, meta = fixtures
    plain = [R.uncompress_segment(data[n], snappy[1]) for n in FILES]
    segs = plain + [data["mixed.log"], _patched(plain[0], 22, [1])]
    rc, first, room, status, tb, blocks, stage = kf.compress_plan(segs)
    walks = [R.walk(s) for s in segs]
    assert rc == 0 and status.tolist() == [w.status for w in walks] == [0, 0, 0, 0, 0, R.CODEC]
    assert tb == sum(len(w.batches) for w in walks)
    assert room.tolist() == [R.max_segment_length(len(s), len(w.batches)) for s, w in zip(segs, walks)]
    pays = [b.length - 49 for w in walks if w.status == 0 for b in w.batches if b.codec == 0 and b.length > 49]
    assert blocks == sum((p + 65535) // 65536 for p in pays) and stage == sum(R.stage_length(p) for p in pays)
    assert kf.stage_length(0) == 0 and kf.stage_length(1) == 64 and kf.stage_length(65536) == 76512
    assert kf.compress_plan(segs, max_batches=tb)[0] == 0
    rc, _, _, status, *_ = kf.compress_plan(segs, max_batches=tb - 1)
    assert rc == 2 and set(status.tolist()) == {R.SM_ERR_ARGUMENT}
    # the room holds the reference's encoding of every fixture, with the bound to spare for the worst case
    for s, r in zip(plain, room.tolist()):
        assert len(R.compress_segment(s, snappy[0])) <= r


def test_write_batch_equals_the_reference(kf):
    body = bytes.fromhex(HEX_BODY)
    assert kf.write_batch(b"abc", 5, 1, 0, R.tail_fields(0, 1000, 1001, -1, -1, -1, 1)) == \
        bytes.fromhex(HEX_HEAD) + struct.pack(">I", R.crc32c(body)) + body
    for records, attributes in ((b"", 0), (b"\x00", 0x20), (bytes(range(256)) * 40, 0x18), (R.XERIAL_MAGIC, 0xFFF8)):
        tail = R.tail_fields(7, 1 << 40, (1 << 40) + 9, 12345, 6, 700, 8)
        assert kf.write_batch(records, 1 << 50, 0xFFFFFFFF, attributes, tail) == \
            R.write_batch(records, 1 << 50, -1, attributes, tail)
    assert kf.write_batch(b"xyz") == R.write_batch(b"xyz")  # the default tail: no producer, no records counted
    with pytest.raises(kf.KafkaError) as e:
        kf.write_batch(b"abc", attributes=2)  # the codec bits are the library's
    assert e.value.code == R.SM_ERR_ARGUMENT
    with pytest.raises(ValueError):
        kf.write_batch(b"abc", tail=bytes(37))


def test_status_messages_and_version(kf):
    for code in range(104, 110):
        assert kf.status_message(code).startswith("Log segment: ")
    assert kf.status_message(57).startswith("Log segment: ") and kf.status_message(18) == "Could not decode varint32."
    assert kf.status_message(110) == kf.status_message(95)  # both unused
    assert kf.version().startswith("snappy_mi355x_kafka gfx950 ")
    assert (kf.SMK_ERR_TRUNCATED, kf.SMK_ERR_MAGIC, kf.SMK_ERR_LENGTH, kf.SMK_ERR_CODEC, kf.SMK_ERR_TOO_LARGE, kf.SMK_ERR_CRC) == \
        (R.TRUNCATED, R.MAGIC, R.LENGTH, R.CODEC, R.TOO_LARGE, R.CRC)
    for header in os.listdir(os.path.join(ROOT, "include")):
        text = open(os.path.join(ROOT, "include", header)).read()
        taken = re.findall(r"_ERR_\w+ = (10[4-9]|1[1-9]\d)\b", text)
        assert taken == ([str(c) for c in range(104, 110)] if header == "snappy_mi355x_kafka.h" else []), header


# ---- the bindings ----------------------------------------------------------------------------------------

SCALARS = {"size_t": ctypes.c_size_t, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "int": ctypes.c_int,
           "int32_t": ctypes.c_int32, "sm_status": ctypes.c_int32}


def _declarations():
    with open(os.path.join(ROOT, "include", "snappy_mi355x_kafka.h")) as f:
        src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S))
    out = {}
    for m in re.finditer(r"([\w\s\*]+?)\b(smk_\w+)\s*\(([^;{]*?)\)\s*;", src, re.S):
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


def test_table_matches_the_header(sm, kf):
    binding = importlib.import_module("snappy_jl_amd._binding")
    declared, table = _declarations(), binding.KAFKA
    assert len(declared) == 16 and set(declared) == set(table)
    for name, (ret, params) in declared.items():
        restype, argtypes = binding.prototype(table[name])
        assert len(argtypes) == len(params), name
        assert _class(restype) == _c_class(ret), name
        for k, (t, p) in enumerate(zip(argtypes, params)):
            assert t is not None and _class(t) == _c_class(p), "%s: argument %d (%s)" % (name, k, p.strip())
    assert assert_device_elements(binding, declared, table) == 16 + 9  # the pointer parameters of the *_device functions, ctx and stream among them
    assert kf.KAFKA_ABI_SYMBOLS == tuple(table)
    assert not set(table) & set().union(*binding.TABLES)  # a group of its own
    assert ctypes.sizeof(kf.KafkaSummary) == 24  # smk_summary: 8 + 8 + 4 + 4
    for name in table:  # every symbol is exported
        assert getattr(kf.lib(), name) is not None


def test_tables_tuple_is_unchanged(sm):
    binding = importlib.import_module("snappy_jl_amd._binding")
    assert binding.TABLES == (binding.RAW, binding.FRAMING, binding.MULTI, binding.MULTI_RANGE, binding.BLOCKS, binding.ORC,
                              binding.PARQUET, binding.PARQUET_WRITE, binding.AVRO, binding.TABLE)
    assert binding.MORE_TABLES == (binding.KAFKA,)
    assert len({n for t in binding.TABLES for n in t if n.endswith("_device")}) == 36
    assert [k for k, _, _ in binding.tensor_plan("smk_compress_segments_device")] == [1, 2, 3, 8, 9, 10, 11]
    assert binding.tensor_plan("sm_compress_batch_device")[0] == (1, "b", None)  # TABLES is still searched


def test_library_links_its_companions_by_name(kf):
    out = subprocess.run(["readelf", "-d", kf.library_path()], capture_output=True, text=True).stdout
    for name in ("multi", "blocks", "framing"):
        assert "libsnappy_mi355x_%s.so" % name in out
    assert "libsnappy_mi355x.so" in out and "$ORIGIN" in out


# ---- the device wrappers, on CPU tensors -------------------------------------------------------------

NS, MB = 3, 5
# (argument name, position in the C function, element letter, elements, elements the table ties it to or None)
DECODE = [("d_in", 1, "b", 64, None), ("d_in_off", 2, "d", NS, NS), ("d_in_len", 3, "d", NS, NS), ("d_out", 9, "b", 64, None),
          ("d_out_off", 10, "d", NS, NS), ("d_out_cap", 11, "d", NS, NS), ("d_out_len", 12, "d", NS, NS),
          ("d_status", 13, "t", NS, NS), ("d_batch_first", 14, "w", NS + 1, NS + 1), ("d_batch_in_off", 15, "d", MB, MB),
          ("d_batch_out_off", 16, "d", MB, MB), ("d_batch_len", 17, "d", MB, MB), ("d_batch_codec", 18, "w", MB, MB),
          ("d_batch_status", 19, "t", MB, MB)]
ENCODE = [("d_in", 1, "b", 64, None), ("d_in_off", 2, "d", NS, NS), ("d_in_len", 3, "d", NS, NS), ("d_out", 8, "b", 64, None),
          ("d_out_off", 9, "d", NS, NS), ("d_out_len", 10, "d", NS, NS), ("d_status", 11, "t", NS, NS)]
DTYPE = {"b": "uint8", "w": "int32", "d": "int64", "t": "int32"}
WRONG = {"b": "int32", "w": "int64", "d": "int32", "t": "int64"}


@pytest.mark.parametrize("wrapper,cname,spec,others", [
    ("uncompress_segments_device", "smk_uncompress_segments_device", DECODE, {"max_batches": MB, "max_chunks": 4, "max_fragments": 0}),
    ("compress_segments_device", "smk_compress_segments_device", ENCODE, {"max_batches": MB, "max_blocks": 4, "stage_bytes": 1024}),
])
def test_device_wrappers_judge_every_tensor(kf, monkeypatch, wrapper, cname, spec, others):
    import torch
    binding = importlib.import_module("snappy_jl_amd._binding")
    assert [k for k, _, _ in binding.tensor_plan(cname)] == [p for _, p, _, _, _ in spec]
    monkeypatch.setattr(kf, "_lib", None)  # nothing is loaded or launched: every call ends in the checks
    before = dict(kf._ctx)
    call = getattr(kf, wrapper)

    def make(letter, n, wrong=False, strided=False):
        dtype = getattr(torch, (WRONG if wrong else DTYPE)[letter])
        return torch.zeros(2 * n, dtype=dtype)[::2] if strided else torch.zeros(n, dtype=dtype)

    good = {name: make(letter, n) for name, _, letter, n, _ in spec}
    with pytest.raises(TypeError) as e:  # checks 1 to 3 take the set; check 4 refuses its first tensor
        call(**good, **others)
    assert str(e.value).startswith("%s argument 1: expected a CUDA tensor" % cname)
    for name, position, letter, n, tied in spec:
        trials = [(TypeError, make(letter, n, wrong=True)), (ValueError, make(letter, n, strided=True))]
        if tied and name != "d_in_len":
            trials.append((ValueError, make(letter, tied - 1)))
        for error, value in trials:
            with pytest.raises(error) as e:
                call(**dict(good, **{name: value}), **others)
            assert str(e.value).startswith("%s argument %d: expected" % (cname, position)), (name, str(e.value))
            assert "CUDA" not in str(e.value)
    # d_in_len gives the count: a shorter one makes every array it ties one element too long, which is
    # no error; a longer one makes d_in_off short
    with pytest.raises(ValueError) as e:
        call(**dict(good, d_in_len=make("d", NS + 1)), **others)
    assert str(e.value).startswith("%s argument 2: expected at least %d elements, given %d" % (cname, NS + 1, NS))
    with pytest.raises(TypeError) as e:
        call(**dict(good, d_in_len=None), **others)
    assert "gives a count or a capacity of the call is None" in str(e.value)
    if wrapper == "uncompress_segments_device":  # the optional arrays may be left out
        few = {k: v for k, v in good.items() if not k.startswith("d_batch_")}
        with pytest.raises(TypeError) as e:
            call(**few, **others)
        assert "expected a CUDA tensor" in str(e.value)
    assert kf._lib is None and kf._ctx == before
