"""The Kafka segment library on the GPU (snappy.jl_amd/kafka.py over libsnappy_mi355x_kafka.so):
smk_uncompress_segments_device over the fixtures of tests/golden/kafka/ laid back to back at odd
offsets between guard bytes, one mutated segment per step of the status order, a batch header at
every offset of the walker's window, every input and output alignment, walker-workgroup and
scan-tile edges, the bounds, the fragment path, the encoder against the reference writer, the round
trip, and the host-buffer and Python calls.  Every expected byte comes from the plain-Python
reference (tests/kafka_ref.py), the CPU oracle and pyarrow's libsnappy."""
import functools
import importlib
import json
import os
import struct

import numpy as np
import pytest

import avro_ref
import kafka_ref as R
from conftest import ROOT, load_package, read_testfile

pytestmark = pytest.mark.gpu

GUARD = 0xA5
ARG = R.SM_ERR_ARGUMENT
GOLDEN = os.path.join(ROOT, "tests", "golden", "kafka")
FILES = ("mixed.log", "bigbatch.log", "small_batches.log", "empty.log")


@pytest.fixture(scope="module")
def kf(gpu_available):
    load_package()
    return importlib.import_module("snappy_jl_amd.kafka")


def _torch():
    import torch
    return torch


def _dev():
    return _torch().device("cuda", 0)


def _i64(values):
    return _torch().from_numpy(np.array(values, dtype=np.uint64).view(np.int64)).to(_dev())


def _full(n, value, dtype):
    return _torch().full((max(n, 1),), value, dtype=dtype, device=_dev())


def _oracle():
    import oracle as O
    O.lib()
    return O


def oracle_status(payload):
    """(status, bytes or None) of the raw decoder on `payload`."""
    return _oracle().uncompress_status(payload)


@functools.lru_cache(maxsize=None)
def pa():
    return avro_ref.libsnappy()


@functools.lru_cache(maxsize=None)
def fixture(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def fixture_meta():
    with open(os.path.join(GOLDEN, "kafka_fixture.json")) as f:
        return json.load(f)["files"]


@functools.lru_cache(maxsize=None)
def plain(name):
    """The fixture with every batch rewritten uncompressed, by the reference."""
    return R.uncompress_segment(fixture(name), pa()[1])


@functools.lru_cache(maxsize=None)
def text(n, skip=0):
    t = read_testfile("alice29.txt")
    return (t * ((n + skip) // len(t) + 1))[skip:skip + n]


def patched(seg, at, new):
    return seg[:at] + bytes(new) + seg[at + len(new):]


def recrc(seg, b):
    """The segment with batch b's crc made right again."""
    return patched(seg, b.pos + 17, struct.pack(">I", R.crc32c_fast(seg[b.pos + 21:b.pos + 12 + b.length])))


def small_segment(i=0):
    """A stored, a snappy-java and a raw batch of a few hundred bytes."""
    c = pa()[0]
    return b"".join([R.write_batch(text(200 + i, 10 * i), 3 * i, 0, 0x10),
                     R.write_batch(R.write_xerial(text(700 + 3 * i, 7 * i), c, 256), 3 * i + 1, 0, 2),
                     R.write_batch(c(text(300 + i, 5 * i)), 3 * i + 2, 0, 2)])


# ---- the model: what the rules of the header say of one segment, by the reference and the oracle ------

class Model:
    pass


@functools.lru_cache(maxsize=None)
def model(seg, cap=None, verify=True):
    m = Model()
    w = R.walk(seg)
    p = R.plan(seg, cap)
    m.walk, m.plan, m.pre, m.out_len = w, p, p.status, p.out_len
    m.status, m.pieces, m.table = p.status, [], []
    out_off = 0
    for b in w.batches:
        m.table.append([b.pos, out_off, b.declared, b.codec, 0])
        out_off += R.HEADER + b.declared
    if p.status != 0:
        return m
    first = 0
    for k, b in enumerate(w.batches):
        payload = seg[b.pos + R.HEADER:b.pos + 12 + b.length]
        st, records = 0, payload if b.codec == 0 else b""
        if b.kind == R.XERIAL:
            parts = []
            for o, n, d in R.walk_xerial(payload)[1]:
                cst, data = oracle_status(payload[o:o + n])
                if cst == 0 and len(data) != d:
                    cst = -1
                st = st or cst
                parts.append(data if cst == 0 else b"")
            records = b"".join(parts)
        elif b.kind == R.RAW:
            st, records = oracle_status(payload)
        stored = struct.unpack_from(">I", seg, b.pos + 17)[0]
        if verify and stored != R.crc32c_fast(seg[b.pos + 21:b.pos + 12 + b.length]):
            st = R.CRC
        m.table[k][4] = st
        first = first or st
        if st == 0:
            m.pieces.append((m.table[k][1], R._rewrite(seg, b, records, 0)))
    m.status = first
    return m


def lay(buffers, lead=1, aligns=None):
    """The buffers in one device tensor between guard bytes: directly behind one another with the
    first at an address that is `lead` mod 16, or buffer i at an address that is aligns[i] mod 16."""
    offs, pos = [], lead
    for i, b in enumerate(buffers):
        if aligns is not None:
            pos += (aligns[i] - pos) % 16
        offs.append(pos)
        pos += len(b)
    host = np.full(pos + 16, 0x5A, np.uint8)
    for o, b in zip(offs, buffers):
        host[o:o + len(b)] = np.frombuffer(bytes(b), np.uint8)
    d = _torch().from_numpy(host).to(_dev())
    assert d.data_ptr() % 16 == 0
    return d, offs, [len(b) for b in buffers]


def place(rooms, lead=3, gap=5, aligns=None):
    offs, pos = [], lead
    for i, c in enumerate(rooms):
        if aligns is not None:
            pos += (aligns[i] - pos) % 16
        offs.append(pos)
        pos += c + gap
    return offs, pos


def run_segments(kf, segs, caps=None, verify=True, max_batches=None, max_chunks=None, max_fragments=0, lead=1, aligns=None,
                 out_aligns=None):
    """smk_uncompress_segments_device over `segs`, every optional output asked for, and the checks
    that hold for every call: each segment's status, length, bytes and batch table against the
    model, and guard bytes wherever nothing may be written."""
    torch = _torch()
    k = len(segs)
    if caps is None:
        caps = [model(s, None, verify).out_len for s in segs]
    models = [model(s, c, verify) for s, c in zip(segs, caps)]
    need_batches, need_chunks, _ = R.plan_totals([m.plan for m in models])
    m = need_batches if max_batches is None else max_batches
    mc = need_chunks if max_chunks is None else max_chunks
    over = m < need_batches or mc < need_chunks
    d_in, in_off, in_len = lay(segs, lead, aligns)
    out_off, size = place(caps, aligns=out_aligns)
    d_out = _full(size + 32, GUARD, torch.uint8)
    d_out_len, d_status = _full(k, -7, torch.int64), _full(k, -7, torch.int32)
    d_first = _full(k + 1, -7, torch.int32)
    per = {key: _full(m, -7, torch.int32 if key in ("codec", "status") else torch.int64) for key in kf.BATCH_KEYS}
    kf.uncompress_segments_device(d_in, _i64(in_off), _i64(in_len), m, mc, max_fragments, d_out, _i64(out_off), _i64(caps),
                                  d_out_len, d_status, verify_crc=verify, d_batch_first=d_first, d_batch_in_off=per["in_off"],
                                  d_batch_out_off=per["out_off"], d_batch_len=per["len"], d_batch_codec=per["codec"],
                                  d_batch_status=per["status"])
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    status, out_len, first = d_status.cpu().tolist()[:k], d_out_len.cpu().tolist()[:k], d_first.cpu().tolist()
    got = {key: t.cpu().tolist() for key, t in per.items()}
    want = np.full(out.size, GUARD, np.uint8)
    loose = np.zeros(out.size, bool)  # a failing batch's own range: unspecified bytes
    if over:
        assert status == [ARG] * k and out_len == [0] * k
    else:
        assert status == [mo.status for mo in models]
        assert out_len == [mo.out_len for mo in models]
        assert first == np.concatenate(([0], np.cumsum([len(mo.table) for mo in models]))).tolist()
        for t, mo in enumerate(models):
            rows = [[got[key][first[t] + j] for key in kf.BATCH_KEYS] for j in range(len(mo.table))]
            if mo.pre == 0:
                assert rows == mo.table, t
                loose[out_off[t]:out_off[t] + mo.out_len] = True
                for at, piece in mo.pieces:
                    want[out_off[t] + at:out_off[t] + at + len(piece)] = np.frombuffer(piece, np.uint8)
                    loose[out_off[t] + at:out_off[t] + at + len(piece)] = False
            else:  # not written: the batches that were recorded, with no status
                assert [r[0] for r in rows] == [r[0] for r in mo.table] and [r[3] for r in rows] == [r[3] for r in mo.table]
                assert [r[4] for r in rows] == [0] * len(rows)
    bad = np.nonzero((out != want) & ~loose)[0]
    assert bad.size == 0, "first wrong output byte at %d" % bad[0]
    return models, status, out_len, out, out_off


# ---- decode -----------------------------------------------------------------------------------------

def test_the_fixtures_in_one_batch(kf):
    segs = [fixture(n) for n in FILES]
    models, status, out_len, out, out_off = run_segments(kf, segs, lead=1)
    assert status == [0, 0, 0, 0]
    meta = fixture_meta()
    for name, mo, n, at in zip(FILES, models, out_len, out_off):
        assert n == meta[name]["decoded_bytes"] and out[at:at + n].tobytes() == plain(name)
        assert [[r[0], r[1], r[2], r[3]] for r in mo.table] == \
            [[b["pos"], b["out_off"], b["declared"], b["codec"]] for b in meta[name]["batches"]]
    run_segments(kf, segs[::-1], lead=7, verify=False)


def test_good_beside_bad_by_the_status_order(kf):
    good = small_segment(0)
    w = R.walk(good)
    stored, xerial, raw = w.batches
    chunk = R.walk_xerial(good[xerial.pos + 61:xerial.pos + 12 + xerial.length])[1][1]
    broken_raw = patched(good, raw.pos + 61 + 2, [0xFE, 0xFF, 0xFF])      # its first tag: a copy from far in front of the output
    broken_chunk = patched(good, xerial.pos + 61 + chunk[0] + 2, [0xFE, 0xFF, 0xFF])
    segs = [good,
            good[:-1],                                                      # 1: the walk's error
            patched(good, stored.pos + 22, [0x14]),                         # 1: codec 4
            patched(good, raw.pos + 61, [0xFF] * 5),                        # 1: a failing head (varint)
            patched(good, xerial.pos + 61 + 16, struct.pack(">I", 1 << 30)),  # 1: a failing head (snappy-java walk)
            good,                                                           # 3: no room (below)
            patched(good, stored.pos + 70, [0x00]),                         # 5: a stored batch's checksum
            broken_raw,                                                     # 5: the checksum outranks the decoder
            recrc(broken_raw, raw),                                         # 6: the decoder's status
            recrc(broken_chunk, xerial),                                    # 6: a chunk's
            good]
    caps = [model(s).out_len for s in segs]
    caps[5] -= 1
    models, status, out_len, _, _ = run_segments(kf, segs, caps=caps)
    raw_status = models[8].table[2][4]
    assert raw_status not in (0, R.CRC) and models[9].table[1][4] not in (0, R.CRC)
    assert status == [0, R.TRUNCATED, R.CODEC, R.SM_ERR_VARINT, R.SMB_TRUNCATED, 2, R.CRC, R.CRC, raw_status, models[9].table[1][4], 0]
    assert out_len[1] == len(plain_of(good)) - 61 - raw.declared and out_len[2] == 0
    assert out_len[3] == 61 + stored.declared + 61 + xerial.declared and out_len[4] == 61 + stored.declared
    assert out_len[5] == caps[5] + 1
    # without the checksums the same batches report the decoder's status, and the stored one none
    models, status, _, _, _ = run_segments(kf, segs, caps=caps, verify=False)
    assert status[6:9] == [0, raw_status, raw_status]


def plain_of(seg):
    return R.uncompress_segment(seg, pa()[1])


def test_a_batch_header_at_every_offset_of_the_window(kf):
    c = pa()[0]
    segs = [R.write_batch(text(49 + k, k), k, 0, 0) + R.write_batch(c(text(90, k)), k + 1, 0, 2) +
            R.write_batch(R.write_xerial(text(60, 2 * k), c, 32), k + 2, 0, 2) for k in range(64)]
    assert sorted((61 + 49 + k) % 64 for k in range(64)) == list(range(64))
    _, status, _, _, _ = run_segments(kf, segs)
    assert status == [0] * 64


def test_every_input_and_output_alignment(kf):
    segs = [small_segment(i) for i in range(16)]
    aligns, out_aligns = list(range(16)), [(7 * i + 3) % 16 for i in range(16)]
    assert sorted(out_aligns) == list(range(16))
    _, status, _, _, _ = run_segments(kf, segs, aligns=aligns, out_aligns=out_aligns)
    assert status == [0] * 16


@pytest.mark.parametrize("nsegments,nbatches", [(3, 255), (4, 256), (5, 257)])
def test_walker_workgroups_and_the_scan_tile(kf, nsegments, nbatches):
    c = pa()[0]
    kinds = [lambda i: R.write_batch(text(5 + i % 7, i), i, 0, 0), lambda i: R.write_batch(c(text(9 + i % 5, i)), i, 0, 2),
             lambda i: R.write_batch(R.write_xerial(text(11 + i % 3, i), c, 8), i, 0, 2)]
    counts = [nbatches - 2 * (nsegments - 1)] + [2] * (nsegments - 1)
    segs, at = [], 0
    for n in counts:
        segs.append(b"".join(kinds[(at + j) % 3](at + j) for j in range(n)))
        at += n
    models, status, _, _, _ = run_segments(kf, segs)
    assert status == [0] * nsegments and sum(len(m.table) for m in models) == nbatches


def test_the_bounds_exact_and_one_short(kf):
    segs = [small_segment(1), fixture("empty.log"), small_segment(2), R.write_batch(R.XERIAL_HEADER + bytes([0, 0, 0, 1, 0]), 9, 0, 2)]
    plans = [model(s).plan for s in segs]
    batches, chunks, _ = R.plan_totals(plans)
    assert batches == 7 and chunks > 4
    run_segments(kf, segs, max_batches=batches, max_chunks=chunks)
    for bounds in ({"max_batches": batches - 1}, {"max_chunks": chunks - 1}, {"max_batches": 0}, {"max_chunks": 0}):
        _, status, out_len, _, _ = run_segments(kf, segs, **bounds)
        assert status == [ARG] * 4 and out_len == [0] * 4
    caps = [p.out_len for p in plans]
    caps[2] -= 1
    _, status, out_len, _, _ = run_segments(kf, segs, caps=caps)
    assert status == [0, 0, 2, 0] and out_len[2] == caps[2] + 1
    # with no room anywhere only the snappy-java stream of no bytes takes its chunk's slot: one is enough, none is not
    _, status, out_len, _, _ = run_segments(kf, segs, caps=[0, 0, 0, 0], max_chunks=1)
    assert status == [2, 0, 2, 2] and out_len == [p.out_len for p in plans]
    _, status, _, _, _ = run_segments(kf, segs, caps=[0, 0, 0, 0], max_chunks=0)
    assert status == [ARG] * 4


def test_bigbatch_decodes_by_fragments_when_it_can(kf):
    seg = fixture("bigbatch.log")
    x, r = fixture_meta()["bigbatch.log"]["fragments"]
    assert (x, r) == (2, 3)
    for max_fragments, indexed in ((0, 0), (3, 2), (2, 1), (1, 0)):
        _, status, out_len, out, out_off = run_segments(kf, [seg], max_fragments=max_fragments)
        assert status == [0] and out[out_off[0]:out_off[0] + out_len[0]].tobytes() == plain("bigbatch.log")
        assert kf.last_indexed(0) == indexed


# ---- encode -----------------------------------------------------------------------------------------

def run_compress(kf, segs, mode="reference", max_batches=None, max_blocks=None, stage_bytes=None, lead=1, aligns=None):
    """smk_compress_segments_device over `segs`: (statuses, the segments written, or None)."""
    torch = _torch()
    k = len(segs)
    walks = [R.walk(s) for s in segs]
    pays = [b.length - 49 for w in walks if w.status == 0 for b in w.batches if b.codec == 0 and b.length > 49]
    need = (sum(len(w.batches) for w in walks), sum((p + 65535) // 65536 for p in pays), sum(R.stage_length(p) for p in pays))
    m, mb, sb = (need[i] if v is None else v for i, v in enumerate((max_batches, max_blocks, stage_bytes)))
    over = m < need[0] or mb < need[1] or sb < need[2]
    rooms = [R.max_segment_length(len(s), len(w.batches)) for s, w in zip(segs, walks)]
    d_in, in_off, in_len = lay(segs, lead, aligns)
    out_off, size = place(rooms)
    d_out = _full(size + 32, GUARD, torch.uint8)
    d_out_len, d_status = _full(k, -7, torch.int64), _full(k, -7, torch.int32)
    kf.compress_segments_device(d_in, _i64(in_off), _i64(in_len), m, mb, sb, d_out, _i64(out_off), d_out_len, d_status, mode=mode)
    torch.cuda.synchronize()
    out, status, out_len = d_out.cpu().numpy(), d_status.cpu().tolist()[:k], d_out_len.cpu().tolist()[:k]
    written = np.zeros(out.size, bool)
    res = []
    for t in range(k):
        if over:
            assert status[t] == ARG and out_len[t] == 0
        else:
            assert status[t] == walks[t].status and (status[t] == 0 or out_len[t] == 0) and out_len[t] <= rooms[t]
        written[out_off[t]:out_off[t] + out_len[t]] = True
        res.append(out[out_off[t]:out_off[t] + out_len[t]].tobytes() if status[t] == 0 else None)
    assert (out[~written] == GUARD).all()
    return status, res


def mode_compress(mode):
    if mode == "reference":
        return _oracle().compress
    sm = load_package()
    return lambda piece: sm.compress_batch([piece], mode=mode)[0]


@pytest.mark.parametrize("mode", ["reference", "fast", "dense"])
def test_encode_equals_the_reference_writer_and_round_trips(kf, mode):
    """Byte for byte the reference's snappy-java writer at 64 KiB pieces over the mode's own raw
    compressor; already-compressed batches pass through; and for every segment S of uncompressed
    batches with valid crcs decode(encode(S)) == S, header and crc included."""
    segs = [plain(n) for n in FILES] + [fixture("mixed.log"), plain_of(small_segment(3))]
    status, enc = run_compress(kf, segs, mode=mode, lead=5)
    assert status == [0] * len(segs)
    c = mode_compress(mode)
    for s, e in zip(segs, enc):
        assert e == R.compress_segment(s, c, 65536)
    mixed = R.walk(fixture("mixed.log"))
    for b in mixed.batches:
        if b.codec == 2:  # unchanged, crc included
            assert fixture("mixed.log")[b.pos:b.pos + 12 + b.length] in enc[4]
    assert len(enc[0]) < len(segs[0]) and enc[3] == b""
    _, st, out_len, out, out_off = run_segments(kf, enc, max_fragments=8)
    assert st == [0] * len(segs)
    for s, n, at in zip(segs[:4] + segs[5:], out_len[:4] + out_len[5:], out_off[:4] + out_off[5:]):
        assert out[at:at + n].tobytes() == s
    assert out[out_off[4]:out_off[4] + out_len[4]].tobytes() == plain("mixed.log")


def test_encoder_bounds_and_errors(kf):
    segs = [plain_of(small_segment(4)), b"", patched(plain("mixed.log"), 22, [1]), plain("bigbatch.log")[:61 + 100000]]
    walks = [R.walk(s) for s in segs]
    assert [w.status for w in walks] == [0, 0, R.CODEC, 0]
    status, enc = run_compress(kf, segs, aligns=[3, 0, 9, 14])
    assert status == [0, 0, R.CODEC, 0] and enc[1] == b"" and enc[3] == R.compress_segment(segs[3], _oracle().compress)
    pays = [b.length - 49 for w in walks if w.status == 0 for b in w.batches if b.length > 49]
    batches, blocks, stage = sum(len(w.batches) for w in walks), sum((p + 65535) // 65536 for p in pays), sum(map(R.stage_length, pays))
    assert blocks == 3 + 2 and kf.compress_plan(segs)[4:] == (batches, blocks, stage)
    for bounds in ({"max_batches": batches - 1}, {"max_blocks": blocks - 1}, {"stage_bytes": stage - 1}):
        status, enc = run_compress(kf, segs, **bounds)
        assert status == [ARG] * 4 and enc == [None] * 4


# ---- the host-buffer twins and the Python calls ---------------------------------------------------------

def test_python_calls_over_host_buffers(kf):
    segs = [fixture(n) for n in FILES] + [small_segment(5)]
    res = kf.uncompress_segments(segs)
    for s, (data, table) in zip(segs, res):
        mo = model(s)
        assert data == plain_of(s) and [list(r) for r in zip(*(table[key].tolist() for key in kf.BATCH_KEYS))] == mo.table
    assert kf.uncompress_segments([]) == [] and kf.compress_segments([]) == []
    data, table = kf.uncompress_segment(b"")
    assert data == b"" and all(len(a) == 0 for a in table.values())
    recs, table = kf.uncompress_segment(fixture("mixed.log"), records=True)
    w = R.walk(fixture("mixed.log"))
    assert recs == [R.records_of(fixture("mixed.log"), b, pa()[1]) for b in w.batches]
    # a failing segment beside good ones: its status and number, or None in its place
    bad = patched(segs[4], 70, [0])
    with pytest.raises(kf.KafkaError) as e:
        kf.uncompress_segments([segs[4], bad])
    assert e.value.code == R.CRC and e.value.index == 1
    res, codes = kf.uncompress_segments([segs[4], bad, segs[4][:-1]], statuses=True)
    assert codes == [0, R.CRC, R.TRUNCATED] and res[1][0] is None and res[0][0] == plain_of(segs[4])
    assert kf.uncompress_segment(bad, verify_crc=False)[0] == plain_of(bad)  # (under a crc of its own)
    with pytest.raises(kf.KafkaError) as e:
        kf.uncompress_segment(segs[4][:-1])
    assert e.value.code == R.TRUNCATED and e.value.index is None
    # write_batch, compress and back
    seg = kf.write_batch(text(70000), 0, 0, 0) + kf.write_batch(b"", 1) + kf.write_batch(text(10, 3), 1, 2, 0x20)
    enc = kf.compress_segment(seg, mode="reference")
    assert enc == R.compress_segment(seg, _oracle().compress) and len(enc) < len(seg)
    assert kf.compress_segments([seg, b"", enc], mode="reference") == [enc, b"", enc]
    assert kf.uncompress_segment(enc)[0] == seg
    with pytest.raises(kf.KafkaError) as e:
        kf.compress_segments([seg, patched(seg, 22, [3])])
    assert e.value.code == R.CODEC and e.value.index == 1
