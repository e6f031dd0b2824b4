"""The Avro container library on the GPU (snappy.jl_amd/avro.py over libsnappy_mi355x_avro.so):
sma_uncompress_streams_device over the fixtures of tests/golden/avro/ and over mixed batches laid
back to back at odd alignments between guard bytes, the slot bounds, scan-tile and walker-workgroup
edges, the CRC-32 verdicts, block runs, the sync search against bytes.find, the encoder in its three
modes against the reference writer, and the host-buffer and Python calls.  Every expected value
comes from the plain-Python reference (tests/avro_ref.py), the CPU oracle, pyarrow's libsnappy and
zlib."""
import functools
import importlib
import os
import zlib

import numpy as np
import pytest

import avro_ref as R
from conftest import ROOT, load_package, read_testfile

pytestmark = pytest.mark.gpu

GUARD = 0xA5
ARG = R.SM_ERR_ARGUMENT
GOLDEN = os.path.join(ROOT, "tests", "golden", "avro")
FILES = ("blocks_64k.avro", "small_blocks.avro", "bigblock.avro", "meta_forms.avro")
SCHEMA = b'{"type": "record", "name": "r", "fields": [{"name": "b", "type": "bytes"}]}'
SYNC = bytes(range(0xC0, 0xD0))


@pytest.fixture(scope="module")
def av(gpu_available):
    load_package()
    return importlib.import_module("snappy_jl_amd.avro")


def _torch():
    import torch
    return torch


def _dev():
    return _torch().device("cuda", 0)


def _i64(values):
    return _torch().from_numpy(np.array(values, dtype=np.uint64).view(np.int64)).to(_dev())


def _i32(values):
    return _torch().from_numpy(np.array(values, dtype=np.uint32).view(np.int32)).to(_dev())


def _u8(data):
    return _torch().from_numpy(np.frombuffer(bytes(data) or b"\0", np.uint8).copy()).to(_dev())


def _oracle():
    import oracle as O
    O.lib()
    return O


@functools.lru_cache(maxsize=None)
def fixture(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def text(n):
    t = read_testfile("alice29.txt")
    return (t * (n // len(t) + 1))[:n]


def lay(buffers, lead=1):
    """The buffers directly behind one another in one device tensor, the first at an address that is
    `lead` mod 16, guard bytes around them: (tensor, offsets, lengths)."""
    offs, pos = [], lead
    for b in buffers:
        offs.append(pos)
        pos += len(b)
    host = np.full(pos + 16, 0x5A, np.uint8)
    for o, b in zip(offs, buffers):
        host[o:o + len(b)] = np.frombuffer(bytes(b), np.uint8)
    d = _torch().from_numpy(host).to(_dev())
    assert d.data_ptr() % 16 == 0
    return d, offs, [len(b) for b in buffers]


# ---- decode -----------------------------------------------------------------------------------------

class Model:
    """What the device call owes one stream with `cap` bytes of room."""

    def __init__(self, stream, cap, kind=R.FILE, sync=None, verify=True):
        w = R.walk(stream, kind, sync)
        self.walk, self.length, self.objects = w, w.total, w.objects
        self.status = w.status or (R.SM_BUFFER_TOO_SMALL if w.total > cap else 0)
        self.slots = len(w.blocks) if self.status == 0 else 0
        self.pieces, self.block_status = [], []
        if self.slots:
            for b in w.blocks:
                st, data = block_verdict(bytes(stream[b.pay_off:b.pay_off + b.pay_len]), b.crc, verify)
                self.pieces.append(data)
                self.block_status.append(st)
            self.status = next((st for st in self.block_status if st), 0)


@functools.lru_cache(maxsize=None)
def block_verdict(payload, crc, verify):
    """(status, bytes or None): the oracle's status where it rejects the payload, else SMA_ERR_CRC
    where the decoded bytes do not have the stored checksum."""
    st, data = _oracle().uncompress_status(payload)
    if st:
        return st, None
    data = bytes(data)
    return (R.CRC if verify and zlib.crc32(data) != crc else 0), data


def run_decode(av, streams, caps, max_blocks, max_fragments=0, verify=True, kind=R.FILE, syncs=None, table=True, lead=1):
    """One sma_uncompress_streams_device call over the streams laid back to back; every output has
    its cap bytes in a guard-filled buffer with at least 16 guard bytes on both sides, at odd places."""
    torch = _torch()
    d_in, in_off, in_len = lay(streams, lead)
    offs, pos = [], 33
    for c in caps:
        offs.append(pos)
        pos += c + 16 + (c % 3)
    d_out = torch.full((pos + 32,), GUARD, dtype=torch.uint8, device=_dev())
    k, m = len(streams), max(max_blocks, 1)
    d_ol = torch.full((k,), -1, dtype=torch.int64, device=_dev())
    d_ob = torch.full((k,), -1, dtype=torch.int64, device=_dev())
    d_st = torch.full((k,), 77, dtype=torch.int32, device=_dev())
    d_bf = torch.full((k + 1,), -1, dtype=torch.int32, device=_dev())
    d_bs = torch.full((m,), 77, dtype=torch.int32, device=_dev())
    d_tab = None
    if table:
        d_tab = {key: torch.full((m,), -1, dtype=torch.int64 if av.BLOCK_DTYPES[key] == np.uint64 else torch.int32, device=_dev())
                 for key in av.INDEX_KEYS}
    d_sync = None if syncs is None else _u8(b"".join(syncs))
    av.uncompress_avro_streams_device(d_in, _i64(in_off), _i64(in_len), max_blocks, max_fragments, d_out, _i64(offs), _i64(caps),
                                      d_ol, d_st, kind=kind, d_sync=d_sync, verify_crc=verify, d_objects=d_ob, d_block_first=d_bf,
                                      d_block_status=d_bs, d_blocks=d_tab)
    torch.cuda.synchronize()
    tab = None if d_tab is None else {key: d_tab[key].cpu().numpy()[:max_blocks].astype(np.int64).tolist() for key in av.INDEX_KEYS}
    return dict(status=d_st.cpu().tolist(), length=d_ol.cpu().tolist(), objects=d_ob.cpu().tolist(), out=d_out.cpu().numpy(),
                offs=offs, first=d_bf.cpu().tolist(), block_status=d_bs.cpu().tolist()[:max_blocks], table=tab)


def check_decode(streams, caps, models, res, max_blocks):
    """Per stream the status, the length, the objects and every good block's bytes against the model;
    the block statuses and the table; every byte outside the decoded streams' content is the guard's."""
    out, offs = res["out"], res["offs"]
    outside = np.ones(out.size, bool)
    wrong, first, want_bs = [], [0], []
    want_tab = {key: [] for key in R.Block._fields}
    for s, m in enumerate(models):
        ok = (res["status"][s], res["length"][s], res["objects"][s]) == (m.status, m.length, m.objects)
        if m.slots:
            assert m.length <= caps[s]
            outside[offs[s]:offs[s] + m.length] = False
            for piece, b in zip(m.pieces, m.walk.blocks):
                if piece is not None and len(piece) == b.ulen:
                    ok = ok and out[offs[s] + b.out_off:offs[s] + b.out_off + b.ulen].tobytes() == piece
                for key in R.Block._fields:
                    want_tab[key].append(getattr(b, key))
        first.append(first[-1] + m.slots)
        want_bs += m.block_status
        if not ok:
            wrong.append((s, res["status"][s], res["length"][s], res["objects"][s], m.status, m.length, m.objects))
    assert not wrong, wrong[:8]
    assert (out[outside] == GUARD).all()
    assert res["first"] == first
    assert res["block_status"] == want_bs + [0] * (max_blocks - len(want_bs))
    if res["table"] is not None:
        for key in R.Block._fields:
            got = [v & 0xFFFFFFFF if key in ("pay_len", "ulen", "crc") else v for v in res["table"][key]]
            assert got == want_tab[key] + [0] * (max_blocks - len(want_tab[key])), key


def decode_case(av, streams, caps=None, max_blocks=None, **kw):
    syncs = kw.get("syncs")
    if caps is None:
        caps = [R.walk(s, kw.get("kind", R.FILE), None if syncs is None else syncs[i]).total for i, s in enumerate(streams)]
    models = [Model(s, c, kw.get("kind", R.FILE), None if syncs is None else syncs[i], kw.get("verify", True))
              for i, (s, c) in enumerate(zip(streams, caps))]
    total = sum(m.slots for m in models)
    max_blocks = total if max_blocks is None else max_blocks
    res = run_decode(av, streams, caps, max_blocks, **kw)
    check_decode(streams, caps, models, res, max_blocks)
    return res, models


@pytest.mark.parametrize("fragments", [0, "enough"])
def test_the_four_fixtures_in_one_batch(av, fragments):
    streams = [fixture(n) for n in FILES]
    frags = av.avro_plan(streams)[6]
    assert frags == 4 + 258 + 4 + 4
    res, models = decode_case(av, streams, max_fragments=frags if fragments else 0)
    assert res["status"] == [0, 0, 0, 0] and res["objects"] == [3609, 3102, 3609, 157]
    assert [m.slots for m in models] == [4, 300, 1, 4]
    # pyarrow's libsnappy wrote the one block of more than 64 KiB: it decodes by fragments when it may
    assert av.last_indexed(0) == (1 if fragments else 0)


def test_mixed_batch_writes_only_the_good_file(av):
    small, meta = fixture("small_blocks.avro"), fixture("meta_forms.avro")
    cases = R.mutations(small, meta)
    header_only = meta[:R.walk(meta).header_len]
    streams = [meta] + [c[1] for c in cases] + [meta, header_only]
    caps = [R.walk(s).total for s in streams]
    caps[-2] -= 1  # one byte over its capacity
    res, models = decode_case(av, streams, caps)
    assert res["status"] == [0] + [c[2] for c in cases] + [R.SM_BUFFER_TOO_SMALL, 0]
    assert {c[2] for c in cases} == {R.NO_HEADER, R.BAD_HEADER, R.TRUNCATED, R.VARLONG, R.CODEC, R.BLOCK, R.TOO_LARGE, R.SYNC,
                                     R.SM_ERR_VARINT}
    assert res["length"][-2] == caps[-2] + 1 and res["length"][-1] == 0 and res["first"][-1] == 4
    written = res["out"] != GUARD
    assert written[res["offs"][0]:res["offs"][0] + caps[0]].sum() > 0.99 * caps[0]
    written[res["offs"][0]:res["offs"][0] + caps[0]] = False
    assert not written.any()


def test_slot_bounds(av):
    streams = [fixture("meta_forms.avro"), fixture("blocks_64k.avro"), fixture("meta_forms.avro")[:-1]]
    res, _ = decode_case(av, streams, max_blocks=8)  # exactly reached
    assert res["status"] == [0, 0, R.TRUNCATED]
    res, _ = decode_case(av, streams, max_blocks=11)  # more than needed: the spare slots stay empty
    assert res["status"] == [0, 0, R.TRUNCATED]
    caps = [R.walk(s).total for s in streams]
    res = run_decode(av, streams, caps, 7)  # one short
    assert res["status"] == [ARG] * 3 and res["length"] == [0] * 3 and res["objects"] == [0] * 3
    assert (res["out"] == GUARD).all() and res["block_status"] == [0] * 7 and res["first"] == [0, 4, 8, 8]
    res = run_decode(av, streams, caps, 0)
    assert res["status"] == [ARG] * 3 and (res["out"] == GUARD).all()
    res = run_decode(av, [streams[2], b""], [0, 0], 0)  # no slots needed, none given
    assert res["status"] == [R.TRUNCATED, R.NO_HEADER] and res["length"] == [R.walk(streams[2]).total, 0]


def test_more_than_256_blocks_and_more_than_4_streams(av):
    small, meta = fixture("small_blocks.avro"), fixture("meta_forms.avro")
    header_only = small[:658]
    streams = [small, meta, header_only, small, meta[:-1], meta, small, b"", meta]
    res, models = decode_case(av, streams, table=False)
    assert sum(m.slots for m in models) == 3 * 300 + 3 * 4 and res["first"][-1] == 912
    assert res["status"] == [0, 0, 0, 0, R.TRUNCATED, 0, 0, R.NO_HEADER, 0]
    res, _ = decode_case(av, streams, max_fragments=3 * 258 + 3 * 4, lead=7)


def test_a_flipped_checksum_byte(av):
    meta, b64 = fixture("meta_forms.avro"), fixture("blocks_64k.avro")
    w = R.walk(b64)
    at = w.blocks[2].pay_off + w.blocks[2].pay_len + 3  # the third block's checksum, its last byte
    bad = b64[:at] + bytes([b64[at] ^ 0x10]) + b64[at + 1:]
    res, models = decode_case(av, [meta, bad, b64])
    assert res["status"] == [0, R.CRC, 0] and res["block_status"] == [0] * 4 + [0, 0, R.CRC, 0] + [0] * 4
    res, _ = decode_case(av, [meta, bad, b64], verify=False)
    assert res["status"] == [0, 0, 0] and res["block_status"] == [0] * 12
    # the bytes are decoded either way: the verdict does not take them back
    assert res["out"][res["offs"][1]:res["offs"][1] + w.total].tobytes() == res["out"][res["offs"][2]:res["offs"][2] + w.total].tobytes()


def test_flipped_payload_bytes(av):
    """200 seeded positions inside the payloads of blocks_64k.avro, one flipped bit each, all in one
    batch with max_fragments = 0: the oracle's status where it rejects the payload, else
    SMA_ERR_CRC where the bytes differ, else SM_OK; a flip in a payload's varint may also turn into
    a walk status.  No case is left out."""
    b64 = fixture("blocks_64k.avro")
    w = R.walk(b64)
    rng = np.random.default_rng(20240916)
    streams = []
    for i in range(200):
        b = w.blocks[i % len(w.blocks)]
        at = b.pay_off + (int(rng.integers(0, b.pay_len)) if i >= 8 else i % 4)  # (the first eight: the varint's bytes)
        streams.append(b64[:at] + bytes([b64[at] ^ (1 << int(rng.integers(0, 8)))]) + b64[at + 1:])
    res, models = decode_case(av, streams, table=False)
    seen = {m.status for m in models}
    assert R.CRC in seen and seen & {19, 20, 21} and len(seen) >= 3, seen


def test_streams_past_one_scan_tile(av):
    """301 streams in one batch, every third cut short (a walk error: no slots): the scan of the
    streams' slot counts runs over two tiles of 256 with zeros among the counts, and block_first is
    the model's on both sides of the edge."""
    meta = fixture("meta_forms.avro")  # (four blocks)
    streams = [meta[:-5] if i % 3 == 1 else meta for i in range(301)]
    res, models = decode_case(av, streams, table=False)
    assert [m.slots for m in models[255:258]] == [4, 0, 4]
    assert res["status"][256] != 0 and res["status"][255] == 0 and res["status"][300] == 0


def test_block_runs_behind_every_marker(av):
    small = fixture("small_blocks.avro")
    w = R.walk(small)
    starts = [w.header_len] + [b.pay_off + b.pay_len + 20 for b in w.blocks]
    starts = starts[:8] + starts[8::9] + starts[-2:]  # the first, every ninth, the last and the empty run
    streams = [small[s:] for s in starts]
    syncs = [w.sync] * len(streams)
    other = bytes(b ^ 0xFF for b in w.sync)
    streams += [small[starts[1]:], small[starts[-1]:], small]
    syncs += [other, other, w.sync]
    res, models = decode_case(av, streams, kind=R.BLOCKS, syncs=syncs, table=False)
    k = len(starts)
    assert res["status"][:k] == [0] * k and res["length"][0] == w.total and res["length"][k - 1] == 0
    for i, s in enumerate(starts):  # the file's tail
        first = next((b for b in w.blocks if b.pay_off > s), None)
        tail = w.total - (first.out_off if first else w.total)
        assert res["length"][i] == tail
    assert res["status"][k:] == [R.SYNC, 0, R.BLOCK]  # a wrong marker; no block, no marker to hold; a file is no run


# ---- the sync search -----------------------------------------------------------------------------------

def test_find_sync_against_bytes_find(av):
    rng = np.random.default_rng(20240917)
    noise = rng.integers(0, 256, 70000, dtype=np.uint8).tobytes()
    m = SYNC

    def with_marks(n, places, base=noise):
        buf = bytearray((base * (n // len(base) + 1))[:n])
        for p in places:
            buf[p:p + 16] = m
        return bytes(buf)

    streams, queries = [], []

    def add(stream, starts):
        streams.append(stream)
        queries.extend((len(streams) - 1, s) for s in starts)

    for p in range(65536 - 33, 65536 + 18):  # every straddle of a 64 KiB edge, wherever the granules fall
        add(with_marks(70000, [p]), [0, 5, p, p + 1])
    add(with_marks(70000, [69984]), [0, 69983, 69984, 69985, 70000, 70001])  # at n - 16
    add(with_marks(5000, [100, 3000]), [0, 100, 101, 2999, 3000, 3001])  # the first wins; several queries on one stream
    add(with_marks(5000, []), [0, 4984, 4999])  # none
    false_start = bytearray(with_marks(5000, [1000, 2000]))
    false_start[1015] ^= 1  # a 15-byte false start
    add(bytes(false_start), [0, 1000, 1001])
    add(m, [0, 1])  # the marker alone
    add(m[:15], [0])  # too short for one
    add(b"", [0])
    add(m * 3 + m[:8], [0, 1, 16, 17, 33, 40])  # back to back
    big = with_marks(1200000, [900000, 1100000, 1199984], base=bytes(4096))  # many tiles, the rows of the grid
    add(big, [0, 65536, 899999, 900000, 900001, 1100001, 1199985])
    add(with_marks(200000, [], base=m[:15] + b"\xff"), [0, 100000])  # 15 of 16 bytes everywhere
    want = [R.find_sync(streams[s], m, f) for s, f in queries]
    for lead in (1, 0, 9):
        torch = _torch()
        d_in, offs, lens = lay(streams, lead)
        d_pos = torch.full((len(queries),), -1, dtype=torch.int64, device=_dev())
        av.find_sync_device(d_in, _i64(offs), _i64(lens), _u8(m * len(streams)), _i32([q[0] for q in queries]),
                            _i64([q[1] for q in queries]), d_pos)
        torch.cuda.synchronize()
        got = d_pos.cpu().tolist()
        wrong = [(q, g, x) for q, g, x in zip(queries, got, want) if g != x]
        assert not wrong, (lead, wrong[:8])
    assert av.find_sync_host(streams, [m] * len(streams), queries) == want
    assert av.find_sync(streams[-3:], [m] * 3, [(1, 900001), (0, 0)]) == [1100000, 0]
    # a file's own markers: every split point lands on a block run
    small = fixture("small_blocks.avro")
    w = R.walk(small)
    cuts = list(range(0, len(small), 7919))
    got = av.find_sync([small], [w.sync], [(0, c) for c in cuts])
    assert got == [R.find_sync(small, w.sync, c) for c in cuts]


# ---- encode ---------------------------------------------------------------------------------------------

SIZES = (0, 1, 63, 64, 65535, 65536, 65537, 200000)
COUNTS = (0, 1, 63, 64, 2**31)


@functools.lru_cache(maxsize=None)
def encode_input():
    """Two streams: the eight sizes with the five counts in turn, then three blocks more."""
    one = [text(n) for n in SIZES]
    two = [text(300)[::-1], b"", np.random.default_rng(5).integers(0, 256, 70000, dtype=np.uint8).tobytes()]
    return [(one, [COUNTS[i % 5] for i in range(len(one))]), (two, [COUNTS[4], 7, 1])]


def run_encode(av, streams, syncs, heads, mode, max_blocks=None, stage=None, fragments=None):
    torch = _torch()
    blocks = [b for bs, _ in streams for b in bs]
    counts = [c for _, cs in streams for c in cs]
    d_in, offs, lens = lay(blocks + (heads or []), lead=3)
    nb, k = len(blocks), len(streams)
    first = np.cumsum([0] + [len(bs) for bs, _ in streams]).tolist()
    room = [(len(heads[s]) if heads else 0) + sum(av.max_block_length(len(b)) for b in streams[s][0]) for s in range(k)]
    out_off, pos = [], 17
    for r in room:
        out_off.append(pos)
        pos += r + 16
    d_out = torch.full((pos + 32,), GUARD, dtype=torch.uint8, device=_dev())
    d_ol = torch.full((k,), -1, dtype=torch.int64, device=_dev())
    d_st = torch.full((k,), 77, dtype=torch.int32, device=_dev())
    need_stage = sum(av.lib().sma_stage_length(len(b)) for b in blocks)
    need_frags = sum(-(-len(b) // 65536) for b in blocks if len(b) > 65536)
    av.compress_avro_streams_device(
        d_in, _i32(first), _i64(offs[:nb]), _i32(lens[:nb]), _i64(counts), _u8(b"".join(syncs)),
        nb if max_blocks is None else max_blocks, need_stage if stage is None else stage,
        need_frags if fragments is None else fragments, d_out, _i64(out_off), d_ol, d_st,
        d_head_off=_i64(offs[nb:]) if heads else None, d_head_len=_i64(lens[nb:]) if heads else None, mode=mode)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    return dict(status=d_st.cpu().tolist(), length=d_ol.cpu().tolist(), out=out, offs=out_off, room=room,
                bounds=(nb, need_stage, need_frags))


@pytest.mark.parametrize("with_header", [True, False])
@pytest.mark.parametrize("mode", ["reference", "fast", "dense"])
def test_encode_equals_the_reference_writer(av, mode, with_header):
    sm = load_package()
    streams = encode_input()
    syncs = [SYNC, bytes(reversed(SYNC))]
    heads = [R.header(SCHEMA, s, [(b"writer", b"test")]) for s in syncs] if with_header else None
    res = run_encode(av, streams, syncs, heads, mode)
    assert res["status"] == [0, 0]
    compress = functools.lru_cache(maxsize=None)(lambda b: sm.compress(b, mode=mode, device=0))
    _, lib_uncompress = R.libsnappy()
    outside = np.ones(res["out"].size, bool)
    for s, ((blocks, counts), sync) in enumerate(zip(streams, syncs)):
        want = (heads[s] if heads else b"") + R.write_blocks(blocks, counts, sync, compress)
        got = res["out"][res["offs"][s]:res["offs"][s] + res["length"][s]].tobytes()
        assert res["length"][s] == len(want) <= res["room"][s] and got == want, s
        if mode == "reference":  # byte for byte the reference writer over the oracle
            assert got == (heads[s] if heads else b"") + R.write_blocks(blocks, counts, sync, _oracle().compress)
        outside[res["offs"][s]:res["offs"][s] + len(want)] = False
        # every payload decodes under libsnappy, every checksum is zlib's
        w = R.walk(got, R.FILE if heads else R.BLOCKS, sync)
        assert w.status == 0 and [b.count for b in w.blocks] == counts
        for b, data in zip(w.blocks, blocks):
            assert lib_uncompress(got[b.pay_off:b.pay_off + b.pay_len]) == data and b.crc == zlib.crc32(data)
        # and the file round-trips through the decoder with its checksums verified
        if heads:
            back, table = av.uncompress_avro(got, verify_crc=True, device=0)
            assert back == b"".join(blocks) and table["count"].tolist() == counts
        else:
            (back, table), = av.uncompress_avro_streams([got], "blocks", [sync], verify_crc=True, device=0)
            assert back == b"".join(blocks)
    assert (res["out"][outside] == GUARD).all()


def test_encode_bounds(av):
    streams = encode_input()
    syncs = [SYNC, SYNC]
    exact = run_encode(av, streams, syncs, None, "fast")
    nb, stage, frags = exact["bounds"]
    assert (nb, frags) == (11, 4 + 2 + 2) and exact["status"] == [0, 0]
    for kw in (dict(max_blocks=nb - 1), dict(stage=stage - 1), dict(fragments=frags - 1), dict(max_blocks=0)):
        res = run_encode(av, streams, syncs, None, "fast", **kw)
        assert res["status"] == [ARG, ARG] and res["length"] == [0, 0] and (res["out"] == GUARD).all(), kw
    res = run_encode(av, streams, syncs, None, "fast", max_blocks=nb + 5, stage=stage + 100, fragments=frags + 3)  # spare slots
    assert res["status"] == [0, 0] and res["length"] == exact["length"]
    for s in range(2):
        assert (res["out"][res["offs"][s]:res["offs"][s] + res["length"][s]] ==
                exact["out"][exact["offs"][s]:exact["offs"][s] + exact["length"][s]]).all()
    # a stream without blocks is its header alone; a batch without blocks writes the headers
    head = R.header(SCHEMA, SYNC)
    res = run_encode(av, [([], []), ([b"abc"], [1]), ([], [])], [SYNC] * 3, [head, head, b""], "reference")
    assert res["status"] == [0, 0, 0] and res["length"] == [len(head), len(head) + 2 + 5 + 4 + 16, 0]
    assert res["out"][res["offs"][1]:res["offs"][1] + res["length"][1]].tobytes() == R.write([b"abc"], [1], SCHEMA, SYNC, _oracle().compress)
    res = run_encode(av, [([], [])], [SYNC], [head], "fast")
    assert res["status"] == [0] and res["out"][res["offs"][0]:res["offs"][0] + len(head)].tobytes() == head


# ---- host buffers and Python ---------------------------------------------------------------------------

def test_host_buffer_and_python_calls(av):
    b64, meta = fixture("blocks_64k.avro"), fixture("meta_forms.avro")
    _, uncompress = R.libsnappy()
    want = R.read(b64, uncompress)[1]
    data, table = av.uncompress_avro(b64)
    assert data == want and table["ulen"].tolist() == [b.ulen for b in R.walk(b64).blocks]
    w = R.walk(b64)
    at = w.blocks[1].pay_off + w.blocks[1].pay_len  # a checksum's first byte
    bad = b64[:at] + bytes([b64[at] ^ 1]) + b64[at + 1:]
    with pytest.raises(av.AvroError) as e:
        av.uncompress_avro(bad)
    assert e.value.code == R.CRC and e.value.stream is None and "CRC" in str(e.value)
    assert av.uncompress_avro(bad, verify_crc=False)[0] == want
    res, codes = av.uncompress_avro_streams([meta, bad, meta[:-1], b64], statuses=True)
    assert codes == [0, R.CRC, R.TRUNCATED, 0] and res[0][0] == R.read(meta, uncompress)[1] and res[3][0] == want
    assert res[1][0] is None and res[2][0] is None
    with pytest.raises(av.AvroError) as e:
        av.uncompress_avro_streams([meta, meta[:-1]])
    assert e.value.code == R.TRUNCATED and e.value.stream == 1
    assert av.uncompress_avro_streams([]) == [] and av.compress_avro_streams([], []) == []
    blocks, counts = [text(70000), b"", text(10)], [3, 0, 2**40]
    made = av.compress_avro(blocks, counts, SCHEMA, SYNC, meta=[(b"k", b"v")], mode="reference")
    assert made == R.write(blocks, counts, SCHEMA, SYNC, _oracle().compress, [(b"k", b"v")])
    assert av.uncompress_avro(made)[0] == b"".join(blocks)
    runs = av.compress_avro_streams([(blocks, counts), ([], [])], [SYNC, SYNC], mode="fast")
    assert runs[1] == b"" and av.uncompress_avro_streams([runs[0]], "blocks", [SYNC])[0][0] == b"".join(blocks)
    assert av.find_sync([made], [SYNC], [(0, 0), (0, 100)]) == [R.find_sync(made, SYNC, 0), R.find_sync(made, SYNC, 100)]


def test_smoke_runs_its_avro_line(gpu_available):
    import importlib.util
    spec = importlib.util.spec_from_file_location("graft_entry_for_avro", os.path.join(ROOT, "__graft_entry__.py"))
    entry = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(entry)
    entry.smoke()
