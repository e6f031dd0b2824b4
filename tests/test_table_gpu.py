"""The LevelDB table library on the GPU (snappy.jl_amd/table.py over libsnappy_mi355x_table.so):
smt_uncompress_tables_device over the fixtures of tests/golden/table/ and over mixed batches laid
back to back at odd alignments between guard bytes, one mutated table per step of the status order,
the bounds, scan-tile and walker-workgroup edges, every input alignment, index entries across the
walker's 64-byte window, the handle-level decode, the index call alone, the encoder against the
reference writer, and the host-buffer and Python calls.  Every expected value comes from the
plain-Python reference (tests/table_ref.py), the CPU oracle and pyarrow's libsnappy."""
import functools
import importlib
import os
import struct

import numpy as np
import pytest

import avro_ref
import table_ref as R
from conftest import ROOT, load_package, read_testfile

pytestmark = pytest.mark.gpu

GUARD = 0xA5
ARG = R.SM_ERR_ARGUMENT
GOLDEN = os.path.join(ROOT, "tests", "golden", "table")
FILES = ("mixed.ldb", "bigblock.ldb", "bigindex.ldb", "empty.ldb")


@pytest.fixture(scope="module")
def tb(gpu_available):
    load_package()
    return importlib.import_module("snappy_jl_amd.table")


def _torch():
    import torch
    return torch


def _dev():
    return _torch().device("cuda", 0)


def _i64(values):
    return _torch().from_numpy(np.array(values, dtype=np.uint64).view(np.int64)).to(_dev())


def _i32(values):
    return _torch().from_numpy(np.array(values, dtype=np.uint32).view(np.int32)).to(_dev())


def _full(n, value, dtype):
    return _torch().full((max(n, 1),), value, dtype=dtype, device=_dev())


def _oracle():
    import oracle as O
    O.lib()
    return O


def oracle_uncompress(payload):
    """The decoded bytes, or the raw decoder's status where it refuses the payload."""
    st, data = _oracle().uncompress_status(payload)
    return st if st else bytes(data)


@functools.lru_cache(maxsize=None)
def pa_compress():
    return avro_ref.libsnappy()[0]


@functools.lru_cache(maxsize=None)
def fixture(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def text(n, skip=0):
    t = read_testfile("alice29.txt")
    return (t * ((n + skip) // len(t) + 1))[skip:skip + n]


@functools.lru_cache(maxsize=None)
def plan(table, cap=None, verify=True):
    return R.plan(table, oracle_uncompress, cap, verify)


def round16(n):
    return (n + 15) // 16 * 16


def index_need(table):
    """The decoded index length the index stage places (0 where the footer or the head fails)."""
    try:
        return R.block_head(table, R.read_footer(table)[1])[1]
    except R.Stop:
        return 0


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


# ---- decode -----------------------------------------------------------------------------------------

def run_tables(tb, tables, caps=None, verify=True, max_blocks=None, max_index_bytes=None, max_fragments=0, lead=1, aligns=None):
    """smt_uncompress_tables_device over `tables`, every optional output asked for, and the checks
    that hold for every call: each table's status, length, bytes and per-block arrays against the
    reference's plan, and guard bytes wherever nothing may be written."""
    torch = _torch()
    k = len(tables)
    free = [plan(t, None, verify) for t in tables]
    if caps is None:
        caps = [p.out_len for p in free]
    models = [plan(t, c, verify) for t, c in zip(tables, caps)]
    need_blocks = sum(len(p.handles) for p in models)
    need_index = sum(round16(index_need(t)) for t in tables)
    m = need_blocks if max_blocks is None else max_blocks
    mib = need_index if max_index_bytes is None else max_index_bytes
    over = m < need_blocks or mib < need_index
    d_in, in_off, in_len = lay(tables, lead, aligns)
    out_off, pos = [], 3
    for c in caps:
        out_off.append(pos)
        pos += c + 5
    d_out = _full(pos + 32, GUARD, torch.uint8)
    d_ol, d_st = _full(k, -1, torch.int64), _full(k, 77, torch.int32)
    d_bf = _full(k + 1, -1, torch.int32)
    d_ho, d_hs, d_bo, d_bl = (_full(m, -1, torch.int64) for _ in range(4))
    d_bs = _full(m, 77, torch.int32)
    tb.uncompress_tables_device(d_in, _i64(in_off), _i64(in_len), m, mib, max_fragments, d_out, _i64(out_off), _i64(caps), d_ol, d_st,
                                verify_crc=verify, d_block_first=d_bf, d_handle_off=d_ho, d_handle_size=d_hs, d_block_out_off=d_bo,
                                d_block_len=d_bl, d_block_status=d_bs)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    res = {"status": d_st.cpu().tolist()[:k], "length": d_ol.cpu().tolist()[:k], "first": d_bf.cpu().tolist(), "out": out,
           "out_off": out_off, "models": models, "need_blocks": need_blocks, "need_index": need_index,
           "block_status": d_bs.cpu().tolist(), "handles": list(zip(d_ho.cpu().tolist(), d_hs.cpu().tolist()))}
    written = np.zeros(out.size, bool)
    if over:
        assert res["status"] == [ARG] * k and res["length"] == [0] * k
        assert res["first"] == [-1] * (k + 1) and set(res["block_status"]) <= {77}
    else:
        assert res["status"] == [p.status for p in models]
        assert res["length"] == [p.out_len for p in models]
        first = [0]
        for p in models:
            first.append(first[-1] + len(p.handles))
        assert res["first"] == first
        bo, bl = d_bo.cpu().tolist(), d_bl.cpu().tolist()
        for t, p in enumerate(models):
            lo, hi = first[t], first[t + 1]
            assert res["handles"][lo:hi] == p.handles, t
            if p.decoded is None:
                if p.block_len:  # (well formed but too long: the per-block arrays are there, nothing is decoded)
                    assert (bo[lo:hi], bl[lo:hi], res["block_status"][lo:hi]) == (p.block_out_off, p.block_len, p.block_status), t
                continue
            assert (bo[lo:hi], bl[lo:hi], res["block_status"][lo:hi]) == (p.block_out_off, p.block_len, p.block_status), t
            at = out_off[t]
            written[at:at + p.out_len] = True
            for o, n, st in zip(p.block_out_off, p.block_len, p.block_status):
                if st == 0:
                    assert out[at + o:at + o + n].tobytes() == p.decoded[o:o + n], t
    assert (out[~written] == GUARD).all()  # nothing outside the decoded tables' own ranges
    return res


def test_fixtures_in_one_batch(tb):
    tables = [fixture(n) for n in FILES]
    for frags in (0, 8192):
        res = run_tables(tb, tables, max_fragments=frags)
        assert res["status"] == [0, 0, 0, 0] and res["first"] == [0, 12, 13, 4513, 4513]
        assert tb.last_indexed(0) == (1 if frags else 0)  # the 200 KiB block, by fragments
    assert res["length"][1] > 3 * 65536 and res["need_index"] > 65536 + 432


def test_good_beside_bad(tb):
    mixed, big = fixture("mixed.ldb"), fixture("bigblock.ldb")
    bad = [mixed[:-1], mixed[:40], b"", mutate_crc(mixed, 3)]
    tables = [mixed, bad[0], big, bad[1], bad[2], fixture("empty.ldb"), bad[3], mixed]
    res = run_tables(tb, tables, max_fragments=8, lead=7)
    assert res["status"] == [0, R.MAGIC_ERR, 0, R.TRUNCATED, R.TRUNCATED, 0, R.CRC, 0]
    assert res["models"][6].block_status[3] == R.CRC and sum(map(bool, res["models"][6].block_status)) == 1


# ---- one mutated copy of mixed.ldb per step of the status order ----------------------------------------

def put(data, at, new):
    return data[:at] + bytes(new) + data[at + len(new):]


def parts(data):
    """(index handle, decoded index contents, data handles) of a well-formed table."""
    _, index = R.read_footer(data)
    raw = data[index[0]:index[0] + index[1]]
    contents = oracle_uncompress(raw) if data[index[0] + index[1]] == 1 else raw
    return index, contents, R.walk_index(contents, len(data))[1]


def retail(data, contents, compress):
    """The table with its index block replaced by `contents` (compressed where the rule says so)."""
    _, _, handles = parts(data)
    base = handles[-1][0] + handles[-1][1] + 5
    meta, msize = R.stored_block(R.build_block([]))
    index, isize = R.stored_block(contents, compress)
    foot = R.put_handle((base, msize)) + R.put_handle((base + len(meta), isize))
    return data[:base] + meta + index + foot + bytes(40 - len(foot)) + R.MAGIC


def refused(data, lo, hi):
    """`data` with the first byte of [lo, hi) whose change makes the raw decoder refuse data[lo:hi] changed."""
    for at in range(lo + 5, hi):  # (behind the varint: the declared length stays)
        for x in (0xFF, 0x55):
            cand = put(data, at, [data[at] ^ x])
            if isinstance(oracle_uncompress(cand[lo:hi]), int):
                return cand
    raise AssertionError("no refused payload found")


def mutate_crc(data, block):
    o, s = parts(data)[2][block]
    return put(data, o + s + 2, [data[o + s + 2] ^ 0x10])


def compressed_block(data):
    handles = parts(data)[2]
    return next(j for j, (o, s) in enumerate(handles) if data[o + s] == 1 and j >= 2)


@functools.lru_cache(maxsize=None)
def mutations():
    """(name, table, verify, expected status, expected length or None)."""
    data = fixture("mixed.ldb")
    n = len(data)
    (ioff, isize), contents, handles = parts(data)
    meta = R.read_footer(data)[0]
    foot = lambda m, i: R.put_handle(m) + R.put_handle(i)
    j = compressed_block(data)
    o, s = handles[j]
    before = sum(R.block_head(data, h)[1] for h in handles[:j])
    whole = plan(data).out_len
    bad_handles = list(handles)
    bad_handles[5] = (n - 48 - 4, 0)
    keys = [b"k%02d" % i for i in range(len(handles))]
    first_fields = R.get_varint32(contents, 0, len(contents))
    flipped = refused(data, o, o + s)
    return [
        ("the magic", put(data, n - 1, [data[-1] ^ 1]), True, R.MAGIC_ERR, 0),
        ("a cut file", data[:47], True, R.TRUNCATED, 0),
        ("a footer varint", put(data, n - 48, b"\xff" * 40), True, R.FOOTER, 0),
        ("the index handle past the end", put(data, n - 48, (foot(meta, (ioff + 44, isize)) + bytes(40))[:40]), True, R.HANDLE, 0),
        ("the index type", put(data, ioff + isize, [2]), True, R.TYPE, 0),
        ("an index CRC byte", put(data, ioff + isize + 1, [data[ioff + isize + 1] ^ 0x80]), True, R.CRC, 0),
        ("an index payload byte, checked", refused(data, ioff, ioff + isize), True, R.CRC, 0),
        ("an index payload byte", refused(data, ioff, ioff + isize), False, None, 0),
        ("the index varint", put(data, ioff, b"\xff" * 5), False, R.SM_ERR_VARINT, 0),
        ("an index entry's shared", retail(data, put(contents, 0, [first_fields[0] + 1]), pa_compress()), True, R.INDEX, 0),
        ("the restart count", retail(data, contents[:-4] + struct.pack("<I", len(contents)), pa_compress()), True, R.INDEX, 0),
        ("a data handle past the end", retail(data, R.build_index(keys, bad_handles), pa_compress()), True, R.HANDLE, 0),
        ("a data type", put(data, o + s, [2]), True, R.TYPE, before),
        ("a data varint", put(data, o, b"\xff" * 5), True, R.SM_ERR_VARINT, before),
        ("a data varint of 2^31", put(data, o, bytes.fromhex("8080808008")), True, R.TOO_LARGE, before),
        ("data content, checked", flipped, True, R.CRC, whole),
        ("data content", flipped, False, None, whole),
        ("a stored CRC byte", mutate_crc(data, j), True, R.CRC, whole),
        ("a stored CRC byte, unchecked", mutate_crc(data, j), False, 0, whole),
    ]


@pytest.mark.parametrize("verify", [True, False])
def test_status_order(tb, verify):
    cases = [c for c in mutations() if c[2] == verify]
    tables = [c[1] for c in cases] + [fixture("mixed.ldb")]
    res = run_tables(tb, tables, verify=verify, lead=5)
    for (name, _, _, status, length), got, glen, model in zip(cases, res["status"], res["length"], res["models"]):
        if status is None:  # the raw decoder's own status: the oracle's, through the reference's plan
            assert got == model.status and got not in (0, R.CRC) and got < 96, name
        else:
            assert got == status, name
        assert glen == length, name
    assert res["status"][-1] == 0
    refusals = [c for c in cases if c[3] is None]
    assert len(refusals) == (0 if verify else 2)


def test_bounds(tb):
    tables = [fixture("mixed.ldb"), fixture("empty.ldb"), fixture("mixed.ldb")[:-1], fixture("mixed.ldb")]
    res = run_tables(tb, tables)
    assert res["need_blocks"] == 24 and res["need_index"] == 2 * 432 + 16 and res["status"] == [0, 0, R.MAGIC_ERR, 0]
    run_tables(tb, tables, max_blocks=23)
    run_tables(tb, tables, max_index_bytes=res["need_index"] - 1)
    caps = [res["length"][0] - 1, 0, 0, res["length"][3]]
    short = run_tables(tb, tables, caps=caps)
    assert short["status"] == [R.SM_BUFFER_TOO_SMALL, 0, R.MAGIC_ERR, 0] and short["length"][0] == caps[0] + 1
    roomy = run_tables(tb, tables, caps=[c + 9 for c in caps[:1]] + caps[1:], max_blocks=40, max_index_bytes=5000)
    assert roomy["status"] == [0, 0, R.MAGIC_ERR, 0]


@functools.lru_cache(maxsize=None)
def small_table(seed, nblocks=5):
    rng = np.random.default_rng(seed)
    blocks = []
    for b in range(nblocks):
        size = int(rng.integers(0, 200))
        blocks.append(text(size, seed * 131 + b * 17) if b % 2 == 0 else rng.integers(0, 256, size, dtype=np.uint8).tobytes())
    keys = [b"key-%d-%d" % (seed, b) for b in range(nblocks)]
    return R.write_table(blocks, keys, pa_compress(), compress_index=seed % 2 == 0)


def test_grid_edges(tb):
    """300 tables of 5 blocks (more than 4 waves' tables, more than one scan tile of tables, more
    than 256 entries) and one table of 4,500 blocks between them."""
    tables = [small_table(i % 7) for i in range(300)]
    tables.insert(150, fixture("bigindex.ldb"))
    res = run_tables(tb, tables, lead=3)
    assert res["status"] == [0] * 301 and res["first"][-1] == 1500 + 4500 and res["first"][151] - res["first"][150] == 4500


def test_every_input_alignment(tb):
    tables = [small_table(20 + i, nblocks=3) for i in range(16)]
    res = run_tables(tb, tables, aligns=list(range(16)))
    assert res["status"] == [0] * 16
    res = run_tables(tb, [fixture("mixed.ldb")] * 16, aligns=[(5 * i + 3) % 16 for i in range(16)])
    assert res["status"] == [0] * 16


def test_window_edges(tb):
    """The first key's length swept over 0 .. 70 pushes every later entry's fields and handle across
    the walker's 64-byte window at every phase; a 300-byte key is stepped over."""
    blocks = [text(40, 7 * i) for i in range(6)]
    tables = []
    for first in list(range(71)) + [300]:
        keys = [b"a" * first] + [b"key%d" % i * (i + 1) for i in range(1, 6)]
        tables.append(R.write_table(blocks, keys, pa_compress() if first % 3 == 0 else None, compress_index=first % 2 == 1))
    res = run_tables(tb, tables, lead=9)
    assert res["status"] == [0] * 72 and res["first"][-1] == 72 * 6


# ---- the index call alone ------------------------------------------------------------------------------

def test_index_tables_device(tb):
    torch = _torch()
    tables = [fixture("mixed.ldb"), fixture("bigindex.ldb"), fixture("mixed.ldb")[:-3], fixture("empty.ldb"),
              mutations()[5][1], mutations()[9][1]]
    want = [plan(t) for t in tables]
    need = sum(len(p.handles) for p in want)
    mib = sum(round16(index_need(t)) for t in tables)
    for m, bytes_ in ((need, mib), (need - 1, mib), (need, mib - 1)):
        d_in, in_off, in_len = lay(tables, 11)
        d_bf, d_st = _full(len(tables) + 1, -1, torch.int32), _full(len(tables), 77, torch.int32)
        d_ho, d_hs = _full(m, -1, torch.int64), _full(m, -1, torch.int64)
        tb.index_tables_device(d_in, _i64(in_off), _i64(in_len), m, bytes_, d_bf, d_ho, d_hs, d_st)
        torch.cuda.synchronize()
        if (m, bytes_) != (need, mib):
            assert d_st.cpu().tolist() == [ARG] * len(tables) and set(d_bf.cpu().tolist()) == {-1} and set(d_ho.cpu().tolist()) == {-1}
            continue
        assert d_st.cpu().tolist() == [0, 0, R.MAGIC_ERR, 0, R.CRC, R.INDEX]
        assert d_bf.cpu().tolist() == [0, 12, 4512, 4512, 4512, 4512, 4512]
        assert list(zip(d_ho.cpu().tolist(), d_hs.cpu().tolist())) == want[0].handles + want[1].handles


# ---- the handle-level decode ---------------------------------------------------------------------------

def test_blocks_by_handle(tb):
    torch = _torch()
    files = [fixture("mixed.ldb"), fixture("bigblock.ldb"), mutate_crc(fixture("mixed.ldb"), 2), put(fixture("mixed.ldb"), parts(fixture("mixed.ldb"))[2][1][0] + parts(fixture("mixed.ldb"))[2][1][1], [7])]
    d_in, in_off, _ = lay(files, 13)
    blocks = []  # (absolute offset, size, the file, its handle)
    for f, base in zip(files, in_off):
        for h in parts(fixture("mixed.ldb") if f is not files[1] else f)[2]:
            blocks.append((base + h[0], h[1], f, h))
    order = np.random.default_rng(3).permutation(len(blocks)).tolist()
    blocks = [blocks[i] for i in order]
    want = []
    for _, _, f, h in blocks:
        try:
            st, data = R.read_block(f, h, oracle_uncompress)
            want.append((st, data, R.block_head(f, h)[1]))
        except R.Stop as e:
            want.append((e.status, None, 0))
    caps = [w[2] for w in want]
    short = next(i for i, w in enumerate(want) if w[0] == 0 and w[2] > 100)
    caps[short] -= 1
    for frags in (0, 64):
        out_off, pos = [], 1
        for c in caps:
            out_off.append(pos)
            pos += c + 3
        d_out = _full(pos + 16, GUARD, torch.uint8)
        d_ol, d_st = _full(len(blocks), -1, torch.int64), _full(len(blocks), 77, torch.int32)
        tb.uncompress_table_blocks_device(d_in, _i64([b[0] for b in blocks]), _i64([b[1] for b in blocks]), frags, d_out,
                                          _i64(out_off), _i64(caps), d_ol, d_st)
        torch.cuda.synchronize()
        out, written = d_out.cpu().numpy(), np.zeros(pos + 16, bool)
        for i, ((st, data, d), got_st, got_len) in enumerate(zip(want, d_st.cpu().tolist(), d_ol.cpu().tolist())):
            if i == short:
                assert (got_st, got_len) == (R.SM_BUFFER_TOO_SMALL, d)
                continue
            assert (got_st, got_len) == (st, d), i
            if st in (0, R.CRC):
                written[out_off[i]:out_off[i] + d] = True
            if st == 0:
                assert out[out_off[i]:out_off[i] + d].tobytes() == data, i
        assert (out[~written] == GUARD).all()
        assert tb.last_indexed(0) == (1 if frags else 0)
    assert sorted({w[0] for w in want}) == [0, R.TYPE, R.CRC]


# ---- the encoder ---------------------------------------------------------------------------------------

def encoder_blocks():
    rng = np.random.default_rng(11)
    rand = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    return [[text(4096), rand(4096), b"", text(7), text(70000, 99), rand(300) + text(3000)], [], [text(100, 5)],
            [rand(1) for _ in range(3)] + [text(2000, i) for i in range(300)]]


def run_encode(tb, tables, mode, max_blocks=None, stage=None, fragments=None):
    torch = _torch()
    k = len(tables)
    flat = [b for t in tables for b in t]
    d_in, off, lens = lay(flat, 3)
    first = [0]
    for t in tables:
        first.append(first[-1] + len(t))
    need = (len(flat), sum(round16(32 + n + n // 6) for n in lens), sum(-(-n // 65536) for n in lens if n > 65536))
    m = need[0] if max_blocks is None else max_blocks
    bounds = (m, need[1] if stage is None else stage, need[2] if fragments is None else fragments)
    out_off, pos = [], 5
    for t in tables:
        out_off.append(pos)
        pos += sum(len(b) + 5 for b in t) + 3
    d_out = _full(pos + 16, GUARD, torch.uint8)
    d_ol, d_st = _full(k, -1, torch.int64), _full(k, 77, torch.int32)
    d_ho, d_hs = _full(m, -1, torch.int64), _full(m, -1, torch.int64)
    tb.compress_table_blocks_device(d_in, _i32(first), _i64(off), _i32(lens), bounds[0], bounds[1], bounds[2], d_out, _i64(out_off),
                                    d_ho, d_hs, d_ol, d_st, mode=mode)
    torch.cuda.synchronize()
    return (d_out.cpu().numpy(), out_off, d_ol.cpu().tolist()[:k], d_st.cpu().tolist()[:k], first,
            list(zip(d_ho.cpu().tolist(), d_hs.cpu().tolist())), need)


@pytest.mark.parametrize("mode", ["reference", "fast", "dense"])
def test_encoder_equals_the_reference_writer(tb, mode):
    sm = load_package()
    tables = encoder_blocks()
    compress = (lambda b: sm.compress(b, mode=mode, device=0)) if mode != "reference" else _oracle().compress
    out, out_off, lens, status, first, handles, need = run_encode(tb, tables, mode)
    assert status == [0] * len(tables)
    written = np.zeros(out.size, bool)
    kinds = set()
    for t, blocks in enumerate(tables):
        want, want_handles = R.write_blocks(blocks, compress)
        assert lens[t] == len(want) and out[out_off[t]:out_off[t] + lens[t]].tobytes() == want, t
        assert handles[first[t]:first[t + 1]] == want_handles, t
        kinds |= {want[o + s] for o, s in want_handles}
        written[out_off[t]:out_off[t] + lens[t]] = True
    assert kinds == {0, 1} and (out[~written] == GUARD).all()
    assert need[2] == 2  # the 70,000-byte block, by fragments


def test_encoder_bounds(tb):
    tables = encoder_blocks()
    need = run_encode(tb, tables, "fast")[6]
    for kw in ({"max_blocks": need[0] - 1}, {"stage": need[1] - 1}, {"fragments": need[2] - 1}):
        out, _, lens, status, _, handles, _ = run_encode(tb, tables, "fast", **kw)
        assert status == [ARG] * len(tables) and lens == [0] * len(tables) and (out == GUARD).all()


# ---- the host-buffer and Python calls ------------------------------------------------------------------

def test_python_round_trip(tb):
    blocks = [R.build_block([(b"key%04d" % (100 * b + i), text(50, 31 * i + b)) for i in range(40)]) for b in range(5)]
    blocks += [np.random.default_rng(2).integers(0, 256, 5000, dtype=np.uint8).tobytes(), b"", text(150000, 1000)]
    keys = [b"key%04d" % (100 * b + 99) for b in range(len(blocks))]
    for mode in ("fast", "reference"):
        table = tb.write_table(blocks, keys, mode=mode)
        p = plan(table)  # the reference reads the library's file
        assert p.status == 0 and [p.decoded[o:o + n] for o, n in zip(p.block_out_off, p.block_len)] == blocks
        assert {table[o + s] for o, s in p.handles} == {0, 1} and table[-8:] == R.MAGIC
        got, handles = tb.uncompress_table(table)
        assert got == blocks and handles == p.handles
        assert dict(R.entries(got[2]))[b"key0207"] == text(50, 31 * 7 + 2)  # a key looked up in a decoded block
    data, handles = tb.compress_table_blocks(blocks, mode="reference")
    assert (data, handles) == R.write_blocks(blocks, _oracle().compress)
    assert tb.uncompress_table_blocks(table, handles[::-1]) == blocks[::-1]
    assert tb.uncompress_table(R.write_table([], [], None)) == ([], [])


def test_python_batches_and_errors(tb):
    mixed, big, index = fixture("mixed.ldb"), fixture("bigblock.ldb"), fixture("bigindex.ldb")
    bad = mutate_crc(mixed, 4)
    res, codes = tb.uncompress_tables([mixed, bad, mixed[:-1], big, fixture("empty.ldb"), index], statuses=True)
    assert codes == [0, R.CRC, R.MAGIC_ERR, 0, 0, 0]
    for (blocks, handles), table, code in zip(res, [mixed, bad, mixed[:-1], big, fixture("empty.ldb"), index], codes):
        p = plan(table)
        assert handles == p.handles
        if code == 0:
            assert blocks == [p.decoded[o:o + n] for o, n in zip(p.block_out_off, p.block_len)]
        else:
            assert blocks is None
    assert tb.uncompress_tables([mixed], verify_crc=False)[0][0] == tb.uncompress_tables([bad], verify_crc=False)[0][0]
    with pytest.raises(tb.TableError) as e:
        tb.uncompress_tables([mixed, mixed[:-1]])
    assert e.value.code == R.MAGIC_ERR and e.value.index == 1
    with pytest.raises(tb.TableError) as e:
        tb.uncompress_table(bad)
    assert e.value.code == R.CRC and e.value.index is None and "CRC-32C" in str(e.value)
    got, codes = tb.uncompress_table_blocks(bad, plan(mixed).handles, statuses=True)
    assert codes == [R.CRC if i == 4 else 0 for i in range(12)] and got[4] is None and got[5] == res[0][0][5]
    assert tb.uncompress_tables([]) == [] and tb.uncompress_table_blocks(mixed, []) == []
    assert tb.uncompress_tables([mixed[:-1], b""], statuses=True) == ([(None, []), (None, [])], [R.MAGIC_ERR, R.TRUNCATED])  # no entries at all
