"""The ranged decode of indexed raw streams on the device (include/snappy_mi355x_multi_range.h):
smm_uncompress_ranges_device, its host twin and the Python wrappers.

Expected bytes are slices of the original data; expected statuses come from the contract, from
tests/multi_range_ref.py's plain statement of it, and for a damaged fragment from the existing
sm_uncompress_fragments_device call over that fragment alone.  Outputs sit at odd byte offsets with
0xA5 guard bytes between them, and the whole output buffer is compared."""
import importlib

import numpy as np
import pytest

import multi_range_ref as M
import multi_ref as R

pytestmark = pytest.mark.gpu

GUARD = 0xA5
GAP = 37
ROOM_MAX = 1 << 20  # a range that asks for more has no room of its own: it must fail and write nothing
A = M.SM_ERR_ARGUMENT


@pytest.fixture(scope="module")
def mu(sm, gpu_available):
    return importlib.import_module("snappy_jl_amd.multi")


def _dev():
    import torch
    return torch.device("cuda", 0)


def _aligned_u8(host):
    import torch
    raw = torch.empty(host.size + 32, dtype=torch.uint8, device=_dev())
    sh = (-raw.data_ptr()) % 16
    t = raw[sh:sh + host.size]
    t.copy_(torch.from_numpy(np.array(host, dtype=np.uint8)))
    return t


def _i64(vals):
    import torch
    return torch.from_numpy(np.array([int(v) for v in vals], dtype=np.uint64).view(np.int64)).to(_dev())


def _i32(vals):
    import torch
    return torch.from_numpy(np.array([int(v) for v in vals], dtype=np.uint64).astype(np.uint32).view(np.int32)).to(_dev())


def odd_layout(ranges):
    """Output offsets of the ranges: odd, GAP or more guard bytes apart; (offsets, total)."""
    offs, cur = [], GAP
    for _, _, ln in ranges:
        cur |= 1
        offs.append(cur)
        cur += (ln if ln <= ROOM_MAX else 0) + GAP
    return offs, cur


def run_ranges(mu, strs, first, pos, ranges, m, nentries=None, stream=None):
    """One smm_uncompress_ranges_device call: (output buffer, offsets, statuses, lengths)."""
    import torch
    gap = bytes([0x5A]) * 3  # the streams lie three bytes apart, so most start at an odd address
    buf = np.frombuffer(gap + gap.join(strs) + gap, np.uint8)
    in_off = np.cumsum([3] + [len(s) + 3 for s in strs[:-1]])
    out_off, total = odd_layout(ranges)
    d_in = _aligned_u8(buf)
    d_out = _aligned_u8(np.full(total, GUARD, np.uint8))
    k = len(ranges)
    d_len = torch.full((k,), 7, dtype=torch.int32, device=_dev())
    d_st = torch.full((k,), -1, dtype=torch.int32, device=_dev())
    pos = np.asarray(pos, np.uint32)
    ne = pos.size if nentries is None else nentries
    args = (d_in, _i64(in_off), _i32([len(s) for s in strs]), _i32(first), _i32(pos if pos.size else [0]),
            _i32([r[0] for r in ranges]), _i32([r[1] for r in ranges]), _i32([r[2] for r in ranges]), m, d_out,
            _i64(out_off), d_len, d_st)
    torch.cuda.synchronize()
    if stream is None:
        mu.uncompress_stream_ranges_device(*args, nentries=ne)
    else:
        with torch.cuda.stream(stream):
            mu.uncompress_stream_ranges_device(*args, nentries=ne)
        stream.synchronize()
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), out_off, d_st.cpu().numpy().tolist(), d_len.cpu().numpy().view(np.uint32).tolist()


def expect_buffer(ranges, out_off, total, datas, ok):
    """The whole output buffer: guards, and the data's slice where ok[r]."""
    want = np.full(total, GUARD, np.uint8)
    for (s, lo, ln), o, good in zip(ranges, out_off, ok):
        if good and ln:
            want[o:o + ln] = np.frombuffer(datas[s][lo:lo + ln], np.uint8)
    return want


def index_arrays(positions):
    first = np.concatenate([[0], np.cumsum([len(p) for p in positions])]).astype(np.uint32)
    return first, np.array([x for p in positions for x in p], np.uint32)


def ladder_ranges(datas):
    """(stream, lo, len) over lo in {0, 1, 65535, 65536, 65537, D - 1, D} and len in {0, 1, 2, 65535,
    65536, 65537, D - lo}: the ones inside the stream, and the ones that end past D."""
    out = []
    for s, d in enumerate(datas):
        D = len(d)
        for lo in sorted({0, 1, 65535, 65536, 65537, max(D - 1, 0), D}):
            for ln in sorted({0, 1, 2, 65535, 65536, 65537, max(D - lo, 0)}):
                out.append((s, lo, ln))
    return out


def check_ladder(mu, datas, strs, first, pos):
    ranges = ladder_ranges(datas) + [(15, 0xFFFFFFFF, 2), (7, 0xFFFFFFFF, 2), (len(datas), 0, 1), (len(datas), 0, 0)]
    inside = [s < len(datas) and lo + ln <= len(datas[s]) for s, lo, ln in ranges]
    want_st = [0 if (ln == 0 or ins) else A for (s, lo, ln), ins in zip(ranges, inside)]
    m = sum(M.range_fragment_count(lo, ln) for (s, lo, ln), ins in zip(ranges, inside) if ins)
    assert M.plan(strs, first, pos, len(pos), ranges)[3:] == (want_st, m)  # the model agrees with the contract
    out, out_off, st, ol = run_ranges(mu, strs, first, pos, ranges, m)
    assert st == want_st
    assert ol == [ln if ins else 0 for (s, lo, ln), ins in zip(ranges, inside)]
    assert all(o % 2 == 1 for o in out_off)
    want = expect_buffer(ranges, out_off, out.size, datas, inside)
    bad = np.nonzero(out != want)[0]
    assert bad.size == 0, "first differing byte at %d" % bad[0]  # bytes, and every guard byte
    assert sum(1 for x in inside if not x) > 100 and m > 256  # (more slots than one scan tile)


@pytest.mark.parametrize("mode", ["reference", "fast", "dense"])
def test_ladder(mu, mode):
    datas = R.ladder_datas()
    assert sorted(set(len(d) for d in datas)) == list(R.LADDER)
    strs, (first, pos) = mu.compress_streams(datas, mode=mode, return_index=True)
    check_ladder(mu, datas, strs, first, pos)


def test_foreign_writers(mu, oracle):
    """Streams a CPU compressor wrote, with the index built on the device."""
    datas = R.ladder_datas()
    strs = [oracle.compress(d) for d in datas]
    first, pos, built = mu.index_streams(strs)
    assert built.tolist() == [1 if len(d) > 65536 else 0 for d in datas]
    check_ladder(mu, datas, strs, first, pos)


def _first_copy(stream, at, end):
    """(position of the tag, its kind 1 or 2) of the first copy tag in stream[at:end)."""
    while at < end:
        t = stream[at]
        if t & 3 == 0:
            n = t >> 2
            extra = max(n - 59, 0)
            length = (int.from_bytes(stream[at + 1:at + 1 + extra], "little") if extra else n) + 1
            at += 1 + extra + length
        else:
            return at, t & 3
    raise AssertionError("no copy in the fragment")


def test_damage(mu, sm, oracle):
    """One byte of fragment 1 changed so that its first copy has offset 0: ranges touching fragment 1
    report what the fragment decoder gives that fragment alone, ranges beside it are served."""
    import torch
    text = R.sources()[0]
    data = text[:65536] + b"wxyz" * 12 + text[70000:70000 + 65536 - 48] + text[5:1005]
    assert len(data) == 2 * 65536 + 1000
    stream, pos = R.cpu_index(data, oracle)
    at, kind = _first_copy(stream, pos[1], pos[2])
    s = bytearray(stream)
    if kind == 1:
        assert s[at] >> 5 == 0 and s[at + 1] != 0  # the offset's high bits are 0: its low byte decides
    else:
        assert kind == 2 and s[at + 2] == 0 and s[at + 1] != 0
    s[at + 1] = 0
    s = bytes(s)
    # the fragment decoder's status for fragment 1 alone, from the existing call
    d_in = _aligned_u8(np.frombuffer(s, np.uint8))
    d_out = torch.zeros(65536, dtype=torch.uint8, device=_dev())
    d_ol = torch.zeros(1, dtype=torch.int32, device=_dev())
    d_st = torch.zeros(1, dtype=torch.int32, device=_dev())
    sm.uncompress_fragments_device(d_in, _i64([pos[1]]), _i32([pos[2] - pos[1]]), d_out, _i64([0]), _i32([65536]), d_ol, d_st)
    torch.cuda.synchronize()
    X = int(d_st.item())
    assert X not in (0, A)
    first, p = index_arrays([pos])
    ranges = [(0, 0, 65536), (0, 100, 1000), (0, 65535, 1), (0, 131072, 1000), (0, 131073, 5), (0, 65536, 65536),
              (0, 65536, 1), (0, 70000, 10), (0, 131071, 1), (0, 65535, 2), (0, 131071, 2), (0, 0, len(data)),
              (0, 1, len(data) - 2)]
    touches = [lo >> 16 <= 1 <= (lo + ln - 1) >> 16 for _, lo, ln in ranges]
    want_st = [X if t else 0 for t in touches]
    model = M.decode_model([s], first, p, p.size, ranges, lambda s_, f, lo, hi: X if f == 1 else 0, [data])
    assert [r[0] for r in model] == want_st
    m = M.plan([s], first, p, p.size, ranges)[4]
    out, out_off, st, ol = run_ranges(mu, [s], first, p, ranges, m)
    assert st == want_st
    assert ol == [0 if t else ln for (_, lo, ln), t in zip(ranges, touches)]
    want = expect_buffer(ranges, out_off, out.size, [data], [not t for t in touches])
    for (_, lo, ln), o, t in zip(ranges, out_off, touches):  # a failing range's bytes are unspecified, inside its room
        if t:
            want[o:o + ln] = out[o:o + ln]
    assert np.array_equal(out, want)


def test_hostile_index(mu, oracle):
    """Streams [A, empty, B, empty, C]: B's entries and frag_first words are broken one way per call;
    the ranges on A and C in the same call are served, and every guard byte stays."""
    src = R.sources()
    dA, dB, dC = src[0][11:11 + 196613], src[1][3:3 + 150000], src[2][9:9 + 70001]
    (sA, pA), (sB, pB), (sC, pC) = (R.cpu_index(d, oracle) for d in (dA, dB, dC))
    empty = b"\x00"
    datas = [dA, b"", dB, b"", dC]
    strs = [sA, empty, sB, empty, sC]
    first0, pos0 = index_arrays([pA, [], pB, [], pC])
    assert first0.tolist() == [0, 4, 4, 7, 7, 9]
    n = len(sB)
    hv, t1, t2 = pB
    healthy = [(0, 65530, 70000), (4, 0, 70001), (0, 196612, 1), (4, 65535, 2), (1, 0, 0)]
    frag = {0: (2, 10, 100), 1: (2, 65536 + 5, 100), 2: (2, 131072 + 5, 100), 12: (2, 131071, 2), 3: (2, 0, 150000)}

    def case(name, first, pos, b_ranges, want_b, nentries=None, strs_=None, datas_=None):
        strs_ = strs if strs_ is None else strs_
        datas_ = datas if datas_ is None else datas_
        ranges = healthy[:2] + b_ranges + healthy[2:]
        ne = len(pos) if nentries is None else nentries
        rc, f_, c_, plan_st, total = M.plan(strs_, first, pos, ne, ranges)
        want_st = [0, 0] + want_b + [0, 0, 0]
        assert plan_st == want_st, name  # the model: every status here is known before any decode
        got = mu.range_plan(strs_, (first, pos), ranges, nentries=ne)
        assert got[2].tolist() == want_st and got[3] == total, name
        out, out_off, st, ol = run_ranges(mu, strs_, first, pos, ranges, total, nentries=ne)
        assert st == want_st, name
        ok = [x == 0 for x in want_st]
        assert ol == [ln if good else 0 for (_, _, ln), good in zip(ranges, ok)], name
        want = expect_buffer(ranges, out_off, out.size, datas_, ok)
        for (_, _, ln), o, good, slots in zip(ranges, out_off, ok, c_):
            if not good and slots:  # a touched fragment failed: the range's own bytes are unspecified
                want[o:o + ln] = out[o:o + ln]
        assert np.array_equal(out, want), name

    case("healthy", first0, pos0, [frag[0], frag[1], frag[2], frag[12], frag[3]], [0] * 5)
    # zeroed entries: a foreign stream whose index could not be built
    sF, dF, _ = R.foreign_stream(31, 140000)
    strsF = [sA, empty, sF, empty, sC]
    fF, pF, built = mu.index_streams(strsF)
    cnt = R.frag_count(len(dF))
    assert built.tolist() == [1, 0, 0, 0, 1] and pF[4:4 + cnt].tolist() == [0] * cnt
    case("zeroed", fF, pF, [(2, 10, 100), (2, 65536, 10), (2, 0, len(dF))], [A] * 3, strs_=strsF,
         datas_=[dA, b"", dF, b"", dC])
    p = pos0.copy()
    p[5] = t2 + 5  # decreasing: hv, t2 + 5, t2
    case("decreasing", first0, p, [frag[1], frag[12], frag[2]], [A, A, 0])
    p[5] = t2      # equal neighbours
    case("equal", first0, p, [frag[1], frag[12], frag[2]], [A, A, 0])
    p = pos0.copy()
    p[6] = n       # the last position at the stream's end
    case("at n", first0, p, [frag[0], frag[2]], [0, A])
    p[6] = n + 7   # ... and past it: fragment 1 ends outside the stream too
    case("past n", first0, p, [frag[0], frag[1], frag[2]], [0, A, A])
    p[6] = 0xFFFFFFFF
    case("far past n", first0, p, [frag[0], frag[1], frag[2]], [0, A, A])
    p = pos0.copy()
    p[4] = hv + 1  # the first position is not the varint's length
    case("first position", first0, p, [frag[0], frag[1], frag[2], frag[3]], [A, 0, 0, A])
    f = first0.copy()
    f[2], f[3] = 7, 4  # frag_first[s] > frag_first[s + 1]
    case("first words decreasing", f, pos0, [frag[0], frag[1], frag[2]], [A] * 3)
    f = first0.copy()
    f[3] = 1000        # frag_first[s + 1] > nentries
    case("first word past nentries", f, pos0, [frag[0], frag[2]], [A] * 2)
    f = first0.copy()
    f[3] = 6           # a count mismatch: two entries for three fragments
    case("count", f, pos0, [frag[0], frag[1], frag[2]], [A] * 3)


def test_bound(mu):
    datas = [R.sources()[0][:196613], R.sources()[1][:70000]]
    strs, (first, pos) = mu.compress_streams(datas, mode="fast", return_index=True)
    ranges = [(0, 1, 196612), (1, 65530, 10), (0, 5, 0), (1, 0, 70000), (0, 131072, 7)]
    total = 4 + 2 + 0 + 2 + 1
    assert M.plan(strs, first, pos, len(pos), ranges)[4] == total
    out, out_off, st, ol = run_ranges(mu, strs, first, pos, ranges, total - 1)
    assert st == [A] * 5 and ol == [0] * 5 and (out == GUARD).all()
    out, out_off, st, ol = run_ranges(mu, strs, first, pos, ranges, total)
    assert st == [0] * 5 and ol == [r[2] for r in ranges]
    assert np.array_equal(out, expect_buffer(ranges, out_off, out.size, datas, [True] * 5))
    out, out_off, st, ol = run_ranges(mu, strs, first, pos, ranges, total + 9)  # (a looser bound)
    assert st == [0] * 5 and np.array_equal(out, expect_buffer(ranges, out_off, out.size, datas, [True] * 5))


def test_scan_tiles(mu):
    """More ranges and more slots than one 256-wide scan tile, fragments shared by many ranges, on a
    stream that is not the default one."""
    import torch
    text = R.sources()[0]
    datas = [text[1000 * k:1000 * k + 200000] for k in range(8)]
    strs, (first, pos) = mu.compress_streams(datas, mode="fast", return_index=True)
    rng = np.random.default_rng(4242)
    ranges = []
    for _ in range(1000):
        ln = int(rng.integers(1, 8193))
        ranges.append((int(rng.integers(0, 8)), int(rng.integers(0, 200000 - ln + 1)), ln))
    m = sum(M.range_fragment_count(lo, ln) for _, lo, ln in ranges)
    touched = [(s, f) for s, lo, ln in ranges for f in range(lo >> 16, ((lo + ln - 1) >> 16) + 1)]
    assert m == len(touched) > 1000 > 256 and len(set(touched)) == 32  # every fragment is shared
    out, out_off, st, ol = run_ranges(mu, strs, first, pos, ranges, m, stream=torch.cuda.Stream(device=_dev()))
    assert st == [0] * 1000 and ol == [r[2] for r in ranges]
    assert np.array_equal(out, expect_buffer(ranges, out_off, out.size, datas, [True] * 1000))


def test_host_twin_and_python(mu):
    datas = [R.sources()[0][:196613], b"", R.sources()[2][:65536], R.sources()[1][:70001], R.sources()[3][:300]]
    strs, (first, pos) = mu.compress_streams(datas, mode="fast", return_index=True)
    whole, st = mu.uncompress_streams(strs, index=(first, pos))
    assert not st.any()
    ranges = [(0, 65530, 70000), (3, 0, 70001), (2, 0, 65536), (4, 299, 1), (0, 7, 0), (3, 65535, 2), (0, 0, 196613),
              (2, 1, 65535), (4, 0, 300), (1, 0, 0)]
    got = mu.uncompress_stream_ranges(strs, (first, pos), ranges)
    assert got == [whole[s][lo:lo + ln] for s, lo, ln in ranges] == [datas[s][lo:lo + ln] for s, lo, ln in ranges]
    assert mu.uncompress_stream_ranges(strs, (first, pos), []) == []
    # a failing range raises its status
    with pytest.raises(mu.SnappyError) as e:
        mu.uncompress_stream_ranges(strs, (first, pos), [(0, 0, 10), (3, 70000, 2)])
    assert e.value.code == A
    # a stream that no range names may be garbage
    junk = list(strs)
    junk[3] = np.random.default_rng(5).integers(0, 256, 5000, dtype=np.uint8).tobytes()
    keep = [r for r in ranges if r[0] != 3]
    assert mu.uncompress_stream_ranges(junk, (first, pos), keep) == [datas[s][lo:lo + ln] for s, lo, ln in keep]


def _twin(mu, ctx, strs, index, ranges):
    """One smm_uncompress_ranges call on ctx: (return code, statuses, lengths, output buffer, offsets);
    the outputs lie GAP guard bytes apart."""
    buf, in_off, in_len, first, pos, rs, lo, ln = mu._range_arrays(strs, index, ranges)
    out_off, total = odd_layout(ranges)
    out = np.full(total, GUARD, np.uint8)
    off = np.array(out_off, np.uint64)
    out_len = np.full(len(ranges), 7, np.uint32)
    status = np.full(len(ranges), -1, np.int32)
    rc = mu.lib().smm_uncompress_ranges(ctx, buf.ctypes.data, mu._addr(in_off), mu._addr(in_len), len(strs),
                                        first.ctypes.data, pos.ctypes.data, rs.ctypes.data, lo.ctypes.data,
                                        ln.ctypes.data, len(ranges), out.ctypes.data, off.ctypes.data,
                                        out_len.ctypes.data, status.ctypes.data)
    return rc, status.tolist(), out_len.tolist(), out, out_off


def test_host_twin_failing_range_on_a_far_stream(mu):
    """A range that fails the stream-level rule names a stream that does not go up, far behind the
    ones that do: on a context that has seen no call (its input buffer is the healthy streams' few
    bytes, and holds nothing from earlier) the device must not look at that stream, the failing range
    gets its status from the rule, and the healthy ranges beside it their bytes."""
    a, c = R.sources()[0][:100], R.sources()[1][:300]
    b = np.random.default_rng(7).integers(0, 256, 1 << 20, dtype=np.uint8).tobytes()  # 1 MiB between the two
    datas = [a, b, c]
    strs, (first, pos) = mu.compress_streams(datas, mode="fast", return_index=True)
    assert len(strs[1]) >= 1 << 20
    short = np.array(first, np.uint32)
    short[3] -= 1  # stream 2 loses its one entry: a count mismatch
    junk = [strs[0], strs[1], b"\xff" * 8]  # a varint that does not parse
    cases = [("lo + len past D", strs, first, [(0, 0, 10), (2, 300, 1), (0, 90, 10), (2, 0, 0)], [0, A, 0, 0]),
             ("count mismatch", strs, short, [(2, 0, 1), (0, 1, 99)], [A, 0]),
             ("varint", junk, first, [(0, 0, 100), (2, 0, 1), (2, 299, 1)], [0, A, A]),
             ("stream number", strs, first, [(3, 0, 1), (0, 50, 1)], [A, 0])]
    for k, (name, strs_, first_, ranges, want) in enumerate(cases):
        ctx = mu.context(("far-stream-%d" % k, 0, 1))  # a context of its own, fresh
        rc, st, ol, out, out_off = _twin(mu, ctx, strs_, (first_, pos), ranges)
        assert rc == 0 and st == want, name
        assert ol == [r[2] if w == 0 else 0 for r, w in zip(ranges, want)], name
        assert np.array_equal(out, expect_buffer(ranges, out_off, out.size, datas, [w == 0 for w in want])), name
