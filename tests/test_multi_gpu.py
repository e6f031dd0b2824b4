"""The multi-stream companion library on the device (include/snappy_mi355x_multi.h): mixed batches
of streams of any length, compressed and decoded in one call each.

Every expected value comes from the CPU oracle, from libsnappy, or from tests/multi_ref.py's plain
statement of the contract over the oracle; the one exception is named in the fast-mode test.  Inputs
and output slots sit at every address mod 16 with canary bytes between them, and the whole buffers
are compared.  Each compress result is computed once per mode and shared."""
import importlib

import numpy as np
import pytest

import multi_ref as R
import streams as S

pytestmark = pytest.mark.gpu

SM_ERR_INPUT_TOO_LARGE = 16
SM_ERR_ARGUMENT = 33
GAP = 48


@pytest.fixture(scope="module")
def mu(sm, gpu_available):
    return importlib.import_module("snappy_jl_amd.multi")


def canary(n):
    return ((np.arange(n, dtype=np.int64) * 131 + 7) & 0xFF).astype(np.uint8)


def _dev():
    import torch
    return torch.device("cuda", 0)


def _aligned_u8(host):
    """host (uint8 array) on the device in a tensor whose data_ptr() is 0 mod 16."""
    import torch
    raw = torch.empty(host.size + 32, dtype=torch.uint8, device=_dev())
    sh = (-raw.data_ptr()) % 16
    t = raw[sh:sh + host.size]
    t.copy_(torch.from_numpy(np.ascontiguousarray(host, dtype=np.uint8)))
    return t


def _i64(vals):
    import torch
    return torch.from_numpy(np.array([int(v) % (1 << 64) for v in vals], dtype=np.uint64).view(np.int64)).to(_dev())


def _i32(vals):
    import torch
    return torch.from_numpy(np.array([int(v) for v in vals], dtype=np.uint64).astype(np.uint32).view(np.int32)).to(_dev())


def _u32(t):
    return t.cpu().numpy().view(np.uint32).astype(np.int64)


def layout(sizes, first_mod=0):
    """Offsets of ranges of these sizes, GAP or more canary bytes apart, range k at an offset that is
    (first_mod + k) mod 16; (offsets, total bytes)."""
    offs, cur = [], GAP
    for k, n in enumerate(sizes):
        cur += (first_mod + k - cur) % 16
        offs.append(cur)
        cur += n + GAP
    return offs, cur


def pack_inputs(items, first_mod=0):
    offs, total = layout([len(d) for d in items], first_mod)
    buf = canary(total)
    for o, d in zip(offs, items):
        buf[o:o + len(d)] = np.frombuffer(d, np.uint8)
    return buf, offs


def run_compress(mu, datas, mode, max_fragments=None, index=True, lens=None):
    """One smm_compress_device call.  lens: the lengths passed instead of the datas' own."""
    import torch
    n = len(datas)
    buf, in_off = pack_inputs(datas)
    lens = [len(d) for d in datas] if lens is None else lens
    rooms = [R.max_compressed_length(len(d)) for d in datas]
    out_off, total = layout(rooms, first_mod=5)
    fill = canary(total)
    d_in, d_out = _aligned_u8(buf), _aligned_u8(fill)
    m = int(mu.frag_first_of(lens)[-1]) if max_fragments is None else max_fragments
    d_len = torch.full((n,), 7, dtype=torch.int32, device=_dev())
    d_st = torch.full((n,), -1, dtype=torch.int32, device=_dev())
    d_first = torch.full((n + 1,), -1, dtype=torch.int32, device=_dev()) if index else None
    d_pos = torch.full((max(m, 1),), -1, dtype=torch.int32, device=_dev()) if index else None
    mu.compress_streams_device(d_in, _i64(in_off), _i32(lens), m, d_out, _i64(out_off), d_len, d_st, d_first, d_pos,
                               mode=mode)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    ol, st = _u32(d_len), d_st.cpu().numpy()
    outside = np.ones(total, bool)
    for o, r in zip(out_off, rooms):
        outside[o:o + r] = False
    return {"streams": [out[o:o + int(l)].tobytes() for o, l in zip(out_off, ol)], "len": ol, "status": st,
            "first": _u32(d_first) if index else None, "pos": _u32(d_pos) if index else None, "m": m,
            "stray": int(((out != fill) & outside).sum()), "untouched": bool((out == fill).all()),
            "in_mod": [(d_in.data_ptr() + o) % 16 for o in in_off], "out_mod": [(d_out.data_ptr() + o) % 16 for o in out_off]}


def run_uncompress(mu, strs, caps, first=None, pos=None, m=None):
    """One smm_uncompress_device call: (outputs or None, status, lengths, streams decoded by
    fragments, bytes changed outside the streams' output ranges)."""
    import torch
    n = len(strs)
    buf, in_off = pack_inputs(strs, first_mod=3)
    out_off, total = layout(caps, first_mod=9)
    fill = canary(total)
    d_in, d_out = _aligned_u8(buf), _aligned_u8(fill)
    d_len = torch.full((n,), 7, dtype=torch.int32, device=_dev())
    d_st = torch.full((n,), -1, dtype=torch.int32, device=_dev())
    d_first = d_pos = None
    if first is not None:
        m = len(pos) if m is None else m
        d_first = _i32(first)
        d_pos = _i32(list(pos) + [0xDEADBEEF] * max(m - len(pos), 1))
    mu.uncompress_streams_device(d_in, _i64(in_off), _i32([len(s) for s in strs]), m or 0, d_out, _i64(out_off), _i32(caps),
                                 d_len, d_st, d_first, d_pos)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    ol, st = _u32(d_len), d_st.cpu().numpy()
    outside = np.ones(total, bool)
    for o, c in zip(out_off, caps):
        outside[o:o + c] = False
    outs = [out[o:o + int(l)].tobytes() if s == 0 else None for o, l, s in zip(out_off, ol, st)]
    return outs, st, ol, mu.last_indexed(0), int(((out != fill) & outside).sum())


def check_against_model(mu, oracle, strs, caps, first, pos, m, what):
    want = R.model_batch(strs, caps, first, pos, m, oracle)
    outs, st, ol, nidx, stray = run_uncompress(mu, strs, caps, first, pos, m)
    assert stray == 0, what
    bad = [(k, int(st[k]), w[0]) for k, w in enumerate(want) if int(st[k]) != w[0]]
    assert not bad, (what, bad[:8])
    for k, w in enumerate(want):
        assert int(ol[k]) == (len(w[1]) if w[0] == 0 else 0), (what, k)
        assert outs[k] == w[1], (what, k)
    assert nidx == sum(1 for w in want if w[2]), what
    return want


_LADDER = {}


def ladder(mu, mode):
    if mode not in _LADDER:
        _LADDER[mode] = run_compress(mu, R.ladder_datas(), mode)
    return _LADDER[mode]


# ---- 1-3. compress over the ladder ---------------------------------------------------------------------

def test_ladder_reference_is_the_oracles_bytes(mu, oracle):
    datas = R.ladder_datas()
    assert sorted(len(d) for d in datas) == sorted(R.LADDER * 2)
    r = ladder(mu, "reference")
    assert set(r["in_mod"]) == set(range(16)) and set(r["out_mod"]) == set(range(16))
    assert not r["status"].any()
    for k, d in enumerate(datas):
        want = oracle.compress(d)
        assert int(r["len"][k]) == len(want), k
        assert r["streams"][k] == want, (k, len(d))
    assert r["stray"] == 0


@pytest.mark.parametrize("mode", ["fast", "dense"])
def test_ladder_fast_modes(mu, sm, oracle, request, mode):
    """Every stream decodes under the oracle and libsnappy, and equals sm.compress(data, mode) -- the
    one expectation here that comes from the library: both are built from the same fragments."""
    datas = R.ladder_datas()
    r = ladder(mu, mode)
    assert not r["status"].any() and r["stray"] == 0
    try:
        libsnappy = request.getfixturevalue("libsnappy")
    except pytest.skip.Exception:  # (libsnappy is not on this host: the oracle alone)
        libsnappy = None
    for k, d in enumerate(datas):
        s = r["streams"][k]
        assert len(s) <= R.max_compressed_length(len(d))
        assert oracle.uncompress(s) == d, k
        assert libsnappy is None or libsnappy.uncompress(s) == d, k
        assert s == sm.compress(d, mode=mode), (k, len(d))


@pytest.mark.parametrize("mode", ["reference", "fast", "dense"])
def test_index(mu, oracle, mode):
    datas = R.ladder_datas()
    r = ladder(mu, mode)
    want_first = np.concatenate([[0], np.cumsum([R.frag_count(len(d)) for d in datas])])
    assert r["first"].tolist() == want_first.tolist() == mu.frag_first_of([len(d) for d in datas]).tolist()
    for k, d in enumerate(datas):
        s = r["streams"][k]
        ent = r["pos"][want_first[k]:want_first[k + 1]].tolist() + [len(s)]
        if d:
            assert ent[0] == len(S.varint(len(d)))
        for f in range(len(ent) - 1):
            part = d[f * R.BLOCK:(f + 1) * R.BLOCK]
            assert oracle.uncompress(S.varint(len(part)) + s[ent[f]:ent[f + 1]]) == part, (k, f)


# ---- 4. decode of those outputs -------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["reference", "fast", "dense"])
def test_decode_with_and_without_index(mu, oracle, mode):
    datas = R.ladder_datas()
    r = ladder(mu, mode)
    caps = [len(d) for d in datas]
    nlong = sum(1 for d in datas if len(d) > R.BLOCK)
    assert nlong == 8
    for first, pos, want_idx in ((r["first"], r["pos"].tolist(), nlong), (None, None, 0)):
        outs, st, ol, nidx, stray = run_uncompress(mu, r["streams"], caps, first, pos, r["m"] if first is not None else 0)
        assert not st.any() and stray == 0
        assert ol.tolist() == caps
        assert outs == datas
        assert nidx == want_idx
    # the model agrees about which streams are indexed
    want = R.model_batch(r["streams"], caps, r["first"], r["pos"], r["m"], oracle)
    assert [w[2] for w in want] == [len(d) > R.BLOCK for d in datas]


# ---- 5. foreign streams ------------------------------------------------------------------------------

def test_foreign_streams_fall_back(mu, oracle):
    strs, caps, first, pos = [], [], [0], []
    for seed, target in ((1, 70000), (2, 140000), (3, 190000)):
        s, e, p = R.foreign_stream(seed, target)
        assert 2 <= len(p) <= 3
        assert oracle.uncompress(s) == e
        strs.append(s)
        caps.append(len(e))
        pos += p
        first.append(len(pos))
    want = check_against_model(mu, oracle, strs, caps, first, pos, len(pos), "foreign")
    assert all(w[0] == 0 for w in want) and not any(w[2] for w in want)  # decoded, through the fallback


# ---- 6. index abuse ------------------------------------------------------------------------------------

def _abuse_base(oracle):
    datas = [R.sources()[k][5:5 + n] for k, n in ((0, 196613), (3, 300), (1, 65537), (4, 0), (2, 131073))]
    idx = [R.cpu_index(d, oracle) for d in datas]
    return datas, [i[0] for i in idx], [list(i[1]) for i in idx]


def _flat(entries):
    first = [0]
    for e in entries:
        first.append(first[-1] + len(e))
    return first, [p for e in entries for p in e]


ABUSE = ("good", "count_minus", "count_plus", "equal_neighbours", "decreasing", "first_not_hv", "last_at_length",
         "last_past_length", "first_decreasing", "first_past_max", "stray_byte")


@pytest.mark.parametrize("name", ABUSE)
def test_index_abuse(mu, oracle, name):
    datas, strs, ent = _abuse_base(oracle)
    caps = [len(d) for d in datas]
    ent = [list(e) for e in ent]
    strs = list(strs)
    first_override = m = None
    if name == "count_minus":
        ent[0] = ent[0][:-1]
    elif name == "count_plus":
        ent[0] = ent[0] + [ent[0][-1] + 1]
    elif name == "equal_neighbours":
        ent[0][2] = ent[0][1]
    elif name == "decreasing":
        ent[4][1], ent[4][2] = ent[4][2], ent[4][1]
    elif name == "first_not_hv":
        ent[0][0] += 1
        ent[2][0] -= 1
    elif name == "last_at_length":
        ent[2][-1] = len(strs[2])
    elif name == "last_past_length":
        ent[0][-1] = 0xFFFFFFF0
        ent[4][1] = len(strs[4]) + 5
    elif name == "stray_byte":  # a byte behind fragment 0 of stream 0, the index moved along with it
        at = ent[0][1]
        strs[0] = strs[0][:at] + b"\x00" + strs[0][at:]
        ent[0] = [ent[0][0]] + [p + 1 for p in ent[0][1:]]
    first, pos = _flat(ent)
    if name == "first_decreasing":
        first[2], first[3] = first[3], first[2]
    elif name == "first_past_max":
        m = len(pos) - 1
    m = len(pos) if m is None else m
    want = check_against_model(mu, oracle, strs, caps, first, pos, m, name)
    indexed = [w[2] for w in want]
    if name == "good":
        assert indexed == [True, False, True, False, True] and all(w[0] == 0 for w in want)
    elif name in ("first_decreasing", "first_past_max"):
        assert not any(indexed) and all(w[0] == 0 for w in want)
    elif name == "stray_byte":
        # the leniency: fragment by fragment the oracle accepts the byte, in stream order it does not
        assert indexed == [True, False, True, False, True] and want[0][0] == 0 and want[0][1] == datas[0]
        assert oracle.uncompress_status(strs[0])[0] != 0
    else:
        assert not all(i == (len(d) > R.BLOCK) for i, d in zip(indexed, datas))


# ---- 7. mutation fuzz -----------------------------------------------------------------------------------

def test_mutation_fuzz_matches_the_model(mu, oracle):
    """400 mutated streams with their original indexes in one call: status, length and (where OK)
    bytes equal the contract's model; nothing outside the output ranges is written."""
    cases = R.fuzz_cases(oracle)
    first, pos, m = R.fuzz_index(cases)
    want = R.fuzz_model(oracle)
    strs, caps = [c[0] for c in cases], [c[1] for c in cases]
    outs, st, ol, nidx, stray = run_uncompress(mu, strs, caps, first.tolist(), pos.tolist(), m)
    assert stray == 0
    bad = [(k, int(st[k]), w[0], w[2]) for k, w in enumerate(want) if int(st[k]) != w[0]]
    assert not bad, bad[:10]
    for k, w in enumerate(want):
        assert int(ol[k]) == (len(w[1]) if w[0] == 0 else 0), k
        assert outs[k] == w[1], k
    assert nidx == sum(1 for w in want if w[2])


# ---- 8. the bound, the empty call, a stream too large --------------------------------------------------

@pytest.mark.parametrize("index", [False, True])
def test_max_fragments_one_too_small(mu, index):
    datas = R.ladder_datas()
    lens = [len(d) for d in datas]
    need = int(mu.frag_first_of(lens)[-1]) if index else sum(R.frag_count(n) for n in lens if n > R.BLOCK)
    r = run_compress(mu, datas, "fast", max_fragments=need - 1, index=index)
    assert r["status"].tolist() == [SM_ERR_ARGUMENT] * len(datas)
    assert r["len"].tolist() == [0] * len(datas)
    assert r["untouched"]
    if index:
        assert set(r["first"].tolist()) == {0xFFFFFFFF} and set(r["pos"].tolist()) == {0xFFFFFFFF}
    r = run_compress(mu, datas, "fast", max_fragments=need, index=index)  # the exact bound
    assert not r["status"].any() and r["streams"] == ladder(mu, "fast")["streams"]


def test_no_streams_and_one(mu, oracle):
    import torch
    e8 = torch.zeros(0, dtype=torch.uint8, device=_dev())
    e64 = torch.zeros(0, dtype=torch.int64, device=_dev())
    e32 = torch.zeros(0, dtype=torch.int32, device=_dev())
    first = torch.full((1,), -1, dtype=torch.int32, device=_dev())
    pos = torch.full((1,), -1, dtype=torch.int32, device=_dev())
    mu.compress_streams_device(e8, e64, e32, 0, e8, e64, e32, e32, first, pos, mode="fast")
    mu.uncompress_streams_device(e8, e64, e32, 0, e8, e64, e32, e32, e32, first, pos)
    torch.cuda.synchronize()
    assert first.item() == 0 and pos.item() == -1 and mu.last_indexed(0) == 0
    for d in (R.sources()[0][:70000], b"", b"x"):
        r = run_compress(mu, [d], "reference")
        assert r["status"].tolist() == [0] and r["streams"] == [oracle.compress(d)] and r["stray"] == 0
        outs, st, ol, nidx, stray = run_uncompress(mu, r["streams"], [len(d)], r["first"], r["pos"].tolist(), r["m"])
        assert outs == [d] and nidx == (1 if len(d) > R.BLOCK else 0) and stray == 0


def test_stream_too_large_fails_alone(mu, oracle):
    datas = [R.sources()[0][:70000], b"never read", R.sources()[1][:300]]
    lens = [70000, 0x80000000, 300]
    r = run_compress(mu, datas, "reference", lens=lens)
    assert r["status"].tolist() == [0, SM_ERR_INPUT_TOO_LARGE, 0]
    assert r["len"][1] == 0 and r["stray"] == 0
    assert r["streams"][0] == oracle.compress(datas[0]) and r["streams"][2] == oracle.compress(datas[2])
    assert r["first"].tolist() == [0, 2, 2, 3] and r["m"] == 3


# ---- 9. the Python host API ----------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["reference", "fast"])
def test_host_api_round_trip(mu, oracle, mode):
    datas = R.ladder_datas()
    strs, (first, pos) = mu.compress_streams(datas, mode=mode, return_index=True)
    assert strs == ladder(mu, mode)["streams"]
    assert first.tolist() == ladder(mu, mode)["first"].tolist() and pos.tolist() == ladder(mu, mode)["pos"][:pos.size].tolist()
    assert mu.compress_streams(datas, mode=mode) == strs
    for index, nidx in (((first, pos), 8), (None, 0)):
        outs, st = mu.uncompress_streams(strs, index=index)
        assert not st.any() and outs == datas
        assert mu.last_indexed(0) == nidx
    assert mu.compress_streams([]) == [] and mu.uncompress_streams([])[0] == []
    assert mu.index_check(strs, (first, pos)).tolist() == [int(len(d) > R.BLOCK) for d in datas]
