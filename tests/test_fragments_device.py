"""The device fragment API at its edges: sm_compress_fragments_device, sm_place_fragments_device and
sm_uncompress_fragments_device, the three entry points the sharded single-stream path (config 5,
snappy.jl_amd/dist.py) is built from.

Every expected value comes from numpy (`place_reference`, a Python loop with slice assignment) or
from the CPU oracle; the one exception is named in the chain test.  Many cases are packed into each
launch.  Groups:

1. placement matrix: every fragment length x source alignment x destination alignment, gapped over
   a canary and back to back, against `place_reference` (k_place: the 16-byte-unit path for aligned
   sources, the byte loop for the others; stray stores show in the canary);
2. the varint header and the host-side argument contract of sm_place_fragments_device;
3. the error contract of placement (error marks, capacity, wrapped offsets, header overlap);
4. raw-mode decode (no varint header, declared length from d_frag_len) under 3,000 seeded
   mutations, against the oracle;
5. the chain compress -> place -> decode at small shapes and odd shard counts, in one process;
6. CPU checks of this file's own model and of its coverage conditions (not marked `gpu`).
"""
import functools

import numpy as np
import pytest

import streams
from conftest import load_package, read_testfile

gpu = pytest.mark.gpu

SM_BUFFER_TOO_SMALL = 2
SM_ERR_INPUT_TOO_LARGE = 16
SM_ERR_DEVICE = 32
SM_OUT_LEN_ERROR = 0xFFF00000
BLOCK = 65536
MAXC = 76490  # sm_max_compressed_length(65536)

# 16,384 bytes are one pass of the 256-thread x 4-blockIdx.y x 16-byte stride: the last four take
# the stride loop
LENGTHS = (0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 47, 48, 49, 255, 256, 257, 4095, 4096, 4097, 16383, 16384, 16400,
           32773, MAXC)
SRC_MOD = (0, 1, 4, 8, 15)  # source address mod 16: 0 = the 16-byte-unit path, the rest = the byte loop
BIG_BASE = 0x123456789  # dst_off[0] without the header: large (> 2^32) and odd
SRC_PAD = 64


def canary(n):
    return ((np.arange(n, dtype=np.int64) * 131 + 7) & 0xFF).astype(np.uint8)


def place_reference(src, src_off, lens, dst_off, total, write_header, dst_init):
    """sm_place_fragments_device in plain Python.  src, dst_init: uint8 arrays; src_off, lens (u32
    values), dst_off: sequences of ints.  Returns (destination bytes, local offsets as Python ints
    mod 2^64, status): status is SM_ERR_DEVICE when a fragment was refused (it is not copied),
    else 0."""
    dst = np.array(dst_init, dtype=np.uint8, copy=True)
    cap = dst.size
    header = streams.varint(total) if write_header else b""
    hv = len(header)
    dst[:hv] = np.frombuffer(header, np.uint8)
    base = 0 if write_header or len(lens) == 0 else int(dst_off[0])
    status, local = 0, []
    for so, n, do in zip(src_off, lens, dst_off):
        so, n = int(so), int(n)
        at = (int(do) - base) % (1 << 64)
        local.append(at)
        if n >= SM_OUT_LEN_ERROR or at > cap or cap - at < n or at < hv:
            status = SM_ERR_DEVICE
            continue
        dst[at:at + n] = src[so:so + n]
    return dst, local, status


# ---- device helpers -----------------------------------------------------------------------------

def _dev():
    import torch
    return torch.device("cuda", 0)


def _aligned_u8(host, mis=0):
    """host (uint8 array) on the device in a tensor whose data_ptr() is `mis` mod 16."""
    import torch
    raw = torch.empty(host.size + 32, dtype=torch.uint8, device=_dev())
    sh = (mis - raw.data_ptr()) % 16
    t = raw[sh:sh + host.size]
    t.copy_(torch.from_numpy(np.array(host, dtype=np.uint8)))
    assert t.data_ptr() % 16 == mis or host.size == 0
    return t


def _i64(vals):
    """u64 values as the int64 tensor the wrappers take."""
    import torch
    return torch.from_numpy(np.array([int(v) % (1 << 64) for v in vals], dtype=np.uint64).view(np.int64)).to(_dev())


def _i32(vals):
    """u32 values as torch int32 (an error mark is negative there, as in bench.py)."""
    import torch
    return torch.from_numpy(np.array([int(v) for v in vals], dtype=np.uint64).astype(np.uint32).view(np.int32)).to(_dev())


def _assert_bytes(got_t, want, what):
    """A device uint8 tensor equals a host array; names the first difference."""
    import torch
    assert got_t.numel() == want.size, what
    if torch.equal(got_t, torch.from_numpy(want).to(got_t.device)):
        return
    got = got_t.cpu().numpy()
    bad = np.nonzero(got != want)[0]
    raise AssertionError("%s: %d bytes differ, first at %d (got %d, want %d)"
                         % (what, bad.size, bad[0], got[bad[0]], want[bad[0]]))


def _place(sm, plan, d_src, header, want_local=True, status0=0):
    """One launch of plan (dict: src_off, lens, dst_off, total, dst_init) -> (d_dst, local, status)."""
    import torch
    d_dst = _aligned_u8(plan["dst_init"])
    n = len(plan["lens"])
    d_loc = torch.full((n,), -1, dtype=torch.int64, device=_dev()) if want_local else None
    d_st = torch.full((1,), status0, dtype=torch.int32, device=_dev()) if status0 is not None else None
    sm.place_fragments_device(d_src, _i64(plan["src_off"]), _i32(plan["lens"]), _i64(plan["dst_off"]), d_dst,
                              plan["total"], header, d_local_off=d_loc, d_status=d_st)
    torch.cuda.synchronize()
    local = [int(x) % (1 << 64) for x in d_loc.cpu().numpy()] if want_local else None
    return d_dst, local, (int(d_st.item()) if d_st is not None else None)


# ---- 1. the placement matrix --------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def matrix_source():
    """Every (length, source class, destination alignment) once: (source bytes, [(src_off, len,
    source class, destination alignment)]) for a source tensor whose data_ptr() is 0 mod 16.  Seeded
    random bytes (gaps included), so neighbouring fragments differ; SRC_PAD bytes behind the last."""
    frags, cur = [], 0
    for n in LENGTHS:
        for sm_ in SRC_MOD:
            for da in range(16):
                off = cur + (sm_ - cur) % 16
                frags.append((off, n, sm_, da))
                cur = off + n
    src = np.random.default_rng(20261).integers(0, 256, cur + SRC_PAD, dtype=np.uint8)
    return src, tuple(frags)


@functools.lru_cache(maxsize=None)
def matrix_plan(layout, header):
    """The destination side for a destination tensor whose data_ptr() is 0 mod 16.
    layout "A": fragments in matrix order, each at its destination alignment behind 32..47 canary
    bytes; layout "B": a seeded shuffle, back to back (neighbours share 16-byte units)."""
    src, frags = matrix_source()
    total = 3 * BLOCK + 77  # (any u32: only the header's bytes depend on it; 3 of them here)
    hv = len(streams.varint(total)) if header else 0
    order = list(range(len(frags)))
    if layout == "B":
        np.random.default_rng(77).shuffle(order)
    at, cur = [], hv
    for k, i in enumerate(order):
        n, da = frags[i][1], frags[i][3]
        if layout == "A" and not (k == 0 and not header):  # (without the header fragment 0 is at 0)
            cur += 32 + (da - (cur + 32)) % 16
        at.append(cur)
        cur += n
    base = 0 if header else BIG_BASE
    return {"src_off": [frags[i][0] for i in order], "lens": [frags[i][1] for i in order],
            "src_mod": [frags[i][2] for i in order], "dst_align": [frags[i][3] for i in order],
            "local": at, "dst_off": [base + a for a in at], "total": total, "dst_init": canary(cur + 64)}


def _coverage(plan, src_ptr, dst_ptr, min_len):
    """{source path: set of destination addresses mod 16} over the fragments of >= min_len bytes."""
    cov = {True: set(), False: set()}
    for so, n, a in zip(plan["src_off"], plan["lens"], plan["local"]):
        if n >= min_len:
            cov[(src_ptr + so) % 16 == 0].add((dst_ptr + a) % 16)
    return cov


def _check_matrix_plan(layout, header, src_ptr=0, dst_ptr=0):
    plan = matrix_plan(layout, header)
    src, _ = matrix_source()
    assert src.size - max(o + n for o, n in zip(plan["src_off"], plan["lens"])) >= SRC_PAD
    assert sorted(plan["lens"]) == sorted(LENGTHS * (16 * len(SRC_MOD)))
    for so, m in zip(plan["src_off"], plan["src_mod"]):
        assert (src_ptr + so) % 16 == m
    if layout == "A":  # every combination at exactly its alignment, 32..47 canary bytes between
        combos = set()
        for k, (n, m, da, a) in enumerate(zip(plan["lens"], plan["src_mod"], plan["dst_align"], plan["local"])):
            if k or header:
                assert (dst_ptr + a) % 16 == da
                prev_end = plan["local"][k - 1] + plan["lens"][k - 1] if k else len(streams.varint(plan["total"]))
                assert 32 <= a - prev_end <= 47
            combos.add((n, m, (dst_ptr + a) % 16))
        assert len(combos) == len(LENGTHS) * len(SRC_MOD) * 16
    else:  # the shuffle reaches every destination alignment on both source paths, short fragments aside
        ends = [a + n for a, n in zip(plan["local"], plan["lens"])]
        assert plan["local"][1:] == ends[:-1]
        cov = _coverage(plan, src_ptr, dst_ptr, 49)
        assert cov[True] == set(range(16)) and cov[False] == set(range(16)), cov
    if not header:
        assert plan["dst_off"][0] == BIG_BASE and BIG_BASE % 2 == 1 and BIG_BASE > 1 << 32


@pytest.mark.parametrize("header", [0, 1])
@pytest.mark.parametrize("layout", ["A", "B"])
def test_matrix_plan_coverage(layout, header):
    """CPU: the matrix really holds every combination (A) / every alignment on both paths (B)."""
    _check_matrix_plan(layout, header)


@gpu
@pytest.mark.parametrize("header", [0, 1])
@pytest.mark.parametrize("layout", ["A", "B"])
def test_place_matrix(sm, gpu_available, layout, header):
    """1,920 fragments per launch: the whole destination (canaries included), the local offsets and
    the status equal place_reference; a status word of 7 stays 7; null outputs work."""
    src, _ = matrix_source()
    plan = matrix_plan(layout, header)
    d_src = _aligned_u8(src)
    want, want_local, want_st = place_reference(src, plan["src_off"], plan["lens"], plan["dst_off"], plan["total"],
                                                header, plan["dst_init"])
    assert want_st == 0 and want_local == plan["local"]
    d_dst, local, st = _place(sm, plan, d_src, header)
    # the addresses, from data_ptr(): the plan's alignments are the device's
    _check_matrix_plan(layout, header, d_src.data_ptr(), d_dst.data_ptr())
    _assert_bytes(d_dst, want, "layout %s header %d" % (layout, header))
    assert local == [d - (0 if header else BIG_BASE) for d in plan["dst_off"]]
    assert st == 0
    d_dst, local, st = _place(sm, plan, d_src, header, status0=7)  # never cleared
    _assert_bytes(d_dst, want, "status 7")
    assert st == 7 and local == want_local
    d_dst, _, _ = _place(sm, plan, d_src, header, want_local=False, status0=None)  # null outputs
    _assert_bytes(d_dst, want, "null outputs")


# ---- 2. header and host-side argument contract ---------------------------------------------------

TOTALS = (0, 1, 127, 128, 16383, 16384, 2**21 - 1, 2**21, 2**28 - 1, 2**28, 2**32 - 1)


@gpu
def test_place_header_varint_boundaries(sm, gpu_available):
    import torch
    rng = np.random.default_rng(5)
    src = rng.integers(0, 256, 200 + SRC_PAD, dtype=np.uint8)
    d_src = _aligned_u8(src)
    empty64 = torch.zeros(0, dtype=torch.int64, device=_dev())
    empty32 = torch.zeros(0, dtype=torch.int32, device=_dev())
    for total in TOTALS:
        hdr = np.frombuffer(streams.varint(total), np.uint8)
        hv = hdr.size
        assert hv == 1 + (total >= 1 << 7) + (total >= 1 << 14) + (total >= 1 << 21) + (total >= 1 << 28)
        # no fragments: the header alone (rank 0 of the empty stream), the canary behind it untouched
        want = canary(64)
        want[:hv] = hdr
        d_dst = _aligned_u8(canary(64))
        d_st = torch.zeros(1, dtype=torch.int32, device=_dev())
        sm.place_fragments_device(empty64.to(torch.uint8), empty64, empty32, empty64, d_dst, total, 1, d_status=d_st)
        torch.cuda.synchronize()
        _assert_bytes(d_dst, want, "header alone, total %d" % total)
        assert int(d_st.item()) == 0
        # two fragments right behind the header (sources on both paths)
        plan = {"src_off": [16, 81], "lens": [33, 70], "dst_off": [hv, hv + 33], "total": total,
                "dst_init": canary(hv + 33 + 70 + 64)}
        want, want_local, want_st = place_reference(src, plan["src_off"], plan["lens"], plan["dst_off"], total, 1,
                                                    plan["dst_init"])
        assert bytes(want[:hv]) == streams.varint(total) and want_st == 0
        d_dst, local, st = _place(sm, plan, d_src, 1)
        _assert_bytes(d_dst, want, "header + fragments, total %d" % total)
        assert local == want_local and st == 0


@gpu
def test_place_host_argument_contract(sm, gpu_available):
    import torch
    src = np.random.default_rng(6).integers(0, 256, 100 + SRC_PAD, dtype=np.uint8)
    d_src = _aligned_u8(src)
    d_big = _aligned_u8(canary(256))
    d_st = torch.full((1,), 7, dtype=torch.int32, device=_dev())
    args = (d_src, _i64([0]), _i32([40]), _i64([5]))
    # a total past u32: SM_ERR_INPUT_TOO_LARGE, with and without the header, fragments or none
    for header in (0, 1):
        with pytest.raises(sm.SnappyError) as e:
            sm.place_fragments_device(*args, d_big, 2**32, header, d_status=d_st)
        assert e.value.code == SM_ERR_INPUT_TOO_LARGE
    # room for less than the header: SM_BUFFER_TOO_SMALL, nothing written
    for total, hv in ((128, 2), (2**21, 4), (2**28, 5), (2**32 - 1, 5)):
        assert len(streams.varint(total)) == hv
        for cap in range(1, hv):
            with pytest.raises(sm.SnappyError) as e:
                sm.place_fragments_device(*args, d_big[64:64 + cap], total, 1, d_status=d_st)
            assert e.value.code == SM_BUFFER_TOO_SMALL
    # no fragments and no header: returns normally, nothing written
    e64 = torch.zeros(0, dtype=torch.int64, device=_dev())
    sm.place_fragments_device(e64.to(torch.uint8), e64, e64.to(torch.int32), e64, d_big[64:128], 1000, 0, d_status=d_st)
    sm.place_fragments_device(e64.to(torch.uint8), e64, e64.to(torch.int32), e64, d_big[64:64], 1000, 0)
    torch.cuda.synchronize()
    _assert_bytes(d_big, canary(256), "refused calls wrote")
    assert int(d_st.item()) == 7


# ---- 3. the error contract of placement ----------------------------------------------------------

GOOD_LENS = (0, 1, 17, 48, 255, 4097, 16400)
FRONT = 256  # canary in front of and behind d_dst (the same allocation): wrapped or late stores show


def _error_case(name):
    """(plan, header, cap, bad indices): good fragments of GOOD_LENS, 40 canary bytes apart, with the
    case's bad fragments among them.  dst_off are offsets in d_dst (plus BIG_BASE without the header)."""
    rng = np.random.default_rng(9)
    header = 0 if name.endswith("_noheader") or name == "wrap" else 1
    total = 2**21  # (a 4-byte header)
    hv = len(streams.varint(total)) if header else 0
    frags, cur, soff = [], hv, 0  # (src_off, len, at, bad)

    def add(n, at=None, bad=False, real=None):
        nonlocal cur, soff
        real = n if real is None else real  # (the source bytes reserved for it)
        soff += int(rng.integers(0, 16))
        if at is None:
            at = cur = cur + (40 if frags or header else 0)
            cur += real
        frags.append((soff, n, at, bad))
        soff += real

    def goods(k):
        for n in GOOD_LENS[k::2]:
            add(n)

    goods(0)
    if name.startswith("marks"):
        for mark in (0xFFF00000, 0xFFF00001, 0xFFFFFFFF):
            add(mark, bad=True, real=64)
            add(33)
    elif name == "wrap":
        add(64, at=-5, bad=True)
        add(0, at=-1, bad=True)
    elif name == "header_overlap":
        # (a fragment at exactly hv is good: test_place_header_varint_boundaries)
        frags.insert(0, (soff, 17, hv - 1, True))  # fragment 0, as a bad offset table would have it
        soff += 17
        add(17, at=0, bad=True)
        add(0, at=2, bad=True)
    goods(1)
    cap = cur + 40
    if name.startswith("cap"):
        add(0, at=cap)  # an empty fragment at the very end: good
        if name.startswith("cap_exact"):
            add(29, at=cap - 29)  # ends exactly at capacity: good
        else:
            add(29, at=cap - 28, bad=True)  # ends one byte past it
            add(0, at=cap + 1, bad=True)
            add(1, at=cap, bad=True)
    src = rng.integers(0, 256, soff + SRC_PAD, dtype=np.uint8)
    base = 0 if header else BIG_BASE
    if not header:
        assert frags[0][2] == 0 and not frags[0][3]
    plan = {"src_off": [f[0] for f in frags], "lens": [f[1] for f in frags], "local": [f[2] % (1 << 64) for f in frags],
            "dst_off": [base + f[2] for f in frags], "total": total}
    return src, plan, header, cap, [i for i, f in enumerate(frags) if f[3]]


ERROR_CASES = ("marks", "marks_noheader", "cap_exact", "cap_exact_noheader", "cap_past", "cap_past_noheader", "wrap",
               "header_overlap")


@gpu
@pytest.mark.parametrize("name", ERROR_CASES)
def test_place_error_contract(sm, gpu_available, name):
    """A bad fragment among good ones in one launch: status SM_ERR_DEVICE, its destination bytes
    still canary, every good fragment (and the header) placed exactly, nothing else written."""
    import torch
    src, plan, header, cap, bad = _error_case(name)
    whole = canary(FRONT + cap + FRONT)
    want, want_local, want_st = place_reference(src, plan["src_off"], plan["lens"], plan["dst_off"], plan["total"],
                                                header, whole[FRONT:FRONT + cap])
    assert want_local == plan["local"]
    assert want_st == (SM_ERR_DEVICE if bad else 0) and (bad or name.startswith("cap_exact"))
    want_whole = whole.copy()
    want_whole[FRONT:FRONT + cap] = want
    d_src = _aligned_u8(src)
    for status0 in (0, 7):
        d_whole = _aligned_u8(whole)
        d_loc = torch.full((len(plan["lens"]),), -1, dtype=torch.int64, device=_dev())
        d_st = torch.full((1,), status0, dtype=torch.int32, device=_dev())
        sm.place_fragments_device(d_src, _i64(plan["src_off"]), _i32(plan["lens"]), _i64(plan["dst_off"]),
                                  d_whole[FRONT:FRONT + cap], plan["total"], header, d_local_off=d_loc, d_status=d_st)
        torch.cuda.synchronize()
        got = d_whole.cpu().numpy()
        assert int(d_st.item()) == (SM_ERR_DEVICE if bad else status0)
        hv = len(streams.varint(plan["total"])) if header else 0
        assert bytes(got[FRONT:FRONT + hv]) == (streams.varint(plan["total"]) if header else b""), "header"
        for i, (so, n, at) in enumerate(zip(plan["src_off"], plan["lens"], plan["local"])):
            if i in bad:
                if n < SM_OUT_LEN_ERROR and at < cap:  # its bytes (behind the header) are still canary
                    a, b = FRONT + max(at, hv), min(FRONT + at + n, whole.size)
                    assert np.array_equal(got[a:b], whole[a:b]), "bad fragment %d was copied" % i
            else:
                assert np.array_equal(got[FRONT + at:FRONT + at + n], src[so:so + n]), "good fragment %d" % i
        _assert_bytes(d_whole, want_whole, name)
        assert [int(x) % (1 << 64) for x in d_loc.cpu().numpy()] == want_local


# ---- 4. raw-mode decode against the oracle -------------------------------------------------------

_FUZZ = {}


def fuzz_cases(oracle):
    """[(body, declared length, oracle status, oracle output or None)]: every base body unmodified,
    then 3,000 seeded mutations.  The oracle sees varint(decl) + body."""
    if "cases" in _FUZZ:
        return _FUZZ["cases"]
    datas = [read_testfile(f)[:n] for f in ("html", "alice29.txt", "kppkn.gtb", "urls.10K") for n in (1, 63, 700, 4096)]
    datas += [b"ab" * 700, bytes(range(256)) * 3, b"", bytes(5000), read_testfile("alice29.txt")[:BLOCK]]
    bases = []
    for d in datas:
        body = oracle.compress(d)[len(streams.varint(len(d))):]
        assert body == oracle.compress_fragment(d, len(d))
        bases.append((body, len(d), d))
    rng = np.random.default_rng(4321)
    for target, max_off in ((2000, 300), (30000, 4096), (60000, 65535)):
        s, e = streams.build(streams.random_ops(rng, target, max_off=max_off))
        assert len(e) <= BLOCK
        bases.append((s[len(streams.varint(len(e))):], len(e), e))
    cases = [(body, decl) for body, decl, _ in bases]
    for i in range(3000):
        body, decl, _ = bases[i % len(bases)]
        s = bytearray(body)
        kind = int(rng.integers(0, 6))
        if kind == 0 and s:  # 1-3 byte flips
            for _ in range(int(rng.integers(1, 4))):
                s[int(rng.integers(0, len(s)))] = int(rng.integers(0, 256))
        elif kind == 1 and s:  # truncation
            s = s[: int(rng.integers(0, len(s)))]
        elif kind == 2:  # 1-5 appended bytes
            s += rng.integers(0, 256, int(rng.integers(1, 6)), dtype=np.uint8).tobytes()
        elif kind == 3 and s:  # a flip plus tail trim
            s[int(rng.integers(0, len(s)))] = int(rng.integers(0, 256))
            s = s[: max(1, len(s) - int(rng.integers(0, 8)))]
        elif kind == 4:  # a wrong declared length
            decl = min(max(decl + int(rng.choice([-17, -1, 1, 40])), 0), BLOCK)
        cases.append((bytes(s), decl))  # (kind 5, and an empty body's flips: unmodified)
    out = []
    for k, (body, decl) in enumerate(cases):
        st, dec = oracle.uncompress_status(streams.varint(decl) + body)
        if k < len(bases):  # a valid body: the data it was made from (random_ops: build()'s expectation)
            assert st == 0 and dec == bases[k][2]
        assert st != 0 or len(dec) == decl
        out.append((body, decl, st, dec))
    _FUZZ["cases"] = out
    return out


def test_fuzz_case_spread(oracle):
    """CPU: the oracle's statuses over the case set include every decode error, often."""
    st = np.array([c[2] for c in fuzz_cases(oracle)])
    counts = {code: int((st == code).sum()) for code in (0, 17, 19, 20, 21)}
    assert all(v >= 100 for v in counts.values()), counts
    assert sum(counts.values()) == st.size, np.unique(st)


@gpu
def test_raw_decode_fuzz_matches_oracle(sm, oracle, gpu_available):
    """One launch: status and d_out_len equal the oracle's for every case, the bytes wherever it
    returns OK, error-mark lengths give SM_ERR_DEVICE, and no byte outside the fragments' own output
    ranges is written.  Inputs and output slots are packed back to back."""
    import torch
    cases = list(fuzz_cases(oracle))
    marks = {len(cases) // 3: 0xFFF00000, 2 * len(cases) // 3: 0xFFFFFFFF}  # index -> d_in_len
    for k in sorted(marks):
        cases.insert(k, (b"\x00" * 40, 100, SM_ERR_DEVICE, None))
    n = len(cases)
    in_len = np.array([len(c[0]) for c in cases], np.int64)
    decl = np.array([c[1] for c in cases], np.int64)
    in_off = np.cumsum(in_len) - in_len
    out_off = np.cumsum(decl) - decl
    inp = np.concatenate([np.frombuffer(b"".join(c[0] for c in cases), np.uint8), np.zeros(256, np.uint8)])
    fill = canary(int(decl.sum()) + 256)
    want, own = fill.copy(), np.zeros(fill.size, bool)  # own: a failed fragment's range (unspecified)
    for (body, d, st, dec), o, k in zip(cases, out_off, range(n)):
        if st == 0:
            want[o:o + d] = np.frombuffer(dec, np.uint8)
        elif k not in marks:
            own[o:o + d] = True
    d_in = _aligned_u8(inp)
    d_out = _aligned_u8(fill)
    d_len = in_len.copy()
    for k, m in marks.items():
        d_len[k] = m
    d_out_len = torch.full((n,), 7, dtype=torch.int32, device=_dev())
    d_st = torch.full((n,), -1, dtype=torch.int32, device=_dev())
    sm.uncompress_fragments_device(d_in, _i64(in_off), _i32(d_len), d_out, _i64(out_off), _i32(decl), d_out_len, d_st)
    torch.cuda.synchronize()
    st_g, len_g, got = d_st.cpu().numpy(), d_out_len.cpu().numpy(), d_out.cpu().numpy()
    st_o = np.array([c[2] for c in cases], np.int32)
    diff = np.nonzero(st_g != st_o)[0]
    assert diff.size == 0, [(int(k), int(st_g[k]), int(st_o[k])) for k in diff[:8]]
    assert np.array_equal(len_g, np.where(st_o == 0, decl, 0).astype(np.int32))
    bad = np.nonzero((got != want) & ~own)[0]
    assert bad.size == 0, (bad.size, int(bad[0]), int(np.searchsorted(out_off, bad[0], "right") - 1))


# ---- 5. the chain, at small shapes and odd shard counts ------------------------------------------

WORLDS = (1, 2, 3, 5, 7)


def chain_datas():
    return [read_testfile("html_x_4")[: 4 * BLOCK + 1234], b"z", b""]


def _shards(D, total, world):
    nfrag = (total + BLOCK - 1) // BLOCK
    return nfrag, [D.shard_range(nfrag, r, world) for r in range(world)]


def _dist():
    load_package()
    from importlib import import_module
    return import_module("snappy_jl_amd.dist")


def test_place_reference_builds_the_oracle_stream(oracle):
    """CPU: place_reference over the oracle's own fragments, rank by rank into exactly-sized ranges,
    is oracle.compress(data), at every world size of the chain test."""
    D = _dist()
    for data in chain_datas():
        total = len(data)
        hv = len(streams.varint(total))
        for world in WORLDS:
            nfrag, shards = _shards(D, total, world)
            frags = [oracle.compress_fragment(data[f * BLOCK:(f + 1) * BLOCK], total) for f in range(nfrag)]
            sizes = np.array([len(f) for f in frags], np.int64)
            offs = hv + np.cumsum(sizes) - sizes
            assert sorted(hi - lo for lo, hi in shards)[0] == (0 if world > nfrag else nfrag // world)
            stream = b""
            for rank, (lo, hi) in enumerate(shards):
                mine = frags[lo:hi]
                src = np.frombuffer(b"".join(mine), np.uint8)
                src_off = np.cumsum(sizes[lo:hi]) - sizes[lo:hi]
                size = int(sizes[lo:hi].sum()) + (hv if rank == 0 else 0)
                dst, local, st = place_reference(src, src_off, sizes[lo:hi], offs[lo:hi], total, rank == 0, canary(size))
                assert st == 0
                stream += dst.tobytes()
            assert stream == oracle.compress(data)


@gpu
@pytest.mark.parametrize("mode", ["reference", "fast", "dense"])
def test_chain_odd_shard_counts(sm, oracle, gpu_available, mode):
    """compress -> place -> decode per rank in a plain loop: the concatenated ranges are the
    oracle's stream (reference) or decode under it and equal sm.compress(data, mode) -- the one
    expectation here that comes from the library, the single-GPU stream of the same input."""
    import torch
    D = _dist()
    dev = _dev()
    for data in chain_datas():
        total = len(data)
        hv = len(streams.varint(total))
        data_np = np.frombuffer(data, np.uint8)
        expect = oracle.compress(data) if mode == "reference" else sm.compress(data, mode=mode)
        for world in WORLDS:
            nfrag, shards = _shards(D, total, world)
            ranks = []
            for rank, (lo, hi) in enumerate(shards):
                nf = hi - lo
                a, b = lo * BLOCK, min(hi * BLOCK, total)
                lens = np.minimum(BLOCK, total - np.arange(lo, hi, dtype=np.int64) * BLOCK)
                # odd ranks: slots at a pitch and base that are no multiples of 16 (k_place's byte loop)
                pitch, first = (MAXC + 6, 0) if rank % 2 == 0 else (MAXC + 11, 3)
                assert (MAXC + 6) % 16 == 0
                r = {"nf": nf, "d_in": _aligned_u8(data_np[a:b]), "in_off": _i64(np.arange(nf) * BLOCK),
                     "in_len": _i32(lens), "d_comp": _aligned_u8(canary(first + max(nf, 1) * pitch)),
                     "comp_off": _i64(first + np.arange(nf) * pitch),
                     "comp_len": torch.zeros(nf, dtype=torch.int32, device=dev)}
                sm.compress_fragments_device(r["d_in"], r["in_off"], r["in_len"], r["d_comp"], r["comp_off"],
                                             r["comp_len"], total, mode=mode)
                ranks.append(r)
            torch.cuda.synchronize()
            sizes = np.concatenate([r["comp_len"].cpu().numpy().astype(np.int64) & 0xFFFFFFFF for r in ranks])
            assert sizes.size == nfrag and (sizes <= MAXC).all()
            offs = hv + np.cumsum(sizes) - sizes  # the exclusive scan over all ranks behind the header
            stream = b""
            for rank, ((lo, hi), r) in enumerate(zip(shards, ranks)):
                size = int(sizes[lo:hi].sum()) + (hv if rank == 0 else 0)
                d_whole = _aligned_u8(canary(64 + size + 64))
                d_rng = d_whole[64:64 + size]  # the rank's exactly-sized range
                r["loc"] = torch.full((r["nf"],), -1, dtype=torch.int64, device=dev)
                d_st = torch.zeros(1, dtype=torch.int32, device=dev)
                sm.place_fragments_device(r["d_comp"], r["comp_off"], r["comp_len"], _i64(offs[lo:hi]), d_rng, total,
                                          rank == 0, d_local_off=r["loc"], d_status=d_st)
                torch.cuda.synchronize()
                assert int(d_st.item()) == 0
                got = d_whole.cpu().numpy()
                assert np.array_equal(got[:64], canary(64)) and np.array_equal(got[64 + size:], canary(128 + size)[64 + size:])
                assert r["loc"].cpu().tolist() == [int(o) - (0 if rank == 0 else int(offs[lo])) for o in offs[lo:hi]]
                stream += got[64:64 + size].tobytes()
                # back: the rank's fragments decoded out of its placed range
                d_dec = _aligned_u8(canary(r["d_in"].numel() + 64))
                dec_len = torch.full((r["nf"],), 7, dtype=torch.int32, device=dev)
                status = torch.full((r["nf"],), -1, dtype=torch.int32, device=dev)
                sm.uncompress_fragments_device(d_rng, r["loc"], r["comp_len"], d_dec, r["in_off"], r["in_len"],
                                               dec_len, status)
                torch.cuda.synchronize()
                assert not status.cpu().numpy().any()
                assert torch.equal(dec_len, r["in_len"])
                want = canary(r["d_in"].numel() + 64)
                want[: r["d_in"].numel()] = data_np[lo * BLOCK: min(hi * BLOCK, total)]
                _assert_bytes(d_dec, want, "decode back, world %d rank %d" % (world, rank))
            assert oracle.uncompress(stream) == data
            assert stream == expect, (mode, total, world)


@gpu
@pytest.mark.parametrize("mode", ["reference", "fast", "dense"])
def test_oversize_block_is_marked(sm, oracle, gpu_available, mode):
    """A 65,537-byte block among good ones: d_out_len 0xffffffff and an untouched slot in both
    device compressors, the other blocks as ever; the mark poisons the stream index and placement."""
    import torch
    D = _dist()
    dev = _dev()
    raw = read_testfile("alice29.txt")
    blocks = [raw[:BLOCK], raw[70000:71000], raw[1000:1000 + BLOCK + 1], raw[5000:5300]]
    big = 2
    lens = np.array([len(b) for b in blocks], np.int64)
    total = len(blocks) * BLOCK  # the stream these would be the fragments of (table size, header, index)
    d_in = _aligned_u8(np.frombuffer(b"".join(blocks), np.uint8))
    in_off, in_len = _i64(np.cumsum(lens) - lens), _i32(lens)
    pitch = MAXC + 22  # (a multiple of 16; room for the batch call's varint header)
    comp_off = np.arange(len(blocks)) * pitch
    fill = canary(len(blocks) * pitch)
    for batch in (False, True):
        d_comp = _aligned_u8(fill)
        comp_len = torch.zeros(len(blocks), dtype=torch.int32, device=dev)
        if batch:
            sm.compress_batch_device(d_in, in_off, in_len, d_comp, _i64(comp_off), comp_len, mode=mode)
        else:
            sm.compress_fragments_device(d_in, in_off, in_len, d_comp, _i64(comp_off), comp_len, total, mode=mode)
        torch.cuda.synchronize()
        cl = comp_len.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
        out = d_comp.cpu().numpy()
        assert cl[big] == 0xFFFFFFFF
        assert np.array_equal(out[big * pitch:(big + 1) * pitch], fill[big * pitch:(big + 1) * pitch])
        for k, blk in enumerate(blocks):
            if k == big:
                continue
            room = 32 + len(blk) + len(blk) // 6 + (5 if batch else 0)  # the slot's documented room
            assert cl[k] <= room
            s = out[k * pitch: k * pitch + cl[k]].tobytes()
            assert np.array_equal(out[k * pitch + room:(k + 1) * pitch], fill[k * pitch + room:(k + 1) * pitch])
            if mode == "reference":
                assert s == (oracle.compress(blk) if batch else oracle.compress_fragment(blk, total))
            assert oracle.uncompress(s if batch else streams.varint(len(blk)) + s) == blk
        if batch:
            continue
        # the stream index is poisoned (total -1), and placement refuses the mark
        offs, tot = D.stream_offsets_device(comp_len, total, 0, 1)
        assert int(tot.item()) == -1 and offs.numel() == len(blocks)
        hv = len(streams.varint(total))
        cap = hv + int(cl[:big].sum()) + 64
        d_dst = _aligned_u8(canary(cap))
        d_st = torch.zeros(1, dtype=torch.int32, device=dev)
        sm.place_fragments_device(d_comp, _i64(comp_off), comp_len, offs, d_dst, total, 1, d_status=d_st)
        torch.cuda.synchronize()
        assert int(d_st.item()) == SM_ERR_DEVICE
        want, _, want_st = place_reference(out, comp_off, cl, offs.cpu().tolist(), total, 1, canary(cap))
        assert want_st == SM_ERR_DEVICE
        _assert_bytes(d_dst, want, "placement around the mark")
