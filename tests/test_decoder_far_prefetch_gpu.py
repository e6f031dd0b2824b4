"""The batch decoder's loop order at its edges, against the oracle.

A batch issues the loads of its far copy sources (those before the LDS output window), walks the
NEXT batch's tags while the loads arrive, and only then runs its own tags' pieces.
The next batch's walk is therefore made early, from the position this batch ends at, and must be
dropped or not made at all when a long literal follows, the batch is the last, a fragment ends, or
the input ring has to be refilled.  These hand-built streams (a few KiB each; one launch decodes
them all) sit on those edges:

 * window edge: a copy whose source starts before, at and after the window's first byte -- the
   window placed by a long literal (no shift yet) and by a shift -- swept byte by byte over 41
   positions around the base, so the edge is hit whatever the base's exact value;
 * mixed lanes: far copies of 17, 33 and 64 bytes (later pieces) beside window copies, literals of
   every kind and in-order copies in one batch;
 * a long-form literal (2-4 length bytes, and over 200 bytes) right after a batch;
 * a batch capped at 512 output bytes, so the next one starts inside the first walk's window;
 * the position after a batch on both sides of ring base + 256 (ring advance) and + 512 (refill);
 * a last batch that ends at N - 1 (one unparsed byte follows) and at N;
 * a 64 KiB fragment limit between two batches and inside one (sm_uncompress, two blocks);
 * a valid batch followed by a batch whose lane 0 or lane 63 fails each check: the status is that
   tag's and no output is claimed.

Status and output must equal the oracle's through the batch decoder, through the raw fragment
decoder and, as the second 64 KiB block of a larger stream, through sm_uncompress.
"""
import functools

import numpy as np
import pytest

import streams
from test_decoder_batch_checks_gpu import ERR_LENGTH, ERR_LITERAL, ERR_OFFSET, Body, copy2, lit

gpu = pytest.mark.gpu

WIN, KEEP, BATCH_OUT = 2560, 480, 512  # the decoder's window, what a shift keeps, a batch's output cap
SWEEP = 20                             # source positions on each side of the expected window base


def raw_lit(k, data):
    """A literal with k length bytes, whatever its length (k = 0: the short form, <= 60 bytes)."""
    n = len(data) - 1
    if k == 0:
        assert n < 60
        return bytes([n << 2]) + bytes(data)
    return bytes([(59 + k) << 2]) + n.to_bytes(k, "little") + bytes(data)


class S:
    """A stream body built tag by tag: `out` bytes made, `pos` = stream position after the last tag
    (a two-byte varint header in front, which every case here has)."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.b = bytearray()
        self.out = 0

    @property
    def pos(self):
        return 2 + len(self.b)

    def data(self, n):
        return self.rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    def lit(self, n, k=None):
        d = self.data(n)
        self.b += lit(d) if k is None else raw_lit(k, d)
        self.out += n
        return self

    def copy(self, offset, length):
        assert 1 <= offset <= self.out and 1 <= length <= 64
        self.b += copy2(offset, length)
        self.out += length
        return self

    def fill60(self, batches):
        """Batches of five 60-byte literals: 305 stream bytes and 300 output bytes each (the fifth
        tag starts at window byte 244, the sixth would start at 305)."""
        for _ in range(5 * batches):
            self.lit(60)
        return self

    def lits_to(self, target):
        """Literals so that the stream position becomes exactly `target`."""
        while target - self.pos > 61:
            self.lit(60 if target - self.pos - 61 >= 2 else 30)
        n = target - self.pos - 1
        assert 1 <= n <= 60
        return self.lit(n)


def shifted(seed):
    """A long literal, then eight batches of 60-byte literals: the window has shifted once, at
    output 2,400 (2,400 - 0 + 300 + 32 > 2,560), to base (2,400 - 480) & ~15 = 1,920; 2,700 bytes
    are out."""
    s = S(seed).lit(300).fill60(8)
    assert s.out == 2700
    return s, (2400 - KEEP) & ~15


def placed(seed):
    """A 1,000-byte literal alone: it restarts the window at (1,000 - 480) & ~15 = 512."""
    return S(seed).lit(1000), (1000 - KEEP) & ~15


def _cases():
    """[(name, body bytes, declared length, expected status)]"""
    cases = []

    def add(name, s, decl=None, want=0):
        body = bytes(s.b)
        assert len(body) < 8000, name
        decl = s.out if decl is None else decl
        assert 128 <= decl < 16384, name  # (a two-byte header: S.pos relies on it)
        cases.append((name, body, decl, want))

    # window edge, before a shift (the base a long literal left) and after one
    for where, start in (("placed", placed), ("shifted", shifted)):
        for ln in (5, 20):
            for d in range(-SWEEP, SWEEP + 1):
                s, base = start(1000 + d)
                s.lit(1).lit(2).lit(1)
                s.copy(s.out - (base + d), ln).lit(3).copy(40, 12).lit(1)
                add("edge-%s-len%d-%+d" % (where, ln, d), s)

    # mixed lanes: far copies with later pieces beside everything else a batch can hold
    for far_len in (17, 33, 64):
        s, base = shifted(2000 + far_len)
        s.lit(5).copy(s.out - 100, far_len).copy(100, 10).lit(30).copy(s.out - 700, 16).copy(300, 40)
        s.lit(100)                       # 65..200 bytes: the whole wave copies it
        s.copy(3, 10).copy(1, 20)        # offset < 16: in stream order
        s.copy(s.out - 1000, far_len).copy(far_len, far_len)  # a far copy, and a copy of its output
        s.copy(s.out - (base - 8), 64)   # far, running into the window
        s.lit(60).lit(1)
        add("mixed-far%d" % far_len, s)

    # a long-form literal right after a batch (an early walk must be dropped), tags after it
    for k, n in ((2, 10), (3, 150), (4, 50), (1, 150), (1, 201), (2, 250), (2, 1000), (3, 300), (4, 2000)):
        for far in (False, True):
            s = shifted(3000 + n)[0] if far else S(3000 + n).lit(300)
            for _ in range(40):
                s.lit(1)
            s.copy(s.out - 20 if far else 100, 33)
            s.lit(n, k)
            s.lit(2).copy(n // 2 + 1, 20).copy(s.out - 50, 40).lit(7)
            add("big-%dbytes-len%d-%s" % (k, n, "far" if far else "near"), s)

    # a batch capped at 512 output bytes: 30 copies of 64 bytes in one walk
    for far in (False, True):
        for ln in (64, 37):
            s = shifted(4000 + ln)[0] if far else S(4000 + ln).lit(300)
            for i in range(30):
                s.copy(s.out - 30 - i if far else 200 + i, ln)
            s.lit(9).copy(20, 20)
            add("capped-%s-len%d" % ("far" if far else "near", ln), s)

    # the position after a batch around ring base + 256 and + 512 (the ring's base is 0 at first)
    for e1 in (250, 255, 256, 257, 300):
        for e2 in (511, 512, 513):
            s = S(5000 + e1).lits_to(e1)
            assert s.pos == e1
            s.lits_to(e2)
            s.fill60(1).copy(s.out - 10, 40).lit(33)
            add("ring-%d-%d" % (e1, e2), s)
    for e1 in (255, 256, 257):  # and again one slot later, far copies in the batches
        s, _ = shifted(5100 + e1)
        w = (s.pos & ~255) + 256
        s.copy(s.out - 5, 20).lits_to(w + e1 - 256)
        s.copy(s.out - 9, 20).lits_to(w + e1).copy(s.out - 3, 64).lit(20)
        add("ring-late-%d" % e1, s)

    # the last batch ends at N - 1 (a byte that is never parsed follows), and at N
    for far in (False, True):
        for extra in (b"", b"\x07", b"\xfc"):
            for ntags in (3, 64, 70):
                s = shifted(6000 + ntags)[0] if far else S(6000 + ntags).lit(300)
                for i in range(ntags):
                    s.copy(s.out - 40 - i, 5) if far and i % 3 == 0 else s.lit(1)
                s.b += extra
                add("last-%s-%dtags-extra%s" % ("far" if far else "near", ntags, extra.hex()), s)

    # first error in stream order: a valid batch, then a batch whose lane 0 / lane 63 fails
    for lane in (64, 127):
        def body():
            return Body(True).fill(lane)
        b = body()
        add("err-offset0-%d" % lane, b.tag(copy2(0, 4), 4).fill(3), b.out, ERR_OFFSET)
        b = body()
        add("err-offset-beyond-%d" % lane, b.tag(copy2(b.out + 1, 4), 4).fill(3), b.out, ERR_OFFSET)
        b = body()
        decl = b.out + 19
        add("err-copy-past-size-%d" % lane, b.tag(copy2(20, 20), 20).fill(3), decl, ERR_LENGTH)
        b = body()
        decl = b.out + 4
        add("err-literal-past-size-%d" % lane, b.tag(lit(b"abcde"), 5).fill(3), decl, ERR_LITERAL)
        b = body()
        add("err-literal-past-input-%d" % lane, b.tag(lit(b"0123456789")[:6], 10), b.out, ERR_LITERAL)
    return cases


@functools.lru_cache(maxsize=None)
def reference():
    """(cases, [(status, output or None)] from the oracle), computed once."""
    import oracle as O
    cases = _cases()
    return cases, [O.uncompress_status(streams.varint(decl) + body) for _, body, decl, _ in cases]


def test_cases_are_what_they_claim(oracle):
    """CPU: every case has the status its name says and the length it declares."""
    cases, ref = reference()
    assert len(cases) > 200
    for (name, body, decl, want), (st, out) in zip(cases, ref):
        assert st == want, (name, st, want)
        assert st != 0 or len(out) == decl, name


@gpu
def test_batch_decoder_matches_oracle(sm, oracle, gpu_available):
    cases, ref = reference()
    outs, status = sm.uncompress_batch([streams.varint(decl) + body for _, body, decl, _ in cases])
    for (name, _, _, _), (st_o, out_o), st, out in zip(cases, ref, status, outs):
        assert (int(st), out) == (st_o, out_o), name


@gpu
def test_fragment_decoder_matches_oracle(sm, oracle, gpu_available):
    """The same bodies, without their headers, as fragments of declared lengths."""
    import torch
    from test_fragments_device import _aligned_u8, _dev, _i32, _i64, canary
    cases, ref = reference()
    n = len(cases)
    in_len = np.array([len(c[1]) for c in cases], np.int64)
    decl = np.array([c[2] for c in cases], np.int64)
    in_off, out_off = np.cumsum(in_len) - in_len, np.cumsum(decl) - decl
    inp = np.concatenate([np.frombuffer(b"".join(c[1] for c in cases), np.uint8), np.zeros(256, np.uint8)])
    fill = canary(int(decl.sum()) + 256)
    d_out = _aligned_u8(fill)
    d_out_len = torch.full((n,), 7, dtype=torch.int32, device=_dev())
    d_st = torch.full((n,), -1, dtype=torch.int32, device=_dev())
    sm.uncompress_fragments_device(_aligned_u8(inp), _i64(in_off), _i32(in_len), d_out, _i64(out_off), _i32(decl),
                                   d_out_len, d_st)
    torch.cuda.synchronize()
    st_g, len_g, got = d_st.cpu().numpy(), d_out_len.cpu().numpy(), d_out.cpu().numpy()
    for k, ((name, _, _, _), (st_o, out_o)) in enumerate(zip(cases, ref)):
        assert (int(st_g[k]), int(len_g[k])) == (st_o, len(out_o) if st_o == 0 else 0), name
        if st_o == 0:
            assert got[out_off[k]:out_off[k] + decl[k]].tobytes() == out_o, name
    assert np.array_equal(got[int(decl.sum()):], fill[int(decl.sum()):])


def _uncompress(sm, s):
    try:
        return 0, sm.uncompress(s)
    except sm.SnappyError as e:
        return e.code, None


@gpu
def test_second_block_of_a_large_stream(sm, oracle, gpu_available):
    """One case of each kind behind a 64 KiB literal block: the decoder of large streams takes the
    second block as a fragment of its own (output limit and source floor in force)."""
    cases, _ = reference()
    first = np.random.default_rng(78).integers(0, 256, 65536, dtype=np.uint8).tobytes()
    names = ("edge-shifted-len20--1", "edge-shifted-len20-+0", "edge-placed-len5-+1", "mixed-far33",
             "big-2bytes-len10-far", "big-2bytes-len1000-near", "capped-far-len64", "ring-256-512",
             "last-far-64tags-extra07", "err-offset0-64", "err-literal-past-size-127")
    picked = [c for c in cases if c[0] in names]
    assert len(picked) == len(names)
    for name, body, decl, _ in picked:
        s = streams.varint(65536 + decl) + lit(first) + body
        assert _uncompress(sm, s) == oracle.uncompress_status(s), name


@gpu
def test_fragment_limit_between_and_inside_batches(sm, oracle, gpu_available):
    """Two 64 KiB blocks in one stream.  The first block's last tags are one-byte literals after a
    long literal: 64 of them (a full batch ends exactly at the limit: it falls between two batches)
    or 20 (the limit falls inside the batch whose walk also holds the second block's first tags)."""
    rng = np.random.default_rng(79)
    for k in (64, 20, 1, 63):
        body = bytearray(lit(rng.integers(0, 256, 65536 - k, dtype=np.uint8).tobytes()))
        for i in range(k):
            body += lit(bytes([i]))
        second = S(7000 + k)
        for i in range(100):
            second.lit(1)
        second.copy(50, 30).lit(70).copy(120, 64).fill60(9).copy(2600, 33).lit(5)
        s = streams.varint(65536 + second.out) + bytes(body) + bytes(second.b)
        want = oracle.uncompress_status(s)
        assert want[0] == 0
        assert _uncompress(sm, s) == want, k
