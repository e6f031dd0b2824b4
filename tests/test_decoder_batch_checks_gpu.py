"""The batch decoder's checks, tag by tag, against the oracle.

The decoder settles the reference's length checks once per 64-tag batch where one uniform test
decides them, and falls back to the full per-tag checks where it does not.  These hand-built
streams put the first failing tag in lane 0, in a middle lane and in lane 63 of a batch and in
lane 0 of the next batch, for every check, pair an offset error with an overflow in both orders,
and add the valid streams at the checks' edges.  Every stream is at most two batches of tags
(under 1 KiB); all of them decode in one launch.  Status and output (so out_len) must equal the
oracle's, through the batch decoder, through the raw fragment decoder, and, as the second 64 KiB
block of a larger stream, through sm_uncompress.

A stream is a list of tags.  One-byte literals are the filler: 2 stream bytes and 1 output byte
each, so tag k of the fillers sits in lane k % 64 of batch k // 64.  With `prefix`, a 201-byte
literal (too long for a batch: the decoder copies it on its own) comes first, so that lane 0 of the
first batch can hold a copy with output behind it.
"""
import functools

import numpy as np
import pytest

import streams

gpu = pytest.mark.gpu

ERR_INVALID, ERR_OFFSET, ERR_LENGTH, ERR_LITERAL = 17, 19, 20, 21
LANES = (0, 31, 63, 64)  # tag index of the first failing tag: batch 0 lanes 0/31/63, batch 1 lane 0
PREFIX = 201
TAIL = 3  # filler tags after the failing one: later tags must not change the verdict


def lit(data):
    return streams.lit_tag(len(data)) + bytes(data)


def copy2(offset, length):
    """A copy with a two-byte offset, whatever the offset (0 included)."""
    return bytes([2 | ((length - 1) << 2)]) + int(offset).to_bytes(2, "little")


class Body:
    """Tags appended one by one; `out` is the output a decoder has made before the next tag."""

    def __init__(self, prefix):
        self.b = bytearray()
        self.out = 0
        self.tags = 0
        if prefix:
            self.b += lit(bytes((7 * k + 1) & 0xFF for k in range(PREFIX)))
            self.out = PREFIX

    def fill(self, n):
        for _ in range(n):
            self.b += lit(bytes([(self.tags * 5 + 3) & 0xFF]))
            self.out += 1
            self.tags += 1
        return self

    def tag(self, raw, produces):
        self.b += raw
        self.out += produces
        self.tags += 1
        return self


def _cases():
    """[(name, body bytes, declared length, expected status)]"""
    cases = []

    def add(name, body, decl, want):
        assert len(body.b) <= 1024 and body.tags <= 130, name
        cases.append((name, bytes(body.b), decl, want))

    for prefix in (True, False):
        for lane in LANES:
            tagname = "%s-lane%d" % ("prefix" if prefix else "plain", lane)
            # copy offset 0, and an offset one past the output produced
            for what, off in (("offset0", lambda o: 0), ("offset-beyond", lambda o: o + 1)):
                b = Body(prefix).fill(lane)
                b.tag(copy2(off(b.out), 4), 4).fill(TAIL)
                add("%s-%s" % (what, tagname), b, b.out, ERR_OFFSET)
            if prefix or lane:
                # a copy running one byte past the declared size: len <= 16 and > 16, offset < 8
                # and >= 8 (the :505 leniency cannot apply: avail_out < len <= 16)
                for ln in (10, 20):
                    for off in (3, 20):
                        b = Body(prefix).fill(lane)
                        decl = b.out + ln - 1
                        b.tag(copy2(off, ln), ln).fill(TAIL)
                        add("copy-past-size-len%d-off%d-%s" % (ln, off, tagname), b, decl, ERR_LENGTH)
                        # the same copy ending exactly at the declared size, as the last tag: valid
                        b = Body(prefix).fill(lane).tag(copy2(off, ln), ln)
                        add("copy-to-size-len%d-off%d-%s" % (ln, off, tagname), b, b.out, 0)
                # the leniency's own side: len <= 16, offset >= 8, 16 or more bytes left
                b = Body(prefix).fill(lane).tag(copy2(20, 10), 10).fill(16)
                add("copy-lenient-%s" % tagname, b, b.out, 0)
            # a literal one byte past the declared size
            b = Body(prefix).fill(lane)
            decl = b.out + 4
            b.tag(lit(b"abcde"), 5).fill(TAIL)
            add("literal-past-size-%s" % tagname, b, decl, ERR_LITERAL)
            # a literal past the input end: 10 bytes announced, 5 there
            b = Body(prefix).fill(lane)
            b.tag(lit(b"0123456789")[:6], 10)
            add("literal-past-input-%s" % tagname, b, b.out, ERR_LITERAL)

    # pairs: an offset error at tag i and an overflow at tag j, in both orders
    for i, j in ((10, 40), (40, 10), (60, 70), (70, 60), (63, 64), (64, 63)):
        for over in ("copy", "literal"):
            b = Body(True)
            decl = None
            for k in range(max(i, j) + 1 + TAIL):
                if k == i:
                    b.tag(copy2(0, 4), 4)
                elif k == j:
                    decl = b.out + 4
                    b.tag(copy2(20, 5), 5) if over == "copy" else b.tag(lit(b"abcde"), 5)
                else:
                    b.fill(1)
            want = ERR_OFFSET if i < j else (ERR_LENGTH if over == "copy" else ERR_LITERAL)
            add("pair-offset%d-%s%d" % (i, over, j), b, decl, want)

    # valid streams at the checks' edges
    for n in (1, 63, 64, 65, 128):
        b = Body(False).fill(n)
        add("exact-%d-tags" % n, b, b.out, 0)
        b = Body(True).fill(n)
        b.tag(copy2(b.out, 64), 64)  # the farthest legal offset
        add("exact-prefix-%d-tags-copy" % n, b, b.out, 0)
        b = Body(False).fill(n)
        b.b += b"\x07"  # a tag on the last input byte is never parsed (:416)
        add("tag-on-last-byte-%d" % n, b, b.out, 0)
        b = Body(True).fill(n)
        b.tag(copy2(5, 4)[:2], 4)  # the offset's high byte lies past the input: read as zero
        add("copy-trailer-crosses-end-%d" % n, b, b.out, 0)
        b = Body(True).fill(n)
        add("declares-one-more-%d" % n, b, b.out + 1, ERR_INVALID)
    return cases


@functools.lru_cache(maxsize=None)
def reference():
    """(cases, [(status, output or None)] from the oracle), computed once."""
    import oracle as O
    cases = _cases()
    return cases, [O.uncompress_status(streams.varint(decl) + body) for _, body, decl, _ in cases]


def test_cases_are_what_they_claim(oracle):
    """CPU: the oracle gives every case the status its name says, so each check is really hit."""
    cases, ref = reference()
    assert len(cases) > 120
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


@gpu
def test_second_block_of_a_large_stream(sm, oracle, gpu_available):
    """Plain cases (no prefix) behind a 64 KiB literal block: the decoder of large streams takes
    the second block as a fragment of its own, with the general form of the checks."""
    cases, _ = reference()
    first = np.random.default_rng(77).integers(0, 256, 65536, dtype=np.uint8).tobytes()
    picked = [c for c in cases if c[0] in ("exact-65-tags", "offset0-plain-lane31", "offset0-plain-lane64",
                                           "copy-past-size-len20-off20-plain-lane63", "literal-past-size-plain-lane0",
                                           "literal-past-input-plain-lane64", "copy-to-size-len10-off3-plain-lane31")]
    assert len(picked) == 7
    for name, body, decl, _ in picked:
        s = streams.varint(65536 + decl) + lit(first) + body
        st_o, out_o = oracle.uncompress_status(s)
        try:
            got = (0, sm.uncompress(s))
        except sm.SnappyError as e:
            got = (e.code, None)
        assert got == (st_o, out_o), name
