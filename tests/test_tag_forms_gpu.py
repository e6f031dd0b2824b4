"""Every tag form at every decoder walker that takes a scalar step.

The walkers read one tag through one rule (sm_format.h decode_tag) and judge it through one
function (check_tag).  The suite's random and corpus streams reach those sites often; these
hand-built streams pin each form of the format at each of them:

  literals  0 length bytes: 1, 60 bytes;  1 length byte: 61, 200, 201, 256 bytes;
            2 length bytes: 5 and 257 (non-minimal), 4096 bytes;  3 and 4 length bytes: 5 bytes
  copies    kind 1: lengths 4, 11, offsets 1, 2047;  kind 2: lengths 1, 64, offsets 1, 65535;
            kind 3: lengths 1, 64, offset 1 -- and, in the large stream only, an offset above 65536

Each form stands twice: behind three one-byte literals, where a window walk meets it among short
tags, and directly behind a 201-byte literal -- which no window walk takes -- where the scalar
step's successor meets it.  A copy's offset cannot exceed the output before it, so the small
stream holds the forms with offsets up to 2047 and the large ones hold all.

  small   about 16 KiB (two 4096-byte literals and the rest; path 4 needs 4096 bytes of output and
          a body no longer than it): the batch decoder, validate, sm_uncompress path 4 and path 0
  large   four 64 KiB blocks and a short fifth (the parallel decode starts at 256 KiB), path 4 off:
          block-structured (path 1), and with the copies that reach into an earlier block (path 2)

Every failing twin -- a copy with offset 0 or one past the output, a copy or a literal running
past the declared size, a literal running past the input, and the wrapped length 0xffffffff + 1
-- must get the oracle's status from every entry point that reports one.  A twin declares at
least 4096 bytes with a body shorter than that, so path 4's walkers see it before the fall back.
No case is skipped: a stream that does not take the path named for it fails the test, and the CPU
test checks beforehand that each is eligible for it.
"""
import functools

import numpy as np
import pytest

import streams
from test_gpu_parity import literal_path, small_path

gpu = pytest.mark.gpu

ERR_INVALID, ERR_OFFSET, ERR_LENGTH, ERR_LITERAL = 17, 19, 20, 21
LONG = 201  # a literal no window walk takes (more than 200 bytes)
FAR = 70000  # a copy offset above 65536 (kind 3 only)

LITERALS = [(1, 0), (60, 0), (61, 1), (200, 1), (201, 1), (256, 1), (5, 2), (257, 2), (4096, 2), (5, 3), (5, 4)]
COPIES = ([(1, off, ln) for ln in (4, 11) for off in (1, 2047)] + [(2, off, ln) for ln in (1, 64) for off in (1, 65535)] +
          [(3, 1, ln) for ln in (1, 64)])
FAR_COPIES = [(3, FAR, ln) for ln in (1, 64)]
PLACES = ("window", "scalar")


def lit_tag(n, nb):
    """A literal tag for n bytes with nb length bytes (0: the length in the tag byte)."""
    if nb == 0:
        assert 1 <= n <= 60
        return bytes([(n - 1) << 2])
    assert n - 1 < 256 ** nb
    return bytes([(59 + nb) << 2]) + (n - 1).to_bytes(nb, "little")


def copy_tag(kind, offset, length):
    """A copy tag of the given kind, whatever the offset (0 and beyond the output included)."""
    if kind == 1:
        assert 4 <= length <= 11 and offset < 2048
        return bytes([1 | ((length - 4) << 2) | ((offset >> 8) << 5), offset & 0xFF])
    assert 1 <= length <= 64
    return bytes([kind | ((length - 1) << 2)]) + int(offset).to_bytes(2 if kind == 2 else 4, "little")


class Body:
    """Tags appended one by one; `out` is their LZ77 meaning (decompress_all_tags! on a valid stream)."""

    def __init__(self, seed):
        self.b = bytearray()
        self.out = bytearray()
        self.rng = np.random.default_rng(seed)

    def lit(self, n, nb):
        data = self.rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        self.b += lit_tag(n, nb) + data
        self.out += data
        return self

    def copy(self, kind, offset, length):
        assert 1 <= offset <= len(self.out)
        self.b += copy_tag(kind, offset, length)
        for _ in range(length):
            self.out.append(self.out[-offset])
        return self

    def shorts(self, n):
        for _ in range(n):
            self.lit(1, 0)
        return self

    def lead(self, place):
        """What stands before a form: short tags of its window, or a literal the walk stops at."""
        return self.shorts(3) if place == "window" else self.lit(LONG, 1)

    def ballast(self):
        """4396 bytes of output from about 500 bytes of stream."""
        self.lit(300, 2)
        for _ in range(64):
            self.copy(2, 300, 64)
        return self

    def forms(self, max_offset):
        for form in LITERALS:
            for place in PLACES:
                self.lead(place).lit(*form).shorts(2)
        for kind, off, ln in COPIES:
            if off <= max_offset:
                for place in PLACES:
                    self.lead(place).copy(kind, off, ln).shorts(2)
        return self

    def stream(self, declared=None):
        return streams.varint(len(self.out) if declared is None else declared) + bytes(self.b)


def small_stream():
    b = Body(1).ballast().forms(2047)
    for _ in range(8):  # (a body shorter than its output, whatever the literals' tag bytes add)
        b.copy(2, 1, 64)
    return b.stream(), bytes(b.out)


def block(b, k, far_end):
    """64 KiB of output from an output position that is a multiple of 65536: the forms, literals up
    to the block's last byte and, as that byte, the copy of length 1 at offset 65535 -- the one
    position where it reads its own block only (far_end: behind short tags or a long literal)."""
    start = len(b.out)
    assert start % 65536 == 0
    b.forms(2047)
    tail = 3 if far_end == "window" else LONG
    while start + 65535 - len(b.out) - tail > 0:
        b.lit(min(3000, start + 65535 - len(b.out) - tail), 2)
    b.lead(far_end).copy(2, 65535, 1)
    assert len(b.out) == start + 65536 and k == start // 65536


def large_streams():
    """(block-structured stream, its output), (the same with copies into earlier blocks, output)"""
    a = Body(2)
    for k in range(4):
        block(a, k, PLACES[k % 2])
    a.forms(2047)  # (a short fifth block)
    c = Body(2)
    for k in range(2):
        block(c, k, PLACES[k % 2])
    for kind, off, ln in [(2, 65535, 64)] + FAR_COPIES:
        for place in PLACES:
            c.lead(place).copy(kind, off, ln).shorts(2)
    c.forms(65535)
    while len(c.out) < len(a.out):
        c.lit(3000, 2)
    return (a.stream(), bytes(a.out)), (c.stream(), bytes(c.out))


def twins():
    """[(name, stream, the status its construction asks for)]"""
    cases = []
    seed = [100]

    def fresh():
        seed[0] += 1
        return Body(seed[0])

    for place in PLACES:
        # offsets: the bad copy early, ballast behind it (never decoded) for the declared length
        for kind, ln in sorted({(k, n) for k, _, n in COPIES}):
            for what in ("offset0", "offset-beyond"):
                b = fresh().lit(70, 1).lead(place)
                at, out_at = len(b.b), len(b.out)
                b.copy(kind, 1, ln).shorts(2).ballast()
                bad = copy_tag(kind, 0 if what == "offset0" else out_at + 1, ln)
                s = streams.varint(len(b.out)) + bytes(b.b[:at]) + bad + bytes(b.b[at + len(bad):])
                cases.append(("%s-kind%d-len%d-%s" % (what, kind, ln, place), s, ERR_OFFSET))
        # a copy one byte past the declared size
        for kind, off, ln in COPIES:
            if off <= 2047:
                b = fresh().ballast().lead(place)
                decl = len(b.out) + ln - 1
                b.copy(kind, off, ln).shorts(2)
                cases.append(("copy-past-size-kind%d-off%d-len%d-%s" % (kind, off, ln, place), b.stream(decl), ERR_LENGTH))
        for n, nb in LITERALS:
            # a literal one byte past the declared size, and one whose last byte the input lacks
            b = fresh().ballast().lead(place)
            decl = len(b.out) + n - 1
            b.lit(n, nb).shorts(2)
            cases.append(("literal-past-size-%d-%d-%s" % (n, nb, place), b.stream(decl), ERR_LITERAL))
            # (of a one-byte literal that leaves the tag on the input's last byte, which is never
            # parsed, internal.jl:416: the output then ends short of the declared length)
            b = fresh().ballast().lead(place).lit(n, nb)
            cases.append(("literal-past-input-%d-%d-%s" % (n, nb, place), b.stream()[:-1],
                          ERR_LITERAL if n + nb > 1 else ERR_INVALID))
        # four length bytes of 0xff: 1 + 0xffffffff wraps to a literal of no bytes, which is valid
        b = fresh().ballast().lead(place)
        b.b += bytes([63 << 2, 0xFF, 0xFF, 0xFF, 0xFF])
        b.shorts(2).lit(LONG, 1)
        cases.append(("wrapped-length-%s" % place, b.stream(), 0))
    return cases


@functools.lru_cache(maxsize=None)
def reference():
    """The streams and the oracle's verdict on each, computed once."""
    import oracle as O
    small = small_stream()
    large, crossing = large_streams()
    tw = twins()
    return {"small": small, "large": large, "crossing": crossing, "twins": tw,
            "twin_ref": [O.uncompress_status(s) for _, s, _ in tw]}


def parallel_eligible(sm, comp):
    """sm_host_rules.h parallel_candidate: 256 KiB of output from a body of two index chunks."""
    size, hdr = sm.parse32(comp, 0)
    return size >= 4 * 65536 and len(comp) - hdr >= 2 * 4096


def test_streams_are_what_they_claim(sm, oracle):
    """CPU: the oracle decodes the valid streams to their LZ77 meaning, gives every twin the status
    it was built for, and each stream is eligible for the path named for it."""
    ref = reference()
    for name in ("small", "large", "crossing"):
        s, want = ref[name]
        assert oracle.uncompress(s) == want, name
        assert not literal_path(sm, s), name
    s, want = ref["small"]
    assert 4096 <= len(want) < 20000 and small_path(sm, s) and not parallel_eligible(sm, s)
    for name in ("large", "crossing"):
        s, want = ref[name]
        assert 4 * 65536 < len(want) < 4 * 65536 + 20000 and parallel_eligible(sm, s), name
    assert len(ref["twins"]) > 80
    for (name, s, want), (st, out) in zip(ref["twins"], ref["twin_ref"]):
        assert st == want, (name, st, want)
        assert small_path(sm, s) and not literal_path(sm, s) and not parallel_eligible(sm, s), name


def _device_decode(sm, comps):
    """uncompress_batch_device and validate_batch_device over comps: (statuses, outputs or None, validate's statuses)"""
    import torch
    dev = torch.device("cuda", 0)
    in_len = np.array([len(c) for c in comps], np.int64)
    cap = np.array([sm.parse32(c, 0)[0] for c in comps], np.int64)
    in_off, out_off = np.cumsum(in_len) - in_len, np.cumsum(cap) - cap
    d_in = torch.from_numpy(np.frombuffer(b"".join(comps) + b"\0" * 16, np.uint8).copy()).to(dev)
    d_in_off, d_in_len = torch.from_numpy(in_off).to(dev), torch.from_numpy(in_len.astype(np.int32)).to(dev)
    d_out = torch.zeros(int(cap.sum()) + 16, dtype=torch.uint8, device=dev)
    d_out_len = torch.zeros(len(comps), dtype=torch.int32, device=dev)
    d_st = torch.full((len(comps),), -1, dtype=torch.int32, device=dev)
    d_vst = torch.full((len(comps),), -1, dtype=torch.int32, device=dev)
    sm.uncompress_batch_device(d_in, d_in_off, d_in_len, d_out, torch.from_numpy(out_off).to(dev),
                               torch.from_numpy(cap.astype(np.int32)).to(dev), d_out_len, d_st)
    sm.validate_batch_device(d_in, d_in_off, d_in_len, d_vst)
    torch.cuda.synchronize()
    st, ln, out = d_st.cpu().numpy(), d_out_len.cpu().numpy(), d_out.cpu().numpy()
    outs = [out[o:o + n].tobytes() if s == 0 else None for o, n, s in zip(out_off, ln, st)]
    return [int(x) for x in st], outs, [int(x) for x in d_vst.cpu().numpy()]


def _single(sm, comp):
    try:
        return 0, sm.uncompress(comp)
    except sm.SnappyError as e:
        return e.code, None


@gpu
def test_small_stream_at_every_entry_point(sm, oracle, gpu_available):
    s, want = reference()["small"]
    st, outs, vst = _device_decode(sm, [s])
    assert (st, outs, vst) == ([0], [want], [0])
    try:
        for small, path in ((True, 4), (False, 0)):
            sm.set_small_decode(small)
            assert _single(sm, s) == (0, want)
            assert sm.last_uncompress_path() == path
    finally:
        sm.set_small_decode(True)


@gpu
def test_large_streams_by_fragments_and_by_origin_pointers(sm, oracle, gpu_available):
    ref = reference()
    try:
        sm.set_small_decode(False)
        for name, path in (("large", 1), ("crossing", 2)):
            s, want = ref[name]
            assert _single(sm, s) == (0, want), name
            assert sm.last_uncompress_path() == path, name
    finally:
        sm.set_small_decode(True)


@gpu
def test_failing_twins_get_the_oracles_status(sm, oracle, gpu_available):
    ref = reference()
    comps = [s for _, s, _ in ref["twins"]]
    st, outs, vst = _device_decode(sm, comps)
    for (name, _, _), (st_o, out_o), st_g, out_g, st_v in zip(ref["twins"], ref["twin_ref"], st, outs, vst):
        assert (st_g, out_g, st_v) == (st_o, out_o, st_o), name
    try:
        for small in (True, False):
            sm.set_small_decode(small)
            for (name, s, _), want in zip(ref["twins"], ref["twin_ref"]):
                assert _single(sm, s) == want, (name, small)
    finally:
        sm.set_small_decode(True)
