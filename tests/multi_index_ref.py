"""The rule of smm_index_device / smm_index_host in plain Python (test helper of
test_multi_index_host.py and test_multi_index_gpu.py): a stream's entry count, the walk over tag
sizes that finds the tag at every 64 KiB of output, the batch's scan and its overflow -- and the
hand-built streams and the staging sweep both tests run.  Nothing here calls the library under test.
"""
import numpy as np

import multi_ref as R
import streams as S

BLOCK = 65536
OUT_LEN_ERROR = 0xFFF00000  # SM_OUT_LEN_ERROR: a compressor's error mark, never a length
SM_OK = 0
SM_ERR_ARGUMENT = 33
GUARD = 0xDEADBEEF
NO_CAP = 0xFFFFFFFF


def tag_size(p, x, n):
    """(bytes in the stream, output bytes) of the tag at x: the format's tag table, the trailer's
    bytes at or past n read as zero, the literal length in 32-bit arithmetic (it wraps)."""
    c = p[x]
    at = lambda i: p[i] if i < n else 0
    kind, hi = c & 3, c >> 2
    if kind == 0:
        extra = hi - 59 if hi >= 60 else 0
        base = 1 if hi >= 60 else hi + 1
        trailer = sum(at(x + 1 + k) << (8 * k) for k in range(extra))
        length = (base + trailer) & 0xFFFFFFFF
        return 1 + extra + length, length
    if kind == 1:
        return 2, 4 + (hi & 7)
    return (3 if kind == 2 else 5), hi + 1


def count_of(p, n, cap):
    """(D, hv, count) of one stream; count 0 (and D, hv 0) when it gets no entries."""
    if n >= OUT_LEN_ERROR:
        return 0, 0, 0
    h = R.parse_varint(bytes(p[:min(n, 5)]))
    if h is None or h[0] > cap:
        return 0, 0, 0
    return h[0], h[1], R.frag_count(h[0])


def _short_tags():
    """(size, output) per tag byte whose size needs no other byte: copies and literals up to 60."""
    table = []
    for c in range(256):
        table.append(tag_size(bytes([c, 0, 0, 0, 0]), 0, 5) if (c & 3) or (c >> 2) < 60 else None)
    return table


_SHORT = _short_tags()


def walk(p, n, hv, count):
    """The positions of a stream that declares more than 64 KiB, or None."""
    x, o, f, pos = hv, 0, 0, []
    at = 0  # 65536 f
    while True:
        if x >= n:
            return None
        if o >= at:
            if o > at:
                return None
            pos.append(x)
            f += 1
            at += BLOCK
            if f == count:
                return pos
        t = _SHORT[p[x]] or tag_size(p, x, n)
        x += t[0]
        o += t[1]


def model(strs, caps, max_fragments, lens=None, guard=0):
    """(frag_first, frag_pos with `guard` sentinel entries behind max_fragments, built, status) of
    one call.  caps None: no cap; lens: lengths to pass instead of the streams' own."""
    n = len(strs)
    lens = [len(s) for s in strs] if lens is None else lens
    caps = [NO_CAP] * n if caps is None else caps
    counts = [count_of(s, l, c) for s, l, c in zip(strs, lens, caps)]
    pos = np.full(max_fragments + guard, GUARD, np.uint32)
    built = np.zeros(n, np.uint8)
    if sum(c[2] for c in counts) > max_fragments:
        return np.zeros(n + 1, np.uint32), pos, built, np.full(n, SM_ERR_ARGUMENT, np.int32)
    first = np.concatenate([[0], np.cumsum([c[2] for c in counts])]).astype(np.uint32)
    for k, (s, l, (D, hv, cnt)) in enumerate(zip(strs, lens, counts)):
        e = int(first[k])
        if D > BLOCK:
            w = walk(s, l, hv, cnt)
            pos[e:e + cnt] = w if w is not None else 0
            built[k] = w is not None
        elif cnt:
            pos[e] = hv
    return first, pos, built, np.zeros(n, np.int32)


# ---- hand-built streams ----------------------------------------------------------------------------

def lits(declared, *lengths):
    """varint(declared), then literals of these lengths (filler bytes)."""
    return S.varint(declared) + b"".join(S.lit_tag(n) + b"a" * n for n in lengths)


def hand_cases():
    """[(name, stream, cap or None, length to pass or None)]"""
    K = BLOCK
    short = [60] * 1092  # 65,520 bytes in one-byte tags
    whole = lits(2 * K + 5, K, K, 5)
    return [
        ("ends-on-65536", lits(K + 1, K, 1), None, None),
        ("short-tags-end-on-65536", lits(K + 1, *short, 16, 1), None, None),
        ("short-literal-straddles", lits(K + 5, *short, 17, 1, 3), None, None),
        ("literal-70000-crosses", lits(70010, 70000, 10), None, None),
        ("literal-65536-lands-then-more", whole, None, None),
        ("literal-crosses-two", lits(140010, 140000, 10), None, None),
        ("cut-before-last", whole[:3 + 3 + K + 100], None, None),
        ("boundary-at-end", lits(K + 1, K), None, None),
        ("stray-byte-at-boundary", lits(K + 1, K) + b"\x00", None, None),
        ("header-only", S.varint(K + 1), None, None),
        ("wrapping-literal-length", S.varint(K + 1) + b"\xfc\xff\xff\xff\xff" + b"a" * 40, None, None),
        ("declares-more-than-cap", lits(K + 1, K, 1), K, None),
        ("declares-the-cap", lits(K + 1, K, 1), K + 1, None),
        ("varint-unfinished", b"\x85\x80", None, None),
        ("varint-fifth-byte", b"\xff\xff\xff\xff\x10\x00\x00", None, None),
        ("empty", b"", None, None),
        ("error-mark", b"\x85\x80\x0c", None, OUT_LEN_ERROR),
        ("declares-0", lits(0), None, None),
        ("declares-1", lits(1, 1), None, None),
        ("declares-65536", lits(K, K), None, None),
    ]


# ---- the staging sweep -----------------------------------------------------------------------------

def sweep_stream(a, ncopies, last, last_off):
    """A leading literal of a bytes, ncopies copies (offset 1, length 64), a last copy of `last`
    bytes, a 5-byte literal: tag bytes only, nothing is expanded."""
    body = S.lit_tag(a) + b"a" * a + S.copy_tag(1, 64) * ncopies + S.copy_tag(last_off, last) + S.lit_tag(5) + b"tail."
    return S.varint(BLOCK + 5) + body


def sweep_cases(stage):
    """[(stream, the boundary tag's position P, crosses)]: for every P within 300 bytes of 1 x stage
    and 2 x stage a stream whose output reaches 65,536 exactly at the tag at P, and its twin whose
    last copy is one byte longer.  With t and u the bytes of the literal's and the last copy's tags,
    P = 3 + t + a + 3 c + u and a + 64 c + last = 65,536, so 61 c = 65,539 + t + u - last - P: the
    last copy's length (1..63, room for the twin) is searched for the residue that fits.  One
    residue needs the three-byte tag at a length the near form would take in two: that copy has
    offset 2,048 (the walk reads no offset, and these streams are never decoded)."""
    cases = []
    for j in (1, 2):
        for P in range(j * stage - 300, j * stage + 301):
            found = None
            for last_off in (1, 2048):
                for last in range(1, 64):
                    u = len(S.copy_tag(last_off, last))
                    for t in (2, 3):
                        c, rem = divmod(BLOCK + 3 + t + u - last - P, 61)
                        a = BLOCK - last - 64 * c
                        if rem == 0 and c >= 0 and a >= 1 and len(S.lit_tag(a)) == t and found is None:
                            found = (a, c, last, last_off)
            assert found, P
            a, c, last, last_off = found
            assert 3 + len(S.lit_tag(a)) + a + 3 * c + len(S.copy_tag(last_off, last)) == P
            for extra in (0, 1):
                cases.append((sweep_stream(a, c, last + extra, last_off), P, bool(extra)))
    return cases


# ---- the calls both tests make ---------------------------------------------------------------------

CPU_INDEX_LENGTHS = (65537, 131072, 150000, 196613)
_CACHE = {}


def cpu_index_cases(oracle):
    """[(stream, the oracle's own fragment positions)] at lengths around one, two and three blocks."""
    if "cpu" not in _CACHE:
        src = R.sources()
        _CACHE["cpu"] = [R.cpu_index(src[k % 3][3:3 + n], oracle) for k, n in enumerate(CPU_INDEX_LENGTHS)]
    return _CACHE["cpu"]


def exact_bound(strs, caps=None, lens=None):
    lens = [len(s) for s in strs] if lens is None else lens
    caps = [NO_CAP] * len(strs) if caps is None else caps
    return sum(count_of(s, l, c)[2] for s, l, c in zip(strs, lens, caps))


def groups(oracle):
    """{name: (streams, caps or None, lengths or None, max_fragments)}: one call each."""
    if "groups" in _CACHE:
        return _CACHE["groups"]
    g = {}
    ladder = [oracle.compress(d) for d in R.ladder_datas()]
    g["ladder"] = (ladder, None, None, exact_bound(ladder))
    cpu = [c[0] for c in cpu_index_cases(oracle)]
    g["cpu_index"] = (cpu, None, None, exact_bound(cpu) + 3)
    foreign = [R.foreign_stream(seed, target)[0] for seed, target in ((31, 140000), (32, 190000))]
    g["foreign"] = (foreign, None, None, exact_bound(foreign))
    fuzz = R.fuzz_cases(oracle)
    fs, fc = [c[0] for c in fuzz], [c[1] for c in fuzz]
    g["fuzz"] = (fs, fc, None, exact_bound(fs, fc))
    hand = hand_cases()
    hs = [h[1] for h in hand]
    hc = [NO_CAP if h[2] is None else h[2] for h in hand]
    hl = [len(h[1]) if h[3] is None else h[3] for h in hand]
    m = exact_bound(hs, hc, hl)
    g["hand"] = (hs, hc, hl, m)
    g["hand_no_cap"] = (hs, None, hl, exact_bound(hs, None, hl))
    g["hand_overflow"] = (hs, hc, hl, m - 1)
    _CACHE["groups"] = g
    return g


GUARDS = 3


def group_model(oracle, name):
    key = ("model", name)
    if key not in _CACHE:
        strs, caps, lens, m = groups(oracle)[name]
        _CACHE[key] = model(strs, caps, m, lens, GUARDS)
    return _CACHE[key]


def pack(strs, lens=None):
    """(buffer of exactly the streams' total size, offsets, lengths): the streams back to back."""
    buf = np.frombuffer(b"".join(strs), np.uint8) if strs else np.zeros(0, np.uint8)
    off = np.zeros(len(strs), np.uint64)
    own = np.array([len(s) for s in strs], np.uint64)
    if len(strs) > 1:
        off[1:] = np.cumsum(own[:-1])
    return buf, off, np.array(own if lens is None else lens, np.uint32)
