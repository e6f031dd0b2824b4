"""The ranged decode of indexed raw streams (include/snappy_mi355x_multi_range.h) in plain Python:
test helper of test_multi_range_host.py and test_multi_range_gpu.py.  The stream-level rule, the
touched span, the entry check, the placement and the verdicts, restated from the header -- nothing
here calls the library under test -- and pinned by known answers worked out by hand
(test_multi_range_host.py::test_model_known_answers)."""
import multi_ref as R

BLOCK = 65536
SM_OK = 0
SM_BUFFER_TOO_SMALL = 2
SM_ERR_ARGUMENT = 33
OUT_LEN_ERROR = 0xFFF00000


def range_fragment_count(lo, length):
    if length == 0:
        return 0
    return (lo + length - 1) // BLOCK - lo // BLOCK + 1


def stream_level(streams, first, nentries, s, lo, length, in_len=None):
    """(status, D, hv, e0, count) of range (s, lo, length): what is decided before any fragment byte
    is read.  in_len: the lengths passed to the call (default: the streams' own)."""
    bad = (SM_ERR_ARGUMENT, 0, 0, 0, 0)
    if length == 0:
        return (SM_OK, 0, 0, 0, 0)
    if s >= len(streams):
        return bad
    n = len(streams[s]) if in_len is None else in_len[s]
    if n >= OUT_LEN_ERROR:
        return bad
    h = R.parse_varint(streams[s][:n])
    if h is None:
        return bad
    D, hv = h
    e0, e1 = int(first[s]), int(first[s + 1])
    if e0 > e1 or e1 > nentries:
        return bad
    if e1 - e0 != R.frag_count(D):
        return bad
    if lo + length > D:
        return bad
    return (SM_OK, D, hv, e0, e1 - e0)


def touched(lo, length):
    """(first fragment, fragments) of a non-empty range."""
    return lo >> 16, ((lo + length - 1) >> 16) - (lo >> 16) + 1


def entry_check(entries, f, hv, n):
    """Fragment f's bytes (lo, hi) in a stream of n bytes by its entries, or None."""
    lo = int(entries[f])
    hi = int(entries[f + 1]) if f + 1 < len(entries) else n
    if f == 0 and lo != hv:
        return None
    if not (hv <= lo < hi <= n):
        return None
    return lo, hi


def fragment_length(D, f, count):
    return BLOCK if f + 1 < count else D - BLOCK * (count - 1)


def fragment_place(D, f, count, lo, length):
    """("direct", output offset) for a whole 64 KiB inside the range; else ("edge", src, n, dst):
    bytes [src, src + n) of the decoded fragment go to output offset dst."""
    a = BLOCK * f
    b = a + fragment_length(D, f, count)
    if a >= lo and b <= lo + length and b - a == BLOCK:
        return ("direct", a - lo)
    s, e = max(a, lo), min(b, lo + length)
    return ("edge", s - a, e - s, s - lo)


def plan(streams, first, pos, nentries, ranges, bound=None, in_len=None):
    """smm_range_plan: (return code, first[], count[], status[], total)."""
    rows, total = [], 0
    for s, lo, length in ranges:
        st, D, hv, e0, count = stream_level(streams, first, nentries, s, lo, length, in_len)
        f0, k = touched(lo, length) if st == SM_OK and length else (0, 0)
        if st == SM_OK and k:
            n = len(streams[s]) if in_len is None else in_len[s]
            entries = [int(x) for x in pos[e0:e0 + count]]
            if any(entry_check(entries, f, hv, n) is None for f in range(f0, f0 + k)):
                st = SM_ERR_ARGUMENT
        rows.append((f0, k, st))
        total += k
    stop = bound is not None and total > bound
    return (SM_BUFFER_TOO_SMALL if stop else SM_OK, [r[0] for r in rows], [r[1] for r in rows],
            [SM_ERR_ARGUMENT if stop else r[2] for r in rows], total)


def decode_model(streams, first, pos, nentries, ranges, fragment_status, datas):
    """[(status, bytes or None)] of a device call under the bound.  fragment_status(s, f, lo, hi): the
    fragment decoder's status for bytes [lo, hi) of stream s as fragment f; datas[s]: the content of
    a stream whose touched fragments all decode."""
    out = []
    for s, lo, length in ranges:
        st, D, hv, e0, count = stream_level(streams, first, nentries, s, lo, length)
        if st != SM_OK:
            out.append((st, None))
            continue
        if length == 0:
            out.append((SM_OK, b""))
            continue
        f0, k = touched(lo, length)
        entries = [int(x) for x in pos[e0:e0 + count]]
        for f in range(f0, f0 + k):  # the first failing touched fragment in stream order
            span = entry_check(entries, f, hv, len(streams[s]))
            st = SM_ERR_ARGUMENT if span is None else fragment_status(s, f, span[0], span[1])
            if st != SM_OK:
                break
        out.append((st, datas[s][lo:lo + length] if st == SM_OK else None))
    return out
