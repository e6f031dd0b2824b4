"""Ranged reads of a framed stream in plain Python: the reference of the seek-index tests.

Built on tests/framing_ref.py (R.walk, the CRC) and the CPU oracle for raw Snappy.  A range
[lo, lo + length) of the stream's content touches the data chunks of non-zero declared length
whose bytes meet it; each touched chunk is decoded whole and its CRC checked, and the first
failure in stream order is the range's status.  Nothing here calls the library under test."""
import functools

import numpy as np

import framing_ref as R

SM_OK = 0
SM_ERR_ARGUMENT = 33
BLOCK = R.BLOCK
VICTIM = 4  # the foreign stream's chunk of 16 bytes: content [4, 20)


def foreign_stream(oracle):
    """A hand-built stream of 37 content bytes: data chunks of 0, 1, 3, 0, 16, 17 and 0 bytes, both
    chunk types, with a skippable chunk, padding and a repeated identifier in between."""
    data = bytes(range(100, 137))
    parts = [data[0:0], data[0:1], data[1:4], data[4:4], data[4:20], data[20:37], data[37:37]]
    stream = (R.IDENTIFIER + R.raw_chunk(parts[0]) + R.compressed_chunk(parts[1], oracle) +
              R.chunk(0x80, b"skip me") + R.raw_chunk(parts[2]) + R.compressed_chunk(parts[3], oracle) +
              R.IDENTIFIER + R.compressed_chunk(parts[4], oracle) + R.chunk(0xFE, bytes(5)) + R.raw_chunk(parts[5]) +
              R.raw_chunk(parts[6]))
    return stream, data


def all_ranges(total):
    """Every (lo, length) inside a content of `total` bytes, the empty ranges included, and the
    ranges that end one byte past it."""
    return [(lo, n) for lo in range(total + 1) for n in range(total - lo + 2)]


def chunk_offsets(chunks):
    """The exclusive scan of the declared lengths of R.walk's chunks, the total last."""
    off = [0]
    for c in chunks:
        off.append(off[-1] + c[4])
    return off


@functools.lru_cache(maxsize=8)
def _decoded(stream, oracle):
    """Per data chunk (offset in the content, declared length, status, bytes), each decoded once."""
    out, at = [], 0
    for ctype, off, plen, stored, declared in R.walk(stream):
        payload = stream[off:off + plen]
        if ctype == 0:
            st, data = oracle.uncompress_status(payload)
        else:
            st, data = 0, payload
        if st == 0 and R.mask(R.crc32c(data)) != stored:
            st = R.CRC
        out.append((at, declared, st, data if st == 0 else b""))
        at += declared
    return out, at


def touched(offsets, lo, length):
    """Indices of the chunks a range touches, from the offsets (chunk_offsets) alone."""
    return [c for c in range(len(offsets) - 1)
            if length > 0 and offsets[c + 1] > offsets[c] and offsets[c] < lo + length and offsets[c + 1] > lo]


def plan(offsets, lo, length):
    """(first touched chunk, slots, status) as smf_range_plan reports them for a good index: the
    slots run from the first to the last touched chunk (empty chunks in between keep theirs)."""
    if length == 0:
        return 0, 0, SM_OK
    if lo + length >= 1 << 64 or lo + length > offsets[-1]:
        return 0, 0, SM_ERR_ARGUMENT
    t = touched(offsets, lo, length)
    return t[0], t[-1] - t[0] + 1, SM_OK


def read_range(stream, lo, length, oracle):
    """(status, bytes) of range [lo, lo + length) of the stream's content."""
    chunks, total = _decoded(stream, oracle)
    if length == 0:
        return SM_OK, b""
    if lo + length >= 1 << 64 or lo + length > total:
        return SM_ERR_ARGUMENT, b""
    parts = []
    for at, declared, st, data in chunks:
        if declared == 0 or at >= lo + length or at + declared <= lo:
            continue
        if st:
            return st, b""
        parts.append(data[max(lo - at, 0):lo + length - at])
    return SM_OK, b"".join(parts)


def hostile_indexes(make, index, n):
    """Damaged copies of the foreign stream's index (`make(arrays, chunk_off)` builds one; n = the
    stream's length): (name, index, chunk the damage sits in or None: every non-empty range fails)."""
    def variant(**changes):
        arrays = {k: v.copy() for k, v in index.arrays().items()}
        off = index.chunk_off.copy()
        for k, (where, value) in changes.items():
            if k == "chunk_off":
                off[where] = value
            else:
                arrays[k][where] = value
        return make(arrays, off)

    top = np.iinfo(np.uint64).max
    everywhere = slice(None)
    return [
        ("type_7", variant(type=(VICTIM, 7)), VICTIM),
        ("pay_off_near_top", variant(pay_off=(VICTIM, top - 3)), VICTIM),
        ("payload_past_the_end", variant(pay_off=(VICTIM, n - 15)), VICTIM),
        ("ulen_65537", variant(ulen=(VICTIM, 65537), pay_len=(VICTIM, 65537)), VICTIM),
        ("raw_lengths_differ", variant(pay_len=(5, 16)), 5),
        ("chunk_off_constant", variant(chunk_off=(everywhere, 9)), None),
        ("chunk_off_decreasing", variant(chunk_off=(everywhere, np.arange(40, 0, -5, dtype=np.uint64))), None),
        ("chunk_off_uint64_max", variant(chunk_off=(everywhere, top)), None),
    ]


def hostile_want(index, total_claimed, victim, lo, n):
    """The status a hostile index's range has before any byte is decoded."""
    if n == 0:
        return 0
    if lo + n > total_claimed:
        return SM_ERR_ARGUMENT
    if victim is None:
        return SM_ERR_ARGUMENT
    return SM_ERR_ARGUMENT if victim in touched(index.chunk_off.tolist(), lo, n) else 0
