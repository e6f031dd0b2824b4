"""The batched stream calls' per-stream model in plain Python: what one framed stream of a batch
must give, whatever its neighbours are -- the walk, then per chunk the oracle's decode and the CRC.
Built on tests/framing_ref.py; raw Snappy comes from the CPU oracle passed in.  Nothing here calls
the library under test."""
import collections

import framing_ref as R

SM_ERR_ARGUMENT = 33
BLOCK = R.BLOCK

# status: the stream's; length: d_out_len; slots: the data chunks it decodes (0 when it is not
# decoded); pieces: per slot the chunk's bytes, or None for a failing chunk; chunk_status: per slot
Result = collections.namedtuple("Result", "status length slots pieces chunk_status")


def walk_prefix(stream):
    """(data chunks before the end or the first structural error, that error or 0): R.walk, which
    gives no chunks with an error, run over the growing prefixes of whole chunks."""
    try:
        return R.walk(stream), R.SM_OK
    except R.FramingRefError as e:
        code = e.code
    # the chunks before the error: walk the longest prefix of whole chunks that is well formed
    pos, good = 0, 0
    while pos + 4 <= len(stream):
        pos += 4 + (stream[pos + 1] | stream[pos + 2] << 8 | stream[pos + 3] << 16)
        if pos > len(stream):
            break
        try:
            R.walk(stream[:pos])
        except R.FramingRefError:
            break
        good = pos
    return (R.walk(stream[:good]) if good else []), code


def model(stream, cap, oracle):
    """What stream `stream` with `cap` bytes of room gives."""
    chunks, code = walk_prefix(stream)
    length = sum(c[4] for c in chunks)
    if code:
        return Result(code, length, 0, [], [])
    if length > cap:
        return Result(R.SM_BUFFER_TOO_SMALL, length, 0, [], [])
    pieces, statuses = [], []
    for ctype, off, plen, stored, declared in chunks:
        payload = stream[off:off + plen]
        st, data = oracle.uncompress_status(payload) if ctype == 0 else (0, payload)
        if st == 0 and R.mask(R.crc32c(data)) != stored:
            st = R.CRC
        assert st or len(data) == declared
        pieces.append(None if st else bytes(data))
        statuses.append(st)
    first = next((s for s in statuses if s), R.SM_OK)
    return Result(first, length, len(chunks), pieces, statuses)


def plan(streams, caps, max_chunks):
    """smf_streams_plan's outputs for a batch: (rc, first, out_len, status, total) -- what is known
    before any byte is decoded."""
    first, out_len, status, total = [], [], [], 0
    for stream, cap in zip(streams, caps):
        chunks, code = walk_prefix(stream)
        length = sum(c[4] for c in chunks)
        if code == 0 and cap is not None and length > cap:
            code = R.SM_BUFFER_TOO_SMALL
        first.append(total)
        out_len.append(length)
        status.append(code)
        total += len(chunks) if code == 0 else 0
    first.append(total)
    if total > max_chunks:
        return R.SM_BUFFER_TOO_SMALL, first, [0] * len(streams), [SM_ERR_ARGUMENT] * len(streams), total
    return 0, first, out_len, status, total


def long_foreign_stream(n=300):
    """n one-byte 0x01 chunks with padding and a repeated identifier between them: more chunks in
    one stream than a scan tile holds.  (stream, content)"""
    parts, content = [R.IDENTIFIER], bytearray()
    for i in range(n):
        b = bytes([i % 251])
        parts.append(R.raw_chunk(b))
        content += b
        if i % 7 == 3:
            parts.append(R.chunk(0xFE, bytes(i % 5)))
        if i % 50 == 49:
            parts.append(R.IDENTIFIER)
    return b"".join(parts), bytes(content)
