"""A plain-Python reference of the Kafka log segment (record batches of magic 2, uncompressed or
Snappy), written from Kafka's protocol guide ("Record Batch"), snappy-java's SnappyOutputStream
framing and the status order of include/snappy_mi355x_kafka.h: a batch writer, a walker, a
snappy-java stream writer and reader with a configurable chunk size, a rewriter in both directions, a
decode plan and a bitwise CRC-32C.  It shares no code with the library.  Payloads come from the
`compress` / `uncompress` the caller hands in (pyarrow's libsnappy, or the oracle).
tests/test_kafka_host.py pins it by known answers that do not come from it."""
import collections
import struct

SM_OK = 0
SM_BUFFER_TOO_SMALL = 2
SM_ERR_ARGUMENT = 33
SM_ERR_VARINT = 18
SMB_NO_HEADER, SMB_BAD_HEADER, SMB_TRUNCATED, SMB_CHUNK_TOO_LARGE = 56, 57, 58, 59
TRUNCATED, MAGIC, LENGTH, CODEC, TOO_LARGE, CRC = range(104, 110)
HEADER = 61
XERIAL_MAGIC = bytes.fromhex("82534e4150505900")
XERIAL_HEADER = XERIAL_MAGIC + struct.pack(">II", 1, 1)
MAX_DECLARED = 0x7FFFFFFF - 49
STORED, XERIAL, RAW = 0, 1, 2

Batch = collections.namedtuple("Batch", "pos length codec kind declared status chunks fragments")
Walk = collections.namedtuple("Walk", "status batches valid")
Plan = collections.namedtuple("Plan", "status out_len batches chunks zero_chunks x_fragments r_fragments")


def crc32c(data, crc=0):
    """CRC-32C (Castagnoli, reflected polynomial 0x82F63B78), bit by bit."""
    crc ^= 0xFFFFFFFF
    for b in bytes(data):
        crc ^= b
        for _ in range(8):
            crc = (crc >> 1) ^ (0x82F63B78 if crc & 1 else 0)
    return crc ^ 0xFFFFFFFF


_TABLE = []


def crc32c_fast(data):
    """The same function by a byte table (the fixtures are a few hundred KB); pinned against crc32c."""
    if not _TABLE:
        for i in range(256):
            c = i
            for _ in range(8):
                c = (c >> 1) ^ (0x82F63B78 if c & 1 else 0)
            _TABLE.append(c)
    crc = 0xFFFFFFFF
    for b in bytes(data):
        crc = (crc >> 8) ^ _TABLE[(crc ^ b) & 0xFF]
    return crc ^ 0xFFFFFFFF


# ---- the batch ---------------------------------------------------------------------------------------

def tail_fields(last_offset_delta=0, base_timestamp=0, max_timestamp=0, producer_id=-1, producer_epoch=-1, base_sequence=-1,
                records_count=0):
    """The 38 bytes from lastOffsetDelta to recordsCount."""
    return struct.pack(">iqqqhii", last_offset_delta, base_timestamp, max_timestamp, producer_id, producer_epoch, base_sequence,
                       records_count)


def write_batch(payload, base_offset=0, epoch=0, attributes=0, tail=None, magic=2, crc=None):
    """One batch around `payload` as it stands (the codec bits of `attributes` say what it is)."""
    tail = tail_fields() if tail is None else bytes(tail)
    assert len(tail) == 38
    body = struct.pack(">H", attributes) + tail + bytes(payload)
    c = crc32c_fast(body) if crc is None else crc
    return struct.pack(">qiiBI", base_offset, 49 + len(payload), epoch, magic, c) + body


# ---- snappy-java's stream ------------------------------------------------------------------------------

def write_xerial(data, compress, chunk=32768, repeat_header=False):
    out = [XERIAL_HEADER]
    for k, o in enumerate(range(0, len(data), chunk)):
        if repeat_header and k:
            out.append(XERIAL_HEADER)
        c = compress(data[o:o + chunk])
        out.append(struct.pack(">I", len(c)) + c)
    return b"".join(out)


def _varint(buf):
    """(value, status) of a raw stream's varint32 over buf's first 5 bytes."""
    v = 0
    for i, b in enumerate(buf[:5]):
        if i == 4:
            return (v | (b << 28), SM_OK) if b < 0x10 else (0, SM_ERR_VARINT)
        v |= (b & 0x7F) << (7 * i)
        if b < 0x80:
            return v, SM_OK
    return 0, SM_ERR_VARINT


def walk_xerial(buf):
    """(status, [(payload offset, payload length, declared)], total) of a snappy-java stream."""
    n = len(buf)
    if n == 0 or buf[:8] != XERIAL_MAGIC[:min(n, 8)]:
        return SMB_NO_HEADER, [], 0
    if n < 16:
        return SMB_TRUNCATED, [], 0
    if struct.unpack_from(">I", buf, 8)[0] == 0:
        return SMB_BAD_HEADER, [], 0
    pos, chunks, total = 16, [], 0
    while pos != n:
        if n - pos < 4:
            return SMB_TRUNCATED, chunks, total
        (length,) = struct.unpack_from(">I", buf, pos)
        if length == 0x82534E41:
            if n - pos < 16:
                return SMB_TRUNCATED, chunks, total
            if buf[pos + 4:pos + 8] != XERIAL_MAGIC[4:] or struct.unpack_from(">I", buf, pos + 8)[0] == 0:
                return SMB_BAD_HEADER, chunks, total
            pos += 16
            continue
        if length > n - pos - 4:
            return SMB_TRUNCATED, chunks, total
        d, st = _varint(buf[pos + 4:pos + 4 + length])
        if st:
            return st, chunks, total
        if d > 0x7FFFFFFF:
            return SMB_CHUNK_TOO_LARGE, chunks, total
        chunks.append((pos + 4, length, d))
        total += d
        pos += 4 + length
    return SM_OK, chunks, total


def read_xerial(buf, uncompress):
    st, chunks, _ = walk_xerial(buf)
    assert st == SM_OK, st
    return b"".join(uncompress(buf[o:o + n]) for o, n, _ in chunks)


# ---- the walk and the heads ---------------------------------------------------------------------------

def _frags(d):
    return (d + 65535) // 65536


def head(seg, pos, length, codec):
    payload = seg[pos + HEADER:pos + 12 + length]
    if codec == 0 or not payload:
        return Batch(pos, length, codec, STORED, len(payload) if codec == 0 else 0, SM_OK, 0, 0)
    if payload[:8] == XERIAL_MAGIC:
        st, chunks, total = walk_xerial(payload)
        if st == SM_OK and total > MAX_DECLARED:
            st = TOO_LARGE
        if st:
            return Batch(pos, length, codec, XERIAL, 0, st, 0, 0)
        return Batch(pos, length, codec, XERIAL, total, SM_OK, len(chunks), sum(_frags(d) for _, _, d in chunks))
    d, st = _varint(payload)
    if st == SM_OK and d > MAX_DECLARED:
        st = TOO_LARGE
    return Batch(pos, length, codec, RAW, 0 if st else d, st, 0, 0 if st else _frags(d))


def walk(seg):
    """Walk(status, [Batch], valid_length): the walk's status alone; the heads stand in the batches."""
    seg = bytes(seg)
    n, pos, batches = len(seg), 0, []
    while pos != n:
        left = n - pos
        if left < 17:
            return Walk(TRUNCATED, batches, pos)
        if seg[16 + pos] != 2:
            return Walk(MAGIC, batches, pos)
        (length,) = struct.unpack_from(">i", seg, pos + 8)
        if length < 49:
            return Walk(LENGTH, batches, pos)
        if 12 + length > left:
            return Walk(TRUNCATED, batches, pos)
        codec = seg[pos + 22] & 7
        if codec not in (0, 2):
            return Walk(CODEC, batches, pos)
        batches.append(head(seg, pos, length, codec))
        pos += 12 + length
    return Walk(SM_OK, batches, pos)


def index_status(w):
    """smk_index's summary: (status, total_length)."""
    total, first = 0, SM_OK
    for b in w.batches:
        if b.status:
            first = b.status
            break
        total += HEADER + b.declared
    return (w.status or first), total


def plan(seg, cap=None):
    """What smk_segments_plan says of one segment."""
    w = walk(seg)
    st, total = index_status(w)
    if st == SM_OK and cap is not None and total > cap:
        st = SM_BUFFER_TOO_SMALL
    zero = sum(b.chunks for b in w.batches if b.status == SM_OK and b.kind == XERIAL and b.declared == 0)
    live = w.batches if st == SM_OK else []
    return Plan(st, total, len(w.batches), sum(b.chunks for b in live), zero,
                sum(b.fragments for b in live if b.kind == XERIAL), sum(b.fragments for b in live if b.kind == RAW))


def plan_totals(plans):
    """(batches, chunks, fragments) of a call over these segments, as smk_segments_plan sums them."""
    chunks = max(sum(p.chunks for p in plans), sum(p.zero_chunks for p in plans))
    return (sum(p.batches for p in plans), chunks,
            max(sum(p.x_fragments for p in plans), sum(p.r_fragments for p in plans)))


# ---- the rewriters -------------------------------------------------------------------------------------

def records_of(seg, b, uncompress):
    payload = seg[b.pos + HEADER:b.pos + 12 + b.length]
    if b.kind == STORED:
        return payload if b.codec == 0 else b""
    if b.kind == XERIAL:
        return read_xerial(payload, uncompress)
    return uncompress(payload)


def _rewrite(seg, b, payload, codec):
    attributes = (struct.unpack_from(">H", seg, b.pos + 21)[0] & ~7) | codec
    body = struct.pack(">H", attributes) + seg[b.pos + 23:b.pos + HEADER] + payload
    return seg[b.pos:b.pos + 8] + struct.pack(">i", 49 + len(payload)) + seg[b.pos + 12:b.pos + 17] + \
        struct.pack(">I", crc32c_fast(body)) + body


def uncompress_segment(seg, uncompress):
    """The segment with every batch rewritten uncompressed (a well-formed segment of valid payloads)."""
    seg = bytes(seg)
    w = walk(seg)
    assert w.status == SM_OK and not any(b.status for b in w.batches)
    return b"".join(_rewrite(seg, b, records_of(seg, b, uncompress), 0) for b in w.batches)


def compress_segment(seg, compress, chunk=65536):
    """The segment with every uncompressed batch rewritten as a snappy-java batch of `chunk`-byte
    pieces; a batch without records becomes its header alone; compressed batches pass through."""
    seg = bytes(seg)
    w = walk(seg)
    assert w.status == SM_OK
    out = []
    for b in w.batches:
        if b.codec != 0:
            out.append(seg[b.pos:b.pos + 12 + b.length])
            continue
        payload = seg[b.pos + HEADER:b.pos + 12 + b.length]
        out.append(_rewrite(seg, b, write_xerial(payload, compress, chunk) if payload else b"", 2))
    return b"".join(out)


def max_segment_length(n, nbatches):
    return n + n // 6 + 36 * (n // 65536) + 52 * nbatches


def stage_length(n):
    if n == 0:
        return 0
    full, rest = divmod(n, 65536)
    bound = 16 + full * (4 + 32 + 65536 + 65536 // 6) + ((4 + 32 + rest + rest // 6) if rest else 0)
    return (bound + 15) // 16 * 16
