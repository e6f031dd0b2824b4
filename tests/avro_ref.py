"""A plain-Python reference of the Avro object container file with the snappy codec, written from
the Avro 1.11 specification ("Object Container Files", "Binary Encoding") and the status order of
include/snappy_mi355x_avro.h: a writer, a walker, a reader, the split rule and the decode plan.  It
shares no code with the library.  Payloads come from the `compress` / `uncompress` the caller hands
in (pyarrow's libsnappy, or the oracle); checksums from zlib.crc32.  tests/test_avro_host.py pins it
by known answers that do not come from it."""
import collections
import zlib

SM_OK = 0
SM_BUFFER_TOO_SMALL = 2
SM_ERR_ARGUMENT = 33
SM_ERR_VARINT = 18
NO_HEADER, BAD_HEADER, TRUNCATED, VARLONG, CODEC, BLOCK, TOO_LARGE, SYNC, CRC = range(80, 89)
FILE, BLOCKS = "file", "blocks"
MAGIC = b"Obj\x01"
MAX_DECLARED = 0x7FFFFFFF

Block = collections.namedtuple("Block", "pay_off pay_len ulen count crc out_off")
Walk = collections.namedtuple("Walk", "status blocks total objects header_len sync")


class _Stop(Exception):
    def __init__(self, status):
        self.status = status


# ---- binary encoding --------------------------------------------------------------------------------

def encode_long(v):
    u = (v << 1) ^ (v >> 63)  # zigzag, on Python's unbounded integers
    u &= (1 << 64) - 1
    out = bytearray()
    while True:
        if u < 0x80:
            out.append(u)
            return bytes(out)
        out.append(0x80 | (u & 0x7F))
        u >>= 7


def decode_long(buf, pos):
    """(value, position behind it); _Stop(TRUNCATED) past the end, _Stop(VARLONG) for more than 64 bits."""
    u = 0
    for i in range(10):
        if pos >= len(buf):
            raise _Stop(TRUNCATED)
        b = buf[pos]
        pos += 1
        if i == 9:
            if b > 1:
                raise _Stop(VARLONG)
            u |= b << 63
            break
        u |= (b & 0x7F) << (7 * i)
        if b < 0x80:
            break
    return (u >> 1) ^ -(u & 1), pos


def encode_bytes(b):
    return encode_long(len(b)) + bytes(b)


def raw_varint(payload):
    """The declared length of a raw Snappy stream (its varint32 header), or None."""
    v = 0
    for i, b in enumerate(payload[:5]):
        if i == 4 and b >= 0x10:
            return None
        v |= (b & 0x7F) << (7 * i)
        if b < 0x80:
            return v
    return None


# ---- the writer ---------------------------------------------------------------------------------------

def header(schema, sync, meta=(), codec=b"snappy"):
    """The file header: one map block with avro.schema, avro.codec and then `meta`'s pairs."""
    pairs = [(b"avro.schema", bytes(schema)), (b"avro.codec", codec)] + [(bytes(k), bytes(v)) for k, v in meta]
    out = MAGIC + encode_long(len(pairs))
    for k, v in pairs:
        out += encode_bytes(k) + encode_bytes(v)
    return out + encode_long(0) + bytes(sync)


def header_maps(maps, sync):
    """A header whose metadata map is written as the given map blocks: (pairs, negative) each, the
    negative form carrying the count negated and the block's byte size."""
    out = MAGIC
    for pairs, negative in maps:
        body = b"".join(encode_bytes(k) + encode_bytes(v) for k, v in pairs)
        out += (encode_long(-len(pairs)) + encode_long(len(body)) if negative else encode_long(len(pairs))) + body
    return out + encode_long(0) + bytes(sync)


def libsnappy():
    """(compress, uncompress) of pyarrow's bundled libsnappy: independent of the oracle and of the
    project.  uncompress gives None for a payload libsnappy refuses."""
    import pyarrow as pa
    codec = pa.Codec("snappy")

    def compress(data):
        return codec.compress(bytes(data)).to_pybytes()

    def uncompress(payload):
        n = raw_varint(payload)
        if n is None:
            return None
        try:
            return codec.decompress(bytes(payload), decompressed_size=n).to_pybytes()
        except Exception:
            return None

    return compress, uncompress


def block(data, count, sync, compress):
    payload = compress(bytes(data))
    return (encode_long(count) + encode_long(len(payload) + 4) + payload + (zlib.crc32(bytes(data)) & 0xFFFFFFFF).to_bytes(4, "big")
            + bytes(sync))


def write_blocks(blocks, counts, sync, compress):
    return b"".join(block(d, c, sync, compress) for d, c in zip(blocks, counts))


def write(blocks, counts, schema, sync, compress, meta=()):
    return header(schema, sync, meta) + write_blocks(blocks, counts, sync, compress)


# ---- the walker ---------------------------------------------------------------------------------------

def _walk_header(buf):
    n = len(buf)
    if n == 0 or buf[:4] != MAGIC[:min(n, 4)]:
        raise _Stop(NO_HEADER)
    if n < 4:
        raise _Stop(TRUNCATED)
    pos, codec = 4, None
    while True:
        c, pos = decode_long(buf, pos)
        if c == 0:
            break
        if c < 0:
            if c == -(1 << 63):
                raise _Stop(BAD_HEADER)
            c = -c
            size, pos = decode_long(buf, pos)
            if size < 0:
                raise _Stop(BAD_HEADER)
        for _ in range(c):
            pair = []
            for _ in range(2):
                length, pos = decode_long(buf, pos)
                if length < 0:
                    raise _Stop(BAD_HEADER)
                if length > n - pos:
                    raise _Stop(TRUNCATED)
                pair.append(bytes(buf[pos:pos + length]))
                pos += length
            if pair[0] == b"avro.codec":
                codec = pair[1]
    if n - pos < 16:
        raise _Stop(TRUNCATED)
    sync = bytes(buf[pos:pos + 16])
    if codec != b"snappy":
        raise _Stop(CODEC)
    return pos + 16, sync


def walk(buf, kind=FILE, sync=None):
    """Walk(status, blocks, total, objects, header_len, sync) of a stream, by the documented order."""
    buf = bytes(buf)
    n, blocks, total, objects, header_len = len(buf), [], 0, 0, 0
    status, pos = SM_OK, 0
    try:
        if kind == FILE:
            sync = bytes(16)
            pos, sync = _walk_header(buf)
            header_len = pos
        while pos != n:
            count, pos = decode_long(buf, pos)
            if count < 0:
                raise _Stop(BLOCK)
            size, pos = decode_long(buf, pos)
            if size < 4:
                raise _Stop(BLOCK)
            rest = n - pos
            if size > rest or rest - size < 16:
                raise _Stop(TRUNCATED)
            if size - 4 > MAX_DECLARED:
                raise _Stop(TOO_LARGE)
            if buf[pos + size:pos + size + 16] != sync:
                raise _Stop(SYNC)
            d = raw_varint(buf[pos:pos + size - 4])
            if d is None:
                raise _Stop(SM_ERR_VARINT)
            if d > MAX_DECLARED:
                raise _Stop(TOO_LARGE)
            blocks.append(Block(pos, size - 4, d, count, int.from_bytes(buf[pos + size - 4:pos + size], "big"), total))
            total += d
            objects = min(objects + count, (1 << 64) - 1)
            pos += size + 16
    except _Stop as e:
        status = e.status
    return Walk(status, blocks, total, objects, header_len, bytes(sync))


# ---- one input per walk status -----------------------------------------------------------------------

def mutations(small, meta):
    """(name, stream, status), one or more per walk status: each a fixture (small_blocks.avro,
    meta_forms.avro) changed at a named byte."""
    w = walk(small)
    big = next(b for b in w.blocks if b.pay_len >= 5)
    first = w.header_len  # the first block's count

    def put(data, at, new):
        return data[:at] + new + data[at + len(new):]

    key = small.index(b"avro.codec")
    codec = key + 11  # (behind the key and the value's one-byte length)
    return [
        ("the magic's first byte", put(small, 0, b"P"), NO_HEADER),
        ("the magic's last byte", put(small, 3, b"\x02"), NO_HEADER),
        ("the last byte cut off", small[:-1], TRUNCATED),
        ("the file cut inside the header's marker", small[:first - 1], TRUNCATED),
        ("the negative map block's byte size made -1", put(meta, 5, b"\x01"), BAD_HEADER),
        ("the map count made the one that cannot be negated", put(meta, 4, b"\xff" * 9 + b"\x01"), BAD_HEADER),
        ("the first key's length made -1", put(small, 5, b"\x01"), BAD_HEADER),
        ("the first block's count made an 11-byte long", put(small, first, b"\x80" * 10 + b"\x00"), VARLONG),
        ("the first block's count with a 10th byte of 2", put(small, first, b"\xff" * 9 + b"\x02"), VARLONG),
        ("the codec's last letter", put(small, codec + 5, b"x"), CODEC),
        ("the codec key's first letter", put(small, key, b"b"), CODEC),
        ("the first block's count made -1", put(small, first, b"\x01"), BLOCK),
        ("the first block's size made 3", put(small, first + 1, b"\x06"), BLOCK),
        ("a payload's varint made 2^31", put(small, big.pay_off, bytes.fromhex("8080808008")), TOO_LARGE),
        ("a marker's first byte", put(small, big.pay_off + big.pay_len + 4, bytes([small[big.pay_off + big.pay_len + 4] ^ 1])), SYNC),
        ("a marker's last byte", put(small, big.pay_off + big.pay_len + 19, bytes([small[big.pay_off + big.pay_len + 19] ^ 0x80])), SYNC),
        ("a payload's varint made five bytes of ff", put(small, big.pay_off, b"\xff" * 5), SM_ERR_VARINT),
    ]


# ---- the reader ---------------------------------------------------------------------------------------

def read(buf, uncompress, kind=FILE, sync=None, verify_crc=True):
    """(status, bytes or None, Walk): every block decoded by `uncompress` (None for a payload it
    refuses, which this reader reports as status -1) and held against its CRC-32."""
    w = walk(buf, kind, sync)
    if w.status != SM_OK:
        return w.status, None, w
    out, status = [], SM_OK
    for b in w.blocks:
        data = uncompress(bytes(buf[b.pay_off:b.pay_off + b.pay_len]))
        if data is None or len(data) != b.ulen:
            status = status or -1
            out.append(bytes(b.ulen))
            continue
        if verify_crc and zlib.crc32(data) & 0xFFFFFFFF != b.crc:
            status = status or CRC
        out.append(data)
    return status, b"".join(out), w


def find_sync(buf, sync, start):
    """The split rule: the first position at or after `start` where the marker stands, else len(buf)."""
    at = bytes(buf).find(bytes(sync), start) if start <= len(buf) else -1
    return len(buf) if at < 0 else at


# ---- the decode plan ----------------------------------------------------------------------------------

def plan(streams, kind=FILE, syncs=None, caps=None, max_blocks=MAX_DECLARED):
    """(rc, first, out_len, status, objects, total_blocks, total_fragments) as sma_streams_plan gives them."""
    first, out_len, status, objects, total, frags = [0], [], [], [], 0, 0
    for i, s in enumerate(streams):
        w = walk(s, kind, None if syncs is None else syncs[i])
        st = w.status
        if st == SM_OK and caps is not None and w.total > caps[i]:
            st = SM_BUFFER_TOO_SMALL
        status.append(st)
        out_len.append(w.total)
        objects.append(w.objects)
        if st == SM_OK:
            total += len(w.blocks)
            frags += sum(-(-b.ulen // 65536) for b in w.blocks)
        first.append(min(total, 0xFFFFFFFF))
    if total > max_blocks:
        return SM_BUFFER_TOO_SMALL, first, [0] * len(streams), [SM_ERR_ARGUMENT] * len(streams), [0] * len(streams), total, frags
    return SM_OK, first, out_len, status, objects, total, frags
