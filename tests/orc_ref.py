"""A plain-Python writer, walker and reader of ORC's compression chunks
(include/snappy_mi355x_orc.h) over a raw codec that is passed in: the CPU oracle, libsnappy, or the
library's own sm.compress for the encoder's byte-exact check.  Written from the format rules; it
shares no code with the library.  Pinned by known answers that do not come from it
(tests/test_orc_host.py): the ORC specification's two example headers."""
import collections

HEADER = 3
MAX_BLOCK_SIZE = 0x7FFFFF
FRAGMENT = 65536

SM_OK = 0
SM_BUFFER_TOO_SMALL = 2
SM_ERR_VARINT = 18
SM_ERR_COPY_OFFSET = 19
SM_ERR_ARGUMENT = 33
TRUNCATED, CHUNK_TOO_LARGE = 64, 65


def header(length, original):
    """The 3-byte little-endian header of a chunk of `length` payload bytes."""
    assert 0 <= length <= MAX_BLOCK_SIZE
    return ((length << 1) | (1 if original else 0)).to_bytes(3, "little")


def stored(data):
    return header(len(data), True) + data


def compressed(payload):
    return header(len(payload), False) + payload


def varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def parse_varint(b):
    """(value, length) of the varint32 at the start of b, or None: at most 5 bytes, the 5th below 0x10."""
    v = 0
    for i in range(min(len(b), 5)):
        v |= (b[i] & 0x7F) << (7 * i)
        if i == 4:
            return (v, 5) if b[i] < 0x10 else None
        if b[i] < 0x80:
            return v, i + 1
    return None


def max_length(n, block_size):
    return n + HEADER * -(-n // block_size)


def pieces(data, block_size):
    return [data[o:o + block_size] for o in range(0, len(data), block_size)]


def encode(data, block_size, compress):
    """The encoder rule: pieces of block_size bytes; a piece whose raw stream is shorter than it is a
    compressed chunk, any other a stored one; the empty input is the empty stream."""
    assert 1 <= block_size <= MAX_BLOCK_SIZE
    out = bytearray()
    for piece in pieces(data, block_size):
        raw = compress(piece)
        out += compressed(raw) if len(raw) < len(piece) else stored(piece)
    return bytes(out)


Chunk = collections.namedtuple("Chunk", "pay_off pay_len ulen original out")


def walk(s, block_size):
    """(status, chunks, total): the chunks recorded before the walk ended, the declared lengths."""
    if not 1 <= block_size <= MAX_BLOCK_SIZE:
        return SM_ERR_ARGUMENT, [], 0
    n, pos, total, chunks = len(s), 0, 0, []
    while pos != n:
        if n - pos < HEADER:
            return TRUNCATED, chunks, total
        H = int.from_bytes(s[pos:pos + 3], "little")
        L, original = H >> 1, H & 1
        if L > n - pos - HEADER:
            return TRUNCATED, chunks, total
        if original:
            d = L
        else:
            parsed = parse_varint(s[pos + HEADER:pos + HEADER + min(L, 5)])
            if parsed is None:
                return SM_ERR_VARINT, chunks, total
            d = parsed[0]
        if d > block_size:
            return CHUNK_TOO_LARGE, chunks, total
        chunks.append(Chunk(pos + HEADER, L, d, original, total))
        total += d
        pos += HEADER + L
    return SM_OK, chunks, total


Model = collections.namedtuple("Model", "status length slots pieces chunk_status")


def oracle_status(oracle):
    """payload -> (status, bytes) by the CPU oracle"""
    return oracle.uncompress_status


def libsnappy_status(libsnappy):
    """payload -> (0, bytes) or (1, None) by libsnappy, which has no status codes of this project's"""
    def run(payload):
        out = libsnappy.uncompress(payload)
        return (0, out) if out is not None else (1, None)
    return run


def model(s, block_size, cap, decode_status):
    """What the batched decode gives for stream s with cap bytes of room: the status, the length, the
    slots it takes, per chunk its bytes (None for a failing one) and its status.  A compressed
    chunk decodes with capacity equal to its declared length."""
    st, chunks, total = walk(s, block_size)
    if st:
        return Model(st, total, 0, [], [])
    if total > cap:
        return Model(SM_BUFFER_TOO_SMALL, total, 0, [], [])
    out, codes = [], []
    for c in chunks:
        payload = s[c.pay_off:c.pay_off + c.pay_len]
        code, got = (0, payload) if c.original else decode_status(payload)
        out.append(got if code == 0 else None)
        codes.append(code)
    first = next((c for c in codes if c), 0)
    return Model(first, total, len(chunks), out, codes)


def decode(s, block_size, decode_status):
    m = model(s, block_size, 1 << 62, decode_status)
    if m.status:
        raise ValueError("status %d" % m.status)
    return b"".join(m.pieces)


def plan(streams, block_size, caps, max_chunks):
    """smo_streams_plan's results: (rc, first, out_len, status, total_chunks, total_fragments)."""
    first, out_len, status, frags = [0], [], [], 0
    for s, cap in zip(streams, caps):
        st, chunks, total = walk(s, block_size)
        if st == 0 and total > cap:
            st = SM_BUFFER_TOO_SMALL
        first.append(first[-1] + (len(chunks) if st == 0 else 0))
        if st == 0:
            frags += sum(-(-c.ulen // FRAGMENT) for c in chunks if not c.original)
        out_len.append(total)
        status.append(st)
    if first[-1] > max_chunks:
        return SM_BUFFER_TOO_SMALL, first, [0] * len(streams), [SM_ERR_ARGUMENT] * len(streams), first[-1], frags
    return 0, first, out_len, status, first[-1], frags


def postscript(file_bytes):
    """(PostScript length, compression block size) of an ORC file: its last byte is the PostScript's
    length, the PostScript a protobuf message whose field 3 (a varint) is the block size.  Only the
    varint (wire type 0) and length-delimited (2) fields an ORC PostScript has are stepped over."""
    ps_len = file_bytes[-1]
    ps = file_bytes[len(file_bytes) - 1 - ps_len:len(file_bytes) - 1]
    pos, block_size = 0, None

    def number(pos):
        v = shift = 0
        while True:
            b = ps[pos]
            v |= (b & 0x7F) << shift
            shift += 7
            pos += 1
            if b < 0x80:
                return v, pos

    while pos < len(ps):
        key, pos = number(pos)
        value, pos = number(pos)
        assert key & 7 in (0, 2), key
        if key & 7 == 2:
            pos += value
        elif key >> 3 == 3:
            block_size = value
    return ps_len, block_size


def file_streams(file_bytes):
    """The bytes between the "ORC" magic and the PostScript: every stream of the file (data, index,
    stripe footers, metadata, file footer) is a whole number of chunks, so they walk as one sequence."""
    assert file_bytes[:3] == b"ORC"
    return file_bytes[3:len(file_bytes) - 1 - file_bytes[-1]]


ABC = bytes([0x03, 0x08, 0x61, 0x62, 0x63])  # compress("abc"): varint 3, a literal of 3, "abc"
CASE_BLOCK = 1000  # the structural cases' compression block size


def lit(data):
    """A raw stream of one literal (at most 60 bytes)."""
    assert 0 < len(data) <= 60
    return varint(len(data)) + bytes([(len(data) - 1) << 2]) + data


def structural_cases():
    """(name, stream, status, nchunks, total) at block size CASE_BLOCK: every walk status at the
    smallest stream that shows it.  The expected values are written out here, not computed."""
    c_abc, s_abc = compressed(ABC), stored(b"abc")
    return [
        ("empty stream", b"", 0, 0, 0),
        ("one stray byte", b"\x07", TRUNCATED, 0, 0),
        ("two stray bytes", b"\x07\x00", TRUNCATED, 0, 0),
        ("abc stored", s_abc, 0, 1, 3),
        ("abc compressed", c_abc, 0, 1, 3),
        ("stored payload one byte short", s_abc[:-1], TRUNCATED, 0, 0),
        ("compressed payload one byte short", c_abc[:-1], TRUNCATED, 0, 0),
        ("header alone, L 3", header(3, True), TRUNCATED, 0, 0),
        ("L 0 stored", header(0, True), 0, 1, 0),
        ("L 0 compressed", header(0, False), SM_ERR_VARINT, 0, 0),
        ("L 0 stored between two", s_abc + header(0, True) + c_abc, 0, 3, 6),
        ("L 0x7fffff", header(0x7FFFFF, True) + b"abc", TRUNCATED, 0, 0),
        ("second chunk cut at 1", c_abc + s_abc[:1], TRUNCATED, 1, 3),
        ("second chunk cut at 2", c_abc + s_abc[:2], TRUNCATED, 1, 3),
        ("second chunk's payload cut", s_abc + c_abc[:7], TRUNCATED, 1, 3),
        ("varint of 1 byte", compressed(b"\x7f"), 0, 1, 0x7F),
        ("varint of 2 bytes", compressed(b"\xe8\x07"), 0, 1, 1000),
        ("varint unterminated", compressed(b"\x80\x80"), SM_ERR_VARINT, 0, 0),
        ("varint of 5 bytes overflows", compressed(b"\x80\x80\x80\x80\x10"), SM_ERR_VARINT, 0, 0),
        ("varint of 6 bytes", compressed(b"\x80\x80\x80\x80\x80\x01"), SM_ERR_VARINT, 0, 0),
        ("varint of 5 bytes, too large", compressed(b"\xff\xff\xff\xff\x07"), CHUNK_TOO_LARGE, 0, 0),
        ("varint unterminated behind a chunk", s_abc + compressed(b"\xff"), SM_ERR_VARINT, 1, 3),
        ("stored, d == block_size", stored(b"x" * 1000), 0, 1, 1000),
        ("stored, d == block_size + 1", stored(b"x" * 1001), CHUNK_TOO_LARGE, 0, 0),
        ("compressed, d == block_size", compressed(b"\xe8\x07"), 0, 1, 1000),
        ("compressed, d == block_size + 1", compressed(b"\xe9\x07"), CHUNK_TOO_LARGE, 0, 0),
        ("too large behind a chunk", c_abc + compressed(b"\xe9\x07"), CHUNK_TOO_LARGE, 1, 3),
    ]
