"""A plain-Python writer, walker and reader of the two block containers of
include/snappy_mi355x_blocks.h (Hadoop's BlockCompressorStream and snappy-java's SnappyOutputStream)
over the CPU oracle's raw codec.  Written from the format rules; it shares no code with the library.
Pinned by known answers that do not come from it (tests/test_blocks_host.py)."""
import collections
import struct

HADOOP, XERIAL = "hadoop", "xerial"
FORMATS = (HADOOP, XERIAL)
BLOCK = 65536
MAGIC = bytes([0x82, 0x53, 0x4E, 0x41, 0x50, 0x50, 0x59, 0x00])
HEADER = MAGIC + struct.pack(">II", 1, 1)
MAGIC_WORD = 0x82534E41
LIMIT = 0x7FFFFFFF

SM_OK = 0
SM_BUFFER_TOO_SMALL = 2
SM_ERR_VARINT = 18
SM_ERR_COPY_OFFSET = 19
SM_ERR_ARGUMENT = 33
NO_HEADER, BAD_HEADER, TRUNCATED, CHUNK_TOO_LARGE, BLOCK_LENGTH = 56, 57, 58, 59, 60


def be(v):
    return struct.pack(">I", v)


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


def chunk(payload):
    return be(len(payload)) + payload


def max_compressed_length(n):
    return 32 + n + n // 6


def max_length(n, fmt):
    pieces = [min(BLOCK, n - o) for o in range(0, n, BLOCK)]
    body = sum(max_compressed_length(p) + (8 if fmt == HADOOP else 4) for p in pieces)
    if fmt == XERIAL:
        return 16 + body
    return body if n else 4


def encode(data, fmt, compress):
    """The encoder rule: 64 KiB pieces, one chunk each holding compress(piece); in HADOOP every piece
    is a block of its own; the empty input is one empty block, or the header alone."""
    out = bytearray(HEADER if fmt == XERIAL else b"")
    for o in range(0, len(data), BLOCK):
        piece = data[o:o + BLOCK]
        if fmt == HADOOP:
            out += be(len(piece))
        out += chunk(compress(piece))
    if fmt == HADOOP and not data:
        out += be(0)
    return bytes(out)


Chunk = collections.namedtuple("Chunk", "pay_off pay_len ulen out")


def _header_status(s, pos, first):
    """0 for a good header at pos, else the status."""
    have = s[pos:pos + 16]
    if first:
        if not have or have[:8] != MAGIC[:len(have[:8])]:
            return NO_HEADER
    if len(have) < 16:
        return TRUNCATED
    if have[:8] != MAGIC:
        return NO_HEADER if first else BAD_HEADER
    return BAD_HEADER if struct.unpack(">I", have[8:12])[0] == 0 else 0


def walk(s, fmt):
    """(status, chunks, total): the chunks recorded before the walk ended, the declared lengths."""
    n, pos, total, chunks = len(s), 0, 0, []

    def a_chunk(pos, total):
        """(status, d, next pos) of the chunk whose length field is at pos"""
        L = struct.unpack(">I", s[pos:pos + 4])[0]
        if L > n - pos - 4:
            return TRUNCATED, 0, pos
        parsed = parse_varint(s[pos + 4:pos + 4 + min(L, 5)])
        if parsed is None:
            return SM_ERR_VARINT, 0, pos
        d = parsed[0]
        if d > LIMIT:
            return CHUNK_TOO_LARGE, 0, pos
        chunks.append(Chunk(pos + 4, L, d, total))
        return 0, d, pos + 4 + L

    if fmt == XERIAL:
        st = _header_status(s, 0, True)
        if st:
            return st, chunks, total
        pos = 16
        while pos != n:
            if n - pos < 4:
                return TRUNCATED, chunks, total
            if struct.unpack(">I", s[pos:pos + 4])[0] == MAGIC_WORD:
                st = _header_status(s, pos, False)
                if st:
                    return st, chunks, total
                pos += 16
                continue
            st, d, pos = a_chunk(pos, total)
            if st:
                return st, chunks, total
            total += d
        return 0, chunks, total
    while pos != n:
        if n - pos < 4:
            return TRUNCATED, chunks, total
        U = struct.unpack(">I", s[pos:pos + 4])[0]
        pos += 4
        if U > LIMIT:
            return CHUNK_TOO_LARGE, chunks, total
        got = 0
        while got < U:
            if n - pos < 4:
                return TRUNCATED, chunks, total
            st, d, pos = a_chunk(pos, total)
            if st:
                return st, chunks, total
            total += d
            if got + d > U:
                return BLOCK_LENGTH, chunks, total
            got += d
    return 0, chunks, total


Model = collections.namedtuple("Model", "status length slots pieces chunk_status")


def model(s, fmt, cap, oracle):
    """What the batched decode gives for stream s with cap bytes of room: the status, the length, the
    slots it takes, per chunk its decoded bytes (None for a failing one) and its status."""
    st, chunks, total = walk(s, fmt)
    if st:
        return Model(st, total, 0, [], [])
    if total > cap:
        return Model(SM_BUFFER_TOO_SMALL, total, 0, [], [])
    pieces, codes = [], []
    for c in chunks:
        code, out = oracle.uncompress_status(s[c.pay_off:c.pay_off + c.pay_len])
        pieces.append(out if code == 0 else None)
        codes.append(code)
    first = next((c for c in codes if c), 0)
    return Model(first, total, len(chunks), pieces, codes)


def decode(s, fmt, oracle):
    m = model(s, fmt, 1 << 62, oracle)
    if m.status:
        raise ValueError("status %d" % m.status)
    return b"".join(m.pieces)


def plan(streams, fmt, caps, max_chunks):
    """smb_streams_plan's results: (rc, first, out_len, status, total_chunks, total_fragments)."""
    first, out_len, status, frags = [0], [], [], 0
    for s, cap in zip(streams, caps):
        st, chunks, total = walk(s, fmt)
        if st == 0 and total > cap:
            st = SM_BUFFER_TOO_SMALL
        first.append(first[-1] + (len(chunks) if st == 0 else 0))
        if st == 0:
            frags += sum(-(-c.ulen // BLOCK) for c in chunks)
        out_len.append(total)
        status.append(st)
    if first[-1] > max_chunks:
        return SM_BUFFER_TOO_SMALL, first, [0] * len(streams), [SM_ERR_ARGUMENT] * len(streams), first[-1], frags
    return 0, first, out_len, status, first[-1], frags


ABC = bytes([0x03, 0x08, 0x61, 0x62, 0x63])  # compress("abc"): varint 3, a literal of 3, "abc"


def lit(data):
    """A raw stream of one literal (at most 60 bytes)."""
    assert 0 < len(data) <= 60
    return varint(len(data)) + bytes([(len(data) - 1) << 2]) + data


def structural_cases():
    """(name, format, stream, status, nchunks, total): every walk status at the smallest stream that
    shows it.  The expected values are written out here, not computed."""
    H, X = HADOOP, XERIAL
    abc, c_abc = ABC, chunk(ABC)
    one = be(3) + c_abc  # a block of "abc"
    cases = [
        ("empty stream", H, b"", 0, 0, 0),
        ("empty block", H, be(0), 0, 0, 0),
        ("abc", H, one, 0, 1, 3),
        ("payload one byte short", H, one[:-1], TRUNCATED, 0, 0),
        ("clen 0", H, be(3) + be(0), SM_ERR_VARINT, 0, 0),
        ("clen just over the rest", H, be(3) + be(6) + abc, TRUNCATED, 0, 0),
        ("clen 0xffffffff", H, be(3) + be(0xFFFFFFFF) + abc, TRUNCATED, 0, 0),
        ("ulen 0x80000000", H, be(0x80000000) + c_abc, CHUNK_TOO_LARGE, 0, 0),
        ("ulen 0x7fffffff, no chunk", H, be(0x7FFFFFFF), TRUNCATED, 0, 0),
        ("two chunks sum to ulen", H, be(6) + c_abc + c_abc, 0, 2, 6),
        ("two chunks one byte over", H, be(5) + c_abc + c_abc, BLOCK_LENGTH, 2, 6),
        ("one chunk over", H, be(2) + c_abc, BLOCK_LENGTH, 1, 3),
        ("block short of its chunks", H, be(7) + c_abc + c_abc, TRUNCATED, 2, 6),
        ("empty block between two", H, one + be(0) + one, 0, 2, 6),
        ("empty blocks only", H, be(0) + be(0), 0, 0, 0),
        ("a chunk declaring 0 inside a block", H, be(3) + chunk(b"\x00") + c_abc, 0, 2, 3),
        ("varint of 1 byte", H, be(0x7F) + chunk(b"\x7f"), 0, 1, 0x7F),
        ("varint of 2 bytes", H, be(0x3FFF) + chunk(b"\xff\x7f"), 0, 1, 0x3FFF),
        ("varint of 3 bytes", H, be(0x1FFFFF) + chunk(b"\xff\xff\x7f"), 0, 1, 0x1FFFFF),
        ("varint of 4 bytes", H, be(0xFFFFFFF) + chunk(b"\xff\xff\xff\x7f"), 0, 1, 0xFFFFFFF),
        ("varint of 5 bytes", H, be(0x7FFFFFFF) + chunk(b"\xff\xff\xff\xff\x07"), 0, 1, 0x7FFFFFFF),
        ("varint 0x80000000", H, be(0x7FFFFFFF) + chunk(b"\x80\x80\x80\x80\x08"), CHUNK_TOO_LARGE, 0, 0),
        ("varint unterminated", H, be(3) + chunk(b"\x80\x80"), SM_ERR_VARINT, 0, 0),
        ("varint too long", H, be(3) + chunk(b"\x80\x80\x80\x80\x10"), SM_ERR_VARINT, 0, 0),
        ("varint of 6 bytes", H, be(3) + chunk(b"\x80\x80\x80\x80\x80\x01"), SM_ERR_VARINT, 0, 0),
        ("second block cut", H, one + be(3) + c_abc[:6], TRUNCATED, 1, 3),
    ]
    for cut in (1, 2, 3):
        cases.append(("ulen cut at %d" % cut, H, one[:cut], TRUNCATED, 0, 0))
        cases.append(("clen cut at %d" % cut, H, one[:4 + cut], TRUNCATED, 0, 0))
        cases.append(("second ulen cut at %d" % cut, H, one + one[:cut], TRUNCATED, 1, 3))
    cases.append(("clen missing", H, one[:4], TRUNCATED, 0, 0))
    cases += [
        ("header alone", X, HEADER, 0, 0, 0),
        ("abc", X, HEADER + c_abc, 0, 1, 3),
        ("two chunks", X, HEADER + c_abc + chunk(b"\x00"), 0, 2, 3),
        ("version 0", X, MAGIC + be(0) + be(1) + c_abc, BAD_HEADER, 0, 0),
        ("version 2, compatible version 0", X, MAGIC + be(2) + be(0) + c_abc, 0, 1, 3),
        ("repeated header", X, HEADER + c_abc + HEADER + c_abc, 0, 2, 6),
        ("repeated header at the end", X, HEADER + c_abc + HEADER, 0, 1, 3),
        ("repeated header cut short", X, HEADER + c_abc + HEADER[:15], TRUNCATED, 1, 3),
        ("repeated header cut after its word", X, HEADER + c_abc + HEADER[:4], TRUNCATED, 1, 3),
        ("repeated header, wrong second half", X, HEADER + c_abc + HEADER[:7] + b"\x01" + HEADER[8:], BAD_HEADER, 1, 3),
        ("repeated header, version 0", X, HEADER + c_abc + MAGIC + be(0) + be(1), BAD_HEADER, 1, 3),
        ("clen 0", X, HEADER + be(0), SM_ERR_VARINT, 0, 0),
        ("clen just over the rest", X, HEADER + be(6) + abc, TRUNCATED, 0, 0),
        ("clen 0xffffffff", X, HEADER + be(0xFFFFFFFF), TRUNCATED, 0, 0),
        ("payload one byte short", X, HEADER + c_abc[:-1], TRUNCATED, 0, 0),
        ("varint unterminated", X, HEADER + c_abc + chunk(b"\xff"), SM_ERR_VARINT, 1, 3),
        ("varint 0x80000000", X, HEADER + chunk(b"\x80\x80\x80\x80\x08"), CHUNK_TOO_LARGE, 0, 0),
        ("hadoop stream", X, one, NO_HEADER, 0, 0),
    ]
    for cut in (1, 2, 3):
        cases.append(("clen cut at %d" % cut, X, HEADER + c_abc + c_abc[:cut], TRUNCATED, 1, 3))
    for i in range(8):
        bad = bytearray(HEADER + c_abc)
        bad[i] ^= 0x20
        cases.append(("magic byte %d wrong" % i, X, bytes(bad), NO_HEADER, 0, 0))
    for n in range(16):
        cases.append(("header cut to %d" % n, X, HEADER[:n], NO_HEADER if n == 0 else TRUNCATED, 0, 0))
    cases.append(("one wrong byte alone", X, b"\x83", NO_HEADER, 0, 0))
    cases.append(("wrong byte 3 of 5", X, MAGIC[:2] + b"\x00" + MAGIC[3:5], NO_HEADER, 0, 0))
    return cases


def cases_of(fmt):
    return [c for c in structural_cases() if c[1] == fmt]
