"""The framing format in plain Python: the reference the framing tests compare against.

Written from the format's rules (include/snappy_mi355x_framing.h): a bytewise table CRC-32C that
the known-answer table pins, an encoder with the fixed encoder rule, a decoder, and hand-built
streams for every structural case.  Raw Snappy comes from the CPU oracle passed in.  Nothing here
calls the library under test."""
import struct

BLOCK = 65536
IDENTIFIER = b"\xff\x06\x00\x00sNaPpY"

SM_OK = 0
SM_BUFFER_TOO_SMALL = 2
SM_ERR_VARINT = 18
NO_IDENTIFIER, BAD_IDENTIFIER, RESERVED_CHUNK, TRUNCATED, CHUNK_TOO_LARGE, CRC = 48, 49, 50, 51, 52, 53

_TABLE = []
for _b in range(256):
    _c = _b
    for _ in range(8):
        _c = (_c >> 1) ^ (0x82F63B78 if _c & 1 else 0)
    _TABLE.append(_c)


def crc32c(data):
    c = 0xFFFFFFFF
    for b in bytes(data):
        c = _TABLE[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def mask(crc):
    return ((((crc >> 15) | (crc << 17)) & 0xFFFFFFFF) + 0xA282EAD8) & 0xFFFFFFFF


# (input, crc, masked); the first five unmasked values are the RFC 3720 vectors
KNOWN_ANSWERS = [
    (b"123456789", 0xE3069283, 0xC78AB0E5),
    (bytes(32), 0x8A9136AA, 0x0FD7FFFA),
    (b"\xff" * 32, 0x62A8AB43, 0xF909B029),
    (bytes(range(32)), 0x46DD794E, 0x951F7892),
    (bytes(range(31, -1, -1)), 0x113FDB5C, 0x593B0D57),
    (b"", 0x00000000, 0xA282EAD8),
    (b"a", 0xC1D04330, 0x28E46E78),
    (bytes(65536), 0x72C0C4A4, 0x2BCBD059),
]
GOLDEN_A = bytes.fromhex("ff060000734e61507059" "01050000" "786ee428" "61")


def chunk(ctype, data, length=None):
    """One chunk; `length` overrides the length field (cut or over-long chunks)."""
    n = len(data) if length is None else length
    return bytes([ctype]) + struct.pack("<I", n)[:3] + data


def crc_field(data):
    return struct.pack("<I", mask(crc32c(data)))


def raw_chunk(data):
    return chunk(0x01, crc_field(data) + data)


def compressed_chunk(data, oracle):
    return chunk(0x00, crc_field(data) + oracle.compress(data))


def max_framed_length(n):
    return 10 + 8 * ((n + BLOCK - 1) // BLOCK) + n


def encode(data, oracle):
    """The fixed encoder rule: 64 KiB blocks, 0x00 iff the Snappy stream is strictly shorter."""
    out = [IDENTIFIER]
    for o in range(0, len(data), BLOCK):
        block = data[o:o + BLOCK]
        comp = oracle.compress(block)
        if len(comp) < len(block):
            out.append(chunk(0x00, crc_field(block) + comp))
        else:
            out.append(chunk(0x01, crc_field(block) + block))
    return b"".join(out)


class FramingRefError(Exception):
    def __init__(self, code):
        self.code = code
        super().__init__("framing status %d" % code)


def walk(stream):
    """The data chunks of a stream as (type, payload offset, payload length, stored crc, declared
    length), or FramingRefError with the first structural error."""
    pos, first, out = 0, True, []
    n = len(stream)
    if n == 0:
        raise FramingRefError(NO_IDENTIFIER)
    while pos < n:
        ctype = stream[pos]
        if first and ctype != 0xFF:
            raise FramingRefError(NO_IDENTIFIER)
        if n - pos < 4:
            raise FramingRefError(TRUNCATED)
        length = stream[pos + 1] | stream[pos + 2] << 8 | stream[pos + 3] << 16
        rem = n - pos - 4
        data = stream[pos + 4:pos + 4 + length]
        if ctype == 0xFF:
            if length != 6:
                raise FramingRefError(BAD_IDENTIFIER)
            if rem < 6:
                raise FramingRefError(TRUNCATED)
            if data != b"sNaPpY":
                raise FramingRefError(BAD_IDENTIFIER)
            first = False
        elif ctype >= 0x80:
            if rem < length:
                raise FramingRefError(TRUNCATED)
        elif ctype >= 2:
            raise FramingRefError(RESERVED_CHUNK)
        else:
            if length < 4:
                raise FramingRefError(TRUNCATED)
            if ctype == 1 and length > BLOCK + 4:
                raise FramingRefError(CHUNK_TOO_LARGE)
            if rem < length:
                raise FramingRefError(TRUNCATED)
            stored = struct.unpack("<I", data[:4])[0]
            if ctype == 1:
                declared = length - 4
            else:
                declared = _varint(data[4:])
                if declared > BLOCK:
                    raise FramingRefError(CHUNK_TOO_LARGE)
            out.append((ctype, pos + 8, length - 4, stored, declared))
        pos += 4 + length
    return out


def _varint(b):
    v = 0
    for i in range(min(5, len(b))):
        c = b[i]
        if i < 4:
            v |= (c & 0x7F) << (7 * i)
            if c < 0x80:
                return v
        elif c < 0x10:
            return v | (c << 28)
    raise FramingRefError(SM_ERR_VARINT)


def decode(stream, oracle):
    """The stream's bytes; FramingRefError with the first failing chunk's status (structure, the
    oracle's raw status, or CRC)."""
    out = []
    for ctype, off, plen, stored, declared in walk(stream):
        payload = stream[off:off + plen]
        if ctype == 0:
            st, data = oracle.uncompress_status(payload)
            if st:
                raise FramingRefError(st)
        else:
            data = payload
        if mask(crc32c(data)) != stored:
            raise FramingRefError(CRC)
        out.append(data)
    return b"".join(out)


def structural_cases():
    """(name, stream, expected status, data chunks before the end or the error)."""
    a = raw_chunk(b"a")
    hello = chunk(0x00, crc_field(b"hello") + b"\x05\x10hello")  # varint 5, one literal tag
    I = IDENTIFIER
    cases = [
        ("identifier_only", I, SM_OK, 0),
        ("padding", I + chunk(0xFE, bytes(7)) + a, SM_OK, 1),
        ("skippable_0x80", I + chunk(0x80, b"xyz") + a, SM_OK, 1),
        ("skippable_0xfd", I + a + chunk(0xFD, b"xyz") + hello, SM_OK, 2),
        ("repeated_identifier", I + a + I + a, SM_OK, 2),
        ("zero_length_chunks", I + chunk(0xFE, b"") + chunk(0x80, b"") + a, SM_OK, 1),
        ("empty_data_chunks", I + chunk(0x01, crc_field(b"")) + chunk(0x00, crc_field(b"") + b"\x00"), SM_OK, 2),
        ("empty_stream", b"", NO_IDENTIFIER, 0),
        ("missing_identifier", a, NO_IDENTIFIER, 0),
        ("padding_first", chunk(0xFE, b"") + I, NO_IDENTIFIER, 0),
        ("wrong_identifier", chunk(0xFF, b"sNaPpy") + a, BAD_IDENTIFIER, 0),
        ("identifier_length_5", chunk(0xFF, b"sNaPp") + a, BAD_IDENTIFIER, 0),
        ("wrong_repeated_identifier", I + a + chunk(0xFF, b"SNaPpY"), BAD_IDENTIFIER, 1),
        ("identifier_cut", I[:7], TRUNCATED, 0),
        ("reserved_0x02", I + chunk(0x02, b"abcd"), RESERVED_CHUNK, 0),
        ("reserved_0x7f", I + a + chunk(0x7F, b""), RESERVED_CHUNK, 1),
        ("payload_cut_short", I + a + hello[:-1], TRUNCATED, 1),
        ("padding_cut_short", I + chunk(0xFE, b"abc", 4), TRUNCATED, 0),
        ("data_chunk_of_3_bytes", I + chunk(0x01, b"abc"), TRUNCATED, 0),
        ("data_chunk_of_0_bytes", I + chunk(0x00, b""), TRUNCATED, 0),
        ("uncompressed_65541", I + chunk(0x01, b"x" * (65541 + 4)), CHUNK_TOO_LARGE, 0),
        ("uncompressed_65540", I + chunk(0x01, b"x" * (65536 + 4)), SM_OK, 1),
        ("varint_65537", I + chunk(0x00, b"abcd" + b"\x81\x80\x04"), CHUNK_TOO_LARGE, 0),
        ("varint_65536", I + chunk(0x00, b"abcd" + b"\x80\x80\x04"), SM_OK, 1),
        ("varint_unterminated", I + chunk(0x00, b"abcd" + b"\x80\x80"), SM_ERR_VARINT, 0),
        ("varint_missing", I + chunk(0x00, b"abcd"), SM_ERR_VARINT, 0),
    ]
    for cut in (1, 2, 3):
        cases.append(("first_header_cut_%d" % cut, I[:cut], TRUNCATED, 0))
        cases.append(("later_header_cut_%d" % cut, I + a + a[:cut], TRUNCATED, 1))
    return cases
