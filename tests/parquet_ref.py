"""A plain-Python reader and writer of the Thrift compact protocol, as far as a Parquet PageHeader
needs it, and the walk over a column chunk's pages (include/snappy_mi355x_parquet.h) over a raw
codec that is passed in: libsnappy or the CPU oracle.  Written from the format rules; it shares no
code with the library.  The writer exists so that tests can build headers no Parquet writer emits.
Pinned by known answers that do not come from it (tests/test_parquet_host.py): bytes of PageHeaders
pyarrow wrote, and zlib's CRC-32."""
import collections
import zlib

SM_OK = 0
SM_BUFFER_TOO_SMALL = 2
SM_ERR_VARINT = 18
SM_ERR_ARGUMENT = 33
HEADER, TRUNCATED, SIZE_MISMATCH, CRC = 72, 73, 74, 75
DATA_PAGE, INDEX_PAGE, DICTIONARY_PAGE, DATA_PAGE_V2 = 0, 1, 2, 3
HAS_CRC, COMPRESSED = 1, 2
MAX_DEPTH = 8
FRAGMENT = 65536

T_TRUE, T_FALSE, T_BYTE, T_I16, T_I32, T_I64, T_DOUBLE, T_BINARY, T_LIST, T_SET, T_MAP, T_STRUCT = range(1, 13)


class Malformed(Exception):
    def __init__(self, status):
        super().__init__(status)
        self.status = status


# ---- the writer ------------------------------------------------------------------------------------
# A value is (type, payload): ints for the integer types, bytes for a binary and for T_BYTE / T_DOUBLE
# (1 and 8 raw bytes), None for the bools, (elemtype, [payloads]) for a list or set,
# (keytype, valuetype, [(key, value)]) for a map, and for a struct a list of (field id, value), or of
# (field id, value, True) to write the id in the long form whatever the delta.

def varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def zigzag(v):
    return varint((v << 1) ^ (v >> 63) if v >= 0 else ((-v) << 1) - 1)


def write_value(t, v, element=False):
    if t in (T_TRUE, T_FALSE):
        return bytes([t]) if element else b""
    if t in (T_BYTE, T_DOUBLE):
        assert len(v) == (1 if t == T_BYTE else 8)
        return bytes(v)
    if t in (T_I16, T_I32, T_I64):
        return zigzag(v)
    if t == T_BINARY:
        return varint(len(v)) + bytes(v)
    if t in (T_LIST, T_SET):
        et, items = v
        head = bytes([(len(items) << 4) | et]) if len(items) < 15 else bytes([0xF0 | et]) + varint(len(items))
        return head + b"".join(write_value(et, x, True) for x in items)
    if t == T_MAP:
        kt, vt, pairs = v
        if not pairs:
            return b"\x00"
        return varint(len(pairs)) + bytes([(kt << 4) | vt]) + b"".join(
            write_value(kt, k, True) + write_value(vt, x, True) for k, x in pairs)
    assert t == T_STRUCT
    return write_struct(v)


def write_struct(fields):
    out, last = bytearray(), 0
    for f in fields:
        fid, (t, v), long_form = f[0], f[1], len(f) > 2 and f[2]
        delta = fid - last
        if 0 < delta <= 15 and not long_form:
            out.append((delta << 4) | t)
        else:
            out.append(t)
            out += zigzag(fid)
        out += write_value(t, v)
        last = fid
    out.append(0)
    return bytes(out)


def i32(v):
    return (T_I32, v)


def page_header(ptype, usize, csize, crc=None, extra=(), long_ids=False, **sub):
    """The bytes of a PageHeader.  sub: num_values, encoding and, for a v2 page, def_len, rep_len,
    is_compressed, num_nulls, num_rows; sub_extra: further fields of the page type's struct; extra:
    further fields of the PageHeader itself, sorted in by id."""
    fields = [(1, i32(ptype)), (2, i32(usize)), (3, i32(csize))]
    if crc is not None:
        fields.append((4, i32(crc - (1 << 32) if crc >= 1 << 31 else crc)))
    nv, enc = sub.get("num_values", 10), sub.get("encoding", 0)
    sub_extra = list(sub.get("sub_extra", ()))
    if ptype == DATA_PAGE:
        fields.append((5, (T_STRUCT, sorted([(1, i32(nv)), (2, i32(enc)), (3, i32(3)), (4, i32(3))] + sub_extra,
                                            key=lambda f: f[0]))))
    elif ptype == DICTIONARY_PAGE:
        fields.append((7, (T_STRUCT, sorted([(1, i32(nv)), (2, i32(enc))] + sub_extra, key=lambda f: f[0]))))
    elif ptype == DATA_PAGE_V2:
        v2 = [(1, i32(nv)), (2, i32(sub.get("num_nulls", 0))), (3, i32(sub.get("num_rows", nv))), (4, i32(enc)),
              (5, i32(sub.get("def_len", 0))), (6, i32(sub.get("rep_len", 0)))]
        if "is_compressed" in sub:
            v2.append((7, (T_TRUE if sub["is_compressed"] else T_FALSE, None)))
        fields.append((8, (T_STRUCT, sorted(v2 + sub_extra, key=lambda f: f[0]))))
    fields = sorted(fields + list(extra), key=lambda f: f[0])
    if long_ids:
        fields = [(f[0], f[1], True) for f in fields]
    return write_struct(fields)


def page_v1(payload, compress, crc=False, ptype=DATA_PAGE, **kw):
    body = compress(payload)
    return page_header(ptype, len(payload), len(body), crc=zlib.crc32(body) if crc else None, **kw) + body


def page_v2(levels_rep, levels_def, values, compress, crc=False, is_compressed=None, **kw):
    sec = values if is_compressed is False or not values else compress(values)
    body = levels_rep + levels_def + sec
    if is_compressed is not None:
        kw["is_compressed"] = is_compressed
    return page_header(DATA_PAGE_V2, len(levels_rep) + len(levels_def) + len(values), len(body),
                       crc=zlib.crc32(body) if crc else None, rep_len=len(levels_rep), def_len=len(levels_def), **kw) + body


# ---- the reader ------------------------------------------------------------------------------------

class Reader:
    def __init__(self, buf, pos=0):
        self.b, self.pos = buf, pos

    def byte(self):
        if self.pos >= len(self.b):
            raise Malformed(TRUNCATED)
        self.pos += 1
        return self.b[self.pos - 1]

    def varint(self, max_bytes):
        v = 0
        for i in range(max_bytes):
            b = self.byte()
            v |= (b & 0x7F) << (7 * i)
            if b < 0x80:
                return v & ((1 << 64) - 1)
        raise Malformed(HEADER)

    def zigzag(self, max_bytes):
        v = self.varint(max_bytes)
        return (v >> 1) ^ -(v & 1)

    def i32(self):
        v = self.zigzag(5)
        if not -(1 << 31) <= v < (1 << 31):
            raise Malformed(HEADER)
        return v

    def advance(self, k):
        if k > len(self.b) - self.pos:
            raise Malformed(TRUNCATED)
        self.pos += k

    def field(self, last):
        """(id, type) of the next field, or None at the struct's end"""
        b = self.byte()
        if b == 0:
            return None
        t, delta = b & 15, b >> 4
        if not 1 <= t <= 12:
            raise Malformed(HEADER)
        return (last + delta if delta else self.zigzag(3)), t

    def skip(self, t, depth, element=False):
        """steps over a value of type t that stands at `depth`"""
        if t in (T_TRUE, T_FALSE):
            if element:
                self.advance(1)
        elif t == T_BYTE:
            self.advance(1)
        elif t in (T_I16, T_I32, T_I64):
            self.varint({T_I16: 3, T_I32: 5, T_I64: 10}[t])
        elif t == T_DOUBLE:
            self.advance(8)
        elif t == T_BINARY:
            self.advance(self.varint(5))
        elif t in (T_LIST, T_SET, T_MAP, T_STRUCT):
            if depth + 1 > MAX_DEPTH:
                raise Malformed(HEADER)
            if t == T_STRUCT:
                while True:
                    f = self.field(0)
                    if f is None:
                        return
                    self.skip(f[1], depth + 1)
            elif t == T_MAP:
                size = self.varint(5)
                if size:
                    b = self.byte()
                    kt, vt = b >> 4, b & 15
                    if not (1 <= kt <= 12 and 1 <= vt <= 12) or size > 0x7FFFFFFF:
                        raise Malformed(HEADER)
                    for _ in range(size):
                        self.skip(kt, depth + 1, True)
                        self.skip(vt, depth + 1, True)
            else:
                b = self.byte()
                size, et = b >> 4, b & 15
                if size == 15:
                    size = self.varint(5)
                if size and not 1 <= et <= 12:
                    raise Malformed(HEADER)
                if et <= T_BYTE or et == T_DOUBLE:
                    self.advance(size * (8 if et == T_DOUBLE else 1))
                    return
                if size > 0xFFFFFFFF:
                    raise Malformed(HEADER)
                for _ in range(size):
                    self.skip(et, depth + 1, True)
        else:
            raise Malformed(HEADER)


Page = collections.namedtuple("Page", "hdr_off hdr_len body_len usize levels out_off num_values type encoding flags crc output")
TABLE_KEYS = Page._fields[:11]  # smq_pages' arrays, in its order


def read_header(r):
    """The PageHeader at r.pos: a dict of what the walk reads."""
    h = dict(seen=set(), type=0, usize=0, csize=0, crc=0, num_values=[0, 0, 0], encoding=[0, 0, 0], def_len=0, rep_len=0,
             is_compressed=True)
    last = 0
    while True:
        f = r.field(last)
        if f is None:
            return h
        last, t = f
        if 1 <= last <= 4 and t == T_I32:
            h[("type", "usize", "csize", "crc")[last - 1]] = r.i32()
            h["seen"].add(last)
        elif last in (5, 7, 8) and t == T_STRUCT:
            which = (5, 7, 8).index(last)
            sub_last = 0
            while True:
                g = r.field(sub_last)
                if g is None:
                    break
                sub_last, st = g
                if sub_last == 1 and st == T_I32:
                    h["num_values"][which] = r.i32()
                elif sub_last == (4 if which == 2 else 2) and st == T_I32:
                    h["encoding"][which] = r.i32()
                elif which == 2 and sub_last == 5 and st == T_I32:
                    h["def_len"] = r.i32()
                elif which == 2 and sub_last == 6 and st == T_I32:
                    h["rep_len"] = r.i32()
                elif which == 2 and sub_last == 7 and st in (T_TRUE, T_FALSE):
                    h["is_compressed"] = st == T_TRUE
                else:
                    r.skip(st, 2)
            h["seen"].add(last)
        else:
            r.skip(t, 1)


def parse_varint32(b):
    """(value, length) of the varint32 at the start of b, or None: at most 5 bytes, the 5th below 0x10."""
    v = 0
    for i in range(min(len(b), 5)):
        v |= (b[i] & 0x7F) << (7 * i)
        if i == 4:
            return (v, 5) if b[i] < 0x10 else None
        if b[i] < 0x80:
            return v, i + 1
    return None


def walk(s):
    """(status, pages, total): the pages recorded before the walk ended, the uncompressed sizes."""
    s = bytes(s)
    n, pos, total, pages = len(s), 0, 0, []
    while pos != n:
        r = Reader(s, pos)
        try:
            h = read_header(r)
        except Malformed as e:
            return e.status, pages, total
        if not {1, 2, 3} <= h["seen"] or h["usize"] < 0 or h["csize"] < 0:
            return HEADER, pages, total
        sub = {DATA_PAGE: 0, DICTIONARY_PAGE: 1, DATA_PAGE_V2: 2}.get(h["type"], -1)
        if sub >= 0 and (5, 7, 8)[sub] not in h["seen"]:
            return HEADER, pages, total
        levels = 0
        if sub == 2:
            if h["def_len"] < 0 or h["rep_len"] < 0:
                return HEADER, pages, total
            levels = h["def_len"] + h["rep_len"]
            if levels > h["usize"] or levels > h["csize"]:
                return HEADER, pages, total
        if h["csize"] > n - r.pos:
            return TRUNCATED, pages, total
        flags = HAS_CRC if 4 in h["seen"] else 0
        if sub >= 0:
            sec_len, want = h["csize"] - levels, h["usize"] - levels
            if sub == 2 and not h["is_compressed"]:
                if sec_len != want:
                    return SIZE_MISMATCH, pages, total
            elif sec_len == 0:
                if want:
                    return SIZE_MISMATCH, pages, total
            else:
                at = r.pos + levels
                parsed = parse_varint32(s[at:at + min(sec_len, 5)])
                if parsed is None:
                    return SM_ERR_VARINT, pages, total
                if parsed[0] != want:
                    return SIZE_MISMATCH, pages, total
                flags |= COMPRESSED
        pages.append(Page(pos, r.pos - pos, h["csize"], h["usize"], levels, total, h["num_values"][sub] if sub >= 0 else 0,
                          h["type"], h["encoding"][sub] if sub >= 0 else 0, flags, h["crc"] & 0xFFFFFFFF if 4 in h["seen"] else 0,
                          sub >= 0))
        if sub >= 0:
            total += h["usize"]
        pos = r.pos + h["csize"]
    return SM_OK, pages, total


def table(pages):
    """The page table as lists, keyed as smq_pages' arrays."""
    return {k: [getattr(p, k) for p in pages] for k in TABLE_KEYS}


def oracle_status(oracle):
    """section -> (status, bytes) by the CPU oracle"""
    return oracle.uncompress_status


def libsnappy_status(libsnappy):
    """section -> (0, bytes) or (1, None) by libsnappy, which has no status codes of this project's"""
    def run(payload):
        out = libsnappy.uncompress(payload)
        return (0, out) if out is not None else (1, None)
    return run


Model = collections.namedtuple("Model", "status length slots pieces page_status pages")


def model(s, cap, decode_status, verify_crc=True):
    """What the batched decode gives for chunk s with cap bytes of room: the status, the length, the
    slots it takes, per page its output bytes (None for a failing one, b"" for one stepped over) and
    its status, and the pages.  A compressed section decodes with capacity equal to `want`."""
    s = bytes(s)
    st, pages, total = walk(s)
    if st:
        return Model(st, total, 0, [], [], pages)
    if total > cap:
        return Model(SM_BUFFER_TOO_SMALL, total, 0, [], [], pages)
    out, codes = [], []
    for p in pages:
        body = s[p.hdr_off + p.hdr_len:p.hdr_off + p.hdr_len + p.body_len]
        code, got = 0, b""
        if p.output:
            if p.flags & COMPRESSED:
                code, values = decode_status(body[p.levels:])
                if code == 0 and len(values) != p.usize - p.levels:
                    code, values = 1, None
                got = body[:p.levels] + values if code == 0 else None
            else:
                got = body
            if verify_crc and p.flags & HAS_CRC and zlib.crc32(body) != p.crc:
                code, got = CRC, None
        out.append(got)
        codes.append(code)
    first = next((c for c in codes if c), 0)
    return Model(first, total, len(pages), out, codes, pages)


def decode(s, decode_status, verify_crc=True):
    m = model(s, 1 << 62, decode_status, verify_crc)
    if m.status:
        raise ValueError("status %d" % m.status)
    return b"".join(m.pieces)


def plan(chunks, caps, max_pages):
    """smq_chunks_plan's results: (rc, first, out_len, status, total_pages, total_fragments)."""
    first, out_len, status, frags = [0], [], [], 0
    for s, cap in zip(chunks, caps):
        st, pages, total = walk(s)
        if st == 0 and total > cap:
            st = SM_BUFFER_TOO_SMALL
        first.append(first[-1] + (len(pages) if st == 0 else 0))
        if st == 0:
            frags += sum(-(-(p.usize - p.levels) // FRAGMENT) for p in pages if p.flags & COMPRESSED)
        out_len.append(total)
        status.append(st)
    if first[-1] > max_pages:
        return SM_BUFFER_TOO_SMALL, first, [0] * len(chunks), [SM_ERR_ARGUMENT] * len(chunks), first[-1], frags
    return 0, first, out_len, status, first[-1], frags


# ---- synthetic chunks: every header shape and every rejection, at its smallest ----------------------

def payload(k, n):
    """n bytes of mildly compressible content, different for every k"""
    return bytes((i * (k + 3) + (i >> 3) * 7 + k) & 0xFF if i % 11 else 32 for i in range(n))


STATS_300 = (5, (T_STRUCT, [(1, (T_BINARY, bytes(range(256)) + bytes(44))), (3, (T_I64, 12345678901234)),
                            (5, (T_BINARY, b"max"))]))  # a Statistics struct with a 300-byte binary
UNKNOWN_EVERY_TYPE = [  # field ids no PageHeader has, one of every wire type
    (20, (T_TRUE, None)), (21, (T_FALSE, None)), (22, (T_BYTE, b"\x7f")), (23, (T_I16, -300)), (24, (T_I32, 1 << 30)),
    (25, (T_I64, -(1 << 62))), (26, (T_DOUBLE, bytes(8))), (27, (T_BINARY, b"some bytes")),
    (28, (T_LIST, (T_I32, list(range(20))))), (29, (T_SET, (T_BINARY, [b"a", b"bc"]))),
    (30, (T_MAP, (T_BINARY, T_I32, [(b"k1", 1), (b"k2", -2)]))), (31, (T_MAP, (T_I32, T_I32, []))),
    (32, (T_STRUCT, [(1, (T_LIST, (T_STRUCT, [[(1, i32(5))], [(2, (T_BINARY, b"x"))]])))])),  # struct > list > struct
    (33, (T_LIST, (T_TRUE, [None, None, None]))), (34, (T_LIST, (T_DOUBLE, [bytes(8)] * 3))),
    (300, (T_I32, 7)),  # (a delta above 15: the long form)
]


def nested(depth):
    """an unknown field whose containers reach `depth` (the PageHeader is depth 1)"""
    v = (T_I32, 1)
    for _ in range(depth - 1):
        v = (T_STRUCT, [(1, v)])
    return (40, v)


def shape_cases(compress):
    """(name, chunk): well-formed chunks of header shapes pyarrow never writes; 100 to 300 payload bytes a page"""
    P = payload
    two = page_v1(P(1, 130), compress, crc=True, ptype=DICTIONARY_PAGE) + page_v1(P(2, 290), compress, crc=True)
    return [
        ("long-form field ids", page_v1(P(3, 100), compress, crc=True, long_ids=True) + page_v1(P(4, 200), compress, long_ids=True)),
        ("unknown fields of every type", page_v1(P(5, 150), compress, crc=True, extra=UNKNOWN_EVERY_TYPE,
                                                 sub_extra=UNKNOWN_EVERY_TYPE) + page_v1(P(6, 101), compress)),
        ("statistics of 300 bytes", page_v1(P(7, 300), compress, crc=True, sub_extra=[STATS_300]) +
         page_v2(b"", b"\x03\x04", P(8, 120), compress, crc=True, sub_extra=[(8, STATS_300[1])])),
        ("nesting depth 8", page_v1(P(9, 111), compress, extra=[nested(8)])),
        ("v2 not compressed", page_v2(b"\x01\x02\x03", b"\x04\x05", P(10, 170), compress, crc=True, is_compressed=False) +
         page_v2(b"", b"", P(11, 100), compress, is_compressed=False)),
        ("v2 with an empty values section", page_v2(b"\x09" * 7, b"\x08" * 120, b"", compress, crc=True) +
         page_v2(b"\x01", b"\x02" * 99, P(12, 100), compress, crc=True, is_compressed=True)),
        ("an index page between data pages", page_v1(P(13, 140), compress, crc=True) +
         page_header(INDEX_PAGE, 500, 37, crc=123) + bytes(range(37)) + page_header(9, 0, 0) + page_v1(P(14, 260), compress, crc=True)),
        ("the empty chunk", b""),
        ("two pages", two),
    ]


def rejection_cases(compress):
    """(name, chunk): one good page, then a page that ends the walk"""
    P = payload
    good = page_v1(P(20, 120), compress, crc=True)
    body = compress(P(21, 100))
    return [
        ("nesting depth 9", good + page_v1(P(21, 100), compress, extra=[nested(9)])),
        ("unknown type nibble", good + b"\x1d\x00" + page_v1(P(21, 100), compress)),
        ("unknown element type", good + write_struct([(1, i32(0)), (2, i32(0)), (3, i32(0))])[:-1] + b"\x19\x2d\x00"),
        ("field 3 missing", good + write_struct([(1, i32(1)), (2, i32(5))])),
        ("field 2 not an i32", good + write_struct([(1, i32(1)), (2, (T_I64, 5)), (3, i32(0))])),
        ("negative size", good + page_header(INDEX_PAGE, -1, 0)),
        ("negative compressed size", good + page_header(INDEX_PAGE, 0, -1)),
        ("data page header missing", good + page_header(INDEX_PAGE, 100, len(body)).replace(b"\x15\x02", b"\x15\x00", 1) + body),
        ("levels above the size", good + page_header(DATA_PAGE_V2, 10, 12, def_len=6, rep_len=5) + bytes(12)),
        ("negative level length", good + page_header(DATA_PAGE_V2, 10, 12, def_len=-1, rep_len=0) + bytes(12)),
        ("i32 varint of 6 bytes", good + b"\x15\x00\x15\x80\x80\x80\x80\x80\x01\x15\x00\x00"),
        ("i32 above 32 bits", good + b"\x15\x00\x15\xfe\xff\xff\xff\x3f\x15\x00\x00"),
        ("section varint differs from want", good + page_header(DATA_PAGE, 101, len(body)) + body),
        ("section varint does not parse", good + page_header(DATA_PAGE, 100, 3) + b"\x80\x80\x80"),
        ("empty section, bytes wanted", good + page_header(DATA_PAGE, 1, 0)),
        ("stored section of another size", good + page_header(DATA_PAGE_V2, 10, 9, def_len=2, is_compressed=False) + bytes(9)),
        ("body cut", good + page_header(DATA_PAGE, 100, len(body)) + body[:-1]),
        ("binary runs past the end", good + write_struct([(1, i32(0)), (2, i32(0)), (3, i32(0)), (9, (T_BINARY, bytes(50)))])[:-20]),
    ]


REJECTION_STATUS = {
    "nesting depth 9": HEADER, "unknown type nibble": HEADER, "unknown element type": HEADER, "field 3 missing": HEADER,
    "field 2 not an i32": HEADER, "negative size": HEADER, "negative compressed size": HEADER, "data page header missing": HEADER,
    "levels above the size": HEADER, "negative level length": HEADER, "i32 varint of 6 bytes": HEADER,
    "i32 above 32 bits": HEADER, "section varint differs from want": SIZE_MISMATCH, "section varint does not parse": SM_ERR_VARINT,
    "empty section, bytes wanted": SIZE_MISMATCH, "stored section of another size": SIZE_MISMATCH, "body cut": TRUNCATED,
    "binary runs past the end": TRUNCATED,
}
