"""A plain-Python restatement of the Parquet page encoder (include/snappy_mi355x_parquet_write.h): the
encode walk with its patch sites, the header rewrite, and the transcoder of a plain column chunk into
a compression=SNAPPY one over any `compress` callable (libsnappy, the CPU oracle, the identity).
Built on the reader of tests/parquet_ref.py; it shares no code with the library.  The rewrite here
splices byte strings where the library computes each output byte's source, so the two agree only if
both are right.

A generic Thrift compact-protocol tree (read_tree / write_tree) serves one purpose: to splice
transcoded chunks into a file that pyarrow wrote and rewrite its footer (splice_file), so that an
independent reader can judge the result."""
import struct
import zlib

import parquet_ref as R

SM_ERR_INPUT_TOO_LARGE = 16
SM_ERR_DEVICE = 32
MAX_BODY = 0x7FFFFFFF
STAGE_DUMP = 32
SITE_KEYS = ("f3_at", "f3_len", "f4_at", "f4_len", "f7_at")


# ---- the encode walk --------------------------------------------------------------------------------

def read_header(r):
    """The PageHeader at r.pos as the encode walk reads it: (fields as parquet_ref.read_header gives
    them, positions of the patch sites in the buffer, whether a patched field came twice)."""
    h = dict(seen=set(), type=0, usize=0, csize=0, crc=0, num_values=[0, 0, 0], encoding=[0, 0, 0], def_len=0, rep_len=0)
    at = dict(f3=None, f4=None, f7=None)
    repeated = False
    last = 0
    while True:
        f = r.field(last)
        if f is None:
            return h, at, repeated
        last, t = f
        if 1 <= last <= 4 and t == R.T_I32:
            start = r.pos
            h[("type", "usize", "csize", "crc")[last - 1]] = r.i32()
            if last >= 3:
                repeated |= last in h["seen"]
                at["f%d" % last] = (start, r.pos - start)
            h["seen"].add(last)
        elif last in (5, 7, 8) and t == R.T_STRUCT:
            which = (5, 7, 8).index(last)
            sub_last = 0
            while True:
                field_at = r.pos
                g = r.field(sub_last)
                if g is None:
                    break
                sub_last, st = g
                if sub_last == 1 and st == R.T_I32:
                    h["num_values"][which] = r.i32()
                elif sub_last == (4 if which == 2 else 2) and st == R.T_I32:
                    h["encoding"][which] = r.i32()
                elif which == 2 and sub_last == 5 and st == R.T_I32:
                    h["def_len"] = r.i32()
                elif which == 2 and sub_last == 6 and st == R.T_I32:
                    h["rep_len"] = r.i32()
                elif which == 2 and sub_last == 7 and st in (R.T_TRUE, R.T_FALSE):
                    repeated |= at["f7"] is not None
                    at["f7"] = field_at
                else:
                    r.skip(st, 2)
            h["seen"].add(last)
        else:
            r.skip(t, 1)


def sites_of(at, start):
    """The five words of a header's patch sites, from the header's first byte."""
    f3, f4, f7 = at["f3"], at["f4"], at["f7"]
    return (f3[0] - start, f3[1], f4[0] - start if f4 else 0, f4[1] if f4 else 0, f7 - start if f7 is not None else 0)


def walk(s):
    """(status, pages, sites, total) of a chunk in its plain form: parquet_ref.Page entries of the
    INPUT's pages (flags: HAS_CRC alone) and per page its five site words."""
    s = bytes(s)
    n, pos, total, pages, sites = len(s), 0, 0, [], []
    while pos != n:
        r = R.Reader(s, pos)
        try:
            h, at, repeated = read_header(r)
        except R.Malformed as e:
            return e.status, pages, sites, total
        if not {1, 2, 3} <= h["seen"] or h["usize"] < 0 or h["csize"] < 0 or repeated:
            return R.HEADER, pages, sites, total
        sub = {R.DATA_PAGE: 0, R.DICTIONARY_PAGE: 1, R.DATA_PAGE_V2: 2}.get(h["type"], -1)
        if sub >= 0 and (5, 7, 8)[sub] not in h["seen"]:
            return R.HEADER, pages, sites, total
        levels = 0
        if sub == 2:
            if h["def_len"] < 0 or h["rep_len"] < 0:
                return R.HEADER, pages, sites, total
            levels = h["def_len"] + h["rep_len"]
            if levels > h["usize"] or levels > h["csize"]:
                return R.HEADER, pages, sites, total
        if h["csize"] > n - r.pos:
            return R.TRUNCATED, pages, sites, total
        if sub >= 0 and h["csize"] != h["usize"]:
            return R.SIZE_MISMATCH, pages, sites, total
        has_crc = 4 in h["seen"]
        pages.append(R.Page(pos, r.pos - pos, h["csize"], h["usize"], levels, total, h["num_values"][sub] if sub >= 0 else 0,
                            h["type"], h["encoding"][sub] if sub >= 0 else 0, R.HAS_CRC if has_crc else 0,
                            h["crc"] & 0xFFFFFFFF if has_crc else 0, sub >= 0))
        sites.append(sites_of(at, pos))
        if sub >= 0:
            total += h["usize"]
        pos = r.pos + h["csize"]
    return R.SM_OK, pages, sites, total


# ---- the header rewrite -------------------------------------------------------------------------------

def as_i32(crc):
    return crc - (1 << 32) if crc >= 1 << 31 else crc


def patch(header, site, new_body_len, crc):
    """The header's bytes with its sites patched: the later site first, so that no position moves."""
    f3_at, f3_len, f4_at, f4_len, f7_at = site
    b = bytearray(header)
    if f7_at:
        b[f7_at] = (b[f7_at] & 0xF0) | R.T_TRUE
    edits = [(f3_at, f3_len, R.zigzag(new_body_len))]
    if f4_len:
        edits.append((f4_at, f4_len, R.zigzag(as_i32(crc & 0xFFFFFFFF))))
    for at, length, new in sorted(edits, reverse=True):
        b[at:at + length] = new
    return bytes(b)


def rewrite_header(buf, new_body_len, crc):
    """smqe_rewrite_header: (status, bytes or None) for the PageHeader at the start of buf."""
    r = R.Reader(bytes(buf), 0)
    try:
        h, at, repeated = read_header(r)
    except R.Malformed as e:
        return e.status, None
    if not {1, 2, 3} <= h["seen"] or h["usize"] < 0 or h["csize"] < 0 or repeated:
        return R.HEADER, None
    if new_body_len > MAX_BODY:
        return SM_ERR_INPUT_TOO_LARGE, None
    return 0, patch(bytes(buf[:r.pos]), sites_of(at, 0), new_body_len, crc)


# ---- the transcoder -------------------------------------------------------------------------------------

def transcode(s, compress):
    """(status, the compression=SNAPPY chunk or None) of the plain chunk s."""
    s = bytes(s)
    st, pages, sites, _ = walk(s)
    if st:
        return st, None
    out = bytearray()
    for p, site in zip(pages, sites):
        header = s[p.hdr_off:p.hdr_off + p.hdr_len]
        body = s[p.hdr_off + p.hdr_len:p.hdr_off + p.hdr_len + p.body_len]
        if not p.output:
            out += header + body
            continue
        new = body[:p.levels] + compress(body[p.levels:])
        if len(new) > MAX_BODY:
            return SM_ERR_INPUT_TOO_LARGE, None
        out += patch(header, site, len(new), zlib.crc32(new)) + new
    return 0, bytes(out)


def max_compressed_length(n):
    return 32 + n + n // 6


def plan(chunks, max_pages):
    """smqe_chunks_plan's results: (rc, first, status, out_bound, total_pages, stage_bytes, total_fragments)."""
    first, status, bound, stage, frags = [0], [], [], STAGE_DUMP, 0
    for s in chunks:
        st, pages, _, _ = walk(s)
        first.append(first[-1] + (len(pages) if st == 0 else 0))
        status.append(st)
        if st:
            bound.append(0)
            continue
        b = 0
        for p in pages:
            want = p.usize - p.levels
            if p.output:
                stage += (p.levels + max_compressed_length(want) + 15) // 16 * 16
                frags += -(-want // R.FRAGMENT) if want > R.FRAGMENT else 0
                b += p.hdr_len + 8 + p.levels + max_compressed_length(want)
            else:
                b += p.hdr_len + p.body_len
        bound.append(b)
    if first[-1] > max_pages:
        return R.SM_BUFFER_TOO_SMALL, first, [R.SM_ERR_ARGUMENT] * len(chunks), [0] * len(chunks), first[-1], stage, frags
    return 0, first, status, bound, first[-1], stage, frags


def plain_page_v1(payload, crc=False, ptype=R.DATA_PAGE, **kw):
    """A v1 page in its plain form (the crc, where there is one, is the plain body's, as a writer has it)."""
    return R.page_header(ptype, len(payload), len(payload), crc=zlib.crc32(payload) if crc else None, **kw) + payload


def plain_page_v2(levels_rep, levels_def, values, crc=False, is_compressed=None, **kw):
    body = levels_rep + levels_def + values
    if is_compressed is not None:
        kw["is_compressed"] = is_compressed
    return R.page_header(R.DATA_PAGE_V2, len(body), len(body), crc=zlib.crc32(body) if crc else None, rep_len=len(levels_rep),
                         def_len=len(levels_def), **kw) + body


def rejection_cases():
    """(name, chunk, status): one good plain page, then a page that ends the encode walk -- the decode
    walk's header rejections as far as they do not depend on a section, and the encoder's own."""
    P = R.payload
    good = plain_page_v1(P(20, 120), crc=True)
    body = P(21, 100)
    i32 = R.i32
    H = R.page_header
    dup3 = R.write_struct([(1, i32(0)), (2, i32(100)), (3, i32(100)), (3, i32(100), True), (5, (R.T_STRUCT, [(1, i32(1)), (2, i32(0))]))])
    dup4 = R.write_struct([(1, i32(0)), (2, i32(100)), (3, i32(100)), (4, i32(5)), (4, i32(6), True),
                           (5, (R.T_STRUCT, [(1, i32(1)), (2, i32(0))]))])
    v2 = [(1, i32(1)), (4, i32(0)), (5, i32(0)), (6, i32(0))]
    dup7 = R.write_struct([(1, i32(3)), (2, i32(100)), (3, i32(100)),
                           (8, (R.T_STRUCT, v2 + [(7, (R.T_FALSE, None)), (7, (R.T_TRUE, None), True)]))])
    two8 = R.write_struct([(1, i32(3)), (2, i32(100)), (3, i32(100)), (8, (R.T_STRUCT, v2 + [(7, (R.T_FALSE, None))])),
                           (8, (R.T_STRUCT, v2 + [(7, (R.T_FALSE, None))]), True)])
    return [
        ("nesting depth 9", good + plain_page_v1(body, extra=[R.nested(9)]), R.HEADER),
        ("unknown type nibble", good + b"\x1d\x00" + plain_page_v1(body), R.HEADER),
        ("unknown element type", good + R.write_struct([(1, i32(0)), (2, i32(0)), (3, i32(0))])[:-1] + b"\x19\x2d\x00", R.HEADER),
        ("field 3 missing", good + R.write_struct([(1, i32(1)), (2, i32(5))]), R.HEADER),
        ("field 2 not an i32", good + R.write_struct([(1, i32(1)), (2, (R.T_I64, 5)), (3, i32(0))]), R.HEADER),
        ("negative size", good + H(R.INDEX_PAGE, -1, 0), R.HEADER),
        ("negative compressed size", good + H(R.INDEX_PAGE, 0, -1), R.HEADER),
        ("data page header missing", good + H(R.INDEX_PAGE, 100, 100).replace(b"\x15\x02", b"\x15\x00", 1) + body, R.HEADER),
        ("levels above the size", good + H(R.DATA_PAGE_V2, 10, 10, def_len=6, rep_len=5) + bytes(10), R.HEADER),
        ("negative level length", good + H(R.DATA_PAGE_V2, 10, 10, def_len=-1, rep_len=0) + bytes(10), R.HEADER),
        ("i32 varint of 6 bytes", good + b"\x15\x00\x15\x80\x80\x80\x80\x80\x01\x15\x00\x00", R.HEADER),
        ("i32 above 32 bits", good + b"\x15\x00\x15\xfe\xff\xff\xff\x3f\x15\x00\x00", R.HEADER),
        ("body cut", good + H(R.DATA_PAGE, 100, 100) + body[:-1], R.TRUNCATED),
        ("binary runs past the end", good + R.write_struct([(1, i32(0)), (2, i32(0)), (3, i32(0)), (9, (R.T_BINARY, bytes(50)))])[:-20],
         R.TRUNCATED),
        ("compressed size below the size", good + H(R.DATA_PAGE, 100, 99) + body[:99], R.SIZE_MISMATCH),
        ("compressed size above the size", good + H(R.DICTIONARY_PAGE, 99, 100) + body, R.SIZE_MISMATCH),
        ("v2 sizes differ", good + H(R.DATA_PAGE_V2, 100, 98, def_len=2) + body[:98], R.SIZE_MISMATCH),
        ("field 3 twice", good + dup3 + body, R.HEADER),
        ("field 4 twice", good + dup4 + body, R.HEADER),
        ("field 8.7 twice", good + dup7 + body, R.HEADER),
        ("field 8 twice, each with a field 7", good + two8 + body, R.HEADER),
    ]


def shape_cases(sections=(0, 1, 40, 100)):
    """(name, chunk): well-formed plain chunks of the header shapes of parquet_ref.shape_cases"""
    P = R.payload
    return [
        ("long-form field ids", plain_page_v1(P(3, 100), crc=True, long_ids=True) + plain_page_v1(P(4, 200), long_ids=True)),
        ("unknown fields of every type", plain_page_v1(P(5, 150), crc=True, extra=R.UNKNOWN_EVERY_TYPE,
                                                       sub_extra=R.UNKNOWN_EVERY_TYPE) + plain_page_v1(P(6, 101))),
        ("statistics of 300 bytes", plain_page_v1(P(7, 300), crc=True, sub_extra=[R.STATS_300]) +
         plain_page_v2(b"", b"\x03\x04", P(8, 120), crc=True, sub_extra=[(8, R.STATS_300[1])])),
        ("v2 said to be stored", plain_page_v2(b"\x01\x02\x03", b"\x04\x05", P(10, 170), crc=True, is_compressed=False) +
         plain_page_v2(b"", b"", P(11, 100), is_compressed=False)),
        ("v2 said to be compressed", plain_page_v2(b"\x01", b"\x02" * 99, P(12, 100), crc=True, is_compressed=True)),
        ("v2 of levels only", plain_page_v2(b"\x09" * 7, b"\x08" * 120, b"", crc=True) + plain_page_v2(b"", b"\x07" * 3, b"")),
        ("a dictionary page", plain_page_v1(P(1, 130), crc=True, ptype=R.DICTIONARY_PAGE) + plain_page_v1(P(2, 290), crc=True)),
        ("an index page and an unknown type between data pages", plain_page_v1(P(13, 140), crc=True) +
         R.page_header(R.INDEX_PAGE, 500, 37, crc=123) + bytes(range(37)) + R.page_header(9, 0, 0) + plain_page_v1(P(14, 260), crc=True)),
        ("crc before the sizes' field", R.write_struct([(1, R.i32(0)), (2, R.i32(60)), (4, R.i32(77), True), (3, R.i32(60), True),
                                                        (5, (R.T_STRUCT, [(1, R.i32(5)), (2, R.i32(0))]))]) + P(15, 60)),
        ("the empty chunk", b""),
    ] + [("a section of %d bytes" % n, plain_page_v1(P(30 + k, n), crc=True)) for k, n in enumerate(sections)]


# ---- a generic Thrift tree, for the footer alone ----------------------------------------------------------
# A struct is a list of [field id, type, value]; a bool field's value is in its type.  A list or set is
# (elemtype, [values]), a map (keytype, valuetype, [(key, value)]); integers are ints, T_BYTE and
# T_DOUBLE raw bytes, a binary bytes.

def read_tree(r, t, element=False):
    if t in (R.T_TRUE, R.T_FALSE):
        return (r.byte() == R.T_TRUE) if element else (t == R.T_TRUE)
    if t == R.T_BYTE:
        return bytes([r.byte()])
    if t in (R.T_I16, R.T_I32, R.T_I64):
        return r.zigzag(10)
    if t in (R.T_DOUBLE, R.T_BINARY):
        n = 8 if t == R.T_DOUBLE else r.varint(5)
        r.advance(n)
        return bytes(r.b[r.pos - n:r.pos])
    if t in (R.T_LIST, R.T_SET):
        b = r.byte()
        size, et = b >> 4, b & 15
        if size == 15:
            size = r.varint(5)
        return et, [read_tree(r, et, True) for _ in range(size)]
    if t == R.T_MAP:
        size = r.varint(5)
        if not size:
            return 0, 0, []
        b = r.byte()
        return b >> 4, b & 15, [(read_tree(r, b >> 4, True), read_tree(r, b & 15, True)) for _ in range(size)]
    assert t == R.T_STRUCT
    fields, last = [], 0
    while True:
        f = r.field(last)
        if f is None:
            return fields
        last = f[0]
        fields.append([f[0], f[1], read_tree(r, f[1])])


def write_tree(t, v, element=False):
    if t in (R.T_TRUE, R.T_FALSE):
        return bytes([R.T_TRUE if v else R.T_FALSE]) if element else b""
    if t in (R.T_BYTE, R.T_DOUBLE):
        return bytes(v)
    if t in (R.T_I16, R.T_I32, R.T_I64):
        return R.zigzag(v)
    if t == R.T_BINARY:
        return R.varint(len(v)) + bytes(v)
    if t in (R.T_LIST, R.T_SET):
        et, items = v
        head = bytes([(len(items) << 4) | et]) if len(items) < 15 else bytes([0xF0 | et]) + R.varint(len(items))
        return head + b"".join(write_tree(et, x, True) for x in items)
    if t == R.T_MAP:
        kt, vt, pairs = v
        if not pairs:
            return b"\x00"
        return R.varint(len(pairs)) + bytes([(kt << 4) | vt]) + b"".join(write_tree(kt, k, True) + write_tree(vt, x, True) for k, x in pairs)
    out, last = bytearray(), 0
    for fid, ft, fv in v:
        if ft in (R.T_TRUE, R.T_FALSE):
            ft = R.T_TRUE if fv else R.T_FALSE
        delta = fid - last
        out += bytes([(delta << 4) | ft]) if 0 < delta <= 15 else bytes([ft]) + R.zigzag(fid)
        out += write_tree(ft, fv)
        last = fid
    return bytes(out) + b"\x00"


def field(struct_fields, fid):
    """the [id, type, value] entry of a struct's field, or None"""
    return next((f for f in struct_fields if f[0] == fid), None)


CODEC_SNAPPY = 1


def splice_file(data, compress, transcoded=None):
    """A Parquet file written with compression=NONE as the same file with compression=SNAPPY: every
    column chunk transcoded (or taken from `transcoded`, a dict by the chunk's old offset) and the
    footer's codec, sizes and offsets rewritten.  The untouched footer must round-trip byte for byte."""
    data = bytes(data)
    assert data[:4] == b"PAR1" and data[-4:] == b"PAR1"
    footer_len = struct.unpack("<I", data[-8:-4])[0]
    footer_at = len(data) - 8 - footer_len
    footer = data[footer_at:footer_at + footer_len]
    r = R.Reader(footer, 0)
    meta = read_tree(r, R.T_STRUCT)
    assert r.pos == footer_len and write_tree(R.T_STRUCT, meta) == footer, "the footer does not round-trip"
    out, pos = bytearray(), 0
    for group in field(meta, 4)[2][1]:
        starts, lengths = [], []
        for column in field(group, 1)[2][1]:
            md = field(column, 3)[2]
            assert field(md, 4)[2] == 0, "the file is not compression=NONE"
            dict_off, data_off = field(md, 11), field(md, 9)
            start = dict_off[2] if dict_off is not None else data_off[2]
            old = data[start:start + field(md, 7)[2]]
            if transcoded is not None:
                new = transcoded[start]
            else:
                st, new = transcode(old, compress)
                assert st == 0
            out += data[pos:start]
            pos = start + len(old)
            at = len(out)
            out += new
            pages = R.walk(new)[1]
            field(md, 4)[2] = CODEC_SNAPPY
            field(md, 7)[2] = len(new)
            data_off[2] = at + next(p.hdr_off for p in pages if p.type in (R.DATA_PAGE, R.DATA_PAGE_V2))
            if dict_off is not None:
                dict_off[2] = at + next(p.hdr_off for p in pages if p.type == R.DICTIONARY_PAGE)
            if field(column, 2) is not None and field(column, 2)[2]:
                field(column, 2)[2] += at + len(new) - (start + len(old))
            for fid in (4, 5, 6, 7):
                assert field(column, fid) is None, "page indexes are not moved"
            starts.append(at)
            lengths.append(len(new))
        if field(group, 5) is not None:
            field(group, 5)[2] = starts[0]
        if field(group, 6) is not None:
            field(group, 6)[2] = sum(lengths)
    out += data[pos:footer_at]
    new_footer = write_tree(R.T_STRUCT, meta)
    return bytes(out) + new_footer + struct.pack("<I", len(new_footer)) + b"PAR1"
