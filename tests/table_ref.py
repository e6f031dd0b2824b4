"""A plain-Python reference of the LevelDB table file, written from LevelDB's doc/table_format.md and
the rules and status order of include/snappy_mi355x_table.h: a block builder (prefix compression,
restart interval 16), an index builder (interval 1), a table writer (the 12.5 % rule), a footer and
index reader, a block reader, an entry iterator, a CRC-32C and the decode plan.  It shares no code
with the library.  Payloads come from the `compress` / `uncompress` the caller hands in (pyarrow's
libsnappy, or the oracle).  tests/test_table_host.py pins it by known answers that do not come from
it."""
import collections
import struct

SM_OK = 0
SM_BUFFER_TOO_SMALL = 2
SM_ERR_ARGUMENT = 33
SM_ERR_VARINT = 18
TRUNCATED, MAGIC_ERR, FOOTER, HANDLE, TOO_LARGE, TYPE, INDEX, CRC = range(96, 104)
MAGIC = bytes.fromhex("57fb808b247547db")
FOOTER_LEN = 48
TRAILER = 5
MAX_SIZE = 0x7FFFFFFE
MAX_DECLARED = 0x7FFFFFFF
DECODER_REFUSED = -1  # a payload the caller's uncompress refuses: whatever status the raw decoder gives

Plan = collections.namedtuple("Plan", "status out_len decoded handles block_out_off block_len block_status")


class Stop(Exception):
    def __init__(self, status):
        self.status = status


# ---- CRC-32C --------------------------------------------------------------------------------------

def _crc_table():
    table = []
    for i in range(256):
        c = i
        for _ in range(8):
            c = (c >> 1) ^ (0x82F63B78 if c & 1 else 0)
        table.append(c)
    return table


_TABLE = _crc_table()


def crc32c(data):
    c = 0xFFFFFFFF
    for b in bytes(data):
        c = (c >> 8) ^ _TABLE[(c ^ b) & 0xFF]
    return c ^ 0xFFFFFFFF


def mask(c):
    return (((c >> 15) | (c << 17)) + 0xA282EAD8) & 0xFFFFFFFF


# ---- varints --------------------------------------------------------------------------------------

def put_varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append(0x80 | (v & 0x7F))
        v >>= 7
    out.append(v)
    return bytes(out)


def get_varint32(buf, pos, end):
    """(value, position behind it), or None: truncated, more than 5 bytes, or a 5th byte of 0x10 or more."""
    v = 0
    for i in range(5):
        if pos + i >= end:
            return None
        b = buf[pos + i]
        if i == 4 and b >= 0x10:
            return None
        v |= (b & 0x7F) << (7 * i)
        if b < 0x80:
            return v, pos + i + 1
    return None


def get_varint64(buf, pos, end):
    """(value, position behind it), or None: truncated, or a 10th byte above 1."""
    v = 0
    for i in range(10):
        if pos + i >= end:
            return None
        b = buf[pos + i]
        if i == 9:
            if b > 1:
                return None
            return v | (b << 63), pos + 10
        v |= (b & 0x7F) << (7 * i)
        if b < 0x80:
            return v, pos + i + 1
    return None


def put_handle(h):
    return put_varint(h[0]) + put_varint(h[1])


# ---- the writer -----------------------------------------------------------------------------------

def build_block(entries, interval=16):
    """A block's contents from (key, value) pairs in key order: prefix-compressed entries, a restart
    point every `interval` entries, the restart array and its count."""
    out, restarts, last = bytearray(), [], b""
    for i, (key, value) in enumerate(entries):
        key, value = bytes(key), bytes(value)
        shared = 0
        if i % interval == 0:
            restarts.append(len(out))
        else:
            while shared < min(len(last), len(key)) and last[shared] == key[shared]:
                shared += 1
        out += put_varint(shared) + put_varint(len(key) - shared) + put_varint(len(value)) + key[shared:] + value
        last = key
    if not restarts:
        restarts = [0]
    return bytes(out) + b"".join(struct.pack("<I", r) for r in restarts) + struct.pack("<I", len(restarts))


def build_index(keys, handles):
    return build_block([(k, put_handle(h)) for k, h in zip(keys, handles)], interval=1)


def stored_block(contents, compress=None):
    """contents + type + masked crc, by the 12.5 % rule when a compressor is given: (bytes, size)."""
    contents = bytes(contents)
    body, kind = contents, 0
    if compress is not None:
        c = compress(contents)
        if len(c) < len(contents) - len(contents) // 8:
            body, kind = c, 1
    body += bytes([kind])
    return body + struct.pack("<I", mask(crc32c(body))), len(body) - 1


def write_tail(keys, handles, base, compress=None):
    """The metaindex block (empty), the index block and the footer behind `base` bytes of data blocks."""
    meta, msize = stored_block(build_block([]))
    index, isize = stored_block(build_index(keys, handles), compress)
    foot = put_handle((base, msize)) + put_handle((base + len(meta), isize))
    return meta + index + foot + bytes(40 - len(foot)) + MAGIC


def write_blocks(blocks, compress):
    """The data blocks back to back: (bytes, handles)."""
    out, handles = bytearray(), []
    for b in blocks:
        stored, size = stored_block(b, compress)
        handles.append((len(out), size))
        out += stored
    return bytes(out), handles


def write_table(blocks, keys, compress, compress_index=False):
    data, handles = write_blocks(blocks, compress)
    return data + write_tail(keys, handles, len(data), compress if compress_index else None)


# ---- the reader -----------------------------------------------------------------------------------

def check_handle(h, n):
    if h[0] + h[1] + TRAILER > n - FOOTER_LEN:
        raise Stop(HANDLE)
    if h[1] > MAX_SIZE:
        raise Stop(TOO_LARGE)


def read_footer(buf):
    """(metaindex handle, index handle); Stop(status) by the footer rule."""
    n = len(buf)
    if n < FOOTER_LEN:
        raise Stop(TRUNCATED)
    if bytes(buf[n - 8:]) != MAGIC:
        raise Stop(MAGIC_ERR)
    pos, end, vals = n - FOOTER_LEN, n - 8, []
    for _ in range(4):
        got = get_varint64(buf, pos, end)
        if got is None:
            raise Stop(FOOTER)
        vals.append(got[0])
        pos = got[1]
    meta, index = (vals[0], vals[1]), (vals[2], vals[3])
    check_handle(meta, n)
    check_handle(index, n)
    return meta, index


def block_head(buf, h):
    """(type, declared length) of the block at handle h; Stop(TYPE / SM_ERR_VARINT / TOO_LARGE)."""
    off, size = h
    kind = buf[off + size]
    if kind == 0:
        return 0, size
    if kind != 1:
        raise Stop(TYPE)
    got = get_varint32(buf, off, off + min(size, 5))
    if got is None:
        raise Stop(SM_ERR_VARINT)
    if got[0] > MAX_DECLARED:
        raise Stop(TOO_LARGE)
    return 1, got[0]


def crc_ok(buf, h):
    off, size = h
    return struct.unpack_from("<I", buf, off + size + 1)[0] == mask(crc32c(buf[off:off + size + 1]))


def read_block(buf, h, uncompress, verify_crc=True):
    """(status, contents or None) of one block by block rules 5 and 6; head errors raise Stop."""
    kind, declared = block_head(buf, h)
    if verify_crc and not crc_ok(buf, h):
        return CRC, None
    off, size = h
    if kind == 0:
        return SM_OK, bytes(buf[off:off + size])
    return decode(uncompress, bytes(buf[off:off + size]), declared)


def decode(uncompress, payload, declared):
    """(status, bytes or None) of a raw stream: uncompress gives the bytes, None for a payload it
    refuses (DECODER_REFUSED), or the raw decoder's own status as an int where the caller knows it."""
    data = uncompress(payload)
    if isinstance(data, int):
        return data, None
    if data is None or len(data) != declared:
        return DECODER_REFUSED, None
    return SM_OK, data


def walk_index(contents, table_len):
    """(status, handles before the error) by the index rule."""
    c, m, handles = bytes(contents), len(contents), []
    try:
        if m < 4:
            raise Stop(INDEX)
        r = struct.unpack_from("<I", c, m - 4)[0]
        if r > (m - 4) // 4:
            raise Stop(INDEX)
        limit, p, key_len = m - 4 * (1 + r), 0, 0
        while p != limit:
            if limit - p < 3:
                raise Stop(INDEX)
            f = []
            for _ in range(3):
                got = get_varint32(c, p, limit)
                if got is None:
                    raise Stop(INDEX)
                f.append(got[0])
                p = got[1]
            shared, non_shared, value_len = f
            if non_shared + value_len > limit - p:
                raise Stop(INDEX)
            if shared > key_len:
                raise Stop(INDEX)
            key_len = shared + non_shared
            v, vend = p + non_shared, p + non_shared + value_len
            off = get_varint64(c, v, vend)
            size = get_varint64(c, off[1], vend) if off else None
            if size is None:
                raise Stop(INDEX)
            h = (off[0], size[0])
            check_handle(h, table_len)
            handles.append(h)
            p = vend
    except Stop as e:
        return e.status, handles
    return SM_OK, handles


def entries(contents):
    """The (key, value) pairs of a decoded block, by LevelDB's Block iterator (no error handling:
    for blocks the tests wrote)."""
    c, m = bytes(contents), len(contents)
    r = struct.unpack_from("<I", c, m - 4)[0]
    limit, p, key = m - 4 * (1 + r), 0, b""
    while p < limit:
        shared, p = get_varint32(c, p, limit)
        non_shared, p = get_varint32(c, p, limit)
        value_len, p = get_varint32(c, p, limit)
        key = key[:shared] + c[p:p + non_shared]
        yield key, c[p + non_shared:p + non_shared + value_len]
        p += non_shared + value_len


# ---- the decode plan ------------------------------------------------------------------------------

def plan(buf, uncompress, cap=None, verify_crc=True):
    """What smt_uncompress_tables_device gives for one table with `cap` bytes of room (None: enough):
    Plan(status, out_len, decoded bytes or None, handles, block_out_off, block_len, block_status).  A
    block the caller's uncompress refuses has status DECODER_REFUSED, which stands for the raw
    decoder's status, whatever it is."""
    buf = bytes(buf)
    n = len(buf)
    try:
        _, index = read_footer(buf)
        kind, declared = None, None
        try:
            kind, declared = block_head(buf, index)
        except Stop as e:
            if e.status == TYPE:
                raise
            head = e.status
        else:
            head = SM_OK
        if verify_crc and not crc_ok(buf, index):
            raise Stop(CRC)
        if head != SM_OK:
            raise Stop(head)
        contents = bytes(buf[index[0]:index[0] + index[1]])
        if kind == 1:
            st, contents = decode(uncompress, contents, declared)
            if st != SM_OK:
                raise Stop(st)
    except Stop as e:
        return Plan(e.status, 0, None, [], [], [], [])
    status, handles = walk_index(contents, n)
    if status != SM_OK:
        return Plan(status, 0, None, [], [], [], [])
    lens, total = [], 0
    for h in handles:
        try:
            lens.append(block_head(buf, h)[1])
        except Stop as e:
            return Plan(e.status, total, None, handles, [], [], [])
        total += lens[-1]
    offs = [sum(lens[:i]) for i in range(len(lens))] if len(lens) < 64 else _scan(lens)
    if cap is not None and total > cap:
        return Plan(SM_BUFFER_TOO_SMALL, total, None, handles, offs, lens, [0] * len(lens))
    out, sts = bytearray(), []
    for h, d in zip(handles, lens):
        st, data = read_block(buf, h, uncompress, verify_crc)
        sts.append(st)
        out += data if data is not None else bytes(d)
    first = next((s for s in sts if s != SM_OK), SM_OK)
    return Plan(first, total, bytes(out), handles, offs, lens, sts)


def _scan(lens):
    out, at = [], 0
    for d in lens:
        out.append(at)
        at += d
    return out
