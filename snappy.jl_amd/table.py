"""LevelDB table files (.ldb / .sst: blocks stored or Snappy-compressed, each with a type byte and a
masked CRC-32C, found through an index block), over include/snappy_mi355x_table.h --
libsnappy_mi355x_table.so, the companion of libsnappy_mi355x_multi.so, libsnappy_mi355x_framing.so
(its batched CRC-32C) and libsnappy_mi355x.so.  The table's block layer only: no key is compared and
no data block's entries are parsed.

    uncompress_table(data, verify_crc=True)      -> (blocks, handles)   one table (a batch of one)
    uncompress_tables(tables)                    -> list of (blocks, handles)   one batched call
    uncompress_table_blocks(data, handles)       -> list of bytes   blocks named by handle
    compress_table_blocks(blocks, mode)          -> (bytes, handles)   the data blocks, packed
    write_table(blocks, keys, mode)              -> bytes   a whole file the decoder reads back
    read_footer(data), index_bound(data), walk_index(contents, table_len), block_head(data, handle),
    write_tail(keys, handles, base), max_blocks(n), max_block_length(n)   (host, no device)

and, on torch tensors resident in HBM: index_tables_device, uncompress_tables_device,
uncompress_table_blocks_device, compress_table_blocks_device (no host synchronisation), last_indexed.

A handle is (offset from the table's first byte, size of the stored contents); the 5-byte trailer
follows the contents.  The package imports without this library; it is loaded on the first call
here.  No CPU fallback: every codec call needs the four HIP libraries and a device.
"""
import ctypes
import os

import numpy as np

from . import HERE, MODES, SnappyError, _in_arg, _mode
from ._binding import TABLE, Summary, check, context_cache, device_caller, exclusive_scan, lay_out, load, numel

LIB_PATH = os.path.join(HERE, "libsnappy_mi355x_table.so")

SMT_ERR_TRUNCATED = 96
SMT_ERR_MAGIC = 97
SMT_ERR_FOOTER = 98
SMT_ERR_HANDLE = 99
SMT_ERR_TOO_LARGE = 100
SMT_ERR_TYPE = 101
SMT_ERR_INDEX = 102
SMT_ERR_CRC = 103
MAGIC = bytes.fromhex("57fb808b247547db")
FOOTER_LENGTH = 48
BLOCK_TRAILER = 5

TABLE_ABI_SYMBOLS = tuple(TABLE)  # exported symbols of include/snappy_mi355x_table.h (tests/test_table_host.py)

_lib = None


def library_path():
    return LIB_PATH


def lib():
    """Load libsnappy_mi355x_table.so (raises OSError if it was not built)."""
    global _lib
    if _lib is None:
        _lib = load(LIB_PATH, TABLE, "libsnappy_mi355x_table.so not built (run __graft_entry__.build())")
    return _lib


def status_message(code):
    return lib().smt_status_message(int(code)).decode()


def version():
    return lib().smt_version().decode()


class TableError(SnappyError):
    """A SnappyError whose message comes from smt_status_message (the SMT_ERR_* texts too); for a
    table or a block of a batch `index` is its number in the batch, else None."""

    def __init__(self, code, index=None):
        super().__init__(code, status_message(code))
        self.index = index


# context(device=0): the per-device smt_ctx (an smm_ctx and an smf_ctx of its own plus scratch)
_ctx, _ctx_lock, context = context_cache(lib, "smt_ctx_create", SnappyError,
                                         "no usable HIP device %d for snappy_mi355x_table")


# ---- host helpers (no device) ---------------------------------------------------------------

def max_blocks(index_bytes):
    """smt_max_blocks: the most entries index contents of that many bytes hold (5 bytes each at the least)."""
    return lib().smt_max_blocks(int(index_bytes))


def max_block_length(n):
    """smt_max_block_length: the room the encoder needs for a block of n bytes (n + 5)."""
    return lib().smt_max_block_length(int(n))


def read_footer(data, status=False):
    """smt_footer: ((metaindex offset, size), (index offset, size)).  A bad footer raises TableError;
    with status=True the result is (status, those two handles) and nothing is raised."""
    src, n, keep = _in_arg(data)
    v = [ctypes.c_uint64(0) for _ in range(4)]
    st = lib().smt_footer(src, n, *[ctypes.byref(x) for x in v])
    handles = ((v[0].value, v[1].value), (v[2].value, v[3].value))
    if status:
        return int(st), handles
    check(st, TableError)
    return handles


def index_bound(data, status=False):
    """smt_index_bound: the exact decoded length of the table's index block, from the footer and the
    index block's head alone."""
    src, n, keep = _in_arg(data)
    v = ctypes.c_uint64(0)
    st = lib().smt_index_bound(src, n, ctypes.byref(v))
    if status:
        return int(st), v.value
    check(st, TableError)
    return v.value


def block_head(data, handle, status=False):
    """smt_block_head: (type, declared length) of the block at `handle`."""
    src, n, keep = _in_arg(data)
    t, d = ctypes.c_uint32(0), ctypes.c_uint64(0)
    st = lib().smt_block_head(src, n, int(handle[0]), int(handle[1]), ctypes.byref(t), ctypes.byref(d))
    if status:
        return int(st), t.value, d.value
    check(st, TableError)
    return t.value, d.value


def walk_index(contents, table_len, max_entries=None):
    """smt_walk_index over already-decoded index contents: (status, entries walked, handles) -- the
    handles a list of (offset, size) of the entries before the error."""
    src, m, keep = _in_arg(contents)
    s = Summary()
    if max_entries is None:
        lib().smt_walk_index(src, m, int(table_len), None, None, 0, ctypes.byref(s))
        max_entries = s.nchunks
    off, size = np.zeros(max(max_entries, 1), np.uint64), np.zeros(max(max_entries, 1), np.uint64)
    lib().smt_walk_index(src, m, int(table_len), off.ctypes.data, size.ctypes.data, int(max_entries), ctypes.byref(s))
    k = min(s.nchunks, max_entries)
    return int(s.status), int(s.nchunks), list(zip(off[:k].tolist(), size[:k].tolist()))


def write_tail(keys, handles, base):
    """smt_write_tail: the metaindex block, the index block (restart interval 1) over `keys` and
    `handles`, and the footer, for data blocks that take `base` bytes in front."""
    keys = [bytes(k) for k in keys]
    if len(keys) != len(handles):
        raise ValueError("one key per handle")
    buf = np.frombuffer(b"".join(keys), np.uint8) if any(keys) else np.zeros(1, np.uint8)
    koff = exclusive_scan([len(k) for k in keys], total=True)
    hoff = np.array([h[0] for h in handles] + [0], np.uint64)
    hsize = np.array([h[1] for h in handles] + [0], np.uint64)
    n = ctypes.c_size_t(0)
    args = (buf.ctypes.data, koff.ctypes.data, len(keys), hoff.ctypes.data, hsize.ctypes.data, int(base))
    check(lib().smt_write_tail(*args, None, 0, ctypes.byref(n)), TableError)
    out = np.empty(n.value, np.uint8)
    check(lib().smt_write_tail(*args, out.ctypes.data, out.size, ctypes.byref(n)), TableError)
    return out.tobytes()


# ---- host buffers -----------------------------------------------------------------------

def _raise_first(codes):
    for i, code in enumerate(codes):
        if code:
            raise TableError(code, i)


def _decode_call(buf, offs, lens, caps, verify_crc, device, entries):
    k = len(lens)
    cap = np.ascontiguousarray(caps, dtype=np.uint64)
    out_off = exclusive_scan(cap, total=True)
    out = np.empty(max(int(out_off[-1]), 1), np.uint8)
    out_len, status = np.zeros(k, np.uint64), np.zeros(k, np.int32)
    first = np.zeros(k + 1, np.uint32)
    n = max(entries, 1)
    hoff, hsize, blen, bst = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.int32)
    check(lib().smt_uncompress_tables(context(device), buf.ctypes.data, offs.ctypes.data, lens.ctypes.data, k,
                                      1 if verify_crc else 0, out.ctypes.data, out_off.ctypes.data, cap.ctypes.data,
                                      out_len.ctypes.data, status.ctypes.data, first.ctypes.data, entries, hoff.ctypes.data,
                                      hsize.ctypes.data, blen.ctypes.data, bst.ctypes.data), TableError)
    return out, out_off, out_len, status, first, hoff, hsize, blen, bst


def uncompress_tables(tables, verify_crc=True, device=0, statuses=False):
    """Decode every data block of every table of `tables` in batched calls (smt_uncompress_tables):
    a list of (blocks, handles) -- the decoded blocks as a list of bytes and their handles as a list
    of (offset, size).  The first call, with no room, learns every table's decoded size (each
    well-formed table answers SM_BUFFER_TOO_SMALL with it); the second decodes.  A failing table
    raises TableError (the first failing table's status, its number as `.index`); with statuses=True
    nothing is raised and the result is (that list, with None for a failing table's blocks; list of
    statuses)."""
    tables = list(tables)
    k = len(tables)
    if not k:
        return ([], []) if statuses else []
    buf, offs, lens = lay_out(tables)
    entries = 0
    for t in tables:
        st, ib = index_bound(t, status=True)
        entries += max_blocks(ib) if st == 0 else 0
    _, _, need, pre, _, _, _, _, _ = _decode_call(buf, offs, lens, np.zeros(k, np.uint64), verify_crc, device, entries)
    fits = (pre == 2) | ((pre == 0) & (need == 0))  # SM_BUFFER_TOO_SMALL; an empty table needs no second look
    caps = np.where(fits, need, 0).astype(np.uint64)
    out, out_off, out_len, status, first, hoff, hsize, blen, _ = _decode_call(buf, offs, lens, caps, verify_crc, device, entries)
    codes = status.tolist()
    if not statuses:
        _raise_first(codes)
    res = []
    for t in range(k):
        lo, hi = int(first[t]), int(first[t + 1])
        handles = list(zip(hoff[lo:hi].tolist(), hsize[lo:hi].tolist()))
        if codes[t]:
            res.append((None, handles))
            continue
        at = int(out_off[t]) + np.concatenate(([0], np.cumsum(blen[lo:hi], dtype=np.uint64))).astype(np.int64)
        res.append(([out[at[i]:at[i + 1]].tobytes() for i in range(hi - lo)], handles))
    return (res, codes) if statuses else res


def uncompress_table(data, verify_crc=True, device=0):
    """One table: (its data blocks decoded, their handles)."""
    try:
        return uncompress_tables([data], verify_crc=verify_crc, device=device)[0]
    except TableError as e:
        raise TableError(e.code) from None  # (a table alone has no number)


def uncompress_table_blocks(data, handles, verify_crc=True, device=0, statuses=False):
    """The blocks of `data` named by `handles` (a list of (offset, size); trusted to lie inside
    `data` with their trailers), decoded in one batched call (smt_uncompress_blocks): a list of
    bytes.  A failing block raises TableError (its number as `.index`); with statuses=True the result
    is (that list, with None for a failing block; list of statuses)."""
    handles = [(int(o), int(s)) for o, s in handles]
    k = len(handles)
    if not k:
        return ([], []) if statuses else []
    src, n, keep = _in_arg(data)
    heads = [block_head(data, h, status=True) for h in handles]
    cap = np.array([d if st == 0 else 0 for st, _, d in heads], np.uint64)
    out_off = exclusive_scan(cap, total=True)
    out = np.empty(max(int(out_off[-1]), 1), np.uint8)
    off, size = np.array([h[0] for h in handles], np.uint64), np.array([h[1] for h in handles], np.uint64)
    out_len, status = np.zeros(k, np.uint64), np.zeros(k, np.int32)
    check(lib().smt_uncompress_blocks(context(device), src, n, off.ctypes.data, size.ctypes.data, k, 1 if verify_crc else 0,
                                      out.ctypes.data, out_off.ctypes.data, cap.ctypes.data, out_len.ctypes.data,
                                      status.ctypes.data), TableError)
    codes = status.tolist()
    if not statuses:
        _raise_first(codes)
    res = [None if c else out[int(o):int(o) + int(m)].tobytes() for o, m, c in zip(out_off, out_len, codes)]
    return (res, codes) if statuses else res


def compress_tables_blocks(tables, mode="fast", device=0):
    """For every table of `tables` (a list of blocks each) its data blocks compressed by LevelDB's
    12.5 % rule, checksummed and packed back to back, in one batched call (smt_compress_blocks): a
    list of (bytes, handles)."""
    tables = [[bytes(b) for b in blocks] for blocks in tables]
    k = len(tables)
    if not k:
        return []
    parts = [b for blocks in tables for b in blocks]
    buf, offs, lens = lay_out(parts)
    m = len(parts)
    first = exclusive_scan([len(b) for b in tables], np.uint32, total=True)
    block_len = lens.astype(np.uint32) if m else np.zeros(1, np.uint32)
    block_off = offs if m else np.zeros(1, np.uint64)
    room = [sum(len(b) + BLOCK_TRAILER for b in blocks) for blocks in tables]
    out_off = exclusive_scan(room, total=True)
    out = np.empty(max(int(out_off[-1]), 1), np.uint8)
    out_len, status = np.zeros(k, np.uint64), np.zeros(k, np.int32)
    hoff, hsize = np.zeros(max(m, 1), np.uint64), np.zeros(max(m, 1), np.uint64)
    check(lib().smt_compress_blocks(context(device), buf.ctypes.data, first.ctypes.data, block_off.ctypes.data,
                                    block_len.ctypes.data, k, out.ctypes.data, out_off.ctypes.data, hoff.ctypes.data,
                                    hsize.ctypes.data, out_len.ctypes.data, status.ctypes.data, _mode(mode)), TableError)
    _raise_first(status.tolist())
    return [(out[int(out_off[t]):int(out_off[t]) + int(out_len[t])].tobytes(),
             list(zip(hoff[first[t]:first[t + 1]].tolist(), hsize[first[t]:first[t + 1]].tolist()))) for t in range(k)]


def compress_table_blocks(blocks, mode="fast", device=0):
    """One table's data blocks: (bytes, handles)."""
    try:
        return compress_tables_blocks([blocks], mode=mode, device=device)[0]
    except TableError as e:
        raise TableError(e.code) from None


def write_table(blocks, keys, mode="fast", device=0):
    """A whole table file: the data blocks compressed, checksummed and packed on the device, then
    the metaindex block, the index block over `keys` (one separator key per block: at or above the
    block's last key and below the next block's first) and the footer, written on the host."""
    if len(blocks) != len(keys):
        raise ValueError("one key per block")
    data, handles = compress_table_blocks(blocks, mode=mode, device=device)
    return data + write_tail(keys, handles, len(data))


# ---- device API (torch tensors resident in HBM; asynchronous on `stream`) ---------------------

_device = device_caller(lib, context, TableError)


def index_tables_device(d_in, d_in_off, d_in_len, max_blocks, max_index_bytes, d_block_first, d_handle_off, d_handle_size,
                        d_status, verify_crc=True, stream=None, device=None):
    """smt_index_tables_device: table t = d_in[d_in_off[t] : d_in_off[t] + d_in_len[t]] (int64 both);
    d_block_first int32[ntables + 1], d_handle_off / d_handle_size int64[max_blocks], d_status
    int32[ntables].  max_index_bytes bounds the decoded index lengths, each rounded up to 16.  Nothing
    is synchronised.
    Arguments are checked first (_binding.device_caller; README, Device API).
    Length not checked: d_handle_off, d_handle_size."""
    _device("smt_index_tables_device", d_status, device, stream, d_in, d_in_off, d_in_len, numel(d_in_len), int(max_blocks),
            int(max_index_bytes), 1 if verify_crc else 0, d_block_first, d_handle_off, d_handle_size, d_status)


def uncompress_tables_device(d_in, d_in_off, d_in_len, max_blocks, max_index_bytes, max_fragments, d_out, d_out_off, d_out_cap,
                             d_out_len, d_status, verify_crc=True, d_block_first=None, d_handle_off=None, d_handle_size=None,
                             d_block_out_off=None, d_block_len=None, d_block_status=None, stream=None, device=None):
    """smt_uncompress_tables_device: every data block of table t decodes into d_out[d_out_off[t] :
    d_out_off[t] + d_out_cap[t]]; per table d_out_len (int64) and d_status (int32).  Optional:
    d_block_first int32[ntables + 1] and, with max_blocks entries each, d_handle_off, d_handle_size,
    d_block_out_off, d_block_len (int64) and d_block_status (int32).  Nothing is synchronised.
    Arguments are checked first (_binding.device_caller; README, Device API).
    Length not checked: d_handle_off, d_handle_size, d_block_out_off, d_block_len, d_block_status."""
    _device("smt_uncompress_tables_device", d_out, device, stream, d_in, d_in_off, d_in_len, numel(d_in_len), int(max_blocks),
            int(max_index_bytes), int(max_fragments), 1 if verify_crc else 0, d_out, d_out_off, d_out_cap, d_out_len, d_status,
            d_block_first, d_handle_off, d_handle_size, d_block_out_off, d_block_len, d_block_status)


def uncompress_table_blocks_device(d_in, d_blk_off, d_blk_size, max_fragments, d_out, d_out_off, d_out_cap, d_out_len, d_status,
                                   verify_crc=True, stream=None, device=None):
    """smt_uncompress_blocks_device: block j's contents are d_in[d_blk_off[j] : + d_blk_size[j]]
    (int64, trusted) with its trailer behind; it decodes into d_out[d_out_off[j] : + d_out_cap[j]];
    per block d_out_len (int64) and d_status (int32).  Nothing is synchronised.
    Arguments are checked first (_binding.device_caller; README, Device API)."""
    _device("smt_uncompress_blocks_device", d_out, device, stream, d_in, d_blk_off, d_blk_size, numel(d_blk_off),
            int(max_fragments), 1 if verify_crc else 0, d_out, d_out_off, d_out_cap, d_out_len, d_status)


def compress_table_blocks_device(d_in, d_block_first, d_block_off, d_block_len, max_blocks, stage_bytes, max_fragments, d_out,
                                 d_out_off, d_handle_off, d_handle_size, d_out_len, d_status, mode="fast", stream=None,
                                 device=None):
    """smt_compress_blocks_device: table t is the blocks d_block_first[t] .. d_block_first[t + 1]
    (int32[ntables + 1]) of d_block_off (int64) and d_block_len (int32), written back to back at
    d_out[d_out_off[t]:], where the sum of max_block_length(len) is left for it; per block
    d_handle_off / d_handle_size (int64), per table d_out_len (int64) and d_status (int32).
    max_blocks, stage_bytes (the sum of smt_stage_length) and max_fragments bound the batch.  Nothing
    is synchronised.
    Arguments are checked first (_binding.device_caller; README, Device API).
    Length not checked: d_block_off, d_block_len, d_handle_off, d_handle_size."""
    _device("smt_compress_blocks_device", d_out, device, stream, d_in, d_block_first, d_block_off, d_block_len,
            numel(d_out_off), int(max_blocks), int(stage_bytes), int(max_fragments), d_out, d_out_off, d_handle_off,
            d_handle_size, d_out_len, d_status, _mode(mode))


def last_indexed(device=0):
    """Diagnostic (smt_ctx_last_indexed): how many blocks the device's last decode call took by
    fragments (waits for the device); -1 before the first call."""
    return int(lib().smt_ctx_last_indexed(context(device)))


__all__ = ["TABLE_ABI_SYMBOLS", "MODES", "MAGIC", "TableError", "uncompress_table", "uncompress_tables",
           "uncompress_table_blocks", "compress_table_blocks", "compress_tables_blocks", "write_table", "write_tail",
           "read_footer", "index_bound", "walk_index", "block_head", "max_blocks", "max_block_length", "index_tables_device",
           "uncompress_tables_device", "uncompress_table_blocks_device", "compress_table_blocks_device", "last_indexed",
           "status_message", "version"]
