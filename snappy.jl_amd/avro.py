"""Avro object container files whose avro.codec is snappy, over include/snappy_mi355x_avro.h --
libsnappy_mi355x_avro.so, the companion of libsnappy_mi355x_multi.so, libsnappy_mi355x_parquet.so
(its batched CRC-32) and libsnappy_mi355x.so.  The container layer only: blocks of serialized bytes
and their object counts; no record is parsed and no schema interpreted.

    uncompress_avro(file, verify_crc=True)        -> (bytes, blocks)  one file (a batch of one)
    uncompress_avro_streams(files, kind, sync)    -> list of (bytes, blocks)   one batched call
    compress_avro(blocks, counts, schema, sync)   -> bytes            a whole file
    compress_avro_streams(streams, syncs, heads)  -> list of bytes    many streams, one batched call
    write_header(schema, sync, meta)              -> bytes            the header alone (host)
    find_sync(streams, syncs, queries)            -> positions        the split rule, on the device
    index_avro(x, kind, sync)                     -> (summary, arrays)  the host walk
    avro_plan(xs, kind, syncs), find_sync_host, max_blocks(n), max_block_length(n)   (host, no device)

and, on torch tensors resident in HBM: uncompress_avro_streams_device, compress_avro_streams_device,
find_sync_device (no host synchronisation), last_indexed.

The package imports without this library; it is loaded on the first call here.  No CPU fallback:
every codec call needs the four HIP libraries and a device.
"""
import ctypes
import os

import numpy as np

from . import HERE, MODES, SnappyError, _in_arg, _mode
from ._binding import (AVRO, AVRO_BLOCK_KEYS, AvroBlocks, AvroSummary, check, collect, context_cache, device_caller,
                       exclusive_scan, field_dtypes, lay_out, load, numel)

LIB_PATH = os.path.join(HERE, "libsnappy_mi355x_avro.so")

KINDS = {"file": 0, "blocks": 1}
SMA_ERR_NO_HEADER = 80
SMA_ERR_BAD_HEADER = 81
SMA_ERR_TRUNCATED = 82
SMA_ERR_VARLONG = 83
SMA_ERR_CODEC = 84
SMA_ERR_BLOCK = 85
SMA_ERR_TOO_LARGE = 86
SMA_ERR_SYNC = 87
SMA_ERR_CRC = 88
MAGIC = b"Obj\x01"
SYNC_LENGTH = 16
INDEX_KEYS = AVRO_BLOCK_KEYS  # sma_blocks' arrays, in its order
BLOCK_DTYPES = field_dtypes(AvroBlocks)  # the arrays' element types as the C ABI declares them (AvroBlocks.elements)

AVRO_ABI_SYMBOLS = tuple(AVRO)  # exported symbols of include/snappy_mi355x_avro.h (tests/test_avro_host.py)

_lib = None


def library_path():
    return LIB_PATH


def lib():
    """Load libsnappy_mi355x_avro.so (raises OSError if it was not built)."""
    global _lib
    if _lib is None:
        _lib = load(LIB_PATH, AVRO, "libsnappy_mi355x_avro.so not built (run __graft_entry__.build())")
    return _lib


def status_message(code):
    return lib().sma_status_message(int(code)).decode()


def version():
    return lib().sma_version().decode()


class AvroError(SnappyError):
    """A SnappyError whose message comes from sma_status_message (the SMA_ERR_* texts too); for a
    stream of a batch `stream` is its number in the batch, else None."""

    def __init__(self, code, stream=None):
        super().__init__(code, status_message(code))
        self.stream = stream


# context(device=0): the per-device sma_ctx (an smm_ctx and an smq_ctx of its own plus scratch)
_ctx, _ctx_lock, context = context_cache(lib, "sma_ctx_create", SnappyError,
                                         "no usable HIP device %d for snappy_mi355x_avro")


def _kind(kind):
    if kind not in KINDS:
        raise ValueError("kind must be 'file' or 'blocks'")
    return KINDS[kind]


def _syncs(syncs, k, needed):
    """The k markers behind one another as a uint8 array, or None."""
    if syncs is None:
        if needed:
            raise ValueError("a block run needs its 16-byte sync marker")
        return None
    syncs = [bytes(s) for s in syncs]
    if len(syncs) != k or any(len(s) != SYNC_LENGTH for s in syncs):
        raise ValueError("one 16-byte sync marker per stream")
    return np.frombuffer(b"".join(syncs), np.uint8) if k else np.zeros(0, np.uint8)


# ---- host helpers (no device) ---------------------------------------------------------------

def max_blocks(n):
    """sma_max_blocks: the most blocks n bytes can hold (23 bytes each at the least)."""
    return lib().sma_max_blocks(int(n))


def max_block_length(n):
    """sma_max_block_length: the room the encoder needs for a block of n bytes."""
    return lib().sma_max_block_length(int(n))


def index_avro(data, kind="file", sync=None, max_blocks=None):
    """The host walk (sma_index): (AvroSummary, dict of numpy arrays keyed as INDEX_KEYS, of the
    blocks).  max_blocks=None sizes the arrays by a counting walk first."""
    src, n, keep = _in_arg(data)
    k = _kind(kind)
    marker = _syncs(None if sync is None else [sync], 1, k == 1)
    mp = None if marker is None else marker.ctypes.data
    s = AvroSummary()
    if max_blocks is None:
        lib().sma_index(src, n, k, mp, None, 0, ctypes.byref(s))
        max_blocks = s.nblocks
    arrays = {key: np.zeros(max_blocks, BLOCK_DTYPES[key]) for key in INDEX_KEYS}
    table = AvroBlocks(*(arrays[key].ctypes.data for key in INDEX_KEYS))
    lib().sma_index(src, n, k, mp, ctypes.byref(table), max_blocks, ctypes.byref(s))
    return s, arrays


def length_uncompressed(data, kind="file", sync=None):
    """The stream's total uncompressed length from its blocks' varints (no device)."""
    src, n, keep = _in_arg(data)
    k = _kind(kind)
    marker = _syncs(None if sync is None else [sync], 1, k == 1)
    res = ctypes.c_size_t(0)
    check(lib().sma_uncompressed_length(src, n, k, None if marker is None else marker.ctypes.data, ctypes.byref(res)), AvroError)
    return res.value


def avro_plan(streams, kind="file", syncs=None, out_cap=None, max_blocks=0x7FFFFFFF):
    """sma_streams_plan, the device's decode plan on the host, for a list of streams: (rc, first,
    out_len, status, objects, total_blocks, total_fragments) -- per stream what is known before any
    byte is decoded (the walk's error, SM_BUFFER_TOO_SMALL against out_cap[s], or 0), the size needed,
    the objects, the exclusive scan of the slots (len(streams) + 1 entries), and the device call's two
    bounds."""
    buf, offs, lens = lay_out(streams)
    k = len(streams)
    marker = _syncs(syncs, k, _kind(kind) == 1 and k > 0)
    cap = None if out_cap is None else np.ascontiguousarray(out_cap, dtype=np.uint64)
    first, out_len, status = np.zeros(k + 1, np.uint32), np.zeros(k, np.uint64), np.zeros(k, np.int32)
    objects = np.zeros(k, np.uint64)
    blocks, fragments = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = lib().sma_streams_plan(buf.ctypes.data, offs.ctypes.data, lens.ctypes.data, k, _kind(kind),
                                None if marker is None else marker.ctypes.data, None if cap is None else cap.ctypes.data,
                                int(max_blocks), first.ctypes.data, out_len.ctypes.data, status.ctypes.data, objects.ctypes.data,
                                ctypes.byref(blocks), ctypes.byref(fragments))
    return int(rc), first, out_len, status, objects, blocks.value, fragments.value


def find_sync_host(streams, syncs, queries):
    """sma_find_sync, the split rule on the host: for each query (stream, from) the position of the
    first occurrence of that stream's marker at or after `from`, else the stream's length."""
    buf, offs, lens = lay_out(streams)
    marker = _syncs(syncs, len(streams), True)
    qs = np.array([q[0] for q in queries], np.uint32)
    qf = np.array([q[1] for q in queries], np.uint64)
    pos = np.zeros(len(queries), np.uint64)
    check(lib().sma_find_sync(buf.ctypes.data, offs.ctypes.data, lens.ctypes.data, marker.ctypes.data, len(streams),
                              qs.ctypes.data, qf.ctypes.data, len(queries), pos.ctypes.data), AvroError)
    return pos.tolist()


def write_header(schema, sync, meta=()):
    """sma_write_header: a file header with avro.schema = schema, avro.codec = snappy, then the
    (key, value) pairs of `meta`, and the marker."""
    schema, sync = bytes(schema), bytes(sync)
    if len(sync) != SYNC_LENGTH:
        raise ValueError("the sync marker is 16 bytes")
    parts = [bytes(x) for pair in meta for x in pair]
    extra = np.frombuffer(b"".join(parts), np.uint8) if parts else np.zeros(1, np.uint8)
    eoff = exclusive_scan([len(p) for p in parts], total=True)
    n = ctypes.c_size_t(0)
    args = (schema, len(schema), extra.ctypes.data, eoff.ctypes.data, len(parts) // 2, sync)
    check(lib().sma_write_header(*args, None, 0, ctypes.byref(n)), AvroError)
    out = np.empty(n.value, np.uint8)
    check(lib().sma_write_header(*args, out.ctypes.data, out.size, ctypes.byref(n)), AvroError)
    return out.tobytes()


# ---- host buffers -----------------------------------------------------------------------

def _raise_first(codes):
    for s, code in enumerate(codes):
        if code:
            raise AvroError(code, s)


def uncompress_avro_streams(streams, kind="file", syncs=None, verify_crc=True, device=0, statuses=False):
    """Decode a list of files (or, with kind="blocks" and their markers, block runs) in one batched
    call (sma_uncompress_streams): a list of (bytes, block table), the table a dict of numpy arrays
    as index_avro gives it.  With verify_crc every block's CRC-32 is checked on the device.  A
    failing stream raises AvroError (the first failing stream's status, its number as `.stream`);
    with statuses=True nothing is raised and the result is (that list, with None for a failing
    stream's bytes; list of statuses)."""
    streams = list(streams)
    k = len(streams)
    if not streams:
        return ([], []) if statuses else []
    kd = _kind(kind)
    marker = _syncs(syncs, k, kd == 1)
    buf, offs, lens = lay_out(streams)
    _, _, need, pre, _, _, _ = avro_plan(streams, kind, syncs)
    cap = np.where(pre == 0, need, 0).astype(np.uint64)
    out_off = exclusive_scan(cap, total=True)
    out = np.empty(max(int(out_off[-1]), 1), np.uint8)
    out_len, status, objects = np.zeros(k, np.uint64), np.zeros(k, np.int32), np.zeros(k, np.uint64)
    check(lib().sma_uncompress_streams(context(device), kd, buf.ctypes.data, offs.ctypes.data, lens.ctypes.data,
                                       None if marker is None else marker.ctypes.data, k, 1 if verify_crc else 0,
                                       out.ctypes.data, out_off.ctypes.data, cap.ctypes.data, out_len.ctypes.data,
                                       status.ctypes.data, objects.ctypes.data), AvroError)
    codes = status.tolist()
    if not statuses:
        _raise_first(codes)
    tables = [index_avro(s, kind, None if syncs is None else syncs[i])[1] for i, s in enumerate(streams)]
    res = list(zip(collect(out, out_off, out_len, codes), tables))
    return (res, codes) if statuses else res


def uncompress_avro(data, verify_crc=True, device=0):
    """One file: (its blocks' serialized bytes back to back, the block table)."""
    try:
        return uncompress_avro_streams([data], verify_crc=verify_crc, device=device)[0]
    except AvroError as e:
        raise AvroError(e.code) from None  # (a file alone has no number)


def compress_avro_streams(streams, syncs, heads=None, mode="fast", device=0):
    """Every stream of `streams` -- a pair (blocks, counts): the serialized bytes of each block and
    how many objects it holds -- as one run of blocks with the marker syncs[s] behind each, in one
    batched call (sma_compress_streams): a list of bytes.  heads: per stream the bytes copied
    verbatim in front (a header from write_header), or None for block runs."""
    streams = [([bytes(b) for b in blocks], [int(c) for c in counts]) for blocks, counts in streams]
    k = len(streams)
    if not k:
        return []
    if any(len(b) != len(c) for b, c in streams) or (heads is not None and len(heads) != k):
        raise ValueError("one count per block, one head per stream")
    marker = _syncs(syncs, k, True)
    heads = None if heads is None else [bytes(h) for h in heads]
    parts = [b for blocks, _ in streams for b in blocks]
    buf, offs, lens = lay_out(parts + (heads or []))
    nb = len(parts)
    first = exclusive_scan([len(b) for b, _ in streams], np.uint32, total=True)
    block_len = lens[:nb].astype(np.uint32)
    counts = np.array([c for _, cs in streams for c in cs], np.uint64)
    room = [(len(heads[s]) if heads else 0) + sum(lib().sma_max_block_length(len(b)) for b in streams[s][0]) for s in range(k)]
    out_off = exclusive_scan(room, total=True)
    out = np.empty(max(int(out_off[-1]), 1), np.uint8)
    out_len, status = np.zeros(k, np.uint64), np.zeros(k, np.int32)
    head_off = np.ascontiguousarray(offs[nb:]) if heads is not None else None
    head_len = np.ascontiguousarray(lens[nb:]) if heads is not None else None
    block_off = np.ascontiguousarray(offs[:nb])
    check(lib().sma_compress_streams(context(device), buf.ctypes.data, first.ctypes.data, block_off.ctypes.data,
                                     block_len.ctypes.data, counts.ctypes.data, marker.ctypes.data,
                                     None if head_off is None else head_off.ctypes.data,
                                     None if head_len is None else head_len.ctypes.data, k, out.ctypes.data,
                                     out_off.ctypes.data, out_len.ctypes.data, status.ctypes.data, _mode(mode)), AvroError)
    _raise_first(status.tolist())
    return collect(out, out_off, out_len)


def compress_avro(blocks, counts, schema, sync, meta=(), mode="fast", device=0):
    """A whole file: write_header(schema, sync, meta), then every block of `blocks` (serialized
    records; counts[i] objects each) compressed and checksummed on the device."""
    try:
        return compress_avro_streams([(blocks, counts)], [sync], heads=[write_header(schema, sync, meta)], mode=mode,
                                     device=device)[0]
    except AvroError as e:
        raise AvroError(e.code) from None


def find_sync(streams, syncs, queries, device=0):
    """The split rule on the device (sma_find_sync_device): for each query (stream, from) the
    position of the first occurrence of that stream's marker at or after `from`, else the stream's
    length.  The result plus 16 is where a block run starts."""
    import torch
    queries = list(queries)
    if not queries:
        return []
    buf, offs, lens = lay_out(streams)
    marker = _syncs(syncs, len(streams), True)
    dev = torch.device("cuda", device)
    i64 = lambda a: torch.from_numpy(np.asarray(a).astype(np.int64)).to(dev)
    d_in, d_sync = torch.from_numpy(buf.copy()).to(dev), torch.from_numpy(marker.copy()).to(dev)
    d_off, d_len = i64(offs), i64(lens)
    d_qs = torch.tensor([q[0] for q in queries], dtype=torch.int32, device=dev)
    d_qf = torch.tensor([q[1] for q in queries], dtype=torch.int64, device=dev)
    d_pos = torch.zeros(len(queries), dtype=torch.int64, device=dev)
    find_sync_device(d_in, d_off, d_len, d_sync, d_qs, d_qf, d_pos, device=device)
    return d_pos.cpu().tolist()


# ---- device API (torch tensors resident in HBM; asynchronous on `stream`) ---------------------

_device = device_caller(lib, context, AvroError)


def uncompress_avro_streams_device(d_in, d_in_off, d_in_len, max_blocks, max_fragments, d_out, d_out_off, d_out_cap, d_out_len,
                                   d_status, kind="file", d_sync=None, verify_crc=True, d_objects=None, d_block_first=None,
                                   d_block_status=None, d_blocks=None, stream=None, device=None):
    """sma_uncompress_streams_device: stream s = d_in[d_in_off[s] : d_in_off[s] + d_in_len[s]] decodes
    into d_out[d_out_off[s] : d_out_off[s] + d_out_cap[s]]; per stream d_out_len (int64), d_status
    (int32) and optionally d_objects (int64).  kind "blocks" takes d_sync, uint8[16 * nstreams].
    max_blocks bounds the blocks summed over the streams that are decoded; max_fragments (avro_plan's
    second total, or 0) lets blocks of more than 64 KiB decode by fragments.  Optional, both or
    neither: d_block_first int32[nstreams + 1], d_block_status int32[max_blocks].  Optional: d_blocks,
    a dict of tensors of max_blocks entries keyed as INDEX_KEYS (int64 for pay_off, count and out_off,
    int32 for the others), the block table.  Nothing is synchronised.
    Arguments are checked first (_binding.device_caller; README, Device API).
    Length not checked: d_sync, d_blocks, d_block_status."""
    _device("sma_uncompress_streams_device", d_out, device, stream, _kind(kind), d_in, d_in_off, d_in_len, d_sync,
            numel(d_in_len), int(max_blocks), int(max_fragments), 1 if verify_crc else 0, d_out, d_out_off, d_out_cap, d_out_len,
            d_status, d_objects, d_block_first, d_blocks, d_block_status)


def find_sync_device(d_in, d_in_off, d_in_len, d_sync, d_q_stream, d_q_from, d_pos, stream=None, device=None):
    """sma_find_sync_device: d_pos[i] (int64) = the first position at or after d_q_from[i] (int64) of
    stream d_q_stream[i] (int32) that holds the stream's marker d_sync[16 s : 16 s + 16], else the
    stream's length.  Nothing is synchronised.
    Arguments are checked first (_binding.device_caller; README, Device API).  Length not checked: d_sync."""
    _device("sma_find_sync_device", d_pos, device, stream, d_in, d_in_off, d_in_len, d_sync, numel(d_in_len), d_q_stream,
            d_q_from, numel(d_q_stream), d_pos)


def compress_avro_streams_device(d_in, d_block_first, d_block_off, d_block_len, d_block_count, d_sync, max_blocks, stage_bytes,
                                 max_fragments, d_out, d_out_off, d_out_len, d_status, d_head_off=None, d_head_len=None,
                                 mode="fast", stream=None, device=None):
    """sma_compress_streams_device: stream s is the blocks d_block_first[s] .. d_block_first[s + 1]
    (int32[nstreams + 1]) of d_block_off (int64), d_block_len (int32) and d_block_count (int64), the
    header d_in[d_head_off[s] : + d_head_len[s]] (int64, both or neither) copied in front, written to
    d_out[d_out_off[s]:], where the header's length plus the sum of max_block_length(len) is left for
    it.  max_blocks, stage_bytes (the sum of sma_stage_length) and max_fragments bound the batch.
    Nothing is synchronised.
    Arguments are checked first (_binding.device_caller; README, Device API).
    Length not checked: d_block_off, d_block_len, d_block_count, d_sync."""
    _device("sma_compress_streams_device", d_out, device, stream, d_in, d_block_first, d_block_off, d_block_len, d_block_count,
            d_sync, d_head_off, d_head_len, numel(d_out_off), int(max_blocks), int(stage_bytes), int(max_fragments), d_out,
            d_out_off, d_out_len, d_status, _mode(mode))


def last_indexed(device=0):
    """Diagnostic (sma_ctx_last_indexed): how many blocks the device's last decode call took by
    fragments (waits for the device); -1 before the first call."""
    return int(lib().sma_ctx_last_indexed(context(device)))


__all__ = ["AVRO_ABI_SYMBOLS", "MODES", "KINDS", "INDEX_KEYS", "MAGIC", "AvroError", "uncompress_avro", "uncompress_avro_streams",
           "compress_avro", "compress_avro_streams", "write_header", "find_sync", "find_sync_host", "index_avro",
           "length_uncompressed", "avro_plan", "max_blocks", "max_block_length", "uncompress_avro_streams_device",
           "find_sync_device", "compress_avro_streams_device", "last_indexed", "status_message", "version"]
