"""The compression-stream format of ORC files written with compress=SNAPPY over
include/snappy_mi355x_orc.h -- libsnappy_mi355x_orc.so, the companion of
libsnappy_mi355x_multi.so and libsnappy_mi355x.so.  A stream is a sequence of chunks, each a 3-byte
little-endian header and a payload that is a raw Snappy stream or, where compression did not pay,
the original bytes.  `block_size` is the file's compression block size (from its PostScript); the
caller supplies it and the streams' byte ranges -- no ORC metadata is parsed here.

    compress_orc(x, block_size) / uncompress_orc(x, block_size)   -> bytes   one stream (a batch of one)
    compress_orc_streams(xs, block_size)          -> list of bytes   many inputs, one batched call
    uncompress_orc_streams(xs, block_size)        -> list of bytes   many streams, one batched call
    index_chunks(x, block_size)                   -> (summary, arrays)  the host walk
    streams_plan(xs, block_size), max_chunks(n), max_length(n, block_size)   (host, no device)

and, on torch tensors resident in HBM: compress_orc_streams_device, uncompress_orc_streams_device
(no host synchronisation), last_indexed.

The package imports without this library; it is loaded on the first call here.  No CPU fallback:
every codec call needs the three HIP libraries and a device.
"""
import ctypes
import os

import numpy as np

from . import HERE, MODES, SnappyError, _in_arg, _mode
from ._binding import ORC, OrcChunks, Summary, check, collect, context_cache, device_caller, exclusive_scan, lay_out, load, numel

LIB_PATH = os.path.join(HERE, "libsnappy_mi355x_orc.so")

SMO_ERR_TRUNCATED = 64
SMO_ERR_CHUNK_TOO_LARGE = 65
HEADER_LENGTH = 3
MAX_BLOCK_SIZE = 0x7FFFFF
DEFAULT_BLOCK_SIZE = 262144  # the ORC writers' default compression block size
INDEX_KEYS = ("pay_off", "pay_len", "ulen", "original")  # smo_chunks' arrays, in its order

ORC_ABI_SYMBOLS = tuple(ORC)  # exported symbols of include/snappy_mi355x_orc.h (tests/test_orc_host.py)

_lib = None


def library_path():
    return LIB_PATH


def lib():
    """Load libsnappy_mi355x_orc.so (raises OSError if it was not built)."""
    global _lib
    if _lib is None:
        _lib = load(LIB_PATH, ORC, "libsnappy_mi355x_orc.so not built (run __graft_entry__.build())")
    return _lib


def status_message(code):
    return lib().smo_status_message(int(code)).decode()


def version():
    return lib().smo_version().decode()


class OrcError(SnappyError):
    """A SnappyError whose message comes from smo_status_message (the SMO_ERR_* texts too); for a
    stream of a batch `stream` is its number in the batch, else None."""

    def __init__(self, code, stream=None):
        super().__init__(code, status_message(code))
        self.stream = stream


# context(device=0): the per-device smo_ctx (an smm_ctx of its own plus scratch)
_ctx, _ctx_lock, context = context_cache(lib, "smo_ctx_create", SnappyError,
                                         "no usable HIP device %d for snappy_mi355x_orc")


def _block_size(block_size):
    block_size = int(block_size)
    if not 1 <= block_size <= MAX_BLOCK_SIZE:
        raise ValueError("block_size must lie in 1 .. 0x7fffff")
    return block_size


# ---- host helpers (no device) ---------------------------------------------------------------

def max_length(n, block_size=DEFAULT_BLOCK_SIZE):
    """smo_max_length: the room the encoder needs for an n-byte input, n + 3 * ceil(n / block_size)."""
    return lib().smo_max_length(int(n), _block_size(block_size))


def max_chunks(n):
    """smo_max_chunks: the most chunks an n-byte stream can hold (3 bytes each at the least)."""
    return lib().smo_max_chunks(int(n))


def index_chunks(data, block_size=DEFAULT_BLOCK_SIZE, max_chunks=None):
    """The host walk (smo_index): (Summary, dict of numpy arrays pay_off / pay_len / ulen / original
    of the chunks).  max_chunks=None sizes the arrays by a counting walk first.  The block size is
    passed as it is: out of range the summary's status is SM_ERR_ARGUMENT."""
    src, n, keep = _in_arg(data)
    bs = int(block_size)
    s = Summary()
    if max_chunks is None:
        s.status = lib().smo_index(src, n, bs, None, 0, ctypes.byref(s))
        max_chunks = s.nchunks
    arrays = {"pay_off": np.zeros(max_chunks, np.uint64), "pay_len": np.zeros(max_chunks, np.uint32),
              "ulen": np.zeros(max_chunks, np.uint32), "original": np.zeros(max_chunks, np.uint8)}
    ch = OrcChunks(*(arrays[k].ctypes.data for k in INDEX_KEYS))
    s.status = lib().smo_index(src, n, bs, ctypes.byref(ch), max_chunks, ctypes.byref(s))
    return s, arrays


def length_uncompressed(data, block_size=DEFAULT_BLOCK_SIZE):
    """The stream's total uncompressed length from its chunk headers and varints (no device)."""
    src, n, keep = _in_arg(data)
    res = ctypes.c_size_t(0)
    check(lib().smo_uncompressed_length(src, n, int(block_size), ctypes.byref(res)), OrcError)
    return res.value


def streams_plan(streams, block_size=DEFAULT_BLOCK_SIZE, out_cap=None, max_chunks=0x7FFFFFFF):
    """smo_streams_plan, the device's decode plan on the host, for a list of streams: (rc, first,
    out_len, status, total_chunks, total_fragments) -- per stream what is known before any byte is
    decoded (the walk's error, SM_BUFFER_TOO_SMALL against out_cap[s], or 0), the size needed, the
    exclusive scan of the slots (len(streams) + 1 entries), and the device call's two bounds."""
    buf, offs, lens = lay_out(streams)
    k = len(streams)
    cap = None if out_cap is None else np.ascontiguousarray(out_cap, dtype=np.uint64)
    first, out_len, status = np.zeros(k + 1, np.uint32), np.zeros(k, np.uint64), np.zeros(k, np.int32)
    chunks, fragments = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = lib().smo_streams_plan(buf.ctypes.data, offs.ctypes.data, lens.ctypes.data, k, int(block_size),
                                None if cap is None else cap.ctypes.data, int(max_chunks), first.ctypes.data,
                                out_len.ctypes.data, status.ctypes.data, ctypes.byref(chunks), ctypes.byref(fragments))
    return int(rc), first, out_len, status, chunks.value, fragments.value


# ---- host buffers -----------------------------------------------------------------------

def _raise_first(codes):
    for s, code in enumerate(codes):
        if code:
            raise OrcError(code, s)


def compress_orc_streams(datas, block_size=DEFAULT_BLOCK_SIZE, mode="fast", device=0):
    """Every buffer of `datas` as a stream of its own in one batched call (smo_compress_streams): a
    list of bytes.  The input is cut into pieces of block_size bytes, each one chunk holding
    compress(piece, mode) where that is shorter than the piece, else the piece itself."""
    datas = list(datas)
    bs = _block_size(block_size)
    if not datas:
        return []
    buf, offs, lens = lay_out(datas)
    out_off = exclusive_scan([lib().smo_max_length(int(n), bs) for n in lens], total=True)
    out = np.empty(max(int(out_off[-1]), 1), np.uint8)
    out_len, status = np.zeros(len(datas), np.uint64), np.zeros(len(datas), np.int32)
    check(lib().smo_compress_streams(context(device), bs, buf.ctypes.data, offs.ctypes.data, lens.ctypes.data, len(datas),
                                     out.ctypes.data, out_off.ctypes.data, out_len.ctypes.data, status.ctypes.data,
                                     _mode(mode)), OrcError)
    _raise_first(status.tolist())
    return collect(out, out_off, out_len)


def uncompress_orc_streams(streams, block_size=DEFAULT_BLOCK_SIZE, device=0, statuses=False):
    """Decode a list of streams in one batched call (smo_uncompress_streams): a list of bytes.  A
    failing stream raises OrcError (the first failing stream's status, its number as `.stream`);
    with statuses=True nothing is raised and the result is (list of bytes, or None for a failing
    stream; list of statuses)."""
    streams = list(streams)
    bs = _block_size(block_size)
    if not streams:
        return ([], []) if statuses else []
    buf, offs, lens = lay_out(streams)
    k = len(streams)
    _, _, need, pre, _, _ = streams_plan(streams, bs)
    cap = np.where(pre == 0, need, 0).astype(np.uint64)
    out_off = exclusive_scan(cap, total=True)
    out = np.empty(max(int(out_off[-1]), 1), np.uint8)
    out_len, status = np.zeros(k, np.uint64), np.zeros(k, np.int32)
    check(lib().smo_uncompress_streams(context(device), bs, buf.ctypes.data, offs.ctypes.data, lens.ctypes.data, k,
                                       out.ctypes.data, out_off.ctypes.data, cap.ctypes.data, out_len.ctypes.data,
                                       status.ctypes.data), OrcError)
    codes = status.tolist()
    if not statuses:
        _raise_first(codes)
    res = collect(out, out_off, out_len, codes)
    return (res, codes) if statuses else res


def _one(call, data, block_size, **kw):
    try:
        return call([data], block_size, **kw)[0]
    except OrcError as e:
        raise OrcError(e.code) from None  # (a stream alone has no number)


def compress_orc(data, block_size=DEFAULT_BLOCK_SIZE, mode="fast", device=0):
    """`data` as an ORC compression stream: per piece of block_size bytes one chunk, compressed or stored."""
    return _one(compress_orc_streams, data, block_size, mode=mode, device=device)


def uncompress_orc(data, block_size=DEFAULT_BLOCK_SIZE, device=0):
    return _one(uncompress_orc_streams, data, block_size, device=device)


# ---- device API (torch tensors resident in HBM; asynchronous on `stream`) ---------------------

_device = device_caller(lib, context, OrcError)


def compress_orc_streams_device(block_size, d_in, d_in_off, d_in_len, max_pieces, d_out, d_out_off, d_out_len, d_status,
                                mode="fast", stream=None, device=None):
    """smo_compress_streams_device: input s = d_in[d_in_off[s] : d_in_off[s] + d_in_len[s]] becomes one
    stream at d_out[d_out_off[s]:], where max_length(d_in_len[s], block_size) bytes are left for it.
    d_in / d_out uint8, d_in_off / d_in_len / d_out_off / d_out_len int64[nstreams], d_status
    int32[nstreams]; max_pieces bounds the sum of ceil(d_in_len[s] / block_size).  Nothing is synchronised.
    Arguments are checked first (_binding.device_caller; README, Device API)."""
    _device("smo_compress_streams_device", d_out, device, stream, int(block_size), d_in, d_in_off, d_in_len,
            numel(d_in_len), int(max_pieces), d_out, d_out_off, d_out_len, d_status, _mode(mode))


def uncompress_orc_streams_device(block_size, d_in, d_in_off, d_in_len, max_chunks, max_fragments, d_out, d_out_off,
                                  d_out_cap, d_out_len, d_status, d_chunk_first=None, d_chunk_status=None, stream=None,
                                  device=None):
    """smo_uncompress_streams_device: stream s = d_in[d_in_off[s] : d_in_off[s] + d_in_len[s]] decodes
    into d_out[d_out_off[s] : d_out_off[s] + d_out_cap[s]]; per stream d_out_len (int64) and d_status
    (int32).  max_chunks bounds the chunks summed over the streams that are decoded; max_fragments
    (streams_plan's second total, or 0) lets compressed chunks of more than 64 KiB decode by
    fragments.  Optional, both or neither: d_chunk_first int32[nstreams + 1], d_chunk_status
    int32[max_chunks].  Nothing is synchronised.
    Arguments are checked first (_binding.device_caller; README, Device API).  Length not checked: d_chunk_status."""
    _device("smo_uncompress_streams_device", d_out, device, stream, int(block_size), d_in, d_in_off, d_in_len,
            numel(d_in_len), int(max_chunks), int(max_fragments), d_out, d_out_off, d_out_cap, d_out_len, d_status,
            d_chunk_first, d_chunk_status)


def last_indexed(device=0):
    """Diagnostic (smo_ctx_last_indexed): how many chunks the device's last decode call took by
    fragments (waits for the device); -1 before the first call."""
    return int(lib().smo_ctx_last_indexed(context(device)))


__all__ = ["ORC_ABI_SYMBOLS", "MODES", "OrcError", "DEFAULT_BLOCK_SIZE", "MAX_BLOCK_SIZE", "compress_orc", "uncompress_orc",
           "compress_orc_streams", "uncompress_orc_streams", "index_chunks", "length_uncompressed", "streams_plan",
           "max_chunks", "max_length", "compress_orc_streams_device", "uncompress_orc_streams_device", "last_indexed",
           "status_message", "version"]
