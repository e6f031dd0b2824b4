"""The two length-prefixed block containers around raw Snappy streams over
include/snappy_mi355x_blocks.h -- libsnappy_mi355x_blocks.so, the companion of
libsnappy_mi355x_multi.so and libsnappy_mi355x.so:

    "hadoop"  what Hadoop's SnappyCodec / BlockCompressorStream write (.snappy part-files of
              MapReduce, Hive and Spark text output, SequenceFile blocks)
    "xerial"  what snappy-java's SnappyOutputStream writes (Kafka's Snappy record batches)

    compress_hadoop(x) / uncompress_hadoop(x)   -> bytes   one stream (a batch of one)
    compress_xerial(x) / uncompress_xerial(x)   -> bytes
    compress_block_streams(xs, format)          -> list of bytes   many inputs, one batched call
    uncompress_block_streams(xs, format)        -> list of bytes   many streams, one batched call
    index_blocks(x, format)                     -> (summary, arrays)  the host walk
    streams_plan(xs, format), max_chunks(n, format), max_length(n, format)   (host, no device)

and, on torch tensors resident in HBM: compress_block_streams_device, uncompress_block_streams_device
(no host synchronisation), last_indexed.

The package imports without this library; it is loaded on the first call here.  No CPU fallback:
every codec call needs the three HIP libraries and a device.
"""
import ctypes
import os

import numpy as np

from . import HERE, MODES, SnappyError, _in_arg, _mode
from ._binding import BLOCKS, BlockChunks, Summary, check, collect, context_cache, device_caller, exclusive_scan, lay_out, load, numel

LIB_PATH = os.path.join(HERE, "libsnappy_mi355x_blocks.so")

FORMATS = {"hadoop": 0, "xerial": 1}
SMB_ERR_NO_HEADER = 56
SMB_ERR_BAD_HEADER = 57
SMB_ERR_TRUNCATED = 58
SMB_ERR_CHUNK_TOO_LARGE = 59
SMB_ERR_BLOCK_LENGTH = 60
XERIAL_MAGIC = b"\x82SNAPPY\x00"
XERIAL_HEADER = XERIAL_MAGIC + b"\x00\x00\x00\x01\x00\x00\x00\x01"
INDEX_KEYS = ("pay_off", "pay_len", "ulen")  # smb_chunks' arrays, in its order

BLOCKS_ABI_SYMBOLS = tuple(BLOCKS)  # exported symbols of include/snappy_mi355x_blocks.h (tests/test_blocks_host.py)

_lib = None


def library_path():
    return LIB_PATH


def lib():
    """Load libsnappy_mi355x_blocks.so (raises OSError if it was not built)."""
    global _lib
    if _lib is None:
        _lib = load(LIB_PATH, BLOCKS, "libsnappy_mi355x_blocks.so not built (run __graft_entry__.build())")
    return _lib


def status_message(code):
    return lib().smb_status_message(int(code)).decode()


def version():
    return lib().smb_version().decode()


class BlocksError(SnappyError):
    """A SnappyError whose message comes from smb_status_message (the SMB_ERR_* texts too); for a
    stream of a batch `stream` is its number in the batch, else None."""

    def __init__(self, code, stream=None):
        super().__init__(code, status_message(code))
        self.stream = stream


# context(device=0): the per-device smb_ctx (an smm_ctx of its own plus scratch)
_ctx, _ctx_lock, context = context_cache(lib, "smb_ctx_create", SnappyError,
                                         "no usable HIP device %d for snappy_mi355x_blocks")


def _format(format):
    if format not in FORMATS:
        raise ValueError("format must be 'hadoop' or 'xerial'")
    return FORMATS[format]


# ---- host helpers (no device) ---------------------------------------------------------------

def max_length(n, format):
    """smb_max_length: the room the encoder needs for an n-byte input."""
    return lib().smb_max_length(int(n), _format(format))


def max_chunks(n, format):
    """smb_max_chunks: the most chunks an n-byte stream can hold (5 bytes each at the least)."""
    return lib().smb_max_chunks(int(n), _format(format))


def index_blocks(data, format, max_chunks=None):
    """The host walk (smb_index): (Summary, dict of numpy arrays pay_off / pay_len / ulen of the
    chunks).  max_chunks=None sizes the arrays by a counting walk first."""
    src, n, keep = _in_arg(data)
    f = _format(format)
    s = Summary()
    if max_chunks is None:
        lib().smb_index(src, n, f, None, 0, ctypes.byref(s))
        max_chunks = s.nchunks
    arrays = {"pay_off": np.zeros(max_chunks, np.uint64), "pay_len": np.zeros(max_chunks, np.uint32),
              "ulen": np.zeros(max_chunks, np.uint32)}
    ch = BlockChunks(*(arrays[k].ctypes.data for k in INDEX_KEYS))
    lib().smb_index(src, n, f, ctypes.byref(ch), max_chunks, ctypes.byref(s))
    return s, arrays


def length_uncompressed(data, format):
    """The stream's total uncompressed length from its length fields and varints (no device)."""
    src, n, keep = _in_arg(data)
    res = ctypes.c_size_t(0)
    check(lib().smb_uncompressed_length(src, n, _format(format), ctypes.byref(res)), BlocksError)
    return res.value


def streams_plan(streams, format, out_cap=None, max_chunks=0x7FFFFFFF):
    """smb_streams_plan, the device's decode plan on the host, for a list of streams: (rc, first,
    out_len, status, total_chunks, total_fragments) -- per stream what is known before any byte is
    decoded (the walk's error, SM_BUFFER_TOO_SMALL against out_cap[s], or 0), the size needed, the
    exclusive scan of the slots (len(streams) + 1 entries), and the device call's two bounds."""
    buf, offs, lens = lay_out(streams)
    k = len(streams)
    cap = None if out_cap is None else np.ascontiguousarray(out_cap, dtype=np.uint64)
    first, out_len, status = np.zeros(k + 1, np.uint32), np.zeros(k, np.uint64), np.zeros(k, np.int32)
    chunks, fragments = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = lib().smb_streams_plan(buf.ctypes.data, offs.ctypes.data, lens.ctypes.data, k, _format(format),
                                None if cap is None else cap.ctypes.data, int(max_chunks), first.ctypes.data,
                                out_len.ctypes.data, status.ctypes.data, ctypes.byref(chunks), ctypes.byref(fragments))
    return int(rc), first, out_len, status, chunks.value, fragments.value


# ---- host buffers -----------------------------------------------------------------------

def _raise_first(codes):
    for s, code in enumerate(codes):
        if code:
            raise BlocksError(code, s)


def compress_block_streams(datas, format, mode="fast", device=0):
    """Every buffer of `datas` as a stream of its own in one batched call (smb_compress_streams): a
    list of bytes.  The input is cut into 64 KiB pieces, each one chunk holding compress(piece, mode);
    in "hadoop" every piece is a block of its own."""
    datas = list(datas)
    f = _format(format)
    if not datas:
        return []
    buf, offs, lens = lay_out(datas)
    out_off = exclusive_scan([lib().smb_max_length(int(n), f) for n in lens], total=True)
    out = np.empty(max(int(out_off[-1]), 1), np.uint8)
    out_len, status = np.zeros(len(datas), np.uint64), np.zeros(len(datas), np.int32)
    check(lib().smb_compress_streams(context(device), f, buf.ctypes.data, offs.ctypes.data, lens.ctypes.data, len(datas),
                                     out.ctypes.data, out_off.ctypes.data, out_len.ctypes.data, status.ctypes.data,
                                     _mode(mode)), BlocksError)
    _raise_first(status.tolist())
    return collect(out, out_off, out_len)


def uncompress_block_streams(streams, format, device=0, statuses=False):
    """Decode a list of streams in one batched call (smb_uncompress_streams): a list of bytes.  A
    failing stream raises BlocksError (the first failing stream's status, its number as `.stream`);
    with statuses=True nothing is raised and the result is (list of bytes, or None for a failing
    stream; list of statuses)."""
    streams = list(streams)
    f = _format(format)
    if not streams:
        return ([], []) if statuses else []
    buf, offs, lens = lay_out(streams)
    k = len(streams)
    _, _, need, pre, _, _ = streams_plan(streams, format)
    cap = np.where(pre == 0, need, 0).astype(np.uint64)
    out_off = exclusive_scan(cap, total=True)
    out = np.empty(max(int(out_off[-1]), 1), np.uint8)
    out_len, status = np.zeros(k, np.uint64), np.zeros(k, np.int32)
    check(lib().smb_uncompress_streams(context(device), f, buf.ctypes.data, offs.ctypes.data, lens.ctypes.data, k,
                                       out.ctypes.data, out_off.ctypes.data, cap.ctypes.data, out_len.ctypes.data,
                                       status.ctypes.data), BlocksError)
    codes = status.tolist()
    if not statuses:
        _raise_first(codes)
    res = collect(out, out_off, out_len, codes)
    return (res, codes) if statuses else res


def _one(call, data, format, **kw):
    try:
        return call([data], format, **kw)[0]
    except BlocksError as e:
        raise BlocksError(e.code) from None  # (a stream alone has no number)


def compress_hadoop(data, mode="fast", device=0):
    """`data` as a Hadoop block stream: per 64 KiB piece its length, then one chunk."""
    return _one(compress_block_streams, data, "hadoop", mode=mode, device=device)


def uncompress_hadoop(data, device=0):
    return _one(uncompress_block_streams, data, "hadoop", device=device)


def compress_xerial(data, mode="fast", device=0):
    """`data` as a snappy-java stream: the 16-byte header, then one chunk per 64 KiB piece."""
    return _one(compress_block_streams, data, "xerial", mode=mode, device=device)


def uncompress_xerial(data, device=0):
    return _one(uncompress_block_streams, data, "xerial", device=device)


# ---- device API (torch tensors resident in HBM; asynchronous on `stream`) ---------------------

_device = device_caller(lib, context, BlocksError)


def compress_block_streams_device(format, d_in, d_in_off, d_in_len, max_blocks, d_out, d_out_off, d_out_len, d_status,
                                  mode="fast", stream=None, device=None):
    """smb_compress_streams_device: input s = d_in[d_in_off[s] : d_in_off[s] + d_in_len[s]] becomes one
    stream at d_out[d_out_off[s]:], where max_length(d_in_len[s], format) bytes are left for it.  d_in /
    d_out uint8, d_in_off / d_in_len / d_out_off / d_out_len int64[nstreams], d_status int32[nstreams];
    max_blocks bounds the sum of ceil(d_in_len[s] / 65536).  Nothing is synchronised.
    Arguments are checked first (_binding.device_caller; README, Device API)."""
    _device("smb_compress_streams_device", d_out, device, stream, _format(format), d_in, d_in_off, d_in_len,
            numel(d_in_len), int(max_blocks), d_out, d_out_off, d_out_len, d_status, _mode(mode))


def uncompress_block_streams_device(format, d_in, d_in_off, d_in_len, max_chunks, max_fragments, d_out, d_out_off,
                                    d_out_cap, d_out_len, d_status, d_chunk_first=None, d_chunk_status=None, stream=None,
                                    device=None):
    """smb_uncompress_streams_device: stream s = d_in[d_in_off[s] : d_in_off[s] + d_in_len[s]] decodes
    into d_out[d_out_off[s] : d_out_off[s] + d_out_cap[s]]; per stream d_out_len (int64) and d_status
    (int32).  max_chunks bounds the chunks summed over the streams that are decoded; max_fragments
    (streams_plan's second total, or 0) lets chunks of more than 64 KiB decode by fragments.
    Optional, both or neither: d_chunk_first int32[nstreams + 1], d_chunk_status int32[max_chunks].
    Nothing is synchronised.
    Arguments are checked first (_binding.device_caller; README, Device API).  Length not checked: d_chunk_status."""
    _device("smb_uncompress_streams_device", d_out, device, stream, _format(format), d_in, d_in_off, d_in_len,
            numel(d_in_len), int(max_chunks), int(max_fragments), d_out, d_out_off, d_out_cap, d_out_len, d_status,
            d_chunk_first, d_chunk_status)


def last_indexed(device=0):
    """Diagnostic (smb_ctx_last_indexed): how many chunks the device's last decode call took by
    fragments (waits for the device); -1 before the first call."""
    return int(lib().smb_ctx_last_indexed(context(device)))


__all__ = ["BLOCKS_ABI_SYMBOLS", "MODES", "FORMATS", "BlocksError", "XERIAL_MAGIC", "XERIAL_HEADER", "compress_hadoop",
           "uncompress_hadoop", "compress_xerial", "uncompress_xerial", "compress_block_streams",
           "uncompress_block_streams", "index_blocks", "length_uncompressed", "streams_plan", "max_chunks", "max_length",
           "compress_block_streams_device", "uncompress_block_streams_device", "last_indexed"]
