"""The Snappy framing format (framing_format.txt of google/snappy: .sz files, snzip, Go's
snappy.Writer) over include/snappy_mi355x_framing.h -- libsnappy_mi355x_framing.so, the companion
of libsnappy_mi355x.so.

    compress_framed(x)           -> bytes   identifier + one chunk per 64 KiB block, CRC-32C each
    uncompress_framed(x)         -> bytes   CRC-checked; raises SnappyError
    length_uncompressed_framed(x) -> int    from the chunk headers alone (host, no device)
    validate_framed(x)           -> status  what uncompress_framed would raise with, or 0
    index_framed(x)              -> (summary, arrays)  the host chunk walker
    seek_index_framed(x)         -> FramedIndex  the walker's arrays plus chunk_off
    compress_framed(x, return_index=True) -> (bytes, FramedIndex)  the encoder's own index
    uncompress_framed_range(x, lo, length)  -> bytes   only the touched chunks are decoded
    uncompress_framed_ranges(x, ranges)     -> (list of bytes, statuses)  one batched call
    compress_framed_streams(xs)             -> list of bytes   many inputs, one batched call
    uncompress_framed_streams(xs)           -> list of bytes   many streams, one batched call
    streams_plan(xs), max_data_chunks(n)    the batched decode's plan and chunk bound (host)

and, on torch tensors resident in HBM: crc32c_batch_device, compress_framed_device,
index_framed_device, uncompressed_length_framed_device, uncompress_chunks_device,
uncompress_framed_device, compress_framed_indexed_device, chunk_offsets_device,
uncompress_ranges_device, compress_framed_streams_device, uncompress_framed_streams_device.

The package imports without this library; it is loaded on the first call here.  No CPU
fallback: every codec call needs both HIP libraries and a device.
"""
import ctypes
import os

import numpy as np

from . import HERE, MODES, SnappyError, _in_arg, _mode, _out_buffer
from ._binding import (FRAMING, FRAMING_RANGE, FRAMING_STREAMS, INDEX_KEYS, Chunks, Summary, check, collect,
                       context_cache, device_caller, exclusive_scan, field_dtypes, load, numel)
from ._binding import lay_out as _lay_out

LIB_PATH = os.path.join(HERE, "libsnappy_mi355x_framing.so")

SMF_ERR_NO_IDENTIFIER = 48
SMF_ERR_BAD_IDENTIFIER = 49
SMF_ERR_RESERVED_CHUNK = 50
SMF_ERR_TRUNCATED = 51
SMF_ERR_CHUNK_TOO_LARGE = 52
SMF_ERR_CRC = 53
IDENTIFIER = b"\xff\x06\x00\x00sNaPpY"

# exported symbols of include/snappy_mi355x_framing.h (checked by tests/test_framing_host.py), among
# them the seek index and the ranged decode (tests/test_framing_range_host.py) and a batch of
# streams per call (tests/test_framing_streams_host.py)
FRAMING_ABI_SYMBOLS = tuple(FRAMING)
RANGE_ABI_SYMBOLS = tuple(FRAMING_RANGE)
STREAMS_ABI_SYMBOLS = tuple(FRAMING_STREAMS)

# the index arrays' element types (Chunks.elements): as the C ABI declares them, and as torch tensors
# hold the same bits
_UNSIGNED = field_dtypes(Chunks)
_SIGNED = field_dtypes(Chunks, signed=True)

_lib = None


def library_path():
    return LIB_PATH


def lib():
    """Load libsnappy_mi355x_framing.so (raises OSError if it was not built)."""
    global _lib
    if _lib is None:
        _lib = load(LIB_PATH, FRAMING, "libsnappy_mi355x_framing.so not built (run __graft_entry__.build())")
    return _lib


def status_message(code):
    return lib().smf_status_message(int(code)).decode()


def version():
    return lib().smf_version().decode()


class FramingError(SnappyError):
    """A SnappyError whose message comes from smf_status_message (the SMF_ERR_* texts too)."""

    def __init__(self, code):
        super().__init__(code, status_message(code))


# context(device=0): the per-device smf_ctx (an sm_ctx of its own plus scratch)
_ctx, _ctx_lock, context = context_cache(lib, "smf_ctx_create", SnappyError,
                                         "no usable HIP device %d for snappy_mi355x_framing")


def max_framed_length(n):
    """10 + 8 * ceil(n / 65536) + n: the identifier, a header and a CRC per block, the bytes."""
    return lib().smf_max_framed_length(int(n))


def crc32c(data):
    """CRC-32C of a host buffer on the host (the bytewise table), unmasked."""
    src, n, keep = _in_arg(data)
    return lib().smf_crc32c(src, n)


def mask_crc(crc):
    return lib().smf_crc32c_mask(int(crc))


# ---- host buffers -----------------------------------------------------------------------

def index_framed(data, max_chunks=None):
    """The host chunk walker (smf_index): (Summary, dict of numpy arrays type / pay_off / pay_len /
    crc / ulen of the data chunks).  max_chunks=None sizes the arrays by a counting walk first."""
    src, n, keep = _in_arg(data)
    s = Summary()
    if max_chunks is None:
        lib().smf_index(src, n, None, 0, ctypes.byref(s))
        max_chunks = s.nchunks
    arrays = {k: np.zeros(max_chunks, _UNSIGNED[k]) for k in INDEX_KEYS}
    ch = Chunks(*(arrays[k].ctypes.data for k in INDEX_KEYS))
    lib().smf_index(src, n, ctypes.byref(ch), max_chunks, ctypes.byref(s))
    return s, arrays


class FramedIndex:
    """The seek index of a framed stream: numpy arrays type / pay_off / pay_len / crc / ulen, one
    entry per data chunk, and chunk_off (nchunks + 1, the exclusive scan of ulen: chunk c holds
    bytes [chunk_off[c], chunk_off[c + 1]) of the content)."""

    def __init__(self, arrays, chunk_off):
        for k in INDEX_KEYS:
            setattr(self, k, np.ascontiguousarray(arrays[k]))
        self.chunk_off = np.ascontiguousarray(chunk_off, dtype=np.uint64)

    @property
    def nchunks(self):
        return self.chunk_off.size - 1

    @property
    def total_length(self):
        return int(self.chunk_off[-1])

    def arrays(self):
        return {k: getattr(self, k) for k in INDEX_KEYS}

    def _struct(self):
        return Chunks(*(getattr(self, k).ctypes.data for k in INDEX_KEYS))


def chunk_offsets(ulen):
    """smf_chunk_offsets: the exclusive scan of ulen, with the total as the last entry (uint64)."""
    ulen = np.ascontiguousarray(ulen, dtype=np.uint32)
    off = np.zeros(ulen.size + 1, np.uint64)
    check(lib().smf_chunk_offsets(ulen.ctypes.data, ulen.size, off.ctypes.data), FramingError)
    return off


def seek_index_framed(data):
    """index_framed plus chunk_off, as a FramedIndex; raises SnappyError with the walk's
    structural error."""
    s, arrays = index_framed(data)
    check(s.status, FramingError)
    return FramedIndex(arrays, chunk_offsets(arrays["ulen"]))


def range_chunk_count(lo, length):
    """smf_range_chunk_count: the chunks bytes [lo, lo + length) touch in a stream of this
    library's encoder (a foreign stream may have smaller chunks: see range_plan)."""
    return lib().smf_range_chunk_count(int(lo), int(length))


def range_plan(index, n, ranges, max_range_chunks=0xFFFFFFFF):
    """smf_range_plan, the device's plan on the host: (rc, first, count, status, total) for the
    (lo, length) pairs `ranges` over `index` (a FramedIndex) of an n-byte framed stream."""
    lo = np.array([r[0] for r in ranges], dtype=np.uint64)
    ln = np.array([r[1] for r in ranges], dtype=np.uint64)
    first, count = np.zeros(lo.size, np.uint32), np.zeros(lo.size, np.uint32)
    status = np.zeros(lo.size, np.int32)
    total = ctypes.c_uint64(0)
    ch = index._struct()
    rc = lib().smf_range_plan(ctypes.byref(ch), index.chunk_off.ctypes.data, index.nchunks, int(n), lo.ctypes.data,
                              ln.ctypes.data, lo.size, int(max_range_chunks), first.ctypes.data, count.ctypes.data,
                              status.ctypes.data, ctypes.byref(total))
    return int(rc), first, count, status, total.value


def length_uncompressed_framed(data):
    """The stream's total uncompressed length from its chunk headers (no device, no CRC check)."""
    src, n, keep = _in_arg(data)
    res = ctypes.c_size_t(0)
    check(lib().smf_uncompressed_length(src, n, ctypes.byref(res)), FramingError)
    return res.value


def compress_framed(data, mode="fast", device=0, return_index=False):
    """Frame `data`: the stream identifier, then one chunk per 64 KiB block -- compressed (0x00)
    iff its Snappy stream is strictly shorter than the block, else uncompressed (0x01) -- each
    with the masked CRC-32C of its uncompressed bytes.  Computed on the GPU.  return_index=True:
    (bytes, FramedIndex), the index being the encoder's own (smf_compress_indexed_device)."""
    if return_index:
        return _compress_framed_indexed(data, mode, device)
    src, n, keep = _in_arg(data)
    cap = 10 + 8 * ((n + 65535) // 65536) + n
    ptr, buf = _out_buffer(cap)
    ol = ctypes.c_size_t(cap)
    st = lib().smf_compress(context(device), src, n, ptr, ctypes.byref(ol), _mode(mode))
    if st:
        raise FramingError(st)
    return ctypes.string_at(ptr, ol.value)


def uncompress_framed(data, device=0):
    """Decode a framed stream on the GPU, every chunk's CRC-32C checked; raises SnappyError with
    the first failing chunk's status (structure, the raw decoder's code, or SMF_ERR_CRC)."""
    size = length_uncompressed_framed(data)
    src, n, keep = _in_arg(data)
    ptr, buf = _out_buffer(size)
    ol = ctypes.c_size_t(size)
    st = lib().smf_uncompress(context(device), src, n, ptr, ctypes.byref(ol))
    if st:
        raise FramingError(st)
    return ctypes.string_at(ptr, ol.value)


def _upload(data, dev):
    """(the bytes of `data` as a uint8 tensor on dev, their count)."""
    import torch
    src, n, keep = _in_arg(data)
    host = np.frombuffer(ctypes.string_at(src, n), np.uint8) if n else np.zeros(0, np.uint8)
    return torch.from_numpy(host.copy()).to(dev), n


def _compress_framed_indexed(data, mode, device):
    import torch
    dev = "cuda:%d" % device
    d_in, n = _upload(data, dev)
    nblk = (n + 65535) // 65536
    d_out = torch.empty(10 + 8 * nblk + n, dtype=torch.uint8, device=dev)
    d_len = torch.zeros(1, dtype=torch.int64, device=dev)
    d_st = torch.zeros(1, dtype=torch.int32, device=dev)
    arrays, d_off = device_chunks(nblk, device), torch.zeros(nblk + 1, dtype=torch.int64, device=dev)
    d_nc = torch.zeros(1, dtype=torch.int32, device=dev)
    compress_framed_indexed_device(d_in, d_out, d_len, d_st, arrays, d_off, d_nc, mode=mode)
    check(int(d_st.item()), FramingError)
    nc = int(d_nc.item())
    index = FramedIndex({k: arrays[k][:nc].cpu().numpy().view(_UNSIGNED[k]) for k in INDEX_KEYS},
                        d_off[:nc + 1].cpu().numpy().view(np.uint64))
    return d_out[:int(d_len.item())].cpu().numpy().tobytes(), index


def uncompress_framed_range(data, lo, length, index=None, device=0):
    """Bytes [lo, lo + length) of the framed stream's content; only the chunks they touch are
    uploaded, decoded and CRC-checked.  index=None: the stream is walked on the host
    (smf_uncompress_range), and a structural error anywhere in it is raised; with a FramedIndex
    (from compress_framed(..., return_index=True) or seek_index_framed) nothing is walked."""
    if index is not None:
        out, st = uncompress_framed_ranges(data, [(lo, length)], index=index, device=device)
        check(int(st[0]), FramingError)
        return out[0]
    if int(lo) + int(length) > length_uncompressed_framed(data):  # (before any room is made for it)
        raise FramingError(33)
    src, n, keep = _in_arg(data)
    ptr, buf = _out_buffer(int(length))
    ol = ctypes.c_size_t(int(length))
    check(lib().smf_uncompress_range(context(device), src, n, int(lo), int(length), ptr, ctypes.byref(ol)), FramingError)
    return ctypes.string_at(ptr, ol.value)


def uncompress_framed_ranges(data, ranges, index=None, device=0):
    """One batched ranged decode (smf_uncompress_ranges_device) of the (lo, length) pairs
    `ranges`: (list of bytes, int32 array of statuses); a failing range gives b"" and its status.
    index=None walks the stream on the host first (raises on a structural error)."""
    import torch
    if index is None:
        index = seek_index_framed(data)
    dev = "cuda:%d" % device
    ranges = [(int(lo), int(ln)) for lo, ln in ranges]
    if not ranges:
        return [], np.zeros(0, np.int32)
    d_in, n = _upload(data, dev)
    rc, _, count, status, total = range_plan(index, n, ranges)
    arrays = {k: torch.from_numpy(getattr(index, k).view(_SIGNED[k])).to(dev) for k in INDEX_KEYS}
    d_off = torch.from_numpy(index.chunk_off.view(np.int64)).to(dev)
    # outputs behind one another, each at a 16-byte boundary; a range that leaves the stream is
    # rejected before anything is written and gets no room
    room = [ln if lo + ln <= index.total_length else 0 for lo, ln in ranges]
    out_off = exclusive_scan([(r + 15) // 16 * 16 for r in room], np.int64, total=True)
    d_out = torch.empty(max(int(out_off[-1]), 1), dtype=torch.uint8, device=dev)
    d_lo = torch.tensor(np.array([r[0] for r in ranges], np.uint64).view(np.int64), device=dev)
    d_ln = torch.tensor(np.array([r[1] for r in ranges], np.uint64).view(np.int64), device=dev)
    d_oo = torch.from_numpy(out_off[:-1].copy()).to(dev)
    d_ol = torch.zeros(len(ranges), dtype=torch.int64, device=dev)
    d_st = torch.zeros(len(ranges), dtype=torch.int32, device=dev)
    uncompress_ranges_device(d_in, arrays, d_off, index.nchunks, d_lo, d_ln, int(total), d_out, d_oo, d_ol, d_st, n=n)
    return collect(d_out.cpu().numpy(), out_off, d_ol.cpu().numpy()), d_st.cpu().numpy()


def max_data_chunks(n):
    """smf_max_data_chunks: the most data chunks an n-byte framed stream can hold, (n - 10) // 8.
    For a stream of this library's encoder ceil(uncompressed length / 65536) is the count."""
    return lib().smf_max_data_chunks(int(n))


def streams_plan(streams, out_cap=None, max_chunks=0x7FFFFFFF):
    """smf_streams_plan, the device's decode plan on the host, for a list of framed streams:
    (rc, first, out_len, status, total) -- per stream what is known before any byte is decoded
    (the walk's error, SM_BUFFER_TOO_SMALL against out_cap[s], or 0), the size needed, and the
    exclusive scan of the slots (len(streams) + 1 entries)."""
    buf, offs, lens = _lay_out(streams)
    k = len(streams)
    cap = None if out_cap is None else np.ascontiguousarray(out_cap, dtype=np.uint64)
    first, out_len, status = np.zeros(k + 1, np.uint32), np.zeros(k, np.uint64), np.zeros(k, np.int32)
    total = ctypes.c_uint64(0)
    rc = lib().smf_streams_plan(buf.ctypes.data, offs.ctypes.data, lens.ctypes.data, k,
                                None if cap is None else cap.ctypes.data, int(max_chunks), first.ctypes.data,
                                out_len.ctypes.data, status.ctypes.data, ctypes.byref(total))
    return int(rc), first, out_len, status, total.value


def compress_framed_streams(datas, mode="fast", device=0):
    """Frame every buffer of `datas` as a stream of its own in one batched call
    (smf_compress_streams): a list of bytes, each what compress_framed gives for that input."""
    datas = list(datas)
    if not datas:
        return []
    buf, offs, lens = _lay_out(datas)
    out_off = exclusive_scan(10 + 8 * ((lens + 65535) // 65536) + lens, total=True)  # max_framed_length each
    out = np.empty(int(out_off[-1]), np.uint8)
    out_len, status = np.zeros(len(datas), np.uint64), np.zeros(len(datas), np.int32)
    check(lib().smf_compress_streams(context(device), buf.ctypes.data, offs.ctypes.data, lens.ctypes.data, len(datas),
                                     out.ctypes.data, out_off.ctypes.data, out_len.ctypes.data, status.ctypes.data,
                                     _mode(mode)), FramingError)
    _raise_first(status.tolist())
    return collect(out, out_off, out_len)


class StreamError(FramingError):
    """A FramingError of one stream of a batch: `stream` is its number in the batch."""

    def __init__(self, code, stream):
        super().__init__(code)
        self.stream = stream


def _raise_first(codes):
    for s, code in enumerate(codes):
        if code:
            raise StreamError(code, s)


def uncompress_framed_streams(streams, device=0, return_status=False):
    """Decode a list of framed streams in one batched call (smf_uncompress_streams), every chunk's
    CRC-32C checked: a list of bytes.  A failing stream raises StreamError (a FramingError with the
    first failing stream's status and its number as `.stream`); with return_status=True nothing is
    raised and the result is (list of bytes, or None for a failing stream; list of statuses)."""
    streams = list(streams)
    if not streams:
        return ([], []) if return_status else []
    buf, offs, lens = _lay_out(streams)
    k = len(streams)
    _, _, need, pre, _ = streams_plan(streams)
    cap = np.where(pre == 0, need, 0).astype(np.uint64)
    out_off = exclusive_scan(cap, total=True)
    out = np.empty(max(int(out_off[-1]), 1), np.uint8)
    out_len, status = np.zeros(k, np.uint64), np.zeros(k, np.int32)
    check(lib().smf_uncompress_streams(context(device), buf.ctypes.data, offs.ctypes.data, lens.ctypes.data, k,
                                       out.ctypes.data, out_off.ctypes.data, cap.ctypes.data, out_len.ctypes.data,
                                       status.ctypes.data), FramingError)
    codes = status.tolist()
    if not return_status:
        _raise_first(codes)
    res = collect(out, out_off, out_len, codes)
    return (res, codes) if return_status else res


def validate_framed(data, device=0):
    """SM_OK (0) or the status uncompress_framed(data) would raise with."""
    src, n, keep = _in_arg(data)
    return int(lib().smf_validate(context(device), src, n))


# ---- device API (torch tensors resident in HBM; asynchronous on `stream`) ---------------------

_device = device_caller(lib, context, FramingError)
_device_status = device_caller(lib, context, None)


def _or_null(d_in, n):
    """The input argument of a call over d_in[:n]: a tensor of no bytes goes as a null pointer (what is
    no tensor goes on to the argument checks)."""
    return None if not n and hasattr(d_in, "numel") else d_in


def device_chunks(max_chunks, device=0):
    """Index arrays for up to max_chunks data chunks on the device: a dict of torch tensors (type
    uint8, pay_off int64, pay_len / crc / ulen int32: the C ABI's unsigned values, bit for bit)."""
    import torch
    n = max(int(max_chunks), 1)
    return {k: torch.zeros(n, dtype=getattr(torch, np.dtype(_SIGNED[k]).name), device="cuda:%d" % device)
            for k in INDEX_KEYS}


def crc32c_batch_device(d_in, d_off, d_len, d_crc, masked=False, stream=None, device=None):
    """d_crc[b] = CRC-32C of d_in[d_off[b] : d_off[b] + d_len[b]] (masked: the framing format's
    stored form).  d_in uint8, d_off int64, d_len / d_crc int32 CUDA tensors.
    Arguments are checked first (_binding.device_caller; README, Device API)."""
    _device("smf_crc32c_batch_device", d_in, device, stream, d_in, d_off, d_len, numel(d_len), d_crc,
            1 if masked else 0)


def compress_framed_device(d_in, d_out, d_out_len, d_status, mode="fast", stream=None, device=None):
    """Frame the uint8 tensor d_in into d_out (at least max_framed_length(numel(d_in)) bytes);
    d_out_len (int64[1]) and d_status (int32[1]) receive the stream's length and status.
    Arguments are checked first (_binding.device_caller; README, Device API)."""
    n = numel(d_in)
    _device("smf_compress_device", d_out, device, stream, _or_null(d_in, n), n, d_out, numel(d_out), d_out_len,
            d_status, _mode(mode))


def index_framed_device(d_in, arrays, d_summary, n=None, stream=None, device=None):
    """Walk the framed stream d_in[:n] on the device with one wave.  arrays: device_chunks(...) or
    None (count only); d_summary: 16 bytes (a uint8[16] or int64[2] tensor) receiving smf_summary
    -- read it with read_summary() after synchronising.
    Arguments are checked first (_binding.device_caller; README, Device API).  Length not checked: arrays."""
    n = numel(d_in) if n is None else int(n)
    _device("smf_index_device", d_summary, device, stream, _or_null(d_in, n), n,
            arrays, numel(arrays["type"]) if isinstance(arrays, dict) and "type" in arrays else 0,
            d_summary)


def read_summary(d_summary):
    """The Summary a d_summary tensor holds (copies it to the host: synchronises)."""
    raw = d_summary.view(-1).cpu().numpy().tobytes()[:16]
    return Summary.from_buffer_copy(raw)


def uncompressed_length_framed_device(d_in, d_len, d_status, n=None, stream=None, device=None):
    """d_len (int64[1]) = the total uncompressed length of the framed stream d_in[:n], d_status
    (int32[1]) = the walk's status.
    Arguments are checked first (_binding.device_caller; README, Device API)."""
    n = numel(d_in) if n is None else int(n)
    _device("smf_uncompressed_length_device", d_len, device, stream, _or_null(d_in, n), n, d_len, d_status)


def uncompress_chunks_device(d_in, arrays, nchunks, d_out, d_chunk_status, d_out_len, d_status, stream=None,
                             device=None):
    """Decode the first nchunks indexed data chunks of d_in into d_out and check their CRCs
    (smf_uncompress_chunks_device): d_chunk_status int32[nchunks], d_out_len int64[1], d_status
    int32[1].
    Arguments are checked first (_binding.device_caller; README, Device API)."""
    _device("smf_uncompress_chunks_device", d_out, device, stream, d_in, arrays, int(nchunks), d_out,
            numel(d_out), d_chunk_status, d_out_len, d_status)


def uncompress_framed_device(d_in, d_out, d_out_len, d_status, n=None, stream=None, device=None):
    """Index plus decode of the framed stream d_in[:n] into d_out, with one host synchronisation
    of `stream` between them.  Returns the host-known status (0, a structural error, or
    SM_BUFFER_TOO_SMALL with the needed size in d_out_len) instead of raising; the decode's own
    status (CRC, payload errors) arrives in d_status on the stream.
    Arguments are checked first (_binding.device_caller; README, Device API)."""
    n = numel(d_in) if n is None else int(n)
    return _device_status("smf_uncompress_device", d_out, device, stream, _or_null(d_in, n), n, d_out, numel(d_out),
                          d_out_len, d_status)


def compress_framed_indexed_device(d_in, d_out, d_out_len, d_status, arrays, d_chunk_off, d_nchunks, mode="fast",
                                   stream=None, device=None):
    """compress_framed_device that also writes the stream's seek index (smf_compress_indexed_device):
    arrays = device_chunks(max_chunks), d_chunk_off int64[max_chunks + 1], d_nchunks int32[1];
    max_chunks is taken from d_chunk_off and must be at least ceil(numel(d_in) / 65536).
    Arguments are checked first (_binding.device_caller; README, Device API).  Length not checked: arrays."""
    n = numel(d_in)
    _device("smf_compress_indexed_device", d_out, device, stream, _or_null(d_in, n), n, d_out, numel(d_out),
            d_out_len, d_status, _mode(mode), arrays, d_chunk_off, max(numel(d_chunk_off) - 1, 0), d_nchunks)


def chunk_offsets_device(d_ulen, nchunks, d_chunk_off, stream=None, device=None):
    """d_chunk_off (int64[nchunks + 1]) = the exclusive scan of d_ulen[:nchunks] (int32, as
    device_chunks()["ulen"]): completes an index_framed_device index.
    Arguments are checked first (_binding.device_caller; README, Device API)."""
    _device("smf_chunk_offsets_device", d_chunk_off, device, stream, d_ulen, int(nchunks), d_chunk_off)


def uncompress_ranges_device(d_in, arrays, d_chunk_off, nchunks, d_lo, d_len, max_range_chunks, d_out, d_out_off,
                             d_out_len, d_range_status, n=None, stream=None, device=None):
    """Batched ranged decode (smf_uncompress_ranges_device) of the indexed framed stream d_in[:n]:
    range r = bytes [d_lo[r], d_lo[r] + d_len[r]) of the content, written to d_out[d_out_off[r]:];
    d_lo / d_len / d_out_off / d_out_len int64[nranges], d_range_status int32[nranges].
    Arguments are checked first (_binding.device_caller; README, Device API)."""
    n = numel(d_in) if n is None else int(n)
    _device("smf_uncompress_ranges_device", d_out, device, stream, _or_null(d_in, n), n, arrays,
            d_chunk_off, int(nchunks), d_lo, d_len, numel(d_lo), int(max_range_chunks), d_out, d_out_off, d_out_len,
            d_range_status)


def compress_framed_streams_device(d_in, d_in_off, d_in_len, max_blocks, d_out, d_out_off, d_out_len, d_status,
                                   mode="fast", stream=None, device=None):
    """Batched framing (smf_compress_streams_device): input s = d_in[d_in_off[s] : d_in_off[s] +
    d_in_len[s]] becomes one framed stream at d_out[d_out_off[s]:], where max_framed_length(d_in_len[s])
    bytes are left for it.  d_in / d_out uint8, d_in_off / d_in_len / d_out_off / d_out_len
    int64[nstreams], d_status int32[nstreams]; max_blocks bounds the sum of ceil(d_in_len[s] / 65536).
    Arguments are checked first (_binding.device_caller; README, Device API)."""
    _device("smf_compress_streams_device", d_out, device, stream, d_in, d_in_off, d_in_len, numel(d_in_len),
            int(max_blocks), d_out, d_out_off, d_out_len, d_status, _mode(mode))


def uncompress_framed_streams_device(d_in, d_in_off, d_in_len, max_chunks, d_out, d_out_off, d_out_cap, d_out_len,
                                     d_status, d_chunk_first=None, d_chunk_status=None, stream=None, device=None):
    """Batched decode (smf_uncompress_streams_device): framed stream s = d_in[d_in_off[s] :
    d_in_off[s] + d_in_len[s]] decodes into d_out[d_out_off[s] : d_out_off[s] + d_out_cap[s]]; per
    stream d_out_len (int64) and d_status (int32) as uncompress_framed_device leaves them for that
    stream alone.  max_chunks bounds the data chunks summed over the streams that are decoded.
    Optional, both or neither: d_chunk_first int32[nstreams + 1], d_chunk_status int32[max_chunks].
    Arguments are checked first (_binding.device_caller; README, Device API).  Length not checked: d_chunk_status."""
    _device("smf_uncompress_streams_device", d_out, device, stream, d_in, d_in_off, d_in_len, numel(d_in_len),
            int(max_chunks), d_out, d_out_off, d_out_cap, d_out_len, d_status, d_chunk_first, d_chunk_status)


__all__ = ["FRAMING_ABI_SYMBOLS", "MODES", "compress_framed_streams", "uncompress_framed_streams", "streams_plan",
           "max_data_chunks", "compress_framed_streams_device", "uncompress_framed_streams_device", "StreamError", "compress_framed", "uncompress_framed", "length_uncompressed_framed",
           "validate_framed", "index_framed", "crc32c_batch_device", "compress_framed_device", "index_framed_device",
           "uncompressed_length_framed_device", "uncompress_chunks_device", "uncompress_framed_device", "FramedIndex",
           "seek_index_framed", "chunk_offsets", "range_chunk_count", "range_plan", "uncompress_framed_range",
           "uncompress_framed_ranges", "compress_framed_indexed_device", "chunk_offsets_device",
           "uncompress_ranges_device"]
