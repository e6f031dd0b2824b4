"""The Snappy framing format (framing_format.txt of google/snappy: .sz files, snzip, Go's
snappy.Writer) over include/snappy_mi355x_framing.h -- libsnappy_mi355x_framing.so, the companion
of libsnappy_mi355x.so.

    compress_framed(x)           -> bytes   identifier + one chunk per 64 KiB block, CRC-32C each
    uncompress_framed(x)         -> bytes   CRC-checked; raises SnappyError
    length_uncompressed_framed(x) -> int    from the chunk headers alone (host, no device)
    validate_framed(x)           -> status  what uncompress_framed would raise with, or 0
    index_framed(x)              -> (summary, arrays)  the host chunk walker

and, on torch tensors resident in HBM: crc32c_batch_device, compress_framed_device,
index_framed_device, uncompressed_length_framed_device, uncompress_chunks_device,
uncompress_framed_device.

The package imports without this library; it is loaded on the first call here.  No CPU
fallback: every codec call needs both HIP libraries and a device.
"""
import ctypes
import os
import threading

import numpy as np

from . import HERE, MODES, SnappyError, _in_arg, _mode, _out_buffer, _ptr, _stream

LIB_PATH = os.path.join(HERE, "libsnappy_mi355x_framing.so")

SMF_ERR_NO_IDENTIFIER = 48
SMF_ERR_BAD_IDENTIFIER = 49
SMF_ERR_RESERVED_CHUNK = 50
SMF_ERR_TRUNCATED = 51
SMF_ERR_CHUNK_TOO_LARGE = 52
SMF_ERR_CRC = 53
IDENTIFIER = b"\xff\x06\x00\x00sNaPpY"

# exported symbols of include/snappy_mi355x_framing.h (checked by tests/test_framing_host.py)
FRAMING_ABI_SYMBOLS = (
    "smf_status_message", "smf_version", "smf_max_framed_length", "smf_crc32c", "smf_crc32c_mask", "smf_index",
    "smf_uncompressed_length", "smf_ctx_create", "smf_ctx_destroy", "smf_crc32c_batch_device", "smf_compress_device",
    "smf_index_device", "smf_uncompressed_length_device", "smf_uncompress_chunks_device", "smf_uncompress_device",
    "smf_compress", "smf_uncompress", "smf_validate",
)


class Chunks(ctypes.Structure):
    """smf_chunks: five parallel arrays, one entry per data chunk."""
    _fields_ = [("type", ctypes.c_void_p), ("pay_off", ctypes.c_void_p), ("pay_len", ctypes.c_void_p),
                ("crc", ctypes.c_void_p), ("ulen", ctypes.c_void_p)]


class Summary(ctypes.Structure):
    """smf_summary."""
    _fields_ = [("total_length", ctypes.c_uint64), ("nchunks", ctypes.c_uint32), ("status", ctypes.c_int32)]


_lib = None
_ctx = {}
_ctx_lock = threading.Lock()


def library_path():
    return LIB_PATH


def lib():
    """Load libsnappy_mi355x_framing.so (raises OSError if it was not built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OSError("libsnappy_mi355x_framing.so not built (run __graft_entry__.build())")
        L = ctypes.CDLL(LIB_PATH)
        vp, sz, i32, u32, u64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint64
        pch, psum = ctypes.POINTER(Chunks), ctypes.POINTER(Summary)
        L.smf_status_message.restype = ctypes.c_char_p
        L.smf_status_message.argtypes = [i32]
        L.smf_version.restype = ctypes.c_char_p
        L.smf_version.argtypes = []
        L.smf_max_framed_length.restype = sz
        L.smf_max_framed_length.argtypes = [sz]
        L.smf_crc32c.restype = u32
        L.smf_crc32c.argtypes = [vp, sz]
        L.smf_crc32c_mask.restype = u32
        L.smf_crc32c_mask.argtypes = [u32]
        L.smf_index.restype = i32
        L.smf_index.argtypes = [vp, sz, pch, u32, psum]
        L.smf_uncompressed_length.restype = i32
        L.smf_uncompressed_length.argtypes = [vp, sz, ctypes.POINTER(sz)]
        L.smf_ctx_create.restype = vp
        L.smf_ctx_create.argtypes = [ctypes.c_int]
        L.smf_ctx_destroy.restype = None
        L.smf_ctx_destroy.argtypes = [vp]
        L.smf_crc32c_batch_device.restype = i32
        L.smf_crc32c_batch_device.argtypes = [vp, vp, vp, vp, u32, vp, ctypes.c_int, vp]
        L.smf_compress_device.restype = i32
        L.smf_compress_device.argtypes = [vp, vp, u64, vp, u64, vp, vp, ctypes.c_int, vp]
        L.smf_index_device.restype = i32
        L.smf_index_device.argtypes = [vp, vp, u64, pch, u32, vp, vp]
        L.smf_uncompressed_length_device.restype = i32
        L.smf_uncompressed_length_device.argtypes = [vp, vp, u64, vp, vp, vp]
        L.smf_uncompress_chunks_device.restype = i32
        L.smf_uncompress_chunks_device.argtypes = [vp, vp, pch, u32, vp, u64, vp, vp, vp, vp]
        L.smf_uncompress_device.restype = i32
        L.smf_uncompress_device.argtypes = [vp, vp, u64, vp, u64, vp, vp, vp]
        L.smf_compress.restype = i32
        L.smf_compress.argtypes = [vp, vp, sz, vp, ctypes.POINTER(sz), ctypes.c_int]
        L.smf_uncompress.restype = i32
        L.smf_uncompress.argtypes = [vp, vp, sz, vp, ctypes.POINTER(sz)]
        L.smf_validate.restype = i32
        L.smf_validate.argtypes = [vp, vp, sz]
        _lib = L
    return _lib


def status_message(code):
    return lib().smf_status_message(int(code)).decode()


def version():
    return lib().smf_version().decode()


class FramingError(SnappyError):
    """A SnappyError whose message comes from smf_status_message (the SMF_ERR_* texts too)."""

    def __init__(self, code):
        super().__init__(code, status_message(code))


def context(device=0):
    """Per-device smf_ctx (an sm_ctx of its own plus scratch).  Raises if no device is usable."""
    with _ctx_lock:
        c = _ctx.get(device)
        if c is None:
            c = lib().smf_ctx_create(device)
            if not c:
                raise SnappyError(32, "no usable HIP device %d for snappy_mi355x_framing" % device)
            _ctx[device] = c
    return c


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
    arrays = {"type": np.zeros(max_chunks, np.uint8), "pay_off": np.zeros(max_chunks, np.uint64),
              "pay_len": np.zeros(max_chunks, np.uint32), "crc": np.zeros(max_chunks, np.uint32),
              "ulen": np.zeros(max_chunks, np.uint32)}
    ch = Chunks(*(arrays[k].ctypes.data for k in ("type", "pay_off", "pay_len", "crc", "ulen")))
    lib().smf_index(src, n, ctypes.byref(ch), max_chunks, ctypes.byref(s))
    return s, arrays


def length_uncompressed_framed(data):
    """The stream's total uncompressed length from its chunk headers (no device, no CRC check)."""
    src, n, keep = _in_arg(data)
    res = ctypes.c_size_t(0)
    st = lib().smf_uncompressed_length(src, n, ctypes.byref(res))
    if st:
        raise FramingError(st)
    return res.value


def compress_framed(data, mode="fast", device=0):
    """Frame `data`: the stream identifier, then one chunk per 64 KiB block -- compressed (0x00)
    iff its Snappy stream is strictly shorter than the block, else uncompressed (0x01) -- each
    with the masked CRC-32C of its uncompressed bytes.  Computed on the GPU."""
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


def validate_framed(data, device=0):
    """SM_OK (0) or the status uncompress_framed(data) would raise with."""
    src, n, keep = _in_arg(data)
    return int(lib().smf_validate(context(device), src, n))


# ---- device API (torch tensors resident in HBM; asynchronous on `stream`) ---------------------

def _dev(t, device):
    return t.device.index if device is None else device


def _sp(stream, dev):
    return ctypes.c_void_p(_stream(stream, dev))


def device_chunks(max_chunks, device=0):
    """Index arrays for up to max_chunks data chunks on the device: a dict of torch tensors (type
    uint8, pay_off int64, pay_len / crc / ulen int32: the C ABI's unsigned values, bit for bit)."""
    import torch
    dev = "cuda:%d" % device
    n = max(int(max_chunks), 1)
    return {"type": torch.zeros(n, dtype=torch.uint8, device=dev), "pay_off": torch.zeros(n, dtype=torch.int64, device=dev),
            "pay_len": torch.zeros(n, dtype=torch.int32, device=dev), "crc": torch.zeros(n, dtype=torch.int32, device=dev),
            "ulen": torch.zeros(n, dtype=torch.int32, device=dev)}


def _chunks_struct(arrays):
    return Chunks(*(arrays[k].data_ptr() for k in ("type", "pay_off", "pay_len", "crc", "ulen")))


def crc32c_batch_device(d_in, d_off, d_len, d_crc, masked=False, stream=None, device=None):
    """d_crc[b] = CRC-32C of d_in[d_off[b] : d_off[b] + d_len[b]] (masked: the framing format's
    stored form).  d_in uint8, d_off int64, d_len / d_crc int32 CUDA tensors."""
    dev = _dev(d_in, device)
    st = lib().smf_crc32c_batch_device(context(dev), _ptr(d_in), _ptr(d_off), _ptr(d_len), d_len.numel(), _ptr(d_crc),
                                       1 if masked else 0, _sp(stream, dev))
    if st:
        raise FramingError(st)


def compress_framed_device(d_in, d_out, d_out_len, d_status, mode="fast", stream=None, device=None):
    """Frame the uint8 tensor d_in into d_out (at least max_framed_length(d_in.numel()) bytes);
    d_out_len (int64[1]) and d_status (int32[1]) receive the stream's length and status."""
    dev = _dev(d_out, device)
    n = d_in.numel()
    st = lib().smf_compress_device(context(dev), _ptr(d_in) if n else None, n, _ptr(d_out), d_out.numel(),
                                   _ptr(d_out_len), _ptr(d_status), _mode(mode), _sp(stream, dev))
    if st:
        raise FramingError(st)


def index_framed_device(d_in, arrays, d_summary, n=None, stream=None, device=None):
    """Walk the framed stream d_in[:n] on the device with one wave.  arrays: device_chunks(...) or
    None (count only); d_summary: 16 bytes (a uint8[16] or int64[2] tensor) receiving smf_summary
    -- read it with read_summary() after synchronising."""
    dev = _dev(d_summary, device)
    n = d_in.numel() if n is None else int(n)
    ch = _chunks_struct(arrays) if arrays is not None else None
    cap = arrays["type"].numel() if arrays is not None else 0
    st = lib().smf_index_device(context(dev), _ptr(d_in) if n else None, n, ctypes.byref(ch) if ch is not None else None,
                                cap, _ptr(d_summary), _sp(stream, dev))
    if st:
        raise FramingError(st)


def read_summary(d_summary):
    """The Summary a d_summary tensor holds (copies it to the host: synchronises)."""
    raw = d_summary.view(-1).cpu().numpy().tobytes()[:16]
    return Summary.from_buffer_copy(raw)


def uncompressed_length_framed_device(d_in, d_len, d_status, n=None, stream=None, device=None):
    """d_len (int64[1]) = the total uncompressed length of the framed stream d_in[:n], d_status
    (int32[1]) = the walk's status."""
    dev = _dev(d_len, device)
    n = d_in.numel() if n is None else int(n)
    st = lib().smf_uncompressed_length_device(context(dev), _ptr(d_in) if n else None, n, _ptr(d_len), _ptr(d_status),
                                              _sp(stream, dev))
    if st:
        raise FramingError(st)


def uncompress_chunks_device(d_in, arrays, nchunks, d_out, d_chunk_status, d_out_len, d_status, stream=None,
                             device=None):
    """Decode the first nchunks indexed data chunks of d_in into d_out and check their CRCs
    (smf_uncompress_chunks_device): d_chunk_status int32[nchunks], d_out_len int64[1], d_status
    int32[1]."""
    dev = _dev(d_out, device)
    ch = _chunks_struct(arrays)
    st = lib().smf_uncompress_chunks_device(context(dev), _ptr(d_in), ctypes.byref(ch), int(nchunks), _ptr(d_out),
                                            d_out.numel(), _ptr(d_chunk_status), _ptr(d_out_len), _ptr(d_status),
                                            _sp(stream, dev))
    if st:
        raise FramingError(st)


def uncompress_framed_device(d_in, d_out, d_out_len, d_status, n=None, stream=None, device=None):
    """Index plus decode of the framed stream d_in[:n] into d_out, with one host synchronisation
    of `stream` between them.  Returns the host-known status (0, a structural error, or
    SM_BUFFER_TOO_SMALL with the needed size in d_out_len) instead of raising; the decode's own
    status (CRC, payload errors) arrives in d_status on the stream."""
    dev = _dev(d_out, device)
    n = d_in.numel() if n is None else int(n)
    return int(lib().smf_uncompress_device(context(dev), _ptr(d_in) if n else None, n, _ptr(d_out), d_out.numel(),
                                           _ptr(d_out_len), _ptr(d_status), _sp(stream, dev)))


__all__ = ["FRAMING_ABI_SYMBOLS", "MODES", "compress_framed", "uncompress_framed", "length_uncompressed_framed",
           "validate_framed", "index_framed", "crc32c_batch_device", "compress_framed_device", "index_framed_device",
           "uncompressed_length_framed_device", "uncompress_chunks_device", "uncompress_framed_device"]
