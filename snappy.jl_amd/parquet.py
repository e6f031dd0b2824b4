"""The pages of Parquet column chunks written with compression=SNAPPY over
include/snappy_mi355x_parquet.h -- libsnappy_mi355x_parquet.so, the companion of
libsnappy_mi355x_multi.so and libsnappy_mi355x.so.  A column chunk is a run of pages, each a Thrift
compact-protocol PageHeader and a body: a raw Snappy stream, behind the stored level bytes of a v2
data page.  The caller supplies each chunk's byte range (from the footer's ColumnMetaData: start =
dictionary_page_offset if present, else data_page_offset; length = total_compressed_size) and
promises that its codec is SNAPPY -- no footer, schema or encoding is parsed here.

    uncompress_column_chunk(x)                 -> (bytes, page table)   one chunk (a batch of one)
    uncompress_column_chunks(xs)               -> list of (bytes, page table)   one batched call
    index_column_chunk(x)                      -> (summary, arrays)     the host walk
    chunks_plan(xs), max_pages(n), length_uncompressed(x)               (host, no device)

and, on torch tensors resident in HBM: uncompress_column_chunks_device, crc32_device (no host
synchronisation), last_indexed.

The page encoder (include/snappy_mi355x_parquet_write.h, the same library) goes the other way: a
chunk in its plain form -- pages with compressed_page_size == uncompressed_page_size, what a writer
holds before compression and what parquet-cpp writes with compression=NONE -- becomes the
compression=SNAPPY chunk the calls above read, its page headers rewritten around the new bodies:

    compress_column_chunk(x, mode)             -> bytes                 one chunk (a batch of one)
    compress_column_chunks(xs, mode)           -> list of bytes         one batched call
    index_plain_column_chunk(x)                -> (summary, arrays, sites)   the encode walk on the host
    rewrite_page_header(h, new_body_len, crc), compress_chunks_plan(xs), max_compressed_chunk_length(n, pages)

and compress_column_chunks_device on tensors.

A chunk's output is its pages' uncompressed bytes back to back, what a CPU reader holds after
decompression; the page table says where each page's bytes lie and what its header declares.

The package imports without this library; it is loaded on the first call here.  No CPU fallback:
every decode needs the three HIP libraries and a device.
"""
import ctypes
import os

import numpy as np

from . import HERE, SnappyError, _in_arg, _mode
from ._binding import (PAGE_KEYS, PARQUET, PARQUET_WRITE, Pages, Summary, check, collect, context_cache, device_caller,
                       exclusive_scan, field_dtypes, lay_out, load, numel)

LIB_PATH = os.path.join(HERE, "libsnappy_mi355x_parquet.so")

SMQ_ERR_HEADER = 72
SMQ_ERR_TRUNCATED = 73
SMQ_ERR_SIZE_MISMATCH = 74
SMQ_ERR_CRC = 75
PAGE_DATA, PAGE_INDEX, PAGE_DICTIONARY, PAGE_DATA_V2 = 0, 1, 2, 3
PAGE_HAS_CRC, PAGE_COMPRESSED = 1, 2
INDEX_KEYS = PAGE_KEYS  # smq_pages' arrays, in its order
PAGE_DTYPES = field_dtypes(Pages)  # the arrays' element types as the C ABI declares them (Pages.elements)

PARQUET_ABI_SYMBOLS = tuple(PARQUET)  # exported symbols of include/snappy_mi355x_parquet.h (tests/test_parquet_host.py)
PARQUET_WRITE_ABI_SYMBOLS = tuple(PARQUET_WRITE)  # and of include/snappy_mi355x_parquet_write.h (tests/test_parquet_write_host.py)
SITE_KEYS = ("f3_at", "f3_len", "f4_at", "f4_len", "f7_at")  # a page's patch sites, SMQE_SITES words

_lib = None


def library_path():
    return LIB_PATH


def lib():
    """Load libsnappy_mi355x_parquet.so (raises OSError if it was not built)."""
    global _lib
    if _lib is None:
        _lib = load(LIB_PATH, {**PARQUET, **PARQUET_WRITE}, "libsnappy_mi355x_parquet.so not built (run __graft_entry__.build())")
    return _lib


def status_message(code):
    return lib().smq_status_message(int(code)).decode()


def version():
    return lib().smq_version().decode()


class ParquetError(SnappyError):
    """A SnappyError whose message comes from smq_status_message (the SMQ_ERR_* texts too); for a
    chunk of a batch `chunk` is its number in the batch, else None."""

    def __init__(self, code, chunk=None):
        super().__init__(code, status_message(code))
        self.chunk = chunk


# context(device=0): the per-device smq_ctx (an smm_ctx of its own, the CRC tables and scratch)
_ctx, _ctx_lock, context = context_cache(lib, "smq_ctx_create", SnappyError,
                                         "no usable HIP device %d for snappy_mi355x_parquet")


# ---- host helpers (no device) ---------------------------------------------------------------

def max_pages(n):
    """smq_max_pages: the most pages an n-byte chunk can hold (7 bytes each at the least)."""
    return lib().smq_max_pages(int(n))


def index_column_chunk(data, max_pages=None):
    """The host walk (smq_index): (Summary, dict of numpy arrays, keyed as INDEX_KEYS, of the pages).
    max_pages=None sizes the arrays by a counting walk first."""
    src, n, keep = _in_arg(data)
    s = Summary()
    if max_pages is None:
        s.status = lib().smq_index(src, n, None, 0, ctypes.byref(s))
        max_pages = s.nchunks
    arrays = {k: np.zeros(max_pages, PAGE_DTYPES[k]) for k in INDEX_KEYS}
    pages = Pages(*(arrays[k].ctypes.data for k in INDEX_KEYS))
    s.status = lib().smq_index(src, n, ctypes.byref(pages), max_pages, ctypes.byref(s))
    return s, arrays


def length_uncompressed(data):
    """The chunk's total uncompressed length from its page headers (no device)."""
    src, n, keep = _in_arg(data)
    res = ctypes.c_size_t(0)
    check(lib().smq_uncompressed_length(src, n, ctypes.byref(res)), ParquetError)
    return res.value


def chunks_plan(chunks, out_cap=None, max_pages=0x7FFFFFFF):
    """smq_chunks_plan, the device's decode plan on the host, for a list of chunks: (rc, first,
    out_len, status, total_pages, total_fragments) -- per chunk what is known before any byte is
    decoded (the walk's error, SM_BUFFER_TOO_SMALL against out_cap[c], or 0), the size needed, the
    exclusive scan of the slots (len(chunks) + 1 entries), and the device call's two bounds."""
    buf, offs, lens = lay_out(chunks)
    k = len(chunks)
    cap = None if out_cap is None else np.ascontiguousarray(out_cap, dtype=np.uint64)
    first, out_len, status = np.zeros(k + 1, np.uint32), np.zeros(k, np.uint64), np.zeros(k, np.int32)
    pages, fragments = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = lib().smq_chunks_plan(buf.ctypes.data, offs.ctypes.data, lens.ctypes.data, k, None if cap is None else cap.ctypes.data,
                               int(max_pages), first.ctypes.data, out_len.ctypes.data, status.ctypes.data, ctypes.byref(pages),
                               ctypes.byref(fragments))
    return int(rc), first, out_len, status, pages.value, fragments.value


# ---- the page encoder's host helpers (no device) ----------------------------------------------------

def max_compressed_chunk_length(n, pages):
    """smqe_max_chunk_length: an upper bound on the SNAPPY form of an n-byte plain chunk of `pages` pages."""
    return lib().smqe_max_chunk_length(int(n), int(pages))


def rewrite_page_header(header, new_body_len, crc=0):
    """smqe_rewrite_header, the rewrite rule alone: the bytes of the PageHeader at the start of
    `header` with compressed_page_size = new_body_len, its crc field (if it has one) = crc, and a v2
    is_compressed (if it has one) true.  Raises ParquetError for a header the encode walk refuses."""
    src, n, keep = _in_arg(header)
    out = np.empty(n + 8, np.uint8)  # (each of the two varints grows by 4 bytes at the most)
    got = ctypes.c_size_t(0)
    check(lib().smqe_rewrite_header(src, n, int(new_body_len), int(crc) & 0xFFFFFFFF, out.ctypes.data, out.size,
                                    ctypes.byref(got)), ParquetError)
    return out[:got.value].tobytes()


def index_plain_column_chunk(data, max_pages=None):
    """The encode walk on the host (smqe_index) over a chunk in its plain form: (Summary, dict of numpy
    arrays keyed as INDEX_KEYS -- the input's pages --, uint32 array [pages, 5] of the headers' patch
    sites, columns as SITE_KEYS).  max_pages=None sizes the arrays by a counting walk first."""
    src, n, keep = _in_arg(data)
    s = Summary()
    if max_pages is None:
        s.status = lib().smqe_index(src, n, None, None, 0, ctypes.byref(s))
        max_pages = s.nchunks
    arrays = {k: np.zeros(max_pages, PAGE_DTYPES[k]) for k in INDEX_KEYS}
    sites = np.zeros((max_pages, len(SITE_KEYS)), np.uint32)
    pages = Pages(*(arrays[k].ctypes.data for k in INDEX_KEYS))
    s.status = lib().smqe_index(src, n, ctypes.byref(pages), sites.ctypes.data, max_pages, ctypes.byref(s))
    return s, arrays, sites


def compress_chunks_plan(chunks, max_pages=0x7FFFFFFF):
    """smqe_chunks_plan, the device's encode plan on the host, for a list of plain chunks: (rc, first,
    status, out_bound, total_pages, stage_bytes, total_fragments) -- per chunk the walk's error or 0,
    the exclusive scan of the slots (len(chunks) + 1 entries), an output capacity that always
    suffices, and the device call's three bounds."""
    buf, offs, lens = lay_out(chunks)
    k = len(chunks)
    first, status, bound = np.zeros(k + 1, np.uint32), np.zeros(k, np.int32), np.zeros(k, np.uint64)
    pages, stage, fragments = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = lib().smqe_chunks_plan(buf.ctypes.data, offs.ctypes.data, lens.ctypes.data, k, int(max_pages), first.ctypes.data,
                                status.ctypes.data, bound.ctypes.data, ctypes.byref(pages), ctypes.byref(stage),
                                ctypes.byref(fragments))
    return int(rc), first, status, bound, pages.value, stage.value, fragments.value


# ---- host buffers -----------------------------------------------------------------------

def uncompress_column_chunks(chunks, verify_crc=True, device=0, statuses=False):
    """Decode a list of column chunks in one batched call (smq_uncompress_chunks): a list of (bytes,
    page table), the table a dict of numpy arrays as index_column_chunk gives it.  With verify_crc
    the pages whose header carries a crc are checked on the device.  A failing chunk raises
    ParquetError (the first failing chunk's status, its number as `.chunk`); with statuses=True
    nothing is raised and the result is (that list, with None for a failing chunk's bytes; list of
    statuses)."""
    chunks = list(chunks)
    if not chunks:
        return ([], []) if statuses else []
    buf, offs, lens = lay_out(chunks)
    k = len(chunks)
    _, _, need, pre, _, _ = chunks_plan(chunks)
    cap = np.where(pre == 0, need, 0).astype(np.uint64)
    out_off = exclusive_scan(cap, total=True)
    out = np.empty(max(int(out_off[-1]), 1), np.uint8)
    out_len, status = np.zeros(k, np.uint64), np.zeros(k, np.int32)
    check(lib().smq_uncompress_chunks(context(device), buf.ctypes.data, offs.ctypes.data, lens.ctypes.data, k,
                                      1 if verify_crc else 0, out.ctypes.data, out_off.ctypes.data, cap.ctypes.data,
                                      out_len.ctypes.data, status.ctypes.data), ParquetError)
    codes = status.tolist()
    if not statuses:
        for c, code in enumerate(codes):
            if code:
                raise ParquetError(code, c)
    res = list(zip(collect(out, out_off, out_len, codes), [index_column_chunk(c)[1] for c in chunks]))
    return (res, codes) if statuses else res


def uncompress_column_chunk(data, verify_crc=True, device=0):
    """One column chunk: (its pages' uncompressed bytes back to back, the page table)."""
    try:
        return uncompress_column_chunks([data], verify_crc=verify_crc, device=device)[0]
    except ParquetError as e:
        raise ParquetError(e.code) from None  # (a chunk alone has no number)


def compress_column_chunks(chunks, mode="fast", device=0, statuses=False):
    """Compress a list of plain column chunks in one batched call (smqe_compress_chunks): a list of
    bytes, each the compression=SNAPPY form of its chunk.  A failing chunk raises ParquetError (its
    status, its number as `.chunk`); with statuses=True nothing is raised and the result is (that
    list, with None for a failing chunk; list of statuses)."""
    chunks = list(chunks)
    if not chunks:
        return ([], []) if statuses else []
    buf, offs, lens = lay_out(chunks)
    k = len(chunks)
    cap = compress_chunks_plan(chunks)[3]
    out_off = exclusive_scan(cap, total=True)
    out = np.empty(max(int(out_off[-1]), 1), np.uint8)
    out_len, status = np.zeros(k, np.uint64), np.zeros(k, np.int32)
    check(lib().smqe_compress_chunks(context(device), buf.ctypes.data, offs.ctypes.data, lens.ctypes.data, k, out.ctypes.data,
                                     out_off.ctypes.data, cap.ctypes.data, out_len.ctypes.data, status.ctypes.data,
                                     _mode(mode)), ParquetError)
    codes = status.tolist()
    if not statuses:
        for c, code in enumerate(codes):
            if code:
                raise ParquetError(code, c)
    res = collect(out, out_off, out_len, codes)
    return (res, codes) if statuses else res


def compress_column_chunk(data, mode="fast", device=0):
    """One plain column chunk: its compression=SNAPPY form."""
    try:
        return compress_column_chunks([data], mode=mode, device=device)[0]
    except ParquetError as e:
        raise ParquetError(e.code) from None  # (a chunk alone has no number)


# ---- device API (torch tensors resident in HBM; asynchronous on `stream`) ---------------------

_device = device_caller(lib, context, ParquetError)


def uncompress_column_chunks_device(d_in, d_in_off, d_in_len, max_pages, max_fragments, d_out, d_out_off, d_out_cap, d_out_len,
                                    d_status, verify_crc=True, d_page_first=None, d_page_status=None, d_pages=None, stream=None,
                                    device=None):
    """smq_uncompress_chunks_device: chunk c = d_in[d_in_off[c] : d_in_off[c] + d_in_len[c]] decodes
    into d_out[d_out_off[c] : d_out_off[c] + d_out_cap[c]]; per chunk d_out_len (int64) and d_status
    (int32).  max_pages bounds the pages summed over the chunks that are decoded; max_fragments
    (chunks_plan's second total, or 0) lets compressed sections of more than 64 KiB decode by
    fragments.  Optional, both or neither: d_page_first int32[nchunks + 1], d_page_status
    int32[max_pages].  Optional: d_pages, a dict of tensors of max_pages entries keyed as INDEX_KEYS
    (int64 for hdr_off and out_off, int32 for the others), the page table.  Nothing is synchronised.
    Arguments are checked first (_binding.device_caller; README, Device API).
    Length not checked: d_pages, d_page_status."""
    _device("smq_uncompress_chunks_device", d_out, device, stream, d_in, d_in_off, d_in_len, numel(d_in_len), int(max_pages),
            int(max_fragments), 1 if verify_crc else 0, d_out, d_out_off, d_out_cap, d_out_len, d_status, d_page_first, d_pages,
            d_page_status)


def compress_column_chunks_device(d_in, d_in_off, d_in_len, max_pages, stage_bytes, max_fragments, d_out, d_out_off, d_out_cap,
                                  d_out_len, d_status, mode="fast", d_page_first=None, d_page_status=None, d_pages=None,
                                  stream=None, device=None):
    """smqe_compress_chunks_device: the plain chunk c = d_in[d_in_off[c] : d_in_off[c] + d_in_len[c]]
    becomes a compression=SNAPPY chunk in d_out[d_out_off[c] : d_out_off[c] + d_out_cap[c]]; per chunk
    d_out_len (int64) and d_status (int32).  max_pages, stage_bytes and max_fragments are
    compress_chunks_plan's three totals (or bounds on them).  Optional, both or neither: d_page_first
    int32[nchunks + 1], d_page_status int32[max_pages].  Optional: d_pages, a dict of tensors of
    max_pages entries keyed as INDEX_KEYS, the OUTPUT chunks' page table.  Nothing is synchronised.
    Arguments are checked first (_binding.device_caller; README, Device API).
    Length not checked: d_pages, d_page_status."""
    _device("smqe_compress_chunks_device", d_out, device, stream, d_in, d_in_off, d_in_len, numel(d_in_len), int(max_pages),
            int(stage_bytes), int(max_fragments), d_out, d_out_off, d_out_cap, d_out_len, d_status, d_page_first, d_pages,
            d_page_status, _mode(mode))


def crc32_device(d_in, d_off, d_len, d_crc, stream=None, device=None):
    """smq_crc32_device: d_crc[i] (int32, the CRC's 32 bits) = the CRC-32 (zlib.crc32) of
    d_in[d_off[i] : d_off[i] + d_len[i]]; d_off and d_len int64.  Nothing is synchronised.
    Arguments are checked first (_binding.device_caller; README, Device API)."""
    _device("smq_crc32_device", d_crc, device, stream, d_in, d_off, d_len, numel(d_len), d_crc)


def last_indexed(device=0):
    """Diagnostic (smq_ctx_last_indexed): how many values sections the device's last decode call
    took by fragments (waits for the device); -1 before the first call."""
    return int(lib().smq_ctx_last_indexed(context(device)))


__all__ = ["PARQUET_ABI_SYMBOLS", "PARQUET_WRITE_ABI_SYMBOLS", "INDEX_KEYS", "SITE_KEYS", "ParquetError",
           "uncompress_column_chunk", "uncompress_column_chunks", "index_column_chunk", "length_uncompressed", "chunks_plan",
           "max_pages", "uncompress_column_chunks_device", "crc32_device", "last_indexed", "status_message", "version",
           "compress_column_chunk", "compress_column_chunks", "compress_chunks_plan", "index_plain_column_chunk",
           "rewrite_page_header", "max_compressed_chunk_length", "compress_column_chunks_device"]
