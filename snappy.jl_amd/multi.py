"""Batches of raw Snappy streams of any length over include/snappy_mi355x_multi.h --
libsnappy_mi355x_multi.so, the companion of libsnappy_mi355x.so.

    compress_streams(list_of_bytes)         -> list of streams (and the fragment index when asked)
    uncompress_streams(streams, index=...)  -> (list of bytes-or-None, status array)
    index_streams(streams)                  -> (frag_first, frag_pos, built): the index of streams
                                               that came without one, built on the GPU

    uncompress_stream_ranges(streams, index, ranges) -> the bytes of each (stream, lo, len), decoding
                                               only the 64 KiB fragments the ranges touch

and, on torch tensors resident in HBM: compress_streams_device, uncompress_streams_device (no host
synchronisation), index_streams_device, uncompress_stream_ranges_device, last_indexed.
index_streams_host runs the index rule on the CPU, range_plan the ranged decode's plan
(include/snappy_mi355x_multi_range.h).

A stream of at most 64 KiB is what compress_batch gives, a longer one what compress gives; the
index (frag_first, frag_pos) names every 64 KiB fragment's offset in its stream, and with it the
decoder runs every fragment of every stream in parallel.  It is a hint: a wrong index costs time,
never correctness (the stream is then decoded in stream order).

The package imports without this library; it is loaded on the first call here.  No CPU fallback:
every codec call needs both HIP libraries and a device.
"""
import ctypes
import os

import numpy as np

from . import HERE, MODES, SnappyError, _capacities, _mode, pack_blocks, slot_offsets
from ._binding import MULTI, MULTI_RANGE, check, collect, context_cache, device_caller, exclusive_scan, load, numel

LIB_PATH = os.path.join(HERE, "libsnappy_mi355x_multi.so")
BLOCK = 65536
MAX_INPUT = 0x7FFFFFFF
INDEX_STAGE = 4096  # kIndexStage (csrc/multi/smm_plan.h): the bytes the index walk stages per piece

MULTI_ABI_SYMBOLS = tuple(MULTI)  # exported symbols of include/snappy_mi355x_multi.h (checked by tests/test_multi_host.py)
RANGE_ABI_SYMBOLS = tuple(MULTI_RANGE)  # ... of include/snappy_mi355x_multi_range.h (tests/test_multi_range_host.py)

_lib = None


def library_path():
    return LIB_PATH


def lib():
    """Load libsnappy_mi355x_multi.so (raises OSError if it was not built)."""
    global _lib
    if _lib is None:
        _lib = load(LIB_PATH, {**MULTI, **MULTI_RANGE}, "libsnappy_mi355x_multi.so not built (run __graft_entry__.build())")
    return _lib


def version():
    return lib().smm_version().decode()


def status_message(code):
    return lib().smm_status_message(int(code)).decode()


# context(device=0): the per-device smm_ctx (an sm_ctx of its own plus scratch)
_ctx, _ctx_lock, context = context_cache(lib, "smm_ctx_create", SnappyError,
                                         "no usable HIP device %d for snappy_mi355x_multi")


def fragment_count(n):
    """ceil(n / 65536): the 64 KiB fragments (and index entries) of an n-byte input."""
    return lib().smm_fragment_count(int(n))


def scratch_bytes(nstreams, max_fragments):
    return lib().smm_scratch_bytes(int(nstreams), int(max_fragments))


def frag_first_of(lengths):
    """The index's frag_first for inputs of these lengths, on the host: the exclusive scan of
    fragment_count (nstreams + 1 entries)."""
    counts = [(int(n) + BLOCK - 1) // BLOCK if int(n) <= MAX_INPUT else 0 for n in lengths]
    return exclusive_scan(counts, np.uint32, total=True)


def _addr(a):
    return a.ctypes.data if a is not None and a.size else None


def _raise_first(status):
    """SnappyError with the first status of a batch that is not 0."""
    if status.any():
        raise SnappyError(int(status[np.nonzero(status)[0][0]]))


def index_check(streams, index, capacities=None, max_fragments=None):
    """Which streams the decoder would take by fragments given this index (structure only, on the
    host; smm_index_check): a uint8 array."""
    buf, in_off, in_len = pack_blocks(streams)
    cap = _capacities(streams, capacities)
    first = pos = None
    if index is not None:
        first = np.ascontiguousarray(index[0], dtype=np.uint32)
        pos = np.ascontiguousarray(index[1], dtype=np.uint32)
    if max_fragments is None:
        max_fragments = pos.size if pos is not None else 0
    if pos is not None and pos.size < max_fragments:
        raise ValueError("frag_pos is shorter than max_fragments")
    out = np.zeros(len(streams), np.uint8)
    keep = np.zeros(1, np.uint8)
    check(lib().smm_index_check(_addr(buf) or keep.ctypes.data, _addr(in_off), _addr(in_len), len(streams),
                                int(max_fragments), _addr(cap), first.ctypes.data if first is not None else None,
                                (_addr(pos) or keep.ctypes.data) if pos is not None else None, _addr(out)), SnappyError)
    return out


# ---- host buffers -----------------------------------------------------------------------

def compress_streams(datas, mode="fast", device=0, return_index=False):
    """Compress independent inputs of any length (each at most 2^31 - 1 bytes) in one call on the
    GPU; returns a list of raw Snappy streams (bytes), and with return_index also the index
    (frag_first, frag_pos) as uint32 arrays.  Raises SnappyError with the first failing stream's
    status."""
    datas = [bytes(d) if not isinstance(d, bytes) else d for d in datas]
    n = len(datas)
    if any(len(d) > MAX_INPUT for d in datas):
        raise SnappyError(16)
    buf, in_off, in_len = pack_blocks(datas)
    first = np.zeros(n + 1, np.uint32)
    entries = int(frag_first_of(in_len)[-1])
    pos = np.zeros(max(entries, 1), np.uint32)
    outs = []
    if n:
        out_off, caps = slot_offsets(in_len)
        out = np.empty(int(out_off[-1] + caps[-1]), dtype=np.uint8)
        out_len = np.zeros(n, np.uint32)
        status = np.zeros(n, np.int32)
        keep = np.zeros(1, np.uint8)
        check(lib().smm_compress(context(device), _addr(buf) or keep.ctypes.data, in_off.ctypes.data, in_len.ctypes.data,
                                 n, out.ctypes.data, out_off.ctypes.data, out_len.ctypes.data, status.ctypes.data,
                                 first.ctypes.data if return_index else None, pos.ctypes.data if return_index else None,
                                 _mode(mode)), SnappyError)
        _raise_first(status)
        outs = collect(out, out_off, out_len)
    if return_index:
        return outs, (first, pos[:entries])
    return outs


def _index_call(streams, capacities, max_fragments, call):
    """The host arrays of an index call, and call(in, in_off, in_len, n, m, cap, first, pos, built,
    status): (frag_first, frag_pos[:frag_first[-1]], built)."""
    n = len(streams)
    buf, in_off, in_len = pack_blocks(streams)
    cap = None if capacities is None else np.array(capacities, dtype=np.uint32)
    if max_fragments is None:
        max_fragments = index_bound(streams, capacities)
    first = np.zeros(n + 1, np.uint32)
    pos = np.zeros(max(int(max_fragments), 1), np.uint32)
    built = np.zeros(max(n, 1), np.uint8)
    status = np.zeros(max(n, 1), np.int32)
    keep = np.zeros(1, np.uint8)
    check(call(_addr(buf) or keep.ctypes.data, _addr(in_off), _addr(in_len), n, int(max_fragments), _addr(cap),
               first.ctypes.data, pos.ctypes.data, built.ctypes.data, status.ctypes.data), SnappyError)
    _raise_first(status[:n])
    return first, pos[:int(first[-1])], built[:n]


def index_bound(streams, capacities=None):
    """A max_fragments that holds the index of these streams: every stream counted by the length
    its header declares (as far as its capacity allows)."""
    cap = _capacities(streams, None)
    if capacities is not None:
        cap = np.where(cap <= np.array(capacities, dtype=np.uint32), cap, 0)
    return int(((cap.astype(np.uint64) + BLOCK - 1) // BLOCK).sum())


def index_streams(streams, capacities=None, device=0, max_fragments=None):
    """Build on the GPU the index of raw streams that came without one (a CPU compressor wrote them):
    (frag_first, frag_pos, built), what uncompress_streams takes as index=(frag_first, frag_pos).
    built[s] = 1 for a stream of more than 64 KiB in which a tag starts at every 64 KiB of output --
    every block compressor's stream; the others decode in stream order.  capacities: the output room
    per stream (a stream that declares more gets no entries); None: no cap.  Raises SnappyError(33)
    when max_fragments (default: what the headers declare) is too small."""
    ctx = context(device)
    return _index_call(streams, capacities, max_fragments, lambda *a: lib().smm_index(ctx, *a))


def index_streams_host(streams, capacities=None, max_fragments=None):
    """index_streams on the CPU (smm_index_host): the same rule as a scalar loop, no device."""
    return _index_call(streams, capacities, max_fragments, lib().smm_index_host)


def _uncompress_building(buf, in_off, in_len, cap, out_off, out_len, status, out, device):
    """uncompress_streams(index="build"): the streams go up once, and the two device calls run back
    to back on one stream with the index staying in device memory."""
    import torch
    dev = torch.device("cuda", device)
    n = in_len.size
    m = int(((cap.astype(np.uint64) + BLOCK - 1) // BLOCK).sum())

    def up(a, dtype):
        return torch.from_numpy(np.array(a).view(dtype)).to(dev)  # (a copy: the packed bytes are read-only)

    with torch.cuda.device(dev):
        d_in = up(buf, np.uint8) if buf.size else torch.zeros(1, dtype=torch.uint8, device=dev)
        d_in_off, d_in_len, d_cap = up(in_off, np.int64), up(in_len, np.int32), up(cap, np.int32)
        d_out_off = up(out_off, np.int64)
        d_out = torch.empty(out.size, dtype=torch.uint8, device=dev)
        d_out_len = torch.zeros(n, dtype=torch.int32, device=dev)
        d_status = torch.zeros(n, dtype=torch.int32, device=dev)
        d_first = torch.zeros(n + 1, dtype=torch.int32, device=dev)
        d_pos = torch.zeros(max(m, 1), dtype=torch.int32, device=dev)
        d_built = torch.zeros(n, dtype=torch.uint8, device=dev)
        index_streams_device(d_in, d_in_off, d_in_len, m, d_first, d_pos, d_built, d_status, d_out_cap=d_cap)
        uncompress_streams_device(d_in, d_in_off, d_in_len, m, d_out, d_out_off, d_cap, d_out_len, d_status, d_first, d_pos)
        out_len[:] = d_out_len.cpu().numpy().view(np.uint32)
        status[:] = d_status.cpu().numpy()
        out[:] = d_out.cpu().numpy()


def uncompress_streams(streams, index=None, capacities=None, device=0):
    """Decode independent raw Snappy streams of any length in one call on the GPU; returns (list
    of bytes-or-None, status array).  index: the (frag_first, frag_pos) compress_streams returned
    for exactly these streams -- a hint that lets every fragment decode in parallel -- or "build":
    the index is built on the device first (index_streams) and used from there."""
    n = len(streams)
    if n == 0:
        return [], np.zeros(0, np.int32)
    if isinstance(index, str) and index != "build":
        raise ValueError("index must be None, (frag_first, frag_pos) or 'build'")
    buf, in_off, in_len = pack_blocks(streams)
    cap = _capacities(streams, capacities)
    out_off = exclusive_scan(cap, total=True)
    out = np.empty(max(int(out_off[-1]), 1), dtype=np.uint8)
    out_len = np.zeros(n, np.uint32)
    status = np.zeros(n, np.int32)
    first = pos = None
    if isinstance(index, str):
        _uncompress_building(buf, in_off, in_len, cap, out_off[:-1], out_len, status, out, device)
        return collect(out, out_off, out_len, status), status
    if index is not None:
        first = np.ascontiguousarray(index[0], dtype=np.uint32)
        pos = np.ascontiguousarray(index[1], dtype=np.uint32)
        if first.size != n + 1 or pos.size < int(first[-1]):
            raise ValueError("index does not fit the streams")
        if pos.size == 0:
            pos = np.zeros(1, np.uint32)
    keep = np.zeros(1, np.uint8)
    check(lib().smm_uncompress(context(device), _addr(buf) or keep.ctypes.data, in_off.ctypes.data, in_len.ctypes.data, n,
                               out.ctypes.data, out_off.ctypes.data, cap.ctypes.data, out_len.ctypes.data,
                               status.ctypes.data, _addr(first), _addr(pos)), SnappyError)
    return collect(out, out_off, out_len, status), status


# ---- ranged decode (include/snappy_mi355x_multi_range.h) ----------------------------------------------

def range_fragment_count(lo, length):
    """The 64 KiB fragments that bytes [lo, lo + length) of a stream's content touch; 0 for length 0."""
    return lib().smm_range_fragment_count(int(lo), int(length))


def range_scratch_bytes(nranges, max_range_fragments):
    return lib().smm_range_scratch_bytes(int(nranges), int(max_range_fragments))


def _range_arrays(streams, index, ranges):
    """The host arrays of a ranged call: (buf, in_off, in_len, first, pos, range_stream, lo, len); buf and
    pos hold an element at the least."""
    buf, in_off, in_len = pack_blocks(streams)
    first = np.ascontiguousarray(index[0], dtype=np.uint32)
    pos = np.ascontiguousarray(index[1], dtype=np.uint32)
    if first.size != len(streams) + 1:
        raise ValueError("frag_first does not fit the streams")
    r = np.array([tuple(int(x) for x in t) for t in ranges], dtype=np.uint32).reshape(-1, 3)
    cols = [np.ascontiguousarray(r[:, k]) for k in range(3)]
    return (buf if buf.size else np.zeros(1, np.uint8), in_off, in_len, first,
            pos if pos.size else np.zeros(1, np.uint32), *cols)


def range_plan(streams, index, ranges, max_range_fragments=None, nentries=None):
    """The plan of uncompress_stream_ranges on the host (smm_range_plan: the device's rules, nothing
    decoded): (first, count, status, total) -- per range the touched fragments [first, first + count)
    of its stream and what is known before any of them is decoded (0, or 33), and the slots of all
    ranges.  index = (frag_first, frag_pos), of which nentries entries (default: all) may be read;
    over max_range_fragments (default: no bound) every status is 33."""
    buf, in_off, in_len, first, pos, rs, lo, ln = _range_arrays(streams, index, ranges)
    k = rs.size
    if nentries is None:
        nentries = np.asarray(index[1]).size
    if int(nentries) > np.asarray(index[1]).size:
        raise ValueError("frag_pos is shorter than nentries")
    bound = 0xFFFFFFFF if max_range_fragments is None else int(max_range_fragments)
    f = np.zeros(max(k, 1), np.uint32)
    c = np.zeros(max(k, 1), np.uint32)
    st = np.zeros(max(k, 1), np.int32)
    total = ctypes.c_uint64(0)
    rc = lib().smm_range_plan(buf.ctypes.data, _addr(in_off), _addr(in_len), len(streams), first.ctypes.data,
                              pos.ctypes.data, int(nentries), _addr(rs), _addr(lo), _addr(ln), k, bound, f.ctypes.data,
                              c.ctypes.data, st.ctypes.data, ctypes.byref(total))
    if rc not in (0, 2):  # (2: over the bound, which the statuses say)
        raise SnappyError(rc)
    return f[:k], c[:k], st[:k], int(total.value)


def uncompress_stream_ranges(streams, index, ranges, device=0):
    """Bytes [lo, lo + len) of the decoded content of streams[stream] for every (stream, lo, len) of
    `ranges`, in one call on the GPU that decodes only the 64 KiB fragments the ranges touch; a list
    of bytes.  index: the (frag_first, frag_pos) of exactly these streams, from compress_streams or
    index_streams.  A stream that no range names is not read.  Raises SnappyError with the first
    failing range's status: there is no fallback, and a stream whose index could not be built is
    decoded whole (uncompress_streams)."""
    buf, in_off, in_len, first, pos, rs, lo, ln = _range_arrays(streams, index, ranges)
    k = rs.size
    if k == 0:
        return []
    if pos.size < int(first[-1]):
        raise ValueError("index does not fit the streams")
    out_off = exclusive_scan(ln, total=True)
    out = np.empty(max(int(out_off[-1]), 1), dtype=np.uint8)
    out_len = np.zeros(k, np.uint32)
    status = np.zeros(k, np.int32)
    check(lib().smm_uncompress_ranges(context(device), buf.ctypes.data, _addr(in_off), _addr(in_len), len(streams),
                                      first.ctypes.data, pos.ctypes.data, rs.ctypes.data, lo.ctypes.data, ln.ctypes.data, k,
                                      out.ctypes.data, out_off.ctypes.data, out_len.ctypes.data, status.ctypes.data),
          SnappyError)
    _raise_first(status)
    return collect(out, out_off, out_len)


# ---- device API (torch tensors resident in HBM; asynchronous on `stream`) ---------------------

_device = device_caller(lib, context, SnappyError)


def compress_streams_device(d_in, d_in_off, d_in_len, max_fragments, d_out, d_out_off, d_out_len, d_status,
                            d_frag_first=None, d_frag_pos=None, mode="fast", stream=None, device=None):
    """smm_compress_device: d_in / d_out uint8, d_in_off / d_out_off int64, d_in_len / d_out_len /
    d_status int32 CUDA tensors (the C ABI's unsigned values, bit for bit); the index tensors
    (int32, nstreams + 1 and max_fragments entries) both or neither.  Nothing is synchronised.
    Arguments are checked first (_binding.device_caller; README, Device API).  Length not checked: d_frag_pos."""
    _device("smm_compress_device", d_out, device, stream, d_in, d_in_off, d_in_len, numel(d_in_len), int(max_fragments),
            d_out, d_out_off, d_out_len, d_status, d_frag_first, d_frag_pos, _mode(mode))


def uncompress_streams_device(d_in, d_in_off, d_in_len, max_fragments, d_out, d_out_off, d_out_cap, d_out_len, d_status,
                              d_frag_first=None, d_frag_pos=None, stream=None, device=None):
    """smm_uncompress_device (tensor types as in compress_streams_device).  max_fragments: the
    entries of d_frag_pos.  Nothing is synchronised.
    Arguments are checked first (_binding.device_caller; README, Device API).  Length not checked: d_frag_pos."""
    _device("smm_uncompress_device", d_out, device, stream, d_in, d_in_off, d_in_len, numel(d_in_len),
            int(max_fragments), d_out, d_out_off, d_out_cap, d_out_len, d_status, d_frag_first, d_frag_pos)


def index_streams_device(d_in, d_in_off, d_in_len, max_fragments, d_frag_first, d_frag_pos, d_built, d_status,
                         d_out_cap=None, stream=None, device=None):
    """smm_index_device (tensor types as in compress_streams_device; d_built uint8, nstreams
    entries; d_frag_pos max_fragments entries; d_out_cap None: no cap).  Nothing is synchronised.
    Arguments are checked first (_binding.device_caller; README, Device API).  Length not checked: d_frag_pos."""
    _device("smm_index_device", d_in, device, stream, d_in, d_in_off, d_in_len, numel(d_in_len), int(max_fragments),
            d_out_cap, d_frag_first, d_frag_pos, d_built, d_status)


def uncompress_stream_ranges_device(d_in, d_in_off, d_in_len, d_frag_first, d_frag_pos, d_range_stream, d_lo, d_len,
                                    max_range_fragments, d_out, d_out_off, d_out_len, d_status, nentries=None,
                                    stream=None, device=None):
    """smm_uncompress_ranges_device (tensor types as in compress_streams_device; d_range_stream, d_lo,
    d_len, d_out_len and d_status int32 with an entry per range, d_out_off int64).  nentries: the
    entries of d_frag_pos (default: all of the tensor).  max_range_fragments: at least the sum of
    range_fragment_count over the ranges.  Nothing is synchronised.
    Arguments are checked first (_binding.device_caller; README, Device API)."""
    _device("smm_uncompress_ranges_device", d_out, device, stream, d_in, d_in_off, d_in_len, numel(d_in_len), d_frag_first,
            d_frag_pos, numel(d_frag_pos) if nentries is None else int(nentries), d_range_stream, d_lo, d_len,
            numel(d_lo), int(max_range_fragments), d_out, d_out_off, d_out_len, d_status)


def last_indexed(device=0):
    """Diagnostic: how many streams the device's last uncompress call decoded by fragments (waits
    for the device); -1 before the first call."""
    return int(lib().smm_ctx_last_indexed(context(device)))


__all__ = ["MULTI_ABI_SYMBOLS", "MODES", "compress_streams", "uncompress_streams", "compress_streams_device",
           "uncompress_streams_device", "index_streams", "index_streams_host", "index_streams_device",
           "index_bound", "INDEX_STAGE", "fragment_count", "scratch_bytes", "frag_first_of", "index_check", "last_indexed",
           "RANGE_ABI_SYMBOLS", "range_fragment_count", "range_scratch_bytes", "range_plan", "uncompress_stream_ranges",
           "uncompress_stream_ranges_device"]
