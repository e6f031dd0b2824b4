"""Kafka log segments (record batches of magic 2: .log files, fetch responses, tiered-storage
objects) whose batches are uncompressed or Snappy-compressed -- a snappy-java stream or a bare raw
stream -- each under a CRC-32C, over include/snappy_mi355x_kafka.h -- libsnappy_mi355x_kafka.so, the
companion of libsnappy_mi355x_blocks.so, libsnappy_mi355x_multi.so, libsnappy_mi355x_framing.so and
libsnappy_mi355x.so.  The batch layer only: no record is parsed, no offset or timestamp interpreted.

    uncompress_segment(data, verify_crc=True)    -> (segment of uncompressed batches, batch table)
    uncompress_segment(data, records=True)       -> (list of the batches' records, batch table)
    uncompress_segments(segments)                -> list of those   one batched call
    compress_segment(data, mode), compress_segments(segments, mode)   uncompressed batches -> snappy
    index_segment(data), segments_plan(segments), compress_plan(segments), write_batch(records, ...),
    max_segment_length(n, nbatches), stage_length(n)   (host, no device)

and, on torch tensors resident in HBM: uncompress_segments_device, compress_segments_device (no host
synchronisation), last_indexed.

A batch table is a dict of numpy arrays, one entry per batch: in_off (from the segment's first
byte), out_off (in the rewritten segment; the records alone are at + 61), len (the records'
uncompressed length), codec and status.  The package imports without this library; it is loaded on
the first call here.  No CPU fallback: every codec call needs the five HIP libraries and a device.
"""
import ctypes
import os

import numpy as np

from . import HERE, MODES, SnappyError, _in_arg, _mode
from ._binding import KAFKA, check, context_cache, device_caller, exclusive_scan, lay_out, load, numel

LIB_PATH = os.path.join(HERE, "libsnappy_mi355x_kafka.so")

SMK_ERR_TRUNCATED = 104
SMK_ERR_MAGIC = 105
SMK_ERR_LENGTH = 106
SMK_ERR_CODEC = 107
SMK_ERR_TOO_LARGE = 108
SMK_ERR_CRC = 109
BATCH_HEADER_LENGTH = 61
CODEC_NONE, CODEC_SNAPPY = 0, 2
BATCH_KEYS = ("in_off", "out_off", "len", "codec", "status")

KAFKA_ABI_SYMBOLS = tuple(KAFKA)  # exported symbols of include/snappy_mi355x_kafka.h (tests/test_kafka_host.py)


class KafkaSummary(ctypes.Structure):
    """smk_summary."""
    _fields_ = [("total_length", ctypes.c_uint64), ("valid_length", ctypes.c_uint64), ("nbatches", ctypes.c_uint32),
                ("status", ctypes.c_int32)]


_lib = None


def library_path():
    return LIB_PATH


def lib():
    """Load libsnappy_mi355x_kafka.so (raises OSError if it was not built)."""
    global _lib
    if _lib is None:
        _lib = load(LIB_PATH, KAFKA, "libsnappy_mi355x_kafka.so not built (run __graft_entry__.build())")
    return _lib


def status_message(code):
    return lib().smk_status_message(int(code)).decode()


def version():
    return lib().smk_version().decode()


class KafkaError(SnappyError):
    """A SnappyError whose message comes from smk_status_message (the SMK_ERR_* texts too); for a
    segment of a batch `index` is its number in the batch, else None."""

    def __init__(self, code, index=None):
        super().__init__(code, status_message(code))
        self.index = index


# context(device=0): the per-device smk_ctx (an smb_ctx, an smm_ctx and an smf_ctx of its own plus scratch)
_ctx, _ctx_lock, context = context_cache(lib, "smk_ctx_create", SnappyError,
                                         "no usable HIP device %d for snappy_mi355x_kafka")


# ---- host helpers (no device) ---------------------------------------------------------------

def max_segment_length(n, nbatches):
    """smk_max_segment_length: the room the encoder needs for an n-byte segment of nbatches batches."""
    return lib().smk_max_segment_length(int(n), int(nbatches))


def stage_length(n):
    """smk_stage_length: a payload's share of the encoder's stage."""
    return lib().smk_stage_length(int(n))


def index_segment(data, max_batches=None):
    """The host walk and the heads (smk_index): (KafkaSummary, dict of numpy arrays pos / length /
    codec / declared / status of the recorded batches).  max_batches=None sizes the arrays by a
    counting walk first."""
    src, n, keep = _in_arg(data)
    s = KafkaSummary()
    if max_batches is None:
        lib().smk_index(src, n, None, None, None, None, None, 0, ctypes.byref(s))
        max_batches = s.nbatches
    k = max(int(max_batches), 1)
    arrays = {"pos": np.zeros(k, np.uint64), "length": np.zeros(k, np.uint32), "codec": np.zeros(k, np.uint32),
              "declared": np.zeros(k, np.uint64), "status": np.zeros(k, np.int32)}
    lib().smk_index(src, n, *(arrays[key].ctypes.data for key in ("pos", "length", "codec", "declared", "status")),
                    int(max_batches), ctypes.byref(s))
    used = min(s.nbatches, int(max_batches))
    return s, {key: a[:used] for key, a in arrays.items()}


def segments_plan(segments, out_cap=None, max_batches=0x7FFFFFFF, max_chunks=0x7FFFFFFF):
    """smk_segments_plan, the device's decode plan on the host, for a list of segments: (rc, first,
    out_len, status, total_batches, total_chunks, total_fragments)."""
    buf, offs, lens = lay_out(segments)
    k = len(segments)
    cap = None if out_cap is None else np.ascontiguousarray(out_cap, dtype=np.uint64)
    first, out_len, status = np.zeros(k + 1, np.uint32), np.zeros(max(k, 1), np.uint64), np.zeros(max(k, 1), np.int32)
    totals = [ctypes.c_uint64(0) for _ in range(3)]
    rc = lib().smk_segments_plan(buf.ctypes.data, offs.ctypes.data, lens.ctypes.data, k, None if cap is None else cap.ctypes.data,
                                 int(max_batches), int(max_chunks), first.ctypes.data, out_len.ctypes.data, status.ctypes.data,
                                 *(ctypes.byref(t) for t in totals))
    return (int(rc), first, out_len[:k], status[:k]) + tuple(t.value for t in totals)


def compress_plan(segments, max_batches=0x7FFFFFFF):
    """smk_compress_plan for a list of segments: (rc, first, room, status, total_batches,
    total_blocks, stage_bytes)."""
    buf, offs, lens = lay_out(segments)
    k = len(segments)
    first, room, status = np.zeros(k + 1, np.uint32), np.zeros(max(k, 1), np.uint64), np.zeros(max(k, 1), np.int32)
    totals = [ctypes.c_uint64(0) for _ in range(3)]
    rc = lib().smk_compress_plan(buf.ctypes.data, offs.ctypes.data, lens.ctypes.data, k, int(max_batches), first.ctypes.data,
                                 room.ctypes.data, status.ctypes.data, *(ctypes.byref(t) for t in totals))
    return (int(rc), first, room[:k], status[:k]) + tuple(t.value for t in totals)


def write_batch(records, base_offset=0, partition_leader_epoch=0, attributes=0, tail=None):
    """smk_write_batch: one valid uncompressed batch around `records` (bytes, not interpreted).
    `tail` is the 38 bytes of the fields from lastOffsetDelta to recordsCount as they stand in a batch;
    None: no offsets, no timestamps, no producer (-1), a recordsCount of 0."""
    if tail is None:
        tail = bytes(20) + b"\xff" * 14 + bytes(4)
    tail = bytes(tail)
    if len(tail) != 38:
        raise ValueError("tail: the 38 bytes from lastOffsetDelta to recordsCount")
    src, n, keep = _in_arg(records)
    out = np.empty(BATCH_HEADER_LENGTH + n, np.uint8)
    got = ctypes.c_size_t(0)
    check(lib().smk_write_batch(int(base_offset), int(partition_leader_epoch), int(attributes), tail, src, n, out.ctypes.data,
                                out.size, ctypes.byref(got)), KafkaError)
    return out[:got.value].tobytes()


# ---- host buffers -----------------------------------------------------------------------

def _raise_first(codes):
    for i, code in enumerate(codes):
        if code:
            raise KafkaError(code, i)


def _decode_call(buf, offs, lens, caps, verify_crc, device, entries):
    k = len(lens)
    cap = np.ascontiguousarray(caps, dtype=np.uint64)
    out_off = exclusive_scan(cap, total=True)
    out = np.empty(max(int(out_off[-1]), 1), np.uint8)
    out_len, status = np.zeros(k, np.uint64), np.zeros(k, np.int32)
    first = np.zeros(k + 1, np.uint32)
    n = max(entries, 1)
    table = {"in_off": np.zeros(n, np.uint64), "out_off": np.zeros(n, np.uint64), "len": np.zeros(n, np.uint64),
             "codec": np.zeros(n, np.uint32), "status": np.zeros(n, np.int32)}
    check(lib().smk_uncompress_segments(context(device), buf.ctypes.data, offs.ctypes.data, lens.ctypes.data, k,
                                        1 if verify_crc else 0, out.ctypes.data, out_off.ctypes.data, cap.ctypes.data,
                                        out_len.ctypes.data, status.ctypes.data, first.ctypes.data, entries,
                                        *(table[key].ctypes.data for key in BATCH_KEYS)), KafkaError)
    return out, out_off, out_len, status, first, table


def uncompress_segments(segments, verify_crc=True, records=False, device=0, statuses=False):
    """Rewrite every batch of every segment of `segments` uncompressed in one batched call
    (smk_uncompress_segments): a list of (segment, batch table); with records=True of (list of the
    batches' records, batch table).  The sizes come from the host plan.  A failing segment raises
    KafkaError (its status, its number as `.index`); with statuses=True nothing is raised and the
    result is (that list, with None for a failing segment's bytes; list of statuses)."""
    segments = list(segments)
    k = len(segments)
    if not k:
        return ([], []) if statuses else []
    buf, offs, lens = lay_out(segments)
    _, _, need, pre, entries, _, _ = segments_plan(segments)
    caps = np.where(pre == 0, need, 0).astype(np.uint64)
    out, out_off, out_len, status, first, table = _decode_call(buf, offs, lens, caps, verify_crc, device, int(entries))
    codes = status.tolist()
    if not statuses:
        _raise_first(codes)
    res = []
    for t in range(k):
        lo, hi = int(first[t]), int(first[t + 1])
        mine = {key: a[lo:hi].copy() for key, a in table.items()}
        if codes[t]:
            res.append((None, mine))
            continue
        seg = out[int(out_off[t]):int(out_off[t]) + int(out_len[t])]
        if records:
            at = mine["out_off"].astype(np.int64) + BATCH_HEADER_LENGTH
            res.append(([seg[a:a + int(n)].tobytes() for a, n in zip(at, mine["len"])], mine))
        else:
            res.append((seg.tobytes(), mine))
    return (res, codes) if statuses else res


def uncompress_segment(data, verify_crc=True, records=False, device=0):
    """One segment: (the segment of uncompressed batches -- or, with records=True, the list of the
    batches' records --, its batch table)."""
    try:
        return uncompress_segments([data], verify_crc=verify_crc, records=records, device=device)[0]
    except KafkaError as e:
        raise KafkaError(e.code) from None  # (a segment alone has no number)


def compress_segments(segments, mode="fast", device=0):
    """Every uncompressed batch of every segment becomes a snappy batch (a snappy-java stream of 64 KiB
    pieces) in one batched call (smk_compress_segments); batches already compressed pass through: a
    list of bytes."""
    segments = list(segments)
    k = len(segments)
    if not k:
        return []
    buf, offs, lens = lay_out(segments)
    _, _, room, pre, _, _, _ = compress_plan(segments)
    _raise_first(pre.tolist())
    out_off = exclusive_scan(room, total=True)
    out = np.empty(max(int(out_off[-1]), 1), np.uint8)
    out_len, status = np.zeros(k, np.uint64), np.zeros(k, np.int32)
    check(lib().smk_compress_segments(context(device), buf.ctypes.data, offs.ctypes.data, lens.ctypes.data, k, out.ctypes.data,
                                      out_off.ctypes.data, room.ctypes.data, out_len.ctypes.data, status.ctypes.data,
                                      _mode(mode)), KafkaError)
    _raise_first(status.tolist())
    return [out[int(o):int(o) + int(n)].tobytes() for o, n in zip(out_off, out_len)]


def compress_segment(data, mode="fast", device=0):
    """One segment."""
    try:
        return compress_segments([data], mode=mode, device=device)[0]
    except KafkaError as e:
        raise KafkaError(e.code) from None


# ---- device API (torch tensors resident in HBM; asynchronous on `stream`) ---------------------

_device = device_caller(lib, context, KafkaError)


def uncompress_segments_device(d_in, d_in_off, d_in_len, max_batches, max_chunks, max_fragments, d_out, d_out_off, d_out_cap,
                               d_out_len, d_status, verify_crc=True, d_batch_first=None, d_batch_in_off=None, d_batch_out_off=None,
                               d_batch_len=None, d_batch_codec=None, d_batch_status=None, stream=None, device=None):
    """smk_uncompress_segments_device: segment s = d_in[d_in_off[s] : d_in_off[s] + d_in_len[s]]
    (int64 both) is rewritten uncompressed into d_out[d_out_off[s] : d_out_off[s] + d_out_cap[s]]; per
    segment d_out_len (int64) and d_status (int32).  Optional: d_batch_first int32[nsegments + 1]
    and, with max_batches entries each, d_batch_in_off, d_batch_out_off, d_batch_len (int64),
    d_batch_codec and d_batch_status (int32).  max_batches and max_chunks bound the batch
    (segments_plan); max_fragments is a speed hint.  Nothing is synchronised.
    Arguments are checked first (_binding.device_caller; README, Device API)."""
    _device("smk_uncompress_segments_device", d_out, device, stream, d_in, d_in_off, d_in_len, numel(d_in_len), int(max_batches),
            int(max_chunks), int(max_fragments), 1 if verify_crc else 0, d_out, d_out_off, d_out_cap, d_out_len, d_status,
            d_batch_first, d_batch_in_off, d_batch_out_off, d_batch_len, d_batch_codec, d_batch_status)


def compress_segments_device(d_in, d_in_off, d_in_len, max_batches, max_blocks, stage_bytes, d_out, d_out_off, d_out_len,
                             d_status, mode="fast", stream=None, device=None):
    """smk_compress_segments_device: segment s is rewritten with every uncompressed batch as a snappy
    batch at d_out[d_out_off[s]:], where max_segment_length(d_in_len[s], its batches) bytes are left
    for it; per segment d_out_len (int64) and d_status (int32).  max_batches, max_blocks and
    stage_bytes bound the batch (compress_plan).  Nothing is synchronised.
    Arguments are checked first (_binding.device_caller; README, Device API)."""
    _device("smk_compress_segments_device", d_out, device, stream, d_in, d_in_off, d_in_len, numel(d_in_len), int(max_batches),
            int(max_blocks), int(stage_bytes), d_out, d_out_off, d_out_len, d_status, _mode(mode))


def last_indexed(device=0):
    """Diagnostic (smk_ctx_last_indexed): how many snappy-java chunks and raw batches the device's
    last decode call took by fragments (waits for the device); -1 before the first call."""
    return int(lib().smk_ctx_last_indexed(context(device)))


__all__ = ["KAFKA_ABI_SYMBOLS", "MODES", "BATCH_HEADER_LENGTH", "KafkaError", "KafkaSummary", "uncompress_segment",
           "uncompress_segments", "compress_segment", "compress_segments", "index_segment", "segments_plan", "compress_plan",
           "write_batch", "max_segment_length", "stage_length", "uncompress_segments_device", "compress_segments_device",
           "last_indexed", "status_message", "version"]
