"""What the eight ctypes bindings of this package share (__init__.py, framing.py, multi.py, blocks.py, orc.py,
parquet.py, avro.py, table.py): the
prototype table of each library, the loader and the per-device context cache, the status, stream
and device rules of the device wrappers, and the layout of a batch in one host buffer.

A prototype is "<return> <arguments>", one letter per C type:

    v void        c const char* (a returned text)     p any other pointer, as an address
    i int         s sm_status / int32_t               u uint32_t     q uint64_t     z size_t
    Z size_t*     U uint32_t*    Q uint64_t*          (results the wrappers pass by reference)
    C smf_chunks*                S smf_summary* / smb_summary* / smo_summary* / smq_summary* / smt_summary* (one layout)
    B smb_chunks*                O smo_chunks*                G smq_pages*
    A sma_blocks*                Y sma_summary*

tests/test_bindings.py holds every entry against the declaration in include/*.h
(tests/test_blocks_host.py: the BLOCKS table; tests/test_orc_host.py: ORC;
tests/test_multi_range_host.py: MULTI_RANGE; tests/test_parquet_host.py: PARQUET;
tests/test_parquet_write_host.py: PARQUET_WRITE; tests/test_avro_host.py: AVRO;
tests/test_table_host.py: TABLE).
"""
import ctypes
import os
import threading

import numpy as np

INDEX_KEYS = ("type", "pay_off", "pay_len", "crc", "ulen")  # smf_chunks' arrays, in its order


class Chunks(ctypes.Structure):
    """smf_chunks: five parallel arrays, one entry per data chunk."""
    _fields_ = [(k, ctypes.c_void_p) for k in INDEX_KEYS]


class BlockChunks(ctypes.Structure):
    """smb_chunks: three parallel arrays, one entry per chunk."""
    _fields_ = [(k, ctypes.c_void_p) for k in ("pay_off", "pay_len", "ulen")]


class OrcChunks(ctypes.Structure):
    """smo_chunks: four parallel arrays, one entry per chunk."""
    _fields_ = [(k, ctypes.c_void_p) for k in ("pay_off", "pay_len", "ulen", "original")]


PAGE_KEYS = ("hdr_off", "hdr_len", "body_len", "usize", "levels", "out_off", "num_values", "type", "encoding", "flags", "crc")


class Pages(ctypes.Structure):
    """smq_pages: eleven parallel arrays, one entry per page."""
    _fields_ = [(k, ctypes.c_void_p) for k in PAGE_KEYS]


AVRO_BLOCK_KEYS = ("pay_off", "pay_len", "ulen", "count", "crc", "out_off")  # sma_blocks' arrays, in its order


class AvroBlocks(ctypes.Structure):
    """sma_blocks: six parallel arrays, one entry per block."""
    _fields_ = [(k, ctypes.c_void_p) for k in AVRO_BLOCK_KEYS]


class AvroSummary(ctypes.Structure):
    """sma_summary: Summary's three fields (nblocks for nchunks), then the objects, the header's length and the marker."""
    _fields_ = [("total_length", ctypes.c_uint64), ("nblocks", ctypes.c_uint32), ("status", ctypes.c_int32),
                ("objects", ctypes.c_uint64), ("header_length", ctypes.c_uint64), ("sync", ctypes.c_uint8 * 16)]


class Summary(ctypes.Structure):
    """smf_summary, and smb_summary, smo_summary and smq_summary (npages for nchunks) with the same fields."""
    _fields_ = [("total_length", ctypes.c_uint64), ("nchunks", ctypes.c_uint32), ("status", ctypes.c_int32)]


CTYPES = {
    "v": None, "c": ctypes.c_char_p, "p": ctypes.c_void_p, "i": ctypes.c_int, "s": ctypes.c_int32,
    "u": ctypes.c_uint32, "q": ctypes.c_uint64, "z": ctypes.c_size_t, "Z": ctypes.POINTER(ctypes.c_size_t),
    "U": ctypes.POINTER(ctypes.c_uint32), "Q": ctypes.POINTER(ctypes.c_uint64), "C": ctypes.POINTER(Chunks),
    "S": ctypes.POINTER(Summary), "B": ctypes.POINTER(BlockChunks), "O": ctypes.POINTER(OrcChunks),
    "G": ctypes.POINTER(Pages), "A": ctypes.POINTER(AvroBlocks), "Y": ctypes.POINTER(AvroSummary),
}

RAW = {  # include/snappy_mi355x.h
    "sm_status_message": "c s",
    "sm_max_compressed_length": "z z",
    "sm_uncompressed_length": "s pzZ",
    "sm_parse32": "s pzzUZ",
    "sm_encode32": "z pu",
    "sm_ctx_create": "p i",
    "sm_ctx_destroy": "v p",
    "sm_ctx_stream": "p p",
    "sm_compress": "s ppzpZi",
    "sm_uncompress": "s ppzpZ",
    "sm_compress_batch_device": "s ppppupppip",
    "sm_uncompress_batch_device": "s ppppupppppp",
    "sm_compress_batch": "s ppppupppi",
    "sm_uncompress_batch": "s ppppuppppp",
    "sm_version": "c",
    "sm_compress_fragments_device": "s ppppupppqip",
    "sm_batch_parts_plan": "v uuUU",
    "sm_ctx_last_batch_parts": "i p",
    "sm_ctx_last_path": "i p",
    "sm_ctx_set_small_decode": "s pi",
    "sm_ctx_set_split_compress": "s pi",
    "sm_ctx_last_compress_split": "i p",
    "sm_find_match_length": "s pzzzzZ",
    "sm_validate_batch_device": "s ppppupp",
    "sm_uncompressed_length_batch_device": "s ppppuppp",
    "sm_validate_compressed_buffer": "s ppz",
    "sm_compress_batch_sharded": "s pipppupppi",
    "sm_uncompress_batch_sharded": "s pipppuppppp",
    "sm_uncompress_fragments_device": "s ppppupppppp",
    "sm_place_fragments_device": "s ppppupqipqppp",
    # snappy-c.h shape (test/libsnappy.jl:5-30): (char*, size_t, char*, size_t*) -> int
    "sm_snappy_compress": "s pzpZ",
    "sm_snappy_uncompress": "s pzpZ",
    "sm_snappy_max_compressed_length": "z z",
    "sm_snappy_uncompressed_length": "s pzZ",
    "sm_snappy_validate_compressed_buffer": "s pz",
    "sm_snappy_set_mode": "s i",
}

FRAMING_BASE = {  # include/snappy_mi355x_framing.h
    "smf_status_message": "c s",
    "smf_version": "c",
    "smf_max_framed_length": "z z",
    "smf_crc32c": "u pz",
    "smf_crc32c_mask": "u u",
    "smf_index": "s pzCuS",
    "smf_uncompressed_length": "s pzZ",
    "smf_ctx_create": "p i",
    "smf_ctx_destroy": "v p",
    "smf_crc32c_batch_device": "s ppppupip",
    "smf_compress_device": "s ppqpqppip",
    "smf_index_device": "s ppqCupp",
    "smf_uncompressed_length_device": "s ppqppp",
    "smf_uncompress_chunks_device": "s ppCupqpppp",
    "smf_uncompress_device": "s ppqpqppp",
    "smf_compress": "s ppzpZi",
    "smf_uncompress": "s ppzpZ",
    "smf_validate": "s ppz",
}
FRAMING_RANGE = {  # the seek index and the ranged decode
    "smf_chunk_offsets": "s pup",
    "smf_range_chunk_count": "q qq",
    "smf_range_plan": "s CpuqppuupppQ",
    "smf_range_scratch_bytes": "z uu",
    "smf_chunk_offsets_device": "s ppupp",
    "smf_compress_indexed_device": "s ppqpqppiCpupp",
    "smf_uncompress_ranges_device": "s ppqCpuppuuppppp",
    "smf_uncompress_range": "s ppzqqpZ",
}
FRAMING_STREAMS = {  # a batch of streams per call
    "smf_max_data_chunks": "q q",
    "smf_streams_plan": "s pppupupppQ",
    "smf_streams_scratch_bytes": "z uu",
    "smf_uncompress_streams_device": "s ppppuupppppppp",
    "smf_compress_streams_device": "s ppppuuppppip",
    "smf_compress_streams": "s ppppuppppi",
    "smf_uncompress_streams": "s ppppuppppp",
}
FRAMING = {**FRAMING_BASE, **FRAMING_RANGE, **FRAMING_STREAMS}

MULTI = {  # include/snappy_mi355x_multi.h
    "smm_ctx_create": "p i",
    "smm_ctx_destroy": "v p",
    "smm_version": "c",
    "smm_status_message": "c s",
    "smm_fragment_count": "u q",
    "smm_scratch_bytes": "z uu",
    "smm_index_check": "s pppuupppp",
    "smm_compress_device": "s ppppuuppppppip",
    "smm_uncompress_device": "s ppppuupppppppp",
    "smm_ctx_last_indexed": "i p",
    "smm_compress": "s ppppuppppppi",
    "smm_uncompress": "s ppppuppppppp",
    "smm_index_host": "s pppuuppppp",
    "smm_index_device": "s ppppuupppppp",
    "smm_index": "s ppppuuppppp",
}

MULTI_RANGE = {  # include/snappy_mi355x_multi_range.h: the ranged decode, exported by the multi library
    "smm_range_fragment_count": "u uu",
    "smm_range_scratch_bytes": "z uu",
    "smm_range_plan": "s pppuppupppuupppQ",
    "smm_uncompress_ranges_device": "s ppppuppupppuuppppp",
    "smm_uncompress_ranges": "s ppppupppppupppp",
}

BLOCKS = {  # include/snappy_mi355x_blocks.h
    "smb_status_message": "c s",
    "smb_version": "c",
    "smb_max_length": "z zi",
    "smb_max_chunks": "q qi",
    "smb_index": "s pziBuS",
    "smb_uncompressed_length": "s pziZ",
    "smb_streams_plan": "s pppuipupppQQ",
    "smb_streams_scratch_bytes": "z uuu",
    "smb_ctx_create": "p i",
    "smb_ctx_destroy": "v p",
    "smb_ctx_last_indexed": "i p",
    "smb_uncompress_streams_device": "s pipppuuupppppppp",
    "smb_compress_streams_device": "s pipppuuppppip",
    "smb_compress_streams": "s pipppuppppi",
    "smb_uncompress_streams": "s pipppuppppp",
}

ORC = {  # include/snappy_mi355x_orc.h
    "smo_status_message": "c s",
    "smo_version": "c",
    "smo_max_length": "z zu",
    "smo_max_chunks": "q q",
    "smo_index": "s pzuOuS",
    "smo_uncompressed_length": "s pzuZ",
    "smo_streams_plan": "s pppuupupppQQ",
    "smo_streams_scratch_bytes": "z uuuu",
    "smo_ctx_create": "p i",
    "smo_ctx_destroy": "v p",
    "smo_ctx_last_indexed": "i p",
    "smo_uncompress_streams_device": "s pupppuuupppppppp",
    "smo_compress_streams_device": "s pupppuuppppip",
    "smo_compress_streams": "s pupppuppppi",
    "smo_uncompress_streams": "s pupppuppppp",
}

PARQUET = {  # include/snappy_mi355x_parquet.h
    "smq_status_message": "c s",
    "smq_version": "c",
    "smq_max_pages": "q q",
    "smq_index": "s pzGuS",
    "smq_uncompressed_length": "s pzZ",
    "smq_chunks_plan": "s pppupupppQQ",
    "smq_chunks_scratch_bytes": "z uuu",
    "smq_ctx_create": "p i",
    "smq_ctx_destroy": "v p",
    "smq_ctx_last_indexed": "i p",
    "smq_uncompress_chunks_device": "s ppppuuuippppppGpp",
    "smq_crc32_device": "s ppppupp",
    "smq_uncompress_chunks": "s ppppuippppp",
}

PARQUET_WRITE = {  # include/snappy_mi355x_parquet_write.h: the page encoder, exported by the parquet library
    "smqe_max_chunk_length": "q qq",
    "smqe_stage_bound": "q qq",
    "smqe_rewrite_header": "s pzqupzZ",
    "smqe_index": "s pzGpuS",
    "smqe_chunks_plan": "s pppuupppQQQ",
    "smqe_scratch_bytes": "z uuq",
    "smqe_compress_chunks_device": "s ppppuuquppppppGpip",
    "smqe_compress_chunks": "s ppppupppppi",
}

AVRO = {  # include/snappy_mi355x_avro.h
    "sma_status_message": "c s",
    "sma_version": "c",
    "sma_max_blocks": "q q",
    "sma_max_block_length": "q q",
    "sma_stage_length": "q q",
    "sma_index": "s pzipAuY",
    "sma_uncompressed_length": "s pzipZ",
    "sma_streams_plan": "s pppuippuppppQQ",
    "sma_streams_scratch_bytes": "z uuuq",
    "sma_find_sync": "s ppppuppup",
    "sma_write_header": "s pzppuppzZ",
    "sma_ctx_create": "p i",
    "sma_ctx_destroy": "v p",
    "sma_ctx_last_indexed": "i p",
    "sma_uncompress_streams_device": "s pippppuuuipppppppApp",
    "sma_find_sync_device": "s pppppuppupp",
    "sma_compress_streams_device": "s pppppppppuuquppppip",
    "sma_uncompress_streams": "s pippppuipppppp",
    "sma_compress_streams": "s pppppppppuppppi",
}

TABLE = {  # include/snappy_mi355x_table.h (smt_summary has Summary's layout)
    "smt_status_message": "c s",
    "smt_version": "c",
    "smt_footer": "s pzQQQQ",
    "smt_index_bound": "s pzQ",
    "smt_max_blocks": "q q",
    "smt_walk_index": "s pzqppuS",
    "smt_block_head": "s pzqqUQ",
    "smt_max_block_length": "q q",
    "smt_stage_length": "q q",
    "smt_tables_scratch_bytes": "z uuquq",
    "smt_write_tail": "s ppuppqpzZ",
    "smt_ctx_create": "p i",
    "smt_ctx_destroy": "v p",
    "smt_ctx_last_indexed": "i p",
    "smt_index_tables_device": "s ppppuuqippppp",
    "smt_uncompress_blocks_device": "s ppppuuipppppp",
    "smt_uncompress_tables_device": "s ppppuuquipppppppppppp",
    "smt_compress_blocks_device": "s pppppuuquppppppip",
    "smt_uncompress_tables": "s ppppuippppppupppp",
    "smt_uncompress_blocks": "s ppzppuippppp",
    "smt_compress_blocks": "s pppppuppppppi",
}


def prototype(sig):
    """(restype, argtypes) of a table entry."""
    ret, _, args = sig.partition(" ")
    return CTYPES[ret], [CTYPES[a] for a in args]


def load(path, table, not_built=None):
    """The library at `path` with the prototypes of `table` set.  not_built: the OSError text for
    a path that does not exist (None: whatever the dynamic loader says)."""
    if not_built is not None and not os.path.exists(path):
        raise OSError(not_built)
    L = ctypes.CDLL(path)
    for name, sig in table.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = prototype(sig)
    return L


def context_cache(lib, create, error, no_device):
    """The contexts of one library, made on first use: (cache, lock, context).  context(device) is
    cache[device]: that device's own context, or for a tuple (name, device, k) a further context of
    the same device.  `create` names the library's constructor; without a usable device
    error(32, no_device % device) is raised."""
    cache, lock = {}, threading.Lock()

    def context(device=0):
        """The library's context on `device` (a HIP stream and scratch of its own), made on the first
        call.  Raises if no device is usable."""
        with lock:
            c = cache.get(device)
            if c is None:
                index = device[1] if isinstance(device, tuple) else device
                c = getattr(lib(), create)(index)
                if not c:
                    raise error(32, no_device % index)
                cache[device] = c
        return c

    return cache, lock, context


# ---- device wrappers (torch tensors resident in HBM) ------------------------------------------

def check(st, error):
    if st:
        raise error(st)


def stream_handle(stream, dev):
    """The hipStream_t of a wrapper's `stream` argument: None is torch's current stream on device
    `dev`, a torch.cuda.Stream gives its handle, anything else is taken as the raw handle."""
    if stream is None:
        import torch
        stream = torch.cuda.current_stream(dev)
    return getattr(stream, "cuda_stream", stream)


def device_of(tensor, device):
    return tensor.device.index if device is None else device


def device_caller(lib, context, error):
    """call(name, where, device, stream, *args) for one library: its function `name` with the
    context of device_of(where, device) in front of args and the stream's handle behind them.
    Tensors among args go as their addresses; None, integers and byref() structures as they are.
    A status other than 0 raises error(status); with error None the status is returned."""
    def call(name, where, device, stream, *args):
        dev = device_of(where, device)
        st = getattr(lib(), name)(context(dev), *[ctypes.c_void_p(a.data_ptr()) if hasattr(a, "data_ptr") else a
                                                  for a in args], ctypes.c_void_p(stream_handle(stream, dev)))
        if error is None:
            return int(st)
        check(st, error)

    return call


# ---- a batch in one host buffer ---------------------------------------------------------------

def exclusive_scan(lens, dtype=np.uint64, total=False):
    """offs[i] = lens[0] + ... + lens[i - 1] as `dtype`; with total one more entry, the sum."""
    offs = np.zeros(len(lens) + 1, dtype)
    np.cumsum(lens, dtype=dtype, out=offs[1:])
    return offs if total else offs[:-1]


def pack(parts, len_dtype):
    """Byte buffers behind one another: (uint8 array, uint64 offsets, lengths as len_dtype)."""
    lens = np.array([memoryview(p).nbytes for p in parts], dtype=len_dtype)
    buf = np.frombuffer(b"".join(parts), np.uint8) if parts else np.zeros(0, np.uint8)
    return buf, exclusive_scan(lens), lens


def pack_blocks(blocks):
    """list of byte strings -> (packed u8 array, u64 offsets, u32 lengths)."""
    return pack([bytes(b) for b in blocks], np.uint32)


def lay_out(datas):
    """The buffers `datas` (byte strings or arrays of any dtype) behind one another: (uint8 array,
    never empty, uint64 offsets, uint64 lengths)."""
    buf, offs, lens = pack([d if isinstance(d, (bytes, bytearray, memoryview)) else
                            np.ascontiguousarray(d).view(np.uint8).reshape(-1) for d in datas], np.uint64)
    return (buf if buf.size else np.zeros(1, np.uint8)), offs, lens


def slot_offsets(in_len):
    """Fixed output slots of max_compressed_length(len) bytes (16-B aligned)."""
    n = in_len.astype(np.uint64)
    caps = (32 + n + n // 6 + 15) // 16 * 16
    return exclusive_scan(caps), caps


def collect(out, offs, lens, status=None):
    """The results of a batch as bytes, out[offs[i] : offs[i] + lens[i]] each; None where
    status[i] is not 0."""
    if status is None:
        status = [0] * len(lens)
    return [None if s else out[int(o):int(o) + int(n)].tobytes() for o, n, s in zip(offs, lens, status)]
