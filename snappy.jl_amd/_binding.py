"""What the nine ctypes bindings of this package share (__init__.py, framing.py, multi.py, blocks.py, orc.py,
parquet.py, avro.py, table.py, kafka.py): the
prototype table of each library, the loader and the per-device context cache, the status, stream
and device rules of the device wrappers, and the layout of a batch in one host buffer.

A prototype is "<return> <arguments>", one letter per C type:

    v void        c const char* (a returned text)     p any other pointer, as an address
    i int         s sm_status / int32_t               u uint32_t     q uint64_t     z size_t
    Z size_t*     U uint32_t*    Q uint64_t*          (results the wrappers pass by reference)
    C smf_chunks*                S smf_summary* / smb_summary* / smo_summary* / smq_summary* / smt_summary* (one layout)
    B smb_chunks*                O smo_chunks*                G smq_pages*
    A sma_blocks*                Y sma_summary*

A pointer of a *_device function that receives a torch tensor carries its element type, and where
the C contract ties the array's length to a count argument of the same call, a mark behind it:

    b uint8_t* / char*    w uint32_t*    d uint64_t*    t int32_t*
    r smf_summary* in device memory (16 bytes: a uint8[16] or an int64[2] tensor)
    [k]   one entry per item of argument k (ctx is argument 0): at least that many elements
    [k+]  one more than that (the `first`-style scans)
    [=c]  at least c elements

C, B, O, G and A take the same marks in a *_device function, where they receive a dict of tensors;
the element type of each of their arrays stands in the structure's `elements`.  An array without a
mark is bounded by a max_* argument or by a value only the device knows: its length is not checked.
device_caller() judges every tensor against its entry before anything is loaded or launched.

tests/test_bindings.py holds every entry against the declaration in include/*.h
(tests/test_blocks_host.py: the BLOCKS table; tests/test_orc_host.py: ORC;
tests/test_multi_range_host.py: MULTI_RANGE; tests/test_parquet_host.py: PARQUET;
tests/test_parquet_write_host.py: PARQUET_WRITE; tests/test_avro_host.py: AVRO;
tests/test_table_host.py: TABLE; tests/test_kafka_host.py: KAFKA).
"""
import ctypes
import os
import re
import sys
import threading

import numpy as np

INDEX_KEYS = ("type", "pay_off", "pay_len", "crc", "ulen")  # smf_chunks' arrays, in its order


class Chunks(ctypes.Structure):
    """smf_chunks: five parallel arrays, one entry per data chunk."""
    _fields_ = [(k, ctypes.c_void_p) for k in INDEX_KEYS]
    elements = "bdwww"


class BlockChunks(ctypes.Structure):
    """smb_chunks: three parallel arrays, one entry per chunk."""
    _fields_ = [(k, ctypes.c_void_p) for k in ("pay_off", "pay_len", "ulen")]
    elements = "dww"


class OrcChunks(ctypes.Structure):
    """smo_chunks: four parallel arrays, one entry per chunk."""
    _fields_ = [(k, ctypes.c_void_p) for k in ("pay_off", "pay_len", "ulen", "original")]
    elements = "dwwb"


PAGE_KEYS = ("hdr_off", "hdr_len", "body_len", "usize", "levels", "out_off", "num_values", "type", "encoding", "flags", "crc")


class Pages(ctypes.Structure):
    """smq_pages: eleven parallel arrays, one entry per page."""
    _fields_ = [(k, ctypes.c_void_p) for k in PAGE_KEYS]
    elements = "dwwwwdtttww"


AVRO_BLOCK_KEYS = ("pay_off", "pay_len", "ulen", "count", "crc", "out_off")  # sma_blocks' arrays, in its order


class AvroBlocks(ctypes.Structure):
    """sma_blocks: six parallel arrays, one entry per block."""
    _fields_ = [(k, ctypes.c_void_p) for k in AVRO_BLOCK_KEYS]
    elements = "dwwdwd"


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
    "b": ctypes.c_void_p, "w": ctypes.c_void_p, "d": ctypes.c_void_p, "t": ctypes.c_void_p, "r": ctypes.c_void_p,
}

# a tensor's element letter: (the C element type, the numpy dtype of the same bits, the torch dtypes taken for it)
ELEMENTS = {
    "b": ("uint8_t", np.uint8, ("uint8",)),
    "w": ("uint32_t", np.uint32, ("int32", "uint32")),
    "d": ("uint64_t", np.uint64, ("int64", "uint64")),
    "t": ("int32_t", np.int32, ("int32",)),
}
SUMMARY_ELEMENTS = {"uint8": 16, "int64": 2, "uint64": 2}  # r: the torch dtypes taken, and the elements that hold 16 bytes
ARRAYS = {"C": Chunks, "B": BlockChunks, "O": OrcChunks, "G": Pages, "A": AvroBlocks}  # the structures of parallel arrays


def field_dtypes(struct, signed=False):
    """{field: numpy dtype} of a structure of parallel arrays, as the C ABI declares them; signed:
    as torch tensors hold the same bits (int32 for uint32, int64 for uint64)."""
    out = {}
    for (key, _), e in zip(struct._fields_, struct.elements):
        dtype = np.dtype(ELEMENTS[e][1])
        out[key] = np.dtype(dtype.name.lstrip("u")).type if signed and dtype.itemsize > 1 else dtype.type
    return out

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
    "sm_compress_batch_device": "s pbd[4]w[4]ubd[4]w[4]ip",
    "sm_uncompress_batch_device": "s pbd[4]w[4]ubd[4]w[4]w[4]t[4]p",
    "sm_compress_batch": "s ppppupppi",
    "sm_uncompress_batch": "s ppppuppppp",
    "sm_version": "c",
    "sm_compress_fragments_device": "s pbd[4]w[4]ubd[4]w[4]qip",
    "sm_batch_parts_plan": "v uuUU",
    "sm_ctx_last_batch_parts": "i p",
    "sm_ctx_last_path": "i p",
    "sm_ctx_set_small_decode": "s pi",
    "sm_ctx_set_split_compress": "s pi",
    "sm_ctx_last_compress_split": "i p",
    "sm_find_match_length": "s pzzzzZ",
    "sm_validate_batch_device": "s pbd[4]w[4]ut[4]p",
    "sm_uncompressed_length_batch_device": "s pbd[4]w[4]uw[4]t[4]p",
    "sm_validate_compressed_buffer": "s ppz",
    "sm_compress_batch_sharded": "s pipppupppi",
    "sm_uncompress_batch_sharded": "s pipppuppppp",
    "sm_uncompress_fragments_device": "s pbd[4]w[4]ubd[4]w[4]w[4]t[4]p",
    "sm_place_fragments_device": "s pbd[4]w[4]ud[4]qibqd[4]t[=1]p",
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
    "smf_crc32c_batch_device": "s pbd[4]w[4]uw[4]ip",
    "smf_compress_device": "s pbqbqdtip",
    "smf_index_device": "s pbqCurp",
    "smf_uncompressed_length_device": "s pbqdtp",
    "smf_uncompress_chunks_device": "s pbC[3]ubqt[3]dtp",
    "smf_uncompress_device": "s pbqbqdtp",
    "smf_compress": "s ppzpZi",
    "smf_uncompress": "s ppzpZ",
    "smf_validate": "s ppz",
}
FRAMING_RANGE = {  # the seek index and the ranged decode
    "smf_chunk_offsets": "s pup",
    "smf_range_chunk_count": "q qq",
    "smf_range_plan": "s CpuqppuupppQ",
    "smf_range_scratch_bytes": "z uu",
    "smf_chunk_offsets_device": "s pw[2]ud[2+]p",
    "smf_compress_indexed_device": "s pbqbqdtiCd[=1]uwp",
    "smf_uncompress_ranges_device": "s pbqC[5]d[5+]ud[8]d[8]uubd[8]d[8]t[8]p",
    "smf_uncompress_range": "s ppzqqpZ",
}
FRAMING_STREAMS = {  # a batch of streams per call
    "smf_max_data_chunks": "q q",
    "smf_streams_plan": "s pppupupppQ",
    "smf_streams_scratch_bytes": "z uu",
    "smf_uncompress_streams_device": "s pbd[4]d[4]uubd[4]d[4]d[4]t[4]w[4+]tp",
    "smf_compress_streams_device": "s pbd[4]d[4]uubd[4]d[4]t[4]ip",
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
    "smm_compress_device": "s pbd[4]w[4]uubd[4]w[4]t[4]w[4+]wip",
    "smm_uncompress_device": "s pbd[4]w[4]uubd[4]w[4]w[4]t[4]w[4+]wp",
    "smm_ctx_last_indexed": "i p",
    "smm_compress": "s ppppuppppppi",
    "smm_uncompress": "s ppppuppppppp",
    "smm_index_host": "s pppuuppppp",
    "smm_index_device": "s pbd[4]w[4]uuw[4]w[4+]wb[4]t[4]p",
    "smm_index": "s ppppuuppppp",
}

MULTI_RANGE = {  # include/snappy_mi355x_multi_range.h: the ranged decode, exported by the multi library
    "smm_range_fragment_count": "u uu",
    "smm_range_scratch_bytes": "z uu",
    "smm_range_plan": "s pppuppupppuupppQ",
    "smm_uncompress_ranges_device": "s pbd[4]w[4]uw[4+]w[7]uw[11]w[11]w[11]uubd[11]w[11]t[11]p",
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
    "smb_uncompress_streams_device": "s pibd[5]d[5]uuubd[5]d[5]d[5]t[5]w[5+]tp",
    "smb_compress_streams_device": "s pibd[5]d[5]uubd[5]d[5]t[5]ip",
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
    "smo_uncompress_streams_device": "s pubd[5]d[5]uuubd[5]d[5]d[5]t[5]w[5+]tp",
    "smo_compress_streams_device": "s pubd[5]d[5]uubd[5]d[5]t[5]ip",
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
    "smq_uncompress_chunks_device": "s pbd[4]d[4]uuuibd[4]d[4]d[4]t[4]w[4+]Gtp",
    "smq_crc32_device": "s pbd[4]d[4]uw[4]p",
    "smq_uncompress_chunks": "s ppppuippppp",
}

PARQUET_WRITE = {  # include/snappy_mi355x_parquet_write.h: the page encoder, exported by the parquet library
    "smqe_max_chunk_length": "q qq",
    "smqe_stage_bound": "q qq",
    "smqe_rewrite_header": "s pzqupzZ",
    "smqe_index": "s pzGpuS",
    "smqe_chunks_plan": "s pppuupppQQQ",
    "smqe_scratch_bytes": "z uuq",
    "smqe_compress_chunks_device": "s pbd[4]d[4]uuqubd[4]d[4]d[4]t[4]w[4+]Gtip",
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
    "sma_uncompress_streams_device": "s pibd[6]d[6]buuuibd[6]d[6]d[6]t[6]d[6]w[6+]Atp",
    "sma_find_sync_device": "s pbd[5]d[5]buw[8]d[8]ud[8]p",
    "sma_compress_streams_device": "s pbw[9+]dwdbd[9]d[9]uuqubd[9]d[9]t[9]ip",
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
    "smt_index_tables_device": "s pbd[4]d[4]uuqiw[4+]ddt[4]p",
    "smt_uncompress_blocks_device": "s pbd[4]d[4]uuibd[4]d[4]d[4]t[4]p",
    "smt_uncompress_tables_device": "s pbd[4]d[4]uuquibd[4]d[4]d[4]t[4]w[4+]ddddtp",
    "smt_compress_blocks_device": "s pbw[5+]dwuuqubd[5]ddd[5]t[5]ip",
    "smt_uncompress_tables": "s ppppuippppppupppp",
    "smt_uncompress_blocks": "s ppzppuippppp",
    "smt_compress_blocks": "s pppppuppppppi",
}

KAFKA = {  # include/snappy_mi355x_kafka.h (smk_summary is kafka.py's own structure, passed by reference)
    "smk_status_message": "c s",
    "smk_version": "c",
    "smk_index": "s pzpppppup",
    "smk_segments_plan": "s pppupuupppQQQ",
    "smk_compress_plan": "s pppuupppQQQ",
    "smk_max_segment_length": "q qq",
    "smk_stage_length": "q q",
    "smk_segments_scratch_bytes": "z uuuq",
    "smk_write_batch": "s quuppzpzZ",
    "smk_ctx_create": "p i",
    "smk_ctx_destroy": "v p",
    "smk_ctx_last_indexed": "i p",
    "smk_uncompress_segments_device": "s pbd[4]d[4]uuuuibd[4]d[4]d[4]t[4]w[4+]d[5]d[5]d[5]w[5]t[5]p",
    "smk_compress_segments_device": "s pbd[4]d[4]uuuqbd[4]d[4]t[4]ip",
    "smk_uncompress_segments": "s ppppuippppppuppppp",
    "smk_compress_segments": "s ppppupppppi",
}


_ARGUMENT = re.compile(r"([A-Za-z])(?:\[(=?)(\d+)(\+?)\])?")


def arguments(sig):
    """(return letter, [(letter, mark)]) of a table entry; mark: None, (k, extra) for [k] and [k+]
    -- at least args[k] + extra elements --, or (None, c) for [=c]."""
    ret, _, args = sig.partition(" ")
    out, at = [], 0
    for m in _ARGUMENT.finditer(args):
        assert m.start() == at, sig
        at = m.end()
        letter, fixed, k, plus = m.groups()
        out.append((letter, None if k is None else (None, int(k)) if fixed else (int(k), 1 if plus else 0)))
    assert at == len(args), sig
    return ret, out


def prototype(sig):
    """(restype, argtypes) of a table entry."""
    ret, args = arguments(sig)
    return CTYPES[ret], [CTYPES[a] for a, _ in args]


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


def numel(tensor):
    """tensor.numel() for a wrapper that takes a count or a capacity from an argument; 0 for what is no
    tensor, which check_arguments then refuses.  None is refused here: such an argument is never
    optional, and check_arguments lets None pass."""
    if tensor is None:
        raise TypeError("an argument that gives a count or a capacity of the call is None: expected a tensor")
    return tensor.numel() if hasattr(tensor, "numel") else 0


TABLES = (RAW, FRAMING, MULTI, MULTI_RANGE, BLOCKS, ORC, PARQUET, PARQUET_WRITE, AVRO, TABLE)
MORE_TABLES = (KAFKA,)  # the libraries behind those: searched after TABLES, judged alike
_BYREF = type(ctypes.byref(ctypes.c_int()))
_plans, _dtypes = {}, {}


def tensor_plan(name):
    """[(position, letter, mark)] of the arguments of the C function `name` that receive tensors,
    from its table entry; position counts as the header does (ctx is 0)."""
    plan = _plans.get(name)
    if plan is None:
        sig = next(t[name] for t in TABLES + MORE_TABLES if name in t)
        plan = _plans[name] = [(k, letter, mark) for k, (letter, mark) in enumerate(arguments(sig)[1])
                               if letter in ELEMENTS or letter in ARRAYS or letter == "r"]
    return plan


def _accepted(letter):
    """The torch dtypes taken for an element letter (torch is imported on the first call)."""
    got = _dtypes.get(letter)
    if got is None:
        torch = sys.modules.get("torch") or __import__("torch")
        names = SUMMARY_ELEMENTS if letter == "r" else ELEMENTS[letter][2]
        got = _dtypes[letter] = {getattr(torch, n): n for n in names if hasattr(torch, n)}
    return got


def _where(name, position, field):
    return "%s argument %d%s" % (name, position, "" if field is None else ", field %s" % field)


def judge(name, position, field, letter, need, a):
    """Checks 1 to 3 of one argument at a tensor's place: `a` is None, an integer (a raw address) or
    a byref() object, which pass, or a tensor of the letter's dtype (TypeError), one-dimensional
    and contiguous (ValueError) with at least `need` elements (ValueError; None: any number)."""
    if a is None or isinstance(a, (int, _BYREF)):
        return
    taken = _accepted(letter)
    if not hasattr(a, "data_ptr") or a.dtype not in taken:
        ctype = "smf_summary, 16 bytes" if letter == "r" else ELEMENTS[letter][0]
        given = "a %s tensor" % (a.dtype,) if hasattr(a, "data_ptr") else type(a).__name__
        raise TypeError("%s: expected a tensor of dtype %s (%s), given %s"
                        % (_where(name, position, field), " or ".join(taken.values()), ctype, given))
    if a.dim() != 1 or not (a.is_contiguous() or a.numel() == 0):
        raise ValueError("%s: expected a one-dimensional contiguous tensor, given shape %s with strides %s"
                         % (_where(name, position, field), tuple(a.shape), tuple(a.stride())))
    if letter == "r":
        need = SUMMARY_ELEMENTS[taken[a.dtype]]
    if need is not None and a.numel() < need:
        raise ValueError("%s: expected at least %d elements, given %d" % (_where(name, position, field), need, a.numel()))


def check_arguments(name, args):
    """Checks 1 to 3 of every tensor among the arguments `args` of the C function `name` (args[0] is
    its argument 1), a dict of tensors at a structure's place field by field: the first failure
    raises.  Returns [(position, field, tensor)] of the tensors, for check_devices."""
    found = []
    for k, letter, mark in tensor_plan(name):
        a = args[k - 1]
        if a is None:
            continue
        need = None if mark is None else mark[1] if mark[0] is None else int(args[mark[0] - 1]) + mark[1]
        if letter not in ARRAYS:
            judge(name, k, None, letter, need, a)
            if hasattr(a, "data_ptr"):
                found.append((k, None, a))
        elif isinstance(a, dict):
            struct = ARRAYS[letter]
            for (key, _), e in zip(struct._fields_, struct.elements):
                t = a.get(key)
                if not hasattr(t, "data_ptr"):
                    raise TypeError("%s: expected a tensor of dtype %s (%s), given %s"
                                    % (_where(name, k, key), " or ".join(_accepted(e).values()), ELEMENTS[e][0],
                                       type(t).__name__))
                judge(name, k, key, e, need, t)
                found.append((k, key, t))
        elif not isinstance(a, _BYREF):
            raise TypeError("%s: expected a dict of tensors keyed %s, given %s"
                            % (_where(name, k, None), ", ".join(n for n, _ in ARRAYS[letter]._fields_), type(a).__name__))
    return found


def check_devices(name, tensors, dev):
    """Check 4 of check_arguments' tensors: each is a CUDA tensor (TypeError) on device `dev`, the
    device the call runs on (ValueError)."""
    for k, field, t in tensors:
        d = t.device
        if d.type != "cuda":
            raise TypeError("%s: expected a CUDA tensor on device %s, given a tensor on %s" % (_where(name, k, field), dev, d))
        if d.index != dev:
            raise ValueError("%s: expected a tensor on the call's device cuda:%s, given one on %s"
                             % (_where(name, k, field), dev, d))


def device_caller(lib, context, error):
    """call(name, where, device, stream, *args) for one library: its function `name` with the
    context of device_of(where, device) in front of args and the stream's handle behind them.
    Before anything is looked up, loaded or launched every tensor among args is judged against the
    function's table entry (check_arguments, then check_devices).  Tensors then go as their
    addresses, a dict of tensors as its structure by reference; None, a Python int (a raw address;
    no other integer type) and byref() structures as they are.  A status other than 0 raises
    error(status); with error None the status is returned.

    Checked, in this order, a TypeError or ValueError naming the C function and the argument: each
    tensor's dtype, one contiguous dimension, at least as many elements as the table's mark asks
    (the arrays with an entry per block, stream, chunk, range or query of the call), a CUDA tensor
    on the call's device.  Not checked: the values in the tensors (the caller's contract: reading
    them would synchronise), and the length of arrays that carry no mark -- those bounded by a max_*
    argument or by a count only the device knows, and the byte buffers."""
    def call(name, where, device, stream, *args):
        tensors = check_arguments(name, args)
        dev = device_of(where, device)
        check_devices(name, tensors, dev[1] if isinstance(dev, tuple) else dev)  # (a further context of device dev[1])
        cargs = list(args)
        for k, letter, _ in tensor_plan(name):
            a = cargs[k - 1]
            if hasattr(a, "data_ptr"):
                cargs[k - 1] = ctypes.c_void_p(a.data_ptr())
            elif isinstance(a, dict):
                cargs[k - 1] = ctypes.byref(ARRAYS[letter](*(a[key].data_ptr() for key, _ in ARRAYS[letter]._fields_)))
        st = getattr(lib(), name)(context(dev), *cargs, ctypes.c_void_p(stream_handle(stream, dev)))
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
