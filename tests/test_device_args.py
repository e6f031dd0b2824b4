"""The argument checks of the device wrappers (snappy.jl_amd/_binding.py: check_arguments and
check_devices, run by device_caller before anything is loaded or launched).

Without a GPU: the checker against verdicts written out here, and a sweep of every device wrapper
with one well-formed set of CPU tensors in which each tensor argument in turn is swapped for a
wrong dtype, a strided view and one an element short, and each argument that gives the call its
count for what is no tensor.  None of it can reach a kernel.

On the GPU: the rejection cases with the library replaced by a recorder that no call may reach,
the marshalling of one wrapper per library into that recorder, and acceptance cases (unsigned
dtypes, offset slices between guards, arrays one element longer, an empty batch) with the real
library, decoded by the CPU oracle."""
import ctypes
import importlib

import numpy as np
import pytest

gpu = pytest.mark.gpu
MODULES = ("", ".framing", ".multi", ".blocks", ".orc", ".parquet", ".avro", ".table", ".dist")

# The arrays of the structures of parallel arrays, as include/*.h declares them: b uint8_t, i
# uint32_t / int32_t (an int32 tensor), q uint64_t (an int64 tensor).
FIELDS = {
    "C": [("type", "b"), ("pay_off", "q"), ("pay_len", "i"), ("crc", "i"), ("ulen", "i")],
    "G": [("hdr_off", "q"), ("hdr_len", "i"), ("body_len", "i"), ("usize", "i"), ("levels", "i"), ("out_off", "q"),
          ("num_values", "i"), ("type", "i"), ("encoding", "i"), ("flags", "i"), ("crc", "i")],
    "A": [("pay_off", "q"), ("pay_len", "i"), ("ulen", "i"), ("count", "q"), ("crc", "i"), ("out_off", "q")],
}

# One well-formed call of every device wrapper: two streams (blocks, chunks), three ranges or
# queries, four index entries, and max_* bounds of 4 or 5 (0 for max_fragments of a decode), so that
# no two uint32_t arguments of a call are equal and a mark that names the wrong one is seen:
# (module, wrapper, C function, tensor arguments, other arguments).  A tensor argument is
# name:position:type:elements[!need] -- position as the header counts (ctx is 0); type b, i, q or a
# structure of FIELDS; !need where the header ties the array to a count of the call: `need`
# elements are the fewest the call takes, so need - 1 must be refused; !0 for the argument whose own
# length the wrapper takes as that count (d_in_len), which cannot be short of it.
BATCH = "d_in:1:b:8 d_in_off:2:q:2!2 d_in_len:3:i:2!0 "
STREAMS = "d_in:1:b:64 d_in_off:2:q:2!2 d_in_len:3:q:2!0 "
STREAMS2 = "d_in:2:b:64 d_in_off:3:q:2!2 d_in_len:4:q:2!0 "
DECODED = "d_out:8:b:8 d_out_off:9:q:2!2 d_out_cap:10:q:2!2 d_out_len:11:q:2!2 d_status:12:i:2!2 "
CASES = [
    ("", "compress_batch_device", "sm_compress_batch_device", BATCH + "d_out:5:b:96 d_out_off:6:q:2!2 d_out_len:7:i:2!2", {}),
    ("", "compress_fragments_device", "sm_compress_fragments_device",
     BATCH + "d_out:5:b:96 d_out_off:6:q:2!2 d_out_len:7:i:2!2", {"total_len": 8}),
    ("", "uncompress_batch_device", "sm_uncompress_batch_device",
     BATCH + "d_out:5:b:8 d_out_off:6:q:2!2 d_out_cap:7:i:2!2 d_out_len:8:i:2!2 d_status:9:i:2!2", {}),
    ("", "uncompress_fragments_device", "sm_uncompress_fragments_device",
     BATCH + "d_out:5:b:8 d_out_off:6:q:2!2 d_frag_len:7:i:2!2 d_out_len:8:i:2!2 d_status:9:i:2!2", {}),
    ("", "place_fragments_device", "sm_place_fragments_device",
     "d_src:1:b:8 d_src_off:2:q:2!2 d_len:3:i:2!0 d_dst_off:5:q:2!2 d_dst:8:b:16 d_local_off:10:q:2!2 d_status:11:i:2!1",
     {"total_len": 8, "write_header": True}),
    ("", "validate_batch_device", "sm_validate_batch_device", BATCH + "d_status:5:i:2!2", {}),
    ("", "uncompressed_length_batch_device", "sm_uncompressed_length_batch_device", BATCH + "d_len:5:i:2!2 d_status:6:i:2!2", {}),
    (".framing", "crc32c_batch_device", "smf_crc32c_batch_device", "d_in:1:b:8 d_off:2:q:2!2 d_len:3:i:2!0 d_crc:5:i:2!2", {}),
    (".framing", "compress_framed_device", "smf_compress_device", "d_in:1:b:8 d_out:3:b:32 d_out_len:5:q:2 d_status:6:i:2", {}),
    (".framing", "index_framed_device", "smf_index_device", "d_in:1:b:32 arrays:3:C:2 d_summary:5:b:16!16", {}),
    (".framing", "uncompressed_length_framed_device", "smf_uncompressed_length_device",
     "d_in:1:b:32 d_len:3:q:2 d_status:4:i:2", {}),
    (".framing", "uncompress_chunks_device", "smf_uncompress_chunks_device",
     "d_in:1:b:32 arrays:2:C:2!2 d_out:4:b:8 d_chunk_status:6:i:2!2 d_out_len:7:q:2 d_status:8:i:2", {"nchunks": 2}),
    (".framing", "uncompress_framed_device", "smf_uncompress_device", "d_in:1:b:32 d_out:3:b:8 d_out_len:5:q:2 d_status:6:i:2", {}),
    (".framing", "compress_framed_indexed_device", "smf_compress_indexed_device",
     "d_in:1:b:8 d_out:3:b:32 d_out_len:5:q:2 d_status:6:i:2 arrays:8:C:2 d_chunk_off:9:q:3!1 d_nchunks:11:i:2", {}),
    (".framing", "chunk_offsets_device", "smf_chunk_offsets_device", "d_ulen:1:i:2!2 d_chunk_off:3:q:3!3", {"nchunks": 2}),
    (".framing", "uncompress_ranges_device", "smf_uncompress_ranges_device",
     "d_in:1:b:32 arrays:3:C:2!2 d_chunk_off:4:q:3!3 d_lo:6:q:3!0 d_len:7:q:3!3 d_out:10:b:8 d_out_off:11:q:3!3 "
     "d_out_len:12:q:3!3 d_range_status:13:i:3!3", {"nchunks": 2, "max_range_chunks": 4}),
    (".framing", "compress_framed_streams_device", "smf_compress_streams_device",
     STREAMS + "d_out:6:b:96 d_out_off:7:q:2!2 d_out_len:8:q:2!2 d_status:9:i:2!2", {"max_blocks": 5}),
    (".framing", "uncompress_framed_streams_device", "smf_uncompress_streams_device",
     STREAMS + "d_out:6:b:8 d_out_off:7:q:2!2 d_out_cap:8:q:2!2 d_out_len:9:q:2!2 d_status:10:i:2!2 d_chunk_first:11:i:3!3 "
     "d_chunk_status:12:i:4", {"max_chunks": 4}),
    (".multi", "compress_streams_device", "smm_compress_device",
     BATCH + "d_out:6:b:96 d_out_off:7:q:2!2 d_out_len:8:i:2!2 d_status:9:i:2!2 d_frag_first:10:i:3!3 d_frag_pos:11:i:2",
     {"max_fragments": 5}),
    (".multi", "uncompress_streams_device", "smm_uncompress_device",
     BATCH + "d_out:6:b:8 d_out_off:7:q:2!2 d_out_cap:8:i:2!2 d_out_len:9:i:2!2 d_status:10:i:2!2 d_frag_first:11:i:3!3 "
     "d_frag_pos:12:i:2", {"max_fragments": 5}),
    (".multi", "index_streams_device", "smm_index_device",
     BATCH + "d_out_cap:6:i:2!2 d_frag_first:7:i:3!3 d_frag_pos:8:i:2 d_built:9:b:2!2 d_status:10:i:2!2", {"max_fragments": 5}),
    (".multi", "uncompress_stream_ranges_device", "smm_uncompress_ranges_device",
     BATCH + "d_frag_first:5:i:3!3 d_frag_pos:6:i:4!4 d_range_stream:8:i:3!3 d_lo:9:i:3!0 d_len:10:i:3!3 d_out:13:b:8 "
     "d_out_off:14:q:3!3 d_out_len:15:i:3!3 d_status:16:i:3!3", {"max_range_fragments": 5, "nentries": 4}),
    (".blocks", "compress_block_streams_device", "smb_compress_streams_device",
     STREAMS2 + "d_out:7:b:96 d_out_off:8:q:2!2 d_out_len:9:q:2!2 d_status:10:i:2!2", {"format": "hadoop", "max_blocks": 5}),
    (".blocks", "uncompress_block_streams_device", "smb_uncompress_streams_device",
     STREAMS2 + DECODED + "d_chunk_first:13:i:3!3 d_chunk_status:14:i:4", {"format": "xerial", "max_chunks": 4, "max_fragments": 0}),
    (".orc", "compress_orc_streams_device", "smo_compress_streams_device",
     STREAMS2 + "d_out:7:b:96 d_out_off:8:q:2!2 d_out_len:9:q:2!2 d_status:10:i:2!2", {"block_size": 65536, "max_pieces": 5}),
    (".orc", "uncompress_orc_streams_device", "smo_uncompress_streams_device",
     STREAMS2 + DECODED + "d_chunk_first:13:i:3!3 d_chunk_status:14:i:4",
     {"block_size": 65536, "max_chunks": 4, "max_fragments": 0}),
    (".parquet", "uncompress_column_chunks_device", "smq_uncompress_chunks_device",
     STREAMS + DECODED + "d_page_first:13:i:3!3 d_pages:14:G:4 d_page_status:15:i:4", {"max_pages": 4, "max_fragments": 0}),
    (".parquet", "compress_column_chunks_device", "smqe_compress_chunks_device",
     STREAMS + DECODED + "d_page_first:13:i:3!3 d_pages:14:G:4 d_page_status:15:i:4",
     {"max_pages": 4, "stage_bytes": 64, "max_fragments": 5}),
    (".parquet", "crc32_device", "smq_crc32_device", "d_in:1:b:8 d_off:2:q:2!2 d_len:3:q:2!0 d_crc:5:i:2!2", {}),
    (".avro", "uncompress_avro_streams_device", "sma_uncompress_streams_device",
     STREAMS2 + "d_sync:5:b:32 d_out:10:b:8 d_out_off:11:q:2!2 d_out_cap:12:q:2!2 d_out_len:13:q:2!2 d_status:14:i:2!2 "
     "d_objects:15:q:2!2 d_block_first:16:i:3!3 d_blocks:17:A:4 d_block_status:18:i:4",
     {"kind": "blocks", "max_blocks": 4, "max_fragments": 0}),
    (".avro", "find_sync_device", "sma_find_sync_device",
     STREAMS + "d_sync:4:b:32 d_q_stream:6:i:3!0 d_q_from:7:q:3!3 d_pos:9:q:3!3", {}),
    (".avro", "compress_avro_streams_device", "sma_compress_streams_device",
     "d_in:1:b:8 d_block_first:2:i:3!3 d_block_off:3:q:2 d_block_len:4:i:2 d_block_count:5:q:2 d_sync:6:b:32 "
     "d_head_off:7:q:2!2 d_head_len:8:q:2!2 d_out:13:b:96 d_out_off:14:q:2!0 d_out_len:15:q:2!2 d_status:16:i:2!2",
     {"max_blocks": 5, "stage_bytes": 64, "max_fragments": 5}),
    (".table", "index_tables_device", "smt_index_tables_device",
     STREAMS + "d_block_first:8:i:3!3 d_handle_off:9:q:4 d_handle_size:10:q:4 d_status:11:i:2!2",
     {"max_blocks": 4, "max_index_bytes": 64}),
    (".table", "uncompress_tables_device", "smt_uncompress_tables_device",
     STREAMS + "d_out:9:b:8 d_out_off:10:q:2!2 d_out_cap:11:q:2!2 d_out_len:12:q:2!2 d_status:13:i:2!2 d_block_first:14:i:3!3 "
     "d_handle_off:15:q:4 d_handle_size:16:q:4 d_block_out_off:17:q:4 d_block_len:18:q:4 d_block_status:19:i:4",
     {"max_blocks": 4, "max_index_bytes": 64, "max_fragments": 0}),
    (".table", "uncompress_table_blocks_device", "smt_uncompress_blocks_device",
     "d_in:1:b:32 d_blk_off:2:q:2!0 d_blk_size:3:q:2!2 d_out:7:b:8 d_out_off:8:q:2!2 d_out_cap:9:q:2!2 d_out_len:10:q:2!2 "
     "d_status:11:i:2!2", {"max_fragments": 0}),
    (".table", "compress_table_blocks_device", "smt_compress_blocks_device",
     "d_in:1:b:8 d_block_first:2:i:3!3 d_block_off:3:q:2 d_block_len:4:i:2 d_out:9:b:96 d_out_off:10:q:2!0 d_handle_off:11:q:2 "
     "d_handle_size:12:q:2 d_out_len:13:q:2!2 d_status:14:i:2!2", {"max_blocks": 5, "stage_bytes": 64, "max_fragments": 5}),
]
# one wrapper per library for the GPU tests, and the counts and scalars its C call must receive: {position: value}
ONE_PER_LIBRARY = {
    "sm_compress_batch_device": {4: 2, 8: 1},
    "smf_uncompress_ranges_device": {2: 32, 5: 2, 8: 3, 9: 4},
    "smm_uncompress_ranges_device": {4: 2, 7: 4, 11: 3, 12: 5},
    "smb_uncompress_streams_device": {1: 1, 5: 2, 6: 4, 7: 0},
    "smo_uncompress_streams_device": {1: 65536, 5: 2, 6: 4, 7: 0},
    "smq_uncompress_chunks_device": {4: 2, 5: 4, 6: 0, 7: 1},
    "sma_uncompress_streams_device": {1: 1, 6: 2, 7: 4, 8: 0, 9: 1},
    "smt_uncompress_tables_device": {4: 2, 5: 4, 6: 64, 7: 0, 8: 1},
}
TORCH = {"b": "uint8", "i": "int32", "q": "int64"}
WRONG = {"b": "int32", "i": "int64", "q": "int32"}  # a dtype of another width for each


@pytest.fixture(scope="module")
def binding(sm):
    return importlib.import_module("snappy_jl_amd._binding")


def _module(suffix):
    return importlib.import_module("snappy_jl_amd" + suffix)


def _tensors(spec):
    """[(name, position, type, elements, need or None)] of a case's tensor arguments."""
    out = []
    for word in spec.split():
        name, position, kind, size = word.split(":")
        size, _, need = size.partition("!")
        out.append((name, int(position), kind, int(size), int(need) if need else None))
    return out


def _make(kind, n, device, dtype=None, strided=False):
    """A tensor of n elements of the case type `kind` (a dict of them for a structure)."""
    import torch
    if kind in FIELDS:
        return {key: _make(k, n, device, dtype, strided) for key, k in FIELDS[kind]}
    t = torch.zeros(2 * n if strided else n, dtype=getattr(torch, dtype or TORCH[kind]), device=device)
    return t[::2] if strided else t


def _arguments(spec, device):
    return {name: _make(kind, size, device) for name, _, kind, size, _ in _tensors(spec)}


def _swapped(args, name, kind, value, field):
    """args with the tensor `name` (its array `field` for a structure) replaced by value."""
    out = dict(args)
    out[name] = dict(args[name], **{field: value}) if kind in FIELDS else value
    return out


def _places(spec):
    """Every tensor of a case, a structure's arrays one by one: (name, position, structure or type,
    field or None, element type, elements, need)."""
    for name, position, kind, size, need in _tensors(spec):
        for field, k in FIELDS.get(kind, [(None, kind)]):
            yield name, position, kind, field, k, size, need


def _named(message, cname, position, field):
    return message.startswith("%s argument %d%s:" % (cname, position, ", field %s" % field if field else ""))


# ---- the checker alone -------------------------------------------------------------------------------

DTYPES = ("uint8", "int8", "int16", "int32", "int64", "uint16", "uint32", "uint64", "bool", "float32")
TAKEN = {"b": {"uint8"}, "w": {"int32", "uint32"}, "d": {"int64", "uint64"}, "t": {"int32"}}  # the issue's list
# (shape of the tensor handed over, need) -> the verdict; need None: the table ties the array to no count
SHAPES = [
    ("0-D", None, ValueError), ("2-D", None, ValueError), ("strided", None, ValueError), ("offset slice", None, None),
    ("offset slice", 5, None), ("offset slice", 6, ValueError), ("no elements", None, None), ("no elements", 0, None),
    ("no elements", 1, ValueError), ("2-D of no elements", None, ValueError), ("one strided element", 1, None),
    (2, 3, ValueError), (3, 3, None), (4, 3, None), (2, 4, ValueError), (3, 4, ValueError), (4, 4, None), (5, 4, None),
]


def _shaped(shape, dtype):
    import torch
    base = torch.zeros(16, dtype=dtype)
    if isinstance(shape, int):
        return base[:shape]
    return {"0-D": lambda: base[0], "2-D": lambda: base.reshape(4, 4), "strided": lambda: base[::2],
            "offset slice": lambda: base[11:], "no elements": lambda: base[:0], "2-D of no elements": lambda: base[:0].reshape(0, 4),
            "one strided element": lambda: base[3:5:2]}[shape]()


def test_the_checker_against_a_pinned_list(binding):
    import torch
    for letter, taken in TAKEN.items():
        for name in DTYPES:
            t = torch.zeros(4, dtype=getattr(torch, name))
            if name in taken:
                binding.judge("f", 3, None, letter, 4, t)
            else:
                with pytest.raises(TypeError) as e:
                    binding.judge("f", 3, None, letter, 4, t)
                assert str(e.value).startswith("f argument 3: expected") and "torch." + name in str(e.value), (letter, name)
        for name in sorted(taken):
            for shape, need, verdict in SHAPES:
                t = _shaped(shape, getattr(torch, name))
                if verdict is None:
                    binding.judge("f", 3, "ulen", letter, need, t)
                else:
                    with pytest.raises(verdict) as e:
                        binding.judge("f", 3, "ulen", letter, need, t)
                    assert str(e.value).startswith("f argument 3, field ulen: expected"), (letter, name, shape, need)
        # what is no tensor: None, an address and a byref() object pass as they are; anything else is refused
        for a in (None, 0, 0x7F0000000000, ctypes.byref(ctypes.c_int())):
            binding.judge("f", 3, None, letter, 4, a)
        for a in ([0, 1, 2, 3], np.zeros(4, np.uint8), 1.5, b"abcd"):
            with pytest.raises(TypeError) as e:
                binding.judge("f", 3, None, letter, 4, a)
            assert type(a).__name__ in str(e.value)
    # the 16 bytes of an smf_summary: uint8[16] or int64[2] (uint64[2])
    for name, n, verdict in (("uint8", 16, None), ("uint8", 15, ValueError), ("int64", 2, None), ("uint64", 2, None),
                             ("int64", 1, ValueError), ("int32", 4, TypeError), ("uint8", 32, None)):
        t = torch.zeros(n, dtype=getattr(torch, name))
        if verdict is None:
            binding.judge("f", 5, None, "r", None, t)
        else:
            with pytest.raises(verdict):
                binding.judge("f", 5, None, "r", None, t)


@pytest.mark.parametrize("n", [0, 3])
def test_the_marks_against_n_and_n_plus_one(binding, n):
    """smf_chunk_offsets_device: d_ulen has nchunks entries, d_chunk_off nchunks + 1."""
    import torch
    i32, i64 = (lambda k: torch.zeros(k, dtype=torch.int32)), (lambda k: torch.zeros(k, dtype=torch.int64))
    for k_ulen, k_off, verdict in ((n, n + 1, None), (n + 1, n + 2, None), (n, n, "argument 3"), (n - 1, n + 1, "argument 1"),
                                   (n - 1, n, "argument 1")):
        if k_ulen < 0:
            continue
        args = (i32(k_ulen), n, i64(k_off))
        if verdict is None:
            found = binding.check_arguments("smf_chunk_offsets_device", args)
            assert [(k, f) for k, f, _ in found] == [(1, None), (3, None)] and found[0][2] is args[0] and found[1][2] is args[2]
        else:
            with pytest.raises(ValueError) as e:
                binding.check_arguments("smf_chunk_offsets_device", args)
            assert str(e.value).startswith("smf_chunk_offsets_device %s: expected at least" % verdict)


def test_every_tensor_pointer_has_a_case(binding):
    """CASES names every tensor position of the tables, and ties exactly the arrays that the tables tie."""
    cases = {c[2]: c for c in CASES}
    names = {n for t in binding.TABLES for n in t if n.endswith("_device")}
    assert len(CASES) == len(cases) == 36 and set(cases) == names
    for cname, (_, _, _, spec, _) in cases.items():
        plan = {k: (letter, mark) for k, letter, mark in binding.tensor_plan(cname)}
        mine = {position: (kind, need) for _, position, kind, _, need in _tensors(spec)}
        assert sorted(plan) == sorted(mine), cname
        for k, (letter, mark) in plan.items():
            assert (mark is not None or letter == "r") == (mine[k][1] is not None), (cname, k)


# ---- every wrapper, on CPU tensors ------------------------------------------------------------------

def test_sweep_of_every_device_wrapper(binding, monkeypatch):
    reached = []
    checker = binding.check_arguments
    monkeypatch.setattr(binding, "check_arguments", lambda name, args: (reached.append(name), checker(name, args))[1])
    modules = [_module(m) for m in MODULES]
    # "No library loaded, no context made": other tests of a session may have loaded libraries and made
    # contexts before this one, so the sweep starts from _lib = None (put back afterwards) and holds
    # _ctx against what it was, instead of asking for an empty _ctx; alone, that is the same thing.
    before = [dict(getattr(m, "_ctx", {})) for m in modules]
    for m in modules:
        if hasattr(m, "_lib"):
            monkeypatch.setattr(m, "_lib", None)
    swaps = 0
    for suffix, wrapper, cname, spec, others in CASES:
        call = getattr(_module(suffix), wrapper)
        good = _arguments(spec, "cpu")
        with pytest.raises(TypeError) as e:  # the set is what checks 1 to 3 take: check 4 refuses its first tensor
            call(**good, **others)
        first = next(_places(spec))
        assert _named(str(e.value), cname, first[1], first[3]) and "expected a CUDA tensor" in str(e.value), cname
        for name, position, kind, field, k, size, need in _places(spec):
            trials = [(TypeError, _make(k, size, "cpu", dtype=WRONG[k])), (ValueError, _make(k, size, "cpu", strided=True))]
            if need:
                trials.append((ValueError, _make(k, need - 1, "cpu")))
            elif need == 0:  # its length is the call's count: what is no tensor must not count as an empty batch
                trials += [(TypeError, [0] * size), (TypeError, np.zeros(size, np.int32))]
                with pytest.raises(TypeError) as e:  # (never optional; the wrapper itself refuses None there)
                    call(**_swapped(good, name, kind, None, field), **others)
                assert "gives a count or a capacity of the call is None" in str(e.value)
            for error, value in trials:
                with pytest.raises(error) as e:
                    call(**_swapped(good, name, kind, value, field), **others)
                assert _named(str(e.value), cname, position, field), (cname, name, field, str(e.value))
                assert "CUDA" not in str(e.value)
                swaps += 1
    # 314 tensors and structure arrays, a wrong dtype and a strided view each; 147 an element short; a list and a
    # numpy array at each of the 31 arguments that give a count
    assert swaps == 2 * 314 + 147 + 2 * 31
    assert set(reached) == {n for t in binding.TABLES for n in t if n.endswith("_device")} and len(set(reached)) == 36
    for m, ctx in zip(modules, before):  # nothing was loaded, no context made
        assert getattr(m, "_lib", None) is None and getattr(m, "_ctx", {}) == ctx


def test_the_five_failures_of_the_issue(sm):
    """What reached a kernel unnoticed: each now raises, naming the C function and the position."""
    import torch
    good = _arguments(CASES[0][3], "cpu")

    def refused(error, text, **swap):
        with pytest.raises(error) as e:
            sm.compress_batch_device(**dict(good, **swap))
        assert str(e.value).startswith("sm_compress_batch_device argument %s" % text), str(e.value)

    refused(TypeError, "3: expected a tensor of dtype int32 or uint32 (uint32_t), given a torch.int64 tensor",
            d_in_len=torch.tensor([4, 4]))
    refused(TypeError, "2: expected a tensor of dtype int64 or uint64 (uint64_t), given a torch.int32 tensor",
            d_in_off=torch.tensor([0, 4], dtype=torch.int32))
    refused(ValueError, "1: expected a one-dimensional contiguous tensor, given shape (8,) with strides (2,)",
            d_in=torch.zeros(16, dtype=torch.uint8)[::2])
    refused(TypeError, "1: expected a CUDA tensor")  # a CPU tensor
    refused(ValueError, "7: expected at least 2 elements, given 1", d_out_len=torch.zeros(1, dtype=torch.int32))
    refused(TypeError, "3: expected a tensor of dtype int32 or uint32 (uint32_t), given list", d_in_len=[4, 4])
    # place_fragments_device turns tensors of no fragments into null pointers: only tensors
    place = _arguments(CASES[4][3], "cpu")
    for d_len, given in (([3, 5], "list"), ((3, 5), "tuple"), (np.array([3, 5], np.int32), "ndarray")):
        with pytest.raises(TypeError) as e:
            sm.place_fragments_device(**dict(place, d_len=d_len), total_len=8, write_header=True)
        assert str(e.value) == ("sm_place_fragments_device argument 3: expected a tensor of dtype int32 or uint32 "
                                "(uint32_t), given " + given)


class OnGpu:
    """A tensor as the checks see one, on cuda:`index`, in the style of test_stream_and_device_rules' Tensor."""

    def __init__(self, index, dtype, n, address=None):
        import torch
        self.device = torch.device("cuda", index)
        self.dtype, self.shape, self.n, self.address = getattr(torch, dtype), (n,), n, address

    def dim(self):
        return 1

    def numel(self):
        return self.n

    def is_contiguous(self):
        return True

    def stride(self):
        return (1,)

    def data_ptr(self):
        assert self.address is not None, "a refused call took a tensor's address"
        return self.address


def test_a_tensor_on_another_gpu(sm, monkeypatch):
    monkeypatch.setattr(sm, "_lib", None)
    spec = CASES[0][3]
    on0 = {name: OnGpu(0, TORCH[kind], size) for name, _, kind, size, _ in _tensors(spec)}
    for name, position, kind, size, _ in _tensors(spec):
        args = dict(on0, **{name: OnGpu(1, TORCH[kind], size)})
        with pytest.raises(ValueError) as e:
            sm.compress_batch_device(**args, device=0)
        assert str(e.value) == ("sm_compress_batch_device argument %d: expected a tensor on the call's device cuda:0, "
                                "given one on cuda:1" % position)
    # the call's device is d_in's where none is given
    with pytest.raises(ValueError) as e:
        sm.compress_batch_device(**dict(on0, d_in=OnGpu(1, "uint8", 8)))
    assert str(e.value).startswith("sm_compress_batch_device argument 2: expected a tensor on the call's device cuda:1")
    # checks 1 to 3 come first
    with pytest.raises(TypeError) as e:
        sm.compress_batch_device(**dict(on0, d_in=OnGpu(1, "uint8", 8), d_out_len=OnGpu(0, "int64", 2)), device=0)
    assert str(e.value).startswith("sm_compress_batch_device argument 7: expected a tensor of dtype")
    assert sm._lib is None


def test_a_further_context_of_a_device(sm, recorder):
    """device=(name, d, k) names a further context of device d (context_cache): the tensors belong on cuda:d."""
    rec = recorder(sm)
    spec = CASES[0][3]
    on0 = {name: OnGpu(0, TORCH[kind], size, 0x1000 * position) for name, position, kind, size, _ in _tensors(spec)}
    with pytest.raises(ValueError) as e:
        sm.compress_batch_device(**on0, device=("own", 1, 0), stream=0x99)
    assert str(e.value).startswith("sm_compress_batch_device argument 1: expected a tensor on the call's device cuda:1")
    assert rec.calls == []
    sm.compress_batch_device(**on0, device=("own", 0, 0), stream=0x99)
    assert [c[0] for c in rec.calls] == ["sm_ctx_create", "sm_compress_batch_device"] and rec.calls[0][1] == (0,)
    args = rec.calls[1][1]
    assert [a.value if isinstance(a, ctypes.c_void_p) else a for a in args] == \
           [0xC0DE, 0x1000, 0x2000, 0x3000, 2, 0x5000, 0x6000, 0x7000, 1, 0x99]


# ---- on the GPU: the library replaced by a recorder ---------------------------------------------------

class Recorder:
    """In a module's _lib: every function of the library records its call and returns 0 (a
    *_ctx_create a made-up handle)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def function(*args):
            self.calls.append((name, args))
            return 0xC0DE if name.endswith("_ctx_create") else 0
        return function


@pytest.fixture
def recorder(monkeypatch):
    """install(module) -> the Recorder now in module._lib; the contexts it handed out are dropped afterwards."""
    kept = []

    def install(module):
        rec = Recorder()
        kept.append((module._ctx, dict(module._ctx)))
        monkeypatch.setattr(module, "_lib", rec)
        return rec

    yield install
    for cache, before in kept:
        cache.clear()
        cache.update(before)


def _gpu_cases():
    return [c for c in CASES if c[2] in ONE_PER_LIBRARY]


@gpu
@pytest.mark.parametrize("case", range(8))
def test_rejections_never_reach_the_library(gpu_available, recorder, case):
    suffix, wrapper, cname, spec, others = _gpu_cases()[case]
    module = _module(suffix)
    rec, call = recorder(module), getattr(module, wrapper)
    good = _arguments(spec, "cuda:0")
    places = list(_places(spec))
    lengths = next(p for p in places if p[4] == "i")   # an int64 tensor where uint32_t / int32_t is read
    offsets = next(p for p in places if p[4] == "q")   # an int32 tensor where uint64_t is read
    trials = [(TypeError, places[-1], _make(places[-1][4], places[-1][5], "cpu")),
              (TypeError, lengths, _make("i", lengths[5], "cuda:0", dtype="int64")),
              (TypeError, offsets, _make("q", offsets[5], "cuda:0", dtype="int32")),
              (ValueError, places[0], _make(places[0][4], places[0][5], "cuda:0", strided=True))]
    for error, (name, position, kind, field, k, size, need), value in trials:
        with pytest.raises(error) as e:
            call(**_swapped(good, name, kind, value, field), **others)
        assert _named(str(e.value), cname, position, field), str(e.value)
    assert rec.calls == []  # no context was asked for, no function called


@gpu
@pytest.mark.parametrize("case", range(8))
def test_marshalling(gpu_available, recorder, case):
    import torch
    suffix, wrapper, cname, spec, others = _gpu_cases()[case]
    module = _module(suffix)
    rec = recorder(module)
    good = _arguments(spec, "cuda:0")
    side = torch.cuda.Stream(device=0)
    for stream, handle in ((None, torch.cuda.current_stream(0).cuda_stream), (side, side.cuda_stream), (0x5EED, 0x5EED)):
        del rec.calls[:]
        getattr(module, wrapper)(**good, **others, stream=stream)
        calls = [c for c in rec.calls if not c[0].endswith("_ctx_create")]
        assert [c[0] for c in calls] == [cname]
        args = calls[0][1]
        want = dict(ONE_PER_LIBRARY[cname])
        for name, position, kind, _, _ in _tensors(spec):
            if kind in FIELDS:
                struct = args[position]._obj
                assert [(key, getattr(struct, key)) for key, _ in FIELDS[kind]] == \
                       [(key, good[name][key].data_ptr()) for key, _ in FIELDS[kind]]
            else:
                assert isinstance(args[position], ctypes.c_void_p) and args[position].value == good[name].data_ptr(), name
            want[position] = None
        assert len(args) == len(want) + 2 and isinstance(args[-1], ctypes.c_void_p) and (args[-1].value or 0) == handle
        assert args[0] in (0xC0DE, module._ctx.get(0))
        for position, value in want.items():
            assert value is None or (type(args[position]) is int and args[position] == value), (cname, position)


# ---- on the GPU: what the checks must let through, with the real library -----------------------------

GUARD = 0x5A
BLOCKS = (1, 300, 65536)


def _inputs():
    rng = np.random.default_rng(11)
    text = (b"device wrappers take what the C contract takes. " * 1400)[:BLOCKS[2]]
    noisy = bytearray(text)
    for i in rng.integers(0, len(noisy), 2000):
        noisy[i] = int(rng.integers(0, 256))
    return [b"x", bytes(rng.integers(0, 4, BLOCKS[1], dtype=np.uint8)), bytes(noisy)]


class Arrays:
    """Tensors for an acceptance case, made in one of four ways: 'signed' (int32 / int64, exact
    length), 'unsigned' (uint32 / uint64), 'slice' (an offset slice of a larger tensor with three
    guard entries before and behind) and 'longer' (one guard entry more than needed).  status: an
    int32_t array, int32 in every case; exact: the array whose length the wrapper takes as the count
    of the call, never longer."""

    def __init__(self, how):
        self.how, self.made = how, []

    def __call__(self, values, bits, status=False, exact=False):
        import torch
        unsigned = {8: np.uint8, 32: np.uint32, 64: np.uint64}[bits]
        signed = {8: np.uint8, 32: np.int32, 64: np.int64}[bits]
        values = np.asarray(values, dtype=unsigned)
        guard = np.full(3, GUARD * 0x0101010101010101 % (1 << bits), dtype=unsigned)
        n = values.size
        if self.how == "slice":
            whole = np.concatenate([guard, values, guard])
        elif self.how == "longer" and not exact:
            whole = np.concatenate([values, guard[:1]])
        else:
            whole = values
        whole = torch.from_numpy(whole.copy() if self.how == "unsigned" and not status else whole.view(signed).copy()).to("cuda:0")
        t = whole[3:3 + n] if self.how == "slice" else whole
        self.made.append((whole, t, n, guard))
        return t

    def guards_intact(self):
        for whole, t, n, guard in self.made:
            host = whole.cpu().numpy().view(guard.dtype)
            outside = np.concatenate([host[:3], host[3 + n:]]) if self.how == "slice" else host[n:]
            if outside.size and not (outside == guard[0]).all():
                return False
        return True


def _host(t, n, dtype):
    return t.cpu().numpy().view(dtype)[:n]


def _round_trip(compress, uncompress, oracle, how, len_bits):
    """The inputs through compress(...) and uncompress(...) with every array made by Arrays(how):
    the streams decode to the inputs under the oracle, the device decode gives them back, the
    guards stand."""
    import torch
    datas = _inputs()
    assert [len(d) for d in datas] == list(BLOCKS)
    n, lens = len(datas), [len(d) for d in datas]
    rooms = [(32 + k + k // 6 + 15) // 16 * 16 for k in lens]
    A = Arrays(how)
    d_in = A(np.frombuffer(b"".join(datas), np.uint8), 8)
    d_in_off, d_in_len = A(np.cumsum([0] + lens[:-1]), 64), A(lens, 32, exact=True)
    c_off = np.cumsum([0] + rooms[:-1])
    d_c, d_c_off, d_c_len = A(np.full(sum(rooms), GUARD, np.uint8), 8), A(c_off, 64), A([7] * n, 32)
    d_c_st = A([0xFFFFFFFF] * n, 32, status=True) if len_bits else None
    compress(d_in, d_in_off, d_in_len, d_c, d_c_off, d_c_len, d_c_st)
    torch.cuda.synchronize()
    c_len = _host(d_c_len, n, np.uint32).tolist()
    packed = _host(d_c, sum(rooms), np.uint8)
    streams = [packed[o:o + k].tobytes() for o, k in zip(c_off.tolist(), c_len)]
    assert [oracle.uncompress(s) for s in streams] == datas
    assert d_c_st is None or _host(d_c_st, n, np.int32).tolist() == [0] * n
    for o, k, room in zip(c_off.tolist(), c_len, rooms):
        assert (packed[o + k:o + room] == GUARD).all()
    d_out, d_out_off = A(np.full(sum(lens), GUARD, np.uint8), 8), A(np.cumsum([0] + lens[:-1]), 64)
    d_out_cap, d_out_len, d_st = A(lens, 32), A([7] * n, 32), A([0xFFFFFFFF] * n, 32, status=True)
    uncompress(d_c, d_c_off, d_c_len[:n], d_out, d_out_off, d_out_cap, d_out_len, d_st)
    torch.cuda.synchronize()
    assert _host(d_st, n, np.int32).tolist() == [0] * n and _host(d_out_len, n, np.uint32).tolist() == lens
    assert _host(d_out, sum(lens), np.uint8).tobytes() == b"".join(datas)
    assert A.guards_intact()


HOWS = ("signed", "unsigned", "slice", "longer")


@gpu
@pytest.mark.parametrize("how", HOWS)
def test_batch_calls_take_what_the_contract_takes(sm, oracle, gpu_available, how):
    _round_trip(lambda i, io, il, o, oo, ol, st: sm.compress_batch_device(i, io, il, o, oo, ol, mode="fast"),
                sm.uncompress_batch_device, oracle, how, 0)


@gpu
@pytest.mark.parametrize("how", HOWS)
def test_stream_calls_take_what_the_contract_takes(sm, oracle, gpu_available, how):
    mu = _module(".multi")
    _round_trip(lambda i, io, il, o, oo, ol, st: mu.compress_streams_device(i, io, il, 3, o, oo, ol, st, mode="fast"),
                lambda i, io, il, o, oo, cap, ol, st: mu.uncompress_streams_device(i, io, il, 0, o, oo, cap, ol, st),
                oracle, how, 32)


@gpu
def test_an_empty_batch_and_no_fragments(sm, gpu_available):
    import torch
    mu = _module(".multi")
    e8, e32, e64 = (torch.zeros(0, dtype=d, device="cuda:0") for d in (torch.uint8, torch.int32, torch.int64))
    guard = torch.full((64,), GUARD, dtype=torch.uint8, device="cuda:0")
    sm.compress_batch_device(e8, e64, e32, guard[8:40], e64, e32)
    sm.uncompress_batch_device(e8, e64, e32, guard[8:40], e64, e32, e32, e32)
    mu.compress_streams_device(e8, e64, e32, 0, guard[8:40], e64, e32, e32)
    mu.uncompress_streams_device(e8, e64, e32, 0, guard[8:40], e64, e32, e32, e32)
    torch.cuda.synchronize()
    assert (guard.cpu().numpy() == GUARD).all()
    # no fragments with a header: varint(300) alone, and a status the call leaves at 0
    d_st = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    d_local = torch.full((1,), -1, dtype=torch.int64, device="cuda:0")
    sm.place_fragments_device(e8, e64, e32, e64, guard[8:40], 300, True, d_local_off=d_local[:0], d_status=d_st)
    torch.cuda.synchronize()
    want = np.full(64, GUARD, np.uint8)
    want[8:10] = (0xAC, 0x02)
    assert (guard.cpu().numpy() == want).all() and int(d_st.item()) == 0 and int(d_local.item()) == -1
