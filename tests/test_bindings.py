"""snappy.jl_amd/_binding.py on the CPU: the prototype tables against the three headers, the batch
layout helpers against pinned results, and the lazy loaders with their context caches."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

from prototype_types import assert_device_elements

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = {"size_t": ctypes.c_size_t, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "int": ctypes.c_int,
           "int32_t": ctypes.c_int32, "sm_status": ctypes.c_int32}


@pytest.fixture(scope="module")
def fr(sm):
    return importlib.import_module("snappy_jl_amd.framing")


@pytest.fixture(scope="module")
def mu(sm):
    return importlib.import_module("snappy_jl_amd.multi")


@pytest.fixture(scope="module")
def binding(sm):
    return importlib.import_module("snappy_jl_amd._binding")


def _declarations(header):
    """{name: (return type, [parameter types])} of include/<header>, comments stripped, the way
    test_julia_shim._header_arity matches `name(params);`."""
    with open(os.path.join(ROOT, "include", header)) as f:
        src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S))
    out = {}
    for m in re.finditer(r"([\w\s\*]+?)\b(sm[fm]?_\w+)\s*\(([^;{]*?)\)\s*;", src, re.S):
        params = m.group(3).strip()
        types = [] if params in ("", "void") else [re.sub(r"\w+$", "", p.strip()) for p in params.split(",")]
        assert m.group(2) not in out
        out[m.group(2)] = (m.group(1), types)
    return out


def _class(ctype):
    """('pointer',) or (bytes, signed) of a ctypes type; None for void."""
    if ctype is None:
        return None
    if ctype in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(ctype, ctypes._Pointer):
        return ("pointer",)
    return (ctypes.sizeof(ctype), ctype(-1).value < 0)


def _c_class(decl):
    words = decl.replace("const", " ").split()
    if "*" in decl:
        return ("pointer",)
    if words == ["void"]:
        return None
    assert len(words) == 1 and words[0] in SCALARS, decl
    return _class(SCALARS[words[0]])


DEVICE_POINTERS = {"RAW": 58, "FRAMING": 81, "MULTI": 33}  # the pointer parameters of the *_device functions, ctx and stream among them


@pytest.mark.parametrize("header, table, count", [("snappy_mi355x.h", "RAW", 36), ("snappy_mi355x_framing.h", "FRAMING", 33),
                                                  ("snappy_mi355x_multi.h", "MULTI", 15)])
def test_tables_match_the_headers(binding, header, table, count):
    device_pointers = DEVICE_POINTERS[table]
    declared, table = _declarations(header), getattr(binding, table)
    assert len(declared) == count and set(declared) == set(table)
    for name, (ret, params) in declared.items():
        restype, argtypes = binding.prototype(table[name])
        assert len(argtypes) == len(params), name
        assert _class(restype) == _c_class(ret), name
        for k, (t, p) in enumerate(zip(argtypes, params)):
            assert t is not None and _class(t) == _c_class(p), "%s: argument %d (%s)" % (name, k, p.strip())
    assert assert_device_elements(binding, declared, table) == device_pointers


def test_every_function_is_in_one_table(binding, sm, fr, mu):
    groups = [binding.RAW, binding.FRAMING_BASE, binding.FRAMING_RANGE, binding.FRAMING_STREAMS, binding.MULTI]
    assert sum(len(g) for g in groups) == len(set().union(*groups)) == 84
    assert sm.ABI_SYMBOLS == tuple(binding.RAW) and mu.MULTI_ABI_SYMBOLS == tuple(binding.MULTI)
    assert fr.FRAMING_ABI_SYMBOLS == tuple(binding.FRAMING)
    assert len(binding.FRAMING) == len(binding.FRAMING_BASE) + 8 + 7
    assert set(fr.RANGE_ABI_SYMBOLS) == {
        "smf_chunk_offsets", "smf_range_chunk_count", "smf_range_plan", "smf_range_scratch_bytes",
        "smf_chunk_offsets_device", "smf_compress_indexed_device", "smf_uncompress_ranges_device", "smf_uncompress_range"}
    assert set(fr.STREAMS_ABI_SYMBOLS) == {
        "smf_max_data_chunks", "smf_streams_plan", "smf_streams_scratch_bytes", "smf_uncompress_streams_device",
        "smf_compress_streams_device", "smf_compress_streams", "smf_uncompress_streams"}
    assert fr.INDEX_KEYS == tuple(name for name, _ in fr.Chunks._fields_) == ("type", "pay_off", "pay_len", "crc", "ulen")


# ---- the batch layout, pinned to what the functions gave before they shared _binding.py ----------

MIX = [b"ab", bytearray(b"cde"), memoryview(b"f"), np.array([7, 8], np.uint8)]
LAYOUTS = [  # (input, buffer, offsets, lengths); _lay_out's buffer is one zero byte where there is no data
    ([], [], [], []),
    ([b""], [], [0], [0]),
    ([b"", b"a", b""], [97], [0, 0, 1], [0, 1, 0]),
    (MIX, [97, 98, 99, 100, 101, 102, 7, 8], [0, 2, 5, 6], [2, 3, 1, 2]),
]


def _same(arr, dtype, values):
    return arr.dtype == np.dtype(dtype) and arr.ndim == 1 and arr.tolist() == values


@pytest.mark.parametrize("case", range(len(LAYOUTS)))
def test_pack_blocks_and_lay_out(sm, fr, case):
    datas, buf, offs, lens = LAYOUTS[case]
    b, o, n = sm.pack_blocks(datas)
    assert _same(b, np.uint8, buf) and _same(o, np.uint64, offs) and _same(n, np.uint32, lens)
    b, o, n = fr._lay_out(datas)
    assert _same(b, np.uint8, buf or [0]) and _same(o, np.uint64, offs) and _same(n, np.uint64, lens)


def test_lay_out_views_other_dtypes_as_bytes(fr):
    b, o, n = fr._lay_out([np.array([1, 258], np.uint16), b"z"])
    assert _same(b, np.uint8, [1, 0, 2, 1, 122]) and _same(o, np.uint64, [0, 4]) and _same(n, np.uint64, [4, 1])


def test_slot_offsets(sm):
    offs, caps = sm.slot_offsets(np.array([0, 1, 6, 65535, 65536], np.uint32))
    assert _same(offs, np.uint64, [0, 32, 80, 128, 76624]) and _same(caps, np.uint64, [32, 48, 48, 76496, 76496])


def test_frag_first_of(mu):
    assert _same(mu.frag_first_of([0, 1, 65536, 65537, 2**31 - 1, 2**31]), np.uint32, [0, 0, 1, 2, 4, 32772, 32772])
    assert _same(mu.frag_first_of([]), np.uint32, [0])


def test_exclusive_scan(binding):
    assert _same(binding.exclusive_scan(np.zeros(0, np.uint32)), np.uint64, [])
    assert _same(binding.exclusive_scan(np.zeros(0, np.uint32), np.int64, total=True), np.int64, [0])
    assert _same(binding.exclusive_scan(np.array([5], np.uint32)), np.uint64, [0])
    assert _same(binding.exclusive_scan([5], np.uint32, total=True), np.uint32, [0, 5])
    big = binding.exclusive_scan(np.array([0xFFFFFFFF, 0xFFFFFFFF, 1], np.uint32), total=True)  # (no uint32 carry)
    assert _same(big, np.uint64, [0, 0xFFFFFFFF, 0x1FFFFFFFE, 0x1FFFFFFFF])


def test_collect(binding):
    out = np.frombuffer(b"abcdefgh", np.uint8)
    offs, lens = np.array([0, 2, 5, 8], np.uint64), np.array([2, 3, 0], np.uint32)
    assert binding.collect(out, offs, lens) == [b"ab", b"cde", b""]
    assert binding.collect(out, offs, lens, np.array([0, 17, 0], np.int32)) == [b"ab", None, b""]
    assert binding.collect(out, offs[:0], lens[:0], []) == []


# ---- the loaders and the context caches -----------------------------------------------------------

def test_stream_and_device_rules(binding):
    class Stream:
        cuda_stream = 0x1234

    class Tensor:
        class device:
            index = 3

    assert binding.stream_handle(Stream(), 0) == 0x1234 and binding.stream_handle(0x99, 0) == 0x99
    assert binding.device_of(Tensor(), None) == 3 and binding.device_of(Tensor(), 1) == 1


def test_importing_loads_no_library():
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); from conftest import load_package; import importlib; "
            "mods = [load_package(), importlib.import_module('snappy_jl_amd.framing'), "
            "importlib.import_module('snappy_jl_amd.multi')]; "
            "assert all(m._lib is None and m._ctx == {} for m in mods); "
            "assert 'libsnappy_mi355x' not in open('/proc/self/maps').read()" % os.path.join(ROOT, "tests"))
    subprocess.run([sys.executable, "-c", code], check=True)


def test_sharded_contexts_need_a_device(sm):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is usable here")
    with pytest.raises(sm.SnappyError) as e:
        sm.contexts([0, 0])
    assert e.value.code == 32 and str(e.value) == "no usable HIP device 0 for snappy_mi355x"
    assert not sm._ctx


@pytest.mark.parametrize("module, name", [("", "libsnappy_mi355x.so"), (".framing", "libsnappy_mi355x_framing.so"),
                                          (".multi", "libsnappy_mi355x_multi.so")])
def test_not_built_message(sm, monkeypatch, tmp_path, module, name):
    mod = importlib.import_module("snappy_jl_amd" + module)
    monkeypatch.setattr(mod, "_lib", None)
    monkeypatch.setattr(mod, "LIB_PATH", str(tmp_path / name))
    with pytest.raises(OSError) as e:
        mod.lib()
    assert str(e.value) == name + " not built (run __graft_entry__.build())"
    assert mod._lib is None
