"""CPU checks of the framing format's companion library (include/snappy_mi355x_framing.h,
snappy.jl_amd/libsnappy_mi355x_framing.so): the Python reference CRC against the known answers, the
size helper, the exported ABI, and the host chunk walker smf_index over hand-built streams
(tests/framing_ref.py).  No kernel is launched here."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import framing_ref as R
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "snappy_mi355x_framing.h")


@pytest.fixture(scope="module")
def fr(sm):
    return importlib.import_module("snappy_jl_amd.framing")


def declared_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1) for m in re.finditer(r"\b(smf_[a-z0-9_]+)\s*\(", src)}


@pytest.mark.parametrize("data,crc,masked", R.KNOWN_ANSWERS, ids=lambda v: None)
def test_reference_crc_known_answers(data, crc, masked):
    assert R.crc32c(data) == crc
    assert R.mask(crc) == masked


def test_host_crc_matches_reference(fr):
    for data, crc, masked in R.KNOWN_ANSWERS:
        assert fr.crc32c(data) == crc and fr.mask_crc(crc) == masked
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 4, 5, 63, 64, 65, 1000):
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert fr.crc32c(data) == R.crc32c(data)


def test_golden_framed_a():
    assert R.IDENTIFIER + R.raw_chunk(b"a") == R.GOLDEN_A


@pytest.mark.parametrize("n", [0, 1, 65535, 65536, 65537, 3 * 65536, 3 * 65536 + 1, 10 ** 9])
def test_max_framed_length(fr, n):
    assert fr.max_framed_length(n) == 10 + 8 * -(-n // 65536) + n == R.max_framed_length(n)


def test_header_symbols_export_with_c_linkage(fr):
    syms = declared_symbols()
    assert syms and set(fr.FRAMING_ABI_SYMBOLS) == syms
    out = subprocess.run(["nm", "-D", "--defined-only", fr.library_path()], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for s in sorted(syms):
        assert s in exported, s
        assert hasattr(fr.lib(), s), s
    # the companion's own prefix only: the main library's sm_ ABI is pinned elsewhere
    assert not [s for s in exported if s.startswith("sm_")]


def test_links_main_library_by_name_and_no_oracle(fr):
    out = subprocess.run(["readelf", "-d", fr.library_path()], capture_output=True, text=True).stdout
    assert "libsnappy_mi355x.so" in out and "$ORIGIN" in out
    assert "oracle" not in subprocess.run(["ldd", fr.library_path()], capture_output=True, text=True).stdout


def test_package_imports_without_the_framing_library(sm):
    # snappy.jl_amd/__init__.py neither imports framing.py nor names its library
    src = open(os.path.join(ROOT, "snappy.jl_amd", "__init__.py")).read()
    assert "framing" not in src


def test_status_messages(fr, sm):
    msgs = [fr.status_message(code) for code in range(R.NO_IDENTIFIER, R.CRC + 1)]
    assert len(set(msgs)) == 6 and all(m.startswith("Framed stream") for m in msgs)
    assert fr.status_message(18) == sm.status_message(18) == "Could not decode varint32."
    assert fr.version().startswith("snappy_mi355x_framing gfx950 ")


def test_ctx_create_without_gpu_returns_null(fr):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    assert not fr.lib().smf_ctx_create(0)
    with pytest.raises(fr.SnappyError):
        fr.compress_framed(b"abc")


@pytest.mark.parametrize("name,stream,status,nchunks", R.structural_cases(), ids=[c[0] for c in R.structural_cases()])
def test_index_structural(fr, name, stream, status, nchunks):
    s, arrays = fr.index_framed(stream, max_chunks=8)
    assert s.status == status
    assert s.nchunks == nchunks
    try:
        ref = R.walk(stream)
    except R.FramingRefError as e:
        assert e.code == status
    else:
        assert status == R.SM_OK and len(ref) == nchunks
        assert s.total_length == sum(c[4] for c in ref)
        got = list(zip(*(arrays[k][:nchunks].tolist() for k in ("type", "pay_off", "pay_len", "crc", "ulen"))))
        assert got == ref
    if status == R.SM_OK:
        assert fr.length_uncompressed_framed(stream) == s.total_length
    else:
        with pytest.raises(fr.SnappyError) as e:
            fr.length_uncompressed_framed(stream)
        assert e.value.code == status


def test_index_capacity_too_small(fr):
    a = R.raw_chunk(b"a")
    stream = R.IDENTIFIER + a + R.chunk(0xFE, b"pad") + R.raw_chunk(b"bc") + a
    s, arrays = fr.index_framed(stream, max_chunks=2)
    assert (s.status, s.nchunks, s.total_length) == (R.SM_BUFFER_TOO_SMALL, 3, 4)
    assert arrays["ulen"].tolist() == [1, 2]  # the entries that fit are filled
    s, arrays = fr.index_framed(stream)  # sized by a counting walk
    assert (s.status, s.nchunks) == (R.SM_OK, 3) and arrays["pay_off"].tolist() == [18, 19 + 7 + 8, 19 + 7 + 10 + 8]
    # a structural error wins over the capacity
    s, _ = fr.index_framed(stream + R.chunk(0x02, b""), max_chunks=1)
    assert (s.status, s.nchunks) == (R.RESERVED_CHUNK, 3)


def test_index_arguments(fr):
    s = fr.Summary()
    assert fr.lib().smf_index(None, 4, None, 0, ctypes.byref(s)) == 33
    assert fr.lib().smf_index(b"abcd", 4, None, 0, None) == 33


def test_python_decoder_reads_python_encoder(oracle):
    rng = np.random.default_rng(9)
    text = (b"the quick brown fox jumps over the lazy dog. " * 2000)[:70000]
    data = text + rng.integers(0, 256, 65536, dtype=np.uint8).tobytes() + text[:100]
    framed = R.encode(data, oracle)
    assert len(framed) <= R.max_framed_length(len(data))
    types = [c[0] for c in R.walk(framed)]
    assert 0 in types and 1 in types
    assert R.decode(framed, oracle) == data
    assert R.encode(b"", oracle) == R.IDENTIFIER and R.decode(R.IDENTIFIER, oracle) == b""
    assert R.encode(b"a", oracle) == R.GOLDEN_A
