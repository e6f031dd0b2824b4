"""CPU checks of the framing library's batched stream calls (include/snappy_mi355x_framing.h):
smf_streams_plan -- the decode plan the device runs -- against the per-stream model of
tests/framing_streams_ref.py over every structural case laid back to back, the chunk bound and the
scratch size helpers, the argument checks that need no device, and the exported symbols.  No kernel
is launched here."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import framing_ref as R
import framing_streams_ref as SR
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "snappy_mi355x_framing.h")
ARG = SR.SM_ERR_ARGUMENT
NEW = {"smf_max_data_chunks", "smf_streams_plan", "smf_streams_scratch_bytes", "smf_uncompress_streams_device",
       "smf_compress_streams_device", "smf_compress_streams", "smf_uncompress_streams"}


@pytest.fixture(scope="module")
def fr(sm):
    return importlib.import_module("snappy_jl_amd.framing")


@pytest.fixture(scope="module")
def batch():
    """Every structural case, as one batch: the streams and the room each needs."""
    streams = [c[1] for c in R.structural_cases()]
    caps = [sum(ch[4] for ch in SR.walk_prefix(s)[0]) for s in streams]
    return streams, caps


def check_plan(fr, streams, caps, max_chunks):
    rc, first, out_len, status, total = fr.streams_plan(streams, out_cap=caps, max_chunks=max_chunks)
    want = SR.plan(streams, caps, max_chunks)
    assert (rc, first.tolist(), out_len.tolist(), status.tolist(), total) == want
    return want


def test_model_agrees_with_the_structural_cases(batch):
    streams, caps = batch
    for (name, stream, status, nchunks), cap in zip(R.structural_cases(), caps):
        chunks, code = SR.walk_prefix(stream)
        assert (code, len(chunks)) == (status, nchunks), name


def test_plan_of_all_structural_cases_back_to_back(fr, batch):
    streams, caps = batch
    rc, first, out_len, status, total = check_plan(fr, streams, caps, 0x7FFFFFFF)
    assert rc == 0 and status == [c[2] for c in R.structural_cases()]
    assert total == sum(c[3] for c in R.structural_cases() if c[2] == 0) > 0
    # no room limit: the same plan
    got = fr.streams_plan(streams)
    assert (got[0], got[1].tolist(), got[2].tolist(), got[3].tolist(), got[4]) == (rc, first, out_len, status, total)


def test_plan_with_one_capacity_a_byte_short(fr, batch):
    streams, caps = batch
    full = SR.plan(streams, caps, 0x7FFFFFFF)
    victims = [s for s, c in enumerate(R.structural_cases()) if c[2] == 0 and caps[s] > 0]
    assert len(victims) >= 5
    for v in victims:
        short = list(caps)
        short[v] -= 1
        rc, first, out_len, status, total = check_plan(fr, streams, short, 0x7FFFFFFF)
        assert status[v] == R.SM_BUFFER_TOO_SMALL and out_len[v] == caps[v] and first[v + 1] == first[v]
        assert [s for i, s in enumerate(status) if i != v] == [s for i, s in enumerate(full[3]) if i != v]


def test_plan_with_max_chunks_one_below_the_total(fr, batch):
    streams, caps = batch
    total = SR.plan(streams, caps, 0x7FFFFFFF)[4]
    assert check_plan(fr, streams, caps, total)[0] == 0
    rc, first, out_len, status, total2 = check_plan(fr, streams, caps, total - 1)
    assert rc == R.SM_BUFFER_TOO_SMALL and total2 == total and set(status) == {ARG} and set(out_len) == {0}


def test_plan_without_streams(fr):
    rc, first, out_len, status, total = fr.streams_plan([])
    assert (rc, first.tolist(), out_len.size, status.size, total) == (0, [0], 0, 0, 0)
    total = ctypes.c_uint64(9)
    assert fr.lib().smf_streams_plan(None, None, None, 0, None, 0, None, None, None, ctypes.byref(total)) == 0
    assert total.value == 0


def test_plan_reads_no_neighbour(fr):
    """A stream cut in the middle of its last chunk with a whole stream directly behind it: the cut
    is seen, whatever the next bytes would complete."""
    whole = R.IDENTIFIER + R.raw_chunk(b"abc") + R.raw_chunk(b"defgh")
    for cut in range(1, len(R.raw_chunk(b"defgh"))):
        streams = [whole[:-cut], whole]
        rc, first, out_len, status, total = check_plan(fr, streams, [8, 8], 0x7FFFFFFF)
        assert status == [R.TRUNCATED, 0] and out_len == [3, 8] and first == [0, 0, 2]


@pytest.mark.parametrize("n,want", [(0, 0), (9, 0), (10, 0), (17, 0), (18, 1), (10 + 8 * 12345, 12345),
                                    (10 + 8 * 12345 + 7, 12345)])
def test_max_data_chunks(fr, n, want):
    assert fr.max_data_chunks(n) == want


def test_max_data_chunks_is_reached(fr):
    stream = R.IDENTIFIER + R.raw_chunk(b"") * 40
    assert len(R.walk(stream)) == 40 == fr.max_data_chunks(len(stream))


def test_scratch_bytes_is_monotone(fr):
    f = fr.lib().smf_streams_scratch_bytes
    sizes = (0, 1, 2, 3, 4, 5, 63, 64, 65, 1000, 10000)
    for a in sizes:
        for lo, hi in zip(sizes, sizes[1:]):
            assert f(a, lo) <= f(a, hi) and f(lo, a) <= f(hi, a)
    assert f(3, 7) > f(3, 6) and f(4, 7) >= f(3, 7) and f(0, 0) > 0
    assert f(1, 100) >= 100 * (32 + 65536 + 65536 // 6)  # the raw compressor's slots


def test_argument_errors_without_a_device(fr):
    """The checks that come before the ctx is looked at: a ctx that is no ctx must not be touched."""
    L = fr.lib()
    a = np.zeros(8, np.uint64)
    p = a.ctypes.data
    assert L.smf_uncompress_streams_device(None, p, p, p, 1, 1, p, p, p, p, p, None, None, None) == ARG
    assert L.smf_compress_streams_device(None, p, p, p, 1, 1, p, p, p, p, 1, None) == ARG
    assert L.smf_compress_streams(None, p, p, p, 1, p, p, p, p, 1) == ARG
    assert L.smf_uncompress_streams(None, p, p, p, 1, p, p, p, p, p) == ARG
    fake = np.zeros(4096, np.uint8).ctypes.data  # (never dereferenced: every call below fails first)
    assert L.smf_uncompress_streams_device(fake, p, p, p, 1, 1, p, p, p, p, p, p, None, None) == ARG
    assert L.smf_uncompress_streams_device(fake, p, p, p, 1, 1, p, p, p, p, p, None, p, None) == ARG
    assert L.smf_uncompress_streams_device(fake, p, p, p, 1 << 31, 1, p, p, p, p, p, None, None, None) == ARG
    assert L.smf_uncompress_streams_device(fake, p, p, p, 1, 1 << 31, p, p, p, p, p, None, None, None) == ARG
    for hole in range(8):  # d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap, d_out_len, d_status
        args = [p] * 8
        args[hole] = None
        assert L.smf_uncompress_streams_device(fake, args[0], args[1], args[2], 1, 1, *args[3:], None, None, None) == ARG
    for hole in range(7):
        args = [p] * 7
        args[hole] = None
        assert L.smf_compress_streams_device(fake, args[0], args[1], args[2], 1, 1, *args[3:], 1, None) == ARG
    assert L.smf_compress_streams_device(fake, p, p, p, 1, 1, p, p, p, p, 7, None) == ARG  # no such mode
    assert L.smf_compress_streams_device(fake, p, p, p, 1, 1 << 31, p, p, p, p, 1, None) == ARG
    assert L.smf_compress_streams(fake, p, p, p, 1, p, p, p, p, 7) == ARG
    assert L.smf_compress_streams(fake, p, None, p, 1, p, p, p, p, 1) == ARG
    assert L.smf_uncompress_streams(fake, p, p, None, 1, p, p, p, p, p) == ARG
    assert L.smf_streams_plan(None, p, p, 1 << 31, None, 0, None, None, None, None) == ARG
    assert L.smf_streams_plan(p, None, p, 1, None, 0, None, None, None, None) == ARG
    one = np.ones(1, np.uint64).ctypes.data
    assert L.smf_streams_plan(None, p, one, 1, None, 0, None, None, None, None) == ARG  # bytes, but no buffer
    # no streams: nothing to do, whatever the other arguments
    assert L.smf_uncompress_streams_device(fake, None, None, None, 0, 0, None, None, None, None, None, None, None, None) == 0
    assert L.smf_compress_streams_device(fake, None, None, None, 0, 0, None, None, None, None, 1, None) == 0


def test_new_symbols_export_with_c_linkage(fr):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = {m.group(1) for m in re.finditer(r"\b(smf_[a-z0-9_]+)\s*\(", src)}
    assert NEW <= declared and set(fr.STREAMS_ABI_SYMBOLS) == NEW <= set(fr.FRAMING_ABI_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", fr.library_path()], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for s in sorted(NEW):
        assert s in exported, s
        assert hasattr(fr.lib(), s), s
