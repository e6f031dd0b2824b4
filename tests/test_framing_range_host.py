"""CPU checks of the framing library's seek index and range plan (include/snappy_mi355x_framing.h):
smf_chunk_offsets, smf_range_chunk_count and smf_range_plan -- the rules the device plan runs --
against the plain-Python reference of tests/framing_range_ref.py, over a good index of a hand-built
foreign stream and over hostile ones; the stand-alone sanitizer driver; the exported symbols.  No
kernel is launched here."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import framing_range_ref as RR
import framing_ref as R
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "snappy_mi355x_framing.h")
FRAMING_SRC = os.path.join(ROOT, "snappy.jl_amd", "csrc", "framing")
ARG = RR.SM_ERR_ARGUMENT


@pytest.fixture(scope="module")
def fr(sm):
    return importlib.import_module("snappy_jl_amd.framing")


@pytest.fixture(scope="module")
def foreign(fr, oracle):
    stream, data = RR.foreign_stream(oracle)
    assert R.decode(stream, oracle) == data and len(data) == 37
    return stream, data, fr.seek_index_framed(stream)


@pytest.mark.parametrize("nchunks", [0, 1, 257])
def test_chunk_offsets(fr, nchunks):
    rng = np.random.default_rng(nchunks)
    ulen = rng.integers(0, 65537, nchunks, dtype=np.uint32)
    ulen[::5] = 0
    ulen[1::7] = 65536
    off = fr.chunk_offsets(ulen)
    assert off.dtype == np.uint64 and off.tolist() == [0] + np.cumsum(ulen.astype(np.uint64)).tolist()
    assert fr.lib().smf_chunk_offsets(None, 1, None) == ARG


@pytest.mark.parametrize("lo,length,want", [(0, 0, 0), (0, 1, 1), (65535, 1, 1), (65535, 2, 2), (65536, 65536, 1),
                                            (1, 131072, 3)])
def test_range_chunk_count(fr, lo, length, want):
    assert fr.range_chunk_count(lo, length) == want


def test_seek_index_of_foreign_stream(fr, foreign):
    stream, data, index = foreign
    ref = R.walk(stream)
    assert index.ulen.tolist() == [0, 1, 3, 0, 16, 17, 0] == [c[4] for c in ref]
    assert index.chunk_off.tolist() == RR.chunk_offsets(ref) and index.total_length == 37
    assert list(zip(*(a.tolist() for a in index.arrays().values()))) == ref
    # index_framed is what it was: five arrays, no chunk_off
    assert sorted(fr.index_framed(stream)[1]) == ["crc", "pay_len", "pay_off", "type", "ulen"]


def test_range_plan_exhaustive(fr, foreign):
    stream, data, index = foreign
    ranges = RR.all_ranges(37)
    rc, first, count, status, total = fr.range_plan(index, len(stream), ranges)
    offsets = index.chunk_off.tolist()
    want = [RR.plan(offsets, lo, n) for lo, n in ranges]
    assert rc == 0 and total == sum(w[1] for w in want)
    got = list(zip(first.tolist(), count.tolist(), status.tolist()))
    bad = [(r, g, w) for r, g, w in zip(ranges, got, want) if g != w]
    assert not bad, bad[:5]
    # the slots hold every touched chunk, and only empty chunks besides
    for (lo, n), (f, k, st) in zip(ranges, got):
        t = RR.touched(offsets, lo, n) if st == 0 else []
        assert all(f <= c < f + k for c in t) and (not t or (t[0], t[-1]) == (f, f + k - 1))
    # one below the true total: too many
    rc, _, _, status, total2 = fr.range_plan(index, len(stream), ranges, max_range_chunks=total - 1)
    assert rc == R.SM_BUFFER_TOO_SMALL and total2 == total and set(status.tolist()) == {ARG}
    assert fr.range_plan(index, len(stream), ranges, max_range_chunks=total)[0] == 0


def test_range_plan_hostile_index(fr, foreign):
    stream, data, index = foreign
    ranges = RR.all_ranges(37) + [(5, (1 << 64) - 2), ((1 << 64) - 1, 1), (37, 0)]
    for name, bad, victim in RR.hostile_indexes(fr.FramedIndex, index, len(stream)):
        rc, first, count, status, total = fr.range_plan(bad, len(stream), ranges)
        assert rc == 0, name
        assert all(k == 0 or f + k <= bad.nchunks for f, k in zip(first.tolist(), count.tolist())), name
        want = [RR.hostile_want(index, int(bad.chunk_off[-1]), victim, lo, n) for lo, n in ranges]
        wrong = [(r, g, w) for r, g, w in zip(ranges, status.tolist(), want) if g != w]
        assert not wrong, (name, wrong[:5])


def test_range_plan_only_empty_chunks(fr):
    stream = R.IDENTIFIER + R.raw_chunk(b"") + R.chunk(0x00, R.crc_field(b"") + b"\x00") + R.raw_chunk(b"")
    index = fr.seek_index_framed(stream)
    assert index.nchunks == 3 and index.total_length == 0
    rc, first, count, status, total = fr.range_plan(index, len(stream), [(0, 0), (0, 1), (1, 0)])
    assert (rc, total, count.tolist(), status.tolist()) == (0, 0, [0, 0, 0], [0, ARG, 0])


def test_host_check_under_sanitizers():
    r = subprocess.run(["make", "-C", FRAMING_SRC, "host_check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "smf_host_check ok" in r.stdout


def test_new_symbols_export_with_c_linkage(fr):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = {m.group(1) for m in re.finditer(r"\b(smf_[a-z0-9_]+)\s*\(", src)}
    new = {"smf_chunk_offsets", "smf_range_chunk_count", "smf_range_plan", "smf_range_scratch_bytes",
           "smf_chunk_offsets_device", "smf_compress_indexed_device", "smf_uncompress_ranges_device",
           "smf_uncompress_range"}
    assert new <= declared and set(fr.RANGE_ABI_SYMBOLS) == new
    out = subprocess.run(["nm", "-D", "--defined-only", fr.library_path()], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for s in sorted(new):
        assert s in exported, s
        assert hasattr(fr.lib(), s), s
    assert fr.lib().smf_range_scratch_bytes(3, 7) >= 6 * 65536
