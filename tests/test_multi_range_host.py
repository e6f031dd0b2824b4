"""CPU checks of the ranged decode of indexed raw streams (include/snappy_mi355x_multi_range.h,
exported by snappy.jl_amd/libsnappy_mi355x_multi.so): the ABI and its prototype table, the Python
statement of the rules (tests/multi_range_ref.py) against known answers worked out by hand, the
host run of the plan (smm_range_plan, the code the kernels compile) against that statement over
the length ladder and over seeded hostile indexes and ranges, the sanitizer driver, and the
argument checks that need no device.  No kernel is launched here."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

from prototype_types import assert_device_elements

import multi_range_ref as M
import multi_ref as R
from conftest import ROOT

HEADER = "snappy_mi355x_multi_range.h"
CSRC = os.path.join(ROOT, "snappy.jl_amd", "csrc", "multi")
SCALARS = {"size_t": ctypes.c_size_t, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "int": ctypes.c_int,
           "int32_t": ctypes.c_int32, "sm_status": ctypes.c_int32}
NAMES = {"smm_range_fragment_count", "smm_range_scratch_bytes", "smm_range_plan", "smm_uncompress_ranges_device",
         "smm_uncompress_ranges"}


@pytest.fixture(scope="module")
def mu(sm):
    return importlib.import_module("snappy_jl_amd.multi")


@pytest.fixture(scope="module")
def binding(sm):
    return importlib.import_module("snappy_jl_amd._binding")


def _declarations(header):
    """{name: (return type, [parameter types])} of include/<header>, comments and preprocessor lines
    stripped."""
    with open(os.path.join(ROOT, "include", header)) as f:
        src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S))
    src = re.sub(r"^[ \t]*#[^\n]*$", "", src, flags=re.M)
    out = {}
    for m in re.finditer(r"([\w\s\*]+?)\b(smm_\w+)\s*\(([^;{]*?)\)\s*;", src, re.S):
        params = m.group(3).strip()
        types = [] if params in ("", "void") else [re.sub(r"\w+$", "", p.strip()) for p in params.split(",")]
        assert m.group(2) not in out
        out[m.group(2)] = (m.group(1), types)
    return out


def _class(ctype):
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


def test_table_matches_the_header(mu, binding):
    declared, table = _declarations(HEADER), binding.MULTI_RANGE
    assert set(declared) == set(table) == set(mu.RANGE_ABI_SYMBOLS) == NAMES
    assert mu.RANGE_ABI_SYMBOLS == tuple(table) and not set(table) & set(binding.MULTI)
    for name, (ret, params) in declared.items():
        restype, argtypes = binding.prototype(table[name])
        assert len(argtypes) == len(params), name
        assert _class(restype) == _c_class(ret), name
        for k, (t, p) in enumerate(zip(argtypes, params)):
            assert t is not None and _class(t) == _c_class(p), "%s: argument %d (%s)" % (name, k, p.strip())
    assert assert_device_elements(binding, declared, table) == 14  # the pointer parameters of the *_device functions, ctx and stream among them


def test_symbols_export_from_the_multi_library(mu):
    out = subprocess.run(["nm", "-D", "--defined-only", mu.library_path()], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for s in sorted(NAMES):
        assert s in exported, s
        assert hasattr(mu.lib(), s), s
    # the multi header keeps its own 15 functions, and its table is theirs alone
    assert len(_declarations("snappy_mi355x_multi.h")) == 15 == len(mu.MULTI_ABI_SYMBOLS)
    assert not NAMES & set(_declarations("snappy_mi355x_multi.h"))


def test_sources_are_in_the_version_hash():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=(.*)$", mk, re.M).group(1).split()
    hdrs = re.search(r"^HDRS\s*=(.*)$", mk, re.M).group(1).split()
    assert "smm_range.hip" in srcs and "smm_range.h" in hdrs and "../../../include/" + HEADER in hdrs


# ---- the Python statement of the rules, against answers worked out by hand ---------------------

def test_model_known_answers(mu):
    for count in (M.range_fragment_count, mu.range_fragment_count):
        assert count(65535, 2) == 2
        assert count(65536, 65536) == 1
        assert count(0xFFFFFFFF, 2) == 2
        for lo in (0, 1, 65535, 65536, 12345678, 0xFFFFFFFF):
            assert count(lo, 0) == 0
        assert count(0, 1) == 1 and count(0, 65536) == 1 and count(0, 65537) == 2 and count(0, 0xFFFFFFFF) == 65536
    # a 3-fragment stream with D = 131073, range (1, 131072): fragments 0 and 2 go to edge slots,
    # fragment 1 goes direct at output offset 65535
    assert M.touched(1, 131072) == (0, 3)
    assert M.fragment_place(131073, 0, 3, 1, 131072) == ("edge", 1, 65535, 0)
    assert M.fragment_place(131073, 1, 3, 1, 131072) == ("direct", 65535)
    assert M.fragment_place(131073, 2, 3, 1, 131072) == ("edge", 0, 1, 131071)
    assert M.fragment_length(131073, 2, 3) == 1 and M.fragment_length(131073, 1, 3) == 65536
    # the stream's short last fragment goes to an edge slot even where the range holds all of it:
    # D = 131073, range (65536, 65537) is fragment 1 direct at 0 and the one byte of fragment 2 by
    # an edge slot to output offset 65536 -- one edge slot, not none
    assert M.touched(65536, 65537) == (1, 2)
    assert M.fragment_place(131073, 1, 3, 65536, 65537) == ("direct", 0)
    assert M.fragment_place(131073, 2, 3, 65536, 65537) == ("edge", 0, 1, 65536)
    # a last fragment of a whole 64 KiB is direct: D = 131072 has no edge slot for (0, 131072) or (65536, 65536)
    assert M.fragment_place(131072, 0, 2, 0, 131072) == ("direct", 0)
    assert M.fragment_place(131072, 1, 2, 0, 131072) == ("direct", 65536)
    assert M.fragment_place(131072, 1, 2, 65536, 65536) == ("direct", 0)
    assert M.fragment_place(131072, 1, 2, 65537, 65535) == ("edge", 1, 65535, 0)
    # entries: the first is the varint's length, then strictly increasing, the end inside the stream
    assert M.entry_check([3, 100, 200], 0, 3, 300) == (3, 100) and M.entry_check([3, 100, 200], 2, 3, 300) == (200, 300)
    assert M.entry_check([2, 100, 200], 0, 3, 300) is None and M.entry_check([3, 100, 100], 1, 3, 300) is None
    assert M.entry_check([3, 100, 300], 2, 3, 300) is None and M.entry_check([3, 100, 300], 1, 3, 300) == (100, 300)
    assert M.entry_check([3, 0, 0], 1, 3, 300) is None and M.entry_check([3, 250, 200], 0, 3, 300) == (3, 250)


def test_scratch_bytes(mu):
    K = 65536
    assert 2 * K <= mu.range_scratch_bytes(1, 17) < 3 * K      # two edge slots for one range
    assert 3 * K <= mu.range_scratch_bytes(10, 3) < 4 * K      # never more edge slots than slots
    assert mu.range_scratch_bytes(4, 9) > mu.range_scratch_bytes(4, 8) > mu.range_scratch_bytes(3, 8)


# ---- smm_range_plan against the model ----------------------------------------------------------------

def _ladder(oracle):
    datas = [R.sources()[k % 5][3 * k:3 * k + n] for k, n in enumerate(R.LADDER)]
    idx = [R.cpu_index(d, oracle) for d in datas]
    strs = [i[0] for i in idx]
    first = np.concatenate([[0], np.cumsum([len(i[1]) for i in idx])]).astype(np.uint32)
    pos = np.array([p for i in idx for p in i[1]], np.uint32)
    return datas, strs, first, pos


def ladder_ranges(lengths):
    """Every (stream, lo, len) of the ladder: lo in {0, 1, 65535, 65536, 65537, D - 1, D}, len in
    {0, 1, 2, 65535, 65536, 65537, D - lo}, the ones past D included."""
    out = []
    for s, D in enumerate(lengths):
        for lo in sorted({0, 1, 65535, 65536, 65537, max(D - 1, 0), D}):
            for ln in sorted({0, 1, 2, 65535, 65536, 65537, max(D - lo, 0)}):
                out.append((s, lo, ln))
    return out


def _same(mu, strs, first, pos, ranges, bound=None, nentries=None):
    ne = len(pos) if nentries is None else nentries
    want = M.plan(strs, first, pos, ne, ranges, bound)
    f, c, st, total = mu.range_plan(strs, (first, pos), ranges, max_range_fragments=bound, nentries=ne)
    assert (f.tolist(), c.tolist(), st.tolist(), total) == (want[1], want[2], want[3], want[4])
    return want


def test_plan_on_the_ladder(mu, oracle):
    datas, strs, first, pos = _ladder(oracle)
    assert first.tolist() == [0, 0, 1, 2, 3, 5, 7, 10, 14]
    ranges = ladder_ranges(R.LADDER) + [(0, 0xFFFFFFFF, 2), (7, 0xFFFFFFFF, 2), (8, 0, 1), (8, 0, 0), (7, 1, 0xFFFFFFFF)]
    rc, f, c, st, total = _same(mu, strs, first, pos, ranges)
    assert rc == 0
    for (s, lo, ln), f_, c_, st_ in zip(ranges, f, c, st):  # ... and the model says what the contract says
        inside = s < 8 and lo + ln <= R.LADDER[s]
        assert st_ == (0 if ln == 0 or inside else 33), (s, lo, ln)
        assert c_ == (M.range_fragment_count(lo, ln) if inside else 0)
        assert f_ == (lo >> 16 if inside and ln else 0)
    assert total == sum(c) > len(ranges) // 2


def test_bound_one_below_the_need(mu, oracle):
    datas, strs, first, pos = _ladder(oracle)
    ranges = [(7, 1, 196612), (4, 65536, 1), (2, 5, 0), (6, 65535, 2)]
    need = 4 + 1 + 0 + 2
    assert _same(mu, strs, first, pos, ranges, bound=need)[3] == [0, 0, 0, 0]
    rc, f, c, st, total = _same(mu, strs, first, pos, ranges, bound=need - 1)
    assert rc == M.SM_BUFFER_TOO_SMALL and st == [33] * 4 and total == need and c == [4, 1, 0, 2]
    # the C call itself returns SM_BUFFER_TOO_SMALL
    buf, in_off, in_len = importlib.import_module("snappy_jl_amd").pack_blocks(strs)
    r = np.array(ranges, np.uint32)
    cols = [np.ascontiguousarray(r[:, k]) for k in range(3)]
    status = np.zeros(4, np.int32)
    total = ctypes.c_uint64(0)
    rc = mu.lib().smm_range_plan(buf.ctypes.data, in_off.ctypes.data, in_len.ctypes.data, len(strs), first.ctypes.data,
                                 pos.ctypes.data, pos.size, cols[0].ctypes.data, cols[1].ctypes.data, cols[2].ctypes.data,
                                 4, need - 1, None, None, status.ctypes.data, ctypes.byref(total))
    assert rc == 2 and status.tolist() == [33] * 4 and total.value == need


def test_plan_fuzz_of_hostile_indexes_and_ranges(mu, oracle):
    """2,000 seeded cases: one mutation of the index (a frag_first word decreasing or past nentries;
    a position zero, decreasing, equal to its neighbour, at or past n, a first position that is not
    hv; a count off by one; a stream whose header is broken) and four ranges drawn from the edges
    (len 0, the stream's end, past D, past 2^32, a stream number that is nstreams), sometimes with the
    bound one below the need."""
    datas = [R.sources()[k][5:5 + n] for k, n in ((0, 196613), (3, 300), (1, 65537), (4, 0), (2, 131073))]
    idx = [R.cpu_index(d, oracle) for d in datas]
    strs0 = [i[0] for i in idx]
    first0 = np.concatenate([[0], np.cumsum([len(i[1]) for i in idx])]).astype(np.uint32)
    pos0 = np.array([p for i in idx for p in i[1]], np.uint32)
    rng = np.random.default_rng(20260)
    seen_status, seen_rc, kinds = set(), set(), set()
    for trial in range(2000):
        strs, f2, p2 = list(strs0), first0.copy(), pos0.copy()
        ne = None
        kind = trial % 9
        s = int(rng.choice([0, 2, 4]))  # a stream with entries to break
        e0, e1 = int(f2[s]), int(f2[s + 1])
        if kind == 0:    # frag_first: decreasing
            f2[s], f2[s + 1] = f2[s + 1], f2[s]
        elif kind == 1:  # frag_first: past nentries
            if rng.random() < 0.5:
                f2[s + 1] = int(rng.choice([p2.size + 1, 0xFFFFFFFF]))
            else:
                ne = e1 - 1
        elif kind == 2:  # a position: zero
            p2[int(rng.integers(e0, e1))] = 0
        elif kind == 3:  # a position: decreasing, or equal to its neighbour
            k = int(rng.integers(e0, e1))
            p2[k] = (int(p2[k - 1]) - int(rng.integers(0, 2))) % (1 << 32) if k > e0 else int(p2[min(k + 1, e1 - 1)])
        elif kind == 4:  # a position: at or past n
            p2[int(rng.integers(e0, e1))] = len(strs[s]) + int(rng.choice([0, 1, 0x7FFFFFFF]))
        elif kind == 5:  # the first position is not hv
            p2[e0] = int(p2[e0]) + int(rng.choice([-1, 1]))
        elif kind == 6:  # a count off by one: an entry inserted or removed, the later streams shifted
            if rng.random() < 0.5:
                p2 = np.insert(p2, e1, p2[e1 - 1] + 1)
                f2[s + 1:] += 1
            else:
                p2 = np.delete(p2, e1 - 1)
                f2[s + 1:] -= 1
        elif kind == 7:  # a header that does not parse
            strs[s] = bytes([0x85, 0x80])
        ranges = []
        for _ in range(4):
            rs = int(rng.choice([s, s, int(rng.integers(0, 6))]))
            D = len(datas[rs]) if rs < 5 else 70000
            lo = int(rng.choice([0, 1, 65535, 65536, 65537, 131072, max(D - 1, 0), D, 0xFFFFFFFF, int(rng.integers(0, D + 1))]))
            ln = int(rng.choice([0, 1, 2, 65536, 65537, max(D - min(lo, D), 0), D + 1, 0xFFFFFFFF, int(rng.integers(0, D + 2))]))
            ranges.append((rs, lo, ln))
        want = _same(mu, strs, f2, p2, ranges, nentries=ne)
        if want[4] and trial % 5 == 0:
            below = _same(mu, strs, f2, p2, ranges, bound=want[4] - 1, nentries=ne)
            assert below[0] == 2 and set(below[3]) == {33}
            seen_rc.add(below[0])
        seen_rc.add(want[0])
        for (rs, lo, ln), c_, st_ in zip(ranges, want[2], want[3]):
            seen_status.add((st_, c_ > 0, ln == 0))
            if st_ == 33 and c_ > 0:
                kinds.add(kind)  # an entry failed behind a stream-level rule that passed
    assert seen_rc == {0, 2}
    assert {(0, True, False), (0, False, True), (33, False, False), (33, True, False)} <= seen_status, seen_status
    assert kinds >= {2, 3, 4, 5}, kinds


def test_host_check_runs_clean(tmp_path):
    """make host_check with the range plan's structural cases, under ASan and UBSan as a stand-alone
    program."""
    src = open(os.path.join(CSRC, "smm_host_check.cpp")).read()
    assert "smm_range_plan" in src and "range_cases();" in src
    r = subprocess.run(["make", "-C", CSRC, "host_check", "OBJ=%s" % tmp_path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "smm_host_check: ok" in r.stdout


def test_null_arguments_need_no_device(mu):
    L = mu.lib()
    one = np.zeros(4, np.uint64)
    p = one.ctypes.data
    # a NULL ctx is refused before anything else, by both calls
    assert L.smm_uncompress_ranges_device(None, p, p, p, 1, p, p, 1, p, p, p, 1, 1, p, p, p, p, None) == 33
    assert L.smm_uncompress_ranges(None, p, p, p, 1, p, p, p, p, p, 1, p, p, p, p) == 33
    assert L.smm_uncompress_ranges_device(None, p, p, p, 1, p, p, 1, p, p, p, 0, 0, p, p, p, p, None) == 33
    assert L.smm_range_plan(None, p, p, 1, p, p, 1, p, p, p, 1, 1, None, None, None, None) == 33
    assert L.smm_range_plan(None, None, None, 0, None, None, 0, None, None, None, 0, 0, None, None, None, None) == 0
