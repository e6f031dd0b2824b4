"""CPU checks of the index build of the multi-stream library (include/snappy_mi355x_multi.h:
smm_index_host, the rule smm_index_device runs on the GPU): the exported symbols, the sanitizer
driver, and smm_index_host against the plain-Python statement of the rule (tests/multi_index_ref.py)
on oracle-compressed streams, foreign streams, the 400 mutation cases and hand-built streams.  No
kernel is launched here."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import multi_index_ref as X
import multi_ref as R
from conftest import ROOT

CSRC = os.path.join(ROOT, "snappy.jl_amd", "csrc", "multi")
INDEX_SYMBOLS = ("smm_index_host", "smm_index_device", "smm_index")


@pytest.fixture(scope="module")
def mu(sm):
    return importlib.import_module("snappy_jl_amd.multi")


def host_call(mu, strs, caps, lens, m, guard=X.GUARDS):
    """smm_index_host over buffers of exactly the documented sizes (and `guard` sentinels behind
    frag_pos): (frag_first, frag_pos, built, status)."""
    buf, off, ln = X.pack(strs, lens)
    n = len(strs)
    cap = None if caps is None else np.array(caps, np.uint32)
    first = np.full(n + 1, X.GUARD, np.uint32)
    pos = np.full(m + guard, X.GUARD, np.uint32)
    built = np.full(max(n, 1), 7, np.uint8)
    status = np.full(max(n, 1), -1, np.int32)
    keep = np.zeros(1, np.uint8)
    st = mu.lib().smm_index_host(buf.ctypes.data if buf.size else keep.ctypes.data, off.ctypes.data, ln.ctypes.data, n, m,
                                 cap.ctypes.data if cap is not None else None, first.ctypes.data, pos.ctypes.data,
                                 built.ctypes.data, status.ctypes.data)
    assert st == 0
    return first, pos, built[:n], status[:n]


def same(got, want, what):
    for g, w, name in zip(got, want, ("frag_first", "frag_pos", "built", "status")):
        assert np.array_equal(g, w), (what, name, np.nonzero(np.asarray(g) != np.asarray(w))[0][:8])


def test_symbols_export_with_c_linkage(mu):
    out = subprocess.run(["nm", "-D", "--defined-only", mu.library_path()], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for s in INDEX_SYMBOLS:
        assert s in exported and s in mu.MULTI_ABI_SYMBOLS and hasattr(mu.lib(), s), s
    header = open(os.path.join(ROOT, "include", "snappy_mi355x_multi.h")).read()
    plan = open(os.path.join(CSRC, "smm_plan.h")).read()
    assert "kIndexStage = %d;" % mu.INDEX_STAGE in plan and "smm_index_device(" in header
    assert mu.INDEX_STAGE >= 1024  # "multi-KiB": the sweep of test_multi_index_gpu.py stays inside a stream


def test_host_check_runs_clean(tmp_path):
    r = subprocess.run(["make", "-C", CSRC, "host_check", "OBJ=%s" % tmp_path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "smm_host_check: ok" in r.stdout
    assert "smm_index_host" in open(os.path.join(CSRC, "smm_host_check.cpp")).read()


def test_scratch_never_shrinks(mu):
    """smm_scratch_bytes covers the index call's arrays without dropping below what the compress and
    decode layouts needed before it existed (the values that formula gave at these shapes)."""
    before = ((0, 0, 304), (1, 0, 432), (1, 1, 77056), (16, 28, 2146016), (640, 10240, 784238384), (100000, 0, 9200304),
              (400, 1078, 82590368))
    for n, m, floor in before:
        assert mu.scratch_bytes(n, m) >= floor, (n, m)
        assert mu.scratch_bytes(n, m) >= 256 + 8 * n + 16  # the index call: two words per stream and one more


@pytest.mark.parametrize("name", ["ladder", "cpu_index", "foreign", "fuzz", "hand", "hand_no_cap", "hand_overflow"])
def test_host_equals_the_model(mu, oracle, name):
    strs, caps, lens, m = X.groups(oracle)[name]
    same(host_call(mu, strs, caps, lens, m), X.group_model(oracle, name), name)


def test_cpu_index_positions(mu, oracle):
    """On the oracle's streams the built positions are the oracle's own fragment offsets."""
    cases = X.cpu_index_cases(oracle)
    strs, caps, lens, m = X.groups(oracle)["cpu_index"]
    first, pos, built, status = host_call(mu, strs, caps, lens, m)
    want = [p for c in cases for p in c[1]]
    assert [len(c[1]) for c in cases] == [2, 2, 3, 4] and built.tolist() == [1, 1, 1, 1]
    assert pos[:len(want)].tolist() == want and first.tolist() == [0, 2, 4, 7, 11]
    assert pos[len(want):].tolist() == [X.GUARD] * (m + X.GUARDS - len(want))  # a looser bound: untouched behind


def test_ladder_built_is_length_above_a_block(mu, oracle):
    first, pos, built, status = X.group_model(oracle, "ladder")
    datas = R.ladder_datas()
    assert built.tolist() == [int(len(d) > 65536) for d in datas]
    assert first.tolist() == np.concatenate([[0], np.cumsum([R.frag_count(len(d)) for d in datas])]).tolist()


def test_foreign_streams_are_not_built(mu, oracle):
    strs, caps, lens, m = X.groups(oracle)["foreign"]
    first, pos, built, status = host_call(mu, strs, caps, lens, m)
    assert built.tolist() == [0, 0] and m == 6 and pos[:m].tolist() == [0] * 6 and status.tolist() == [0, 0]


def test_fuzz_set_is_two_sided(oracle):
    built = X.group_model(oracle, "fuzz")[2]
    assert len(built) == 400 and int(built.sum()) >= 100 and int((built == 0).sum()) >= 100, int(built.sum())


def test_hand_cases_one_by_one(mu, oracle):
    """Each hand-built stream alone, with the expectations that can be read off its construction."""
    K = 65536
    expect = {
        "ends-on-65536": ([3, 3 + 3 + K], 1), "short-tags-end-on-65536": ([3, 3 + 1092 * 61 + 17], 1),
        "short-literal-straddles": ([0, 0], 0), "literal-70000-crosses": ([0, 0], 0),
        "literal-65536-lands-then-more": ([3, 3 + 3 + K, 3 + 2 * (3 + K)], 1), "literal-crosses-two": ([0, 0, 0], 0),
        "cut-before-last": ([0, 0, 0], 0), "boundary-at-end": ([0, 0], 0), "stray-byte-at-boundary": ([3, 3 + 3 + K], 1),
        "header-only": ([0, 0], 0), "declares-more-than-cap": ([], 0), "declares-the-cap": ([3, 3 + 3 + K], 1),
        "varint-unfinished": ([], 0), "varint-fifth-byte": ([], 0), "empty": ([], 0), "error-mark": ([], 0),
        "declares-0": ([], 0), "declares-1": ([1], 0), "declares-65536": ([3], 0),
    }
    for name, s, cap, ln in X.hand_cases():
        caps, lens = (None if cap is None else [cap]), (None if ln is None else [ln])
        m = X.exact_bound([s], caps, lens) + 1
        got = host_call(mu, [s], caps, lens, m)
        same(got, X.model([s], caps, m, lens, X.GUARDS), name)
        if name in expect:
            want, b = expect[name]
            assert got[1][:len(want)].tolist() == want and int(got[0][1]) == len(want) and got[2].tolist() == [b], name
        assert got[1][int(got[0][1]):].tolist() == [X.GUARD] * (m + X.GUARDS - int(got[0][1])), name


def test_overflow_by_one(mu, oracle):
    strs, caps, lens, m = X.groups(oracle)["hand_overflow"]
    first, pos, built, status = host_call(mu, strs, caps, lens, m)
    assert first.tolist() == [0] * (len(strs) + 1) and not built.any()
    assert status.tolist() == [X.SM_ERR_ARGUMENT] * len(strs) and pos.tolist() == [X.GUARD] * (m + X.GUARDS)
    assert not host_call(mu, strs, caps, lens, m + 1)[3].any()


def test_python_wrapper(mu, oracle):
    strs, caps, lens, m = X.groups(oracle)["cpu_index"]
    first, pos, built = mu.index_streams_host(strs)
    assert pos.tolist() == [p for c in X.cpu_index_cases(oracle) for p in c[1]] and built.tolist() == [1] * 4
    assert mu.index_bound(strs) == int(first[-1]) == 11
    assert mu.index_check(strs, (first, pos), [len(oracle.uncompress(s)) for s in strs]).tolist() == [1] * 4
    with pytest.raises(mu.SnappyError):
        mu.index_streams_host(strs, max_fragments=10)
    f0, p0, b0 = mu.index_streams_host([])
    assert f0.tolist() == [0] and p0.size == 0 and b0.size == 0
