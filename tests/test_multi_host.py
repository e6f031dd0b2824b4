"""CPU checks of the multi-stream companion library (include/snappy_mi355x_multi.h,
snappy.jl_amd/libsnappy_mi355x_multi.so): the exported ABI, the size helpers, the host run of the
index rules (the code the device plan compiles) against the Python statement of the contract
(tests/multi_ref.py), the sanitizer driver, and the spread of the decode model over the mutation
cases that tests/test_multi_gpu.py decodes.  No kernel is launched here."""
import glob
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import multi_ref as R
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "snappy_mi355x_multi.h")
CSRC = os.path.join(ROOT, "snappy.jl_amd", "csrc", "multi")


@pytest.fixture(scope="module")
def mu(sm):
    return importlib.import_module("snappy_jl_amd.multi")


def _declared(path, prefix):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return {m.group(1) for m in re.finditer(r"\b(%s_[a-z0-9_]+)\s*\(" % prefix, src)}


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return {l.split()[-1] for l in out.splitlines() if " T " in l}


def test_header_symbols_export_with_c_linkage(mu):
    syms = _declared(HEADER, "smm")
    assert syms and set(mu.MULTI_ABI_SYMBOLS) == syms
    assert not _declared(HEADER, "sm")  # no main-library declaration outside comments
    exported = _exported(mu.library_path())
    for s in sorted(syms):
        assert s in exported, s
        assert hasattr(mu.lib(), s), s
    assert not [s for s in exported if s.startswith("sm_") or s.startswith("smf_")]


def test_main_library_exports_unchanged(sm, mu):
    """The main library exports what its own header declares and nothing of this companion."""
    exported = _exported(sm.library_path())
    declared = _declared(os.path.join(ROOT, "include", "snappy_mi355x.h"), "sm")
    assert {s for s in exported if s.startswith("sm_")} == declared
    assert not [s for s in exported if s.startswith("smm_")]


def test_links_main_library_by_name(mu):
    out = subprocess.run(["readelf", "-d", mu.library_path()], capture_output=True, text=True).stdout
    assert "libsnappy_mi355x.so" in out and "$ORIGIN" in out
    assert "oracle" not in subprocess.run(["ldd", mu.library_path()], capture_output=True, text=True).stdout


def test_package_imports_without_the_multi_library(sm):
    src = open(os.path.join(ROOT, "snappy.jl_amd", "__init__.py")).read()
    assert "multi" not in src
    names = [os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*"))]
    for f in ("Makefile", "smm_api.hip", "smm_kernels.hip", "smm_plan.h", "smm_host.cpp", "smm_host_check.cpp"):
        assert f in names


@pytest.mark.parametrize("n", R.LADDER + (0x7FFFFFFF, 0x80000000, 0xFFFFFFFF))
def test_fragment_count(mu, n):
    assert mu.fragment_count(n) == -(-n // 65536) == R.frag_count(n)


def test_helpers(mu, sm):
    assert mu.version().startswith("snappy_mi355x_multi gfx950 ")
    assert mu.status_message(18) == sm.status_message(18) == "Could not decode varint32."
    pitch = (32 + 65536 + 65536 // 6 + 8 + 255) // 256 * 256
    assert pitch == 76544
    assert mu.scratch_bytes(4, 10) >= 10 * pitch and mu.scratch_bytes(4, 11) - mu.scratch_bytes(4, 10) >= pitch
    assert mu.frag_first_of(R.LADDER).tolist() == [0, 0, 1, 2, 3, 5, 7, 10, 14]
    assert mu.frag_first_of([5, 0x80000000, 70000]).tolist() == [0, 1, 1, 3]


def test_ctx_create_without_gpu_returns_null(mu):
    import torch
    if torch.cuda.is_available():
        assert mu.context(0)
        return
    assert not mu.lib().smm_ctx_create(0)
    assert mu.lib().smm_ctx_last_indexed(None) == -1
    with pytest.raises(mu.SnappyError):
        mu.compress_streams([b"abc"])


def test_host_check_runs_clean(tmp_path):
    """make host_check: the index rules over every structural case under ASan and UBSan, as a
    stand-alone program."""
    r = subprocess.run(["make", "-C", CSRC, "host_check", "OBJ=%s" % tmp_path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "smm_host_check: ok" in r.stdout


# ---- the host run of the index rules against the Python statement of the contract -------------------

def _base(oracle):
    datas = [R.sources()[k][5:5 + n] for k, n in ((0, 196613), (3, 300), (1, 65537), (4, 0), (2, 131073))]
    idx = [R.cpu_index(d, oracle) for d in datas]
    strs = [i[0] for i in idx]
    first = np.concatenate([[0], np.cumsum([len(i[1]) for i in idx])]).astype(np.uint32)
    pos = np.array([p for i in idx for p in i[1]], np.uint32)
    return datas, strs, first, pos


def _want(strs, caps, first, pos, m):
    if first is None or not R.first_ok(first, len(strs), m):
        return [0] * len(strs)
    return [1 if R.structural(s, c, [int(x) for x in pos[int(first[k]):int(first[k + 1])]]) else 0
            for k, (s, c) in enumerate(zip(strs, caps))]


def test_cpu_index_is_the_oracles_stream(oracle):
    datas, strs, first, pos = _base(oracle)
    assert first.tolist() == [0, 4, 5, 7, 7, 10]
    for d, s, k in zip(datas, strs, range(5)):
        assert oracle.uncompress(s) == d
        ent = [int(x) for x in pos[first[k]:first[k + 1]]] + [len(s)]
        for f in range(len(ent) - 1):  # every fragment alone is that 64 KiB of the data
            part = d[f * 65536:(f + 1) * 65536]
            assert oracle.uncompress(R.S.varint(len(part)) + s[ent[f]:ent[f + 1]]) == part


def test_index_check_matches_the_contract(mu, oracle):
    datas, strs, first, pos = _base(oracle)
    caps = [len(d) for d in datas]
    m = int(first[-1])
    assert mu.index_check(strs, (first, pos), caps).tolist() == [1, 0, 1, 0, 1] == _want(strs, caps, first, pos, m)
    assert mu.index_check(strs, None, caps).tolist() == [0] * 5
    rng = np.random.default_rng(17)
    seen = set()
    for trial in range(300):
        f2, p2, c2, m2 = first.copy(), pos.copy(), list(caps), m
        kind = trial % 6
        if kind == 0:  # one position moved: to a neighbour's value, past the end, by one
            k = int(rng.integers(0, p2.size))
            p2[k] = int(rng.choice([p2[k] + 1, max(int(p2[k]), 1) - 1, p2[(k + 1) % p2.size], 0xFFFFFFFF, 0,
                                    len(strs[0]), len(strs[0]) - 1]))
        elif kind == 1:  # one entry of frag_first moved
            k = int(rng.integers(0, f2.size))
            f2[k] = int(rng.choice([f2[k] + 1, max(int(f2[k]), 1) - 1, 0, 0xFFFFFFFF, m]))
        elif kind == 2:  # the bound
            m2 = int(rng.choice([m - 1, m, m + 3]))
            p2 = np.concatenate([p2, np.zeros(3, np.uint32)])[:max(m2, 1)]
        elif kind == 3:  # the room
            k = int(rng.integers(0, 5))
            c2[k] = int(rng.choice([c2[k] - 1, c2[k] + 1, 65536, 0])) % (1 << 32)
        elif kind == 4:  # a count off by one: an entry inserted or removed, the later streams shifted
            k = int(rng.choice([0, 2, 4]))
            if rng.random() < 0.5:
                p2 = np.insert(p2, int(f2[k + 1]), p2[int(f2[k + 1]) - 1] + 1)
                f2[k + 1:] += 1
            else:
                p2 = np.delete(p2, int(f2[k + 1]) - 1)
                f2[k + 1:] -= 1
            m2 = int(f2[-1])
        got = mu.index_check(strs, (f2, p2), c2, max_fragments=m2).tolist()
        assert got == _want(strs, c2, f2, p2, m2), (trial, kind)
        seen.add(tuple(got))
    # one mutation knocks out each indexed stream alone, all of them, or none
    assert seen >= {(1, 0, 1, 0, 1), (0, 0, 1, 0, 1), (1, 0, 0, 0, 1), (1, 0, 1, 0, 0), (0, 0, 0, 0, 0)}, seen


def test_fuzz_model_spread(oracle):
    """The decode model's statuses over the 400 mutation cases include OK and each decode error at
    least ten times, and both the indexed path and the fallback."""
    res = R.fuzz_model(oracle)
    st = np.array([r[0] for r in res])
    counts = {code: int((st == code).sum()) for code in (0, 17, 19, 20, 21)}
    assert len(res) == R.FUZZ_N == 400
    assert all(v >= 10 for v in counts.values()), counts
    idx = sum(1 for r in res if r[2])
    assert idx >= 10 and sum(1 for r in res if r[0] == 0 and not r[2]) >= 10, idx
    for (s, cap, pos), r in zip(R.fuzz_cases(oracle), res):
        assert r[0] != 0 or len(r[1]) <= cap
