"""The device batch calls' remainder rule: sm_compress_batch_device and sm_compress_fragments_device
parse the last nblk % grid blocks of a fast-mode batch in parts on their own workgroups when they
are at most half the grid, and must leave exactly the bytes and lengths of
the whole-block parse.

The expected bytes come from the same library in a fresh child process with SM_BATCH_PARTS=0 (the
whole-block kernel for every block); every stream must also decode to its input under the CPU
oracle.  Each of the two child processes (switch off, switch on) runs the one case list below once;
the tests compare case by case.

Cases (g = the device's compute-unit count, read from the device):
  A. nblk = 1, 3, g/2, g/2+1, g+1, g+16, 2g-1 blocks of 64 KiB: text windows, one random block (the
     screen's literal) and one constant block among the last three;
  B. a last block of 1, 1,023, 1,025 and 65,535 bytes (nblk 3, and g+3 once);
  C. slots whose offsets are no multiples of 16;
  D. no header: the fragment call, whole-stream table size;
  E. the fragment call with a total length that selects a smaller table (one short fragment);
  F. a 100-byte block (the blocks behind it start at odd addresses), a block that passes the screen
     but parses to more than one literal (the writer's fallback, which the gather repeats per
     block), and an empty block.
All in fast and dense mode: 19 cases each.  sm_ctx_last_batch_parts, recorded after every call,
shows that the calls with the rule on did parse their remainder in parts.  Four host threads
calling on the one context and stream must each get their own batch's bytes.  An oversize block's mark through the parts is test_fragments_device's
test_oversize_block_is_marked (4 blocks: all of them remainder blocks).
"""
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import streams
from conftest import load_package, read_testfile

BLOCK = 65536
MAXC = 76490  # sm_max_compressed_length(65536)
HASH_MUL = 0x1E35A7BD
MODES = ("fast", "dense")
NBLK = ("1", "3", "g/2", "g/2+1", "g+1", "g+16", "2g-1")


def nblk_of(name, g):
    return {"1": 1, "3": 3, "g/2": g // 2, "g/2+1": g // 2 + 1, "g+1": g + 1, "g+16": g + 16, "2g-1": 2 * g - 1,
            "5": 5, "g+3": g + 3}[name]


def rule(nblk, g):
    """The remainder rule in plain Python: (rem, parts)."""
    r = nblk % g
    if r == 0 or r > g // 2:
        return 0, 0
    p = 1
    while p < 16 and r * 2 * p <= g:
        p *= 2
    return r, p


@functools.lru_cache(maxsize=None)
def _raw_text():
    return read_testfile("lcet10.txt") + read_testfile("plrabn12.txt")


def text_block(i, n=BLOCK):
    raw = _raw_text()
    return raw[(7919 * i) % (len(raw) - BLOCK):][:n]


@functools.lru_cache(maxsize=None)
def random_block():
    return np.random.default_rng(0xBA7C4).integers(0, 256, BLOCK, dtype=np.uint8).tobytes()


def is_anchor(word):
    return ((word * HASH_MUL) & 0xFFFFFFFF) >> 26 == 0


@functools.lru_cache(maxsize=None)
def fallback_block():
    """Random bytes with one 6-byte string, built around an anchor word of the screen, at 30 places
    of the first 8 KiB: the screen counts 29 repeated anchors (8 make a block compressible) and
    hands the block to the parse, whose copies (at most 30 of 6 bytes) save less than the tags of
    64 super-chunks' literal runs cost -- the parse is longer than one literal of the block."""
    rng = np.random.default_rng(0xFA11)
    blk = bytearray(rng.integers(0, 256, BLOCK, dtype=np.uint8).tobytes())
    word = next(w for w in range(0x61626364, 0x71626364) if is_anchor(w))
    piece = word.to_bytes(4, "little") + b"\x5a\xa5"
    for k in range(30):
        at = 100 + 260 * k + int(rng.integers(0, 200))
        blk[at:at + 6] = piece
    return bytes(blk)


def mixed_blocks(nblk):
    """nblk 64 KiB blocks: text windows, with a constant block third from the end and the random
    block second from the end (both among the remainder blocks whenever there are two or more)."""
    out = [text_block(i) for i in range(nblk)]
    if nblk >= 2:
        out[nblk - 2] = random_block()
    if nblk >= 3:
        out[nblk - 3] = b"\x37" * BLOCK
    return out


def case_list(g):
    """[(name, call, mode, blocks, (slot pitch, first slot's offset))]; call: "batch" or "frag"."""
    aligned, odd = (MAXC + 22, 0), (MAXC + 11, 3)
    assert aligned[0] % 16 == 0 and odd[0] % 2 == 1
    cases = []
    for mode in MODES:
        for nb in NBLK:
            cases.append(("A-%s-%s" % (nb, mode), "batch", mode, mixed_blocks(nblk_of(nb, g)), aligned))
        for last in (1, 1023, 1025, 65535):
            cases.append(("B-3-%d-%s" % (last, mode), "batch", mode, [text_block(1), text_block(2), text_block(3, last)],
                          aligned))
        cases.append(("B-g+3-1025-%s" % mode, "batch", mode, mixed_blocks(g + 2) + [text_block(9, 1025)], aligned))
        for nb in ("5", "g+1"):
            cases.append(("C-%s-%s" % (nb, mode), "batch", mode, mixed_blocks(nblk_of(nb, g)), odd))
        for nb in ("3", "g+1"):
            cases.append(("D-%s-%s" % (nb, mode), "frag", mode, mixed_blocks(nblk_of(nb, g)), aligned))
        cases.append(("D-odd-%s" % mode, "frag", mode, mixed_blocks(4) + [text_block(5, 4321)], odd))
        cases.append(("E-5000-%s" % mode, "frag", mode, [text_block(4, 5000)], aligned))
        cases.append(("F-%s" % mode, "batch", mode, [text_block(7, 100), text_block(6), fallback_block(), b""], odd))
    return cases


CASE_NAMES = [c[0] for c in case_list(256)]  # (the names do not depend on g)


def canary(n):
    return ((np.arange(n, dtype=np.int64) * 131 + 7) & 0xFF).astype(np.uint8)


def run_case(sm, case):
    """One call on the device: (d_out_len as u32 array, the slots' bytes [0, len) behind one
    another, sm_ctx_last_batch_parts after the call)."""
    import torch
    _, call, mode, blocks, (pitch, first) = case
    dev = torch.device("cuda", 0)
    lens = np.array([len(b) for b in blocks], np.int64)
    total = int(lens.sum())
    n = len(blocks)
    d_in = torch.from_numpy(np.frombuffer(b"".join(blocks) + bytes(16), np.uint8).copy()).to(dev)
    in_off = torch.from_numpy(np.cumsum(lens) - lens).to(dev)
    in_len = torch.from_numpy(lens.astype(np.int32)).to(dev)
    fill = canary(first + n * pitch)
    d_out = torch.from_numpy(fill.copy()).to(dev)
    assert d_out.data_ptr() % 16 == 0
    off = first + np.arange(n, dtype=np.int64) * pitch
    out_off = torch.from_numpy(off).to(dev)
    out_len = torch.full((n,), 7, dtype=torch.int32, device=dev)
    if call == "batch":
        sm.compress_batch_device(d_in, in_off, in_len, d_out, out_off, out_len, mode=mode)
    else:
        sm.compress_fragments_device(d_in, in_off, in_len, d_out, out_off, out_len, total, mode=mode)
    parts = sm.last_batch_parts(0)  # the remainder blocks this call parsed in parts
    torch.cuda.synchronize()
    cl = out_len.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    out = d_out.cpu().numpy()
    room = 32 + lens + lens // 6 + (5 if call == "batch" else 0)
    assert (cl <= room).all(), (case[0], cl[cl > room][:4])
    body = np.concatenate([out[o:o + c] for o, c in zip(off, cl)] + [np.zeros(0, np.uint8)])
    # nothing past a slot's documented room, nor before the first slot, was written
    keep = np.ones(out.size, bool)
    for o, r in zip(off, room):
        keep[o:o + r] = False
    assert np.array_equal(out[keep], fill[keep]), case[0]
    return cl.astype(np.uint32), body, parts


def key(name, what):
    return name.replace("/", "_") + "." + what


def run_all(sm):
    import torch
    g = torch.cuda.get_device_properties(0).multi_processor_count
    res = {}
    for case in case_list(g):
        cl, body, parts = run_case(sm, case)
        res[key(case[0], "len")] = cl
        res[key(case[0], "bytes")] = body
        res[key(case[0], "parts")] = np.array([parts])
    res["threads"] = np.array(run_threads(sm, g))
    return g, res


THREADS, THREAD_CALLS = 4, 25


def run_threads(sm, g):
    """THREADS host threads, each THREAD_CALLS calls of its own 3-block batch into its own slots,
    all on the one context and torch's one current stream: [calls whose slots or lengths differ
    from the same batch compressed alone, calls in all].  (A call's parts go through a scratch the
    context keeps per stream; its launches must not interleave with another thread's.)"""
    import threading
    import torch
    dev = torch.device("cuda", 0)
    pitch = MAXC + 22
    jobs = []
    for t in range(THREADS):
        blocks = [text_block(40 + 3 * t + k) for k in range(3)]
        d_in = torch.from_numpy(np.frombuffer(b"".join(blocks), np.uint8).copy()).to(dev)
        in_off = torch.arange(3, dtype=torch.int64, device=dev) * BLOCK
        in_len = torch.full((3,), BLOCK, dtype=torch.int32, device=dev)
        out_off = torch.arange(3, dtype=torch.int64, device=dev) * pitch
        outs = [(torch.zeros(3 * pitch, dtype=torch.uint8, device=dev), torch.zeros(3, dtype=torch.int32, device=dev))
                for _ in range(THREAD_CALLS + 1)]
        jobs.append((d_in, in_off, in_len, out_off, outs))
    for d_in, in_off, in_len, out_off, outs in jobs:  # each batch alone: the last output pair
        sm.compress_batch_device(d_in, in_off, in_len, outs[-1][0], out_off, outs[-1][1], mode="fast")
    torch.cuda.synchronize()
    start = threading.Barrier(THREADS)

    def work(job):
        d_in, in_off, in_len, out_off, outs = job
        start.wait()
        for d_out, out_len in outs[:-1]:
            sm.compress_batch_device(d_in, in_off, in_len, d_out, out_off, out_len, mode="fast")

    threads = [threading.Thread(target=work, args=(j,)) for j in jobs]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    torch.cuda.synchronize()
    bad = 0
    for d_in, in_off, in_len, out_off, outs in jobs:
        want_out, want_len = outs[-1]
        assert int(want_len.min()) > 0 and int(want_len.max()) <= MAXC
        for d_out, out_len in outs[:-1]:
            bad += 0 if (torch.equal(d_out, want_out) and torch.equal(out_len, want_len)) else 1
    return [bad, THREADS * THREAD_CALLS]


# ---- CPU ----------------------------------------------------------------------------------------

def test_parts_rule(sm):
    """The library's (rem, parts) for every nblk up to three grids on a few grid sizes equals the
    rule as the design states it, and keeps its invariants."""
    for g in (1, 2, 3, 64, 104, 256, 304):
        for nblk in range(0, 3 * g + 2):
            rem, parts = sm.batch_parts_plan(nblk, g)
            assert (rem, parts) == rule(nblk, g), (g, nblk)
            if rem:
                assert rem == nblk % g and rem <= g // 2 and (nblk - rem) % g == 0
                assert parts in (2, 4, 8, 16) and rem * parts <= g
                assert parts == 16 or rem * parts * 2 > g  # the largest such power of two
                assert 64 // parts >= 4  # a part is at least 4 super-chunks
            else:
                assert parts == 0 and (nblk % g == 0 or nblk % g > g // 2)
    assert sm.batch_parts_plan(10000, 256) == (16, 16)  # the benchmark's batch
    assert sm.batch_parts_plan(1288, 256) == (8, 16) and sm.batch_parts_plan(64, 256) == (64, 4)
    assert sm.batch_parts_plan(5, 0) == (0, 0)


def test_fallback_block_passes_the_screen():
    """CPU: the designed block repeats an anchor word of the screen 29 times in its first 8 KiB."""
    blk = np.frombuffer(fallback_block(), np.uint8)[:8192].astype(np.uint64)
    words = (blk[:-3] | (blk[1:-2] << 8) | (blk[2:-1] << 16) | (blk[3:] << 24)).astype(np.uint64)
    anchors = words[((words * HASH_MUL) & 0xFFFFFFFF) >> 26 == 0]
    vals, counts = np.unique(anchors, return_counts=True)
    assert counts.max() == 30 and int((counts - 1).sum()) >= 29


def test_case_names_are_unique():
    assert len(set(CASE_NAMES)) == len(CASE_NAMES)
    for g in (104, 256, 304):
        assert [c[0] for c in case_list(g)] == CASE_NAMES


# ---- GPU ----------------------------------------------------------------------------------------

def _child(parts_on):
    """Every case in a fresh process (this file as a script): {key: array}."""
    env = {k: v for k, v in os.environ.items() if k != "SM_BATCH_PARTS"}
    if not parts_on:
        env["SM_BATCH_PARTS"] = "0"
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "cases.npz")
        subprocess.run([sys.executable, os.path.abspath(__file__), path], check=True, env=env, timeout=300)
        with np.load(path) as z:
            return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def expected(gpu_available):
    """SM_BATCH_PARTS=0: the whole-block parse of every block."""
    return _child(False)


@pytest.fixture(scope="module")
def got(gpu_available):
    """The library as shipped: the remainder rule on.  (A process of its own as well: the switch is
    read once per process, and this one may have been started with it set.)"""
    return _child(True)


@pytest.mark.gpu
def test_cases_reach_both_paths(sm, got):
    """On this device the case list has batches with and without remainder parts, with whole rounds
    before them and without, and every part count the rule can give for a short batch."""
    g = int(got["grid"][0])
    plans = {c[0]: sm.batch_parts_plan(len(c[3]), g) for c in case_list(g)}
    assert plans["A-1-fast"] == (1, 16) and plans["A-g/2+1-fast"] == (0, 0) and plans["A-2g-1-fast"] == (0, 0)
    assert plans["A-g/2-fast"] == (g // 2, 2) and plans["A-g+1-fast"] == (1, 16)
    assert plans["A-g+16-fast"][0] == 16 and plans["B-g+3-1025-fast"][0] == 3 and plans["F-fast"][0] == 4


@pytest.mark.gpu
def test_parts_path_ran(sm, got, expected):
    """The library's own account of every call (sm_ctx_last_batch_parts): with the rule on, the
    remainder blocks the rule gives were parsed in parts -- no silent fall-back to the whole-block
    path -- and with SM_BATCH_PARTS=0 none were.  So the comparisons below set the new kernels'
    bytes against the whole-block kernel's."""
    g = int(got["grid"][0])
    some = 0
    for case in case_list(g):
        rem, _ = rule(len(case[3]), g)
        assert int(got[key(case[0], "parts")][0]) == rem, case[0]
        assert int(expected[key(case[0], "parts")][0]) == 0, case[0]
        some += rem > 0
    assert some >= len(CASE_NAMES) - 4  # all but the two batch sizes without a remainder in parts, per mode


@pytest.mark.gpu
def test_threads_on_one_stream(got, expected):
    """Calls from several host threads on one context and one stream leave each batch's own bytes,
    with the rule on and off."""
    for res in (got, expected):
        bad, calls = (int(x) for x in res["threads"])
        assert calls == THREADS * THREAD_CALLS and bad == 0, (bad, calls)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_same_bytes_as_whole_block_parse(sm, oracle, got, expected, name):
    g = int(got["grid"][0])
    assert int(expected["grid"][0]) == g
    case = next(c for c in case_list(g) if c[0] == name)
    cl, body = got[key(name, "len")], got[key(name, "bytes")]
    want_cl, want_body = expected[key(name, "len")], expected[key(name, "bytes")]
    assert np.array_equal(cl, want_cl), (name, np.nonzero(cl != want_cl)[0][:8])
    if not np.array_equal(body, want_body):
        ends = np.cumsum(cl.astype(np.int64))
        bad = np.nonzero(body != want_body)[0]
        raise AssertionError("%s: %d bytes differ, the first in block %d" % (name, bad.size, np.searchsorted(ends, bad[0], "right")))
    at = 0
    for blk, c in zip(case[3], cl):
        s = body[at:at + int(c)].tobytes()
        at += int(c)
        assert oracle.uncompress(s if case[1] == "batch" else streams.varint(len(blk)) + s) == blk, name
    if name.startswith("F-"):  # the fallback block is one literal: header, 3-byte tag, the bytes
        assert int(cl[2]) == 3 + 3 + BLOCK and int(cl[3]) == 1 and bytes(body[-1:]) == b"\0"


if __name__ == "__main__":  # the child process of `expected` and `got`
    grid, result = run_all(load_package())
    result["grid"] = np.array([grid])
    np.savez(sys.argv[1], **result)
