"""Rates of the framing library's seek index and ranged decode, on the stream of DESIGN.md 8.1
(bench.py text_blocks: 10,000 x 64 KiB windows of the text files, framed by this build).

What is timed, each call by a pair of HIP events around it on the current stream, `--reps` times
after `--warmup` untimed calls (median, minimum and maximum in milliseconds; the method of
tools/framing_rates.py):

  whole_stream_walk_and_decode   smf_uncompress_device: the only route to any byte without an index
  compress / compress_indexed    smf_compress_device next to smf_compress_indexed_device
  a_index_then_chunks            the encoder's index into smf_uncompress_chunks_device: no walk
  b_range_1_chunk / _16_chunks / _1MiB_unaligned   one range, in the middle of the stream
  c_10000_ranges_4KiB            10,000 ranges of 4 KiB at random lo, one call

and, with --parent-lib, a same-box A/B of smf_compress_device and smf_uncompress_chunks_device
between a build of the parent commit and this build, the two interleaved call by call: the medians
may differ by no more than the parent's own min-max spread.  Needs a GPU.

    python tools/framing_range_rates.py --out profiles/framing_range_rates.json [--parent-lib PATH]
"""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
BLOCK = 65536


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "reps": len(ms)}


def timed(torch, fns, reps, warmup):
    """The calls `fns`, interleaved: one timed call of each per repetition."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return [summary(m) for m in ms]


class Build:
    """smf_compress_device and smf_uncompress_chunks_device of one build of the framing library,
    through the same ctypes path for both sides of the A/B."""

    def __init__(self, path, fr):
        vp, u32, u64, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int32
        self.lib = ctypes.CDLL(path)
        self.lib.smf_ctx_create.restype = vp
        self.lib.smf_ctx_create.argtypes = [ctypes.c_int]
        self.lib.smf_version.restype = ctypes.c_char_p
        self.lib.smf_compress_device.restype = i32
        self.lib.smf_compress_device.argtypes = [vp, vp, u64, vp, u64, vp, vp, ctypes.c_int, vp]
        self.lib.smf_uncompress_chunks_device.restype = i32
        self.lib.smf_uncompress_chunks_device.argtypes = [vp, vp, ctypes.POINTER(fr.Chunks), u32, vp, u64, vp, vp, vp, vp]
        self.ctx = self.lib.smf_ctx_create(0)
        assert self.ctx
        self.version = self.lib.smf_version().decode()

    def compress(self, d_in, d_out, d_len, d_st, stream):
        rc = self.lib.smf_compress_device(self.ctx, d_in.data_ptr(), d_in.numel(), d_out.data_ptr(), d_out.numel(),
                                          d_len.data_ptr(), d_st.data_ptr(), 1, stream)
        assert rc == 0

    def uncompress_chunks(self, d_in, ch, nchunks, d_out, d_cs, d_len, d_st, stream):
        rc = self.lib.smf_uncompress_chunks_device(self.ctx, d_in.data_ptr(), ctypes.byref(ch), nchunks, d_out.data_ptr(),
                                                   d_out.numel(), d_cs.data_ptr(), d_len.data_ptr(), d_st.data_ptr(), stream)
        assert rc == 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="libsnappy_mi355x_framing.so built from the parent commit")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import bench
    from framing_rates import clocks
    if not torch.cuda.is_available():
        print("framing_range_rates.py needs a GPU", file=sys.stderr)
        return 2
    sm = bench.load_package()
    fr = importlib.import_module("snappy_jl_amd.framing")
    dev = torch.device("cuda", 0)
    nblk = args.blocks
    batch = bench.Batch(bench.text_blocks(nblk, 0x5EED), dev)
    d_in = batch.d_in
    n = nblk * BLOCK
    assert d_in.numel() == n
    res = {}

    def one(name, fn):
        res[name] = timed(torch, [fn], args.reps, args.warmup)[0]

    def i64(values):
        return torch.from_numpy(np.array(values, dtype=np.int64)).to(dev)

    # ---- the encoder and its index
    d_framed = torch.empty(fr.max_framed_length(n), dtype=torch.uint8, device=dev)
    d_len = torch.zeros(1, dtype=torch.int64, device=dev)
    d_st = torch.zeros(1, dtype=torch.int32, device=dev)
    arrays = fr.device_chunks(nblk)
    d_off = torch.zeros(nblk + 1, dtype=torch.int64, device=dev)
    d_nc = torch.zeros(1, dtype=torch.int32, device=dev)
    res["compress"], res["compress_indexed"] = timed(torch, [
        lambda: fr.compress_framed_device(d_in, d_framed, d_len, d_st, mode="fast"),
        lambda: fr.compress_framed_indexed_device(d_in, d_framed, d_len, d_st, arrays, d_off, d_nc, mode="fast"),
    ], args.reps, args.warmup)
    framed_len = int(d_len.item())
    assert int(d_st.item()) == 0 and int(d_nc.item()) == nblk and int(d_off[-1].item()) == n

    # ---- the route without an index: walk + decode of the whole stream
    d_dec = batch.d_dec
    d_dec.fill_(0xAA)
    one("whole_stream_walk_and_decode",
        lambda: fr.uncompress_framed_device(d_framed, d_dec, d_len, d_st, n=framed_len))
    assert int(d_st.item()) == 0 and bool(torch.equal(d_dec, d_in))

    # ---- (a) the encoder's index, no walk
    d_cs = torch.zeros(nblk, dtype=torch.int32, device=dev)
    d_dec.fill_(0xAA)
    one("a_index_then_chunks", lambda: fr.uncompress_chunks_device(d_framed, arrays, nblk, d_dec, d_cs, d_len, d_st))
    assert int(d_st.item()) == 0 and int(d_len.item()) == n and bool(torch.equal(d_dec, d_in))

    # ---- (b), (c): ranges
    def ranges_case(name, ranges):
        k = len(ranges)
        slots = sum(fr.range_chunk_count(lo, ln) for lo, ln in ranges)
        out_off = np.concatenate([[0], np.cumsum([(ln + 15) // 16 * 16 for lo, ln in ranges])])
        d_out = torch.full((int(out_off[-1]),), 0xAA, dtype=torch.uint8, device=dev)
        d_lo, d_ln, d_oo = i64([r[0] for r in ranges]), i64([r[1] for r in ranges]), i64(out_off[:-1])
        d_ol = torch.zeros(k, dtype=torch.int64, device=dev)
        d_rs = torch.zeros(k, dtype=torch.int32, device=dev)
        one(name, lambda: fr.uncompress_ranges_device(d_framed, arrays, d_off, nblk, d_lo, d_ln, slots, d_out, d_oo, d_ol,
                                                      d_rs, n=framed_len))
        assert not bool(d_rs.any()) and d_ol.cpu().tolist() == [r[1] for r in ranges]
        for i in sorted({0, k // 2, k - 1}):
            lo, ln = ranges[i]
            o = int(out_off[i])
            assert bool(torch.equal(d_out[o:o + ln], d_in[lo:lo + ln])), (name, i)
        res[name]["ranges"], res[name]["slots"], res[name]["bytes"] = k, slots, int(sum(r[1] for r in ranges))

    mid = (nblk // 2) * BLOCK
    ranges_case("b_range_1_chunk", [(mid, BLOCK)])
    ranges_case("b_range_16_chunks", [(mid, 16 * BLOCK)])
    ranges_case("b_range_1MiB_unaligned", [(mid + 12345, 1 << 20)])
    rng = np.random.default_rng(0x5EED)
    ranges_case("c_10000_ranges_4KiB", [(int(lo), 4096) for lo in rng.integers(0, n - 4096, 10000)])

    report = {
        "workload": "%d x 64 KiB text blocks (bench.py text_blocks, seed 0x5EED), %d bytes, framed: %d bytes"
                    % (nblk, n, framed_len),
        "method": "HIP events around each call on one stream; %d warm-ups, %d timed calls; median, min, max"
                  % (args.warmup, args.reps),
        "device": torch.cuda.get_device_name(0),
        "library": sm.version(),
        "framing_library": fr.version(),
        "ms": res,
    }
    whole = res["whole_stream_walk_and_decode"]["median_ms"]
    report["faster_than_whole_stream"] = {k: bool(v["median_ms"] < whole) for k, v in res.items()
                                          if k.startswith(("a_", "b_"))}

    # ---- the existing calls, parent build against this build, interleaved
    if args.parent_lib:
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        builds = [Build(args.parent_lib, fr), Build(fr.LIB_PATH, fr)]
        ch = fr.Chunks(*(arrays[k].data_ptr() for k in ("type", "pay_off", "pay_len", "crc", "ulen")))
        ab = {}
        ab["compress"] = timed(torch, [lambda b=b: b.compress(d_in, d_framed, d_len, d_st, stream) for b in builds],
                               args.reps, args.warmup)
        assert int(d_st.item()) == 0 and int(d_len.item()) == framed_len
        ab["uncompress_chunks"] = timed(
            torch, [lambda b=b: b.uncompress_chunks(d_framed, ch, nblk, d_dec, d_cs, d_len, d_st, stream) for b in builds],
            args.reps, args.warmup)
        assert int(d_st.item()) == 0 and bool(torch.equal(d_dec, d_in))
        report["ab_parent_vs_this"] = {
            "parent_library": builds[0].version, "this_library": builds[1].version,
            "calls": {k: {"parent": v[0], "this": v[1],
                          "median_difference_ms": round(v[1]["median_ms"] - v[0]["median_ms"], 4),
                          "parent_spread_ms": round(v[0]["max_ms"] - v[0]["min_ms"], 4),
                          "within_parent_spread": bool(abs(v[1]["median_ms"] - v[0]["median_ms"])
                                                       <= v[0]["max_ms"] - v[0]["min_ms"])}
                      for k, v in ab.items()}}
    report["clocks_after"] = clocks()
    line = json.dumps(report, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
