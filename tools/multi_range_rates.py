"""Rates of the multi-stream library's ranged decode (smm_uncompress_ranges_device) on the headline
text as ONE raw stream: bench.py text_blocks, 10,000 x 64 KiB windows of the text files, compressed
in fast mode by smm_compress_device, which hands out the stream's 10,000-entry index.

What is timed, each call by a pair of HIP events around it on the current stream, `--reps` times
after `--warmup` untimed rounds, the cases alternating inside one process (every repetition times
each of them once; median, minimum and maximum in milliseconds):

  whole_stream_indexed          smm_uncompress_device with the index: the only route to any byte today
  range_1_fragment              one range of one fragment, in the middle of the stream
  range_16_fragments            one range of 16 fragments
  range_1MiB_unaligned          one range of 1 MiB at an unaligned lo
  ranges_10000_x_4KiB           10,000 ranges of 4 KiB at seeded random lo, one call

and, with --parent-lib, a same-box A/B of smm_compress_device and smm_uncompress_device between a
build of the parent commit and this build, the two interleaved call by call: the medians may differ
by no more than the parent's own min-max spread.  Clocks are read before and after.  Needs a GPU.

    python tools/multi_range_rates.py --out profiles/multi_range_rates.json [--parent-lib PATH]
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


def alternate(torch, cases, reps, warmup):
    """{name: stats} of the callables in `cases`, each timed once per repetition, in turn."""
    for _ in range(warmup):
        for fn in cases.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in cases}
    for _ in range(reps):
        for k, fn in cases.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                "reps": reps} for k, v in ms.items()}


class Build:
    """smm_compress_device and smm_uncompress_device of one build of the multi library, with a ctx of
    its own, through the same ctypes path for both sides of the A/B."""

    def __init__(self, path):
        vp, u32, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32
        self.lib = ctypes.CDLL(path)
        self.lib.smm_ctx_create.restype = vp
        self.lib.smm_ctx_create.argtypes = [ctypes.c_int]
        self.lib.smm_version.restype = ctypes.c_char_p
        self.lib.smm_compress_device.restype = i32
        self.lib.smm_compress_device.argtypes = [vp, vp, vp, vp, u32, u32, vp, vp, vp, vp, vp, vp, ctypes.c_int, vp]
        self.lib.smm_uncompress_device.restype = i32
        self.lib.smm_uncompress_device.argtypes = [vp, vp, vp, vp, u32, u32, vp, vp, vp, vp, vp, vp, vp, vp]
        self.ctx = self.lib.smm_ctx_create(0)
        assert self.ctx
        self.version = self.lib.smm_version().decode()

    def compress(self, d_in, in_off, in_len, n, m, d_out, out_off, out_len, status, first, pos, stream):
        rc = self.lib.smm_compress_device(self.ctx, d_in.data_ptr(), in_off.data_ptr(), in_len.data_ptr(), n, m,
                                          d_out.data_ptr(), out_off.data_ptr(), out_len.data_ptr(), status.data_ptr(),
                                          first.data_ptr(), pos.data_ptr(), 1, stream)
        assert rc == 0

    def uncompress(self, d_in, in_off, in_len, n, m, d_out, out_off, cap, out_len, status, first, pos, stream):
        rc = self.lib.smm_uncompress_device(self.ctx, d_in.data_ptr(), in_off.data_ptr(), in_len.data_ptr(), n, m,
                                            d_out.data_ptr(), out_off.data_ptr(), cap.data_ptr(), out_len.data_ptr(),
                                            status.data_ptr(), first.data_ptr(), pos.data_ptr(), stream)
        assert rc == 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="libsnappy_mi355x_multi.so built from the parent commit")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import bench
    from framing_rates import clocks
    if not torch.cuda.is_available():
        print("multi_range_rates.py needs a GPU", file=sys.stderr)
        return 2
    clocks_before = clocks()
    sm = bench.load_package()
    mu = importlib.import_module("snappy_jl_amd.multi")
    dev = torch.device("cuda", 0)
    nblk = args.blocks
    n = nblk * BLOCK
    batch = bench.Batch(bench.text_blocks(nblk, 0x5EED), dev)
    d_in, d_dec = batch.d_in, batch.d_dec
    assert d_in.numel() == n

    def i64(a):
        return torch.from_numpy(np.asarray(a, dtype=np.int64)).to(dev)

    def i32(a):
        return torch.from_numpy(np.asarray(a, dtype=np.int64).astype(np.uint32).view(np.int32)).to(dev)

    # ---- the one stream and the encoder's index
    room = 32 + n + n // 6
    zero, one_len, cap = i64([0]), i32([n]), i32([n])
    d_stream = torch.empty(room, dtype=torch.uint8, device=dev)
    s_len = torch.zeros(1, dtype=torch.int32, device=dev)
    status = torch.full((1,), -1, dtype=torch.int32, device=dev)
    first = torch.zeros(2, dtype=torch.int32, device=dev)
    pos = torch.zeros(nblk, dtype=torch.int32, device=dev)
    dec_len = torch.zeros(1, dtype=torch.int32, device=dev)
    mu.compress_streams_device(d_in, zero, one_len, nblk, d_stream, zero, s_len, status, first, pos, mode="fast")
    torch.cuda.synchronize()
    assert int(status.item()) == 0 and first.tolist() == [0, nblk]
    stream_bytes = int(s_len.item())

    def whole():
        mu.uncompress_streams_device(d_stream, zero, s_len, nblk, d_dec, zero, cap, dec_len, status, first, pos)

    d_dec.fill_(0xAA)
    whole()
    torch.cuda.synchronize()
    assert int(status.item()) == 0 and mu.last_indexed(0) == 1 and bool(torch.equal(d_dec, d_in))

    # ---- the ranges
    shapes = {}

    def ranges_case(name, ranges):
        k = len(ranges)
        slots = sum(mu.range_fragment_count(lo, ln) for lo, ln in ranges)
        out_off = np.concatenate([[0], np.cumsum([(ln + 15) // 16 * 16 for lo, ln in ranges])])
        d_out = torch.full((int(out_off[-1]),), 0xAA, dtype=torch.uint8, device=dev)
        d_rs, d_lo, d_ln, d_oo = i32([0] * k), i32([r[0] for r in ranges]), i32([r[1] for r in ranges]), i64(out_off[:-1])
        d_ol = torch.zeros(k, dtype=torch.int32, device=dev)
        d_rst = torch.full((k,), -1, dtype=torch.int32, device=dev)

        def call():
            mu.uncompress_stream_ranges_device(d_stream, zero, s_len, first, pos, d_rs, d_lo, d_ln, slots, d_out, d_oo, d_ol,
                                               d_rst)

        call()
        torch.cuda.synchronize()
        assert not bool(d_rst.any()) and d_ol.cpu().tolist() == [r[1] for r in ranges]
        for i in sorted({0, k // 2, k - 1}):
            lo, ln = ranges[i]
            o = int(out_off[i])
            assert bool(torch.equal(d_out[o:o + ln], d_in[lo:lo + ln])), (name, i)
        shapes[name] = {"ranges": k, "slots": slots, "bytes": int(sum(r[1] for r in ranges))}
        return call

    mid = (nblk // 2) * BLOCK
    rng = np.random.default_rng(0x5EED)
    cases = {
        "whole_stream_indexed": whole,
        "range_1_fragment": ranges_case("range_1_fragment", [(mid, BLOCK)]),
        "range_16_fragments": ranges_case("range_16_fragments", [(mid, 16 * BLOCK)]),
        "range_1MiB_unaligned": ranges_case("range_1MiB_unaligned", [(mid + 12345, 1 << 20)]),
        "ranges_10000_x_4KiB": ranges_case("ranges_10000_x_4KiB", [(int(lo), 4096) for lo in rng.integers(0, n - 4096, 10000)]),
    }
    res = alternate(torch, cases, args.reps, args.warmup)
    for k, v in shapes.items():
        res[k].update(v)
    whole_ms = res["whole_stream_indexed"]["median_ms"]
    report = {
        "workload": "one raw stream of %d x 64 KiB text windows (bench.py text_blocks, seed 0x5EED), %d bytes, fast mode: "
                    "%d bytes, with the encoder's index" % (nblk, n, stream_bytes),
        "method": "HIP events around each call on one stream, the cases alternating; %d warm-up rounds, %d timed; "
                  "median, min, max" % (args.warmup, args.reps),
        "device": torch.cuda.get_device_name(0),
        "library": sm.version(),
        "multi_library": mu.version(),
        "clocks_before": clocks_before,
        "ms": res,
        "faster_than_whole_stream": {k: bool(v["median_ms"] < whole_ms) for k, v in res.items() if k != "whole_stream_indexed"},
    }

    # ---- the existing calls, parent build against this build, interleaved call by call
    if args.parent_lib:
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        builds = {"parent": Build(args.parent_lib), "this": Build(mu.LIB_PATH)}
        ab = {}
        r = alternate(torch, {k: (lambda b=b: b.compress(d_in, zero, one_len, 1, nblk, d_stream, zero, s_len, status, first,
                                                         pos, stream)) for k, b in builds.items()}, args.reps, args.warmup)
        assert int(status.item()) == 0 and int(s_len.item()) == stream_bytes
        ab["smm_compress_device"] = r
        d_dec.fill_(0xAA)
        r = alternate(torch, {k: (lambda b=b: b.uncompress(d_stream, zero, s_len, 1, nblk, d_dec, zero, cap, dec_len, status,
                                                           first, pos, stream)) for k, b in builds.items()},
                      args.reps, args.warmup)
        assert int(status.item()) == 0 and bool(torch.equal(d_dec, d_in))
        ab["smm_uncompress_device"] = r
        report["ab_parent_vs_this"] = {
            "parent_library": builds["parent"].version, "this_library": builds["this"].version,
            "calls": {k: {"parent": v["parent"], "this": v["this"],
                          "median_difference_ms": round(v["this"]["median_ms"] - v["parent"]["median_ms"], 4),
                          "parent_spread_ms": round(v["parent"]["max_ms"] - v["parent"]["min_ms"], 4),
                          "within_parent_spread": bool(abs(v["this"]["median_ms"] - v["parent"]["median_ms"])
                                                       <= v["parent"]["max_ms"] - v["parent"]["min_ms"])}
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
