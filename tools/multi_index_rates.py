"""Rates of the multi-stream library's index build (smm_index_device) on the workload of
tools/multi_rates.py: 640 streams of 1 MiB, each 16 consecutive 64 KiB windows of the headline text
(bench.py text_blocks), compressed in fast mode by smm_compress_device -- and the same bytes as 8
streams of 80 MiB, the shape one wave per stream does not help.

    (a) smm_uncompress_device without an index (stream order) -- with --baseline-lib, through that
        build of libsnappy_mi355x_multi.so (the parent commit's, built beside this one)
    (b) smm_index_device alone
    (c) smm_index_device, then smm_uncompress_device with the index it built
    (d) smm_uncompress_device with the compressor's own index
    (e) (b) and (c) on the 8 long streams

The cases of one shape alternate inside one process: every repetition times each of them once, by
a pair of HIP events on the current stream, after `--warmup` untimed rounds; the report gives the
median, the minimum and the maximum in milliseconds.  Kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats` (a short one: --reps 3), whose kernel_stats CSV --kernel-stats
folds into the report.  Needs a GPU; nothing here falls back to the CPU.

    python tools/multi_index_rates.py --out profiles/multi_index_rates.json
"""
import argparse
import csv
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


def baseline_library(path):
    """smm_uncompress_device of another build of the companion library, with a ctx of its own."""
    L = ctypes.CDLL(path)
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    L.smm_ctx_create.restype = vp
    L.smm_ctx_create.argtypes = [ctypes.c_int]
    L.smm_version.restype = ctypes.c_char_p
    L.smm_uncompress_device.restype = ctypes.c_int32
    L.smm_uncompress_device.argtypes = [vp, vp, vp, vp, u32, u32, vp, vp, vp, vp, vp, vp, vp, vp]
    ctx = L.smm_ctx_create(0)
    if not ctx:
        raise RuntimeError("no ctx from %s" % path)
    return L, ctx


def kernel_stats(path):
    """The k_index_* rows (and the decoders') of a rocprofv3 kernel_stats CSV."""
    rows = {}
    with open(path) as fh:
        for r in csv.DictReader(fh):
            name = r.get("Name", "")
            short = name.split("(")[0].split("::")[-1]
            if "k_index" in name or "k_decompress" in name:
                rows[short] = {"calls": int(r["Calls"]), "average_us": round(float(r["AverageNs"]) / 1e3, 1),
                               "min_us": round(float(r["MinNs"]) / 1e3, 1), "max_us": round(float(r["MaxNs"]) / 1e3, 1)}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=640)
    ap.add_argument("--per-stream", type=int, default=16, help="64 KiB windows per stream")
    ap.add_argument("--long-streams", type=int, default=8, help="0: skip case (e)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import bench
    if not torch.cuda.is_available():
        print("multi_index_rates.py needs a GPU", file=sys.stderr)
        return 2
    sm = bench.load_package()
    mu = importlib.import_module("snappy_jl_amd.multi")
    dev = torch.device("cuda", 0)
    nblk = args.streams * args.per_stream
    n = nblk * BLOCK
    batch = bench.Batch(bench.text_blocks(nblk, 0x5EED), dev)
    base = baseline_library(args.baseline_lib) if args.baseline_lib else None

    def i64(a):
        return torch.from_numpy(np.asarray(a, dtype=np.int64)).to(dev)

    def i32(a):
        return torch.from_numpy(np.asarray(a, dtype=np.int64).astype(np.uint32).view(np.int32)).to(dev)

    def shape(ns):
        """The batch's bytes as ns streams: compressed with the compressor's index, and the cases over them."""
        per = nblk // ns
        slen = per * BLOCK
        room = (32 + slen + slen // 6 + 255) // 256 * 256
        in_off, in_len, cap = i64(np.arange(ns) * slen), i32(np.full(ns, slen)), i32(np.full(ns, slen))
        out_off = i64(np.arange(ns) * room)
        d_streams = torch.empty(ns * room, dtype=torch.uint8, device=dev)
        s_len = torch.zeros(ns, dtype=torch.int32, device=dev)
        status = torch.full((ns,), -1, dtype=torch.int32, device=dev)
        c_first = torch.zeros(ns + 1, dtype=torch.int32, device=dev)
        c_pos = torch.zeros(nblk, dtype=torch.int32, device=dev)
        mu.compress_streams_device(batch.d_in, in_off, in_len, nblk, d_streams, out_off, s_len, status, c_first, c_pos,
                                   mode="fast")
        assert int(status.abs().sum()) == 0
        b_first = torch.full((ns + 1,), -1, dtype=torch.int32, device=dev)
        b_pos = torch.full((nblk,), -1, dtype=torch.int32, device=dev)
        built = torch.zeros(ns, dtype=torch.uint8, device=dev)
        i_status = torch.full((ns,), -1, dtype=torch.int32, device=dev)
        dec_len = torch.zeros(ns, dtype=torch.int32, device=dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def index():
            mu.index_streams_device(d_streams, out_off, s_len, nblk, b_first, b_pos, built, i_status, d_out_cap=cap)

        def decode(first, pos):
            mu.uncompress_streams_device(d_streams, out_off, s_len, nblk if first is not None else 0, batch.d_dec, in_off,
                                         cap, dec_len, status, first, pos)

        def stream_order():
            if base is None:
                return decode(None, None)
            st = base[0].smm_uncompress_device(base[1], d_streams.data_ptr(), out_off.data_ptr(), s_len.data_ptr(), ns, 0,
                                               batch.d_dec.data_ptr(), in_off.data_ptr(), cap.data_ptr(), dec_len.data_ptr(),
                                               status.data_ptr(), None, None, stream)
            assert st == 0

        def index_then_decode():
            index()
            decode(b_first, b_pos)

        # once, checked: the built index is the compressor's, and every path gives the input back
        index()
        torch.cuda.synchronize()
        assert int(i_status.abs().sum()) == 0 and int(built.sum()) == ns
        assert bool(torch.equal(b_first, c_first)) and bool(torch.equal(b_pos, c_pos))
        for fn, nidx in ((stream_order, 0 if base is None else None), (index_then_decode, ns), (lambda: decode(c_first, c_pos), ns)):
            batch.d_dec.fill_(0xAA)
            fn()
            torch.cuda.synchronize()
            assert int(status.abs().sum()) == 0 and bool(torch.equal(batch.d_dec, batch.d_in))
            assert nidx is None or mu.last_indexed(0) == nidx
        return {"a_stream_order": stream_order, "b_index": index, "c_index_then_indexed": index_then_decode,
                "d_compressor_index": lambda: decode(c_first, c_pos)}, int(s_len.to(torch.int64).sum())

    cases, stream_bytes = shape(args.streams)
    res = alternate(torch, cases, args.reps, args.warmup)
    report = {
        "workload": "%d streams of %d x 64 KiB text windows (bench.py text_blocks, seed 0x5EED), %d bytes, fast mode"
                    % (args.streams, args.per_stream, n),
        "method": "HIP events around each case on one stream, the cases alternating; %d warm-up rounds, %d timed; "
                  "median, min, max" % (args.warmup, args.reps),
        "device": torch.cuda.get_device_name(0),
        "library": sm.version(),
        "multi_library": mu.version(),
        "baseline_multi_library": base[0].smm_version().decode() if base else "this build (the call is not changed)",
        "index_stage": mu.INDEX_STAGE,
        "stream_bytes": stream_bytes,
        "ms": res,
        "GBps_out": {k: round(n / (v["median_ms"] * 1e6), 1) for k, v in res.items()},
        "c_max_below_a_min": res["c_index_then_indexed"]["max_ms"] < res["a_stream_order"]["min_ms"],
    }
    if args.long_streams:
        del cases
        lcases, lbytes = shape(args.long_streams)
        lres = alternate(torch, {k: lcases[k] for k in ("a_stream_order", "b_index", "c_index_then_indexed")},
                         max(args.reps // 4, 3), 1)
        report["e_long"] = {"workload": "the same bytes as %d streams of %d MiB" % (args.long_streams, nblk // args.long_streams // 16),
                            "stream_bytes": lbytes, "reps": max(args.reps // 4, 3), "ms": lres}
    if args.kernel_stats:
        report["kernel_stats"] = {"source": "rocprofv3 --kernel-trace --stats, a run of its own", "us": kernel_stats(args.kernel_stats)}
    line = json.dumps(report, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
