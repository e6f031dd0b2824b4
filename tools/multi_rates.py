"""Rates of the multi-stream library's device calls against the raw batched calls of the same build
on the same bytes: 640 streams of 1 MiB, each 16 consecutive 64 KiB windows of the headline text
(bench.py text_blocks), against those 10,240 windows as independent blocks.

Each call is timed by a pair of HIP events around it on the current stream, `--reps` times after
`--warmup` untimed calls; the report gives the median, the minimum and the maximum (the spread) in
milliseconds, and the clocks rocm-smi shows when the timing ends.  The raw fragment calls on the same
fragments are timed too: what the multi-stream call takes beyond them is its plan, pack and reduce
kernels and the masked raw call over the streams.  Needs a GPU; nothing here falls back to the CPU.

    python tools/multi_rates.py --out profiles/multi_rates.json
    python tools/multi_rates.py --streams 64 --reps 3      # a short run, e.g. under a kernel trace
"""
import argparse
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
BLOCK = 65536
PER_STREAM = 16  # 64 KiB windows per stream: 1 MiB


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=30).stdout
    except (OSError, subprocess.SubprocessError):
        return "not read"
    keep = [l.split(":", 1)[1].strip() for l in out.splitlines() if "sclk" in l or "mclk" in l]
    return "; ".join(keep) if keep else "not read"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=640)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import bench
    from framing_rates import timed
    if not torch.cuda.is_available():
        print("multi_rates.py needs a GPU", file=sys.stderr)
        return 2
    sm = bench.load_package()
    mu = importlib.import_module("snappy_jl_amd.multi")
    dev = torch.device("cuda", 0)
    ns, nblk = args.streams, args.streams * PER_STREAM
    slen = PER_STREAM * BLOCK
    n = nblk * BLOCK
    batch = bench.Batch(bench.text_blocks(nblk, 0x5EED), dev)  # the blocks; the streams are the same bytes
    res = {}

    def i64(a):
        return torch.from_numpy(np.asarray(a, dtype=np.int64)).to(dev)

    def i32(a):
        return torch.from_numpy(np.asarray(a, dtype=np.int64).astype(np.uint32).view(np.int32)).to(dev)

    # the streams: 1 MiB inputs back to back, output slots of sm_max_compressed_length(1 MiB) rounded up to 256
    room = (32 + slen + slen // 6 + 255) // 256 * 256
    s_in_off, s_in_len = i64(np.arange(ns) * slen), i32(np.full(ns, slen))
    s_out_off = i64(np.arange(ns) * room)
    d_streams = torch.empty(ns * room, dtype=torch.uint8, device=dev)
    s_out_len = torch.zeros(ns, dtype=torch.int32, device=dev)
    s_status = torch.full((ns,), -1, dtype=torch.int32, device=dev)
    d_first = torch.zeros(ns + 1, dtype=torch.int32, device=dev)
    d_pos = torch.zeros(nblk, dtype=torch.int32, device=dev)
    s_cap = i32(np.full(ns, slen))
    s_dec_len = torch.zeros(ns, dtype=torch.int32, device=dev)

    # (a) compress
    res["raw_compress_batch_fast"] = timed(torch, lambda: batch.compress(sm, "fast"), args.reps, args.warmup)
    res["raw_compress_fragments_fast"] = timed(
        torch, lambda: sm.compress_fragments_device(batch.d_in, batch.in_off, batch.in_len, batch.d_comp, batch.comp_off,
                                                    batch.comp_len, 2 * BLOCK, mode="fast"), args.reps, args.warmup)
    res["multi_compress_fast"] = timed(
        torch, lambda: mu.compress_streams_device(batch.d_in, s_in_off, s_in_len, nblk, d_streams, s_out_off, s_out_len,
                                                  s_status, d_first, d_pos, mode="fast"), args.reps, args.warmup)
    assert int(s_status.abs().sum()) == 0
    stream_bytes = int(s_out_len.to(torch.int64).sum())
    assert d_first.cpu().tolist() == list(range(0, nblk + 1, PER_STREAM))

    # the same fragments for the raw fragment decoder: where the index says they are
    pos = d_pos.cpu().numpy().astype(np.int64).reshape(ns, PER_STREAM)
    lens = s_out_len.cpu().numpy().astype(np.int64)
    ends = np.concatenate([pos[:, 1:], lens[:, None]], axis=1)
    f_in_off = i64((pos + np.arange(ns)[:, None] * room).reshape(-1))
    f_in_len = i32((ends - pos).reshape(-1))
    f_len = torch.zeros(nblk, dtype=torch.int32, device=dev)
    f_st = torch.zeros(nblk, dtype=torch.int32, device=dev)

    # (b), (c) uncompress
    batch.compress(sm, "fast")
    res["raw_uncompress_batch"] = timed(torch, lambda: batch.uncompress(sm), args.reps, args.warmup)
    res["raw_uncompress_fragments"] = timed(
        torch, lambda: sm.uncompress_fragments_device(d_streams, f_in_off, f_in_len, batch.d_dec, batch.in_off,
                                                      batch.in_len, f_len, f_st), args.reps, args.warmup)
    assert int(f_st.abs().sum()) == 0
    batch.d_dec.fill_(0xAA)
    res["multi_uncompress_indexed"] = timed(
        torch, lambda: mu.uncompress_streams_device(d_streams, s_out_off, s_out_len, nblk, batch.d_dec, s_in_off, s_cap,
                                                    s_dec_len, s_status, d_first, d_pos), args.reps, args.warmup)
    assert int(s_status.abs().sum()) == 0 and bool(torch.equal(batch.d_dec, batch.d_in)) and mu.last_indexed(0) == ns
    batch.d_dec.fill_(0xAA)
    res["multi_uncompress_stream_order"] = timed(
        torch, lambda: mu.uncompress_streams_device(d_streams, s_out_off, s_out_len, 0, batch.d_dec, s_in_off, s_cap,
                                                    s_dec_len, s_status), max(args.reps // 4, 3), 1)
    assert int(s_status.abs().sum()) == 0 and bool(torch.equal(batch.d_dec, batch.d_in)) and mu.last_indexed(0) == 0

    med = {k: v["median_ms"] for k, v in res.items()}
    report = {
        "workload": "%d streams of 1 MiB = %d x 64 KiB text windows (bench.py text_blocks, seed 0x5EED), %d bytes; "
                    "the raw calls take the same windows as %d blocks" % (ns, nblk, n, nblk),
        "method": "HIP events around each call on one stream; %d warm-ups, %d timed calls (stream order: %d after 1); "
                  "median, min, max" % (args.warmup, args.reps, max(args.reps // 4, 3)),
        "device": torch.cuda.get_device_name(0),
        "clocks_after": clocks(),
        "library": sm.version(),
        "multi_library": mu.version(),
        "stream_bytes": stream_bytes,
        "scratch_bytes": mu.scratch_bytes(ns, nblk),
        "ms": res,
        "GBps_in": {k: round(n / (v * 1e6), 1) for k, v in med.items()},
        "a_multi_over_raw_batch_compress": round(med["multi_compress_fast"] / med["raw_compress_batch_fast"], 3),
        "a_compress_extra_ms_over_raw_fragments": round(med["multi_compress_fast"] - med["raw_compress_fragments_fast"], 4),
        "b_stream_order_over_indexed": round(med["multi_uncompress_stream_order"] / med["multi_uncompress_indexed"], 2),
        "c_indexed_over_raw_batch_uncompress": round(med["multi_uncompress_indexed"] / med["raw_uncompress_batch"], 3),
        "c_uncompress_extra_ms_over_raw_fragments": round(
            med["multi_uncompress_indexed"] - med["raw_uncompress_fragments"], 4),
    }
    line = json.dumps(report, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
