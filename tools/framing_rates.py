"""Rates of the framing format's device calls against the raw batched calls of the same build, on
the headline workload's blocks (bench.py text_blocks: 10,000 x 64 KiB windows of the text files).

Each call is timed by a pair of HIP events around it on the current stream, `--reps` times after
`--warmup` untimed calls; the report gives the median, the minimum and the maximum (the spread) in
milliseconds, and the clocks rocm-smi shows when the timing ends.  Needs a GPU; nothing here falls
back to the CPU.

    python tools/framing_rates.py --out profiles/framing_rates.json
    python tools/framing_rates.py --only crc --reps 3          # a short run, e.g. under a counter pass
    python tools/framing_rates.py --pmc-dir DIR --out F.json    # add k_crc32c's LDS conflict share from
                                                                # a rocprofv3 --pmc SQ_LDS_BANK_CONFLICT
                                                                # SQ_LDS_IDX_ACTIVE pass into F.json
"""
import argparse
import csv
import glob
import importlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BLOCK = 65536


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=30).stdout
    except (OSError, subprocess.SubprocessError):
        return "not read"
    keep = [l.split(":", 1)[1].strip() for l in out.splitlines() if "sclk" in l or "mclk" in l]
    return "; ".join(keep) if keep else "not read"


def timed(torch, fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "reps": reps}


def lds_conflict_share(pmc_dir):
    """k_crc32c's SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE over the dispatches of a counter pass."""
    tot = {"SQ_LDS_BANK_CONFLICT": 0.0, "SQ_LDS_IDX_ACTIVE": 0.0}
    for f in glob.glob(os.path.join(pmc_dir, "**", "*counter_collection.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            if "k_crc32c" in row.get("Kernel_Name", "") and row["Counter_Name"] in tot:
                tot[row["Counter_Name"]] += float(row["Counter_Value"])
    if not tot["SQ_LDS_IDX_ACTIVE"]:
        return None
    return {"bank_conflict_cycles": tot["SQ_LDS_BANK_CONFLICT"], "lds_active_cycles": tot["SQ_LDS_IDX_ACTIVE"],
            "conflict_share": round(tot["SQ_LDS_BANK_CONFLICT"] / tot["SQ_LDS_IDX_ACTIVE"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["crc"], default=None)
    ap.add_argument("--pmc-dir", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    if args.pmc_dir:  # no device work: fold a counter pass into an existing report
        report = json.load(open(args.out))
        report["crc32c_lds"] = lds_conflict_share(args.pmc_dir) or "no k_crc32c rows in the counter pass"
        json.dump(report, open(args.out, "w"), indent=1)
        print(json.dumps(report["crc32c_lds"]))
        return 0

    import torch
    import bench
    if not torch.cuda.is_available():
        print("framing_rates.py needs a GPU", file=sys.stderr)
        return 2
    sm = bench.load_package()
    fr = importlib.import_module("snappy_jl_amd.framing")
    dev = torch.device("cuda", 0)
    nblk = args.blocks
    blocks = bench.text_blocks(nblk, 0x5EED)
    batch = bench.Batch(blocks, dev)
    n = nblk * BLOCK
    res = {}

    d_crc = torch.zeros(nblk, dtype=torch.int32, device=dev)
    res["crc32c_batch"] = timed(torch, lambda: fr.crc32c_batch_device(batch.d_in, batch.in_off, batch.in_len, d_crc,
                                                                        masked=True), args.reps, args.warmup)
    if args.only != "crc":
        res["raw_compress_batch_fast"] = timed(torch, lambda: batch.compress(sm, "fast"), args.reps, args.warmup)
        res["raw_uncompress_batch"] = timed(torch, lambda: batch.uncompress(sm), args.reps, args.warmup)

        d_framed = torch.empty(fr.max_framed_length(n), dtype=torch.uint8, device=dev)
        d_len = torch.zeros(1, dtype=torch.int64, device=dev)
        d_st = torch.zeros(1, dtype=torch.int32, device=dev)
        res["framed_compress_fast"] = timed(
            torch, lambda: fr.compress_framed_device(batch.d_in, d_framed, d_len, d_st, mode="fast"), args.reps, args.warmup)
        framed_len = int(d_len.item())
        assert int(d_st.item()) == 0

        arrays = fr.device_chunks(nblk)
        d_sum = torch.zeros(16, dtype=torch.uint8, device=dev)
        res["index_one_wave"] = timed(torch, lambda: fr.index_framed_device(d_framed, arrays, d_sum, n=framed_len),
                                      args.reps, args.warmup)
        s = fr.read_summary(d_sum)
        assert (s.status, s.nchunks, s.total_length) == (0, nblk, n)
        res["index_one_wave"]["us_per_chunk"] = round(1000 * res["index_one_wave"]["median_ms"] / nblk, 4)

        d_cs = torch.zeros(nblk, dtype=torch.int32, device=dev)
        batch.d_dec.fill_(0xAA)
        res["framed_uncompress_chunks"] = timed(
            torch, lambda: fr.uncompress_chunks_device(d_framed, arrays, nblk, batch.d_dec, d_cs, d_len, d_st),
            args.reps, args.warmup)
        assert int(d_st.item()) == 0 and int(d_len.item()) == n and bool(torch.equal(batch.d_dec, batch.d_in))

    report = {
        "workload": "%d x 64 KiB text blocks (bench.py text_blocks, seed 0x5EED), %d bytes" % (nblk, n),
        "method": "HIP events around each call on one stream; %d warm-ups, %d timed calls; median, min, max"
                  % (args.warmup, args.reps),
        "device": torch.cuda.get_device_name(0),
        # (not in a short --only run: that is the one made under a counter pass, whose profiler
        # library would load into the rocm-smi child as well)
        "clocks_after": clocks() if args.only is None else "not read",
        "library": sm.version(),
        "framing_library": fr.version(),
        "ms": res,
        "GBps_in": {k: round(n / (v["median_ms"] * 1e6), 1) for k, v in res.items() if k != "index_one_wave"},
    }
    if args.only != "crc":
        report["framed_bytes"] = framed_len
        report["crc_over_raw_uncompress"] = round(res["crc32c_batch"]["median_ms"] / res["raw_uncompress_batch"]["median_ms"], 3)
        report["framed_over_raw_compress"] = round(
            res["framed_compress_fast"]["median_ms"] / res["raw_compress_batch_fast"]["median_ms"], 3)
        report["framed_over_raw_uncompress"] = round(
            res["framed_uncompress_chunks"]["median_ms"] / res["raw_uncompress_batch"]["median_ms"], 3)
    line = json.dumps(report, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
