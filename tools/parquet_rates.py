"""Rates of the Parquet page library's batched decode against its floor, on the column chunks of
tests/golden/parquet/ (v1.parquet, v2.parquet, bigpage.parquet: the page shapes pyarrow writes)
repeated to about `--mib` MiB of decoded bytes.

The alternatives are timed interleaved call by call in one process, each by a pair of HIP events
around it on the current stream, `--reps` times after `--warmup` untimed rounds (median, minimum and
maximum in milliseconds; the method of tools/orc_rates.py):

  verify     smq_uncompress_chunks_device with verify_crc (max_fragments: the plan's)
  no_verify  the same without the CRC pass
  floor      smm_uncompress_device alone over the same compressed sections, with the index
             smm_index_device built for them beforehand (not timed): no page walk, no copies of level
             bytes, no CRC

so the layer's own cost shows as a ratio.  No number is a gate.  Needs a GPU.

    python tools/parquet_rates.py --out profiles/parquet_rates.json
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
GOLDEN = os.path.join(ROOT, "tests", "golden", "parquet")
FILES = ("v1.parquet", "v2.parquet", "bigpage.parquet")


def commit():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              timeout=30).stdout.strip() or "not read"
    except (OSError, subprocess.SubprocessError):
        return "not read"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256, help="decoded bytes of the workload, about")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--commit", default=None, help="the commit the numbers are taken at (default: git's HEAD)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import bench
    from framing_range_rates import timed
    from framing_rates import clocks
    if not torch.cuda.is_available():
        print("parquet_rates.py needs a GPU", file=sys.stderr)
        return 2
    sm = bench.load_package()
    pq = importlib.import_module("snappy_jl_amd.parquet")
    mu = importlib.import_module("snappy_jl_amd.multi")
    dev = torch.device("cuda", 0)
    clocks_before = clocks()

    with open(os.path.join(GOLDEN, "parquet_fixture.json")) as fh:
        record = json.load(fh)["files"]
    base = []
    for name in FILES:
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            data = fh.read()
        base += [data[c["offset"]:c["offset"] + c["length"]] for c in record[name]["chunks"]]
    once = sum(pq.index_column_chunk(c)[0].total_length for c in base)
    copies = max(1, (args.mib << 20) // once)
    chunks = base * copies

    def i64(values):
        return torch.from_numpy(np.asarray(values, dtype=np.int64)).to(dev)

    def i32(values):
        return torch.from_numpy(np.asarray(values, dtype=np.int32)).to(dev)

    def zeros(k, dtype):
        return torch.zeros(max(k, 1), dtype=dtype, device=dev)

    # the chunks back to back, their outputs at multiples of 16
    in_off, out_off, caps, pos, opos = [], [], [], 0, 0
    tables = [pq.index_column_chunk(c) for c in base] * copies
    for c, (s, _) in zip(chunks, tables):
        in_off.append(pos)
        pos += len(c)
        out_off.append(opos)
        caps.append(int(s.total_length))
        opos += (caps[-1] + 15) // 16 * 16
    d_in = torch.from_numpy(np.frombuffer(b"".join(chunks), np.uint8).copy()).to(dev)
    d_out = torch.empty(opos, dtype=torch.uint8, device=dev)
    k = len(chunks)
    rc, first, need, status, pages, frags = pq.chunks_plan(base, out_cap=caps[:len(base)])
    assert rc == 0 and not status.any()
    pages, frags = pages * copies, frags * copies
    d_in_off, d_in_len, d_out_off, d_cap = i64(in_off), i64([len(c) for c in chunks]), i64(out_off), i64(caps)
    d_ol, d_st = zeros(k, torch.int64), zeros(k, torch.int32)

    # the floor's streams: every compressed section, where the walk found it
    sec_off, sec_len, sec_out, sec_cap, with_crc, copied = [], [], [], [], 0, 0
    for ci, (s, a) in enumerate(tables):
        for p in range(s.nchunks):
            with_crc += int(a["flags"][p]) & pq.PAGE_HAS_CRC
            if int(a["flags"][p]) & pq.PAGE_COMPRESSED:
                levels = int(a["levels"][p])
                sec_off.append(in_off[ci] + int(a["hdr_off"][p]) + int(a["hdr_len"][p]) + levels)
                sec_len.append(int(a["body_len"][p]) - levels)
                sec_out.append(out_off[ci] + int(a["out_off"][p]) + levels)
                sec_cap.append(int(a["usize"][p]) - levels)
                copied += levels
            elif int(a["type"][p]) in (0, 2, 3):
                copied += int(a["body_len"][p])
    ns = len(sec_off)
    d_so, d_sl, d_sout, d_sc = i64(sec_off), i32(sec_len), i64(sec_out), i32(sec_cap)
    d_ff, d_fp, d_built = zeros(ns + 1, torch.int32), zeros(frags, torch.int32), zeros(ns, torch.uint8)
    d_ist, d_sol, d_sst = zeros(ns, torch.int32), zeros(ns, torch.int32), zeros(ns, torch.int32)
    mu.index_streams_device(d_in, d_so, d_sl, frags, d_ff, d_fp, d_built, d_ist, d_out_cap=d_sc)
    torch.cuda.synchronize()
    assert not bool(d_ist.any())

    def verify():
        pq.uncompress_column_chunks_device(d_in, d_in_off, d_in_len, pages, frags, d_out, d_out_off, d_cap, d_ol, d_st,
                                           verify_crc=True)

    def no_verify():
        pq.uncompress_column_chunks_device(d_in, d_in_off, d_in_len, pages, frags, d_out, d_out_off, d_cap, d_ol, d_st,
                                           verify_crc=False)

    def floor():
        mu.uncompress_streams_device(d_in, d_so, d_sl, frags, d_out, d_sout, d_sc, d_sol, d_sst, d_ff, d_fp)

    verify()
    torch.cuda.synchronize()
    assert not bool(d_st.any()) and d_ol.cpu().tolist() == caps
    want = d_out.clone()
    for fn in (no_verify, floor):
        fn()
        torch.cuda.synchronize()
    assert not bool(d_st.any()) and not bool(d_sst.any())
    t = timed(torch, [verify, no_verify, floor], args.reps, args.warmup)
    assert not bool(d_st.any()) and bool(torch.equal(d_out, want))
    decoded = sum(caps)
    report = {
        "workload": "the %d column chunks of %s, %d times: %d chunks, %d pages (%d with a crc), %d compressed sections, "
                    "%d bytes in, %d bytes decoded, %d of them copied as stored" %
                    (len(base), ", ".join(FILES), copies, k, pages, with_crc, ns, pos, decoded, copied),
        "method": "HIP events around each call on one stream; the alternatives interleaved call by call; %d warm-up "
                  "rounds, %d timed; median, min, max" % (args.warmup, args.reps),
        "commit": args.commit or commit(),
        "device": torch.cuda.get_device_name(0),
        "library": sm.version(),
        "multi_library": mu.version(),
        "parquet_library": pq.version(),
        "plan_fragments": frags,
        "ms": {"verify": t[0], "no_verify": t[1], "floor_smm_uncompress_device": t[2]},
        "GBps_decoded": {"verify": round(decoded / t[0]["median_ms"] / 1e6, 1), "no_verify": round(decoded / t[1]["median_ms"] / 1e6, 1),
                         "floor_smm_uncompress_device": round(decoded / t[2]["median_ms"] / 1e6, 1)},
        "verify_over_floor": round(t[0]["median_ms"] / t[2]["median_ms"], 3),
        "no_verify_over_floor": round(t[1]["median_ms"] / t[2]["median_ms"], 3),
        "clocks_before": clocks_before,
        "clocks_after": clocks(),
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
