"""Rates of the Parquet page encoder's batched call against its floor, on the plain column chunks of
tests/golden/parquet_write/ (what pyarrow writes with compression="none") repeated to about `--mib`
MiB of input, in fast mode.

Two workloads, since the headers and not an argument decide whether a page's CRC is computed:

  crc     the chunks of v1.parquet, v2.parquet and bigpage.parquet: the headers of the first two carry a crc
  no_crc  the chunks of v1_nocrc.parquet and bigpage.parquet: none does

and for each, timed interleaved call by call in one process, each by a pair of HIP events around it on
the current stream, `--reps` times after `--warmup` untimed rounds (median, minimum and maximum in
milliseconds; the method of tools/parquet_rates.py):

  call    smqe_compress_chunks_device with the plan's three bounds
  floor   smm_compress_device alone over the same values sections, at the offsets a host walk found
          beforehand (not timed), into slots of their own: no page walk, no level bytes, no CRC, no pack

so the layer's own cost shows as a ratio.  No number is a gate.  Needs a GPU.

    python tools/parquet_write_rates.py --out profiles/parquet_write_rates.json
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
GOLDEN = os.path.join(ROOT, "tests", "golden", "parquet_write")
WORKLOADS = {"crc": ("v1.parquet", "v2.parquet", "bigpage.parquet"), "no_crc": ("v1_nocrc.parquet", "bigpage.parquet")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256, help="input bytes of each workload, about")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--mode", default="fast")
    ap.add_argument("--commit", default=None, help="the commit the numbers are taken at (default: git's HEAD)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import bench
    from framing_range_rates import timed
    from framing_rates import clocks
    from parquet_rates import commit
    if not torch.cuda.is_available():
        print("parquet_write_rates.py needs a GPU", file=sys.stderr)
        return 2
    sm = bench.load_package()
    pq = importlib.import_module("snappy_jl_amd.parquet")
    mu = importlib.import_module("snappy_jl_amd.multi")
    dev = torch.device("cuda", 0)
    clocks_before = clocks()
    with open(os.path.join(GOLDEN, "parquet_write_fixture.json")) as fh:
        record = json.load(fh)["files"]

    def i64(values):
        return torch.from_numpy(np.asarray(values, dtype=np.int64)).to(dev)

    def i32(values):
        return torch.from_numpy(np.asarray(values, dtype=np.int32)).to(dev)

    def zeros(k, dtype):
        return torch.zeros(max(k, 1), dtype=dtype, device=dev)

    calls, notes = [], {}
    for label, files in WORKLOADS.items():
        base = []
        for name in files:
            with open(os.path.join(GOLDEN, name), "rb") as fh:
                data = fh.read()
            base += [data[c["offset"]:c["offset"] + c["length"]] for c in record[name]["chunks"]]
        copies = max(1, (args.mib << 20) // sum(len(c) for c in base))
        chunks = base * copies
        k = len(chunks)
        rc, first, status, bound, pages, stage, frags = pq.compress_chunks_plan(base)
        assert rc == 0 and not status.any()
        pages, frags, stage = pages * copies, frags * copies, 32 + (stage - 32) * copies
        caps = bound.tolist() * copies
        # the chunks back to back, their outputs at multiples of 16
        in_off, out_off, pos, opos = [], [], 0, 0
        for c, cap in zip(chunks, caps):
            in_off.append(pos)
            pos += len(c)
            out_off.append(opos)
            opos += (cap + 15) // 16 * 16
        d_in = torch.from_numpy(np.frombuffer(b"".join(chunks), np.uint8).copy()).to(dev)
        d_out = torch.empty(opos, dtype=torch.uint8, device=dev)
        d_in_off, d_in_len, d_out_off, d_cap = i64(in_off), i64([len(c) for c in chunks]), i64(out_off), i64(caps)
        d_ol, d_st = zeros(k, torch.int64), zeros(k, torch.int32)

        # the floor's streams: every values section, where the host's encode walk found it
        tables = [pq.index_plain_column_chunk(c)[:2] for c in base] * copies
        sec_off, sec_len, slot_off, spos, with_crc, levels_bytes, stepped = [], [], [], 0, 0, 0, 0
        for ci, (s, a) in enumerate(tables):
            for p in range(s.nchunks):
                if int(a["type"][p]) not in (0, 2, 3):
                    stepped += 1
                    continue
                with_crc += int(a["flags"][p]) & pq.PAGE_HAS_CRC
                levels = int(a["levels"][p])
                levels_bytes += levels
                sec_off.append(in_off[ci] + int(a["hdr_off"][p]) + int(a["hdr_len"][p]) + levels)
                sec_len.append(int(a["usize"][p]) - levels)
                slot_off.append(spos)
                spos += (32 + sec_len[-1] + sec_len[-1] // 6 + 15) // 16 * 16
        ns = len(sec_off)
        d_so, d_sl, d_slot = i64(sec_off), i32(sec_len), i64(slot_off)
        d_floor_out = torch.empty(spos, dtype=torch.uint8, device=dev)
        d_sol, d_sst = zeros(ns, torch.int32), zeros(ns, torch.int32)

        def call(a=(d_in, d_in_off, d_in_len, pages, stage, frags, d_out, d_out_off, d_cap, d_ol, d_st)):
            pq.compress_column_chunks_device(*a, mode=args.mode)

        def floor(a=(d_in, d_so, d_sl, frags, d_floor_out, d_slot, d_sol, d_sst)):
            mu.compress_streams_device(*a, mode=args.mode)

        call()
        floor()
        torch.cuda.synchronize()
        assert not bool(d_st.any()) and not bool(d_sst.any())
        written = int(d_ol.sum().item())
        # what was written decodes, with CRC verification on, to the pages' plain bodies
        back = pq.uncompress_column_chunks([bytes(d_out[o:o + n].cpu().numpy()) for o, n in
                                            list(zip(out_off, d_ol.cpu().tolist()))[:len(base)]], verify_crc=True)
        assert sum(len(b) for b, _ in back) == sum(int(s.total_length) for s, _ in tables[:len(base)])
        calls += [call, floor]
        notes[label] = dict(chunks=k, pages=pages, with_crc=with_crc, sections=ns, stepped_over=stepped, bytes_in=pos, bytes_out=written,
                            level_bytes=levels_bytes, stage_bytes=stage, plan_fragments=frags, copies=copies, files=", ".join(files))

    t = timed(torch, calls, args.reps, args.warmup)
    report = {
        "method": "HIP events around each call on one stream; the alternatives of both workloads interleaved call by call; %d "
                  "warm-up rounds, %d timed; median, min, max" % (args.warmup, args.reps),
        "mode": args.mode,
        "commit": args.commit or commit(),
        "device": torch.cuda.get_device_name(0),
        "library": sm.version(),
        "multi_library": mu.version(),
        "parquet_library": pq.version(),
        "workloads": {},
        "clocks_before": clocks_before,
        "clocks_after": clocks(),
    }
    for i, label in enumerate(WORKLOADS):
        c, f, n = t[2 * i], t[2 * i + 1], notes[label]
        report["workloads"][label] = {
            "workload": "the column chunks of %(files)s, %(copies)d times: %(chunks)d chunks, %(pages)d pages (%(with_crc)d with a crc, "
                        "%(stepped_over)d stepped over), %(sections)d values sections, %(bytes_in)d bytes in, %(bytes_out)d bytes "
                        "out, %(level_bytes)d level bytes, %(stage_bytes)d bytes of stage, %(plan_fragments)d fragments" % n,
            "ms": {"call": c, "floor_smm_compress_device": f},
            "GBps_in": {"call": round(n["bytes_in"] / c["median_ms"] / 1e6, 1), "floor_smm_compress_device": round(n["bytes_in"] / f["median_ms"] / 1e6, 1)},
            "call_over_floor": round(c["median_ms"] / f["median_ms"], 3),
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
