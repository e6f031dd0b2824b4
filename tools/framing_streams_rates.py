"""Rates of the framing library's batched stream calls against a loop of the single-stream calls,
on bench.py's text_blocks (10,000 x 64 KiB windows of the text files, seed 0x5EED) cut into

  a_10000x1    10,000 streams of one 64 KiB block each
  b_100x100    100 streams of 100 blocks each

For each workload and each direction three things are timed, interleaved call by call in one
process, each by a pair of HIP events around it on the current stream, `--reps` times after
`--warmup` untimed rounds (median, minimum and maximum in milliseconds; the method of
tools/framing_range_rates.py):

  batch   smf_compress_streams_device / smf_uncompress_streams_device: one call for all streams
  loop    smf_compress_device / smf_uncompress_device, stream after stream (the events surround the
          whole loop): the only way to do the job without the batched calls
  floor   the same blocks as ONE stream: smf_compress_device, and smf_uncompress_chunks_device with
          a ready index -- no walk and no per-stream work at all

The batch call's median has to be below the loop's in both directions on both workloads; the ratio
to the floor is recorded without a threshold.  With --parent-lib, a same-box A/B of
smf_compress_device, smf_uncompress_chunks_device and smf_uncompress_device between a build of the
parent commit and this build, the two interleaved call by call: the medians may differ by no more
than the parent's own min-max spread.  Needs a GPU.

    python tools/framing_streams_rates.py --out profiles/framing_streams_rates.json [--parent-lib PATH]
"""
import argparse
import ctypes
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
BLOCK = 65536
MODE_FAST = 1


class Build:
    """The single-stream device calls of one build of the framing library, through one ctypes path
    for both sides of the A/B and for the loops."""

    def __init__(self, path, fr):
        vp, u32, u64, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int32
        self.lib = L = ctypes.CDLL(path)
        L.smf_ctx_create.restype = vp
        L.smf_ctx_create.argtypes = [ctypes.c_int]
        L.smf_version.restype = ctypes.c_char_p
        L.smf_compress_device.restype = i32
        L.smf_compress_device.argtypes = [vp, vp, u64, vp, u64, vp, vp, ctypes.c_int, vp]
        L.smf_uncompress_chunks_device.restype = i32
        L.smf_uncompress_chunks_device.argtypes = [vp, vp, ctypes.POINTER(fr.Chunks), u32, vp, u64, vp, vp, vp, vp]
        L.smf_uncompress_device.restype = i32
        L.smf_uncompress_device.argtypes = [vp, vp, u64, vp, u64, vp, vp, vp]
        self.ctx = L.smf_ctx_create(0)
        assert self.ctx
        self.version = L.smf_version().decode()

    def compress(self, p_in, n, p_out, cap, p_len, p_st, stream):
        assert self.lib.smf_compress_device(self.ctx, p_in, n, p_out, cap, p_len, p_st, MODE_FAST, stream) == 0

    def uncompress(self, p_in, n, p_out, cap, p_len, p_st, stream):
        assert self.lib.smf_uncompress_device(self.ctx, p_in, n, p_out, cap, p_len, p_st, stream) == 0

    def uncompress_chunks(self, p_in, ch, nchunks, p_out, cap, p_cs, p_len, p_st, stream):
        assert self.lib.smf_uncompress_chunks_device(self.ctx, p_in, ctypes.byref(ch), nchunks, p_out, cap, p_cs, p_len,
                                                     p_st, stream) == 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent-lib", default=None, help="libsnappy_mi355x_framing.so built from the parent commit")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import bench
    from framing_range_rates import timed
    from framing_rates import clocks
    if not torch.cuda.is_available():
        print("framing_streams_rates.py needs a GPU", file=sys.stderr)
        return 2
    sm = bench.load_package()
    fr = importlib.import_module("snappy_jl_amd.framing")
    dev = torch.device("cuda", 0)
    nblk = args.blocks
    d_in = torch.from_numpy(bench.text_blocks(nblk, 0x5EED).reshape(-1)).to(dev)
    n = nblk * BLOCK
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    this = Build(fr.LIB_PATH, fr)

    def i64(values):
        return torch.from_numpy(np.asarray(values, dtype=np.int64)).to(dev)

    def zeros(k, dtype):
        return torch.zeros(k, dtype=dtype, device=dev)

    # ---- the floor: the same blocks as one stream, and its ready index
    d_one = torch.empty(fr.max_framed_length(n), dtype=torch.uint8, device=dev)
    d_len1, d_st1 = zeros(1, torch.int64), zeros(1, torch.int32)
    arrays, d_coff, d_nc = fr.device_chunks(nblk), zeros(nblk + 1, torch.int64), zeros(1, torch.int32)
    fr.compress_framed_indexed_device(d_in, d_one, d_len1, d_st1, arrays, d_coff, d_nc, mode="fast")
    one_len = int(d_len1.item())
    assert int(d_st1.item()) == 0 and int(d_nc.item()) == nblk
    ch = fr.Chunks(*(arrays[k].data_ptr() for k in ("type", "pay_off", "pay_len", "crc", "ulen")))
    d_cs = zeros(nblk, torch.int32)
    d_dec = torch.empty(n, dtype=torch.uint8, device=dev)

    def floor_compress():
        this.compress(d_in.data_ptr(), n, d_one.data_ptr(), d_one.numel(), d_len1.data_ptr(), d_st1.data_ptr(), stream)

    def floor_decode():
        this.uncompress_chunks(d_one.data_ptr(), ch, nblk, d_dec.data_ptr(), n, d_cs.data_ptr(), d_len1.data_ptr(),
                               d_st1.data_ptr(), stream)

    res = {}

    def workload(name, nstreams, per):
        assert nstreams * per == nblk
        size = per * BLOCK
        room = (fr.max_framed_length(size) + 15) // 16 * 16
        in_off, out_off = [s * size for s in range(nstreams)], [s * room for s in range(nstreams)]
        d_in_off, d_in_len, d_f_off = i64(in_off), i64([size] * nstreams), i64(out_off)
        d_framed = torch.empty(nstreams * room, dtype=torch.uint8, device=dev)   # the batch call's
        d_framed2 = torch.empty(nstreams * room, dtype=torch.uint8, device=dev)  # the loop's
        d_flen, d_fst = zeros(nstreams, torch.int64), zeros(nstreams, torch.int32)
        d_flen2, d_fst2 = zeros(nstreams, torch.int64), zeros(nstreams, torch.int32)

        def batch_compress():
            fr.compress_framed_streams_device(d_in, d_in_off, d_in_len, nblk, d_framed, d_f_off, d_flen, d_fst, mode="fast")

        cargs = [(d_in.data_ptr() + in_off[s], size, d_framed2.data_ptr() + out_off[s], room, d_flen2.data_ptr() + 8 * s,
                  d_fst2.data_ptr() + 4 * s, stream) for s in range(nstreams)]

        def loop_compress():
            for a in cargs:
                this.compress(*a)

        c = timed(torch, [batch_compress, loop_compress, floor_compress], args.reps, args.warmup)
        flen = d_flen.cpu().tolist()
        assert not bool(d_fst.any()) and not bool(d_fst2.any()) and flen == d_flen2.cpu().tolist()
        for s in sorted({0, nstreams // 2, nstreams - 1}):
            o = out_off[s]
            assert bool(torch.equal(d_framed[o:o + flen[s]], d_framed2[o:o + flen[s]])), (name, s)

        # decode: the streams the batch call framed, where they lie
        d_out_off, d_cap = d_in_off, d_in_len
        d_ol, d_ds = zeros(nstreams, torch.int64), zeros(nstreams, torch.int32)
        d_ol2, d_ds2 = zeros(nstreams, torch.int64), zeros(nstreams, torch.int32)
        d_dec2 = torch.empty(n, dtype=torch.uint8, device=dev)

        def batch_decode():
            fr.uncompress_framed_streams_device(d_framed, d_f_off, d_flen, nblk, d_dec, d_out_off, d_cap, d_ol, d_ds)

        dargs = [(d_framed.data_ptr() + out_off[s], flen[s], d_dec2.data_ptr() + in_off[s], size, d_ol2.data_ptr() + 8 * s,
                  d_ds2.data_ptr() + 4 * s, stream) for s in range(nstreams)]

        def loop_decode():
            for a in dargs:
                this.uncompress(*a)

        d_dec.fill_(0xAA)
        d_dec2.fill_(0xAA)
        batch_decode()
        assert not bool(d_ds.any()) and bool((d_ol == size).all()) and bool(torch.equal(d_dec, d_in)), name
        d = timed(torch, [batch_decode, loop_decode, floor_decode], args.reps, args.warmup)
        assert not bool(d_ds.any()) and not bool(d_ds2.any()) and bool(torch.equal(d_dec2, d_in)), name
        assert int(d_st1.item()) == 0 and bool(torch.equal(d_dec, d_in)), name
        res[name] = {
            "streams": nstreams, "blocks_per_stream": per,
            "compress": {"batch": c[0], "loop": c[1], "floor_one_stream": c[2],
                         "batch_below_loop": bool(c[0]["median_ms"] < c[1]["median_ms"]),
                         "batch_over_floor": round(c[0]["median_ms"] / c[2]["median_ms"], 3)},
            "decode": {"batch": d[0], "loop": d[1], "floor_chunks_with_index": d[2],
                       "batch_below_loop": bool(d[0]["median_ms"] < d[1]["median_ms"]),
                       "batch_over_floor": round(d[0]["median_ms"] / d[2]["median_ms"], 3)},
        }
        print(name, json.dumps(res[name]), flush=True)

    workload("a_10000x1", nblk, 1)
    workload("b_100x100", nblk // 100, 100)

    report = {
        "workload": "%d x 64 KiB text blocks (bench.py text_blocks, seed 0x5EED), %d bytes, fast mode" % (nblk, n),
        "method": "HIP events around each call (around the whole loop of single-stream calls) on one stream; the "
                  "alternatives interleaved call by call; %d warm-up rounds, %d timed; median, min, max"
                  % (args.warmup, args.reps),
        "device": torch.cuda.get_device_name(0),
        "library": sm.version(),
        "framing_library": fr.version(),
        "ms": res,
        "conditions_met": bool(all(w[d]["batch_below_loop"] for w in res.values() for d in ("compress", "decode"))),
    }

    # ---- the existing calls, parent build against this build, interleaved
    if args.parent_lib:
        builds = [Build(args.parent_lib, fr), this]
        d_ol, d_ds = zeros(1, torch.int64), zeros(1, torch.int32)
        ab = {}
        ab["compress"] = timed(torch, [lambda b=b: b.compress(d_in.data_ptr(), n, d_one.data_ptr(), d_one.numel(),
                                                               d_len1.data_ptr(), d_st1.data_ptr(), stream)
                                       for b in builds], args.reps, args.warmup)
        assert int(d_st1.item()) == 0 and int(d_len1.item()) == one_len
        ab["uncompress_chunks"] = timed(
            torch, [lambda b=b: b.uncompress_chunks(d_one.data_ptr(), ch, nblk, d_dec.data_ptr(), n, d_cs.data_ptr(),
                                                    d_ol.data_ptr(), d_ds.data_ptr(), stream) for b in builds],
            args.reps, args.warmup)
        assert int(d_ds.item()) == 0 and bool(torch.equal(d_dec, d_in))
        d_dec.fill_(0xAA)
        ab["uncompress"] = timed(torch, [lambda b=b: b.uncompress(d_one.data_ptr(), one_len, d_dec.data_ptr(), n,
                                                                   d_ol.data_ptr(), d_ds.data_ptr(), stream)
                                         for b in builds], args.reps, args.warmup)
        assert int(d_ds.item()) == 0 and int(d_ol.item()) == n and bool(torch.equal(d_dec, d_in))
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
