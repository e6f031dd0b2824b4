"""Rates of the ORC library's batched calls against their floors, at block_size 262144, on

  text_100     bench.py's text_blocks (10,000 x 64 KiB, seed 0x5EED) as 100 streams of 25 pieces each
  text_2500    the same bytes as 2,500 streams of one piece (one chunk) each
  random_100   as many random bytes as 100 streams: every chunk is stored

For each workload and each direction the alternatives are timed interleaved call by call in one
process, each by a pair of HIP events around it on the current stream, `--reps` times after
`--warmup` untimed rounds (median, minimum and maximum in milliseconds; the method of
tools/blocks_rates.py):

  batch   smo_compress_streams_device / smo_uncompress_streams_device (max_fragments: the plan's)
  batch0  the decode with max_fragments = 0 (no index is built)
  floor   smm_compress_device / smm_uncompress_device over the same 262,144-byte pieces with no
          container: no walk, no choice, no pack; the raw streams lie in slots at multiples of 256
          (decode: with the index smm_compress_device handed out)
  memcpy  random_100 only: one device-to-device hipMemcpyAsync of the same number of bytes

No number is a gate.  Needs a GPU.

    python tools/orc_rates.py --out profiles/orc_rates.json
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
BLOCK_SIZE = 262144
PITCH = (32 + BLOCK_SIZE + BLOCK_SIZE // 6 + 255) // 256 * 256  # a piece's raw stream: its bound, rounded up to 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=10000, help="64 KiB blocks of input (a multiple of 400)")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import bench
    from framing_range_rates import timed
    from framing_rates import clocks
    if not torch.cuda.is_available():
        print("orc_rates.py needs a GPU", file=sys.stderr)
        return 2
    sm = bench.load_package()
    orc = importlib.import_module("snappy_jl_amd.orc")
    mu = importlib.import_module("snappy_jl_amd.multi")
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    dev = torch.device("cuda", 0)
    n = args.blocks * BLOCK
    npieces = n // BLOCK_SIZE
    assert args.blocks % 400 == 0 and npieces * BLOCK_SIZE == n
    frags = npieces * (BLOCK_SIZE // BLOCK)
    clocks_before = clocks()

    def i64(values):
        return torch.from_numpy(np.asarray(values, dtype=np.int64)).to(dev)

    def i32(values):
        return torch.from_numpy(np.asarray(values, dtype=np.int32)).to(dev)

    def zeros(k, dtype):
        return torch.zeros(k, dtype=dtype, device=dev)

    # what every workload shares: the pieces' places, the floor's slots and index, the decoded bytes
    p_off, p_len = i64([p * BLOCK_SIZE for p in range(npieces)]), i32([BLOCK_SIZE] * npieces)
    s_off = i64([p * PITCH for p in range(npieces)])
    d_slots = torch.empty(npieces * PITCH, dtype=torch.uint8, device=dev)
    d_clen, d_cst = zeros(npieces, torch.int32), zeros(npieces, torch.int32)
    d_ff, d_fp = zeros(npieces + 1, torch.int32), zeros(frags, torch.int32)
    d_dec = torch.empty(n, dtype=torch.uint8, device=dev)
    d_dlen, d_dst = zeros(npieces, torch.int32), zeros(npieces, torch.int32)
    res = {}

    def workload(name, d_in, nstreams, all_stored):
        per = npieces // nstreams
        assert per * nstreams == npieces
        size = per * BLOCK_SIZE
        room = (orc.max_length(size, BLOCK_SIZE) + 15) // 16 * 16
        in_off, out_off = [s * size for s in range(nstreams)], [s * room for s in range(nstreams)]
        d_in_off, d_in_len, d_o_off = i64(in_off), i64([size] * nstreams), i64(out_off)
        d_packed = torch.empty(nstreams * room, dtype=torch.uint8, device=dev)
        d_plen, d_pst = zeros(nstreams, torch.int64), zeros(nstreams, torch.int32)
        d_ol, d_ds = zeros(nstreams, torch.int64), zeros(nstreams, torch.int32)

        def floor_compress():
            mu.compress_streams_device(d_in, p_off, p_len, frags, d_slots, s_off, d_clen, d_cst, d_ff, d_fp, mode="fast")

        def floor_decode():
            mu.uncompress_streams_device(d_slots, s_off, d_clen, frags, d_dec, p_off, p_len, d_dlen, d_dst, d_ff, d_fp)

        def batch_compress():
            orc.compress_orc_streams_device(BLOCK_SIZE, d_in, d_in_off, d_in_len, npieces, d_packed, d_o_off, d_plen, d_pst,
                                            mode="fast")

        def batch_decode(max_fragments=None):
            orc.uncompress_orc_streams_device(BLOCK_SIZE, d_packed, d_o_off, d_plen, npieces,
                                              plan_frags if max_fragments is None else max_fragments, d_dec, d_in_off,
                                              d_in_len, d_ol, d_ds)

        def memcpy():
            st = hip.hipMemcpyAsync(d_dec.data_ptr(), d_in.data_ptr(), n, 3, torch.cuda.current_stream().cuda_stream)
            assert st == 0

        floor_compress()
        d_dec.fill_(0xAA)
        floor_decode()
        assert not bool(d_cst.any()) and not bool(d_dst.any()) and bool(torch.equal(d_dec, d_in)), name
        batch_compress()
        assert not bool(d_pst.any()), name
        # the chunks as the host walk sees them: the plan's fragment bound, and how many are stored
        packed, plen = d_packed.cpu().numpy(), d_plen.cpu().tolist()
        stored = chunks = plan_frags = 0
        for s in range(nstreams):
            stream = packed[out_off[s]:out_off[s] + plen[s]]
            summary, arrays = orc.index_chunks(stream, BLOCK_SIZE)
            assert (summary.status, summary.nchunks, summary.total_length) == (0, per, size), name
            chunks += summary.nchunks
            stored += int(arrays["original"].sum())
            plan_frags += int(sum(-(-int(u) // BLOCK) for u, o in zip(arrays["ulen"], arrays["original"]) if not o))
        assert stored == (chunks if all_stored else 0), (name, stored, chunks)
        for m in (None, 0):
            d_dec.fill_(0xAA)
            batch_decode(m)
            assert not bool(d_ds.any()) and bool((d_ol == size).all()) and bool(torch.equal(d_dec, d_in)), (name, m)
        c = timed(torch, [batch_compress, floor_compress], args.reps, args.warmup)
        fns = [batch_decode, lambda: batch_decode(0), floor_decode] + ([memcpy] if all_stored else [])
        d = timed(torch, fns, args.reps, args.warmup)
        assert not bool(d_pst.any()) and not bool(d_ds.any()) and not bool(d_dst.any()) and bool(torch.equal(d_dec, d_in)), name
        res[name] = {
            "streams": nstreams, "pieces_per_stream": per, "chunks": chunks, "stored_chunks": stored,
            "packed_bytes": int(sum(plen)), "plan_fragments": plan_frags,
            "compress": {"batch": c[0], "floor_no_container": c[1],
                         "batch_over_floor": round(c[0]["median_ms"] / c[1]["median_ms"], 3)},
            "decode": {"batch": d[0], "batch_max_fragments_0": d[1], "floor_no_container": d[2],
                       "batch_over_floor": round(d[0]["median_ms"] / d[2]["median_ms"], 3),
                       "batch0_over_floor": round(d[1]["median_ms"] / d[2]["median_ms"], 3)},
        }
        if all_stored:
            res[name]["decode"].update({
                "memcpy_device_to_device": d[3],
                "batch0_over_memcpy": round(d[1]["median_ms"] / d[3]["median_ms"], 3),
                "batch0_GBps_of_output": round(n / d[1]["median_ms"] / 1e6, 1),
                "memcpy_GBps": round(n / d[3]["median_ms"] / 1e6, 1)})
        print(name, json.dumps(res[name]), flush=True)

    d_text = torch.from_numpy(bench.text_blocks(args.blocks, 0x5EED).reshape(-1)).to(dev)
    workload("text_100", d_text, 100, False)
    workload("text_2500", d_text, npieces, False)
    del d_text
    d_rand = torch.from_numpy(np.random.default_rng(0x5EED).integers(0, 256, n, dtype=np.uint8)).to(dev)
    workload("random_100", d_rand, 100, True)

    report = {
        "workload": "%d bytes at block_size %d (%d pieces), fast mode; text: bench.py text_blocks, seed 0x5EED" %
                    (n, BLOCK_SIZE, npieces),
        "method": "HIP events around each call on one stream; the alternatives interleaved call by call; %d warm-up "
                  "rounds, %d timed; median, min, max" % (args.warmup, args.reps),
        "device": torch.cuda.get_device_name(0),
        "library": sm.version(),
        "multi_library": mu.version(),
        "orc_library": orc.version(),
        "ms": res,
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
