"""Rates of the blocks library's batched calls (Hadoop and snappy-java containers) against their
floor, on bench.py's text_blocks (10,000 x 64 KiB windows of the text files, seed 0x5EED) cut into

  a_10000x1    10,000 streams of one 64 KiB block each
  b_100x100    100 streams of 100 blocks each

For each workload, each format and each direction the alternatives are timed interleaved call by
call in one process, each by a pair of HIP events around it on the current stream, `--reps` times
after `--warmup` untimed rounds (median, minimum and maximum in milliseconds; the method of
tools/framing_range_rates.py):

  batch   smb_compress_streams_device / smb_uncompress_streams_device (max_fragments: the plan's)
  batch0  the decode with max_fragments = 0 (no index is built)
  floor   smm_compress_device / smm_uncompress_device over the same 64 KiB pieces with no container:
          no walk, no pack, no per-stream work at all; the raw streams lie in slots at multiples of 256
  place   the decode floor over the payloads where they lie inside the packed streams, at any byte
          alignment (their offsets from the host walk): what the raw decoder alone takes there

and the HADOOP decode of `--big` streams of one 218,000-byte chunk each (the size Hadoop's default
buffer gives; the payloads by the multi library's block compressor), with the index built on the
device (max_fragments from the plan) and with max_fragments = 0 (every chunk one wave, in stream
order).  No number is a gate.  Needs a GPU.

    python tools/blocks_rates.py --out profiles/blocks_rates.json
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
BLOCK = 65536
PITCH = 76544  # a piece's raw stream: its bound, rounded up to 256
BIG = 218000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=10000)
    ap.add_argument("--big", type=int, default=400)
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
        print("blocks_rates.py needs a GPU", file=sys.stderr)
        return 2
    sm = bench.load_package()
    bl = importlib.import_module("snappy_jl_amd.blocks")
    mu = importlib.import_module("snappy_jl_amd.multi")
    dev = torch.device("cuda", 0)
    nblk = args.blocks
    host_in = bench.text_blocks(nblk, 0x5EED).reshape(-1)
    d_in = torch.from_numpy(host_in).to(dev)
    n = nblk * BLOCK
    clocks_before = clocks()

    def i64(values):
        return torch.from_numpy(np.asarray(values, dtype=np.int64)).to(dev)

    def i32(values):
        return torch.from_numpy(np.asarray(values, dtype=np.int32)).to(dev)

    def zeros(k, dtype):
        return torch.zeros(k, dtype=dtype, device=dev)

    # ---- the floor: the pieces as raw streams in slots, no container
    p_off, p_len = i64([b * BLOCK for b in range(nblk)]), i32([BLOCK] * nblk)
    s_off = i64([b * PITCH for b in range(nblk)])
    d_slots = torch.empty(nblk * PITCH, dtype=torch.uint8, device=dev)
    d_clen, d_cst = zeros(nblk, torch.int32), zeros(nblk, torch.int32)
    d_dec = torch.empty(n, dtype=torch.uint8, device=dev)
    d_dlen, d_dst = zeros(nblk, torch.int32), zeros(nblk, torch.int32)

    def floor_compress():
        mu.compress_streams_device(d_in, p_off, p_len, 0, d_slots, s_off, d_clen, d_cst, mode="fast")

    def floor_decode():
        mu.uncompress_streams_device(d_slots, s_off, d_clen, 0, d_dec, p_off, p_len, d_dlen, d_dst)

    floor_compress()
    floor_decode()
    assert not bool(d_cst.any()) and not bool(d_dst.any()) and bool(torch.equal(d_dec, d_in))
    res = {}

    def workload(name, nstreams, per):
        assert nstreams * per == nblk
        size = per * BLOCK
        res[name] = {"streams": nstreams, "blocks_per_stream": per}
        for fmt in ("hadoop", "xerial"):
            room = (bl.max_length(size, fmt) + 15) // 16 * 16
            in_off, out_off = [s * size for s in range(nstreams)], [s * room for s in range(nstreams)]
            d_in_off, d_in_len, d_o_off = i64(in_off), i64([size] * nstreams), i64(out_off)
            d_packed = torch.empty(nstreams * room, dtype=torch.uint8, device=dev)
            d_plen, d_pst = zeros(nstreams, torch.int64), zeros(nstreams, torch.int32)

            def batch_compress():
                bl.compress_block_streams_device(fmt, d_in, d_in_off, d_in_len, nblk, d_packed, d_o_off, d_plen, d_pst,
                                                 mode="fast")

            c = timed(torch, [batch_compress, floor_compress], args.reps, args.warmup)
            assert not bool(d_pst.any())
            d_ol, d_ds = zeros(nstreams, torch.int64), zeros(nstreams, torch.int32)

            def batch_decode(max_fragments=nblk):
                bl.uncompress_block_streams_device(fmt, d_packed, d_o_off, d_plen, nblk, max_fragments, d_dec, d_in_off,
                                                   d_in_len, d_ol, d_ds)

            # the payloads where they lie: the host walk of every packed stream
            packed, plen = d_packed.cpu().numpy(), d_plen.cpu().tolist()
            q_off, q_len = [], []
            for s in range(nstreams):
                summary, arrays = bl.index_blocks(packed[out_off[s]:out_off[s] + plen[s]], fmt)
                assert (summary.status, summary.nchunks, summary.total_length) == (0, per, size)
                q_off += (arrays["pay_off"] + np.uint64(out_off[s])).tolist()
                q_len += arrays["pay_len"].tolist()
            d_q_off, d_q_len = i64(q_off), i32(q_len)
            d_qlen, d_qst = zeros(nblk, torch.int32), zeros(nblk, torch.int32)

            def place_decode():
                mu.uncompress_streams_device(d_packed, d_q_off, d_q_len, 0, d_dec, p_off, p_len, d_qlen, d_qst)

            d_dec.fill_(0xAA)
            batch_decode()
            assert not bool(d_ds.any()) and bool((d_ol == size).all()) and bool(torch.equal(d_dec, d_in)), (name, fmt)
            d_dec.fill_(0xAA)
            place_decode()
            assert not bool(d_qst.any()) and bool(torch.equal(d_dec, d_in)), (name, fmt)
            d = timed(torch, [batch_decode, lambda: batch_decode(0), floor_decode, place_decode], args.reps, args.warmup)
            assert not bool(d_ds.any()) and not bool(d_dst.any()) and bool(torch.equal(d_dec, d_in)), (name, fmt)
            res[name][fmt] = {
                "compress": {"batch": c[0], "floor_no_container": c[1],
                             "batch_over_floor": round(c[0]["median_ms"] / c[1]["median_ms"], 3)},
                "decode": {"batch": d[0], "batch_max_fragments_0": d[1], "floor_no_container": d[2],
                           "floor_in_place": d[3],
                           "batch_over_floor": round(d[0]["median_ms"] / d[2]["median_ms"], 3),
                           "batch0_over_floor": round(d[1]["median_ms"] / d[2]["median_ms"], 3),
                           "batch0_over_floor_in_place": round(d[1]["median_ms"] / d[3]["median_ms"], 3)},
            }
            print(name, fmt, json.dumps(res[name][fmt]), flush=True)

    workload("a_10000x1", nblk, 1)
    workload("b_100x100", nblk // 100, 100)

    # ---- HADOOP decode of 218,000-byte chunks: the index built on the device against stream order
    nbig = args.big
    big_in = d_in[:nbig * BIG]
    b_off, b_len = i64([s * BIG for s in range(nbig)]), i32([BIG] * nbig)
    cap = (32 + BIG + BIG // 6 + 15) // 16 * 16
    r_off = i64([s * cap for s in range(nbig)])
    d_raw = torch.empty(nbig * cap, dtype=torch.uint8, device=dev)
    d_rlen, d_rst = zeros(nbig, torch.int32), zeros(nbig, torch.int32)
    frags = nbig * ((BIG + BLOCK - 1) // BLOCK)
    mu.compress_streams_device(big_in, b_off, b_len, frags, d_raw, r_off, d_rlen, d_rst, mode="fast")
    assert not bool(d_rst.any())
    raw, rlen = d_raw.cpu().numpy(), d_rlen.cpu().tolist()
    streams = [BIG.to_bytes(4, "big") + rlen[s].to_bytes(4, "big") + raw[s * cap:s * cap + rlen[s]].tobytes()
               for s in range(nbig)]
    rc, _, _, _, chunks, plan_frags = bl.streams_plan(streams, "hadoop")
    assert (rc, chunks, plan_frags) == (0, nbig, frags)
    h_off = np.zeros(nbig + 1, np.int64)
    np.cumsum([len(s) for s in streams], out=h_off[1:])
    d_h = torch.from_numpy(np.frombuffer(b"".join(streams), np.uint8).copy()).to(dev)
    d_h_off, d_h_len = i64(h_off[:-1]), i64([len(s) for s in streams])
    d_bout = torch.empty(nbig * BIG, dtype=torch.uint8, device=dev)
    d_bol, d_bst = zeros(nbig, torch.int64), zeros(nbig, torch.int32)
    d_bcap = i64([BIG] * nbig)

    def big_decode(max_fragments):
        bl.uncompress_block_streams_device("hadoop", d_h, d_h_off, d_h_len, nbig, max_fragments, d_bout, b_off, d_bcap,
                                           d_bol, d_bst)

    indexed = {}
    for m in (frags, 0):
        d_bout.fill_(0xAA)
        big_decode(m)
        indexed[m] = bl.last_indexed(0)
        assert not bool(d_bst.any()) and bool(torch.equal(d_bout, big_in)), m
    assert indexed == {frags: nbig, 0: 0}, indexed
    b = timed(torch, [lambda: big_decode(frags), lambda: big_decode(0)], args.reps, args.warmup)
    res["hadoop_218000_byte_chunks"] = {
        "streams": nbig, "bytes": nbig * BIG, "with_index": b[0], "max_fragments_0": b[1],
        "index_gain": round(b[1]["median_ms"] / b[0]["median_ms"], 2),
        "with_index_GBps": round(nbig * BIG / b[0]["median_ms"] / 1e6, 2),
    }
    print("hadoop_218000_byte_chunks", json.dumps(res["hadoop_218000_byte_chunks"]), flush=True)

    report = {
        "workload": "%d x 64 KiB text blocks (bench.py text_blocks, seed 0x5EED), %d bytes, fast mode" % (nblk, n),
        "method": "HIP events around each call on one stream; the alternatives interleaved call by call; %d warm-up "
                  "rounds, %d timed; median, min, max" % (args.warmup, args.reps),
        "device": torch.cuda.get_device_name(0),
        "library": sm.version(),
        "multi_library": mu.version(),
        "blocks_library": bl.version(),
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
