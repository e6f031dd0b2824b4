"""Rates of the Kafka segment library's device calls next to the blocks library's XERIAL calls on
identical payloads, on bench.py's text_blocks (10,000 x 64 KiB windows of the text files, seed
0x5EED), each window the records payload of one uncompressed batch (smk_write_batch), cut into

  a_10000x1    10,000 segments of one 64 KiB batch each
  b_100x100    100 segments of 100 batches each

For each workload the alternatives are timed interleaved call by call in one process, each by a pair
of HIP events around it on the current stream, `--reps` times after `--warmup` untimed rounds
(median, minimum and maximum in milliseconds; the method of tools/table_rates.py):

  encode   smk_compress_segments_device (walks, the snappy-java encoder into a stage, pack, headers,
           checksums) against smb_compress_streams_device (XERIAL) over the same payloads
  decode   smk_uncompress_segments_device with verify_crc, the same without (the difference is the
           stored bytes' checksum's share), against smb_uncompress_streams_device (XERIAL) over the
           streams the blocks call wrote; all with max_fragments = 0 (every chunk is at most 64 KiB)

The decode's output is held against the segments the encoder read: the round trip is byte exact.
No number is a gate.  Needs a GPU.

    python tools/kafka_rates.py --out profiles/kafka_rates.json
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
HEADER = 61


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", choices=("a", "b", "both"), default="both", help="for a kernel trace of one workload")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import bench
    from framing_range_rates import timed
    from framing_rates import clocks
    if not torch.cuda.is_available():
        print("kafka_rates.py needs a GPU", file=sys.stderr)
        return 2
    sm = bench.load_package()
    kf = importlib.import_module("snappy_jl_amd.kafka")
    bl = importlib.import_module("snappy_jl_amd.blocks")
    dev = torch.device("cuda", 0)
    nblk = args.blocks
    n = nblk * BLOCK
    payloads = bench.text_blocks(nblk, 0x5EED).reshape(-1)
    # every window as one uncompressed batch, back to back: both workloads read the same bytes
    pitch = HEADER + BLOCK
    plain = np.empty(nblk * pitch, np.uint8)
    tail = bytes(20) + b"\xff" * 14 + (1).to_bytes(4, "big")
    got = ctypes.c_size_t(0)
    for j in range(nblk):
        st = kf.lib().smk_write_batch(j, 0, 0, tail, payloads.ctypes.data + j * BLOCK, BLOCK, plain.ctypes.data + j * pitch, pitch,
                                      ctypes.byref(got))
        assert st == 0 and got.value == pitch
    d_plain = torch.from_numpy(plain).to(dev)
    clocks_before = clocks()

    def i64(values):
        return torch.from_numpy(np.asarray(values, dtype=np.int64)).to(dev)

    def zeros(k, dtype):
        return torch.zeros(k, dtype=dtype, device=dev)

    # the blocks library's side: the payloads where they stand in the segments, a stream each
    x_room = (bl.max_length(BLOCK, "xerial") + 15) // 16 * 16
    d_p_off, d_p_len = i64([j * pitch + HEADER for j in range(nblk)]), i64([BLOCK] * nblk)
    d_x_off = i64([j * x_room for j in range(nblk)])
    d_xerial = torch.empty(nblk * x_room, dtype=torch.uint8, device=dev)
    d_xlen, d_xst = zeros(nblk, torch.int64), zeros(nblk, torch.int32)
    d_raw = torch.empty(n, dtype=torch.uint8, device=dev)
    d_r_off, d_r_cap = i64([j * BLOCK for j in range(nblk)]), i64([BLOCK] * nblk)
    d_rlen, d_rst = zeros(nblk, torch.int64), zeros(nblk, torch.int32)
    d_payloads = torch.from_numpy(payloads).to(dev)
    stage = nblk * kf.stage_length(BLOCK)
    d_dec = torch.empty(nblk * pitch, dtype=torch.uint8, device=dev)
    res = {}

    def blocks_encode():
        bl.compress_block_streams_device("xerial", d_plain, d_p_off, d_p_len, nblk, d_xerial, d_x_off, d_xlen, d_xst, mode="fast")

    def blocks_decode():
        bl.uncompress_block_streams_device("xerial", d_xerial, d_x_off, d_xlen, nblk, 0, d_raw, d_r_off, d_r_cap, d_rlen, d_rst)

    def workload(name, nseg, per):
        assert nseg * per == nblk
        size = per * pitch
        room = (kf.max_segment_length(size, per) + 15) // 16 * 16
        d_s_off, d_s_len = i64([t * size for t in range(nseg)]), i64([size] * nseg)
        d_o_off = i64([t * room for t in range(nseg)])
        d_enc = torch.empty(nseg * room, dtype=torch.uint8, device=dev)
        d_elen, d_est = zeros(nseg, torch.int64), zeros(nseg, torch.int32)

        def kafka_encode():
            kf.compress_segments_device(d_plain, d_s_off, d_s_len, nblk, nblk, stage, d_enc, d_o_off, d_elen, d_est, mode="fast")

        c = timed(torch, [kafka_encode, blocks_encode], args.reps, args.warmup)
        assert not bool(d_est.any()) and not bool(d_xst.any())
        d_cap = i64([size] * nseg)
        d_dlen, d_dst = zeros(nseg, torch.int64), zeros(nseg, torch.int32)

        def kafka_decode(verify=True):
            kf.uncompress_segments_device(d_enc, d_o_off, d_elen, nblk, nblk, 0, d_dec, d_s_off, d_cap, d_dlen, d_dst, verify_crc=verify)

        for verify in (True, False):
            d_dec.fill_(0xAA)
            kafka_decode(verify)
            assert not bool(d_dst.any()) and bool((d_dlen == size).all()) and bool(torch.equal(d_dec, d_plain)), name
        d_raw.fill_(0xAA)
        blocks_decode()
        assert not bool(d_rst.any()) and bool(torch.equal(d_raw, d_payloads)), name
        d = timed(torch, [kafka_decode, lambda: kafka_decode(False), blocks_decode], args.reps, args.warmup)
        assert not bool(d_dst.any())
        gb = lambda t: round(n / t["median_ms"] / 1e6, 2)
        res[name] = {
            "segments": nseg, "batches_per_segment": per, "segment_bytes": int(d_elen.sum()), "xerial_bytes": int(d_xlen.sum()),
            "encode": {"kafka": c[0], "blocks_xerial": c[1], "kafka_GBps": gb(c[0]), "blocks_GBps": gb(c[1]),
                       "kafka_over_blocks": round(c[0]["median_ms"] / c[1]["median_ms"], 3)},
            "decode": {"kafka_verify_crc": d[0], "kafka_no_crc": d[1], "blocks_xerial": d[2], "kafka_verify_GBps": gb(d[0]),
                       "kafka_no_crc_GBps": gb(d[1]), "blocks_GBps": gb(d[2]),
                       "crc_share_of_verify": round(1 - d[1]["median_ms"] / d[0]["median_ms"], 3),
                       "kafka_no_crc_over_blocks": round(d[1]["median_ms"] / d[2]["median_ms"], 3),
                       "kafka_verify_over_blocks": round(d[0]["median_ms"] / d[2]["median_ms"], 3)},
        }
        print(name, json.dumps(res[name]), flush=True)

    if args.workload in ("a", "both"):
        workload("a_10000x1", nblk, 1)
    if args.workload in ("b", "both"):
        workload("b_100x100", nblk // 100, 100)

    report = {
        "workload": "%d x 64 KiB text blocks (bench.py text_blocks, seed 0x5EED), %d bytes of records, fast mode" % (nblk, n),
        "method": "HIP events around each call on one stream; the alternatives interleaved call by call; %d warm-up "
                  "rounds, %d timed; median, min, max; GB/s over the uncompressed records" % (args.warmup, args.reps),
        "device": torch.cuda.get_device_name(0),
        "library": sm.version(),
        "kafka_library": kf.version(),
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
