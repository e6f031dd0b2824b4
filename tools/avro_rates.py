"""Rates of the Avro container library's device calls next to the blocks library's on identical
payloads, on bench.py's text_blocks (10,000 x 64 KiB windows of the text files, seed 0x5EED) cut into

  a_10000x1    10,000 files of one 64 KiB block each
  b_100x100    100 files of 100 blocks each

For each workload the alternatives are timed interleaved call by call in one process, each by a pair
of HIP events around it on the current stream, `--reps` times after `--warmup` untimed rounds
(median, minimum and maximum in milliseconds; the method of tools/blocks_rates.py):

  encode   sma_compress_streams_device (header, blocks, checksums, markers) against
           smb_compress_streams_device writing the same pieces as Hadoop blocks
  decode   sma_uncompress_streams_device with verify_crc, the same without (the difference is the
           checksum's share), against smb_uncompress_streams_device over the Hadoop streams; all with
           max_fragments = 0 (every payload is at most 64 KiB)
  sync     sma_find_sync_device: one query per MiB of every file of the workload (the split points of
           a parallel reader), and one query over all the uncompressed input as a single stream that
           holds no marker (the plain scan)

No number is a gate.  Needs a GPU.

    python tools/avro_rates.py --out profiles/avro_rates.json
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
SCHEMA = b'{"type": "record", "name": "Line", "fields": [{"name": "line", "type": "string"}]}'
OBJECTS = 1000  # per block: a two-byte long


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
        print("avro_rates.py needs a GPU", file=sys.stderr)
        return 2
    sm = bench.load_package()
    av = importlib.import_module("snappy_jl_amd.avro")
    bl = importlib.import_module("snappy_jl_amd.blocks")
    dev = torch.device("cuda", 0)
    nblk = args.blocks
    n = nblk * BLOCK
    sync = bytes(range(0x30, 0x40))
    head = av.write_header(SCHEMA, sync)
    host_in = bench.text_blocks(nblk, 0x5EED).reshape(-1)
    # the header behind the blocks: the encoder copies it in front of every file
    d_in = torch.from_numpy(np.concatenate([host_in, np.frombuffer(head, np.uint8)])).to(dev)
    clocks_before = clocks()

    def i64(values):
        return torch.from_numpy(np.asarray(values, dtype=np.int64)).to(dev)

    def i32(values):
        return torch.from_numpy(np.asarray(values, dtype=np.int32)).to(dev)

    def zeros(k, dtype):
        return torch.zeros(k, dtype=dtype, device=dev)

    b_off, b_len, b_cnt = i64([b * BLOCK for b in range(nblk)]), i32([BLOCK] * nblk), i64([OBJECTS] * nblk)
    stage = nblk * av.lib().sma_stage_length(BLOCK)
    d_dec = torch.empty(n, dtype=torch.uint8, device=dev)
    res = {}

    def workload(name, nstreams, per):
        assert nstreams * per == nblk
        size = per * BLOCK
        room = (len(head) + per * av.max_block_length(BLOCK) + 15) // 16 * 16
        d_first = i32([s * per for s in range(nstreams + 1)])
        d_sync = torch.from_numpy(np.frombuffer(sync * nstreams, np.uint8).copy()).to(dev)
        d_h_off, d_h_len = i64([n] * nstreams), i64([len(head)] * nstreams)
        out_off = [s * room for s in range(nstreams)]
        d_o_off = i64(out_off)
        d_avro = torch.empty(nstreams * room, dtype=torch.uint8, device=dev)
        d_alen, d_ast = zeros(nstreams, torch.int64), zeros(nstreams, torch.int32)

        def avro_encode():
            av.compress_avro_streams_device(d_in, d_first, b_off, b_len, b_cnt, d_sync, nblk, stage, 0, d_avro, d_o_off, d_alen,
                                            d_ast, d_head_off=d_h_off, d_head_len=d_h_len, mode="fast")

        h_room = (bl.max_length(size, "hadoop") + 15) // 16 * 16
        d_s_off, d_s_len, d_ho_off = i64([s * size for s in range(nstreams)]), i64([size] * nstreams), i64([s * h_room for s in range(nstreams)])
        d_hadoop = torch.empty(nstreams * h_room, dtype=torch.uint8, device=dev)
        d_hlen, d_hst = zeros(nstreams, torch.int64), zeros(nstreams, torch.int32)

        def blocks_encode():
            bl.compress_block_streams_device("hadoop", d_in, d_s_off, d_s_len, nblk, d_hadoop, d_ho_off, d_hlen, d_hst, mode="fast")

        c = timed(torch, [avro_encode, blocks_encode], args.reps, args.warmup)
        assert not bool(d_ast.any()) and not bool(d_hst.any())
        # the first file under the host walk: what was written is a file of `per` blocks
        first = d_avro[:int(d_alen[0])].cpu().numpy().tobytes()
        s, _ = av.index_avro(first)
        assert (s.status, s.nblocks, s.total_length, s.objects) == (0, per, size, per * OBJECTS)
        d_cap = i64([size] * nstreams)
        d_ol, d_ds, d_ob = zeros(nstreams, torch.int64), zeros(nstreams, torch.int32), zeros(nstreams, torch.int64)

        def avro_decode(verify=True):
            av.uncompress_avro_streams_device(d_avro, d_o_off, d_alen, nblk, 0, d_dec, d_s_off, d_cap, d_ol, d_ds,
                                              verify_crc=verify, d_objects=d_ob)

        def blocks_decode():
            bl.uncompress_block_streams_device("hadoop", d_hadoop, d_ho_off, d_hlen, nblk, 0, d_dec, d_s_off, d_cap, d_ol, d_ds)

        for fn in (avro_decode, blocks_decode):
            d_dec.fill_(0xAA)
            fn()
            assert not bool(d_ds.any()) and bool((d_ol == size).all()) and bool(torch.equal(d_dec, d_in[:n])), name
        d = timed(torch, [avro_decode, lambda: avro_decode(False), blocks_decode], args.reps, args.warmup)
        assert not bool(d_ds.any())
        # the split points: one per MiB of every file
        alen = d_alen.cpu().tolist()
        queries = [(s, f) for s in range(nstreams) for f in range(0, alen[s], 1 << 20)]
        d_qs, d_qf = i32([q[0] for q in queries]), i64([q[1] for q in queries])
        d_pos = zeros(len(queries), torch.int64)

        def splits():
            av.find_sync_device(d_avro, d_o_off, d_alen, d_sync, d_qs, d_qf, d_pos)

        splits()
        pos = d_pos.cpu().tolist()
        assert pos[0] == len(head) - 16 and all(q[1] <= p <= alen[q[0]] for p, q in zip(pos, queries))
        y = timed(torch, [splits], args.reps, args.warmup)
        gb = lambda t: round(n / t["median_ms"] / 1e6, 2)
        res[name] = {
            "files": nstreams, "blocks_per_file": per, "avro_bytes": int(sum(alen)), "hadoop_bytes": int(d_hlen.sum()),
            "encode": {"avro": c[0], "blocks_hadoop": c[1], "avro_GBps": gb(c[0]), "blocks_GBps": gb(c[1]),
                       "avro_over_blocks": round(c[0]["median_ms"] / c[1]["median_ms"], 3)},
            "decode": {"avro_verify_crc": d[0], "avro_no_crc": d[1], "blocks_hadoop": d[2], "avro_verify_GBps": gb(d[0]),
                       "avro_no_crc_GBps": gb(d[1]), "blocks_GBps": gb(d[2]),
                       "crc_share_of_verify": round(1 - d[1]["median_ms"] / d[0]["median_ms"], 3),
                       "avro_no_crc_over_blocks": round(d[1]["median_ms"] / d[2]["median_ms"], 3),
                       "avro_verify_over_blocks": round(d[0]["median_ms"] / d[2]["median_ms"], 3)},
            "sync_search": {"queries": len(queries), "splits": y[0]},
        }
        print(name, json.dumps(res[name]), flush=True)

    if args.workload in ("a", "both"):
        workload("a_10000x1", nblk, 1)
    if args.workload in ("b", "both"):
        workload("b_100x100", nblk // 100, 100)

    # ---- the plain scan: all the input as one stream without a marker
    d_one_off, d_one_len = i64([0]), i64([n])
    d_m = torch.from_numpy(np.frombuffer(sync, np.uint8).copy()).to(dev)
    d_q0, d_f0, d_p0 = i32([0]), i64([0]), zeros(1, torch.int64)

    def scan():
        av.find_sync_device(d_in, d_one_off, d_one_len, d_m, d_q0, d_f0, d_p0)

    scan()
    assert int(d_p0[0]) == n
    t = timed(torch, [scan], args.reps, args.warmup)[0]
    res["sync_scan_no_marker"] = {"bytes": n, "scan": t, "GBps": round(n / t["median_ms"] / 1e6, 2)}
    print("sync_scan_no_marker", json.dumps(res["sync_scan_no_marker"]), flush=True)

    report = {
        "workload": "%d x 64 KiB text blocks (bench.py text_blocks, seed 0x5EED), %d bytes, fast mode" % (nblk, n),
        "method": "HIP events around each call on one stream; the alternatives interleaved call by call; %d warm-up "
                  "rounds, %d timed; median, min, max; GB/s over the uncompressed bytes" % (args.warmup, args.reps),
        "device": torch.cuda.get_device_name(0),
        "library": sm.version(),
        "avro_library": av.version(),
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
