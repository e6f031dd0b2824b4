"""Rates of the LevelDB table library's device calls next to the blocks library's on identical
payloads, on bench.py's text_blocks (10,000 x 64 KiB windows of the text files, seed 0x5EED) cut into

  a_10000x1    10,000 tables of one 64 KiB data block each
  b_100x100    100 tables of 100 data blocks each

For each workload the alternatives are timed interleaved call by call in one process, each by a pair
of HIP events around it on the current stream, `--reps` times after `--warmup` untimed rounds
(median, minimum and maximum in milliseconds; the method of tools/blocks_rates.py):

  encode   smt_compress_blocks_device (compress, the 12.5 % rule, pack, checksums) against
           smb_compress_streams_device writing the same pieces as Hadoop blocks
  decode   smt_uncompress_tables_device with verify_crc, the same without (the difference is the
           checksum's share), against smb_uncompress_streams_device over the Hadoop streams; all with
           max_fragments = 0 (every block is at most 64 KiB)
  index    smt_index_tables_device alone: footers, index blocks, walks

The tables are whole files: the device-written data blocks with the tail smt_write_tail gives them.
No number is a gate.  Needs a GPU.

    python tools/table_rates.py --out profiles/table_rates.json
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
        print("table_rates.py needs a GPU", file=sys.stderr)
        return 2
    sm = bench.load_package()
    tb = importlib.import_module("snappy_jl_amd.table")
    bl = importlib.import_module("snappy_jl_amd.blocks")
    dev = torch.device("cuda", 0)
    nblk = args.blocks
    n = nblk * BLOCK
    host_in = bench.text_blocks(nblk, 0x5EED).reshape(-1)
    d_in = torch.from_numpy(host_in).to(dev)
    clocks_before = clocks()

    def i64(values):
        return torch.from_numpy(np.asarray(values, dtype=np.int64)).to(dev)

    def i32(values):
        return torch.from_numpy(np.asarray(values, dtype=np.int32)).to(dev)

    def zeros(k, dtype):
        return torch.zeros(k, dtype=dtype, device=dev)

    b_off, b_len = i64([b * BLOCK for b in range(nblk)]), i32([BLOCK] * nblk)
    stage = nblk * tb.lib().smt_stage_length(BLOCK)
    d_dec = torch.empty(n, dtype=torch.uint8, device=dev)
    res = {}

    def workload(name, ntables, per):
        assert ntables * per == nblk
        size = per * BLOCK
        room = (per * tb.max_block_length(BLOCK) + 15) // 16 * 16
        d_first = i32([t * per for t in range(ntables + 1)])
        out_off = [t * room for t in range(ntables)]
        d_o_off = i64(out_off)
        d_data = torch.empty(ntables * room, dtype=torch.uint8, device=dev)
        d_tlen, d_tst = zeros(ntables, torch.int64), zeros(ntables, torch.int32)
        d_ho, d_hs = zeros(nblk, torch.int64), zeros(nblk, torch.int64)

        def table_encode():
            tb.compress_table_blocks_device(d_in, d_first, b_off, b_len, nblk, stage, 0, d_data, d_o_off, d_ho, d_hs, d_tlen, d_tst,
                                            mode="fast")

        h_room = (bl.max_length(size, "hadoop") + 15) // 16 * 16
        d_s_off, d_s_len, d_ho_off = i64([t * size for t in range(ntables)]), i64([size] * ntables), i64([t * h_room for t in range(ntables)])
        d_hadoop = torch.empty(ntables * h_room, dtype=torch.uint8, device=dev)
        d_hlen, d_hst = zeros(ntables, torch.int64), zeros(ntables, torch.int32)

        def blocks_encode():
            bl.compress_block_streams_device("hadoop", d_in, d_s_off, d_s_len, nblk, d_hadoop, d_ho_off, d_hlen, d_hst, mode="fast")

        c = timed(torch, [table_encode, blocks_encode], args.reps, args.warmup)
        assert not bool(d_tst.any()) and not bool(d_hst.any())
        # whole files: each table's data blocks with the tail the host helper writes for them
        data, tlen = d_data.cpu().numpy(), d_tlen.cpu().tolist()
        ho, hs = d_ho.cpu().tolist(), d_hs.cpu().tolist()
        pieces, t_off, t_len, pos, index_bytes = [], [], [], 0, 0
        for t in range(ntables):
            handles = list(zip(ho[t * per:(t + 1) * per], hs[t * per:(t + 1) * per]))
            tail = tb.write_tail([b"key%08d" % (t * per + j) for j in range(per)], handles, tlen[t])
            pieces += [data[out_off[t]:out_off[t] + tlen[t]], np.frombuffer(tail, np.uint8)]
            t_off.append(pos)
            t_len.append(tlen[t] + len(tail))
            pos += t_len[-1]
            # the tail: the 13-byte metaindex block, the stored index block with its trailer, the footer
            index_bytes += (len(tail) - 13 - 5 - 48 + 15) // 16 * 16
        files = np.concatenate(pieces)
        first = files[t_off[0]:t_off[0] + t_len[0]].tobytes()
        ib = tb.index_bound(first)
        assert len(tb.walk_index(first[tb.read_footer(first)[1][0]:][:ib], len(first))[2]) == per
        d_files = torch.from_numpy(files).to(dev)
        d_t_off, d_t_len = i64(t_off), i64(t_len)
        d_cap = i64([size] * ntables)
        d_ol, d_ds = zeros(ntables, torch.int64), zeros(ntables, torch.int32)

        def table_decode(verify=True):
            tb.uncompress_tables_device(d_files, d_t_off, d_t_len, nblk, index_bytes, 0, d_dec, d_s_off, d_cap, d_ol, d_ds,
                                        verify_crc=verify)

        def blocks_decode():
            bl.uncompress_block_streams_device("hadoop", d_hadoop, d_ho_off, d_hlen, nblk, 0, d_dec, d_s_off, d_cap, d_ol, d_ds)

        for fn in (table_decode, blocks_decode):
            d_dec.fill_(0xAA)
            fn()
            assert not bool(d_ds.any()) and bool((d_ol == size).all()) and bool(torch.equal(d_dec, d_in)), name
        d = timed(torch, [table_decode, lambda: table_decode(False), blocks_decode], args.reps, args.warmup)
        assert not bool(d_ds.any())
        d_bf, d_xo, d_xs, d_xst = zeros(ntables + 1, torch.int32), zeros(nblk, torch.int64), zeros(nblk, torch.int64), zeros(ntables, torch.int32)

        def index_only(verify=True):
            tb.index_tables_device(d_files, d_t_off, d_t_len, nblk, index_bytes, d_bf, d_xo, d_xs, d_xst, verify_crc=verify)

        index_only()
        assert not bool(d_xst.any()) and int(d_bf[-1]) == nblk and bool(torch.equal(d_xs, d_hs))
        x = timed(torch, [index_only, lambda: index_only(False)], args.reps, args.warmup)
        gb = lambda t: round(n / t["median_ms"] / 1e6, 2)
        res[name] = {
            "tables": ntables, "blocks_per_table": per, "table_bytes": int(sum(t_len)), "hadoop_bytes": int(d_hlen.sum()),
            "index_bytes_bound": int(index_bytes),
            "encode": {"table": c[0], "blocks_hadoop": c[1], "table_GBps": gb(c[0]), "blocks_GBps": gb(c[1]),
                       "table_over_blocks": round(c[0]["median_ms"] / c[1]["median_ms"], 3)},
            "decode": {"table_verify_crc": d[0], "table_no_crc": d[1], "blocks_hadoop": d[2], "table_verify_GBps": gb(d[0]),
                       "table_no_crc_GBps": gb(d[1]), "blocks_GBps": gb(d[2]),
                       "crc_share_of_verify": round(1 - d[1]["median_ms"] / d[0]["median_ms"], 3),
                       "table_no_crc_over_blocks": round(d[1]["median_ms"] / d[2]["median_ms"], 3),
                       "table_verify_over_blocks": round(d[0]["median_ms"] / d[2]["median_ms"], 3)},
            "index_stage": {"verify_crc": x[0], "no_crc": x[1]},
        }
        print(name, json.dumps(res[name]), flush=True)

    if args.workload in ("a", "both"):
        workload("a_10000x1", nblk, 1)
    if args.workload in ("b", "both"):
        workload("b_100x100", nblk // 100, 100)

    report = {
        "workload": "%d x 64 KiB text blocks (bench.py text_blocks, seed 0x5EED), %d bytes, fast mode" % (nblk, n),
        "method": "HIP events around each call on one stream; the alternatives interleaved call by call; %d warm-up "
                  "rounds, %d timed; median, min, max; GB/s over the uncompressed bytes" % (args.warmup, args.reps),
        "device": torch.cuda.get_device_name(0),
        "library": sm.version(),
        "table_library": tb.version(),
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
