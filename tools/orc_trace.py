"""The kernels of the ORC library's batched calls under `rocprofv3 --kernel-trace`, in a run of its
own (tools/orc_rates.py times the calls with the profiler off):

    rocprofv3 --kernel-trace --output-format csv -d DIR_T -o orc -- python tools/orc_trace.py run text
    rocprofv3 --kernel-trace --output-format csv -d DIR_R -o orc -- python tools/orc_trace.py run random
    python tools/orc_trace.py summarise DIR_T DIR_R profiles/orc_kernel_stats.csv

`run`: at block_size 262144, bench.py's text blocks as 100 streams of 25 pieces, or as many random
bytes as 100 streams (every chunk stored): 3 smo_compress_streams_device calls, then 5
smo_uncompress_streams_device calls with max_fragments 0 and 5 with the plan's bound.
`summarise`: per workload and kernel name, in order of first dispatch, the dispatches and the
median, minimum and maximum duration in microseconds.  Needs a GPU.
"""
import csv
import importlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BLOCK_SIZE = 262144
NOTE = ("# rocprofv3 --kernel-trace, one process per workload, block_size 262144, fast mode: text = 100 streams of 25 pieces of\n"
        "# bench.py's text blocks, random = 100 streams of as many random bytes (every chunk stored); 3 smo_compress_streams_device\n"
        "# calls, then 5 smo_uncompress_streams_device calls with max_fragments 0 and 5 with the plan's bound (text: 10000, random: 0)\n")


def run(kind):
    import numpy as np
    import torch
    import bench
    bench.load_package()
    orc = importlib.import_module("snappy_jl_amd.orc")
    dev = torch.device("cuda", 0)
    nstreams, size = 100, 25 * BLOCK_SIZE
    n, npieces = nstreams * size, nstreams * 25
    room = (orc.max_length(size, BLOCK_SIZE) + 15) // 16 * 16

    def i64(values):
        return torch.from_numpy(np.asarray(values, dtype=np.int64)).to(dev)

    in_off, in_len, out_off = i64([s * size for s in range(nstreams)]), i64([size] * nstreams), i64([s * room for s in range(nstreams)])
    d_packed = torch.empty(nstreams * room, dtype=torch.uint8, device=dev)
    d_dec = torch.empty(n, dtype=torch.uint8, device=dev)
    d_plen, d_pst = torch.zeros(nstreams, dtype=torch.int64, device=dev), torch.zeros(nstreams, dtype=torch.int32, device=dev)
    d_ol, d_ds = torch.zeros(nstreams, dtype=torch.int64, device=dev), torch.zeros(nstreams, dtype=torch.int32, device=dev)
    if kind == "text":
        host, frags = bench.text_blocks(n // 65536, 0x5EED).reshape(-1), npieces * 4
    else:
        host, frags = np.random.default_rng(0x5EED).integers(0, 256, n, dtype=np.uint8), 0
    d_in = torch.from_numpy(host).to(dev)
    for _ in range(3):
        orc.compress_orc_streams_device(BLOCK_SIZE, d_in, in_off, in_len, npieces, d_packed, out_off, d_plen, d_pst)
    for m in [0] * 5 + [frags] * 5:
        orc.uncompress_orc_streams_device(BLOCK_SIZE, d_packed, out_off, d_plen, npieces, m, d_dec, in_off, in_len, d_ol, d_ds)
    torch.cuda.synchronize()
    assert not bool(d_pst.any()) and not bool(d_ds.any()) and bool(torch.equal(d_dec, d_in))
    print("orc_trace run ok:", kind)


def kernel_times(trace_dir):
    rows = {}
    for d, _, files in os.walk(trace_dir):
        for f in files:
            if not f.endswith("kernel_trace.csv"):
                continue
            with open(os.path.join(d, f), newline="") as fh:
                for r in csv.DictReader(fh):
                    name = r["Kernel_Name"].split("(")[0].replace("void ", "").replace(",", ";")
                    if not name.startswith(("smo::", "smm::", "sm::")):  # (torch's own fills and compares)
                        continue
                    start, end = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
                    rows.setdefault(name, []).append((start, (end - start) / 1000.0))
    assert rows, "no kernel_trace.csv under %s" % trace_dir
    return rows


def summarise(text_dir, random_dir, out_path):
    with open(out_path, "w") as fh:
        fh.write(NOTE)
        fh.write("workload,kernel,dispatches,median_us,min_us,max_us\n")
        for kind, d in (("text", text_dir), ("random", random_dir)):
            for name, v in sorted(kernel_times(d).items(), key=lambda kv: min(t for t, _ in kv[1])):
                us = [u for _, u in v]
                fh.write("%s,%s,%d,%.1f,%.1f,%.1f\n" % (kind, name, len(us), statistics.median(us), min(us), max(us)))
    print(open(out_path).read())


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run" and sys.argv[2] in ("text", "random"):
        run(sys.argv[2])
    elif len(sys.argv) == 5 and sys.argv[1] == "summarise":
        summarise(sys.argv[2], sys.argv[3], sys.argv[4])
    else:
        sys.exit(__doc__)
