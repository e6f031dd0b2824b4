"""bench.py --dump-outputs and the plain run: the dumped arrays are what the step computed
(sizes, statuses, per-block checksums, a fixed seeded sample of the bytes), and a run without
--full times the headline alone."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

NAMES = {"comp_len", "dec_len", "status", "comp_checksum", "dec_checksum", "sample_blocks", "comp_sample",
         "dec_sample"}


def _bench():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def _load(d):
    assert {f[:-4] for f in os.listdir(d) if f.endswith(".npy")} == NAMES
    out = {n: np.load(os.path.join(d, n + ".npy")) for n in NAMES}
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    assert sum(a.nbytes for a in out.values()) <= 64 * 2**20
    return out


def _weighted(row):
    return int((row.astype(np.int64) * (np.arange(row.size) % 251 + 1)).sum())


def test_dump_outputs_host_batch(oracle, tmp_path):
    """dump_outputs on a host-resident batch whose streams the oracle wrote: more blocks than the
    sample and than one checksum chunk, slot tails full of junk."""
    import torch
    bench = _bench()
    nblk = bench.DUMP_SAMPLE + 6
    blocks = bench.text_blocks(nblk, 0x5EED)
    b = bench.Batch(blocks, torch.device("cpu"))
    slots = np.full((nblk, bench.SLOT), 0xEE, dtype=np.uint8)
    for i in range(nblk):
        c = np.frombuffer(oracle.compress(blocks[i]), dtype=np.uint8)
        slots[i, :c.size] = c
        b.comp_len[i] = c.size
    b.d_comp.copy_(torch.from_numpy(slots.reshape(-1)))
    b.d_dec.copy_(b.d_in)
    b.dec_len.fill_(bench.BLOCK)
    bench.dump_outputs(b, str(tmp_path / "a"), chunk=32)
    bench.dump_outputs(b, str(tmp_path / "b"))
    got, again = _load(tmp_path / "a"), _load(tmp_path / "b")
    for n in NAMES:
        assert np.array_equal(got[n], again[n]), n
    clen = b.comp_len.numpy()
    assert np.array_equal(got["comp_len"], clen) and np.array_equal(got["dec_len"], np.full(nblk, bench.BLOCK))
    assert not got["status"].any()
    assert got["comp_checksum"].tolist() == [_weighted(slots[i, :clen[i]]) for i in range(nblk)]
    assert got["dec_checksum"].tolist() == [_weighted(blocks[i]) for i in range(nblk)]
    rows = got["sample_blocks"].astype(np.int64)
    assert rows.size == bench.DUMP_SAMPLE and np.all(np.diff(rows) > 0) and rows[-1] < nblk
    assert np.array_equal(got["dec_sample"], blocks[rows])
    for k, i in enumerate(rows):
        assert np.array_equal(got["comp_sample"][k, :clen[i]], slots[i, :clen[i]])
        assert not got["comp_sample"][k, clen[i]:].any()


@pytest.mark.gpu
def test_plain_run_times_the_headline_alone(oracle, gpu_available, tmp_path):
    """A run without --full prints the headline's line and nothing that takes runs of its own;
    what it dumps decodes, under the oracle, to the blocks the benchmark compressed."""
    bench = _bench()
    nblk, steps = 300, 3
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           "--blocks", str(nblk), "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["metric"] == bench.METRIC and line["unit"] == "GB/s" and line["dtype"] == "u8"
    assert line["higher_is_better"] is True and line["steps"] == steps and line["roundtrip_bit_exact"] is True
    # value is the bytes of one step's round trip over ms_per_step (both rounded in the line)
    assert line["value"] == pytest.approx(2 * nblk * bench.BLOCK / (line["ms_per_step"] * 1e-3) / 1e9, rel=1e-3)
    for key in ("random", "large", "cpu_baseline", "roofline", "reference_mode", "compress_GBps"):
        assert key not in line
    got = _load(tmp_path)
    assert got["comp_len"].shape == (nblk,) and not got["status"].any()
    assert np.array_equal(got["dec_len"], np.full(nblk, bench.BLOCK))
    blocks = bench.text_blocks(nblk, 0x5EED)
    rows = got["sample_blocks"].astype(np.int64)
    assert np.array_equal(got["dec_sample"], blocks[rows])
    assert got["dec_checksum"].tolist() == [_weighted(blocks[i]) for i in range(nblk)]
    for k, i in enumerate(rows):
        stream = got["comp_sample"][k, :int(got["comp_len"][i])].astype(np.uint8)
        assert bytes(oracle.uncompress(stream.tobytes())) == blocks[i].tobytes()
        assert got["comp_checksum"][i] == _weighted(stream)
