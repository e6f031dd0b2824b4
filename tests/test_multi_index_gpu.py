"""The index build of the multi-stream library on the device (include/snappy_mi355x_multi.h,
smm_index_device; kernels in csrc/multi/smm_index.hip): the index it builds for the library's own
streams is the compressor's, the device agrees with smm_index_host and with the plain-Python rule
(tests/multi_index_ref.py) on every case of test_multi_index_host.py, on a sweep of the boundary
tag's position over the staged pieces' edges, through the decoder, and under graph capture.  Input
buffers have exactly the streams' size, and frag_pos carries sentinel entries behind the bound."""
import importlib

import numpy as np
import pytest

import multi_index_ref as X
import multi_ref as R
from test_multi_index_host import host_call, same

pytestmark = pytest.mark.gpu

MODES = ("reference", "fast", "dense")


@pytest.fixture(scope="module")
def mu(sm, gpu_available):
    return importlib.import_module("snappy_jl_amd.multi")


def _dev():
    import torch
    return torch.device("cuda", 0)


def _t(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(dtype)).to(_dev())


class DeviceCall:
    """The device arrays of one smm_index_device call: the streams at the given offsets of a buffer of
    exactly `total` bytes (default: back to back), the results preset to sentinels."""

    def __init__(self, strs, caps, lens, m, offs=None, guard=X.GUARDS):
        import torch
        n = len(strs)
        own = [len(s) for s in strs]
        if offs is None:
            offs = np.concatenate([[0], np.cumsum(own)])[:n].tolist()
        total = max([o + l for o, l in zip(offs, own)] + [1])
        buf = np.zeros(total, np.uint8)
        for o, s in zip(offs, strs):
            buf[o:o + len(s)] = np.frombuffer(s, np.uint8)
        self.n, self.m = n, m
        self.d_in = _t(buf, np.uint8)
        assert self.d_in.data_ptr() % 16 == 0
        self.mods = [(self.d_in.data_ptr() + o) % 16 for o in offs]
        self.d_off = _t(np.array(offs, np.uint64), np.int64)
        self.d_len = _t(np.array(own if lens is None else lens, np.uint32), np.int32)
        self.d_cap = None if caps is None else _t(np.array(caps, np.uint32), np.int32)
        self.d_first = _t(np.full(n + 1, X.GUARD, np.uint32), np.int32)
        self.d_pos = _t(np.full(m + guard, X.GUARD, np.uint32), np.int32)
        self.d_built = torch.full((max(n, 1),), 7, dtype=torch.uint8, device=_dev())
        self.d_status = torch.full((max(n, 1),), -1, dtype=torch.int32, device=_dev())

    def launch(self, mu):
        mu.index_streams_device(self.d_in, self.d_off, self.d_len, self.m, self.d_first, self.d_pos, self.d_built,
                                self.d_status, d_out_cap=self.d_cap)

    def results(self):
        import torch
        torch.cuda.synchronize()
        return (self.d_first.cpu().numpy().view(np.uint32), self.d_pos.cpu().numpy().view(np.uint32),
                self.d_built.cpu().numpy()[:self.n], self.d_status.cpu().numpy()[:self.n])


def device_call(mu, strs, caps, lens, m, offs=None):
    c = DeviceCall(strs, caps, lens, m, offs)
    c.launch(mu)
    return c.results()


# ---- 5. the compressor's own index ---------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_ladder_index_is_the_compressors(mu, mode):
    datas = R.ladder_datas()
    strs, (first, pos) = mu.compress_streams(datas, mode=mode, return_index=True)
    offs, cur = [], 0
    for k, s in enumerate(strs):  # stream k at the next address that is k mod 16; the buffer ends with the last
        cur += (k - cur) % 16
        offs.append(cur)
        cur += len(s)
    c = DeviceCall(strs, None, None, int(first[-1]), offs)
    assert c.mods == [k % 16 for k in range(16)] and c.d_in.numel() == offs[-1] + len(strs[-1])
    c.launch(mu)
    got_first, got_pos, built, status = c.results()
    assert got_first.tolist() == first.tolist()
    assert got_pos.tolist() == pos.tolist() + [X.GUARD] * X.GUARDS
    assert built.tolist() == [int(len(d) > 65536) for d in datas] and not status.any()


# ---- 6. device = host = model ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["ladder", "cpu_index", "foreign", "fuzz", "hand", "hand_no_cap", "hand_overflow"])
def test_device_host_and_model_agree(mu, oracle, name):
    strs, caps, lens, m = X.groups(oracle)[name]
    want = X.group_model(oracle, name)
    same(host_call(mu, strs, caps, lens, m), want, name + " (host)")
    same(device_call(mu, strs, caps, lens, m), want, name + " (device)")
    if name == "foreign":
        assert not want[2].any()
    if name == "cpu_index":
        assert want[1][:11].tolist() == [p for c in X.cpu_index_cases(oracle) for p in c[1]] and want[2].all()


def test_host_buffer_call_and_no_streams(mu, oracle):
    import torch
    strs, caps, lens, m = X.groups(oracle)["cpu_index"]
    want = X.group_model(oracle, "cpu_index")
    first, pos, built = mu.index_streams(strs, max_fragments=m)
    assert first.tolist() == want[0].tolist() and pos.tolist() == want[1][:11].tolist() and built.tolist() == [1] * 4
    with pytest.raises(mu.SnappyError):
        mu.index_streams(strs, max_fragments=10)
    first, pos, built = mu.index_streams([])
    assert first.tolist() == [0] and pos.size == 0
    c = DeviceCall([], None, None, 0)
    c.launch(mu)
    got = c.results()
    assert got[0].tolist() == [0] and got[1].tolist() == [X.GUARD] * X.GUARDS


# ---- 7. the boundary tag at every position around the staged pieces' edges ---------------------------------

def test_staging_sweep(mu):
    stage = mu.INDEX_STAGE
    cases = X.sweep_cases(stage)
    assert len(cases) >= 1200
    assert {c[1] for c in cases} == {p for j in (1, 2) for p in range(j * stage - 300, j * stage + 301)}
    assert {c[1] % 256 for c in cases} == set(range(256))
    strs = [c[0] for c in cases]
    m = 2 * len(strs)
    want = X.model(strs, None, m, None, X.GUARDS)
    assert want[2].tolist() == [0 if c[2] else 1 for c in cases]
    assert all(int(want[1][2 * k + 1]) == (0 if c[2] else c[1]) for k, c in enumerate(cases))
    same(device_call(mu, strs, None, None, m), want, "sweep")


# ---- 8. through the decoder -------------------------------------------------------------------------------

def test_fuzz_decodes_with_the_built_index(mu, oracle):
    strs, caps, lens, m = X.groups(oracle)["fuzz"]
    first, pos, built, status = X.group_model(oracle, "fuzz")
    want = R.model_batch(strs, caps, first, pos[:m], m, oracle)
    outs, st = mu.uncompress_streams(strs, index="build", capacities=caps)
    nidx = mu.last_indexed(0)
    bad = [(k, int(st[k]), w[0]) for k, w in enumerate(want) if int(st[k]) != w[0]]
    assert not bad, bad[:8]
    assert all(o == w[1] for o, w in zip(outs, want))
    count = sum(1 for w in want if w[2])
    assert nidx == count and count >= 50, (nidx, count)


def test_oracle_streams_decode_by_fragments(mu, oracle):
    datas = R.ladder_datas() + [R.sources()[k % 3][3:3 + n] for k, n in enumerate(X.CPU_INDEX_LENGTHS)]
    strs = X.groups(oracle)["ladder"][0] + X.groups(oracle)["cpu_index"][0]
    outs, st = mu.uncompress_streams(strs, index="build")
    assert not st.any() and outs == datas
    assert mu.last_indexed(0) == sum(1 for d in datas if len(d) > 65536) == 12
    outs, st = mu.uncompress_streams(strs)  # the default: no index, as before
    assert not st.any() and outs == datas and mu.last_indexed(0) == 0
    with pytest.raises(ValueError):
        mu.uncompress_streams(strs, index="guess")


# ---- 9. capture ---------------------------------------------------------------------------------------------

def test_index_call_under_graph_capture(mu, oracle):
    import torch
    strs, caps, lens, m = X.groups(oracle)["ladder"]
    want = X.group_model(oracle, "ladder")
    c = DeviceCall(strs, caps, lens, m)
    c.launch(mu)  # (the ctx's scratch is allocated outside the capture)
    same(c.results(), want, "eager")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c.launch(mu)
    for _ in range(2):
        c.d_first.fill_(-1)
        c.d_pos.fill_(-1)
        c.d_built.fill_(7)
        c.d_status.fill_(-1)
        g.replay()
        got = c.results()
        assert got[1][m:].tolist() == [0xFFFFFFFF] * X.GUARDS
        same((got[0], got[1][:m], got[2], got[3]), (want[0], want[1][:m], want[2], want[3]), "replay")
