"""The `stream` and `device` arguments of the device wrappers, one wrapper per library and per way
it used to resolve them: stream None (torch's current stream), a torch.cuda.Stream and that
stream's raw handle, each with the device taken from the tensor and given explicitly.  Every form
must give the bytes of the matching host-buffer call, and those decode to the input under the CPU
oracle.  Valid inputs of the smallest shapes that take every branch."""
import importlib

import numpy as np
import pytest

import framing_ref as FR
from conftest import read_testfile

pytestmark = pytest.mark.gpu

TEXT = read_testfile("alice29.txt")
BLOCKS = [b"", b"x", TEXT[:300]]            # raw: an empty block, one byte, one with matches
FRAMED_INPUT = TEXT[:70000]                 # framing: two chunks
STREAM_INPUTS = [TEXT[:100], TEXT[:70000]]  # streams of any length: one of a single fragment, one of two


@pytest.fixture(scope="module")
def fr(sm, gpu_available):
    return importlib.import_module("snappy_jl_amd.framing")


@pytest.fixture(scope="module")
def mu(sm, gpu_available):
    return importlib.import_module("snappy_jl_amd.multi")


@pytest.fixture(scope="module")
def forms(gpu_available):
    """(name, stream argument, device argument, the torch stream to wait for)."""
    import torch
    side = torch.cuda.Stream(device=0)
    current = torch.cuda.current_stream(0)
    return [("none", None, None, current), ("stream", side, None, side), ("handle", side.cuda_stream, None, side),
            ("none, device given", None, 0, current), ("handle, device given", side.cuda_stream, 0, side)]


def _u8(data):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(data) or b"\0", np.uint8).copy()).to("cuda:0")


def _ints(values, dtype):
    import torch
    return torch.from_numpy(np.array(values, dtype=np.int64).astype(dtype)).to("cuda:0")


def _zeros(n, dtype):
    import torch
    return torch.zeros(max(n, 1), dtype=dtype, device="cuda:0")


def _every_form(forms, reset, call, read):
    """read() after reset() and call(stream, device) on every form: {form name: result}.  The
    device is idle before the call (reset's fills run on another stream than the call may), and the
    form's stream is synchronised behind it."""
    import torch
    got = {}
    for name, stream, device, wait in forms:
        reset()
        torch.cuda.synchronize()
        call(stream, device)
        wait.synchronize()
        got[name] = read()
    return got


def test_raw_compress_batch_device(sm, oracle, forms):
    import torch
    host = sm.compress_batch(BLOCKS, mode="fast")
    assert [oracle.uncompress(s) for s in host] == BLOCKS
    buf, in_off, in_len = sm.pack_blocks(BLOCKS)
    out_off, caps = sm.slot_offsets(in_len)
    d_in, d_in_off, d_in_len = _u8(buf.tobytes()), _ints(in_off, np.int64), _ints(in_len, np.int32)
    d_out_off = _ints(out_off, np.int64)
    d_out, d_out_len = _zeros(int(out_off[-1] + caps[-1]), torch.uint8), _zeros(len(BLOCKS), torch.int32)

    def reset():
        d_out.zero_()
        d_out_len.fill_(-1)

    def call(stream, device):
        sm.compress_batch_device(d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_len, mode="fast", stream=stream,
                                 device=device)

    def read():
        out = d_out.cpu().numpy()
        return [out[int(o):int(o) + int(n)].tobytes() for o, n in zip(out_off, d_out_len.cpu().numpy().view(np.uint32))]

    for name, streams in _every_form(forms, reset, call, read).items():
        assert streams == host, name


def test_raw_validate_batch_device(sm, forms):
    import torch
    streams = sm.compress_batch(BLOCKS, mode="fast")
    assert [sm.validate(s) for s in streams] == [0, 0, 0]
    buf, in_off, in_len = sm.pack_blocks(streams)
    d_in, d_in_off, d_in_len = _u8(buf.tobytes()), _ints(in_off, np.int64), _ints(in_len, np.int32)
    d_status = _zeros(len(streams), torch.int32)

    def call(stream, device):
        sm.validate_batch_device(d_in, d_in_off, d_in_len, d_status, stream=stream, device=device)

    for name, status in _every_form(forms, lambda: d_status.fill_(-1), call, lambda: d_status.cpu().tolist()).items():
        assert status == [0, 0, 0], name


def test_framing_compress_framed_device(fr, oracle, forms):
    import torch
    host = fr.compress_framed(FRAMED_INPUT, mode="fast")
    assert FR.decode(host, oracle) == FRAMED_INPUT and len(list(FR.walk(host))) == 2
    d_in, d_out = _u8(FRAMED_INPUT), _zeros(fr.max_framed_length(len(FRAMED_INPUT)), torch.uint8)
    d_len, d_status = _zeros(1, torch.int64), _zeros(1, torch.int32)

    def reset():
        d_out.zero_()
        d_len.fill_(-1)
        d_status.fill_(77)

    def call(stream, device):
        fr.compress_framed_device(d_in, d_out, d_len, d_status, mode="fast", stream=stream, device=device)

    def read():
        return int(d_status.item()), d_out.cpu().numpy()[:int(d_len.item())].tobytes()

    for name, result in _every_form(forms, reset, call, read).items():
        assert result == (0, host), name


def test_streams_compress_streams_device(sm, mu, oracle, forms):
    import torch
    host, (first, pos) = mu.compress_streams(STREAM_INPUTS, mode="fast", return_index=True)
    assert [oracle.uncompress(s) for s in host] == STREAM_INPUTS
    assert first.tolist() == mu.frag_first_of([len(d) for d in STREAM_INPUTS]).tolist() == [0, 1, 3]
    buf, in_off, in_len = sm.pack_blocks(STREAM_INPUTS)
    out_off, caps = sm.slot_offsets(in_len)
    n, m = len(STREAM_INPUTS), int(first[-1])
    d_in, d_in_off, d_in_len = _u8(buf.tobytes()), _ints(in_off, np.int64), _ints(in_len, np.int32)
    d_out_off = _ints(out_off, np.int64)
    d_out, d_out_len = _zeros(int(out_off[-1] + caps[-1]), torch.uint8), _zeros(n, torch.int32)
    d_status, d_first, d_pos = _zeros(n, torch.int32), _zeros(n + 1, torch.int32), _zeros(m, torch.int32)

    def reset():
        for t, fill in ((d_out, 0), (d_out_len, -1), (d_status, 77), (d_first, -1), (d_pos, -1)):
            t.fill_(fill)

    def call(stream, device):
        mu.compress_streams_device(d_in, d_in_off, d_in_len, m, d_out, d_out_off, d_out_len, d_status, d_first, d_pos,
                                   mode="fast", stream=stream, device=device)

    def read():
        out = d_out.cpu().numpy()
        lens = d_out_len.cpu().numpy().view(np.uint32)
        return (d_status.cpu().tolist(), [out[int(o):int(o) + int(k)].tobytes() for o, k in zip(out_off, lens)],
                d_first.cpu().tolist(), d_pos.cpu().tolist())

    for name, result in _every_form(forms, reset, call, read).items():
        assert result == ([0, 0], host, first.tolist(), pos.tolist()), name
