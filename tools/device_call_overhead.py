"""Host time of the Python side of one compress_batch_device call: the wrapper, the argument checks
of device_caller, the stream lookup and the ctypes marshalling, with the library replaced by a
recorder that returns at once (no kernel is launched, nothing is synchronised).

    python tools/device_call_overhead.py [PACKAGE_DIR ...]

Each PACKAGE_DIR is a snappy.jl_amd directory (default: this tree's); give a second tree's to
compare.  The trees are timed in alternation, `--rounds` rounds of `--calls` calls each, and the
median round of each is printed as one JSON line.  Needs a GPU (the tensors are CUDA tensors)."""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Recorder:
    def __getattr__(self, name):
        value = 0xC0DE if name.endswith("_ctx_create") else 0
        function = lambda *args: value
        setattr(self, name, function)
        return function


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(path, "__init__.py"), submodule_search_locations=[path])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    mod._lib = Recorder()
    return mod


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("packages", nargs="*", default=[os.path.join(ROOT, "snappy.jl_amd")])
    ap.add_argument("--rounds", type=int, default=31)
    ap.add_argument("--calls", type=int, default=20000)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    mods = [load(os.path.abspath(p), "overhead_pkg_%d" % k) for k, p in enumerate(a.packages)]
    z = lambda n, dtype: torch.zeros(n, dtype=dtype, device=dev)
    args = (z(8, torch.uint8), z(2, torch.int64), z(2, torch.int32), z(96, torch.uint8), z(2, torch.int64), z(2, torch.int32))
    rounds = [[] for _ in mods]
    for r in range(a.rounds + 1):  # (the first round warms up and is dropped)
        for k, mod in enumerate(mods):
            call = mod.compress_batch_device
            t0 = time.perf_counter()
            for _ in range(a.calls):
                call(*args)
            dt = time.perf_counter() - t0
            if r:
                rounds[k].append(dt / a.calls * 1e6)
    for p, us in zip(a.packages, rounds):
        print(json.dumps({"package": p, "us_per_call_median": round(statistics.median(us), 3), "min": round(min(us), 3),
                          "max": round(max(us), 3), "rounds": a.rounds, "calls": a.calls}))


if __name__ == "__main__":
    main()
