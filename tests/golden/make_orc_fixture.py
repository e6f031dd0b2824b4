"""The recipe of tests/golden/orc/: two ORC files written by pyarrow (the Apache ORC C++ writer) with
compression="snappy", at compression block sizes 65536 and 262144, and orc_fixture.json with what
the plain-Python reference (tests/orc_ref.py) over libsnappy reads from them.  The table: 4,000 rows
of an int64 counter, a repetitive string and 24 random bytes, from a seeded generator.  The tests
read the committed files only; this script needs pyarrow and libsnappy and is run by hand:

    python tests/golden/make_orc_fixture.py
"""
import ctypes
import ctypes.util
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import orc_ref as R  # noqa: E402

ROWS = 4000
COLUMNS = ("counter", "label", "payload")
FILES = {"snappy_64k.orc": 65536, "snappy_256k.orc": 262144}


def table():
    import pyarrow as pa
    rng = np.random.default_rng(20240611)
    blobs = rng.integers(0, 256, (ROWS, 24), dtype=np.uint8)
    return pa.table({
        COLUMNS[0]: pa.array(np.arange(ROWS, dtype=np.int64)),
        COLUMNS[1]: pa.array(["row %d of the fixture: the quick brown fox" % (i % 7) for i in range(ROWS)]),
        COLUMNS[2]: pa.array([b.tobytes() for b in blobs], type=pa.binary()),
    })


def libsnappy_uncompress():
    conda = "/opt/conda/lib/libsnappy.so.1"  # (where tests/conftest.py looks for it)
    L = ctypes.CDLL(conda if os.path.exists(conda) else ctypes.util.find_library("snappy") or "libsnappy.so.1")

    def uncompress(x):
        n = ctypes.c_size_t(0)
        if L.snappy_uncompressed_length(x, ctypes.c_size_t(len(x)), ctypes.byref(n)) != 0:
            return 1, None
        out = ctypes.create_string_buffer(max(n.value, 1))
        if L.snappy_uncompress(x, ctypes.c_size_t(len(x)), out, ctypes.byref(n)) != 0:
            return 1, None
        return 0, out.raw[:n.value]

    return uncompress


def describe(data, uncompress):
    ps_len, block_size = R.postscript(data)
    body = R.file_streams(data)
    status, chunks, total = R.walk(body, block_size)
    assert status == 0
    decoded = R.decode(body, block_size, uncompress)
    assert len(decoded) == total
    return {"file_bytes": len(data), "postscript_length": ps_len, "block_size": block_size, "chunks": len(chunks),
            "stored_chunks": sum(c.original for c in chunks), "decoded_bytes": total,
            "largest_chunk": max(c.ulen for c in chunks), "sha256": hashlib.sha256(decoded).hexdigest()}


def main():
    import pyarrow.orc as po
    out_dir = os.path.join(HERE, "orc")
    os.makedirs(out_dir, exist_ok=True)
    uncompress = libsnappy_uncompress()
    record = {"columns": list(COLUMNS), "rows": ROWS, "files": {}}
    for name, block_size in FILES.items():
        path = os.path.join(out_dir, name)
        po.write_table(table(), path, compression="snappy", compression_block_size=block_size)
        with open(path, "rb") as f:
            data = f.read()
        record["files"][name] = describe(data, uncompress)
        assert record["files"][name]["block_size"] == block_size
    with open(os.path.join(out_dir, "orc_fixture.json"), "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(record, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
