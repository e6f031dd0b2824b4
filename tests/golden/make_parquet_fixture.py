"""The recipe of tests/golden/parquet/: four Parquet files written by pyarrow (parquet-cpp) with
compression="snappy", and parquet_fixture.json with what the plain-Python reference
(tests/parquet_ref.py) over libsnappy reads from their column chunks.  The chunks' byte ranges come
from pyarrow's own metadata.  The tests read the committed files only; this script needs pyarrow and
libsnappy and is run by hand:

    python tests/golden/make_parquet_fixture.py
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
import parquet_ref as R  # noqa: E402

ROWS = 4000


def base_columns():
    import pyarrow as pa
    rng = np.random.default_rng(20240923)
    blobs = rng.integers(0, 256, (ROWS, 24), dtype=np.uint8)
    return {
        "counter": pa.array(np.arange(ROWS, dtype=np.int64)),
        "label": pa.array(["row %d of the fixture: the quick brown fox" % (i % 7) for i in range(ROWS)]),
        "payload": pa.array([b.tobytes() for b in blobs], type=pa.binary()),
    }


def v1_table():
    import pyarrow as pa
    cols = base_columns()
    schema = pa.schema([pa.field("counter", pa.int64(), nullable=False), pa.field("label", pa.string()),
                        pa.field("payload", pa.binary())])
    return pa.table(cols, schema=schema)


def v2_table():
    import pyarrow as pa
    cols = base_columns()
    cols["maybe"] = pa.array([None if i % 5 == 0 else "value %d" % (i % 13) for i in range(ROWS)])
    cols["numbers"] = pa.array([None if i % 7 == 0 else list(range(i % 4)) for i in range(ROWS)], type=pa.list_(pa.int32()))
    fields = [pa.field("counter", pa.int64(), nullable=False), pa.field("label", pa.string()), pa.field("payload", pa.binary()),
              pa.field("maybe", pa.string()), pa.field("numbers", pa.list_(pa.int32()))]
    return pa.table(cols, schema=pa.schema(fields))


def big_table():
    import pyarrow as pa
    rng = np.random.default_rng(7)
    words = ["alpha", "beta", "gamma", "delta", "epsilon", "zeta", "eta", "theta"]
    return pa.table({"text": pa.array([" ".join(words[int(k)] for k in rng.integers(0, 8, 6)) for _ in range(5000)])})


FILES = {  # name: (table, write_table's arguments)
    "v1.parquet": (v1_table, dict(data_page_version="1.0", write_page_checksum=True, data_page_size=4096,
                                  use_dictionary=["label"])),
    "v2.parquet": (v2_table, dict(data_page_version="2.0", write_page_checksum=True, data_page_size=4096,
                                  use_dictionary=["label"])),
    "bigpage.parquet": (big_table, dict(data_page_version="1.0", write_page_checksum=False, data_page_size=1 << 22,
                                        use_dictionary=False)),
    "v1_nocrc.parquet": (v1_table, dict(data_page_version="1.0", write_page_checksum=False, data_page_size=16384,
                                        use_dictionary=["label"])),
}


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


def describe(path, data, uncompress):
    import pyarrow.parquet as pq
    meta = pq.ParquetFile(path).metadata
    chunks = []
    for g in range(meta.num_row_groups):
        for c in range(meta.num_columns):
            col = meta.row_group(g).column(c)
            assert col.compression == "SNAPPY"
            start = col.dictionary_page_offset if col.dictionary_page_offset is not None else col.data_page_offset
            raw = data[start:start + col.total_compressed_size]
            status, pages, total = R.walk(raw)
            assert status == 0 and total == col.total_uncompressed_size - sum(p.hdr_len for p in pages), (path, c)
            decoded = R.decode(raw, uncompress)
            assert len(decoded) == total
            chunks.append({"column": col.path_in_schema, "row_group": g, "offset": start, "length": len(raw),
                           "pages": len(pages), "page_types": [p.type for p in pages], "decoded_bytes": total,
                           "with_crc": sum(1 for p in pages if p.flags & R.HAS_CRC),
                           "levels": sum(p.levels for p in pages), "largest_page": max(p.usize for p in pages),
                           "sha256": hashlib.sha256(decoded).hexdigest()})
    return {"file_bytes": len(data), "chunks": chunks}


def main():
    import pyarrow.parquet as pq
    out_dir = os.path.join(HERE, "parquet")
    os.makedirs(out_dir, exist_ok=True)
    uncompress = libsnappy_uncompress()
    record = {"rows": ROWS, "files": {}}
    for name, (make, args) in FILES.items():
        path = os.path.join(out_dir, name)
        pq.write_table(make(), path, compression="snappy", **args)
        with open(path, "rb") as f:
            data = f.read()
        assert len(data) <= 300000, (name, len(data))
        record["files"][name] = describe(path, data, uncompress)
    with open(os.path.join(out_dir, "parquet_fixture.json"), "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    for name, rec in record["files"].items():
        print(name, rec["file_bytes"], [(c["column"], c["pages"], c["largest_page"], c["levels"]) for c in rec["chunks"]])


if __name__ == "__main__":
    main()
