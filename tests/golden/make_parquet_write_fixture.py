"""The recipe of tests/golden/parquet_write/: the four tables of make_parquet_fixture.py written by
pyarrow (parquet-cpp) with compression="none" and otherwise the same arguments -- column chunks in
the plain form the page encoder takes (include/snappy_mi355x_parquet_write.h) -- and
parquet_write_fixture.json with what the plain-Python encode walk (tests/parquet_write_ref.py) reads
from them.  The chunks' byte ranges come from pyarrow's own metadata.  The tests read the committed
files only; this script needs pyarrow and is run by hand:

    python tests/golden/make_parquet_write_fixture.py
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import parquet_write_ref as W  # noqa: E402
from make_parquet_fixture import FILES, ROWS  # noqa: E402


def describe(path, data):
    import pyarrow.parquet as pq
    meta = pq.ParquetFile(path).metadata
    chunks = []
    for g in range(meta.num_row_groups):
        for c in range(meta.num_columns):
            col = meta.row_group(g).column(c)
            assert col.compression == "UNCOMPRESSED"
            start = col.dictionary_page_offset if col.dictionary_page_offset is not None else col.data_page_offset
            raw = data[start:start + col.total_compressed_size]
            status, pages, sites, total = W.walk(raw)
            assert status == 0 and total == col.total_uncompressed_size - sum(p.hdr_len for p in pages), (path, c)
            bodies = b"".join(raw[p.hdr_off + p.hdr_len:p.hdr_off + p.hdr_len + p.body_len] for p in pages)
            assert len(bodies) == total
            chunks.append({"column": col.path_in_schema, "row_group": g, "offset": start, "length": len(raw),
                           "pages": len(pages), "page_types": [p.type for p in pages],
                           "with_crc": sum(1 for p in pages if p.flags & W.R.HAS_CRC),
                           "levels": [p.levels for p in pages], "largest_page": max(p.usize for p in pages),
                           "sha256": hashlib.sha256(bodies).hexdigest()})
    return {"file_bytes": len(data), "chunks": chunks}


def main():
    import pyarrow.parquet as pq
    out_dir = os.path.join(HERE, "parquet_write")
    os.makedirs(out_dir, exist_ok=True)
    record = {"rows": ROWS, "files": {}}
    for name, (make, args) in FILES.items():
        path = os.path.join(out_dir, name)
        pq.write_table(make(), path, compression="none", **args)
        with open(path, "rb") as f:
            data = f.read()
        assert len(data) <= 300000, (name, len(data))
        record["files"][name] = describe(path, data)
    with open(os.path.join(out_dir, "parquet_write_fixture.json"), "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    for name, rec in record["files"].items():
        print(name, rec["file_bytes"], [(c["column"], c["pages"], c["largest_page"], sum(c["levels"])) for c in rec["chunks"]])


if __name__ == "__main__":
    main()
