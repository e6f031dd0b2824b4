"""The recipe of tests/golden/table/: four LevelDB table files written by the plain-Python reference
(tests/table_ref.py) with payloads from pyarrow's libsnappy and its own CRC-32C, and
table_fixture.json with their SHA-256s and the handles the reference reads back from them.  No
LevelDB wrote or read them: none is at hand.  The data blocks are real blocks (prefix-compressed
entries, restart interval 16) whose values are lines of tests/golden/testdata/alice29.txt or random
bytes.  The files are data only.  The tests read the committed files; this script needs pyarrow and
is run by hand:

    python tests/golden/make_table_fixture.py

    mixed.ldb     data blocks of about 4 KiB, text and random by turns, so both block types occur;
                  the index block is compressed
    bigblock.ldb  one data block of about 200 KiB decoded: it decodes by fragments
    bigindex.ldb  4,500 tiny data blocks under 24-byte keys: the decoded index exceeds 64 KiB and is
                  stored compressed (type 1)
    empty.ldb     no data blocks
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import avro_ref  # noqa: E402  (libsnappy())
import table_ref as R  # noqa: E402


def lines():
    with open(os.path.join(HERE, "testdata", "alice29.txt"), "rb") as f:
        return [x.rstrip(b"\r") for x in f.read().split(b"\n")]


def key(i):
    return b"fixture/key/%012d" % i  # 24 bytes


def blocks_of(values, limit, start=0):
    """Blocks of at least `limit` bytes of entries key(i) -> values[i]: (contents, separator keys)."""
    blocks, keys, cur, i = [], [], [], start
    size = 0
    for v in values:
        cur.append((key(i), v))
        size += 30 + len(v)
        i += 1
        if size >= limit:
            blocks.append(R.build_block(cur))
            keys.append(cur[-1][0])
            cur, size = [], 0
    if cur:
        blocks.append(R.build_block(cur))
        keys.append(cur[-1][0])
    return blocks, keys


def describe(data, uncompress):
    p = R.plan(data, uncompress)
    assert p.status == 0, p.status
    _, index = R.read_footer(data)
    return {"file_bytes": len(data), "sha256_file": hashlib.sha256(data).hexdigest(),
            "sha256_decoded": hashlib.sha256(p.decoded).hexdigest(), "decoded_bytes": p.out_len, "blocks": len(p.handles),
            "index_handle": list(index), "index_type": data[index[0] + index[1]], "index_bytes": R.block_head(data, index)[1],
            "types": [data[o + s] for o, s in p.handles][:64], "handles": [list(h) for h in p.handles][:64],
            "handles_sha256": hashlib.sha256(json.dumps([list(h) for h in p.handles]).encode()).hexdigest()}


def main():
    out_dir = os.path.join(HERE, "table")
    os.makedirs(out_dir, exist_ok=True)
    compress, uncompress = avro_ref.libsnappy()
    rng = np.random.default_rng(20241021)
    text = lines()
    files = {}
    # mixed: runs of text lines and of random values, a block of about 4 KiB each
    values, at = [], 0
    for run in range(12):
        size = 0
        while size < 4096:
            v = text[at % len(text)] if run % 2 == 0 else rng.integers(0, 256, 100, dtype=np.uint8).tobytes()
            values.append(v)
            size += 30 + len(v)
            at += 1
    blocks, keys = blocks_of(values, 4096)
    files["mixed.ldb"] = R.write_table(blocks, keys, compress, compress_index=True)
    blocks, keys = blocks_of((text + text)[:4400], 1 << 30)
    files["bigblock.ldb"] = R.write_table(blocks, keys, compress, compress_index=False)
    blocks, keys = blocks_of([b"v%d" % (i % 7) for i in range(4500)], 1)
    files["bigindex.ldb"] = R.write_table(blocks, keys, compress, compress_index=True)
    files["empty.ldb"] = R.write_table([], [], compress)
    record = {"writer": "tests/table_ref.py over pyarrow's libsnappy", "files": {}}
    for name, data in files.items():
        assert len(data) < 400 * 1024, (name, len(data))
        with open(os.path.join(out_dir, name), "wb") as f:
            f.write(data)
        record["files"][name] = describe(data, uncompress)
    d = record["files"]
    assert set(d["mixed.ldb"]["types"]) == {0, 1} and d["mixed.ldb"]["index_type"] == 1
    assert d["bigblock.ldb"]["blocks"] == 1 and d["bigblock.ldb"]["decoded_bytes"] > 3 * 65536
    assert d["bigindex.ldb"]["blocks"] == 4500 and d["bigindex.ldb"]["index_bytes"] > 65536 and d["bigindex.ldb"]["index_type"] == 1
    assert d["empty.ldb"]["blocks"] == 0
    with open(os.path.join(out_dir, "table_fixture.json"), "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: {x: y for x, y in v.items() if x not in ("handles", "types")} for k, v in d.items()}, indent=1))


if __name__ == "__main__":
    main()
