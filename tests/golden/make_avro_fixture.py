"""The recipe of tests/golden/avro/: four Avro object container files with avro.codec = snappy,
written by the plain-Python reference (tests/avro_ref.py) with payloads from pyarrow's libsnappy and
checksums from zlib.crc32, and avro_fixture.json with what the reference reads back from them.  No
Avro library wrote or read them: none is at hand.  The records are Avro binary (a long id, a string
source, a string line) of the text of tests/golden/testdata/alice29.txt.  The files are data only.
The tests read the committed files; this script needs pyarrow and is run by hand:

    python tests/golden/make_avro_fixture.py

    blocks_64k.avro    a schema of a few KiB, blocks of about 64,000 bytes (Java's default sync interval)
    small_blocks.avro  300 tiny blocks, counts on both sides of 64 (one-byte and two-byte longs)
    bigblock.avro      one block of about 200,000 bytes: it decodes by fragments
    meta_forms.avro    the metadata map in its negative-count form with a byte size, keys before and
                       after avro.codec, and a second map block
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import avro_ref as R  # noqa: E402

FIELDS = [("id", "long", "The line's number in the source text, from 0."),
          ("source", "string", "The name of the text the line comes from."),
          ("line", "string", "The line itself, without its line end.")]


def schema(doc_repeat):
    """A record schema; its doc strings are repeated to give the header its size."""
    fields = [{"name": n, "type": t, "doc": " ".join([d] * doc_repeat)} for n, t, d in FIELDS]
    extra = [{"name": "unused_%02d" % i, "type": ["null", "string"], "default": None,
              "doc": "A field no record of the fixture carries a value for: it pads the schema."} for i in range(doc_repeat)]
    return json.dumps({"type": "record", "name": "Line", "namespace": "fixture.snappy", "doc": "A line of text.",
                       "fields": fields + extra}, indent=1).encode()


def records():
    with open(os.path.join(HERE, "testdata", "alice29.txt"), "rb") as f:
        lines = f.read().split(b"\n")
    for i, line in enumerate(lines):
        line = line.rstrip(b"\r")
        yield R.encode_long(i) + R.encode_bytes(b"alice29.txt") + R.encode_bytes(line)


def blocks_of(limit, max_bytes):
    """The records in blocks of at least `limit` bytes, up to max_bytes in all: (blocks, counts)."""
    blocks, counts, cur, n, total = [], [], b"", 0, 0
    for rec in records():
        if total + len(cur) + len(rec) > max_bytes:
            break
        cur += rec
        n += 1
        if len(cur) >= limit:
            blocks.append(cur)
            counts.append(n)
            total += len(cur)
            cur, n = b"", 0
    if cur:
        blocks.append(cur)
        counts.append(n)
    return blocks, counts


def small_blocks():
    """300 blocks of 0 to 7 records, every tenth of 60 to 70: their counts and their sizes fall on
    both sides of 64."""
    recs = list(records())
    rng = np.random.default_rng(20240915)
    sizes = [0, 1, 63, 64, 65, 2] + [int(rng.integers(60, 71)) if i % 10 == 0 else int(rng.integers(0, 8)) for i in range(294)]
    blocks, counts, at = [], [], 0
    for k in sizes:
        assert at + k <= len(recs)
        blocks.append(b"".join(recs[at:at + k]))
        counts.append(k)
        at += k
    return blocks, counts


def describe(data, uncompress):
    status, decoded, w = R.read(data, uncompress)
    assert status == 0, status
    return {"file_bytes": len(data), "header_length": w.header_len, "sync": w.sync.hex(), "blocks": len(w.blocks),
            "objects": w.objects, "decoded_bytes": w.total, "largest_block": max(b.ulen for b in w.blocks),
            "one_byte_counts": sum(b.count < 64 for b in w.blocks), "two_byte_counts": sum(b.count >= 64 for b in w.blocks),
            "sha256": hashlib.sha256(decoded).hexdigest()}


def main():
    out_dir = os.path.join(HERE, "avro")
    os.makedirs(out_dir, exist_ok=True)
    compress, uncompress = R.libsnappy()
    rng = np.random.default_rng(20240914)
    syncs = [rng.integers(0, 256, 16, dtype=np.uint8).tobytes() for _ in range(4)]
    files = {}
    blocks, counts = blocks_of(64000, 260000)
    files["blocks_64k.avro"] = R.write(blocks, counts, schema(12), syncs[0], compress)
    blocks, counts = small_blocks()
    files["small_blocks.avro"] = R.write(blocks, counts, schema(1), syncs[1], compress)
    blocks, counts = blocks_of(200000, 200000 + 64000)
    files["bigblock.avro"] = R.write(blocks[:1], counts[:1], schema(1), syncs[2], compress)
    blocks, counts = blocks_of(3000, 10000)
    maps = [([(b"fixture.before", b"a key in front of the codec"), (b"avro.codec", b"null"), (b"avro.schema", schema(1))], True),
            ([(b"avro.codec", b"snappy"), (b"fixture.after", b"")], False),
            ([(b"fixture.last", bytes(range(256)))], True)]
    files["meta_forms.avro"] = R.header_maps(maps, syncs[3]) + R.write_blocks(blocks, counts, syncs[3], compress)
    record = {"writer": "tests/avro_ref.py over pyarrow's libsnappy and zlib.crc32", "files": {}}
    for name, data in files.items():
        assert len(data) < 200 * 1024, (name, len(data))
        with open(os.path.join(out_dir, name), "wb") as f:
            f.write(data)
        record["files"][name] = describe(data, uncompress)
    with open(os.path.join(out_dir, "avro_fixture.json"), "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(record, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
