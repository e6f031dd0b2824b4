"""The recipe of tests/golden/kafka/: four Kafka log segments written by the plain-Python reference
(tests/kafka_ref.py) with payloads from pyarrow's libsnappy and its own CRC-32C, and
kafka_fixture.json with their SHA-256s and, per batch, what the reference reads back from them.  No
Kafka broker or client wrote or read them: none is at hand.  The records payloads are lines of
tests/golden/testdata/alice29.txt (no record is framed: the library never looks inside).  The files
are data only.  The tests read the committed files; this script needs pyarrow and is run by hand:

    python tests/golden/make_kafka_fixture.py

    mixed.log          an uncompressed batch; a snappy-java batch with 32 KiB chunks over about 100 KB;
                       a bare raw-stream batch; a control batch and a transactional batch, stored; a
                       batch of no records, uncompressed and again with the snappy codec; a 1-byte
                       payload; a snappy-java batch that repeats its header between chunks
    bigbatch.log       a snappy-java batch of one chunk of 100,000 bytes and a raw batch of 150,000:
                       both decode by fragments
    small_batches.log  300 batches of about 200 bytes: stored, snappy-java, raw by turns
    empty.log          0 bytes
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import avro_ref  # noqa: E402  (libsnappy())
import kafka_ref as R  # noqa: E402


def describe(seg, uncompress):
    w = R.walk(seg)
    assert w.status == 0 and w.valid == len(seg)
    decoded = R.uncompress_segment(seg, uncompress)
    batches, out_off = [], 0
    for b in w.batches:
        assert b.status == 0
        records = R.records_of(seg, b, uncompress)
        assert len(records) == b.declared
        batches.append({"pos": b.pos, "length": b.length, "codec": b.codec, "kind": b.kind, "declared": b.declared,
                        "out_off": out_off, "sha256_records": hashlib.sha256(records).hexdigest()})
        out_off += R.HEADER + b.declared
    assert out_off == len(decoded)
    p = R.plan(seg)
    return {"file_bytes": len(seg), "sha256_file": hashlib.sha256(seg).hexdigest(), "decoded_bytes": len(decoded),
            "sha256_decoded": hashlib.sha256(decoded).hexdigest(), "chunks": p.chunks,
            "fragments": [p.x_fragments, p.r_fragments], "batches": batches}


def main():
    out_dir = os.path.join(HERE, "kafka")
    os.makedirs(out_dir, exist_ok=True)
    compress, uncompress = avro_ref.libsnappy()
    with open(os.path.join(HERE, "testdata", "alice29.txt"), "rb") as f:
        text = f.read()

    def tail(i, count):
        return R.tail_fields(count - 1 if count else 0, 1700000000000 + i, 1700000000000 + i + count, 4000 + i, i % 7, 10 * i, count)

    files = {}
    xerial = R.write_xerial(text[2000:102000], compress, 32768)
    repeated = R.write_xerial(text[20000:50000], compress, 10000, repeat_header=True)
    files["mixed.log"] = b"".join([
        R.write_batch(text[:2000], 0, 3, 0, tail(0, 20)),
        R.write_batch(xerial, 20, 3, 2, tail(1, 900)),
        R.write_batch(compress(text[102000:122000]), 920, 3, 2, tail(2, 150)),
        R.write_batch(text[300:310], 1070, 4, 0x20, tail(3, 1)),           # a control batch
        R.write_batch(text[400:1400], 1071, 4, 0x10, tail(4, 9)),          # a transactional batch
        R.write_batch(b"", 1080, 4, 0, tail(5, 0)),                        # no records
        R.write_batch(b"", 1080, 4, 2, tail(6, 0)),                        # no records, snappy
        R.write_batch(b"\x00", 1080, 5, 0x08, tail(7, 1)),                 # a 1-byte payload (timestamp type bit set)
        R.write_batch(repeated, 1081, 5, 2, tail(8, 300)),
    ])
    files["bigbatch.log"] = b"".join([
        R.write_batch(R.write_xerial(text[:100000], compress, 1 << 20), 0, 0, 2, tail(0, 1000)),
        R.write_batch(compress(text[:150000]), 1000, 0, 2, tail(1, 1500)),
    ])
    small, at = [], 0
    for i in range(300):
        n = 150 + (i * 37) % 100
        piece = text[at:at + n]
        at += n
        payload = piece if i % 3 == 0 else R.write_xerial(piece, compress, 32768) if i % 3 == 1 else compress(piece)
        small.append(R.write_batch(payload, 5 * i, 1, 0 if i % 3 == 0 else 2, tail(i, 5)))
    files["small_batches.log"] = b"".join(small)
    files["empty.log"] = b""
    meta = {}
    for name, seg in files.items():
        assert len(seg) <= 300000, (name, len(seg))
        with open(os.path.join(out_dir, name), "wb") as f:
            f.write(seg)
        meta[name] = describe(seg, uncompress)
        print(name, len(seg), "->", meta[name]["decoded_bytes"], len(meta[name]["batches"]), "batches")
    with open(os.path.join(out_dir, "kafka_fixture.json"), "w") as f:
        json.dump({"files": meta}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
