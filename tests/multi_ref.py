"""The multi-stream library's contract in plain Python (test helper of test_multi_host.py and
test_multi_gpu.py): the length ladder, the index of a stream built on the CPU from the oracle's
fragments, the index rules of smm_uncompress_device, the decode model (fragment-wise oracle decode
when the stream is indexed and every fragment is OK, else the whole stream under the oracle), and
the seeded mutation cases.  Nothing here calls the library under test."""
import numpy as np

import streams as S
from conftest import read_testfile

BLOCK = 65536
SM_BUFFER_TOO_SMALL = 2
SM_ERR_INPUT_TOO_LARGE = 16
SM_ERR_VARINT = 18
SM_ERR_ARGUMENT = 33
LADDER = (0, 1, 65535, 65536, 65537, 131072, 131073, 196613)

_CACHE = {}


def frag_count(n):
    return (n + BLOCK - 1) // BLOCK


def max_compressed_length(n):
    return 32 + n + n // 6


def sources():
    """The five inputs every case is cut from: text, markup, a binary table, seeded random bytes
    (the screen's literal path) and zeros."""
    if "src" not in _CACHE:
        rnd = np.random.default_rng(2026).integers(0, 256, 200000, dtype=np.uint8).tobytes()
        _CACHE["src"] = [read_testfile("alice29.txt") * 2, read_testfile("html_x_4"), read_testfile("kppkn.gtb") * 2, rnd,
                         bytes(200000)]
    return _CACHE["src"]


def ladder_datas():
    """16 inputs, every ladder length twice, from sources that rotate (stream k starts at an address
    that is k mod 16 in the device tests)."""
    src = sources()
    return [src[k % 5][7 * k: 7 * k + LADDER[k % 8]] for k in range(16)]


def parse_varint(b):
    """(value, bytes) of the varint32 at b[0:], or None (src/varint.jl:12-37)."""
    v = 0
    for i in range(min(5, len(b))):
        c = b[i]
        if i < 4:
            v |= (c & 0x7F) << (7 * i)
            if c < 0x80:
                return v, i + 1
        elif c < 0x10:
            return v | (c << 28), 5
    return None


def cpu_index(data, oracle):
    """(stream, positions) of data as the reference compresses it, the fragments' offsets from the
    oracle's own fragment sizes."""
    stream = oracle.compress(data)
    hv = len(S.varint(len(data)))
    pos, at = [], hv
    for f in range(frag_count(len(data))):
        pos.append(at)
        at += len(oracle.compress_fragment(data[f * BLOCK:(f + 1) * BLOCK], len(data)))
    assert at == len(stream)
    return stream, pos


def first_ok(first, nstreams, max_fragments):
    first = [int(x) for x in first]
    return (len(first) == nstreams + 1 and first[0] == 0 and all(a <= b for a, b in zip(first, first[1:]))
            and first[-1] <= max_fragments)


def structural(stream, cap, entries):
    """The per-stream index rules: entries = the stream's positions.  (D, hv) when indexed, else None."""
    h = parse_varint(stream)
    if h is None:
        return None
    D, hv = h
    if not (BLOCK < D <= cap) or len(entries) != frag_count(D):
        return None
    e = [int(x) for x in entries]
    if e[0] != hv or any(a >= b for a, b in zip(e, e[1:])) or e[-1] >= len(stream):
        return None
    return D, hv


def model(stream, cap, entries, oracle):
    """(status, bytes or None, indexed) of one stream.  entries: its positions, or None when the
    call has no usable index."""
    if entries is not None:
        ok = structural(stream, cap, entries)
        if ok:
            D, _ = ok
            ends = [int(x) for x in entries[1:]] + [len(stream)]
            outs = []
            for f, (lo, hi) in enumerate(zip(entries, ends)):
                L = min(BLOCK, D - f * BLOCK)
                st, dec = oracle.uncompress_status(S.varint(L) + stream[int(lo):hi])
                if st != 0:
                    break
                outs.append(dec)
            else:
                return 0, b"".join(outs), True
    h = parse_varint(stream)
    if h is None:
        return SM_ERR_VARINT, None, False
    if h[0] > cap:
        return SM_BUFFER_TOO_SMALL, None, False
    st, dec = oracle.uncompress_status(stream)
    return st, (dec if st == 0 else None), False


def model_batch(strs, caps, first, pos, max_fragments, oracle):
    """[(status, bytes or None, indexed)] of a call; first / pos None: no index."""
    usable = first is not None and first_ok(first, len(strs), max_fragments)
    out = []
    for k, (s, c) in enumerate(zip(strs, caps)):
        entries = [int(x) for x in pos[int(first[k]):int(first[k + 1])]] if usable else None
        out.append(model(s, c, entries, oracle))
    return out


def foreign_stream(seed, target, max_off=100000):
    """A stream no block compressor writes: copies reach back across 64 KiB boundaries.  (stream,
    data, a syntactically valid index: the right count, evenly spaced positions)."""
    rng = np.random.default_rng(seed)
    s, e = S.build(S.random_ops(rng, target, max_off=max_off))
    hv = len(S.varint(len(e)))
    cnt = frag_count(len(e))
    pos = [hv + (len(s) - hv) * f // cnt for f in range(cnt)]
    return s, e, pos


FUZZ_SEED = 8642
FUZZ_N = 400
FUZZ_CAP = 300000  # a mutated header may declare anything: the room is the declared length up to this


def fuzz_cases(oracle):
    """[(stream, capacity, the base's positions)]: 400 seeded mutations of streams of 65,537 to
    200,000 input bytes, the kinds of tests/test_fragments_device.py fuzz_cases (byte flips,
    truncation, appended bytes, a flip plus tail trim, a wrong declared length, unmodified).  The
    index stays the base's own."""
    if "fuzz" in _CACHE:
        return _CACHE["fuzz"]
    src = sources()
    cuts = [(0, 150000), (1, 200000), (2, 180000), (3, 70001), (4, 100000), (0, 65537), (1, 131072)]
    bases = []
    for k, n in cuts:
        data = src[k][11:11 + n]
        bases.append(cpu_index(data, oracle) + (n,))
    for seed, target in ((31, 140000), (32, 190000)):
        s, e, pos = foreign_stream(seed, target)
        assert 65537 <= len(e) <= 200000
        bases.append((s, pos, len(e)))
    rng = np.random.default_rng(FUZZ_SEED)
    cases = []
    for i in range(FUZZ_N):
        stream, pos, decl = bases[i % len(bases)]
        hv = len(S.varint(decl))
        s = bytearray(stream)
        kind = int(rng.integers(0, 6))
        if kind == 0:  # 1-3 byte flips
            for _ in range(int(rng.integers(1, 4))):
                s[int(rng.integers(0, len(s)))] = int(rng.integers(0, 256))
        elif kind == 1:  # truncation
            s = s[: int(rng.integers(0, len(s)))]
        elif kind == 2:  # 1-5 appended bytes
            s += rng.integers(0, 256, int(rng.integers(1, 6)), dtype=np.uint8).tobytes()
        elif kind == 3:  # a flip plus tail trim
            s[int(rng.integers(0, len(s)))] = int(rng.integers(0, 256))
            s = s[: max(1, len(s) - int(rng.integers(0, 8)))]
        elif kind == 4:  # a wrong declared length
            s = bytearray(S.varint(max(decl + int(rng.choice([-17, -1, 1, 40, BLOCK])), 0))) + s[hv:]
        h = parse_varint(bytes(s))
        cases.append((bytes(s), min(h[0], FUZZ_CAP) if h else 0, pos))
    _CACHE["fuzz"] = cases
    return cases


def fuzz_index(cases):
    """(frag_first, frag_pos, max_fragments) of the cases' original indexes, as one call's arrays."""
    counts = [len(c[2]) for c in cases]
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    pos = np.array([p for c in cases for p in c[2]], np.uint32)
    return first, pos, int(first[-1])


def fuzz_model(oracle):
    if "fuzz_model" not in _CACHE:
        cases = fuzz_cases(oracle)
        first, pos, m = fuzz_index(cases)
        _CACHE["fuzz_model"] = model_batch([c[0] for c in cases], [c[1] for c in cases], first, pos, m, oracle)
    return _CACHE["fuzz_model"]
