"""In fast and dense mode the stream of a block is a function of the block's bytes and the mode
alone (snappy_mi355x.h on the parts rule: "The bytes and lengths do not depend on any of this").
Nothing else in the suite holds the compressor to that: round trips pass whatever valid stream
comes out.  Here every probe of a small catalogue is compressed once in a call of its own (nblk = 1,
input and slot on 16-byte boundaries): its canonical stream, which must decode to the probe under
the CPU oracle -- the only place where correctness rests on the oracle.  Every placement below must
then give exactly those bytes and that length, and leave everything outside the slots' documented
room (32 + n + n/6 + 5 bytes) as it was:

  A. every probe 16 times in one batch, copy k with its input at an address = k (mod 16) and its
     slot at 5k + 3 (mod 16) -- all 16 residues of both -- between gap bytes (0x00 before and 0xFF
     behind, swapped on odd k) that a read of a neighbour's bytes would bring into the stream;
  B. 2g + r blocks (g = the device's compute units): a round of one filler kind, then the probes, so
     each probe is parsed in the LDS its workgroup parsed the filler in, then r more probes (r = 1:
     16 parts, g/2: 2 parts, g/2 + 1: a third whole round); fillers: 64 KiB of text, of 0xFF, of
     random bytes (the screen takes them: the probe is the workgroup's first block), empty, and an
     oversize block (its length must come back as the error mark, its slot untouched); input
     residues 0 (the register prefetch for full blocks, the 16-byte loop for the others) and 9 (the
     byte loop);
  C. the other entry points: compress_batch, compress with the split parse on and off, and the
     fragment call with two table sizes (the stream without its varint);
  D. A and B (text filler) in reference mode against the oracle's compress: B has more blocks than
     compute units, so the reference kernel reads its blocks in place at every residue;
  E. input, slots, streams and decoded output at offsets beyond 4 GiB, in buffers that hold offset
     0 as well: a truncated offset lands in a canary region and shows;
  F. a call captured into a graph on a stream its context has never seen (no parts scratch: every
     block whole), replayed over rewritten inputs, then an eager call on that stream (parts).

The comparison (slot_diffs, canary_diffs) names probe, placement, mode, where in the placement and
the first differing byte; the CPU tests at the top check the layouts and that the comparison finds
one flipped byte, one length off by one and one byte written outside a slot."""
import collections
import functools

import numpy as np
import pytest

from test_batch_parts_gpu import BLOCK, MAXC, canary, fallback_block, random_block, rule, text_block

gpu = pytest.mark.gpu

MODES = ("fast", "dense")
LENGTHS = (0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3839, 3840, 3841, 4097, 20001,
           65535, 65536)
KINDS = ("text", "abc3", "period7", "const", "planted", "texttail", "random")
NOT_A_BLOCK = 0xFFFFFFFF
OVERSIZE = -1  # a block index of the layouts: no probe, 65,537 bytes of text
COPIES = 16


# ---- 1. the probes ------------------------------------------------------------------------------

def make_block(kind, n, seed):
    rng = np.random.default_rng([0x91ACE, seed, n])
    if kind == "text":  # a window of lcet10.txt
        return text_block(seed % 40, n)
    if kind == "abc3":
        return (rng.integers(0, 3, n, dtype=np.uint8) + 97).tobytes()
    if kind == "period7":
        return np.resize(rng.permutation(256)[:7].astype(np.uint8), n).tobytes()
    if kind == "const":
        return bytes([0xFF if n == BLOCK else 0x00 if n == BLOCK - 1 else 0x41 + seed % 26]) * n
    if kind == "planted":  # random bytes with planted copies at distances 1..2000 (test_gpu_fuzz's last kind)
        b = rng.integers(0, 256, n, dtype=np.uint8)
        for _ in range(min(40, 1 + n // 64)):
            L, d = int(rng.integers(4, 300)), int(rng.integers(1, 2000))
            p = int(rng.integers(0, max(1, n - L)))
            for k in range(min(L, n - p)):
                if p + k - d >= 0:
                    b[p + k] = b[p + k - d]
        return b.tobytes()
    if kind == "texttail":  # text, then a random tail
        cut = n - n // 3
        return text_block(seed % 40 + 1, n)[:cut] + rng.integers(0, 256, n - cut, dtype=np.uint8).tobytes()
    if kind == "random":  # (a full block of it is the screen's literal)
        return random_block() if n == BLOCK else rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    if kind == "fallback":  # passes the screen, parses to more than one literal
        return fallback_block()[:n]
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def catalogue():
    """[(name, bytes)]: every length below 64 KiB with one kind, the lengths from 1,023 on with a
    second, a few small compressible ones, and the two largest lengths with most kinds."""
    spec = [(KINDS[i % 7], n) for i, n in enumerate(LENGTHS[:-2])]
    spec += [(KINDS[(i + 3) % 7], n) for i, n in enumerate(LENGTHS[:-2]) if n >= 1023]
    spec += [("const", 255), ("period7", 256), ("abc3", 257), ("period7", 20001)]
    spec += [(k, BLOCK - 1) for k in ("text", "const", "random", "fallback")]
    spec += [(k, BLOCK) for k in ("text", "const", "random", "fallback", "abc3", "period7", "planted", "texttail")]
    out = [("%s-%d" % (k, n), make_block(k, n, i)) for i, (k, n) in enumerate(spec)]
    assert all(len(b) == n for (_, b), (_, n) in zip(out, spec))
    return out


NAMES = [name for name, _ in catalogue()]
TEXT, FF, RANDOM, EMPTY = (NAMES.index(x) for x in ("text-65536", "const-65536", "random-65536", "text-0"))
FILLERS = {"text": TEXT, "ff": FF, "random": RANDOM, "empty": EMPTY, "oversize": OVERSIZE}


def probe(i):
    return text_block(77, BLOCK + 1) if i == OVERSIZE else catalogue()[i][1]


def room_of(n, header=True):
    """A slot's documented room: sm_max_compressed_length(n) and the header."""
    return 0 if n > BLOCK else 32 + n + n // 6 + (5 if header else 0)


# ---- 2. layouts (plain Python, checked on the CPU) ----------------------------------------------

# One block of a call: which probe (an index of the catalogue, or OVERSIZE), where in the
# placement (the report's words), input and slot offsets, and the gap bytes that are this block's
# own before and behind its input.
Place = collections.namedtuple("Place", "probe where in_off out_off before behind")
Layout = collections.namedtuple("Layout", "places in_size out_size")


def lay_out(blocks, in_res, out_res, first_gap=17):
    """blocks: [(probe, where)]; in_res(j), out_res(j): block j's residues (mod 16).  Inputs lie
    behind one another, each between gaps of its own of 17 to 32 bytes before it and 17 behind it
    (more than any 16-byte read reaches); slots behind one another with their whole room and at
    least one byte between two."""
    places, ci, co = [], 0, 16
    for j, (p, where) in enumerate(blocks):
        n = len(probe(p))
        start = ci
        ci += first_gap
        ci += (in_res(j) - ci) % 16
        co += 1 + (out_res(j) - co - 1) % 16
        places.append(Place(p, where, ci, co, ci - start, 17))
        ci += n + 17
        co += room_of(min(n, BLOCK))  # (an oversize block keeps a slot's space: nothing may be written there)
    return Layout(places, ci + 16, co + 64)


def residue_layout():
    """A: copy k of every probe, k-major."""
    blocks = [(p, "copy k=%d" % k) for k in range(COPIES) for p in range(len(NAMES))]
    return lay_out(blocks, lambda j: j // len(NAMES), lambda j: (5 * (j // len(NAMES)) + 3) % 16)


B_CASES = [(f, res) for f in ("text", "ff", "random", "empty", "oversize") for res in (0, 9)]
B_ROUNDS = ("1", "g/2", "g/2+1")
B_NAMES = ["%s-in%d" % c for c in B_CASES]


def rounds_of(case, g):
    """B: the case's r -- the three values go round over the ten cases."""
    return {"1": 1, "g/2": g // 2, "g/2+1": g // 2 + 1}[B_ROUNDS[B_CASES.index(case) % 3]]


def rounds_layout(case, g):
    """B: g fillers, g probes (cycled from the catalogue's start), r probes (cycled from its middle)."""
    filler, res = case
    P, r = len(NAMES), rounds_of(case, g)
    blocks = [(FILLERS[filler], "filler %d" % j) for j in range(g)]
    blocks += [(j % P, "round 2, block g+%d" % j) for j in range(g)]
    blocks += [((j + P // 2) % P, "round 3, block 2g+%d" % j) for j in range(r)]
    return lay_out(blocks, lambda j: res, lambda j: res)


def fill_input(layout):
    """The host copy of d_in: every block's bytes between its own gap bytes (gap_bytes)."""
    buf = np.zeros(layout.in_size, np.uint8)
    for j, pl in enumerate(layout.places):
        b = np.frombuffer(probe(pl.probe), np.uint8)
        lo, hi = gap_bytes(pl, j)
        buf[pl.in_off - pl.before:pl.in_off] = lo
        buf[pl.in_off:pl.in_off + b.size] = b
        buf[pl.in_off + b.size:pl.in_off + b.size + pl.behind] = hi
    return buf


def gap_bytes(pl, j):
    """(the byte before, the byte behind) block j: swapped on odd copies in A, on odd blocks elsewhere."""
    odd = int(pl.where.rsplit("=", 1)[1]) & 1 if pl.where.startswith("copy k=") else j & 1
    return (0xFF, 0x00) if odd else (0x00, 0xFF)


# ---- 3. the comparison --------------------------------------------------------------------------

class Diff(collections.namedtuple("Diff", "placement mode probe where what offset")):
    def __str__(self):
        at = "" if self.offset is None else ", first differing byte at offset %d" % self.offset
        return "%s %s: probe %s (%s): %s%s" % (self.placement, self.mode, self.probe, self.where, self.what, at)


def first_diff(a, b):
    k = min(a.size, b.size)
    bad = np.nonzero(a[:k] != b[:k])[0]
    return int(bad[0]) if bad.size else None


def slot_diffs(placement, mode, layout, want, out, lens, base=0, header=True):
    """Every block of the layout against its canonical stream: want[probe index] -> bytes (the
    stream; the error mark for OVERSIZE), out = the output buffer from offset `base` on, lens =
    d_out_len as unsigned.  One Diff per block whose length or bytes differ."""
    diffs = []
    for pl, got_len in zip(layout.places, lens):
        name = "oversize" if pl.probe == OVERSIZE else NAMES[pl.probe]
        got_len, off = int(got_len), pl.out_off - base
        if pl.probe == OVERSIZE:
            if got_len != NOT_A_BLOCK:
                diffs.append(Diff(placement, mode, name, pl.where, "length %#x, not the error mark" % got_len, None))
            continue
        w = np.frombuffer(want[pl.probe], np.uint8)
        slot = out[off:off + min(max(got_len, w.size), room_of(len(probe(pl.probe)), header))]
        at = first_diff(slot, w)
        if got_len != w.size:
            diffs.append(Diff(placement, mode, name, pl.where, "length %d, canonical %d" % (got_len, w.size), at))
        elif at is not None:
            diffs.append(Diff(placement, mode, name, pl.where, "bytes differ", at))
    return diffs


def canary_diffs(placement, mode, layout, out, fill, base=0, header=True):
    """Bytes of `out` outside every slot's documented room that are not `fill`'s: one Diff per run's
    neighbour slot (the slot that starts last before the byte)."""
    keep = np.ones(out.size, bool)
    for pl in layout.places:
        keep[pl.out_off - base:pl.out_off - base + room_of(len(probe(pl.probe)), header)] = False
    bad = np.nonzero(keep & (out != fill))[0]
    diffs, starts = [], np.array([pl.out_off - base for pl in layout.places])
    for at in bad[:1].tolist() + bad[1:][np.diff(bad) > 1][:15].tolist():
        j = max(int(np.searchsorted(starts, at, "right")) - 1, 0)
        pl = layout.places[j]
        name = "oversize" if pl.probe == OVERSIZE else NAMES[pl.probe]
        diffs.append(Diff(placement, mode, name, pl.where, "a byte outside the slots' room was written", at - starts[j]))
    return diffs


def report(diffs):
    assert not diffs, "%d differ:\n%s" % (len(diffs), "\n".join(str(d) for d in diffs[:24]))


# ---- CPU ----------------------------------------------------------------------------------------

def test_catalogue():
    """About 40 probes, every length, every kind, the two largest lengths with text, constant,
    random and fallback; fixed seeds (the same bytes on every build of the list)."""
    assert 38 <= len(NAMES) <= 48 and len(set(NAMES)) == len(NAMES)
    assert {len(b) for _, b in catalogue()} == set(LENGTHS)
    kinds = {n.split("-")[0] for n in NAMES}
    assert kinds == set(KINDS) | {"fallback"}
    for n in (BLOCK - 1, BLOCK):
        assert {"%s-%d" % (k, n) for k in ("text", "const", "random", "fallback")} <= set(NAMES)
    assert probe(FF) == b"\xff" * BLOCK and probe(EMPTY) == b"" and probe(RANDOM) == random_block()
    assert len(probe(OVERSIZE)) == BLOCK + 1
    catalogue.cache_clear()
    again = catalogue()
    assert [n for n, _ in again] == NAMES and all(a[1] == probe(i) for i, a in enumerate(again))


def check_layout(layout, in_res, out_res):
    """Residues as asked, every block between gap bytes of its own (at least one each side) that
    belong to no other block, no two slots' rooms overlapping, everything inside the buffers."""
    owner = np.zeros(layout.in_size, np.int32)
    end_out = 16
    for j, pl in enumerate(layout.places):
        n = len(probe(pl.probe))
        assert pl.in_off % 16 == in_res(j) and pl.out_off % 16 == out_res(j), (j, pl)
        assert pl.before >= 1 and pl.behind >= 1
        lo, hi = pl.in_off - pl.before, pl.in_off + n + pl.behind
        assert 0 <= lo and hi + 16 <= layout.in_size
        assert not owner[lo:hi].any(), (j, pl)
        owner[lo:hi] = j + 1
        assert pl.out_off > end_out, (j, pl)  # (a byte of canary between two rooms)
        end_out = pl.out_off + room_of(min(n, BLOCK))
    assert end_out + 16 <= layout.out_size


def test_residue_layout():
    """A: every probe at all 16 input residues and all 16 slot residues, gaps that differ between
    neighbouring copies, no overlap."""
    lay = residue_layout()
    P = len(NAMES)
    assert len(lay.places) == COPIES * P
    check_layout(lay, lambda j: j // P, lambda j: (5 * (j // P) + 3) % 16)
    for p in range(P):
        mine = [pl for pl in lay.places if pl.probe == p]
        assert sorted(pl.in_off % 16 for pl in mine) == list(range(16))
        assert sorted(pl.out_off % 16 for pl in mine) == list(range(16))
    buf = fill_input(lay)
    for j, pl in enumerate(lay.places):
        n, k = len(probe(pl.probe)), j // P
        lo, hi = (0xFF, 0x00) if k & 1 else (0x00, 0xFF)
        assert pl.where == "copy k=%d" % k
        assert (buf[pl.in_off - pl.before:pl.in_off] == lo).all() and (buf[pl.in_off + n:pl.in_off + n + 17] == hi).all()
        assert buf[pl.in_off:pl.in_off + n].tobytes() == probe(pl.probe)


def test_rounds_layout():
    """B: the case names (module constants: they do not depend on g) are unique; on a few grid sizes
    every filler kind meets both residues, every r meets both residues, the rule gives 16 parts, 2
    parts and none, and every probe sits one grid behind a filler."""
    assert len(set(B_NAMES)) == len(B_NAMES) == 10
    assert {f for f, _ in B_CASES} == set(FILLERS) and all({(f, 0), (f, 9)} <= set(B_CASES) for f in FILLERS)
    for g in (104, 256, 304):
        seen = set()
        for case in B_CASES:
            lay = rounds_layout(case, g)
            r = rounds_of(case, g)
            seen.add((r, case[1]))
            assert len(lay.places) == 2 * g + r
            check_layout(lay, lambda j: case[1], lambda j: case[1])
            assert all(pl.probe == FILLERS[case[0]] for pl in lay.places[:g])
            assert {pl.probe for pl in lay.places[g:2 * g]} == set(range(len(NAMES)))  # every probe behind a filler
            assert rule(2 * g + r, g) == {1: (1, 16), g // 2: (g // 2, 2), g // 2 + 1: (0, 0)}[r]
        assert seen == {(r, res) for r in (1, g // 2, g // 2 + 1) for res in (0, 9)}
        assert {rounds_of(c, g) for c in B_CASES if c[0] == "text"} == {1, g // 2}


def _model(layout, want, header=True):
    """What a faultless device would leave: (out, fill, lens)."""
    fill = canary(layout.out_size)
    out = fill.copy()
    lens = []
    for pl in layout.places:
        w = np.frombuffer(want[pl.probe], np.uint8) if pl.probe != OVERSIZE else np.zeros(0, np.uint8)
        out[pl.out_off:pl.out_off + w.size] = w
        lens.append(NOT_A_BLOCK if pl.probe == OVERSIZE else w.size)
    return out, fill, np.array(lens, np.uint32)


def test_comparison_has_teeth(oracle):
    """The comparison, fed a faultless result and then one flipped byte of one stream, one length
    off by one, one lost error mark and one byte written between two slots, names the right probe,
    placement, mode, block and offset each time -- on A's layout and on one of B's."""
    want = {i: oracle.compress(b) for i, (_, b) in enumerate(catalogue())}
    for placement, lay in (("A", residue_layout()), ("B-oversize-in9", rounds_layout(("oversize", 9), 104))):
        out, fill, lens = _model(lay, want)
        assert slot_diffs(placement, "fast", lay, want, out, lens) == []
        assert canary_diffs(placement, "fast", lay, out, fill) == []
        j = next(j for j, pl in enumerate(lay.places)
                 if pl.probe == NAMES.index("period7-1025") and j > len(lay.places) // 2)
        pl = lay.places[j]
        # one byte of one stream
        bad = out.copy()
        bad[pl.out_off + 9] ^= 0x20
        d = slot_diffs(placement, "fast", lay, want, bad, lens)
        assert d == [Diff(placement, "fast", "period7-1025", pl.where, "bytes differ", 9)]
        assert "period7-1025" in str(d[0]) and pl.where in str(d[0]) and "offset 9" in str(d[0]) and "fast" in str(d[0])
        # its last byte, and its first
        for at in (0, len(want[pl.probe]) - 1):
            bad = out.copy()
            bad[pl.out_off + at] ^= 1
            assert [x.offset for x in slot_diffs(placement, "dense", lay, want, bad, lens)] == [at]
        # one length off by one, either way (the bytes as they were)
        for delta in (1, -1):
            off = lens.astype(np.int64)
            off[j] += delta
            d = slot_diffs(placement, "dense", lay, want, out, off)
            assert len(d) == 1 and d[0][:4] == (placement, "dense", "period7-1025", pl.where)
            assert d[0].what == "length %d, canonical %d" % (len(want[pl.probe]) + delta, len(want[pl.probe]))
        # a byte just behind a slot's room, and one just before a slot
        room = room_of(1025)
        for at, owner in ((pl.out_off + room, j), (pl.out_off - 1, j - 1)):
            bad = out.copy()
            bad[at] ^= 0x80
            assert slot_diffs(placement, "fast", lay, want, bad, lens) == []
            d = canary_diffs(placement, "fast", lay, bad, fill)
            assert len(d) == 1 and d[0].where == lay.places[owner].where and d[0].offset == at - lay.places[owner].out_off
    # the oversize block's mark lost, and its slot written
    lens2 = lens.astype(np.int64)
    lens2[5] = 0
    d = slot_diffs("B", "fast", lay, want, out, lens2)
    assert len(d) == 1 and d[0].probe == "oversize" and d[0].where == "filler 5"
    bad = out.copy()
    bad[lay.places[5].out_off] ^= 1
    d = canary_diffs("B", "fast", lay, bad, fill)
    assert len(d) == 1 and d[0].probe == "oversize" and d[0].where == "filler 5" and d[0].offset == 0


# ---- GPU ----------------------------------------------------------------------------------------

def device_call(sm, mode, layout, call="batch", total_len=0, stream=None, device=None):
    """One call on the device over the layout: (d_out_len as unsigned, the output buffer, its
    canary fill, sm_ctx_last_batch_parts after the call)."""
    import torch
    dev = torch.device("cuda", 0)
    d_in = torch.from_numpy(fill_input(layout)).to(dev)
    fill = canary(layout.out_size)
    d_out = torch.from_numpy(fill.copy()).to(dev)
    assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    in_off = torch.tensor([pl.in_off for pl in layout.places], dtype=torch.int64, device=dev)
    in_len = torch.tensor([len(probe(pl.probe)) for pl in layout.places], dtype=torch.int32, device=dev)
    out_off = torch.tensor([pl.out_off for pl in layout.places], dtype=torch.int64, device=dev)
    out_len = torch.full((len(layout.places),), 7, dtype=torch.int32, device=dev)
    if call == "batch":
        sm.compress_batch_device(d_in, in_off, in_len, d_out, out_off, out_len, mode=mode, stream=stream, device=device)
    else:
        sm.compress_fragments_device(d_in, in_off, in_len, d_out, out_off, out_len, total_len, mode=mode,
                                     stream=stream, device=device)
    parts = sm.last_batch_parts(0 if device is None else device)
    torch.cuda.synchronize()
    return out_len.cpu().numpy().astype(np.int64) & 0xFFFFFFFF, d_out.cpu().numpy(), fill, parts


def alone(i):
    """Probe i in a call of its own: one block, input and slot on 16-byte boundaries."""
    return Layout([Place(i, "alone", 16, 16, 16, 17)], 16 + len(probe(i)) + 48, 16 + room_of(len(probe(i))) + 64)


@pytest.fixture(scope="module")
def canon(sm, oracle, gpu_available):
    """{mode: {probe index: its canonical stream}}; reference mode's are the oracle's."""
    res = {"reference": {i: oracle.compress(b) for i, (_, b) in enumerate(catalogue())}}
    for mode in MODES:
        res[mode] = {}
        for i, (name, b) in enumerate(catalogue()):
            lay = alone(i)
            assert lay.places[0].in_off % 16 == 0 and lay.places[0].out_off % 16 == 0
            lens, out, fill, _ = device_call(sm, mode, lay)
            assert 0 < lens[0] <= room_of(len(b)), (name, mode, lens[0])
            report(canary_diffs("alone", mode, lay, out, fill))
            s = out[16:16 + int(lens[0])].tobytes()
            assert oracle.uncompress(s) == b, (name, mode)
            res[mode][i] = s
    return res


@pytest.fixture(scope="module")
def grid(gpu_available):
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def header_of(n):
    return 1 if n < 128 else 2 if n < 16384 else 3


@gpu
@pytest.mark.parametrize("mode", MODES)
def test_catalogue_covers_the_three_outcomes(canon, mode):
    """The canonical streams hold the screen's literal, the writer's one-literal fallback and at
    least ten parsed blocks of less than half their length."""
    size = {NAMES[i]: len(s) for i, s in canon[mode].items()}
    n_of = {name: len(b) for name, b in catalogue()}
    literal = lambda name: size[name] == header_of(n_of[name]) + 3 + n_of[name]
    assert literal("random-65536") and literal("random-65535")  # the screen's
    assert size["fallback-65536"] == 3 + 3 + BLOCK and literal("fallback-65535")  # the writer's
    small = [name for name in NAMES if n_of[name] and size[name] < n_of[name] // 2]
    assert len(small) >= 10, small


def run_placement(sm, placement, mode, layout, want, g=None):
    lens, out, fill, parts = device_call(sm, mode, layout)
    if g is not None and mode != "reference":
        assert parts == rule(len(layout.places), g)[0], (placement, mode, parts)
    report(slot_diffs(placement, mode, layout, want, out, lens) + canary_diffs(placement, mode, layout, out, fill))


@gpu
@pytest.mark.parametrize("mode", MODES + ("reference",))
def test_a_every_residue(sm, canon, mode):
    """A (and D's half of it): all 16 input and all 16 slot residues for every probe, one call."""
    run_placement(sm, "A", mode, residue_layout(), canon[mode])


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", B_NAMES)
def test_b_rounds_and_predecessors(sm, canon, grid, name, mode):
    """B: every probe behind every filler kind in its workgroup's LDS, at both input residues, and
    the remainder in 16 parts, in 2 parts and as a third whole round."""
    case = B_CASES[B_NAMES.index(name)]
    run_placement(sm, "B-" + name, mode, rounds_layout(case, grid), canon[mode], grid)


@gpu
@pytest.mark.parametrize("name", [n for n in B_NAMES if n.startswith("text-")])
def test_d_reference_mode_in_place(sm, canon, grid, name):
    """D: more blocks than compute units, so the reference kernel reads every block in place from
    its address: all probes at input residues 0 and 9 (A in reference mode has the other 14)."""
    case = B_CASES[B_NAMES.index(name)]
    run_placement(sm, "D-" + name, "reference", rounds_layout(case, grid), canon["reference"])


@gpu
@pytest.mark.parametrize("mode", MODES)
def test_c_entry_points(sm, canon, mode):
    """C: the host batch call, the single-buffer call with the split parse on and off, and the
    fragment call with the stream's own table size and with the largest."""
    diffs = []

    def same(where, i, got, want):
        g, w = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        if got != want:
            what = "bytes differ" if g.size == w.size else "length %d, canonical %d" % (g.size, w.size)
            diffs.append(Diff("C", mode, NAMES[i], where, what, first_diff(g, w)))

    for i, (name, b) in enumerate(catalogue()):
        want = canon[mode][i]
        same("compress_batch", i, sm.compress_batch([b], mode=mode)[0], want)
        try:
            for on in (True, False):
                sm.set_split_compress(on)
                same("compress, split %s" % ("on" if on else "off"), i, sm.compress(b, mode=mode), want)
        finally:
            sm.set_split_compress(True)
        lay = alone(i)
        for total in (len(b), 1 << 20):
            where = "compress_fragments_device, total_len %d" % total
            lens, out, fill, _ = device_call(sm, mode, lay, "frag", total)
            frag = {i: want[header_of(len(b)):]}
            diffs.extend(slot_diffs("C", mode, Layout([lay.places[0]._replace(where=where)], 0, 0), frag, out, lens,
                                    header=False))
            diffs.extend(canary_diffs("C", mode, lay, out, fill, header=False))
    report(diffs)


# ---- E. beyond 4 GiB ----------------------------------------------------------------------------

BIG, LOW = 1 << 32, 16 << 20
FAR_PITCH = 76533  # odd: the 14 blocks meet 14 residues; a slot's room (76,495) and a gap


def far_layout(g=None):
    """The 64 KiB probes and six short ones, input and slot of block i at BIG + 3 + i FAR_PITCH (14
    blocks: all of them remainder blocks, parsed in parts).  With g, short probes behind them up to
    g + 1 blocks: a whole round for the persistent workgroups, one block in parts, and more blocks
    than compute units for the reference kernel."""
    idx = [i for i, (_, b) in enumerate(catalogue()) if len(b) == BLOCK]
    idx += [next(i for i, (_, b) in enumerate(catalogue()) if len(b) == n) for n in (0, 1, 17, 257, 1025, 4097)]
    places = [Place(p, "block %d at 2^32 + %d" % (i, 3 + i * FAR_PITCH), BIG + 3 + i * FAR_PITCH,
                    BIG + 3 + i * FAR_PITCH, 3, 17) for i, p in enumerate(idx)]
    if g is not None:
        short = [i for i, (_, b) in enumerate(catalogue()) if len(b) <= 4097]
        at = 3 + len(idx) * FAR_PITCH
        for j in range(len(idx), g + 1):
            p = NAMES.index("text-20001") if j == g else short[j % len(short)]
            places.append(Place(p, "block %d at 2^32 + %d" % (j, at), BIG + at, BIG + at, 17, 17))
            at += room_of(len(probe(p))) + 18
    return Layout(places, BIG + LOW, BIG + LOW)


def test_far_layout():
    lay = far_layout()
    assert len(lay.places) == 14 and FAR_PITCH > room_of(BLOCK) + 17 and FAR_PITCH > BLOCK + 1 + 17
    assert len({pl.in_off % 16 for pl in lay.places}) == 14
    for g in (104, 256, 304):
        more = far_layout(g)
        assert more.places[:14] == lay.places and len(more.places) == g + 1 and rule(g + 1, g) == (1, 16)
        end = BIG
        for pl in more.places:
            assert pl.in_off == pl.out_off > end  # (input and slot at the same offset of their buffers)
            assert (pl.in_off & 0xFFFFFFFF) < LOW  # truncated, it lies in the low canary
            end = pl.out_off + room_of(len(probe(pl.probe)))
        assert end + 64 < BIG + LOW
        assert len({pl.in_off % 16 for pl in more.places}) == 16


def far_calls(sm, canon, lay, what, bufs):
    """E's calls over one layout: compress in every mode, then the three decode calls on the streams
    where they lie."""
    import torch
    d_a, d_b, d_fill, fill = bufs
    dev = d_a.device
    n = len(lay.places)
    far_in = fill.copy()
    for pl in lay.places:
        b = np.frombuffer(probe(pl.probe), np.uint8)
        far_in[pl.in_off - BIG:pl.in_off - BIG + b.size] = b
    d_far_in = torch.from_numpy(far_in).to(dev)
    off = torch.tensor([pl.in_off for pl in lay.places], dtype=torch.int64, device=dev)
    lens_in = torch.tensor([len(probe(pl.probe)) for pl in lay.places], dtype=torch.int32, device=dev)

    def low_untouched(call):
        for name, d in (("d_in", d_a), ("d_out", d_b)):
            assert torch.equal(d[:LOW], d_fill), "%s, %s: %s's bytes below 16 MiB changed (a truncated offset)" % (
                what, call, name)

    for mode in MODES + ("reference",):
        d_a[:LOW].copy_(d_fill)
        d_a[BIG:].copy_(d_far_in)
        for lo in (0, BIG):
            d_b[lo:lo + LOW].copy_(d_fill)
        out_len = torch.full((n,), 7, dtype=torch.int32, device=dev)
        sm.compress_batch_device(d_a, off, lens_in, d_b, off, out_len, mode=mode)
        if mode != "reference":
            assert sm.last_batch_parts(0) == rule(n, torch.cuda.get_device_properties(0).multi_processor_count)[0]
        torch.cuda.synchronize()
        low_untouched("compress, " + mode)
        assert torch.equal(d_a[BIG:], d_far_in), (what, mode)
        lens = out_len.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
        out = d_b[BIG:].cpu().numpy()
        report(slot_diffs(what, mode, lay, canon[mode], out, lens, base=BIG) +
               canary_diffs(what, mode, lay, out, fill, base=BIG))
        # the streams where they lie, decoded to the far offsets of the first buffer
        d_a[BIG:].copy_(d_fill)
        dec_len = torch.full((n,), 7, dtype=torch.int32, device=dev)
        status = torch.full((n,), -1, dtype=torch.int32, device=dev)
        sm.uncompress_batch_device(d_b, off, out_len, d_a, off, lens_in, dec_len, status)
        v_status = torch.full((n,), -1, dtype=torch.int32, device=dev)
        sm.validate_batch_device(d_b, off, out_len, v_status)
        l_len = torch.full((n,), 7, dtype=torch.int32, device=dev)
        l_status = torch.full((n,), -1, dtype=torch.int32, device=dev)
        sm.uncompressed_length_batch_device(d_b, off, out_len, l_len, l_status)
        torch.cuda.synchronize()
        low_untouched("decode, " + mode)
        assert status.tolist() == [0] * n and v_status.tolist() == [0] * n and l_status.tolist() == [0] * n, (what, mode)
        assert dec_len.tolist() == lens_in.tolist() == l_len.tolist(), (what, mode)
        assert torch.equal(d_a[BIG:], d_far_in), "%s, %s: the decoded far region is not the probes between untouched bytes" % (
            what, mode)
        assert np.array_equal(d_b[BIG:].cpu().numpy(), out), (what, mode)  # (the decode calls write no input)


@gpu
def test_e_offsets_beyond_4gib(sm, canon, grid):
    """E: every u64 offset of the batch compress and decode calls above 2^32, in buffers that hold
    the truncated offsets too (canary there: a 32-bit offset reads or writes it and shows).  Two
    layouts: 14 blocks (the fast modes parse all of them in parts, the reference kernel stages
    them) and g + 1 (the persistent workgroups' round and one block in parts; the reference kernel
    in place)."""
    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    assert free >= 9 << 30, "two buffers of 2^32 + 16 MiB bytes need about 9 GiB, %d MiB are free" % (free >> 20)
    fill = canary(LOW)
    d_fill = torch.from_numpy(fill).to(dev)
    d_a = torch.empty(BIG + LOW, dtype=torch.uint8, device=dev)
    d_b = torch.empty(BIG + LOW, dtype=torch.uint8, device=dev)
    assert d_a.data_ptr() % 16 == 0 and d_b.data_ptr() % 16 == 0
    far_calls(sm, canon, far_layout(), "E-14", (d_a, d_b, d_fill, fill))
    far_calls(sm, canon, far_layout(grid), "E-g+1", (d_a, d_b, d_fill, fill))
    del d_a, d_b
    torch.cuda.empty_cache()


# ---- F. under capture ---------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("mode", MODES)
def test_f_under_graph_capture(sm, canon, mode):
    """F: a 3-block call captured on a stream that its context (a fresh one) has never seen
    allocates nothing and parses every block whole; each replay gives the canonical streams of what
    the input holds then; the eager call behind it gets the scratch and parses in parts."""
    import torch
    dev = torch.device("cuda", 0)
    ctx = ("placement-capture", 0, MODES.index(mode))  # a context of its own on device 0
    pick = lambda *names: [NAMES.index(x) for x in names]
    sets = [pick("text-65536", "period7-1025", "fallback-65536"), pick("const-65536", "text-20001", "random-65535"),
            pick("texttail-65536", "text-0", "planted-65536")]
    in_pitch, pitch = BLOCK + 16, MAXC + 22
    side = torch.cuda.Stream(dev)
    d_in = torch.zeros(3 * in_pitch, dtype=torch.uint8, device=dev)
    in_off = torch.arange(3, dtype=torch.int64, device=dev) * in_pitch
    out_off = torch.arange(3, dtype=torch.int64, device=dev) * pitch + 16
    in_len = torch.zeros(3, dtype=torch.int32, device=dev)
    fill = canary(16 + 3 * pitch)
    d_fill = torch.from_numpy(fill).to(dev)
    d_out = d_fill.clone()
    out_len = torch.full((3,), 7, dtype=torch.int32, device=dev)

    def load(which):  # in place: the captured call reads these tensors
        host = np.zeros(3 * in_pitch, np.uint8)
        for j, p in enumerate(which):
            host[j * in_pitch:j * in_pitch + len(probe(p))] = np.frombuffer(probe(p), np.uint8)
        d_in.copy_(torch.from_numpy(host))
        in_len.copy_(torch.tensor([len(probe(p)) for p in which], dtype=torch.int32))
        d_out.copy_(d_fill)
        out_len.fill_(7)
        torch.cuda.synchronize()

    def check(which, where):
        torch.cuda.synchronize()
        lay = Layout([Place(p, "%s, block %d" % (where, j), j * in_pitch, 16 + j * pitch, 0, 0)
                      for j, p in enumerate(which)], 0, fill.size)
        lens = out_len.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
        out = d_out.cpu().numpy()
        report(slot_diffs("F", mode, lay, canon[mode], out, lens) + canary_diffs("F", mode, lay, out, fill))

    load(sets[0])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        sm.compress_batch_device(d_in, in_off, in_len, d_out, out_off, out_len, mode=mode, stream=side, device=ctx)
        assert sm.last_batch_parts(ctx) == 0  # no scratch, none allocated: every block whole
    for which in sets[1:]:
        load(which)
        with torch.cuda.stream(side):
            graph.replay()
        check(which, "replay")
    load(sets[0])
    sm.compress_batch_device(d_in, in_off, in_len, d_out, out_off, out_len, mode=mode, stream=side, device=ctx)
    assert sm.last_batch_parts(ctx) == 3  # the scratch now exists: all three blocks in parts
    check(sets[0], "eager")
