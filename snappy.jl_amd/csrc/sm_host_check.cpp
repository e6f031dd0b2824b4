// sm_host_check.cpp -- stand-alone driver of sm_host_rules.h (no device, no HIP): what the main
// library's host side decides from bytes it does not trust, on heap buffers of exactly the
// documented sizes, so that AddressSanitizer and UBSan (make host_check) see one byte of over-read.
// Also the rules the kernels' walkers share with it (sm_format.h decode_tag and check_tag,
// common/smc_layout.h parse_varint32): swept here as the plain C++ they are.
// Expected values come from the CPU oracle (oracle/snappy_oracle.c), from a byte-at-a-time tag
// walker written here, or from the construction of the case -- never from the code under test.
//   sm_host_check <text file of at least 150000 bytes>   (tests/golden/testdata/alice29.txt)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <set>
#include <vector>

#include "../../oracle/snappy_oracle.h"
#include "sm_host_rules.h"

namespace {

int failures = 0;

#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      ++failures;                                                 \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);  \
    }                                                             \
  } while (0)

typedef std::vector<uint8_t> Bytes;

template <typename T>
std::unique_ptr<T[]> exact(const std::vector<T>& v) {  // a heap array of exactly v.size() elements
  std::unique_ptr<T[]> p(new T[v.size()]);
  if (!v.empty()) memcpy(p.get(), v.data(), v.size() * sizeof(T));
  return p;
}

void put_varint(Bytes& o, uint32_t v) {
  while (v >= 0x80) {
    o.push_back((uint8_t)(v | 0x80));
    v >>= 7;
  }
  o.push_back((uint8_t)v);
}

// the header of a stream, parsed here: false when it is not a whole varint32
bool header(const Bytes& s, uint32_t* size, size_t* hdr) {
  uint64_t v = 0;
  for (size_t i = 0; i < 5 && i < s.size(); ++i) {
    v |= (uint64_t)(s[i] & 0x7f) << (7 * i);
    if (s[i] < 0x80) {
      *size = (uint32_t)v;
      *hdr = i + 1;
      return v <= 0xffffffffull;
    }
  }
  return false;
}

uint8_t filler(size_t i) { return (uint8_t)(i * 131 + 7); }

// a literal of len bytes with nb length bytes behind its tag (0: the length in the tag, len <= 60)
void put_literal(Bytes& o, uint32_t len, uint32_t nb) {
  if (nb == 0) {
    o.push_back((uint8_t)((len - 1) << 2));
  } else {
    o.push_back((uint8_t)((59 + nb) << 2));
    for (uint32_t k = 0; k < nb; ++k) o.push_back((uint8_t)((len - 1) >> (8 * k)));
  }
  for (uint32_t k = 0; k < len; ++k) o.push_back(filler(o.size()));
}

Bytes oracle_compress(const Bytes& in) {
  Bytes out(smo_max_compressed_length(in.size()));
  size_t n = out.size();
  EXPECT(smo_compress(in.data(), in.size(), out.data(), &n, 0) == SMO_OK);
  out.resize(n);
  return out;
}

// ---- literal_only -----------------------------------------------------------------------------

// Runs literal_only on an exact copy of s against the oracle's decode; returns whether it accepted.
bool literal_case(const Bytes& s) {
  uint32_t size = 0;
  size_t hdr = 0;
  if (!header(s, &size, &hdr)) return false;
  const auto c = exact(s);
  sm::LitSpans sp;
  const bool ok = sm::literal_only(c.get(), s.size(), hdr, size, sp);
  // (a tag makes at most 64 bytes of output: a larger declared length fails under any capacity)
  Bytes out((size_t)std::min<uint64_t>(size, 64 * (uint64_t)s.size()) + 1);
  size_t got = 0;
  const int st = smo_uncompress(c.get(), s.size(), out.data(), out.size(), &got);
  if (st != SMO_OK) EXPECT(!ok);
  if (ok) {
    EXPECT(st == SMO_OK && got == size);
    EXPECT(sp.n >= 1 && sp.n <= sm::kLitSpans && sp.dst[0] == 0 && sp.dst[sp.n] == size);
    Bytes cat;
    for (uint32_t k = 0; k < sp.n && failures == 0; ++k) {
      const uint32_t len = sp.dst[k + 1] - sp.dst[k];
      EXPECT(sp.dst[k + 1] > sp.dst[k] && (size_t)sp.src[k] + len <= s.size());
      if (failures == 0) cat.insert(cat.end(), s.begin() + sp.src[k], s.begin() + sp.src[k] + len);
    }
    EXPECT(st == SMO_OK && cat.size() == got && memcmp(cat.data(), out.data(), got) == 0);
  }
  return ok;
}

Bytes literal_stream(uint32_t declared, const std::vector<std::pair<uint32_t, uint32_t>>& lits) {
  Bytes s;
  put_varint(s, declared);
  for (const auto& l : lits) put_literal(s, l.first, l.second);
  return s;
}

void check_literal_only() {
  for (uint32_t k = 1; k <= 17; ++k) {  // 1 to 16 literals; 17 must refuse
    std::vector<std::pair<uint32_t, uint32_t>> lits(k, {5u, 0u});
    EXPECT(literal_case(literal_stream(5 * k, lits)) == (k <= 16));
  }
  const uint32_t lens[5] = {60, 200, 300, 70000, 70000};
  for (uint32_t nb = 0; nb <= 4; ++nb)  // 0 to 3 length bytes; 4 must refuse
    EXPECT(literal_case(literal_stream(lens[nb] + 7, {{7u, 0u}, {lens[nb], nb}})) == (nb <= 3));
  const std::vector<std::pair<uint32_t, uint32_t>> mixed = {{9u, 0u}, {100u, 1u}, {1000u, 2u}, {12u, 3u}};
  const uint32_t sum = 9 + 100 + 1000 + 12;
  const Bytes valid = literal_stream(sum, mixed);
  EXPECT(literal_case(valid));
  for (size_t at = 0; at <= mixed.size(); ++at) {  // a copy tag at every tag position
    Bytes s;
    put_varint(s, sum + 4);
    for (size_t k = 0; k <= mixed.size(); ++k) {
      if (k == at) {
        s.push_back(0x01);  // copy, 1 offset byte: length 4
        s.push_back(0x01);
      }
      if (k < mixed.size()) put_literal(s, mixed[k].first, mixed[k].second);
    }
    EXPECT(!literal_case(s));
  }
  for (size_t n = 0; n < valid.size(); ++n) EXPECT(!literal_case(Bytes(valid.begin(), valid.begin() + n)));  // every truncation
  EXPECT(!literal_case(literal_stream(sum - 1, mixed)));
  EXPECT(!literal_case(literal_stream(sum + 1, mixed)));
  EXPECT(!literal_case(literal_stream(0, {})));  // an empty body
  EXPECT(!literal_case(literal_stream(5, {})));
  Bytes wrap;  // a length of 2^32 (q + len wraps at 32 bits), and the longest 3-byte length in a short stream
  put_varint(wrap, 0xffffffffu);
  wrap.insert(wrap.end(), {(uint8_t)(63 << 2), 0xff, 0xff, 0xff, 0xff, 1, 2, 3});
  EXPECT(!literal_case(wrap));
  Bytes big;
  put_varint(big, 1u << 24);
  big.insert(big.end(), {(uint8_t)(62 << 2), 0xff, 0xff, 0xff, 1, 2, 3});
  EXPECT(!literal_case(big));
}

// ---- the tag walker of this check (byte at a time, bytes past n read as zero) ---------------------

struct Walk {
  uint64_t exit, out;
};
Walk ref_walk(const Bytes& s, uint64_t p, uint64_t lim, std::vector<uint64_t>* tags = nullptr,
              std::vector<uint64_t>* before = nullptr) {  // tags: every tag start; before: the output before it
  uint64_t o = 0;
  while (p < lim) {
    if (tags) tags->push_back(p);
    if (before) before->push_back(o);
    const uint32_t tag = s[p], kind = tag & 3, up = tag >> 2;
    if (kind == 0) {
      uint64_t len = up + 1, extra = 0;
      if (up >= 60) {
        extra = up - 59;
        len = 1;
        for (uint64_t k = 0; k < extra; ++k) len += (uint64_t)(p + 1 + k < s.size() ? s[p + 1 + k] : 0) << (8 * k);
      }
      p += 1 + extra + len;
      o += len;
    } else {
      p += kind == 1 ? 2 : kind == 2 ? 3 : 5;
      o += kind == 1 ? 4 + (up & 7) : up + 1;
    }
  }
  return {p, o};
}

// literals with 2 and 3 length bytes and the three copy kinds (the walk reads no copy offset's meaning)
Bytes hand_stream(uint32_t* declared) {
  Bytes b;
  put_literal(b, 300, 2);
  b.insert(b.end(), {(uint8_t)(1 | (3 << 2)), 0x10});                     // copy 1: 7 bytes
  put_literal(b, 70000, 3);
  b.insert(b.end(), {(uint8_t)(2 | (39 << 2)), 0x00, 0x01});              // copy 2: 40 bytes
  put_literal(b, 33, 0);
  b.insert(b.end(), {(uint8_t)(3 | (63 << 2)), 0x00, 0x01, 0x00, 0x00});  // copy 4: 64 bytes
  put_literal(b, 61, 1);
  *declared = 300 + 7 + 70000 + 40 + 33 + 64 + 61;
  Bytes s;
  put_varint(s, *declared);
  s.insert(s.end(), b.begin(), b.end());
  return s;
}

void walk_case(const Bytes& s) {
  uint32_t size = 0;
  size_t hdr = 0;
  EXPECT(header(s, &size, &hdr));
  const uint32_t n = (uint32_t)s.size();
  const auto c = exact(s);
  std::vector<uint64_t> tags, before;
  const Walk all = ref_walk(s, hdr, n, &tags, &before);
  EXPECT(all.exit == n && all.out == size);  // (the case is a valid stream)
  uint64_t ex = 0, out = 0;
  sm::host_walk(c.get(), n, hdr, n, &ex, &out);
  EXPECT(ex == n && out == size);
  tags.push_back(n);
  before.push_back(size);
  for (size_t k = 0; k < tags.size(); ++k) {  // in two pieces split at every tag boundary
    uint64_t e1, o1, e2, o2;
    sm::host_walk(c.get(), n, hdr, tags[k], &e1, &o1);
    sm::host_walk(c.get(), n, tags[k], n, &e2, &o2);
    EXPECT(e1 == tags[k] && e2 == n && o1 + o2 == size && o1 == before[k]);
  }
  for (uint32_t k = 1; k <= 4 && k < n; ++k) {  // entering just before the end: nothing past n is read
    sm::host_walk(c.get(), n, n - k, n, &ex, &out);
    const Walk w = ref_walk(s, n - k, n);
    EXPECT(ex == w.exit && out == w.out);
  }
}

// ---- the true path and the fragment table ----------------------------------------------------------

// the index records of s as the index kernel defines them, by the walker above
std::vector<uint32_t> records(const Bytes& s, uint32_t ip0) {
  const uint32_t n = (uint32_t)s.size(), nchunks = (n - ip0 + sm::kIdxChunk - 1) / sm::kIdxChunk;
  std::vector<uint32_t> rec(2 * (size_t)nchunks * sm::kIdxEntries);
  for (uint32_t c = 0; c < nchunks; ++c)
    for (uint32_t l = 0; l < sm::kIdxEntries; ++l) {
      const uint64_t base = ip0 + (uint64_t)c * sm::kIdxChunk, lim = std::min<uint64_t>(base + sm::kIdxChunk, (uint64_t)n - 1);
      const Walk w = ref_walk(s, base + l, lim);
      rec[2 * ((size_t)c * sm::kIdxEntries + l)] = (uint32_t)w.exit;
      rec[2 * ((size_t)c * sm::kIdxEntries + l) + 1] = (uint32_t)w.out;
    }
  return rec;
}

struct PathRun {
  sm::PathEnd end;
  std::vector<sm::PathChunk> path;
  uint32_t nchunks;
};
PathRun path_case(const Bytes& s, const std::vector<uint32_t>* rec_in = nullptr) {
  uint32_t size = 0;
  size_t hdr = 0;
  EXPECT(header(s, &size, &hdr));
  const std::vector<uint32_t> rec = rec_in ? *rec_in : records(s, (uint32_t)hdr);
  const auto c = exact(s);
  const auto r = exact(rec);
  PathRun run;
  run.nchunks = (uint32_t)(rec.size() / (2 * sm::kIdxEntries));
  run.end = sm::true_path(c.get(), (uint32_t)s.size(), (uint32_t)hdr, size, r.get(), run.path);
  return run;
}

// an exact path against the walker: every element starts at a tag, with the output before it
void expect_exact(const Bytes& s, const PathRun& run) {
  uint32_t size = 0;
  size_t hdr = 0;
  EXPECT(header(s, &size, &hdr) && run.end == sm::PathEnd::kExact && !run.path.empty());
  std::vector<uint64_t> tags;
  ref_walk(s, hdr, s.size(), &tags);
  const std::set<uint64_t> starts(tags.begin(), tags.end());
  for (const sm::PathChunk& e : run.path) EXPECT(starts.count(e.y) && ref_walk(s, hdr, e.y).out == e.O && e.ex > e.y);
  const std::vector<sm::StreamFrag> frags = sm::path_frags(run.path, size);
  EXPECT(frags.size() == ((uint64_t)size + 65535) / 65536);
  for (size_t f = 0; f < frags.size(); ++f) {
    EXPECT(starts.count(frags[f].y) && frags[f].O <= frags[f].F && frags[f].F == f * 65536);
    EXPECT(ref_walk(s, hdr, frags[f].y).out == frags[f].O);
    for (const sm::PathChunk& e : run.path)  // the last element that starts at or before F: it reaches past F
      if (e.y == frags[f].y) EXPECT(e.O + e.out > frags[f].F || &e == &run.path.back());
    EXPECT(frags[f].lim == (f + 1 == frags.size() ? 0xffffffffu : (uint32_t)(f + 1) * 65536));
  }
}

Bytes redeclared(const Bytes& s, uint32_t size) {  // the same body under another declared length
  uint32_t old = 0;
  size_t hdr = 0;
  EXPECT(header(s, &old, &hdr));
  Bytes o;
  put_varint(o, size);
  o.insert(o.end(), s.begin() + hdr, s.end());
  return o;
}

void check_paths(const Bytes& text) {
  Bytes five(text.begin(), text.begin() + 150000);
  five.insert(five.end(), text.begin(), text.begin() + 150000);  // 300000 bytes: 5 fragments
  const Bytes s5 = oracle_compress(five);
  const PathRun r5 = path_case(s5);
  EXPECT(r5.nchunks > 9);
  expect_exact(s5, r5);
  EXPECT(sm::path_frags(r5.path, 300000).size() == 5);
  EXPECT(path_case(redeclared(s5, 300001)).end == sm::PathEnd::kFirstError);
  EXPECT(path_case(redeclared(s5, 299999)).end == sm::PathEnd::kFirstError);
  {  // a record that makes no progress
    uint32_t size = 0;
    size_t hdr = 0;
    EXPECT(header(s5, &size, &hdr));
    std::vector<uint32_t> rec = records(s5, (uint32_t)hdr);
    rec[0] = (uint32_t)hdr;
    EXPECT(path_case(s5, &rec).end == sm::PathEnd::kFallBack);
  }
  {  // literals that end deep inside the next chunk: entries past kIdxEntries (the host_walk branch)
    Bytes s;
    put_varint(s, 4000 + 300 + 5000 + 10);
    put_literal(s, 4000, 2);
    put_literal(s, 300, 2);
    put_literal(s, 5000, 2);
    put_literal(s, 10, 0);
    const PathRun r = path_case(s);
    expect_exact(s, r);
    bool deep = false;
    for (const sm::PathChunk& e : r.path) deep = deep || (e.y - 2) % sm::kIdxChunk >= sm::kIdxEntries;
    EXPECT(deep);
  }
  bool one = false, nine = false;  // one chunk, nine chunks (the prefetched record stays inside the array)
  for (uint32_t len = 2000; len <= 150000 && !(one && nine); len += 1000) {
    const Bytes s = oracle_compress(Bytes(text.begin(), text.begin() + len));
    const PathRun r = path_case(s);
    if ((r.nchunks == 1 && !one) || (r.nchunks == 9 && !nine)) {
      expect_exact(s, r);
      (r.nchunks == 1 ? one : nine) = true;
    }
  }
  EXPECT(one && nine);
  // the saturating conversion: O and out at and beyond 2^32
  const uint64_t G = 1ull << 32;
  const std::vector<sm::PathChunk> far = {{5, 100, 50, 9}, {9, G - 1, 5, 11}, {11, G, G, 12}, {12, 2 * G, 1, G + 7}, {13, 100, G, 14}};
  const std::vector<sm::OriginPath> sat = sm::origin_path(far, true);
  EXPECT(sat.size() == far.size());
  for (size_t e = 0; e < sat.size(); ++e) {
    EXPECT((uint64_t)sat[e].O + sat[e].out <= 0xffffffffull && sat[e].y == far[e].y);
    EXPECT(sat[e].O == std::min<uint64_t>(far[e].O, G - 1) && sat[e].ex == std::min<uint64_t>(far[e].ex, G - 1));
    EXPECT(sat[e].out == std::min<uint64_t>(far[e].out, G - 1 - sat[e].O));
  }
  const std::vector<sm::OriginPath> plain = sm::origin_path({far[0]}, false);
  EXPECT(plain.size() == 1 && plain[0].y == 5 && plain[0].ex == 9 && plain[0].O == 100 && plain[0].out == 50);
}

// ---- host batches -----------------------------------------------------------------------------

void check_shards() {
  for (uint32_t nblk : {0u, 1u, 7u})
    for (int nctx : {1, 3, 8}) {
      std::vector<uint64_t> in_off(nblk), out_off(nblk);
      for (uint32_t b = 0; b < nblk; ++b) {  // unsorted
        in_off[b] = (uint64_t)((b * 5) % 7) * 1000 + 17;
        out_off[b] = (uint64_t)((b * 3) % 7) * 4096 + 5;
      }
      const auto i = exact(in_off), o = exact(out_off);
      const std::vector<sm::Shard> sh = sm::make_shards(nctx, nblk, i.get(), o.get());
      EXPECT(sh.size() == (size_t)nctx);
      uint32_t next = 0;
      for (const sm::Shard& s : sh) {
        if (s.n == 0) continue;
        EXPECT(s.b0 == next && s.in_off.size() == s.n && s.out_off.size() == s.n);  // each block once, in order
        for (uint32_t k = 0; k < s.n && s.b0 + k < nblk; ++k) {
          EXPECT(s.in_base <= in_off[s.b0 + k] && s.out_base <= out_off[s.b0 + k]);  // rebased offsets >= 0
          EXPECT(s.in_base + s.in_off[k] == in_off[s.b0 + k] && s.out_base + s.out_off[k] == out_off[s.b0 + k]);
        }
        next = s.b0 + s.n;
      }
      EXPECT(next == nblk);
    }
}

void check_lengths() {
  const std::vector<uint32_t> in_len = {0, 1, 100, 65535, 65536};
  std::vector<uint32_t> bound;
  for (uint32_t n : in_len) bound.push_back(32 + n + n / 6);  // include/snappy_mi355x.h
  const auto il = exact(in_len);
  EXPECT(sm::check_compressed_lengths(exact(bound).get(), il.get(), (uint32_t)in_len.size()) == SM_OK);
  EXPECT(sm::check_compressed_lengths(exact(bound).get(), il.get(), 0) == SM_OK);
  for (size_t b = 0; b < in_len.size(); ++b) {
    const struct {
      uint32_t len;
      sm_status want;
    } cases[] = {{bound[b] + 1, SM_ERR_ARGUMENT}, {SM_OUT_LEN_ERROR, SM_ERR_DEVICE}, {0xffffffffu, SM_ERR_DEVICE}};
    for (const auto& cs : cases) {
      std::vector<uint32_t> ol = bound;
      ol[b] = cs.len;
      EXPECT(sm::check_compressed_lengths(exact(ol).get(), il.get(), (uint32_t)in_len.size()) == cs.want);
    }
  }
}

void check_varint() {
  for (uint32_t v : {0u, 1u, 127u, 128u, 16383u, 16384u, 300000u, (1u << 28) - 1, 1u << 28, 0xffffffffu}) {
    uint8_t a[5], b[5];
    const size_t na = sm::encode32(a, v), nb = smo_encode32(b, v);
    EXPECT(na == nb && memcmp(a, b, na) == 0);
    for (size_t len = 0; len <= na; ++len) {  // every truncation, on an exact buffer
      const auto c = exact(Bytes(a, a + len));
      uint32_t got = 0, want = 0;
      size_t next = 0, wnext = 0;
      const sm_status st = sm::parse32(c.get(), len, 0, &got, &next);
      EXPECT((int)st == smo_parse32(c.get(), len, 0, &want, &wnext));
      if (st == SM_OK) EXPECT(len == na && got == v && next == na && want == v && wnext == na);
    }
  }
  const uint8_t over[5] = {0xff, 0xff, 0xff, 0xff, 0x10};  // a fifth byte >= 0x10
  EXPECT(sm::parse32(over, 5, 0, nullptr, nullptr) == SM_ERR_VARINT);
}

// ---- the shared rules: one tag, the reference's checks, the varint (sm_format.h, smc_layout.h) ----

const uint8_t kTrailerBytes[7] = {0x00, 0x01, 0x7f, 0x80, 0xc7, 0xc8, 0xff};

// decode_tag for every tag byte and trailer bytes at the mask's edges in each of the four
// positions, against the oracle's table and the rule restated: kind, extra bytes, length, offset
void check_tags() {
  for (uint32_t c = 0; c < 256; ++c)
    for (uint32_t k = 0; k < 7 * 7 * 7 * 7; ++k) {
      const uint8_t b[4] = {kTrailerBytes[k % 7], kTrailerBytes[k / 7 % 7], kTrailerBytes[k / 49 % 7], kTrailerBytes[k / 343]};
      const uint32_t tr = b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24;
      const sm::Tag t = sm::decode_tag(c, tr);
      const uint32_t entry = smo_char_table((uint8_t)c);
      const uint32_t kind = c & 3, up = c >> 2;
      const uint32_t extra = kind == 0 ? (up >= 60 ? up - 59 : 0) : kind == 1 ? 1 : kind == 2 ? 2 : 4;
      uint32_t trailer = 0;
      for (uint32_t i = 0; i < extra; ++i) trailer |= (uint32_t)b[i] << (8 * i);
      bool ok = t.c == c && t.entry == entry && t.taglen == extra && t.taglen == entry >> 11 && t.trailer == trailer;
      if (kind == 0) {
        const uint32_t lit = (up < 60 ? up + 1 : 1) + trailer;  // (wraps at 32 bits for ff ff ff ff)
        ok = ok && !t.is_copy() && t.literal_len() == lit && t.out_bytes() == lit && t.size() == 1ull + extra + lit;
        if (extra == 0 || (extra == 1 && lit <= 200)) ok = ok && sm::window_out_bytes(c, 1 + extra + lit) == lit;
      } else {
        const uint32_t len = kind == 1 ? 4 + (up & 7) : up + 1;
        const uint32_t off = (kind == 1 ? (c >> 5) << 8 : 0) + trailer;
        ok = ok && t.is_copy() && t.len() == len && t.out_bytes() == len && t.offset() == off && t.size() == 1ull + extra;
        ok = ok && sm::window_out_bytes(c, 1 + extra) == len;
      }
      const sm::Tag t8 = sm::decode_tag8((uint64_t)tr << 8 | c);
      ok = ok && t8.c == t.c && t8.entry == t.entry && t8.taglen == t.taglen && t8.trailer == t.trailer;
      if (!ok) {
        EXPECT(ok);
        fprintf(stderr, "  tag byte %02x, trailer %08x\n", c, tr);
        return;
      }
    }
}

// a stream's status by decode_tag and check_tag alone, on the reference's loop (internal.jl:411-466)
int shared_status(const Bytes& s) {
  uint32_t size = 0;
  size_t hdr = 0;
  if (!header(s, &size, &hdr)) return sm::kErrVarint;
  const uint32_t n = (uint32_t)s.size();
  uint64_t op = 0, p = hdr;
  while (p + 1 < n) {
    uint32_t tr = 0;
    for (uint32_t k = 0; k < 4; ++k) tr |= (p + 1 + k < n ? (uint32_t)s[p + 1 + k] : 0u) << (8 * k);
    const sm::Tag t = sm::decode_tag(s[p], tr);
    const int32_t st = sm::check_tag(t, op, size, p + 1 + t.taglen, n);
    if (st != sm::kOk) return st;
    op += t.out_bytes();
    p += t.size();
  }
  return op == size ? sm::kOk : sm::kErrInvalid;
}

int checks_run = 0, checks_failing = 0;
void checks_case(const Bytes& s, uint32_t declared) {
  const auto c = exact(s);
  Bytes out((size_t)declared + 64);
  size_t got = 0;
  const int want = smo_uncompress(c.get(), s.size(), out.data(), out.size(), &got);
  const int have = shared_status(s);
  EXPECT(have == want);
  ++checks_run;
  checks_failing += want != SMO_OK;
}

Bytes raw_copy(uint32_t kind, uint32_t offset, uint32_t len) {
  if (kind == 1) return {(uint8_t)(1 | (len - 4) << 2 | (offset >> 8) << 5), (uint8_t)offset};
  Bytes b = {(uint8_t)(kind | (len - 1) << 2)};
  for (uint32_t k = 0; k < (kind == 2 ? 2u : 4u); ++k) b.push_back((uint8_t)(offset >> (8 * k)));
  return b;
}

// one- and two-tag streams around each bound of the three checks: the verdict of check_tag must be
// the oracle's status
void check_checks() {
  for (uint32_t op : {1u, 9u, 20u})  // a literal of op bytes, then a copy
    for (uint32_t kind : {1u, 2u, 3u})
      for (uint32_t len : {1u, 4u, 11u, 16u, 17u, 64u}) {
        if (kind == 1 ? (len < 4 || len > 11) : false) continue;
        for (uint32_t offset : {0u, 1u, 8u, op, op + 1})
          for (int d : {-1, 0, 1, 16}) {  // the declared size: one short of the copy's end, exact, beyond (with the leniency's 16)
            const uint32_t declared = op + len + d;
            Bytes s;
            put_varint(s, declared);
            put_literal(s, op, 0);
            const Bytes cp = raw_copy(kind, offset, len);
            s.insert(s.end(), cp.begin(), cp.end());
            checks_case(s, declared);
            s.push_back(0x00);  // (and with a byte behind it: the copy is then not the input's last tag)
            s.push_back(0x55);
            checks_case(s, declared);
          }
      }
  for (uint32_t nb = 0; nb <= 4; ++nb)  // one literal: to the input's end and the declared size, and one past either
    for (uint32_t n : {1u, 5u, 60u}) {
      for (int din : {-1, 0, 1})
        for (int dout : {-1, 0, 1}) {
          const uint32_t declared = n + dout;
          Bytes s;
          put_varint(s, declared);
          put_literal(s, n, nb);
          if (din < 0) s.pop_back();
          if (din > 0) s.push_back(0x00);
          checks_case(s, declared);
        }
    }
  // four length bytes at the wrap: 1 + 0xfffffffe = 0xffffffff bytes (past everything), 1 + 0xffffffff = 0 bytes
  for (uint8_t low : {(uint8_t)0xfe, (uint8_t)0xff})
    for (uint32_t declared : {0u, 3u})
      for (uint32_t behind : {0u, 3u}) {
        Bytes s;
        put_varint(s, declared);
        s.insert(s.end(), {(uint8_t)(63 << 2), low, 0xff, 0xff, 0xff});
        if (behind) put_literal(s, behind, 0);
        checks_case(s, declared);
      }
  EXPECT(checks_run > 600 && checks_failing > 200 && checks_run - checks_failing > 50);
}

// parse_varint32 against the oracle's parse32: every length from 0 to 6 bytes, every last byte at
// the rule's edges, on exact buffers
void check_varint_rule() {
  const uint8_t last[6] = {0x00, 0x0f, 0x10, 0x7f, 0x80, 0xff}, lead[3] = {0x80, 0xff, 0x01};
  for (uint32_t len = 0; len <= 6; ++len) {
    uint32_t leads = 1;
    for (uint32_t k = 1; k < len; ++k) leads *= 3;
    for (uint32_t l = 0; l < (len ? 6u : 1u); ++l)
      for (uint32_t m = 0; m < leads; ++m) {
        Bytes b;
        for (uint32_t k = 0, r = m; k + 1 < len; ++k, r /= 3) b.push_back(lead[r % 3]);
        if (len) b.push_back(last[l]);
        const auto c = exact(b);
        const uint8_t* q = c.get();
        uint32_t got = 0, hv = 0, want = 0;
        size_t wnext = 0;
        const int32_t st = smc::parse_varint32([&](uint32_t i) { return (uint32_t)q[i]; }, len, got, hv);
        EXPECT(st == smo_parse32(q, len, 0, &want, &wnext));
        EXPECT(st == 0 || st == SM_ERR_VARINT);
        if (st == 0) EXPECT(got == want && hv == wnext && smc::varint_len(got) <= hv);
        uint32_t got2 = 0;
        size_t next2 = 0;
        EXPECT((int)sm::parse32(q, len, 0, &got2, &next2) == st && (st != 0 || (got2 == got && next2 == hv)));
      }
  }
  for (uint32_t v : {0u, 127u, 128u, 16383u, 16384u, (1u << 21) - 1, 1u << 21, (1u << 28) - 1, 1u << 28, 0xffffffffu}) {
    uint8_t a[5];
    EXPECT(smc::varint_len(v) == smo_encode32(a, v));
  }
}

// ---- the emit rules (sm_format.h, smc_layout.h) --------------------------------------------------
// Expected values: the oracle's encoder and decoder, decode_tag's round trip (itself swept against
// the oracle's table above), and the reference's loops and tables written out here.

Bytes tag_bytes(const sm::TagBytes& t) {
  Bytes b;
  for (uint32_t j = 0; j < t.size; ++j) b.push_back(t.byte(j));
  return b;
}
sm::Tag decode_bytes(const Bytes& b) {
  uint32_t tr = 0;
  for (uint32_t k = 0; k < 4; ++k) tr |= (1 + k < b.size() ? (uint32_t)b[1 + k] : 0u) << (8 * k);
  return sm::decode_tag(b[0], tr);
}

// varint(len), the rule's literal tag, len filler bytes
Bytes literal_stream(uint32_t len, sm::LiteralRule rule, const Bytes& body) {
  Bytes s;
  put_varint(s, len);
  const Bytes t = tag_bytes(sm::literal_tag(len, rule));
  s.insert(s.end(), t.begin(), t.end());
  s.insert(s.end(), body.begin(), body.end());
  return s;
}

// emit_copy!'s loop (internal.jl:306-329), written out: the pieces' lengths
std::vector<uint32_t> copy_pieces(uint32_t len) {
  std::vector<uint32_t> p;
  while (len >= 68) { p.push_back(64); len -= 64; }
  if (len > 64) { p.push_back(60); len -= 60; }
  p.push_back(len);
  return p;
}

void check_emit_rules() {
  // varint_byte: every length class, both ends of each
  for (uint32_t v : {0u, 127u, 128u, 16383u, 16384u, (1u << 21) - 1, 1u << 21, (1u << 28) - 1, 1u << 28, 0xffffffffu}) {
    uint8_t a[5];
    const size_t na = smo_encode32(a, v);
    for (size_t i = 0; i < na; ++i) EXPECT(smc::varint_byte(v, (uint32_t)i, (uint32_t)na) == a[i]);
  }
  // literal_tag, standard rule
  for (uint32_t len : {1u, 59u, 60u, 61u, 255u, 256u, 257u, 65535u, 65536u, 65537u, 1u << 24, (1u << 24) + 1, 0xffffffffu}) {
    const sm::TagBytes t = sm::literal_tag(len, sm::kLiteralStd);
    const uint32_t want = len <= 60 ? 1 : len <= 256 ? 2 : len <= 65536 ? 3 : len <= (1u << 24) ? 4 : 5;
    const sm::Tag d = decode_bytes(tag_bytes(t));
    EXPECT(t.size == want && sm::literal_tag_bytes(len) == want && t.size <= 5 && (t.size == 5 || t.bytes >> (8 * t.size) == 0));
    EXPECT(!d.is_copy() && d.literal_len() == len && 1 + d.taglen == t.size);
    if (len <= 65536) {
      Bytes body(len), out(len + 1);
      for (uint32_t k = 0; k < len; ++k) body[k] = filler(k);
      const Bytes s = literal_stream(len, sm::kLiteralStd, body);
      size_t got = 0;
      EXPECT(smo_uncompress(s.data(), s.size(), out.data(), out.size(), &got) == SMO_OK && got == len &&
             memcmp(out.data(), body.data(), len) == 0);
      EXPECT(sm::block_literal_bytes(len, true) == s.size() && sm::block_literal_bytes(len, false) == s.size() - smc::varint_len(len));
      for (uint32_t j = 0; j + len < s.size(); ++j) {
        EXPECT(sm::block_literal_head_byte(len, true, j) == s[j]);
        if (j >= smc::varint_len(len)) EXPECT(sm::block_literal_head_byte(len, false, j - smc::varint_len(len)) == s[j]);
      }
    }
  }
  EXPECT(sm::block_literal_bytes(0, true) == 1 && sm::block_literal_bytes(0, false) == 0 && sm::block_literal_head_byte(0, true, 0) == 0);
  // ... and the reference's rule (Q3): another tag at 60 and nowhere else; the streams are the oracle's
  for (uint32_t len = 1; len <= 70000; ++len) {
    const sm::TagBytes a = sm::literal_tag(len, sm::kLiteralStd), q = sm::literal_tag(len, sm::kLiteralQ3);
    EXPECT((a.size == q.size && a.bytes == q.bytes) == (len != 60));
    if (len < 60) EXPECT(q.size == 1 && q.bytes == sm::literal_tag1(len) && sm::literal_tag1(len) == ((len - 1) << 2));
  }
  {
    const sm::TagBytes q = sm::literal_tag(60, sm::kLiteralQ3);
    EXPECT(q.size == 2 && q.bytes == (0xf0u | 59u << 8) && decode_bytes(tag_bytes(q)).literal_len() == 60);
    Bytes in(60);
    for (uint32_t k = 0; k < 60; ++k) in[k] = (uint8_t)(k * 37 + 11);  // 60 distinct bytes: no match
    for (int compat = 0; compat < 2; ++compat) {
      Bytes out(smo_max_compressed_length(in.size()));
      size_t n = out.size();
      EXPECT(smo_compress(in.data(), in.size(), out.data(), &n, compat) == SMO_OK);
      out.resize(n);
      EXPECT(out == literal_stream(60, compat ? sm::kLiteralStd : sm::kLiteralQ3, in));
    }
  }
  // copy_piece: every length of a piece against both offset classes' edges
  for (uint32_t len = 4; len <= 64; ++len)
    for (uint32_t off : {1u, 7u, 2047u, 2048u, 65535u}) {
      const sm::TagBytes c = sm::copy_piece(off, len);
      const sm::Tag d = decode_bytes(tag_bytes(c));
      EXPECT(c.size == ((len < 12 && off < 2048) ? 2u : 3u) && c.bytes >> (8 * c.size) == 0);
      EXPECT(d.is_copy() && d.offset() == off && d.len() == len && 1 + d.taglen == c.size);
    }
  // copy_piece_len stepped, and copy_tag_bytes' closed form, against the loop above
  for (uint32_t len = 4; len <= 65536; ++len) {
    const std::vector<uint32_t> want = copy_pieces(len);
    std::vector<uint32_t> got;
    for (uint32_t r = len; r;) {
      got.push_back(sm::copy_piece_len(r));
      r -= got.back();
    }
    const uint32_t last = want.back(), before = 3 * ((uint32_t)want.size() - 1);
    const bool ok = got == want && sm::copy_tag_bytes(1, len) == before + (last < 12 ? 2 : 3) &&
                    sm::copy_tag_bytes(2047, len) == before + (last < 12 ? 2 : 3) && sm::copy_tag_bytes(2048, len) == before + 3 &&
                    sm::copy_tag_bytes(65535, len) == before + 3;
    if (!ok) {
      EXPECT(ok);
      fprintf(stderr, "  copy length %u\n", len);
      break;
    }
  }
  // parts_verdict: a block of 1000 bytes (its literal: 3 + 1000, with header 2 more) in 4 parts of pitch 400
  struct Case {
    std::vector<uint32_t> len;
    uint32_t n;
    bool header, part0;
    uint32_t mark, bytes;
    bool literal;
    std::vector<uint32_t> before;
  };
  const uint32_t E = sm::kOutLenError;
  const Case cases[] = {
      {{100, 200, 300, 50}, 1000, false, false, 0, 650, false, {0, 100, 300, 600}},     // all parts fine
      {{400, 400, 203, 0}, 1000, false, false, 0, 1003, false, {0, 400, 800, 1003}},    // the literal's size: the parts
      {{400, 400, 204, 0}, 1000, false, false, 0, 1003, true, {0, 0, 0, 0}},            // one over: the literal
      {{400, 400, 205, 0}, 1000, true, false, 0, 1005, false, {0, 400, 800, 1005}},     // ... with the header
      {{400, 400, 206, 0}, 1000, true, false, 0, 1005, true, {0, 0, 0, 0}},
      {{100, E | 4, 300, 50}, 1000, false, false, E | 4, 0, false, {}},                 // a part's own mark
      {{100, E | 4, 401, E | 2}, 1000, false, false, E | 4 | 8 | 2, 0, false, {}},      // ... or-ed with the others
      {{0xffffffffu, 0, 0, 0}, 1000, false, true, 0xffffffffu, 0, false, {}},           // not a block
      {{400, 401, 0, 0}, 1000, false, false, E | 8, 0, false, {}},                      // a part over its pitch
      {{401, 0, 0, 0}, 1000, false, false, E | 8, 0, false, {}},
      {{1008, 0, 0, 0}, 1000, false, false, E | 8, 0, false, {}},                       // no allowance unless asked for
      {{1003, 0, 0, 0}, 1000, false, true, 0, 1003, false, {0, 1003, 1003, 1003}},      // a screened part 0
      {{1008, 0, 0, 0}, 1000, false, true, 0, 1003, true, {0, 0, 0, 0}},                // ... at lit + 5
      {{1009, 0, 0, 0}, 1000, false, true, E | 8, 0, false, {}},                        // ... and one over
      {{300, 0, 0, 0}, 100, false, true, 0, 102, true, {0, 0, 0, 0}},                   // (lit + 5 below the pitch: the pitch)
      {{401, 0, 0, 0}, 100, false, true, E | 8, 0, false, {}},
      {{0, 0, 0, 0}, 0, true, false, 0, 1, true, {0, 0, 0, 0}},                         // an empty block: its header
      {{0, 0, 0, 0}, 0, false, false, 0, 0, true, {0, 0, 0, 0}},                        // ... or nothing
  };
  for (const Case& c : cases) {
    const auto pl = exact(c.len);
    for (uint32_t j = 0; j < 4; ++j) {
      const sm::PartsVerdict v = sm::parts_verdict(pl.get(), 4, j, 400, c.n, c.header, c.part0);
      bool ok = v.mark == c.mark;
      if (!c.mark) ok = ok && v.bytes == c.bytes && v.literal == c.literal && v.before == c.before[j];
      if (!ok) {
        EXPECT(ok);
        fprintf(stderr, "  parts case %zu, part %u: mark %x bytes %u before %u literal %d\n", (size_t)(&c - cases), j, v.mark,
                v.bytes, v.before, (int)v.literal);
      }
    }
  }
}

// ---- scratch layouts --------------------------------------------------------------------------

struct Array {
  const void* p;
  size_t need;  // the bytes the kernels' interfaces (sm_internal.h) document
};
void expect_layout(const uint8_t* base, size_t end, const std::vector<Array>& arrays) {
  for (size_t i = 0; i < arrays.size(); ++i) {
    const uint8_t* p = (const uint8_t*)arrays[i].p;
    EXPECT(((uintptr_t)p & 15) == 0 && p >= base && p + arrays[i].need <= base + end);
    for (size_t j = 0; j < i; ++j) {
      const uint8_t* q = (const uint8_t*)arrays[j].p;
      EXPECT(arrays[i].need == 0 || arrays[j].need == 0 || p + arrays[i].need <= q || q + arrays[j].need <= p);
    }
  }
}

// carve(base) returns the layout's arrays and its end; a null base must measure the same end
template <typename F>
void layout_case(F&& carve) {
  std::vector<Array> arrays;
  const size_t end = carve(nullptr, &arrays);
  uint8_t* base = (uint8_t*)aligned_alloc(16, end + 16);
  arrays.clear();
  EXPECT(carve(base, &arrays) == end && end % 16 == 0);
  expect_layout(base, end, arrays);
  free(base);
}

void check_carves() {
  for (size_t n : {(size_t)0, (size_t)1, (size_t)3, (size_t)1000}) {
    for (bool decode : {false, true})
      layout_case([&](void* b, std::vector<Array>* a) {
        const sm::BatchTables t = sm::carve_batch(b, n, decode);
        *a = {{t.in_off, 8 * n}, {t.out_off, 8 * n}, {t.in_len, 4 * n}, {t.out_len, 4 * n}};
        if (decode) a->insert(a->end(), {{t.out_cap, 4 * n}, {t.status, 4 * n}});
        return t.end;
      });
    layout_case([&](void* b, std::vector<Array>* a) {
      const sm::FragTables t = sm::carve_frags(b, n);
      *a = {{t.in_off, 8 * n}, {t.out_off, 8 * n}, {t.dst_off, 8 * n}, {t.in_len, 4 * n}, {t.out_len, 4 * n}, {t.part_len, 4 * 256}};
      return t.end;
    });
    layout_case([&](void* b, std::vector<Array>* a) {  // (n chunks, n fragments)
      const sm::ParallelScratch t = sm::carve_parallel(b, n, n);
      *a = {{t.rec, n * 64 * 8}, {t.frags, n * 16}, {t.st, n * 4}};
      return t.end;
    });
    for (size_t size : {(size_t)0, n})  // (size 0: path_first_error's use)
      layout_case([&](void* b, std::vector<Array>* a) {
        const sm::OriginScratch t = sm::carve_origin(b, size, n);
        *a = {{t.P, size * 4}, {t.path, n * 16}, {t.st, n * 4}, {t.pend, 4}};
        return t.end;
      });
    for (size_t rounds : {(size_t)1, (size_t)3})
      layout_case([&](void* b, std::vector<Array>* a) {
        const sm::SmallScratch t = sm::carve_small(b, n, rounds);
        *a = {{t.rec, n * 64 * 8 + n * 4 * 4 * 16}, {t.path, n * 16}, {t.ctl, 4 * (4 + rounds)}};
        return t.end;
      });
  }
  layout_case([&](void* b, std::vector<Array>* a) {
    const sm::SingleMeta t = sm::carve_single(b);
    *a = {{t.off, 8}, {t.in_len, 4}, {t.cap, 4}, {t.out_len, 8}};
    EXPECT((const void*)t.status == (const void*)(t.out_len + 1));  // the pair launch_to_host reads
    return t.end;
  });
  static_assert(sizeof(sm::StreamFrag) == 16 && sizeof(sm::OriginPath) == 16, "the kernels' element sizes");
  static_assert(sm::kIdxEntries == 64 && sm::kDeepChains * sm::kDeepLevels == 16 && sm::kMaxParts == 256, "as counted above");
}

Bytes read_file(const char* path) {
  Bytes b;
  FILE* f = fopen(path, "rb");
  if (!f) return b;
  uint8_t buf[65536];
  for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) b.insert(b.end(), buf, buf + k);
  fclose(f);
  return b;
}

}  // namespace

int main(int argc, char** argv) {
  const Bytes text = argc > 1 ? read_file(argv[1]) : Bytes();
  if (text.size() < 150000) {
    fprintf(stderr, "usage: sm_host_check <text file of at least 150000 bytes>\n");
    return 2;
  }
  check_literal_only();
  walk_case(oracle_compress(Bytes(text.begin(), text.begin() + 70000)));
  Bytes random(70000);
  uint32_t x = 12345;
  for (uint8_t& b : random) b = (uint8_t)((x = x * 1664525u + 1013904223u) >> 24);
  walk_case(oracle_compress(random));
  uint32_t declared = 0;
  walk_case(hand_stream(&declared));
  check_paths(text);
  check_shards();
  check_lengths();
  check_varint();
  check_tags();
  check_checks();
  check_varint_rule();
  check_emit_rules();
  check_carves();
  if (failures) {
    fprintf(stderr, "sm_host_check: %d failure(s)\n", failures);
    return 1;
  }
  printf("sm_host_check: ok\n");
  return 0;
}
