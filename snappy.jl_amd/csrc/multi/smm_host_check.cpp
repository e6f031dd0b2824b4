// smm_host_check.cpp -- stand-alone driver of smm_host.cpp (no device, no HIP): the index rules of
// smm_uncompress_device over every structural case, on heap buffers of exactly the documented sizes,
// so that AddressSanitizer and UBSan (make host_check) see any read past an array that an index
// value could cause.  The rules are the device plan's own code (smm_plan.h).  Then smm_index_host,
// the rule that builds an index, over streams built from tag bytes on heap buffers of exactly the
// streams' size: a walk that read past a stream's end, or wrote past its entries, stops here.
// Then smm_range_plan, the plan of the ranged decode (smm_range.h): every case alone on heap arrays
// of exactly the documented sizes, so an entry or a frag_first word read that the rules do not allow
// is a read past an array.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "smm_plan.h"
#include "smm_range.h"

namespace {

int failures = 0;

#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      ++failures;                                                 \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);  \
    }                                                             \
  } while (0)

template <typename T>
std::unique_ptr<T[]> exact(const std::vector<T>& v) {  // a heap array of exactly v.size() elements
  std::unique_ptr<T[]> p(new T[v.size()]);
  if (!v.empty()) memcpy(p.get(), v.data(), v.size() * sizeof(T));
  return p;
}

std::vector<uint8_t> varint(uint32_t v) {
  std::vector<uint8_t> o;
  while (v >= 0x80) {
    o.push_back((uint8_t)(v | 0x80));
    v >>= 7;
  }
  o.push_back((uint8_t)v);
  return o;
}

struct Stream {
  std::vector<uint8_t> bytes;
  uint32_t cap;
};

// a stream's bytes: header, then filler (the rules never look behind the header)
Stream make(uint32_t declared, uint32_t total_bytes, uint32_t cap) {
  Stream s{varint(declared), cap};
  while (s.bytes.size() < total_bytes) s.bytes.push_back(0xfc);
  s.bytes.resize(total_bytes);
  return s;
}

std::vector<uint8_t> run(const std::vector<Stream>& streams, uint32_t max_fragments, const std::vector<uint32_t>* first,
                         const std::vector<uint32_t>* pos) {
  std::vector<uint8_t> in;
  std::vector<uint64_t> off;
  std::vector<uint32_t> len, cap;
  for (const Stream& s : streams) {
    off.push_back(in.size());
    len.push_back((uint32_t)s.bytes.size());
    cap.push_back(s.cap);
    in.insert(in.end(), s.bytes.begin(), s.bytes.end());
  }
  const uint32_t n = (uint32_t)streams.size();
  if (in.empty()) in.push_back(0);
  auto d_in = exact(in);
  auto d_off = exact(off);
  auto d_len = exact(len);
  auto d_cap = exact(cap);
  std::unique_ptr<uint32_t[]> d_first, d_pos;
  if (first) {
    EXPECT(first->size() == n + 1);
    std::vector<uint32_t> p = *pos;
    p.resize(max_fragments, 0xdeadbeefu);  // exactly max_fragments entries
    d_first = exact(*first);
    d_pos = exact(p);
  }
  std::unique_ptr<uint8_t[]> indexed(new uint8_t[n ? n : 1]);
  const sm_status st = smm_index_check(d_in.get(), d_off.get(), d_len.get(), n, max_fragments, d_cap.get(), d_first.get(),
                                       d_pos.get(), indexed.get());
  EXPECT(st == SM_OK);
  return std::vector<uint8_t>(indexed.get(), indexed.get() + n);
}

typedef std::vector<uint32_t> U;
typedef std::vector<uint8_t> B;

// ---- smm_index_host: streams built from tag bytes, the expected entries worked out by hand --------
void put_lit(B& s, uint32_t n) {  // a literal of n filler bytes: the tag, 0..3 length bytes, the bytes
  const uint32_t m = n - 1;
  if (m < 60) {
    s.push_back((uint8_t)(m << 2));
  } else {
    const uint32_t k = m < 256 ? 1 : m < 65536 ? 2 : 3;
    s.push_back((uint8_t)((59 + k) << 2));
    for (uint32_t i = 0; i < k; ++i) s.push_back((uint8_t)(m >> (8 * i)));
  }
  s.insert(s.end(), n, (uint8_t)'a');
}
void put_copy(B& s, uint32_t offset, uint32_t len) {  // the three-byte copy
  s.push_back((uint8_t)(2 | ((len - 1) << 2)));
  s.push_back((uint8_t)offset);
  s.push_back((uint8_t)(offset >> 8));
}
B stream_of(uint32_t declared, const U& lits) {
  B s = varint(declared);
  for (uint32_t n : lits) put_lit(s, n);
  return s;
}

struct IndexResult {
  sm_status st;
  U first, pos;  // pos: max_fragments entries and `guard` more behind them
  B built;
  std::vector<int32_t> status;
};
constexpr uint32_t kGuard = 0xdeadbeefu;

// One call over heap buffers of exactly the streams' size.  len_as: a length to pass instead of the
// first stream's own (an error mark); caps empty: no cap array.
IndexResult index_run(const std::vector<B>& streams, const U& caps, uint32_t max_fragments, uint32_t guard = 2,
                      uint32_t len_as = 0) {
  B in;
  std::vector<uint64_t> off;
  U len;
  for (const B& s : streams) {
    off.push_back(in.size());
    len.push_back((uint32_t)s.size());
    in.insert(in.end(), s.begin(), s.end());
  }
  if (len_as) len[0] = len_as;
  const uint32_t n = (uint32_t)streams.size();
  if (in.empty()) in.push_back(0);
  auto d_in = exact(in);
  auto d_off = exact(off);
  auto d_len = exact(len);
  auto d_cap = exact(caps);
  IndexResult r;
  auto first = exact(U(n + 1, kGuard));
  auto pos = exact(U(max_fragments + guard, kGuard));
  auto built = exact(B(n ? n : 1, 7));
  auto status = exact(std::vector<int32_t>(n ? n : 1, -1));
  r.st = smm_index_host(d_in.get(), d_off.get(), d_len.get(), n, max_fragments, caps.empty() ? nullptr : d_cap.get(),
                        first.get(), pos.get(), built.get(), status.get());
  r.first.assign(first.get(), first.get() + n + 1);
  r.pos.assign(pos.get(), pos.get() + max_fragments + guard);
  r.built.assign(built.get(), built.get() + n);
  r.status.assign(status.get(), status.get() + n);
  return r;
}

void index_cases() {
  const uint32_t G = kGuard, K = 65536;
  const std::vector<int32_t> ok1 = {SM_OK};
  // one stream per call: {entries..., guards}
  auto one = [&](const B& s, uint32_t m, const U& want_pos, uint8_t want_built, uint32_t cap = 0xffffffffu) {
    const IndexResult r = index_run({s}, cap == 0xffffffffu ? U{} : U{cap}, m);
    U want = want_pos;
    const uint32_t cnt = (uint32_t)want_pos.size();
    want.resize(m + 2, G);
    EXPECT(r.st == SM_OK && r.status == ok1);
    EXPECT(r.first == (U{0, cnt}));
    EXPECT(r.pos == want);
    EXPECT(r.built == B{want_built});
  };
  EXPECT(varint(K + 1).size() == 3);
  // a 65,536-byte literal (tag, two length bytes) ends exactly on the multiple; D = 65,537
  one(stream_of(K + 1, {K, 1}), 2, {3, 3 + 3 + K}, 1);
  one(stream_of(K + 1, {K, 1}), 5, {3, 3 + 3 + K}, 1);  // (a looser bound: the rest is untouched)
  // ... in short tags: 1,092 literals of 60 bytes, one of 16, then the last byte
  {
    U lits(1092, 60);
    lits.push_back(16);
    lits.push_back(1);
    one(stream_of(K + 1, lits), 2, {3, 3 + 1092 * 61 + 17}, 1);
    lits[1092] = 17;  // the short literal straddles the multiple
    lits.push_back(3);
    one(stream_of(K + 5, lits), 2, {0, 0}, 0);
  }
  {  // copies up to the multiple (offset 1, length 64), one byte longer: crosses
    B s = varint(K + 5);
    put_lit(s, 64);
    for (uint32_t i = 0; i < 1022; ++i) put_copy(s, 1, 64);
    B t = s;
    put_copy(s, 1, 64);
    put_lit(s, 5);
    one(s, 2, {3, 3 + 66 + 3 * 1023}, 1);
    put_copy(t, 1, 60);
    put_copy(t, 1, 4);
    put_lit(t, 5);
    one(t, 2, {3, 3 + 66 + 3 * 1024}, 1);
    t = varint(K + 5);
    put_lit(t, 64);
    for (uint32_t i = 0; i < 1022; ++i) put_copy(t, 1, 64);
    put_copy(t, 1, 63);
    put_copy(t, 1, 4);
    put_lit(t, 2);
    one(t, 2, {0, 0}, 0);
  }
  one(stream_of(70010, {70000, 10}), 2, {0, 0}, 0);               // a 70,000-byte literal crosses
  one(stream_of(2 * K + 5, {K, K, 5}), 3, {3, 3 + 3 + K, 3 + 2 * (3 + K)}, 1);  // lands exactly, then more
  one(stream_of(140010, {140000, 10}), 3, {0, 0, 0}, 0);          // a literal crosses two multiples
  {
    B s = stream_of(2 * K + 5, {K, K, 5});
    s.resize(3 + 3 + K + 100);  // cut before the last multiple
    one(s, 3, {0, 0, 0}, 0);
    s = stream_of(K + 1, {K});  // the multiple is reached exactly at x == n
    one(s, 2, {0, 0}, 0);
    s.push_back(0);             // one stray byte there: a tag starts on it
    one(s, 2, {3, 3 + 3 + K}, 1);
    s = varint(K + 1);          // nothing behind the header
    one(s, 2, {0, 0}, 0);
  }
  one(stream_of(K + 1, {K, 1}), 2, {}, 0, K);          // D > cap: no entries
  one(stream_of(K + 1, {K, 1}), 2, {3, 3 + 3 + K}, 1, K + 1);
  one(B{0x85, 0x80}, 2, {}, 0);                         // a varint that does not end
  one(B{0xff, 0xff, 0xff, 0xff, 0x10, 0, 0}, 2, {}, 0);
  one(B{}, 2, {}, 0);                                   // n = 0
  one(stream_of(0, {}), 2, {}, 0);                      // D = 0
  one(stream_of(1, {1}), 2, {1}, 0);                    // D = 1: the entry is hv, not built
  one(stream_of(K, {K}), 2, {3}, 0);                    // D = 65,536
  {  // n an error mark: nothing is read
    const IndexResult r = index_run({B{0x85, 0x80, 0x0c}}, {}, 2, 2, 0xfff00000u);
    EXPECT(r.st == SM_OK && r.first == (U{0, 0}) && r.built == B{0} && r.pos == (U{G, G, G, G}) && r.status == ok1);
  }
  {  // a batch: the scan, a failed stream's zeros between its neighbours, the guards behind
    const std::vector<B> v = {stream_of(1, {1}), stream_of(K + 1, {K, 1}), B{}, stream_of(70010, {70000, 10}),
                              stream_of(2 * K + 5, {K, K, 5})};
    IndexResult r = index_run(v, {}, 8, 3);
    EXPECT(r.st == SM_OK && r.first == (U{0, 1, 3, 3, 5, 8}) && r.built == (B{0, 1, 0, 0, 1}));
    EXPECT(r.pos == (U{1, 3, 3 + 3 + K, 0, 0, 3, 3 + 3 + K, 3 + 2 * (3 + K), G, G, G}));
    EXPECT(r.status == std::vector<int32_t>(5, SM_OK));
    r = index_run(v, {}, 7, 3);  // one entry too many
    EXPECT(r.st == SM_OK && r.first == U(6, 0) && r.built == B(5, 0) && r.pos == U(10, G));
    EXPECT(r.status == std::vector<int32_t>(5, SM_ERR_ARGUMENT));
  }
  {
    uint32_t first = 9;
    EXPECT(smm_index_host(nullptr, nullptr, nullptr, 0, 0, nullptr, &first, nullptr, nullptr, nullptr) == SM_OK && first == 0);
    EXPECT(smm_index_host(nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == SM_ERR_ARGUMENT);
  }
}

// ---- smm_range_plan ------------------------------------------------------------------------------------
struct Range {
  uint32_t s, lo, len;
};
struct PlanResult {
  sm_status st;
  U first, count;
  std::vector<int32_t> status;
  uint64_t total;
};
const uint32_t kAll = 0xffffffffu;

// One call: the streams' bytes, frag_first, nentries entries of pos and the ranges each on a heap
// array of exactly its size.  len_as: a length to pass instead of stream 1's own.
PlanResult plan_run(const std::vector<Stream>& streams, const U& first, const U& pos, const std::vector<Range>& ranges,
                    uint32_t bound = kAll, uint32_t len_as = 0) {
  B in;
  std::vector<uint64_t> off;
  U len, rs, lo, ln;
  for (const Stream& s : streams) {
    off.push_back(in.size());
    len.push_back((uint32_t)s.bytes.size());
    in.insert(in.end(), s.bytes.begin(), s.bytes.end());
  }
  if (len_as) len[1] = len_as;
  for (const Range& r : ranges) {
    rs.push_back(r.s);
    lo.push_back(r.lo);
    ln.push_back(r.len);
  }
  const uint32_t n = (uint32_t)streams.size(), k = (uint32_t)ranges.size();
  EXPECT(first.size() == n + 1);
  auto d_in = exact(in);
  auto d_off = exact(off);
  auto d_len = exact(len);
  auto d_first = exact(first);
  auto d_pos = exact(pos);
  auto d_rs = exact(rs);
  auto d_lo = exact(lo);
  auto d_ln = exact(ln);
  auto o_first = exact(U(k, kGuard));
  auto o_count = exact(U(k, kGuard));
  auto o_status = exact(std::vector<int32_t>(k, -1));
  PlanResult r;
  r.total = 77;
  r.st = smm_range_plan(d_in.get(), d_off.get(), d_len.get(), n, d_first.get(), d_pos.get(), (uint32_t)pos.size(),
                        d_rs.get(), d_lo.get(), d_ln.get(), k, bound, o_first.get(), o_count.get(), o_status.get(), &r.total);
  r.first.assign(o_first.get(), o_first.get() + k);
  r.count.assign(o_count.get(), o_count.get() + k);
  r.status.assign(o_status.get(), o_status.get() + k);
  // every output pointer may be NULL: the same return
  EXPECT(smm_range_plan(d_in.get(), d_off.get(), d_len.get(), n, d_first.get(), d_pos.get(), (uint32_t)pos.size(),
                        d_rs.get(), d_lo.get(), d_ln.get(), k, bound, nullptr, nullptr, nullptr, nullptr) == r.st);
  return r;
}

void range_cases() {
  const uint32_t K = 65536, D3 = 196600, A = SM_ERR_ARGUMENT;
  typedef std::vector<int32_t> S;
  EXPECT(smm_range_fragment_count(65535, 2) == 2 && smm_range_fragment_count(65536, 65536) == 1);
  EXPECT(smm_range_fragment_count(0xffffffffu, 2) == 2 && smm_range_fragment_count(0, 0xffffffffu) == 65536);
  EXPECT(smm_range_fragment_count(0, 0) == 0 && smm_range_fragment_count(12345, 0) == 0 && smm_range_fragment_count(0xffffffffu, 0) == 0);
  EXPECT(smm_range_fragment_count(0, 1) == 1 && smm_range_fragment_count(0, K) == 1 && smm_range_fragment_count(0, K + 1) == 2);
  EXPECT(smm_range_fragment_count(0xffffffffu, 0xffffffffu) == 65537);
  EXPECT(smm_range_scratch_bytes(1, 17) >= 2 * K && smm_range_scratch_bytes(1, 17) < 3 * K);
  EXPECT(smm_range_scratch_bytes(10, 3) >= 3 * K && smm_range_scratch_bytes(10, 3) < 4 * K);
  EXPECT(smm_range_scratch_bytes(0, 0) >= K && smm_range_scratch_bytes(3, 9) - smm_range_scratch_bytes(3, 5) > K);
  {  // the placement: a 3-fragment stream with D = 131,073, range (1, 131,072)
    const smm::Place p0 = smm::fragment_place(131073, 0, 3, 1, 131072), p1 = smm::fragment_place(131073, 1, 3, 1, 131072),
                     p2 = smm::fragment_place(131073, 2, 3, 1, 131072);
    EXPECT(p0.edge == 1 && p0.src == 1 && p0.n == 65535 && p0.dst == 0);
    EXPECT(p1.edge == 0 && p1.n == K && p1.dst == 65535);
    EXPECT(p2.edge == 1 && p2.src == 0 && p2.n == 1 && p2.dst == 131071);
    EXPECT(smm::range_edges(131073, 3, 0, 3, 1, 131072) == 2 && smm::edge_which(131073, 3, 0, 2, 1, 131072) == 1);
    EXPECT(smm::range_edges(131073, 3, 0, 3, 0, 131073) == 1 && smm::range_edges(131073, 3, 0, 2, 0, 131072) == 0);
    EXPECT(smm::range_edges(131073, 3, 1, 2, K, K + 1) == 1);  // the short last fragment, even whole: an edge slot
    EXPECT(smm::range_edges(131072, 2, 0, 2, 0, 131072) == 0 && smm::range_edges(131073, 3, 0, 1, 5, 7) == 1);
    EXPECT(smm::edge_which(131073, 3, 0, 1, 0, K + 5) == 0);   // the first fragment direct: the last takes slot 0
  }
  // a short stream (1 entry), a three-fragment stream, an empty stream (0 entries), a two-fragment one
  const std::vector<Stream> base = {make(100, 60, 0), make(D3, 300, 0), make(0, 1, 0), make(65537, 90, 0)};
  const U first = {0, 1, 4, 4, 6};
  const U pos = {1, 3, 100, 200, 3, 89};
  const std::vector<Range> all = {{1, 0, D3}, {1, 65535, 2}, {1, K, K}, {0, 10, 90}, {3, K, 1}, {1, D3 - 1, 1}, {3, 0, 65537}};
  {
    const PlanResult r = plan_run(base, first, pos, all);
    EXPECT(r.st == SM_OK && r.total == 3 + 2 + 1 + 1 + 1 + 1 + 2);
    EXPECT(r.first == (U{0, 0, 1, 0, 1, 2, 0}) && r.count == (U{3, 2, 1, 1, 1, 1, 2}) && r.status == S(7, SM_OK));
  }
  // one range per call from here on: {first, count, status}
  auto one = [&](const std::vector<Stream>& v, const U& f, const U& p, Range g, uint32_t wf, uint32_t wc, int32_t ws,
                 uint32_t len_as = 0) {
    const PlanResult r = plan_run(v, f, p, {g}, kAll, len_as);
    EXPECT(r.st == SM_OK && r.first == U{wf} && r.count == U{wc} && r.status == S{ws} && r.total == wc);
  };
  {  // hostile frag_first: decreasing; past nentries; wild words of streams the range does not name
    U f = {0, 4, 1, 4, 6};
    one(base, f, pos, {1, 0, 10}, 0, 0, A);
    one(base, f, pos, {0, 0, 10}, 0, 0, A);  // (entries [0, 4) of a stream that declares 100)
    one(base, f, pos, {3, K, 1}, 1, 1, SM_OK);
    f = {0, 1, 4, 4, 7};
    one(base, f, pos, {3, K, 1}, 0, 0, A);
    one(base, f, pos, {1, K, 1}, 1, 1, SM_OK);
    f = {0xfffffff0u, 1, 4, 0xffffffffu, 0};
    one(base, f, pos, {1, K, 1}, 1, 1, SM_OK);
    one(base, f, pos, {0, 0, 1}, 0, 0, A);
    one(base, f, pos, {3, 0, 1}, 0, 0, A);
    f = {0, 1, 0xffffffffu, 0xffffffffu, 0xffffffffu};
    one(base, f, pos, {1, 0, 1}, 0, 0, A);
  }
  {  // positions: zero, decreasing, equal, at and past n, a first position that is not hv
    U p = pos;
    p[2] = 0;  // 3, 0, 200
    one(base, first, p, {1, K, 10}, 1, 1, A);
    one(base, first, p, {1, 0, 10}, 0, 1, A);        // (fragment 0 ends where fragment 1 starts)
    one(base, first, p, {1, 2 * K, 10}, 2, 1, SM_OK);  // (the last fragment reads its own entry alone)
    one(base, first, U{1, 0, 0, 0, 3, 89}, {1, 0, D3}, 0, 3, A);  // zeroed entries: no index was built
    p = pos;
    p[2] = 250;  // 3, 250, 200
    one(base, first, p, {1, 0, 10}, 0, 1, SM_OK);
    one(base, first, p, {1, K, 10}, 1, 1, A);
    one(base, first, p, {1, 2 * K, 10}, 2, 1, SM_OK);
    one(base, first, p, {1, 0, D3}, 0, 3, A);
    p = pos;
    p[3] = 100;  // 3, 100, 100
    one(base, first, p, {1, K, 10}, 1, 1, A);
    one(base, first, p, {1, 0, 10}, 0, 1, SM_OK);
    one(base, first, p, {1, 2 * K, 10}, 2, 1, SM_OK);
    p[3] = 300;  // at n
    one(base, first, p, {1, 2 * K, 10}, 2, 1, A);
    one(base, first, p, {1, K, 10}, 1, 1, SM_OK);
    p[3] = 299;
    one(base, first, p, {1, 2 * K, 10}, 2, 1, SM_OK);
    p[3] = 0xffffffffu;
    one(base, first, p, {1, 2 * K, 10}, 2, 1, A);
    one(base, first, p, {1, K, 10}, 1, 1, A);
    one(base, first, p, {1, 0, 10}, 0, 1, SM_OK);
    p = pos;
    p[1] = 2;  // not hv
    one(base, first, p, {1, 0, 10}, 0, 1, A);
    one(base, first, p, {1, K, 10}, 1, 1, SM_OK);
    p[1] = 4;
    one(base, first, p, {1, 0, 10}, 0, 1, A);
    p = pos;
    p[0] = 0;  // the short stream's one entry
    one(base, first, p, {0, 0, 100}, 0, 1, A);
    p[0] = 1;
    one(base, first, p, {0, 0, 100}, 0, 1, SM_OK);
    p[1] = 1;  // a position below hv in a later fragment
    p[2] = 2;
    one(base, first, p, {1, K, 10}, 1, 1, A);
  }
  {  // a count mismatch, either way (the neighbour keeps its own count)
    U f = {0, 1, 3, 3, 5}, p = {1, 3, 100, 3, 89};
    one(base, f, p, {1, 0, 10}, 0, 0, A);
    one(base, f, p, {3, 0, 10}, 0, 1, SM_OK);
    f = {0, 1, 5, 5, 7};
    p = {1, 3, 100, 200, 250, 3, 89};
    one(base, f, p, {1, 0, 10}, 0, 0, A);
    one(base, f, p, {3, 0, 10}, 0, 1, SM_OK);
  }
  // lo + len past D, and past 2^32
  one(base, first, pos, {1, D3 - 1, 2}, 0, 0, A);
  one(base, first, pos, {1, D3, 1}, 0, 0, A);
  one(base, first, pos, {1, 0, D3 + 1}, 0, 0, A);
  one(base, first, pos, {1, 0xffffffffu, 2}, 0, 0, A);
  one(base, first, pos, {1, 1, 0xffffffffu}, 0, 0, A);
  one(base, first, pos, {1, 0xffffffffu, 0xffffffffu}, 0, 0, A);
  one(base, first, pos, {2, 0, 1}, 0, 0, A);   // D = 0 holds no byte
  one(base, first, pos, {4, 0, 1}, 0, 0, A);   // the stream number is nstreams
  one(base, first, pos, {kAll, 0, 1}, 0, 0, A);
  {  // len == 0: SM_OK whatever else holds, nothing read
    std::vector<Stream> v = base;
    v[1].bytes = {0x85, 0x80};  // a varint that does not end
    one(v, first, pos, {1, 0, 1}, 0, 0, A);
    one(v, first, pos, {1, 0, 0}, 0, 0, SM_OK);
    one(v, first, pos, {1, 0xffffffffu, 0}, 0, 0, SM_OK);
    one(v, first, pos, {99, 5, 0}, 0, 0, SM_OK);
    one(base, U{9, 8, 7, 6, 5}, pos, {1, 7, 0}, 0, 0, SM_OK);
    v[1].bytes = {0xff, 0xff, 0xff, 0xff, 0x10, 0, 0, 0};
    one(v, first, pos, {1, 0, 1}, 0, 0, A);
    v[1].bytes.clear();
    one(v, first, pos, {1, 0, 1}, 0, 0, A);
    // a length that is an error mark: nothing of the stream is read (its three bytes would parse)
    v[1].bytes = {0x85, 0x80, 0x0c};
    one(v, first, pos, {1, 0, 1}, 0, 0, A, 0xfff00000u);
    one(v, first, pos, {1, 0, 0}, 0, 0, SM_OK, 0xfff00000u);
  }
  {  // the bound: one below the need, the need
    PlanResult r = plan_run(base, first, pos, all, 10);
    EXPECT(r.st == SM_BUFFER_TOO_SMALL && r.total == 11 && r.status == S(7, A) && r.count == (U{3, 2, 1, 1, 1, 1, 2}));
    r = plan_run(base, first, pos, all, 11);
    EXPECT(r.st == SM_OK && r.total == 11 && r.status == S(7, SM_OK));
    r = plan_run(base, first, pos, {{1, 0, 1}, {1, 5, 0}}, 0);  // (an empty range's status too)
    EXPECT(r.st == SM_BUFFER_TOO_SMALL && r.total == 1 && r.status == S(2, A));
    r = plan_run(base, first, pos, {{1, 5, 0}, {9, 0, 1}}, 0);  // nothing to decode fits a bound of 0
    EXPECT(r.st == SM_OK && r.total == 0 && r.status == (S{SM_OK, A}));
  }
  {  // no ranges; NULL inputs
    uint64_t total = 5;
    EXPECT(smm_range_plan(nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, 0, nullptr,
                          nullptr, nullptr, &total) == SM_OK && total == 0);
    const uint32_t z = 0;
    EXPECT(smm_range_plan(nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0, &z, &z, &z, 1, 0, nullptr, nullptr, nullptr,
                          &total) == SM_ERR_ARGUMENT);
  }
}

}  // namespace

int main() {
  const uint32_t D3 = 196600;  // three fragments, a 3-byte varint
  EXPECT(smm_fragment_count(0) == 0 && smm_fragment_count(1) == 1 && smm_fragment_count(65535) == 1);
  EXPECT(smm_fragment_count(65536) == 1 && smm_fragment_count(65537) == 2 && smm_fragment_count(131072) == 2);
  EXPECT(smm_fragment_count(131073) == 3 && smm_fragment_count(196613) == 4 && smm_fragment_count(D3) == 3);
  EXPECT(smm_fragment_count(0x80000000ull) == 32768 && smm_fragment_count(0xffffffffull) == 65536);
  EXPECT(smm_scratch_bytes(0, 0) >= 256 && smm_scratch_bytes(3, 8) >= 8 * 76544u);
  EXPECT(varint(D3).size() == 3);

  // a short stream (1 entry), a three-fragment stream, an empty stream (0 entries), a two-fragment one
  const std::vector<Stream> base = {make(100, 60, 100), make(D3, 300, D3), make(0, 1, 0), make(65537, 90, 70000)};
  const U first = {0, 1, 4, 4, 6};
  const U pos = {1, 3, 100, 200, 3, 89};
  EXPECT(run(base, 6, &first, &pos) == (B{0, 1, 0, 1}));
  EXPECT(run(base, 9, &first, &pos) == (B{0, 1, 0, 1}));  // (a looser bound)
  EXPECT(run(base, 6, nullptr, nullptr) == (B{0, 0, 0, 0}));  // no index
  const U first0 = {0}, pos0 = {};
  EXPECT(run({}, 0, &first0, &pos0) == B{});  // no streams

  {  // count off by one, either way (the neighbours keep their own counts)
    U f = {0, 1, 3, 3, 5}, p = {1, 3, 100, 3, 89};
    EXPECT(run(base, 5, &f, &p) == (B{0, 0, 0, 1}));
    f = {0, 1, 5, 5, 7};
    p = {1, 3, 100, 200, 250, 3, 89};
    EXPECT(run(base, 7, &f, &p) == (B{0, 0, 0, 1}));
  }
  {  // equal neighbouring positions; decreasing positions
    U p = pos;
    p[2] = 3;
    EXPECT(run(base, 6, &first, &p) == (B{0, 0, 0, 1}));
    p = pos;
    p[3] = 100;
    EXPECT(run(base, 6, &first, &p) == (B{0, 0, 0, 1}));
    p = pos;
    p[2] = 250;  // 3, 250, 200
    EXPECT(run(base, 6, &first, &p) == (B{0, 0, 0, 1}));
  }
  {  // the first position is not the varint's length
    U p = pos;
    p[1] = 2;
    EXPECT(run(base, 6, &first, &p) == (B{0, 0, 0, 1}));
    p[1] = 4;
    EXPECT(run(base, 6, &first, &p) == (B{0, 0, 0, 1}));
    p = pos;
    p[4] = 0;
    EXPECT(run(base, 6, &first, &p) == (B{0, 1, 0, 0}));
  }
  {  // the last position at and past the stream's length (and far past it)
    U p = pos;
    p[3] = 300;
    EXPECT(run(base, 6, &first, &p) == (B{0, 0, 0, 1}));
    p[3] = 299;
    EXPECT(run(base, 6, &first, &p) == (B{0, 1, 0, 1}));
    p[3] = 0xffffffffu;
    EXPECT(run(base, 6, &first, &p) == (B{0, 0, 0, 1}));
    p = pos;
    p[5] = 90;
    EXPECT(run(base, 6, &first, &p) == (B{0, 1, 0, 0}));
    p[2] = 0xfffffff0u;  // a middle position past everything
    EXPECT(run(base, 6, &first, &p) == (B{0, 0, 0, 0}));
  }
  {  // d_frag_first: decreasing, not from 0, past max_fragments, wild values
    U f = {0, 4, 1, 4, 6};
    EXPECT(run(base, 6, &f, &pos) == (B{0, 0, 0, 0}));
    f = {1, 1, 4, 4, 6};
    EXPECT(run(base, 6, &f, &pos) == (B{0, 0, 0, 0}));
    EXPECT(run(base, 5, &first, &pos) == (B{0, 0, 0, 0}));  // frag_first[n] = 6 > max_fragments
    f = {0, 0xfffffffdu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
    EXPECT(run(base, 6, &f, &pos) == (B{0, 0, 0, 0}));
    f = {0, 0, 0, 0, 0};
    EXPECT(run(base, 6, &f, &pos) == (B{0, 0, 0, 0}));
  }
  {  // the header: truncated, five bytes with a bad last one, declared length above the room, at most 64 KiB
    std::vector<Stream> v = base;
    v[1].bytes = {0x85, 0x80};  // a varint that does not end
    U p = pos;
    EXPECT(run(v, 6, &first, &p) == (B{0, 0, 0, 1}));
    v[1].bytes = {0xff, 0xff, 0xff, 0xff, 0x10, 0, 0, 0};
    EXPECT(run(v, 6, &first, &p) == (B{0, 0, 0, 1}));
    v[1].bytes.clear();  // an empty stream with entries
    EXPECT(run(v, 6, &first, &p) == (B{0, 0, 0, 1}));
    v = base;
    v[1].cap = D3 - 1;
    EXPECT(run(v, 6, &first, &pos) == (B{0, 0, 0, 1}));
    v = base;
    v[3] = make(65536, 90, 70000);  // one fragment: the decoder in stream order takes it
    U f = {0, 1, 4, 4, 5};
    p = {1, 3, 100, 200, 3};
    EXPECT(run(v, 5, &f, &p) == (B{0, 1, 0, 0}));
  }
  {  // an error mark as a length is no candidate (and nothing of it is read)
    std::vector<uint8_t> in = {0x85, 0x80, 0x0c};
    const uint64_t off = 0;
    const uint32_t len = 0xfff00000u, cap = D3, f[2] = {0, 3}, p[3] = {3, 100, 200};
    uint8_t idx = 7;
    auto d_in = exact(in);
    EXPECT(smm_index_check(d_in.get(), &off, &len, 1, 3, &cap, f, p, &idx) == SM_OK && idx == 0);
    EXPECT(smm_index_check(d_in.get(), &off, &len, 1, 3, &cap, f, nullptr, &idx) == SM_ERR_ARGUMENT);
  }
  index_cases();
  range_cases();
  if (failures) {
    fprintf(stderr, "smm_host_check: %d failure(s)\n", failures);
    return 1;
  }
  printf("smm_host_check: ok\n");
  return 0;
}
