// smf_host_check.cpp -- stand-alone driver of the host-only framing code (smf_host.cpp), built with
// -fsanitize=address,undefined by `make host_check`.  Every buffer is a heap block of exactly the
// stream's size, so a walker that reads past a cut stream trips the sanitizer; the batched decode's
// plan (smf_streams_plan) runs over the same cases laid directly behind one another.  It also runs the
// CRC kernel's arithmetic (k_crc32c: the tables, the per-lane granule steps, the x^(128 t)
// multipliers) lane by lane on the CPU against the bytewise CRC, the slot stage's two verdict rules
// (smf_slots.h) against a table, and the kernels' shared byte mover (smc::copy_bytes) thread by thread.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../common/smc_device.h"
#include "smf_format.h"
#include "smf_range.h"
#include "smf_slots.h"
#include "smf_streams.h"

namespace {

int failures = 0;

void expect(bool ok, const char* what) {
  if (!ok) {
    std::printf("FAIL %s\n", what);
    ++failures;
  }
}

typedef std::string S;

S chunk(uint8_t type, const S& data, long len = -1) {
  const uint32_t L = len < 0 ? (uint32_t)data.size() : (uint32_t)len;
  S s;
  s += (char)type;
  s += (char)(L & 0xff);
  s += (char)((L >> 8) & 0xff);
  s += (char)((L >> 16) & 0xff);
  return s + data;
}

const S kId = S("\xff\x06\x00\x00sNaPpY", 10);

S crc_field(const S& bytes) {
  const uint32_t m = smf_crc32c_mask(smf_crc32c(bytes.data(), bytes.size()));
  S s;
  for (int i = 0; i < 4; ++i) s += (char)((m >> (8 * i)) & 0xff);
  return s;
}

S raw_chunk(const S& bytes) { return chunk(0x01, crc_field(bytes) + bytes); }

struct Result {
  smf_summary sum;
  std::vector<uint8_t> type;
  std::vector<uint64_t> off;
  std::vector<uint32_t> len, crc, ulen;
};

Result walk(const S& stream, uint32_t max_chunks = 16) {
  Result r;
  r.type.resize(max_chunks);
  r.off.resize(max_chunks);
  r.len.resize(max_chunks);
  r.crc.resize(max_chunks);
  r.ulen.resize(max_chunks);
  uint8_t* heap = (uint8_t*)std::malloc(stream.size() ? stream.size() : 1);
  std::memcpy(heap, stream.data(), stream.size());
  const smf_chunks ch{r.type.data(), r.off.data(), r.len.data(), r.crc.data(), r.ulen.data()};
  smf_index(heap, stream.size(), &ch, max_chunks, &r.sum);
  smf_summary count;
  smf_index(heap, stream.size(), nullptr, 0, &count);
  expect(count.nchunks == r.sum.nchunks && count.total_length == r.sum.total_length, "count-only walk agrees");
  std::free(heap);
  return r;
}

struct Case {
  S stream;
  int32_t status;
  uint32_t nchunks;
  uint64_t total;
};
std::vector<Case> cases;  // every status_case, for streams_cases

void status_case(const char* name, const S& stream, int32_t status, uint32_t nchunks = 0, uint64_t total = 0) {
  cases.push_back(Case{stream, status, nchunks, total});
  const Result r = walk(stream);
  if (r.sum.status != status || r.sum.nchunks != nchunks || r.sum.total_length != total) {
    std::printf("FAIL %s: status %d (want %d), chunks %u (want %u), total %llu (want %llu)\n", name, r.sum.status, status,
                r.sum.nchunks, nchunks, (unsigned long long)r.sum.total_length, (unsigned long long)total);
    ++failures;
  }
}

// k_crc32c's arithmetic, one lane after another
uint32_t crc_like_kernel(const smf::CrcLut& T, const uint8_t* p, uint32_t n) {
  const uint32_t* tab = &T.tab[0][0];
  const uint32_t head = std::min<uint32_t>(n, (16u - (uint32_t)((uintptr_t)p & 15)) & 15u);
  const uint32_t G = (n - head) / 16;
  uint32_t acc = 0;
  for (uint32_t t = 0; t < smf::kCrcThreads; ++t) {
    uint32_t s = 0;
    if (t < G) {
      uint32_t idx = (G - 1 - t) % smf::kCrcThreads;
      for (uint32_t cnt = (G - 1 - t) / smf::kCrcThreads + 1; cnt; --cnt, idx += smf::kCrcThreads) {
        uint32_t w[4];
        std::memcpy(w, p + head + 16 * (size_t)idx, 16);
        s = smf::crc_granule(tab, s, w);
      }
      s = smf::gf_mul(T.xpow[t], s);
    }
    if (t == smf::kCrcThreads - 1) {
      uint32_t h = 0xffffffffu;
      for (uint32_t i = 0; i < head; ++i) h = tab[15 * 256 + ((h ^ p[i]) & 0xff)] ^ (h >> 8);
      s ^= smf::gf_mul(smf::gf_xpow(&T, G), h);
    }
    acc ^= s;
  }
  for (uint32_t i = head + 16 * G; i < n; ++i) acc = tab[15 * 256 + ((acc ^ p[i]) & 0xff)] ^ (acc >> 8);
  return acc ^ 0xffffffffu;
}

// ---- the seek index and the range plan (smf_range.h through smf_range_plan) --------------------
// An index in heap blocks of exactly its size, so a search or a check that leaves an array trips
// the sanitizer.  The stream behind it is never read by the plan: only its length counts.
struct Index {
  uint32_t nc;
  uint64_t n;  // the framed stream's length
  uint8_t* type;
  uint64_t *pay_off, *chunk_off;
  uint32_t *pay_len, *crc, *ulen;
  // 0x01 chunks of the given lengths behind the identifier
  Index(const std::vector<uint32_t>& lens) : nc((uint32_t)lens.size()) {
    type = (uint8_t*)std::malloc(nc ? nc : 1);
    pay_off = (uint64_t*)std::malloc(8 * (size_t)(nc ? nc : 1));
    chunk_off = (uint64_t*)std::malloc(8 * ((size_t)nc + 1));
    pay_len = (uint32_t*)std::malloc(4 * (size_t)(nc ? nc : 1));
    crc = (uint32_t*)std::malloc(4 * (size_t)(nc ? nc : 1));
    ulen = (uint32_t*)std::malloc(4 * (size_t)(nc ? nc : 1));
    uint64_t pos = 10;
    for (uint32_t c = 0; c < nc; ++c) {
      type[c] = 1;
      pay_off[c] = pos + 8;
      pay_len[c] = ulen[c] = lens[c];
      crc[c] = 0;
      pos += 8 + lens[c];
    }
    n = pos;
    expect(smf_chunk_offsets(ulen, nc, chunk_off) == SM_OK, "chunk offsets");
  }
  ~Index() {
    std::free(type);
    std::free(pay_off);
    std::free(chunk_off);
    std::free(pay_len);
    std::free(crc);
    std::free(ulen);
  }
  smf_chunks chunks() const { return smf_chunks{type, pay_off, pay_len, crc, ulen}; }
  uint64_t total() const { return chunk_off[nc]; }
};

struct Planned {
  sm_status rc;
  uint32_t first, count;
  int32_t status;
  uint64_t total;
};

Planned plan_one(const Index& ix, uint64_t lo, uint64_t len, uint32_t max_range_chunks = 0xffffffffu) {
  Planned p{};
  uint64_t* a = (uint64_t*)std::malloc(16);
  a[0] = lo;
  a[1] = len;
  const smf_chunks ch = ix.chunks();
  p.rc = smf_range_plan(&ch, ix.chunk_off, ix.nc, ix.n, a, a + 1, 1, max_range_chunks, &p.first, &p.count, &p.status,
                        &p.total);
  std::free(a);
  return p;
}

// every (lo, len) of the index: the plan stays inside the arrays (the sanitizer's business) and
// inside [0, nc); touch(c) tells which ranges are expected to fail
template <typename F>
void sweep(const Index& ix, uint64_t total, const char* what, F bad_touched) {
  for (uint64_t lo = 0; lo <= total + 1; ++lo)
    for (uint64_t len = 0; len <= total + 1 - lo + 1; ++len) {
      const Planned p = plan_one(ix, lo, len);
      const bool in_bounds = p.count == 0 || (p.first < ix.nc && p.count <= ix.nc - p.first);
      if (!in_bounds || p.rc != SM_OK) {
        std::printf("FAIL %s: (%llu, %llu) leaves the index\n", what, (unsigned long long)lo, (unsigned long long)len);
        ++failures;
      }
      const int want = bad_touched(lo, len, p);
      if (want >= 0 && p.status != want) {
        std::printf("FAIL %s: (%llu, %llu) status %d, want %d\n", what, (unsigned long long)lo, (unsigned long long)len,
                    p.status, want);
        ++failures;
      }
    }
}

void range_cases() {
  // smf_chunk_offsets: 0, 1 and 257 chunks, lengths including 0 and 65536
  for (uint32_t nc : {0u, 1u, 257u}) {
    std::vector<uint32_t> lens(nc);
    for (uint32_t c = 0; c < nc; ++c) lens[c] = c % 5 == 0 ? 0u : (c % 7 == 0 ? 65536u : c * 37u % 65537u);
    const Index ix(lens);
    uint64_t at = 0;
    bool ok = true;
    for (uint32_t c = 0; c < nc; ++c) {
      ok = ok && ix.chunk_off[c] == at;
      at += lens[c];
    }
    expect(ok && ix.chunk_off[nc] == at, "chunk offsets: the scan");
  }
  expect(smf_chunk_offsets(nullptr, 1, nullptr) == SM_ERR_ARGUMENT, "chunk offsets: null");
  expect(smf_range_chunk_count(0, 0) == 0 && smf_range_chunk_count(0, 1) == 1 && smf_range_chunk_count(65535, 1) == 1 &&
             smf_range_chunk_count(65535, 2) == 2 && smf_range_chunk_count(65536, 65536) == 1 &&
             smf_range_chunk_count(1, 131072) == 3 && smf_range_chunk_count(UINT64_MAX, 2) == 0,
         "range chunk count");
  expect(smf_range_scratch_bytes(1, 0) >= 2 * 65536 && smf_range_scratch_bytes(3, 7) > smf_range_scratch_bytes(3, 6),
         "range scratch bytes");

  const std::vector<uint32_t> lens = {0, 1, 3, 0, 16, 17, 0};
  const uint64_t total = 37;
  // a good index: which chunks, and the edges of the contract
  {
    const Index ix(lens);
    sweep(ix, total, "good index", [&](uint64_t lo, uint64_t len, const Planned& p) {
      if (len == 0) return p.count == 0 ? (int)SM_OK : 99;
      if (lo + len > total) return p.count == 0 ? (int)SM_ERR_ARGUMENT : 99;
      // the chunk holding lo and the chunk holding lo + len - 1, empty ones skipped
      uint32_t f = 0, l = 0;
      for (uint32_t c = 0; c < ix.nc; ++c) {
        if (ix.ulen[c] && ix.chunk_off[c] <= lo && lo < ix.chunk_off[c + 1]) f = c;
        if (ix.ulen[c] && ix.chunk_off[c] <= lo + len - 1 && lo + len - 1 < ix.chunk_off[c + 1]) l = c;
      }
      return p.first == f && p.count == l - f + 1 ? (int)SM_OK : 99;
    });
    expect(plan_one(ix, total, 0).status == SM_OK, "lo == total, len == 0");
    expect(plan_one(ix, total, 1).status == SM_ERR_ARGUMENT, "lo == total, len == 1");
    expect(plan_one(ix, 5, UINT64_MAX - 2).status == SM_ERR_ARGUMENT, "lo + len overflows");
    expect(plan_one(ix, UINT64_MAX, 1).status == SM_ERR_ARGUMENT, "lo + len overflows to 0");
    const Planned all = plan_one(ix, 0, total);
    expect(all.rc == SM_OK && all.first == 1 && all.count == 5 && all.total == 5, "the whole stream");
    const Planned over = plan_one(ix, 0, total, 4);
    expect(over.rc == SM_BUFFER_TOO_SMALL && over.total == 5 && over.status == SM_ERR_ARGUMENT, "one slot short");
  }
  // hostile entries: exactly the ranges that touch chunk `victim` (ulen 16, content [4, 20)) fail
  const uint32_t victim = 4;
  auto touches = [&](uint64_t lo, uint64_t len) { return len && lo + len <= total && lo < 20 && lo + len > 4; };
  auto by_victim = [&](uint64_t lo, uint64_t len, const Planned&) {
    if (len == 0) return (int)SM_OK;
    if (lo + len > total) return (int)SM_ERR_ARGUMENT;
    return touches(lo, len) ? (int)SM_ERR_ARGUMENT : (int)SM_OK;
  };
  {
    Index ix(lens);
    ix.type[victim] = 7;
    sweep(ix, total, "type 7", by_victim);
  }
  {
    Index ix(lens);
    ix.pay_off[victim] = UINT64_MAX - 3;
    sweep(ix, total, "pay_off near the top", by_victim);
    ix.pay_off[victim] = ix.n - 15;  // one byte past the stream's end
    sweep(ix, total, "payload one byte past the end", by_victim);
  }
  {
    Index ix(lens);
    ix.pay_len[victim] = 15;  // a 0x01 chunk whose lengths differ
    sweep(ix, total, "0x01 lengths differ", by_victim);
  }
  // an ulen that chunk_off does not agree with; 65537 fails the size rule first
  {
    Index ix(lens);
    ix.ulen[victim] = ix.pay_len[victim] = 65537;
    sweep(ix, total, "ulen 65537", by_victim);
  }
  // hostile chunk_off: whatever it holds, the plan stays inside the arrays and never accepts a
  // chunk whose bytes are not [chunk_off[c], chunk_off[c + 1]) of its length
  auto any = [](uint64_t, uint64_t, const Planned&) { return -1; };
  {
    Index ix(lens);
    for (uint32_t c = 0; c <= ix.nc; ++c) ix.chunk_off[c] = 9;  // constant
    sweep(ix, total, "chunk_off constant", [&](uint64_t lo, uint64_t len, const Planned& p) {
      return len == 0 ? (int)SM_OK : (int)SM_ERR_ARGUMENT;  // past the "total" of 9, or chunks of no bytes
    });
  }
  {
    Index ix(lens);
    for (uint32_t c = 0; c <= ix.nc; ++c) ix.chunk_off[c] = 40 - 5 * c;  // decreasing
    sweep(ix, total, "chunk_off decreasing", [&](uint64_t lo, uint64_t len, const Planned& p) {
      return len == 0 ? (int)SM_OK : (int)SM_ERR_ARGUMENT;
    });
  }
  {
    Index ix(lens);
    for (uint32_t c = 0; c <= ix.nc; ++c) ix.chunk_off[c] = UINT64_MAX;
    sweep(ix, total, "chunk_off UINT64_MAX", [&](uint64_t lo, uint64_t len, const Planned& p) {
      return len == 0 ? (int)SM_OK : (int)SM_ERR_ARGUMENT;
    });
    expect(plan_one(ix, UINT64_MAX - 1, 1).status == SM_ERR_ARGUMENT, "chunk_off UINT64_MAX: the last byte");
    ix.chunk_off[0] = 0;  // one chunk claims everything
    sweep(ix, total, "chunk_off 0 then UINT64_MAX", any);
    expect(plan_one(ix, 7, UINT64_MAX - 7).status == SM_ERR_ARGUMENT, "a chunk of 2^64 bytes");
    ix.chunk_off[3] = 2;  // not monotone in the middle
    sweep(ix, total, "chunk_off not monotone", any);
  }
  // a stream of only empty data chunks, and one without chunks
  {
    const Index ix(std::vector<uint32_t>{0, 0, 0});
    expect(plan_one(ix, 0, 0).status == SM_OK && plan_one(ix, 0, 0).count == 0, "empty chunks: (0, 0)");
    expect(plan_one(ix, 0, 1).status == SM_ERR_ARGUMENT && plan_one(ix, 1, 0).status == SM_OK, "empty chunks: past the end");
    const Index none(std::vector<uint32_t>{});
    expect(plan_one(none, 0, 0).status == SM_OK && plan_one(none, 0, 1).status == SM_ERR_ARGUMENT, "no chunks");
    none.chunk_off[0] = 100;  // a total without chunks
    expect(plan_one(none, 0, 50).status == SM_ERR_ARGUMENT && plan_one(none, 0, 50).count == 0, "no chunks, hostile total");
  }
  // place rule: the chunk_place arithmetic for every chunk position against a byte-by-byte model
  for (uint64_t a = 0; a < 12; ++a)
    for (uint32_t u = 1; u < 8; ++u)
      for (uint64_t lo = 0; lo < 14; ++lo)
        for (uint64_t len = 1; len < 14; ++len)
          for (int pos = 0; pos < 4; ++pos) {
            const smf::Place p = smf::chunk_place(a, u, lo, len, pos & 1, pos & 2);
            bool ok;
            const bool meets = (a > lo ? a : lo) < (a + u < lo + len ? a + u : lo + len);
            if (p.status != SM_OK) ok = !(a >= lo && a + u <= lo + len) && (pos == 0 || !meets);
            else if (p.edge == 0) ok = a >= lo && a + u <= lo + len && p.dst == a - lo;
            else ok = p.n > 0 && p.src + p.n <= u && p.dst + p.n <= len && a + p.src == lo + p.dst && pos != 0 &&
                      p.edge == ((pos & 1) ? 1u : 2u);
            expect(ok, "chunk_place");
          }
}

// ---- the batched decode's plan (smf_streams.h through smf_streams_plan) --------------------------
// Every structural case as one batch, the streams directly behind one another in a heap block of
// exactly their size: a walk that leaves its stream reads its neighbour (a wrong status) or, at the
// last stream, trips the sanitizer.  Expected values are the single-stream cases' own.
void streams_cases() {
  const uint32_t k = (uint32_t)cases.size();
  std::vector<uint64_t> off(k), len(k), cap(k), out_len(k);
  std::vector<uint32_t> first(k + 1), want_first(k + 1);
  std::vector<int32_t> status(k);
  uint64_t n = 0, slots = 0;
  for (uint32_t s = 0; s < k; ++s) {
    off[s] = n;
    len[s] = cases[s].stream.size();
    n += len[s];
    cap[s] = cases[s].total;
    want_first[s] = (uint32_t)slots;
    slots += cases[s].status == SM_OK ? cases[s].nchunks : 0;
  }
  want_first[k] = (uint32_t)slots;
  uint8_t* heap = (uint8_t*)std::malloc(n);
  for (uint32_t s = 0; s < k; ++s) std::memcpy(heap + off[s], cases[s].stream.data(), len[s]);
  auto run = [&](uint32_t max_chunks, uint64_t& total) {
    return smf_streams_plan(heap, off.data(), len.data(), k, cap.data(), max_chunks, first.data(), out_len.data(),
                            status.data(), &total);
  };
  uint64_t total = 0;
  expect(run((uint32_t)slots, total) == SM_OK && total == slots && first == want_first, "streams plan: the scan");
  for (uint32_t s = 0; s < k; ++s)
    if (status[s] != cases[s].status || out_len[s] != cases[s].total) {
      std::printf("FAIL streams plan: stream %u status %d (want %d), length %llu (want %llu)\n", s, status[s],
                  cases[s].status, (unsigned long long)out_len[s], (unsigned long long)cases[s].total);
      ++failures;
    }
  // a byte short: that stream alone changes, and it gives its slots up
  for (uint32_t v = 0; v < k; ++v) {
    if (cases[v].status != SM_OK || cases[v].total == 0) continue;
    --cap[v];
    expect(run((uint32_t)slots, total) == SM_OK && total == slots - cases[v].nchunks, "a byte short: the total");
    for (uint32_t s = 0; s < k; ++s)
      expect(status[s] == (s == v ? (int32_t)SM_BUFFER_TOO_SMALL : cases[s].status) && out_len[s] == cases[s].total,
             "a byte short: the statuses");
    expect(first[v + 1] == first[v], "a byte short: no slots");
    ++cap[v];
  }
  // one slot short: nothing is planned
  expect(run((uint32_t)slots - 1, total) == SM_BUFFER_TOO_SMALL && total == slots, "one slot short");
  for (uint32_t s = 0; s < k; ++s) expect(status[s] == SM_ERR_ARGUMENT && out_len[s] == 0, "one slot short: the statuses");
  // no room limit, no outputs, no streams, bad arguments
  expect(smf_streams_plan(heap, off.data(), len.data(), k, nullptr, 0x7fffffffu, nullptr, nullptr, nullptr, &total) == SM_OK &&
             total == slots,
         "streams plan: null outputs");
  expect(smf_streams_plan(heap, off.data(), len.data(), k, nullptr, 0x7fffffffu, nullptr, nullptr, nullptr, nullptr) == SM_OK,
         "streams plan: null total");
  first[0] = 7;
  expect(smf_streams_plan(nullptr, nullptr, nullptr, 0, nullptr, 0, first.data(), nullptr, nullptr, &total) == SM_OK &&
             total == 0 && first[0] == 0,
         "streams plan: no streams");
  expect(smf_streams_plan(nullptr, off.data(), len.data(), k, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == SM_ERR_ARGUMENT &&
             smf_streams_plan(heap, nullptr, len.data(), k, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == SM_ERR_ARGUMENT &&
             smf_streams_plan(heap, off.data(), len.data(), 0x80000000u, nullptr, 0, nullptr, nullptr, nullptr, nullptr) ==
                 SM_ERR_ARGUMENT,
         "streams plan: arguments");
  std::free(heap);
  expect(smf_max_data_chunks(0) == 0 && smf_max_data_chunks(9) == 0 && smf_max_data_chunks(10) == 0 &&
             smf_max_data_chunks(17) == 0 && smf_max_data_chunks(18) == 1 && smf_max_data_chunks(10 + 8 * 1000) == 1000,
         "max data chunks");
  expect(smf_streams_scratch_bytes(3, 7) > smf_streams_scratch_bytes(3, 6) &&
             smf_streams_scratch_bytes(4, 7) >= smf_streams_scratch_bytes(3, 7) && smf_streams_scratch_bytes(0, 0) > 0,
         "streams scratch bytes");
}

// ---- the slot stage's verdict rules (smf_slots.h), the functions the kernels run -------------------
// Every combination against a table written out here, row by row: why the slot was not decoded
// wins, then the raw decoder's status for a 0x00 chunk, then the CRC; over the bound wins for a
// group, then its plan's status, then its first failing slot's.
void verdict_cases() {
  const int32_t OK = SM_OK, ARG = SM_ERR_ARGUMENT, SMALL = SM_BUFFER_TOO_SMALL, LARGE = SMF_ERR_CHUNK_TOO_LARGE,
                DEC = SM_ERR_VARINT, CRC = SMF_ERR_CRC;
  const struct {
    int32_t pre;
    uint32_t type;
    int32_t dec;
    bool crc_differs;
    int32_t want;
  } slot[] = {
      {OK, 0, OK, false, OK},       {OK, 0, OK, true, CRC},       {OK, 0, DEC, false, DEC},      {OK, 0, DEC, true, DEC},
      {OK, 1, OK, false, OK},       {OK, 1, OK, true, CRC},       {OK, 1, DEC, false, OK},       {OK, 1, DEC, true, CRC},
      {ARG, 0, OK, false, ARG},     {ARG, 0, OK, true, ARG},      {ARG, 0, DEC, false, ARG},     {ARG, 0, DEC, true, ARG},
      {ARG, 1, OK, false, ARG},     {ARG, 1, OK, true, ARG},      {ARG, 1, DEC, false, ARG},     {ARG, 1, DEC, true, ARG},
      {SMALL, 0, OK, false, SMALL}, {SMALL, 0, OK, true, SMALL},  {SMALL, 0, DEC, false, SMALL}, {SMALL, 0, DEC, true, SMALL},
      {SMALL, 1, OK, false, SMALL}, {SMALL, 1, OK, true, SMALL},  {SMALL, 1, DEC, false, SMALL}, {SMALL, 1, DEC, true, SMALL},
      {LARGE, 0, OK, false, LARGE}, {LARGE, 0, OK, true, LARGE},  {LARGE, 0, DEC, false, LARGE}, {LARGE, 0, DEC, true, LARGE},
      {LARGE, 1, OK, false, LARGE}, {LARGE, 1, OK, true, LARGE},  {LARGE, 1, DEC, false, LARGE}, {LARGE, 1, DEC, true, LARGE},
  };
  static_assert(sizeof(slot) / sizeof(slot[0]) == 4 * 2 * 2 * 2, "every combination");
  for (const auto& r : slot) {
    const uint32_t want_crc = 0x12345678u;
    const int32_t got = smf::slot_verdict(r.pre, r.type, r.dec, r.crc_differs ? ~want_crc : want_crc, want_crc);
    if (got != r.want) {
      std::printf("FAIL slot_verdict(pre %d, type %u, dec %d, crc %s): %d, want %d\n", r.pre, r.type, r.dec,
                  r.crc_differs ? "differs" : "equal", got, r.want);
      ++failures;
    }
  }
  const int32_t TRUNC = SMF_ERR_TRUNCATED;
  const struct {
    bool over;
    int32_t pre;
    bool failed;  // a slot failed, with SMF_ERR_CRC; else the slot status handed in is never looked at
    int32_t want;
  } group[] = {
      {false, OK, false, OK},     {false, OK, true, CRC},     {false, TRUNC, false, TRUNC}, {false, TRUNC, true, TRUNC},
      {true, OK, false, ARG},     {true, OK, true, ARG},      {true, TRUNC, false, ARG},    {true, TRUNC, true, ARG},
  };
  static_assert(sizeof(group) / sizeof(group[0]) == 2 * 2 * 2, "every combination");
  for (const auto& r : group) {
    const int32_t got = smf::group_verdict(r.over, r.pre, r.failed ? 3u : smf::kNoSlot, r.failed ? CRC : DEC);
    if (got != r.want) {
      std::printf("FAIL group_verdict(over %d, pre %d, %s): %d, want %d\n", r.over, r.pre, r.failed ? "a failing slot" : "none",
                  got, r.want);
      ++failures;
    }
  }
  expect(smf::group_verdict(false, OK, 0u, CRC) == CRC, "group_verdict: slot 0 fails");
}

// ---- the shared byte mover (../common/smc_device.h), every tid one after another ----------------
// The source is a heap block that ends exactly at src + n, so a read past the end trips the
// sanitizer; the function's own assert (host build) holds every 16-byte load to an aligned address
// not below src.  The destination lies between canary bytes.
void copy_bytes_cases() {
  std::vector<uint32_t> ns;
  for (uint32_t n = 0; n <= 48; ++n) ns.push_back(n);
  for (uint32_t n : {63u, 64u, 65u, 255u, 256u, 257u, 4095u, 4096u, 65535u, 65536u}) ns.push_back(n);
  const uint32_t kCanary = 32;
  for (uint32_t n : ns)
    for (uint32_t sa = 0; sa < 16; ++sa) {
      void* block = nullptr;
      if (posix_memalign(&block, 16, sa + n ? sa + n : 1) != 0) std::abort();
      uint8_t* const src = (uint8_t*)block + sa;
      for (uint32_t i = 0; i < n; ++i) src[i] = (uint8_t)(i * 131u + 7u * sa + n);
      std::vector<uint8_t> room(16 + kCanary + 16 + n + kCanary);
      uint8_t* const base = room.data() + ((16 - ((uintptr_t)room.data() & 15)) & 15);
      for (uint32_t da = 0; da < 16; ++da)
        for (uint32_t nthreads : {1u, 64u, 256u, 1024u}) {
          std::memset(room.data(), 0xa5, room.size());
          uint8_t* const dst = base + kCanary + da;
          for (uint32_t tid = 0; tid < nthreads; ++tid) smc::copy_bytes(src, n, dst, tid, nthreads);
          bool ok = std::memcmp(dst, src, n) == 0;
          for (const uint8_t* p = room.data(); p < room.data() + room.size(); ++p)
            if ((p < dst || p >= dst + n) && *p != 0xa5) ok = false;
          if (!ok) {
            std::printf("FAIL copy_bytes: n %u, source align %u, destination align %u, %u threads\n", n, sa, da, nthreads);
            ++failures;
          }
        }
      std::free(block);
    }
}

}  // namespace

int main() {
  // CRC known answers (the first five: RFC 3720)
  {
    S inc, dec;
    for (int i = 0; i < 32; ++i) {
      inc += (char)i;
      dec += (char)(31 - i);
    }
    struct {
      S in;
      uint32_t crc, masked;
    } kat[] = {{"123456789", 0xe3069283u, 0xc78ab0e5u}, {S(32, '\0'), 0x8a9136aau, 0x0fd7fffau},
               {S(32, '\xff'), 0x62a8ab43u, 0xf909b029u}, {inc, 0x46dd794eu, 0x951f7892u},
               {dec, 0x113fdb5cu, 0x593b0d57u},           {"", 0u, 0xa282ead8u},
               {"a", 0xc1d04330u, 0x28e46e78u},           {S(65536, '\0'), 0x72c0c4a4u, 0x2bcbd059u}};
    for (auto& k : kat) {
      const uint32_t c = smf_crc32c(k.in.data(), k.in.size());
      expect(c == k.crc && smf_crc32c_mask(c) == k.masked, "crc known answer");
    }
  }
  // the kernel's arithmetic against the bytewise CRC: every alignment, lengths around every edge
  {
    smf::CrcLut* T = new smf::CrcLut();
    smf::build_crc_lut(T);
    std::vector<uint8_t> buf(16 + 70000 + 16);
    uint32_t x = 12345;
    for (auto& b : buf) {
      x = x * 1664525u + 1013904223u;
      b = (uint8_t)(x >> 24);
    }
    const uint32_t lens[] = {0,   1,   2,    3,    4,    5,    7,    8,    15,    16,    17,    31,   32,
                             33,  63,  64,   65,   255,  256,  257,  1023, 1024,  1025,  4095,  4096, 4097,
                             4111, 4112, 8191, 8192, 8193, 65535, 65536, 65537, 69999, 70000};
    uint8_t* base = buf.data() + ((16 - ((uintptr_t)buf.data() & 15)) & 15);
    for (uint32_t a = 0; a < 16; ++a)
      for (uint32_t n : lens)
        if (crc_like_kernel(*T, base + a, n) != smf_crc32c(base + a, n)) {
          std::printf("FAIL kernel arithmetic: align %u length %u\n", a, n);
          ++failures;
        }
    delete T;
  }
  expect(smf_max_framed_length(0) == 10 && smf_max_framed_length(1) == 19 && smf_max_framed_length(65536) == 65554 &&
             smf_max_framed_length(65537) == 65537 + 26,
         "max framed length");

  const S a = raw_chunk("a");
  expect(kId + a == S("\xff\x06\x00\x00sNaPpY\x01\x05\x00\x00\x78\x6e\xe4\x28\x61", 19), "golden framed 'a'");
  // a compressed chunk: varint 5, literal tag (4 << 2), "hello"
  const S hello = chunk(0x00, crc_field("hello") + S("\x05\x10hello", 7));

  status_case("identifier only", kId, SM_OK);
  status_case("one raw chunk", kId + a, SM_OK, 1, 1);
  status_case("compressed chunk", kId + hello, SM_OK, 1, 5);
  status_case("padding", kId + chunk(0xfe, S(7, '\0')) + a, SM_OK, 1, 1);
  status_case("skippable 0x80", kId + chunk(0x80, "xyz") + a, SM_OK, 1, 1);
  status_case("skippable 0xfd", kId + a + chunk(0xfd, "xyz") + hello, SM_OK, 2, 6);
  status_case("repeated identifier", kId + a + kId + a, SM_OK, 2, 2);
  status_case("zero-length chunks", kId + chunk(0xfe, "") + chunk(0x80, "") + a, SM_OK, 1, 1);
  status_case("empty data chunks", kId + chunk(0x01, crc_field("")) + chunk(0x00, crc_field("") + S(1, '\0')), SM_OK, 2, 0);
  status_case("empty stream", "", SMF_ERR_NO_IDENTIFIER);
  status_case("missing identifier", a, SMF_ERR_NO_IDENTIFIER);
  status_case("padding first", chunk(0xfe, "") + kId, SMF_ERR_NO_IDENTIFIER);
  status_case("wrong identifier", chunk(0xff, "sNaPpy") + a, SMF_ERR_BAD_IDENTIFIER);
  status_case("identifier length 5", chunk(0xff, "sNaPp") + a, SMF_ERR_BAD_IDENTIFIER);
  status_case("wrong repeated identifier", kId + a + chunk(0xff, "SNaPpY"), SMF_ERR_BAD_IDENTIFIER, 1, 1);
  status_case("identifier cut", kId.substr(0, 7), SMF_ERR_TRUNCATED);
  status_case("reserved 0x02", kId + chunk(0x02, "abcd"), SMF_ERR_RESERVED_CHUNK);
  status_case("reserved 0x7f", kId + a + chunk(0x7f, ""), SMF_ERR_RESERVED_CHUNK, 1, 1);
  for (size_t cut = 1; cut <= 3; ++cut) {
    status_case("first header cut", kId.substr(0, cut), SMF_ERR_TRUNCATED);
    status_case("later header cut", kId + a + a.substr(0, cut), SMF_ERR_TRUNCATED, 1, 1);
  }
  status_case("payload cut short", kId + a + hello.substr(0, hello.size() - 1), SMF_ERR_TRUNCATED, 1, 1);
  status_case("padding cut short", kId + chunk(0xfe, "abc", 4), SMF_ERR_TRUNCATED);
  status_case("data chunk of 3 bytes", kId + chunk(0x01, "abc"), SMF_ERR_TRUNCATED);
  status_case("data chunk of 0 bytes", kId + chunk(0x00, ""), SMF_ERR_TRUNCATED);
  status_case("uncompressed chunk of 65541", kId + chunk(0x01, S(65541 + 4, 'x')), SMF_ERR_CHUNK_TOO_LARGE);
  status_case("uncompressed chunk of 65540", kId + chunk(0x01, S(65536 + 4, 'x')), SM_OK, 1, 65536);
  status_case("varint 65537", kId + chunk(0x00, S("abcd") + S("\x81\x80\x04", 3)), SMF_ERR_CHUNK_TOO_LARGE);
  status_case("varint 65536", kId + chunk(0x00, S("abcd") + S("\x80\x80\x04", 3)), SM_OK, 1, 65536);
  status_case("varint unterminated", kId + chunk(0x00, S("abcd") + S("\x80\x80", 2)), SM_ERR_VARINT);
  status_case("varint missing", kId + chunk(0x00, "abcd"), SM_ERR_VARINT);
  status_case("varint too long", kId + chunk(0x00, S("abcd") + S("\x80\x80\x80\x80\x10", 5)), SM_ERR_VARINT);

  // the entries, and a capacity that is too small
  {
    const S s = kId + a + chunk(0xfe, "pad") + hello + a;
    const Result r = walk(s);
    expect(r.sum.status == SM_OK && r.sum.nchunks == 3 && r.sum.total_length == 7, "entries: summary");
    expect(r.type[0] == 1 && r.off[0] == 18 && r.len[0] == 1 && r.ulen[0] == 1 && r.crc[0] == 0x28e46e78u, "entries: chunk 0");
    expect(r.type[1] == 0 && r.off[1] == 19 + 7 + 8 && r.len[1] == 7 && r.ulen[1] == 5, "entries: chunk 1");
    const Result small = walk(s, 2);
    expect(small.sum.status == SM_BUFFER_TOO_SMALL && small.sum.nchunks == 3 && small.type[1] == 0, "capacity too small");
    size_t total = 0;
    expect(smf_uncompressed_length((const uint8_t*)s.data(), s.size(), &total) == SM_OK && total == 7, "uncompressed length");
    smf_summary sum;
    expect(smf_index(nullptr, 4, nullptr, 0, &sum) == SM_ERR_ARGUMENT, "null buffer");
    expect(smf_index((const uint8_t*)s.data(), s.size(), nullptr, 0, nullptr) == SM_ERR_ARGUMENT, "null summary");
  }
  expect(smf::host_message(SMF_ERR_CRC) != nullptr && smf::host_message(SM_OK) == nullptr, "messages");
  range_cases();
  streams_cases();
  verdict_cases();
  copy_bytes_cases();

  if (failures) {
    std::printf("%d failure(s)\n", failures);
    return 1;
  }
  std::printf("smf_host_check ok\n");
  return 0;
}
