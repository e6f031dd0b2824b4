// smq_host_check.cpp -- stand-alone driver of the host-only Parquet page code (smq_host.cpp), built
// with -fsanitize=address,undefined by `make host_check`.  Every buffer is a heap block of exactly
// the chunk's size, so a walk that reads past a cut chunk trips the sanitizer; the batched decode's
// plan (smq_chunks_plan) runs over the same cases laid directly behind one another; the CRC
// kernel's arithmetic runs lane by lane (crc32_model) over heap blocks of exactly the range's size
// at every alignment; the page encoder's rewrite rule, its walk and its plan (smqe_*) run case by case
// over exact-size heap blocks too.  The expected values are written out here; none comes from the code
// under test.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "smq_chunks.h"
#include "smq_crc.h"
#include "smq_encode.h"
#include "smq_format.h"

namespace {

int failures = 0;

void expect(bool ok, const char* what) {
  if (!ok) {
    std::printf("FAIL %s\n", what);
    ++failures;
  }
}

typedef std::string S;

S zz(int64_t v) {  // a zigzag varint
  uint64_t u = ((uint64_t)v << 1) ^ (uint64_t)(v >> 63);
  S s;
  while (u >= 0x80) {
    s += (char)((u & 0x7f) | 0x80);
    u >>= 7;
  }
  s += (char)u;
  return s;
}

S fld(uint32_t delta, uint32_t type) { return S(1, (char)((delta << 4) | type)); }
S i32f(uint32_t delta, int64_t v) { return fld(delta, 5) + zz(v); }
const S kStopByte(1, '\0');

// PageHeader{1 type, 2 usize, 3 csize [, 4 crc]} up to where the page type's struct goes
S head(int32_t type, int32_t usize, int32_t csize, const int64_t* crc = nullptr) {
  return i32f(1, type) + i32f(1, usize) + i32f(1, csize) + (crc ? i32f(1, *crc) : S());
}
// field 5 (behind field `last`): data_page_header{1 num_values, 2 encoding, 3, 4}
S data_header(uint32_t last, int32_t nv, int32_t enc) {
  return fld(5 - last, 12) + i32f(1, nv) + i32f(1, enc) + i32f(1, 3) + i32f(1, 3) + kStopByte;
}
S dict_header(uint32_t last, int32_t nv, int32_t enc) { return fld(7 - last, 12) + i32f(1, nv) + i32f(1, enc) + kStopByte; }
S v2_header(uint32_t last, int32_t nv, int32_t enc, int32_t def, int32_t rep, int compressed /* -1: absent */) {
  return fld(8 - last, 12) + i32f(1, nv) + i32f(1, 0) + i32f(1, nv) + i32f(1, enc) + i32f(1, def) + i32f(1, rep) +
         (compressed < 0 ? S() : fld(1, compressed ? 1 : 2)) + kStopByte;
}

const S kAbc = S("\x03\x08" "abc", 5);  // compress("abc")

S v1_page(const S& body, int32_t usize, int32_t nv = 3) { return head(0, usize, (int32_t)body.size()) + data_header(3, nv, 0) + kStopByte + body; }

struct Result {
  smq_summary sum;
  std::vector<uint64_t> hdr_off, out_off;
  std::vector<uint32_t> hdr_len, body_len, usize, levels, flags, crc;
  std::vector<int32_t> num_values, type, encoding;
};

Result walk(const S& chunk, uint32_t max_pages = 16) {
  Result r;
  r.hdr_off.resize(max_pages);
  r.out_off.resize(max_pages);
  for (auto* v : {&r.hdr_len, &r.body_len, &r.usize, &r.levels, &r.flags, &r.crc}) v->resize(max_pages);
  for (auto* v : {&r.num_values, &r.type, &r.encoding}) v->resize(max_pages);
  uint8_t* heap = (uint8_t*)std::malloc(chunk.size() ? chunk.size() : 1);
  std::memcpy(heap, chunk.data(), chunk.size());
  const smq_pages pg{r.hdr_off.data(), r.hdr_len.data(), r.body_len.data(), r.usize.data(),    r.levels.data(), r.out_off.data(),
                     r.num_values.data(), r.type.data(), r.encoding.data(), r.flags.data(), r.crc.data()};
  r.sum = smq_summary{0, 0, 0};
  r.sum.status = smq_index(heap, chunk.size(), &pg, max_pages, &r.sum);
  smq_summary count{0, 0, 0};
  smq_index(heap, chunk.size(), nullptr, 0, &count);
  expect(count.npages == r.sum.npages && count.total_length == r.sum.total_length, "count-only walk agrees");
  std::free(heap);
  return r;
}

struct Case {
  S chunk;
  int32_t status;
  uint32_t npages;
  uint64_t total;
};
std::vector<Case> cases;  // every status_case, for chunks_cases

void status_case(const char* name, const S& chunk, int32_t status, uint32_t npages = 0, uint64_t total = 0) {
  cases.push_back(Case{chunk, status, npages, total});
  const Result r = walk(chunk);
  if (r.sum.status != status || r.sum.npages != npages || r.sum.total_length != total) {
    std::printf("FAIL %s: status %d (want %d), pages %u (want %u), total %llu (want %llu)\n", name, r.sum.status, status,
                r.sum.npages, npages, (unsigned long long)r.sum.total_length, (unsigned long long)total);
    ++failures;
  }
}

// Every case as one batch, the chunks directly behind one another in a heap block of exactly their
// size: a walk that leaves its chunk reads its neighbour (a wrong status) or, at the last chunk,
// trips the sanitizer.
void chunks_cases() {
  const std::vector<Case>& cs = cases;
  const uint32_t k = (uint32_t)cs.size();
  std::vector<uint64_t> off(k), len(k), cap(k), out_len(k);
  std::vector<uint32_t> first(k + 1), want_first(k + 1);
  std::vector<int32_t> status(k);
  uint64_t n = 0, slots = 0;
  for (uint32_t s = 0; s < k; ++s) {
    off[s] = n;
    len[s] = cs[s].chunk.size();
    n += len[s];
    cap[s] = cs[s].total;
    want_first[s] = (uint32_t)slots;
    slots += cs[s].status == SM_OK ? cs[s].npages : 0;
  }
  want_first[k] = (uint32_t)slots;
  uint8_t* heap = (uint8_t*)std::malloc(n);
  for (uint32_t s = 0; s < k; ++s) std::memcpy(heap + off[s], cs[s].chunk.data(), len[s]);
  uint64_t total = 0, frags = 0;
  auto run = [&](uint32_t max_pages) {
    return smq_chunks_plan(heap, off.data(), len.data(), k, cap.data(), max_pages, first.data(), out_len.data(), status.data(),
                           &total, &frags);
  };
  expect(run((uint32_t)slots) == SM_OK && total == slots && first == want_first, "chunks plan: the scan");
  for (uint32_t s = 0; s < k; ++s)
    if (status[s] != cs[s].status || out_len[s] != cs[s].total) {
      std::printf("FAIL chunks plan: chunk %u status %d (want %d), length %llu (want %llu)\n", s, status[s], cs[s].status,
                  (unsigned long long)out_len[s], (unsigned long long)cs[s].total);
      ++failures;
    }
  // a byte short: that chunk alone changes, and it gives its slots up
  for (uint32_t v = 0; v < k; ++v) {
    if (cs[v].status != SM_OK || cs[v].total == 0) continue;
    --cap[v];
    expect(run((uint32_t)slots) == SM_OK && total == slots - cs[v].npages, "a byte short: the total");
    for (uint32_t s = 0; s < k; ++s)
      expect(status[s] == (s == v ? (int32_t)SM_BUFFER_TOO_SMALL : cs[s].status) && out_len[s] == cs[s].total,
             "a byte short: the statuses");
    expect(first[v + 1] == first[v], "a byte short: no slots");
    ++cap[v];
  }
  // one slot short: nothing is planned
  expect(run((uint32_t)slots - 1) == SM_BUFFER_TOO_SMALL && total == slots, "one slot short");
  for (uint32_t s = 0; s < k; ++s) expect(status[s] == SM_ERR_ARGUMENT && out_len[s] == 0, "one slot short: the statuses");
  expect(smq_chunks_plan(heap, off.data(), len.data(), k, nullptr, 0x7fffffffu, nullptr, nullptr, nullptr, &total, nullptr) ==
                 SM_OK && total == slots,
         "chunks plan: null outputs");
  first[0] = 7;
  expect(smq_chunks_plan(nullptr, nullptr, nullptr, 0, nullptr, 0, first.data(), nullptr, nullptr, &total, &frags) == SM_OK &&
             total == 0 && frags == 0 && first[0] == 0,
         "chunks plan: no chunks");
  expect(smq_chunks_plan(nullptr, off.data(), len.data(), k, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr) ==
                 SM_ERR_ARGUMENT &&
             smq_chunks_plan(heap, nullptr, len.data(), k, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr) ==
                 SM_ERR_ARGUMENT &&
             smq_chunks_plan(heap, off.data(), len.data(), 0x80000000u, nullptr, 0, nullptr, nullptr, nullptr, nullptr,
                             nullptr) == SM_ERR_ARGUMENT,
         "chunks plan: arguments");
  std::free(heap);
}

uint32_t crc32_bytewise(const uint8_t* p, size_t n) {  // the textbook bit loop
  uint32_t c = 0xffffffffu;
  for (size_t i = 0; i < n; ++i) {
    c ^= p[i];
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1) ? 0xEDB88320u : 0u);
  }
  return ~c;
}

void crc_cases() {
  smq::CrcLut* T = (smq::CrcLut*)std::malloc(sizeof(smq::CrcLut));
  smq::build_crc_lut(T);
  expect(smq::crc32_model(T, (const uint8_t*)"123456789", 9) == 0xCBF43926u, "crc32 check value");
  expect(smq::crc32_model(T, nullptr, 0) == 0, "crc32 of nothing");
  const uint32_t seg = smq::kCrcSegment;
  const uint32_t lens[] = {1, 15, 16, 17, 4095, 4096 + 16, seg - 1, seg, seg + 1, 2 * seg + 3, 5 * seg};
  for (uint32_t n : lens)
    for (uint32_t a = 0; a < 16; a += (n > 2 * seg ? 5 : 1)) {
      uint8_t* heap = (uint8_t*)std::malloc(n + a);  // (malloc's blocks are 16-byte aligned: the range ends the block)
      uint32_t x = n * 2654435761u + a;
      for (uint32_t i = 0; i < n; ++i) {
        x = x * 1664525u + 1013904223u;
        heap[a + i] = (uint8_t)(x >> 24);
      }
      if (smq::crc32_model(T, heap + a, n) != crc32_bytewise(heap + a, n)) {
        std::printf("FAIL crc32 of %u bytes at alignment %u\n", n, a);
        ++failures;
      }
      std::free(heap);
    }
  expect(smq::crc_segments(0) == 0 && smq::crc_segments(1) == 1 && smq::crc_segments(seg) == 1 && smq::crc_segments(seg + 1) == 2 &&
             smq::crc_segments(0x7fffffffu) == 32768,
         "crc segments");
  expect(smq::crc_first_segment(0) == 0 && smq::crc_first_segment(5) == 5 && smq::crc_first_segment(seg) == seg &&
             smq::crc_first_segment(seg + 7) == 7 && smq::crc_segment_start(seg + 7, 1) == 7 &&
             smq::crc_segment_start(3 * seg, 2) == 2 * seg && smq::crc_segment_len(seg + 7, 0) == 7 &&
             smq::crc_segment_len(seg + 7, 1) == seg,
         "crc segment places");
  std::free(T);
}

// ---- the page encoder (include/snappy_mi355x_parquet_write.h) ------------------------------------------
// smqe_rewrite_header over a heap block of exactly the header's size, into one of exactly `cap` bytes
struct Rewritten {
  sm_status status;
  size_t len;
  S bytes;
};
Rewritten rewrite(const S& hdr, uint64_t body, uint32_t crc, size_t cap) {
  uint8_t* in = (uint8_t*)std::malloc(hdr.size() ? hdr.size() : 1);
  std::memcpy(in, hdr.data(), hdr.size());
  uint8_t* out = (uint8_t*)std::malloc(cap ? cap : 1);
  std::memset(out, 0xee, cap ? cap : 1);
  Rewritten r{SM_OK, 0, S()};
  r.status = smqe_rewrite_header(in, hdr.size(), body, crc, cap ? out : nullptr, cap, &r.len);
  r.bytes = S((const char*)out, cap);
  std::free(in);
  std::free(out);
  return r;
}

void rewrite_case(const char* name, const S& hdr, uint64_t body, uint32_t crc, const S& want) {
  const Rewritten exact = rewrite(hdr, body, crc, want.size());
  const Rewritten roomy = rewrite(hdr + "behind", body, crc, want.size() + 3);
  const Rewritten tight = rewrite(hdr, body, crc, want.size() - 1);
  const Rewritten measure = rewrite(hdr, body, crc, 0);
  if (exact.status != SM_OK || exact.len != want.size() || exact.bytes != want || roomy.status != SM_OK ||
      roomy.bytes != want + S(3, '\xee') || tight.status != SM_BUFFER_TOO_SMALL || tight.len != want.size() ||
      tight.bytes != S(want.size() - 1, '\xee') || measure.status != SM_BUFFER_TOO_SMALL || measure.len != want.size()) {
    std::printf("FAIL rewrite: %s (status %d, length %zu, want %zu)\n", name, exact.status, exact.len, want.size());
    ++failures;
  }
}

struct EncodeResult {
  smq_summary sum;
  std::vector<uint32_t> sites, hdr_len, body_len, flags;
};
EncodeResult encode_walk(const S& chunk, uint32_t max_pages = 8) {
  EncodeResult r;
  std::vector<uint64_t> hdr_off(max_pages), out_off(max_pages);
  std::vector<uint32_t> usize(max_pages), levels(max_pages), crc(max_pages);
  std::vector<int32_t> nv(max_pages), type(max_pages), enc(max_pages);
  r.sites.assign((size_t)max_pages * SMQE_SITES, 0xeeeeeeeeu);
  r.hdr_len.resize(max_pages);
  r.body_len.resize(max_pages);
  r.flags.resize(max_pages);
  uint8_t* heap = (uint8_t*)std::malloc(chunk.size() ? chunk.size() : 1);
  std::memcpy(heap, chunk.data(), chunk.size());
  const smq_pages pg{hdr_off.data(), r.hdr_len.data(), r.body_len.data(), usize.data(), levels.data(), out_off.data(),
                     nv.data(),      type.data(),      enc.data(),        r.flags.data(), crc.data()};
  r.sum = smq_summary{0, 0, 0};
  smqe_index(heap, chunk.size(), &pg, r.sites.data(), max_pages, &r.sum);
  smq_summary count{0, 0, 0};
  smqe_index(heap, chunk.size(), nullptr, nullptr, 0, &count);
  expect(count.npages == r.sum.npages && count.total_length == r.sum.total_length, "encode walk: the count-only walk agrees");
  std::free(heap);
  return r;
}

void encode_status(const char* name, const S& chunk, int32_t status, uint32_t npages) {
  const EncodeResult r = encode_walk(chunk);
  if (r.sum.status != status || r.sum.npages != npages) {
    std::printf("FAIL encode walk: %s: status %d (want %d), pages %u (want %u)\n", name, r.sum.status, status, r.sum.npages, npages);
    ++failures;
  }
}

void encode_cases() {
  const int64_t crc = -2, imin = INT32_MIN;
  // both varints grow; the rest of the header stays
  const S v1 = head(0, 3, 3, &crc) + data_header(4, 3, 0) + kStopByte;
  rewrite_case("both varints grow", v1, 64, 0x80000000u, head(0, 3, 64, &imin) + data_header(4, 3, 0) + kStopByte);
  const int64_t big_crc = 0x12345678;
  const S wide = head(0, 0x7fffffff, 0x7fffffff, &big_crc) + data_header(4, 3, 0) + kStopByte;
  const int64_t zero = 0;
  rewrite_case("both varints shrink", wide, 0, 0, head(0, 0x7fffffff, 0, &zero) + data_header(4, 3, 0) + kStopByte);
  rewrite_case("the longest body", v1, 0x7fffffffu, 0xfffffffeu, head(0, 3, 0x7fffffff, &crc) + data_header(4, 3, 0) + kStopByte);
  // no crc: none is added, and the crc argument is not looked at
  rewrite_case("no crc", head(0, 3, 3) + data_header(3, 3, 0) + kStopByte, 8192, 0xdeadbeefu,
               head(0, 3, 8192) + data_header(3, 3, 0) + kStopByte);
  // v2: is_compressed false becomes true, true stays, absent stays absent
  const S v2_false = head(3, 6, 6) + v2_header(3, 9, 8, 2, 1, 0) + kStopByte;
  rewrite_case("v2 false", v2_false, 5, 0, head(3, 6, 5) + v2_header(3, 9, 8, 2, 1, 1) + kStopByte);
  rewrite_case("v2 true", head(3, 6, 6) + v2_header(3, 9, 8, 2, 1, 1) + kStopByte, 5, 0,
               head(3, 6, 5) + v2_header(3, 9, 8, 2, 1, 1) + kStopByte);
  rewrite_case("v2 absent", head(3, 6, 6) + v2_header(3, 9, 8, 2, 1, -1) + kStopByte, 5, 0,
               head(3, 6, 5) + v2_header(3, 9, 8, 2, 1, -1) + kStopByte);
  // the crc before the size, both in the long form, an unknown field between them
  const S lf3 = S("\x05", 1) + zz(3), lf4 = S("\x05", 1) + zz(4), unknown = S("\x08", 1) + zz(90) + S("\x03" "abc", 4);
  rewrite_case("crc before the size", i32f(1, 0) + i32f(1, 3) + lf4 + zz(-2) + unknown + lf3 + zz(3) + data_header(3, 3, 0) + kStopByte,
               8192, 1, i32f(1, 0) + i32f(1, 3) + lf4 + zz(1) + unknown + lf3 + zz(8192) + data_header(3, 3, 0) + kStopByte);
  // a page type the walk steps over: the rule is the same
  rewrite_case("an index page", head(1, 99, 4, &crc) + kStopByte, 4, 0xfffffffeu, head(1, 99, 4, &crc) + kStopByte);
  // rejections
  expect(rewrite(v1, 0x80000000ull, 0, 64).status == SM_ERR_INPUT_TOO_LARGE, "rewrite: a body above 2 GiB - 1");
  for (size_t cut = 0; cut < v1.size(); ++cut)
    expect(rewrite(v1.substr(0, cut), 5, 5, 64).status == SMQ_ERR_TRUNCATED, "rewrite: a cut header");
  const S twice3 = i32f(1, 1) + i32f(1, 0) + i32f(1, 0) + lf3 + zz(0) + kStopByte;
  const S twice4 = head(1, 0, 0, &crc) + lf4 + zz(0) + kStopByte;
  const S twice7 = head(3, 6, 6) + v2_header(3, 9, 8, 2, 1, 0).substr(0, 14) + S("\x01", 1) + zz(7) + kStopByte + kStopByte;
  expect(rewrite(twice3, 5, 5, 64).status == SMQ_ERR_HEADER, "rewrite: field 3 twice");
  expect(rewrite(twice4, 5, 5, 64).status == SMQ_ERR_HEADER, "rewrite: field 4 twice");
  expect(rewrite(twice7, 5, 5, 64).status == SMQ_ERR_HEADER, "rewrite: field 8.7 twice");
  expect(rewrite(i32f(1, 1) + i32f(1, 0) + kStopByte, 5, 5, 64).status == SMQ_ERR_HEADER, "rewrite: field 3 missing");
  size_t len = 0;
  expect(smqe_rewrite_header((const uint8_t*)v1.data(), v1.size(), 5, 5, nullptr, 0, nullptr) == SM_ERR_ARGUMENT &&
             smqe_rewrite_header(nullptr, 4, 5, 5, nullptr, 0, &len) == SM_ERR_ARGUMENT &&
             smqe_rewrite_header((const uint8_t*)v1.data(), v1.size(), 5, 5, nullptr, 4, &len) == SM_ERR_ARGUMENT,
         "rewrite: arguments");

  // the encode walk: plain pages, their sites
  const S abc = head(0, 3, 3) + data_header(3, 3, 0) + kStopByte + "abc";
  const S v2 = head(3, 6, 6, &crc) + v2_header(4, 9, 8, 2, 1, 0) + kStopByte + "LLLabc";
  const S index_page = head(1, 99, 4) + kStopByte + "skip";
  {
    const EncodeResult r = encode_walk(abc + index_page + v2);
    expect(r.sum.status == SM_OK && r.sum.npages == 3 && r.sum.total_length == 9, "encode walk: summary");
    const uint32_t want[3][SMQE_SITES] = {{5, 1, 0, 0, 0}, {6, 1, 0, 0, 0}, {5, 1, 7, 1, 21}};
    for (uint32_t k = 0; k < 3; ++k)
      for (uint32_t i = 0; i < SMQE_SITES; ++i) expect(r.sites[k * SMQE_SITES + i] == want[k][i], "encode walk: sites");
    expect(r.sites[3 * SMQE_SITES] == 0xeeeeeeeeu, "encode walk: no site behind the last page");
    expect(r.body_len[0] == 3 && r.body_len[1] == 4 && r.body_len[2] == 6 && r.flags[0] == 0 && r.flags[1] == 0 &&
               r.flags[2] == SMQ_PAGE_HAS_CRC && r.hdr_len[2] == v2.size() - 6,
           "encode walk: entries");
    const EncodeResult small = encode_walk(abc + index_page + v2, 2);
    expect(small.sum.status == SM_BUFFER_TOO_SMALL && small.sum.npages == 3, "encode walk: capacity too small");
  }
  encode_status("empty chunk", "", SM_OK, 0);
  encode_status("a section that is Snappy already", abc + head(0, 3, 5) + data_header(3, 3, 0) + kStopByte + kAbc, SMQ_ERR_SIZE_MISMATCH, 1);
  encode_status("a v2 page whose sizes differ", head(3, 6, 8) + v2_header(3, 9, 8, 2, 1, 0) + kStopByte + "LLL" + kAbc, SMQ_ERR_SIZE_MISMATCH, 0);
  encode_status("an index page whose sizes differ", index_page, SM_OK, 1);
  encode_status("field 3 twice", abc + twice3, SMQ_ERR_HEADER, 1);
  encode_status("field 4 twice", abc + twice4, SMQ_ERR_HEADER, 1);
  encode_status("field 8.7 twice", abc + twice7 + "LLLabc", SMQ_ERR_HEADER, 1);
  encode_status("field 3 missing", i32f(1, 1) + i32f(1, 0) + kStopByte, SMQ_ERR_HEADER, 0);
  encode_status("levels above the size", head(3, 2, 2) + v2_header(3, 9, 8, 2, 1, -1) + kStopByte + "LL", SMQ_ERR_HEADER, 0);
  encode_status("nothing of a section is looked at", head(0, 3, 3) + data_header(3, 3, 0) + kStopByte + S("\x80\x80\x80", 3), SM_OK, 1);
  for (size_t cut = 1; cut < v2.size(); ++cut) encode_status("v2 cut", v2.substr(0, cut), SMQ_ERR_TRUNCATED, 0);
  for (size_t cut = 1; cut < v2.size(); ++cut) encode_status("second page cut", abc + v2.substr(0, cut), SMQ_ERR_TRUNCATED, 1);

  // the plan: chunks directly behind one another in a heap block of exactly their size
  {
    const S big = head(0, 200000, 200000) + data_header(3, 1, 0) + kStopByte + S(200000, 'x');
    const S bad = head(0, 3, 5) + data_header(3, 3, 0) + kStopByte + kAbc;
    const S parts[5] = {abc, v2 + index_page, bad, big, ""};
    uint64_t off[5], len[5], n = 0;
    for (int i = 0; i < 5; ++i) {
      off[i] = n;
      len[i] = parts[i].size();
      n += len[i];
    }
    uint8_t* heap = (uint8_t*)std::malloc(n);
    for (int i = 0; i < 5; ++i) std::memcpy(heap + off[i], parts[i].data(), len[i]);
    uint32_t first[6];
    int32_t st[5];
    uint64_t bound[5], pages = 0, stage = 0, frags = 0;
    expect(smqe_chunks_plan(heap, off, len, 5, 4, first, st, bound, &pages, &stage, &frags) == SM_OK, "encode plan: status");
    expect(pages == 4 && frags == 4 && stage == 32 + 48 + 48 + 233376, "encode plan: the three bounds");
    expect(first[0] == 0 && first[1] == 1 && first[2] == 3 && first[3] == 3 && first[4] == 4 && first[5] == 4, "encode plan: the scan");
    expect(st[0] == SM_OK && st[1] == SM_OK && st[2] == SMQ_ERR_SIZE_MISMATCH && st[3] == SM_OK && st[4] == SM_OK, "encode plan: statuses");
    expect(bound[0] == abc.size() - 3 + 8 + 35 && bound[1] == (v2.size() - 6) + 8 + 3 + 35 + index_page.size() && bound[2] == 0 &&
               bound[3] == (big.size() - 200000) + 8 + 32 + 200000 + 33333 && bound[4] == 0,
           "encode plan: the output bounds");
    expect(smqe_chunks_plan(heap, off, len, 5, 3, first, st, bound, &pages, &stage, &frags) == SM_BUFFER_TOO_SMALL && pages == 4,
           "encode plan: one slot short");
    for (int i = 0; i < 5; ++i) expect(st[i] == SM_ERR_ARGUMENT && bound[i] == 0, "encode plan: one slot short: the statuses");
    expect(smqe_chunks_plan(heap, off, len, 5, 4, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == SM_OK &&
               smqe_chunks_plan(nullptr, off, len, 5, 4, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == SM_ERR_ARGUMENT &&
               smqe_chunks_plan(nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, &pages, &stage, &frags) == SM_OK &&
               pages == 0 && stage == 32 && frags == 0,
           "encode plan: arguments");
    std::free(heap);
  }
  expect(smqe_max_chunk_length(600, 2) == 600 + 100 + 80 && smqe_stage_bound(600, 2) == 32 + 600 + 100 + 96, "encoder bounds");
  expect(smqe_scratch_bytes(3, 7, 1000) > smqe_scratch_bytes(3, 6, 1000) && smqe_scratch_bytes(3, 7, 5000) >= smqe_scratch_bytes(3, 7, 1000) + 3984 &&
             smqe_scratch_bytes(0, 0, 0) > 0,
         "encoder scratch bytes");
  // the verdicts
  expect(smq::page_verdict(false, 0, 0, 5) == SM_OK && smq::page_verdict(true, 3, 10, SM_OK) == SM_OK &&
             smq::page_verdict(true, 3, 0, SM_OK) == SM_ERR_DEVICE && smq::page_verdict(true, 3, 10, SM_ERR_DEVICE) == SM_ERR_DEVICE &&
             smq::page_verdict(true, 0x7ffffff0u, 16, SM_OK) == SM_ERR_INPUT_TOO_LARGE && smq::page_verdict(true, 0x7ffffff0u, 15, SM_OK) == SM_OK,
         "page verdict");
  {
    const smq::EncodeVerdict over = smq::encode_verdict(true, SM_OK, false, 0, 10, 10), pre = smq::encode_verdict(false, SMQ_ERR_HEADER, true, 32, 10, 10),
                             fail = smq::encode_verdict(false, SM_OK, true, 32, 10, 10), tight = smq::encode_verdict(false, SM_OK, false, 0, 11, 10),
                             fits = smq::encode_verdict(false, SM_OK, false, 0, 10, 10);
    expect(over.status == SM_ERR_ARGUMENT && over.length == 0 && pre.status == SMQ_ERR_HEADER && pre.length == 0 && fail.status == 32 &&
               fail.length == 0 && tight.status == SM_BUFFER_TOO_SMALL && tight.length == 11 && fits.status == SM_OK && fits.length == 10,
           "encode verdict");
  }
}

}  // namespace

int main() {
  // golden: a PageHeader parquet-cpp wrote (tests/golden/parquet/v1.parquet, the counter column's
  // first page): a v1 data page of 1,024 PLAIN values, 8,192 bytes compressed to 4,106, crc
  // 0x41ee9ac7, with a Statistics struct (binaries, an i64, two bools) that is stepped over.  The body
  // here is the section's varint and zeros: structure only.
  {
    const S h("\x15\x00\x15\x80\x80\x01\x15\x94\x40\x15\x8e\xeb\xf4\x9e\x08\x1c\x15\x80\x10\x15\x00\x15\x06\x15\x06\x1c\x18\x08"
              "\xff\x03\x00\x00\x00\x00\x00\x00\x18\x08\x00\x00\x00\x00\x00\x00\x00\x00\x16\x00\x28\x08\xff\x03\x00\x00\x00\x00"
              "\x00\x00\x18\x08\x00\x00\x00\x00\x00\x00\x00\x00\x11\x11\x00\x00\x00", 73);
    const Result r = walk(h + S("\x80\x40", 2) + S(4104, '\0'));
    expect(r.sum.status == SM_OK && r.sum.npages == 1 && r.sum.total_length == 8192 && r.hdr_len[0] == 73 && r.body_len[0] == 4106 &&
               r.usize[0] == 8192 && r.num_values[0] == 1024 && r.type[0] == 0 && r.encoding[0] == 0 && r.crc[0] == 0x41ee9ac7u &&
               r.flags[0] == (SMQ_PAGE_HAS_CRC | SMQ_PAGE_COMPRESSED),
           "golden: a data page header parquet-cpp wrote");
    expect(head(0, 8192, 4106) == h.substr(0, 9), "golden: the builders write parquet-cpp's bytes");
  }

  const S abc = v1_page(kAbc, 3);
  const int64_t crc = -2;  // (0xfffffffe)
  const S dict = head(2, 3, 5, &crc) + dict_header(4, 7, 2) + kStopByte + kAbc;
  const S v2c = head(3, 6, 8) + v2_header(3, 9, 8, 2, 1, -1) + kStopByte + "LLL" + kAbc;       // levels 3, compressed
  const S v2s = head(3, 6, 6) + v2_header(3, 9, 8, 2, 1, 0) + kStopByte + "LLLabc";            // stored
  const S v2e = head(3, 3, 3) + v2_header(3, 9, 8, 2, 1, 1) + kStopByte + "LLL";               // no values
  const S index_page = head(1, 99, 4) + kStopByte + "skip";
  const S other_page = head(77, 0, 0) + kStopByte;
  status_case("empty chunk", "", SM_OK);
  status_case("abc, v1", abc, SM_OK, 1, 3);
  status_case("dictionary page", dict, SM_OK, 1, 3);
  status_case("v2 compressed", v2c, SM_OK, 1, 6);
  status_case("v2 stored", v2s, SM_OK, 1, 6);
  status_case("v2 without values", v2e, SM_OK, 1, 3);
  status_case("index page", index_page, SM_OK, 1, 0);
  status_case("index page between", abc + index_page + other_page + dict, SM_OK, 4, 6);
  for (size_t cut = 1; cut < abc.size(); ++cut)
    status_case("abc cut", abc.substr(0, cut), SMQ_ERR_TRUNCATED);
  status_case("second page cut", dict + abc.substr(0, abc.size() - 1), SMQ_ERR_TRUNCATED, 1, 3);
  status_case("field 3 missing", i32f(1, 1) + i32f(1, 0) + kStopByte, SMQ_ERR_HEADER);
  status_case("field 1 missing", i32f(2, 0) + i32f(1, 0) + kStopByte, SMQ_ERR_HEADER);
  status_case("field 2 an i64", i32f(1, 1) + fld(1, 6) + zz(0) + i32f(1, 0) + kStopByte, SMQ_ERR_HEADER);
  status_case("negative size", head(1, -1, 0) + kStopByte, SMQ_ERR_HEADER);
  status_case("negative compressed size", head(1, 0, -1) + kStopByte, SMQ_ERR_HEADER);
  status_case("data page without its header", head(0, 3, 5) + kStopByte + kAbc, SMQ_ERR_HEADER);
  status_case("v2 page with a v1 header", head(3, 3, 5) + data_header(3, 1, 0) + kStopByte + kAbc, SMQ_ERR_HEADER);
  status_case("levels above the size", head(3, 2, 8) + v2_header(3, 9, 8, 2, 1, -1) + kStopByte + "LLL" + kAbc, SMQ_ERR_HEADER);
  status_case("negative levels", head(3, 6, 8) + v2_header(3, 9, 8, -2, 1, -1) + kStopByte + "LLL" + kAbc, SMQ_ERR_HEADER);
  status_case("unknown type nibble", fld(1, 13) + kStopByte, SMQ_ERR_HEADER);
  status_case("type nibble 0 with a delta", S("\x10", 1) + kStopByte, SMQ_ERR_HEADER);
  status_case("i32 varint of 6 bytes", fld(1, 5) + S("\x80\x80\x80\x80\x80\x01", 6) + kStopByte, SMQ_ERR_HEADER);
  status_case("i32 above 32 bits", fld(1, 5) + S("\xfe\xff\xff\xff\x3f", 5) + kStopByte, SMQ_ERR_HEADER);
  status_case("i32 varint cut", fld(1, 5) + S("\x80\x80", 2), SMQ_ERR_TRUNCATED);
  status_case("varint differs from want", v1_page(kAbc, 4), SMQ_ERR_SIZE_MISMATCH);
  status_case("varint does not parse", v1_page(S("\x80\x80", 2), 4), SM_ERR_VARINT);
  status_case("varint of 5 bytes overflows", v1_page(S("\x80\x80\x80\x80\x10", 5), 4), SM_ERR_VARINT);
  status_case("empty section, bytes wanted", v1_page("", 1), SMQ_ERR_SIZE_MISMATCH);
  status_case("empty section, none wanted", v1_page("", 0), SM_OK, 1, 0);
  status_case("stored section too long", head(3, 5, 6) + v2_header(3, 9, 8, 2, 1, 0) + kStopByte + "LLLabc", SMQ_ERR_SIZE_MISMATCH);
  status_case("mismatch behind a page", abc + v1_page(kAbc, 4), SMQ_ERR_SIZE_MISMATCH, 1, 3);
  // unknown fields: skipped by type at any place, a long-form id, a binary that only moves the position
  {
    const S unknown = fld(1, 1) + fld(1, 2) + fld(1, 3) + "b" + fld(1, 4) + zz(-300) + fld(1, 6) + zz(-(1ll << 62)) +
                      fld(1, 7) + S(8, 'd') + fld(1, 8) + S("\x05" "bytes", 6) +
                      fld(1, 9) + S("\x35\x02\x04\x06", 4) +                                   // list<i32> of 3
                      fld(1, 9) + S("\xf1\x10", 2) + S(16, '\x01') +                           // list<bool> of 16, long size
                      fld(1, 11) + S("\x02\x85", 2) + S("\x01k\x02\x01q\x04", 6) +              // map<binary,i32> of 2
                      fld(1, 11) + S("\x00", 1) +                                              // the empty map
                      fld(1, 12) + fld(1, 9) + S("\x2c", 1) + i32f(1, 5) + kStopByte + kStopByte + kStopByte +  // struct{list<struct>}
                      S("\x05", 1) + zz(300) + zz(7);                                          // id 300 in the long form
    // (the fields above have ids 9.. behind field 8's place: put them behind the data page header)
    const S page = head(0, 3, 5) + data_header(3, 3, 0) + fld(4, 5) + zz(1) + unknown + kStopByte + kAbc;
    status_case("unknown fields of every type", page, SM_OK, 1, 3);
    const S big = head(0, 3, 5) + data_header(3, 3, 0) + fld(4, 8) + S("\xac\x02", 2) + S(300, 's') + kStopByte + kAbc;
    status_case("a binary of 300 bytes", big, SM_OK, 1, 3);
    status_case("a binary past the end", big.substr(0, 40), SMQ_ERR_TRUNCATED);
    S deep8, deep9;  // containers down to depth 8 and 9 (the PageHeader is 1)
    for (int d = 2; d <= 8; ++d) deep8 += fld(1, 12);
    deep9 = deep8 + fld(1, 12);
    status_case("nesting depth 8", head(1, 0, 0) + deep8 + S(7, '\0') + kStopByte, SM_OK, 1, 0);
    status_case("nesting depth 9", head(1, 0, 0) + deep9 + S(8, '\0') + kStopByte, SMQ_ERR_HEADER);
    status_case("unknown element type", head(1, 0, 0) + fld(1, 9) + S("\x2d", 1) + kStopByte, SMQ_ERR_HEADER);
    // long-form ids for the known fields
    const S lf = S("\x05", 1) + zz(1) + zz(0) + S("\x05", 1) + zz(2) + zz(3) + S("\x05", 1) + zz(3) + zz(5) + S("\x0c", 1) + zz(5) +
                 S("\x05", 1) + zz(1) + zz(3) + kStopByte + kStopByte + kAbc;
    status_case("long-form ids", lf, SM_OK, 1, 3);
  }

  // the entries
  {
    const S s = abc + index_page + v2c + dict + v2s;
    const Result r = walk(s);
    expect(r.sum.status == SM_OK && r.sum.npages == 5 && r.sum.total_length == 18, "entries: summary");
    const uint64_t o1 = abc.size(), o2 = o1 + index_page.size(), o3 = o2 + v2c.size(), o4 = o3 + dict.size();
    expect(r.hdr_off[0] == 0 && r.hdr_len[0] == abc.size() - 5 && r.body_len[0] == 5 && r.usize[0] == 3 && r.levels[0] == 0 &&
               r.out_off[0] == 0 && r.num_values[0] == 3 && r.type[0] == 0 && r.encoding[0] == 0 &&
               r.flags[0] == SMQ_PAGE_COMPRESSED && r.crc[0] == 0,
           "entries: page 0");
    expect(r.hdr_off[1] == o1 && r.body_len[1] == 4 && r.usize[1] == 99 && r.out_off[1] == 3 && r.type[1] == 1 && r.flags[1] == 0 &&
               r.num_values[1] == 0,
           "entries: the index page");
    expect(r.hdr_off[2] == o2 && r.body_len[2] == 8 && r.usize[2] == 6 && r.levels[2] == 3 && r.out_off[2] == 3 &&
               r.num_values[2] == 9 && r.type[2] == 3 && r.encoding[2] == 8 && r.flags[2] == SMQ_PAGE_COMPRESSED,
           "entries: the v2 page");
    expect(r.hdr_off[3] == o3 && r.usize[3] == 3 && r.out_off[3] == 9 && r.num_values[3] == 7 && r.type[3] == 2 &&
               r.encoding[3] == 2 && r.flags[3] == (SMQ_PAGE_HAS_CRC | SMQ_PAGE_COMPRESSED) && r.crc[3] == 0xfffffffeu,
           "entries: the dictionary page");
    expect(r.hdr_off[4] == o4 && r.body_len[4] == 6 && r.levels[4] == 3 && r.out_off[4] == 12 && r.flags[4] == 0,
           "entries: the stored v2 page");
    const Result small = walk(s, 4);
    expect(small.sum.status == SM_BUFFER_TOO_SMALL && small.sum.npages == 5 && small.hdr_off[3] == o3, "capacity too small");
    size_t total = 0;
    expect(smq_uncompressed_length((const uint8_t*)s.data(), s.size(), &total) == SM_OK && total == 18, "uncompressed length");
    smq_summary sum;
    expect(smq_index(nullptr, 4, nullptr, 0, &sum) == SM_ERR_ARGUMENT, "null buffer");
    expect(smq_index((const uint8_t*)s.data(), s.size(), nullptr, 0, nullptr) == SM_ERR_ARGUMENT, "null summary");
    smq_pages none{};
    expect(smq_index((const uint8_t*)s.data(), s.size(), &none, 1, &sum) == SM_ERR_ARGUMENT, "null arrays");
  }
  expect(smq::host_message(SMQ_ERR_HEADER) && smq::host_message(SMQ_ERR_TRUNCATED) && smq::host_message(SMQ_ERR_SIZE_MISMATCH) &&
             smq::host_message(SMQ_ERR_CRC) && !smq::host_message(SM_OK) && !smq::host_message(71) && !smq::host_message(76),
         "messages");
  chunks_cases();

  // the second total: a compressed section of 200,000 bytes is four fragments, a stored one none
  {
    const S big = head(0, 200000, 3) + data_header(3, 1, 0) + kStopByte + S("\xc0\x9a\x0c", 3);  // (structure only)
    const S raw = head(3, 70000, 70000) + v2_header(3, 1, 0, 0, 0, 0) + kStopByte + S(70000, 'r');
    const S batch = abc + big + big + raw;
    const uint64_t off[4] = {0, abc.size(), abc.size() + big.size(), abc.size() + 2 * big.size()};
    const uint64_t len[4] = {abc.size(), big.size(), big.size(), raw.size()}, cap[4] = {3, 200000, 199999, 70000};
    uint64_t pages = 0, frags = 0;
    int32_t st[4];
    expect(smq_chunks_plan((const uint8_t*)batch.data(), off, len, 4, cap, 3, nullptr, nullptr, st, &pages, &frags) == SM_OK &&
               pages == 3 && frags == 5 && st[0] == SM_OK && st[1] == SM_OK && st[2] == SM_BUFFER_TOO_SMALL && st[3] == SM_OK,
           "chunks plan: the fragments");
  }
  expect(smq_max_pages(0) == 0 && smq_max_pages(6) == 0 && smq_max_pages(7) == 1 && smq_max_pages(7000) == 1000, "max pages");
  expect(head(1, 0, 0).size() + 1 == 7, "the shortest page");
  expect(smq_chunks_scratch_bytes(3, 7, 0) > smq_chunks_scratch_bytes(3, 6, 0) &&
             smq_chunks_scratch_bytes(4, 7, 9) >= smq_chunks_scratch_bytes(3, 7, 9) && smq_chunks_scratch_bytes(0, 0, 0) > 0 &&
             smq_chunks_scratch_bytes(3, 0, 1000) > smq_chunks_scratch_bytes(3, 0, 1),
         "chunks scratch bytes");
  // the verdicts, the owner search and the copies' rows
  expect(smc::plan_verdict(true, SM_OK, smq::kNoSlot, 0) == SM_ERR_ARGUMENT &&
             smc::plan_verdict(false, SMQ_ERR_TRUNCATED, 3, 19) == SMQ_ERR_TRUNCATED && smc::plan_verdict(false, SM_OK, 3, 19) == 19 &&
             smc::plan_verdict(false, SM_OK, smq::kNoSlot, 19) == SM_OK,
         "chunk verdict");
  expect(smq::slot_verdict(smq::kNoSlot, true, 1, 2, true, 19) == SM_OK && smq::slot_verdict(2, true, 1, 2, true, 19) == SMQ_ERR_CRC &&
             smq::slot_verdict(2, true, 2, 2, true, 19) == 19 && smq::slot_verdict(2, false, 1, 2, true, 19) == 19 &&
             smq::slot_verdict(2, false, 1, 2, false, 19) == SM_OK && smq::slot_verdict(2, true, 2, 2, true, 0) == SM_OK,
         "slot verdict");
  {
    uint32_t* first = (uint32_t*)std::malloc(6 * sizeof(uint32_t));
    const uint32_t f[6] = {0, 0, 2, 2, 2, 5};  // owners 1 and 4 have items
    std::memcpy(first, f, sizeof(f));
    const uint32_t want[5] = {1, 1, 4, 4, 4};
    for (uint32_t j = 0; j < 5; ++j) expect(smc::slot_owner(first, 5, j) == want[j], "scan owner");
    std::free(first);
  }
  expect(smc::copy_rows(1, smq::kCopyTypical) == 64 && smc::copy_rows(100, smq::kCopyTypical) == 20 && smc::copy_rows(2500, smq::kCopyTypical) == 1 && smc::copy_rows(0, smq::kCopyTypical) == 64 &&
             smc::copy_rows(0x7fffffff, smq::kCopyTypical) == 1,
         "copy rows");
  {
    smq::Page p{0, 10, 8, 6, 3, 9, 3, 8, SMQ_PAGE_COMPRESSED, 0, true};
    expect(smq::section_len(p) == 5 && smq::section_want(p) == 3 && smq::copy_len(p) == 3, "a compressed page's parts");
    p.flags = 0;
    expect(smq::copy_len(p) == 8, "a stored page's copy");
    p.output = false;
    expect(smq::copy_len(p) == 0, "a page that is stepped over copies nothing");
  }
  crc_cases();
  encode_cases();

  if (failures) {
    std::printf("%d failure(s)\n", failures);
    return 1;
  }
  std::printf("smq_host_check ok\n");
  return 0;
}
