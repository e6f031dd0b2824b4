// smo_host_check.cpp -- stand-alone driver of the host-only ORC code (smo_host.cpp), built with
// -fsanitize=address,undefined by `make host_check`.  Every buffer is a heap block of exactly the
// stream's size, so a walk that reads past a cut stream trips the sanitizer; the batched decode's
// plan (smo_streams_plan) runs over the same cases laid directly behind one another.  The expected
// values are written out here; none comes from the code under test.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "smo_format.h"
#include "smo_streams.h"

namespace {

int failures = 0;

void expect(bool ok, const char* what) {
  if (!ok) {
    std::printf("FAIL %s\n", what);
    ++failures;
  }
}

typedef std::string S;

S header(uint32_t L, bool original) {
  const uint32_t H = (L << 1) | (original ? 1u : 0u);
  S s;
  for (int i = 0; i < 3; ++i) s += (char)((H >> (8 * i)) & 0xff);
  return s;
}

S stored(const S& bytes) { return header((uint32_t)bytes.size(), true) + bytes; }
S compressed(const S& payload) { return header((uint32_t)payload.size(), false) + payload; }

const S kAbc = S("\x03\x08" "abc", 5);  // compress("abc")
const uint32_t kBlock = 1000;           // the cases' compression block size

struct Result {
  smo_summary sum;
  std::vector<uint64_t> off;
  std::vector<uint32_t> len, ulen;
  std::vector<uint8_t> original;
};

Result walk(const S& stream, uint32_t block_size, uint32_t max_chunks = 16) {
  Result r;
  r.off.resize(max_chunks);
  r.len.resize(max_chunks);
  r.ulen.resize(max_chunks);
  r.original.resize(max_chunks);
  uint8_t* heap = (uint8_t*)std::malloc(stream.size() ? stream.size() : 1);
  std::memcpy(heap, stream.data(), stream.size());
  const smo_chunks ch{r.off.data(), r.len.data(), r.ulen.data(), r.original.data()};
  r.sum = smo_summary{0, 0, 0};
  r.sum.status = smo_index(heap, stream.size(), block_size, &ch, max_chunks, &r.sum);  // (a refused call leaves the summary)
  smo_summary count{0, 0, 0};
  smo_index(heap, stream.size(), block_size, nullptr, 0, &count);
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
  const Result r = walk(stream, kBlock);
  if (r.sum.status != status || r.sum.nchunks != nchunks || r.sum.total_length != total) {
    std::printf("FAIL %s: status %d (want %d), chunks %u (want %u), total %llu (want %llu)\n", name, r.sum.status, status,
                r.sum.nchunks, nchunks, (unsigned long long)r.sum.total_length, (unsigned long long)total);
    ++failures;
  }
}

// Every structural case as one batch, the streams directly behind one another in a heap block of
// exactly their size: a walk that leaves its stream reads its neighbour (a wrong status) or, at the
// last stream, trips the sanitizer.
void streams_cases() {
  const std::vector<Case>& cs = cases;
  const uint32_t k = (uint32_t)cs.size();
  std::vector<uint64_t> off(k), len(k), cap(k), out_len(k);
  std::vector<uint32_t> first(k + 1), want_first(k + 1);
  std::vector<int32_t> status(k);
  uint64_t n = 0, slots = 0;
  for (uint32_t s = 0; s < k; ++s) {
    off[s] = n;
    len[s] = cs[s].stream.size();
    n += len[s];
    cap[s] = cs[s].total;
    want_first[s] = (uint32_t)slots;
    slots += cs[s].status == SM_OK ? cs[s].nchunks : 0;
  }
  want_first[k] = (uint32_t)slots;
  uint8_t* heap = (uint8_t*)std::malloc(n);
  for (uint32_t s = 0; s < k; ++s) std::memcpy(heap + off[s], cs[s].stream.data(), len[s]);
  uint64_t total = 0, frags = 0;
  auto run = [&](uint32_t max_chunks) {
    return smo_streams_plan(heap, off.data(), len.data(), k, kBlock, cap.data(), max_chunks, first.data(), out_len.data(),
                            status.data(), &total, &frags);
  };
  expect(run((uint32_t)slots) == SM_OK && total == slots && first == want_first, "streams plan: the scan");
  for (uint32_t s = 0; s < k; ++s)
    if (status[s] != cs[s].status || out_len[s] != cs[s].total) {
      std::printf("FAIL streams plan: stream %u status %d (want %d), length %llu (want %llu)\n", s, status[s], cs[s].status,
                  (unsigned long long)out_len[s], (unsigned long long)cs[s].total);
      ++failures;
    }
  // a byte short: that stream alone changes, and it gives its slots up
  for (uint32_t v = 0; v < k; ++v) {
    if (cs[v].status != SM_OK || cs[v].total == 0) continue;
    --cap[v];
    expect(run((uint32_t)slots) == SM_OK && total == slots - cs[v].nchunks, "a byte short: the total");
    for (uint32_t s = 0; s < k; ++s)
      expect(status[s] == (s == v ? (int32_t)SM_BUFFER_TOO_SMALL : cs[s].status) && out_len[s] == cs[s].total,
             "a byte short: the statuses");
    expect(first[v + 1] == first[v], "a byte short: no slots");
    ++cap[v];
  }
  // one slot short: nothing is planned
  expect(run((uint32_t)slots - 1) == SM_BUFFER_TOO_SMALL && total == slots, "one slot short");
  for (uint32_t s = 0; s < k; ++s) expect(status[s] == SM_ERR_ARGUMENT && out_len[s] == 0, "one slot short: the statuses");
  // no room limit, no outputs, no streams, bad arguments
  expect(smo_streams_plan(heap, off.data(), len.data(), k, kBlock, nullptr, 0x7fffffffu, nullptr, nullptr, nullptr, &total,
                          nullptr) == SM_OK && total == slots,
         "streams plan: null outputs");
  first[0] = 7;
  expect(smo_streams_plan(nullptr, nullptr, nullptr, 0, kBlock, nullptr, 0, first.data(), nullptr, nullptr, &total, &frags) ==
                 SM_OK && total == 0 && frags == 0 && first[0] == 0,
         "streams plan: no streams");
  expect(smo_streams_plan(nullptr, off.data(), len.data(), k, kBlock, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr) ==
                 SM_ERR_ARGUMENT &&
             smo_streams_plan(heap, nullptr, len.data(), k, kBlock, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr) ==
                 SM_ERR_ARGUMENT &&
             smo_streams_plan(heap, off.data(), len.data(), k, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr) ==
                 SM_ERR_ARGUMENT &&
             smo_streams_plan(heap, off.data(), len.data(), k, 0x800000u, nullptr, 0, nullptr, nullptr, nullptr, nullptr,
                              nullptr) == SM_ERR_ARGUMENT &&
             smo_streams_plan(heap, off.data(), len.data(), 0x80000000u, kBlock, nullptr, 0, nullptr, nullptr, nullptr,
                              nullptr, nullptr) == SM_ERR_ARGUMENT,
         "streams plan: arguments");
  std::free(heap);
}

}  // namespace

int main() {
  // the ORC specification's two examples, and this project's pinned stream of "abc"
  expect(header(100000, false) == S("\x40\x0d\x03", 3), "golden: 100,000 compressed bytes");
  expect(header(5, true) == S("\x0b\x00\x00", 3), "golden: five stored bytes");
  expect(stored("abc") == S("\x07\x00\x00" "abc", 6), "golden 'abc' stored");
  {
    S h;
    for (uint32_t i = 0; i < 3; ++i) h += (char)smo::chunk_header_byte(i, 100000, false);
    for (uint32_t i = 0; i < 3; ++i) h += (char)smo::chunk_header_byte(i, 5, true);
    expect(h == S("\x40\x0d\x03\x0b\x00\x00", 6), "header bytes the pack kernel writes");
    expect(smo::piece_stored(3, 5) && smo::piece_stored(5, 5) && !smo::piece_stored(6, 5), "the stored choice");
  }

  const S c_abc = compressed(kAbc), s_abc = stored("abc");
  status_case("empty stream", "", SM_OK);
  status_case("one stray byte", S("\x07", 1), SMO_ERR_TRUNCATED);
  status_case("two stray bytes", S("\x07\x00", 2), SMO_ERR_TRUNCATED);
  status_case("abc stored", s_abc, SM_OK, 1, 3);
  status_case("abc compressed", c_abc, SM_OK, 1, 3);
  status_case("stored payload one byte short", s_abc.substr(0, s_abc.size() - 1), SMO_ERR_TRUNCATED);
  status_case("compressed payload one byte short", c_abc.substr(0, c_abc.size() - 1), SMO_ERR_TRUNCATED);
  status_case("header alone, L 3", header(3, true), SMO_ERR_TRUNCATED);
  status_case("L 0 stored", header(0, true), SM_OK, 1, 0);
  status_case("L 0 compressed", header(0, false), SM_ERR_VARINT);
  status_case("L 0 stored between two", s_abc + header(0, true) + c_abc, SM_OK, 3, 6);
  status_case("L 0x7fffff", header(0x7fffff, true) + "abc", SMO_ERR_TRUNCATED);
  status_case("second chunk cut at 1", c_abc + s_abc.substr(0, 1), SMO_ERR_TRUNCATED, 1, 3);
  status_case("second chunk cut at 2", c_abc + s_abc.substr(0, 2), SMO_ERR_TRUNCATED, 1, 3);
  status_case("second chunk's payload cut", s_abc + c_abc.substr(0, 7), SMO_ERR_TRUNCATED, 1, 3);
  status_case("varint of 1 byte", compressed("\x7f"), SM_OK, 1, 0x7f);
  status_case("varint of 2 bytes", compressed("\xe8\x07"), SM_OK, 1, 1000);
  status_case("varint unterminated", compressed("\x80\x80"), SM_ERR_VARINT);
  status_case("varint of 5 bytes overflows", compressed("\x80\x80\x80\x80\x10"), SM_ERR_VARINT);
  status_case("varint of 6 bytes", compressed("\x80\x80\x80\x80\x80\x01"), SM_ERR_VARINT);
  status_case("varint of 5 bytes, too large", compressed("\xff\xff\xff\xff\x07"), SMO_ERR_CHUNK_TOO_LARGE);
  status_case("varint unterminated behind a chunk", s_abc + compressed("\xff"), SM_ERR_VARINT, 1, 3);
  status_case("stored, d == block_size", stored(S(1000, 'x')), SM_OK, 1, 1000);
  status_case("stored, d == block_size + 1", stored(S(1001, 'x')), SMO_ERR_CHUNK_TOO_LARGE);
  status_case("compressed, d == block_size", compressed("\xe8\x07"), SM_OK, 1, 1000);
  status_case("compressed, d == block_size + 1", compressed("\xe9\x07"), SMO_ERR_CHUNK_TOO_LARGE);
  status_case("too large behind a chunk", c_abc + compressed("\xe9\x07"), SMO_ERR_CHUNK_TOO_LARGE, 1, 3);

  // the entries, a capacity that is too small, the block size's range
  {
    const S s = s_abc + header(0, true) + compressed(kAbc + "x") + stored("hello");  // (a stray payload byte: structure only)
    const Result r = walk(s, kBlock);
    expect(r.sum.status == SM_OK && r.sum.nchunks == 4 && r.sum.total_length == 11, "entries: summary");
    expect(r.off[0] == 3 && r.len[0] == 3 && r.ulen[0] == 3 && r.original[0] == 1, "entries: chunk 0");
    expect(r.off[1] == 9 && r.len[1] == 0 && r.ulen[1] == 0 && r.original[1] == 1, "entries: chunk 1");
    expect(r.off[2] == 12 && r.len[2] == 6 && r.ulen[2] == 3 && r.original[2] == 0, "entries: chunk 2");
    expect(r.off[3] == 21 && r.len[3] == 5 && r.ulen[3] == 5 && r.original[3] == 1, "entries: chunk 3");
    const Result small = walk(s, kBlock, 3);
    expect(small.sum.status == SM_BUFFER_TOO_SMALL && small.sum.nchunks == 4 && small.off[2] == 12, "capacity too small");
    expect(walk(s, 5).sum.status == SM_OK && walk(s, 4).sum.status == SMO_ERR_CHUNK_TOO_LARGE && walk(s, 4).sum.nchunks == 3,
           "block size 5 and 4");
    expect(walk(s, 0x7fffff).sum.status == SM_OK && walk(s, 0).sum.status == SM_ERR_ARGUMENT &&
               walk(s, 0x800000).sum.status == SM_ERR_ARGUMENT,
           "block size range");
    size_t total = 0;
    expect(smo_uncompressed_length((const uint8_t*)s.data(), s.size(), kBlock, &total) == SM_OK && total == 11,
           "uncompressed length");
    smo_summary sum;
    expect(smo_index(nullptr, 4, kBlock, nullptr, 0, &sum) == SM_ERR_ARGUMENT, "null buffer");
    expect(smo_index((const uint8_t*)s.data(), s.size(), kBlock, nullptr, 0, nullptr) == SM_ERR_ARGUMENT, "null summary");
  }
  expect(smo::host_message(SMO_ERR_TRUNCATED) != nullptr && smo::host_message(SMO_ERR_CHUNK_TOO_LARGE) != nullptr &&
             smo::host_message(SM_OK) == nullptr && smo::host_message(63) == nullptr && smo::host_message(66) == nullptr,
         "messages");
  streams_cases();

  // the second total: a compressed chunk of 200,000 bytes is four fragments, a stored one none; a
  // stream that is not decoded has none
  {
    const S big = compressed(S("\xc0\x9a\x0c", 3)), raw = stored(S(70000, 'r')), batch = c_abc + big + big + raw;
    const uint64_t off[4] = {0, c_abc.size(), c_abc.size() + big.size(), c_abc.size() + 2 * big.size()};
    const uint64_t len[4] = {c_abc.size(), big.size(), big.size(), raw.size()}, cap[4] = {3, 200000, 199999, 70000};
    uint64_t chunks = 0, frags = 0;
    int32_t st[4];
    expect(smo_streams_plan((const uint8_t*)batch.data(), off, len, 4, 262144, cap, 3, nullptr, nullptr, st, &chunks, &frags) ==
                   SM_OK && chunks == 3 && frags == 5 && st[0] == SM_OK && st[1] == SM_OK && st[2] == SM_BUFFER_TOO_SMALL &&
               st[3] == SM_OK,
           "streams plan: the fragments");
  }
  // the size helpers
  expect(smo_max_length(0, 1000) == 0 && smo_max_length(1, 1000) == 4 && smo_max_length(1000, 1000) == 1003 &&
             smo_max_length(1001, 1000) == 1007 && smo_max_length(7, 1) == 28 && smo_max_length(5, 0) == 0 &&
             smo_max_length(5, 0x800000) == 0 && smo_max_length(0x7fffff, 0x7fffff) == 0x7fffff + 3,
         "max length");
  expect(smo_max_chunks(0) == 0 && smo_max_chunks(2) == 0 && smo_max_chunks(3) == 1 && smo_max_chunks(5) == 1 &&
             smo_max_chunks(3000) == 1000,
         "max chunks");
  expect(smo::stream_pieces(0, 7) == 0 && smo::stream_pieces(7, 7) == 1 && smo::stream_pieces(8, 7) == 2 &&
             smo::piece_fragment_bound(10, 65536) == 0 && smo::piece_fragment_bound(10, 65537) == 20 &&
             smo::piece_fragment_bound(10, 262144) == 40,
         "pieces and their fragment bound");
  expect(smo_streams_scratch_bytes(3, 7, 0, 1000) > smo_streams_scratch_bytes(3, 6, 0, 1000) &&
             smo_streams_scratch_bytes(4, 7, 9, 1000) >= smo_streams_scratch_bytes(3, 7, 9, 1000) &&
             smo_streams_scratch_bytes(0, 0, 0, 1000) > 0 && smo_streams_scratch_bytes(1, 10, 0, 262144) >= 10 * 305920u,
         "streams scratch bytes");
  // the verdicts, the slot search and the copies' rows
  expect(smc::plan_verdict(true, SM_OK, smo::kNoSlot, 0) == SM_ERR_ARGUMENT &&
             smc::plan_verdict(true, SMO_ERR_TRUNCATED, 3, 19) == SM_ERR_ARGUMENT &&
             smc::plan_verdict(false, SMO_ERR_TRUNCATED, 3, 19) == SMO_ERR_TRUNCATED &&
             smc::plan_verdict(false, SM_OK, 3, 19) == 19 && smc::plan_verdict(false, SM_OK, 0, 19) == 19 &&
             smc::plan_verdict(false, SM_OK, smo::kNoSlot, 19) == SM_OK,
         "stream verdict");
  expect(smo::slot_verdict(smo::kNoSlot, smo::kNoCopy, 19) == SM_OK && smo::slot_verdict(2, 0, 19) == SM_OK &&
             smo::slot_verdict(2, 70000, 18) == SM_OK && smo::slot_verdict(2, smo::kNoCopy, 19) == 19 &&
             smo::slot_verdict(2, smo::kNoCopy, SM_OK) == SM_OK,
         "slot verdict");
  {
    uint32_t* first = (uint32_t*)std::malloc(6 * sizeof(uint32_t));
    const uint32_t f[6] = {0, 0, 2, 2, 2, 5};  // streams 1 and 4 have slots
    std::memcpy(first, f, sizeof(f));
    const uint32_t want[5] = {1, 1, 4, 4, 4};
    for (uint32_t j = 0; j < 5; ++j) expect(smc::slot_owner(first, 5, j) == want[j], "slot stream");
    first[1] = 1;
    expect(smc::slot_owner(first, 1, 0) == 0, "slot stream: one stream");
    std::free(first);
  }
  expect(smc::copy_rows(1, 1) == 1 && smc::copy_rows(1, 16384) == 1 && smc::copy_rows(1, 16385) == 2 &&
             smc::copy_rows(1, 0x7fffff) == 512 && smc::copy_rows(100, 0x7fffff) == 20 && smc::copy_rows(2500, 262144) == 1 &&
             smc::copy_rows(0, 262144) == 16 && smc::copy_rows(0x7fffffff, 0x7fffff) == 1,
         "copy rows");

  if (failures) {
    std::printf("%d failure(s)\n", failures);
    return 1;
  }
  std::printf("smo_host_check ok\n");
  return 0;
}
