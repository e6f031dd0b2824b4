// smb_host_check.cpp -- stand-alone driver of the host-only blocks code (smb_host.cpp), built with
// -fsanitize=address,undefined by `make host_check`.  Every buffer is a heap block of exactly the
// stream's size, so a walk that reads past a cut stream trips the sanitizer; the batched decode's
// plan (smb_streams_plan) runs over the same cases laid directly behind one another.  The expected
// values are written out here; none comes from the code under test.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../common/smc_staging.h"
#include "smb_format.h"
#include "smb_streams.h"

namespace {

int failures = 0;

void expect(bool ok, const char* what) {
  if (!ok) {
    std::printf("FAIL %s\n", what);
    ++failures;
  }
}

typedef std::string S;

S be(uint32_t v) {
  S s;
  for (int i = 3; i >= 0; --i) s += (char)((v >> (8 * i)) & 0xff);
  return s;
}

S chunk(const S& payload) { return be((uint32_t)payload.size()) + payload; }

const S kMagic = S("\x82SNAPPY\0", 8);
const S kHeader = kMagic + be(1) + be(1);
const S kAbc = S("\x03\x08" "abc", 5);  // compress("abc")

struct Result {
  smb_summary sum;
  std::vector<uint64_t> off;
  std::vector<uint32_t> len, ulen;
};

Result walk(const S& stream, int format, uint32_t max_chunks = 16) {
  Result r;
  r.off.resize(max_chunks);
  r.len.resize(max_chunks);
  r.ulen.resize(max_chunks);
  uint8_t* heap = (uint8_t*)std::malloc(stream.size() ? stream.size() : 1);
  std::memcpy(heap, stream.data(), stream.size());
  const smb_chunks ch{r.off.data(), r.len.data(), r.ulen.data()};
  smb_index(heap, stream.size(), format, &ch, max_chunks, &r.sum);
  smb_summary count;
  smb_index(heap, stream.size(), format, nullptr, 0, &count);
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
std::vector<Case> cases[2];  // every status_case by format, for streams_cases

void status_case(const char* name, int format, const S& stream, int32_t status, uint32_t nchunks = 0, uint64_t total = 0) {
  cases[format].push_back(Case{stream, status, nchunks, total});
  const Result r = walk(stream, format);
  if (r.sum.status != status || r.sum.nchunks != nchunks || r.sum.total_length != total) {
    std::printf("FAIL %s (format %d): status %d (want %d), chunks %u (want %u), total %llu (want %llu)\n", name, format,
                r.sum.status, status, r.sum.nchunks, nchunks, (unsigned long long)r.sum.total_length,
                (unsigned long long)total);
    ++failures;
  }
}

// Every structural case of one format as one batch, the streams directly behind one another in a
// heap block of exactly their size: a walk that leaves its stream reads its neighbour (a wrong
// status) or, at the last stream, trips the sanitizer.
void streams_cases(int format) {
  const std::vector<Case>& cs = cases[format];
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
    return smb_streams_plan(heap, off.data(), len.data(), k, format, cap.data(), max_chunks, first.data(), out_len.data(),
                            status.data(), &total, &frags);
  };
  expect(run((uint32_t)slots) == SM_OK && total == slots && first == want_first, "streams plan: the scan");
  for (uint32_t s = 0; s < k; ++s)
    if (status[s] != cs[s].status || out_len[s] != cs[s].total) {
      std::printf("FAIL streams plan (format %d): stream %u status %d (want %d), length %llu (want %llu)\n", format, s,
                  status[s], cs[s].status, (unsigned long long)out_len[s], (unsigned long long)cs[s].total);
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
  expect(smb_streams_plan(heap, off.data(), len.data(), k, format, nullptr, 0x7fffffffu, nullptr, nullptr, nullptr, &total,
                          nullptr) == SM_OK && total == slots,
         "streams plan: null outputs");
  first[0] = 7;
  expect(smb_streams_plan(nullptr, nullptr, nullptr, 0, format, nullptr, 0, first.data(), nullptr, nullptr, &total, &frags) ==
                 SM_OK && total == 0 && frags == 0 && first[0] == 0,
         "streams plan: no streams");
  expect(smb_streams_plan(nullptr, off.data(), len.data(), k, format, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr) ==
                 SM_ERR_ARGUMENT &&
             smb_streams_plan(heap, nullptr, len.data(), k, format, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr) ==
                 SM_ERR_ARGUMENT &&
             smb_streams_plan(heap, off.data(), len.data(), k, 2, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr) ==
                 SM_ERR_ARGUMENT &&
             smb_streams_plan(heap, off.data(), len.data(), 0x80000000u, format, nullptr, 0, nullptr, nullptr, nullptr,
                              nullptr, nullptr) == SM_ERR_ARGUMENT,
         "streams plan: arguments");
  std::free(heap);
}

}  // namespace

int main() {
  const int H = SMB_FORMAT_HADOOP, X = SMB_FORMAT_XERIAL;
  const S c_abc = chunk(kAbc), one = be(3) + c_abc;
  expect(one == S("\0\0\0\x03\0\0\0\x05\x03\x08" "abc", 13), "golden HADOOP 'abc'");
  expect(kHeader + c_abc == S("\x82SNAPPY\0\0\0\0\x01\0\0\0\x01\0\0\0\x05\x03\x08" "abc", 25), "golden XERIAL 'abc'");

  status_case("empty stream", H, "", SM_OK);
  status_case("empty block", H, be(0), SM_OK);
  status_case("abc", H, one, SM_OK, 1, 3);
  status_case("payload one byte short", H, one.substr(0, one.size() - 1), SMB_ERR_TRUNCATED);
  status_case("clen 0", H, be(3) + be(0), SM_ERR_VARINT);
  status_case("clen just over the rest", H, be(3) + be(6) + kAbc, SMB_ERR_TRUNCATED);
  status_case("clen 0xffffffff", H, be(3) + be(0xffffffffu) + kAbc, SMB_ERR_TRUNCATED);
  status_case("ulen 0x80000000", H, be(0x80000000u) + c_abc, SMB_ERR_CHUNK_TOO_LARGE);
  status_case("ulen 0x7fffffff, no chunk", H, be(0x7fffffffu), SMB_ERR_TRUNCATED);
  status_case("two chunks sum to ulen", H, be(6) + c_abc + c_abc, SM_OK, 2, 6);
  status_case("two chunks one byte over", H, be(5) + c_abc + c_abc, SMB_ERR_BLOCK_LENGTH, 2, 6);
  status_case("one chunk over", H, be(2) + c_abc, SMB_ERR_BLOCK_LENGTH, 1, 3);
  status_case("block short of its chunks", H, be(7) + c_abc + c_abc, SMB_ERR_TRUNCATED, 2, 6);
  status_case("empty block between two", H, one + be(0) + one, SM_OK, 2, 6);
  status_case("empty blocks only", H, be(0) + be(0), SM_OK);
  status_case("a chunk declaring 0 inside a block", H, be(3) + chunk(S(1, '\0')) + c_abc, SM_OK, 2, 3);
  status_case("varint of 1 byte", H, be(0x7f) + chunk("\x7f"), SM_OK, 1, 0x7f);
  status_case("varint of 2 bytes", H, be(0x3fff) + chunk("\xff\x7f"), SM_OK, 1, 0x3fff);
  status_case("varint of 3 bytes", H, be(0x1fffff) + chunk("\xff\xff\x7f"), SM_OK, 1, 0x1fffff);
  status_case("varint of 4 bytes", H, be(0xfffffff) + chunk("\xff\xff\xff\x7f"), SM_OK, 1, 0xfffffff);
  status_case("varint of 5 bytes", H, be(0x7fffffffu) + chunk("\xff\xff\xff\xff\x07"), SM_OK, 1, 0x7fffffffu);
  status_case("varint 0x80000000", H, be(0x7fffffffu) + chunk("\x80\x80\x80\x80\x08"), SMB_ERR_CHUNK_TOO_LARGE);
  status_case("varint unterminated", H, be(3) + chunk("\x80\x80"), SM_ERR_VARINT);
  status_case("varint too long", H, be(3) + chunk("\x80\x80\x80\x80\x10"), SM_ERR_VARINT);
  status_case("varint of 6 bytes", H, be(3) + chunk("\x80\x80\x80\x80\x80\x01"), SM_ERR_VARINT);
  status_case("second block cut", H, one + be(3) + c_abc.substr(0, 6), SMB_ERR_TRUNCATED, 1, 3);
  for (size_t cut = 1; cut <= 3; ++cut) {
    status_case("ulen cut", H, one.substr(0, cut), SMB_ERR_TRUNCATED);
    status_case("clen cut", H, one.substr(0, 4 + cut), SMB_ERR_TRUNCATED);
    status_case("second ulen cut", H, one + one.substr(0, cut), SMB_ERR_TRUNCATED, 1, 3);
  }
  status_case("clen missing", H, one.substr(0, 4), SMB_ERR_TRUNCATED);

  status_case("header alone", X, kHeader, SM_OK);
  status_case("abc", X, kHeader + c_abc, SM_OK, 1, 3);
  status_case("two chunks", X, kHeader + c_abc + chunk(S(1, '\0')), SM_OK, 2, 3);
  status_case("version 0", X, kMagic + be(0) + be(1) + c_abc, SMB_ERR_BAD_HEADER);
  status_case("version 2, compatible version 0", X, kMagic + be(2) + be(0) + c_abc, SM_OK, 1, 3);
  status_case("repeated header", X, kHeader + c_abc + kHeader + c_abc, SM_OK, 2, 6);
  status_case("repeated header at the end", X, kHeader + c_abc + kHeader, SM_OK, 1, 3);
  status_case("repeated header cut short", X, kHeader + c_abc + kHeader.substr(0, 15), SMB_ERR_TRUNCATED, 1, 3);
  status_case("repeated header cut after its word", X, kHeader + c_abc + kHeader.substr(0, 4), SMB_ERR_TRUNCATED, 1, 3);
  status_case("repeated header, wrong second half", X, kHeader + c_abc + kHeader.substr(0, 7) + S("\x01", 1) + kHeader.substr(8),
              SMB_ERR_BAD_HEADER, 1, 3);
  status_case("repeated header, version 0", X, kHeader + c_abc + kMagic + be(0) + be(1), SMB_ERR_BAD_HEADER, 1, 3);
  status_case("clen 0", X, kHeader + be(0), SM_ERR_VARINT);
  status_case("clen just over the rest", X, kHeader + be(6) + kAbc, SMB_ERR_TRUNCATED);
  status_case("clen 0xffffffff", X, kHeader + be(0xffffffffu), SMB_ERR_TRUNCATED);
  status_case("payload one byte short", X, kHeader + c_abc.substr(0, c_abc.size() - 1), SMB_ERR_TRUNCATED);
  status_case("varint unterminated", X, kHeader + c_abc + chunk("\xff"), SM_ERR_VARINT, 1, 3);
  status_case("varint 0x80000000", X, kHeader + chunk("\x80\x80\x80\x80\x08"), SMB_ERR_CHUNK_TOO_LARGE);
  status_case("hadoop stream", X, one, SMB_ERR_NO_HEADER);
  for (size_t cut = 1; cut <= 3; ++cut) status_case("clen cut", X, kHeader + c_abc + c_abc.substr(0, cut), SMB_ERR_TRUNCATED, 1, 3);
  for (size_t i = 0; i < 8; ++i) {
    S bad = kHeader + c_abc;
    bad[i] ^= 0x20;
    status_case("magic byte wrong", X, bad, SMB_ERR_NO_HEADER);
  }
  for (size_t n = 0; n < 16; ++n) status_case("header cut", X, kHeader.substr(0, n), n ? SMB_ERR_TRUNCATED : SMB_ERR_NO_HEADER);
  status_case("one wrong byte alone", X, "\x83", SMB_ERR_NO_HEADER);
  status_case("wrong byte 3 of 5", X, kMagic.substr(0, 2) + S(1, '\0') + kMagic.substr(3, 2), SMB_ERR_NO_HEADER);

  // the entries, and a capacity that is too small
  {
    const S s = one + be(0) + be(6) + c_abc + chunk(kAbc + "x");  // (the last payload has a stray byte: structure only)
    const Result r = walk(s, H);
    expect(r.sum.status == SM_OK && r.sum.nchunks == 3 && r.sum.total_length == 9, "entries: summary");
    expect(r.off[0] == 8 && r.len[0] == 5 && r.ulen[0] == 3, "entries: chunk 0");
    expect(r.off[1] == 13 + 4 + 4 + 4 && r.len[1] == 5 && r.ulen[1] == 3, "entries: chunk 1");
    expect(r.off[2] == 13 + 4 + 4 + 9 + 4 && r.len[2] == 6 && r.ulen[2] == 3, "entries: chunk 2");
    const Result small = walk(s, H, 2);
    expect(small.sum.status == SM_BUFFER_TOO_SMALL && small.sum.nchunks == 3 && small.off[1] == 25, "capacity too small");
    const Result x = walk(kHeader + c_abc + kHeader + c_abc, X);
    expect(x.off[0] == 20 && x.off[1] == 20 + 5 + 16 + 4 && x.ulen[1] == 3, "entries: XERIAL");
    size_t total = 0;
    expect(smb_uncompressed_length((const uint8_t*)s.data(), s.size(), H, &total) == SM_OK && total == 9, "uncompressed length");
    smb_summary sum;
    expect(smb_index(nullptr, 4, H, nullptr, 0, &sum) == SM_ERR_ARGUMENT, "null buffer");
    expect(smb_index((const uint8_t*)s.data(), s.size(), H, nullptr, 0, nullptr) == SM_ERR_ARGUMENT, "null summary");
    expect(smb_index((const uint8_t*)s.data(), s.size(), 2, nullptr, 0, &sum) == SM_ERR_ARGUMENT, "unknown format");
  }
  expect(smb::host_message(SMB_ERR_BLOCK_LENGTH) != nullptr && smb::host_message(SM_OK) == nullptr &&
             smb::host_message(61) == nullptr && smb::host_message(55) == nullptr,
         "messages");
  streams_cases(H);
  streams_cases(X);

  // the second total: a chunk of 200,000 bytes is four fragments; a stream that is not decoded has none
  {
    const S big = be(200000) + chunk(S("\xc0\x9a\x0c", 3)), batch = one + big + big;
    const uint64_t off[3] = {0, 13, 13 + big.size()}, len[3] = {13, big.size(), big.size()}, cap[3] = {3, 200000, 199999};
    uint64_t chunks = 0, frags = 0;
    int32_t st[3];
    expect(smb_streams_plan((const uint8_t*)batch.data(), off, len, 3, H, cap, 2, nullptr, nullptr, st, &chunks, &frags) == SM_OK &&
               chunks == 2 && frags == 5 && st[0] == SM_OK && st[1] == SM_OK && st[2] == SM_BUFFER_TOO_SMALL,
           "streams plan: the fragments");
  }
  // the size helpers: 32 + n + n / 6 per piece, 8 or 4 a chunk, 16 for the header
  expect(smb_max_length(0, H) == 4 && smb_max_length(0, X) == 16 && smb_max_length(1, H) == 41 && smb_max_length(1, X) == 53 &&
             smb_max_length(65536, H) == 76490 + 8 && smb_max_length(65537, H) == 76490 + 8 + 33 + 8 &&
             smb_max_length(131073, X) == 16 + 2 * (76490 + 4) + 33 + 4,
         "max length");
  expect(smb_max_chunks(0, H) == 0 && smb_max_chunks(4, H) == 0 && smb_max_chunks(5, H) == 1 && smb_max_chunks(5000, H) == 1000 &&
             smb_max_chunks(15, X) == 0 && smb_max_chunks(20, X) == 0 && smb_max_chunks(21, X) == 1 &&
             smb_max_chunks(16 + 5000, X) == 1000,
         "max chunks");
  expect(smb_streams_scratch_bytes(3, 7, 0) > smb_streams_scratch_bytes(3, 6, 0) &&
             smb_streams_scratch_bytes(4, 7, 9) >= smb_streams_scratch_bytes(3, 7, 9) && smb_streams_scratch_bytes(0, 0, 0) > 0,
         "streams scratch bytes");
  // the verdict and the slot search
  expect(smc::plan_verdict(true, SM_OK, smb::kNoSlot, 0) == SM_ERR_ARGUMENT &&
             smc::plan_verdict(true, SMB_ERR_TRUNCATED, 3, 19) == SM_ERR_ARGUMENT &&
             smc::plan_verdict(false, SMB_ERR_TRUNCATED, 3, 19) == SMB_ERR_TRUNCATED &&
             smc::plan_verdict(false, SM_OK, 3, 19) == 19 && smc::plan_verdict(false, SM_OK, 0, 19) == 19 &&
             smc::plan_verdict(false, SM_OK, smb::kNoSlot, 19) == SM_OK,
         "stream verdict");
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
  // the host-buffer calls' staging (../common/smc_staging.h): the inputs behind one another in the
  // order of the streams, wherever they stand in the caller's buffer (a heap block of exactly the
  // bytes in use), each output from a 16-byte boundary, an empty stream in between, and no stream
  {
    const S text = "....abcdefg.xy";  // stream 0: "xy" at 12, stream 1: empty (its offset past the end), stream 2: "abcdefg" at 4
    uint8_t* in = (uint8_t*)std::malloc(text.size());
    std::memcpy(in, text.data(), text.size());
    const uint64_t off[3] = {12, 1000, 4}, len[3] = {2, 0, 7}, room[3] = {17, 0, 16};
    const StreamStaging h(in, off, len, 3, room);
    expect(h.bytes.size() == 9 && std::memcmp(h.bytes.data(), "xyabcdefg", 9) == 0, "staging: the packed bytes");
    expect(h.in_off[0] == 0 && h.in_off[1] == 2 && h.in_off[2] == 2, "staging: input offsets");
    expect(h.out_off[0] == 0 && h.out_off[1] == 32 && h.out_off[2] == 32 && h.out_total == 48, "staging: output offsets");
    std::free(in);
    const uint64_t none = 0;
    const StreamStaging e(nullptr, &none, &none, 1, &none);  // one empty stream of a null buffer
    expect(e.bytes.empty() && e.in_off[0] == 0 && e.out_off[0] == 0 && e.out_total == 0, "staging: an empty stream");
    const StreamStaging z(nullptr, nullptr, nullptr, 0, nullptr);
    expect(z.bytes.empty() && z.in_off.empty() && z.out_off.empty() && z.out_total == 0, "staging: no stream");
    expect(smc::round16(0) == 0 && smc::round16(1) == 16 && smc::round16(16) == 16 && smc::round16(17) == 32 &&
               smc::round16(0xfffffffffffffff0ull) == 0xfffffffffffffff0ull,
           "round16");
    // the call's arrays: six of them, each from a 16-byte boundary, none for no stream
    const StreamCallArrays a = carve_stream_call(4096, 3);
    expect((uintptr_t)a.in_off == 4096 && (uintptr_t)a.in_len == 4096 + 32 && (uintptr_t)a.out_off == 4096 + 64 &&
               (uintptr_t)a.out_cap == 4096 + 96 && (uintptr_t)a.out_len == 4096 + 128 && (uintptr_t)a.status == 4096 + 160 &&
               a.end == 4096 + 176,
           "stream call arrays");
    expect(stream_call_bytes(0) == 0 && stream_call_bytes(1) == 96 && stream_call_bytes(3) == 176 &&
               stream_call_bytes(4) == 5 * 32 + 16,
           "stream call bytes");
  }
  // the prefix bytes the pack kernel writes
  {
    S h, x, hdr;
    for (uint32_t i = 0; i < 8; ++i) h += (char)smb::chunk_prefix_byte(H, i, 0x01020304u, 0x0a0b0c0du);
    for (uint32_t i = 0; i < 4; ++i) x += (char)smb::chunk_prefix_byte(X, i, 0x01020304u, 0x0a0b0c0du);
    for (uint32_t i = 0; i < 16; ++i) hdr += (char)smb::stream_prefix_byte(X, i);
    expect(h == S("\x01\x02\x03\x04\x0a\x0b\x0c\x0d", 8) && x == S("\x0a\x0b\x0c\x0d", 4) && hdr == kHeader, "prefix bytes");
    expect(smb::stream_fixed_bytes(H, 0) == 4 && smb::stream_fixed_bytes(H, 1) == 0 && smb::stream_fixed_bytes(X, 0) == 16 &&
               smb::stream_prefix_byte(H, 3) == 0 && smb::stream_blocks(0) == 0 && smb::stream_blocks(65536) == 1 &&
               smb::stream_blocks(65537) == 2,
           "fixed bytes");
  }

  if (failures) {
    std::printf("%d failure(s)\n", failures);
    return 1;
  }
  std::printf("smb_host_check ok\n");
  return 0;
}
