// sma_host_check.cpp -- stand-alone driver of the host-only Avro container code (sma_host.cpp),
// built with -fsanitize=address,undefined by `make host_check`.  Every buffer is a heap block of
// exactly the stream's size, so a walk that reads past a cut stream trips the sanitizer; the batched
// decode's plan (sma_streams_plan) runs over the same cases laid directly behind one another.  The
// expected values are written out here; none comes from the code under test.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "sma_format.h"
#include "sma_streams.h"

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

// a long, written out the slow way: zigzag, then 7 bits a byte
S lng(long long v) {
  unsigned long long u = v < 0 ? ((unsigned long long)(-(v + 1)) * 2 + 1) : (unsigned long long)v * 2;
  S s;
  do {
    unsigned char b = (unsigned char)(u % 128);
    u /= 128;
    if (u) b = (unsigned char)(b + 128);
    s += (char)b;
  } while (u);
  return s;
}

S str(const S& t) { return lng((long long)t.size()) + t; }

const S kMagic = S("Obj\x01", 4);
const S kSync = S("0123456789abcdef", 16);
const S kOther = S("0123456789abcdeX", 16);
const S kAbc = S("\x03\x08" "abc", 5);   // compress("abc")
const uint32_t kAbcCrc = 0x352441c2u;     // CRC-32 of "abc"

S meta(const S& codec) { return lng(2) + str("avro.schema") + str("\"bytes\"") + str("avro.codec") + str(codec) + lng(0); }
S header(const S& codec = "snappy") { return kMagic + meta(codec) + kSync; }
S block(long long count, const S& payload, uint32_t crc, const S& sync = kSync) {
  return lng(count) + lng((long long)payload.size() + 4) + payload + be(crc) + sync;
}

struct Result {
  sma_summary sum;
  std::vector<uint64_t> pay_off, count, out_off;
  std::vector<uint32_t> pay_len, ulen, crc;
};

Result walk(const S& stream, int kind, uint32_t max_blocks = 16) {
  Result r;
  r.pay_off.resize(max_blocks);
  r.count.resize(max_blocks);
  r.out_off.resize(max_blocks);
  r.pay_len.resize(max_blocks);
  r.ulen.resize(max_blocks);
  r.crc.resize(max_blocks);
  uint8_t* heap = (uint8_t*)std::malloc(stream.size() ? stream.size() : 1);
  std::memcpy(heap, stream.data(), stream.size());
  const sma_blocks b{r.pay_off.data(), r.pay_len.data(), r.ulen.data(), r.count.data(), r.crc.data(), r.out_off.data()};
  sma_index(heap, stream.size(), kind, (const uint8_t*)kSync.data(), &b, max_blocks, &r.sum);
  sma_summary count;
  sma_index(heap, stream.size(), kind, (const uint8_t*)kSync.data(), nullptr, 0, &count);
  expect(count.nblocks == r.sum.nblocks && count.total_length == r.sum.total_length && count.objects == r.sum.objects,
         "count-only walk agrees");
  std::free(heap);
  return r;
}

struct Case {
  S stream;
  int32_t status;
  uint32_t nblocks;
  uint64_t total;
};
std::vector<Case> cases;  // every file status_case, for streams_cases

void status_case(const char* name, int kind, const S& stream, int32_t status, uint32_t nblocks = 0, uint64_t total = 0,
                 uint64_t objects = 0) {
  if (kind == SMA_INPUT_FILE) cases.push_back(Case{stream, status, nblocks, total});
  const Result r = walk(stream, kind);
  if (r.sum.status != status || r.sum.nblocks != nblocks || r.sum.total_length != total || r.sum.objects != objects) {
    std::printf("FAIL %s (kind %d): status %d (want %d), blocks %u (want %u), total %llu (want %llu), objects %llu (want %llu)\n",
                name, kind, r.sum.status, status, r.sum.nblocks, nblocks, (unsigned long long)r.sum.total_length,
                (unsigned long long)total, (unsigned long long)r.sum.objects, (unsigned long long)objects);
    ++failures;
  }
}

void long_cases() {
  struct {
    long long v;
    const char* hex;
  } known[] = {{0, "00"}, {-1, "01"}, {1, "02"}, {63, "7e"}, {64, "8001"}, {-64, "7f"}, {-65, "8101"},
               {2147483648ll, "8080808010"}, {4611686018427387904ll, "808080808080808080" "01"},
               {-4611686018427387904ll, "ffffffffffffffff7f"}};
  for (const auto& k : known) {
    S want;
    for (const char* p = k.hex; *p; p += 2) want += (char)std::strtol(S(p, 2).c_str(), nullptr, 16);
    expect(lng(k.v) == want, "the driver's own long writer");
    const uint32_t nb = sma::long_len(k.v);
    S got;
    for (uint32_t i = 0; i < nb; ++i) got += (char)sma::long_byte(k.v, i, nb);
    expect(got == want, "long_byte / long_len");
    sma::ByteFetch fetch{(const uint8_t*)want.data()};
    uint64_t pos = 0;
    int64_t v = 0;
    expect(sma::read_long(fetch, want.size(), pos, v) == SM_OK && v == k.v && pos == want.size(), "read_long");
    pos = 0;
    expect(sma::read_long(fetch, want.size() - 1, pos, v) == SMA_ERR_TRUNCATED, "read_long cut");
  }
  const S min64("\xff\xff\xff\xff\xff\xff\xff\xff\xff\x01", 10), over("\xff\xff\xff\xff\xff\xff\xff\xff\xff\x02", 10),
      more("\x80\x80\x80\x80\x80\x80\x80\x80\x80\x80\x00", 11);
  int64_t v = 0;
  uint64_t pos = 0;
  sma::ByteFetch f1{(const uint8_t*)min64.data()};
  expect(sma::read_long(f1, 10, pos, v) == SM_OK && v == INT64_MIN, "the least long");
  pos = 0;
  sma::ByteFetch f2{(const uint8_t*)over.data()};
  expect(sma::read_long(f2, 10, pos, v) == SMA_ERR_VARLONG, "a 10th byte above 1");
  pos = 0;
  sma::ByteFetch f3{(const uint8_t*)more.data()};
  expect(sma::read_long(f3, 11, pos, v) == SMA_ERR_VARLONG, "a 10th byte with the continuation bit");
}

void walk_cases() {
  const S h = header();
  const S abc = block(1, kAbc, kAbcCrc);
  status_case("empty stream", SMA_INPUT_FILE, "", SMA_ERR_NO_HEADER);
  status_case("wrong magic", SMA_INPUT_FILE, "Obk\x01", SMA_ERR_NO_HEADER);
  status_case("wrong first byte", SMA_INPUT_FILE, "X", SMA_ERR_NO_HEADER);
  status_case("cut magic", SMA_INPUT_FILE, "Ob", SMA_ERR_TRUNCATED);
  status_case("magic alone", SMA_INPUT_FILE, kMagic, SMA_ERR_TRUNCATED);
  status_case("header only", SMA_INPUT_FILE, h, SM_OK);
  status_case("one block", SMA_INPUT_FILE, h + abc, SM_OK, 1, 3, 1);
  status_case("two blocks", SMA_INPUT_FILE, h + abc + block(64, kAbc, 0), SM_OK, 2, 6, 65);
  status_case("null codec", SMA_INPUT_FILE, header("null") + abc, SMA_ERR_CODEC);
  status_case("deflate codec", SMA_INPUT_FILE, header("deflate"), SMA_ERR_CODEC);
  status_case("no codec", SMA_INPUT_FILE, kMagic + lng(1) + str("avro.schema") + str("\"bytes\"") + lng(0) + kSync, SMA_ERR_CODEC);
  status_case("codec before truncation", SMA_INPUT_FILE, header("null").substr(0, header("null").size() - 1), SMA_ERR_TRUNCATED);
  status_case("last codec wins", SMA_INPUT_FILE,
              kMagic + lng(2) + str("avro.codec") + str("null") + str("avro.codec") + str("snappy") + lng(0) + kSync + abc, SM_OK, 1, 3, 1);
  status_case("last codec loses", SMA_INPUT_FILE,
              kMagic + lng(1) + str("avro.codec") + str("snappy") + lng(1) + str("avro.codec") + str("null") + lng(0) + kSync,
              SMA_ERR_CODEC);
  status_case("negative map count", SMA_INPUT_FILE,
              kMagic + lng(-1) + lng(99) + str("avro.codec") + str("snappy") + lng(-1) + lng(0) + str("k") + str("") + lng(0) + kSync + abc,
              SM_OK, 1, 3, 1);
  status_case("map count that cannot be negated", SMA_INPUT_FILE, kMagic + S("\xff\xff\xff\xff\xff\xff\xff\xff\xff\x01", 10) + lng(1),
              SMA_ERR_BAD_HEADER);
  status_case("negative map byte size", SMA_INPUT_FILE, kMagic + lng(-1) + lng(-1), SMA_ERR_BAD_HEADER);
  status_case("negative key length", SMA_INPUT_FILE, kMagic + lng(1) + lng(-3), SMA_ERR_BAD_HEADER);
  status_case("negative value length", SMA_INPUT_FILE, kMagic + lng(1) + str("k") + lng(-3), SMA_ERR_BAD_HEADER);
  status_case("key past the end", SMA_INPUT_FILE, kMagic + lng(1) + lng(5) + "abcd", SMA_ERR_TRUNCATED);
  status_case("value past the end", SMA_INPUT_FILE, kMagic + lng(1) + str("k") + lng(1ll << 40), SMA_ERR_TRUNCATED);
  status_case("huge map count", SMA_INPUT_FILE, kMagic + lng(1ll << 62) + str("k") + str("v"), SMA_ERR_TRUNCATED);
  status_case("long of 11 bytes in the map", SMA_INPUT_FILE, kMagic + S("\x80\x80\x80\x80\x80\x80\x80\x80\x80\x80\x00", 11),
              SMA_ERR_VARLONG);
  status_case("cut marker", SMA_INPUT_FILE, h.substr(0, h.size() - 1), SMA_ERR_TRUNCATED);
  status_case("negative count", SMA_INPUT_FILE, h + abc + lng(-1) + lng(9), SMA_ERR_BLOCK, 1, 3, 1);
  status_case("negative size", SMA_INPUT_FILE, h + lng(1) + lng(-1), SMA_ERR_BLOCK);
  status_case("size 3", SMA_INPUT_FILE, h + lng(1) + lng(3) + "abc" + kSync, SMA_ERR_BLOCK);
  status_case("cut count", SMA_INPUT_FILE, h + S("\x80", 1), SMA_ERR_TRUNCATED);
  status_case("count alone", SMA_INPUT_FILE, h + lng(1), SMA_ERR_TRUNCATED);
  status_case("size past the end", SMA_INPUT_FILE, h + lng(1) + lng(10) + kAbc + be(0), SMA_ERR_TRUNCATED);
  status_case("cut sync", SMA_INPUT_FILE, (h + abc).substr(0, h.size() + abc.size() - 1), SMA_ERR_TRUNCATED);
  status_case("payload over 2 GiB", SMA_INPUT_FILE, h + lng(1) + lng(0x80000004ll), SMA_ERR_TRUNCATED);
  status_case("wrong sync", SMA_INPUT_FILE, h + block(1, kAbc, kAbcCrc, kOther), SMA_ERR_SYNC);
  status_case("sync outranks varint", SMA_INPUT_FILE, h + block(1, S("\xff\xff", 2), 0, kOther), SMA_ERR_SYNC);
  status_case("empty payload", SMA_INPUT_FILE, h + abc + block(0, "", 0), SM_ERR_VARINT, 1, 3, 1);
  status_case("cut varint", SMA_INPUT_FILE, h + block(1, S("\xff\xff", 2), 0), SM_ERR_VARINT);
  status_case("varint of 2^31", SMA_INPUT_FILE, h + block(1, S("\x80\x80\x80\x80\x08", 5), 0), SMA_ERR_TOO_LARGE);
  status_case("empty raw stream", SMA_INPUT_FILE, h + block(0, S("\x00", 1), 0), SM_OK, 1, 0, 0);
  status_case("saturating objects", SMA_INPUT_FILE, h + block(0x7fffffffffffffffll, kAbc, 0) + block(0x7fffffffffffffffll, kAbc, 0) + block(2, kAbc, 0),
              SM_OK, 3, 9, UINT64_MAX);
  // block runs: the caller's marker, no header
  status_case("empty run", SMA_INPUT_BLOCKS, "", SM_OK);
  status_case("run of two", SMA_INPUT_BLOCKS, abc + abc, SM_OK, 2, 6, 2);
  status_case("run with another marker", SMA_INPUT_BLOCKS, block(1, kAbc, kAbcCrc, kOther), SMA_ERR_SYNC);
  status_case("run that is a file", SMA_INPUT_BLOCKS, h + abc, SMA_ERR_BLOCK);  // ("O" reads as the count -40)
  // the fields of a recorded block
  const Result r = walk(h + abc + block(64, kAbc, 0xdeadbeefu), SMA_INPUT_FILE);
  expect(r.sum.header_length == h.size() && std::memcmp(r.sum.sync, kSync.data(), 16) == 0, "header length and marker");
  expect(r.pay_off[0] == h.size() + 2 && r.pay_len[0] == 5 && r.ulen[0] == 3 && r.count[0] == 1 && r.crc[0] == kAbcCrc && r.out_off[0] == 0,
         "first block's fields");
  expect(r.pay_off[1] == h.size() + abc.size() + 3 && r.count[1] == 64 && r.crc[1] == 0xdeadbeefu && r.out_off[1] == 3,
         "second block's fields");
  const Result few = walk(h + abc + abc, SMA_INPUT_FILE, 1);
  expect(few.sum.status == SM_BUFFER_TOO_SMALL && few.sum.nblocks == 2 && few.sum.total_length == 6, "one entry too few");
  // every truncation of a two-block file: never SM_OK but at the three whole prefixes, never a read past the cut
  const S whole = h + abc + abc;
  for (size_t n = 0; n < whole.size(); ++n) {
    const Result t = walk(whole.substr(0, n), SMA_INPUT_FILE);
    const bool at_edge = n == h.size() || n == h.size() + abc.size();
    expect((t.sum.status == SM_OK) == at_edge, "truncation");
    if (!at_edge && n >= 4) expect(t.sum.status == SMA_ERR_TRUNCATED, "a cut file is truncated");
  }
}

void streams_cases() {
  // all file cases back to back in one heap block
  S all;
  std::vector<uint64_t> off, len, cap;
  uint64_t want_blocks = 0;
  for (const Case& c : cases) {
    off.push_back(all.size());
    len.push_back(c.stream.size());
    cap.push_back(c.total);
    all += c.stream;
    if (c.status == SM_OK) want_blocks += c.nblocks;
  }
  const uint32_t k = (uint32_t)cases.size();
  uint8_t* heap = (uint8_t*)std::malloc(all.size());
  std::memcpy(heap, all.data(), all.size());
  std::vector<uint32_t> first(k + 1);
  std::vector<uint64_t> out_len(k), objects(k);
  std::vector<int32_t> status(k);
  uint64_t blocks = 0, frags = 0;
  sm_status rc = sma_streams_plan(heap, off.data(), len.data(), k, SMA_INPUT_FILE, nullptr, cap.data(), 0x7fffffffu, first.data(),
                                  out_len.data(), status.data(), objects.data(), &blocks, &frags);
  expect(rc == SM_OK && blocks == want_blocks && frags == want_blocks - 1, "plan totals");  // (one block declares 0 bytes)
  uint32_t at = 0;
  for (uint32_t r = 0; r < k; ++r) {
    expect(status[r] == cases[r].status && out_len[r] == cases[r].total && first[r] == at, "plan per stream");
    if (cases[r].status == SM_OK) at += cases[r].nblocks;
  }
  expect(first[k] == at, "plan scan end");
  rc = sma_streams_plan(heap, off.data(), len.data(), k, SMA_INPUT_FILE, nullptr, cap.data(), (uint32_t)want_blocks - 1, first.data(),
                        out_len.data(), status.data(), objects.data(), &blocks, &frags);
  expect(rc == SM_BUFFER_TOO_SMALL && blocks == want_blocks, "plan one slot short");
  for (uint32_t r = 0; r < k; ++r) expect(status[r] == SM_ERR_ARGUMENT && out_len[r] == 0 && objects[r] == 0, "plan over the bound");
  // a byte short gives the slots up
  for (uint32_t r = 0; r < k; ++r)
    if (cases[r].status == SM_OK && cases[r].total) cap[r] -= 1;
  rc = sma_streams_plan(heap, off.data(), len.data(), k, SMA_INPUT_FILE, nullptr, cap.data(), 0x7fffffffu, first.data(), out_len.data(),
                        status.data(), nullptr, &blocks, &frags);
  expect(rc == SM_OK && blocks == 1, "plan a byte short");  // (the block that declares 0 bytes still fits)
  for (uint32_t r = 0; r < k; ++r)
    if (cases[r].status == SM_OK && cases[r].total) expect(status[r] == SM_BUFFER_TOO_SMALL && out_len[r] == cases[r].total, "too small");
  std::free(heap);
  expect(sma_streams_plan(nullptr, nullptr, nullptr, 0, SMA_INPUT_FILE, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == SM_OK,
         "empty batch");
  expect(sma_streams_plan(nullptr, nullptr, nullptr, 0, 2, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == SM_ERR_ARGUMENT,
         "unknown kind");
}

void sync_cases() {
  // the marker at every position of a short buffer, at its very end, cut by the end, and twice
  for (size_t n : {16u, 17u, 40u, 100u}) {
    for (size_t at = 0; at + 16 <= n; ++at) {
      S buf(n, 'x');
      buf.replace(at, 16, kSync);
      uint8_t* heap = (uint8_t*)std::malloc(n);
      std::memcpy(heap, buf.data(), n);
      const uint64_t off = 0, len = n;
      const uint32_t q[3] = {0, 0, 0};
      const uint64_t from[3] = {0, at, at + 1};
      uint64_t pos[3];
      expect(sma_find_sync(heap, &off, &len, (const uint8_t*)kSync.data(), 1, q, from, 3, pos) == SM_OK, "find_sync runs");
      expect(pos[0] == at && pos[1] == at && pos[2] == n, "find_sync positions");
      std::free(heap);
    }
  }
  S two = S(5, 'y') + kSync.substr(0, 15) + "!" + kSync + "zz" + kSync;  // a 15-byte false start, then two
  uint8_t* heap = (uint8_t*)std::malloc(two.size());
  std::memcpy(heap, two.data(), two.size());
  const uint64_t off = 0, len = two.size(), from[3] = {0, 22, 100};
  const uint32_t q[3] = {0, 0, 0};
  uint64_t pos[3];
  sma_find_sync(heap, &off, &len, (const uint8_t*)kSync.data(), 1, q, from, 3, pos);
  expect(pos[0] == 21 && pos[1] == 39 && pos[2] == two.size(), "find_sync: false start, the first wins, from behind the end");
  std::free(heap);
  uint64_t none;
  const uint64_t zero = 0;
  expect(sma_find_sync(nullptr, &zero, &zero, (const uint8_t*)kSync.data(), 1, q, &zero, 1, &none) == SM_OK && none == 0, "empty stream");
  // marker_at at every byte shift
  uint64_t w[4];
  for (uint32_t k = 0; k < 16; ++k) {
    uint8_t bytes[32];
    std::memset(bytes, 0x55, 32);
    std::memcpy(bytes + k, kSync.data(), 16);
    std::memcpy(w, bytes, 32);
    const sma::Marker m = sma::load_marker((const uint8_t*)kSync.data());
    for (uint32_t j = 0; j < 16; ++j) expect(sma::marker_at(w, j, m) == (j == k), "marker_at");
  }
}

void header_cases() {
  const S schema = "\"bytes\"";
  const S want = kMagic + lng(2) + str("avro.schema") + str(schema) + str("avro.codec") + str("snappy") + lng(0) + kSync;
  size_t n = 0;
  expect(sma_write_header((const uint8_t*)schema.data(), schema.size(), nullptr, nullptr, 0, (const uint8_t*)kSync.data(), nullptr, 0, &n) == SM_OK &&
             n == want.size(),
         "header size");
  uint8_t* heap = (uint8_t*)std::malloc(n);
  expect(sma_write_header((const uint8_t*)schema.data(), schema.size(), nullptr, nullptr, 0, (const uint8_t*)kSync.data(), heap, n, &n) == SM_OK &&
             std::memcmp(heap, want.data(), n) == 0,
         "header bytes");
  for (size_t cap = 0; cap < n; ++cap) {
    uint8_t* small = (uint8_t*)std::malloc(cap ? cap : 1);
    size_t got = 0;
    expect(sma_write_header((const uint8_t*)schema.data(), schema.size(), nullptr, nullptr, 0, (const uint8_t*)kSync.data(), small, cap, &got) ==
                   SM_BUFFER_TOO_SMALL &&
               got == n,
           "header too small");
    std::free(small);
  }
  sma_summary s;
  expect(sma_index(heap, n, SMA_INPUT_FILE, nullptr, nullptr, 0, &s) == SM_OK && s.header_length == n, "the written header walks");
  std::free(heap);
  const S extra = S("k1") + "value" + "" + "v";
  const uint64_t eoff[5] = {0, 2, 7, 7, 8};
  const S want2 = kMagic + lng(4) + str("avro.schema") + str(schema) + str("avro.codec") + str("snappy") + str("k1") + str("value") + str("") +
                  str("v") + lng(0) + kSync;
  std::vector<uint8_t> out(want2.size());
  expect(sma_write_header((const uint8_t*)schema.data(), schema.size(), (const uint8_t*)extra.data(), eoff, 2, (const uint8_t*)kSync.data(),
                          out.data(), out.size(), &n) == SM_OK &&
             n == want2.size() && std::memcmp(out.data(), want2.data(), n) == 0,
         "header with extra pairs");
}

void size_cases() {
  expect(sma_max_blocks(0) == 0 && sma_max_blocks(22) == 0 && sma_max_blocks(23) == 1 && sma_max_blocks(46) == 2, "max_blocks");
  expect(block(0, S("\x00", 1), 0).size() == 23, "the shortest block");
  expect(sma_max_block_length(0) == 72 && sma_max_block_length(65536) == 32 + 65536 + 10922 + 40, "max_block_length");
  expect(sma_stage_length(0) == 32 && sma_stage_length(1) == 48 && sma_stage_length(65536) == 76496, "stage_length");
  expect(sma::block_bytes(1, 5) == 1 + 1 + 5 + 4 + 16 && sma::block_bytes(64, 60) == 2 + 2 + 60 + 4 + 16, "block_bytes");
  expect(sma::slot_verdict(SM_OK, true, 1, 2) == SMA_ERR_CRC && sma::slot_verdict(SM_OK, false, 1, 2) == SM_OK &&
             sma::slot_verdict(17, true, 1, 2) == 17 && sma::slot_verdict(SM_OK, true, 7, 7) == SM_OK,
         "slot_verdict");
  expect(sma_streams_scratch_bytes(3, 7, 0, 0) > sma_streams_scratch_bytes(3, 6, 0, 0) &&
             sma_streams_scratch_bytes(1, 1, 0, 1 << 20) > (1u << 20),
         "scratch bytes");
  for (int st = 80; st <= 88; ++st) expect(sma::host_message((sm_status)st) != nullptr, "status text");
  expect(sma::host_message((sm_status)79) == nullptr && sma::host_message((sm_status)89) == nullptr, "no text outside");
}

}  // namespace

int main() {
  long_cases();
  walk_cases();
  streams_cases();
  sync_cases();
  header_cases();
  size_cases();
  if (failures) {
    std::printf("sma_host_check: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("sma_host_check ok\n");
  return 0;
}
