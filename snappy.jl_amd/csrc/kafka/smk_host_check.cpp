// smk_host_check.cpp -- the sanitizer driver of the Kafka segment library's host-only part
// (smk_host.cpp and the rules of smk_format.h, with the blocks and framing libraries' host-only
// files they call into): the walk, the heads, the two plans and the batch writer, on inputs whose
// expected results are written out here, then on the fixtures of tests/golden/kafka/ and a few
// thousand seeded mutations of them.  Built with -fsanitize=address,undefined by `make host_check`;
// CPU only.  Every buffer is a heap block of the exact length, so a read past an input's end is
// reported.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../../include/snappy_mi355x_framing.h"
#include "smk_format.h"

static int failures = 0;
#define EXPECT(x)                                             \
  do {                                                        \
    if (!(x)) {                                               \
      printf("FAILED line %d: %s\n", __LINE__, #x);           \
      ++failures;                                             \
    }                                                         \
  } while (0)

typedef std::vector<uint8_t> Bytes;

// an exact-length heap copy: the sanitizer sees any read past the end
struct Exact {
  uint8_t* p;
  size_t n;
  explicit Exact(const Bytes& b) : p(b.empty() ? nullptr : (uint8_t*)malloc(b.size())), n(b.size()) {
    if (n) memcpy(p, b.data(), n);
  }
  ~Exact() { free(p); }
};

static void put_be(Bytes& b, uint64_t v, int bytes) {
  for (int i = bytes - 1; i >= 0; --i) b.push_back((uint8_t)(v >> (8 * i)));
}

// a batch by hand: the crc is left zero (the walk and the heads do not read it)
static Bytes batch(uint32_t codec, const Bytes& payload, uint32_t attributes = 0, uint32_t magic = 2) {
  Bytes b;
  put_be(b, 7, 8);
  put_be(b, 49 + payload.size(), 4);
  put_be(b, 0, 4);
  b.push_back((uint8_t)magic);
  put_be(b, 0, 4);
  put_be(b, attributes | codec, 2);
  b.resize(61, 0x5a);
  b.insert(b.end(), payload.begin(), payload.end());
  return b;
}

// a raw Snappy stream of one literal (n < 61)
static Bytes raw_literal(const Bytes& text) {
  Bytes b;
  b.push_back((uint8_t)text.size());
  if (!text.empty()) {
    b.push_back((uint8_t)((text.size() - 1) << 2));
    b.insert(b.end(), text.begin(), text.end());
  }
  return b;
}

static const uint8_t kXerialHeader[16] = {0x82, 'S', 'N', 'A', 'P', 'P', 'Y', 0, 0, 0, 0, 1, 0, 0, 0, 1};

static Bytes xerial(const std::vector<Bytes>& chunks) {
  Bytes b(kXerialHeader, kXerialHeader + 16);
  for (const Bytes& c : chunks) {
    put_be(b, c.size(), 4);
    b.insert(b.end(), c.begin(), c.end());
  }
  return b;
}

static Bytes cat(const std::vector<Bytes>& parts) {
  Bytes b;
  for (const Bytes& p : parts) b.insert(b.end(), p.begin(), p.end());
  return b;
}

struct Index {
  std::vector<uint64_t> pos, declared;
  std::vector<uint32_t> length, codec;
  std::vector<int32_t> status;
  smk_summary s;
  sm_status st;
};

static Index index_of(const Bytes& seg, uint32_t max = 64) {
  Index r;
  r.pos.resize(max + 1);
  r.declared.resize(max + 1);
  r.length.resize(max + 1);
  r.codec.resize(max + 1);
  r.status.resize(max + 1);
  Exact e(seg);
  r.st = smk_index(e.p, e.n, r.pos.data(), r.length.data(), r.codec.data(), r.declared.data(), r.status.data(), max, &r.s);
  return r;
}

static void check_walk() {
  const Bytes abc = {'a', 'b', 'c'};
  Index r = index_of(Bytes());
  EXPECT(r.st == SM_OK && r.s.nbatches == 0 && r.s.valid_length == 0 && r.s.total_length == 0);
  const Bytes one = batch(0, abc);
  EXPECT(one.size() == 64);
  r = index_of(one);
  EXPECT(r.st == SM_OK && r.s.nbatches == 1 && r.s.valid_length == 64 && r.s.total_length == 64);
  EXPECT(r.pos[0] == 0 && r.length[0] == 52 && r.codec[0] == 0 && r.declared[0] == 3 && r.status[0] == SM_OK);
  // every cut of two batches: whole batches, then SMK_ERR_TRUNCATED, never a read past the end
  const Bytes two = cat({one, batch(2, raw_literal(abc), 0x10)});
  for (size_t cut = 0; cut <= two.size(); ++cut) {
    r = index_of(Bytes(two.begin(), two.begin() + cut));
    const uint32_t whole = cut == two.size() ? 2 : cut >= 64 ? 1 : 0;
    EXPECT(r.s.nbatches == whole && r.s.valid_length == (whole == 2 ? two.size() : whole * 64));
    EXPECT(r.st == (cut == 0 || cut == 64 || cut == two.size() ? (sm_status)SM_OK : (sm_status)SMK_ERR_TRUNCATED));
  }
  r = index_of(two);
  EXPECT(r.codec[1] == 2 && r.declared[1] == 3 && r.s.total_length == 128 && r.pos[1] == 64);
  EXPECT(index_of(two, 1).st == SM_BUFFER_TOO_SMALL);
  for (uint32_t magic : {0u, 1u, 3u}) EXPECT(index_of(cat({one, batch(0, abc, 0, magic)})).st == SMK_ERR_MAGIC);
  for (uint32_t codec : {1u, 3u, 4u, 5u, 6u, 7u}) {
    r = index_of(cat({one, batch(codec, abc)}));
    EXPECT(r.st == SMK_ERR_CODEC && r.s.nbatches == 1 && r.s.valid_length == 64);
  }
  EXPECT(index_of(batch(0, abc, 0xfff8)).st == SM_OK);  // every other attribute bit is the caller's
  {
    Bytes b = batch(0, Bytes());
    EXPECT(index_of(b).st == SM_OK);
    b[11] = 48;
    EXPECT(index_of(b).st == SMK_ERR_LENGTH);
    b[11] = 50;
    EXPECT(index_of(b).st == SMK_ERR_TRUNCATED);
    b[8] = 0x80;
    b[11] = 0;
    EXPECT(index_of(b).st == SMK_ERR_LENGTH);  // negative as an int32
    b[8] = 0x7f;
    EXPECT(index_of(b).st == SMK_ERR_TRUNCATED);
    Bytes c(b.begin(), b.begin() + 17);  // the first 17 bytes alone: the magic is judged, then the length
    c[8] = 0;
    c[11] = 49;
    EXPECT(index_of(c).st == SMK_ERR_TRUNCATED);
    c[16] = 1;
    EXPECT(index_of(c).st == SMK_ERR_MAGIC);
    EXPECT(index_of(Bytes(c.begin(), c.begin() + 16)).st == SMK_ERR_TRUNCATED);
  }
}

static void check_heads() {
  const Bytes abc = {'a', 'b', 'c'}, de = {'d', 'e'};
  Index r = index_of(batch(2, Bytes()));
  EXPECT(r.st == SM_OK && r.declared[0] == 0 && r.s.total_length == 61);
  r = index_of(batch(2, xerial({raw_literal(abc), raw_literal(de)})));
  EXPECT(r.st == SM_OK && r.declared[0] == 5 && r.status[0] == SM_OK);
  r = index_of(batch(2, xerial({})));
  EXPECT(r.st == SM_OK && r.declared[0] == 0);
  {  // the magic alone is a snappy-java stream without the rest of its header; seven bytes of it are a raw stream
    Bytes m(kXerialHeader, kXerialHeader + 8);
    r = index_of(batch(2, m));
    EXPECT(r.st == SMB_ERR_TRUNCATED && r.status[0] == SMB_ERR_TRUNCATED && r.s.nbatches == 1 && r.s.total_length == 0);
    m.pop_back();
    r = index_of(batch(2, m));
    EXPECT(r.st == SM_OK && r.declared[0] == 10626);  // 82 53 as a varint
  }
  {
    Bytes x = xerial({raw_literal(abc)});
    x[11] = 0;  // version 0
    EXPECT(index_of(batch(2, x)).st == SMB_ERR_BAD_HEADER);
    x[11] = 1;
    x[19] = 9;  // a chunk longer than the payload
    EXPECT(index_of(batch(2, x)).st == SMB_ERR_TRUNCATED);
  }
  EXPECT(index_of(batch(2, Bytes{0x80})).st == SM_ERR_VARINT);
  EXPECT(index_of(batch(2, Bytes{0xff, 0xff, 0xff, 0xff, 0x10})).st == SM_ERR_VARINT);
  EXPECT(index_of(batch(2, Bytes{0xce, 0xff, 0xff, 0xff, 0x07})).st == SM_OK);            // 0x7fffffff - 49
  EXPECT(index_of(batch(2, Bytes{0xcf, 0xff, 0xff, 0xff, 0x07})).st == SMK_ERR_TOO_LARGE);  // one more
  // a failing head: the lengths before it; the walk goes on behind it
  r = index_of(cat({batch(0, abc), batch(2, Bytes{0x80}), batch(0, de)}));
  EXPECT(r.st == SM_ERR_VARINT && r.s.nbatches == 3 && r.s.total_length == 64 && r.status[1] == SM_ERR_VARINT && r.status[2] == SM_OK);
  // the walk's error outranks a failing head in front of it
  r = index_of(cat({batch(2, Bytes{0x80}), batch(1, de)}));
  EXPECT(r.st == SMK_ERR_CODEC && r.s.nbatches == 1 && r.s.total_length == 0);
}

static void check_plans() {
  const Bytes abc = {'a', 'b', 'c'};
  const Bytes x = batch(2, xerial({raw_literal(abc), raw_literal(abc)}));
  const Bytes segs = cat({batch(0, abc), x, batch(2, raw_literal(abc)), batch(2, xerial({raw_literal(Bytes())})), batch(1, abc)});
  const uint64_t good = 64 + x.size() + 66 + 61 + 16 + 4 + 1;
  Exact e(segs);
  const uint64_t off[3] = {0, good, 0}, len[3] = {good, segs.size() - good, 64};
  uint32_t first[4];
  uint64_t out_len[3], batches, chunks, fragments;
  int32_t status[3];
  EXPECT(smk_segments_plan(e.p, off, len, 3, nullptr, 6, 3, first, out_len, status, &batches, &chunks, &fragments) == SM_OK);
  EXPECT(status[0] == SM_OK && status[1] == SMK_ERR_CODEC && status[2] == SM_OK && batches == 5 && chunks == 3 && fragments == 2);
  EXPECT(out_len[0] == 64 + 67 + 64 + 61 && out_len[1] == 0 && out_len[2] == 64 && first[0] == 0 && first[1] == 4 && first[3] == 5);
  EXPECT(smk_segments_plan(e.p, off, len, 3, nullptr, 4, 3, first, out_len, status, nullptr, nullptr, nullptr) == SM_BUFFER_TOO_SMALL);
  EXPECT(status[0] == SM_ERR_ARGUMENT && status[2] == SM_ERR_ARGUMENT && out_len[0] == 0);
  EXPECT(smk_segments_plan(e.p, off, len, 3, nullptr, 5, 2, first, out_len, status, nullptr, nullptr, nullptr) == SM_BUFFER_TOO_SMALL);
  const uint64_t cap[3] = {0, 0, 63};
  EXPECT(smk_segments_plan(e.p, off, len, 3, cap, 5, 1, first, out_len, status, &batches, &chunks, &fragments) == SM_OK);
  // (no room: the snappy-java stream of no bytes still takes its chunk's slot in the sizing call)
  EXPECT(status[0] == SM_BUFFER_TOO_SMALL && status[2] == SM_BUFFER_TOO_SMALL && out_len[2] == 64 && chunks == 1 && fragments == 0);
  uint64_t room[3], blocks, stage;
  EXPECT(smk_compress_plan(e.p, off, len, 3, 5, first, room, status, &batches, &blocks, &stage) == SM_OK);
  EXPECT(status[0] == SM_OK && status[1] == SMK_ERR_CODEC && batches == 5 && blocks == 2 && stage == 2 * 64);
  EXPECT(room[2] == 64 + 10 + 52 && smk_max_segment_length(64, 1) == room[2]);
  EXPECT(smk_compress_plan(e.p, off, len, 3, 4, first, room, status, &batches, &blocks, &stage) == SM_BUFFER_TOO_SMALL);
  EXPECT(status[1] == SM_ERR_ARGUMENT);
  // the stage is the blocks library's bound, and a segment's room holds every batch's
  for (uint64_t n : {0ull, 1ull, 3ull, 65535ull, 65536ull, 65537ull, 131072ull, 1000000ull}) {
    EXPECT(smk::xerial_max_length(n) == smb_max_length(n, SMB_FORMAT_XERIAL));
    EXPECT(smk_stage_length(n) == (n ? (smb_max_length(n, SMB_FORMAT_XERIAL) + 15) / 16 * 16 : 0));
    EXPECT(61 + smb_max_length(n, SMB_FORMAT_XERIAL) <= smk_max_segment_length(61 + n, 1));
  }
  EXPECT(smk_segments_scratch_bytes(1, 1, 0, 1 << 20) > (1 << 20) && smk_segments_scratch_bytes(0, 0, 0, 0) > 0);
  EXPECT(smk_segments_scratch_bytes(3, 7, 0, 0) > smk_segments_scratch_bytes(3, 6, 0, 0));
}

static void check_writer() {
  // by hand: offset 0x0102030405060708, epoch 9, a control batch (bit 5), the 38 bytes 00 .. 25, records "abc"
  uint8_t tail[38];
  for (int i = 0; i < 38; ++i) tail[i] = (uint8_t)i;
  const uint8_t rec[3] = {'a', 'b', 'c'};
  size_t n = 0;
  EXPECT(smk_write_batch(0x0102030405060708ull, 9, 0x20, tail, rec, 3, nullptr, 0, &n) == SM_OK && n == 64);
  Bytes out(64);
  EXPECT(smk_write_batch(0x0102030405060708ull, 9, 0x20, tail, rec, 3, out.data(), 63, &n) == SM_BUFFER_TOO_SMALL);
  EXPECT(smk_write_batch(0x0102030405060708ull, 9, 0x22, tail, rec, 3, out.data(), 64, &n) == SM_ERR_ARGUMENT);
  EXPECT(smk_write_batch(0x0102030405060708ull, 9, 0x20, tail, rec, 3, out.data(), 64, &n) == SM_OK);
  const uint8_t head[17] = {1, 2, 3, 4, 5, 6, 7, 8, 0, 0, 0, 52, 0, 0, 0, 9, 2};
  EXPECT(memcmp(out.data(), head, 17) == 0 && out[21] == 0 && out[22] == 0x20 && memcmp(out.data() + 23, tail, 38) == 0);
  EXPECT(memcmp(out.data() + 61, rec, 3) == 0);
  const uint32_t c = smf_crc32c(out.data() + 21, 43);
  EXPECT(out[17] == (uint8_t)(c >> 24) && out[18] == (uint8_t)(c >> 16) && out[19] == (uint8_t)(c >> 8) && out[20] == (uint8_t)c);
  EXPECT(smf_crc32c("123456789", 9) == 0xe3069283u);  // the check value of CRC-32C
  Index r = index_of(out);
  EXPECT(r.st == SM_OK && r.declared[0] == 3);
  // the rewritten header: the length and the codec bits change, the crc reads as zero, the rest stays
  for (uint32_t i = 0; i < 61; ++i) {
    const uint8_t b = smk::header_byte([&](uint32_t k) { return (uint32_t)out[k]; }, i, 0x01020304u, 2);
    const uint8_t want = i >= 8 && i < 12 ? (uint8_t)(i - 7) : i >= 17 && i < 21 ? 0 : i == 22 ? 0x22 : out[i];
    EXPECT(b == want);
  }
}

// the fixtures, and seeded mutations of them: whatever the bytes, the walk stays inside them and its
// summary is consistent
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rng() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(rng_state >> 33);
}

static bool read_file(const std::string& path, Bytes& out) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return false;
  out.clear();
  uint8_t buf[65536];
  size_t k;
  while ((k = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + k);
  fclose(f);
  return true;
}

static void consistent(const Bytes& seg) {
  Exact e(seg);
  smk_summary s;
  const sm_status st = smk_index(e.p, e.n, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &s);
  EXPECT(st == s.status && s.valid_length <= seg.size() && s.valid_length >= 61ull * s.nbatches);
  EXPECT(st != SM_OK || s.valid_length == seg.size());
  const uint64_t off = 0, len = seg.size();
  uint64_t out_len, batches, chunks, fragments, room, blocks, stage;
  int32_t status, cstatus;
  EXPECT(smk_segments_plan(e.p, &off, &len, 1, nullptr, 0x7fffffff, 0x7fffffff, nullptr, &out_len, &status, &batches, &chunks, &fragments) == SM_OK);
  EXPECT(status == st && batches == s.nbatches && out_len == s.total_length);
  EXPECT(smk_compress_plan(e.p, &off, &len, 1, 0x7fffffff, nullptr, &room, &cstatus, &batches, &blocks, &stage) == SM_OK);
  EXPECT(batches == s.nbatches && (cstatus == SM_OK) == (s.valid_length == seg.size()));
}

static void check_fixtures() {
  const char* names[] = {"mixed.log", "bigbatch.log", "small_batches.log", "empty.log"};
  const uint32_t want[] = {9, 2, 300, 0};
  for (int f = 0; f < 4; ++f) {
    Bytes seg;
    if (!read_file(std::string("../../../tests/golden/kafka/") + names[f], seg)) {
      printf("FAILED: fixture %s not found\n", names[f]);
      ++failures;
      continue;
    }
    Index r = index_of(seg, 512);
    EXPECT(r.st == SM_OK && r.s.nbatches == want[f] && r.s.valid_length == seg.size());
    consistent(seg);
    if (seg.empty()) continue;
    const int rounds = seg.size() > 100000 ? 300 : 1500;
    for (int k = 0; k < rounds; ++k) {
      Bytes m = seg;
      const uint32_t kind = rng() % 4;
      if (kind == 0) m.resize(rng() % m.size());
      else if (kind == 1) m[rng() % m.size()] ^= (uint8_t)(1u << (rng() % 8));
      else if (kind == 2) {  // a header field of some batch
        const uint32_t j = rng() % r.s.nbatches;
        m[r.pos[j] + rng() % 80 % (12 + r.length[j])] = (uint8_t)rng();
      } else {  // the first bytes of some payload
        const uint32_t j = rng() % r.s.nbatches;
        if (r.length[j] > 49) m[r.pos[j] + 61 + rng() % 24 % (r.length[j] - 49)] = (uint8_t)rng();
      }
      consistent(m);
    }
  }
}

int main() {
  check_walk();
  check_heads();
  check_plans();
  check_writer();
  check_fixtures();
  if (failures) {
    printf("smk_host_check: %d failures\n", failures);
    return 1;
  }
  printf("smk_host_check ok\n");
  return 0;
}
