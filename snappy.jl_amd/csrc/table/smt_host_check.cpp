// smt_host_check.cpp -- the sanitizer driver of the table library's host-only part (smt_host.cpp
// and the rules of smt_format.h): the footer, the index walk, a block's head and the tail writer,
// on inputs whose expected results are written out here.  Built with -fsanitize=address,undefined
// by `make host_check`; CPU only.  Every buffer is a heap block of the exact length, so a read past
// an input's end is reported.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "smt_format.h"

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

static void put_varint(Bytes& b, uint64_t v) {
  while (v >= 128) {
    b.push_back((uint8_t)(v | 128));
    v >>= 7;
  }
  b.push_back((uint8_t)v);
}

static const uint8_t kMagicBytes[8] = {0x57, 0xfb, 0x80, 0x8b, 0x24, 0x75, 0x47, 0xdb};

// `body` bytes of blocks, then a footer with the two handles
static Bytes table_with(size_t body, uint64_t moff, uint64_t msize, uint64_t ioff, uint64_t isize) {
  Bytes b(body, 0);
  Bytes foot;
  put_varint(foot, moff);
  put_varint(foot, msize);
  put_varint(foot, ioff);
  put_varint(foot, isize);
  foot.resize(40, 0);
  b.insert(b.end(), foot.begin(), foot.end());
  b.insert(b.end(), kMagicBytes, kMagicBytes + 8);
  return b;
}

static sm_status footer_of(const Bytes& b, uint64_t* v) {
  Exact e(b);
  return smt_footer(e.p, e.n, &v[0], &v[1], &v[2], &v[3]);
}

static void check_footer() {
  uint64_t v[4];
  EXPECT(footer_of(Bytes(), v) == SMT_ERR_TRUNCATED);
  EXPECT(footer_of(Bytes(47, 0), v) == SMT_ERR_TRUNCATED);
  EXPECT(footer_of(Bytes(48, 0), v) == SMT_ERR_MAGIC);
  Bytes ok = table_with(26, 0, 8, 13, 8);
  EXPECT(footer_of(ok, v) == SM_OK && v[0] == 0 && v[1] == 8 && v[2] == 13 && v[3] == 8);
  for (int i = 0; i < 8; ++i) {
    Bytes bad = ok;
    bad[bad.size() - 8 + i] ^= 1;
    EXPECT(footer_of(bad, v) == SMT_ERR_MAGIC);
  }
  EXPECT(footer_of(table_with(26, 0, 8, 13, 9), v) == SMT_ERR_HANDLE);  // ends a byte behind n - 48
  EXPECT(footer_of(table_with(26, 22, 0, 13, 8), v) == SMT_ERR_HANDLE);
  EXPECT(footer_of(table_with(26, 0, 8, ~0ull, 8), v) == SMT_ERR_HANDLE);  // off + size overflows
  EXPECT(footer_of(table_with(26, 0, 8, 8, ~0ull), v) == SMT_ERR_HANDLE);
  {  // a 10-byte varint64 (2^63), then one whose tenth byte is 2
    Bytes b = ok;
    uint8_t* f = b.data() + 26;
    memset(f, 0x80, 9);
    f[9] = 1;
    memset(f + 10, 0, 30);
    EXPECT(footer_of(b, v) == SMT_ERR_HANDLE && v[0] == 1ull << 63);
    f[9] = 2;
    EXPECT(footer_of(b, v) == SMT_ERR_FOOTER);
    memset(f, 0x80, 40);  // a varint that leaves the 40 bytes
    EXPECT(footer_of(b, v) == SMT_ERR_FOOTER);
  }
  uint64_t ib = 0;
  {
    Exact e(ok);
    EXPECT(smt_index_bound(e.p, e.n, &ib) == SM_OK && ib == 8);  // type 0: the size
    Bytes t = ok;
    t[13 + 8] = 2;
    Exact e2(t);
    EXPECT(smt_index_bound(e2.p, e2.n, &ib) == SMT_ERR_TYPE);
    t[13 + 8] = 1;
    t[13] = 0xac;
    t[14] = 0x02;  // varint 300
    Exact e3(t);
    EXPECT(smt_index_bound(e3.p, e3.n, &ib) == SM_OK && ib == 300);
    memset(t.data() + 13, 0xff, 5);
    Exact e4(t);
    EXPECT(smt_index_bound(e4.p, e4.n, &ib) == SM_ERR_VARINT);
  }
}

// index contents: entries, then the restart array of r zeros and r
static Bytes index_of(const Bytes& entries, uint32_t r) {
  Bytes b = entries;
  for (uint32_t i = 0; i <= r; ++i) {
    const uint32_t v = i == r ? r : 0;
    for (int k = 0; k < 4; ++k) b.push_back((uint8_t)(v >> (8 * k)));
  }
  return b;
}

static void put_entry(Bytes& b, uint32_t shared, size_t klen, uint64_t off, uint64_t size, size_t trailing = 0) {
  Bytes h;
  put_varint(h, off);
  put_varint(h, size);
  h.resize(h.size() + trailing, 0xee);
  put_varint(b, shared);
  put_varint(b, klen);
  put_varint(b, h.size());
  b.resize(b.size() + klen, 'k');
  b.insert(b.end(), h.begin(), h.end());
}

static sm_status walk(const Bytes& c, uint64_t n, smt_summary* s, uint64_t* off = nullptr, uint64_t* size = nullptr, uint32_t max = 0) {
  Exact e(c);
  return smt_walk_index(e.p, e.n, n, off, size, max, s);
}

static void check_index() {
  smt_summary s;
  const uint64_t n = 1000 + 48;
  EXPECT(walk(Bytes(3, 0), n, &s) == SMT_ERR_INDEX);
  EXPECT(walk(Bytes(4, 0), n, &s) == SM_OK && s.nblocks == 0);
  EXPECT(walk(index_of(Bytes(), 1), n, &s) == SM_OK && s.nblocks == 0);
  {
    Bytes b(8, 0);
    b[4] = 2;  // r one over (m - 4) / 4
    EXPECT(walk(b, n, &s) == SMT_ERR_INDEX);
  }
  const size_t klens[] = {0, 1, 63, 64, 65, 300};
  for (size_t klen : klens) {
    Bytes e;
    put_entry(e, 0, klen, 10, 20);
    put_entry(e, (uint32_t)klen, 2, 35, 40, 3);  // shares the whole previous key; trailing bytes in the value
    put_entry(e, (uint32_t)klen + 2, 0, 995, 0);  // ends exactly at n - 48
    uint64_t off[3], size[3];
    EXPECT(walk(index_of(e, 3), n, &s, off, size, 3) == SM_OK && s.nblocks == 3 && s.total_length == 60);
    EXPECT(off[0] == 10 && size[0] == 20 && off[1] == 35 && size[1] == 40 && off[2] == 995 && size[2] == 0);
    EXPECT(walk(index_of(e, 3), n, &s, off, size, 2) == SM_BUFFER_TOO_SMALL && s.nblocks == 3);
    // every cut of the entries is an error or fewer entries, never a read past the end
    for (size_t cut = 0; cut < e.size(); ++cut) {
      Bytes c(e.begin(), e.begin() + cut);
      const sm_status st = walk(index_of(c, 1), n, &s);
      EXPECT(st == SMT_ERR_INDEX || (st == SM_OK && s.nblocks < 3));
    }
    Bytes over;
    put_entry(over, 0, klen, 10, 20);
    put_entry(over, (uint32_t)klen + 1, 2, 35, 40);  // shared one over the previous key's length
    EXPECT(walk(index_of(over, 1), n, &s) == SMT_ERR_INDEX && s.nblocks == 1);
  }
  {
    Bytes e;
    put_entry(e, 0, 4, 996, 0);  // a byte behind n - 48
    EXPECT(walk(index_of(e, 1), n, &s) == SMT_ERR_HANDLE && s.nblocks == 0);
    Bytes one;  // a value holding one varint only
    put_varint(one, 0);
    put_varint(one, 1);
    put_varint(one, 1);
    one.push_back('k');
    one.push_back(5);
    EXPECT(walk(index_of(one, 1), n, &s) == SMT_ERR_INDEX);
    Bytes big;
    put_entry(big, 0, 1, 0, 0x7fffffffull);
    EXPECT(walk(index_of(big, 1), 0x100000000ull, &s) == SMT_ERR_TOO_LARGE);
    Bytes five;  // a varint32 whose fifth byte is 0x10
    const uint8_t v5[5] = {0x80, 0x80, 0x80, 0x80, 0x10};
    five.insert(five.end(), v5, v5 + 5);
    five.resize(12, 0);
    EXPECT(walk(index_of(five, 1), n, &s) == SMT_ERR_INDEX);
  }
}

static void check_head() {
  uint32_t type;
  uint64_t d;
  Bytes b = {0x03, 0x08, 'a', 'b', 'c', 1, 0, 0, 0, 0, 0};
  Exact e(b);
  EXPECT(smt_block_head(e.p, e.n, 0, 5, &type, &d) == SM_OK && type == 1 && d == 3);
  EXPECT(smt_block_head(e.p, e.n, 0, 7, &type, &d) == SMT_ERR_HANDLE);
  EXPECT(smt_block_head(e.p, e.n, 6, 5, &type, &d) == SMT_ERR_HANDLE);
  EXPECT(smt_block_head(e.p, e.n, 5, 0, &type, &d) == SM_ERR_VARINT);  // type 1 with no contents
  EXPECT(smt_block_head(e.p, e.n, 1, 4, &type, &d) == SM_OK && type == 1 && d == 8);
  EXPECT(smt_block_head(e.p, e.n, 0, 2, &type, &d) == SMT_ERR_TYPE && type == 'a');
  EXPECT(smt_block_head(e.p, e.n, 1, 5, &type, &d) == SM_OK && type == 0 && d == 5);
  Bytes big = {0xff, 0xff, 0xff, 0xff, 0x08, 1, 0, 0, 0, 0};
  Exact e2(big);
  EXPECT(smt_block_head(e2.p, e2.n, 0, 5, &type, &d) == SMT_ERR_TOO_LARGE);
  EXPECT(smt_max_blocks(4) == 0 && smt_max_blocks(5) == 1 && smt_max_blocks(157108) == 31421);
  EXPECT(smt_max_block_length(0) == 5 && smt_max_block_length(4096) == 4101 && smt_stage_length(65536) == 76496);
  EXPECT(smt_tables_scratch_bytes(1, 1, 0, 0, 1 << 20) > (1 << 20) && smt_tables_scratch_bytes(0, 0, 0, 0, 0) > 0);
  EXPECT(smt_tables_scratch_bytes(3, 7, 100, 0, 0) > smt_tables_scratch_bytes(3, 6, 100, 0, 0));
}

static void check_tail() {
  // the empty table, byte for byte: the metaindex block, an index block alike, the footer
  size_t len = 0;
  EXPECT(smt_write_tail(nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, &len) == SM_OK && len == 74);
  Bytes out(74);
  EXPECT(smt_write_tail(nullptr, nullptr, 0, nullptr, nullptr, 0, out.data(), 73, &len) == SM_BUFFER_TOO_SMALL);
  EXPECT(smt_write_tail(nullptr, nullptr, 0, nullptr, nullptr, 0, out.data(), 74, &len) == SM_OK);
  const uint8_t block[13] = {0, 0, 0, 0, 1, 0, 0, 0, 0, 0xc0, 0xf2, 0xa1, 0xb0};  // (the masked CRC-32C of those nine bytes)
  EXPECT(memcmp(out.data(), block, 13) == 0 && memcmp(out.data() + 13, block, 13) == 0);
  const uint8_t foot[4] = {0, 8, 13, 8};
  EXPECT(memcmp(out.data() + 26, foot, 4) == 0 && memcmp(out.data() + 66, kMagicBytes, 8) == 0);
  uint64_t v[4];
  EXPECT(footer_of(out, v) == SM_OK && v[2] == 13 && v[3] == 8);
  // three blocks under keys of 0, 5 and 200 bytes: what the writer wrote, the walk reads back
  Bytes keys(205, 'q');
  const uint64_t key_off[4] = {0, 0, 5, 205}, hoff[3] = {0, 105, 100000}, hsize[3] = {100, 70000, 7};
  const uint64_t base = 100012;
  EXPECT(smt_write_tail(keys.data(), key_off, 3, hoff, hsize, base, nullptr, 0, &len) == SM_OK);
  Bytes tail(len);
  EXPECT(smt_write_tail(keys.data(), key_off, 3, hoff, hsize, base, tail.data(), len, &len) == SM_OK && len == tail.size());
  Bytes file(base, 0);
  file.insert(file.end(), tail.begin(), tail.end());
  EXPECT(footer_of(file, v) == SM_OK && v[0] == base && v[1] == 8 && v[2] == base + 13);
  smt_summary s;
  uint64_t off[3], size[3];
  Bytes contents(file.begin() + v[2], file.begin() + v[2] + v[3]);
  EXPECT(walk(contents, file.size(), &s, off, size, 3) == SM_OK && s.nblocks == 3);
  EXPECT(memcmp(off, hoff, sizeof off) == 0 && memcmp(size, hsize, sizeof size) == 0);
  EXPECT(file[v[2] + v[3]] == 0);  // stored
  // the restart array: one offset per entry, then the count
  uint32_t r;
  memcpy(&r, contents.data() + contents.size() - 4, 4);
  EXPECT(r == 3);
  uint32_t r1;
  memcpy(&r1, contents.data() + contents.size() - 12, 4);
  EXPECT(r1 == 5);  // entry 0: three fields and a two-byte handle
}

int main() {
  check_footer();
  check_index();
  check_head();
  check_tail();
  if (failures) {
    printf("smt_host_check: %d failures\n", failures);
    return 1;
  }
  printf("smt_host_check ok\n");
  return 0;
}
