// smm_host_check.cpp -- stand-alone driver of smm_host.cpp (no device, no HIP): the index rules of
// smm_uncompress_device over every structural case, on heap buffers of exactly the documented sizes,
// so that AddressSanitizer and UBSan (make host_check) see any read past an array that an index
// value could cause.  The rules are the device plan's own code (smm_plan.h).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "smm_plan.h"

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
  if (failures) {
    fprintf(stderr, "smm_host_check: %d failure(s)\n", failures);
    return 1;
  }
  printf("smm_host_check: ok\n");
  return 0;
}
