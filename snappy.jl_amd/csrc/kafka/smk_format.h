// smk_format.h -- the rules of the Kafka log segment (include/snappy_mi355x_kafka.h), shared by the
// host (smk_host.cpp) and the kernels (smk_kernels.hip): the walk over the batches, a batch's head,
// a batch's and a segment's verdict, the encoder's sizes and the scratch layouts.  Plain functions,
// compiled for the host and the device alike, so the host checker tests the code the kernels run.
// Not part of the public ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <initializer_list>

#include "../../../include/snappy_mi355x_blocks.h"
#include "../../../include/snappy_mi355x_kafka.h"
#include "../common/smc_layout.h"
#include "../common/smc_slots.h"

namespace smk {

constexpr uint32_t kHeader = SMK_BATCH_HEADER_LENGTH;  // the bytes in front of the records
constexpr uint32_t kLengthEnd = 12;                    // batchLength counts the bytes behind itself
constexpr uint32_t kMinLength = kHeader - kLengthEnd;  // 49: a batch without records
constexpr uint32_t kWalkBytes = 17;                    // through the magic byte
constexpr uint32_t kCrcAt = 17, kCrcFrom = 21;         // the crc, and the first byte it covers
constexpr uint32_t kAttributesAt = 21;
constexpr uint32_t kMagic = 2;
constexpr uint32_t kCodecMask = 7;
constexpr uint64_t kMaxDeclared = 0x7fffffffull - kMinLength;
constexpr uint32_t kMaxCount = 0x7fffffffu;  // more segments, batches or chunks: SM_ERR_ARGUMENT
constexpr uint32_t kBlock = 65536;           // the encoder's piece, the decoders' fragment
using smc::kNoSlot;
using smc::round16;
enum : uint32_t { kCodecNone = SMK_CODEC_NONE, kCodecSnappy = SMK_CODEC_SNAPPY };
enum : uint32_t { kStored = 0, kXerial = 1, kRaw = 2 };  // how a batch's records are held

// 82 53 4e 41 50 50 59 00: snappy-java's stream magic, byte i
SMC_HD inline uint32_t xerial_magic_byte(uint32_t i) { return (uint32_t)(0x00595050414e5382ull >> (8 * i)) & 0xffu; }

template <typename Fetch>
SMC_HD inline uint32_t be32(Fetch& fetch, uint64_t pos) {
  uint32_t v = 0;
  for (uint32_t i = 0; i < 4; ++i) v = (v << 8) | (fetch(pos + i) & 0xffu);
  return v;
}

struct Batch {
  uint64_t pos;     // from the segment's first byte
  uint32_t length;  // batchLength
  uint32_t codec;
};

struct Walk {
  uint64_t valid = 0;  // the bytes of the recorded batches
  uint32_t nbatches = 0;
  int32_t status = SM_OK;
};

// The one walk over the n bytes of a segment.  fetch(p), p < n, is the only access, and of a batch
// only the bytes 8-11, 16 and 22 are asked for.  batch(k, b) gets batch k.
template <typename Fetch, typename Each>
SMC_HD inline Walk walk_segment(Fetch& fetch, uint64_t n, Each batch) {
  Walk w;
  uint64_t pos = 0;
  while (pos != n) {
    const uint64_t left = n - pos;
    w.status = SMK_ERR_TRUNCATED;
    if (left < kWalkBytes) break;
    const uint32_t L = be32(fetch, pos + 8);  // (read first: a walker's window then holds the other two bytes)
    w.status = SMK_ERR_MAGIC;
    if ((fetch(pos + 16) & 0xffu) != kMagic) break;
    w.status = SMK_ERR_LENGTH;
    if (L < kMinLength || L > 0x7fffffffu) break;
    w.status = SMK_ERR_TRUNCATED;
    if ((uint64_t)kLengthEnd + L > left) break;
    const uint32_t codec = fetch(pos + kAttributesAt + 1) & kCodecMask;
    w.status = SMK_ERR_CODEC;
    if (codec != kCodecNone && codec != kCodecSnappy) break;
    w.status = SM_OK;
    batch(w.nbatches, Batch{pos, L, codec});
    ++w.nbatches;
    pos += (uint64_t)kLengthEnd + L;
    w.valid = pos;
  }
  return w;
}

// the walk's fetch from a host buffer
struct ByteFetch {
  const uint8_t* p;
  uint32_t operator()(uint64_t pos) const { return p[pos]; }
};

struct Head {
  uint32_t kind;
  uint32_t declared;  // kStored and kRaw; a kXerial batch's comes from the blocks library's walk
  int32_t status;
};

// The head of a recorded batch: at most the first 8 bytes of its payload are read.
template <typename Fetch>
SMC_HD inline Head batch_head(Fetch& fetch, const Batch& b) {
  const uint32_t p = b.length - kMinLength;
  if (b.codec == kCodecNone || p == 0) return Head{kStored, b.codec == kCodecNone ? p : 0u, SM_OK};
  const uint64_t at = b.pos + kHeader;
  bool magic = p >= 8;
  for (uint32_t i = 0; magic && i < 8; ++i) magic = (fetch(at + i) & 0xffu) == xerial_magic_byte(i);
  if (magic) return Head{kXerial, 0, SM_OK};
  uint32_t d, hv;
  if (smc::parse_varint32([&](uint32_t i) { return fetch(at + i); }, p > 5 ? 5u : p, d, hv) != 0) return Head{kRaw, 0, SM_ERR_VARINT};
  if (d > kMaxDeclared) return Head{kRaw, 0, SMK_ERR_TOO_LARGE};
  return Head{kRaw, d, SM_OK};
}

// What the blocks library's walk says of a snappy-java batch (the status and the length of a decode
// call with no room, or smb_index's): the head's status and the declared length.  SM_ERR_ARGUMENT is
// that call's word for more chunks than the bound, and is passed on.
SMC_HD inline int32_t xerial_head(int32_t walk_status, uint64_t total, uint32_t& declared) {
  declared = 0;
  if (walk_status != SM_OK && walk_status != SM_BUFFER_TOO_SMALL) return walk_status;
  if (total > kMaxDeclared) return SMK_ERR_TOO_LARGE;
  declared = (uint32_t)total;
  return SM_OK;
}

SMC_HD inline uint64_t rewritten_length(uint32_t declared) { return (uint64_t)kHeader + declared; }

// byte i (< 61) of a rewritten header: h(i) is byte i of the batch as it stands; the length field
// is `length`, the codec bits `codec`; the crc's four bytes are written later and read as 0 here
template <typename At>
SMC_HD inline uint8_t header_byte(At h, uint32_t i, uint32_t length, uint32_t codec) {
  if (i >= 8 && i < 12) return (uint8_t)(length >> (8 * (11 - i)));
  if (i >= kCrcAt && i < kCrcFrom) return 0;
  if (i == kAttributesAt + 1) return (uint8_t)((h(i) & ~kCodecMask) | codec);
  return (uint8_t)h(i);
}

// ---- verdicts -----------------------------------------------------------------------------------
// A segment's status before any batch is written, and whether it is written: the walk's, its first
// failing head's, SM_BUFFER_TOO_SMALL against its room.
SMC_HD inline int32_t segment_plan(int32_t walk_status, int32_t head_status, uint64_t total, uint64_t cap) {
  if (walk_status != SM_OK) return walk_status;
  if (head_status != SM_OK) return head_status;
  return total > cap ? (int32_t)SM_BUFFER_TOO_SMALL : (int32_t)SM_OK;
}

// A written batch's status: the checksum covers the stored bytes, so it outranks the decoder.
SMC_HD inline int32_t batch_verdict(bool verify, uint32_t stored, uint32_t computed, uint32_t kind, int32_t xerial_status,
                                    int32_t raw_status) {
  if (verify && stored != computed) return SMK_ERR_CRC;
  return kind == kXerial ? xerial_status : kind == kRaw ? raw_status : (int32_t)SM_OK;
}

// ---- the encoder's sizes --------------------------------------------------------------------------
SMC_HD inline uint64_t blocks_of(uint64_t len) { return (len + kBlock - 1) / kBlock; }
// smb_max_length(len, SMB_FORMAT_XERIAL): the header, and per piece its length field and the raw bound
SMC_HD inline uint64_t xerial_max_length(uint64_t len) {
  const uint64_t full = len / kBlock, rest = len % kBlock;
  return SMB_XERIAL_HEADER_LENGTH + full * (4 + smc::max_compressed_length(kBlock)) + (rest ? 4 + smc::max_compressed_length(rest) : 0u);
}
SMC_HD inline uint64_t stage_length(uint64_t len) { return len ? round16(xerial_max_length(len)) : 0u; }
SMC_HD inline uint64_t max_segment_length(uint64_t n, uint64_t nbatches) { return n + n / 6 + 36 * (n / kBlock) + 52 * nbatches; }
SMC_HD inline bool compressed_here(const Batch& b) { return b.codec == kCodecNone && b.length > kMinLength; }
// the size of an encoded batch whose payload became clen bytes (0: it had none)
SMC_HD inline uint64_t encoded_length(const Batch& b, uint64_t clen) {
  return b.codec == kCodecNone ? (uint64_t)kHeader + clen : (uint64_t)kLengthEnd + b.length;
}
SMC_HD inline uint64_t decode_fragments(uint64_t ulen) { return (ulen + kBlock - 1) / kBlock; }

const char* host_message(sm_status st);  // smk_host.cpp: the SMK_ERR_* and SMB_ERR_* texts, else NULL

// ---- scratch (smc::Carve: a null base measures) ------------------------------------------------
using Header = smc::PlanHeader;  // total: batches recorded; over: more than one of the caller's bounds

// per segment (ns), what both calls' walks keep
struct Segments {
  uint32_t *count, *first, *fail;  // first: ns + 1
  int32_t *walk, *pre;
};

// per batch (m), what both calls' walks keep
struct Batches {
  uint64_t* pos;
  uint32_t *length, *codec, *segment;
};

struct Decode {
  Header* hdr;
  Segments g;
  Batches b;
  uint64_t* prefix;  // m + 1: the exclusive scan of the rewritten lengths
  uint32_t *kind, *decl;
  int32_t* head;
  // the snappy-java batches as streams of the blocks library's call, twice: the sizes, the decode
  uint64_t *x_in_off, *x_in_len, *x_out_off, *x_cap, *x_len;
  int32_t* x_status;
  // the raw batches as streams of the multi library's calls
  uint64_t *r_in_off, *r_out_off;
  uint32_t *r_in_len, *r_cap, *r_out_len, *frag_first, *frag_pos;  // frag_first: m + 1; frag_pos: max(max_fragments, 1)
  int32_t *r_status, *r_index_status;
  uint8_t* built;
  uint32_t* copy;  // the stored batches' payload lengths (0: nothing to copy)
  uint64_t* out_at;  // a written batch's first output byte in d_out
  // the checksums: of the stored bytes, of the rewritten ones
  uint64_t *ci_off, *co_off;
  uint32_t *ci_len, *co_len, *stored, *computed, *crc;
  int32_t* status;
  uintptr_t end;
};

inline void carve_walk(smc::Carve& c, Segments& g, Batches& b, size_t ns, size_t m) {
  g.count = c.take<uint32_t>(ns);
  g.first = c.take<uint32_t>(ns + 1);
  g.fail = c.take<uint32_t>(ns);
  g.walk = c.take<int32_t>(ns);
  g.pre = c.take<int32_t>(ns);
  b.pos = c.take<uint64_t>(m);
  for (uint32_t** p : {&b.length, &b.codec, &b.segment}) *p = c.take<uint32_t>(m);
}

inline Decode carve_decode(uint8_t* buf, size_t ns, size_t m, size_t max_fragments) {
  smc::Carve c{reinterpret_cast<uintptr_t>(buf)};
  Decode s;
  s.hdr = c.take<Header>(1);
  carve_walk(c, s.g, s.b, ns, m);
  s.prefix = c.take<uint64_t>(m + 1);
  for (uint64_t** p : {&s.x_in_off, &s.x_in_len, &s.x_out_off, &s.x_cap, &s.x_len, &s.r_in_off, &s.r_out_off, &s.out_at, &s.ci_off, &s.co_off})
    *p = c.take<uint64_t>(m);
  for (uint32_t** p : {&s.kind, &s.decl, &s.r_in_len, &s.r_cap, &s.r_out_len, &s.copy, &s.ci_len, &s.co_len, &s.stored, &s.computed, &s.crc})
    *p = c.take<uint32_t>(m);
  for (int32_t** p : {&s.head, &s.x_status, &s.r_status, &s.r_index_status, &s.status}) *p = c.take<int32_t>(m);
  s.frag_first = c.take<uint32_t>(m + 1);
  s.frag_pos = c.take<uint32_t>(max_fragments ? max_fragments : 1);
  s.built = c.take<uint8_t>(m);
  s.end = c.p;
  return s;
}
inline size_t decode_bytes(size_t ns, size_t m, size_t max_fragments) { return (size_t)carve_decode(nullptr, ns, m, max_fragments).end; }

struct Compress {
  Header* hdr;
  Segments g;
  Batches b;
  uint64_t* size_scan;  // m + 1: the exclusive scan of the encoded batch sizes
  uint64_t *c_in_off, *c_in_len, *slot_off, *c_len, *co_off;
  uint32_t *co_len, *crc;
  int32_t* c_status;
  uint8_t* stage;  // stage_bytes: the blocks library's streams
  uintptr_t end;
};

inline Compress carve_compress(uint8_t* buf, size_t ns, size_t m, size_t stage_bytes) {
  smc::Carve c{reinterpret_cast<uintptr_t>(buf)};
  Compress s;
  s.hdr = c.take<Header>(1);
  carve_walk(c, s.g, s.b, ns, m);
  s.size_scan = c.take<uint64_t>(m + 1);
  for (uint64_t** p : {&s.c_in_off, &s.c_in_len, &s.slot_off, &s.c_len, &s.co_off}) *p = c.take<uint64_t>(m);
  for (uint32_t** p : {&s.co_len, &s.crc}) *p = c.take<uint32_t>(m);
  s.c_status = c.take<int32_t>(m);
  s.stage = c.take<uint8_t>(stage_bytes ? stage_bytes : 1);
  s.end = c.p;
  return s;
}
inline size_t compress_bytes(size_t ns, size_t m, size_t stage_bytes) { return (size_t)carve_compress(nullptr, ns, m, stage_bytes).end; }

}  // namespace smk
