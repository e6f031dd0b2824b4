// smq_thrift.h -- a reader of the Thrift compact protocol (include/snappy_mi355x_parquet.h), as far
// as a Parquet PageHeader needs it: field headers, the integer types and a generic skip of any value
// at any nesting up to SMQ_MAX_DEPTH.  The bytes come through a `fetch` functor alone -- fetch(pos)
// is byte pos of a buffer of n bytes, asked only for pos < n -- so nothing at or behind the end is
// ever read, whatever lies there.  Plain C++, compiled for the host and the device alike: on the
// device one wave runs it, every lane taking the same steps.  Not part of the public ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../../include/snappy_mi355x_parquet.h"
#include "../common/smc_layout.h"

// The reader and the walk over it are inlined into their kernel whole: the reader's cursor and
// status then live in the wave's scalar registers, not in a stack frame behind a call.
#define SMQ_INLINE SMC_HD inline __attribute__((always_inline))

namespace smq {

enum : uint32_t {
  kStop = 0, kTrue = 1, kFalse = 2, kByte = 3, kI16 = 4, kI32 = 5, kI64 = 6, kDouble = 7, kBinary = 8, kList = 9, kSet = 10,
  kMap = 11, kStruct = 12
};

// one open container of a skip: a struct (its fields up to the stop byte), or the `left` values
// still to come of a list or set (all of type a) or of a map (in turn of types a and b)
struct Frame {
  uint32_t left;
  uint8_t kind, a, b;  // kind: kStruct, kList or kMap
};

// A value every lane of the walking wave holds alike, read back from the frames: on the device it
// is made the wave's own again, so what it steers stays the wave's work.
SMC_HD inline uint32_t uniform(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_readfirstlane(v);
#else
  return v;
#endif
}

template <typename Fetch>
struct Reader {
  Fetch& fetch;
  uint64_t n;
  Frame* stack;  // SMQ_MAX_DEPTH frames, the skip's own
  uint64_t pos = 0;
  int32_t status = SM_OK;  // the first error; behind it every read gives 0 and nothing moves

  SMC_HD Reader(Fetch& f, uint64_t n_, Frame* stack_) : fetch(f), n(n_), stack(stack_) {}

  SMQ_INLINE bool ok() const { return status == SM_OK; }
  SMQ_INLINE void fail(int32_t st) {
    if (status == SM_OK) status = st;
  }

  SMQ_INLINE uint32_t byte() {
    if (status != SM_OK) return 0;
    if (pos >= n) {
      status = SMQ_ERR_TRUNCATED;
      return 0;
    }
    return fetch(pos++);
  }

  // an unsigned varint of at most max_bytes bytes (bits above 64 are dropped)
  SMQ_INLINE uint64_t varint(uint32_t max_bytes) {
    uint64_t v = 0;
    uint32_t shift = 0;
    for (uint32_t i = 0; i < max_bytes; ++i, shift += 7) {
      const uint32_t b = byte();
      if (status != SM_OK) return 0;
      if (shift < 64) v |= (uint64_t)(b & 0x7f) << shift;
      if (b < 0x80) return v;
    }
    fail(SMQ_ERR_HEADER);
    return 0;
  }

  SMQ_INLINE int64_t zigzag(uint32_t max_bytes) {
    const uint64_t v = varint(max_bytes);
    return (int64_t)(v >> 1) ^ -(int64_t)(v & 1);
  }

  // an i32 field's value; one that does not fit 32 bits is SMQ_ERR_HEADER
  SMQ_INLINE int32_t i32() {
    const int64_t v = zigzag(5);
    if (v < INT32_MIN || v > INT32_MAX) {
      fail(SMQ_ERR_HEADER);
      return 0;
    }
    return status == SM_OK ? (int32_t)v : 0;
  }

  SMQ_INLINE void advance(uint64_t k) {
    if (status != SM_OK) return;
    if (k > n - pos) {
      status = SMQ_ERR_TRUNCATED;
      return;
    }
    pos += k;
  }

  // The next field header of a struct whose previous field id was `id`: false at the stop byte (or
  // after an error), else the field's type (1 .. 12) and its id.
  SMQ_INLINE bool field(int32_t& id, uint32_t& type) {
    const uint32_t b = byte();
    if (status != SM_OK || b == kStop) return false;
    type = b & 15;
    if (type == kStop || type > kStruct) {
      fail(SMQ_ERR_HEADER);
      return false;
    }
    const uint32_t delta = b >> 4;
    id = delta ? (int32_t)((uint32_t)id + delta) : (int32_t)zigzag(3);
    return status == SM_OK;
  }

  // Steps over a value of `type` that stands at depth `depth` (a PageHeader's fields at 1); element:
  // a list's, set's or map's, where a bool is a byte of its own.
  SMQ_INLINE void skip(uint32_t type, uint32_t depth, bool element = false) {
    uint32_t top = 0;  // open frames; frame k's values stand at depth + 1 + k
    open(type, depth, element, top);
    while (status == SM_OK && top) {
      Frame& f = stack[top - 1];
      const uint32_t kind = uniform(f.kind), left = uniform(f.left);
      uint32_t t;
      bool elem = true;
      if (kind == kStruct) {
        int32_t id = 0;  // (a skip needs no ids)
        if (!field(id, t)) {
          --top;
          continue;
        }
        elem = false;
      } else {
        if (left == 0) {
          --top;
          continue;
        }
        t = uniform(kind == kMap && (left & 1) ? f.b : f.a);  // (a map's keys come at an even count left)
        f.left = left - 1;
      }
      open(t, depth + top, elem, top);
    }
  }

 private:
  // a scalar is stepped over; a container opens a frame (or fails at depth SMQ_MAX_DEPTH + 1)
  SMQ_INLINE void open(uint32_t type, uint32_t depth, bool element, uint32_t& top) {
    switch (type) {
      case kTrue:
      case kFalse: if (element) advance(1); return;
      case kByte: advance(1); return;
      case kI16: (void)varint(3); return;
      case kI32: (void)varint(5); return;
      case kI64: (void)varint(10); return;
      case kDouble: advance(8); return;
      case kBinary: {
        const uint64_t len = varint(5);
        advance(len);
        return;
      }
      case kList:
      case kSet:
      case kMap:
      case kStruct: break;
      default: fail(SMQ_ERR_HEADER); return;
    }
    if (depth + 1 > SMQ_MAX_DEPTH) {  // the container's own depth
      fail(SMQ_ERR_HEADER);
      return;
    }
    Frame f{0, (uint8_t)kStruct, 0, 0};
    if (type == kList || type == kSet) {
      const uint32_t b = byte();
      uint64_t size = b >> 4;
      if (size == 15) size = varint(5);
      f.kind = kList;
      f.a = (uint8_t)(b & 15);
      if (status != SM_OK) return;
      if (size && !valid_element(f.a)) {
        fail(SMQ_ERR_HEADER);
        return;
      }
      // elements of a fixed size are stepped over at once
      const uint32_t fixed = f.a <= kByte ? 1 : f.a == kDouble ? 8 : 0;
      if (fixed) {
        advance(size * fixed);
        size = 0;
      }
      f.left = (uint32_t)size;  // (a varint of 5 bytes is above 32 bits only with bits the next line refuses)
      if (size > 0xffffffffull) fail(SMQ_ERR_HEADER);
    } else if (type == kMap) {
      const uint64_t size = varint(5);
      f.kind = kMap;
      if (size) {
        const uint32_t b = byte();
        f.a = (uint8_t)(b >> 4);
        f.b = (uint8_t)(b & 15);
        if (status == SM_OK && (!valid_element(f.a) || !valid_element(f.b) || size > 0x7fffffffull)) fail(SMQ_ERR_HEADER);
      }
      f.left = (uint32_t)(2 * size);  // keys and values in turn: an even count left means a key is next
    }
    if (status != SM_OK) return;
    stack[top++] = f;
  }

  SMC_HD static bool valid_element(uint32_t t) { return t >= kTrue && t <= kStruct; }
};

}  // namespace smq
