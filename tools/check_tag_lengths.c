// Design check for the decoder's batch checks (decode_stream_batch in
// snappy.jl_amd/csrc/sm_decompress.hip): a tag that the window walk hands to a lane -- one whose
// speculative size is not 255 -- decodes to a bounded length, and its size is what the clean-batch
// lemma says.  For every tag byte c, every next byte b and the following three bytes at their
// extremes, with the fields decoded as the engine decodes them (char_entry, the low taglen bytes
// of the zero-padded lookahead):
//   * a copy makes len <= 64 bytes and has size 1 + taglen;
//   * a literal makes litlen <= kMaxBatchLit (200) bytes and has size 1 + taglen + litlen, so
//     lsrc + litlen is the next tag's position;
// so min(olen, 65537) never binds and a batch of 64 tags makes at most 64 * 200 bytes.  The same
// loop checks the fields the batch decode derives from that size (csz) instead of char_entry's
// select tree: a copy's trailer bytes csz - 1, length and high offset bits from the kind; a
// literal's length bytes (c + 16) >> 8 and length csz - 1 - those.
// spec_size restates the per-byte definition that tools/check_tag_sizes.c checks pack_sizes
// against.  Plain C; run by tests/test_decoder_batch_invariant.py.
#include <stdint.h>
#include <stdio.h>
static uint32_t char_entry(uint32_t c) {
  uint32_t kind = c & 3, hi = c >> 2;
  if (kind == 0) return hi < 60 ? hi + 1 : (((hi - 59) << 11) | 1);
  if (kind == 1) return (1u << 11) | ((c >> 5) << 8) | (4 + ((c >> 2) & 7));
  if (kind == 2) return (2u << 11) | (hi + 1);
  return (4u << 11) | (hi + 1);
}
// the per-byte definition (255: a literal the batch walk leaves to the general path)
static uint32_t spec_size(uint32_t c, uint32_t trailer) {
  uint32_t entry = char_entry(c), taglen = entry >> 11;
  if (c & 3) return 1 + taglen;
  uint32_t hi = c >> 2;
  if (hi < 60) return 1 + (entry & 0xff);
  if (hi > 60) return 255u;  // two to four length bytes
  uint32_t lit = 1 + (trailer & 0xff);
  return lit > 200 ? 255u : 1 + taglen + lit;
}
int main(void) {
  static const uint32_t rest[] = {0x000000u, 0xffffffu, 0x0000ffu, 0xff0000u, 0x5a3c96u};
  long bad = 0, walked = 0;
  uint32_t max_copy = 0, max_lit = 0;
  for (uint32_t c = 0; c < 256; ++c)
    for (uint32_t b = 0; b < 256; ++b)
      for (unsigned r = 0; r < sizeof rest / sizeof rest[0]; ++r) {
        const uint32_t tr_raw = b | (rest[r] << 8);  // the four bytes after the tag byte
        const uint32_t size = spec_size(c, tr_raw);
        if (size == 255) continue;
        ++walked;
        const uint32_t entry = char_entry(c), len = entry & 0xff, taglen = entry >> 11;
        const uint32_t trailer = taglen >= 4 ? tr_raw : (tr_raw & ((1u << (8 * taglen)) - 1u));
        const int iscopy = (c & 3) != 0;
        const uint32_t litlen = len + trailer, olen = iscopy ? len : litlen;
        int ok = olen <= 200 && olen >= 1;
        // the fields as the batch decode takes them from the walk's size instead of char_entry
        const uint32_t kind = c & 3, hi = c >> 2, tl = (c + 16) >> 8;
        if (iscopy) {
          ok = ok && olen <= 64 && size == 1 + taglen;
          ok = ok && len == (kind == 1 ? 4 + (hi & 7) : hi + 1);
          ok = ok && (entry & 0x700) == (kind == 1 ? (c << 3) & 0x700u : 0u);
          if (olen > max_copy) max_copy = olen;
        } else {
          ok = ok && size == 1 + taglen + litlen;
          ok = ok && tl == taglen && litlen == size - 1 - tl;
          if (olen > max_lit) max_lit = olen;
        }
        if (!ok) {
          if (bad < 5) printf("tag %02x next %02x rest %06x: size %u olen %u taglen %u\n", c, b, rest[r], size, olen, taglen);
          ++bad;
        }
      }
  printf("bad %ld of %ld walked tags, longest copy %u, longest literal %u\n", bad, walked, max_copy, max_lit);
  return bad != 0;
}
