/*
 * snappy_mi355x_table.h -- C ABI of libsnappy_mi355x_table.so: LevelDB table files (.ldb / .sst),
 * whose blocks are stored or Snappy-compressed and carry a masked CRC-32C, in batches on the
 * device.  A companion of libsnappy_mi355x_multi.so (snappy_mi355x_multi.h),
 * libsnappy_mi355x_framing.so (snappy_mi355x_framing.h, for its batched masked CRC-32C) and
 * libsnappy_mi355x.so (snappy_mi355x.h).
 *
 * This is the table's block layer and nothing above it: no key is compared, no data block's entries
 * are parsed, no filter block is read, and the metaindex handle is parsed but never followed.
 *
 * It is layered on the public entry points smm_index_device, smm_uncompress_device,
 * smm_compress_device and smf_crc32c_batch_device and links those libraries and the main one by
 * name; all four must sit in one directory.  Status codes are snappy_mi355x.h's plus SMT_ERR_* below.
 *
 * ---- the format (LevelDB doc/table_format.md), and the rules -----------------------------------
 * VARINTS.  An index entry's three fields are varint32 by the raw decoder's rule: up to 5 bytes of
 * 7-bit groups.  LevelDB's GetVarint32Ptr drops the high bits of a fifth byte; here a fifth byte of
 * 0x10 or more is an error, as is a sixth byte.  A block handle is two varint64 (offset, size): up to
 * 10 bytes of 7-bit groups each; a tenth byte above 1, or running past the field's end, is an error.
 *
 * THE FOOTER is the last 48 bytes of the n bytes of a table:
 *   n < 48: SMT_ERR_TRUNCATED.
 *   The last 8 bytes are not 57 fb 80 8b 24 75 47 db (0xdb4775248b80fb57, little-endian):
 *     SMT_ERR_MAGIC.
 *   The 40 bytes before the magic hold the metaindex handle, then the index handle; the rest is
 *     padding and is ignored.  A varint64 that fails or leaves the 40 bytes: SMT_ERR_FOOTER.
 *   A handle (off, size) is valid when off + size + 5 <= n - 48, computed without overflow; else
 *     SMT_ERR_HANDLE.  Then size > 0x7ffffffe: SMT_ERR_TOO_LARGE.  The metaindex handle is checked
 *     first, then the index handle.  Only the index handle is followed.
 *
 * A STORED BLOCK at handle (off, size): `size` bytes of contents, then the type (1 byte), then the
 * fixed32 little-endian crc: the masked CRC-32C (Castagnoli, reflected polynomial 0x82F63B78) of the
 * size + 1 bytes of contents plus type, masked = ((c >> 15) | (c << 17)) + 0xa282ead8.
 *   type 0: the contents are the block; its declared length is size.
 *   type 1: the contents are one raw Snappy stream; its declared length d is the raw decoder's
 *     varint over the first min(size, 5) bytes.  It does not parse (size 0 included):
 *     SM_ERR_VARINT.  d > 0x7fffffff: SMT_ERR_TOO_LARGE.
 *   any other type: SMT_ERR_TYPE (newer LevelDB's zstd type 2 is refused, not guessed at).
 *
 * THE INDEX BLOCK's contents, over their m decoded bytes (LevelDB's Block and DecodeEntry):
 *   m < 4: SMT_ERR_INDEX.  r = the u32 at m - 4; r > (m - 4) / 4: SMT_ERR_INDEX.
 *   limit = m - 4 (1 + r).  The restart array itself is not consulted.
 *   Entries run from p = 0; p == limit ends the walk.  Each entry:
 *     fewer than 3 bytes left in [p, limit): SMT_ERR_INDEX;
 *     shared, non_shared, value_len: three varint32 inside [p, limit); a bad one: SMT_ERR_INDEX;
 *     non_shared + value_len past limit: SMT_ERR_INDEX;
 *     shared above the previous entry's key length (shared + non_shared of that entry; 0 before the
 *       first): SMT_ERR_INDEX -- LevelDB's key_.size() < shared check, made without touching a key
 *       byte;
 *     the value holds a handle, two varint64 inside the value (trailing bytes are ignored, as
 *       LevelDB does); a parse failure: SMT_ERR_INDEX;
 *     the handle is checked against the table like the footer's (SMT_ERR_HANDLE, SMT_ERR_TOO_LARGE).
 *   The walk stops at its first error.
 *
 * STATUS ORDER FOR A TABLE (checksum rules apply when verify_crc is not 0):
 *   1. The first failure among: the footer; the index block's type; the index block's CRC
 *      (SMT_ERR_CRC); the raw decoder's status on the index block (its varint included); the index
 *      contents; the first data block, in block order, whose head fails (SMT_ERR_TYPE,
 *      SM_ERR_VARINT, SMT_ERR_TOO_LARGE).
 *   2. A table failing at any of these is not decoded and takes no slots.  d_out_len[t] = the sum of
 *      the declared lengths of the blocks before the failure (0 when it precedes the data blocks).
 *   3. A well-formed table longer than d_out_cap[t]: SM_BUFFER_TOO_SMALL, d_out_len[t] = the size
 *      needed.  Nothing is decoded.
 *   4. Otherwise every block decodes to d_out_off[t] plus the declared lengths before it.
 *   5. A block's status is SMT_ERR_CRC where the stored checksum differs.  The checksum covers the
 *      STORED bytes, so it is known before any decode and outranks the decoder.
 *   6. Failing that, the block's status is the raw decoder's; for a type-0 block SM_OK.
 *   7. The table's status is its first failing block's, in block order.  A failing block does not
 *      stop the others; its output range holds unspecified bytes inside its own range.
 *
 * THE ENCODER.  A block is written compressed (type 1, contents exactly sm_compress(block, mode))
 * when the compressor's status is SM_OK and clen < len - len / 8 (LevelDB's 12.5 % rule), else
 * stored (type 0).  It takes chosen + 5 bytes: smt_max_block_length(len) = len + 5.
 *
 * ROCKSDB.  By RocksDB's format documentation its block-based tables written with kCRC32c and
 * format_version below 6 use this block and trailer layout for Snappy and uncompressed blocks, so a
 * caller who holds the handles can use the handle-level calls; nothing here has been held against a
 * RocksDB file.  Its footer and index encodings are out of scope: a non-LevelDB magic is
 * SMT_ERR_MAGIC.
 *
 * Threading: an smt_ctx owns an smm_ctx, an smf_ctx and scratch, and one caller at a time may use
 * it: the *_device calls keep their per-call arrays (and the decoded index blocks) in the ctx's
 * scratch, so two of them on one ctx must be on one stream (or ordered by the caller), and a call
 * that grows the scratch waits for the device first (hipFree).  The host-buffer calls lock the ctx.
 * No *_device call synchronises otherwise: every decision is taken on the device.
 */
#ifndef SNAPPY_MI355X_TABLE_H_
#define SNAPPY_MI355X_TABLE_H_

#include <stddef.h>
#include <stdint.h>

#include "snappy_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
  SMT_ERR_TRUNCATED = 96,  /* a table of fewer than 48 bytes */
  SMT_ERR_MAGIC = 97,      /* the last 8 bytes are not LevelDB's table magic */
  SMT_ERR_FOOTER = 98,     /* a footer handle's varint64 fails or leaves the footer */
  SMT_ERR_HANDLE = 99,     /* a handle's block and trailer do not lie in front of the footer */
  SMT_ERR_TOO_LARGE = 100, /* a handle's size above 0x7ffffffe, or a declared length above 0x7fffffff */
  SMT_ERR_TYPE = 101,      /* a block's type byte is neither 0 (stored) nor 1 (Snappy) */
  SMT_ERR_INDEX = 102,     /* the index block's contents are malformed */
  SMT_ERR_CRC = 103        /* a block's stored masked CRC-32C differs from that of its bytes */
};

#define SMT_FOOTER_LENGTH 48
#define SMT_BLOCK_TRAILER 5

typedef struct smt_ctx smt_ctx;

typedef struct smt_summary {
  uint64_t total_length; /* the sizes of the recorded handles, summed */
  uint32_t nblocks;      /* entries walked: all of them, or those before the error */
  int32_t status;        /* SM_OK, a walk error, or SM_BUFFER_TOO_SMALL (nblocks > max) */
} smt_summary;

/* ---- host helpers (no device needed) ------------------------------------------------- */
/* the SMT_ERR_* texts, else the main library's */
const char* smt_status_message(sm_status st);
/* library build identification ("snappy_mi355x_table gfx950 <source hash>") */
const char* smt_version(void);
/* The footer rule.  SM_ERR_ARGUMENT for a NULL result or buffer. */
sm_status smt_footer(const uint8_t* buf, size_t n, uint64_t* meta_off, uint64_t* meta_size, uint64_t* index_off,
                     uint64_t* index_size);
/* The footer plus the index block's head: *index_bytes = the exact decoded length of the index
 * block, without decoding it.  The footer's status, else the head's (SMT_ERR_TYPE, SM_ERR_VARINT,
 * SMT_ERR_TOO_LARGE). */
sm_status smt_index_bound(const uint8_t* buf, size_t n, uint64_t* index_bytes);
/* the most entries index contents of that many bytes hold: index_bytes / 5 (the shortest entry is
 * three one-byte fields and a two-byte handle) */
uint64_t smt_max_blocks(uint64_t index_bytes);
/* The index rule over already-decoded contents of m bytes, for a table of table_len bytes.  Entries
 * [0, min(nblocks, max)) are stored when both arrays are given; more entries than max with the
 * arrays given: SM_BUFFER_TOO_SMALL.  Returns summary->status. */
sm_status smt_walk_index(const uint8_t* contents, size_t m, uint64_t table_len, uint64_t* handles_off,
                         uint64_t* handles_size, uint32_t max, smt_summary* summary);
/* The head of the block at the (trusted) handle (off, size) of a buffer of n bytes: its type and
 * declared length.  SMT_ERR_HANDLE when off + size + 5 > n. */
sm_status smt_block_head(const uint8_t* buf, size_t n, uint64_t off, uint64_t size, uint32_t* type, uint64_t* declared);
/* the encoder's bound for a block of len bytes: len + 5 */
uint64_t smt_max_block_length(uint64_t len);
/* a block's share of the encoder's stage: sm_max_compressed_length(len) rounded up to 16 */
uint64_t smt_stage_length(uint64_t len);
/* the device memory a *_device call of that shape keeps in the ctx (the larger of the decoder's and
 * the encoder's needs, the decoded index blocks and the encoder's stage included), the smm_ctx's
 * and the smf_ctx's own scratch not counted */
size_t smt_tables_scratch_bytes(uint32_t ntables, uint32_t max_blocks, uint64_t max_index_bytes, uint32_t max_fragments,
                                uint64_t stage_bytes);
/* The tail of a table whose data blocks (nblocks of them, with their trailers, handles from the
 * table's first byte) take the `base` bytes in front: an empty metaindex block (00 00 00 00 01 00
 * 00 00, type 0), a stored index block with restart interval 1 (every shared is 0) whose entry j has
 * the key keys[key_off[j] .. key_off[j + 1]) -- the caller's separator keys, not interpreted -- and
 * the handle (handle_off[j], handle_size[j]), each with its trailer, then the footer.  *out_len =
 * its size; written when out is given and out_cap suffices, else (out given) SM_BUFFER_TOO_SMALL. */
sm_status smt_write_tail(const uint8_t* keys, const uint64_t* key_off, uint32_t nblocks, const uint64_t* handle_off,
                         const uint64_t* handle_size, uint64_t base, uint8_t* out, size_t out_cap, size_t* out_len);

/* ---- context ------------------------------------------------------------------------ */
/* NULL without a usable device */
smt_ctx* smt_ctx_create(int device);
void smt_ctx_destroy(smt_ctx* ctx);
/* diagnostic: smm_ctx_last_indexed of the ctx's smm_ctx -- the number of blocks the last decode
 * call took by fragments; waits for the device.  -1 for a NULL ctx or before the first decode. */
int smt_ctx_last_indexed(smt_ctx* ctx);

/* ---- device memory, asynchronous on `stream` (a hipStream_t; NULL = the default stream) ----
 * The offset, length and capacity arrays are trusted; the table bytes are not.  There is no host
 * synchronisation except when the scratch grows.
 *
 * Index.  Table t = d_in[d_in_off[t] .. +d_in_len[t]) at any alignment.  Stages: the footers (a
 * thread per table) with the index block's head; the index blocks' masked CRC-32C (verify_crc, one
 * smf_crc32c_batch_device call); the index blocks into the ctx's scratch, each at a 16-byte
 * boundary -- one smm_uncompress_device call for the compressed ones, one tiled copy for the stored
 * ones; the walk over those bytes, one wave per table, twice (count, fill) with a scan between.
 * d_status[t] = the first failure of steps footer .. index contents of the status order above, else
 * SM_OK.  A failing table has no entries.  d_block_first (ntables + 1) = the exclusive scan of the
 * entry counts; d_handle_off / d_handle_size (max_blocks entries) = entry j's handle, its offset
 * from the table's first byte.
 * max_blocks bounds d_block_first[ntables]; max_index_bytes bounds the sum of the decoded index
 * lengths, each rounded up to 16 (smt_index_bound).  Over either bound every d_status[t] =
 * SM_ERR_ARGUMENT and nothing else is written.
 * Returns SM_ERR_ARGUMENT for a NULL ctx or array, ntables or max_blocks above 0x7fffffff;
 * SM_ERR_DEVICE when a launch or an allocation failed. */
sm_status smt_index_tables_device(smt_ctx* ctx, const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                  uint32_t ntables, uint32_t max_blocks, uint64_t max_index_bytes, int verify_crc,
                                  uint32_t* d_block_first, uint64_t* d_handle_off, uint64_t* d_handle_size,
                                  int32_t* d_status, void* stream);

/* Decode by handles.  Block j's contents are d_in[d_blk_off[j] .. +d_blk_size[j]) with the 5-byte
 * trailer behind them; the handles are trusted (d_blk_size[j] <= 0x7ffffffe).  Per block, with its
 * declared length d: a failing head: d_status[j] = SMT_ERR_TYPE, SM_ERR_VARINT or
 * SMT_ERR_TOO_LARGE, d_out_len[j] = 0; d > d_out_cap[j]: SM_BUFFER_TOO_SMALL, d_out_len[j] = d; in
 * both cases nothing of it is written.  Otherwise it decodes (type 1) or is copied (type 0) to
 * d_out + d_out_off[j], d_out_len[j] = d, and d_status[j] follows block rules 5 and 6 above.
 * All compressed blocks go through smm_index_device (max_fragments > 0) and smm_uncompress_device
 * once each, so a block above 64 KiB decodes by fragments; max_fragments is a speed hint only, as in
 * snappy_mi355x_avro.h.  Stored blocks go through one tiled copy; the checksums through one
 * smf_crc32c_batch_device call (masked) over the stored size + 1 bytes. */
sm_status smt_uncompress_blocks_device(smt_ctx* ctx, const uint8_t* d_in, const uint64_t* d_blk_off,
                                       const uint64_t* d_blk_size, uint32_t nblocks, uint32_t max_fragments, int verify_crc,
                                       uint8_t* d_out, const uint64_t* d_out_off, const uint64_t* d_out_cap,
                                       uint64_t* d_out_len, int32_t* d_status, void* stream);

/* Decode whole tables: smt_index_tables_device, a thread-per-block head kernel, the scan of the
 * declared lengths (which also gives each table's first failing head), then the decode of
 * smt_uncompress_blocks_device over all blocks of all tables that are decoded -- the table rules
 * above.  Table t decodes into d_out[d_out_off[t] .. +d_out_cap[t]); d_out_len[t] and d_status[t]
 * per table.  No byte is read outside a table's own range and none written outside its room.
 * Optional outputs (NULL: not wanted): d_block_first (ntables + 1); per entry (max_blocks each)
 * d_handle_off, d_handle_size, d_block_out_off (from the table's first output byte), d_block_len
 * (the declared length) and d_block_status (0 for a block of a table that is not decoded).
 * Over max_blocks or max_index_bytes: every d_status[t] = SM_ERR_ARGUMENT, every d_out_len[t] = 0
 * and nothing else is written. */
sm_status smt_uncompress_tables_device(smt_ctx* ctx, const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                       uint32_t ntables, uint32_t max_blocks, uint64_t max_index_bytes,
                                       uint32_t max_fragments, int verify_crc, uint8_t* d_out, const uint64_t* d_out_off,
                                       const uint64_t* d_out_cap, uint64_t* d_out_len, int32_t* d_status,
                                       uint32_t* d_block_first, uint64_t* d_handle_off, uint64_t* d_handle_size,
                                       uint64_t* d_block_out_off, uint64_t* d_block_len, int32_t* d_block_status,
                                       void* stream);

/* Encode.  Table t is the blocks d_block_first[t] .. d_block_first[t + 1] of the flat arrays: block
 * j = d_in[d_block_off[j] .. +d_block_len[j]), written by the encoder rule above, back to back, at
 * d_out + d_out_off[t], where the sum of smt_max_block_length(d_block_len[j]) must be free.
 * d_handle_off[j] (from the table's first output byte) and d_handle_size[j] per block; d_out_len[t]
 * = the bytes written; d_status[t] = SM_OK, or SM_ERR_INPUT_TOO_LARGE (a block above 0x7ffffffe
 * bytes: nothing of the table is written).
 * The pipeline: one smm_compress_device call into a stage, the 12.5 % decision, the scan of the
 * sizes, the pack (contents and type byte), one smf_crc32c_batch_device call (masked) over the packed
 * size + 1 ranges, and a kernel that stores the four checksum bytes at any alignment.
 * max_blocks bounds d_block_first[ntables], stage_bytes the sum of smt_stage_length(d_block_len[j]),
 * max_fragments the sum of smm_fragment_count(d_block_len[j]) over the blocks of more than 64 KiB;
 * over any of them every d_status[t] = SM_ERR_ARGUMENT, every d_out_len[t] = 0 and nothing is
 * written to d_out.  mode: SM_MODE_*. */
sm_status smt_compress_blocks_device(smt_ctx* ctx, const uint8_t* d_in, const uint32_t* d_block_first,
                                     const uint64_t* d_block_off, const uint32_t* d_block_len, uint32_t ntables,
                                     uint32_t max_blocks, uint64_t stage_bytes, uint32_t max_fragments, uint8_t* d_out,
                                     const uint64_t* d_out_off, uint64_t* d_handle_off, uint64_t* d_handle_size,
                                     uint64_t* d_out_len, int32_t* d_status, int mode, void* stream);

/* ---- host memory (one upload, the device path, one download; synchronous; lock the ctx) ----
 * The arrays as above, in host memory; the bounds are sized here with smt_index_bound and
 * smt_max_blocks.  Only each table's (block's) own range out[out_off .. +out_len) is written, and
 * only when out_len fits its capacity; where the status is not SM_OK that range holds unspecified
 * bytes.  smt_uncompress_tables: block_first (ntables + 1) and the four per-entry arrays are
 * optional, all or none, with room for max_entries entries; more entries than that:
 * SM_BUFFER_TOO_SMALL and nothing is written. */
sm_status smt_uncompress_tables(smt_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len,
                                uint32_t ntables, int verify_crc, uint8_t* out, const uint64_t* out_off,
                                const uint64_t* out_cap, uint64_t* out_len, int32_t* status, uint32_t* block_first,
                                uint32_t max_entries, uint64_t* handle_off, uint64_t* handle_size, uint64_t* block_len,
                                int32_t* block_status);
sm_status smt_uncompress_blocks(smt_ctx* ctx, const uint8_t* in, size_t n, const uint64_t* blk_off, const uint64_t* blk_size,
                                uint32_t nblocks, int verify_crc, uint8_t* out, const uint64_t* out_off,
                                const uint64_t* out_cap, uint64_t* out_len, int32_t* status);
sm_status smt_compress_blocks(smt_ctx* ctx, const uint8_t* in, const uint32_t* block_first, const uint64_t* block_off,
                              const uint32_t* block_len, uint32_t ntables, uint8_t* out, const uint64_t* out_off,
                              uint64_t* handle_off, uint64_t* handle_size, uint64_t* out_len, int32_t* status, int mode);

#ifdef __cplusplus
}
#endif
#endif /* SNAPPY_MI355X_TABLE_H_ */
