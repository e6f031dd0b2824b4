/*
 * snappy_mi355x_avro.h -- C ABI of libsnappy_mi355x_avro.so: Avro object container files whose
 * avro.codec is snappy, in batches on the device.  A companion of libsnappy_mi355x_multi.so
 * (snappy_mi355x_multi.h), libsnappy_mi355x_parquet.so (snappy_mi355x_parquet.h, for its batched
 * CRC-32) and libsnappy_mi355x.so (snappy_mi355x.h).
 *
 * This is the container layer and nothing above it: no Avro record is parsed and no schema is
 * interpreted.  The library deals in blocks of serialized bytes and their object counts.  Files of
 * any other codec (null, deflate, bzip2, xz, zstandard) are refused, not guessed at.
 *
 * It is layered on the public entry points smm_index_device, smm_uncompress_device,
 * smm_compress_device and smq_crc32_device and links those libraries and the main one by name; all
 * four must sit in one directory.  Status codes are snappy_mi355x.h's plus SMA_ERR_* below.
 *
 * ---- the format, and the one walk --------------------------------------------------------------
 * A LONG is a zigzag varint: up to 10 bytes, little-endian 7-bit groups, v = (u >> 1) ^ -(u & 1).
 * A 10th byte above 1 (a 10th byte with the continuation bit included): SMA_ERR_VARLONG.  Running
 * past the stream's end: SMA_ERR_TRUNCATED.
 *
 * The file header (input kind SMA_INPUT_FILE), over the n bytes of a stream:
 *   n == 0, or the bytes present of the first 4 differ from 4f 62 6a 01 ("Obj\1"):
 *     SMA_ERR_NO_HEADER; a matching prefix with n < 4: SMA_ERR_TRUNCATED.
 *   Then the metadata map.  Repeat: c = long.  c == 0 ends the map.  c < 0: c = -c (the one value
 *     that cannot be negated is SMA_ERR_BAD_HEADER), and a long byte size follows; a negative one is
 *     SMA_ERR_BAD_HEADER, otherwise it is ignored.  Then c pairs of key (long length, bytes) and
 *     value (long length, bytes): a negative length is SMA_ERR_BAD_HEADER, a length past the end
 *     SMA_ERR_TRUNCATED.  A key equal to the 10 bytes "avro.codec" records whether its value is the
 *     6 bytes "snappy"; the last such key wins.  The loop needs no count bound: every pair consumes
 *     at least two bytes.
 *   Behind the map come 16 bytes of sync marker; fewer left: SMA_ERR_TRUNCATED.
 *   Then, if no avro.codec was seen or its value is not snappy: SMA_ERR_CODEC.
 *
 * A block run (input kind SMA_INPUT_BLOCKS): no header.  The 16-byte marker comes from the caller
 * (sync + 16 * s) and the walk starts at the stream's first byte.  This is what a split reader has
 * behind sma_find_sync_device.
 *
 * The blocks, from pos with total = 0 and objects = 0:
 *   pos == n ends the walk (SM_OK): a header followed by no block is a valid empty file.
 *   count = long; negative: SMA_ERR_BLOCK.
 *   size = long; negative or below 4 (no room for the checksum): SMA_ERR_BLOCK.
 *   With rest = the bytes behind the two longs: size > rest, or rest - size < 16: SMA_ERR_TRUNCATED.
 *   size - 4 > 0x7fffffff: SMA_ERR_TOO_LARGE.
 *   The 16 bytes at pos + size differ from the marker: SMA_ERR_SYNC.
 *   The payload is the first size - 4 bytes, one raw Snappy stream; its declared length d is the
 *     raw decoder's varint over its first min(size - 4, 5) bytes.  It does not parse (an empty
 *     payload included): SM_ERR_VARINT.  d > 0x7fffffff: SMA_ERR_TOO_LARGE.
 *   The stored checksum is the big-endian u32 at pos + size - 4: the CRC-32 (IEEE: reflected
 *     polynomial 0xEDB88320, init and final xor 0xffffffff; "123456789" gives 0xCBF43926) of the
 *     block's UNCOMPRESSED bytes.
 *   The block is recorded (pay_off, pay_len = size - 4, ulen = d, count, crc, its output at total);
 *     total += d, objects += count (saturating), pos moves behind the marker.
 *
 * The encoder: every block's payload is exactly sm_compress(block, mode); a block takes
 * len(long(count)) + len(long(clen + 4)) + clen + 4 + 16 bytes.
 *
 * Threading: an sma_ctx owns an smm_ctx, an smq_ctx and scratch, and one caller at a time may use
 * it: the *_device calls keep their per-call arrays in the ctx's scratch, so two of them on one ctx
 * must be on one stream (or ordered by the caller), and a call that grows the scratch waits for the
 * device first (hipFree).  sma_compress_streams / sma_uncompress_streams lock the ctx.  No *_device
 * call synchronises otherwise: every decision is taken on the device.
 */
#ifndef SNAPPY_MI355X_AVRO_H_
#define SNAPPY_MI355X_AVRO_H_

#include <stddef.h>
#include <stdint.h>

#include "snappy_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SMA_INPUT_FILE = 0, SMA_INPUT_BLOCKS = 1 };

enum {
  SMA_ERR_NO_HEADER = 80,  /* the stream is empty or does not start with "Obj\1" */
  SMA_ERR_BAD_HEADER = 81, /* the metadata map has a count that cannot be negated or a negative size or length */
  SMA_ERR_TRUNCATED = 82,  /* a long, the header, a payload or a marker runs past the end of the stream */
  SMA_ERR_VARLONG = 83,    /* a long of more than 64 bits */
  SMA_ERR_CODEC = 84,      /* the header's avro.codec is missing or is not snappy */
  SMA_ERR_BLOCK = 85,      /* a block with a negative count, or a size that is negative or leaves no room for the checksum */
  SMA_ERR_TOO_LARGE = 86,  /* a payload or its declared length above 0x7fffffff bytes */
  SMA_ERR_SYNC = 87,       /* the 16 bytes behind a block are not the sync marker */
  SMA_ERR_CRC = 88         /* a block's decoded bytes do not have the stored CRC-32 */
};

#define SMA_SYNC_LENGTH 16

typedef struct sma_ctx sma_ctx;

/* a stream's blocks, as parallel arrays (host memory for sma_index, device memory for the device call) */
typedef struct sma_blocks {
  uint64_t* pay_off; /* the payload (a raw Snappy stream), from the stream's first byte */
  uint32_t* pay_len;
  uint32_t* ulen;    /* the length the payload's varint declares */
  uint64_t* count;   /* the block's objects */
  uint32_t* crc;     /* the stored CRC-32 of the uncompressed bytes */
  uint64_t* out_off; /* the block's output, from the stream's first output byte */
} sma_blocks;

typedef struct sma_summary {
  uint64_t total_length;  /* the declared lengths: of the whole stream, or before the error */
  uint32_t nblocks;       /* blocks recorded: all of them, or those before the error */
  int32_t status;         /* SM_OK, a walk error, or SM_BUFFER_TOO_SMALL (nblocks > max_blocks) */
  uint64_t objects;       /* the counts of the recorded blocks (saturating) */
  uint64_t header_length; /* SMA_INPUT_FILE: the bytes in front of the first block; 0 when the header failed */
  uint8_t sync[SMA_SYNC_LENGTH]; /* the marker: the header's (zeros when it failed), or the caller's */
} sma_summary;

/* ---- host helpers (no device needed) ------------------------------------------------- */
/* the SMA_ERR_* texts, else the main library's */
const char* sma_status_message(sm_status st);
/* library build identification ("snappy_mi355x_avro gfx950 <source hash>") */
const char* sma_version(void);
/* the most blocks n bytes can hold: n / 23.  The shortest block is a one-byte count, a one-byte
 * size, a payload of one byte (the empty raw stream) with its 4-byte checksum, and the 16-byte
 * marker: 1 + 1 + 5 + 16 bytes.  (A header only lowers the number.) */
uint64_t sma_max_blocks(uint64_t n);
/* the encoder's bound for a block of len bytes: sm_max_compressed_length(len) + 40 (two longs of
 * at most 10 bytes, the checksum, the marker); a stream's bound is its header plus the sum */
uint64_t sma_max_block_length(uint64_t len);
/* a block's share of the encoder's stage: sm_max_compressed_length(len) rounded up to 16 */
uint64_t sma_stage_length(uint64_t len);
/* The walk over a host buffer.  kind: SMA_INPUT_*; sync: the caller's marker (SMA_INPUT_BLOCKS),
 * NULL for a file.  blocks NULL: count only.  Entries [0, min(nblocks, max_blocks)) are stored;
 * more blocks than max_blocks with blocks given: SM_BUFFER_TOO_SMALL.  Returns summary->status;
 * SM_ERR_ARGUMENT for a NULL summary or buffer, an unknown kind or a block run without a marker. */
sm_status sma_index(const uint8_t* buf, size_t n, int kind, const uint8_t* sync, const sma_blocks* blocks,
                    uint32_t max_blocks, sma_summary* summary);
sm_status sma_uncompressed_length(const uint8_t* buf, size_t n, int kind, const uint8_t* sync, size_t* result);
/* The decode plan of sma_uncompress_streams_device on the host, by the code the kernels run: per
 * stream status[s] (the walk's error, SM_BUFFER_TOO_SMALL against out_cap[s], or SM_OK: what is known
 * before any byte is decoded), out_len[s] (the size needed, or the declared lengths before the
 * error), objects[s] and first[0, nstreams] (the exclusive scan of the slots: a stream that is
 * decoded takes one per block, any other none).  *total_blocks = the slots, *total_fragments = the
 * sum of smm_fragment_count(ulen) over them: the two bounds of the device call.  sync: 16 bytes per
 * stream (SMA_INPUT_BLOCKS), else NULL.  out_cap NULL: no limit; every output pointer may be NULL.
 * More slots than max_blocks: SM_BUFFER_TOO_SMALL, every status SM_ERR_ARGUMENT and every out_len
 * and objects 0, as the device call leaves them. */
sm_status sma_streams_plan(const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nstreams, int kind,
                           const uint8_t* sync, const uint64_t* out_cap, uint32_t max_blocks, uint32_t* first,
                           uint64_t* out_len, int32_t* status, uint64_t* objects, uint64_t* total_blocks,
                           uint64_t* total_fragments);
/* the device memory a *_streams_device call of that shape keeps in the ctx (the larger of the two
 * calls' needs, the encoder's stage of stage_bytes included), the smm_ctx's and the smq_ctx's own
 * scratch not counted */
size_t sma_streams_scratch_bytes(uint32_t nstreams, uint32_t max_blocks, uint32_t max_fragments, uint64_t stage_bytes);
/* The sync search on the host, by the device call's rule: pos[i] = the least p >= q_from[i] with
 * p + 16 <= in_len[s] and stream s = q_stream[i] holding its marker sync[16 s ..) at p, else
 * in_len[s].  pos + 16 is where a block run starts. */
sm_status sma_find_sync(const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, const uint8_t* sync,
                        uint32_t nstreams, const uint32_t* q_stream, const uint64_t* q_from, uint32_t nqueries,
                        uint64_t* pos);
/* A file header: "Obj\1", one map block of 2 + npairs pairs -- avro.schema = schema, avro.codec =
 * snappy, then the caller's pairs (key i = extra[extra_off[2 i] .. extra_off[2 i + 1]), value i =
 * extra[extra_off[2 i + 1] .. extra_off[2 i + 2])) -- the map's end and the marker.  *out_len = its
 * size; written when out is given and out_cap suffices, else (out given) SM_BUFFER_TOO_SMALL. */
sm_status sma_write_header(const uint8_t* schema, size_t schema_len, const uint8_t* extra, const uint64_t* extra_off,
                           uint32_t npairs, const uint8_t* sync, uint8_t* out, size_t out_cap, size_t* out_len);

/* ---- context ------------------------------------------------------------------------ */
/* NULL without a usable device */
sma_ctx* sma_ctx_create(int device);
void sma_ctx_destroy(sma_ctx* ctx);
/* diagnostic: smm_ctx_last_indexed of the ctx's smm_ctx -- the number of blocks the last decode
 * call took by fragments; waits for the device.  -1 for a NULL ctx or before the first decode. */
int sma_ctx_last_indexed(sma_ctx* ctx);

/* ---- device memory, asynchronous on `stream` (a hipStream_t; NULL = the default stream) ----
 * The offset, length and capacity arrays are trusted; the stream bytes are not.
 *
 * Decode.  Stream s = d_in[d_in_off[s] .. +d_in_len[s]) at any alignment, of `kind` (with
 * SMA_INPUT_BLOCKS its marker at d_sync + 16 s; d_sync may be NULL for files), into
 * d_out[d_out_off[s] .. +d_out_cap[s]).  Per stream:
 *   a walk error: d_status[s] = that status, d_out_len[s] = the declared lengths before the error;
 *     nothing of it is decoded and it takes no slots;
 *   well formed but longer than d_out_cap[s]: SM_BUFFER_TOO_SMALL, d_out_len[s] = the size needed;
 *     nothing is decoded;
 *   otherwise every block takes a slot and decodes, with capacity exactly its declared length, to
 *     d_out_off[s] plus the declared lengths before it.  A block's status is the raw decoder's when
 *     that is not SM_OK; otherwise, when verify_crc is not 0, SMA_ERR_CRC where the CRC-32 of the
 *     decoded bytes differs from the stored one (the checksum covers the output, so the decoder's
 *     verdict comes first).  d_status[s] = the first failing block's status in block order, else
 *     SM_OK (a failing block does not stop the others); d_out_len[s] = the total.
 * d_objects (optional): d_objects[s] = the sum of the counts of the blocks the walk recorded.
 * No byte is read outside a stream's own input range and none written outside
 * [d_out_off[s], d_out_off[s] + d_out_cap[s]).
 * max_blocks: the caller's bound on the slots (sma_streams_plan, or sma_max_blocks summed); it
 * sizes the launches and the scratch.  When the device counts more, every d_status[s] =
 * SM_ERR_ARGUMENT, every d_out_len[s] and d_objects[s] = 0 and nothing is written to d_out.
 * d_block_first (nstreams + 1) and d_block_status (max_blocks), both or neither: the exclusive scan
 * of the slots, and per slot its status (0 for a slot no block took).
 * d_blocks (optional): device arrays of max_blocks entries each, filled per slot with the block's
 * fields (offsets from the stream's first byte and its first output byte; zeros for a slot no block
 * took).
 * max_fragments is a speed hint only, as in snappy_mi355x_blocks.h: the slots go through
 * smm_index_device with that bound (0: no index is built) and then through smm_uncompress_device,
 * so a block of more than 64 KiB that a block compressor wrote decodes fragment by fragment.
 * There is no host synchronisation except when the scratch grows.
 * Returns SM_ERR_ARGUMENT for a NULL ctx or array, an unknown kind, a block run without d_sync,
 * one of d_block_first / d_block_status without the other, a NULL array in d_blocks, nstreams or
 * max_blocks above 0x7fffffff; SM_ERR_DEVICE when a launch or an allocation failed. */
sm_status sma_uncompress_streams_device(sma_ctx* ctx, int kind, const uint8_t* d_in, const uint64_t* d_in_off,
                                        const uint64_t* d_in_len, const uint8_t* d_sync, uint32_t nstreams,
                                        uint32_t max_blocks, uint32_t max_fragments, int verify_crc, uint8_t* d_out,
                                        const uint64_t* d_out_off, const uint64_t* d_out_cap, uint64_t* d_out_len,
                                        int32_t* d_status, uint64_t* d_objects, uint32_t* d_block_first,
                                        const sma_blocks* d_blocks, int32_t* d_block_status, void* stream);

/* Split reading.  Query i: d_pos[i] = the position of the first occurrence of stream s =
 * d_q_stream[i]'s marker (d_sync + 16 s) at or after d_q_from[i] in d_in[d_in_off[s] ..
 * +d_in_len[s]), or d_in_len[s] where there is none (a marker must lie wholly inside the stream).
 * A grid runs over 64 KiB tiles of the searched ranges; a tile also looks 15 bytes into the next,
 * so a marker across a tile edge is found by exactly one tile; candidates are compared 16 bytes at
 * a time and the minimum goes through a 64-bit atomic min per query.  d_pos[i] + 16 is where a
 * block run starts.  No byte outside a stream's range is read. */
sm_status sma_find_sync_device(sma_ctx* ctx, const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                               const uint8_t* d_sync, uint32_t nstreams, const uint32_t* d_q_stream,
                               const uint64_t* d_q_from, uint32_t nqueries, uint64_t* d_pos, void* stream);

/* Compress.  Stream s is made of the blocks d_block_first[s] .. d_block_first[s + 1] of the flat
 * arrays: block j = d_in[d_block_off[j] .. +d_block_len[j]), serialized records holding
 * d_block_count[j] objects (at most 0x7fffffffffffffff).  At d_out + d_out_off[s]: the header range
 * d_in[d_head_off[s] .. +d_head_len[s]) copied verbatim (trusted, not checked; d_head_off and
 * d_head_len both NULL: none, a block run), then every block by the encoder rule above with the
 * marker d_sync + 16 s.  The room there must be d_head_len[s] plus the sum of
 * sma_max_block_length(d_block_len[j]).  d_out_len[s] = the size; d_status[s] = SM_OK, or
 * SM_ERR_INPUT_TOO_LARGE (a block above 0x7fffffff bytes) or SM_ERR_DEVICE (the raw compressor left
 * an error mark; never expected): the stream is then unusable.
 * The checksums come from one smq_crc32_device call over the input blocks.
 * max_blocks bounds d_block_first[nstreams], stage_bytes the sum of sma_stage_length(d_block_len[j]),
 * max_fragments the sum of smm_fragment_count(d_block_len[j]) over the blocks of more than 64 KiB;
 * over any of them every d_status[s] = SM_ERR_ARGUMENT, every d_out_len[s] = 0 and nothing is
 * written to d_out.  mode: SM_MODE_*. */
sm_status sma_compress_streams_device(sma_ctx* ctx, const uint8_t* d_in, const uint32_t* d_block_first,
                                      const uint64_t* d_block_off, const uint32_t* d_block_len,
                                      const uint64_t* d_block_count, const uint8_t* d_sync, const uint64_t* d_head_off,
                                      const uint64_t* d_head_len, uint32_t nstreams, uint32_t max_blocks,
                                      uint64_t stage_bytes, uint32_t max_fragments, uint8_t* d_out,
                                      const uint64_t* d_out_off, uint64_t* d_out_len, int32_t* d_status, int mode,
                                      void* stream);

/* ---- host memory (one upload, the device path, one download; synchronous; lock the ctx) ----
 * The arrays as above, in host memory; the bounds are counted here.  Only each stream's own bytes
 * are copied back: out is otherwise untouched. */
sm_status sma_uncompress_streams(sma_ctx* ctx, int kind, const uint8_t* in, const uint64_t* in_off,
                                 const uint64_t* in_len, const uint8_t* sync, uint32_t nstreams, int verify_crc,
                                 uint8_t* out, const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len,
                                 int32_t* status, uint64_t* objects);
sm_status sma_compress_streams(sma_ctx* ctx, const uint8_t* in, const uint32_t* block_first, const uint64_t* block_off,
                               const uint32_t* block_len, const uint64_t* block_count, const uint8_t* sync,
                               const uint64_t* head_off, const uint64_t* head_len, uint32_t nstreams, uint8_t* out,
                               const uint64_t* out_off, uint64_t* out_len, int32_t* status, int mode);

#ifdef __cplusplus
}
#endif
#endif /* SNAPPY_MI355X_AVRO_H_ */
