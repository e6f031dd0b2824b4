/*
 * snappy_mi355x_kafka.h -- C ABI of libsnappy_mi355x_kafka.so: Kafka log segments (record batches of
 * magic 2, the format of .log files, fetch responses and tiered-storage objects) whose batches are
 * uncompressed or Snappy-compressed, in batches of segments on the device.  A companion of
 * libsnappy_mi355x_blocks.so (snappy_mi355x_blocks.h: the snappy-java stream), libsnappy_mi355x_multi.so
 * (snappy_mi355x_multi.h: raw streams of any length), libsnappy_mi355x_framing.so
 * (snappy_mi355x_framing.h, for its batched CRC-32C) and libsnappy_mi355x.so (snappy_mi355x.h).
 *
 * This is the batch layer and nothing above it: no record is parsed, no offset or timestamp is
 * interpreted, no index file is read.  Whole segments are transcoded both ways, and a table of the
 * batches is handed back.
 *
 * It is layered on the public entry points smb_uncompress_streams_device,
 * smb_compress_streams_device, smm_index_device, smm_uncompress_device and smf_crc32c_batch_device
 * (and, on the host, smb_index, smb_streams_plan and smf_crc32c) and links those libraries and the
 * main one by name; all five must sit in one directory.  Status codes are snappy_mi355x.h's and
 * snappy_mi355x_blocks.h's plus SMK_ERR_* below.
 *
 * ---- the format (Kafka protocol guide, "Record Batch"), and the rules ----------------------------
 * All integers are big-endian.  A segment of n bytes is a sequence of batches.  A batch at pos:
 *    0   8  baseOffset
 *    8   4  batchLength L: the bytes behind this field; the batch takes 12 + L
 *   12   4  partitionLeaderEpoch
 *   16   1  magic
 *   17   4  crc: the plain (unmasked) CRC-32C (Castagnoli) of the bytes [21, 12 + L)
 *   21   2  attributes; bits 0-2 the codec: 0 none, 1 gzip, 2 snappy, 3 lz4, 4 zstd
 *   23  38  lastOffsetDelta, baseTimestamp, maxTimestamp, producerId, producerEpoch, baseSequence,
 *           recordsCount
 *   61      the records payload, L - 49 bytes
 *
 * THE WALK runs from pos = 0:
 *   pos == n ends it (SM_OK; the empty segment is valid);
 *   fewer than 17 bytes left: SMK_ERR_TRUNCATED;
 *   magic is not 2: SMK_ERR_MAGIC (the message sets of magic 0 and 1 are refused, not guessed at);
 *   L < 49, or L negative as an int32: SMK_ERR_LENGTH;
 *   12 + L is more than the bytes left: SMK_ERR_TRUNCATED;
 *   the codec is neither 0 nor 2: SMK_ERR_CODEC;
 *   otherwise the batch is recorded and pos += 12 + L.
 * The walk stops at its first error.  valid_length is the bytes of the whole batches before it: a
 * caller holding a fetch response with a partial last batch can call again with that length.
 *
 * A BATCH'S HEAD, once the batch is known, is independent of every other batch's.  Its declared
 * length d is the length of its records once uncompressed:
 *   codec 0: stored, d = L - 49.
 *   codec 2, empty payload: d = 0.
 *   codec 2, a payload of at least 8 bytes whose first 8 are 82 53 4e 41 50 50 59 00: a snappy-java
 *     stream (what the Java clients and the broker write) under exactly the SMB_FORMAT_XERIAL walk
 *     of snappy_mi355x_blocks.h; its errors are that library's statuses, and d is the sum of its
 *     chunks' declared lengths.
 *   codec 2, anything else: one raw Snappy stream (what librdkafka-based clients write; snappy-java's
 *     reader accepts it too); d is the raw decoder's varint over the payload's first min(L - 49, 5)
 *     bytes, SM_ERR_VARINT if it does not parse.  The choice is unambiguous: no valid raw stream
 *     begins with those 8 magic bytes -- 0x82 0x53 is the varint 10626, and 0x4e is then a copy with a
 *     2-byte offset at output position 0, which every decoder refuses.
 *   d > 0x7fffffff - 49: SMK_ERR_TOO_LARGE.
 *
 * DECODE rewrites every batch as an uncompressed batch, back to back: bytes 0-7, 12-16 and 23-60
 * are copied, batchLength becomes 49 + d, the attributes keep every bit but the codec, which becomes
 * 0, the payload is the decoded (or copied) records, and crc is the CRC-32C of the new bytes
 * [21, end).  The output is a valid segment that any reader takes without a codec.  A batch is
 * rewritten to 61 + d bytes.
 *
 * STATUS ORDER FOR A SEGMENT (rules 1-7 of snappy_mi355x_table.h, for batches):
 *   1. The walk's error, else the first failing head in batch order (a snappy-java walk error,
 *      SM_ERR_VARINT, SMK_ERR_TOO_LARGE).
 *   2. A segment failing at either is not written.  d_out_len[s] = the rewritten size of the batches
 *      before the first failing head or, with none, of all batches before the walk's error.  (Those
 *      batches are in the table and count against max_batches; nothing of them is decoded.)
 *   3. A well-formed segment longer than d_out_cap[s]: SM_BUFFER_TOO_SMALL, d_out_len[s] = the size
 *      needed.  Nothing is written.
 *   4. Otherwise every batch is written at d_out_off[s] plus the rewritten sizes before it.
 *   5. With verify_crc a batch whose stored crc differs from that of its stored bytes is
 *      SMK_ERR_CRC.  The checksum covers the STORED bytes, so it is known before any decode and
 *      outranks the decoder.
 *   6. Failing that, the batch's status is the decoder's: the snappy-java stream's (its first failing
 *      chunk's), the raw decoder's, SM_OK for a stored batch.
 *   7. The segment's status is its first failing batch's, in batch order.  A failing batch does not
 *      stop the others; its payload holds unspecified bytes inside its own range, under a header and
 *      a crc that are consistent with them.
 *
 * ENCODE.  A batch of codec 0 becomes a batch of codec 2: its payload goes through the blocks
 * library's SMB_FORMAT_XERIAL encoder unchanged (the 16-byte header, then 64 KiB pieces, each a
 * 4-byte length and exactly sm_compress(piece, mode)); batchLength and the codec bits are rewritten,
 * the other 55 header bytes copied, the crc recomputed.  A batch with an empty payload becomes its
 * header alone (codec bits 2, L = 49).  A batch already of codec 2 is copied unchanged, crc included.
 * Any other codec is SMK_ERR_CODEC for the segment, found by the same walk.  decode(encode(S)) == S
 * byte for byte for every segment S of uncompressed batches with valid crcs.
 *   smk_stage_length(len)          = smb_max_length(len, SMB_FORMAT_XERIAL) rounded up to 16 (0 for
 *                                    len 0): a batch's share of the encoder's stage;
 *   smk_max_segment_length(n, nb)  = n + n / 6 + 36 (n / 65536) + 52 nb: the room an n-byte segment of
 *                                    nb batches needs.  From smb_max_length: a payload of p bytes in k
 *                                    pieces becomes at most 16 + p + p / 6 + 36 k bytes, and
 *                                    k <= p / 65536 + 1.
 *
 * Threading: an smk_ctx owns an smb_ctx, an smm_ctx, an smf_ctx and scratch, and one caller at a
 * time may use it: the *_device calls keep their per-call arrays in the ctx's scratch, so two of them
 * on one ctx must be on one stream (or ordered by the caller), and a call that grows the scratch
 * waits for the device first (hipFree).  The host-buffer calls lock the ctx.  No *_device call
 * synchronises otherwise: every decision is taken on the device.
 */
#ifndef SNAPPY_MI355X_KAFKA_H_
#define SNAPPY_MI355X_KAFKA_H_

#include <stddef.h>
#include <stdint.h>

#include "snappy_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
  SMK_ERR_TRUNCATED = 104, /* fewer than 17 bytes of a batch, or a batch that runs past the segment's end */
  SMK_ERR_MAGIC = 105,     /* a batch whose magic byte is not 2 */
  SMK_ERR_LENGTH = 106,    /* a batchLength below 49 or negative */
  SMK_ERR_CODEC = 107,     /* a batch whose codec is neither none nor snappy */
  SMK_ERR_TOO_LARGE = 108, /* a batch that declares more than 0x7fffffff - 49 bytes of records */
  SMK_ERR_CRC = 109        /* a batch's stored CRC-32C differs from that of its bytes */
};

#define SMK_BATCH_HEADER_LENGTH 61
#define SMK_CODEC_NONE 0
#define SMK_CODEC_SNAPPY 2

typedef struct smk_ctx smk_ctx;

typedef struct smk_summary {
  uint64_t total_length; /* the rewritten (uncompressed) size of the batches before the first failure */
  uint64_t valid_length; /* the bytes of the whole batches the walk recorded */
  uint32_t nbatches;     /* batches the walk recorded: all of them, or those before its error */
  int32_t status;        /* SM_OK, the walk's error, the first failing head's, or SM_BUFFER_TOO_SMALL (nbatches > max) */
} smk_summary;

/* ---- host helpers (no device needed) ------------------------------------------------- */
/* the SMK_ERR_* and SMB_ERR_* texts, else the main library's */
const char* smk_status_message(sm_status st);
/* library build identification ("snappy_mi355x_kafka gfx950 <source hash>") */
const char* smk_version(void);
/* The walk and the heads over a host buffer.  Per recorded batch k < min(nbatches, max_batches),
 * each array optional: pos[k] (from the segment's first byte), length[k] (batchLength), codec[k],
 * declared[k] (d; for a failing head what is known of it, else 0) and status[k] (the head's).
 * More batches than max_batches with an array given: SM_BUFFER_TOO_SMALL.  Returns summary->status;
 * SM_ERR_ARGUMENT for a NULL summary or buffer. */
sm_status smk_index(const uint8_t* buf, size_t n, uint64_t* pos, uint32_t* length, uint32_t* codec, uint64_t* declared,
                    int32_t* status, uint32_t max_batches, smk_summary* summary);
/* The decode plan of smk_uncompress_segments_device on the host, by the code the kernels run: per
 * segment status[s] (rules 1-3: what is known before any byte is decoded), out_len[s] and
 * first[0, nsegments] (the exclusive scan of the recorded batches).  *total_batches = the recorded
 * batches, *total_chunks = the snappy-java chunks of the batches (the device call sizes its
 * snappy-java streams with every capacity 0 first, and only a stream that declares 0 bytes takes its
 * chunks' slots then: this is the larger of the two calls' needs), *total_fragments = the larger of:
 * the sum of smm_fragment_count over those chunks; that sum over the raw batches -- all three over
 * the segments that are decoded.  out_cap NULL: no limit; every output pointer may be NULL.  More
 * batches than max_batches or more chunks than max_chunks: SM_BUFFER_TOO_SMALL, every status
 * SM_ERR_ARGUMENT and every out_len 0, as the device call leaves them. */
sm_status smk_segments_plan(const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nsegments,
                            const uint64_t* out_cap, uint32_t max_batches, uint32_t max_chunks, uint32_t* first,
                            uint64_t* out_len, int32_t* status, uint64_t* total_batches, uint64_t* total_chunks,
                            uint64_t* total_fragments);
/* The encoder's plan: per segment status[s] (the walk's error or SM_OK), room[s] =
 * smk_max_segment_length of it, first[0, nsegments]; *total_batches, *total_blocks (the 64 KiB pieces
 * of the payloads that are compressed) and *stage_bytes (the sum of smk_stage_length over them): the
 * three bounds of smk_compress_segments_device.  More batches than max_batches: SM_BUFFER_TOO_SMALL
 * and every status SM_ERR_ARGUMENT. */
sm_status smk_compress_plan(const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nsegments,
                            uint32_t max_batches, uint32_t* first, uint64_t* room, int32_t* status, uint64_t* total_batches,
                            uint64_t* total_blocks, uint64_t* stage_bytes);
uint64_t smk_max_segment_length(uint64_t n, uint64_t nbatches);
uint64_t smk_stage_length(uint64_t len);
/* the device memory a *_device call of that shape keeps in the ctx (the larger of the decoder's and
 * the encoder's needs, the stage included), the other libraries' contexts' own scratch not counted */
size_t smk_segments_scratch_bytes(uint32_t nsegments, uint32_t max_batches, uint32_t max_fragments, uint64_t stage_bytes);
/* One valid uncompressed batch around the caller's records: base_offset, partition_leader_epoch and
 * attributes (whose codec bits must be 0) as given, `tail` = the 38 bytes of the fields from
 * lastOffsetDelta to recordsCount as they stand in the batch (not interpreted), then the records;
 * batchLength and the crc (smf_crc32c) are computed.  *out_len = 61 + records_len; written when out
 * is given and out_cap suffices, else (out given) SM_BUFFER_TOO_SMALL.  SM_ERR_ARGUMENT for codec
 * bits, SM_ERR_INPUT_TOO_LARGE for more than 0x7fffffff - 49 bytes of records. */
sm_status smk_write_batch(uint64_t base_offset, uint32_t partition_leader_epoch, uint32_t attributes, const uint8_t* tail,
                          const uint8_t* records, size_t records_len, uint8_t* out, size_t out_cap, size_t* out_len);

/* ---- context ------------------------------------------------------------------------ */
/* NULL without a usable device */
smk_ctx* smk_ctx_create(int device);
void smk_ctx_destroy(smk_ctx* ctx);
/* diagnostic: the number of snappy-java chunks plus the number of raw batches the last decode call
 * took by fragments (smb_ctx_last_indexed plus smm_ctx_last_indexed); waits for the device.  -1 for
 * a NULL ctx or before the first decode. */
int smk_ctx_last_indexed(smk_ctx* ctx);

/* ---- device memory, asynchronous on `stream` (a hipStream_t; NULL = the default stream) ----
 * The offset, length and capacity arrays are trusted; the segment bytes are not.  There is no host
 * synchronisation except when the scratch grows.
 *
 * Decode.  Segment s = d_in[d_in_off[s] .. +d_in_len[s]) at any alignment, rewritten by the rules
 * above into d_out[d_out_off[s] .. +d_out_cap[s]); d_out_len[s] and d_status[s] per segment.  No
 * byte is read outside a segment's own range and none written outside its room.
 * Optional outputs (NULL: not wanted): d_batch_first (nsegments + 1); per batch (max_batches each)
 * d_batch_in_off (from the segment's first byte), d_batch_out_off (from the segment's first output
 * byte; the records alone are at + 61), d_batch_len (d), d_batch_codec and d_batch_status (0 for a
 * batch of a segment that is not written).
 * max_batches bounds the recorded batches of all segments, max_chunks the snappy-java chunks
 * (smk_segments_plan gives both).  Over either every d_status[s] = SM_ERR_ARGUMENT, every
 * d_out_len[s] = 0 and nothing is written to d_out.  max_fragments is a speed hint only, as in
 * snappy_mi355x_blocks.h: it bounds, each on its own, the fragments of the snappy-java chunks and
 * those of the raw batches; a set over it decodes in stream order, to the same bytes.
 * The pipeline: the counting walk, the scan and the storing walk, one wave per segment; the heads, a
 * thread per batch; one smb_uncompress_streams_device call over the snappy-java batches with every
 * capacity 0, which reports their sizes and decodes nothing; the scan of 61 + d, the segments'
 * plans, the slots; one smb_uncompress_streams_device call (snappy-java), smm_index_device and
 * smm_uncompress_device once (raw), one tiled copy (stored), the 61 header bytes; with verify_crc
 * one smf_crc32c_batch_device call over the input ranges; one over the output ranges and the store
 * of those four bytes; the verdicts and the results.
 * Returns SM_ERR_ARGUMENT for a NULL ctx or array, nsegments, max_batches or max_chunks above
 * 0x7fffffff; SM_ERR_DEVICE when a launch or an allocation failed. */
sm_status smk_uncompress_segments_device(smk_ctx* ctx, const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                         uint32_t nsegments, uint32_t max_batches, uint32_t max_chunks, uint32_t max_fragments,
                                         int verify_crc, uint8_t* d_out, const uint64_t* d_out_off, const uint64_t* d_out_cap,
                                         uint64_t* d_out_len, int32_t* d_status, uint32_t* d_batch_first,
                                         uint64_t* d_batch_in_off, uint64_t* d_batch_out_off, uint64_t* d_batch_len,
                                         uint32_t* d_batch_codec, int32_t* d_batch_status, void* stream);

/* Encode.  Segment s is rewritten by the encoder rule above at d_out + d_out_off[s], where
 * smk_max_segment_length(d_in_len[s], its batches) bytes must be free.  d_out_len[s] = the bytes
 * written; d_status[s] = SM_OK, the walk's error (nothing of the segment is written, d_out_len[s] =
 * 0) or SM_ERR_DEVICE (the compressor failed for one of its batches; never expected).
 * max_batches bounds the recorded batches, max_blocks the 64 KiB pieces and stage_bytes the sum of
 * smk_stage_length over the payloads that are compressed (smk_compress_plan gives all three); over
 * any of them every d_status[s] = SM_ERR_ARGUMENT, every d_out_len[s] = 0 and nothing is written to
 * d_out.  mode: SM_MODE_*.
 * The pipeline: the walks as above; the plan; one smb_compress_streams_device call into the stage;
 * the scan of the sizes; the pack (the stream, the header, the batches that pass through); one
 * smf_crc32c_batch_device call over the packed ranges and the store of those four bytes. */
sm_status smk_compress_segments_device(smk_ctx* ctx, const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                       uint32_t nsegments, uint32_t max_batches, uint32_t max_blocks, uint64_t stage_bytes,
                                       uint8_t* d_out, const uint64_t* d_out_off, uint64_t* d_out_len, int32_t* d_status,
                                       int mode, void* stream);

/* ---- host memory (one upload, the device path, one download; synchronous; lock the ctx) ----
 * The arrays as above, in host memory; the bounds are counted here with the two plans.  Only each
 * segment's own range out[out_off .. +out_len) is written, and only when out_len fits its capacity.
 * smk_uncompress_segments: batch_first (nsegments + 1) and the five per-batch arrays are optional,
 * all or none, with room for max_entries entries; more entries than that: SM_BUFFER_TOO_SMALL.
 * smk_compress_segments: out_cap[s] must be at least the plan's room[s], else SM_ERR_ARGUMENT. */
sm_status smk_uncompress_segments(smk_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len,
                                  uint32_t nsegments, int verify_crc, uint8_t* out, const uint64_t* out_off,
                                  const uint64_t* out_cap, uint64_t* out_len, int32_t* status, uint32_t* batch_first,
                                  uint32_t max_entries, uint64_t* batch_in_off, uint64_t* batch_out_off, uint64_t* batch_len,
                                  uint32_t* batch_codec, int32_t* batch_status);
sm_status smk_compress_segments(smk_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len,
                                uint32_t nsegments, uint8_t* out, const uint64_t* out_off, const uint64_t* out_cap,
                                uint64_t* out_len, int32_t* status, int mode);

#ifdef __cplusplus
}
#endif
#endif /* SNAPPY_MI355X_KAFKA_H_ */
