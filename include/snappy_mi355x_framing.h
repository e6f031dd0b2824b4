/*
 * snappy_mi355x_framing.h -- C ABI of the Snappy framing format on the MI355X (gfx950),
 * libsnappy_mi355x_framing.so: a companion of libsnappy_mi355x.so (snappy_mi355x.h), which it
 * links by name and whose public batched device entry points it calls for the raw codec.
 *
 * The framing format (framing_format.txt of google/snappy; what .sz files, snzip and Go's
 * snappy.Writer produce) is a sequence of chunks: one type byte, a 3-byte little-endian length
 * of the data that follows, then the data.
 *   0xff  stream identifier: length 6, data "sNaPpY".  The stream starts with it; it may occur
 *         again (concatenated streams) and is then checked and skipped.
 *   0x00  compressed data: a 4-byte LE masked CRC-32C of the UNCOMPRESSED bytes, then one raw
 *         Snappy stream (varint + body) of at most 65536 uncompressed bytes.
 *   0x01  uncompressed data: the same CRC field, then at most 65536 bytes.
 *   0xfe  padding, 0x80..0xfd reserved skippable: the data is skipped.
 *   0x02..0x7f reserved unskippable: an error.
 * CRC-32C: reflected polynomial 0x82F63B78, init and final xor 0xffffffff; the stored value is
 * masked: ((crc >> 15) | (crc << 17)) + 0xa282ead8 mod 2^32.
 *
 * Encoder rule (fixed, so the output is deterministic): the input is cut into 64 KiB blocks; a
 * block becomes a 0x00 chunk if and only if its Snappy stream is strictly shorter than the
 * block, else a 0x01 chunk; the empty input is the identifier alone.
 *
 * Statuses: the codes of snappy_mi355x.h plus SMF_ERR_* (48..53).  A corrupt Snappy payload
 * keeps the raw decoder's SM_ERR_* code.  A decode's overall status is the first failing
 * chunk's in stream order; the other chunks still decode and report SM_OK.
 *
 * Threading: an smf_ctx owns one sm_ctx (device, stream) and scratch.  The host-buffer entry
 * points lock the ctx.  The *_device entry points launch on the caller's stream and use the
 * ctx's scratch without a lock: one caller per ctx at a time, and calls on one ctx go to one
 * stream (or are ordered by the caller), since consecutive calls reuse the scratch.
 */
#ifndef SNAPPY_MI355X_FRAMING_H_
#define SNAPPY_MI355X_FRAMING_H_

#include <stddef.h>
#include <stdint.h>

#include "snappy_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
  SMF_ERR_NO_IDENTIFIER = 48,   /* the stream does not start with a 0xff chunk (or is empty) */
  SMF_ERR_BAD_IDENTIFIER = 49,  /* a 0xff chunk whose length is not 6 or whose data is not "sNaPpY" */
  SMF_ERR_RESERVED_CHUNK = 50,  /* an unskippable reserved chunk type, 0x02..0x7f */
  SMF_ERR_TRUNCATED = 51,       /* a chunk header or its data runs past the end of the stream, or a
                                   data chunk has no room for its CRC (length < 4) */
  SMF_ERR_CHUNK_TOO_LARGE = 52, /* a data chunk of more than 65536 uncompressed bytes */
  SMF_ERR_CRC = 53              /* the chunk's bytes do not have the stored CRC-32C */
};

#define SMF_CHUNK_COMPRESSED 0x00u
#define SMF_CHUNK_UNCOMPRESSED 0x01u
#define SMF_IDENTIFIER_LENGTH 10u

typedef struct smf_ctx smf_ctx;

/* The index of a framed stream: one entry per DATA chunk (0x00 / 0x01), in stream order.  Five
 * parallel arrays of at least max_chunks entries, all in host memory (smf_index) or all in device
 * memory (the *_device calls). */
typedef struct smf_chunks {
  uint8_t* type;      /* SMF_CHUNK_COMPRESSED or SMF_CHUNK_UNCOMPRESSED */
  uint64_t* pay_off;  /* offset in the stream of the payload (the bytes behind the CRC field) */
  uint32_t* pay_len;  /* its length: the chunk length - 4 */
  uint32_t* crc;      /* the stored (masked) CRC */
  uint32_t* ulen;     /* declared uncompressed length: the payload's varint (0x00), pay_len (0x01) */
} smf_chunks;

/* What a walk found.  status: SM_OK, the first structural error (the walk stops there; nchunks
 * and total_length then cover the data chunks before it), or SM_BUFFER_TOO_SMALL when the stream
 * is well formed but has more than max_chunks data chunks (nchunks = the count needed; the first
 * max_chunks entries are filled). */
typedef struct smf_summary {
  uint64_t total_length; /* the sum of the declared uncompressed lengths */
  uint32_t nchunks;      /* data chunks */
  int32_t status;
} smf_summary;

/* Message for a status code: the SMF_ERR_* texts, else the companion library's message. */
const char* smf_status_message(sm_status st);
/* library build identification ("snappy_mi355x_framing gfx950 <source hash>") */
const char* smf_version(void);

/* ---- format helpers (host, no device needed) ------------------------------------ */
/* The largest framed stream of an n-byte input under the encoder rule:
 * 10 + 8 * ceil(n / 65536) + n. */
size_t smf_max_framed_length(size_t n);
/* CRC-32C of a host buffer (unmasked), and the mask. */
uint32_t smf_crc32c(const void* buf, size_t n);
uint32_t smf_crc32c_mask(uint32_t crc);
/* Walks a framed stream in HOST memory.  chunks may be NULL (max_chunks is then ignored: count
 * and total only).  Returns summary->status (SM_ERR_ARGUMENT for a NULL summary or buffer). */
sm_status smf_index(const uint8_t* buf, size_t n, const smf_chunks* chunks, uint32_t max_chunks,
                    smf_summary* summary);
/* The stream's total uncompressed length, from its chunk headers alone (no CRC or payload check). */
sm_status smf_uncompressed_length(const uint8_t* buf, size_t n, size_t* result);

/* ---- the seek index (host helpers, no device needed) ------------------------------- */
/* The seek index of a framed stream is its smf_chunks arrays plus chunk_off: nchunks + 1 u64, the
 * exclusive scan of ulen, so chunk c holds bytes [chunk_off[c], chunk_off[c + 1]) of the
 * uncompressed content and chunk_off[nchunks] is the total length.
 * smf_chunk_offsets fills chunk_off from ulen (host arrays). */
sm_status smf_chunk_offsets(const uint32_t* ulen, uint32_t nchunks, uint64_t* chunk_off);
/* The chunks that bytes [lo, lo + len) touch in a stream of full 64 KiB chunks:
 * floor((lo + len - 1) / 65536) - floor(lo / 65536) + 1, or 0 for len == 0 (and for lo + len
 * overflowing).  Exact for streams of this library's encoder.  A foreign stream may have smaller
 * or empty chunks, so a range of it may touch more: there the caller bounds max_range_chunks
 * itself (smf_range_plan counts, or nchunks per range always suffices). */
uint64_t smf_range_chunk_count(uint64_t lo, uint64_t len);
/* The plan of smf_uncompress_ranges_device over HOST arrays, by the rules the device runs: for
 * range r, first[r] / count[r] = the chunks [first, first + count) that get a slot (from the chunk
 * holding lo to the chunk holding lo + len - 1; empty chunks in between keep their slot and are
 * passed over), and status[r] = SM_OK, SM_ERR_ARGUMENT for a range that leaves the stream, or
 * SM_ERR_ARGUMENT for a touched entry that fails its checks (below) -- what is known before any
 * byte is decoded.  *total = the sum of the counts.  n = the framed stream's length.  Returns
 * SM_OK, or SM_BUFFER_TOO_SMALL when *total > max_range_chunks (every status[r] is then
 * SM_ERR_ARGUMENT, as on the device).  first / count / status / total may each be NULL. */
sm_status smf_range_plan(const smf_chunks* chunks, const uint64_t* chunk_off, uint32_t nchunks, uint64_t n,
                         const uint64_t* lo, const uint64_t* len, uint32_t nranges, uint32_t max_range_chunks,
                         uint32_t* first, uint32_t* count, int32_t* status, uint64_t* total);
/* Bytes of ctx scratch a smf_uncompress_ranges_device call with these bounds needs: the per-slot
 * arrays and 2 * nranges edge slots of 65536 bytes. */
size_t smf_range_scratch_bytes(uint32_t nranges, uint32_t max_range_chunks);

/* ---- a batch of streams per call (host helpers, no device needed) ------------------- */
/* The most data chunks an n-byte framed stream can hold: 0 for n < 10, else (n - 10) / 8 -- the
 * identifier takes 10 bytes and a data chunk 8 at the least (an empty 0x01 chunk).  It bounds
 * max_chunks for foreign streams of unknown content; a caller who knows a stream's uncompressed
 * length should use ceil(length / 65536) for this library's streams, which is far smaller. */
uint64_t smf_max_data_chunks(uint64_t n);
/* The plan of smf_uncompress_streams_device over HOST arrays, by the rules the device runs: stream s
 * is in[in_off[s], in_off[s] + in_len[s]) with out_cap[s] bytes of room (out_cap == NULL: no
 * limit).  It fills what is known before any byte is decoded: status[s] = the walk's structural
 * error, SM_BUFFER_TOO_SMALL for a well-formed stream longer than out_cap[s], or SM_OK;
 * out_len[s] = the declared lengths of the data chunks before the error, else of all of them (the
 * size needed); first[0, nstreams] = the exclusive scan of the slots -- a stream's data chunks when
 * its status is SM_OK, else 0; *total = their sum.  No byte outside a stream's own range is read.
 * Returns SM_OK, or SM_BUFFER_TOO_SMALL when *total > max_chunks (every status[s] is then
 * SM_ERR_ARGUMENT and every out_len[s] 0, as on the device).  first / out_len / status / total may
 * each be NULL. */
sm_status smf_streams_plan(const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nstreams,
                           const uint64_t* out_cap, uint32_t max_chunks, uint32_t* first, uint64_t* out_len,
                           int32_t* status, uint64_t* total);
/* Bytes of ctx scratch that a smf_uncompress_streams_device or smf_compress_streams_device call of
 * nstreams streams and max_slots slots (max_chunks / max_blocks) keeps, the larger of the two: the
 * per-stream and per-slot arrays and, for compress, the raw compressor's output slots. */
size_t smf_streams_scratch_bytes(uint32_t nstreams, uint32_t max_slots);

/* ---- context ---------------------------------------------------------------------- */
/* NULL without a usable device. */
smf_ctx* smf_ctx_create(int device);
void smf_ctx_destroy(smf_ctx* ctx);

/* ---- device memory (the GPU hot path) ------------------------------------------------ */
/* Block b: d_crc[b] = CRC-32C of d_in[d_off[b] .. +d_len[b]), masked when masked != 0.  Any
 * length (0 gives 0, masked 0xa282ead8) and any source alignment; reads stay inside the 16-byte-
 * aligned granules that hold the block's bytes, and of a granule the block only partly covers only
 * the block's own bytes are read.  Asynchronous on `stream`. */
sm_status smf_crc32c_batch_device(smf_ctx* ctx, const uint8_t* d_in, const uint64_t* d_off, const uint32_t* d_len,
                                  uint32_t nblk, uint32_t* d_crc, int masked, void* stream);

/* Frames d_in[0, n) into d_out: the identifier, then one chunk per 64 KiB block (encoder rule
 * above).  *d_out_len (device, u64) = the stream's length; *d_status (device) = SM_OK, or
 * SM_ERR_DEVICE when the compressor returned an error mark for a block (nothing is packed for that
 * block; never expected).  out_capacity < smf_max_framed_length(n) returns SM_BUFFER_TOO_SMALL
 * and launches nothing.  mode: SM_MODE_*.  Asynchronous on `stream`, except when the ctx's
 * scratch has to grow (first call, or a larger n than any before: hipMalloc). */
sm_status smf_compress_device(smf_ctx* ctx, const uint8_t* d_in, uint64_t n, uint8_t* d_out, uint64_t out_capacity,
                              uint64_t* d_out_len, int32_t* d_status, int mode, void* stream);

/* smf_index for a stream that lives in DEVICE memory: one wave walks the chunk chain (serial: a
 * chunk's position is known only from its predecessor's length).  d_chunks points to a HOST
 * struct of DEVICE arrays (NULL: count only); *d_summary is in device memory.  Asynchronous. */
sm_status smf_index_device(smf_ctx* ctx, const uint8_t* d_in, uint64_t n, const smf_chunks* d_chunks,
                           uint32_t max_chunks, smf_summary* d_summary, void* stream);
/* *d_len (device, u64) = the total uncompressed length, *d_status (device) = the walk's status. */
sm_status smf_uncompressed_length_device(smf_ctx* ctx, const uint8_t* d_in, uint64_t n, uint64_t* d_len,
                                         int32_t* d_status, void* stream);

/* Decodes the nchunks data chunks of an indexed stream (d_chunks: a HOST struct of DEVICE arrays,
 * as smf_index_device fills them) into d_out, chunk c at the sum of the declared lengths before
 * it: 0x00 chunks by the raw batched decoder with capacity = the declared length, 0x01 chunks by a
 * copy kernel; then the CRC of every chunk's output is recomputed and compared.
 * d_chunk_status[c] (device, nchunks) = SM_OK, the raw decoder's SM_ERR_* code, SMF_ERR_CRC,
 * SMF_ERR_CHUNK_TOO_LARGE (a declared length over 65536, or a 0x01 chunk whose lengths differ), or
 * SM_BUFFER_TOO_SMALL (the chunk would end past out_capacity; it is not decoded).
 * *d_status (device) = the first failing chunk's status in stream order, else SM_OK;
 * *d_out_len (device, u64) = the sum of the declared lengths (the size needed).
 * Asynchronous on `stream`, except when the ctx's scratch has to grow. */
sm_status smf_uncompress_chunks_device(smf_ctx* ctx, const uint8_t* d_in, const smf_chunks* d_chunks,
                                       uint32_t nchunks, uint8_t* d_out, uint64_t out_capacity,
                                       int32_t* d_chunk_status, uint64_t* d_out_len, int32_t* d_status, void* stream);

/* Index plus decode of a stream in device memory.  ONE host synchronisation of `stream`, between
 * the index walk and the decode (the host needs the chunk count to size the launches); a second
 * one when the stream has more chunks than the ctx's index scratch held (it grows, and the walk
 * runs again).  Returns, and stores in *d_status, the walk's structural error, or
 * SM_BUFFER_TOO_SMALL when out_capacity is less than the total length (*d_out_len = the size
 * needed; nothing is decoded); otherwise returns SM_OK with the decode queued on `stream`, and
 * *d_status / *d_out_len are those of smf_uncompress_chunks_device. */
sm_status smf_uncompress_device(smf_ctx* ctx, const uint8_t* d_in, uint64_t n, uint8_t* d_out, uint64_t out_capacity,
                                uint64_t* d_out_len, int32_t* d_status, void* stream);

/* d_chunk_off[0, nchunks] (device) = the exclusive scan of d_ulen[0, nchunks) (device): completes
 * an index that smf_index_device produced, of a foreign stream too.  One kernel, asynchronous. */
sm_status smf_chunk_offsets_device(smf_ctx* ctx, const uint32_t* d_ulen, uint32_t nchunks, uint64_t* d_chunk_off,
                                   void* stream);

/* smf_compress_device that also hands out the seek index of the stream it packs, so that nobody
 * has to walk it: the framed bytes, *d_out_len and *d_status are exactly smf_compress_device's;
 * d_chunks (a HOST struct of DEVICE arrays of max_chunks entries), d_chunk_off (device,
 * max_chunks + 1) and *d_nchunks (device) receive what smf_index_device followed by
 * smf_chunk_offsets_device would give for it, entry for entry.  max_chunks < ceil(n / 65536)
 * returns SM_BUFFER_TOO_SMALL and launches nothing.  With *d_status = SM_ERR_DEVICE the index is
 * unspecified and *d_nchunks = 0.  No host synchronisation (scratch growth as smf_compress_device). */
sm_status smf_compress_indexed_device(smf_ctx* ctx, const uint8_t* d_in, uint64_t n, uint8_t* d_out,
                                      uint64_t out_capacity, uint64_t* d_out_len, int32_t* d_status, int mode,
                                      const smf_chunks* d_chunks, uint64_t* d_chunk_off, uint32_t max_chunks,
                                      uint32_t* d_nchunks, void* stream);

/* Ranged decode, batched: range r asks for bytes [d_lo[r], d_lo[r] + d_len[r]) of the uncompressed
 * content of the indexed stream d_in[0, n), written to d_out + d_out_off[r].  Only the chunks a
 * range touches -- those with ulen > 0 whose [chunk_off[c], chunk_off[c + 1]) meets it -- are
 * decoded, each whole and with its CRC checked whole; damage elsewhere is not seen.
 *   d_len[r] == 0: nothing is touched, SM_OK, d_out_len[r] = 0.
 *   lo + len overflowing or past chunk_off[nchunks]: SM_ERR_ARGUMENT, d_out_len[r] = 0, nothing written.
 *   else d_range_status[r] = SM_OK and d_out_len[r] = len with the bytes decode(stream)[lo : lo + len],
 *   or the status of the first failing touched chunk in stream order (what
 *   smf_uncompress_chunks_device reports for it: the raw decoder's SM_ERR_*, SMF_ERR_CRC) and
 *   d_out_len[r] = 0; a failing range's bytes are unspecified but stay inside its own output.
 * The index is an untrusted hint: no value in it causes a read outside d_in[0, n) or a write
 * outside a range's [d_out_off[r], + len).  A touched entry fails its chunk with SM_ERR_ARGUMENT
 * unless type <= 1, ulen <= 65536, chunk_off[c + 1] - chunk_off[c] == ulen, pay_off + pay_len <= n
 * without overflow, for a 0x01 chunk pay_len == ulen, and, lying only partly inside the range, it
 * is the range's first or last chunk.  chunk_off should be non-decreasing; the searches are
 * bounded by nchunks whatever it holds.
 * max_range_chunks: the caller's bound on the slots summed over all ranges (smf_range_plan's
 * counts; smf_range_chunk_count for this library's streams); it sizes the launches and the ctx
 * scratch (smf_range_scratch_bytes).  If the device plan counts more, every d_range_status[r] =
 * SM_ERR_ARGUMENT, every d_out_len[r] = 0 and nothing is written to d_out.
 * A chunk that lies wholly inside its range decodes straight into d_out; the at most two others of
 * a range decode into ctx-owned edge slots, of which the covered bytes are copied out.  Chunks that
 * several ranges touch are decoded once per range.  Ranges whose outputs overlap race.
 * nchunks and nranges are at most 2^31 - 1.  No host synchronisation, except when the ctx's
 * scratch has to grow. */
sm_status smf_uncompress_ranges_device(smf_ctx* ctx, const uint8_t* d_in, uint64_t n, const smf_chunks* d_chunks,
                                       const uint64_t* d_chunk_off, uint32_t nchunks, const uint64_t* d_lo,
                                       const uint64_t* d_len, uint32_t nranges, uint32_t max_range_chunks,
                                       uint8_t* d_out, const uint64_t* d_out_off, uint64_t* d_out_len,
                                       int32_t* d_range_status, void* stream);

/* Decodes a batch of framed streams in one call.  Stream s is d_in[d_in_off[s], d_in_off[s] +
 * d_in_len[s]) (u64 offsets and lengths, any alignment) and decodes to d_out + d_out_off[s], where
 * d_out_cap[s] bytes are its own.  The offset, length and capacity arrays are the caller's and are
 * trusted; the stream bytes are not.  Each stream is walked by a wave of its own, and all data
 * chunks of all streams go through the raw batched decoder, the copy kernel and the CRC pass once.
 * For stream s, d_status[s], d_out_len[s] and the bytes are what smf_uncompress_device leaves for
 * that stream alone with out_capacity = d_out_cap[s]:
 *   a structural error from the walk: that status; d_out_len[s] = the declared lengths of the data
 *     chunks before the error; nothing of the stream is decoded and it takes no slots;
 *   well formed but longer than d_out_cap[s]: SM_BUFFER_TOO_SMALL, d_out_len[s] = the size needed;
 *     nothing is decoded, no slots;
 *   else every data chunk takes a slot and decodes to d_out_off[s] + the declared lengths before it
 *     in its stream; d_status[s] = the first failing chunk's status in stream order (the raw
 *     decoder's SM_ERR_*, or SMF_ERR_CRC), else SM_OK; d_out_len[s] = the sum of the declared
 *     lengths; a failing chunk does not stop the other chunks of its stream.
 * Streams do not affect each other: no byte is read outside a stream's own input range (a stream cut
 * in the middle of a chunk is SMF_ERR_TRUNCATED whatever lies behind it) and none is written
 * outside [d_out_off[s], d_out_off[s] + d_out_cap[s]).  Streams whose outputs overlap race.
 * max_chunks: the caller's bound on the slots summed over all streams (smf_streams_plan's total;
 * ceil(length / 65536) per stream of this library's encoder; smf_max_data_chunks for any stream);
 * it sizes the launches and the ctx scratch (smf_streams_scratch_bytes).  If the device plan counts
 * more, every d_status[s] = SM_ERR_ARGUMENT, every d_out_len[s] = 0 and nothing is written to d_out.
 * d_chunk_first (nstreams + 1) and d_chunk_status (max_chunks) are optional, both given or both
 * NULL: d_chunk_first = the exclusive scan of the slots per stream, and
 * d_chunk_status[d_chunk_first[s] + k] = data chunk k's status of stream s, as
 * smf_uncompress_chunks_device reports it (slots no chunk took: SM_OK).
 * nstreams and max_chunks are at most 2^31 - 1; nstreams == 0 launches nothing.  No host
 * synchronisation, except when the ctx's scratch has to grow. */
sm_status smf_uncompress_streams_device(smf_ctx* ctx, const uint8_t* d_in, const uint64_t* d_in_off,
                                        const uint64_t* d_in_len, uint32_t nstreams, uint32_t max_chunks, uint8_t* d_out,
                                        const uint64_t* d_out_off, const uint64_t* d_out_cap, uint64_t* d_out_len,
                                        int32_t* d_status, uint32_t* d_chunk_first, int32_t* d_chunk_status,
                                        void* stream);

/* Frames a batch of inputs in one call.  Input s is d_in[d_in_off[s], d_in_off[s] + d_in_len[s])
 * (trusted arrays, any alignment) and becomes one complete framed stream at d_out + d_out_off[s],
 * where the caller leaves room for smf_max_framed_length(d_in_len[s]) bytes: the bytes
 * smf_compress_device gives for that input alone in the same mode (the identifier, then one chunk
 * per 64 KiB block by the encoder rule; the empty input: the identifier alone, 10 bytes).
 * d_out_len[s] = the stream's length; d_status[s] = SM_OK, or SM_ERR_DEVICE when the raw
 * compressor left an error mark in one of its blocks (that block is not packed; never expected;
 * the other streams are unaffected).  All blocks of all inputs go through the raw batched
 * compressor and the CRC pass once.
 * max_blocks: the caller's bound on the sum of ceil(d_in_len[s] / 65536); it sizes the launches and
 * the ctx scratch.  If the device counts more, every d_status[s] = SM_ERR_ARGUMENT, every
 * d_out_len[s] = 0 and nothing is written to d_out.  nstreams and max_blocks are at most 2^31 - 1.
 * No seek index is handed out.  No host synchronisation, except when the ctx's scratch has to grow. */
sm_status smf_compress_streams_device(smf_ctx* ctx, const uint8_t* d_in, const uint64_t* d_in_off,
                                      const uint64_t* d_in_len, uint32_t nstreams, uint32_t max_blocks, uint8_t* d_out,
                                      const uint64_t* d_out_off, uint64_t* d_out_len, int32_t* d_status, int mode,
                                      void* stream);

/* ---- host memory (H2D + the device path + D2H, synchronous) ------------------------- */
/* smf_compress_streams_device / smf_uncompress_streams_device over the same arrays in HOST memory:
 * the streams' bytes go up in one copy, the device call runs, and only each stream's own bytes
 * come back to out + out_off[s] (compress: out_len[s] bytes of the smf_max_framed_length(in_len[s])
 * the caller leaves; uncompress: the stream's length when it was decoded, within out_cap[s]).  Both
 * count their bound themselves, the blocks from the lengths and the chunks by smf_streams_plan.
 * The per-stream results are out_len[s] and status[s]; the return value is SM_OK unless the call
 * itself failed (SM_ERR_ARGUMENT, SM_ERR_DEVICE, SM_ERR_INPUT_TOO_LARGE for more than 2^31 - 1
 * blocks or chunks). */
sm_status smf_compress_streams(smf_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len,
                               uint32_t nstreams, uint8_t* out, const uint64_t* out_off, uint64_t* out_len,
                               int32_t* status, int mode);
sm_status smf_uncompress_streams(smf_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len,
                                 uint32_t nstreams, uint8_t* out, const uint64_t* out_off, const uint64_t* out_cap,
                                 uint64_t* out_len, int32_t* status);

/* Bytes [lo, lo + len) of the uncompressed content of a framed stream in host memory.  The stream
 * is indexed on the host; only the bytes from the first touched chunk's payload to the last
 * touched chunk's end are uploaded, and smf_uncompress_ranges_device decodes them.
 * *out_len: in = capacity (< len: SM_BUFFER_TOO_SMALL, *out_len = len), out = bytes written.
 * Returns the walk's structural error as smf_uncompress does, also when it lies behind the range;
 * SM_ERR_ARGUMENT for a range that leaves the stream; else the range's status. */
sm_status smf_uncompress_range(smf_ctx* ctx, const uint8_t* framed, size_t n, uint64_t lo, uint64_t len,
                               uint8_t* output, size_t* out_len);
/* *framed_length: in = capacity (>= smf_max_framed_length(n)), out = bytes written. */
sm_status smf_compress(smf_ctx* ctx, const uint8_t* input, size_t n, uint8_t* framed, size_t* framed_length, int mode);
/* The stream is indexed on the host, decoded and CRC-checked on the device.
 * *length: in = capacity, out = bytes written (with SM_BUFFER_TOO_SMALL: the size needed). */
sm_status smf_uncompress(smf_ctx* ctx, const uint8_t* framed, size_t n, uint8_t* output, size_t* length);
/* The status smf_uncompress would return with enough room (decodes into device scratch). */
sm_status smf_validate(smf_ctx* ctx, const uint8_t* framed, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* SNAPPY_MI355X_FRAMING_H_ */
