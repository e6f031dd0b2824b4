/*
 * snappy_mi355x_blocks.h -- C ABI of libsnappy_mi355x_blocks.so: the two length-prefixed block
 * containers around raw Snappy streams, in batches on the device.  A companion of
 * libsnappy_mi355x_multi.so (snappy_mi355x_multi.h) and libsnappy_mi355x.so (snappy_mi355x.h).
 *
 *   SMB_FORMAT_HADOOP  what Hadoop's SnappyCodec / BlockCompressorStream write: the .snappy files of
 *                      MapReduce, Hive and Spark text output, SequenceFile blocks;
 *   SMB_FORMAT_XERIAL  what snappy-java's SnappyOutputStream writes: Kafka's Snappy record batches.
 *
 * Neither has a checksum, and neither bounds a block at 64 KiB.
 *
 * It is layered on the multi library's public smm_*_device entry points and links that library and
 * the main one by name; all three must sit in one directory.  Status codes are snappy_mi355x.h's
 * plus SMB_ERR_* below.
 *
 * ---- the formats ----------------------------------------------------------------------------
 * Integers are 4 bytes, big-endian, unsigned.  A CHUNK is clen, then clen bytes that are one
 * complete raw Snappy stream (varint header and body); its declared length d is that varint, parsed
 * by the raw decoder's rule over the payload's first min(clen, 5) bytes.
 *   HADOOP  stream = block*, block = ulen chunk*: chunks follow until their declared lengths sum to
 *           ulen.  A block with ulen == 0 has no chunks and the walk GOES ON behind it (Hadoop's own
 *           reader stops there): so concatenated files decode to the concatenated contents.  The
 *           empty stream (0 bytes) is valid and empty.
 *   XERIAL  stream = header chunk*, header = 82 53 4e 41 50 50 59 00 ("\x82SNAPPY\0"), version
 *           00 00 00 01, compatible version 00 00 00 01.  Where a chunk would start and clen reads
 *           0x82534e41, a repeated header stands there (concatenated streams): it is checked like the
 *           first and skipped.  A header is good when its 8 magic bytes match and its version field
 *           is at least 1; the compatible-version field is not checked.
 *
 * The walk, from pos = 0 and total = 0 over the n bytes of a stream:
 *   XERIAL, the header at 0: n == 0, or the bytes present of the first 8 differ from the magic:
 *     SMB_ERR_NO_HEADER; a matching prefix but n < 16: SMB_ERR_TRUNCATED; version 0:
 *     SMB_ERR_BAD_HEADER; else pos = 16.
 *   XERIAL, the loop: pos == n ends the walk (SM_OK); fewer than 4 bytes left: SMB_ERR_TRUNCATED;
 *     L = be32; L == 0x82534e41: fewer than 16 bytes from pos: SMB_ERR_TRUNCATED, magic bytes 4..7
 *     wrong or version 0: SMB_ERR_BAD_HEADER, else pos += 16; any other L is a chunk.
 *   HADOOP, the loop: pos == n ends the walk; fewer than 4 bytes left: SMB_ERR_TRUNCATED; U = be32,
 *     pos += 4; U > 0x7fffffff: SMB_ERR_CHUNK_TOO_LARGE; got = 0, and while got < U: fewer than 4
 *     bytes left: SMB_ERR_TRUNCATED; L = be32, a chunk; got + d > U: SMB_ERR_BLOCK_LENGTH (the chunk
 *     that overruns its block is counted in the lengths the walk reports); got += d.
 *   A chunk at pos with length L: L > n - pos - 4: SMB_ERR_TRUNCATED; its varint does not parse
 *     (L == 0 included): SM_ERR_VARINT; d > 0x7fffffff: SMB_ERR_CHUNK_TOO_LARGE; else the chunk is
 *     recorded (pay_off = pos + 4, pay_len = L, ulen = d, its output at total), total += d,
 *     pos += 4 + L.  A chunk with d == 0 is recorded like any other.
 *
 * The encoder, for both formats: the input is cut into 64 KiB pieces and each piece becomes one
 * chunk whose payload is exactly sm_compress(piece, mode).  In HADOOP every piece is a block of its
 * own (ulen = the piece's length, one chunk).  The empty input is 00 00 00 00 in HADOOP (what Hadoop
 * writes) and the header alone in XERIAL.
 *
 * Threading: an smb_ctx owns an smm_ctx and scratch, and one caller at a time may use it, as an
 * smf_ctx: the *_device calls keep their per-call arrays in the ctx's scratch, so two of them on one
 * ctx must be on one stream (or ordered by the caller), and a call that grows the scratch waits for
 * the device first (hipFree).  smb_compress_streams / smb_uncompress_streams lock the ctx.  No
 * *_device call synchronises otherwise: every decision is taken on the device.
 */
#ifndef SNAPPY_MI355X_BLOCKS_H_
#define SNAPPY_MI355X_BLOCKS_H_

#include <stddef.h>
#include <stdint.h>

#include "snappy_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SMB_FORMAT_HADOOP = 0, SMB_FORMAT_XERIAL = 1 };

enum {
  SMB_ERR_NO_HEADER = 56,       /* XERIAL: the stream is empty or does not start with the magic bytes */
  SMB_ERR_BAD_HEADER = 57,      /* XERIAL: a header with version 0, or a repeated header whose second half is wrong */
  SMB_ERR_TRUNCATED = 58,       /* a length field, a header or a payload runs past the end of the stream */
  SMB_ERR_CHUNK_TOO_LARGE = 59, /* a block or a chunk declares more than 0x7fffffff bytes */
  SMB_ERR_BLOCK_LENGTH = 60     /* HADOOP: a block's chunks declare more bytes than the block */
};

#define SMB_XERIAL_HEADER_LENGTH 16

typedef struct smb_ctx smb_ctx;

/* a stream's chunks, as parallel arrays (host memory) */
typedef struct smb_chunks {
  uint64_t* pay_off; /* the payload (a raw Snappy stream), from the stream's first byte */
  uint32_t* pay_len;
  uint32_t* ulen;    /* the length the payload's varint declares */
} smb_chunks;

typedef struct smb_summary {
  uint64_t total_length; /* the declared lengths: of the whole stream, or before the error */
  uint32_t nchunks;
  int32_t status;        /* SM_OK, a walk error, or SM_BUFFER_TOO_SMALL (nchunks > max_chunks) */
} smb_summary;

/* ---- host helpers (no device needed) ------------------------------------------------- */
/* the SMB_ERR_* texts, else the main library's */
const char* smb_status_message(sm_status st);
/* library build identification ("snappy_mi355x_blocks gfx950 <source hash>") */
const char* smb_version(void);
/* The encoder's bound for an n-byte input: over its 64 KiB pieces sm_max_compressed_length(piece)
 * plus 8 (HADOOP) or 4 (XERIAL) each; in XERIAL 16 more for the header; 4 for the empty HADOOP input. */
size_t smb_max_length(size_t n, int format);
/* the most chunks an n-byte stream can hold (a chunk takes at least 5 bytes): n / 5, in XERIAL
 * (n - 16) / 5 and 0 below 16 */
uint64_t smb_max_chunks(uint64_t n, int format);
/* The walk over a host buffer.  chunks NULL: count only.  Entries [0, min(nchunks, max_chunks)) are
 * stored; more chunks than max_chunks with chunks given: SM_BUFFER_TOO_SMALL.  Returns
 * summary->status; SM_ERR_ARGUMENT for a NULL summary or buffer or an unknown format. */
sm_status smb_index(const uint8_t* buf, size_t n, int format, const smb_chunks* chunks, uint32_t max_chunks,
                    smb_summary* summary);
sm_status smb_uncompressed_length(const uint8_t* buf, size_t n, int format, size_t* result);
/* The decode plan of smb_uncompress_streams_device on the host, by the code the kernels run: per
 * stream status[s] (the walk's error, SM_BUFFER_TOO_SMALL against out_cap[s], or SM_OK: what is known
 * before any byte is decoded), out_len[s] (the size needed, or the declared lengths before the
 * error) and first[0, nstreams] (the exclusive scan of the slots: a stream that is decoded takes one
 * per chunk, any other none).  *total_chunks = the slots, *total_fragments = the sum of
 * smm_fragment_count(ulen) over them: the two bounds of the device call.  out_cap NULL: no limit;
 * every output pointer may be NULL.  More slots than max_chunks: SM_BUFFER_TOO_SMALL, every status
 * SM_ERR_ARGUMENT and every out_len 0, as the device call leaves them. */
sm_status smb_streams_plan(const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nstreams,
                           int format, const uint64_t* out_cap, uint32_t max_chunks, uint32_t* first, uint64_t* out_len,
                           int32_t* status, uint64_t* total_chunks, uint64_t* total_fragments);
/* the device memory a *_streams_device call of that shape keeps in the ctx (the larger of the two
 * calls' needs; max_slots = max_chunks or max_blocks), the smm_ctx's own scratch not counted */
size_t smb_streams_scratch_bytes(uint32_t nstreams, uint32_t max_slots, uint32_t max_fragments);

/* ---- context ------------------------------------------------------------------------ */
/* NULL without a usable device */
smb_ctx* smb_ctx_create(int device);
void smb_ctx_destroy(smb_ctx* ctx);
/* diagnostic: smm_ctx_last_indexed of the ctx's smm_ctx -- the number of chunks the last decode
 * call took by fragments; waits for the device.  -1 for a NULL ctx or before the first decode. */
int smb_ctx_last_indexed(smb_ctx* ctx);

/* ---- device memory, asynchronous on `stream` (a hipStream_t; NULL = the default stream) ----
 * The offset, length and capacity arrays are trusted; the stream bytes are not.
 *
 * Decode.  Stream s = d_in[d_in_off[s] .. +d_in_len[s]) at any alignment, of `format`, into
 * d_out[d_out_off[s] .. +d_out_cap[s]).  Per stream:
 *   a structural error from the walk: d_status[s] = that status, d_out_len[s] = the declared lengths
 *     before the error; nothing of it is decoded and it takes no slots;
 *   well formed but longer than d_out_cap[s]: SM_BUFFER_TOO_SMALL, d_out_len[s] = the size needed;
 *     nothing is decoded;
 *   otherwise every chunk takes a slot and decodes, with capacity equal to its declared length, to
 *     d_out_off[s] plus the declared lengths before it; d_status[s] = the first failing chunk's raw
 *     decoder status in stream order, else SM_OK (a failing chunk does not stop the others);
 *     d_out_len[s] = the total.
 * No byte is read outside a stream's own input range and none written outside
 * [d_out_off[s], d_out_off[s] + d_out_cap[s]).
 * max_chunks: the caller's bound on the slots (smb_streams_plan, or smb_max_chunks summed); it
 * sizes the launches and the scratch.  When the device counts more, every d_status[s] =
 * SM_ERR_ARGUMENT, every d_out_len[s] = 0 and nothing is written to d_out.
 * d_chunk_first (nstreams + 1) and d_chunk_status (max_chunks), both or neither: the exclusive scan
 * of the slots, and per slot its raw decoder status (0 for a slot no chunk took).
 * max_fragments is a speed hint only: the slots go through smm_index_device with that bound and then
 * through smm_uncompress_device with the index it built, so a chunk of more than 64 KiB that a block
 * compressor wrote (Hadoop's default buffer gives chunks of about 218,000 bytes) decodes fragment by
 * fragment.  With 0 no index is built, and when the index builder counts more than the bound it
 * hands back its empty index: every slot then decodes in stream order.  Bytes and statuses are the same either way, with
 * the one exception of smm_uncompress_device's documented leniency: a stray unparsed last byte at a
 * fragment's end is accepted fragment by fragment, while the decoder in stream order parses it as a
 * tag.  A payload of 0xfff00000 bytes or more reads as the raw codec's error mark and is refused.
 * There is no host synchronisation except when the scratch grows.
 * Returns SM_ERR_ARGUMENT for a NULL ctx or array, an unknown format, one of d_chunk_first /
 * d_chunk_status without the other, nstreams or max_chunks above 0x7fffffff; SM_ERR_DEVICE when a
 * launch or an allocation failed. */
sm_status smb_uncompress_streams_device(smb_ctx* ctx, int format, const uint8_t* d_in, const uint64_t* d_in_off,
                                        const uint64_t* d_in_len, uint32_t nstreams, uint32_t max_chunks,
                                        uint32_t max_fragments, uint8_t* d_out, const uint64_t* d_out_off,
                                        const uint64_t* d_out_cap, uint64_t* d_out_len, int32_t* d_status,
                                        uint32_t* d_chunk_first, int32_t* d_chunk_status, void* stream);

/* Compress.  Input s = d_in[d_in_off[s] .. +d_in_len[s]) becomes one stream of `format` by the
 * encoder rule above at d_out + d_out_off[s], where smb_max_length(d_in_len[s], format) bytes are
 * left for it; d_out_len[s] = its size; d_status[s] = SM_OK, or SM_ERR_DEVICE when the raw
 * compressor left an error mark for one of its pieces (never expected; the stream is then unusable).
 * max_blocks: the caller's bound on the sum of ceil(d_in_len[s] / 65536); over it every d_status[s]
 * = SM_ERR_ARGUMENT, every d_out_len[s] = 0 and nothing is written to d_out.  mode: SM_MODE_*. */
sm_status smb_compress_streams_device(smb_ctx* ctx, int format, const uint8_t* d_in, const uint64_t* d_in_off,
                                      const uint64_t* d_in_len, uint32_t nstreams, uint32_t max_blocks, uint8_t* d_out,
                                      const uint64_t* d_out_off, uint64_t* d_out_len, int32_t* d_status, int mode,
                                      void* stream);

/* ---- host memory (one upload, the device path, one download; synchronous; lock the ctx) ----
 * The arrays as above, in host memory; the bounds are counted here.  Only each stream's own bytes
 * are copied back: out is otherwise untouched.  A stream alone is a batch of one. */
sm_status smb_compress_streams(smb_ctx* ctx, int format, const uint8_t* in, const uint64_t* in_off,
                               const uint64_t* in_len, uint32_t nstreams, uint8_t* out, const uint64_t* out_off,
                               uint64_t* out_len, int32_t* status, int mode);
sm_status smb_uncompress_streams(smb_ctx* ctx, int format, const uint8_t* in, const uint64_t* in_off,
                                 const uint64_t* in_len, uint32_t nstreams, uint8_t* out, const uint64_t* out_off,
                                 const uint64_t* out_cap, uint64_t* out_len, int32_t* status);

#ifdef __cplusplus
}
#endif
#endif /* SNAPPY_MI355X_BLOCKS_H_ */
