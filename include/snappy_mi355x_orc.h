/*
 * snappy_mi355x_orc.h -- C ABI of libsnappy_mi355x_orc.so: the compression-stream format of ORC
 * files written with compress=SNAPPY, in batches on the device.  A companion of
 * libsnappy_mi355x_multi.so (snappy_mi355x_multi.h) and libsnappy_mi355x.so (snappy_mi355x.h).
 *
 * Every stream of such a file (data, index, stripe footer, metadata, file footer) is a sequence of
 * compression chunks, each a raw Snappy stream or, where compression did not pay, the original
 * bytes.  This library is that layer and nothing above it: the caller supplies the streams' byte
 * ranges and the file's compression block size (both are in the file's PostScript and footers); no
 * protobuf metadata, stripe layout or RLE encoding is parsed here.
 *
 * It is layered on the multi library's public smm_*_device entry points and links that library and
 * the main one by name; all three must sit in one directory.  Status codes are snappy_mi355x.h's
 * plus SMO_ERR_* below.
 *
 * ---- the format -----------------------------------------------------------------------------
 * A stream of n bytes is chunk*.  A CHUNK is a 3-byte header and L payload bytes.  The header is the
 * little-endian number H = h0 | h1 << 8 | h2 << 16, with L = H >> 1 and original = H & 1 (each field
 * is put together from single bytes: a stream sits at any alignment).  original == 1: the payload is
 * the chunk's L bytes themselves.  original == 0: the payload is one complete raw Snappy stream
 * (varint header and body).  From the ORC specification: a chunk compressed to 100,000 bytes has the
 * header 40 0d 03; five stored bytes have the header 0b 00 00.
 *
 * block_size is the file's compression block size, the most bytes a chunk may hold once decoded.
 * It is an argument of every call and must lie in 1 .. 0x7fffff (L has 23 bits); anything else is
 * SM_ERR_ARGUMENT.
 *
 * The walk, from pos = 0 and total = 0 over the n bytes of a stream:
 *   pos == n ends the walk (SM_OK): the empty stream is valid and empty;
 *   one or two bytes left: SMO_ERR_TRUNCATED;
 *   L > n - pos - 3: SMO_ERR_TRUNCATED;
 *   original: the declared length d = L (L == 0 is a valid empty chunk, recorded like any other);
 *   compressed: d = the payload's varint, parsed by the raw decoder's rule over the payload's first
 *     min(L, 5) bytes; a varint that does not parse (L == 0 included): SM_ERR_VARINT;
 *   d > block_size: SMO_ERR_CHUNK_TOO_LARGE;
 *   else the chunk is recorded (pay_off = pos + 3, pay_len = L, ulen = d, original, its output at
 *     total), total += d, pos += 3 + L.
 *
 * The encoder: the input is cut into pieces of block_size bytes (the last may be shorter).  For each
 * piece raw = sm_compress(piece, mode) -- what smm_compress_device gives for a stream of that length:
 * a piece above 64 KiB is its varint and its 64 KiB fragments.  len(raw) < len(piece): the chunk is
 * header(len(raw), 0) raw; otherwise header(len(piece), 1) piece, the ORC writers' rule.  (A piece
 * the raw compressor's incompressible screen leaves as literals is longer than the piece, so it is
 * always stored.)  The empty input is the empty stream.
 *
 * Threading: an smo_ctx owns an smm_ctx and scratch, and one caller at a time may use it, as an
 * smb_ctx: the *_device calls keep their per-call arrays in the ctx's scratch, so two of them on one
 * ctx must be on one stream (or ordered by the caller), and a call that grows the scratch waits for
 * the device first (hipFree).  smo_compress_streams / smo_uncompress_streams lock the ctx.  No
 * *_device call synchronises otherwise: every decision is taken on the device.
 */
#ifndef SNAPPY_MI355X_ORC_H_
#define SNAPPY_MI355X_ORC_H_

#include <stddef.h>
#include <stdint.h>

#include "snappy_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
  SMO_ERR_TRUNCATED = 64,      /* a chunk header or a payload runs past the end of the stream */
  SMO_ERR_CHUNK_TOO_LARGE = 65 /* a chunk declares more than block_size bytes */
};

#define SMO_HEADER_LENGTH 3
#define SMO_MAX_BLOCK_SIZE 0x7fffff

typedef struct smo_ctx smo_ctx;

/* a stream's chunks, as parallel arrays (host memory) */
typedef struct smo_chunks {
  uint64_t* pay_off; /* the payload, from the stream's first byte */
  uint32_t* pay_len;
  uint32_t* ulen;     /* the declared length: the payload's varint, or pay_len of a stored chunk */
  uint8_t* original;  /* 1: the payload is the chunk's bytes; 0: a raw Snappy stream */
} smo_chunks;

typedef struct smo_summary {
  uint64_t total_length; /* the declared lengths: of the whole stream, or before the error */
  uint32_t nchunks;
  int32_t status;        /* SM_OK, a walk error, or SM_BUFFER_TOO_SMALL (nchunks > max_chunks) */
} smo_summary;

/* ---- host helpers (no device needed) ------------------------------------------------- */
/* the SMO_ERR_* texts, else the main library's */
const char* smo_status_message(sm_status st);
/* library build identification ("snappy_mi355x_orc gfx950 <source hash>") */
const char* smo_version(void);
/* the encoder's bound for an n-byte input: n + 3 * ceil(n / block_size) (a chunk is never longer
 * than its piece); 0 for a block_size outside 1 .. 0x7fffff */
size_t smo_max_length(size_t n, uint32_t block_size);
/* the most chunks an n-byte stream can hold (a chunk takes at least its header): n / 3 */
uint64_t smo_max_chunks(uint64_t n);
/* The walk over a host buffer.  chunks NULL: count only.  Entries [0, min(nchunks, max_chunks)) are
 * stored; more chunks than max_chunks with chunks given: SM_BUFFER_TOO_SMALL.  Returns
 * summary->status; SM_ERR_ARGUMENT for a NULL summary or buffer or a block_size out of range. */
sm_status smo_index(const uint8_t* buf, size_t n, uint32_t block_size, const smo_chunks* chunks, uint32_t max_chunks,
                    smo_summary* summary);
sm_status smo_uncompressed_length(const uint8_t* buf, size_t n, uint32_t block_size, size_t* result);
/* The decode plan of smo_uncompress_streams_device on the host, by the code the kernels run: per
 * stream status[s] (the walk's error, SM_BUFFER_TOO_SMALL against out_cap[s], or SM_OK: what is known
 * before any byte is decoded), out_len[s] (the size needed, or the declared lengths before the
 * error) and first[0, nstreams] (the exclusive scan of the slots: a stream that is decoded takes one
 * per chunk, stored or compressed, any other none).  *total_chunks = the slots, *total_fragments =
 * the sum of smm_fragment_count(ulen) over the compressed ones: the two bounds of the device call.
 * out_cap NULL: no limit; every output pointer may be NULL.  More slots than max_chunks:
 * SM_BUFFER_TOO_SMALL, every status SM_ERR_ARGUMENT and every out_len 0, as the device call leaves
 * them. */
sm_status smo_streams_plan(const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nstreams,
                           uint32_t block_size, const uint64_t* out_cap, uint32_t max_chunks, uint32_t* first,
                           uint64_t* out_len, int32_t* status, uint64_t* total_chunks, uint64_t* total_fragments);
/* the device memory a *_streams_device call of that shape keeps in the ctx (the larger of the two
 * calls' needs; max_slots = max_chunks or max_pieces; the compress call's output slots are
 * sm_max_compressed_length(block_size), rounded up to 256, each), the smm_ctx's own scratch not
 * counted */
size_t smo_streams_scratch_bytes(uint32_t nstreams, uint32_t max_slots, uint32_t max_fragments, uint32_t block_size);

/* ---- context ------------------------------------------------------------------------ */
/* NULL without a usable device */
smo_ctx* smo_ctx_create(int device);
void smo_ctx_destroy(smo_ctx* ctx);
/* diagnostic: smm_ctx_last_indexed of the ctx's smm_ctx -- the number of chunks the last decode
 * call took by fragments; waits for the device.  -1 for a NULL ctx or before the first decode. */
int smo_ctx_last_indexed(smo_ctx* ctx);

/* ---- device memory, asynchronous on `stream` (a hipStream_t; NULL = the default stream) ----
 * The offset, length and capacity arrays are trusted; the stream bytes are not.
 *
 * Decode.  Stream s = d_in[d_in_off[s] .. +d_in_len[s]) at any alignment into
 * d_out[d_out_off[s] .. +d_out_cap[s]).  Per stream:
 *   a structural error from the walk: d_status[s] = that status, d_out_len[s] = the declared lengths
 *     before the error; nothing of it is decoded and it takes no slots;
 *   well formed but longer than d_out_cap[s]: SM_BUFFER_TOO_SMALL, d_out_len[s] = the size needed;
 *     nothing is decoded;
 *   otherwise every chunk takes a slot and goes to d_out_off[s] plus the declared lengths before it:
 *     a stored chunk is copied (its status is SM_OK), a compressed one decodes with capacity equal
 *     to its declared length; d_status[s] = the first failing chunk's raw decoder status in stream
 *     order, else SM_OK (a failing chunk does not stop the others); d_out_len[s] = the total.
 * No byte is read outside a stream's own input range and none written outside
 * [d_out_off[s], d_out_off[s] + d_out_cap[s]).
 * max_chunks: the caller's bound on the slots (smo_streams_plan, or smo_max_chunks summed); it
 * sizes the launches and the scratch.  When the device counts more, every d_status[s] =
 * SM_ERR_ARGUMENT, every d_out_len[s] = 0 and nothing is written to d_out.
 * d_chunk_first (nstreams + 1) and d_chunk_status (max_chunks), both or neither: the exclusive scan
 * of the slots, and per slot its status (0 for a stored chunk and for a slot no chunk took).
 * max_fragments is a speed hint only: the compressed slots go through smm_index_device with that
 * bound and then through smm_uncompress_device with the index it built, so a chunk of more than
 * 64 KiB that a block compressor wrote decodes fragment by fragment.  With 0 no index is built, and
 * when the index builder counts more than the bound it hands back its empty index: every slot then
 * decodes in stream order.  Bytes and statuses are the same either way, with the one exception of
 * smm_uncompress_device's documented leniency: a stray unparsed last byte at a fragment's end is
 * accepted fragment by fragment, while the decoder in stream order parses it as a tag.
 * There is no host synchronisation except when the scratch grows.
 * Returns SM_ERR_ARGUMENT for a NULL ctx or array, a block_size out of range, one of d_chunk_first /
 * d_chunk_status without the other, nstreams or max_chunks above 0x7fffffff; SM_ERR_DEVICE when a
 * launch or an allocation failed. */
sm_status smo_uncompress_streams_device(smo_ctx* ctx, uint32_t block_size, const uint8_t* d_in, const uint64_t* d_in_off,
                                        const uint64_t* d_in_len, uint32_t nstreams, uint32_t max_chunks,
                                        uint32_t max_fragments, uint8_t* d_out, const uint64_t* d_out_off,
                                        const uint64_t* d_out_cap, uint64_t* d_out_len, int32_t* d_status,
                                        uint32_t* d_chunk_first, int32_t* d_chunk_status, void* stream);

/* Compress.  Input s = d_in[d_in_off[s] .. +d_in_len[s]) becomes one stream by the encoder rule
 * above at d_out + d_out_off[s], where smo_max_length(d_in_len[s], block_size) bytes are left for
 * it; d_out_len[s] = its size; d_status[s] = SM_OK, or SM_ERR_DEVICE when the raw compressor left an
 * error mark for one of its pieces (never expected; the stream is then unusable).
 * max_pieces: the caller's bound on the sum of ceil(d_in_len[s] / block_size); over it every
 * d_status[s] = SM_ERR_ARGUMENT, every d_out_len[s] = 0 and nothing is written to d_out.  The bound
 * smm_compress_device needs on the pieces' 64 KiB fragments is derived here: max_pieces *
 * ceil(block_size / 65536) when block_size > 65536, else 0; a product above 0x7fffffff is
 * SM_ERR_ARGUMENT.  mode: SM_MODE_*. */
sm_status smo_compress_streams_device(smo_ctx* ctx, uint32_t block_size, const uint8_t* d_in, const uint64_t* d_in_off,
                                      const uint64_t* d_in_len, uint32_t nstreams, uint32_t max_pieces, uint8_t* d_out,
                                      const uint64_t* d_out_off, uint64_t* d_out_len, int32_t* d_status, int mode,
                                      void* stream);

/* ---- host memory (one upload, the device path, one download; synchronous; lock the ctx) ----
 * The arrays as above, in host memory; the bounds are counted here.  Only each stream's own bytes
 * are copied back: out is otherwise untouched.  A stream alone is a batch of one. */
sm_status smo_compress_streams(smo_ctx* ctx, uint32_t block_size, const uint8_t* in, const uint64_t* in_off,
                               const uint64_t* in_len, uint32_t nstreams, uint8_t* out, const uint64_t* out_off,
                               uint64_t* out_len, int32_t* status, int mode);
sm_status smo_uncompress_streams(smo_ctx* ctx, uint32_t block_size, const uint8_t* in, const uint64_t* in_off,
                                 const uint64_t* in_len, uint32_t nstreams, uint8_t* out, const uint64_t* out_off,
                                 const uint64_t* out_cap, uint64_t* out_len, int32_t* status);

#ifdef __cplusplus
}
#endif
#endif /* SNAPPY_MI355X_ORC_H_ */
