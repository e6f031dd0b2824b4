/*
 * snappy_mi355x_multi.h -- C ABI of libsnappy_mi355x_multi.so: batches of raw Snappy streams of
 * ANY length on the device, the companion of libsnappy_mi355x.so (snappy_mi355x.h).
 *
 * The main library's batched calls take items of at most 64 KiB; its 64 KiB fragment loop of a
 * longer input (src/Snappy.jl:29-33) serves one stream per call.  This library plans a mixed batch
 * on the device: streams of at most 64 KiB go through the batch compressor as they are, the
 * fragments of every longer stream go through the fragment compressor together, and a pack kernel
 * places them behind their stream's varint header.  The pack knows every fragment's offset in its
 * stream: it can hand them out as an INDEX, with which the decoder runs every 64 KiB fragment of
 * every stream as a block of its own instead of one wave per stream.
 *
 * It is layered on the main library's public *_device entry points and links that library by
 * name; both must sit in one directory.  Status codes are snappy_mi355x.h's.
 *
 * Threading: an smm_ctx owns an sm_ctx and scratch, and one caller at a time may use it: the
 * *_device calls keep their per-call arrays in the ctx's scratch, so two of them on one ctx must
 * be on one stream (or ordered by the caller), and a call that grows the scratch waits for the
 * device first (hipFree), as smf_compress_device does.  smm_compress / smm_uncompress / smm_index lock
 * the ctx.  No *_device call synchronises otherwise: every decision is taken on the device.
 */
#ifndef SNAPPY_MI355X_MULTI_H_
#define SNAPPY_MI355X_MULTI_H_

#include <stddef.h>
#include <stdint.h>

#include "snappy_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct smm_ctx smm_ctx;

/* NULL without a usable device */
smm_ctx* smm_ctx_create(int device);
void smm_ctx_destroy(smm_ctx* ctx);
/* library build identification ("snappy_mi355x_multi gfx950 <source hash>") */
const char* smm_version(void);
/* the main library's text for a status code */
const char* smm_status_message(sm_status st);

/* ---- host helpers (no device needed) ------------------------------------------------- */
/* the 64 KiB fragments of a len-byte input: ceil(len / 65536), 0 for 0 */
uint32_t smm_fragment_count(uint64_t len);
/* the device memory a *_device call of that shape keeps in the ctx (the larger of the two calls'
 * needs): per-stream and per-fragment arrays, and for compress max_fragments output slots of
 * 76,544 bytes (sm_max_compressed_length(65536) + 8, rounded up to 256) */
size_t smm_scratch_bytes(uint32_t nstreams, uint32_t max_fragments);
/* The index rules of smm_uncompress_device over host arrays, structure only (nothing is decoded):
 * indexed[s] = 1 when stream s would be decoded by fragments, given that each of them decodes, else
 * 0.  The same code as the device plan's.  frag_first / frag_pos NULL: no index, every entry 0. */
sm_status smm_index_check(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint32_t nstreams,
                          uint32_t max_fragments, const uint32_t* out_cap, const uint32_t* frag_first,
                          const uint32_t* frag_pos, uint8_t* indexed);

/* The index rule of smm_index_device (below) on the CPU, over host arrays: the same results, no
 * device and no ctx.  frag_pos has max_fragments entries. */
sm_status smm_index_host(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint32_t nstreams,
                         uint32_t max_fragments, const uint32_t* out_cap, uint32_t* frag_first, uint32_t* frag_pos,
                         uint8_t* built, int32_t* status);

/* ---- device memory, asynchronous on `stream` (a hipStream_t; NULL = the default stream) ----
 * Compress. Stream s: input d_in[d_in_off[s] .. +d_in_len[s]) at any alignment -> one complete raw
 * Snappy stream at d_out + d_out_off[s], which must have room for
 * sm_max_compressed_length(d_in_len[s]) bytes: varint(len), then the fragments of
 * src/Snappy.jl:29-33 with no gaps -- what sm_compress gives for that input in the same mode, and
 * in SM_MODE_REFERENCE Snappy.jl's exact bytes (a stream of at most 64 KiB with the table size of
 * its own length, every fragment of a longer one with 16,384 entries: src/Snappy.jl:27).
 * d_out_len[s] = its size and d_status[s] = SM_OK, or d_out_len[s] = 0 and
 *   SM_ERR_INPUT_TOO_LARGE  d_in_len[s] > 0x7fffffff; nothing of it is read;
 *   SM_ERR_DEVICE           the raw compressor left an error mark (never expected).
 * max_fragments: the caller's bound on the sum of smm_fragment_count(d_in_len[s]) over the streams
 * longer than 64 KiB; it sizes the launches and the ctx's fragment slots.  With an index (below) it
 * must bound that sum over ALL streams of at most 0x7fffffff bytes, which is what the index holds.
 * When the device plan counts more than max_fragments, every d_status[s] = SM_ERR_ARGUMENT, every
 * d_out_len[s] = 0 and nothing is written to d_out (nor to the index).
 * Index, when both pointers are given:
 *   d_frag_first (nstreams + 1)  the exclusive scan of smm_fragment_count(d_in_len[s]) over all
 *                                streams, the short ones included (a too-large stream counts 0);
 *   d_frag_pos (max_fragments)   d_frag_pos[d_frag_first[s] + f] = the offset inside stream s of
 *                                fragment f's first byte; fragment 0's is the varint's length.  A
 *                                stream with SM_ERR_DEVICE has zeros.
 * Returns SM_ERR_ARGUMENT for a NULL ctx or array or one index pointer without the other, an
 * unknown mode; SM_ERR_DEVICE when a launch or the scratch allocation failed. */
sm_status smm_compress_device(smm_ctx* ctx, const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                              uint32_t nstreams, uint32_t max_fragments, uint8_t* d_out, const uint64_t* d_out_off,
                              uint32_t* d_out_len, int32_t* d_status, uint32_t* d_frag_first, uint32_t* d_frag_pos,
                              int mode, void* stream);

/* Uncompress.  Stream s: d_in[d_in_off[s] .. +d_in_len[s]) -> d_out + d_out_off[s] with capacity
 * d_out_cap[s]; d_status[s] / d_out_len[s] as in the main library's batched decoder.
 * Stream s is INDEXED when all of these hold:
 *   - both index arrays are given, d_frag_first is non-decreasing from 0 and
 *     d_frag_first[nstreams] <= max_fragments (max_fragments: the entries of d_frag_pos);
 *   - its varint parses, with hv bytes, and declares D with 65536 < D <= d_out_cap[s];
 *   - its entry count d_frag_first[s + 1] - d_frag_first[s] equals ceil(D / 65536);
 *   - its first position is hv, its positions increase strictly and the last is below d_in_len[s].
 * Fragment f of an indexed stream is the bytes from its position to the next fragment's position
 * (the last: to the stream's end) and must decode to 65536 bytes (the last: the remainder) as a raw
 * fragment does -- the reference's decoding of varint(that length) + bytes.  When every fragment
 * does, the output is their concatenation (each decoded straight to d_out_off[s] + 65536 f),
 * d_status[s] = SM_OK and d_out_len[s] = D.
 * In every other case -- no index, a bad index, a failing fragment, a stream of at most 64 KiB, a
 * foreign stream whose copies cross 64 KiB -- d_out_len[s], d_status[s] and the bytes are exactly
 * what the main library's batched decoder gives for the stream: it is called for those streams.
 * The index is an untrusted hint: no value in it causes a read outside the stream's input range
 * or a write outside [d_out_off[s], +d_out_cap[s]).
 * Leniency: a stray unparsed last byte at a fragment's end is accepted fragment by fragment, as
 * the raw fragment decoder accepts it; the decoder in stream order would parse it as a tag. */
sm_status smm_uncompress_device(smm_ctx* ctx, const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                uint32_t nstreams, uint32_t max_fragments, uint8_t* d_out, const uint64_t* d_out_off,
                                const uint32_t* d_out_cap, uint32_t* d_out_len, int32_t* d_status,
                                const uint32_t* d_frag_first, const uint32_t* d_frag_pos, void* stream);

/* Index.  Builds, for raw streams that arrive without one (a CPU compressor wrote them, or the
 * index was not kept), the index smm_uncompress_device accepts: no host synchronisation, no output
 * bytes.  Every block compressor emits 64 KiB blocks independently (src/Snappy.jl:29-33), so a tag
 * starts at every output multiple of 65536, and finding those tags is a walk over tag sizes.
 * Stream s, bytes p[0 .. n) with n = d_in_len[s] and cap = d_out_cap[s] (d_out_cap NULL: no cap):
 *   count(s)     = smm_fragment_count(D) when n is no error mark (n < SM_OUT_LEN_ERROR), the varint
 *                  header parses to D with hv bytes, and D <= cap; else 0;
 *   d_frag_first (nstreams + 1)  the exclusive scan of count, as smm_compress_device writes it;
 *   D <= 65536:  the stream's entry (if any) is hv; d_built[s] = 0 (never decoded by fragments);
 *   D > 65536:   tags are sized from x = hv with output o = 0 and f = 0, bytes at or past n reading
 *                as zero, positions and outputs in 64 bits, no offset or length checked.  Before
 *                each tag: x >= n fails; o == 65536 f records d_frag_pos[d_frag_first[s] + f] = x
 *                and steps f, and f == count ends the walk with d_built[s] = 1; o > 65536 f fails
 *                (a tag crosses the multiple: no block compressor wrote the stream).  A failed
 *                stream has d_built[s] = 0 and all its entries 0, as a failed stream has from
 *                smm_compress_device: smm_uncompress_device then decodes it in stream order.
 * When the counts sum to more than max_fragments: every d_status[s] = SM_ERR_ARGUMENT, every
 * d_built[s] = 0, d_frag_first is all zeros (a usable empty index) and d_frag_pos is untouched.
 * Otherwise every d_status[s] = SM_OK.  Entries of d_frag_pos at or past d_frag_first[nstreams] are
 * never written.  The result says nothing about validity: it stays an untrusted hint, and the
 * fragment decode and its fallback decide as before.  A stream is one serial walk by one wave, so a
 * batch of many streams is what this call is for.
 * Returns SM_ERR_ARGUMENT for a NULL ctx or array (d_out_cap may be NULL; d_frag_pos may be with
 * max_fragments 0); SM_ERR_DEVICE when a launch or the scratch allocation failed. */
sm_status smm_index_device(smm_ctx* ctx, const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                           uint32_t nstreams, uint32_t max_fragments, const uint32_t* d_out_cap, uint32_t* d_frag_first,
                           uint32_t* d_frag_pos, uint8_t* d_built, int32_t* d_status, void* stream);

/* diagnostic: the number of streams the ctx's last smm_uncompress_device (or smm_uncompress)
 * decoded by fragments; waits for the device.  -1 for a NULL ctx or before the first call. */
int smm_ctx_last_indexed(smm_ctx* ctx);

/* ---- host memory (H2D, the device path, D2H; synchronous; lock the ctx) -------------------
 * The arrays as above, in host memory.  max_fragments is counted here.  frag_first (nstreams + 1)
 * and frag_pos (the sum of smm_fragment_count over all streams) are both given or both NULL.  Only
 * each stream's own bytes are copied back: out is otherwise untouched. */
sm_status smm_compress(smm_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,
                       uint32_t nstreams, uint8_t* out, const uint64_t* out_off, uint32_t* out_len, int32_t* status,
                       uint32_t* frag_first, uint32_t* frag_pos, int mode);
/* frag_first[nstreams] entries of frag_pos are read (at most 0x7fffffff; a decreasing frag_first
 * is passed on as no usable index). */
sm_status smm_uncompress(smm_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,
                         uint32_t nstreams, uint8_t* out, const uint64_t* out_off, const uint32_t* out_cap,
                         uint32_t* out_len, int32_t* status, const uint32_t* frag_first, const uint32_t* frag_pos);
/* smm_index_device over host arrays; frag_pos has max_fragments entries, of which the first
 * frag_first[nstreams] are written. */
sm_status smm_index(smm_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint32_t nstreams,
                    uint32_t max_fragments, const uint32_t* out_cap, uint32_t* frag_first, uint32_t* frag_pos,
                    uint8_t* built, int32_t* status);

#ifdef __cplusplus
}
#endif
#endif /* SNAPPY_MI355X_MULTI_H_ */
