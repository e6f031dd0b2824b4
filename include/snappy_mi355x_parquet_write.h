/*
 * snappy_mi355x_parquet_write.h -- the page encoder of libsnappy_mi355x_parquet.so: column chunks
 * whose pages a writer holds in their plain form become compression=SNAPPY chunks, in batches on the
 * device.  The same library and the same smq_ctx as snappy_mi355x_parquet.h, whose reader
 * (smq_uncompress_chunks_device) reads what this writes; the Thrift rules, the page types, smq_pages
 * and the SMQ_ERR_* codes are that header's.
 *
 * The input is what a writer emits before it knows any compressed size, and what parquet-cpp writes
 * with compression=NONE: a run of pages, each a compact-protocol PageHeader and its body, with
 * compressed_page_size == uncompressed_page_size.  It describes itself, so there are no side tables.
 * No footer is written: the caller puts the new sizes and offsets into its ColumnMetaData.
 *
 * ---- the encode walk, from pos = 0 over the n bytes of a chunk ----------------------------------
 * The decode walk of snappy_mi355x_parquet.h with the same header rules and statuses -- fields 1, 2
 * and 3 as i32 and no size below 0, the page type's own struct, the level lengths of a v2 page, the
 * body inside the chunk (SMQ_ERR_HEADER, SMQ_ERR_TRUNCATED) -- and these differences:
 *   PageHeader field 3 or 4 occurring more than once as an i32, or field 7 (is_compressed) of
 *     data_page_header_v2 occurring more than once as a bool: SMQ_ERR_HEADER (a patched field must be
 *     the one a reader takes; the decode walk's "the last counts" stays what it is for decoding);
 *   types 0, 2 and 3: compressed_page_size != uncompressed_page_size is SMQ_ERR_SIZE_MISMATCH.  No
 *     byte of a section is looked at: it is not Snappy yet, and is_compressed may say anything;
 *   a page's flags hold SMQ_PAGE_HAS_CRC alone; its crc is the header's, which nobody checks;
 *   up to three patch sites are recorded per header, as offsets from the header's first byte:
 *     f3_at, f3_len: the bytes of field 3's value; f4_at, f4_len: those of field 4's value (f4_len 0:
 *     no field 4); f7_at: the field header byte of the v2 field 7 (0: there is none).
 *
 * ---- per page of type 0, 2 or 3, with levels and want = uncompressed_page_size - levels ----------
 *   raw = what smm_compress_device gives for the want bytes behind the level bytes in `mode`: what
 *     sm_compress gives for them.  The empty section gives the one byte 00; a section above 64 KiB
 *     its varint and its 64 KiB fragments.  Nothing is ever stored instead: Parquet v1 has no stored
 *     form, parquet-cpp and parquet-mr compress whatever the gain, and so does this for v2 too;
 *   the new body is the level bytes and raw;
 *   levels + len(raw) > 0x7fffffff: the page's status is SM_ERR_INPUT_TOO_LARGE;
 *   an error mark of the raw compressor (never expected): SM_ERR_DEVICE.
 * ---- the header rewrite ---------------------------------------------------------------------------
 * The header's bytes are copied as they are, except:
 *   field 3's value becomes the zigzag varint of the new body's length;
 *   if and only if the header has a field 4, its value becomes the zigzag varint of the CRC-32 (IEEE)
 *     of the new body as an i32.  A header without a crc stays without one: a new field would change
 *     the next field's delta, and a writer that wants checksums writes the field;
 *   the header byte of a v2 field 7, if there is one, gets type nibble 1 (true); none means true.
 * Unknown fields, statistics, long-form ids and the fields' order stay, since nothing else is
 * touched.  Each varint takes 1 to 5 bytes whatever it took before, so the header's length, and with
 * it the body's place, depends on the body's CRC: the bodies are staged and packed afterwards.
 * A page the walk steps over (an index page, an unknown type) is copied as it is, header and body.
 */
#ifndef SNAPPY_MI355X_PARQUET_WRITE_H_
#define SNAPPY_MI355X_PARQUET_WRITE_H_

#include <stddef.h>
#include <stdint.h>

#include "snappy_mi355x_parquet.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SMQE_SITES 5 /* uint32_t per page: f3_at, f3_len, f4_at, f4_len, f7_at */

/* ---- host helpers (no device needed) ------------------------------------------------- */
/* An upper bound on the output of an n-byte chunk of that many pages: n + n / 6 + 40 pages.  A body
 * of b bytes becomes at most sm_max_compressed_length(b) = 32 + b + b / 6 (the level bytes do not
 * grow), and each of a header's two varints grows by at most 4 bytes. */
uint64_t smqe_max_chunk_length(uint64_t n, uint64_t pages);
/* An upper bound on stage_bytes for chunks of total_in_bytes in all with that many pages:
 * 32 + total_in_bytes + total_in_bytes / 6 + 48 pages (a page's slot is its level bytes and
 * sm_max_compressed_length(want), rounded up to 16; the first 32 bytes belong to no page). */
uint64_t smqe_stage_bound(uint64_t total_in_bytes, uint64_t pages);
/* The rewrite rule alone.  hdr[0, n) begins with a PageHeader (what lies behind its end is not
 * read): it is parsed by the encode walk's reader, and must have fields 1, 2 and 3 and no patched
 * field twice (else SMQ_ERR_HEADER, SMQ_ERR_TRUNCATED as the walk gives them); the page type's rules
 * are not applied.  new_body_len > 0x7fffffff: SM_ERR_INPUT_TOO_LARGE.  *out_len = the new header's
 * length; more than cap: SM_BUFFER_TOO_SMALL and nothing is written (out NULL with cap 0 measures). */
sm_status smqe_rewrite_header(const uint8_t* hdr, size_t n, uint64_t new_body_len, uint32_t crc, uint8_t* out, size_t cap,
                              size_t* out_len);
/* The encode walk over a host buffer, as smq_index is the decode walk: pages describes the INPUT's
 * pages; sites, optional, gets SMQE_SITES words per stored page.  pages NULL: count only (sites is
 * then not written).  summary->total_length = the uncompressed sizes, as for smq_index. */
sm_status smqe_index(const uint8_t* buf, size_t n, const smq_pages* pages, uint32_t* sites, uint32_t max_pages,
                     smq_summary* summary);
/* The plan of smqe_compress_chunks_device on the host, by the code the kernels run: per chunk
 * status[c] (the walk's error or SM_OK: what is known before any byte is compressed), first[0,
 * nchunks] (the exclusive scan of the slots: a chunk without a walk error takes one per page) and
 * out_bound[c] (an upper bound on its output, exact for the pages that are stepped over: a
 * d_out_cap[c] that always suffices; 0 with a walk error).  *total_pages, *stage_bytes and
 * *total_fragments (the sum of smm_fragment_count(want) over the sections above 64 KiB) are the three
 * bounds of the device call.  Every output pointer may be NULL.  More slots than max_pages:
 * SM_BUFFER_TOO_SMALL, every status SM_ERR_ARGUMENT and every out_bound 0. */
sm_status smqe_chunks_plan(const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nchunks,
                           uint32_t max_pages, uint32_t* first, int32_t* status, uint64_t* out_bound, uint64_t* total_pages,
                           uint64_t* stage_bytes, uint64_t* total_fragments);
/* the device memory an smqe_compress_chunks_device call of that shape keeps in the ctx, the stage
 * included, the smm_ctx's own scratch and the CRC tables not counted */
size_t smqe_scratch_bytes(uint32_t nchunks, uint32_t max_pages, uint64_t stage_bytes);

/* ---- device memory, asynchronous on `stream` (a hipStream_t; NULL = the default stream) ----
 * The offset, length and capacity arrays are trusted; the chunk bytes are not.
 *
 * Chunk c = d_in[d_in_off[c] .. +d_in_len[c]) at any alignment, in the plain form, becomes a
 * compression=SNAPPY chunk in d_out[d_out_off[c] .. +d_out_cap[c]) at any alignment.  Per chunk:
 *   an error from the encode walk: d_status[c] = that status, d_out_len[c] = 0; it takes no slots;
 *   otherwise every page takes a slot and, with output, a stage slot; the sections of all pages of
 *     all chunks are compressed by one smm_compress_device call in `mode` (SM_MODE_*).  A page's
 *     status is SM_ERR_DEVICE, SM_ERR_INPUT_TOO_LARGE (above) or SM_OK; d_status[c] = the first
 *     failing page's status in page order, with d_out_len[c] = 0;
 *   no page failed but the chunk is longer than d_out_cap[c]: SM_BUFFER_TOO_SMALL, d_out_len[c] =
 *     the size needed;
 *   else SM_OK, d_out_len[c] = its size, and the pages stand back to back at d_out_off[c]: rewritten
 *     header and new body, or the page as it was.
 * Only a chunk with SM_OK is written.  No byte is read outside a chunk's own input range and none
 * written outside [d_out_off[c], d_out_off[c] + d_out_cap[c]).
 * The three bounds (smqe_chunks_plan, or smq_max_pages summed and smqe_stage_bound) size the
 * launches and the scratch: when the device counts more slots than max_pages, more stage than
 * stage_bytes or more fragments than max_fragments, every d_status[c] = SM_ERR_ARGUMENT, every
 * d_out_len[c] = 0 and nothing is written to d_out.
 * d_page_first (nchunks + 1) and d_page_status (max_pages), both or neither: the exclusive scan of
 * the slots, and per slot its page's status (0 for a slot no page took).  d_pages, optional: a host
 * struct of device arrays of max_pages entries each; slot d_page_first[c] + k holds page k of the
 * OUTPUT chunk c as smq_index gives it for that chunk (a slot no page took: zeros; those of a chunk
 * that is not written mean nothing).
 * There is no host synchronisation except when the scratch grows.
 * Returns SM_ERR_ARGUMENT for a NULL ctx or array, an unknown mode, one of d_page_first /
 * d_page_status without the other, a NULL array in d_pages, nchunks or max_pages above 0x7fffffff;
 * SM_ERR_DEVICE when a launch or an allocation failed. */
sm_status smqe_compress_chunks_device(smq_ctx* ctx, const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                      uint32_t nchunks, uint32_t max_pages, uint64_t stage_bytes, uint32_t max_fragments,
                                      uint8_t* d_out, const uint64_t* d_out_off, const uint64_t* d_out_cap, uint64_t* d_out_len,
                                      int32_t* d_status, uint32_t* d_page_first, const smq_pages* d_pages,
                                      int32_t* d_page_status, int mode, void* stream);

/* ---- host memory (one upload, the device path, one download; synchronous; locks the ctx) ----
 * The arrays as above, in host memory; the three bounds are counted here.  Only each written chunk's
 * own bytes are copied back: out is otherwise untouched. */
sm_status smqe_compress_chunks(smq_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len,
                               uint32_t nchunks, uint8_t* out, const uint64_t* out_off, const uint64_t* out_cap,
                               uint64_t* out_len, int32_t* status, int mode);

#ifdef __cplusplus
}
#endif
#endif /* SNAPPY_MI355X_PARQUET_WRITE_H_ */
