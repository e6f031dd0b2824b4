/*
 * snappy_mi355x_parquet.h -- C ABI of libsnappy_mi355x_parquet.so: the pages of Parquet column
 * chunks written with compression=SNAPPY, in batches on the device.  A companion of
 * libsnappy_mi355x_multi.so (snappy_mi355x_multi.h) and libsnappy_mi355x.so (snappy_mi355x.h).
 *
 * A column chunk is a run of pages, each a Thrift compact-protocol PageHeader and a body.  This
 * library is that layer and nothing above it: the caller supplies each chunk's byte range and
 * promises that its codec is SNAPPY.  The range is in the footer's ColumnMetaData: it starts at
 * dictionary_page_offset if present, else at data_page_offset, and is total_compressed_size long.
 * No footer, schema, encoding (RLE, dictionary, delta), bloom filter, column or offset index,
 * encryption or other codec is parsed here, and nothing is written: the page encoder of this library
 * has a header of its own, snappy_mi355x_parquet_write.h.
 *
 * It is layered on the multi library's public smm_*_device entry points and links that library and
 * the main one by name; all three must sit in one directory.  Status codes are snappy_mi355x.h's
 * plus SMQ_ERR_* below.
 *
 * ---- Thrift compact protocol, as far as a PageHeader needs it ------------------------------
 * A struct is fields up to a 0x00 byte.  A field header is (delta << 4) | type, the field's id
 * being the previous id of that struct (0 at first) plus delta; with delta == 0 the id follows as a
 * zigzag varint of at most 3 bytes.  The types: 1 and 2 bool true and false (no bytes), 3 a byte,
 * 4, 5 and 6 zigzag varints of at most 3, 5 and 10 bytes (i16, i32, i64), 7 eight bytes, 8 a varint
 * length (at most 5 bytes) and that many bytes, 9 and 10 a list and a set: (size << 4) | elemtype,
 * with a varint size (at most 5 bytes) behind it when the nibble is 15, bool elements one byte
 * each; 11 a map: a varint size (at most 5 bytes), then, when it is not 0, one byte
 * (keytype << 4) | valuetype and the pairs; 12 a struct.
 * A field this library does not know, or knows under another type, is skipped by these rules at
 * any nesting up to depth 8: the PageHeader is depth 1, and every struct, list, set or map inside
 * another is one deeper.  Skipping a binary only advances the position.  Depth 9, a type nibble of
 * 0 (other than a struct's end) or above 12, or a varint with more bytes than its type allows is
 * SMQ_ERR_HEADER; running out of bytes is SMQ_ERR_TRUNCATED.  No byte at or behind the chunk's end
 * is ever read.
 *
 * ---- the walk, from pos = 0 and total = 0 over the n bytes of a chunk --------------------------
 *   pos == n ends the walk (SM_OK): the empty chunk is valid and empty;
 *   the PageHeader at pos: 1 type, 2 uncompressed_page_size, 3 compressed_page_size, 4 crc (all
 *     i32; of a repeated field the last counts), 5 data_page_header {1 num_values, 2 encoding},
 *     7 dictionary_page_header {1 num_values, 2 encoding}, 8 data_page_header_v2 {1 num_values,
 *     4 encoding, 5 definition_levels_byte_length, 6 repetition_levels_byte_length (all i32; a
 *     missing one is 0), 7 is_compressed (a bool, true when missing)};
 *   field 1, 2 or 3 missing or not an i32, or a size below 0: SMQ_ERR_HEADER;
 *   type 0 (DATA_PAGE) without field 5, 2 (DICTIONARY_PAGE) without 7, 3 (DATA_PAGE_V2) without 8:
 *     SMQ_ERR_HEADER;
 *   type 3: levels = repetition + definition byte lengths; one of them below 0, or levels above
 *     either page size: SMQ_ERR_HEADER.  Types 0 and 2: levels = 0;
 *   compressed_page_size > the bytes left behind the header: SMQ_ERR_TRUNCATED;
 *   type 1 (INDEX_PAGE) and every other type: the page is recorded and stepped over, as readers do
 *     -- no output, no decode and no CRC check, flags without SMQ_PAGE_COMPRESSED;
 *   types 0, 2, 3: the body's first `levels` bytes are stored as they are.  With sec = the body
 *     behind them and want = uncompressed_page_size - levels:
 *       type 3 with is_compressed false: len(sec) != want is SMQ_ERR_SIZE_MISMATCH; sec is stored;
 *       else len(sec) == 0: want != 0 is SMQ_ERR_SIZE_MISMATCH; nothing is decoded;
 *       else sec is one raw Snappy stream: its varint, parsed by the raw decoder's rule over its
 *         first min(len(sec), 5) bytes, must parse (else SM_ERR_VARINT) and equal want (else
 *         SMQ_ERR_SIZE_MISMATCH); the page has SMQ_PAGE_COMPRESSED;
 *     the page is recorded, its output at total; total += uncompressed_page_size;
 *   pos moves behind the body.
 * A chunk's output is therefore its pages' uncompressed bytes back to back -- what a CPU reader
 * holds after decompression: of a v2 data page the level bytes and then the values.
 *
 * The optional crc of a PageHeader is the CRC-32 (IEEE: reflected polynomial 0xEDB88320, init and
 * final xor 0xffffffff; "123456789" gives 0xCBF43926) of the page's body as it is stored.
 *
 * Threading: an smq_ctx owns an smm_ctx and scratch, and one caller at a time may use it, as an
 * smo_ctx: the *_device calls keep their per-call arrays in the ctx's scratch, so two of them on one
 * ctx must be on one stream (or ordered by the caller), and a call that grows the scratch waits for
 * the device first (hipFree).  smq_uncompress_chunks locks the ctx.  No *_device call synchronises
 * otherwise: every decision is taken on the device.
 */
#ifndef SNAPPY_MI355X_PARQUET_H_
#define SNAPPY_MI355X_PARQUET_H_

#include <stddef.h>
#include <stdint.h>

#include "snappy_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
  SMQ_ERR_HEADER = 72,        /* a PageHeader that is malformed or lacks a field the page needs */
  SMQ_ERR_TRUNCATED = 73,     /* a PageHeader or a page body runs past the end of the chunk */
  SMQ_ERR_SIZE_MISMATCH = 74, /* a values section does not have the length its header declares */
  SMQ_ERR_CRC = 75            /* a page body does not have the CRC-32 of its header */
};

#define SMQ_PAGE_DATA 0
#define SMQ_PAGE_INDEX 1
#define SMQ_PAGE_DICTIONARY 2
#define SMQ_PAGE_DATA_V2 3

#define SMQ_PAGE_HAS_CRC 1u    /* flags: the header carries a crc */
#define SMQ_PAGE_COMPRESSED 2u /* flags: the values section is a raw Snappy stream that is decoded */

#define SMQ_MAX_DEPTH 8

typedef struct smq_ctx smq_ctx;

/* a chunk's pages, as parallel arrays (host memory for smq_index, device memory for the device call) */
typedef struct smq_pages {
  uint64_t* hdr_off;   /* the PageHeader, from the chunk's first byte; the body is at hdr_off + hdr_len */
  uint32_t* hdr_len;
  uint32_t* body_len;  /* compressed_page_size */
  uint32_t* usize;     /* uncompressed_page_size */
  uint32_t* levels;    /* the stored level bytes at the body's start (v2 data pages), else 0 */
  uint64_t* out_off;   /* the page's output, from the chunk's first output byte */
  int32_t* num_values; /* of the page type's own header; 0 for a page that is stepped over */
  int32_t* type;       /* PageType: SMQ_PAGE_*, or whatever else the header holds */
  int32_t* encoding;   /* of the page type's own header; 0 for a page that is stepped over */
  uint32_t* flags;     /* SMQ_PAGE_HAS_CRC | SMQ_PAGE_COMPRESSED */
  uint32_t* crc;       /* the header's crc, 0 without one */
} smq_pages;

typedef struct smq_summary {
  uint64_t total_length; /* the uncompressed sizes: of the whole chunk, or before the error */
  uint32_t npages;       /* pages recorded: all of them, or those before the error */
  int32_t status;        /* SM_OK, a walk error, or SM_BUFFER_TOO_SMALL (npages > max_pages) */
} smq_summary;

/* ---- host helpers (no device needed) ------------------------------------------------- */
/* the SMQ_ERR_* texts, else the main library's */
const char* smq_status_message(sm_status st);
/* library build identification ("snappy_mi355x_parquet gfx950 <source hash>") */
const char* smq_version(void);
/* the most pages an n-byte chunk can hold: n / 7 (the shortest PageHeader is three i32 fields of
 * two bytes each and the struct's end, of an index page without a body) */
uint64_t smq_max_pages(uint64_t n);
/* The walk over a host buffer.  pages NULL: count only.  Entries [0, min(npages, max_pages)) are
 * stored; more pages than max_pages with pages given: SM_BUFFER_TOO_SMALL.  Returns
 * summary->status; SM_ERR_ARGUMENT for a NULL summary or buffer or a NULL array in pages. */
sm_status smq_index(const uint8_t* buf, size_t n, const smq_pages* pages, uint32_t max_pages, smq_summary* summary);
sm_status smq_uncompressed_length(const uint8_t* buf, size_t n, size_t* result);
/* The plan of smq_uncompress_chunks_device on the host, by the code the kernels run: per chunk
 * status[c] (the walk's error, SM_BUFFER_TOO_SMALL against out_cap[c], or SM_OK: what is known
 * before any byte is decoded), out_len[c] (the size needed, or the uncompressed sizes before the
 * error) and first[0, nchunks] (the exclusive scan of the slots: a chunk that is decoded takes one
 * per page, any other none).  *total_pages = the slots, *total_fragments = the sum of
 * smm_fragment_count(want) over the pages with SMQ_PAGE_COMPRESSED: the two bounds of the device
 * call.  out_cap NULL: no limit; every output pointer may be NULL.  More slots than max_pages:
 * SM_BUFFER_TOO_SMALL, every status SM_ERR_ARGUMENT and every out_len 0, as the device call leaves
 * them. */
sm_status smq_chunks_plan(const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t nchunks,
                          const uint64_t* out_cap, uint32_t max_pages, uint32_t* first, uint64_t* out_len, int32_t* status,
                          uint64_t* total_pages, uint64_t* total_fragments);
/* the device memory an smq_uncompress_chunks_device call of that shape keeps in the ctx, the
 * smm_ctx's own scratch and the CRC tables not counted */
size_t smq_chunks_scratch_bytes(uint32_t nchunks, uint32_t max_pages, uint32_t max_fragments);

/* ---- context ------------------------------------------------------------------------ */
/* NULL without a usable device */
smq_ctx* smq_ctx_create(int device);
void smq_ctx_destroy(smq_ctx* ctx);
/* diagnostic: smm_ctx_last_indexed of the ctx's smm_ctx -- the number of values sections the last
 * decode call took by fragments; waits for the device.  -1 for a NULL ctx or before the first decode. */
int smq_ctx_last_indexed(smq_ctx* ctx);

/* ---- device memory, asynchronous on `stream` (a hipStream_t; NULL = the default stream) ----
 * The offset, length and capacity arrays are trusted; the chunk bytes are not.
 *
 * Decode.  Chunk c = d_in[d_in_off[c] .. +d_in_len[c]) at any alignment into
 * d_out[d_out_off[c] .. +d_out_cap[c]).  Per chunk:
 *   an error from the walk: d_status[c] = that status, d_out_len[c] = the uncompressed sizes before
 *     the error; nothing of it is decoded and it takes no slots;
 *   well formed but longer than d_out_cap[c]: SM_BUFFER_TOO_SMALL, d_out_len[c] = the size needed;
 *     nothing is decoded;
 *   otherwise every page takes a slot and goes to d_out_off[c] plus the uncompressed sizes before
 *     it: level bytes and stored sections are copied, a compressed section decodes with capacity
 *     exactly `want`.  A page's status: SMQ_ERR_CRC when verify_crc is not 0, its header carries a
 *     crc and the body's CRC-32 differs (this outranks the decoder's status); else the raw decoder's
 *     status of its compressed section; else SM_OK.  d_status[c] = the first failing page's status
 *     in page order, else SM_OK (a failing page does not stop the others); d_out_len[c] = the total.
 * No byte is read outside a chunk's own input range and none written outside
 * [d_out_off[c], d_out_off[c] + d_out_cap[c]).
 * max_pages: the caller's bound on the slots (smq_chunks_plan, or smq_max_pages summed); it sizes
 * the launches and the scratch.  When the device counts more, every d_status[c] = SM_ERR_ARGUMENT,
 * every d_out_len[c] = 0 and nothing is written to d_out.
 * d_page_first (nchunks + 1) and d_page_status (max_pages), both or neither: the exclusive scan of
 * the slots, and per slot its page's status (0 for a slot no page took).  d_pages, optional: the page
 * table, a host struct of device arrays of max_pages entries each, slot d_page_first[c] + k holding
 * page k of chunk c as smq_index gives it (a slot no page took: zeros).
 * max_fragments is a speed hint only, as in smo_uncompress_streams_device: the compressed sections
 * go through smm_index_device with that bound and then through smm_uncompress_device with the index
 * it built, so a page of more than 64 KiB that a block compressor wrote decodes fragment by
 * fragment.  With 0 no index is built.
 * There is no host synchronisation except when the scratch grows.
 * Returns SM_ERR_ARGUMENT for a NULL ctx or array, one of d_page_first / d_page_status without the
 * other, a NULL array in d_pages, nchunks or max_pages above 0x7fffffff; SM_ERR_DEVICE when a launch
 * or an allocation failed. */
sm_status smq_uncompress_chunks_device(smq_ctx* ctx, const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                       uint32_t nchunks, uint32_t max_pages, uint32_t max_fragments, int verify_crc,
                                       uint8_t* d_out, const uint64_t* d_out_off, const uint64_t* d_out_cap,
                                       uint64_t* d_out_len, int32_t* d_status, uint32_t* d_page_first,
                                       const smq_pages* d_pages, int32_t* d_page_status, void* stream);

/* CRC-32 (IEEE) of n byte ranges: d_crc[i] = the CRC of d_in[d_off[i] .. +d_len[i]), at any
 * alignment and of any length up to 0x7fffffff (the arrays are trusted).  A range is cut into
 * segments of 64 KiB, the short one first, one workgroup each. */
sm_status smq_crc32_device(smq_ctx* ctx, const uint8_t* d_in, const uint64_t* d_off, const uint64_t* d_len, uint32_t n,
                           uint32_t* d_crc, void* stream);

/* ---- host memory (one upload, the device path, one download; synchronous; locks the ctx) ----
 * The arrays as above, in host memory; the two bounds are counted here.  Only each chunk's own bytes
 * are copied back: out is otherwise untouched. */
sm_status smq_uncompress_chunks(smq_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len,
                                uint32_t nchunks, int verify_crc, uint8_t* out, const uint64_t* out_off,
                                const uint64_t* out_cap, uint64_t* out_len, int32_t* status);

#ifdef __cplusplus
}
#endif
#endif /* SNAPPY_MI355X_PARQUET_H_ */
