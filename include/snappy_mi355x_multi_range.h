/*
 * snappy_mi355x_multi_range.h -- ranged decode of indexed raw Snappy streams on the device: further
 * entry points of libsnappy_mi355x_multi.so (snappy_mi355x_multi.h, whose smm_ctx and threading
 * rules they share).
 *
 * A raw stream from any block compressor is independently decodable 64 KiB fragments
 * (src/Snappy.jl:29-33), and the index of snappy_mi355x_multi.h says where each one starts:
 * smm_compress_device hands it out, smm_index_device builds it for streams a CPU compressor wrote.
 * With it, bytes [lo, lo + len) of a stream's content cost the fragments they touch, not the
 * stream: a batch of ranges over a batch of streams is planned on the device, every touched
 * fragment is decoded by the main library's fragment decoder, and only the asked bytes are stored.
 *
 * The index is an untrusted hint, as it is for smm_uncompress_device: no value in it causes a read
 * outside a stream's input or a write outside a range's output.  Status codes are snappy_mi355x.h's.
 */
#ifndef SNAPPY_MI355X_MULTI_RANGE_H_
#define SNAPPY_MI355X_MULTI_RANGE_H_

#include <stddef.h>
#include <stdint.h>

#include "snappy_mi355x_multi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- host helpers (no device needed) ------------------------------------------------- */
/* The fragments that bytes [lo, lo + len) touch: floor((lo + len - 1) / 65536) - floor(lo / 65536)
 * + 1, the sum taken in 64 bits; 0 for len == 0.  Exact for every stream: raw fragments are always
 * 65,536 bytes of content apart. */
uint32_t smm_range_fragment_count(uint32_t lo, uint32_t len);
/* the device memory an smm_uncompress_ranges_device call of that shape keeps in the ctx: the
 * per-range arrays, the per-slot arrays (a slot: one touched fragment of one range), and
 * min(2 * nranges, max_range_fragments) edge slots of 65,536 bytes (one at the least) */
size_t smm_range_scratch_bytes(uint32_t nranges, uint32_t max_range_fragments);
/* The plan of smm_uncompress_ranges_device (below) over HOST arrays: the same rules, compiled from
 * the same code, with nothing decoded.  Per range r: first[r] / count[r] = the touched fragments
 * [first, first + count) of its stream (0, 0 for an empty range and for one that fails the
 * stream-level rule), and status[r] = what is known before any fragment is decoded: SM_OK, or
 * SM_ERR_ARGUMENT for a failed stream-level rule or a touched fragment whose index entry fails.
 * *total = the sum of count.  When *total > max_range_fragments the call returns
 * SM_BUFFER_TOO_SMALL and every status[r] = SM_ERR_ARGUMENT (first, count and *total still say what
 * the ranges need).  Each of first, count, status and total may be NULL.  Returns SM_ERR_ARGUMENT
 * for another NULL array with nranges > 0; nranges == 0 returns SM_OK with *total = 0. */
sm_status smm_range_plan(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint32_t nstreams,
                         const uint32_t* frag_first, const uint32_t* frag_pos, uint32_t nentries,
                         const uint32_t* range_stream, const uint32_t* lo, const uint32_t* len, uint32_t nranges,
                         uint32_t max_range_fragments, uint32_t* first, uint32_t* count, int32_t* status,
                         uint64_t* total);

/* ---- device memory, asynchronous on `stream` (a hipStream_t; NULL = the default stream) ----
 * Ranged decode.  The streams are those of smm_uncompress_device: stream s is
 * d_in[d_in_off[s] .. +d_in_len[s]), with the index d_frag_first (nstreams + 1) and d_frag_pos
 * (nentries entries).  Range r asks for bytes [d_lo[r], d_lo[r] + d_len[r]) of the decoded content
 * of stream s = d_range_stream[r], written to d_out + d_out_off[r] (room: d_len[r] bytes, any
 * alignment).  lo and len are 32-bit; their sum is taken in 64 bits.
 *
 * d_len[r] == 0: nothing of the stream, the index or d_out is touched; d_status[r] = SM_OK and
 * d_out_len[r] = 0, whatever else holds for the range (except over the bound, below).
 *
 * The stream-level rule is decided before any fragment byte is read.  Each of these gives
 * d_status[r] = SM_ERR_ARGUMENT, d_out_len[r] = 0 and nothing written:
 *   - s >= nstreams;
 *   - n = d_in_len[s] is an error mark (n >= SM_OUT_LEN_ERROR);
 *   - the varint header does not parse (over the first min(n, 5) bytes; it gives the declared
 *     length D and its own length hv);
 *   - d_frag_first[s] > d_frag_first[s + 1], or d_frag_first[s + 1] > nentries;
 *   - d_frag_first[s + 1] - d_frag_first[s] != smm_fragment_count(D);
 *   - lo + len > D.
 * Only the two d_frag_first words of the named stream are read, and there is no pass over all
 * streams: the rest of d_frag_first may hold anything.  A stream with D <= 65536 is served: it has
 * one entry, hv.
 *
 * Touched fragments: f0 = lo >> 16 through f1 = (lo + len - 1) >> 16, one slot each.  Each is
 * checked as smm_uncompress_device checks it: fragment 0's position is hv, fragment f's bytes run
 * from its position (>= hv) to the next fragment's position (the last: to n), strictly increasing,
 * the end <= n.  A failing entry is that fragment's SM_ERR_ARGUMENT.  Only the entries f0 .. f1 + 1
 * of the stream are read: a range costs what it touches.
 * Decode: a touched fragment must decode to 65536 bytes (the stream's last: the remainder of D), as
 * sm_uncompress_fragments_device decides.  A 64 KiB fragment wholly inside the range decodes
 * straight to d_out_off[r] + 65536 f - lo; the at most two others (the first and the last touched:
 * partly covered, or the stream's short last fragment) decode into edge slots the ctx owns, and the
 * covered bytes are copied out.
 * Result: d_status[r] = SM_OK, d_out_len[r] = len and the bytes are decode(stream)[lo : lo + len];
 * or d_status[r] = the status of the first failing touched fragment in stream order and
 * d_out_len[r] = 0.  Damage in fragments the range does not touch is not seen.  A failing range's
 * bytes are unspecified but stay inside [d_out_off[r], +len).
 *
 * Foreign streams: one whose index could not be built (zeroed entries: smm_index_device reports
 * d_built[s] = 0) is SM_ERR_ARGUMENT; one whose tags align at the 64 KiB multiples but whose copies
 * reach back across them fails with the fragment decoder's status.  In both cases the caller
 * decodes that stream whole (smm_uncompress_device): there is no fallback here.
 * Leniency: a stray unparsed last byte at a fragment's end is accepted fragment by fragment, as the
 * raw fragment decoder accepts it; the decoder in stream order would parse it as a tag.
 *
 * max_range_fragments: the caller's bound on the sum of smm_range_fragment_count(lo, len) over the
 * ranges that pass the stream-level rule (smm_range_plan counts it); it sizes the launches and the
 * ctx's scratch.  Over the bound -- the device plan counts more slots -- every d_status[r] =
 * SM_ERR_ARGUMENT (an empty range's too), every d_out_len[r] = 0, and nothing is written to d_out.
 * A fragment that several ranges touch is decoded once per range.  Ranges whose outputs overlap
 * race.  No host synchronisation, except when the ctx's scratch has to grow (hipFree waits).
 * Returns SM_ERR_ARGUMENT for a NULL ctx or array; SM_ERR_DEVICE when a launch or the scratch
 * allocation failed; nranges == 0 returns SM_OK and touches nothing. */
sm_status smm_uncompress_ranges_device(smm_ctx* ctx, const uint8_t* d_in, const uint64_t* d_in_off,
                                       const uint32_t* d_in_len, uint32_t nstreams, const uint32_t* d_frag_first,
                                       const uint32_t* d_frag_pos, uint32_t nentries, const uint32_t* d_range_stream,
                                       const uint32_t* d_lo, const uint32_t* d_len, uint32_t nranges,
                                       uint32_t max_range_fragments, uint8_t* d_out, const uint64_t* d_out_off,
                                       uint32_t* d_out_len, int32_t* d_status, void* stream);

/* ---- host memory (H2D, the device path, D2H; synchronous; locks the ctx) -------------------
 * The arrays as above, in host memory; nentries = frag_first[nstreams] (at most 0x7fffffff) and
 * max_range_fragments are taken here.  The stream-level rule runs on the host first.  Each stream
 * that at least one range passes it on goes up once and whole, with its index entries.  A range
 * that fails it has its status from the host, and the device reads nothing for it: its stream does
 * not go up on its account.  A stream no range names is not read at all and may hold anything; of
 * a stream only failing ranges name, the host reads the first min(n, 5) bytes and its two
 * frag_first words, and no more.  Only each successful range's own len bytes are copied
 * back: out is otherwise untouched.  (Uploading only the touched fragments' bytes is not done: the
 * device rule reads the stream's varint, and a sliced index would need a second rule.) */
sm_status smm_uncompress_ranges(smm_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,
                                uint32_t nstreams, const uint32_t* frag_first, const uint32_t* frag_pos,
                                const uint32_t* range_stream, const uint32_t* lo, const uint32_t* len, uint32_t nranges,
                                uint8_t* out, const uint64_t* out_off, uint32_t* out_len, int32_t* status);

#ifdef __cplusplus
}
#endif
#endif /* SNAPPY_MI355X_MULTI_RANGE_H_ */
