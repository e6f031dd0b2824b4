// smt_kernels.hip -- batches of LevelDB table files (smt_index_tables_device,
// smt_uncompress_blocks_device, smt_uncompress_tables_device, smt_compress_blocks_device): gfx950
// kernels and their launchers (smt_internal.h).  Plumbing around the multi library's three device
// calls and the framing library's batched masked CRC-32C; the decisions are the shared rules of
// smt_format.h, taken per table and per block on the device, so a call needs no host
// synchronisation.  A table is a two-stage pipeline: its index block is decoded (or copied) into the
// scratch first, and the walk that finds the data blocks runs over those bytes; once the handles are
// known every block's head is independent of the others and is read by a thread of its own.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../common/smc_device.h"
#include "smt_format.h"
#include "smt_internal.h"

namespace smt {

namespace {

constexpr uint32_t kCopyRows = 4;   // workgroups that share one block's copy

// a thread's own bytes of global memory, one load each, at any alignment
struct DeviceFetch {
  const uint8_t* p;
  __device__ uint32_t operator()(uint64_t pos) const { return p[pos]; }
};

// Block j's arguments for the multi library's two calls, the copy and the checksum call.  A block
// that is not decoded is an empty stream with no room, which those calls return from at once.
__device__ inline void set_slot(const Decode& s, uint32_t j, bool live, uint64_t abs, uint32_t size, uint32_t type, uint32_t decl,
                                uint64_t out_off, bool verify) {
  const bool snappy = live && type == kSnappy;
  s.b_in_off[j] = live ? abs : 0u;
  s.b_in_len[j] = snappy ? size : 0u;
  s.b_cap[j] = snappy ? decl : 0u;
  s.b_out_off[j] = live ? out_off : 0u;
  s.b_copy[j] = live && type == kStored ? 1u : 0u;
  s.b_crc_off[j] = live ? abs : 0u;
  s.b_crc_len[j] = live && verify ? size + 1 : 0u;
}

}  // namespace

// ---- the index stage -----------------------------------------------------------------------------
// A thread per table: the footer, then the head of the index block it names.
__global__ __launch_bounds__(256) void k_tab_footer(DecodeArgs a) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.nt) return;
  const uint64_t n = a.in_len[t];
  DeviceFetch fetch{a.in + a.in_off[t]};
  Handle meta, index;
  const int32_t footer = read_footer(fetch, n, meta, index);
  uint32_t type = 0, stored = 0;
  uint64_t declared = 0;
  int32_t head = SM_OK;
  if (footer == SM_OK) {  // (the handle lies inside the table with its trailer)
    head = block_head(fetch, index.off, index.size, type, declared);
    stored = block_crc(fetch, index.off, index.size);
  }
  const bool ok = footer == SM_OK && head == SM_OK;
  a.s.ix_footer[t] = footer;
  a.s.ix_head[t] = head;
  a.s.ix_type[t] = type;
  a.s.ix_stored[t] = stored;
  a.s.ix_size[t] = footer == SM_OK ? (uint32_t)index.size : 0u;
  a.s.ix_len[t] = ok ? (uint32_t)declared : 0u;
  a.s.ix_in_off[t] = footer == SM_OK ? a.in_off[t] + index.off : 0u;
  a.s.t_len[t] = n;
  a.s.fail[t] = kNone;
  a.s.count[t] = 0;
}

// By one workgroup: the index blocks' places in the scratch (each at a 16-byte boundary) against
// max_index_bytes, then per table the arguments of the decode, the copy and the checksum call.
__global__ __launch_bounds__(256) void k_tab_place(DecodeArgs a) {
  __shared__ uint64_t sh[4];
  const uint64_t sum = smc::tile_scan(
      a.nt, sh, [&](uint32_t t) { return round16(a.s.ix_len[t]); }, [&](uint32_t t, uint64_t, uint64_t at) { a.s.ix_out_off[t] = at; });
  const bool over = sum > a.index_bytes;
  if (threadIdx.x == 0) {
    a.s.hdr->over = over ? 1u : 0u;
    a.s.hdr->total = 0;
  }
  for (uint32_t t = threadIdx.x; t < a.nt; t += 256) {
    const bool there = !over && a.s.ix_footer[t] == SM_OK;
    const bool live = there && a.s.ix_head[t] == SM_OK;
    const bool snappy = live && a.s.ix_type[t] == kSnappy;
    a.s.ix_live[t] = live ? 1 : 0;
    a.s.ix_in_len[t] = snappy ? a.s.ix_size[t] : 0u;
    a.s.ix_cap[t] = snappy ? a.s.ix_len[t] : 0u;
    if (!live) a.s.ix_out_off[t] = 0;
    a.s.ix_crc_off[t] = there ? a.s.ix_in_off[t] : 0u;
    a.s.ix_crc_len[t] = there && a.verify && a.s.ix_head[t] != SMT_ERR_TYPE ? a.s.ix_size[t] + 1 : 0u;
    a.s.ix_computed[t] = 0;
    a.s.ix_dec[t] = SM_OK;
  }
}

hipError_t launch_index_heads(const DecodeArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_tab_footer, dim3((a.nt + 255) / 256), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_tab_place, dim3(1), dim3(256), 0, s, a);
  return hipGetLastError();
}

// blockIdx.x = the table, blockIdx.y strides the bytes: a stored index block into the scratch
__global__ __launch_bounds__(256) void k_tab_copy(DecodeArgs a) {
  const uint32_t t = blockIdx.x;
  if (!a.s.ix_live[t] || a.s.ix_type[t] != kStored) return;
  smc::copy_bytes(a.in + a.s.ix_in_off[t], a.s.ix_len[t], a.s.index + a.s.ix_out_off[t], blockIdx.y * blockDim.x + threadIdx.x,
                  gridDim.y * blockDim.x);
}

// a thread per table: what is known before its index is walked (index_verdict)
__global__ __launch_bounds__(256) void k_tab_verdict(DecodeArgs a) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.nt) return;
  a.s.ix_status[t] = index_verdict(a.s.ix_footer[t], a.s.ix_head[t], a.verify != 0 && a.s.ix_crc_len[t] != 0, a.s.ix_stored[t],
                                   a.s.ix_computed[t], a.s.ix_type[t], a.s.ix_dec[t]);
}

// The counting walk, one wave per table, over the table's decoded index block in the scratch.  The
// walks of a workgroup's waves are independent: no barrier in here.
__global__ __launch_bounds__(256) void k_tab_count(DecodeArgs a) {
  const uint32_t t = smc::walker_index();
  if (t >= a.nt || a.s.hdr->over || a.s.ix_status[t] != SM_OK) return;
  smc::WindowFetch fetch{a.s.index + a.s.ix_out_off[t], a.s.ix_len[t], threadIdx.x & 63};
  const IndexWalk w = walk_index(fetch, a.s.ix_len[t], a.s.t_len[t], [](uint32_t, const Handle&) {});
  if (fetch.lane == 0) {
    a.s.count[t] = w.status == SM_OK ? w.nblocks : 0u;
    a.s.ix_status[t] = w.status;
  }
}

// The exclusive scan of the tables' entries against the bound m, by one workgroup.
__global__ __launch_bounds__(256) void k_tab_scan(DecodeArgs a) {
  __shared__ uint64_t sh[4];
  const uint64_t sum = smc::tile_scan(
      a.nt, sh, [&](uint32_t t) { return a.s.count[t]; }, [&](uint32_t t, uint64_t, uint64_t at) { a.s.first[t] = smc::sat32(at); });
  if (threadIdx.x == 0) {
    const bool over = a.s.hdr->over != 0 || sum > a.m;
    a.s.first[a.nt] = smc::sat32(sum);
    a.s.hdr->over = over ? 1u : 0u;
    a.s.hdr->total = over ? 0u : (uint32_t)sum;
  }
}

// The entries no table took (all of them over a bound) are marked; then the storing walk of the
// tables that have entries: entry k of table t is entry first[t] + k.
__global__ __launch_bounds__(256) void k_tab_fill(DecodeArgs a) {
  for (uint64_t j = (uint64_t)a.s.hdr->total + (uint64_t)blockIdx.x * 256u + threadIdx.x; j < a.m; j += (uint64_t)gridDim.x * 256u) {
    a.s.h_off[j] = 0;
    a.s.h_size[j] = 0;
    a.s.b_table[j] = kNone;
  }
  const uint32_t t = smc::walker_index();
  if (t >= a.nt || a.s.hdr->over) return;
  const uint32_t cnt = a.s.count[t], base = a.s.first[t];
  if (cnt == 0) return;
  smc::WindowFetch fetch{a.s.index + a.s.ix_out_off[t], a.s.ix_len[t], threadIdx.x & 63};
  const uint32_t lane = fetch.lane;
  walk_index(fetch, a.s.ix_len[t], a.s.t_len[t], [&](uint32_t k, const Handle& h) {
    if (lane != 0 || k >= cnt) return;
    const uint32_t j = base + k;
    a.s.h_off[j] = h.off;
    a.s.h_size[j] = h.size;
    a.s.b_table[j] = t;
    if (a.handle_off) a.handle_off[j] = h.off;
    if (a.handle_size) a.handle_size[j] = h.size;
  });
}

// the index call's results: over a bound SM_ERR_ARGUMENT and nothing else
__global__ __launch_bounds__(256) void k_tab_index_result(DecodeArgs a) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.nt) return;
  const bool over = a.s.hdr->over != 0;
  a.status[t] = over ? (int32_t)SM_ERR_ARGUMENT : a.s.ix_status[t];
  if (over || !a.block_first) return;
  a.block_first[t] = a.s.first[t];
  if (t == a.nt - 1) a.block_first[a.nt] = a.s.first[a.nt];
}

hipError_t launch_index_walk(const DecodeArgs& a, hipStream_t s) {
  const uint32_t walkers = (a.nt + smc::kWalkWaves - 1) / smc::kWalkWaves;
  hipLaunchKernelGGL(k_tab_copy, dim3(a.nt, kCopyRows), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_tab_verdict, dim3((a.nt + 255) / 256), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_tab_count, dim3(walkers), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_tab_scan, dim3(1), dim3(256), 0, s, a);
  if (a.m) hipLaunchKernelGGL(k_tab_fill, dim3(walkers), dim3(256), 0, s, a);
  if (!a.decode) hipLaunchKernelGGL(k_tab_index_result, dim3((a.nt + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError();
}

// ---- the block stage of the tables call ----------------------------------------------------------
// A thread per entry: the block's head, at most six bytes of it and the four of its checksum, at any
// alignment, all inside the table's range (the walk checked the handle against it).  A failing
// head bids for its table's first.
__global__ __launch_bounds__(256) void k_blk_head(DecodeArgs a) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.m) return;
  uint32_t type = 0, stored = 0;
  uint64_t declared = 0;
  int32_t head = SM_OK;
  const uint32_t t = j < a.s.hdr->total ? a.s.b_table[j] : kNone;
  if (t != kNone) {
    DeviceFetch fetch{a.in + a.in_off[t]};
    head = block_head(fetch, a.s.h_off[j], a.s.h_size[j], type, declared);
    stored = block_crc(fetch, a.s.h_off[j], a.s.h_size[j]);
    if (head != SM_OK) atomicMin(&a.s.fail[t], j);
  }
  a.s.b_head[j] = head;
  a.s.b_type[j] = type;
  a.s.b_decl[j] = head == SM_OK ? (uint32_t)declared : 0u;
  a.s.b_stored[j] = stored;
  a.s.b_computed[j] = 0;
  a.s.b_dec[j] = SM_OK;
}

// the scan of the declared lengths over all entries, by one workgroup
__global__ __launch_bounds__(256) void k_blk_scan(DecodeArgs a) {
  __shared__ uint64_t sh[4];
  const uint32_t used = a.s.hdr->total;
  const uint64_t sum = smc::tile_scan(
      used, sh, [&](uint32_t j) { return a.s.b_decl[j]; }, [&](uint32_t j, uint64_t, uint64_t at) { a.s.prefix[j] = at; });
  if (threadIdx.x == 0) a.s.prefix[used] = sum;
}

// A thread per table: its status before any decode (table_plan) and its length -- the declared
// lengths of its blocks, or of those before its first failing head.
__global__ __launch_bounds__(256) void k_tab_plan(DecodeArgs a) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.nt) return;
  if (a.s.hdr->over) {
    a.s.t_pre[t] = SM_ERR_ARGUMENT;
    a.status[t] = SM_ERR_ARGUMENT;
    a.out_len[t] = 0;
    return;
  }
  const uint32_t lo = a.s.first[t], hi = a.s.first[t + 1], f = a.s.fail[t];
  const uint64_t sum = a.s.prefix[f != kNone ? f : hi] - a.s.prefix[lo];
  a.s.t_pre[t] = table_plan(a.s.ix_status[t], f != kNone ? a.s.b_head[f] : (int32_t)SM_OK, sum, a.out_cap[t]);
  a.out_len[t] = sum;
  a.s.fail[t] = kNone;  // (from here on: the first block whose decode or checksum fails)
  if (a.block_first) {
    a.block_first[t] = lo;
    if (t == a.nt - 1) a.block_first[a.nt] = a.s.first[a.nt];
  }
}

// a thread per entry: its slot, and the caller's per-entry arrays
__global__ __launch_bounds__(256) void k_blk_place(DecodeArgs a) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.m) return;
  const uint32_t t = j < a.s.hdr->total ? a.s.b_table[j] : kNone;
  if (t == kNone) {
    set_slot(a.s, j, false, 0, 0, 0, 0, 0, false);
    return;
  }
  const uint64_t rel = a.s.prefix[j] - a.s.prefix[a.s.first[t]];
  set_slot(a.s, j, a.s.t_pre[t] == SM_OK, a.in_off[t] + a.s.h_off[j], (uint32_t)a.s.h_size[j], a.s.b_type[j], a.s.b_decl[j],
           a.out_off[t] + rel, a.verify != 0);
  if (a.block_out_off) a.block_out_off[j] = rel;
  if (a.block_len) a.block_len[j] = a.s.b_decl[j];
  if (a.block_status) a.block_status[j] = SM_OK;
}

hipError_t launch_block_plan(const DecodeArgs& a, hipStream_t s) {
  if (a.m) hipLaunchKernelGGL(k_blk_head, dim3((a.m + 255) / 256), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_blk_scan, dim3(1), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_tab_plan, dim3((a.nt + 255) / 256), dim3(256), 0, s, a);
  if (a.m) hipLaunchKernelGGL(k_blk_place, dim3((a.m + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError();
}

// ---- the handle-level call -----------------------------------------------------------------------
// a thread per block: its head by the caller's trusted handle, what is known before the decode, its slot
__global__ __launch_bounds__(256) void k_handle_plan(DecodeArgs a) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.m) return;
  DeviceFetch fetch{a.in};
  const uint64_t off = a.blk_off[j], size = a.blk_size[j];
  uint32_t type;
  uint64_t declared;
  int32_t st = block_head(fetch, off, size, type, declared);
  a.out_len[j] = st == SM_OK ? declared : 0u;
  if (st == SM_OK && declared > a.out_cap[j]) st = SM_BUFFER_TOO_SMALL;
  a.s.b_head[j] = st;
  a.s.b_type[j] = type;
  a.s.b_decl[j] = (uint32_t)declared;
  a.s.b_stored[j] = block_crc(fetch, off, size);
  a.s.b_computed[j] = 0;
  a.s.b_dec[j] = SM_OK;
  set_slot(a.s, j, st == SM_OK, off, (uint32_t)size, type, (uint32_t)declared, a.out_off[j], a.verify != 0);
}

hipError_t launch_handle_plan(const DecodeArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_handle_plan, dim3((a.m + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError();
}

// ---- both: the stored blocks, the verdicts -------------------------------------------------------
// blockIdx.x strides the blocks, blockIdx.y the bytes of one
__global__ __launch_bounds__(256) void k_blk_copy(DecodeArgs a, uint8_t* out) {
  for (uint32_t j = blockIdx.x; j < a.m; j += gridDim.x) {
    if (!a.s.b_copy[j]) continue;
    smc::copy_bytes(a.in + a.s.b_in_off[j], a.s.b_decl[j], out + a.s.b_out_off[j], blockIdx.y * blockDim.x + threadIdx.x,
                    gridDim.y * blockDim.x);
  }
}

hipError_t launch_block_copy(const DecodeArgs& a, uint8_t* out, hipStream_t s) {
  if (a.m) hipLaunchKernelGGL(k_blk_copy, dim3(a.m < 65535 ? a.m : 65535, kCopyRows), dim3(256), 0, s, a, out);
  return hipGetLastError();
}

// A thread per block: its verdict (block_verdict).  In the tables call a failing block bids for its
// table's first; in the handle-level call the verdict is the block's result.
__global__ __launch_bounds__(256) void k_blk_verdict(DecodeArgs a) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.m) return;
  if (!a.decode) {
    if (a.s.b_head[j] == SM_OK)
      a.status[j] = block_verdict(a.verify != 0, a.s.b_stored[j], a.s.b_computed[j], a.s.b_type[j], a.s.b_dec[j]);
    else a.status[j] = a.s.b_head[j];
    return;
  }
  const uint32_t t = j < a.s.hdr->total ? a.s.b_table[j] : kNone;
  if (t == kNone || a.s.t_pre[t] != SM_OK) return;
  const int32_t st = block_verdict(a.verify != 0, a.s.b_stored[j], a.s.b_computed[j], a.s.b_type[j], a.s.b_dec[j]);
  a.s.b_head[j] = st;
  if (a.block_status) a.block_status[j] = st;
  if (st != SM_OK) atomicMin(&a.s.fail[t], j);
}

__global__ __launch_bounds__(256) void k_tab_result(DecodeArgs a) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.nt || a.s.hdr->over) return;
  const int32_t pre = a.s.t_pre[t];
  const uint32_t f = a.s.fail[t];
  a.status[t] = pre != SM_OK ? pre : f != kNone ? a.s.b_head[f] : (int32_t)SM_OK;
}

hipError_t launch_block_result(const DecodeArgs& a, hipStream_t s) {
  if (a.m) hipLaunchKernelGGL(k_blk_verdict, dim3((a.m + 255) / 256), dim3(256), 0, s, a);
  if (a.decode) hipLaunchKernelGGL(k_tab_result, dim3((a.nt + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError();
}

// ---- compress ------------------------------------------------------------------------------------
// By one workgroup: the blocks against max_blocks, the scan of their stage slots against
// stage_bytes, their fragments against max_fragments.  Over a bound nothing is compressed.
__global__ __launch_bounds__(256) void k_ctab_plan(CompressArgs a) {
  __shared__ uint64_t sh[4];
  const uint32_t total = a.block_first[a.nt];
  const uint32_t used = total > a.m ? 0u : total;
  uint64_t mine = 0;  // the fragments of this thread's blocks: a sum, not a scan
  const uint64_t stage = smc::tile_scan(
      used, sh,
      [&](uint32_t j) {
        const uint32_t len = a.block_len[j];
        mine += encode_fragments(len);
        return stage_length(len);
      },
      [&](uint32_t j, uint64_t, uint64_t at) { a.s.slot_off[j] = at; });
  uint64_t frags;
  (void)smc::block_scan(mine, sh, frags);
  for (uint32_t t = threadIdx.x; t < a.nt; t += 256) a.s.fail[t] = kNone;
  if (threadIdx.x == 0) {
    const bool over = total > a.m || stage > a.stage_bytes || frags > a.max_fragments;
    a.s.hdr->over = over ? 1u : 0u;
    a.s.hdr->total = over ? 0u : total;
  }
}

// Slot j: its block, its table.  An unused slot (all of them over a bound) is an empty block that
// packs nothing.  A block too long for a handle bids for its table's first failure.
__global__ __launch_bounds__(256) void k_ctab_slots(CompressArgs a) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.m) return;
  const bool used = j < a.s.hdr->total;
  const uint32_t len = used ? a.block_len[j] : 0u;
  const uint32_t t = used ? smc::slot_owner(a.block_first, a.nt, j) : kNone;
  const bool fits = len <= kMaxSize;
  a.s.in_off[j] = used ? a.block_off[j] : 0u;
  a.s.in_len[j] = fits ? len : 0u;
  a.s.table[j] = t;
  a.s.crc_off[j] = 0;
  a.s.crc_len[j] = 0;
  if (!used) a.s.slot_off[j] = a.stage_bytes;  // (the spare bytes behind the stage)
  if (used && !fits) atomicMin(&a.s.fail[t], j);
}

hipError_t launch_compress_plan(const CompressArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_ctab_plan, dim3(1), dim3(256), 0, s, a);
  if (a.m) hipLaunchKernelGGL(k_ctab_slots, dim3((a.m + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError();
}

// The 12.5 % decision per block and the scan of the packed sizes over all used slots, by one
// workgroup: a block's place in its table is its scan minus the scan at its table's first block.
__global__ __launch_bounds__(256) void k_ctab_sizes(CompressArgs a) {
  __shared__ uint64_t sh[4];
  const uint32_t used = a.s.hdr->total;
  const uint64_t sum = smc::tile_scan(
      used, sh,
      [&](uint32_t j) -> uint64_t {
        const uint32_t len = a.s.in_len[j];
        const bool keep = keep_compressed(a.s.comp_status[j], a.s.comp_len[j], len);
        a.s.type[j] = keep ? kSnappy : kStored;
        a.s.chosen[j] = keep ? a.s.comp_len[j] : len;
        return max_block_length(a.s.chosen[j]);
      },
      [&](uint32_t j, uint64_t, uint64_t at) { a.s.size_scan[j] = at; });
  if (threadIdx.x == 0) a.s.size_scan[used] = sum;
}

// blockIdx.x strides the slots, blockIdx.y the contents of one; the first row also writes the type
// byte, the handle and the checksum call's range (the contents and the type byte)
__global__ __launch_bounds__(256) void k_ctab_pack(CompressArgs a) {
  const uint32_t used = a.s.hdr->total;
  for (uint32_t j = blockIdx.x; j < used; j += gridDim.x) {
    const uint32_t t = a.s.table[j];
    if (a.s.fail[t] != kNone) continue;
    const uint32_t c = a.s.chosen[j], type = a.s.type[j];
    const uint64_t rel = a.s.size_scan[j] - a.s.size_scan[a.block_first[t]];
    uint8_t* const d = a.out + a.out_off[t] + rel;
    const uint8_t* const src = type == kSnappy ? a.s.stage + a.s.slot_off[j] : a.in + a.s.in_off[j];
    if (blockIdx.y == 0 && threadIdx.x == 0) {
      d[c] = (uint8_t)type;
      a.handle_off[j] = rel;
      a.handle_size[j] = c;
      a.s.crc_off[j] = a.out_off[t] + rel;
      a.s.crc_len[j] = c + 1;
    }
    smc::copy_bytes(src, c, d, blockIdx.y * blockDim.x + threadIdx.x, gridDim.y * blockDim.x);
  }
}

hipError_t launch_compress_pack(const CompressArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_ctab_sizes, dim3(1), dim3(256), 0, s, a);
  if (a.m) hipLaunchKernelGGL(k_ctab_pack, dim3(a.m < 65535 ? a.m : 65535, kCopyRows), dim3(256), 0, s, a);
  return hipGetLastError();
}

// a thread per block: the four bytes of its masked checksum behind the type byte, little-endian,
// byte by byte (a trailer sits at any alignment)
__global__ __launch_bounds__(256) void k_ctab_crc(CompressArgs a) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.s.hdr->total || a.s.crc_len[j] == 0) return;
  uint8_t* const p = a.out + a.s.crc_off[j] + a.s.crc_len[j];
  const uint32_t c = a.s.crc[j];
  for (uint32_t i = 0; i < 4; ++i) p[i] = (uint8_t)(c >> (8 * i));
}

__global__ __launch_bounds__(256) void k_ctab_result(CompressArgs a) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.nt) return;
  const bool over = a.s.hdr->over != 0;
  const bool failed = !over && a.s.fail[t] != kNone;
  a.status[t] = over ? (int32_t)SM_ERR_ARGUMENT : failed ? (int32_t)SM_ERR_INPUT_TOO_LARGE : (int32_t)SM_OK;
  a.out_len[t] = over || failed ? 0u : a.s.size_scan[a.block_first[t + 1]] - a.s.size_scan[a.block_first[t]];
}

hipError_t launch_compress_result(const CompressArgs& a, hipStream_t s) {
  if (a.m) hipLaunchKernelGGL(k_ctab_crc, dim3((a.m + 255) / 256), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_ctab_result, dim3((a.nt + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace smt
