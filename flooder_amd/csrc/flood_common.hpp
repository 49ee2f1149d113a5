// flood_common.hpp - helpers shared by the kernels of libflooder_hip.so (internal, not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <type_traits>

#include "../../include/flooder_hip.h"

namespace flooder {

constexpr uint32_t INF_BITS = 0x7f800000u;

// the tuning options, one `extern int g_<name>;` per row of flood_options.def (defined in flood_kernels.hip)
#define FLOODER_OPTION(name, def, lo, hi, desc) extern int g_##name;
#define FLOODER_OPTION_LIST(name, def, desc, ...) extern int g_##name;
#include "flood_options.def"
#undef FLOODER_OPTION
#undef FLOODER_OPTION_LIST
// face planes of every simplex (flood_cell.hip: simplex_planes_kernel), 24 floats per simplex
int launch_simplex_planes(int dim, const float* verts, int k1, int64_t n_simplices, float* tab, hipStream_t st);
char* err_buf();
int fail(int code, const char* msg);
// fail with a formatted message (internal: the library's list of exported symbols stays what it was)
int failf(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3), visibility("hidden")));
int check_launch(const char* what);

__host__ __device__ constexpr int padded_dim(int dim) { return dim <= 2 ? 2 : (dim <= 4 ? 4 : 8); }

// One padded row (DP floats) with a single vector load (per-lane address).
template <int DP>
__device__ __forceinline__ void load_row(const float* __restrict__ p, float (&out)[DP]) {
  if constexpr (DP == 2) {
    float2 t = *reinterpret_cast<const float2*>(p);
    out[0] = t.x; out[1] = t.y;
  } else if constexpr (DP == 4) {
    float4 t = *reinterpret_cast<const float4*>(p);
    out[0] = t.x; out[1] = t.y; out[2] = t.z; out[3] = t.w;
  } else {
    float4 a = *reinterpret_cast<const float4*>(p);
    float4 b = *reinterpret_cast<const float4*>(p + 4);
    out[0] = a.x; out[1] = a.y; out[2] = a.z; out[3] = a.w;
    out[4] = b.x; out[5] = b.y; out[6] = b.z; out[7] = b.w;
  }
}

__device__ __forceinline__ int wave_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

__device__ __forceinline__ int64_t wave_uniform64(int64_t v) {
  uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)(v & 0xffffffffu));
  uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// Wave-uniform rows come in through the scalar cache: the pointer is cast to the constant address
// space so each padded row is one s_load_dwordx2/x4/x8 into SGPRs, and the VALU reads the
// coordinates as scalar operands (no LDS staging, no barrier, no VGPR per candidate).
typedef float v2f __attribute__((ext_vector_type(2)));

template <int DP>
struct RowVec {
  typedef float type __attribute__((ext_vector_type(DP)));
};

template <int DP>
__device__ __forceinline__ typename RowVec<DP>::type load_uniform_row(const float* p) {
  typedef typename RowVec<DP>::type vec_t;
  typedef const __attribute__((address_space(4))) vec_t* cptr_t;
  return *((cptr_t)(uintptr_t)p);
}

// ---- sharded work queue of the persistent kernels.  One returning atomic on ONE head word serves ~88 pops per
// microsecond chip-wide (MI355X_MICROARCH.md, "dequeue") - half a million chunks of a cfg 5 sweep would spend 5.7 ms
// just queueing for it.  FLOODER_QUEUE_SHARDS heads, 128 B apart; item i lives in shard i % SHARDS (every shard keeps
// the global order); a wave starts at its home shard and moves on, for good, when a shard is exhausted.
constexpr int QSHARDS = FLOODER_QUEUE_SHARDS;
constexpr int QSTRIDE = FLOODER_QUEUE_WORDS / FLOODER_QUEUE_SHARDS;
__device__ __forceinline__ int64_t queue_pop(int32_t* __restrict__ heads, int& shard, int& tried, int64_t n_items, int lane) {
  // (shard and tried are wave-uniform by construction; say so, or they cost vector registers in kernels that sit at
  // their register limit: the cell sweep went from 0 to 21 spilled VGPRs = 91 MB of scratch writes per launch)
  shard = __builtin_amdgcn_readfirstlane(shard);
  tried = __builtin_amdgcn_readfirstlane(tried);
  while (tried < QSHARDS) {
    int j = 0;
    if (lane == 0) j = atomicAdd(&heads[shard * QSTRIDE], 1);
    j = __builtin_amdgcn_readfirstlane(j);
    const int64_t item = (int64_t)j * QSHARDS + shard;
    if (item < n_items) return item;
    shard = shard + 1 == QSHARDS ? 0 : shard + 1;
    ++tried;
  }
  return -1;
}

// ---- the same queue, XCD-local.  The eight XCDs have an L2 each (4 MB, not coherent with the others); items that
// follow each other in a queue are neighbours in space - the ~20 chunks of a simplex share most of their leaves, the
// next simplex of the axis-ordered queue many - and the interleaved queue above deals them to all eight L2s (cfg 5:
// 17 GB of L2 misses per launch for a 256 MB cloud).  Here item blocks of 2^blk CONSECUTIVE items go to the shards in
// turn, shards 2x and 2x+1 are the home of the waves of XCD x (HW_REG_XCC_ID), and a wave leaves its XCD's shards
// only when both are dry: j-th pop of shard h -> item ((j >> blk) * QSHARDS + h) << blk | (j & (2^blk - 1)), which
// grows with j, so a shard is exhausted at the first item past the end.  Shards are visited in the order
// home ^ 0, 1, 2 ...: the partner shard of the own XCD first, then another XCD's pair, a different one for every XCD.
__device__ __forceinline__ int xcc_id() { return (int)__builtin_amdgcn_s_getreg(20 | (3 << 11)) & 7; }  // hwreg(HW_REG_XCC_ID, 0, 4)
static_assert(FLOODER_QUEUE_SHARDS == 16, "two shards per XCD");
__device__ __forceinline__ int queue_home_local(int wave_in_block) { return xcc_id() * 2 + (wave_in_block & 1); }
__device__ __forceinline__ int64_t queue_pop_local(int32_t* __restrict__ heads, int home, int& tried, int64_t n_items, int lane, int blk) {
  home = __builtin_amdgcn_readfirstlane(home);
  tried = __builtin_amdgcn_readfirstlane(tried);
  while (tried < QSHARDS) {
    const int shard = home ^ tried;
    int j = 0;
    if (lane == 0) j = atomicAdd(&heads[shard * QSTRIDE], 1);
    j = __builtin_amdgcn_readfirstlane(j);
    const int64_t item = ((((int64_t)(j >> blk) * QSHARDS + shard) << blk) | (int64_t)(j & ((1 << blk) - 1)));
    if (item < n_items) return item;
    ++tried;
  }
  return -1;
}

// ---- 64-lane reductions on the DPP network (no LDS): result is wave-uniform.
// FLOODER_DPP_ASM (default): every step is ONE instruction - the operation itself with the DPP lane pattern on its
// first operand (v_min_f32_dpp x, x, x quad_perm:...; a lane whose source lane is masked off keeps x).  Written through
// __builtin_amdgcn_update_dpp the compiler emits a copy, the permuting move, a canonicalising max (floats) or a
// compare + select (unsigned) and the operation: 3 - 4 vector instructions per step, 18 - 24 per reduction, in
// kernels whose searches are chains of such reductions.  (s_nop 1: the two wait states a DPP read needs after the
// vector write of its source, which the compiler cannot place inside an asm block; the block OPENS with s_nop 4: five
// wait states cover a VALU write of EXEC directly in front of it as well - hipcc's wave64 control flow writes EXEC with
// scalar instructions today, tests/test_host.py greps the ISA for v_cmpx, but nothing here depends on that any more.)
#ifndef FLOODER_DPP_ASM
#define FLOODER_DPP_ASM 1
#endif
#define FLOODER_DPP_REDUCE(OP, x)                                                   \
  asm volatile("s_nop 4\n\t" OP " %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t" \
               "s_nop 1\n\t" OP " %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t" \
               "s_nop 1\n\t" OP " %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"     \
               "s_nop 1\n\t" OP " %0, %0, %0 row_mirror row_mask:0xf bank_mask:0xf\n\t"          \
               "s_nop 1\n\t" OP " %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"        \
               "s_nop 1\n\t" OP " %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"        \
               "s_nop 1"                                                            \
               : "+v"(x))
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_move(float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(x), __float_as_int(x), CTRL, ROW_MASK, 0xF, false));
}

__device__ __forceinline__ float wave_min_f32(float x) {
#if FLOODER_DPP_ASM
  FLOODER_DPP_REDUCE("v_min_f32_dpp", x);
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 63));
#endif
  x = __builtin_fminf(x, dpp_move<0xB1, 0xF>(x));   // quad_perm [1,0,3,2]
  x = __builtin_fminf(x, dpp_move<0x4E, 0xF>(x));   // quad_perm [2,3,0,1]
  x = __builtin_fminf(x, dpp_move<0x141, 0xF>(x));  // row_half_mirror
  x = __builtin_fminf(x, dpp_move<0x140, 0xF>(x));  // row_mirror: every row of 16 holds its min
  x = __builtin_fminf(x, dpp_move<0x142, 0xA>(x));  // row_bcast15 into rows 1 and 3
  x = __builtin_fminf(x, dpp_move<0x143, 0xC>(x));  // row_bcast31 into rows 2 and 3
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 63));
}

__device__ __forceinline__ float wave_max_f32(float x) {
#if FLOODER_DPP_ASM
  FLOODER_DPP_REDUCE("v_max_f32_dpp", x);
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 63));
#endif
  x = __builtin_fmaxf(x, dpp_move<0xB1, 0xF>(x));
  x = __builtin_fmaxf(x, dpp_move<0x4E, 0xF>(x));
  x = __builtin_fmaxf(x, dpp_move<0x141, 0xF>(x));
  x = __builtin_fmaxf(x, dpp_move<0x140, 0xF>(x));
  x = __builtin_fmaxf(x, dpp_move<0x142, 0xA>(x));
  x = __builtin_fmaxf(x, dpp_move<0x143, 0xC>(x));
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 63));
}

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_move_u32(uint32_t x) {
  return (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, CTRL, ROW_MASK, 0xF, false);
}

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t x) {
#if FLOODER_DPP_ASM
  FLOODER_DPP_REDUCE("v_min_u32_dpp", x);
  return (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
#endif
  uint32_t t;
  t = dpp_move_u32<0xB1, 0xF>(x); x = t < x ? t : x;
  t = dpp_move_u32<0x4E, 0xF>(x); x = t < x ? t : x;
  t = dpp_move_u32<0x141, 0xF>(x); x = t < x ? t : x;
  t = dpp_move_u32<0x140, 0xF>(x); x = t < x ? t : x;
  t = dpp_move_u32<0x142, 0xA>(x); x = t < x ? t : x;
  t = dpp_move_u32<0x143, 0xC>(x); x = t < x ? t : x;
  return (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
}

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t x) {
#if FLOODER_DPP_ASM
  FLOODER_DPP_REDUCE("v_max_u32_dpp", x);
  return (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
#endif
  uint32_t t;
  t = dpp_move_u32<0xB1, 0xF>(x); x = t > x ? t : x;
  t = dpp_move_u32<0x4E, 0xF>(x); x = t > x ? t : x;
  t = dpp_move_u32<0x141, 0xF>(x); x = t > x ? t : x;
  t = dpp_move_u32<0x140, 0xF>(x); x = t > x ? t : x;
  t = dpp_move_u32<0x142, 0xA>(x); x = t > x ? t : x;
  t = dpp_move_u32<0x143, 0xC>(x); x = t > x ? t : x;
  return (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
}

__device__ __forceinline__ uint32_t wave_or_u32(uint32_t x) {
#if FLOODER_DPP_ASM
  FLOODER_DPP_REDUCE("v_or_b32_dpp", x);
  return (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
#endif
  x |= dpp_move_u32<0xB1, 0xF>(x);
  x |= dpp_move_u32<0x4E, 0xF>(x);
  x |= dpp_move_u32<0x141, 0xF>(x);
  x |= dpp_move_u32<0x140, 0xF>(x);
  x |= dpp_move_u32<0x142, 0xA>(x);
  x |= dpp_move_u32<0x143, 0xC>(x);
  return (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
}

// Fused per-face maxima (flooder_sweep_cell_faces_f32 / flooder_finish_faces_f32): memb[r] = bit mask of the
// faces sample row r lies on, face_bits[s * n_faces + f] = running maximum of the d2 bits over the samples of
// face f whose nearest neighbour is settled.  In this mode the d2 buffer is scratch: only tiles handed to the
// finish are written, and bit 31 of a word marks a sample the cell sweep has already settled.
constexpr uint32_t SETTLED_BIT = 0x80000000u;
struct FaceAcc {
  const uint32_t* memb;
  uint32_t* face_bits;
  int n_faces;
  // per simplex: (largest upper bound of an open sample << 32 | tile id) of its flagged tiles, and the list of
  // simplices that have one; filled by the cell sweep's probe, read by the finish (may be null: no probe)
  unsigned long long* top;
  int32_t* top_list;
  int32_t* top_count;
  // slot of (simplex s, face f) in face_bits: slot[s * n_faces + f], or s * n_faces + f when null.  A triangle, an
  // edge or a vertex is a face of several simplices and its samples have bit-identical coordinates from each of them
  // (the zero weights contribute exact zeros): with one slot per DISTINCT face the first simplex that settles a face
  // lets every other one drop that face's samples in the finish.
  const int32_t* slot;
  // cell sweep -> finish: the probe's bound of every flagged tile (parallel to the flag list) and a histogram of the
  // bounds' top 12 bits: the finish starts the tiles with the largest bounds - the longest searches - first
  uint32_t* flag_key = nullptr;
  int32_t* flag_hist = nullptr;
  // face ownership (null: off; needs `slot`): owner[slot] = key of the ONE incident simplex that evaluates the samples
  // whose minimal face is that slot's face (owner_key below; 0 = nobody has asked), min_face[r] = minimal face of sample
  // row r (0: the full simplex - interior rows are always evaluated), chunk_faces / tile_faces = OR of 1 << min_face
  // over every aligned run of 256 / 64 rows.  A shared face's samples have bit-identical coordinates in every incident
  // simplex, so the others skip them; what they would have delivered to their own words comes back through the
  // closure of the face values (flood_finish.hip: face_closure_kernel).
  const unsigned long long* owner = nullptr;
  const uint8_t* min_face = nullptr;
  const uint32_t* chunk_faces = nullptr;
  const uint32_t* tile_faces = nullptr;
  // mask of the faces of simplex s whose own samples s evaluates (all 64 lanes active; wave-uniform result)
  __device__ __forceinline__ uint32_t own_mask(int64_t s, int lane) const {
    bool mine = false;
    if (lane > 0 && lane < n_faces) {
      const unsigned long long k =
          __hip_atomic_load(owner + slot[s * (int64_t)n_faces + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      mine = (uint32_t)k == ~(uint32_t)s;
    }
    return (uint32_t)__ballot(mine) | 1u;
  }
  __device__ __forceinline__ int64_t slot_of(int64_t s, int f) const {
    return slot ? (int64_t)slot[s * (int64_t)n_faces + f] : s * (int64_t)n_faces + f;
  }
};

// Key of simplex s (its row in this call) for FaceAcc::owner: the largest key wins (atomicMax on zeroed words) - a
// simplex the witness sweep has handled (weight < 0: it has evaluated all its rows already) before a lighter one (the
// dense neighbour is the one that skips) before a lower row.
__device__ __forceinline__ unsigned long long owner_key(int s, float w) {
  const uint32_t wb = __float_as_uint(w) < 0x7f800000u ? __float_as_uint(w) : 0x7f800000u;
  const uint32_t hi = w < 0.f ? 0xffffffffu : 0x7fffffffu - wb;
  return ((unsigned long long)hi << 32) | (unsigned long long)(~(uint32_t)s);
}

template <template <int> class F, typename... Args>
int dispatch_dim(int dim, Args&&... args) {
  switch (dim) {
    case 1: return F<1>::run(args...);
    case 2: return F<2>::run(args...);
    case 3: return F<3>::run(args...);
    case 4: return F<4>::run(args...);
    case 5: return F<5>::run(args...);
    case 6: return F<6>::run(args...);
    case 7: return F<7>::run(args...);
    case 8: return F<8>::run(args...);
    default: return fail(FLOODER_E_ARG, "dim must be in 1..8");
  }
}


// ---- what kind of cloud is this?  Four words behind the density grid (flooder_density_grid_words counts them): [2] =
// points in INTERIOR cells of a COARSE grid (16^3 / 64^2: four fine cells per axis pooled) - occupied cells whose axis
// neighbours inside the grid are all occupied -, [3] = all points.  A cloud that fills a volume (Gaussian, swiss
// cheese; 20 k to 16 M points) has 91 - 99 % of its points in interior cells, one that lies on a surface (the noisy
// torus) 7 - 21 %: there a second, doubled cell size per chunk of the cell sweep keeps thousands of points for samples
// the finish settles sooner (cfg 3 3.88 -> 3.75 ms with one try; cfg 2 1.18 -> 1.20) - the sweep reads the two words
// and decides (option "cell_surface_pct").  Results do not depend on it.  (The fine grid itself will not do: at a
// million points it holds a quarter of a leaf per cell, and a uniform cloud looks as hollow as a surface.)
// 16 workgroups of 256 threads, no communication between them: workgroup b owns the coarse slab z = b (3-D; in the
// plane: rows 4b .. 4b+3), a thread pools its own cell AND its two neighbours along z (y) - 48 (12) vector loads in
// flight together, one memory round trip -, the neighbours along the other axes come from the workgroup's LDS; two
// atomics per workgroup.  flooder_index_rows_f32 lets them ride in spare workgroups of the launch that builds the
// first inner tree level (a launch of their own after the index: +17 us; on a side stream: +40 us of cross-stream
// dependencies; coarse counts added atomically by the leaf pass: +46 us on the Gaussian, whose dense core hits a few
// hundred addresses: all measured); flooder_cloud_kind is the stand-alone form.
constexpr int KIND_WORDS = 4;
template <int DIM>
__device__ __forceinline__ void cloud_kind_block(const int32_t* __restrict__ fine, int32_t* __restrict__ kind, int block, int tid,
                                                 int* s_own, int* s_red) {
  constexpr int G = DIM == 2 ? 64 : 16;      // coarse cells per axis
  constexpr int GF = 4 * G;                  // fine cells per axis
  // coarse cell of this thread: (cx, cy [, cz]); the axis handled through the thread's own extra sums is the LAST one
  // in 3-D (z = block) and y in the plane (y = 4 * block + tid / 64)
  const int cx = DIM == 3 ? (tid & 15) : (tid & 63);
  const int cy = DIM == 3 ? (tid >> 4) : (4 * block + (tid >> 6));
  const int cz = DIM == 3 ? block : 0;
  const int own_axis = DIM == 3 ? cz : cy;
  int4 r[3][DIM == 3 ? 16 : 4];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const int a = own_axis + d - 1;          // the pooled cell along the own axis: below, own, above
    const bool ok = a >= 0 && a < G;
    if constexpr (DIM == 3) {
#pragma unroll
      for (int z = 0; z < 4; ++z)
#pragma unroll
        for (int y = 0; y < 4; ++y)
          r[d][4 * z + y] = ok ? *reinterpret_cast<const int4*>(fine + ((4 * a + z) * GF + (4 * cy + y)) * GF + 4 * cx)
                               : int4{0, 0, 0, 0};
    } else {
#pragma unroll
      for (int y = 0; y < 4; ++y)
        r[d][y] = ok ? *reinterpret_cast<const int4*>(fine + (4 * a + y) * GF + 4 * cx) : int4{0, 0, 0, 0};
    }
  }
  int sum[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    int t = 0;
#pragma unroll
    for (int q = 0; q < (DIM == 3 ? 16 : 4); ++q) t += r[d][q].x + r[d][q].y + r[d][q].z + r[d][q].w;
    sum[d] = t;
  }
  s_own[tid] = sum[1];
  __syncthreads();
  const int c = sum[1];
  bool in = c > 0;
  in = in && (own_axis == 0 || sum[0] > 0) && (own_axis == G - 1 || sum[2] > 0);
  in = in && (cx == 0 || s_own[tid - 1] > 0) && (cx == G - 1 || s_own[tid + 1] > 0);
  if constexpr (DIM == 3) in = in && (cy == 0 || s_own[tid - 16] > 0) && (cy == 15 || s_own[tid + 16] > 0);
  int inner = in ? c : 0, all = c;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    inner += __shfl_xor(inner, o);
    all += __shfl_xor(all, o);
  }
  if ((tid & 63) == 0) { s_red[tid >> 6] = inner; s_red[4 + (tid >> 6)] = all; }
  __syncthreads();
  if (tid == 0) {
    const int a = s_red[0] + s_red[1] + s_red[2] + s_red[3], b = s_red[4] + s_red[5] + s_red[6] + s_red[7];
    if (b != 0) {
      atomicAdd(&kind[2], a);
      atomicAdd(&kind[3], b);
    }
  }
}
template <int DIM>
__global__ __launch_bounds__(256) void cloud_kind_kernel(const int32_t* __restrict__ fine, int32_t* __restrict__ kind) {
  __shared__ int s_own[256];
  __shared__ int s_red[8];
  cloud_kind_block<DIM>(fine, kind, blockIdx.x, threadIdx.x, s_own, s_red);
}
inline void launch_cloud_kind(int dim, int32_t* grid, hipStream_t st) {   // grid: the fine grid; the words sit behind it
  if (dim == 2) hipLaunchKernelGGL((cloud_kind_kernel<2>), dim3(16), dim3(256), 0, st, grid, grid + 256 * 256);
  else if (dim == 3) hipLaunchKernelGGL((cloud_kind_kernel<3>), dim3(16), dim3(256), 0, st, grid, grid + 64 * 64 * 64);
}

// The size / abi rule of a parameter block (include/flooder_hip.h): the caller's struct (its `size` bytes) laid over a
// zeroed struct of OUR size - fields the caller does not have read as NULL / 0, a caller that has fields we do not know
// is refused with `who`.
template <typename T>
int take(const T* p, T& out, const char* who) {
  if (!p) return fail(FLOODER_E_ARG, who);
  if (p->abi != FLOODER_PARAMS_ABI || p->size < 2 * sizeof(uint32_t) || p->size > sizeof(T)) return fail(FLOODER_E_ARG, who);
  memset(&out, 0, sizeof(T));
  memcpy(&out, p, p->size);
  return 0;
}

// ---- the k-nearest family (flood_knn.hip, flood_knn_merge.hip, flooder_witness_knn in flood_grad.hip), host side.
// A lane keeps its k best in K registers, K = k rounded up to 2, 4, 8, 16 or 32, one kernel instantiation each:
// f(std::integral_constant<int, K>{}) for the K that holds k.
template <class F>
void with_knn_slots(int k, F&& f) {
  if (k <= 2) f(std::integral_constant<int, 2>{});
  else if (k <= 4) f(std::integral_constant<int, 4>{});
  else if (k <= 8) f(std::integral_constant<int, 8>{});
  else if (k <= 16) f(std::integral_constant<int, 16>{});
  else f(std::integral_constant<int, 32>{});
}

// The range checks the entries share, in each entry's order: k (1..`k_max`: FLOODER_KNN_MAX, FLOODER_KNN_WIDE_MAX for
// the wide entry), dim, stat, then fewer points than k (`needs_k_points`: the witness and wide entries - the sweeps say
// so with their pointer check, behind "nothing to do") and more points than 32-bit ids hold (`ids`).  `who` opens each.
inline int knn_check_ranges(const char* who, int k, int k_max, int dim, int stat, int64_t n_pts, bool needs_k_points,
                            bool ids) {
  if (k < 1 || k > k_max) return failf(FLOODER_E_ARG, "%s: k must be in 1..%d", who, k_max);
  if (dim < 2 || dim > FLOODER_MAX_DIM) return failf(FLOODER_E_ARG, "%s: dim must be in 2..8", who);
  if (stat != 0 && stat != 1) return failf(FLOODER_E_ARG, "%s: stat must be 0 (kth) or 1 (dtm)", who);
  if (needs_k_points && n_pts < k) return failf(FLOODER_E_ARG, "%s: fewer points than k", who);
  if (ids && n_pts > 0x7fffffffLL) return failf(FLOODER_E_ARG, "%s: more than 2^31 - 1 points", who);
  return 0;
}

// The launches that have a parameter block (include/flooder_hip.h), each ONE function on its block: it makes the checks
// and fills the kernel's own structs from the named fields.  flood_params.hip calls them with the caller's block, the
// positional exports with a zeroed block they have filled by name (so: no density grid, no run table and planes_ready 0
// from the positional witness entry, planes_ready 0 from the positional cell entry).
int fused_witness(const flooder_fused_sweep_t& a, void* stream);   // flood_wit.hip
int fused_cell(const flooder_fused_sweep_t& a, void* stream);      // flood_cell.hip
int fused_finish(const flooder_fused_sweep_t& a, void* stream);    // flood_finish.hip
enum class SortedMode { minima, shard, faces };                    // out_d2 of all tiles / of one rank's tiles / face maxima
int sorted_sweep(const flooder_sorted_sweep_t& a, SortedMode mode, void* stream);   // flood_sorted.hip
int fps_batched(const flooder_fps_batched_t& a, void* stream);     // flood_fps2.hip

}  // namespace flooder
