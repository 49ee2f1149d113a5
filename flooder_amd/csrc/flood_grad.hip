// flood_grad.hip - exact witnesses of the filtration values and the deterministic scatter of their gradients (gfx950).
//
// A filtration value is f = sqrt(d2*) with d2* = max over the samples p of a face of min_x |p - x|^2.  Its gradient
// needs the two arguments the sweeps never keep: the sample p* that attains the maximum and the point x* = points[j*]
// that attains its minimum.  Both are recovered here from the per-sample minima of the unfused sweep, exactly:
//
//   face_argmax      one pass over the (S, R) d2 bits of a dimension pass: per (simplex, face) the 64-bit key
//                    (d2 bits << 32 | ~row), the largest d2 with the smallest sample row among equal ones (the row of
//                    the caller's weight table, not the swept column: row_id maps one to the other).
//   witness_search   per distinct face: p* rebuilt from (vertices, swept weight row) with the sweeps' own fma order,
//                    then a fixed-radius walk of the box tree of the cloud (flood_bvh.hpp): only leaves whose lower
//                    bound is <= the known d2 are opened, and the smallest original id whose d2, in the sweeps'
//                    arithmetic, has exactly the target bits is the witness.  A face with no such point is counted.
//   witness_knn      the robust filtration's witness: the k smallest (d2 word, original id) keys of p* over the whole
//                    cloud, in order, and a check that they reproduce the swept statistic bit for bit.
//   segment_sum      backward: contributions sorted (stably) by their target row are summed segment by segment in
//                    that order - no float atomics, the gradient is bit-identical run to run.

#include "../../include/flooder_hip.h"
#include "flood_common.hpp"
#include "flood_bvh.hpp"

using namespace flooder;

namespace {

// ------------------------------------------------------------------------------------------------ face argmax
// One wave per simplex (persistent, grid-stride).  The rows of a face are read in ascending column order (the caller
// sorts each face's CSR segment), so a face that spans the whole row reads it coalesced.  Lanes keep a running 64-bit
// key, the wave folds it once per face: no atomics.
__global__ __launch_bounds__(256) void face_argmax_kernel(const uint32_t* __restrict__ d2, int64_t n_simplices, int R,
                                                          const int32_t* __restrict__ face_ptr,
                                                          const int32_t* __restrict__ face_rows,
                                                          const int32_t* __restrict__ row_id, int n_faces,
                                                          unsigned long long* __restrict__ out_key) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int64_t n_waves = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t s = wave; s < n_simplices; s += n_waves) {
    const uint32_t* row = d2 + s * (int64_t)R;
    for (int f = 0; f < n_faces; ++f) {
      const int lo = face_ptr[f], hi = face_ptr[f + 1];
      uint32_t kb = 0u, kr = 0u;   // (d2 bits, 0xffffffff - sample row) of this lane's best; (0, 0) = nothing seen
      for (int i = lo + lane; i < hi; i += 64) {
        const int c = face_rows[i];
        const uint32_t b = row[c];
        const uint32_t r = 0xffffffffu - (uint32_t)(row_id ? row_id[c] : c);
        if (b > kb || (b == kb && r > kr)) { kb = b; kr = r; }
      }
      const uint32_t mb = wave_max_u32(kb);
      const uint32_t mr = wave_max_u32(kb == mb ? kr : 0u);
      if (lane == 0) out_key[s * (int64_t)n_faces + f] = ((unsigned long long)mb << 32) | mr;
    }
  }
}

// ------------------------------------------------------------------------------------------------ witness search
// One wave per query.  The stack holds groups of 64 sibling nodes (level, group); a popped group is tested one node per
// lane, the qualifying inner nodes push their child groups, the qualifying leaves are evaluated four at a time (16
// points each, one point per lane).  DFS keeps at most 64 entries per level on the stack (STACK: flood_bvh.hpp).

template <int DIM>
__global__ __launch_bounds__(256) void witness_search_kernel(const float* __restrict__ pts, int64_t n_pts,
                                                             const float* __restrict__ nodes, Levels lv,
                                                             const int32_t* __restrict__ order,
                                                             const float* __restrict__ verts,
                                                             const float* __restrict__ weights, int k1, int R,
                                                             int64_t n_simplices, int64_t n_queries,
                                                             const int32_t* __restrict__ q_simplex,
                                                             const int32_t* __restrict__ q_row,
                                                             const uint32_t* __restrict__ q_d2,
                                                             int64_t* __restrict__ out_point,
                                                             int32_t* __restrict__ not_found) {
  constexpr int DP = padded_dim(DIM);
  __shared__ int32_t s_stack[WAVES_PER_BLOCK][STACK];
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  const int64_t wave = (int64_t)blockIdx.x * WAVES_PER_BLOCK + wv;
  const int64_t n_waves = (int64_t)gridDim.x * WAVES_PER_BLOCK;
  const unsigned long long below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  const int top = lv.n_levels - 1;
  for (int64_t q = wave; q < n_queries; q += n_waves) {
    const int64_t s = q_simplex[q];
    const int64_t r = q_row[q];
    const uint32_t target = q_d2[q];
    const float tf = __uint_as_float(target);
    if (s < 0 || s >= n_simplices || r < 0 || r >= R) {   // (not a swept sample: no witness)
      if (lane == 0) {
        out_point[q] = -1;
        atomicAdd(not_found, 1);
      }
      continue;
    }
    // p* exactly as the sweeps build a sample: p = 0; p[k] = fma(w_j, v_j[k], p[k]) in vertex order
    float p[DIM];
#pragma unroll
    for (int k = 0; k < DIM; ++k) p[k] = 0.f;
    const float* vs = verts + s * (int64_t)k1 * DIM;
    for (int j = 0; j < k1; ++j) {
      const float w = weights[r * k1 + j];
#pragma unroll
      for (int k = 0; k < DIM; ++k) p[k] = __builtin_fmaf(w, vs[j * DIM + k], p[k]);
    }
    uint32_t best = 0xffffffffu;
    int sp = 1;
    if (lane == 0) s_stack[wv][0] = top;   // (level top, group 0): the <= 64 top nodes
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    while (sp > 0) {
      --sp;
      const int e = s_stack[wv][sp];
      const int lvl = e & 7;
      const int64_t grp = e >> 3;
      const int64_t idx = grp * FAN + lane;
      bool ok = false;
      if (idx < lv.count[lvl]) {   // (child_point_bound of flood_bvh.hpp, its load written out: see witness_knn_kernel)
        float lo[DP], hi[DP];
        const float* nb = nodes + (lv.off[lvl] + idx) * 2 * DP;
        load_row<DP>(nb, lo);
        load_row<DP>(nb + DP, hi);
        ok = box_gap2<DIM>(p, lo, hi) * SAFE <= tf;
      }
      unsigned long long mask = __ballot(ok);
      __builtin_amdgcn_wave_barrier();   // (every lane has read the popped entry before a push may overwrite it)
      if (lvl == 0) {
        while (mask) {
          // (the pop above and the next four leaves, one point per lane: the same steps in witness_knn_kernel; keep in step)
          int64_t leaf[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            if (mask) {
              const int j = __builtin_ctzll(mask);
              mask &= mask - 1;
              leaf[u] = grp * FAN + j;
            } else {
              leaf[u] = -1;
            }
          }
          const int u = lane >> 4;
          const int64_t lf = u == 0 ? leaf[0] : (u == 1 ? leaf[1] : (u == 2 ? leaf[2] : leaf[3]));
          const int64_t rw = lf * LEAF + (lane & 15);
          if (lf >= 0 && rw < n_pts) {
            float x[DP];
            load_row<DP>(pts + rw * DP, x);
            const float d2 = dist2<DIM>(p, x);
            if (__float_as_uint(d2) == target) {
              const uint32_t id = (uint32_t)order[rw];
              best = id < best ? id : best;
            }
          }
        }
      } else {
        if (ok) s_stack[wv][sp + __popcll(mask & below)] = (int)((idx << 3) | (lvl - 1));
        sp += __popcll(mask);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
      }
    }
    best = wave_min_u32(best);
    if (lane == 0) {
      out_point[q] = best == 0xffffffffu ? -1 : (int64_t)best;
      if (best == 0xffffffffu) atomicAdd(not_found, 1);
    }
  }
}

template <int DIM>
struct WitnessOp {
  static int run(const flooder_witness_search_t& a, const Levels& lv, hipStream_t st) {
    hipLaunchKernelGGL(witness_search_kernel<DIM>, stack_walk_grid(a.n_queries), dim3(64 * WAVES_PER_BLOCK), 0, st,
                       a.pts_sorted, a.n_pts, a.nodes, lv, a.order, a.verts, a.weights, a.k1, a.R, a.n_simplices,
                       a.n_queries, a.q_simplex, a.q_row, a.q_d2, a.out_point, a.not_found);
    return check_launch("witness_search");
  }
};

// ------------------------------------------------------------------------------------------------ witness k nearest
// The witness of a robust value (flood_complex(neighbors=k)): WHICH k points realise the statistic of the sample p*.
// One wave per query, the stack of witness_search_kernel.  The wave keeps the k smallest keys (d2 word, original id)
// seen so far sorted ascending, one key per lane (k <= 32 < 64; the other lanes hold the all-ones key).  A popped
// group's children are tested one per lane; the nearest qualifying child is pushed LAST, so the first thing a query
// does is walk down to the leaf group nearest to it and the k-th best is small from then on.  Leaves are evaluated
// four at a time, one point per lane, and the leaves still waiting are tested again after every four.
//
// Exactness.  Keys are distinct (ids are), so "the k smallest keys of all points" is one set, and inserting any
// superset of it in any order leaves exactly that set, sorted.  A subtree or leaf is skipped only when
// lb * SAFE > (k-th best d2) - every point in it then has d2 > the k-th best and hence a LARGER key, whatever its
// id.  A box at lb == k-th best is opened: a point at an equal d2 with a smaller id displaces the k-th entry.
// Nothing is skipped before the list holds k points (its k-th d2 word is all ones: +inf here).
template <int DIM>
__global__ __launch_bounds__(256) void witness_knn_kernel(const float* __restrict__ pts, int64_t n_pts,
                                                          const float* __restrict__ nodes, Levels lv,
                                                          const int32_t* __restrict__ order,
                                                          const float* __restrict__ verts,
                                                          const float* __restrict__ weights, int k1, int R,
                                                          int64_t n_simplices, int64_t n_queries, int k, int stat,
                                                          const int32_t* __restrict__ q_simplex,
                                                          const int32_t* __restrict__ q_row,
                                                          const uint32_t* __restrict__ q_stat,
                                                          int64_t* __restrict__ out_ids, uint32_t* __restrict__ out_d2,
                                                          int32_t* __restrict__ not_found) {
  constexpr int DP = padded_dim(DIM);
  __shared__ int32_t s_stack[WAVES_PER_BLOCK][STACK];
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  const int64_t wave = (int64_t)blockIdx.x * WAVES_PER_BLOCK + wv;
  const int64_t n_waves = (int64_t)gridDim.x * WAVES_PER_BLOCK;
  const unsigned long long below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  const int top = lv.n_levels - 1;
  for (int64_t q = wave; q < n_queries; q += n_waves) {
    const int64_t s = q_simplex[q];
    const int64_t r = q_row[q];
    bool found = !(s < 0 || s >= n_simplices || r < 0 || r >= R);   // (else: not a swept sample, no witness)
    uint32_t l_hi = 0xffffffffu, l_lo = 0xffffffffu;   // this lane's entry of the list: (d2 word, original id)
    if (found) {
      // p* exactly as the sweeps build a sample: p = 0; p[c] = fma(w_j, v_j[c], p[c]) in vertex order
      float p[DIM];
#pragma unroll
      for (int c = 0; c < DIM; ++c) p[c] = 0.f;
      const float* vs = verts + s * (int64_t)k1 * DIM;
      for (int j = 0; j < k1; ++j) {
        const float w = weights[r * k1 + j];
#pragma unroll
        for (int c = 0; c < DIM; ++c) p[c] = __builtin_fmaf(w, vs[j * DIM + c], p[c]);
      }
      uint32_t kth_hi = 0xffffffffu, kth_lo = 0xffffffffu;   // the list's k-th key (wave-uniform)
      float kth_f = __builtin_inff();
      int sp = 1;
      if (lane == 0) s_stack[wv][0] = top;   // (level top, group 0): the <= 64 top nodes
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_wave_barrier();
      while (sp > 0) {
        --sp;
        const int e = s_stack[wv][sp];
        const int lvl = e & 7;
        const int64_t grp = e >> 3;
        const int64_t idx = grp * FAN + lane;
        bool ok = false;
        float lb = __builtin_inff();
        if (idx < lv.count[lvl]) {   // (child_point_bound of flood_bvh.hpp, its load written out: the call cost k = 32 3 %)
          float lo[DP], hi[DP];
          const float* nb = nodes + (lv.off[lvl] + idx) * 2 * DP;
          load_row<DP>(nb, lo);
          load_row<DP>(nb + DP, hi);
          lb = box_gap2<DIM>(p, lo, hi);
          ok = !(lb * SAFE > kth_f);
        }
        unsigned long long mask = __ballot(ok);
        __builtin_amdgcn_wave_barrier();   // (every lane has read the popped entry before a push may overwrite it)
        if (lvl == 0) {
          while (mask) {
            // (the pop above and the next four leaves, one point per lane: the steps of witness_search_kernel)
            int64_t leaf[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              if (mask) {
                const int j = __builtin_ctzll(mask);
                mask &= mask - 1;
                leaf[u] = grp * FAN + j;
              } else {
                leaf[u] = -1;
              }
            }
            const int u = lane >> 4;
            const int64_t lf = u == 0 ? leaf[0] : (u == 1 ? leaf[1] : (u == 2 ? leaf[2] : leaf[3]));
            const int64_t rw = lf * LEAF + (lane & 15);
            uint32_t c_hi = 0xffffffffu, c_lo = 0xffffffffu;   // this lane's candidate key
            if (lf >= 0 && rw < n_pts) {   // (rows of the padded last leaf are never candidates)
              float x[DP];
              load_row<DP>(pts + rw * DP, x);
              const float d2 = dist2<DIM>(p, x);
              c_hi = __float_as_uint(d2);
              c_lo = (uint32_t)order[rw];
            }
            // insert every candidate below the k-th key, first lane first
            for (;;) {
              const unsigned long long better = __ballot(c_hi < kth_hi || (c_hi == kth_hi && c_lo < kth_lo));
              if (!better) break;
              const int j = __builtin_ctzll(better);
              const uint32_t b_hi = (uint32_t)__builtin_amdgcn_readlane((int)c_hi, j);
              const uint32_t b_lo = (uint32_t)__builtin_amdgcn_readlane((int)c_lo, j);
              if (lane == j) c_hi = c_lo = 0xffffffffu;
              const int pos = __popcll(__ballot(l_hi < b_hi || (l_hi == b_hi && l_lo < b_lo)));
              const uint32_t u_hi = (uint32_t)__shfl_up((int)l_hi, 1);
              const uint32_t u_lo = (uint32_t)__shfl_up((int)l_lo, 1);
              if (lane > pos) { l_hi = u_hi; l_lo = u_lo; }
              if (lane == pos) { l_hi = b_hi; l_lo = b_lo; }
              if (lane >= k) l_hi = l_lo = 0xffffffffu;   // (what fell off the end)
              kth_hi = (uint32_t)__builtin_amdgcn_readlane((int)l_hi, k - 1);
              kth_lo = (uint32_t)__builtin_amdgcn_readlane((int)l_lo, k - 1);
            }
            kth_f = kth_hi == 0xffffffffu ? __builtin_inff() : __uint_as_float(kth_hi);
            mask &= __ballot(!(lb * SAFE > kth_f));   // the leaves still waiting, against the new k-th best
          }
        } else {
          if (mask) {
            // the nearest qualifying child goes on top of the stack, the others below it in lane order
            const float mn = wave_min_f32(ok ? lb : __builtin_inff());
            const int jn = __builtin_ctzll(__ballot(ok && lb == mn));
            const unsigned long long rest = mask & ~(1ull << jn);
            if (ok) {
              const int at = lane == jn ? __popcll(rest) : __popcll(rest & below);
              s_stack[wv][sp + at] = (int)((idx << 3) | (lvl - 1));
            }
            sp += __popcll(mask);
          }
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
          __builtin_amdgcn_wave_barrier();
        }
      }
      // the statistic of the k words, as sweep_knn_kernel computes it
      float v = __uint_as_float(kth_hi);
      if (stat != 0) {
        float acc = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)l_hi, 0));
        for (int i = 1; i < k; ++i) acc = acc + __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)l_hi, i));
        v = acc / (float)k;
      }
      found = kth_hi != 0xffffffffu && __float_as_uint(v) == q_stat[q];
    }
    if (lane < k) {
      out_ids[q * k + lane] = found ? (int64_t)l_lo : -1;
      if (out_d2) out_d2[q * k + lane] = found ? l_hi : 0xffffffffu;
    }
    if (!found && lane == 0) atomicAdd(not_found, 1);
  }
}

template <int DIM>
struct WitnessKnnOp {
  static int run(const flooder_witness_knn_t& a, const Levels& lv, hipStream_t st) {
    if constexpr (DIM < 2) {
      return fail(FLOODER_E_ARG, "flooder_witness_knn: dim must be in 2..8");
    } else {
      hipLaunchKernelGGL(witness_knn_kernel<DIM>, stack_walk_grid(a.n_queries), dim3(64 * WAVES_PER_BLOCK), 0, st,
                         a.pts_sorted, a.n_pts, a.nodes, lv, a.order, a.verts, a.weights, a.k1, a.R, a.n_simplices,
                         a.n_queries, a.k, a.stat, a.q_simplex, a.q_row, a.q_stat, a.out_ids, a.out_d2, a.not_found);
      return check_launch("witness_knn");
    }
  }
};

// ------------------------------------------------------------------------------------------------ segment sum
// Thread (segment, axis): out[target[g], k] = sum of vals[order[i], k] over i in [seg_ptr[g], seg_ptr[g+1]), in order.
__global__ __launch_bounds__(256) void segment_sum_kernel(const float* __restrict__ vals, int dim,
                                                          const int64_t* __restrict__ order,
                                                          const int64_t* __restrict__ seg_ptr,
                                                          const int64_t* __restrict__ seg_target, int64_t n_seg,
                                                          float* __restrict__ out) {
  const int64_t n = n_seg * dim;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t g = t / dim;
    const int k = (int)(t - g * dim);
    float acc = 0.f;
    for (int64_t i = seg_ptr[g]; i < seg_ptr[g + 1]; ++i) acc += vals[order[i] * dim + k];
    out[seg_target[g] * dim + k] = acc;
  }
}

}  // namespace

extern "C" {

int flooder_face_argmax_f32(const uint32_t* d2, int64_t n_simplices, int R, const int32_t* face_ptr,
                            const int32_t* face_rows, const int32_t* row_id, int n_faces, uint64_t* out_key,
                            void* stream) {
  if (n_simplices == 0) return FLOODER_OK;
  if (!d2 || !face_ptr || !face_rows || !out_key || n_faces < 1 || R < 1 || n_simplices < 0)
    return fail(FLOODER_E_ARG, "flooder_face_argmax_f32: bad argument");
  int64_t blocks = (n_simplices + 3) / 4;
  if (blocks > 256 * 8) blocks = 256 * 8;
  hipLaunchKernelGGL(face_argmax_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, d2, n_simplices, R,
                     face_ptr, face_rows, row_id, n_faces, reinterpret_cast<unsigned long long*>(out_key));
  return check_launch("face_argmax");
}

int flooder_witness_search(const flooder_witness_search_t* p, void* stream) {
  flooder_witness_search_t a;
  if (int rc = take(p, a, "flooder_witness_search: bad parameter block (abi / size)")) return rc;
  if (a.n_queries == 0) return FLOODER_OK;
  if (!a.pts_sorted || !a.nodes || !a.order || !a.verts || !a.weights || !a.q_simplex || !a.q_row || !a.q_d2 ||
      !a.out_point || !a.not_found || a.n_pts < 1 || a.k1 < 1 || a.R < 1 || a.n_queries < 0 || a.dim < 2 || a.dim > 8 ||
      a.n_pts > 0x7fffffffLL)
    return fail(FLOODER_E_ARG, "flooder_witness_search: bad argument");
  Levels lv;
  if (int rc = stack_walk_levels("flooder_witness_search", a.n_pts, lv)) return rc;
  return dispatch_dim<WitnessOp>(a.dim, a, lv, (hipStream_t)stream);
}

int flooder_witness_knn(const flooder_witness_knn_t* p, void* stream) {
  flooder_witness_knn_t a;
  if (int rc = take(p, a, "flooder_witness_knn: bad parameter block (abi / size)")) return rc;
  if (int rc = knn_check_ranges("flooder_witness_knn", a.k, FLOODER_KNN_MAX, a.dim, a.stat, a.n_pts, true, true)) return rc;
  if (a.n_queries == 0) return FLOODER_OK;
  if (!a.pts_sorted || !a.nodes || !a.order || !a.verts || !a.weights || !a.q_simplex || !a.q_row || !a.q_stat ||
      !a.out_ids || !a.not_found || a.k1 < 1 || a.R < 1 || a.n_queries < 0)
    return fail(FLOODER_E_ARG, "flooder_witness_knn: bad argument (null pointer, k1, R, n_queries)");
  Levels lv;
  if (int rc = stack_walk_levels("flooder_witness_knn", a.n_pts, lv)) return rc;
  return dispatch_dim<WitnessKnnOp>(a.dim, a, lv, (hipStream_t)stream);
}

int flooder_segment_sum_f32(const float* vals, int dim, const int64_t* order, const int64_t* seg_ptr,
                            const int64_t* seg_target, int64_t n_seg, float* out, void* stream) {
  if (n_seg == 0) return FLOODER_OK;
  if (!vals || !order || !seg_ptr || !seg_target || !out || dim < 1 || n_seg < 0)
    return fail(FLOODER_E_ARG, "flooder_segment_sum_f32: bad argument");
  int64_t blocks = (n_seg * dim + 255) / 256;
  if (blocks > 256 * 16) blocks = 256 * 16;
  hipLaunchKernelGGL(segment_sum_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, vals, dim, order,
                     seg_ptr, seg_target, n_seg, out);
  return check_launch("segment_sum");
}

}  // extern "C"
