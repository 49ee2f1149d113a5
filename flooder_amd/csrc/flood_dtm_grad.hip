// flood_dtm_grad.hip - the closed-form backward of the distance to a measure for every k of the wide sweep (gfx950).
//
// distance_to_measure(points, queries, ...) has, per query q with neighbours x_(1) .. x_(m) (m = k for "dtm", m = 1 -
// x_(k) alone - for "kth") and a coefficient c_q the caller forms from the value and the incoming gradient,
//
//     d/dq      =  c_q * sum_i (q - x_(i))                      grad_queries: one wave per query, a gather and a sum
//     d/dx_j    = -sum over the entries (q, i) with id = j of c_q * (q - x_j)          grad_points: the transpose
//
// Neither kernel keeps a contribution in memory: both read the caller's own (., dim) rows in input order, the int32 ids
// of flooder_knn_wide_f32 and one coefficient per query - no tree, no (Q, k, dim) tensor.  No atomics; every output
// word is written once per launch by a plain store, in a summation order that is a function of the arguments alone:
//
//   grad_queries   lane l of the wave adds the differences of the list positions l, l + 64, l + 128, ... < m to its
//                  own partial sum (which starts as +0), left to right; the 64 partial sums (+0 in the lanes >= m) are
//                  then added in a butterfly: with lane l holding a_l, a_l = a_l + a_(l ^ 32), then ^ 16, 8, 4, 2, 1 -
//                  float addition commutes, so every lane ends with the same word; the product with c_q comes last.
//   grad_points    thread (segment, axis) walks its segment of the sorted entry list front to back and continues the
//                  value already in out_p: acc = fma(-c_q, q[axis] - x_j[axis], acc), one rounding per difference and
//                  one per step.  The entries of a segment ascend by query row, so launches over consecutive groups of
//                  query rows give, word for word, what one launch over all of them gives: the rule of
//                  flooder_segment_sum_f32, continued across launches.

#include "../../include/flooder_hip.h"
#include "flood_common.hpp"

using namespace flooder;

namespace {

constexpr int GRAD_WAVES = 4;   // waves of a workgroup of grad_queries: ~20 VGPRs, no LDS - occupancy is the wave limit

// ------------------------------------------------------------------------------------------------ grad_queries
// One wave per query (grid-stride).  The ids of a row are read coalesced, 64 at a time; each lane then gathers its
// own neighbour's row: 64 independent dependent-load chains per wave, eight waves per SIMD hide the rest.
template <int DIM>
__global__ __launch_bounds__(64 * GRAD_WAVES) void dtm_grad_queries_kernel(const float* __restrict__ points,
                                                                          int64_t n_points,
                                                                          const float* __restrict__ queries,
                                                                          int64_t n_queries,
                                                                          const int32_t* __restrict__ ids,
                                                                          int64_t ld_ids, int m,
                                                                          const float* __restrict__ coef,
                                                                          float* __restrict__ out_q) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * GRAD_WAVES + (threadIdx.x >> 6);
  const int64_t n_waves = (int64_t)gridDim.x * GRAD_WAVES;
  for (int64_t q = wave; q < n_queries; q += n_waves) {
    float x0[DIM], acc[DIM];
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      x0[c] = queries[q * DIM + c];
      acc[c] = 0.f;
    }
    const int32_t* row = ids + q * ld_ids;
    for (int i = lane; i < m; i += 64) {
      const int64_t j = row[i];
      if (j < 0 || j >= n_points) continue;   // (no row of points: never read, adds nothing)
      const float* x = points + j * DIM;
#pragma unroll
      for (int c = 0; c < DIM; ++c) acc[c] = acc[c] + (x0[c] - x[c]);
    }
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
#pragma unroll
      for (int s = 32; s >= 1; s >>= 1) acc[c] = acc[c] + __shfl_xor(acc[c], s);
    }
    if (lane == 0) {
      const float cf = coef[q];
#pragma unroll
      for (int c = 0; c < DIM; ++c) out_q[q * DIM + c] = cf * acc[c];
    }
  }
}

template <int DIM>
struct GradQueriesOp {
  static int run(const float* points, int64_t n_points, const float* queries, int64_t n_queries, const int32_t* ids,
                 int64_t ld_ids, int m, const float* coef, float* out_q, hipStream_t st) {
    if constexpr (DIM < 2) {
      return fail(FLOODER_E_ARG, "flooder_dtm_grad_queries_f32: dim must be in 2..8");
    } else {
      int64_t blocks = (n_queries + GRAD_WAVES - 1) / GRAD_WAVES;
      if (blocks > 256 * 16) blocks = 256 * 16;
      hipLaunchKernelGGL(dtm_grad_queries_kernel<DIM>, dim3((unsigned)blocks), dim3(64 * GRAD_WAVES), 0, st, points,
                         n_points, queries, n_queries, ids, ld_ids, m, coef, out_q);
      return check_launch("dtm_grad_queries");
    }
  }
};

// ------------------------------------------------------------------------------------------------ grad_points
// Thread (segment, axis), consecutive threads on the axes of one target: the DIM threads of a segment read the same
// entry and coefficient (one broadcast load) and neighbouring words of the query row.  The chain of a segment is
// sequential by contract; four entries' loads are issued together and their steps taken in order.
__global__ __launch_bounds__(256) void dtm_grad_points_kernel(const float* __restrict__ points, int64_t n_points,
                                                              const float* __restrict__ queries, int64_t n_queries,
                                                              int dim, const float* __restrict__ coef,
                                                              const int64_t* __restrict__ entries,
                                                              const int64_t* __restrict__ seg_ptr,
                                                              const int32_t* __restrict__ seg_target, int64_t n_seg,
                                                              float* __restrict__ out_p) {
  const int64_t n = n_seg * dim;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t g = t / dim;
    const int c = (int)(t - g * dim);
    const int64_t j = seg_target ? (int64_t)seg_target[g] : g;
    int64_t i = seg_ptr[g];
    const int64_t end = seg_ptr[g + 1];
    if (j < 0 || j >= n_points || i >= end) continue;   // (no row of points, or an empty segment: nothing is touched)
    const float x = points[j * dim + c];
    float acc = out_p[j * dim + c];
    for (; i + 4 <= end; i += 4) {
      int64_t q[4];
      float cf[4], v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) q[u] = (int64_t)(uint32_t)entries[i + u];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const bool ok = q[u] < n_queries;   // (no query row: never read, adds nothing)
        cf[u] = ok ? coef[q[u]] : 0.f;
        v[u] = ok ? queries[q[u] * dim + c] : x;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) acc = __builtin_fmaf(-cf[u], v[u] - x, acc);
    }
    for (; i < end; ++i) {
      const int64_t q = (int64_t)(uint32_t)entries[i];
      if (q < n_queries) acc = __builtin_fmaf(-coef[q], queries[q * dim + c] - x, acc);
    }
    out_p[j * dim + c] = acc;
  }
}

}  // namespace

extern "C" {

int flooder_dtm_grad_queries_f32(const float* points, int64_t n_points, const float* queries, int64_t n_queries, int dim,
                                 const int32_t* ids, int64_t ld_ids, int m, const float* coef, float* out_q,
                                 void* stream) {
  if (dim < 2 || dim > 8) return fail(FLOODER_E_ARG, "flooder_dtm_grad_queries_f32: dim must be in 2..8");
  if (m < 1 || m > FLOODER_KNN_WIDE_MAX)
    return fail(FLOODER_E_ARG, "flooder_dtm_grad_queries_f32: m must be in 1..FLOODER_KNN_WIDE_MAX");
  if (n_points < 0 || n_queries < 0 || ld_ids < m)
    return fail(FLOODER_E_ARG, "flooder_dtm_grad_queries_f32: bad argument (negative count, ld_ids < m)");
  if (!points || !queries || !ids || !coef || !out_q)
    return fail(FLOODER_E_ARG, "flooder_dtm_grad_queries_f32: bad argument (null pointer)");
  if (n_queries == 0) return FLOODER_OK;
  return dispatch_dim<GradQueriesOp>(dim, points, n_points, queries, n_queries, ids, ld_ids, m, coef, out_q,
                                     (hipStream_t)stream);
}

int flooder_dtm_grad_points_f32(const float* points, int64_t n_points, const float* queries, int64_t n_queries, int dim,
                                const float* coef, const int64_t* entries, const int64_t* seg_ptr,
                                const int32_t* seg_target, int64_t n_seg, float* out_p, void* stream) {
  if (dim < 2 || dim > 8) return fail(FLOODER_E_ARG, "flooder_dtm_grad_points_f32: dim must be in 2..8");
  if (n_points < 0 || n_queries < 0 || n_seg < 0)
    return fail(FLOODER_E_ARG, "flooder_dtm_grad_points_f32: bad argument (negative count)");
  if (!points || !queries || !coef || !entries || !seg_ptr || !out_p)
    return fail(FLOODER_E_ARG, "flooder_dtm_grad_points_f32: bad argument (null pointer)");
  if (n_queries == 0 || n_seg == 0) return FLOODER_OK;
  int64_t blocks = (n_seg * dim + 255) / 256;
  if (blocks > 256 * 16) blocks = 256 * 16;
  hipLaunchKernelGGL(dtm_grad_points_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, points,
                     n_points, queries, n_queries, dim, coef, entries, seg_ptr, seg_target, n_seg, out_p);
  return check_launch("dtm_grad_points");
}

}  // extern "C"
