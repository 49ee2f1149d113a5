// flood_mass_grad.hip - the closed-form backward of the distance to a WEIGHTED measure (gfx950): the weighted siblings of
// flood_dtm_grad.hip, with its contracts.
//
// distance_to_weighted_measure(sites, masses, queries, ...) lists, per reached query q, the sites y_(0) .. y_(j*) up to
// the crossing position j* = count - 1 (flooder_knn_mass_f32).  With tau the target mass, M the cumulative mass before
// the crossing and rho = tau - M, the entry coefficients are a_t = mu_(t) for t < j* and a_(j*) = rho, and with a
// coefficient c_q the caller forms from the value and the incoming gradient ("dtm": grad_out / (f tau), 0 where f = 0;
// grad_out * 2 / tau for the squared value)
//
//     d/dq      =  c_q * sum_t a_t (q - y_(t))                  mass_grad_queries: one wave per query, a gather and a sum
//     d/dy_j    = -c_q * a_t (q - y_j) at the entry with id j   mass_grad_points: the transpose, over sorted entries
//     d/dmu_l   =  h_q * (d2(q, y_l) - d2(q, y_(j*)))           mass_grad_masses: the same transpose for the sites listed
//                                                               BEFORE the crossing, h_q = c_q / 2
//
// (the term every mass gets because tau depends on it is one number: the caller's reduction).  Two layouts keep every
// entry at a dozen arguments and every per-entry read of the transposes at one 16-byte load:
//
//   sites  (n, dim + 1) float32: the row of a site is its dim coordinates, then its mass;
//   qrow   (Q, 4) 32-bit words, the crossing row of a query: c_q (float32; the caller's), rho (float32), the crossing
//          id (int32, -1 without a list) and dstar2 = d2(q, y_(j*)) (float32) - the last three written by
//          mass_grad_queries, all four read by the transposes.
//
// No kernel keeps a contribution in memory; no atomics; every output word is written once per launch by a plain store,
// in a summation order that is a function of the arguments alone:
//
//   mass_grad_queries  lane l adds the float64 masses of the list positions l, l + 64, ... < count - 1 to a partial sum
//                      that starts as +0, left to right; the 64 partial sums are added in a butterfly (a_l = a_l +
//                      a_(l ^ s), s = 32, 16, 8, 4, 2, 1) to M; rho = (float)(tau - M), the subtraction in double.  Lane l
//                      then takes acc = fmaf(a_t, q - y_(t), acc) over its positions l, l + 64, ... < count, left to
//                      right from +0, the partial sums are added in the same butterfly, the product with c_q comes last.
//   mass_grad_points   thread (segment, axis) walks its segment of the sorted entry list front to back and continues the
//                      value already in out_p: e = c_q * a (one float32 product), acc = fmaf(-e, q[axis] - y_j[axis],
//                      acc).
//   mass_grad_masses   thread (segment) continues out_m: acc = fmaf(h_q, d2(q, y_j) - dstar2_q, acc) over the entries
//                      that are not their query's crossing entry.
//   d2, dstar2         t0 * t0 + t1 * t1 + ... left to right, every product and sum rounded (no fused step): the same
//                      routine in both kernels, so the two are the same word for the same pair.
//   The entries of a segment ascend by query row, so launches over consecutive groups of query rows give what one launch
//   gives, word for word.
//
// rho is exact - and the forward's rho, bit for bit - whenever the prefix sums are exact float64 numbers in every order
// of addition: integer masses with a total below 2^53 (a coreset's counts).  For other masses M is within count * 2^-53
// relative of the forward's prefix sum (another fixed order of the same non-negative terms), so rho differs from the
// forward's by at most count * 2^-52 * M + 2^-24 * rho: the same number run to run, and a relative error of the
// gradient far below its float32 roundings unless rho is about 0 - where the entry adds about nothing.

#include "../../include/flooder_hip.h"
#include "flood_common.hpp"

using namespace flooder;

namespace {

constexpr int MASS_GRAD_WAVES = 4;   // as grad_queries of flood_dtm_grad.hip: no LDS, 8 waves per SIMD

struct alignas(16) QRow {            // the crossing row of a query
  float coef, rho;
  int32_t cross;
  float dstar2;
};

// |q - y|^2 as the plain float32 sum: every product and every sum rounded, left to right.
template <int DIM>
__device__ __forceinline__ float plain_d2(const float (&q)[DIM], const float* __restrict__ y) {
  const float t0 = q[0] - y[0];
  float d2 = __fmul_rn(t0, t0);
#pragma unroll
  for (int c = 1; c < DIM; ++c) {
    const float t = q[c] - y[c];
    d2 = __fadd_rn(d2, __fmul_rn(t, t));
  }
  return d2;
}

// ------------------------------------------------------------------------------------------------ mass_grad_queries
// One wave per query (grid-stride).  The ids of a row are read coalesced, 64 at a time, in both passes (the second from
// L1); each lane then gathers its own site's row, mass included: 64 independent dependent-load chains per wave.
template <int DIM>
__global__ __launch_bounds__(64 * MASS_GRAD_WAVES) void mass_grad_queries_kernel(
    const float* __restrict__ sites, int64_t n_sites, const float* __restrict__ queries, int64_t n_queries,
    const int32_t* __restrict__ ids, int64_t ld_ids, const int32_t* __restrict__ count,
    const double* __restrict__ tau, QRow* __restrict__ qrow, float* __restrict__ out_q) {
  constexpr int LD = DIM + 1;
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * MASS_GRAD_WAVES + (threadIdx.x >> 6);
  const int64_t n_waves = (int64_t)gridDim.x * MASS_GRAD_WAVES;
  const double target = *tau;
  for (int64_t q = wave; q < n_queries; q += n_waves) {
    int64_t kk = count[q];
    if (kk > ld_ids) kk = ld_ids;   // (a count beyond the row: the row's entries, nothing past them is read)
    const int32_t* row = ids + q * ld_ids;
    if (kk <= 0) {                  // (no list: zeros, no crossing)
      if (lane == 0) {
#pragma unroll
        for (int c = 0; c < DIM; ++c) out_q[q * DIM + c] = 0.f;
        qrow[q].rho = 0.f;
        qrow[q].cross = -1;
        qrow[q].dstar2 = 0.f;
      }
      continue;
    }
    const int last = (int)kk - 1;
    double m_part = 0.0;
    for (int i = lane; i < last; i += 64) {
      const int64_t j = row[i];
      if (j < 0 || j >= n_sites) continue;   // (no site: never read, no mass)
      m_part = m_part + (double)sites[j * LD + DIM];
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) m_part = m_part + __shfl_xor(m_part, s);
    const float rho = (float)(target - m_part);
    const float cf = qrow[q].coef;
    float x0[DIM], acc[DIM];
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      x0[c] = queries[q * DIM + c];
      acc[c] = 0.f;
    }
    if (cf != 0.f) {                          // (wave-uniform; a zero coefficient: +0 words, nothing gathered)
      for (int i = lane; i <= last; i += 64) {
        const int64_t j = row[i];
        if (j < 0 || j >= n_sites) continue;
        const float* x = sites + j * LD;
        const float a = i == last ? rho : x[DIM];
#pragma unroll
        for (int c = 0; c < DIM; ++c) acc[c] = __builtin_fmaf(a, x0[c] - x[c], acc[c]);
      }
#pragma unroll
      for (int c = 0; c < DIM; ++c) {
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) acc[c] = acc[c] + __shfl_xor(acc[c], s);
      }
    }
    if (lane == 0) {
      const int64_t jx = row[last];
#pragma unroll
      for (int c = 0; c < DIM; ++c) out_q[q * DIM + c] = cf != 0.f ? cf * acc[c] : 0.f;
      qrow[q].rho = rho;
      qrow[q].cross = (int32_t)jx;
      qrow[q].dstar2 = jx >= 0 && jx < n_sites ? plain_d2<DIM>(x0, sites + jx * LD) : 0.f;
    }
  }
}

template <int DIM>
struct MassGradQueriesOp {
  static int run(const float* sites, int64_t n_sites, const float* queries, int64_t n_queries, const int32_t* ids,
                 int64_t ld_ids, const int32_t* count, const double* tau, void* qrow, float* out_q, hipStream_t st) {
    if constexpr (DIM < 2) {
      return fail(FLOODER_E_ARG, "flooder_mass_grad_queries_f32: dim must be in 2..8");
    } else {
      int64_t blocks = (n_queries + MASS_GRAD_WAVES - 1) / MASS_GRAD_WAVES;
      if (blocks > 256 * 16) blocks = 256 * 16;
      hipLaunchKernelGGL(mass_grad_queries_kernel<DIM>, dim3((unsigned)blocks), dim3(64 * MASS_GRAD_WAVES), 0, st, sites,
                         n_sites, queries, n_queries, ids, ld_ids, count, tau, (QRow*)qrow, out_q);
      return check_launch("mass_grad_queries");
    }
  }
};

// ------------------------------------------------------------------------------------------------ mass_grad_points
// Thread (segment, axis) as dtm_grad_points_kernel, consecutive threads on the axes of one target: the DIM threads of a
// segment read the same entry and crossing row (one broadcast 16-byte load) and neighbouring words of the query row.
// The chain of a segment is sequential by contract; four entries' loads are issued together, their steps taken in order.
__global__ __launch_bounds__(256) void mass_grad_points_kernel(
    const float* __restrict__ sites, int64_t n_sites, const float* __restrict__ queries, int64_t n_queries, int dim,
    const QRow* __restrict__ qrow, const int64_t* __restrict__ entries, const int64_t* __restrict__ seg_ptr,
    const int32_t* __restrict__ seg_target, int64_t n_seg, float* __restrict__ out_p) {
  const int ld = dim + 1;
  const int64_t n = n_seg * dim;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t g = t / dim;
    const int c = (int)(t - g * dim);
    const int64_t j = seg_target ? (int64_t)seg_target[g] : g;
    int64_t i = seg_ptr[g];
    const int64_t end = seg_ptr[g + 1];
    if (j < 0 || j >= n_sites || i >= end) continue;   // (no site, or an empty segment: nothing is touched)
    const float x = sites[j * ld + c];
    const float mu = sites[j * ld + dim];
    float acc = out_p[j * dim + c];
    for (; i + 4 <= end; i += 4) {
      int64_t q[4];
      float e[4], v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) q[u] = (int64_t)(uint32_t)entries[i + u];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const bool ok = q[u] < n_queries;               // (no query row: never read, adds nothing)
        QRow r = {0.f, 0.f, -1, 0.f};
        if (ok) r = qrow[q[u]];
        e[u] = __fmul_rn(r.coef, (int64_t)r.cross == j ? r.rho : mu);
        v[u] = ok ? queries[q[u] * dim + c] : x;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) acc = __builtin_fmaf(-e[u], v[u] - x, acc);
    }
    for (; i < end; ++i) {
      const int64_t q = (int64_t)(uint32_t)entries[i];
      if (q >= n_queries) continue;
      const QRow r = qrow[q];
      acc = __builtin_fmaf(-__fmul_rn(r.coef, (int64_t)r.cross == j ? r.rho : mu), queries[q * dim + c] - x, acc);
    }
    out_p[j * dim + c] = acc;
  }
}

// ------------------------------------------------------------------------------------------------ mass_grad_masses
// Thread (segment): the same walk, one word per site.  An entry reads the crossing row and the whole query row.
template <int DIM>
__global__ __launch_bounds__(256) void mass_grad_masses_kernel(
    const float* __restrict__ sites, int64_t n_sites, const float* __restrict__ queries, int64_t n_queries,
    const QRow* __restrict__ qrow, const int64_t* __restrict__ entries, const int64_t* __restrict__ seg_ptr,
    const int32_t* __restrict__ seg_target, int64_t n_seg, float* __restrict__ out_m) {
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n_seg; g += (int64_t)gridDim.x * blockDim.x) {
    const int64_t j = seg_target ? (int64_t)seg_target[g] : g;
    int64_t i = seg_ptr[g];
    const int64_t end = seg_ptr[g + 1];
    if (j < 0 || j >= n_sites || i >= end) continue;
    const float* y = sites + j * (DIM + 1);
    float acc = out_m[j];
    for (; i < end; ++i) {
      const int64_t q = (int64_t)(uint32_t)entries[i];
      if (q >= n_queries) continue;
      const QRow r = qrow[q];
      if ((int64_t)r.cross == j) continue;              // (the crossing entry: its mass is not in the value)
      float x0[DIM];
#pragma unroll
      for (int c = 0; c < DIM; ++c) x0[c] = queries[q * DIM + c];
      acc = __builtin_fmaf(0.5f * r.coef, plain_d2<DIM>(x0, y) - r.dstar2, acc);
    }
    out_m[j] = acc;
  }
}

template <int DIM>
struct MassGradMassesOp {
  static int run(const float* sites, int64_t n_sites, const float* queries, int64_t n_queries, const void* qrow,
                 const int64_t* entries, const int64_t* seg_ptr, const int32_t* seg_target, int64_t n_seg, float* out_m,
                 hipStream_t st) {
    if constexpr (DIM < 2) {
      return fail(FLOODER_E_ARG, "flooder_mass_grad_masses_f32: dim must be in 2..8");
    } else {
      int64_t blocks = (n_seg + 255) / 256;
      if (blocks > 256 * 16) blocks = 256 * 16;
      hipLaunchKernelGGL(mass_grad_masses_kernel<DIM>, dim3((unsigned)blocks), dim3(256), 0, st, sites, n_sites, queries,
                         n_queries, (const QRow*)qrow, entries, seg_ptr, seg_target, n_seg, out_m);
      return check_launch("mass_grad_masses");
    }
  }
};

// The argument checks of the two transposes (one set of refusals, the entry's name first).
int check_transpose(const char* dim_msg, const char* count_msg, const char* null_msg, const void* sites, int64_t n_sites,
                    const void* queries, int64_t n_queries, int dim, const void* qrow, const void* entries,
                    const void* seg_ptr, int64_t n_seg, const void* out) {
  if (dim < 2 || dim > 8) return fail(FLOODER_E_ARG, dim_msg);
  if (n_sites < 0 || n_queries < 0 || n_seg < 0) return fail(FLOODER_E_ARG, count_msg);
  if (!sites || !queries || !qrow || !entries || !seg_ptr || !out) return fail(FLOODER_E_ARG, null_msg);
  return FLOODER_OK;
}

}  // namespace

extern "C" {

int flooder_mass_grad_queries_f32(const float* sites, int64_t n_sites, const float* queries, int64_t n_queries, int dim,
                                  const int32_t* ids, int64_t ld_ids, const int32_t* count, const double* tau,
                                  void* qrow, float* out_q, void* stream) {
  if (dim < 2 || dim > 8) return fail(FLOODER_E_ARG, "flooder_mass_grad_queries_f32: dim must be in 2..8");
  if (ld_ids < 1 || ld_ids > FLOODER_KNN_WIDE_MAX)
    return fail(FLOODER_E_ARG, "flooder_mass_grad_queries_f32: ld_ids must be in 1..FLOODER_KNN_WIDE_MAX");
  if (n_sites < 0 || n_queries < 0)
    return fail(FLOODER_E_ARG, "flooder_mass_grad_queries_f32: bad argument (negative count)");
  if (!sites || !queries || !ids || !count || !tau || !qrow || !out_q)
    return fail(FLOODER_E_ARG, "flooder_mass_grad_queries_f32: bad argument (null pointer)");
  if (n_queries == 0) return FLOODER_OK;
  return dispatch_dim<MassGradQueriesOp>(dim, sites, n_sites, queries, n_queries, ids, ld_ids, count, tau, qrow, out_q,
                                         (hipStream_t)stream);
}

int flooder_mass_grad_points_f32(const float* sites, int64_t n_sites, const float* queries, int64_t n_queries, int dim,
                                 const void* qrow, const int64_t* entries, const int64_t* seg_ptr,
                                 const int32_t* seg_target, int64_t n_seg, float* out_p, void* stream) {
  const int rc = check_transpose("flooder_mass_grad_points_f32: dim must be in 2..8",
                                 "flooder_mass_grad_points_f32: bad argument (negative count)",
                                 "flooder_mass_grad_points_f32: bad argument (null pointer)", sites, n_sites, queries,
                                 n_queries, dim, qrow, entries, seg_ptr, n_seg, out_p);
  if (rc != FLOODER_OK) return rc;
  if (n_queries == 0 || n_seg == 0) return FLOODER_OK;
  int64_t blocks = (n_seg * dim + 255) / 256;
  if (blocks > 256 * 16) blocks = 256 * 16;
  hipLaunchKernelGGL(mass_grad_points_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, sites, n_sites,
                     queries, n_queries, dim, (const QRow*)qrow, entries, seg_ptr, seg_target, n_seg, out_p);
  return check_launch("mass_grad_points");
}

int flooder_mass_grad_masses_f32(const float* sites, int64_t n_sites, const float* queries, int64_t n_queries, int dim,
                                 const void* qrow, const int64_t* entries, const int64_t* seg_ptr,
                                 const int32_t* seg_target, int64_t n_seg, float* out_m, void* stream) {
  const int rc = check_transpose("flooder_mass_grad_masses_f32: dim must be in 2..8",
                                 "flooder_mass_grad_masses_f32: bad argument (negative count)",
                                 "flooder_mass_grad_masses_f32: bad argument (null pointer)", sites, n_sites, queries,
                                 n_queries, dim, qrow, entries, seg_ptr, n_seg, out_m);
  if (rc != FLOODER_OK) return rc;
  if (n_queries == 0 || n_seg == 0) return FLOODER_OK;
  return dispatch_dim<MassGradMassesOp>(dim, sites, n_sites, queries, n_queries, qrow, entries, seg_ptr, seg_target, n_seg,
                                        out_m, (hipStream_t)stream);
}

}  // extern "C"
