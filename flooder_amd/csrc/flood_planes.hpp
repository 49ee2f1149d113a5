// flood_planes.hpp - the face-plane table row of one simplex (flood_cell.hip's comment on the slab test says what
// the numbers are for): shared by simplex_planes_kernel (flood_cell.hip) and the launch that prepares a sweep
// (simplex weights + plane rows + the zero fill of the control words in ONE launch: flood_finish.hip).
#pragma once
#include "flood_common.hpp"

namespace flooder {

constexpr int PLANE_ROW = 24;

template <int DIM>
__device__ __forceinline__ void simplex_planes_row(const float* __restrict__ verts, int k1, int64_t s, float* __restrict__ tab) {
  // The source decides the arithmetic: no contraction by the compiler in here, every fused step is written as an fma.
  // Both writers of the table and the float32 replica of the tests (tests/wit_reference.py: plane_row, pinned word for
  // word by tests/test_gpu_plane_rows.py) then compute the same 24 words.
#pragma clang fp contract(off)
  const float* vs = verts + s * (int64_t)k1 * DIM;
  float pn[DIM + 1][DIM], po[DIM + 1], pslack[DIM + 1], org[DIM];
  float sext2 = 0.f;  // squared extent of the simplex around org
#pragma unroll
  for (int k = 0; k < DIM; ++k) org[k] = vs[k];
  for (int j = 1; j < k1; ++j) {
    float e2 = 0.f;
#pragma unroll
    for (int k = 0; k < DIM; ++k) e2 = __builtin_fmaf(vs[j * DIM + k] - org[k], vs[j * DIM + k] - org[k], e2);
    sext2 = __builtin_fmaxf(sext2, e2);
  }
  const float sext = __builtin_sqrtf(sext2);
#pragma unroll
  for (int f = 0; f <= DIM; ++f) {
    po[f] = 3.0e38f;  // disabled plane: the test always passes
    pslack[f] = 0.f;
#pragma unroll
    for (int k = 0; k < DIM; ++k) pn[f][k] = 0.f;
  }
  if (k1 == DIM + 1) {
#pragma unroll
    for (int f = 0; f <= DIM; ++f) {
      int id[DIM];
      int qq = 0;
#pragma unroll
      for (int j = 0; j <= DIM; ++j)
        if (j != f) id[qq++] = j;
      float nrm[DIM];
      float l12;  // |e1|^2 |e2|^2 (3D) or |e|^2 (2D): len2 / l12 = sin^2 of the angle between the edges
      if constexpr (DIM == 3) {
        float e1[3], e2[3];
        float l1 = 0.f, l2 = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          e1[k] = vs[id[1] * 3 + k] - vs[id[0] * 3 + k];
          e2[k] = vs[id[2] * 3 + k] - vs[id[0] * 3 + k];
          l1 = __builtin_fmaf(e1[k], e1[k], l1);
          l2 = __builtin_fmaf(e2[k], e2[k], l2);
        }
        nrm[0] = __builtin_fmaf(e1[1], e2[2], -(e1[2] * e2[1]));
        nrm[1] = __builtin_fmaf(e1[2], e2[0], -(e1[0] * e2[2]));
        nrm[2] = __builtin_fmaf(e1[0], e2[1], -(e1[1] * e2[0]));
        l12 = l1 * l2;
      } else {
        const float ex = vs[id[1] * 2 + 0] - vs[id[0] * 2 + 0];
        const float ey = vs[id[1] * 2 + 1] - vs[id[0] * 2 + 1];
        nrm[0] = ey;
        nrm[1] = -ex;
        l12 = __builtin_fmaf(ex, ex, ey * ey);
      }
      float len2 = 0.f, side = 0.f;
#pragma unroll
      for (int k = 0; k < DIM; ++k) {
        len2 = __builtin_fmaf(nrm[k], nrm[k], len2);
        side = __builtin_fmaf(nrm[k], vs[f * DIM + k] - vs[id[0] * DIM + k], side);
      }
      const bool ok = len2 > 1e-30f && len2 >= 1e-8f * l12 && side * side >= 1e-8f * len2 * sext2;
      const float sc = ok ? (side > 0.f ? -1.f : 1.f) / __builtin_sqrtf(len2) : 0.f;
      float off = 0.f;
#pragma unroll
      for (int k = 0; k < DIM; ++k) {
        pn[f][k] = nrm[k] * sc;
        off = __builtin_fmaf(pn[f][k], vs[id[0] * DIM + k] - org[k], off);
      }
      po[f] = ok ? off : 3.0e38f;
      pslack[f] = ok ? 1e-6f * __builtin_sqrtf(l12 / len2) : 0.f;
    }
  }
  float* row = tab + s * PLANE_ROW;
#pragma unroll
  for (int i = 0; i < PLANE_ROW; ++i) row[i] = 0.f;
#pragma unroll
  for (int k = 0; k < DIM; ++k) row[k] = org[k];
  row[3] = sext;
#pragma unroll
  for (int f = 0; f <= DIM; ++f) {
#pragma unroll
    for (int k = 0; k < DIM; ++k) row[4 + 5 * f + k] = pn[f][k];
    row[4 + 5 * f + 3] = po[f];
    row[4 + 5 * f + 4] = pslack[f];
  }
}

// Node box against the slabs of a region (flood_cell.hip: keep_point).  A point x is kept there when, for every
// plane f, dd_f(x) = fl(sum_k pn[f][k] * fl(x_k - org_k) - po[f]) - a chain of DIM fmas that starts at -po[f] - lies
// in [slab_lo[f], slab_hi[f]].  `false` here says that no x with lo <= x <= hi can pass that test: the node, inner
// node or leaf, holds nothing for the region.  (The cell sweep asks for the leaves a gather has collected.)
//
// Per plane the support interval [smin, smax] of the box along pn[f]: with a_k = fl(lo_k - org_k), b_k = fl(hi_k -
// org_k) - rounding is monotone, so fl(x_k - org_k) lies in [a_k, b_k] for every x in the box - the sum over the axes
// of min / max(pn_k * a_k, pn_k * b_k), minus po[f].  The node goes when smin - pad > slab_hi[f] or smax + pad <
// slab_lo[f].
//
// The pad.  u = 2^-24 (half an ulp), m_k = max(|a_k|, |b_k|), M = |po| + sum_k |pn_k| m_k: no partial sum of either
// computation exceeds M (1 + u)^3 in magnitude.
//   keep_point's chain: DIM fmas, each rounds a partial sum once, u M each              <= 3 u M
//   the support sum:    DIM products rounded, u |pn_k| m_k each, together <= u M;
//                       DIM - 1 additions and the subtraction of po, u M each          <= 4 u M
//   M itself:           |po| + sum_k max(|pn_k a_k|, |pn_k b_k|) - the rounded products, which are fl(|pn_k| m_k) -
//                       a sum of non-negative terms, DIM + DIM roundings: relative error 6 u, taken from below
//   smin - pad, smax + pad: one rounding of a number below M + pad                     <= u (M + pad)
// all of it with second-order terms below 8.1 u M for DIM <= 3: pad = 16 u M = 2^-20 M leaves a factor of two.  The
// absolute term stands for products that leave the normal range (4 roundings of at most 2^-126 each way, or as many
// operands flushed to zero).
// Every comparison is written so that NaN gives "keep": a NaN slab limit, interval end or pad drops nothing.  An
// empty box (lo = +inf, hi = -inf: pad rows of the tree) gives products of infinite size and pad = inf, or NaN
// (0 * inf under a zero normal); a plane switched off (pn = 0, po = 3e38) gives smin = smax = -po = dd of every point, so it drops a node
// only where it drops every point.  fmin / fmax skip a NaN operand, so a NaN box coordinate is NOT covered: callers
// ask here only about nodes that passed the box test, which such a node (and an empty one) fails.
// (tests/test_gather_planes_cpu.py holds the float32 replica and shows that pad = 0 is not enough.)
constexpr float GATHER_PAD_REL = 9.5367431640625e-07f;  // 2^-20
constexpr float GATHER_PAD_ABS = 1.0e-36f;
#ifndef FLOODER_GATHER_PLANES
#define FLOODER_GATHER_PLANES 1  // 0: the cell sweep classifies every leaf whose box meets the region's box (A/B builds)
#endif

template <int DIM, int DP>
__device__ __forceinline__ bool node_meets_slabs(const float (&lo)[DP], const float (&hi)[DP], const float (&pn)[DIM + 1][DIM],
                                                 const float (&po)[DIM + 1], const float (&org)[DIM],
                                                 const float (&slab_lo)[DIM + 1], const float (&slab_hi)[DIM + 1]) {
#pragma clang fp contract(off)
  float a[DIM], b[DIM];
#pragma unroll
  for (int k = 0; k < DIM; ++k) {
    a[k] = lo[k] - org[k];
    b[k] = hi[k] - org[k];
  }
  bool out = false;
#pragma unroll
  for (int f = 0; f <= DIM; ++f) {
    float smin = 0.f, smax = 0.f, mag = __builtin_fabsf(po[f]);
#pragma unroll
    for (int k = 0; k < DIM; ++k) {
      const float pa = pn[f][k] * a[k], pb = pn[f][k] * b[k];
      const float mn = __builtin_fminf(pa, pb), mx = __builtin_fmaxf(pa, pb);
      smin = k == 0 ? mn : smin + mn;
      smax = k == 0 ? mx : smax + mx;
      mag = mag + __builtin_fmaxf(__builtin_fabsf(pa), __builtin_fabsf(pb));  // = fl(|pn_k| m_k)
    }
    smin = smin - po[f];
    smax = smax - po[f];
    const float pad = __builtin_fmaf(GATHER_PAD_REL, mag, GATHER_PAD_ABS);
    out = out || (smin - pad > slab_hi[f]) || (smax + pad < slab_lo[f]);
  }
  return !out;
}

}  // namespace flooder
