// flood_bvh.hpp - the implicit box tree shared by the tree and cell kernels: its level layout, and the float32 bound
// and distance arithmetic of the exact tree walks (internal).
#pragma once
#include "flood_common.hpp"

namespace flooder {

constexpr int LEAF = FLOODER_BVH_LEAF;        // points per leaf
constexpr int FAN = FLOODER_BVH_FANOUT;       // children per inner node (= wave size)
constexpr int MAXL = FLOODER_BVH_MAX_LEVELS;  // levels incl. leaves

struct Levels {
  int n_levels;          // level 0 = leaves ... level n_levels-1 = top (<= 64 nodes)
  int64_t off[MAXL];     // first node of the level in the node array (levels padded to x64)
  int64_t count[MAXL];   // real nodes of the level
};

inline Levels make_levels(int64_t n_pts) {
  Levels lv;
  memset(&lv, 0, sizeof(lv));
  int64_t c = (n_pts + LEAF - 1) / LEAF;
  if (c < 1) c = 1;
  int64_t off = 0;
  int l = 0;
  for (;;) {
    lv.count[l] = c;
    lv.off[l] = off;
    off += (c + FAN - 1) / FAN * FAN;
    ++l;
    if (c <= FAN || l == MAXL) break;
    c = (c + FAN - 1) / FAN;
  }
  lv.n_levels = l;
  return lv;
}

inline int64_t total_nodes(const Levels& lv) {
  const int t = lv.n_levels - 1;
  return lv.off[t] + (lv.count[t] + FAN - 1) / FAN * FAN;
}

// ---- the stack walk, one wave per query (witness_search_kernel, witness_knn_kernel, knn_wide_kernel), host side.  A
// stack word is (group of FAN siblings << 3 | level), at most FAN words per level.
constexpr int WAVES_PER_BLOCK = 4;
constexpr int STACK = FAN * MAXL;
// The cloud's levels, or the refusal of entry `who`: the group has 27 bits, so the leaves make fewer than 2^27 groups.
inline int stack_walk_levels(const char* who, int64_t n_pts, Levels& lv) {
  lv = make_levels(n_pts);
  if ((lv.count[0] + FAN - 1) / FAN < (1LL << 27)) return 0;
  return failf(FLOODER_E_ARG, "%s: cloud too large for the search stack encoding", who);
}
inline dim3 stack_walk_grid(int64_t n) {   // a wave per query, grid-stride above 256 * 16 blocks
  const int64_t blocks = (n + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
  return dim3((unsigned)(blocks < 256 * 16 ? blocks : 256 * 16));
}

// ---- the float32 arithmetic of every path that promises the exhaustive minima bit for bit:
// the tree sweep, the sorted-sample sweep, the finish, the k-nearest sweep and the witness searches of the gradient
// call these, so a change to the margin or to the order of the fmafs is made once.  A call that changed a kernel's
// registers or spills, or that cost it time, was not kept (profiles/tree_helpers_isa.txt): such a site carries the
// arithmetic written out under a comment that names the helper.  Not shared at all, and to be kept in step by hand: the
// sample as an fmaf chain over the vertices (grep "__builtin_fmaf(w"), the 16-row leaf loop (flood_bvh.hip,
// flood_finish.hip, flood_sorted.hip, flood_cell.hip), the frontier walk of the six sweeps (sweep_knn_ids_kernel's is a
// copy of sweep_knn_kernel's with strict culls) and the stack walk of the two witness kernels, witness_power_kernel,
// knn_wide_kernel and knn_mass_kernel: five copies on the device (the last two share their list helpers and ladder,
// flood_knn_list.hpp); the wide entry's HOST side is the family's (above; knn_check_ranges).  For the two sweep_knn
// kernels one shared body under an IDS template flag was tried at compile level, in two wordings: it moved the
// registers of nearly every instantiation of flood_knn.hip, those of the untouched value path included.  No such build
// has been timed, so the copy stands (the note above sweep_knn_ids_kernel has the figures).  The double sweep of
// flood_f64.hip shares no rounding with any of this.

// Culling margin: a box, a leaf or a level is skipped only when !(lb * SAFE < bound).  lb is a float32 LOWER bound
// of a squared distance whose rounding error is a few ulp; 1e-5 relative is far above that, so a cull never removes a
// pair that could change a minimum.
constexpr float SAFE = 0.99999f;

// Squared gap between the boxes [lo, hi] and [tlo, thi]: gap = max(max(lo - thi, tlo - hi), 0) per axis, summed from
// 0.f with one fmaf per axis, in axis order.
template <int DIM, class B, class T>
__device__ __forceinline__ float box_gap2(const B& lo, const B& hi, const T& tlo, const T& thi) {
  float lb = 0.f;
#pragma unroll
  for (int k = 0; k < DIM; ++k) {
    const float gap = __builtin_fmaxf(__builtin_fmaxf(lo[k] - thi[k], tlo[k] - hi[k]), 0.f);
    lb = __builtin_fmaf(gap, gap, lb);
  }
  return lb;
}
// ... between the point p (its own box) and the box [lo, hi]
template <int DIM, class P, class B>
__device__ __forceinline__ float box_gap2(const P& p, const B& lo, const B& hi) {
  return box_gap2<DIM>(lo, hi, p, p);
}

// v of lane j, axis by axis (j wave-uniform)
template <int DIM>
__device__ __forceinline__ void readlane_row(const float (&v)[DIM], int j, float (&out)[DIM]) {
#pragma unroll
  for (int k = 0; k < DIM; ++k) out[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v[k]), j));
}

// Child `lane` of group `grp` at level `lvl`: its box into (c_lo, c_hi) and its box_gap2 to [tlo, thi]; a lane past the
// end of the level holds the empty box and +inf.
template <int DIM>
__device__ __forceinline__ float child_box_bound(const float* __restrict__ nodes, const Levels& lv, int lvl, int64_t grp,
                                                 int lane, const float (&tlo)[DIM], const float (&thi)[DIM],
                                                 float (&c_lo)[DIM], float (&c_hi)[DIM]) {
  constexpr int DP = padded_dim(DIM);
  const int64_t idx = grp * FAN + lane;
  float lb = __builtin_inff();
#pragma unroll
  for (int k = 0; k < DIM; ++k) { c_lo[k] = __builtin_inff(); c_hi[k] = -__builtin_inff(); }
  if (idx < lv.count[lvl]) {
    float lo[DP], hi[DP];
    const float* nb = nodes + (lv.off[lvl] + idx) * 2 * DP;
    load_row<DP>(nb, lo);
    load_row<DP>(nb + DP, hi);
#pragma unroll
    for (int k = 0; k < DIM; ++k) { c_lo[k] = lo[k]; c_hi[k] = hi[k]; }
    lb = box_gap2<DIM>(lo, hi, tlo, thi);
  }
  return lb;
}
// ... against one point (the searches that own a single sample keep no child boxes)
template <int DIM>
__device__ __forceinline__ float child_point_bound(const float* __restrict__ nodes, const Levels& lv, int lvl,
                                                   int64_t grp, int lane, const float (&p)[DIM]) {
  float c_lo[DIM], c_hi[DIM];
  return child_box_bound<DIM>(nodes, lv, lvl, grp, lane, p, p, c_lo, c_hi);
}

// Squared distance: t * t on axis 0, then one fmaf per further axis (t = p - x).
template <int DIM, class P, class X>
__device__ __forceinline__ float dist2(const P& p, const X& x) {
  float d;
#pragma unroll
  for (int k = 0; k < DIM; ++k) {
    const float t = p[k] - x[k];
    d = k == 0 ? t * t : __builtin_fmaf(t, t, d);
  }
  return d;
}

}  // namespace flooder
