// flood_power.hip - the weighted (power-distance) tree sweep (gfx950): flood_complex(point_weights=w).
//
// Every point x of the cloud carries a weight w_x >= 0 and a sample p is measured by
//     f(p)^2 = min_x ( |p - x|^2 + w_x^2 ),
// the power distance of the weighted Cech / DTM filtration.  flooder_sweep_power_f32 writes the float32 bits of that
// minimum into the (S, R) buffer that flooder_face_max_f32 reads - the square root and the face maxima stay there.
//
//   sweep_power<DIM>   sweep_knn_kernel<DIM, K, false, SORTED> at one value per lane: one wave owns 64 consecutive
//                      entries of the sample order - NULL: the identity order g = 0 .. N-1 cut simplex by simplex, a tile
//                      is 64 consecutive rows of ONE simplex as in flooder_sweep_knn_f32 (flat tiles of 64 straddle the
//                      compact 64-row runs of the lattice whenever R is no multiple of 64: 3x the leaf tests at cfg 2,
//                      DESIGN.md 10) -, one sample per lane rebuilt in registers (fma in vertex order), the nearest-
//                      first wave-uniform walk over the same nodes with the LDS level stack, the 16 rows of a leaf AND
//                      its 16 weights through the scalar cache.  The word of a pair is
//                          fmaf(w, w, dist2<DIM>(p, x))
//                      - the project's squared distance followed by ONE fma with the weight itself - and a lane keeps
//                      the smallest.
//
// Bounds.  node_w[c] (flooder_node_min_f32 of the weights) is the smallest weight below node c, so
//     child:  fmaf(node_w[c], node_w[c], box_gap2(box of c, box of the tile))
//     leaf:   fmaf(node_w[leaf], node_w[leaf], box_gap2(p, box of the leaf))
// are the Euclidean bounds of the family with the node's weight added the way a pair adds its own.  Rounded fma is
// monotone in each non-negative argument, the gap is a lower bound of every distance below the node up to a few ulp
// and the node's weight is <= every weight below it: both are lower bounds of every pair word below the node within
// the margin SAFE, as the Euclidean ones are.  A child, a leaf or a level is skipped only when !(lb * SAFE < bound),
// bound = the largest running minimum of the wave (levels, children) or the lane's own (leaf test).
//
// Exactness.  A minimum does not depend on the order in which its elements are offered, and what is skipped cannot
// lower any lane's minimum - so the word written is the minimum over ALL points, bit for bit, whatever the tree and
// whichever samples share a wave.  Zero weights give fmaf(0, 0, d2) = d2: the words of the k = 1 sweeps.  The lift
// (x, w) in DIM + 1 dimensions swept by flooder_sweep_knn_sorted_f32 at k = 1 against (p, 0) ends its dist2 chain in
// fmaf(0 - w, 0 - w, d2) - the same word: the oracle of tests/test_gpu_power_kernel.py, not the path.
//
// flooder_node_min_f32 builds node_w: the minimum of a value per tree row over every node of the box tree, in the
// layout of the node array (Levels), padding slots +inf.  One launch per level, plain vector stores, no atomics.
//
//   witness_power<DIM> WHICH point attains a power word (flooder_witness_power; power_filtration, power_nearest): one
//                      wave per query, the LDS group stack of witness_search_kernel (flood_grad.hip).  The sample p* is
//                      rebuilt with the sweeps' fma in vertex order; a node of level lvl, slot idx is opened iff
//                          fmaf(nw, nw, box_gap2(p*, box)) * SAFE <= target,   nw = node_w[lv.off[lvl] + idx]
//                      - the leaf bound above against the KNOWN minimum, non-strict: a box exactly at the target is
//                      opened -, leaves are evaluated four at a time, one point per lane, with the word of the sweep,
//                      fmaf(w, w, dist2(p*, x)), and the witness is the smallest original id whose word has exactly
//                      the target bits.  Every pair word below a node is at least the node's bound within SAFE (Bounds),
//                      so a skipped node holds no point at the target: the search is exhaustive over the points that
//                      can match.  Padding rows (coordinates and weight +inf) never match and rw < n_pts guards them
//                      as well.  Zero weights: fmaf(0, 0, x) = x in the bound and in the word - node for node and
//                      point for point the tests of witness_search_kernel, the same outputs.

#include "flood_common.hpp"
#include "flood_bvh.hpp"

using namespace flooder;

namespace {

// level 0: node i = min over the LEAF rows of leaf i; `padded` = the level's slot count (x64), slots past `count` +inf
__global__ __launch_bounds__(256) void node_min_leaf_kernel(const float* __restrict__ vals, int64_t count, int64_t padded,
                                                            float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= padded) return;
  float m = __builtin_inff();
  if (i < count) {
    static_assert(LEAF % 4 == 0, "a leaf's values are read as float4");
    const float4* v = reinterpret_cast<const float4*>(vals + i * LEAF);
#pragma unroll
    for (int q = 0; q < LEAF / 4; ++q) {
      const float4 t = v[q];
      m = __builtin_fminf(m, __builtin_fminf(__builtin_fminf(t.x, t.y), __builtin_fminf(t.z, t.w)));
    }
  }
  out[i] = m;
}

// level l > 0: one wave per node, lane j reads child j (the child level is padded to x64 with +inf)
__global__ __launch_bounds__(256) void node_min_inner_kernel(const float* __restrict__ child, int64_t count, int64_t padded,
                                                             float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= padded) return;
  float m = __builtin_inff();
  if (i < count) m = wave_min_f32(child[i * FAN + lane]);
  if (lane == 0) out[i] = m;
}

template <int DIM>
__global__ __launch_bounds__(256) void sweep_power_kernel(
    const float* __restrict__ pts, const float* __restrict__ nodes, Levels lv, const float* __restrict__ verts,
    const float* __restrict__ weights, int k1, int R, int64_t n_simplices, int32_t* __restrict__ queue,
    uint32_t* __restrict__ out_bits, unsigned long long* __restrict__ stats, const uint32_t* __restrict__ order,
    const float* __restrict__ w_sorted, const float* __restrict__ node_w) {
  constexpr int DP = padded_dim(DIM);
  __shared__ float s_lb[4][MAXL][FAN];
  __shared__ int64_t s_grp[4][MAXL];
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  const int tiles = (R + 63) / 64;
  const int64_t n_samples = n_simplices * (int64_t)R;
  const int64_t n_items = order ? (n_samples + 63) / 64 : n_simplices * tiles;
  const int top = lv.n_levels - 1;
  unsigned long long n_leaf_eval = 0, n_leaf_test = 0, n_node_test = 0, max_item_tests = 0;

  int q_shard = (int)(((int64_t)blockIdx.x * 4 + wv) % QSHARDS), q_tried = 0;
  for (;;) {
    const int64_t g = queue_pop(queue, q_shard, q_tried, n_items, lane);  // sharded heads (flood_common.hpp)
    if (g < 0) break;
    const unsigned long long tests_before = n_leaf_test + n_node_test;
    // ---- this lane's sample (s, r): entry `lane` of the item's run of the order, or (order NULL: the identity order
    // simplex by simplex) of the item's simplex - the rows of a simplex come in compact runs of 64 (sample_order), and
    // a tile that straddled two runs or two simplices would search for both
    int64_t s;
    int r;
    bool live;
    if (order) {
      const int64_t pos = g * 64 + lane;
      live = pos < n_samples;
      const uint32_t id = order[live ? pos : n_samples - 1];  // duplicate of the last entry, never stored
      const uint32_t si = id / (uint32_t)R;
      s = (int64_t)si;
      r = (int)(id - si * (uint32_t)R);
    } else {
      s = g / tiles;
      r = (int)(g - s * tiles) * 64 + lane;
      live = r < R;
      if (!live) r = R - 1;  // duplicate of the last sample, never stored
    }
    // p = sum_j w[r,j] * v[s,j,:], as sweep_bvh builds it
    float p[DIM];
    const float* vs = verts + s * (int64_t)k1 * DIM;
#pragma unroll
    for (int c = 0; c < DIM; ++c) p[c] = 0.f;
    for (int j = 0; j < k1; ++j) {
      const float w = weights[(int64_t)r * k1 + j];
#pragma unroll
      for (int c = 0; c < DIM; ++c) p[c] = __builtin_fmaf(w, vs[j * DIM + c], p[c]);
    }
    // (the int32 word of the float: never negative and never NaN, so the signed integer order is the value order)
    int best = (int)INF_BITS;

    // ---- bounding box of the tile (wave-uniform)
    float tlo[DIM], thi[DIM];
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      tlo[c] = wave_min_f32(p[c]);
      thi[c] = wave_max_f32(p[c]);
    }
    float M = __builtin_inff();  // largest running minimum of the tile (wave-uniform)

    // child `lane` of group `grp` at level `lvl`: its box (registers) and the lower bound of every pair word below it
    // against the tile box (a lane past the end of the level: +inf; its slot of node_w is padding, +inf as well)
    float c_lo[DIM], c_hi[DIM];
    auto child_bounds = [&](int lvl, int64_t grp) -> float {
      const float gap2 = child_box_bound<DIM>(nodes, lv, lvl, grp, lane, tlo, thi, c_lo, c_hi);
      const float nw = node_w[lv.off[lvl] + grp * FAN + lane];
      return __builtin_fmaf(nw, nw, gap2);
    };

    // inner levels keep their per-lane bounds in LDS; the leaf level runs in registers (lb0, c_lo / c_hi)
    int lvl = top;
    float lb0 = child_bounds(top, 0);
    int64_t grp0 = 0;
    ++n_node_test;
    if (top > 0) {
      s_lb[wv][top][lane] = lb0;
      if (lane == 0) s_grp[wv][top] = 0;
    }
    for (;;) {
      if (lvl > 0) {
        const float lbv = s_lb[wv][lvl][lane];
        const float mn = wave_min_f32(lbv);
        if (!(mn * SAFE < M)) {  // nothing left at this level can lower a minimum of the tile
          if (++lvl > top) break;
          continue;
        }
        const int j = __builtin_ctzll(__ballot(lbv == mn));
        if (lane == j) s_lb[wv][lvl][lane] = __builtin_inff();  // visited
        const int64_t c = wave_uniform64(s_grp[wv][lvl]) * FAN + j;
        --lvl;
        const float lb = child_bounds(lvl, c);
        ++n_node_test;
        if (lvl > 0) {
          s_lb[wv][lvl][lane] = lb;
          if (lane == 0) s_grp[wv][lvl] = c;
        } else {
          lb0 = lb;
          grp0 = c;
        }
        continue;
      }
      // ---- leaf level: nearest unvisited leaf of the current group
      const float mn = wave_min_f32(lb0);
      if (!(mn * SAFE < M)) {
        if (++lvl > top) break;
        continue;
      }
      const int j = __builtin_ctzll(__ballot(lb0 == mn));
      if (lane == j) lb0 = __builtin_inff();  // visited
      const int64_t c = grp0 * FAN + j;
      ++n_leaf_test;
      // can the minimum of any lane still drop against leaf c?  (its box comes from lane j, its weight is wave-uniform)
      float lbp = 0.f;  // (readlane_row + box_gap2 of flood_bvh.hpp, axis by axis, as sweep_knn_kernel has it)
#pragma unroll
      for (int a = 0; a < DIM; ++a) {
        const float blo = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c_lo[a]), j));
        const float bhi = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c_hi[a]), j));
        const float gap = __builtin_fmaxf(__builtin_fmaxf(blo - p[a], p[a] - bhi), 0.f);
        lbp = __builtin_fmaf(gap, gap, lbp);
      }
      const float wl = node_w[c];   // level 0 starts the node array: the smallest weight of leaf c
      lbp = __builtin_fmaf(wl, wl, lbp);
      if (__ballot(lbp * SAFE < __int_as_float(best)) == 0ull) continue;
      ++n_leaf_eval;
      const float* cp = pts + c * (int64_t)LEAF * DP;
      const float* cw = w_sorted + c * (int64_t)LEAF;
      constexpr int NB = DP == 8 ? 4 : 8;   // rows in SGPRs at a time (32 scalar registers at most) and their weights
      // (8-float rows: not unrolled - unrolled, DIM 5..8 take 82..119 vector registers instead of 62..87 and lose one
      // to two waves per SIMD; 2- and 4-float rows: both halves of the leaf in flight, fewer scalar registers moved
      // to vector lanes - profiles/power_kernel_resources.txt)
      constexpr int UNROLL = DP == 8 ? 1 : LEAF / NB;
#pragma unroll UNROLL
      for (int h = 0; h < LEAF; h += NB) {
        typename RowVec<DP>::type cc[NB];
#pragma unroll
        for (int u = 0; u < NB; ++u) cc[u] = load_uniform_row<DP>(cp + (h + u) * DP);
        const typename RowVec<NB>::type ww = load_uniform_row<NB>(cw + h);
#pragma unroll
        for (int u = 0; u < NB; ++u) {
          float d;  // (dist2 of flood_bvh.hpp written out, then the weight)
#pragma unroll
          for (int a = 0; a < DIM; ++a) {
            const float t = p[a] - cc[u][a];
            d = a == 0 ? t * t : __builtin_fmaf(t, t, d);
          }
          d = __builtin_fmaf(ww[u], ww[u], d);
          const int di = __float_as_int(d);
          best = di < best ? di : best;
        }
      }
      M = wave_max_f32(__int_as_float(best));
    }

    if (live) out_bits[s * (int64_t)R + r] = (uint32_t)best;
    const unsigned long long item_tests = n_leaf_test + n_node_test - tests_before;
    max_item_tests = item_tests > max_item_tests ? item_tests : max_item_tests;
  }
  if (stats && lane == 0 && (n_node_test | n_leaf_test) != 0ull) {
    atomicMax(&stats[3], max_item_tests);
    atomicAdd(&stats[0], n_leaf_eval);
    atomicAdd(&stats[1], n_leaf_test);
    atomicAdd(&stats[2], n_node_test);
  }
}

template <int DIM>
struct PowerLaunch {
  static int run(const flooder_knn_sorted_t& a, const float* w_sorted, const float* node_w, const Levels& lv,
                 hipStream_t st) {
    if constexpr (DIM < 2) {
      return fail(FLOODER_E_ARG, "dim must be in 2..8");
    } else {
      const int64_t n_items = a.sample_order ? (a.n_simplices * (int64_t)a.R + 63) / 64
                                             : a.n_simplices * ((a.R + 63) / 64);
      int64_t grid = g_bvh_grid;  // persistent blocks; 4 independent waves each
      if (grid > (n_items + 3) / 4) grid = (n_items + 3) / 4;
      hipLaunchKernelGGL((sweep_power_kernel<DIM>), dim3((unsigned)grid), dim3(256), 0, st, a.pts_sorted, a.nodes, lv,
                         a.verts, a.weights, a.k1, a.R, a.n_simplices, a.queue, a.out_bits,
                         reinterpret_cast<unsigned long long*>(a.stats),
                         reinterpret_cast<const uint32_t*>(a.sample_order), w_sorted, node_w);
      return check_launch("sweep_power");
    }
  }
};

// ---- several weight vectors in one walk (flooder_sweep_power_profile_f32; power_profile, dtm_profile) -------------
//
// node_min_cols: node_min_leaf_kernel / node_min_inner_kernel for nc interleaved columns - a thread (a wave) per
// (node, column), the same minima, plain stores.
__global__ __launch_bounds__(256) void node_min_cols_leaf_kernel(const float* __restrict__ vals, int64_t count,
                                                                 int64_t padded, int nc, float* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= padded * nc) return;
  const int64_t i = t / nc;
  const int c = (int)(t - i * nc);
  float m = __builtin_inff();
  if (i < count) {
    const float* v = vals + i * LEAF * nc + c;
#pragma unroll
    for (int q = 0; q < LEAF; ++q) m = __builtin_fminf(m, v[(int64_t)q * nc]);
  }
  out[t] = m;
}

__global__ __launch_bounds__(256) void node_min_cols_inner_kernel(const float* __restrict__ child, int64_t count,
                                                                  int64_t padded, int nc, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= padded * nc) return;
  const int64_t i = t / nc;
  const int c = (int)(t - i * nc);
  float m = __builtin_inff();
  if (i < count) m = wave_min_f32(child[(i * FAN + lane) * nc + c]);
  if (lane == 0) out[t] = m;
}

// sweep_power_profile<DIM, NC>: sweep_power_kernel with NC running minima per lane, NC = n_cols rounded up to 1, 2, 4
// or 8 = the row length of w_cols and node_w_cols.  Per pair ONE dist2 chain, then fmaf(w_c, w_c, d2) and a min per
// column: plane c holds the word sweep_power_kernel writes with column c's weights - a minimum does not depend on the
// order of its elements, nor on further elements that are not below it.
//
// Binding rule.  With lb_c = fmaf(nw_c, nw_c, gap2) (nw_c = node_w_cols[node, c]) a child, a leaf or a level is skipped
// only when !(lb_c * SAFE < bound_c) in EVERY column c < n_cols: bound_c = M[c], the largest running minimum of the
// tile in column c (children, levels), or the lane's own best[c] (leaves).  What is visited beyond a column's own walk
// offers it points that are not below its minimum.
//   - a group of children is tested per lane when it is loaded: a child dead in every column gets gap +inf (the M[c]
//     only shrink: it stays dead); the others keep their GEOMETRIC gap2, one float per child, in registers (leaf level)
//     or in the LDS level stack (inner levels) - the stack is not multiplied by NC;
//   - the walk takes the live child of the smallest gap2 first.  mn = that gap2 is a lower bound of every lb_c of every
//     child left, so !(mn * SAFE < max_c M[c]) ends the level; else the child's own NC node weights come in by one
//     scalar load and its columns are tested against the M[c] of NOW before it is opened.
// Padding columns (n_cols <= c < NC) are LEFT OUT of every test - they never keep a node alive, whatever they hold
// (flooder_amd fills them with +inf) - their minima are computed and thrown away, and no plane is written for them.
// A leaf row's NC weights are loaded with the row (never all 16 rows and their weights at once: SGPRs).
template <int DIM, int NC>
__global__ __launch_bounds__(256) void sweep_power_profile_kernel(
    const float* __restrict__ pts, const float* __restrict__ nodes, Levels lv, const float* __restrict__ verts,
    const float* __restrict__ weights, int k1, int R, int64_t n_simplices, int32_t* __restrict__ queue,
    uint32_t* __restrict__ out_bits, unsigned long long* __restrict__ stats, const uint32_t* __restrict__ order,
    const float* __restrict__ w_cols, const float* __restrict__ node_w_cols, int n_cols) {
  constexpr int DP = padded_dim(DIM);
  __shared__ float s_lb[4][MAXL][FAN];
  __shared__ int64_t s_grp[4][MAXL];
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  const int tiles = (R + 63) / 64;
  const int64_t n_samples = n_simplices * (int64_t)R;
  const int64_t n_items = order ? (n_samples + 63) / 64 : n_simplices * tiles;
  const int top = lv.n_levels - 1;
  unsigned long long n_leaf_eval = 0, n_leaf_test = 0, n_node_test = 0, max_item_tests = 0;

  int q_shard = (int)(((int64_t)blockIdx.x * 4 + wv) % QSHARDS), q_tried = 0;
  for (;;) {
    const int64_t g = queue_pop(queue, q_shard, q_tried, n_items, lane);  // sharded heads (flood_common.hpp)
    if (g < 0) break;
    const unsigned long long tests_before = n_leaf_test + n_node_test;
    // ---- this lane's sample (s, r), as sweep_power_kernel takes it
    int64_t s;
    int r;
    bool live;
    if (order) {
      const int64_t pos = g * 64 + lane;
      live = pos < n_samples;
      const uint32_t id = order[live ? pos : n_samples - 1];  // duplicate of the last entry, never stored
      const uint32_t si = id / (uint32_t)R;
      s = (int64_t)si;
      r = (int)(id - si * (uint32_t)R);
    } else {
      s = g / tiles;
      r = (int)(g - s * tiles) * 64 + lane;
      live = r < R;
      if (!live) r = R - 1;  // duplicate of the last sample, never stored
    }
    float p[DIM];
    const float* vs = verts + s * (int64_t)k1 * DIM;
#pragma unroll
    for (int c = 0; c < DIM; ++c) p[c] = 0.f;
    for (int j = 0; j < k1; ++j) {
      const float w = weights[(int64_t)r * k1 + j];
#pragma unroll
      for (int c = 0; c < DIM; ++c) p[c] = __builtin_fmaf(w, vs[j * DIM + c], p[c]);
    }
    int best[NC];   // (the int32 words of the floats: never negative, never NaN)
    float M[NC];    // largest running minimum of the tile per column (wave-uniform)
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      best[c] = (int)INF_BITS;
      M[c] = __builtin_inff();
    }
    float Mmax = __builtin_inff();   // max over the real columns of M[c]

    float tlo[DIM], thi[DIM];
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      tlo[c] = wave_min_f32(p[c]);
      thi[c] = wave_max_f32(p[c]);
    }

    // child `lane` of group `grp` at level `lvl`: its box (registers) and its geometric gap2 to the tile box, +inf when
    // no real column can still gain below it (or the lane is past the end of the level)
    float c_lo[DIM], c_hi[DIM];
    auto child_gaps = [&](int lvl, int64_t grp) -> float {
      const float gap2 = child_box_bound<DIM>(nodes, lv, lvl, grp, lane, tlo, thi, c_lo, c_hi);
      float nw[NC];   // (a slot past the end of the level is padding of the node array: +inf in every column)
      if constexpr (NC == 1) nw[0] = node_w_cols[lv.off[lvl] + grp * FAN + lane];
      else load_row<NC>(node_w_cols + (lv.off[lvl] + grp * FAN + lane) * NC, nw);
      bool alive = false;
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c < n_cols) alive = alive || __builtin_fmaf(nw[c], nw[c], gap2) * SAFE < M[c];
      return alive ? gap2 : __builtin_inff();
    };
    // the node weights of ONE node (wave-uniform address): does any real column pass with the gap `gap2`?
    auto node_alive = [&](int64_t node, float gap2) -> bool {
      const typename RowVec<NC>::type nw = load_uniform_row<NC>(node_w_cols + node * NC);
      bool alive = false;
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c < n_cols) alive = alive || __builtin_fmaf(nw[c], nw[c], gap2) * SAFE < M[c];
      return alive;
    };

    int lvl = top;
    float lb0 = child_gaps(top, 0);
    int64_t grp0 = 0;
    ++n_node_test;
    if (top > 0) {
      s_lb[wv][top][lane] = lb0;
      if (lane == 0) s_grp[wv][top] = 0;
    }
    for (;;) {
      if (lvl > 0) {
        const float lbv = s_lb[wv][lvl][lane];
        const float mn = wave_min_f32(lbv);
        if (!(mn * SAFE < Mmax)) {  // nothing left at this level can lower a minimum of the tile in any column
          if (++lvl > top) break;
          continue;
        }
        const int j = __builtin_ctzll(__ballot(lbv == mn));
        if (lane == j) s_lb[wv][lvl][lane] = __builtin_inff();  // visited
        const int64_t c = wave_uniform64(s_grp[wv][lvl]) * FAN + j;
        if (!node_alive(lv.off[lvl] + c, mn)) continue;   // (node c of this level) dead in every column by now
        --lvl;
        const float lb = child_gaps(lvl, c);
        ++n_node_test;
        if (lvl > 0) {
          s_lb[wv][lvl][lane] = lb;
          if (lane == 0) s_grp[wv][lvl] = c;
        } else {
          lb0 = lb;
          grp0 = c;
        }
        continue;
      }
      // ---- leaf level: nearest unvisited live leaf of the current group
      const float mn = wave_min_f32(lb0);
      if (!(mn * SAFE < Mmax)) {
        if (++lvl > top) break;
        continue;
      }
      const int j = __builtin_ctzll(__ballot(lb0 == mn));
      if (lane == j) lb0 = __builtin_inff();  // visited
      const int64_t c = grp0 * FAN + j;
      // the leaf's NC smallest weights (level 0 starts the node array; wave-uniform: one scalar load)
      const typename RowVec<NC>::type wl = load_uniform_row<NC>(node_w_cols + c * NC);
      ++n_leaf_test;
      float lbp = 0.f;  // gap2 of the lane's own sample to the leaf's box (it comes from lane j)
#pragma unroll
      for (int a = 0; a < DIM; ++a) {
        const float blo = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c_lo[a]), j));
        const float bhi = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c_hi[a]), j));
        const float gap = __builtin_fmaxf(__builtin_fmaxf(blo - p[a], p[a] - bhi), 0.f);
        lbp = __builtin_fmaf(gap, gap, lbp);
      }
      bool gain = false;   // can this lane's minimum still drop in some real column?
#pragma unroll
      for (int cc = 0; cc < NC; ++cc)
        if (cc < n_cols) gain = gain || __builtin_fmaf(wl[cc], wl[cc], lbp) * SAFE < __int_as_float(best[cc]);
      if (__ballot(gain) == 0ull) continue;
      ++n_leaf_eval;
      const float* cp = pts + c * (int64_t)LEAF * DP;
      const float* cw = w_cols + c * (int64_t)LEAF * NC;
      // rows in SGPRs at a time, each with its NC weights: at most 48 scalar registers
      constexpr int NB = (DP + NC) * 8 <= 48 ? 8 : ((DP + NC) * 4 <= 48 ? 4 : 2);
      // (not unrolled for 8-float rows, as in sweep_power_kernel, nor for 8 columns: unrolled, <2..4, 8> moved 115 to 220
      // scalar registers to vector lanes and ran 4 waves per SIMD - profiles/power_profile_kernel_resources.txt)
      constexpr int UNROLL = DP == 8 || NC == 8 ? 1 : LEAF / NB;
#pragma unroll UNROLL
      for (int h = 0; h < LEAF; h += NB) {
        typename RowVec<DP>::type xr[NB];
        typename RowVec<NC>::type wr[NB];
#pragma unroll
        for (int u = 0; u < NB; ++u) {
          xr[u] = load_uniform_row<DP>(cp + (h + u) * DP);
          wr[u] = load_uniform_row<NC>(cw + (h + u) * NC);
        }
#pragma unroll
        for (int u = 0; u < NB; ++u) {
          float d;  // (dist2 of flood_bvh.hpp written out, then the weight of every column)
#pragma unroll
          for (int a = 0; a < DIM; ++a) {
            const float t = p[a] - xr[u][a];
            d = a == 0 ? t * t : __builtin_fmaf(t, t, d);
          }
#pragma unroll
          for (int cc = 0; cc < NC; ++cc) {
            const int di = __float_as_int(__builtin_fmaf(wr[u][cc], wr[u][cc], d));
            best[cc] = di < best[cc] ? di : best[cc];
          }
        }
      }
      Mmax = 0.f;
#pragma unroll
      for (int cc = 0; cc < NC; ++cc) {
        M[cc] = wave_max_f32(__int_as_float(best[cc]));
        if (cc < n_cols) Mmax = __builtin_fmaxf(Mmax, M[cc]);
      }
    }

    if (live) {
      const int64_t cell = s * (int64_t)R + r;
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c < n_cols) out_bits[c * n_samples + cell] = (uint32_t)best[c];
    }
    const unsigned long long item_tests = n_leaf_test + n_node_test - tests_before;
    max_item_tests = item_tests > max_item_tests ? item_tests : max_item_tests;
  }
  if (stats && lane == 0 && (n_node_test | n_leaf_test) != 0ull) {
    atomicMax(&stats[3], max_item_tests);
    atomicAdd(&stats[0], n_leaf_eval);
    atomicAdd(&stats[1], n_leaf_test);
    atomicAdd(&stats[2], n_node_test);
  }
}

template <int DIM>
struct PowerProfileLaunch {
  template <int NC>
  static void launch(const flooder_knn_sorted_t& a, int n_cols, const float* w_cols, const float* node_w_cols,
                     const Levels& lv, dim3 grid, hipStream_t st) {
    hipLaunchKernelGGL((sweep_power_profile_kernel<DIM, NC>), grid, dim3(256), 0, st, a.pts_sorted, a.nodes, lv, a.verts,
                       a.weights, a.k1, a.R, a.n_simplices, a.queue, a.out_bits,
                       reinterpret_cast<unsigned long long*>(a.stats),
                       reinterpret_cast<const uint32_t*>(a.sample_order), w_cols, node_w_cols, n_cols);
  }
  static int run(const flooder_knn_sorted_t& a, int n_cols, const float* w_cols, const float* node_w_cols,
                 const Levels& lv, hipStream_t st) {
    if constexpr (DIM < 2) {
      return fail(FLOODER_E_ARG, "dim must be in 2..8");
    } else {
      const int64_t n_items = a.sample_order ? (a.n_simplices * (int64_t)a.R + 63) / 64
                                             : a.n_simplices * ((a.R + 63) / 64);
      int64_t grid = g_bvh_grid;  // persistent blocks; 4 independent waves each
      if (grid > (n_items + 3) / 4) grid = (n_items + 3) / 4;
      const dim3 gd((unsigned)grid);
      // the row length of w_cols / node_w_cols: n_cols rounded up to 1, 2, 4 or 8
      if (n_cols <= 1) launch<1>(a, n_cols, w_cols, node_w_cols, lv, gd, st);
      else if (n_cols <= 2) launch<2>(a, n_cols, w_cols, node_w_cols, lv, gd, st);
      else if (n_cols <= 4) launch<4>(a, n_cols, w_cols, node_w_cols, lv, gd, st);
      else launch<8>(a, n_cols, w_cols, node_w_cols, lv, gd, st);
      return check_launch("sweep_power_profile");
    }
  }
};

// One wave per query; the stack holds groups of 64 sibling nodes (level, group) as in witness_search_kernel
// (flood_grad.hip: the pop, the push and the four-leaf step are its steps; keep in step).
template <int DIM>
__global__ __launch_bounds__(256) void witness_power_kernel(const float* __restrict__ pts, int64_t n_pts,
                                                            const float* __restrict__ nodes, Levels lv,
                                                            const int32_t* __restrict__ order,
                                                            const float* __restrict__ verts,
                                                            const float* __restrict__ weights, int k1, int R,
                                                            int64_t n_simplices, int64_t n_queries,
                                                            const int32_t* __restrict__ q_simplex,
                                                            const int32_t* __restrict__ q_row,
                                                            const uint32_t* __restrict__ q_word,
                                                            int64_t* __restrict__ out_point,
                                                            int32_t* __restrict__ not_found,
                                                            const float* __restrict__ w_sorted,
                                                            const float* __restrict__ node_w) {
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
    const uint32_t target = q_word[q];
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
      if (idx < lv.count[lvl]) {
        float lo[DP], hi[DP];
        const float* nb = nodes + (lv.off[lvl] + idx) * 2 * DP;
        load_row<DP>(nb, lo);
        load_row<DP>(nb + DP, hi);
        const float nw = node_w[lv.off[lvl] + idx];   // the smallest weight below the node
        ok = __builtin_fmaf(nw, nw, box_gap2<DIM>(p, lo, hi)) * SAFE <= tf;
      }
      unsigned long long mask = __ballot(ok);
      __builtin_amdgcn_wave_barrier();   // (every lane has read the popped entry before a push may overwrite it)
      if (lvl == 0) {
        while (mask) {
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
          if (lf >= 0 && rw < n_pts) {   // (rows of the padded last leaf are never candidates)
            float x[DP];
            load_row<DP>(pts + rw * DP, x);
            const float w = w_sorted[rw];
            const float word = __builtin_fmaf(w, w, dist2<DIM>(p, x));   // the word of sweep_power_kernel
            if (__float_as_uint(word) == target) {
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
struct WitnessPowerOp {
  static int run(const flooder_witness_search_t& a, const float* w_sorted, const float* node_w, const Levels& lv,
                 hipStream_t st) {
    if constexpr (DIM < 2) {
      return fail(FLOODER_E_ARG, "flooder_witness_power: dim must be in 2..8");
    } else {
      hipLaunchKernelGGL(witness_power_kernel<DIM>, stack_walk_grid(a.n_queries), dim3(64 * WAVES_PER_BLOCK), 0, st,
                         a.pts_sorted, a.n_pts, a.nodes, lv, a.order, a.verts, a.weights, a.k1, a.R, a.n_simplices,
                         a.n_queries, a.q_simplex, a.q_row, a.q_d2, a.out_point, a.not_found, w_sorted, node_w);
      return check_launch("witness_power");
    }
  }
};

}  // namespace

extern "C" int flooder_node_min_f32(const float* leaf_vals, int64_t n_pts, float* node_min, void* stream) {
  if (!leaf_vals || !node_min || n_pts < 1)
    return fail(FLOODER_E_ARG, "flooder_node_min_f32: bad argument (null pointer, n_pts < 1)");
  const Levels lv = make_levels(n_pts);
  hipStream_t st = (hipStream_t)stream;
  for (int l = 0; l < lv.n_levels; ++l) {
    const int64_t padded = (lv.count[l] + FAN - 1) / FAN * FAN;
    float* out = node_min + lv.off[l];
    if (l == 0)
      hipLaunchKernelGGL(node_min_leaf_kernel, dim3((unsigned)((padded + 255) / 256)), dim3(256), 0, st, leaf_vals,
                         lv.count[0], padded, out);
    else
      hipLaunchKernelGGL(node_min_inner_kernel, dim3((unsigned)((padded + 3) / 4)), dim3(256), 0, st,
                         node_min + lv.off[l - 1], lv.count[l], padded, out);
  }
  return check_launch("node_min");
}

extern "C" int flooder_sweep_power_f32(const flooder_knn_sorted_t* p, const float* w_sorted, const float* node_w,
                                       void* stream) {
  static const char* who = "flooder_sweep_power_f32";
  flooder_knn_sorted_t a;
  if (int rc = take(p, a, "flooder_sweep_power_f32: bad parameter block (abi / size)")) return rc;
  if (int rc = knn_check_ranges(who, a.k, 1, a.dim, a.stat, a.n_pts, false, false)) return rc;
  if (a.stat != 0 || a.reserved != 0) return failf(FLOODER_E_ARG, "%s: stat and reserved must be 0", who);
  if (a.n_simplices == 0 || a.R == 0) return FLOODER_OK;
  if (!a.pts_sorted || !a.nodes || !a.verts || !a.weights || !a.queue || !a.out_bits || !w_sorted || !node_w ||
      a.n_pts < 1 || a.k1 < 1 || a.k1 > FLOODER_MAX_VERTS || a.R < 0 || a.n_simplices < 0)
    return failf(FLOODER_E_ARG, "%s: bad argument (null pointer, no points, k1, R)", who);
  if (a.n_simplices > 0xfffffffeLL || a.n_simplices * (int64_t)a.R > 0xfffffffdLL)   // (ids are 32-bit words)
    return failf(FLOODER_E_ARG, "%s: n_simplices * R must be below 2^32 - 2", who);
  return dispatch_dim<PowerLaunch>(a.dim, a, w_sorted, node_w, make_levels(a.n_pts), (hipStream_t)stream);
}

extern "C" int flooder_node_min_cols_f32(const float* leaf_vals, int64_t n_pts, int nc, float* node_min, void* stream) {
  if (!leaf_vals || !node_min || n_pts < 1 || nc < 1 || nc > FLOODER_POWER_COLS_MAX)
    return fail(FLOODER_E_ARG, "flooder_node_min_cols_f32: bad argument (null pointer, n_pts < 1, nc outside 1..8)");
  const Levels lv = make_levels(n_pts);
  hipStream_t st = (hipStream_t)stream;
  for (int l = 0; l < lv.n_levels; ++l) {
    const int64_t padded = (lv.count[l] + FAN - 1) / FAN * FAN;
    float* out = node_min + lv.off[l] * nc;
    if (l == 0)
      hipLaunchKernelGGL(node_min_cols_leaf_kernel, dim3((unsigned)((padded * nc + 255) / 256)), dim3(256), 0, st,
                         leaf_vals, lv.count[0], padded, nc, out);
    else
      hipLaunchKernelGGL(node_min_cols_inner_kernel, dim3((unsigned)((padded * nc + 3) / 4)), dim3(256), 0, st,
                         node_min + lv.off[l - 1] * nc, lv.count[l], padded, nc, out);
  }
  return check_launch("node_min_cols");
}

extern "C" int flooder_sweep_power_profile_f32(const flooder_knn_sorted_t* p, int n_cols, const float* w_cols,
                                               const float* node_w_cols, void* stream) {
  static const char* who = "flooder_sweep_power_profile_f32";
  flooder_knn_sorted_t a;
  if (int rc = take(p, a, "flooder_sweep_power_profile_f32: bad parameter block (abi / size)")) return rc;
  if (n_cols < 1 || n_cols > FLOODER_POWER_COLS_MAX)
    return failf(FLOODER_E_ARG, "%s: n_cols must be in 1..%d", who, FLOODER_POWER_COLS_MAX);
  if (int rc = knn_check_ranges(who, a.k, 1, a.dim, a.stat, a.n_pts, false, false)) return rc;
  if (a.stat != 0 || a.reserved != 0) return failf(FLOODER_E_ARG, "%s: stat and reserved must be 0", who);
  if (a.n_simplices == 0 || a.R == 0) return FLOODER_OK;
  if (!a.pts_sorted || !a.nodes || !a.verts || !a.weights || !a.queue || !a.out_bits || !w_cols || !node_w_cols ||
      a.n_pts < 1 || a.k1 < 1 || a.k1 > FLOODER_MAX_VERTS || a.R < 0 || a.n_simplices < 0)
    return failf(FLOODER_E_ARG, "%s: bad argument (null pointer, no points, k1, R)", who);
  if (a.n_simplices > 0xfffffffeLL || a.n_simplices * (int64_t)a.R > 0xfffffffdLL)   // (ids are 32-bit words)
    return failf(FLOODER_E_ARG, "%s: n_simplices * R must be below 2^32 - 2", who);
  return dispatch_dim<PowerProfileLaunch>(a.dim, a, n_cols, w_cols, node_w_cols, make_levels(a.n_pts),
                                          (hipStream_t)stream);
}

extern "C" int flooder_witness_power(const flooder_witness_search_t* p, const float* w_sorted, const float* node_w,
                                     void* stream) {
  flooder_witness_search_t a;
  if (int rc = take(p, a, "flooder_witness_power: bad parameter block (abi / size)")) return rc;
  if (a.n_queries == 0) return FLOODER_OK;
  if (!a.pts_sorted || !a.nodes || !a.order || !a.verts || !a.weights || !a.q_simplex || !a.q_row || !a.q_d2 ||
      !a.out_point || !a.not_found || !w_sorted || !node_w || a.n_pts < 1 || a.k1 < 1 || a.R < 1 || a.n_queries < 0 ||
      a.dim < 2 || a.dim > 8 || a.n_pts > 0x7fffffffLL)
    return fail(FLOODER_E_ARG, "flooder_witness_power: bad argument");
  Levels lv;
  if (int rc = stack_walk_levels("flooder_witness_power", a.n_pts, lv)) return rc;
  return dispatch_dim<WitnessPowerOp>(a.dim, a, w_sorted, node_w, lv, (hipStream_t)stream);
}
