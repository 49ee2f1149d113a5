// flood_knn.hip - tree sweep that keeps the k nearest points of every sample (gfx950): the robust filtration.
//
// flooder_sweep_knn_f32 writes, per (simplex, sample), the float32 bits of the SQUARED k-distance (the k-th smallest
// squared distance to the cloud, duplicates counted with their multiplicity) or of the squared distance to the
// empirical measure (the mean of the k smallest squared distances) into the (S, R) buffer that flooder_face_max_f32
// reads - the square root and the face maxima stay there.
//
//   sweep_knn<DIM, K>   one wave owns (simplex, tile of 64 samples), one sample per lane, rebuilt in registers as in
//                       sweep_bvh (fma in vertex order) with the same squared distance (t0*t0, then fma(t, t, d2)).
//                       Every lane keeps its k smallest d2 as an ascending list in K registers, K the smallest of
//                       2, 4, 8, 16, 32 that holds k.  The list sits at the END of the K registers and the K - k in
//                       front of it hold -inf: a candidate passes them unchanged, so the insertion is the same
//                       branch-free chain of K (min, max) pairs for every k, and the k-th best is ALWAYS the last
//                       register - no register indexed by a run-time k.  (The k live slots start at +inf.)
//                       Traversal is sweep_bvh's, wave-uniform and nearest-first over the same nodes with the same
//                       lower bounds and the same safety margin; what it culls against is M = the largest k-th best
//                       of the wave (+inf until every lane has seen k points).  The nearest-first order IS a greedy
//                       descent: the first thing a wave does is walk down to the leaf nearest to its tile, so M is
//                       finite after ceil(k / 16) leaves.
//
// Exactness.  The k-th smallest value of a multiset does not depend on the order in which its elements are offered,
// and a point whose d2 is >= the current k-th best can never lower it - so a subtree whose lower bound is >= M, a leaf
// whose box is >= the k-th best of every lane, and a point no lane improves on are skipped without changing any list.
// What is skipped is never among the k smallest of a lane unless it TIES the k-th, and a tie leaves every one of the k
// values as it is.  The lists at the end are therefore the k smallest d2 of ALL points, value for value, whatever the
// tree looks like; the mean adds them in ascending order, smallest first, in float32, and divides by (float)k with the
// correctly rounded division - a function of those k values alone.
//
// flooder_sweep_knn_profile_f32 is the same sweep at k_max = the largest k of a list of (k, stat) columns with another
// epilogue (PROFILE): the first t live registers of a lane ARE its t smallest d2, and the running ascending sum
// over them is the sum the single sweep forms at k = t, so one walk of the K slots stores the word of every listed
// column into that column's (S, R) plane - the words flooder_sweep_knn_f32 writes for that (k, stat), bit for bit.
// One kernel body serves both; the epilogue is selected at compile time.
//
// flooder_sweep_knn_sorted_f32 is the same sweep over SORTED TILES (SORTED): a wave takes 64 consecutive entries of
// `sample_order` - the samples of ALL simplices along the curve order of flood_sorted.hip, neighbours in space whatever
// simplex they belong to - instead of the samples of one simplex, and stores each word to its own cell (scattered
// 4-byte stores, every cell written once).  Only where a wave gets its 64 samples and where it stores them differs: the
// walk, the lists and the epilogue are the lines below for every form.  The exactness argument above does not mention
// which samples share a wave, so the words are those of flooder_sweep_knn_f32; the order is a performance input only.
// With k1 = 1, R = 1 and weights = [[1.0]] a "simplex" is a query point (fma(1.0f, v, 0.0f) is v): the form that
// flooder_amd.neighbor_distance runs.
//
// flooder_knn_ids_sorted_f32 is the sweep over sorted tiles keeping (d2 word, original id) KEYS per lane: which points
// the k nearest are (flooder_amd.nearest_neighbors, the backward of neighbor_distance).  Ties decide there, so its culls
// are strict and its kernel is a sibling (sweep_knn_ids_kernel below, with its own exactness and termination argument).

#include "flood_common.hpp"
#include "flood_bvh.hpp"

using namespace flooder;

namespace {

struct KnnProfileCols {   // column of (statistic, rank - 1), -1: not asked for (kernarg segment: scalar look-ups)
  int32_t col_of[2][FLOODER_KNN_MAX];
};

// PROFILE = false: flooder_sweep_knn_f32, one word per sample (`stat` of its k values; `cols` is not read).
// PROFILE = true: flooder_sweep_knn_profile_f32, k = the largest k of the columns, out_bits holds a plane per column.
// SORTED = false: an item is (simplex, tile of 64 of its samples; `order` is not read).
// SORTED = true: flooder_sweep_knn_sorted_f32, an item is 64 consecutive entries of `order` (n_simplices * R of them).
template <int DIM, int K, bool PROFILE, bool SORTED>
__global__ __launch_bounds__(256) void sweep_knn_kernel(
    const float* __restrict__ pts, const float* __restrict__ nodes, Levels lv, const float* __restrict__ verts,
    const float* __restrict__ weights, int k1, int R, int64_t n_simplices, int k, int stat,
    int32_t* __restrict__ queue, uint32_t* __restrict__ out_bits, unsigned long long* __restrict__ stats,
    KnnProfileCols cols, const uint32_t* __restrict__ order) {
  constexpr int DP = padded_dim(DIM);
  __shared__ float s_lb[4][MAXL][FAN];
  __shared__ int64_t s_grp[4][MAXL];
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  const int tiles = (R + 63) / 64;
  const int64_t n_samples = n_simplices * (int64_t)R;
  const int64_t n_items = SORTED ? (n_samples + 63) / 64 : n_simplices * tiles;
  const int top = lv.n_levels - 1;
  const int first = K - k;   // the k live slots are list[first .. K-1]  (wave-uniform)
  unsigned long long n_leaf_eval = 0, n_leaf_test = 0, n_node_test = 0, max_item_tests = 0;

  int q_shard = (int)(((int64_t)blockIdx.x * 4 + wv) % QSHARDS), q_tried = 0;
  for (;;) {
    const int64_t g = queue_pop(queue, q_shard, q_tried, n_items, lane);  // sharded heads (flood_common.hpp)
    if (g < 0) break;
    const unsigned long long tests_before = n_leaf_test + n_node_test;
    // ---- this lane's sample (s, r): of the item's simplex, or entry `lane` of the item's run of the sorted order
    int64_t s;
    int r;
    bool live;
    if constexpr (SORTED) {
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
    // (kept as the int32 words of the floats: d2 is never negative and never NaN, so the signed integer order of the
    // words is the order of the values, -inf included, and v_min_i32 / v_max_i32 need no canonicalising copy)
    int list[K];
#pragma unroll
    for (int i = 0; i < K; ++i) list[i] = i >= first ? (int)INF_BITS : (int)0xff800000u;

    // ---- bounding box of the tile (wave-uniform)
    float tlo[DIM], thi[DIM];
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      tlo[c] = wave_min_f32(p[c]);
      thi[c] = wave_max_f32(p[c]);
    }
    float M = __builtin_inff();  // largest k-th best of the tile (wave-uniform)

    // child `lane` of group `grp` at level `lvl`: its box (registers) and the lower bound to the tile box
    float c_lo[DIM], c_hi[DIM];
    auto child_bounds = [&](int lvl, int64_t grp) -> float {
      return child_box_bound<DIM>(nodes, lv, lvl, grp, lane, tlo, thi, c_lo, c_hi);
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
        if (!(mn * SAFE < M)) {  // nothing left at this level can lower a k-th best of the tile
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
      // can the k-th best of any lane still drop against leaf c?  (its box comes from lane j)
      float lbp = 0.f;  // (readlane_row + box_gap2 of flood_bvh.hpp, axis by axis: a call cost K = 32 0.4 % of its time; keep in step)
#pragma unroll
      for (int a = 0; a < DIM; ++a) {
        const float blo = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c_lo[a]), j));
        const float bhi = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c_hi[a]), j));
        const float gap = __builtin_fmaxf(__builtin_fmaxf(blo - p[a], p[a] - bhi), 0.f);
        lbp = __builtin_fmaf(gap, gap, lbp);
      }
      if (__ballot(lbp * SAFE < __int_as_float(list[K - 1])) == 0ull) continue;
      ++n_leaf_eval;
      const float* cp = pts + c * (int64_t)LEAF * DP;
      constexpr int NB = DP == 8 ? 4 : 8;   // rows in SGPRs at a time (32 scalar registers at most)
#pragma unroll 1
      for (int h = 0; h < LEAF; h += NB) {   // (not unrolled: the body holds NB insertion chains)
        typename RowVec<DP>::type cc[NB];
#pragma unroll
        for (int u = 0; u < NB; ++u) cc[u] = load_uniform_row<DP>(cp + (h + u) * DP);
#pragma unroll
        for (int u = 0; u < NB; ++u) {
          float d;  // (dist2 of flood_bvh.hpp written out, as above)
#pragma unroll
          for (int a = 0; a < DIM; ++a) {
            const float t = p[a] - cc[u][a];
            d = a == 0 ? t * t : __builtin_fmaf(t, t, d);
          }
          // the chain only when some lane improves (wave vote); a lane that does not passes d through its list
          // unchanged anyway: every slot is <= its k-th best <= d
          int di = __float_as_int(d);
          if (__ballot(di < list[K - 1]) != 0ull) {
#pragma unroll
            for (int i = 0; i < K; ++i) {
              const int hi = list[i] > di ? list[i] : di;
              list[i] = list[i] < di ? list[i] : di;
              di = hi;
            }
          }
        }
      }
      M = wave_max_f32(__int_as_float(list[K - 1]));
    }

    if constexpr (PROFILE) {
      // every listed (k', stat) with k' <= k from the one list: its first t live slots are the t smallest d2, and the
      // running ascending sum after slot i is the sum the other branch forms at k = i - first + 1
      if (live) {
        const int64_t plane = n_simplices * (int64_t)R, cell = s * (int64_t)R + r;
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < K; ++i) {
          if (i >= first) {   // live slot of rank t + 1 (wave-uniform; the register index i is a constant)
            const int t = i - first;
            const float v = __int_as_float(list[i]);
            acc = t == 0 ? v : acc + v;
            const int c_kth = cols.col_of[0][t], c_dtm = cols.col_of[1][t];
            if (c_kth >= 0) out_bits[c_kth * plane + cell] = __float_as_uint(v);
            if (c_dtm >= 0) out_bits[c_dtm * plane + cell] = __float_as_uint(acc / (float)(t + 1));
          }
        }
      }
    } else if (live) {
      float v = __int_as_float(list[K - 1]);
      if (stat != 0) {   // mean of the k smallest: ascending, smallest first, sequential float32 adds
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < K; ++i) {
          if (i == first) acc = __int_as_float(list[i]);
          else if (i > first) acc = acc + __int_as_float(list[i]);
        }
        v = acc / (float)k;
      }
      out_bits[s * (int64_t)R + r] = __float_as_uint(v);
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

// ---------------------------------------------------------------------------------------------- neighbour ids
// flooder_knn_ids_sorted_f32: the sweep over sorted tiles keeping KEYS (d2 word, original id) instead of d2 words - WHICH
// points the k nearest are, under the tie rule of flooder_witness_knn (flood_grad.hip).  A sibling of sweep_knn_kernel,
// not a flag of it: the value sweeps keep their code.  The walk is the one above (keep in step); what differs is listed
// below.  One shared body (a __forceinline__ function with an IDS template flag under two thin kernels, the culls behind
// lambdas or the value path kept token for token under `if constexpr`) was tried at compile level: it moved the
// registers of 138 to 140 of the file's 142 kernel symbols, the value kernels' included (<7, 4, false, false>: 58 -> 72
// VGPRs; the parent's table is profiles/knn_ids_kernel_resources.txt).  Nobody has timed such a build, so the copy stands.
//
//   the list   K (hi, lo) register pairs per lane, hi the d2 word compared as a signed int as above, lo the id compared
//              unsigned.  The K - k front slots hold (-inf, 0), the
//              smallest key there is; the k live slots start at (+inf, 0xffffffff), above every real key - ids are
//              below 2^31, and a real d2 that overflowed to +inf still sorts in front of an empty slot.  No hi word
//              is ever a NaN (d2 of finite inputs is not, and the two fillers are infinities): the culls read
//              list[K-1].hi as a float.
//   the culls  STRICT: a node, a leaf or a point is skipped only when lb * SAFE > bound (a point: key > k-th key).
//   the marks  a visited child and a child past the end of its level hold CLOSED (-1; a bound is never negative), and a
//              level is left when no child is open or the nearest open one is strictly farther than M.  A bound of
//              +inf is a bound like any other: while M is +inf (some lane holds fewer than k points) nothing open is
//              skipped.
//   the ids    order[row] of the NB rows of a step, wave-uniform, fetched beside the rows through the scalar cache.  Rows
//              of the padded last leaf (row >= n_pts) are no candidates and order is not read there (the index is
//              clamped; the row is skipped by a wave-uniform test, whatever its +inf coordinates give).
//
// Exactness.  Keys are distinct (ids are), so "the k smallest keys of all points" is ONE set, and inserting any superset
// of it in any order leaves exactly that set, ascending.  A subtree or a leaf is skipped only when lb * SAFE > the k-th
// d2 of every lane concerned: each of its points then has a strictly larger d2, hence a larger key whatever its id.  A
// box at lb == k-th d2 is opened and a point at d2 == k-th d2 is compared by its id: a smaller id displaces the k-th
// entry.  Nothing is skipped while a lane holds fewer than k points.  The d2 words are those of the value sweep
// (same samples, same arithmetic), so out_bits - the value sweep's epilogue over the k hi words - is its word, bit for bit.
//
// Termination.  Every step of the walk either closes one open child (a mark that no comparison of bounds can undo:
// `inf <= inf` never reopens anything), descends into a child just closed, or leaves a level for good; levels and
// children are finite.  At k == n_pts the lists fill only with the last leaf and M stays +inf until then: the walk visits
// every child once and ends when none is open.
constexpr float CLOSED = -1.f;

__device__ __forceinline__ uint32_t load_uniform_u32(const uint32_t* p) {   // (load_uniform_row, for one word)
  typedef const __attribute__((address_space(4))) uint32_t* cptr_t;
  return *((cptr_t)(uintptr_t)p);
}

// key (ah, al) < key (bh, bl): hi signed, lo unsigned  (three 32-bit comparisons: as one signed 64-bit comparison of
// (hi << 32 | lo) the list wants aligned register pairs, 8 to 30 VGPRs more and a wave per SIMD fewer at K = 8 and 16;
// timed, the two forms are within 5 % of each other, either way, at every k)
__device__ __forceinline__ bool key_less(int ah, uint32_t al, int bh, uint32_t bl) {
  return ah < bh || (ah == bh && al < bl);
}

typedef uint32_t v4u __attribute__((ext_vector_type(4)));

template <int DIM, int K>
__global__ __launch_bounds__(256) void sweep_knn_ids_kernel(
    const float* __restrict__ pts, int64_t n_pts, const float* __restrict__ nodes, Levels lv,
    const float* __restrict__ verts, const float* __restrict__ weights, int k1, int R, int64_t n_simplices, int k,
    int stat, int32_t* __restrict__ queue, const uint32_t* __restrict__ order, const uint32_t* __restrict__ pt_id,
    uint32_t* __restrict__ out_ids, uint32_t* __restrict__ out_d2, uint32_t* __restrict__ out_bits,
    unsigned long long* __restrict__ stats) {
  constexpr int DP = padded_dim(DIM);
  __shared__ float s_lb[4][MAXL][FAN];
  __shared__ int64_t s_grp[4][MAXL];
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  const int64_t n_samples = n_simplices * (int64_t)R;
  const int64_t n_items = (n_samples + 63) / 64;
  const int top = lv.n_levels - 1;
  const int first = K - k;   // the k live slots are list[first .. K-1]  (wave-uniform)
  unsigned long long n_leaf_eval = 0, n_leaf_test = 0, n_node_test = 0, max_item_tests = 0;

  int q_shard = (int)(((int64_t)blockIdx.x * 4 + wv) % QSHARDS), q_tried = 0;
  for (;;) {
    const int64_t g = queue_pop(queue, q_shard, q_tried, n_items, lane);
    if (g < 0) break;
    const unsigned long long tests_before = n_leaf_test + n_node_test;
    // ---- this lane's sample (s, r): entry `lane` of the item's run of the sorted order
    const int64_t pos = g * 64 + lane;
    const bool live = pos < n_samples;
    const uint32_t sid = order[live ? pos : n_samples - 1];  // duplicate of the last entry, never stored
    const uint32_t si = sid / (uint32_t)R;
    const int64_t s = (int64_t)si;
    const int r = (int)(sid - si * (uint32_t)R);
    float p[DIM];
    const float* vs = verts + s * (int64_t)k1 * DIM;
#pragma unroll
    for (int c = 0; c < DIM; ++c) p[c] = 0.f;
    for (int j = 0; j < k1; ++j) {
      const float w = weights[(int64_t)r * k1 + j];
#pragma unroll
      for (int c = 0; c < DIM; ++c) p[c] = __builtin_fmaf(w, vs[j * DIM + c], p[c]);
    }
    int lh[K];        // d2 words
    uint32_t ll[K];   // original ids
#pragma unroll
    for (int i = 0; i < K; ++i) {
      lh[i] = i >= first ? (int)INF_BITS : (int)0xff800000u;
      ll[i] = i >= first ? 0xffffffffu : 0u;
    }

    // ---- bounding box of the tile (wave-uniform)
    float tlo[DIM], thi[DIM];
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      tlo[c] = wave_min_f32(p[c]);
      thi[c] = wave_max_f32(p[c]);
    }
    float M = __builtin_inff();  // largest k-th d2 of the tile (wave-uniform)

    // child `lane` of group `grp` at level `lvl`: its box (registers) and the lower bound to the tile box, CLOSED past
    // the end of the level
    float c_lo[DIM], c_hi[DIM];
    auto child_bounds = [&](int lvl, int64_t grp) -> float {
      const float lb = child_box_bound<DIM>(nodes, lv, lvl, grp, lane, tlo, thi, c_lo, c_hi);
      return grp * FAN + lane < lv.count[lvl] ? lb : CLOSED;
    };

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
        const bool open = lbv >= 0.f;
        const float mn = wave_min_f32(open ? lbv : __builtin_inff());
        if (__ballot(open) == 0ull || mn * SAFE > M) {  // nothing open, or nothing open that holds a key below a k-th
          if (++lvl > top) break;
          continue;
        }
        const int j = __builtin_ctzll(__ballot(open && lbv == mn));
        if (lane == j) s_lb[wv][lvl][lane] = CLOSED;  // visited
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
      // ---- leaf level: nearest open leaf of the current group
      const bool open = lb0 >= 0.f;
      const float mn = wave_min_f32(open ? lb0 : __builtin_inff());
      if (__ballot(open) == 0ull || mn * SAFE > M) {
        if (++lvl > top) break;
        continue;
      }
      const int j = __builtin_ctzll(__ballot(open && lb0 == mn));
      if (lane == j) lb0 = CLOSED;  // visited
      const int64_t c = grp0 * FAN + j;
      ++n_leaf_test;
      // can leaf c hold a key below the k-th of any lane?  (its box comes from lane j)
      float lbp = 0.f;
#pragma unroll
      for (int a = 0; a < DIM; ++a) {
        const float blo = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c_lo[a]), j));
        const float bhi = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c_hi[a]), j));
        const float gap = __builtin_fmaxf(__builtin_fmaxf(blo - p[a], p[a] - bhi), 0.f);
        lbp = __builtin_fmaf(gap, gap, lbp);
      }
      if (__ballot(!(lbp * SAFE > __int_as_float(lh[K - 1]))) == 0ull) continue;
      ++n_leaf_eval;
      const int64_t row0 = c * (int64_t)LEAF;
      const float* cp = pts + row0 * DP;
      constexpr int NB = DP == 8 ? 4 : 8;   // rows (and their ids) in SGPRs at a time
#pragma unroll 1
      for (int h = 0; h < LEAF; h += NB) {
        if (row0 + h >= n_pts) break;   // the rest of the padded last leaf
        typename RowVec<DP>::type cc[NB];
        uint32_t id[NB];
#pragma unroll
        for (int u = 0; u < NB; ++u) {
          cc[u] = load_uniform_row<DP>(cp + (h + u) * DP);
          const int64_t rw = row0 + h + u;
          id[u] = load_uniform_u32(pt_id + (rw < n_pts ? rw : n_pts - 1));
        }
#pragma unroll
        for (int u = 0; u < NB; ++u) {
          if (row0 + h + u < n_pts) {   // (wave-uniform)
            float d;
#pragma unroll
            for (int a = 0; a < DIM; ++a) {
              const float t = p[a] - cc[u][a];
              d = a == 0 ? t * t : __builtin_fmaf(t, t, d);
            }
            // the chain only when some lane's k-th key is above this one (wave vote); a lane where it is not passes
            // the key through its list unchanged: every slot is below it
            int ch = __float_as_int(d);
            uint32_t cl = id[u];
            if (__ballot(key_less(ch, cl, lh[K - 1], ll[K - 1])) != 0ull) {
#pragma unroll
              for (int i = 0; i < K; ++i) {
                const bool lt = key_less(ch, cl, lh[i], ll[i]);
                const int nh = lt ? lh[i] : ch;
                const uint32_t nl = lt ? ll[i] : cl;
                lh[i] = lt ? ch : lh[i];
                ll[i] = lt ? cl : ll[i];
                ch = nh;
                cl = nl;
              }
            }
          }
        }
      }
      M = wave_max_f32(__int_as_float(lh[K - 1]));
    }

    if (live) {
      const int64_t cell = s * (int64_t)R + r;
      uint32_t* oi = out_ids + cell * k;
      uint32_t* od = out_d2 ? out_d2 + cell * k : nullptr;
      bool wide = false;   // rows of k words, k a multiple of 4, in 16-byte aligned buffers: 16-byte stores
      if constexpr (K >= 4) wide = (k & 3) == 0 && (((uintptr_t)out_ids | (uintptr_t)out_d2) & 15) == 0;
      if (wide) {
        if constexpr (K >= 4) {
#pragma unroll
          for (int i = 0; i < K; i += 4) {
            if (i >= first) {   // (first is a multiple of 4 here; the register indices are constants)
              *reinterpret_cast<v4u*>(oi + (i - first)) = v4u{ll[i], ll[i + 1], ll[i + 2], ll[i + 3]};
              if (od)
                *reinterpret_cast<v4u*>(od + (i - first)) =
                    v4u{(uint32_t)lh[i], (uint32_t)lh[i + 1], (uint32_t)lh[i + 2], (uint32_t)lh[i + 3]};
            }
          }
        }
      } else {
#pragma unroll
        for (int i = 0; i < K; ++i) {
          if (i >= first) {
            oi[i - first] = ll[i];
            if (od) od[i - first] = (uint32_t)lh[i];
          }
        }
      }
      if (out_bits) {   // the epilogue of sweep_knn_kernel over the hi words
        float v = __int_as_float(lh[K - 1]);
        if (stat != 0) {
          float acc = 0.f;
#pragma unroll
          for (int i = 0; i < K; ++i) {
            if (i == first) acc = __int_as_float(lh[i]);
            else if (i > first) acc = acc + __int_as_float(lh[i]);
          }
          v = acc / (float)k;
        }
        out_bits[cell] = __float_as_uint(v);
      }
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

// ---- host side: one block, one set of checks, one launch.
// flooder_knn_sweep_t is a prefix of flooder_knn_sorted_t and that one of flooder_knn_ids_t - same names, types and
// offsets, stated below.  Every entry takes ITS block by its own size rule and lays it over a zeroed flooder_knn_ids_t:
// the fields its block does not have read as NULL, as `take` reads the tail of a short block.  knn_sweep<FORM> makes the
// checks of the form in the entry's order and holds the launch.
#define FLOODER_KNN_SWEEP_FIELDS(X)                                                                                  \
  X(size) X(abi) X(pts_sorted) X(n_pts) X(dim) X(k1) X(nodes) X(verts) X(weights) X(R) X(k) X(n_simplices) X(stat) \
  X(reserved) X(queue) X(out_bits) X(stats)
template <typename Short, typename Long>
constexpr bool knn_sweep_fields_match() {
#define X(f) && offsetof(Short, f) == offsetof(Long, f) && std::is_same<decltype(Short::f), decltype(Long::f)>::value
  return true FLOODER_KNN_SWEEP_FIELDS(X);
#undef X
}
static_assert(knn_sweep_fields_match<flooder_knn_sweep_t, flooder_knn_sorted_t>() &&
                  sizeof(flooder_knn_sweep_t) == offsetof(flooder_knn_sorted_t, sample_order),
              "flooder_knn_sweep_t must be a prefix of flooder_knn_sorted_t");
static_assert(knn_sweep_fields_match<flooder_knn_sorted_t, flooder_knn_ids_t>() &&
                  offsetof(flooder_knn_sorted_t, sample_order) == offsetof(flooder_knn_ids_t, sample_order) &&
                  sizeof(flooder_knn_sorted_t) == offsetof(flooder_knn_ids_t, order),
              "flooder_knn_sorted_t must be a prefix of flooder_knn_ids_t");

template <typename Block>
flooder_knn_ids_t widened(const Block& a) {
  flooder_knn_ids_t w;
  memset(&w, 0, sizeof(w));
  memcpy(&w, &a, sizeof(a));
  return w;
}

// per-simplex tiles / tiles of the sorted order / sorted tiles keeping ids / per-simplex tiles, a plane per column
enum class KnnForm { simplex, sorted, ids, profile };

// The launch at K = the smallest of 2, 4, 8, 16, 32 that holds k: sweep_knn_ids_kernel for the ids form, else
// sweep_knn_kernel<DIM, K, PROFILE, SORTED>.  (the tree sweeps exist for one ambient dimension as well; the k-nearest
// sweep is defined for 2 .. 8 and knn_sweep has refused the rest)
template <KnnForm FORM>
struct KnnLaunch {
  template <int DIM>
  struct Op {
    static int run(const flooder_knn_ids_t& a, const KnnProfileCols& cols, const Levels& lv, const char* what,
                   hipStream_t st) {
      if constexpr (DIM < 2) {
        return fail(FLOODER_E_ARG, "dim must be in 2..8");
      } else {
        constexpr bool SORTED = FORM == KnnForm::sorted || FORM == KnnForm::ids;
        const int64_t n_items = SORTED ? (a.n_simplices * (int64_t)a.R + 63) / 64 : a.n_simplices * ((a.R + 63) / 64);
        int64_t grid = g_bvh_grid;  // persistent blocks; 4 independent waves each
        if (grid > (n_items + 3) / 4) grid = (n_items + 3) / 4;
        auto* stats = reinterpret_cast<unsigned long long*>(a.stats);
        auto* order = reinterpret_cast<const uint32_t*>(a.sample_order);
        with_knn_slots(a.k, [&](auto kc) {
          constexpr int K = decltype(kc)::value;
          if constexpr (FORM == KnnForm::ids)
            hipLaunchKernelGGL((sweep_knn_ids_kernel<DIM, K>), dim3((unsigned)grid), dim3(256), 0, st, a.pts_sorted,
                               a.n_pts, a.nodes, lv, a.verts, a.weights, a.k1, a.R, a.n_simplices, a.k, a.stat, a.queue,
                               order, reinterpret_cast<const uint32_t*>(a.order), reinterpret_cast<uint32_t*>(a.out_ids),
                               a.out_d2, a.out_bits, stats);
          else
            hipLaunchKernelGGL((sweep_knn_kernel<DIM, K, FORM == KnnForm::profile, SORTED>), dim3((unsigned)grid),
                               dim3(256), 0, st, a.pts_sorted, a.nodes, lv, a.verts, a.weights, a.k1, a.R, a.n_simplices,
                               a.k, a.stat, a.queue, a.out_bits, stats, cols, order);
        });
        return check_launch(what);
      }
    }
  };
};

// `who`: the entry's name, in front of every message; `what`: the launch's name for check_launch.  The profile form comes
// with k = the largest k of its columns and stat 0 (both in range by construction).
template <KnnForm FORM>
int knn_sweep(const flooder_knn_ids_t& a, const KnnProfileCols& cols, const char* who, const char* what, void* stream) {
  constexpr bool IDS = FORM == KnnForm::ids, PROFILE = FORM == KnnForm::profile;
  if (int rc = knn_check_ranges(who, a.k, FLOODER_KNN_MAX, a.dim, a.stat, a.n_pts, false, IDS)) return rc;
  if (PROFILE && a.n_pts < a.k) return failf(FLOODER_E_ARG, "%s: fewer points than the largest k", who);
  if (a.n_simplices == 0 || a.R == 0) return FLOODER_OK;
  if (!a.pts_sorted || !a.nodes || !a.verts || !a.weights || !a.queue || (!a.out_bits && !IDS) || a.n_pts < a.k ||
      a.k1 < 1 || a.k1 > FLOODER_MAX_VERTS || a.R < 0 || a.n_simplices < 0)
    return failf(FLOODER_E_ARG, PROFILE ? "%s: bad argument (null pointer, k1, R)"
                                        : "%s: bad argument (null pointer, fewer points than k, k1, R)", who);
  if constexpr (FORM == KnnForm::sorted || IDS) {
    if (!a.sample_order) return failf(FLOODER_E_ARG, "%s: sample_order is NULL", who);
    if (IDS && !a.order) return failf(FLOODER_E_ARG, "%s: order is NULL", who);
    if (IDS && !a.out_ids) return failf(FLOODER_E_ARG, "%s: out_ids is NULL", who);
    if (a.n_simplices > 0xfffffffeLL || a.n_simplices * (int64_t)a.R > 0xfffffffdLL)   // (ids are 32-bit words)
      return failf(FLOODER_E_ARG, "%s: n_simplices * R must be below 2^32 - 2", who);
  }
  return dispatch_dim<KnnLaunch<FORM>::template Op>(a.dim, a, cols, make_levels(a.n_pts), what, (hipStream_t)stream);
}

}  // namespace

extern "C" int flooder_sweep_knn_f32(const flooder_knn_sweep_t* p, void* stream) {
  flooder_knn_sweep_t a;
  if (int rc = take(p, a, "flooder_sweep_knn_f32: bad parameter block (abi / size)")) return rc;
  return knn_sweep<KnnForm::simplex>(widened(a), KnnProfileCols{}, "flooder_sweep_knn_f32", "sweep_knn", stream);
}

extern "C" int flooder_sweep_knn_sorted_f32(const flooder_knn_sorted_t* p, void* stream) {
  flooder_knn_sorted_t a;
  if (int rc = take(p, a, "flooder_sweep_knn_sorted_f32: bad parameter block (abi / size)")) return rc;
  return knn_sweep<KnnForm::sorted>(widened(a), KnnProfileCols{}, "flooder_sweep_knn_sorted_f32", "sweep_knn_sorted",
                                    stream);
}

extern "C" int flooder_knn_ids_sorted_f32(const flooder_knn_ids_t* p, void* stream) {
  flooder_knn_ids_t a;
  if (int rc = take(p, a, "flooder_knn_ids_sorted_f32: bad parameter block (abi / size)")) return rc;
  return knn_sweep<KnnForm::ids>(a, KnnProfileCols{}, "flooder_knn_ids_sorted_f32", "knn_ids_sorted", stream);
}

extern "C" int flooder_sweep_knn_profile_f32(const flooder_knn_profile_t* p, void* stream) {
  flooder_knn_profile_t a;
  if (int rc = take(p, a, "flooder_sweep_knn_profile_f32: bad parameter block (abi / size)")) return rc;
  if (a.n_cols < 1 || a.n_cols > FLOODER_KNN_COLS_MAX)
    return fail(FLOODER_E_ARG, "flooder_sweep_knn_profile_f32: n_cols must be in 1..64");
  KnnProfileCols cols;
  for (int s = 0; s < 2; ++s)
    for (int t = 0; t < FLOODER_KNN_MAX; ++t) cols.col_of[s][t] = -1;
  flooder_knn_ids_t w;   // the sweep at k = the largest k of the columns
  memset(&w, 0, sizeof(w));
  for (int c = 0; c < a.n_cols; ++c) {
    const int k = a.col_k[c], s = a.col_stat[c];
    if (k < 1 || k > FLOODER_KNN_MAX) return fail(FLOODER_E_ARG, "flooder_sweep_knn_profile_f32: col_k must be in 1..32");
    if (s != 0 && s != 1)
      return fail(FLOODER_E_ARG, "flooder_sweep_knn_profile_f32: col_stat must be 0 (kth) or 1 (dtm)");
    if (cols.col_of[s][k - 1] >= 0)
      return fail(FLOODER_E_ARG, "flooder_sweep_knn_profile_f32: a (k, stat) column is listed twice");
    cols.col_of[s][k - 1] = c;
    if (k > w.k) w.k = k;
  }
  w.pts_sorted = a.pts_sorted, w.n_pts = a.n_pts, w.dim = a.dim, w.k1 = a.k1, w.nodes = a.nodes, w.verts = a.verts;
  w.weights = a.weights, w.R = a.R, w.n_simplices = a.n_simplices, w.queue = a.queue, w.out_bits = a.out_bits;
  w.stats = a.stats;
  return knn_sweep<KnnForm::profile>(w, cols, "flooder_sweep_knn_profile_f32", "sweep_knn_profile", stream);
}
