// flood_knn_wide.hip - the k nearest points of every sample for k up to FLOODER_KNN_WIDE_MAX = 1024, one wave per cell
// (gfx950): the robust filtration by MASS (flood_complex(neighbor_mass=m), flooder_amd.distance_to_measure).
//
// The k-nearest family of flood_knn.hip keeps a lane's k best in registers and stops at k = 32.  Here a WAVE owns one
// cell g = s * R + r and keeps the k smallest keys (d2 word << 32 | original id) seen so far, sorted ascending, in LDS:
// position i of the list sits in slot i / 64 of lane i % 64, i.e. at word i - consecutive lanes read consecutive 8-byte
// words.  One instantiation per list capacity 64, 128, 256, 512, 1024 (SLOTS = 1, 2, 4, 8, 16), so that k = 40 does
// not pay for 1024.  It is the wave-per-query form of witness_knn_kernel (flood_grad.hip) with a batched insertion.
//
// Traversal: witness_knn_kernel's.  A per-wave stack of (level, group of 64 siblings); a popped group's children are
// tested one per lane, the nearest qualifying child is pushed LAST (so a query first walks down to the leaf group
// nearest to it), leaves are evaluated four at a time, one point per lane, and the leaves still waiting are tested
// again whenever the k-th key has changed.
//
// Insertion: every lane compares its candidate key with the wave-uniform k-th key of the list; the survivors are
// compacted (ballot + popcount) into a per-wave buffer of BUF = 128 keys.  The buffer is merged into the list
//   - before a batch of four leaves when fewer than 64 places are free,
//   - after a leaf group when it holds at least min(k, 64) keys (small k: the k-th key tightens early),
//   - at the end of the walk.
// A merge ranks the buffer's keys among themselves by counting (the keys are distinct), writes them back sorted, and
// gives every key its place in the merged sequence: a buffer key goes to (rank in the buffer) + (list keys below it: a
// binary search of the list), a list key at i to i + (buffer keys below it: a binary search of the sorted buffer).
// Places >= k fall off; the k-th key is re-read.  The list starts as k all-ones keys, which sort behind every real key
// (ids are < 2^31), so until k real keys are in, the k-th key is all ones and every candidate passes.
//
// Exactness.  Keys are distinct (ids are; a point is evaluated at most once per cell, every leaf being opened at most
// once), so "the k smallest keys of all points" is one set.  A candidate is dropped only when its key is not below
// the CURRENT k-th key, which is never below the final one; a subtree or leaf is skipped only when lb * SAFE > the
// current k-th d2, so every point in it has a larger d2 and hence a larger key whatever its id (a box AT the k-th d2 is
// opened: an equal d2 with a smaller id displaces the k-th entry).  The buffer only DELAYS insertions: the k-th key it
// delays is larger than the true one, which culls less, never more.  With k == n_pts the k-th key stays all ones until
// the last point is in: nothing is culled and the walk ends because the stack empties.
//
// No atomics, nothing in inline assembly of its own; every output word is written once by plain vector stores.  The
// rule of the statistic (the strided sum of stat 1) is stated with the entry in include/flooder_hip.h.
//
// Profile (flooder_knn_wide_profile_f32; distance_to_measure_profile).  The list a wave ends a cell with holds the k
// smallest keys ascending, so its first k' entries are the k' smallest keys and wide_statistic over them is the word of
// the single call at (k', stat'): the epilogue - and nothing else - is a compile-time variant (COLS) that writes one
// word per listed column, planes plane_stride words apart.  The walk culls against the k-th key of the LARGEST k.

#include "../../include/flooder_hip.h"
#include "flood_knn_list.hpp"

using namespace flooder;

namespace {

// The columns of the epilogue, a compile-time variant of the ONE kernel: NoCols (flooder_knn_wide_f32) writes the word
// of (k, stat) to out_bits[g]; WideCols (flooder_knn_wide_profile_f32) a word per listed (k', stat') with k' <= k to
// out_bits[c * plane_stride + g].  The walk, the insertion and the id / d2 rows do not know which it is.
struct NoCols {};
struct WideCols {
  int64_t plane_stride;
  int n_cols;
  int col_k[FLOODER_KNN_COLS_MAX];
  int col_stat[FLOODER_KNN_COLS_MAX];
};

// The squared statistic of the first kk keys of the ascending list (wave-uniform kk, stat; the same value in every lane)
__device__ __forceinline__ float wide_statistic(const wkey_t* list, int kk, int stat, int lane) {
  if (stat == 0) return __uint_as_float((uint32_t)(list[kk - 1] >> 32));
  // S_l = w_l + w_(l+64) + w_(l+128) + ... (positions < kk), then S_0 + S_1 + ... + S_(min(kk,64)-1): both sequential
  // float32 sums in that order; for kk <= 64 the plain ascending sequential sum of the value sweeps
  float part = 0.f;
  if (lane < kk) {
    part = __uint_as_float((uint32_t)(list[lane] >> 32));
    for (int i = lane + 64; i < kk; i += 64) part = part + __uint_as_float((uint32_t)(list[i] >> 32));
  }
  const int L = kk < 64 ? kk : 64;   // the lanes that hold a partial sum
  float acc = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(part), 0));
  for (int l = 1; l < L; ++l)
    acc = acc + __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(part), l));
  return acc / (float)kk;
}

template <int DIM, int SLOTS, class COLS>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void knn_wide_kernel(
    const float* __restrict__ pts, int64_t n_pts, const float* __restrict__ nodes, Levels lv,
    const int32_t* __restrict__ order, const float* __restrict__ verts, const float* __restrict__ weights, int k1, int R,
    int64_t n_cells, int k, int stat, const int32_t* __restrict__ sample_order, uint32_t* __restrict__ out_bits,
    int32_t* __restrict__ out_ids, uint32_t* __restrict__ out_d2, const COLS cols) {
  constexpr int DP = padded_dim(DIM);
  constexpr int CAP = 64 * SLOTS;
  __shared__ wkey_t s_list[WAVES_PER_BLOCK][CAP];
  __shared__ wkey_t s_buf[WAVES_PER_BLOCK][BUF];
  __shared__ int32_t s_stack[WAVES_PER_BLOCK][STACK];
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  wkey_t* list = s_list[wv];
  wkey_t* buf = s_buf[wv];
  const int64_t wave = (int64_t)blockIdx.x * WAVES_PER_BLOCK + wv;
  const int64_t n_waves = (int64_t)gridDim.x * WAVES_PER_BLOCK;
  const unsigned long long below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  const int top = lv.n_levels - 1;
  const int merge_at = k < 64 ? k : 64;
  for (int64_t t = wave; t < n_cells; t += n_waves) {
    const int64_t g = sample_order ? (int64_t)(uint32_t)sample_order[t] : t;
    if (g >= n_cells) continue;   // (not a cell: the caller's order is out of bounds there, nothing is written)
    const int64_t s = g / R;
    const int r = (int)(g - s * R);
    // the sample exactly as the sweeps build it: p = 0; p[c] = fma(w_j, v_j[c], p[c]) in vertex order
    float p[DIM];
#pragma unroll
    for (int c = 0; c < DIM; ++c) p[c] = 0.f;
    const float* vs = verts + s * (int64_t)k1 * DIM;
    for (int j = 0; j < k1; ++j) {
      const float w = weights[(int64_t)r * k1 + j];
#pragma unroll
      for (int c = 0; c < DIM; ++c) p[c] = __builtin_fmaf(w, vs[j * DIM + c], p[c]);
    }
    for (int i = lane; i < k; i += 64) list[i] = NOKEY;
    wkey_t kth = NOKEY;   // the list's k-th key (wave-uniform)
    float kth_f = __builtin_inff();
    int cnt = 0;         // keys waiting in the buffer (wave-uniform)
    int sp = 1;
    if (lane == 0) s_stack[wv][0] = top;   // (level top, group 0): the <= 64 top nodes
    lds_handoff();
    while (sp > 0) {
      --sp;
      const int e = s_stack[wv][sp];
      const int lvl = e & 7;
      const int64_t grp = e >> 3;
      const int64_t idx = grp * FAN + lane;
      bool ok = false;
      float lb = __builtin_inff();
      if (idx < lv.count[lvl]) {   // (child_point_bound of flood_bvh.hpp, its load written out as in witness_knn_kernel)
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
          if (cnt > BUF - 64) {   // fewer than 64 free places: merge, and test the waiting leaves against the new k-th
            merge_buffer<SLOTS>(list, buf, k, cnt, lane);
            cnt = 0;
            kth = list[k - 1];
            kth_f = kth == NOKEY ? __builtin_inff() : __uint_as_float((uint32_t)(kth >> 32));
            mask &= __ballot(!(lb * SAFE > kth_f));
            if (!mask) break;
          }
          // the next four leaves, one point per lane (the steps of witness_knn_kernel)
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
          wkey_t c = NOKEY;   // this lane's candidate key
          if (lf >= 0 && rw < n_pts) {   // (rows of the padded last leaf are never candidates)
            float x[DP];
            load_row<DP>(pts + rw * DP, x);
            const float d2 = dist2<DIM>(p, x);
            c = ((wkey_t)__float_as_uint(d2) << 32) | (wkey_t)(uint32_t)(order ? order[rw] : (int32_t)rw);
          }
          const bool in = c < kth;
          const unsigned long long take_mask = __ballot(in);
          if (in) buf[cnt + __popcll(take_mask & below)] = c;   // (cnt <= BUF - 64 here: at most 64 more)
          cnt += __popcll(take_mask);
        }
        if (cnt >= merge_at) {
          merge_buffer<SLOTS>(list, buf, k, cnt, lane);
          cnt = 0;
          kth = list[k - 1];
          kth_f = kth == NOKEY ? __builtin_inff() : __uint_as_float((uint32_t)(kth >> 32));
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
        lds_handoff();
      }
    }
    if (cnt > 0) merge_buffer<SLOTS>(list, buf, k, cnt, lane);
    lds_handoff();
    // ---- the k keys, ascending: ids, d2 words, and the statistic of the d2 words
    const int64_t row = g * (int64_t)k;
    for (int i = lane; i < k; i += 64) {
      const wkey_t key = list[i];
      if (out_ids) out_ids[row + i] = (int32_t)(uint32_t)key;
      if (out_d2) out_d2[row + i] = (uint32_t)(key >> 32);
    }
    if (out_bits) {
      if constexpr (std::is_same<COLS, NoCols>::value) {
        const float v = wide_statistic(list, k, stat, lane);
        if (lane == 0) out_bits[g] = __float_as_uint(v);
      } else {
        // the first k' keys of the list are the k' smallest: column c is the single call at (col_k[c], col_stat[c])
        for (int c = 0; c < cols.n_cols; ++c) {
          const float v = wide_statistic(list, cols.col_k[c], cols.col_stat[c], lane);
          if (lane == 0) out_bits[(int64_t)c * cols.plane_stride + g] = __float_as_uint(v);
        }
      }
    }
    lds_handoff();   // (every lane has read the list before the next cell resets it)
  }
}

template <int DIM>
struct KnnWideOp {
  template <int SLOTS, class COLS>
  static void launch(const flooder_knn_wide_t& a, const COLS& cols, const Levels& lv, int64_t n_cells, hipStream_t st) {
    hipLaunchKernelGGL((knn_wide_kernel<DIM, SLOTS, COLS>), stack_walk_grid(n_cells), dim3(64 * WAVES_PER_BLOCK), 0, st,
                       a.pts_sorted, a.n_pts, a.nodes, lv, a.order, a.verts, a.weights, a.k1, a.R, n_cells, a.k, a.stat,
                       a.sample_order, a.out_bits, a.out_ids, a.out_d2, cols);
  }
  template <class COLS>
  static int run(const flooder_knn_wide_t& a, const COLS& cols, const Levels& lv, int64_t n_cells, hipStream_t st) {
    if constexpr (DIM < 2) {
      return fail(FLOODER_E_ARG, "flooder_knn_wide_f32: dim must be in 2..8");
    } else {
      with_list_slots(a.k, [&](auto slots) { launch<decltype(slots)::value>(a, cols, lv, n_cells, st); });
      return check_launch("knn_wide");
    }
  }
};

// The checks of both entries (the profile entry has made its column checks already) and the launch
template <class COLS>
int knn_wide(const char* who, const flooder_knn_wide_t& a, const COLS& cols, int64_t plane_stride, void* stream) {
  if (int rc = knn_check_ranges(who, a.k, FLOODER_KNN_WIDE_MAX, a.dim, a.stat, a.n_pts, true, true)) return rc;
  if (a.n_simplices > 0 && a.R > 0 && a.n_simplices > ((1LL << 32) - 3) / a.R)
    return failf(FLOODER_E_ARG, "%s: n_simplices * R must be below 2^32 - 2", who);
  Levels lv;
  if (int rc = stack_walk_levels(who, a.n_pts, lv)) return rc;
  if (!a.out_bits && !a.out_ids && !a.out_d2)
    return failf(FLOODER_E_ARG, "%s: no output (out_bits, out_ids and out_d2 are all NULL)", who);
  if (a.out_ids && !a.order) return failf(FLOODER_E_ARG, "%s: out_ids needs order (tree row -> original id)", who);
  if (!std::is_same<COLS, NoCols>::value && a.n_simplices > 0 && a.R > 0 && plane_stride < a.n_simplices * (int64_t)a.R)
    return failf(FLOODER_E_ARG, "%s: plane_stride must be at least n_simplices * R", who);
  if (a.n_simplices == 0 || a.R == 0) return FLOODER_OK;
  if (!a.pts_sorted || !a.nodes || !a.verts || !a.weights || a.k1 < 1 || a.R < 0 || a.n_simplices < 0)
    return failf(FLOODER_E_ARG, "%s: bad argument (null pointer, k1, R, n_simplices)", who);
  return dispatch_dim<KnnWideOp>(a.dim, a, cols, lv, a.n_simplices * (int64_t)a.R, (hipStream_t)stream);
}

}  // namespace

extern "C" int flooder_knn_wide_f32(const flooder_knn_wide_t* p, void* stream) {
  flooder_knn_wide_t a;
  if (int rc = take(p, a, "flooder_knn_wide_f32: bad parameter block (abi / size)")) return rc;
  return knn_wide("flooder_knn_wide_f32", a, NoCols{}, 0, stream);
}

extern "C" int flooder_knn_wide_profile_f32(const flooder_knn_wide_t* p, int n_cols, const int32_t* col_k,
                                            const int32_t* col_stat, int64_t plane_stride, void* stream) {
  static const char* who = "flooder_knn_wide_profile_f32";
  flooder_knn_wide_t a;   // the walk of the single entry at k = the largest k of the columns
  if (int rc = take(p, a, "flooder_knn_wide_profile_f32: bad parameter block (abi / size)")) return rc;
  if (n_cols < 1 || n_cols > FLOODER_KNN_COLS_MAX)
    return failf(FLOODER_E_ARG, "%s: n_cols must be in 1..%d", who, FLOODER_KNN_COLS_MAX);
  if (!col_k || !col_stat) return failf(FLOODER_E_ARG, "%s: col_k and col_stat must not be NULL", who);
  if (a.k < 1 || a.k > FLOODER_KNN_WIDE_MAX)
    return failf(FLOODER_E_ARG, "%s: k must be in 1..%d", who, FLOODER_KNN_WIDE_MAX);
  WideCols cols;
  memset(&cols, 0, sizeof(cols));
  cols.plane_stride = plane_stride;
  cols.n_cols = n_cols;
  int k_max = 0;
  for (int c = 0; c < n_cols; ++c) {
    const int k = col_k[c], s = col_stat[c];
    if (k < 1 || k > a.k) return failf(FLOODER_E_ARG, "%s: col_k must be in 1..k", who);
    if (s != 0 && s != 1) return failf(FLOODER_E_ARG, "%s: col_stat must be 0 (kth) or 1 (dtm)", who);
    for (int b = 0; b < c; ++b)
      if (col_k[b] == k && col_stat[b] == s)
        return failf(FLOODER_E_ARG, "%s: a (k, stat) column is listed twice", who);
    cols.col_k[c] = k;
    cols.col_stat[c] = s;
    if (k > k_max) k_max = k;
  }
  if (a.k != k_max) return failf(FLOODER_E_ARG, "%s: k must equal the largest col_k", who);
  return knn_wide(who, a, cols, plane_stride, stream);
}
