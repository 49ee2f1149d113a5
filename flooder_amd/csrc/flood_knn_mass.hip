// flood_knn_mass.hip - the distance to a WEIGHTED measure, one wave per cell (gfx950): the nearest sites of every sample
// up to the one at which their cumulative mass reaches a target tau, however many that are (at most a list capacity
// C <= 1024).  flooder_amd.distance_to_weighted_measure; the coreset of flooder_amd.voxel_measure.
//
// The measure is sum_i mu_i delta_(x_i) with mu_i >= 0 (masses[id], float32).  Per cell the sites are ordered by the key
// (d2 word << 32 | id) of flooder_knn_wide_f32, M_j = mu_(0) + ... + mu_(j) is the cumulative mass in that order and
// j* the first position with M_j* >= tau: the CROSSING.  The kernel returns the keys 0 .. j*, their number and the
// statistic of include/flooder_hip.h.  With unit masses and tau = k it is flooder_knn_wide_f32 at k, word for word.
//
// Walk: knn_wide_kernel's (flood_knn_wide.hip; lds_handoff, keys_below, merge_buffer and the capacity ladder are
// flood_knn_list.hpp's, shared with it; the walk itself is a COPY, kept in step by hand - that header says why).  A wave
// keeps the ascending key list in LDS, the same stack walk, four leaves at a time, the same insertion buffer.  What differs:
//   - the list has L = min(C, n_pts) places: a cloud smaller than the capacity is legal;
//   - after every merge the wave computes the cumulative masses of the list in float64 (a wave scan per row of 64
//     positions, carried row to row; masses[id] is GATHERED from global memory, an empty slot has mass 0) and looks for
//     the crossing;
//   - the cull bound is the crossing key list[j*] while the list has a crossing, else the last key list[L - 1] (all
//     ones, i.e. +inf, while that slot is empty);
//   - once a crossing exists only the places 0 .. j* are kept (len = j* + 1), and the next merge of m buffered keys
//     runs over len + m places (at most L): the work of a merge follows the crossing, not the capacity.
// The list may not simply be CUT at j* + 1 places for good: a site of small (or zero) mass that is inserted in front of
// the crossing moves it to a LATER position - [a: 5, b: 5] at tau = 10 crosses at b, position 1; a zero-mass site z
// nearer than a makes it [z: 0, a: 5, b: 5], still crossing at b, now position 2 - so a list of two places would lose
// the crossing key.  Every buffered key lies in front of the crossing key, so m of them move it back by at most m
// places: len + m places hold everything that matters, and what stood behind the crossing is never needed again.
//
// Exactness.  Keys are distinct and every point is offered at most once (as in the wide kernel).  Call B the cull bound.
//   (1) Offering more points only adds mass in front of a given key, so the cumulative mass AT a key never decreases and
//       the crossing key never increases; a list with a crossing whose crossing key falls off the end (C lighter keys
//       in front of it) continues with its L-th key, which is smaller.  So B never increases during a walk.
//   (2) A candidate is dropped only when its key is behind B (c < B fails; keys are distinct), a subtree or leaf only
//       when lb * SAFE > the d2 word of B, so that every point in it has a larger d2 and hence a larger key.
//   (3) Let F be the final answer over the WHOLE cloud: the crossing key if the L smallest keys reach tau, else the
//       L-th smallest key.  At every moment B >= F: the list holds a subset of the cloud, so its cumulative mass at any
//       key is at most the cloud's, and without a crossing its L-th key is not below the cloud's (a list that crosses at
//       B < F would make the cloud cross before F).  Hence nothing at or before F is ever dropped or emptied - what is
//       emptied lies behind B -, the final list holds every key of the cloud up to F, in order, and j*, the keys
//       0 .. j* and their masses are those of the whole cloud.
//   (4) The buffer only DELAYS insertions, as in the wide kernel: a delayed B is larger, which culls less.
// If the L smallest keys of the whole cloud do not reach tau the cell is NOT REACHED: its word is +inf, its count L.
// The crossing position is exact whenever the prefix sums are exactly representable - for every order of addition when
// the masses are integers with a total below 2^53, the coreset's counts.  For general masses the scan's order is fixed
// (Hillis-Steele within a row, then + carry), so the result is the same run to run; across an ambiguous crossing the
// value is continuous, the residual weight on the next key being about 0.
//
// Profile (flooder_knn_mass_profile_f32; distance_to_weighted_measure_profile): ONE walk to tau_max, the largest of the
// columns' targets (formed by every wave from the device array: nothing goes through the host), and an epilogue - it,
// and nothing else, is a compile-time variant (COLS) - that runs the crossing() scan of the final len places once per
// column at tau_c and writes the word and the count of (tau_c, stat_c) to plane c.
//   (5) Column c is the single call at (tau_c, stat_c) and the same capacity, word for word.  By (3) the final list
//       holds every key of the cloud up to F(tau_max), in order.  F(tau_c) <= F(tau_max) for tau_c <= tau_max: the cloud's
//       cumulative mass reaches the smaller target no later, and when it reaches neither within L keys both are the L-th
//       key.  So the list also holds every key of the cloud up to F(tau_c) in order - the places 0 .. j_c of the list the
//       single call at tau_c ends with.  M_j as crossing() computes it is a function of the places 0 .. j alone: the
//       Hillis-Steele scan of a row gives lane l the sum of the lanes <= l in an order fixed by l, the carry is the
//       total of the full rows in front, and places behind j (real keys here, emptied ones in the single call) enter
//       neither.  So j_c, M_(j_c - 1), rho_c and the strided sum over 0 .. j_c are those of the single call.  If the
//       walk's cell is not reached the list is the L smallest keys of the cloud, which is also what the single call at
//       tau_c ends with: it crosses at the same place or, like the walk, nowhere (word +inf, count L).  A column with no
//       crossing in a list that WAS cut (sums of masses that are no integers rounding to just below tau_c) takes the
//       last place, the single entry's fallback; there, and only there, the two may read an ambiguous crossing
//       differently, with a residual weight of about 0.
//
// No atomics, nothing in inline assembly; every output word is written once by plain vector stores.

#include "../../include/flooder_hip.h"
#include "flood_knn_list.hpp"

using namespace flooder;

namespace {

constexpr uint32_t INF_WORD = 0x7f800000u;

// The crossing of the ascending list[0..len): the first position j with M_j >= tau, or -1 (wave-uniform).  M_j is the
// float64 sum of masses[id] over the positions 0 .. j, an empty slot counting 0: an inclusive scan over the 64 lanes of
// a row (position i in lane i % 64), plus the carry of the rows before it.  m_prev: M_(j-1), 0 for j = 0 (it is below
// tau: j is the first).  n_real: the real keys among the positions scanned - all of them when there is no crossing.
__device__ __forceinline__ int crossing(const wkey_t* list, const float* __restrict__ masses, int len, double tau,
                                        int lane, double& m_prev, int& n_real) {
  double carry = 0.0;
  n_real = 0;
  for (int base = 0; base < len; base += 64) {
    const int i = base + lane;
    double v = 0.0;
    bool real = false;
    if (i < len) {
      const wkey_t key = list[i];
      real = key != NOKEY;
      if (real) v = (double)masses[(uint32_t)key];
    }
    n_real += __popcll(__ballot(real));
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const double u = __shfl_up(v, o);
      if (lane >= o) v += u;
    }
    v += carry;
    const unsigned long long hit = __ballot(real && v >= tau);   // (an empty slot adds nothing: it never crosses)
    if (hit) {
      const int l = __builtin_ctzll(hit);
      const double before = __shfl(v, l > 0 ? l - 1 : 0);
      m_prev = l > 0 ? before : carry;
      return base + l;
    }
    carry = __shfl(v, 63);   // (lanes past len added 0: lane 63 holds the row's total)
  }
  m_prev = carry;
  return -1;
}

// The squared "dtm" statistic of the positions 0 .. j of the list, j the crossing: the terms t_i = mu_i * w_i for i < j
// (float32 product of the float32 mass and the d2 word) and t_j = rho * w_j, added in the strided order of the wide
// kernel's statistic over kk = j + 1 positions (S_l = t_l + t_(l+64) + ..., then S_0 + S_1 + ... + S_(min(kk,64)-1),
// both left to right in float32), divided by tau_f.  Products and sums are separate roundings (no fused multiply-add).
__device__ __forceinline__ float mass_statistic(const wkey_t* list, const float* __restrict__ masses, int j, float rho,
                                                float tau_f, int lane) {
  const int kk = j + 1;
  float part = 0.f;
  if (lane < kk) {
    for (int i = lane; i < kk; i += 64) {
      const wkey_t key = list[i];
      const float w = __uint_as_float((uint32_t)(key >> 32));
      const float mu = i == j ? rho : masses[(uint32_t)key];
      const float t = __fmul_rn(mu, w);
      part = i == lane ? t : __fadd_rn(part, t);
    }
  }
  const int L = kk < 64 ? kk : 64;   // the lanes that hold a partial sum
  float acc = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(part), 0));
  for (int l = 1; l < L; ++l)
    acc = __fadd_rn(acc, __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(part), l)));
  return __fdiv_rn(acc, tau_f);
}

// One merge and what follows it.  `len` (wave-uniform) is the prefix of the list that still matters: the whole list
// (L entries) until a crossing exists, then the positions 0 .. j*.  The cnt buffer keys are all in front of the bound, so
// merged they take the places 0 .. len + cnt - 1: those behind len are emptied first (what stood there lies behind the
// crossing key and is not kept), the merge runs over km = min(L, len + cnt) places - its work follows the length -, and
// the crossing is looked for among them.  Sets len, the bound B and its d2; returns the crossing (or -1).
template <int SLOTS>
__device__ __forceinline__ int merge_and_cross(wkey_t* list, wkey_t* buf, const float* __restrict__ masses, int L,
                                               double tau, int lane, int& len, int cnt, wkey_t& bound, float& bound_f,
                                               double& m_prev, int& n_real) {
  const int km = len + cnt < L ? len + cnt : L;
  lds_handoff();   // (every lane has read the list before places are emptied)
  for (int i = len + lane; i < km; i += 64) list[i] = NOKEY;
  merge_buffer<SLOTS>(list, buf, km, cnt, lane);
  const int j = crossing(list, masses, km, tau, lane, m_prev, n_real);
  len = j >= 0 ? j + 1 : km;
  bound = list[len - 1];
  bound_f = bound == NOKEY ? __builtin_inff() : __uint_as_float((uint32_t)(bound >> 32));
  return j;
}

// The columns of the epilogue, a compile-time variant of the ONE kernel (the form of knn_wide_kernel): NoCols
// (flooder_knn_mass_f32) walks to tau = *target and writes the word of (tau, stat) to out_bits[g]; MassCols
// (flooder_knn_mass_profile_f32) walks to the largest of targets[0..n_cols) and writes a word and a count per listed
// (tau_c, stat_c) to out_bits / out_count[c * plane_stride + g].  The walk and the merges do not know which it is.
// target_t is what the kernel takes in the place of the target: the single entry's pointer, or the columns by value -
// so the single entry's kernel keeps its argument list to the byte.
struct NoCols {
  typedef const double* __restrict__ target_t;
};
struct MassCols {
  typedef MassCols target_t;
  int64_t plane_stride;
  const double* targets;   // DEVICE, n_cols
  int n_cols;
  int col_stat[FLOODER_KNN_COLS_MAX];
};

// The largest target of the columns (wave-uniform; every wave forms it itself: nothing goes through the host)
__device__ __forceinline__ double walk_target(const MassCols& cols) {
  double tau = cols.targets[0];
  for (int c = 1; c < cols.n_cols; ++c) {
    const double t = cols.targets[c];
    tau = t > tau ? t : tau;
  }
  return tau;
}

template <int DIM, int SLOTS, class COLS>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void knn_mass_kernel(
    const float* __restrict__ pts, int64_t n_pts, const float* __restrict__ nodes, Levels lv,
    const int32_t* __restrict__ order, const float* __restrict__ verts, const float* __restrict__ weights, int k1, int R,
    int64_t n_cells, int stat, const int32_t* __restrict__ sample_order, const float* __restrict__ masses,
    const typename COLS::target_t target, int ld_out, uint32_t* __restrict__ out_bits, int32_t* __restrict__ out_count,
    int32_t* __restrict__ out_ids, uint32_t* __restrict__ out_d2) {
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
  const int k = n_pts < CAP ? (int)n_pts : CAP;   // the list's length L: the capacity, or the whole cloud
  const int merge_at = k < 64 ? k : 64;
  double tau;   // the target of the walk
  if constexpr (std::is_same<COLS, NoCols>::value) tau = *target;
  else tau = walk_target(target);
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
    wkey_t bound = NOKEY;   // the cull bound B: the crossing key, else the list's last key (wave-uniform)
    float bound_f = __builtin_inff();
    double m_prev;
    int n_real;
    int len = k;         // the prefix of the list that still matters (wave-uniform): see merge_and_cross
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
        ok = !(lb * SAFE > bound_f);
      }
      unsigned long long mask = __ballot(ok);
      __builtin_amdgcn_wave_barrier();   // (every lane has read the popped entry before a push may overwrite it)
      if (lvl == 0) {
        while (mask) {
          if (cnt > BUF - 64) {   // fewer than 64 free places: merge, and test the waiting leaves against the new bound
            merge_and_cross<SLOTS>(list, buf, masses, k, tau, lane, len, cnt, bound, bound_f, m_prev, n_real);
            cnt = 0;
            mask &= __ballot(!(lb * SAFE > bound_f));
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
          const bool in = c < bound;
          const unsigned long long take_mask = __ballot(in);
          if (in) buf[cnt + __popcll(take_mask & below)] = c;   // (cnt <= BUF - 64 here: at most 64 more)
          cnt += __popcll(take_mask);
        }
        if (cnt >= merge_at) {
          merge_and_cross<SLOTS>(list, buf, masses, k, tau, lane, len, cnt, bound, bound_f, m_prev, n_real);
          cnt = 0;
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
    if (cnt > 0) merge_and_cross<SLOTS>(list, buf, masses, k, tau, lane, len, cnt, bound, bound_f, m_prev, n_real);
    lds_handoff();
    // ---- the crossing of the final list (the same scan over the same len places as after the last merge); its keys,
    // their number and the statistic
    if constexpr (std::is_same<COLS, NoCols>::value) {
      int j = crossing(list, masses, len, tau, lane, m_prev, n_real);
      if (j < 0 && len < k) {
        // A crossing existed (len shrank) and the float64 sums of this arrangement round to just below tau - masses that
        // are no integers only.  The crossing is the last place; its residual is about its whole mass.
        j = len - 1;
        m_prev -= (double)masses[(uint32_t)list[j]];
      }
      const int count = j >= 0 ? j + 1 : n_real;
      if (out_ids || out_d2) {
        const int64_t row = g * (int64_t)ld_out;
        for (int i = lane; i < ld_out; i += 64) {
          const wkey_t key = i < count ? list[i] : NOKEY;
          if (out_ids) out_ids[row + i] = i < count ? (int32_t)(uint32_t)key : -1;
          if (out_d2) out_d2[row + i] = i < count ? (uint32_t)(key >> 32) : INF_WORD;
        }
      }
      if (out_count && lane == 0) out_count[g] = count;
      if (out_bits) {
        uint32_t word = INF_WORD;   // not reached
        if (j >= 0) {
          if (stat == 0) {
            word = (uint32_t)(list[j] >> 32);
          } else {
            const float rho = (float)(tau - m_prev);
            word = __float_as_uint(mass_statistic(list, masses, j, rho, (float)tau, lane));
          }
        }
        if (lane == 0) out_bits[g] = word;
      }
    } else {
      // Column c is the single call at (targets[c], col_stat[c]) - (5) of the header: the same scan over the places
      // 0 .. j_c of the same keys, the same fallback, the same statistic.  No rows: lists are per target.
      const MassCols& cols = target;
      for (int c = 0; c < cols.n_cols; ++c) {
        const double tau_c = cols.targets[c];
        int j = crossing(list, masses, len, tau_c, lane, m_prev, n_real);
        if (j < 0 && len < k) {   // (the list was cut and its sums round to just below tau_c: the last place)
          j = len - 1;
          m_prev -= (double)masses[(uint32_t)list[j]];
        }
        uint32_t word = INF_WORD;   // not reached
        if (j >= 0) {
          if (cols.col_stat[c] == 0) {
            word = (uint32_t)(list[j] >> 32);
          } else {
            const float rho = (float)(tau_c - m_prev);
            word = __float_as_uint(mass_statistic(list, masses, j, rho, (float)tau_c, lane));
          }
        }
        if (lane == 0) {
          const int64_t at = (int64_t)c * cols.plane_stride + g;
          out_bits[at] = word;
          if (out_count) out_count[at] = j >= 0 ? j + 1 : n_real;
        }
      }
    }
    lds_handoff();   // (every lane has read the list before the next cell resets it)
  }
}

// What the entries add to the block of flooder_knn_wide_f32 (whose k is the capacity here)
struct MassArgs {
  const float* masses;
  const double* target;   // the single entry's tau; not used with columns (they carry theirs)
  int ld_out;
  int32_t* out_count;
};

template <int DIM>
struct KnnMassOp {
  template <int SLOTS, class COLS>
  static void launch(const flooder_knn_wide_t& a, const MassArgs& m, const COLS& cols, const Levels& lv, int64_t n_cells,
                     hipStream_t st) {
    typename COLS::target_t target;
    if constexpr (std::is_same<COLS, NoCols>::value) target = m.target;
    else target = cols;
    hipLaunchKernelGGL((knn_mass_kernel<DIM, SLOTS, COLS>), stack_walk_grid(n_cells), dim3(64 * WAVES_PER_BLOCK), 0, st,
                       a.pts_sorted, a.n_pts, a.nodes, lv, a.order, a.verts, a.weights, a.k1, a.R, n_cells, a.stat,
                       a.sample_order, m.masses, target, m.ld_out, a.out_bits, m.out_count, a.out_ids, a.out_d2);
  }
  template <class COLS>
  static int run(const flooder_knn_wide_t& a, const MassArgs& m, const COLS& cols, const Levels& lv, int64_t n_cells,
                 hipStream_t st) {
    if constexpr (DIM < 2) {
      return fail(FLOODER_E_ARG, "flooder_knn_mass_f32: dim must be in 2..8");
    } else {
      with_list_slots(a.k, [&](auto slots) { launch<decltype(slots)::value>(a, m, cols, lv, n_cells, st); });
      return check_launch("knn_mass");
    }
  }
};

// The checks of both entries (the profile entry has made its column checks already) and the launch
template <class COLS>
int knn_mass(const char* who, const flooder_knn_wide_t& a, const MassArgs& m, const COLS& cols, int64_t plane_stride,
             void* stream) {
  constexpr bool single = std::is_same<COLS, NoCols>::value;
  if (a.k < 1 || a.k > FLOODER_KNN_WIDE_MAX)
    return failf(FLOODER_E_ARG, "%s: capacity (the block's k) must be in 1..%d", who, FLOODER_KNN_WIDE_MAX);
  if (a.dim < 2 || a.dim > FLOODER_MAX_DIM) return failf(FLOODER_E_ARG, "%s: dim must be in 2..8", who);
  if (a.stat != 0 && a.stat != 1) return failf(FLOODER_E_ARG, "%s: stat must be 0 (kth) or 1 (dtm)", who);
  if (a.n_pts < 1) return failf(FLOODER_E_ARG, "%s: no points", who);
  if (a.n_pts > 0x7fffffffLL) return failf(FLOODER_E_ARG, "%s: more than 2^31 - 1 points", who);
  if (a.n_simplices > 0 && a.R > 0 && a.n_simplices > ((1LL << 32) - 3) / a.R)
    return failf(FLOODER_E_ARG, "%s: n_simplices * R must be below 2^32 - 2", who);
  Levels lv;
  if (int rc = stack_walk_levels(who, a.n_pts, lv)) return rc;
  if (single) {
    if (!a.out_bits && !m.out_count && !a.out_ids && !a.out_d2)
      return failf(FLOODER_E_ARG, "%s: no output (out_bits, out_count, out_ids and out_d2 are all NULL)", who);
    if (a.out_ids && !a.order) return failf(FLOODER_E_ARG, "%s: out_ids needs order (tree row -> original id)", who);
    const int cap = list_capacity(a.k);
    if ((a.out_ids || a.out_d2) && (m.ld_out < 1 || m.ld_out > cap))
      return failf(FLOODER_E_ARG, "%s: ld_out must be in 1..%d (the list capacity that holds capacity = %d)", who, cap,
                   a.k);
    if (!m.masses || !m.target) return failf(FLOODER_E_ARG, "%s: masses and target must not be NULL", who);
  } else {
    if (a.out_ids || a.out_d2)
      return failf(FLOODER_E_ARG, "%s: out_ids and out_d2 must be NULL (lists are per target)", who);
    if (!a.out_bits) return failf(FLOODER_E_ARG, "%s: out_bits (the planes) must not be NULL", who);
    if (!m.masses) return failf(FLOODER_E_ARG, "%s: masses must not be NULL", who);
    if (a.n_simplices > 0 && a.R > 0 && plane_stride < a.n_simplices * (int64_t)a.R)
      return failf(FLOODER_E_ARG, "%s: plane_stride must be at least n_simplices * R", who);
  }
  if (a.n_simplices == 0 || a.R == 0) return FLOODER_OK;
  if (!a.pts_sorted || !a.nodes || !a.verts || !a.weights || a.k1 < 1 || a.R < 0 || a.n_simplices < 0)
    return failf(FLOODER_E_ARG, "%s: bad argument (null pointer, k1, R, n_simplices)", who);
  return dispatch_dim<KnnMassOp>(a.dim, a, m, cols, lv, a.n_simplices * (int64_t)a.R, (hipStream_t)stream);
}

}  // namespace

extern "C" int flooder_knn_mass_f32(const flooder_knn_wide_t* p, const float* masses, const double* target, int32_t ld_out,
                                    int32_t* out_count, void* stream) {
  flooder_knn_wide_t a;
  if (int rc = take(p, a, "flooder_knn_mass_f32: bad parameter block (abi / size)")) return rc;
  return knn_mass("flooder_knn_mass_f32", a, MassArgs{masses, target, ld_out, out_count}, NoCols{}, 0, stream);
}

extern "C" int flooder_knn_mass_profile_f32(const flooder_knn_wide_t* p, const float* masses, int n_cols,
                                            const double* targets, const int32_t* col_stat, int64_t plane_stride,
                                            int32_t* out_count, void* stream) {
  static const char* who = "flooder_knn_mass_profile_f32";
  flooder_knn_wide_t a;   // the walk of the single entry at the largest target of the columns
  if (int rc = take(p, a, "flooder_knn_mass_profile_f32: bad parameter block (abi / size)")) return rc;
  if (n_cols < 1 || n_cols > FLOODER_KNN_COLS_MAX)
    return failf(FLOODER_E_ARG, "%s: n_cols must be in 1..%d", who, FLOODER_KNN_COLS_MAX);
  if (!targets || !col_stat) return failf(FLOODER_E_ARG, "%s: targets and col_stat must not be NULL", who);
  MassCols cols;
  memset(&cols, 0, sizeof(cols));
  cols.plane_stride = plane_stride;
  cols.targets = targets;
  cols.n_cols = n_cols;
  for (int c = 0; c < n_cols; ++c) {
    if (col_stat[c] != 0 && col_stat[c] != 1)
      return failf(FLOODER_E_ARG, "%s: col_stat must be 0 (kth) or 1 (dtm)", who);
    cols.col_stat[c] = col_stat[c];
  }
  return knn_mass(who, a, MassArgs{masses, nullptr, 0, out_count}, cols, plane_stride, stream);
}
