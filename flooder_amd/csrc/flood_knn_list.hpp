// flood_knn_list.hpp - the LDS key list of the one-wave-per-cell family (gfx950): knn_wide_kernel (flood_knn_wide.hip,
// the k nearest keys, k <= 1024) and knn_mass_kernel (flood_knn_mass.hip, the nearest keys up to a cumulative mass)
// keep a wave's ascending keys (d2 word << 32 | original id) in LDS and merge a buffer of BUF candidates into them with
// the ONE merge_buffer below; the capacity ladder of both entries is with_list_slots (internal).
//
// The two kernels' stack walks stay a copy each, kept in step by hand: one kernel over a LIST policy compiled to the
// parent's registers, LDS and scratch in every instantiation, but the wide family missed the time rule in two of its
// figures (HISTORY.md, "Wide k-nearest and mass sweeps"; profiles/knn_list_isa.txt, profiles/knn_list_times.jsonl).

#pragma once
#include "flood_common.hpp"
#include "flood_bvh.hpp"

namespace flooder {

constexpr int BUF = 128;                 // keys of a wave's insertion buffer (two per lane in a merge)
constexpr unsigned long long NOKEY = ~0ull;
typedef unsigned long long wkey_t;

// The list capacity that holds k keys - 64, 128, 256, 512 or 1024 - as its SLOTS = capacity / 64, one kernel
// instantiation each: f(std::integral_constant<int, SLOTS>{}) (with_knn_slots of flood_common.hpp is the register
// family's).  neighbors._CAPACITIES mirrors the ladder.
template <class F>
void with_list_slots(int k, F&& f) {
  if (k <= 64) f(std::integral_constant<int, 1>{});
  else if (k <= 128) f(std::integral_constant<int, 2>{});
  else if (k <= 256) f(std::integral_constant<int, 4>{});
  else if (k <= 512) f(std::integral_constant<int, 8>{});
  else f(std::integral_constant<int, 16>{});
}
inline int list_capacity(int k) {   // ... and that capacity as a number
  int cap = 0;
  with_list_slots(k, [&](auto slots) { cap = 64 * decltype(slots)::value; });
  return cap;
}

// Same-wave hand-off through LDS: what the lanes wrote is complete before any lane reads it (the pairing used around
// s_stack in flood_grad.hip, with the acquire side spelled out).
__device__ __forceinline__ void lds_handoff() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// number of keys of the ascending a[0..n) that are below x
__device__ __forceinline__ int keys_below(const wkey_t* a, int n, wkey_t x) {
  int lo = 0;
  while (n > 0) {
    const int half = n >> 1;
    if (a[lo + half] < x) {
      lo += half + 1;
      n -= half + 1;
    } else {
      n = half;
    }
  }
  return lo;
}

// The m <= BUF keys of buf (any order, distinct, none of them in the list) into the ascending list of k keys; what
// ends up at a place >= k falls off.  Leaves buf free and the list visible to every lane.
template <int SLOTS>
__device__ __forceinline__ void merge_buffer(wkey_t* list, wkey_t* buf, int k, int m, int lane) {
  lds_handoff();   // (the buffer's keys are in)
  wkey_t b[2];
  int rank[2], place[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    b[u] = lane + 64 * u < m ? buf[lane + 64 * u] : NOKEY;
    rank[u] = 0;
  }
  for (int j = 0; j < m; ++j) {
    const wkey_t x = buf[j];   // (one address: broadcast)
    rank[0] += x < b[0] ? 1 : 0;
    rank[1] += x < b[1] ? 1 : 0;
  }
  lds_handoff();   // (every lane has read the buffer before it is rewritten in order)
#pragma unroll
  for (int u = 0; u < 2; ++u)
    if (lane + 64 * u < m) {
      buf[rank[u]] = b[u];
      place[u] = rank[u] + keys_below(list, k, b[u]);
    }
  lds_handoff();   // (the sorted buffer is in)
  wkey_t l[SLOTS];
  int to[SLOTS];
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) {
    const int i = lane + 64 * s;
    to[s] = i;
    if (i < k) {
      l[s] = list[i];
      to[s] = i + keys_below(buf, m, l[s]);
    }
  }
  lds_handoff();   // (every lane has read the old list and the buffer)
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) {
    const int i = lane + 64 * s;
    if (i < k && to[s] != i && to[s] < k) list[to[s]] = l[s];
  }
#pragma unroll
  for (int u = 0; u < 2; ++u)
    if (lane + 64 * u < m && place[u] < k) list[place[u]] = b[u];
  lds_handoff();   // (the merged list is in)
}

}  // namespace flooder
