// flood_knn_merge.hip - exact k-best merge of the robust filtration over point shards (gfx950).
//
// flooder_knn_merge_f32 takes, per cell (simplex, sample), W ascending lists of k squared distances - the k smallest of
// each of W point shards, as flooder_sweep_knn_profile_f32 writes them with the columns (1, "kth") .. (k, "kth") - and
// writes the word flooder_sweep_knn_f32 would write for the union of the shards: the k-th smallest of the W * k values
// ("kth") or the mean of the k smallest ("dtm").
//
//   knn_merge<K>   one lane per cell.  The running list is sweep_knn_kernel's: int32 words of the float32 values (d2 is
//                  never negative and never NaN: signed integer order is value order, -inf included) in K registers, K
//                  the smallest of 2, 4, 8, 16, 32 that holds k, the list in the LAST k of them behind K - k words of
//                  -inf, so that the k-th best is always the last register and the insertion is one branch-free chain
//                  of K (min, max) pairs - no register indexed by a run-time value.  List 0 is loaded straight into the
//                  registers (it is ascending).  Every further list is read plane by plane, one coalesced dword load
//                  per plane; a wave vote `candidate < k-th best in any lane` decides whether the chain runs.  A list is
//                  ascending per lane and a lane's k-th best never grows, so a plane that no lane improves on ends that
//                  list for the wave: everything behind it is >= a value that was already >= the k-th best.  The break
//                  is wave-uniform.  No atomics, no LDS; every output word is written once by a plain vector store.
//
// Exactness.  A point among the k nearest of a sample over the whole cloud is among the k nearest of its own shard (at
// most k - 1 points of the cloud, let alone of the shard, are nearer - ties: a shard list that drops a point tying its
// k-th value keeps k values <= it, and only VALUES are merged).  So the union of the W lists contains the global list
// as a multiset, and its k smallest values are the global k smallest, value for value.  The merge depends on values
// only - no tie rule, no rule for doubled points, no dependence on the order of the lists.  +inf words (a shard with
// fewer than k points) never pass the vote.  The epilogue is sweep_knn_kernel's: "dtm" adds the k values ascending,
// smallest first, by sequential float32 additions and divides by (float)k with the correctly rounded division.

#include "flood_common.hpp"


using namespace flooder;

namespace {

template <int K>
__global__ __launch_bounds__(256) void knn_merge_kernel(const int32_t* __restrict__ lists, int W, int k, int stat,
                                                        int64_t n, uint32_t* __restrict__ out_bits) {
  const int64_t cell = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = cell < n;
  const int64_t c = live ? cell : n - 1;   // duplicate of the last cell, never stored
  const int first = K - k;                 // the k live slots are list[first .. K-1]  (wave-uniform)

  int list[K];
#pragma unroll
  for (int i = 0; i < K; ++i) {
    list[i] = (int)0xff800000u;
    if (i >= first) list[i] = lists[(int64_t)(i - first) * n + c];   // (uniform branch; the register index is constant)
  }

  for (int w = 1; w < W; ++w) {
    const int32_t* lw = lists + (int64_t)w * k * n + c;
#pragma unroll 1
    for (int j = 0; j < k; ++j) {   // (not unrolled: the body holds an insertion chain)
      int di = lw[(int64_t)j * n];
      // ascending per lane: a plane no lane improves on ends this list for the wave
      if (__ballot(di < list[K - 1]) == 0ull) break;
#pragma unroll
      for (int i = 0; i < K; ++i) {
        const int hi = list[i] > di ? list[i] : di;
        list[i] = list[i] < di ? list[i] : di;
        di = hi;
      }
    }
  }

  if (live) {
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
    out_bits[cell] = __float_as_uint(v);
  }
}

}  // namespace

extern "C" int flooder_knn_merge_f32(const flooder_knn_merge_t* p, void* stream) {
  flooder_knn_merge_t a;
  if (int rc = take(p, a, "flooder_knn_merge_f32: bad parameter block (abi / size)")) return rc;
  if (a.k < 1 || a.k > FLOODER_KNN_MAX) return fail(FLOODER_E_ARG, "flooder_knn_merge_f32: k must be in 1..32");
  if (a.stat != 0 && a.stat != 1) return fail(FLOODER_E_ARG, "flooder_knn_merge_f32: stat must be 0 (kth) or 1 (dtm)");
  if (a.n_lists < 1) return fail(FLOODER_E_ARG, "flooder_knn_merge_f32: n_lists must be at least 1");
  if (a.n_cells < 0) return fail(FLOODER_E_ARG, "flooder_knn_merge_f32: n_cells must not be negative");
  if (a.n_cells == 0) return FLOODER_OK;
  if (!a.lists || !a.out_bits || a.n_cells > 0xffffff00LL)   // (a launch holds fewer than 2^32 threads)
    return fail(FLOODER_E_ARG, "flooder_knn_merge_f32: bad argument (null pointer, more than 2^32 - 256 cells)");
  const int64_t blocks = (a.n_cells + 255) / 256;
  with_knn_slots(a.k, [&](auto kc) {
    hipLaunchKernelGGL((knn_merge_kernel<decltype(kc)::value>), dim3((unsigned)blocks), dim3(256), 0,
                       (hipStream_t)stream, a.lists, a.n_lists, a.k, a.stat, a.n_cells, a.out_bits);
  });
  return check_launch("knn_merge");
}
