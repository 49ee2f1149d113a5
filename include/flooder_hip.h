/*
 * flooder_hip.h - C ABI of the MI355X (gfx950) coverage-sweep library, libflooder_hip.so.
 *
 * The reference (plus-rkwitt/flooder) is a pure-Python package; the seam its hot path crosses is the
 * pair of Triton kernel wrappers in flooder/triton_kernels.py and their call sites in
 * flooder/core.py:200-226.  Each entry point below names the reference interface it replaces.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer unless it says "host"; memory is owned by the caller, the
 *     library never allocates, frees or synchronises; work is enqueued on `stream` (a hipStream_t,
 *     passed as void*; NULL = the default stream) and the pointers must stay valid until that work
 *     has completed;
 *   - return value 0 = success, negative = error (FLOODER_E_*); flooder_last_error() gives the text
 *     for the calling thread; nothing throws;
 *   - points / candidates are float32, row-major, `ld` floats per row (ld >= dim);
 *   - squared distances travel as the uint32 bit pattern of a non-negative float32 ("d2 bits"):
 *     for non-negative floats unsigned integer order equals numeric order, so min/max over them are
 *     exact integer atomics.  +inf (0x7f800000) means "no candidate seen" (triton_kernels.py:70).
 */
#ifndef FLOODER_HIP_H
#define FLOODER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FLOODER_ABI_VERSION 1

#define FLOODER_OK 0
#define FLOODER_E_ARG (-1)    /* bad argument (null pointer, unsupported dim, ...) */
#define FLOODER_E_LAUNCH (-2) /* HIP reported an error at launch                    */
#define FLOODER_E_DEVICE (-3) /* no gfx950 device / wrong architecture              */

#define FLOODER_MAX_DIM 8      /* ambient dimensions 1..8 are compiled              */
#define FLOODER_MAX_VERTS 9    /* vertices per simplex: max_dimension + 1 <= 9      */
#define FLOODER_CAND_ALIGN 8   /* each simplex's candidate list is padded to x8     */
#define FLOODER_SWEEP_CHUNK 2048 /* candidates per sweep work item                   */
#define FLOODER_TILE_SAMPLES 512 /* samples per sweep work item (64 lanes x 8)       */
#define FLOODER_BVH_LEAF 16      /* points per leaf of the point hierarchy            */
#define FLOODER_BVH_FANOUT 64    /* children per inner node (one per lane)            */
#define FLOODER_BVH_MAX_LEVELS 6 /* 16 * 64^5 points                                  */
#define FLOODER_QUEUE_SHARDS 16    /* heads of a sharded work queue ...                        */
#define FLOODER_QUEUE_WORDS 512    /* ... and the zeroed int32 words one queue takes (heads 128 B apart) */
#define FLOODER_BBOX_BLOCKS 1024  /* partial results of flooder_bbox_f32               */
#define FLOODER_WIT_MAX_COARSE 256  /* coarse samples per simplex of flooder_sweep_witness_f32 (4 per lane) */
#define FLOODER_WIT_MAX_ROWS 8192   /* samples per simplex it takes at most                                  */

int flooder_abi_version(void);
const char* flooder_last_error(void);

/* Name of the GPU architecture of `device` copied into buf (e.g. "gfx950:sramecc+:xnack-"). */
int flooder_device_arch(int device, char* buf, int buflen);

/* Tuning options (process-wide ints); none of them changes a result bit.  THE list - every name with its default, the
 * values it accepts and what it does - is flooder_amd/csrc/flood_options.def, one row per option; the comments of the
 * entry points below name the options that bear on them.  flooder_set_option returns FLOODER_E_ARG for a NULL or
 * unknown name and for a value outside the option's row, and then changes nothing.  flooder_get_option stores the
 * current value in *value (FLOODER_E_ARG: NULL or unknown name, NULL value): save and restore with it instead of
 * copying defaults.  The options are read by the host code of the entry points when they are called - set them between
 * calls, from one thread at a time. */
int flooder_set_option(const char* name, int value);
int flooder_get_option(const char* name, int* value);

/* Row stride (floats) of a padded point / candidate row for ambient dimension `dim`:
 * 1,2 -> 2; 3,4 -> 4; 5..8 -> 8.  Rows in this layout are read with one vector load. */
int flooder_padded_dim(int dim);

/*
 * Ball membership count.  Replaces compute_mask + the per-row count of compute_mask_kernel
 * (flooder/triton_kernels.py:99-158, call site flooder/core.py:210-217): point j is a candidate of
 * simplex i iff sum_k (pts[j,k]-centers[i,k])^2 <= radii[i]^2 (squared, "<=", no sqrt; :137-148).
 * Instead of materialising the (n, m+512) bool mask it only counts, per simplex, over that simplex's
 * own slab [slab_lo[i], slab_hi[i]) of the cloud sorted along its widest axis (core.py:140-144,
 * 201-208; the per-simplex slab is a subset of the reference's per-batch slab and still contains the
 * whole ball, so the candidate sets are identical).
 *   counts[i] (int32) must be zeroed by the caller; it receives the number of candidates.
 */
int flooder_ball_count_f32(const float* pts, int64_t n_pts, int dim, int ld,
                           const float* centers /* n_simplices x dim */,
                           const float* radii /* n_simplices */,
                           const int64_t* slab_lo, const int64_t* slab_hi, int64_t n_simplices,
                           int32_t* counts, void* stream);

/*
 * Candidate compaction.  Replaces torch.nonzero(mask) + the index casts + the gather
 * y[w_idx] inside compute_filtration_kernel (core.py:218, triton_kernels.py:33,39,80-85): writes
 * the coordinates of simplex i's candidates to cand rows [cand_off[i], cand_off[i]+counts[i]) and
 * +inf rows up to cand_off[i+1] (the reference pads with indices that load +inf, :39), in
 * unspecified order.  cand has padded rows (flooder_padded_dim(dim) floats).
 *   cand_off: (n_simplices+1) int64, multiples of FLOODER_CAND_ALIGN;  cursor: n_simplices int32,
 *   zeroed by the caller (scratch).
 */
int flooder_ball_fill_f32(const float* pts, int64_t n_pts, int dim, int ld,
                          const float* centers, const float* radii,
                          const int64_t* slab_lo, const int64_t* slab_hi, int64_t n_simplices,
                          const int32_t* counts, const int64_t* cand_off, int32_t* cursor,
                          float* cand, void* stream);

/*
 * Coverage sweep.  Replaces compute_filtration / compute_filtration_kernel
 * (flooder/triton_kernels.py:12-96, call site core.py:219-226) fused with the sample generation
 * points_on_simplex = weights @ simplex_vertices (core.py:188): for simplex s and sample r
 *     p = sum_j weights[r,j] * verts[s,j,:]
 *     out_d2[s,r] = min(out_d2[s,r], min_w sum_k (p_k - cand[w,k])^2)      (direct differences, :36-44)
 * over the candidates w of s.  out_d2 (n_simplices x R uint32 d2 bits) must be pre-set to +inf bits
 * (flooder_fill_u32); it is combined with atomic min so several launches (point shards) or several
 * work items may target the same cell.  Work is split into items of (simplex, 512-sample tile,
 * 2048-candidate chunk); item_prefix (n_simplices+1 int64) = exclusive prefix sum of
 * tiles * ceil(count/2048) per simplex; queue = one int32 zeroed by the caller (work-queue head).
 */
int flooder_sweep_f32(const float* cand, const int64_t* cand_off, const int32_t* counts, int dim,
                      const float* verts /* n_simplices x k1 x dim */, const float* weights /* R x k1 */,
                      int k1, int R, int64_t n_simplices, const int64_t* item_prefix, int32_t* queue,
                      uint32_t* out_d2, void* stream);

/*
 * Face maxima.  Replaces the extraction at core.py:251-276: out_face[s,f] =
 * sqrt(max_{r in rows of face f} out_d2[s,r]) where face f's rows are
 * face_rows[face_ptr[f] .. face_ptr[f+1]) (CSR over the concatenated faces of every codimension,
 * grid mode) or all R rows (random mode: n_faces = 1, face_ptr = {0,R}, face_rows = 0..R-1).
 * out_dist (n_simplices x R float32, may be NULL) receives sqrt of every cell (the reference's
 * `distances` tensor, triton_kernels.py:44).
 */
int flooder_face_max_f32(const uint32_t* d2, int64_t n_simplices, int R, const int32_t* face_ptr,
                         const int32_t* face_rows, int n_faces, float* out_face, float* out_dist,
                         void* stream);

/*
 * ---- Hierarchically culled sweep (default device path) ---------------------------------------------
 * Replaces the reference's pruning chain as a whole - slab selection by searchsorted (core.py:201-208),
 * compute_mask (triton_kernels.py:161-223), torch.nonzero (core.py:218) and compute_filtration
 * (triton_kernels.py:48-96): instead of a bounding ball per simplex, an implicit bounding-box tree over
 * the Morton-sorted cloud is traversed per tile of samples, and only leaves that can still lower a
 * running minimum are evaluated.  The value computed is the exact minimum over ALL points (what the
 * reference's CPU branch returns, core.py:197-199), with the same direct-difference arithmetic.
 */

/* Bounding box of the cloud, on the device: box[0:dim] = min, box[8:8+dim] = max (box: 16 floats;
 * partial: FLOODER_BBOX_BLOCKS * 16 floats of scratch).  Replaces points.max(dim=0) - points.min(dim=0)
 * of core.py:140-142 without a host round trip. */
int flooder_bbox_f32(const float* pts, int64_t n_pts, int dim, int ld, float* box, float* partial, void* stream);

/* The two stages of flooder_bbox_f32 on their own, for a cloud that arrives in chunks (BASELINE.json configs[4]:
 * points streamed from pinned host memory; the reference's counterpart is its batch-bounded slabs, core.py:193-217):
 * flooder_bbox_chunk_f32 reduces the n_rows rows of one chunk with n_blocks blocks into partial[0 : 16 * n_blocks]
 * as soon as the chunk's copy has landed (enqueue it behind the copy's event), flooder_bbox_reduce_f32 folds the
 * n_partial rows of all chunks into box.  flooder_amd.PointIndex.from_host is the caller. */
int flooder_bbox_chunk_f32(const float* pts, int64_t n_rows, int dim, int ld, float* partial, int n_blocks,
                           void* stream);
int flooder_bbox_reduce_f32(const float* partial, int n_partial, int dim, float* box, void* stream);

/* 64-bit space-filling-curve codes of the points relative to `box` (DEVICE, layout of flooder_bbox_f32);
 * floor(63/dim) (max 21) bits per axis.  The caller sorts the cloud by these codes.  Hilbert codes by
 * default (option "curve" = 1; 0 = Morton / Z-order): consecutive points are neighbours in space, so the
 * 16-point leaves of the box tree are tight - the tree sweep of cfg 2 takes 3.3 ms instead of 6.5 ms. */
int flooder_morton_f32(const float* pts, int64_t n_pts, int dim, int ld, const float* box, int64_t* codes,
                       void* stream);
/* The same, and `zero_words` int32 words at `zero_buf` are set to zero on the way: the density grid that the kernels of
 * flooder_index_rows_f32 - enqueued behind this one - add into, without a fill launch of its own. */
int flooder_morton_zero_f32(const float* pts, int64_t n_pts, int dim, int ld, const float* box, int64_t* codes,
                            int32_t* zero_buf, int64_t zero_words, void* stream);

/* Number of low bits a curve code of flooder_morton_f32 occupies for ambient dimension dim (bits per axis x dim;
 * option "curve_bits": bits per axis, default 8 in 3D, 12 elsewhere, at most floor(63 / dim) and 21).  When
 * this is <= 32 the `codes` buffers of flooder_morton_f32 / flooder_index_sort hold n uint32 words (in the first
 * half of the n x int64 allocation), else n int64 words. */
int flooder_curve_key_bits(int dim);

/* Sort of the curve codes: order[j] = index of the point with the j-th smallest code (stable), codes_sorted = the
 * codes in that order.  rocprim::radix_sort_pairs over the low key_bits bits only (flooder_curve_key_bits).
 * tmp: flooder_index_sort_bytes(n_pts) bytes of device scratch.  Replaces torch.argsort of core.py:143. */
int64_t flooder_index_sort_bytes(int64_t n_pts);
int flooder_index_sort(const int64_t* codes, int64_t n_pts, int key_bits, int64_t* codes_sorted, int32_t* order,
                       void* tmp, int64_t tmp_bytes, void* stream);

/* The same sort (same library kernels, same stable order) without the seven fill launches the library call makes for
 * three 8-bit passes: its state - digit histograms, one look-back array and one block ticket per pass - is
 * `flooder_index_sort_state_words(n_pts, key_bits)` int32 words that the CALLER has zeroed on this stream before the
 * call (the curve-code kernel does it on its way: hand flooder_morton_zero_f32 a zero_buf that ends in them).  Keys
 * of at most 32 bits and fewer than 2^30 rows (state_words returns 0 otherwise: use flooder_index_sort); tmp: 8 * n_pts
 * bytes (flooder_index_sort_bytes is enough).  cfg 2's index build: 7 launches and ~17 us less.  The passes also run
 * in a block shape chosen by the cloud's size instead of the library's 1024 x 16 keys (62 blocks for a million keys on
 * 256 CUs): 512 x 8 below 1.5 M keys, 1024 x 8 above (option "sort_shape" 0; 1 / 2 / 3 force 512 x 8 / 1024 x 16 /
 * 1024 x 8) - index build 163 -> 136 us at 1 M points, 947 -> 905 us at 16 M.  Same order whatever the shape. */
int64_t flooder_index_sort_state_words(int64_t n_pts, int key_bits);
int flooder_index_sort_zeroed(const int64_t* codes, int64_t n_pts, int key_bits, int64_t* codes_sorted, int32_t* order,
                              void* tmp, int64_t tmp_bytes, int32_t* state, void* stream);

/* Order of a balanced k-d tree over the cloud (default of the point index above 3 dimensions; core.KD_ORDER_ABOVE_DIM):
 * order[j] = index of the point at row j, such that every ALIGNED group of 16 * 2^i rows - the leaves and inner nodes
 * of the implicit box tree - is a cell of the tree (each level splits every group along the widest axis of its box at
 * the positional median).  One (segmented box, key, radix sort) round per level; no curve codes.  In 6D the boxes of
 * the 1024-point nodes overlap 3x less than those of a Hilbert order and the sorted sweep tests and evaluates fewer
 * leaves.  Any order is a valid index: results do not depend on it.  tmp: flooder_kd_order_bytes(n_pts) bytes of device
 * scratch (-1: too many points, n_pts <= 2^31 - 1).  Replaces torch.argsort of core.py:143 like flooder_index_sort. */
int64_t flooder_kd_order_bytes(int64_t n_pts);
int flooder_kd_order_f32(const float* pts, int64_t n_pts, int dim, int ld, int32_t* order, void* tmp, int64_t tmp_bytes,
                         void* stream);

/* Sub-cloud of a block of simplices (block-sharded runs): the rows of pts (n_pts x dim floats, row stride ld) that lie
 * inside the box (box: 2 * dim device floats, lo then hi, bounds inclusive) AND - dim 2 / 3, with cell_flags
 * (flooder_select_grid_bytes(dim) zeroed bytes), cloud_box (the 16 floats of flooder_bbox_f32) and n_balls bounding
 * balls (centers n_balls x dim, radii) given - in a cell of a coarse grid over the cloud's box that one of the balls
 * reaches; compacted into out (room for n_pts rows of dim floats; any order), their number in *count (zeroed by the
 * caller).  With landmarks that are cloud points every witness of a simplex lies in its bounding ball
 * (core.py:156-172), so the sweep of the block against this sub-cloud gives the values of the whole cloud. */
int64_t flooder_select_grid_bytes(int dim);
int flooder_box_select_f32(const float* pts, int64_t n_pts, int dim, int ld, const float* box, const float* cloud_box,
                           const float* centers, const float* radii, int64_t n_balls, uint8_t* cell_flags, float* out,
                           int32_t* count, void* stream);

/* out (n_pad x flooder_padded_dim(dim) floats) = rows order[0], order[1], ... of pts, padding columns 0, then
 * +inf rows up to n_pad (a multiple of FLOODER_BVH_LEAF).  Replaces points[indices] of core.py:143. */
int flooder_gather_rows_f32(const float* pts, int64_t n_pts, int dim, int ld, const int32_t* order, float* out,
                            int64_t n_pad, void* stream);

/* Number of nodes (all levels, each padded to a multiple of 64) of the tree over n_pts points. */
int64_t flooder_bvh_node_count(int64_t n_pts);

/* Build the tree.  pts_sorted: padded rows (flooder_padded_dim(dim) floats) in ANY order (the boxes are taken from the
 * rows as they come; curve or k-d order only makes them tight), row count rounded up to a multiple of
 * FLOODER_BVH_LEAF with +inf rows.  nodes: flooder_bvh_node_count(n_pts) x 2 x padded_dim floats (box lo then hi per
 * node). */
int flooder_bvh_build_f32(const float* pts_sorted, int64_t n_pts, int dim, float* nodes, void* stream);

/* flooder_gather_rows_f32 + flooder_bvh_build_f32 in one call: the rows are written in curve order and the leaf boxes
 * are reduced from them while they are in registers (one pass over the cloud instead of two), then the inner levels.
 * density_grid / cloud_box (both NULL, or flooder_density_grid_words(dim) ZEROED int32 and the 16-float box of
 * flooder_bbox_f32; dim 2 and 3): the same pass accumulates the density grid the cell sweep reads its first cell size
 * from (what flooder_density_grid_f32 computes from a finished tree). */
int flooder_index_rows_f32(const float* pts, int64_t n_pts, int dim, int ld, const int32_t* order, float* rows,
                           int64_t n_pad, float* nodes, int32_t* density_grid, const float* cloud_box, void* stream);

/* Sweep: out_d2[s, r] = bits(min over all points of |p(s,r) - x|^2) with p as in flooder_sweep_f32.
 * Plain stores (every cell is written exactly once); queue = FLOODER_QUEUE_WORDS zeroed int32 (sharded heads, see
 * flooder_sweep_cell_f32); stats = NULL or four
 * zeroed uint64 counters {leaves evaluated, leaves tested, inner nodes expanded, most tests by one item}. */
int flooder_sweep_bvh_f32(const float* pts_sorted, int64_t n_pts, int dim, const float* nodes,
                          const float* verts, const float* weights, int k1, int R, int64_t n_simplices,
                          int32_t* queue, uint32_t* out_d2, uint64_t* stats, void* stream);

/* Tree sweep over spatially sorted samples (default of flood_complex above 3 dimensions).  Same result in the same
 * (S, R) buffer as flooder_sweep_bvh_f32 - out_d2[s, r] = bits(min over ALL points), bit for bit - but a wave takes 64
 * consecutive samples of a Z-order of ALL (simplex, sample) pairs instead of the samples of one simplex: tight tile
 * boxes whatever the size of the simplices (coarse lattices on large simplices in 6D: 6x fewer box tests).
 *   flooder_sample_key_bits(dim)   bits of a sample key (floor(32 / dim) per axis, at most 10)
 *   flooder_sample_keys_f32        keys[s * R + r] = Morton code of sample (s, r) inside box (16 floats, [0:dim] = min,
 *                                  [8:8+dim] = max: the cloud's box from flooder_bbox_f32); n_simplices * R < 2^32 - 1
 *   (sort)                         flooder_index_sort(keys, n_simplices * R, key bits, ...) -> sample_order
 *   flooder_sweep_bvh_sorted_f32   the sweep; queue = FLOODER_QUEUE_WORDS zeroed int32; stats as flooder_sweep_bvh_f32.
 * Replaces compute_mask + nonzero + compute_filtration (core.py:210-226) like the other sweeps. */
int flooder_sample_key_bits(int dim);
int flooder_sorted_tile_samples(void);   /* samples per tile of the sorted sweep (64 x option "sorted_ks") */
int flooder_sample_keys_f32(const float* verts, const float* weights, int k1, int R, int64_t n_simplices, int dim,
                            const float* box, uint32_t* keys, void* stream);
int flooder_sweep_bvh_sorted_f32(const float* pts_sorted, int64_t n_pts, int dim, const float* nodes,
                                 const float* verts, const float* weights, int k1, int R, int64_t n_simplices,
                                 const int32_t* sample_order, int32_t* queue, uint32_t* out_d2, uint64_t* stats,
                                 void* stream);
/* The same sweep over ONE RANK'S tiles of a multi-GPU run: the contiguous run [T r / W, T (r + 1) / W) of the T tiles
 * of the sorted order - tiles of the unsharded sweep (above 3D a rank that took every W-th SIMPLEX would sweep a W times
 * thinner sample set in W^(1/dim) times wider tiles) in one region of space.  out_d2 is written for the rank's samples
 * only: zero it first, take the face maxima over all of it and combine the ranks' (S, F) values with MAX. */
int flooder_sweep_bvh_sorted_shard_f32(const float* pts_sorted, int64_t n_pts, int dim, const float* nodes,
                                       const float* verts, const float* weights, int k1, int R, int64_t n_simplices,
                                       const int32_t* sample_order, int shard_rank, int shard_world, int32_t* queue,
                                       uint32_t* out_d2, uint64_t* stats, void* stream);

/* The sorted sweep fused with the per-face maxima (core.py:251-276 folded in; the default above 3 dimensions when only
 * the face values are wanted): no (S, R) buffer.  A sample whose running minimum - the distance to a real point - does
 * not exceed the running maximum of any face it lies on (memb[r]: bit f = row r lies on face f, n_faces <= 32;
 * face_bits: n_simplices x n_faces zeroed uint32, or as many words as face_slot addresses) leaves the tile's pruning
 * radius; the samples still in the running at the end of a traversal are exact and raise face_bits (integer atomic
 * max on the d2 bits).  Values equal the exhaustive result bit for bit; flooder_face_values_f32 takes the roots.
 * flooder_sample_keys_late_f32: as flooder_sample_keys_f32, but the rows with late_rows[r] != 0 sort behind all
 * others (top key bit) - the caller marks every row except one PILOT near the centre of each face, so the face
 * maxima are close to final when the bulk of the samples is swept.  Sort over 32 key bits.  Option "sorted_refresh"
 * (4): evaluated leaves between two readings of the face maxima. */
int flooder_sample_keys_late_f32(const float* verts, const float* weights, int k1, int R, int64_t n_simplices, int dim,
                                 const float* box, const uint8_t* late_rows, uint32_t* keys, void* stream);
int flooder_sweep_bvh_sorted_faces_f32(const float* pts_sorted, int64_t n_pts, int dim, const float* nodes,
                                       const float* verts, const float* weights, int k1, int R, int64_t n_simplices,
                                       const int32_t* sample_order, int32_t* queue, const uint32_t* memb, int n_faces,
                                       uint32_t* face_bits, const int32_t* face_slot, uint64_t* stats, void* stream);

/* Same sweep restricted to an explicit work list and SEEDED with the minima already in out_d2 (upper
 * bounds from an earlier pass): item_list[i] = simplex * ceil(R/64) + tile, tiles are 64 consecutive
 * samples; *n_items (device int32) entries.  Finishes what flooder_sweep_cell_f32 could not verify.
 * budget > 0: a wave abandons a tile after that many box tests, stores its current minima and appends the
 * tile to list2 / *count2 (zeroed by the caller) - call again on list2 with budget 0, where each tile is
 * split over up to 64 waves (tiles near the medial axis of the cloud have huge candidate sets). */
int flooder_sweep_bvh_items_f32(const float* pts_sorted, int64_t n_pts, int dim, const float* nodes,
                                const float* verts, const float* weights, int k1, int R,
                                int64_t n_simplices, const int32_t* item_list, const int32_t* n_items,
                                int32_t* queue, uint32_t* out_d2, int budget, int32_t* list2,
                                int32_t* count2, uint64_t* stats, void* stream);

/* Density grid of the cloud for the cell sweep (dim 2 and 3): point counts in 64^3 (256^2) cells over the cloud's
 * box, accumulated from the leaves of the box tree (nodes: the array of flooder_index_rows_f32, leaves first).
 * grid: flooder_density_grid_words(dim) int32, ZEROED - the fine grid, then four words that flooder_cloud_kind fills. */
int64_t flooder_density_grid_words(int dim);
int flooder_density_grid_f32(const float* nodes, int64_t n_pts, int dim, const float* cloud_box, int32_t* grid,
                             void* stream);
/* What kind of cloud is it?  Pools the filled density grid into 16^3 (64^2) coarse cells and counts the points in
 * INTERIOR cells - occupied cells whose axis neighbours are all occupied: 91 - 99 % of a cloud that fills a volume
 * (Gaussian, swiss cheese, annulus in the plane), 7 - 21 % of one that lies on a surface (the noisy torus); words [2]
 * and [3] behind the fine grid.  The cell sweep reads them and tries ONE cell size per chunk instead of two on surface
 * clouds (option "cell_surface_pct", 60; 0 = never): cfg 3 3.88 -> 3.75 ms; flooder_fused_witness reads them too and
 * tries no simplex at all on such a cloud (option "wit_surface_pct", 60; 0 = always try): 3.75 -> 3.70 ms.  flooder_index_rows_f32 computes the
 * statistic itself (in spare workgroups of the launch that builds the first inner tree level; a tree of one level, at
 * most 1024 points, has no such launch and gets one for the statistic alone: the same words for every cloud size); this
 * entry point is for grids filled by flooder_density_grid_f32 (one launch; the four words must be zero).  Words [0] and
 * [1] are reserved: nothing writes them, they stay zero.
 * Without it the words stay zero and the sweep tries two sizes, as before round 6.  No result depends on it. */
int flooder_cloud_kind(int32_t* density_grid, int dim, void* stream);

/*
 * Cell sweep (dim 2 and 3; the default device path there).  One wave per chunk of 256 consecutive
 * samples of a simplex: the cloud's density inside the chunk's bounding box gives a cell size
 * c = alpha * (volume / points)^(1/dim); the points within c of the chunk are gathered through the box
 * tree and counting-sorted into a cell grid in LDS; every sample visits the 3^dim cells around it.  A
 * minimum <= (0.999 c)^2 is provably the nearest neighbour; otherwise c doubles (up to 3 rounds).  Tiles
 * of 64 samples that stay unverified or do not fit the LDS stage are appended to flag_list
 * (n_simplices * ceil(R/64) int32; *flag_count zeroed by the caller) for flooder_sweep_bvh_items_f32,
 * which finishes them exactly.  alpha > 0 only trades speed (1.35 is a good value), never correctness.
 * queue: 3 x FLOODER_QUEUE_WORDS zeroed int32 (the sharded work-queue heads of up to three launches: one returning
 * atomic on a single head word serves ~88 pops per microsecond chip-wide - half a million chunks would queue for
 * 5.7 ms - so a queue has FLOODER_QUEUE_SHARDS heads 128 B apart).  stats: NULL or nine zeroed uint64 {pairs evaluated, points staged, tiles
 * flagged, re-staging rounds, chunks given up: tree gather overflow at density / at staging, kept list
 * full, cell doublings exhausted; rounds evaluated exhaustively because the LDS stage was full}.
 * plane_scratch: 24 * n_simplices floats of device scratch (the face planes of every simplex, computed once by a
 * small kernel instead of by each of its chunks; this entry point and the positional witness / cell-face entry points
 * below each launch that kernel themselves - chained, they repeat it: same rows, same values.  Only the parameter-block
 * forms can be told that the rows are there: flooder_fused_sweep_t, planes_ready).
 * density_grid / cloud_box (both NULL, or the grid of flooder_density_grid_f32 and the 16-float box of
 * flooder_bbox_f32): with them a chunk whose box lies over well filled cells (option "cell_density_grid": at least
 * that many points in each, default 16; 0 = never) takes the local density from the grid instead of walking the tree
 * and counting the points under its box.
 */
int flooder_sweep_cell_f32(const float* pts_sorted, int64_t n_pts, int dim, const float* nodes,
                           const float* verts, const float* weights, int k1, int R, int64_t n_simplices,
                           float alpha, int32_t* queue, uint32_t* out_d2, int32_t* flag_list, int32_t* flag_count,
                           float* plane_scratch, const int32_t* density_grid, const float* cloud_box, uint64_t* stats,
                           void* stream);

/*
 * Cell sweep fused with the per-face maxima (core.py:251-276 folded into the sweep): as flooder_sweep_cell_f32 over
 * all R rows, but every sample whose nearest neighbour is settled raises face_bits[s * n_faces + f] (integer
 * atomic max on the d2 bits; zeroed by the caller) for each face f whose bit is set in memb[r] (n_faces <= 32;
 * random mode: one face, every memb word = 1).  face_slot (NULL, or n_simplices x n_faces int32): the word of
 * face_bits that face f of simplex s uses, face_slot[s * n_faces + f], so that a triangle / edge / vertex shared by
 * several simplices (its samples are bit-identical from each) has ONE running maximum.  The (S, R) buffer becomes scratch: only the tiles appended to
 * flag_list are written (bit 31 of a word = that sample is already settled), the other cells stay undefined.
 * top / top_list / top_count (all NULL, or n_simplices zeroed uint64 / n_simplices int32 / one zeroed int32): the
 * probe of the finish folded into the sweep - every flagged tile gets one greedy tree descent for its open samples
 * (finite upper bounds) while they are still in registers, and top[s] = (largest such bound << 32 | tile id).
 * defer_list / defer_c / defer_ctl (all NULL, or 5 * n_simplices * ceil(R / 256) int32 / as many float32 / eight
 * zeroed int32): three launches instead of one - first every run of four consecutive chunks (1024 samples) is
 * gathered, filtered and staged ONCE and its chunks are queried against that stage; runs that do not fit the stage and
 * chunks that keep open samples are appended to defer_list and worked off chunk by chunk by the second launch; a chunk
 * whose kept points overflow the stage there (a dense or a surface cloud) hands its open tiles of 64 samples on to
 * the third launch (entries behind the first n_simplices * ceil(R / 256) of both buffers), one sample per lane and
 * a region a quarter the size, instead of evaluating every kept point against all 256 samples - only with option
 * "cell_tiles" 1; off by default: four re-centred gathers and classifications cost more than the exhaustive loop they
 * replace (cfg 3 sweep 3.95 vs 2.55 ms).
 * simplex_weight (NULL or n_simplices floats of flooder_simplex_weight_f32) with light_list / heavy_list
 * (n_simplices int32 scratch each): simplices heavier than option "cell_super_weight" (2000) skip the first launch -
 * in a dense region no run of four chunks fits the stage - and are worked off chunk by chunk by the second.  When
 * fewer than half of the simplices are sparse (weight <= option "cell_super_sparse", 600) the first launch gets no
 * work at all and the second sweeps everything in plain order.
 * Queue order (option "cell_weight_classes", default 1): the heavy list of a long queue - and every simplex of a short
 * one (fewer than "cell_super_min_chunks" chunks: a rank's share, no runs) - is taken in descending weight class
 * (powers of two around "cell_super_weight", the given order kept inside a class), so that the densest simplices -
 * their chunks overflow the stage and keep ONE wave busy for 150 us and more - start first; the chunks the runs
 * deferred come ahead of the heavy simplices ("cell_listed_first", default 1).  A short queue is launched with one
 * workgroup per "cell_chunks_per_block" (12) chunks, at least "cell_min_grid" (384).
 * Option "cell_one_pass" (default 125, 0 = off): a chunk of the per-chunk launch whose kept points outgrow the stage
 * stops recording and evaluates them as they come, so that its candidates are streamed and classified once instead of
 * twice - unless the kept set, extrapolated from the share of the candidates seen so far, exceeds this percentage of
 * the cap ("cell_exh_dense" / "cell_exh_sparse") beyond which the chunk is left to the finish anyway.
 * flag_key / flag_hist (both NULL, or as many uint32 as flag_list holds / FLOODER_FLAG_HIST_WORDS zeroed int32; need top): the probe's
 * bound of every flagged tile, parallel to flag_list, and a histogram of the bounds' top 12 bits - with them the
 * finish works the tiles off longest search first.
 * plane_scratch: as flooder_sweep_cell_f32.
 * Followed by flooder_finish_faces_f32 (probed = 1 when top was passed here) and flooder_face_values_f32.
 */
int flooder_sweep_cell_faces_f32(const float* pts_sorted, int64_t n_pts, int dim, const float* nodes,
                                 const float* verts, const float* weights, int k1, int R, int64_t n_simplices,
                                 float alpha, int32_t* queue, uint32_t* d2_scratch, const uint32_t* memb,
                                 int n_faces, uint32_t* face_bits, const int32_t* face_slot, int32_t* flag_list,
                                 int32_t* flag_count, uint32_t* flag_key, int32_t* flag_hist, uint64_t* top,
                                 int32_t* top_list, int32_t* top_count, int32_t* defer_list,
                                 float* defer_c, int32_t* defer_ctl, const float* simplex_weight,
                                 int32_t* light_list, int32_t* heavy_list, float* plane_scratch,
                                 const int32_t* density_grid, const float* cloud_box, uint64_t* stats, void* stream);

/*
 * Witness sweep (dim 2 and 3): the sparse simplices of the fused path, a whole simplex per wave, BEFORE
 * flooder_sweep_cell_faces_f32 (same buffers; replaces compute_filtration_kernel, triton_kernels.py:12-45, and the
 * per-face amax of core.py:251-276 for those simplices).  The points around the simplex are gathered and staged once;
 * a coarse sub-lattice of its samples (coarse_rows: n_coarse <= FLOODER_WIT_MAX_COARSE row numbers padded with -1 to
 * FLOODER_WIT_MAX_COARSE entries) is evaluated first and every coarse sample keeps its witness, the point attaining
 * its minimum; every other sample takes the distance to the witnesses of four nearby coarse samples (parents[r]: four
 * coarse slots, 8 bits each; a coarse row's first parent is itself) as an upper bound, and is dropped when that bound
 * cannot raise the running maximum of any face it lies on.  What is left is evaluated against the stage; samples whose
 * nearest point may lie beyond the staged region are handed to flooder_finish_faces_f32 through flag_list / flag_key /
 * flag_hist / top (as the cell sweep's open tiles; their rows of d2_scratch hold the bound, the other rows of such a
 * tile are marked settled).  Face values are bit-identical to the exhaustive result.
 * simplex_weight (n_simplices floats of flooder_simplex_weight_f32, READ AND WRITTEN): simplices heavier than option
 * "wit_weight" (800), or whose neighbourhood does not fit one LDS stage, are left alone; a simplex handled here gets
 * weight -1, which flooder_sweep_cell_faces_f32 skips.  R <= FLOODER_WIT_MAX_ROWS.  queue: FLOODER_QUEUE_WORDS zeroed
 * int32.  item_list: n_simplices int32 of scratch (the simplices light enough, heaviest class first).  stats: NULL or 24 zeroed uint64 {simplices handled, too heavy, gather overflow, too dense for the stage,
 * points staged, coarse samples certified, samples live after the bound, evaluation rounds, samples handed to the
 * finish, tiles flagged, pairs evaluated, excess bins kept; [12:22] cycles per phase in builds with -DFLOODER_WIT_TIMERS -
 * without them [21] = runs of samples dropped by the run test (flooder_fused_witness with a run table only); [22], [23]
 * focus rounds, gather overflows in them}.  Options: "wit_cmax_pct" (250: gather radius in percent of
 * the local point spacing), "wit_min_bins" (48), "wit_grid"; "wit_sorted_stage" (1: the stage is filled in the order of
 * the excess bins, and a wave leaves a pair loop at the first bin whose points are provably farther than the running
 * minimum of every sample it holds - "pairs evaluated" counts what was actually evaluated; 0: any order, whole loops;
 * same face values either way).
 */
int flooder_wit_max_rows(void);
int flooder_wit_max_coarse(void);
int flooder_sweep_witness_f32(const float* pts_sorted, int64_t n_pts, int dim, const float* nodes, const float* verts,
                              const float* weights, int k1, int R, int64_t n_simplices, const int32_t* coarse_rows,
                              int n_coarse, const uint32_t* parents, int32_t* queue, uint32_t* d2_scratch,
                              const uint32_t* memb, int n_faces, uint32_t* face_bits, const int32_t* face_slot,
                              int32_t* flag_list, int32_t* flag_count, uint32_t* flag_key, int32_t* flag_hist,
                              uint64_t* top, int32_t* top_list, int32_t* top_count, float* simplex_weight,
                              int32_t* item_list, float* plane_scratch, uint64_t* stats, void* stream);

/*
 * Exact finish of the flagged tiles when only the face maxima are wanted.  A sample whose upper bound does not
 * exceed the running maximum of every face it lies on cannot change a result and is dropped; the others are
 * traversed exactly (box tree, nearest first) and delivered with integer atomic max.  Passes: a probe (one greedy
 * descent per tile: finite upper bounds, and per simplex the tile with the largest one; skipped when the cell sweep
 * did it), optionally ("finish_top" 1) the top tile of every simplex, then all tiles, largest bound first.  Face
 * values equal the exhaustive result bit for bit.
 *   ctl: 24 + 3 * FLOODER_QUEUE_WORDS zeroed int32 (list lengths and the team passes' queue heads, then the sharded
 *   queue heads of the per-wave passes; ctl[3] = number of entries of top_list, which the cell
 *   sweep's probe may already have filled: then probed = 1 and the probe pass is skipped); top: n_simplices uint64
 *   (zeroed unless probed); top_list: n_simplices int32;
 *   flag_key / flag_hist / flag_sorted: all NULL, or what flooder_sweep_cell_faces_f32 filled plus scratch of the
 *   size of flag_list (flag_hist: FLOODER_FLAG_HIST_WORDS zeroed int32, its second half the sort's) - a counting sort by descending bound puts the long searches first in the last pass's queue
 *   (option "finish_order" 0 turns it off);
 *   hard_scratch / hard_cap: NULL / 0, or 4 * hard_cap uint64 of scratch - a tile that has evaluated more leaves
 *   than option "finish_budget" (14; a wave raises its issue priority after 32 leaves, so a long search runs ahead of
 *   the three it shares its SIMD with) times the tiles per wave of the whole list is taken off its wave and put on a
 *   list of at most hard_cap entries; the next launch gives every such tile to a workgroup of 16 waves, each
 *   searching an interleaved share of the level-1 nodes of the box tree, the minima combined in LDS round by round
 *   (one more launch; without scratch, or with the budget 0, one wave works every tile off alone);
 *   stats: NULL or 7 zeroed uint64 {leaves evaluated, leaves tested, nodes expanded, -, tiles dropped on arrival in
 *   the last pass, samples live on arrival in the last pass, focus rounds}.
 * A list of at most flooder_finish_single_tiles() tiles first gets a launch with ONE WAVE PER SAMPLE (wave w: sample
 * w % 64 of tile flag_list[w / 64]; lanes = the child boxes of a node on the way down, then the 16 points of four
 * candidate leaves per step).  A sample that costs more than flooder_finish_single_batches() such steps writes the
 * bound it reached and is counted in ctl[8]; the passes above run behind that launch, drop what is settled and
 * search the left-overs, so the values do not depend on it.  It counts leaves, nodes and live samples in stats like
 * the passes, but no focus rounds: stats[6] = 0 with stats[0] > 0 says the short-list launch did all the work.
 * Option "bvh_subs" 1 (tiles are not split over waves) turns it off; the batch budget follows option
 * "finish_budget_min" in proportion (48 batches at its default of 64 leaves, never fewer than one).
 */
int flooder_finish_single_tiles(void);
int flooder_finish_single_batches(void);
int flooder_finish_faces_f32(const float* pts_sorted, int64_t n_pts, int dim, const float* nodes,
                             const float* verts, const float* weights, int k1, int R, int64_t n_simplices,
                             const int32_t* flag_list, const int32_t* flag_count, const uint32_t* flag_key,
                             int32_t* flag_hist, int32_t* flag_sorted, int32_t* ctl,
                             uint64_t* top, int32_t* top_list, int probed, uint32_t* d2_scratch,
                             const uint32_t* memb, int n_faces, uint32_t* face_bits, const int32_t* face_slot,
                             uint64_t* hard_scratch, int hard_cap, uint64_t* stats, void* stream);

/*
 * Control words of the fused sweep, by name (int32 word offsets; what the prose above calls ctl[3], defer_ctl + 2, ...).
 * `ctl` of flooder_finish_faces_f32 (flooder_fused_sweep_t: finish_ctl), FLOODER_FINISH_CTL_WORDS zeroed words:
 */
#define FLOODER_FINISH_CTL_PASS_HEADS 0     /* [0..2] a word per pass (probe / top / rest) kept for its head    */
#define FLOODER_FINISH_CTL_TOP_COUNT 3      /* entries of top_list (what top_count of the sweeps points at)      */
#define FLOODER_FINISH_CTL_TOP_HARD_HEAD 4  /* top pass: queue head of its hard entries ...                      */
#define FLOODER_FINISH_CTL_TOP_HARD_LEN 5   /* ... and how many it listed                                        */
#define FLOODER_FINISH_CTL_REST_HARD_HEAD 6 /* rest pass: the same two                                           */
#define FLOODER_FINISH_CTL_REST_HARD_LEN 7
#define FLOODER_FINISH_CTL_SINGLE_LEFT 8    /* samples the short-list launch left over                           */
#define FLOODER_FINISH_CTL_QUEUES 24        /* sharded heads of pass p: + p * FLOODER_QUEUE_WORDS (p = 0, 1, 2)  */
#define FLOODER_FINISH_CTL_WORDS (FLOODER_FINISH_CTL_QUEUES + 3 * FLOODER_QUEUE_WORDS)
/* flag_hist of the three launches, zeroed words: the histogram of the flagged tiles' bounds (the top 12 bits: 4096
 * buckets), then as many cursors of the finish's counting sort */
#define FLOODER_FLAG_HIST_WORDS 8192
/* defer_ctl of flooder_sweep_cell_faces_f32, FLOODER_DEFER_CTL_WORDS zeroed words: */
#define FLOODER_DEFER_CTL_COUNT 0           /* chunks on defer_list ...                                          */
#define FLOODER_DEFER_CTL_QUEUE 1           /* ... and a word kept for their queue head (popped from `queue`)    */
#define FLOODER_DEFER_CTL_LIGHT 2           /* simplices on light_list,                                          */
#define FLOODER_DEFER_CTL_HEAVY 3           /* on heavy_list,                                                    */
#define FLOODER_DEFER_CTL_SPLIT_DONE 4      /* 1 once both lists are filled                                      */
#define FLOODER_DEFER_CTL_TILE_COUNT 6      /* tiles handed to the third launch (option "cell_tiles")            */
#define FLOODER_DEFER_CTL_WORDS 8
/* queue areas: `queue` of the cell sweeps holds the heads of its three launches, FLOODER_QUEUE_WORDS each; the last word
 * of the witness sweep's one queue is the length of its item list */
#define FLOODER_CELL_QUEUE_RUNS 0
#define FLOODER_CELL_QUEUE_CHUNKS FLOODER_QUEUE_WORDS
#define FLOODER_CELL_QUEUE_TILES (2 * FLOODER_QUEUE_WORDS)
#define FLOODER_CELL_QUEUE_WORDS (3 * FLOODER_QUEUE_WORDS)
#define FLOODER_WIT_QUEUE_ITEM_COUNT (FLOODER_QUEUE_WORDS - 1)

/* out_face[i] = sqrt(float(face_bits[i])), i < n: the filtration values (core.py:257, 272: distances, not squares). */
int flooder_face_values_f32(const uint32_t* face_bits, int64_t n, float* out_face, void* stream);

/* The same for face words filled under face ownership (flooder_fused_sweep_t, face_owner), where a simplex's words hold
 * only what that simplex delivered: one thread per (simplex s, face f) writes
 *   out_face[slot[s, f]] = sqrt(max over the faces g of s inside f, f included, of face_bits[slot[s, g]]),
 * the maximum over the face's closure.  sub_faces: n_faces words, bit g of word f set when face g lies inside face f.
 * Only the raw words are read, so no order between the threads is needed; the writers of one slot write identical bits
 * (every sample of a face is delivered to that face's own word by the owner of the sample's minimal face).  Slots of no
 * (s, f) are not written: the caller zeroes out_face.  face_slot (n_simplices x n_faces, as in the sweep) is required. */
int flooder_face_closure_f32(const uint32_t* face_bits, const int32_t* face_slot, const uint32_t* sub_faces,
                             int64_t n_simplices, int n_faces, float* out_face, void* stream);

/* weight[s] = rough number of cloud points inside the bounding box of simplex s (walk of the box tree down to its
 * 1024-point nodes, overlapped volume fractions).  The host queues the simplices by descending weight: work per
 * simplex is heavy-tailed and the long ones should start first.  Replaces the sort by ball centre of core.py:174-179
 * as the work order (the order of the simplices never changes a value). */
int flooder_simplex_weight_f32(const float* nodes, int64_t n_pts, int dim, const float* verts, int k1,
                               int64_t n_simplices, float* weight, void* stream);

/* The same launch PREPARING a fused sweep: weights as above, plus (plane_scratch != NULL, dim 2 / 3) the face-plane rows
 * the witness and the cell sweep read - flooder_fused_witness / flooder_fused_cell skip their own plane launch when
 * the caller says so (flooder_fused_sweep_t, planes_ready) - plus a zero fill of zero_words int32 words at zero_buf (the control
 * words, queue heads and face words the sweep's launches start from; NULL / 0: none).  One launch instead of three
 * (fill, weights, planes): ~8 us of cfg 2's step. */
int flooder_simplex_prepare_f32(const float* nodes, int64_t n_pts, int dim, const float* verts, int k1,
                                int64_t n_simplices, float* weight, float* plane_scratch, int32_t* zero_buf,
                                int64_t zero_words, void* stream);
/* Does nothing; exported so that callers of earlier versions still link (whether the plane rows are written is the
 * caller's to say: flooder_fused_sweep_t, planes_ready). */
void flooder_simplex_planes_forget(void);

/* Test-facing probe of the witness sweep's margin arithmetic (dim 2 / 3): phase 1 of the sweep - plane rows, Region,
 * Excess, c_max = cmax_frac x the longest side of the vertices' box, bin_scale, gather box - for S simplices of dim + 1
 * vertices, then excess and bin of the points pts[pt_off[s] .. pt_off[s + 1]) of every simplex s, and for every weight
 * row (R, dim + 1) the sample, its slack and limit(slack, k / bin_scale), k = 0 .. 64.  `out` (float32 words, in this
 * order; W = (dim + 1) dim + 4 (dim + 1) + 3 dim + 2): 24 S plane rows | W S Region words | (2 dim + 3 (dim + 1)) S
 * Excess words | (2 + 2 dim) S scalars | n_points excesses | (dim + 1) R S samples and slacks | 65 R S limits.
 * `bins`: n_points int32, 64 where excess x bin_scale is not below 64.  What the words are: csrc/flood_wit.hip. */
int flooder_wit_probe_f32(const float* verts, int dim, int64_t n_simplices, float cmax_frac, const float* pts,
                          const int64_t* pt_off, int64_t n_points, const float* weights, int R, float* out, int32_t* bins,
                          void* stream);

/* Device self-test of the 64-lane DPP reductions: out128[0:64] = min(in64), out128[64:128] = max. */
int flooder_selftest(const float* in64, float* out128, void* stream);

/* Set n uint32 words to `value` (used to initialise d2 buffers to +inf bits). */
int flooder_fill_u32(uint32_t* buf, int64_t n, uint32_t value, void* stream);

/*
 * Farthest-point sampling.  Replaces fpsample.bucket_fps_kdline_sampling as called by
 * generate_landmarks (flooder/core.py:337-343): exact FPS order starting at `start`.
 *   out_idx: n_lms int64 (selection order, out_idx[0] = start);
 *   work_min: 4 * n_pts float32 scratch, 16-byte aligned (rows x, y, z, running squared distance to the
 *             selected set for dim <= 3; the first n_pts floats otherwise);
 *   work_best: 64 * n_lms uint64 scratch, zeroed by the caller (64 arg-max slots per iteration).
 */
int flooder_fps_f32(const float* pts, int64_t n_pts, int dim, int ld, int n_lms, int64_t start,
                    int64_t* out_idx, float* work_min, uint64_t* work_best, void* stream);

/*
 * ---- float64 sweep -------------------------------------------------------------------------------------------------
 * The reference's kernels are instantiated with DTYPE = fp64 for float64 inputs (triton_kernels.py:226-229).  Here:
 * the box tree of the float32-rounded cloud (flooder_bvh_build_f32) with the float64 rows gathered in the same order;
 * boxes are widened by one float32 ulp per side inside the kernel and every bound and distance is evaluated in double.
 *   flooder_gather_rows_f64: as flooder_gather_rows_f32 for double rows (padding rows +inf, padding columns 0);
 *   flooder_sweep_bvh_f64:   out_d2[s, r] = bit pattern of the double min over all points of |p(s, r) - x|^2
 *                            (non-negative doubles order like unsigned 64-bit integers); queue: FLOODER_QUEUE_WORDS zeroed int32;
 *   flooder_face_max_f64:    face maxima + sqrt in double (layout as flooder_face_max_f32).
 */
int flooder_gather_rows_f64(const double* pts, int64_t n_pts, int dim, int ld, const int32_t* order, double* out,
                            int64_t n_pad, void* stream);
int flooder_sweep_bvh_f64(const double* pts_sorted, int64_t n_pts, int dim, const float* nodes, const double* verts,
                          const double* weights, int k1, int R, int64_t n_simplices, int32_t* queue,
                          uint64_t* out_d2, void* stream);
int flooder_face_max_f64(const uint64_t* d2, int64_t n_simplices, int R, const int32_t* face_ptr,
                         const int32_t* face_rows, int n_faces, double* out_face, double* out_dist, void* stream);

/*
 * Bucketed exact farthest-point sampling (dim <= 3) over the curve-sorted copy of the cloud that the sweeps use.
 * Replaces fpsample.bucket_fps_kdline_sampling (flooder/core.py:337-343: exact FPS accelerated by kd-tree buckets):
 * buckets of 64 or 256 consecutive sorted rows carry a bounding box and their largest running minimum; a new
 * landmark only updates the buckets whose box is closer to it than that maximum.  Same selection as
 * flooder_fps_f32, bit for bit (same per-point arithmetic; ties: lowest original index).
 *   pts / ld: the cloud in its ORIGINAL order (out_idx refers to it); pts_sorted: padded rows in curve order;
 *   order: int32, order[j] = original index of sorted row j;
 *   rows: 4 * n_pts float32 scratch (16-byte aligned); bucket_box: 8 * flooder_fps_bucket_count(n_pts) float32;
 *   bucket_key: flooder_fps_bucket_count(n_pts) uint64; work_best: 64 * n_lms uint64, zeroed by the caller.
 * Options "fps_switch" (first bucketed iteration; 0 = auto) and "fps_rpl" (rows per lane and bucket: 1 or 4; 0 = auto).
 */
int64_t flooder_fps_bucket_count(int64_t n_pts);
int flooder_fps_indexed_f32(const float* pts, int64_t n_pts, int dim, int ld, const float* pts_sorted,
                            const int32_t* order, int n_lms, int64_t start, int64_t* out_idx, float* rows,
                            float* bucket_box, uint64_t* bucket_key, uint64_t* work_best, void* stream);

/* The same selection with SEVERAL landmarks per launch (default of generate_landmarks on ROCm tensors, dim <= 8).
 * FPS is sequential, but the runners-up of the arg-max stay the next landmarks as long as each is at least its own
 * running minimum away from the ones before it (flood_fps2.hip): a launch selects such a prefix (<= 8) and applies
 * all its updates at once - same indices as flooder_fps_indexed_f32 / flooder_fps_f32 in a fraction of the launches.
 * pts_sorted / order: rows of the cloud in curve order (flooder_padded_dim(dim) floats each) and the sorted row ->
 * original index map (flooder_index_rows_f32 / flooder_index_sort).  n_pts <= flooder_fps_batched_max_points().
 * Workspaces (device): minsq n_pts floats; bucket_box 2 * padded_dim * flooder_fps_bucket_count(n_pts) floats;
 * bucket_keys 3 * bucket count uint64; bucket_coord padded_dim * bucket count floats; work_best 64 * n_lms uint64,
 * ZEROED; work_rec flooder_fps_batched_rec_words(n_pts, dim, n_lms) uint32; work_ctr n_lms + 4 int32, ZEROED.
 * launches_out (host pointer, may be NULL): kernel launches used.
 * The number of launches depends on the data.  UNLIKE every other entry point this one therefore WAITS for the
 * device: every launch stores (launches done, landmarks selected) into a pinned host word (one per device, allocated
 * at first use), the host keeps 24 launches in flight beyond the last one it has seen complete and returns when the
 * word says "all selected" (the stream itself is not drained: a few no-op launches may still be queued).  Option
 * "fps_rounds" = 1 (and a host where pinned memory cannot be had): doubling rounds of launches with a read-back of
 * the landmark counter (4 bytes, hipStreamSynchronize) between rounds.  "fps_lane_best" = 1: test hook, ranks at most
 * one candidate per lane (the path more than 64 candidates take). */
int64_t flooder_fps_batched_max_points(void);
int64_t flooder_fps_batched_rec_words(int64_t n_pts, int dim, int n_lms);
int flooder_fps_batched_f32(const float* pts, int64_t n_pts, int dim, int ld, const float* pts_sorted,
                            const int32_t* order, int n_lms, int64_t start, int64_t* out_idx, float* minsq,
                            float* bucket_box, uint64_t* bucket_keys, float* bucket_coord, uint64_t* work_best,
                            uint32_t* work_rec, int32_t* work_ctr, int32_t* launches_out, void* stream);

/*
 * ---- parameter blocks ----------------------------------------------------------------------------------------------
 * The entry points of the DEFAULT path that take more than a dozen arguments also exist in a form that takes ONE
 * struct: the three launches of the fused 2-D / 3-D sweep share almost all of their buffers (flooder_fused_sweep_t,
 * filled once, passed three times), the sorted-sample sweep above 3-D and the batched landmark selection have a block
 * each.  A maintainer binds a struct field by NAME (cgo / ctypes.Structure / JNA) - a transposed pointer in a run of
 * thirty positional void* is a silently wrong answer, a misspelt field is a compile error.  Every block opens with
 * `size` (sizeof of the struct as the caller compiled it) and `abi` (FLOODER_PARAMS_ABI): a library that knows a longer
 * struct reads the fields the caller has and takes the documented default (NULL / 0) for the rest; a caller newer than
 * the library is refused (FLOODER_E_ARG).  Pointers are device pointers unless said otherwise; what every field
 * means, and which may be NULL, is documented at the positional function of the same launch.  Inside the library the
 * block IS the argument list: every launch is one function on the block, which checks the fields and fills the kernels'
 * own structs from them by name.  The forwarding runs from the positional functions to it - each copies its arguments
 * into a zeroed block, field by field, and makes the same call; they stay exported as they were (same symbols, same
 * behaviour; flooder_amd's own default path does not call them).
 */
#define FLOODER_PARAMS_ABI 1

typedef struct flooder_fused_sweep_s {
  uint32_t size, abi;
  /* the cloud and its index (flooder_index_rows_f32 / flooder_bvh_build_f32 / flooder_density_grid_f32) */
  const float* pts_sorted;
  int64_t n_pts;
  int32_t dim;
  int32_t k1;                 /* vertices per simplex */
  const float* nodes;
  const int32_t* density_grid;
  const float* cloud_box;
  /* simplices and sample lattice */
  const float* verts;
  const float* weights;
  int32_t R;
  int32_t n_faces;
  int64_t n_simplices;
  const uint32_t* memb;
  float alpha;
  int32_t n_coarse;           /* witness plan: flooder_sweep_witness_f32 */
  const int32_t* coarse_rows;
  const uint32_t* parents;
  /* result */
  uint32_t* face_bits;
  const int32_t* face_slot;
  /* scratch shared by the three launches */
  uint32_t* d2_scratch;
  int32_t* flag_list;
  int32_t* flag_count;
  uint32_t* flag_key;
  int32_t* flag_hist;         /* FLOODER_FLAG_HIST_WORDS zeroed int32 */
  int32_t* flag_sorted;
  uint64_t* top;
  int32_t* top_list;
  int32_t* top_count;
  float* simplex_weight;
  float* plane_scratch;
  /* witness sweep */
  int32_t* wit_queue;
  int32_t* wit_item_list;
  uint64_t* wit_stats;
  /* cell sweep */
  int32_t* cell_queue;
  int32_t* defer_list;
  float* defer_c;
  int32_t* defer_ctl;
  int32_t* light_list;
  int32_t* heavy_list;
  uint64_t* cell_stats;
  /* finish */
  int32_t* finish_ctl;
  uint64_t* hard_scratch;
  int32_t hard_cap;
  int32_t probed;
  uint64_t* finish_stats;
  /* witness sweep, run test (fields added behind the first release of the struct: a caller that does not have them
   * gets no run test).  wit_runs: NULL, or wit_n_runs rows of 8 words, one per aligned run of wit_run_len (a power of
   * two >= 8) consecutive rows of `weights`: {4 float centre weights (non-negative, sum 1, zero beyond k1), uint32 OR
   * of the members' words of `memb`, uint32 parent word (as `parents`), float radius: the largest 2-norm of
   * (member's weight row - centre weights), rounded up, 0}.  wit_n_runs * wit_run_len <= R (rows behind the last whole
   * run are always looked at one by one); 32-byte aligned; k1 <= 4.  Every weight row and the centre weights must sum
   * to the same value within 2^-21.  Option "wit_runs" 0 switches the test off. */
  const uint32_t* wit_runs;
  int32_t wit_run_len;
  int32_t wit_n_runs;
  /* non-zero: the caller vouches that plane_scratch already holds the plane rows of exactly these `verts` - written by
   * flooder_simplex_prepare_f32, flooder_fused_witness or flooder_fused_cell on the SAME stream, and `verts` unchanged
   * since - and flooder_fused_witness / flooder_fused_cell skip their plane-row launch.  0 (and every caller whose
   * struct ends before this field): they launch it.  The library keeps no memory of what it wrote between calls. */
  int32_t planes_ready;
  int32_t reserved;
  /* face ownership (fields added behind planes_ready: a caller that does not have them, or passes face_owner NULL, gets
   * none).  Needs face_slot with ONE slot per distinct face of the complex, built from cells with ascending vertex ids
   * (a shared face's samples then have bit-identical coordinates in every incident simplex), and simplex_weight (the
   * launch that splits the simplices by weight chooses the owners).  face_owner: one ZEROED 64-bit word per slot, 8-byte
   * aligned; flooder_fused_cell writes, per proper face, the key of the incident simplex that evaluates the face's own
   * samples - a simplex the witness sweep has handled before a lighter one before a lower row - and the cell sweep builds
   * every row whose MINIMAL face (min_face: R bytes, the face of the fewest vertices the row lies on; face 0 = the full
   * simplex, always evaluated) this simplex does not own as an absent sample.  chunk_faces / tile_faces: per aligned run
   * of 256 / 64 rows the OR of (1 << min_face) over its rows.  The face words then hold, per simplex, only what that
   * simplex delivered: read them through flooder_face_closure_f32. */
  uint64_t* face_owner;
  const uint8_t* min_face;
  const uint32_t* chunk_faces;
  const uint32_t* tile_faces;
} flooder_fused_sweep_t;

/* flooder_sweep_witness_f32, flooder_sweep_cell_faces_f32, flooder_finish_faces_f32 on the fields of *p (host memory;
 * read during the call only).  flooder_fused_witness also hands `density_grid` (may be NULL) to the witness sweep, which
 * then stands back on a cloud that lies on a surface (option "wit_surface_pct"), and the run table (wit_runs): a
 * whole run of samples is dropped with one bound - the distance of the run's centre to a parent's witness plus the
 * run's radius - where that bound cannot raise a face value; the positional function has neither argument: it always
 * tries and looks at every sample.  Face values are the same bit for bit either way.  planes_ready (see the field) is
 * likewise a field only: the positional functions always write the plane rows themselves, so a caller that chains the
 * positional witness and cell entry points pays one redundant small launch; the values are the same. */
int flooder_fused_witness(const flooder_fused_sweep_t* p, void* stream);
int flooder_fused_cell(const flooder_fused_sweep_t* p, void* stream);
int flooder_fused_finish(const flooder_fused_sweep_t* p, void* stream);

typedef struct flooder_sorted_sweep_s {   /* flooder_sweep_bvh_sorted_faces_f32 / _sorted_f32 / _sorted_shard_f32 */
  uint32_t size, abi;
  const float* pts_sorted;
  int64_t n_pts;
  int32_t dim;
  int32_t k1;
  const float* nodes;
  const float* verts;
  const float* weights;
  int32_t R;
  int32_t n_faces;
  int64_t n_simplices;
  const int32_t* sample_order;
  int32_t* queue;
  const uint32_t* memb;
  uint32_t* face_bits;
  const int32_t* face_slot;
  uint64_t* stats;
  uint32_t* out_d2;           /* flooder_sorted_minima only: the (S, R) minima */
  int32_t shard_rank;         /* flooder_sorted_minima: this rank's run of the tiles when shard_world > 1 */
  int32_t shard_world;        /* 0 or 1: all tiles */
} flooder_sorted_sweep_t;
int flooder_sorted_faces(const flooder_sorted_sweep_t* p, void* stream);    /* fused with the face maxima */
int flooder_sorted_minima(const flooder_sorted_sweep_t* p, void* stream);   /* minima into out_d2 (all tiles / a shard) */

typedef struct flooder_fps_batched_s {    /* flooder_fps_batched_f32 */
  uint32_t size, abi;
  const float* pts;
  int64_t n_pts;
  int32_t dim;
  int32_t ld;
  const float* pts_sorted;
  const int32_t* order;
  int64_t start;
  int32_t n_lms;
  int32_t reserved;
  int64_t* out_idx;
  float* minsq;
  float* bucket_box;
  uint64_t* bucket_keys;
  float* bucket_coord;
  uint64_t* work_best;
  uint32_t* work_rec;
  int32_t* work_ctr;
  int32_t* launches_out;      /* host */
} flooder_fps_batched_t;
int flooder_fps_batched(const flooder_fps_batched_t* p, void* stream);

/*
 * ---- Witnesses of the filtration values (csrc/flood_grad.hip; flooder_amd.grad) ---------------------------------
 * flooder_face_argmax_f32: over the (n_simplices x R) minimum d2 bits of an unfused sweep and the face CSR (face_rows:
 * columns of d2, each face's segment ascending), out_key[s * n_faces + f] = (max d2 bits << 32) | (0xffffffff - r)
 * with r the smallest sample row attaining it: r = row_id[c] for column c (the caller's weight-table row of a swept
 * column; NULL: r = c).
 * flooder_witness_search: per query q, p* = sum_j weights[q_row[q], j] * verts[q_simplex[q], j, :] (fma in vertex
 * order, as the sweeps), then out_point[q] = the smallest original id (order[row]) of the points at squared distance
 * with exactly the bits q_d2[q] (t0*t0, then fma(t, t, d2) over the remaining axes), -1 if none; every query without
 * a point adds 1 to *not_found (one zeroed word).
 * flooder_segment_sum_f32: out[seg_target[g], k] = sum over i in [seg_ptr[g], seg_ptr[g+1]) of vals[order[i], k], in
 * that order (deterministic; rows of out no segment targets are left as they are).
 */
int flooder_face_argmax_f32(const uint32_t* d2, int64_t n_simplices, int R, const int32_t* face_ptr,
                            const int32_t* face_rows, const int32_t* row_id, int n_faces, uint64_t* out_key,
                            void* stream);

typedef struct flooder_witness_search_s {   /* flooder_witness_search */
  uint32_t size, abi;
  const float* pts_sorted;    /* PointIndex.pts: (n_pad, DP) rows in tree order */
  int64_t n_pts;
  int32_t dim;
  int32_t k1;                 /* vertices of a swept simplex */
  const float* nodes;         /* PointIndex.nodes */
  const int32_t* order;       /* PointIndex.order32: tree row -> original id */
  const float* verts;         /* (n_simplices, k1, dim) vertex rows of the swept simplices */
  const float* weights;       /* (R, k1) the swept weight rows */
  int32_t R;
  int32_t reserved;
  int64_t n_simplices;        /* rows of verts */
  int64_t n_queries;
  const int32_t* q_simplex;   /* (n_queries,) queue position of the simplex */
  const int32_t* q_row;       /* (n_queries,) weight row */
  const uint32_t* q_d2;       /* (n_queries,) target d2 bits */
  int64_t* out_point;         /* (n_queries,) */
  int32_t* not_found;         /* one zeroed word */
} flooder_witness_search_t;
int flooder_witness_search(const flooder_witness_search_t* p, void* stream);

int flooder_segment_sum_f32(const float* vals, int dim, const int64_t* order, const int64_t* seg_ptr,
                            const int64_t* seg_target, int64_t n_seg, float* out, void* stream);

/*
 * ---- Robust filtration: the k nearest points of every sample (csrc/flood_knn.hip) --------------------------------
 * flooder_sweep_knn_f32: the tree sweep of flooder_sweep_bvh_f32 (same samples p = sum_j weights[r, j] *
 * verts[s, j, :], fma in vertex order; same squared distance t0*t0, then fma(t, t, d2); same (S, R) output buffer,
 * plain stores, every cell written once) keeping the k smallest squared distances of every sample, duplicates of a
 * point counted with their multiplicity.  out_bits[s, r] = the float32 bits of the SQUARED statistic:
 *   stat 0 ("kth")  the k-th smallest d2;
 *   stat 1 ("dtm")  the k smallest d2 added in ascending order, smallest first, by sequential float32 additions,
 *                   divided by (float)k (correctly rounded).
 * flooder_face_max_f32 takes the square roots and the face maxima.  Both are exact and independent of the tree and
 * of the order of traversal; k = 1 gives flooder_sweep_bvh_f32's words.  k in 1..FLOODER_KNN_MAX, k <= n_pts, dim in
 * 2..8.  A lane keeps its best in K vector registers, K = k rounded up to 2, 4, 8, 16 or 32 (one kernel each): the
 * insertion costs what K costs - k = 17 as much as k = 32 - and 32 is what leaves the kernel four waves per SIMD.
 * queue: FLOODER_QUEUE_WORDS zeroed int32.  stats: NULL or four zeroed uint64 {leaves evaluated, leaf tests, node
 * tests, most tests of one tile} as flooder_sweep_bvh_f32.
 */
#define FLOODER_KNN_MAX 32

typedef struct flooder_knn_sweep_s {        /* flooder_sweep_knn_f32 */
  uint32_t size, abi;
  const float* pts_sorted;    /* PointIndex.pts: (n_pad, DP) rows in tree order */
  int64_t n_pts;
  int32_t dim;
  int32_t k1;                 /* vertices of a swept simplex */
  const float* nodes;         /* PointIndex.nodes */
  const float* verts;         /* (n_simplices, k1, dim) */
  const float* weights;       /* (R, k1) */
  int32_t R;
  int32_t k;                  /* neighbours, 1..FLOODER_KNN_MAX */
  int64_t n_simplices;
  int32_t stat;               /* 0 = kth, 1 = dtm */
  int32_t reserved;
  int32_t* queue;
  uint32_t* out_bits;         /* (n_simplices, R) */
  uint64_t* stats;            /* may be NULL */
} flooder_knn_sweep_t;
int flooder_sweep_knn_f32(const flooder_knn_sweep_t* p, void* stream);

/*
 * flooder_sweep_knn_sorted_f32: flooder_sweep_knn_f32 over SORTED TILES.  A wave takes 64 consecutive entries of
 * sample_order - N = n_simplices * R ids g = s * R + r, each once, as flooder_sample_keys_f32 + flooder_index_sort
 * produce them for flooder_sorted_minima - instead of the samples of one simplex: ceil(N / 64) tiles of samples that
 * are neighbours in space whatever simplex they belong to, all 64 lanes busy.  Everything else is the kernel of
 * flooder_sweep_knn_f32 (same samples, same distances, same lists, same epilogue, same counters per tile), and
 * out_bits[s, r] receives, by a scattered 4-byte store, every cell once, the word flooder_sweep_knn_f32 writes there:
 * the k smallest of a multiset depend neither on the order of offering nor on which samples share a wave.  The order
 * is a performance input only - any permutation of 0 .. N - 1 gives the same words; an entry >= N is out of bounds.
 * Query form: k1 = 1, R = 1, weights = {1.0f} and verts = (Q, dim) query points give out_bits[q] = the squared
 * statistic of query q (flooder_amd.neighbor_distance); queries must be finite.
 * Refused (FLOODER_E_ARG) as flooder_sweep_knn_f32 refuses, and: sample_order NULL, n_simplices * R >= 2^32 - 2.
 * n_simplices == 0 or R == 0: FLOODER_OK, no pointer is looked at.
 */
typedef struct flooder_knn_sorted_s {       /* flooder_sweep_knn_sorted_f32 */
  uint32_t size, abi;
  const float* pts_sorted;    /* PointIndex.pts: (n_pad, DP) rows in tree order */
  int64_t n_pts;
  int32_t dim;
  int32_t k1;                 /* vertices of a swept simplex */
  const float* nodes;         /* PointIndex.nodes */
  const float* verts;         /* (n_simplices, k1, dim) */
  const float* weights;       /* (R, k1) */
  int32_t R;
  int32_t k;                  /* neighbours, 1..FLOODER_KNN_MAX */
  int64_t n_simplices;
  int32_t stat;               /* 0 = kth, 1 = dtm */
  int32_t reserved;
  int32_t* queue;
  uint32_t* out_bits;         /* (n_simplices, R) */
  uint64_t* stats;            /* may be NULL */
  const int32_t* sample_order;  /* N = n_simplices * R entries, as flooder_sorted_sweep_t's */
} flooder_knn_sorted_t;
int flooder_sweep_knn_sorted_f32(const flooder_knn_sorted_t* p, void* stream);

/*
 * flooder_sweep_knn_profile_f32: ONE sweep at k_max = max(col_k) that writes a plane of flooder_sweep_knn_f32's words
 * for every listed (k, stat) column (flooder_amd.flood_profile).  A lane ends a tile with its k_max smallest d2
 * ascending in registers; the first t of them are its t smallest, and the running ascending float32 sum over them is
 * the sum flooder_sweep_knn_f32 forms at k = t - so out_bits[c, s, r] equals, word for word, what
 * flooder_sweep_knn_f32 with k = col_k[c], stat = col_stat[c] writes to out_bits[s, r].  Plane c belongs to column c in
 * the caller's order; plane offsets are 64-bit.  n_cols in 1..FLOODER_KNN_COLS_MAX, col_k in 1..FLOODER_KNN_MAX,
 * col_stat 0 or 1, no (k, stat) pair twice, k_max <= n_pts, dim in 2..8.  queue and stats as flooder_sweep_knn_f32
 * (the traversal, and so the counters, are those of the single sweep at k_max).
 */
#define FLOODER_KNN_COLS_MAX 64

typedef struct flooder_knn_profile_s {      /* flooder_sweep_knn_profile_f32 */
  uint32_t size, abi;
  const float* pts_sorted;    /* PointIndex.pts: (n_pad, DP) rows in tree order */
  int64_t n_pts;
  int32_t dim;
  int32_t k1;                 /* vertices of a swept simplex */
  const float* nodes;         /* PointIndex.nodes */
  const float* verts;         /* (n_simplices, k1, dim) */
  const float* weights;       /* (R, k1) */
  int32_t R;
  int32_t n_cols;             /* columns, 1..FLOODER_KNN_COLS_MAX */
  int64_t n_simplices;
  int32_t* queue;
  uint32_t* out_bits;         /* (n_cols, n_simplices, R) */
  uint64_t* stats;            /* may be NULL */
  int32_t col_k[FLOODER_KNN_COLS_MAX];      /* neighbours of column c, 1..FLOODER_KNN_MAX */
  int32_t col_stat[FLOODER_KNN_COLS_MAX];   /* 0 = kth, 1 = dtm */
} flooder_knn_profile_t;
int flooder_sweep_knn_profile_f32(const flooder_knn_profile_t* p, void* stream);

/*
 * flooder_witness_knn (csrc/flood_grad.hip; flooder_amd.grad with neighbors > 1): the witness of a robust value.  Per
 * query q, p* = sum_j weights[q_row[q], j] * verts[q_simplex[q], j, :] (fma in vertex order, as the sweeps), then the
 * k smallest keys (d2 word, original id = order[row]) over ALL n_pts points - d2 = t0*t0, then fma(t, t, d2), a point
 * that occurs twice is two ids, rows of the padded last leaf are no candidates - are written ascending:
 * out_ids[q, 0..k) and, unless NULL, out_d2[q, 0..k).  The statistic is recomputed from the k words as
 * flooder_sweep_knn_f32 computes it (stat 0: the last word; stat 1: ascending sequential float32 sum / (float)k) and
 * compared with q_stat[q]: if the bits differ, or q_simplex / q_row is out of range, the whole row is -1 (all ones in
 * out_d2) and *not_found (one zeroed word) grows by 1.  k in 1..FLOODER_KNN_MAX, k <= n_pts <= 2^31 - 1, dim in 2..8.
 */
typedef struct flooder_witness_knn_s {      /* flooder_witness_knn */
  uint32_t size, abi;
  const float* pts_sorted;    /* PointIndex.pts */
  int64_t n_pts;
  int32_t dim;
  int32_t k1;                 /* vertices of a swept simplex */
  const float* nodes;         /* PointIndex.nodes */
  const int32_t* order;       /* PointIndex.order32: tree row -> original id */
  const float* verts;         /* (n_simplices, k1, dim) */
  const float* weights;       /* (R, k1) the swept weight rows */
  int32_t R;
  int32_t k;                  /* neighbours, 1..FLOODER_KNN_MAX */
  int64_t n_simplices;
  int64_t n_queries;
  const int32_t* q_simplex;   /* (n_queries,) queue position of the simplex */
  const int32_t* q_row;       /* (n_queries,) weight row */
  const uint32_t* q_stat;     /* (n_queries,) bits of the squared statistic, as flooder_sweep_knn_f32 wrote them */
  int64_t* out_ids;           /* (n_queries, k) */
  uint32_t* out_d2;           /* (n_queries, k); may be NULL */
  int32_t* not_found;         /* one zeroed word */
  int32_t stat;               /* 0 = kth, 1 = dtm */
  int32_t reserved;
} flooder_witness_knn_t;
int flooder_witness_knn(const flooder_witness_knn_t* p, void* stream);

/*
 * flooder_knn_ids_sorted_f32 (csrc/flood_knn.hip; flooder_amd.nearest_neighbors, the backward of neighbor_distance):
 * flooder_sweep_knn_sorted_f32 keeping KEYS - WHICH points the k nearest of every sample are.  Per cell g = s * R + r
 * (N = n_simplices * R of them, rows in cell order whatever sample_order says) the k smallest keys (d2 word, original
 * id = order[row]) over ALL n_pts points, d2 = t0*t0, then fma(t, t, d2) as every sweep, are written ascending:
 * out_ids[g, 0..k) and, unless NULL, out_d2[g, 0..k).  This is flooder_witness_knn's rule and its output word for word
 * (ids as int32 here): a point that occurs twice is two ids, among equidistant points the smaller id comes first, rows
 * of the padded last leaf are no candidates and order is never read there.  Unless NULL, out_bits[g] receives the word
 * flooder_sweep_knn_sorted_f32 writes for `stat`, formed from the k d2 words by the same arithmetic (stat 0: the last
 * word; stat 1: ascending sequential float32 sum / (float)k).  Every output word is written once, by plain stores (16
 * bytes at a time when k is a multiple of 4 and out_ids / out_d2 are 16-byte aligned); no atomics.
 * One query per lane over tiles of 64 consecutive entries of sample_order, the list in K (d2 word, id) register pairs, K
 * as flooder_sweep_knn_f32.  Ties decide which ids are reported, so unlike the value sweeps every cull is STRICT: a node,
 * a leaf or a point is skipped only when its lower bound (times the safety margin) is strictly above the k-th d2 it is
 * compared with - every point skipped has a larger d2 and so a larger key whatever its id, and keys being distinct the k
 * smallest are one set, independent of the tree and of the order of traversal.  Visited children carry a mark of their
 * own, not a bound of +inf, so the walk ends (each step closes a child or leaves a level) even at k == n_pts, where no
 * list is full before the tree is exhausted and nothing is ever culled.
 * Query form as flooder_sweep_knn_sorted_f32 (k1 = 1, R = 1, weights = {1.0f}, verts = the queries).
 * Refused (FLOODER_E_ARG) as flooder_sweep_knn_sorted_f32 refuses (out_bits may be NULL here), and: order NULL, out_ids
 * NULL, n_pts > 2^31 - 1.  n_simplices == 0 or R == 0: FLOODER_OK, no pointer is looked at.
 */
typedef struct flooder_knn_ids_s {          /* flooder_knn_ids_sorted_f32 */
  uint32_t size, abi;
  const float* pts_sorted;    /* PointIndex.pts: (n_pad, DP) rows in tree order */
  int64_t n_pts;
  int32_t dim;
  int32_t k1;                 /* vertices of a swept simplex */
  const float* nodes;         /* PointIndex.nodes */
  const float* verts;         /* (n_simplices, k1, dim) */
  const float* weights;       /* (R, k1) */
  int32_t R;
  int32_t k;                  /* neighbours, 1..FLOODER_KNN_MAX */
  int64_t n_simplices;
  int32_t stat;               /* 0 = kth, 1 = dtm: the statistic of out_bits */
  int32_t reserved;
  int32_t* queue;
  uint32_t* out_bits;         /* (n_simplices, R); may be NULL */
  uint64_t* stats;            /* may be NULL */
  const int32_t* sample_order;  /* N = n_simplices * R entries, as flooder_sorted_sweep_t's */
  const int32_t* order;       /* PointIndex.order32: tree row -> original id */
  int32_t* out_ids;           /* (N, k) */
  uint32_t* out_d2;           /* (N, k); may be NULL */
} flooder_knn_ids_t;
int flooder_knn_ids_sorted_f32(const flooder_knn_ids_t* p, void* stream);

/*
 * flooder_knn_merge_f32 (csrc/flood_knn_merge.hip; flood_complex(neighbor_reduce_hook=...), the robust filtration over
 * point shards): the exact k-best merge.  lists holds, for each of n_cells = S * R cells, n_lists ascending lists of k
 * float32 bit patterns - (n_lists, k, n_cells) int32, cell index contiguous: list w is the (k, S, R) plane buffer that
 * flooder_sweep_knn_profile_f32 with the columns (1, "kth") .. (k, "kth") writes for shard w, a list of a shard with
 * fewer than k points ending in +inf words (0x7f800000).  out_bits[cell] = the word flooder_sweep_knn_f32 writes for
 * the union of the shards:
 *   stat 0 ("kth")  the k-th smallest of the n_lists * k words of the cell;
 *   stat 1 ("dtm")  the k smallest added in ascending order, smallest first, by sequential float32 additions, divided
 *                   by (float)k (correctly rounded) - the arithmetic of the sweep's own epilogue.
 * Exact: a point among the k nearest of a sample over the whole cloud is among the k nearest of its shard, so the
 * union of the lists contains the global list as a multiset; only values are merged, so ties and doubled points need
 * no rule and the order of the lists does not matter.  One lane per cell, the running list in K registers (K = k
 * rounded up to 2, 4, 8, 16 or 32) as the sweep keeps it; no atomics, no LDS, every output word written once; plane
 * offsets are 64-bit.  n_lists >= 1, k in 1..FLOODER_KNN_MAX, 0 <= n_cells <= 2^32 - 256.
 */
typedef struct flooder_knn_merge_s {        /* flooder_knn_merge_f32 */
  uint32_t size, abi;
  const int32_t* lists;       /* (n_lists, k, n_cells) */
  int64_t n_cells;            /* S * R */
  int32_t n_lists;            /* W: shards, >= 1 */
  int32_t k;                  /* neighbours, 1..FLOODER_KNN_MAX */
  int32_t stat;               /* 0 = kth, 1 = dtm */
  int32_t reserved;
  uint32_t* out_bits;         /* (n_cells,) */
} flooder_knn_merge_t;
int flooder_knn_merge_f32(const flooder_knn_merge_t* p, void* stream);

/*
 * flooder_knn_wide_f32 (csrc/flood_knn_wide.hip; flood_complex(neighbor_mass=m), flooder_amd.distance_to_measure): the k
 * nearest points of every cell for k up to FLOODER_KNN_WIDE_MAX, one WAVE per cell, the list in LDS - the robust
 * filtration by mass, where k = mass * n_pts runs into the hundreds.  FLOODER_KNN_MAX and the entries above are
 * untouched.  Per cell g = s * R + r (N = n_simplices * R of them) the sample p = sum_j weights[r, j] * verts[s, j, :]
 * (p = 0, then p[c] = fma(w_j, v_j[c], p[c]) in vertex order, as every sweep), d2 = t0*t0, then fma(t, t, d2) per further
 * axis, and the k smallest keys (d2 word, original id = order[row]) over ALL n_pts points, ascending: the rule of
 * flooder_witness_knn and flooder_knn_ids_sorted_f32 word for word - a point that occurs twice is two ids, among equal
 * d2 words the smaller id comes first (the k-th place included), rows of the padded last leaf are no candidates, every
 * cull is strict (a node or leaf is skipped only when lb * SAFE > the current k-th d2; nothing before the list holds k
 * keys), and k == n_pts works (nothing is culled, the walk ends with the tree).  Unless NULL:
 *   out_ids[g, 0..k)   the ids (int32), ascending by key; needs order;
 *   out_d2[g, 0..k)    their d2 words w_0 <= w_1 <= ... <= w_(k-1);
 *   out_bits[g]        the float32 bits of the SQUARED statistic of those words:
 *     stat 0 ("kth")   w_(k-1);
 *     stat 1 ("dtm")   a sum fixed by the sorted words alone.  With L = min(k, 64): for l = 0 .. L-1 the partial sum
 *                      S_l = w_l + w_(l+64) + w_(l+128) + ... over the positions < k, added left to right in float32
 *                      (S_l starts AS w_l, not as 0 + w_l); then T = S_0 + S_1 + ... + S_(L-1), added left to right in
 *                      float32 (T starts as S_0); the word is T / (float)k, correctly rounded.  For k <= 64 every S_l
 *                      is w_l and T is the plain ascending sequential sum: at k <= FLOODER_KNN_MAX the word of
 *                      flooder_sweep_knn_f32 and flooder_knn_ids_sorted_f32, bit for bit.  Above 64 it costs k / 64
 *                      additions per lane and 64 serial ones instead of k serial ones; its rounding error is at most
 *                      (ceil(k / 64) - 1 + 63) half-ulps, below 78 * 2^-24 relative on the squared value at k = 1024.
 * At least one of the three must be given.  sample_order: NULL = cells in the order g = 0 .. N-1, else a permutation of
 * 0 .. N-1 (as flooder_sweep_knn_sorted_f32 takes it) that decides only WHEN a cell is computed - neighbouring cells
 * walk the same part of the tree -, never what is written or where; an entry >= N is skipped.  order may be NULL when
 * out_ids is: equal d2 words are then ordered by tree row, which changes no d2 word and no statistic.
 * Query form: k1 = 1, R = 1, weights = {1.0f}, verts = (Q, dim) query points; queries must be finite.
 * No work queue (a grid-stride loop over the cells), no atomics, every output word written once by plain stores.
 * Refused (FLOODER_E_ARG, the message opens with the entry's name), all before a pointer is read: a bad block size or
 * abi; k outside 1..FLOODER_KNN_WIDE_MAX; dim outside 2..8; stat not 0 or 1; n_pts < k; n_pts > 2^31 - 1;
 * n_simplices * R >= 2^32 - 2; a cloud too large for the stack encoding (as flooder_witness_knn); all three outputs
 * NULL; out_ids without order.  Then n_simplices == 0 or R == 0: FLOODER_OK, nothing is touched.
 */
#define FLOODER_KNN_WIDE_MAX 1024

typedef struct flooder_knn_wide_s {         /* flooder_knn_wide_f32 */
  uint32_t size, abi;
  const float* pts_sorted;    /* PointIndex.pts: (n_pad, DP) rows in tree order */
  int64_t n_pts;
  int32_t dim;
  int32_t k1;                 /* vertices of a swept simplex */
  const float* nodes;         /* PointIndex.nodes */
  const float* verts;         /* (n_simplices, k1, dim) */
  const float* weights;       /* (R, k1) */
  int32_t R;
  int32_t k;                  /* neighbours, 1..FLOODER_KNN_WIDE_MAX */
  int64_t n_simplices;
  int32_t stat;               /* 0 = kth, 1 = dtm: the statistic of out_bits */
  int32_t reserved;
  const int32_t* order;       /* PointIndex.order32: tree row -> original id; may be NULL when out_ids is */
  const int32_t* sample_order;  /* N = n_simplices * R entries; may be NULL */
  uint32_t* out_bits;         /* (n_simplices, R); may be NULL */
  int32_t* out_ids;           /* (N, k); may be NULL */
  uint32_t* out_d2;           /* (N, k); may be NULL */
} flooder_knn_wide_t;
int flooder_knn_wide_f32(const flooder_knn_wide_t* p, void* stream);

/*
 * flooder_knn_wide_profile_f32: ONE walk of flooder_knn_wide_f32 at k = max(col_k) that writes a plane of its
 * statistic words for every listed (k, stat) column (flooder_amd.distance_to_measure_profile).  A wave ends a cell with
 * the k smallest keys ascending in LDS; the first t of them are the t smallest keys, and both statistics are fixed by
 * the sorted words alone - so
 *   out_bits[c * plane_stride + g]
 * equals, word for word, what flooder_knn_wide_f32 with k = col_k[c], stat = col_stat[c] writes to out_bits[g] (stat 1:
 * the strided sum over the positions < col_k[c] with L = min(col_k[c], 64), then / (float)col_k[c]).  The block is that
 * of flooder_knn_wide_f32 (the form of flooder_sweep_power_f32: an existing block plus what the entry adds); its k is
 * max(col_k), its stat is not used (the columns carry theirs) and must still be 0 or 1.  col_k and col_stat are HOST
 * arrays of n_cols int32 each, read before the launch and not kept.  plane_stride counts words and is at least
 * n_simplices * R: a driver that works in groups of cells hands over a slice of a (n_cols, Q) buffer, whose planes are
 * Q words apart; the words between the planes are never touched.  The traversal, the insertion, sample_order, order,
 * out_ids and out_d2 (rows of k = max(col_k) entries, both optional) are those of flooder_knn_wide_f32; the list
 * capacity is chosen from k.
 * Refused (FLOODER_E_ARG, the message opens with the entry's name), all before a device pointer is read: what
 * flooder_knn_wide_f32 refuses (all three outputs NULL included), and: n_cols outside 1..FLOODER_KNN_COLS_MAX; col_k or
 * col_stat NULL; a col_k outside 1..k; a col_stat that is not 0 or 1; a (k, stat) pair listed twice; k != max(col_k);
 * plane_stride < n_simplices * R.  Then n_simplices == 0 or R == 0: FLOODER_OK, nothing is touched.
 */
int flooder_knn_wide_profile_f32(const flooder_knn_wide_t* p, int n_cols, const int32_t* col_k, const int32_t* col_stat,
                                 int64_t plane_stride, void* stream);

/*
 * flooder_knn_mass_f32 (csrc/flood_knn_mass.hip; flooder_amd.distance_to_weighted_measure): the distance to a WEIGHTED
 * measure sum_i mu_i delta_(x_i), mu_i = masses[i] >= 0 - the nearest sites of every cell up to the one at which their
 * cumulative mass reaches tau = *target, however many that are, one WAVE per cell, the list in LDS.  The number of
 * neighbours differs from cell to cell; a site that stands for 20 points makes its list entry count 20-fold, so a mass
 * that is thousands of POINTS is tens of SITES.  flooder_knn_wide_f32 and its translation unit are untouched.
 * Rule.  Per cell g = s * R + r the sample p, the d2 words and the keys (d2 word, id = order[row]) are those of
 * flooder_knn_wide_f32, ascending: (w_0, id_0) < (w_1, id_1) < ...  M_j = mu_(id_0) + ... + mu_(id_j) in float64 and j*
 * is the first position with M_j* >= tau (the "crossing"; ">=": a prefix sum that EQUALS tau crosses there).  Sites of
 * mass 0 are listed and counted but add nothing.  The list has the length L = min(C, n_pts), C = capacity rounded up to
 * 64, 128, 256, 512 or 1024 (n_pts < C is legal).  If the L smallest keys of the whole cloud do not reach tau the cell
 * is NOT REACHED.  Unless NULL:
 *   out_count[g]         j* + 1 (int32); not reached: L;
 *   out_ids[g, 0..ld_out)  the ids of the first min(count, ld_out) keys, then -1; needs order;
 *   out_d2[g, 0..ld_out)   their d2 words, then the word of +inf (0x7f800000);
 *   out_bits[g]          the float32 bits of the SQUARED statistic; not reached: the word of +inf;
 *     stat 0 ("kth")     w_j*: the squared radius at which the ball around p holds the mass tau;
 *     stat 1 ("dtm")     ( sum_(i < j*) mu_i w_i + (tau - M_(j*-1)) w_j* ) / tau, computed as: the terms t_i = mu_i * w_i
 *                        (i < j*) and t_j* = rho * w_j* with rho = (float)(tau - M_(j*-1)) (the subtraction in double,
 *                        M_(-1) = 0), each ONE float32 product; the terms are added in the strided order of
 *                        flooder_knn_wide_f32's stat 1 over kk = j* + 1 positions (S_l = t_l + t_(l+64) + ..., then
 *                        S_0 + S_1 + ... + S_(min(kk,64)-1), both left to right in float32, each starting AS its first
 *                        term, no fused multiply-add); the word is that sum / (float)tau, correctly rounded.
 *                        All terms are >= 0, so the roundings add up: one per product, ceil(kk / 64) - 1 + 63 on
 *                        the longest chain of additions, one for rho, one for (float)tau, one for the division -
 *                        ceil(kk / 64) + 66 roundings of 2^-24 each; with the second-order terms and the float64
 *                        roundings of M the word is within (ceil(kk / 64) + 67) * 2^-24 relative of the real-number
 *                        value of the rule for the float32 masses and d2 words given (83 * 2^-24 at kk = 1024).
 * With masses all 1.0f and an integer tau = k <= L every product is exact, rho = 1 and (float)tau = (float)k: out_bits,
 * out_ids[:, :k] and out_d2[:, :k] are those of flooder_knn_wide_f32 at k, word for word, and the count is k.
 * The crossing position is exact whenever the prefix sums are exactly representable in float64 - for every order of
 * addition when the masses are integers with a total below 2^53 (a coreset's counts).  For other masses the order of
 * the float64 additions is fixed (a scan over the 64 positions of a row, plus the carry of the rows before), so the
 * result is the same run to run; where it is ambiguous which of two neighbouring positions crosses, rho is about 0 and
 * both readings give the same value up to rounding.  tau is read on the device (one float64): the caller forms
 * mass * sum(mu) there and nothing synchronises with the host; tau > 0 and finite, masses >= 0 and finite are the
 * caller's contract (a tau that is not positive crosses at position 0, a NaN is not reached; nothing is read or written
 * out of bounds either way).  masses is indexed by the key's id: the original id with order, the tree row when order is
 * NULL.  sample_order, order, the query form (k1 = R = 1) and the walk are those of flooder_knn_wide_f32; the cull bound
 * is the crossing key while the list has one, else its L-th key (csrc/flood_knn_mass.hip has the exactness argument).
 * No work queue, no atomics, every output word written once by plain stores.
 * Arguments: the block of flooder_knn_wide_f32 (the form of flooder_knn_wide_profile_f32 and flooder_sweep_power_f32:
 * an existing block plus what the entry adds - the header keeps its eleven blocks).  Its k is the CAPACITY, the list
 * entries wanted, 1..FLOODER_KNN_WIDE_MAX, rounded up to C; its stat, order, sample_order, out_bits, out_ids and out_d2
 * are as there, rows of out_ids / out_d2 having ld_out entries.  Then: masses ((n_pts,) float32 mu >= 0, indexed by id),
 * target (DEVICE pointer to one float64, tau), ld_out (entries of a row of out_ids / out_d2, 1..C; not looked at when
 * both are NULL), out_count ((N,) int32; may be NULL).
 * Refused (FLOODER_E_ARG, the message opens with the entry's name), all before a device pointer is read: a bad block
 * size or abi; capacity (the block's k) outside 1..FLOODER_KNN_WIDE_MAX; dim outside 2..8; stat not 0 or 1; n_pts < 1; n_pts > 2^31 - 1;
 * n_simplices * R >= 2^32 - 2; a cloud too large for the stack encoding; all four outputs NULL; out_ids without order;
 * with out_ids or out_d2, ld_out outside 1..C; masses or target NULL.  Then n_simplices == 0 or R == 0: FLOODER_OK,
 * nothing is touched.
 */
int flooder_knn_mass_f32(const flooder_knn_wide_t* p, const float* masses, const double* target, int32_t ld_out,
                         int32_t* out_count, void* stream);

/*
 * flooder_knn_mass_profile_f32: ONE walk of flooder_knn_mass_f32 at tau_max = max(targets[0..n_cols)) that writes a
 * plane of statistic words and a plane of counts for every listed (tau_c, stat_c) column
 * (flooder_amd.distance_to_weighted_measure_profile).  A wave ends a cell with every key of the cloud up to the
 * crossing of tau_max, ascending; the crossing of a smaller target lies in that list, and the cumulative mass AT a place
 * is a function of the places up to it alone (the scan of a row of 64 plus the carry of the rows in front) - so
 *   out_bits[c * plane_stride + g]   and   out_count[c * plane_stride + g]
 * equal, word for word, what flooder_knn_mass_f32 with *target = targets[c], stat = col_stat[c] and the same capacity
 * writes to out_bits[g] and out_count[g] (rho_c = (float)(tau_c - M_(j_c - 1)), the sum divided by (float)tau_c;
 * csrc/flood_knn_mass.hip, (5), has the argument).  A column that is not reached in a list that was never cut has the
 * word of +inf and the count L; the smaller columns of such a cell are still those of their single calls.  For masses
 * that are no integers a column whose prefix sums round to just below tau_c in a list that WAS cut takes the last
 * place, as the single entry does; such a crossing is ambiguous (rho about 0) and the single call may read it at the
 * neighbouring place.  tau_max is formed on the device by every wave; nothing is read back to the host.
 * Arguments: the block of flooder_knn_wide_f32 as flooder_knn_mass_f32 takes it (its k is the CAPACITY; its stat is not
 * used - the columns carry theirs - and must still be 0 or 1; its out_bits is the plane buffer; out_ids and out_d2 must
 * be NULL: lists are per target).  Then: masses as there; n_cols in 1..FLOODER_KNN_COLS_MAX; targets, a DEVICE array of
 * n_cols float64 (tau_c > 0 and finite are the caller's contract); col_stat, a HOST array of n_cols int32 read before
 * the launch and not kept; plane_stride, in words, at least n_simplices * R (a driver that works in groups of cells
 * hands over a slice of a (n_cols, Q) buffer: the words between and behind the planes are never touched); out_count, the
 * planes of counts with the same stride, may be NULL.  Two columns with the same target and stat are legal (the targets
 * live on the device: the host cannot compare them).
 * Refused (FLOODER_E_ARG, the message opens with the entry's name), all before a device pointer is read: a bad block
 * size or abi; n_cols outside 1..FLOODER_KNN_COLS_MAX; targets or col_stat NULL; a col_stat that is not 0 or 1; what
 * flooder_knn_mass_f32 refuses of capacity, dim, stat, n_pts, n_simplices * R and the stack encoding; out_ids or out_d2
 * not NULL; out_bits NULL; masses NULL; plane_stride < n_simplices * R.  Then n_simplices == 0 or R == 0: FLOODER_OK,
 * nothing is touched.
 */
int flooder_knn_mass_profile_f32(const flooder_knn_wide_t* p, const float* masses, int n_cols, const double* targets,
                                 const int32_t* col_stat, int64_t plane_stride, int32_t* out_count, void* stream);

/*
 * ---- Weighted filtration: the power distance (csrc/flood_power.hip; flood_complex(point_weights=w)) ----------------
 * Every point x carries a weight w_x >= 0 and a sample p is measured by f(p)^2 = min_x ( |p - x|^2 + w_x^2 ).
 *
 * flooder_node_min_f32: the minimum of one value per tree row over every node of the box tree.
 *   leaf_vals  (n_pad,) values in tree-row order, n_pad = n_pts rounded up to FLOODER_BVH_LEAF; the rows of the padded
 *              last leaf hold +inf.
 *   node_min   flooder_bvh_node_count of n_pts floats in the layout of PointIndex.nodes: leaves first, then one level
 *              per factor FLOODER_BVH_FANOUT, every level padded to a multiple of 64 slots.  Level 0 = the minimum over a
 *              leaf's 16 rows, level l = the minimum over the up-to-64 children; padding slots receive +inf.
 * One launch per level, plain vector stores, no atomics.  Refused: a NULL pointer, n_pts < 1.
 *
 * flooder_sweep_power_f32: the tree sweep of flooder_sweep_knn_sorted_f32 at k = 1 with the word of a pair
 *     fmaf(w, w, d2),   d2 = t0*t0, then fma(t, t, d2) per further axis (t = p - x), w the weight ITSELF (not w^2),
 * and out_bits[s, r] = the float32 bits of the minimum of that word over ALL n_pts points (squared, non-negative:
 * integer order == value order; flooder_face_max_f32 takes the roots and the face maxima unchanged).  The block is
 * that of the sorted k-nearest sweep: k must be 1, stat 0, reserved 0; sample_order NULL = the identity order
 * g = 0 .. N - 1, cut into tiles simplex by simplex (64 consecutive rows of one simplex share a wave, as in
 * flooder_sweep_knn_f32), else any permutation of it in tiles of 64 consecutive entries (a performance input only:
 * the same words).
 *   w_sorted   (n_pad,) |w| in tree-row order (w gathered by PointIndex.order32), pad rows +inf;
 *   node_w     flooder_node_min_f32 of w_sorted.
 * A child of the walk is worth fmaf(node_w[c], node_w[c], gap2 of its box to the tile's box), a leaf against a lane's
 * own sample fmaf(node_w[leaf], node_w[leaf], gap2 of the sample to its box): lower bounds of every pair word below
 * the node, culled only when !(lb * SAFE < bound) as in every tree sweep - so the words do not depend on the tree, on
 * the order or on which samples share a wave.  Zero weights give the words of the k = 1 sweeps.  Weights must be
 * finite (not checked).  queue: FLOODER_QUEUE_WORDS zeroed int32; stats as flooder_sweep_knn_f32.
 * Refused (FLOODER_E_ARG, the message opens with the entry's name), before a pointer is read: a bad block size or
 * abi; k != 1; dim outside 2..8; stat != 0; reserved != 0.  Then n_simplices == 0 or R == 0: FLOODER_OK, nothing is
 * touched.  Then: a NULL pointer (w_sorted and node_w included; sample_order and stats may be NULL), n_pts < 1, k1,
 * n_simplices * R >= 2^32 - 2.
 *
 * flooder_witness_power: WHICH point attains a power word (power_filtration, power_nearest).  The block and its
 * meaning are flooder_witness_search's, with q_d2[q] = the target POWER word - the bits flooder_sweep_power_f32 wrote
 * for the sample (q_simplex[q], q_row[q]) - and w_sorted, node_w as above.  out_point[q] = the smallest original id
 * (order[row]) among the points whose word fmaf(w, w, d2) has exactly the target bits, -1 if there is none or if
 * (q_simplex[q], q_row[q]) is no swept sample; each such query adds 1 to *not_found (one zeroed word, the only atomic).
 * One wave per query walks the box tree with a stack of sibling groups; a node is opened iff
 * fmaf(node_w[node], node_w[node], gap2 of p* to its box) * SAFE <= target (non-strict), the sweep's leaf bound: a
 * skipped node holds no point at the target.  Zero weights: the outputs of flooder_witness_search on the same block.
 * Refused (FLOODER_E_ARG), the outputs untouched: a bad block size or abi; then n_queries == 0 is FLOODER_OK; then a
 * NULL pointer (w_sorted and node_w included), dim outside 2..8, n_pts < 1 or above 2^31 - 1, k1 < 1, R < 1.
 */
int flooder_witness_power(const flooder_witness_search_t* p, const float* w_sorted, const float* node_w, void* stream);
int flooder_node_min_f32(const float* leaf_vals, int64_t n_pts, float* node_min, void* stream);
int flooder_sweep_power_f32(const flooder_knn_sorted_t* p, const float* w_sorted, const float* node_w, void* stream);

/*
 * The same sweep for several weight vectors in ONE walk of the tree (flooder_amd.power_profile, dtm_profile).
 *
 * flooder_node_min_cols_f32: flooder_node_min_f32 for nc interleaved columns, nc in 1..FLOODER_POWER_COLS_MAX.
 *   leaf_vals  (n_pad, nc): the nc values of a tree row are contiguous; the rows of the padded last leaf hold +inf.
 *   node_min   (flooder_bvh_node_count of n_pts, nc): node_min[node * nc + c] is what flooder_node_min_f32 writes to
 *              node_min[node] for column c, padding slots +inf.
 * One launch per level, plain vector stores, no atomics.  Refused: a NULL pointer, n_pts < 1, nc out of range.
 *
 * flooder_sweep_power_profile_f32: the block is that of flooder_sweep_power_f32 (k 1, stat 0, reserved 0), out_bits
 * holds n_cols planes (n_cols, n_simplices, R) with 64-bit plane offsets, and out_bits[c, s, r] equals, word for word,
 * what flooder_sweep_power_f32 writes to out_bits[s, r] with column c of the weights, for any tree, sample order (NULL
 * and sorted, as there) and tile company.  NC = n_cols rounded up to 1, 2, 4 or 8 is the row length of both arrays:
 *   w_cols       (n_pad, NC): |w| of column c of tree row i at w_cols[i * NC + c], pad rows +inf;
 *   node_w_cols  flooder_node_min_cols_f32 of w_cols with nc = NC.
 * The columns c >= n_cols are padding: they enter no test and no plane is written for them, whatever they hold.  Per
 * pair one squared distance and per column one fmaf(w_c, w_c, d2) and one minimum; per child and per leaf one gap and
 * per column one bound fmaf(nw_c, nw_c, gap2).  A child, a leaf or a level is skipped only when the test of
 * flooder_sweep_power_f32, !(lb_c * SAFE < bound_c), fails in EVERY column c < n_cols - a minimum does not depend on
 * which further points it was offered, so a column that is shown points it would have culled alone keeps its word.
 * queue and stats as flooder_sweep_power_f32 (the counters are those of the one walk).
 * Refused (FLOODER_E_ARG, the message opens with the entry's name), before a pointer is read: a bad block size or abi;
 * n_cols outside 1..FLOODER_POWER_COLS_MAX; k != 1; dim outside 2..8; stat != 0; reserved != 0.  Then n_simplices == 0
 * or R == 0: FLOODER_OK, nothing is touched.  Then: a NULL pointer (w_cols and node_w_cols included; sample_order and
 * stats may be NULL), n_pts < 1, k1, n_simplices * R >= 2^32 - 2.
 */
#define FLOODER_POWER_COLS_MAX 8

int flooder_node_min_cols_f32(const float* leaf_vals, int64_t n_pts, int nc, float* node_min, void* stream);
int flooder_sweep_power_profile_f32(const flooder_knn_sorted_t* p, int n_cols, const float* w_cols,
                                    const float* node_w_cols, void* stream);

/*
 * ---- Backward of the distance to a measure (csrc/flood_dtm_grad.hip; distance_to_measure(differentiable=True)) -----
 * Per query q the value of flooder_knn_wide_f32 depends on the m listed neighbours x_(i) = points[ids[q, i]] (m = k for
 * "dtm"; m = 1, the column k - 1, for "kth") through the differences q - x_(i), each with the coefficient coef[q] the
 * caller forms (grad_out / (f m), 0 where f = 0; grad_out * 2 / m for the squared value).  points (n_points, dim) and
 * queries (n_queries, dim) are the caller's contiguous float32 rows in input order: no tree, and no contribution is
 * ever stored.  No atomics; plain vector loads and stores; every output word is written once per launch.
 *
 * flooder_dtm_grad_queries_f32: out_q[q, c] = coef[q] * sum_i (queries[q, c] - points[ids[q * ld_ids + i], c]) over
 * i = 0 .. m - 1 (ld_ids >= m: the row stride of ids in words; "kth" passes ids + k - 1, ld_ids = k, m = 1).  One wave
 * per query.  Order of the sum, a function of m and the 64 lanes alone: lane l adds the differences of the positions
 * l, l + 64, l + 128, ... < m, left to right, to a partial sum that starts as +0; the 64 partial sums a_0 .. a_63 (+0
 * in the lanes >= m) are added in a butterfly, a_l = a_l + a_(l ^ s) for s = 32, 16, 8, 4, 2, 1 in turn (addition
 * commutes: every lane holds the same word); the product with coef[q] comes last.  An id outside 0 .. n_points - 1 is
 * not read and adds nothing.
 *
 * flooder_dtm_grad_points_f32: the transpose.  entries: (seg_ptr[n_seg],) int64, the list of all (target, query row)
 * pairs sorted by target and, inside a target, ascending by query row; of each entry the LOW 32 bits are read, the
 * query row (so the sorted packed keys (target << 32) | query row serve as they are).  Segment g = the entries
 * [seg_ptr[g], seg_ptr[g + 1]) and belongs to the row j = seg_target[g] of points (seg_target NULL: j = g; the targets
 * of one launch are distinct).  Thread (g, c) starts from the word already in out_p[j, c] and takes its entries front
 * to back: acc = fma(-coef[q], queries[q, c] - points[j, c], acc), one rounding for the difference and one for the
 * step; then out_p[j, c] = acc.  So launches over consecutive groups of ascending query rows (queries, coef and the
 * entries' rows relative to the group's first row) continue one sequential sum per (target, axis): the result does not
 * depend on the groups, bit for bit - the rule of flooder_segment_sum_f32, continued across launches.  Rows of out_p
 * without a non-empty segment are left as they are; a target outside 0 .. n_points - 1 or a query row >= n_queries is
 * not read and adds nothing.  A segment may have any length (it is not bounded by FLOODER_KNN_WIDE_MAX: a point can be
 * a neighbour of every query).
 *
 * Refused (FLOODER_E_ARG, the message opens with the entry's name), all before a pointer is read: dim outside 2..8; m
 * outside 1..FLOODER_KNN_WIDE_MAX and ld_ids < m (grad_queries); a negative count; a NULL pointer (seg_target may be).
 * Then n_queries == 0 or n_seg == 0: FLOODER_OK, nothing is touched.
 */
int flooder_dtm_grad_queries_f32(const float* points, int64_t n_points, const float* queries, int64_t n_queries, int dim,
                                 const int32_t* ids, int64_t ld_ids, int m, const float* coef, float* out_q,
                                 void* stream);
int flooder_dtm_grad_points_f32(const float* points, int64_t n_points, const float* queries, int64_t n_queries, int dim,
                                const float* coef, const int64_t* entries, const int64_t* seg_ptr,
                                const int32_t* seg_target, int64_t n_seg, float* out_p, void* stream);

/*
 * ---- Backward of the distance to a weighted measure (csrc/flood_mass_grad.hip;
 *      distance_to_weighted_measure(differentiable=True), stat "dtm") -------------------------------------------------
 * Per reached query q flooder_knn_mass_f32 lists the sites y_(t), t = 0 .. j*, j* = count[q] - 1 the crossing position.
 * With tau = *tau, M the cumulative mass of the positions before j* and rho = tau - M, the squared value is
 * F = sum_t a_t |q - y_(t)|^2 / tau with a_t = the mass of y_(t) for t < j* and a_(j*) = rho.  c_q is the coefficient the
 * caller forms (grad_out / (f tau), 0 where f = 0; grad_out * 2 / tau for the squared value) and h_q = c_q / 2.  No
 * tree, no contribution is ever stored, no atomics, plain loads and stores, every output word written once per launch.
 * ("kth" needs none of these entries: it is flooder_dtm_grad_*_f32 on the column of crossing ids with m = 1.)
 * Two layouts keep every entry at a dozen arguments and every per-entry read of the transposes at one 16-byte load:
 *   sites  (n_sites, dim + 1) float32, contiguous, input order: the row of a site is its dim coordinates, then its mass;
 *   qrow   (n_queries, 4) 32-bit words, 16-byte aligned, the crossing row of a query: [0] c_q (float32, the caller's),
 *          [1] rho (float32), [2] the crossing id (int32; -1 without a list), [3] dstar2 = d2(q, y_(j*)) (float32);
 *          flooder_mass_grad_queries_f32 reads word 0 and writes words 1 to 3, the transposes read all four.
 * d2(q, y) is everywhere t_0 * t_0 + t_1 * t_1 + ..., t_a = q[a] - y[a], every product and every sum rounded to float32,
 * left to right (no fused step).  queries (n_queries, dim) are the caller's contiguous float32 rows.
 *
 * flooder_mass_grad_queries_f32: one wave per query.  kk = min(count[q], ld_ids).  kk <= 0: out_q[q, :] = +0,
 * rho = 0, crossing id = -1, dstar2 = 0.  Else lane l adds (double)mass of the positions l, l + 64, ... < kk - 1 to a
 * partial sum that starts as +0, left to right; the 64 sums are added in the butterfly of flooder_dtm_grad_queries_f32
 * (a_l = a_l + a_(l ^ s), s = 32, 16, 8, 4, 2, 1) to M; rho = (float)(tau - M), the subtraction in double; the crossing
 * id is ids[q, kk - 1] and dstar2 the d2 of q to that site (0 if the id is no site).  Then lane l takes
 * acc = fmaf(a_t, queries[q, c] - y_(t)[c], acc) over its positions l, l + 64, ... < kk from +0, the sums are added in
 * the same butterfly and out_q[q, c] = c_q * sum; a c_q that is 0 gives +0 words (nothing is gathered; words 1 to 3 are
 * written all the same).  An id outside 0 .. n_sites - 1 is not read and adds neither mass nor difference.  With masses
 * all 1.0f and tau = kk the words of out_q are those of flooder_dtm_grad_queries_f32 at m = kk.
 * rho is exact, and the rho of flooder_knn_mass_f32 bit for bit, whenever every partial sum of the masses is an exact
 * float64 number - integer masses with a total below 2^53 (a coreset's counts).  Otherwise M is another fixed order of
 * the same non-negative float64 terms as the forward's prefix sum: the two differ by at most kk * 2^-52 * M, rho by
 * that plus its own rounding of 2^-24 relative; the same word run to run.
 *
 * flooder_mass_grad_points_f32 and flooder_mass_grad_masses_f32: the transposes.  entries, seg_ptr, seg_target and
 * n_seg are those of flooder_dtm_grad_points_f32 (the LOW 32 bits of an entry are the query row; segment g belongs to
 * the site j = seg_target[g], j = g when seg_target is NULL; inside a segment the entries ascend by query row).
 *   points  thread (g, c) starts from the word in out_p[j, c] ((n_sites, dim) rows) and takes its entries front to back:
 *           a = rho_q when q's crossing id is j, else the mass of j; e = c_q * a, ONE float32 product;
 *           acc = fmaf(-e, queries[q, c] - y_j[c], acc); then out_p[j, c] = acc.
 *   masses  thread (g) starts from out_m[j] ((n_sites,)) and takes the entries whose crossing id is NOT j front to back:
 *           acc = fmaf(0.5f * c_q, d2(q, y_j) - dstar2_q, acc); then out_m[j] = acc.
 * Launches over consecutive groups of ascending query rows (queries, qrow and the entries' rows relative to the group's
 * first row) continue one sequential sum per word: the result does not depend on the groups, bit for bit.  Words without
 * a non-empty segment are left as they are; a target outside 0 .. n_sites - 1 or a query row >= n_queries is not read
 * and adds nothing.  With masses all 1.0f and rho 1.0f the words of out_p are those of flooder_dtm_grad_points_f32.
 *
 * Refused (FLOODER_E_ARG, the message opens with the entry's name), all before a pointer is read: dim outside 2..8;
 * ld_ids outside 1..FLOODER_KNN_WIDE_MAX (grad_queries); a negative count; a NULL pointer (seg_target may be).  Then
 * n_queries == 0 or n_seg == 0: FLOODER_OK, nothing is touched.
 */
int flooder_mass_grad_queries_f32(const float* sites, int64_t n_sites, const float* queries, int64_t n_queries, int dim,
                                  const int32_t* ids, int64_t ld_ids, const int32_t* count, const double* tau,
                                  void* qrow, float* out_q, void* stream);
int flooder_mass_grad_points_f32(const float* sites, int64_t n_sites, const float* queries, int64_t n_queries, int dim,
                                 const void* qrow, const int64_t* entries, const int64_t* seg_ptr,
                                 const int32_t* seg_target, int64_t n_seg, float* out_p, void* stream);
int flooder_mass_grad_masses_f32(const float* sites, int64_t n_sites, const float* queries, int64_t n_queries, int dim,
                                 const void* qrow, const int64_t* entries, const int64_t* seg_ptr,
                                 const int32_t* seg_target, int64_t n_seg, float* out_m, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FLOODER_HIP_H */
