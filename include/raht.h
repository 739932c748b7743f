/*
 * raht.h -- C ABI of the MI355X-native RAHT attribute codec (libraht_hip.so, gfx950).
 *
 * Drop-in boundary: the three-entry operator table every reference driver dispatches through,
 *     raht_fn = {"RAHT", "iRAHT", "RAHT_param"}      (reference python/encode_3dgs.py:23-27,
 *                                                      encode_ply.py:20-24, encode_dataset.py:20-24)
 * plus the voxelizer that produces its input (python/voxelize_pc.py:62-172) and the driver-inline
 * quantize / reorder arithmetic (python/encode_3dgs.py:204-217, 261-268).
 *
 * Conventions
 *   - every function returns an int status: 0 = RAHT_OK, negative = error; raht_last_error()
 *     returns a thread-local, human-readable description of the last failure;
 *   - no C++ exceptions, no torch types: plain pointers and sizes only;
 *   - all data pointers are DEVICE pointers (HBM) unless a parameter says "host";
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream). Transform entry points
 *     (raht_fwd*, raht_inv*, raht_quant*, raht_dequant*) only enqueue kernels on `stream`: no
 *     host synchronisation and, after the first call for a given (element type, D) or after
 *     raht_plan_prepare, no allocation: safe to capture in a hipGraph. Plan construction and
 *     raht_voxelize allocate and synchronise `stream` (they size outputs from device counts);
 *   - every other entry point with a `stream` argument is one of two kinds, and all its device
 *     work is on `stream`: it reads its device inputs behind whatever the caller has enqueued
 *     there before the call, on a non-blocking stream too. Where the description of an entry
 *     point says which kind it is, that holds; for the ones that do not:
 *       enqueue only, never synchronise:
 *         raht_voxel_keys, raht_morton, raht_demorton, raht_merge_clusters, raht_rows_gather,
 *         raht_rows_scatter, raht_transpose_i32, raht_sqdiff_columns, raht_plan_order,
 *         raht_plan_copy_array, raht_plan_roots, raht_region_layout, raht_region_layout_set,
 *         raht_region_assemble, raht_region_assemble_set, raht_octree_encode_inter,
 *         raht_octree_decode_inter, raht_octree_bytes_used;
 *       synchronise `stream`:
 *         raht_sort_keys (it reads back the word that says whether the sort must be repeated);
 *         raht_plan_set_top_level when the new level differs from the plan's and truncates the
 *         tree (it reads back the number of roots; otherwise it returns without waiting);
 *         raht_plan_set_row_map with a map (it reads back an error word; with NULL it waits for
 *         the whole device if a map was set, and for nothing otherwise); raht_region_cells,
 *         raht_region_needs and raht_region_needs_bi (they return counts); raht_voxelize_all,
 *         raht_voxelize_plan and raht_voxelize_merge (as raht_voxelize).
 *     raht_plan_export_level has no stream argument and needs none: what it copies to the host
 *     was written by plan construction, which has synchronised, and is never rewritten.
 *     A call that enqueues only may still wait for the device when its host thread's pool of
 *     temporary blocks has to hand it a block last used on another stream (below);
 *   - the caller owns every data buffer; a plan is an opaque handle owning its own HBM;
 *   - rows of C / T are the points in Morton order, row-major, `ld*` = row stride in ELEMENTS;
 *   - N < 2^31 rows; element offsets are 64-bit;
 *   - devices and threads: every call works on the calling thread's current HIP device, which must be the
 *     device the plan and the buffers live on (one process per GPU is the intended use, but a process may
 *     hold plans on several devices: a plan remembers its device, all cached device memory is kept per
 *     device, and an entry point called with a plan while ANOTHER device is current returns
 *     RAHT_ERR_INVALID instead of mixing memory of two GPUs; raht_plan_destroy alone may be called with any
 *     device current). Different plans
 *     may be used from different host threads at once; ONE plan runs one transform at a time (it owns its
 *     workspaces), i.e. calls on the same plan must be ordered on one stream or serialised by the caller.
 *     Temporary device blocks are pooled per host thread and reused in call order: a host thread that
 *     switches streams between calls must order those streams itself (event or synchronise).
 */
#ifndef RAHT_H
#define RAHT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RAHT_VERSION 300

enum raht_status {
    RAHT_OK = 0,
    RAHT_ERR_INVALID = -1,      /* bad argument (NULL, N < 1, depth out of range, D < 1 ...)          */
    RAHT_ERR_UNSORTED = -2,     /* Morton keys not strictly increasing (unsorted or duplicate voxels):
                                   the reference silently mis-pairs these (SURVEY 8a iii/iv)          */
    RAHT_ERR_BOUNDS = -3,       /* a coordinate is < 0 or >= 2^depth (reference RAHT_param.py:26-27
                                   raises ValueError in the slow path, the fast path does not check) */
    RAHT_ERR_HIP = -4,          /* a HIP runtime call failed                                          */
    RAHT_ERR_NOMEM = -5,
    RAHT_ERR_UNSUPPORTED = -6
};

enum raht_dtype { RAHT_F32 = 0, RAHT_F64 = 1, RAHT_I32 = 2, RAHT_I64 = 3 };

/* Which kernel family executes a transform.
 *   RAHT_ENGINE_TILE  : LDS-tile-fused stages (default): a block stages a run of Morton-contiguous
 *                       rows in LDS and performs every butterfly whose subtree lies inside the run;
 *                       the few surviving low-pass rows are merged by later, much smaller stages.
 *   RAHT_ENGINE_LEVEL : one launch per binary level (= per octree level per axis), rows gathered
 *                       from HBM pairwise. Kept as the simple formulation and as a cross-check. */
enum raht_engine { RAHT_ENGINE_TILE = 0, RAHT_ENGINE_LEVEL = 1 };

typedef struct raht_plan raht_plan;
typedef void *raht_stream_t;

const char *raht_last_error(void);
int raht_version(void);

/* ------------------------------------------------------------------------------------------------
 * Plan ("RAHT_param").  Replaces RAHT_param_reorder_fast(V, minV, width, depth)
 * (reference python/RAHT_param.py:190-279).
 *
 * V: N x 3 (x, y, z) coordinates holding integers, already Morton-sorted and duplicate-free, in
 * v_dtype. Vint = floor((V - minV) / (width / 2^depth)); key = sum_k (z_k + 2 y_k + 4 x_k) << 3k.
 * The arithmetic is IEEE float64 for EVERY element type (RAHT_F32, RAHT_I32 and RAHT_I64 coordinates are
 * converted to double first, as RAHT_param.py:21-24 promotes them): subtract, divide, floor, bit for bit
 * what the reference computes on the CPU, also on and next to voxel faces and for a width that is no
 * power of two. depth is 1..21 (up to 63-bit keys). Any coordinate whose index is not in [0, 2^depth) is
 * RAHT_ERR_BOUNDS, and so is any non-finite one (NaN, +-inf) and any value no int64 holds: the real value
 * is tested before it is converted. The error text names the first offending row.
 * Instead of the reference's per-level List / Flags / weights the plan stores three arrays of
 * length N derived from the sorted keys:
 *     lvl[i] = msb(key[i] ^ key[i-1])    the one binary level at which row i is a right sibling
 *     wl[i]  = i - i0                    weight (leaf count) of its left sibling, i0 = partner row
 *     wr[i]  = nxt(i) - i                weight of the subtree rooted at row i
 * plus order_RAGFT (coarse-to-fine coefficient permutation, RAHT_param.py:251-274).
 * Errors: RAHT_ERR_UNSORTED, RAHT_ERR_BOUNDS (both checked on device; the reference checks neither).
 * N == 1 yields order = [0] (the reference returns None and its drivers crash).
 */
int raht_plan_create(const void *V, int v_dtype, int64_t N, const double minV[3], double width,
                     int depth, raht_stream_t stream, raht_plan **out);

/* Same, from strictly increasing Morton keys (device, uint64) of `nbits` significant bits (<= 63).
 * leaf_weights (device int64[N], may be NULL = all ones) gives every row an occupancy weight: used
 * when rows are themselves roots of already-transformed subtrees (multi-GPU top levels). */
int raht_plan_create_from_keys(const uint64_t *keys_sorted, int64_t N, int nbits,
                               const int64_t *leaf_weights, raht_stream_t stream, raht_plan **out);
/* The same without the 8 N-byte copy of the keys: the plan reads the CALLER's array for as long as it lives (the
 * caller keeps `keys_sorted` allocated and unchanged until raht_plan_destroy). What a per-frame pipeline wants: the
 * voxelizer's sorted key buffer outlives the frame's plan anyway. */
int raht_plan_create_from_keys_borrowed(const uint64_t *keys_sorted, int64_t N, int nbits,
                                        const int64_t *leaf_weights, raht_stream_t stream, raht_plan **out);

/* Truncated trees (Morton-prefix sharded scenes): butterflies at binary levels >= top_level are
 * NOT performed by this plan's transforms; the rows that still carry a low-pass value afterwards
 * ("roots": row 0 and every row whose level is >= top_level, i.e. the first row of every
 * top-level prefix node) are stitched by the caller's top stage. Default top_level = 64 (whole
 * tree, one root = the DC row). Call before the first transform; rebuilds the tile schedules.
 *   raht_plan_roots           : number of roots and (optionally) their rows, ascending, into a
 *                               DEVICE int64[n_roots] buffer;
 *   raht_plan_set_root_buffer : DEVICE buffer of n_roots x D elements of the transform's type
 *                               (row stride D), or NULL. When set, forward transforms write the roots'
 *                               low-pass rows there (and, in the fused-quantization entry, leave
 *                               their Q rows untouched), inverse transforms read the roots from
 *                               there instead of from T / Q.
 *   raht_plan_set_root_buffer_wide : the second root buffer of the MIXED-precision entries (raht_fwd_quant_mixed,
 *                               raht_dequant_inv_mixed): DEVICE n_roots x n_wide doubles (row stride n_wide), or NULL.
 *                               With both buffers set, the mixed forward writes the roots' columns [n_wide, D) to the
 *                               float buffer and their columns [0, n_wide) to this one, in float64, unrounded (their Q
 *                               rows untouched); the mixed inverse reads them from the two. What the float buffer's
 *                               columns [0, n_wide) hold is unspecified: nothing may read them. Truncated plans run the
 *                               mixed entries only with both buffers set; the other entries ignore this one. */
int raht_plan_set_top_level(raht_plan *plan, int top_level, raht_stream_t stream);
int raht_plan_roots(const raht_plan *plan, int64_t *n_roots, int64_t *rows_dev, raht_stream_t stream);
int raht_plan_set_root_buffer(raht_plan *plan, void *buf_dev);
int raht_plan_set_root_buffer_wide(raht_plan *plan, double *buf_dev);

/* Row map (small plans only: N <= 8192, they run as ONE launch): plan row i lives in row map[i] of the
 * matrices handed to raht_fwd* / raht_inv* (which then have n_matrix_rows rows; rows outside the map are not
 * touched). map_dev: DEVICE int64[N], copied; NULL removes the map. This is how the replicated top tree of a
 * Morton-prefix sharded scene works IN PLACE on the padded all-gather buffer (world x max_roots rows) instead
 * of on a compacted copy of it. Not available with the fused-quantization entries or with w != NULL. */
int raht_plan_set_row_map(raht_plan *plan, const int64_t *map_dev, int64_t n_matrix_rows, raht_stream_t stream);

int raht_plan_destroy(raht_plan *plan);
int64_t raht_plan_size(const raht_plan *plan);          /* N */
int raht_plan_nbits(const raht_plan *plan);             /* 3 * depth */

/* Engine / tile-size selection (tile_rows = 0 keeps the automatic choice). tile_rows applies to
 * stage 0 (the HBM-heavy launch); raht_plan_set_tail_tile sets the geometry of the later, small
 * stages: rows per tile, channels per chunk (rounded so that every chunk holds at least 16 bytes of
 * channels), and `final_rows`: once at most that many entries are left, ONE launch (the top stage)
 * finishes the tree (0 = automatic: 4096; at most 8192). */
int raht_plan_set_engine(raht_plan *plan, int engine, int tile_rows);
int raht_plan_set_tail_tile(raht_plan *plan, int tail_rows, int tail_channels, int final_rows);
/* Upper bound on the number of stages (= kernel launches per direction) of a tile schedule, 1..64,
 * default 24. A scene whose schedule would need more falls back to the one-launch-per-level engine (same
 * results): with >= 64 rows per tile every stage makes progress, so the bound is what decides. Mainly a
 * testing aid for that fallback; call before the first transform (drops the cached schedules). */
int raht_plan_set_max_stages(raht_plan *plan, int max_stages);

/* Plans, schedules and workspaces take their device memory from a process-wide cache of freed blocks
 * (a codec that builds one plan per frame stops paying hipMalloc / hipFree once the cache is warm;
 * at most 8 GiB stay cached by default). This returns the cached blocks to HIP. */
int raht_release_cached_memory(void);
/* Upper bound, in bytes, on what the cache keeps (process-wide, all devices together; default 8 GiB). A block that is given
 * back while the cache holds that much goes to hipFree instead. 0 caches nothing. Takes effect for the blocks given back
 * after the call: what is cached already stays until it is handed out again or raht_release_cached_memory() is called.
 * RAHT_ERR_INVALID for bytes < 0. */
int raht_set_cached_memory_limit(int64_t bytes);

/* Reference-shaped views, for parity tests and the drivers' DEBUG save_lists
 * (reference python/encode_3dgs.py:165). HOST output buffers.
 *   raht_plan_levels       = len(Flags) of the reference
 *   raht_plan_export_level : List[l] (int64), Flags[l] (uint8 0/1), weights[l] (int64); any of the
 *                            three may be NULL; *n receives the length of level l. */
int raht_plan_levels(const raht_plan *plan);
int raht_plan_export_level(const raht_plan *plan, int level, int64_t *list, uint8_t *flags,
                           int64_t *weights, int64_t *n);
/* order_RAGFT into a DEVICE int64[N] buffer (usable by index_select / argsort as the drivers do,
 * reference python/encode_3dgs.py:210,267). */
int raht_plan_order(const raht_plan *plan, int64_t *order_dev, raht_stream_t stream);
/* Device pointers of the internal arrays (valid until destroy), for inspection / tests. */
int raht_plan_arrays(const raht_plan *plan, const uint64_t **keys, const uint8_t **lvl,
                     const int32_t **wl, const int32_t **wr);
/* Copy one internal array into a caller-provided DEVICE buffer of N elements:
 * which = 0 keys (uint64), 1 lvl (uint8), 2 wl (int32), 3 wr (int32). */
int raht_plan_copy_array(const raht_plan *plan, int which, void *dst_dev, raht_stream_t stream);
/* Tile-engine schedule statistics: number of stages and active rows per stage (host int64[]). */
int raht_plan_stage_stats(raht_plan *plan, int elem_size, int D, int *n_stages, int64_t *rows_per_stage,
                          int max_stages, int *tile_rows);

/* ------------------------------------------------------------------------------------------------
 * Forward transform ("RAHT").  Replaces RAHT2_optimized(C, List, Flags, weights) -> (T, w)
 * (reference python/RAHT.py:252-336): T[i0] = a x0 + b x1, T[i1] = -b x0 + a x1 with
 * a = sqrt(w0/(w0+w1)), b = sqrt(w1/(w0+w1)) (weights are integer leaf counts; a, b are evaluated
 * in float64 and rounded once). C is never modified; T may not alias C. w (N, may be NULL) receives
 * the node weights of RAHT.py:325-328.
 * f32: fp32 arithmetic, tolerance vs the float64 reference is stated in DESIGN.md / tests;
 * f64: float64 arithmetic (the reference's own precision), rtol = atol = 1e-12.
 * Row strides (ld*, in elements) may be anything >= D; strides above 2^18 elements and rows shorter
 * than 16 bytes take the one-launch-per-level engine instead of the LDS-tile engine (same results).
 */
int raht_fwd(const raht_plan *plan, const float *C, int64_t ldc, int D, float *T, int64_t ldt,
             float *w, raht_stream_t stream);
int raht_fwd_f64(const raht_plan *plan, const double *C, int64_t ldc, int D, double *T, int64_t ldt,
                 double *w, raht_stream_t stream);

/* Inverse transform ("iRAHT").  Replaces inverse_RAHT_optimized(T, List, Flags, weights) -> C
 * (reference python/iRAHT.py:40-114): x0 = a T0 - b T1, x1 = b T0 + a T1, levels top-down. */
int raht_inv(const raht_plan *plan, const float *T, int64_t ldt, int D, float *C, int64_t ldc,
             raht_stream_t stream);
int raht_inv_f64(const raht_plan *plan, const double *T, int64_t ldt, int D, double *C, int64_t ldc,
                 raht_stream_t stream);

/* Fused variants for the float32 tile engine: the coefficient matrix T is never materialised.
 *   raht_fwd_quant   = raht_fwd + raht_quant_reorder      (encode_3dgs.py:159,204,210,215)
 *   raht_dequant_inv = raht_dequant_unreorder + raht_inv  (encode_3dgs.py:261,267-268,274)
 * Same results as the two-call sequences (identical float32 arithmetic).
 *
 * PRECISION OF THE float32 INTEGERS (against the reference's float64 floor(T / step + 0.5)). A float32 coefficient carries
 * ~1e-7 of its own magnitude in error, so an integer differs from the reference's when a rounding boundary falls inside
 * |dT| / step: on unit-range attribute channels that is +-1 in about 1e-8 (step 1) to 1e-6 (step 0.01) of the integers
 * (measured and bounded in tests/test_gpu_fullsize.py). The quotient itself has 24 significant bits: a channel whose
 * coefficients reach |T| / step >= 2^23 -- the xyz columns of a 59-channel frame at steps below ~0.1: |T| is ~1e6 there --
 * cannot be integer-exact in float32 (differences of tens of units at step 0.01). Callers that need the reference's integers
 * on such channels use raht_fwd_quant_f64 / raht_dequant_inv_f64 (same kernels in float64, Q bit-identical to the
 * float64 two-call sequence) or a per-channel step table with coarser steps on those channels. */
int raht_fwd_quant(const raht_plan *plan, const float *C, int64_t ldc, int D, const float *steps,
                   int n_steps, int32_t *Q, int64_t ldq, raht_stream_t stream);
int raht_dequant_inv(const raht_plan *plan, const int32_t *Q, int64_t ldq, int D, const float *steps,
                     int n_steps, float *C, int64_t ldc, raht_stream_t stream);

/* ONE forward pass, k quantizations: the drivers quantize one coefficient matrix at nine steps (python/encode_3dgs.py:28 colorStep,
 * :199-217), i.e. the forward transform of a frame is the same for every step. Q[i] = floor(T / steps[i] + 0.5), reordered, for
 * i < k -- each bit-identical to raht_fwd_quant(plan, C, ..., &steps[i], 1, Q[i], ...) -- from one pass over C: the write-back of
 * every finalised row quantizes it k times. steps: HOST float[k] (one step for all channels each); Q: HOST array of k DEVICE
 * matrices (N x D int32, row stride ldq, distinct). Level engine / row-mapped / truncated plans: k single calls inside. */
int raht_fwd_quant_multi(const raht_plan *plan, const float *C, int64_t ldc, int D, const float *steps, int k,
                         int32_t *const *Q, int64_t ldq, raht_stream_t stream);

/* raht_dequant_inv fused with the drivers' distortion measurement (python/encode_3dgs.py:274 C_rec = iRAHT(...), then :298-310
 * torch.mean((C - C_rec) ** 2) over all / quats / scales / opacity / colour columns): the stage-0 kernel of the fused inverse
 * compares every row it reconstructs with the ORIGINAL attributes C_ref on its way out.
 *   sqdiff : DEVICE double[D]: sum over rows of (C_rec[i, c] - C_ref[i, c])^2 -- differences in float32, squares and sums in
 *            float64, summed in a fixed order (deterministic); what raht_sqdiff_columns(C_ref, C_rec) returns, up to the order
 *            of the float64 additions;
 *   C_rec  : the reconstruction, bit-identical to raht_dequant_inv's -- or NULL: then it is never written (the PSNR columns
 *            need the sums only), and a decode step is one pass over Q and C_ref instead of Q -> C_rec, then C_ref and C_rec.
 * Shapes outside the fused path (D > 64, trees of one launch, level engine, truncated plans) run the two calls inside. */
int raht_dequant_inv_sqdiff(const raht_plan *plan, const int32_t *Q, int64_t ldq, int D, const float *steps, int n_steps,
                            const float *C_ref, int64_t ld_ref, float *C_rec, int64_t ldc, double *sqdiff, raht_stream_t stream);

/* The same two at the reference's own precision (python/encode_3dgs.py:82-83: float64 coefficients are what
 * :204 quantizes): the float64 tile kernels with the float64 quantizer (IEEE double division, float64 steps) in their
 * write-back / row gather -- one pass, no N x D temporary. Q is bit-identical to raht_fwd_f64 + raht_quant_reorder_f64,
 * i.e. to floor(T64 / step + 0.5) of the float64 transform. (Level engine / D < 2: the two-call sequence.) */
int raht_fwd_quant_f64(const raht_plan *plan, const double *C, int64_t ldc, int D, const double *steps,
                       int n_steps, int32_t *Q, int64_t ldq, raht_stream_t stream);
int raht_dequant_inv_f64(const raht_plan *plan, const int32_t *Q, int64_t ldq, int D, const double *steps,
                         int n_steps, double *C, int64_t ldc, raht_stream_t stream);

/* MIXED PRECISION: float32 rows whose first n_wide channels (1..4) are carried in float64 through the whole transform, in the
 * SAME launches as the float32 channels (csrc/transform_mx.hip). What it is for: the reference quantizes float64 coefficients
 * (python/encode_3dgs.py:82-83,204), and on a 59-column frame whose columns 0-2 are the voxel coordinates
 * (python/voxelize_pc.py:155) those three columns' coefficients reach 1e6, i.e. |T| / step > 2^24 at the steps the attribute
 * channels need -- float32 integers are tens of units off there (see above) while the 56 attribute columns are fine.
 *   channels [0, n_wide)  : input converted exactly to float64, float64 butterflies with float64 a / b, IEEE double division by
 *                           the float64 step: Q bit-identical to raht_fwd_quant_f64 on those columns, i.e. the reference's
 *                           integers (up to 1-ulp transform noise on exact rounding ties); the inverse rounds once, on output;
 *   channels [n_wide, D)  : float32 arithmetic with (float) steps[c]: bit-identical to raht_fwd_quant / raht_dequant_inv.
 * steps: HOST float64[n_steps], n_steps == 1 or D. D - n_wide >= 4 and D <= 68 run the mixed tile kernels (one pass, ~5 % slower
 * than the float32 kernels); other shapes, and plans switched to the level engine, run the float32 path followed by a float64
 * pass over the n_wide columns (same results up to rounding ties). Not available for row-mapped plans. Root buffers: both
 * (raht_plan_set_root_buffer + raht_plan_set_root_buffer_wide) or neither; truncated plans need both -- the shard-local
 * half of a Morton-prefix sharded step (the roots' Q rows are left to the caller's top stage). */
int raht_fwd_quant_mixed(const raht_plan *plan, const float *C, int64_t ldc, int D, const double *steps, int n_steps,
                         int n_wide, int32_t *Q, int64_t ldq, raht_stream_t stream);
int raht_dequant_inv_mixed(const raht_plan *plan, const int32_t *Q, int64_t ldq, int D, const double *steps, int n_steps,
                           int n_wide, float *C, int64_t ldc, raht_stream_t stream);
/* The two driver-loop fusions of the float32 entries (raht_fwd_quant_multi, raht_dequant_inv_sqdiff) in mixed precision: a
 * 59-column frame gets the fusions AND the reference's integers on its wide columns.
 *   raht_fwd_quant_mixed_multi : ONE mixed forward pass, k quantizations. steps: HOST double[k], one scalar step per output
 *     matrix; Q: HOST array of k distinct DEVICE matrices (N x D int32, row stride ldq). Q[i] is bit-identical to
 *     raht_fwd_quant_mixed(plan, C, ldc, D, &steps[i], 1, n_wide, Q[i], ldq, stream). Any k >= 1 (chunked internally by 12
 *     matrices per pass). Argument rules: those of raht_fwd_quant_mixed for every steps[i] (n_wide 1..4 and <= D, steps[i] > 0
 *     also as float32, no row-mapped plans, both root buffers or neither), plus k >= 1 and no two Q[i] the same.
 *   raht_dequant_inv_mixed_sqdiff : raht_dequant_inv_mixed whose stage-0 kernel compares every row it writes with C_ref.
 *     C_rec, when not NULL, is bit-identical to raht_dequant_inv_mixed's; with C_rec == NULL nothing is written there.
 *     sqdiff: DEVICE double[D], sqdiff[c] = sum over rows of (C_rec[i, c] - C_ref[i, c])^2, taken from the float32 values the
 *     mixed inverse writes (the wide columns after their one rounding to float32, as raht_dequant_inv_sqdiff defines it):
 *     differences in float32, squares and sums in float64, summed in a fixed order (deterministic); equal to
 *     raht_sqdiff_columns(C_ref, C_rec) up to the order of the float64 additions. Argument rules: those of
 *     raht_dequant_inv_mixed, plus C_ref and sqdiff set.
 * Shapes outside the mixed tile kernels (raht_plan_mixed_stats(...) tile_rows == 0: level engine, D - n_wide < 4, D > 68),
 * trees of one launch and plans with root buffers (truncated plans) run the single calls inside, with the same results: k x
 * raht_fwd_quant_mixed, or raht_dequant_inv_mixed into C_rec (or a scratch matrix) followed by raht_sqdiff_columns. Under
 * raht_plan_set_concurrent_directions, multi is a forward-direction call and sqdiff an inverse-direction call: each uses that
 * direction's workspaces and the schedule and tile programs of the single mixed calls. */
int raht_fwd_quant_mixed_multi(const raht_plan *plan, const float *C, int64_t ldc, int D, const double *steps, int k,
                               int n_wide, int32_t *const *Q, int64_t ldq, raht_stream_t stream);
int raht_dequant_inv_mixed_sqdiff(const raht_plan *plan, const int32_t *Q, int64_t ldq, int D, const double *steps, int n_steps,
                                  int n_wide, const float *C_ref, int64_t ld_ref, float *C_rec, int64_t ldc, double *sqdiff,
                                  raht_stream_t stream);
/* Tile rows / stage sizes the mixed kernels use for (D, n_wide); *tile_rows = 0 when the shape takes the two-pass path. */
int raht_plan_mixed_stats(raht_plan *plan, int D, int n_wide, int *tile_rows, int *n_stages, int64_t *rows_per_stage,
                          int max_stages);

/* SEVERAL SCENES IN ONE SET OF LAUNCHES (BASELINE configs[3] is a batch of scenes; the frames of a dynamic sequence are
 * one too). Scene i = (plans[i], C[i] / Q[i] with row strides ldc[i] / ldq[i]); all scenes share D and the step table.
 * Stage k of every scene runs in ONE tile-kernel launch (a workgroup finds its scene from its index) and the top stages in
 * one launch with blockIdx.y = scene: a frame of ~1 M Gaussians on its own fills the 768 workgroup slots of the chip two
 * and a half times and then spends a third of its step in three latency-bound tail launches; in a batch the partial rounds
 * of the scenes fill each other and all tails are one launch per stage. Results are BIT-IDENTICAL to n calls of the
 * single-scene entry points (same kernels, same tiles: tests/test_gpu_parity.py::test_batch_*). Any n >= 1 (launches carry
 * up to 8 scenes each); float32 tile engine -- scenes that need the level engine (D < 4, strides > 2^18, pathological key
 * patterns) or a row map run through their single-scene entry point inside the same call. Plans must be distinct objects
 * (a plan owns its workspaces) on the current device. Arrays of pointers / strides are HOST arrays. Nothing of the tile
 * engine is launched unless the arguments of every (scene, stage) are there. A plan with stage-0 events set
 * (raht_plan_set_stage0_events) stays in the batch launches, and these four calls do NOT record its events: a batched launch
 * is not one scene's stage 0. */
int raht_fwd_batch(int n, raht_plan *const *plans, const float *const *C, const int64_t *ldc, int D,
                   float *const *T, const int64_t *ldt, raht_stream_t stream);
int raht_inv_batch(int n, raht_plan *const *plans, const float *const *T, const int64_t *ldt, int D,
                   float *const *C, const int64_t *ldc, raht_stream_t stream);
int raht_fwd_quant_batch(int n, raht_plan *const *plans, const float *const *C, const int64_t *ldc, int D,
                         const float *steps, int n_steps, int32_t *const *Q, const int64_t *ldq, raht_stream_t stream);
int raht_dequant_inv_batch(int n, raht_plan *const *plans, const int32_t *const *Q, const int64_t *ldq, int D,
                           const float *steps, int n_steps, float *const *C, const int64_t *ldc, raht_stream_t stream);

/* The same for the MIXED-PRECISION fused entries (59-column frames: the xyz columns in float64, above): scene i's output is
 * BIT-IDENTICAL to raht_fwd_quant_mixed(plans[i], C[i], ldc[i], D, steps, n_steps, n_wide, Q[i], ldq[i], stream), resp.
 * raht_dequant_inv_mixed(plans[i], Q[i], ldq[i], D, steps, n_steps, n_wide, C[i], ldc[i], stream)
 * (tests/test_gpu_mixed_batch.py). What is batched: round r of the forward carries stage r of every scene that has one (the
 * inverse walks the rounds backwards from the deepest schedule); within a round the tile stages of equal launch shape go out
 * up to 8 scenes per launch and the top stages likewise (blockIdx.y = scene); a group of one is the single call's own launch.
 * What runs through raht_fwd_quant_mixed / raht_dequant_inv_mixed inside the same call, in place in the stream and with the
 * same results: scenes whose shape takes the two-pass path (raht_plan_mixed_stats(...) tile_rows == 0: level engine,
 * D - n_wide < 4, D > 68, a row stride > 2^18), plans with root buffers (truncated plans, the shard-local half of a sharded
 * step) and plans with stage-0 events set (raht_plan_set_stage0_events). What is refused: row-mapped plans
 * (RAHT_ERR_UNSUPPORTED, as in the single calls), and with RAHT_ERR_INVALID every breach of the single calls' argument rules
 * for any scene (n_wide 1..4 and <= D, n_steps 1 or D, steps > 0 also as float32, row strides >= D, both root buffers or
 * neither) or of the batch rules above (n >= 1, HOST arrays of pointers / strides all set, distinct plans on the current
 * device). The rules that need no plan are checked first, before any plan is dereferenced and before any HIP call; nothing is
 * launched for any scene unless every scene passed. raht_last_error() names the function and, where it applies, the scene.
 * Under raht_plan_set_concurrent_directions the forward batch is a forward-direction call and the inverse batch an
 * inverse-direction call of every plan in it. */
int raht_fwd_quant_mixed_batch(int n, raht_plan *const *plans, const float *const *C, const int64_t *ldc, int D,
                               const double *steps, int n_steps, int n_wide,
                               int32_t *const *Q, const int64_t *ldq, raht_stream_t stream);
int raht_dequant_inv_mixed_batch(int n, raht_plan *const *plans, const int32_t *const *Q, const int64_t *ldq, int D,
                                 const double *steps, int n_steps, int n_wide,
                                 float *const *C, const int64_t *ldc, raht_stream_t stream);
/* Dry run of the grouping those two calls perform (the same function, told to count instead of launching): the number of
 * batched or single-stage tile launches, of top-stage launches and of scenes that would run through the single-scene call, for
 * contiguous rows (row stride D) and the plans' present root buffers / events (a truncated plan counts as a single-scene call).
 * May build schedules and tile programs, as raht_plan_mixed_stats does; launches no transform kernel. */
int raht_mixed_batch_stats(int n, raht_plan *const *plans, int D, int n_wide, int inverse,
                           int *tile_launches, int *top_launches, int *single_scene_calls);

/* Pre-build the tile schedule and the per-stage workspaces for (elem_size in {4, 8}, D). The
 * first transform with a new (element type, D) does this implicitly (allocating and synchronising
 * once); after raht_plan_prepare the transform entry points only enqueue kernels (hipGraph-safe).
 * A plan owns its workspaces: do not run transforms of one plan concurrently on several streams. */
int raht_plan_prepare(raht_plan *plan, int elem_size, int D, raht_stream_t stream);

/* A plan owns ONE set of per-stage workspaces, so its transforms must be ordered on one stream (above). With this switched on it
 * keeps one set PER DIRECTION: one forward-direction call (raht_fwd*, raht_fwd_quant*) and one inverse-direction call (raht_inv*,
 * raht_dequant_inv*) of the same plan may then be in flight at the same time on two streams -- the shape of the drivers' loop
 * over quantization steps (python/encode_3dgs.py:199-275): the forward of step s + 1 does not depend on the inverse of step s,
 * and one direction's latency-bound tail stages then run under the other's HBM-bound first stage. Costs a second copy of the
 * workspaces (~5 % of a coefficient matrix); they are re-allocated by the next transform or raht_plan_prepare. Two calls of the
 * SAME direction still have to be ordered by the caller. The arrays derived from a tile schedule (tile heights; the mixed-precision
 * kernels' tile programs) are written by kernels that the call building them enqueues on its own stream and does not wait for; a
 * later call on ANOTHER stream first makes its stream wait for an event recorded behind them, so the first inverse may run on a
 * side stream right behind the forward that built the schedule. */
int raht_plan_set_concurrent_directions(raht_plan *plan, int on);

/* Profiling aid: HIP events (hipEvent_t, created by the caller with timing enabled) recorded on the
 * launch stream immediately before and after the STAGE-0 kernel of every following transform of this
 * plan, so that the dominant kernel can be timed inside a real step (hipEventElapsedTime after the
 * stream has been synchronised). Stage 0 is the first launch of a forward and the last of an inverse,
 * a tile stage or, for a tree of one launch, the top stage; every single-scene transform entry of the
 * tile engines records the pair (tests/test_gpu_stage0_events.py), the level engine and the float32
 * batch entries do not. NULL, NULL switches it off. */
int raht_plan_set_stage0_events(raht_plan *plan, void *ev_before, void *ev_after);

/* Profiling aid: enqueue ONE stage of the float32 tile schedule (stage 0 is the HBM-heavy launch).
 * Not a transform by itself; bench.py uses it to time the dominant kernel with HIP events.
 *   Q == NULL : plain kernels   (forward: mat = C in, mat2 = T out;  inverse: mat = T in, mat2 = C out)
 *   Q != NULL : fused-quantization kernels (forward: mat = C in, Q out;  inverse: Q in, mat2 = C out)
 * ablate: 0 = the real kernel; 1 = skip the butterflies; 2 = also skip merge resolution (a pure
 * staged copy) -- timing experiments only, the output is then not a transform. Ablations exist only in a
 * profiling build of the library (make ABLATE=1); the product build returns RAHT_ERR_UNSUPPORTED for
 * ablate != 0 and its kernels carry no ablation branches. */
int raht_debug_run_stage(const raht_plan *plan, int inverse, int stage, const float *mat, int64_t ld_mat,
                         int D, float *mat2, int64_t ld_mat2, int32_t *Q, int64_t ldq, float step,
                         int ablate, raht_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Quantize + reorder / dequantize + un-reorder (driver-inline in the reference,
 * python/encode_3dgs.py:204 floor(x/step+0.5), :210 index_select(0, order_RAGFT), :215 int32;
 * :261 x*step, :267-268 gather by argsort(order_RAGFT)).
 *   Q[k, c] = (int32) floor(T[order[k], c] / step_c + 0.5)        T[order[k], c] = Q[k, c] * step_c
 * steps: HOST array of n_steps values, n_steps == 1 (one step for all channels) or == D.
 *
 * THE OUT-OF-RANGE RULE, for this and every other entry point that quantizes (raht_fwd_quant*, raht_quant_rows*, the mixed, multi and
 * batch forms, raht_rlgr_seg_rate): for a coefficient x and a step s of type T (float or double) all arithmetic is in T -- q = x / s
 * (IEEE division), r = floor(q + 0.5) -- and the integer is
 *   r          if -2^31 <= r <= 2^31 - 1  (float: q + 0.5f rounds to even from 2^23 on, as float32 arithmetic does)
 *   INT32_MAX  if r > 2^31 - 1, +inf included   (x = +inf, or a quotient that overflows T)
 *   INT32_MIN  if r < -2^31, -inf included
 *   0          if r is NaN                       (x is NaN)
 * The reference leaves these cases to the platform's conversion (encode_3dgs.py:215), which differs between the CPU and a GPU; here
 * the device kernels, the host twins, the oracle and the torch helper of the unfused drivers (ops.to_int32) return the same integers,
 * bit for bit (tests/test_gpu_quant_edges.py, tests/test_quant_edges_model.py). A saturated integer is not reported: a caller keeps a
 * column whole by keeping |x| / s below 2^31 -- for the DC term of a column, |mean| * sqrt(N) / s < 2^31. */
int raht_quant_reorder(const raht_plan *plan, const float *T, int64_t ldt, int D, const float *steps,
                       int n_steps, int32_t *Q, int64_t ldq, raht_stream_t stream);
int raht_dequant_unreorder(const raht_plan *plan, const int32_t *Q, int64_t ldq, int D,
                           const float *steps, int n_steps, float *T, int64_t ldt,
                           raht_stream_t stream);
/* float64 coefficients and steps (the reference's precision): IEEE double division, as torch on the CPU. */
int raht_quant_reorder_f64(const raht_plan *plan, const double *T, int64_t ldt, int D, const double *steps,
                           int n_steps, int32_t *Q, int64_t ldq, raht_stream_t stream);
int raht_dequant_unreorder_f64(const raht_plan *plan, const int32_t *Q, int64_t ldq, int D,
                               const double *steps, int n_steps, double *T, int64_t ldt,
                               raht_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Voxelizer.  Replaces voxelize_pc_batched(PC, vmin, width, J) (reference
 * python/voxelize_pc.py:62-172) and get_morton_code (:25-59): shift by vmin, Vint =
 * clamp(floor((V - vmin) / (width / 2^J)), 0, 2^J - 1) in float32 as torch does, 3J-bit Morton
 * key, STABLE LSD radix sort on device, voxel starts where the key changes, per-voxel attribute
 * mean (sequential in sorted order, so bit-reproducible). The division is the IEEE float32 division torch performs on
 * the CPU (where the reference's golden vectors come from); a GPU run of the reference multiplies by 1 / voxel_size
 * instead and may put a point that sits within 1 ulp of a voxel face into the neighbouring voxel (fixtures
 * tests/golden/vox_boundary*_j9.npz: width 7.3, points at k * voxel_size and one float32 step either side).
 *   PC      : N x (3 + d) float32, row stride ldpc elements
 *   vmin_in : HOST float[3] or NULL (-> per-axis minimum);  width_in < 0 -> max over axes of V - vmin
 * Outputs (DEVICE, caller-allocated for N rows; any may be NULL):
 *   keys_sorted uint64[N], sort_idx int64[N], voxel_indices int64[<=N], PCvox float[<=N x (3+d)]
 *   (integer voxel coordinates as floats, then mean attributes), Vvox int64[<=N x 3].
 * HOST outputs: *n_vox, vmin_out[3], *width_out, *voxel_size_out. */
int raht_voxelize(const float *PC, int64_t ldpc, int64_t N, int d, const float *vmin_in,
                  double width_in, int J, uint64_t *keys_sorted, int64_t *sort_idx,
                  int64_t *voxel_indices, float *PCvox, int64_t *Vvox, int64_t *n_vox,
                  float vmin_out[3], double *width_out, double *voxel_size_out,
                  raht_stream_t stream);

/* voxelize_pc_batched with ALL its outputs in one call (reference python/voxelize_pc.py:62-172 returns PCvox, PCsorted,
 * voxel_indices, DeltaPC together): raht_voxelize plus PCsorted (N x (3+d), may be NULL) and DeltaPC (N x (3+d), may be NULL;
 * needs PCvox) as raht_voxelize_residuals defines them, produced by the SAME pass over the gathered rows that forms the
 * per-voxel means (clouds with >= 5 attribute columns; narrower ones run the two-call sequence inside and then need sort_idx).
 * Bit-identical to raht_voxelize followed by raht_voxelize_residuals. */
int raht_voxelize_all(const float *PC, int64_t ldpc, int64_t N, int d, const float *vmin_in, double width_in,
                      int J, uint64_t *keys_sorted, int64_t *sort_idx, int64_t *voxel_indices, float *PCvox,
                      int64_t *Vvox, float *PCsorted, float *DeltaPC, int64_t *n_vox, float vmin_out[3],
                      double *width_out, double *voxel_size_out, raht_stream_t stream);

/* One frame's prelude in one call: raht_voxelize, then the RAHT plan built STRAIGHT from the voxelizer's own sorted,
 * unique voxel keys (the reference goes through a PLY file and re-derives the same Morton keys from the voxel coordinates:
 * voxelize_pc_batched, python/voxelize_pc.py:62-172, then RAHT_param_reorder_fast, python/RAHT_param.py:190-279).
 *   voxel_keys : DEVICE uint64[N], caller-allocated, REQUIRED: the first n_vox entries receive the voxels' keys and are
 *                BORROWED by the plan (as raht_plan_create_from_keys_borrowed: keep them alive and unchanged while the plan lives)
 *   other arguments as raht_voxelize; PCvox[:, 3:] is the attribute matrix in the plan's row order.
 * *plan is NULL on failure. */
int raht_voxelize_plan(const float *PC, int64_t ldpc, int64_t N, int d, const float *vmin_in, double width_in,
                       int J, uint64_t *voxel_keys, int64_t *voxel_indices, float *PCvox, int64_t *n_vox,
                       float vmin_out[3], double *width_out, double *voxel_size_out, raht_stream_t stream,
                       raht_plan **plan);

/* The voxelizer's secondary outputs (reference python/voxelize_pc.py:103-111, 147-156), from the primary ones of
 * raht_voxelize: PCsorted[k, :] = PC[sort_idx[k], :] (N x (3+d), may be NULL) and the residuals DeltaPC (N x (3+d)):
 * positions V0 - voxel_size * floor(V0 / voxel_size) with V0 = V - vmin, attributes minus their voxel's mean (PCvox).
 * DEVICE pointers except vmin (HOST float[3]); only enqueues kernels on `stream`. */
int raht_voxelize_residuals(const float *PC, int64_t ldpc, int64_t N, int d, const uint64_t *keys_sorted,
                            const int64_t *sort_idx, const float *PCvox, const float vmin[3], double voxel_size,
                            float *PCsorted, float *DeltaPC, raht_stream_t stream);

/* The voxelizer's first phase alone: the (unsorted) 3J-bit Morton key of every point for a GIVEN bounding box
 * (vmin: HOST float[3]; width > 0), same arithmetic as raht_voxelize. A Morton-prefix sharded front end buckets
 * points by the top key bits with it before the all-to-all (sharded.exchange_by_prefix). keys: DEVICE uint64[N]. */
int raht_voxel_keys(const float *PC, int64_t ldpc, int64_t N, const float vmin[3], double width, int J,
                    uint64_t *keys, raht_stream_t stream);

/* Morton keys of integer coordinates (get_morton_code, voxelize_pc.py:25-59). V: N x 3 int64. */
int raht_morton(const int64_t *V, int64_t N, int J, uint64_t *keys, raht_stream_t stream);

/* Stable LSD radix sort of uint64 keys (nbits significant) with an int64 index payload
 * (idx_out[k] = original position). DEVICE buffers. */
int raht_sort_keys(const uint64_t *keys_in, int64_t N, int nbits, uint64_t *keys_out,
                   int64_t *idx_out, raht_stream_t stream);
/* The sort runs one launch per digit pass whose tiles hand their offsets to each other inside the launch (csrc/scan_sort.hip).
 * A tile waits for the tiles numbered before it; tiles are numbered by workgroup index, which cannot deadlock as long as the
 * lowest-numbered unfinished workgroup is resident -- how this GPU dispatches, but not a documented guarantee -- so every wait is
 * bounded by the wall clock (0.2 s): a tile that gives up raises an error word, nothing is written through stale offsets, and
 * the call (raht_sort_keys, raht_voxelize*) REPEATS the sort with one launch chain per digit, which needs no such property.
 * The caller sees a correct result and a slower call; this counter (process-wide, monotonic) says how often it happened.
 * Expected 0: tools/check_big.py and the GPU suite assert it. The tests make a tile give up through raht_debug_sort_form and
 * watch this counter grow. */
int64_t raht_sort_fallbacks(void);

/* ------------------------------------------------------------------------------------------------
 * Per-voxel Gaussian merge. Replaces merge_clusters_cuda / merge_weighted_mean_kernel
 * (reference cuda/merge_cluster_wrapper.cu:11-116, cuda/merge_cluster.cu:2-111): cluster c owns the
 * Gaussians cluster_indices[cluster_offsets[c] .. cluster_offsets[c+1]); weight = opacity (or 1);
 * means / scales / colours = weighted means, quaternion = normalised weighted sum (identity
 * (0,0,0,1) if the norm is 0), opacity = min(sum, 1); empty clusters produce zeros. DEVICE pointers,
 * int32 indices / offsets, float32 data, row-major [N,3] [N,4] [N,3] [N] [N,color_dim]. */
int raht_merge_clusters(const int32_t *cluster_indices, const int32_t *cluster_offsets, int64_t num_clusters,
                        const float *means, const float *quats, const float *scales, const float *opacities,
                        const float *colors, int color_dim, int weight_by_opacity, float *merged_means,
                        float *merged_quats, float *merged_scales, float *merged_opacities,
                        float *merged_colors, raht_stream_t stream);

/* VOXELIZE + MERGE in one call and one pass over the rows (the reference runs its voxelizer and then its CUDA merge
 * kernel back to back: python/test_voxelize_3dgs.py:203-257, cuda/merge_cluster.cu:2-111 -- the sort permutation and the voxel
 * starts are the merge's cluster indices / offsets, :225-233).
 *   G    : N whole Gaussians, row-major [x y z | quat(4) | scale(3) | opacity | colour(color_dim)], row stride ldg >= 11 + color_dim
 *   Gvox : <= N rows of 11 + color_dim: the voxel's INTEGER coordinates as floats (like PCvox), then the merged attributes --
 *          the frame the RAHT path takes (59 columns at color_dim = 48); merged_means (<= N x 3, may be NULL): the merged positions
 * Per column exactly raht_merge_clusters' arithmetic on the members in sorted order (weight = opacity, or 1): bit-identical to
 * raht_voxelize (sort_idx, voxel_indices) followed by raht_merge_clusters on the five split arrays. Other arguments as raht_voxelize. */
int raht_voxelize_merge(const float *G, int64_t ldg, int64_t N, int color_dim, int weight_by_opacity, const float *vmin_in,
                        double width_in, int J, uint64_t *keys_sorted, int64_t *sort_idx, int64_t *voxel_indices, float *Gvox,
                        float *merged_means, int64_t *n_vox, float vmin_out[3], double *width_out, double *voxel_size_out,
                        raht_stream_t stream);

/* A few rows at explicit positions: Q[pos[i], :] = floor(X[i, :] / step + 0.5) and X[i, :] =
 * Q[pos[i], :] * step (pos: DEVICE int64[n], NULL = identity). Used for the <= 512 top coefficients of
 * a Morton-prefix sharded scene, which the shard-local fused kernels leave to the caller (no
 * counterpart in the reference; same arithmetic as python/encode_3dgs.py:204,215,261). */
int raht_quant_rows(const float *X, int64_t ldx, int64_t n, int D, const float *steps, int n_steps,
                    const int64_t *pos, int32_t *Q, int64_t ldq, raht_stream_t stream);
int raht_dequant_rows(const int32_t *Q, int64_t ldq, const int64_t *pos, int64_t n, int D, const float *steps,
                      int n_steps, float *X, int64_t ldx, raht_stream_t stream);
/* The same at the reference's precision (float64 X, float64 steps, IEEE double division as raht_quant_reorder_f64): the
 * sharded driver quantizes the top tree's wide columns of a mixed-precision step with these. */
int raht_quant_rows_f64(const double *X, int64_t ldx, int64_t n, int D, const double *steps, int n_steps,
                        const int64_t *pos, int32_t *Q, int64_t ldq, raht_stream_t stream);
int raht_dequant_rows_f64(const int32_t *Q, int64_t ldq, const int64_t *pos, int64_t n, int D, const double *steps,
                          int n_steps, double *X, int64_t ldx, raht_stream_t stream);

/* Rows at explicit positions, no arithmetic (elem_size 4 or 8 bytes per element; pos: DEVICE int64[n]):
 *   raht_rows_gather :  dst[i, :] = src[pos[i], :]        raht_rows_scatter :  dst[pos[i], :] = src[i, :]
 * One launch each; the sharded driver moves a shard's <= 512 root rows between the coefficient matrix and the
 * all-gather buffers with them. */
int raht_rows_gather(const void *src, int64_t ld_src, const int64_t *pos, int64_t n, int D, int elem_size, void *dst,
                     int64_t ld_dst, raht_stream_t stream);
int raht_rows_scatter(const void *src, int64_t ld_src, const int64_t *pos, int64_t n, int D, int elem_size, void *dst,
                      int64_t ld_dst, raht_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * RLGR entropy stage: adaptive Run-Length / Golomb-Rice coder, byte-exact with the
 * reference's vendored PyRLGR (python/PyRLGR/src/libs/rlgr/membuf.cpp:258-423, call sites
 * python/encode_3dgs.py:229-245). HOST pointers throughout: the coder is sequential and stays on
 * the CPU (as in the reference), but works on strided int32 columns of the quantized coefficient
 * matrix and codes the D channels on a pool of host threads.
 *   raht_rlgr_bound           : bytes that always suffice for n symbols
 *   raht_rlgr_encode          : == m = membuf(); m.rlgrWrite(seq, flag); m.close(); m.get_buffer()
 *   raht_rlgr_decode          : == membuf(buf).rlgrRead(n, flag)
 *   raht_rlgr_encode_channels : symbol n of channel c is Q[n * sym_stride + c * chan_stride] (row-major
 *                               N x D matrix: sym_stride = ld, chan_stride = 1; channel-major D x N as
 *                               produced by raht_transpose_i32: sym_stride = 1, chan_stride = N);
 *                               stream of channel c -> out + c * cap_per_channel, nbytes[c];
 *                               nthreads <= 0 = all host cores
 *   raht_rlgr_decode_channels : the inverse.
 *   raht_transpose_i32        : DEVICE int32 transpose (rows x cols, ld_in) -> (cols x rows, ld_out)
 *                               so that the host coder gets contiguous channels after the D2H copy. */
int64_t raht_rlgr_bound(int64_t n);
int raht_rlgr_encode(const int32_t *seq, int64_t n, int64_t stride, int flag_signed, uint8_t *out,
                     int64_t cap, int64_t *nbytes);
int raht_rlgr_decode(const uint8_t *buf, int64_t nbytes, int64_t n, int flag_signed, int32_t *seq,
                     int64_t stride);
int raht_rlgr_encode_channels(const int32_t *Q, int64_t N, int D, int64_t sym_stride, int64_t chan_stride,
                              int flag_signed, uint8_t *out, int64_t cap_per_channel, int64_t *nbytes,
                              int nthreads);
int raht_rlgr_decode_channels(const uint8_t *bufs, int64_t cap_per_channel, const int64_t *nbytes,
                              int64_t N, int D, int flag_signed, int32_t *Q, int64_t sym_stride,
                              int64_t chan_stride, int nthreads);
int raht_transpose_i32(const int32_t *in, int64_t ld_in, int64_t rows, int64_t cols, int32_t *out,
                       int64_t ld_out, raht_stream_t stream);
/* ------------------------------------------------------------------------------------------------
 * DIRECT all-gather for Morton-prefix sharded scenes (one process per GPU; SURVEY.md 5 / 8e: "a direct all-gather -- each
 * GPU writes its <= 15 KB slice to its 7 peers over the 7 point-to-point links -- beats a ring"). Opt-in alternative to
 * the RCCL all_gather_into_tensor of raht_3dgs_codec_amd.sharded (ShardedRaht(direct=True)); the reference has no
 * multi-GPU path at all.
 *   raht_xchg_alloc   : this rank's exchange block (fine-grained device memory: 2 x world x slot_bytes of data, double
 *                       buffered, + flags) and its 64-byte hipIpc handle, which the caller sends to the peers (once)
 *   raht_xchg_open    : map a peer's block from its handle;  raht_xchg_close / raht_xchg_free: undo
 *   raht_xchg_gather  : ONE launch (one workgroup per peer): write `send` into slot `rank` of buffer (seq & 1) of every
 *                       peer's block, raise the peer's flag, wait until every peer's slot has landed here. seq = 1, 2, 3, ...
 *                       identical on all ranks. Waits are bounded (20 s): a missing peer ends in status 1, not a hung GPU.
 *   raht_xchg_buffer  : device address of buffer (seq & 1): world slots of slot_bytes, slot r = rank r's rows
 *   raht_xchg_status  : (synchronises the stream) 0 = fine, 1 = a wait timed out
 * slot_bytes: a multiple of 16; world <= 8. */
int raht_xchg_bytes(int world, int64_t slot_bytes, int64_t *total);
int raht_xchg_alloc(int world, int64_t slot_bytes, void **base, void *handle64);
int raht_xchg_open(const void *handle64, void **base);
int raht_xchg_close(void *base);
int raht_xchg_free(void *base);
int raht_xchg_gather(const void *send, int64_t slot_bytes, void *const *peers, int rank, int world, uint32_t seq,
                     raht_stream_t stream);
int raht_xchg_buffer(void *base, int world, int64_t slot_bytes, uint32_t seq, void **buf);
int raht_xchg_status(void *base, int world, int64_t slot_bytes, raht_stream_t stream, int *status);

/* ------------------------------------------------------------------------------------------------
 * The RLGR stage ON THE GPU, segmented (csrc/rlgr_seg.hip; SURVEY.md 8f-1 "GPU-segmented"). Every channel is cut into
 * segments of seg_len symbols, every segment is an independent RLGR stream -- byte-identical to what the reference's
 * membuf::rlgrWrite (python/PyRLGR/src/libs/rlgr/membuf.cpp:340-423) emits for that slice of the channel, so any RLGR decoder
 * reads it -- and one lane codes one segment. The container (lengths + offsets + concatenated streams, 4-byte slots) is this
 * library's own: the reference codes a channel as ONE stream (raht_rlgr_encode_channels does exactly that, on the host).
 *   Q        : DEVICE int32, channel-major: symbol n of channel c at Q[c * chan_stride + n] (raht_transpose_i32's output)
 *   seg_bytes: DEVICE uint32[D * nseg], nseg = ceil(N / seg_len): exact stream length of segment c * nseg + s
 *   seg_off  : DEVICE uint32[D * nseg + 1]: its offset in `out` (slots padded to 4 bytes); the last entry = bytes used
 *   out      : DEVICE, 4-byte aligned, cap bytes. RAHT_ERR_NOMEM (and *total_bytes = what is needed) when cap is too small.
 * raht_rlgr_seg_encode synchronises the stream (it returns the size); raht_rlgr_seg_decode does not.
 *
 * DAMAGED PAYLOADS (every raht_rlgr_seg_decode* entry point below as well). The tables and the bytes come off the wire. A table
 * entry that reaches outside `in` is reported: that segment decodes as zeros, nothing of it is read, and its frame's bit of
 * *bad_dev is set. A PAYLOAD that is not what the encoder wrote -- cut short, a flipped bit, another segment's bytes, a length
 * that is shorter or (inside `in`) longer than the stream -- is not an error and is not reported: *bad_dev speaks of tables only
 * (with expect[], bits 16 + j report a frame that differs from what was expected, as for any other difference). The decoder
 * then still writes exactly the n symbols of that segment and nothing else -- every store is at a symbol i < n of the segment's
 * own place in Q, so every other segment holds what its own bytes say -- and reads only inside in[0, in_bytes): the words of the
 * segment's 4-byte slot and, through the aligned 32-byte pieces of the batch decoders, other words of the same container. Bits
 * past a segment's length read as zeros: the bytes behind it, in its last word and beyond, never count (an empty stream is
 * the pattern 0, 0, -1, -1, -1, 0, ..., not zeros). The symbols are the same on every entry point, in either layout, for either
 * table width, whatever the payload's alignment and whatever frames share the launch. They are the symbols the reference's
 * decoder (membuf.cpp:258-338) gives for the segment's bytes followed by zeros, with its runs stopped at symbol n, as long as
 * the decoder's state fits 32 bits: every Golomb-Rice value below 2^32, every symbol an int32, no run header doubled at k >= 31.
 * Past that the symbols are some definite garbage, still the same everywhere and inside the same bounds. */
int raht_rlgr_seg_encode(const int32_t *Q, int64_t N, int D, int64_t chan_stride, int seg_len, int flag_signed,
                         uint32_t *seg_bytes, uint32_t *seg_off, uint8_t *out, int64_t cap, int64_t *total_bytes,
                         raht_stream_t stream);
int raht_rlgr_seg_decode(const uint8_t *in, int64_t in_bytes, const uint32_t *seg_off, const uint32_t *seg_bytes, int64_t N,
                         int D, int seg_len, int flag_signed, int32_t *Q, int64_t chan_stride, uint32_t *bad_dev,
                         raht_stream_t stream);

/* The same coder on ANY of the two layouts of the quantized coefficients: channel-major (sym_stride = 1, chan_stride >= N: the
 * two functions above) or ROW-MAJOR (chan_stride = 1, sym_stride = ld >= D: symbol n of channel c at Q[n * ld + c], i.e. Q exactly
 * as raht_fwd_quant leaves it and raht_dequant_inv takes it -- no raht_transpose_i32 in front of the encoder or behind the
 * decoder: the lanes of a wave are then neighbouring channels at the same position of their segments, so every step of the wave
 * reads / writes one contiguous piece of a row). Same segments, same container, byte for byte. With these 32-bit offset tables the
 * container is limited to 4 GiB: inputs whose worst case could exceed it are refused (RAHT_ERR_INVALID) -- they go through
 * raht_rlgr_seg_encode64 / raht_rlgr_seg_decode64 below; raht_rlgr_seg_offsets_width says which of the two a shape needs. */
int raht_rlgr_seg_encode_strided(const int32_t *Q, int64_t N, int D, int64_t sym_stride, int64_t chan_stride, int seg_len,
                                 int flag_signed, uint32_t *seg_bytes, uint32_t *seg_off, uint8_t *out, int64_t cap,
                                 int64_t *total_bytes, raht_stream_t stream);
int raht_rlgr_seg_decode_strided(const uint8_t *in, int64_t in_bytes, const uint32_t *seg_off, const uint32_t *seg_bytes, int64_t N,
                                 int D, int seg_len, int flag_signed, int32_t *Q, int64_t sym_stride, int64_t chan_stride,
                                 uint32_t *bad_dev, raht_stream_t stream);

/* Frames of any size: 64-BIT OFFSET TABLES. The 32-bit entry points above refuse every shape whose WORST case
 * ((raht_rlgr_bound(seg_len) + 4) * D * nseg bytes: every symbol an escape) reaches 4 GiB -- at seg_len = 2048 that is
 * N x D >= 330 M symbols, e.g. 6 M x 56 -- because their offsets and totals could wrap. The container on the wire never
 * held offsets (a length per segment, uint32, and an int64 payload size), so only the device-side table changes width:
 *   raht_rlgr_seg_offsets_width : HOST arithmetic, no device call. 32: the 32-bit entry points take (N, D, seg_len); 64: they
 *                                 refuse it for its size and the *64 ones are needed; RAHT_ERR_INVALID: nobody takes it (N < 1,
 *                                 D < 1, seg_len < 64, 2^31 segments or more, a seg_len whose worst-case segment does not fit
 *                                 the uint32 length table). The one place the rule lives.
 *   raht_rlgr_seg_encode64      : raht_rlgr_seg_encode_strided with seg_off: DEVICE uint64[D * nseg + 1]. Takes EVERY valid
 *                                 shape, small ones too, and then writes the same seg_bytes and the same streams as the 32-bit
 *                                 form, offsets equal as integers. *total_bytes and the size RAHT_ERR_NOMEM reports may be
 *                                 4 GiB and more. Synchronises.
 *   raht_rlgr_seg_decode64      : raht_rlgr_seg_decode_strided from such a table. An offset is checked against in_bytes as the
 *                                 64-bit number it is (alignment, past the end, length past the end) before anything is
 *                                 read: a bad entry decodes as zeros and sets *bad_dev. Does not synchronise.
 * Everything else -- layouts, argument rules, one pass into slots + compaction with the two exact passes behind it -- is that
 * of the 32-bit forms; lengths stay uint32. */
int raht_rlgr_seg_offsets_width(int64_t N, int D, int seg_len);
int raht_rlgr_seg_encode64(const int32_t *Q, int64_t N, int D, int64_t sym_stride, int64_t chan_stride, int seg_len,
                           int flag_signed, uint32_t *seg_bytes, uint64_t *seg_off, uint8_t *out, int64_t cap,
                           int64_t *total_bytes, raht_stream_t stream);
int raht_rlgr_seg_decode64(const uint8_t *in, int64_t in_bytes, const uint64_t *seg_off, const uint32_t *seg_bytes, int64_t N,
                           int D, int seg_len, int flag_signed, int32_t *Q, int64_t sym_stride, int64_t chan_stride,
                           uint32_t *bad_dev, raht_stream_t stream);

/* k frames of ONE shape in one set of launches -- the quantization steps of a frame (python/encode_3dgs.py:199-275 codes them one
 * after the other; nothing connects them). One frame of 3 M x 56 symbols is 1.25 waves per SIMD of independent streams, and the
 * coder's time is that of one wave walking its segments; k frames behind blockIdx.y fill the chip's wave slots. Arrays of k
 * HOST pointers / sizes; every frame keeps its own tables and container and gets EXACTLY the bytes the one-frame entry points
 * above leave for it (same layouts, same limits per frame, 1 <= k <= RAHT_RLGR_BATCH_MAX). The encoder synchronises and
 * fills total_bytes[k] (RAHT_ERR_NOMEM: some cap[j] < total_bytes[j]); the decoder does not synchronise and sets bit j of
 * *bad_dev when a table entry of frame j reached outside in[j]. */
#define RAHT_RLGR_BATCH_MAX 12
int raht_rlgr_seg_encode_batch(int k, const int32_t *const *Q, int64_t N, int D, int64_t sym_stride, int64_t chan_stride, int seg_len,
                               int flag_signed, uint32_t *const *seg_bytes, uint32_t *const *seg_off, uint8_t *const *out,
                               const int64_t *cap, int64_t *total_bytes, raht_stream_t stream);
int raht_rlgr_seg_decode_batch(int k, const uint8_t *const *in, const int64_t *in_bytes, const uint32_t *const *seg_off,
                               const uint32_t *const *seg_bytes, int64_t N, int D, int seg_len, int flag_signed, int32_t *const *Q,
                               int64_t sym_stride, int64_t chan_stride, uint32_t *bad_dev, raht_stream_t stream);
/* The same, ROW-MAJOR frames only (chan_stride = 1), with the drivers' round-trip assertion (python/encode_3dgs.py:242-245: what was
 * decoded equals what was encoded) inside the decoder: expect[j] (DEVICE, layout and strides of Q[j]) is compared symbol by symbol
 * on the way out -- in this layout one more contiguous read per iteration of a wave -- and bit 16 + j of *bad_dev (required) is set
 * when frame j differs. Replaces a comparison pass over two N x D arrays per frame. */
int raht_rlgr_seg_decode_batch_check(int k, const uint8_t *const *in, const int64_t *in_bytes, const uint32_t *const *seg_off,
                                     const uint32_t *const *seg_bytes, int64_t N, int D, int seg_len, int flag_signed,
                                     int32_t *const *Q, const int32_t *const *expect, int64_t sym_stride, int64_t chan_stride,
                                     uint32_t *bad_dev, raht_stream_t stream);

/* The batch entry points with 64-bit offset tables (seg_off[j]: DEVICE uint64[D * nseg + 1]), for the shapes
 * raht_rlgr_seg_offsets_width calls 64 and any other. raht_rlgr_seg_encode_batch64 = raht_rlgr_seg_encode_batch.
 * raht_rlgr_seg_decode_batch64 is both decoders: expect == NULL decodes as raht_rlgr_seg_decode_batch does (either layout,
 * bad_dev may be NULL); otherwise as raht_rlgr_seg_decode_batch_check (row-major frames, bad_dev required, no expect[j] NULL). */
int raht_rlgr_seg_encode_batch64(int k, const int32_t *const *Q, int64_t N, int D, int64_t sym_stride, int64_t chan_stride,
                                 int seg_len, int flag_signed, uint32_t *const *seg_bytes, uint64_t *const *seg_off,
                                 uint8_t *const *out, const int64_t *cap, int64_t *total_bytes, raht_stream_t stream);
int raht_rlgr_seg_decode_batch64(int k, const uint8_t *const *in, const int64_t *in_bytes, const uint64_t *const *seg_off,
                                 const uint32_t *const *seg_bytes, int64_t N, int D, int seg_len, int flag_signed,
                                 int32_t *const *Q, const int32_t *const *expect, int64_t sym_stride, int64_t chan_stride,
                                 uint32_t *bad_dev, raht_stream_t stream);

/* k frames of k SHAPES in one set of launches -- the frames of a sequence: a different voxel count in every frame, D, seg_len and
 * flag_signed shared. N[j], sym_stride[j], chan_stride[j]: HOST arrays of k entries; all frames channel-major or all row-major,
 * each within the stride rules of raht_rlgr_seg_encode_strided. 32-bit offset tables only: a frame for which
 * raht_rlgr_seg_offsets_width(N[j], D, seg_len) is not 32 is refused (RAHT_ERR_INVALID, the text names the frame) -- such a
 * frame fills the chip alone. The contract is that of the same-shape batch, which is this launch with N[j] = N: every frame gets
 * EXACTLY the bytes, seg_bytes, seg_off (its closing entry seg_off[D * nseg_j] included) and total_bytes[j] that
 * raht_rlgr_seg_encode_strided leaves for it alone. The encoder synchronises and fills total_bytes[k] (RAHT_ERR_NOMEM: some
 * cap[j] < total_bytes[j]); a segment that outgrows its slot sends the call to the exact passes, frame by frame. The decoder does
 * not synchronise; it sets bit j of *bad_dev when a table entry of frame j reached outside in[j] (that segment decodes as zeros)
 * and, with expect != NULL (row-major frames only, bad_dev required, no expect[j] NULL), bit 16 + j when frame j differs from
 * expect[j]. */
int raht_rlgr_seg_encode_ragged(int k, const int32_t *const *Q, const int64_t *N, int D, const int64_t *sym_stride,
                                const int64_t *chan_stride, int seg_len, int flag_signed, uint32_t *const *seg_bytes,
                                uint32_t *const *seg_off, uint8_t *const *out, const int64_t *cap, int64_t *total_bytes,
                                raht_stream_t stream);
int raht_rlgr_seg_decode_ragged(int k, const uint8_t *const *in, const int64_t *in_bytes, const uint32_t *const *seg_off,
                                const uint32_t *const *seg_bytes, const int64_t *N, int D, int seg_len, int flag_signed,
                                int32_t *const *Q, const int32_t *const *expect, const int64_t *sym_stride,
                                const int64_t *chan_stride, uint32_t *bad_dev, raht_stream_t stream);

/* The SIZE of that container at k quantization steps, and the squared quantization error beside it, from ONE read of the
 * coefficients (csrc/rlgr_rate.hip): the rate-distortion curve of a frame without a quantized matrix, a slot buffer or a stream
 * being written. A lane walks one segment of one channel and advances up to RAHT_RLGR_RATE_MAX independent coder states, each
 * quantizing the coefficient it loaded with its own step and COUNTING the bits the coder above would emit (larger k: several
 * passes, RAHT_RLGR_RATE_MAX steps each).
 *   T        : DEVICE, N x D coefficients of dtype RAHT_F32 or RAHT_F64 in CODED order (row i is row i of the quantized matrix:
 *              behind the order_RAGFT reorder), row-major, row stride ldt >= D elements
 *   steps    : HOST, k x n_steps values of T's dtype, n_steps 1 or D: step j of channel c = steps[j * n_steps + (n_steps == 1 ? 0 : c)]
 *   seg_bytes: DEVICE uint32[k * G], G = D * ceil(N / seg_len), segment g = c * nseg + s as above. seg_bytes[j * G + g] = unpadded
 *              length of the RLGR stream of q = floor(T / step_j + 0.5) over symbols [s * seg_len, min(N, (s + 1) * seg_len)) of channel
 *              c: entry for entry the seg_bytes table raht_rlgr_seg_encode_strided leaves for the matrix raht_quant_rows (float32) /
 *              raht_quant_rows_f64 (float64) makes of the same T and step. The container of step j then takes
 *              8 + 40 + 4 G + sum over g of ((seg_bytes[j * G + g] + 3) & ~3) bytes.
 *   seg_sse  : DEVICE double[k * G] or NULL (not computed): seg_sse[j * G + g] = sum over the segment's symbols, in symbol order,
 *              of ((double)T - (double)q * (double)step_j)^2 -- a fixed order: deterministic.
 * RAHT_ERR_INVALID (nothing enqueued, no device touched): T, steps or seg_bytes NULL; an unknown dtype; N < 1, D < 1, ldt < D, k < 1,
 * n_steps not 1 or D; a (N, D, seg_len) raht_rlgr_seg_encode_strided refuses (seg_len < 64, 2^31 segments, a worst case of 4 GiB);
 * flag_signed not 0 or 1; a step that is not finite and positive, or, float32, outside [2^-100, 2^100] (the range in which the
 * float32 quantizer's division needs no scaling). Quotients beyond int32 saturate, as in every quantizer of this library (the out-of-range rule at raht_quant_reorder);
 * the squared error is that of the saturated integer.
 * Device memory: the k * n_steps steps, nothing else. Enqueues only: `steps` goes to the device with an asynchronous copy on
 * `stream`, which has read pageable memory by the time the call returns; a table in page-locked memory must stay unchanged
 * until the stream has passed this call. */
#define RAHT_RLGR_RATE_MAX 8     /* steps walked per pass; larger k is chunked inside */
int raht_rlgr_seg_rate(const void *T, int dtype, int64_t ldt, int64_t N, int D, const void *steps, int k, int n_steps, int seg_len,
                       int flag_signed, uint32_t *seg_bytes, double *seg_sse, raht_stream_t stream);

/* How the decoders' symbols leave the lanes: -1 = chosen by the number of lanes in flight (default: one 4-byte store per symbol
 * below 200 000 lanes, where the L2 still gathers a lane's line; above, a 16-word LDS column per lane written out as aligned
 * 64-byte pieces -- with the steps of a frame decoded together the one-word stores cost 5.9 x the symbols' bytes in HBM writes),
 * 0 = words, 2 = LDS columns. Row-major output: 4 = from the per-lane decoder with strided stores, 3 = from the symbol-synchronous
 * one again (the default). Any other value restores the default, as -1 does. Same output in every mode (tests walk all of them); a
 * testing hook, process-wide. Returns the previous setting. */
int raht_debug_rlgr_decode_out(int mode);
/* The same for the words of the ENCODER's streams on their way into its slots (one frame or k, by the lanes in flight as above):
 * -1 = by the lanes in flight, 0 = one 4-byte store per word, 2 = LDS columns, 64-byte pieces (9 steps of a 3 M x 56 frame:
 * 0.79 -> 0.71 ms per step). */
int raht_debug_rlgr_encode_out(int mode);
/* Tile stages whose butterfly heights one launch computes while a schedule is built (default 8, the most a launch holds): a
 * smaller n makes ordinary schedules walk the several-launches path that only very deep ones reach. n = 0 or out of [1, 8]
 * restores the default. While a non-default value is set, the heights are launched behind the schedule builder's read-back
 * instead of in front of it. Same schedules, same transforms; a testing hook, process-wide. Returns the previous value. */
int raht_debug_height_stages_per_launch(int n);
/* The form the key sort takes (csrc/scan_sort.hip), for the tests and tools that walk every form of one sort:
 *   onesweep  : 1 = one launch per digit pass with look-back between the tiles (default), 0 = pass by pass, four launches per digit
 *   rounds    : items per lane of a one-sweep tile, 8 / 12 / 16 = tiles of 2048 / 3072 / 4096 items; 0 = chosen by N (default)
 *   fail_tile : this tile of every one-sweep pass gives up as if its bounded wait had run out (the tiles behind it pass the
 *               error on, the grid drains, the call repeats the sort pass by pass and raht_sort_fallbacks() grows);
 *               < 0 = none (default), at most 2^24 - 1
 * Same keys and permutation in every form. A testing hook, process-wide; a sort reads it once, when it is called. Returns the
 * previous form packed as onesweep | rounds << 1 | (fail_tile + 1) << 6 (never negative), so that
 * raht_debug_sort_form(p & 1, (p >> 1) & 31, (p >> 6) - 1) restores it; RAHT_ERR_INVALID (nothing changed) for any other
 * rounds or a larger fail_tile. */
int raht_debug_sort_form(int onesweep, int rounds, int64_t fail_tile);
/* Device blocks of the library's block cache that are handed out and not yet given back (plan arrays, schedules, workspaces
 * of every live plan, on every device). Scratch-pool blocks and borrowed key arrays are not counted. A testing hook: after a plan
 * is destroyed, or a constructor has failed, the count is what it was before. */
int64_t raht_debug_live_blocks(void);
/* Freed blocks the cache currently keeps (what raht_release_cached_memory() would return to HIP), on every device. */
int64_t raht_debug_cached_blocks(void);
/* The form raht_motion_search takes for rows of D floats: the rows of a workgroup's tile whose weighted columns are staged in LDS
 * -- 256 for D <= 59, 192 for D <= 79, 128 for D <= 121, 64 for D <= 243 -- or 0 when no tile fits and X is read through the cache
 * (256 rows per workgroup step then); 0 for D < 1 too. The entry point calls the same function. Host only, no GPU work; a testing
 * hook: the tests assert the form they mean to exercise. */
int raht_debug_motion_tile(int D);

/* out[c] = sum over rows of (A[i, c] - B[i, c])^2, DEVICE double[D]: what the drivers' five PSNR columns are made of
 * (python/encode_3dgs.py:298-310: torch.mean((C - C_rec) ** 2) over all / quats / scales / opacity / colour columns -- each a
 * sum of these D numbers divided by the element count). A, B: N x D DEVICE matrices of dtype RAHT_F32 or RAHT_F64 (differences
 * in that type, squares and sums in float64, deterministic). Two launches, no host round trip. */
int raht_sqdiff_columns(const void *A, int64_t lda, const void *B, int64_t ldb, int64_t N, int D, int dtype, double *out,
                        raht_stream_t stream);

/* Host: are two contiguous int32 arrays equal? *first_diff = index of the first difference or -1. Threaded (the drivers'
 * round-trip assertion, python/encode_3dgs.py:242-245, on 10^8 symbols). */
int raht_i32_equal(const int32_t *a, const int32_t *b, int64_t n, int nthreads, int64_t *first_diff);

/* ------------------------------------------------------------------------------------------------
 * Octree geometry (csrc/octree.hip): the lossless code of the occupied voxels, i.e. of the sorted Morton keys every plan is
 * built from. With it a frame leaves the machine as bytes that decode on their own (python: geometry.py, bitstream.py).
 *
 * Input: N >= 1 strictly ascending keys < 8^J, 1 <= J <= 21, digits as raht_morton writes them (digit = z + 2 y + 4 x, the
 * finest digit in bits 0-2).
 *   node of level g (0 = root ... J = voxel) : a distinct value of key >> 3 (J - g); n_g of them, n_0 = 1, n_J = N
 *   occupancy byte of an internal node       : bit d set <=> the child with digit d exists (never 0)
 *   occupancy stream                         : the bytes of level 0, then level 1, ... level J - 1, ascending key order inside
 *                                              a level; n_nodes = n_0 + ... + n_(J-1) bytes
 *   geometry section  : "OCTG0001" | int64 J, N, mode, n_nodes, seg_len | int64 n_0 ... n_J | body
 *                       mode 0: the n_nodes bytes. mode 1: byte_of_rank[256], then the body of a segmented RLGR container
 *                       (raht_rlgr_seg_*) of ONE unsigned channel of n_nodes symbols: the uint32 length of every segment, then
 *                       the streams in 4-byte slots. Symbol = rank of the occupancy byte; ranks by descending count over the
 *                       whole stream, ties by ascending byte value, so the table is unique. Byte 0 never occurs: its rank is the
 *                       number of byte values in use, and a symbol at or above it is an error.
 *   frame container   : "RAHTF001" | int64 J, N, D, n_wide, n_steps | float64 steps[n_steps] | float64 vmin[3], width |
 *                       int64 length + geometry section | int64 length + the attribute container ("RLGS0001" ...).
 *                       n_wide = 0: the float32 path (raht_fwd_quant / raht_dequant_inv, steps cast to float32 on both sides);
 *                       n_wide > 0: the mixed path (raht_fwd_quant_mixed / raht_dequant_inv_mixed, float64 steps).
 *
 *   raht_octree_counts  : counts[0 .. J] (HOST) = n_0 ... n_J from one pass over the keys, which also checks them:
 *                         RAHT_ERR_INVALID when they are not strictly ascending or not below 8^J. Synchronises (it returns sizes).
 *   raht_octree_encode  : occ[n_nodes] from the keys and the counts of raht_octree_counts. Level by level, bottom-up; enqueues only.
 *   raht_octree_decode  : keys[counts[J]] from the stream. counts (HOST) come from a header: they must satisfy n_0 = 1,
 *                         n_g <= n_(g+1) <= 8 n_g < 2^31 (RAHT_ERR_INVALID otherwise) and size everything -- no synchronisation,
 *                         and EVERY store is bounded by them whatever the bytes say. A zero byte, or a level whose popcounts do
 *                         not add up to the next count, sets *bad (DEVICE int32, never cleared here); keys then hold garbage.
 *   raht_octree_symbols : sym[i] (DEVICE int32) = rank of occ[i]; byte_of_rank[256] (HOST) = the table. Synchronises.
 *   raht_octree_bytes   : the inverse with a table from a header (HOST; must be a permutation of 0 .. 255); a symbol outside
 *                         the ranks in use sets *bad and decodes as 0. Enqueues only.
 *   raht_demorton       : V (N x 3 int64) from keys: the inverse of raht_morton.
 * All pointers DEVICE unless marked HOST; sym 4-byte aligned. */
int raht_octree_counts(const uint64_t *keys_sorted, int64_t N, int J, int64_t *counts, raht_stream_t stream);
int raht_octree_encode(const uint64_t *keys_sorted, int64_t N, int J, const int64_t *counts, uint8_t *occ, raht_stream_t stream);
int raht_octree_decode(const uint8_t *occ, const int64_t *counts, int J, uint64_t *keys, int32_t *bad, raht_stream_t stream);
int raht_octree_symbols(const uint8_t *occ, int64_t n_nodes, uint8_t *byte_of_rank, int32_t *sym, raht_stream_t stream);
int raht_octree_bytes(const int32_t *sym, int64_t n_nodes, const uint8_t *byte_of_rank, uint8_t *occ, int32_t *bad,
                      raht_stream_t stream);
int raht_demorton(const uint64_t *keys, int64_t N, int J, int64_t *V, raht_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Predicted octree geometry (csrc/octree_inter.hip): a frame's occupancy stream coded against the REFERENCE frame's occupancy of
 * the same cells (python: geometry.OctreeCoder.encode / decode with ref_keys; bitstream.encode_sequence_bytes(...,
 * geometry_inter)). Where part of a scene stands still most residual bytes are 0.
 *
 * The frame: N strictly ascending keys k < 8^J. The reference: N_ref >= 1 strictly ascending keys r of the same J.
 *   pred[v]  for the node v of level g (0 <= g < J) with cell key c, s = 3 (J - g): the reference's occupancy byte of the same
 *            cell -- bit d set <=> some r[i] has r[i] >> (s - 3) == 8 c + d; 0 where the reference has no voxel in the cell
 *   res[v]   = occ[v] ^ pred[v], in the order of the occupancy stream (level 0 first, ascending key inside a level)
 *   predicted section : "OCTP0001" | int64 J, N, mode, n_nodes, seg_len, N_ref, n_used | int64 n_0 ... n_J | body
 *                       The body is laid out as in "OCTG0001". mode 0: the n_nodes residual bytes (n_used = 0). mode 1:
 *                       byte_of_rank[256], the uint32 length of every RLGR segment, the streams in 4-byte slots; the ranks follow
 *                       the rule of raht_octree_symbols applied to res. Byte 0 is an ordinary value here (normally rank 0), so the
 *                       header carries n_used, the number of byte values that occur (1 .. 256): a symbol >= n_used is an error.
 *
 *   raht_octree_encode_inter : res[n_nodes] from the keys, the counts of raht_octree_counts and the reference's keys. The
 *                              bottom-up walk of raht_octree_encode, every level's bytes XORed with pred. Enqueues only.
 *   raht_octree_decode_inter : keys[counts[J]] from res. Top-down: at level g pred of the level's node keys, occ = res ^ pred, then
 *                              the expansion of raht_octree_decode, under its rules: counts (HOST) from a header size everything,
 *                              EVERY store is bounded by them whatever the bytes say; a reconstructed byte of 0, or popcounts
 *                              that do not add up to the next count, set *bad. Enqueues only.
 *   raht_octree_bytes_used   : raht_octree_bytes with the number of ranks in use taken from the header (n_used, 1 .. 256), not from
 *                              the position of byte 0. The encoder's side is raht_octree_symbols unchanged.
 * No atomics; deterministic. The reference's keys are not checked here (a sequence coder hands in keys that raht_octree_counts
 * has seen): keys out of order give a pred that means nothing, possibly another one in the decoder -- *bad then -- but no search
 * leaves [0, N_ref). RAHT_ERR_INVALID with nothing enqueued: J outside 1 .. 21, N or N_ref outside 1 .. 2^31 - 1,
 * NULL pointers, counts that fail the rules of raht_octree_decode (encode: counts[J] != N), n_used outside 1 .. 256.
 * All pointers DEVICE unless marked HOST. */
int raht_octree_encode_inter(const uint64_t *keys_sorted, int64_t N, int J, const int64_t *counts, const uint64_t *ref_keys,
                             int64_t N_ref, uint8_t *res, raht_stream_t stream);
int raht_octree_decode_inter(const uint8_t *res, const int64_t *counts, int J, const uint64_t *ref_keys, int64_t N_ref, uint64_t *keys,
                             int32_t *bad, raht_stream_t stream);
int raht_octree_bytes_used(const int32_t *sym, int64_t n_nodes, const uint8_t *byte_of_rank, int n_used, uint8_t *res, int32_t *bad,
                           raht_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Regions of a frame (csrc/region.hip): where the rows of a run of octree cells lie in the frame's coded order, so that a decoder
 * can rebuild them from the segments that hold them (python: bitstream.decode_region_bytes).
 *
 * Buckets: a row i >= 1 has bucket msb(key[i] ^ key[i-1]) / 3 (0 .. 20), row 0 has bucket 21 = RAHT_REGION_BUCKETS - 1. The coded
 * order of a frame (order_RAGFT) is the stable sort of its rows by DESCENDING bucket. For the cells of octree depth d of a frame
 * of depth J, top_level = 3 (J - d): the rows of the buckets >= J - d are the first rows of the occupied depth-d cells, and they
 * are the first coded rows; in every bucket below, the rows [row_lo, row_hi) of a run of such cells are ONE run of coded rows.
 * keys_sorted: N >= 1 strictly ascending keys below 2^nbits, 1 <= nbits <= 63 (what raht_plan_create_from_keys takes; not checked
 * again here).
 *   raht_region_layout   : table (DEVICE int64[3 * RAHT_REGION_BUCKETS]) = rows per bucket in the whole frame, in [0, row_lo) and
 *                          in [row_lo, row_hi), from one pass over the keys. Enqueues only (a memset and one launch).
 *   raht_region_cells    : the rows with i == 0 or msb(key[i] ^ key[i-1]) >= top_level, in row order: cell_keys[j] = key >>
 *                          top_level (DEVICE uint64[n_cells]), cell_first[j] = the row (DEVICE int64[n_cells + 1], the last entry
 *                          N). n_cells is the caller's expectation (the level count of a geometry header); every store is
 *                          bounded by it, and a different count is RAHT_ERR_INVALID. SYNCHRONISES `stream` (it reads the count
 *                          back). top_level: a multiple of 3 in [3, nbits - 3].
 *   raht_region_assemble : dst (n_dst_rows x D int32, row stride ld_dst) from runs of rows of src (n_src_rows x D int32, row
 *                          stride ld_src): runs (HOST int64[3 * n_runs], n_runs <= RAHT_REGION_BUCKETS) holds (src_row, dst_row,
 *                          count) triples with ascending, disjoint destinations; they travel to the kernel by value. dst rows
 *                          that no run covers are set to 0. One launch, enqueues only.
 * RAHT_ERR_INVALID, with nothing enqueued: NULL pointers, N < 1, row_lo > row_hi or row_hi > N, nbits or top_level out of range,
 * a run that leaves either matrix. */
#define RAHT_REGION_BUCKETS 22
int raht_region_layout(const uint64_t *keys_sorted, int64_t N, int nbits, int64_t row_lo, int64_t row_hi, int64_t *table,
                       raht_stream_t stream);
int raht_region_cells(const uint64_t *keys_sorted, int64_t N, int nbits, int top_level, int64_t n_cells, uint64_t *cell_keys,
                      int64_t *cell_first, raht_stream_t stream);
int raht_region_assemble(const int32_t *src, int64_t ld_src, int64_t n_src_rows, int32_t *dst, int64_t ld_dst, int64_t n_dst_rows, int D,
                         const int64_t *runs, int n_runs, raht_stream_t stream);

/* A SET of row ranges (python: bitstream.decode_cells_bytes, decode_sequence_region). The rows of R ascending,
 * disjoint runs of depth-d cells, concatenated, are the region; its own coded order (the plan over the concatenated keys,
 * truncated at top_level) keeps the first row of every cell in the root part and, in a finer bucket, holds range 0's rows of the
 * bucket, then range 1's, and so on: one run of coded rows per (bucket, range).
 *   raht_region_layout_set   : row_bounds (DEVICE int64[2 R]: lo_0, hi_0, lo_1, ..., ascending, 0 <= lo_r <= hi_r <= lo_(r+1) <= N;
 *                              1 <= R <= RAHT_REGION_MAX_RANGES) -> table (DEVICE int64[(1 + 2 R) * RAHT_REGION_BUCKETS]): rows per
 *                              bucket in the whole frame, then for every range in [0, lo_r) and in [lo_r, hi_r). One pass over the
 *                              keys whatever R is; integer sums. For R = 1 it is raht_region_layout's table. The bounds are not
 *                              read on the host: bounds that do not ascend give counts that mean nothing, and nothing else.
 *                              Enqueues only (a memset and two launches).
 *   raht_region_assemble_set : raht_region_assemble with the table in device memory: runs (DEVICE int64[3 * n_runs], n_runs <=
 *                              RAHT_REGION_BUCKETS * RAHT_REGION_MAX_RANGES), destinations ascending and disjoint. runs_host (HOST,
 *                              may be NULL): the caller's copy of the same table, held to raht_region_assemble's rules before
 *                              anything is enqueued. Whatever the device table holds, the kernel clamps every source row into src
 *                              and writes the n_dst_rows rows of dst only. One launch, enqueues only.
 *   raht_region_needs        : the depth-d cells (top_level = 3 (J - d)) of ANOTHER frame that a prediction of these rows reaches
 *                              into: cells (DEVICE uint64[capacity]) = the ascending, duplicate-free values of
 *                              (k' >> w) << (w - top_level), w = max(top_level, 3 up), over the rows i with a match, k' being the
 *                              shifted key of "Motion compensation" below under the field mv (block_first, n_blocks, block_log2 as
 *                              raht_predict_mc takes them), or k[i] itself when mv is NULL (block_first is then not read). Where
 *                              3 up > top_level a value stands for the aligned group of 8^(up - (J - d)) cells that starts with
 *                              it; widening it is the caller's. *n_cells (HOST) = their number; every store is bounded by
 *                              capacity, and a larger number is RAHT_ERR_INVALID (with *n_cells set). SYNCHRONISES `stream`. */
#define RAHT_REGION_MAX_RANGES 512
int raht_region_layout_set(const uint64_t *keys_sorted, int64_t N, int nbits, const int64_t *row_bounds, int R, int64_t *table,
                           raht_stream_t stream);
int raht_region_assemble_set(const int32_t *src, int64_t ld_src, int64_t n_src_rows, int32_t *dst, int64_t ld_dst, int64_t n_dst_rows, int D,
                             const int64_t *runs, const int64_t *runs_host, int n_runs, raht_stream_t stream);
int raht_region_needs(const uint64_t *keys_sorted, int64_t N, int J, int top_level, int up, const int64_t *block_first, int64_t n_blocks,
                      const int8_t *mv, int block_log2, uint64_t *cells, int64_t capacity, int64_t *n_cells, raht_stream_t stream);

/* The needed sets of a B frame (python: bitstream.decode_sequence_cells): for the rows keys_sorted of a frame with two
 * references -- or of a region of one --, the cells of reference 0 (cells0) and of reference 1 (cells1) that the two-reference
 * predictor ("Two references" and "Block modes" below) can reach into, from ONE pass over the keys. cells_r (DEVICE
 * uint64[capacity]) holds raht_region_needs' entries for reference r -- (k' >> w) << (w - top_level), w = max(top_level, 3 up),
 * ascending and duplicate-free -- over the rows whose voxel, shifted by the vector mv_r of the row's block, stays in the cube AND
 * whose block's mode uses reference r: mode 0 uses both references, 1 reference 0 alone, 2 reference 1 alone, 3 neither; a mode byte
 * above 3 counts as 3. mv0, mv1 (DEVICE int8[3 n_blocks]) and mode (DEVICE uint8[n_blocks]) may each be NULL: a zero field, every
 * block in mode 0. block_first (DEVICE int64[n_blocks], rows of keys_sorted), n_blocks and block_log2 are required as soon as one of
 * the three is given, under raht_region_needs' rules, and are not read otherwise. n_cells (HOST int64[2]) = the two counts; every
 * store is bounded by capacity, and a larger count in either list is RAHT_ERR_INVALID (with both counts set). With mode NULL and
 * mv1 == mv0 both lists are raht_region_needs' under that field, with all three NULL its answer without one. SYNCHRONISES `stream`.
 * RAHT_ERR_INVALID, with nothing enqueued, for what raht_region_needs refuses; more than 2^31 - 1 candidate cells (N >= 2^30 rows)
 * are refused as well. */
int raht_region_needs_bi(const uint64_t *keys_sorted, int64_t N, int J, int top_level, int up, const int64_t *block_first, int64_t n_blocks,
                         int block_log2, const int8_t *mv0, const int8_t *mv1, const uint8_t *mode, uint64_t *cells0, uint64_t *cells1,
                         int64_t capacity, int64_t *n_cells, raht_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Inter-frame prediction (csrc/predict.hip): a frame of a sequence predicted from the RECONSTRUCTION of another one, so that only
 * the residual is coded (python: bitstream.encode_sequence_bytes(..., gop, up, inter) / decode_sequence_bytes).
 *
 * The predictor. keys_sorted: the N strictly ascending keys of the frame; ref_keys_sorted / C_ref: the N_ref strictly ascending
 * keys of the reference frame (the same depth) and its N_ref x D float32 attributes, row stride ld_ref. shift = 3 up, up = 0 .. 3.
 * Row i lies in the cell c = key[i] >> shift; its run [lo, hi) in the reference is every row r with ref_key[r] >> shift == c
 * (contiguous: the keys are sorted; at most 8^up rows). P[i, ch] = 0 for an empty run; otherwise s = C_ref[lo, ch], then
 * s = s + C_ref[r, ch] for r = lo + 1 .. hi - 1 in this order in float32, and P[i, ch] = s / (float)(hi - lo), one IEEE division.
 * The order of the sum is part of the definition: encoder and decoder, and every implementation, give the same bits. With
 * shift = 0 the prediction is the co-located voxel's row, exactly.
 *   raht_predict : Y (N x D, row stride ldy) = X - P (add = 0) or X + P (add = 1), one float32 operation per element; Y = P when X
 *                  is NULL. Y may be X (in place). n_matched (DEVICE int64, may be NULL) = the number of rows with a non-empty run.
 *                  One launch (and a memset when n_matched is given); enqueues only, never synchronises.
 * RAHT_ERR_INVALID, with nothing enqueued: NULL keys / ref keys / C_ref / Y, N or N_ref outside 1 .. 2^31 - 1, shift not one of
 * 0, 3, 6, 9, D < 1, a row stride below D, add not 0 or 1.
 *
 *   predicted frame   : "RAHTP001" | int64 ref_back (>= 1: the reference is ref_back frames earlier; encoders write 1) |
 *                       int64 up (0 .. 3) | a whole "RAHTF001" frame container whose attributes are the residual X - P.
 *                       It exists only inside a sequence container ("RAHTS001"), never at index 0; its reconstruction is the
 *                       inner frame's plus P of the reference's reconstruction. */
int raht_predict(const uint64_t *keys_sorted, int64_t N, const uint64_t *ref_keys_sorted, int64_t N_ref, int shift, const float *C_ref,
                 int64_t ld_ref, const float *X, int64_t ldx, int D, int add, float *Y, int64_t ldy, int64_t *n_matched,
                 raht_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Motion compensation (csrc/motion.hip): the predictor above follows a motion field, one integer vector per block, and a block
 * search finds the field (python: ops.motion_search / ops.predict_mc, bitstream.encode_sequence_bytes(..., motion, block_log2,
 * motion_weights)).
 *
 * Blocks. The frame has depth J and N strictly ascending keys k[0 .. N); block_log2 = m, 1 <= m <= J. The block of row i is
 * k[i] >> 3 m. The occupied blocks, ascending, are n_blocks = n_(J - m) of the geometry header's level counts, and
 * block_first[0 .. n_blocks] (DEVICE int64; the last entry N) is cell_first of raht_region_cells(keys, N, 3 J, top_level = 3 m,
 * n_blocks, ...) (m = J: one block, block_first = {0, N}).
 * Shifted key. Digits as raht_morton writes them (digit = z + 2 y + 4 x, the finest digit in bits 0-2). (x, y, z) = the voxel
 * of k[i], v = (dx, dy, dz), sums in int64. If x + dx, y + dy or z + dz lies outside [0, 2^J), row i has NO MATCH under v;
 * otherwise k' = the key of (x + dx, y + dy, z + dz). v points from the current voxel to the reference voxel: a cloud translated
 * by t between the reference and the current frame has v = -t.
 * Compensated prediction. P_v[i, :] is raht_predict's P evaluated for the key k' instead of k[i], with the same shift = 3 up: the
 * run ref_key[r] >> shift == k' >> shift, the sequential float32 sum in row order, one IEEE division; 0 for an empty run and for
 * a row with no match. With a motion field mv[n_blocks][3] (int8), row i uses v = mv[block(i)]; with mv = 0 this is raht_predict
 * bit for bit.
 * Cost of a candidate. weights w[D] (DEVICE float32, finite and >= 0: the caller's contract) and candidates cand[K][3] (DEVICE
 * int32, 1 <= K <= 512). Row cost: c = 0.0f; for ch ascending with w[ch] != 0: t = fl(X[i, ch] - P_v[i, ch]); t = |t|;
 * t = fl(w[ch] t); c = fl(c + t) -- the product is rounded before the sum, nothing is fused; columns of weight 0 are not read.
 * q = (uint64) floorf(fminf(c, 1048576.0f) * 1024.0f): +inf and NaN take the cap 2^30 (fminf(NaN, x) = x), the product is exact.
 * cost[b][k] = the sum of q over the rows of block b: an integer sum, independent of order and of how rows are split up.
 * Selection. best_k[b] = the smallest k among those with the smallest cost[b][k]; best_cost[b] = that cost.
 *   raht_motion_search : best_k (DEVICE int32[n_blocks]), best_cost (DEVICE uint64[n_blocks], may be NULL) and, when the caller
 *                        passes one, the whole table cost_table (DEVICE uint64[n_blocks * K]; NULL: scratch of the library's pool).
 *                        A memset of the table and two launches; enqueues only, never synchronises.
 *   raht_predict_mc    : raht_predict under the field mv (DEVICE int8[3 * n_blocks]): Y = X - P (add = 0), X + P (add = 1) or P
 *                        (X NULL); Y may be X; n_matched (DEVICE int64, may be NULL) = the rows with a non-empty run. One launch
 *                        (and a memset when n_matched is given); enqueues only, never synchronises.
 * RAHT_ERR_INVALID, with nothing enqueued: NULL required pointers, N or N_ref outside 1 .. 2^31 - 1, J outside 1 .. 21, block_log2
 * outside 1 .. J, n_blocks outside 1 .. N, shift not one of 0, 3, 6, 9, D < 1, a row stride below D, K outside 1 .. 512, add not
 * 0 or 1.
 *
 *   compensated frame : "RAHTM001" | int64 ref_back | int64 up | int64 block_log2 | int64 n_blocks | int8 mv[n_blocks][3] | zero
 *                       bytes up to a multiple of 8 | a whole "RAHTF001" frame container whose attributes are the residual
 *                       X - P_mv. Every int8 value is legal (a vector that leaves the cube predicts 0). n_blocks is the inner
 *                       geometry header's n_(J - block_log2). The rules of a predicted frame hold: only inside a sequence
 *                       container, never at index 0; the reconstruction is the inner frame's plus P_mv of the reference's.
 *
 * Hierarchical search (python: ops.motion_search_around / ops.motion_pyramid / ops.motion_search_hier,
 * bitstream.encode_sequence_bytes(..., motion_levels)): vectors beyond the reach of an exhaustive search, at a cost
 * that does not grow with the cube of the reach. Inputs: the frame's (k, X), a reference (k', C') of the same J and D,
 * block_log2 = m, weights w, up, a number of levels L with 0 <= L <= min(3, m - 1) and J - L >= 1, and a top radius r in 1 .. 3.
 * Pyramid. Level 0 of a frame (k, C) is the frame. Level l has as keys the distinct values of k >> 3 l, ascending, at depth J - l;
 * its row for a cell is the run mean of C over the cell's rows -- the sequential float32 sum in row order and one IEEE division,
 * the bits raht_predict(cell_keys << 3 l, k, C, X = NULL, shift = 3 l) returns. The frame's blocks are the same cells at every
 * level: at level l they have block_log2 = m - l and n_blocks is unchanged.
 * Search. v_L = raht_motion_search on level L of both frames with every vector of [-r, r]^3 (ordered by squared length, then
 * dx, dy, dz: index 0 is no motion), w and shift 0. For l = L - 1 .. 0: v_l = raht_motion_search_around on level l of both frames
 * with base = 2 v_(l+1), the 27 vectors of [-1, 1]^3 in that order, w, shift 0 above level 0 and the caller's 3 up at level 0.
 * The result is v_0; its reach is r 2^L + 2^L - 1 <= 31 per component. L = 0 is raht_motion_search.
 * Search around a base. base (DEVICE int8[3 * n_blocks]): the vector of the pair (block b, candidate k) is base[b] + cand[k],
 * formed in integers. The cost of the pair is the cost above under that vector: shifted key, resolve, run mean, fl order, cap,
 * 2^-10 fixed point, integer block sums. A pair with a component outside -127 .. 127 is INVALID: its table entry is 2^64 - 1
 * after the call and it is never selected. best_k[b] = the smallest k among the valid pairs of the smallest cost, best_cost[b]
 * that cost, mv[b] = base[b] + cand[best_k[b]]; a block with no valid pair gets best_k = -1, best_cost = 2^64 - 1 and mv = 0.
 * With base = 0 the table and the selection are raht_motion_search's; with a constant base v the table is raht_motion_search's
 * for the candidates v + cand[k].
 *   raht_motion_search_around : raht_motion_search's arguments, base, and mv (DEVICE int8[3 * n_blocks], written by the library).
 *                               A memset of the table and two launches; enqueues only, never synchronises.
 * RAHT_ERR_INVALID, with nothing enqueued: every rule of raht_motion_search, a NULL base, a NULL mv. */
int raht_motion_search(const uint64_t *keys_sorted, int64_t N, int J, int block_log2, const int64_t *block_first, int64_t n_blocks,
                       const uint64_t *ref_keys_sorted, int64_t N_ref, int shift, const float *C_ref, int64_t ld_ref, const float *X,
                       int64_t ldx, int D, const float *weights, const int32_t *cand, int K, int32_t *best_k, uint64_t *best_cost,
                       uint64_t *cost_table, raht_stream_t stream);
int raht_motion_search_around(const uint64_t *keys_sorted, int64_t N, int J, int block_log2, const int64_t *block_first, int64_t n_blocks,
                              const uint64_t *ref_keys_sorted, int64_t N_ref, int shift, const float *C_ref, int64_t ld_ref, const float *X,
                              int64_t ldx, int D, const float *weights, const int8_t *base, const int32_t *cand, int K, int32_t *best_k,
                              uint64_t *best_cost, int8_t *mv, uint64_t *cost_table, raht_stream_t stream);
int raht_predict_mc(const uint64_t *keys_sorted, int64_t N, int J, int block_log2, const int64_t *block_first, int64_t n_blocks,
                    const int8_t *mv, const uint64_t *ref_keys_sorted, int64_t N_ref, int shift, const float *C_ref, int64_t ld_ref,
                    const float *X, int64_t ldx, int D, int add, float *Y, int64_t ldy, int64_t *n_matched, raht_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Two references (csrc/predict_bi.hip): the predictor of a B frame, which lies between two coded frames and is a reference of
 * none (python: ops.predict_bi, bitstream.encode_sequence_bytes(..., bframes)).
 *
 * The frame's keys k[0 .. N), two references (k0', C0') and (k1', C1') of the same depth and D, shift = 3 up as above, and
 * optionally one motion field per reference, mv0 and mv1 (DEVICE int8[3 * n_blocks] over the FRAME's blocks: J, block_log2,
 * block_first, n_blocks as raht_predict_mc takes them; a NULL field is all zero, and with both NULL none of the four is read).
 * For reference r, m_r[i, ch] is exactly raht_predict's P (raht_predict_mc's under mv_r) against that reference -- the sequential
 * float32 sum over the run in row order, one IEEE division -- and len_r the run's length, 0 for an empty cell or a shifted voxel
 * outside the cube. Then
 *     P = m0                      where len1 == 0
 *     P = m1                      where len0 == 0        (+0.0f where both are 0)
 *     P = fl(0.5f * fl(m0 + m1))  where both have a run: the sum is rounded, then the product; neither is contracted with what
 *                                 follows (a sum that overflows, overflows)
 * and Y = fl(X - P) (add = 0), fl(X + P) (add = 1) or P (X NULL): one float32 operation per element, also where P = 0. A row
 * with a run in one reference only has raht_predict(_mc)'s bits for that reference; two identical references give raht_predict's
 * bits for finite |m| < FLT_MAX / 2.
 *   raht_predict_bi : Y may be X (a lane reads only what it writes); neither reference may overlap Y. n_matched (DEVICE int64[3],
 *                     may be NULL) = the rows with a run in reference 0, in reference 1, in both. One launch (and a memset when
 *                     n_matched is given); enqueues only, never synchronises.
 * RAHT_ERR_INVALID, with nothing enqueued: raht_predict's rules for either reference, and with a field raht_predict_mc's rules
 * for J, block_log2, block_first and n_blocks.
 *
 *   B frame : "RAHTB001" | int64 ref_back (>= 1) | int64 ref_fwd (>= 1) | int64 up | int64 block_log2 (0: no fields, else 1 .. J) |
 *             int64 n_blocks (0 iff block_log2 == 0) | with fields: int8 mv0[n_blocks][3], zero bytes up to a multiple of 8, int8
 *             mv1[n_blocks][3], padded likewise | a whole "RAHTF001" frame container whose attributes are the residual X - P.
 *             Frame i is predicted from the frames i - ref_back (reference 0) and i + ref_fwd (reference 1), neither of which is a
 *             B frame; only inside a sequence container, never at index 0, never reaching past the last frame. A predicted
 *             geometry section is coded against reference 0's keys. */
int raht_predict_bi(const uint64_t *keys_sorted, int64_t N, int J, int block_log2, const int64_t *block_first, int64_t n_blocks,
                    const int8_t *mv0, const int8_t *mv1, const uint64_t *ref0_keys_sorted, int64_t N_ref0, const float *C_ref0,
                    int64_t ld_ref0, const uint64_t *ref1_keys_sorted, int64_t N_ref1, const float *C_ref1, int64_t ld_ref1, int shift,
                    const float *X, int64_t ldx, int D, int add, float *Y, int64_t ldy, int64_t *n_matched, raht_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Block modes (csrc/mode_search.hip, csrc/predict_bi.hip): every occupied block of a B frame picks its own predictor (python:
 * ops.mode_search, ops.predict_bi(..., modes), bitstream.encode_sequence_bytes(..., block_modes)).
 *
 * The frame, its two references, shift and the optional fields mv0, mv1 are raht_predict_bi's; the blocks (J, block_log2,
 * block_first, n_blocks) are raht_motion_search's and are needed with or without fields. With m_r and len_r as above, the
 * prediction of a row under the mode of its block is
 *     mode 0 : raht_predict_bi's P -- the mean where both references have a run, the one that has where one has, +0 where none has
 *     mode 1 : m0 -- raht_predict's P (raht_predict_mc's under mv0) against reference 0, +0 where it has no run: reference 1 is
 *              not looked at
 *     mode 2 : m1, likewise against reference 1
 *     mode 3 : +0
 * Cost. The cost of a row under a mode is raht_motion_search's row cost against that mode's P: weights w[D] (DEVICE float32,
 * finite and >= 0: the caller's contract), c = 0.0f; for ch ascending with w[ch] != 0: t = fl(X[i, ch] - P[i, ch]); t = |t|;
 * t = fl(w[ch] t); c = fl(c + t); q = (uint64) floorf(fminf(c, 1048576.0f) * 1024.0f) -- NaN and +inf take the cap. cost[b][mode] =
 * the sum of q over the rows of block b: integers, independent of order and of how rows are cut into tiles. With every weight 0
 * the table is 0.
 * Selection. mode[b] = the smallest mode among those with the smallest cost[b][mode]; best_cost[b] = that cost. Two references
 * that predict the same choose mode 0 everywhere.
 *   raht_mode_search      : mode (DEVICE uint8[n_blocks]), best_cost (DEVICE uint64[n_blocks], may be NULL) and, when the caller
 *                           passes one, the whole table cost_table (DEVICE uint64[n_blocks * 4]; NULL: scratch of the library's
 *                           pool). One pass over the frame: a row resolves its key once per reference and walks the weighted
 *                           columns once for all four costs. A memset of the table and two launches; enqueues only, never
 *                           synchronises.
 *   raht_predict_bi_modes : raht_predict_bi under mode (DEVICE uint8[n_blocks]; a value above 3 predicts as 3): Y = X - P
 *                           (add = 0), X + P (add = 1) or P (X NULL), one float32 operation per element also where P = +0; Y may
 *                           be X. With every mode 0 the bits are raht_predict_bi's, with every mode 1 (2) raht_predict's or
 *                           raht_predict_mc's against reference 0 (1). n_matched (DEVICE int64[3], may be NULL) = the rows whose
 *                           prediction uses a run of reference 0, of reference 1, of both. One launch (and a memset when
 *                           n_matched is given); enqueues only, never synchronises.
 * RAHT_ERR_INVALID, with nothing enqueued: raht_predict's rules for either reference, raht_predict_mc's rules for J, block_log2,
 * block_first and n_blocks (fields or none), a NULL mode, and for the search a NULL X or NULL weights. Whatever block_first, the
 * fields and the modes hold, no store leaves a buffer.
 *
 *   B frame with modes : "RAHTB002" | int64 ref_back (>= 1) | int64 ref_fwd (>= 1) | int64 up | int64 block_log2 (1 .. J) | int64
 *             n_blocks (>= 1) | int64 flags (bit 0: two motion fields follow; every other bit 0) | with bit 0: int8
 *             mv0[n_blocks][3], zero bytes up to a multiple of 8, int8 mv1[n_blocks][3], padded likewise | uint8 mode[n_blocks]
 *             (0 .. 3), zero bytes up to a multiple of 8 | a whole "RAHTF001" frame container whose attributes are the residual
 *             X - P under the modes. n_blocks is the inner geometry header's n_(J - block_log2). Everything else is the B
 *             frame's; "RAHTB001" stays what a B frame whose modes are all 0 is written as. */
int raht_mode_search(const uint64_t *keys_sorted, int64_t N, int J, int block_log2, const int64_t *block_first, int64_t n_blocks,
                     const int8_t *mv0, const int8_t *mv1, const uint64_t *ref0_keys_sorted, int64_t N_ref0, const float *C_ref0,
                     int64_t ld_ref0, const uint64_t *ref1_keys_sorted, int64_t N_ref1, const float *C_ref1, int64_t ld_ref1, int shift,
                     const float *X, int64_t ldx, int D, const float *weights, uint8_t *mode, uint64_t *best_cost, uint64_t *cost_table,
                     raht_stream_t stream);
int raht_predict_bi_modes(const uint64_t *keys_sorted, int64_t N, int J, int block_log2, const int64_t *block_first, int64_t n_blocks,
                          const uint8_t *mode, const int8_t *mv0, const int8_t *mv1, const uint64_t *ref0_keys_sorted, int64_t N_ref0,
                          const float *C_ref0, int64_t ld_ref0, const uint64_t *ref1_keys_sorted, int64_t N_ref1, const float *C_ref1,
                          int64_t ld_ref1, int shift, const float *X, int64_t ldx, int D, int add, float *Y, int64_t ldy, int64_t *n_matched,
                          raht_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RAHT_H */
