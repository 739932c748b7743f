// predict_device.h -- the inter-frame predictor's device code, shared by predict.hip (the co-located predictor), motion.hip
// (the motion-compensated one and the motion search), predict_bi.hip (the two-reference one) and mode_search.hip (the per-block
// choice among a B frame's predictors): the resolve of a key to its run in the reference, the run mean, the predictor kernel, whose
// KEY functor says for which key a row is resolved, and the row cost and block sums of the searches (include/raht.h, "Inter-frame
// prediction", "Motion compensation", "Two references" and "Block modes").
// Row i of the current frame lies in the cell c = key[i] >> shift; its prediction is the mean of the reference rows of that cell,
// which are ONE run [lo, hi) of the reference's sorted keys: summed in float32 in row order from the run's first row, divided once
// by the run's length, 0 for an empty run. The order of the sum is part of the definition (a run holds at most 8^up <= 512 rows),
// so every implementation gives the same bits, and with shift = 0 the prediction is the co-located voxel's row exactly.
//
//   one launch, PR_TILE_ROWS rows per workgroup step:
//     resolve   one thread per row finds lo by binary search in the reference keys (an L2-resident table: 8 N' bytes) and hi by
//               another inside the 8^up rows behind lo; (lo, hi - lo) go to LDS, the rows with a run are counted.
//     move      the tile's elements flat. Matrices without padding (every row stride == D) move in 16-byte chunks that may
//               straddle rows (59 columns: 236-byte rows), X and Y nontemporal (touched once), the reference rows through the
//               cache (neighbouring voxels of a cell re-read them when shift > 0), two chunks per lane and round with their X
//               loads issued first; padded matrices move element by element.
//   Every row recomputes the mean of its run: no table of cell means is built (DESIGN.md 18 has the numbers).
#pragma once
#include "raht_common.h"
#include "raht_device.h"

namespace raht {

constexpr int PR_THREADS = 256;
constexpr int PR_MAX_GRID = 2048;                        // grids are capped and grid-strided
constexpr int PR_TILE_ROWS = PR_THREADS;                 // rows a workgroup resolves per step: one thread per row

// first r in [a, b) with (ref[r] >> shift) >= c (UPPER: > c); b when there is none
template <bool UPPER>
__device__ __forceinline__ int32_t pr_bound(const uint64_t *__restrict__ ref, int32_t a, int32_t b, int shift, uint64_t c)
{
    while (a < b) {
        const int32_t m = a + ((b - a) >> 1);
        const uint64_t v = ref[m] >> shift;
        if (UPPER ? v <= c : v < c) a = m + 1; else b = m;
    }
    return a;
}

// the run of the cell c = key >> shift in the reference -> lo, the return value its length (0: the cell is empty)
__device__ __forceinline__ int32_t pr_resolve(const uint64_t *__restrict__ ref_keys, int32_t n_ref, int shift, uint64_t key, int32_t &lo)
{
    const uint64_t c = key >> shift;
    lo = pr_bound<false>(ref_keys, 0, n_ref, shift, c);
    // strictly ascending keys: a cell holds at most 8^up = 2^shift rows, so the run ends inside that window
    return pr_bound<true>(ref_keys, lo, (int32_t)min((int64_t)n_ref, (int64_t)lo + ((int64_t)1 << shift)), shift, c) - lo;
}

// The key a row is resolved for. SameKey: its own (raht_predict).
struct SameKey {
    __device__ __forceinline__ bool operator()(int64_t, uint64_t key, uint64_t &out) const { out = key; return true; }
};

// the key of the voxel (x + dx, y + dy, z + dz) of a frame of depth J (digit = z + 2 y + 4 x, as raht_morton writes it); false when
// the voxel lies outside the cube [0, 2^J)^3: the row has no match
__device__ __forceinline__ bool pr_shift_key(const VoxCoords &v, int64_t dx, int64_t dy, int64_t dz, int J, uint64_t &out)
{
    const int64_t x = (int64_t)v.x + dx, y = (int64_t)v.y + dy, z = (int64_t)v.z + dz, n = (int64_t)1 << J;
    if (x < 0 || y < 0 || z < 0 || x >= n || y >= n || z >= n) return false;
    out = vx_spread3((uint64_t)z) | (vx_spread3((uint64_t)y) << 1) | (vx_spread3((uint64_t)x) << 2);
    return true;
}

// the block of a row: the last b with block_first[b] <= row (block_first[0] = 0, ascending, n_blocks entries are read)
__device__ __forceinline__ int64_t pr_block_of(const int64_t *__restrict__ block_first, int64_t n_blocks, int64_t row)
{
    int64_t a = 0, b = n_blocks;                         // first entry > row, in [1, n_blocks]
    while (a < b) {
        const int64_t m = a + ((b - a) >> 1);
        if (block_first[m] <= row) a = m + 1; else b = m;
    }
    return a > 0 ? a - 1 : 0;
}

// MvKey: the key shifted by the motion vector of the row's block (raht_predict_mc)
struct MvKey {
    const int64_t *block_first;
    int64_t n_blocks;
    const int8_t *mv;
    int J;
    __device__ __forceinline__ bool operator()(int64_t row, uint64_t key, uint64_t &out) const
    {
        const int8_t *v = mv + 3 * pr_block_of(block_first, n_blocks, row);
        return pr_shift_key(vox_coords(key), v[0], v[1], v[2], J, out);
    }
};

// prediction of channel ch of a row whose run is [lo, lo + len): the sequential float32 sum, one IEEE division
__device__ __forceinline__ float pr_mean(const float *__restrict__ C_ref, int64_t ld_ref, int32_t lo, int32_t len, int ch)
{
    if (len == 0) return 0.0f;
    const float *p = C_ref + (int64_t)lo * ld_ref + ch;
    float s = p[0];
    for (int32_t r = 1; r < len; ++r) s = s + p[(int64_t)r * ld_ref];
    return len > 1 ? __fdiv_rn(s, (float)len) : s;       // (s / 1.0f is s)
}

// MODE 0: Y = P, 1: Y = X - P, 2: Y = X + P
template <int MODE> __device__ __forceinline__ float pr_apply(float x, float p) { return MODE == 0 ? p : (MODE == 1 ? x - p : x + p); }

// the 16-byte chunk of a flat tile that starts at element e: four predictions applied to x
template <int MODE>
__device__ __forceinline__ RegChunk<float> pr_chunk(const float *__restrict__ C_ref, int64_t ld_ref, const int32_t *run_lo, const int32_t *run_len,
                                                    uint32_t e, uint32_t D, const RegChunk<float> &x)
{
    uint32_t j = e / D, ch = e - j * D;
    RegChunk<float> y;
    if (ch + 4 <= D) {                                   // the chunk lies in one row: its run in 16-byte loads
        const int32_t len = run_len[j];
        RegChunk<float> s;
#pragma unroll
        for (int i = 0; i < 4; ++i) s.v[i] = 0.0f;
        if (len > 0) {
            const float *p = C_ref + (int64_t)run_lo[j] * ld_ref + ch;
            s = ld_chunk<float>(p);
            for (int32_t r = 1; r < len; ++r) {
                const RegChunk<float> a = ld_chunk<float>(p + (int64_t)r * ld_ref);
#pragma unroll
                for (int i = 0; i < 4; ++i) s.v[i] = s.v[i] + a.v[i];
            }
            if (len > 1) {
                const float d = (float)len;
#pragma unroll
                for (int i = 0; i < 4; ++i) s.v[i] = __fdiv_rn(s.v[i], d);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) y.v[i] = pr_apply<MODE>(x.v[i], s.v[i]);
    } else {                                             // the chunk straddles rows (as many as four when D = 1)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            y.v[i] = pr_apply<MODE>(x.v[i], pr_mean(C_ref, ld_ref, run_lo[j], run_len[j], (int)ch));
            if (++ch == D) { ch = 0; ++j; }
        }
    }
    return y;
}

// pr_chunk's mean without the apply, for the two-reference predictor (predict_bi.hip): the means of channels ch .. ch + 3 of ONE
// row whose run is [lo, lo + len), the bits of pr_mean per channel; +0 for an empty run
__device__ __forceinline__ RegChunk<float> pr_chunk_mean(const float *__restrict__ C_ref, int64_t ld_ref, int32_t lo, int32_t len, uint32_t ch)
{
    RegChunk<float> s;
#pragma unroll
    for (int i = 0; i < 4; ++i) s.v[i] = 0.0f;
    if (len > 0) {
        const float *p = C_ref + (int64_t)lo * ld_ref + ch;
        s = ld_chunk<float>(p);
        for (int32_t r = 1; r < len; ++r) {
            const RegChunk<float> a = ld_chunk<float>(p + (int64_t)r * ld_ref);
#pragma unroll
            for (int i = 0; i < 4; ++i) s.v[i] = s.v[i] + a.v[i];
        }
        if (len > 1) {
            const float d = (float)len;
#pragma unroll
            for (int i = 0; i < 4; ++i) s.v[i] = __fdiv_rn(s.v[i], d);
        }
    }
    return s;
}

// the two-reference prediction from the two means (each +0 for an empty run): the one that has a run, or fl(0.5 fl(m0 + m1)) --
// the sum rounded, then the product, neither contracted with what is done with the result
__device__ __forceinline__ float pr_bi(float m0, int32_t len0, float m1, int32_t len1)
{
    if (len1 == 0) return m0;
    if (len0 == 0) return m1;
    return __fmul_rn(0.5f, __fadd_rn(m0, m1));
}

// a reference of the two-reference kernels (predict_bi.hip, mode_search.hip): its sorted keys and its reconstruction
struct PrRef {
    const uint64_t *keys;
    int32_t n;
    const float *C;
    int64_t ld;
};

// ---- what the search kernels share (motion.hip: the motion search, mode_search.hip: the mode search) ----------------------------
constexpr int MS_THREADS = 256;                          // the largest tile: one thread per row
constexpr int MS_MAX_GRID = 2048;                        // grids are capped and grid-strided
constexpr size_t MS_LDS_BYTES = 65536 - 64;              // dynamic LDS a workgroup may ask for (the kernels' statics: 16 bytes)
constexpr float MS_COST_CAP = 1048576.0f;                // 2^20 per row; q = floor(min(c, cap) * 2^10) <= 2^30

// the fixed-point cost of a row from its float32 cost: NaN and +inf take the cap (fminf(NaN, x) = x), the product is exact
__device__ __forceinline__ unsigned long long ms_fixed(float c)
{
    const float m = fminf(c, MS_COST_CAP);
    return m > 0.0f ? (unsigned long long)floorf(m * 1024.0f) : 0ull;
}

// dynamic LDS of a tile: acc[2][tile] uint64 | wcol[D] int32 | wval[D] float | xs[tile * x_stride] float (STAGED only)
static inline size_t ms_lds_bytes(int tile, int D, int x_stride) { return (size_t)tile * 16 + (size_t)D * 8 + (size_t)tile * x_stride * 4; }

// the rows of a staged tile for rows of D floats (row stride D | 1 in LDS): the largest of 256 / 192 / 128 / 64 whose rows fit the
// LDS budget; 0: none fits, X is read through the cache (raht_debug_motion_tile)
static inline int ms_tile_rows(int D)
{
    if (D < 1 || D > 4096) return 0;
    for (int t = MS_THREADS; t >= 64; t -= 64)
        if (ms_lds_bytes(t, D, D | 1) <= MS_LDS_BYTES) return t;
    return 0;
}

// One column of a cost table, summed per block over a tile whose rows are lanes: q is this row's cost, slot the tile row at which
// its block begins (blocks are runs of lanes), tail / head: the last lane of its block in this wave / the block's first row of the
// tile. A segmented scan inside the wave, the wave's segment tails add into the LDS slot of their block (acc: one zeroed uint64
// per tile row), and after the barrier the head adds the slot to *cell -- ONE 64-bit atomic per (block, column, workgroup) -- and
// zeroes it. Every thread of the workgroup calls this; consecutive columns alternate between two sets of slots, so a column
// costs one barrier.
__device__ __forceinline__ void ms_block_add(unsigned long long q, int slot, int lane, int tid, bool tail, bool head, unsigned long long *acc,
                                             unsigned long long *cell)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long u = __shfl_up(q, d);
        const int s = __shfl_up(slot, d);
        if (lane >= d && s == slot) q += u;
    }
    if (tail && q) atomicAdd(acc + slot, q);
    __syncthreads();
    if (head) {
        const unsigned long long v = acc[tid];
        if (v) {
            atomicAdd(cell, v);
            acc[tid] = 0;                                // (this set is added to again two columns on: a barrier lies between)
        }
    }
}

// FLAT: every row stride == D, the tile is one run of rows * D floats (X, Y element-aligned only). X and Y may be the same matrix:
// a thread reads what it writes and nothing else of them.
template <int MODE, bool FLAT, typename KEY>
__global__ __launch_bounds__(PR_THREADS) void predict_kernel(const uint64_t *__restrict__ keys, int64_t n, const uint64_t *__restrict__ ref_keys,
                                                             int32_t n_ref, int shift, const float *__restrict__ C_ref, int64_t ld_ref,
                                                             const float *X, int64_t ldx, int D, float *Y, int64_t ldy,
                                                             unsigned long long *__restrict__ n_matched, const KEY key_of)
{
    __shared__ int32_t run_lo[PR_TILE_ROWS], run_len[PR_TILE_ROWS];
    __shared__ uint32_t hits;
    if (threadIdx.x == 0) hits = 0;
    uint32_t mine = 0;
    const int64_t n_tiles = (n + PR_TILE_ROWS - 1) / PR_TILE_ROWS;
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int64_t r0 = t * PR_TILE_ROWS;
        const int rows = (int)min((int64_t)PR_TILE_ROWS, n - r0);
        __syncthreads();                                 // the previous step's readers are done with the runs
        if ((int)threadIdx.x < rows) {
            uint64_t key;
            int32_t lo = 0, len = 0;
            if (key_of(r0 + threadIdx.x, keys[r0 + threadIdx.x], key)) len = pr_resolve(ref_keys, n_ref, shift, key, lo);
            run_lo[threadIdx.x] = lo;
            run_len[threadIdx.x] = len;
            mine += len > 0;
        }
        __syncthreads();
        const uint32_t n_el = (uint32_t)rows * (uint32_t)D;
        if constexpr (FLAT) {
            const float *xt = MODE ? X + r0 * D : nullptr;
            float *yt = Y + r0 * D;
            const uint32_t n_chunks = n_el >> 2;
            // two chunks per round, their loads of X first: 32 bytes of X and two reference chunks per lane in flight
            for (uint32_t q = threadIdx.x; q < n_chunks; q += 2 * PR_THREADS) {
                const uint32_t e0 = q << 2, e1 = (q + PR_THREADS) << 2;
                const bool two = q + PR_THREADS < n_chunks;
                RegChunk<float> x0 = {}, x1 = {};
                if constexpr (MODE != 0) {
                    x0 = ld_chunk<float, true>(xt + e0);
                    if (two) x1 = ld_chunk<float, true>(xt + e1);
                }
                const RegChunk<float> y0 = pr_chunk<MODE>(C_ref, ld_ref, run_lo, run_len, e0, (uint32_t)D, x0);
                if (two) {
                    const RegChunk<float> y1 = pr_chunk<MODE>(C_ref, ld_ref, run_lo, run_len, e1, (uint32_t)D, x1);
                    st_chunk<float, true>(yt + e0, y0);
                    st_chunk<float, true>(yt + e1, y1);
                } else {
                    st_chunk<float, true>(yt + e0, y0);
                }
            }
            // the last elements of the frame's last tile (rows * D no multiple of 4)
            const uint32_t e = (n_chunks << 2) + threadIdx.x;
            if (e < n_el) {
                const uint32_t j = e / (uint32_t)D, ch = e - j * (uint32_t)D;
                yt[e] = pr_apply<MODE>(MODE ? xt[e] : 0.0f, pr_mean(C_ref, ld_ref, run_lo[j], run_len[j], (int)ch));
            }
        } else {
            for (int64_t e = threadIdx.x; e < (int64_t)rows * D; e += PR_THREADS) {      // (also the home of D >= 2^22: 64-bit indices)
                const int64_t j = e / D, ch = e - j * D;
                const float x = MODE ? X[(r0 + j) * ldx + ch] : 0.0f;
                Y[(r0 + j) * ldy + ch] = pr_apply<MODE>(x, pr_mean(C_ref, ld_ref, run_lo[j], run_len[j], (int)ch));
            }
        }
    }
    if (n_matched) {                                     // an integer sum: whatever the order, the same number
        if (mine) atomicAdd(&hits, mine);
        __syncthreads();
        if (threadIdx.x == 0 && hits) atomicAdd(n_matched, (unsigned long long)hits);
    }
}

template <int MODE, typename KEY>
static void predict_launch(bool flat, unsigned grid, hipStream_t s, const uint64_t *keys, int64_t N, const uint64_t *ref_keys, int64_t N_ref,
                           int shift, const float *C_ref, int64_t ld_ref, const float *X, int64_t ldx, int D, float *Y, int64_t ldy,
                           int64_t *n_matched, const KEY &key_of)
{
    if (flat)
        hipLaunchKernelGGL((predict_kernel<MODE, true, KEY>), dim3(grid), dim3(PR_THREADS), 0, s, keys, N, ref_keys, (int32_t)N_ref, shift,
                           C_ref, ld_ref, X, ldx, D, Y, ldy, (unsigned long long *)n_matched, key_of);
    else
        hipLaunchKernelGGL((predict_kernel<MODE, false, KEY>), dim3(grid), dim3(PR_THREADS), 0, s, keys, N, ref_keys, (int32_t)N_ref, shift,
                           C_ref, ld_ref, X, ldx, D, Y, ldy, (unsigned long long *)n_matched, key_of);
}

// the argument rules the predictors share (`who`: the entry point's name) ...
static inline int predict_check(const char *who, const void *keys, int64_t N, const void *ref_keys, int64_t N_ref, int shift, const void *C_ref,
                                int64_t ld_ref, const void *X, int64_t ldx, int D, int add, const void *Y, int64_t ldy)
{
    if (!keys || !ref_keys || !C_ref || !Y) { set_error("%s: NULL keys, reference or output", who); return RAHT_ERR_INVALID; }
    if (N < 1 || N >= ((int64_t)1 << 31) || N_ref < 1 || N_ref >= ((int64_t)1 << 31)) {
        set_error("%s: N and N_ref must be 1 .. 2^31 - 1", who);
        return RAHT_ERR_INVALID;
    }
    if (shift != 0 && shift != 3 && shift != 6 && shift != 9) { set_error("%s: shift=%d (0, 3, 6 or 9)", who, shift); return RAHT_ERR_INVALID; }
    if (D < 1 || ld_ref < D || ldy < D || (X && ldx < D)) { set_error("%s: D must be >= 1 and no row stride below it", who); return RAHT_ERR_INVALID; }
    if (add != 0 && add != 1) { set_error("%s: add=%d (0 or 1)", who, add); return RAHT_ERR_INVALID; }
    return RAHT_OK;
}

// the rules of a frame's blocks, shared by every entry point that takes a motion field
static inline int motion_check_blocks(const char *who, int J, int block_log2, const void *block_first, int64_t n_blocks, int64_t N)
{
    if (!block_first) { set_error("%s: NULL block_first", who); return RAHT_ERR_INVALID; }
    if (J < 1 || J > 21) { set_error("%s: J=%d outside 1 .. 21", who, J); return RAHT_ERR_INVALID; }
    if (block_log2 < 1 || block_log2 > J) { set_error("%s: block_log2=%d outside 1 .. J", who, block_log2); return RAHT_ERR_INVALID; }
    if (n_blocks < 1 || n_blocks > N) { set_error("%s: n_blocks must be 1 .. N", who); return RAHT_ERR_INVALID; }
    return RAHT_OK;
}

// ... and their one launch (and a memset when n_matched is given), for checked arguments
template <typename KEY>
static int predict_enqueue(const uint64_t *keys_sorted, int64_t N, const uint64_t *ref_keys_sorted, int64_t N_ref, int shift, const float *C_ref,
                           int64_t ld_ref, const float *X, int64_t ldx, int D, int add, float *Y, int64_t ldy, int64_t *n_matched,
                           const KEY &key_of, hipStream_t s)
{
    if (n_matched) RAHT_HIP_CHECK(hipMemsetAsync(n_matched, 0, sizeof(int64_t), s));
    const int64_t tiles = ceil_div(N, PR_TILE_ROWS);
    const unsigned grid = (unsigned)(tiles > PR_MAX_GRID ? PR_MAX_GRID : tiles);
    const bool flat = ldy == D && (!X || ldx == D) && D < (1 << 22);      // (flat tiles index their elements with 32 bits)
    if (!X) predict_launch<0>(flat, grid, s, keys_sorted, N, ref_keys_sorted, N_ref, shift, C_ref, ld_ref, X, ldx, D, Y, ldy, n_matched, key_of);
    else if (!add) predict_launch<1>(flat, grid, s, keys_sorted, N, ref_keys_sorted, N_ref, shift, C_ref, ld_ref, X, ldx, D, Y, ldy, n_matched, key_of);
    else predict_launch<2>(flat, grid, s, keys_sorted, N, ref_keys_sorted, N_ref, shift, C_ref, ld_ref, X, ldx, D, Y, ldy, n_matched, key_of);
    RAHT_HIP_CHECK(hipGetLastError());
    return RAHT_OK;
}

}  // namespace raht
