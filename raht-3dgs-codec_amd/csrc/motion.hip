// motion.hip -- block motion search and the motion-compensated predictor of a sequence (include/raht.h, "Motion compensation";
// DESIGN.md 19). A block is a cell of the octree level block_log2 above the voxels; its rows are one run of the sorted keys
// (block_first: raht_region_cells). A candidate vector v moves every voxel of the block to the voxel x + v of the reference; the
// prediction of the row is raht_predict's for THAT key (predict_device.h: the same resolve, the same run mean, the same bits).
//
//   raht_motion_search   memset of the cost table, then
//     search   MS tile rows per workgroup step, one thread per row. The weighted columns of the tile's X rows are staged in LDS
//              once (row stride odd: a lane per row reads conflict-free), then every candidate is walked against them: shift the
//              key, resolve it in the reference keys (L2-resident, as in the predictor), form the run mean column by column,
//              accumulate c in the order of the definition (product rounded before the sum: __fmul_rn / __fadd_rn), q = the
//              fixed-point cost. Rows of a block are contiguous, so q is summed per block by a segmented scan inside the wave,
//              the wave's segment tails add into an LDS slot per block of the tile, and the block's first row of the tile issues
//              ONE 64-bit atomic per (block, candidate, workgroup) into the table. Two sets of slots alternate, so a candidate
//              costs one barrier. Integer sums: the table does not depend on the order or on how a block is cut into tiles.
//              Matrices too wide for the LDS budget (D > 243) read X through the cache instead.
//     select   one thread per block: the smallest cost, the smallest k among equals.
//   raht_motion_search_around   the same two launches: the vector of the pair (block b, candidate k) is base[b] + cand[k].
//     search   the AROUND instantiations: a row reads its block's three base bytes once per tile and shifts its key by the sum; a
//              pair with a component outside +-127 is skipped (its rows add nothing).
//     select   tests the same rule from base and cand, writes 2^64 - 1 into the table for such a pair, never selects it, and
//              writes the chosen vector mv = base[b] + cand[best_k] (no valid pair: best_k = -1, cost 2^64 - 1, mv = 0).
//   raht_predict_mc      predict_device.h's kernel with MvKey: the key is shifted by the block's vector before the resolve.
#include <optional>

#include "predict_device.h"

namespace raht {

constexpr int MS_MAX_K = 512;                            // (the tile, the LDS budget, the row cost and the block sums: predict_device.h)

// a component of a vector base + cand that the int8 field can hold (-128 is not a vector: the rule is symmetric)
__device__ __forceinline__ bool ms_in_range(int64_t v) { return v >= -127 && v <= 127; }

// STAGED: blockDim.x rows per tile, their weighted columns in LDS. Otherwise X and the weights are read through the cache.
// AROUND: the vector of (block, candidate) is base[block] + cand (raht_motion_search_around); otherwise base is not read.
template <bool STAGED, bool AROUND>
__global__ __launch_bounds__(MS_THREADS) void motion_search_kernel(const uint64_t *__restrict__ keys, int64_t n, int J,
                                                                  const int64_t *__restrict__ block_first, int64_t n_blocks,
                                                                  const uint64_t *__restrict__ ref_keys, int32_t n_ref, int shift,
                                                                  const float *__restrict__ C_ref, int64_t ld_ref,
                                                                  const float *__restrict__ X, int64_t ldx, int D,
                                                                  const float *__restrict__ weights, const int32_t *__restrict__ cand, int K,
                                                                  unsigned long long *__restrict__ table, int x_stride,
                                                                  const int8_t *__restrict__ base)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ms_lds[];
    __shared__ int n_weighted;
    const int tile = (int)blockDim.x, tid = (int)threadIdx.x, lane = tid & 63;
    unsigned long long *acc = (unsigned long long *)ms_lds;                      // [2][tile]
    int32_t *wcol = (int32_t *)(acc + 2 * tile);                                 // [D] (STAGED)
    float *wval = (float *)(wcol + (STAGED ? D : 0));                            // [D] (STAGED)
    float *xs = wval + (STAGED ? D : 0);                                         // [tile][x_stride] (STAGED)

    acc[tid] = 0;
    acc[tile + tid] = 0;
    if (tid == 0) {                                      // the weighted columns, ascending (D <= 243 when STAGED)
        int nw = 0;
        for (int ch = 0; ch < D; ++ch) {
            const float w = weights[ch];
            if (w != 0.0f) {
                if (STAGED) { wcol[nw] = ch; wval[nw] = w; }
                ++nw;
            }
        }
        n_weighted = nw;
    }
    __syncthreads();
    const int nw = n_weighted;
    if (nw == 0) return;                                 // every cost is 0: the table stays as the memset left it

    const int64_t n_tiles = (n + tile - 1) / tile;
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int64_t r0 = t * tile;
        const int rows = (int)min((int64_t)tile, n - r0);
        const bool active = tid < rows;
        __syncthreads();                                 // the previous step's readers are done with xs, its flushes with acc
        if constexpr (STAGED) {
            for (int e = tid; e < rows * nw; e += tile) {
                const int r = e / nw, j = e - r * nw;
                xs[r * x_stride + j] = X[(r0 + r) * ldx + wcol[j]];
            }
        }
        // this row: its voxel, its block, the slot of its block in the tile (the block's first row of the tile)
        VoxCoords vox = {0, 0, 0};
        int64_t b = 0;
        int slot = -1;
        [[maybe_unused]] int bx = 0, by = 0, bz = 0;     // (AROUND) the base of this row's block
        if (active) {
            vox = vox_coords(keys[r0 + tid]);
            b = pr_block_of(block_first, n_blocks, r0 + tid);
            if constexpr (AROUND) {
                bx = base[3 * b];
                by = base[3 * b + 1];
                bz = base[3 * b + 2];
            }
            const int64_t first = block_first[b] - r0;   // (bounded for any block_first: 0 <= slot <= tid)
            slot = (int)(first < 0 ? 0 : (first > tid ? tid : first));
        }
        const int slot_next = __shfl_down(slot, 1);
        const bool tail = active && (lane == 63 || slot_next != slot);           // the last lane of its block in this wave
        const bool head = active && slot == tid;                                 // the block's first row of the tile flushes
        __syncthreads();                                 // xs is staged
        for (int k = 0; k < K; ++k) {
            unsigned long long q = 0;
            if (active) {
                uint64_t key;
                int32_t lo = 0, len = 0;
                [[maybe_unused]] bool valid = true;      // (AROUND) the rows of an invalid pair add nothing: select writes its entry
                if constexpr (AROUND) {
                    const int64_t dx = (int64_t)bx + cand[3 * k], dy = (int64_t)by + cand[3 * k + 1], dz = (int64_t)bz + cand[3 * k + 2];     // (any int32 candidate)
                    valid = ms_in_range(dx) && ms_in_range(dy) && ms_in_range(dz);
                    if (valid && pr_shift_key(vox, dx, dy, dz, J, key)) len = pr_resolve(ref_keys, n_ref, shift, key, lo);
                } else {
                    if (pr_shift_key(vox, cand[3 * k], cand[3 * k + 1], cand[3 * k + 2], J, key)) len = pr_resolve(ref_keys, n_ref, shift, key, lo);
                }
                if (valid) {
                    float c = 0.0f;
                    if constexpr (STAGED) {
                        const float *x = xs + tid * x_stride;
                        for (int j = 0; j < nw; ++j) {
                            const float d = fabsf(__fsub_rn(x[j], pr_mean(C_ref, ld_ref, lo, len, wcol[j])));
                            c = __fadd_rn(c, __fmul_rn(wval[j], d));
                        }
                    } else {
                        const float *x = X + (r0 + tid) * ldx;
                        for (int ch = 0; ch < D; ++ch) {
                            const float w = weights[ch];
                            if (w == 0.0f) continue;
                            const float d = fabsf(__fsub_rn(x[ch], pr_mean(C_ref, ld_ref, lo, len, ch)));
                            c = __fadd_rn(c, __fmul_rn(w, d));
                        }
                    }
                    q = ms_fixed(c);
                }
            }
            ms_block_add(q, slot, lane, tid, tail, head, acc + (k & 1) * tile, table + b * K + k);
        }
    }
}

__global__ __launch_bounds__(MS_THREADS) void motion_select_kernel(const unsigned long long *__restrict__ table, int64_t n_blocks, int K,
                                                                  int32_t *__restrict__ best_k, unsigned long long *__restrict__ best_cost)
{
    for (int64_t b = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x; b < n_blocks; b += (int64_t)gridDim.x * MS_THREADS) {
        const unsigned long long *row = table + b * K;
        unsigned long long best = row[0];
        int32_t at = 0;
        for (int k = 1; k < K; ++k) {
            const unsigned long long v = row[k];
            if (v < best) { best = v; at = k; }          // strictly smaller: the smallest k among equals stays
        }
        best_k[b] = at;
        if (best_cost) best_cost[b] = best;
    }
}

// raht_motion_search_around's selection: a pair (b, k) with a component of base[b] + cand[k] outside +-127 is invalid -- its table
// entry becomes 2^64 - 1 (no cost reaches it: fewer than 2^31 rows of at most 2^30) and it is never chosen
__global__ __launch_bounds__(MS_THREADS) void motion_select_around_kernel(unsigned long long *__restrict__ table, int64_t n_blocks, int K,
                                                                         const int8_t *__restrict__ base, const int32_t *__restrict__ cand,
                                                                         int32_t *__restrict__ best_k, unsigned long long *__restrict__ best_cost,
                                                                         int8_t *__restrict__ mv)
{
    for (int64_t b = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x; b < n_blocks; b += (int64_t)gridDim.x * MS_THREADS) {
        unsigned long long *row = table + b * K;
        const int bx = base[3 * b], by = base[3 * b + 1], bz = base[3 * b + 2];
        unsigned long long best = ~0ull;
        int32_t at = -1;
        int vx = 0, vy = 0, vz = 0;
        for (int k = 0; k < K; ++k) {
            const int64_t dx = (int64_t)bx + cand[3 * k], dy = (int64_t)by + cand[3 * k + 1], dz = (int64_t)bz + cand[3 * k + 2];     // (any int32 candidate)
            if (!(ms_in_range(dx) && ms_in_range(dy) && ms_in_range(dz))) { row[k] = ~0ull; continue; }
            const unsigned long long v = row[k];
            if (at < 0 || v < best) { best = v; at = k; vx = (int)dx; vy = (int)dy; vz = (int)dz; }     // strictly smaller: the smallest k among equals stays
        }
        best_k[b] = at;
        if (best_cost) best_cost[b] = best;
        mv[3 * b] = (int8_t)vx;
        mv[3 * b + 1] = (int8_t)vy;
        mv[3 * b + 2] = (int8_t)vz;
    }
}

// both search entry points, checked: the memset of the table and the two launches. base and mv: raht_motion_search_around's (both
// given), or both NULL.
static int motion_search_enqueue(const char *who, const uint64_t *keys_sorted, int64_t N, int J, const int64_t *block_first, int64_t n_blocks,
                                 const uint64_t *ref_keys_sorted, int64_t N_ref, int shift, const float *C_ref, int64_t ld_ref, const float *X,
                                 int64_t ldx, int D, const float *weights, const int32_t *cand, int K, const int8_t *base, int32_t *best_k,
                                 uint64_t *best_cost, int8_t *mv, uint64_t *cost_table, hipStream_t s)
{
    return guarded(who, [&]() -> int {
        const size_t table_bytes = sizeof(uint64_t) * (size_t)n_blocks * (size_t)K;
        std::optional<Scratch> ws;                       // (the caller's table, or one from the pool)
        if (!cost_table) {
            ws.emplace(table_bytes, s);
            if (!ws->ok()) { set_error("%s: out of device memory", who); return RAHT_ERR_NOMEM; }
        }
        unsigned long long *table = cost_table ? (unsigned long long *)cost_table : ws->as<unsigned long long>();
        RAHT_HIP_CHECK(hipMemsetAsync(table, 0, table_bytes, s));
        // the largest tile whose rows fit the LDS budget; none: X through the cache
        const int staged_rows = ms_tile_rows(D);
        const bool staged = staged_rows != 0;
        const int x_stride = staged ? (D | 1) : 0;
        const int tile = staged ? staged_rows : MS_THREADS;
        const int64_t tiles = ceil_div(N, tile);
        const dim3 grid((unsigned)(tiles > MS_MAX_GRID ? MS_MAX_GRID : tiles)), wg(tile);
        const size_t lds = staged ? ms_lds_bytes(tile, D, x_stride) : ms_lds_bytes(tile, 0, 0);
        auto *kernel = staged ? (base ? motion_search_kernel<true, true> : motion_search_kernel<true, false>)
                              : (base ? motion_search_kernel<false, true> : motion_search_kernel<false, false>);
        hipLaunchKernelGGL(kernel, grid, wg, lds, s, keys_sorted, N, J, block_first, n_blocks, ref_keys_sorted, (int32_t)N_ref, shift, C_ref,
                           ld_ref, X, ldx, D, weights, cand, K, table, x_stride, base);
        RAHT_HIP_CHECK(hipGetLastError());
        const int64_t sel = ceil_div(n_blocks, MS_THREADS);
        const dim3 sel_grid((unsigned)(sel > MS_MAX_GRID ? MS_MAX_GRID : sel));
        if (base)
            hipLaunchKernelGGL(motion_select_around_kernel, sel_grid, dim3(MS_THREADS), 0, s, table, n_blocks, K, base, cand, best_k,
                               (unsigned long long *)best_cost, mv);
        else
            hipLaunchKernelGGL(motion_select_kernel, sel_grid, dim3(MS_THREADS), 0, s, table, n_blocks, K, best_k,
                               (unsigned long long *)best_cost);
        RAHT_HIP_CHECK(hipGetLastError());
        return RAHT_OK;
    });
}

// the argument rules of both search entry points
static int motion_search_check(const char *who, const uint64_t *keys_sorted, int64_t N, int J, int block_log2, const int64_t *block_first,
                               int64_t n_blocks, const uint64_t *ref_keys_sorted, int64_t N_ref, int shift, const float *C_ref, int64_t ld_ref,
                               const float *X, int64_t ldx, int D, const float *weights, const int32_t *cand, int K, const int32_t *best_k)
{
    if (!X || !weights || !cand || !best_k) { set_error("%s: NULL X, weights, candidates or best_k", who); return RAHT_ERR_INVALID; }
    // (the predictor's rules: X stands in for the output, whose stride is then X's)
    RAHT_RET(predict_check(who, keys_sorted, N, ref_keys_sorted, N_ref, shift, C_ref, ld_ref, X, ldx, D, 0, X, ldx));
    RAHT_RET(motion_check_blocks(who, J, block_log2, block_first, n_blocks, N));
    if (K < 1 || K > MS_MAX_K) { set_error("%s: K=%d outside 1 .. %d", who, K, MS_MAX_K); return RAHT_ERR_INVALID; }
    return RAHT_OK;
}

}  // namespace raht

using namespace raht;

extern "C" {

int raht_debug_motion_tile(int D) { return ms_tile_rows(D); }

int raht_motion_search(const uint64_t *keys_sorted, int64_t N, int J, int block_log2, const int64_t *block_first, int64_t n_blocks,
                       const uint64_t *ref_keys_sorted, int64_t N_ref, int shift, const float *C_ref, int64_t ld_ref, const float *X,
                       int64_t ldx, int D, const float *weights, const int32_t *cand, int K, int32_t *best_k, uint64_t *best_cost,
                       uint64_t *cost_table, raht_stream_t stream)
{
    const char *who = "raht_motion_search";
    RAHT_RET(motion_search_check(who, keys_sorted, N, J, block_log2, block_first, n_blocks, ref_keys_sorted, N_ref, shift, C_ref, ld_ref, X, ldx,
                                 D, weights, cand, K, best_k));
    return motion_search_enqueue(who, keys_sorted, N, J, block_first, n_blocks, ref_keys_sorted, N_ref, shift, C_ref, ld_ref, X, ldx, D, weights,
                                 cand, K, nullptr, best_k, best_cost, nullptr, cost_table, (hipStream_t)stream);
}

int raht_motion_search_around(const uint64_t *keys_sorted, int64_t N, int J, int block_log2, const int64_t *block_first, int64_t n_blocks,
                              const uint64_t *ref_keys_sorted, int64_t N_ref, int shift, const float *C_ref, int64_t ld_ref, const float *X,
                              int64_t ldx, int D, const float *weights, const int8_t *base, const int32_t *cand, int K, int32_t *best_k,
                              uint64_t *best_cost, int8_t *mv, uint64_t *cost_table, raht_stream_t stream)
{
    const char *who = "raht_motion_search_around";
    if (!base || !mv) { set_error("%s: NULL base or mv", who); return RAHT_ERR_INVALID; }
    RAHT_RET(motion_search_check(who, keys_sorted, N, J, block_log2, block_first, n_blocks, ref_keys_sorted, N_ref, shift, C_ref, ld_ref, X, ldx,
                                 D, weights, cand, K, best_k));
    return motion_search_enqueue(who, keys_sorted, N, J, block_first, n_blocks, ref_keys_sorted, N_ref, shift, C_ref, ld_ref, X, ldx, D, weights,
                                 cand, K, base, best_k, best_cost, mv, cost_table, (hipStream_t)stream);
}

int raht_predict_mc(const uint64_t *keys_sorted, int64_t N, int J, int block_log2, const int64_t *block_first, int64_t n_blocks,
                    const int8_t *mv, const uint64_t *ref_keys_sorted, int64_t N_ref, int shift, const float *C_ref, int64_t ld_ref,
                    const float *X, int64_t ldx, int D, int add, float *Y, int64_t ldy, int64_t *n_matched, raht_stream_t stream)
{
    const char *who = "raht_predict_mc";
    if (!mv) { set_error("%s: NULL mv", who); return RAHT_ERR_INVALID; }
    RAHT_RET(predict_check(who, keys_sorted, N, ref_keys_sorted, N_ref, shift, C_ref, ld_ref, X, ldx, D, add, Y, ldy));
    RAHT_RET(motion_check_blocks(who, J, block_log2, block_first, n_blocks, N));
    return predict_enqueue(keys_sorted, N, ref_keys_sorted, N_ref, shift, C_ref, ld_ref, X, ldx, D, add, Y, ldy, n_matched,
                           MvKey{block_first, n_blocks, mv, J}, (hipStream_t)stream);
}

}  // extern "C"
