// mode_search.hip -- the per-block choice among the predictors of a B frame (include/raht.h, "Block modes"). A block
// (raht_motion_search's: a cell of the octree level block_log2 above the voxels, one run of the sorted keys) is predicted in one of
// four ways: 0 the two-reference rule of raht_predict_bi, 1 from reference 0 alone, 2 from reference 1 alone, 3 not at all. The cost
// of a row under a mode is raht_motion_search's row cost against that mode's prediction, a block's cost the integer sum over its
// rows; the smallest cost wins, the smallest mode among equals.
//
//   raht_mode_search   memset of the cost table, then
//     search   the motion search's tile (predict_device.h): MS tile rows per workgroup step, one thread per row, the weighted columns
//              of the tile's X rows staged in LDS (D <= 243; wider matrices read X through the cache). A row resolves its key ONCE
//              per reference (shifted by its block's vector under a field), then walks the weighted columns once: m0, m1 and the
//              two-reference mean are formed in registers and the four costs accumulate side by side in the order of the
//              definition (product rounded before the sum). The four fixed-point costs are summed per block one after the other by
//              ms_block_add: ONE 64-bit atomic per (block, mode, workgroup). Integer sums: the table does not depend on how a block
//              is cut into tiles or waves.
//     select   one thread per block: the smallest cost, the smallest mode among equals.
#include <optional>

#include "predict_device.h"

namespace raht {

constexpr int MD_MODES = 4;

// STAGED: blockDim.x rows per tile, their weighted columns in LDS. Otherwise X and the weights are read through the cache.
// KEY0 / KEY1: the key a row is resolved for in reference 0 / 1 (SameKey or MvKey).
template <bool STAGED, typename KEY0, typename KEY1>
__global__ __launch_bounds__(MS_THREADS) void mode_search_kernel(const uint64_t *__restrict__ keys, int64_t n,
                                                                const int64_t *__restrict__ block_first, int64_t n_blocks, const PrRef r0,
                                                                const PrRef r1, int shift, const float *__restrict__ X, int64_t ldx, int D,
                                                                const float *__restrict__ weights, unsigned long long *__restrict__ table,
                                                                int x_stride, const KEY0 key0, const KEY1 key1)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char md_lds[];
    __shared__ int n_weighted;
    const int tile = (int)blockDim.x, tid = (int)threadIdx.x, lane = tid & 63;
    unsigned long long *acc = (unsigned long long *)md_lds;                      // [2][tile]
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
        const int64_t r0w = t * tile;
        const int rows = (int)min((int64_t)tile, n - r0w);
        const bool active = tid < rows;
        __syncthreads();                                 // the previous step's readers are done with xs, its flushes with acc
        if constexpr (STAGED) {
            for (int e = tid; e < rows * nw; e += tile) {
                const int r = e / nw, j = e - r * nw;
                xs[r * x_stride + j] = X[(r0w + r) * ldx + wcol[j]];
            }
        }
        // this row: its run in either reference, its block, the slot of its block in the tile (the block's first row of the tile)
        int4 r = make_int4(0, 0, 0, 0);                  // (lo0, len0, lo1, len1)
        int64_t b = 0;
        int slot = -1;
        if (active) {
            const int64_t row = r0w + tid;
            const uint64_t own = keys[row];
            uint64_t key;
            if (key0(row, own, key)) r.y = pr_resolve(r0.keys, r0.n, shift, key, r.x);
            if (key1(row, own, key)) r.w = pr_resolve(r1.keys, r1.n, shift, key, r.z);
            b = pr_block_of(block_first, n_blocks, row);
            const int64_t first = block_first[b] - r0w;  // (bounded for any block_first: 0 <= slot <= tid)
            slot = (int)(first < 0 ? 0 : (first > tid ? tid : first));
        }
        const int slot_next = __shfl_down(slot, 1);
        const bool tail = active && (lane == 63 || slot_next != slot);           // the last lane of its block in this wave
        const bool head = active && slot == tid;                                 // the block's first row of the tile flushes
        __syncthreads();                                 // xs is staged
        unsigned long long q[MD_MODES] = {0, 0, 0, 0};
        if (active) {
            float c[MD_MODES] = {0.0f, 0.0f, 0.0f, 0.0f};
            // one weighted column: the two means, the four predictions, the four costs
            auto column = [&](float x, float w, int ch) {
                const float m0 = pr_mean(r0.C, r0.ld, r.x, r.y, ch), m1 = pr_mean(r1.C, r1.ld, r.z, r.w, ch);
                const float p[MD_MODES] = {pr_bi(m0, r.y, m1, r.w), m0, m1, 0.0f};
#pragma unroll
                for (int k = 0; k < MD_MODES; ++k) c[k] = __fadd_rn(c[k], __fmul_rn(w, fabsf(__fsub_rn(x, p[k]))));
            };
            if constexpr (STAGED) {
                const float *x = xs + tid * x_stride;
                for (int j = 0; j < nw; ++j) column(x[j], wval[j], wcol[j]);
            } else {
                const float *x = X + (r0w + tid) * ldx;
                for (int ch = 0; ch < D; ++ch) {
                    const float w = weights[ch];
                    if (w != 0.0f) column(x[ch], w, ch);
                }
            }
#pragma unroll
            for (int k = 0; k < MD_MODES; ++k) q[k] = ms_fixed(c[k]);
        }
#pragma unroll
        for (int k = 0; k < MD_MODES; ++k) ms_block_add(q[k], slot, lane, tid, tail, head, acc + (k & 1) * tile, table + b * MD_MODES + k);
    }
}

__global__ __launch_bounds__(MS_THREADS) void mode_select_kernel(const unsigned long long *__restrict__ table, int64_t n_blocks,
                                                                uint8_t *__restrict__ mode, unsigned long long *__restrict__ best_cost)
{
    for (int64_t b = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x; b < n_blocks; b += (int64_t)gridDim.x * MS_THREADS) {
        const unsigned long long *row = table + b * MD_MODES;
        unsigned long long best = row[0];
        uint8_t at = 0;
#pragma unroll
        for (int k = 1; k < MD_MODES; ++k) {
            const unsigned long long v = row[k];
            if (v < best) { best = v; at = (uint8_t)k; }  // strictly smaller: the smallest mode among equals stays
        }
        mode[b] = at;
        if (best_cost) best_cost[b] = best;
    }
}

struct ModeLaunch {
    dim3 grid, wg;
    size_t lds;
    bool staged;
    hipStream_t s;
    const uint64_t *keys;
    int64_t N;
    const int64_t *block_first;
    int64_t n_blocks;
    PrRef r0, r1;
    int shift;
    const float *X;
    int64_t ldx;
    int D;
    const float *weights;
    unsigned long long *table;
    int x_stride;
};

template <typename KEY0, typename KEY1>
static void mode_search_launch(const ModeLaunch &a, const KEY0 &key0, const KEY1 &key1)
{
    auto *kernel = a.staged ? mode_search_kernel<true, KEY0, KEY1> : mode_search_kernel<false, KEY0, KEY1>;
    hipLaunchKernelGGL(kernel, a.grid, a.wg, a.lds, a.s, a.keys, a.N, a.block_first, a.n_blocks, a.r0, a.r1, a.shift, a.X, a.ldx, a.D,
                       a.weights, a.table, a.x_stride, key0, key1);
}

}  // namespace raht

using namespace raht;

extern "C" {

int raht_mode_search(const uint64_t *keys_sorted, int64_t N, int J, int block_log2, const int64_t *block_first, int64_t n_blocks,
                     const int8_t *mv0, const int8_t *mv1, const uint64_t *ref0_keys_sorted, int64_t N_ref0, const float *C_ref0,
                     int64_t ld_ref0, const uint64_t *ref1_keys_sorted, int64_t N_ref1, const float *C_ref1, int64_t ld_ref1, int shift,
                     const float *X, int64_t ldx, int D, const float *weights, uint8_t *mode, uint64_t *best_cost, uint64_t *cost_table,
                     raht_stream_t stream)
{
    const char *who = "raht_mode_search";
    if (!X || !weights || !mode) { set_error("%s: NULL X, weights or mode", who); return RAHT_ERR_INVALID; }
    // (the predictor's rules for either reference: X stands in for the output, whose stride is then X's)
    RAHT_RET(predict_check(who, keys_sorted, N, ref0_keys_sorted, N_ref0, shift, C_ref0, ld_ref0, X, ldx, D, 0, X, ldx));
    RAHT_RET(predict_check(who, keys_sorted, N, ref1_keys_sorted, N_ref1, shift, C_ref1, ld_ref1, X, ldx, D, 0, X, ldx));
    RAHT_RET(motion_check_blocks(who, J, block_log2, block_first, n_blocks, N));
    hipStream_t s = (hipStream_t)stream;
    return guarded(who, [&]() -> int {
        const size_t table_bytes = sizeof(uint64_t) * (size_t)n_blocks * MD_MODES;
        std::optional<Scratch> ws;                       // (the caller's table, or one from the pool)
        if (!cost_table) {
            ws.emplace(table_bytes, s);
            if (!ws->ok()) { set_error("%s: out of device memory", who); return RAHT_ERR_NOMEM; }
        }
        ModeLaunch a;
        a.table = cost_table ? (unsigned long long *)cost_table : ws->as<unsigned long long>();
        RAHT_HIP_CHECK(hipMemsetAsync(a.table, 0, table_bytes, s));
        // the motion search's tile: the largest whose rows fit the LDS budget; none: X through the cache
        const int staged_rows = ms_tile_rows(D);
        a.staged = staged_rows != 0;
        a.x_stride = a.staged ? (D | 1) : 0;
        const int tile = a.staged ? staged_rows : MS_THREADS;
        const int64_t tiles = ceil_div(N, tile);
        a.grid = dim3((unsigned)(tiles > MS_MAX_GRID ? MS_MAX_GRID : tiles));
        a.wg = dim3(tile);
        a.lds = a.staged ? ms_lds_bytes(tile, D, a.x_stride) : ms_lds_bytes(tile, 0, 0);
        a.s = s;
        a.keys = keys_sorted;
        a.N = N;
        a.block_first = block_first;
        a.n_blocks = n_blocks;
        a.r0 = PrRef{ref0_keys_sorted, (int32_t)N_ref0, C_ref0, ld_ref0};
        a.r1 = PrRef{ref1_keys_sorted, (int32_t)N_ref1, C_ref1, ld_ref1};
        a.shift = shift;
        a.X = X;
        a.ldx = ldx;
        a.D = D;
        a.weights = weights;
        const MvKey f0{block_first, n_blocks, mv0, J}, f1{block_first, n_blocks, mv1, J};
        if (mv0 && mv1) mode_search_launch(a, f0, f1);
        else if (mv0) mode_search_launch(a, f0, SameKey());
        else if (mv1) mode_search_launch(a, SameKey(), f1);
        else mode_search_launch(a, SameKey(), SameKey());
        RAHT_HIP_CHECK(hipGetLastError());
        const int64_t sel = ceil_div(n_blocks, MS_THREADS);
        hipLaunchKernelGGL(mode_select_kernel, dim3((unsigned)(sel > MS_MAX_GRID ? MS_MAX_GRID : sel)), dim3(MS_THREADS), 0, s, a.table, n_blocks,
                           mode, (unsigned long long *)best_cost);
        RAHT_HIP_CHECK(hipGetLastError());
        return RAHT_OK;
    });
}

}  // extern "C"
