// tile_host.h -- host-side pieces shared by the two tile engines (transform.hip: float32 / float64, transform_mx.hip: mixed
// precision): the launch of a kernel with a large dynamic LDS block, the IDENT x SLOTS dispatch, the plan check and the
// round-by-round grouping of a batch. Host code only.
#pragma once
#include "raht_common.h"

#include <algorithm>
#include <type_traits>

namespace raht {

constexpr int BATCH_MAX = 8;                               // scenes per launch of the batch kernels (raht_*_batch)
constexpr size_t TILE_LDS_LIMIT = 160 * 1024;              // dynamic LDS a tile kernel may ask for ...
constexpr size_t TOP_LDS_LIMIT = 160 * 1024 - 1024;        // ... and a top kernel (which also has static LDS)

// Launch of a kernel whose dynamic LDS block may pass 64 KiB: that must be allowed per function AND per device, once.
template <auto Kernel, typename... Args>
static int launch_lds(dim3 grid, dim3 block, size_t lds_bytes, size_t lds_limit, hipStream_t s, const Args &...args)
{
    static PerDeviceOnce attr;
    if (attr.first(current_device()))
        RAHT_HIP_CHECK(hipFuncSetAttribute((const void *)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_limit));
    hipLaunchKernelGGL(Kernel, grid, block, lds_bytes, s, args...);
    RAHT_HIP_CHECK(hipGetLastError());
    return RAHT_OK;
}

// f(IDENT, SLOTS) with the two as compile-time constants (decltype(ident)::value): the tile kernels are instantiated for stage 0
// (identity row list) or a later stage, and for one or two rows per thread.
template <typename F>
static int by_ident_slots(bool ident, bool one_slot, F &&f)
{
    typedef std::integral_constant<int, 1> S1;
    typedef std::integral_constant<int, 2> S2;
    if (ident) return one_slot ? f(std::true_type{}, S1{}) : f(std::true_type{}, S2{});
    return one_slot ? f(std::false_type{}, S1{}) : f(std::false_type{}, S2{});
}

// The plans of a batch, before any of them is dereferenced: none is NULL, none appears twice.
static inline int check_batch_plans(const char *what, int n, raht_plan *const *plans)
{
    for (int i = 0; i < n; ++i) {
        if (!plans[i]) { set_error("%s: NULL plan (scene %d)", what, i); return RAHT_ERR_INVALID; }
        for (int j = 0; j < i; ++j)
            if (plans[j] == plans[i]) { set_error("%s: scenes %d and %d share a plan (a plan owns its workspaces)", what, j, i); return RAHT_ERR_INVALID; }
    }
    return RAHT_OK;
}

// THE grouping of a batch. n_stages(i): stages of scene i's schedule, 0 = the scene runs through its single-scene call;
// is_top(i, k): stage k of scene i is a top stage; same_tile(i, j, k) / same_top(i, j, k): stage k of scenes i and j may share a
// launch. Calls single(i) for every scene without a schedule first, in place in the stream; then round r of the forward direction
// carries stage r of every scene that has one (inverse: the rounds backwards from the deepest schedule, a scene joining when its
// own last stage comes up). Within a round the tile stages of equal launch shape go out up to BATCH_MAX scenes per launch,
// tile(m, idx, k) = stage k of the m scenes idx[0..m), the top stages likewise through top(m, idx, k). Counts what it called: the
// runners pass callbacks that launch, raht_mixed_batch_stats callbacks that do nothing.
struct BatchCounts { int tile = 0, top = 0, single = 0; };

template <bool INV, typename NS, typename IT, typename ST, typename SP, typename FS, typename FT, typename FP>
static int group_batch_rounds(int n, NS &&n_stages, IT &&is_top, ST &&same_tile, SP &&same_top, BatchCounts &cnt, FS &&single,
                              FT &&tile, FP &&top)
{
    int maxK = 0;
    for (int i = 0; i < n; ++i) {
        if (n_stages(i) == 0) { ++cnt.single; RAHT_RET(single(i)); }
        else maxK = std::max(maxK, n_stages(i));
    }
    for (int r = 0; r < maxK; ++r) {
        const int k = INV ? maxK - 1 - r : r;
        int idx_tile[BATCH_MAX], idx_top[BATCH_MAX], n_tile = 0, n_top = 0;
        auto flush_tile = [&]() -> int {
            if (n_tile == 0) return RAHT_OK;
            const int m = n_tile;
            n_tile = 0;
            ++cnt.tile;
            return tile(m, idx_tile, k);
        };
        auto flush_top = [&]() -> int {
            if (n_top == 0) return RAHT_OK;
            const int m = n_top;
            n_top = 0;
            ++cnt.top;
            return top(m, idx_top, k);
        };
        for (int i = 0; i < n; ++i) {
            if (k >= n_stages(i)) continue;
            if (is_top(i, k)) {
                if (n_top > 0 && !same_top(i, idx_top[0], k)) RAHT_RET(flush_top());
                idx_top[n_top++] = i;
                if (n_top == BATCH_MAX) RAHT_RET(flush_top());
            } else {
                if (n_tile > 0 && !same_tile(i, idx_tile[0], k)) RAHT_RET(flush_tile());     // another launch shape: its own launch
                idx_tile[n_tile++] = i;
                if (n_tile == BATCH_MAX) RAHT_RET(flush_tile());
            }
        }
        RAHT_RET(flush_tile());
        RAHT_RET(flush_top());
    }
    return RAHT_OK;
}

}  // namespace raht
