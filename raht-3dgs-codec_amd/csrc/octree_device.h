// octree_device.h -- the level walks of the octree geometry coder, shared by the intra coder (octree.hip) and the coder of a
// frame predicted from a reference frame (octree_inter.hip): one level up (children's keys -> parents' keys and occupancy
// bytes), one level down (parents' keys and bytes -> children's keys), the kernels and the host loops around them.
//
// Both loops take a HOOK that sees every level's node keys next to the level's bytes: the intra coder passes OctNoHook (nothing
// is generated for it), the predicted coder XORs the bytes with the reference frame's occupancy of the same cells
//   encode   after a level's bytes and node keys are written   (occupancy -> residual, in place)
//   decode   before a level's bytes are expanded               (residual -> occupancy, into a buffer of its own)
// A hook has  static constexpr bool active;
//             __device__ void level(int g, const uint64_t *node_keys, int64_t n, int64_t off) const;   (a whole workgroup calls it)
//             int launch(int g, const uint64_t *node_keys, int64_t n, int64_t off, hipStream_t s) const;
// g: the level, node_keys: its n ascending cell keys (NULL: the root), off: where the level starts in the stream.
#pragma once
#include "raht_common.h"
#include "raht_device.h"

namespace raht {

constexpr int OCT_THREADS = 256;                         // one workgroup size everywhere in the octree files
constexpr int OCT_ITEMS = 8;                             // consecutive nodes per thread
constexpr int OCT_CHUNK = OCT_THREADS * OCT_ITEMS;       // nodes per workgroup step
constexpr int OCT_MAX_GRID = 2048;                       // grids are capped and grid-strided
constexpr int OCT_SELF_PREFIX = 2048;                    // up to this many chunks a workgroup sums the chunks before it by itself
constexpr int OCT_MAX_J = 21;

struct OctCounts { int64_t n[OCT_MAX_J + 1]; };

struct OctNoHook {
    static constexpr bool active = false;
    __device__ __forceinline__ void level(int, const uint64_t *, int64_t, int64_t) const {}
    int launch(int, const uint64_t *, int64_t, int64_t, hipStream_t) const { return RAHT_OK; }
};

// exclusive prefix of v over the workgroup (256 threads) and the workgroup's total; reusable inside a loop
__device__ __forceinline__ uint32_t oct_block_scan(uint32_t v, uint32_t *total)
{
    __shared__ uint32_t wsum[OCT_THREADS / RAHT_WAVE];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < RAHT_WAVE; d <<= 1) {
        const uint32_t t = __shfl_up(inc, d, RAHT_WAVE);
        if (lane >= d) inc += t;
    }
    __syncthreads();                                     // the previous call's readers are done with wsum
    if (lane == RAHT_WAVE - 1) wsum[wid] = inc;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < OCT_THREADS / RAHT_WAVE; ++w) {
        const uint32_t c = wsum[w];
        if (w < wid) base += c;
        tot += c;
    }
    *total = tot;
    return base + inc - v;
}

// number of items of the chunks before chunk c: blk already scanned, or summed here
__device__ __forceinline__ uint32_t oct_before(const uint32_t *blk, int64_t c, int scanned)
{
    if (scanned) return blk[c];
    uint32_t part = 0, tot;
    for (int64_t b = threadIdx.x; b < c; b += OCT_THREADS) part += blk[b];
    (void)oct_block_scan(part, &tot);
    return tot;
}

// ---- encode: one level up ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool oct_is_head(int64_t i, int64_t n, uint64_t x, uint64_t prev)
{
    return i < n && (i == 0 || (x >> 3) != (prev >> 3));
}

__device__ __forceinline__ void oct_load_chunk(const uint64_t *cur, int64_t n, int64_t base, uint64_t (&x)[OCT_ITEMS], uint64_t &prev)
{
#pragma unroll
    for (int k = 0; k < OCT_ITEMS; ++k) x[k] = (base + k < n) ? cur[base + k] : 0ull;
    prev = (base > 0 && base < n) ? cur[base - 1] : 0ull;
}

__device__ __forceinline__ uint32_t oct_count_heads(int64_t n, int64_t base, const uint64_t (&x)[OCT_ITEMS], uint64_t prev)
{
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < OCT_ITEMS; ++k) c += oct_is_head(base + k, n, x[k], k ? x[k - 1] : prev) ? 1u : 0u;
    return c;
}

// chunk c of level g + 1 (cur, n keys) -> its parents' keys and occupancy bytes at rank `before` + (rank inside the chunk).
// A head's run may reach into the items of the following threads: those (at most 7) keys are read again.
__device__ __forceinline__ void oct_up_chunk(const uint64_t *cur, int64_t n, int64_t c, uint32_t before, uint64_t *parent,
                                             uint8_t *occ, int64_t n_parent)
{
    const int64_t base = c * OCT_CHUNK + (int64_t)threadIdx.x * OCT_ITEMS;
    uint64_t x[OCT_ITEMS], prev;
    oct_load_chunk(cur, n, base, x, prev);
    uint32_t tot;
    int64_t pos = (int64_t)before + oct_block_scan(oct_count_heads(n, base, x, prev), &tot);
    bool open = false;
    uint32_t byte = 0;
    uint64_t pk = 0;
#pragma unroll
    for (int k = 0; k < OCT_ITEMS; ++k) {
        if (oct_is_head(base + k, n, x[k], k ? x[k - 1] : prev)) {
            if (open) {
                if (pos < n_parent) { occ[pos] = (uint8_t)byte; parent[pos] = pk; }
                ++pos;
            }
            open = true;
            byte = 0;
            pk = x[k] >> 3;
        }
        if (open && base + k < n) byte |= 1u << (uint32_t)(x[k] & 7ull);
    }
    if (open) {
        for (int64_t j = base + OCT_ITEMS; j < n && j < base + OCT_ITEMS + 7; ++j) {
            const uint64_t y = cur[j];
            if ((y >> 3) != pk) break;
            byte |= 1u << (uint32_t)(y & 7ull);
        }
        if (pos < n_parent) { occ[pos] = (uint8_t)byte; parent[pos] = pk; }
    }
}

static __global__ __launch_bounds__(OCT_THREADS) void oct_head_count_kernel(const uint64_t *__restrict__ cur, int64_t n, int64_t nchunks,
                                                                            uint32_t *__restrict__ blk)
{
    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int64_t base = c * OCT_CHUNK + (int64_t)threadIdx.x * OCT_ITEMS;
        uint64_t x[OCT_ITEMS], prev;
        oct_load_chunk(cur, n, base, x, prev);
        uint32_t tot;
        (void)oct_block_scan(oct_count_heads(n, base, x, prev), &tot);
        if (threadIdx.x == 0) blk[c] = tot;
    }
}

static __global__ __launch_bounds__(OCT_THREADS) void oct_level_up_kernel(const uint64_t *__restrict__ cur, int64_t n, int64_t nchunks,
                                                                          const uint32_t *__restrict__ blk, int scanned,
                                                                          uint64_t *__restrict__ parent, uint8_t *__restrict__ occ,
                                                                          int64_t n_parent)
{
    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) oct_up_chunk(cur, n, c, oct_before(blk, c, scanned), parent, occ, n_parent);
}

// the coarse levels: steps g = g_first, g_first - 1, ... 0 (each reads level g + 1, at most one chunk) in one workgroup
template <typename Hook>
__global__ __launch_bounds__(OCT_THREADS) void oct_top_up_kernel(const uint64_t *src, uint64_t *a, uint64_t *b, int g_first,
                                                                 const OctCounts cn, uint8_t *occ, const Hook hook)
{
    int64_t off = 0;
    for (int g = 0; g < g_first; ++g) off += cn.n[g];
    const uint64_t *cur = src;
    uint64_t *dst = a, *other = b;
    for (int g = g_first; g >= 0; --g) {
        oct_up_chunk(cur, cn.n[g + 1], 0, 0u, dst, occ + off, cn.n[g]);
        __syncthreads();                                 // this level's parent keys are the next step's input
        if (Hook::active) hook.level(g, dst, cn.n[g], off);              // (a thread touches its own bytes only)
        cur = dst;
        uint64_t *t = dst; dst = other; other = t;
        if (g > 0) off -= cn.n[g - 1];
    }
}

// ---- decode: one level down --------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t oct_load_bytes(const uint8_t *occ, int64_t n, int64_t base, uint32_t (&o)[OCT_ITEMS])
{
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < OCT_ITEMS; ++k) {
        o[k] = (base + k < n) ? (uint32_t)occ[base + k] : 0u;
        c += (uint32_t)__popc(o[k]);
    }
    return c;
}

// chunk c of level g (n parents: keys `parent`, or the root when parent == NULL; bytes occ) -> the keys of its children. Every
// store is bounded by n_child; a zero byte, or a level whose popcounts do not add up to n_child, raises *bad.
__device__ __forceinline__ void oct_down_chunk(const uint64_t *parent, const uint8_t *occ, int64_t n, int64_t c, int64_t nchunks,
                                               uint32_t before, uint64_t *child, int64_t n_child, int32_t *bad)
{
    const int64_t base = c * OCT_CHUNK + (int64_t)threadIdx.x * OCT_ITEMS;
    uint32_t o[OCT_ITEMS], tot;
    const uint32_t cnt = oct_load_bytes(occ, n, base, o);
    int64_t pos = (int64_t)before + oct_block_scan(cnt, &tot);
    bool zero = false;
#pragma unroll
    for (int k = 0; k < OCT_ITEMS; ++k) {
        if (base + k < n) {
            const uint64_t pk = parent ? parent[base + k] : 0ull;
            zero |= o[k] == 0u;
            for (uint32_t m = o[k]; m; m &= m - 1u) {
                if (pos < n_child) child[pos] = (pk << 3) | (uint64_t)(__ffs((int)m) - 1);
                ++pos;
            }
        }
    }
    if (zero) *bad = 1;
    if (c == nchunks - 1 && threadIdx.x == 0 && (int64_t)before + (int64_t)tot != n_child) *bad = 1;
}

static __global__ __launch_bounds__(OCT_THREADS) void oct_pop_count_kernel(const uint8_t *__restrict__ occ, int64_t n, int64_t nchunks,
                                                                           uint32_t *__restrict__ blk)
{
    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        uint32_t o[OCT_ITEMS], tot;
        (void)oct_block_scan(oct_load_bytes(occ, n, c * OCT_CHUNK + (int64_t)threadIdx.x * OCT_ITEMS, o), &tot);
        if (threadIdx.x == 0) blk[c] = tot;
    }
}

static __global__ __launch_bounds__(OCT_THREADS) void oct_level_down_kernel(const uint64_t *__restrict__ parent, const uint8_t *__restrict__ occ,
                                                                            int64_t n, int64_t nchunks, const uint32_t *__restrict__ blk,
                                                                            int scanned, uint64_t *__restrict__ child, int64_t n_child,
                                                                            int32_t *bad)
{
    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x)
        oct_down_chunk(parent, occ, n, c, nchunks, oct_before(blk, c, scanned), child, n_child, bad);
}

// steps g = 0 .. g_end - 1 (each at most one chunk of parents) in one workgroup; step g writes into (g & 1) ? b : a
template <typename Hook>
__global__ __launch_bounds__(OCT_THREADS) void oct_top_down_kernel(const uint8_t *occ, int g_end, const OctCounts cn, uint64_t *a,
                                                                   uint64_t *b, int32_t *bad, const Hook hook)
{
    int64_t off = 0;
    const uint64_t *cur = nullptr;
    for (int g = 0; g < g_end; ++g) {
        uint64_t *dst = (g & 1) ? b : a;
        if (Hook::active) {
            hook.level(g, cur, cn.n[g], off);
            __syncthreads();                             // the level's bytes are whole before they are expanded
        }
        oct_down_chunk(cur, occ + off, cn.n[g], 0, 1, 0u, dst, cn.n[g + 1], bad);
        __syncthreads();
        cur = dst;
        off += cn.n[g];
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------
static inline unsigned oct_grid(int64_t items, int64_t per_block, int cap = OCT_MAX_GRID)
{
    const int64_t g = ceil_div(items, per_block);
    return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

// the plausibility rules of a count list (the header of a geometry section comes off the wire)
static inline int oct_check_counts(const char *what, const int64_t *counts, int J, int64_t *n_nodes)
{
    if (J < 1 || J > OCT_MAX_J) { set_error("%s: J must be 1 .. 21", what); return RAHT_ERR_INVALID; }
    if (!counts) { set_error("%s: NULL counts", what); return RAHT_ERR_INVALID; }
    if (counts[0] != 1) { set_error("%s: counts[0] must be 1 (the root)", what); return RAHT_ERR_INVALID; }
    int64_t tot = 0;
    for (int g = 0; g < J; ++g) {
        if (counts[g + 1] < counts[g] || counts[g + 1] > 8 * counts[g] || counts[g + 1] >= ((int64_t)1 << 31)) {
            set_error("%s: counts[%d] = %lld does not go with counts[%d] = %lld (n_g <= n_g+1 <= 8 n_g, below 2^31)", what, g + 1,
                      (long long)counts[g + 1], g, (long long)counts[g]);
            return RAHT_ERR_INVALID;
        }
        tot += counts[g];
    }
    *n_nodes = tot;
    return RAHT_OK;
}

static inline void oct_fill(OctCounts &cn, const int64_t *counts, int J)
{
    for (int g = 0; g <= OCT_MAX_J; ++g) cn.n[g] = g <= J ? counts[g] : 0;
}

// THE bottom-up walk: occ[n_nodes] from the keys and checked counts (n_nodes their sum); `hook` after every level. Enqueues only.
template <typename Hook>
static int oct_encode_levels(const char *what, const uint64_t *keys_sorted, int64_t N, int J, const int64_t *counts, int64_t n_nodes,
                             uint8_t *occ, const Hook &hook, hipStream_t s)
{
    Scratch ka(sizeof(uint64_t) * (size_t)counts[J - 1], s), kb(sizeof(uint64_t) * (size_t)(J > 1 ? counts[J - 2] : 1), s);
    Scratch blk(sizeof(uint32_t) * (size_t)ceil_div(N, OCT_CHUNK), s);
    if (!ka.ok() || !kb.ok() || !blk.ok()) { set_error("%s: out of device memory", what); return RAHT_ERR_NOMEM; }
    OctCounts cn;
    oct_fill(cn, counts, J);
    uint64_t *bufs[2] = {ka.as<uint64_t>(), kb.as<uint64_t>()};
    const uint64_t *src = keys_sorted;
    int w = 0, g = J - 1;
    int64_t off = n_nodes;
    for (; g >= 0 && counts[g + 1] > OCT_CHUNK; --g) {
        const int64_t n = counts[g + 1], nchunks = ceil_div(n, OCT_CHUNK);
        const int scanned = nchunks > OCT_SELF_PREFIX;
        off -= counts[g];
        hipLaunchKernelGGL(oct_head_count_kernel, dim3(oct_grid(nchunks, 1)), dim3(OCT_THREADS), 0, s, src, n, nchunks,
                           blk.as<uint32_t>());
        if (scanned) RAHT_RET(exclusive_scan_u32(blk.as<uint32_t>(), blk.as<uint32_t>(), nchunks, nullptr, s));
        hipLaunchKernelGGL(oct_level_up_kernel, dim3(oct_grid(nchunks, 1)), dim3(OCT_THREADS), 0, s, src, n, nchunks,
                           (const uint32_t *)blk.as<uint32_t>(), scanned, bufs[w], occ + off, counts[g]);
        RAHT_RET(hook.launch(g, bufs[w], counts[g], off, s));
        src = bufs[w];
        w ^= 1;
    }
    if (g >= 0)
        hipLaunchKernelGGL(oct_top_up_kernel<Hook>, dim3(1), dim3(OCT_THREADS), 0, s, src, bufs[w], bufs[w ^ 1], g, cn, occ, hook);
    RAHT_HIP_CHECK(hipGetLastError());
    return RAHT_OK;
}

// THE top-down walk: keys[counts[J]] from the stream occ and checked counts; `hook` before every level is expanded (an active
// hook WRITES occ). Enqueues only; every store is bounded by the counts.
template <typename Hook>
static int oct_decode_levels(const char *what, const uint8_t *occ, const int64_t *counts, int J, uint64_t *keys, int32_t *bad,
                             const Hook &hook, hipStream_t s)
{
    const int64_t N = counts[J];
    Scratch tmp(sizeof(uint64_t) * (size_t)counts[J - 1], s);
    Scratch blk(sizeof(uint32_t) * (size_t)ceil_div(N, OCT_CHUNK), s);
    if (!tmp.ok() || !blk.ok()) { set_error("%s: out of device memory", what); return RAHT_ERR_NOMEM; }
    OctCounts cn;
    oct_fill(cn, counts, J);
    // step g writes level g + 1; the last step (g = J - 1) writes `keys`, the steps before it alternate
    uint64_t *even = ((J - 1) & 1) ? tmp.as<uint64_t>() : keys, *odd = ((J - 1) & 1) ? keys : tmp.as<uint64_t>();
    int g_end = 1;
    while (g_end < J && counts[g_end] <= OCT_CHUNK) ++g_end;
    hipLaunchKernelGGL(oct_top_down_kernel<Hook>, dim3(1), dim3(OCT_THREADS), 0, s, occ, g_end, cn, even, odd, bad, hook);
    int64_t off = 0;
    for (int g = 0; g < g_end; ++g) off += counts[g];
    for (int g = g_end; g < J; ++g) {
        const int64_t n = counts[g], nchunks = ceil_div(n, OCT_CHUNK);
        const int scanned = nchunks > OCT_SELF_PREFIX;
        const uint64_t *parent = ((g - 1) & 1) ? odd : even;
        uint64_t *child = (g & 1) ? odd : even;
        RAHT_RET(hook.launch(g, parent, n, off, s));
        hipLaunchKernelGGL(oct_pop_count_kernel, dim3(oct_grid(nchunks, 1)), dim3(OCT_THREADS), 0, s, occ + off, n, nchunks,
                           blk.as<uint32_t>());
        if (scanned) RAHT_RET(exclusive_scan_u32(blk.as<uint32_t>(), blk.as<uint32_t>(), nchunks, nullptr, s));
        hipLaunchKernelGGL(oct_level_down_kernel, dim3(oct_grid(nchunks, 1)), dim3(OCT_THREADS), 0, s, parent, occ + off, n, nchunks,
                           (const uint32_t *)blk.as<uint32_t>(), scanned, child, counts[g + 1], bad);
        off += n;
    }
    RAHT_HIP_CHECK(hipGetLastError());
    return RAHT_OK;
}

}  // namespace raht
