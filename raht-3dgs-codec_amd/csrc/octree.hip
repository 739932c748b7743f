// octree.hip -- lossless geometry: the breadth-first octree occupancy code of the occupied voxels (include/raht.h,
// "Octree geometry"). The input is what every plan is built from -- strictly ascending Morton keys -- and the output is one
// occupancy byte per internal node, level 0 first, ascending key order inside a level.
//
//   counts   one pass over the leaf keys: row i opens a new node at every level deeper than the number c_i of leading base-8
//            digits it shares with row i - 1, so a J-bin histogram of c_i gives every level's node count (and the same pass
//            checks order and range). Everything after it is sized from these counts: no buffer is allocated by guesswork.
//   encode   bottom-up, one level per step: the nodes of level g + 1 are an ascending key array, the run heads of key >> 3 are
//            the parents, a parent's children are contiguous and at most 8, so the thread that holds the head ORs its followers'
//            digits and writes one byte and one parent key -- no atomics, deterministic. Two launches per level (head counts
//            per 2048-node chunk; ranks + bytes), two ping-pong key arrays; every level of at most one chunk is finished by
//            ONE single-workgroup launch that walks the remaining levels.
//   decode   top-down, the mirror image: popcounts per chunk; offsets + expansion (parent << 3 | digit). No host round trip:
//            the header's counts size every level, and every write index is bounded by them whatever the bytes say.
//   symbols  256-bin histogram (per-wave LDS bins, one global atomic per non-empty bin per workgroup), the rank table on the
//            device (descending count, ties by ascending byte), byte -> int32 rank for the segmented RLGR coder; and back.
#include "raht_common.h"
#include "raht_device.h"

#include <cstring>

namespace raht {

constexpr int OCT_THREADS = 256;                         // one workgroup size everywhere in this file
constexpr int OCT_ITEMS = 8;                             // consecutive nodes per thread
constexpr int OCT_CHUNK = OCT_THREADS * OCT_ITEMS;       // nodes per workgroup step
constexpr int OCT_MAX_GRID = 2048;                       // grids are capped and grid-strided
constexpr int OCT_SELF_PREFIX = 2048;                    // up to this many chunks a workgroup sums the chunks before it by itself
constexpr int OCT_MAX_J = 21;
constexpr int OCT_HIST_GRID = 512;

struct OctCounts { int64_t n[OCT_MAX_J + 1]; };

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

// ---- counts ------------------------------------------------------------------------------------------------------------------
// hist[c], c < J: rows that share exactly c leading digits with their predecessor (row 0: c = 0); hist[31] != 0: bad input
__global__ __launch_bounds__(OCT_THREADS) void oct_counts_kernel(const uint64_t *__restrict__ keys, int64_t n, int J,
                                                                 uint32_t *__restrict__ hist)
{
    __shared__ uint32_t bins[32];
    const int lane = threadIdx.x & 63;
    if (threadIdx.x < 32) bins[threadIdx.x] = 0;
    __syncthreads();
    uint32_t acc = 0, err = 0;
    for (int64_t i0 = (int64_t)blockIdx.x * OCT_THREADS; i0 < n; i0 += (int64_t)gridDim.x * OCT_THREADS) {
        const int64_t i = i0 + threadIdx.x;
        const bool valid = i < n;
        const uint64_t x = valid ? keys[i] : 0ull;
        int c = valid ? 0 : 32;
        if (valid && i > 0) {
            const uint64_t p = keys[i - 1];
            if (x <= p) {
                err = 1;
            } else {
                const int digit = (63 - __clzll((long long)(x ^ p))) / 3;     // coarsest digit that differs
                c = J - 1 - digit;
                if (c < 0) c = 0;                                            // (out of range: flagged below)
            }
        }
        if (valid && (x >> (3 * J)) != 0ull) err = 1;
        for (int b = 0; b < J; ++b) {
            const uint32_t m = (uint32_t)__popcll(__ballot(c == b));
            acc += (lane == b) ? m : 0u;
        }
    }
    if (lane < J && acc) atomicAdd(&bins[lane], acc);
    if (err) atomicOr(&bins[31], 1u);
    __syncthreads();
    if (threadIdx.x < 32 && bins[threadIdx.x]) atomicAdd(&hist[threadIdx.x], bins[threadIdx.x]);
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

__global__ __launch_bounds__(OCT_THREADS) void oct_head_count_kernel(const uint64_t *__restrict__ cur, int64_t n, int64_t nchunks,
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

__global__ __launch_bounds__(OCT_THREADS) void oct_level_up_kernel(const uint64_t *__restrict__ cur, int64_t n, int64_t nchunks,
                                                                   const uint32_t *__restrict__ blk, int scanned,
                                                                   uint64_t *__restrict__ parent, uint8_t *__restrict__ occ,
                                                                   int64_t n_parent)
{
    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) oct_up_chunk(cur, n, c, oct_before(blk, c, scanned), parent, occ, n_parent);
}

// the coarse levels: steps g = g_first, g_first - 1, ... 0 (each reads level g + 1, at most one chunk) in one workgroup
__global__ __launch_bounds__(OCT_THREADS) void oct_top_up_kernel(const uint64_t *src, uint64_t *a, uint64_t *b, int g_first,
                                                                 const OctCounts cn, uint8_t *occ)
{
    int64_t off = 0;
    for (int g = 0; g < g_first; ++g) off += cn.n[g];
    const uint64_t *cur = src;
    uint64_t *dst = a, *other = b;
    for (int g = g_first; g >= 0; --g) {
        oct_up_chunk(cur, cn.n[g + 1], 0, 0u, dst, occ + off, cn.n[g]);
        __syncthreads();                                 // this level's parent keys are the next step's input
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

__global__ __launch_bounds__(OCT_THREADS) void oct_pop_count_kernel(const uint8_t *__restrict__ occ, int64_t n, int64_t nchunks,
                                                                    uint32_t *__restrict__ blk)
{
    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        uint32_t o[OCT_ITEMS], tot;
        (void)oct_block_scan(oct_load_bytes(occ, n, c * OCT_CHUNK + (int64_t)threadIdx.x * OCT_ITEMS, o), &tot);
        if (threadIdx.x == 0) blk[c] = tot;
    }
}

__global__ __launch_bounds__(OCT_THREADS) void oct_level_down_kernel(const uint64_t *__restrict__ parent, const uint8_t *__restrict__ occ,
                                                                     int64_t n, int64_t nchunks, const uint32_t *__restrict__ blk,
                                                                     int scanned, uint64_t *__restrict__ child, int64_t n_child,
                                                                     int32_t *bad)
{
    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x)
        oct_down_chunk(parent, occ, n, c, nchunks, oct_before(blk, c, scanned), child, n_child, bad);
}

// steps g = 0 .. g_end - 1 (each at most one chunk of parents) in one workgroup; step g writes into (g & 1) ? b : a
__global__ __launch_bounds__(OCT_THREADS) void oct_top_down_kernel(const uint8_t *occ, int g_end, const OctCounts cn, uint64_t *a,
                                                                   uint64_t *b, int32_t *bad)
{
    int64_t off = 0;
    const uint64_t *cur = nullptr;
    for (int g = 0; g < g_end; ++g) {
        uint64_t *dst = (g & 1) ? b : a;
        oct_down_chunk(cur, occ + off, cn.n[g], 0, 1, 0u, dst, cn.n[g + 1], bad);
        __syncthreads();
        cur = dst;
        off += cn.n[g];
    }
}

// ---- byte <-> rank -----------------------------------------------------------------------------------------------------------
// VEC: occ is 4-byte aligned (and the symbols 16-byte aligned): 4 nodes per thread and step; the n % 4 last ones one by one
template <bool VEC>
__global__ __launch_bounds__(OCT_THREADS) void oct_hist_kernel(const uint8_t *__restrict__ occ, int64_t n, uint32_t *__restrict__ hist)
{
    __shared__ uint32_t bins[OCT_THREADS / RAHT_WAVE][256];
    uint32_t *mine = bins[threadIdx.x >> 6];
    for (int t = threadIdx.x; t < (OCT_THREADS / RAHT_WAVE) * 256; t += OCT_THREADS) (&bins[0][0])[t] = 0;
    __syncthreads();
    const int64_t gtid = (int64_t)blockIdx.x * OCT_THREADS + threadIdx.x, gsz = (int64_t)gridDim.x * OCT_THREADS;
    const int64_t nq = VEC ? n / 4 : 0;
    if (VEC) {
        const uint32_t *w = (const uint32_t *)occ;
        for (int64_t j = gtid; j < nq; j += gsz) {
            const uint32_t q = w[j];
            atomicAdd(&mine[q & 255u], 1u);
            atomicAdd(&mine[(q >> 8) & 255u], 1u);
            atomicAdd(&mine[(q >> 16) & 255u], 1u);
            atomicAdd(&mine[q >> 24], 1u);
        }
    }
    for (int64_t j = 4 * nq + gtid; j < n; j += gsz) atomicAdd(&mine[occ[j]], 1u);
    __syncthreads();
    for (int t = threadIdx.x; t < 256; t += OCT_THREADS) {
        uint32_t s = 0;
#pragma unroll
        for (int w = 0; w < OCT_THREADS / RAHT_WAVE; ++w) s += bins[w][t];
        if (s) atomicAdd(&hist[t], s);
    }
}

// tab[0..255] = rank of every byte, tab[256..511] = byte of every rank: descending count, ties by ascending byte value
__global__ __launch_bounds__(OCT_THREADS) void oct_rank_kernel(const uint32_t *__restrict__ hist, uint8_t *__restrict__ tab)
{
    __shared__ uint32_t cnt[256];
    const uint32_t b = threadIdx.x;
    cnt[b] = hist[b];
    __syncthreads();
    const uint32_t mine = cnt[b];
    uint32_t r = 0;
    for (uint32_t o = 0; o < 256; ++o) r += (cnt[o] > mine || (cnt[o] == mine && o < b)) ? 1u : 0u;
    tab[b] = (uint8_t)r;
    tab[256 + r] = (uint8_t)b;
}

template <bool VEC>
__global__ __launch_bounds__(OCT_THREADS) void oct_symbols_kernel(const uint8_t *__restrict__ occ, int64_t n, const uint8_t *__restrict__ tab,
                                                                  int32_t *__restrict__ sym)
{
    __shared__ uint8_t rank_of[256];
    rank_of[threadIdx.x] = tab[threadIdx.x];
    __syncthreads();
    const int64_t gtid = (int64_t)blockIdx.x * OCT_THREADS + threadIdx.x, gsz = (int64_t)gridDim.x * OCT_THREADS;
    const int64_t nq = VEC ? n / 4 : 0;
    if (VEC) {
        const uint32_t *w = (const uint32_t *)occ;
        int4 *o = (int4 *)sym;
        for (int64_t j = gtid; j < nq; j += gsz) {
            const uint32_t q = w[j];
            o[j] = make_int4(rank_of[q & 255u], rank_of[(q >> 8) & 255u], rank_of[(q >> 16) & 255u], rank_of[q >> 24]);
        }
    }
    for (int64_t j = 4 * nq + gtid; j < n; j += gsz) sym[j] = rank_of[occ[j]];
}

struct OctTable { uint8_t byte_of[256]; uint32_t used; };

template <bool VEC>
__global__ __launch_bounds__(OCT_THREADS) void oct_bytes_kernel(const int32_t *__restrict__ sym, int64_t n, const OctTable tb,
                                                                uint8_t *__restrict__ occ, int32_t *bad)
{
    __shared__ uint8_t byte_of[256];
    byte_of[threadIdx.x] = tb.byte_of[threadIdx.x];
    __syncthreads();
    const int64_t gtid = (int64_t)blockIdx.x * OCT_THREADS + threadIdx.x, gsz = (int64_t)gridDim.x * OCT_THREADS;
    const int64_t nq = VEC ? n / 4 : 0;
    bool wrong = false;
    if (VEC) {
        const int4 *q = (const int4 *)sym;
        uint32_t *o = (uint32_t *)occ;
        for (int64_t j = gtid; j < nq; j += gsz) {
            const int4 s = q[j];
            const uint32_t v[4] = {(uint32_t)s.x, (uint32_t)s.y, (uint32_t)s.z, (uint32_t)s.w};
            uint32_t out = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool ok = v[k] < tb.used;
                wrong |= !ok;
                out |= (ok ? (uint32_t)byte_of[v[k]] : 0u) << (8 * k);
            }
            o[j] = out;
        }
    }
    for (int64_t j = 4 * nq + gtid; j < n; j += gsz) {
        const uint32_t v = (uint32_t)sym[j];
        const bool ok = v < tb.used;
        wrong |= !ok;
        occ[j] = ok ? byte_of[v] : (uint8_t)0;
    }
    if (wrong) *bad = 1;
}

// ---- keys -> coordinates -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(OCT_THREADS) void oct_demorton_kernel(const uint64_t *__restrict__ keys, int64_t n, uint64_t mask,
                                                                   int64_t *__restrict__ V)
{
    for (int64_t i = (int64_t)blockIdx.x * OCT_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * OCT_THREADS) {
        const uint64_t k = keys[i] & mask;
        V[3 * i + 0] = (int64_t)vx_compact3(k >> 2);
        V[3 * i + 1] = (int64_t)vx_compact3(k >> 1);
        V[3 * i + 2] = (int64_t)vx_compact3(k);
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------
static inline unsigned oct_grid(int64_t items, int64_t per_block, int cap = OCT_MAX_GRID)
{
    const int64_t g = ceil_div(items, per_block);
    return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

// the plausibility rules of a count list (the header of a geometry section comes off the wire)
static int oct_check_counts(const char *what, const int64_t *counts, int J, int64_t *n_nodes)
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

static void oct_fill(OctCounts &cn, const int64_t *counts, int J)
{
    for (int g = 0; g <= OCT_MAX_J; ++g) cn.n[g] = g <= J ? counts[g] : 0;
}

}  // namespace raht

using namespace raht;

extern "C" {

int raht_octree_counts(const uint64_t *keys_sorted, int64_t N, int J, int64_t *counts, raht_stream_t stream)
{
    if (!keys_sorted || !counts) { set_error("raht_octree_counts: NULL argument"); return RAHT_ERR_INVALID; }
    if (N < 1 || N >= ((int64_t)1 << 31)) { set_error("raht_octree_counts: N must be 1 .. 2^31 - 1"); return RAHT_ERR_INVALID; }
    if (J < 1 || J > OCT_MAX_J) { set_error("raht_octree_counts: J must be 1 .. 21"); return RAHT_ERR_INVALID; }
    hipStream_t s = (hipStream_t)stream;
    return guarded("raht_octree_counts", [&]() -> int {
        Scratch hist(sizeof(uint32_t) * 32, s);
        if (!hist.ok()) { set_error("raht_octree_counts: out of device memory"); return RAHT_ERR_NOMEM; }
        RAHT_HIP_CHECK(hipMemsetAsync(hist.ptr(), 0, sizeof(uint32_t) * 32, s));
        hipLaunchKernelGGL(oct_counts_kernel, dim3(oct_grid(N, OCT_THREADS * 4)), dim3(OCT_THREADS), 0, s, keys_sorted, N, J,
                           hist.as<uint32_t>());
        RAHT_HIP_CHECK(hipGetLastError());
        uint32_t h[32];
        RAHT_RET(read_back_u32(h, hist.as<uint32_t>(), 32, nullptr, nullptr, 0, s));
        if (h[31]) {
            set_error("raht_octree_counts: the keys are not strictly ascending or not below 8^J");
            return RAHT_ERR_INVALID;
        }
        counts[0] = 1;
        for (int g = 1; g <= J; ++g) counts[g] = (g == 1 ? 0 : counts[g - 1]) + (int64_t)h[g - 1];
        return RAHT_OK;
    });
}

int raht_octree_encode(const uint64_t *keys_sorted, int64_t N, int J, const int64_t *counts, uint8_t *occ, raht_stream_t stream)
{
    if (!keys_sorted || !occ) { set_error("raht_octree_encode: NULL argument"); return RAHT_ERR_INVALID; }
    if (N < 1 || N >= ((int64_t)1 << 31)) { set_error("raht_octree_encode: N must be 1 .. 2^31 - 1"); return RAHT_ERR_INVALID; }
    int64_t n_nodes = 0;
    RAHT_RET(oct_check_counts("raht_octree_encode", counts, J, &n_nodes));
    if (counts[J] != N) { set_error("raht_octree_encode: counts[J] must be N"); return RAHT_ERR_INVALID; }
    hipStream_t s = (hipStream_t)stream;
    return guarded("raht_octree_encode", [&]() -> int {
        Scratch ka(sizeof(uint64_t) * (size_t)counts[J - 1], s), kb(sizeof(uint64_t) * (size_t)(J > 1 ? counts[J - 2] : 1), s);
        Scratch blk(sizeof(uint32_t) * (size_t)ceil_div(N, OCT_CHUNK), s);
        if (!ka.ok() || !kb.ok() || !blk.ok()) { set_error("raht_octree_encode: out of device memory"); return RAHT_ERR_NOMEM; }
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
            src = bufs[w];
            w ^= 1;
        }
        if (g >= 0)
            hipLaunchKernelGGL(oct_top_up_kernel, dim3(1), dim3(OCT_THREADS), 0, s, src, bufs[w], bufs[w ^ 1], g, cn, occ);
        RAHT_HIP_CHECK(hipGetLastError());
        return RAHT_OK;
    });
}

int raht_octree_decode(const uint8_t *occ, const int64_t *counts, int J, uint64_t *keys, int32_t *bad, raht_stream_t stream)
{
    if (!occ || !keys || !bad) { set_error("raht_octree_decode: NULL argument"); return RAHT_ERR_INVALID; }
    int64_t n_nodes = 0;
    RAHT_RET(oct_check_counts("raht_octree_decode", counts, J, &n_nodes));
    hipStream_t s = (hipStream_t)stream;
    return guarded("raht_octree_decode", [&]() -> int {
        const int64_t N = counts[J];
        Scratch tmp(sizeof(uint64_t) * (size_t)counts[J - 1], s);
        Scratch blk(sizeof(uint32_t) * (size_t)ceil_div(N, OCT_CHUNK), s);
        if (!tmp.ok() || !blk.ok()) { set_error("raht_octree_decode: out of device memory"); return RAHT_ERR_NOMEM; }
        OctCounts cn;
        oct_fill(cn, counts, J);
        // step g writes level g + 1; the last step (g = J - 1) writes `keys`, the steps before it alternate
        uint64_t *even = ((J - 1) & 1) ? tmp.as<uint64_t>() : keys, *odd = ((J - 1) & 1) ? keys : tmp.as<uint64_t>();
        int g_end = 1;
        while (g_end < J && counts[g_end] <= OCT_CHUNK) ++g_end;
        hipLaunchKernelGGL(oct_top_down_kernel, dim3(1), dim3(OCT_THREADS), 0, s, occ, g_end, cn, even, odd, bad);
        int64_t off = 0;
        for (int g = 0; g < g_end; ++g) off += counts[g];
        for (int g = g_end; g < J; ++g) {
            const int64_t n = counts[g], nchunks = ceil_div(n, OCT_CHUNK);
            const int scanned = nchunks > OCT_SELF_PREFIX;
            const uint64_t *parent = ((g - 1) & 1) ? odd : even;
            uint64_t *child = (g & 1) ? odd : even;
            hipLaunchKernelGGL(oct_pop_count_kernel, dim3(oct_grid(nchunks, 1)), dim3(OCT_THREADS), 0, s, occ + off, n, nchunks,
                               blk.as<uint32_t>());
            if (scanned) RAHT_RET(exclusive_scan_u32(blk.as<uint32_t>(), blk.as<uint32_t>(), nchunks, nullptr, s));
            hipLaunchKernelGGL(oct_level_down_kernel, dim3(oct_grid(nchunks, 1)), dim3(OCT_THREADS), 0, s, parent, occ + off, n, nchunks,
                               (const uint32_t *)blk.as<uint32_t>(), scanned, child, counts[g + 1], bad);
            off += n;
        }
        RAHT_HIP_CHECK(hipGetLastError());
        return RAHT_OK;
    });
}

int raht_octree_symbols(const uint8_t *occ, int64_t n_nodes, uint8_t *byte_of_rank, int32_t *sym, raht_stream_t stream)
{
    if (!occ || !byte_of_rank || !sym) { set_error("raht_octree_symbols: NULL argument"); return RAHT_ERR_INVALID; }
    if (n_nodes < 1 || n_nodes >= ((int64_t)1 << 31)) { set_error("raht_octree_symbols: n_nodes must be 1 .. 2^31 - 1"); return RAHT_ERR_INVALID; }
    if ((uintptr_t)sym & 3) { set_error("raht_octree_symbols: sym must be 4-byte aligned"); return RAHT_ERR_INVALID; }
    hipStream_t s = (hipStream_t)stream;
    return guarded("raht_octree_symbols", [&]() -> int {
        Scratch ws(sizeof(uint32_t) * 256 + 512, s);
        if (!ws.ok()) { set_error("raht_octree_symbols: out of device memory"); return RAHT_ERR_NOMEM; }
        uint32_t *hist = ws.as<uint32_t>();
        uint8_t *tab = (uint8_t *)(hist + 256);
        const bool vec = (((uintptr_t)occ & 3) | ((uintptr_t)sym & 15)) == 0;
        RAHT_HIP_CHECK(hipMemsetAsync(hist, 0, sizeof(uint32_t) * 256, s));
        const dim3 gh(oct_grid(n_nodes, OCT_THREADS * 16, OCT_HIST_GRID)), gm(oct_grid(n_nodes, OCT_THREADS * 4)), blk(OCT_THREADS);
        if (vec) hipLaunchKernelGGL(oct_hist_kernel<true>, gh, blk, 0, s, occ, n_nodes, hist);
        else hipLaunchKernelGGL(oct_hist_kernel<false>, gh, blk, 0, s, occ, n_nodes, hist);
        hipLaunchKernelGGL(oct_rank_kernel, dim3(1), blk, 0, s, (const uint32_t *)hist, tab);
        if (vec) hipLaunchKernelGGL(oct_symbols_kernel<true>, gm, blk, 0, s, occ, n_nodes, (const uint8_t *)tab, sym);
        else hipLaunchKernelGGL(oct_symbols_kernel<false>, gm, blk, 0, s, occ, n_nodes, (const uint8_t *)tab, sym);
        RAHT_HIP_CHECK(hipGetLastError());
        uint32_t back[64];
        RAHT_RET(read_back_u32(back, (const uint32_t *)(tab + 256), 64, nullptr, nullptr, 0, s));
        memcpy(byte_of_rank, back, 256);
        return RAHT_OK;
    });
}

int raht_octree_bytes(const int32_t *sym, int64_t n_nodes, const uint8_t *byte_of_rank, uint8_t *occ, int32_t *bad, raht_stream_t stream)
{
    if (!sym || !byte_of_rank || !occ || !bad) { set_error("raht_octree_bytes: NULL argument"); return RAHT_ERR_INVALID; }
    if (n_nodes < 1 || n_nodes >= ((int64_t)1 << 31)) { set_error("raht_octree_bytes: n_nodes must be 1 .. 2^31 - 1"); return RAHT_ERR_INVALID; }
    if ((uintptr_t)sym & 3) { set_error("raht_octree_bytes: sym must be 4-byte aligned"); return RAHT_ERR_INVALID; }
    OctTable tb;
    bool seen[256] = {};
    tb.used = 256;
    for (int r = 0; r < 256; ++r) {
        const uint8_t b = byte_of_rank[r];
        if (seen[b]) { set_error("raht_octree_bytes: byte_of_rank is not a permutation of 0 .. 255"); return RAHT_ERR_INVALID; }
        seen[b] = true;
        tb.byte_of[r] = b;
        if (b == 0) tb.used = (uint32_t)r;       // no node has an empty occupancy byte: byte 0 leads the unused ranks
    }
    hipStream_t s = (hipStream_t)stream;
    const bool vec = (((uintptr_t)occ & 3) | ((uintptr_t)sym & 15)) == 0;
    const dim3 gm(oct_grid(n_nodes, OCT_THREADS * 4)), blk(OCT_THREADS);
    if (vec) hipLaunchKernelGGL(oct_bytes_kernel<true>, gm, blk, 0, s, sym, n_nodes, tb, occ, bad);
    else hipLaunchKernelGGL(oct_bytes_kernel<false>, gm, blk, 0, s, sym, n_nodes, tb, occ, bad);
    RAHT_HIP_CHECK(hipGetLastError());
    return RAHT_OK;
}

int raht_demorton(const uint64_t *keys, int64_t N, int J, int64_t *V, raht_stream_t stream)
{
    if (N < 0 || J < 1 || J > OCT_MAX_J) { set_error("raht_demorton: bad argument"); return RAHT_ERR_INVALID; }
    if (N == 0) return RAHT_OK;
    if (!keys || !V) { set_error("raht_demorton: NULL argument"); return RAHT_ERR_INVALID; }
    hipLaunchKernelGGL(oct_demorton_kernel, dim3(oct_grid(N, OCT_THREADS)), dim3(OCT_THREADS), 0, (hipStream_t)stream, keys, N,
                       (~0ull) >> (64 - 3 * J), V);
    RAHT_HIP_CHECK(hipGetLastError());
    return RAHT_OK;
}

}  // extern "C"
