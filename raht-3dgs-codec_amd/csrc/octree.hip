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
// The level walks themselves (kernels and host loops) live in octree_device.h: octree_inter.hip runs them too.
#include "octree_device.h"

#include <cstring>

namespace raht {

constexpr int OCT_HIST_GRID = 512;

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
        return oct_encode_levels("raht_octree_encode", keys_sorted, N, J, counts, n_nodes, occ, OctNoHook(), s);
    });
}

int raht_octree_decode(const uint8_t *occ, const int64_t *counts, int J, uint64_t *keys, int32_t *bad, raht_stream_t stream)
{
    if (!occ || !keys || !bad) { set_error("raht_octree_decode: NULL argument"); return RAHT_ERR_INVALID; }
    int64_t n_nodes = 0;
    RAHT_RET(oct_check_counts("raht_octree_decode", counts, J, &n_nodes));
    hipStream_t s = (hipStream_t)stream;
    return guarded("raht_octree_decode", [&]() -> int {
        return oct_decode_levels("raht_octree_decode", occ, counts, J, keys, bad, OctNoHook(), s);
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

// ranks -> bytes under a table from a header; n_used < 0: the ranks in use end where byte 0 stands
static int oct_bytes_run(const char *what, const int32_t *sym, int64_t n_nodes, const uint8_t *byte_of_rank, int n_used, uint8_t *out,
                         int32_t *bad, raht_stream_t stream)
{
    if (!sym || !byte_of_rank || !out || !bad) { set_error("%s: NULL argument", what); return RAHT_ERR_INVALID; }
    if (n_nodes < 1 || n_nodes >= ((int64_t)1 << 31)) { set_error("%s: n_nodes must be 1 .. 2^31 - 1", what); return RAHT_ERR_INVALID; }
    if ((uintptr_t)sym & 3) { set_error("%s: sym must be 4-byte aligned", what); return RAHT_ERR_INVALID; }
    OctTable tb;
    bool seen[256] = {};
    tb.used = 256;
    for (int r = 0; r < 256; ++r) {
        const uint8_t b = byte_of_rank[r];
        if (seen[b]) { set_error("%s: byte_of_rank is not a permutation of 0 .. 255", what); return RAHT_ERR_INVALID; }
        seen[b] = true;
        tb.byte_of[r] = b;
        if (b == 0 && n_used < 0) tb.used = (uint32_t)r;   // no node has an empty occupancy byte: byte 0 leads the unused ranks
    }
    if (n_used >= 0) tb.used = (uint32_t)n_used;
    hipStream_t s = (hipStream_t)stream;
    const bool vec = (((uintptr_t)out & 3) | ((uintptr_t)sym & 15)) == 0;
    const dim3 gm(oct_grid(n_nodes, OCT_THREADS * 4)), blk(OCT_THREADS);
    if (vec) hipLaunchKernelGGL(oct_bytes_kernel<true>, gm, blk, 0, s, sym, n_nodes, tb, out, bad);
    else hipLaunchKernelGGL(oct_bytes_kernel<false>, gm, blk, 0, s, sym, n_nodes, tb, out, bad);
    RAHT_HIP_CHECK(hipGetLastError());
    return RAHT_OK;
}

int raht_octree_bytes(const int32_t *sym, int64_t n_nodes, const uint8_t *byte_of_rank, uint8_t *occ, int32_t *bad, raht_stream_t stream)
{
    return oct_bytes_run("raht_octree_bytes", sym, n_nodes, byte_of_rank, -1, occ, bad, stream);
}

// the residual bytes of a predicted section (octree_inter.hip): byte 0 is an ordinary value there, the header says how many ranks are in use
int raht_octree_bytes_used(const int32_t *sym, int64_t n_nodes, const uint8_t *byte_of_rank, int n_used, uint8_t *res, int32_t *bad,
                           raht_stream_t stream)
{
    if (n_used < 1 || n_used > 256) { set_error("raht_octree_bytes_used: n_used must be 1 .. 256"); return RAHT_ERR_INVALID; }
    return oct_bytes_run("raht_octree_bytes_used", sym, n_nodes, byte_of_rank, n_used, res, bad, stream);
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
