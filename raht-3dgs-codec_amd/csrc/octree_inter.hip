// octree_inter.hip -- the geometry of a frame PREDICTED from a reference frame's (include/raht.h, "Predicted octree geometry"):
// every occupancy byte is XORed with the occupancy byte the reference frame has for the same cell, so a scene that stands
// still codes as zeros. The level walks are the intra coder's (octree_device.h); this file adds the hook that turns a level's
// bytes into residuals (encode) or back (decode), and the search behind it.
//
//   pred     node of level g with cell key c, s = 3 (J - g): the reference's keys of the cell are the rows [lo, hi) with
//            key >> s == c -- two binary searches, the second inside the 8^(J - g) rows a cell can hold at most. Inside them
//            the children are visited in ascending order: the row at `pos` names a child d = (key >> (s - 3)) & 7, and the
//            next child starts at lower_bound((8 c + d + 1) << (s - 3)) in [pos + 1, hi). At most 8 hops; at g = J - 1 the
//            children are the keys themselves and a hop is a step. Everything is unsigned: (c + 1) << s reaches 2^63 at J = 21.
//            One thread per node: the searches are chains of dependent loads, and it is the number of waves in flight that
//            hides them (no LDS, few registers: the grid fills every SIMD's wave slots).
//   top      the coarse levels run in ONE workgroup (oct_top_up_kernel / oct_top_down_kernel), where nothing hides a chain: a
//            node there would cost 2 + 8 searches of ~log2 N_ref loads one after the other (measured on a 1 M voxel frame: the
//            decode stage 0.73 ms that way, 0.37 ms this way). So there eight lanes share a node, one child each --
//            one search of the whole reference per lane, the eight answers ORed with three shuffles -- and a lane runs
//            OCT_TOP_ILP such searches in lockstep (the same step count for all: their loads are in flight together).
//            Neither the keys of a corrupt stream nor reference keys out of order can take a search outside [0, N_ref).
#include "octree_device.h"

namespace raht {

// first row of r[lo, hi) whose key is >= x (hi when there is none)
__device__ __forceinline__ int64_t oct_lower_bound(const uint64_t *__restrict__ r, int64_t lo, int64_t hi, uint64_t x)
{
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (r[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the reference's occupancy byte of the cell c of the level whose cells are 2^s keys wide (s = 3 (J - g), 3 <= s <= 63)
__device__ __forceinline__ uint32_t oct_pred_byte(const uint64_t *__restrict__ r, int64_t n_ref, uint64_t c, int s)
{
    if (s < 63 && (c >> (63 - s)) != 0ull) return 0u;      // (a cell key off a corrupt stream: c << s would leave 63 bits)
    const int64_t lo = oct_lower_bound(r, 0, n_ref, c << s);
    int64_t hi = n_ref;
    if (s < 31 && n_ref - lo > ((int64_t)1 << s)) hi = lo + ((int64_t)1 << s);      // a cell holds 2^s keys at most
    hi = oct_lower_bound(r, lo, hi, (c + 1ull) << s);
    uint32_t byte = 0;
    int64_t pos = lo;
    while (pos < hi) {
        const uint64_t child = r[pos] >> (s - 3);
        if ((child >> 3) != c) break;                       // (reference keys out of order)
        byte |= 1u << (uint32_t)(child & 7ull);
        if ((child & 7ull) == 7ull) break;
        pos = (s == 3) ? pos + 1 : oct_lower_bound(r, pos + 1, hi, (child + 1ull) << (s - 3));
    }
    return byte;
}

constexpr int OCT_TOP_ILP = 4;

// K lower bounds in r[0, n) at once: pos[k] = first row whose key is >= x[k] (n when there is none). Every search takes the same
// steps, whatever it looks for, so the K loads of a step are independent of each other.
template <int K>
__device__ __forceinline__ void oct_lower_bounds(const uint64_t *__restrict__ r, int64_t n, const uint64_t (&x)[K], int64_t (&pos)[K])
{
#pragma unroll
    for (int k = 0; k < K; ++k) pos[k] = 0;
    int64_t len = n;                                       // the answer lies in [pos, pos + len]
    while (len > 1) {
        const int64_t half = len >> 1;
#pragma unroll
        for (int k = 0; k < K; ++k) pos[k] += (r[pos[k] + half - 1] < x[k]) ? half : 0;
        len -= half;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) pos[k] += (r[pos[k]] < x[k]) ? 1 : 0;
}

// the hook of the level walks: out[off + i] = in[off + i] ^ pred(node i of level g)
struct OctPredXor {
    static constexpr bool active = true;
    const uint64_t *ref;
    int64_t n_ref;
    int J;
    const uint8_t *in;
    uint8_t *out;

    __device__ __forceinline__ void level(int g, const uint64_t *node_keys, int64_t n, int64_t off) const
    {
        // item 8 i + d: does the reference hold a key of child d of node i? (the same trips for every lane: the shuffles below)
        constexpr int K = OCT_TOP_ILP;
        const int s = 3 * (J - g);
        for (int64_t base = 0; base < 8 * n; base += K * OCT_THREADS) {
            uint64_t child[K], x[K];
            int64_t pos[K];
            bool ok[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int64_t item = base + k * OCT_THREADS + threadIdx.x, i = item >> 3;
                const uint64_t c = (i < n && node_keys) ? node_keys[i] : 0ull;
                ok[k] = i < n && (s == 63 || (c >> (63 - s)) == 0ull);       // (a cell key off a corrupt stream: no shift leaves 63 bits)
                child[k] = ok[k] ? ((c << 3) | (uint64_t)(item & 7)) : 0ull;
                x[k] = child[k] << (s - 3);
            }
            oct_lower_bounds<K>(ref, n_ref, x, pos);
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int64_t item = base + k * OCT_THREADS + threadIdx.x, i = item >> 3;
                uint32_t bits = (ok[k] && pos[k] < n_ref && (ref[pos[k]] >> (s - 3)) == child[k]) ? 1u << (uint32_t)(item & 7) : 0u;
                bits |= __shfl_xor(bits, 1, RAHT_WAVE);
                bits |= __shfl_xor(bits, 2, RAHT_WAVE);
                bits |= __shfl_xor(bits, 4, RAHT_WAVE);
                if (i < n && (item & 7) == 0) out[off + i] = (uint8_t)(in[off + i] ^ bits);
            }
        }
    }
    int launch(int g, const uint64_t *node_keys, int64_t n, int64_t off, hipStream_t s) const;
};

__global__ __launch_bounds__(OCT_THREADS) void oct_pred_xor_kernel(const uint64_t *__restrict__ node_keys, int64_t n, int s,
                                                                   const uint64_t *__restrict__ ref, int64_t n_ref,
                                                                   const uint8_t *in, uint8_t *out)
{
    for (int64_t i = (int64_t)blockIdx.x * OCT_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * OCT_THREADS)
        out[i] = (uint8_t)(in[i] ^ oct_pred_byte(ref, n_ref, node_keys[i], s));
}

int OctPredXor::launch(int g, const uint64_t *node_keys, int64_t n, int64_t off, hipStream_t s) const
{
    hipLaunchKernelGGL(oct_pred_xor_kernel, dim3(oct_grid(n, OCT_THREADS)), dim3(OCT_THREADS), 0, s, node_keys, n, 3 * (J - g), ref, n_ref,
                       in + off, out + off);
    return RAHT_OK;
}

static int oct_check_ref(const char *what, const uint64_t *ref_keys, int64_t N_ref)
{
    if (!ref_keys) { set_error("%s: NULL ref_keys", what); return RAHT_ERR_INVALID; }
    if (N_ref < 1 || N_ref >= ((int64_t)1 << 31)) { set_error("%s: N_ref must be 1 .. 2^31 - 1", what); return RAHT_ERR_INVALID; }
    return RAHT_OK;
}

}  // namespace raht

using namespace raht;

extern "C" {

int raht_octree_encode_inter(const uint64_t *keys_sorted, int64_t N, int J, const int64_t *counts, const uint64_t *ref_keys,
                             int64_t N_ref, uint8_t *res, raht_stream_t stream)
{
    const char *what = "raht_octree_encode_inter";
    if (!keys_sorted || !res) { set_error("%s: NULL argument", what); return RAHT_ERR_INVALID; }
    if (N < 1 || N >= ((int64_t)1 << 31)) { set_error("%s: N must be 1 .. 2^31 - 1", what); return RAHT_ERR_INVALID; }
    int64_t n_nodes = 0;
    RAHT_RET(oct_check_counts(what, counts, J, &n_nodes));
    if (counts[J] != N) { set_error("%s: counts[J] must be N", what); return RAHT_ERR_INVALID; }
    RAHT_RET(oct_check_ref(what, ref_keys, N_ref));
    hipStream_t s = (hipStream_t)stream;
    return guarded(what, [&]() -> int {
        return oct_encode_levels(what, keys_sorted, N, J, counts, n_nodes, res, OctPredXor{ref_keys, N_ref, J, res, res}, s);
    });
}

int raht_octree_decode_inter(const uint8_t *res, const int64_t *counts, int J, const uint64_t *ref_keys, int64_t N_ref, uint64_t *keys,
                             int32_t *bad, raht_stream_t stream)
{
    const char *what = "raht_octree_decode_inter";
    if (!res || !keys || !bad) { set_error("%s: NULL argument", what); return RAHT_ERR_INVALID; }
    int64_t n_nodes = 0;
    RAHT_RET(oct_check_counts(what, counts, J, &n_nodes));
    RAHT_RET(oct_check_ref(what, ref_keys, N_ref));
    hipStream_t s = (hipStream_t)stream;
    return guarded(what, [&]() -> int {
        Scratch occ((size_t)n_nodes, s);                   // the occupancy stream, rebuilt level by level as the keys come down
        if (!occ.ok()) { set_error("%s: out of device memory", what); return RAHT_ERR_NOMEM; }
        return oct_decode_levels(what, occ.as<uint8_t>(), counts, J, keys, bad, OctPredXor{ref_keys, N_ref, J, res, occ.as<uint8_t>()}, s);
    });
}

}  // extern "C"
