// predict_bi.hip -- the two-reference inter-frame predictor of a sequence's B frames (include/raht.h, "Two references").
// Row i has a run in each of two references, resolved as raht_predict / raht_predict_mc resolve it (its own key, or the key shifted
// by the vector of the row's block in that reference's motion field); m0, m1 are the means of the two runs with pr_mean's bits. The
// prediction is the mean of the reference that has a run where only one has, +0 where neither has, and fl(0.5 fl(m0 + m1)) where
// both have: two rounded operations, never contracted with the X - P or X + P behind them.
//
//   one launch, PR_TILE_ROWS rows per workgroup step (predict_device.h's kernel with a second reference):
//     resolve   one thread per row finds both runs; (lo0, len0, lo1, len1) go to LDS as one 16-byte entry (4 KB a workgroup); the
//               rows with a run in reference 0, in reference 1 and in both are counted.
//     move      the tile's elements flat in 16-byte chunks where no matrix is padded, X and Y nontemporal, both references through
//               the cache, two chunks per lane and round with their X loads issued before the runs are walked; padded matrices
//               and chunks that straddle rows move element by element. X and Y may be the same matrix: a lane reads only what it
//               writes.
//   raht_predict_bi_modes   the same launch under a mode per block of the frame (include/raht.h, "Block modes"): the
//     resolve step reads the mode of the row's block and leaves the run of a reference the mode does not use empty -- what the move
//     step does with an empty run is the rule above, so mode 0 has raht_predict_bi's bits, modes 1 and 2 the one-reference
//     predictors', and mode 3 predicts +0. The counters count the runs that are used.
#include "predict_device.h"

namespace raht {

// The predictors a row may use. AllRefs: both references (raht_predict_bi).
struct AllRefs {
    __device__ __forceinline__ void operator()(int64_t, bool &use0, bool &use1) const { use0 = use1 = true; }
};

// BlockModes: by the mode of the row's block (raht_predict_bi_modes) -- 0: both, 1: reference 0 only, 2: reference 1 only, 3 and
// above: neither. A reference that is not used is not resolved: its run stays empty, and pr_bi gives the other mean, or +0.
struct BlockModes {
    const int64_t *block_first;
    int64_t n_blocks;
    const uint8_t *mode;
    __device__ __forceinline__ void operator()(int64_t row, bool &use0, bool &use1) const
    {
        const uint8_t m = mode[pr_block_of(block_first, n_blocks, row)];
        use0 = m == 0 || m == 1;
        use1 = m == 0 || m == 2;
    }
};

// the prediction of channel ch of a row whose runs are r = (lo0, len0, lo1, len1)
__device__ __forceinline__ float pr_bi_mean(const PrRef &r0, const PrRef &r1, const int4 &r, int ch)
{
    return pr_bi(pr_mean(r0.C, r0.ld, r.x, r.y, ch), r.y, pr_mean(r1.C, r1.ld, r.z, r.w, ch), r.w);
}

// the 16-byte chunk of a flat tile that starts at element e: four predictions applied to x
template <int MODE>
__device__ __forceinline__ RegChunk<float> pr_bi_chunk(const PrRef &r0, const PrRef &r1, const int4 *runs, uint32_t e, uint32_t D,
                                                       const RegChunk<float> &x)
{
    uint32_t j = e / D, ch = e - j * D;
    RegChunk<float> y;
    if (ch + 4 <= D) {                                   // the chunk lies in one row: both runs in 16-byte loads
        const int4 r = runs[j];
        const RegChunk<float> m0 = pr_chunk_mean(r0.C, r0.ld, r.x, r.y, ch);
        const RegChunk<float> m1 = pr_chunk_mean(r1.C, r1.ld, r.z, r.w, ch);
#pragma unroll
        for (int i = 0; i < 4; ++i) y.v[i] = pr_apply<MODE>(x.v[i], pr_bi(m0.v[i], r.y, m1.v[i], r.w));
    } else {                                             // the chunk straddles rows (as many as four when D = 1)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            y.v[i] = pr_apply<MODE>(x.v[i], pr_bi_mean(r0, r1, runs[j], (int)ch));
            if (++ch == D) { ch = 0; ++j; }
        }
    }
    return y;
}

// MODE, FLAT: as predict_kernel's. KEY0 / KEY1: the key a row is resolved for in reference 0 / 1 (SameKey or MvKey).
// USE: the references a row's prediction may use (AllRefs or BlockModes).
// n_matched: three counters -- rows whose prediction uses a run of reference 0, of reference 1, of both.
template <int MODE, bool FLAT, typename KEY0, typename KEY1, typename USE>
__global__ __launch_bounds__(PR_THREADS) void predict_bi_kernel(const uint64_t *__restrict__ keys, int64_t n, const PrRef r0, const PrRef r1,
                                                                int shift, const float *X, int64_t ldx, int D, float *Y, int64_t ldy,
                                                                unsigned long long *__restrict__ n_matched, const KEY0 key0, const KEY1 key1,
                                                                const USE use)
{
    __shared__ int4 runs[PR_TILE_ROWS];
    __shared__ uint32_t hits[3];
    if (threadIdx.x < 3) hits[threadIdx.x] = 0;
    uint32_t mine0 = 0, mine1 = 0, both = 0;
    const int64_t n_tiles = (n + PR_TILE_ROWS - 1) / PR_TILE_ROWS;
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int64_t r0w = t * PR_TILE_ROWS;
        const int rows = (int)min((int64_t)PR_TILE_ROWS, n - r0w);
        __syncthreads();                                 // the previous step's readers are done with the runs
        if ((int)threadIdx.x < rows) {
            const int64_t row = r0w + threadIdx.x;
            const uint64_t own = keys[row];
            uint64_t key;
            int4 r = make_int4(0, 0, 0, 0);
            bool use0, use1;
            use(row, use0, use1);
            if (use0 && key0(row, own, key)) r.y = pr_resolve(r0.keys, r0.n, shift, key, r.x);
            if (use1 && key1(row, own, key)) r.w = pr_resolve(r1.keys, r1.n, shift, key, r.z);
            runs[threadIdx.x] = r;
            mine0 += r.y > 0;
            mine1 += r.w > 0;
            both += r.y > 0 && r.w > 0;
        }
        __syncthreads();
        const uint32_t n_el = (uint32_t)rows * (uint32_t)D;
        if constexpr (FLAT) {
            const float *xt = MODE ? X + r0w * D : nullptr;
            float *yt = Y + r0w * D;
            const uint32_t n_chunks = n_el >> 2;
            // two chunks per round, their loads of X first: 32 bytes of X in flight while the runs are walked
            for (uint32_t q = threadIdx.x; q < n_chunks; q += 2 * PR_THREADS) {
                const uint32_t e0 = q << 2, e1 = (q + PR_THREADS) << 2;
                const bool two = q + PR_THREADS < n_chunks;
                RegChunk<float> x0 = {}, x1 = {};
                if constexpr (MODE != 0) {
                    x0 = ld_chunk<float, true>(xt + e0);
                    if (two) x1 = ld_chunk<float, true>(xt + e1);
                }
                const RegChunk<float> y0 = pr_bi_chunk<MODE>(r0, r1, runs, e0, (uint32_t)D, x0);
                if (two) {
                    const RegChunk<float> y1 = pr_bi_chunk<MODE>(r0, r1, runs, e1, (uint32_t)D, x1);
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
                yt[e] = pr_apply<MODE>(MODE ? xt[e] : 0.0f, pr_bi_mean(r0, r1, runs[j], (int)ch));
            }
        } else {
            for (int64_t e = threadIdx.x; e < (int64_t)rows * D; e += PR_THREADS) {      // (also the home of D >= 2^22: 64-bit indices)
                const int64_t j = e / D, ch = e - j * D;
                const float x = MODE ? X[(r0w + j) * ldx + ch] : 0.0f;
                Y[(r0w + j) * ldy + ch] = pr_apply<MODE>(x, pr_bi_mean(r0, r1, runs[j], (int)ch));
            }
        }
    }
    if (n_matched) {                                     // integer sums: whatever the order, the same numbers
        if (mine0) atomicAdd(&hits[0], mine0);
        if (mine1) atomicAdd(&hits[1], mine1);
        if (both) atomicAdd(&hits[2], both);
        __syncthreads();
        if (threadIdx.x < 3 && hits[threadIdx.x]) atomicAdd(n_matched + threadIdx.x, (unsigned long long)hits[threadIdx.x]);
    }
}

struct BiLaunch {
    unsigned grid;
    bool flat;
    hipStream_t s;
    const uint64_t *keys;
    int64_t N;
    PrRef r0, r1;
    int shift;
    const float *X;
    int64_t ldx;
    int D, add;
    float *Y;
    int64_t ldy;
    unsigned long long *n_matched;
};

template <int MODE, bool FLAT, typename KEY0, typename KEY1, typename USE>
static void predict_bi_launch(const BiLaunch &a, const KEY0 &key0, const KEY1 &key1, const USE &use)
{
    hipLaunchKernelGGL((predict_bi_kernel<MODE, FLAT, KEY0, KEY1, USE>), dim3(a.grid), dim3(PR_THREADS), 0, a.s, a.keys, a.N, a.r0, a.r1,
                       a.shift, a.X, a.ldx, a.D, a.Y, a.ldy, a.n_matched, key0, key1, use);
}

// the kernel of a call's use (P, X - P, X + P) and layout, for the key functors of its two references
template <typename KEY0, typename KEY1, typename USE>
static void predict_bi_uses(const BiLaunch &a, const KEY0 &key0, const KEY1 &key1, const USE &use)
{
    const int mode = !a.X ? 0 : (a.add ? 2 : 1);
    if (a.flat) {
        if (mode == 0) predict_bi_launch<0, true>(a, key0, key1, use);
        else if (mode == 1) predict_bi_launch<1, true>(a, key0, key1, use);
        else predict_bi_launch<2, true>(a, key0, key1, use);
    } else {
        if (mode == 0) predict_bi_launch<0, false>(a, key0, key1, use);
        else if (mode == 1) predict_bi_launch<1, false>(a, key0, key1, use);
        else predict_bi_launch<2, false>(a, key0, key1, use);
    }
}

// both entry points, checked: the memset of the counters and the one launch
template <typename USE>
static int predict_bi_enqueue(const uint64_t *keys_sorted, int64_t N, int J, const int64_t *block_first, int64_t n_blocks, const int8_t *mv0,
                              const int8_t *mv1, const PrRef &r0, const PrRef &r1, int shift, const float *X, int64_t ldx, int D, int add,
                              float *Y, int64_t ldy, int64_t *n_matched, const USE &use, hipStream_t s)
{
    if (n_matched) RAHT_HIP_CHECK(hipMemsetAsync(n_matched, 0, 3 * sizeof(int64_t), s));
    const int64_t tiles = ceil_div(N, PR_TILE_ROWS);
    BiLaunch a;
    a.grid = (unsigned)(tiles > PR_MAX_GRID ? PR_MAX_GRID : tiles);
    a.flat = ldy == D && (!X || ldx == D) && D < (1 << 22);                 // (flat tiles index their elements with 32 bits)
    a.s = s;
    a.keys = keys_sorted;
    a.N = N;
    a.r0 = r0;
    a.r1 = r1;
    a.shift = shift;
    a.X = X;
    a.ldx = ldx;
    a.D = D;
    a.add = add;
    a.Y = Y;
    a.ldy = ldy;
    a.n_matched = (unsigned long long *)n_matched;
    const MvKey f0{block_first, n_blocks, mv0, J}, f1{block_first, n_blocks, mv1, J};
    if (mv0 && mv1) predict_bi_uses(a, f0, f1, use);
    else if (mv0) predict_bi_uses(a, f0, SameKey(), use);
    else if (mv1) predict_bi_uses(a, SameKey(), f1, use);
    else predict_bi_uses(a, SameKey(), SameKey(), use);
    RAHT_HIP_CHECK(hipGetLastError());
    return RAHT_OK;
}

}  // namespace raht

using namespace raht;

extern "C" {

int raht_predict_bi(const uint64_t *keys_sorted, int64_t N, int J, int block_log2, const int64_t *block_first, int64_t n_blocks,
                    const int8_t *mv0, const int8_t *mv1, const uint64_t *ref0_keys_sorted, int64_t N_ref0, const float *C_ref0,
                    int64_t ld_ref0, const uint64_t *ref1_keys_sorted, int64_t N_ref1, const float *C_ref1, int64_t ld_ref1, int shift,
                    const float *X, int64_t ldx, int D, int add, float *Y, int64_t ldy, int64_t *n_matched, raht_stream_t stream)
{
    const char *who = "raht_predict_bi";
    RAHT_RET(predict_check(who, keys_sorted, N, ref0_keys_sorted, N_ref0, shift, C_ref0, ld_ref0, X, ldx, D, add, Y, ldy));
    RAHT_RET(predict_check(who, keys_sorted, N, ref1_keys_sorted, N_ref1, shift, C_ref1, ld_ref1, X, ldx, D, add, Y, ldy));
    if (mv0 || mv1) RAHT_RET(motion_check_blocks(who, J, block_log2, block_first, n_blocks, N));
    return predict_bi_enqueue(keys_sorted, N, J, block_first, n_blocks, mv0, mv1, PrRef{ref0_keys_sorted, (int32_t)N_ref0, C_ref0, ld_ref0},
                              PrRef{ref1_keys_sorted, (int32_t)N_ref1, C_ref1, ld_ref1}, shift, X, ldx, D, add, Y, ldy, n_matched, AllRefs(),
                              (hipStream_t)stream);
}

int raht_predict_bi_modes(const uint64_t *keys_sorted, int64_t N, int J, int block_log2, const int64_t *block_first, int64_t n_blocks,
                          const uint8_t *mode, const int8_t *mv0, const int8_t *mv1, const uint64_t *ref0_keys_sorted, int64_t N_ref0,
                          const float *C_ref0, int64_t ld_ref0, const uint64_t *ref1_keys_sorted, int64_t N_ref1, const float *C_ref1,
                          int64_t ld_ref1, int shift, const float *X, int64_t ldx, int D, int add, float *Y, int64_t ldy, int64_t *n_matched,
                          raht_stream_t stream)
{
    const char *who = "raht_predict_bi_modes";
    if (!mode) { set_error("%s: NULL mode", who); return RAHT_ERR_INVALID; }
    RAHT_RET(predict_check(who, keys_sorted, N, ref0_keys_sorted, N_ref0, shift, C_ref0, ld_ref0, X, ldx, D, add, Y, ldy));
    RAHT_RET(predict_check(who, keys_sorted, N, ref1_keys_sorted, N_ref1, shift, C_ref1, ld_ref1, X, ldx, D, add, Y, ldy));
    RAHT_RET(motion_check_blocks(who, J, block_log2, block_first, n_blocks, N));      // (the modes lie over the blocks, fields or none)
    return predict_bi_enqueue(keys_sorted, N, J, block_first, n_blocks, mv0, mv1, PrRef{ref0_keys_sorted, (int32_t)N_ref0, C_ref0, ld_ref0},
                              PrRef{ref1_keys_sorted, (int32_t)N_ref1, C_ref1, ld_ref1}, shift, X, ldx, D, add, Y, ldy, n_matched,
                              BlockModes{block_first, n_blocks, mode}, (hipStream_t)stream);
}

}  // extern "C"
