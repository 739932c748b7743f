// region.hip -- where a Morton-prefix region of a frame lies in the frame's coded order (include/raht.h, "Regions of a frame").
// The attribute rows of a frame are coded in order_RAGFT order: a stable sort of the rows by bucket, coarse to fine, row 0 first
// (plan.hip: order_scatter_kernel). The rows [row_lo, row_hi) of a run of octree cells therefore form ONE run of coded rows in
// every bucket finer than the cells, and the numbers that place those runs are three histograms of the rows' buckets:
//
//   layout    one pass over the keys: rows per bucket in the whole frame, before the region and inside it. The wave counts a
//             bucket with a ballot and keeps the count in the lane of that bucket; one LDS atomic per wave and bin at the end of
//             the grid-stride loop, one global atomic per workgroup and non-empty bin. Integer sums: deterministic.
//   cells     the first row of every occupied cell of a depth (flag, the library's scan, scatter): the keys and leaf weights of
//             the plan of the tree above that depth, and the row range of a range of cells.
//   assemble  the region's runs out of the matrix the selected segments decode to, into the region's own coded order.
//
// A SET of row ranges (a region that a motion field has dilated is not one Morton range) has the same three steps in one pass each:
//   layout_set    the 2R ascending bounds cut the rows into 2R + 1 intervals (gap, range, gap, ...). A wave counts the buckets of
//                 the interval it is in with ballots, keeps the counts in its lanes while it stays there, and adds them to the
//                 interval's bins when it leaves; a second launch turns the bins into the table (a prefix sum over the intervals).
//   assemble_set  the run table lies in device memory; a destination row finds its run by binary search over the destinations.
//   needs         the cells of another frame that a prediction of these rows reaches into: flag / scan / scatter of the rows whose
//                 (shifted) cell differs from the row before, and under a motion field a sort and a second pass over that list.
//   needs_bi      the same for the two references of a B frame from ONE pass over the keys: a row's block is found once, both
//                 candidate cells are formed in registers, reference 1's carry a tag bit above the cell bits, and one sort and one
//                 flag / scan / pick serve both lists, split at the tag.
#include "raht_common.h"
#include "predict_device.h"

namespace raht {

constexpr int REG_THREADS = 256;
constexpr int REG_MAX_GRID = 2048;                       // grids are capped and grid-strided
constexpr int REG_BINS = 3 * RAHT_REGION_BUCKETS;
constexpr int REG_TILE_ROWS = 64;                        // destination rows per workgroup step of the assemble kernel

struct RegionRuns { int64_t src[RAHT_REGION_BUCKETS], dst[RAHT_REGION_BUCKETS], count[RAHT_REGION_BUCKETS]; int n; };

// bucket of row i (i >= 1) with predecessor key p: msb(x ^ p) / 3; equal keys (never in a valid frame) count as the finest bucket
__device__ __forceinline__ int region_bucket(uint64_t x, uint64_t p)
{
    const uint64_t d = x ^ p;
    const int b = d ? (63 - __clzll((long long)d)) / 3 : 0;
    return min(b, RAHT_REGION_BUCKETS - 2);
}

__global__ __launch_bounds__(REG_THREADS) void region_layout_kernel(const uint64_t *__restrict__ keys, int64_t n, int64_t row_lo,
                                                                    int64_t row_hi, unsigned long long *__restrict__ table)
{
    __shared__ uint32_t bins[REG_BINS];
    const int lane = threadIdx.x & 63;
    if (threadIdx.x < REG_BINS) bins[threadIdx.x] = 0;
    __syncthreads();
    uint32_t all = 0, before = 0, inside = 0;            // lane b: this wave's rows of bucket b
    for (int64_t i0 = (int64_t)blockIdx.x * REG_THREADS; i0 < n; i0 += (int64_t)gridDim.x * REG_THREADS) {
        const int64_t i = i0 + threadIdx.x;
        int b = -1;
        if (i < n) b = i ? region_bucket(keys[i], keys[i - 1]) : RAHT_REGION_BUCKETS - 1;
        const uint64_t m_lo = __ballot(i < row_lo), m_in = __ballot(i >= row_lo && i < row_hi);
        for (int t = 0; t < RAHT_REGION_BUCKETS; ++t) {
            const uint64_t m = __ballot(b == t);
            if (lane == t) { all += (uint32_t)__popcll(m); before += (uint32_t)__popcll(m & m_lo); inside += (uint32_t)__popcll(m & m_in); }
        }
    }
    if (lane < RAHT_REGION_BUCKETS) {
        if (all) atomicAdd(&bins[lane], all);
        if (before) atomicAdd(&bins[RAHT_REGION_BUCKETS + lane], before);
        if (inside) atomicAdd(&bins[2 * RAHT_REGION_BUCKETS + lane], inside);
    }
    __syncthreads();
    if (threadIdx.x < REG_BINS && bins[threadIdx.x]) atomicAdd(&table[threadIdx.x], (unsigned long long)bins[threadIdx.x]);
}

__global__ __launch_bounds__(REG_THREADS) void region_cell_flag_kernel(const uint64_t *__restrict__ keys, int64_t n, int top_level,
                                                                       uint32_t *__restrict__ flag)
{
    for (int64_t i = (int64_t)blockIdx.x * REG_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * REG_THREADS)
        flag[i] = (i == 0 || ((keys[i] ^ keys[i - 1]) >> top_level) != 0ull) ? 1u : 0u;
}

// every store is bounded by n_cells, whatever the keys hold
__global__ __launch_bounds__(REG_THREADS) void region_cell_scatter_kernel(const uint64_t *__restrict__ keys, int64_t n, int top_level,
                                                                          const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pos,
                                                                          int64_t n_cells, uint64_t *__restrict__ cell_keys,
                                                                          int64_t *__restrict__ cell_first)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) cell_first[n_cells] = n;
    for (int64_t i = (int64_t)blockIdx.x * REG_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * REG_THREADS) {
        if (!flag[i]) continue;
        const int64_t j = (int64_t)pos[i];
        if (j < n_cells) { cell_keys[j] = keys[i] >> top_level; cell_first[j] = i; }
    }
}

// REG_TILE_ROWS destination rows per step: the source row of each (or -1) once into LDS, then the rows' elements flat
__global__ __launch_bounds__(REG_THREADS) void region_assemble_kernel(const int32_t *__restrict__ src, int64_t ld_src,
                                                                      int32_t *__restrict__ dst, int64_t ld_dst, int D, const RegionRuns runs,
                                                                      int64_t n_dst_rows)
{
    __shared__ int64_t from[REG_TILE_ROWS];
    const int64_t n_tiles = (n_dst_rows + REG_TILE_ROWS - 1) / REG_TILE_ROWS;
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int64_t r0 = t * REG_TILE_ROWS;
        const int rows = (int)min((int64_t)REG_TILE_ROWS, n_dst_rows - r0);
        __syncthreads();                                 // the previous step's readers are done with `from`
        if ((int)threadIdx.x < rows) {
            const int64_t r = r0 + threadIdx.x;
            int64_t f = -1;
            for (int k = 0; k < runs.n; ++k)
                if (r >= runs.dst[k] && r < runs.dst[k] + runs.count[k]) f = runs.src[k] + (r - runs.dst[k]);
            from[threadIdx.x] = f;
        }
        __syncthreads();
        for (uint32_t e = threadIdx.x; e < (uint32_t)rows * (uint32_t)D; e += REG_THREADS) {
            const uint32_t j = e / (uint32_t)D, c = e - j * (uint32_t)D;
            const int64_t f = from[j];
            dst[(r0 + j) * ld_dst + c] = f >= 0 ? src[f * ld_src + c] : 0;
        }
    }
}

// the interval of row i among nb ascending bounds: how many bounds are <= i (0 .. nb); odd: inside range (t - 1) / 2
__device__ __forceinline__ int region_interval(const int64_t *bounds, int nb, int64_t i)
{
    int a = 0, b = nb;
    while (a < b) {
        const int m = (a + b) >> 1;
        if (bounds[m] <= i) a = m + 1; else b = m;
    }
    return a;
}

// bins: (nb + 1) x RAHT_REGION_BUCKETS, zeroed by the caller. Whatever the bounds hold, an interval index is 0 .. nb.
__global__ __launch_bounds__(REG_THREADS) void region_layout_set_kernel(const uint64_t *__restrict__ keys, int64_t n,
                                                                        const int64_t *__restrict__ bounds, int nb,
                                                                        unsigned long long *__restrict__ bins)
{
    __shared__ int64_t sb[2 * RAHT_REGION_MAX_RANGES];
    for (int k = threadIdx.x; k < nb; k += REG_THREADS) sb[k] = bounds[k];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    uint32_t acc = 0;                                    // lane b: this wave's rows of bucket b in the interval `cur`
    int cur = -1;
    for (int64_t i0 = (int64_t)blockIdx.x * REG_THREADS; i0 < n; i0 += (int64_t)gridDim.x * REG_THREADS) {
        const int64_t i = i0 + threadIdx.x;
        int b = -1, t = -1;
        if (i < n) {
            b = i ? region_bucket(keys[i], keys[i - 1]) : RAHT_REGION_BUCKETS - 1;
            t = region_interval(sb, nb, i);
        }
        uint64_t todo = __ballot(i < n);
        while (todo) {                                   // one round per interval the wave's 64 rows touch: nearly always one
            const int tt = __shfl(t, __ffsll((unsigned long long)todo) - 1);
            const uint64_t m_t = __ballot(t == tt);
            if (tt != cur) {
                if (cur >= 0 && lane < RAHT_REGION_BUCKETS && acc) atomicAdd(&bins[(int64_t)cur * RAHT_REGION_BUCKETS + lane], (unsigned long long)acc);
                acc = 0;
                cur = tt;
            }
            for (int k = 0; k < RAHT_REGION_BUCKETS; ++k) {
                const uint64_t m = __ballot(b == k);
                if (lane == k) acc += (uint32_t)__popcll(m & m_t);
            }
            todo &= ~m_t;
        }
    }
    if (cur >= 0 && lane < RAHT_REGION_BUCKETS && acc) atomicAdd(&bins[(int64_t)cur * RAHT_REGION_BUCKETS + lane], (unsigned long long)acc);
}

// bins -> table: the whole frame, then per range the rows before it (a running sum over the intervals) and inside it
__global__ void region_layout_set_table_kernel(const unsigned long long *__restrict__ bins, int R, int64_t *__restrict__ table)
{
    const int b = threadIdx.x;
    if (b >= RAHT_REGION_BUCKETS) return;
    int64_t run = 0;
    for (int r = 0; r < R; ++r) {
        run += (int64_t)bins[(int64_t)(2 * r) * RAHT_REGION_BUCKETS + b];
        const int64_t inside = (int64_t)bins[(int64_t)(2 * r + 1) * RAHT_REGION_BUCKETS + b];
        table[(int64_t)(1 + 2 * r) * RAHT_REGION_BUCKETS + b] = run;
        table[(int64_t)(2 + 2 * r) * RAHT_REGION_BUCKETS + b] = inside;
        run += inside;
    }
    table[b] = run + (int64_t)bins[(int64_t)(2 * R) * RAHT_REGION_BUCKETS + b];
}

// region_assemble_kernel with the runs in device memory (3 int64 per run: source row, destination row, count). A destination row
// belongs to the last run that starts at or before it; every source row is clamped into src, so that no table reads outside it.
__global__ __launch_bounds__(REG_THREADS) void region_assemble_set_kernel(const int32_t *__restrict__ src, int64_t ld_src, int64_t n_src_rows,
                                                                          int32_t *__restrict__ dst, int64_t ld_dst, int D,
                                                                          const int64_t *__restrict__ runs, int n_runs, int64_t n_dst_rows)
{
    __shared__ int64_t from[REG_TILE_ROWS];
    const int64_t n_tiles = (n_dst_rows + REG_TILE_ROWS - 1) / REG_TILE_ROWS;
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int64_t r0 = t * REG_TILE_ROWS;
        const int rows = (int)min((int64_t)REG_TILE_ROWS, n_dst_rows - r0);
        __syncthreads();                                 // the previous step's readers are done with `from`
        if ((int)threadIdx.x < rows) {
            const int64_t r = r0 + threadIdx.x;
            int a = 0, b = n_runs;                       // first run whose destination is > r
            while (a < b) {
                const int m = (a + b) >> 1;
                if (runs[3 * (int64_t)m + 1] <= r) a = m + 1; else b = m;
            }
            int64_t f = -1;
            if (a > 0) {
                const int64_t *run = runs + 3 * (int64_t)(a - 1);
                const int64_t off = r - run[1];
                if (off < run[2]) f = max(min(max(run[0], (int64_t)0) + off, n_src_rows - 1), (int64_t)0);      // (max: a sum that wrapped)
            }
            from[threadIdx.x] = f;
        }
        __syncthreads();
        for (uint32_t e = threadIdx.x; e < (uint32_t)rows * (uint32_t)D; e += REG_THREADS) {
            const uint32_t j = e / (uint32_t)D, c = e - j * (uint32_t)D;
            const int64_t f = from[j];
            dst[(r0 + j) * ld_dst + c] = f >= 0 ? src[f * ld_src + c] : 0;
        }
    }
}

constexpr uint64_t NEEDS_NONE = ~0ull;                   // the cell of a row without a match (no cell index has 64 bits)

// the cell a prediction of row i reaches into: the key KEY resolves the row for, cut to its `wide`-bit cell and written as the
// first cell of that group at top_level (wide >= top_level)
template <typename KEY>
__device__ __forceinline__ uint64_t needs_cell(const uint64_t *__restrict__ keys, int64_t i, int top_level, int wide, const KEY &key_of)
{
    uint64_t k;
    if (!key_of(i, keys[i], k)) return NEEDS_NONE;
    return (k >> wide) << (wide - top_level);
}

template <typename KEY>
__global__ __launch_bounds__(REG_THREADS) void region_needs_flag_kernel(const uint64_t *__restrict__ keys, int64_t n, int top_level, int wide,
                                                                        const KEY key_of, uint32_t *__restrict__ flag)
{
    for (int64_t i = (int64_t)blockIdx.x * REG_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * REG_THREADS) {
        const uint64_t c = needs_cell(keys, i, top_level, wide, key_of);
        flag[i] = (c != NEEDS_NONE && (i == 0 || needs_cell(keys, i - 1, top_level, wide, key_of) != c)) ? 1u : 0u;
    }
}

// every store is bounded by cap
template <typename KEY>
__global__ __launch_bounds__(REG_THREADS) void region_needs_scatter_kernel(const uint64_t *__restrict__ keys, int64_t n, int top_level, int wide,
                                                                           const KEY key_of, const uint32_t *__restrict__ flag,
                                                                           const uint32_t *__restrict__ pos, int64_t cap,
                                                                           uint64_t *__restrict__ out)
{
    for (int64_t i = (int64_t)blockIdx.x * REG_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * REG_THREADS) {
        if (!flag[i]) continue;
        const int64_t j = (int64_t)pos[i];
        if (j < cap) out[j] = needs_cell(keys, i, top_level, wide, key_of);
    }
}

// the second pass, over the sorted list: an entry that differs from the one before it
__global__ __launch_bounds__(REG_THREADS) void region_needs_first_kernel(const uint64_t *__restrict__ list, int64_t n, uint32_t *__restrict__ flag)
{
    for (int64_t i = (int64_t)blockIdx.x * REG_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * REG_THREADS)
        flag[i] = (i == 0 || list[i] != list[i - 1]) ? 1u : 0u;
}

__global__ __launch_bounds__(REG_THREADS) void region_needs_pick_kernel(const uint64_t *__restrict__ list, int64_t n, const uint32_t *__restrict__ flag,
                                                                        const uint32_t *__restrict__ pos, int64_t cap, uint64_t *__restrict__ out)
{
    for (int64_t i = (int64_t)blockIdx.x * REG_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * REG_THREADS) {
        if (!flag[i]) continue;
        const int64_t j = (int64_t)pos[i];
        if (j < cap) out[j] = list[i];
    }
}

// ---- the needed sets of a B frame: both references from one pass over the keys (raht_region_needs_bi) ---------------------------
// the cell of the key a row resolves in one reference, under the vector v of its block (NULL: the key itself)
__device__ __forceinline__ uint64_t needs_bi_cell(uint64_t key, const int8_t *__restrict__ v, int J, int top_level, int wide)
{
    uint64_t k = key;
    if (v && !pr_shift_key(vox_coords(key), v[0], v[1], v[2], J, k)) return NEEDS_NONE;
    return (k >> wide) << (wide - top_level);
}

// One pass: the block of a row is found once, its mode byte and both vectors are read once, and both candidate cells are formed in
// registers. cand[i] is the row's cell in reference 0, cand[n + i] its cell in reference 1 with the bit `tag` set (the bit above
// the cell bits), NEEDS_NONE where the mode does not use the reference or the shifted voxel leaves the cube. A candidate is flagged
// unless the row before it IN THE WAVE has the same one: neighbouring repeats go here, the rest after the sort.
__global__ __launch_bounds__(REG_THREADS) void region_needs_bi_kernel(const uint64_t *__restrict__ keys, int64_t n, int J, int top_level, int wide,
                                                                      const int64_t *__restrict__ block_first, int64_t n_blocks,
                                                                      const int8_t *__restrict__ mv0, const int8_t *__restrict__ mv1,
                                                                      const uint8_t *__restrict__ mode, uint64_t tag,
                                                                      uint64_t *__restrict__ cand, uint32_t *__restrict__ flag)
{
    const int lane = threadIdx.x & 63;
    for (int64_t i0 = (int64_t)blockIdx.x * REG_THREADS; i0 < n; i0 += (int64_t)gridDim.x * REG_THREADS) {
        const int64_t i = i0 + threadIdx.x;
        uint64_t c0 = NEEDS_NONE, c1 = NEEDS_NONE;
        if (i < n) {
            const uint64_t key = keys[i];
            const int64_t b = block_first ? pr_block_of(block_first, n_blocks, i) : 0;
            const uint32_t md = mode ? min((uint32_t)mode[b], 3u) : 0u;      // (a byte above 3 counts as 3: no reference)
            if (md == 0u || md == 1u) c0 = needs_bi_cell(key, mv0 ? mv0 + 3 * b : nullptr, J, top_level, wide);
            if (md == 0u || md == 2u) c1 = needs_bi_cell(key, mv1 ? mv1 + 3 * b : nullptr, J, top_level, wide);
        }
        const uint64_t p0 = (uint64_t)__shfl_up((unsigned long long)c0, 1), p1 = (uint64_t)__shfl_up((unsigned long long)c1, 1);       // (every lane of the wave is here: i0 is the workgroup's)
        if (i < n) {
            flag[i] = (c0 != NEEDS_NONE && (lane == 0 || p0 != c0)) ? 1u : 0u;
            flag[n + i] = (c1 != NEEDS_NONE && (lane == 0 || p1 != c1)) ? 1u : 0u;
            cand[i] = c0;
            cand[n + i] = c1 == NEEDS_NONE ? c1 : (c1 | tag);
        }
    }
}

// region_needs_pick_kernel over the sorted, tagged list: the entries without the tag go to cells0, those with it to cells1 without
// it. first1: where the tagged entries begin in the list (m: there are none); that entry differs from the one before it, so its
// position is the number of cells of reference 0. Every store is bounded by cap.
__global__ __launch_bounds__(REG_THREADS) void region_needs_bi_pick_kernel(const uint64_t *__restrict__ list, int64_t m, const uint32_t *__restrict__ flag,
                                                                           const uint32_t *__restrict__ pos, const uint32_t *__restrict__ total,
                                                                           int64_t first1, uint64_t tag, int64_t cap, uint64_t *__restrict__ cells0,
                                                                           uint64_t *__restrict__ cells1)
{
    const int64_t n0 = first1 < m ? (int64_t)pos[first1] : (int64_t)*total;
    for (int64_t i = (int64_t)blockIdx.x * REG_THREADS + threadIdx.x; i < m; i += (int64_t)gridDim.x * REG_THREADS) {
        if (!flag[i]) continue;
        const uint64_t v = list[i];
        const int64_t j = (int64_t)pos[i];
        if (!(v & tag)) { if (j < cap) cells0[j] = v; }
        else if (j >= n0 && j - n0 < cap) cells1[j - n0] = v & ~tag;
    }
}

static inline unsigned region_grid(int64_t items, int64_t per_block)
{
    const int64_t g = ceil_div(items, per_block);
    return (unsigned)(g < 1 ? 1 : (g > REG_MAX_GRID ? REG_MAX_GRID : g));
}

// the rules the three entry points share: N as every plan takes it, nbits as raht_plan_create_from_keys takes it
static int region_check_keys(const char *what, const void *keys, int64_t N, int nbits)
{
    if (!keys) { set_error("%s: NULL keys", what); return RAHT_ERR_INVALID; }
    if (N < 1 || N >= ((int64_t)1 << 31)) { set_error("%s: N must be 1 .. 2^31 - 1", what); return RAHT_ERR_INVALID; }
    if (nbits < 1 || nbits > 63) { set_error("%s: nbits=%d (1..63)", what, nbits); return RAHT_ERR_INVALID; }
    return RAHT_OK;
}

// raht_region_needs for checked arguments: the rows' cells with neighbouring repeats dropped -> first (capacity cap), their number
template <typename KEY>
static int region_needs_first(const uint64_t *keys, int64_t N, int top_level, int wide, const KEY &key_of, uint32_t *flag, uint32_t *pos,
                              uint32_t *total, uint64_t *first, int64_t cap, uint32_t *found, hipStream_t s)
{
    const dim3 grid(region_grid(N, REG_THREADS * 4)), blk(REG_THREADS);
    hipLaunchKernelGGL(region_needs_flag_kernel<KEY>, grid, blk, 0, s, keys, N, top_level, wide, key_of, flag);
    RAHT_RET(exclusive_scan_u32(flag, pos, N, total, s));
    hipLaunchKernelGGL(region_needs_scatter_kernel<KEY>, grid, blk, 0, s, keys, N, top_level, wide, key_of, (const uint32_t *)flag,
                       (const uint32_t *)pos, cap, first);
    RAHT_HIP_CHECK(hipGetLastError());
    return read_back_u32(found, total, 1, nullptr, nullptr, 0, s);
}

}  // namespace raht

using namespace raht;

extern "C" {

int raht_region_layout(const uint64_t *keys_sorted, int64_t N, int nbits, int64_t row_lo, int64_t row_hi, int64_t *table,
                       raht_stream_t stream)
{
    RAHT_RET(region_check_keys("raht_region_layout", keys_sorted, N, nbits));
    if (!table) { set_error("raht_region_layout: NULL table"); return RAHT_ERR_INVALID; }
    if (row_lo < 0 || row_lo > row_hi || row_hi > N) { set_error("raht_region_layout: rows must satisfy 0 <= row_lo <= row_hi <= N"); return RAHT_ERR_INVALID; }
    hipStream_t s = (hipStream_t)stream;
    RAHT_HIP_CHECK(hipMemsetAsync(table, 0, sizeof(int64_t) * REG_BINS, s));
    hipLaunchKernelGGL(region_layout_kernel, dim3(region_grid(N, REG_THREADS * 4)), dim3(REG_THREADS), 0, s, keys_sorted, N, row_lo, row_hi,
                       (unsigned long long *)table);
    RAHT_HIP_CHECK(hipGetLastError());
    return RAHT_OK;
}

int raht_region_cells(const uint64_t *keys_sorted, int64_t N, int nbits, int top_level, int64_t n_cells, uint64_t *cell_keys,
                      int64_t *cell_first, raht_stream_t stream)
{
    RAHT_RET(region_check_keys("raht_region_cells", keys_sorted, N, nbits));
    if (!cell_keys || !cell_first) { set_error("raht_region_cells: NULL output"); return RAHT_ERR_INVALID; }
    if (top_level % 3 || top_level < 3 || top_level > nbits - 3) {
        set_error("raht_region_cells: top_level=%d must be a multiple of 3 in [3, nbits - 3]", top_level);
        return RAHT_ERR_INVALID;
    }
    if (n_cells < 1 || n_cells > N) { set_error("raht_region_cells: n_cells must be 1 .. N"); return RAHT_ERR_INVALID; }
    hipStream_t s = (hipStream_t)stream;
    return guarded("raht_region_cells", [&]() -> int {
        Scratch ws(sizeof(uint32_t) * (2 * (size_t)N + 1), s);
        if (!ws.ok()) { set_error("raht_region_cells: out of device memory"); return RAHT_ERR_NOMEM; }
        uint32_t *flag = ws.as<uint32_t>(), *pos = flag + N, *total = pos + N;
        const dim3 grid(region_grid(N, REG_THREADS * 4)), blk(REG_THREADS);
        hipLaunchKernelGGL(region_cell_flag_kernel, grid, blk, 0, s, keys_sorted, N, top_level, flag);
        RAHT_RET(exclusive_scan_u32(flag, pos, N, total, s));
        hipLaunchKernelGGL(region_cell_scatter_kernel, grid, blk, 0, s, keys_sorted, N, top_level, (const uint32_t *)flag,
                           (const uint32_t *)pos, n_cells, cell_keys, cell_first);
        RAHT_HIP_CHECK(hipGetLastError());
        uint32_t found = 0;
        RAHT_RET(read_back_u32(&found, total, 1, nullptr, nullptr, 0, s));
        if ((int64_t)found != n_cells) {
            set_error("raht_region_cells: the keys hold %u cells at level %d, the caller expected %lld", found, top_level, (long long)n_cells);
            return RAHT_ERR_INVALID;
        }
        return RAHT_OK;
    });
}

int raht_region_assemble(const int32_t *src, int64_t ld_src, int64_t n_src_rows, int32_t *dst, int64_t ld_dst, int64_t n_dst_rows, int D,
                         const int64_t *runs, int n_runs, raht_stream_t stream)
{
    if (!src || !dst || (n_runs > 0 && !runs)) { set_error("raht_region_assemble: NULL argument"); return RAHT_ERR_INVALID; }
    if (D < 1 || ld_src < D || ld_dst < D) { set_error("raht_region_assemble: bad D/ld"); return RAHT_ERR_INVALID; }
    if (n_src_rows < 1 || n_dst_rows < 1 || n_src_rows >= ((int64_t)1 << 31) || n_dst_rows >= ((int64_t)1 << 31)) {
        set_error("raht_region_assemble: both matrices hold 1 .. 2^31 - 1 rows");
        return RAHT_ERR_INVALID;
    }
    if (n_runs < 0 || n_runs > RAHT_REGION_BUCKETS) { set_error("raht_region_assemble: n_runs must be 0 .. %d", RAHT_REGION_BUCKETS); return RAHT_ERR_INVALID; }
    RegionRuns rr = {};
    rr.n = n_runs;
    int64_t dst_end = 0;                                 // destination runs ascending and disjoint: a row has one source
    for (int k = 0; k < n_runs; ++k) {
        const int64_t sr = runs[3 * k], dr = runs[3 * k + 1], cnt = runs[3 * k + 2];
        if (cnt < 0 || sr < 0 || sr > n_src_rows - cnt || dr < dst_end || dr > n_dst_rows - cnt) {
            set_error("raht_region_assemble: run %d (%lld, %lld, %lld) leaves a matrix or overlaps the run before it", k, (long long)sr,
                      (long long)dr, (long long)cnt);
            return RAHT_ERR_INVALID;
        }
        rr.src[k] = sr; rr.dst[k] = dr; rr.count[k] = cnt;
        dst_end = dr + cnt;
    }
    hipLaunchKernelGGL(region_assemble_kernel, dim3(region_grid(n_dst_rows, REG_TILE_ROWS)), dim3(REG_THREADS), 0, (hipStream_t)stream, src,
                       ld_src, dst, ld_dst, D, rr, n_dst_rows);
    RAHT_HIP_CHECK(hipGetLastError());
    return RAHT_OK;
}

int raht_region_layout_set(const uint64_t *keys_sorted, int64_t N, int nbits, const int64_t *row_bounds, int R, int64_t *table,
                           raht_stream_t stream)
{
    RAHT_RET(region_check_keys("raht_region_layout_set", keys_sorted, N, nbits));
    if (!row_bounds || !table) { set_error("raht_region_layout_set: NULL row_bounds or table"); return RAHT_ERR_INVALID; }
    if (R < 1 || R > RAHT_REGION_MAX_RANGES) { set_error("raht_region_layout_set: R=%d (1..%d)", R, RAHT_REGION_MAX_RANGES); return RAHT_ERR_INVALID; }
    hipStream_t s = (hipStream_t)stream;
    const size_t n_bins = (size_t)(2 * R + 1) * RAHT_REGION_BUCKETS;
    Scratch ws(sizeof(unsigned long long) * n_bins, s);  // (returns to the pool stream-ordered, behind the two launches)
    if (!ws.ok()) { set_error("raht_region_layout_set: out of device memory"); return RAHT_ERR_NOMEM; }
    unsigned long long *bins = ws.as<unsigned long long>();
    RAHT_HIP_CHECK(hipMemsetAsync(bins, 0, sizeof(unsigned long long) * n_bins, s));
    hipLaunchKernelGGL(region_layout_set_kernel, dim3(region_grid(N, REG_THREADS * 4)), dim3(REG_THREADS), 0, s, keys_sorted, N, row_bounds,
                       2 * R, bins);
    hipLaunchKernelGGL(region_layout_set_table_kernel, dim3(1), dim3(64), 0, s, (const unsigned long long *)bins, R, table);
    RAHT_HIP_CHECK(hipGetLastError());
    return RAHT_OK;
}

int raht_region_assemble_set(const int32_t *src, int64_t ld_src, int64_t n_src_rows, int32_t *dst, int64_t ld_dst, int64_t n_dst_rows, int D,
                             const int64_t *runs, const int64_t *runs_host, int n_runs, raht_stream_t stream)
{
    if (!src || !dst || (n_runs > 0 && !runs)) { set_error("raht_region_assemble_set: NULL argument"); return RAHT_ERR_INVALID; }
    if (D < 1 || ld_src < D || ld_dst < D) { set_error("raht_region_assemble_set: bad D/ld"); return RAHT_ERR_INVALID; }
    if (n_src_rows < 1 || n_dst_rows < 1 || n_src_rows >= ((int64_t)1 << 31) || n_dst_rows >= ((int64_t)1 << 31)) {
        set_error("raht_region_assemble_set: both matrices hold 1 .. 2^31 - 1 rows");
        return RAHT_ERR_INVALID;
    }
    if (n_runs < 0 || n_runs > RAHT_REGION_BUCKETS * RAHT_REGION_MAX_RANGES) {
        set_error("raht_region_assemble_set: n_runs must be 0 .. %d", RAHT_REGION_BUCKETS * RAHT_REGION_MAX_RANGES);
        return RAHT_ERR_INVALID;
    }
    int64_t dst_end = 0;                                 // the caller's host copy of the table, when there is one: raht_region_assemble's rules
    for (int k = 0; runs_host && k < n_runs; ++k) {
        const int64_t sr = runs_host[3 * k], dr = runs_host[3 * k + 1], cnt = runs_host[3 * k + 2];
        if (cnt < 0 || sr < 0 || sr > n_src_rows - cnt || dr < dst_end || dr > n_dst_rows - cnt) {
            set_error("raht_region_assemble_set: run %d (%lld, %lld, %lld) leaves a matrix or overlaps the run before it", k, (long long)sr,
                      (long long)dr, (long long)cnt);
            return RAHT_ERR_INVALID;
        }
        dst_end = dr + cnt;
    }
    hipLaunchKernelGGL(region_assemble_set_kernel, dim3(region_grid(n_dst_rows, REG_TILE_ROWS)), dim3(REG_THREADS), 0, (hipStream_t)stream, src,
                       ld_src, n_src_rows, dst, ld_dst, D, runs, n_runs, n_dst_rows);
    RAHT_HIP_CHECK(hipGetLastError());
    return RAHT_OK;
}

int raht_region_needs(const uint64_t *keys_sorted, int64_t N, int J, int top_level, int up, const int64_t *block_first, int64_t n_blocks,
                      const int8_t *mv, int block_log2, uint64_t *cells, int64_t capacity, int64_t *n_cells, raht_stream_t stream)
{
    if (J < 1 || J > 21) { set_error("raht_region_needs: J=%d (1..21)", J); return RAHT_ERR_INVALID; }
    RAHT_RET(region_check_keys("raht_region_needs", keys_sorted, N, 3 * J));
    if (!cells || !n_cells || capacity < 1) { set_error("raht_region_needs: NULL output or no capacity"); return RAHT_ERR_INVALID; }
    if (top_level % 3 || top_level < 3 || top_level > 3 * J - 3) {
        set_error("raht_region_needs: top_level=%d must be a multiple of 3 in [3, 3 J - 3]", top_level);
        return RAHT_ERR_INVALID;
    }
    if (up < 0 || up > 3) { set_error("raht_region_needs: up=%d (0..3)", up); return RAHT_ERR_INVALID; }
    if (mv && (!block_first || n_blocks < 1 || n_blocks > N || block_log2 < 1 || block_log2 > J)) {
        set_error("raht_region_needs: a motion field needs block_first, 1 <= n_blocks <= N and block_log2 in 1 .. J");
        return RAHT_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    const int wide = 3 * up > top_level ? 3 * up : top_level;
    return guarded("raht_region_needs", [&]() -> int {
        // without a field the rows' cells ascend: the first pass is the answer. Under one they do not: its list is sorted and passed again.
        Scratch ws((mv ? 2 * sizeof(uint64_t) + sizeof(uint32_t) : 0) * (size_t)N + sizeof(uint32_t) * (2 * (size_t)N + 2), s);
        if (!ws.ok()) { set_error("raht_region_needs: out of device memory"); return RAHT_ERR_NOMEM; }
        uint64_t *first = mv ? ws.as<uint64_t>() : cells, *sorted = mv ? first + N : nullptr;
        uint32_t *flag = mv ? (uint32_t *)(sorted + N) : ws.as<uint32_t>(), *pos = flag + N, *total = pos + N, *idx = total + 2;
        uint32_t found = 0;
        if (mv)
            RAHT_RET(region_needs_first(keys_sorted, N, top_level, wide, MvKey{block_first, n_blocks, mv, J}, flag, pos, total, first, N, &found, s));
        else
            RAHT_RET(region_needs_first(keys_sorted, N, top_level, wide, SameKey{}, flag, pos, total, first, capacity, &found, s));
        if (mv && found) {
            const int64_t M = (int64_t)found;            // (<= N: one flag per row)
            RAHT_RET(sort_keys_u32idx(first, M, 3 * J - top_level, sorted, idx, s));
            const dim3 grid(region_grid(M, REG_THREADS * 4)), blk(REG_THREADS);
            hipLaunchKernelGGL(region_needs_first_kernel, grid, blk, 0, s, (const uint64_t *)sorted, M, flag);
            RAHT_RET(exclusive_scan_u32(flag, pos, M, total, s));
            hipLaunchKernelGGL(region_needs_pick_kernel, grid, blk, 0, s, (const uint64_t *)sorted, M, (const uint32_t *)flag,
                               (const uint32_t *)pos, capacity, cells);
            RAHT_HIP_CHECK(hipGetLastError());
            RAHT_RET(read_back_u32(&found, total, 1, nullptr, nullptr, 0, s));
        }
        *n_cells = (int64_t)found;
        if ((int64_t)found > capacity) {
            set_error("raht_region_needs: %u cells, the caller's buffer holds %lld", found, (long long)capacity);
            return RAHT_ERR_INVALID;
        }
        return RAHT_OK;
    });
}

int raht_region_needs_bi(const uint64_t *keys_sorted, int64_t N, int J, int top_level, int up, const int64_t *block_first, int64_t n_blocks,
                         int block_log2, const int8_t *mv0, const int8_t *mv1, const uint8_t *mode, uint64_t *cells0, uint64_t *cells1,
                         int64_t capacity, int64_t *n_cells, raht_stream_t stream)
{
    const char *who = "raht_region_needs_bi";
    if (J < 1 || J > 21) { set_error("%s: J=%d (1..21)", who, J); return RAHT_ERR_INVALID; }
    RAHT_RET(region_check_keys(who, keys_sorted, N, 3 * J));
    if (!cells0 || !cells1 || !n_cells || capacity < 1) { set_error("%s: NULL output or no capacity", who); return RAHT_ERR_INVALID; }
    if (top_level % 3 || top_level < 3 || top_level > 3 * J - 3) {
        set_error("%s: top_level=%d must be a multiple of 3 in [3, 3 J - 3]", who, top_level);
        return RAHT_ERR_INVALID;
    }
    if (up < 0 || up > 3) { set_error("%s: up=%d (0..3)", who, up); return RAHT_ERR_INVALID; }
    const bool blocks = mv0 || mv1 || mode;
    if (blocks && (!block_first || n_blocks < 1 || n_blocks > N || block_log2 < 1 || block_log2 > J)) {
        set_error("%s: a motion field or block modes need block_first, 1 <= n_blocks <= N and block_log2 in 1 .. J", who);
        return RAHT_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    const int wide = 3 * up > top_level ? 3 * up : top_level;
    return guarded(who, [&]() -> int {
        uint32_t found[2] = {0, 0};                      // the cells of reference 0, of reference 1
        if (!blocks) {
            // no field, every block in mode 0: the rows' own cells ascend, raht_region_needs' first pass is both answers
            Scratch ws(sizeof(uint32_t) * (2 * (size_t)N + 2), s);
            if (!ws.ok()) { set_error("%s: out of device memory", who); return RAHT_ERR_NOMEM; }
            uint32_t *flag = ws.as<uint32_t>(), *pos = flag + N, *total = pos + N;
            RAHT_RET(region_needs_first(keys_sorted, N, top_level, wide, SameKey{}, flag, pos, total, cells0, capacity, &found[0], s));
            found[1] = found[0];
            const size_t kept = (size_t)((int64_t)found[0] < capacity ? (int64_t)found[0] : capacity);
            if (kept) RAHT_HIP_CHECK(hipMemcpyAsync(cells1, cells0, sizeof(uint64_t) * kept, hipMemcpyDeviceToDevice, s));
        } else {
            // candidates and flags of both references (2 N each) | the flagged candidates | scan | total | the sort's indices
            const size_t N2 = 2 * (size_t)N;
            Scratch ws(2 * sizeof(uint64_t) * N2 + sizeof(uint32_t) * (3 * N2 + 2), s);
            if (!ws.ok()) { set_error("%s: out of device memory", who); return RAHT_ERR_NOMEM; }
            uint64_t *cand = ws.as<uint64_t>(), *first = cand + N2;
            uint32_t *flag = (uint32_t *)(first + N2), *pos = flag + N2, *total = pos + N2, *idx = total + 2;
            const int cell_bits = 3 * J - top_level;     // (<= 60: the tag is bit 60 at most)
            const uint64_t tag = 1ull << cell_bits;
            const dim3 blk(REG_THREADS);
            hipLaunchKernelGGL(region_needs_bi_kernel, dim3(region_grid(N, REG_THREADS * 4)), blk, 0, s, keys_sorted, N, J, top_level, wide,
                               block_first, n_blocks, mv0, mv1, mode, tag, cand, flag);
            RAHT_RET(exclusive_scan_u32(flag, pos, (int64_t)N2, total, s));
            hipLaunchKernelGGL(region_needs_pick_kernel, dim3(region_grid((int64_t)N2, REG_THREADS * 4)), blk, 0, s, (const uint64_t *)cand,
                               (int64_t)N2, (const uint32_t *)flag, (const uint32_t *)pos, (int64_t)N2, first);
            RAHT_HIP_CHECK(hipGetLastError());
            uint32_t m_all = 0, m_0 = 0;                 // the flagged candidates, those of reference 0 (they come first)
            RAHT_RET(read_back_u32(&m_all, total, 1, &m_0, pos + N, 1, s));
            if ((int64_t)m_all >= ((int64_t)1 << 31)) {  // (the sort's limit; 2^30 rows at least)
                set_error("%s: %u candidate cells, 2^31 - 1 at most", who, m_all);
                return RAHT_ERR_INVALID;
            }
            if (m_all) {
                const int64_t M = (int64_t)m_all, first1 = (int64_t)m_0;
                uint64_t *sorted = cand;                 // (the candidates are compacted: their buffer is free)
                RAHT_RET(sort_keys_u32idx(first, M, cell_bits + 1, sorted, idx, s));
                const dim3 grid(region_grid(M, REG_THREADS * 4));
                hipLaunchKernelGGL(region_needs_first_kernel, grid, blk, 0, s, (const uint64_t *)sorted, M, flag);
                RAHT_RET(exclusive_scan_u32(flag, pos, M, total, s));
                hipLaunchKernelGGL(region_needs_bi_pick_kernel, grid, blk, 0, s, (const uint64_t *)sorted, M, (const uint32_t *)flag,
                                   (const uint32_t *)pos, (const uint32_t *)total, first1, tag, capacity, cells0, cells1);
                RAHT_HIP_CHECK(hipGetLastError());
                uint32_t all = 0, n0 = 0;
                RAHT_RET(read_back_u32(&all, total, 1, &n0, pos + (first1 < M ? first1 : 0), 1, s));
                found[0] = first1 < M ? n0 : all;
                found[1] = all - found[0];
            }
        }
        n_cells[0] = (int64_t)found[0];
        n_cells[1] = (int64_t)found[1];
        if ((int64_t)found[0] > capacity || (int64_t)found[1] > capacity) {
            set_error("%s: %u and %u cells, the caller's buffers hold %lld each", who, found[0], found[1], (long long)capacity);
            return RAHT_ERR_INVALID;
        }
        return RAHT_OK;
    });
}

}  // extern "C"
