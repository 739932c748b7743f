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
#include "raht_common.h"

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

}  // extern "C"
