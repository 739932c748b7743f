// schedule.hip -- the tile schedule of a plan (raht_common.h: Schedule, Stage): which rows every tile stage holds, what survives
// it, the butterfly heights and tile programs of the tile stages and the TOP stage that finishes the tree. Two builders: a chain
// of launches that never returns to the host (build_schedule_fast) and the exact one that reads every stage's size back
// (get_schedule_exact). A schedule owns its blocks (DevBuf); free_schedule / raht_plan_destroy release them behind a device
// synchronisation.
#include "raht_common.h"

#include <algorithm>
#include <atomic>

namespace raht {

__global__ void compact_scatter_kernel(const uint32_t *in, const uint32_t *flag, const uint32_t *pos, uint32_t *out, int64_t n);

// ---- tile schedule -----------------------------------------------------------------------------
// Entry j of a stage (row r = rows ? rows[j] : j) is merged inside its tile iff the whole subtree
// [r - wl, r + wr) lies inside the tile's row range; otherwise it survives to the next stage.
__global__ void stage_survivor_kernel(const uint32_t *__restrict__ rows, int64_t n, int R, int64_t N,
                                      const int32_t *__restrict__ wl, const int32_t *__restrict__ wr,
                                      const uint8_t *__restrict__ lvl, int top_level,
                                      uint32_t *__restrict__ survivor)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int64_t r = rows ? rows[j] : j;
    const int64_t t = j / R;
    const int64_t j0 = t * R, j1 = j0 + R;
    const int64_t start = rows ? rows[j0] : j0;
    const int64_t end = (j1 < n) ? (rows ? (int64_t)rows[j1] : j1) : N;
    const bool merged = (r > 0) && ((int)lvl[r] < top_level) && (r - wl[r] >= start) && (r + wr[r] <= end);
    survivor[j] = merged ? 0u : 1u;
}

// Channels per chunk (<= max_dc) such that every chunk, the last one included, holds at least one
// whole 16-byte lane chunk (the tile kernel fetches a row's tail as the 16 bytes that end with it).
static int fit_chunk_channels(int elem_size, int D, int max_dc)
{
    const int vn = 16 / elem_size;
    const int hi = std::max(std::min(max_dc, 64), vn);
    if (D <= hi) return D;
    for (int Dc = hi; Dc >= vn; --Dc) {
        const int r = D % Dc;
        if (r == 0 || r >= vn) return Dc;
    }
    for (int Dc = hi + 1; Dc <= 64; ++Dc) {               // nothing that narrow fits: widen
        const int r = D % Dc;
        if (r == 0 || r >= vn) return Dc;
    }
    return std::min(D, 64);                               // not reached (61..64 cover every remainder for D > 64)
}

int pick_chunk_channels(int elem_size, int D)
{
    return fit_chunk_channels(elem_size, D, 64);
}

size_t tile_lds_bytes(int R, int elem_size, int Dc, bool ident, bool qm)
{
    // data tile + per-slot butterfly record (16 B float / 24 B double), row id (later stages only),
    // Q position (fused quantization only), flag + histograms (1 KiB) + survivor slot list
    // (R x uint16) + the inverse's survivor prefetch area (12 rows)
    // (must match the carve-up in transform.hip: tile_kernel)
    const int vn = 16 / elem_size;
    const size_t Dp = (size_t)((Dc + vn - 1) / vn) * vn;                 // rows padded to whole 16-byte chunks
    size_t data = (size_t)R * Dp * elem_size;
    size_t meta = (size_t)R * ((elem_size == 4 ? 16 : 24) + (ident ? 0 : 4) + (qm ? 4 : 0) + 1);
    size_t surv = ((size_t)R * 2 + 15) & ~(size_t)15;
    return data + ((meta + 15) & ~(size_t)15) + 1024 + surv + (size_t)12 * Dp * elem_size;
}

int pick_tile_rows(const raht_plan *plan, int elem_size, int Dc)
{
    if (plan->tile_rows_override > 0) return plan->tile_rows_override;
    // Three 512-thread workgroups per CU. gfx950 hands out its 160 KiB of LDS in 128 granules of
    // 1280 bytes, so each workgroup may use 42 granules. Measured best on MI355X for the
    // 59-channel float32 case (R = 192); see DESIGN.md for the sweep.
    const size_t budget = (size_t)42 * 1280;
    for (int R = 512; R >= 64; R -= 8)
        if (tile_lds_bytes(R, elem_size, Dc, true, true) <= budget) return R;
    return 0;
}

void pick_tail_geometry(const raht_plan *plan, int elem_size, int D, int stage0_rows, int *tail_rows, int *tail_chunk,
                        int *final_rows)
{
    // Later stages hold a few % of the rows. Default: the same geometry as stage 0, trimmed so that
    // three workgroups still fit per CU with the slightly larger later-stage LDS layout (row ids).
    // Much larger chunked tiles (e.g. 1024 x 32) cut the number of stages but measured slower on cfg3
    // (one workgroup per CU, no overlap): 1.02 vs 0.955 ms per fused step.
    int Dc = std::min(D, 64), R = stage0_rows;
    if (D > 64) Dc = pick_chunk_channels(elem_size, D);
    if (plan->tail_chunk_override > 0) Dc = fit_chunk_channels(elem_size, D, std::min(plan->tail_chunk_override, std::min(D, 64)));
    if (plan->tail_rows_override > 0) {
        R = plan->tail_rows_override;
        while (R > 64 && tile_lds_bytes(R, elem_size, Dc, false, true) > (size_t)128 * 1280) R -= 64;
    } else {
        while (R > 64 && tile_lds_bytes(R, elem_size, Dc, false, true) > (size_t)42 * 1280) R -= 8;
    }
    *tail_rows = R;
    *tail_chunk = Dc;
    // The top of the tree is latency-bound: once at most this many entries are left, ONE launch
    // (top_kernel: a workgroup per 16-byte channel chunk, all entries in LDS, 16 bytes per entry)
    // finishes the tree. 8192 entries = 128 KiB of the CU's 160 KiB.
    // Default 1536 (rounds 1-2: 4096): one workgroup per chunk touching EVERY entry's row (one 128-byte line per
    // 16 useful bytes, on ceil(D / 4) CUs only) costs 6 us + 7.8 ns per entry (439 entries 9.4 us, 2310 entries 24 us,
    // 7013 entries 41 us), a tile stage 11 us and leaves 1/18 of its entries: above ~1500 entries one more tile stage
    // is cheaper. The reference's own shape (J = 10, ~1 M voxels x 56) leaves 2310 entries after two tile stages:
    // 0.239 -> 0.225 ms per fused step with the third tile stage (r03 sweep, tools/sweep_tail2.sh).
    int Rf = 1536;
    if (plan->final_rows_override > 0) Rf = std::min(plan->final_rows_override, RAHT_TOP_MAX_ROWS);
    *final_rows = Rf;
}

void free_schedule(Schedule &sc)
{
    // blocks go back to the cache and may be handed out again at once: nothing enqueued may still use
    // them (hipFree used to imply this wait; schedules are only dropped on rare, synchronous paths)
    if (!sc.stages.empty()) (void)hipDeviceSynchronize();
    sc.stages.clear();
    sc.ready = OwnedEvent();
}

int ensure_workspace(Schedule *sc, size_t row_bytes, bool split)
{
    if (row_bytes <= sc->ws_row_bytes && split == sc->ws_split) return RAHT_OK;
    row_bytes = std::max(row_bytes, sc->ws_row_bytes);
    for (size_t k = 1; k < sc->stages.size(); ++k) {
        Stage &st = sc->stages[k];
        if (st.ws) { (void)hipDeviceSynchronize(); st.ws.reset(); }
        const size_t one = (row_bytes * (size_t)st.n_entries + 255) & ~(size_t)255;
        if (st.ws.alloc(split ? 2 * one : one) != hipSuccess) {
            set_error("workspace allocation failed (%zu bytes)", split ? 2 * one : one);
            sc->ws_row_bytes = 0;
            return RAHT_ERR_NOMEM;
        }
        st.ws_inv_off = split ? one : 0;
    }
    sc->ws_row_bytes = row_bytes;
    sc->ws_split = split;
    return RAHT_OK;
}

__global__ void tile_start_kernel(const uint32_t *__restrict__ pos, int64_t n, int R, int64_t n_tiles,
                                  uint32_t total, uint32_t *__restrict__ surv_off)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t > n_tiles) return;
    surv_off[t] = (t < n_tiles) ? pos[t * R] : total;
    (void)n;
}

__global__ void gather_meta_kernel(const uint32_t *__restrict__ rows, int64_t n, const int32_t *__restrict__ wl,
                                   const int32_t *__restrict__ wr, const uint8_t *__restrict__ lvl,
                                   const uint32_t *__restrict__ inv_order, int32_t *__restrict__ e_wl,
                                   int32_t *__restrict__ e_wr, uint8_t *__restrict__ e_lvl, uint32_t *__restrict__ e_pos)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t r = rows[j];
    e_wl[j] = wl[r]; e_wr[j] = wr[r]; e_lvl[j] = lvl[r]; e_pos[j] = inv_order[r];
}

// ---- butterfly heights of the tile stages -----------------------------------------------------------
// One wave per tile, every tile stage of a schedule in ONE launch. The recurrence is the forward transform's own order:
// walk the binary levels present in the tile upwards; a butterfly (partner slot p, own slot j) gets h = 1 + max(cur[p],
// cur[j]) and leaves it in cur[p], the slot that carries the merged node on. Butterflies of one level touch disjoint slots,
// so a level is: every lane reads the two values of its (<= SPL) butterflies, then writes them -- two LDS round trips. A
// lane keeps its slots' level / partner / height in registers; LDS holds one byte per slot (and the row ids of a later
// stage, for the partner search). What "merged in this tile" means is the tile kernel's own predicate (transform.hip, P1).
constexpr int HT_MAX_ROWS = 1024, HT_MAX_STAGES = 8;
struct HeightStage {
    const uint32_t *rows; const int32_t *wl, *wr; const uint8_t *lvl; uint8_t *ht;
    int64_t n; int R; uint32_t first_tile;
    // launched BEFORE the host knows the stage sizes (build_schedule_fast): the entry count and whether the stage is a tile
    // stage at all come from the schedule builder's device state; first_tile then counts the tiles of the stages' CAPACITIES
    const uint32_t *n_dev, *kind_dev; uint32_t kind_tile;
};
struct HeightArgs { HeightStage st[HT_MAX_STAGES]; int n_stages; uint32_t n_tiles; int64_t N; int top_level; };

template <int SPL>
__global__ __launch_bounds__(64) void tile_heights_kernel(const HeightArgs H)
{
    extern __shared__ __align__(16) unsigned char ht_smem[];
    int k = 0;
#pragma unroll
    for (int q = 1; q < HT_MAX_STAGES; ++q) k += (q < H.n_stages && blockIdx.x >= H.st[q].first_tile) ? 1 : 0;
    PL_STAMP(1, blockIdx.x, 0);
    const HeightStage &S = H.st[k];
    const int R = S.R;
    const int lane = threadIdx.x;
    const int64_t e0 = (int64_t)(blockIdx.x - S.first_tile) * R;
    if (S.kind_dev && *S.kind_dev != S.kind_tile) return;
    const int64_t Sn = S.n_dev ? (int64_t)*S.n_dev : S.n;
    if (e0 >= Sn) return;
    const uint32_t *__restrict__ rows = S.rows;
    const int nt = (int)min((int64_t)R, Sn - e0);
    uint8_t *s_cur = ht_smem;                                   // [R]
    uint32_t *s_row = (uint32_t *)(ht_smem + ((R + 15) & ~15)); // [R], later stages only
    const int64_t start_row = rows ? (int64_t)rows[e0] : e0;
    const int64_t end_row = (e0 + R < Sn) ? (rows ? (int64_t)rows[e0 + R] : e0 + R) : H.N;
    int lv[SPL], part[SPL];
    int32_t wlv[SPL], wrv[SPL];
    int64_t r[SPL];
#pragma unroll
    for (int s = 0; s < SPL; ++s) {                          // all loads first: one round trip
        const int j = lane + s * 64;
        lv[s] = 255; wlv[s] = 0; wrv[s] = 0; r[s] = 0;
        if (j < nt) {
            r[s] = rows ? (int64_t)rows[e0 + j] : e0 + j;
            lv[s] = (int)S.lvl[e0 + j]; wlv[s] = S.wl[e0 + j]; wrv[s] = S.wr[e0 + j];
        }
    }
    if (rows) {
#pragma unroll
        for (int s = 0; s < SPL; ++s) { const int j = lane + s * 64; if (j < nt) s_row[j] = (uint32_t)r[s]; }
    }
#pragma unroll
    for (int s = 0; s < SPL; ++s) { const int j = lane + s * 64; if (j < nt) s_cur[j] = 0; }
    __syncthreads();
    PL_STAMP(1, blockIdx.x, 1);                       // metadata loaded
    uint64_t mask = 0;
#pragma unroll
    for (int s = 0; s < SPL; ++s) {
        const int j = lane + s * 64;
        const bool merged = (j < nt) && (r[s] > 0) && (lv[s] < H.top_level) && (r[s] - wlv[s] >= start_row) && (r[s] + wrv[s] <= end_row);
        part[s] = 0;
        if (merged) {
            if (!rows) part[s] = j - wlv[s];
            else {                                          // the partner row r - wl is an entry of this tile
                const uint32_t want = (uint32_t)(r[s] - wlv[s]);
                int lo = 0, hi = j - 1;
                while (lo < hi) { const int mid = (lo + hi) >> 1; if (s_row[mid] < want) lo = mid + 1; else hi = mid; }
                part[s] = lo;
            }
            mask |= (uint64_t)1 << lv[s];
        } else {
            lv[s] = 255;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)mask, d, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(mask >> 32), d, 64);
        mask |= (uint64_t)lo | ((uint64_t)hi << 32);
    }
    int ht[SPL];
#pragma unroll
    for (int s = 0; s < SPL; ++s) ht[s] = 0;
    PL_STAMP(1, blockIdx.x, 2);                       // partners resolved, level mask reduced
    PL_NOTE_LEVELS(blockIdx.x, __popcll(mask));
    // (the reduced mask is the same in every lane but lives in vector registers: made scalar, the loop's counter, find-first-set
    // and branch run on the scalar unit -- see level_extent_kernel)
    mask = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)mask) |
           ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(mask >> 32)) << 32);
    while (mask) {
        const int l = __ffsll((unsigned long long)mask) - 1;
        mask &= mask - 1;
        int h[SPL];
#pragma unroll
        for (int s = 0; s < SPL; ++s) {
            h[s] = 0;
            if (lv[s] == l) h[s] = 1 + max((int)s_cur[part[s]], (int)s_cur[lane + s * 64]);
        }
#pragma unroll
        for (int s = 0; s < SPL; ++s)
            if (lv[s] == l) { ht[s] = h[s]; s_cur[part[s]] = (uint8_t)h[s]; }
        __syncthreads();                                    // one wave: orders the LDS traffic of consecutive levels
    }
    PL_STAMP(1, blockIdx.x, 3);                       // levels walked
#pragma unroll
    for (int s = 0; s < SPL; ++s) { const int j = lane + s * 64; if (j < nt) S.ht[e0 + j] = (uint8_t)ht[s]; }
    PL_STAMP(1, blockIdx.x, 4);
}

// f(SPL) with the slots per lane of a one-wave-per-tile kernel as a compile-time constant (decltype(spl)::value): the smallest of
// 3, 4, 8, 16 that covers R rows (R <= HT_MAX_ROWS). In the style of by_ident_slots (tile_host.h).
template <typename F>
static void by_lane_slots(int R, F &&f)
{
    const int spl = (R + 63) / 64;
    if (spl <= 3) f(std::integral_constant<int, 3>{});
    else if (spl <= 4) f(std::integral_constant<int, 4>{});
    else if (spl <= 8) f(std::integral_constant<int, 8>{});
    else f(std::integral_constant<int, 16>{});
}

static void launch_heights_kernel(const HeightArgs &H, int maxR, bool any_rows, hipStream_t s)
{
    const size_t lds = (size_t)((maxR + 15) & ~15) + (any_rows ? (size_t)maxR * 4 : 0);
    by_lane_slots(maxR, [&](auto spl) { hipLaunchKernelGGL(tile_heights_kernel<decltype(spl)::value>, dim3(H.n_tiles), dim3(64), lds, s, H); });
}

// One HeightStage of a launch: its arrays, and where its tiles start in the launch's grid.
static HeightStage height_stage(const StageArrays &a, int R, uint32_t first_tile)
{
    HeightStage h;
    h.rows = a.rows; h.wl = a.wl; h.wr = a.wr; h.lvl = a.lvl; h.ht = a.ht; h.n = 0; h.R = R; h.first_tile = first_tile;
    h.n_dev = nullptr; h.kind_dev = nullptr; h.kind_tile = 0;
    return h;
}

// Testing hook (raht.h: raht_debug_height_stages_per_launch): tile stages per heights launch, HT_MAX_STAGES unless set.
static std::atomic<int> g_height_group{HT_MAX_STAGES};

// heights of every tile stage of a finished schedule: one launch (sizes are known on the host by now; enqueued, not
// waited for: the transforms that read them run behind this on the same stream)
static int launch_stage_heights(raht_plan *plan, Schedule &sc, hipStream_t s)
{
    // up to HT_MAX_STAGES tile stages per launch; deeper schedules (deep or unbalanced key sets, small tail_rows / final_rows
    // overrides: get_schedule_exact builds up to plan->max_stages = 24 of them) take several launches
    HeightArgs H;
    int maxR = 0;
    bool any_rows = false;
    auto reset = [&]() { H.n_stages = 0; H.n_tiles = 0; H.N = plan->N; H.top_level = plan->top_level; maxR = 0; any_rows = false; };
    auto flush = [&]() -> int {
        if (H.n_stages == 0) return RAHT_OK;
        for (int q = H.n_stages; q < HT_MAX_STAGES; ++q) H.st[q] = H.st[0];
        launch_heights_kernel(H, maxR, any_rows, s);
        RAHT_HIP_CHECK(hipGetLastError());
        reset();
        return RAHT_OK;
    };
    reset();
    const int group = g_height_group.load();      // (a testing hook cuts it to walk the several-launches path on ordinary scenes)
    for (size_t k = 0; k < sc.stages.size(); ++k) {
        Stage &st = sc.stages[k];
        if (st.is_top || st.n_entries < 1) continue;
        if (st.tile_rows > HT_MAX_ROWS) { set_error("tile heights: %d rows per tile not supported", st.tile_rows); return RAHT_ERR_UNSUPPORTED; }
        if (!st.e_ht) RAHT_HIP_CHECK(st.e_ht.alloc((size_t)st.n_entries));
        HeightStage &h = H.st[H.n_stages++];
        h = height_stage(stage_arrays(plan, st), st.tile_rows, H.n_tiles);
        h.n = st.n_entries;
        H.n_tiles += (uint32_t)st.n_tiles;
        maxR = std::max(maxR, st.tile_rows);
        any_rows = any_rows || st.rows != nullptr;
        if (H.n_stages == group) RAHT_RET(flush());
    }
    return flush();
}

// ---- tile programs of the mixed-precision tile kernels (Stage::prog, raht_common.h) -------------------
// One wave per tile, one launch per tile stage. Same predicate and partner search as tile_heights_kernel (and the tile kernels
// that resolved their butterflies at run time before); the heights come from Stage::e_ht. Records of one height touch disjoint
// slots, so their order inside a height (here: the LDS cursor's) does not change any result.
struct ProgStage {
    const uint32_t *rows; const int32_t *wl, *wr; const uint8_t *lvl, *ht; const uint32_t *pos;
    uint32_t *prog; int64_t n; int R; uint32_t stride, ab; int compact;
};

template <int SPL>
__global__ __launch_bounds__(64) void tile_program_kernel(const ProgStage S, int64_t N, int top_level, const int64_t *__restrict__ wsum)
{
    extern __shared__ __align__(16) unsigned char pg_smem[];
    __shared__ uint32_t s_hist[64], s_cur[64];
    uint32_t *s_row = (uint32_t *)pg_smem;                  // [R], later stages only
    const int R = S.R;
    const int lane = threadIdx.x;
    const int64_t e0 = (int64_t)blockIdx.x * R;
    if (e0 >= S.n) return;
    const uint32_t *__restrict__ rows = S.rows;
    const int nt = (int)min((int64_t)R, S.n - e0);
    const int64_t start_row = rows ? (int64_t)rows[e0] : e0;
    const int64_t end_row = (e0 + R < S.n) ? (rows ? (int64_t)rows[e0 + R] : e0 + R) : N;
    uint32_t *pg = S.prog + (size_t)blockIdx.x * S.stride;
    uint32_t *rw = pg + 32, *rec = pg + 32 + R;
    double *ab = (double *)(pg + S.ab);
    int lv[SPL], ht[SPL];
    int32_t wlv[SPL], wrv[SPL];
    uint32_t pos[SPL];
    int64_t r[SPL];
#pragma unroll
    for (int s = 0; s < SPL; ++s) {                          // all loads first: one round trip
        const int j = lane + s * 64;
        lv[s] = 255; wlv[s] = 0; wrv[s] = 0; r[s] = 0; ht[s] = 0; pos[s] = 0;
        if (j < nt) {
            r[s] = rows ? (int64_t)rows[e0 + j] : e0 + j;
            lv[s] = (int)S.lvl[e0 + j]; wlv[s] = S.wl[e0 + j]; wrv[s] = S.wr[e0 + j];
            ht[s] = S.ht[e0 + j] & 63; pos[s] = S.pos[e0 + j];
        }
    }
    s_hist[lane] = 0;
    if (rows) {
#pragma unroll
        for (int s = 0; s < SPL; ++s) { const int j = lane + s * 64; if (j < nt) s_row[j] = (uint32_t)r[s]; }
    }
    __syncthreads();
    bool merged[SPL];
    int part[SPL];
#pragma unroll
    for (int s = 0; s < SPL; ++s) {
        const int j = lane + s * 64;
        merged[s] = (j < nt) && (r[s] > 0) && (lv[s] < top_level) && (r[s] - wlv[s] >= start_row) && (r[s] + wrv[s] <= end_row);
        part[s] = 0;
        if (merged[s]) {
            if (!rows) part[s] = j - wlv[s];
            else {                                          // the partner row r - wl is an entry of this tile
                const uint32_t want = (uint32_t)(r[s] - wlv[s]);
                int lo = 0, hi = j - 1;
                while (lo < hi) { const int mid = (lo + hi) >> 1; if (s_row[mid] < want) lo = mid + 1; else hi = mid; }
                part[s] = lo;
            }
            atomicAdd(&s_hist[ht[s]], 1u);
        }
        if (j < nt) rw[j] = pos[s] | (merged[s] ? 0x80000000u : 0u);
    }
    __syncthreads();
    const uint32_t c = s_hist[lane];
    uint32_t inc = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(inc, d, 64);
        if (lane >= d) inc += t;
    }
    ((uint16_t *)pg)[lane] = (uint16_t)inc;
    s_cur[lane] = inc - c;
    const uint32_t n_merged = (uint32_t)__shfl((int)inc, 63, 64);
    __syncthreads();
    const uint64_t lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    uint32_t n_surv = 0;
#pragma unroll
    for (int s = 0; s < SPL; ++s) {
        const int j = lane + s * 64;
        const bool surv = j < nt && !merged[s];
        const uint64_t bal = __ballot(surv);
        if (surv) rec[n_merged + n_surv + (uint32_t)__popcll(bal & lt)] = (uint32_t)j;
        n_surv += (uint32_t)__popcll(bal);
        if (merged[s]) {
            const uint32_t k = atomicAdd(&s_cur[ht[s]], 1u);
            if (S.compact) {
                rec[k] = (uint32_t)j | ((uint32_t)wlv[s] << 10) | ((uint32_t)wrv[s] << 20);
            } else {
                double w0, w1;
                pair_weights(r[s], wlv[s], wrv[s], wsum, w0, w1);
                const double den = w0 + w1;
                rec[k] = (uint32_t)part[s] | ((uint32_t)j << 16);
                ab[2 * k] = sqrt(w0 / den);                  // RAHT.py:321-322
                ab[2 * k + 1] = sqrt(w1 / den);
            }
        }
    }
}

int build_tile_programs(raht_plan *plan, Schedule *sc, hipStream_t s)
{
    bool built = false;
    for (auto &st : sc->stages) {
        if (st.is_top || st.n_entries < 1 || st.prog) continue;
        const int R = st.tile_rows;
        if (R > HT_MAX_ROWS || !st.e_ht) { set_error("tile programs: %d rows per tile not supported", R); return RAHT_ERR_UNSUPPORTED; }
        ProgStage P;
        const StageArrays a = stage_arrays(plan, st);
        P.rows = a.rows; P.wl = a.wl; P.wr = a.wr; P.lvl = a.lvl; P.pos = a.pos; P.ht = a.ht;
        P.n = st.n_entries; P.R = R;
        // compact records: stage 0 rows are tile slots, so a butterfly merged inside a tile of <= 1024 rows has extents <= 1023
        P.compact = (st.rows == nullptr && plan->wsum == nullptr) ? 1 : 0;
        P.ab = (uint32_t)(32 + 2 * R + 3) & ~3u;
        P.stride = P.compact ? P.ab : P.ab + 4 * (uint32_t)R;
        if (!P.wl || !P.wr || !P.lvl || !P.pos) { set_error("tile programs: missing plan arrays"); return RAHT_ERR_INVALID; }
        RAHT_HIP_CHECK(st.prog.alloc((size_t)P.stride * (size_t)st.n_tiles));
        P.prog = st.prog;
        const size_t lds = st.rows ? (size_t)R * 4 : 0;
        const unsigned grid = (unsigned)st.n_tiles;
        by_lane_slots(R, [&](auto spl) {
            hipLaunchKernelGGL(tile_program_kernel<decltype(spl)::value>, dim3(grid), dim3(64), lds, s, P, plan->N, plan->top_level, plan->wsum);
        });
        RAHT_HIP_CHECK(hipGetLastError());
        st.prog_stride = P.stride; st.prog_ab = P.ab; st.prog_compact = P.compact != 0;
        built = true;
    }
    if (built) {
        if (!sc->ready) RAHT_HIP_CHECK(hipEventCreateWithFlags(&sc->ready.ev, hipEventDisableTiming));
        RAHT_HIP_CHECK(hipEventRecord(sc->ready, s));
        sc->ready_on = s;
    }
    return RAHT_OK;
}

// ---- TOP stage: every butterfly still to do, resolved against the stage's entry list ----------------
__global__ void top_resolve_kernel(const uint32_t *__restrict__ rows, int64_t n, const int32_t *__restrict__ wl,
                                   const int32_t *__restrict__ wr, const uint8_t *__restrict__ lvl,
                                   const int64_t *__restrict__ wsum, int top_level, uint32_t *__restrict__ pj,
                                   double *__restrict__ ab, uint8_t *__restrict__ bucket, uint32_t *__restrict__ is_root)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const int64_t r = rows ? (int64_t)rows[e] : e;
    const int l = (int)lvl[r];
    const bool merged = (r > 0) && (l < top_level);
    is_root[e] = merged ? 0u : 1u;
    bucket[e] = merged ? (uint8_t)l : (uint8_t)63;       // roots sort behind every butterfly (levels are <= 62)
    uint32_t rec = 0;
    double a = 0.0, b = 0.0;
    if (merged) {
        const int64_t want = r - wl[r];                  // the partner row is an entry of this stage as well
        int64_t p = want;
        if (rows) {
            int64_t lo = 0, hi = e - 1;
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if ((int64_t)rows[mid] < want) lo = mid + 1; else hi = mid;
            }
            p = lo;
        }
        double w0, w1;
        pair_weights(r, wl[r], wr[r], wsum, w0, w1);
        const double den = w0 + w1;
        a = sqrt(w0 / den);                              // RAHT.py:321-322
        b = sqrt(w1 / den);
        rec = (uint32_t)p | ((uint32_t)e << 16);
    }
    pj[e] = rec; ab[2 * e] = a; ab[2 * e + 1] = b;
}

__global__ void top_gather_kernel(const uint32_t *__restrict__ perm, uint32_t n_merges, const uint32_t *__restrict__ pj,
                                  const double *__restrict__ ab, uint32_t *__restrict__ t_pj,
                                  float *__restrict__ t_ab32, double *__restrict__ t_ab64)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_merges) return;
    const uint32_t e = perm[k];
    t_pj[k] = pj[e];
    const double a = ab[2 * e], b = ab[2 * e + 1];
    t_ab64[2 * k] = a; t_ab64[2 * k + 1] = b;
    t_ab32[2 * k] = (float)a; t_ab32[2 * k + 1] = (float)b;
}

__global__ void top_root_rank_kernel(const uint32_t *__restrict__ is_root, const uint32_t *__restrict__ pos, int64_t n,
                                     uint32_t *__restrict__ t_root)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) t_root[e] = is_root[e] ? pos[e] : 0xffffffffu;
}

// entry-ordered copies of the plan metadata of a stage with a row list (st.rows, st.n_entries)
static hipError_t gather_stage_meta(const raht_plan *plan, Stage &st, hipStream_t s)
{
    const size_t n = (size_t)st.n_entries;
    hipError_t e = hipSuccess;
    if ((e = st.e_wl.alloc(n)) != hipSuccess || (e = st.e_wr.alloc(n)) != hipSuccess || (e = st.e_lvl.alloc(n)) != hipSuccess ||
        (e = st.e_pos.alloc(n)) != hipSuccess) return e;
    hipLaunchKernelGGL(gather_meta_kernel, dim3((unsigned)ceil_div((int64_t)n, 256)), dim3(256), 0, s, st.rows, (int64_t)n, plan->wl,
                       plan->wr, plan->lvl, plan->inv_order, st.e_wl, st.e_wr, st.e_lvl, st.e_pos);
    return hipSuccess;
}

// the n entries st.rows (nullptr: the identity) become the TOP stage
static int build_top_stage(raht_plan *plan, int64_t n, hipStream_t s, Stage &st)
{
    st.is_top = true;
    st.n_entries = n;
    st.n_tiles = 1;
    st.tile_rows = (int)n;
    const uint32_t *rows = st.rows;
    const unsigned gb = (unsigned)ceil_div(n, 256);
    if (rows) RAHT_HIP_CHECK(gather_stage_meta(plan, st, s));
    // scratch: pj | is_root | pos | perm | boff[65] | total | ab (double, 8-byte aligned first) | bucket
    Scratch buf(sizeof(double) * 2 * (size_t)n + sizeof(uint32_t) * (4 * (size_t)n + 66) + (size_t)n, s);
    if (!buf.ok()) return RAHT_ERR_NOMEM;
    double *ab = buf.as<double>();
    uint32_t *pj = (uint32_t *)(ab + 2 * n), *is_root = pj + n, *pos = is_root + n, *perm = pos + n, *boff = perm + n,
             *total = boff + 65;
    uint8_t *bucket = (uint8_t *)(total + 1);
    hipLaunchKernelGGL(top_resolve_kernel, dim3(gb), dim3(256), 0, s, rows, n, plan->wl, plan->wr, plan->lvl, plan->wsum,
                       plan->top_level, pj, ab, bucket, is_root);
    RAHT_RET(exclusive_scan_u32(is_root, pos, n, total, s));
    RAHT_HIP_CHECK(st.t_root.alloc((size_t)n));
    hipLaunchKernelGGL(top_root_rank_kernel, dim3(gb), dim3(256), 0, s, is_root, pos, n, st.t_root);
    RAHT_RET(bucket_sort_u8(bucket, perm, n, 6, boff, s));
    RAHT_RET(read_back_u32(st.t_loff, boff, 65, nullptr, nullptr, 0, s));
    st.n_merges = st.t_loff[63];
    {
        // the level program: non-empty levels, ascending; the trailing run of levels with at most 64
        // butterflies each (the top of the tree) is chained by one wave
        uint32_t *lev = st.t_lev_host;                    // lives in the stage: the upload below stays asynchronous
        int nlev = 0;
        for (int l = 0; l < 63; ++l)
            if (st.t_loff[l + 1] > st.t_loff[l]) { lev[2 * nlev] = st.t_loff[l]; lev[2 * nlev + 1] = st.t_loff[l + 1]; ++nlev; }
        int nbig = nlev;
        while (nbig > 0 && lev[2 * (nbig - 1) + 1] - lev[2 * (nbig - 1)] <= 64) --nbig;
        // the chained records live in LDS next to the entries (16 B each + 12 / 20 B per record)
        const size_t lds_budget = 160 * 1024 - 1024;
        while (nbig < nlev && (size_t)n * 16 + (size_t)(st.n_merges - lev[2 * nbig]) * 20 > lds_budget) ++nbig;
        st.t_nlev = nlev; st.t_nbig = nbig;
        st.t_small_start = (nbig < nlev) ? lev[2 * nbig] : st.n_merges;
        RAHT_HIP_CHECK(st.t_lev.alloc(2 * 64));
        // staged through a scratch-independent pageable copy: hipMemcpyAsync from pageable memory copies the
        // source before it returns, so `st` may be moved afterwards
        RAHT_HIP_CHECK(hipMemcpyAsync(st.t_lev, lev, sizeof(uint32_t) * 2 * (size_t)std::max(nlev, 1), hipMemcpyHostToDevice, s));
    }
    const size_t nm = std::max<size_t>(st.n_merges, 1);
    RAHT_HIP_CHECK(st.t_pj.alloc(nm));
    RAHT_HIP_CHECK(st.t_ab32.alloc(2 * nm));
    RAHT_HIP_CHECK(st.t_ab64.alloc(2 * nm));
    if (st.n_merges)
        hipLaunchKernelGGL(top_gather_kernel, dim3((unsigned)ceil_div(st.n_merges, 256)), dim3(256), 0, s, perm, st.n_merges,
                           pj, ab, st.t_pj, st.t_ab32, st.t_ab64);
    return RAHT_OK;                                  // (the scratch goes back to the pool: stream-ordered reuse)
}

// ---- schedule build, device-driven ----------------------------------------------------------------
// The exact builder below (get_schedule_exact) reads every stage's size back to the host before it can size
// and launch the next stage: 4-5 round trips of ~20 us each, during which the GPU idles -- more than half of
// a cfg3 plan build. Here the chain of stages runs on the device: every stage is two launches
// (sched_count_kernel: survivor flags + per-block counts; sched_emit_kernel: the next stage's entry list,
// its entry-ordered plan metadata and this stage's per-tile survivor offsets in one pass), the TOP stage is
// ONE single-workgroup launch (sched_top_kernel), each kernel decides from the device-resident SchedState
// whether it has anything to do, buffers are sized from generous bounds (a stage keeps < 1/3 of its entries:
// measured 1/20 at 184 rows per tile, 1/6 at 64), and ONE read-back at the end tells the host how it went.
// Anything unusual (a bound exceeded, more stages than were enqueued, no progress) -> the exact builder.
constexpr int SB_THREADS = 256, SB_ITEMS = 8, SB_BLOCK = SB_THREADS * SB_ITEMS;
constexpr int SCHED_SPEC_MAX = 8;                  // stages enqueued speculatively, at most
enum { SK_NONE = 0, SK_TILE = 1, SK_TOP = 2 };

struct SchedState {
    uint32_t n[SCHED_SPEC_MAX + 2];                // entries of stage k
    uint32_t kind[SCHED_SPEC_MAX + 2];             // what stage k is (written by the stage before it)
    uint32_t finished;                             // the tree is done: last_stage / last_is_top are valid
    uint32_t last_stage, last_is_top;
    uint32_t trouble;                              // 1 = a buffer bound was exceeded, 2 = a stage made no progress
    uint32_t top[4];                               // TOP stage: n_merges, nlev, nbig, small_start
};
constexpr int SCHED_STATE_WORDS = sizeof(SchedState) / 4;

__device__ __forceinline__ uint32_t block_sum_256(uint32_t v, uint32_t *red /* [4] */)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const uint32_t t = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
    return t;
}

// wl / wr / lvl are ENTRY-ordered for this stage (stage 0: the plan arrays, entry = row)
// n_first >= 0: this is the FIRST launch of the chain (stage 0 as a tile stage of n_first entries): nothing has
// written the state yet -- block 0 does (the launches behind this one read it), every block takes n from the argument
__device__ __forceinline__ void sched_state_init(SchedState *S, uint32_t n0, uint32_t kind0)
{
    uint32_t *w = (uint32_t *)S;
    for (int i = threadIdx.x; i < SCHED_STATE_WORDS; i += blockDim.x) w[i] = 0;
    __syncthreads();
    if (threadIdx.x == 0) { S->n[0] = n0; S->kind[0] = kind0; }
}

__global__ __launch_bounds__(SB_THREADS) void sched_count_kernel(SchedState *__restrict__ S, int k, const uint32_t *__restrict__ rows,
                                                                 const int32_t *__restrict__ wl, const int32_t *__restrict__ wr,
                                                                 const uint8_t *__restrict__ lvl, int R, int64_t N, int top_level,
                                                                 uint8_t *__restrict__ flags, uint32_t *__restrict__ blk_cnt, int64_t n_first)
{
    __shared__ uint32_t red[4];
    if (n_first >= 0) { if (blockIdx.x == 0) sched_state_init(S, (uint32_t)n_first, SK_TILE); }
    else if (S->kind[k] != SK_TILE) return;
    const int64_t n = n_first >= 0 ? n_first : (int64_t)S->n[k];
    const int64_t base = (int64_t)blockIdx.x * SB_BLOCK + (int64_t)threadIdx.x * SB_ITEMS;
    if ((int64_t)blockIdx.x * SB_BLOCK >= n) return;
    uint32_t cnt = 0;
    // tile bounds by 32-bit arithmetic, carried along the thread's 8 consecutive entries (a 64-bit division per
    // entry was most of this kernel's time)
    uint32_t j0 = (uint32_t)base / (uint32_t)R * (uint32_t)R;
    int64_t start = 0, end = 0;
    bool fresh = true;
    // the thread's 8 consecutive entries in a few wide loads (32 / 32 / 8 / 32 bytes) instead of 8 x 4 narrow ones: the launch is
    // bound by its load instructions, not by the 27 MB it reads on cfg3 (20 -> ~12 us)
    int32_t v_wl[SB_ITEMS], v_wr[SB_ITEMS];
    uint32_t v_row[SB_ITEMS];
    uint8_t v_lv[SB_ITEMS];
    if (base + SB_ITEMS <= n) {
        const int4 a0 = *(const int4 *)(wl + base), a1 = *(const int4 *)(wl + base + 4);
        const int4 b0 = *(const int4 *)(wr + base), b1 = *(const int4 *)(wr + base + 4);
        const uint2 l8 = *(const uint2 *)(lvl + base);
        v_wl[0] = a0.x; v_wl[1] = a0.y; v_wl[2] = a0.z; v_wl[3] = a0.w; v_wl[4] = a1.x; v_wl[5] = a1.y; v_wl[6] = a1.z; v_wl[7] = a1.w;
        v_wr[0] = b0.x; v_wr[1] = b0.y; v_wr[2] = b0.z; v_wr[3] = b0.w; v_wr[4] = b1.x; v_wr[5] = b1.y; v_wr[6] = b1.z; v_wr[7] = b1.w;
#pragma unroll
        for (int q = 0; q < 4; ++q) { v_lv[q] = (uint8_t)(l8.x >> (8 * q)); v_lv[4 + q] = (uint8_t)(l8.y >> (8 * q)); }
        if (rows) {
            const uint4 r0 = *(const uint4 *)(rows + base), r1 = *(const uint4 *)(rows + base + 4);
            v_row[0] = r0.x; v_row[1] = r0.y; v_row[2] = r0.z; v_row[3] = r0.w; v_row[4] = r1.x; v_row[5] = r1.y; v_row[6] = r1.z; v_row[7] = r1.w;
        }
    } else {
#pragma unroll
        for (int q = 0; q < SB_ITEMS; ++q) {
            const int64_t j = min(base + q, n - 1);
            v_wl[q] = wl[j]; v_wr[q] = wr[j]; v_lv[q] = lvl[j]; v_row[q] = rows ? rows[j] : 0u;
        }
    }
    uint8_t fl[SB_ITEMS];
#pragma unroll
    for (int q = 0; q < SB_ITEMS; ++q) {
        const int64_t j = base + q;
        fl[q] = 0;
        if (j < n) {
            if ((uint32_t)j >= j0 + (uint32_t)R) { j0 += (uint32_t)R; fresh = true; }
            if (fresh) {
                const int64_t j1 = (int64_t)j0 + R;
                start = rows ? (int64_t)rows[j0] : (int64_t)j0;
                end = (j1 < n) ? (rows ? (int64_t)rows[j1] : j1) : N;
                fresh = false;
            }
            const int64_t r = rows ? (int64_t)v_row[q] : j;
            const bool merged = (r > 0) && ((int)v_lv[q] < top_level) && (r - v_wl[q] >= start) && (r + v_wr[q] <= end);
            fl[q] = merged ? 0 : 1;
            cnt += merged ? 0u : 1u;
        }
    }
    if (base + SB_ITEMS <= n) {
        uint2 f8;
        f8.x = (uint32_t)fl[0] | ((uint32_t)fl[1] << 8) | ((uint32_t)fl[2] << 16) | ((uint32_t)fl[3] << 24);
        f8.y = (uint32_t)fl[4] | ((uint32_t)fl[5] << 8) | ((uint32_t)fl[6] << 16) | ((uint32_t)fl[7] << 24);
        *(uint2 *)(flags + base) = f8;
    } else {
#pragma unroll
        for (int q = 0; q < SB_ITEMS; ++q) if (base + q < n) flags[base + q] = fl[q];
    }
    const uint32_t tot = block_sum_256(cnt, red);
    if (threadIdx.x == 0) blk_cnt[blockIdx.x] = tot;
}

// p_* are the PLAN arrays (row-indexed): the next stage's entry-ordered copies are gathered from them here
__global__ __launch_bounds__(SB_THREADS) void sched_emit_kernel(SchedState *__restrict__ S, int k, const uint32_t *__restrict__ rows,
                                                                const uint8_t *__restrict__ flags, const uint32_t *__restrict__ blk_cnt,
                                                                int R, uint32_t Rf, uint32_t n_roots,
                                                                const int32_t *__restrict__ p_wl, const int32_t *__restrict__ p_wr,
                                                                const uint8_t *__restrict__ p_lvl, const uint32_t *__restrict__ p_inv,
                                                                uint32_t *__restrict__ n_rows, int32_t *__restrict__ n_wl, int32_t *__restrict__ n_wr,
                                                                uint8_t *__restrict__ n_lvl, uint32_t *__restrict__ n_pos, uint32_t cap_next,
                                                                uint32_t *__restrict__ surv_off)
{
    __shared__ uint32_t red[4];
    __shared__ uint32_t wsum[4];
    if (S->kind[k] != SK_TILE) return;
    const int64_t n = S->n[k];
    const int64_t nblk = (n + SB_BLOCK - 1) / SB_BLOCK;
    if ((int64_t)blockIdx.x >= nblk) return;
    // survivors in the blocks before this one (<= a few thousand words from L2)
    uint32_t part = 0;
    for (int64_t b = threadIdx.x; b < (int64_t)blockIdx.x; b += SB_THREADS) part += blk_cnt[b];
    const uint32_t block_base = block_sum_256(part, red);
    // exclusive scan of this block's flags (8 consecutive entries per thread)
    const int64_t base = (int64_t)blockIdx.x * SB_BLOCK + (int64_t)threadIdx.x * SB_ITEMS;
    uint8_t f[SB_ITEMS];
    uint32_t mine = 0;
    if (base + SB_ITEMS <= n) {                             // (8 flags in one load: the buffer is 16-byte aligned)
        const uint2 f8 = *(const uint2 *)(flags + base);
#pragma unroll
        for (int q = 0; q < 4; ++q) { f[q] = (uint8_t)(f8.x >> (8 * q)); f[4 + q] = (uint8_t)(f8.y >> (8 * q)); }
#pragma unroll
        for (int q = 0; q < SB_ITEMS; ++q) mine += f[q];
    } else {
#pragma unroll
        for (int q = 0; q < SB_ITEMS; ++q) { f[q] = (base + q < n) ? flags[base + q] : 0; mine += f[q]; }
    }
    uint32_t inc = mine;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t t = __shfl_up(inc, d, 64); if (lane >= d) inc += t; }
    if (lane == 63) wsum[wid] = inc;
    __syncthreads();
    uint32_t before = 0, block_tot = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) { if (w < wid) before += wsum[w]; block_tot += wsum[w]; }
    uint32_t pos = block_base + before + inc - mine;
    uint32_t tile = (uint32_t)base / (uint32_t)R;
    uint32_t next_start = tile * (uint32_t)R;               // first tile boundary at or after `base`
    if (next_start < (uint32_t)base) { ++tile; next_start += (uint32_t)R; }
    // three loops -- the survivors' rows, their plan entries, the stores -- so that every load of a phase is in flight before the
    // first one is used (one loop made each survivor two dependent round trips of its own: see sched_tail_kernel)
    uint32_t g_r[SB_ITEMS], g_pos[SB_ITEMS], g_inv[SB_ITEMS];
    int32_t g_wl[SB_ITEMS], g_wr[SB_ITEMS];
    uint8_t g_lv[SB_ITEMS];
    bool keep[SB_ITEMS];
#pragma unroll
    for (int q = 0; q < SB_ITEMS; ++q) {
        const int64_t j = base + q;
        keep[q] = false; g_pos[q] = 0; g_r[q] = (uint32_t)j;
        if (j < n) {
            if ((uint32_t)j == next_start) { surv_off[tile] = pos; ++tile; next_start += (uint32_t)R; }   // first survivor of the tile
            if (f[q]) {
                keep[q] = pos < cap_next;
                g_pos[q] = pos;
                if (keep[q] && rows) g_r[q] = rows[j];
                ++pos;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < SB_ITEMS; ++q) {
        g_wl[q] = 0; g_wr[q] = 0; g_lv[q] = 0; g_inv[q] = 0;
        if (keep[q]) { const uint32_t r = g_r[q]; g_wl[q] = p_wl[r]; g_wr[q] = p_wr[r]; g_lv[q] = p_lvl[r]; g_inv[q] = p_inv[r]; }
    }
#pragma unroll
    for (int q = 0; q < SB_ITEMS; ++q)
        if (keep[q]) { const uint32_t o = g_pos[q]; n_rows[o] = g_r[q]; n_wl[o] = g_wl[q]; n_wr[o] = g_wr[q]; n_lvl[o] = g_lv[q]; n_pos[o] = g_inv[q]; }
    if ((int64_t)blockIdx.x == nblk - 1 && threadIdx.x == 0) {
        const uint32_t total = block_base + block_tot;
        surv_off[(n + R - 1) / R] = total;
        S->n[k + 1] = total;
        if (total > cap_next) S->trouble = 1;                                                     // (and the chain stops: kind[k + 1] stays SK_NONE)
        else if (total == n_roots) { S->finished = 1; S->last_stage = (uint32_t)k; S->last_is_top = 0; }   // only the roots are left
        else if (total >= (uint32_t)n) S->trouble = 2;                                              // no progress
        else S->kind[k + 1] = (total <= Rf) ? SK_TOP : SK_TILE;
    }
}

// The TOP stage in one workgroup: every butterfly still to do, resolved against the stage's entry list, bucketed by
// level; root ranks; the level program (what build_top_stage does with a dozen launches and a read-back).
constexpr int ST_THREADS = 1024;
struct SchedTopOut { uint32_t *t_pj; float *t_ab32; double *t_ab64; uint32_t *t_root; uint32_t *t_lev; };

__device__ __forceinline__ void sched_top_body(SchedState *__restrict__ S, int k, int n, const uint32_t *__restrict__ rows,
                                               const int32_t *__restrict__ p_wl, const int32_t *__restrict__ p_wr,
                                               const uint8_t *__restrict__ p_lvl, const int64_t *__restrict__ wsum,
                                               int top_level, const SchedTopOut &O)
{
    __shared__ uint32_t s_rows[RAHT_TOP_MAX_ROWS];
    __shared__ uint32_t hist[64], cursor[64], wtot[ST_THREADS / 64];
    __shared__ uint32_t root_base;
    uint32_t *__restrict__ t_pj = O.t_pj, *__restrict__ t_root = O.t_root, *__restrict__ t_lev = O.t_lev;
    float *__restrict__ t_ab32 = O.t_ab32;
    double *__restrict__ t_ab64 = O.t_ab64;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    if (tid < 64) hist[tid] = 0;
    if (tid == 0) root_base = 0;
    for (int e = tid; e < n; e += ST_THREADS) s_rows[e] = rows ? rows[e] : (uint32_t)e;
    __syncthreads();
    PL_STAMP(2, 0, 8);                                              // top: entry rows in LDS
    // pass 1: level histogram of the butterflies; root ranks in entry order
    for (int e0 = 0; e0 < n; e0 += ST_THREADS) {
        const int e = e0 + tid;
        bool root = false;
        if (e < n) {
            const uint32_t r = s_rows[e];
            const int l = (int)p_lvl[r];
            const bool merged = (r > 0) && (l < top_level);
            root = !merged;
            if (merged) atomicAdd(&hist[l], 1u);
        }
        const uint64_t bal = __ballot(root);
        if (lane == 0) wtot[wid] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t before = root_base;
        for (int w = 0; w < wid; ++w) before += wtot[w];
        if (e < n) t_root[e] = root ? before + (uint32_t)__popcll(bal & (((uint64_t)1 << lane) - 1)) : 0xffffffffu;
        __syncthreads();
        if (tid == 0) { uint32_t t = 0; for (int w = 0; w < ST_THREADS / 64; ++w) t += wtot[w]; root_base += t; }
        __syncthreads();
    }
    PL_STAMP(2, 0, 9);                                              // top: pass 1 done
    // level offsets + the level program: wave 0, lane l = binary level l
    if (wid == 0) {
        const uint32_t h = (lane < 63) ? hist[lane] : 0u;
        uint32_t inc = h;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const uint32_t t = __shfl_up(inc, d, 64); if (lane >= d) inc += t; }
        const uint32_t first = inc - h;
        cursor[lane] = first;
        const uint32_t n_merges = (uint32_t)__shfl((int)inc, 63, 64);
        const uint64_t nonempty = __ballot(h > 0), below = ((uint64_t)1 << lane) - 1;
        const int nlev = __popcll(nonempty);
        const int my = __popcll(nonempty & below);              // index of this level among the non-empty ones
        if (h > 0) { t_lev[2 * my] = first; t_lev[2 * my + 1] = first + h; }
        // the trailing run of levels with <= 64 butterflies each is chained by one wave; its records live in LDS next
        // to the entries (16 B per entry + 12 / 20 B per record; 160 KiB - 1 KiB): walk it down from the top while it fits
        const uint64_t big = __ballot(h > 64);
        int nbig = big ? __popcll(nonempty & (((uint64_t)2 << (63 - __clzll((long long)big))) - 1)) : 0;
        const size_t lds_budget = 160 * 1024 - 1024;
        uint32_t small_start = n_merges;
        // first butterfly of the non-empty level with index q: broadcast from the lane that owns it
        for (;;) {
            uint32_t cand = n_merges;
            if (nbig < nlev) {
                const uint64_t owner = __ballot(h > 0 && my == nbig);
                cand = (uint32_t)__shfl((int)first, __ffsll((unsigned long long)owner) - 1, 64);
            }
            if (nbig < nlev && (size_t)n * 16 + (size_t)(n_merges - cand) * 20 > lds_budget) { ++nbig; continue; }
            small_start = cand;
            break;
        }
        if (lane == 0) {
            S->top[0] = n_merges; S->top[1] = (uint32_t)nlev; S->top[2] = (uint32_t)nbig; S->top[3] = small_start;
            S->finished = 1; S->last_stage = (uint32_t)k; S->last_is_top = 1;
        }
    }
    __syncthreads();
    PL_STAMP(2, 0, 10);                                             // top: level program written
    // pass 2: resolve and place every butterfly (any order inside a level: they are independent)
    for (int e = tid; e < n; e += ST_THREADS) {
        const uint32_t r = s_rows[e];
        const int l = (int)p_lvl[r];
        if (!((r > 0) && (l < top_level))) continue;
        const int32_t wlr = p_wl[r], wrr = p_wr[r];
        const uint32_t want = r - (uint32_t)wlr;            // the partner row is an entry of this stage as well
        int lo = 0, hi = e - 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_rows[mid] < want) lo = mid + 1; else hi = mid;
        }
        double w0, w1;
        pair_weights((int64_t)r, wlr, wrr, wsum, w0, w1);
        const double den = w0 + w1;
        const double a = sqrt(w0 / den), b = sqrt(w1 / den);        // RAHT.py:321-322
        const uint32_t pos = atomicAdd(&cursor[l], 1u);
        t_pj[pos] = (uint32_t)lo | ((uint32_t)e << 16);
        t_ab64[2 * pos] = a; t_ab64[2 * pos + 1] = b;
        t_ab32[2 * pos] = (float)a; t_ab32[2 * pos + 1] = (float)b;
    }
    PL_STAMP(2, 0, 11);                                             // top: pass 2 issued
}

// The END of the chain in ONE launch of one workgroup: from stage k0 on, every tile stage of at most `tail_max`
// entries (flags, survivor scan, the next stage's entry list and this stage's per-tile survivor offsets: what
// sched_count_kernel + sched_emit_kernel do for the large stages) and the TOP stage. On cfg3 that is stage 2
// (7 013 entries) and the top stage (439): two launches of work instead of the eight (two of them empty) that the
// launch-per-step chain enqueued -- back-to-back launches cost 4.6 us each even when they have nothing to do.
struct SchedStageBufs {                         // buffers of stage k (entry-ordered copies; surv: its per-tile survivor offsets)
    uint32_t *rows[SCHED_SPEC_MAX + 2]; int32_t *wl[SCHED_SPEC_MAX + 2], *wr[SCHED_SPEC_MAX + 2];
    uint8_t *lvl[SCHED_SPEC_MAX + 2]; uint32_t *pos[SCHED_SPEC_MAX + 2], *surv[SCHED_SPEC_MAX + 2];
    uint32_t cap[SCHED_SPEC_MAX + 2];
};

__global__ __launch_bounds__(ST_THREADS) void sched_tail_kernel(SchedState *S, int k_multi, int k_last, SchedStageBufs B, int R, uint32_t Rf,
                                                                uint32_t n_roots, int64_t N, int top_level, uint32_t tail_max,
                                                                const int32_t *__restrict__ p_wl, const int32_t *__restrict__ p_wr,
                                                                const uint8_t *__restrict__ p_lvl, const uint32_t *__restrict__ p_inv,
                                                                const int64_t *__restrict__ wsum, SchedTopOut O, int64_t n_first)
{
    __shared__ uint32_t wcnt[8 * (ST_THREADS / 64)], woff[8 * (ST_THREADS / 64) + 1];
    __shared__ uint32_t s_kind[SCHED_SPEC_MAX + 2], s_n[SCHED_SPEC_MAX + 2];   // the chain's state: ONE read at the start, then kept here
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    PL_SLOT_DECL;
    PL_STAMP_NEXT();                                                        // [0] start
    if (n_first >= 0) { sched_state_init(S, (uint32_t)n_first, SK_TOP); __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __syncthreads(); }   // (a tree that fits the top stage)
    // stages 1 .. k_multi - 1 had the multi-workgroup launches if they were tile stages; one of them may have turned out
    // to be the top stage already (a tree that shrank faster than expected)
    // (what this workgroup itself decides about stage k + 1 goes to the state in memory AND into these copies: a global read
    // per stage was a ~2 us round trip on a chip that runs nothing else)
    if (tid < SCHED_SPEC_MAX + 2) {
        s_kind[tid] = (n_first >= 0) ? (tid == 0 ? (uint32_t)SK_TOP : (uint32_t)SK_NONE) : __atomic_load_n(&S->kind[tid], __ATOMIC_RELAXED);
        s_n[tid] = (n_first >= 0) ? (tid == 0 ? (uint32_t)n_first : 0u) : __atomic_load_n(&S->n[tid], __ATOMIC_RELAXED);
    }
    __syncthreads();
    for (int k = (k_multi == 0) ? 0 : 1; k <= k_last; ++k) {
        const uint32_t kind = s_kind[k], n = s_n[k];
        PL_STAMP_NEXT();                                                    // state of stage k read
        if (kind == SK_TOP) {
            sched_top_body(S, k, (int)n, B.rows[k], p_wl, p_wr, p_lvl, wsum, top_level, O);
            return;
        }
        if (kind == SK_TILE && k < k_multi) continue;                       // done by its own launches
        if (kind != SK_TILE || n > tail_max || n > B.cap[k] || k == k_last) return;   // nothing left / larger than expected: exact builder
        const uint32_t *__restrict__ rows = B.rows[k];
        const int32_t *__restrict__ wl = B.wl[k], *__restrict__ wr = B.wr[k];
        const uint8_t *__restrict__ lvl = B.lvl[k];
        uint32_t *__restrict__ surv_off = B.surv[k];
        uint32_t *__restrict__ n_rows = B.rows[k + 1], *__restrict__ n_pos = B.pos[k + 1];
        int32_t *__restrict__ n_wl = B.wl[k + 1], *__restrict__ n_wr = B.wr[k + 1];
        uint8_t *__restrict__ n_lvl = B.lvl[k + 1];
        const uint32_t cap_next = B.cap[k + 1];
        uint32_t running = 0;                                               // survivors in front of this pass (uniform)
        // TI x 1024 entries per pass (entry j = base + q * 1024 + tid): the loads of a pass are independent of each
        // other, so a 7 013-entry stage is ONE round of dependent L2 round trips instead of seven
        constexpr int TI = 8, NWV = ST_THREADS / 64;
        for (uint32_t base = 0; base < n; base += ST_THREADS * TI) {
            // every load of a pass is issued before the first one is used (two loops): with the survivor test in the loading
            // loop the compiler waited per iteration -- eight dependent round trips of ~2 us for one 7 013-entry stage
            uint32_t r[TI], e_start[TI], e_end[TI];
            int32_t e_wl[TI], e_wr[TI];
            uint8_t e_lv[TI];
            uint64_t bal[TI];
#pragma unroll
            for (int q = 0; q < TI; ++q) {
                const uint32_t j = min(base + (uint32_t)(q * ST_THREADS + tid), n - 1);
                const uint32_t j0 = j / (uint32_t)R * (uint32_t)R, j1 = j0 + (uint32_t)R;
                r[q] = rows[j]; e_lv[q] = lvl[j]; e_wl[q] = wl[j]; e_wr[q] = wr[j];
                e_start[q] = rows[j0];
                e_end[q] = rows[min(j1, n - 1)];
            }
#pragma unroll
            for (int q = 0; q < TI; ++q) {
                const uint32_t j = base + (uint32_t)(q * ST_THREADS + tid);
                bool surv = false;
                if (j < n) {
                    const uint32_t j1 = j / (uint32_t)R * (uint32_t)R + (uint32_t)R;
                    const int64_t start = (int64_t)e_start[q], end = (j1 < n) ? (int64_t)e_end[q] : N;
                    const bool merged = (r[q] > 0) && ((int)e_lv[q] < top_level) && ((int64_t)r[q] - e_wl[q] >= start) && ((int64_t)r[q] + e_wr[q] <= end);
                    surv = !merged;
                }
                bal[q] = __ballot(surv);
                if (lane == 0) wcnt[q * NWV + wid] = (uint32_t)__popcll(bal[q]);
            }
            __syncthreads();
            if (wid == 0) {                                                 // exclusive offsets of the TI * 16 (q, wave) counts
                const uint32_t c0 = wcnt[2 * lane], c1 = wcnt[2 * lane + 1];
                uint32_t inc = c0 + c1;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) { const uint32_t t = __shfl_up(inc, d, 64); if (lane >= d) inc += t; }
                woff[2 * lane] = inc - c0 - c1;
                woff[2 * lane + 1] = inc - c1;
                if (lane == 63) woff[TI * NWV] = inc;
            }
            // the survivors' plan rows: gathered (all in flight) while wave 0 scans, stored once the offsets are known
            int32_t g_wl[TI], g_wr[TI];
            uint32_t g_inv[TI];
            uint8_t g_lv[TI];
#pragma unroll
            for (int q = 0; q < TI; ++q) {
                g_wl[q] = 0; g_wr[q] = 0; g_inv[q] = 0; g_lv[q] = 0;
                if ((bal[q] >> lane) & 1) { const uint32_t rr = r[q]; g_wl[q] = p_wl[rr]; g_wr[q] = p_wr[rr]; g_lv[q] = p_lvl[rr]; g_inv[q] = p_inv[rr]; }
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < TI; ++q) {
                const uint32_t j = base + (uint32_t)(q * ST_THREADS + tid);
                if (j < n) {
                    const uint32_t pos = running + woff[q * NWV + wid] + (uint32_t)__popcll(bal[q] & (((uint64_t)1 << lane) - 1));
                    if (j % (uint32_t)R == 0) surv_off[j / (uint32_t)R] = pos;     // first survivor of the tile
                    if (((bal[q] >> lane) & 1) && pos < cap_next) {
                        n_rows[pos] = r[q]; n_wl[pos] = g_wl[q]; n_wr[pos] = g_wr[q]; n_lvl[pos] = g_lv[q]; n_pos[pos] = g_inv[q];
                    }
                }
            }
            running += woff[TI * NWV];
            __syncthreads();
        }
        if (tid == 0) {
            const uint32_t total = running;
            surv_off[(n + (uint32_t)R - 1) / (uint32_t)R] = total;
            S->n[k + 1] = total;
            s_n[k + 1] = total;
            if (total > cap_next) S->trouble = 1;                                                      // (and the chain stops)
            else if (total == n_roots) { S->finished = 1; S->last_stage = (uint32_t)k; S->last_is_top = 0; }   // only the roots are left
            else if (total >= n) S->trouble = 2;                                                       // no progress
            else { const uint32_t nk = (total <= Rf) ? SK_TOP : SK_TILE; S->kind[k + 1] = nk; s_kind[k + 1] = nk; }
        }
        // The next stage of THIS workgroup reads what this one wrote: workgroup scope (its waves share the CU's vector cache;
        // the stores are complete before the barrier). An agent-scope __threadfence() here wrote the XCD's whole L2 back -- tens
        // of MB of the earlier kernels' dirty lines -- once per wave: 18 of this kernel's 24 us (profiles/r04b_plan_phase_clocks.txt).
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __syncthreads();
    }
}

static int get_schedule_exact(raht_plan *plan, int R0, int R1, int Rf, hipStream_t s, Schedule **out);

// -> RAHT_OK and *built = true when the schedule was built; *built = false: use the exact builder
static int build_schedule_fast(raht_plan *plan, int R0, int R1, int Rf, hipStream_t s, Schedule &sc, bool *built, bool *heights_done)
{
    *built = false;
    *heights_done = false;
    const int64_t N = plan->N;
    // Sizes are unknown on the host. Stages expected to be large (a stage keeps ~1/20 of its entries at 184 rows per
    // tile, ~1/6 at 64: assume 1/16 resp. 1/4) get the two multi-workgroup launches; from the first stage expected to
    // be small on, ONE single-workgroup launch finishes the chain (sched_tail_kernel: up to TAIL_MAX entries per stage).
    // Buffers hold 1/3 of the stage before (+ slack). A stage larger than expected at the tail, or a bound exceeded ->
    // the state says so and the exact builder takes over.
    constexpr uint32_t TAIL_MAX = 65536;
    constexpr int KB = SCHED_SPEC_MAX;                    // stages with buffers: 0 .. KB
    int64_t cap[SCHED_SPEC_MAX + 2];
    cap[0] = N;
    for (int k = 0; k <= KB; ++k) cap[k + 1] = std::min<int64_t>(cap[k], cap[k] / 3 + 2048);
    int KS = 0;                                           // stages given the multi-workgroup launches: k = 0 .. KS - 1
    if (N > Rf) {
        double expect = (double)N;
        while (KS < KB - 1 && KS < plan->max_stages && (KS == 0 || expect > (double)TAIL_MAX * 0.5)) { ++KS; expect /= (R0 >= 128 ? 16.0 : 4.0); }
    }
    // speculative stages 0 .. KB + 1 (stage k >= 1: its entry list and entry-ordered copies; a tile stage's survivor offsets and
    // heights) and the arrays of the TOP stage, whichever stage that turns out to be. They own their blocks: what the schedule
    // does not take over goes back to the cache when this function returns.
    std::vector<Stage> spec((size_t)KB + 2);
    Stage top;
    bool ok = true;
    auto take = [&](auto &buf, size_t count) { if (ok && buf.alloc(count) != hipSuccess) ok = false; };
    for (int k = 0; k < KB && N > Rf; ++k) {
        const int R = (k == 0) ? R0 : R1;
        take(spec[(size_t)k].surv_off, (size_t)(ceil_div(cap[k], R) + 1));
        Stage &nx = spec[(size_t)k + 1];
        const size_t c = (size_t)cap[k + 1];
        take(nx.rows, c); take(nx.e_wl, c); take(nx.e_wr, c); take(nx.e_lvl, c); take(nx.e_pos, c);
    }
    // The butterfly heights of every tile stage are enqueued right behind the chain, BEFORE the read-back below: their launch
    // takes sizes and stage kinds from the device state and a grid that covers the stages' capacities, so the host's wait for the
    // read-back (~15-20 us of wake-up and launch latency, during which the GPU used to idle) overlaps the kernel.
    // (A non-default raht_debug_height_stages_per_launch, the testing hook of launch_stage_heights, keeps the launch behind the
    // read-back.)
    const bool early_heights = N > Rf && KB <= HT_MAX_STAGES && std::max(R0, R1) <= HT_MAX_ROWS && g_height_group.load() == HT_MAX_STAGES;
    if (early_heights)
        for (int k = 0; k < KB; ++k) take(spec[(size_t)k].e_ht, (size_t)cap[k]);
    const size_t tm = (size_t)std::max(Rf, 1);
    take(top.t_pj, tm); take(top.t_ab32, 2 * tm); take(top.t_ab64, 2 * tm); take(top.t_root, tm); take(top.t_lev, 128);
    // scratch: state | per-block counts | flags
    const size_t nblk0 = (size_t)ceil_div(N, SB_BLOCK);
    Scratch scr(sizeof(SchedState) + sizeof(uint32_t) * nblk0 + (size_t)N + 16, s);
    // (the blocks taken so far go back to the cache on return: nothing enqueued may still use them)
    if (!ok || !scr.ok()) { (void)hipDeviceSynchronize(); return RAHT_ERR_NOMEM; }
    SchedState *dS = scr.as<SchedState>();
    uint32_t *blk_cnt = (uint32_t *)(dS + 1);
    uint8_t *flags = (uint8_t *)(((uintptr_t)(blk_cnt + nblk0) + 15) & ~(uintptr_t)15);      // (sched_count_kernel stores 8 flags at a time)
    SchedStageBufs SB;
    for (int k = 0; k <= KB + 1 && k < SCHED_SPEC_MAX + 2; ++k) {
        const Stage &b = spec[(size_t)k];
        SB.rows[k] = b.rows; SB.wl[k] = b.e_wl; SB.wr[k] = b.e_wr; SB.lvl[k] = b.e_lvl; SB.pos[k] = b.e_pos; SB.surv[k] = b.surv_off;
        SB.cap[k] = (uint32_t)cap[k];
    }
    const SchedTopOut TO = {top.t_pj, top.t_ab32, top.t_ab64, top.t_root, top.t_lev};
    // the first launch of the chain also initialises the state (no upload, no memset: ~5 us each)
    for (int k = 0; k < KS; ++k) {
        const Stage &cur = spec[(size_t)k], &nx = spec[(size_t)k + 1];
        const StageArrays a = stage_arrays(plan, cur);
        const int R = (k == 0) ? R0 : R1;
        const unsigned gb = (unsigned)ceil_div(cap[k], SB_BLOCK);
        hipLaunchKernelGGL(sched_count_kernel, dim3(gb), dim3(SB_THREADS), 0, s, dS, k, a.rows, a.wl, a.wr, a.lvl, R, N, plan->top_level,
                           flags, blk_cnt, k == 0 ? N : (int64_t)-1);
        hipLaunchKernelGGL(sched_emit_kernel, dim3(gb), dim3(SB_THREADS), 0, s, dS, k, a.rows, flags, blk_cnt, R, (uint32_t)Rf,
                           (uint32_t)plan->n_roots, plan->wl, plan->wr, plan->lvl, plan->inv_order, nx.rows, nx.e_wl, nx.e_wr, nx.e_lvl,
                           nx.e_pos, (uint32_t)cap[k + 1], cur.surv_off);
    }
    hipLaunchKernelGGL(sched_tail_kernel, dim3(1), dim3(ST_THREADS), 0, s, dS, KS, KB, SB, R1, (uint32_t)Rf, (uint32_t)plan->n_roots, N,
                       plan->top_level, TAIL_MAX, plan->wl, plan->wr, plan->lvl, plan->inv_order, plan->wsum, TO, KS == 0 ? N : (int64_t)-1);
    auto heights_behind = [&]() {
        HeightArgs H;
        H.n_stages = 0; H.n_tiles = 0; H.N = N; H.top_level = plan->top_level;
        for (int k = 0; k < KB; ++k) {
            HeightStage &h = H.st[H.n_stages++];
            h = height_stage(stage_arrays(plan, spec[(size_t)k]), (k == 0) ? R0 : R1, H.n_tiles);
            h.n_dev = &dS->n[k]; h.kind_dev = &dS->kind[k]; h.kind_tile = SK_TILE;
            H.n_tiles += (uint32_t)ceil_div(cap[k], h.R);
        }
        for (int q = H.n_stages; q < HT_MAX_STAGES; ++q) H.st[q] = H.st[0];
        launch_heights_kernel(H, std::max(R0, R1), true, s);
    };
    hipError_t e = hipGetLastError();
    SchedState hs;
    int rc = RAHT_ERR_HIP;
    if (e == hipSuccess) {
        rc = read_back_u32((uint32_t *)&hs, (const uint32_t *)dS, SCHED_STATE_WORDS, plan->pend_host, plan->pend_dev, plan->pend_n, s,
                           early_heights ? std::function<void()>(heights_behind) : std::function<void()>());
        if (rc == RAHT_OK && hipGetLastError() != hipSuccess) rc = RAHT_ERR_HIP;
        if (rc == RAHT_OK) plan->pend_n = 0;              // delivered
    }
    if (rc != RAHT_OK || !hs.finished || hs.trouble || (int)hs.last_stage >= plan->max_stages) {
        (void)hipStreamSynchronize(s);                    // (every block taken above goes back to the cache on return)
        (void)hipGetLastError();
        return rc == RAHT_OK ? RAHT_OK : rc;             // *built stays false: the exact builder decides
    }
    const int K = (int)hs.last_stage + 1;
    for (int k = 0; k < K; ++k) {
        Stage &st = spec[(size_t)k];
        st.n_entries = hs.n[k];
        if (k == K - 1 && hs.last_is_top) {
            st.is_top = true;
            st.n_tiles = 1;
            st.tile_rows = (int)st.n_entries;
            st.n_merges = hs.top[0]; st.t_nlev = (int)hs.top[1]; st.t_nbig = (int)hs.top[2]; st.t_small_start = hs.top[3];
            st.t_pj = std::move(top.t_pj); st.t_ab32 = std::move(top.t_ab32); st.t_ab64 = std::move(top.t_ab64);
            st.t_root = std::move(top.t_root); st.t_lev = std::move(top.t_lev);
            st.surv_off.reset(); st.e_ht.reset();         // (a tile stage's arrays)
        } else {
            st.tile_rows = (k == 0) ? R0 : R1;
            st.n_tiles = ceil_div(st.n_entries, st.tile_rows);
        }
        sc.stages.push_back(std::move(st));
    }
    *built = true;
    *heights_done = early_heights;
    return RAHT_OK;                                       // (the blocks of stages that were not needed go back to the cache here)
}

static int build_schedule(raht_plan *plan, int R0, int R1, int Rf, hipStream_t s, Schedule **out);

// The kernels that fill a new schedule's arrays (heights, later the tile programs) are enqueued on the building stream and
// not waited for. A cached schedule handed to a caller on ANOTHER stream (raht_plan_set_concurrent_directions) first makes that
// stream wait for them.
int get_schedule(raht_plan *plan, int R0, int R1, int Rf, hipStream_t s, Schedule **out)
{
    for (auto &sc : plan->schedules)
        if (sc.tile_rows == R0 && sc.tail_rows == R1 && sc.final_rows == Rf) {
            if (sc.ready && sc.ready_on != s) RAHT_HIP_CHECK(hipStreamWaitEvent(s, sc.ready, 0));
            *out = &sc;
            return RAHT_OK;
        }
    RAHT_RET(build_schedule(plan, R0, R1, Rf, s, out));
    Schedule &sc = **out;
    if (!sc.ready) RAHT_HIP_CHECK(hipEventCreateWithFlags(&sc.ready.ev, hipEventDisableTiming));
    RAHT_HIP_CHECK(hipEventRecord(sc.ready, s));
    sc.ready_on = s;
    return RAHT_OK;
}

static int build_schedule(raht_plan *plan, int R0, int R1, int Rf, hipStream_t s, Schedule **out)
{
    if (R0 >= 64 && R1 >= 64 && Rf >= 1 && Rf <= RAHT_TOP_MAX_ROWS) {
        Schedule sc;
        sc.tile_rows = R0; sc.tail_rows = R1; sc.final_rows = Rf; sc.valid = true;
        bool built = false, heights_done = false;
        RAHT_RET(build_schedule_fast(plan, R0, R1, Rf, s, sc, &built, &heights_done));
        if (built) {
            const int rch = heights_done ? RAHT_OK : launch_stage_heights(plan, sc, s);
            if (rch != RAHT_OK) { free_schedule(sc); return rch; }
            plan->schedules.push_back(std::move(sc));
            *out = &plan->schedules.back();
            return RAHT_OK;
        }
    }
    return get_schedule_exact(plan, R0, R1, Rf, s, out);
}

static int get_schedule_exact(raht_plan *plan, int R0, int R1, int Rf, hipStream_t s, Schedule **out)
{
    Schedule sc;
    sc.tile_rows = R0;
    sc.tail_rows = R1;
    sc.final_rows = Rf;
    sc.valid = true;
    const int64_t N = plan->N;
    Scratch buf(sizeof(uint32_t) * (2 * (size_t)N + 1), s);
    if (!buf.ok()) return RAHT_ERR_NOMEM;
    uint32_t *flag = buf.as<uint32_t>(), *pos = flag + N, *dtotal = pos + N;
    DevBuf<uint32_t> rows;         // rows of the next stage (nullptr = identity)
    int64_t n = N;
    int rc = RAHT_OK;
    const int max_stages = std::max(1, plan->max_stages);
    for (int k = 0; k < max_stages; ++k) {
        const int R = (k == 0) ? R0 : R1;
        // the stage is the schedule's from its first block on: whichever way the loop is left, free_schedule finds it
        sc.stages.emplace_back();
        Stage &st = sc.stages.back();
        st.rows = std::move(rows);
        if (n <= Rf) {                                       // few entries left: the TOP stage finishes the tree
            rc = build_top_stage(plan, n, s, st);
            break;
        }
        st.n_entries = n;
        st.n_tiles = ceil_div(n, R);
        st.tile_rows = R;
        if (st.rows && gather_stage_meta(plan, st, s) != hipSuccess) { rc = RAHT_ERR_NOMEM; break; }
        hipLaunchKernelGGL(stage_survivor_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s,
                           st.rows, n, R, N, plan->wl, plan->wr, plan->lvl, plan->top_level, flag);
        rc = exclusive_scan_u32(flag, pos, n, dtotal, s);
        if (rc != RAHT_OK) break;
        uint32_t cnt32 = 0;
        rc = read_back_u32(&cnt32, dtotal, 1, nullptr, nullptr, 0, s);
        if (rc != RAHT_OK) break;
        const int64_t cnt = cnt32;
        const bool last = (cnt == plan->n_roots);            // only the roots are left: tree finished
        // no progress, or more stages than the plan allows. (With >= 64 rows per tile and <= 63 key bits a stage
        // always merges something -- the minimum-level entry of the first tile cannot reach past it, DESIGN.md
        // 4.2 -- so in practice only the stage limit, raht_plan_set_max_stages, ends up here.)
        if (!last && (cnt >= n || k == max_stages - 1)) { sc.valid = false; break; }
        if (st.surv_off.alloc((size_t)(st.n_tiles + 1)) != hipSuccess) { rc = RAHT_ERR_NOMEM; break; }
        hipLaunchKernelGGL(tile_start_kernel, dim3((unsigned)ceil_div(st.n_tiles + 1, 256)), dim3(256), 0, s,
                           pos, n, R, st.n_tiles, cnt32, st.surv_off);
        if (last) break;
        if (rows.alloc((size_t)cnt) != hipSuccess) { rc = RAHT_ERR_NOMEM; break; }
        hipLaunchKernelGGL(compact_scatter_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, st.rows,
                           flag, pos, rows, n);
        n = cnt;
    }
    hipError_t e = hipStreamSynchronize(s);
    if (rc == RAHT_OK && e != hipSuccess) rc = RAHT_ERR_HIP;
    if (rc != RAHT_OK) {
        free_schedule(sc);
        set_error("schedule build failed");
        return rc;
    }
    if (sc.valid) {
        rc = launch_stage_heights(plan, sc, s);
        if (rc != RAHT_OK) { free_schedule(sc); return rc; }
    }
    plan->schedules.push_back(std::move(sc));        // std::deque: earlier schedules keep their addresses
    *out = &plan->schedules.back();
    return RAHT_OK;
}

#ifdef RAHT_PHASE_CLOCKS
int read_phase_clocks_sched(unsigned long long *dst, int which, int n_blocks)
{
    RAHT_HIP_CHECK(hipDeviceSynchronize());
    RAHT_HIP_CHECK(hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_phase_clk_plan), sizeof(unsigned long long) * PL_CLK_SLOTS * (size_t)std::min(n_blocks, PL_CLK_BLOCKS),
                                       sizeof(unsigned long long) * PL_CLK_SLOTS * PL_CLK_BLOCKS * (size_t)which));
    return PL_CLK_SLOTS;
}
#endif

}  // namespace raht

extern "C" int raht_debug_height_stages_per_launch(int n)
{
    return raht::g_height_group.exchange((n >= 1 && n <= raht::HT_MAX_STAGES) ? n : raht::HT_MAX_STAGES);
}
