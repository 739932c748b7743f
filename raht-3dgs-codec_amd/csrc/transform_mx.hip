// transform_mx.hip -- MIXED-PRECISION fused RAHT kernels: float32 rows whose first `n_wide` channels are carried in float64.
//
// Why: the reference quantizes float64 coefficients (python/encode_3dgs.py:82-83 DTYPE = float64, :204 floor(Coeff / step + 0.5)).
// On a 59-column frame (python/voxelize_pc.py:155: columns 0-2 of PCvox are the voxel coordinates, 0 .. 2^J - 1) the xyz
// coefficients reach 1e6, so at step 0.01 the quotient exceeds 2^24 and no float32 pipeline can return the reference's integers
// there (round 3: up to 56 units off), while the 56 attribute columns are fine in float32. The all-float64 kernels return the
// reference's integers everywhere at half the throughput. Here ONE set of launches carries the wide-range columns in float64 --
// float32 input converted exactly, float64 butterflies with float64 a / b, IEEE double division by the float64 step -- and the
// other columns in float32, bit-identical to raht_fwd_quant / raht_dequant_inv.
//
// Tile layout. An LDS row is NCp 16-byte chunk places: NW2 = ceil(n_wide / 2) places of two doubles, then NF = ceil((D - n_wide) / 4)
// places of four floats (the last one = the 16 bytes that END the row, as in transform.hip). 59 channels, 3 wide: 2 + 14 = 16
// places = 256 bytes = one lane group of 16 with no idle lane. A lane owns one chunk place of a row for the whole kernel; the
// wide lanes take the float64 branch of every butterfly (v_fma_f64 issues at the rate of v_fma_f32 on this chip), the others the
// float32 branch. Rows travel HBM -> LDS with global_load_lds_dwordx4 as in the float32 kernels: the float chunks to their places,
// the row's first 16 bytes (the n_wide <= 4 wide channels, raw float32 / int32) into the wide area, where the lane that loaded
// them widens them in place once they have landed. The workspaces between stages hold LDS row images (16 NCp bytes per row), so
// the later stages and the top stage read and write whole chunks. Butterfly records carry a and b in float64 (24 bytes); the
// float32 lanes round them once, exactly as the float32 kernels round sqrt(w0 / (w0 + w1)).
//
// Replaces, on the wide columns, what raht_fwd_quant_f64 / raht_dequant_inv_f64 compute (same arithmetic, same order), and on the
// other columns what raht_fwd_quant / raht_dequant_inv compute. Reference: python/RAHT.py:252-336, python/iRAHT.py:40-114,
// python/encode_3dgs.py:204,210,215,261,267-268,274.
#include "raht_common.h"
#include "raht_device.h"
#include "tile_engine.h"
#include "tile_host.h"

#include <algorithm>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <vector>

namespace raht {

// Profiling build only (-DRAHT_PHASE_CLOCKS, tools/phase_clocks_mx.py): thread 0 of the first stage-0 workgroups stamps the
// shader clock at the phase boundaries of its tile.
#ifdef RAHT_PHASE_CLOCKS
constexpr int MX_CLK_TILES = 4096, MX_CLK_SLOTS = 12;
__device__ unsigned long long g_phase_clk_mx[MX_CLK_TILES][MX_CLK_SLOTS];
#define MX_STAMP(k) do { if (IDENT && threadIdx.x == 0 && tile_id < MX_CLK_TILES) g_phase_clk_mx[tile_id][k] = __builtin_readcyclecounter(); } while (0)
#else
#define MX_STAMP(k) do { } while (0)
#endif

constexpr int MX_MAX_WIDE = 4;          // the wide channels are the row's first 16 bytes
constexpr int MX_THREADS = 512;
constexpr int MX_TOP_THREADS = 1024;
constexpr int MX_TOP_SLOTS = RAHT_TOP_MAX_ROWS / MX_TOP_THREADS;

struct StepTableMX {
    StepTable f;                        // float32 steps of every channel ((float)step, what raht_fwd_quant would be given)
    double w[MX_MAX_WIDE];              // float64 steps of the wide channels
};

// (must match the carve-up in tile_body_mx)
static size_t tile_lds_bytes_mx(int R, int NF, int nwide)
{
    const size_t data = (size_t)R * NF * 16 + (((size_t)R * nwide * 8 + 15) & ~(size_t)15);   // float tile + wide tile (8 bytes per wide channel)
    const size_t meta = (size_t)R * (16 + 4 + 4);                             // a, b (float64) + operand slots; Q position
    const size_t surv = ((size_t)R * 2 + 15) & ~(size_t)15;
    return data + meta + surv;
}

// the wide parts of the workspaces a stage touches (a workspace row is stored as two dense arrays: the float places of every
// entry, then the wide places of every entry; TileArgs::in / out / wsn point at the float parts)
struct MxPtrs {
    const double *in_w;      // fwd, stages >= 1: wide part of ws_k (n_wide doubles per entry)
    double *out_w;           // inv, stages >= 1: wide part of ws_k
    double *wsn_w;           // wide part of ws_{k+1}
    double *root_w;          // last stage of a plan with root buffers: the roots' wide channels (n_wide doubles per root); their
                             // float channels go through TileArgs::root_buf (D floats per root, the wide columns' floats unspecified)
    const uint32_t *prog;    // the stage's tile programs (Stage::prog): prog_stride words per tile, a / b pairs at word prog_ab
    uint32_t prog_stride, prog_ab;
    int prog_compact;
};

// raht_fwd_quant_mixed_multi: k scalar steps, one output matrix each (the float32 entry's MultiQ, with the steps in float64: the
// wide channels divide by step[i], the float lanes by (float)step[i])
struct MxMultiQ {
    int k;
    uint32_t fast_div;                  // bit i: (float)step[i] within [2^-100, 2^100] (the single call's rule, raht_device.h: quantize_one)
    double step[MULTI_Q_MAX];
    int32_t *Q[MULTI_Q_MAX];
};

// ROOTS: last stage of a plan with root buffers (TileArgs::root_buf, MxPtrs::root_w): the roots' low-pass rows go to / come from
// the caller's buffers instead of Q. A kernel of its own (tile_kernel_mx_roots), so that every other launch runs the code it ran
// without them. MULTI (forward) and SQ (inverse, stage 0) are the fused driver-loop variants, each a kernel of its own as well
// (tile_kernel_mx_multi, tile_kernel_mx_sq): only their write-backs differ.
template <bool INV, bool IDENT, int SLOTS, bool ROOTS, bool MULTI = false, bool SQ = false>
__device__ __forceinline__ void tile_body_mx(const TileArgs<float> &A, const MxPtrs &P, const StepTableMX &ST, const int64_t tile_id,
                                             const MxMultiQ *MQ = nullptr)
{
    extern __shared__ __align__(16) unsigned char smem[];
    typedef RegChunk<float> V16;
    typedef RegChunk<double> W16;
    typedef RegChunk<int32_t> I16;
    const int R = A.R;
    const int tid0 = threadIdx.x;
    const int nthreads = blockDim.x, nwv = nthreads >> 6;
    const int nwide = A.nwide;                             // wide channels (1 .. 4): one double each per row of the wide tile
    const int lgw = nwide > 2 ? 2 : nwide - 1;             // log2(lanes per butterfly in the wide pass)
    const int Df = A.D;                                    // the float tile holds ALL D channels, laid out as in the float32 kernels
    const int Fp = A.Dp, NF = Fp >> 2;                     // float tile: row stride in floats, chunk places per row
    const int lg = A.lg, lr = 6 - A.lg;                    // 2^lg >= NF lanes per row
    const uint32_t NFm = ((1u << 20) + (uint32_t)NF - 1) / (uint32_t)NF;     // c / NF == (c * NFm) >> 20 for c < 2^15
    auto sync_lds = [&]() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };
    auto wait_landed = [&]() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); };

    // ---- LDS carve-up (must match tile_lds_bytes_mx) ----
    size_t off = 0;
    float *ftile = (float *)smem; off += (size_t)R * Fp * 4;              // float32 channels, NF places per row
    double *wd = (double *)(smem + off); off += ((size_t)R * nwide * 8 + 15) & ~(size_t)15;   // wide channels: nwide doubles per row
    W16 *rec_ab = (W16 *)(smem + off); off += (size_t)R * 16;             // butterfly records: a, b in float64 ...
    uint32_t *rec_pj = (uint32_t *)(smem + off); off += (size_t)R * 4;    // ... and the two operand slots (partner | own << 16)
    int32_t *sdst = (int32_t *)(smem + off); off += (size_t)R * 4;        // Q position | finalised here << 31
    uint16_t *ssurv = (uint16_t *)(smem + off);                           // survivor slots, in rank order

    // lane geometry of the row loops, as in the float32 kernels: lane c4 of a group of 2^lg works on float place fl = min(c4, NF - 1)
    // of one row (channels goff .. goff + 3; lanes past the last place shadow it: same reads, same writes). The lane of place 0
    // is the row's HEAD lane: the wide channels are the first n_wide <= 4 channels of its chunk, and in the write-backs it
    // substitutes their float64 results for what the float32 arithmetic made of them.
    auto lane_geom = [&](int tid, int &lane, int &wid, int &g, int &c4, int &fl, int &sp, int &goff, bool &head) {
        lane = tid & 63;
        wid = __builtin_amdgcn_readfirstlane(tid >> 6);
        g = lane >> lg;
        c4 = lane & ((1 << lg) - 1);
        fl = min(c4, NF - 1);
        head = c4 == 0;
        sp = fl;
        goff = min(fl * 4, Df - 4);
    };
    // The float32 steps of this lane's four channels. One step for all channels (ST.f.n == 1, the usual call) is a scalar kernel
    // argument: use_steps reads it where it is needed. A per-channel table is indexed by lane, i.e. fetched from the kernarg
    // segment with vector loads: fetch_steps issues them at kernel start, next to the program fetch (a round trip to memory every
    // tile sits through anyway), NOT behind the barrier in front of the first use, where all eight waves would sit through one
    // more. (Issued whatever ST.f.n is -- a single step's lanes all read the table's first 16 bytes, unused: a branch around
    // the loads ends in register copies where the paths join, and the compiler waits for the loads in front of those.)
    float my_step[4], my_rcp[4], tab_step[4];
    auto fetch_steps = [&](int place) {
        const int g0 = ST.f.n == 1 ? 0 : min(place * 4, Df - 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) tab_step[i] = ST.f.v[g0 + i];
    };
    auto use_steps = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            my_step[i] = ST.f.n == 1 ? ST.f.v[0] : tab_step[i];
            my_rcp[i] = refined_rcp(my_step[i]);
        }
    };

    int tid = tid0;
    asm volatile("" : "+v"(tid));
    int lane, wid, g, c4, fl, sp, goff; bool head;
    lane_geom(tid, lane, wid, g, c4, fl, sp, goff, head);
    const int64_t e0 = tile_id * R;
    const int nt = (int)min((int64_t)R, A.n_entries - e0);
    MX_STAMP(0);
    if constexpr (!MULTI) fetch_steps(fl);                 // (MULTI: one scalar step per output matrix, MxMultiQ)

    // ---- P0a. the tile's program (schedule.hip: tile_program_kernel; raht_common.h: Stage::prog), fetched first: every butterfly,
    // survivor and destination of this tile, resolved once per schedule. Each wave reads the height offsets into its lanes
    // (lane h: butterflies of height <= h), each thread the words of its slots.
    const uint32_t *pg = P.prog + (uint64_t)tile_id * P.prog_stride;
    const int end_v = ((const uint16_t *)pg)[lane];
    const int endm_v = lane ? ((const uint16_t *)pg)[lane - 1] : 0;
    uint32_t surv_raw = A.surv_off ? A.surv_off[tile_id + (tid0 & 1)] : 0u;   // (lane-dependent: see TileMeta::surv_raw)
    uint32_t m_rw[SLOTS], m_rec[SLOTS];
    W16 m_ab[SLOTS];
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
        const int j = tid0 + s * nthreads;
        m_rw[s] = 0; m_rec[s] = 0; m_ab[s].v[0] = 0.0; m_ab[s].v[1] = 0.0;
        if (j < nt) {
            m_rw[s] = pg[32 + j];
            m_rec[s] = pg[32 + R + j];
            if (!P.prog_compact) m_ab[s] = ((const W16 *)(pg + P.prog_ab))[j];
        }
    }
    // behind wait_landed(): what the compiler's own early loads fetched is there as well, and it is told so here -- else it waits for
    // them where they are first used, in the write-back, with a vmcnt(0) that also sits out the survivor stores just issued
    auto early_loads_landed = [&]() {
        asm volatile("" : "+v"(surv_raw));
        if constexpr (!MULTI) asm volatile("" : "+v"(tab_step[0]), "+v"(tab_step[1]), "+v"(tab_step[2]), "+v"(tab_step[3]));
    };
    // (a row is finalised in this tile when it merges here, or when this is the last stage and its low-pass row goes to Q)
    auto fin_of = [&](uint32_t rw) { return (rw >> 31) != 0 || (A.last_stage && !ROOTS); };
    auto write_dst = [&]() {
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            const int j = tid0 + s * nthreads;
            if (j < nt) sdst[j] = (int32_t)((m_rw[s] & 0x7fffffffu) | (fin_of(m_rw[s]) ? 0x80000000u : 0u));
        }
    };
    auto write_survivors = [&](uint32_t n_merged) {
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            const uint32_t k = (uint32_t)(tid0 + s * nthreads);
            if (k >= n_merged && k < (uint32_t)nt) ssurv[k - n_merged] = (uint16_t)m_rec[s];
        }
    };
    // record k -> LDS slot k (compact records: a, b from the extents, the expression pair_weights + RAHT.py:321-322 evaluate)
    auto write_records = [&](uint32_t n_merged) {
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            const uint32_t k = (uint32_t)(tid0 + s * nthreads);
            if (k < n_merged) {
                uint32_t pj = m_rec[s];
                W16 ab = m_ab[s];
                if (P.prog_compact) {
                    const uint32_t j = pj & 1023u, l = (pj >> 10) & 1023u, r = (pj >> 20) & 1023u;
                    const double w0 = (double)(int)l, w1 = (double)(int)r;
                    const double den = w0 + w1;
                    ab.v[0] = sqrt(w0 / den);
                    ab.v[1] = sqrt(w1 / den);
                    pj = (j - l) | (j << 16);
                }
                rec_ab[k] = ab;
                rec_pj[k] = pj;
            }
        }
    };

    // LDS-direct transfers, lane-linear: instruction `it` of a transfer fills LDS bytes [1024 it, 1024 it + 1024) of its region.
    //   contiguous: row images (both parts of a workspace row are stored as separate, dense arrays)
    //   caller rows (C / Q: 4-byte elements either way): the float places from channels n_wide + 4 ch .., and the row's first 16
    //   bytes -- the raw wide channels, widened in place by widen_row once landed -- into the row's first wide place
    auto load_linear = [&](const float *dst, int chunks, const float *src) {
        const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const void *)dst;
        for (int it = wid; (it << 6) < chunks; it += nwv) {
            const int c = (it << 6) + lane;
            if (c < chunks) glds16<0>(src + (uint32_t)c * 4u, lds0 + ((uint32_t)it << 10));
        }
    };
    auto load_caller_rows = [&](int rows, auto src) {
        const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const void *)ftile;
        const int total = rows * NF;
        for (int it = wid; (it << 6) < total; it += nwv) {
            const int c = (it << 6) + lane;
            const int jr = (int)(((uint32_t)c * NFm) >> 20), ch = c - jr * NF;
            if (c < total) { const void *a = src(jr, (uint32_t)min(ch * 4, Df - 4)); if (a) glds16<1>(a, lds0 + ((uint32_t)it << 10)); }
        }
    };
    // Widening of the wide channels a caller row arrived with (the first n_wide elements of its first float chunk): float32 ->
    // float64 into the wide tile. One ROW per thread, after the barrier behind which every wave's rows have landed. (The float
    // tile keeps those elements and carries them through its float32 butterflies like any other channel: the write-backs drop
    // what comes out of that.)
    auto widen_row = [&](int j) {
        double *row = wd + __mul24(j, nwide);
        const V16 raw = *(const V16 *)(ftile + __mul24(j, Fp));          // the row's first chunk, as it arrived
        double d[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) d[i] = i < nwide ? (double)raw.v[i] : 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) if (i < nwide) row[i] = d[i];
    };

    if constexpr (!INV) {
        // ---- P0b. this stage's rows ----
        if constexpr (IDENT) {
            const uint32_t ldc = (uint32_t)A.ld_in;
            const float *src = A.in + e0 * (int64_t)ldc;
            load_caller_rows(nt, [&](int jr, uint32_t go) { return row_at(src, (uint32_t)jr, ldc, go); });
        } else {
            load_linear(ftile, nt * NF, A.in + e0 * (int64_t)Fp);
            load_linear((const float *)wd, (nt * nwide + 1) >> 1, (const float *)(P.in_w + e0 * (int64_t)nwide));      // (16-byte chunks: may read one double past the tile's rows -- the next tile's, or the array's slack)
        }
        MX_STAMP(9);
        const uint32_t n_merged = (uint32_t)__builtin_amdgcn_readlane(end_v, 63);
        write_dst();
        write_survivors(n_merged);
        write_records(n_merged);
        MX_STAMP(1);
        wait_landed();                                                     // this wave's rows are in LDS
        early_loads_landed();
        sync_lds();                                                        // sync #1: every wave's rows, the records
        MX_STAMP(2);
        if constexpr (IDENT) {
#pragma unroll
            for (int s = 0; s < SLOTS; ++s) {
                const int j = tid + s * nthreads;
                if (j < nt) widen_row(j);
            }
            sync_lds();                                                    // sync #2
        }
        MX_STAMP(3);
        MX_STAMP(4);
    } else {
        const uint32_t n_merged = (uint32_t)__builtin_amdgcn_readlane(end_v, 63);
        write_dst();
        write_survivors(n_merged);
        MX_STAMP(1);
        sync_lds();                                                        // sync #1: destinations and survivor slots
        MX_STAMP(2);
        // ---- P0b. every finalised slot's quantized row (survivor rows come from the stage above and are not read from Q at all)
        load_caller_rows(nt, [&](int jr, uint32_t go) -> const void * {
            const uint32_t d = (uint32_t)sdst[jr];
            return (d >> 31) ? (const void *)row_far((const int32_t *)A.Q, d & 0x7fffffffu, (uint32_t)A.ldq, go) : nullptr; });
        write_records(n_merged);
        const uint32_t surv_base = (uint32_t)__builtin_amdgcn_readlane((int)surv_raw, 0);
        const uint32_t surv_cnt = (uint32_t)__builtin_amdgcn_readlane((int)surv_raw, 1) - surv_base;
        if (!A.last_stage) {
            // the survivors, from the stage above (row images) into their slots
            if (c4 < NF) for (uint32_t it = wid; (it << lr) < surv_cnt; it += nwv) {
                const uint32_t qc = min((it << lr) + g, surv_cnt - 1);
                const V16 x = ld_chunk<float>(row_at((const float *)A.wsn + (int64_t)surv_base * Fp, qc, (uint32_t)Fp, (uint32_t)(fl * 4)));
                *(V16 *)&ftile[__mul24((int)ssurv[qc], Fp) + fl * 4] = x;
            }
            for (uint32_t c = (uint32_t)tid; c < surv_cnt * (uint32_t)nwide; c += (uint32_t)nthreads) {
                const uint32_t qc = c / (uint32_t)nwide, i = c - qc * (uint32_t)nwide;
                wd[__mul24((int)ssurv[qc], nwide) + i] = P.wsn_w[(int64_t)surv_base * nwide + c];
            }
        } else if (ROOTS) {
            // last stage of a plan with root buffers (a truncated tree's top rows): the roots' low-pass rows come from the caller's
            // two buffers -- the float places at their channels in the float buffer (row stride D), the wide channels from the
            // float64 one -- instead of from Q
            if (c4 < NF) for (uint32_t it = wid; (it << lr) < surv_cnt; it += nwv) {
                const uint32_t qc = min((it << lr) + g, surv_cnt - 1);
                const V16 x = ld_chunk<float>(A.root_buf + (int64_t)(surv_base + qc) * Df + goff);
                *(V16 *)&ftile[__mul24((int)ssurv[qc], Fp) + fl * 4] = x;
            }
            for (uint32_t c = (uint32_t)tid; c < surv_cnt * (uint32_t)nwide; c += (uint32_t)nthreads) {
                const uint32_t qc = c / (uint32_t)nwide, i = c - qc * (uint32_t)nwide;
                wd[__mul24((int)ssurv[qc], nwide) + i] = P.root_w[(int64_t)surv_base * nwide + c];
            }
        }
        MX_STAMP(3);
        wait_landed();                                                     // this wave's Q rows are in LDS
        early_loads_landed();
        sync_lds();                                                        // sync #2: every row, every record
        MX_STAMP(4);
        use_steps();
        // the wide channels of the rows finalised here, from the raw integers that arrived with them (one ROW per thread)
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            const int j = tid0 + s * nthreads;
            if (j < nt && fin_of(m_rw[s])) {
                double *row = wd + __mul24(j, nwide);
                const I16 raw = *(const I16 *)(ftile + __mul24(j, Fp));
#pragma unroll
                for (int i = 0; i < 4; ++i) if (i < nwide) row[i] = (double)raw.v[i] * ST.w[i];
            }
        }
        if (A.last_stage && !ROOTS) {
            // roots finalised by a last TILE stage come straight from Q as well: dequantize them in place (no butterfly will; the
            // wide elements stay raw: the widening above reads them)
            const uint32_t n_fin = (uint32_t)nt - n_merged;
            if (c4 < NF) for (uint32_t it = wid; (it << lr) < n_fin; it += nwv) {
                const uint32_t qc = (it << lr) + g;
                if (qc < n_fin) {
                    V16 *pr = (V16 *)&ftile[__mul24((int)ssurv[qc], Fp) + fl * 4];
                    const I16 raw = *(const I16 *)pr;
                    V16 x;
#pragma unroll
                    for (int i = 0; i < 4; ++i)       // encode_3dgs.py:261
                        x.v[i] = (head && i < nwide) ? __int_as_float(raw.v[i]) : (float)raw.v[i] * my_step[i];
                    *pr = x;
                }
            }
        }
        sync_lds();                                                        // sync #3
    }
    MX_STAMP(5);
    // ---- P4. butterflies, one round per height present ----
    // The float32 channels run exactly as in the float32 kernels: a lane group per butterfly (head and idle lanes shadow the
    // group's last float lane: same reads, same writes, no exec-mask juggling). The wide channels of a level are a SEPARATE, dense
    // pass over their own LDS array -- a lane per (butterfly, channel), 16 to 64 butterflies per wave instruction -- on other waves.
    // Levels that fit one wave instruction (most: the chain of small levels needs no workgroup barrier, a wave's LDS operations
    // execute in order) are walked by wave 0 (float) and wave 1 (wide) side by side. (First version: one row array with the wide
    // places in front, the wide lanes taking a float64 branch inside every float butterfly instruction: both branches issued for
    // every instruction of every wave, and every same-place access of many 256-byte rows a bank conflict: LDS busy twice as long
    // as in the float32 kernel, rocprofv3 SQ_LDS_BANK_CONFLICT 39 M against 11 M cycles per launch.)
    {
        const uint32_t stride = (uint32_t)(nwv << lr);
        const uint32_t gw = (uint32_t)lane >> lgw, cw = (uint32_t)min(lane & ((1 << lgw) - 1), nwide - 1);   // (three channels: the group's 4th lane shadows the 3rd)
        const uint32_t bw = 64u >> lgw;                        // wide butterflies per wave instruction
        const uint32_t cf = (uint32_t)fl * 4u;
        bool chained = false;
        const int loff_v = endm_v, hist_v = end_v - endm_v;
        uint64_t mask = __ballot(hist_v > 0);
        while (mask) {
            const int l = INV ? (63 - __clzll((long long)mask)) : (__ffsll((long long)mask) - 1);
            mask &= ~(1ull << l);
            const uint32_t base = (uint32_t)__builtin_amdgcn_readlane(loff_v, l), cnt = (uint32_t)__builtin_amdgcn_readlane(hist_v, l);
            auto apply_f = [&](auto UC, uint32_t mb) {
                constexpr int U = decltype(UC)::value;
                W16 ab[U];
                uint32_t pj[U];
#pragma unroll
                for (int u = 0; u < U; ++u) { const uint32_t m = base + min(mb + u * stride + g, cnt - 1); pj[u] = rec_pj[m]; ab[u] = rec_ab[m]; }
                uint32_t ip[U], ij[U];
                V16 x0[U], x1[U];
#pragma unroll
                for (int u = 0; u < U; ++u) { ip[u] = __umul24(pj[u] & 0xffffu, (uint32_t)Fp) + cf; ij[u] = __umul24(pj[u] >> 16, (uint32_t)Fp) + cf; }
#pragma unroll
                for (int u = 0; u < U; ++u) { x0[u] = *(const V16 *)&ftile[ip[u]]; x1[u] = *(const V16 *)&ftile[ij[u]]; }
                if constexpr (INV) {                          // the high-pass operand is still the quantized integer (encode_3dgs.py:261)
#pragma unroll
                    for (int u = 0; u < U; ++u) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) x1[u].v[i] = (float)__float_as_int(x1[u].v[i]) * my_step[i];
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const float ca = (float)ab[u].v[0], cb = (float)ab[u].v[1];
                    V16 lo, hi;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        if (!INV) {                           // RAHT.py:331-332
                            lo.v[i] = ca * x0[u].v[i] + cb * x1[u].v[i];
                            hi.v[i] = ca * x1[u].v[i] - cb * x0[u].v[i];
                        } else {                              // iRAHT.py:108-109
                            lo.v[i] = ca * x0[u].v[i] - cb * x1[u].v[i];
                            hi.v[i] = cb * x0[u].v[i] + ca * x1[u].v[i];
                        }
                    }
                    if (u == 0 || mb + u * stride < cnt) { *(V16 *)&ftile[ip[u]] = lo; *(V16 *)&ftile[ij[u]] = hi; }
                }
            };
            auto pass_f = [&](auto UC) {
                constexpr int U = decltype(UC)::value;
                for (uint32_t mb = (uint32_t)(wid << lr); mb < cnt; mb += stride * U) apply_f(UC, mb);
            };
            // butterflies m0 + gw of this level, wide channels (lanes past the last one redo it in lockstep with its owner)
            auto apply_w = [&](uint32_t m0) {
                const uint32_t m = base + min(m0 + gw, cnt - 1);
                const uint32_t pj = rec_pj[m];
                const W16 ab = rec_ab[m];
                const uint32_t ip = __umul24(pj & 0xffffu, (uint32_t)nwide) + cw, ij = __umul24(pj >> 16, (uint32_t)nwide) + cw;
                const double d0 = wd[ip], d1 = wd[ij];
                const double ca = ab.v[0], cb = ab.v[1];
                double lo, hi;
                if (!INV) {                                   // RAHT.py:331-332
                    lo = ca * d0 + cb * d1;
                    hi = ca * d1 - cb * d0;
                } else {                                      // iRAHT.py:108-109
                    lo = ca * d0 - cb * d1;
                    hi = cb * d0 + ca * d1;
                }
                wd[ip] = lo; wd[ij] = hi;
            };
            if (cnt <= (1u << lr)) {
                if (wid == 0) pass_f(std::integral_constant<int, 1>());
                else if (wid == 1) { for (uint32_t m0 = 0; m0 < cnt; m0 += bw) apply_w(m0); }     // (narrow rows: a float instruction may hold more butterflies than a wide one)
                chained = true;
            } else {
                if (chained) { __syncthreads(); chained = false; }
                if (cnt <= stride) pass_f(std::integral_constant<int, 1>());
                else pass_f(std::integral_constant<int, TILE_ROUND_U>());
                for (uint32_t m0 = (uint32_t)(nwv - 1 - wid) * bw; m0 < cnt; m0 += (uint32_t)nwv * bw) apply_w(m0);   // from the last wave down
                __syncthreads();
            }
        }
        if (chained) __syncthreads();
    }

    MX_STAMP(6);
    // ---- P5. write back ----
    {
        int tid5 = tid0;
        asm volatile("" : "+v"(tid5));
        lane_geom(tid5, lane, wid, g, c4, fl, sp, goff, head);
    }
    const bool rowlane = c4 < NF;
    if constexpr (INV) {
        if constexpr (IDENT) {
            // stage 0 -> the caller's C rows [e0, e0 + nt). ONE store instruction writes a whole row: the float lanes their chunks,
            // the head lane the row's first 16 bytes -- the wide channels rounded to float32 and, behind them, the first
            // 4 - n_wide float channels once more (the same values their own lane stores). A row start written by a second,
            // narrower store instruction becomes a partial-line write of its own: the fused forward took 0.92 ms instead of
            // 0.31 ms that way (rows are 236 bytes: every line is shared by two rows)
            float *base = A.out + e0 * A.ld_out;
            // SQ (raht_dequant_inv_mixed_sqdiff): every row is also compared with A.ref on its way out, chunk for chunk -- the
            // head lane's chunk with the wide channels already rounded to float32 -- differences in float32, squares and sums in
            // float64 per lane; A.out == nullptr: nothing is stored
            double acc[4] = {0.0, 0.0, 0.0, 0.0};
            const float *rbase = SQ ? A.ref + e0 * A.ld_ref : nullptr;
            // Two row instructions per trip. The head lanes alone read their rows' wide results (clamped indices: no branch per
            // channel, all reads of a trip in flight together); what follows is branch-free -- selects, then ONE store instruction
            // per row group, pinned behind an empty asm so that the compiler cannot sink it into a head / non-head diamond again
            // (it did: the rows' first 16 bytes left as a second, narrow store instruction, i.e. a partial-line write per row, and
            // every wide channel was its own LDS round trip)
            if (rowlane) for (int it = wid; (it << lr) < nt; it += 2 * nwv) {
                int j[2]; V16 x[2]; double w[2][4] = {};
                V16 c[2];
                if constexpr (SQ) {
#pragma unroll
                    for (int u = 0; u < 2; ++u)
                        c[u] = ld_chunk<float, true>(row_at(rbase, (uint32_t)min(((it + u * nwv) << lr) + g, nt - 1), (uint32_t)A.ld_ref, (uint32_t)goff));
                }
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    j[u] = min(((it + u * nwv) << lr) + g, nt - 1);
                    x[u] = *(const V16 *)&ftile[__mul24(j[u], Fp) + sp * 4];
                }
                if (head) {
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) w[u][i] = wd[__mul24(j[u], nwide) + min(i, nwide - 1)];
                    }
                }
                asm volatile("" : "+v"(w[0][0]), "+v"(w[0][1]), "+v"(w[0][2]), "+v"(w[0][3]), "+v"(w[1][0]), "+v"(w[1][1]), "+v"(w[1][2]), "+v"(w[1][3]));
#pragma unroll
                for (int u = 0; u < 2; ++u) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) { const float f = (float)w[u][i]; x[u].v[i] = (head && i < nwide) ? f : x[u].v[i]; }
                    asm volatile("" : "+v"(x[u].v[0]), "+v"(x[u].v[1]), "+v"(x[u].v[2]), "+v"(x[u].v[3]));
                    if constexpr (SQ) {
                        if (u == 0 || ((it + nwv) << lr) < nt) {            // (wave-uniform)
                            if (A.out) st_chunk<float, true>(row_at(base, (uint32_t)j[u], (uint32_t)A.ld_out, (uint32_t)goff), x[u]);
                            if (((it + u * nwv) << lr) + g < nt) {
#pragma unroll
                                for (int i = 0; i < 4; ++i) { const float d = x[u].v[i] - c[u].v[i]; acc[i] += (double)d * (double)d; }
                            }
                        }
                    } else if (u == 0 || ((it + nwv) << lr) < nt) {         // (wave-uniform)
                        st_chunk<float, true>(row_at(base, (uint32_t)j[u], (uint32_t)A.ld_out, (uint32_t)goff), x[u]);
                    }
                }
            }
            if constexpr (SQ) {
                // per tile, in a fixed order: a chunk place's lanes across the wave's row groups (shuffles), then the waves (LDS)
                // -> one float64 per float place element in sq_part (the element layout sq_final_kernel reads: 4 NF per tile)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    for (int sh = 1 << lg; sh < 64; sh <<= 1) acc[i] += __shfl_xor(acc[i], sh, 64);
                }
                __syncthreads();                                                  // every wave has read its rows: the tile's LDS is free
                double *sacc = (double *)smem;                                    // [nwv][4 NF]
                if (g == 0 && rowlane) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) sacc[(wid * NF + c4) * 4 + i] = acc[i];
                }
                __syncthreads();
                if (tid0 < NF * 4) {
                    double t = 0.0;
                    for (int w = 0; w < nwv; ++w) t += sacc[w * NF * 4 + tid0];
                    A.sq_part[tile_id * (NF * 4) + tid0] = t;
                }
            }
        } else {
            // stage k -> ws_k: both parts are contiguous runs of chunks
            float *bf = A.out + e0 * (int64_t)Fp;
            double *bw_ = P.out_w + e0 * (int64_t)nwide;
            for (int c = tid; c < nt * NF; c += nthreads) st_chunk<float>(bf + c * 4, *(const V16 *)&ftile[c * 4]);
            for (int c = tid; c < nt * nwide; c += nthreads) bw_[c] = wd[c];
        }
    } else {
        // survivors, compacted, to the next stage's workspace (row images, two dense arrays); last stage of a plan with root
        // buffers: the roots to the caller's two buffers (float: row stride D, each place at its channels; wide: n_wide doubles)
        if (!A.last_stage || ROOTS) {
            const uint32_t surv_base = (uint32_t)__builtin_amdgcn_readlane((int)surv_raw, 0);
            const uint32_t surv_cnt = (uint32_t)__builtin_amdgcn_readlane((int)surv_raw, 1) - surv_base;
            constexpr bool to_roots = ROOTS;
            float *bf = to_roots ? A.root_buf + (int64_t)surv_base * Df : A.wsn + (int64_t)surv_base * Fp;
            double *bw_ = (to_roots ? P.root_w : P.wsn_w) + (int64_t)surv_base * nwide;
            const uint32_t ldb = (uint32_t)(to_roots ? Df : Fp), cb = (uint32_t)(to_roots ? goff : fl * 4);
            if (c4 < NF) for (uint32_t it = wid; (it << lr) < surv_cnt; it += nwv) {
                const uint32_t q = min((it << lr) + g, surv_cnt - 1);
                const V16 x = *(const V16 *)&ftile[__mul24((int)ssurv[q], Fp) + fl * 4];
                st_chunk<float>(row_at(bf, q, ldb, cb), x);
            }
            for (uint32_t c = (uint32_t)tid; c < surv_cnt * (uint32_t)nwide; c += (uint32_t)nthreads) {
                const uint32_t q = c / (uint32_t)nwide, i = c - q * (uint32_t)nwide;
                bw_[c] = wd[__mul24((int)ssurv[q], nwide) + i];
            }
        }
        if constexpr (MULTI) {
            // raht_fwd_quant_mixed_multi: the write-back below ((a), then (b)) once per step. The wide doubles must outlive every
            // quantization, so the integers of step kk go to an area of their own: the butterfly records' (16 bytes per row >=
            // n_wide int32), free since the last butterfly round. One barrier after (a) -- (b) reads other threads' rows -- and
            // one after (b), before the next step's (a) overwrites the area.
            int32_t *qa = (int32_t *)rec_ab;
            auto store_step = [&](auto fast_div, int32_t *Qd) {
                if (rowlane) for (int it = wid; (it << lr) < nt; it += 2 * nwv) {
                    int jc[2]; V16 x[2]; I16 qi[2] = {}; uint32_t dv[2];
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        jc[u] = min(((it + u * nwv) << lr) + g, nt - 1);
                        x[u] = *(const V16 *)&ftile[__mul24(jc[u], Fp) + sp * 4];
                        dv[u] = (uint32_t)sdst[jc[u]];
                    }
                    if (head) {
#pragma unroll
                        for (int u = 0; u < 2; ++u) {
#pragma unroll
                            for (int i = 0; i < 4; ++i) qi[u].v[i] = qa[__mul24(jc[u], nwide) + min(i, nwide - 1)];
                        }
                    }
                    asm volatile("" : "+v"(x[0].v[0]), "+v"(x[1].v[0]), "+v"(qi[0].v[0]), "+v"(qi[0].v[1]), "+v"(qi[0].v[2]), "+v"(qi[0].v[3]),
                                 "+v"(qi[1].v[0]), "+v"(qi[1].v[1]), "+v"(qi[1].v[2]), "+v"(qi[1].v[3]));
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        I16 qv;
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int32_t q = quantize_one(x[u].v[i], my_step[i], my_rcp[i], decltype(fast_div)::value);
                            qv.v[i] = (head && i < nwide) ? qi[u].v[i] : q;
                        }
                        asm volatile("" : "+v"(qv.v[0]), "+v"(qv.v[1]), "+v"(qv.v[2]), "+v"(qv.v[3]));
                        if ((dv[u] >> 31) && (u == 0 || ((it + nwv) << lr) < nt))
                            st_chunk<int32_t, true>(row_far(Qd, dv[u] & 0x7fffffffu, (uint32_t)A.ldq, (uint32_t)goff), qv);
                    }
                }
            };
            for (int kk = 0; kk < MQ->k; ++kk) {
                const double sw = MQ->step[kk];
#pragma unroll
                for (int s = 0; s < SLOTS; ++s) {
                    const int j = tid0 + s * nthreads;
                    if (j < nt && ((uint32_t)sdst[j] >> 31)) {
                        const double *row = &wd[__mul24(j, nwide)];
                        int32_t *qrow = &qa[__mul24(j, nwide)];
#pragma unroll
                        for (int i = 0; i < 4; ++i) if (i < nwide) qrow[i] = quantize_one_f64(row[i], sw);
                    }
                }
                sync_lds();
                const float sf = (float)sw, rf = refined_rcp(sf);
#pragma unroll
                for (int i = 0; i < 4; ++i) { my_step[i] = sf; my_rcp[i] = rf; }
                if ((MQ->fast_div >> kk) & 1u) store_step(std::true_type(), MQ->Q[kk]);
                else store_step(std::false_type(), MQ->Q[kk]);
                sync_lds();
            }
        } else {
            // rows finalised here, quantized to Q[inv_order[row]] (encode_3dgs.py:204,210,215).
            // (a) the wide channels: one ROW per thread -- the IEEE double division is ~40 instructions a channel, so it runs on
            //     whole waves of rows -- and the integers go back into the row's first wide place (a row finalised here is nobody's
            //     survivor)
            MX_STAMP(10);
#pragma unroll
            for (int s = 0; s < SLOTS; ++s) {
                const int j = tid0 + s * nthreads;
                if (j < nt && ((uint32_t)sdst[j] >> 31)) {
                    double *row = &wd[__mul24(j, nwide)];
                    double d[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                    for (int i = 0; i < 4; ++i) if (i < nwide) d[i] = row[i];
                    asm volatile("" ::: "memory");                // (the integers go over the doubles they were made of: every read is above)
                    int32_t *qrow = (int32_t *)row;
#pragma unroll
                    for (int i = 0; i < 4; ++i) if (i < nwide) qrow[i] = quantize_one_f64(d[i], ST.w[i]);
                }
            }
            sync_lds();
            MX_STAMP(7);
            // (b) ONE store instruction per row group writes whole rows of Q: the float lanes their quantized chunks, the head lane the
            //     row's first 16 bytes = the wide integers and, behind them, the first 4 - n_wide float channels quantized once more
            //     (same values as their own lane's). See the inverse's write-back for why.
            use_steps();                                           // (sp == fl: the places fetch_steps fetched)
#ifdef RAHT_PHASE_CLOCKS
            asm volatile("" :: "v"(my_step[0]), "v"(my_rcp[3]));
#endif
            MX_STAMP(11);
            auto store_final = [&](auto fast_div) {
                if (rowlane) for (int it = wid; (it << lr) < nt; it += 2 * nwv) {
                    int jc[2]; V16 x[2]; I16 qi[2] = {}; uint32_t dv[2];
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        jc[u] = min(((it + u * nwv) << lr) + g, nt - 1);
                        x[u] = *(const V16 *)&ftile[__mul24(jc[u], Fp) + sp * 4];
                        dv[u] = (uint32_t)sdst[jc[u]];
                    }
                    if (head) {                                   // (only the head lanes; clamped indices: no branch per channel)
#pragma unroll
                        for (int u = 0; u < 2; ++u) {
                            const int32_t *qrow = (const int32_t *)&wd[__mul24(jc[u], nwide)];
#pragma unroll
                            for (int i = 0; i < 4; ++i) qi[u].v[i] = qrow[min(i, nwide - 1)];
                        }
                    }
                    asm volatile("" : "+v"(x[0].v[0]), "+v"(x[1].v[0]), "+v"(qi[0].v[0]), "+v"(qi[0].v[1]), "+v"(qi[0].v[2]), "+v"(qi[0].v[3]),
                                 "+v"(qi[1].v[0]), "+v"(qi[1].v[1]), "+v"(qi[1].v[2]), "+v"(qi[1].v[3]));
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        // branch-free up to ONE store instruction per row group (see the inverse's write-back)
                        I16 qv;
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int32_t q = quantize_one(x[u].v[i], my_step[i], my_rcp[i], decltype(fast_div)::value);
                            qv.v[i] = (head && i < nwide) ? qi[u].v[i] : q;
                        }
                        asm volatile("" : "+v"(qv.v[0]), "+v"(qv.v[1]), "+v"(qv.v[2]), "+v"(qv.v[3]));
                        if ((dv[u] >> 31) && (u == 0 || ((it + nwv) << lr) < nt))
                            st_chunk<int32_t, true>(row_far(A.Q, dv[u] & 0x7fffffffu, (uint32_t)A.ldq, (uint32_t)goff), qv);
                    }
                }
            };
            if (ST.f.fast_div) store_final(std::true_type()); else store_final(std::false_type());
        }
    }
    MX_STAMP(8);
}

template <bool INV, bool IDENT, int SLOTS>
__global__ __launch_bounds__(MX_THREADS, 6) void tile_kernel_mx(const TileArgs<float> A, const MxPtrs P, const StepTableMX ST)
{
    tile_body_mx<INV, IDENT, SLOTS, false>(A, P, ST, (int64_t)blockIdx.x);
}
// the last stage of a plan with root buffers
template <bool INV, bool IDENT, int SLOTS>
__global__ __launch_bounds__(MX_THREADS, 6) void tile_kernel_mx_roots(const TileArgs<float> A, const MxPtrs P, const StepTableMX ST)
{
    tile_body_mx<INV, IDENT, SLOTS, true>(A, P, ST, (int64_t)blockIdx.x);
}
// raht_fwd_quant_mixed_multi: every stage of the forward, k quantizations per finalised row
template <bool IDENT, int SLOTS>
__global__ __launch_bounds__(MX_THREADS, 6) void tile_kernel_mx_multi(const TileArgs<float> A, const MxPtrs P, const StepTableMX ST, const MxMultiQ M)
{
    tile_body_mx<false, IDENT, SLOTS, false, true, false>(A, P, ST, (int64_t)blockIdx.x, &M);
}
// raht_dequant_inv_mixed_sqdiff: stage 0 of the inverse, comparing its rows with TileArgs::ref on the way out
template <int SLOTS>
__global__ __launch_bounds__(MX_THREADS, 6) void tile_kernel_mx_sq(const TileArgs<float> A, const MxPtrs P, const StepTableMX ST)
{
    tile_body_mx<true, true, SLOTS, false, false, true>(A, P, ST, (int64_t)blockIdx.x);
}

// Several scenes, one launch (raht_fwd_quant_mixed_batch / raht_dequant_inv_mixed_batch): the same stage of up to BATCH_MAX
// scenes, as tile_kernel_batch does for the float32 engine (transform.hip). first_tile[q] = number of tiles of the scenes before q;
// a workgroup finds its scene with scalar compares on blockIdx.x and runs ONE tile of it through tile_body_mx, reading that
// scene's arguments where they lie in the kernarg segment (a scalar offset, no private copy of the struct).
struct TileBatchMX {
    TileArgs<float> a[BATCH_MAX];
    MxPtrs p[BATCH_MAX];
    uint32_t first_tile[BATCH_MAX + 1];
    int n;
};
static_assert(sizeof(TileBatchMX) + sizeof(StepTableMX) <= 4096, "tile_kernel_mx_batch: arguments exceed the 4 KB kernarg segment");

template <bool INV, bool IDENT, int SLOTS>
__global__ __launch_bounds__(MX_THREADS, 6) void tile_kernel_mx_batch(const TileBatchMX B, const StepTableMX ST)
{
    int s = 0;
#pragma unroll
    for (int q = 1; q < BATCH_MAX; ++q) s += (q < B.n && blockIdx.x >= B.first_tile[q]) ? 1 : 0;
    tile_body_mx<INV, IDENT, SLOTS, false>(B.a[s], B.p[s], ST, (int64_t)(blockIdx.x - B.first_tile[s]));
}

// ------------------------------------------------------------------------------------------------
// TOP stage, mixed: one workgroup per chunk place keeps that place of ALL entries in LDS (transform.hip: top_kernel);
// workgroups [0, NW2) run the float64 instantiation on the wide places, the others the float32 one.
// ------------------------------------------------------------------------------------------------
struct TopArgsMX {
    const float *in_rows;  int64_t ld_in;    // fwd, single-stage schedule: the caller's C rows (entry = row)
    const float *in_img; const double *in_img_w;   // fwd, later stage: workspace row images, entry order (float places; n_wide doubles)
    float *out_rows;       int64_t ld_out;   // inv, single-stage schedule: the caller's C rows
    float *out_img; double *out_img_w;       // inv, later stage: workspace row images
    int32_t *Q;            int64_t ldq;
    const uint32_t *e_pos;                   // entry -> position in Q
    const uint32_t *pj;                      // butterflies sorted by level: partner entry | own entry << 16
    const float *ab32;  const double *ab64;  // a, b per butterfly
    int n, n_merges, D, nwide, Fp;           // Fp: floats per row of the float part of an image
    const uint32_t *lev;
    int nlev, nbig;
    uint32_t small_start;
    const uint32_t *root_rank;               // entry -> row of the root buffers (~0u: not a root)
    float *root_f; double *root_w;           // the caller's root buffers (n_roots x D floats, n_roots x n_wide doubles), or nullptr
};

template <bool WIDE, bool INV, bool ROOTS, bool MULTI = false>
__device__ __forceinline__ void top_body_mx(const TopArgsMX &A, const StepTableMX &ST, const int chunk, const MxMultiQ *MQ = nullptr)
{
    typedef typename std::conditional<WIDE, double, float>::type T;
    constexpr int VN = WIDE ? 2 : 4;
    typedef RegChunk<T> V16;
    extern __shared__ __align__(16) unsigned char smem[];
    V16 *tile = (V16 *)smem;
    __shared__ uint32_t s_lev[2 * 64];
    const int tid = threadIdx.x;
    const int nwide = A.nwide;
    const int goff = WIDE ? 2 * chunk : min(chunk * 4, A.D - 4);            // first channel of this chunk in the caller's rows
    // (float chunk 0 holds the wide channels too, as float32 ballast: it never writes them to Q / C -- the wide workgroups do)
    const int ioff = chunk * 4;                                              // a float chunk's place in a row image (floats)
    const int n = A.n, nm = A.n_merges;
    if (tid < 2 * A.nlev) s_lev[tid] = A.lev[tid];
    const T *ab = WIDE ? (const T *)A.ab64 : (const T *)A.ab32;
    const int n_small = nm - (int)A.small_start;
    uint32_t *s_pj = (uint32_t *)(smem + (size_t)n * 16);
    T *s_ab = (T *)(s_pj + ((n_small + 3) & ~3));
    for (int i = tid; i < n_small; i += MX_TOP_THREADS) {
        s_pj[i] = A.pj[A.small_start + i];
        s_ab[2 * i] = ab[2 * (A.small_start + i)];
        s_ab[2 * i + 1] = ab[2 * (A.small_start + i) + 1];
    }
    T my_step[VN];
    float my_rcp[VN];
    bool live[VN];                                         // wide: channel goff + i exists
#pragma unroll
    for (int i = 0; i < VN; ++i) {
        if constexpr (WIDE) { live[i] = goff + i < nwide; my_step[i] = live[i] ? ST.w[goff + i] : 1.0; my_rcp[i] = 1.0f; }
        else { live[i] = !(chunk == 0 && i < nwide); my_step[i] = ST.f.v[ST.f.n == 1 ? 0 : goff + i]; my_rcp[i] = refined_rcp(my_step[i]); }
    }
    uint32_t pj[MX_TOP_SLOTS];
    T ra[MX_TOP_SLOTS], rb[MX_TOP_SLOTS];
#pragma unroll
    for (int k = 0; k < MX_TOP_SLOTS; ++k) {
        const int idx = min(k * MX_TOP_THREADS + tid, max(nm - 1, 0));
        pj[k] = A.pj[idx]; ra[k] = ab[2 * idx]; rb[k] = ab[2 * idx + 1];
    }
    uint32_t m_dst[MX_TOP_SLOTS], m_rr[MX_TOP_SLOTS];
#pragma unroll
    for (int k = 0; k < MX_TOP_SLOTS; ++k) {
        m_dst[k] = A.e_pos[min(k * MX_TOP_THREADS + tid, n - 1)];
        m_rr[k] = ROOTS ? A.root_rank[min(k * MX_TOP_THREADS + tid, n - 1)] : 0xffffffffu;
    }
    // the entries
#pragma unroll
    for (int k = 0; k < MX_TOP_SLOTS; ++k) {
        const int e = k * MX_TOP_THREADS + tid;
        if (e >= n) continue;
        V16 v;
        if constexpr (!INV) {
            if (A.in_img) {
                if constexpr (WIDE) {
#pragma unroll
                    for (int i = 0; i < VN; ++i) v.v[i] = live[i] ? A.in_img_w[(int64_t)e * nwide + goff + i] : 0.0;
                } else {
                    v = *(const V16 *)(A.in_img + (int64_t)e * A.Fp + ioff);
                }
            } else if constexpr (WIDE) {
#pragma unroll
                for (int i = 0; i < VN; ++i) v.v[i] = live[i] ? (double)A.in_rows[(int64_t)e * A.ld_in + goff + i] : 0.0;
            } else {
                v = ld_chunk<float>(A.in_rows + (int64_t)e * A.ld_in + goff);
            }
        } else if (m_rr[k] != 0xffffffffu) {                // a root: its low-pass row from the caller's root buffers
            if constexpr (WIDE) {
#pragma unroll
                for (int i = 0; i < VN; ++i) v.v[i] = live[i] ? A.root_w[(int64_t)m_rr[k] * nwide + goff + i] : 0.0;
            } else {
                v = ld_chunk<float>(A.root_f + (int64_t)m_rr[k] * A.D + goff);
            }
        } else {
            const int32_t *q = A.Q + (int64_t)m_dst[k] * A.ldq + goff;
            if constexpr (WIDE) {
#pragma unroll
                for (int i = 0; i < VN; ++i) v.v[i] = live[i] ? (double)q[i] * my_step[i] : 0.0;        // encode_3dgs.py:261
            } else {
                const RegChunk<int32_t> raw = ld_chunk<int32_t>(q);
#pragma unroll
                for (int i = 0; i < VN; ++i) v.v[i] = (float)raw.v[i] * my_step[i];
            }
        }
        tile[e] = v;
    }
    __syncthreads();

    auto butterfly = [&](uint32_t rec, T a, T b) {
        const uint32_t ip = rec & 0xffffu, ij = rec >> 16;
        const V16 x0 = tile[ip], x1 = tile[ij];
        V16 vlo, vhi;
#pragma unroll
        for (int i = 0; i < VN; ++i) {
            if (!INV) {                                   // RAHT.py:331-332
                vlo.v[i] = a * x0.v[i] + b * x1.v[i];
                vhi.v[i] = a * x1.v[i] - b * x0.v[i];
            } else {                                      // iRAHT.py:108-109
                vlo.v[i] = a * x0.v[i] - b * x1.v[i];
                vhi.v[i] = b * x0.v[i] + a * x1.v[i];
            }
        }
        tile[ip] = vlo; tile[ij] = vhi;
    };
    auto big_levels = [&]() {
#pragma unroll 1
        for (int q = 0; q < A.nbig; ++q) {
            const int li = INV ? A.nbig - 1 - q : q;
            const uint32_t lo = s_lev[2 * li], hi = s_lev[2 * li + 1];
#pragma unroll
            for (int k = 0; k < MX_TOP_SLOTS; ++k) {
                const uint32_t idx = (uint32_t)(k * MX_TOP_THREADS + tid);
                if ((uint32_t)(k * MX_TOP_THREADS) < hi && (uint32_t)((k + 1) * MX_TOP_THREADS) > lo && idx >= lo && idx < hi)
                    butterfly(pj[k], ra[k], rb[k]);
            }
            __syncthreads();
        }
    };
    auto small_levels = [&]() {
        if (tid < 64) {
#pragma unroll 1
            for (int q = A.nbig; q < A.nlev; ++q) {
                const int li = INV ? A.nlev - 1 - (q - A.nbig) : q;
                const uint32_t lo = s_lev[2 * li], hi = s_lev[2 * li + 1];
                const uint32_t i = lo - A.small_start + (uint32_t)tid;
                if (lo + (uint32_t)tid < hi) butterfly(s_pj[i], s_ab[2 * i], s_ab[2 * i + 1]);
            }
        }
        __syncthreads();
    };
    if (!INV) { big_levels(); small_levels(); }
    else { small_levels(); big_levels(); }

#pragma unroll
    for (int k = 0; k < MX_TOP_SLOTS; ++k) {
        const int e = k * MX_TOP_THREADS + tid;
        if (e >= n) continue;
        const V16 v = tile[e];
        if constexpr (INV) {
            if (A.out_img) {
                if constexpr (WIDE) {
#pragma unroll
                    for (int i = 0; i < VN; ++i) if (live[i]) A.out_img_w[(int64_t)e * nwide + goff + i] = v.v[i];
                } else {
                    *(V16 *)(A.out_img + (int64_t)e * A.Fp + ioff) = v;
                }
            } else if constexpr (WIDE) {
#pragma unroll
                for (int i = 0; i < VN; ++i) if (live[i]) A.out_rows[(int64_t)e * A.ld_out + goff + i] = (float)v.v[i];
            } else if (chunk == 0) {
#pragma unroll
                for (int i = 0; i < VN; ++i) if (live[i]) A.out_rows[(int64_t)e * A.ld_out + goff + i] = v.v[i];
            } else {
                st_chunk<float>(A.out_rows + (int64_t)e * A.ld_out + goff, v);
            }
        } else if (m_rr[k] != 0xffffffffu) {                // a root: still a low-pass value, the caller's top stage takes it
            if constexpr (WIDE) {
#pragma unroll
                for (int i = 0; i < VN; ++i) if (live[i]) A.root_w[(int64_t)m_rr[k] * nwide + goff + i] = v.v[i];
            } else {
                st_chunk<float>(A.root_f + (int64_t)m_rr[k] * A.D + goff, v);
            }
        } else if constexpr (MULTI) {
            // raht_fwd_quant_mixed_multi: one quantization per step, each into its own matrix
            for (int kk = 0; kk < MQ->k; ++kk) {
                int32_t *q = MQ->Q[kk] + (int64_t)m_dst[k] * A.ldq + goff;
                if constexpr (WIDE) {
#pragma unroll
                    for (int i = 0; i < VN; ++i) if (live[i]) q[i] = quantize_one_f64(v.v[i], MQ->step[kk]);
                } else {
                    const float sf = (float)MQ->step[kk], rf = refined_rcp(sf);
                    const int fd = (int)((MQ->fast_div >> kk) & 1u);
                    RegChunk<int32_t> qv;
#pragma unroll
                    for (int i = 0; i < VN; ++i) qv.v[i] = quantize_one(v.v[i], sf, rf, fd);
                    if (chunk == 0) {
#pragma unroll
                        for (int i = 0; i < VN; ++i) if (live[i]) q[i] = qv.v[i];
                    } else {
                        st_chunk<int32_t>(q, qv);
                    }
                }
            }
        } else {
            int32_t *q = A.Q + (int64_t)m_dst[k] * A.ldq + goff;
            if constexpr (WIDE) {
#pragma unroll
                for (int i = 0; i < VN; ++i) if (live[i]) q[i] = quantize_one_f64(v.v[i], my_step[i]);
            } else {
                RegChunk<int32_t> qv;
#pragma unroll
                for (int i = 0; i < VN; ++i) qv.v[i] = quantize_one(v.v[i], my_step[i], my_rcp[i], ST.f.fast_div);
                if (chunk == 0) {
#pragma unroll
                    for (int i = 0; i < VN; ++i) if (live[i]) q[i] = qv.v[i];
                } else {
                    st_chunk<int32_t>(q, qv);
                }
            }
        }
    }
}

template <bool INV>
__global__ __launch_bounds__(MX_TOP_THREADS) void top_kernel_mx(const TopArgsMX A, const StepTableMX ST)
{
    const int NW2 = (A.nwide + 1) >> 1;
    if ((int)blockIdx.x < NW2) top_body_mx<true, INV, false>(A, ST, (int)blockIdx.x);
    else top_body_mx<false, INV, false>(A, ST, (int)blockIdx.x - NW2);
}
// a plan with root buffers (a separate kernel, as for the tile stages)
template <bool INV>
__global__ __launch_bounds__(MX_TOP_THREADS) void top_kernel_mx_roots(const TopArgsMX A, const StepTableMX ST)
{
    const int NW2 = (A.nwide + 1) >> 1;
    if ((int)blockIdx.x < NW2) top_body_mx<true, INV, true>(A, ST, (int)blockIdx.x);
    else top_body_mx<false, INV, true>(A, ST, (int)blockIdx.x - NW2);
}

// the top stages of several scenes in one launch (the mixed batch entries): blockIdx.y = scene, blockIdx.x = chunk place
struct TopBatchMX { TopArgsMX a[BATCH_MAX]; };
static_assert(sizeof(TopBatchMX) + sizeof(StepTableMX) <= 4096, "top_kernel_mx_batch: arguments exceed the 4 KB kernarg segment");

template <bool INV>
__global__ __launch_bounds__(MX_TOP_THREADS) void top_kernel_mx_batch(const TopBatchMX B, const StepTableMX ST)
{
    const TopArgsMX &A = B.a[blockIdx.y];
    const int NW2 = (A.nwide + 1) >> 1;
    if ((int)blockIdx.x < NW2) top_body_mx<true, INV, false>(A, ST, (int)blockIdx.x);
    else top_body_mx<false, INV, false>(A, ST, (int)blockIdx.x - NW2);
}

// raht_fwd_quant_mixed_multi (plans without root buffers)
__global__ __launch_bounds__(MX_TOP_THREADS) void top_kernel_mx_multi(const TopArgsMX A, const StepTableMX ST, const MxMultiQ M)
{
    const int NW2 = (A.nwide + 1) >> 1;
    if ((int)blockIdx.x < NW2) top_body_mx<true, false, false, true>(A, ST, (int)blockIdx.x, &M);
    else top_body_mx<false, false, false, true>(A, ST, (int)blockIdx.x - NW2, &M);
}

// the wide columns of caller rows <-> a compact float64 matrix (fallback path only)
__global__ void mx_cols_to_f64_kernel(const float *__restrict__ C, int64_t ldc, int64_t N, int nwide, double *__restrict__ W)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N * nwide) return;
    const int64_t i = e / nwide;
    W[e] = (double)C[i * ldc + (e - i * nwide)];
}
__global__ void mx_cols_from_f64_kernel(const double *__restrict__ W, int64_t N, int nwide, float *__restrict__ C, int64_t ldc)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N * nwide) return;
    const int64_t i = e / nwide;
    C[i * ldc + (e - i * nwide)] = (float)W[e];
}

// ---- host side -------------------------------------------------------------------------------------------------------
struct MxGeom {
    int nwide = 0, NCp = 0, Dp = 0, lg = 0;     // NCp: chunk places per row (wide + float); Dp: floats per row of the float tile
    int R0 = 0, R1 = 0, Rf = 0;
};

// Chunk places and tile rows for (D, n_wide). false: the mixed tile kernels do not cover this shape (fallback).
static bool mx_geometry(const raht_plan *p, int D, int nwide, MxGeom &g)
{
    // D - 4 >= n_wide: the row's LAST 16-byte chunk (channels [D - 4, D), which overlaps its neighbour when D % 4 != 0) must not
    // reach into the wide channels, whose float32 copies are ballast that only the first chunk's lane knows to replace
    if (D - 4 < nwide || D > 64 + MX_MAX_WIDE) return false;
    g.nwide = nwide;
    const int NF = (D + 3) / 4;                           // float places: ALL D channels, the float32 kernels' row layout
    g.NCp = (nwide + 1) / 2 + NF;
    g.Dp = NF * 4;
    g.lg = 0;
    while ((1 << g.lg) < NF) ++g.lg;
    int r1 = 0, dc1 = 0;
    pick_tail_geometry(p, 4, D, 512, &r1, &dc1, &g.Rf);
    const size_t budget = (size_t)42 * 1280;              // three workgroups per CU
    auto fit = [&](int hi, bool ident, size_t cap) {
        for (int R = hi; R >= 64; --R) if (tile_lds_bytes_mx(R, NF, nwide) <= cap) return R;
        return 0;
    };
    g.R0 = p->tile_rows_override > 0 ? fit(std::min(p->tile_rows_override, TILE_MAX_SLOTS * MX_THREADS), true, (size_t)128 * 1280)
                                     : fit(512, true, budget);
    if (p->tile_rows_override > 0 && p->tile_rows_override < 64) g.R0 = 0;
    if (g.R0 == 0) return false;
    g.R1 = p->tail_rows_override > 0 ? fit(std::min(p->tail_rows_override, TILE_MAX_SLOTS * MX_THREADS), false, (size_t)128 * 1280)
                                     : fit(g.R0, false, budget);
    if (p->tail_rows_override > 0 && p->tail_rows_override < 64) g.R1 = 0;
    return g.R1 != 0;
}

static void fill_steps_mx(StepTableMX &t, const double *steps, int n_steps, int nwide)
{
    float f[MAX_STEP_CH];
    for (int c = 0; c < n_steps; ++c) f[c] = (float)steps[c];
    fill_step_table(t.f, f, n_steps);
    for (int i = 0; i < MX_MAX_WIDE; ++i) t.w[i] = i < nwide ? steps[n_steps == 1 ? 0 : i] : 1.0;
}

// KIND: which tile kernel a stage launches -- the plain one (tile_kernel_mx / _roots), the forward multi-step one, or the
// inverse's comparing stage 0
enum { MX_PLAIN = 0, MX_MULTI = 1, MX_SQ = 2 };

// one tile stage of one scene: the kernel for (KIND, ROOTS, stage 0 or later, one or two rows per thread)
template <bool INV, bool ROOTS, int KIND>
static int launch_tile_mx(bool ident, const TileArgs<float> &A, const MxPtrs &P, const StepTableMX &st, const MxMultiQ *M, unsigned n_tiles,
                          size_t lds, hipStream_t s)
{
    const dim3 grid(n_tiles), block(MX_THREADS);
    return by_ident_slots(ident, A.R <= MX_THREADS, [&](auto id, auto slots) -> int {
        constexpr bool IDENT = decltype(id)::value;
        constexpr int SLOTS = decltype(slots)::value;
        if constexpr (KIND == MX_MULTI) {
            static_assert(!INV && !ROOTS, "multi: forward, no root buffers");
            return launch_lds<tile_kernel_mx_multi<IDENT, SLOTS>>(grid, block, lds, TILE_LDS_LIMIT, s, A, P, st, *M);
        } else if constexpr (KIND == MX_SQ) {
            static_assert(INV && !ROOTS, "sqdiff: inverse stage 0, no root buffers");
            if constexpr (IDENT) return launch_lds<tile_kernel_mx_sq<SLOTS>>(grid, block, lds, TILE_LDS_LIMIT, s, A, P, st);
            else { set_error("mixed sqdiff: stage 0 only"); return RAHT_ERR_INVALID; }
        } else if constexpr (ROOTS) {
            return launch_lds<tile_kernel_mx_roots<INV, IDENT, SLOTS>>(grid, block, lds, TILE_LDS_LIMIT, s, A, P, st);
        } else {
            return launch_lds<tile_kernel_mx<INV, IDENT, SLOTS>>(grid, block, lds, TILE_LDS_LIMIT, s, A, P, st);
        }
    });
}

struct MxIO {
    const float *C_in = nullptr; float *C_out = nullptr; int64_t ldc = 0;
    int32_t *Q = nullptr; int64_t ldq = 0;
    const MxMultiQ *multi = nullptr;                       // forward: raht_fwd_quant_mixed_multi's steps and matrices (Q unused)
    const float *ref = nullptr; int64_t ld_ref = 0;        // inverse stage 0, sqdiff: the reference rows ...
    double *sq_part = nullptr;                             // ... and the per-tile partial sums (C_out may then be NULL)
};

// What one (scene, stage, direction) launches: the kernel arguments, filled and validated by prepare_stage_mx, and the launch
// shape. The single-scene calls launch it as it is (launch_prepared_mx); the batch entries collect stages of equal shape into one
// launch (run_batch_mx).
struct MxStageLaunch {
    bool is_top = false;
    TopArgsMX T;                                           // top stage
    TileArgs<float> A; MxPtrs P;                           // tile stage
    unsigned n_tiles = 0;
    size_t lds = 0;
};

template <bool INV>
static int prepare_stage_mx(const raht_plan *p, const Schedule &sc, int k, const MxIO &io, int D, const MxGeom &g, MxStageLaunch &L)
{
    const Stage &st = sc.stages[(size_t)k];
    const int K = (int)sc.stages.size();
    // a stage's workspace: the float places of every entry, then the wide places of every entry
    float *ws_k = (k >= 1) ? (float *)stage_ws(st, INV) : nullptr;
    float *ws_n = (k + 1 < K) ? (float *)stage_ws(sc.stages[(size_t)k + 1], INV) : nullptr;
    double *ws_k_w = ws_k ? (double *)(ws_k + (size_t)st.n_entries * g.Dp) : nullptr;
    double *ws_n_w = ws_n ? (double *)(ws_n + (size_t)sc.stages[(size_t)k + 1].n_entries * g.Dp) : nullptr;
    if (k >= 1 && !ws_k) { set_error("mixed stage %d: missing stage workspace", k); return RAHT_ERR_INVALID; }
    L.is_top = st.is_top;
    if (st.is_top) {
        TopArgsMX &A = L.T;
        A.in_rows = nullptr; A.ld_in = 0; A.in_img = nullptr; A.in_img_w = nullptr;
        A.out_rows = nullptr; A.ld_out = 0; A.out_img = nullptr; A.out_img_w = nullptr;
        if (!INV) { if (k == 0) { A.in_rows = io.C_in; A.ld_in = io.ldc; } else { A.in_img = ws_k; A.in_img_w = ws_k_w; } }
        else { if (k == 0) { A.out_rows = io.C_out; A.ld_out = io.ldc; } else { A.out_img = ws_k; A.out_img_w = ws_k_w; } }
        A.Q = io.Q; A.ldq = io.ldq;
        A.e_pos = stage_arrays(p, st).pos;
        A.root_rank = st.t_root;
        A.root_f = (float *)p->root_buf; A.root_w = p->root_buf_w;      // (mx_check_args: both or neither)
        A.pj = st.t_pj; A.ab32 = st.t_ab32; A.ab64 = st.t_ab64;
        A.n = (int)st.n_entries; A.n_merges = (int)st.n_merges; A.D = D; A.nwide = g.nwide; A.Fp = g.Dp;
        A.lev = st.t_lev; A.nlev = st.t_nlev; A.nbig = st.t_nbig; A.small_start = st.t_small_start;
        if (!A.e_pos || !A.pj || !A.ab32 || !A.ab64 || !A.lev || !A.Q || (A.root_f && !A.root_rank)) { set_error("mixed top stage: missing plan arrays"); return RAHT_ERR_INVALID; }
        if (!INV && io.multi && A.root_f) { set_error("mixed multi top stage: root buffers"); return RAHT_ERR_INVALID; }
        const size_t n_small = st.n_merges - st.t_small_start;
        L.lds = (size_t)st.n_entries * 16 + ((n_small + 3) & ~(size_t)3) * 4 + n_small * 2 * sizeof(double);
        L.n_tiles = 0;
        return RAHT_OK;
    }
    TileArgs<float> &A = L.A;
    A.rows = st.rows; A.surv_off = st.surv_off; A.n_entries = st.n_entries; A.N = p->N; A.R = st.tile_rows;
    A.D = D; A.Dc = D; A.Dp = g.Dp; A.lg = g.lg; A.nwide = g.nwide;
    A.last_stage = (k == K - 1) ? 1 : 0;
    A.wsum = p->wsum;
    const StageArrays a = stage_arrays(p, st);
    A.lvl = a.lvl; A.wl = a.wl; A.wr = a.wr; A.inv_order = a.pos; A.ht = a.ht;
    A.Q = io.Q; A.ldq = io.ldq;
    A.top_level = p->top_level; A.root_buf = A.last_stage ? (float *)p->root_buf : nullptr; A.dbg = 0; A.ref = nullptr; A.ld_ref = 0; A.sq_part = nullptr;
    A.ld_ws = g.Dp; A.wsn = ws_n;
    A.fin = nullptr; A.ld_fin = 0;
    if (!INV) { A.in = (k == 0) ? io.C_in : ws_k; A.ld_in = (k == 0) ? io.ldc : g.Dp; A.out = nullptr; A.ld_out = 0; }
    else { A.in = nullptr; A.ld_in = 0; A.out = (k == 0) ? io.C_out : ws_k; A.ld_out = (k == 0) ? io.ldc : g.Dp; }
    {
        // every pointer the kernel dereferences for this (direction, stage) must be there before the launch
        const char *bad = nullptr;
        if (!A.lvl || !A.wl || !A.wr || !A.ht) bad = "plan arrays";
        else if (!A.last_stage && (!A.wsn || !A.surv_off)) bad = "survivor workspace of a non-final stage";
        else if (!A.Q || !A.inv_order) bad = "Q / inv_order";
        else if (!INV && !A.in) bad = "forward input";
        else if (INV && !A.out && !(k == 0 && io.sq_part)) bad = "inverse output";
        else if (k == 0 && io.sq_part && (!INV || !io.ref || A.root_buf || (int64_t)st.tile_rows * io.ld_ref * 4 >= ((int64_t)1 << 31))) bad = "sqdiff reference rows";
        else if (!INV && io.multi && A.root_buf) bad = "multi-step write-back without root buffers";
        else if ((st.rows == nullptr) != (k == 0)) bad = "stage order";
        else if (st.tile_rows < 1 || st.tile_rows > TILE_MAX_SLOTS * MX_THREADS ||
                 (int64_t)st.tile_rows * std::max<int64_t>(io.ldc, g.Dp) * 4 >= ((int64_t)1 << 31)) bad = "tile geometry (32-bit row offsets)";
        if (bad) { set_error("mixed tile stage %d (%s): missing %s", k, INV ? "inverse" : "forward", bad); return RAHT_ERR_INVALID; }
    }
    MxPtrs &P = L.P;
    P.in_w = (!INV && k >= 1) ? ws_k_w : nullptr;
    P.out_w = (INV && k >= 1) ? ws_k_w : nullptr;
    P.wsn_w = ws_n_w;
    P.root_w = A.last_stage ? p->root_buf_w : nullptr;
    P.prog = st.prog; P.prog_stride = st.prog_stride; P.prog_ab = st.prog_ab; P.prog_compact = st.prog_compact ? 1 : 0;
    if (!P.prog) { set_error("mixed tile stage %d: missing tile programs", k); return RAHT_ERR_INVALID; }
    L.lds = tile_lds_bytes_mx(st.tile_rows, g.Dp / 4, g.nwide);
    L.n_tiles = (unsigned)st.n_tiles;
    if (INV && k == 0 && io.sq_part) {                     // the comparing stage 0 (raht_dequant_inv_mixed_sqdiff)
        A.out = io.C_out; A.ld_out = io.C_out ? io.ldc : 0;
        A.ref = io.ref; A.ld_ref = io.ld_ref; A.sq_part = io.sq_part;
    }
    return RAHT_OK;
}

// one prepared stage of ONE scene: the launch of the single-scene calls. Stage 0 of a transform, tile or top, is bracketed by the
// plan's profiling events (raht_plan_set_stage0_events) -- the only place of this file that records them.
template <bool INV>
static int launch_prepared_mx(const raht_plan *p, int k, const MxIO &io, const MxStageLaunch &L, const MxGeom &g,
                              const StepTableMX &stp, hipStream_t s)
{
    auto launch = [&]() -> int {
        if (L.is_top) {
            const dim3 grid((unsigned)g.NCp), block(MX_TOP_THREADS);
            if constexpr (!INV) { if (io.multi) return launch_lds<top_kernel_mx_multi>(grid, block, L.lds, TOP_LDS_LIMIT, s, L.T, stp, *io.multi); }
            if (L.T.root_f) return launch_lds<top_kernel_mx_roots<INV>>(grid, block, L.lds, TOP_LDS_LIMIT, s, L.T, stp);
            return launch_lds<top_kernel_mx<INV>>(grid, block, L.lds, TOP_LDS_LIMIT, s, L.T, stp);
        }
        if constexpr (!INV) { if (io.multi) return launch_tile_mx<false, false, MX_MULTI>(k == 0, L.A, L.P, stp, io.multi, L.n_tiles, L.lds, s); }
        if constexpr (INV) { if (k == 0 && io.sq_part) return launch_tile_mx<true, false, MX_SQ>(true, L.A, L.P, stp, nullptr, L.n_tiles, L.lds, s); }
        return L.A.root_buf ? launch_tile_mx<INV, true, MX_PLAIN>(k == 0, L.A, L.P, stp, nullptr, L.n_tiles, L.lds, s)
                            : launch_tile_mx<INV, false, MX_PLAIN>(k == 0, L.A, L.P, stp, nullptr, L.n_tiles, L.lds, s);
    };
    if (!(k == 0 && p->ev_before)) return launch();
    RAHT_HIP_CHECK(hipEventRecord(p->ev_before, s));
    const int rc = launch();
    RAHT_HIP_CHECK(hipEventRecord(p->ev_after, s));
    return rc;
}

template <bool INV>
static int launch_stage_mx(const raht_plan *p, const Schedule &sc, int k, const MxIO &io, int D, const MxGeom &g,
                           const StepTableMX &stp, hipStream_t s)
{
    MxStageLaunch L;
    RAHT_RET((prepare_stage_mx<INV>(p, sc, k, io, D, g, L)));
    return launch_prepared_mx<INV>(p, k, io, L, g, stp, s);
}

static int mx_check_args(const raht_plan *p, const void *a, const void *b, int D, int64_t lda, int64_t ldb, const double *steps,
                         int n_steps, int n_wide, const char *what)
{
    if (!p || !a || !b || D < 1 || lda < D || ldb < D) { set_error("%s: bad argument", what); return RAHT_ERR_INVALID; }
    RAHT_RET(check_plan_device(p, what));
    if (n_wide < 1 || n_wide > MX_MAX_WIDE || n_wide > D) { set_error("%s: n_wide must be 1..%d (and <= D)", what, MX_MAX_WIDE); return RAHT_ERR_INVALID; }
    RAHT_RET(check_quant_steps(what, steps, n_steps, D, true));
    if (p->row_map) { set_error("%s: not available for row-mapped plans", what); return RAHT_ERR_UNSUPPORTED; }
    // root buffers: both (float n_roots x D, float64 n_roots x n_wide) or neither; a truncated plan's roots need them
    if ((p->root_buf == nullptr) != (p->root_buf_w == nullptr)) {
        set_error("%s: set both root buffers (raht_plan_set_root_buffer and raht_plan_set_root_buffer_wide) or neither", what);
        return RAHT_ERR_UNSUPPORTED;
    }
    if (p->top_level < 64 && !p->root_buf) {
        set_error("%s: a truncated plan needs both root buffers (raht_plan_set_root_buffer, raht_plan_set_root_buffer_wide)", what);
        return RAHT_ERR_UNSUPPORTED;
    }
    return RAHT_OK;
}

// fallback path: a float64 call over the compact wide columns, with the plan's root pointer on the wide root buffer (n_wide doubles
// per root, i.e. that call's own row stride) for its duration
template <typename F>
static int with_wide_roots(raht_plan *p, F &&call)
{
    void *const saved = p->root_buf;
    if (saved) p->root_buf = p->root_buf_w;
    const int rc = call();
    p->root_buf = saved;
    return rc;
}

// schedule for the mixed tile kernels, or *sc_out = nullptr when this (plan, D, n_wide) takes the fallback
static int mx_setup(raht_plan *p, int D, int n_wide, int64_t max_ld, hipStream_t s, Schedule **sc_out, MxGeom &g)
{
    *sc_out = nullptr;
    if (p->engine == RAHT_ENGINE_LEVEL || max_ld > ((int64_t)1 << 18)) return RAHT_OK;
    if (!mx_geometry(p, D, n_wide, g)) return RAHT_OK;
    Schedule *sc = nullptr;
    RAHT_RET(get_schedule(p, g.R0, g.R1, g.Rf, s, &sc));
    if (!sc->valid) return RAHT_OK;
    RAHT_RET(build_tile_programs(p, sc, s));
    RAHT_RET(ensure_workspace(sc, (size_t)g.Dp * 4 + (size_t)g.nwide * 8 + 8, p->split_ws));      // float chunks + n_wide doubles (+ slack: the wide part is fetched in 16-byte chunks)
    *sc_out = sc;
    return RAHT_OK;
}

static int fwd_quant_mixed_impl(const raht_plan *cp, const float *C, int64_t ldc, int D, const double *steps, int n_steps, int n_wide,
                                int32_t *Q, int64_t ldq, raht_stream_t stream)
{
    raht_plan *p = const_cast<raht_plan *>(cp);
    hipStream_t s = (hipStream_t)stream;
    RAHT_RET(mx_check_args(p, C, Q, D, ldc, ldq, steps, n_steps, n_wide, "raht_fwd_quant_mixed"));
    Schedule *sc = nullptr;
    MxGeom g;
    RAHT_RET(mx_setup(p, D, n_wide, std::max(ldc, ldq), s, &sc, g));
    if (!sc) {
        // shapes / plans the mixed tile kernels do not cover (level engine, D - n_wide < 4, very wide rows): the float32 path for
        // every channel, then the wide columns once more in float64 through a compact N x n_wide matrix. Root buffers: the float32
        // pass writes the float one, the float64 pass the wide one (the plan holds ONE root pointer: swapped around that call).
        float f[MAX_STEP_CH];
        for (int c = 0; c < n_steps; ++c) f[c] = (float)steps[c];
        RAHT_RET(raht_fwd_quant(p, C, ldc, D, f, n_steps, Q, ldq, stream));
        Scratch tmp(sizeof(double) * 2 * (size_t)p->N * (size_t)n_wide, s);
        if (!tmp.ok()) return RAHT_ERR_NOMEM;
        double *W = tmp.as<double>(), *TW = W + (size_t)p->N * n_wide;
        hipLaunchKernelGGL(mx_cols_to_f64_kernel, dim3((unsigned)ceil_div(p->N * n_wide, 256)), dim3(256), 0, s, C, ldc, p->N, n_wide, W);
        RAHT_HIP_CHECK(hipGetLastError());
        RAHT_RET(with_wide_roots(p, [&]() { return raht_fwd_f64(p, W, n_wide, n_wide, TW, n_wide, nullptr, stream); }));
        double ws[MX_MAX_WIDE];
        for (int i = 0; i < n_wide; ++i) ws[i] = steps[n_steps == 1 ? 0 : i];
        return raht_quant_reorder_f64(p, TW, n_wide, n_wide, ws, n_wide, Q, ldq, stream);
    }
    StepTableMX stp;
    fill_steps_mx(stp, steps, n_steps, n_wide);
    MxIO io;
    io.C_in = C; io.ldc = ldc; io.Q = Q; io.ldq = ldq;
    const int K = (int)sc->stages.size();
    for (int k = 0; k < K; ++k) RAHT_RET((launch_stage_mx<false>(p, *sc, k, io, D, g, stp, s)));
    return RAHT_OK;
}

static int dequant_inv_mixed_impl(const raht_plan *cp, const int32_t *Q, int64_t ldq, int D, const double *steps, int n_steps, int n_wide,
                                  float *C, int64_t ldc, raht_stream_t stream)
{
    raht_plan *p = const_cast<raht_plan *>(cp);
    hipStream_t s = (hipStream_t)stream;
    RAHT_RET(mx_check_args(p, Q, C, D, ldq, ldc, steps, n_steps, n_wide, "raht_dequant_inv_mixed"));
    Schedule *sc = nullptr;
    MxGeom g;
    RAHT_RET(mx_setup(p, D, n_wide, std::max(ldc, ldq), s, &sc, g));
    if (!sc) {
        float f[MAX_STEP_CH];
        for (int c = 0; c < n_steps; ++c) f[c] = (float)steps[c];
        RAHT_RET(raht_dequant_inv(p, Q, ldq, D, f, n_steps, C, ldc, stream));
        Scratch tmp(sizeof(double) * 2 * (size_t)p->N * (size_t)n_wide, s);
        if (!tmp.ok()) return RAHT_ERR_NOMEM;
        double *W = tmp.as<double>(), *TW = W + (size_t)p->N * n_wide;
        double ws[MX_MAX_WIDE];
        for (int i = 0; i < n_wide; ++i) ws[i] = steps[n_steps == 1 ? 0 : i];
        RAHT_RET(raht_dequant_unreorder_f64(p, Q, ldq, n_wide, ws, n_wide, TW, n_wide, stream));
        RAHT_RET(with_wide_roots(p, [&]() { return raht_inv_f64(p, TW, n_wide, n_wide, W, n_wide, stream); }));
        hipLaunchKernelGGL(mx_cols_from_f64_kernel, dim3((unsigned)ceil_div(p->N * n_wide, 256)), dim3(256), 0, s, W, p->N, n_wide, C, ldc);
        RAHT_HIP_CHECK(hipGetLastError());
        return RAHT_OK;
    }
    StepTableMX stp;
    fill_steps_mx(stp, steps, n_steps, n_wide);
    MxIO io;
    io.C_out = C; io.ldc = ldc; io.Q = const_cast<int32_t *>(Q); io.ldq = ldq;
    const int K = (int)sc->stages.size();
    for (int k = K - 1; k >= 0; --k) RAHT_RET((launch_stage_mx<true>(p, *sc, k, io, D, g, stp, s)));
    return RAHT_OK;
}

/* One mixed forward pass, k scalar steps: Q[i] bit-identical to raht_fwd_quant_mixed(..., &steps[i], 1, n_wide, Q[i], ...). The
 * stages, survivors and workspaces are the single call's; only the write-back of every finalised row runs once per step. */
static int fwd_quant_mixed_multi_impl(const raht_plan *cp, const float *C, int64_t ldc, int D, const double *steps, int k, int n_wide,
                                      int32_t *const *Q, int64_t ldq, raht_stream_t stream)
{
    const char *what = "raht_fwd_quant_mixed_multi";
    raht_plan *p = const_cast<raht_plan *>(cp);
    hipStream_t s = (hipStream_t)stream;
    if (!p || !C || !Q || !steps || k < 1) { set_error("%s: bad argument (plan, C, Q, steps must be set, k >= 1)", what); return RAHT_ERR_INVALID; }
    for (int i = 0; i < k; ++i) {
        if (!Q[i]) { set_error("%s: Q[%d] is NULL", what, i); return RAHT_ERR_INVALID; }
        for (int j = 0; j < i; ++j) if (Q[j] == Q[i]) { set_error("%s: Q[%d] and Q[%d] are the same matrix", what, j, i); return RAHT_ERR_INVALID; }
    }
    for (int i = 0; i < k; ++i) RAHT_RET(mx_check_args(p, C, Q[i], D, ldc, ldq, &steps[i], 1, n_wide, what));
    Schedule *sc = nullptr;
    MxGeom g;
    if (!p->root_buf) RAHT_RET(mx_setup(p, D, n_wide, std::max(ldc, ldq), s, &sc, g));
    if (!sc) {
        // the single calls' fallback shapes, and plans with root buffers (every call writes the same roots): one call per step
        for (int i = 0; i < k; ++i) RAHT_RET(fwd_quant_mixed_impl(p, C, ldc, D, &steps[i], 1, n_wide, Q[i], ldq, stream));
        return RAHT_OK;
    }
    const int K = (int)sc->stages.size();
    for (int k0 = 0; k0 < k; k0 += MULTI_Q_MAX) {
        MxMultiQ M;
        M.k = std::min(MULTI_Q_MAX, k - k0);
        M.fast_div = 0;
        for (int i = 0; i < MULTI_Q_MAX; ++i) {
            M.step[i] = steps[k0 + std::min(i, M.k - 1)];
            M.Q[i] = Q[k0 + std::min(i, M.k - 1)];
            const float f = (float)M.step[i];
            if (f >= 0x1p-100f && f <= 0x1p100f) M.fast_div |= 1u << i;        // (fill_step_table's rule, per step)
        }
        StepTableMX stp;
        fill_steps_mx(stp, &steps[k0], 1, n_wide);
        MxIO io;
        io.C_in = C; io.ldc = ldc; io.Q = M.Q[0]; io.ldq = ldq; io.multi = &M;
        for (int kk = 0; kk < K; ++kk) RAHT_RET((launch_stage_mx<false>(p, *sc, kk, io, D, g, stp, s)));
    }
    return RAHT_OK;
}

/* raht_dequant_inv_mixed whose stage 0 also compares every row it writes with C_ref: per-column sums of squared differences of
 * the float32 values the mixed inverse writes (the wide channels after their one rounding), the fixed-order reduction of
 * raht_dequant_inv_sqdiff. C_rec == NULL: the reconstruction is not written. */
static int dequant_inv_mixed_sqdiff_impl(const raht_plan *cp, const int32_t *Q, int64_t ldq, int D, const double *steps, int n_steps,
                                         int n_wide, const float *Cref, int64_t ldref, float *Crec, int64_t ldc, double *sq,
                                         raht_stream_t stream)
{
    const char *what = "raht_dequant_inv_mixed_sqdiff";
    raht_plan *p = const_cast<raht_plan *>(cp);
    hipStream_t s = (hipStream_t)stream;
    if (!p || !Q || !Cref || !sq || D < 1 || ldref < D || (Crec && ldc < D)) { set_error("%s: bad argument (plan, Q, C_ref, sqdiff must be set)", what); return RAHT_ERR_INVALID; }
    RAHT_RET(mx_check_args(p, Q, Cref, D, ldq, ldref, steps, n_steps, n_wide, what));
    Schedule *sc = nullptr;
    MxGeom g;
    if (!p->root_buf) RAHT_RET(mx_setup(p, D, n_wide, std::max(std::max(ldq, ldref), Crec ? ldc : (int64_t)D), s, &sc, g));
    if (!sc || sc->stages.size() < 2 || sc->stages[0].is_top) {
        // shapes outside the mixed tile kernels, one-launch trees, plans with root buffers: the mixed inverse, then the sums
        Scratch tmp(Crec ? 16 : sizeof(float) * (size_t)p->N * (size_t)D, s);
        if (!tmp.ok()) return RAHT_ERR_NOMEM;
        float *out = Crec ? Crec : tmp.as<float>();
        const int64_t ldo = Crec ? ldc : D;
        RAHT_RET(dequant_inv_mixed_impl(p, Q, ldq, D, steps, n_steps, n_wide, out, ldo, stream));
        return raht_sqdiff_columns(Cref, ldref, out, ldo, p->N, D, RAHT_F32, sq, stream);
    }
    const int ncv = g.Dp;                                  // 4 NF partials per tile
    const Stage &st0 = sc->stages[0];
    Scratch part(sizeof(double) * (size_t)st0.n_tiles * (size_t)ncv, s);
    if (!part.ok()) return RAHT_ERR_NOMEM;
    if ((size_t)(MX_THREADS / 64) * (size_t)ncv * 8 > tile_lds_bytes_mx(st0.tile_rows, g.Dp / 4, g.nwide)) {
        set_error("%s: unexpected stage-0 geometry", what);
        return RAHT_ERR_INVALID;
    }
    StepTableMX stp;
    fill_steps_mx(stp, steps, n_steps, n_wide);
    MxIO io;
    io.C_out = Crec; io.ldc = Crec ? ldc : 0; io.Q = const_cast<int32_t *>(Q); io.ldq = ldq;
    io.ref = Cref; io.ld_ref = ldref; io.sq_part = part.as<double>();
    const int K = (int)sc->stages.size();
    for (int k = K - 1; k >= 0; --k) RAHT_RET((launch_stage_mx<true>(p, *sc, k, io, D, g, stp, s)));
    return launch_sq_final(part.as<double>(), (int64_t)st0.n_tiles, D, ncv, sq, s);
}

// ---- several scenes, one set of launches (raht_fwd_quant_mixed_batch / raht_dequant_inv_mixed_batch) ---------------------------
// Round r of the forward direction carries stage r of every scene that has one; the inverse walks the rounds backwards from the
// deepest schedule. Within a round the tile stages of equal launch shape go out up to BATCH_MAX scenes per launch
// (tile_kernel_mx_batch), the top stages likewise (top_kernel_mx_batch, blockIdx.y = scene); a group of one is the single-scene
// launch. Scenes the batch kernels do not cover run through the single-scene entry, in place in the stream.
struct MxScene {
    raht_plan *p = nullptr;
    Schedule *sc = nullptr;                                // nullptr: the single-scene call
    MxGeom g;
    MxIO io;
};

// the batch kernels cover: a mixed tile schedule, no root buffers (a truncated plan always has them here: mx_check_args), no
// stage-0 events (they bracket ONE scene's stage-0 launch)
static bool mx_batchable(const raht_plan *p, const Schedule *sc)
{
    return sc && !p->root_buf && !p->root_buf_w && p->top_level >= 64 && !p->ev_before;
}

// what makes two tile stages one launch: the kernel instantiation (IDENT, SLOTS), the LDS bytes and the row layout
struct MxShape {
    bool ident; int slots; size_t lds; int nwide, NCp, Dp, lg;
    bool operator==(const MxShape &o) const
    { return ident == o.ident && slots == o.slots && lds == o.lds && nwide == o.nwide && NCp == o.NCp && Dp == o.Dp && lg == o.lg; }
};
static MxShape mx_tile_shape(const Stage &st, int k, const MxGeom &g)
{
    return MxShape{k == 0, st.tile_rows <= MX_THREADS ? 1 : 2, tile_lds_bytes_mx(st.tile_rows, g.Dp / 4, g.nwide), g.nwide, g.NCp, g.Dp, g.lg};
}

// group_batch_rounds (tile_host.h) over mixed scenes: the tile stages of a launch agree in MxShape, the top stages in the row layout
template <bool INV, typename FS, typename FT, typename FP>
static int group_mx_scenes(int n, const MxScene *scn, BatchCounts &cnt, FS &&single, FT &&tile, FP &&top)
{
    return group_batch_rounds<INV>(n, [&](int i) { return scn[i].sc ? (int)scn[i].sc->stages.size() : 0; },
                                   [&](int i, int k) { return scn[i].sc->stages[(size_t)k].is_top; },
                                   [&](int i, int j, int k) { return mx_tile_shape(scn[i].sc->stages[(size_t)k], k, scn[i].g) == mx_tile_shape(scn[j].sc->stages[(size_t)k], k, scn[j].g); },
                                   [&](int i, int j, int) { return scn[i].g.NCp == scn[j].g.NCp && scn[i].g.Dp == scn[j].g.Dp; },
                                   cnt, single, tile, top);
}

// the same tile stage of m <= BATCH_MAX scenes (equal launch shape) in one launch, one tile per workgroup. (Tile counts: a
// plan's rows are indexed with 32 bits and a tile holds >= 64 of them, so eight scenes stay far below 2^32 tiles.)
template <bool INV>
static int launch_tile_batch_mx(int m, const MxStageLaunch *const *Ls, bool ident, const StepTableMX &stp, hipStream_t s)
{
    TileBatchMX B;
    B.n = m;
    uint32_t tot = 0;
    for (int i = 0; i < BATCH_MAX; ++i) {
        B.a[i] = Ls[i < m ? i : 0]->A;
        B.p[i] = Ls[i < m ? i : 0]->P;
        B.first_tile[i] = tot;
        if (i < m) tot += Ls[i]->n_tiles;
    }
    B.first_tile[BATCH_MAX] = tot;
    return by_ident_slots(ident, Ls[0]->A.R <= MX_THREADS, [&](auto id, auto slots) -> int {
        return launch_lds<tile_kernel_mx_batch<INV, decltype(id)::value, decltype(slots)::value>>(dim3(tot), dim3(MX_THREADS), Ls[0]->lds, TILE_LDS_LIMIT, s, B, stp);
    });
}

// the top stages of m scenes: one launch, blockIdx.y = scene; the dynamic LDS block is the largest scene's
template <bool INV>
static int launch_top_batch_mx(int m, const MxStageLaunch *const *Ls, int NCp, const StepTableMX &stp, hipStream_t s)
{
    TopBatchMX B;
    size_t lds = 0;
    for (int i = 0; i < BATCH_MAX; ++i) B.a[i] = Ls[i < m ? i : 0]->T;
    for (int i = 0; i < m; ++i) lds = std::max(lds, Ls[i]->lds);
    return launch_lds<top_kernel_mx_batch<INV>>(dim3((unsigned)NCp, (unsigned)m), dim3(MX_TOP_THREADS), lds, TOP_LDS_LIMIT, s, B, stp);
}

// Everything that can be judged from the arguments alone, before any plan is dereferenced and before any HIP call (a / b: the
// input and output matrices of the direction)
static int mx_batch_check_args(const char *what, int n, raht_plan *const *plans, const void *const *a, const int64_t *lda,
                               const void *const *b, const int64_t *ldb, int D, const double *steps, int n_steps, int n_wide)
{
    if (n < 1 || !plans || !a || !lda || !b || !ldb || D < 1) { set_error("%s: bad argument (n >= 1, D >= 1, the arrays of plans, matrices and strides must be set)", what); return RAHT_ERR_INVALID; }
    if (n_wide < 1 || n_wide > MX_MAX_WIDE || n_wide > D) { set_error("%s: n_wide must be 1..%d (and <= D)", what, MX_MAX_WIDE); return RAHT_ERR_INVALID; }
    RAHT_RET(check_quant_steps(what, steps, n_steps, D, true));
    RAHT_RET(check_batch_plans(what, n, plans));
    for (int i = 0; i < n; ++i)
        if (!a[i] || !b[i] || lda[i] < D || ldb[i] < D) { set_error("%s: bad matrix argument (scene %d: NULL pointer or row stride < D)", what, i); return RAHT_ERR_INVALID; }
    return RAHT_OK;
}

// the single calls' plan rules for scene i (device, row map, root buffers), the scene named in the error
static int mx_batch_check_plan(const char *what, int i, const raht_plan *p, const void *a, const void *b, int D, int64_t lda, int64_t ldb,
                               const double *steps, int n_steps, int n_wide)
{
    const int rc = mx_check_args(p, a, b, D, lda, ldb, steps, n_steps, n_wide, what);
    if (rc != RAHT_OK) {
        const std::string msg = raht_last_error();
        set_error("%s (scene %d)", msg.c_str(), i);
    }
    return rc;
}

template <bool INV>
static int run_batch_mx(const char *what, int n, raht_plan *const *plans, const MxIO *ios, int D, const double *steps, int n_steps,
                        int n_wide, hipStream_t s)
{
    std::vector<MxScene> scn((size_t)n);
    for (int i = 0; i < n; ++i) {
        const MxIO &io = ios[i];
        const void *a = INV ? (const void *)io.Q : (const void *)io.C_in, *b = INV ? (const void *)io.C_out : (const void *)io.Q;
        RAHT_RET(mx_batch_check_plan(what, i, plans[i], a, b, D, INV ? io.ldq : io.ldc, INV ? io.ldc : io.ldq, steps, n_steps, n_wide));
    }
    // schedules, tile programs, workspaces; then the arguments of every (scene, stage): nothing is launched unless all are there
    std::vector<size_t> first((size_t)n + 1, 0);
    for (int i = 0; i < n; ++i) {
        MxScene &S = scn[(size_t)i];
        S.p = plans[i]; S.io = ios[i];
        Schedule *sc = nullptr;
        RAHT_RET(mx_setup(S.p, D, n_wide, std::max(S.io.ldc, S.io.ldq), s, &sc, S.g));
        S.sc = mx_batchable(S.p, sc) ? sc : nullptr;
        first[(size_t)i + 1] = first[(size_t)i] + (S.sc ? S.sc->stages.size() : 0);
    }
    std::vector<MxStageLaunch> prep(first[(size_t)n]);
    for (int i = 0; i < n; ++i) {
        const MxScene &S = scn[(size_t)i];
        if (!S.sc) continue;
        for (int k = 0; k < (int)S.sc->stages.size(); ++k) {
            const int rc = prepare_stage_mx<INV>(S.p, *S.sc, k, S.io, D, S.g, prep[first[(size_t)i] + (size_t)k]);
            if (rc != RAHT_OK) {
                const std::string msg = raht_last_error();
                set_error("%s: %s (scene %d)", what, msg.c_str(), i);
                return rc;
            }
        }
    }
    StepTableMX stp;
    fill_steps_mx(stp, steps, n_steps, n_wide);
    auto stage_of = [&](int i, int k) -> const MxStageLaunch & { return prep[first[(size_t)i] + (size_t)k]; };
    auto single = [&](int i) -> int {
        const MxIO &io = scn[(size_t)i].io;
        if constexpr (INV) return dequant_inv_mixed_impl(scn[(size_t)i].p, io.Q, io.ldq, D, steps, n_steps, n_wide, io.C_out, io.ldc, (raht_stream_t)s);
        else return fwd_quant_mixed_impl(scn[(size_t)i].p, io.C_in, io.ldc, D, steps, n_steps, n_wide, io.Q, io.ldq, (raht_stream_t)s);
    };
    auto tile = [&](int m, const int *idx, int k) -> int {
        if (m == 1) return launch_prepared_mx<INV>(scn[(size_t)idx[0]].p, k, scn[(size_t)idx[0]].io, stage_of(idx[0], k), scn[(size_t)idx[0]].g, stp, s);
        const MxStageLaunch *Ls[BATCH_MAX];
        for (int q = 0; q < m; ++q) Ls[q] = &stage_of(idx[q], k);
        return launch_tile_batch_mx<INV>(m, Ls, k == 0, stp, s);
    };
    auto top = [&](int m, const int *idx, int k) -> int {
        if (m == 1) return launch_prepared_mx<INV>(scn[(size_t)idx[0]].p, k, scn[(size_t)idx[0]].io, stage_of(idx[0], k), scn[(size_t)idx[0]].g, stp, s);
        const MxStageLaunch *Ls[BATCH_MAX];
        for (int q = 0; q < m; ++q) Ls[q] = &stage_of(idx[q], k);
        return launch_top_batch_mx<INV>(m, Ls, scn[(size_t)idx[0]].g.NCp, stp, s);
    };
    BatchCounts cnt;
    return group_mx_scenes<INV>(n, scn.data(), cnt, single, tile, top);
}

// the dry run of the grouping: schedules and tile programs may be built, no transform kernel is launched
static int mixed_batch_stats_impl(int n, raht_plan *const *plans, int D, int n_wide, int inverse, int *tile_launches, int *top_launches,
                                  int *single_scene_calls)
{
    const char *what = "raht_mixed_batch_stats";
    if (n < 1 || !plans || !tile_launches || !top_launches || !single_scene_calls || D < 1 || n_wide < 1 || n_wide > MX_MAX_WIDE || n_wide > D) {
        set_error("%s: bad argument", what);
        return RAHT_ERR_INVALID;
    }
    RAHT_RET(check_batch_plans(what, n, plans));
    std::vector<MxScene> scn((size_t)n);
    for (int i = 0; i < n; ++i) {
        MxScene &S = scn[(size_t)i];
        S.p = plans[i];
        RAHT_RET(check_plan_device(S.p, what));
        if (S.p->row_map) { set_error("%s: not available for row-mapped plans (scene %d)", what, i); return RAHT_ERR_UNSUPPORTED; }
        Schedule *sc = nullptr;
        RAHT_RET(mx_setup(S.p, D, n_wide, D, nullptr, &sc, S.g));
        S.sc = mx_batchable(S.p, sc) ? sc : nullptr;
    }
    BatchCounts cnt;
    auto none1 = [](int) { return (int)RAHT_OK; };
    auto none3 = [](int, const int *, int) { return (int)RAHT_OK; };
    if (inverse) RAHT_RET((group_mx_scenes<true>(n, scn.data(), cnt, none1, none3, none3)));
    else RAHT_RET((group_mx_scenes<false>(n, scn.data(), cnt, none1, none3, none3)));
    *tile_launches = cnt.tile; *top_launches = cnt.top; *single_scene_calls = cnt.single;
    return RAHT_OK;
}

}  // namespace raht

using namespace raht;

extern "C" {

int raht_fwd_quant_mixed(const raht_plan *plan, const float *C, int64_t ldc, int D, const double *steps, int n_steps, int n_wide,
                         int32_t *Q, int64_t ldq, raht_stream_t stream)
{
    return guarded("raht_fwd_quant_mixed", [&]() { return fwd_quant_mixed_impl(plan, C, ldc, D, steps, n_steps, n_wide, Q, ldq, stream); });
}

int raht_dequant_inv_mixed(const raht_plan *plan, const int32_t *Q, int64_t ldq, int D, const double *steps, int n_steps, int n_wide,
                           float *C, int64_t ldc, raht_stream_t stream)
{
    return guarded("raht_dequant_inv_mixed", [&]() { return dequant_inv_mixed_impl(plan, Q, ldq, D, steps, n_steps, n_wide, C, ldc, stream); });
}

int raht_fwd_quant_mixed_multi(const raht_plan *plan, const float *C, int64_t ldc, int D, const double *steps, int k, int n_wide,
                               int32_t *const *Q, int64_t ldq, raht_stream_t stream)
{
    return guarded("raht_fwd_quant_mixed_multi", [&]() { return fwd_quant_mixed_multi_impl(plan, C, ldc, D, steps, k, n_wide, Q, ldq, stream); });
}

int raht_dequant_inv_mixed_sqdiff(const raht_plan *plan, const int32_t *Q, int64_t ldq, int D, const double *steps, int n_steps,
                                  int n_wide, const float *C_ref, int64_t ld_ref, float *C_rec, int64_t ldc, double *sqdiff,
                                  raht_stream_t stream)
{
    return guarded("raht_dequant_inv_mixed_sqdiff", [&]() {
        return dequant_inv_mixed_sqdiff_impl(plan, Q, ldq, D, steps, n_steps, n_wide, C_ref, ld_ref, C_rec, ldc, sqdiff, stream); });
}

int raht_fwd_quant_mixed_batch(int n, raht_plan *const *plans, const float *const *C, const int64_t *ldc, int D,
                               const double *steps, int n_steps, int n_wide, int32_t *const *Q, const int64_t *ldq, raht_stream_t stream)
{
    const char *what = "raht_fwd_quant_mixed_batch";
    return guarded(what, [&]() -> int {
        RAHT_RET(mx_batch_check_args(what, n, plans, (const void *const *)C, ldc, (const void *const *)Q, ldq, D, steps, n_steps, n_wide));
        std::vector<MxIO> ios((size_t)n);
        for (int i = 0; i < n; ++i) { MxIO &io = ios[(size_t)i]; io.C_in = C[i]; io.ldc = ldc[i]; io.Q = Q[i]; io.ldq = ldq[i]; }
        return run_batch_mx<false>(what, n, plans, ios.data(), D, steps, n_steps, n_wide, (hipStream_t)stream);
    });
}

int raht_dequant_inv_mixed_batch(int n, raht_plan *const *plans, const int32_t *const *Q, const int64_t *ldq, int D,
                                 const double *steps, int n_steps, int n_wide, float *const *C, const int64_t *ldc, raht_stream_t stream)
{
    const char *what = "raht_dequant_inv_mixed_batch";
    return guarded(what, [&]() -> int {
        RAHT_RET(mx_batch_check_args(what, n, plans, (const void *const *)Q, ldq, (const void *const *)C, ldc, D, steps, n_steps, n_wide));
        std::vector<MxIO> ios((size_t)n);
        for (int i = 0; i < n; ++i) { MxIO &io = ios[(size_t)i]; io.C_out = C[i]; io.ldc = ldc[i]; io.Q = const_cast<int32_t *>(Q[i]); io.ldq = ldq[i]; }
        return run_batch_mx<true>(what, n, plans, ios.data(), D, steps, n_steps, n_wide, (hipStream_t)stream);
    });
}

int raht_mixed_batch_stats(int n, raht_plan *const *plans, int D, int n_wide, int inverse, int *tile_launches, int *top_launches,
                           int *single_scene_calls)
{
    return guarded("raht_mixed_batch_stats", [&]() {
        return mixed_batch_stats_impl(n, plans, D, n_wide, inverse, tile_launches, top_launches, single_scene_calls); });
}

#ifdef RAHT_PHASE_CLOCKS
int raht_debug_read_phase_clocks_mx(unsigned long long *dst, int n_tiles)
{
    RAHT_HIP_CHECK(hipDeviceSynchronize());
    RAHT_HIP_CHECK(hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_phase_clk_mx), sizeof(unsigned long long) * MX_CLK_SLOTS * (size_t)std::min(n_tiles, MX_CLK_TILES)));
    return MX_CLK_SLOTS;
}
#endif

/* Tile rows and stage sizes the mixed kernels use for (D, n_wide): tile_rows = 0 when this shape takes the two-pass fallback. */
int raht_plan_mixed_stats(raht_plan *plan, int D, int n_wide, int *tile_rows, int *n_stages, int64_t *rows_per_stage, int max_stages)
{
    return guarded("raht_plan_mixed_stats", [&]() -> int {
        if (!plan || !tile_rows || !n_stages || D < 1 || n_wide < 1 || n_wide > MX_MAX_WIDE) { set_error("raht_plan_mixed_stats: bad argument"); return RAHT_ERR_INVALID; }
        RAHT_RET(check_plan_device(plan, "raht_plan_mixed_stats"));
        *tile_rows = 0; *n_stages = 0;
        if (plan->row_map) return RAHT_OK;
        Schedule *sc = nullptr;
        MxGeom g;
        RAHT_RET(mx_setup(plan, D, n_wide, D, nullptr, &sc, g));
        if (!sc) return RAHT_OK;
        *tile_rows = g.R0;
        *n_stages = (int)sc->stages.size();
        for (int k = 0; k < *n_stages && k < max_stages && rows_per_stage; ++k) rows_per_stage[k] = sc->stages[(size_t)k].n_entries;
        return RAHT_OK;
    });
}

}  // extern "C"
