// voxelize.hip -- on-device voxelizer: shift / quantize / clamp, 3J-bit Morton key, stable LSD radix
// sort (8-bit digits, wave64 ballot ranking -- scan_sort.hip), voxel boundaries, per-voxel mean.
// Replaces voxelize_pc_batched (reference python/voxelize_pc.py:62-172). Float32 arithmetic, as
// torch performs it on a float32 point cloud; integer outputs are bit-exact.
#include "raht_common.h"
#include "raht_device.h"

#include <algorithm>
#include <cmath>

namespace raht {

// ---- per-axis min / global max reductions (two-stage: block partials, then host) ---------------
__global__ __launch_bounds__(256) void minmax_kernel(const float *__restrict__ PC, int64_t ld, int64_t N,
                                                     float s0, float s1, float s2,
                                                     float *__restrict__ part /* [grid][4]: min x,y,z, max */)
{
    float mn0 = INFINITY, mn1 = INFINITY, mn2 = INFINITY, mx = -INFINITY;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        const float x = PC[i * ld + 0], y = PC[i * ld + 1], z = PC[i * ld + 2];
        mn0 = fminf(mn0, x); mn1 = fminf(mn1, y); mn2 = fminf(mn2, z);
        mx = fmaxf(mx, fmaxf(x - s0, fmaxf(y - s1, z - s2)));      // voxelize_pc.py:92,95
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        mn0 = fminf(mn0, __shfl_xor(mn0, d, 64)); mn1 = fminf(mn1, __shfl_xor(mn1, d, 64));
        mn2 = fminf(mn2, __shfl_xor(mn2, d, 64)); mx = fmaxf(mx, __shfl_xor(mx, d, 64));
    }
    __shared__ float sm[4][4];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) { sm[wid][0] = mn0; sm[wid][1] = mn1; sm[wid][2] = mn2; sm[wid][3] = mx; }
    __syncthreads();
    if (threadIdx.x < 4) {
        float v = sm[0][threadIdx.x];
        for (int w = 1; w < 4; ++w) v = (threadIdx.x < 3) ? fminf(v, sm[w][threadIdx.x]) : fmaxf(v, sm[w][threadIdx.x]);
        part[blockIdx.x * 4 + threadIdx.x] = v;
    }
}

__global__ void boundary_kernel(const uint64_t *__restrict__ keys, int64_t N, uint32_t *__restrict__ flag)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    flag[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;       // voxelize_pc.py:114-118
}

// The voxelizer's secondary outputs (voxelize_pc.py:103-111, 147-156): one lane per output element, rows gathered
// through the sort permutation. vid[k] = voxel of sorted point k (boundary flags scanned).
__global__ __launch_bounds__(256) void residual_kernel(const float *__restrict__ PC, int64_t ldpc, int64_t N, int ld,
                                                       const int64_t *__restrict__ sort_idx, const uint32_t *__restrict__ pos,
                                                       const uint32_t *__restrict__ flag, const float *__restrict__ PCvox,
                                                       float m0, float m1, float m2, float vs, float *__restrict__ PCsorted,
                                                       float *__restrict__ Delta)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N * ld) return;
    const int64_t k = e / ld;
    const int c = (int)(e - k * ld);
    const float x = PC[sort_idx[k] * ldpc + c];
    if (PCsorted) PCsorted[e] = x;                                      // :103-108
    if (c < 3) {
        Delta[e] = vox_pos_residual(x, c, m0, m1, m2, vs);              // :92, :103, :110-111
    } else {
        const int64_t v = (int64_t)pos[k] + (int64_t)flag[k] - 1;       // :129-132
        Delta[e] = x - PCvox[v * ld + c];                               // :147-148
    }
}

// The same in 16-byte row chunks (ld >= 4): a lane owns 4 consecutive columns of a row, 2^lg lanes cover a row, four row
// groups in flight per lane; the last chunk of a row is the 16 bytes that END it (overlapping columns are computed twice
// with identical results). One lane per element spent a 64-bit division per element and moved 4 bytes per instruction:
// 0.86 ms for 3 M x 59 (2.8 GB of gathers and streams), against ~0.55 ms for this form.
__global__ __launch_bounds__(256) void residual_chunk_kernel(const float *__restrict__ PC, int64_t ldpc, int64_t N, int ld, int lg,
                                                             const int64_t *__restrict__ sort_idx, const uint32_t *__restrict__ pos,
                                                             const uint32_t *__restrict__ flag, const float *__restrict__ PCvox,
                                                             float m0, float m1, float m2, float vs, float *__restrict__ PCsorted,
                                                             float *__restrict__ Delta)
{
    const int lane = threadIdx.x & 63;
    const int G = 1 << lg, rpi = 64 >> lg;
    const int g = lane >> lg, c4 = lane & (G - 1);
    const int NC = (ld + 3) >> 2;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int cc = c4; cc < NC; cc += G) {                 // one pass unless ld > 256
        const int goff = min(cc * 4, ld - 4);
        for (int64_t k0 = wave * rpi * 4; k0 < N; k0 += nwaves * rpi * 4) {
            int64_t k[4];
            RegChunk<float> x[4], pv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                k[u] = min(k0 + u * rpi + g, N - 1);
                const int64_t r = sort_idx[k[u]];
                x[u] = ld_chunk<float, true>(PC + r * ldpc + goff);
                if (goff + 3 >= 3 && PCvox) {
                    const int64_t v = (int64_t)pos[k[u]] + (int64_t)flag[k[u]] - 1;       // :129-132
                    pv[u] = ld_chunk<float>(PCvox + v * ld + goff);
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (k0 + u * rpi + g >= N) continue;
                if (PCsorted) st_chunk<float, true>(PCsorted + k[u] * ld + goff, x[u]);   // :103-108
                RegChunk<float> dl;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int c = goff + i;
                    if (c < 3) dl.v[i] = vox_pos_residual(x[u].v[i], c, m0, m1, m2, vs);     // :92, :103, :110-111
                    else dl.v[i] = x[u].v[i] - pv[u].v[i];                                 // :147-148
                }
                st_chunk<float, true>(Delta + k[u] * ld + goff, dl);
            }
        }
    }
}

// What the launches in front of the voxel kernels leave on the device for them: the sort's error word and the voxel count (the host
// reads both back in one piece, at the end of the call: no host round trip in between). A sort that gave up (never seen; the host
// then repeats it pass by pass) left stale indices behind: nothing may be gathered through them.
struct VoxCount { uint32_t sort_err, nvox; };
static_assert(sizeof(VoxCount) == 2 * sizeof(uint32_t), "read back as two words");

// Per-voxel attribute mean. A wave takes 16 voxels per iteration: lanes fetch the 16 (+1) voxel
// starts, first-member indices and keys with vector loads, then the first-member rows are loaded 8 at
// a time (lanes = attribute columns) so that several HBM round trips overlap; further members (rare:
// most voxels hold one point) are added sequentially in sorted order -- the same order as a CPU
// scatter_add_ (voxelize_pc.py:140-144), so the float32 sums are bit-reproducible.
// (Lanes are COLUMNS here and the voxels' extents come through readlane: not the chunk kernels' walk below.)
__global__ __launch_bounds__(256) void voxel_mean_kernel(const float *__restrict__ PC, int64_t ld, int64_t N, int d,
                                                         const uint64_t *__restrict__ keys_sorted,
                                                         const uint32_t *__restrict__ sort_idx,
                                                         const uint32_t *__restrict__ vstart, const VoxCount *__restrict__ cnt,
                                                         float *__restrict__ PCvox, int64_t *__restrict__ Vvox)
{
    if (cnt->sort_err != 0u) return;
    const int64_t nvox = cnt->nvox;
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int ldo = 3 + d;
    for (int64_t v0 = wave * 16; v0 < nvox; v0 += nwaves * 16) {
        const int64_t vi = v0 + lane;
        const uint32_t vs = (lane <= 16 && vi < nvox) ? vstart[vi] : (uint32_t)N;
        uint32_t first = 0;
        if (lane < 16 && vi < nvox) {
            first = sort_idx[vs];
            const VoxCoords k = vox_coords(keys_sorted[vs]);
            if (PCvox) { PCvox[vi * ldo + 0] = (float)k.x; PCvox[vi * ldo + 1] = (float)k.y; PCvox[vi * ldo + 2] = (float)k.z; }
            if (Vvox) { Vvox[vi * 3 + 0] = k.x; Vvox[vi * 3 + 1] = k.y; Vvox[vi * 3 + 2] = k.z; }
        }
        if (!PCvox || d == 0) continue;
        for (int c0 = 0; c0 < d; c0 += 64) {
            const int c = c0 + lane;
            const int cc = min(c, d - 1);
            for (int u0 = 0; u0 < 16; u0 += 8) {
                float acc[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const uint32_t i0 = (uint32_t)__builtin_amdgcn_readlane((int)first, u0 + u);
                    acc[u] = PC[(int64_t)i0 * ld + 3 + cc];
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int64_t v = v0 + u0 + u;
                    if (v >= nvox) break;                                      // wave-uniform
                    const int64_t s = (uint32_t)__builtin_amdgcn_readlane((int)vs, u0 + u);
                    const int64_t e = (uint32_t)__builtin_amdgcn_readlane((int)vs, u0 + u + 1);
                    float a = acc[u];
                    for (int64_t i = s + 1; i < e; ++i) a += PC[(int64_t)sort_idx[i] * ld + 3 + cc];
                    if (c < d) PCvox[v * ldo + 3 + c] = __fdiv_rn(a, (float)(e - s));   // :137,:144
                }
            }
        }
    }
}

// ---- THE voxel walk of the chunk kernels ----------------------------------------------------------------------------------------
// Rows of ld >= 8 floats in 16-byte chunks: 2^lg lanes (lg >= 1) cover a row, a wave holds rpi = 64 >> lg <= 32 row groups and
// keeps U <= 4 voxels per row group in flight, vpi = U * rpi <= 32 voxels per iteration. The lane geometry ...
struct VoxWalk {
    int64_t nvox, first, step;           // voxels of the call; this wave's first voxel and its advance per iteration
    int lane, G, rpi, U, vpi, g, c4, NC; // lanes per row, row groups, voxels in flight; this lane's row group and chunk; chunks per row
};
// ... and one iteration as a lane sees it
struct VoxGroup {
    uint32_t s0[4], e0[4], i0[4];        // this lane's voxels: extents [s0, e0) in sorted order, first member's row
    uint32_t kl[4], kh[4];               // ... and key
    __device__ __forceinline__ VoxCoords coords(int u) const { return vox_coords(((uint64_t)kh[u] << 32) | kl[u]); }
};
// false: nothing to do (reads the count and error words)
__device__ __forceinline__ bool vox_walk_begin(VoxWalk &W, const VoxCount *__restrict__ cnt, int ld, int lg)
{
    if (cnt->sort_err != 0u) return false;
    W.nvox = cnt->nvox;
    W.lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    W.G = 1 << lg; W.rpi = 64 >> lg;
    W.U = min(4, 32 / W.rpi);
    W.vpi = W.U * W.rpi;
    W.g = W.lane >> lg; W.c4 = W.lane & (W.G - 1);
    W.NC = (ld + 3) >> 2;
    W.first = wave * W.vpi; W.step = nwaves * W.vpi;
    return true;
}
// the voxels of the iteration that starts at voxel v0. Vvox (may be NULL): their integer coordinates, written on the way
__device__ __forceinline__ VoxGroup vox_walk_fetch(const VoxWalk &W, int64_t v0, int64_t N, const uint64_t *__restrict__ keys_sorted,
                                                   const uint32_t *__restrict__ sort_idx, const uint32_t *__restrict__ vstart,
                                                   int64_t *__restrict__ Vvox)
{
    const int64_t vi = v0 + W.lane;
    const uint32_t vs = (W.lane <= W.vpi && vi < W.nvox) ? vstart[vi] : (uint32_t)N;
    uint32_t first = 0, klo = 0, khi = 0;
    if (W.lane < W.vpi && vi < W.nvox) {
        first = sort_idx[vs];
        const uint64_t k = keys_sorted[vs];
        klo = (uint32_t)k; khi = (uint32_t)(k >> 32);
        if (Vvox) {
            const VoxCoords c = vox_coords(k);
            Vvox[vi * 3 + 0] = c.x; Vvox[vi * 3 + 1] = c.y; Vvox[vi * 3 + 2] = c.z;
        }
    }
    // this lane's voxels: extents, first member, key. Shuffled here, with every lane active -- inside the chunk loop the
    // idle lanes of a row group are masked off and a shuffle would read garbage from them (an extent of garbage is a
    // multi-million-iteration member loop)
    VoxGroup X;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int sel = min(u, W.U - 1) * W.rpi + W.g;
        X.s0[u] = (uint32_t)__shfl((int)vs, sel, 64);
        X.e0[u] = (uint32_t)__shfl((int)vs, sel + 1, 64);
        X.i0[u] = (uint32_t)__shfl((int)first, sel, 64);
        X.kl[u] = (uint32_t)__shfl((int)klo, sel, 64);
        X.kh[u] = (uint32_t)__shfl((int)khi, sel, 64);
    }
    return X;
}

// Mean AND the voxelizer's secondary outputs in one pass over the gathered rows (ld = 3 + d >= 8 columns, 16-byte chunks of
// the WHOLE row: chunk 0 = x, y, z and the first attribute). Two kernels (a mean kernel, then residual_chunk_kernel)
// gather every point's row twice and read PCvox back once per point: 5 GB on 3 M x 59 where this form moves 3.2 GB. Per voxel
// and chunk: first member's chunk (four voxel groups in flight), further members added in sorted order (:140-144), the mean
// (:137,:144; columns < 3: the voxel's integer coordinates from its key, :152,:155), then -- members of a multi-point voxel are
// gathered once more, the usual single point is still in its register -- PCsorted[k] = the row (:103-108) and DeltaPC[k] =
// row - mean, positions: V0 - voxel_size * floor(V0 / voxel_size) (:110-111, :147-156). Same operations on the same operands
// in the same order as the two kernels: bit-identical outputs.
__global__ __launch_bounds__(256) void voxel_full_chunk_kernel(const float *__restrict__ PC, int64_t ldin, int64_t N, int ld, int lg,
                                                               const uint64_t *__restrict__ keys_sorted,
                                                               const uint32_t *__restrict__ sort_idx,
                                                               const uint32_t *__restrict__ vstart, const VoxCount *__restrict__ cnt,
                                                               float *__restrict__ PCvox, int64_t *__restrict__ Vvox,
                                                               float *__restrict__ PCsorted, float *__restrict__ Delta,
                                                               float m0, float m1, float m2, float vsz)
{
    VoxWalk W;
    if (!vox_walk_begin(W, cnt, ld, lg)) return;
    for (int64_t v0 = W.first; v0 < W.nvox; v0 += W.step) {
        const VoxGroup X = vox_walk_fetch(W, v0, N, keys_sorted, sort_idx, vstart, Vvox);
        for (int cc = W.c4; cc < W.NC; cc += W.G) {
            const int goff = min(cc * 4, ld - 4);
            RegChunk<float> acc[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[u] = ld_chunk<float, true>(PC + (int64_t)X.i0[u] * ldin + goff);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t v = v0 + u * W.rpi + W.g;
                if (u >= W.U || v >= W.nvox) continue;
                const uint32_t s = X.s0[u], e = X.e0[u];
                RegChunk<float> a = acc[u];
                for (uint32_t i = s + 1; i < e; ++i) {               // further members (rare), sorted order (:140-144)
                    const RegChunk<float> b = ld_chunk<float, true>(PC + (int64_t)sort_idx[i] * ldin + goff);
#pragma unroll
                    for (int q = 0; q < 4; ++q) a.v[q] += b.v[q];
                }
                const float cnt_f = (float)(e - s);
#pragma unroll
                for (int q = 0; q < 4; ++q) a.v[q] = __fdiv_rn(a.v[q], cnt_f);                // :137,:144
                if (goff < 3) {                                                                 // integer voxel coordinates from the key (:152,:155)
                    const VoxCoords k = X.coords(u);
                    const float cx = (float)k.x, cy = (float)k.y, cz = (float)k.z;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int c = goff + q;
                        if (c < 3) a.v[q] = (c == 0) ? cx : (c == 1 ? cy : cz);
                    }
                }
                if (PCvox) st_chunk<float, true>(PCvox + v * ld + goff, a);
                if (!PCsorted && !Delta) continue;
                for (uint32_t i = s; i < e; ++i) {
                    const RegChunk<float> x = (i == s) ? acc[u] : ld_chunk<float, true>(PC + (int64_t)sort_idx[i] * ldin + goff);
                    if (PCsorted) st_chunk<float, true>(PCsorted + (int64_t)i * ld + goff, x);  // :103-108
                    if (Delta) {
                        RegChunk<float> dl;
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int c = goff + q;
                            if (c < 3) dl.v[q] = vox_pos_residual(x.v[q], c, m0, m1, m2, vsz);  // :92, :103, :110-111
                            else dl.v[q] = x.v[q] - a.v[q];                                     // :147-148
                        }
                        st_chunk<float, true>(Delta + (int64_t)i * ld + goff, dl);
                    }
                }
            }
        }
    }
}

// VOXELIZE + MERGE in one pass over the gathered rows ("fused into the voxelize dedup"). The reference runs the
// voxelizer and then its CUDA merge kernel back to back (python/test_voxelize_3dgs.py:203-257; cuda/merge_cluster.cu:2-111): the
// sort permutation and the voxel starts ARE the cluster indices / offsets (:225-233). Here the kernel that walks every voxel's
// member rows merges them on the way: rows are whole Gaussians [xyz(3) | quat(4) | scale(3) | opacity(1) | colour(cd)], weight =
// opacity, and per column the arithmetic of merge.hip / merge_cluster.cu -- members in sorted (= index) order, acc = fma(x, w, acc),
// then merge_quat_norm2 / merge_finish (raht_device.h), the very functions merge_kernel finishes with -- so the result is
// bit-identical to raht_voxelize followed by raht_merge_clusters. Output rows: the voxel's integer coordinates (from its key, as
// PCvox carries them, voxelize_pc.py:152,155) and the merged attributes; the merged means optionally on their own. One read of
// every member row instead of two gathers (mean pass + merge pass over five separate arrays).
__global__ __launch_bounds__(256) void voxel_merge_chunk_kernel(const float *__restrict__ PC, int64_t ldin, int64_t N, int ld, int lg,
                                                                const uint64_t *__restrict__ keys_sorted, const uint32_t *__restrict__ sort_idx,
                                                                const uint32_t *__restrict__ vstart, const VoxCount *__restrict__ cnt,
                                                                float *__restrict__ Gvox, float *__restrict__ merged_means, int weight_by_opacity)
{
    VoxWalk W;
    if (!vox_walk_begin(W, cnt, ld, lg)) return;
    for (int64_t v0 = W.first; v0 < W.nvox; v0 += W.step) {
        const VoxGroup X = vox_walk_fetch(W, v0, N, keys_sorted, sort_idx, vstart, nullptr);
        for (int cb = 0; cb < W.NC; cb += W.G) {               // (every lane walks every block of chunks: the shuffles below need them all)
            const int cc = cb + W.c4;
            const bool act = cc < W.NC;
            const int goff = min(min(cc, W.NC - 1) * 4, ld - 4);
            RegChunk<float> x0[4];
            float w0[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                x0[u] = ld_chunk<float, true>(PC + (int64_t)X.i0[u] * ldin + goff);
                w0[u] = weight_by_opacity ? PC[(int64_t)X.i0[u] * ldin + 10] : 1.0f;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t v = v0 + u * W.rpi + W.g;
                const bool live = u < W.U && v < W.nvox;
                float tw = w0[u];
                RegChunk<float> acc;
#pragma unroll
                for (int q = 0; q < 4; ++q) acc.v[q] = (goff + q == 10) ? x0[u].v[q] : __fmaf_rn(x0[u].v[q], w0[u], 0.0f);     // merge_cluster.cu:38-63
                if (live) for (uint32_t i = X.s0[u] + 1; i < X.e0[u]; ++i) {      // further members, sorted (= index) order
                    const int64_t r = (int64_t)sort_idx[i] * ldin;
                    const RegChunk<float> b = ld_chunk<float, true>(PC + r + goff);
                    const float w = weight_by_opacity ? PC[r + 10] : 1.0f;
                    tw += w;
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc.v[q] = (goff + q == 10) ? acc.v[q] + b.v[q] : __fmaf_rn(b.v[q], w, acc.v[q]);
                }
                // quaternion norm (merge_cluster.cu:76-78): columns 3 .. 6 sit in chunks 0 and 1 of this row group's first block
                float n2 = 0.0f;
                if (cb == 0) {
                    const int l0 = W.g << lg, l1 = l0 + 1;
                    n2 = merge_quat_norm2(__shfl(acc.v[3], l0, 64), __shfl(acc.v[0], l1, 64), __shfl(acc.v[1], l1, 64), __shfl(acc.v[2], l1, 64));
                }
                if (!live || !act) continue;
                RegChunk<float> r;
#pragma unroll
                for (int q = 0; q < 4; ++q) r.v[q] = merge_finish(goff + q, acc.v[q], tw, n2);
                if (goff < 3) {
                    const VoxCoords k = X.coords(u);
                    const float cx = (float)k.x, cy = (float)k.y, cz = (float)k.z;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int c = goff + q;
                        if (c < 3) { if (merged_means) merged_means[v * 3 + c] = r.v[q]; r.v[q] = (c == 0) ? cx : (c == 1 ? cy : cz); }
                    }
                }
                st_chunk<float, true>(Gvox + v * ld + goff, r);
            }
        }
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
// lanes per row of the chunk kernels: 2^lg 16-byte chunks cover `columns` floats, at most 2^cap lanes (rows wider than that take
// several passes). 8 columns and more give lg >= 1, which the voxel walk needs.
static int row_lanes_lg(int columns, int cap)
{
    int lg = 0;
    while ((1 << lg) < (columns + 3) / 4 && lg < cap) ++lg;
    return lg;
}

static int out_of_device_memory(const char *what) { set_error("%s: out of device memory", what); return RAHT_ERR_NOMEM; }

// One reduction over the cloud: launch, read back, fold. out[0 .. 2] = per-axis minima, out[3] = max over points and axes of
// V - shift (voxelize_pc.py:87-95). Synchronises the stream.
static int minmax_reduce(const char *what, const float *PC, int64_t ldpc, int64_t N, const float shift[3], float out[4], hipStream_t s)
{
    const int nb = (int)std::min<int64_t>(ceil_div(N, 256), 1024);
    Scratch partb(sizeof(float) * 4 * (size_t)nb, s);
    if (!partb.ok()) return out_of_device_memory(what);
    float hp[1024 * 4];                              // nb <= 1024 partial results (no host allocation: nothing can throw)
    hipLaunchKernelGGL(minmax_kernel, dim3(nb), dim3(256), 0, s, PC, ldpc, N, shift[0], shift[1], shift[2], partb.as<float>());
    RAHT_HIP_CHECK(hipMemcpyAsync(hp, partb.ptr(), sizeof(float) * 4 * (size_t)nb, hipMemcpyDeviceToHost, s));
    RAHT_HIP_CHECK(hipStreamSynchronize(s));
    for (int a = 0; a < 4; ++a) {
        float m = hp[a];
        for (int b = 1; b < nb; ++b) m = (a < 3) ? std::fmin(m, hp[(size_t)b * 4 + a]) : std::fmax(m, hp[(size_t)b * 4 + a]);
        out[a] = m;
    }
    return RAHT_OK;
}

static int voxel_residuals(const char *what, const float *PC, int64_t ldpc, int64_t N, int d, const uint64_t *keys_sorted,
                           const int64_t *sort_idx, const float *PCvox, const float vmin[3], double voxel_size,
                           float *PCsorted, float *DeltaPC, hipStream_t s)
{
    if (!PC || !keys_sorted || !sort_idx || !vmin || !DeltaPC || N < 1 || d < 0 || ldpc < 3 + d || !(voxel_size > 0) || (d > 0 && !PCvox)) {
        set_error("%s: bad argument", what);
        return RAHT_ERR_INVALID;
    }
    if (N >= ((int64_t)1 << 31)) { set_error("%s: N too large", what); return RAHT_ERR_INVALID; }
    Scratch buf(sizeof(uint32_t) * 2 * (size_t)N, s);
    if (!buf.ok()) return out_of_device_memory(what);
    uint32_t *flag = buf.as<uint32_t>(), *pos = flag + N;
    hipLaunchKernelGGL(boundary_kernel, dim3((unsigned)ceil_div(N, 256)), dim3(256), 0, s, keys_sorted, N, flag);
    RAHT_RET(exclusive_scan_u32(flag, pos, N, nullptr, s));
    const int ld = 3 + d;
    if (ld >= 4) {
        const int lg = row_lanes_lg(ld, 6);
        const int64_t rows_per_block = (int64_t)4 * 4 * (64 >> lg);            // 4 waves x 4 row groups in flight
        const unsigned gb = (unsigned)std::min<int64_t>(ceil_div(N, rows_per_block), 16384);
        hipLaunchKernelGGL(residual_chunk_kernel, dim3(gb), dim3(256), 0, s, PC, ldpc, N, ld, lg, sort_idx, pos, flag,
                           PCvox, vmin[0], vmin[1], vmin[2], (float)voxel_size, PCsorted, DeltaPC);
    } else
    hipLaunchKernelGGL(residual_kernel, dim3((unsigned)ceil_div(N * ld, 256)), dim3(256), 0, s, PC, ldpc, N, ld, sort_idx, pos, flag,
                       PCvox, vmin[0], vmin[1], vmin[2], (float)voxel_size, PCsorted, DeltaPC);
    RAHT_HIP_CHECK(hipGetLastError());
    return RAHT_OK;
}

// What the voxel kernel of a call makes of a voxel's member rows
enum class VoxMode { plain /* attribute means */, merge_by_opacity /* whole Gaussians merged, weight = opacity */, merge_unweighted /* weight = 1 */ };
// One voxelizer call: every entry point fills one of these. Pointers as raht.h describes them; any output may be NULL but n_vox.
struct VoxelizeArgs {
    const char *what;                    // the entry point, in front of every message
    const float *PC; int64_t ldpc, N; int d;
    const float *vmin_in; double width_in; int J;
    uint64_t *keys_sorted; int64_t *sort_idx, *voxel_indices;
    float *PCvox; int64_t *Vvox;
    uint64_t *voxel_keys;                // key of every voxel (raht_voxelize_plan)
    float *PCsorted, *DeltaPC;           // raht_voxelize_all
    float *merged_means; VoxMode mode;   // raht_voxelize_merge (PCvox: the merged rows)
    int64_t *n_vox; float *vmin_out; double *width_out, *voxel_size_out;
    hipStream_t stream;
};

static int voxelize_impl(const VoxelizeArgs &A)
{
    const char *what = A.what;
    const int64_t N = A.N;
    const int d = A.d, J = A.J;
    if (!A.PC || N < 1 || d < 0 || A.ldpc < 3 + d || J < 1 || J > 21 || !A.n_vox) { set_error("%s: bad argument", what); return RAHT_ERR_INVALID; }
    if (N >= ((int64_t)1 << 31)) { set_error("%s: N too large", what); return RAHT_ERR_INVALID; }
    if (!(A.width_in < 0) && !(A.width_in > 0)) { set_error("%s: width must be > 0 (got %g)", what, A.width_in); return RAHT_ERR_INVALID; }
    const bool want_res = A.PCsorted || A.DeltaPC;
    const bool fused = A.PCvox && d >= 5;                               // whole rows in 16-byte chunks: 3 + d >= 8 columns
    if (want_res && !fused && !A.sort_idx) { set_error("%s: residuals of a cloud with fewer than 5 attribute columns need sort_idx", what); return RAHT_ERR_INVALID; }
    hipStream_t s = A.stream;
    // ---- vmin / width (voxelize_pc.py:87-95) ----
    float vmin[3], mm[4];
    double width = A.width_in;
    if (A.vmin_in) { vmin[0] = A.vmin_in[0]; vmin[1] = A.vmin_in[1]; vmin[2] = A.vmin_in[2]; }
    else {
        const float zero[3] = {0.f, 0.f, 0.f};
        RAHT_RET(minmax_reduce(what, A.PC, A.ldpc, N, zero, mm, s));
        vmin[0] = mm[0]; vmin[1] = mm[1]; vmin[2] = mm[2];
    }
    if (A.width_in < 0) {
        RAHT_RET(minmax_reduce(what, A.PC, A.ldpc, N, vmin, mm, s));
        width = (double)mm[3];
    }
    if (!(width > 0)) { set_error("%s: width must be > 0 (got %g)", what, width); return RAHT_ERR_INVALID; }
    const double voxel_size = width / (double)((uint64_t)1 << J);   // :97
    const float vs = (float)voxel_size;

    // ---- keys, sort ----
    Scratch kb(sizeof(uint64_t) * 2 * (size_t)N, s), ib(sizeof(uint32_t) * 2 * (size_t)N + sizeof(VoxCount), s);
    if (!kb.ok() || !ib.ok()) return out_of_device_memory(what);
    uint64_t *keys = kb.as<uint64_t>();
    uint64_t *ks = A.keys_sorted ? A.keys_sorted : keys + N;
    uint32_t *idx = ib.as<uint32_t>(), *vstart = idx + N;
    VoxCount *cnt = (VoxCount *)(vstart + N);
    VoxCount back = {0, 0};
    // ONE host round trip per call, at the end: keys + histogram, digit bases, the sort's passes, voxel starts (count on the
    // device), means / residuals are enqueued back to back; the read-back of the count and of the sort's error word is the wait
    const VoxGrid G = {A.PC, A.ldpc, vmin[0], vmin[1], vmin[2], vs, J};
    for (int attempt = 0; attempt < 2; ++attempt) {
        RAHT_RET(sort_keys_u32idx(keys, N, 3 * J, ks, idx, s, &cnt->sort_err, A.sort_idx, &G, attempt == 0));
        RAHT_RET(run_starts_u64(ks, N, vstart, A.voxel_indices, A.voxel_keys, &cnt->nvox, s));
        if (A.PCvox || A.Vvox || want_res) {
            const unsigned gv = (unsigned)std::min<int64_t>(ceil_div(N, 64), 8192);        // (N >= the voxel count)
            if (A.mode != VoxMode::plain)             // at most 16 lanes per row: rows wider than 64 columns take several blocks of chunks
                hipLaunchKernelGGL(voxel_merge_chunk_kernel, dim3(gv), dim3(256), 0, s, A.PC, A.ldpc, N, 3 + d, row_lanes_lg(3 + d, 4), ks, idx, vstart, cnt,
                                   A.PCvox, A.merged_means, A.mode == VoxMode::merge_by_opacity ? 1 : 0);
            else if (fused)
                hipLaunchKernelGGL(voxel_full_chunk_kernel, dim3(gv), dim3(256), 0, s, A.PC, A.ldpc, N, 3 + d, row_lanes_lg(3 + d, 6), ks, idx, vstart, cnt,
                                   A.PCvox, A.Vvox, A.PCsorted, A.DeltaPC, vmin[0], vmin[1], vmin[2], vs);
            else
                hipLaunchKernelGGL(voxel_mean_kernel, dim3(gv), dim3(256), 0, s, A.PC, A.ldpc, N, d, ks, idx, vstart, cnt, A.PCvox, A.Vvox);
        }
        RAHT_HIP_CHECK(hipGetLastError());
        RAHT_RET(read_back_u32((uint32_t *)&back, (const uint32_t *)cnt, 2, nullptr, nullptr, 0, s));
        if (!back.sort_err) break;                           // (else: once more with the pass-by-pass sort)
        note_sort_fallback();
    }
    if (want_res && !fused) {
        // narrow clouds: the two-call sequence (sort_idx as int64 is what the residual kernels take)
        if (A.DeltaPC) RAHT_RET(voxel_residuals(what, A.PC, A.ldpc, N, d, ks, A.sort_idx, A.PCvox, vmin, voxel_size, A.PCsorted, A.DeltaPC, s));
        else RAHT_RET(raht_rows_gather(A.PC, A.ldpc, A.sort_idx, N, 3 + d, 4, A.PCsorted, 3 + d, (raht_stream_t)s));
        RAHT_HIP_CHECK(hipStreamSynchronize(s));
    }
    *A.n_vox = back.nvox;
    if (A.vmin_out) { A.vmin_out[0] = vmin[0]; A.vmin_out[1] = vmin[1]; A.vmin_out[2] = vmin[2]; }
    if (A.width_out) *A.width_out = width;
    if (A.voxel_size_out) *A.voxel_size_out = voxel_size;
    return RAHT_OK;
}

}  // namespace raht

using namespace raht;

extern "C" {

int raht_voxel_keys(const float *PC, int64_t ldpc, int64_t N, const float vmin[3], double width, int J,
                    uint64_t *keys, raht_stream_t stream)
{
    return guarded("raht_voxel_keys", [&]() -> int {
        if (!vmin || N < 0 || J < 1 || J > 21 || !(width > 0)) { set_error("raht_voxel_keys: bad argument"); return RAHT_ERR_INVALID; }
        if (N == 0) return RAHT_OK;                          // empty rank of a sharded cloud: nothing to do; an empty tensor has
                                                             // neither a data pointer nor meaningful strides
        if (!PC || !keys || ldpc < 3) { set_error("raht_voxel_keys: bad argument"); return RAHT_ERR_INVALID; }
        const float vs = (float)(width / (double)((uint64_t)1 << J));        // voxelize_pc.py:97, as raht_voxelize
        const VoxGrid G = {PC, ldpc, vmin[0], vmin[1], vmin[2], vs, J};
        return vox_keys(G, N, keys, (hipStream_t)stream);
    });
}

int raht_voxelize_residuals(const float *PC, int64_t ldpc, int64_t N, int d, const uint64_t *keys_sorted,
                            const int64_t *sort_idx, const float *PCvox, const float vmin[3], double voxel_size,
                            float *PCsorted, float *DeltaPC, raht_stream_t stream)
{
    return guarded("raht_voxelize_residuals", [&]() -> int {
        return voxel_residuals("raht_voxelize_residuals", PC, ldpc, N, d, keys_sorted, sort_idx, PCvox, vmin, voxel_size, PCsorted, DeltaPC,
                               (hipStream_t)stream);
    });
}

int raht_voxelize(const float *PC, int64_t ldpc, int64_t N, int d, const float *vmin_in, double width_in,
                  int J, uint64_t *keys_sorted, int64_t *sort_idx, int64_t *voxel_indices, float *PCvox,
                  int64_t *Vvox, int64_t *n_vox, float vmin_out[3], double *width_out,
                  double *voxel_size_out, raht_stream_t stream)
{
    return guarded("raht_voxelize", [&]() -> int {
        return voxelize_impl({.what = "raht_voxelize", .PC = PC, .ldpc = ldpc, .N = N, .d = d, .vmin_in = vmin_in, .width_in = width_in, .J = J,
                              .keys_sorted = keys_sorted, .sort_idx = sort_idx, .voxel_indices = voxel_indices, .PCvox = PCvox, .Vvox = Vvox,
                              .mode = VoxMode::plain, .n_vox = n_vox, .vmin_out = vmin_out, .width_out = width_out, .voxel_size_out = voxel_size_out,
                              .stream = (hipStream_t)stream});
    });
}

int raht_voxelize_merge(const float *G, int64_t ldg, int64_t N, int color_dim, int weight_by_opacity, const float *vmin_in, double width_in, int J,
                        uint64_t *keys_sorted, int64_t *sort_idx, int64_t *voxel_indices, float *Gvox, float *merged_means, int64_t *n_vox,
                        float vmin_out[3], double *width_out, double *voxel_size_out, raht_stream_t stream)
{
    return guarded("raht_voxelize_merge", [&]() -> int {
        if (color_dim < 0 || !Gvox) { set_error("raht_voxelize_merge: bad argument"); return RAHT_ERR_INVALID; }
        return voxelize_impl({.what = "raht_voxelize_merge", .PC = G, .ldpc = ldg, .N = N, .d = 8 + color_dim, .vmin_in = vmin_in, .width_in = width_in,
                              .J = J, .keys_sorted = keys_sorted, .sort_idx = sort_idx, .voxel_indices = voxel_indices, .PCvox = Gvox,
                              .merged_means = merged_means, .mode = weight_by_opacity ? VoxMode::merge_by_opacity : VoxMode::merge_unweighted,
                              .n_vox = n_vox, .vmin_out = vmin_out, .width_out = width_out, .voxel_size_out = voxel_size_out,
                              .stream = (hipStream_t)stream});
    });
}

int raht_voxelize_all(const float *PC, int64_t ldpc, int64_t N, int d, const float *vmin_in, double width_in,
                      int J, uint64_t *keys_sorted, int64_t *sort_idx, int64_t *voxel_indices, float *PCvox,
                      int64_t *Vvox, float *PCsorted, float *DeltaPC, int64_t *n_vox, float vmin_out[3], double *width_out,
                      double *voxel_size_out, raht_stream_t stream)
{
    return guarded("raht_voxelize_all", [&]() -> int {
        if (DeltaPC && d > 0 && !PCvox) { set_error("raht_voxelize_all: DeltaPC needs PCvox"); return RAHT_ERR_INVALID; }
        return voxelize_impl({.what = "raht_voxelize_all", .PC = PC, .ldpc = ldpc, .N = N, .d = d, .vmin_in = vmin_in, .width_in = width_in, .J = J,
                              .keys_sorted = keys_sorted, .sort_idx = sort_idx, .voxel_indices = voxel_indices, .PCvox = PCvox, .Vvox = Vvox,
                              .PCsorted = PCsorted, .DeltaPC = DeltaPC, .mode = VoxMode::plain, .n_vox = n_vox, .vmin_out = vmin_out, .width_out = width_out, .voxel_size_out = voxel_size_out,
                              .stream = (hipStream_t)stream});
    });
}

int raht_voxelize_plan(const float *PC, int64_t ldpc, int64_t N, int d, const float *vmin_in, double width_in,
                       int J, uint64_t *voxel_keys, int64_t *voxel_indices, float *PCvox, int64_t *n_vox,
                       float vmin_out[3], double *width_out, double *voxel_size_out, raht_stream_t stream, raht_plan **plan)
{
    return guarded("raht_voxelize_plan", [&]() -> int {
        if (!voxel_keys || !plan) { set_error("raht_voxelize_plan: NULL argument"); return RAHT_ERR_INVALID; }
        *plan = nullptr;
        int64_t nv = 0;
        RAHT_RET(voxelize_impl({.what = "raht_voxelize_plan", .PC = PC, .ldpc = ldpc, .N = N, .d = d, .vmin_in = vmin_in, .width_in = width_in, .J = J,
                                .voxel_indices = voxel_indices, .PCvox = PCvox, .voxel_keys = voxel_keys, .mode = VoxMode::plain, .n_vox = &nv, .vmin_out = vmin_out, .width_out = width_out, .voxel_size_out = voxel_size_out,
                                .stream = (hipStream_t)stream}));
        if (n_vox) *n_vox = nv;
        // the voxels' keys are sorted and unique by construction; the plan build checks them anyway (it reads them to find the
        // levels) and BORROWS the caller's array
        return raht_plan_create_from_keys_borrowed(voxel_keys, nv, 3 * J, nullptr, stream, plan);
    });
}

}  // extern "C"
