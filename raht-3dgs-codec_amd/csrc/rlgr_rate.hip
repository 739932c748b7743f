// rlgr_rate.hip -- the SIZE of a frame's segmented RLGR container at k quantization steps from ONE read of its coefficients
// (raht_rlgr_seg_rate), and the squared quantization error of every segment beside it: the rate-distortion curve of a frame
// without a quantized matrix, a slot buffer or a stream ever being written.
//
// The coder of rlgr_seg.hip is a state machine whose output length depends on the bits it would emit, not on their storing
// (encode_segment<WRITE = false> only counts). Here the counting is all there is: a lane walks the symbols of one segment of one
// channel, quantizes the coefficient it loaded with KS steps (quantize_one / quantize_one_f64: the arithmetic of the kernels
// behind raht_fwd_quant / raht_quant_rows, so the integers are theirs bit for bit) and advances KS independent coder states,
// each of which keeps k_P, k_RP, the run counter m, "a run is open" and a bit count. A segment's length is ceil(bits / 8):
// DevBitWriter::close pads to a byte and counts whole bytes. Every put of encode_segment has its term below:
//   run mode (k = k_P / L > 0), symbol != 0 : 1 + k bits (the 0 flag and the run length), then the Golomb-Rice code of u - 1
//   run mode, symbol == 0                   : nothing, or 1 bit (the 1 flag) when the run reaches 2^k
//   Golomb-Rice code, p = u >> k_R          : p + 1 + k_R bits for p < 32, 64 bits (32 ones + 32 raw bits) for the escape
//   behind the last symbol, run still open  : 1 + k_P / L bits (membuf.cpp:410-413)
// The KS chains of a lane share the load, the loop and the address arithmetic, and they are independent: where one chain of
// the sequential coder leaves issue slots empty (a wave per SIMD waits out every dependent instruction), the others fill them.
#include "raht_common.h"
#include "raht_device.h"
#include "rlgr_seg_lane.h"

#include <algorithm>
#include <cmath>

namespace raht {
namespace rlgr_rate {

using rlgr_seg::L;
using rlgr_seg::U0;
using rlgr_seg::U1;
static_assert(rlgr_seg::D0 == 1 && rlgr_seg::D1 == 1, "Chain::step folds the two decrements, as rlgr_seg.hip does");
constexpr int KMAX = RAHT_RLGR_RATE_MAX;

// one coder state (membuf.cpp:340-423 without the bits)
struct Chain {
    uint32_t k_P = 0, k_RP = 2 * L, m = 0;
    bool open = false;                           // the last symbol left a run open (k != 0 and u == 0 behind the loop)
    uint64_t bits = 0;                           // (an escape is 64 bits: 2^26 symbols would wrap 32)

    __device__ __forceinline__ void step(int32_t v, int flag_signed)
    {
        uint32_t u = flag_signed ? (v < 0 ? ((uint32_t)(-(int64_t)v) << 1) - 1u : (uint32_t)v << 1) : (uint32_t)v;     // _s2u, membuf.cpp:4-13
        const uint32_t k = k_P / L, k_R = k_RP / L;
        const bool nz = u != 0;
        if (k && !nz) {                                              // a zero inside a run (k <= 31: a segment has < 2^31 symbols)
            if (++m == (1u << k)) { bits += 1; k_P += U1; m = 0; }
            open = true;
            return;
        }
        uint32_t nb = 0;
        if (k) { --u; nb = k + 1; }                                  // the run ends: a 0 bit and its length in k bits; the symbol minus one
        const uint32_t p = (k_R < 32) ? (u >> k_R) : 0u;             // (k_R reaches 32 after an escape)
        nb += (p < 32) ? p + 1 + k_R : 64u;
        bits += nb;
        if (p) k_RP = (p > 32 * L) ? 32 * L : min(k_RP + p - 1, 32 * L);
        else k_RP = (k_RP < 2) ? 0 : k_RP - 2;
        if (k || nz) k_P = k_P ? k_P - 1u : 0u;
        else k_P += U0;
        m = 0;
        open = k && !u;
    }
    __device__ __forceinline__ uint32_t close() const                // membuf.cpp:410-413, :47-58
    {
        const uint64_t b = bits + (open ? 1 + k_P / L : 0);
        return (uint32_t)((b + 7) >> 3);
    }
};

template <typename T> struct Quant;
template <> struct Quant<float> {
    float sp, rc;
    __device__ __forceinline__ void set(float s) { sp = s; rc = refined_rcp(s); }
    __device__ __forceinline__ int32_t q(float x) const { return quantize_one(x, sp, rc, 1); }      // (steps within [2^-100, 2^100]: the host checked)
};
template <> struct Quant<double> {
    double sp;
    __device__ __forceinline__ void set(double s) { sp = s; }
    __device__ __forceinline__ int32_t q(double x) const { return quantize_one_f64(x, sp); }
};

// thread -> segment as the row-major encoder (SegLane): the lanes of a wave are neighbouring channels at the same position of
// their segments. steps: DEVICE, kact x n_steps; chains j >= kact repeat chain kact - 1 and are not stored.
// seg_bytes / seg_sse: already offset to the first step of this launch; row j at + j * G.
template <typename T, int KS, bool SSE>
__global__ __launch_bounds__(64) void seg_rate_kernel(const T *__restrict__ X, int64_t ldt, int64_t N, int D, int S, int nseg, int flag_signed,
                                                      const T *__restrict__ steps, int n_steps, int kact, uint32_t *__restrict__ seg_bytes,
                                                      double *__restrict__ seg_sse)
{
    rlgr_seg::SegLane ln;
    if (!ln.init(N, D, S, nseg, true)) return;
    const int64_t G = (int64_t)D * nseg, g = ln.g;
    const int c = ln.c, n = ln.n;
    Chain ch[KS];
    Quant<T> qz[KS];
    double sse[KS];
#pragma unroll
    for (int j = 0; j < KS; ++j) {
        qz[j].set(steps[(int64_t)min(j, kact - 1) * n_steps + (n_steps == 1 ? 0 : c)]);
        sse[j] = 0.0;
    }
    const T *rp = X + ln.at(ldt, 1);                                 // (walked by pointer: a 64-bit multiply per symbol otherwise)
    T nxt = *rp;                                                     // n >= 1
    for (int i = 0; i < n; ++i) {
        const T x = nxt;
        if (i + 1 < n) { rp += ldt; nxt = *rp; }                     // one symbol ahead: the load is off the dependent chains
#pragma unroll
        for (int j = 0; j < KS; ++j) {
            const int32_t q = qz[j].q(x);
            if (SSE) {
                // plain double arithmetic, every operation rounded: where q * step needs more than 53 bits a fused multiply-add
                // would give another (no less valid) e than the formula of raht.h evaluated on a host
#pragma clang fp contract(off)
                const double e = (double)x - (double)q * (double)qz[j].sp;
                sse[j] += e * e;
            }
            ch[j].step(q, flag_signed);
        }
    }
#pragma unroll
    for (int j = 0; j < KS; ++j) {
        if (j < kact) {
            seg_bytes[(int64_t)j * G + g] = ch[j].close();
            if (SSE) seg_sse[(int64_t)j * G + g] = sse[j];
        }
    }
}

template <typename T, int KS>
static void launch_ks(bool sse, unsigned gb, hipStream_t s, const T *X, int64_t ldt, int64_t N, int D, int S, int nseg, int flag_signed, const T *steps,
                      int n_steps, int kact, uint32_t *seg_bytes, double *seg_sse)
{
    if (sse) hipLaunchKernelGGL((seg_rate_kernel<T, KS, true>), dim3(gb), dim3(64), 0, s, X, ldt, N, D, S, nseg, flag_signed, steps, n_steps, kact, seg_bytes, seg_sse);
    else hipLaunchKernelGGL((seg_rate_kernel<T, KS, false>), dim3(gb), dim3(64), 0, s, X, ldt, N, D, S, nseg, flag_signed, steps, n_steps, kact, seg_bytes, seg_sse);
}

static bool step_ok(float s) { return std::isfinite(s) && s >= 0x1p-100f && s <= 0x1p100f; }     // fill_step_table's fast_div range
static bool step_ok(double s) { return std::isfinite(s) && s > 0.0; }

template <typename T>
static int rate_impl(const T *X, int64_t ldt, int64_t N, int D, const T *steps, int k, int n_steps, int seg_len, int flag_signed, uint32_t *seg_bytes,
                     double *seg_sse, int64_t nseg, int64_t G, hipStream_t s)
{
    for (int64_t i = 0; i < (int64_t)k * n_steps; ++i)
        if (!step_ok(steps[i])) {
            set_error(sizeof(T) == 4 ? "raht_rlgr_seg_rate: step %d of table %d must be finite and within [2^-100, 2^100]" : "raht_rlgr_seg_rate: step %d of table %d must be finite and > 0",
                      (int)(i % n_steps), (int)(i / n_steps));
            return RAHT_ERR_INVALID;
        }
    Scratch dsteps(sizeof(T) * (size_t)k * (size_t)n_steps, s);
    if (!dsteps.ok()) return RAHT_ERR_NOMEM;
    // (hipMemcpyAsync from pageable memory copies the source before it returns: the caller's table may go away)
    RAHT_HIP_CHECK(hipMemcpyAsync(dsteps.ptr(), steps, sizeof(T) * (size_t)k * (size_t)n_steps, hipMemcpyHostToDevice, s));
    const unsigned gb = (unsigned)ceil_div(G, 64);
    for (int j0 = 0; j0 < k; j0 += KMAX) {                           // KMAX steps per pass over the coefficients
        const int kact = std::min(KMAX, k - j0);
        const T *st = dsteps.as<T>() + (size_t)j0 * n_steps;
        uint32_t *sb = seg_bytes + (size_t)j0 * (size_t)G;
        double *se = seg_sse ? seg_sse + (size_t)j0 * (size_t)G : nullptr;
        const bool sse = seg_sse != nullptr;
        if (kact > 4) launch_ks<T, 8>(sse, gb, s, X, ldt, N, D, seg_len, (int)nseg, flag_signed, st, n_steps, kact, sb, se);
        else if (kact > 2) launch_ks<T, 4>(sse, gb, s, X, ldt, N, D, seg_len, (int)nseg, flag_signed, st, n_steps, kact, sb, se);
        else if (kact > 1) launch_ks<T, 2>(sse, gb, s, X, ldt, N, D, seg_len, (int)nseg, flag_signed, st, n_steps, kact, sb, se);
        else launch_ks<T, 1>(sse, gb, s, X, ldt, N, D, seg_len, (int)nseg, flag_signed, st, n_steps, kact, sb, se);
    }
    RAHT_HIP_CHECK(hipGetLastError());
    return RAHT_OK;
}

}  // namespace rlgr_rate
}  // namespace raht

using namespace raht;

extern "C" {

int raht_rlgr_seg_rate(const void *T, int dtype, int64_t ldt, int64_t N, int D, const void *steps, int k, int n_steps, int seg_len, int flag_signed,
                       uint32_t *seg_bytes, double *seg_sse, raht_stream_t stream)
{
    if (!T || !steps || !seg_bytes) { set_error("raht_rlgr_seg_rate: T, steps and seg_bytes are required"); return RAHT_ERR_INVALID; }
    if (dtype != RAHT_F32 && dtype != RAHT_F64) { set_error("raht_rlgr_seg_rate: dtype must be RAHT_F32 or RAHT_F64"); return RAHT_ERR_INVALID; }
    if (N < 1 || D < 1 || ldt < D || k < 1 || !(n_steps == 1 || n_steps == D)) {
        set_error("raht_rlgr_seg_rate: bad argument (N, D, k >= 1, ldt >= D, n_steps 1 or D)");
        return RAHT_ERR_INVALID;
    }
    if (flag_signed != 0 && flag_signed != 1) { set_error("raht_rlgr_seg_rate: flag_signed must be 0 or 1"); return RAHT_ERR_INVALID; }
    // the shapes raht_rlgr_seg_encode_strided takes: seg_len >= 64, fewer than 2^31 segments, 32-bit offsets and lengths
    if (seg_len < 64) { set_error("raht_rlgr_seg_rate: seg_len must be >= 64"); return RAHT_ERR_INVALID; }
    const int width = raht_rlgr_seg_offsets_width(N, D, seg_len);
    if (width != 32) {
        if (width == 64) set_error("raht_rlgr_seg_rate: %lld x %d symbols may need a container of 4 GiB or more (32-bit segment offsets): split the frame", (long long)N, D);
        else set_error("raht_rlgr_seg_rate: %lld x %d symbols in segments of %d: too many segments, or a segment whose length may not fit 32 bits", (long long)N, D, seg_len);
        return RAHT_ERR_INVALID;
    }
    const int64_t nseg = (N - 1) / seg_len + 1, G = nseg * D;
    if (dtype == RAHT_F32)
        return rlgr_rate::rate_impl<float>((const float *)T, ldt, N, D, (const float *)steps, k, n_steps, seg_len, flag_signed, seg_bytes, seg_sse, nseg, G, (hipStream_t)stream);
    return rlgr_rate::rate_impl<double>((const double *)T, ldt, N, D, (const double *)steps, k, n_steps, seg_len, flag_signed, seg_bytes, seg_sse, nseg, G, (hipStream_t)stream);
}

}  // extern "C"
