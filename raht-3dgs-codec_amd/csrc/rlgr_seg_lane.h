// rlgr_seg_lane.h -- what the kernels of the segmented RLGR stage (rlgr_seg.hip, rlgr_rate.hip) share outside the coder
// itself: the coder's constants, which segment a lane works on, when 16-byte accesses are allowed, and when a table entry
// that came off the wire may be followed.
#pragma once
#include "raht_common.h"

namespace raht {
namespace rlgr_seg {

constexpr uint32_t L = 4, U0 = 3, D0 = 1, U1 = 2, D1 = 1;        // membuf.h:18-22

// segment g = c * nseg + s  <->  symbols [i0, i0 + n) = [s * S, min(N, (s + 1) * S)) of channel c
//
// thread t -> segment g. Channel-major data (sym_stride == 1): t = g, a lane walks its own contiguous run.
// Row-major data (the quantized coefficients as the transform kernels leave them: symbol n of channel c at Q[n * ld + c]):
// t = s * D + c -- the lanes of a wave are NEIGHBOURING CHANNELS at the same position of their segments, so every step of
// the wave reads (writes) one contiguous piece of a row: no transpose in front of (behind) the coder.
struct SegLane {
    int c, s;
    int64_t g, i0;
    int n;

    // blocks of 64 threads along x; false: no segment is left for this thread
    __device__ __forceinline__ bool init(int64_t N, int D, int S, int nseg, bool row_major)
    {
        const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
        if (t >= (int64_t)D * nseg) return false;
        if (row_major) { s = (int)(t / D); c = (int)(t - (int64_t)s * D); }
        else { c = (int)(t / nseg); s = (int)(t - (int64_t)c * nseg); }
        g = (int64_t)c * nseg + s;
        i0 = (int64_t)s * S;
        n = (int)min((int64_t)S, N - i0);
        return true;
    }
    // the lane's first symbol in a matrix with these strides
    __device__ __forceinline__ int64_t at(int64_t sym_stride, int64_t chan_stride) const { return (int64_t)c * chan_stride + i0 * sym_stride; }
};

// 16-byte loads / stores of a lane's symbols (a wave-uniform choice): unit symbol stride and every segment start on a 16-byte
// boundary. The encoder reads whole groups of four, the last one up to three symbols past N: those are readable because the
// host admits channel-major data only with chan_stride >= N, and a chan_stride that is a multiple of four is then at least N
// rounded up to four -- the group ends inside the channel's own stride.
__device__ __forceinline__ bool seg_aligned16(const void *Q, int64_t sym_stride, int64_t chan_stride, int S)
{
    return sym_stride == 1 && (((uintptr_t)Q) & 15) == 0 && (chan_stride & 3) == 0 && (S & 3) == 0;
}

// The decoder's tables come off the wire: a segment at `off` of `nb` bytes is followed only when it lies inside the `in_bytes` of
// its container and starts on a word (its last word is read whole: 4-byte slots). The whole offset is judged, in 64 bits, whatever
// the table's width -- nothing sees a narrowed one -- and the length is padded in 64 bits: 2^32 - 1 must not wrap to 0.
__device__ __forceinline__ bool seg_entry_ok(uint64_t off, uint32_t nb, uint64_t in_bytes)
{
    return !((off & 3) || off > in_bytes || (((uint64_t)nb + 3u) & ~(uint64_t)3) > in_bytes - off);
}

}  // namespace rlgr_seg
}  // namespace raht
