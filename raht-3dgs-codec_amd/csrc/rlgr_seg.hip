// rlgr_seg.hip -- the RLGR entropy stage ON THE GPU, segmented (second half: "GPU-segmented").
//
// The reference's coder (python/PyRLGR/src/libs/rlgr/membuf.cpp:258-423, parameters membuf.h:18-22) is one sequential
// adaptive stream per channel: ~3 M symbols that each depend on the state all earlier ones left. csrc/rlgr.hip runs the 56
// channels of a frame on the host threads, byte-exact, and that is what bounds a frame end to end (round 3: 65 ms per pass
// on 16 CPUs next to 0.6 ms of transforms, plus 12 ms of PCIe each way for the raw integers). Here every channel is cut
// into SEGMENTS of `seg_len` symbols and every segment is its own RLGR stream -- the coder's state starts afresh (k_P = 0,
// k_RP = 2 L), the stream is padded to a byte boundary and, in the container, to a 4-byte boundary. One lane codes one
// segment; 3 M x 56 symbols at 4096 per segment are 41 k independent streams = 656 waves.
//
// What "parity" means here: segment (c, s) is BYTE-IDENTICAL to what the reference's membuf::rlgrWrite produces for the
// slice Q[c, s * seg_len : (s + 1) * seg_len] -- tests compare every segment with the host coder of rlgr.hip (itself pinned
// byte for byte by reference-built streams, tests/test_rlgr.py), so any RLGR decoder reads a segment. The CONTAINER (sizes
// table + concatenated segments) is this repo's: the reference has no segmented format. Cost of the restarts: the coder
// re-adapts within a few dozen symbols; tests / DESIGN.md quote the measured size difference.
#include "raht_common.h"
#include "rlgr_seg_lane.h"

namespace raht {
namespace rlgr_seg {

// MSB-first bit writer, same byte stream as membuf::write / flush (and as BitWriter of rlgr.hip): < 32 bits pending after
// every put, whole 32-bit words leave big-endian. WRITE = false only counts. `out` is 4-byte aligned.
// LDSOUT (out32 16-byte aligned): the words of a lane collect in a 16-word LDS column ([16][64] words per wave, as in the
// decoder below) and leave as one 64-byte piece -- with the steps of a frame coded together the one-word stores of 738 k lanes
// cost 8 x the streams' bytes in HBM writes (3.7 GB for 0.47 GB, rocprofv3 WRITE_SIZE).
template <bool WRITE, bool LDSOUT = false>
struct DevBitWriter {
    uint32_t *out32;
    uint32_t size = 0;       // bytes (keeps counting past cap: the exact length is known either way)
    uint32_t cap = 0xffffffffu;   // bytes that may be written at out32 (a multiple of 4); past it nothing is stored
    uint64_t acc = 0;
    int nbits = 0;
    uint32_t *col = nullptr; // LDSOUT: this lane's column

    __device__ __forceinline__ void store_word(uint32_t w)          // the word at byte offset `size`
    {
        if (!WRITE || size + 4 > cap) return;
        if (LDSOUT) {
            const uint32_t wi = size >> 2, q = wi & 15u;
            col[q * 64] = w;
            if (q == 15u) {
                uint4 x[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) x[t] = make_uint4(col[(4 * t) * 64], col[(4 * t + 1) * 64], col[(4 * t + 2) * 64], col[(4 * t + 3) * 64]);
#pragma unroll
                for (int t = 0; t < 4; ++t) *(uint4 *)(out32 + wi - 15 + 4 * t) = x[t];
            }
        } else {
            out32[size >> 2] = w;
        }
    }
    __device__ __forceinline__ void put(uint64_t v, int bits)      // bits <= 32, v < 2^bits
    {
        acc = (acc << bits) | v;
        nbits += bits;
        if (nbits >= 32) {
            nbits -= 32;
            store_word(__builtin_bswap32((uint32_t)(acc >> nbits)));
            size += 4;
        }
    }
    __device__ __forceinline__ void put_wide(uint32_t v, int bits)   // the run length m in k bits (k <= 32 inside a segment)
    {
        if (bits > 32) { put(0, bits - 32); put(v, 32); }
        else put(bits == 32 ? v : (bits ? (v & ((1u << bits) - 1u)) : 0u), bits);
    }
    __device__ __forceinline__ void golomb_rice(uint32_t u, int k)  // membuf.cpp:242-256; k <= 32
    {
        const uint32_t p = (k < 32) ? (u >> k) : 0u;
        const uint32_t rem = (k >= 32) ? u : (u & ((1u << k) - 1u));
        if (p < 32) {
            const uint32_t pre = (uint32_t)((1ull << (p + 1)) - 2);               // p ones and a zero
            if (p + 1 + (uint32_t)k <= 32) put(((uint64_t)pre << k) | rem, (int)p + 1 + k);
            else { put(pre, (int)p + 1); put(rem, k); }
        } else {
            put(0xffffffffull, 32);                                               // escape: 32 ones, then 32 raw bits
            put(u, 32);
        }
    }
    __device__ __forceinline__ void close()                         // membuf.cpp:47-58
    {
        if (nbits & 7) put(0, 8 - (nbits & 7));
        uint32_t words = size >> 2;                                 // whole words so far
        if (nbits > 0) {                                            // 1..3 whole bytes left: the last, partial word (zero filled)
            const uint32_t word = (uint32_t)(acc << (32 - nbits));
            store_word(__builtin_bswap32(word));
            if (size + 4 <= cap) ++words;
            size += (uint32_t)(nbits >> 3);
            nbits = 0;
        }
        if (WRITE && LDSOUT) {                                      // the last, partial column (a full one left when its 16th word came)
            const uint32_t stored = min(words, cap >> 2);
            for (uint32_t wi = stored & ~15u; wi < stored; ++wi) out32[wi] = col[(wi & 15u) * 64];
        }
    }
};

__device__ __forceinline__ uint64_t s2u(int64_t v) { return v < 0 ? (((uint64_t)(-v)) << 1) - 1 : ((uint64_t)v) << 1; }
__device__ __forceinline__ int64_t u2s(uint64_t v) { const int64_t d = (int64_t)(v >> 1); return (v & 1) ? -d - 1 : d; }

#define RLGS_ADAPT_KRP(p)                                            \
    do {                                                             \
        if (p) { k_RP += (p) - 1; if (k_RP > 32 * L) k_RP = 32 * L; } \
        else { k_RP = (k_RP < 2) ? 0 : k_RP - 2; }                   \
    } while (0)

// (p - 1 may not fit 32 bits together with k_RP: saturate first)
#define RLGS_ADAPT_KRP32(p)                                                              \
    do {                                                                                 \
        if (p) { k_RP = ((p) > 32 * L) ? 32 * L : min(k_RP + (p) - 1, 32 * L); }         \
        else { k_RP = (k_RP < 2) ? 0 : k_RP - 2; }                                       \
    } while (0)

// membuf.cpp:340-423 on one segment
// VEC: the segment starts on a 16-byte boundary -- symbols are fetched four at a time (a lane walks its own segment, so a
// wave's loads touch 64 different lines either way: 16-byte loads make it a quarter as many instructions and lookups)
// What bounds this coder is instruction issue, one wave per SIMD at most: ~170 instructions per symbol (both modes' paths
// are walked by a wave whose lanes disagree), 2.6 waves per SIMD at 1024 symbols per segment, 0.64 at 4096 -- the time per pass is
// that of ONE wave walking its segments: proportional to seg_len above ~1500. Staging the symbols / the output through LDS in
// blocks of 64 (to take the loads and stores off each other's wait counter) changed nothing for the encoder and made the
// decoder slower (round 3): memory is not what a lane waits for.
template <bool WRITE, bool VEC, bool LDSOUT = false>
__device__ __forceinline__ uint32_t encode_segment(const int32_t *__restrict__ seq, int n, int flag_signed, uint32_t *out32, uint32_t cap = 0xffffffffu,
                                                   int64_t sstr = 1,     // sstr: distance between consecutive symbols (VEC: 1)
                                                   uint32_t *lds = nullptr)
{
    DevBitWriter<WRITE, LDSOUT> w;
    w.out32 = out32;
    w.cap = cap;
    w.col = lds + (threadIdx.x & 63);
    // 32-bit state: u = s2u(int32) < 2^32; inside a segment of n < 2^31 symbols the run counter m and the run exponent
    // k (<= log2 n + 1) stay far below 32 bits; k_RP is capped at 32 L. (The host coder carries them in 64 bits because one
    // stream may hold 2^32 symbols and more; 64-bit integer arithmetic is several instructions per operation here.)
    uint32_t u = 0, k_P = 0, k_RP = 2 * L, m = 0, k = 0;
    int32_t nxt = (!VEC && n > 0) ? seq[0] : 0;
    const int32_t *rp = seq;                                         // (walked by pointer: a 64-bit multiply per symbol otherwise)
    int4 cur4 = make_int4(0, 0, 0, 0), nxt4 = make_int4(0, 0, 0, 0);
    if (VEC && n > 0) nxt4 = *(const int4 *)seq;                     // (whole groups of four are readable: see the kernel)
    for (int i = 0; i < n; ++i) {
        int32_t v;
        if (VEC) {
            if ((i & 3) == 0) { cur4 = nxt4; if (i + 4 < n) nxt4 = *(const int4 *)(seq + i + 4); }    // one group ahead
            const int q = i & 3;
            v = q == 0 ? cur4.x : q == 1 ? cur4.y : q == 2 ? cur4.z : cur4.w;
        } else {
            v = nxt;
            if (i + 1 < n) { rp += sstr; nxt = *rp; }                // one symbol ahead: the load is off the dependent chain
        }
        u = flag_signed ? (v < 0 ? ((uint32_t)(-(int64_t)v) << 1) - 1u : (uint32_t)v << 1) : (uint32_t)v;     // _s2u, membuf.cpp:4-13
        k = k_P / L;
        const uint32_t k_R = k_RP / L;
        // ONE Golomb-Rice site for both modes (the symbol that ends a run and a no-run symbol differ by what precedes the code and by
        // the k_P step): a wave whose lanes disagree about the mode walks the code path once, not twice
        bool code = true;
        const bool nz = u != 0;
        if (k) {                                                    // run mode
            if (nz) {
                --u;                                                // (in place, as membuf.cpp does: the open-run test behind the loop sees it)
                if (k < 32) w.put((uint64_t)(m & ((1u << k) - 1u)), (int)k + 1);      // a 0 bit, then the run length in k bits
                else { w.put(0, 1); w.put_wide(m, (int)k); }
            } else {
                code = false;
                if (++m == ((k < 32) ? (1u << k) : 0u)) {           // (k >= 32 needs 2^32 zeros in one segment: never)
                    w.put(1, 1);
                    k_P += U1;
                    m = 0;
                }
            }
        }
        if (code) {
            w.golomb_rice(u, (int)k_R);
            const uint32_t p = (k_R < 32) ? (u >> k_R) : 0u;        // (k_R reaches 32 after an escape: a 32-bit shift by 32 is not 0)
            RLGS_ADAPT_KRP32(p);
            if (k || nz) k_P = k_P ? k_P - 1u : 0u;                  // D0 = D1 = 1 (run mode: always; no-run mode: after a nonzero symbol)
            else k_P += U0;
            m = 0;
        }
    }
    if (n > 0 && k && !u) {                                         // membuf.cpp:410-413: flush the open run
        w.put(0, 1);
        w.put_wide(m, (int)(k_P / L));
    }
    w.close();
    return w.size;
}

// MSB-first bit reader over a 4-byte aligned segment of `size` bytes; bits past the end read as zeros
// LDSIN: the stream's words come through an 8-word LDS column per lane ([8][64] words per wave), fetched as one aligned 32-byte
// piece (2 x 16 bytes) when the lane crosses into it -- a lane's 4-byte reads, far apart in time, found their line evicted
// between two of them once the steps of a frame decode together (FETCH_SIZE 12 x the streams' bytes). Pieces are aligned
// in memory, not to the segment: the first one may begin before the segment (inside the container: `lo`), the last one may
// reach past it (`hi`: words at or beyond it read as zero and are never consumed: fill() stops at `size`).
// MODE 2 (the symbol-synchronous decoder): a RING of 16 words per lane ([16][64] words per wave) that ALL lanes of the wave top up
// at the same iterations (top_up(), every 32 symbols): the wave then waits for stream words once per 32 iterations instead of
// whenever some lane crosses into a new piece -- with 64 lanes that was most iterations, and for a frame on its own (1.25 waves
// per SIMD, nothing else to run meanwhile) each such wait is a memory round trip on the wave's only chain. A lane that drains its
// ring before the next top-up (more than 16 bits per symbol over 32 symbols) reads its words one by one until then.
template <int MODE>
struct DevBitReaderT {
    static constexpr bool LDSIN = MODE == 1;
    static constexpr int RING = 16;
    uint32_t have = 0;           // MODE 2: words [0, have) have been fetched (the ring holds the last RING of them at most)
    const uint32_t *in32;
    uint32_t size, pos = 0;      // bytes; pos is a multiple of 4 (whole words are consumed, the last one zero-extended)
    uint64_t acc = 0;
    int nbits = 0;
    uint32_t *col = nullptr;     // LDSIN: this lane's column
    uint32_t w0 = 0;             // LDSIN: word index of the segment's start inside its first 32-byte piece
    int64_t hi_words = 0;        // LDSIN: words from the segment's start to the end of the container

    __device__ __forceinline__ void top_up()                         // MODE 2, called by every lane of the wave at the same time
    {
        const uint32_t next = pos >> 2, nwords = (size + 3u) >> 2;  // next word to consume; words of this stream
        if (have < next) have = next;                               // (the lane read ahead of its ring word by word)
#pragma unroll
        for (int t = 0; t < RING; ++t) {
            const uint32_t w = have + (uint32_t)t;
            if (w < next + RING && w < nwords) col[(w & (RING - 1)) * 64] = in32[w];
        }
        have = min(min(have + (uint32_t)RING, next + (uint32_t)RING), nwords);
    }
    __device__ __forceinline__ uint32_t word(uint32_t w)
    {
        if (MODE == 2) return (w < have) ? col[(w & (RING - 1)) * 64] : in32[w];
        if (!LDSIN) return in32[w];
        const uint32_t gw = w + w0, q = gw & 7u;
        if (q == 0 || w == 0) {                                      // into a new piece (or the very first word): fetch it
            const int64_t first = (int64_t)w - (int64_t)q;           // word index (from the segment's start) of the piece's first word; >= -7
            const uint4 *src = (const uint4 *)(in32 + first);
            uint4 a = make_uint4(0, 0, 0, 0), b = a;
            if (first + 8 <= hi_words) { a = src[0]; b = src[1]; }
            else {                                                   // the container ends inside this piece: word by word
                const uint32_t *sw = in32 + first;
                if (first + 0 < hi_words) a.x = sw[0];
                if (first + 1 < hi_words) a.y = sw[1];
                if (first + 2 < hi_words) a.z = sw[2];
                if (first + 3 < hi_words) a.w = sw[3];
                if (first + 4 < hi_words) b.x = sw[4];
                if (first + 5 < hi_words) b.y = sw[5];
                if (first + 6 < hi_words) b.z = sw[6];
                if (first + 7 < hi_words) b.w = sw[7];
            }
            col[0 * 64] = a.x; col[1 * 64] = a.y; col[2 * 64] = a.z; col[3 * 64] = a.w;
            col[4 * 64] = b.x; col[5 * 64] = b.y; col[6 * 64] = b.z; col[7 * 64] = b.w;
        }
        return col[q * 64];
    }
    __device__ __forceinline__ void fill()                           // afterwards nbits > 32 unless the stream ended
    {
        if (nbits <= 32 && pos < size) {
            uint32_t w = __builtin_bswap32(word(pos >> 2));
            const uint32_t left = size - pos;
            int got = 32;
            if (left < 4) { got = (int)left * 8; w >>= (32 - got); }   // the last, partial word: only its bytes count
            acc = (acc << got) | w;
            nbits += got;
            pos += 4;
        }
    }
    __device__ __forceinline__ uint32_t bit()
    {
        if (!nbits) { fill(); if (!nbits) return 0; }
        --nbits;
        return (uint32_t)((acc >> nbits) & 1u);
    }
    __device__ __forceinline__ uint64_t get(int bits)                 // bits <= 32
    {
        if (!bits) return 0;
        if (nbits < bits) fill();
        if (nbits < bits) { const int miss = bits - nbits; acc <<= miss; nbits += miss; }   // zero padding
        nbits -= bits;
        return (acc >> nbits) & ((1ull << bits) - 1);
    }
    __device__ __forceinline__ uint64_t get_wide(int bits)
    {
        if (bits > 32) { const uint64_t hi = get(bits - 32) << 32; return hi + get(32); }
        return get(bits);
    }
    __device__ __forceinline__ uint64_t golomb_rice(int k)            // membuf.cpp:228-240
    {
        if (nbits < 33) fill();
        uint64_t p;
        if (nbits >= 33) {
            const uint64_t top = acc << (64 - nbits);
            p = (uint64_t)__builtin_clzll(~top | (1ull << 30));      // leading ones, at most 33 counted
            if (p >= 32) { nbits -= 32; return get(32); }
            nbits -= (int)p + 1;
        } else {
            p = 0;
            while (bit()) { if (++p >= 32) return get(32); }
        }
        return (p << k) + get(k);
    }
};

// How the decoded symbols leave (OUT_*). A lane decodes its own segment, so a wave's store of one symbol per lane touches 64
// different lines, four bytes each. While few lanes are in flight (one frame: 82 k) the L2 gathers a lane's consecutive symbols
// into whole lines before they go to HBM; with the steps of a frame decoded together (738 k lanes, 8 waves per SIMD) the
// half-written lines no longer fit and leave early: 35.4 GB of HBM writes for 6.05 GB of symbols (rocprofv3 WRITE_SIZE,
// profiles/r04b_rlgr_batch_sq_counters.txt), and that traffic -- not the instruction stream -- was the decoder's time.
// OUT_LDS: a lane parks its symbols in a 16-word column of LDS ([16][64] words: the bank is the lane, no conflicts) and
// writes them as one aligned 64-byte piece (4 x 16 bytes, back to back) whenever the column is full. Needs unit symbol stride
// and 16-byte aligned segment starts.
enum { OUT_WORD = 0, OUT_LDS = 2 };
constexpr int DEC_LDS_WORDS = 16 * 64;

template <int OUT, bool LDSIN = false>
__device__ __forceinline__ void decode_segment(const uint32_t *in32, uint32_t nbytes, int n, int flag_signed, int32_t *__restrict__ seq, int64_t sstr = 1,
                                               int32_t *lds = nullptr, int32_t *lds_in = nullptr, int64_t hi_words = 0)
{
    DevBitReaderT<LDSIN> r;
    r.in32 = in32; r.size = nbytes;
    if (LDSIN) { r.col = (uint32_t *)lds_in + (threadIdx.x & 63); r.w0 = (uint32_t)(((uintptr_t)in32 & 31) >> 2); r.hi_words = hi_words; }
    // 32-bit state, as in the encoder: inside a segment of n < 2^31 symbols of int32 data the symbol values (< 2^32), the run
    // length m and the exponents stay within 32 bits; a corrupt stream may overflow them -- it then decodes to different garbage
    // than a 64-bit decoder would, inside the same bounds (every store is at i < n, every read below `size`).
    uint32_t k_P = 0, k_RP = 2 * L;
    int i = 0;
    int32_t *col = lds + (threadIdx.x & 63);                          // OUT_LDS: this lane's column
    auto emit = [&](int32_t v) {
        if (OUT == OUT_LDS) {
            col[(i & 15) * 64] = v;
            ++i;
            if ((i & 15) == 0) {                                     // the column is full: one aligned 64-byte piece
                int4 x[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) x[q] = make_int4(col[(4 * q) * 64], col[(4 * q + 1) * 64], col[(4 * q + 2) * 64], col[(4 * q + 3) * 64]);
#pragma unroll
                for (int q = 0; q < 4; ++q) *(int4 *)(seq + i - 16 + 4 * q) = x[q];
            }
        } else {
            seq[(int64_t)i * sstr] = v;
            ++i;
        }
    };
    while (i < n) {                                                  // membuf.cpp:270-331
        uint32_t k = k_P / L;
        const uint32_t k_R = k_RP / L;
        if (k) {
            uint32_t m = 0;
            while (r.bit()) {
                if (k >= 31) { m = (uint32_t)n; break; }             // corrupt stream guard (a run of 2^31 zeros in one segment)
                m += 1u << k;
                k_P += U1;
                k = k_P / L;
                if (m > (uint32_t)n) break;                          // corrupt stream guard
            }
            m += (uint32_t)r.get_wide((int)min(k, 32u));
            while (m-- && i < n) emit(0);
            if (i >= n) break;
        }
        // ONE Golomb-Rice site for both modes (a run's closing symbol is coded minus one and always steps k_P down)
        const bool closing = k != 0;
        const uint32_t u = (uint32_t)r.golomb_rice((int)k_R);
        const uint32_t uu = closing ? u + 1u : u;
        emit(flag_signed ? ((uu & 1u) ? -(int32_t)(uu >> 1) - 1 : (int32_t)(uu >> 1)) : (int32_t)uu);
        const uint32_t p = (k_R < 32) ? (u >> k_R) : 0u;
        RLGS_ADAPT_KRP32(p);
        if (closing || u) k_P = k_P ? k_P - 1u : 0u;                 // D0 = D1 = 1
        else k_P += U0;
    }
    if (OUT == OUT_LDS && (i & 15)) {                                // the last, partial column
        const int b = i & ~15;
        for (int q = 0; q < (i & 15); ++q) seq[b + q] = col[q * 64];
    }
}

// SYMBOL-SYNCHRONOUS decoding (row-major output). decode_segment above lets every lane run ahead on its own: a lane in a run of
// zeros emits them in an inner loop while the wave's other lanes wait, and the lanes of a wave are at different symbols at any
// time -- in a row-major layout their stores then hit 64 different rows. Here every iteration of the wave produces symbol i of
// EVERY lane: a lane inside a run just counts it down (its zeros cost nothing beside the other lanes' codes), a lane that starts a
// run reads the run's header and emits its first zero, everybody else decodes one Golomb-Rice code (the run's closing symbol
// and an ordinary symbol share that code path; they differ by selects). The lanes of a wave are neighbouring channels at the
// SAME row, so the store of an iteration is one contiguous piece of a row: no LDS staging, no transpose behind the decoder.
// Same streams, same symbols (membuf.cpp:270-331 with the run's state carried across iterations: z zeros still to come, tail = its
// closing symbol still to decode -- not decoded when the segment ends first, as in the original's break).
// expect (may be NULL): what the symbols should be, same layout as seq -- the drivers' round-trip assertion
// (python/encode_3dgs.py:242-245) inside the decoder: in this layout the comparison is one more contiguous read per iteration.
// -> true when a symbol differs.
template <int RMODE>
__device__ __forceinline__ bool decode_segment_sync(const uint32_t *in32, uint32_t nbytes, int n, int flag_signed, int32_t *__restrict__ seq, int64_t sstr,
                                                    int32_t *lds_in = nullptr, int64_t hi_words = 0, const int32_t *__restrict__ expect = nullptr)
{
    bool differs = false;
    DevBitReaderT<RMODE> r;
    r.in32 = in32; r.size = nbytes;
    if (RMODE != 0) { r.col = (uint32_t *)lds_in + (threadIdx.x & 63); r.w0 = (uint32_t)(((uintptr_t)in32 & 31) >> 2); r.hi_words = hi_words; }
    uint32_t k_P = 0, k_RP = 2 * L, z = 0;
    bool tail = false;
    int32_t *wp = seq;                                               // (walked by pointer: a 64-bit multiply per symbol otherwise)
    const int32_t *ep = expect;
    for (int i = 0; i < n; ++i, wp += sstr) {
        if (RMODE == 2 && (i & 31) == 0) r.top_up();
        int32_t v = 0;
        if (z) {
            --z;
        } else {
            bool code = true;
            if (!tail) {
                uint32_t k = k_P / L;
                if (k) {                                             // a run starts: its header
                    uint32_t m = 0;
                    while (r.bit()) {
                        if (k >= 31) { m = (uint32_t)n; break; }     // corrupt stream guard (a run of 2^31 zeros in one segment)
                        m += 1u << k;
                        k_P += U1;
                        k = k_P / L;
                        if (m > (uint32_t)n) break;                  // corrupt stream guard
                    }
                    m += (uint32_t)r.get_wide((int)min(k, 32u));
                    tail = true;
                    if (m) { z = m - 1; code = false; }              // this iteration emits the first of its zeros
                }
            }
            if (code) {
                const uint32_t k_R = k_RP / L;
                const uint32_t u = (uint32_t)r.golomb_rice((int)k_R);
                const uint32_t uu = tail ? u + 1u : u;               // (membuf.cpp: the symbol that ends a run is coded minus one)
                v = flag_signed ? ((uu & 1u) ? -(int32_t)(uu >> 1) - 1 : (int32_t)(uu >> 1)) : (int32_t)uu;
                const uint32_t p = (k_R < 32) ? (u >> k_R) : 0u;
                RLGS_ADAPT_KRP32(p);
                if (tail || u) k_P = k_P ? k_P - 1u : 0u;            // D0 = D1 = 1
                else k_P += U0;
                tail = false;
            }
        }
        *wp = v;
        if (expect) { differs |= *ep != v; ep += sstr; }
    }
    return differs;
}
static_assert(D0 == 1 && D1 == 1, "decode_segment_sync folds the two decrements");

// Which way the decoded symbols leave (see OUT_*): by the number of lanes in flight. One 3 M x 56 frame (82 k lanes, 1.25 waves
// per SIMD) is bound by ONE wave's instruction stream and the L2 still gathers its lines: OUT_WORD 2.86 ms, OUT_LDS 3.36 ms. Nine
// such frames by one launch (738 k lanes): OUT_WORD 1.76 ms per frame (HBM writes 5.9 x the symbols), OUT_LDS 0.99 ms. (Four
// symbols buffered in registers and stored as 16 bytes: 3.97 ms and 1.81 ms -- the component selects cost more than the stores
// save.) The words of the encoder's streams go the same way on their way into the slots (DevBitWriter). The tests force a mode
// through raht_debug_rlgr_decode_out / _encode_out: their frames are far too small to reach the LDS columns by themselves.
constexpr int64_t LDS_FROM_LANES = 200000;
static int g_decode_out = -1;                                       // raht_debug_rlgr_decode_out: -1, OUT_WORD or OUT_LDS
static int g_encode_out = -1;                                       // raht_debug_rlgr_encode_out: the same
static int decode_out_mode(int64_t lanes) { return g_decode_out >= 0 ? g_decode_out : lanes >= LDS_FROM_LANES ? OUT_LDS : OUT_WORD; }
static bool encode_lds_out(int64_t lanes) { return g_encode_out >= 0 ? g_encode_out == OUT_LDS : lanes >= LDS_FROM_LANES; }

// row-major output comes from the symbol-synchronous decoder; raht_debug_rlgr_decode_out(4) / (3) switch to the per-lane one with
// strided stores and back, for the tests
static int g_decode_sync = -1;
static bool decode_sync_rows() { return g_decode_sync != 0; }

// The offset tables come in two widths (OffT): uint32_t -- containers below 4 GiB, the raht_rlgr_seg_* entry points -- and
// uint64_t -- the raht_rlgr_seg_*64 ones, for frames whose worst case is larger. Lengths stay uint32 (one segment is at most
// 16 + 13 seg_len bytes). A kernel loads its offset in the table's width and from there on carries it in 64 bits, as the 32-bit
// kernels always did: the two instantiations differ by that load (and the store of seg_off[G]). The flag words of frame j:
// [overflow bits, container bytes] for 32-bit tables, [overflow bits, -, container bytes (64 bits, 8-byte aligned)] for 64-bit ones.
template <typename OffT> struct SegFlags;
template <> struct SegFlags<uint32_t> {
    static constexpr int WORDS = 2;
    static __host__ __device__ __forceinline__ uint32_t *total(uint32_t *flags, int j) { return flags + 2 * j + 1; }
};
template <> struct SegFlags<uint64_t> {
    static constexpr int WORDS = 4;
    static __host__ __device__ __forceinline__ uint64_t *total(uint32_t *flags, int j) { return (uint64_t *)(flags + 4 * j + 2); }
};

// The two EXACT passes over one frame (thread -> segment: SegLane): WRITE = false sizes every segment; WRITE = true, behind the
// offset scan, writes it at its place in the container.
template <bool WRITE, typename OffT = uint32_t>
__global__ __launch_bounds__(64) void seg_encode_kernel(const int32_t *__restrict__ Q, int64_t N, int D, int64_t sym_stride, int64_t chan_stride, int S, int nseg,
                                                        int flag_signed, uint32_t *__restrict__ seg_bytes, const OffT *__restrict__ seg_off,
                                                        uint8_t *__restrict__ out, uint64_t cap, uint32_t *__restrict__ overflow)
{
    SegLane ln;
    if (!ln.init(N, D, S, nseg, sym_stride != 1)) return;
    const int32_t *seq = Q + ln.at(sym_stride, chan_stride);
    const bool vec = seg_aligned16(Q, sym_stride, chan_stride, S);
    if (!WRITE) {
        seg_bytes[ln.g] = vec ? encode_segment<false, true>(seq, ln.n, flag_signed, nullptr) : encode_segment<false, false>(seq, ln.n, flag_signed, nullptr, 0xffffffffu, sym_stride);
    } else {
        const uint64_t off = seg_off[ln.g];                           // 4-byte aligned
        const uint32_t need = (seg_bytes[ln.g] + 3u) & ~3u;
        if (off + need > cap) { atomicOr(overflow, 1u); return; }
        if (vec) (void)encode_segment<true, true>(seq, ln.n, flag_signed, (uint32_t *)(out + off));
        else (void)encode_segment<true, false>(seq, ln.n, flag_signed, (uint32_t *)(out + off), 0xffffffffu, sym_stride);
    }
}

// a segment whose table entry reaches outside the buffer: n zeros, and nothing is read (raht.h: "decodes as zeros". An empty
// RLGR stream is not that: zero bits decode to a pattern of 0 and -1)
__device__ __forceinline__ void zero_segment(int32_t *__restrict__ seq, int n, int64_t sstr)
{
    for (int i = 0; i < n; ++i, seq += sstr) *seq = 0;
}

// ---- k frames in one set of launches (blockIdx.y = frame) ------------------------------------------------------------
// What bounds the coders is the number of independent lanes: one frame (3 M x 56 at 2048 symbols per segment) is 1.25 waves
// per SIMD, and a wave that is alone on its SIMD waits out the latency of every one of its ~480 k dependent instructions.
// The quantization steps of a frame (python/encode_3dgs.py:199-275: nine of them) are nine such frames of the same shape with
// nothing between them: coded by ONE launch they fill every wave slot of the chip. Each frame keeps its own tables and
// container. The one-frame entry points are k = 1 of the same kernels: the bytes of a frame cannot depend on its company.
// The frames of a SEQUENCE (a different voxel count in every frame, D and seg_len shared) go the same way: the job tables below
// are the only place where a kernel learns a frame's shape -- N, nseg and the strides are per frame, the grid is as wide as the
// largest frame needs and a lane past the end of ITS frame leaves through SegLane::init, as the lanes of a last, partial
// workgroup always did. The frames of one shape are the ragged launch with N[j] = N: there is no instantiation of their own.
// K: the entries of the job table a kernel is built for. RAHT_RLGR_BATCH_MAX: a batch. 1: the one-frame entry points' own instantiation
// -- no blockIdx.y, a table of one entry and, in the decoder, neither the comparison with expect[] nor the stream words' way
// through LDS: a lone wave per SIMD pays for every instruction on its chain (measured with the batch instantiation on one 3 M x 56
// frame: decode 1.73 -> 1.77 ms).
template <typename OffT, int K>
struct SegEncJobs {
    const int32_t *Q[K]; uint32_t *seg_bytes[K]; OffT *seg_off[K]; uint8_t *out[K];
    uint64_t cap[K];
    int64_t N[K], sym_stride[K], chan_stride[K];
    int64_t slot0[K];                            // the frame's first slot of the scratch (and entry of `padded`): G of the frames before it
    int nseg[K];
};
template <typename OffT, int K>
struct SegDecJobs {
    const uint8_t *in[K]; uint64_t in_bytes[K]; const OffT *seg_off[K]; const uint32_t *seg_bytes[K];
    int32_t *Q[K];
    const int32_t *expect[K];                    // (may be NULL) what Q[j] should become: compared inside the row-major decoder (K > 1)
    int64_t N[K], sym_stride[K], chan_stride[K];
    int nseg[K];
};
template <int K> __device__ __forceinline__ int seg_frame() { return K == 1 ? 0 : (int)blockIdx.y; }

// ONE encoding pass: every segment into a fixed slot of `slot` bytes (what the raw integers would take, + 16) of a scratch buffer, its exact length recorded; seg_compact_kernel then moves the streams to their places in the
// containers. A segment that does not fit its slot (incompressible data) raises bit 0 of its frame's flag words and the caller
// falls back to the two exact passes. flags: SegFlags<OffT>::WORDS words per frame (overflow bits, container bytes).
// LDSOUT: the streams' words leave through LDS columns (DevBitWriter; the host's choice: encode_lds_out).
template <typename OffT, int K, bool LDSOUT>
__global__ __launch_bounds__(64) void seg_encode_slots_kernel(const SegEncJobs<OffT, K> J, int D, int S, int flag_signed, uint8_t *__restrict__ slots, uint32_t slot,
                                                              uint32_t *__restrict__ flags)
{
    uint32_t *col = nullptr;
    if constexpr (LDSOUT) {
        __shared__ uint32_t s_col[16 * 64];
        col = s_col;
    }
    const int j = seg_frame<K>();
    const int64_t sym_stride = J.sym_stride[j], chan_stride = J.chan_stride[j];
    SegLane ln;
    if (!ln.init(J.N[j], D, S, J.nseg[j], sym_stride != 1)) return;
    const int32_t *Q = J.Q[j];
    const int32_t *seq = Q + ln.at(sym_stride, chan_stride);
    uint32_t *o = (uint32_t *)(slots + ((size_t)J.slot0[j] + (size_t)ln.g) * slot);
    const uint32_t nb = seg_aligned16(Q, sym_stride, chan_stride, S) ? encode_segment<true, true, LDSOUT>(seq, ln.n, flag_signed, o, slot, 1, col)
                                                                     : encode_segment<true, false, LDSOUT>(seq, ln.n, flag_signed, o, slot, sym_stride, col);
    J.seg_bytes[j][ln.g] = nb;
    if (((nb + 3u) & ~3u) > slot) atomicOr(flags + SegFlags<OffT>::WORDS * j, 1u);
}

// padded size of every segment (its place in the container): the input of the offset scan
template <typename OffT, int K>
__global__ void seg_pad_kernel(const SegEncJobs<OffT, K> J, int D, uint32_t *__restrict__ padded)
{
    const int j = seg_frame<K>();
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g < (int64_t)D * J.nseg[j]) padded[(size_t)J.slot0[j] + g] = (J.seg_bytes[j][g] + 3u) & ~3u;
}

// one wave per segment: its words from the slot to its offset in the container
// (also closes every frame's offset table: seg_off[G] = its container's bytes, left in the frame's flag words by the scan)
template <typename OffT, int K>
__global__ __launch_bounds__(256) void seg_compact_kernel(const SegEncJobs<OffT, K> J, const uint8_t *__restrict__ slots, uint32_t slot, int D,
                                                          uint32_t *__restrict__ flags)
{
    const int j = seg_frame<K>();
    const int64_t G = (int64_t)D * J.nseg[j];
    const int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (blockIdx.x == 0 && threadIdx.x == 0) J.seg_off[j][G] = *SegFlags<OffT>::total(flags, j);
    if (g >= G) return;
    const uint32_t nw = (J.seg_bytes[j][g] + 3u) >> 2;
    if (4ull * nw > slot) return;                                     // it outgrew its slot (the encoder raised the flag): nothing of it is there
    const uint64_t off = J.seg_off[j][g];
    if (off + 4ull * nw > J.cap[j]) { if (lane == 0) atomicOr(flags + SegFlags<OffT>::WORDS * j, 2u); return; }
    const uint32_t *src = (const uint32_t *)(slots + ((size_t)J.slot0[j] + (size_t)g) * slot);
    uint32_t *dst = (uint32_t *)(J.out[j] + off);
    for (uint32_t i = lane; i < nw; i += 64) dst[i] = src[i];
}

// bad: bit j when a table entry of frame j reached outside in[j]; bit 16 + j when a symbol of frame j differs from expect[j]
template <typename OffT, int K>
__global__ __launch_bounds__(64) void seg_decode_kernel(const SegDecJobs<OffT, K> J, int D, int S, int flag_signed, uint32_t *__restrict__ bad, int out_mode,
                                                        int sync_rows)
{
    __shared__ int32_t s_col[DEC_LDS_WORDS];
    const int j = seg_frame<K>();
    const int64_t sym_stride = J.sym_stride[j], chan_stride = J.chan_stride[j];
    SegLane ln;
    if (!ln.init(J.N[j], D, S, J.nseg[j], sym_stride != 1)) return;
    const uint64_t off = J.seg_off[j][ln.g], in_bytes = J.in_bytes[j];
    const uint32_t nb = J.seg_bytes[j][ln.g];
    const int64_t at = ln.at(sym_stride, chan_stride);
    int32_t *seq = J.Q[j] + at;
    if (!seg_entry_ok(off, nb, in_bytes)) {
        if (bad) atomicOr(bad, 1u << j);
        zero_segment(seq, ln.n, sym_stride);
        return;
    }
    const bool aligned = seg_aligned16(J.Q[j], sym_stride, chan_stride, S);
    const uint64_t o = nb ? off : 0;
    const uint32_t *in32 = (const uint32_t *)(J.in[j] + o);
    if constexpr (K > 1) {
        __shared__ int32_t s_in[8 * 64];
        if (sym_stride != 1 && (sync_rows || J.expect[j])) {
            const int32_t *ex = J.expect[j] ? J.expect[j] + at : nullptr;
            const bool differs = decode_segment_sync<2>(in32, nb, ln.n, flag_signed, seq, sym_stride, s_col, 0, ex);
            if (__ballot(differs) && (threadIdx.x & 63) == 0 && bad) atomicOr(bad, 1u << (16 + j));
            return;
        }
        if (aligned && out_mode == OUT_LDS && (((uintptr_t)J.in[j]) & 31) == 0) {             // (the LDSIN reader fetches aligned 32-byte pieces)
            decode_segment<OUT_LDS, true>(in32, nb, ln.n, flag_signed, seq, 1, s_col, s_in, (int64_t)((in_bytes - o) >> 2));
            return;
        }
    } else if (sym_stride != 1 && sync_rows) {
        decode_segment_sync<2>(in32, nb, ln.n, flag_signed, seq, sym_stride, s_col);
        return;
    }
    if (aligned && out_mode == OUT_LDS) decode_segment<OUT_LDS>(in32, nb, ln.n, flag_signed, seq, 1, s_col);
    else decode_segment<OUT_WORD>(in32, nb, ln.n, flag_signed, seq, sym_stride);
}

}  // namespace rlgr_seg
}  // namespace raht

using namespace raht;

namespace {

using rlgr_seg::SegFlags;

template <typename OffT> int scan_offsets(const uint32_t *padded, OffT *off, int64_t n, OffT *total, hipStream_t s);
template <> inline int scan_offsets<uint32_t>(const uint32_t *padded, uint32_t *off, int64_t n, uint32_t *total, hipStream_t s)
{
    return exclusive_scan_u32(padded, off, n, total, s);
}
template <> inline int scan_offsets<uint64_t>(const uint32_t *padded, uint64_t *off, int64_t n, uint64_t *total, hipStream_t s)
{
    return exclusive_scan_u32_u64(padded, off, n, total, s);
}

// frame j's container bytes out of the flag words as they were read back
template <typename OffT> inline uint64_t total_of(const uint32_t *back, int j)
{
    const uint32_t *w = back + SegFlags<OffT>::WORDS * j;
    return sizeof(OffT) == 8 ? ((uint64_t)w[3] << 32) | w[2] : (uint64_t)w[1];
}

// nseg and G of a shape (N, D >= 1, seg_len >= 64) -> the width its offsets need, as raht_rlgr_seg_offsets_width answers it: 32
// when the container stays below 4 GiB whatever the data (worst case: every symbol escapes -- 8 bytes and a bit,
// raht_rlgr_bound(seg_len) per segment -- plus the 4-byte padding of every segment), 64 otherwise. 0: too many segments
// (nseg, G are not set); -1: the length of a segment may not fit 32 bits (the lengths stay uint32 in either table).
int shape_width(int64_t N, int D, int seg_len, int64_t *nseg, int64_t *G)
{
    *nseg = (N - 1) / seg_len + 1;
    if (*nseg >= ((int64_t)1 << 31) || *nseg * D >= ((int64_t)1 << 31)) return 0;
    *G = *nseg * D;
    const int64_t per_seg = raht_rlgr_bound(seg_len) + 4;                       // < 2^35
    if (per_seg - 4 >= ((int64_t)1 << 32)) return -1;
    return per_seg * *G >= ((int64_t)1 << 32) ? 64 : 32;                        // (< 2^66 / 2: G < 2^31, per_seg < 2^32 -- no overflow)
}

// What the host knows of the k frames of a call: every frame's shape, and where its slots begin (the running sum of G)
struct SegFrames {
    int k = 0;
    int64_t N[RAHT_RLGR_BATCH_MAX], sym_stride[RAHT_RLGR_BATCH_MAX], chan_stride[RAHT_RLGR_BATCH_MAX];
    int64_t nseg[RAHT_RLGR_BATCH_MAX], G[RAHT_RLGR_BATCH_MAX], slot0[RAHT_RLGR_BATCH_MAX];
    int64_t sumG = 0, maxG = 0;

    void add(int64_t n, int64_t sym, int64_t chan, int64_t ns, int64_t g)       // (k < RAHT_RLGR_BATCH_MAX; ns, g: shape_width's)
    {
        N[k] = n; sym_stride[k] = sym; chan_stride[k] = chan; nseg[k] = ns; G[k] = g;
        slot0[k] = sumG;
        sumG += g;
        maxG = g > maxG ? g : maxG;
        ++k;
    }
    SegFrames one(int j) const { SegFrames F1; F1.add(N[j], sym_stride[j], chan_stride[j], nseg[j], G[j]); return F1; }   // frame j alone
    // the shape of frame j < K into a job table (the entries behind k repeat frame 0: no kernel reads them)
    template <typename Jobs> void fill(Jobs &J, int j) const
    {
        const int q = j < k ? j : 0;
        J.N[j] = N[q]; J.sym_stride[j] = sym_stride[q]; J.chan_stride[j] = chan_stride[q]; J.nseg[j] = (int)nseg[q];
    }
};

// the kernels' view of k <= K frames (the entries behind k repeat frame 0: no kernel reads them)
template <typename OffT, int K>
rlgr_seg::SegEncJobs<OffT, K> enc_jobs(const SegFrames &F, const int32_t *const *Q, uint32_t *const *seg_bytes, OffT *const *seg_off, uint8_t *const *out, const int64_t *cap)
{
    rlgr_seg::SegEncJobs<OffT, K> J;
    for (int j = 0; j < K; ++j) {
        const int q = j < F.k ? j : 0;
        J.Q[j] = Q[q]; J.seg_bytes[j] = seg_bytes[q]; J.seg_off[j] = seg_off[q]; J.out[j] = out[q]; J.cap[j] = (uint64_t)cap[q];
        J.slot0[j] = F.slot0[q];
        F.fill(J, j);
    }
    return J;
}

template <typename OffT, int K>
rlgr_seg::SegDecJobs<OffT, K> dec_jobs(const SegFrames &F, const uint8_t *const *in, const int64_t *in_bytes, const OffT *const *seg_off, const uint32_t *const *seg_bytes,
                                       int32_t *const *Q, const int32_t *const *expect)
{
    rlgr_seg::SegDecJobs<OffT, K> J;
    for (int j = 0; j < K; ++j) {
        const int q = j < F.k ? j : 0;
        J.in[j] = in[q]; J.in_bytes[j] = (uint64_t)in_bytes[q]; J.seg_off[j] = seg_off[q]; J.seg_bytes[j] = seg_bytes[q]; J.Q[j] = Q[q];
        J.expect[j] = expect ? expect[q] : nullptr;
        F.fill(J, j);
    }
    return J;
}

// The k frames of a call as an entry point was handed them -> F, checked. D and seg_len are shared; N and the two strides are one
// value for all frames (per_frame false: one frame, or k of one shape) or one per frame. Every frame is channel-major (sym_stride
// 1, chan_stride >= N) or row-major (chan_stride 1, sym_stride >= D), all frames of a call the same; no frame has too many
// segments or needs offsets wider than `widest` (32: what raht_rlgr_seg_offsets_width calls 64 is refused -- segment offsets and
// the container's total could wrap; a decoder whose offsets came with its container takes either).
int seg_frames(const char *fn, int widest, int k, const int64_t *N, const int64_t *sym_stride, const int64_t *chan_stride, bool per_frame, int D, int seg_len,
               SegFrames *F)
{
    if (k < 1 || k > RAHT_RLGR_BATCH_MAX || !N || !sym_stride || !chan_stride || D < 1 || seg_len < 64) {
        set_error("%s: bad argument (1 <= k <= %d, D >= 1, seg_len >= 64)", fn, RAHT_RLGR_BATCH_MAX);
        return RAHT_ERR_INVALID;
    }
    bool all_cm = true, all_rm = true;
    for (int j = 0; j < k; ++j) {
        const int q = per_frame ? j : 0;
        const int64_t n = N[q], sym = sym_stride[q], chan = chan_stride[q];
        char who[24] = "";
        if (per_frame) snprintf(who, sizeof(who), "frame %d: ", j);
        const bool cm = n >= 1 && sym == 1 && chan >= n, rm = n >= 1 && chan == 1 && sym >= D;
        if (!cm && !rm) {
            set_error("%s: bad argument (%sN >= 1; channel-major: sym_stride 1, chan_stride >= N; row-major: chan_stride 1, sym_stride >= D)", fn, who);
            return RAHT_ERR_INVALID;
        }
        all_cm = all_cm && cm;
        all_rm = all_rm && rm;
        int64_t nseg, G;
        const int width = shape_width(n, D, seg_len, &nseg, &G);
        if (width == 0) { set_error("%s: %stoo many segments", fn, who); return RAHT_ERR_INVALID; }
        if (width < 0) { set_error("%s: seg_len = %d: the length of a segment may not fit 32 bits", fn, seg_len); return RAHT_ERR_INVALID; }
        if (width > widest) {
            set_error("%s: %s%lld x %d symbols may need a container of 4 GiB or more (32-bit segment offsets): code it alone, with 64-bit offsets", fn, who, (long long)n, D);
            return RAHT_ERR_INVALID;
        }
        F->add(n, sym, chan, nseg, G);
    }
    if (!all_cm && !all_rm) { set_error("%s: the frames of a call are all channel-major or all row-major", fn); return RAHT_ERR_INVALID; }
    return RAHT_OK;
}

// the tables of an encode call: every frame's input, tables and container (cap >= 16 bytes, 4-byte aligned)
template <typename OffT>
int enc_tables_ok(const char *fn, const SegFrames &F, const int32_t *const *Q, uint32_t *const *seg_bytes, OffT *const *seg_off, uint8_t *const *out, const int64_t *cap,
                  const int64_t *total_bytes)
{
    if (!Q || !seg_bytes || !seg_off || !out || !cap || !total_bytes) { set_error("%s: bad argument (a table is NULL)", fn); return RAHT_ERR_INVALID; }
    for (int j = 0; j < F.k; ++j)
        if (!Q[j] || !seg_bytes[j] || !seg_off[j] || !out[j] || cap[j] < 16 || ((uintptr_t)out[j] & 3)) { set_error("%s: bad argument (frame %d)", fn, j); return RAHT_ERR_INVALID; }
    return RAHT_OK;
}

// the tables of a decode call: every frame's streams (4-byte aligned, a multiple of 4 bytes long), tables and output; with
// expect[] (its faults report as fnx) bad_dev, row-major frames and every expect[j]
template <typename OffT>
int dec_tables_ok(const char *fn, const char *fnx, const SegFrames &F, int D, const uint8_t *const *in, const int64_t *in_bytes, const OffT *const *seg_off,
                  const uint32_t *const *seg_bytes, int32_t *const *Q, const int32_t *const *expect, const uint32_t *bad_dev)
{
    if (!in || !in_bytes || !seg_off || !seg_bytes || !Q) { set_error("%s: bad argument (a table is NULL)", fn); return RAHT_ERR_INVALID; }
    for (int j = 0; j < F.k; ++j) {
        if (!in[j] || in_bytes[j] < 0 || (in_bytes[j] & 3) || ((uintptr_t)in[j] & 3) || !seg_off[j] || !seg_bytes[j] || !Q[j]) {
            set_error("%s: bad argument (frame %d)", fn, j);
            return RAHT_ERR_INVALID;
        }
        if (expect && (!bad_dev || F.chan_stride[j] != 1 || F.sym_stride[j] < D || !expect[j])) {
            set_error("%s: expect[] needs bad_dev, row-major frames (chan_stride 1) and every expect[j] (frame %d)", fnx, j);
            return RAHT_ERR_INVALID;
        }
    }
    return RAHT_OK;
}

// a slot: what the raw integers of a segment would take, + 16; for the LDS-column output in whole 64-byte pieces (it needs
// 16-byte aligned starts; 64: whole pieces). Fits: raht_rlgr_bound(seg_len) < 2^32.
inline uint32_t slot_bytes(int seg_len, bool lds_out) { return lds_out ? (4u * (uint32_t)seg_len + 16u + 63u) & ~63u : 4u * (uint32_t)seg_len + 16u; }

// The slots pass over the frames of J / F: every segment into its slot, the padded sizes, one offset scan per frame, the compaction
// (which closes the frames' tables), the flag words back (synchronises: the scratch may go back to the pool). The grid is as wide
// as the largest frame; the lanes in flight -- which decide between words and LDS columns -- are those of all frames together.
//   RAHT_OK              total_bytes[] are set and the containers written
//   RAHT_ERR_NOMEM       total_bytes[] are set and some container is too small (the text names the frame when name_frame)
//   RAHT_ERR_UNSUPPORTED a segment outgrew its slot (incompressible data), or there is no scratch for the slots: nothing
//                        useful was written and the caller runs the two exact passes
template <typename OffT, int K>
int seg_encode_slots(const char *fn, bool name_frame, const rlgr_seg::SegEncJobs<OffT, K> &J, const SegFrames &F, int D, int seg_len, int flag_signed,
                     int64_t *total_bytes, hipStream_t s)
{
    constexpr int FW = SegFlags<OffT>::WORDS;
    const int k = F.k;
    const bool lds_out = rlgr_seg::encode_lds_out(F.sumG);
    const uint32_t slot = slot_bytes(seg_len, lds_out);
    const size_t npad = ((size_t)F.sumG + 1) & ~(size_t)1;                  // (the flag words behind it stay 8-byte aligned)
    Scratch tmp(sizeof(uint32_t) * (npad + FW * (size_t)k), s);
    Scratch slots((size_t)F.sumG * slot, s);
    if (!tmp.ok() || !slots.ok()) { (void)hipGetLastError(); return RAHT_ERR_UNSUPPORTED; }
    uint32_t *padded = tmp.as<uint32_t>(), *flags = padded + npad;
    RAHT_HIP_CHECK(hipMemsetAsync(flags, 0, 4 * FW * (size_t)k, s));
    const dim3 lanes((unsigned)ceil_div(F.maxG, 64), (unsigned)k);
    if (lds_out)
        hipLaunchKernelGGL((rlgr_seg::seg_encode_slots_kernel<OffT, K, true>), lanes, dim3(64), 0, s, J, D, seg_len, flag_signed, slots.as<uint8_t>(), slot, flags);
    else
        hipLaunchKernelGGL((rlgr_seg::seg_encode_slots_kernel<OffT, K, false>), lanes, dim3(64), 0, s, J, D, seg_len, flag_signed, slots.as<uint8_t>(), slot, flags);
    hipLaunchKernelGGL((rlgr_seg::seg_pad_kernel<OffT, K>), dim3((unsigned)ceil_div(F.maxG, 256), (unsigned)k), dim3(256), 0, s, J, D, padded);
    for (int j = 0; j < k; ++j) RAHT_RET(scan_offsets<OffT>(padded + (size_t)F.slot0[j], J.seg_off[j], F.G[j], SegFlags<OffT>::total(flags, j), s));
    hipLaunchKernelGGL((rlgr_seg::seg_compact_kernel<OffT, K>), dim3((unsigned)ceil_div(F.maxG * 64, 256), (unsigned)k), dim3(256), 0, s, J, (const uint8_t *)slots.as<uint8_t>(), slot, D, flags);
    RAHT_HIP_CHECK(hipGetLastError());
    uint32_t back[FW * K] = {0};
    RAHT_RET(read_back_u32(back, flags, FW * k, nullptr, nullptr, 0, s));
    for (int j = 0; j < k; ++j)
        if (back[FW * j] & 1u) return RAHT_ERR_UNSUPPORTED;
    int rc = RAHT_OK;
    for (int j = 0; j < k; ++j) {
        const uint64_t total = total_of<OffT>(back, j);
        total_bytes[j] = (int64_t)total;
        if ((back[FW * j] & 2u) || total > J.cap[j]) {
            if (name_frame) set_error("%s: frame %d needs %llu bytes, cap = %lld", fn, j, (unsigned long long)total, (long long)J.cap[j]);
            else set_error("%s: %llu bytes needed, cap = %lld", fn, (unsigned long long)total, (long long)J.cap[j]);
            rc = RAHT_ERR_NOMEM;
        }
    }
    return rc;
}

// The one frame of F (arguments checked) through the encoder, with the kernels of one frame
template <typename OffT>
int seg_encode_one(const char *fn, const SegFrames &F, const int32_t *Q, int D, int seg_len, int flag_signed, uint32_t *seg_bytes, OffT *seg_off, uint8_t *out,
                   int64_t cap, int64_t *total_bytes, raht_stream_t stream)
{
    const int64_t N = F.N[0], sym_stride = F.sym_stride[0], chan_stride = F.chan_stride[0], nseg = F.nseg[0], G = F.G[0];
    hipStream_t s = (hipStream_t)stream;
    constexpr int FW = SegFlags<OffT>::WORDS;
    return guarded(fn, [&]() -> int {
        const rlgr_seg::SegEncJobs<OffT, 1> J = enc_jobs<OffT, 1>(F, &Q, &seg_bytes, &seg_off, &out, &cap);
        // ONE encoding pass into fixed slots + a compaction, when a scratch buffer of the raw size is to be had; the two exact
        // passes (sizes, then streams) otherwise, and whenever a segment outgrows its slot
        if ((uint64_t)G * slot_bytes(seg_len, rlgr_seg::encode_lds_out(G)) < ((uint64_t)1 << 33)) {
            const int rc = seg_encode_slots<OffT, 1>(fn, false, J, F, D, seg_len, flag_signed, total_bytes, s);
            if (rc != RAHT_ERR_UNSUPPORTED) return rc;
        }
        const size_t npad = ((size_t)G + 1) & ~(size_t)1;                   // (the flag words behind it stay 8-byte aligned)
        Scratch tmp(sizeof(uint32_t) * (npad + FW), s);
        if (!tmp.ok()) return RAHT_ERR_NOMEM;
        uint32_t *padded = tmp.as<uint32_t>(), *flags = padded + npad;      // flags[0] = overflow, SegFlags::total = total
        OffT *dtotal = SegFlags<OffT>::total(flags, 0);
        RAHT_HIP_CHECK(hipMemsetAsync(flags, 0, 4 * FW, s));
        const unsigned gb = (unsigned)ceil_div(G, 64);
        hipLaunchKernelGGL((rlgr_seg::seg_encode_kernel<false, OffT>), dim3(gb), dim3(64), 0, s, Q, N, D, sym_stride, chan_stride, seg_len, (int)nseg, flag_signed,
                           seg_bytes, (const OffT *)nullptr, (uint8_t *)nullptr, (uint64_t)0, flags);
        hipLaunchKernelGGL((rlgr_seg::seg_pad_kernel<OffT, 1>), dim3((unsigned)ceil_div(G, 256)), dim3(256), 0, s, J, D, padded);
        RAHT_RET(scan_offsets<OffT>(padded, seg_off, G, dtotal, s));
        RAHT_HIP_CHECK(hipMemcpyAsync(seg_off + G, dtotal, sizeof(OffT), hipMemcpyDeviceToDevice, s));
        hipLaunchKernelGGL((rlgr_seg::seg_encode_kernel<true, OffT>), dim3(gb), dim3(64), 0, s, Q, N, D, sym_stride, chan_stride, seg_len, (int)nseg, flag_signed,
                           seg_bytes, (const OffT *)seg_off, out, (uint64_t)cap, flags);
        RAHT_HIP_CHECK(hipGetLastError());
        uint32_t back[FW] = {0};
        RAHT_RET(read_back_u32(back, flags, FW, nullptr, nullptr, 0, s));
        const uint64_t total = total_of<OffT>(back, 0);
        *total_bytes = (int64_t)total;
        if (back[0] || (int64_t)total > cap) { set_error("%s: %llu bytes needed, cap = %lld", fn, (unsigned long long)total, (long long)cap); return RAHT_ERR_NOMEM; }
        return RAHT_OK;
    });
}

// one launch for the k <= K frames of F, whose arguments have been checked
template <typename OffT, int K>
int seg_decode_launch(const SegFrames &F, const uint8_t *const *in, const int64_t *in_bytes, const OffT *const *seg_off, const uint32_t *const *seg_bytes, int D,
                      int seg_len, int flag_signed, int32_t *const *Q, const int32_t *const *expect, uint32_t *bad_dev, raht_stream_t stream)
{
    const rlgr_seg::SegDecJobs<OffT, K> J = dec_jobs<OffT, K>(F, in, in_bytes, seg_off, seg_bytes, Q, expect);
    hipLaunchKernelGGL((rlgr_seg::seg_decode_kernel<OffT, K>), dim3((unsigned)ceil_div(F.maxG, 64), (unsigned)F.k), dim3(64), 0, (hipStream_t)stream, J, D, seg_len,
                       flag_signed, bad_dev, rlgr_seg::decode_out_mode(F.sumG), (int)rlgr_seg::decode_sync_rows());
    RAHT_HIP_CHECK(hipGetLastError());
    return RAHT_OK;
}

// The frames of F (arguments checked) through the encoder: one set of launches, or frame by frame -- a lone frame (its own
// instantiation and its texts) and whenever the slots pass gives up.
// fn: the batch entry point's name; fn1: the one-frame entry point of the same width (the frame-by-frame fallback reports as it)
template <typename OffT>
int seg_encode_frames(const char *fn, const char *fn1, const SegFrames &F, const int32_t *const *Q, int D, int seg_len, int flag_signed, uint32_t *const *seg_bytes,
                      OffT *const *seg_off, uint8_t *const *out, const int64_t *cap, int64_t *total_bytes, raht_stream_t stream)
{
    int rc = RAHT_ERR_UNSUPPORTED;
    if (F.k > 1)
        rc = guarded(fn, [&]() -> int {
            return seg_encode_slots<OffT, RAHT_RLGR_BATCH_MAX>(fn, true, enc_jobs<OffT, RAHT_RLGR_BATCH_MAX>(F, Q, seg_bytes, seg_off, out, cap), F, D, seg_len, flag_signed,
                                                              total_bytes, (hipStream_t)stream);
        });
    if (rc != RAHT_ERR_UNSUPPORTED) return rc;
    int rc_all = RAHT_OK;                                                   // frame by frame
    for (int j = 0; j < F.k; ++j) {
        rc = seg_encode_one<OffT>(fn1, F.one(j), Q[j], D, seg_len, flag_signed, seg_bytes[j], seg_off[j], out[j], cap[j], &total_bytes[j], stream);
        if (rc != RAHT_OK && rc_all == RAHT_OK) rc_all = rc;
        if (rc != RAHT_OK && rc != RAHT_ERR_NOMEM) return rc;
    }
    return rc_all;
}

}  // namespace

extern "C" {

/* Which offset tables a shape needs. HOST arithmetic only. 32: raht_rlgr_seg_encode* take it -- the container stays below 4 GiB
 * whatever the data (worst case: every symbol escapes, 8 bytes and a bit, raht_rlgr_bound(seg_len) per segment, plus the 4-byte
 * padding of every segment). 64: they refuse it and raht_rlgr_seg_encode64 / _batch64 take it. RAHT_ERR_INVALID: nobody does. */
int raht_rlgr_seg_offsets_width(int64_t N, int D, int seg_len)
{
    if (N < 1 || D < 1 || seg_len < 64) { set_error("raht_rlgr_seg_offsets_width: bad argument (N, D >= 1, seg_len >= 64)"); return RAHT_ERR_INVALID; }
    int64_t nseg, G;
    const int width = shape_width(N, D, seg_len, &nseg, &G);
    if (width == 0) { set_error("raht_rlgr_seg_offsets_width: too many segments"); return RAHT_ERR_INVALID; }
    if (width < 0) { set_error("raht_rlgr_seg_offsets_width: seg_len = %d: the length of a segment may not fit 32 bits", seg_len); return RAHT_ERR_INVALID; }
    return width;
}

/* Segmented RLGR on the device. Q: DEVICE int32, channel-major (symbol n of channel c at Q[c * chan_stride + n], what
 * raht_transpose_i32 produces); seg_len symbols per segment (>= 64), nseg = ceil(N / seg_len) segments per channel.
 * Outputs (DEVICE): seg_bytes[D * nseg] = exact byte length of every segment's stream, seg_off[D * nseg + 1] = its offset in
 * `out` (segments are laid out in order, each padded to 4 bytes; seg_off[last] = bytes used), out[cap] = the streams.
 * *total_bytes (HOST) = bytes used. RAHT_ERR_NOMEM when cap is too small (nothing useful in out; 4 N D + 64 D nseg bytes
 * always suffice for data a raw int32 dump would not beat, raht_rlgr_bound(seg_len) * D * nseg for anything). Synchronises. */
int raht_rlgr_seg_encode(const int32_t *Q, int64_t N, int D, int64_t chan_stride, int seg_len, int flag_signed, uint32_t *seg_bytes,
                         uint32_t *seg_off, uint8_t *out, int64_t cap, int64_t *total_bytes, raht_stream_t stream)
{
    if (chan_stride < N) { set_error("raht_rlgr_seg_encode: bad argument"); return RAHT_ERR_INVALID; }
    return raht_rlgr_seg_encode_strided(Q, N, D, 1, chan_stride, seg_len, flag_signed, seg_bytes, seg_off, out, cap, total_bytes, stream);
}

int raht_rlgr_seg_encode_strided(const int32_t *Q, int64_t N, int D, int64_t sym_stride, int64_t chan_stride, int seg_len, int flag_signed,
                                 uint32_t *seg_bytes, uint32_t *seg_off, uint8_t *out, int64_t cap, int64_t *total_bytes, raht_stream_t stream)
{
    const char *fn = "raht_rlgr_seg_encode";
    SegFrames F;
    RAHT_RET(seg_frames(fn, 32, 1, &N, &sym_stride, &chan_stride, false, D, seg_len, &F));
    RAHT_RET(enc_tables_ok(fn, F, &Q, &seg_bytes, &seg_off, &out, &cap, total_bytes));
    return seg_encode_frames<uint32_t>(fn, fn, F, &Q, D, seg_len, flag_signed, &seg_bytes, &seg_off, &out, &cap, total_bytes, stream);
}

/* The same with 64-bit offsets (seg_off: DEVICE uint64[D * nseg + 1]) for the shapes raht_rlgr_seg_offsets_width calls 64 -- and
 * for any other: same seg_bytes, same streams, offsets equal as integers. */
int raht_rlgr_seg_encode64(const int32_t *Q, int64_t N, int D, int64_t sym_stride, int64_t chan_stride, int seg_len, int flag_signed,
                           uint32_t *seg_bytes, uint64_t *seg_off, uint8_t *out, int64_t cap, int64_t *total_bytes, raht_stream_t stream)
{
    const char *fn = "raht_rlgr_seg_encode64";
    SegFrames F;
    RAHT_RET(seg_frames(fn, 64, 1, &N, &sym_stride, &chan_stride, false, D, seg_len, &F));
    RAHT_RET(enc_tables_ok(fn, F, &Q, &seg_bytes, &seg_off, &out, &cap, total_bytes));
    return seg_encode_frames<uint64_t>(fn, fn, F, &Q, D, seg_len, flag_signed, &seg_bytes, &seg_off, &out, &cap, total_bytes, stream);
}

/* The inverse: streams `in` (DEVICE, 4-byte aligned, in_bytes long -- a multiple of 4) with their offsets / lengths (DEVICE, as
 * raht_rlgr_seg_encode wrote them) -> Q (DEVICE, channel-major). Does not synchronise. The tables come off the wire: a
 * segment whose offset / length reaches outside `in` decodes as an empty stream (zeros) and sets *bad_dev (DEVICE uint32,
 * may be NULL) instead of reading there. */
int raht_rlgr_seg_decode(const uint8_t *in, int64_t in_bytes, const uint32_t *seg_off, const uint32_t *seg_bytes, int64_t N, int D, int seg_len,
                         int flag_signed, int32_t *Q, int64_t chan_stride, uint32_t *bad_dev, raht_stream_t stream)
{
    if (chan_stride < N) { set_error("raht_rlgr_seg_decode: bad argument"); return RAHT_ERR_INVALID; }
    return raht_rlgr_seg_decode_strided(in, in_bytes, seg_off, seg_bytes, N, D, seg_len, flag_signed, Q, 1, chan_stride, bad_dev, stream);
}

int raht_rlgr_seg_decode_strided(const uint8_t *in, int64_t in_bytes, const uint32_t *seg_off, const uint32_t *seg_bytes, int64_t N, int D, int seg_len,
                                 int flag_signed, int32_t *Q, int64_t sym_stride, int64_t chan_stride, uint32_t *bad_dev, raht_stream_t stream)
{
    const char *fn = "raht_rlgr_seg_decode";
    SegFrames F;
    RAHT_RET(seg_frames(fn, 64, 1, &N, &sym_stride, &chan_stride, false, D, seg_len, &F));
    RAHT_RET(dec_tables_ok(fn, fn, F, D, &in, &in_bytes, &seg_off, &seg_bytes, &Q, nullptr, bad_dev));
    return seg_decode_launch<uint32_t, 1>(F, &in, &in_bytes, &seg_off, &seg_bytes, D, seg_len, flag_signed, &Q, nullptr, bad_dev, stream);
}

/* ... from 64-bit offsets (the whole offset is checked against in_bytes before anything is read) */
int raht_rlgr_seg_decode64(const uint8_t *in, int64_t in_bytes, const uint64_t *seg_off, const uint32_t *seg_bytes, int64_t N, int D, int seg_len,
                           int flag_signed, int32_t *Q, int64_t sym_stride, int64_t chan_stride, uint32_t *bad_dev, raht_stream_t stream)
{
    const char *fn = "raht_rlgr_seg_decode64";
    SegFrames F;
    RAHT_RET(seg_frames(fn, 64, 1, &N, &sym_stride, &chan_stride, false, D, seg_len, &F));
    RAHT_RET(dec_tables_ok(fn, fn, F, D, &in, &in_bytes, &seg_off, &seg_bytes, &Q, nullptr, bad_dev));
    return seg_decode_launch<uint64_t, 1>(F, &in, &in_bytes, &seg_off, &seg_bytes, D, seg_len, flag_signed, &Q, nullptr, bad_dev, stream);
}

int raht_debug_rlgr_decode_out(int mode)
{
    const int prev = rlgr_seg::g_decode_out;
    if (mode == 3 || mode == 4) { rlgr_seg::g_decode_sync = (mode == 3); return prev; }     // row-major output: symbol-synchronous decoder on / off
    rlgr_seg::g_decode_out = (mode == rlgr_seg::OUT_WORD || mode == rlgr_seg::OUT_LDS) ? mode : -1;
    if (mode < 0) rlgr_seg::g_decode_sync = -1;
    return prev;
}

int raht_debug_rlgr_encode_out(int mode)
{
    const int prev = rlgr_seg::g_encode_out;
    rlgr_seg::g_encode_out = (mode == rlgr_seg::OUT_WORD || mode == rlgr_seg::OUT_LDS) ? mode : -1;
    return prev;
}

/* k frames of one shape (N, D, strides, seg_len) in one set of launches: the quantization steps of a frame coded together.
 * Every frame j has its own input Q[j], tables seg_bytes[j] / seg_off[j], container out[j] of cap[j] bytes and total_bytes[j]:
 * exactly what raht_rlgr_seg_encode_strided leaves for that frame alone (same bytes). Synchronises. RAHT_ERR_NOMEM when a
 * container is too small (total_bytes[] holds what every frame needs). */
int raht_rlgr_seg_encode_batch(int k, const int32_t *const *Q, int64_t N, int D, int64_t sym_stride, int64_t chan_stride, int seg_len, int flag_signed,
                               uint32_t *const *seg_bytes, uint32_t *const *seg_off, uint8_t *const *out, const int64_t *cap, int64_t *total_bytes,
                               raht_stream_t stream)
{
    const char *fn = "raht_rlgr_seg_encode_batch";
    SegFrames F;                                                              // (k frames of ONE shape: the ragged launch with N[j] = N)
    RAHT_RET(seg_frames(fn, 32, k, &N, &sym_stride, &chan_stride, false, D, seg_len, &F));
    RAHT_RET(enc_tables_ok(fn, F, Q, seg_bytes, seg_off, out, cap, total_bytes));
    return seg_encode_frames<uint32_t>(fn, "raht_rlgr_seg_encode", F, Q, D, seg_len, flag_signed, seg_bytes, seg_off, out, cap, total_bytes, stream);
}

int raht_rlgr_seg_encode_batch64(int k, const int32_t *const *Q, int64_t N, int D, int64_t sym_stride, int64_t chan_stride, int seg_len, int flag_signed,
                                 uint32_t *const *seg_bytes, uint64_t *const *seg_off, uint8_t *const *out, const int64_t *cap, int64_t *total_bytes,
                                 raht_stream_t stream)
{
    const char *fn = "raht_rlgr_seg_encode_batch64";
    SegFrames F;
    RAHT_RET(seg_frames(fn, 64, k, &N, &sym_stride, &chan_stride, false, D, seg_len, &F));
    RAHT_RET(enc_tables_ok(fn, F, Q, seg_bytes, seg_off, out, cap, total_bytes));
    return seg_encode_frames<uint64_t>(fn, "raht_rlgr_seg_encode64", F, Q, D, seg_len, flag_signed, seg_bytes, seg_off, out, cap, total_bytes, stream);
}

/* The inverse for k frames of one shape: in[j] / in_bytes[j] / seg_off[j] / seg_bytes[j] -> Q[j], one launch. Does not
 * synchronise. *bad_dev (DEVICE uint32, may be NULL): bit j set when a table entry of frame j reached outside in[j]. */
int raht_rlgr_seg_decode_batch(int k, const uint8_t *const *in, const int64_t *in_bytes, const uint32_t *const *seg_off, const uint32_t *const *seg_bytes,
                               int64_t N, int D, int seg_len, int flag_signed, int32_t *const *Q, int64_t sym_stride, int64_t chan_stride,
                               uint32_t *bad_dev, raht_stream_t stream)
{
    const char *fn = "raht_rlgr_seg_decode_batch";
    SegFrames F;
    RAHT_RET(seg_frames(fn, 64, k, &N, &sym_stride, &chan_stride, false, D, seg_len, &F));
    RAHT_RET(dec_tables_ok(fn, fn, F, D, in, in_bytes, seg_off, seg_bytes, Q, nullptr, bad_dev));
    return seg_decode_launch<uint32_t, RAHT_RLGR_BATCH_MAX>(F, in, in_bytes, seg_off, seg_bytes, D, seg_len, flag_signed, Q, nullptr, bad_dev, stream);
}

/* ... and compares every frame with what it should decode to (expect[j]: DEVICE, the layout and strides of Q[j]; ROW-MAJOR only:
 * chan_stride = 1) on the way: bit 16 + j of *bad_dev (required) is set when a symbol of frame j differs -- the drivers'
 * round-trip assertion (python/encode_3dgs.py:242-245) without a pass of its own over two N x D arrays. */
int raht_rlgr_seg_decode_batch_check(int k, const uint8_t *const *in, const int64_t *in_bytes, const uint32_t *const *seg_off, const uint32_t *const *seg_bytes,
                                     int64_t N, int D, int seg_len, int flag_signed, int32_t *const *Q, const int32_t *const *expect, int64_t sym_stride,
                                     int64_t chan_stride, uint32_t *bad_dev, raht_stream_t stream)
{
    const char *fn = "raht_rlgr_seg_decode_batch", *fnx = "raht_rlgr_seg_decode_batch_check";
    if (!expect) { set_error("%s: needs expect[]", fnx); return RAHT_ERR_INVALID; }
    SegFrames F;
    RAHT_RET(seg_frames(fn, 64, k, &N, &sym_stride, &chan_stride, false, D, seg_len, &F));
    RAHT_RET(dec_tables_ok(fn, fnx, F, D, in, in_bytes, seg_off, seg_bytes, Q, expect, bad_dev));
    return seg_decode_launch<uint32_t, RAHT_RLGR_BATCH_MAX>(F, in, in_bytes, seg_off, seg_bytes, D, seg_len, flag_signed, Q, expect, bad_dev, stream);
}

/* Both of them from 64-bit offsets: expect == NULL decodes (any layout, bad_dev may be NULL); expect != NULL also compares
 * (row-major frames, bad_dev required, every expect[j] set). */
int raht_rlgr_seg_decode_batch64(int k, const uint8_t *const *in, const int64_t *in_bytes, const uint64_t *const *seg_off, const uint32_t *const *seg_bytes,
                                 int64_t N, int D, int seg_len, int flag_signed, int32_t *const *Q, const int32_t *const *expect, int64_t sym_stride,
                                 int64_t chan_stride, uint32_t *bad_dev, raht_stream_t stream)
{
    const char *fn = "raht_rlgr_seg_decode_batch64";
    SegFrames F;
    RAHT_RET(seg_frames(fn, 64, k, &N, &sym_stride, &chan_stride, false, D, seg_len, &F));
    RAHT_RET(dec_tables_ok(fn, fn, F, D, in, in_bytes, seg_off, seg_bytes, Q, expect, bad_dev));
    return seg_decode_launch<uint64_t, RAHT_RLGR_BATCH_MAX>(F, in, in_bytes, seg_off, seg_bytes, D, seg_len, flag_signed, Q, expect, bad_dev, stream);
}

/* k frames of k SHAPES in one set of launches: the frames of a sequence. D, seg_len and flag_signed are shared; N[j] and the two
 * strides are per frame (all frames channel-major or all row-major, each within the rules of raht_rlgr_seg_encode_strided);
 * 32-bit offset tables only: a frame raht_rlgr_seg_offsets_width does not call 32 is refused (RAHT_ERR_INVALID, the text names
 * it). Every frame gets exactly the bytes, seg_bytes, seg_off and total_bytes[j] raht_rlgr_seg_encode_strided leaves for it
 * alone. Synchronises; RAHT_ERR_NOMEM when some cap[j] is too small (total_bytes[] holds what every frame needs). */
int raht_rlgr_seg_encode_ragged(int k, const int32_t *const *Q, const int64_t *N, int D, const int64_t *sym_stride, const int64_t *chan_stride, int seg_len,
                                int flag_signed, uint32_t *const *seg_bytes, uint32_t *const *seg_off, uint8_t *const *out, const int64_t *cap,
                                int64_t *total_bytes, raht_stream_t stream)
{
    const char *fn = "raht_rlgr_seg_encode_ragged";
    SegFrames F;
    RAHT_RET(seg_frames(fn, 32, k, N, sym_stride, chan_stride, true, D, seg_len, &F));
    RAHT_RET(enc_tables_ok(fn, F, Q, seg_bytes, seg_off, out, cap, total_bytes));
    return seg_encode_frames<uint32_t>(fn, "raht_rlgr_seg_encode", F, Q, D, seg_len, flag_signed, seg_bytes, seg_off, out, cap, total_bytes, stream);
}

/* The inverse, one launch, no synchronisation. *bad_dev (DEVICE uint32; may be NULL without expect): bit j when a table entry of
 * frame j reached outside in[j] (that segment decodes as zeros); with expect (may be NULL; ROW-MAJOR frames only, every
 * expect[j] set, in the layout and strides of Q[j]) bit 16 + j when frame j differs from expect[j]. */
int raht_rlgr_seg_decode_ragged(int k, const uint8_t *const *in, const int64_t *in_bytes, const uint32_t *const *seg_off, const uint32_t *const *seg_bytes,
                                const int64_t *N, int D, int seg_len, int flag_signed, int32_t *const *Q, const int32_t *const *expect,
                                const int64_t *sym_stride, const int64_t *chan_stride, uint32_t *bad_dev, raht_stream_t stream)
{
    const char *fn = "raht_rlgr_seg_decode_ragged";
    SegFrames F;                                                              // (32: a frame beyond the 32-bit tables fills the chip alone)
    RAHT_RET(seg_frames(fn, 32, k, N, sym_stride, chan_stride, true, D, seg_len, &F));
    RAHT_RET(dec_tables_ok(fn, fn, F, D, in, in_bytes, seg_off, seg_bytes, Q, expect, bad_dev));
    return seg_decode_launch<uint32_t, RAHT_RLGR_BATCH_MAX>(F, in, in_bytes, seg_off, seg_bytes, D, seg_len, flag_signed, Q, expect, bad_dev, stream);
}

}  // extern "C"
