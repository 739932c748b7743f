// device_memory.hip -- the library's device memory and its way back to the host: the thread-local scratch pool (Scratch), the
// process-wide cache of long-lived blocks (dev_malloc / dev_free, what every DevBuf holds) and the polled mailbox of the small
// device -> host read-backs (read_back_u32). Declared in raht_common.h; every other translation unit uses them.
#include "raht_common.h"
#include <map>
#include <mutex>
#include <unordered_map>

namespace raht {

// ------------------------------------------------------------------------------------------------
// Scratch pool
// ------------------------------------------------------------------------------------------------
struct PoolBlock { void *p; size_t bytes; bool used; int device; hipStream_t last_stream; bool touched; };
static thread_local std::vector<PoolBlock> g_pool;

Scratch::Scratch(size_t bytes, hipStream_t stream)
{
    if (bytes == 0) bytes = 16;
    const int dev = current_device();
    int best = -1, n_dev = 0;
    // best fit among the free blocks whose last user ran on THIS stream (or that were never used). A block last used on another
    // stream is handed out only once the pool holds 40 blocks for the device, and only after a device synchronisation (below):
    // until then a caller that moves between streams gets a new block instead of a wait for the device to drain
    int best_other = -1;
    for (int i = 0; i < (int)g_pool.size(); ++i) {
        const PoolBlock &b = g_pool[(size_t)i];
        if (b.device != dev || !b.p) continue;
        ++n_dev;
        if (b.used || b.bytes < bytes) continue;
        if (!b.touched || b.last_stream == stream) { if (best < 0 || b.bytes < g_pool[(size_t)best].bytes) best = i; }
        else if (best_other < 0 || b.bytes < g_pool[(size_t)best_other].bytes) best_other = i;
    }
    if (best < 0 && best_other >= 0 && n_dev >= 40) best = best_other;
    if (best < 0) {
        // recycle the largest free block (of this device) that is too small, else grow the pool
        int victim = -1, empty = -1;
        for (int i = 0; i < (int)g_pool.size(); ++i) {
            const PoolBlock &b = g_pool[(size_t)i];
            if (!b.p && !b.used) { if (empty < 0) empty = i; continue; }
            if (b.device == dev && !b.used && (victim < 0 || b.bytes > g_pool[(size_t)victim].bytes)) victim = i;
        }
        void *q = nullptr;
        const size_t want = bytes + bytes / 4;                 // head-room against slow growth
        if (victim >= 0 && n_dev >= 48) {
            (void)hipFree(g_pool[(size_t)victim].p);
            // a failed allocation leaves an EMPTY slot behind: erasing it would shift the slot indices that
            // live Scratch objects hold, and a later destructor would release somebody else's block
            g_pool[(size_t)victim] = {nullptr, 0, false, dev, nullptr, false};
            if (hipMalloc(&q, want) != hipSuccess) { (void)hipGetLastError(); set_error("scratch: out of device memory (%zu bytes)", want); return; }
            g_pool[(size_t)victim] = {q, want, false, dev, nullptr, false};
            best = victim;
        } else {
            if (hipMalloc(&q, want) != hipSuccess) { (void)hipGetLastError(); set_error("scratch: out of device memory (%zu bytes)", want); return; }
            if (empty >= 0) { g_pool[(size_t)empty] = {q, want, false, dev, nullptr, false}; best = empty; }
            else { g_pool.push_back({q, want, false, dev, nullptr, false}); best = (int)g_pool.size() - 1; }
        }
    }
    PoolBlock &blk = g_pool[(size_t)best];
    // the block's previous user may still be running on another stream (see raht_common.h)
    if (blk.touched && blk.last_stream != stream) (void)hipDeviceSynchronize();
    blk.used = true;
    blk.touched = true;
    blk.last_stream = stream;
    p_ = blk.p;
    slot_ = best;
}

Scratch::~Scratch()
{
    if (slot_ >= 0 && slot_ < (int)g_pool.size()) g_pool[(size_t)slot_].used = false;
}

// ------------------------------------------------------------------------------------------------
// Cache of long-lived device blocks (see raht_common.h).
// ------------------------------------------------------------------------------------------------
namespace {
struct LiveBlock { size_t cls; int device; };
struct DevCache {
    std::mutex mu;
    std::unordered_map<void *, LiveBlock> live;                    // block -> (class size, device)
    std::multimap<std::pair<int, size_t>, void *> free_blocks;     // (device, class size) -> block
    size_t cached = 0, limit = (size_t)8 << 30;                    // limit: raht_set_cached_memory_limit
};
DevCache &dev_cache()
{
    static DevCache c;
    return c;
}
size_t size_class(size_t bytes)
{
    if (bytes < 4096) return 4096;
    int hb = 63 - __builtin_clzll((unsigned long long)bytes);
    const size_t step = (size_t)1 << (hb - 3);           // eight classes per power of two
    return (bytes + step - 1) / step * step;
}
}  // namespace

hipError_t dev_malloc(void **p, size_t bytes)
{
    DevCache &c = dev_cache();
    const size_t cls = size_class(bytes);
    const int dev = current_device();
    {
        std::lock_guard<std::mutex> g(c.mu);
        auto it = c.free_blocks.find(std::make_pair(dev, cls));
        if (it != c.free_blocks.end()) {
            *p = it->second;
            c.free_blocks.erase(it);
            c.cached -= cls;
            c.live[*p] = LiveBlock{cls, dev};
            return hipSuccess;
        }
    }
    hipError_t e = hipMalloc(p, cls);
    if (e != hipSuccess) {                               // under memory pressure: drop the cache and retry
        (void)hipGetLastError();
        raht_release_cached_memory();
        e = hipMalloc(p, cls);
    }
    if (e == hipSuccess) {
        std::lock_guard<std::mutex> g(c.mu);
        c.live[*p] = LiveBlock{cls, dev};
    }
    return e;
}

void dev_free(void *p)
{
    if (!p) return;
    DevCache &c = dev_cache();
    size_t cls = 0;
    {
        std::lock_guard<std::mutex> g(c.mu);
        int dev = 0;
        auto it = c.live.find(p);
        if (it != c.live.end()) { cls = it->second.cls; dev = it->second.device; c.live.erase(it); }
        if (cls && c.cached + cls <= c.limit) {
            c.free_blocks.emplace(std::make_pair(dev, cls), p);      // back to the bucket of the block's OWN device
            c.cached += cls;
            return;
        }
    }
    (void)hipFree(p);
}

extern "C" int64_t raht_debug_live_blocks(void)
{
    DevCache &c = dev_cache();
    std::lock_guard<std::mutex> g(c.mu);
    return (int64_t)c.live.size();
}

extern "C" int64_t raht_debug_cached_blocks(void)
{
    DevCache &c = dev_cache();
    std::lock_guard<std::mutex> g(c.mu);
    return (int64_t)c.free_blocks.size();
}

extern "C" int raht_set_cached_memory_limit(int64_t bytes)
{
    if (bytes < 0) { set_error("raht_set_cached_memory_limit: bytes must be >= 0"); return RAHT_ERR_INVALID; }
    DevCache &c = dev_cache();
    std::lock_guard<std::mutex> g(c.mu);
    c.limit = (size_t)bytes;
    return RAHT_OK;
}

// ------------------------------------------------------------------------------------------------
// Small device -> host read-backs through a polled mailbox in mapped pinned memory.
// ------------------------------------------------------------------------------------------------
static constexpr int MAILBOX_WORDS = 192;

__global__ void __launch_bounds__(64) mailbox_publish_kernel(const uint32_t *__restrict__ a, int na,
                                                             const uint32_t *__restrict__ b, int nb,
                                                             volatile uint32_t *box, uint32_t seq)
{
    // one wave: the data stores are complete (system scope) before lane 0 raises the sequence word
    for (int t = threadIdx.x; t < na; t += 64) box[1 + t] = a[t];
    for (int t = threadIdx.x; t < nb; t += 64) box[1 + na + t] = b[t];
    __threadfence_system();
    if (threadIdx.x == 0) box[0] = seq;
}

struct Mailbox {
    std::mutex mu;
    uint32_t *box = nullptr;      // [0] = sequence word, [1 ..] = payload
    uint32_t seq = 0;
};
static Mailbox &mailbox() { static Mailbox m; return m; }

int read_back_u32(uint32_t *dst_a, const uint32_t *dev_a, int na, uint32_t *dst_b, const uint32_t *dev_b, int nb,
                  hipStream_t s, const std::function<void()> &behind)
{
    bool behind_called = false;
    if (na < 0 || nb < 0 || na + nb > MAILBOX_WORDS) { set_error("read_back_u32: too many words"); return RAHT_ERR_INVALID; }
    Mailbox &m = mailbox();
    std::lock_guard<std::mutex> g(m.mu);
    if (!m.box) {
        // portable + mapped + coherent: the same pointer is valid on the host and on every device
        if (hipHostMalloc((void **)&m.box, sizeof(uint32_t) * (MAILBOX_WORDS + 1),
                          hipHostMallocPortable | hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {
            m.box = nullptr;
            (void)hipGetLastError();
        } else {
            m.box[0] = 0;
        }
    }
    bool done = false;
    if (m.box) {
        const uint32_t seq = ++m.seq ? m.seq : ++m.seq;            // never 0
        hipLaunchKernelGGL(mailbox_publish_kernel, dim3(1), dim3(64), 0, s, dev_a, na, dev_b, nb, m.box, seq);
        if (hipGetLastError() == hipSuccess) {
            if (behind) { behind(); behind_called = true; }
            volatile uint32_t *flag = m.box;
            for (uint32_t it = 1;; ++it) {
                if (*flag == seq) { done = true; break; }
                if ((it & 0xfffu) == 0) {
                    // a failed or finished stream ends the wait even if the word never arrives
                    const hipError_t q = hipStreamQuery(s);
                    if (q != hipErrorNotReady) { done = (q == hipSuccess && *flag == seq); break; }
                }
                __builtin_ia32_pause();
            }
            if (done) {
                __atomic_thread_fence(__ATOMIC_ACQUIRE);
                for (int t = 0; t < na; ++t) dst_a[t] = flag[1 + t];
                for (int t = 0; t < nb; ++t) dst_b[t] = flag[1 + na + t];
            }
        }
    }
    if (!done) {                                                     // no mailbox / stream error: the plain way
        if (behind && !behind_called) behind();
        hipError_t e = hipSuccess;
        if (na) e = hipMemcpyAsync(dst_a, dev_a, sizeof(uint32_t) * (size_t)na, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && nb) e = hipMemcpyAsync(dst_b, dev_b, sizeof(uint32_t) * (size_t)nb, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) { set_error("read-back: %s", hipGetErrorString(e)); return RAHT_ERR_HIP; }
    }
    return RAHT_OK;
}

}  // namespace raht

extern "C" int raht_release_cached_memory(void)
{
    auto &c = raht::dev_cache();
    std::vector<void *> blocks;
    {
        std::lock_guard<std::mutex> g(c.mu);
        for (auto &kv : c.free_blocks) blocks.push_back(kv.second);
        c.free_blocks.clear();
        c.cached = 0;
    }
    for (void *q : blocks) (void)hipFree(q);
    return RAHT_OK;
}
