// The device-memory block cache behind every DevBuf (common.h), as host bookkeeping alone: no HIP header, no device call.
// Blocks of 512 B ... 32 MB in power-of-two sizes, kept per device when handed back, up to POOL_CAP bytes per device; larger
// requests go straight to the raw allocator.  pool.hip binds it to hipMalloc / hipFree / hipGetDevice;
// tests/cpp/pool_check.cpp drives it with a raw allocator of tokens, under the address, undefined-behaviour and thread sanitizers.
//
// Raw supplies, as static members:
//     void *alloc(size_t bytes)          nullptr = out of memory
//     void release(void *p)
//     bool current_device(int *dev)      false = not known (the request then bypasses the cache)
//     void forget_failure()              called once between a failed alloc and its retry (HIP: clears the thread's last error)
#pragma once
#include <cstddef>
#include <mutex>
#include <vector>

namespace rwr {

constexpr size_t POOL_MIN = 512, POOL_MAX = 32ull << 20, POOL_CAP = 2ull << 30;
constexpr int POOL_DEVICES = 16, POOL_CLASSES = 17;                 // 512 B << 16 = 32 MB
// In front of the shared cache, a cache per host thread that needs no lock: the harness's ten threads (Program.cs:11) each
// build and drop graphs of ~30 device arrays, and ten threads taking one mutex a thousand times per call spent more time
// in the mutex's slow path than in the rest of the library (measured: 25 ns per operation alone, 3.5 us with ten threads).
// A thread keeps what it frees, up to TL_CAP bytes / TL_PER_CLASS blocks per size; the rest, and everything it holds when it
// ends, goes to the shared cache.
constexpr size_t TL_CAP = 256ull << 20;
constexpr size_t TL_PER_CLASS = 512;

inline int pool_class(size_t bytes, size_t *size)
{
    size_t sz = POOL_MIN;
    int c = 0;
    while (sz < bytes) { sz <<= 1; ++c; }
    *size = sz;
    return c;
}

struct PoolCounts { size_t blocks, bytes; };

template <class Raw>
struct BlockCache {
    struct PoolDev { std::vector<void *> free_blocks[POOL_CLASSES]; size_t cached = 0; };
    struct ThreadCache {
        int dev = -1;
        std::vector<void *> blocks[POOL_CLASSES];
        size_t bytes = 0;
        void flush()
        {
            if (dev < 0 || dev >= POOL_DEVICES) return;
            std::lock_guard<std::mutex> lk(g_mutex);
            size_t size = POOL_MIN;
            for (int c = 0; c < POOL_CLASSES; ++c, size <<= 1) {
                for (void *p : blocks[c]) {
                    g_pool[dev].free_blocks[c].push_back(p);          // (may exceed POOL_CAP: nothing is freed from a destructor)
                    g_pool[dev].cached += size;
                }
                blocks[c].clear();
            }
            bytes = 0;
        }
        ~ThreadCache() { flush(); }
    };
    static inline std::mutex g_mutex;
    static inline PoolDev g_pool[POOL_DEVICES];
    static inline thread_local ThreadCache tl_cache;

    // *got = bytes actually reserved
    static void *alloc(size_t bytes, size_t *got)
    {
        void *p = nullptr;
        if (bytes > POOL_MAX) {
            *got = bytes;
            return Raw::alloc(bytes);
        }
        size_t size = 0;
        const int c = pool_class(bytes, &size);
        *got = size;
        int dev = 0;
        const bool dev_ok = Raw::current_device(&dev) && dev >= 0 && dev < POOL_DEVICES;
        if (dev_ok && tl_cache.dev == dev && !tl_cache.blocks[c].empty()) {
            p = tl_cache.blocks[c].back();
            tl_cache.blocks[c].pop_back();
            tl_cache.bytes -= size;
            return p;
        }
        if (dev_ok) {
            std::lock_guard<std::mutex> lk(g_mutex);
            auto &fl = g_pool[dev].free_blocks[c];
            if (!fl.empty()) {
                p = fl.back();
                fl.pop_back();
                g_pool[dev].cached -= size;
                return p;
            }
        }
        if ((p = Raw::alloc(size))) return p;
        // out of memory with blocks parked in the cache: give them back to the driver and try once more
        Raw::forget_failure();
        std::vector<void *> drop;
        if (dev >= 0 && dev < POOL_DEVICES) {
            if (tl_cache.dev == dev) tl_cache.flush();             // (this thread's own cache too; other threads' stay with them)
            std::lock_guard<std::mutex> lk(g_mutex);
            for (auto &fl : g_pool[dev].free_blocks) { drop.insert(drop.end(), fl.begin(), fl.end()); fl.clear(); }
            g_pool[dev].cached = 0;
        }
        for (void *q : drop) Raw::release(q);
        return Raw::alloc(size);
    }

    static void free(void *p, size_t got)
    {
        if (!p) return;
        int dev = -1;
        if (got <= POOL_MAX && got >= POOL_MIN && (got & (got - 1)) == 0 && Raw::current_device(&dev) && dev >= 0 &&
            dev < POOL_DEVICES) {
            // (the block belongs to the current device: every entry point binds the handle's device before it touches memory)
            size_t size = 0;
            const int c = pool_class(got, &size);
            if (tl_cache.dev != dev && tl_cache.bytes == 0) tl_cache.dev = dev;
            if (tl_cache.dev == dev && tl_cache.bytes + size <= TL_CAP && tl_cache.blocks[c].size() < TL_PER_CLASS) {
                tl_cache.blocks[c].push_back(p);
                tl_cache.bytes += size;
                return;
            }
            std::lock_guard<std::mutex> lk(g_mutex);
            if (g_pool[dev].cached + size <= POOL_CAP) {
                g_pool[dev].free_blocks[c].push_back(p);
                g_pool[dev].cached += size;
                return;
            }
        }
        Raw::release(p);
    }

    // what the caches hold (for the check; the library does not ask)
    static PoolCounts shared_counts(int dev)
    {
        std::lock_guard<std::mutex> lk(g_mutex);
        PoolCounts n{0, g_pool[dev].cached};
        for (const auto &fl : g_pool[dev].free_blocks) n.blocks += fl.size();
        return n;
    }
    static PoolCounts thread_counts()
    {
        PoolCounts n{0, tl_cache.bytes};
        for (const auto &b : tl_cache.blocks) n.blocks += b.size();
        return n;
    }
};

}  // namespace rwr
