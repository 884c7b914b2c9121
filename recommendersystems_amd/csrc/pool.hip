// The block cache of pool.h bound to the HIP runtime: rwr::pool_alloc / rwr::pool_free behind every DevBuf (common.h).
#include "common.h"
#include "pool.h"

namespace rwr {

namespace {
struct HipRaw {
    static void *alloc(size_t bytes)
    {
        void *p = nullptr;
        return hipMalloc(&p, bytes) == hipSuccess ? p : nullptr;   // (a failure stays in the thread's last error: DevBuf::alloc reads it)
    }
    static void release(void *p) { (void)hipFree(p); }
    static bool current_device(int *dev) { return hipGetDevice(dev) == hipSuccess; }
    static void forget_failure() { (void)hipGetLastError(); }
};
}  // namespace

void *pool_alloc(size_t bytes, size_t *got) { return BlockCache<HipRaw>::alloc(bytes, got); }

void pool_free(void *p, size_t got) { BlockCache<HipRaw>::free(p, got); }

}  // namespace rwr
