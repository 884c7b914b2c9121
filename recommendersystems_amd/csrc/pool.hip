// The process-wide pools behind the runtime's slow allocations: the block cache of pool.h bound to the HIP runtime
// (rwr::pool_alloc / rwr::pool_free behind every DevBuf, common.h) and the pinned host buffers of a rwr_eval_graphs call.
#include "engine.h"
#include "pool.h"

#include <mutex>
#include <vector>

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

// Pinned host buffers of one rwr_eval_graphs call, grown on demand: slot 0 the graphs' staging slots and read-back areas,
// the others the small tables the batch kernels take (argument arrays, test sets, results).  Every host<->device copy of a
// batch goes through pinned memory: an "asynchronous" copy from pageable memory is staged by the runtime under a process-wide
// lock and waits for the device.  Allocating pinned memory costs milliseconds, so the sets are recycled through a process-wide
// pool (a call takes one, gives it back at its end); the calling thread reaches its set through a thread-local pointer.
constexpr int MULTI_SLOTS = 6;
struct MultiPins {
    void *pin[MULTI_SLOTS] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    size_t cap[MULTI_SLOTS] = {0, 0, 0, 0, 0, 0};
};
static std::mutex g_pins_mutex;
static std::vector<MultiPins *> g_pins;          // parked sets (never freed: a handful of MB per concurrent caller)
static thread_local MultiPins *tl_pins = nullptr;
void multi_pins_acquire()
{
    if (tl_pins) return;
    {
        std::lock_guard<std::mutex> lk(g_pins_mutex);
        if (!g_pins.empty()) { tl_pins = g_pins.back(); g_pins.pop_back(); }
    }
    if (!tl_pins) tl_pins = new MultiPins();
}
void multi_pins_release()
{
    if (!tl_pins) return;
    std::lock_guard<std::mutex> lk(g_pins_mutex);
    g_pins.push_back(tl_pins);
    tl_pins = nullptr;
}
int32_t multi_pinned(int slot, size_t bytes, void **out)
{
    if (!tl_pins) { set_error("multi_pinned: no pinned set acquired"); return RWR_E_INVALID; }
    MultiPins &a = *tl_pins;
    if (a.cap[slot] < bytes) {
        if (a.pin[slot]) { (void)hipHostFree(a.pin[slot]); a.pin[slot] = nullptr; a.cap[slot] = 0; }
        const size_t cap = bytes + bytes / 2 + 4096;
        RWR_HIP(hipHostMalloc(&a.pin[slot], cap, hipHostMallocMapped | hipHostMallocPortable));
        a.cap[slot] = cap;
    }
    *out = a.pin[slot];
    return RWR_OK;
}

}  // namespace rwr
