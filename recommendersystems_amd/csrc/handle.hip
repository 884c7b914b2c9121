// Handles (handle.h): the device check, the pool of recycled stream / event / pinned-buffer sets, option resolution, and
// opening and closing an rwr_graph.
#include <mutex>
#include <new>
#include <vector>
#include <stdlib.h>
#include <string.h>

#include "handle.h"

namespace rwr {

int usable_devices()
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

// asked once per device and process: hipGetDeviceProperties goes to the driver under a runtime-wide
// lock, and the reference's harness creates a graph per fold and methodology from ten threads (Program.cs:11)
int32_t check_gfx950(int device)
{
    static std::mutex mu;
    static int state[64];            // 0 unknown, 1 gfx950, 2 something else
    static char names[64][64];
    if (device < 0 || device >= 64) { set_error("device %d out of range", device); return RWR_E_NO_DEVICE; }
    std::lock_guard<std::mutex> lk(mu);
    if (state[device] == 0) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) != hipSuccess) { set_error("hipGetDeviceProperties failed"); return RWR_E_HIP; }
        snprintf(names[device], sizeof(names[device]), "%s", prop.gcnArchName);
        state[device] = strncmp(prop.gcnArchName, "gfx950", 6) == 0 ? 1 : 2;
    }
    if (state[device] != 1) {
        set_error("device %d is %s; librwr is built for gfx950 only", device, names[device]);
        return RWR_E_NO_DEVICE;
    }
    return RWR_OK;
}

static std::mutex g_kit_mutex;
static std::vector<HandleKit> g_kits;
constexpr size_t KIT_POOL_MAX = 32;

bool kit_take(int device, HandleKit *out)
{
    std::lock_guard<std::mutex> lk(g_kit_mutex);
    for (size_t i = 0; i < g_kits.size(); ++i)
        if (g_kits[i].device == device) {
            *out = g_kits[i];
            g_kits.erase(g_kits.begin() + (long)i);
            return true;
        }
    return false;
}
void kit_destroy(HandleKit &k)
{
    if (k.ev_fork) (void)hipEventDestroy(k.ev_fork);
    if (k.ev_join) (void)hipEventDestroy(k.ev_join);
    if (k.ev_a) (void)hipEventDestroy(k.ev_a);
    if (k.ev_b) (void)hipEventDestroy(k.ev_b);
    if (k.ev_h0) (void)hipEventDestroy(k.ev_h0);
    if (k.ev_h1) (void)hipEventDestroy(k.ev_h1);
    if (k.stream3) (void)hipStreamDestroy(k.stream3);
    if (k.stream) (void)hipStreamDestroy(k.stream);
    if (k.stream2) (void)hipStreamDestroy(k.stream2);
    if (k.pin) (void)hipHostFree(k.pin);
    if (k.stage) (void)hipHostFree(k.stage);
    k = HandleKit{};
}
void kit_give(HandleKit &k)
{
    {
        std::lock_guard<std::mutex> lk(g_kit_mutex);
        if (k.stream && k.stream2 && k.stream3 && g_kits.size() < KIT_POOL_MAX) {
            try {
                g_kits.push_back(k);
                k = HandleKit{};
                return;
            } catch (const std::bad_alloc &) {}        // (no host memory to park it: destroyed; rwr_graph_destroy throws nothing)
        }
    }
    kit_destroy(k);
}

int32_t kit_acquire(int device, HandleKit *kit)
{
    if (!kit_take(device, kit)) {
        // the seed-row chain (stream2) is latency-bound and must not queue behind the SpMM's half-million
        // workgroups: give its stream the highest dispatch priority
        int prio_lo = 0, prio_hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
        if (hipStreamCreateWithFlags(&kit->stream, hipStreamNonBlocking) != hipSuccess ||
            hipStreamCreateWithPriority(&kit->stream2, hipStreamNonBlocking, prio_hi) != hipSuccess ||
            hipStreamCreateWithPriority(&kit->stream3, hipStreamNonBlocking, prio_hi) != hipSuccess ||
            hipEventCreateWithFlags(&kit->ev_h0, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&kit->ev_h1, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&kit->ev_fork, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&kit->ev_join, hipEventDisableTiming) != hipSuccess ||
            hipEventCreate(&kit->ev_a) != hipSuccess || hipEventCreate(&kit->ev_b) != hipSuccess) {
            set_error("stream/event creation failed: %s", hipGetErrorString(hipGetLastError()));
            kit_destroy(*kit);
            return RWR_E_HIP;
        }
    }
    kit->device = device;
    return RWR_OK;
}

int32_t resolve_opts(const char *who, const rwr_opts *opts, int ndev, bool env_mode, rwr_opts *out)
{
    rwr_opts o{};
    o.struct_size = sizeof(rwr_opts);
    o.device = -1;
    o.mode = -1;
    if (opts) {
        size_t sz = opts->struct_size > 0 ? (size_t)opts->struct_size : sizeof(rwr_opts);
        if (sz > sizeof(rwr_opts)) sz = sizeof(rwr_opts);
        memcpy(&o, opts, sz);
    }
    if (o.device < 0) {
        const char *e = getenv("RWR_DEVICE");
        if (e && *e) o.device = atoi(e);
        else {
            int cur = 0;
            if (hipGetDevice(&cur) != hipSuccess) cur = 0;
            o.device = cur;
        }
    }
    if (o.mode < 0) {
        const char *e = env_mode ? getenv("RWR_MODE") : nullptr;
        o.mode = (e && strcmp(e, "fast") == 0) ? 1 : RWR_MODE_EXACT;
    }
    if (o.device >= ndev) {
        set_error("%s: device %d requested but only %d visible", who, o.device, ndev);
        return RWR_E_NO_DEVICE;
    }
    if (o.mode != RWR_MODE_EXACT) {
        // (mode 1 was FAST until ABI 3: re-associated sums with no ranking guarantee and no speed advantage -- removed)
        set_error("%s: unknown mode %d (the only arithmetic mode is RWR_MODE_EXACT = 0%s)", who, o.mode, env_mode ? "; FAST was removed" : "");
        return RWR_E_INVALID;
    }
    *out = o;
    return RWR_OK;
}

int32_t graph_open(int32_t n, const int64_t *node_id, const uint8_t *node_type, const int64_t *rowptr, const int32_t *dst,
                   const uint8_t *etype, const double *w, const rwr_opts *opts, rwr_graph **out)
{
    const int ndev = usable_devices();
    if (ndev <= 0) { set_error("no usable HIP device (librwr has no CPU fallback)"); return RWR_E_NO_DEVICE; }
    rwr_graph *g = new (std::nothrow) rwr_graph();
    if (!g) { set_error("out of host memory"); return RWR_E_NOMEM; }
    int32_t rc = resolve_opts("rwr_graph_create", opts, ndev, true, &g->opts);
    if (rc != RWR_OK) {
        delete g;
        return rc;
    }
    g->device = g->opts.device;
    g->n = n;
    g->nnz_raw = rowptr[n];
    auto fail = [&](int32_t code) {
        graph_close(g);
        return code;
    };
    DeviceGuard dev_guard(g->device);
    if (dev_guard.rc != RWR_OK) return fail(dev_guard.rc);
    if ((rc = check_gfx950(g->device)) != RWR_OK) return fail(rc);
    HandleKit kit;
    if ((rc = kit_acquire(g->device, &kit)) != RWR_OK) return fail(rc);
    g->stream = kit.stream; g->stream2 = kit.stream2; g->stream3 = kit.stream3;
    g->ev_fork = kit.ev_fork; g->ev_join = kit.ev_join; g->ev_a = kit.ev_a; g->ev_b = kit.ev_b;
    g->ev_h0 = kit.ev_h0; g->ev_h1 = kit.ev_h1;
    g->sm_pin = kit.pin;
    g->sm_stage = kit.stage;
    // (a host exception of the build closes the handle like any other failure: graph_close synchronises its streams first)
    rc = no_throw("rwr_graph_create", [&] { return graph_build(g, node_id, node_type, rowptr, dst, etype, w); });
    if (rc != RWR_OK) return fail(rc);
    g->stats.struct_size = sizeof(rwr_stats);
    g->stats.n = n;
    g->stats.nnz_raw = g->nnz_raw;
    g->stats.nnz = g->nnz;
    g->stats.uniform = g->uniform;
    g->stats.mode = g->opts.mode;
    *out = g;
    return RWR_OK;
}

void graph_close(rwr_graph *g)
{
    DeviceGuard dev_guard(g->device);
    if (g->stream) (void)hipStreamSynchronize(g->stream);
    if (g->stream2) (void)hipStreamSynchronize(g->stream2);
    if (g->stream3) (void)hipStreamSynchronize(g->stream3);
    HandleKit kit;
    kit.device = g->device;
    kit.stream = g->stream; kit.stream2 = g->stream2; kit.stream3 = g->stream3;
    kit.ev_h0 = g->ev_h0; kit.ev_h1 = g->ev_h1;
    kit.ev_fork = g->ev_fork; kit.ev_join = g->ev_join; kit.ev_a = g->ev_a; kit.ev_b = g->ev_b;
    kit.pin = g->sm_pin;
    kit.stage = g->sm_stage;
    kit_give(kit);            // (parked for the next handle on this device, or destroyed when the pool is full)
    delete g;
}

}  // namespace rwr
