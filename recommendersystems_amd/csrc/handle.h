// What a handle is made of (internal): the gfx950 device check, the guard that binds a handle's device for one entry point, the
// recycled set of streams, events and pinned buffers (HandleKit), option resolution, and opening / closing an rwr_graph.
#pragma once
#include "engine.h"

namespace rwr {

int usable_devices();
// "is device d a gfx950" -- asked once per device and process
int32_t check_gfx950(int device);

// Makes the graph's device current for the duration of one entry point and gives the caller's device back on every
// return path: a host that shares the thread with PyTorch / RCCL keeps its own current device.
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    int32_t rc = RWR_OK;
    explicit DeviceGuard(int device)
    {
        if (hipGetDevice(&prev) != hipSuccess) { (void)hipGetLastError(); prev = -1; }
        if (prev != device) {
            hipError_t e = hipSetDevice(device);
            if (e != hipSuccess) {
                set_error("hipSetDevice(%d) failed: %s", device, hipGetErrorString(e));
                rc = RWR_E_HIP;
                return;
            }
            switched = true;
        }
    }
    ~DeviceGuard()
    {
        if (switched && prev >= 0) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

// Streams, events and the pinned result buffer of a handle are expensive to create and destroy (several hundred
// microseconds together) -- more than everything else the library does for an ego-network-sized graph, and the harness
// creates and drops one Graph per fold and methodology (Experiment.cs:69-105).  They are therefore recycled: a destroyed
// handle parks its set in a small per-process pool (per device), the next created handle on that device takes it.
struct HandleKit {
    int device = -1;
    hipStream_t stream = nullptr, stream2 = nullptr, stream3 = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_a = nullptr, ev_b = nullptr, ev_h0 = nullptr, ev_h1 = nullptr;
    void *pin = nullptr, *stage = nullptr;
};
bool kit_take(int device, HandleKit *out);
void kit_destroy(HandleKit &k);
void kit_give(HandleKit &k);   // parked for the next handle on its device, or destroyed when the pool is full
// a kit of `device` (current): one from the pool (idle: its streams were synchronised) or a full new set of streams and events
int32_t kit_acquire(int device, HandleKit *kit);

// The options a handle is created with: the struct_size-bounded copy of `opts` (may be NULL), then RWR_DEVICE or the current
// device for a device < 0, then the checks against the ndev visible devices and the one arithmetic mode.  `who` names the entry in
// the messages.  env_mode is the one difference between the two callers, inherited, not designed: rwr_graph_create reads
// RWR_MODE for a mode < 0 and its message says what became of "fast"; rwr_eval_graphs never read the variable.
int32_t resolve_opts(const char *who, const rwr_opts *opts, int ndev, bool env_mode, rwr_opts *out);

// rwr_graph_create after its argument checks / rwr_graph_destroy
int32_t graph_open(int32_t n, const int64_t *node_id, const uint8_t *node_type, const int64_t *rowptr, const int32_t *dst,
                   const uint8_t *etype, const double *w, const rwr_opts *opts, rwr_graph **out);
void graph_close(rwr_graph *g);

}  // namespace rwr
