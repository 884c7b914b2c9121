// Ego-network-sized graphs: the limits of the one-launch paths, the layout of the pinned staging buffer such a graph is
// uploaded through and read back from, and the argument block of the one-launch build (build.hip: k_build_small; host side:
// build_small.hip).  Plain C++ with no HIP types: tests/cpp/stage_layout_check.cpp compiles it on its own.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace rwr {

// The largest graph the one-launch paths take: the staged upload and the one-launch build (graph_fits_small_build), and
// small.hip's one-launch Recommendation (link count).  ONE_LAUNCH_MAX_N also sizes the pinned read-back area of a staged graph:
// a graph that grows past either limit leaves the staged path (append.hip).
constexpr int32_t ONE_LAUNCH_MAX_N = 8192;
constexpr int64_t ONE_LAUNCH_MAX_M = 65536;

// The six raw arrays arrive as ONE copy out of the pinned staging buffer and are dealt to their device arrays by the build's
// kernel (six pageable copies cost ~100 us of a ~0.5 ms build): byte offsets of the arrays in that copy, 8-byte arrays first
struct StageLayout { size_t id, rp, w, dst, nt, et, total; };
inline StageLayout stage_layout(int32_t n, int64_t m)
{
    StageLayout L;
    L.id = 0;
    L.rp = L.id + 8 * (size_t)n;
    L.w = L.rp + 8 * ((size_t)n + 1);
    L.dst = L.w + 8 * (size_t)m;
    L.nt = L.dst + ((4 * (size_t)m + 7) & ~(size_t)7);
    L.et = L.nt + (((size_t)n + 7) & ~(size_t)7);
    L.total = L.et + (size_t)m;
    return L;
}

// What the host needs back is written by the kernel straight into pinned host memory: the link count (int64), the four flag
// words, in_ptr (n + 1 int64), dangling (n bytes)
constexpr size_t STAGE_OUT_NNZ = 0;
constexpr size_t STAGE_OUT_FLAGS = 8;
constexpr size_t STAGE_OUT_IN_PTR = 32;
constexpr size_t stage_out_dangling(int32_t n) { return STAGE_OUT_IN_PTR + 8 * ((size_t)n + 1); }
constexpr size_t stage_out_bytes(int32_t n) { return stage_out_dangling(n) + (size_t)n; }

// one pinned buffer per handle: inputs below STAGE_OUT_OFF, the read-back area above
constexpr size_t STAGE_OUT_OFF = 1u << 20;
constexpr size_t STAGE_BYTES = STAGE_OUT_OFF + stage_out_bytes(ONE_LAUNCH_MAX_N) + 256;

struct BuildSmallArgs {
    int32_t n, n_items, first, do_stage_in;
    int32_t zero_flags, pad0;        // the kernel clears the flag words itself (batch builds: no memset per graph)
    int64_t m;
    const uint8_t *stage; StageLayout L;
    int64_t *node_id; uint8_t *node_type; int64_t *rowptr; int32_t *dst; uint8_t *etype; double *w_raw;
    double *w_norm; int32_t *esrc; uint32_t *skey, *skey2, *sval, *sval2; uint8_t *dangling; double *w_src; int *flags;
    int64_t *in_ptr; int32_t *in_src; double *in_w;
    int32_t *row_order, *row_order_x, *item_rows, *item_order;
    uint64_t *ikey, *ikey2; uint32_t *ival, *ival2;
    int order_mode, n_bits, id_key_bits; uint64_t id_key_top;
    uint8_t *pin_out;
    unsigned long long *stamps;      // experiments build: s_memrealtime (100 MHz) at the stage boundaries; nullptr otherwise
};

}  // namespace rwr
