// The shifted block copies of one segment of the resident raw lists: what a workgroup of SEG_THREADS lanes does with the old
// positions [a, b) that all move by the same sh -- up in k_append_merge (append.hip), down in k_remove_compact
// (remove.hip, §3.23).  Every lane calls with its own tid; together the lanes write out[a + sh .. b + sh) exactly once and
// nothing else, and read src[a .. b) alone.  Plain C++ behind __host__ __device__, so that tests/cpp/remove_plan_check.cpp
// replays the lanes on the host.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define SEG_HD __host__ __device__ __forceinline__
#else
#define SEG_HD inline
#endif

namespace rwr {

constexpr int SEG_THREADS = 256;

// three coalesced block copies by the whole workgroup: this one for the weights (T = double) and the targets (int32_t)
template <typename T>
SEG_HD void copy_seg(const T *__restrict__ src, T *__restrict__ out, int64_t a, int64_t b, int64_t sh, int tid)
{
    int64_t e = a + tid;
    for (; e + 3 * SEG_THREADS < b; e += 4 * SEG_THREADS) {     // four loads in flight per lane
        const T v0 = src[e], v1 = src[e + SEG_THREADS], v2 = src[e + 2 * SEG_THREADS], v3 = src[e + 3 * SEG_THREADS];
        out[e + sh] = v0;
        out[e + sh + SEG_THREADS] = v1;
        out[e + sh + 2 * SEG_THREADS] = v2;
        out[e + sh + 3 * SEG_THREADS] = v3;
    }
    for (; e < b; e += SEG_THREADS) out[e + sh] = src[e];
}
// ... of the byte array: four elements per lane, stored as one aligned dword (the source is as aligned as the shift leaves it:
// it is read byte by byte, from lines the neighbouring lanes read as well).  A head and a tail of up to three bytes each keep
// every dword inside the segment's image, so a neighbouring segment's bytes are never touched.
SEG_HD void copy_seg_bytes(const uint8_t *__restrict__ src, uint8_t *__restrict__ out, int64_t a, int64_t b, int64_t sh, int tid)
{
    const int64_t len = b - a;
    int64_t head = (int64_t)((4 - (reinterpret_cast<uintptr_t>(out + a + sh) & 3)) & 3);
    if (head > len) head = len;
    if (tid < head) out[a + sh + tid] = src[a + tid];
    const int64_t nd = (len - head) >> 2;                      // whole dwords
    const uint8_t *s4 = src + a + head;
    uint32_t *o4 = reinterpret_cast<uint32_t *>(out + a + sh + head);
    for (int64_t d = tid; d < nd; d += SEG_THREADS) {
        const uint8_t *q = s4 + 4 * d;
        o4[d] = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
    }
    const int64_t t0 = head + 4 * nd;                          // up to three bytes left
    if (tid < len - t0) out[a + sh + t0 + tid] = src[a + t0 + tid];
}

}  // namespace rwr
