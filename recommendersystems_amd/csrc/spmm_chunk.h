// How the chunked SpMM (iterate.hip: spmm_chunked_body) cuts a row's in-list into index loads.  One load is
// one instruction of a lane group: lane k < LW fetches entry p + k.  Plain C++17, host and device, so that
// tests/cpp/spmm_chunk_check.cpp checks the rule on the host.
// The rule decides the SpMM's index traffic, but this file is not among the sources bench.py fingerprints for
// profiles/traffic_*.json (iterate.hip, build.hip, common.h, pf.h): after a change here, refresh that profile by hand.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RWR_CHUNK_HD __host__ __device__
#else
#define RWR_CHUNK_HD
#endif

namespace rwr {

// Entries the next load of a list takes: `left` > 0 entries remain from position p of in_src, LW (a power of two) lanes
// load.  A list that fits takes one load (at most two LW-entry lines, each touched once).  A longer one is first cut at the
// next multiple of LW, so that every later load starts on a line -- at LW = 32 a 128-byte line of in_src -- and no line is
// fetched by two loads that lie a gather round trip apart.  left <= 0 gives 0.
constexpr RWR_CHUNK_HD int spmm_next_load(int64_t p, int64_t left, int LW)
{
    return left <= 0 ? 0 : left <= LW ? (int)left : LW - (int)(p & (int64_t)(LW - 1));
}

}   // namespace rwr
