// Host-side check of the chunked SpMM's load cutting (recommendersystems_amd/csrc/spmm_chunk.h), built against the header
// alone by tests/test_spmm_chunk.py.  For every list start p in 0..95, every length in 0..200 and LW in {8, 16, 32}: the
// loads partition [p, p + left) in order, every length is in 1..LW, at LW = 32 a load that is not the only one lies inside
// one 32-entry line, and there are at most ceil(left / LW) + 1 loads.  Prints every failure and exits non-zero if there is one.
#include "spmm_chunk.h"

#include <cstdint>
#include <cstdio>
#include <vector>

using namespace rwr;

static int failures = 0;

static void fail(const char *what, int64_t p, int64_t left, int LW, int64_t at, int len)
{
    if (++failures <= 40)
        std::printf("FAIL %s: p=%lld left=%lld LW=%d load at %lld of %d\n", what, (long long)p, (long long)left, LW, (long long)at, len);
}

static_assert(spmm_next_load(5, 20, 32) == 20, "a list that fits is one load");
static_assert(spmm_next_load(5, 40, 32) == 27, "a longer list is cut at the next line");
static_assert(spmm_next_load(64, 40, 32) == 32 && spmm_next_load(7, 0, 32) == 0, "whole lines; nothing left");

int main()
{
    long checked = 0;
    for (int LW : {8, 16, 32})
        for (int64_t p0 = 0; p0 <= 95; ++p0)
            for (int64_t left0 = 0; left0 <= 200; ++left0) {
                std::vector<std::pair<int64_t, int>> loads;
                int64_t p = p0, left = left0;
                bool bad = false;
                while (left > 0) {
                    const int len = spmm_next_load(p, left, LW);
                    if (len < 1 || len > LW || len > left) {   // (a bad length would also stall or overrun this loop)
                        fail("length outside 1..min(LW, left)", p0, left0, LW, p, len);
                        bad = true;
                        break;
                    }
                    loads.push_back({p, len});
                    p += len;
                    left -= len;
                }
                if (bad) continue;
                if (spmm_next_load(p, 0, LW) != 0) fail("an empty rest must give 0", p0, left0, LW, p, spmm_next_load(p, 0, LW));
                // in-order partition of [p0, p0 + left0)
                int64_t at = p0;
                for (const auto &l : loads) {
                    if (l.first != at) fail("loads do not follow one another", p0, left0, LW, l.first, l.second);
                    at = l.first + l.second;
                }
                if (at != p0 + left0) fail("loads do not end at the list's end", p0, left0, LW, at, 0);
                if (LW == 32 && loads.size() > 1)
                    for (const auto &l : loads)
                        if (l.first / 32 != (l.first + l.second - 1) / 32) fail("load crosses a 32-entry line", p0, left0, LW, l.first, l.second);
                if ((int64_t)loads.size() > (left0 + LW - 1) / LW + 1)
                    fail("more than ceil(left / LW) + 1 loads", p0, left0, LW, (int64_t)loads.size(), 0);
                ++checked;
            }
    std::printf("%ld combinations, %d failures\n", checked, failures);
    return failures ? 1 : 0;
}
