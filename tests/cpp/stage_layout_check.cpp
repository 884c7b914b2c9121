// Host check of recommendersystems_amd/csrc/stage_layout.h (tests/test_stage_layout.py): the staging copy of an
// ego-network-sized graph and its read-back area, at the smallest graphs, an odd one and both sides of the limits.
#include "stage_layout.h"

#include <cstdio>

using namespace rwr;

// the limits small.hip (small_path_ok) and append.hip (graph_append) test against, and the buffers are sized for
static_assert(ONE_LAUNCH_MAX_N == 8192, "node limit of the one-launch paths");
static_assert(ONE_LAUNCH_MAX_M == 65536, "link limit of the one-launch paths");

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d (n %d, m %lld): %s\n", __FILE__, __LINE__, n, (long long)m, #cond); } } while (0)

static void check(int32_t n, int64_t m)
{
    const StageLayout L = stage_layout(n, m);
    const size_t N = (size_t)n, M = (size_t)m;
    // every 8-byte array starts 8-aligned (node_id, rowptr, w); dst is read as int32
    CHECK(L.id % 8 == 0);
    CHECK(L.rp % 8 == 0);
    CHECK(L.w % 8 == 0);
    CHECK(L.dst % 4 == 0);
    // the six regions, in order and disjoint: [id, 8n) [rp, 8(n+1)) [w, 8m) [dst, 4m) [nt, n) [et, m)
    CHECK(L.id == 0);
    CHECK(L.id + 8 * N <= L.rp);
    CHECK(L.rp + 8 * (N + 1) <= L.w);
    CHECK(L.w + 8 * M <= L.dst);
    CHECK(L.dst + 4 * M <= L.nt);
    CHECK(L.nt + N <= L.et);
    CHECK(L.et + M == L.total);
    // the copy ends below the read-back area, and the read-back area inside the buffer
    CHECK(L.total <= STAGE_OUT_OFF);
    CHECK(STAGE_OUT_OFF + stage_out_bytes(n) <= STAGE_BYTES);
    // the read-back offsets as the build wrote them out before they had names
    CHECK(STAGE_OUT_NNZ == 0);
    CHECK(STAGE_OUT_FLAGS == 8);
    CHECK(STAGE_OUT_IN_PTR == 32);
    CHECK(stage_out_dangling(n) == 32 + 8 * (N + 1));
    CHECK(stage_out_bytes(n) == 32 + 8 * (N + 1) + N);
    CHECK((STAGE_OUT_OFF + STAGE_OUT_IN_PTR) % 8 == 0);
}

int main()
{
    check(1, 0);
    check(1, 1);
    check(7, 9);
    check(8191, 65535);
    check(ONE_LAUNCH_MAX_N, ONE_LAUNCH_MAX_M);
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
