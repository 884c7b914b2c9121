// Host-side check of the device-memory block cache (recommendersystems_amd/csrc/pool.h), built against the header alone by
// tests/test_pool.py: once with the address and undefined-behaviour sanitizers, once with the thread sanitizer.  The raw
// allocator below hands out tokens that are never dereferenced, so the 2 GB and 256 MB caps are exercised at their real values
// without host memory; it counts its calls, traps a token that is released twice or unknown, and fails on request.  A side table
// of owners traps a block the cache hands out twice.  Both tables are relaxed atomics and take no lock, so that under the thread
// sanitizer they add no ordering of their own to the cache's.  Prints every failure and exits non-zero if there is one.
#include "pool.h"

#include <atomic>
#include <cstdint>
#include <cstdio>
#include <random>
#include <string>
#include <thread>
#include <vector>

using namespace rwr;

static std::atomic<int> failures{0};

static void fail(const std::string &what)
{
    if (++failures <= 40) std::printf("FAIL %s\n", what.c_str());
}
#define CHECK(cond, what) do { if (!(cond)) fail(std::string(what) + " (line " + std::to_string(__LINE__) + ")"); } while (0)

constexpr size_t MAX_TOKENS = (size_t)1 << 20, TOKEN_STEP = 4096;
constexpr int NOBODY = -1;

struct FakeRaw {
    // per token: 0 never handed out, 1 live, 2 released
    static inline std::atomic<uint8_t> state[MAX_TOKENS];
    static inline std::atomic<int> owner[MAX_TOKENS];       // the thread that holds the block through the cache, NOBODY = none
    static inline std::atomic<size_t> next{0}, allocs{0}, releases{0}, forgotten{0};
    static inline std::atomic<int> fail_next{0};            // the next so many alloc calls fail
    static inline thread_local int device = 0;
    static inline thread_local bool device_known = true;

    static void *token(size_t id) { return (void *)(uintptr_t)((id + 1) * TOKEN_STEP); }
    // the token's number; traps an address this allocator never made
    static size_t id_of(void *p)
    {
        const uintptr_t u = (uintptr_t)p;
        if (u == 0 || u % TOKEN_STEP != 0 || u / TOKEN_STEP > next.load(std::memory_order_relaxed)) {
            fail("unknown token");
            return MAX_TOKENS - 1;
        }
        return (size_t)(u / TOKEN_STEP - 1);
    }
    static void *alloc(size_t)
    {
        int k = fail_next.load(std::memory_order_relaxed);
        while (k > 0 && !fail_next.compare_exchange_weak(k, k - 1, std::memory_order_relaxed)) {}
        if (k > 0) return nullptr;
        const size_t id = next.fetch_add(1, std::memory_order_relaxed);
        if (id >= MAX_TOKENS - 1) { fail("token table full"); return nullptr; }
        if (state[id].exchange(1, std::memory_order_relaxed) != 0) fail("token handed out twice");
        owner[id].store(NOBODY, std::memory_order_relaxed);
        allocs.fetch_add(1, std::memory_order_relaxed);
        return token(id);
    }
    static void release(void *p)
    {
        const size_t id = id_of(p);
        if (state[id].exchange(2, std::memory_order_relaxed) != 1) fail("token released twice or never handed out");
        if (owner[id].load(std::memory_order_relaxed) != NOBODY) fail("token released raw while a caller holds it");
        releases.fetch_add(1, std::memory_order_relaxed);
    }
    static bool current_device(int *dev)
    {
        if (device_known) *dev = device;
        return device_known;
    }
    static void forget_failure() { forgotten.fetch_add(1, std::memory_order_relaxed); }

    static size_t live() { return allocs.load() - releases.load(); }
};

using Cache = BlockCache<FakeRaw>;

// the cache's two calls as thread `who` makes them, with the owner table kept: nobody else may hold a block handed out, and
// nobody else may have been handed it when it comes back
static void *take(int who, size_t bytes, size_t *got)
{
    void *p = Cache::alloc(bytes, got);
    if (p && FakeRaw::owner[FakeRaw::id_of(p)].exchange(who, std::memory_order_relaxed) != NOBODY) fail("block handed out while another caller holds it");
    return p;
}
static void give(int who, void *p, size_t got)
{
    if (FakeRaw::owner[FakeRaw::id_of(p)].exchange(NOBODY, std::memory_order_relaxed) != who) fail("block changed hands before its free");
    Cache::free(p, got);
}

// everything the caches hold goes back to the raw allocator: per device, POOL_MIN blocks are taken until one needs a raw call,
// which fails once and so empties the device's shared cache and, where it is that device's, the thread's; the blocks taken are
// then freed with a `got` of 0, which releases them raw
static void drain()
{
    const int dev0 = FakeRaw::device;
    for (int dev = 0; dev < POOL_DEVICES; ++dev) {
        FakeRaw::device = dev;
        std::vector<void *> taken;
        size_t got = 0;
        FakeRaw::fail_next = 1;
        while (FakeRaw::fail_next.load() != 0) taken.push_back(take(0, POOL_MIN, &got));
        for (void *p : taken) give(0, p, 0);
    }
    FakeRaw::device = dev0;
}

struct Counters { size_t allocs, releases; };
static Counters counters() { return {FakeRaw::allocs.load(), FakeRaw::releases.load()}; }

static void single_threaded()
{
    size_t got = 0;
    FakeRaw::device = 0;

    // reserved sizes: the smallest power of two >= max(POOL_MIN, request)
    for (size_t bytes : {(size_t)1, POOL_MIN - 1, POOL_MIN, POOL_MIN + 1, POOL_MAX - 1, POOL_MAX}) {
        size_t want = POOL_MIN;
        while (want < bytes) want <<= 1;
        void *p = take(0, bytes, &got);
        CHECK(p && got == want, "reserved size of " + std::to_string(bytes) + " bytes is " + std::to_string(got));
        give(0, p, got);
    }
    CHECK((POOL_MIN << (POOL_CLASSES - 1)) == POOL_MAX, "POOL_CLASSES spans POOL_MIN .. POOL_MAX");
    drain();
    CHECK(FakeRaw::live() == 0, "drain leaves nothing live");

    {   // oversized: exactly the request, raw both ways, every time
        for (int rep = 0; rep < 2; ++rep) {
            const Counters c0 = counters();
            void *p = take(0, POOL_MAX + 1, &got);
            CHECK(p && got == POOL_MAX + 1, "an oversized request reserves exactly itself");
            CHECK(counters().allocs == c0.allocs + 1, "an oversized request goes to the raw allocator");
            give(0, p, got);
            CHECK(counters().releases == c0.releases + 1, "an oversized block is released raw");
        }
        CHECK(Cache::thread_counts().blocks == 0 && Cache::shared_counts(0).blocks == 0, "oversized blocks are not cached");
    }

    {   // reuse: a freed block is the next one of its class, without a raw call
        void *a = take(0, 3000, &got);
        void *b = take(0, 3000, &got);
        give(0, a, got);
        const Counters c0 = counters();
        void *c = take(0, 2049, &got);
        CHECK(c == a && got == 4096, "the freed block is handed out next");
        CHECK(counters().allocs == c0.allocs, "reuse makes no raw call");
        void *d = take(0, 4097, &got);
        CHECK(d && d != a && d != b && got == 8192, "another class does not get the block");
        give(0, d, got);
        give(0, b, 4096);
        give(0, c, 4096);
        drain();
    }

    {   // per-thread per-class cap
        std::vector<void *> ps;
        for (size_t i = 0; i < TL_PER_CLASS + 1; ++i) ps.push_back(take(0, POOL_MIN, &got));
        for (void *p : ps) give(0, p, got);
        CHECK(Cache::thread_counts().blocks == TL_PER_CLASS, "TL_PER_CLASS blocks of a class stay with the thread");
        CHECK(Cache::shared_counts(0).blocks == 1 && Cache::shared_counts(0).bytes == POOL_MIN, "the next one goes to the shared cache");
        drain();
    }

    {   // per-thread byte cap, then the shared cap: the free that would pass POOL_CAP is released raw
        const size_t tl_fit = TL_CAP / POOL_MAX, shared_fit = POOL_CAP / POOL_MAX;
        std::vector<void *> ps;
        for (size_t i = 0; i < tl_fit + shared_fit + 1; ++i) ps.push_back(take(0, POOL_MAX, &got));
        const Counters c0 = counters();
        for (size_t i = 0; i < ps.size(); ++i) {
            give(0, ps[i], got);
            CHECK(Cache::thread_counts().bytes <= TL_CAP, "the thread's cache stays within TL_CAP");
            CHECK(Cache::shared_counts(0).bytes <= POOL_CAP, "the shared cache stays within POOL_CAP");
            if (i + 1 == tl_fit) CHECK(Cache::thread_counts().bytes == tl_fit * POOL_MAX && Cache::shared_counts(0).blocks == 0, "the thread's cache fills first");
            if (i + 1 == tl_fit + 1) CHECK(Cache::thread_counts().blocks == tl_fit && Cache::shared_counts(0).blocks == 1, "its overflow goes to the shared cache");
            if (i + 1 == tl_fit + shared_fit) CHECK(counters().releases == c0.releases, "no raw release below the caps");
        }
        CHECK(Cache::shared_counts(0).blocks == shared_fit && Cache::shared_counts(0).bytes == shared_fit * POOL_MAX, "the shared cache holds POOL_CAP");
        CHECK(counters().releases == c0.releases + 1, "the free past POOL_CAP is released raw");
        drain();
    }

    {   // one device per thread cache
        void *a = take(0, 1000, &got);
        give(0, a, got);                                  // (device 0: the thread's cache is device 0's now)
        FakeRaw::device = 1;
        const Counters c0 = counters();
        void *b = take(0, 1000, &got);
        CHECK(b && b != a && counters().allocs == c0.allocs + 1, "device 1 does not get a block freed on device 0");
        give(0, b, got);
        CHECK(Cache::thread_counts().blocks == 1, "the thread's cache keeps device 0's block only");
        CHECK(Cache::shared_counts(1).blocks == 1 && Cache::shared_counts(0).blocks == 0, "the block freed under device 1 is in device 1's shared cache");
        void *c = take(0, 1000, &got);
        CHECK(c == b && counters().allocs == c0.allocs + 1, "device 1 gets its own block back");
        give(0, c, got);
        FakeRaw::device = 0;
        void *d = take(0, 1000, &got);
        CHECK(d == a, "device 0 gets its own block back");
        give(0, d, got);
        drain();
    }

    {   // a device outside [0, POOL_DEVICES), or none known: raw both ways
        for (int which = 0; which < 3; ++which) {
            FakeRaw::device = which == 0 ? POOL_DEVICES : which == 1 ? -1 : 0;
            FakeRaw::device_known = which != 2;
            const Counters c0 = counters();
            void *p = take(0, 1000, &got);
            CHECK(p && got == 1024 && counters().allocs == c0.allocs + 1, "an out-of-range device allocates raw");
            give(0, p, got);
            CHECK(counters().releases == c0.releases + 1, "an out-of-range device releases raw");
            void *q = take(0, 1000, &got);
            CHECK(q && q != p && counters().allocs == c0.allocs + 2, "... every time");
            give(0, q, got);
        }
        FakeRaw::device = 0;
        FakeRaw::device_known = true;
        CHECK(Cache::thread_counts().blocks == 0, "nothing of it was cached");
    }

    {   // out of memory, retry succeeds: this device's shared blocks and the thread's own go back, another device's stay
        std::vector<void *> ps;
        FakeRaw::device = 1;
        void *other = take(0, POOL_MIN, &got);
        for (size_t i = 0; i < TL_PER_CLASS + 3; ++i) ps.push_back(take(0, POOL_MIN, &got));
        for (void *p : ps) give(0, p, POOL_MIN);          // (TL_PER_CLASS with the thread, 3 shared on device 1)
        FakeRaw::device = 0;
        give(0, other, POOL_MIN);                         // (shared on device 0: the thread's cache is device 1's)
        FakeRaw::device = 1;
        CHECK(Cache::thread_counts().blocks == TL_PER_CLASS && Cache::shared_counts(1).blocks == 3 && Cache::shared_counts(0).blocks == 1, "the caches before the failure");
        const Counters c0 = counters();
        const size_t f0 = FakeRaw::forgotten.load();
        FakeRaw::fail_next = 1;
        void *p = take(0, 4 * POOL_MIN, &got);
        CHECK(p && got == 4 * POOL_MIN, "the retry succeeds");
        CHECK(FakeRaw::fail_next.load() == 0 && FakeRaw::forgotten.load() == f0 + 1, "one failure, forgotten once");
        CHECK(counters().releases == c0.releases + TL_PER_CLASS + 3, "the device's shared blocks and the thread's own are released raw");
        CHECK(counters().allocs == c0.allocs + 1, "one raw allocation succeeded");
        CHECK(Cache::thread_counts().blocks == 0 && Cache::thread_counts().bytes == 0 && Cache::shared_counts(1).blocks == 0 && Cache::shared_counts(1).bytes == 0, "both are empty afterwards");
        CHECK(Cache::shared_counts(0).blocks == 1 && Cache::shared_counts(0).bytes == POOL_MIN, "another device's cache is untouched");
        give(0, p, got);
        FakeRaw::device = 0;
        drain();
    }

    {   // out of memory, retry fails: null, nothing leaked, nothing released twice
        std::vector<void *> ps;
        for (int i = 0; i < 5; ++i) ps.push_back(take(0, 5000, &got));
        for (void *p : ps) give(0, p, got);
        const Counters c0 = counters();
        FakeRaw::fail_next = 2;
        void *p = take(0, POOL_MIN, &got);
        CHECK(p == nullptr && got == POOL_MIN, "two failures give null");
        CHECK(FakeRaw::fail_next.load() == 0, "the allocation is retried once");
        CHECK(counters().allocs == c0.allocs && counters().releases == c0.releases + 5, "the cached blocks went back, once each");
        CHECK(FakeRaw::live() == 0 && Cache::thread_counts().blocks == 0 && Cache::shared_counts(0).blocks == 0, "nothing is left");
    }

    {   // a `got` that is no class size: released raw
        for (size_t bad : {POOL_MIN / 2, POOL_MIN + POOL_MIN / 2, 3 * POOL_MIN, POOL_MAX - 1, 2 * POOL_MAX, (size_t)0}) {
            void *p = take(0, POOL_MIN, &got);
            const Counters c0 = counters();
            give(0, p, bad);
            CHECK(counters().releases == c0.releases + 1, "got = " + std::to_string(bad) + " is released raw");
        }
        const Counters c0 = counters();
        Cache::free(nullptr, POOL_MIN);
        CHECK(counters().releases == c0.releases && Cache::thread_counts().blocks == 0, "a null pointer is ignored");
    }

    {   // thread exit: what a thread held is in the shared cache, and another thread gets it without a raw call
        std::vector<void *> ps;
        std::thread t([&] {
            FakeRaw::device = 0;
            size_t g1 = 0;
            for (int i = 0; i < 4; ++i) ps.push_back(take(1, 70000, &g1));
            for (void *p : ps) give(1, p, g1);
            CHECK(Cache::thread_counts().blocks == 4 && Cache::shared_counts(0).blocks == 0, "the thread holds its blocks while it runs");
        });
        t.join();
        size_t reserved = 0;
        pool_class(70000, &reserved);
        CHECK(Cache::shared_counts(0).blocks == 4 && Cache::shared_counts(0).bytes == 4 * reserved, "an ended thread's blocks are in the shared cache");
        const Counters c0 = counters();
        for (int i = 0; i < 4; ++i) {
            void *p = take(0, 70000, &got);
            bool known = false;
            for (void *q : ps) known = known || q == p;
            CHECK(known, "another thread gets the ended thread's block");
            give(0, p, got);
        }
        CHECK(counters().allocs == c0.allocs, "... without a raw call");
        drain();
        CHECK(FakeRaw::live() == 0, "nothing live after the single-threaded cases");
    }
}

// Ten threads, the harness's count (Program.cs:11), interleave allocations and frees of mixed classes on two devices
static void threaded()
{
    constexpr int THREADS = 10, OPS = 4000, HOLD = 48;
    std::vector<std::thread> ts;
    for (int t = 0; t < THREADS; ++t)
        ts.emplace_back([t] {
            std::mt19937 rng(1234u + (unsigned)t);
            struct Held { void *p; size_t got; int dev; };
            std::vector<Held> held;
            FakeRaw::device = t % 2;
            auto drop = [&](size_t at) {
                FakeRaw::device = held[at].dev;         // (as every entry point binds the handle's device before it frees)
                give(t + 1, held[at].p, held[at].got);
                held[at] = held.back();
                held.pop_back();
            };
            for (int op = 0; op < OPS; ++op) {
                if (op % 500 == 499) FakeRaw::device = (int)(rng() % 2);
                if (held.size() < HOLD && (held.empty() || rng() % 2)) {
                    // mostly small classes, now and then a large or an oversized one
                    const unsigned r = rng() % 100;
                    const size_t bytes = r < 90 ? (size_t)1 << (rng() % 14) : r < 98 ? (size_t)1 << (14 + rng() % 12) : POOL_MAX + 1 + rng() % 4096;
                    size_t got = 0;
                    void *p = take(t + 1, bytes, &got);
                    if (!p || got < bytes) fail("threaded: allocation failed or too small");
                    else held.push_back({p, got, FakeRaw::device});
                } else {
                    drop(rng() % held.size());
                }
            }
            while (!held.empty()) drop(held.size() - 1);
        });
    for (auto &t : ts) t.join();
    size_t shared = 0;
    for (int dev = 0; dev < POOL_DEVICES; ++dev) shared += Cache::shared_counts(dev).blocks;
    CHECK(Cache::thread_counts().blocks == 0, "threaded: the main thread holds nothing");
    CHECK(FakeRaw::live() == shared, "threaded: raw allocations - raw releases = " + std::to_string(FakeRaw::live()) + ", the shared caches report " + std::to_string(shared));
    CHECK(shared > 0, "threaded: the ended threads left their blocks in the shared cache");
    drain();
    CHECK(FakeRaw::live() == 0, "threaded: nothing live after the drain");
}

int main()
{
    single_threaded();
    threaded();
    std::printf("%d failures\n", failures.load());
    return failures.load() ? 1 : 0;
}
