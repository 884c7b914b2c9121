// EXACT mode, the seed's own row as a literal fold.  Model.deliverRanks (Model.cs:76-100) adds into nextRank[seed], besides the
// seed's in-links, the restart mass of EVERY node interleaved in node order (Model.cs:91-93,96-97): an n-term sequential fp64
// chain per seed.  The kernels here reproduce it add by add -- one lane per seed (k_seed_chain, the reference form), over the
// non-zero rows only while X is sparse (k_seed_chain_sparse), or role-specialised with the rank matrix staged through LDS
// (k_seed_chain_roles, the default) -- on a second stream beside the batched SpMM of iterate.hip, which skips the seeds' rows
// and waits at k_gate until the fold's workgroups are resident.  k_seed_terms forms the addends of the links into the seeds
// ahead of the fold.  The parallel form of the same chain is the binade scan of chain_scan.hip; seed_row.h declares both.
//
// Arithmetic per link is the reference's:  rw = (1-d)*x_i  (Model.cs:84), then nextRank += rw * weight (Model.cs:87) -- two
// roundings, never an FMA (the file is built with -ffp-contract=off).
#include "seed_row.h"
#include "bool_dispatch.h"

#include <climits>

namespace rwr {

// EXACT mode: the seed's own row.  Model.cs:78-99 for target == seed: for i ascending,
// first i's links into the seed (list order), then the restart addend
// rank[i] - rw (non-dangling, Model.cs:91-93) or rank[i] (dangling, Model.cs:96-97).
template <int G>
__global__ __launch_bounds__(64) void k_seed_chain(int32_t n, int ntiles, const int64_t *__restrict__ in_ptr,
                                                   const int32_t *__restrict__ in_src,
                                                   const double *__restrict__ in_w,
                                                   const uint8_t *__restrict__ dangling,
                                                   const double *__restrict__ X, double *__restrict__ Y,
                                                   const int32_t *__restrict__ seeds, double c1,
                                                   uint32_t *__restrict__ nz_out)
{
    constexpr int U = 8;
    const int q = blockIdx.x * blockDim.x + threadIdx.x;   // (tile, k)
    if (q >= ntiles * G) return;
    const int tile = q / G, k = q % G;
    const int32_t s = seeds[q];
    if (s < 0) return;
    const double *x = X + (size_t)tile * (size_t)n * G + k;
    int64_t p = in_ptr[s];
    const int64_t e = in_ptr[s + 1];
    int32_t nxt = (p < e) ? in_src[p] : INT_MAX;
    double acc = 0.0;
    int32_t i = 0;
    for (; i + U <= n; i += U) {
        double xv[U];
        uint8_t dg[U];
#pragma unroll
        for (int u = 0; u < U; ++u) xv[u] = x[(size_t)(i + u) * G];
#pragma unroll
        for (int u = 0; u < U; ++u) dg[u] = dangling[i + u];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            double rw = c1 * xv[u];
            while (nxt == i + u) {
                acc += rw * in_w[p];
                ++p;
                nxt = (p < e) ? in_src[p] : INT_MAX;
            }
            acc += dg[u] ? xv[u] : (xv[u] - rw);
        }
    }
    for (; i < n; ++i) {
        double xi = x[(size_t)i * G];
        double rw = c1 * xi;
        while (nxt == i) {
            acc += rw * in_w[p];
            ++p;
            nxt = (p < e) ? in_src[p] : INT_MAX;
        }
        acc += dangling[i] ? xi : (xi - rw);
    }
    Y[(size_t)tile * (size_t)n * G + (size_t)s * G + k] = acc;
    if (nz_out && acc != 0.0)
        atomicOr(&nz_out[(size_t)tile * (((size_t)n + 31) / 32) + ((uint32_t)s >> 5)], 1u << (s & 31));
}

// Holds the main stream until `expected` chain workgroups have checked in (or ~1 ms has passed: the spin is
// bounded, so a chain kernel that cannot become fully resident only costs the overlap, never a hang).
// Without it the chain kernel, although launched first on a high-priority stream, is dispatched only after the
// SpMM's ~half-million workgroups have all been issued, i.e. it runs after the SpMM instead of beside it.
__global__ void k_gate(const unsigned int *__restrict__ gate, unsigned int expected)
{
    const long long t0 = __builtin_amdgcn_s_memrealtime();          // 100 MHz
    while (__hip_atomic_load(gate, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < expected) {
        if (__builtin_amdgcn_s_memrealtime() - t0 > 100000) break;  // 1 ms
        __builtin_amdgcn_s_sleep(32);
    }
}

// EXACT mode helper: the addends of the links INTO each seed, ((1-d) x_src) * w in list order
// (Model.cs:84,87 for target == seed), computed in parallel ahead of the sequential fold.
// (VF: X is the z matrix, whose entries ARE those addends)
template <int G, bool VF>
__global__ __launch_bounds__(256) void k_seed_terms(int32_t n, const int64_t *__restrict__ in_ptr,
                                                    const int32_t *__restrict__ in_src,
                                                    const double *__restrict__ in_w, const double *__restrict__ X,
                                                    const int32_t *__restrict__ seeds, double c1,
                                                    const int64_t *__restrict__ evoff, double *__restrict__ evterm,
                                                    const uint32_t *__restrict__ nz)
{
    const int slot = blockIdx.y;                 // tile * G + k
    const int32_t s = seeds[slot];
    if (s < 0) return;
    const int tile = slot / G, k = slot % G;
    const double *x = X + (size_t)tile * (size_t)n * G + k;
    const int64_t p0 = in_ptr[s], deg = in_ptr[s + 1] - p0;
    double *out = evterm + evoff[slot];
    // nz (frontier steps): the tile's bitmap of the rows of X that hold a non-zero.  A row whose bit is clear is zero or
    // stale and is never read: its addend is +0.0, what (1-d)*0*w gives with non-negative weights
    if (nz) nz += (size_t)tile * (((size_t)n + 31) / 32);
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < deg; q += (int64_t)gridDim.x * blockDim.x) {
        const int32_t i = in_src[p0 + q];
        if (nz && !((nz[(uint32_t)i >> 5] >> (i & 31)) & 1u)) {
            out[q] = 0.0;
        } else if (VF) {
            out[q] = x[(size_t)i * G];
        } else {
            const double rw = c1 * x[(size_t)i * G];
            out[q] = rw * in_w[p0 + q];
        }
    }
}

// EXACT mode while X is still sparse (iterations 0 and 1): all-zero rows add +0.0 to the seed row's chain, so the
// chain only has to visit the non-zero rows of X -- in ascending node order, taking the links INTO the seed that
// come from such a row first (Model.cs:85-93).  One wave per tile walks the tile's non-zero-row bitmap; lane = seed.
template <int G>
__global__ __launch_bounds__(64) void k_seed_chain_sparse(int32_t n, const int64_t *__restrict__ in_ptr,
                                                          const int32_t *__restrict__ in_src,
                                                          const uint8_t *__restrict__ dangling,
                                                          const double *__restrict__ X, double *__restrict__ Y,
                                                          const int32_t *__restrict__ seeds, double c1,
                                                          const int64_t *__restrict__ evoff,
                                                          const double *__restrict__ evterm,
                                                          const uint32_t *__restrict__ nz_x, uint32_t *__restrict__ nz_out,
                                                          unsigned int *__restrict__ gate)
{
    if (threadIdx.x == 0 && gate) __hip_atomic_fetch_add(gate, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int tile = blockIdx.x, lane = threadIdx.x;
    const size_t nzw = ((size_t)n + 31) / 32;
    const uint32_t *bits = nz_x + (size_t)tile * nzw;
    const double *x = X + (size_t)tile * (size_t)n * G;
    const bool consumer = lane < G;
    const int k = lane % G;
    int32_t s = -1;
    int64_t p = 0, e = 0;
    const double *termp = evterm;
    if (consumer) {
        s = seeds[tile * G + k];
        if (s >= 0) {
            p = in_ptr[s];
            e = in_ptr[s + 1];
            termp = evterm + evoff[tile * G + k] - p;
        }
    }
    double acc = 0.0;
    for (size_t w0 = 0; w0 < nzw; w0 += WAVE) {
        const uint32_t word = (w0 + lane < nzw) ? bits[w0 + lane] : 0u;
        unsigned long long mask = __ballot(word != 0u);
        while (mask) {
            const int l = __builtin_ctzll(mask);
            mask &= mask - 1;
            uint32_t wv = (uint32_t)__builtin_amdgcn_readlane((int)word, l);
            while (wv) {
                const int b = __builtin_ctz(wv);
                wv &= wv - 1;
                const int32_t i = (int32_t)((w0 + l) * 32 + b);
                if (consumer && s >= 0) {
                    while (p < e && in_src[p] < i) ++p;                 // links from all-zero rows: addend +0.0
                    while (p < e && in_src[p] == i) { acc += termp[p]; ++p; }   // links i -> seed first (Model.cs:85-88)
                    const double xi = x[(size_t)i * G + k];
                    const double rw = c1 * xi;
                    acc += dangling[i] ? xi : (xi - rw);                // then the restart addend (Model.cs:91-93,96-97)
                }
            }
        }
    }
    if (consumer && s >= 0) {
        Y[(size_t)tile * (size_t)n * G + (size_t)s * G + k] = acc;
        if (nz_out && acc != 0.0)
            atomicOr(&nz_out[(size_t)tile * nzw + ((uint32_t)s >> 5)], 1u << (s & 31));
    }
}

// EXACT mode, role-specialised form (the default): wave 0 only FOLDS, waves 1-6 only STAGE.
//   stagers: stream the tile's rank matrix in 48 KiB chunks, two chunks ahead of the fold (2 x 16 coalesced loads
//            in flight per lane), turn each value into its restart addend
//                rr_i = dangling_i ? x_i : x_i - (1-d)*x_i          (Model.cs:91,97)
//            and write it to LDS (double-buffered);
//   folder : adds the staged addends strictly in node order, 16 at a time from registers.  The addends of the
//            links INTO a seed (computed by k_seed_terms) are prefetched per lane two links ahead into registers;
//            a 32-row block that holds such a link is walked row by row so that the link's addend lands before
//            the row's restart addend (Model.cs:85-93).  The folder issues no other global loads, so the n-term
//            chain runs near the dependent v_add_f64 rate (~7.5 cycles per row).
constexpr int CH3_NSW = 6;                      // stager waves
constexpr int CH3_NST = CH3_NSW * WAVE;         // stager threads
constexpr int CH3_LPT = 16;                     // loads per stager thread and chunk
constexpr int CH3_CE = CH3_NST * CH3_LPT;       // 6144 doubles per chunk (48 KiB)
// MASK: X was not cleared and the step before wrote only its frontier list's rows.  nz_x is the tile's bitmap
// of the rows that step left non-zero; a row whose bit is clear is zero or stale, and the stagers take +0.0 for it -- by
// selection, since a stale value may be anything, NaN included.  Its restart addend is then 0 - fl((1-d) 0) = +0.0, which
// leaves the non-negative sum as it is: the fold is bitwise the one over the cleared matrix.  The folder does not change.
template <int G, bool MASK>
__global__ __launch_bounds__(WAVE + CH3_NST) void k_seed_chain_roles(
    int32_t n, const int64_t *__restrict__ in_ptr, const int32_t *__restrict__ in_src,
    const uint8_t *__restrict__ dangling, const double *__restrict__ X, double *__restrict__ Y,
    const int32_t *__restrict__ seeds, double c1, const int64_t *__restrict__ evoff,
    const double *__restrict__ evterm, uint32_t *__restrict__ nz_out, unsigned int *__restrict__ gate,
    const uint32_t *__restrict__ nz_x)
{
    // check in: the main stream holds the SpMM back (k_gate) until the chain workgroups own their CUs
    if (threadIdx.x == 0 && gate) __hip_atomic_fetch_add(gate, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    constexpr int CR = CH3_CE / G;                         // rows per chunk (a multiple of 32)
    static_assert(CR % 32 == 0, "chunk rows must be a multiple of 32");
    extern __shared__ double rr[];                         // [2][CH3_CE]
    const int tile = blockIdx.x;
    const double *x = X + (size_t)tile * (size_t)n * G;
    const int tid = threadIdx.x;
    const int64_t total = (int64_t)n * G;
    const int nchunks = (int)((total + CH3_CE - 1) / CH3_CE);
    if (MASK) nz_x += (size_t)tile * (((size_t)n + 31) / 32);

    if (tid >= WAVE) {
        // ------------------------------------------------------------------ stagers
        const int st = tid - WAVE;
        double rega[CH3_LPT], regb[CH3_LPT];
        uint8_t dga[CH3_LPT], dgb[CH3_LPT];
        // MASK: a chunk's rows start at a multiple of 32, so CR / 32 words of the bitmap cover it.  Every stager loads them all
        // with the chunk's values (the addresses are the same in every lane) instead of one word per value: the stagers run at
        // the rate their loads in flight allow, and a third load per value cost the fold 35 ms on C4
        constexpr int NW = MASK ? CR / 32 : 1;
        uint32_t bwa[NW], bwb[NW];
        const int64_t nzw = ((int64_t)n + 31) / 32;
#define CH3_LOAD(R, D, W, C)                                                    \
    {                                                                           \
        const int64_t base__ = (int64_t)(C) * CH3_CE;                           \
        _Pragma("unroll") for (int u = 0; u < CH3_LPT; ++u) {                   \
            int64_t el = base__ + (int64_t)u * CH3_NST + st;                    \
            el = el < total ? el : total - 1;                                   \
            R[u] = x[el];                                                       \
            D[u] = dangling[el / G];                                            \
        }                                                                       \
        if (MASK) {                                                             \
            _Pragma("unroll") for (int j = 0; j < NW; ++j) {                    \
                int64_t wi__ = (int64_t)(C) * (CR / 32) + j;                    \
                wi__ = wi__ < nzw ? wi__ : nzw - 1; /* (rows past n: staged as +0.0 whatever the word) */ \
                W[j] = nz_x[wi__];                                              \
            }                                                                   \
        }                                                                       \
    }
#define CH3_STAGE(R, D, W, C)                                                                           \
    {                                                                                                   \
        const int64_t base__ = (int64_t)(C) * CH3_CE;                                                   \
        double *buf__ = rr + (size_t)((C) & 1) * CH3_CE;                                                \
        _Pragma("unroll") for (int u = 0; u < CH3_LPT; ++u) {                                           \
            const int off = u * CH3_NST + st;                                                           \
            bool live__ = base__ + off < total;                                                         \
            if (MASK) { /* the row's bit: its word is one of at most three, known once u is unrolled */ \
                const int row__ = off / G, j0__ = (u * CH3_NST / G) >> 5;                               \
                uint32_t wd__ = W[j0__];                                                                \
                _Pragma("unroll") for (int dj = 1; dj <= 2; ++dj)                                       \
                    if (j0__ + dj < NW && (row__ >> 5) == j0__ + dj) wd__ = W[j0__ + dj < NW ? j0__ + dj : 0]; \
                live__ = live__ && ((wd__ >> (row__ & 31)) & 1u);                                       \
            }                                                                                           \
            const double xv = live__ ? R[u] : 0.0; /* past the end, outside the bitmap: +0.0, no effect */ \
            const double rw = c1 * xv;                                                                  \
            buf__[off] = D[u] ? xv : (xv - rw);                                                         \
        }                                                                                               \
    }
        static_assert(!MASK || (CH3_NST - 1) / G + 1 <= 64, "a thread's value of one load lies at most two bitmap words on");
        CH3_LOAD(rega, dga, bwa, 0)
        if (nchunks > 1) CH3_LOAD(regb, dgb, bwb, 1)
        for (int c = 0; c < nchunks; c += 2) {
            CH3_STAGE(rega, dga, bwa, c)
            if (c + 2 < nchunks) CH3_LOAD(rega, dga, bwa, c + 2)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
            __builtin_amdgcn_s_barrier();
            if (c + 1 < nchunks) {
                CH3_STAGE(regb, dgb, bwb, c + 1)
                if (c + 3 < nchunks) CH3_LOAD(regb, dgb, bwb, c + 3)
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
                __builtin_amdgcn_s_barrier();
            }
        }
#undef CH3_LOAD
#undef CH3_STAGE
        return;
    }

    // ---------------------------------------------------------------------- folder (wave 0)
    const bool consumer = tid < G;
    const int k = tid % G;
    int32_t s = -1;
    int64_t p = 0, e = 0;                                  // p = index of the link AFTER the pending one
    const int32_t *srcp = in_src;
    const double *termp = evterm;
    int32_t nxt = INT_MAX, raw_s = INT_MAX;                // current link's source row; pending link's (raw load)
    double tcur = 0.0, raw_t = 0.0;
    bool has2 = false;
    if (consumer) {
        s = seeds[tile * G + k];
        if (s >= 0) {
            p = in_ptr[s];
            e = in_ptr[s + 1];
            termp = evterm + evoff[tile * G + k] - p;      // termp[link index] = addend of that link
            if (p < e) { nxt = srcp[p]; tcur = termp[p]; ++p; }
            if (p < e) { raw_s = srcp[p]; raw_t = termp[p]; has2 = true; ++p; }
        }
    }
    double acc = 0.0;
    __builtin_amdgcn_s_setprio(3);
    for (int c = 0; c < nchunks; ++c) {
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
        const double *buf = rr + (size_t)(c & 1) * CH3_CE;
        const int64_t row0 = (int64_t)c * CR;
        // 32-row blocks, two register sets in flight: the 32 LDS reads of the NEXT block are issued before the 32
        // dependent adds of the current one, so the adds (7.5 cycles each, the chain's floor) never wait for LDS.
        // A block that holds a link into one of the tile's seeds takes the same adds from the same registers, but
        // before row u every lane whose pending link comes from that row takes it first (Model.cs:85-88).
#define CH3_READ(V, R0) _Pragma("unroll") for (int u = 0; u < 32; ++u) V[u] = buf[((R0) + u) * G + k];
#define CH3_FOLD(V, R0)                                                                                     \
    {                                                                                                       \
        const bool evt = __any(consumer && nxt < row0 + (R0) + 32);                                         \
        if (!evt) {                                                                                         \
            _Pragma("unroll") for (int u = 0; u < 32; ++u) acc += V[u];                                     \
        } else {                                                                                            \
            _Pragma("unroll") for (int u = 0; u < 32; ++u) {                                                \
                const int32_t i = (int32_t)(row0 + (R0)) + u;                                               \
                if (__any(consumer && nxt == i)) {                                                          \
                    while (consumer && nxt == i) {                                                          \
                        acc += tcur;                                                                        \
                        nxt = has2 ? raw_s : INT_MAX; /* promote the pending link (loaded at the last take) */ \
                        tcur = raw_t;                                                                       \
                        has2 = p < e; /* and fetch the one after it; untouched until then */                \
                        const int64_t pc = has2 ? p : e - 1;                                                \
                        raw_s = srcp[pc];                                                                   \
                        raw_t = termp[pc];                                                                  \
                        p += has2 ? 1 : 0;                                                                  \
                    }                                                                                       \
                }                                                                                           \
                acc += V[u]; /* then the restart addend (Model.cs:91-93,96-97) */                           \
            }                                                                                               \
        }                                                                                                   \
    }
        double ra[32], rb[32];
        CH3_READ(ra, 0)
#pragma unroll 1
        for (int r0 = 0; r0 + 64 <= CR; r0 += 64) {
            CH3_READ(rb, r0 + 32)
            CH3_FOLD(ra, r0)
            if (r0 + 64 < CR) CH3_READ(ra, r0 + 64)
            CH3_FOLD(rb, r0 + 32)
        }
        if (CR % 64 != 0) CH3_FOLD(ra, CR - 32)        // odd number of 32-row blocks (G = 64): ra already holds the last one
#undef CH3_READ
#undef CH3_FOLD
    }
    __builtin_amdgcn_s_setprio(0);
    if (consumer && s >= 0) {
        Y[(size_t)tile * (size_t)n * G + (size_t)s * G + k] = acc;
        if (nz_out && acc != 0.0)
            atomicOr(&nz_out[(size_t)tile * (((size_t)n + 31) / 32) + ((uint32_t)s >> 5)], 1u << (s & 31));
    }
}

// ------------------------------------------------------------------------------ host side (seed_row.h)

// the addends of the links into the seeds; tiny, runs on the MAIN stream ahead of the fork so that the chain kernel is
// the first thing its stream has to dispatch once the fork event fires (it must get its CUs before the SpMM's
// half-million workgroups flood the dispatcher, or it only starts when the SpMM drains)
void launch_seed_terms(rwr_graph *g, int G, int tg, const double *X, const int32_t *seeds, double c1, const int64_t *evoff,
                       hipStream_t s, const double *Zin, const uint32_t *nz)
{
    const unsigned term_blocks = g->max_in_deg > 256 * 8 ? 8u : cdiv((size_t)(g->max_in_deg > 0 ? g->max_in_deg : 1), 256);
    RWR_DISPATCH_G(G, bool_dispatch([&](auto v) {
        hipLaunchKernelGGL((k_seed_terms<GG, decltype(v)::value>), dim3(term_blocks, tg * GG), dim3(256), 0, s, g->n, g->in_ptr.p,
                           g->in_src.p, g->in_w.p, Zin ? Zin : X, seeds, c1, evoff, g->d_evterm.p, nz);
    }, Zin != nullptr));
}
void launch_chain(rwr_graph *g, int G, int tg, const double *X, double *Y, const int32_t *seeds, double c1, const int64_t *evoff,
                  uint32_t *nz_out, unsigned int *gate, hipStream_t s, Chain kind, const uint32_t *nz_x, bool masked)
{
    if (kind == Chain::Sparse) {   // X still sparse: visit only the non-zero rows of its bitmap nz_x
        RWR_DISPATCH_G(G, hipLaunchKernelGGL(k_seed_chain_sparse<GG>, dim3(tg), dim3(64), 0, s, g->n, g->in_ptr.p, g->in_src.p,
                                             g->dangling.p, X, Y, seeds, c1, evoff, g->d_evterm.p, nz_x, nz_out, gate));
        return;
    }
    if (kind == Chain::Roles) {
        constexpr size_t smem = 2 * CH3_CE * sizeof(double);
        // (per launch, not once per process: the attribute belongs to the current device, and one process may hold
        //  graphs on several devices)
        RWR_DISPATCH_G(G, bool_dispatch([&](auto m) {
            constexpr bool MASK = decltype(m)::value && GG >= 8;   // (frontier lists, hence stale rows, only at G >= 8)
            (void)hipFuncSetAttribute((const void *)k_seed_chain_roles<GG, MASK>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)smem);
            hipLaunchKernelGGL((k_seed_chain_roles<GG, MASK>), dim3(tg), dim3(WAVE + CH3_NST), smem, s, g->n, g->in_ptr.p,
                               g->in_src.p, g->dangling.p, X, Y, seeds, c1, evoff, g->d_evterm.p, nz_out, gate, nz_x);
        }, masked));
        return;
    }
    RWR_DISPATCH_G(G, hipLaunchKernelGGL(k_seed_chain<GG>, dim3(cdiv((size_t)tg * GG, 64)), dim3(64), 0, s, g->n, tg, g->in_ptr.p,
                                         g->in_src.p, g->in_w.p, g->dangling.p, X, Y, seeds, c1, nz_out));
}
void launch_gate(const unsigned int *gate, unsigned int expected, hipStream_t s)
{
    hipLaunchKernelGGL(k_gate, dim3(1), dim3(1), 0, s, gate, expected);
}

}  // namespace rwr
