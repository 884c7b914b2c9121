// Which columns of a tile group of Models leave after which step (rwr_model_run_batch, rwr_model_run_restart_batch; DESIGN
// §3.9): every real column after step T in iteration mode, each column after the first step s >= 1 at which its own
// checkConvergence distance is below the threshold (Model.cs:64) otherwise.  Plain C++17 without HIP, so that
// tests/cpp/column_ends_check.cpp checks it against a per-column simulation; GroupColumns (iterate.h) carries it out.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace rwr {

struct ColumnEnds {
    const int32_t *slot_k;            // [nslots] batch position of the slot's column, -1 = a padding slot
    size_t nslots;
    bool by_count;                    // iteration mode: T steps; else until dist < threshold, T = the step limit
    int64_t T;
    double threshold;
    std::vector<uint8_t> out_done;    // [nslots] the slot's column has left
    int32_t real = 0, live = 0;       // real slots; those whose column has not left yet

    // (the drivers deal every tile's first slot a real column, so real > 0; a group of padding slots alone is done() at once)
    ColumnEnds(const int32_t *slot_k_, size_t nslots_, bool by_count_, int64_t T_, double threshold_)
        : slot_k(slot_k_), nslots(nslots_), by_count(by_count_), T(T_), threshold(threshold_), out_done(nslots_, 0)
    {
        for (size_t q = 0; q < nslots; ++q) real += slot_k[q] >= 0;
        live = real;
    }

    // whether a column can end after `steps` steps
    bool due(int64_t steps) const { return by_count ? steps == T : steps > 0; }

    // The columns whose run ends after `steps` steps (due(steps) holds; dist[q] = slot q's distance of that step, read in the
    // threshold modes only): row_of[q] = the column's staging row 0..m-1 in slot order, -1 for every other slot, and
    // iters_out[k] = steps where iters_out is given.  Returns m.
    int32_t leaving(int64_t steps, const double *dist, int32_t *row_of, int64_t *iters_out)
    {
        int32_t m = 0;
        for (size_t q = 0; q < nslots; ++q) {
            const int32_t k = slot_k[q];
            row_of[q] = -1;
            if (k < 0 || out_done[q] || !(by_count || dist[q] < threshold)) continue;   // Model.cs:64
            row_of[q] = m++;
            out_done[q] = 1;
            if (iters_out) iters_out[k] = steps;
        }
        live -= m;
        return m;
    }

    // the smallest batch position whose column has not left, -1 if there is none
    int32_t stuck() const
    {
        int32_t k = -1;
        for (size_t q = 0; q < nslots; ++q)
            if (slot_k[q] >= 0 && !out_done[q] && (k < 0 || slot_k[q] < k)) k = slot_k[q];
        return k;
    }

    bool done() const { return live == 0; }
};

}  // namespace rwr
