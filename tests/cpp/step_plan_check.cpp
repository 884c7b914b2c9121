// Host-side check of the step plan (recommendersystems_amd/csrc/step_plan.h), built against the header alone by
// tests/test_step_plan.py: pinned plans of a few groups, then DESIGN §3.3.1 / §3.3.2's rules as predicates over a sweep.
// Prints every failure and exits non-zero if there is one.
#include "step_plan.h"

#include <cstdio>
#include <initializer_list>
#include <string>
#include <vector>

using namespace rwr;

static int failures = 0;

static void fail(const std::string &what)
{
    if (++failures <= 40) std::printf("FAIL %s\n", what.c_str());
}

static std::string describe(const StepPlan &p)
{
    static const char *chains[] = {"none", "scan", "scan_side", "sparse", "roles", "simple"};
    std::string s = p.rows.kind == Rows::All ? "all" : p.rows.kind == Rows::Frontier ? "list" : "tail" + std::to_string(p.rows.level);
    for (auto f : {std::make_pair(p.probe, " probe"), {p.write_bits, " write"}, {p.mark, " mark"}, {p.terms_nz, " terms"}})
        if (f.first) s += f.second;
    s += std::string(" ") + chains[(int)p.chain];
    for (auto f : {std::make_pair(p.chain_side, " side"), {p.gate, " gate"}, {p.chain_self, " self"}, {p.form_z, " z"},
                   {p.seed_z, " seed_z"}})
        if (f.first) s += f.second;
    return s;
}

static std::vector<StepPlan> plans(const PlanConfig &c, int64_t T, int64_t steps)
{
    std::vector<StepPlan> v;
    for (int64_t it = 0; it < steps; ++it) v.push_back(plan_step(c, it, T));
    return v;
}

static void pin(const char *name, const PlanConfig &c, int64_t T, const std::vector<std::string> &want)
{
    const std::vector<StepPlan> got = plans(c, T, (int64_t)want.size());
    for (size_t i = 0; i < want.size(); ++i)
        if (describe(got[i]) != want[i])
            fail(std::string(name) + " step " + std::to_string(i) + ": got '" + describe(got[i]) + "', want '" + want[i] + "'");
}

// C4's shape: 6 M nodes, 33 links per node (sparse: two act steps), 32 seeds per tile, a full group; user seeds of a bipartite
// like-graph, whose only need bit below the four tail levels is bit 3
static PlanInput c4_input()
{
    PlanInput in;
    in.n = 6000000;
    in.nnz = 200000000;
    in.G = 32;
    in.tg = 192;
    in.ranking_only = true;
    return in;
}

static PlanConfig with_tails(PlanConfig c, int depth, unsigned need)
{
    if (c.tails) c.tail_depth = depth, c.need = need;
    return c;
}

static void pinned()
{
    const std::string fold = " roles side gate z seed_z", sparse = " sparse side gate z seed_z";
    const PlanConfig c4 = with_tails(plan_config(c4_input()), 4, 8u);
    pin("C4", c4, 10,
        {"list probe write mark terms" + sparse, "list probe write mark terms" + sparse, "all probe write terms" + fold,
         "all probe terms" + fold, "all" + fold, "all" + fold, "tail3" + fold, "tail2 none z", "tail1 none z", "tail0 none"});
    int dense = 0, tail = 0, list = 0, chains = 0;
    for (const StepPlan &p : plans(c4, 10, 10)) {
        dense += p.dense();
        tail += p.rows.kind == Rows::Tail;
        list += p.rows.kind == Rows::Frontier;
        chains += p.chain != Chain::None;
    }
    if (dense != 2 || tail != 4 || list != 2 || chains != 7)
        fail("C4 launches: " + std::to_string(dense) + " dense, " + std::to_string(tail) + " row-list, " + std::to_string(list) +
             " frontier-list, " + std::to_string(chains) + " chains");

    PlanInput in = c4_input();
    in.tail_rows = 0;   // RWR_TAIL_ROWS=0
    pin("RWR_TAIL_ROWS=0", with_tails(plan_config(in), 4, 8u), 10,
        {"list probe write mark terms" + sparse, "list probe write mark terms" + sparse, "all probe write terms" + fold,
         "all probe terms" + fold, "all" + fold, "all" + fold, "all" + fold, "all" + fold, "all" + fold, "all roles side gate"});
    // RWR_TAIL_DEPTH=2: no need bit below the depth, so the last two steps are restricted and chainless
    pin("RWR_TAIL_DEPTH=2", with_tails(plan_config(c4_input()), 2, 8u), 10,
        {"list probe write mark terms" + sparse, "list probe write mark terms" + sparse, "all probe write terms" + fold,
         "all probe terms" + fold, "all" + fold, "all" + fold, "all" + fold, "all" + fold, "tail1 none z", "tail0 none"});
    in = c4_input();
    in.frontier_list = 0;   // RWR_FRONTIER_LIST=0
    pin("RWR_FRONTIER_LIST=0", with_tails(plan_config(in), 4, 8u), 10,
        {"all probe write mark" + sparse, "all probe write mark" + sparse, "all probe write" + fold, "all probe" + fold,
         "all" + fold, "all" + fold, "tail3" + fold, "tail2 none z", "tail1 none z", "tail0 none"});
    in = c4_input();
    in.act_iters = 0;   // RWR_ACT_ITERS=0: no act step, hence no frontier list either
    pin("RWR_ACT_ITERS=0", with_tails(plan_config(in), 4, 8u), 10,
        {"all probe write" + fold, "all probe write" + fold, "all probe write" + fold, "all probe" + fold, "all" + fold,
         "all" + fold, "tail3" + fold, "tail2 none z", "tail1 none z", "tail0 none"});

    // a single seed on a multi-million-node graph: three marked steps, the self-contained scan beside the SpMV, no row lists
    in = c4_input();
    in.G = 1, in.tg = 1, in.scan_self = true;
    const PlanConfig one = plan_config(in);
    if (one.tails || one.flist) fail("single seed: row lists allowed");
    const std::string scan = " scan_side side self";
    pin("single seed", with_tails(one, 4, 8u), 10,
        {"all probe write mark" + scan + " z", "all probe write mark" + scan + " z", "all probe mark" + scan + " z",
         "all" + scan + " z", "all" + scan + " z", "all" + scan + " z", "all" + scan + " z", "all" + scan + " z",
         "all" + scan + " z", "all" + scan});

    // rwr_model_run_batch, iteration mode: the last step is known, no row lists of either kind
    in = c4_input();
    in.ranking_only = false;
    const PlanConfig mb = plan_config(in);
    if (mb.tails || mb.flist) fail("model batch: row lists allowed");
    pin("model batch", mb, 10,
        {"all probe write mark" + sparse, "all probe write mark" + sparse, "all probe write" + fold, "all probe" + fold,
         "all" + fold, "all" + fold, "all" + fold, "all" + fold, "all" + fold, "all roles side gate"});
    // a threshold run (T = -1) may stop after any step: no step is the last, none lists, none is restricted
    pin("threshold run", c4, -1,
        {"all probe write mark terms" + sparse, "all probe write mark terms" + sparse, "all probe write terms" + fold,
         "all probe terms" + fold, "all" + fold, "all" + fold, "all" + fold, "all" + fold, "all" + fold, "all" + fold,
         "all" + fold, "all" + fold});
}

// DESIGN's rules, for every step of one plan
static void predicates(const std::string &name, const PlanConfig &c, int64_t T)
{
    const std::vector<StepPlan> v = plans(c, T, T);
    auto restricted = [&](int64_t i) { return v[i].rows.kind == Rows::Tail; };
    auto listed = [&](int64_t i) { return v[i].rows.kind == Rows::Frontier; };
    // a step writes every row if it is not restricted and either lists nothing or is step 1, which writes over the cleared X_0
    auto whole = [&](int64_t i) { return !restricted(i) && (!listed(i) || i == 1); };
    const int depth = c.tails ? c.tail_depth : 0;
    int64_t first_restricted = T, n_restricted = 0;
    for (int64_t i = T - 1; i >= 0 && restricted(i); --i) first_restricted = i, ++n_restricted;
    for (int64_t i = 0; i < T; ++i) {
        const StepPlan &p = v[i];
        const std::string at = name + " step " + std::to_string(i) + " (" + describe(p) + ")";
        if (listed(i) && !(p.mark && !restricted(i) && i + 1 < T && v[i + 1].probe && (v[i + 1].mark || i == 1)))
            fail(at + ": listed step");
        const bool reads_bitmap = p.probe || p.terms_nz || p.chain == Chain::Sparse;
        if (reads_bitmap && !(i == 0 || v[i - 1].write_bits)) fail(at + ": reads a bitmap its previous step did not write");
        if (restricted(i)) {
            const int64_t k = T - 1 - i;
            if (i < first_restricted) fail(at + ": restricted steps are no suffix");
            if (p.rows.level != k || k >= depth) fail(at + ": walks the wrong level");
            if (p.chain != Chain::None && !(i == first_restricted && ((c.need >> k) & 1u))) fail(at + ": chain of a restricted step");
        }
        const bool whole_chain = p.chain == Chain::Scan || p.chain == Chain::ScanSide || p.chain == Chain::Roles || p.chain == Chain::Simple;
        if (whole_chain && !(i == 0 || whole(i - 1))) fail(at + ": chain reads a step that did not write every row");
        if (p.form_z != (i != T - 1)) fail(at + ": forms z of the last step's ranks, or not of an earlier one's");
    }
    const unsigned below = depth > 0 ? c.need & ((1u << depth) - 1u) : 0u;
    if (c.tails && !below) {
        if (n_restricted != (T < depth ? T : depth)) fail(name + ": " + std::to_string(n_restricted) + " restricted steps");
        for (int64_t i = first_restricted; i < T; ++i)
            if (v[i].chain != Chain::None) fail(name + ": chain without a need bit");
    }
}

static void sweep()
{
    long plans_checked = 0;
    for (int chain : {1, 2})   // auto (the fold at this group size), the binade scan
        for (int lists : {0, 1})
            for (int act = 0; act <= 3; ++act)
                for (int nz = 0; nz <= 4; ++nz) {
                    PlanInput in = c4_input();
                    in.chain = chain, in.frontier_list = lists, in.act_iters = act, in.nz_iters = nz;
                    const PlanConfig base = plan_config(in);
                    for (int depth = 0; depth <= 4; ++depth)
                        for (unsigned need = 0; need < 16; ++need)
                            for (int64_t T = 0; T <= 12; ++T) {
                                const PlanConfig c = with_tails(base, depth, need);
                                predicates("chain " + std::to_string(chain) + " lists " + std::to_string(lists) + " act " +
                                               std::to_string(act) + " nz " + std::to_string(nz) + " depth " +
                                               std::to_string(depth) + " need " + std::to_string(need) + " T " + std::to_string(T),
                                           c, T);
                                ++plans_checked;
                            }
                }
    std::printf("%ld plans checked\n", plans_checked);
}

int main()
{
    pinned();
    sweep();
    std::printf("%d failures\n", failures);
    return failures != 0;
}
