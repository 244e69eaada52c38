// Host-side schedule arithmetic of the native search (capi.hip): the pipeline
// groups, the rounds and ResNet launches of a search, and the control law of
// the adaptive extra rounds. No HIP here, so the CPU tests compile it with
// g++ (tests/test_cpu_schedule.py) and hold it against bench.py's restatement.
#pragma once

#include <algorithm>
#include <cstdint>

constexpr int kMaxPipeline = 8;

// The games split into K contiguous, non-empty groups (pipeline 0 = auto: two
// groups from 64 games on).
struct GroupSplit {
    int K = 1;
    int g0[kMaxPipeline] = {}, ng[kMaxPipeline] = {};
};

inline GroupSplit split_groups(int G, int pipeline) {
    GroupSplit P;
    P.K = std::max(1, std::min({pipeline > 0 ? pipeline : (G >= 64 ? 2 : 1), G, kMaxPipeline}));
    for (int k = 0; k < P.K; ++k) {
        P.g0[k] = (int)((int64_t)G * k / P.K);
        P.ng[k] = (int)((int64_t)G * (k + 1) / P.K) - P.g0[k];
    }
    return P;
}

// One game with T > 1 virtual threads runs the thread-split schedule (a
// stream per thread; one game is always one group)
inline bool thread_split_shape(int G, int T) { return G == 1 && T > 1 && T <= kMaxPipeline; }

// Batches per virtual thread of one search = its NN rounds (search_thread.cpp:50-52)
inline int search_steps(int sims, int L) { return (sims + L - 1) / L; }

// nn_batch slices a group's rows into consecutive launches (0 = one launch)
inline int launch_rows(int group_rows, int nn_batch) { return nn_batch > 0 ? nn_batch : group_rows; }
inline int group_launches(int ng, int L, int nn_batch) {
    const int rows = ng * L, cb = launch_rows(rows, nn_batch);
    return (rows + cb - 1) / cb;
}

// The most extra rounds of a grouped search (chain splitting, k_tree): the
// reference's interleaving only. A cut follows >= budget all-terminal batches
// of its round, and a search has T x steps batches per game: no game can use
// more cuts than that
inline int extra_round_cap(bool exact_interleaving, int chain_budget, int chain_cuts, int T, int steps) {
    if (!exact_interleaving || chain_budget <= 0) return 0;
    return (int)std::min<int64_t>(chain_cuts, (int64_t)T * steps / chain_budget);
}

// Adaptive extra rounds: a grouped search runs X in [min(min_rounds, cap), cap]
// extra rounds (and allows X cuts), X following the searches read back so far.
// on = false: always the cap.
struct AdaptiveRounds {
    // endgame threshold: at most this many empty squares on some game's root
    // -> X = chain_cuts; raised past every root whose search needed cuts
    static constexpr int kEndgameEmpties = 12;
    bool on = true;
    int min_rounds = 1;
    int x = -1;  // the last X picked from a measurement (-1: none yet: the minimum)
    int empties = kEndgameEmpties;

    void reset(bool enable, int min) {
        on = enable;
        min_rounds = min;
        x = -1;  // the next searches run the minimum until one is read back
        empties = kEndgameEmpties;
    }
    // A finished search that ran x_search extra rounds: the most cuts any game
    // used (k_tree reports x_search + 1 for a game that ran out: X = 0 still
    // counts the chains that would have been split) and the fewest empty
    // squares of its roots.
    // The cuts come with the endgame: outside it no chain outlasts the budget
    // (used = 0), within ~9 empty squares of the end a game's whole search can
    // be all terminal (used = 12 of 50 batches per thread at budget 4;
    // profiles/r04/ab/adaptive_demand_log.txt). The root loses one empty
    // square per move, so the fewest empties two searches back announce the
    // endgame before it starts; a search that needed cuts raises the threshold
    // past its root, and the raised threshold decays by one per search without
    // cuts back to kEndgameEmpties (a mid-game chain must not pin
    // the full count for the engine's lifetime). Outside the endgame X = the
    // cuts used + the minimum, or 2X + 2 + the minimum when a game ran out.
    // (As the threshold is raised before it is compared, a search that used
    // cuts always counts as endgame: the last line runs with used = 0 only.
    // Kept as the engine has always applied it.)
    void observe(int x_search, int used, int fewest_empties, int chain_cuts) {
        if (used > 0) empties = std::max(empties, fewest_empties + 3);
        else if (empties > kEndgameEmpties) --empties;
        if (fewest_empties <= empties) x = chain_cuts;
        else x = (used > x_search ? 2 * x_search + 2 : used) + min_rounds;
    }
    // X of the next search. Nothing read back yet: the minimum (games usually
    // start from an opening, and a game that needs more cuts only runs a
    // longer round)
    int pick(int cap) const {
        if (!on) return cap;
        const int lo = std::min(min_rounds, cap);
        return x >= 0 ? std::clamp(x, lo, cap) : lo;
    }
};
