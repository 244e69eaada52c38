// Host internals shared by the units of the C ABI (capi*.hip): the error
// plumbing, the two handle structs and the checks and steps that more than
// one unit uses. Not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>

#include "../../include/othello_mcts_amd.h"
#include "../../include/othello_mcts_amd_experimental.h"
#include "bitboard.h"

#include "engine.h"
#include "host_resources.h"
#include "kernels.h"
#include "replay.h"
#include "schedule.h"
#include "solver.h"
#include "timing.h"

static_assert(oamd::kStatusOk == OAMD_OK && oamd::kStatusRuntime == OAMD_RUNTIME, "host_resources.h status codes");

#define LAUNCHCHK()                                                                       \
    do {                                                                                  \
        hipError_t _e = hipGetLastError();                                                \
        if (_e != hipSuccess) return ::oamd::fail(OAMD_RUNTIME, std::string("kernel launch: ") + hipGetErrorString(_e)); \
    } while (0)

namespace oamd {

// Host waits for a readback (the adaptive extra rounds' cut counts, the
// free-running call's remaining-games counters and its enqueue throttle):
// off the GPU's critical path (the reads are two chunks late), so the thread
// polls the event and sleeps 100 us between polls instead of spinning a CPU
// in hipEventSynchronize (which spins here even on blocking-sync events:
// bench.py's rank table read 1.0 CPU-s per s either way). The host budget of
// 8 ranks on one node is what it saves (cpu_s_per_s).
// OAMD_SPIN_SYNC=1: hipEventSynchronize (A/B only).
inline bool spin_sync() {
    static const bool spin = [] {
        const char* v = std::getenv("OAMD_SPIN_SYNC");
        return v && v[0] == '1';
    }();
    return spin;
}
inline unsigned readback_event_flags() {
    return hipEventDisableTiming | (spin_sync() ? 0u : (unsigned)hipEventBlockingSync);
}
inline hipError_t host_wait(hipEvent_t ev) {
    if (spin_sync()) return hipEventSynchronize(ev);
    for (;;) {
        const hipError_t q = hipEventQuery(ev);
        if (q != hipErrorNotReady) return q;
        std::this_thread::sleep_for(std::chrono::microseconds(100));
    }
}
constexpr int kEvPerBlock = 4;  // timing events per (round, group): tree begin/end, NN begin/end
// device counters (k_tree): [0..1] sims / NN rows of the current search,
// [2..3] cumulative, [4..5] of timed searches, [6] summed descent depths,
// [7] deepest descent, [8..11] the tree work of oamd_engine_tree_work
// (children scanned, expansions, children created, tree launches),
// [12..14] exact leaves (oamd_engine_exact_leaf_counters): solves (the solve
// kernel), hits of solved leaves (k_tree), solver nodes (the solve kernel);
// [15] exact-leaf faults: rows backed up while still pending (k_tree)
constexpr int kCounters = 16;

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

inline bool has_device(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    return device >= 0 && device < n;
}
// the device of a new engine or net
inline int create_device_checks(int device) {
    if (!has_device(0)) return fail(OAMD_RUNTIME, "no HIP device available");
    if (!has_device(device)) return fail(OAMD_INVALID_ARGUMENT, "bad device ordinal");
    return OAMD_OK;
}

}  // namespace oamd

// ===========================================================================
// engine
// ===========================================================================
struct oamd_engine {
    int device = 0;
    int G = 0;
    int64_t cap = 0;
    oamd_search_config cfg{};
    hipStream_t stream = nullptr;
    uint64_t seed = 0;

    oamd::DeviceBuf<oamd::NodeLink> link;
    oamd::DeviceBuf<oamd::NodeStat> stat;
    oamd::DeviceBuf<oamd::NodePos> pos;
    oamd::DeviceBuf<oamd::GameState> games;
    oamd::RowBuffers rows;  // per-row buffers (sized for rows.rows_cap rows)
    // two evaluation-list counters per pipeline group (the round being
    // evaluated, the next round's)
    oamd::DeviceBuf<int32_t> rowcount;
    oamd::DeviceBuf<float> explore_tab;
    oamd::DeviceBuf<unsigned long long> counters;
    oamd::DeviceBuf<int32_t> status_dev;  // [0] games with pool overflow, [1] depth-capped games
    // query scratch
    oamd::DeviceBuf<oamd_root_info> info_dev;
    oamd::DeviceBuf<int32_t> visits_dev;
    oamd::DeviceBuf<float> q_dev;
    oamd::DeviceBuf<float> spd_dev;  // self-play data scratch (8*(1+2H)*64 + 8*65)
    // search state
    int steps_left = 0;
    int steps_total = 0;  // of the step-wise search begun by oamd_engine_search_begin
    bool exact_interleaving = true;  // oamd_engine_set_exact_interleaving
    // native search, exact interleaving: an all-terminal chain stops after
    // chain_budget re-selections in a round, at most X <= chain_cuts times
    // per search (k_tree), X extra rounds per search (pick_extra_rounds).
    // budget 0 = never split
    int chain_budget = 2;
    int chain_cuts = 64;
    // adaptive extra rounds (pick_extra_rounds; the rule: schedule.h), X
    // following the search two back
    static constexpr int kCutSlots = oamd::ReadbackSlots::kSlots;
    AdaptiveRounds adapt;
    int64_t adapt_seq = 0;   // grouped searches enqueued with a cuts slot
    // [kCutSlots][kMaxPipeline][2] per search and group: most cuts, fewest root empties
    oamd::ReadbackSlots cuts;
    int cut_x[kCutSlots] = {-1, -1, -1, -1};  // X of the search in the slot (-1: slot empty)
    int cut_groups[kCutSlots] = {};
    // free-running self-play (oamd_engine_selfplay_steps, tree.hip k_tree_free):
    // games play their moves without waiting for each other; the host enqueues
    // rounds until every group's remaining-games counter (read back two chunks
    // late, pinned memory behind events) is 0
    bool free_running = true;
    // base chunks wait for the chunk two back before they are enqueued
    // (OAMD_SPIN_SYNC=1: no wait, A/B only)
    bool throttle_enqueue = !oamd::spin_sync();
    static constexpr int kFreeSlots = oamd::ReadbackSlots::kSlots;
    static constexpr int kFreeTailRounds = 4;
    oamd::ReadbackSlots remaining;  // dev [kMaxPipeline], host [kFreeSlots][kMaxPipeline]
    int ensure_remaining() {
        return remaining.ensure((size_t)kMaxPipeline, (size_t)kFreeSlots * kMaxPipeline, oamd::readback_event_flags(),
                                "free-running slots");
    }
    oamd::AdjudicateWorkspace adj;  // oamd_engine_selfplay_*_adjudicated, oamd_arena_*_adjudicated
    // playout cap randomization (oamd_engine_set_playout_cap):
    // cap_fast = 0 is off; else a search is full with probability cap_p and
    // runs cap_fast simulations without root noise otherwise
    float cap_p = 1.0f;
    int cap_fast = 0;
    bool playout_cap() const { return cap_fast > 0; }
    // why a search config cannot carry the current cap (nullptr: it can)
    const char* playout_cap_conflict(const oamd_search_config& c) const {
        if (!playout_cap()) return nullptr;
        if (thread_split_shape(G, c.num_threads))
            return "the playout cap does not run on the single-game thread-split schedule (num_games = 1, "
                   "num_threads > 1)";
        if (cap_fast > c.num_simulations) return "the playout cap's fast_simulations exceeds num_simulations";
        return nullptr;
    }
    // forced playouts and policy target pruning (oamd_engine_set_forced_playouts,
    // DESIGN.md §18): forced_k = 0 is off
    float forced_k = 0.0f;
    bool prune_targets = false;
    bool forced_playouts() const { return forced_k > 0.0f; }
    // exact leaf values (oamd_engine_set_exact_leaves): 0 is off.
    // exact_trees: a search ran since the last reset of all games, so some
    // tree was built under the current value and the value may not change
    int exact_empties = 0;
    bool exact_trees = false;
    bool exact_leaves() const { return exact_empties > 0; }
    // workgroups of an extra round's ResNet launch (0 = the regular grid)
    int extra_grid = 128;
    int step_phase = 0;  // 1 = a selected round awaits its backup (step API)
    // pipeline groups (0 = auto); their streams, fork / join events and NN tokens
    int pipeline = 0;
    // rows per k_resnet launch (0 = one launch per group and step); a group's
    // rows are evaluated by consecutive launches on its stream
    int nn_batch = 0;
    oamd::PipelineStreams pipe;
    int nn_chains = 2;  // NN chains (PipelineStreams::nn_token)
    // timing: kEvPerBlock events per (step, group) of a search, in two pools used in
    // turn, so a search never waits for the previous one's events; a pool is
    // summed (waiting for its last event) before reuse or on a timing query
    bool timing = false;
    int timing_stride = 1;     // time every timing_stride-th search (sampled timing)
    int64_t search_count = 0;
    oamd::TimingPools pools;
    int ev_blocks[2] = {0, 0};  // pending (round, group) blocks per pool
    int ev_final[2] = {0, 0};   // first block of the backup-only final round
    int64_t ev_launches[2] = {0, 0};  // k_resnet launches inside those blocks
    int64_t ev_rows[2] = {0, 0};
    oamd::SpanWindow spans;  // NN busy time (oamd_engine_nn_busy), recorded while timing is enabled
    int ev_cur = 0;
    float nn_ms = 0.0f;
    float select_ms = 0.0f;
    float backup_ms = 0.0f;
    int64_t nn_launches = 0;
    int64_t tree_launches = 0;  // timed select rounds (one k_tree launch per round and group)
    int64_t tree_final_launches = 0;  // timed final backup-only rounds (x groups)
    int64_t grouped_searches = 0, grouped_rounds = 0;  // oamd_engine_round_counts
    int64_t nn_rows = 0;

    int resolve_timing(int p) {
        const int n = ev_blocks[p];
        if (!n) return OAMD_OK;
        // NN launch intervals relative to the search's first event: their
        // union is the time some ResNet launch ran (launches of different NN
        // chains overlap; with one chain the union is the sum of durations)
        for (int i = 0; i < n; ++i) {
            const oamd::Event* b = &pools.ev[p][oamd::kEvPerBlock * i];
            float ms = 0.0f;
            // blocks of different groups end on different streams; the final
            // round records no NN events
            const bool nn = i < ev_final[p];
            HIPCHK(hipEventSynchronize(b[1].get()));
            if (nn) HIPCHK(hipEventSynchronize(b[3].get()));
            HIPCHK(hipEventElapsedTime(&ms, b[0].get(), b[1].get()));
            (i < ev_final[p] ? select_ms : backup_ms) += ms;
            if (nn) {
                HIPCHK(hipEventElapsedTime(&ms, b[2].get(), b[3].get()));
                nn_ms += ms;
            }
        }

        nn_launches += ev_launches[p];
        tree_launches += ev_final[p];
        tree_final_launches += n - ev_final[p];
        nn_rows += ev_rows[p];
        ev_blocks[p] = 0;
        return OAMD_OK;
    }
    int resolve_all_timing() {
        int rc = resolve_timing(ev_cur ^ 1);
        return rc ? rc : resolve_timing(ev_cur);
    }
    // n contiguous span slots for one search (nullptr when timing is off)
    int reserve_spans(int64_t n, unsigned long long** out) {
        *out = nullptr;
        return timing ? spans.reserve(n, out) : OAMD_OK;
    }

    int L() const { return cfg.num_threads * cfg.batch_size; }
    int steps() const { return search_steps(cfg.num_simulations, L()); }
    // a search (or what replaces it: a reset, a new config) leaves no step-wise search open
    void end_search() {
        step_phase = 0;
        steps_left = 0;
    }
    // thread-split schedule for one game (OAMD_TREE_SPLIT=0 in the environment: off)
    bool thread_split() const {
        static const bool v = [] {
            const char* e = getenv("OAMD_TREE_SPLIT");
            return e ? atoi(e) != 0 : true;
        }();
        // exact leaves run on the grouped schedule, whose rounds carry the solve kernel
        return v && !exact_leaves() && thread_split_shape(G, cfg.num_threads);
    }
    int FW() const { return oamd::feature_words(cfg.history_size); }

    oamd::EngineView view() const {
        oamd::EngineView E;
        E.G = G;
        E.L = L();
        E.H = cfg.history_size;
        E.FW = FW();
        E.cap = cap;
        E.link = link.get();
        E.stat = stat.get();
        E.pos = pos.get();
        E.games = games.get();
        E.leaf = rows.leaf.get();
        E.depth = rows.depth.get();
        E.trans = rows.trans.get();
        E.path = rows.path.get();
        E.feat = rows.feat.get();
        E.policy = rows.policy.get();
        E.value = rows.value.get();
        E.explore_tab = explore_tab.get();
        E.c_base = cfg.c_puct_base;
        E.c_init = cfg.c_puct_init;
        E.eps = cfg.dirichlet_epsilon;
        E.alpha = cfg.dirichlet_alpha;
        E.counters = counters.get();
        E.rowlist = rows.rowlist.get();
        E.tstate = rows.tstate.get();
        E.steps = steps();
        E.B = cfg.batch_size;
        E.terminal_skip = exact_interleaving ? 1 : 0;
        E.fast_steps = playout_cap() ? search_steps(cap_fast, L()) : 0;
        E.full_probability = cap_p;
        E.forced_k = forced_k;
        E.prune_targets = forced_playouts() && prune_targets ? 1 : 0;
        E.exact_empties = exact_empties;
        E.exact = rows.exact.get();
        return E;
    }
};

// ===========================================================================
// net
// ===========================================================================
struct oamd_net {
    int device = 0;
    oamd_net_desc desc{};
    oamd::DeviceBuf<uint16_t> w;
    oamd::DeviceBuf<float> bias;
    oamd::DeviceBuf<float> head;
    oamd::DeviceBuf<uint16_t> hconv;
    bool loaded = false;
    // oamd_debug_forward_packed: its evaluation list, the counter behind it
    oamd::DeviceBuf<int32_t> debug_list;
    int64_t debug_list_cap = 0;
    std::vector<std::string> keys;
    std::vector<int64_t> numel;

    oamd::NetView view() const {
        oamd::NetView N;
        N.cin = desc.in_channels;
        N.C = desc.conv_channels;
        N.R = desc.num_residual_blocks;
        N.hidden = desc.value_head_hidden_channels;
        N.dtype = desc.dtype;
        N.w = w.get();
        N.bias = bias.get();
        N.head = head.get();
        N.hconv = hconv.get();
        return N;
    }
};

namespace oamd {

// Pipeline groups of a native search: the games split into K contiguous
// groups, each on its own stream, so one group's tree kernels (latency-bound,
// a wave per game) run while another group's ResNet launch owns the MFMA
// units. Games are independent, so the results are identical for every K.
struct GroupPlan : GroupSplit {
    hipStream_t st[kMaxPipeline] = {};
    // ResNet launches of one round: the most of any group (a search's busy-time
    // slots are [group][round][launch]) and over all groups; its rows
    int max_launches = 1;
    int64_t round_launches = 0, round_rows = 0;
};

inline int native_search_checks(const oamd_engine* e, const oamd_net* net) {
    if (!net || !net->loaded) return fail(OAMD_INVALID_ARGUMENT, "native net not loaded");
    if (net->device != e->device) return fail(OAMD_INVALID_ARGUMENT, "net and engine on different devices");
    if (net->desc.in_channels != 1 + 2 * e->cfg.history_size)
        return fail(OAMD_INVALID_ARGUMENT, "net in_channels != 1 + 2 * history_size");
    return OAMD_OK;
}

// capi_play.hip, used by the multi-move self-play of capi.hip as well
int selfplay_cfg_checks(const oamd_selfplay_config* cfg, const float* features_dev, const float* policy_dev);
SelfplayParams selfplay_params(const oamd_selfplay_config* cfg);
int selfplay_move_enqueue(oamd_engine* e, const SelfplayParams& sp, int32_t* actions_dev, int32_t* finished_dev,
                          float* features_dev, float* policy_dev);
int adjudicate_checks(int32_t max_empties, const int32_t* finished_dev);
int adjudicate_begin(oamd_engine* e, int64_t n, int32_t max_empties, bool split, SelfplayParams* sp);
int adjudicate_resolve(oamd_engine* e, int64_t n, int32_t max_empties, bool split, int32_t* finished_dev,
                       int32_t* margin_dev, bool accumulate);

}  // namespace oamd
