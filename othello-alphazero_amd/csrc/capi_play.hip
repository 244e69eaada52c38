// C ABI, playing moves: the self-play move, adjudication by the exact solver,
// random openings and the arena. The searches between the moves are capi.hip's.

#include "capi_internal.h"

using namespace oamd;

// the move-choice part of a self-play config (all of it the arena uses)
static bool move_cfg_ok(const oamd_selfplay_config* cfg) {
    return cfg->temperature_moves >= 0 && cfg->temperature > 0.0f;
}

int oamd::selfplay_cfg_checks(const oamd_selfplay_config* cfg, const float* features_dev, const float* policy_dev) {
    if (!move_cfg_ok(cfg) || cfg->opening_moves < 0) return fail(OAMD_INVALID_ARGUMENT, "bad self-play config");
    if (cfg->emit_targets && (!features_dev || !policy_dev))
        return fail(OAMD_INVALID_ARGUMENT, "emit_targets needs features and policy buffers");
    return OAMD_OK;
}

SelfplayParams oamd::selfplay_params(const oamd_selfplay_config* cfg) {
    return SelfplayParams{cfg->temperature_moves, cfg->temperature, cfg->opening_moves, cfg->emit_targets};
}

// ---------------------------------------------------------------------------
// Adjudication by the exact solver. A call zeroes its pending
// slots on the caller's stream before the moves (adjudicate_begin), the move
// kernels mark them (tree_game.h end_of_game), and the resolve step, on the caller's stream
// after every group has joined, solves them and writes the outcome bits and
// the margins (adjudicate.hip). Everything is enqueued only.
// ---------------------------------------------------------------------------
int oamd::adjudicate_checks(int32_t max_empties, const int32_t* finished_dev) {
    if (max_empties < 0 || max_empties > kSolveMaxEmpties)
        return fail(OAMD_INVALID_ARGUMENT, "Expected 0 <= max_empties <= " + std::to_string(kSolveMaxEmpties) +
                                               ", but got " + std::to_string(max_empties) + ".");
    if (max_empties > 0 && !finished_dev)
        return fail(OAMD_INVALID_ARGUMENT, "adjudication needs the finished buffer");
    return OAMD_OK;
}

static oamd_position* adjudicate_pending(const oamd_engine* e) {
    return reinterpret_cast<oamd_position*>(e->adj.pending.get());
}

// n pending slots, zeroed; sp gets the adjudication fields
int oamd::adjudicate_begin(oamd_engine* e, int64_t n, int32_t max_empties, bool split, SelfplayParams* sp) {
    if (n <= 0) return OAMD_OK;
    const int64_t chunk = e->adj.chunk_for(n);
    if (int rc = e->adj.ensure(e->device, n, sizeof(oamd_position),
                               split ? solve_split_workspace_bytes(chunk) : solve_workspace_bytes(chunk)))
        return rc;
    HIPCHK(hipMemsetAsync(adjudicate_pending(e), 0, sizeof(oamd_position) * (size_t)n, e->stream));
    sp->adj_empties = max_empties;
    sp->adj_pending = adjudicate_pending(e);
    return OAMD_OK;
}

// accumulate: the arena's cumulative words (only ended matches are touched)
int oamd::adjudicate_resolve(oamd_engine* e, int64_t n, int32_t max_empties, bool split, int32_t* finished_dev,
                             int32_t* margin_dev, bool accumulate) {
    if (n <= 0) return OAMD_OK;
    AdjudicateWorkspace& w = e->adj;
    const oamd_position* pending = adjudicate_pending(e);
    constexpr int64_t kNoLimit = (1LL << kSolveStatusShift) - 1;  // <= 16 empties: the solver always finishes
    if (w.want_ms) HIPCHK(hipEventRecord(w.ev[0].get(), e->stream));
    for (int64_t c0 = 0; c0 < n; c0 += w.chunk_cap) {
        const int64_t nc = std::min<int64_t>(w.chunk_cap, n - c0);
        (split ? launch_solve_split : launch_solve)(pending + c0, nc, max_empties, kNoLimit, w.move_scores.get(),
                                                    w.score.get(), nullptr, w.flags.get(), nullptr, w.solve_ws.get(), 0,
                                                    w.cus, e->stream);
        launch_adjudicate_apply(pending + c0, w.score.get(), w.flags.get(), nc, finished_dev + c0,
                                margin_dev ? margin_dev + c0 : nullptr, accumulate ? 1 : 0, e->stream);
    }
    if (w.want_ms) HIPCHK(hipEventRecord(w.ev[1].get(), e->stream));
    w.timed = w.want_ms;
    ++w.resolves;
    LAUNCHCHK();
    return OAMD_OK;
}

int oamd::selfplay_move_enqueue(oamd_engine* e, const SelfplayParams& sp, int32_t* actions_dev, int32_t* finished_dev,
                                float* features_dev, float* policy_dev) {
    launch_selfplay_move(e->view(), sp, 0, e->G, actions_dev, finished_dev, features_dev, policy_dev, e->stream);
    LAUNCHCHK();
    return OAMD_OK;
}

extern "C" {

int oamd_engine_adjudicate_ms(oamd_engine* e, float* ms, int64_t* resolves) {
    if (!ms) return fail(OAMD_INVALID_ARGUMENT, "adjudication: ms is NULL");
    *ms = 0.0f;
    if (resolves) *resolves = e->adj.resolves;
    e->adj.want_ms = true;  // the resolve steps from here on record their events
    if (!e->adj.timed) return OAMD_OK;
    DeviceGuard dg(e->device);
    HIPCHK(hipEventSynchronize(e->adj.ev[1].get()));
    HIPCHK(hipEventElapsedTime(ms, e->adj.ev[0].get(), e->adj.ev[1].get()));
    return OAMD_OK;
}

int oamd_engine_selfplay_move_adjudicated(oamd_engine* e, const oamd_selfplay_config* cfg, int32_t* actions_dev,
                                          int32_t* finished_dev, float* features_dev, float* policy_dev,
                                          int32_t max_empties, int32_t split, int32_t* margin_dev) {
    if (int rc = adjudicate_checks(max_empties, finished_dev)) return rc;
    if (int rc = selfplay_cfg_checks(cfg, features_dev, policy_dev)) return rc;
    DeviceGuard dg(e->device);
    SelfplayParams sp = selfplay_params(cfg);
    if (max_empties == 0) return selfplay_move_enqueue(e, sp, actions_dev, finished_dev, features_dev, policy_dev);
    if (int rc = adjudicate_begin(e, e->G, max_empties, split != 0, &sp)) return rc;
    if (int rc = selfplay_move_enqueue(e, sp, actions_dev, finished_dev, features_dev, policy_dev)) return rc;
    return adjudicate_resolve(e, e->G, max_empties, split != 0, finished_dev, margin_dev, false);
}

int oamd_engine_selfplay_move(oamd_engine* e, const oamd_selfplay_config* cfg, int32_t* actions_dev,
                              int32_t* finished_dev, float* features_dev, float* policy_dev) {
    return oamd_engine_selfplay_move_adjudicated(e, cfg, actions_dev, finished_dev, features_dev, policy_dev, 0, 0,
                                                 nullptr);
}

int oamd_engine_random_openings(oamd_engine* e, int32_t max_moves, uint64_t seed) {
    if (max_moves < 0) return fail(OAMD_INVALID_ARGUMENT, "max_moves must be >= 0");
    DeviceGuard dg(e->device);
    launch_random_openings(e->view(), max_moves, seed, e->stream);
    LAUNCHCHK();
    e->exact_trees = false;  // every game was reset
    return OAMD_OK;
}

// ---------------------------------------------------------------------------
// Arena: G matches between two engines (arena.hip k_arena_begin / k_arena_move)
// ---------------------------------------------------------------------------
static int arena_checks(const oamd_engine* a, const oamd_engine* b) {
    if (!a || !b || a == b) return fail(OAMD_INVALID_ARGUMENT, "arena: expected two different engines");
    if (a->device != b->device) return fail(OAMD_INVALID_ARGUMENT, "arena: engines on different devices");
    if (a->G != b->G)
        return fail(OAMD_INVALID_ARGUMENT, "arena: engines hold different numbers of games (" + std::to_string(a->G) +
                                               " and " + std::to_string(b->G) + ")");
    if (a->stream != b->stream) return fail(OAMD_INVALID_ARGUMENT, "arena: engines on different streams");
    // matches are played with full searches
    if (a->playout_cap() || b->playout_cap())
        return fail(OAMD_INVALID_ARGUMENT, "arena: an engine has a playout cap set (the arena does not use it)");
    // ... and without forced playouts
    if (a->forced_playouts() || b->forced_playouts())
        return fail(OAMD_INVALID_ARGUMENT, "arena: an engine has forced playouts set (the arena does not use them)");
    // ... and without exact leaf values
    if (a->exact_leaves() || b->exact_leaves())
        return fail(OAMD_INVALID_ARGUMENT, "arena: an engine has exact leaves set (the arena does not use them)");
    return OAMD_OK;
}

static int arena_cfg_checks(const oamd_selfplay_config* cfg) {
    if (!cfg || !move_cfg_ok(cfg)) return fail(OAMD_INVALID_ARGUMENT, "arena: bad move config");
    return OAMD_OK;
}

int oamd_arena_begin(oamd_engine* a, oamd_engine* b, const int32_t* openings_dev, int32_t opening_plies,
                     const uint8_t* a_is_white_dev) {
    if (int rc = arena_checks(a, b)) return rc;
    if (opening_plies < 0) return fail(OAMD_INVALID_ARGUMENT, "arena: opening_plies must be >= 0");
    DeviceGuard dg(a->device);
    launch_arena_begin(a->view(), b->view(), a->seed, b->seed, opening_plies > 0 ? openings_dev : nullptr,
                       opening_plies, a_is_white_dev, a->stream);
    LAUNCHCHK();
    a->end_search();
    b->end_search();
    return OAMD_OK;
}

// The pending slots of a match (engine A's workspace, one per match) outlive a
// ply: arena_play zeroes them once and resolves once after the last ply; a
// single arena_move zeroes, moves and resolves.
int oamd_arena_move_adjudicated(oamd_engine* a, oamd_engine* b, const oamd_selfplay_config* cfg,
                                int32_t* actions_dev, int32_t* finished_dev, int32_t* discs_dev,
                                int32_t* remaining_dev, int32_t max_empties, int32_t split, int32_t* margin_dev) {
    if (int rc = adjudicate_checks(max_empties, finished_dev)) return rc;
    if (int rc = arena_checks(a, b)) return rc;
    if (int rc = arena_cfg_checks(cfg)) return rc;
    DeviceGuard dg(a->device);
    SelfplayParams sp{cfg->temperature_moves, cfg->temperature, 0, 0};
    if (max_empties > 0)
        if (int rc = adjudicate_begin(a, a->G, max_empties, split != 0, &sp)) return rc;
    launch_arena_move(a->view(), b->view(), sp, actions_dev, finished_dev, discs_dev, remaining_dev, a->stream);
    LAUNCHCHK();
    if (max_empties > 0) return adjudicate_resolve(a, a->G, max_empties, split != 0, finished_dev, margin_dev, true);
    return OAMD_OK;
}

int oamd_arena_move(oamd_engine* a, oamd_engine* b, const oamd_selfplay_config* cfg, int32_t* actions_dev,
                    int32_t* finished_dev, int32_t* discs_dev, int32_t* remaining_dev) {
    return oamd_arena_move_adjudicated(a, b, cfg, actions_dev, finished_dev, discs_dev, remaining_dev, 0, 0, nullptr);
}

int oamd_arena_play_adjudicated(oamd_engine* a, oamd_net* net_a, oamd_engine* b, oamd_net* net_b,
                                const oamd_selfplay_config* cfg, int32_t max_plies, int32_t* actions_dev,
                                int32_t* finished_dev, int32_t* discs_dev, int32_t* plies_host, int32_t max_empties,
                                int32_t split, int32_t* margin_dev) {
    if (int rc = adjudicate_checks(max_empties, finished_dev)) return rc;
    if (int rc = arena_checks(a, b)) return rc;
    if (int rc = arena_cfg_checks(cfg)) return rc;
    if (int rc = native_search_checks(a, net_a)) return rc;
    if (int rc = native_search_checks(b, net_b)) return rc;
    if (max_plies < 0) return fail(OAMD_INVALID_ARGUMENT, "arena: max_plies must be >= 0");
    if (!actions_dev || !finished_dev || !discs_dev)
        return fail(OAMD_INVALID_ARGUMENT, "arena: actions, finished and discs buffers are required");
    DeviceGuard dg(a->device);
    if (int rc = a->ensure_remaining()) return rc;
    const int G = a->G;
    hipStream_t s = a->stream;
    int32_t* remaining = a->remaining.dev.get();
    SelfplayParams sp{cfg->temperature_moves, cfg->temperature, 0, 0};
    if (max_empties > 0)
        if (int rc = adjudicate_begin(a, G, max_empties, split != 0, &sp)) return rc;
    // every byte 0xFF: action -1 in the plies that are never enqueued
    if (max_plies > 0) HIPCHK(hipMemsetAsync(actions_dev, 0xFF, sizeof(int32_t) * (size_t)max_plies * G, s));
    HIPCHK(hipMemsetAsync(finished_dev, 0, sizeof(int32_t) * G, s));
    HIPCHK(hipMemsetAsync(discs_dev, 0, sizeof(int32_t) * 2 * G, s));
    HIPCHK(hipMemsetAsync(remaining, 0, sizeof(int32_t), s));
    launch_arena_count(a->view(), remaining, s);
    LAUNCHCHK();
    constexpr int kReadEvery = 8;  // plies between two reads of the matches still running
    int ply = 0;
    for (;;) {
        HIPCHK(hipMemcpyAsync(a->remaining.host.get(), remaining, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (a->remaining.host.get()[0] <= 0 || ply >= max_plies) break;
        for (int k = 0; k < kReadEvery && ply < max_plies; ++k, ++ply) {
            // only the side to move of each match is active in its engine
            if (int rc = oamd_engine_search(a, net_a, nullptr, nullptr)) return rc;
            if (int rc = oamd_engine_search(b, net_b, nullptr, nullptr)) return rc;
            launch_arena_move(a->view(), b->view(), sp, actions_dev + (size_t)ply * G, finished_dev, discs_dev,
                              remaining, s);
            LAUNCHCHK();
        }
    }
    if (plies_host) *plies_host = ply;
    // the slots collected every match that ended in this call: margin is
    // written for all G (INT32_MIN: the match did not end here)
    if (max_empties > 0) return adjudicate_resolve(a, G, max_empties, split != 0, finished_dev, margin_dev, false);
    return OAMD_OK;
}

int oamd_arena_play(oamd_engine* a, oamd_net* net_a, oamd_engine* b, oamd_net* net_b, const oamd_selfplay_config* cfg,
                    int32_t max_plies, int32_t* actions_dev, int32_t* finished_dev, int32_t* discs_dev,
                    int32_t* plies_host) {
    return oamd_arena_play_adjudicated(a, net_a, b, net_b, cfg, max_plies, actions_dev, finished_dev, discs_dev,
                                       plies_host, 0, 0, nullptr);
}

}  // extern "C"
