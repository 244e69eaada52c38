// C ABI, data: the packed replay ring, the exact endgame solver, the baseline
// opponents and the relabelling of the ring's value targets. The caller owns
// every buffer.

#include "baseline.h"
#include "capi_internal.h"

using namespace oamd;

// who: the entry point family of the message ("solve", "replay")
static int bytes_check(const int64_t* bytes, const char* who) {
    if (!bytes) return fail(OAMD_INVALID_ARGUMENT, std::string(who) + ": bytes is NULL");
    return OAMD_OK;
}

// positions of one solver call (move_scores indices stay below 2^31)
static int solve_n_check(int64_t n) {
    if (n < 0 || n > INT32_MAX / 65)
        return fail(OAMD_INVALID_ARGUMENT, "Expected 0 <= n <= " + std::to_string(INT32_MAX / 65) + ", but got " +
                                               std::to_string(n) + ".");
    return OAMD_OK;
}

extern "C" {

// ---------------------------------------------------------------------------
// Packed replay buffer (replay.hip): the caller owns the storage
// ---------------------------------------------------------------------------
static int replay_checks(const oamd_replay_view* v) {
    if (!v) return fail(OAMD_INVALID_ARGUMENT, "replay: view is NULL");
    if (!has_device(v->device))
        return fail(OAMD_INVALID_ARGUMENT, "replay: no HIP device " + std::to_string(v->device));
    if (v->num_games < 1)
        return fail(OAMD_INVALID_ARGUMENT, "Expected num_games >= 1, but got " + std::to_string(v->num_games) + ".");
    if (v->history_size < 1 || v->history_size > 15)
        return fail(OAMD_INVALID_ARGUMENT,
                    "Expected 1 <= history_size <= 15, but got " + std::to_string(v->history_size) + ".");
    if (v->max_moves < 1)
        return fail(OAMD_INVALID_ARGUMENT, "Expected max_moves >= 1, but got " + std::to_string(v->max_moves) + ".");
    if ((int64_t)v->num_games * v->max_moves > INT32_MAX)
        return fail(OAMD_INVALID_ARGUMENT, "replay: num_games * max_moves must be below 2^31");
    if (v->capacity < 1)
        return fail(OAMD_INVALID_ARGUMENT, "Expected capacity >= 1, but got " + std::to_string(v->capacity) + ".");
    if (!v->boards || !v->policy || !v->value || !v->player || !v->stage_boards || !v->stage_policy ||
        !v->stage_player || !v->moves || !v->pending || !v->counters)
        return fail(OAMD_INVALID_ARGUMENT, "replay: every buffer of the view is required");
    return OAMD_OK;
}

// exact_dev: the ring's exact bytes, or nullptr for a buffer that keeps none
static int replay_add(const oamd_replay_view* view, int8_t* exact_dev, int32_t n_moves, const int32_t* actions_dev,
                      const int32_t* finished_dev, const float* features_dev, const float* policy_dev,
                      void* stream) {
    if (int rc = replay_checks(view)) return rc;
    if (n_moves < 0) return fail(OAMD_INVALID_ARGUMENT, "replay: n_moves must be >= 0");
    if (n_moves == 0) return OAMD_OK;
    if (!actions_dev || !finished_dev)
        return fail(OAMD_INVALID_ARGUMENT, "replay: actions and finished buffers are required");
    if (!features_dev || !policy_dev)
        return fail(OAMD_INVALID_ARGUMENT,
                    "replay: features and policy buffers are required (self-play moves with emit_targets = 1)");
    DeviceGuard dg(view->device);
    const size_t G = (size_t)view->num_games;
    const size_t C = 1 + 2 * (size_t)view->history_size;
    for (int32_t i = 0; i < n_moves; ++i) {
        launch_replay_add(*view, exact_dev, actions_dev + i * G, finished_dev + i * G,
                          features_dev + i * G * 8 * C * 64, policy_dev + i * G * 8 * 65, (hipStream_t)stream);
        LAUNCHCHK();
    }
    return OAMD_OK;
}

int oamd_replay_add(const oamd_replay_view* view, int32_t n_moves, const int32_t* actions_dev,
                    const int32_t* finished_dev, const float* features_dev, const float* policy_dev, void* stream) {
    return replay_add(view, nullptr, n_moves, actions_dev, finished_dev, features_dev, policy_dev, stream);
}

int oamd_replay_add_tracked(const oamd_replay_view* view, int8_t* exact_dev, int32_t n_moves,
                            const int32_t* actions_dev, const int32_t* finished_dev, const float* features_dev,
                            const float* policy_dev, void* stream) {
    if (!exact_dev) return fail(OAMD_INVALID_ARGUMENT, "replay: the exact buffer is required");
    return replay_add(view, exact_dev, n_moves, actions_dev, finished_dev, features_dev, policy_dev, stream);
}

int oamd_replay_gather(const oamd_replay_view* view, const int64_t* ids_dev, int64_t n, float* features_dev,
                       float* policy_dev, float* value_dev, void* stream) {
    if (int rc = replay_checks(view)) return rc;
    if (n < 0 || n > INT32_MAX) return fail(OAMD_INVALID_ARGUMENT, "replay: n must be in [0, 2^31)");
    if (n == 0) return OAMD_OK;
    if (!ids_dev) return fail(OAMD_INVALID_ARGUMENT, "replay: ids buffer is required");
    if (!features_dev || !policy_dev || !value_dev)
        return fail(OAMD_INVALID_ARGUMENT, "replay: features, policy and value output buffers are required");
    DeviceGuard dg(view->device);
    launch_replay_gather(*view, ids_dev, n, features_dev, policy_dev, value_dev, (hipStream_t)stream);
    LAUNCHCHK();
    return OAMD_OK;
}

int oamd_replay_counters(const oamd_replay_view* view, int64_t* size, int64_t* head, int64_t* games_completed,
                         int32_t* flags, void* stream) {
    if (int rc = replay_checks(view)) return rc;
    DeviceGuard dg(view->device);
    int64_t c[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(c, view->counters, sizeof(c), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    if (head) *head = c[kReplayHead];
    if (size) *size = c[kReplaySize];
    if (games_completed) *games_completed = c[kReplayGames];
    if (flags) *flags = (int32_t)c[kReplayFlags];
    return OAMD_OK;
}

// ---------------------------------------------------------------------------
// Exact endgame solver (solver.h, solver.hip): the caller owns every buffer
// ---------------------------------------------------------------------------
static int solve_limit_checks(int32_t max_empties, int64_t node_limit) {
    if (max_empties < 0 || max_empties > kSolveMaxEmpties)
        return fail(OAMD_INVALID_ARGUMENT, "Expected 0 <= max_empties <= " + std::to_string(kSolveMaxEmpties) +
                                               ", but got " + std::to_string(max_empties) + ".");
    if (node_limit < 1 || node_limit >= (1LL << kSolveStatusShift))
        return fail(OAMD_INVALID_ARGUMENT,
                    "Expected 1 <= node_limit < 2^56, but got " + std::to_string(node_limit) + ".");
    return OAMD_OK;
}

int oamd_solve_workspace_bytes(int64_t n, int64_t* bytes) {
    if (int rc = bytes_check(bytes, "solve")) return rc;
    if (int rc = solve_n_check(n)) return rc;
    *bytes = solve_workspace_bytes(n);
    return OAMD_OK;
}

static int solve_endgames(int32_t device, const oamd_position* pos_dev, int64_t n, int32_t max_empties,
                          int64_t node_limit, int32_t* move_scores_dev, int32_t* score_dev, int32_t* best_action_dev,
                          int32_t* flags_dev, int64_t* nodes_dev, void* workspace_dev, int32_t workgroups,
                          void* stream, bool split = false) {
    static_assert(sizeof(oamd_position) == 40, "layout");
    if (int rc = solve_limit_checks(max_empties, node_limit)) return rc;
    if (int rc = solve_n_check(n)) return rc;
    if (!has_device(device)) return fail(OAMD_INVALID_ARGUMENT, "solve: no HIP device " + std::to_string(device));
    if (n == 0) return OAMD_OK;
    if (!pos_dev || !move_scores_dev || !workspace_dev)
        return fail(OAMD_INVALID_ARGUMENT, "solve: positions, move_scores and workspace buffers are required");
    DeviceGuard dg(device);
    int cus = 0;
    if (int rc = device_cus(device, &cus)) return rc;
    (split ? launch_solve_split : launch_solve)(pos_dev, n, max_empties, node_limit, move_scores_dev, score_dev,
                                                best_action_dev, flags_dev, nodes_dev, workspace_dev, workgroups,
                                                cus, (hipStream_t)stream);
    LAUNCHCHK();
    return OAMD_OK;
}

int oamd_solve_endgames(int32_t device, const oamd_position* pos_dev, int64_t n, int32_t max_empties,
                        int64_t node_limit, int32_t* move_scores_dev, int32_t* score_dev, int32_t* best_action_dev,
                        int32_t* flags_dev, int64_t* nodes_dev, void* workspace_dev, void* stream) {
    return solve_endgames(device, pos_dev, n, max_empties, node_limit, move_scores_dev, score_dev, best_action_dev,
                          flags_dev, nodes_dev, workspace_dev, 0, stream);
}

int oamd_solve_endgames_grid(int32_t device, const oamd_position* pos_dev, int64_t n, int32_t max_empties,
                             int64_t node_limit, int32_t* move_scores_dev, int32_t* score_dev,
                             int32_t* best_action_dev, int32_t* flags_dev, int64_t* nodes_dev, void* workspace_dev,
                             int32_t workgroups, void* stream) {
    if (workgroups < 1)
        return fail(OAMD_INVALID_ARGUMENT, "Expected workgroups >= 1, but got " + std::to_string(workgroups) + ".");
    return solve_endgames(device, pos_dev, n, max_empties, node_limit, move_scores_dev, score_dev, best_action_dev,
                          flags_dev, nodes_dev, workspace_dev, workgroups, stream);
}

int oamd_host_solve_endgame(const oamd_position* pos_host, int32_t max_empties, int64_t node_limit,
                            int32_t* move_scores65, int32_t* score, int32_t* best_action, int32_t* flags,
                            int64_t* nodes) {
    if (int rc = solve_limit_checks(max_empties, node_limit)) return rc;
    if (!pos_host || !move_scores65) return fail(OAMD_INVALID_ARGUMENT, "solve: position and move_scores are required");
    solve_host(pos_host->player, pos_host->player1_discs, pos_host->player2_discs, max_empties, node_limit,
               move_scores65, score, best_action, flags, nodes);
    return OAMD_OK;
}

// The split solver: the same checks and outputs, its own workspace.
int oamd_solve_split_workspace_bytes(int64_t n, int64_t* bytes) {
    if (int rc = bytes_check(bytes, "solve")) return rc;
    if (int rc = solve_n_check(n)) return rc;
    *bytes = solve_split_workspace_bytes(n);
    return OAMD_OK;
}

int oamd_solve_endgames_split(int32_t device, const oamd_position* pos_dev, int64_t n, int32_t max_empties,
                              int64_t node_limit, int32_t* move_scores_dev, int32_t* score_dev,
                              int32_t* best_action_dev, int32_t* flags_dev, int64_t* nodes_dev, void* workspace_dev,
                              void* stream) {
    return solve_endgames(device, pos_dev, n, max_empties, node_limit, move_scores_dev, score_dev, best_action_dev,
                          flags_dev, nodes_dev, workspace_dev, 0, stream, true);
}

int oamd_solve_endgames_split_grid(int32_t device, const oamd_position* pos_dev, int64_t n, int32_t max_empties,
                                   int64_t node_limit, int32_t* move_scores_dev, int32_t* score_dev,
                                   int32_t* best_action_dev, int32_t* flags_dev, int64_t* nodes_dev,
                                   void* workspace_dev, int32_t workgroups, void* stream) {
    if (workgroups < 1)
        return fail(OAMD_INVALID_ARGUMENT, "Expected workgroups >= 1, but got " + std::to_string(workgroups) + ".");
    return solve_endgames(device, pos_dev, n, max_empties, node_limit, move_scores_dev, score_dev, best_action_dev,
                          flags_dev, nodes_dev, workspace_dev, workgroups, stream, true);
}

int oamd_host_solve_endgame_split(const oamd_position* pos_host, int32_t max_empties, int64_t node_limit,
                                  int32_t* move_scores65, int32_t* score, int32_t* best_action, int32_t* flags,
                                  int64_t* nodes) {
    if (int rc = solve_limit_checks(max_empties, node_limit)) return rc;
    if (!pos_host || !move_scores65) return fail(OAMD_INVALID_ARGUMENT, "solve: position and move_scores are required");
    solve_host_split(pos_host->player, pos_host->player1_discs, pos_host->player2_discs, max_empties, node_limit,
                     move_scores65, score, best_action, flags, nodes);
    return OAMD_OK;
}

// ---------------------------------------------------------------------------
// Baseline opponents (baseline.h, baseline.hip): the caller owns every buffer
// ---------------------------------------------------------------------------
static int baseline_checks(int32_t kind, int32_t depth, int64_t node_limit) {
    if (kind < OAMD_BASELINE_RANDOM || kind > OAMD_BASELINE_SEARCH)
        return fail(OAMD_INVALID_ARGUMENT, "Expected a baseline kind in 0..2, but got " + std::to_string(kind) + ".");
    if (kind == OAMD_BASELINE_SEARCH && (depth < 1 || depth > kBaselineMaxDepth))
        return fail(OAMD_INVALID_ARGUMENT, "Expected 1 <= depth <= " + std::to_string(kBaselineMaxDepth) +
                                               ", but got " + std::to_string(depth) + ".");
    if (node_limit < 1 || node_limit >= (1LL << kSolveStatusShift))
        return fail(OAMD_INVALID_ARGUMENT,
                    "Expected 1 <= node_limit < 2^56, but got " + std::to_string(node_limit) + ".");
    return OAMD_OK;
}

int oamd_baseline_workspace_bytes(int64_t n, int64_t* bytes) {
    if (int rc = bytes_check(bytes, "baseline")) return rc;
    if (int rc = solve_n_check(n)) return rc;
    *bytes = baseline_workspace_bytes(n);
    return OAMD_OK;
}

int oamd_baseline_moves(int32_t device, const oamd_position* pos_dev, int64_t n, int32_t kind, int32_t depth,
                        int64_t node_limit, const int64_t* keys_dev, const int64_t* events_dev,
                        int32_t* move_scores_dev, int32_t* score_dev, int32_t* action_dev, int32_t* flags_dev,
                        int64_t* nodes_dev, void* workspace_dev, int32_t workgroups, void* stream) {
    if (int rc = baseline_checks(kind, depth, node_limit)) return rc;
    if (int rc = solve_n_check(n)) return rc;
    if (workgroups < 0)
        return fail(OAMD_INVALID_ARGUMENT, "Expected workgroups >= 0, but got " + std::to_string(workgroups) + ".");
    if (!move_scores_dev || !score_dev || !action_dev || !flags_dev || !nodes_dev)
        return fail(OAMD_INVALID_ARGUMENT,
                    "baseline: move_scores, score, action, flags and nodes output buffers are required");
    if (!has_device(device)) return fail(OAMD_INVALID_ARGUMENT, "baseline: no HIP device " + std::to_string(device));
    if (n == 0) return OAMD_OK;
    if (!pos_dev || !workspace_dev)
        return fail(OAMD_INVALID_ARGUMENT, "baseline: positions and workspace buffers are required");
    DeviceGuard dg(device);
    int cus = 0;
    if (int rc = device_cus(device, &cus)) return rc;
    launch_baseline(pos_dev, n, kind, depth, node_limit, keys_dev, events_dev, move_scores_dev, score_dev, action_dev,
                    flags_dev, nodes_dev, workspace_dev, workgroups, cus, (hipStream_t)stream);
    LAUNCHCHK();
    return OAMD_OK;
}

int oamd_host_baseline_move(const oamd_position* pos_host, int32_t kind, int32_t depth, int64_t node_limit,
                            int32_t has_key, uint64_t key, uint64_t event, int32_t* move_scores65, int32_t* score,
                            int32_t* action, int32_t* flags, int64_t* nodes) {
    if (int rc = baseline_checks(kind, depth, node_limit)) return rc;
    if (!pos_host || !move_scores65 || !score || !action || !flags || !nodes)
        return fail(OAMD_INVALID_ARGUMENT, "baseline: the position and every output are required");
    baseline_host(pos_host->player, pos_host->player1_discs, pos_host->player2_discs, kind, depth, node_limit,
                  has_key != 0, key, event, move_scores65, score, action, flags, nodes);
    return OAMD_OK;
}

// ---------------------------------------------------------------------------
// Exact endgame value targets of the packed replay buffer (replay.hip + solver.hip)
// ---------------------------------------------------------------------------
constexpr int64_t kRelabelMaxBudget = 1 << 20;

static int relabel_budget_check(int64_t budget) {
    if (budget < 1 || budget > kRelabelMaxBudget)
        return fail(OAMD_INVALID_ARGUMENT, "Expected 1 <= budget <= " + std::to_string(kRelabelMaxBudget) +
                                               ", but got " + std::to_string(budget) + ".");
    return OAMD_OK;
}

int oamd_replay_relabel_workspace_bytes(int64_t budget, int64_t* bytes) {
    if (int rc = bytes_check(bytes, "replay")) return rc;
    if (int rc = relabel_budget_check(budget)) return rc;
    *bytes = relabel_workspace_bytes(budget);
    return OAMD_OK;
}

int oamd_replay_relabel_split_workspace_bytes(int64_t budget, int64_t* bytes) {
    if (int rc = bytes_check(bytes, "replay")) return rc;
    if (int rc = relabel_budget_check(budget)) return rc;
    *bytes = relabel_workspace_bytes(budget, true);
    return OAMD_OK;
}

static int replay_relabel(const oamd_replay_view* view, int8_t* exact_dev, int64_t* relabel_counters_dev,
                          int32_t max_empties, int64_t budget, int64_t node_limit, int32_t policy_mode, int32_t retry,
                          void* workspace_dev, void* stream, bool split) {
    if (int rc = solve_limit_checks(max_empties, node_limit)) return rc;
    if (int rc = relabel_budget_check(budget)) return rc;
    if (policy_mode != OAMD_REPLAY_POLICY_KEEP && policy_mode != OAMD_REPLAY_POLICY_OPTIMAL)
        return fail(OAMD_INVALID_ARGUMENT,
                    "Expected policy_mode 0 (keep) or 1 (optimal), but got " + std::to_string(policy_mode) + ".");
    if (int rc = replay_checks(view)) return rc;
    if (view->capacity > INT32_MAX)
        return fail(OAMD_INVALID_ARGUMENT, "replay: relabelling needs capacity < 2^31");
    if (!exact_dev || !relabel_counters_dev || !workspace_dev)
        return fail(OAMD_INVALID_ARGUMENT, "replay: exact, relabel_counters and workspace buffers are required");
    DeviceGuard dg(view->device);
    int cus = 0;
    if (int rc = device_cus(view->device, &cus)) return rc;
    launch_replay_relabel(*view, exact_dev, relabel_counters_dev, max_empties, budget, node_limit, policy_mode,
                          retry != 0, workspace_dev, cus, (hipStream_t)stream, split);
    LAUNCHCHK();
    return OAMD_OK;
}

int oamd_replay_relabel_endgames(const oamd_replay_view* view, int8_t* exact_dev, int64_t* relabel_counters_dev,
                                 int32_t max_empties, int64_t budget, int64_t node_limit, int32_t policy_mode,
                                 int32_t retry, void* workspace_dev, void* stream) {
    return replay_relabel(view, exact_dev, relabel_counters_dev, max_empties, budget, node_limit, policy_mode, retry,
                          workspace_dev, stream, false);
}

int oamd_replay_relabel_endgames_split(const oamd_replay_view* view, int8_t* exact_dev, int64_t* relabel_counters_dev,
                                       int32_t max_empties, int64_t budget, int64_t node_limit, int32_t policy_mode,
                                       int32_t retry, void* workspace_dev, void* stream) {
    return replay_relabel(view, exact_dev, relabel_counters_dev, max_empties, budget, node_limit, policy_mode, retry,
                          workspace_dev, stream, true);
}

}  // extern "C"
