// C ABI (include/othello_mcts_amd.h): the error message, engine lifetime and
// configuration with the reference's exception messages, the step API, the
// queries, and every native search schedule. The net is in capi_net.hip, the
// self-play move, adjudication and the arena in capi_play.hip, the replay ring
// and the endgame solver in capi_data.hip. All compute is in tree.hip, selfplay.hip, arena.hip /
// resnet.hip.

#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>

#include "capi_internal.h"
#include "exact_leaf.h"
#include "forced.h"
#include "positions.h"
#include "rng.h"

using namespace oamd;

namespace {
thread_local std::string g_err;
}

int oamd::fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

namespace {
std::string fstr(float v) { return std::to_string(v); }

// mcts.cpp:167-241 (messages verbatim) + the native engine's own limits
int validate_config(const oamd_search_config* c) {
    if (c->history_size < 1)
        return fail(OAMD_INVALID_ARGUMENT,
                    "Expected history_size >= 1, but got " + std::to_string(c->history_size) + ".");
    if (c->history_size > kMaxHistory)
        return fail(OAMD_INVALID_ARGUMENT, "Expected history_size <= 15 (native engine limit), but got " +
                                               std::to_string(c->history_size) + ".");
    if (c->num_simulations < 1)
        return fail(OAMD_INVALID_ARGUMENT, "Expected num_simulations >= 1, but got " +
                                               std::to_string(c->num_simulations) + ".");
    if (c->num_threads < 1)
        return fail(OAMD_INVALID_ARGUMENT,
                    "Expected num_threads >= 1, but got " + std::to_string(c->num_threads) + ".");
    if (c->batch_size < 1)
        return fail(OAMD_INVALID_ARGUMENT,
                    "Expected batch_size >= 1, but got " + std::to_string(c->batch_size) + ".");
    if ((int64_t)c->num_threads * c->batch_size > kMaxLeaves)
        return fail(OAMD_INVALID_ARGUMENT,
                    "Expected num_threads * batch_size <= 1024 (native engine limit), but got " +
                        std::to_string((int64_t)c->num_threads * c->batch_size) + ".");
    if (!(c->c_puct_base > 0.0f))
        return fail(OAMD_INVALID_ARGUMENT, "Expected c_puct_base > 0.0, but got " + fstr(c->c_puct_base) + ".");
    if (!(c->c_puct_init >= 0.0f))
        return fail(OAMD_INVALID_ARGUMENT, "Expected c_puct_init >= 0.0, but got " + fstr(c->c_puct_init) + ".");
    if (!(0.0f <= c->dirichlet_epsilon && c->dirichlet_epsilon <= 1.0f))
        return fail(OAMD_INVALID_ARGUMENT, "Expected 0.0 <= dirichlet_epsilon <= 1.0, but got " +
                                               fstr(c->dirichlet_epsilon) + ".");
    if (!(c->dirichlet_alpha >= 0.0f))
        return fail(OAMD_INVALID_ARGUMENT,
                    "Expected dirichlet_alpha >= 0.0, but got " + fstr(c->dirichlet_alpha) + ".");
    return OAMD_OK;
}

// exploration_rate table with the HOST's logf (bit-identical to the
// reference's std::log(float), search_thread.cpp:198-203), into a buffer of
// its own: the caller swaps it in once everything else succeeded
int build_tables(const oamd_search_config& cfg, DeviceBuf<float>* tab) {
    std::vector<float> ex(kExploreTab);
    for (int n = 0; n < kExploreTab; ++n)
        ex[n] = std::log(((float)(1 + n) + cfg.c_puct_base) / cfg.c_puct_base) + cfg.c_puct_init;
    if (int rc = tab->alloc(kExploreTab)) return rc;
    HIPCHK(hipMemcpy(tab->get(), ex.data(), ex.size() * sizeof(float), hipMemcpyHostToDevice));
    return OAMD_OK;
}

}  // namespace

extern "C" {

const char* oamd_last_error(void) { return g_err.c_str(); }

int oamd_device_count(int32_t* out) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *out = n;
    return OAMD_OK;
}

// ---------------------------------------------------------------- bitboards
int oamd_get_legal_moves(const uint64_t* me, const uint64_t* opp, uint64_t* out, int64_t n, void* stream) {
    if (n < 0) return fail(OAMD_INVALID_ARGUMENT, "n must be >= 0");
    launch_legal_moves(me, opp, out, n, (hipStream_t)stream);
    LAUNCHCHK();
    return OAMD_OK;
}

int oamd_get_flips(const uint64_t* mv, const uint64_t* me, const uint64_t* opp, uint64_t* out, int64_t n,
                   void* stream) {
    if (n < 0) return fail(OAMD_INVALID_ARGUMENT, "n must be >= 0");
    launch_flips(mv, me, opp, out, n, (hipStream_t)stream);
    LAUNCHCHK();
    return OAMD_OK;
}

int oamd_apply_action(const oamd_position* in, const int32_t* actions, oamd_position* out, int64_t n,
                      void* stream) {
    static_assert(sizeof(oamd_position) == sizeof(Pos), "layout");
    if (n < 0) return fail(OAMD_INVALID_ARGUMENT, "n must be >= 0");
    launch_apply_positions(reinterpret_cast<const Pos*>(in), actions, reinterpret_cast<Pos*>(out), n,
                           (hipStream_t)stream);
    LAUNCHCHK();
    return OAMD_OK;
}

int oamd_initial_position(oamd_position* out) {
    const Pos p = initial_position();
    std::memcpy(out, &p, sizeof(Pos));
    return OAMD_OK;
}

uint64_t oamd_host_legal_moves(uint64_t me, uint64_t opp) { return legal_moves(me, opp); }
uint64_t oamd_host_flips(uint64_t mv, uint64_t me, uint64_t opp) { return flips(mv, me, opp); }
void oamd_host_apply_action(const oamd_position* in, int32_t action, oamd_position* out) {
    Pos p;
    std::memcpy(&p, in, sizeof(Pos));
    const Pos c = apply_action(p, action);
    std::memcpy(out, &c, sizeof(Pos));
}

// ---------------------------------------------------------------- engine
int oamd_engine_create(int32_t device, int32_t num_games, int64_t node_capacity, const oamd_search_config* cfg,
                       uint64_t seed, oamd_engine** out) {
    *out = nullptr;
    int rc = validate_config(cfg);
    if (rc) return rc;
    if (num_games < 1) return fail(OAMD_INVALID_ARGUMENT, "num_games must be >= 1");
    if (node_capacity == 0) node_capacity = (int64_t)1 << 20;
    if (node_capacity < 128 || node_capacity > ((int64_t)1 << 30))
        return fail(OAMD_INVALID_ARGUMENT, "node_capacity must be in [128, 2^30]");
    if ((int64_t)num_games * node_capacity > ((int64_t)1 << 36))
        return fail(OAMD_INVALID_ARGUMENT, "num_games * node_capacity too large");
    if ((rc = create_device_checks(device))) return rc;
    DeviceGuard dg(device);  // also around the engine's release on a failure below
    std::unique_ptr<oamd_engine> e(new oamd_engine());
    e->device = device;
    e->G = num_games;
    e->cap = node_capacity;
    e->cfg = *cfg;
    e->seed = seed;
    const size_t nodes = (size_t)num_games * node_capacity;
    if ((rc = e->link.alloc(nodes)) || (rc = e->stat.alloc(nodes)) || (rc = e->pos.alloc(nodes)) ||
        (rc = e->games.alloc(num_games)) || (rc = e->counters.alloc(kCounters)) ||
        (rc = e->rowcount.alloc(2 * kMaxPipeline)) || (rc = e->status_dev.alloc(2)) ||
        (rc = e->info_dev.alloc(num_games)) || (rc = e->visits_dev.alloc((size_t)num_games * 65)) ||
        (rc = e->q_dev.alloc((size_t)num_games * 65)) ||
        (rc = e->spd_dev.alloc((size_t)8 * (1 + 2 * kMaxHistory) * 64 + 8 * 65)) ||
        (rc = e->rows.ensure((int64_t)num_games * e->L(), e->FW(), kMaxDepth)) ||
        (rc = build_tables(e->cfg, &e->explore_tab)))
        return rc;
    if (hipMemset(e->counters.get(), 0, kCounters * sizeof(unsigned long long)) != hipSuccess ||
        hipMemset(e->rowcount.get(), 0, 2 * kMaxPipeline * sizeof(int32_t)) != hipSuccess)
        return fail(OAMD_RUNTIME, "engine init: counter memset failed");
    launch_reset(e->view(), -1, seed, nullptr);
    hipError_t le = hipGetLastError();
    if (le != hipSuccess || hipDeviceSynchronize() != hipSuccess)
        return fail(OAMD_RUNTIME, std::string("engine init: ") + hipGetErrorString(le));
    *out = e.release();
    return OAMD_OK;
}

int oamd_engine_destroy(oamd_engine* e) {
    if (!e) return OAMD_OK;
    DeviceGuard dg(e->device);
    delete e;
    return OAMD_OK;
}

// All or nothing: the new per-row set and table are built beside the old ones
// and swapped in with the config only when both succeeded; a failure leaves
// the engine as it was.
int oamd_engine_set_config(oamd_engine* e, const oamd_search_config* cfg) {
    int rc = validate_config(cfg);
    if (rc) return rc;
    if (const char* why = e->playout_cap_conflict(*cfg))
        return fail(OAMD_INVALID_ARGUMENT, std::string(why) + " (oamd_engine_set_playout_cap(e, NULL) switches it off)");
    DeviceGuard dg(e->device);
    const bool tabs = cfg->c_puct_base != e->cfg.c_puct_base || cfg->c_puct_init != e->cfg.c_puct_init;
    HIPCHK(hipStreamSynchronize(e->stream));
    const int64_t rows = (int64_t)e->G * cfg->num_threads * cfg->batch_size;
    const int fw = feature_words(cfg->history_size);
    const bool grow = !e->rows.fits(rows, fw);
    RowBuffers grown;
    DeviceBuf<float> tab;
    if (grow && (rc = grown.ensure(rows, fw, kMaxDepth))) return rc;
    if (tabs && (rc = build_tables(*cfg, &tab))) return rc;
    if (grow) e->rows = std::move(grown);
    if (tabs) e->explore_tab = std::move(tab);
    e->cfg = *cfg;
    e->end_search();
    return OAMD_OK;
}

int oamd_engine_get_config(const oamd_engine* e, oamd_search_config* cfg) {
    *cfg = e->cfg;
    return OAMD_OK;
}

int oamd_engine_num_games(const oamd_engine* e, int32_t* out) {
    *out = e->G;
    return OAMD_OK;
}

int oamd_engine_set_stream(oamd_engine* e, void* stream) {
    e->stream = (hipStream_t)stream;
    return OAMD_OK;
}

int oamd_engine_reset(oamd_engine* e, int32_t game, uint64_t seed) {
    if (game < -1 || game >= e->G) return fail(OAMD_OUT_OF_RANGE, "game index out of range");
    DeviceGuard dg(e->device);
    launch_reset(e->view(), game, seed, e->stream);
    LAUNCHCHK();
    e->end_search();
    if (game < 0) e->exact_trees = false;  // no tree left: the exact-leaf setting may change again
    return OAMD_OK;
}

int oamd_engine_search_begin(oamd_engine* e, int32_t* steps) {
    e->steps_left = e->steps();
    e->steps_total = e->steps_left;
    e->step_phase = 0;
    if (steps) *steps = e->steps_left;
    return OAMD_OK;
}

int oamd_engine_select(oamd_engine* e) {
    if (e->steps_left <= 0)
        return fail(OAMD_INVALID_ARGUMENT, "select called out of order (search_begin first)");
    DeviceGuard dg(e->device);
    // a pending round is backed up thread by thread, each thread selecting its
    // next batch right after its backup (the reference's interleaving, k_tree)
    launch_tree(e->view(), e->stream, e->step_phase == 1, true, e->cfg.num_threads, e->cfg.batch_size, 0, -1, 0, -1,
                nullptr, nullptr, e->steps_left == e->steps_total);
    // exact leaves: the round's pending leaves are solved before its backup
    launch_solve_leaves(e->view(), 0, e->G * e->L(), e->stream);
    LAUNCHCHK();
    e->exact_trees = true;
    e->step_phase = 1;
    e->steps_left -= 1;
    return OAMD_OK;
}

int oamd_engine_leaf_flags(oamd_engine* e, uint8_t* host_out) {
    DeviceGuard dg(e->device);
    launch_leaf_flags(e->view(), e->rows.flags.get(), e->stream);
    LAUNCHCHK();
    HIPCHK(hipMemcpyAsync(host_out, e->rows.flags.get(), (size_t)e->G * e->L(), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return OAMD_OK;
}

int oamd_engine_features(oamd_engine* e, float* out, int32_t row_begin, int32_t rows) {
    if (row_begin < 0 || rows < 0 || (int64_t)row_begin + rows > (int64_t)e->G * e->L())
        return fail(OAMD_OUT_OF_RANGE, "row range out of range");
    DeviceGuard dg(e->device);
    launch_features_f32(e->view(), out, row_begin, rows, e->stream);
    LAUNCHCHK();
    return OAMD_OK;
}

int oamd_engine_set_evaluation(oamd_engine* e, const float* pol, const float* val, int32_t row_begin,
                               int32_t rows) {
    if (row_begin < 0 || rows < 0 || (int64_t)row_begin + rows > (int64_t)e->G * e->L())
        return fail(OAMD_OUT_OF_RANGE, "row range out of range");
    DeviceGuard dg(e->device);
    launch_set_evaluation(e->view(), pol, val, row_begin, rows, e->stream);
    LAUNCHCHK();
    return OAMD_OK;
}

int oamd_engine_backup(oamd_engine* e) {
    if (e->step_phase != 1) return fail(OAMD_INVALID_ARGUMENT, "backup called before select");
    DeviceGuard dg(e->device);
    launch_tree(e->view(), e->stream, true, false, e->cfg.num_threads, e->cfg.batch_size);
    LAUNCHCHK();
    e->step_phase = 0;
    return OAMD_OK;
}

int oamd_engine_enable_timing(oamd_engine* e, int32_t enable) {
    if (enable < 0) return fail(OAMD_INVALID_ARGUMENT, "enable_timing: expected >= 0");
    DeviceGuard dg(e->device);
    if (int rc = e->spans.reset()) return rc;
    e->timing = enable != 0;
    e->timing_stride = enable > 1 ? enable : 1;
    e->search_count = 0;
    return OAMD_OK;
}

int oamd_engine_nn_timing(const oamd_engine* ce, float* nn_ms, int64_t* launches, int64_t* rows) {
    oamd_engine* e = const_cast<oamd_engine*>(ce);  // pending events are summed here
    if (int rc = e->resolve_all_timing()) return rc;
    if (nn_ms) *nn_ms = e->nn_ms;
    if (launches) *launches = e->nn_launches;
    if (rows) *rows = e->nn_rows;
    return OAMD_OK;
}

int oamd_engine_nn_busy(const oamd_engine* ce, float* busy_ms, int64_t* launches) {
    oamd_engine* e = const_cast<oamd_engine*>(ce);
    DeviceGuard dg(e->device);
    if (e->spans.dropped)
        return fail(OAMD_RUNTIME, "nn_busy: the timing window outgrew its " + std::to_string(SpanWindow::kWindow) +
                                      " slots; " + std::to_string(e->spans.dropped) +
                                      " launches were not recorded (restart it with oamd_engine_enable_timing)");
    std::vector<std::pair<long long, long long>> iv;
    if (int rc = e->spans.intervals(&iv)) return rc;
    // 100 MHz ticks -> ms, once for the whole union
    if (busy_ms) *busy_ms = (float)(interval_union(iv) * 1e-5);
    // the launches that ran (a search reserves slots for the most launches of
    // any group per round; groups of unequal size may leave some unused)
    if (launches) *launches = (int64_t)iv.size();
    return OAMD_OK;
}

int oamd_engine_tree_timing(const oamd_engine* ce, float* select_ms, float* backup_ms, int64_t* launches) {
    oamd_engine* e = const_cast<oamd_engine*>(ce);
    if (int rc = e->resolve_all_timing()) return rc;
    if (select_ms) *select_ms = e->select_ms;
    if (backup_ms) *backup_ms = e->backup_ms;
    if (launches) *launches = e->tree_launches;
    return OAMD_OK;
}

static GroupPlan plan_groups(oamd_engine* e) {
    GroupPlan P;
    static_cast<GroupSplit&>(P) = split_groups(e->G, e->pipeline);
    for (int k = 0; k < P.K; ++k) {
        P.st[k] = P.K == 1 ? e->stream : e->pipe.stream[k].get();
        const int n = group_launches(P.ng[k], e->L(), e->nn_batch);
        P.max_launches = std::max(P.max_launches, n);
        P.round_launches += n;
        P.round_rows += (int64_t)P.ng[k] * e->L();
    }
    return P;
}

// The most extra rounds of a native grouped search (chain splitting, k_tree)
static int extra_rounds(const oamd_engine* e) {
    return extra_round_cap(e->exact_interleaving, e->chain_budget, e->chain_cuts, e->cfg.num_threads, e->steps());
}

// Extra rounds X of the next grouped search. Fixed: chain_cuts. Adaptive: a
// game cut c times finishes by round steps + c, so the extra rounds past the
// most cuts any game used are empty launches, while a game that would need
// more than X cuts runs its last chain uncut (same results, but a round of up
// to ~10 ms that holds its group's NN launch). X follows the search two back
// (done by now: the previous one is still queued, so the read-back does not
// drain the queue): its most cuts and the fewest empty squares of its roots.
static int pick_extra_rounds(oamd_engine* e, int* X) {
    const int cap = extra_rounds(e);
    *X = cap;
    if (cap == 0 || !e->adapt.on) return OAMD_OK;
    if (int rc = e->cuts.ensure((size_t)2 * oamd_engine::kCutSlots * kMaxPipeline,
                                (size_t)2 * oamd_engine::kCutSlots * kMaxPipeline, readback_event_flags(), "cut slots"))
        return rc;
    const int64_t q = e->adapt_seq - 2;
    const int s = q >= 0 ? (int)(q % oamd_engine::kCutSlots) : 0;
    if (q >= 0 && e->cut_x[s] >= 0) {
        int used = 0, empties = 64;
        for (int k = 0; k < e->cut_groups[s]; ++k) {
            HIPCHK(host_wait(e->cuts.ev[s][k].get()));
            used = std::max(used, (int)e->cuts.host.get()[2 * (s * kMaxPipeline + k)]);
            empties = std::min(empties, (int)e->cuts.host.get()[2 * (s * kMaxPipeline + k) + 1]);
        }
        e->adapt.observe(e->cut_x[s], used, empties, e->chain_cuts);
        static const bool plog = getenv("OAMD_ADAPT_LOG") != nullptr;
        if (plog)
            fprintf(stderr, "adapt search %lld X %d used %d empties %d\n", (long long)q, e->cut_x[s], used, empties);
        e->cut_x[s] = -1;
    }
    *X = e->adapt.pick(cap);
    return OAMD_OK;
}

// Sampled timing of one search: claim the current event pool (every
// timing_stride-th search), sized for NB blocks per round and `steps` NN
// rounds (steps + extra rounds) plus the final backup-only round.
static int timing_begin(oamd_engine* e, int steps, int NB, bool* timed) {
    *timed = e->timing && (e->search_count++ % e->timing_stride) == 0;
    if (!*timed) return OAMD_OK;
    const int pool = e->ev_cur;
    if (int rc = e->resolve_timing(pool)) return rc;
    return e->pools.ensure(pool, (size_t)kEvPerBlock * (steps + 1) * NB);
}

// Hand the claimed pool's recorded blocks over: `blocks` of them, NB per
// round; those from first_final on (a search's backup-only final round; none
// in a free-running chunk) carry no NN events, every round before has
// round_launches ResNet launches of round_rows rows in all.
static void timing_end(oamd_engine* e, int blocks, int first_final, int NB, int64_t round_launches,
                       int64_t round_rows) {
    const int pool = e->ev_cur;
    e->ev_blocks[pool] = blocks;
    e->ev_final[pool] = first_final;
    e->ev_launches[pool] = first_final / NB * round_launches;
    e->ev_rows[pool] = first_final / NB * round_rows;
    e->ev_cur ^= 1;
}
// a grouped search of `rounds` NN rounds (steps + extra rounds) and its final round
static void timing_end_search(oamd_engine* e, int rounds, const GroupPlan& P) {
    timing_end(e, (rounds + 1) * P.K, rounds * P.K, P.K, P.round_launches, P.round_rows);
}

// The NN half of one (round, group) block, on group k's stream after its tree
// launch: the evaluation list `count` rows long at most, in launches of
// nn_batch rows, one after another within the group's NN chain (the token).
// ev: the block's timing events or nullptr; span: the block's busy-time slots
// or nullptr; max_wgs: the ResNet grid (0 = the regular one).
static int enqueue_group_nn(oamd_engine* e, const EngineView& E, const NetView& N, const GroupPlan& P, int k,
                            bool wait_token, const Event* ev, int* count, unsigned long long* span, int max_wgs) {
    hipStream_t sk = P.st[k];
    hipEvent_t token = e->pipe.nn_token[k % std::min(e->nn_chains, P.K)].get();
    // exact leaves: the group's pending leaves are solved
    // between its tree launch and the next one. Before the wait for the NN
    // token, so the solve waves run beside the other group's ResNet launch as
    // the tree waves do (measured against a launch behind this group's ResNet
    // launches). It lies between the block's tree-end and
    // NN-begin events: a timed search counts it in neither. Nothing is
    // launched with the setting off.
    launch_solve_leaves(E, P.g0[k] * E.L, P.ng[k] * E.L, sk);
    if (P.K > 1 && wait_token) HIPCHK(hipStreamWaitEvent(sk, token, 0));
    if (ev) HIPCHK(hipEventRecord(ev[2].get(), sk));
    const int grows = P.ng[k] * E.L, cb = launch_rows(grows, e->nn_batch);
    const size_t r0 = (size_t)P.g0[k] * E.L;
    for (int r = 0, j = 0; r < grows; r += cb, ++j)
        launch_resnet_packed(N, E.feat, E.FW, E.H, std::min(cb, grows - r), E.policy, E.value, sk, E.rowlist + r0 + r,
                             count, r, span ? span + (size_t)2 * j : nullptr, max_wgs);
    if (ev) HIPCHK(hipEventRecord(ev[3].get(), sk));
    if (P.K > 1) HIPCHK(hipEventRecord(token, sk));
    return OAMD_OK;
}

// The rounds of one native search over the groups of P, enqueued on the group
// streams (already forked from the engine stream). chained: the groups'
// streams carry on from a previous search of the same call (a multi-move
// self-play call), so its first NN launch also waits for the NN token.
static int enqueue_group_rounds(oamd_engine* e, const NetView& N, const GroupPlan& P, int steps, int X, bool timed,
                                bool chained) {
    const EngineView E = e->view();
    const int K = P.K;
    const int T = e->cfg.num_threads, B = e->cfg.batch_size;
    const int pool = e->ev_cur;
    // chain splitting (k_tree): X extra rounds (pick_extra_rounds) absorb the
    // rounds a split chain delays its game by; only the reference's
    // interleaving has chains
    // (X = 0 picked by the adaptive count keeps the budget: k_tree reports
    // the chains it could not split)
    const bool splitting = extra_rounds(e) > 0;
    const int budget = splitting ? e->chain_budget : 0;
    const int S = steps + X;
    // adaptive X: each group's most cuts, into this search's slot
    const bool adapt = splitting && e->adapt.on;
    const int cs = (int)(e->adapt_seq % oamd_engine::kCutSlots);
    ++e->grouped_searches;
    e->grouped_rounds += S;
    if (adapt) {
        e->cut_x[cs] = X;
        e->cut_groups[cs] = K;
        ++e->adapt_seq;
    }
    // rounds 0..S (k_tree): round s backs up what the previous rounds selected
    // and selects, thread by thread; the NN evaluates round s's selections
    // between rounds s and s+1; the last round only backs up. A timed search
    // records events for every round, the extra ones included, and counts the
    // NN rows of every round (counters [4..5]): launches, rows and busy time
    // of a timed search cover the same launches (steps + X)
    const int nlg = P.max_launches;
    unsigned long long* span = nullptr;  // this search's busy-time slots (timing on)
    if (int rc = e->reserve_spans((int64_t)K * S * nlg, &span)) return rc;
    for (int s = 0; s <= S; ++s) {
        for (int k = 0; k < K; ++k) {
            hipStream_t sk = P.st[k];
            const Event* ev = timed ? &e->pools.ev[pool][kEvPerBlock * (s * K + k)] : nullptr;
            if (ev) HIPCHK(hipEventRecord(ev[0].get(), sk));
            // evaluation list of group k: round s fills counter s % 2 and zeroes
            // the other one (which round s-1's launch, done by now, read); the
            // final round zeroes counter 0 for the next search's round 0
            int* cnt = e->rowcount.get() + 2 * k;
            int* cuts = adapt ? e->cuts.dev.get() + 2 * (cs * kMaxPipeline + k) : nullptr;
            launch_tree(E, sk, s > 0, s < S, T, B, P.g0[k], P.ng[k], 0, -1, s < S ? cnt + (s & 1) : nullptr,
                        s < S ? cnt + ((s + 1) & 1) : cnt, s == 0, budget, X, timed,
                        s == 0 || s == S ? cuts : nullptr);
            if (ev) HIPCHK(hipEventRecord(ev[1].get(), sk));
            if (s == S) {
                if (adapt) {
                    HIPCHK(hipMemcpyAsync(e->cuts.host.get() + 2 * (cs * kMaxPipeline + k), cuts, 2 * sizeof(int32_t),
                                          hipMemcpyDeviceToHost, sk));
                    HIPCHK(hipEventRecord(e->cuts.ev[cs][k].get(), sk));
                }
                continue;
            }
            // a chain's first launch of a call has no token to wait for; the
            // extra rounds evaluate lagging games only: a small looping grid
            const bool first = s == 0 && k < std::min(e->nn_chains, K) && !chained;
            if (int rc = enqueue_group_nn(e, E, N, P, k, !first, ev, cnt + (s & 1),
                                          span ? span + (size_t)2 * ((k * S + s) * nlg) : nullptr,
                                          s >= steps ? e->extra_grid : 0))
                return rc;
        }
    }
    return OAMD_OK;
}

// n > 1 group or thread streams fork from the caller's stream ...
static int fork_streams(oamd_engine* e, const hipStream_t* st, int n) {
    if (n > 1) {
        HIPCHK(hipEventRecord(e->pipe.fork_ev.get(), e->stream));
        for (int k = 0; k < n; ++k) HIPCHK(hipStreamWaitEvent(st[k], e->pipe.fork_ev.get(), 0));
    }
    return OAMD_OK;
}
// ... and join back into it
static int join_streams(oamd_engine* e, const hipStream_t* st, int n) {
    for (int k = 0; n > 1 && k < n; ++k) {
        HIPCHK(hipEventRecord(e->pipe.join_ev[k].get(), st[k]));
        HIPCHK(hipStreamWaitEvent(e->stream, e->pipe.join_ev[k].get(), 0));
    }
    return OAMD_OK;
}
static int fork_groups(oamd_engine* e, const GroupPlan& P) { return fork_streams(e, P.st, P.K); }
static int join_groups(oamd_engine* e, const GroupPlan& P) { return join_streams(e, P.st, P.K); }

// One game with T > 1 virtual threads (the drop-in MCTS, latency mode):
// virtual thread t's tree operations (backup of its batch s-1 + selection
// of batch s) and its ResNet launches alternate on a stream of its own, so
// thread t's rows are evaluated while the tree kernel backs up and selects
// for thread t+1 (the overlap the reference gets from its T threads,
// search_thread.cpp:59-128). The tree operations keep the order of one
// launch per round (thread 0 .. T-1, round by round) through an event
// from each to the next, so results are identical; an operation waits
// across streams only for the previous thread's tree operation, which ends
// while this thread's ResNet launch still runs (a ResNet launch waiting
// across streams for its selection, and a selection for its thread's
// launch, each cost ~13 us of queue latency per round).
static int search_thread_split(oamd_engine* e, const NetView& N) {
    const EngineView E = e->view();
    const int steps = e->steps();
    const int T = e->cfg.num_threads, B = e->cfg.batch_size;
    if (int rc = e->pipe.ensure(T, T)) return rc;
    // sampled timing: per (round, thread) kEvPerBlock events: tree begin/end,
    // NN begin/end (not in the final round)
    bool timed = false;
    if (int rc = timing_begin(e, steps, T, &timed)) return rc;
    const int pool = e->ev_cur;
    unsigned long long* span = nullptr;  // busy-time slots [thread][round]
    if (int rc = e->reserve_spans((int64_t)T * steps, &span)) return rc;
    hipStream_t st[kMaxPipeline] = {};  // the threads' streams
    for (int t = 0; t < T; ++t) st[t] = e->pipe.stream[t].get();
    if (int rc = fork_streams(e, st, T)) return rc;
    for (int s = 0; s <= steps; ++s) {
        for (int t = 0; t < T; ++t) {
            const Event* ev = timed ? &e->pools.ev[pool][kEvPerBlock * (s * T + t)] : nullptr;
            hipStream_t ts = st[t];  // after this thread's batch s-1 evaluation (stream order)
            if (s > 0 || t > 0)  // after the previous tree operation (thread t-1, or T-1 of round s-1)
                HIPCHK(hipStreamWaitEvent(ts, e->pipe.sel_ev[t > 0 ? t - 1 : T - 1].get(), 0));
            if (ev) HIPCHK(hipEventRecord(ev[0].get(), ts));
            launch_tree(E, ts, s > 0, s < steps, T, B, 0, 1, t, t + 1, nullptr, nullptr, s == 0, 0, 0, timed);
            if (ev) HIPCHK(hipEventRecord(ev[1].get(), ts));
            HIPCHK(hipEventRecord(e->pipe.sel_ev[t].get(), ts));
            if (s == steps) continue;
            if (ev) HIPCHK(hipEventRecord(ev[2].get(), ts));
            launch_resnet_packed(N, E.feat + (size_t)t * B * E.FW, E.FW, E.H, B, E.policy + (size_t)t * B * 65,
                                 E.value + (size_t)t * B, ts, nullptr, nullptr, 0,
                                 span ? span + (size_t)2 * (t * steps + s) : nullptr);
            if (ev) HIPCHK(hipEventRecord(ev[3].get(), ts));
        }
    }
    if (int rc = join_streams(e, st, T)) return rc;
    LAUNCHCHK();
    if (timed) timing_end(e, (steps + 1) * T, steps * T, T, T, e->L());
    return OAMD_OK;
}

// The lock-step grouped search: every group's rounds between a fork from and
// a join into the caller's stream
static int search_grouped(oamd_engine* e, const NetView& N) {
    const int K = plan_groups(e).K;
    if (int rc = e->pipe.ensure(K, K)) return rc;
    const GroupPlan P = plan_groups(e);  // the group streams exist now
    // sampled timing: per (round, group) kEvPerBlock events: tree begin/end, NN
    // begin/end (after its waits; not in the final round)
    bool timed = false;
    int X = 0;
    if (int rc = pick_extra_rounds(e, &X)) return rc;
    const int steps = e->steps();
    if (int rc = timing_begin(e, steps + X, K, &timed)) return rc;
    if (int rc = fork_groups(e, P)) return rc;
    if (int rc = enqueue_group_rounds(e, N, P, steps, X, timed, false)) return rc;
    LAUNCHCHK();
    if (int rc = join_groups(e, P)) return rc;
    if (timed) timing_end_search(e, steps + X, P);
    return OAMD_OK;
}

int oamd_engine_search(oamd_engine* e, oamd_net* net, int64_t* sims, int64_t* evals) {
    if (int rc = native_search_checks(e, net)) return rc;
    DeviceGuard dg(e->device);
    if (sims || evals) HIPCHK(hipMemsetAsync(e->counters.get(), 0, 2 * sizeof(unsigned long long), e->stream));
    const NetView N = net->view();
    e->exact_trees = true;
    if (int rc = e->thread_split() ? search_thread_split(e, N) : search_grouped(e, N)) return rc;
    // without counters requested the search is left in flight (stream order)
    if (sims || evals) {
        unsigned long long c[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(c, e->counters.get(), sizeof(c), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        if (sims) *sims = (int64_t)c[0];
        if (evals) *evals = (int64_t)c[1];
    }
    e->end_search();
    return OAMD_OK;
}

int oamd_engine_work_counters(oamd_engine* e, int64_t* sims, int64_t* evals) {
    DeviceGuard dg(e->device);
    unsigned long long c[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(c, e->counters.get() + 2, sizeof(c), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (sims) *sims = (int64_t)c[0];
    if (evals) *evals = (int64_t)c[1];
    return OAMD_OK;
}

int oamd_engine_descent_depths(oamd_engine* e, int64_t* leaves, int64_t* depth_sum, int32_t* depth_max) {
    DeviceGuard dg(e->device);
    unsigned long long c[kCounters] = {};
    HIPCHK(hipMemcpyAsync(c, e->counters.get(), sizeof(c), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (leaves) *leaves = (int64_t)c[2];
    if (depth_sum) *depth_sum = (int64_t)c[6];
    if (depth_max) *depth_max = (int32_t)c[7];
    return OAMD_OK;
}

int oamd_engine_tree_work(oamd_engine* e, int64_t* levels, int64_t* scanned, int64_t* expansions, int64_t* created,
                          int64_t* launches) {
    DeviceGuard dg(e->device);
    unsigned long long c[kCounters] = {};
    HIPCHK(hipMemcpyAsync(c, e->counters.get(), sizeof(c), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (levels) *levels = (int64_t)c[6];
    if (scanned) *scanned = (int64_t)c[8];
    if (expansions) *expansions = (int64_t)c[9];
    if (created) *created = (int64_t)c[10];
    if (launches) *launches = (int64_t)c[11];
    return OAMD_OK;
}

int oamd_engine_set_pipeline(oamd_engine* e, int32_t groups) {
    if (groups < 0 || groups > kMaxPipeline)
        return fail(OAMD_INVALID_ARGUMENT, "pipeline groups must be in [0, " + std::to_string(kMaxPipeline) + "]");
    e->pipeline = groups;
    return OAMD_OK;
}

int oamd_set_resnet_c128_four_wave(int32_t enable) {
    resnet_set_c128_four_wave(enable);
    return OAMD_OK;
}

int oamd_resnet_c128_four_wave(void) { return resnet_c128_four_wave(); }

int oamd_debug_eval_guards(oamd_engine* e, int32_t* intact) {
    if (!e || !intact) return fail(OAMD_INVALID_ARGUMENT, "eval guards: null argument");
    DeviceGuard dg(e->device);
    *intact = 1;
    const RowBuffers& r = e->rows;
    if (!r.policy.get() || !r.value.get()) return OAMD_OK;
    HIPCHK(hipDeviceSynchronize());
    unsigned char g[2][RowBuffers::kEvalGuard * sizeof(float)];
    HIPCHK(hipMemcpy(g[0], r.policy.get() + r.rows_cap * 65, sizeof(g[0]), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(g[1], r.value.get() + r.rows_cap, sizeof(g[1]), hipMemcpyDeviceToHost));
    for (auto& b : g)
        for (unsigned char c : b)
            if (c != RowBuffers::kEvalGuardByte) *intact = 0;
    return OAMD_OK;
}

int oamd_debug_engine_feature_rows(oamd_engine* e, uint64_t* out_dev, int64_t words) {
    if (!e || !out_dev) return fail(OAMD_INVALID_ARGUMENT, "feature rows: null argument");
    const int64_t have = (int64_t)e->G * e->L() * e->FW();
    if (words != have)
        return fail(OAMD_INVALID_ARGUMENT, "feature rows: expected a buffer of " + std::to_string(have) +
                                               " words, got " + std::to_string(words));
    DeviceGuard dg(e->device);
    HIPCHK(hipMemcpyAsync(out_dev, e->rows.feat.get(), (size_t)have * sizeof(uint64_t), hipMemcpyDeviceToDevice,
                          e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return OAMD_OK;
}

int oamd_debug_read_stamps(uint64_t* out, int64_t n) {
    if (!out || n < 0) return fail(OAMD_INVALID_ARGUMENT, "stamps: bad buffer");
    const int rc = resnet_read_stamps(reinterpret_cast<unsigned long long*>(out), (long long)n);
    if (rc == -2) return fail(OAMD_INVALID_ARGUMENT, "built without OAMD_STAMPS");
    return rc ? fail(OAMD_RUNTIME, "stamp copy failed") : OAMD_OK;
}

int oamd_debug_tree_stamps(uint64_t* out, int64_t n, int32_t reset) {
    if (!out || n < 0) return fail(OAMD_INVALID_ARGUMENT, "tree stamps: bad buffer");
    const int rc = tree_read_stamps(reinterpret_cast<unsigned long long*>(out), (long long)n, reset);
    if (rc == -2) return fail(OAMD_INVALID_ARGUMENT, "built without OAMD_TREE_STAMPS");
    return rc ? fail(OAMD_RUNTIME, "tree stamp copy failed") : OAMD_OK;
}

int oamd_engine_set_nn_chains(oamd_engine* e, int32_t chains) {
    if (chains < 1 || chains > PipelineStreams::kMaxChains)
        return fail(OAMD_INVALID_ARGUMENT, "nn chains must be in [1, " + std::to_string(PipelineStreams::kMaxChains) + "]");
    e->nn_chains = chains;
    return OAMD_OK;
}

int oamd_engine_set_chain_split(oamd_engine* e, int32_t budget, int32_t cuts) {
    if (budget < 0 || cuts < 0 || cuts > 64) return fail(OAMD_INVALID_ARGUMENT, "chain split: budget >= 0, cuts in [0, 64]");
    e->chain_budget = budget;
    e->chain_cuts = cuts;
    return OAMD_OK;
}

int oamd_engine_set_adaptive_extra_rounds(oamd_engine* e, int32_t enable, int32_t min_rounds) {
    if (min_rounds < 0 || min_rounds > 64) return fail(OAMD_INVALID_ARGUMENT, "adaptive extra rounds: min in [0, 64]");
    e->adapt.reset(enable != 0, min_rounds);  // the next two searches run the minimum
    for (int& x : e->cut_x) x = -1;
    return OAMD_OK;
}

int oamd_engine_round_counts(const oamd_engine* ce, int64_t* searches, int64_t* rounds, int64_t* final_launches) {
    oamd_engine* e = const_cast<oamd_engine*>(ce);  // pending events are summed here
    if (int rc = e->resolve_all_timing()) return rc;
    if (searches) *searches = e->grouped_searches;
    if (rounds) *rounds = e->grouped_rounds;
    if (final_launches) *final_launches = e->tree_final_launches;
    return OAMD_OK;
}

int oamd_engine_set_extra_round_grid(oamd_engine* e, int32_t workgroups) {
    if (workgroups < 0) return fail(OAMD_INVALID_ARGUMENT, "extra-round grid must be >= 0");
    e->extra_grid = workgroups;
    return OAMD_OK;
}

int oamd_engine_set_exact_interleaving(oamd_engine* e, int32_t enable) {
    e->exact_interleaving = enable != 0;
    return OAMD_OK;
}

int oamd_engine_set_nn_batch(oamd_engine* e, int32_t rows) {
    if (rows < 0) return fail(OAMD_INVALID_ARGUMENT, "nn batch rows must be >= 0");
    e->nn_batch = rows;
    return OAMD_OK;
}

int oamd_engine_root_info(oamd_engine* e, int32_t game, oamd_root_info* info, int32_t* visits, float* q) {
    if (game < 0 || game >= e->G) return fail(OAMD_OUT_OF_RANGE, "game index out of range");
    DeviceGuard dg(e->device);
    launch_root_stats(e->view(), game, 1, e->info_dev.get(), e->visits_dev.get(), e->q_dev.get(), 0, e->stream);
    LAUNCHCHK();
    oamd_root_info tmp;
    HIPCHK(hipMemcpyAsync(&tmp, e->info_dev.get(), sizeof(tmp), hipMemcpyDeviceToHost, e->stream));
    int32_t v[65];
    float qq[65];
    HIPCHK(hipMemcpyAsync(v, e->visits_dev.get(), sizeof(v), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(qq, e->q_dev.get(), sizeof(qq), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (info) *info = tmp;
    const int nc = tmp.num_children;
    if (visits) std::memcpy(visits, v, sizeof(int32_t) * nc);
    if (q) std::memcpy(q, qq, sizeof(float) * nc);
    return OAMD_OK;
}

int oamd_engine_status(oamd_engine* e, int32_t* overflow_games, int32_t* depth_capped_games) {
    DeviceGuard dg(e->device);
    HIPCHK(hipMemsetAsync(e->status_dev.get(), 0, 2 * sizeof(int32_t), e->stream));
    launch_status(e->view(), e->status_dev.get(), e->stream);
    LAUNCHCHK();
    int32_t h[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(h, e->status_dev.get(), sizeof(h), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (overflow_games) *overflow_games = h[0];
    if (depth_capped_games) *depth_capped_games = h[1];
    return OAMD_OK;
}

int oamd_engine_root_stats(oamd_engine* e, int32_t* visits_dev, float* q_dev, oamd_root_info* info_dev) {
    DeviceGuard dg(e->device);
    launch_root_stats(e->view(), 0, e->G, info_dev ? info_dev : e->info_dev.get(), visits_dev ? visits_dev : e->visits_dev.get(),
                      q_dev ? q_dev : e->q_dev.get(), 1, e->stream);
    LAUNCHCHK();
    return OAMD_OK;
}

int oamd_engine_root_priors(oamd_engine* e, float* priors_dev) {
    if (!priors_dev) return fail(OAMD_INVALID_ARGUMENT, "priors_dev is null");
    DeviceGuard dg(e->device);
    launch_root_priors(e->view(), priors_dev, e->stream);
    LAUNCHCHK();
    return OAMD_OK;
}

int oamd_engine_self_play_data(oamd_engine* e, int32_t game, float* features, float* policy) {
    oamd_root_info info;
    int rc = oamd_engine_root_info(e, game, &info, nullptr, nullptr);
    if (rc) return rc;
    if (info.position.player == 0)
        return fail(OAMD_INVALID_ARGUMENT, "Self-play data cannot be generated from a terminal position.");
    if (info.num_children == 0) return fail(OAMD_INVALID_ARGUMENT, "The root node has not been expanded yet.");
    DeviceGuard dg(e->device);
    const int C = 1 + 2 * e->cfg.history_size;
    float* fd = e->spd_dev.get();
    float* pd = e->spd_dev.get() + (size_t)8 * C * 64;
    launch_self_play_data(e->view(), game, fd, pd, e->stream);
    LAUNCHCHK();
    HIPCHK(hipMemcpyAsync(features, fd, sizeof(float) * 8 * C * 64, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(policy, pd, sizeof(float) * 8 * 65, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return OAMD_OK;
}

int oamd_engine_apply_action(oamd_engine* e, int32_t game, int32_t action) {
    if (game < 0 || game >= e->G) return fail(OAMD_OUT_OF_RANGE, "game index out of range");
    if (!(0 <= action && action < 65))
        return fail(OAMD_OUT_OF_RANGE, "Expected 0 <= action < 65, but got " + std::to_string(action) + ".");
    oamd_root_info info;
    int rc = oamd_engine_root_info(e, game, &info, nullptr, nullptr);
    if (rc) return rc;
    if (action == 64) {
        if (info.position.player == 0)
            return fail(OAMD_INVALID_ARGUMENT, "Pass is not allowed in a terminal position.");
        if (info.position.legal_moves != 0)
            return fail(OAMD_INVALID_ARGUMENT, "Pass is not allowed when there are legal moves.");
    } else if (((1ULL << (63 - action)) & info.position.legal_moves) == 0) {
        return fail(OAMD_INVALID_ARGUMENT, std::to_string(action) + " is not a legal action.");
    }
    if (info.node_count + 1 > e->cap) return fail(OAMD_CAPACITY, "node pool exhausted");
    DeviceGuard dg(e->device);
    launch_apply_one(e->view(), game, action, e->stream);
    LAUNCHCHK();
    return OAMD_OK;
}

int oamd_engine_apply_actions(oamd_engine* e, const int32_t* actions_dev) {
    DeviceGuard dg(e->device);
    launch_apply_actions(e->view(), actions_dev, e->stream);
    LAUNCHCHK();
    return OAMD_OK;
}

// Free-running self-play: n_moves moves of every game, each game on its own
// (tree.hip k_tree_free). Rounds are enqueued in chunks: one per move's worth
// of rounds (steps + 1 for the first search, steps for each later one: a
// schedule estimate only — a search whose batches are all terminal can
// re-select several times in one round and finish sooner, and such a game
// simply plays its next move in the same call), then tail chunks of
// kFreeTailRounds rounds until the group's remaining-games counter, copied to
// pinned memory after every chunk and read two chunks late (so the read never
// drains the queue), is 0. The
// tail chunks' ResNet launches use the small looping grid (extra_grid): only
// lagging games have rows then. Returns once the last chunk is enqueued.
//
// Work budget (sim_budget > 0): n_moves is the slice count and
// the most moves of a game; every game stops after the move whose search used
// its budget of nominal simulations up (k_free_begin). A game runs one batch
// per thread and round, so the budget lasts ceil(sim_budget / L) rounds plus
// the first search's extra one: those are the base chunks, and the tail chunks
// pick up the games that lag or overshoot (by less than one search).
static int selfplay_steps_free(oamd_engine* e, oamd_net* net, const SelfplayParams& sp, int n_moves,
                               int per_move, int32_t* actions, int32_t* finished, float* feat, float* pol,
                               int sim_budget) {
    if (int rc = e->ensure_remaining()) return rc;
    const GroupPlan P = plan_groups(e);
    const int K = P.K;
    const int T = e->cfg.num_threads, B = e->cfg.batch_size;
    const int steps = e->steps();
    const EngineView E = e->view();
    const NetView N = net->view();
    const int budget = e->exact_interleaving && e->chain_budget > 0 ? e->chain_budget : 0;
    const int nlg = P.max_launches;
    if (int rc = fork_groups(e, P)) return rc;
    int64_t round = 0;
    // everything between the fork and the join; on an error the groups are
    // still joined into the caller's stream, so that nothing the caller
    // enqueues next overlaps the rounds already in the group streams
    auto rounds = [&]() -> int {
        for (int k = 0; k < K; ++k) {
            HIPCHK(hipMemsetAsync(e->rowcount.get() + 2 * k, 0, 2 * sizeof(int32_t), P.st[k]));
            HIPCHK(hipMemsetAsync(e->remaining.dev.get() + k, 0, sizeof(int32_t), P.st[k]));
            launch_free_begin(E, P.g0[k], P.ng[k], n_moves, e->remaining.dev.get() + k, actions, finished, per_move,
                              sim_budget, P.st[k]);
        }
        bool gdone[kMaxPipeline] = {};
        const int64_t move_rounds = (int64_t)n_moves * steps + 1;
        const int64_t base_rounds =
            n_moves <= 0 ? 0 : (sim_budget > 0 ? std::min(move_rounds, ((int64_t)sim_budget + E.L - 1) / E.L + 1) : move_rounds);
        // a round completes at least one batch of every game still playing (or
        // its move): a generous bound that only a kernel fault could exceed.
        // Under a budget a game still plays at most n_moves moves of at most
        // `steps` batches per thread each, so the same bound holds.
        const int64_t max_rounds = base_rounds + (int64_t)n_moves * ((int64_t)T * steps + 2) + 4 * oamd_engine::kFreeTailRounds;
        for (int64_t chunk = 0; n_moves > 0; ++chunk) {
            int R;
            const bool tail = round >= base_rounds;
            if (!tail) {
                R = (int)std::min<int64_t>(round == 0 ? steps + 1 : steps, base_rounds - round);
                // keep at most two chunks (~two moves of GPU work) queued ahead:
                // wait (blocking, the thread sleeps) for chunk - 2 to finish.
                // Enqueuing every move at once filled the hardware queues and
                // the host spun a CPU in the launch calls for the whole call
                // (host budget)
                if (chunk >= 2 && e->throttle_enqueue) {
                    const int slot = (int)((chunk - 2) % oamd_engine::kFreeSlots);
                    for (int k = 0; k < K; ++k) HIPCHK(host_wait(e->remaining.ev[slot][k].get()));
                }
            } else {
                if (chunk >= 2) {  // chunk - 2's readback: done by now while chunk - 1 is queued
                    const int slot = (int)((chunk - 2) % oamd_engine::kFreeSlots);
                    for (int k = 0; k < K; ++k) {
                        if (gdone[k]) continue;
                        HIPCHK(host_wait(e->remaining.ev[slot][k].get()));
                        if (e->remaining.host.get()[slot * kMaxPipeline + k] == 0) gdone[k] = true;
                    }
                }
                bool all = true;
                for (int k = 0; k < K; ++k) all = all && gdone[k];
                if (all) break;
                if (round >= max_rounds) return fail(OAMD_RUNTIME, "free-running self-play did not finish");
                R = oamd_engine::kFreeTailRounds;
            }
            bool timed = false;
            if (!tail) {
                if (int rc = timing_begin(e, R, K, &timed)) return rc;
            }
            const int pool = e->ev_cur;
            unsigned long long* span = nullptr;
            if (int rc = e->reserve_spans((int64_t)K * R * nlg, &span)) return rc;
            for (int s = 0; s < R; ++s) {
                const int64_t r = round + s;
                for (int k = 0; k < K; ++k) {
                    if (gdone[k]) continue;
                    hipStream_t sk = P.st[k];
                    const Event* ev = timed ? &e->pools.ev[pool][kEvPerBlock * (s * K + k)] : nullptr;
                    int* cnt = e->rowcount.get() + 2 * k;
                    if (ev) HIPCHK(hipEventRecord(ev[0].get(), sk));
                    launch_tree_free(E, sk, P.g0[k], P.ng[k], B, cnt + (r & 1), cnt + ((r + 1) & 1), budget, timed, sp,
                                     n_moves, per_move, actions, finished, feat, pol, e->remaining.dev.get() + k,
                                     sim_budget);
                    if (ev) HIPCHK(hipEventRecord(ev[1].get(), sk));
                    // a chain's first launch of the call has no token to wait for
                    const bool first = r == 0 && k < std::min(e->nn_chains, K);
                    if (int rc = enqueue_group_nn(e, E, N, P, k, !first, ev, cnt + (r & 1),
                                                  span ? span + (size_t)2 * ((k * R + s) * nlg) : nullptr,
                                                  tail ? e->extra_grid : 0))
                        return rc;
                }
            }
            const int slot = (int)(chunk % oamd_engine::kFreeSlots);
            for (int k = 0; k < K; ++k) {
                if (gdone[k]) continue;
                HIPCHK(hipMemcpyAsync(e->remaining.host.get() + slot * kMaxPipeline + k, e->remaining.dev.get() + k, sizeof(int32_t),
                                      hipMemcpyDeviceToHost, P.st[k]));
                HIPCHK(hipEventRecord(e->remaining.ev[slot][k].get(), P.st[k]));
            }
            if (timed) timing_end(e, R * K, R * K, K, P.round_launches, P.round_rows);
            round += R;
        }
        // the next search (or call) starts with empty evaluation lists
        for (int k = 0; k < K; ++k) HIPCHK(hipMemsetAsync(e->rowcount.get() + 2 * k, 0, 2 * sizeof(int32_t), P.st[k]));
        LAUNCHCHK();
        return OAMD_OK;
    };
    const int rc = rounds();
    const int jrc = join_groups(e, P);
    e->end_search();
    if (rc) return rc;
    // (under a budget: the full searches it pays for; the games' own counts differ)
    e->grouped_searches += sim_budget > 0 ? std::min<int64_t>(n_moves, ((int64_t)sim_budget + (int64_t)steps * E.L - 1) / ((int64_t)steps * E.L)) : n_moves;
    e->grouped_rounds += round;
    return jrc;
}

int oamd_engine_set_playout_cap(oamd_engine* e, const oamd_playout_cap* cap) {
    if (!cap) {
        e->cap_p = 1.0f;
        e->cap_fast = 0;
        return OAMD_OK;
    }
    if (!(cap->full_probability > 0.0f && cap->full_probability <= 1.0f))
        return fail(OAMD_INVALID_ARGUMENT,
                    "Expected 0 < full_probability <= 1, but got " + std::to_string(cap->full_probability) + ".");
    if (cap->fast_simulations < 1 || cap->fast_simulations > e->cfg.num_simulations)
        return fail(OAMD_INVALID_ARGUMENT, "Expected 1 <= fast_simulations <= num_simulations (" +
                                               std::to_string(e->cfg.num_simulations) + "), but got " +
                                               std::to_string(cap->fast_simulations) + ".");
    if (thread_split_shape(e->G, e->cfg.num_threads))
        return fail(OAMD_INVALID_ARGUMENT,
                    "the playout cap does not run on the single-game thread-split schedule (num_games = 1, "
                    "num_threads > 1)");
    e->cap_p = cap->full_probability;
    e->cap_fast = cap->fast_simulations;
    e->end_search();
    return OAMD_OK;
}

int oamd_playout_cap_is_full(uint64_t game_key, int32_t ply, float full_probability) {
    return playout_cap_full(game_key, ply, full_probability) ? 1 : 0;
}

int oamd_engine_set_forced_playouts(oamd_engine* e, const oamd_forced_playouts* fp) {
    if (!fp) {
        e->forced_k = 0.0f;
        e->prune_targets = false;
        e->end_search();
        return OAMD_OK;
    }
    if (!(std::isfinite(fp->k) && fp->k > 0.0f))
        return fail(OAMD_INVALID_ARGUMENT, "Expected a finite forced playout factor k > 0, but got " + std::to_string(fp->k) + ".");
    e->forced_k = fp->k;
    e->prune_targets = fp->prune_targets != 0;
    e->end_search();
    return OAMD_OK;
}

// The rule of tree_game.h root_target_count on the host: the same forced.h code,
// the exploration rate as build_tables computes it.
int oamd_prune_visit_counts(int32_t n_children, int32_t root_visit_count, const int32_t* visits, const float* q,
                            const float* priors, float c_puct_base, float c_puct_init, float k, int32_t* pruned_out) {
    if (n_children < 0 || n_children > 64)
        return fail(OAMD_INVALID_ARGUMENT, "Expected 0 <= n_children <= 64, but got " + std::to_string(n_children) + ".");
    if (!(std::isfinite(k) && k > 0.0f))
        return fail(OAMD_INVALID_ARGUMENT, "Expected a finite forced playout factor k > 0, but got " + std::to_string(k) + ".");
    if (n_children > 0 && (!visits || !q || !priors || !pruned_out))
        return fail(OAMD_INVALID_ARGUMENT, "null array");
    int64_t sum = 0;
    int best = 0;
    for (int j = 0; j < n_children; ++j) {
        if (visits[j] < 0) return fail(OAMD_INVALID_ARGUMENT, "negative visit count");
        pruned_out[j] = visits[j];
        sum += visits[j];
        if (visits[j] > visits[best]) best = j;
    }
    if (sum > INT32_MAX) return fail(OAMD_INVALID_ARGUMENT, "the visit counts' sum exceeds int32");
    if (n_children <= 1 || sum == 0) return OAMD_OK;
    const int32_t total = (int32_t)sum;
    const float er = std::log(((float)(1 + root_visit_count) + c_puct_base) / c_puct_base) + c_puct_init;
    const float mult = er * sqrtf((float)total);
    const float ubest = prune_score(q[best], mult, priors[best], visits[best]);
    for (int j = 0; j < n_children; ++j)
        if (j != best) pruned_out[j] = prune_child(visits[j], q[j], priors[j], mult, ubest, k, total);
    return OAMD_OK;
}

// ---------------------------------------------------------------- exact leaves
int oamd_engine_set_exact_leaves(oamd_engine* e, int32_t max_empties) {
    if (max_empties < 0 || max_empties > kExactMaxEmpties)
        return fail(OAMD_INVALID_ARGUMENT, "Expected 0 <= max_empties <= " + std::to_string(kExactMaxEmpties) +
                                               " (0 = off), but got " + std::to_string(max_empties) + ".");
    if (!exact_setting_change_ok(e->exact_empties, max_empties, e->exact_trees))
        return fail(OAMD_INVALID_ARGUMENT,
                    "exact leaves: the setting cannot change from " + std::to_string(e->exact_empties) + " to " +
                        std::to_string(max_empties) +
                        " while games hold trees built under the old value (reset all games first)");
    e->exact_empties = max_empties;
    e->end_search();
    return OAMD_OK;
}

int oamd_engine_exact_leaf_counters(oamd_engine* e, int64_t* solves, int64_t* hits, int64_t* nodes) {
    DeviceGuard dg(e->device);
    unsigned long long c[3] = {0, 0, 0};
    HIPCHK(hipMemcpyAsync(c, e->counters.get() + 12, sizeof(c), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (solves) *solves = (int64_t)c[0];
    if (hits) *hits = (int64_t)c[1];
    if (nodes) *nodes = (int64_t)c[2];
    return OAMD_OK;
}

int oamd_engine_exact_leaf_faults(oamd_engine* e, int64_t* faults) {
    DeviceGuard dg(e->device);
    unsigned long long c = 0;
    HIPCHK(hipMemcpyAsync(&c, e->counters.get() + 15, sizeof(c), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (faults) *faults = (int64_t)c;
    return OAMD_OK;
}

static int exact_empties_checks(int32_t max_empties) {
    if (max_empties < 1 || max_empties > kExactMaxEmpties)
        return fail(OAMD_INVALID_ARGUMENT, "Expected 1 <= max_empties <= " + std::to_string(kExactMaxEmpties) +
                                               ", but got " + std::to_string(max_empties) + ".");
    return OAMD_OK;
}

int oamd_exact_leaf_sign_nodes(const oamd_position* pos, int32_t max_empties, int32_t* sign_or_none, int64_t* nodes) {
    if (!pos || !sign_or_none) return fail(OAMD_INVALID_ARGUMENT, "exact leaf sign: null argument");
    if (int rc = exact_empties_checks(max_empties)) return rc;
    if ((pos->player1_discs & pos->player2_discs) != 0 || pos->player < 0 || pos->player > 2)
        return fail(OAMD_INVALID_ARGUMENT, "exact leaf sign: not a position (overlapping discs or a bad player)");
    int32_t s = 0;
    int64_t n = 0;
    const bool is_leaf = exact_leaf_host(pos->player, pos->player1_discs, pos->player2_discs, max_empties, &s, &n);
    *sign_or_none = is_leaf ? s : OAMD_SOLVE_NONE;
    if (nodes) *nodes = is_leaf ? n : 0;
    return OAMD_OK;
}

int oamd_exact_leaf_sign(const oamd_position* pos, int32_t max_empties, int32_t* sign_or_none) {
    return oamd_exact_leaf_sign_nodes(pos, max_empties, sign_or_none, nullptr);
}

int oamd_exact_leaf_signs(int32_t device, const oamd_position* pos_dev, int64_t n, int32_t max_empties,
                          int32_t* sign_dev, int64_t* nodes_dev, void* stream) {
    if (n < 0) return fail(OAMD_INVALID_ARGUMENT, "n must be >= 0");
    if (int rc = exact_empties_checks(max_empties)) return rc;
    if (n > 0 && (!pos_dev || !sign_dev)) return fail(OAMD_INVALID_ARGUMENT, "exact leaf signs: null array");
    if (int rc = create_device_checks(device)) return rc;
    DeviceGuard dg(device);
    launch_solve_positions(pos_dev, n, max_empties, sign_dev, nodes_dev, (hipStream_t)stream);
    LAUNCHCHK();
    return OAMD_OK;
}

int oamd_engine_set_free_running(oamd_engine* e, int32_t enable) {
    e->free_running = enable != 0;
    return OAMD_OK;
}

// the moves of oamd_engine_selfplay_steps on one of its three schedules; sp
// carries the adjudication fields (pending slots laid out like `finished`)
static int selfplay_steps_enqueue(oamd_engine* e, oamd_net* net, const SelfplayParams& sp, int32_t n_moves,
                                  int32_t per_move_outputs, int32_t* actions_dev, int32_t* finished_dev,
                                  float* features_dev, float* policy_dev, int32_t sim_budget) {
    const int G = e->G, C = 1 + 2 * e->cfg.history_size;
    // move i's outputs: the i-th slice of per-move buffers, or the same G-game buffers every move
    auto out = [&](int i, auto* p, int64_t per_game) { return p ? p + (per_move_outputs ? (int64_t)i * G * per_game : 0) : p; };
    auto sp_of = [&](int i) {
        SelfplayParams m = sp;
        m.adj_pending = out(i, sp.adj_pending, 1);
        return m;
    };
    GroupPlan P = plan_groups(e);
    const bool split = e->thread_split();
    e->exact_trees = true;
    if (!split && e->free_running) {
        if (int rc = e->pipe.ensure(P.K, P.K)) return rc;
        return selfplay_steps_free(e, net, sp, n_moves, per_move_outputs, actions_dev, finished_dev, features_dev,
                                   policy_dev, sim_budget);
    }
    if (sim_budget > 0)  // (checked by the caller before anything was enqueued)
        return fail(OAMD_INVALID_ARGUMENT, "sim_budget needs the free-running schedule");
    if (split || P.K == 1) {  // one stream: the plain sequence of calls
        for (int i = 0; i < n_moves; ++i) {
            if (int rc = oamd_engine_search(e, net, nullptr, nullptr)) return rc;
            if (int rc = selfplay_move_enqueue(e, sp_of(i), out(i, actions_dev, 1), out(i, finished_dev, 1),
                                               out(i, features_dev, 8 * C * 64), out(i, policy_dev, 8 * 65)))
                return rc;
        }
        return OAMD_OK;
    }
    if (int rc = e->pipe.ensure(P.K, P.K)) return rc;
    P = plan_groups(e);
    const int steps = e->steps();
    const EngineView E = e->view();
    const NetView N = net->view();
    // Each group runs its own chain of searches and moves on its stream: its
    // move and the next search's first selection overlap the other groups'
    // last ResNet launches instead of waiting for a join after every move.
    // Per game the kernels and their order are those of search + move calls.
    int rc = fork_groups(e, P);
    for (int i = 0; !rc && i < n_moves; ++i) {
        bool timed = false;
        int X = 0;
        if ((rc = pick_extra_rounds(e, &X))) break;
        if ((rc = timing_begin(e, steps + X, P.K, &timed))) break;
        if ((rc = enqueue_group_rounds(e, N, P, steps, X, timed, i > 0))) break;
        for (int k = 0; k < P.K; ++k)
            launch_selfplay_move(E, sp_of(i), P.g0[k], P.ng[k], out(i, actions_dev, 1), out(i, finished_dev, 1),
                                 out(i, features_dev, 8 * C * 64), out(i, policy_dev, 8 * 65), P.st[k]);
        if (timed) timing_end_search(e, steps + X, P);
    }
    if (rc) return rc;
    LAUNCHCHK();
    if ((rc = join_groups(e, P))) return rc;
    e->end_search();
    return OAMD_OK;
}

// Adjudication under a budget: the resolve step walks all max_moves x G
// pending slots. A slot no move was played into is still all-zero from
// adjudicate_begin's memset (no discs), which adjudicate.hip treats as empty:
// it is told from a played slot by the pending position, not by `finished`.
int oamd_engine_selfplay_steps_budget(oamd_engine* e, oamd_net* net, const oamd_selfplay_config* cfg,
                                      int32_t max_moves, int32_t sim_budget, int32_t per_move_outputs,
                                      int32_t* actions_dev, int32_t* finished_dev, float* features_dev,
                                      float* policy_dev, int32_t max_empties, int32_t split, int32_t* margin_dev) {
    const int32_t n_moves = max_moves;
    if (int rc = adjudicate_checks(max_empties, finished_dev)) return rc;
    if (n_moves < 0) return fail(OAMD_INVALID_ARGUMENT, "n_moves must be >= 0");
    if (sim_budget < 0) return fail(OAMD_INVALID_ARGUMENT, "sim_budget must be >= 0");
    if (sim_budget > 0 && !per_move_outputs)
        return fail(OAMD_INVALID_ARGUMENT,
                    "sim_budget needs per_move_outputs (games play different numbers of moves in the call)");
    if (sim_budget > 0 && (e->thread_split() || thread_split_shape(e->G, e->cfg.num_threads) || !e->free_running))
        return fail(OAMD_INVALID_ARGUMENT,
                    "sim_budget needs the free-running schedule (oamd_engine_set_free_running, and more than one "
                    "game or one thread)");
    if (max_empties > 0 && n_moves > 1 && !per_move_outputs)
        return fail(OAMD_INVALID_ARGUMENT,
                    "adjudication needs per_move_outputs when n_moves > 1 (a move would overwrite the pending "
                    "positions of the one before)");
    if (int rc = selfplay_cfg_checks(cfg, features_dev, policy_dev)) return rc;
    if (int rc = native_search_checks(e, net)) return rc;
    DeviceGuard dg(e->device);
    SelfplayParams sp = selfplay_params(cfg);
    const int64_t n = max_empties > 0 ? (int64_t)n_moves * e->G : 0;
    if (int rc = adjudicate_begin(e, n, max_empties, split != 0, &sp)) return rc;
    if (int rc = selfplay_steps_enqueue(e, net, sp, n_moves, per_move_outputs, actions_dev, finished_dev,
                                        features_dev, policy_dev, sim_budget))
        return rc;
    // after the groups have joined the caller's stream
    return adjudicate_resolve(e, n, max_empties, split != 0, finished_dev, margin_dev, false);
}

int oamd_engine_selfplay_steps_adjudicated(oamd_engine* e, oamd_net* net, const oamd_selfplay_config* cfg,
                                           int32_t n_moves, int32_t per_move_outputs, int32_t* actions_dev,
                                           int32_t* finished_dev, float* features_dev, float* policy_dev,
                                           int32_t max_empties, int32_t split, int32_t* margin_dev) {
    return oamd_engine_selfplay_steps_budget(e, net, cfg, n_moves, 0, per_move_outputs, actions_dev, finished_dev,
                                             features_dev, policy_dev, max_empties, split, margin_dev);
}

int oamd_engine_selfplay_steps(oamd_engine* e, oamd_net* net, const oamd_selfplay_config* cfg, int32_t n_moves,
                               int32_t per_move_outputs, int32_t* actions_dev, int32_t* finished_dev,
                               float* features_dev, float* policy_dev) {
    return oamd_engine_selfplay_steps_adjudicated(e, net, cfg, n_moves, per_move_outputs, actions_dev, finished_dev,
                                                  features_dev, policy_dev, 0, 0, nullptr);
}

int oamd_engine_game_key(oamd_engine* e, int32_t game, uint64_t* key) {
    if (game < 0 || game >= e->G) return fail(OAMD_OUT_OF_RANGE, "game index out of range");
    DeviceGuard dg(e->device);
    HIPCHK(hipMemcpyAsync(key, &e->games.get()[game].key, sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return OAMD_OK;
}

int oamd_engine_game_event(oamd_engine* e, int32_t game, uint64_t* event) {
    if (game < 0 || game >= e->G) return fail(OAMD_OUT_OF_RANGE, "game index out of range");
    DeviceGuard dg(e->device);
    HIPCHK(hipMemcpyAsync(event, &e->games.get()[game].event, sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return OAMD_OK;
}

int oamd_engine_set_active(oamd_engine* e, const uint8_t* active_dev) {
    DeviceGuard dg(e->device);
    launch_set_active(e->view(), active_dev, e->stream);
    LAUNCHCHK();
    return OAMD_OK;
}

// ------------------------------------------- given positions
int oamd_host_canonical_position(const oamd_position* in, oamd_position* out) {
    if (!in || !out) return fail(OAMD_INVALID_ARGUMENT, "canonical_position: null position");
    const int32_t f = position_fault(in->player, in->player1_discs, in->player2_discs);
    if (f == kSetPosBadPlayer)
        return fail(OAMD_INVALID_ARGUMENT, "Expected player in {0, 1, 2}, but got " + std::to_string(in->player) + ".");
    if (f) return fail(OAMD_INVALID_ARGUMENT, "The two players' disc sets overlap.");
    const Pos c = canonical_position(in->player, in->player1_discs, in->player2_discs);
    std::memcpy(out, &c, sizeof(Pos));
    return OAMD_OK;
}

int oamd_engine_set_positions(oamd_engine* e, const oamd_position* pos_dev, const oamd_position* history_dev,
                              int32_t history_k, const int32_t* hist_len_dev, const uint64_t* keys_dev,
                              const int32_t* ply_dev, const uint8_t* mask_dev, uint64_t seed, int32_t* status_dev) {
    if (!pos_dev) return fail(OAMD_INVALID_ARGUMENT, "set_positions: pos_dev is NULL");
    if (history_k < 0 || history_k > kMaxHistory)
        return fail(OAMD_INVALID_ARGUMENT, "set_positions: Expected 0 <= history_k <= " + std::to_string(kMaxHistory) +
                                               ", but got " + std::to_string(history_k) + ".");
    if (history_k > 0 && !history_dev)
        return fail(OAMD_INVALID_ARGUMENT, "set_positions: history_dev is NULL with history_k > 0");
    DeviceGuard dg(e->device);
    launch_set_positions(e->view(), pos_dev, history_dev, history_k, hist_len_dev, keys_dev, ply_dev, mask_dev, seed,
                         status_dev, e->stream);
    LAUNCHCHK();
    // a reset of single games: no step-wise search stays open, and exact_trees
    // stays as it is (a rejected game keeps its tree, and nobody waited to know)
    e->end_search();
    return OAMD_OK;
}

int oamd_engine_principal_variations(oamd_engine* e, int32_t max_len, int32_t* pv_actions_dev, int32_t* pv_visits_dev,
                                     float* pv_q_dev, int32_t* pv_len_dev) {
    if (max_len < 1 || max_len > 64)
        return fail(OAMD_INVALID_ARGUMENT,
                    "principal_variations: Expected 1 <= max_len <= 64, but got " + std::to_string(max_len) + ".");
    if (!pv_actions_dev || !pv_visits_dev || !pv_q_dev || !pv_len_dev)
        return fail(OAMD_INVALID_ARGUMENT, "principal_variations: null output buffer");
    DeviceGuard dg(e->device);
    launch_principal_variations(e->view(), max_len, pv_actions_dev, pv_visits_dev, pv_q_dev, pv_len_dev, e->stream);
    LAUNCHCHK();
    return OAMD_OK;
}

}  // extern "C"
