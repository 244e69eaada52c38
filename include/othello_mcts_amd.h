/*
 * othello_mcts_amd.h — C ABI of the MI355X-native othello_mcts engine.
 *
 * Plain pointers and sizes only (no torch / pybind types). Every entry point
 * names the reference interface it replaces (yunhao-qian/Othello-AlphaZero,
 * paths relative to cpp/src/). The Python package othello_mcts
 * (othello-alphazero_amd/othello_mcts) is a pybind11 layer over exactly these
 * functions; INTEGRATION.md shows the binding a maintainer of the reference
 * would add.
 *
 * Conventions
 *   - Return value: OAMD_OK (0) or an oamd_status; oamd_last_error() holds the
 *     message (thread-local). The pybind layer maps OAMD_INVALID_ARGUMENT to
 *     ValueError and OAMD_OUT_OF_RANGE to IndexError, like the reference's
 *     std::invalid_argument / std::out_of_range (othello_mcts.cpp, pybind11).
 *   - "dev" pointers are HIP device pointers on the engine's / net's device;
 *     "host" pointers are ordinary host memory.
 *   - `stream` is a hipStream_t (NULL = the legacy default stream).
 *   - Bit order: square i = row*8 + col, bitboard bit (63 - i) (position.h:275).
 *   - Actions: 0..63 squares, 64 = pass (position.h:402-408).
 */
#ifndef OTHELLO_MCTS_AMD_H
#define OTHELLO_MCTS_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OAMD_ABI_VERSION 1

typedef enum oamd_status {
    OAMD_OK = 0,
    OAMD_INVALID_ARGUMENT = 1, /* std::invalid_argument -> ValueError */
    OAMD_OUT_OF_RANGE = 2,     /* std::out_of_range     -> IndexError */
    OAMD_RUNTIME = 3,          /* HIP / device failure  -> RuntimeError */
    OAMD_CAPACITY = 4          /* node pool exhausted   -> RuntimeError */
} oamd_status;

const char *oamd_last_error(void);
int oamd_abi_version(void);
/* Hash of the sources the library was built from (16 hex digits; family
 * "resnet", "tree" or "all", else NULL): build.py compiles them in, and
 * othello_mcts.provenance compares them with the sources on disk. */
const char *oamd_source_hash(const char *family);
/* number of visible HIP devices (0 when no GPU) */
int oamd_device_count(int32_t *out);

/* ------------------------------------------------------------------------ */
/* Batched bitboards (device, bit-exact with position.h)                     */
/* ------------------------------------------------------------------------ */

/* Same memory layout as the engine's Position value type (40 bytes). */
typedef struct oamd_position {
    int32_t player; /* 1 black, 2 white, 0 terminal  (position.h:47) */
    int32_t reserved;
    uint64_t player1_discs;    /* position.h:53 */
    uint64_t player2_discs;    /* position.h:59 */
    uint64_t legal_moves;      /* position.h:74 */
    uint64_t next_legal_moves; /* position.h:148 (private in the reference) */
} oamd_position;

/* replaces othello::get_legal_moves (position.h:202-229), n boards */
int oamd_get_legal_moves(const uint64_t *player_discs_dev, const uint64_t *opponent_discs_dev,
                         uint64_t *out_dev, int64_t n, void *stream);
/* replaces othello::get_flips (position.h:231-262), n boards */
int oamd_get_flips(const uint64_t *move_mask_dev, const uint64_t *player_discs_dev,
                   const uint64_t *opponent_discs_dev, uint64_t *out_dev, int64_t n, void *stream);
/* replaces Position::apply_action (position.h:402-408, unchecked), n positions */
int oamd_apply_action(const oamd_position *in_dev, const int32_t *actions_dev,
                      oamd_position *out_dev, int64_t n, void *stream);
/* replaces Position::initial_position (position.h:264-272) */
int oamd_initial_position(oamd_position *out_host);

/* Scalar host forms of the same functions (the Python Position API and
 * get_legal_moves / get_flips, used by player.py:45-160). Same source as the
 * device kernels (csrc/bitboard.h, __host__ __device__). */
uint64_t oamd_host_legal_moves(uint64_t player_discs, uint64_t opponent_discs);
uint64_t oamd_host_flips(uint64_t move_mask, uint64_t player_discs, uint64_t opponent_discs);
void oamd_host_apply_action(const oamd_position *in_host, int32_t action, oamd_position *out_host);

/* ------------------------------------------------------------------------ */
/* Native network: replaces the Python NeuralNet callback                   */
/* (neural_net.h:15-29, othello_mcts.cpp:19-45) for AlphaZeroNet             */
/* (python/othello_alphazero/neural_net.py:138-172) in eval mode.            */
/* ------------------------------------------------------------------------ */

typedef enum oamd_dtype { OAMD_BF16 = 0, OAMD_FP16 = 1 } oamd_dtype;

typedef struct oamd_net_desc {
    int32_t in_channels;                /* 1 + 2 * history_size, <= 31 */
    int32_t conv_channels;              /* 128 or 256 */
    int32_t num_residual_blocks;        /* >= 0 */
    int32_t value_head_hidden_channels; /* >= 1 */
    int32_t num_squares;                /* must be 64 */
    int32_t num_actions;                /* must be 65 */
    int32_t dtype;                      /* oamd_dtype */
} oamd_net_desc;

typedef struct oamd_net oamd_net;

int oamd_net_create(int32_t device, const oamd_net_desc *desc, oamd_net **out);
int oamd_net_destroy(oamd_net *net);
/* Number of tensors oamd_net_load_state expects (= AlphaZeroNet.state_dict()
 * entries without num_batches_tracked), and the i-th key / element count. */
int oamd_net_state_size(const oamd_net *net, int32_t *n_tensors);
int oamd_net_state_key(const oamd_net *net, int32_t i, const char **key, int64_t *numel);
/* Host fp32 tensors in oamd_net_state_key order. BatchNorm (eval, eps 1e-5)
 * is folded into the preceding convolution; weights are packed into the
 * MFMA fragment layout and converted to the net's dtype. */
int oamd_net_load_state(oamd_net *net, const float *const *tensors_host, int32_t n_tensors);
/* features_dev: (rows, in_channels, 8, 8) fp32; policy_dev (rows, 65)
 * probabilities; value_dev (rows,) in [-1, 1]. */
int oamd_net_forward(oamd_net *net, const float *features_dev, int32_t rows, float *policy_dev,
                     float *value_dev, void *stream);

/* ------------------------------------------------------------------------ */
/* Search engine: G independent games, one tree per game in HBM.             */
/* Replaces othello::MCTS (mcts.h:35-216, mcts.cpp) and SearchThread         */
/* (search_thread.cpp); G = 1 is the reference's single-game object.         */
/* ------------------------------------------------------------------------ */

/* MCTS(...) constructor arguments (othello_mcts.cpp:89-112, keyword names
 * authoritative). torch_device / torch_pin_memory live in the Python layer. */
typedef struct oamd_search_config {
    int32_t history_size;    /* >= 1, <= 15 */
    int32_t num_simulations; /* >= 1 */
    int32_t num_threads;     /* >= 1: virtual search threads */
    int32_t batch_size;      /* >= 1: leaves per virtual thread per step */
    float c_puct_base;       /* > 0 */
    float c_puct_init;       /* >= 0 */
    float dirichlet_epsilon; /* in [0, 1] */
    float dirichlet_alpha;   /* >= 0 */
} oamd_search_config;

typedef struct oamd_engine oamd_engine;

/* node_capacity: nodes per game (0 = default 1<<20). Nodes are never freed
 * while a game lasts (history ancestors stay valid, mcts.cpp:140-165);
 * oamd_engine_reset recycles a game's pool. */
int oamd_engine_create(int32_t device, int32_t num_games, int64_t node_capacity,
                       const oamd_search_config *config, uint64_t seed, oamd_engine **out);
int oamd_engine_destroy(oamd_engine *e);
/* mcts.cpp:167-241 setters (validated; OAMD_INVALID_ARGUMENT with the
 * reference's messages) */
int oamd_engine_set_config(oamd_engine *e, const oamd_search_config *config);
int oamd_engine_get_config(const oamd_engine *e, oamd_search_config *config);
int oamd_engine_num_games(const oamd_engine *e, int32_t *out);
int oamd_engine_set_stream(oamd_engine *e, void *stream);
/* game = -1: all games. Resets to the initial position (mcts.cpp:40-43) and
 * reseeds the game's random stream with (seed, game). */
int oamd_engine_reset(oamd_engine *e, int32_t game, uint64_t seed);

/* Whole search for every active game with the native net
 * (MCTS::search, mcts.h:220-256). Outputs are optional (may be NULL):
 * simulations = leaf selections (sum over games), evaluations = NN rows of
 * non-terminal leaves. With both NULL the call returns once the search is
 * enqueued (stream order; the host does not wait), otherwise after it ends.
 * One game with num_threads > 1 runs thread by thread, each thread's ResNet
 * rows on a stream of their own while the next thread's tree work runs
 * (same results; OAMD_TREE_SPLIT=0 in the environment turns it off). */
int oamd_engine_search(oamd_engine *e, oamd_net *net, int64_t *simulations, int64_t *evaluations);
/* Work done since the engine was created (host outputs; waits for the
 * engine's stream): simulations (leaf selections) and evaluations (NN rows of
 * non-terminal leaves, BASELINE.md's n_eval) over every search, native or
 * step-wise. The reference counts neither; it builds no NN row for a terminal
 * leaf (search_thread.cpp:88-90). */
int oamd_engine_work_counters(oamd_engine *e, int64_t *simulations, int64_t *evaluations);
/* Tree shape since the engine was created (host outputs; waits for the
 * engine's stream): leaves selected (= simulations), the sum of their descent
 * depths (levels below the root, search_thread.cpp:64-67) and the deepest
 * descent. mean depth = depth_sum / leaves. */
int oamd_engine_descent_depths(oamd_engine *e, int64_t *leaves, int64_t *depth_sum, int32_t *depth_max);
/* Rows per ResNet launch in oamd_engine_search (0 = a whole pipeline group per
 * launch): a group's rows are evaluated by consecutive launches of at most
 * `rows` rows on its stream (the NN evaluation batch; configs[4] uses 2048).
 * Results do not depend on it. */
int oamd_engine_set_nn_batch(oamd_engine *e, int32_t rows);
/* Counts since the engine was created: grouped native searches enqueued (all
 * pipeline groups of one search count once), their NN rounds (steps + extra
 * rounds each), and the final backup-only k_tree launches of the timed
 * searches (the launches behind oamd_engine_tree_timing's backup_ms). */
int oamd_engine_round_counts(const oamd_engine *e, int64_t *searches, int64_t *rounds,
                             int64_t *final_launches);
/* enable = 1 (default): the reference's thread interleaving exactly — a
 * virtual thread whose batch is all terminal backs it up without an NN round
 * trip and selects again at once (search_thread.cpp:102-127), in the same
 * round. enable = 0: such a batch waits for its thread's next round like any
 * other (the round-robin of round 2): identical results until a batch is all
 * terminal (endgames), and no round longer than one batch per thread, so the
 * search rounds stay hidden behind the other pipeline group's ResNet launch
 * in sustained self-play. */
int oamd_engine_set_exact_interleaving(oamd_engine *e, int32_t enable);

/* Step-wise search for an external evaluator (the Python NeuralNet callback
 * path, othello_mcts.cpp:36-45). Rows: row = game * L + leaf, L =
 * num_threads * batch_size; virtual thread k of a game owns leaves
 * [k*batch_size, (k+1)*batch_size) (search_thread.cpp:59-128).
 *   begin -> steps;  repeat steps times: select, [features, evaluate,
 *   set_evaluation];  then backup once.
 * select backs up the previous round's batch of each thread right before that
 * thread selects its next batch: the interleaving the reference's threads
 * produce (search_thread.cpp:47-128 with mcts.h:242-251's FIFO NN service).
 * Calling backup after every select gives the lock-step order instead. */
int oamd_engine_search_begin(oamd_engine *e, int32_t *steps);
int oamd_engine_select(oamd_engine *e);
/* host_out[row] = 1 when the row needs the NN this round: a non-terminal leaf
 * of a batch that waits for its evaluation (a virtual thread whose batch was
 * all terminal backed it up without one and selected again,
 * search_thread.cpp:102-127; a thread that ran out of batches has none) */
int oamd_engine_leaf_flags(oamd_engine *e, uint8_t *host_out);
/* features_dev: (rows, 1 + 2H, 8, 8) fp32 of rows [row_begin, row_begin+rows) */
int oamd_engine_features(oamd_engine *e, float *features_dev, int32_t row_begin, int32_t rows);
int oamd_engine_set_evaluation(oamd_engine *e, const float *policy_dev, const float *value_dev,
                               int32_t row_begin, int32_t rows);
int oamd_engine_backup(oamd_engine *e);

/* Root queries (mcts.cpp:45-61, mcts.h:69-71). visits/q are in
 * legal_actions() order, arrays of >= 65 entries. */
typedef struct oamd_root_info {
    oamd_position position;
    int32_t num_children; /* 0 while the root is unexpanded */
    int32_t visit_count;  /* root N (includes virtual-loss increments) */
    int32_t overflow;     /* node pool exhausted during a search */
    int32_t reserved;
    int64_t node_count;
} oamd_root_info;

int oamd_engine_root_info(oamd_engine *e, int32_t game, oamd_root_info *info_host,
                          int32_t *visits_host, float *q_host);
/* Engine health (host outputs; waits for the engine's stream): number of
 * games whose node pool was exhausted (a leaf could not be expanded: the
 * search no longer follows the reference) and of games whose descent hit the
 * path-depth cap, since each game's last reset. Callers raise on nonzero. */
int oamd_engine_status(oamd_engine *e, int32_t *overflow_games, int32_t *depth_capped_games);
/* All games at once (device buffers): visits_dev (G, 65) and q_dev (G, 65)
 * indexed BY ACTION (0 where not a child), info_dev (G) */
int oamd_engine_root_stats(oamd_engine *e, int32_t *visits_dev, float *q_dev,
                           oamd_root_info *info_dev);
/* mcts.cpp:63-112: features (8, 1+2H, 8, 8) fp32, policy (8, 65) fp32, host.
 * OAMD_INVALID_ARGUMENT if the root is terminal or unexpanded. */
int oamd_engine_self_play_data(oamd_engine *e, int32_t game, float *features_host,
                               float *policy_host);
/* mcts.cpp:114-165 for one game (validated, reference messages) */
int oamd_engine_apply_action(oamd_engine *e, int32_t game, int32_t action);
/* Batched: actions_dev (G), -1 = leave the game as is (not validated). */
int oamd_engine_apply_actions(oamd_engine *e, const int32_t *actions_dev);

/* ------------------------------------------------------------------------ */
/* On-device self-play driver (train.py:404-452 per move, all games):        */
/* choose the move from root visits (temperature sampling for the first      */
/* `temperature_moves` plies, argmax with random tie-break afterwards), emit  */
/* the 8-fold training targets of the root (optional), apply the move, and   */
/* restart finished games from a random opening of up to                     */
/* `opening_moves` uniformly random plies.                                   */
/* ------------------------------------------------------------------------ */
typedef struct oamd_selfplay_config {
    int32_t temperature_moves; /* reference: 12 */
    float temperature;         /* reference: 1.0 */
    int32_t opening_moves;     /* random plies after a restart (0 = none) */
    int32_t emit_targets;      /* 1: write features/policy of every move */
} oamd_selfplay_config;

/* Per move, per game outputs (device, may be NULL):
 *   actions_dev (G) chosen action (-1 inactive); finished_dev (G): bits 0-1 =
 *   0 game continues, 1 draw, 2 black won, 3 white won (the game ended with
 *   this move and restarted); bit 2 = the root was unexpanded, no targets were
 *   written (the move was uniform); bit 3 = the game's node pool overflowed;
 *   bit 7 (128) = the move followed a fast search of a playout cap (below): it
 *   was played, but no targets were written;
 *   features_dev (G, 8, 1+2H, 8, 8) and policy_dev (G, 8, 65) targets. */
int oamd_engine_selfplay_move(oamd_engine *e, const oamd_selfplay_config *cfg,
                              int32_t *actions_dev, int32_t *finished_dev, float *features_dev,
                              float *policy_dev);
/* n_moves self-play moves of every game with the native net: per move one
 * oamd_engine_search + oamd_engine_selfplay_move, identical results, but each
 * pipeline group chains its searches and moves on its own stream (no join
 * between moves: a group's move and next selection overlap the other groups'
 * ResNet launches). Enqueued only (stream order). per_move_outputs = 1: the
 * output buffers hold n_moves consecutive slices of the per-move shapes above
 * (move i at offset i x G rows); 0: every move overwrites the same slice.
 * Replaces the reference's per-move loop train.py:404-452 (_self_play). */
int oamd_engine_selfplay_steps(oamd_engine *e, oamd_net *net, const oamd_selfplay_config *cfg,
                               int32_t n_moves, int32_t per_move_outputs, int32_t *actions_dev,
                               int32_t *finished_dev, float *features_dev, float *policy_dev);
/* Adjudication by the exact endgame solver (opt-in; the variants below with
 * max_empties = 0 ARE the calls above). K = max_empties in 1..16: after a
 * searched move has been applied, a new root that is not terminal and has at
 * most K empty squares (a mover that must pass counts) ends the game there. The
 * root is solved exactly (oamd_solve_endgames, or oamd_solve_endgames_split
 * when split != 0, with the largest node limit) and reported like a game that
 * ended on the board: the game restarts in the same launch, and
 *   finished bit 5 (32) = the game was adjudicated at this move; bits 0-1 = 2,
 *     3 or 1 for margin > 0, < 0, = 0, filled in by a resolve step the call
 *     enqueues on the engine's stream after the moves (stream order);
 *   finished bit 6 (64) = the solver flagged the position (no outcome bits;
 *     cannot happen for a position the engine produced);
 *   margin_dev (shaped like finished_dev, may be NULL): the exact score seen
 *     from black (the solver's score, negated when white is to move), black
 *     minus white discs for a game that ended on the board, INT32_MIN where no
 *     game ended.
 * The test runs only after a searched move: a restart whose random opening
 * lands at or below K empties is searched once, then adjudicated. finished_dev
 * is required when max_empties > 0. OAMD_INVALID_ARGUMENT: max_empties outside
 * 0..16; max_empties > 0 with n_moves > 1 and per_move_outputs = 0 (the
 * pending positions of a move would be overwritten by the next). The engine
 * owns the workspace and grows it on demand. Enqueued only. */
int oamd_engine_selfplay_move_adjudicated(oamd_engine *e, const oamd_selfplay_config *cfg,
                                          int32_t *actions_dev, int32_t *finished_dev, float *features_dev,
                                          float *policy_dev, int32_t max_empties, int32_t split,
                                          int32_t *margin_dev);
int oamd_engine_selfplay_steps_adjudicated(oamd_engine *e, oamd_net *net, const oamd_selfplay_config *cfg,
                                           int32_t n_moves, int32_t per_move_outputs, int32_t *actions_dev,
                                           int32_t *finished_dev, float *features_dev, float *policy_dev,
                                           int32_t max_empties, int32_t split, int32_t *margin_dev);

/* Playout cap randomization (KataGo, Wu 2019, section 3.1; DESIGN.md §17;
 * opt-in, off by default). With a cap set, the search of a game at ply `ply`
 * (moves since its last restart or opening) is a FULL one - num_simulations,
 * root noise, its move recorded as a training target - when
 * oamd_playout_cap_is_full(game key, ply, full_probability) says so, which
 * happens with probability full_probability. Otherwise it is a FAST one:
 * fast_simulations (rounded up to whole batches like num_simulations), no
 * root Dirichlet noise (no noise events are consumed), and the self-play
 * move that follows it is chosen and applied as ever but writes no targets
 * and reports finished bit 7 (128). The draw consumes no event of the game's
 * random stream, and the tree is reused across moves as ever. It applies to
 * every search of the engine: oamd_engine_search, the step API
 * (oamd_engine_search_begin still returns the full step count; the rows of a
 * game on a fast search are simply not flagged after its steps) and
 * oamd_engine_selfplay_steps. The arena does not use it and rejects an engine
 * that has it set. */
typedef struct oamd_playout_cap {
    float full_probability;   /* in (0, 1]; 1 = every search is full */
    int32_t fast_simulations; /* in 1..num_simulations */
} oamd_playout_cap;
/* cap = NULL: off. OAMD_INVALID_ARGUMENT: a value out of range; an engine of
 * one game with more than one thread (the thread-split schedule). While a
 * cap is set, oamd_engine_set_config rejects a config it does not fit. */
int oamd_engine_set_playout_cap(oamd_engine *e, const oamd_playout_cap *cap);
/* The full / fast draw (host): 1 = full. The key is oamd_engine_game_key's. */
int oamd_playout_cap_is_full(uint64_t game_key, int32_t ply, float full_probability);
/* oamd_engine_selfplay_steps_adjudicated with a work budget per game in place
 * of a move count (sim_budget = 0 IS that call, max_moves its n_moves).
 * sim_budget > 0: max_moves is the number of output slices and the most moves
 * a game plays in the call; a game stops after the move whose search brought
 * the nominal simulations (batches per thread x num_threads x batch_size) of
 * the searches it started in this call to sim_budget or more. A game always
 * finishes the search it started, so it overshoots by less than one search.
 * Move i of a game goes to slice i; every slice of every game is first filled
 * with action -1 and finished 0 ("nothing played"), so a game's played moves
 * are a prefix of its slices. With adjudication the slots nothing was played
 * into have margin INT32_MIN. OAMD_INVALID_ARGUMENT: sim_budget > 0 with
 * per_move_outputs = 0, with the free-running schedule switched off, or on an
 * engine of one game with more than one thread. */
int oamd_engine_selfplay_steps_budget(oamd_engine *e, oamd_net *net, const oamd_selfplay_config *cfg,
                                      int32_t max_moves, int32_t sim_budget, int32_t per_move_outputs,
                                      int32_t *actions_dev, int32_t *finished_dev, float *features_dev,
                                      float *policy_dev, int32_t max_empties, int32_t split,
                                      int32_t *margin_dev);

/* Forced playouts and policy target pruning (KataGo, Wu 2019, section 3.2;
 * DESIGN.md §18; opt-in, off by default). All arithmetic below is fp32 in the
 * order written.
 *
 * Forced playouts: at the root of a FULL search (every search without a
 * playout cap; never a fast one), a selection with more than one child scores
 * child c with n_c visits (in-flight ones included) as
 *     forced_c = n_c > 0 && (float)n_c * (float)n_c < (k * prob_c) * (float)total
 *     ucb_c    = forced_c ? +inf : q_c + mult * prob_c / (1 + (float)n_c)
 * where prob_c is the prior of this selection's PUCT line (the noised one when
 * dirichlet_epsilon > 0) and total the children's visit sum: a child that has
 * been tried keeps a floor of sqrt(k * prob_c * total) visits. The first
 * maximum wins, so the forced child of the lowest index is taken. The rule
 * consumes no random event and does not depend on dirichlet_epsilon.
 *
 * Policy target pruning (prune_targets != 0): the self-play targets
 * (oamd_engine_self_play_data, oamd_engine_selfplay_move / _steps) are written
 * from the pruned counts of oamd_prune_visit_counts in place of the raw visit
 * counts, n'_j / sum n'. Visit counts and Q as queried, the move choice, every
 * `finished` bit and tree reuse do not change.
 *
 * The arena does not use the setting and rejects an engine that has it. */
typedef struct oamd_forced_playouts {
    float k;               /* finite, > 0; KataGo uses 2 */
    int32_t prune_targets; /* 1: targets from the pruned counts */
} oamd_forced_playouts;
/* fp = NULL: off. OAMD_INVALID_ARGUMENT unless k is finite and > 0. */
int oamd_engine_set_forced_playouts(oamd_engine *e, const oamd_forced_playouts *fp);
/* The pruning rule (host; the code the device runs). visits, q and priors (the
 * stored priors, without noise) are the root's n_children children in child
 * order, root_visit_count the root's own N. With n_children <= 1 or
 * total = sum visits = 0 the counts are copied. Else best = the first child
 * with the most visits, mult = explore_rate(root_visit_count) *
 * sqrtf((float)total) with explore_rate(N) = logf(((float)(1 + N) + c_puct_base)
 * / c_puct_base) + c_puct_init, u(j, m) = q_j + mult * p_j / (1.0f + (float)m),
 * ubest = u(best, n_best), and for every j != best with n_j > 0:
 *     cap = (int)sqrtf((k * p_j) * (float)total);  m = n_j
 *     at most cap times, while m > 0: if u(j, m - 1) < ubest then m -= 1 else stop
 *     if m < n_j and m == 1 then m = 0
 *     pruned_out[j] = m
 * pruned_out[best] = n_best. OAMD_INVALID_ARGUMENT: n_children outside 0..64,
 * a negative count, k not finite or <= 0. */
int oamd_prune_visit_counts(int32_t n_children, int32_t root_visit_count, const int32_t *visits,
                            const float *q, const float *priors, float c_puct_base, float c_puct_init,
                            float k, int32_t *pruned_out);
/* The stored priors P of every game's root children: priors_dev (G, 65) by
 * action like oamd_engine_root_stats, 0 where there is no child. Enqueued
 * only. */
int oamd_engine_root_priors(oamd_engine *e, float *priors_dev);
/* Reset every game to a random opening. */
int oamd_engine_random_openings(oamd_engine *e, int32_t max_moves, uint64_t seed);
/* The random-stream key of a game (DESIGN.md "Random streams"). */
int oamd_engine_game_key(oamd_engine *e, int32_t game, uint64_t *key_host);
/* The number of events the game has drawn from its stream since its last
 * reset or restart: the index of its next draw (waits for the engine's stream). */
int oamd_engine_game_event(oamd_engine *e, int32_t game, uint64_t *event_host);

/* Per-game search mask: active_dev (G) bytes, nonzero = the game is searched,
 * moved by oamd_engine_selfplay_move and by oamd_engine_apply_actions; NULL =
 * every game. A native search of an engine with no active game is a no-op
 * (0 simulations, 0 evaluations). oamd_engine_reset reactivates the games it
 * resets. */
int oamd_engine_set_active(oamd_engine *e, const uint8_t *active_dev);

/* ------------------------------------------------------------------------ */
/* Search from given positions: a root set from outside and  */
/* the principal variation below a searched root. The counterpart of         */
/* MCTS::reset_position (mcts.cpp:40-43) for a position that is not the      */
/* initial one; the reference has no such entry point.                       */
/* ------------------------------------------------------------------------ */

/* The canonical form of a position, from its player and two disc sets alone
 * (the other fields of *in_host are not read): legal_moves and
 * next_legal_moves as Position::apply_action would have left them; a side to
 * move that has no move while the opponent has one stays to move (a pass
 * position: legal_moves 0, next_legal_moves the opponent's moves, action 64
 * legal); player 1 or 2 where neither side has a move becomes terminal
 * (player 0), and a terminal position has no moves. The same code runs on
 * the device in oamd_engine_set_positions (csrc/positions.h).
 * OAMD_INVALID_ARGUMENT: player outside 0..2 or overlapping disc sets. */
int oamd_host_canonical_position(const oamd_position *in_host, oamd_position *out_host);

/* status_dev values of oamd_engine_set_positions */
#define OAMD_SET_POSITIONS_OK 0
#define OAMD_SET_POSITIONS_SKIPPED (-1)           /* the mask left the game alone */
#define OAMD_SET_POSITIONS_BAD_PLAYER 1           /* player outside 0..2 */
#define OAMD_SET_POSITIONS_OVERLAP 2              /* a square holds a disc of both colours */
#define OAMD_SET_POSITIONS_HISTORY_BAD_PLAYER 3   /* ... in one of the game's used history entries */
#define OAMD_SET_POSITIONS_HISTORY_OVERLAP 4
#define OAMD_SET_POSITIONS_BAD_HIST_LEN 5         /* hist_len outside 0..history_k */
#define OAMD_SET_POSITIONS_BAD_PLY 6              /* ply < 0 */
#define OAMD_SET_POSITIONS_CAPACITY 7             /* node_capacity < hist_len + 1 */

/* Put a position at the root of every selected game. All pointers are device
 * pointers with one entry per game of the engine (G); all but pos_dev may be
 * NULL.
 *   pos_dev (G): the roots. Only player and the two disc sets are read; the
 *     engine stores the canonical form (oamd_host_canonical_position), so a
 *     position whose sides both have no move is a terminal root.
 *   history_dev (G, history_k), history_k in 0..15: the positions before the
 *     root, newest first (entry 0 is the root's parent). They fill the history
 *     planes of every feature row and self-play target below this root, as the
 *     game's own earlier roots do; nothing checks that they form a legal game.
 *   hist_len_dev (G), each in 0..history_k: the used entries of each game;
 *     NULL = history_k for every game. Planes past them are zero, as for a
 *     game with fewer moves than history_size (position_iterator.h:24-71).
 *   keys_dev (G): the games' random-stream keys; NULL = the key
 *     oamd_engine_reset(e, game, seed) gives. `seed` is not read otherwise.
 *   ply_dev (G), each >= 0: the moves played so far, which the self-play move's
 *     temperature schedule and the playout cap's draw read; NULL = discs on
 *     the board - 4.
 *   mask_dev (G) bytes: nonzero = set this game; NULL = every game.
 *   status_dev (G) out: OAMD_SET_POSITIONS_OK for a game that was set,
 *     _SKIPPED for one the mask left alone, else the fault (the first of: the
 *     root's, hist_len, ply, capacity, the history's from the newest entry on).
 * A game that is set is as after oamd_engine_reset (a fresh node pool, active,
 * event 0, no arena match, sticky flags cleared) with this root, key and ply.
 * A rejected game is left exactly as it was. Enqueued on the engine's stream;
 * the host does not wait. For the exact-leaf setting (below) the call counts as
 * a reset of the games it sets, one by one: it does not lift the restriction
 * on changing max_empties, which only a reset of all games lifts.
 * OAMD_INVALID_ARGUMENT: pos_dev NULL, history_k outside 0..15, history_dev
 * NULL with history_k > 0. */
int oamd_engine_set_positions(oamd_engine *e, const oamd_position *pos_dev, const oamd_position *history_dev,
                              int32_t history_k, const int32_t *hist_len_dev, const uint64_t *keys_dev,
                              const int32_t *ply_dev, const uint8_t *mask_dev, uint64_t seed, int32_t *status_dev);

/* The principal variation of every game's tree, read on the device after a
 * search: from the root, the child with the most visits (of equally visited
 * children the first in legal_actions() order, i.e. the lowest action), then
 * the same below that child, until a node has no children (unexpanded,
 * terminal, or an exact leaf), its best child has no visit, or max_len (1..64)
 * entries are written. Device outputs:
 *   pv_actions_dev (G, max_len) int32: the actions, -1 past the end;
 *   pv_visits_dev (G, max_len) int32 and pv_q_dev (G, max_len) fp32: N and Q
 *     of each chosen child, as oamd_engine_root_stats reports the children of
 *     the node they hang from (the same sign convention), 0 past the end;
 *   pv_len_dev (G) int32: the entries written; 0 for an inactive game.
 * Enqueued only; reads the trees, changes nothing.
 * OAMD_INVALID_ARGUMENT: max_len outside 1..64 or a NULL output. */
int oamd_engine_principal_variations(oamd_engine *e, int32_t max_len, int32_t *pv_actions_dev,
                                     int32_t *pv_visits_dev, float *pv_q_dev, int32_t *pv_len_dev);

/* ------------------------------------------------------------------------ */
/* Arena: G head-to-head matches between two nets, all on the device.        */
/* Replaces play_game between two AlphaZeroPlayers (player.py:33-95,         */
/* 177-259) as evaluation.py:15-90 runs it. Match g is game g of engine a     */
/* (searched with net A) and game g of engine b (net B): two trees, one per   */
/* player. Per ply only the side to move searches; the chosen action moves    */
/* both roots, so each side keeps its subtree across both sides' moves. A     */
/* forced pass is an ordinary ply (a one-child search, action 64).            */
/* Both engines: same device, same number of games, same stream; their        */
/* search configs may differ. OAMD_INVALID_ARGUMENT otherwise.                */
/* ------------------------------------------------------------------------ */

/* Reset both games of every match (random streams reseeded from each
 * engine's creation seed), play the opening plies in both trees, count plies
 * from 0 after the opening, and activate the side to move only (neither side
 * if the opening ended the game). openings_dev: (G, opening_plies) int32
 * actions, -1 = no more plies (an illegal ply ends that match's opening);
 * NULL or opening_plies = 0: none. a_is_white_dev: (G) bytes, nonzero = net A
 * plays white in that match; NULL = A plays black everywhere. */
int oamd_arena_begin(oamd_engine *a, oamd_engine *b, const int32_t *openings_dev, int32_t opening_plies,
                     const uint8_t *a_is_white_dev);
/* One ply of every match from the roots as searched: the mover's tree gives
 * the action (oamd_engine_selfplay_move's choice: temperature sampling while
 * the ply < cfg->temperature_moves, else argmax with a random tie-break; one
 * draw from the mover's game stream, none from the other side's), both roots
 * move, and the next side to move is activated. cfg->opening_moves and
 * cfg->emit_targets are ignored. Device outputs (may be NULL):
 *   actions_dev (G): the action, -1 once the match is over;
 *   finished_dev (G): UPDATED, never cleared (zero it before the first ply):
 *     bits 0-1 = 1 draw, 2 black won, 3 white won once the match has ended,
 *     bit 2 = a move came from an unexpanded root (uniform), bit 3 = a node
 *     pool overflowed, bit 4 = the two trees' roots differ (the match stops);
 *   discs_dev (G, 2): black and white discs, written when the match ends;
 *   remaining_dev (1): decremented for every match that ends. */
int oamd_arena_move(oamd_engine *a, oamd_engine *b, const oamd_selfplay_config *cfg, int32_t *actions_dev,
                    int32_t *finished_dev, int32_t *discs_dev, int32_t *remaining_dev);
/* Whole matches with native nets: per ply oamd_engine_search(a, net_a),
 * oamd_engine_search(b, net_b) and oamd_arena_move, enqueued without a host
 * wait in between; every 8 plies the number of running matches is read back
 * and the call returns when it is 0 or after max_plies plies. actions_dev
 * (max_plies, G), finished_dev (G) and discs_dev (G, 2) are required and
 * initialised by the call; *plies_host = plies enqueued. */
int oamd_arena_play(oamd_engine *a, oamd_net *net_a, oamd_engine *b, oamd_net *net_b,
                    const oamd_selfplay_config *cfg, int32_t max_plies, int32_t *actions_dev,
                    int32_t *finished_dev, int32_t *discs_dev, int32_t *plies_host);
/* The same with adjudication (the rule of
 * oamd_engine_selfplay_move_adjudicated; max_empties = 0 is the call above).
 * An adjudicated match stops: finished bit 5 is set with the outcome bits of
 * the exact margin, neither tree stays active, remaining is decremented once,
 * later plies report action -1, and discs_dev holds the disc counts AT the
 * adjudicated position. margin_dev (G, may be NULL): the exact margin seen
 * from black, black minus white for a match that ended on the board.
 * oamd_arena_move_adjudicated writes margin_dev only for matches that end at
 * this ply; oamd_arena_play_adjudicated writes all G entries, INT32_MIN for a
 * match that did not end in the call. finished_dev is required when
 * max_empties > 0. */
int oamd_arena_move_adjudicated(oamd_engine *a, oamd_engine *b, const oamd_selfplay_config *cfg,
                                int32_t *actions_dev, int32_t *finished_dev, int32_t *discs_dev,
                                int32_t *remaining_dev, int32_t max_empties, int32_t split, int32_t *margin_dev);
int oamd_arena_play_adjudicated(oamd_engine *a, oamd_net *net_a, oamd_engine *b, oamd_net *net_b,
                                const oamd_selfplay_config *cfg, int32_t max_plies, int32_t *actions_dev,
                                int32_t *finished_dev, int32_t *discs_dev, int32_t *plies_host,
                                int32_t max_empties, int32_t split, int32_t *margin_dev);

/* ------------------------------------------------------------------------ */
/* Packed replay buffer: a ring of POSITIONS (2H bitboards, the side to move, */
/* one 65-entry policy, one value: 16H + 265 bytes) instead of 8 fp32 samples */
/* per position; the 8 board symmetries are produced when a minibatch is      */
/* gathered. Replaces the sample lists of train.py:432-452 (_self_play's      */
/* value assignment) and the per-minibatch indexing of train.py:487-489.      */
/* The caller owns every buffer (the Python layer keeps them as torch         */
/* tensors); the struct below only points at them.                            */
/* ------------------------------------------------------------------------ */

/* sticky bits of counters[3]: rows the add / gather kernels refused */
#define OAMD_REPLAY_OVERFLOW 1   /* finished bit 3: the game's node pool overflowed */
#define OAMD_REPLAY_NO_TARGETS 2 /* finished bit 2 on a played game: no targets were written */
#define OAMD_REPLAY_TOO_LONG 4   /* a game staged more than max_moves moves */
#define OAMD_REPLAY_BAD_ID 8     /* a gather id outside [0, 8 * size) */
#define OAMD_REPLAY_SOLVER_FLAG 16 /* finished bit 6: the solver flagged an adjudicated position */

typedef struct oamd_replay_view {
    int32_t device;       /* HIP device of every pointer below */
    int32_t num_games;    /* G >= 1 */
    int32_t history_size; /* H in [1, 15] */
    int32_t max_moves;    /* staged moves per game, >= 1; G * max_moves < 2^31 */
    int64_t capacity;     /* ring length in positions, >= 1 */
    /* ring, structure of arrays */
    uint64_t *boards; /* (capacity, 2H): planes 1..2H of the untransformed sample, square i = bit 63 - i */
    float *policy;    /* (capacity, 65): the transform-0 policy */
    float *value;     /* (capacity) */
    uint8_t *player;  /* (capacity): plane 0 (0 black to move, 1 white) */
    /* staging: the moves of the games still running */
    uint64_t *stage_boards; /* (G, max_moves, 2H) */
    float *stage_policy;    /* (G, max_moves, 65) */
    uint8_t *stage_player;  /* (G, max_moves) */
    int32_t *moves;         /* (G) staged moves per game */
    int32_t *pending;       /* (G) scratch of the add call */
    /* [0] head (next slot written), [1] size (live positions), [2] games
     * completed, [3] sticky OAMD_REPLAY_* bits; zero-initialised by the caller */
    int64_t *counters;
} oamd_replay_view;

/* One or n_moves moves of every game, as oamd_engine_selfplay_move /
 * oamd_engine_selfplay_steps (emit_targets = 1) wrote them: actions_dev (G),
 * finished_dev (G), features_dev (G, 8, 1+2H, 8, 8), policy_dev (G, 8, 65);
 * n_moves > 1: the stacked per_move_outputs = 1 layout, slices handled in
 * order. Only the transform-0 slice is read. Per move: every game with
 * actions >= 0 stages one record; then the games whose finished bits 0-1 are
 * set move to the ring in ascending game order with their value targets (the
 * outcome for black, negated where white was to move), oldest positions
 * overwritten. A row with finished bit 3, with bit 2 on a played game, or of
 * a game already holding max_moves moves sets its sticky bit instead and is
 * skipped (a game that finished in such a row is dropped). A row with
 * finished bit 6 (an adjudicated game without an outcome) sets
 * OAMD_REPLAY_SOLVER_FLAG and drops the game's staged moves. Enqueued only. */
int oamd_replay_add(const oamd_replay_view *view, int32_t n_moves, const int32_t *actions_dev,
                    const int32_t *finished_dev, const float *features_dev, const float *policy_dev,
                    void *stream);
/* ids_dev (n) int64: id s = position s >> 3 (counted from the oldest live
 * position) under board transform s & 7 (transformation.h:40-57). Outputs:
 * features_dev (n, 1+2H, 8, 8), policy_dev (n, 65), value_dev (n) fp32. An id
 * outside [0, 8 * size) gives a zero row and sets OAMD_REPLAY_BAD_ID.
 * Enqueued only. */
int oamd_replay_gather(const oamd_replay_view *view, const int64_t *ids_dev, int64_t n, float *features_dev,
                       float *policy_dev, float *value_dev, void *stream);
/* Host outputs (each may be NULL); waits for the stream. */
int oamd_replay_counters(const oamd_replay_view *view, int64_t *size, int64_t *head, int64_t *games_completed,
                         int32_t *flags, void *stream);

/* Exact endgame value targets (optional). The caller keeps one more ring
 * array beside the view, exact_dev (capacity) int8, initialised to
 * OAMD_REPLAY_EXACT_UNKNOWN, and feeds the ring with oamd_replay_add_tracked.
 * A slot's byte says where its value comes from: */
#define OAMD_REPLAY_EXACT_UNKNOWN (-128) /* the game's outcome; not examined yet */
#define OAMD_REPLAY_EXACT_GAVE_UP (-127) /* examined, not solved (node limit, invalid record): the game's */
/* -64..64: the exact disc difference at the end of perfect play for the side
 * to move in that record; the slot's value is its sign (-1, 0, +1). */
#define OAMD_REPLAY_POLICY_KEEP 0    /* policy_mode: leave the policy row alone */
#define OAMD_REPLAY_POLICY_OPTIMAL 1 /* 1/m on the m actions whose move_scores equal score, pass included */

/* oamd_replay_add, and every ring slot it writes also gets
 * exact_dev[slot] = OAMD_REPLAY_EXACT_UNKNOWN (same kernel, same lane). */
int oamd_replay_add_tracked(const oamd_replay_view *view, int8_t *exact_dev, int32_t n_moves,
                            const int32_t *actions_dev, const int32_t *finished_dev, const float *features_dev,
                            const float *policy_dev, void *stream);
/* bytes of the caller-owned workspace of a relabel call; budget in [1, 2^20] */
int oamd_replay_relabel_workspace_bytes(int64_t budget, int64_t *bytes);
/* Replace game outcomes by exact results where the solver reaches. Live
 * positions are numbered from the oldest; a candidate has exact ==
 * OAMD_REPLAY_EXACT_UNKNOWN (or OAMD_REPLAY_EXACT_GAVE_UP when retry != 0) and
 * at most max_empties empty squares in history step 0. The first `budget`
 * candidates are solved as {player + 1, boards[0], boards[1]} by
 * oamd_solve_endgames with max_empties and node_limit. No flag: exact = the
 * score for the mover (a terminal root's black-minus-white is negated for
 * white), value = its sign, and with OAMD_REPLAY_POLICY_OPTIMAL a root with
 * actions gets the optimal policy (transform-0 coordinates). Any flag: exact
 * = OAMD_REPLAY_EXACT_GAVE_UP, value and policy untouched.
 * relabel_counters_dev (4) int64, zero-initialised by the caller: [0]
 * positions labelled so far, [1] positions given up so far, [2] candidates
 * this call left behind for lack of budget, [3] candidates it took.
 * Enqueued only; allocates nothing. */
int oamd_replay_relabel_endgames(const oamd_replay_view *view, int8_t *exact_dev, int64_t *relabel_counters_dev,
                                 int32_t max_empties, int64_t budget, int64_t node_limit, int32_t policy_mode,
                                 int32_t retry, void *workspace_dev, void *stream);

/* ------------------------------------------------------------------------ */
/* Exact endgame solver: the last plies solved by brute force on bitboards.  */
/* Stands in for the external engine behind the reference's EgaroucidPlayer  */
/* (player.py:262-321) as a yardstick of correct play. The game ends when     */
/* neither side can move; the result is the plain disc difference (mover      */
/* minus opponent, no bonus for empties: play_game, player.py:83-92).         */
/* move_scores[a], for every legal action a of the position (0..63, or 64     */
/* when the mover must pass), is the exact result for the side to move after  */
/* a and perfect play by both; every other entry is OAMD_SOLVE_NONE. score =  */
/* the maximum, best_action = its first index. A position where neither side  */
/* can move is terminal whatever `player` says: score = black minus white,    */
/* best_action = -1. legal_moves / next_legal_moves are ignored.              */
/* ------------------------------------------------------------------------ */
#define OAMD_SOLVE_NONE (-128)
/* per-position flags; a flagged position has score -128, best_action -1 */
#define OAMD_SOLVE_TOO_MANY_EMPTIES 1 /* more than max_empties empties: not searched */
#define OAMD_SOLVE_NODE_LIMIT 2       /* a root action visited more than node_limit positions */
#define OAMD_SOLVE_INVALID 4          /* overlapping discs, player outside 0..2, or 0 while a side can move */

/* bytes of the caller-owned workspace for n positions */
int oamd_solve_workspace_bytes(int64_t n, int64_t *bytes);
/* n positions on `device`; outputs (device, each may be NULL except move_scores):
 * move_scores_dev (n, 65) int32, score_dev (n) int32, best_action_dev (n) int32,
 * flags_dev (n) int32, nodes_dev (n) int64 (positions visited, summed over the
 * root actions; the same count as the host solver's). max_empties in [0, 16];
 * node_limit >= 1 is a budget per root action. workspace: caller-owned, size
 * from oamd_solve_workspace_bytes(n). Enqueued only. */
int oamd_solve_endgames(int32_t device, const oamd_position *pos_dev, int64_t n, int32_t max_empties,
                        int64_t node_limit, int32_t *move_scores_dev, int32_t *score_dev,
                        int32_t *best_action_dev, int32_t *flags_dev, int64_t *nodes_dev,
                        void *workspace_dev, void *stream);
/* The same solver on the host for one position (scalar form, like
 * oamd_host_legal_moves; same source, csrc/solver.h). move_scores65 is
 * required, the other outputs may be NULL. */
int oamd_host_solve_endgame(const oamd_position *pos_host, int32_t max_empties, int64_t node_limit,
                            int32_t *move_scores65, int32_t *score, int32_t *best_action,
                            int32_t *flags, int64_t *nodes);

/* The split solver (opt-in): the same positions, outputs, flags and limits
 * checks, another algorithm. The work item is one move of the position R one
 * ply below a root action a (Q = the position after a; R = Q, or Q after a
 * pass when Q's mover has none), searched with fastest-first move ordering at
 * nodes with at least 6 empties. Phase A searches one move of R exactly,
 * phase B the others in parallel with its value as the lower bound; two item
 * launches between a planning and a reducing kernel. Scores, best_action and
 * flags equal oamd_solve_endgames' wherever no node limit binds. nodes differ:
 * per root action 1 for Q, 1 more when Q's mover passes, plus the positions
 * its items visited; node_limit is a budget per item, and a root action with
 * an item over it gets OAMD_SOLVE_NONE and flags the position. The workspace
 * is the caller's, oamd_solve_split_workspace_bytes(n). Enqueued only. */
int oamd_solve_split_workspace_bytes(int64_t n, int64_t *bytes);
int oamd_solve_endgames_split(int32_t device, const oamd_position *pos_dev, int64_t n, int32_t max_empties,
                              int64_t node_limit, int32_t *move_scores_dev, int32_t *score_dev,
                              int32_t *best_action_dev, int32_t *flags_dev, int64_t *nodes_dev,
                              void *workspace_dev, void *stream);
/* The split solver on the host for one position: the same source, the same
 * outputs and node counts as the device. */
int oamd_host_solve_endgame_split(const oamd_position *pos_host, int32_t max_empties, int64_t node_limit,
                                  int32_t *move_scores65, int32_t *score, int32_t *best_action,
                                  int32_t *flags, int64_t *nodes);
/* oamd_replay_relabel_endgames with the split solver between the same list
 * and apply kernels; workspace from oamd_replay_relabel_split_workspace_bytes. */
int oamd_replay_relabel_split_workspace_bytes(int64_t budget, int64_t *bytes);
int oamd_replay_relabel_endgames_split(const oamd_replay_view *view, int8_t *exact_dev,
                                       int64_t *relabel_counters_dev, int32_t max_empties, int64_t budget,
                                       int64_t node_limit, int32_t policy_mode, int32_t retry, void *workspace_dev,
                                       void *stream);

/* ------------------------------------------------------------------------ */
/* Baseline opponents: fixed classical players for the whole */
/* game, in place of the reference's RandomPlayer, GreedyPlayer and          */
/* EgaroucidPlayer (player.py:121-175, 262-321). A baseline gives every root */
/* action of a position (0..63, or 64 when the mover must pass) one int32    */
/* score for the side to move and picks one action with the maximal score.   */
/*   RANDOM  every action scores 0                                            */
/*   GREEDY  a square scores the discs it flips, the pass 0                   */
/*   SEARCH  the exact negamax value `depth` disc placements deep (a pass     */
/*           consumes none). A game that is over is worth 4096 sgn(d) + d, d  */
/*           = mover's discs minus the other side's; a position at depth 0 is */
/*           worth 10 (mobility) + 50 (corners) - 20 (X-squares beside an     */
/*           empty corner) + discs, each as mover minus other side, |.| <     */
/*           1000. With depth >= empties the scores are the exact solver's.   */
/* Every move_scores entry that is no legal root action is                    */
/* OAMD_BASELINE_NONE. score = the maximum; action = the lowest action with   */
/* that score, or with a key the k-th lowest of the nt tied ones, k =         */
/* min(nt - 1, (int)(u * nt)), u the first uniform of the random stream       */
/* (key, event, 0): the argmax rule of the self-play move. A position where   */
/* neither side can move has no action: every score OAMD_BASELINE_NONE,       */
/* action -1, flags 0. A flagged position (OAMD_SOLVE_INVALID, or             */
/* OAMD_SOLVE_NODE_LIMIT when a root action visited more than node_limit      */
/* nodes) has the same outputs with its flags. nodes = positions visited      */
/* plus static evaluations, summed over the root actions; 0 for RANDOM and    */
/* GREEDY. legal_moves / next_legal_moves are ignored.                        */
/* ------------------------------------------------------------------------ */
#define OAMD_BASELINE_NONE INT32_MIN
#define OAMD_BASELINE_RANDOM 0
#define OAMD_BASELINE_GREEDY 1
#define OAMD_BASELINE_SEARCH 2 /* depth in 1..10 */

/* bytes of the caller-owned workspace for n positions */
int oamd_baseline_workspace_bytes(int64_t n, int64_t *bytes);
/* n positions on `device`. keys_dev / events_dev: (n) int64 each, or NULL (no
 * keys: the lowest tied action; keys without events: event 0). Outputs
 * (device, all required): move_scores_dev (n, 65) int32, score_dev, action_dev,
 * flags_dev (n) int32, nodes_dev (n) int64. depth is read for SEARCH only;
 * node_limit >= 1 is a budget per root action. workspace: caller-owned, size
 * from oamd_baseline_workspace_bytes(n). workgroups = 0: a chip-filling grid;
 * >= 1: that many 64-lane workgroups (no output depends on it). Enqueued
 * only: allocates nothing, waits for nothing. */
int oamd_baseline_moves(int32_t device, const oamd_position *pos_dev, int64_t n, int32_t kind, int32_t depth,
                        int64_t node_limit, const int64_t *keys_dev, const int64_t *events_dev,
                        int32_t *move_scores_dev, int32_t *score_dev, int32_t *action_dev, int32_t *flags_dev,
                        int64_t *nodes_dev, void *workspace_dev, int32_t workgroups, void *stream);
/* The same code on the host for one position (csrc/baseline.h). has_key = 0:
 * key and event are ignored. Every output is required. */
int oamd_host_baseline_move(const oamd_position *pos_host, int32_t kind, int32_t depth, int64_t node_limit,
                            int32_t has_key, uint64_t key, uint64_t event, int32_t *move_scores65, int32_t *score,
                            int32_t *action, int32_t *flags, int64_t *nodes);

/* ------------------------------------------------------------------------ */
/* Exact leaf values (opt-in, off by default): the search     */
/* solves leaves with few empties instead of asking the net.                 */
/* ------------------------------------------------------------------------ */
/* With max_empties = E in 1..10, wherever the search runs (the step API and
 * the native schedules):
 *  - a child created by an expansion that is not terminal and has at most E
 *    empties is an exact leaf. It is never expanded and never evaluated;
 *  - a node that becomes a game's root (a self-play move, oamd_engine_apply_
 *    action(s), a restart or reset) loses the mark: the root is an ordinary
 *    leaf that the net evaluates and expands;
 *  - a descent that ends at an exact leaf is handled like one ending at a
 *    terminal leaf: no NN row (oamd_engine_leaf_flags reports 0), no random
 *    event, not an evaluation. The first visit solves the leaf with the
 *    endgame solver's state machine, s = the sign of the exact disc difference
 *    for the leaf's side to move under best play; the backup gives every node
 *    on the path what a terminal leaf whose score for the parent's player is
 *    -s would give, and the leaf keeps s for every later visit;
 *  - a batch needs the evaluation round trip if it holds an NN row or a leaf
 *    that is not solved yet; terminal and solved leaves alone are backed up
 *    at once, as all-terminal batches are.
 * One game with num_threads > 1 runs on the grouped schedule instead of the
 * thread-split one (same results). E = 0 is off: no mark is ever written and
 * nothing is launched, the engine is bit for bit the engine without the
 * setting. The value may change only while no game holds a tree built under
 * another value, i.e. before the first search or after oamd_engine_reset of
 * all games (game = -1) or oamd_engine_random_openings: OAMD_INVALID_ARGUMENT
 * otherwise, and for E outside 0..10. oamd_engine_set_positions counts as a
 * reset of each game it sets, like oamd_engine_reset with game >= 0: the host
 * does not learn which games were rejected, so it never lifts the restriction. Independent of the playout cap, forced
 * playouts and adjudication. The arena rejects an engine that has it. */
int oamd_engine_set_exact_leaves(oamd_engine *e, int32_t max_empties);
/* Since the engine was created (host outputs; waits for the engine's stream):
 * solves = rows that ended at a leaf not solved yet (each is solved, also two
 * rows at the same leaf in one round), hits = rows that ended at a solved
 * leaf, nodes = positions the solves visited. */
int oamd_engine_exact_leaf_counters(oamd_engine *e, int64_t *solves, int64_t *hits, int64_t *nodes);
/* Rows that were backed up while their exact leaf had no result (host output;
 * waits for the engine's stream): the solve kernel was not enqueued between
 * the row's selection and its backup, or could not take the row. Such a row
 * backs up a draw. Always 0 unless the host layer or the tree is broken; the
 * Python layer's check_health raises on it. */
int oamd_engine_exact_leaf_faults(oamd_engine *e, int64_t *faults);
/* The rule on the host: *sign_or_none = s (-1, 0, +1) when the position would
 * be an exact leaf at max_empties (1..10): not terminal and at most that many
 * empties; OAMD_SOLVE_NONE otherwise (a position where neither side can move
 * is terminal whatever `player` says). legal_moves / next_legal_moves are
 * ignored. Every root action (the pass when the mover has no move) is searched
 * with the window [-1, 1]. */
int oamd_exact_leaf_sign(const oamd_position *pos_host, int32_t max_empties, int32_t *sign_or_none);
/* The solve kernel's path over n positions on the device: sign_dev (n) as
 * above, nodes_dev (n, may be NULL). Enqueued only. */
int oamd_exact_leaf_signs(int32_t device, const oamd_position *pos_dev, int64_t n, int32_t max_empties,
                          int32_t *sign_dev, int64_t *nodes_dev, void *stream);

/* Timing accumulated over the timed oamd_engine_search calls (HIP events on
 * the launching streams; a query waits for the searches still in flight):
 * total ms spent in the NN kernel, number of NN launches, rows launched
 * (terminal leaves included; oamd_engine_work_counters gives the rows that
 * needed an evaluation). */
int oamd_engine_nn_timing(const oamd_engine *e, float *nn_ms, int64_t *launches, int64_t *rows);
/* Busy time of the ResNet kernel: while timing is enabled, every ResNet
 * launch of a native search (all searches, all rounds, the chain-splitting
 * extra rounds included) records its execution interval in the kernel (first
 * workgroup start to last workgroup end, s_memrealtime); busy_ms is the union
 * of those intervals since timing was last enabled (ms some ResNet launch was
 * running; launches of different NN chains and pipeline groups overlap),
 * launches their count. The rows they evaluated are the difference of
 * oamd_engine_work_counters over the same window, so evals x FLOPs per row /
 * busy is the delivered rate. Waits for the device. */
int oamd_engine_nn_busy(const oamd_engine *e, float *busy_ms, int64_t *launches);
/* Same for the tree kernel (k_tree, one launch per search round and pipeline
 * group): select_ms = total ms of the rounds that select (each also backs up
 * the previous batch, thread by thread), backup_ms = total ms of the final
 * backup-only rounds (one per search and pipeline group). launches = timed
 * select rounds (k_tree launches: rounds x pipeline groups). Timed searches
 * record 4 HIP events per round and pipeline group on the group's stream. */
int oamd_engine_tree_timing(const oamd_engine *e, float *select_ms, float *backup_ms, int64_t *launches);
/* enable: 0 off, 1 time every search, N >= 2 time every N-th search (sampled:
 * a timed search's event packets lengthen the gaps between its launches).
 * The ResNet busy-time window (oamd_engine_nn_busy) restarts here and covers
 * every search while enable != 0; restarting waits for the device. */
int oamd_engine_enable_timing(oamd_engine *e, int32_t enable);

#ifdef __cplusplus
}
#endif

#endif /* OTHELLO_MCTS_AMD_H */
