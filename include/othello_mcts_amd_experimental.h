/*
 * othello_mcts_amd_experimental.h — scheduling knobs and diagnostics of the
 * native engine, outside the product ABI (othello_mcts_amd.h).
 *
 * The product defaults (2 pipeline groups from 64 games, 2 NN chains, chain
 * budget 2 with up to 64 cuts, adaptive extra rounds with minimum 1, a
 * 128-workgroup grid for the extra rounds) were measured in DESIGN.md §7 and
 * need no setting. These setters exist for A/B measurements
 * (bench.py flags, tools/); none of them changes a result — every search
 * output is identical for every setting (tests/test_gpu_configs.py,
 * tests/test_gpu_resnet.py). The debug readers work only in diagnostic builds.
 * Not part of the reference's interface: nothing in othello_mcts.cpp:49-151
 * corresponds to them.
 */
#ifndef OTHELLO_MCTS_AMD_EXPERIMENTAL_H
#define OTHELLO_MCTS_AMD_EXPERIMENTAL_H

#include "othello_mcts_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Split the games into `groups` pipeline groups (own HIP streams) so that tree
 * kernels of one group overlap the NN launch of another (0 = auto: 2 groups
 * from 64 games, else 1; at most 8). Results do not depend on it. */
int oamd_engine_set_pipeline(oamd_engine *e, int32_t groups);
/* The pipeline groups' ResNet launches form `chains` chains (group k in chain
 * k % chains, 1..4, default 2): launches of one chain run one after another,
 * chains run concurrently (the default lets the two groups' launches overlap
 * at their ends). Results do not depend on it. */
int oamd_engine_set_nn_chains(oamd_engine *e, int32_t chains);
/* Native search with the exact interleaving: a virtual thread whose batches
 * come back all terminal selects again at once (search_thread.cpp:102-127),
 * which near a game's end can run a thread's whole remaining search inside one
 * round and hold its pipeline group's ResNet launch. After `budget`
 * re-selections in a round such a chain stops and the game's next round
 * resumes it exactly there (every game keeps its order of operations; only
 * round boundaries move), at most `cuts` times per search, at the cost of
 * up to `cuts` extra rounds per search (see the adaptive count below; never
 * more than T x steps / budget, the most cuts one game's search can use).
 * Default budget 2, cuts 64; budget 0 = never split. Results do not depend on
 * it. */
int oamd_engine_set_chain_split(oamd_engine *e, int32_t budget, int32_t cuts);
/* Adaptive extra rounds (default on, min_rounds 1): a grouped native search
 * runs X extra rounds and allows X cuts per game, X in [min(min_rounds,
 * cuts), cuts], following the search two back (read back without draining
 * the queue; the first two searches run min_rounds): X = cuts when some
 * root of that search was within 12 empty squares of the end (the endgame,
 * where all-terminal chains appear), else
 * the most cuts u any game used + min_rounds (2X + 2 + min_rounds when a
 * game ran out of cuts). Extra rounds past every game's last cut are empty
 * launches; a game that would need more cuts runs its last chain uncut.
 * enable = 0: X = cuts always. Scheduling only: results are identical.
 * (The rule is AdaptiveRounds in csrc/schedule.h. A search that used cuts
 * also raises the 12 to its fewest empties + 3 before the comparison, so it
 * counts as endgame itself; the threshold then falls by one per search
 * without cuts, back to 12.) */
int oamd_engine_set_adaptive_extra_rounds(oamd_engine *e, int32_t enable, int32_t min_rounds);
/* Workgroups of the chain-splitting extra rounds' ResNet launches (default
 * 128; 0 = the regular grid, the list's capacity): those launches hold the
 * rows of lagging games only (none outside endgames), so a small grid loops
 * over them instead of dispatching ~1000 mostly empty workgroups between the
 * other NN chain's. Scheduling only: results are identical. */
int oamd_engine_set_extra_round_grid(oamd_engine *e, int32_t workgroups);
/* Process-wide: which geometry of the fused ResNet kernel evaluates C=128
 * launches of 1024 rows or more. enable != 0: 4 waves per workgroup, one per
 * SIMD, each owning 32 channels x the 256 positions of the workgroup's 4
 * boards, weight fragments queued in registers straight from L2
 * (k_resnet_w4); 0: 8 waves of 32 channels x 128 positions fed from the LDS
 * weight ring (k_resnet_w8). Takes effect at the next launch, for every net
 * and engine of the process. Results do not depend on it, bit for bit.
 * oamd_resnet_c128_four_wave returns the current setting (1 / 0). */
int oamd_set_resnet_c128_four_wave(int32_t enable);
int oamd_resnet_c128_four_wave(void);
/* Diagnostics: copy the ResNet kernel's per-workgroup time stamps and cycle
 * sums (24 u64 per workgroup, resnet.hip kStampStride; see tools/nn_stamps.py)
 * of the last launch. Only in builds with OAMD_EXTRA_FLAGS=-DOAMD_STAMPS;
 * otherwise OAMD_INVALID_ARGUMENT. */
int oamd_debug_read_stamps(uint64_t *out, int64_t n);
/* Diagnostics: the engine keeps 16 guard words behind its policy and its value
 * buffer (the outputs of the native search's ResNet launches); *intact = 1
 * while no launch has written any of them (waits for the device). */
int oamd_debug_eval_guards(oamd_engine *e, int32_t *intact);
/* Diagnostics, for tests/test_gpu_resnet_packed.py: the native search's ResNet
 * launch (bit-packed feature rows read through an evaluation list) on the
 * caller's rows. feat_dev: feat_rows rows of 2 + 2 * history words (history in
 * [1, 15], the net's in_channels = 1 + 2 * history), in the engine's layout:
 * word 0 = meta (bit 0 the player plane, bits 8-10 the board symmetry, bit 16
 * valid; an invalid row is evaluated as an all-zero board, or not at all when
 * every row of its workgroup is invalid), word 1 = 0, words 2 + 2h / 3 + 2h
 * the two disc sets of position h. policy_dev / value_dev: out_rows rows of 65
 * floats / out_rows floats; launch entry i writes row list[i] of both.
 * list_host = NULL (list_len = list_off = 0, count ignored): the dense launch
 * of rows 0 .. rows-1. Otherwise list_host holds list_len row indices and the
 * launch is the engine's: entries list_off .. list_off + rows - 1 of the list,
 * of which those below `count` (the list's filled entries, counted from entry
 * 0) are evaluated. The list and the count are copied into device memory the
 * net owns. max_wgs > 0 caps the grid: the workgroups loop over the board
 * groups (the extra rounds' launch); 0 = one workgroup per board group.
 * Nothing is launched (OAMD_INVALID_ARGUMENT) unless history, the net's
 * in_channels and the sizes agree, rows >= 0, count >= 0, max_wgs >= 0,
 * list_off >= 0 and list_off + rows <= list_len, every list entry (dense:
 * every row below `rows`) is in [0, min(feat_rows, out_rows)), and the
 * buffers a launch would touch are not NULL. Waits for the device before it
 * replaces the list of the previous call; the launch itself is asynchronous
 * on `stream`. */
int oamd_debug_forward_packed(oamd_net *net, const uint64_t *feat_dev, int64_t feat_rows, int32_t history,
                              const int32_t *list_host, int32_t list_len, int32_t count, int32_t list_off,
                              int32_t rows, int32_t max_wgs, float *policy_dev, float *value_dev, int64_t out_rows,
                              void *stream);
/* Diagnostics: copy the engine's packed feature rows (num_games x num_threads
 * x batch_size rows of 2 + 2 * history_size words, as the last select left
 * them) into out_dev, which holds `words` words: exactly that many, else
 * OAMD_INVALID_ARGUMENT. Waits for the engine's stream. */
int oamd_debug_engine_feature_rows(oamd_engine *e, uint64_t *out_dev, int64_t words);
/* Diagnostics: k_tree's phase cycle sums over every wave since the last reset
 * (tools/tree_stamps.py); reset != 0 zeroes them after the copy. Only in
 * builds with OAMD_EXTRA_FLAGS=-DOAMD_TREE_STAMPS; otherwise
 * OAMD_INVALID_ARGUMENT. */
int oamd_debug_tree_stamps(uint64_t *out, int64_t n, int32_t reset);

/* Free-running self-play in oamd_engine_selfplay_steps (default on): every
 * game plays its moves on its own — the round that completes a game's search
 * also runs its move and its next search's first round — so no game waits at
 * a move for the group's slowest one, and no extra rounds are run. Per game
 * the operations and their order are those of n x (oamd_engine_search +
 * oamd_engine_selfplay_move), and every output is identical; enable = 0 gives
 * the lock-step multi-move call (searches with chain-splitting extra rounds).
 * One game with num_threads > 1 (the thread-split schedule) is always
 * lock-step. */
int oamd_engine_set_free_running(oamd_engine *e, int32_t enable);

/* Diagnostics: the tree kernels' algorithmic work since the engine was
 * created (host outputs; waits for the engine's stream), the terms of the
 * byte model of SURVEY.md §8(d) that bench.py prices per k_tree launch:
 * descent levels (= the depth sum of oamd_engine_descent_depths), children
 * whose statistics those levels scanned, expansions, children created, and
 * tree kernel launches (k_tree, k_tree_wide, k_tree_free). Any pointer may be
 * NULL. */
int oamd_engine_tree_work(oamd_engine *e, int64_t *levels, int64_t *children_scanned, int64_t *expansions,
                          int64_t *children_created, int64_t *launches);

/* oamd_solve_endgames with an explicit number of 64-lane workgroups (>= 1)
 * instead of the chip-filling default: one workgroup pushes every item through
 * 64 lanes, each taking the next item when its own is done. Scores, flags and
 * node counts do not depend on it. */
int oamd_solve_endgames_grid(int32_t device, const oamd_position *pos_dev, int64_t n, int32_t max_empties,
                             int64_t node_limit, int32_t *move_scores_dev, int32_t *score_dev,
                             int32_t *best_action_dev, int32_t *flags_dev, int64_t *nodes_dev,
                             void *workspace_dev, int32_t workgroups, void *stream);
/* The same for oamd_solve_endgames_split: both item launches use that grid. */
int oamd_solve_endgames_split_grid(int32_t device, const oamd_position *pos_dev, int64_t n, int32_t max_empties,
                                   int64_t node_limit, int32_t *move_scores_dev, int32_t *score_dev,
                                   int32_t *best_action_dev, int32_t *flags_dev, int64_t *nodes_dev,
                                   void *workspace_dev, int32_t workgroups, void *stream);

/* Diagnostics: device time (HIP events) of the engine's last adjudication
 * resolve step (solver + apply, oamd_engine_*_adjudicated / oamd_arena_*_adjudicated
 * with max_empties > 0) and the number of resolve steps enqueued so far
 * (resolves may be NULL). The first call switches the recording on: resolve
 * steps enqueued before it are not timed (0 ms). Waits for the timed step. */
int oamd_engine_adjudicate_ms(oamd_engine *e, float *ms, int64_t *resolves);

/* oamd_exact_leaf_sign that also returns the positions the solve visited: the
 * figure the device adds to the engine's solver-node counter for that leaf
 * (oamd_engine_exact_leaf_counters). For tests and reports that account for
 * the counters; nodes may be NULL. */
int oamd_exact_leaf_sign_nodes(const oamd_position *pos_host, int32_t max_empties, int32_t *sign_or_none,
                               int64_t *nodes);

#ifdef __cplusplus
}
#endif

#endif /* OTHELLO_MCTS_AMD_EXPERIMENTAL_H */
