// Positions handed to the engine from outside: the canonical
// form of a position and the faults oamd_engine_set_positions reports. Written
// once for the device (positions.hip k_set_positions) and the host
// (oamd_host_canonical_position), like the bitboards it is built from.
#pragma once

#include <stdint.h>

#include "../../include/othello_mcts_amd.h"
#include "bitboard.h"

namespace oamd {

// status[g] of oamd_engine_set_positions: 0 accepted, -1 not selected, else the
// first fault found (the root's before the history's)
constexpr int32_t kSetPosOk = OAMD_SET_POSITIONS_OK;
constexpr int32_t kSetPosSkipped = OAMD_SET_POSITIONS_SKIPPED;
constexpr int32_t kSetPosBadPlayer = OAMD_SET_POSITIONS_BAD_PLAYER;
constexpr int32_t kSetPosOverlap = OAMD_SET_POSITIONS_OVERLAP;
constexpr int32_t kSetPosHistBadPlayer = OAMD_SET_POSITIONS_HISTORY_BAD_PLAYER;
constexpr int32_t kSetPosHistOverlap = OAMD_SET_POSITIONS_HISTORY_OVERLAP;
constexpr int32_t kSetPosBadHistLen = OAMD_SET_POSITIONS_BAD_HIST_LEN;
constexpr int32_t kSetPosBadPly = OAMD_SET_POSITIONS_BAD_PLY;
constexpr int32_t kSetPosCapacity = OAMD_SET_POSITIONS_CAPACITY;

// The fault of (player, p1, p2) as a root: 0 none.
OAMD_HD int32_t position_fault(int32_t player, uint64_t p1, uint64_t p2) {
    if (player < 0 || player > 2) return kSetPosBadPlayer;
    if (p1 & p2) return kSetPosOverlap;
    return kSetPosOk;
}

// Canonical form: what Position::apply_action would have left for these discs
// and this side to move. Reads player, p1 and p2 only. A side to move without
// a move keeps the move when the opponent has one (a pass position: legal = 0,
// next_legal = the opponent's moves); when neither side has one the position
// is terminal (player 0), and a terminal position carries no moves. The input
// must be free of faults (position_fault).
OAMD_HD Pos canonical_position(int32_t player, uint64_t p1, uint64_t p2) {
    Pos c;
    c.player = player;
    c.pad_ = 0;
    c.p1 = p1;
    c.p2 = p2;
    c.legal = 0;
    c.next_legal = 0;
    if (player == 0) return c;
    const uint64_t me = player == 1 ? p1 : p2, opp = player == 1 ? p2 : p1;
    c.legal = legal_moves(me, opp);
    if (c.legal == 0) {
        c.next_legal = legal_moves(opp, me);
        if (c.next_legal == 0) c.player = 0;
    }
    return c;
}

}  // namespace oamd
