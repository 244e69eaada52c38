"""The reference arena match on the CPU, for tests/test_cpu_arena.py and
tests/test_gpu_arena.py.

One match = two oracle searches (oracle.OracleMCTS), one per player, as the
reference's two AlphaZeroPlayers each own an MCTS (player.py:177-259), driven
by play_game's loop (player.py:33-95) in this file's own words: while the
position is not terminal, the side to move searches its own tree with its own
evaluator and chooses; the action is applied to both trees. The choice is the
on-device driver's (OracleMCTS.selfplay_action: argmax of the root visits with
a random tie-break drawn from the mover's game stream, temperature sampling
for the first plies), with the ply counted from the end of the opening.
"""

from __future__ import annotations

import numpy as np

import oracle as O

SETUP = dict(history_size=3, num_simulations=64, num_threads=2, batch_size=8, dirichlet_epsilon=0.0)
MATCHES = 8
OPENING_PLIES = 4


def mix64(z: int) -> int:
    return int(O.lib().orc_mix64(z & 0xFFFFFFFFFFFFFFFF))


def game_key(seed: int, g: int) -> int:
    """Random-stream key of game g of an engine created with `seed` (DESIGN.md "Random streams")."""
    return mix64(seed ^ mix64(g + 0x632BE59BD9B4E019))


def stub_a(features: np.ndarray):
    return O.equivariant_stub(features)


def stub_b(features: np.ndarray):
    """oracle.equivariant_stub with the channel weights reversed and value tanh(-sq.mean)."""
    import torch

    x = torch.from_numpy(np.ascontiguousarray(features))
    C = x.shape[1]
    w = torch.linspace(1, -1, C)
    sq = (x * w.view(1, C, 1, 1)).sum(dim=1).flatten(1)
    logits = torch.cat([sq, torch.full((x.shape[0], 1), -2.0)], dim=1)
    policy = torch.softmax(logits, dim=1)
    value = torch.tanh(-sq.mean(dim=1))
    return policy.numpy(), value.numpy()


def pair_opening(pair: int, plies: int = OPENING_PLIES) -> list[int]:
    """Opening of matches 2 * pair and 2 * pair + 1: `plies` picks of
    np.random.default_rng(pair) among the legal actions."""
    rng = np.random.default_rng(pair)
    p = O.initial_position()
    out = []
    for _ in range(plies):
        legal = O.legal_actions(p)
        a = int(legal[int(rng.integers(len(legal)))])
        out.append(a)
        p = O.apply_action(p, a)
    return out


def openings(matches: int = MATCHES, plies: int = OPENING_PLIES) -> np.ndarray:
    return np.array([pair_opening(g // 2, plies) for g in range(matches)], dtype=np.int32).reshape(matches, plies)


def swapped(matches: int = MATCHES) -> np.ndarray:
    return np.arange(matches) % 2 == 1


def play_match(key_a: int, key_b: int, opening, a_is_white: bool, temperature_moves: int = 0,
               temperature: float = 1.0, setup: dict = SETUP, eval_a=stub_a, eval_b=stub_b) -> dict:
    """One match. Returns its trace: per ply after the opening a dict with
    a_moves, before / after (position tuples), legal (actions of the root's
    children in order), visits, q (the mover's root children, searched),
    action, tied (the argmax set had more than one member), and the final
    result (play_game's 0 draw / 1 black / 2 white) and discs (black, white)."""
    ta = O.OracleMCTS(game_key=key_a, **setup)
    tb = O.OracleMCTS(game_key=key_b, **setup)
    for a in opening:
        ta.apply_action(int(a))
        tb.apply_action(int(a))
    plies = []
    while True:
        pos = ta.position()
        assert pos.tuple() == tb.position().tuple()
        if pos.player == 0:
            break
        a_moves = (pos.player == 1) != bool(a_is_white)
        tree, ev = (ta, eval_a) if a_moves else (tb, eval_b)
        tree.search(ev)
        visits, q = tree.visit_counts(), tree.mean_action_values()
        legal = O.legal_actions(pos)
        action = tree.selfplay_action(len(plies), temperature_moves, temperature)
        assert action in legal
        ta.apply_action(action)
        tb.apply_action(action)
        plies.append(dict(a_moves=a_moves, before=pos.tuple(), after=ta.position().tuple(), legal=legal,
                          visits=visits, q=q, action=action, tied=visits.count(max(visits)) > 1))
    end = ta.position()
    black, white = bin(end.p1).count("1"), bin(end.p2).count("1")
    return dict(plies=plies, result=1 if black > white else (2 if white > black else 0), discs=(black, white))


_CACHE: dict = {}


def reference_matches(temperature_moves: int = 0, eval_a=stub_a, eval_b=stub_b) -> list[dict]:
    """The MATCHES reference matches of the tests' setup (computed once per
    session and pair of evaluators): keys of engines seeded 0 (A) and 1 (B),
    pair openings, odd matches swapped, by default A = equivariant_stub,
    B = stub_b."""
    k = (temperature_moves, eval_a, eval_b)
    if k not in _CACHE:
        ops, sw = openings(), swapped()
        _CACHE[k] = [
            play_match(game_key(0, g), game_key(1, g), ops[g], bool(sw[g]), temperature_moves,
                       eval_a=eval_a, eval_b=eval_b)
            for g in range(MATCHES)]
    return _CACHE[k]


def summary(match: dict) -> tuple[int, int, int, int, int]:
    """(plies after the opening, passes, tied moves, black discs, white discs)"""
    p = match["plies"]
    return (len(p), sum(x["action"] == 64 for x in p), sum(x["tied"] for x in p), *match["discs"])
