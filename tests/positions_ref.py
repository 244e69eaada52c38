"""Plain-Python restatements for the given-positions tests:
the principal-variation walk over a dict tree, and the frozen roots that
tests/test_gpu_positions.py sets (their properties are asserted on the CPU by
tests/test_cpu_positions.py)."""

from __future__ import annotations


def pv_walk(tree: dict, max_len: int) -> list[tuple[int, int, float]]:
    """The principal variation of ``tree`` = {"children": [(action, visits, q,
    subtree or None), ...]} with the children in legal_actions() order (ascending
    action): repeatedly the most visited child, the first of equals; stops at a
    node without children, at a best child without a visit, or at max_len."""
    out = []
    node = tree
    while node is not None and node.get("children") and len(out) < max_len:
        best = None
        for child in node["children"]:
            if best is None or child[1] > best[1]:
                best = child
        if best[1] <= 0:
            break
        out.append((int(best[0]), int(best[1]), float(best[2])))
        node = best[3]
    return out


def root_tree(visits, q, below=None) -> dict:
    """A one-level dict tree from (65,) visits / q by action; ``below`` maps an
    action to its subtree."""
    below = below or {}
    return {"children": [(a, int(visits[a]), float(q[a]), below.get(a)) for a in range(65) if visits[a] > 0 or a in below]}


# Indices into asym_stub.random_game_chains(40) (2,411 chains): two chains
# shorter than H = 4, the two pass positions with 60 positions behind them, and
# four mid-game chains.
ROOT_INDICES = (0, 2, 359, 420, 80, 521, 1000, 344)
ROOT_LENGTHS = (1, 3, 60, 60, 21, 40, 38, 45)
PASS_ROOTS = (359, 420)
