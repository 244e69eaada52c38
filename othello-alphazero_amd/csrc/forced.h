// Forced playouts and policy target pruning (KataGo, Wu 2019, section 3.2;
// DESIGN.md §18): the rule, once, for the device (tree_search.h select_range and
// write_targets) and the host (oamd_prune_visit_counts). All arithmetic is
// fp32 in exactly the order written; both sides are built without contraction
// and with IEEE division and square root, so they agree bit for bit.
#pragma once

#include <math.h>
#include <stdint.h>

#include "rng.h"

namespace oamd {

// A root child that has been tried (n > 0) is forced, i.e. selected before any
// PUCT score, while n < sqrt(k * prob * total): prob is the prior the PUCT
// line of this selection uses (noised when the root draws noise), total the
// children's visit sum with in-flight visits. Compared as squares, so the hot
// loop needs no square root.
OAMD_HD bool forced_playout(int32_t n, float prob, int32_t total, float k) {
    return n > 0 && (float)n * (float)n < (k * prob) * (float)total;
}

// PUCT score of a child with stored prior p and mean value q at m visits
OAMD_HD float prune_score(float q, float mult, float p, int32_t m) { return q + mult * p / (1.0f + (float)m); }

// Pruned visit count of a root child other than the most visited one: up to
// cap = (int)sqrt(k * p * total) visits are taken away one by one while the
// child would still score below the best child's score (ubest) with one visit
// fewer, i.e. while PUCT alone would not have spent that visit; a child that
// was reduced and is left with a single visit loses it too. An integer loop
// on purpose: a closed form would round differently on host and device.
OAMD_HD int32_t prune_child(int32_t n, float q, float p, float mult, float ubest, float k, int32_t total) {
    if (n <= 0) return n;
    const float s = sqrtf((k * p) * (float)total);
    // (int)s, held to n: the loop below cannot run more than n times anyway
    const int32_t cap = s < (float)n ? (int32_t)s : n;
    int32_t m = n;
    for (int32_t i = 0; i < cap && m > 0; ++i) {
        if (!(prune_score(q, mult, p, m - 1) < ubest)) break;
        m -= 1;
    }
    if (m < n && m == 1) m = 0;
    return m;
}

}  // namespace oamd
