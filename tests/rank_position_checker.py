"""Numpy checker of lgcn_amd.metrics.rank_positions / summarize_positions (no torch, no library).

positions_from_keys ranks a [Q, M] uint32 key matrix the way lgcn_select_topk_ranked does — key
descending, candidate index ascending, the query's seen row dropped — by SORTING, and reads each
truth entry's slot off the order. summaries64 computes the summaries straight from their
definitions in float64; AUC by counting (held-out, negative) pairs."""
import math

import numpy as np

METRICS = ("recall", "precision", "hit_rate", "ndcg", "mrr")


def positions_from_keys(keys, truth_of, seen_of):
    """keys: uint32 [Q, M]; truth_of(q) / seen_of(q): the query's truth entries (any integers, in
    row order) and seen candidates. Returns (ptr int64 [Q + 1], pos int32 [nnz], key uint32 [nnz],
    eligible int32 [Q]); pos is -1 and key 0 as lgcn_rank_positions documents them."""
    keys = np.asarray(keys, dtype=np.uint32)
    Q, M = keys.shape
    ptr, pos, tkey, eligible = [0], [], [], []
    for q in range(Q):
        truth = [int(j) for j in truth_of(q)]
        left = np.ones(M, dtype=bool)
        for i in seen_of(q):
            if 0 <= int(i) < M:
                left[int(i)] = False
        cand = np.flatnonzero(left)
        # key descending, then index ascending: a stable sort of the ascending indices on -key
        order = cand[np.argsort(-keys[q, cand].astype(np.int64), kind="stable")]
        slot = {int(i): s for s, i in enumerate(order)}
        for j in truth:
            pos.append(slot.get(j, -1) if 0 <= j < M else -1)
            tkey.append(int(keys[q, j]) if 0 <= j < M else 0)
        ptr.append(len(pos))
        eligible.append(int(left.sum()))
    return (np.array(ptr, np.int64), np.array(pos, np.int32).reshape(-1), np.array(tkey, np.uint32).reshape(-1),
            np.array(eligible, np.int32))


def auc_by_pairs(pos_ranked, eligible):
    """The share of (held-out, negative) pairs with the held-out item above the negative, counted
    pair by pair: the user's ranking has ``eligible`` slots, the held-out items sit at pos_ranked."""
    held = np.unique(np.asarray(pos_ranked, dtype=np.int64))
    negatives = np.setdiff1d(np.arange(eligible, dtype=np.int64), held)
    above = held[:, None] < negatives[None, :]  # one cell per pair
    return int(above.sum()) / above.size


def summaries64(ptr, pos, eligible, ks=()):
    """summarize_positions' dictionary from the definitions, in float64 Python arithmetic."""
    cs = sorted({int(c) for c in ks})
    names = ["auc", "mpr", "mrr", "mean_rank"] + [f"{m}@{c}" for m in METRICS for c in cs]
    sums = dict.fromkeys(names, 0.0)
    users = 0
    for q in range(len(eligible)):
        row = [int(p) for p in pos[ptr[q]:ptr[q + 1]]]
        T, E = len(row), int(eligible[q])
        ranked = [p for p in row if p >= 0]
        if not ranked or E - len(ranked) <= 0:
            continue
        users += 1
        sums["auc"] += auc_by_pairs(ranked, E)
        sums["mpr"] += sum(p / max(E - 1, 1) for p in ranked) / len(ranked)
        sums["mrr"] += 1.0 / (min(ranked) + 1)
        sums["mean_rank"] += sum(ranked) / len(ranked)
        for c in cs:
            hit = sorted(p for p in ranked if p < c)
            idcg = sum(1.0 / math.log2(r + 2) for r in range(min(c, T)))
            sums[f"recall@{c}"] += len(hit) / T
            sums[f"precision@{c}"] += len(hit) / c
            sums[f"hit_rate@{c}"] += 1.0 if hit else 0.0
            sums[f"ndcg@{c}"] += sum(1.0 / math.log2(p + 2) for p in hit) / idcg
            sums[f"mrr@{c}"] += 1.0 / (hit[0] + 1) if hit else 0.0
    out = {"users": users}
    for name in names:
        out[name] = sums[name] / users if users else float("nan")
    return out


def key_scores(keys):
    """float32 scores behind lgcn_score_filter's keys (csrc/lgcn_ragged.h ordered_value)."""
    k = np.asarray(keys).view(np.uint32)
    bits = np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k).astype(np.uint32)
    return bits.view(np.float32)
