"""The float64 numpy restatement of lgcn_amd.metrics that test_rank_metrics.py and
test_gpu_rank_metrics.py check against (a helper module, not a test file)."""
import numpy as np

METRICS = ("recall", "precision", "hit_rate", "ndcg", "mrr")


def counts64(ranked, truth_of, cs):
    """Per-query counts of ranked [Q, k] against truth_of(q) (an integer array, possibly empty):
    hits int [Q, C], dcg float64 [Q, C], first int [Q] (-1: no hit), n_truth int [Q]."""
    Q, k = ranked.shape
    hits = np.zeros((Q, len(cs)), np.int64)
    dcg = np.zeros((Q, len(cs)), np.float64)
    first = np.full(Q, -1, np.int64)
    n_truth = np.zeros(Q, np.int64)
    disc = 1.0 / np.log2(np.arange(k, dtype=np.float64) + 2.0)
    for q in range(Q):
        t = np.asarray(truth_of(q), np.int64)
        n_truth[q] = t.size
        hit = (ranked[q] >= 0) & np.isin(ranked[q], t)
        where = np.flatnonzero(hit)
        if where.size:
            first[q] = where[0]
        for j, c in enumerate(cs):
            hits[q, j] = hit[:c].sum()
            dcg[q, j] = disc[:c][hit[:c]].sum()
    return hits, dcg, first, n_truth


def summarize64(hits, dcg, first, n_truth, cs):
    """The means over the queries with n_truth > 0, in float64, query by query."""
    cs = sorted(set(int(c) for c in cs))
    valid = np.flatnonzero(np.asarray(n_truth) > 0)
    out = {"users": int(valid.size)}
    sums = {f"{m}@{c}": 0.0 for m in METRICS for c in cs}
    for q in valid:
        T = int(n_truth[q])
        for j, c in enumerate(cs):
            h = int(hits[q, j])
            idcg = float((1.0 / np.log2(np.arange(min(c, T), dtype=np.float64) + 2.0)).sum())
            sums[f"recall@{c}"] += h / T
            sums[f"precision@{c}"] += h / c
            sums[f"hit_rate@{c}"] += float(h > 0)
            sums[f"ndcg@{c}"] += float(dcg[q, j]) / idcg
            sums[f"mrr@{c}"] += 1.0 / (int(first[q]) + 1) if 0 <= first[q] < c else 0.0
    for key, s in sums.items():
        out[key] = s / valid.size if valid.size else float("nan")
    return out


def scores64(q, c):
    """Cosine scores in float64 (the checker of test_gpu_recommend.py): normalise, q @ c.T."""
    q, c = q.astype(np.float64), c.astype(np.float64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    c = c / np.linalg.norm(c, axis=1, keepdims=True)
    return q @ c.T


def eligible_order(srow, excl):
    """Eligible candidates of one query in rank order: excluded entries to -inf, score descending,
    index ascending (np.lexsort)."""
    s = srow.copy()
    s[excl] = -np.inf
    order = np.lexsort((np.arange(s.size), -s))
    return order[:s.size - len(excl)]
