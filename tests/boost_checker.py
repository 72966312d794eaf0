"""A numpy restatement of the boosted top-k contract of include/lgcn.h (lgcn_score_filter_boost,
lgcn_score_lists_boost; lgcn_amd.recommend.topk_rows' boost=), for the boost tests.

The key of pair (q, j) is score_key(np.float32(s) + np.float32(b)): s the UNBOOSTED score of the pair
as the library gives it, b the candidate's boost, the sum one f32 addition. The eligible candidates
(not in the query's exclusion row, passing its predicate, and under ``among`` named by its row, as
often as they are named) are ranked by (key descending, index ascending) and the list is padded with
-1 / -inf. Nothing here has a tolerance: indices and score bits are compared with equality.

library_scores gets the unboosted scores from the library itself: topk_rows without a boost over
candidate slices of at most MAX_K rows with k the slice length returns every pair's score, and a
pair's key does not depend on which other candidates are present."""
import numpy as np

NAN_KEY = np.uint32(0xFFFFFFFF)
SIGN = np.uint32(0x80000000)


def score_key(s: np.ndarray) -> np.ndarray:
    """The filter's uint32 key of f32 scores: order-preserving for numbers (-0 just below +0), every
    NaN 0xFFFFFFFF (the highest key)."""
    s = np.ascontiguousarray(s, dtype=np.float32)
    u = s.view(np.uint32)
    key = np.where((u & SIGN) != 0, ~u, u | SIGN).astype(np.uint32)
    return np.where(np.isnan(s), NAN_KEY, key).astype(np.uint32)


def key_score(key: np.ndarray) -> np.ndarray:
    """The f32 value of a key (the NaN key gives the NaN of bits 0x7FFFFFFF)."""
    key = np.ascontiguousarray(key, dtype=np.uint32)
    u = np.where((key & SIGN) != 0, key ^ SIGN, ~key).astype(np.uint32)
    return u.view(np.float32)


def boosted_keys(scores: np.ndarray, boost: np.ndarray) -> np.ndarray:
    """uint32 [Q, M]: the key of every pair, one f32 addition per pair."""
    scores = np.asarray(scores)
    boost = np.asarray(boost)
    assert scores.dtype == np.float32 and boost.dtype == np.float32 and boost.shape == scores.shape[1:]
    with np.errstate(invalid="ignore", over="ignore"):
        return score_key(scores + boost[None, :])


def rank(keys: np.ndarray, idx: np.ndarray, k: int):
    """(idx int64 [k], score f32 [k]) of one query's entries (keys uint32 [n], idx [n], repeats
    allowed): key descending, index ascending, padded with -1 / -inf."""
    order = np.lexsort((idx, -keys.astype(np.int64)))[:k]
    out_i = np.full(k, -1, np.int64)
    out_s = np.full(k, -np.inf, np.float32)
    out_i[:len(order)] = idx[order]
    out_s[:len(order)] = key_score(keys[order])
    return out_i, out_s


def boosted_topk(scores, boost, k: int, excl=None, passes=None, among=None):
    """(idx int64 [Q, k], score f32 [Q, k]) of the contract. scores f32 [Q, M] unboosted, boost f32 [M];
    excl: None or one array of excluded candidate indices per query; passes: None or bool [Q, M], the
    predicate restated by the caller; among: None or one array of entries per query (any order,
    repeats ranked as often as named, entries outside [0, M) ignored)."""
    keys = boosted_keys(scores, boost)
    Q, M = keys.shape
    out_i = np.empty((Q, k), np.int64)
    out_s = np.empty((Q, k), np.float32)
    for q in range(Q):
        ok = np.ones(M, bool) if passes is None else np.asarray(passes[q], bool).copy()
        if excl is not None:
            ok[np.asarray(excl[q], np.int64)] = False
        if among is None:
            cand = np.nonzero(ok)[0]
        else:
            row = np.asarray(among[q], np.int64)
            row = row[(row >= 0) & (row < M)]
            cand = row[ok[row]]
        out_i[q], out_s[q] = rank(keys[q, cand], cand, k)
    return out_i, out_s


def brute_force(scores, boost, k: int):
    """boosted_topk without options by a plain Python sort on (float order with NaN first and -0 below
    +0, index): an independent statement of the order for the hand-made cases."""
    import math

    def order_of(v: np.float32):  # larger tuple = ranked earlier
        if math.isnan(v):
            return (2, 0.0, 0)
        return (1, float(v), 0 if v == 0 and math.copysign(1.0, float(v)) < 0 else 1)

    scores = np.asarray(scores, np.float32)
    boost = np.asarray(boost, np.float32)
    out_i = np.full((scores.shape[0], k), -1, np.int64)
    out_s = np.full((scores.shape[0], k), -np.inf, np.float32)
    for q in range(scores.shape[0]):
        with np.errstate(invalid="ignore", over="ignore"):
            vals = [np.float32(scores[q, j]) + np.float32(boost[j]) for j in range(scores.shape[1])]
        ranked = sorted(range(len(vals)), key=lambda j: (tuple(-x for x in order_of(vals[j])), j))[:k]
        for t, j in enumerate(ranked):
            out_i[q, t] = j
            out_s[q, t] = np.float32(np.nan) if math.isnan(vals[j]) else vals[j]
    return out_i, out_s


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    """f32 arrays equal to the bit, every NaN counting as the NaN key's value."""
    a = np.ascontiguousarray(a, np.float32).copy()
    b = np.ascontiguousarray(b, np.float32).copy()
    a[np.isnan(a)] = key_score(np.array([NAN_KEY]))[0]
    b[np.isnan(b)] = key_score(np.array([NAN_KEY]))[0]
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def library_scores(queries, picked, candidates, slice_rows: int = 1024) -> np.ndarray:
    """f32 [Q, M] on the host: the unboosted score the library gives every pair, from topk_rows over
    candidate slices of at most ``slice_rows`` (<= MAX_K) rows with k the slice length."""
    import torch

    from lgcn_amd.recommend import MAX_K, topk_rows

    assert slice_rows <= MAX_K
    Q, M = torch.as_tensor(picked).numel(), candidates.shape[0]
    out = torch.empty((Q, M), dtype=torch.float32, device=queries.device)
    for c0 in range(0, M, slice_rows):
        c1 = min(M, c0 + slice_rows)
        idx, score = topk_rows(queries, picked, candidates[c0:c1], c1 - c0)
        assert bool((idx >= 0).all())  # nothing excluded: every candidate of the slice is listed once
        out[:, c0:c1].scatter_(1, idx, score)
    return out.cpu().numpy()
