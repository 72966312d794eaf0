"""Host oracle of group recommendation (lgcn_amd.recommend.topk_groups, lgcn_score_filter_groups), numpy.

It starts from the members' full f32 score rows [n, M] — on the GPU tests those are the filter's own
scores, read back through topk_rows — and forms the group's key by the contract of include/lgcn.h, to
the bit:
    any member score a NaN: the NaN key 0xFFFFFFFF;
    min / max: the smallest / largest of the members' score keys (so -0 orders below +0);
    mean: the float32 sum in member order, one addition at a time from member 0's score on, then one
          float32 division by the member count.
Then the floor (a candidate some member scores below it is dropped; a float comparison, so a NaN score
drops nothing), the exclusion row and the attribute predicate, and the ranking: key descending, index
ascending, padded with -1 / -inf."""
from __future__ import annotations

import numpy as np

NAN_KEY = np.uint32(0xFFFFFFFF)
STRATEGIES = ("least_misery", "most_pleasure", "average")


def score_key(s) -> np.ndarray:
    """The filter's uint32 key of f32 scores: order-preserving, -0 just below +0, every NaN highest."""
    s = np.ascontiguousarray(s, dtype=np.float32)
    u = s.view(np.uint32)
    key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    key[np.isnan(s)] = NAN_KEY
    return key


def key_score(key) -> np.ndarray:
    """The f32 score behind a key, as the ranked selection stores it (the NaN key gives bits 0x7FFFFFFF)."""
    key = np.ascontiguousarray(key, dtype=np.uint32)
    u = np.where(key & np.uint32(0x80000000), key ^ np.uint32(0x80000000), ~key).astype(np.uint32)
    return u.view(np.float32)


def group_keys(scores, strategy: str) -> np.ndarray:
    """uint32 [M]: the group key of every candidate from the members' score rows [n, M], n >= 1."""
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    assert scores.ndim == 2 and scores.shape[0] >= 1 and strategy in STRATEGIES
    keys = score_key(scores)
    if strategy == "least_misery":
        out = keys.min(0)
    elif strategy == "most_pleasure":
        out = keys.max(0)
    else:
        with np.errstate(all="ignore"):
            total = scores[0].copy()
            for m in range(1, scores.shape[0]):
                total = (total + scores[m]).astype(np.float32)  # one IEEE f32 addition per member
            out = score_key((total / np.float32(scores.shape[0])).astype(np.float32))
    out = out.astype(np.uint32)
    out[np.isnan(scores).any(0)] = NAN_KEY
    return out


def eligible(scores, floor=None, excl=None, passes=None) -> np.ndarray:
    """bool [M]: candidates no member scores below the floor, outside the exclusion row, passing the predicate."""
    scores = np.asarray(scores, dtype=np.float32)
    ok = np.ones(scores.shape[1], dtype=bool)
    if floor is not None:
        with np.errstate(invalid="ignore"):
            ok &= ~(scores < np.float32(floor)).any(0)
    if excl is not None and len(excl):
        ok[np.asarray(excl, dtype=np.int64)] = False
    if passes is not None:
        ok &= np.asarray(passes, dtype=bool)
    return ok


def rank_group(scores, k: int, strategy: str, floor=None, excl=None, passes=None):
    """(idx int64 [k], score f32 [k]) of one group; scores [n, M], n = 0 for an empty group."""
    idx = np.full(k, -1, dtype=np.int64)
    out = np.full(k, -np.inf, dtype=np.float32)
    scores = np.asarray(scores, dtype=np.float32)
    if scores.shape[0] == 0:
        return idx, out
    keys = group_keys(scores, strategy)
    cand = np.nonzero(eligible(scores, floor, excl, passes))[0]
    order = cand[np.lexsort((cand, -keys[cand].astype(np.int64)))][:k]
    idx[:len(order)] = order
    out[:len(order)] = key_score(keys[order])
    return idx, out


def rank_groups(member_scores, groups, k: int, strategy: str, floor=None, excl=None, passes=None):
    """(idx int64 [G, k], score f32 [G, k]): rank_group per group. member_scores [U, M] holds every
    user's score row, groups the member lists; floor: None, a float or one per group; excl: None or a
    row of candidate indices per group; passes: None, bool [M] or bool [G, M]."""
    G = len(groups)
    idx = np.empty((G, k), dtype=np.int64)
    score = np.empty((G, k), dtype=np.float32)
    for g, members in enumerate(groups):
        f = None if floor is None else (floor if np.ndim(floor) == 0 else floor[g])
        p = None if passes is None else (passes if np.ndim(passes) == 1 else passes[g])
        idx[g], score[g] = rank_group(member_scores[np.asarray(members, dtype=np.int64)], k, strategy, f,
                                      None if excl is None else excl[g], p)
    return idx, score
