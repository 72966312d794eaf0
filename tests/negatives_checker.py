"""Host checker of lgcn_sample_negatives (include/lgcn.h), in Python ints and numpy: the counter
hash, the r-th unseen item of an ascending row, the candidates of a list of triplets, and the
hardest-of-n pick by a float64 cosine with the kernel's tie and NaN rule. Independent of the
library: nothing here imports lgcn_amd."""
from __future__ import annotations

import numpy as np

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15


def mix(z: int) -> int:
    z &= M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z


def draw_hash(seed: int, step: int, b: int, j: int) -> int:
    """h2 of triplet b (its global index) and candidate j."""
    h0 = mix((seed + G * (step + 1)) & M64)
    h1 = mix(h0 ^ (b & M64))
    return mix((h1 + G * (j + 1)) & M64)


def umul64hi(a: int, b: int) -> int:
    return (a * b) >> 64


def rth_unseen(row, r: int) -> int:
    """The r-th (from 0) non-negative integer that the ascending, distinct ``row`` does not hold:
    r + t, t the number of positions p with row[p] - p <= r (non-decreasing in p: one bisection)."""
    lo, hi = 0, len(row)
    while lo < hi:
        mid = (lo + hi) >> 1
        if int(row[mid]) - mid <= r:
            lo = mid + 1
        else:
            hi = mid
    return r + lo


def unseen_brute(row, num_items: int) -> list:
    seen = set(int(x) for x in row)
    return [i for i in range(num_items) if i not in seen]


def candidate(row, num_items: int, seed: int, step: int, b: int, j: int):
    """(candidate j of global triplet b for a user with the seen ``row``, whether the row left none)."""
    h2 = draw_hash(seed, step, b, j)
    m = num_items - len(row)
    if m <= 0:
        return umul64hi(h2, num_items), True
    return rth_unseen(row, umul64hi(h2, m)), False


def user_row(ptr, idx, u: int):
    """User u's row of the CSR (None: nothing seen); empty for a user outside it."""
    if ptr is None or u < 0 or u >= len(ptr) - 1:
        return idx[:0] if idx is not None else np.zeros(0, np.int32)
    return idx[int(ptr[u]):int(ptr[u + 1])]


def candidates(users, ptr, idx, num_items: int, seed: int, step: int, n: int, first: int = 0):
    """(cand int64 [B, n], stats0): every triplet's n candidates and the count of triplets whose user
    had seen every item."""
    users = np.asarray(users, np.int64)
    cand = np.zeros((len(users), n), np.int64)
    all_seen = 0
    for b, u in enumerate(users):
        row = user_row(ptr, idx, int(u))
        full = False
        for j in range(n):
            cand[b, j], full = candidate(row, num_items, seed, step, first + b, j)
        all_seen += bool(full)
    return cand, all_seen


def cosines(users, cand, user_rows, item_rows):
    """float64 [B, n]: cos(user_rows[users[b]], item_rows[cand[b, j]]) = dot / (|u| |c|); NaN for a
    zero row, and for a user outside the table."""
    users = np.asarray(users, np.int64)
    uw, iw = np.asarray(user_rows, np.float64), np.asarray(item_rows, np.float64)
    B, n = cand.shape
    out = np.full((B, n), np.nan)
    ok = (users >= 0) & (users < uw.shape[0])
    with np.errstate(divide="ignore", invalid="ignore"):
        for s in range(0, B, 256):
            sel = np.flatnonzero(ok[s:s + 256]) + s
            if sel.size == 0:
                continue
            u = uw[users[sel]]                       # [b, d]
            c = iw[cand[sel]]                        # [b, n, d]
            dot = np.einsum("bd,bnd->bn", u, c)
            out[sel] = dot / (np.sqrt((u * u).sum(1))[:, None] * np.sqrt((c * c).sum(2)))
    return out


def pick_hardest(scores):
    """j int64 [B]: the largest score, the lowest j among equals; NaN ranks as -inf (all NaN: 0)."""
    key = np.where(np.isnan(scores), -np.inf, scores)
    return np.argmax(key, axis=1)  # the first of equal maxima


def hardest(users, ptr, idx, num_items: int, seed: int, step: int, n: int, user_rows, item_rows, first: int = 0):
    """(out int64 [B], stats [2], cand [B, n], scores f64 [B, n], j [B]) as the kernel defines them for
    n > 1, the scores in float64. A user outside [0, U) takes candidate 0 and counts in stats[1]."""
    users = np.asarray(users, np.int64)
    cand, all_seen = candidates(users, ptr, idx, num_items, seed, step, n, first)
    scores = cosines(users, cand, user_rows, item_rows)
    j = pick_hardest(scores)
    bad = (users < 0) | (users >= np.asarray(user_rows).shape[0])
    j[bad] = 0
    out = cand[np.arange(len(users)), j]
    return out, [all_seen, int(bad.sum())], cand, scores, j


def top_gap(scores):
    """float64 [B]: best minus second-best DISTINCT score of each row (NaN as -inf; inf where there is
    no second one): how far a row is from a tie that rounding could decide."""
    key = np.where(np.isnan(scores), -np.inf, scores)
    best = key.max(axis=1, keepdims=True)
    rest = np.where(key < best, key, -np.inf).max(axis=1)
    with np.errstate(invalid="ignore"):
        gap = best[:, 0] - rest
    return np.where(np.isnan(gap), np.inf, gap)
