"""The float64 numpy restatement of "because you watched" explanations (lgcn_explain_topr,
lgcn_amd.explain) that test_explain.py and test_gpu_explain.py check against (a helper module, not
a test file).

The rule, per query q and slot t with j = rec_idx[q, t]: a slot with j outside [0, M) is empty.
Otherwise entry e of the query's history row, i = idx[e], is eligible when 0 <= i < M and i != j;
its contribution is c_e = w_e * (C[i] . C[j]); the eligible entries are ranked by c descending,
then i ascending, NaN as -inf; the first min(r, eligible) are listed, total is the sum over all.

check_lists, for every (q, t): n is exact; listed items are distinct, eligible and from the row;
each value is within BAR of the float64 contribution of the item beside it (NaN where that is NaN);
values do not increase and among bitwise-equal values the items ascend; no unlisted eligible item
has a float64 contribution above the last listed one's by more than 2 * BAR; tails are -1 / -inf;
|total - ref| <= max(1, eligible) * BAR. A listed position is DECIDED when its float64 contribution
in the reference order is more than 2 * BAR away from both neighbours of that order: there the item
must be the reference's. BAR = 1e-5 is the score bar of test_gpu_recommend.py, the f32 cosine of
unit rows against float64; weights in the tests have magnitude <= 1, so it carries over."""
import numpy as np

BAR = 1e-5


def history_row(ptr, idx, w, row):
    """(items int64, weights float64) of CSR row ``row``; a row outside the CSR is empty."""
    if row < 0 or row >= len(ptr) - 1:
        return np.zeros(0, np.int64), np.zeros(0)
    b, e = int(ptr[row]), int(ptr[row + 1])
    items = np.asarray(idx[b:e], np.int64)
    return items, (np.ones(items.size) if w is None else np.asarray(w[b:e], np.float32).astype(np.float64))


def ranked64(items, w, C, j):
    """All eligible entries of one slot in rank order: (items, contributions float64)."""
    M = C.shape[0]
    if not 0 <= j < M:
        return np.zeros(0, np.int64), np.zeros(0)
    ok = (items >= 0) & (items < M) & (items != j)
    it = items[ok]
    with np.errstate(invalid="ignore"):
        c = w[ok] * (C[it] @ C[j])
    key = np.where(np.isnan(c), -np.inf, c)
    order = np.lexsort((it, -key))
    return it[order], c[order]


def explain64(items, w, C, j, r):
    """The rule for one slot: (idx int64 [r], value float64 [r], n, total)."""
    it, c = ranked64(items, w, C, j)
    n = min(r, it.size)
    idx, val = np.full(r, -1, np.int64), np.full(r, -np.inf)
    idx[:n], val[:n] = it[:n], c[:n]
    return idx, val, n, float(np.sum(c))


def undecided64(c, n):
    """Of the first n positions of the reference order c, those not decided."""
    key = np.where(np.isnan(c), -np.inf, c)
    with np.errstate(invalid="ignore"):
        gap = np.abs(np.diff(key))  # -inf beside -inf: nan, not decided
    close = ~(gap > 2 * BAR)
    und = np.zeros(c.size, bool)
    und[:-1] |= close
    und[1:] |= close
    return und[:n]


def check_lists(rec_idx, ptr, idx, w, rows, C, r, out_idx, out_val, out_n, out_total):
    """The module docstring's checks for rec_idx [Q, k] (numpy arrays; C float64 [M, D], the rows the
    contributions are dot products of; rows None: query q uses CSR row q). Returns
    (decided positions, listed positions)."""
    rec_idx = np.asarray(rec_idx, np.int64)
    out_idx, out_val = np.asarray(out_idx, np.int64), np.asarray(out_val, np.float32)
    Q, k = rec_idx.shape
    assert out_idx.shape == out_val.shape == (Q, k, r) and out_n.shape == out_total.shape == (Q, k)
    decided_n = listed_n = 0
    for q in range(Q):
        items, wq = history_row(ptr, idx, w, q if rows is None else int(rows[q]))
        for t in range(k):
            where = (q, t)
            it, c = ranked64(items, wq, C, int(rec_idx[q, t]))
            n = min(r, it.size)
            gi, gv = out_idx[q, t], out_val[q, t]
            assert int(out_n[q, t]) == n, (where, int(out_n[q, t]), n)
            assert (gi[n:] == -1).all() and np.isneginf(gv[n:]).all(), where
            ref_total, got_total = float(np.sum(c)), float(out_total[q, t])
            if np.isnan(ref_total):
                assert np.isnan(got_total), where
            else:
                assert abs(got_total - ref_total) <= max(1, it.size) * BAR, (where, got_total, ref_total)
            if n == 0:
                continue
            assert len(set(gi[:n].tolist())) == n, (where, gi)
            c_of = dict(zip(it.tolist(), c.tolist()))
            assert all(int(i) in c_of for i in gi[:n]), (where, gi)  # eligible and from the row
            cg = np.array([c_of[int(i)] for i in gi[:n]])
            nan = np.isnan(cg)
            assert (np.isnan(gv[:n]) == nan).all(), (where, gv, cg)
            assert (np.abs(gv[:n][~nan].astype(np.float64) - cg[~nan]) <= BAR).all(), (where, gv, cg)
            gk = gv[:n].copy()  # float32: the ranking treats NaN as -inf
            gk[np.isnan(gk)] = -np.inf
            for p in range(n - 1):
                assert gk[p] >= gk[p + 1], (where, gv)
                if gk[p].view(np.uint32) == gk[p + 1].view(np.uint32):
                    assert gi[p] < gi[p + 1], (where, gi, gv)
            if it.size > n:  # nothing better was left out
                last = -np.inf if np.isnan(cg[-1]) else cg[-1]
                rest = np.array([x for i, x in c_of.items() if i not in set(gi[:n].tolist())])
                rest = np.where(np.isnan(rest), -np.inf, rest)
                assert rest.max() == last or rest.max() <= last + 2 * BAR, (where, rest.max(), last)
            und = undecided64(c, n)
            assert (gi[:n][~und] == it[:n][~und]).all(), (where, gi, it[:n], und)
            decided_n += int((~und).sum())
            listed_n += n
    return decided_n, listed_n
