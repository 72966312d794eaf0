"""The float64 numpy restatement of fold-in (lgcn_foldin_rows, lgcn_amd.foldin) that test_foldin.py
and test_gpu_foldin.py check against (a helper module, not a test file).

The rule, per query q with history row r = rows[q] (q when rows is None; a row outside the CSR is
empty): entry e of the row with i = idx[e] is eligible when 0 <= i < M, n_q counts the eligible
entries (a repeated entry each time), and
    t_e[c] = (w[e] * isd[i]) * table[i, c]          (a factor that is None is 1)
    out[q, c] = s_q * sum_e t_e[c],   s_q = 1 / sqrt(n_q),   a row of zeros when n_q = 0.

The bar (bound64), per component: |out - ref| <= (n + 8) * 2^-24 * s_q * sum_e |t_e[c]|. Summing n
f32 terms in ANY order is off by at most (n - 1) * u * sum|t| to first order, u = 2^-24; each term
carries the roundings of its two products (2 u), the scale s_q is rounded once from float64 (u) and
the final product once more (u): (n + 3) u in all, and the remaining 5 u cover the second-order
terms, which stay below n^2 u^2 <= 2^-32 * u^-1 * u = u / 256 at the n <= 256 the grid uses. At
n <= 256 the bar is at most 264 * 2^-24 < 1.6e-5 of sum|t|, far below one term, so a dropped or
doubled entry cannot hide behind it.
"""
import numpy as np

U24 = 2.0 ** -24


def history_row(ptr, idx, w, row):
    """(items int64, weights float64 or None) of CSR row ``row``; a row outside the CSR is empty."""
    if row < 0 or row >= len(ptr) - 1:
        return np.zeros(0, np.int64), (None if w is None else np.zeros(0))
    b, e = int(ptr[row]), int(ptr[row + 1])
    return np.asarray(idx[b:e], np.int64), (None if w is None else np.asarray(w[b:e], np.float64))


def sums64(ptr, idx, w, rows, Q, table, isd):
    """(sum_e t_e float64 [Q, d], sum_e |t_e| float64 [Q, d], n int64 [Q]) of the rule, unscaled.
    ptr / idx / w / rows / table / isd are numpy arrays (w, rows, isd may be None)."""
    table = np.asarray(table, np.float64)
    M, d = table.shape
    total, absum, n = np.zeros((Q, d)), np.zeros((Q, d)), np.zeros(Q, np.int64)
    for q in range(Q):
        items, wq = history_row(ptr, idx, w, q if rows is None else int(rows[q]))
        ok = (items >= 0) & (items < M)
        it = items[ok]
        f = np.ones(it.size)
        if wq is not None:
            f = f * wq[ok]
        if isd is not None:
            f = f * np.asarray(isd, np.float64)[it]
        with np.errstate(invalid="ignore"):
            t = f[:, None] * table[it]
        total[q], absum[q], n[q] = t.sum(0), np.abs(t).sum(0), it.size
    return total, absum, n


def scale64(n):
    """s_q = 1 / sqrt(n_q) in float64, 0 where n_q = 0."""
    n = np.asarray(n, np.float64)
    return np.where(n > 0, 1.0 / np.sqrt(np.maximum(n, 1.0)), 0.0)


def foldin64(ptr, idx, w, rows, Q, table, isd):
    """(out float64 [Q, d], n int64 [Q], bound float64 [Q, d]) — the rule and the module docstring's
    bar for an f32 implementation of it."""
    total, absum, n = sums64(ptr, idx, w, rows, Q, table, isd)
    s = scale64(n)[:, None]
    return total * s, n, (n[:, None] + 8) * U24 * absum * s


def exact32(ptr, idx, w, rows, Q, table, isd):
    """(out f32 [Q, d], n) for inputs whose terms are multiples of 1/8 with sum|t| * 8 < 2^24 (both
    asserted): every partial sum, in any order, is then a multiple of 1/8 below 2^21 and exact in
    f32. The result is float32(exact sum) * float32(s_q), the one rounded product of the rule, zeros
    where n_q = 0."""
    total, absum, n = sums64(ptr, idx, w, rows, Q, table, isd)
    assert (absum * 8.0 == np.round(absum * 8.0)).all() and absum.max(initial=0.0) * 8.0 < 2.0 ** 24
    assert (total.astype(np.float32) == total).all()
    s = scale64(n).astype(np.float32)[:, None]
    return total.astype(np.float32) * s, n
