"""The float64 numpy restatement of greedy MMR re-ranking (lgcn_rerank_mmr, lgcn_amd.recommend) that
test_rerank.py and test_gpu_rerank.py check against (a helper module, not a test file).

The rule, per query, with d = diversity: position p of the pool is eligible when 0 <= index < M;
it keeps m_p (largest cosine to a pick so far, 0 before the first pick) and a_p (their sum). Step t
picks the eligible, unpicked position with the largest (1 - d) * r_p - d * m_p (NaN as -inf), the
lowest position among equal values, and records (index, r_p, a_p).

check_lists REPLAYS THE KERNEL'S OWN PREFIX: at step t the float64 values are formed given the
kernel's picks 0 .. t - 1, so one close call does not condemn the rest of a list. A step is DECIDED
when the best float64 value exceeds the runner-up by more than 2 * BAR, or one candidate is left:
there the kernel's pick must be the checker's. At every step the float64 value of the kernel's pick
is within 2 * BAR of the best, and |pair[t] - ref| <= max(1, t) * BAR. Always: the score is the
pool's score of that index bit for bit, indices are distinct, eligible and from the pool, the tails
are -1 / -inf / 0 and n is exact. BAR = 1e-5 is the score bar of test_gpu_recommend.py: the kernel's
f32 cosines of unit rows are within it of the float64 ones, a value is one such cosine times d <= 1
plus an exact-to-rounding product, a pair sum is t of them."""
import numpy as np

BAR = 1e-5


def unit_rows64(c):
    """Rows of c normalised in float64 (a zero row becomes NaN, as lgcn_normalize_rows makes it)."""
    c = np.asarray(c, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return c / np.linalg.norm(c, axis=1, keepdims=True)


def _gram(pidx, U):
    """Cosines between the pool's positions (ineligible positions: a row of zeros, never used)."""
    ok = (pidx >= 0) & (pidx < U.shape[0])
    rows = np.where(ok[:, None], U[np.where(ok, pidx, 0)], 0.0) if U.shape[0] else np.zeros((pidx.size, U.shape[1]))
    with np.errstate(invalid="ignore"):
        return ok, rows @ rows.T


def _values(r, m, delta, cand):
    with np.errstate(invalid="ignore"):
        v = (1.0 - delta) * r[cand] - delta * m[cand]
    v[np.isnan(v)] = -np.inf
    return v


def mmr64(pidx, pscore, U, k, delta):
    """The rule for one query in float64: (idx int64 [k], score f32 [k], pair f64 [k], n)."""
    pidx = np.asarray(pidx, np.int64)
    r = np.asarray(pscore, np.float32).astype(np.float64)
    ok, G = _gram(pidx, U)
    taken = np.zeros(pidx.size, bool)
    m, a = np.zeros(pidx.size), np.zeros(pidx.size)
    idx = np.full(k, -1, np.int64)
    score = np.full(k, -np.inf, np.float32)
    pair = np.zeros(k)
    n = 0
    for t in range(k):
        cand = np.flatnonzero(ok & ~taken)
        if cand.size == 0:
            break
        c = cand[np.argmax(_values(r, m, delta, cand))]  # the first maximum: the lowest position
        idx[t], score[t], pair[t] = pidx[c], np.asarray(pscore, np.float32)[c], a[c]
        taken[c] = True
        m = G[:, c].copy() if t == 0 else np.fmax(m, G[:, c])
        a = a + G[:, c]
        n += 1
    return idx, score, pair, n


def check_lists(pool_idx, pool_score, U, k, delta, out_idx, out_score, out_pair, out_n):
    """The module docstring's checks for Q queries (numpy arrays; U = unit_rows64(candidates);
    out_pair / out_n may be None for lists that do not carry them, a short list then being the
    filled prefix). Returns (decided steps, all steps)."""
    pool_idx = np.asarray(pool_idx, np.int64)
    pool_score = np.asarray(pool_score, np.float32)
    out_idx = np.asarray(out_idx, np.int64)
    out_score = np.asarray(out_score, np.float32)
    Q, N = pool_idx.shape
    assert out_idx.shape == out_score.shape == (Q, k)
    decided_n = steps_n = 0
    for q in range(Q):
        pidx = pool_idx[q]
        r = pool_score[q].astype(np.float64)
        ok, G = _gram(pidx, U)
        n = min(k, int(ok.sum()))
        if out_n is not None:
            assert int(out_n[q]) == n, (q, int(out_n[q]), n)
        assert (out_idx[q, n:] == -1).all() and np.isneginf(out_score[q, n:]).all(), q
        if out_pair is not None:
            assert (np.asarray(out_pair)[q, n:] == 0).all(), q
        pos_of = {int(i): p for p, i in enumerate(pidx) if ok[p]}
        taken = np.zeros(N, bool)
        m, a = np.zeros(N), np.zeros(N)
        for t in range(n):
            cand = np.flatnonzero(ok & ~taken)
            v = _values(r, m, delta, cand)
            c = pos_of.get(int(out_idx[q, t]))
            assert c is not None and not taken[c], (q, t, int(out_idx[q, t]))  # from the pool, eligible, distinct
            order = np.argsort(-v, kind="stable")
            best = v[order[0]]
            with np.errstate(invalid="ignore"):  # -inf beside -inf: not decided
                decided = cand.size == 1 or bool(best - v[order[1]] > 2 * BAR)
            if decided:
                assert c == cand[order[0]], (q, t, c, cand[order[0]])
            vc = v[np.searchsorted(cand, c)]
            assert vc == best or vc >= best - 2 * BAR, (q, t, vc, best)
            assert out_score[q, t].view(np.uint32) == pool_score[q, c].view(np.uint32), (q, t)
            if out_pair is not None:
                got = float(np.asarray(out_pair)[q, t])
                if np.isnan(a[c]):
                    assert np.isnan(got), (q, t)
                else:
                    assert abs(got - a[c]) <= max(1, t) * BAR, (q, t, got, a[c])
            taken[c] = True
            m = G[:, c].copy() if t == 0 else np.fmax(m, G[:, c])
            a = a + G[:, c]
            decided_n += int(decided)
            steps_n += 1
    return decided_n, steps_n


def ild64(pair, n, cs):
    """ILD@c in float64, list by list: 1 - 2 * sum(pair[:c']) / (c' (c' - 1)), c' = min(c, n); NaN
    where c' < 2. Columns follow the sorted distinct cutoffs."""
    cs = sorted(set(int(c) for c in cs))
    out = np.full((len(n), len(cs)), np.nan)
    for q in range(len(n)):
        for j, c in enumerate(cs):
            cp = min(c, int(n[q]))
            if cp >= 2:
                out[q, j] = 1.0 - 2.0 * float(np.sum(np.asarray(pair[q][:cp], np.float64))) / (cp * (cp - 1))
    return out
