"""The float64 numpy restatement of calibrated re-ranking (lgcn_attr_profile, lgcn_rerank_calibrated,
lgcn_amd.recommend) that test_calibrate.py and test_gpu_calibrate.py check against (a helper module,
not a test file).

The rule. Genres are the 32 bits of an item's attribute word; an item's own distribution is uniform
over its set bits, b(g|i) = [bit g of attr[i]] / popcount(attr[i]), and an item with a zero word has
none. profile64: p_g = sum_e w_e b(g|i_e) / W over the history entries with 0 <= i < M, a non-zero
word and a weight > 0, W their weight (zeros and W = 0 when there is none). calibrate64, per query
with l = lambda, a = alpha, p the target: position c of the pool is eligible when 0 <= index < M.
After some picks, mass_g = sum of b(g|i) over them, m = the picks with a word, q_g = mass_g /
max(1, m), q~_g = (1 - a) q_g + a p_g and KL = sum_{p_g > 0} p_g ln(p_g / q~_g). A step picks the
eligible, unpicked position with the largest (1 - l) r_c - l KL(picks + c) (NaN as -inf), the lowest
position among equal values, and records (index, r_c, KL(picks + c)). l and a are taken as the f32
numbers the kernel is handed.

check_lists REPLAYS THE KERNEL'S OWN PREFIX: at step t the float64 values are formed given the
kernel's picks 0 .. t - 1, so one close call does not condemn the rest of a list. Every candidate has
its own bar,
    bar_c = 64 * 2^-24 * [(1 - l) |r_c| + l (sum_g p_g + sum_{p_g > 0} p_g (|ln p_g| + |ln q~_g|))],
q~ being that of picks + c: three roundings forming q~ are an absolute 3 eps in ln q~ (the sum_g p_g
term), a log good to 2 ulp adds 2 eps (|ln p_g| + |ln q~_g|), one product per term, at most 32
additions: about 37 eps of that scale, rounded up to 64. A step is DECIDED when the best float64
value exceeds the runner-up by more than 2 * max_c bar_c, or one candidate is left: there the
kernel's pick must be the checker's. At every step the float64 value of the kernel's pick is within
2 * bar of the best, and |out_kl - KL64| <= bar at l = 1's scale. Always: the score is the pool's
score of that index bit for bit, indices are distinct, eligible and from the pool, the tails are
-1 / -inf / 0 and n is exact. check_lists also returns the worst observed error / scale ratios, in
units of 2^-24, of the KL and of the value (the kernel's f32 value rebuilt from its own score and KL)."""
import numpy as np

EPS = 2.0 ** -24
FACTOR = 64.0
GENRES = 32


def item_dists(words):
    """(dist float64 [n, 32], has bool [n]) of uint32 words: uniform over the set bits, zeros for 0."""
    w = np.asarray(words).astype(np.int64) & 0xFFFFFFFF
    bits = ((w[:, None] >> np.arange(GENRES)[None, :]) & 1).astype(np.float64)
    pc = bits.sum(1)
    return bits / np.maximum(pc, 1.0)[:, None], pc > 0


def profile64(idx, weights, attr):
    """(p float64 [32], W) of one history: idx its entries, weights one per entry or None, attr [M]."""
    idx = np.asarray(idx, np.int64)
    w = np.ones(idx.size) if weights is None else np.asarray(weights, np.float32).astype(np.float64)
    attr = np.asarray(attr)
    inside = (idx >= 0) & (idx < attr.size)
    words = np.where(inside, attr[np.where(inside, idx, 0)] if attr.size else 0, 0)
    dist, has = item_dists(words)
    with np.errstate(invalid="ignore"):
        counts = inside & has & (w > 0)  # a NaN weight is not > 0
    W = float(w[counts].sum())
    if not counts.any():
        return np.zeros(GENRES), 0.0
    return (dist[counts] * w[counts, None]).sum(0) / W, W


def _pool(pidx, attr):
    pidx = np.asarray(pidx, np.int64)
    attr = np.asarray(attr)
    ok = (pidx >= 0) & (pidx < attr.size)
    words = np.where(ok, attr[np.where(ok, pidx, 0)] if attr.size else 0, 0)
    dist, has = item_dists(words)
    return ok, dist, has


def _kl_with(p, mass, m, dist, has, cand, alpha):
    """(KL float64 [c], scale float64 [c]) of the list with each candidate of ``cand`` added."""
    pos = p > 0
    mass_c = mass[None, :] + dist[cand]
    m_c = np.maximum(1, m + has[cand].astype(np.int64)).astype(np.float64)
    qt = (1.0 - alpha) * mass_c / m_c[:, None] + alpha * p[None, :]
    pp = p[pos]
    lnp, lnq = np.log(pp)[None, :], np.log(qt[:, pos])
    kl = (pp[None, :] * (lnp - lnq)).sum(1)
    scale = pp.sum() + (pp[None, :] * (np.abs(lnp) + np.abs(lnq))).sum(1)
    return kl, scale


def _values(r, kl, lam, cand):
    with np.errstate(invalid="ignore"):
        v = (1.0 - lam) * r[cand] - lam * kl
    v[np.isnan(v)] = -np.inf
    return v


def calibrate64(pidx, pscore, attr, p, k, lam, alpha):
    """The rule for one query in float64: (idx int64 [k], score f32 [k], kl f64 [k], n)."""
    lam, alpha = float(np.float32(lam)), float(np.float32(alpha))
    pidx = np.asarray(pidx, np.int64)
    p = np.asarray(p, np.float32).astype(np.float64)
    r = np.asarray(pscore, np.float32).astype(np.float64)
    ok, dist, has = _pool(pidx, attr)
    taken = np.zeros(pidx.size, bool)
    mass, m = np.zeros(GENRES), 0
    idx = np.full(k, -1, np.int64)
    score = np.full(k, -np.inf, np.float32)
    kls = np.zeros(k)
    n = 0
    for t in range(k):
        cand = np.flatnonzero(ok & ~taken)
        if cand.size == 0:
            break
        kl, _ = _kl_with(p, mass, m, dist, has, cand, alpha)
        j = int(np.argmax(_values(r, kl, lam, cand)))  # the first maximum: the lowest position
        c = cand[j]
        idx[t], score[t], kls[t] = pidx[c], np.asarray(pscore, np.float32)[c], kl[j]
        taken[c] = True
        mass, m = mass + dist[c], m + int(has[c])
        n += 1
    return idx, score, kls, n


def check_lists(pool_idx, pool_score, attr, target, k, lam, alpha, out_idx, out_score, out_kl, out_n):
    """The module docstring's checks for Q queries (numpy arrays; out_kl / out_n may be None for lists
    that do not carry them, a short list then being the filled prefix). Returns (decided steps, all
    steps, {'value': worst value ratio, 'kl': worst KL ratio}), the ratios in units of 2^-24."""
    lam32, lam, alpha = np.float32(lam), float(np.float32(lam)), float(np.float32(alpha))
    pool_idx = np.asarray(pool_idx, np.int64)
    pool_score = np.asarray(pool_score, np.float32)
    out_idx = np.asarray(out_idx, np.int64)
    out_score = np.asarray(out_score, np.float32)
    target = np.asarray(target, np.float32).astype(np.float64)
    Q, N = pool_idx.shape
    assert out_idx.shape == out_score.shape == (Q, k)
    decided_n = steps_n = 0
    worst = {"value": 0.0, "kl": 0.0}
    for q in range(Q):
        pidx, p = pool_idx[q], target[q]
        r = pool_score[q].astype(np.float64)
        ok, dist, has = _pool(pidx, attr)
        n = min(k, int(ok.sum()))
        if out_n is not None:
            assert int(out_n[q]) == n, (q, int(out_n[q]), n)
        assert (out_idx[q, n:] == -1).all() and np.isneginf(out_score[q, n:]).all(), q
        if out_kl is not None:
            assert (np.asarray(out_kl)[q, n:] == 0).all(), q
        pos_of = {int(i): c for c, i in enumerate(pidx) if ok[c]}
        taken = np.zeros(N, bool)
        mass, m = np.zeros(GENRES), 0
        for t in range(n):
            cand = np.flatnonzero(ok & ~taken)
            kl, scale = _kl_with(p, mass, m, dist, has, cand, alpha)
            v = _values(r, kl, lam, cand)
            with np.errstate(invalid="ignore"):
                vscale = (1.0 - lam) * np.abs(r[cand]) + lam * scale
            vscale[np.isnan(vscale)] = np.inf
            bar = FACTOR * EPS * vscale
            c = pos_of.get(int(out_idx[q, t]))
            assert c is not None and not taken[c], (q, t, int(out_idx[q, t]))  # from the pool, eligible, distinct
            order = np.argsort(-v, kind="stable")
            best = v[order[0]]
            with np.errstate(invalid="ignore"):  # -inf beside -inf: not decided
                decided = cand.size == 1 or bool(best - v[order[1]] > 2 * bar.max())
            if decided:
                assert c == cand[order[0]], (q, t, c, cand[order[0]])
            j = int(np.searchsorted(cand, c))
            assert v[j] == best or v[j] >= best - 2 * bar[j], (q, t, v[j], best, bar[j])
            assert out_score[q, t].view(np.uint32) == pool_score[q, c].view(np.uint32), (q, t)
            if out_kl is not None:
                got = np.float32(np.asarray(out_kl)[q, t])
                err = abs(float(got) - kl[j])
                assert err <= FACTOR * EPS * scale[j], (q, t, float(got), kl[j], err / (EPS * scale[j]))
                if scale[j] > 0:
                    worst["kl"] = max(worst["kl"], err / (EPS * scale[j]))
                if np.isfinite(vscale[j]) and vscale[j] > 0 and np.isfinite(v[j]):
                    with np.errstate(invalid="ignore", over="ignore"):
                        mine = np.float32(np.float32(np.float32(1) - lam32) * pool_score[q, c]) - np.float32(lam32 * got)
                    worst["value"] = max(worst["value"], abs(float(mine) - v[j]) / (EPS * vscale[j]))
            taken[c] = True
            mass, m = mass + dist[c], m + int(has[c])
            decided_n += int(decided)
            steps_n += 1
    return decided_n, steps_n, worst


def ckl64(kl, n, cs):
    """C_KL@c list by list: kl[q, min(c, n) - 1], NaN where n == 0. Columns follow the sorted distinct
    cutoffs."""
    cs = sorted(set(int(c) for c in cs))
    out = np.full((len(n), len(cs)), np.nan)
    for q in range(len(n)):
        for j, c in enumerate(cs):
            cp = min(c, int(n[q]))
            if cp >= 1:
                out[q, j] = float(np.asarray(kl, np.float64)[q, cp - 1])
    return out
