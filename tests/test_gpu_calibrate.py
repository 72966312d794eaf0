"""Calibrated re-ranking on the GPU (lgcn_attr_profile and lgcn_rerank_calibrated in
csrc/lgcn_calibrate.hip, lgcn_amd.recommend's attr_profile / rerank_calibrated / topk_rows_calibrated /
miscalibration, the calibration keyword of lgcn_amd.metrics.evaluate_ranking and
utils.recommend.recommend_for_users) against the float64 numpy restatement of calibrate_checker.py,
whose docstring states the checks and the bar.

Random cases keep to the inputs the decided share was established on (test_gpu_rerank's
standard-normal rows, 2,000 candidates, pools from the top N; 18 genres, 0 to 3 per item with
probabilities .05 / .35 / .4 / .2; histories of 30 random items; alpha = 0.01): more than 0.9 of the
steps of each case must be decided. The grid records the worst observed error / scale ratios of value
and KL (in units of 2^-24, the bar being 64) with parity.record_stats("calibrate", ...)."""
import functools

import numpy as np
import pytest
import torch

import parity
from calibrate_checker import FACTOR, check_lists, ckl64, profile64
from test_gpu_rerank import M_RANDOM, _np, _pools, _random_set

pytestmark = pytest.mark.gpu

ALPHA = 0.01
_WORST = {"value_ratio_eps": 0.0, "kl_ratio_eps": 0.0, "bar_eps": FACTOR, "steps": 0, "decided": 0}


def _genre_words(rng, M, genres=18):
    """uint32 [M]: 0 to 3 of ``genres`` genres per item with probabilities .05 / .35 / .4 / .2."""
    count = rng.choice(4, M, p=[.05, .35, .4, .2])
    words = np.zeros(M, np.uint32)
    for i in range(M):
        for g in rng.choice(genres, count[i], replace=False):
            words[i] |= np.uint32(1 << int(g))
    return words


@functools.lru_cache(maxsize=None)
def _genres():
    """The candidates' genre words and every user's history of 30 random items as a CSR (shared, never
    changed), with the float64 targets."""
    rng = np.random.default_rng(4242)
    words = _genre_words(rng, M_RANDOM)
    rows = [rng.choice(M_RANDOM, 30, replace=False) for _ in range(900)]
    ptr = np.arange(0, 901 * 30, 30, dtype=np.int64)
    hidx = np.concatenate(rows).astype(np.int32)
    p64 = np.stack([profile64(r, None, words)[0] for r in rows])
    return words, ptr, hidx, p64


def _t(gpu, a):
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(gpu)


def _targets(gpu, picked):
    from lgcn_amd.recommend import attr_profile

    words, ptr, hidx, _ = _genres()
    return attr_profile((_t(gpu, ptr), _t(gpu, hidx)), _t(gpu, words), rows=torch.from_numpy(np.asarray(picked)))[0]


def _grid():
    cases = []
    for d in (8, 64):
        for N in (1, 63, 64, 65, 128, 1024):
            for j, k in enumerate(sorted({1, min(10, N), N}) if N <= 128 else [10]):
                Q = 5 if k == N and N >= 64 else 300
                cases.append(pytest.param(Q, d, N, k, 0.3 if (N + j) % 2 else 0.7, id=f"Q{Q}-d{d}-N{N}-k{k}"))
    return cases


@pytest.mark.parametrize("Q,d,N,k,lam", _grid())
def test_grid_matches_checker(gpu, Q, d, N, k, lam):
    from lgcn_amd.recommend import Calibrated, rerank_calibrated

    users, cands, _ = _random_set(d)
    words = _genres()[0]
    picked = np.random.default_rng(N * 1000 + k).choice(900, Q, replace=False)
    pidx, pscore = _pools(gpu, users, picked, cands, N)
    target = _targets(gpu, picked)
    out = rerank_calibrated(pidx, pscore, _t(gpu, words), target, k, lam, ALPHA)
    assert isinstance(out, Calibrated) and out.idx.dtype == torch.int64
    assert out.score.dtype == out.kl.dtype == torch.float32 and out.n.dtype == torch.int32
    assert out.idx.shape == out.score.shape == out.kl.shape == (Q, k) and out.n.shape == (Q,)
    dec, steps, worst = check_lists(*_np(pidx, pscore), words, target.cpu().numpy(), k, lam, ALPHA, *_np(*out))
    differ = int((out.idx != pidx[:, :k]).any(1).sum())
    print(f"Q={Q} d={d} N={N} k={k} lambda={lam}: decided {dec}/{steps}, value {worst['value']:.3f} eps, "
          f"kl {worst['kl']:.3f} eps (bar {FACTOR:g}), {differ} lists differ from the pool prefix")
    _WORST["value_ratio_eps"] = max(_WORST["value_ratio_eps"], worst["value"])
    _WORST["kl_ratio_eps"] = max(_WORST["kl_ratio_eps"], worst["kl"])
    _WORST["steps"] += steps
    _WORST["decided"] += dec
    parity.record_stats("calibrate", _WORST)
    assert steps == Q * k and dec > 0.9 * steps
    assert differ > 0 or k == N or N == 1  # k == N: the same items, and the prefix may be the list


def test_twins_tie_by_position_and_runs_are_bitwise_equal(gpu):
    """Every candidate twice with the same word: pool positions come in (score bits, word) pairs whose
    values are equal at every step, so the lower position of a pair is always picked first."""
    from lgcn_amd.recommend import rerank_calibrated

    users, cands, _ = _random_set(64)
    words = _genres()[0]
    half = 600
    w2 = np.concatenate([words[:half], words[:half]])
    picked = np.arange(0, 200, 5)
    top = _pools(gpu, users, picked, cands[:half], 65)
    # pool positions 2 j and 2 j + 1: candidate i and its twin i + half, with the same score bits
    pidx = torch.stack([top[0], top[0] + half], 2).reshape(40, 130)
    pscore = torch.stack([top[1], top[1]], 2).reshape(40, 130)
    pi, ps = _np(pidx, pscore)
    target = _targets(gpu, picked)
    a = rerank_calibrated(pidx, pscore, _t(gpu, w2), target, 40, 0.5, ALPHA)
    b = rerank_calibrated(pidx, pscore, _t(gpu, w2), target, 40, 0.5, ALPHA)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert torch.equal(a.kl.view(torch.int32), b.kl.view(torch.int32))
    got = a.idx.cpu().numpy()
    for q in range(got.shape[0]):
        at = {int(i): t for t, i in enumerate(got[q])}
        for i, t in at.items():
            if i >= half:
                assert i - half in at and at[i - half] < t, (q, i)  # the upper twin only after the lower one
    assert any((row >= half).any() for row in got)
    check_lists(pi, ps, w2, target.cpu().numpy(), 40, 0.5, ALPHA, *_np(*a))


@functools.lru_cache(maxsize=None)
def _property_case():
    users, cands, _ = _random_set(64)
    picked = np.random.default_rng(5).choice(900, 40, replace=False)
    return users, cands, _genres()[0], picked


def test_zero_calibration_is_the_relevance_list(gpu):
    from lgcn_amd.recommend import rerank_calibrated

    users, cands, words, picked = _property_case()
    pidx, pscore = _pools(gpu, users, picked, cands, 100)
    target = _targets(gpu, picked)
    out = rerank_calibrated(pidx, pscore, _t(gpu, words), target, 20, 0.0, ALPHA)
    assert torch.equal(out.idx, pidx[:, :20]) and torch.equal(out.score.view(torch.int32), pscore[:, :20].view(torch.int32))
    assert (out.n == 20).all()
    check_lists(*_np(pidx, pscore), words, target.cpu().numpy(), 20, 0.0, ALPHA, *_np(*out))  # kl against the checker


def test_smaller_k_is_a_prefix(gpu):
    from lgcn_amd.recommend import rerank_calibrated

    users, cands, words, picked = _property_case()
    pidx, pscore = _pools(gpu, users, picked, cands, 100)
    target, w = _targets(gpu, picked), _t(gpu, words)
    a, b = rerank_calibrated(pidx, pscore, w, target, 5, 0.5, ALPHA), rerank_calibrated(pidx, pscore, w, target, 20, 0.5, ALPHA)
    assert torch.equal(a.idx, b.idx[:, :5]) and torch.equal(a.score, b.score[:, :5]) and torch.equal(a.kl, b.kl[:, :5])
    assert not torch.equal(b.idx, pidx[:, :20])  # the re-rank did something


def test_a_zero_target_row_gives_the_pool_order(gpu):
    from lgcn_amd.recommend import rerank_calibrated

    users, cands, words, picked = _property_case()
    pidx, pscore = _pools(gpu, users, picked, cands, 100)
    target = _targets(gpu, picked).clone()
    target[::2] = 0
    out = rerank_calibrated(pidx, pscore, _t(gpu, words), target, 20, 0.7, ALPHA)
    assert torch.equal(out.idx[::2], pidx[::2, :20]) and (out.kl[::2] == 0).all() and (out.n == 20).all()
    assert not torch.equal(out.idx[1::2], pidx[1::2, :20]) and (out.kl[1::2] > 0).all()
    check_lists(*_np(pidx, pscore), words, target.cpu().numpy(), 20, 0.7, ALPHA, *_np(*out))


def test_full_calibration_to_one_genre_takes_that_genre_first(gpu):
    """lambda = 1, a target with all its weight on one genre and one-genre words: the entries of that
    genre tie at every step (KL stays at its minimum) and come in pool order, before anything else."""
    from lgcn_amd.recommend import rerank_calibrated

    users, cands, _, picked = _property_case()
    rng = np.random.default_rng(77)
    words = (np.uint32(1) << rng.integers(0, 6, M_RANDOM).astype(np.uint32)).astype(np.uint32)
    pidx, pscore = _pools(gpu, users, picked, cands, 100)
    target = torch.zeros((40, 32), device=gpu)
    target[:, 3] = 1.0
    out = rerank_calibrated(pidx, pscore, _t(gpu, words), target, 100, 1.0, ALPHA)
    pi, gi = pidx.cpu().numpy(), out.idx.cpu().numpy()
    for q in range(40):
        mine = [i for i in pi[q] if words[i] == 8]
        rest = [i for i in pi[q] if words[i] != 8]
        assert 0 < len(mine) < 100 and gi[q].tolist() == mine + rest
    check_lists(pi, pscore.cpu().numpy(), words, target.cpu().numpy(), 100, 1.0, ALPHA, *_np(*out))


def test_strided_and_int32_pools_equal_the_contiguous_int64_one(gpu):
    from lgcn_amd.recommend import rerank_calibrated

    users, cands, words, picked = _property_case()
    pidx, pscore = _pools(gpu, users, picked, cands, 100)
    target, w = _targets(gpu, picked), _t(gpu, words)
    want = rerank_calibrated(pidx, pscore, w, target, 10, 0.7, ALPHA)
    wide_i = torch.full((40, 117), 3, dtype=torch.int64, device=gpu)
    wide_s = torch.full((40, 117), 9.0, device=gpu)
    wide_i[:, 5:105], wide_s[:, 5:105] = pidx, pscore
    for dtype in (torch.int64, torch.int32):
        views = (wide_i.to(dtype)[:, 5:105], wide_s[:, 5:105])
        assert not views[0].is_contiguous() and views[0].stride(0) == 117
        got = rerank_calibrated(*views, w, target, 10, 0.7, ALPHA)
        assert got.idx.dtype == dtype and torch.equal(got.idx.to(torch.int64), want.idx)
        assert torch.equal(got.score, want.score) and torch.equal(got.kl, want.kl) and torch.equal(got.n, want.n)
    # leading dimensions that differ between the two tensors are served too (made contiguous)
    got = rerank_calibrated(wide_i[:, 5:105], pscore, w, target, 10, 0.7, ALPHA)
    assert torch.equal(got.idx, want.idx) and torch.equal(got.kl, want.kl)
    # no queries
    none = rerank_calibrated(pidx[:0], pscore[:0], w, target[:0], 10, 0.5, ALPHA)
    assert none.idx.shape == none.score.shape == none.kl.shape == (0, 10) and none.n.shape == (0,)
    assert none.idx.dtype == torch.int64


def test_ineligible_entries_are_skipped(gpu):
    """-1, M and 2**31 - 1 in a pool (and a value past int32 in an int64 pool): the output is what the
    pool without those positions gives; k above the eligible count leaves the right tails."""
    from lgcn_amd.recommend import rerank_calibrated

    users, cands, words, picked = _property_case()
    pidx, pscore = _pools(gpu, users, picked, cands, 70)
    target, w = _targets(gpu, picked), _t(gpu, words)
    holes = [0, 6, 64, 69]  # positions in both lane slots, the first and the last
    keep = [p for p in range(70) if p not in holes]
    want = rerank_calibrated(pidx[:, keep].contiguous(), pscore[:, keep].contiguous(), w, target, 30, 0.5, ALPHA)
    for dtype, junk in ((torch.int32, [-1, M_RANDOM, 2**31 - 1, -7]), (torch.int64, [-1, M_RANDOM, 2**31 - 1, 2**40 + 5])):
        bad = pidx.to(dtype).clone()
        bad[:, holes] = torch.tensor(junk, dtype=dtype, device=gpu)
        got = rerank_calibrated(bad, pscore, w, target, 30, 0.5, ALPHA)
        assert torch.equal(got.idx.to(torch.int64), want.idx) and torch.equal(got.score, want.score)
        assert torch.equal(got.kl, want.kl) and (got.n == 30).all()
        check_lists(*_np(bad, pscore), words, target.cpu().numpy(), 30, 0.5, ALPHA, *_np(*got))
    got = rerank_calibrated(bad, pscore, w, target, 70, 0.5, ALPHA)
    assert (got.n == 66).all() and (got.idx[:, 66:] == -1).all() and torch.isneginf(got.score[:, 66:]).all()
    assert (got.kl[:, 66:] == 0).all()
    check_lists(*_np(bad, pscore), words, target.cpu().numpy(), 70, 0.5, ALPHA, *_np(*got))


def test_genreless_items_never_change_kl(gpu):
    """An item with a zero word adds nothing to the list's distribution and is counted out of m: the KL
    after picking it is the KL before, bit for bit."""
    from lgcn_amd.recommend import rerank_calibrated

    users, cands, words, picked = _property_case()
    words = words.copy()
    words[::3] = 0
    pidx, pscore = _pools(gpu, users, picked, cands, 100)
    target = _targets(gpu, picked)
    out = rerank_calibrated(pidx, pscore, _t(gpu, words), target, 100, 0.3, ALPHA)
    gi, gk = out.idx.cpu().numpy(), out.kl.cpu().numpy()
    check_lists(*_np(pidx, pscore), words, target.cpu().numpy(), 100, 0.3, ALPHA, *_np(*out))
    seen = 0
    for q in range(40):
        for t in range(1, 100):
            if words[gi[q, t]] == 0:
                assert gk[q, t].view(np.uint32) == gk[q, t - 1].view(np.uint32), (q, t)
                seen += 1
    assert seen > 500
    # a list of genre-less items only: m stays 0 and the KL is that of the empty list, -ln(alpha) * sum(p)
    only = rerank_calibrated(pidx, pscore, torch.zeros(M_RANDOM, dtype=torch.int32, device=gpu), target, 5, 0.5, ALPHA)
    assert torch.equal(only.idx, pidx[:, :5])
    np.testing.assert_allclose(only.kl.cpu().numpy(), np.repeat(-np.log(np.float64(np.float32(ALPHA)))
                               * target.double().sum(1).cpu().numpy()[:, None], 5, 1), rtol=1e-5)


def _history_case(rng, M, lengths):
    rows = [rng.integers(0, M, n) for n in lengths]
    ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return rows, ptr, np.concatenate(rows + [np.zeros(0, np.int64)]).astype(np.int32)


def _ulps(got, want64):
    """|got - want| in f32 ulps of want (got f32, want float64)."""
    want32 = want64.astype(np.float32)
    ulp = np.spacing(np.maximum(np.abs(want32), np.float32(1e-30)))
    return np.abs(got.astype(np.float64) - want64) / ulp.astype(np.float64)


def test_attr_profile_matches_float64_and_is_batch_invariant(gpu):
    from lgcn_amd.recommend import attr_profile

    rng = np.random.default_rng(31)
    M = 3000
    words = _genre_words(rng, M, genres=32)
    words[5] = 0xFFFFFFFF
    lengths = [0, 1, 63, 64, 65, 512, 513, 5000, 2, 1300]
    rows, ptr, hidx = _history_case(rng, M, lengths)
    hidx = hidx.copy()
    hidx[rng.random(hidx.size) < 0.05] = -1          # out of range, below
    hidx[rng.random(hidx.size) < 0.05] = M + 7       # and above
    wts = rng.choice(np.array([1.0, 0.5, 3.25, 0.0, -2.0, np.nan], np.float32), hidx.size, p=[.4, .2, .2, .07, .07, .06])
    w_dev, tp, ti = _t(gpu, words), _t(gpu, ptr), _t(gpu, hidx)
    for weights in (None, wts):
        tw = None if weights is None else _t(gpu, weights)
        p, W = attr_profile((tp, ti), w_dev, weights=tw)
        assert p.shape == (len(lengths), 32) and W.shape == (len(lengths),) and p.dtype == W.dtype == torch.float32
        gp, gW = _np(p, W)
        for q, n in enumerate(lengths):
            e = slice(int(ptr[q]), int(ptr[q + 1]))
            want, wantW = profile64(hidx[e], None if weights is None else weights[e], words)
            assert _ulps(gp[q], want).max() <= 1.0, (q, n, _ulps(gp[q], want).max())
            assert gW[q] == np.float32(wantW)
            assert (wantW > 0) == (gp[q].sum() > 0.99)
        assert (gp[0] == 0).all() and gW[0] == 0
        # alone, through rows=, at another batch position, beside a row outside the CSR: the same bits
        order = [7, 99, 3, 6, 0, 5, 7, -4, 9, 1]
        q2, W2 = attr_profile((tp, ti), w_dev, rows=torch.tensor(order), weights=tw)
        g2, gW2 = _np(q2, W2)
        for j, r in enumerate(order):
            if 0 <= r < len(lengths):
                assert (g2[j].view(np.uint32) == gp[r].view(np.uint32)).all() and gW2[j] == gW[r], (j, r)
            else:
                assert (g2[j] == 0).all() and gW2[j] == 0
        for r in (5, 6, 7):
            alone, _ = attr_profile((tp, ti, torch.tensor([r])), w_dev, weights=tw)
            assert torch.equal(alone[0].view(torch.int32), p[r].view(torch.int32))
        again, _ = attr_profile((tp, ti), w_dev, weights=tw)
        assert torch.equal(again.view(torch.int32), p.view(torch.int32))
    # nothing to profile
    empty = attr_profile((torch.zeros(4, dtype=torch.int64), torch.zeros(0, dtype=torch.int32)), w_dev)
    assert empty[0].shape == (3, 32) and (empty[0] == 0).all() and (empty[1] == 0).all() and empty[0].is_cuda
    none = attr_profile((tp, ti), w_dev, rows=torch.zeros(0, dtype=torch.int64))
    assert none[0].shape == (0, 32) and none[1].shape == (0,)


def test_topk_rows_calibrated_is_topk_rows_then_rerank(gpu):
    from lgcn_amd.recommend import attr_profile, candidate_csr, miscalibration, rerank_calibrated, topk_rows, \
        topk_rows_calibrated

    users, cands, words, picked = _property_case()
    _, ptr, hidx, _ = _genres()
    t = lambda a: _t(gpu, a)
    w, pk = t(words), torch.from_numpy(picked)
    hist = (t(ptr), t(hidx), pk)
    target = attr_profile(hist, w)[0]
    excl = hist  # the history is what the user has seen
    for kw in (dict(), dict(where=(0b111, 0, 1 << 4)), dict(among=candidate_csr([np.arange(q, 2000, 3) for q in range(40)]))):
        tk = dict(kw, attrs=w) if "where" in kw else kw
        pidx, pscore = topk_rows(t(users), pk, t(cands), 128, excl=excl, **tk)
        want = rerank_calibrated(pidx, pscore, w, target, 20, 0.6, ALPHA)
        got = topk_rows_calibrated(t(users), pk, t(cands), 20, 0.6, attrs=w, history=hist, pool=128, excl=excl, **kw)
        same = topk_rows_calibrated(t(users), pk, t(cands), 20, 0.6, attrs=w, target=target, pool=128, excl=excl, **kw)
        assert got.idx.dtype == torch.int64
        for a, b, c in zip(got, want, same):
            assert torch.equal(a, b) and torch.equal(a, c)
        gi = got.idx.cpu().numpy()
        assert not np.isin(gi[0], hidx[picked[0] * 30:picked[0] * 30 + 30]).any()
        if "where" in kw:
            assert ((words[gi] & 0b111) != 0).all() and ((words[gi] & (1 << 4)) == 0).all()
        if "among" in kw:
            assert all((gi[q] % 3 == q % 3).all() for q in range(40))
        dec, steps, _ = check_lists(*_np(pidx, pscore), words, target.cpu().numpy(), 20, 0.6, ALPHA, *_np(*got))
        assert dec > 0.9 * steps
        ckl = miscalibration(got.kl, got.n, [5, 20])
        np.testing.assert_array_equal(ckl.cpu().numpy(), ckl64(*_np(got.kl, got.n), [5, 20]))
    # the default pool max(4 * 10, 64) = 64, int32 indices handed on, the pool clamped to M and to the limit
    got = topk_rows_calibrated(t(users), pk, t(cands), 10, 0.3, attrs=w, target=target, index_dtype=torch.int32)
    want = rerank_calibrated(*_pools(gpu, users, picked, cands, 64), w, target, 10, 0.3, ALPHA)
    assert got.idx.dtype == torch.int32 and torch.equal(got.idx.to(torch.int64), want.idx) and torch.equal(got.kl, want.kl)
    few = topk_rows_calibrated(t(users), pk, t(cands[:30]), 10, 0.3, attrs=w[:30], target=target)
    want = rerank_calibrated(*_pools(gpu, users, picked, cands[:30], 30), w[:30], target, 10, 0.3, ALPHA)
    assert torch.equal(few.idx, want.idx) and torch.equal(few.kl, want.kl)
    big = topk_rows_calibrated(t(users), pk[:3], t(cands), 10, 0.3, attrs=w, target=target[:3], pool=5000)
    want = rerank_calibrated(*_pools(gpu, users, picked[:3], cands, 1024), w, target[:3], 10, 0.3, ALPHA)
    assert torch.equal(big.idx, want.idx) and torch.equal(big.kl, want.kl)
    with pytest.raises(ValueError, match="pool=5 is below k=10"):
        topk_rows_calibrated(t(users), pk, t(cands), 10, 0.3, attrs=w, target=target, pool=5)
    with pytest.raises(ValueError, match="target"):
        topk_rows_calibrated(t(users), pk, t(cands), 10, 0.3, attrs=w, target=target[:7])
    # a 2-tuple history has a row per query
    first40 = topk_rows_calibrated(t(users), torch.arange(40), t(cands), 10, 0.5, attrs=w, history=(t(ptr), t(hidx)))
    named = topk_rows_calibrated(t(users), torch.arange(40), t(cands), 10, 0.5, attrs=w,
                                 history=(t(ptr), t(hidx), torch.arange(40)))
    assert torch.equal(first40.idx, named.idx) and torch.equal(first40.kl, named.kl)


def test_evaluate_ranking_with_calibration(gpu):
    from lgcn_amd import metrics
    from lgcn_amd.recommend import attr_profile, topk_rows_calibrated

    users, cands, words, _ = _property_case()
    rng = np.random.default_rng(14)
    t = lambda a: _t(gpu, a)
    csr = lambda rows: (t(np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)),
                        t(np.concatenate(rows + [np.zeros(0, np.int64)]).astype(np.int32)))
    words = words.copy()
    seen_rows = [np.sort(rng.choice(M_RANDOM, 20, replace=False)) for _ in range(900)]
    for u in range(0, 900, 30):  # every tenth evaluated user has seen genre-less movies only: no target
        words[seen_rows[u]] = 0
    truth_rows = [np.sort(rng.choice(np.setdiff1d(np.arange(M_RANDOM), seen_rows[u]), 15, replace=False))
                  if u % 3 == 0 else np.zeros(0, np.int64) for u in range(900)]
    seen, truth, w = csr(seen_rows), csr(truth_rows), t(words)
    ks = (5, 10, 20)
    today = metrics.evaluate_ranking(t(users), t(cands), truth, ks=ks, seen=seen)
    assert set(today) == {"users"} | {f"{m}@{c}" for m in metrics.METRICS for c in ks}  # None: the old key set
    measured = metrics.evaluate_ranking(t(users), t(cands), truth, ks=ks, seen=seen, calibration=0.0, attrs=w)
    assert set(measured) == set(today) | {f"ckl@{c}" for c in ks}
    assert all(measured[key] == today[key] for key in today)
    who = torch.arange(0, 900, 3)
    hist = (seen[0], seen[1], who)
    target, weight = attr_profile(hist, w)
    lists = topk_rows_calibrated(t(users), who, t(cands), 20, 0.0, attrs=w, target=target, excl=hist)
    has = weight.cpu().numpy() > 0
    assert has.sum() == 270
    pool = _np(*_pools(gpu, users, who.numpy(), cands, 80, excl=hist))  # the default pool: max(4 * 20, 64)
    check_lists(*pool, words, target.cpu().numpy(), 20, 0.0, ALPHA, *_np(*lists))  # every kl within the bar of float64
    want = ckl64(*_np(lists.kl, lists.n), ks)[has].mean(0)  # the checker's mean, given the kernel's lists
    for j, c in enumerate(ks):
        assert measured[f"ckl@{c}"] == pytest.approx(want[j], rel=1e-9)
    calibrated = metrics.evaluate_ranking(t(users), t(cands), truth, ks=ks, seen=seen, calibration=0.7, attrs=w, pool=100)
    assert calibrated["users"] == today["users"] == 300
    assert all(calibrated[f"ckl@{c}"] < measured[f"ckl@{c}"] for c in ks)
    assert any(calibrated[key] != today[key] for key in today)
    # users without truth are not averaged, for C_KL either
    everyone = metrics.evaluate_ranking(t(users), t(cands), truth, ks=ks, seen=seen, calibration=0.7, attrs=w, pool=100,
                                        users=torch.arange(900))
    assert everyone["users"] == 300
    assert all(everyone[key] == pytest.approx(calibrated[key], rel=1e-12) for key in calibrated)
    # an explicit history equals the default, and nobody with a target: nan
    explicit = metrics.evaluate_ranking(t(users), t(cands), truth, ks=ks, seen=seen, calibration=0.7, attrs=w, pool=100,
                                        history=seen)
    assert explicit == calibrated
    nobody = metrics.evaluate_ranking(t(users), t(cands), truth, ks=ks, seen=seen, calibration=0.5,
                                      attrs=torch.zeros_like(w), users=torch.arange(0, 30, 3))
    assert nobody["users"] == 10 and all(np.isnan(nobody[f"ckl@{c}"]) for c in ks)
    with pytest.raises(ValueError, match="calibration and diversity"):
        metrics.evaluate_ranking(t(users), t(cands), truth, ks=ks, seen=seen, calibration=0.5, diversity=0.5, attrs=w)


def test_recommend_for_users_with_calibration(gpu, tmp_path):
    import pandas as pd

    from data.dataset_handler import MovieLensDataHandler, write_synthetic_movielens
    from lgcn_amd.recommend import attr_profile, seen_csr, topk_rows
    from models.light_gcn import LightGCN
    from utils import ranking_eval
    from utils import recommend as R

    rp, mp = write_synthetic_movielens(str(tmp_path), 300, 200, 6000, seed=3)
    movies = pd.read_csv(mp)
    rng = np.random.default_rng(9)
    names = ["Action", "Comedy", "Drama", "Horror", "Romance", "Sci-Fi", "Thriller", "Western"]
    movies["genres"] = ["|".join(sorted(rng.choice(names, n, replace=False))) or R.NO_GENRES
                        for n in rng.choice(4, len(movies), p=[.05, .35, .4, .2])]
    movies.to_csv(mp, index=False)
    h = MovieLensDataHandler(rp, mp, device=gpu)
    U, I = h.get_num_users_items()
    torch.manual_seed(11)
    model = LightGCN(U, I, num_layers=2, dim_h=64).to(gpu)
    model.eval()
    title_of = dict(zip(h.movies["movieId"].tolist(), h.movies["title"].tolist()))
    user_ids = list(h.user_id_map)[:63]
    ids = user_ids[:30] + [-5] + user_ids[30:]
    served = R.recommend_for_users(model, ids, h, k=10, calibration=0.5)
    assert len(served) == 64 and served[30] == {"error": "Invalid user ID"}
    lists = served[:30] + served[31:]
    assert all(len(row) == 10 and all(title_of[x["movie_id"]] == x["title"] for x in row) for row in lists)
    # the pools those lists were picked from (the default pool of 64, seen movies left out) and the targets
    uidx = torch.tensor([h.user_id_map[u] for u in user_ids], device=gpu)
    uw, iw = model.user_embedding.weight.detach(), model.item_embedding.weight.detach()
    ptr, seen = seen_csr(h.edge_index.to(gpu), U, I, by="user")
    vocabulary, attrs = R.genre_table(h)
    assert vocabulary == names
    pidx, pscore = topk_rows(uw, uidx, iw, 64, excl=(ptr, seen, uidx))
    target = attr_profile((ptr, seen, uidx), attrs.to(gpu))[0]
    got_idx = np.array([[h.movie_id_map[x["movie_id"]] - U for x in row] for row in lists])
    got_score = np.array([[x["score"] for x in row] for row in lists], np.float32)
    dec, steps, _ = check_lists(*_np(pidx, pscore), attrs.numpy(), target.cpu().numpy(), 10, 0.5, ALPHA, got_idx, got_score,
                                None, None)
    assert steps == 630 and dec > 0.9 * steps
    relevance = R.recommend_for_users(model, user_ids, h, k=10)
    assert [[x["movie_id"] for x in row] for row in relevance] != [[x["movie_id"] for x in row] for row in lists]
    assert R.recommend_for_users(model, user_ids, h, k=10, calibration=0.0) == relevance
    assert R.recommend_for_users(model, user_ids, h, k=10, calibration=None) == relevance
    # explain= still attaches reasons, to the calibrated list
    why = R.recommend_for_users(model, user_ids[:5], h, k=10, calibration=0.5, explain=2)
    assert [[x["movie_id"] for x in row] for row in why] == [[x["movie_id"] for x in row] for row in lists[:5]]
    assert all(0 < len(x["because"]) <= 2 for row in why for x in row)
    # with genres=: comedies only, calibrated within them
    genre_of = dict(zip(h.movies["movieId"].tolist(), h.movies["genres"].tolist()))
    comedies = R.recommend_for_users(model, user_ids[:5], h, k=10, calibration=0.5, genres=["Comedy"])
    assert all(len(row) == 10 and all("Comedy" in genre_of[x["movie_id"]] for x in row) for row in comedies)
    with pytest.raises(ValueError, match="diversity and calibration"):
        R.recommend_for_users(model, user_ids[:5], h, k=10, calibration=0.5, diversity=0.5)
    # a stranger's history: the target is the history's own mix
    watched = [[x["movie_id"] for x in row[:6]] for row in relevance[:4]]
    strangers = R.recommend_for_histories(model, watched, h, k=10, calibration=0.5)
    assert all(len(row) == 10 for row in strangers)
    assert R.recommend_for_histories(model, watched, h, k=10, calibration=0.0) == R.recommend_for_histories(model, watched, h, k=10)
    # the harness-level evaluation passes the keywords through
    ei = h.edge_index
    out = ranking_eval.evaluate_ranking(model, ei[:, ::2], ei[:, 1::2], gpu, ks=(5, 10), calibration=0.5, pool=40,
                                        data_handler=h)
    assert {"ckl@5", "ckl@10", "recall@10"} <= set(out) and 0.0 < out["ckl@10"] < 10.0
    assert "ckl@5" not in ranking_eval.evaluate_ranking(model, ei[:, ::2], ei[:, 1::2], gpu, ks=(5, 10))
