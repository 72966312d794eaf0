"""Per-item score boosts on the GPU (lgcn_amd.recommend.topk_rows' boost=, popularity_boost, the
harness's boost= / less_popular=; lgcn_score_filter_boost and lgcn_score_lists_boost of
csrc/lgcn_recall_boost.hip).

The oracle is tests/boost_checker.py, a numpy restatement of the contract over the UNBOOSTED scores the
library itself gives (topk_rows without a boost over candidate slices, k the slice length): it adds the
boost with one f32 addition, forms the key and ranks. So every comparison is torch.equal on the indices
and on the scores' bits; there is no tolerance."""
import functools

import numpy as np
import pytest
import torch

import boost_checker as bc

pytestmark = pytest.mark.gpu

NINF = np.float32(-np.inf)


def _emb(rng, n, d):
    return rng.standard_normal((n, d)).astype(np.float32)


def _csr(rows, dev):
    ptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    idx = np.concatenate([np.asarray(r, np.int32) for r in rows] + [np.zeros(0, np.int32)])
    return torch.from_numpy(ptr).to(dev), torch.from_numpy(idx).to(dev)


def _same(got, want):
    """Library output against the checker's (or another library output): indices equal, scores equal to the bit."""
    gi, gs = got
    wi, ws = (torch.from_numpy(x).to(gi.device) if isinstance(x, np.ndarray) else x for x in want)
    return torch.equal(gi, wi.to(gi.dtype)) and torch.equal(gs.view(torch.int32), ws.view(torch.int32))


def _count(monkeypatch):
    """The labels lgcn_amd.recommend hands _ffi.check, in call order."""
    from lgcn_amd import _ffi

    calls, check = [], _ffi.check

    def counting(rc, what):
        calls.append(what)
        return check(rc, what)

    monkeypatch.setattr(_ffi, "check", counting)
    return calls


def _quantised_boost(rng, M):
    """-0.0 on about half the items, N(0, 1) quantised to multiples of 0.25 on the rest: values collide."""
    boost = np.full(M, -0.0, np.float32)
    on = rng.random(M) < 0.5
    boost[on] = (0.25 * np.rint(rng.standard_normal(int(on.sum())) / 0.25)).astype(np.float32)
    return boost


class _Case:
    """One seeded problem with the library's unboosted scores S [Q, M] (computed once, never changed)."""

    def __init__(self, d, M, Q, rows, seed):
        rng = np.random.default_rng(seed)
        self.d, self.M, self.Q, self.rng = d, M, Q, rng
        self.users, self.cands = _emb(rng, rows, d), _emb(rng, M, d)
        self.picked = rng.choice(rows, Q, replace=False)
        self.boost = _quantised_boost(rng, M)
        # forty candidate rows duplicated, with equal boosts: exact ties, broken by index
        pairs = rng.choice(M, 80, replace=False)
        self.src, self.dst = pairs[:40], pairs[40:]
        self.cands[self.dst] = self.cands[self.src]
        self.boost[self.dst] = self.boost[self.src]
        free = np.setdiff1d(np.arange(M), pairs)
        special = rng.choice(free, 8, replace=False)
        self.minus, self.plus = np.sort(special[:5]), np.sort(special[5:])
        self.boost[self.minus], self.boost[self.plus] = -np.inf, np.inf
        self.excl = [np.sort(rng.choice(M, int(n), replace=False)).astype(np.int32) for n in rng.integers(0, 51, Q)]
        self.attr = ((rng.random(M) < 0.5).astype(np.int32) | ((rng.random(M) < 0.2).astype(np.int32) << 1))
        self.attr[rng.choice(M, 6, replace=False)] |= 4  # bit 2: exactly six items

    def device(self, dev):
        t = lambda a: torch.from_numpy(a).to(dev)
        self.U, self.C, self.P = t(self.users), t(self.cands), torch.from_numpy(self.picked)
        self.S = bc.library_scores(self.U, self.P, self.C)
        return self


# (any, all, none): everything; bit 0 (about half); not bit 1; bit 2 (six items, fewer than k = 10); a bit no item has
PALETTE = [(0, 0, 0), (1, 0, 0), (0, 0, 2), (4, 0, 0), (0, 1 << 20, 0), (1, 0, 2)]


def _masks(case, seed):
    """Per-query masks drawn from the palette (each used), topk_rows' where= and the restated predicate."""
    rng = np.random.default_rng(seed)
    pick = np.concatenate([np.arange(len(PALETTE)), rng.integers(0, len(PALETTE), case.Q - len(PALETTE))])
    any_, all_, none = (np.array([PALETTE[p][c] for p in pick], np.int64) for c in range(3))
    a = case.attr[None, :].astype(np.int64)
    passes = ((a & none[:, None]) == 0) & ((a & all_[:, None]) == all_[:, None]) & \
        ((any_[:, None] == 0) | ((a & any_[:, None]) != 0))
    return (torch.from_numpy(any_), torch.from_numpy(all_), torch.from_numpy(none)), passes, pick


@functools.lru_cache(maxsize=None)
def _dense_case(d):
    """300 queries picked from 900 rows, M = 2,000, exclusion rows of 0 - 50 entries; beside them three
    queries made so that the special values show: query 0 may only be served the five -inf items and
    three others, query 1 only the -inf items, and query 2 is a duplicated candidate's own row with
    the +inf items excluded and a boost of 8 on both copies, so they lead its list."""
    c = _Case(d, 2000, 300, 900, 1000 + d)
    keep0 = np.concatenate([c.minus, np.setdiff1d(np.arange(c.M), np.concatenate([c.minus, c.plus]))[:3]])
    c.excl[0] = np.setdiff1d(np.arange(c.M), keep0).astype(np.int32)
    c.excl[1] = np.setdiff1d(np.arange(c.M), c.minus).astype(np.int32)
    c.users[c.picked[2]] = c.cands[c.src[0]]
    c.boost[[c.src[0], c.dst[0]]] = 8.0  # above every other finite sum (|score| <= 1, |boost| of a few)
    c.excl[2] = c.plus.astype(np.int32)
    return c.device(torch.device("cuda:0"))


@functools.lru_cache(maxsize=None)
def _list_case():
    """M = 5,000 at d = 64 for cap = 512: above the dense capacity, so _run_filtered runs (the first
    thresholds from every tenth candidate)."""
    return _Case(64, 5000, 200, 400, 77).device(torch.device("cuda:0"))


LIST_KW = dict(cap=512)


@pytest.mark.parametrize("k", [1, 10, 100])
@pytest.mark.parametrize("d", [8, 64, 100, 256])
def test_dense_grid_equals_the_checker(gpu, d, k):
    from lgcn_amd.recommend import topk_rows

    c = _dense_case(d)
    boost = torch.from_numpy(c.boost).to(gpu)
    got = topk_rows(c.U, c.P, c.C, k, excl=_csr(c.excl, gpu), boost=boost)
    want = bc.boosted_topk(c.S, c.boost, k, excl=c.excl)
    assert _same(got, want)
    gi, gs = got[0].cpu().numpy(), got[1].cpu().numpy()
    # the special values actually occur: a +inf winner, a -inf filler, a tie broken by index
    assert np.isposinf(gs[:, 0]).sum() > 200 and np.isin(gi[np.isposinf(gs[:, 0]), 0], c.plus).all()
    assert gi[1, 0] == c.minus[0] and gs[1, 0] == NINF  # served although it is -inf: nothing else is left
    n1 = min(k, 5)
    assert gi[1, :n1].tolist() == c.minus[:n1].tolist() and (gi[1, n1:] == -1).all()
    if k >= 10:
        assert gi[0, 3:8].tolist() == c.minus.tolist() and (gs[0, 3:8] == NINF).all() and (gi[0, 8:] == -1).all()
        assert np.isfinite(gs[0, :3]).all()
    lo, hi = sorted((int(c.src[0]), int(c.dst[0])))
    assert gi[2, 0] == lo  # the two copies of query 2's own row tie at the top: the lower index first
    if k >= 10:
        assert gi[2, 1] == hi and gs[2, 0].view(np.uint32) == gs[2, 1].view(np.uint32)
        tied = (gs[:, 1:].view(np.uint32) == gs[:, :-1].view(np.uint32)) & (gi[:, 1:] >= 0) & np.isfinite(gs[:, 1:])
        assert tied.sum() > 1 and (gi[:, 1:][tied] > gi[:, :-1][tied]).all()


def test_a_nan_boost_ranks_first_unless_excluded(gpu):
    from lgcn_amd.recommend import topk_rows

    c = _dense_case(64)
    boost = c.boost.copy()
    special = np.concatenate([c.minus, c.plus, c.src[:1], c.dst[:1]])
    q5 = next(q for q in range(3, c.Q) if len(np.setdiff1d(c.excl[q], special)))
    item = int(np.setdiff1d(c.excl[q5], special)[0])  # query q5 excludes it, most do not
    boost[item] = np.nan
    got = topk_rows(c.U, c.P, c.C, 10, excl=_csr(c.excl, gpu), boost=torch.from_numpy(boost).to(gpu))
    assert _same(got, bc.boosted_topk(c.S, boost, 10, excl=c.excl))
    gi, gs = got[0].cpu().numpy(), got[1].cpu().numpy()
    has = np.array([item not in set(r.tolist()) for r in c.excl])
    assert has.sum() > 250 and not has[q5]
    assert (gi[has, 0] == item).all() and np.isnan(gs[has, 0]).all() and not np.isnan(gs[has, 1:]).any()
    assert not (gi[~has] == item).any() and not np.isnan(gs[~has]).any()


def test_thresholded_path_with_a_spread_boost(gpu, monkeypatch):
    from lgcn_amd.recommend import topk_rows

    c = _list_case()
    calls = _count(monkeypatch)
    for k in (10, 40):
        got = topk_rows(c.U, c.P, c.C, k, excl=_csr(c.excl, gpu), boost=torch.from_numpy(c.boost).to(gpu), **LIST_KW)
        assert _same(got, bc.boosted_topk(c.S, c.boost, k, excl=c.excl))
    assert "lgcn_score_filter_boost(subset)" in calls and "lgcn_score_filter_boost" in calls
    assert not any(x.startswith("lgcn_score_filter") and "boost" not in x for x in calls)
    assert "lgcn_score_filter_boost(dense)" not in calls


def test_a_boost_the_subset_misses_overflows_and_tightens(gpu, monkeypatch):
    """+0.5 on 600 items that the strided subset (every tenth candidate) does not hold: the first
    thresholds are unboosted scores' k-th best, nearly all 600 lifted items lie above them, a list of
    512 slots overflows and the tightening loop runs."""
    from lgcn_amd.recommend import topk_rows

    c = _list_case()
    rng = np.random.default_rng(3)
    boost = np.full(c.M, -0.0, np.float32)
    off_subset = np.nonzero(np.arange(c.M) % 10 != 0)[0]
    boost[rng.choice(off_subset, 600, replace=False)] = 0.5
    calls = _count(monkeypatch)
    got = topk_rows(c.U, c.P, c.C, 10, excl=_csr(c.excl, gpu), boost=torch.from_numpy(boost).to(gpu), **LIST_KW)
    assert calls.count("lgcn_score_filter_boost(subset)") == 1  # one block
    assert calls.count("lgcn_score_filter_boost") >= 2  # the list pass ran again after an overflow
    assert _same(got, bc.boosted_topk(c.S, boost, 10, excl=c.excl))
    assert (boost[got[0].cpu().numpy()] == 0.5).mean() > 0.9  # the lifted items, which the subset never saw


@pytest.mark.parametrize("path", ["dense", "lists"])
def test_boost_with_an_attribute_filter(gpu, monkeypatch, path):
    from lgcn_amd.recommend import topk_rows

    c, kw = (_dense_case(64), {}) if path == "dense" else (_list_case(), LIST_KW)
    where, passes, pick = _masks(c, 9)
    attrs = torch.from_numpy(c.attr).to(gpu)
    boost = c.boost
    calls = _count(monkeypatch)
    got = topk_rows(c.U, c.P, c.C, 10, excl=_csr(c.excl, gpu), attrs=attrs, where=where,
                    boost=torch.from_numpy(boost).to(gpu), **kw)
    assert _same(got, bc.boosted_topk(c.S, boost, 10, excl=c.excl, passes=passes))
    assert any(x.startswith("lgcn_score_filter_boost") for x in calls)
    assert not any(x.startswith("lgcn_score_filter") and "boost" not in x for x in calls)
    gi = got[0].cpu().numpy()
    nothing, six = np.nonzero(pick == 4)[0], np.nonzero(pick == 3)[0]
    assert len(nothing) and (gi[nothing] == -1).all() and torch.isinf(got[1][torch.from_numpy(nothing).to(gpu)]).all()
    for q in six:  # fewer than k passing items: the list is padded
        n = int((passes[q] & ~np.isin(np.arange(c.M), c.excl[q])).sum())
        assert 0 < n <= 6 and (gi[q, :n] >= 0).all() and (gi[q, n:] == -1).all()


def _among_rows(c, seed):
    """Rows of 0 - 200 entries in any order, with entries named twice and entries equal to -1 and to M,
    and one of 1,300 entries (above the 512 of the one-wave kernel)."""
    rng = np.random.default_rng(seed)
    rows = []
    for n in rng.integers(0, 201, c.Q):
        row = rng.choice(c.M, int(n), replace=False)
        if n >= 4:
            row[1], row[2], row[3] = row[0], -1, c.M
        rows.append(rng.permutation(row).astype(np.int32))
    rows[5] = np.concatenate([rng.integers(0, c.M, 1290), [-1, c.M] * 5]).astype(np.int32)
    rows[5] = rng.permutation(rows[5])
    rows[6] = np.concatenate([c.minus, c.plus, c.src[:3], c.dst[:3]]).astype(np.int32)
    return rows


@pytest.mark.parametrize("k", [10, 64])
def test_among_with_a_boost(gpu, monkeypatch, k):
    from lgcn_amd.recommend import topk_rows

    c = _dense_case(64)
    rows = _among_rows(c, 31)
    assert len(rows[5]) == 1300 and len(np.unique(rows[5])) < 1290  # the long row names candidates twice
    boost = torch.from_numpy(c.boost).to(gpu)
    calls = _count(monkeypatch)
    got = topk_rows(c.U, c.P, c.C, k, among=_csr(rows, gpu), boost=boost)
    assert calls.count("lgcn_score_lists_boost") == 1 and "lgcn_score_lists" not in calls
    assert _same(got, bc.boosted_topk(c.S, c.boost, k, among=rows))
    gi, gs = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert gi[6, :3].tolist() == c.plus.tolist() and np.isposinf(gs[6, :3]).all()
    if k >= 14:  # 3 + 6 + 5 entries: the -inf items fill the last slots of the row's list
        assert gi[6, 9:14].tolist() == c.minus.tolist() and (gs[6, 9:14] == NINF).all() and (gi[6, 14:] == -1).all()
    # with exclusion rows and an attribute filter as well
    where, passes, pick = _masks(c, 10)
    got = topk_rows(c.U, c.P, c.C, k, among=_csr(rows, gpu), excl=_csr(c.excl, gpu), attrs=torch.from_numpy(c.attr).to(gpu),
                    where=where, boost=boost)
    assert _same(got, bc.boosted_topk(c.S, c.boost, k, among=rows, excl=c.excl, passes=passes))


def test_a_minus_zero_boost_is_the_identity_and_no_boost_calls_no_boost_kernel(gpu, monkeypatch):
    from lgcn_amd.recommend import topk_rows

    dense, lists = _dense_case(64), _list_case()
    rows = _among_rows(dense, 37)
    where, _, _ = _masks(lists, 11)
    runs = [
        (dense, dict(excl=_csr(dense.excl, gpu))),
        (lists, dict(excl=_csr(lists.excl, gpu), **LIST_KW)),
        (lists, dict(excl=_csr(lists.excl, gpu), attrs=torch.from_numpy(lists.attr).to(gpu), where=where, **LIST_KW)),
        (dense, dict(among=_csr(rows, gpu), excl=_csr(dense.excl, gpu))),
    ]
    calls = _count(monkeypatch)
    for c, kw in runs:
        del calls[:]
        plain = topk_rows(c.U, c.P, c.C, 10, **kw)
        assert calls and not any("boost" in x for x in calls)  # today's sequence of library calls
        del calls[:]
        same = topk_rows(c.U, c.P, c.C, 10, boost=torch.full((c.M,), -0.0, device=gpu), **kw)
        assert any("boost" in x for x in calls)
        assert _same(same, plain)


def test_wrappers_hand_the_boost_on(gpu):
    from lgcn_amd import metrics
    from lgcn_amd.recommend import (attr_profile, rerank_calibrated, rerank_mmr, topk_items, topk_rows,
                                    topk_rows_calibrated, topk_rows_diverse, topk_users)

    rng = np.random.default_rng(41)
    U, M, d, k = 120, 700, 32, 10
    t = lambda a: torch.from_numpy(a).to(gpu)
    Ut, It = t(_emb(rng, U, d)), t(_emb(rng, M, d))
    seen = [np.sort(rng.choice(M, int(n), replace=False)).astype(np.int32) for n in rng.integers(0, 60, U)]
    scsr = _csr(seen, gpu)
    boost_np = _quantised_boost(rng, M)
    boost = t(boost_np)
    some = torch.tensor([5, 88, 4, 4, 17, 0, 119])
    S = bc.library_scores(Ut, some, It)
    got = topk_items(Ut, It, some, k, seen=scsr, boost=boost)
    assert _same(got, bc.boosted_topk(S, boost_np, k, excl=[seen[u] for u in some.tolist()]))
    # topk_users: the users are the candidates, so the boost is one value per user
    ub = t(_quantised_boost(rng, U))
    got = topk_users(Ut, It, torch.arange(9), k, boost=ub)
    assert _same(got, topk_rows(It, torch.arange(9), Ut, k, boost=ub))
    # the re-ranks see the boosted pool: relevance = the boosted score
    allq = torch.arange(U)
    pool = topk_rows(Ut, allq, It, 40, excl=scsr, boost=boost, index_dtype=torch.int32)
    div = topk_rows_diverse(Ut, allq, It, k, 0.4, pool=40, excl=scsr, boost=boost)
    want = rerank_mmr(pool[0], pool[1], It, k, 0.4)
    assert torch.equal(div.idx, want.idx.to(torch.int64)) and torch.equal(div.score.view(torch.int32), want.score.view(torch.int32))
    assert torch.equal(div.pair.view(torch.int32), want.pair.view(torch.int32))
    unboosted = topk_rows_diverse(Ut, allq, It, k, 0.4, pool=40, excl=scsr)
    assert not torch.equal(div.idx, unboosted.idx)
    attrs = t(rng.integers(1, 16, M).astype(np.int32))
    target = attr_profile(scsr, attrs)[0]
    cal = topk_rows_calibrated(Ut, allq, It, k, 0.5, attrs=attrs, target=target, pool=40, excl=scsr, boost=boost)
    want = rerank_calibrated(pool[0], pool[1], attrs, target, k, 0.5)
    assert torch.equal(cal.idx, want.idx.to(torch.int64)) and torch.equal(cal.score.view(torch.int32), want.score.view(torch.int32))
    assert torch.equal(cal.kl.view(torch.int32), want.kl.view(torch.int32))
    # evaluate_ranking: -0.0 changes nothing; -inf on every held-out item drives recall to 0
    truth = [np.sort(rng.choice(np.setdiff1d(np.arange(M), s), int(n), replace=False)) for s, n in zip(seen, rng.integers(0, 5, U))]
    tcsr = _csr(truth, gpu)
    base = metrics.evaluate_ranking(Ut, It, tcsr, ks=(5, 10), seen=scsr)
    assert base["recall@10"] > 0
    assert metrics.evaluate_ranking(Ut, It, tcsr, ks=(5, 10), seen=scsr, boost=torch.full((M,), -0.0, device=gpu)) == base
    bury = torch.full((M,), -0.0, device=gpu)
    bury[tcsr[1].long()] = float("-inf")
    gone = metrics.evaluate_ranking(Ut, It, tcsr, ks=(5, 10), seen=scsr, boost=bury)
    assert gone["users"] == base["users"] and gone["recall@10"] == 0 and gone["ndcg@10"] == 0 and gone["hit_rate@5"] == 0
    div0 = metrics.evaluate_ranking(Ut, It, tcsr, ks=(5, 10), seen=scsr, boost=boost, diversity=0.0, pool=32)
    assert {key: v for key, v in div0.items() if not key.startswith("ild@")} == \
        metrics.evaluate_ranking(Ut, It, tcsr, ks=(5, 10), seen=scsr, boost=boost)


def test_harness_serves_boosted_lists(gpu, tmp_path):
    from data.dataset_handler import MovieLensDataHandler, write_synthetic_movielens
    from lgcn_amd import metrics
    from lgcn_amd.recommend import candidate_csr, popularity_boost, seen_csr, topk_items
    from models.light_gcn import LightGCN
    from utils import ranking_eval
    from utils import recommend as R

    rp, mp = write_synthetic_movielens(str(tmp_path), 300, 200, 6000, seed=3)
    h = MovieLensDataHandler(rp, mp, device=gpu)
    U, I = h.get_num_users_items()
    torch.manual_seed(11)
    model = LightGCN(U, I, num_layers=2, dim_h=64).to(gpu)
    model.eval()
    rng = np.random.default_rng(12)
    E = h.edge_index.shape[1]
    train = h.edge_index[:, torch.from_numpy(np.sort(rng.permutation(E)[:E * 9 // 10]))]
    ids = list(h.user_id_map)[:40] + [-5]
    users = torch.tensor([h.user_id_map[u] for u in ids[:-1]], device=gpu)
    with torch.no_grad():
        ue, ie = model.get_embeddings(user_indices=torch.arange(U, device=gpu), item_indices=torch.arange(I, device=gpu))
    seen = seen_csr(train.to(gpu), U, I, by="user")
    counts = torch.bincount(seen[1].long(), minlength=I)
    assert torch.equal(counts, (lambda p: p[1:] - p[:-1])(seen_csr(train.to(gpu), U, I, by="item")[0]))

    def movies(idx, score):
        return [[(h.id_movie_map[i + U], s) for i, s in zip(ri, rs) if i >= 0] for ri, rs in zip(idx.tolist(), score.tolist())]

    def served(out):
        assert out[-1] == {"error": "Invalid user ID"}
        return [[(x["movie_id"], x["score"]) for x in lst] for lst in out[:-1]]

    B = R.recommend_for_users_boosted
    plain = R.recommend_for_users(model, ids, h, k=10, train_edge_index=train)
    assert B(model, ids, h, k=10, train_edge_index=train) == plain  # without the two arguments: the same call
    assert served(plain) == movies(*topk_items(ue, ie, users, 10, seen=seen))  # the defaults: today's lists
    assert set(plain[0][0]) == {"movie_id", "title", "score"}
    # less_popular: topk_items with popularity_boost of the training counts
    pen = popularity_boost(counts, 0.3)
    got = B(model, ids, h, k=10, train_edge_index=train, less_popular=0.3)
    assert served(got) == movies(*topk_items(ue, ie, users, 10, seen=seen, boost=pen))
    mean_pop = lambda out: np.mean([float(counts[h.movie_id_map[m] - U]) for lst in served(out) for m, _ in lst])
    assert served(got) != served(plain) and mean_pop(got) < mean_pop(plain)
    # boost=: the mapping form (unnamed movies at -0.0) and the tensor form
    lifted = [m for m, _ in served(plain)[0][7:10]]
    buried = served(plain)[0][0][0]
    mapping = {lifted[0]: 0.5, lifted[1]: 0.5, lifted[2]: 0.5, buried: float("-inf"), 10 ** 9: 1.0}
    vec = torch.full((I,), -0.0)
    for m, v in mapping.items():
        if m in h.movie_id_map:
            vec[h.movie_id_map[m] - U] = v
    want = movies(*topk_items(ue, ie, users, 10, seen=seen, boost=vec.to(gpu)))
    by_map = B(model, ids, h, k=10, train_edge_index=train, boost=mapping)
    assert served(by_map) == want
    assert served(B(model, ids, h, k=10, train_edge_index=train, boost=vec.double())) == want
    assert [m for m, _ in want[0][:3]] == sorted(lifted, key=[m for m, _ in want[0]].index) and buried not in dict(want[0])
    assert B(model, ids, h, k=10, train_edge_index=train, boost={}) == plain  # all -0.0: identical dictionaries
    both = B(model, ids, h, k=10, train_edge_index=train, boost=vec, less_popular=0.3)
    assert served(both) == movies(*topk_items(ue, ie, users, 10, seen=seen, boost=vec.to(gpu) + pen))
    # beside genres and among: topk_items with the same filter / candidate set and the penalty
    vocabulary, words = R.genre_table(h)
    drama = 1 << vocabulary.index("Drama")
    out = B(model, ids, h, k=8, train_edge_index=train, less_popular=0.3, genres=["Drama"])
    assert served(out) == movies(*topk_items(ue, ie, users, 8, seen=seen, attrs=words.to(gpu), where=(drama, 0, 0), boost=pen))
    assert served(B(model, ids, h, k=8, train_edge_index=train, less_popular=0.3, without_genres=["Drama"])) == [[] for _ in users]
    shortlist = list(h.movie_id_map)[:60]
    cptr, cidx = candidate_csr([[h.movie_id_map[m] - U for m in shortlist]], device=gpu)
    out = B(model, ids, h, k=8, train_edge_index=train, less_popular=0.3, among=shortlist)
    want8 = movies(*topk_items(ue, ie, users, 8, seen=seen, among=(cptr, cidx, torch.zeros(len(users), dtype=torch.int64)),
                               boost=pen))
    assert served(out) == want8 and any(want8)
    assert out != R.recommend_for_users(model, ids, h, k=8, train_edge_index=train, among=shortlist)
    # beside the re-ranks at strength 0 (the boosted relevance lists) and explain (the same lists, with 'because')
    ref = B(model, ids, h, k=8, train_edge_index=train, less_popular=0.3)
    assert served(ref) == movies(*topk_items(ue, ie, users, 8, seen=seen, boost=pen))
    assert B(model, ids, h, k=8, train_edge_index=train, less_popular=0.3, diversity=0.0) == ref
    assert B(model, ids, h, k=8, train_edge_index=train, less_popular=0.3, calibration=0.0) == ref
    why = B(model, ids, h, k=8, train_edge_index=train, less_popular=0.3, explain=2)
    assert served(why) == served(ref) and all("because" in x for lst in why[:-1] for x in lst)
    # histories: the counts are the movies' training degrees
    hist = [[m for m, _ in served(plain)[0][:3]], [10 ** 9], list(h.movie_id_map)[5:12]]
    hp = R.recommend_for_histories(model, hist, h, k=10, train_edge_index=train)
    hg = R.recommend_for_histories_boosted(model, hist, h, k=10, train_edge_index=train, less_popular=0.3)
    assert hg[1] == {"error": "No known movie IDs"} and hg != hp
    assert R.recommend_for_histories_boosted(model, hist, h, k=10, train_edge_index=train, boost={}) == hp
    pop = lambda lst: np.mean([float(counts[h.movie_id_map[x["movie_id"]] - U]) for x in lst])
    assert pop(hg[0]) + pop(hg[2]) < pop(hp[0]) + pop(hp[2])
    # the evaluation wrapper passes both through
    a = ranking_eval.evaluate_ranking(model, train, h.edge_index, gpu, ks=(10,))
    assert ranking_eval.evaluate_ranking_boosted(model, train, h.edge_index, gpu, ks=(10,), boost=torch.full((I,), -0.0)) == a
    b = ranking_eval.evaluate_ranking_boosted(model, train, h.edge_index, gpu, ks=(10,), less_popular=0.3)
    truth = seen_csr(h.edge_index.to(gpu), U, I, by="user")
    assert b == metrics.evaluate_ranking(ue, ie, truth, ks=(10,), seen=seen, boost=pen) and b != a


def test_padding_queries_take_nothing_under_an_infinite_or_nan_boost(gpu):
    """The raw entry point over 128 padded queries of which 5 are real, with +inf and NaN boosts (sums
    that no threshold rejects): in list mode the padding queries' counts stay 0 and nothing is stored for
    them, in dense mode their rows are not written; the real queries' keys are the checker's."""
    from lgcn_amd import _ffi
    from lgcn_amd.recall import _normalize_into

    lib = _ffi.load()
    rng = np.random.default_rng(43)
    M, D, Q, Qpad = 300, 64, 5, 128
    users, cands = torch.from_numpy(_emb(rng, Q, D)).to(gpu), torch.from_numpy(_emb(rng, M, D)).to(gpu)
    s = _ffi.stream_of(gpu)
    Qn = torch.empty((Qpad, D), dtype=torch.float32, device=gpu)
    Cn = torch.empty((M, D), dtype=torch.float32, device=gpu)
    _normalize_into(lib, users, None, Q, Qn.data_ptr(), D, Qpad, s)
    _normalize_into(lib, cands, None, M, Cn.data_ptr(), D, M, s)
    boost_np = _quantised_boost(rng, M)
    boost_np[[3, 77, 299]], boost_np[[10, 150]] = np.inf, np.nan
    boost = torch.from_numpy(boost_np).to(gpu)
    want = bc.boosted_keys(bc.library_scores(users, torch.arange(Q), cands), boost_np).astype(np.int64)
    fill = 0x5A5A5A5A
    dkey = torch.full((Qpad, M), fill, dtype=torch.int32, device=gpu)
    didx = torch.full((Qpad, M), -99, dtype=torch.int32, device=gpu)
    _ffi.check(lib.lgcn_score_filter_boost(Qn.data_ptr(), Qpad, Q, Cn.data_ptr(), M, 1, D, None, dkey.data_ptr(),
                                           didx.data_ptr(), None, M, None, None, boost.data_ptr(), s), "dense")
    torch.cuda.synchronize()
    assert (dkey[Q:] == fill).all() and (didx[Q:] == -99).all()
    assert np.array_equal(dkey[:Q].cpu().numpy().view(np.uint32).astype(np.int64), want)
    assert torch.equal(didx[:Q], torch.arange(M, dtype=torch.int32, device=gpu).expand(Q, M))
    attr = torch.ones(M, dtype=torch.int32, device=gpu)
    where = torch.zeros((Qpad, 3), dtype=torch.int32, device=gpu)
    for flt in ((None, None), (attr.data_ptr(), where.data_ptr())):
        cap = 512
        thr = torch.zeros(Qpad, dtype=torch.int32, device=gpu)  # key 0: accept everything
        lkey = torch.full((Qpad, cap), fill, dtype=torch.int32, device=gpu)
        lidx = torch.full((Qpad, cap), -99, dtype=torch.int32, device=gpu)
        ln = torch.zeros(Qpad, dtype=torch.int32, device=gpu)
        _ffi.check(lib.lgcn_score_filter_boost(Qn.data_ptr(), Qpad, Q, Cn.data_ptr(), M, 1, D, thr.data_ptr(),
                                               lkey.data_ptr(), lidx.data_ptr(), ln.data_ptr(), cap, *flt,
                                               boost.data_ptr(), s), "lists")
        torch.cuda.synchronize()
        assert ln.tolist() == [M] * Q + [0] * (Qpad - Q)
        assert (lkey[Q:] == fill).all() and (lidx[Q:] == -99).all()
        li = lidx[:Q, :M].cpu().numpy().astype(np.int64)
        assert (np.sort(li, 1) == np.arange(M)).all()
        got = lkey[:Q, :M].cpu().numpy().view(np.uint32).astype(np.int64)
        assert np.array_equal(got, np.take_along_axis(want, li, 1))
