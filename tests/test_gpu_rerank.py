"""Greedy MMR re-ranking on the GPU (lgcn_rerank_mmr in csrc/lgcn_rerank.hip, lgcn_amd.recommend's
rerank_mmr / topk_rows_diverse / intra_list_diversity, the diversity keyword of
lgcn_amd.metrics.evaluate_ranking and utils.recommend.recommend_for_users) against the float64
numpy restatement of rerank_checker.py, whose docstring states the checks and the bar.

Random cases keep to the inputs the decided share was established on (standard-normal rows, 2,000
candidates, pools from the top N): more than 0.9 of the steps of each case must be decided."""
import functools

import numpy as np
import pytest
import torch

from rerank_checker import BAR, check_lists, ild64, mmr64, unit_rows64

pytestmark = pytest.mark.gpu

M_RANDOM = 2000


@functools.lru_cache(maxsize=None)
def _random_set(d):
    """Users, candidates and the candidates' float64 unit rows for width d (shared, never changed)."""
    rng = np.random.default_rng(7000 + d)
    users = rng.standard_normal((900, d)).astype(np.float32)
    cands = rng.standard_normal((M_RANDOM, d)).astype(np.float32)
    return users, cands, unit_rows64(cands)


def _pools(gpu, users, picked, cands, N, excl=None, index_dtype=torch.int64):
    from lgcn_amd.recommend import topk_rows

    t = lambda a: torch.from_numpy(a).to(gpu)
    return topk_rows(t(users), torch.from_numpy(np.asarray(picked)), t(cands), N, excl=excl, index_dtype=index_dtype)


def _np(*ts):
    return [t.cpu().numpy() for t in ts]


def _grid():
    cases = []
    for d in (8, 64, 100, 256):
        for N in (1, 63, 64, 65, 128) + ((512,) if d == 64 else ()):  # 512 * 64 * 4: the LDS limit exactly
            for j, k in enumerate(sorted({1, min(10, N), N})):
                Q = 1 if N == 1 else 300 if N <= 65 and k <= 10 else 5
                cases.append(pytest.param(Q, d, N, k, 0.3 if (N + j) % 2 else 0.7, id=f"Q{Q}-d{d}-N{N}-k{k}"))
    return cases


@pytest.mark.parametrize("Q,d,N,k,delta", _grid())
def test_grid_matches_checker(gpu, Q, d, N, k, delta):
    from lgcn_amd.recommend import rerank_mmr

    users, cands, U = _random_set(d)
    picked = np.random.default_rng(N * 1000 + k).choice(900, Q, replace=False)
    pidx, pscore = _pools(gpu, users, picked, cands, N)
    out = rerank_mmr(pidx, pscore, torch.from_numpy(cands).to(gpu), k, delta)
    assert out.idx.dtype == torch.int64 and out.score.dtype == out.pair.dtype == torch.float32
    assert out.n.dtype == torch.int32 and out.idx.shape == out.score.shape == out.pair.shape == (Q, k)
    dec, steps = check_lists(*_np(pidx, pscore), U, k, delta, *_np(*out))
    print(f"Q={Q} d={d} N={N} k={k} delta={delta}: decided {dec}/{steps}")
    assert steps == Q * k and dec > 0.9 * steps


def _half_rows(rng, n, distinct):
    """n rows of width 8 with four entries of +-0.5 (unit rows, every dot a multiple of 0.25), drawn
    with repetition from ``distinct`` patterns."""
    base = np.zeros((distinct, 8), np.float32)
    for r in range(distinct):
        base[r, rng.choice(8, 4, replace=False)] = rng.choice([-0.5, 0.5], 4)
    return base[rng.integers(0, distinct, n)]


@pytest.mark.parametrize("delta", [0.25, 0.5])
@pytest.mark.parametrize("N,k", [(64, 20), (100, 100), (130, 40)])
def test_exact_inputs_equal_the_rule_bit_for_bit(gpu, N, k, delta):
    """Every value and every pair sum is exact in f32 here, so ties are real ties: the lists must be
    the float64 rule's, which takes the lowest pool position among equal values and pushes the
    duplicates of a pick down."""
    from lgcn_amd.recommend import rerank_mmr

    rng = np.random.default_rng(N + k)
    cands = _half_rows(rng, 600, 150)
    queries = _half_rows(rng, 40, 40)
    assert np.unique(cands, axis=0).shape[0] < 200  # many exact duplicates
    S = queries.astype(np.float64) @ cands.astype(np.float64).T
    order = np.stack([np.lexsort((np.arange(600), -S[q]))[:N] for q in range(40)])
    pscore = np.take_along_axis(S, order, 1).astype(np.float32)
    assert (pscore.astype(np.float64) == np.take_along_axis(S, order, 1)).all()
    t = lambda a: torch.from_numpy(a).to(gpu)
    out = rerank_mmr(t(order.astype(np.int32)), t(pscore), t(cands), k, delta, normalized=True)
    assert out.idx.dtype == torch.int32
    gi, gs, gp, gn = _np(*out)
    U = cands.astype(np.float64)
    pushed = 0
    for q in range(40):
        wi, ws, wp, wn = mmr64(order[q], pscore[q], U, k, delta)
        np.testing.assert_array_equal(gi[q], wi)
        np.testing.assert_array_equal(gs[q].view(np.uint32), ws.view(np.uint32))
        np.testing.assert_array_equal(gp[q], wp.astype(np.float32))
        assert gn[q] == wn == k
        twin = (cands[order[q, 1]] == cands[order[q, 0]]).all()  # pool position 1 repeats position 0's row
        pushed += int(twin and gi[q, 0] == order[q, 0] and gi[q, 1] != order[q, 1])
    assert pushed > 0


@functools.lru_cache(maxsize=None)
def _property_case():
    users, cands, U = _random_set(64)
    picked = np.random.default_rng(5).choice(900, 40, replace=False)
    return users, cands, U, picked


def test_zero_diversity_is_the_relevance_list(gpu):
    from lgcn_amd.recommend import rerank_mmr

    users, cands, U, picked = _property_case()
    pidx, pscore = _pools(gpu, users, picked, cands, 100)
    out = rerank_mmr(pidx, pscore, torch.from_numpy(cands).to(gpu), 20, 0.0)
    assert torch.equal(out.idx, pidx[:, :20]) and torch.equal(out.score.view(torch.int32), pscore[:, :20].view(torch.int32))
    assert (out.n == 20).all()
    want = ild64(*_np(out.pair, out.n), [20])
    ref = np.array([[1 - (np.sum(U[r] @ U[r].T) - 20) / (20 * 19)] for r in pidx[:, :20].cpu().numpy()])
    np.testing.assert_allclose(want, ref, atol=20 * BAR)


def test_smaller_k_is_a_prefix(gpu):
    from lgcn_amd.recommend import rerank_mmr

    users, cands, U, picked = _property_case()
    pidx, pscore = _pools(gpu, users, picked, cands, 100)
    c = torch.from_numpy(cands).to(gpu)
    a, b = rerank_mmr(pidx, pscore, c, 5, 0.5), rerank_mmr(pidx, pscore, c, 20, 0.5)
    assert torch.equal(a.idx, b.idx[:, :5]) and torch.equal(a.score, b.score[:, :5]) and torch.equal(a.pair, b.pair[:, :5])
    assert not torch.equal(b.idx, pidx[:, :20])  # the re-rank did something


def test_strided_and_int32_pools_equal_the_contiguous_int64_one(gpu):
    from lgcn_amd.recommend import rerank_mmr

    users, cands, U, picked = _property_case()
    pidx, pscore = _pools(gpu, users, picked, cands, 100)
    c = torch.from_numpy(cands).to(gpu)
    want = rerank_mmr(pidx, pscore, c, 10, 0.7)
    wide_i = torch.full((40, 117), 3, dtype=torch.int64, device=gpu)
    wide_s = torch.full((40, 117), 9.0, device=gpu)
    wide_i[:, 5:105], wide_s[:, 5:105] = pidx, pscore
    for dtype in (torch.int64, torch.int32):
        views = (wide_i.to(dtype)[:, 5:105], wide_s[:, 5:105])
        assert not views[0].is_contiguous() and views[0].stride(0) == 117
        got = rerank_mmr(*views, c, 10, 0.7)
        assert got.idx.dtype == dtype and torch.equal(got.idx.to(torch.int64), want.idx)
        assert torch.equal(got.score, want.score) and torch.equal(got.pair, want.pair) and torch.equal(got.n, want.n)
    # leading dimensions that differ between the two tensors are served too (made contiguous)
    got = rerank_mmr(wide_i[:, 5:105], pscore, c, 10, 0.7)
    assert torch.equal(got.idx, want.idx) and torch.equal(got.pair, want.pair)


def test_ineligible_entries_are_skipped(gpu):
    """-1, M and 2**31 - 1 in a pool (and a value past int32 in an int64 pool): the output is what
    the pool without those positions gives."""
    from lgcn_amd.recommend import rerank_mmr

    users, cands, U, picked = _property_case()
    pidx, pscore = _pools(gpu, users, picked, cands, 70)
    c = torch.from_numpy(cands).to(gpu)
    holes = [0, 6, 64, 69]  # positions in both lane slots, the first and the last
    keep = [p for p in range(70) if p not in holes]
    want = rerank_mmr(pidx[:, keep].contiguous(), pscore[:, keep].contiguous(), c, 30, 0.5)
    for dtype, junk in ((torch.int32, [-1, M_RANDOM, 2**31 - 1, -7]), (torch.int64, [-1, M_RANDOM, 2**31 - 1, 2**40 + 5])):
        bad = pidx.to(dtype).clone()
        bad[:, holes] = torch.tensor(junk, dtype=dtype, device=gpu)
        got = rerank_mmr(bad, pscore, c, 30, 0.5)
        assert torch.equal(got.idx.to(torch.int64), want.idx) and torch.equal(got.score, want.score)
        assert torch.equal(got.pair, want.pair) and (got.n == 30).all()
        check_lists(*_np(bad, pscore), U, 30, 0.5, *_np(*got))
    # k above the eligible count: a -1 / -inf / 0 tail and n below k
    got = rerank_mmr(bad, pscore, c, 70, 0.5)
    assert (got.n == 66).all() and (got.idx[:, 66:] == -1).all() and torch.isneginf(got.score[:, 66:]).all()
    assert (got.pair[:, 66:] == 0).all()
    check_lists(*_np(bad, pscore), U, 70, 0.5, *_np(*got))


def test_short_pools_no_queries_and_a_zero_row(gpu):
    from lgcn_amd.recommend import rerank_mmr, topk_rows

    rng = np.random.default_rng(21)
    users = rng.standard_normal((6, 16)).astype(np.float32)
    cands = rng.standard_normal((40, 16)).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(gpu)
    # query q excludes all but 5 + q candidates: topk_rows pads its pool of 20 with -1 / -inf
    rows = [np.sort(rng.choice(40, 35 - q, replace=False)) for q in range(6)]
    ptr = torch.from_numpy(np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)).to(gpu)
    eidx = torch.from_numpy(np.concatenate(rows).astype(np.int32)).to(gpu)
    pidx, pscore = topk_rows(t(users), torch.arange(6), t(cands), 20, excl=(ptr, eidx))
    got = rerank_mmr(pidx, pscore, t(cands), 10, 0.5)
    assert got.n.tolist() == [5, 6, 7, 8, 9, 10]
    check_lists(*_np(pidx, pscore), unit_rows64(cands), 10, 0.5, *_np(*got))
    # no queries
    none = rerank_mmr(pidx[:0], pscore[:0], t(cands), 10, 0.5)
    assert none.idx.shape == none.score.shape == none.pair.shape == (0, 10) and none.n.shape == (0,)
    assert none.idx.dtype == torch.int64
    # one zero candidate row: its cosines are NaN, it ranks first in the pool and is picked last
    cands[17] = 0
    pidx, pscore = topk_rows(t(users), torch.arange(6), t(cands), 40)
    assert (pidx[:, 0] == 17).all() and torch.isnan(pscore[:, 0]).all()
    got = rerank_mmr(pidx, pscore, t(cands), 40, 0.5)
    gi = got.idx.cpu().numpy()
    assert (gi[:, -1] == 17).all() and (got.n == 40).all()
    assert all(np.array_equal(np.sort(r), np.arange(40)) for r in gi)
    check_lists(*_np(pidx, pscore), unit_rows64(cands), 40, 0.5, *_np(*got))


def test_topk_rows_diverse_is_topk_rows_then_rerank(gpu):
    from lgcn_amd.recommend import intra_list_diversity, rerank_mmr, topk_rows_diverse

    users, cands, U, picked = _property_case()
    t = lambda a: torch.from_numpy(a).to(gpu)
    rng = np.random.default_rng(8)
    rows = [np.sort(rng.choice(M_RANDOM, 30, replace=False)) for _ in range(40)]
    excl = (torch.arange(0, 41 * 30, 30, dtype=torch.int64, device=gpu), t(np.concatenate(rows).astype(np.int32)))
    pidx, pscore = _pools(gpu, users, picked, cands, 128, excl=excl)
    mean_ild = {}
    for delta in (0.0, 0.7):
        want = rerank_mmr(pidx, pscore, t(cands), 50, delta)
        got = topk_rows_diverse(t(users), torch.from_numpy(picked), t(cands), 50, delta, pool=128, excl=excl)
        assert got.idx.dtype == torch.int64
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        assert not np.isin(got.idx.cpu().numpy(), rows[0])[0].any()
        dec, steps = check_lists(*_np(pidx, pscore), U, 50, delta, *_np(*got))
        assert dec > 0.9 * steps
        ild = intra_list_diversity(got.pair, got.n, [50])
        np.testing.assert_allclose(ild.cpu().numpy(), ild64(*_np(got.pair, got.n), [50]), rtol=1e-12)
        mean_ild[delta] = float(ild.mean())
    print(f"mean ILD@50: {mean_ild}")
    assert mean_ild[0.7] > mean_ild[0.0]  # the float64 rule: 0.942 against 0.916 on inputs of this kind
    # the default pool max(4 * 10, 64) = 64, int32 indices handed on, the pool clamped to M
    got = topk_rows_diverse(t(users), torch.from_numpy(picked), t(cands), 10, 0.3, index_dtype=torch.int32)
    p64 = _pools(gpu, users, picked, cands, 64)
    want = rerank_mmr(*p64, t(cands), 10, 0.3)
    assert got.idx.dtype == torch.int32 and torch.equal(got.idx.to(torch.int64), want.idx)
    few = topk_rows_diverse(t(users), torch.from_numpy(picked), t(cands[:30]), 10, 0.3)
    want = rerank_mmr(*_pools(gpu, users, picked, cands[:30], 30), t(cands[:30]), 10, 0.3)
    assert torch.equal(few.idx, want.idx) and torch.equal(few.pair, want.pair)


def test_evaluate_ranking_with_diversity(gpu):
    from lgcn_amd import metrics
    from lgcn_amd.recommend import intra_list_diversity, topk_rows_diverse

    users, cands, U, _ = _property_case()
    rng = np.random.default_rng(14)
    t = lambda a: torch.from_numpy(a).to(gpu)
    csr = lambda rows: (t(np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)),
                        t(np.concatenate(rows + [np.zeros(0, np.int64)]).astype(np.int32)))
    seen_rows = [np.sort(rng.choice(M_RANDOM, 20, replace=False)) for _ in range(900)]
    truth_rows = [np.sort(rng.choice(np.setdiff1d(np.arange(M_RANDOM), seen_rows[u]), 15, replace=False))
                  if u % 3 == 0 else np.zeros(0, np.int64) for u in range(900)]
    seen, truth = csr(seen_rows), csr(truth_rows)
    ks = (5, 10, 20)
    today = metrics.evaluate_ranking(t(users), t(cands), truth, ks=ks, seen=seen)
    assert set(today) == {"users"} | {f"{m}@{c}" for m in metrics.METRICS for c in ks}  # None: the old key set
    assert metrics.METRICS == ("recall", "precision", "hit_rate", "ndcg", "mrr")
    measured = metrics.evaluate_ranking(t(users), t(cands), truth, ks=ks, seen=seen, diversity=0.0)
    assert set(measured) == set(today) | {f"ild@{c}" for c in ks}
    assert all(measured[key] == today[key] for key in today)
    who = torch.arange(0, 900, 3)
    lists = topk_rows_diverse(t(users), who, t(cands), 20, 0.0, excl=(seen[0], seen[1], who))
    want = ild64(*_np(lists.pair, lists.n), ks).mean(0)
    for j, c in enumerate(ks):
        assert measured[f"ild@{c}"] == pytest.approx(want[j], rel=1e-9)
    diverse = metrics.evaluate_ranking(t(users), t(cands), truth, ks=ks, seen=seen, diversity=0.7, pool=100)
    assert diverse["users"] == today["users"] == 300
    assert all(diverse[f"ild@{c}"] > measured[f"ild@{c}"] for c in ks)
    assert any(diverse[key] != today[key] for key in today)
    # users without truth are not averaged, for ILD either
    everyone = metrics.evaluate_ranking(t(users), t(cands), truth, ks=ks, seen=seen, diversity=0.7, pool=100,
                                        users=torch.arange(900))
    assert everyone["users"] == 300 and all(everyone[key] == pytest.approx(diverse[key], rel=1e-12) for key in diverse)
    # nobody evaluated: nan
    empty = (torch.zeros(901, dtype=torch.int64, device=gpu), torch.zeros(0, dtype=torch.int32, device=gpu))
    nobody = metrics.evaluate_ranking(t(users), t(cands), empty, ks=ks, seen=seen, diversity=0.5, users=torch.arange(4))
    assert nobody["users"] == 0 and all(np.isnan(nobody[f"ild@{c}"]) for c in ks)


def test_recommend_for_users_with_diversity(gpu, tmp_path):
    from data.dataset_handler import MovieLensDataHandler, write_synthetic_movielens
    from lgcn_amd.recommend import seen_csr, topk_rows
    from models.light_gcn import LightGCN
    from utils import ranking_eval
    from utils import recommend as R

    rp, mp = write_synthetic_movielens(str(tmp_path), 300, 200, 6000, seed=3)
    h = MovieLensDataHandler(rp, mp, device=gpu)
    U, I = h.get_num_users_items()
    torch.manual_seed(11)
    model = LightGCN(U, I, num_layers=2, dim_h=64).to(gpu)
    model.eval()
    title_of = dict(zip(h.movies["movieId"].tolist(), h.movies["title"].tolist()))
    user_ids = list(h.user_id_map)[:63]
    ids = user_ids[:30] + [-5] + user_ids[30:]
    served = R.recommend_for_users(model, ids, h, k=10, diversity=0.5)
    assert len(served) == 64 and served[30] == {"error": "Invalid user ID"}
    lists = served[:30] + served[31:]
    assert all(len(row) == 10 and all(title_of[x["movie_id"]] == x["title"] for x in row) for row in lists)
    # the pools those lists were picked from: the default pool of 64, seen movies left out
    uidx = torch.tensor([h.user_id_map[u] for u in user_ids], device=gpu)
    uw, iw = model.user_embedding.weight.detach(), model.item_embedding.weight.detach()
    ptr, seen = seen_csr(h.edge_index.to(gpu), U, I, by="user")
    pidx, pscore = topk_rows(uw, uidx, iw, 64, excl=(ptr, seen, uidx))
    got_idx = np.array([[h.movie_id_map[x["movie_id"]] - U for x in row] for row in lists])
    got_score = np.array([[x["score"] for x in row] for row in lists], np.float32)
    dec, steps = check_lists(*_np(pidx, pscore), unit_rows64(iw.cpu().numpy()), 10, 0.5, got_idx, got_score, None, None)
    assert steps == 630 and dec > 0.9 * steps
    relevance = R.recommend_for_users(model, user_ids, h, k=10)
    assert [[x["movie_id"] for x in row] for row in relevance] != [[x["movie_id"] for x in row] for row in lists]
    assert R.recommend_for_users(model, user_ids, h, k=10, diversity=0.0) == relevance
    # the harness-level evaluation passes both keywords through
    ei = h.edge_index
    out = ranking_eval.evaluate_ranking(model, ei[:, ::2], ei[:, 1::2], gpu, ks=(5, 10), diversity=0.5, pool=40)
    assert {"ild@5", "ild@10", "recall@10"} <= set(out) and 0.0 < out["ild@10"] < 2.0
    assert "ild@5" not in ranking_eval.evaluate_ranking(model, ei[:, ::2], ei[:, 1::2], gpu, ks=(5, 10))
