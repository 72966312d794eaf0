"""Full-ranking evaluation on the GPU (lgcn_amd.metrics, k_rank_metrics in csrc/lgcn_metrics.hip,
utils.ranking_eval.evaluate_ranking) against the float64 numpy checker of rank_metrics_checker.py.

The kernel sees integers only, so hits, first hit rank and truth length must be EQUAL to the
checker's; its DCG is a float64 sum of at most 1,024 positive terms (off by ~1e-13 relative at
most) rounded once to float32, so |dcg - ref64| <= 2**-23 * ref64.

End to end, a user is SEPARATED when all of its eligible top 21 float64 scores differ by more than
1e-5 (the bar of test_gpu_recommend.py) from their neighbours: the device's top 20 is then the
checker's, and the per-user counts must be equal. Means over separated users: 1e-12 relative for
recall, precision, hit_rate and mrr (integer counts, float64 arithmetic), 2.5e-7 relative for ndcg
(one float32 ulp per user's DCG)."""
import functools

import numpy as np
import pytest
import torch

from rank_metrics_checker import METRICS, counts64, eligible_order, scores64, summarize64

pytestmark = pytest.mark.gpu

BAR = 1e-5
M = 6000  # the candidate universe of the synthetic lists
TRUTH_LENGTHS = (0, 1, 3, 5000, 40, 200)  # row t has about TRUTH_LENGTHS[t % 6] entries
R = 40


def _cutoff_sets(k):
    sets = [(1,), tuple(sorted({1, min(64, k), k})), tuple(sorted({int(c) for c in np.linspace(1, k, 8).round()}))]
    return sorted(set(sets))


@functools.lru_cache(maxsize=None)
def _synthetic(k, Q):
    """Ranked lists (distinct indices, some rows with a -1 tail), a row id per query (some outside
    [0, R)) and R truth rows; a row's entries are drawn partly from the list of a query that uses
    it, so short rows are hit too."""
    rng = np.random.default_rng(k * 10007 + Q)
    ranked = np.stack([rng.permutation(M)[:k] for _ in range(Q)]).astype(np.int32)
    for q in range(0, Q, 3):  # every third query: fewer than k were eligible
        ranked[q, rng.integers(0, k + 1):] = -1
    rows = rng.integers(-2, R + 2, Q).astype(np.int64)
    truth = []
    for t in range(R):
        n = TRUTH_LENGTHS[t % len(TRUTH_LENGTHS)]
        users_of = np.flatnonzero((rows == t) | (np.arange(Q) == t))  # by rows= and by the identity mapping
        own = ranked[users_of[0]] if users_of.size else np.zeros(0, np.int32)
        own = own[own >= 0]
        part = rng.choice(own, min(own.size, (n + 1) // 2), replace=False) if own.size else own
        truth.append(np.unique(np.concatenate([part, rng.choice(M, n - part.size, replace=False)])).astype(np.int32))
    assert [len(t) for t in truth[:3]] == [0, 1, 3] and len(truth[3]) > 4000
    return ranked, rows, truth


def _csr(truth, dev):
    ptr = np.cumsum([0] + [len(t) for t in truth]).astype(np.int64)
    idx = np.concatenate(list(truth) + [np.zeros(0, np.int32)]).astype(np.int32)
    return torch.from_numpy(ptr).to(dev), torch.from_numpy(idx).to(dev)


def _compare(counts, want, what):
    hits, dcg, first, n_truth = (t.cpu().numpy() for t in counts)
    w_hits, w_dcg, w_first, w_truth = want
    assert hits.dtype == np.int32 and dcg.dtype == np.float32 and first.dtype == np.int32 and n_truth.dtype == np.int32
    np.testing.assert_array_equal(hits, w_hits, err_msg=what)
    np.testing.assert_array_equal(first, w_first, err_msg=what)
    np.testing.assert_array_equal(n_truth, w_truth, err_msg=what)
    err = np.abs(dcg.astype(np.float64) - w_dcg)
    assert (err <= 2.0 ** -23 * w_dcg).all(), (what, float((err / np.maximum(w_dcg, 1e-300)).max()))


@pytest.mark.parametrize("Q", [1, 5, 1027])
@pytest.mark.parametrize("k", [1, 63, 64, 65, 100, 1024])
def test_kernel_matches_checker(gpu, k, Q):
    from lgcn_amd.metrics import rank_metrics

    ranked, rows, truth = _synthetic(k, Q)
    csr = _csr(truth, gpu)
    wide = torch.full((Q, k + 7), 123, dtype=torch.int32, device=gpu)  # ld > k: a column slice
    wide[:, :k] = torch.from_numpy(ranked).to(gpu)
    truth_by_row = lambda q: truth[rows[q]] if 0 <= rows[q] < R else np.zeros(0, np.int32)
    truth_by_id = lambda q: truth[q] if q < R else np.zeros(0, np.int32)
    some_hits = 0
    for cs in _cutoff_sets(k):
        want = counts64(ranked, truth_by_row, cs)
        some_hits += int(want[0].sum())
        _compare(rank_metrics(wide[:, :k], csr, cs, rows=torch.from_numpy(rows)), want, f"rows= {cs}")
        # the identity mapping, int64 lists (converted once), cutoffs out of order
        want = counts64(ranked, truth_by_id, cs)
        _compare(rank_metrics(torch.from_numpy(ranked).to(gpu).long(), csr, list(cs[::-1]), rows=None), want,
                 f"identity {cs}")
    if Q == 1027:
        assert some_hits > 0


def test_kernel_hits_every_kind_of_row(gpu):
    """The generator above must exercise what it claims: hits in short rows, the deep row, -1
    tails, rows outside the CSR, several cutoffs with different counts."""
    ranked, rows, truth = _synthetic(100, 1027)
    cs = (1, 64, 100)
    hits, dcg, first, n_truth = counts64(ranked, lambda q: truth[rows[q]] if 0 <= rows[q] < R else [], cs)
    assert ((rows < 0) | (rows >= R)).any() and (ranked[:, -1] == -1).any()
    for n in (1, 3):
        assert hits[(n_truth == n)].sum() > 0
    assert hits[n_truth > 4000].max() > 64
    assert (hits[:, 0] < hits[:, 1]).any() and (hits[:, 1] < hits[:, 2]).any() and (first > 0).any()


def test_empty_truth_and_no_queries(gpu):
    from lgcn_amd.metrics import rank_metrics, summarize

    ranked = torch.arange(20, dtype=torch.int32, device=gpu).repeat(3, 1)
    empty = (torch.zeros(4, dtype=torch.int64, device=gpu), torch.zeros(0, dtype=torch.int32, device=gpu))
    c = rank_metrics(ranked, empty, (5, 20))
    assert not c.hits.any() and not c.dcg.any() and (c.first == -1).all() and not c.n_truth.any()
    assert summarize(c, (5, 20))["users"] == 0
    c = rank_metrics(ranked[:0], empty, (5, 20))
    assert c.hits.shape == (0, 2) and c.first.shape == (0,)


def test_int64_lists_do_not_wrap_and_strided_rows_work(gpu):
    """An int64 candidate of 2**32 + 7 must not be read as 7 (a truth item), and row ids may come
    as a non-contiguous tensor."""
    from lgcn_amd.metrics import rank_metrics

    truth = _csr([np.array([7], np.int32), np.array([3], np.int32)], gpu)
    ranked = torch.tensor([[2 ** 32 + 7, 5, 7], [2 ** 31, 3, -(2 ** 32) + 3]], dtype=torch.int64, device=gpu)
    rows = torch.tensor([[0, 9], [1, 9]], device=gpu)[:, 0]
    assert not rows.is_contiguous()
    c = rank_metrics(ranked, truth, (1, 3), rows=rows)
    assert c.hits.tolist() == [[0, 1], [0, 1]] and c.first.tolist() == [2, 1] and c.n_truth.tolist() == [1, 1]


# --------------------------------------------------------------------------------------------
# end to end

CASES = {"dense": dict(U=300, I=2000, kw={}), "filtered": dict(U=256, I=20000, kw=dict(cap=4096, subset=2048))}
KS = (5, 10, 20)


@functools.lru_cache(maxsize=None)
def _case(name):
    """Embeddings, seen rows (0-50 items), truth rows (1-10 of the checker's eligible top 40; every
    seventh user none; every eleventh user one seen item more, which can never be hit) and the
    checker's eligible order per user."""
    U, I = CASES[name]["U"], CASES[name]["I"]
    rng = np.random.default_rng(U + I)
    ue = rng.standard_normal((U, 64)).astype(np.float32)
    ie = rng.standard_normal((I, 64)).astype(np.float32)
    S = scores64(ue, ie)
    seen = [np.sort(rng.choice(I, rng.integers(0, 51), replace=False)) for _ in range(U)]
    order, truth, sep = [], [], np.zeros(U, bool)
    for u in range(U):
        o = eligible_order(S[u], seen[u])
        t = np.zeros(0, np.int64) if u % 7 == 0 else rng.choice(o[:40], rng.integers(1, 11), replace=False)
        if u % 11 == 1 and len(seen[u]):
            t = np.concatenate([t, seen[u][:1]])
        order.append(o[:KS[-1]])
        truth.append(np.unique(t).astype(np.int32))
        sep[u] = (np.abs(np.diff(S[u, o[:KS[-1] + 1]])) > BAR).all()
    return ue, ie, seen, truth, np.stack(order), sep


@pytest.mark.parametrize("name", list(CASES))
def test_evaluate_ranking_matches_checker(gpu, name):
    from lgcn_amd.metrics import evaluate_ranking, rank_metrics
    from lgcn_amd.recommend import topk_items

    ue, ie, seen, truth, order, sep = _case(name)
    kw = CASES[name]["kw"]
    t = lambda a: torch.from_numpy(a).to(gpu)
    seen_csr, truth_csr = _csr(seen, gpu), _csr(truth, gpu)
    evaluated = np.flatnonzero([len(x) > 0 for x in truth])
    share = sep[evaluated].mean()
    print(f"{name}: {evaluated.size} users evaluated, separated share {share:.4f}")
    assert share > 0.8
    want = counts64(order, lambda u: truth[u], KS)
    assert any(np.isin(truth[u], seen[u]).any() for u in evaluated)  # a truth item that is also seen
    assert (want[0][:, 0] < want[0][:, 2]).any()  # hits vary across the cutoffs
    # per-user counts of the separated users
    users = evaluated[sep[evaluated]]
    idx, _ = topk_items(t(ue), t(ie), t(users), KS[-1], seen=seen_csr, **kw)
    counts = rank_metrics(idx, truth_csr, KS, rows=t(users))
    np.testing.assert_array_equal(counts.hits.cpu().numpy(), want[0][users])
    np.testing.assert_array_equal(counts.first.cpu().numpy(), want[2][users])
    np.testing.assert_array_equal(counts.n_truth.cpu().numpy(), want[3][users])
    # the means
    got = evaluate_ranking(t(ue), t(ie), truth_csr, ks=KS, seen=seen_csr, users=t(users), **kw)
    ref = summarize64(*[a[users] for a in want], KS)
    assert got["users"] == ref["users"] == users.size
    assert set(got) == {"users"} | {f"{m}@{c}" for m in METRICS for c in KS}
    for key, w in ref.items():
        rel = 2.5e-7 if key.startswith("ndcg") else 1e-12
        print(f"{name} {key}: {got[key]!r} (checker {w!r})")
        assert abs(got[key] - w) <= rel * abs(w), key


def test_evaluate_ranking_is_its_public_pieces(gpu):
    from lgcn_amd.metrics import evaluate_ranking, rank_metrics, summarize
    from lgcn_amd.recommend import topk_items

    ue, ie, seen, truth, _, _ = _case("dense")
    ue, ie = torch.from_numpy(ue).to(gpu), torch.from_numpy(ie).to(gpu)
    seen_csr, truth_csr = _csr(seen, gpu), _csr(truth, gpu)
    got = evaluate_ranking(ue, ie, truth_csr, ks=KS, seen=seen_csr)
    users = torch.tensor([u for u, x in enumerate(truth) if len(x)], device=gpu)  # the default: non-empty truth rows
    idx, _ = topk_items(ue, ie, users, max(KS), seen=seen_csr)
    assert idx.dtype == torch.int64  # the public return is unchanged
    by_hand = summarize(rank_metrics(idx, truth_csr, KS, rows=users), KS)
    assert got == by_hand and got["users"] == users.numel()  # to the bit
    assert evaluate_ranking(ue, ie, truth_csr, ks=(20, 5, 5, 10), seen=seen_csr) == got
    # every user evaluated: the users without truth are left out of the means
    everyone = evaluate_ranking(ue, ie, truth_csr, ks=KS, seen=seen_csr, users=torch.arange(len(truth)))
    assert everyone["users"] == got["users"] and everyone == pytest.approx(got, rel=1e-12)
    # without exclusion the lists differ (seen items may rank), so must some metric
    assert evaluate_ranking(ue, ie, truth_csr, ks=KS) != got


def test_harness_evaluate_ranking(gpu, tmp_path):
    from data.dataset_handler import MovieLensDataHandler, write_synthetic_movielens
    from lgcn_amd import metrics
    from lgcn_amd.recommend import seen_csr
    from models.light_gcn import LightGCN
    from utils import ranking_eval as T

    rp, mp = write_synthetic_movielens(str(tmp_path), 300, 200, 6000, seed=3)
    h = MovieLensDataHandler(rp, mp, device=gpu)
    U, I = h.get_num_users_items()
    torch.manual_seed(11)
    model = LightGCN(U, I, num_layers=2, dim_h=64).to(gpu)
    E = h.edge_index.shape[1]
    perm = np.random.default_rng(12).permutation(E)
    train = h.edge_index[:, torch.from_numpy(np.sort(perm[:E * 9 // 10]))].to(gpu)
    held = h.edge_index[:, torch.from_numpy(np.sort(perm[E * 9 // 10:]))]
    seen, truth = seen_csr(train, U, I), seen_csr(held.to(gpu), U, I)
    keys = {"users"} | {f"{m}@{c}" for m in METRICS for c in KS}
    with torch.no_grad():
        raw = T.evaluate_ranking(model, train, held, gpu, ks=KS, embeddings="raw")
        want = metrics.evaluate_ranking(*model.get_embeddings(torch.arange(U, device=gpu), torch.arange(I, device=gpu)),
                                        truth, ks=KS, seen=seen)
        assert raw == want and set(raw) == keys and raw["users"] > 0
        prop = T.evaluate_ranking(model, train, held, gpu, ks=KS, embeddings="propagated")
        want = metrics.evaluate_ranking(*model(train), truth, ks=KS, seen=seen)
        assert prop == want and set(prop) == keys and prop["users"] == raw["users"]
    assert T.evaluate_ranking(model, train, held, gpu)["users"] == raw["users"]  # the default cutoff
    assert set(T.evaluate_ranking(model, train, held, gpu)) == {"users"} | {f"{m}@20" for m in METRICS}
    with pytest.raises(ValueError):
        T.evaluate_ranking(model, train, held, gpu, embeddings="final")
