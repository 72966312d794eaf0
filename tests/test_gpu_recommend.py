"""Top-k recommendation on the GPU (lgcn_amd.recommend, utils.recommend, k_select_ranked in
csrc/lgcn_recall.hip) against a float64 numpy restatement: normalise, q @ c.T, excluded entries to
-inf, np.lexsort on (index, -score).

Rank position j of a query is SEPARATED when its float64 score differs by more than 1e-5 (the
separation bar of test_gpu_recall.py) from both neighbours in the eligible order, position k + 1
included. At every position the returned score, and the float64 score of the returned index, are
within 1e-5 of the checker's score there; at separated positions the index is the checker's.
Always: indices distinct, none excluded, scores non-increasing, equal neighbouring scores in
ascending index order. More than 0.9 of the positions of each case must be separated."""
import functools

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

BAR = 1e-5


def _emb(rng, n, d):
    return rng.standard_normal((n, d)).astype(np.float32)


def _scores64(q, c):
    q, c = q.astype(np.float64), c.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = q / np.linalg.norm(q, axis=1, keepdims=True)
        c = c / np.linalg.norm(c, axis=1, keepdims=True)
    return q @ c.T


def _order(srow, excl):
    """Eligible candidates of one query in rank order (score descending, index ascending)."""
    s = srow.copy()
    s[excl] = -np.inf
    order = np.lexsort((np.arange(s.size), -s))
    return order[:s.size - len(excl)]


def _csr(rows, dev):
    ptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    idx = np.concatenate([np.asarray(r, np.int32) for r in rows] + [np.zeros(0, np.int32)])
    return torch.from_numpy(ptr).to(dev), torch.from_numpy(idx).to(dev)


def _check(S, rows, k, idx, score, exact=False):
    """The module docstring's rules for one call; returns the share of separated positions."""
    idx, score = idx.cpu().numpy(), score.cpu().numpy()
    assert idx.shape == score.shape == (S.shape[0], k) and idx.dtype == np.int64 and score.dtype == np.float32
    sep_n = pos_n = 0
    for q in range(S.shape[0]):
        excl = np.asarray(rows[q], np.int64) if rows is not None else np.zeros(0, np.int64)
        order = _order(S[q], excl)
        n = min(k, order.size)
        gi, gs = idx[q, :n], score[q, :n]
        assert (idx[q, n:] == -1).all() and np.isneginf(score[q, n:]).all(), q
        assert (gi >= 0).all() and np.unique(gi).size == n and not np.isin(gi, excl).any(), q
        ref = S[q, order[:n + 1]]  # position k + 1 included where it exists
        assert np.abs(gs - ref[:n]).max(initial=0) <= BAR, (q, np.abs(gs - ref[:n]).max())
        assert np.abs(S[q, gi] - ref[:n]).max(initial=0) <= BAR, q
        assert (np.diff(gs) <= 0).all(), q
        same = np.diff(gs) == 0
        assert (np.diff(gi)[same] > 0).all(), q
        gap = np.abs(np.diff(ref))
        left = np.concatenate([[np.inf], gap])[:n]
        right = np.concatenate([gap, [np.inf]])[:n]
        sep = (left > BAR) & (right > BAR)
        if exact:
            np.testing.assert_array_equal(gi, order[:n])
        else:
            np.testing.assert_array_equal(gi[sep], order[:n][sep])
        sep_n += int(sep.sum())
        pos_n += n
    return sep_n / max(pos_n, 1)


def _topk_rows(gpu, users, picked, cands, k, rows=None, **kw):
    from lgcn_amd.recommend import topk_rows

    t = lambda a: torch.from_numpy(a).to(gpu)
    excl = None if rows is None else _csr(rows, gpu)
    return topk_rows(t(users), torch.from_numpy(picked), t(cands), k, excl=excl, **kw)


@pytest.mark.parametrize("d", [8, 64, 100, 256])
@pytest.mark.parametrize("k", [1, 10, 100])
def test_grid_matches_checker(gpu, d, k):
    rng = np.random.default_rng(d * 1000 + k)
    users, cands = _emb(rng, 900, d), _emb(rng, 2000, d)
    picked = rng.choice(900, 300, replace=False)
    rows = [np.sort(rng.choice(2000, rng.integers(0, 51), replace=False)) for _ in range(300)]
    idx, score = _topk_rows(gpu, users, picked, cands, k, rows)
    share = _check(_scores64(users[picked], cands), rows, k, idx, score)
    print(f"d={d} k={k}: separated share {share:.4f}")
    assert share > 0.9


@functools.lru_cache(maxsize=1)
def _large_case():
    rng = np.random.default_rng(5)
    users, cands = _emb(rng, 500, 64), _emb(rng, 60000, 64)
    picked = rng.choice(500, 256, replace=False)
    S = _scores64(users[picked], cands)
    # each query excludes its own top 50 (the issue's case; test_threshold_is_formed_after_exclusion
    # is the one a threshold formed before exclusion cannot pass)
    rows = [np.sort(np.argsort(-S[q], kind="stable")[:50]) for q in range(256)]
    return users, cands, picked, S, rows


def _count_filtered_passes(monkeypatch):
    """Counts lgcn_amd.recommend's filtered lgcn_score_filter passes (one per tightening round)."""
    from lgcn_amd import _ffi

    passes, check = [], _ffi.check

    def counting(rc, what):
        if what == "lgcn_score_filter":
            passes.append(what)
        return check(rc, what)

    monkeypatch.setattr(_ffi, "check", counting)
    return passes


@pytest.mark.parametrize("kw", [{}, dict(cap=512, subset=512)], ids=["defaults", "overflow"])
def test_subset_thresholds_and_overflow(gpu, monkeypatch, kw):
    users, cands, picked, S, rows = _large_case()
    passes = _count_filtered_passes(monkeypatch)
    idx, score = _topk_rows(gpu, users, picked, cands, 100, rows, **kw)
    # one query block: one filtered pass when the lists fit, more when the tighten loop ran
    assert len(passes) == 1 if not kw else len(passes) > 1, len(passes)
    share = _check(S, rows, 100, idx, score)
    print(f"60k candidates {kw}: separated share {share:.4f}")
    assert share > 0.9


def test_threshold_is_formed_after_exclusion(gpu, monkeypatch):
    """600 candidates above a capacity of 512, thresholds from every fifth candidate, k = 20, each
    query excluding its own top 250: the 20th best subset score BEFORE exclusion lies above every
    eligible score (asserted on the checker's scores), so a filter run against it keeps no eligible
    candidate at all; the threshold formed from eligible subset entries keeps the eligible top 20."""
    rng = np.random.default_rng(9)
    users, cands = _emb(rng, 64, 32), _emb(rng, 600, 32)
    picked = np.arange(64)
    S = _scores64(users, cands)
    rows = [np.sort(np.argsort(-S[q], kind="stable")[:250]) for q in range(64)]
    for q in range(64):
        before = np.sort(S[q, ::5])[-20]  # stride 5 = ceil(600 / 128)
        assert before > S[q, _order(S[q], rows[q])[0]] + BAR
    passes = _count_filtered_passes(monkeypatch)
    idx, score = _topk_rows(gpu, users, picked, cands, 20, rows, cap=512, subset=128)
    assert len(passes) == 1  # no overflow: the first thresholds themselves were low enough
    assert _check(S, rows, 20, idx, score) > 0.9


def test_rows_outside_the_csr_exclude_nothing(gpu):
    """A query whose row id is outside [0, R) drops nothing, on the dense and the filtered path."""
    from lgcn_amd.recommend import topk_items

    rng = np.random.default_rng(10)
    users, items = _emb(rng, 40, 16), _emb(rng, 300, 16)
    t = lambda a: torch.from_numpy(a).to(gpu)
    rows = [np.sort(rng.choice(300, 30, replace=False)) for _ in range(20)]  # a CSR of 20 users only
    seen = _csr(rows, gpu)
    q = np.arange(40)
    S = _scores64(users, items)
    want_rows = rows + [np.zeros(0, np.int64)] * 20
    for kw in ({}, dict(cap=128, subset=64)):
        idx, score = topk_items(t(users), t(items), torch.from_numpy(q), 5, seen=seen, **kw)
        _check(S, want_rows, 5, idx, score)


def test_empty_shapes(gpu):
    from lgcn_amd.recommend import topk_rows

    rng = np.random.default_rng(13)
    users, cands = _emb(rng, 6, 16), _emb(rng, 3, 16)
    t = lambda a: torch.from_numpy(a).to(gpu)
    # no queries
    idx, score = topk_rows(t(users), torch.arange(0), t(cands), 4)
    assert idx.shape == score.shape == (0, 4) and idx.dtype == torch.int64 and score.dtype == torch.float32
    # no candidates: nothing but the -1 / -inf fill
    idx, score = topk_rows(t(users), torch.arange(6), t(cands[:0]), 4)
    assert (idx == -1).all() and torch.isneginf(score).all() and idx.shape == (6, 4)
    # fewer candidates than k, some of them excluded
    rows = [[1], [], [0, 2], [0, 1, 2], [], [2]]
    idx, score = topk_rows(t(users), torch.arange(6), t(cands), 4, excl=_csr(rows, gpu))
    _check(_scores64(users, cands), rows, 4, idx, score, exact=True)


def test_ties_rank_by_index(gpu):
    rng = np.random.default_rng(6)
    users, base = _emb(rng, 200, 32), _emb(rng, 400, 32)
    cands = np.concatenate([base, base[rng.permutation(400)]])
    picked = rng.choice(200, 100, replace=False)
    S = _scores64(users[picked], cands)
    for k in (1, 7, 20):
        idx, score = _topk_rows(gpu, users, picked, cands, k)
        _check(S, None, k, idx, score, exact=True)
    # drop the lower-index member of the pairs at ranks (0, 1) and (4, 5): the twins move up
    order = [_order(S[q], np.zeros(0, np.int64)) for q in range(100)]
    rows = [np.sort(o[[0, 4]]) for o in order]
    for q, o in enumerate(order):
        assert S[q, o[0]] == S[q, o[1]] and S[q, o[4]] == S[q, o[5]] and o[0] < o[1] and o[4] < o[5]
    idx, score = _topk_rows(gpu, users, picked, cands, 7, rows)
    _check(S, rows, 7, idx, score, exact=True)
    got = idx.cpu().numpy()
    for q, o in enumerate(order):
        np.testing.assert_array_equal(got[q, :5], [o[1], o[2], o[3], o[5], o[6]])


def test_edges_below_the_capacity(gpu):
    from lgcn_amd.recommend import topk_rows

    rng = np.random.default_rng(7)
    users, cands = _emb(rng, 10, 16), _emb(rng, 5, 16)
    picked = np.arange(10)
    S = _scores64(users, cands)
    rows = [np.sort(rng.choice(5, 2, replace=False)) for _ in range(10)]
    # k == the eligible count, then fewer eligible than k (a -1 / -inf tail)
    for k in (3, 5):
        idx, score = _topk_rows(gpu, users, picked, cands, k, rows)
        _check(S, rows, k, idx, score, exact=True)
    assert (idx[:, 3:] == -1).all() and torch.isneginf(score[:, 3:]).all() and (idx[:, :3] >= 0).all()
    # an exclusion CSR with no entry at all is no exclusion, to the bit (lgcn_amd.recommend passes
    # none on); empty rows beside filled ones, below, go through the kernel's exclusion path
    a = _topk_rows(gpu, users, picked, cands, 4)
    b = _topk_rows(gpu, users, picked, cands, 4, [[] for _ in range(10)])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    some = [r if q % 2 else r[:0] for q, r in enumerate(rows)]  # empty rows beside filled ones
    b = _topk_rows(gpu, users, picked, cands, 4, some)
    assert torch.equal(a[0][::2], b[0][::2]) and torch.equal(a[1][::2], b[1][::2])
    assert not torch.equal(a[0][1::2], b[0][1::2])
    # a zero query row scores NaN everywhere: NaN ranks first, ties by index
    users[3] = 0
    idx, score = _topk_rows(gpu, users, picked, cands, 4, rows)
    want = np.setdiff1d(np.arange(5), rows[3])
    np.testing.assert_array_equal(idx[3].cpu().numpy(), [*want, -1])
    assert torch.isnan(score[3, :3]).all() and torch.isneginf(score[3, 3])
    keep = [q for q in range(10) if q != 3]
    _check(S[keep], [rows[q] for q in keep], 4, idx[keep], score[keep], exact=True)
    with pytest.raises(ValueError, match="k=1025"):
        _topk_rows(gpu, users, picked, cands, 1025)
    # above the dense capacity a query short of k eligible candidates is refused
    with pytest.raises(ValueError, match="eligible"):
        topk_rows(torch.from_numpy(users).to(gpu), torch.arange(2), torch.from_numpy(cands).to(gpu), 2,
                  excl=_csr([[0, 1, 2, 4], []], gpu), cap=4, subset=4)


@pytest.mark.parametrize("cap", [None, 512], ids=["dense", "filtered"])
def test_query_blocks_equal_one_block(gpu, monkeypatch, cap):
    from lgcn_amd import recommend as RC

    rng = np.random.default_rng(31)
    users, cands = _emb(rng, 700, 32), _emb(rng, 2000, 32)
    picked = rng.choice(700, 300, replace=False)
    rows = [np.sort(rng.choice(2000, rng.integers(0, 51), replace=False)) for _ in range(300)]
    t = lambda a: torch.from_numpy(a).to(gpu)
    ptr, eidx = _csr(rows, gpu)
    by_user = [np.zeros(0, np.int32)] * 700
    for q, u in enumerate(picked):
        by_user[u] = rows[q]
    forms = [(ptr, eidx), (*_csr(by_user, gpu), torch.from_numpy(picked))]  # row q, and a row per query
    kw = {} if cap is None else dict(cap=cap, subset=cap)
    one = [RC.topk_rows(t(users), torch.from_numpy(picked), t(cands), 10, excl=e, **kw) for e in forms]
    assert torch.equal(one[0][0], one[1][0]) and torch.equal(one[0][1], one[1][1])
    share = _check(_scores64(users[picked], cands), rows, 10, *one[0])
    assert share > 0.9
    monkeypatch.setattr(RC, "BLOCK_BYTES", 8 * (cap or 2000) * 128)  # 128 queries per block: three blocks
    for e, (i1, s1) in zip(forms, one):
        i3, s3 = RC.topk_rows(t(users), torch.from_numpy(picked), t(cands), 10, excl=e, **kw)
        assert torch.equal(i1, i3) and torch.equal(s1, s3)


def _reference_formula(q_row, table, excluded, n=10):
    """The reference's ranking on CPU float32 tensors: normalise, matmul, descending sort, skip
    excluded, first n -> (indices, scores, separated)."""
    q = q_row / torch.norm(q_row, dim=1, keepdim=True)
    c = table / torch.norm(table, dim=1, keepdim=True)
    scores = torch.matmul(q, c.t()).squeeze()
    _, order = torch.sort(scores, descending=True)
    excluded = set() if excluded is None else set(int(x) for x in excluded)
    elig = [int(i) for i in order if int(i) not in excluded]
    s = scores[elig].numpy().astype(np.float64)
    gap = np.abs(np.diff(s))
    left, right = np.concatenate([[np.inf], gap]), np.concatenate([gap, [np.inf]])
    m = min(n, len(elig))
    return elig[:m], s[:m], ((left > BAR) & (right > BAR))[:m]


def _agree(got_names, got_scores, want_names, want_scores, sep):
    assert len(got_names) == len(want_names)
    assert np.abs(np.asarray(got_scores) - np.asarray(want_scores)).max(initial=0) <= BAR
    for g, w, s in zip(got_names, want_names, sep):
        assert not s or g == w
    return int(np.sum(sep)), len(sep)


def test_end_to_end_on_a_movielens_shaped_dataset(gpu, tmp_path):
    from data.dataset_handler import MovieLensDataHandler, write_synthetic_movielens
    from models.light_gcn import LightGCN
    from utils import recommend as R

    rp, mp = write_synthetic_movielens(str(tmp_path), 300, 200, 6000, seed=3)
    h = MovieLensDataHandler(rp, mp, device=gpu)
    U, I = h.get_num_users_items()
    torch.manual_seed(11)
    model = LightGCN(U, I, num_layers=2, dim_h=64).to(gpu)
    model.eval()
    uw, iw = model.user_embedding.weight.detach().cpu(), model.item_embedding.weight.detach().cpu()
    rng = np.random.default_rng(12)
    train = h.edge_index[:, torch.from_numpy(np.sort(rng.permutation(h.edge_index.shape[1])[:h.edge_index.shape[1] * 9 // 10]))]
    title_of = dict(zip(h.movies["movieId"].tolist(), h.movies["title"].tolist()))
    sep_n = pos_n = 0
    user_ids = list(h.user_id_map)[:63]
    singles = []
    for n, uid in enumerate(user_ids):
        u = h.user_id_map[uid]
        # the reference __main__'s exclusion tensor, over both directions of the split edge list
        seen = torch.cat([train[1, train[0] == u], train[0, train[1] == u]]) - U
        got = R.recommend_from_user(model, uid, h, seen if n % 2 else seen.tolist())["recommendations"]
        singles.append(got)
        want, ws, sep = _reference_formula(uw[[u]], iw, seen)
        a, b = _agree([x["title"] for x in got], [x["score"] for x in got],
                      [title_of[h.id_movie_map[i + U]] for i in want], ws, sep)
        sep_n, pos_n = sep_n + a, pos_n + b
    for mid in list(h.movie_id_map)[:20]:
        m = h.movie_id_map[mid] - U
        seen = train[1, train[0] == m + U]  # users with a training edge to the movie
        got = R.recommend_from_movie(model, mid, h, seen)["top_users"]
        want, ws, sep = _reference_formula(iw[[m]], uw, seen)
        a, b = _agree([x["user_id"] for x in got], [x["score"] for x in got], [h.id_user_map[i] for i in want], ws, sep)
        sep_n, pos_n = sep_n + a, pos_n + b
    assert sep_n / pos_n > 0.9
    assert R.recommend_from_user(model, -5, h) == {"error": "Invalid user ID"}
    # the batch call: the per-user answers, and the error dict in the unknown id's slot
    ids = user_ids[:30] + [-5] + user_ids[30:]
    batch = R.recommend_for_users(model, ids, h, k=10, train_edge_index=train)
    assert len(batch) == 64 and batch[30] == {"error": "Invalid user ID"}
    for got, single in zip(batch[:30] + batch[31:], singles):
        assert [(x["title"], x["score"]) for x in got] == [(x["title"], x["score"]) for x in single]
        assert all(title_of[x["movie_id"]] == x["title"] for x in got)
    # without exclusion a user's seen movies may come back
    free = R.recommend_for_users(model, user_ids[:4], h, k=10, exclude_seen=False)
    for uid, got in zip(user_ids[:4], free):
        want, ws, sep = _reference_formula(uw[[h.user_id_map[uid]]], iw, None)
        _agree([x["title"] for x in got], [x["score"] for x in got],
               [title_of[h.id_movie_map[i + U]] for i in want], ws, sep)


def test_replays_the_reference_golden(gpu):
    """tests/golden/recommend.npz holds what the reference's own utils/recommend.py returned
    (tests/golden/make_recommend_golden.py); utils.recommend must return the same titles / user
    ids at separated ranks and the same scores within 1e-5, with more than 0.9 of all recorded
    positions separated."""
    import pandas as pd

    from models.light_gcn import LightGCN
    from utils import recommend as R

    G = np.load(GOLDEN / "recommend.npz")
    uw, iw = G["user_weight"], G["item_weight"]
    U, I = uw.shape[0], iw.shape[0]
    model = LightGCN(U, I, num_layers=1, dim_h=uw.shape[1])
    model.load_state_dict({"user_embedding.weight": torch.from_numpy(uw), "item_embedding.weight": torch.from_numpy(iw)})
    model = model.to(gpu)

    class H:
        user_id_map = {int(u): i for i, u in enumerate(G["user_ids"])}
        movie_id_map = {int(m): i + U for i, m in enumerate(G["movie_ids"])}
        movies = pd.DataFrame({"movieId": G["movie_ids"], "title": G["titles"]})

    def separated(scores):
        gap = np.abs(np.diff(scores.astype(np.float64)))
        return (np.concatenate([[np.inf], gap]) > BAR) & (np.concatenate([gap, [np.inf]]) > BAR)

    sep_n = pos_n = 0
    for n in range(int(G["n_user_calls"])):
        excl = G[f"u{n}_excl"] if G[f"u{n}_has_excl"] else None
        if excl is not None and n % 2:
            excl = torch.from_numpy(excl)
        elif excl is not None:
            excl = excl.tolist()
        got = R.recommend_from_user(model, int(G[f"u{n}_id"]), H, excl)["recommendations"]
        ws = G[f"u{n}_scores"]
        # the golden row ends at rank ten: the last position's right neighbour is not recorded, so
        # it counts as separated only when the row is short (nothing eligible follows it)
        sep = separated(ws)
        if len(ws) == 10:
            sep[-1] = False
        a, b = _agree([x["title"] for x in got], [x["score"] for x in got], G[f"u{n}_titles"].tolist(), ws, sep)
        sep_n, pos_n = sep_n + a, pos_n + b
    for n in range(int(G["n_movie_calls"])):
        excl = G[f"m{n}_excl"].tolist() if G[f"m{n}_has_excl"] else None
        got = R.recommend_from_movie(model, int(G[f"m{n}_id"]), H, excl)["top_users"]
        ws = G[f"m{n}_scores"]
        sep = separated(ws)
        if len(ws) == 10:
            sep[-1] = False
        a, b = _agree([x["user_id"] for x in got], [x["score"] for x in got], G[f"m{n}_users"].tolist(), ws, sep)
        sep_n, pos_n = sep_n + a, pos_n + b
    # the tenth position of a full row is never counted as separated, yet counts as a position
    assert sep_n / pos_n > 0.9
