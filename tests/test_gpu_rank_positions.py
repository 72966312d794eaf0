"""Exact full-ranking positions on the GPU (lgcn_amd.metrics.rank_positions / evaluate_auc,
csrc/lgcn_rankpos.hip, utils.ranking_eval.evaluate_auc, utils.recommend.rank_for_user).

The oracle is existing code, never the code under test: lgcn_score_filter's dense keys for the same
normalised rows, ranked by sorting in rank_position_checker.py. The kernel counts integers under the
same keys, so positions, keys and eligible counts must be EQUAL, with no tolerance."""
import functools

import numpy as np
import pytest
import torch

from rank_position_checker import key_scores, positions_from_keys, summaries64

pytestmark = pytest.mark.gpu

# (d, Q, M): padded widths (8 -> 8, 48 -> 64), padded and several query groups, M no multiple of 32,
# several candidate chunks; d = 128 is the width that takes 4 targets per pass, the others take 8.
# (16, 40, 70) and (24, 40, 70) run the compiled widths 16 and 32 (24 pads to 32): two waves of one
# workgroup with padding queries, three candidate blocks with the last one partial
SHAPES = [(8, 5, 33), (64, 70, 100), (48, 130, 1000), (128, 33, 257), (256, 20, 300), (64, 200, 5000),
          (16, 40, 70), (24, 40, 70)]
TRUTH_LENGTHS = (0, 1, 5, 4, 8, 9, 40)  # none, one, a few, Tc and Tc + 1 of either kind, several passes


def _dense_keys(gpu, queries, picked, candidates):
    """uint32 [Q, M]: lgcn_score_filter's dense keys of queries[picked] against candidates."""
    from lgcn_amd import _ffi, _serving
    from lgcn_amd.recall import _normalize_into

    lib, s = _ffi.load(), _ffi.stream_of(gpu)
    Q, M, d = picked.numel(), candidates.shape[0], queries.shape[1]
    D, Qpad = _serving.width("test", d), -(-Q // 128) * 128
    Qn = torch.empty((Qpad, D), dtype=torch.float32, device=gpu)
    Cn = torch.empty((M, D), dtype=torch.float32, device=gpu)
    picked = picked.to(gpu).contiguous()
    _normalize_into(lib, queries, picked.data_ptr(), Q, Qn.data_ptr(), D, Qpad, s)
    _normalize_into(lib, candidates, None, M, Cn.data_ptr(), D, M, s)
    keys = torch.empty((Qpad, M), dtype=torch.int32, device=gpu)
    idx = torch.empty((Qpad, M), dtype=torch.int32, device=gpu)
    _ffi.check(lib.lgcn_score_filter(Qn.data_ptr(), Qpad, Q, Cn.data_ptr(), M, 1, D, None, keys.data_ptr(),
                                     idx.data_ptr(), None, M, s), "lgcn_score_filter")
    return keys[:Q].cpu().numpy().view(np.uint32)


def _csr(rows, dev):
    ptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    idx = np.concatenate([np.asarray(r, np.int32) for r in rows] + [np.zeros(0, np.int32)]).astype(np.int32)
    return torch.from_numpy(ptr).to(dev), torch.from_numpy(idx).to(dev)


def _compare(got, want, what=""):
    ptr, pos, key, eligible = want
    assert got.pos.dtype == torch.int32 and got.eligible.dtype == torch.int32 and got.score.dtype == torch.float32
    np.testing.assert_array_equal(got.ptr.cpu().numpy(), ptr, err_msg=what)
    np.testing.assert_array_equal(got.eligible.cpu().numpy(), eligible, err_msg=what)
    np.testing.assert_array_equal(got.score.cpu().numpy().view(np.uint32), key_scores(key).view(np.uint32), err_msg=what)
    np.testing.assert_array_equal(got.pos.cpu().numpy(), pos, err_msg=what)


@functools.lru_cache(maxsize=None)
def _case(d, Q, M):
    """A table of Q + 3 query rows picked out of order, M candidates, a truth CSR and a seen CSR of
    their own row counts reached through rows= (some rows outside either CSR)."""
    rng = np.random.default_rng(d * 1000003 + Q * 1009 + M)
    queries = rng.standard_normal((Q + 3, d)).astype(np.float32)
    cands = rng.standard_normal((M, d)).astype(np.float32)
    picked = rng.permutation(Q + 3)[:Q].astype(np.int64)
    long_seen = 600 if M == 1000 else 2500 if M == 5000 else 0
    truth, seen = [], []
    for t in range(len(TRUTH_LENGTHS) + 2):
        n = min(TRUTH_LENGTHS[t % len(TRUTH_LENGTHS)], M)
        truth.append(np.sort(rng.choice(M, n, replace=False)).astype(np.int32))
    for t in range(6):
        n = (0, 3, min(M // 2, 17), long_seen, 1, long_seen + 1 if long_seen else 2)[t]
        seen.append(np.sort(rng.choice(M, n, replace=False)).astype(np.int32))
    truth[1] = seen[4].copy()  # query 1 (truth row 1, seen row 4): its one target is a seen item
    trow = rng.integers(-1, len(truth) + 1, Q).astype(np.int64)  # -1 and len(truth): outside the CSR
    trow[:len(truth)] = np.arange(len(truth))[:Q]                # every kind of row is used
    srow = rng.integers(-2, len(seen) + 2, Q).astype(np.int64)
    srow[:len(seen)] = np.arange(len(seen))[::-1][:Q]
    return queries, cands, picked, truth, seen, trow, srow


def _rows_of(rows, which):
    return lambda q: rows[which[q]] if 0 <= which[q] < len(rows) else []


@pytest.mark.parametrize("d,Q,M", SHAPES)
def test_positions_equal_the_sorted_filter_keys(gpu, d, Q, M):
    from lgcn_amd.metrics import rank_positions

    queries, cands, picked, truth, seen, trow, srow = _case(d, Q, M)
    t = lambda a: torch.from_numpy(a).to(gpu)
    keys = _dense_keys(gpu, t(queries), t(picked), t(cands))
    want = positions_from_keys(keys, _rows_of(truth, trow), _rows_of(seen, srow))
    tcsr, scsr = _csr(truth, gpu), _csr(seen, gpu)
    got = rank_positions(t(queries), t(picked), t(cands), tcsr, seen=(*scsr, t(srow)), rows=t(trow))
    _compare(got, want, f"{d} {Q} {M}")
    assert (want[1] >= 0).any() and (want[1] == -1).any()  # ranked targets, and targets found in a seen row
    if M >= 5000:
        assert (want[1] > 1024).any()  # below any list's reach
    # two runs give identical bytes
    again = rank_positions(t(queries), t(picked), t(cands), tcsr, seen=(*scsr, t(srow)), rows=t(trow))
    assert torch.equal(again.pos, got.pos) and torch.equal(again.eligible, got.eligible)
    assert torch.equal(again.score.view(torch.int32), got.score.view(torch.int32))
    # without a seen CSR nothing is dropped
    bare = rank_positions(t(queries), t(picked), t(cands), tcsr, rows=t(trow))
    _compare(bare, positions_from_keys(keys, _rows_of(truth, trow), lambda q: []), f"{d} {Q} {M} no seen")


@functools.lru_cache(maxsize=None)
def _tie_case():
    """Candidates drawn with repetition from a small pool (repeated rows tie exactly: the index rule
    decides), two zero candidate rows (NaN keys, ranked first), one zero query row (every key NaN)."""
    rng = np.random.default_rng(77)
    d, Q, M = 16, 40, 300
    pool = rng.standard_normal((20, d)).astype(np.float32)
    cands = pool[rng.integers(0, 20, M)].copy()
    cands[[3, 77]] = 0.0
    queries = rng.standard_normal((Q, d)).astype(np.float32)
    queries[5] = 0.0
    truth = [np.sort(rng.choice(M, rng.integers(1, 12), replace=False)).astype(np.int32) for _ in range(Q)]
    truth[0] = np.array([3, 50, 77], np.int32)  # the NaN candidates as targets
    seen = [np.sort(rng.choice(M, rng.integers(0, 30), replace=False)).astype(np.int32) for _ in range(Q)]
    seen[0] = np.union1d(seen[0], [50]).astype(np.int32)  # a target that is seen
    return queries, cands, truth, seen


def test_ties_and_nan_go_by_index(gpu):
    from lgcn_amd.metrics import rank_positions

    queries, cands, truth, seen = _tie_case()
    t = lambda a: torch.from_numpy(a).to(gpu)
    keys = _dense_keys(gpu, t(queries), torch.arange(len(queries)), t(cands))
    assert (keys[:, [3, 77]] == 0xFFFFFFFF).all() and (keys[5] == 0xFFFFFFFF).all()
    assert max(len(np.unique(row)) for row in keys) <= 21  # the rows are full of exact ties
    want = positions_from_keys(keys, lambda q: truth[q], lambda q: seen[q])
    got = rank_positions(t(queries), torch.arange(len(queries)), t(cands), _csr(truth, gpu), seen=_csr(seen, gpu))
    _compare(got, want, "ties")
    # the all-NaN query ranks by index alone
    lo, hi = want[0][5], want[0][6]
    rank_by_index = [int(np.sum(~np.isin(np.arange(j), seen[5]))) if j not in seen[5] else -1 for j in truth[5]]
    assert want[1][lo:hi].tolist() == rank_by_index


@pytest.mark.parametrize("which", ["ties", (64, 70, 100), (128, 33, 257)])
def test_positions_are_the_slots_of_topk_rows(gpu, which):
    """pos = p < k exactly when topk_rows puts the item at slot p: here k = M, every slot."""
    from lgcn_amd.metrics import rank_positions
    from lgcn_amd.recommend import topk_rows

    t = lambda a: torch.from_numpy(a).to(gpu)
    if which == "ties":
        queries, cands, truth, seen = _tie_case()
        picked, tcsr, seen_arg, rows = torch.arange(len(queries)), _csr(truth, gpu), _csr(seen, gpu), None
    else:
        queries, cands, picked, truth, seen, trow, srow = _case(*which)
        picked, tcsr, seen_arg, rows = t(picked), _csr(truth, gpu), (*_csr(seen, gpu), t(srow)), t(trow)
    M = cands.shape[0]
    got = rank_positions(t(queries), picked, t(cands), tcsr, seen=seen_arg, rows=rows)
    idx, score = topk_rows(t(queries), picked, t(cands), M, excl=seen_arg, index_dtype=torch.int32)
    idx, score = idx.cpu().numpy(), score.cpu().numpy()
    ptr, pos, sc = got.ptr.cpu().numpy(), got.pos.cpu().numpy(), got.score.cpu().numpy()
    tptr, tidx = (a.cpu().numpy() for a in tcsr)
    rows = None if rows is None else rows.cpu().numpy()
    checked = dropped = 0
    for q in range(len(ptr) - 1):
        r = q if rows is None else int(rows[q])
        items = tidx[tptr[r]:tptr[r + 1]] if 0 <= r < len(tptr) - 1 else []
        assert len(items) == ptr[q + 1] - ptr[q]
        for j, p, s in zip(items, pos[ptr[q]:ptr[q + 1]], sc[ptr[q]:ptr[q + 1]]):
            if p >= 0:
                assert idx[q, p] == j and score[q, p].view(np.uint32) == s.view(np.uint32)
                checked += 1
            else:
                assert j not in idx[q]
                dropped += 1
    assert checked > 50 and dropped > 0
    assert (got.eligible.cpu().numpy() == (idx >= 0).sum(1)).all()


def test_dropped_targets_leave_the_others_alone(gpu):
    from lgcn_amd.metrics import rank_positions

    queries, cands, picked, truth, seen, _, _ = _case(64, 70, 100)
    t = lambda a: torch.from_numpy(a).to(gpu)
    Q, M = 12, cands.shape[0]
    rng = np.random.default_rng(3)
    srows = [seen[2]] * Q
    unseen = np.setdiff1d(np.arange(M), seen[2])
    clean = [np.sort(rng.choice(unseen, 6, replace=False)).astype(np.int32) for _ in range(Q)]
    extra = [np.array([-5, M, M + 40, 2 ** 31 - 1, *seen[2][:3]], np.int32) for _ in range(Q)]
    dirty = [np.concatenate([c[:2], e[:4], c[2:], e[4:]]) for c, e in zip(clean, extra)]  # unsorted on purpose
    a = rank_positions(t(queries), t(picked[:Q]), t(cands), _csr(clean, gpu), seen=_csr(srows, gpu))
    b = rank_positions(t(queries), t(picked[:Q]), t(cands), _csr(dirty, gpu), seen=_csr(srows, gpu))
    pa, pb, bptr = a.pos.cpu().numpy(), b.pos.cpu().numpy(), b.ptr.cpu().numpy()
    assert (pa >= 0).all() and torch.equal(a.eligible, b.eligible)
    at = 0
    for q in range(Q):
        n = len(clean[q])
        row = pb[bptr[q]:bptr[q + 1]]
        assert row[2:6].tolist() == [-1] * 4 and row[n + 4:].tolist() == [-1] * 3
        assert np.concatenate([row[:2], row[6:n + 4]]).tolist() == pa[at:at + n].tolist()
        at += n
    assert torch.isnan(b.score[2:6]).all()  # outside [0, M): no score; a seen item keeps its score
    assert not torch.isnan(b.score[bptr[1] - 3:bptr[1]]).any()


def test_the_same_pair_ranks_the_same_anywhere(gpu):
    """Alone, in a batch, at any batch position, from a strided or non-contiguous table, with the
    seen row reached directly or through rows."""
    from lgcn_amd.metrics import rank_positions

    queries, cands, picked, truth, seen, trow, srow = _case(48, 130, 1000)
    t = lambda a: torch.from_numpy(a).to(gpu)
    tcsr, scsr = _csr(truth, gpu), _csr(seen, gpu)
    full = rank_positions(t(queries), t(picked), t(cands), tcsr, seen=(*scsr, t(srow)), rows=t(trow))
    ptr = full.ptr.cpu().numpy()
    wide_q = torch.zeros((queries.shape[0], 80), device=gpu)
    wide_q[:, 16:64] = t(queries)
    wide_c = torch.zeros((2 * cands.shape[0], 50), device=gpu)
    wide_c[::2, 1:49] = t(cands)
    qv, cv = wide_q[:, 16:64], wide_c[::2, 1:49]
    assert not qv.is_contiguous() and not cv.is_contiguous()
    for q in (0, 2, 3, 6, 77, 129):  # 0, 2: seen rows above 512 entries; 6: the truth row of 40
        lone = rank_positions(qv, t(picked[q:q + 1]), cv, tcsr, seen=(*scsr, t(srow[q:q + 1])), rows=t(trow[q:q + 1]))
        assert torch.equal(lone.pos, full.pos[ptr[q]:ptr[q + 1]]) and lone.eligible[0] == full.eligible[q]
        assert torch.equal(lone.score.view(torch.int32), full.score[ptr[q]:ptr[q + 1]].view(torch.int32))
    # reversed batch order; the seen rows laid out one per query, no rows argument
    rev = np.arange(len(picked))[::-1].copy()
    direct = _csr([_rows_of(seen, srow)(q) for q in rev], gpu)
    back = rank_positions(qv, t(picked[rev]), cv, tcsr, seen=direct, rows=t(trow[rev]))
    bptr = back.ptr.cpu().numpy()
    for n, q in enumerate(rev):
        assert torch.equal(back.pos[bptr[n]:bptr[n + 1]], full.pos[ptr[q]:ptr[q + 1]]), q
    assert torch.equal(back.eligible, full.eligible.flip(0))


def test_long_truth_rows_get_calls_of_their_own(gpu):
    """Truth rows above metrics.TIER_LENGTHS (300 and 700 entries; 40 entries) put their queries in
    separate library calls, on 128-query boundaries; every position still equals the oracle's and
    comes back in the caller's order."""
    from lgcn_amd import metrics

    queries, cands, _, _, seen, _, srow = _case(48, 130, 1000)
    rng = np.random.default_rng(9)
    Q, M = 300, cands.shape[0]
    picked = rng.integers(0, queries.shape[0], Q).astype(np.int64)
    truth = [np.sort(rng.choice(M, n, replace=False)).astype(np.int32) for n in (3, 300, 0, 40, 700, 1)]
    trow = rng.choice(np.array([0, 2, 3, 3, 3, 3, 5]), Q).astype(np.int64)  # more than 128 rows of 40
    trow[[7, 150, 299]] = [1, 4, 1]  # three long rows among 300 queries
    srows = np.resize(srow, Q)
    t = lambda a: torch.from_numpy(a).to(gpu)
    lens = np.array([len(truth[r]) for r in trow])
    assert metrics._tiers(Q, [(lens > n).sum() for n in metrics.TIER_LENGTHS]) == [(0, 128), (128, 256), (256, 300)]
    keys = _dense_keys(gpu, t(queries), t(picked), t(cands))
    want = positions_from_keys(keys, _rows_of(truth, trow), _rows_of(seen, srows))
    got = metrics.rank_positions(t(queries), t(picked), t(cands), _csr(truth, gpu), seen=(*_csr(seen, gpu), t(srows)),
                                 rows=t(trow))
    _compare(got, want, "tiers")


def test_unit_rows_are_taken_as_they_are(gpu):
    from lgcn_amd.metrics import rank_positions

    queries, cands, picked, truth, seen, trow, srow = _case(64, 70, 100)
    t = lambda a: torch.from_numpy(a).to(gpu)
    unit = lambda x: x / x.norm(dim=1, keepdim=True)
    args = dict(seen=(*_csr(seen, gpu), t(srow)), rows=t(trow))
    a = rank_positions(unit(t(queries)), t(picked), unit(t(cands)), _csr(truth, gpu), normalized=True, **args)
    keys = _dense_keys(gpu, unit(t(queries)), t(picked), unit(t(cands)))  # re-normalising moves a few last bits
    assert a.pos.numel() == positions_from_keys(keys, _rows_of(truth, trow), _rows_of(seen, srow))[1].size
    assert ((a.pos >= 0) == (rank_positions(t(queries), t(picked), t(cands), _csr(truth, gpu), **args).pos >= 0)).all()


def test_empty_inputs(gpu):
    from lgcn_amd.metrics import rank_positions, summarize_positions

    q, c = torch.randn(4, 24, device=gpu), torch.randn(50, 24, device=gpu)
    none = (torch.zeros(5, dtype=torch.int64, device=gpu), torch.zeros(0, dtype=torch.int32, device=gpu))
    seen = _csr([[1, 2], [], [7, 60], [0]], gpu)
    got = rank_positions(q, torch.arange(4), c, none, seen=seen)
    assert got.pos.shape == (0,) and got.score.shape == (0,) and got.ptr.tolist() == [0] * 5
    assert got.eligible.tolist() == [48, 50, 49, 49]
    assert rank_positions(q, torch.arange(4), c, none).eligible.tolist() == [50] * 4
    assert summarize_positions(got, (5,))["users"] == 0
    got = rank_positions(q, torch.arange(0), c, none, seen=seen)
    assert got.pos.shape == (0,) and got.eligible.shape == (0,) and got.ptr.tolist() == [0]
    one = rank_positions(q, torch.arange(4), c[:0], _csr([[0], [], [3], []], gpu))  # no candidates: nothing ranks
    assert one.pos.tolist() == [-1, -1] and one.eligible.tolist() == [0] * 4


# --------------------------------------------------------------------------------------------
# end to end

@functools.lru_cache(maxsize=None)
def _table():
    """A trained-like table: users near a few item clusters, seen rows of 0-60 items, 1-8 held-out
    items per user outside the seen row (every seventh user none)."""
    rng = np.random.default_rng(2024)
    U, I, d = 300, 2000, 64
    centres = rng.standard_normal((12, d)).astype(np.float32)
    ie = (centres[rng.integers(0, 12, I)] + 0.7 * rng.standard_normal((I, d))).astype(np.float32)
    ue = (centres[rng.integers(0, 12, U)] + 0.7 * rng.standard_normal((U, d))).astype(np.float32)
    seen = [np.sort(rng.choice(I, rng.integers(0, 61), replace=False)).astype(np.int32) for _ in range(U)]
    truth = []
    for u in range(U):
        free = np.setdiff1d(np.arange(I), seen[u])
        n = 0 if u % 7 == 0 else rng.integers(1, 9)
        truth.append(np.sort(rng.choice(free, n, replace=False)).astype(np.int32))
    return ue, ie, seen, truth


def test_evaluate_auc_matches_the_checker_and_evaluate_ranking(gpu):
    from lgcn_amd import metrics

    ue, ie, seen, truth = _table()
    t = lambda a: torch.from_numpy(a).to(gpu)
    ks = (5, 20)
    got = metrics.evaluate_auc(t(ue), t(ie), _csr(truth, gpu), seen=_csr(seen, gpu), ks=ks)
    users = np.flatnonzero([len(x) > 0 for x in truth])
    keys = _dense_keys(gpu, t(ue), t(users), t(ie))
    want = summaries64(*[positions_from_keys(keys, lambda q: truth[users[q]], lambda q: seen[users[q]])[i]
                         for i in (0, 1, 3)], ks)
    assert got["users"] == want["users"] == users.size and set(got) == set(want)
    for name, w in want.items():
        print(f"{name}: {got[name]!r} (checker {w!r})")
        assert abs(got[name] - w) <= 1e-12, name
    assert 0.0 < got["auc"] < 1.0 and got["mean_rank"] > 20  # most held-out items lie below the cutoffs
    lists = metrics.evaluate_ranking(t(ue), t(ie), _csr(truth, gpu), ks=ks, seen=_csr(seen, gpu))
    assert lists["users"] == got["users"]
    for c in ks:
        for m in ("recall", "precision", "hit_rate", "mrr"):
            assert got[f"{m}@{c}"] == lists[f"{m}@{c}"], (m, c)  # integer hit counts: equal
        assert abs(got[f"ndcg@{c}"] - lists[f"ndcg@{c}"]) <= 1e-6
    # users given explicitly, cutoffs beyond every list's reach, and no cutoffs at all
    deep = metrics.evaluate_auc(t(ue), t(ie), _csr(truth, gpu), seen=_csr(seen, gpu), users=t(users), ks=(1500, 20))
    assert deep["auc"] == got["auc"] and deep["recall@20"] == got["recall@20"] and deep["recall@1500"] > 4 * got["recall@20"]
    assert set(metrics.evaluate_auc(t(ue), t(ie), _csr(truth, gpu))) == {"users", "auc", "mpr", "mrr", "mean_rank"}


def test_harness_evaluate_auc_and_rank_for_user(gpu, tmp_path, monkeypatch):
    from data.dataset_handler import MovieLensDataHandler, write_synthetic_movielens
    from lgcn_amd import metrics
    from lgcn_amd.recommend import seen_csr
    from models.light_gcn import LightGCN
    from utils import ranking_eval as T
    from utils import recommend as R

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
    with torch.no_grad():
        raw = T.evaluate_auc(model, train, held, gpu, ks=(10,), embeddings="raw")
        want = metrics.evaluate_auc(*model.get_embeddings(torch.arange(U, device=gpu), torch.arange(I, device=gpu)),
                                    truth, seen=seen, ks=(10,))
        assert raw == want and raw["users"] > 0 and 0.0 < raw["auc"] < 1.0
        prop = T.evaluate_auc(model, train, held, gpu, embeddings="propagated")
        assert prop == metrics.evaluate_auc(*model(train), truth, seen=seen) and prop["users"] == raw["users"]
    with pytest.raises(ValueError):
        T.evaluate_auc(model, train, held, gpu, embeddings="final")
    # where do these movies rank: the slots of the served list, None for a seen movie and an unknown id
    uid = next(u for u, i in h.user_id_map.items() if seen[0][i + 1] > seen[0][i])
    served = R.recommend_for_users(model, [uid], h, k=15, train_edge_index=train)[0]
    id_movie = {i: m for m, i in h.movie_id_map.items()}
    a_seen = id_movie[int(seen[1][seen[0][h.user_id_map[uid]]]) + U]
    asked = [served[9]["movie_id"], -12345, served[0]["movie_id"], a_seen, served[14]["movie_id"]]
    got = R.rank_for_user(model, uid, asked, h, train_edge_index=train)
    assert [g["movie_id"] for g in got] == asked and [g["rank"] for g in got] == [10, None, 1, None, 15]
    assert all(set(g) == {"movie_id", "title", "rank", "score", "of"} for g in got)
    assert got[0]["title"] == served[9]["title"] and got[0]["score"] == served[9]["score"]
    assert got[1]["title"] is None and got[3]["title"] is not None and got[3]["score"] is None
    n_seen = int(seen[0][h.user_id_map[uid] + 1] - seen[0][h.user_id_map[uid]])
    assert all(g["of"] == I - n_seen for g in got)
    everything = R.rank_for_user(model, uid, [a_seen], h, exclude_seen=False)
    assert everything[0]["rank"] is not None and everything[0]["of"] == I

    def no_device(*a, **k):
        raise AssertionError("an unknown user must be answered without touching the GPU")

    monkeypatch.setattr(metrics, "rank_positions", no_device)
    monkeypatch.setattr(model, "get_embeddings", no_device)
    assert R.rank_for_user(model, -1, asked, h) == {"error": "Invalid user ID"}
