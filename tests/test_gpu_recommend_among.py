"""Per-query candidate sets on the GPU (lgcn_amd.recommend.topk_rows' among, utils.recommend's among,
utils.ranking_eval.evaluate_sampled; lgcn_score_lists of csrc/lgcn_recall_among.hip).

The oracle is today's path: the same request written as exclusion rows — the complement of the
query's set, joined with whatever else is excluded — through topk_rows without among, in dense
mode; above the dense capacity, rank_positions' exact positions. Keys come from the same MFMA chain
everywhere, so every comparison is torch.equal on the indices and on the scores' bits; there is no
tolerance."""
import numpy as np
import pandas as pd
import pytest
import torch

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 31, 32, 33, 511, 512, 513, 4097]  # both sides of the one-wave / many-wave boundary


def _emb(rng, n, d):
    return rng.standard_normal((n, d)).astype(np.float32)


def _csr(rows, dev):
    ptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    idx = np.concatenate([np.asarray(r, np.int32) for r in rows] + [np.zeros(0, np.int32)])
    return torch.from_numpy(ptr).to(dev), torch.from_numpy(idx).to(dev)


def _same(a, b):
    """Indices equal and scores equal to the bit (NaN included)."""
    return torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def _row(rng, length, M):
    """A shuffled row of ``length`` entries: distinct candidates of [0, M), and entries that name
    nothing (-1, M, ...) in about a quarter of the slots and wherever M runs out."""
    valid = min(length - length // 4, M)
    junk = rng.choice(np.array([-1, M, M + 5, -7, 2 ** 31 - 1]), length - valid)
    row = np.concatenate([rng.choice(M, valid, replace=False), junk]).astype(np.int32)
    rng.shuffle(row)
    return row


def _valid(row, M):
    row = np.asarray(row, np.int64)
    return np.unique(row[(row >= 0) & (row < M)])


def _complement(sets, M, extra=None):
    """The oracle's exclusion rows: everything outside query q's set, joined with extra[q]."""
    out = []
    for q, keep in enumerate(sets):
        drop = np.ones(M, bool)
        drop[np.asarray(keep, np.int64)] = False
        if extra is not None:
            drop[np.asarray(extra[q], np.int64)] = True
        out.append(np.nonzero(drop)[0].astype(np.int32))
    return out


def _grid_case(d, M):
    """70 queries over a CSR of 60 rows: LENGTHS, a row naming all M, random short rows; the rows
    argument permutes them, repeats some and names three rows outside the CSR."""
    rng = np.random.default_rng(d * 100003 + M)
    users, cands = _emb(rng, 200, d), _emb(rng, M, d)
    picked = rng.choice(200, 70, replace=False)
    rows = [_row(rng, n, M) for n in LENGTHS] + [rng.permutation(M).astype(np.int32)]
    rows += [_row(rng, int(n), M) for n in rng.integers(0, 120, 60 - len(rows))]
    names = np.concatenate([rng.permutation(60), [8, 8, 9, 3, 60, -1, 63, 5, 8, 0]]).astype(np.int64)
    rng.shuffle(names)
    sets = [_valid(rows[r], M) if 0 <= r < 60 else np.zeros(0, np.int64) for r in names]
    return users, cands, picked, rows, names, sets


@pytest.mark.parametrize("M", [300, 5000])
@pytest.mark.parametrize("d", [5, 64, 100, 256])
@pytest.mark.parametrize("k", [1, 10, 100])
def test_among_equals_the_complement_exclusion_oracle(gpu, d, k, M):
    from lgcn_amd.recommend import topk_rows

    users, cands, picked, rows, names, sets = _grid_case(d, M)
    t = lambda a: torch.from_numpy(a).to(gpu)
    U, C, P = t(users), t(cands), torch.from_numpy(picked)
    got = topk_rows(U, P, C, k, among=(*_csr(rows, gpu), torch.from_numpy(names)))
    want = topk_rows(U, P, C, k, excl=_csr(_complement(sets, M), gpu))
    assert _same(got, want)
    # sorted rows give the same lists as shuffled ones
    assert _same(topk_rows(U, P, C, k, among=(*_csr([np.sort(r) for r in rows], gpu), torch.from_numpy(names))), got)
    # the query whose row names every candidate has its unrestricted list
    q_all = int(np.nonzero(names == len(LENGTHS))[0][0])
    plain = topk_rows(U, P[q_all:q_all + 1], C, k)
    assert _same((got[0][q_all:q_all + 1], got[1][q_all:q_all + 1]), plain)
    # rows outside the CSR and the empty row: all padding
    gi, gs = got[0].cpu().numpy(), got[1].cpu().numpy()
    for q in np.nonzero((names < 0) | (names >= 60) | (names == 0))[0]:
        assert (gi[q] == -1).all() and np.isneginf(gs[q]).all()
    for q, keep in enumerate(sets):  # nothing outside a query's set is ever returned
        n = min(k, len(keep))
        assert np.isin(gi[q, :n], keep).all() and (gi[q, n:] == -1).all() and np.isneginf(gs[q, n:]).all()


def test_short_rows_are_padded(gpu):
    from lgcn_amd.recommend import topk_rows, topk_rows_diverse

    rng = np.random.default_rng(7)
    M, d = 2000, 24
    users, cands = _emb(rng, 6, d), _emb(rng, M, d)
    rows = [_row(rng, 1500, M), np.array([17, 4, 1999], np.int32), np.zeros(0, np.int32),
            rng.choice(M, 1100, replace=False), np.array([5, M, -1], np.int32), rng.choice(M, 700, replace=False)]
    excl = [np.sort(rng.choice(M, 400, replace=False)) for _ in range(6)]
    excl[1], excl[4] = np.array([4], np.int32), np.array([6, 9], np.int32)
    t = lambda a: torch.from_numpy(a).to(gpu)
    for k in (1024, 5):
        idx, score = topk_rows(t(users), torch.arange(6), t(cands), k, among=_csr(rows, gpu), excl=_csr(excl, gpu))
        idx, score = idx.cpu().numpy(), score.cpu().numpy()
        for q in range(6):
            left = np.setdiff1d(_valid(rows[q], M), excl[q])
            n = min(k, len(left))
            assert (idx[q, :n] >= 0).all() and set(idx[q, :n]) <= set(left) and len(set(idx[q, :n])) == n, q
            assert (idx[q, n:] == -1).all() and np.isneginf(score[q, n:]).all(), q
            if n == len(left):
                assert set(idx[q, :n]) == set(left)
    assert len(np.setdiff1d(_valid(rows[0], M), excl[0])) < 1024 < len(rows[0])  # k = 1024 against a row of 1,500
    got = topk_rows_diverse(t(users), torch.arange(6), t(cands), 8, 0.3, pool=64, among=_csr(rows, gpu),
                            excl=_csr(excl, gpu))
    want_n = [min(8, len(np.setdiff1d(_valid(rows[q], M), excl[q]))) for q in range(6)]
    assert got.n.tolist() == want_n and want_n[1] == 2 and want_n[2] == 0 and want_n[4] == 1
    for q in range(6):
        assert set(got.idx[q, :want_n[q]].tolist()) <= set(_valid(rows[q], M).tolist())
        assert (got.idx[q, want_n[q]:] == -1).all()


def test_ties_nan_and_a_duplicated_entry(gpu):
    from lgcn_amd.recommend import topk_rows

    rng = np.random.default_rng(11)
    M, d, k = 400, 64, 50
    users, cands = _emb(rng, 8, d), _emb(rng, M, d)
    cands[[20, 30, 300]] = cands[10]  # equal keys: ranked by index ascending
    cands[7] = np.nan                 # an all-NaN row: ranked first
    rows = [np.concatenate([[7, 300, 10, 30, 20], rng.choice(np.arange(40, 290), n, replace=False)]).astype(np.int32)
            for n in (0, 20, 45, 100, 200, 250, 27)]
    # a row for the many-wave path: every candidate of 40 .. 289 among 300 entries that name nothing
    rows.append(np.concatenate([rows[0], np.arange(40, 290), np.tile([-1, M], 150)]).astype(np.int32))
    assert len(rows[7]) > 512
    rows = [rng.permutation(r) for r in rows]
    t = lambda a: torch.from_numpy(a).to(gpu)
    args = (t(users), torch.arange(8), t(cands))
    got = topk_rows(*args, k, among=_csr(rows, gpu))
    want = topk_rows(*args, k, excl=_csr(_complement([_valid(r, M) for r in rows], M), gpu))
    assert _same(got, want)
    gi = got[0].cpu().numpy()
    assert (gi[:, 0] == 7).all() and torch.isnan(got[1][:, 0]).all()
    assert gi[0].tolist()[:5] == [7] + sorted(gi[0].tolist()[1:5]) and set(gi[0].tolist()[1:5]) == {10, 20, 30, 300}
    for q in range(8):  # the four equal rows stand together, by index
        at = np.nonzero(gi[q] == 10)[0]
        if len(at) and at[0] + 4 <= k:
            assert gi[q, at[0]:at[0] + 4].tolist() == [10, 20, 30, 300]
    # an entry named twice is ranked twice, in adjacent slots: the deduplicated list with the copy inserted
    for dup in (7, int(want[0][3, 1]), int(want[0][3, 5]), int(want[0][3, k - 1])):
        twice = [np.concatenate([r, [dup]]).astype(np.int32) if q == 3 else r for q, r in enumerate(rows)]
        gd = topk_rows(*args, k, among=_csr(twice, gpu))
        wi, ws = want[0][3].tolist(), want[1][3].view(torch.int32).tolist()
        at = wi.index(dup)
        assert gd[0][3].tolist() == (wi[:at + 1] + wi[at:])[:k]
        assert gd[1][3].view(torch.int32).tolist() == (ws[:at + 1] + ws[at:])[:k]
        keep = [q for q in range(8) if q != 3]
        assert _same((gd[0][keep], gd[1][keep]), (want[0][keep], want[1][keep]))


def test_among_composes_with_exclusion_filter_wrappers_and_diversity(gpu):
    from lgcn_amd.recommend import candidate_csr, topk_items, topk_rows, topk_rows_diverse

    rng = np.random.default_rng(13)
    U, M, d, k = 90, 1500, 48, 20
    users, items = _emb(rng, U, d), _emb(rng, M, d)
    sets = [np.sort(rng.choice(M, int(n), replace=False)) for n in rng.integers(0, 700, U)]
    sets[4] = np.arange(M)
    seen = [np.sort(rng.choice(M, int(n), replace=False)) for n in rng.integers(0, 300, U)]
    attr = rng.integers(0, 16, M).astype(np.int32)
    t = lambda a: torch.from_numpy(a).to(gpu)
    Ut, It = t(users), t(items)
    allq = torch.arange(U)
    among, excl = _csr(sets, gpu), _csr(seen, gpu)
    # among + excl: the union exclusion
    got = topk_rows(Ut, allq, It, k, among=among, excl=excl)
    assert _same(got, topk_rows(Ut, allq, It, k, excl=_csr(_complement(sets, M, seen), gpu)))
    # among + attrs / where: a per-query `any` column, `none` for all, and "nothing passes" for some
    any_ = rng.integers(0, 16, U)
    all_ = np.where(np.arange(U) % 7 == 0, 1 << 20, 0)  # bit 20 is set on no item
    passes = ((attr[None, :] & 8) == 0) & ((attr[None, :] & all_[:, None]) == all_[:, None]) & \
        ((any_[:, None] == 0) | ((attr[None, :] & any_[:, None]) != 0))
    fails = [np.nonzero(~passes[q])[0] for q in range(U)]
    where = (torch.from_numpy(any_), all_.tolist(), 8)
    got = topk_rows(Ut, allq, It, k, among=among, attrs=t(attr), where=where)
    assert _same(got, topk_rows(Ut, allq, It, k, excl=_csr(_complement(sets, M, fails), gpu)))
    assert (got[0][::7] == -1).all()
    both = [np.union1d(seen[q], fails[q]) for q in range(U)]
    got = topk_rows(Ut, allq, It, k, among=among, excl=excl, attrs=t(attr), where=where)
    assert _same(got, topk_rows(Ut, allq, It, k, excl=_csr(_complement(sets, M, both), gpu)))
    # topk_items: a 2-tuple is a CSR over all users, row u being user u's
    some = torch.tensor([5, 88, 4, 4, 17, 0])
    got = topk_items(Ut, It, some, k, seen=excl, among=among)
    pick = some.tolist()
    want = topk_rows(Ut, some, It, k, excl=_csr(_complement([sets[u] for u in pick], M, [seen[u] for u in pick]), gpu))
    assert _same(got, want)
    assert _same(topk_items(Ut, It, some, k, seen=excl, among=(*among, some)), want)
    # candidate_csr of padded lists is the CSR of the sets
    width = max(len(s) for s in sets[:10])
    padded = np.full((10, width + 3), -1, np.int64)
    for q in range(10):
        padded[q, :len(sets[q])] = rng.permutation(sets[q])
        padded[q, width:] = sets[q][:3] if len(sets[q]) >= 3 else -1  # copies: deduplicated
    cp, ci = candidate_csr(t(padded))
    wp, wi = _csr(sets[:10], gpu)
    assert torch.equal(cp, wp) and torch.equal(ci, wi)
    # the diverse lists' picks all lie in the row, and diversity 0 keeps the among ranking
    div = topk_rows_diverse(Ut, allq, It, 10, 0.4, pool=40, among=among, excl=excl)
    rel = topk_rows_diverse(Ut, allq, It, 10, 0.0, pool=40, among=among, excl=excl)
    base = topk_rows(Ut, allq, It, 10, among=among, excl=excl)
    assert _same((rel.idx, rel.score), base)
    di = div.idx.cpu().numpy()
    for q in range(U):
        n = int(div.n[q])
        assert n == min(10, len(np.setdiff1d(sets[q], seen[q]))) and np.isin(di[q, :n], sets[q]).all()
        assert not np.isin(di[q, :n], seen[q]).any() and (di[q, n:] == -1).all()


def test_above_the_dense_capacity_the_order_is_rank_positions(gpu):
    from lgcn_amd import recommend
    from lgcn_amd.metrics import rank_positions

    rng = np.random.default_rng(17)
    M, Q, d, n = 20000, 40, 64, 200
    assert M > recommend.CAP
    users, cands = _emb(rng, Q, d), _emb(rng, M, d)
    cands[rng.choice(M, 50, replace=False)] = cands[123]  # ties in the full ranking too
    rows = [rng.choice(M, n, replace=False).astype(np.int32) for _ in range(Q)]
    rows[0] = np.concatenate([[123, 5000, 9], rng.choice(np.arange(10, 5000), n - 3, replace=False)]).astype(np.int32)
    t = lambda a: torch.from_numpy(a).to(gpu)
    csr = _csr(rows, gpu)
    idx, score = recommend.topk_rows(t(users), torch.arange(Q), t(cands), n, among=csr)
    pos = rank_positions(t(users), torch.arange(Q), t(cands), csr)
    p = pos.pos.view(Q, n).to(torch.int64)
    assert (p >= 0).all()
    order = torch.argsort(p, 1)
    assert torch.equal(p.gather(1, order)[:, 1:] > p.gather(1, order)[:, :-1], torch.ones((Q, n - 1), dtype=torch.bool, device=gpu))
    assert torch.equal(idx, csr[1].view(Q, n).to(torch.int64).gather(1, order))
    assert torch.equal(score.view(torch.int32), pos.score.view(Q, n).gather(1, order).view(torch.int32))


def _spy(monkeypatch):
    """(capacity, queries) of every lgcn_score_lists call recommend makes."""
    from lgcn_amd import _ffi

    lib, calls = _ffi.load(), []
    real = lib.lgcn_score_lists

    def spying(*a):
        calls.append((a[12], a[1]))
        return real(*a)

    monkeypatch.setattr(lib, "lgcn_score_lists", spying, raising=False)
    return calls


def test_blocks_follow_the_row_lengths(gpu, monkeypatch):
    from lgcn_amd import recommend

    d, k, M = 64, 10, 5000
    users, cands, picked, rows, names, sets = _grid_case(d, M)
    t = lambda a: torch.from_numpy(a).to(gpu)
    U, C, P = t(users), t(cands), torch.from_numpy(picked)
    among = (*_csr(rows, gpu), torch.from_numpy(names))
    calls = _spy(monkeypatch)
    whole = recommend.topk_rows(U, P, C, k, among=among)
    assert calls == [(M, 70)]  # one block at the default workspace
    del calls[:]
    monkeypatch.setattr(recommend, "BLOCK_BYTES", 8 * M)
    split = recommend.topk_rows(U, P, C, k, among=among)
    assert _same(split, whole) and len(calls) >= 5 and sum(n for _, n in calls) == 70
    assert [c for c, _ in calls] == sorted((c for c, _ in calls), reverse=True) and min(c for c, _ in calls) >= k
    for cap, n in calls[:-1]:  # every block but the last is as large as its capacity lets it be
        assert n == max(1, M // cap)
    assert 1 <= calls[-1][1] <= max(1, M // calls[-1][0])
    # one 4,097-entry row among rows of at most 33: only its own block has its capacity
    rng = np.random.default_rng(3)
    few = [_row(rng, int(n), M) for n in rng.integers(0, 34, 69)]
    few.insert(40, _row(rng, 4097, M))
    del calls[:]
    monkeypatch.setattr(recommend, "BLOCK_BYTES", 8 * 4097 * 2)
    got = recommend.topk_rows(U, P, C, k, among=_csr(few, gpu))
    assert calls[0][0] == 4097 and calls[0][1] <= 2 and all(cap <= 33 for cap, _ in calls[1:])
    assert max(cap for cap, _ in calls[1:]) >= k and sum(n for _, n in calls) == 70
    monkeypatch.setattr(recommend, "BLOCK_BYTES", 1 << 30)
    assert _same(got, recommend.topk_rows(U, P, C, k, among=_csr(few, gpu)))


def test_raw_entry_point_gives_the_filters_keys(gpu):
    from lgcn_amd import _ffi
    from lgcn_amd.recall import _normalize_into

    lib = _ffi.load()
    rng = np.random.default_rng(19)
    M, d, D, Q = 300, 64, 64, 5
    users, cands = torch.from_numpy(_emb(rng, Q, d)).to(gpu), torch.from_numpy(_emb(rng, M, d)).to(gpu)
    s = _ffi.stream_of(gpu)
    Qn = torch.empty((128, D), dtype=torch.float32, device=gpu)
    Cn = torch.empty((M, D), dtype=torch.float32, device=gpu)
    _normalize_into(lib, users, None, Q, Qn.data_ptr(), D, 128, s)
    _normalize_into(lib, cands, None, M, Cn.data_ptr(), D, M, s)
    dkey = torch.empty((128, M), dtype=torch.int32, device=gpu)
    didx = torch.empty((128, M), dtype=torch.int32, device=gpu)
    _ffi.check(lib.lgcn_score_filter(Qn.data_ptr(), 128, Q, Cn.data_ptr(), M, 1, D, None, dkey.data_ptr(), didx.data_ptr(),
                                     None, M, s), "lgcn_score_filter(dense)")
    rows = [_row(rng, 50, M), rng.integers(-3, M + 3, 700).astype(np.int32), np.zeros(0, np.int32),
            _row(rng, 512, M), _row(rng, 513, M)]
    ptr, idx = _csr(rows, gpu)
    for cap in (1024, 8):
        lkey = torch.full((Q, cap), 0x5A5A5A5A, dtype=torch.int32, device=gpu)
        lidx = torch.full((Q, cap), -99, dtype=torch.int32, device=gpu)
        ln = torch.full((Q,), -5, dtype=torch.int32, device=gpu)  # written, not added to
        _ffi.check(lib.lgcn_score_lists(Qn.data_ptr(), Q, Cn.data_ptr(), M, D, ptr.data_ptr(), idx.data_ptr(), None, Q,
                                        lkey.data_ptr(), lidx.data_ptr(), ln.data_ptr(), cap, s), "lgcn_score_lists")
        torch.cuda.synchronize()
        kept = [r[(r >= 0) & (r < M)] for r in rows]
        assert ln.tolist() == [len(r) for r in kept]  # entries past cap are counted
        for q in range(Q):
            n = min(cap, len(kept[q]))
            li = lidx[q, :n].to(torch.int64)
            assert torch.equal(lkey[q, :n], dkey[q].gather(0, li))  # the filter's key of the pair, bit for bit
            if n == len(kept[q]):  # the list is the row's kept entries, each as often as it is named
                assert sorted(li.tolist()) == sorted(kept[q].tolist())
            else:  # ... or cap of them
                have = np.bincount(li.cpu().numpy(), minlength=M)
                assert (have <= np.bincount(kept[q], minlength=M)).all()
            assert (lidx[q, n:] == -99).all() and (lkey[q, n:] == 0x5A5A5A5A).all()  # nothing stored past the count or cap


def test_no_queries_empty_csr_and_int32_indices(gpu):
    from lgcn_amd.recommend import topk_rows

    rng = np.random.default_rng(23)
    users, cands = torch.from_numpy(_emb(rng, 9, 16)).to(gpu), torch.from_numpy(_emb(rng, 50, 16)).to(gpu)
    empty = (torch.zeros(1, dtype=torch.int64, device=gpu), torch.zeros(0, dtype=torch.int32, device=gpu))
    idx, score = topk_rows(users, torch.arange(0), cands, 4, among=empty)
    assert idx.shape == (0, 4) and idx.dtype == torch.int64 and score.shape == (0, 4)
    none = (torch.zeros(10, dtype=torch.int64, device=gpu), torch.zeros(0, dtype=torch.int32, device=gpu))
    for among in (none, (*empty, [0] * 9), (*empty, [5] * 9)):
        idx, score = topk_rows(users, torch.arange(9), cands, 4, among=among)
        assert (idx == -1).all() and torch.isinf(score).all() and (score < 0).all()
    rows = [rng.choice(50, int(n), replace=False) for n in rng.integers(0, 30, 9)]
    a64 = topk_rows(users, torch.arange(9), cands, 4, among=_csr(rows, gpu))
    a32 = topk_rows(users, torch.arange(9), cands, 4, among=_csr(rows, gpu), index_dtype=torch.int32)
    assert a32[0].dtype == torch.int32 and a64[0].dtype == torch.int64
    assert _same((a32[0].to(torch.int64), a32[1]), a64)
    # CPU CSR tensors are moved like excl's
    cpu = tuple(x.cpu() for x in _csr(rows, gpu))
    assert _same(topk_rows(users, torch.arange(9), cands, 4, among=cpu), a64)


class _Handler:
    """40 movies (ids 100, 103, ...) with a genre each, 30 users with five training and two held-out
    edges each, disjoint (global numbering, both directions)."""

    def __init__(self):
        rng = np.random.default_rng(51)
        ids = [100 + 3 * i for i in range(40)]
        self.user_id_map = {1000 + u: u for u in range(30)}
        self.movie_id_map = {m: 30 + i for i, m in enumerate(ids)}
        self.movies = pd.DataFrame({"movieId": ids, "title": [f"Movie {m}" for m in ids],
                                    "genres": [["Comedy", "Horror", "Drama", "Romance"][i % 4] for i in range(40)]})
        drawn = np.stack([rng.choice(40, 7, replace=False) for _ in range(30)]) + 30
        u = np.repeat(np.arange(30), 5)
        i = drawn[:, :5].reshape(-1)
        self.edge_index = torch.from_numpy(np.stack([np.concatenate([u, i]), np.concatenate([i, u])])).long()
        self.heldout = torch.from_numpy(np.stack([np.repeat(np.arange(30), 2), drawn[:, 5:].reshape(-1)])).long()


def test_harness_serves_among_and_the_sampled_protocol(gpu):
    from models.light_gcn import LightGCN
    from utils import ranking_eval
    from utils import recommend as R

    h = _Handler()
    torch.manual_seed(5)
    model = LightGCN(30, 40, num_layers=2, dim_h=32).to(gpu)
    model.eval()
    ids = list(h.user_id_map)[:12] + [-1]
    shared = [100, 103, 130, 999, 160, 217, 130, 181, 190, 205, 112, 145]  # 999 is no movie, 130 named twice
    full = R.recommend_for_users(model, ids, h, k=40)
    for kw in ({}, dict(explain=2), dict(diversity=0.0), dict(genres=["Comedy", "Drama"])):
        base = {k: v for k, v in kw.items() if k != "diversity"}
        ref = R.recommend_for_users(model, ids, h, k=40, **base)
        got = R.recommend_for_users(model, ids, h, k=5, among=shared, **kw)
        assert got[-1] == {"error": "Invalid user ID"}
        for g, f in zip(got[:-1], ref[:-1]):
            assert g == [x for x in f if x["movie_id"] in shared][:5]
        assert any(got[:-1])
    per_user = {u: [100 + 3 * ((u + j) % 40) for j in range(0, 40, 3)] for u in ids[:10]}
    per_user[ids[3]] = []  # an empty set; ids[10] and ids[11] are not in the mapping at all
    got = R.recommend_for_users(model, ids, h, k=8, among=per_user)
    aligned = R.recommend_for_users(model, ids, h, k=8, among=[per_user.get(u, []) for u in ids])
    assert got == aligned and got[3] == [] and got[10] == [] and got[11] == [] and got[12] == {"error": "Invalid user ID"}
    for u, g, f in zip(ids[:10], got, full):
        assert g == [x for x in f if x["movie_id"] in per_user[u]][:8]
    hist = [[100, 103, 130], [999], [118, 121, 124, 160, 163]]
    ref = R.recommend_for_histories(model, hist, h, k=40)
    got = R.recommend_for_histories(model, hist, h, k=4, among=shared)
    assert got[1] == {"error": "No known movie IDs"}
    for g, f in zip((got[0], got[2]), (ref[0], ref[2])):
        assert g == [x for x in f if x["movie_id"] in shared][:4] and len(g) == 4
    assert R.recommend_for_histories(model, hist, h, k=4, among=[[160], [100], []])[2] == []
    # the sampled protocol: reproducible from the seed; with far more draws than unseen items every unseen
    # item is a candidate (33 of them: a miss has probability 33 * (32 / 33) ** 2048 < 1e-25 per user) and
    # the numbers are the full ranking's
    train, held = h.edge_index, h.heldout
    a = ranking_eval.evaluate_sampled(model, train, held, gpu, negatives=20, ks=(5, 10), seed=3)
    assert a == ranking_eval.evaluate_sampled(model, train, held, gpu, negatives=20, ks=(5, 10), seed=3)
    assert a["users"] == 30 and 2 < a["candidates"] <= 20 + 2
    other = ranking_eval.evaluate_sampled(model, train, held, gpu, negatives=20, ks=(5, 10), seed=4)
    assert other["users"] == 30 and other != a
    big = ranking_eval.evaluate_sampled(model, train, held, gpu, negatives=2048, ks=(5, 10), seed=0)
    want = ranking_eval.evaluate_ranking(model, train, held, gpu, ks=(5, 10))
    assert big.pop("candidates") == 35.0  # every item the user has no training edge to
    assert big == want


def test_evaluate_ranking_hands_among_on(gpu):
    from lgcn_amd import metrics
    from lgcn_amd.recommend import topk_items

    rng = np.random.default_rng(29)
    U, M, d = 60, 500, 32
    t = lambda a: torch.from_numpy(a).to(gpu)
    Ut, It = t(_emb(rng, U, d)), t(_emb(rng, M, d))
    sets = [np.sort(rng.choice(M, int(n), replace=False)) for n in rng.integers(20, 200, U)]
    truth = [rng.choice(s, int(n), replace=False) if n else np.zeros(0, np.int64) for s, n in zip(sets, rng.integers(0, 6, U))]
    seen = [np.setdiff1d(rng.choice(M, 40, replace=False), tr) for tr in truth]
    among, tcsr, scsr = _csr(sets, gpu), _csr([np.sort(x) for x in truth], gpu), _csr(seen, gpu)
    got = metrics.evaluate_ranking(Ut, It, tcsr, ks=(5, 10), seen=scsr, among=among)
    users = torch.nonzero(tcsr[0][1:] > tcsr[0][:-1]).view(-1)
    ranked, _ = topk_items(Ut, It, users, 10, seen=scsr, among=among, index_dtype=torch.int32)
    want = metrics.summarize(metrics.rank_metrics(ranked, tcsr, (5, 10), rows=users), (5, 10))
    assert got == want and got["users"] == int(users.numel()) > 30
    assert got != metrics.evaluate_ranking(Ut, It, tcsr, ks=(5, 10), seen=scsr)
    # the re-ranked lists at diversity 0 are the same lists: same numbers, plus ild
    div = metrics.evaluate_ranking(Ut, It, tcsr, ks=(5, 10), seen=scsr, among=among, diversity=0.0, pool=32)
    assert {k: v for k, v in div.items() if not k.startswith("ild@")} == got
    assert got == metrics.evaluate_ranking(Ut, It, tcsr, ks=(5, 10), seen=scsr, among=(*among, users), users=users)
