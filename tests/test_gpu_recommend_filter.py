"""Attribute-filtered top-k on the GPU (lgcn_amd.recommend.topk_rows' attrs / where, utils.recommend's
genre arguments; lgcn_score_filter_attr and lgcn_select_topk_ranked_attr of csrc/lgcn_recall_attr.hip).

The oracle is the unfiltered path plus a numpy restatement of the predicate (_passes): the same
request written as exclusion rows — the query's own row joined with every candidate that fails for
it — through topk_rows without attrs, in dense mode. Keys come from the same MFMA chain in both, so
the comparison is torch.equal on the indices and on the scores' bits; there is no tolerance."""
import numpy as np
import pandas as pd
import pytest
import torch

pytestmark = pytest.mark.gpu


def _emb(rng, n, d):
    return rng.standard_normal((n, d)).astype(np.float32)


def _u32(x):
    return np.asarray(x, dtype=np.int64).astype(np.uint32)  # python ints in [0, 2**32) as the bit pattern


def _passes(attr, any_, all_, none):
    """bool [Q, M]: the predicate of include/lgcn.h, restated. attr [M], the masks [Q], all uint32."""
    a = _u32(attr)[None, :]
    any_, all_, none = (_u32(m)[:, None] for m in (any_, all_, none))
    return ((a & none) == 0) & ((a & all_) == all_) & ((any_ == 0) | ((a & any_) != 0))


def _i32(x):
    return torch.from_numpy(_u32(x).view(np.int32).copy())


def _union_csr(rows, passes, dev):
    """The exclusion CSR of the oracle: row q = rows[q] joined with every candidate failing for q."""
    drop = ~passes
    for q, r in enumerate(rows):
        drop[q, np.asarray(r, np.int64)] = True
    ptr = np.concatenate([[0], np.cumsum(drop.sum(1))]).astype(np.int64)
    idx = np.nonzero(drop)[1].astype(np.int32)
    return torch.from_numpy(ptr).to(dev), torch.from_numpy(idx).to(dev)


def _csr(rows, dev):
    ptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    idx = np.concatenate([np.asarray(r, np.int32) for r in rows] + [np.zeros(0, np.int32)])
    return torch.from_numpy(ptr).to(dev), torch.from_numpy(idx).to(dev)


def _same(a, b):
    """Indices equal and scores equal to the bit (NaN included)."""
    return torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def _check_lists(idx, score, passes, rows, k):
    """Every returned index passes and is not excluded; the unfilled tail is -1 / -inf and as long as
    the restated predicate says."""
    idx, score = idx.cpu().numpy(), score.cpu().numpy()
    for q in range(idx.shape[0]):
        ok = passes[q].copy()
        ok[np.asarray(rows[q], np.int64)] = False
        n = min(k, int(ok.sum()))
        assert (idx[q, :n] >= 0).all() and ok[idx[q, :n]].all(), q
        assert (idx[q, n:] == -1).all() and np.isneginf(score[q, n:]).all(), q


# (any, all, none) by name; bit 20 is set on no item
PALETTE = [("none", (0, 0, 0)), ("any", (1 << 0 | 1 << 3, 0, 0)), ("all", (0, 1 << 0 | 1 << 1, 0)),
           ("without", (0, 0, 1 << 0)), ("all three", (1 << 1 | 1 << 2, 1 << 0, 1 << 6)),
           ("nothing passes", (0, 1 << 20, 0)), ("bit 31", (1 << 31, 0, 0))]


def _grid_attrs(rng, M):
    """12 attribute bits, bit b set with probability 2^-(b mod 6 + 1), plus the sign bit on a quarter
    of the items; about 3 % of the items carry no bit at all."""
    attr = np.zeros(M, np.uint32)
    for b in range(12):
        attr |= (rng.random(M) < 2.0 ** -(b % 6 + 1)).astype(np.uint32) << np.uint32(b)
    attr |= (rng.random(M) < 0.25).astype(np.uint32) << np.uint32(31)
    attr[rng.random(M) < 0.03] = 0
    return attr


@pytest.mark.parametrize("d", [8, 64, 100, 256])
@pytest.mark.parametrize("k", [1, 10, 100])
def test_dense_grid_equals_the_exclusion_row_oracle(gpu, d, k):
    from lgcn_amd.recommend import topk_rows

    rng = np.random.default_rng(d * 1000 + k)
    users, cands = _emb(rng, 900, d), _emb(rng, 2000, d)
    picked = rng.choice(900, 300, replace=False)
    rows = [np.sort(rng.choice(2000, rng.integers(0, 51), replace=False)) for _ in range(300)]
    attr = _grid_attrs(rng, 2000)
    assert (attr == 0).sum() >= 60  # the 3 % set to zero, and the rows that drew no bit
    which = rng.integers(0, len(PALETTE), 300)
    masks = [[PALETTE[w][1][c] for w in which] for c in range(3)]  # python ints, bit 31 as 2**31
    passes = _passes(attr, *masks)
    t = lambda a: torch.from_numpy(a).to(gpu)
    got = topk_rows(t(users), torch.from_numpy(picked), t(cands), k, excl=_csr(rows, gpu), attrs=_i32(attr).to(gpu),
                    where=tuple(masks))
    want = topk_rows(t(users), torch.from_numpy(picked), t(cands), k, excl=_union_csr(rows, passes, gpu))
    assert _same(got, want)
    _check_lists(*got, passes, rows, k)
    gi, gs = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert (which == 5).any() and (gi[which == 5] == -1).all() and np.isneginf(gs[which == 5]).all()
    for w in range(len(PALETTE)):  # every filter of the palette was drawn, and the others leave something to rank
        assert (which == w).any()
        if w != 5:
            assert (gi[which == w, 0] >= 0).all(), PALETTE[w][0]


def _count(monkeypatch):
    """The labels lgcn_amd.recommend hands _ffi.check, in call order."""
    from lgcn_amd import _ffi

    calls, check = [], _ffi.check

    def counting(rc, what):
        calls.append(what)
        return check(rc, what)

    monkeypatch.setattr(_ffi, "check", counting)
    return calls


def _list_case(seed=21):
    rng = np.random.default_rng(seed)
    users, cands = _emb(rng, 400, 64), _emb(rng, 20000, 64)
    picked = rng.choice(400, 256, replace=False)
    return rng, users, cands, picked


LIST_KW = dict(cap=4096, subset=2048)  # the smallest setting that leaves the dense path at M = 20,000


def test_list_path_keeps_only_passing_candidates(gpu, monkeypatch):
    """Filters passing about 50 %, 5 %, 0.5 % (100 items), exactly 6 items and nothing, mixed in one
    query block. One lgcn_score_filter_attr pass serves the block: a list holds about k * stride = 100
    passing entries, or the at most 100 that pass at all, against 4,096 slots — which a filter applied
    only in the ranked kernel cannot do at 0.5 %, where "accept everything" is 20,000 entries."""
    from lgcn_amd.recommend import topk_rows

    rng, users, cands, picked = _list_case()
    M, k = 20000, 10
    attr = np.zeros(M, np.uint32)
    attr |= (rng.random(M) < 0.5).astype(np.uint32) << np.uint32(0)
    attr |= (rng.random(M) < 0.05).astype(np.uint32) << np.uint32(1)
    attr[rng.choice(M, 100, replace=False)] |= np.uint32(1 << 2)
    six = rng.choice(M, 6, replace=False)
    attr[six] |= np.uint32(1 << 3)
    free = np.setdiff1d(np.arange(M), six)  # exclusion rows leave the six alone: 6 filled, 4 padded
    rows = [np.sort(rng.choice(free, rng.integers(0, 51), replace=False)) for _ in range(256)]
    which = np.arange(256) % 5
    any_ = [1 << int(w) for w in which]  # bit 4 is set on no item
    passes = _passes(attr, any_, [0] * 256, [0] * 256)
    assert [int(passes[q].sum()) for q in range(2, 5)] == [100, 6, 0]
    t = lambda a: torch.from_numpy(a).to(gpu)
    want = topk_rows(t(users), torch.from_numpy(picked), t(cands), k, excl=_union_csr(rows, passes, gpu), cap=32768)
    calls = _count(monkeypatch)
    got = topk_rows(t(users), torch.from_numpy(picked), t(cands), k, excl=_csr(rows, gpu), attrs=_i32(attr).to(gpu),
                    where=(any_, None, None), **LIST_KW)
    assert calls.count("lgcn_score_filter_attr") == 1 and "lgcn_score_filter" not in calls, calls
    assert "lgcn_select_topk_ranked" not in calls and calls.count("lgcn_select_topk_ranked_attr") == 2, calls
    assert _same(got, want)
    _check_lists(*got, passes, rows, k)
    idx = got[0].cpu().numpy()
    assert ((idx[which == 3] >= 0).sum(1) == 6).all() and (idx[which == 4] == -1).all()
    assert ((idx[which <= 2] >= 0).sum(1) == k).all()


def test_threshold_is_formed_after_the_filter(gpu):
    """Item j carries bit j mod 16 and query q refuses the bits of its own three best items: a
    threshold formed before the filter would sit among candidates the query cannot be served."""
    from lgcn_amd.recommend import topk_rows

    rng, users, cands, picked = _list_case(22)
    M, k = 20000, 10
    attr = (np.uint32(1) << (np.arange(M) % 16).astype(np.uint32)).astype(np.uint32)
    rows = [np.sort(rng.choice(M, rng.integers(0, 51), replace=False)) for _ in range(256)]
    t = lambda a: torch.from_numpy(a).to(gpu)
    best, _ = topk_rows(t(users), torch.from_numpy(picked), t(cands), 3, excl=_csr(rows, gpu), cap=32768)
    none = [int(np.bitwise_or.reduce(attr[b])) for b in best.cpu().numpy()]
    passes = _passes(attr, [0] * 256, [0] * 256, none)
    got = topk_rows(t(users), torch.from_numpy(picked), t(cands), k, excl=_csr(rows, gpu), attrs=_i32(attr).to(gpu),
                    where=(0, 0, none), **LIST_KW)
    want = topk_rows(t(users), torch.from_numpy(picked), t(cands), k, excl=_union_csr(rows, passes, gpu), cap=32768)
    assert _same(got, want)
    assert not (got[0][:, :, None] == best[:, None, :]).any()  # no query is served one of its refused three
    _check_lists(*got, passes, rows, k)


@pytest.mark.parametrize("cap", [None, 512], ids=["dense", "filtered"])
def test_strided_attrs_mask_forms_and_query_blocks(gpu, monkeypatch, cap):
    from lgcn_amd import recommend as RC

    rng = np.random.default_rng(33)
    users, cands = _emb(rng, 700, 32), _emb(rng, 2000, 32)
    picked = torch.from_numpy(rng.choice(700, 300, replace=False))
    rows = [np.sort(rng.choice(2000, rng.integers(0, 51), replace=False)) for _ in range(300)]
    attr = _grid_attrs(rng, 2000)
    t = lambda a: torch.from_numpy(a).to(gpu)
    U, C, excl = t(users), t(cands), _csr(rows, gpu)
    kw = {} if cap is None else dict(cap=cap, subset=cap)
    attrs = _i32(attr).to(gpu)
    wide = torch.stack([torch.full_like(attrs, -1), attrs, torch.zeros_like(attrs)], 1)
    assert not wide[:, 1].is_contiguous()
    # one filter for all: ints, tensors, sequences and None members say the same
    one = RC.topk_rows(U, picked, C, 10, excl=excl, attrs=attrs, where=(1 << 31 | 1, 0, 2), **kw)
    forms = [(torch.full((300,), -2 ** 31 + 1, dtype=torch.int32, device=gpu), None, [2] * 300),
             (torch.full((300,), 2 ** 31 + 1, dtype=torch.int64), torch.zeros(300, dtype=torch.int64, device=gpu), 2),
             (-2 ** 31 + 1, None, torch.full((300,), 2, dtype=torch.uint8))]
    offset = torch.cat([torch.full((5,), -1, dtype=torch.int32, device=gpu), attrs])[5:]  # contiguous, not at the base
    assert offset.storage_offset() == 5
    for where, view in zip(forms, (wide[:, 1], offset, wide[:, 1])):
        assert _same(RC.topk_rows(U, picked, C, 10, excl=excl, attrs=view, where=where, **kw), one)
    passes = _passes(attr, [2 ** 31 + 1] * 300, [0] * 300, [2] * 300)
    want = RC.topk_rows(U, picked, C, 10, excl=_union_csr(rows, passes, gpu))
    assert _same(one, want)
    # per-query masks that differ across the block boundaries: three blocks equal one block
    which = np.arange(300) % len(PALETTE)
    masks = tuple([PALETTE[w][1][c] for w in which] for c in range(3))
    passes = _passes(attr, *masks)
    one = RC.topk_rows(U, picked, C, 10, excl=excl, attrs=attrs, where=masks, **kw)
    assert _same(one, RC.topk_rows(U, picked, C, 10, excl=_union_csr(rows, passes, gpu)))
    monkeypatch.setattr(RC, "BLOCK_BYTES", 8 * (cap or 2000) * 128)  # 128 queries per block: three blocks
    calls = _count(monkeypatch)
    three = RC.topk_rows(U, picked, C, 10, excl=excl, attrs=wide[:, 1], where=masks, **kw)
    assert calls.count("lgcn_select_topk_ranked_attr") >= 3
    assert _same(one, three)


def _serving_case(gpu):
    rng = np.random.default_rng(41)
    users, items = _emb(rng, 500, 64), _emb(rng, 1500, 64)
    attr = _grid_attrs(rng, 1500)
    by_user = [np.sort(rng.choice(1500, rng.integers(0, 41), replace=False)) for _ in range(500)]
    t = lambda a: torch.from_numpy(a).to(gpu)
    return rng, t(users), t(items), attr, by_user


WHERE = (1 << 0 | 1 << 2, 0, 1 << 1)  # one filter for every query of the pass-through cases


def test_entry_points_hand_the_filter_on(gpu):
    from lgcn_amd import metrics, recommend as RC

    rng, U, I, attr, by_user = _serving_case(gpu)
    attrs = _i32(attr).to(gpu)
    seen = _csr(by_user, gpu)
    who = torch.from_numpy(rng.choice(500, 200, replace=False))
    rows = [by_user[u] for u in who.tolist()]
    passes = _passes(attr, *([m] * 200 for m in WHERE))
    union = _union_csr(rows, passes, gpu)
    # topk_items
    got = RC.topk_items(U, I, who, 10, seen=seen, attrs=attrs, where=WHERE)
    assert _same(got, RC.topk_rows(U, who, I, 10, excl=union))
    _check_lists(*got, passes, rows, 10)
    # topk_rows_diverse: the pool holds passing items only, so the re-ranked lists agree field by field
    got = RC.topk_rows_diverse(U, who, I, 10, 0.5, pool=64, excl=(seen[0], seen[1], who), attrs=attrs, where=WHERE)
    want = RC.topk_rows_diverse(U, who, I, 10, 0.5, pool=64, excl=union)
    assert torch.equal(got.idx, want.idx) and torch.equal(got.n, want.n)
    assert torch.equal(got.score.view(torch.int32), want.score.view(torch.int32))
    assert torch.equal(got.pair.view(torch.int32), want.pair.view(torch.int32))
    assert (got.n == 10).all()
    # topk_users: the users are the candidates and carry the attribute words
    uattr = _grid_attrs(rng, 500)
    by_item = [np.sort(rng.choice(500, rng.integers(0, 31), replace=False)) for _ in range(1500)]
    items = torch.from_numpy(rng.choice(1500, 150, replace=False))
    irows = [by_item[i] for i in items.tolist()]
    upasses = _passes(uattr, *([m] * 150 for m in WHERE))
    got = RC.topk_users(U, I, items, 10, seen=_csr(by_item, gpu), attrs=_i32(uattr).to(gpu), where=WHERE)
    assert _same(got, RC.topk_rows(I, items, U, 10, excl=_union_csr(irows, upasses, gpu)))
    _check_lists(*got, upasses, irows, 10)
    # evaluate_ranking: the metrics of the filtered lists, against the training CSR rewritten for every user
    truth = _csr([np.sort(rng.choice(1500, rng.integers(1, 8), replace=False)) for _ in range(500)], gpu)
    all_pass = _passes(attr, *([m] * 500 for m in WHERE))
    got = metrics.evaluate_ranking(U, I, truth, ks=(5, 10), seen=seen, attrs=attrs, where=WHERE)
    want = metrics.evaluate_ranking(U, I, truth, ks=(5, 10), seen=_union_csr(by_user, all_pass, gpu))
    plain = metrics.evaluate_ranking(U, I, truth, ks=(5, 10), seen=seen)
    assert got.keys() == want.keys()
    for key in got:
        assert got[key] == want[key] or (got[key] != got[key] and want[key] != want[key]), key
    assert got != plain


class _Handler:
    """40 movies (ids 100, 103, ...), 4 genres, some movies with two, one with the placeholder, one
    without a row in movies (unless ``complete``: the served dictionaries look every title up, so the
    unfiltered lists come from the complete table); 30 users with a handful of edges each (global
    numbering, both directions)."""

    def __init__(self, complete=False):
        rng = np.random.default_rng(51)
        genres = ["Comedy", "Horror", "Drama", "Romance"]
        ids = [100 + 3 * i for i in range(40)]
        self.user_id_map = {1000 + u: u for u in range(30)}
        self.movie_id_map = {m: 30 + i for i, m in enumerate(ids)}
        self.genres_of = {}
        for i, m in enumerate(ids):
            g = [genres[i % 4]] + ([genres[(i // 4) % 4]] if i % 3 == 0 and (i // 4) % 4 != i % 4 else [])
            self.genres_of[m] = g
        self.genres_of[ids[7]] = []   # "(no genres listed)"
        self.genres_of[ids[12]] = []  # no row in movies
        listed = [m for m in ids if complete or m != ids[12]]
        self.movies = pd.DataFrame({"movieId": listed, "title": [f"Movie {m}" for m in listed],
                                    "genres": ["|".join(self.genres_of[m]) or "(no genres listed)" for m in listed]})
        u = np.repeat(np.arange(30), 5)
        # nobody has an edge to the movie without a row: 'because' looks the titles of a history up
        i = np.concatenate([rng.choice(np.setdiff1d(np.arange(40), [12]), 5, replace=False) for _ in range(30)]) + 30
        self.edge_index = torch.from_numpy(np.stack([np.concatenate([u, i]), np.concatenate([i, u])])).long()

    def keeps(self, movie_id):
        g = self.genres_of[movie_id]
        return "Comedy" in g and "Horror" not in g


def test_harness_serves_the_genre_filter(gpu):
    from models.light_gcn import LightGCN
    from utils import recommend as R

    h, whole = _Handler(), _Handler(complete=True)
    assert len(h.movies) == 39 and len(whole.movies) == 40 and torch.equal(h.edge_index, whole.edge_index)
    assert sum(len(g) == 2 for g in h.genres_of.values()) >= 5 and sum(h.keeps(m) for m in h.genres_of) >= 8
    torch.manual_seed(5)
    model = LightGCN(30, 40, num_layers=2, dim_h=32).to(gpu)
    model.eval()
    vocab, attrs = R.genre_table(h)
    assert vocab == ["Comedy", "Drama", "Horror", "Romance"] and attrs[7] == 0 and attrs[12] == 0
    ids = list(h.user_id_map)[:20] + [-1]
    flt = dict(genres=["Comedy"], without_genres=["Horror"])
    for kw in ({}, dict(explain=2)):
        full = R.recommend_for_users(model, ids, whole, k=40, **kw)
        got = R.recommend_for_users(model, ids, h, k=10, **kw, **flt)
        assert got[-1] == full[-1] == {"error": "Invalid user ID"}
        for g, f in zip(got[:-1], full[:-1]):
            assert g == [x for x in f if h.keeps(x["movie_id"])][:10] and 1 <= len(g) <= 10
            assert ("because" in g[0]) == bool(kw)
    full = R.recommend_for_users(model, ids, whole, k=40)
    got = R.recommend_for_users(model, ids, h, k=10, diversity=0.0, **flt)
    for g, f in zip(got[:-1], full[:-1]):
        assert g == [x for x in f if h.keeps(x["movie_id"])][:10]
    hist = [[100, 103, 130], [999], [118, 121, 124, 160, 163]]
    for kw in ({}, dict(explain=2), dict(diversity=0.0)):
        base = {k: v for k, v in kw.items() if k != "diversity"}
        full = R.recommend_for_histories(model, hist, whole, k=40, **base)
        got = R.recommend_for_histories(model, hist, h, k=10, **kw, **flt)
        assert got[1] == full[1] == {"error": "No known movie IDs"}
        for g, f in zip((got[0], got[2]), (full[0], full[2])):
            assert g == [x for x in f if h.keeps(x["movie_id"])][:10] and len(g) >= 1
