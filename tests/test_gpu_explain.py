"""Explanations on the GPU (lgcn_explain_topr in csrc/lgcn_explain.hip, lgcn_amd.explain's
explain_rows / explain_items / history_weights, the explain keyword of
utils.recommend.recommend_for_users) against the float64 numpy restatement of explain_checker.py,
whose docstring states the checks and the bar.

Shapes are the smallest that cross every boundary of the kernel: slot sets of 16 (k = 1, 10, 16,
17, 40, 64), row widths below, at and above one 64-column block (D = 8, 64, 128, 256), history
lengths around the 16 entries a wave takes per round and far above them, all mixed in one call, and
lengths around the 512 entries above which eight waves share a history.
Random cases assert, from the float64 reference alone, that at most 1 % of the listed positions are
undecided, so the tolerance cannot hide a wrong ranking."""
import functools

import numpy as np
import pytest
import torch

from explain_checker import BAR, check_lists, explain64, history_row, ranked64, undecided64
from rerank_checker import unit_rows64

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 150, 300, 1500)


@functools.lru_cache(maxsize=None)
def _random_set(d, M):
    """Candidates and their float64 unit rows for width d (shared, never changed)."""
    cands = np.random.default_rng(9000 + d + M).standard_normal((M, d)).astype(np.float32)
    return cands, unit_rows64(cands)


def _csr(rows):
    ptr = np.cumsum([0] + [len(x) for x in rows]).astype(np.int64)
    return ptr, np.concatenate(list(rows) + [np.zeros(0, np.int64)]).astype(np.int32)


def _histories(rng, M, lengths=LENGTHS):
    return [np.sort(rng.choice(M, min(n, M), replace=False)) for n in lengths]


def _lists(rng, M, k, rows):
    """k distinct recommended items per history row; slot 0 is an item of the history where it has one."""
    rec = np.stack([rng.choice(M, k, replace=False) for _ in rows]).astype(np.int64)
    for q, items in enumerate(rows):
        if len(items) and items[0] not in rec[q]:
            rec[q, 0] = items[0]
    return rec


def _dev(gpu, *arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in arrays]


def _np(out):
    return [t.cpu().numpy() for t in out]


def _undecided(rec, ptr, idx, w, rows, C, r):
    """(undecided, listed) positions of the float64 reference alone."""
    und = listed = 0
    for q in range(rec.shape[0]):
        items, wq = history_row(ptr, idx, w, q if rows is None else int(rows[q]))
        for j in rec[q]:
            c = ranked64(items, wq, C, int(j))[1]
            n = min(r, c.size)
            und += int(undecided64(c, n).sum())
            listed += n
    return und, listed


@pytest.mark.parametrize("d,k,r,M,weighted", [
    (8, 1, 1, 300, False),
    (8, 10, 3, 2000, True),
    (8, 64, 8, 777, False),
    (64, 10, 3, 2000, False),
    (64, 16, 8, 2000, True),
    (64, 17, 1, 777, True),
    (64, 40, 3, 2000, True),
    (64, 64, 3, 2000, False),
    (100, 10, 8, 2000, True),
    (100, 17, 3, 300, False),
    (256, 1, 3, 2000, True),
    (256, 16, 1, 777, False),
    (256, 64, 8, 2000, False),
])
def test_grid_matches_checker(gpu, d, k, r, M, weighted):
    from lgcn_amd.explain import explain_rows

    cands, U = _random_set(d, M)
    rng = np.random.default_rng(1000 * d + 10 * k + r)
    rows = _histories(rng, M)
    ptr, idx = _csr(rows)
    w = (2.0 ** -rng.integers(0, 3, idx.size)).astype(np.float32) if weighted else None
    rec = _lists(rng, M, k, rows)
    und, listed = _undecided(rec, ptr, idx, w, None, U, r)
    print(f"d={d} k={k} r={r} M={M}: undecided {und}/{listed}")
    assert und <= 0.01 * listed
    trec, tptr, tidx, tw, tc = _dev(gpu, rec, ptr, idx, w, cands)
    out = explain_rows(trec, (tptr, tidx), tc, r=r, weights=tw)
    assert out.idx.dtype == torch.int64 and out.value.dtype == out.total.dtype == torch.float32
    assert out.n.dtype == torch.int32 and out.idx.shape == out.value.shape == (len(rows), k, r)
    dec, got_listed = check_lists(rec, ptr, idx, w, None, U, r, *_np(out))
    assert got_listed == listed and dec == listed - und


@pytest.mark.parametrize("d,k,r,weighted", [(64, 10, 3, True), (8, 17, 8, False), (256, 64, 8, False), (100, 40, 1, True)])
def test_histories_around_the_long_history_threshold(gpu, d, k, r, weighted):
    """Histories of more than 512 entries are shared by the eight waves of a workgroup, which serves
    eight consecutive queries: lengths at, just above and far above the threshold, several long ones
    within one group of eight and across two, short ones between them."""
    from lgcn_amd.explain import explain_rows

    M = 2000
    cands, U = _random_set(d, M)
    rng = np.random.default_rng(77 + d + k)
    rows = _histories(rng, M, (513, 2000, 512, 600, 5, 1500, 514, 0, 700, 511, 640, 1100))
    ptr, idx = _csr(rows)
    w = (2.0 ** -rng.integers(0, 3, idx.size)).astype(np.float32) if weighted else None
    rec = _lists(rng, M, k, rows)
    und, listed = _undecided(rec, ptr, idx, w, None, U, r)
    print(f"d={d} k={k} r={r}: undecided {und}/{listed}")
    assert und <= 0.01 * listed
    trec, tptr, tidx, tw, tc = _dev(gpu, rec, ptr, idx, w, cands)
    out = explain_rows(trec, (tptr, tidx), tc, r=r, weights=tw)
    dec, got_listed = check_lists(rec, ptr, idx, w, None, U, r, *_np(out))
    assert got_listed == listed and dec == listed - und


def _eighths(rng, n, d):
    """n rows of width d with entries in {-1, 0, 1} / 8: every dot of two is exact in f32 in any order."""
    return (rng.integers(-1, 2, (n, d)) / 8.0).astype(np.float32)


@pytest.mark.parametrize("d,k,weighted", [(16, 17, True), (64, 10, False), (64, 64, True)])
def test_exact_inputs_equal_the_rule_bit_for_bit(gpu, d, k, weighted):
    """Contributions are multiples of 2^-8 of magnitude at most 1 here, so every dot, product and sum
    is exact and equal contributions abound: idx, value, n and total must be the float64 rule's,
    including the ascending item order among ties."""
    from lgcn_amd.explain import explain_rows

    M, r = 1200, 8  # the longest history, 1200 entries, takes the eight-wave path
    rng = np.random.default_rng(d + k)
    cands = _eighths(rng, M, d)
    rows = _histories(rng, M)
    ptr, idx = _csr(rows)
    w = (2.0 ** -rng.integers(0, 3, idx.size)).astype(np.float32) if weighted else None
    rec = _lists(rng, M, k, rows)
    trec, tptr, tidx, tw, tc = _dev(gpu, rec.astype(np.int32), ptr, idx, w, cands)
    out = explain_rows(trec, (tptr, tidx), tc, r=r, weights=tw, normalized=True)
    assert out.idx.dtype == torch.int32
    gi, gv, gn, gt = _np(out)
    C = cands.astype(np.float64)
    ties = 0
    for q in range(len(rows)):
        items, wq = history_row(ptr, idx, w, q)
        for t in range(k):
            wi, wv, wn, wt = explain64(items, wq, C, int(rec[q, t]), r)
            np.testing.assert_array_equal(gi[q, t], wi)
            np.testing.assert_array_equal(gv[q, t], wv.astype(np.float32))
            assert gn[q, t] == wn and gt[q, t] == np.float32(wt) and float(np.float32(wt)) == wt
            ties += int((np.diff(wv[:wn]) == 0).sum())
    assert ties > 100


def test_an_item_is_never_a_reason_for_itself(gpu):
    """Recommended items taken from the history itself: none appears among its own reasons, and the
    result (total included) is the one of the history without that item."""
    from lgcn_amd.explain import explain_rows

    rng = np.random.default_rng(31)
    cands = _eighths(rng, 300, 32)
    items = np.sort(rng.choice(300, 40, replace=False))
    rec = items[[0, 7, 39, 16, 17]][None]
    tc, = _dev(gpu, cands)
    ptr, idx = _csr([items])
    got = explain_rows(*_dev(gpu, rec), _dev(gpu, ptr, idx), tc, r=8, normalized=True)
    assert got.n.tolist() == [[8] * 5]
    for t in range(5):
        assert rec[0, t] not in got.idx[0, t].tolist()
        p1, i1 = _csr([np.delete(items, np.flatnonzero(items == rec[0, t]))])
        want = explain_rows(*_dev(gpu, rec[:, t:t + 1]), _dev(gpu, p1, i1), tc, r=8, normalized=True)
        assert torch.equal(got.idx[:, t], want.idx[:, 0]) and torch.equal(got.value[:, t], want.value[:, 0])
        assert torch.equal(got.total[:, t], want.total[:, 0])
        total = sum(float(cands[i].astype(np.float64) @ cands[rec[0, t]]) for i in items if i != rec[0, t])
        assert float(got.total[0, t]) == total


def test_empty_slots(gpu):
    """-1, M and 2**31 - 1 in a list (and a value past int32 in an int64 list): n = 0, -1 / -inf and
    total 0 there, the other slots unchanged."""
    from lgcn_amd.explain import explain_rows

    cands, U = _random_set(64, 2000)
    rng = np.random.default_rng(33)
    rows = _histories(rng, 2000, (5, 40, 0, 700))
    ptr, idx = _csr(rows)
    rec = _lists(rng, 2000, 20, rows)
    tptr, tidx, tc = _dev(gpu, ptr, idx, cands)
    want = explain_rows(*_dev(gpu, rec), (tptr, tidx), tc, r=3)
    holes = [0, 6, 16, 19]
    for dtype, junk in ((np.int32, [-1, 2000, 2**31 - 1, -7]), (np.int64, [-1, 2000, 2**31 - 1, 2**40 + 5])):
        bad = rec.astype(dtype)
        bad[:, holes] = junk
        got = explain_rows(*_dev(gpu, bad), (tptr, tidx), tc, r=3)
        assert (got.n[:, holes] == 0).all() and (got.idx[:, holes] == -1).all() and (got.total[:, holes] == 0).all()
        assert torch.isneginf(got.value[:, holes]).all()
        keep = [t for t in range(20) if t not in holes]
        assert torch.equal(got.idx[:, keep].to(torch.int64), want.idx[:, keep])
        assert torch.equal(got.value[:, keep], want.value[:, keep]) and torch.equal(got.n[:, keep], want.n[:, keep])
        assert torch.equal(got.total[:, keep], want.total[:, keep])
        check_lists(bad, ptr, idx, None, None, U, 3, *_np(got))


def test_history_row_edge_cases(gpu):
    """hist_row naming rows out of order, one row for several queries, rows outside the CSR, and a
    history holding indices outside [0, M)."""
    from lgcn_amd.explain import explain_rows

    M = 500
    cands, U = _random_set(64, M)
    rng = np.random.default_rng(35)
    rows = _histories(rng, M, (30, 0, 200, 7))
    rows[3] = np.concatenate([[-9, -1], rows[3], [M, M + 7, 2**31 - 1]])  # ascending, five entries out of range
    ptr, idx = _csr(rows)
    which = np.array([2, 0, 0, 3, -1, 4, 1, 2, 3, 2**40], np.int64)
    rec = np.stack([rng.choice(M, 12, replace=False) for _ in which])
    rec[3, 0] = rows[3][2]
    trec, tptr, tidx, trows, tc = _dev(gpu, rec, ptr, idx, which, cands)
    got = explain_rows(trec, (tptr, tidx, trows), tc, r=8)
    check_lists(rec, ptr, idx, None, which, U, 8, *_np(got))
    assert (got.n[[4, 5, 6, 9]] == 0).all() and (got.total[[4, 5, 6, 9]] == 0).all()  # rows -1, 4, 1 and 2^40
    assert got.n[3, 0] == 6 and (got.n[[3, 8]] <= 7).all() and (got.n[[0, 1, 2, 7]] == 8).all()
    assert ((got.idx[[3, 8]] >= -1) & (got.idx[[3, 8]] < M)).all()
    again = explain_rows(trec[:1].expand(2, 12).contiguous(), (tptr, tidx, trows[[0, 7]]), tc, r=8)
    assert torch.equal(again.idx[0], again.idx[1]) and torch.equal(again.value[0], again.value[1])
    assert torch.equal(again.idx[0], got.idx[0]) and torch.equal(again.total[1], got.total[0])


def test_smaller_r_is_a_prefix(gpu):
    from lgcn_amd.explain import explain_rows

    cands, U = _random_set(64, 2000)
    rng = np.random.default_rng(37)
    rows = _histories(rng, 2000)
    ptr, idx = _csr(rows)
    w = (2.0 ** -rng.integers(0, 3, idx.size)).astype(np.float32)
    rec = _lists(rng, 2000, 17, rows)
    trec, tptr, tidx, tw, tc = _dev(gpu, rec, ptr, idx, w, cands)
    a = explain_rows(trec, (tptr, tidx), tc, r=2, weights=tw)
    b = explain_rows(trec, (tptr, tidx), tc, r=8, weights=tw)
    assert torch.equal(a.idx, b.idx[:, :, :2]) and torch.equal(a.value, b.value[:, :, :2])
    assert torch.equal(a.n, b.n.clamp(max=2)) and torch.equal(a.total, b.total)


def test_strided_int32_lists_equal_the_contiguous_int64_one(gpu):
    from lgcn_amd.explain import explain_rows

    cands, U = _random_set(64, 2000)
    rng = np.random.default_rng(39)
    rows = _histories(rng, 2000)
    ptr, idx = _csr(rows)
    rec = _lists(rng, 2000, 10, rows)
    trec, tptr, tidx, tc = _dev(gpu, rec, ptr, idx, cands)
    want = explain_rows(trec, (tptr, tidx), tc, r=3)
    wide = torch.full((len(rows), 37), 3, dtype=torch.int64, device=gpu)
    wide[:, 5:15] = trec
    for dtype in (torch.int32, torch.int64):
        view = wide.to(dtype)[:, 5:15]
        assert not view.is_contiguous() and view.stride(0) == 37
        got = explain_rows(view, (tptr, tidx), tc, r=3)
        assert got.idx.dtype == dtype and torch.equal(got.idx.to(torch.int64), want.idx)
        assert torch.equal(got.value, want.value) and torch.equal(got.n, want.n) and torch.equal(got.total, want.total)
    got = explain_rows(wide.t()[5:15].t(), (tptr, tidx), tc, r=3)
    assert torch.equal(got.idx, want.idx)


def test_no_queries_and_a_zero_row(gpu):
    from lgcn_amd.explain import explain_rows

    rng = np.random.default_rng(41)
    cands = rng.standard_normal((60, 16)).astype(np.float32)
    cands[17] = 0  # its unit row is NaN: every contribution it takes part in is NaN
    rows = [np.sort(rng.choice(60, 20, replace=False)) for _ in range(4)]
    rows[0] = np.union1d(rows[0], [17])
    rows[1] = np.setdiff1d(rows[1], [17])
    rows[2] = np.array([3, 17, 40])
    ptr, idx = _csr(rows)
    rec = np.stack([rng.choice(np.setdiff1d(np.arange(60), [3, 17, 40]), 6, replace=False) for _ in rows])
    rec[1, 2] = 17  # a NaN row as the recommended item: every reason is NaN, in item order
    tptr, tidx, tc = _dev(gpu, ptr, idx, cands)
    none = explain_rows(*_dev(gpu, rec[:0]), (tptr, tidx), tc, r=3)
    assert none.idx.shape == none.value.shape == (0, 6, 3) and none.n.shape == none.total.shape == (0, 6)
    assert none.idx.dtype == torch.int64
    r = 8
    got = explain_rows(*_dev(gpu, rec), (tptr, tidx), tc, r=r)
    check_lists(rec, ptr, idx, None, None, unit_rows64(cands), r, *_np(got))
    assert torch.isnan(got.total[0]).all() and not (got.idx[0] == 17).any()  # 21 entries, 8 listed: NaN is last
    assert (got.idx[2, :, 2] == 17).all() and torch.isnan(got.value[2, :, 2]).all() and (got.n[2] == 3).all()
    assert torch.isnan(got.value[1, 2]).all() and got.idx[1, 2].tolist() == rows[1][:r].tolist()


def test_a_history_without_entries(gpu):
    """A CSR with no entries at all (ptr all zeros, empty idx): everything empty, nothing faults."""
    from lgcn_amd.explain import explain_rows

    cands, U = _random_set(64, 2000)
    rec = torch.arange(50, device=gpu).view(5, 10)
    ptr = torch.zeros(6, dtype=torch.int64, device=gpu)
    idx = torch.zeros(0, dtype=torch.int32, device=gpu)
    for hist in ((ptr, idx), (ptr, idx, torch.tensor([4, 0, 9, -1, 2]))):
        for weights in (None, torch.zeros(0, device=gpu)):
            got = explain_rows(rec, hist, *_dev(gpu, cands), r=3, weights=weights)
            assert got.idx.shape == (5, 10, 3) and (got.idx == -1).all() and torch.isneginf(got.value).all()
            assert (got.n == 0).all() and (got.total == 0).all() and got.n.dtype == torch.int32
    torch.cuda.synchronize()


def test_first_layer_identity(gpu):
    """With history_weights, normalized=True and raw rows, total[q, t] is the first propagation
    layer's share of the user-item dot product: (sum_e w_e E_i) . E_j, for recommended items outside
    the history. Bar: a contribution is a cosine (within BAR) times the two rows' norms times a
    weight <= 1, so max(1, len) * BAR * (largest norm)^2."""
    from lgcn_amd.explain import explain_rows, history_weights
    from lgcn_amd.recommend import seen_csr

    U_, I_, d = 120, 500, 64
    rng = np.random.default_rng(43)
    E = rng.standard_normal((I_, d)).astype(np.float32)
    edges = np.unique(np.stack([rng.integers(0, U_, 4000), U_ + rng.integers(0, I_, 4000)]), axis=1)
    seen = seen_csr(torch.from_numpy(edges).to(gpu), U_, I_, by="user")
    w = history_weights(seen)
    assert w.is_cuda and w.shape == seen[1].shape
    ptr, idx, wn = seen[0].cpu().numpy(), seen[1].cpu().numpy(), w.cpu().numpy().astype(np.float64)
    users = rng.choice(U_, 40, replace=False)
    rec = np.stack([rng.choice(np.setdiff1d(np.arange(I_), idx[ptr[u]:ptr[u + 1]]), 10, replace=False) for u in users])
    got = explain_rows(*_dev(gpu, rec), (seen[0], seen[1], torch.from_numpy(users).to(gpu)),
                       *_dev(gpu, E), r=3, weights=w, normalized=True)
    E64 = E.astype(np.float64)
    top = float(np.linalg.norm(E64, axis=1).max()) ** 2
    total = got.total.cpu().numpy()
    for q, u in enumerate(users):
        b, e = ptr[u], ptr[u + 1]
        layer = (wn[b:e, None] * E64[idx[b:e]]).sum(0)
        ref = E64[rec[q]] @ layer
        assert (np.abs(total[q] - ref) <= max(1, e - b) * BAR * top).all(), (q, total[q], ref)


def test_explain_items_is_explain_rows_with_the_users_rows(gpu):
    from lgcn_amd.explain import explain_items, explain_rows

    cands, U = _random_set(64, 2000)
    rng = np.random.default_rng(45)
    rows = _histories(rng, 2000, (12, 0, 90, 33, 5))
    ptr, idx = _csr(rows)
    users = np.array([3, 3, 0, 4, 2, 1])
    rec = np.stack([rng.choice(2000, 10, replace=False) for _ in users])
    trec, tptr, tidx, tc = _dev(gpu, rec, ptr, idx, cands)
    w = torch.rand(idx.size, device=gpu)
    for weights in (None, w):
        got = explain_items(tc, users, trec, (tptr, tidx), r=3, weights=weights)
        want = explain_rows(trec, (tptr, tidx, torch.from_numpy(users)), tc, r=3, weights=weights)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
    check_lists(rec, ptr, idx, w.cpu().numpy(), users, U, 3, *_np(got))


def test_recommend_for_users_with_explanations(gpu, tmp_path):
    from data.dataset_handler import MovieLensDataHandler, write_synthetic_movielens
    from lgcn_amd.explain import explain_items
    from lgcn_amd.recommend import seen_csr, topk_rows, topk_rows_diverse
    from models.light_gcn import LightGCN
    from utils import recommend as R

    rp, mp = write_synthetic_movielens(str(tmp_path), 300, 200, 6000, seed=3)
    h = MovieLensDataHandler(rp, mp, device=gpu)
    U, I = h.get_num_users_items()
    torch.manual_seed(11)
    model = LightGCN(U, I, num_layers=2, dim_h=64).to(gpu)
    model.eval()
    title_of = dict(zip(h.movies["movieId"].tolist(), h.movies["title"].tolist()))
    user_ids = list(h.user_id_map)[:40]
    ids = user_ids[:30] + [-5] + user_ids[30:]
    uidx = torch.tensor([h.user_id_map[u] for u in user_ids], device=gpu)
    uw, iw = model.user_embedding.weight.detach(), model.item_embedding.weight.detach()
    seen = seen_csr(h.edge_index.to(gpu), U, I, by="user")
    ptr, sidx = seen[0].cpu().numpy(), seen[1].cpu().numpy()
    inv = {v: key for key, v in h.movie_id_map.items()}
    watched = {u: {inv[U + int(i)] for i in sidx[ptr[ui]:ptr[ui + 1]]} for u, ui in zip(user_ids, uidx.tolist())}

    def compare(served, idx):
        assert len(served) == 41 and served[30] == {"error": "Invalid user ID"}
        lists = served[:30] + served[31:]
        want = explain_items(iw, uidx, idx, seen, r=3)
        wi, wv, wn = want.idx.cpu().numpy(), want.value.cpu().numpy(), want.n.cpu().numpy()
        for q, (u, row) in enumerate(zip(user_ids, lists)):
            assert len(row) == 10 and [h.movie_id_map[x["movie_id"]] - U for x in row] == idx[q].tolist()
            for t, x in enumerate(row):
                assert set(x) == {"movie_id", "title", "score", "because"}
                assert len(x["because"]) == wn[q, t] <= 3
                for p, b in enumerate(x["because"]):
                    assert set(b) == {"movie_id", "title", "similarity"} and title_of[b["movie_id"]] == b["title"]
                    assert b["movie_id"] in watched[u] and b["movie_id"] != x["movie_id"]
                    assert h.movie_id_map[b["movie_id"]] - U == wi[q, t, p]
                    assert np.float32(b["similarity"]) == wv[q, t, p]
        return lists

    served = R.recommend_for_users(model, ids, h, k=10, explain=3)
    idx, score = topk_rows(uw, uidx, iw, 10, excl=(seen[0], seen[1], uidx))
    lists = compare(served, idx)
    assert sum(len(x["because"]) for row in lists for x in row) > 1000
    # seen movies stay in the list with exclude_seen=False, and are still explained from the history
    open_lists = compare(R.recommend_for_users(model, ids, h, k=10, explain=3, exclude_seen=False),
                         topk_rows(uw, uidx, iw, 10)[0])
    assert any(x["movie_id"] in watched[u] for u, row in zip(user_ids, open_lists) for x in row)
    # with diversity: the re-ranked list is the one explained
    diverse = topk_rows_diverse(uw, uidx, iw, 10, 0.5, excl=(seen[0], seen[1], uidx))
    compare(R.recommend_for_users(model, ids, h, k=10, diversity=0.5, explain=3), diverse.idx)
    # explain=None: today's dictionaries
    plain = R.recommend_for_users(model, ids, h, k=10)
    assert R.recommend_for_users(model, ids, h, k=10, explain=None) == plain
    assert all("because" not in x for row in plain if isinstance(row, list) for x in row)
    assert [[(x["movie_id"], x["title"], x["score"]) for x in row] for row in lists] == \
        [[(x["movie_id"], x["title"], x["score"]) for x in row] for row in plain[:30] + plain[31:]]
