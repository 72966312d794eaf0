"""Fold-in on the GPU (lgcn_foldin_rows in csrc/lgcn_foldin.hip, lgcn_amd.foldin's fold_in_rows /
fold_in / layer_tables, utils.recommend.recommend_for_histories, utils.ranking_eval.evaluate_fold_in)
against the float64 numpy restatement of foldin_checker.py, whose docstring derives the bar.

Shapes are the smallest that cross every boundary of the kernel: row widths of one lane (d = 1), of
a few lanes (8), of the flagship (64), of a width that is no power of two and leaves lanes idle
(100) and of the whole wave (256); tables of one row, of an odd count and of several hundred;
batches below, at and above the four histories of a workgroup and the eight of the long kernel's;
history lengths around the 64 lanes, around the long-history threshold and over every wave of the
eight."""
import functools

import numpy as np
import pytest
import torch

from foldin_checker import exact32, foldin64
from parity import assert_rows_close

pytestmark = pytest.mark.gpu


def _csr(rows):
    ptr = np.cumsum([0] + [len(x) for x in rows]).astype(np.int64)
    return ptr, np.concatenate(list(rows) + [np.zeros(0, np.int64)]).astype(np.int32)


def _dev(gpu, *arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in arrays]


def _raw(gpu, ptr, idx, w, rows, Q, table, d, isd, ldo, sentinel=-7.5):
    """lgcn_foldin_rows itself on device tensors: table is [M, ldt] with the rows in its first d
    columns, the output [Q, ldo] pre-filled with a sentinel. Returns (out [Q, ldo], n) as numpy."""
    from lgcn_amd import _ffi

    lib = _ffi.load()
    M, ldt = table.shape
    out = torch.full((Q, ldo), sentinel, dtype=torch.float32, device=gpu)
    n = torch.full((Q,), -1, dtype=torch.int32, device=gpu)
    tptr, tidx, tw, trows, ttab, tisd = _dev(gpu, ptr, idx, w, rows, table, isd)
    _ffi.check(lib.lgcn_foldin_rows(tptr.data_ptr(), tidx.data_ptr(), _ffi.ptr(tw), _ffi.ptr(trows), len(ptr) - 1, Q,
                                    ttab.data_ptr(), M, d, ldt, _ffi.ptr(tisd), out.data_ptr(), ldo, n.data_ptr(),
                                    _ffi.stream_of(gpu)), "lgcn_foldin_rows")
    torch.cuda.synchronize()
    return out.cpu().numpy(), n.cpu().numpy()


@pytest.mark.parametrize("Q", [1, 5, 70])
@pytest.mark.parametrize("M", [1, 37, 500])
@pytest.mark.parametrize("d", [1, 8, 64, 100, 256])
def test_grid_matches_checker(gpu, d, M, Q):
    """Random f32 values, histories of 0 to 256 entries with repeats and a few entries outside
    [0, M), twice per shape: with one choice of {hist_w, isd, hist_row, ldt > d, ldo > d} and with
    the opposite one, so every shape sees each option on and off."""
    case = [1, 8, 64, 100, 256].index(d) * 9 + [1, 37, 500].index(M) * 3 + [1, 5, 70].index(Q)
    rng = np.random.default_rng(5000 + case)
    R = Q + 3
    lengths = rng.integers(0, 257, R)
    lengths[rng.integers(0, R)] = 256
    lengths[rng.integers(0, R)] = 0
    hist = []
    for n in lengths:
        items = rng.integers(0, M, n)
        items[rng.random(n) < 0.03] = rng.choice([-1, M, M + 5, 2**31 - 1, -2**31])
        hist.append(items)
    ptr, idx = _csr(hist)
    w_all = rng.standard_normal(idx.size).astype(np.float32)
    isd_all = rng.uniform(0.05, 1.0, M).astype(np.float32)
    rows_all = rng.integers(-1, R + 1, Q).astype(np.int64)
    for flags in (case % 32, 31 - case % 32):
        w = w_all if flags & 1 else None
        isd = isd_all if flags & 2 else None
        rows = rows_all if flags & 4 else None
        ldt = d + (3 if flags & 8 else 0)  # an odd stride: the rows are then read with scalar loads
        ldo = d + (5 if flags & 16 else 0)
        table = rng.standard_normal((M, ldt)).astype(np.float32)
        ref, n_ref, bound = foldin64(ptr, idx, w, rows, Q, table[:, :d], isd)
        out, n = _raw(gpu, ptr, idx, w, rows, Q, table, d, isd, ldo)
        assert (n == n_ref).all(), (flags, n, n_ref)
        err = np.abs(out[:, :d].astype(np.float64) - ref)
        worst = float((err / np.where(bound > 0, bound, 1.0)).max())
        print(f"d={d} M={M} Q={Q} flags={flags:05b}: worst error {worst:.3f} of the bar")
        assert (err <= bound).all(), (flags, worst)
        assert (out[:, d:] == -7.5).all()
        assert (out[n_ref == 0, :d] == 0).all()


def _exact_inputs(rng, M, d, lengths):
    """Integers in [-8, 8], weights in {0.5, 1, 2}, isd in {0.25, 0.5, 1}: terms are multiples of 1/8 of
    magnitude at most 16, so every partial sum is exact in f32 in any order."""
    table = rng.integers(-8, 9, (M, d)).astype(np.float32)
    hist = [rng.integers(0, M, n) for n in lengths]  # with repeats: M = 300 rows, up to thousands of entries
    ptr, idx = _csr(hist)
    w = rng.choice([0.5, 1.0, 2.0], idx.size).astype(np.float32)
    isd = rng.choice([0.25, 0.5, 1.0], M).astype(np.float32)
    return table, ptr, idx, w, isd


@pytest.mark.parametrize("d", [8, 64, 100, 256])
def test_long_histories_bit_for_bit_on_exact_inputs(gpu, d):
    """Lengths around the 64 lanes of a wave, around the threshold T above which eight waves share a
    history, one past a chunk, and 8 T + 3 (every wave of the eight, the first one twice)."""
    from lgcn_amd import foldin

    T, chunk = foldin.LONG, foldin.CHUNK
    lengths = [0, 1, 63, 64, 65, T - 1, T, T + 1, chunk + 1, 8 * T + 3]
    table, ptr, idx, w, isd = _exact_inputs(np.random.default_rng(600 + d), 300, d, lengths)
    want, n_ref = exact32(ptr, idx, w, None, len(lengths), table, isd)
    assert n_ref.tolist() == lengths
    tptr, tidx, tw, ttab, tisd = _dev(gpu, ptr, idx, w, table, isd)
    got = foldin.fold_in_rows((tptr, tidx), ttab, isd=tisd, weights=tw)
    assert got.rows.dtype == torch.float32 and got.n.dtype == torch.int32 and got.rows.shape == (len(lengths), d)
    assert got.n.cpu().numpy().tolist() == lengths
    np.testing.assert_array_equal(got.rows.cpu().numpy(), want)
    # the same without the factors
    want, _ = exact32(ptr, idx, None, None, len(lengths), table, None)
    np.testing.assert_array_equal(foldin.fold_in_rows((tptr, tidx), ttab).rows.cpu().numpy(), want)


@pytest.mark.parametrize("d", [64, 100])
def test_bits_do_not_depend_on_the_batch_or_the_run(gpu, d):
    """A history of 8 T + 3 random-valued entries and one of 40: the same bits alone, at positions 0,
    3 and 69 of a batch of 70 (other long histories beside them), through hist_row, from a column
    slice of a wider table, and in two consecutive runs."""
    from lgcn_amd import foldin

    T = foldin.LONG
    rng = np.random.default_rng(700 + d)
    M = 500
    table = rng.standard_normal((M, d)).astype(np.float32)
    isd = rng.uniform(0.05, 1.0, M).astype(np.float32)
    ttab, tisd = _dev(gpu, table, isd)
    for n in (8 * T + 3, 40):
        mine = rng.integers(0, M, n)
        mine_w = rng.standard_normal(n).astype(np.float32)

        def run(hist, ws, rows=None, tab=ttab):
            ptr, idx = _csr(hist)
            tptr, tidx, tw, trows = _dev(gpu, ptr, idx, np.concatenate(ws).astype(np.float32), rows)
            out = foldin.fold_in_rows((tptr, tidx) if rows is None else (tptr, tidx, trows), tab, isd=tisd, weights=tw)
            return out.rows, out.n

        alone, n_alone = run([mine], [mine_w])
        assert n_alone.tolist() == [n] and torch.isfinite(alone).all() and (alone != 0).any()
        again, _ = run([mine], [mine_w])
        assert torch.equal(alone, again)
        for at in (0, 3, 69):
            lengths = rng.integers(0, 200, 70)
            lengths[[1, 5, 68]] = (T + 9, 3 * T, 2 * T + 1)
            hist = [rng.integers(0, M, m) for m in lengths]
            ws = [rng.standard_normal(m).astype(np.float32) for m in lengths]
            hist[at], ws[at] = mine, mine_w
            rows, ns = run(hist, ws)
            assert ns[at] == n and torch.equal(rows[at], alone[0]), at
            again, _ = run(hist, ws)
            assert torch.equal(rows, again)
        # through hist_row: the history is CSR row 2 of 4, named by queries 0 and 5 of 6
        hist = [rng.integers(0, M, 7), rng.integers(0, M, T + 1), mine, rng.integers(0, M, 90)]
        ws = [rng.standard_normal(len(h)).astype(np.float32) for h in hist]
        ws[2] = mine_w
        rows, ns = run(hist, ws, rows=np.array([2, 0, 3, 9, 1, 2], np.int64))
        assert ns.tolist() == [n, 7, 90, 0, T + 1, n]
        assert torch.equal(rows[0], alone[0]) and torch.equal(rows[5], alone[0])
        # a column slice of a wider table (16-byte aligned rows or not): read in place, the same bits
        for left, width in ((4, d + 12), (3, d + 5)):
            wide = torch.full((M, width), 9.0, device=gpu)
            wide[:, left:left + d] = ttab
            view = wide[:, left:left + d]
            assert not view.is_contiguous()
            sliced, _ = run([mine], [mine_w], tab=view)
            assert torch.equal(sliced, alone)


def test_edges(gpu):
    from lgcn_amd import foldin

    rng = np.random.default_rng(81)
    M, d = 60, 16
    table = rng.standard_normal((M, d)).astype(np.float32)
    ttab, = _dev(gpu, table)
    # a row outside the CSR, and a history whose entries are all out of range: zero rows, n = 0
    hist = [rng.integers(0, M, 9), np.array([-1, M, M + 3, 2**31 - 1]), rng.integers(0, M, 30)]
    ptr, idx = _csr(hist)
    tptr, tidx = _dev(gpu, ptr, idx)
    got = foldin.fold_in_rows((tptr, tidx, torch.tensor([0, 1, -1, 3, 2, 2**40])), ttab)
    assert got.n.tolist() == [9, 0, 0, 0, 30, 0]
    rows = got.rows.cpu().numpy()
    assert (rows[[1, 2, 3, 5]] == 0).all() and not np.signbit(rows[[1, 2, 3, 5]]).any()
    ref, _, bound = foldin64(ptr, idx, None, np.array([0, 1, -1, 3, 2, 2**40]), 6, table, None)
    assert (np.abs(rows - ref) <= bound).all()
    # an empty CSR, with and without rows, with and without (empty) weights
    zptr = torch.zeros(6, dtype=torch.int64, device=gpu)
    zidx = torch.zeros(0, dtype=torch.int32, device=gpu)
    for h in ((zptr, zidx), (zptr, zidx, torch.tensor([4, 0, 9, -1, 2]))):
        for weights in (None, torch.zeros(0, device=gpu)):
            got = foldin.fold_in_rows(h, ttab, weights=weights)
            assert got.rows.shape == (5, d) and (got.rows == 0).all() and (got.n == 0).all()
    # no queries: nothing is launched
    none = foldin.fold_in_rows((tptr, tidx, torch.zeros(0, dtype=torch.int64)), ttab)
    assert none.rows.shape == (0, d) and none.n.shape == (0,) and none.n.dtype == torch.int32
    one = foldin.fold_in_rows((torch.zeros(1, dtype=torch.int64), zidx), ttab)
    assert one.rows.shape == (0, d)
    # an empty table: every entry is out of range
    got = foldin.fold_in_rows((tptr, tidx), torch.zeros((0, d), device=gpu))
    assert (got.rows == 0).all() and (got.n == 0).all()
    # columns [d, ldo) keep their sentinel (the raw entry; fold_in_rows writes dense rows)
    for dd, ldo in ((16, 20), (16, 17), (13, 16)):
        out, n = _raw(gpu, ptr, idx, None, None, 3, table, dd, None, ldo, sentinel=123.0)
        assert (out[:, dd:] == 123.0).all() and n.tolist() == [9, 0, 30]
        ref, _, bound = foldin64(ptr, idx, None, None, 3, table[:, :dd], None)
        assert (np.abs(out[:, :dd] - ref) <= bound).all()
    # a NaN in one table row reaches only the histories that hold that row
    bad = table.copy()
    bad[17, 3] = np.nan
    hist = [np.array([1, 17, 5]), np.array([1, 5, 16, 18]), np.setdiff1d(np.arange(M), [17]), np.array([17] * 70)]
    ptr, idx = _csr(hist)
    got = foldin.fold_in_rows(tuple(_dev(gpu, ptr, idx)), *_dev(gpu, bad),
                              isd=torch.ones(M, device=gpu)).rows.cpu().numpy()
    assert np.isnan(got[[0, 3], 3]).all() and np.isfinite(np.delete(got, 3, axis=1)).all()
    assert np.isfinite(got[[1, 2]]).all()
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def _smoke_graph():
    """smoke()'s graph, K and d, with the float64 layers x(l) = A^l X from the dense 500 x 500
    normalised adjacency (shared, never changed)."""
    from lgcn_amd import synth

    g = synth.bipartite(300, 200, 3000, seed=1)
    U, I, K, d = g.num_users, g.num_items, 3, 64
    N = U + I
    A = np.zeros((N, N))
    A[g.edge_index[0], g.edge_index[1]] = 1.0
    A = np.maximum(A, A.T)
    deg = A.sum(1)
    dis = np.where(deg > 0, 1.0 / np.sqrt(np.maximum(deg, 1.0)), 0.0)
    A_hat = dis[:, None] * A * dis[None, :]
    X = (0.01 * np.random.default_rng(3).standard_normal((N, d))).astype(np.float32)
    layers = [X.astype(np.float64)]
    for _ in range(K):
        layers.append(A_hat @ layers[-1])
    return g, U, I, K, d, X, deg, layers


def test_identity_with_the_models_forward(gpu):
    """Folding every training node's own history in with new_edge=False against layer_tables' S is
    one propagation layer over the precombined table: c * sum_{l = 1..K} (A^l X)[node]; with c * X
    added it is the model's output row. Users from item histories against S_item, items from user
    lists against S_user; a node of degree 0 gives an exact zero row."""
    from lgcn_amd import foldin
    from lgcn_amd.recommend import seen_csr
    from models.light_gcn import LightGCN

    g, U, I, K, d, X, deg, layers = _smoke_graph()
    assert (deg[:U] == 0).any() or (deg[U:] == 0).any()  # the graph has isolated nodes
    c = 1.0 / (K + 1) ** 2
    upper = c * sum(layers[1:])
    model = LightGCN(U, I, num_layers=K, dim_h=d).to(gpu)
    with torch.no_grad():
        model.user_embedding.weight.copy_(torch.from_numpy(X[:U]))
        model.item_embedding.weight.copy_(torch.from_numpy(X[U:]))
        ei = torch.from_numpy(g.edge_index).to(gpu)
        out_u, out_i = model(ei)
        uw, iw = model.user_embedding.weight.detach(), model.item_embedding.weight.detach()
        S_user, S_item = foldin.layer_tables(uw, iw, model.plan_for(ei), K)
    assert S_user.shape == (U, d) and S_item.shape == (I, d)
    assert_rows_close(torch.cat([S_user, S_item]).cpu().numpy(), c * sum(layers[:K]), what="layer_tables")
    for by, S, lo, hi, model_rows in (("user", S_item, 0, U, out_u), ("item", S_user, U, U + I, out_i)):
        hist = seen_csr(ei, U, I, by=by)
        table_deg = torch.from_numpy(deg[U:] if by == "user" else deg[:U]).to(gpu)
        got = foldin.fold_in(hist, S, count=table_deg, new_edge=False)
        assert got.n.cpu().numpy().tolist() == deg[lo:hi].astype(np.int64).tolist()
        rows = got.rows.cpu().numpy()
        assert_rows_close(rows, upper[lo:hi], what=f"fold-in by {by}")
        assert (rows[deg[lo:hi] == 0] == 0).all()
        assert_rows_close(rows.astype(np.float64) + c * layers[0][lo:hi], model_rows.cpu().numpy().astype(np.float64),
                          what=f"fold-in by {by} + c x(0) against the model")
        assert_rows_close(model_rows.cpu().numpy(), c * sum(layers)[lo:hi], what="the model against float64")


def test_planted_clusters(gpu):
    """Two clusters of items (+- a unit direction plus 1 % noise): five items of cluster A folded in
    and ranked with the history excluded give ten items of cluster A, none of them from the history."""
    from lgcn_amd import foldin
    from lgcn_amd.recommend import topk_rows

    rng = np.random.default_rng(91)
    M, d = 200, 16
    axis = rng.standard_normal(d)
    axis /= np.linalg.norm(axis)
    side = np.where(np.arange(M) % 2 == 0, 1.0, -1.0)  # cluster A: the even items
    table = (side[:, None] * axis[None, :] + 0.01 * rng.standard_normal((M, d))).astype(np.float32)
    mine = np.sort(rng.choice(np.arange(0, M, 2), 5, replace=False))
    ptr, idx = _csr([mine])
    hist = tuple(_dev(gpu, ptr, idx))
    ttab, = _dev(gpu, table)
    count = torch.from_numpy(rng.integers(0, 50, M)).to(gpu)
    folded = foldin.fold_in(hist, ttab, count=count)
    assert folded.n.tolist() == [5]
    top, score = topk_rows(folded.rows, torch.arange(1), ttab, 10, excl=hist)
    top = top[0].tolist()
    assert len(set(top)) == 10 and all(i % 2 == 0 for i in top) and not set(top) & set(mine.tolist())
    assert (score > 0.99).all()


def test_harness(gpu, tmp_path):
    from data.dataset_handler import MovieLensDataHandler, write_synthetic_movielens
    from lgcn_amd import foldin, metrics
    from lgcn_amd.explain import explain_rows
    from lgcn_amd.recommend import seen_csr, topk_rows, topk_rows_diverse
    from models.light_gcn import LightGCN
    from utils import recommend as R
    from utils.ranking_eval import evaluate_fold_in

    rp, mp = write_synthetic_movielens(str(tmp_path), 300, 200, 6000, seed=3)
    h = MovieLensDataHandler(rp, mp, device=gpu)
    U, I = h.get_num_users_items()
    torch.manual_seed(11)
    model = LightGCN(U, I, num_layers=2, dim_h=64).to(gpu)
    model.eval()
    ei = h.edge_index.to(gpu)
    movie_ids = list(h.movie_id_map)
    unknown = [m for m in range(1, 40) if m not in h.movie_id_map][:3]
    assert len(unknown) == 3
    rng = np.random.default_rng(5)
    histories = [[int(m) for m in rng.choice(movie_ids, n, replace=False)] for n in (5, 1, 12, 30, 60)]
    histories[2] = unknown[:2] + histories[2] + [histories[2][0]]  # unknown ids, and one id named twice
    asked = histories[:3] + [unknown, []] + histories[3:]
    known = [0, 1, 2, 5, 6]
    index_of = lambda m: h.movie_id_map[m] - U
    rows = [sorted({index_of(m) for m in hist if m in h.movie_id_map}) for hist in histories]
    ptr, idx = _csr([np.array(r) for r in rows])
    hist_csr = tuple(_dev(gpu, ptr, idx))
    by_item = seen_csr(ei, U, I, by="item")
    degree = by_item[0][1:] - by_item[0][:-1]
    iw = model.item_embedding.weight.detach()
    q_raw = foldin.fold_in(hist_csr, iw, count=degree).rows

    def lists_of(served, idx_want, score_want, because=None):
        assert len(served) == 7 and served[3] == served[4] == {"error": "No known movie IDs"}
        for q, slot in enumerate(known):
            row = served[slot]
            assert len(row) == 10 and [index_of(x["movie_id"]) for x in row] == idx_want[q].tolist()
            assert [np.float32(x["score"]) for x in row] == score_want[q].tolist()
            for x in row:
                assert set(x) == {"movie_id", "title", "score"} | ({"because"} if because else set())
                assert x["title"] == f"Movie {x['movie_id']}"
        return [served[slot] for slot in known]

    # relevance lists: k entries per known history, none of them from the history
    want_idx, want_score = topk_rows(q_raw, torch.arange(5), iw, 10, excl=hist_csr)
    lists = lists_of(R.recommend_for_histories(model, asked, h, k=10), want_idx.cpu(), want_score.cpu())
    for hist, row in zip(histories, lists):
        assert not {x["movie_id"] for x in row} & set(hist)
    # exclude_history=False: the history's own movies may come back (a one-movie history's does)
    open_idx, open_score = topk_rows(q_raw, torch.arange(5), iw, 10)
    open_lists = lists_of(R.recommend_for_histories(model, asked, h, k=10, exclude_history=False), open_idx.cpu(),
                          open_score.cpu())
    assert open_lists[1][0]["movie_id"] == histories[1][0]
    # because: drawn only from the supplied history
    why = explain_rows(want_idx, hist_csr, iw, r=3)
    served = R.recommend_for_histories(model, asked, h, k=10, explain=3)
    explained = lists_of(served, want_idx.cpu(), want_score.cpu(), because=True)
    wi, wn = why.idx.cpu().numpy(), why.n.cpu().numpy()
    for q, (hist, row) in enumerate(zip(histories, explained)):
        for t, x in enumerate(row):
            assert len(x["because"]) == wn[q, t] == min(3, len(rows[q]))
            assert [index_of(b["movie_id"]) for b in x["because"]] == wi[q, t, :wn[q, t]].tolist()
            assert all(b["movie_id"] in hist and set(b) == {"movie_id", "title", "similarity"} for b in x["because"])
    # diversity: 0.0 gives the relevance list, 0.5 topk_rows_diverse's
    assert R.recommend_for_histories(model, asked, h, k=10, diversity=0.0) == \
        R.recommend_for_histories(model, asked, h, k=10)
    div = topk_rows_diverse(q_raw, torch.arange(5), iw, 10, 0.5, pool=40, excl=hist_csr)
    lists_of(R.recommend_for_histories(model, asked, h, k=10, diversity=0.5, pool=40), div.idx.cpu(), div.score.cpu())
    # weights: one per id, following its id through the dropped and repeated ones
    weights = [[float(w) for w in rng.uniform(0.5, 5.0, len(hist))] for hist in asked]
    w_of = [{index_of(m): w for m, w in reversed(list(zip(hist, ws))) if m in h.movie_id_map}
            for hist, ws in zip(asked, weights)]
    tw = torch.tensor([w_of[slot][i] for slot, r in zip(known, rows) for i in r], dtype=torch.float32, device=gpu)
    q_w = foldin.fold_in(hist_csr, iw, count=degree, weights=tw).rows
    assert not torch.equal(q_w, q_raw)
    w_idx, w_score = topk_rows(q_w, torch.arange(5), iw, 10, excl=hist_csr)
    lists_of(R.recommend_for_histories(model, asked, h, k=10, weights=weights), w_idx.cpu(), w_score.cpu())
    # propagated: folded against layer_tables' S_item, ranked against model(edge_index)'s items
    with torch.no_grad():
        items_p = model(ei)[1]
        S_item = foldin.layer_tables(model.user_embedding.weight, iw, model.plan_for(ei), 2)[1]
    q_p = foldin.fold_in(hist_csr, S_item, count=degree).rows
    p_idx, p_score = topk_rows(q_p, torch.arange(5), items_p, 10, excl=hist_csr)
    lists_of(R.recommend_for_histories(model, asked, h, k=10, embeddings="propagated"), p_idx.cpu(), p_score.cpu())
    # evaluate_fold_in: the manual composition, key for key
    held = [np.sort(rng.choice(np.setdiff1d(np.arange(I), r), 4, replace=False)) for r in rows]
    held[1] = held[1][:0]  # a user without held-out items is left out of the means
    truth = tuple(_dev(gpu, *_csr(held)))
    for mode, q, cands in (("raw", q_raw, iw), ("propagated", q_p, items_p)):
        want = metrics.evaluate_ranking(q, cands, truth, ks=(5, 20), seen=hist_csr)
        got = evaluate_fold_in(model, ei, hist_csr, truth, gpu, ks=(5, 20), embeddings=mode)
        assert got == want and got["users"] == 4 and set(got) >= {"recall@5", "ndcg@20", "mrr@20"}
    want = metrics.evaluate_ranking(q_raw, iw, truth, ks=(5,), seen=hist_csr, diversity=0.3, pool=40)
    got = evaluate_fold_in(model, ei, hist_csr, truth, gpu, ks=(5,), diversity=0.3, pool=40)
    assert got.keys() == want.keys() and all(got[k] == want[k] or (got[k] != got[k] and want[k] != want[k]) for k in got)
