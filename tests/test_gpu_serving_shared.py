"""One ragged CSR through all four serving stages on the GPU. topk_rows (exclusion), rank_metrics
(truth), explain_rows and fold_in_rows (history) read a query's CSR row through the same device
helper (csrc/lgcn_ragged.h) and the same argument check (lgcn_amd._serving), so one CSR and one
rows= list must mean the same thing to each of them: the same entries for a row inside the CSR,
nothing for an empty row and for a row outside it.

The smallest shapes that reach every path: 6 queries, 700 items, d = 24 (padded to the kernel width
32), k = 5, r = 3; rows = [0, 3, -1, 6, 1, 1] over a CSR of 6 rows names a short row, a row of 600
entries (above the 512 at which explain and fold-in hand a history to their eight-wave launches), a
row below and a row above the CSR, and an empty row twice, for two queries with the same embedding.
"""
import numpy as np
import pytest
import torch

from explain_checker import check_lists
from foldin_checker import foldin64
from rank_metrics_checker import counts64
from rerank_checker import unit_rows64

pytestmark = pytest.mark.gpu

Q, I, D_COLS, K, R = 6, 700, 24, 5, 3
ROWS = (0, 3, -1, 6, 1, 1)
PICKED = (0, 1, 2, 3, 4, 4)  # queries 4 and 5 are the same query
ROW_LENGTHS = (40, 0, 17, 600, 3, 64)
INSIDE, NOTHING = [0, 1], [2, 3, 4, 5]  # queries with a non-empty row / with an empty or outside row


def inputs(d=D_COLS, seed=20):
    """(queries f32 [5, d], items f32 [I, d], ptr int64 [7], idx int32): numpy, seeded; CSR rows
    ascending and distinct as recommend.seen_csr builds them."""
    rng = np.random.default_rng(seed)
    queries = rng.standard_normal((5, d)).astype(np.float32)
    items = rng.standard_normal((I, d)).astype(np.float32)
    rows = [np.sort(rng.choice(I, n, replace=False)) for n in ROW_LENGTHS]
    # row 0 holds query 0's three best items, so its exclusion changes the list
    best = np.argsort(-(unit_rows64(items) @ queries[0].astype(np.float64)))[:3]
    rows[0] = np.sort(np.concatenate([best, np.setdiff1d(rows[0], best)[:ROW_LENGTHS[0] - 3]]))
    ptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    return queries, items, ptr, np.concatenate(rows).astype(np.int32)


def test_one_csr_means_the_same_to_every_consumer(gpu):
    from lgcn_amd.explain import explain_rows
    from lgcn_amd.foldin import LONG, fold_in_rows
    from lgcn_amd.metrics import rank_metrics
    from lgcn_amd.recommend import topk_rows

    queries, items, ptr, idx = inputs()
    assert ROW_LENGTHS[3] > LONG and ROW_LENGTHS[1] == 0 and len(ROW_LENGTHS) == 6
    row_of = lambda q: idx[ptr[ROWS[q]]:ptr[ROWS[q] + 1]] if 0 <= ROWS[q] < 6 else idx[:0]
    length = np.array([row_of(q).size for q in range(Q)])
    assert length.tolist() == [40, 600, 0, 0, 0, 0]
    t = lambda a, **kw: torch.from_numpy(np.ascontiguousarray(a)).to(gpu, **kw)
    qs, cands, picked, rows = t(queries), t(items), torch.tensor(PICKED, device=gpu), torch.tensor(ROWS, device=gpu)
    csr = (t(ptr), t(idx), rows)
    same = lambda out: all(torch.equal(x[4], x[5]) for x in out)  # bitwise: NaN would fail it, none is expected

    # topk_rows: the exclusion rows
    got = topk_rows(qs, picked, cands, K, excl=csr)
    free = topk_rows(qs, picked, cands, K, excl=None)
    lists = got[0].cpu().numpy()
    assert lists.shape == (Q, K) and (lists >= 0).all() and (lists < I).all()
    for q in INSIDE:
        assert not np.isin(lists[q], row_of(q)).any(), q
        assert np.isin(free[0][q].cpu().numpy(), row_of(q)).any(), q  # the exclusion had something to do
    for q in NOTHING:
        assert torch.equal(got[0][q], free[0][q]) and torch.equal(got[1][q], free[1][q]), q
    assert same(got)

    # rank_metrics: the truth rows (against the lists nothing was excluded from, so that there are hits)
    ks = (1, 3, K)
    counts = rank_metrics(free[0], csr[:2], ks, rows=rows)
    hits, _, first, n_truth = counts64(free[0].cpu().numpy(), row_of, ks)
    assert counts.n_truth.tolist() == length.tolist() == n_truth.tolist()
    assert counts.hits.tolist() == hits.tolist() and counts.first.tolist() == first.tolist() and hits[:2].sum() > 0
    assert not counts.hits[NOTHING].any() and not counts.dcg[NOTHING].any()
    assert same(counts)

    # explain_rows: the history rows
    told = explain_rows(got[0], csr, cands, r=R)
    assert not told.n[NOTHING].any() and (told.total[NOTHING] == 0).all()
    assert (told.idx[NOTHING] == -1).all() and torch.isneginf(told.value[NOTHING]).all()
    inside = torch.tensor(INSIDE, device=gpu)
    check_lists(lists[INSIDE], ptr, idx, None, np.array(ROWS)[INSIDE], unit_rows64(items), R,
                *(x[inside].cpu().numpy() for x in told))
    assert (told.n[INSIDE] == R).all()
    assert same(told)

    # fold_in_rows: the history rows
    folded = fold_in_rows(csr, cands)
    assert folded.n.tolist() == length.tolist()
    assert not folded.rows[NOTHING].any()
    ref, n_ref, bound = foldin64(ptr, idx, None, np.array(ROWS), Q, items, None)
    assert n_ref.tolist() == length.tolist()
    err = np.abs(folded.rows.cpu().numpy().astype(np.float64) - ref)
    print("fold-in: worst error", float((err[INSIDE] / bound[INSIDE]).max()), "of the bar")
    assert (err <= bound).all()
    assert same(folded)
