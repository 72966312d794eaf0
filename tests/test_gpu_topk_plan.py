"""topk_rows' host plan on the GPU: which library calls each of its three block strategies issues, in
which order, and that the lists are right (lgcn_amd.recommend's _Plan, _run_dense, _run_filtered,
_run_among).

Every case runs 130 queries (two 128-query tiles, 126 padding queries) of width 24 (padded to 32)
against 300 candidates for k = 5, with the exclusion given as (ptr, idx), as (ptr, idx, rows) with
some rows outside the CSR, and not at all. The labels lgcn_amd._ffi.check sees are compared with
literal sequences; the lists go through test_gpu_recommend's float64 checker under its rule for
near-ties, a filter or a candidate set restated as exclusion rows. Every tenth candidate leans
towards the queries' common direction, so the strided subset (stride 10 at subset=32) holds each
query's best candidates and no list of the filtered path overflows its 64 slots."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_recommend import _check, _csr, _scores64

pytestmark = pytest.mark.gpu

Q, M, D_, K = 130, 300, 24, 5
EXCL_FORMS = ["ptr_idx", "ptr_idx_rows", "none"]
NONE_BIT = 1 << 2  # where=(0, 0, NONE_BIT): a quarter of the candidates carry the bit and fail
NORMALIZE = ["lgcn_normalize_rows"] * 2


@functools.lru_cache(maxsize=1)
def _case():
    rng = np.random.default_rng(20)
    common = rng.standard_normal(D_)
    users = (1.5 * common + rng.standard_normal((Q, D_))).astype(np.float32)
    cands = rng.standard_normal((M, D_))
    cands[::10] += 3.0 * common
    cands = cands.astype(np.float32)
    S = _scores64(users, cands)
    by_query = [np.sort(rng.choice(M, n, replace=False)).astype(np.int32) for n in rng.integers(0, 21, Q)]
    by_row = [np.sort(rng.choice(M, n, replace=False)).astype(np.int32) for n in rng.integers(0, 21, 100)]
    names = rng.integers(-1, 101, Q).astype(np.int64)  # -1 and 100 are outside the CSR of 100 rows
    names[:4] = [-1, 100, 7, 7]
    attr = (rng.random(M) < 0.25).astype(np.int32) * NONE_BIT | (rng.random(M) < 0.5).astype(np.int32)
    fails = np.nonzero(attr & NONE_BIT)[0]
    # candidate sets of 0, 1, 5, 40 and 300 entries: distinct candidates, entries that name nothing,
    # and in the two longest the row's poorest candidate named again (ranked twice, far below k)
    sets, among = [], []
    for q in range(Q):
        n = (0, 1, 5, 40, 300)[q % 5]
        junk = {0: 0, 1: 0, 5: 1, 40: 2, 300: 10}[n]
        twice = {40: 2, 300: 10}.get(n, 0)
        keep = rng.choice(M, n - junk - twice, replace=False)
        poorest = keep[np.argmin(S[q, keep])] if twice else 0
        row = np.concatenate([keep, rng.choice(np.array([-1, M, M + 7, -9]), junk), np.full(twice, poorest)]).astype(np.int32)
        among.append(rng.permutation(row))
        sets.append(np.unique(keep))
    return dict(users=users, cands=cands, S=S, by_query=by_query, by_row=by_row, names=names, attr=attr, fails=fails,
                sets=sets, among=among)


def _excl(form, gpu):
    """(topk_rows' excl, the checker's row per query)."""
    c = _case()
    if form == "none":
        return None, [np.zeros(0, np.int32)] * Q
    if form == "ptr_idx":
        return _csr(c["by_query"], gpu), c["by_query"]
    rows = [c["by_row"][r] if 0 <= r < 100 else np.zeros(0, np.int32) for r in c["names"]]
    return (*_csr(c["by_row"], gpu), torch.from_numpy(c["names"])), rows


def _spy(monkeypatch):
    """Every label lgcn_amd._ffi.check is handed, in call order."""
    from lgcn_amd import _ffi

    seen, check = [], _ffi.check

    def recording(rc, what):
        seen.append(what)
        return check(rc, what)

    monkeypatch.setattr(_ffi, "check", recording)
    return seen


def _run(gpu, monkeypatch, form, filtered=False, among=False, block_bytes=None, **kw):
    """The labels of one int64 call, its lists checked; an int32 call must repeat the calls and the values."""
    from lgcn_amd import recommend

    c = _case()
    excl, rows = _excl(form, gpu)
    if filtered:
        kw.update(attrs=torch.from_numpy(c["attr"]).to(gpu), where=(0, 0, NONE_BIT))
        rows = [np.union1d(r, c["fails"]) for r in rows]
    if among:
        kw.update(among=_csr(c["among"], gpu))
        rows = [np.union1d(r, np.setdiff1d(np.arange(M), s)) for r, s in zip(rows, c["sets"])]
        for q in range(Q):  # a candidate named twice stays below the list: more than k others are eligible
            assert q % 5 < 3 or M - len(rows[q]) > K + 1
    monkeypatch.setattr(recommend, "BLOCK_BYTES", 1 << 30 if block_bytes is None else block_bytes)
    args = (torch.from_numpy(c["users"]).to(gpu), torch.arange(Q), torch.from_numpy(c["cands"]).to(gpu), K)
    seen = _spy(monkeypatch)
    idx, score = recommend.topk_rows(*args, excl=excl, **kw)
    labels = list(seen)
    share = _check(c["S"], rows, K, idx, score)
    assert share > 0.9, share
    i32, s32 = recommend.topk_rows(*args, excl=excl, index_dtype=torch.int32, **kw)
    assert idx.dtype == torch.int64 and i32.dtype == torch.int32
    assert torch.equal(i32.to(torch.int64), idx) and torch.equal(s32.view(torch.int32), score.view(torch.int32))
    assert seen[len(labels):] == labels  # the index dtype changes no call
    return labels


@pytest.mark.parametrize("form", EXCL_FORMS)
def test_dense_one_filter_and_one_emit_per_block(gpu, monkeypatch, form):
    assert _run(gpu, monkeypatch, form) == NORMALIZE + ["lgcn_score_filter(dense)", "lgcn_select_topk_ranked"]
    # 128 queries per block: the two tiles are a block each
    assert _run(gpu, monkeypatch, form, block_bytes=8 * M * 128) == NORMALIZE + [
        "lgcn_score_filter(dense)", "lgcn_select_topk_ranked", "lgcn_score_filter(dense)", "lgcn_select_topk_ranked"]
    assert _run(gpu, monkeypatch, form, filtered=True) == NORMALIZE + [
        "lgcn_score_filter(dense)", "lgcn_select_topk_ranked_attr"]


@pytest.mark.parametrize("form", EXCL_FORMS)
def test_filtered_subset_thresholds_then_one_list_pass(gpu, monkeypatch, form):
    assert _run(gpu, monkeypatch, form, cap=64, subset=32) == NORMALIZE + [
        "lgcn_score_filter(subset)", "lgcn_select_topk_ranked", "lgcn_score_filter", "lgcn_select_topk_ranked"]
    assert _run(gpu, monkeypatch, form, cap=64, subset=32, block_bytes=8 * 64 * 128) == NORMALIZE + 2 * [
        "lgcn_score_filter(subset)", "lgcn_select_topk_ranked", "lgcn_score_filter", "lgcn_select_topk_ranked"]
    assert _run(gpu, monkeypatch, form, filtered=True, cap=64, subset=32) == NORMALIZE + [
        "lgcn_score_filter(subset)", "lgcn_select_topk_ranked_attr", "lgcn_score_filter_attr",
        "lgcn_select_topk_ranked_attr"]


@pytest.mark.parametrize("form", EXCL_FORMS)
def test_among_one_list_call_and_one_emit_per_block(gpu, monkeypatch, form):
    from lgcn_amd.recommend import _among_blocks

    lengths = sorted((len(r) for r in _case()["among"]), reverse=True)
    bytes_ = 8 * 300 * 16  # 16 queries at the longest rows' capacity: (0, 16), (16, 32) at 300, the rest at 40
    assert _among_blocks(lengths, K, bytes_) == [(0, 16, 300), (16, 32, 300), (32, 130, 40)]
    assert _run(gpu, monkeypatch, form, among=True) == NORMALIZE + ["lgcn_score_lists", "lgcn_select_topk_ranked"]
    assert _run(gpu, monkeypatch, form, among=True, block_bytes=bytes_) == NORMALIZE + 3 * [
        "lgcn_score_lists", "lgcn_select_topk_ranked"]
    assert _run(gpu, monkeypatch, form, among=True, filtered=True, block_bytes=bytes_) == NORMALIZE + 3 * [
        "lgcn_score_lists", "lgcn_select_topk_ranked_attr"]
