"""Full-ranking evaluation on the GPU: rank every item for every user who has held-out items, the
user's training items left out, and report Recall / Precision / HitRate / NDCG / MRR at several
cutoffs — the protocol recommenders are compared by (the reference's compute_recall_at_k is a
sampled Recall and stays in utils/train_test.py for parity).

    ranked lists      recommend.topk_items (lgcn_score_filter + lgcn_select_topk_ranked), int32
    per-query counts  lgcn_rank_metrics (csrc/lgcn_metrics.hip): hits and DCG per cutoff, first hit
                      rank, truth length — one pass for all cutoffs, no [Q * k] key tensors
    means             summarize: float64 torch ops on the counts' device, one host read

Definitions, for a user with truth set of T > 0 items, hits h_c among ranks r < c (0-based), and
the lowest hit rank ``first``:
    recall@c = h_c / T        precision@c = h_c / c        hit_rate@c = [h_c > 0]
    ndcg@c   = DCG_c / IDCG_c,  DCG_c = sum over hit ranks r < c of 1 / log2(r + 2),
                                IDCG_c = sum over r < min(c, T) of 1 / log2(r + 2)
    mrr@c    = 1 / (first + 1) if 0 <= first < c else 0
each averaged over the users with T > 0 (``users`` in the result).
With evaluate_ranking(diversity=...) the lists are recommend.topk_rows_diverse's (greedy MMR over a
relevance pool) and the result also carries ild@c, the mean intra-list diversity
(recommend.intra_list_diversity) over the evaluated users with at least two listed items.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import torch

from . import _ffi, _serving, recommend

MAX_CUTOFFS = _ffi.METRICS_MAX_CUTOFFS
METRICS = ("recall", "precision", "hit_rate", "ndcg", "mrr")


class RankCounts(NamedTuple):
    """lgcn_rank_metrics' outputs for Q queries and C cutoffs, on the device."""
    hits: torch.Tensor     # int32 [Q, C]: hits among ranks below each cutoff
    dcg: torch.Tensor      # f32 [Q, C]: their discounts 1 / log2(rank + 2), summed in float64, rounded once
    first: torch.Tensor    # int32 [Q]: the lowest hit rank, -1 if none
    n_truth: torch.Tensor  # int32 [Q]: the truth row's length


def _cutoffs(ks, k: int | None = None) -> list[int]:
    """ks sorted and deduplicated; ValueError for none, too many, or values outside [1, k]."""
    cs = sorted({int(c) for c in ks})
    if not 1 <= len(cs) <= MAX_CUTOFFS:
        raise ValueError(f"metrics: {len(cs)} distinct cutoffs, need 1 to {MAX_CUTOFFS}")
    if cs[0] < 1 or (k is not None and cs[-1] > k):
        raise ValueError(f"metrics: cutoffs {cs} outside [1, k{'' if k is None else '=' + str(k)}]")
    return cs


def rank_metrics(ranked_idx: torch.Tensor, truth, ks, rows=None) -> RankCounts:
    """Per-query counts of ranked lists against held-out sets, on the device.

    ranked_idx: [Q, k] int32 or int64 (converted once; topk_rows(index_dtype=torch.int32) needs no
    conversion), row q holding query q's candidates in rank order, distinct, negative in unfilled
    slots. An int64 value outside int32 cannot be a truth index and is taken as -1 (never a hit)
    rather than wrapped. Rows may be strided (a column slice of a wider tensor).
    truth: (ptr int64 [R + 1], idx int32) as recommend.seen_csr builds it; rows[q] names the truth
    row of query q (row q when rows is None); a row outside [0, R) is an empty set. Both are checked
    by _serving.csr_arg.
    ks: cutoffs, any iterable of ints in [1, k]; sorted and deduplicated, at most MAX_CUTOFFS.
    The columns of the result follow the sorted cutoffs."""
    if ranked_idx.dim() != 2:
        raise ValueError("rank_metrics: ranked_idx must be [Q, k]")
    Q, k = ranked_idx.shape
    if k < 1 or k > _ffi.RANKED_MAX_K:
        raise ValueError(f"rank_metrics: k={k} outside [1, {_ffi.RANKED_MAX_K}]")
    cs = _cutoffs(ks, k)
    _serving.require_index_dtype("rank_metrics", "ranked_idx", ranked_idx)
    if len(truth) != 2:
        raise ValueError("rank_metrics: truth is (ptr, idx)")
    # a truth CSR may end before the queries do: those queries have empty rows
    truth = tuple(truth) if rows is None else (*truth, rows)
    ptr, idx, rows, _ = _serving.csr_arg("rank_metrics", "truth", truth, Q, short=True)
    lib = _ffi.load()
    for t in (ranked_idx, ptr, idx):
        _ffi.require_device(t, "rank_metrics")
    dev = ranked_idx.device
    ranked_idx, ld = _serving.index_list(ranked_idx)
    ptr, idx = ptr.contiguous(), idx.contiguous()
    if idx.numel() == 0:  # every row is empty: the library still wants an address
        idx = torch.zeros(1, dtype=torch.int32, device=dev)
    if rows is not None:
        rows = rows.to(device=dev, dtype=torch.int64).contiguous()
    C = len(cs)
    hits = torch.empty((Q, C), dtype=torch.int32, device=dev)
    dcg = torch.empty((Q, C), dtype=torch.float32, device=dev)
    first = torch.empty(Q, dtype=torch.int32, device=dev)
    n_truth = torch.empty(Q, dtype=torch.int32, device=dev)
    if Q:
        cut = (ctypes.c_int32 * C)(*cs)
        _ffi.check(lib.lgcn_rank_metrics(ranked_idx.data_ptr(), ld, k, Q, ptr.data_ptr(),
                                         idx.data_ptr(), _ffi.ptr(rows), ptr.numel() - 1, cut, C, hits.data_ptr(),
                                         dcg.data_ptr(), first.data_ptr(), n_truth.data_ptr(), _ffi.stream_of(dev)),
                   "lgcn_rank_metrics")
    return RankCounts(hits, dcg, first, n_truth)


def summarize(counts, ks) -> dict:
    """The means of recall / precision / hit_rate / ndcg / mrr at each cutoff over the queries with
    a non-empty truth row: {'users': n, 'recall@c': ..., 'precision@c': ..., 'hit_rate@c': ...,
    'ndcg@c': ..., 'mrr@c': ...} for every c of ``ks`` (sorted and deduplicated, matching the
    columns of ``counts``). Pure torch on the counts' device (CPU tensors work too), accumulated in
    float64, one host read. With no such query every metric is nan and users is 0.

    A truth entry that the query's seen set also holds can never be ranked, so never hit, yet it
    still counts in the truth length: recall and the ideal DCG are taken over the whole truth row.
    Keeping the held-out set disjoint from the training set is the caller's job."""
    hits, dcg, first, n_truth = counts
    cs = _cutoffs(ks)
    if hits.dim() != 2 or hits.shape[1] != len(cs) or dcg.shape != hits.shape:
        raise ValueError(f"summarize: counts have {tuple(hits.shape)} columns for {len(cs)} cutoffs")
    if first.shape != hits.shape[:1] or n_truth.shape != hits.shape[:1]:
        raise ValueError(f"summarize: first {tuple(first.shape)} / n_truth {tuple(n_truth.shape)} do not match "
                         f"hits {tuple(hits.shape)}")
    dev, f64 = hits.device, torch.float64
    c = torch.tensor(cs, dtype=torch.int64, device=dev)
    valid = n_truth > 0
    w = valid.to(f64)[:, None]
    T = n_truth.to(torch.int64).clamp(min=1)
    h = hits.to(f64)
    # IDCG from a float64 cumulative table: table[m] = sum over r < m of 1 / log2(r + 2)
    table = torch.cat([torch.zeros(1, dtype=f64, device=dev),
                       torch.cumsum(1.0 / torch.log2(torch.arange(2, cs[-1] + 2, dtype=f64, device=dev)), 0)])
    idcg = table[torch.minimum(T[:, None], c[None, :])]
    f = first.to(torch.int64)[:, None]
    rr = torch.where((f >= 0) & (f < c[None, :]), 1.0 / (f + 1).to(f64), torch.zeros((), dtype=f64, device=dev))
    sums = torch.stack([(h / T.to(f64)[:, None] * w).sum(0),
                        (h / c.to(f64)[None, :] * w).sum(0),
                        ((hits > 0).to(f64) * w).sum(0),
                        (dcg.to(f64) / idcg * w).sum(0),
                        (rr * w).sum(0)])
    flat = torch.cat([sums.reshape(-1), valid.sum().to(f64).view(1)]).tolist()  # the host read
    n = int(flat[-1])
    out = {"users": n}
    for m, name in enumerate(METRICS):
        for j, cv in enumerate(cs):
            out[f"{name}@{cv}"] = flat[m * len(cs) + j] / n if n else float("nan")
    return out


def evaluate_ranking(user_emb: torch.Tensor, item_emb: torch.Tensor, truth, ks=(20,), seen=None, users=None,
                     diversity: float | None = None, pool: int | None = None, **topk_kw) -> dict:
    """Full-ranking evaluation of an embedding pair: summarize's dict.

    truth: the held-out CSR over all users, (ptr, idx) as recommend.seen_csr(heldout_edges, U, I)
    builds it; seen: the training CSR whose items are left out of every user's ranking (None:
    nothing excluded); users: the user indices evaluated (default: every user with a non-empty
    truth row); ks: the cutoffs; topk_kw: recommend.topk_rows' cap / subset.
    One recommend.topk_items call for max(ks) items per user, one lgcn_rank_metrics launch, then
    summarize. Host reads: summarize's one; topk_rows' one per query block when the items exceed
    its dense capacity; and, when ``users`` is left to default, the size of torch.nonzero's result
    (pass ``users`` to avoid it — users without truth are left out of the means either way).

    diversity: None evaluates the relevance lists (the keys above, nothing else). A float in [0, 1]
    evaluates what recommend.topk_rows_diverse serves instead — each user's pool of ``pool`` entries
    (its default when None) re-ranked by greedy MMR down to max(ks); 0.0 keeps the relevance lists
    and only measures — and the result also carries 'ild@c' for every cutoff: the mean of
    recommend.intra_list_diversity over the evaluated users (non-empty truth row) with at least two
    listed items, nan when there is none. One more host read."""
    cs = _cutoffs(ks)
    if diversity is None and pool is not None:
        raise ValueError("evaluate_ranking: pool is the re-rank's pool and needs diversity")
    if diversity is not None:
        diversity = recommend._diversity(diversity)
    _ffi.require_device(user_emb, "evaluate_ranking")
    dev = user_emb.device
    ptr, idx = truth[0].to(dev), truth[1].to(dev)
    if users is None:
        users = torch.nonzero(ptr[1:] > ptr[:-1]).view(-1)
    users = torch.as_tensor(users).to(device=dev, dtype=torch.int64).view(-1)
    if diversity is not None:
        excl = None if seen is None else (seen[0], seen[1], users)
        lists = recommend.topk_rows_diverse(user_emb, users, item_emb, cs[-1], diversity, pool=pool, excl=excl,
                                            index_dtype=torch.int32, **topk_kw)
        counts = rank_metrics(lists.idx, (ptr, idx), cs, rows=users)
        out = summarize(counts, cs)
        ild = recommend.intra_list_diversity(lists.pair, lists.n, cs)
        listed = (counts.n_truth > 0)[:, None] & ~torch.isnan(ild)
        sums = torch.where(listed, ild, torch.zeros((), dtype=ild.dtype, device=dev)).sum(0)
        flat = torch.cat([sums, listed.sum(0).to(ild.dtype)]).tolist()  # the host read
        for j, cv in enumerate(cs):
            out[f"ild@{cv}"] = flat[j] / flat[len(cs) + j] if flat[len(cs) + j] else float("nan")
        return out
    ranked, _ = recommend.topk_items(user_emb, item_emb, users, cs[-1], seen=seen, index_dtype=torch.int32, **topk_kw)
    return summarize(rank_metrics(ranked, (ptr, idx), cs, rows=users), cs)
