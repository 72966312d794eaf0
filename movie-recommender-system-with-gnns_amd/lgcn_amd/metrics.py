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
With evaluate_ranking(calibration=...) they are recommend.topk_rows_calibrated's (a greedy re-rank towards
the genre mix of the user's history) and the result carries ckl@c, the mean KL divergence between that mix
and the list's (recommend.miscalibration) over the evaluated users with a non-zero target.

Below the cutoff (no cap of 1,024, no lists): rank_positions gives every (user, held-out item) pair
its exact 0-based position in the user's full ranking (lgcn_rank_positions, csrc/lgcn_rankpos.hip:
a counting pass over all items on the ranking kernels' f32 MFMA keys, the same order and tie rule
as the lists above), summarize_positions turns positions into AUC, mean percentile rank, MRR, mean
rank and the metrics above at ANY cutoffs, and evaluate_auc is the two for an embedding pair.
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
    ptr, idx, rows = _serving.csr_on(dev, ptr, idx, rows)
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
                     diversity: float | None = None, pool: int | None = None, calibration: float | None = None,
                     attrs: torch.Tensor | None = None, history=None, **topk_kw) -> dict:
    """Full-ranking evaluation of an embedding pair: summarize's dict.

    truth: the held-out CSR over all users, (ptr, idx) as recommend.seen_csr(heldout_edges, U, I)
    builds it; seen: the training CSR whose items are left out of every user's ranking (None:
    nothing excluded); users: the user indices evaluated (default: every user with a non-empty
    truth row); ks: the cutoffs; topk_kw: recommend.topk_rows' cap / subset / attrs / where (an attribute
    filter: the metrics of the filtered lists against the same truth) and among (a candidate set per
    user, seen's convention: a 2-tuple is a CSR over all users, a 3-tuple names each evaluated user's
    row; the metrics of the lists ranked among the sets — the sampled-negative protocol's numbers
    when a set is the user's held-out items and sampled negatives; a re-rank pool then holds set
    entries only) and boost (one f32 per item added to every user's scores, recommend.popularity_boost's
    penalty for one: the metrics of the boosted lists, re-ranked ones included, against the same truth).
    One recommend.topk_items call for max(ks) items per user, one lgcn_rank_metrics launch, then
    summarize. Host reads: summarize's one; topk_rows' one per query block when the items exceed
    its dense capacity; and, when ``users`` is left to default, the size of torch.nonzero's result
    (pass ``users`` to avoid it — users without truth are left out of the means either way).

    diversity: None evaluates the relevance lists (the keys above, nothing else). A float in [0, 1]
    evaluates what recommend.topk_rows_diverse serves instead — each user's pool of ``pool`` entries
    (its default when None) re-ranked by greedy MMR down to max(ks); 0.0 keeps the relevance lists
    and only measures — and the result also carries 'ild@c' for every cutoff: the mean of
    recommend.intra_list_diversity over the evaluated users (non-empty truth row) with at least two
    listed items, nan when there is none. One more host read.

    calibration: None as above. A float in [0, 1] evaluates what recommend.topk_rows_calibrated serves
    — each user's pool of ``pool`` entries re-ranked towards the genre mix of the user's history;
    0.0 keeps the relevance lists and only measures — and the result also carries 'ckl@c' for every
    cutoff: the mean of recommend.miscalibration (KL between the history's genre distribution and the
    list's) over the evaluated users whose target is non-zero, nan when there is none. attrs: the
    items' attribute words (int32 [M] on the device; needed, and shared with a where= filter);
    history: the CSR over all users the targets are profiled from (default: ``seen``). One re-rank per
    call: calibration together with diversity is a ValueError. One more host read."""
    cs = _cutoffs(ks)
    if calibration is not None and diversity is not None:
        raise ValueError("evaluate_ranking: calibration and diversity are two re-ranks; one per call")
    if diversity is None and calibration is None and pool is not None:
        raise ValueError("evaluate_ranking: pool is the re-rank's pool and needs diversity")
    if diversity is not None:
        diversity = recommend._diversity(diversity)
    if calibration is not None:
        calibration = recommend._calibration(calibration)
        history = seen if history is None else history
        if history is None:
            raise ValueError("evaluate_ranking: calibration needs history= or seen= (what the targets are profiled from)")
        if attrs is None:
            raise ValueError("evaluate_ranking: calibration needs attrs (the items' attribute words)")
    elif history is not None:
        raise ValueError("evaluate_ranking: history is the calibration's and needs calibration")
    elif attrs is not None:
        topk_kw["attrs"] = attrs
    _ffi.require_device(user_emb, "evaluate_ranking")
    dev = user_emb.device
    ptr, idx = truth[0].to(dev), truth[1].to(dev)
    if users is None:
        users = torch.nonzero(ptr[1:] > ptr[:-1]).view(-1)
    users = torch.as_tensor(users).to(device=dev, dtype=torch.int64).view(-1)
    among = topk_kw.get("among")
    if among is not None and len(among) == 2:
        topk_kw["among"] = (among[0], among[1], users)
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
    if calibration is not None:
        excl = None if seen is None else (seen[0], seen[1], users)
        target, weight = recommend.attr_profile((history[0], history[1], users), attrs)
        lists = recommend.topk_rows_calibrated(user_emb, users, item_emb, cs[-1], calibration, attrs=attrs, target=target,
                                               pool=pool, excl=excl, index_dtype=torch.int32, **topk_kw)
        counts = rank_metrics(lists.idx, (ptr, idx), cs, rows=users)
        out = summarize(counts, cs)
        ckl = recommend.miscalibration(lists.kl, lists.n, cs)
        listed = ((counts.n_truth > 0) & (weight > 0))[:, None] & ~torch.isnan(ckl)
        sums = torch.where(listed, ckl, torch.zeros((), dtype=ckl.dtype, device=dev)).sum(0)
        flat = torch.cat([sums, listed.sum(0).to(ckl.dtype)]).tolist()  # the host read
        for j, cv in enumerate(cs):
            out[f"ckl@{cv}"] = flat[j] / flat[len(cs) + j] if flat[len(cs) + j] else float("nan")
        return out
    ranked, _ = recommend.topk_items(user_emb, item_emb, users, cs[-1], seen=seen, index_dtype=torch.int32, **topk_kw)
    return summarize(rank_metrics(ranked, (ptr, idx), cs, rows=users), cs)


class RankPositions(NamedTuple):
    """lgcn_rank_positions' outputs for Q queries whose truth rows hold nnz entries, on the device."""
    ptr: torch.Tensor       # int64 [Q + 1]: query q's entries are ptr[q] .. ptr[q + 1], in truth-row order
    pos: torch.Tensor       # int32 [nnz]: eligible candidates ranked above the item; -1: seen or outside [0, M)
    score: torch.Tensor     # f32 [nnz]: the score behind the item's key (NaN for an item outside [0, M))
    eligible: torch.Tensor  # int32 [Q]: candidates the query's seen row leaves


# truth-row lengths above which queries (sorted longest row first) are issued as a call of their own
TIER_LENGTHS = (256, 32)


def _tiers(Q: int, longer) -> list:
    """[a, b) query ranges of rank_positions' calls: queries sorted longest truth row first, longer[i]
    of them with rows above TIER_LENGTHS[i]; boundaries on the kernels' 128-query groups. The dense
    count splits the candidates over about 2048 workgroups per call and a query group runs its
    passes one after the other, so the few queries with very long rows get a call of their own, in
    which each workgroup's share of the candidates (one pass) is short."""
    cuts = sorted({min(Q, -(-int(n) // 128) * 128) for n in longer} | {0, Q})
    return [(a, b) for a, b in zip(cuts[:-1], cuts[1:])]


def _issue_positions(lib, tiers, Qn, D, Cn, M, tptr, tidx, trow, sptr, sidx, srow, out_ptr, nnz, pos, key, eligible,
                     ws, stages, stream) -> None:
    """lgcn_rank_positions for each tier's queries: a slice of the query-indexed arrays, the whole of
    the entry-indexed ones (out_ptr holds absolute slots)."""
    for a, b in tiers:
        _ffi.check(lib.lgcn_rank_positions(Qn.data_ptr() + a * D * 4, _serving.padded(b - a), b - a, Cn.data_ptr(), M, D,
                                           *_serving.csr_at(tptr, tidx, trow, a), *_serving.csr_at(sptr, sidx, srow, a),
                                           out_ptr.data_ptr() + a * 8, nnz, pos.data_ptr(), key.data_ptr(),
                                           eligible.data_ptr() + a * 4, ws.data_ptr(), ws.numel(), stages, stream),
                   "lgcn_rank_positions")


def rank_positions(queries: torch.Tensor, picked, candidates: torch.Tensor, truth, seen=None, rows=None,
                   normalized: bool = False) -> RankPositions:
    """Where each held-out item stands in its query's full ranking, on the device.

    Query q is the row queries[picked[q]]; candidates [M, d] are ranked for it by cosine score as
    recommend.topk_rows ranks them (score descending, candidate index ascending, NaN first, the
    query's seen row left out), and for every entry j of its truth row pos is the number of eligible
    candidates ranked above j: pos = p < k exactly when topk_rows(..., k, excl=seen) has j at slot p.
    pos is -1 for an entry that is in the seen row or outside [0, M); other truth entries count as
    candidates. No [Q, M] matrix and no lists exist at any point, and k is not capped.
    truth: (ptr, idx) as recommend.seen_csr builds it; rows[q] names the truth row of query q (row q
    when rows is None); a row outside the CSR is empty. seen: None, (ptr, idx) — row q is query q's —
    or (ptr, idx, rows); rows ascending and distinct. Both are checked by _serving.csr_arg.
    normalized=True takes queries and candidates as unit rows already (only zero-padded).
    One host read: the number of truth entries (the size of pos)."""
    who = "rank_positions"
    if queries.dim() != 2 or candidates.dim() != 2:
        raise ValueError(f"{who}: queries and candidates must be 2-D")
    if queries.dtype != torch.float32 or candidates.dtype != torch.float32:
        raise TypeError(f"{who}: queries and candidates must be float32")
    if candidates.shape[1] != queries.shape[1]:
        raise ValueError(f"{who}: queries and candidates must have the same width")
    d, M = queries.shape[1], candidates.shape[0]
    D = _serving.width(who, d)
    picked = torch.as_tensor(picked).reshape(-1)
    if picked.dtype.is_floating_point or picked.dtype.is_complex or picked.dtype == torch.bool:
        raise TypeError(f"{who}: picked must be integers, got {picked.dtype}")
    Q = picked.numel()
    if truth is None or len(truth) != 2:
        raise ValueError(f"{who}: truth is (ptr, idx)")
    tptr, tidx, trow, _ = _serving.csr_arg(who, "truth", tuple(truth) if rows is None else (*truth, rows), Q, short=True)
    sptr = sidx = srow = None
    if seen is not None:
        sptr, sidx, srow, _ = _serving.csr_arg(who, "seen", seen, Q)
    lib = _ffi.load()
    for t in (queries, candidates, tptr, tidx) + (() if seen is None else (sptr, sidx)):
        _ffi.require_device(t, who)
    dev = queries.device
    s = _ffi.stream_of(dev)
    picked = picked.to(device=dev, dtype=torch.int64).contiguous()
    tptr, tidx, trow = _serving.csr_on(dev, tptr, tidx, trow)
    if seen is not None and sidx.numel() == 0:  # nothing is seen anywhere (and no device address to pass)
        sptr = sidx = srow = None
    elif seen is not None:
        sptr, sidx, srow = _serving.csr_on(dev, sptr, sidx, srow)
    out_ptr = torch.zeros(Q + 1, dtype=torch.int64, device=dev)
    lens = _serving.row_lengths(tptr, trow, Q)
    if Q:
        out_ptr[1:] = torch.cumsum(lens, 0)
    nnz, *longer = torch.stack([out_ptr[-1]] + [(lens > n).sum() for n in TIER_LENGTHS]).tolist()  # the host read
    # The dense count takes a workgroup's 128 queries through as many passes as their longest truth
    # row asks for, so the queries go to the library longest row first (rows of a kind share a
    # workgroup) and the outputs come back in the caller's order. Positions are exact counts: the
    # order changes no value.
    order = None
    if Q > 128 and nnz:
        order = _serving.longest_first(lens).indices
        picked, trow = picked[order], _serving.rows_in(order, trow)
        if sptr is not None:
            srow = _serving.rows_in(order, srow)
        given_ptr, out_ptr = out_ptr, torch.zeros_like(out_ptr)
        out_ptr[1:] = torch.cumsum(lens[order], 0)
    pos = torch.empty(nnz, dtype=torch.int32, device=dev)
    key = torch.empty(nnz, dtype=torch.int32, device=dev)
    eligible = torch.empty(Q, dtype=torch.int32, device=dev)
    if Q and nnz == 0:  # the library launches nothing without truth entries
        if sptr is None:
            eligible.fill_(M)
        else:
            inside = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev),
                                torch.cumsum(((sidx >= 0) & (sidx < M)).to(torch.int64), 0)])
            R = sptr.numel() - 1
            r = torch.arange(Q, device=dev) if srow is None else srow
            ok = (r >= 0) & (r < R)
            rc = r.clamp(0, max(R - 1, 0))
            n = torch.where(ok, inside[sptr[(rc + 1).clamp(max=R)]] - inside[sptr[rc]], torch.zeros_like(rc))
            eligible.copy_(M - n)
    elif Q:
        Qn = _serving.unit_queries(lib, queries, picked, D, _serving.padded(Q), normalized, s)
        Cn = _serving.unit_rows(lib, candidates, D, normalized, s)
        need = ctypes.c_size_t(0)
        _ffi.check(lib.lgcn_rank_positions_workspace_size(Q, nnz, ctypes.byref(need)), "lgcn_rank_positions_workspace_size")
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        tiers = _tiers(Q, longer) if order is not None else [(0, Q)]
        _issue_positions(lib, tiers, Qn, D, Cn, M, tptr, tidx, trow, sptr, sidx, srow, out_ptr, nnz, pos, key,
                         eligible, ws, _ffi.RANKPOS_ALL, s)
    if order is not None:  # back to the caller's order: query q's entries start at out_ptr[where q went]
        moved = _serving.in_caller_order(order, out_ptr[:-1]) - given_ptr[:-1]
        src = torch.repeat_interleave(moved, lens, output_size=nnz) + torch.arange(nnz, device=dev)
        pos, key, eligible, out_ptr = pos[src], key[src], _serving.in_caller_order(order, eligible), given_ptr
    # the score behind a key (csrc/lgcn_ragged.h ordered_value; key 0, "no key", comes out a NaN)
    bits = torch.where(key < 0, key ^ torch.iinfo(torch.int32).min, ~key)
    return RankPositions(out_ptr, pos, bits.view(torch.float32), eligible)


def summarize_positions(positions, ks=()) -> dict:
    """AUC and its relatives from exact positions: {'users', 'auc', 'mpr', 'mrr', 'mean_rank'} plus
    recall@c, precision@c, hit_rate@c, ndcg@c and mrr@c for every c of ``ks`` — any positive
    integers, any number of them (neither MAX_CUTOFFS nor the ranked lists' 1,024 applies).
    For a user with ranked held-out items H' = {pos >= 0}, n = |H'| and N_neg = eligible - n:
        auc       = 1 - (sum of pos - n (n - 1) / 2) / (n * N_neg)   the share of (held-out,
                    negative) pairs the model orders correctly: an item at position p has p - (its
                    rank among H') negatives above it
        mpr       = mean of pos / max(eligible - 1, 1)               0 is best
        mrr       = 1 / (min pos + 1)
        mean_rank = mean of pos
    and the @c metrics exactly as the module docstring defines them, the hit ranks being the
    positions below c and T the whole truth row (a held-out item that can never be ranked still
    counts in T). Every value is the mean over the users with n > 0 and N_neg > 0, 'users' their
    number; nan when there is none. Float64 torch on the tensors' device (CPU tensors work too), one
    host read."""
    ptr, pos, _, eligible = positions
    cs = sorted({int(c) for c in ks})
    if cs and cs[0] < 1:
        raise ValueError(f"summarize_positions: cutoffs {cs} must be positive")
    Q, nnz = eligible.numel(), pos.numel()
    if ptr.numel() != Q + 1:
        raise ValueError(f"summarize_positions: ptr has {ptr.numel()} entries for {Q} queries")
    dev, f64, i64 = pos.device, torch.float64, torch.int64
    T = (ptr[1:] - ptr[:-1]).to(i64)
    qid = torch.repeat_interleave(torch.arange(Q, device=dev), T, output_size=nnz)
    p = pos.to(i64)
    ranked = p >= 0
    per_user = lambda v: torch.zeros(Q, dtype=v.dtype, device=dev).index_add_(0, qid, v)
    n = per_user(ranked.to(i64))
    total = per_user(torch.where(ranked, p, torch.zeros_like(p)))
    far = torch.iinfo(i64).max
    first = torch.full((Q,), far, dtype=i64, device=dev).scatter_reduce_(
        0, qid, torch.where(ranked, p, torch.full_like(p, far)), "amin")
    elig = eligible.to(i64)
    n_neg = elig - n
    valid = (n > 0) & (n_neg > 0)
    nf, tf = n.clamp(min=1).to(f64), total.to(f64)
    cols = [1.0 - (tf - (n * (n - 1)).to(f64) / 2.0) / (nf * n_neg.clamp(min=1).to(f64)),
            tf / nf / (elig - 1).clamp(min=1).to(f64),
            1.0 / (first.clamp(max=far - 1) + 1).to(f64),
            tf / nf]
    names = ["auc", "mpr", "mrr", "mean_rank"]
    if cs:
        c = torch.tensor(cs, dtype=i64, device=dev)
        hit = ranked[:, None] & (p[:, None] < c[None, :])  # [nnz, C]
        hits = torch.zeros((Q, len(cs)), dtype=f64, device=dev).index_add_(0, qid, hit.to(f64))
        gain = 1.0 / torch.log2((p.clamp(min=0) + 2).to(f64))
        dcg = torch.zeros((Q, len(cs)), dtype=f64, device=dev).index_add_(
            0, qid, torch.where(hit, gain[:, None], torch.zeros((), dtype=f64, device=dev)))
        deep = min(cs[-1], max(nnz, 1))  # no truth row is longer than nnz
        table = torch.cat([torch.zeros(1, dtype=f64, device=dev),
                           torch.cumsum(1.0 / torch.log2(torch.arange(2, deep + 2, dtype=f64, device=dev)), 0)])
        idcg = table[torch.minimum(T.clamp(min=1)[:, None], c[None, :]).clamp(max=deep)]
        rr = torch.where(first[:, None] < c[None, :], 1.0 / (first.clamp(max=far - 1) + 1).to(f64)[:, None],
                         torch.zeros((), dtype=f64, device=dev))
        per_c = [hits / T.clamp(min=1).to(f64)[:, None], hits / c.to(f64)[None, :], (hits > 0).to(f64), dcg / idcg, rr]
    w = valid.to(f64)
    zero = torch.zeros((), dtype=f64, device=dev)
    parts = [torch.stack([torch.where(valid, v, zero).sum() for v in cols])]
    if cs:  # summed as summarize sums its [Q, C] columns, so equal counts give equal means
        parts.append(torch.stack([(torch.where(valid[:, None], m, zero) * w[:, None]).sum(0) for m in per_c]).reshape(-1))
        names += [f"{name}@{cv}" for name in METRICS for cv in cs]
    sums = torch.cat(parts + [w.sum().view(1)]).tolist()  # the host read
    users = int(sums[-1])
    out = {"users": users}
    for name, v in zip(names, sums):
        out[name] = v / users if users else float("nan")
    return out


def evaluate_auc(user_emb: torch.Tensor, item_emb: torch.Tensor, truth, seen=None, users=None, ks=()) -> dict:
    """Exact full-ranking AUC of an embedding pair: summarize_positions' dict.

    truth, seen and users are evaluate_ranking's: the held-out CSR over all users, the training CSR
    whose items are left out of every user's ranking, the user indices evaluated (default: every
    user with a non-empty truth row; pass it to avoid the host read of torch.nonzero's size). Rows of
    foldin.fold_in serve as user_emb like any others (users = their indices, truth and seen by the
    same rows). ks: cutoffs for the @c metrics, any positive integers. One rank_positions call (one
    host read), then summarize_positions (one more)."""
    _ffi.require_device(user_emb, "evaluate_auc")
    dev = user_emb.device
    ptr, idx = truth[0].to(dev), truth[1].to(dev)
    if users is None:
        users = torch.nonzero(ptr[1:] > ptr[:-1]).view(-1)
    users = torch.as_tensor(users).to(device=dev, dtype=torch.int64).view(-1)
    positions = rank_positions(user_emb, users, item_emb, (ptr, idx), rows=users,
                               seen=None if seen is None else (seen[0], seen[1], users))
    return summarize_positions(positions, ks)
