"""Top-k recommendation on the GPU: which candidates, in which order, with the rows a query has
already seen left out (the product of reference utils/recommend.py, batched), on the Recall
kernels plus lgcn_select_topk_ranked (csrc/lgcn_recall.hip). No [Q, M] score matrix exists at
any point and the host reads at most one value pair per query block.

    Qn = normalize(queries[picked])      lgcn_normalize_rows (gathered, zero-padded), once
    Cn = normalize(candidates)           lgcn_normalize_rows, once for all query blocks
    per query block (BLOCK_BYTES of list workspace):
      M <= cap:  dense scores            lgcn_score_filter (dense)
                 ranked emit             lgcn_select_topk_ranked
      M >  cap:  thr = k-th best ELIGIBLE entry of a strided subset
                                         lgcn_score_filter (dense) + lgcn_select_topk_ranked (threshold)
                 lists = scores >= thr   lgcn_score_filter (f32 MFMA, all M)
                 ranked emit             lgcn_select_topk_ranked

Ranking rule: score descending, then candidate index ascending (NaN scores first). The threshold
is formed from eligible subset entries only: it is then the k-th best of a subset of the eligible
candidates, so it is a lower bound of the k-th best eligible score of all M, and the filtered list
holds the whole eligible top k whatever was excluded.
"""
from __future__ import annotations

import ctypes

import torch

from . import _ffi
from .recall import _normalize_into

# list workspace of one query block (8 bytes per list slot: key + index); follows recall.STL_BLOCK_BYTES
BLOCK_BYTES = 1 << 30
# per-query list capacity of the filtered path, and the largest M the dense path takes
CAP = 16384
# candidates scored for the first thresholds: max(SUBSET_MIN, SUBSET_PER_K * k), at most the capacity
# (about k * M / subset entries survive the filter)
SUBSET_MIN = 2048
SUBSET_PER_K = 16
MAX_K = _ffi.RANKED_MAX_K


def seen_csr(edge_index: torch.Tensor, num_users: int, num_items: int, by: str = "user"):
    """The exclusion CSR of a training edge set: (ptr int64 [R + 1], idx int32), row u holding the
    0-based item indices user u has an edge to, ascending and deduplicated (by="item": row i holds
    the user indices of item i). edge_index uses the project's global numbering (items at
    num_users + i) and may hold either or both directions; edges that do not join a user and an
    item are ignored. Plain torch ops on edge_index's device."""
    if by not in ("user", "item"):
        raise ValueError(f"seen_csr: by must be 'user' or 'item', got {by!r}")
    U, I = int(num_users), int(num_items)
    src, dst = edge_index[0].to(torch.int64), edge_index[1].to(torch.int64)
    is_user = lambda t: (t >= 0) & (t < U)
    is_item = lambda t: (t >= U) & (t < U + I)
    fwd, bwd = is_user(src) & is_item(dst), is_item(src) & is_user(dst)
    users = torch.cat([src[fwd], dst[bwd]])
    items = torch.cat([dst[fwd], src[bwd]]) - U
    rows, cols, R, C = (users, items, U, I) if by == "user" else (items, users, I, U)
    key = torch.unique(rows * max(C, 1) + cols, sorted=True)
    ptr = torch.zeros(R + 1, dtype=torch.int64, device=edge_index.device)
    if R > 0:
        ptr[1:] = torch.cumsum(torch.bincount(key // max(C, 1), minlength=R), 0)
    return ptr, (key % max(C, 1)).to(torch.int32)


def _excl_args(excl, dev, Q: int):
    """(ptr, idx, rows | None, R) of an exclusion argument, checked and on the device."""
    if excl is None:
        return None, None, None, 0
    if len(excl) not in (2, 3):
        raise ValueError("recommend: excl is (ptr, idx) or (ptr, idx, rows)")
    ptr, idx = excl[0], excl[1]
    rows = excl[2] if len(excl) == 3 else None
    if ptr.dtype != torch.int64 or idx.dtype != torch.int32 or ptr.dim() != 1 or idx.dim() != 1 or ptr.numel() < 1:
        raise TypeError("recommend: excl needs ptr int64 [R + 1] and idx int32 (see seen_csr)")
    ptr, idx = ptr.to(dev).contiguous(), idx.to(dev).contiguous()
    R = ptr.numel() - 1
    if rows is not None:
        rows = torch.as_tensor(rows).to(device=dev, dtype=torch.int64).contiguous().view(-1)
        if rows.numel() != Q:
            raise ValueError(f"recommend: excl rows has {rows.numel()} entries for {Q} queries")
    elif R < Q:
        raise ValueError(f"recommend: excl has {R} rows for {Q} queries (pass the row of each query)")
    if idx.numel() == 0:  # nothing to exclude anywhere (and no device address to pass)
        return None, None, None, 0
    return ptr, idx, rows, R


def topk_rows(queries: torch.Tensor, picked: torch.Tensor, candidates: torch.Tensor, k: int, excl=None,
              cap: int | None = None, subset: int | None = None, index_dtype: torch.dtype = torch.int64):
    """(idx [Q, k] of ``index_dtype``, int64 by default; score f32 [Q, k]) on the device: for query
    row queries[picked[q]], the k best rows of ``candidates`` by cosine score that its exclusion row
    does not name, in rank order (score descending, candidate index ascending; NaN first).

    excl: None, or the CSR (ptr, idx) of seen_csr — row q belongs to query q — or (ptr, idx, rows)
    with rows[q] naming the CSR row of query q. Rows are ascending, deduplicated and within [0, M).
    cap: list slots per query (default CAP); candidates sets of at most ``cap`` rows are scored
    densely, and a query with fewer than k eligible candidates gets index -1 / score -inf in the
    slots it cannot fill. Above ``cap`` the first thresholds come from a strided subset (``subset``
    candidates) and a query with fewer than k eligible candidates raises ValueError; the filter
    does not know the exclusion rows, so ``cap`` must also hold a query's excluded candidates that
    score above its k-th eligible one (RuntimeError after eight tightening rounds otherwise).
    Queries are processed in blocks of at most BLOCK_BYTES of list workspace.
    index_dtype: torch.int64 (the default, what indexing wants) or torch.int32, the kernel's own
    index buffer handed on unconverted (what lgcn_amd.metrics.rank_metrics reads): a view of the
    first Q rows of this call's padded buffer, which lives as long as the view does."""
    k = int(k)
    if index_dtype not in (torch.int64, torch.int32):
        raise ValueError(f"recommend: index_dtype must be torch.int64 or torch.int32, got {index_dtype}")
    if k < 1 or k > MAX_K:
        raise ValueError(f"recommend: k={k} outside [1, {MAX_K}]")
    cap = CAP if cap is None else int(cap)
    if cap < k:
        raise ValueError(f"recommend: k={k} exceeds the list capacity {cap}")
    if cap > _ffi.RANKED_MAX_CAP:
        raise ValueError(f"recommend: cap={cap} exceeds {_ffi.RANKED_MAX_CAP}")
    subset = max(SUBSET_MIN, SUBSET_PER_K * k) if subset is None else int(subset)
    if subset < 1:
        raise ValueError(f"recommend: subset={subset}")
    lib = _ffi.load()
    for t in (queries, candidates):
        _ffi.require_device(t, "recommend")
    dev = queries.device
    d, M = queries.shape[1], candidates.shape[0]
    if candidates.shape[1] != d:
        raise ValueError("recommend: queries and candidates must have the same width")
    Dv, qm = ctypes.c_int32(0), ctypes.c_int32(0)
    _ffi.check(lib.lgcn_recall_width(d, ctypes.byref(Dv), ctypes.byref(qm)), "lgcn_recall_width")
    D, qmul = Dv.value, qm.value
    picked = torch.as_tensor(picked).to(device=dev, dtype=torch.int64).contiguous().view(-1)
    Q = picked.numel()
    ptr, eidx, erow, R = _excl_args(excl, dev, Q)
    if Q == 0:
        return (torch.empty((0, k), dtype=index_dtype, device=dev),
                torch.empty((0, k), dtype=torch.float32, device=dev))
    Qpad = max(qmul, (Q + qmul - 1) // qmul * qmul)
    dense = M <= cap
    if dense:
        cap = max(M, k)  # a dense row needs M slots
    s = _ffi.stream_of(dev)
    queries, candidates = queries.detach(), candidates.detach()
    Qn = torch.empty((Qpad, D), dtype=torch.float32, device=dev)
    Cn = torch.empty((max(M, 1), D), dtype=torch.float32, device=dev)
    _normalize_into(lib, queries, picked.data_ptr(), Q, Qn.data_ptr(), D, Qpad, s)
    _normalize_into(lib, candidates, None, M, Cn.data_ptr(), D, M, s)
    out_idx = torch.empty((Qpad, k), dtype=torch.int32, device=dev)
    out_score = torch.empty((Qpad, k), dtype=torch.float32, device=dev)
    out_n = torch.empty(Qpad, dtype=torch.int32, device=dev)
    blk = min(Qpad, max(qmul, (BLOCK_BYTES // (8 * cap)) // qmul * qmul))
    lkey = torch.empty((blk, cap), dtype=torch.int32, device=dev)
    lidx = torch.empty((blk, cap), dtype=torch.int32, device=dev)
    lcnt = torch.zeros(blk, dtype=torch.int32, device=dev)
    thr = torch.empty(blk, dtype=torch.int32, device=dev)
    stride = max(1, -(-M // min(subset, cap)))
    S = -(-M // stride) if M else 0

    def ranked(q0, nb, qv, counts, dense_n, thr_out, emit):
        if ptr is None:
            ex = (None, None, None, 0)
        elif erow is not None:
            ex = (ptr.data_ptr(), eidx.data_ptr(), erow.data_ptr() + q0 * 8, R)
        else:  # row q of the CSR is query q: the block starts at row q0
            ex = (ptr.data_ptr() + q0 * 8, eidx.data_ptr(), None, R - q0)
        outs = (out_idx.data_ptr() + q0 * k * 4, out_score.data_ptr() + q0 * k * 4,
                out_n.data_ptr() + q0 * 4) if emit else (None, None, None)
        _ffi.check(lib.lgcn_select_topk_ranked(lkey.data_ptr(), lidx.data_ptr(), counts, dense_n, cap, k, nb, qv, *ex,
                                               thr_out, *outs, s), "lgcn_select_topk_ranked")

    for q0 in range(0, Qpad, blk):
        nb = min(blk, Qpad - q0)
        qv = max(0, min(nb, Q - q0))
        qptr = Qn.data_ptr() + q0 * D * 4
        if dense:
            _ffi.check(lib.lgcn_score_filter(qptr, nb, qv, Cn.data_ptr(), M, 1, D, None, lkey.data_ptr(),
                                             lidx.data_ptr(), None, cap, s), "lgcn_score_filter(dense)")
            ranked(q0, nb, qv, None, M, None, True)
            continue
        if qv == 0:
            ranked(q0, nb, 0, None, 0, None, True)
            continue
        # eligible candidates of the block's poorest query, read with the first overflow check
        if ptr is None:
            fewest = torch.full((), M, dtype=torch.int64, device=dev)
        else:
            r = erow[q0:q0 + qv] if erow is not None else torch.arange(q0, q0 + qv, device=dev)
            inside = (r >= 0) & (r < R)  # a row outside the CSR excludes nothing, as in the kernel
            rc = r.clamp(0, R - 1)
            fewest = M - torch.where(inside, ptr[rc + 1] - ptr[rc], torch.zeros_like(rc)).max()
        # first thresholds: the k-th best eligible entry of a strided subset
        _ffi.check(lib.lgcn_score_filter(qptr, nb, qv, Cn.data_ptr(), S, stride, D, None, lkey.data_ptr(),
                                         lidx.data_ptr(), None, cap, s), "lgcn_score_filter(subset)")
        ranked(q0, nb, qv, None, S, thr.data_ptr(), False)
        for _ in range(8):
            lcnt.zero_()
            _ffi.check(lib.lgcn_score_filter(qptr, nb, qv, Cn.data_ptr(), M, 1, D, thr.data_ptr(), lkey.data_ptr(),
                                             lidx.data_ptr(), lcnt.data_ptr(), cap, s), "lgcn_score_filter")
            longest, few = torch.stack([lcnt[:qv].max().to(torch.int64), fewest]).tolist()  # the block's host read
            if few < k:
                raise ValueError(f"recommend: a query has {few} eligible candidates, fewer than k={k} "
                                 f"(M={M} is above the dense capacity {cap}, which pads such rows)")
            if longest <= cap:
                ranked(q0, nb, qv, lcnt.data_ptr(), 0, None, True)
                break
            # a list overflowed: its kept entries are real candidates, so the k-th best eligible one
            # among them is a valid, tighter threshold; filter again
            ranked(q0, nb, qv, lcnt.data_ptr(), 0, thr.data_ptr(), False)
        else:
            raise RuntimeError("recommend: candidate lists kept overflowing (scores too concentrated for the capacity)")
    return (out_idx[:Q].to(torch.int64) if index_dtype == torch.int64 else out_idx[:Q]), out_score[:Q].clone()


def topk_items(user_emb: torch.Tensor, item_emb: torch.Tensor, users, k: int, seen=None, **kw):
    """The k best items for each user index in ``users``; seen: seen_csr(..., by="user") over all
    users (row u is user u's), whose items are left out. Returns topk_rows' (idx, score)."""
    users = torch.as_tensor(users).view(-1)
    return topk_rows(user_emb, users, item_emb, k, excl=None if seen is None else (seen[0], seen[1], users), **kw)


def topk_users(user_emb: torch.Tensor, item_emb: torch.Tensor, items, k: int, seen=None, **kw):
    """The k best users for each item index in ``items``; seen: seen_csr(..., by="item")."""
    items = torch.as_tensor(items).view(-1)
    return topk_rows(item_emb, items, user_emb, k, excl=None if seen is None else (seen[0], seen[1], items), **kw)
