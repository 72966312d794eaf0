"""Fold-in: rows for users and items the model never saw, on the device (lgcn_foldin_rows in
csrc/lgcn_foldin.hip, one wave per history, eight for a long one; no [E, d] gather is materialised
and nothing is added atomically, so the rows are bitwise reproducible).

    fold_in_rows     a history CSR + a table (+ per-row factors, per-entry weights) -> FoldedIn
    fold_in          the same with the table rows' degrees given as counts
    inv_sqrt_degree  1 / sqrt(count + new_edge) in float64, rounded once (plain torch)
    layer_tables     the precombined tables S = c * sum_{l < K} x(l) of a trained model

The rule. A new node with n neighbours j (rows of a trained table, deg_j their degree in the training
graph, w_j an optional weight) gets from one propagation layer
    e(l + 1) = sum_j w_j / sqrt(n * (deg_j + 1)) * e_j(l),
the + 1 being the new edge itself. Every trained row stays as it is: this is the inductive
approximation, not a re-propagation of the graph with the node in it. The new node has no layer-0
row, so under the model's layer-stack scaling c its final row is the same sum over
S = c * sum_{l = 0}^{K - 1} x(l) (layer_tables): one ragged gather-sum against one table. For the raw
rows utils/recommend.py serves, S is the raw table. One function serves both directions: new users
are folded from item histories against S_item, new items from user lists against S_user. The rows go
wherever query rows go: recommend.topk_rows / topk_rows_diverse (the history as ``excl``),
explain.explain_rows, metrics.evaluate_ranking.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import _ffi, _serving

MAX_D = _ffi.FOLDIN_MAX_D  # columns of a table row
LONG = _ffi.FOLDIN_LONG    # history entries above which eight waves share a history
CHUNK = _ffi.FOLDIN_CHUNK  # entries of one wave's chunk of a long history


class FoldedIn(NamedTuple):
    """lgcn_foldin_rows' outputs for Q histories, on the device."""
    rows: torch.Tensor  # f32 [Q, d]: the folded-in rows, exact zeros for a history without eligible entries
    n: torch.Tensor     # int32 [Q]: eligible entries (those naming a table row) of each history


def inv_sqrt_degree(count: torch.Tensor, new_edge: bool = True) -> torch.Tensor:
    """f32 [M]: 1 / sqrt(count + new_edge), formed in float64 and rounded once; 0 where count +
    new_edge is 0, as gcn_norm has it. count: the table rows' degrees in the training graph (any
    integer or float dtype); new_edge counts the edge being folded in. Plain torch on count's device."""
    count = torch.as_tensor(count)
    if count.dim() != 1:
        raise ValueError(f"inv_sqrt_degree: count must be 1-D, got {tuple(count.shape)}")
    deg = count.to(torch.float64) + (1.0 if new_edge else 0.0)
    return torch.where(deg > 0, 1.0 / torch.sqrt(deg.clamp(min=0.0)), torch.zeros_like(deg)).to(torch.float32)


def fold_in_rows(history, table: torch.Tensor, isd: torch.Tensor | None = None,
                 weights: torch.Tensor | None = None) -> FoldedIn:
    """FoldedIn(rows f32 [Q, d], n int32 [Q]): for every history,
        rows[q] = 1 / sqrt(n_q) * sum_e (weights[e] * isd[i_e]) * table[i_e],
    lgcn_foldin_rows' rule (include/lgcn.h): entries outside [0, M) are skipped, a repeated entry
    counts each time, n_q = 0 gives a zero row.

    history: the CSR (ptr int64 [R + 1], idx int32) — one output row per CSR row — or
    (ptr, idx, rows) with rows[q] naming the CSR row of output q (checked by _serving.csr_arg); a row
    outside the CSR is an empty history. table [M, d] f32 on the device, d <= MAX_D: a column slice
    or a row-strided view of a wider tensor is read in place (only a view whose columns are not adjacent is copied). isd: f32
    [M], one factor per table row (inv_sqrt_degree); weights: f32, one per CSR entry; None: 1.
    The same history gives the same bits alone or in a batch, at any position, and run to run.
    ValueError / TypeError for bad arguments before anything is loaded."""
    ptr, hidx, hrow, Q = _serving.csr_arg("fold_in", "history", history)
    if not torch.is_tensor(table) or table.dim() != 2 or table.dtype != torch.float32:
        raise TypeError("fold_in: table must be a 2-D float32 tensor")
    M, d = table.shape
    if d < 1 or d > MAX_D:
        raise ValueError(f"fold_in: rows of {d} columns (1 to {MAX_D} are supported)")
    if isd is not None:
        if not torch.is_tensor(isd) or isd.dtype != torch.float32 or isd.dim() != 1:
            raise TypeError("fold_in: isd must be 1-D float32")
        if isd.numel() != M:
            raise ValueError(f"fold_in: {isd.numel()} isd factors for {M} table rows")
    _serving.check_weights("fold_in", weights, hidx.numel())
    lib = _ffi.load()
    for t in (table,) + tuple(x for x in (isd, weights) if x is not None):
        _ffi.require_device(t, "fold_in")
    dev = table.device
    out = torch.empty((Q, d), dtype=torch.float32, device=dev)
    out_n = torch.empty(Q, dtype=torch.int32, device=dev)
    if Q == 0 or hidx.numel() == 0 or M == 0:  # nothing to sum (and no device address to pass)
        return FoldedIn(out.zero_(), out_n.zero_())
    ptr, hidx, hrow = _serving.csr_on(dev, ptr, hidx, hrow)
    table, ldt = _serving.row_view(table.detach())
    isd = None if isd is None else isd.detach().contiguous()
    weights = None if weights is None else weights.detach().contiguous()
    _ffi.check(lib.lgcn_foldin_rows(ptr.data_ptr(), hidx.data_ptr(), _ffi.ptr(weights), _ffi.ptr(hrow), ptr.numel() - 1,
                                    Q, table.data_ptr(), M, d, ldt, _ffi.ptr(isd), out.data_ptr(), d, out_n.data_ptr(),
                                    _ffi.stream_of(dev)), "lgcn_foldin_rows")
    return FoldedIn(out, out_n)


def fold_in(history, table: torch.Tensor, count: torch.Tensor | None = None, weights: torch.Tensor | None = None,
            new_edge: bool = True) -> FoldedIn:
    """fold_in_rows with the table rows' training-graph degrees given as counts [M] (None: no degree
    factor): isd = inv_sqrt_degree(count, new_edge). new_edge=False folds a node in by the degrees as
    they are — with a training node's own history that is exactly one propagation layer of its row."""
    isd = None
    if count is not None:
        if not torch.is_tensor(table) or table.dim() != 2:
            raise TypeError("fold_in: table must be a 2-D float32 tensor")
        count = torch.as_tensor(count)
        if count.dim() != 1 or count.numel() != table.shape[0]:
            raise ValueError(f"fold_in: count {tuple(count.shape)} for {table.shape[0]} table rows")
        isd = inv_sqrt_degree(count, new_edge).to(table.device)
    return fold_in_rows(history, table, isd=isd, weights=weights)


def layer_tables(user_w: torch.Tensor, item_w: torch.Tensor, plan, K: int) -> tuple[torch.Tensor, torch.Tensor]:
    """(S_user [U, d], S_item [I, d]) = c * sum_{l < K} x(l), x(0) = cat(user_w, item_w) and x(l + 1) one
    propagation layer over ``plan`` (K - 1 lgconv_forward launches), c the layer-stack scaling
    lightgcn_propagate applies: (sum / (K + 1)) * fp32(1 / (K + 1)). A node folded in against S gets
    its final row under a K-layer model (module docstring). K = 0 leaves nothing to aggregate:
    ValueError."""
    K = int(K)
    if K < 1:
        raise ValueError(f"layer_tables: K={K} leaves no layer to aggregate (a 0-layer model has raw rows only)")
    for t, nm in ((user_w, "user_w"), (item_w, "item_w")):
        if not torch.is_tensor(t) or t.dim() != 2 or t.dtype != torch.float32:
            raise TypeError(f"layer_tables: {nm} must be a 2-D float32 tensor")
    if user_w.shape[1] != item_w.shape[1]:
        raise ValueError(f"layer_tables: embedding widths differ: {user_w.shape[1]} vs {item_w.shape[1]}")
    U, I = user_w.shape[0], item_w.shape[0]
    if U + I != plan.num_nodes:
        raise ValueError(f"layer_tables: plan was built for {plan.num_nodes} nodes, tables have {U + I}")
    from .propagate import lgconv_forward

    x = torch.cat([user_w.detach(), item_w.detach()])
    _ffi.require_device(x, "layer_tables")
    acc = x.clone()
    for _ in range(K - 1):
        x = lgconv_forward(x, plan)
        acc += x
    S = (acc / float(K + 1)) * float(np.float32(1.0 / (K + 1)))
    return S[:U], S[U:]
