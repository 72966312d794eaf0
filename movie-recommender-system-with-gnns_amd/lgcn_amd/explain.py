"""Why an item is on a served list: for every recommended slot, the items of the query's history
that point at it most strongly ("recommended because you watched X, Y, Z"), on the device
(lgcn_explain_topr in csrc/lgcn_explain.hip, one wave per query, the recommended rows in LDS, the
ragged history streamed once; no padded [Q, Lmax, D] gather exists at any point).

    explain_rows      rec_idx [Q, k] + a history CSR + the candidates' rows -> Explained
    explain_items     the user/item wrapper (history row of query q = users[q])
    history_weights   the gcn_norm weight of every history edge (plain torch)

Contribution of history item i to recommended item j: weights[e] * (Cn[i] . Cn[j]), Cn the unit rows
of ``candidates`` (a cosine) or, with normalized=True, the rows as given (a plain dot product). An
item is never a reason for itself. Ranking: contribution descending, then item index ascending; NaN
ranks as -inf. With history_weights, normalized=True and the raw item rows, ``total`` is the first
propagation layer's share of the user-item dot product.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import _ffi, _serving

MAX_K = _ffi.EXPLAIN_MAX_K  # recommended slots per query
MAX_R = _ffi.EXPLAIN_MAX_R  # reasons per slot


class Explained(NamedTuple):
    """lgcn_explain_topr's outputs for Q queries, k slots and r reasons, on the device."""
    idx: torch.Tensor    # [Q, k, r], rec_idx's dtype: history items by contribution, -1 in unfilled positions
    value: torch.Tensor  # f32 [Q, k, r]: their contributions, -inf in unfilled positions
    n: torch.Tensor      # int32 [Q, k]: filled positions, min(r, eligible history entries)
    total: torch.Tensor  # f32 [Q, k]: the sum of the contributions of ALL eligible history entries


def explain_rows(rec_idx: torch.Tensor, history, candidates: torch.Tensor, r: int = 3, weights=None,
                 normalized: bool = False) -> Explained:
    """For every slot of rec_idx [Q, k] (int32 or int64; topk_rows' or rerank_mmr's idx, possibly a
    column slice of a wider tensor; a value outside [0, M) is an empty slot), the r entries of the
    query's history row with the largest contribution to the slot's candidate: Explained(idx, value,
    n, total), lgcn_explain_topr's rule (module docstring).

    history: the CSR (ptr, idx) of recommend.seen_csr — row q belongs to query q — or
    (ptr, idx, rows) with rows[q] naming the CSR row of query q (checked by _serving.csr_arg); a row
    outside the CSR is an empty history, entries outside [0, M) are skipped. candidates [M, d] f32: normalised once here; with
    normalized=True taken as they are and only zero-padded to the kernel's width. weights: f32, one
    per CSR entry, on the device (None: 1).
    Limits: 1 <= k <= MAX_K, 1 <= r <= MAX_R, d <= 256 (ValueError before anything is loaded). The
    list for a smaller r is a prefix of the list for a larger one."""
    r = int(r)
    if rec_idx.dim() != 2:
        raise ValueError("explain: rec_idx must be [Q, k]")
    _serving.require_index_dtype("explain", "rec_idx", rec_idx)
    if candidates.dim() != 2 or candidates.dtype != torch.float32:
        raise TypeError("explain: candidates must be 2-D float32")
    Q, k = rec_idx.shape
    M, d = candidates.shape
    if k < 1 or k > MAX_K:
        raise ValueError(f"explain: k={k} recommended slots outside [1, {MAX_K}]")
    if r < 1 or r > MAX_R:
        raise ValueError(f"explain: r={r} outside [1, {MAX_R}]")
    D = _serving.width("explain", d)
    ptr, hidx, hrow, _ = _serving.csr_arg("explain", "history", history, Q)
    _serving.check_weights("explain", weights, hidx.numel())
    lib = _ffi.load()
    for t in (rec_idx, candidates) + (() if weights is None else (weights,)):
        _ffi.require_device(t, "explain")
    dev = rec_idx.device
    index_dtype = rec_idx.dtype
    out_idx = torch.full((Q, k, r), -1, dtype=torch.int32, device=dev)
    out_val = torch.full((Q, k, r), float("-inf"), dtype=torch.float32, device=dev)
    out_n = torch.zeros((Q, k), dtype=torch.int32, device=dev)
    out_sum = torch.zeros((Q, k), dtype=torch.float32, device=dev)
    if Q == 0 or hidx.numel() == 0:  # nothing to explain with (and no device address to pass)
        return Explained(out_idx.to(index_dtype), out_val, out_n, out_sum)
    ptr, hidx, hrow = _serving.csr_on(dev, ptr, hidx, hrow)
    if weights is not None:
        weights = weights.detach().contiguous()
    rec_idx, ld = _serving.index_list(rec_idx)
    s = _ffi.stream_of(dev)
    Cn = _serving.unit_rows(lib, candidates, D, normalized, s)
    _ffi.check(lib.lgcn_explain_topr(rec_idx.data_ptr(), ld, k, Q, ptr.data_ptr(), hidx.data_ptr(), _ffi.ptr(weights),
                                     _ffi.ptr(hrow), ptr.numel() - 1, Cn.data_ptr(), M, D, r, out_idx.data_ptr(),
                                     out_val.data_ptr(), out_n.data_ptr(), out_sum.data_ptr(), s), "lgcn_explain_topr")
    return Explained(out_idx.to(index_dtype), out_val, out_n, out_sum)


def explain_items(item_emb: torch.Tensor, users, rec_idx: torch.Tensor, seen, r: int = 3, weights=None) -> Explained:
    """explain_rows for users and items: rec_idx[q] is the list served to user users[q], seen the
    recommend.seen_csr(..., by="user") CSR over all users (row u is user u's history). The
    contributions are cosines between item rows (times ``weights``, one per entry of seen)."""
    users = torch.as_tensor(users).view(-1)
    return explain_rows(rec_idx, (seen[0], seen[1], users), item_emb, r=r, weights=weights)


def history_weights(seen) -> torch.Tensor:
    """f32, one per entry of the CSR seen = (ptr, idx): 1 / sqrt(len(row) * count(item)), the gcn_norm
    weight of the edge within the history graph (count(item) = the rows that hold the item). Plain
    torch on the CSR's device; CPU tensors work too."""
    ptr, idx = seen[0], seen[1]
    length = ptr[1:] - ptr[:-1]
    row = torch.repeat_interleave(torch.arange(length.numel(), device=ptr.device), length)
    i = idx.to(torch.int64)
    count = torch.bincount(i, minlength=1)
    return torch.rsqrt((length[row] * count[i]).to(torch.float64)).to(torch.float32)
