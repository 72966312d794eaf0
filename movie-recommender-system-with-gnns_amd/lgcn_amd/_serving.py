"""Argument handling shared by the serving modules (recommend, explain, foldin, metrics): one check
of a ragged-CSR argument, one int32 image of an index list, the kernels' padded row width, the
candidates' unit rows, and the per-entry weights check. ``who`` is the caller's message prefix
("recommend", "explain", "fold_in", "rank_metrics", "rank_positions"). Nothing here loads the library; moving tensors
to a device stays with the callers.
"""
from __future__ import annotations

import torch

from .recall import _normalize_into


def csr_arg(who: str, name: str, arg, Q: int | None = None, short: bool = False):
    """(ptr, idx, rows | None, Q) of the argument ``name`` = (ptr, idx) or (ptr, idx, rows), checked:
    ptr an int64 tensor [R + 1], idx an int32 1-D tensor as recommend.seen_csr builds them, rows
    (anything torch.as_tensor takes) integers, returned flattened.
    Q, the caller's query count: rows must name Q rows, and without rows the CSR must have a row per
    query unless ``short`` (the queries past its end then have empty rows). Q=None: the queries are
    the rows named, or every CSR row."""
    if arg is None or len(arg) not in (2, 3):
        raise ValueError(f"{who}: {name} is (ptr, idx) or (ptr, idx, rows)")
    ptr, idx = arg[0], arg[1]
    rows = arg[2] if len(arg) == 3 else None
    if not (torch.is_tensor(ptr) and torch.is_tensor(idx)) or ptr.dtype != torch.int64 or idx.dtype != torch.int32 \
            or ptr.dim() != 1 or idx.dim() != 1 or ptr.numel() < 1:
        raise TypeError(f"{who}: {name} needs ptr int64 [R + 1] and idx int32 (see recommend.seen_csr)")
    R = ptr.numel() - 1
    if rows is None:
        if Q is not None and R < Q and not short:
            raise ValueError(f"{who}: {name} has {R} rows for {Q} queries (pass the row of each query)")
        return ptr, idx, None, R if Q is None else Q
    rows = torch.as_tensor(rows).reshape(-1)
    if rows.dtype.is_floating_point or rows.dtype.is_complex or rows.dtype == torch.bool:
        raise TypeError(f"{who}: {name} rows must be integers, got {rows.dtype}")
    if Q is not None and rows.numel() != Q:
        raise ValueError(f"{who}: {name} rows has {rows.numel()} entries for {Q} queries")
    return ptr, idx, rows, rows.numel()


def row_view(t: torch.Tensor):
    """(t, ld) for the kernels' "row q starts at q * ld" reading of a [Q, k] tensor: a row-strided
    view with adjacent columns (a column slice of a wider tensor) is kept, anything else is copied."""
    Q, k = t.shape
    if t.stride(1) != 1 or t.stride(0) < k:
        t = t.contiguous()
    return t, (t.stride(0) if Q > 1 else k)  # a single row's stride means nothing


def index_list(t: torch.Tensor):
    """row_view of the int32 image of an int32 / int64 [Q, k] index list. A value outside int32 cannot
    name a row: it becomes -1 (skipped by every kernel), never wrapped; no host read."""
    if t.dtype == torch.int64:
        fits = (t >= 0) & (t <= torch.iinfo(torch.int32).max)
        t = torch.where(fits, t, -1).to(torch.int32)
    return row_view(t)


def require_index_dtype(who: str, name: str, t: torch.Tensor) -> None:
    if t.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"{who}: {name} must be int32 or int64, got {t.dtype}")


def width(who: str, d: int) -> int:
    """lgcn_recall_width's D for rows of d columns, formed on the host."""
    if d < 1 or d > 256:
        raise ValueError(f"{who}: rows of {d} columns (1 to 256 are supported)")
    D = 8
    while D < d:
        D <<= 1
    return D


def unit_rows(lib, candidates: torch.Tensor, D: int, normalized: bool, stream) -> torch.Tensor:
    """f32 [max(M, 1), D], 16-byte aligned: the rows of candidates [M, d] normalised (one
    lgcn_normalize_rows launch) or, with normalized=True, as they are, zero-padded to the kernel
    width D; candidates itself where that is already its layout."""
    candidates = candidates.detach()
    M, d = candidates.shape
    if normalized and d == D and candidates.is_contiguous() and candidates.data_ptr() % 16 == 0 and M > 0:
        return candidates
    Cn = torch.zeros((max(M, 1), D), dtype=torch.float32, device=candidates.device)
    if normalized:
        Cn[:M, :d] = candidates
    else:
        _normalize_into(lib, candidates, None, M, Cn.data_ptr(), D, M, stream)
    return Cn


def check_weights(who: str, weights, entries: int) -> None:
    """weights (None: every entry weighs 1) is one float32 per entry of the history's idx."""
    if weights is None:
        return
    if not torch.is_tensor(weights) or weights.dtype != torch.float32 or weights.dim() != 1:
        raise TypeError(f"{who}: weights must be 1-D float32")
    if weights.numel() != entries:
        raise ValueError(f"{who}: {weights.numel()} weights for {entries} history entries")
