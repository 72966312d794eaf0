"""What the serving modules (recall, recommend, explain, foldin, metrics) share on the host.

Arguments: one check of a ragged-CSR argument (csr_arg), one int32 image of an index list, the
per-entry weights check. ``who`` is the caller's message prefix ("recommend", "explain", "fold_in",
"rank_metrics", "rank_positions").
What the library is handed: the kernels' padded row width and query count (width, padded: the host
image of lgcn_recall_width), unit rows of candidates and of gathered queries (normalize_into,
unit_rows, unit_queries), a CSR argument on the device (csr_on) and its addresses for the queries
from some block start on (csr_at), row lengths as the kernels read them (row_lengths), and the
"longest row first" query order with its way back (longest_first, rows_in, in_caller_order).
Nothing here loads the library: ``lib`` is passed in.
"""
from __future__ import annotations

import torch

from . import _ffi

# the kernels take queries in groups of 128: lgcn_recall_width's second output
QUERY_MULTIPLE = 128


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


def row_lengths(ptr: torch.Tensor, rows, Q: int) -> torch.Tensor:
    """int64 [Q] on ptr's device: the length of each query's row of the CSR ptr (rows[q], or q); 0 for
    a row outside the CSR, as in the kernels (lgcn_ragged.h's ragged_row)."""
    R = ptr.numel() - 1
    if R == 0:
        return torch.zeros(Q, dtype=torch.int64, device=ptr.device)
    r = torch.arange(Q, device=ptr.device) if rows is None else rows.to(device=ptr.device, dtype=torch.int64)
    inside = (r >= 0) & (r < R)
    rc = r.clamp(0, R - 1)
    return torch.where(inside, ptr[rc + 1] - ptr[rc], torch.zeros_like(rc)).clamp(min=0)


def csr_on(dev, ptr: torch.Tensor, idx: torch.Tensor, rows):
    """(ptr, idx, rows int64 | None) of a checked CSR argument on ``dev``, contiguous. An empty idx
    comes back as one element: the library always wants an address. A caller for which an empty idx
    means "the argument is absent" decides that before it calls."""
    if idx.numel() == 0:
        idx = torch.zeros(1, dtype=torch.int32, device=dev)
    if rows is not None:
        rows = rows.to(device=dev, dtype=torch.int64).contiguous()
    return ptr.to(dev).contiguous(), idx.to(dev).contiguous(), rows


def csr_at(ptr, idx, rows, a: int):
    """(ptr address, idx address, rows address | None, row count): what the library takes for "this
    CSR argument, for the queries from ``a`` on". With rows, the rows array starts at query a; without,
    row q of the CSR is query q and the CSR itself starts at row a. An absent argument (ptr None) is
    (None, None, None, 0)."""
    if ptr is None:
        return None, None, None, 0
    R = ptr.numel() - 1
    if rows is not None:
        return ptr.data_ptr(), idx.data_ptr(), rows.data_ptr() + 8 * a, R
    return ptr.data_ptr() + 8 * a, idx.data_ptr(), None, R - a


def longest_first(lengths: torch.Tensor):
    """(lengths sorted descending, order): the stable order that takes queries longest row first."""
    return torch.sort(lengths, descending=True, stable=True)


def rows_in(order: torch.Tensor, rows):
    """The CSR row of each query taken in ``order`` (int64, contiguous): rows[order], or order itself
    where row q is query q's."""
    return order if rows is None else rows[order].contiguous()


def in_caller_order(order: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """The per-query tensor ``t`` of queries taken in ``order``, back in the caller's order."""
    out = torch.empty_like(t)
    out[order] = t
    return out


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


def padded(Q: int) -> int:
    """The query count the kernels are launched for: Q rounded up to QUERY_MULTIPLE, at least one group."""
    return max(QUERY_MULTIPLE, -(-Q // QUERY_MULTIPLE) * QUERY_MULTIPLE)


def normalize_into(lib, x: torch.Tensor, idx, rows: int, out_ptr: int, D: int, out_rows: int, stream):
    """lgcn_normalize_rows: unit rows of x (gathered by the int64 address idx, or rows 0 .. rows - 1) at
    out_ptr, zero-padded to width D and to out_rows rows."""
    if x.dim() != 2 or x.dtype != torch.float32 or x.stride(1) != 1:
        raise TypeError("recall: embeddings must be 2-D fp32 with unit column stride")
    _ffi.check(lib.lgcn_normalize_rows(x.data_ptr() if x.numel() else None, idx, rows, x.stride(0), x.shape[1],
                                       out_ptr, D, out_rows, stream), "lgcn_normalize_rows")


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
        normalize_into(lib, candidates, None, M, Cn.data_ptr(), D, M, stream)
    return Cn


def unit_queries(lib, queries: torch.Tensor, picked: torch.Tensor, D: int, out_rows: int, normalized: bool,
                 stream) -> torch.Tensor:
    """f32 [out_rows, D]: unit_rows' gathered counterpart. Row q is queries[picked[q]] (picked int64 on
    the device, contiguous) normalised (one lgcn_normalize_rows launch) or, with normalized=True, as it
    is, zero-padded to the kernel width D; the rows from picked.numel() on are zero either way."""
    queries = queries.detach()
    Q = picked.numel()
    if normalized:
        Qn = torch.zeros((out_rows, D), dtype=torch.float32, device=queries.device)
        Qn[:Q, :queries.shape[1]] = queries[picked]
    else:
        Qn = torch.empty((out_rows, D), dtype=torch.float32, device=queries.device)
        normalize_into(lib, queries, picked.data_ptr(), Q, Qn.data_ptr(), D, out_rows, stream)
    return Qn


def check_weights(who: str, weights, entries: int) -> None:
    """weights (None: every entry weighs 1) is one float32 per entry of the history's idx."""
    if weights is None:
        return
    if not torch.is_tensor(weights) or weights.dtype != torch.float32 or weights.dim() != 1:
        raise TypeError(f"{who}: weights must be 1-D float32")
    if weights.numel() != entries:
        raise ValueError(f"{who}: {weights.numel()} weights for {entries} history entries")
