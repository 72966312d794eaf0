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
    with attrs= / where= (an attribute filter per query: "ten comedies", "anything but horror") the
    ranked selections are lgcn_select_topk_ranked_attr and the lists lgcn_score_filter_attr's, which
    test a candidate's attribute word where they test its score: a list only ever holds candidates
    that pass, so a filter that passes 0.5 % of the items costs no capacity.

    with among= (a candidate set per query, as a CSR: "rank these and only these" — a watchlist, a
    retrieval stage's output, one held-out item among 99 sampled negatives) no filter runs at all:
      queries longest row first, in blocks of capacity max(k, the block's longest row):
                 lists = the row's keys  lgcn_score_lists (csrc/lgcn_recall_among.hip; cost: Σ row lengths)
                 ranked emit             lgcn_select_topk_ranked[_attr]
    and the list is the query's full ranking restricted to its row, bit for bit.

    with boost= (one f32 per candidate: "show less of what everybody has seen", a lift for new releases,
    a second model's item bias; popularity_boost makes the first from interaction counts) every call
    above that forms a key is its _boost twin — lgcn_score_filter_boost for the dense rows, the subset
    and the lists (with the attribute filter or without), lgcn_score_lists_boost for among — and the key
    of a pair is that of score + boost[j], one f32 addition (csrc/lgcn_recall_boost.hip). The thresholds,
    the tightening and the ranked selection read keys and run as they are, so a strongly boosted
    candidate is found wherever it stood in the unboosted ranking; the returned score is the boosted one.

    topk_groups (one list for several query rows: "what do the four of us watch tonight?") runs the same
    dense / filtered blocks with a "query" meaning a group of S member rows (S = 2 .. 32, one plan per size
    class): lgcn_score_filter_groups (csrc/lgcn_recall_group.hip) reduces a candidate's member scores
    to ONE key — the minimum (least misery), the maximum (most pleasure) or the mean, with an optional
    floor no member's score may lie under — before anything is tested or listed, so the lists, the
    thresholds, the exclusion rows and the ranked selection are the group's.

On the host topk_rows is one prepared plan and three block strategies. It checks every argument
before the library is loaded, then builds a _Plan: the query order (the caller's, or the among
sort), Qn and Cn, the output buffers, the exclusion CSR and the attribute table on the device, and
the only two places that choose between a kernel and its _attr or _boost twin (_Plan.filter,
_Plan.select).
_run_dense, _run_filtered and _run_among are the three blocks of the table above, written over the
plan; _Plan.finish puts the lists back in the caller's order and gives them their index dtype. The
pieces that other modules need too (row lengths, a CSR argument's device tensors and block
addresses, unit rows, the padded sizes, the longest-first order) live in _serving.

Ranking rule: score descending, then candidate index ascending (NaN scores first). The threshold
is formed from eligible subset entries only: it is then the k-th best of a subset of the eligible
candidates, so it is a lower bound of the k-th best eligible score of all M, and the filtered list
holds the whole eligible top k whatever was excluded.

Diversity on top of relevance (csrc/lgcn_rerank.hip, one wave per query, the pool's rows in LDS):
    rerank_mmr            greedy Maximal Marginal Relevance over per-query pools   lgcn_rerank_mmr
    topk_rows_diverse     topk_rows for a pool, then rerank_mmr down to k
    intra_list_diversity  ILD@c from rerank_mmr's pair sums (plain torch)

Calibration on top of relevance (csrc/lgcn_calibrate.hip; Steck, RecSys 2018): lists that keep the
genre mix of the user's own history, genres being the bits of the attribute words of ``attrs=``.
    attr_profile          a history CSR -> the target distribution p [Q, 32]      lgcn_attr_profile
    rerank_calibrated     greedy (1 - l) * relevance - l * KL(p || list) picks    lgcn_rerank_calibrated
    topk_rows_calibrated  topk_rows for a pool, then rerank_calibrated down to k
    miscalibration        C_KL@c from rerank_calibrated's KL column (plain torch)
"""
from __future__ import annotations

import operator
from typing import NamedTuple

import torch

from . import _ffi, _serving

# list workspace of one query block (8 bytes per list slot: key + index); follows recall.STL_BLOCK_BYTES
BLOCK_BYTES = 1 << 30
# per-query list capacity of the filtered path, and the largest M the dense path takes
CAP = 16384
# candidates scored for the first thresholds: max(SUBSET_MIN, SUBSET_PER_K * k), at most the capacity
# (about k * M / subset entries survive the filter)
SUBSET_MIN = 2048
SUBSET_PER_K = 16
MAX_K = _ffi.RANKED_MAX_K
# the re-rank kernel's pool: entries per query, and bytes of pool rows (N * D * 4) it stages in LDS
MMR_MAX_POOL = _ffi.MMR_MAX_POOL
MMR_MAX_LDS_BYTES = _ffi.MMR_MAX_LDS_BYTES
# the calibrated re-rank: genres (bits of an attribute word) and pool entries per query
CALIB_GENRES = _ffi.CALIB_GENRES
CALIB_MAX_POOL = _ffi.CALIB_MAX_POOL


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


def attr_bits(labels, vocabulary) -> torch.Tensor:
    """The attribute words of ``attrs=``: int32 [rows] on the CPU, bit b of row r set when
    ``vocabulary[b]`` is among ``labels[r]`` (a collection of labels per row; an empty one gives 0).
    At most 32 labels (bit 31 is the int32's sign bit); a label outside the vocabulary is a
    ValueError naming it."""
    vocabulary = list(vocabulary)
    if len(vocabulary) > 32:
        raise ValueError(f"attr_bits: {len(vocabulary)} labels, an attribute word holds 32")
    bit = {v: b for b, v in enumerate(vocabulary)}
    if len(bit) != len(vocabulary):
        raise ValueError("attr_bits: the vocabulary names a label twice")
    words = []
    for r, row in enumerate(labels):
        w = 0
        for label in row:
            if label not in bit:
                raise ValueError(f"attr_bits: row {r} carries {label!r}, which is not in the vocabulary {vocabulary}")
            w |= 1 << bit[label]
        words.append(w - (1 << 32) if w >= 1 << 31 else w)
    return torch.tensor(words, dtype=torch.int32)


def _mask_column(name: str, m, Q: int) -> torch.Tensor:
    """One member of ``where`` as int64 [Q] or [1] values in [-2**31, 2**31): ints of [0, 2**32) are
    taken as the uint32 bit pattern."""
    if m is None:
        m = 0
    if isinstance(m, bool) or (isinstance(m, torch.Tensor) and (m.dtype == torch.bool or m.is_floating_point()
                                                                 or m.is_complex())):
        raise TypeError(f"recommend: where's {name} mask must be an int or integers, got {m!r}")
    if isinstance(m, int):
        if not -(1 << 31) <= m < 1 << 32:
            raise ValueError(f"recommend: where's {name} mask {m} is outside 32 bits")
        t = torch.tensor([m], dtype=torch.int64)
    elif isinstance(m, torch.Tensor) and m.dtype in (torch.int32, torch.int16, torch.int8, torch.uint8):
        if m.numel() != Q:
            raise ValueError(f"recommend: where's {name} mask has {m.numel()} entries for {Q} queries")
        return m.detach().to(torch.int64).reshape(-1)  # in range as it is: nothing to read back
    else:
        try:
            t = m.detach().to(torch.int64).reshape(-1) if isinstance(m, torch.Tensor) else \
                torch.tensor([operator.index(x) for x in m], dtype=torch.int64)
        except (TypeError, ValueError, RuntimeError, OverflowError) as e:
            raise TypeError(f"recommend: where's {name} mask must be an int or integers ({e})") from None
        if t.numel() != Q:
            raise ValueError(f"recommend: where's {name} mask has {t.numel()} entries for {Q} queries")
    if t.numel() and (int(t.min()) < -(1 << 31) or int(t.max()) >= 1 << 32):
        raise ValueError(f"recommend: where's {name} mask has a value outside 32 bits")
    return torch.where(t >= 1 << 31, t - (1 << 32), t)


def _where_arg(attrs, where, M: int, Q: int):
    """topk_rows' filter arguments, checked: None without a filter, else the int32 [Q, 3] table of
    (any, all, none) rows, on the device of whichever mask was a device tensor (the CPU otherwise)."""
    if attrs is None and where is None:
        return None
    if attrs is None:
        raise ValueError("recommend: where needs attrs (the candidates' attribute words)")
    if where is None:
        raise ValueError("recommend: attrs needs where=(any, all, none)")
    if not isinstance(attrs, torch.Tensor) or attrs.dtype != torch.int32 or attrs.dim() != 1:
        raise TypeError("recommend: attrs must be an int32 tensor [M]")
    if attrs.numel() != M:
        raise ValueError(f"recommend: attrs has {attrs.numel()} entries for {M} candidates")
    if isinstance(where, (str, bytes, torch.Tensor)) or not hasattr(where, "__len__") or len(where) != 3:
        raise ValueError("recommend: where is (any, all, none)")
    cols = [_mask_column(n, m, Q) for n, m in zip(("any", "all", "none"), where)]
    dev = next((c.device for c in cols if c.is_cuda), torch.device("cpu"))
    return torch.stack([c.to(dev).expand(Q) for c in cols], 1).to(torch.int32)


def _boost_arg(boost, M: int, device) -> None:
    """topk_rows' boost, checked (nothing is read): None, or a float32 tensor [M] on ``device``."""
    if boost is None:
        return
    if not isinstance(boost, torch.Tensor) or boost.dtype != torch.float32:
        raise ValueError(f"recommend: boost must be a float32 tensor [M], got "
                         f"{boost.dtype if isinstance(boost, torch.Tensor) else type(boost).__name__}")
    if boost.dim() != 1 or boost.numel() != M:
        raise ValueError(f"recommend: boost has shape {tuple(boost.shape)} for {M} candidates, not [{M}]")
    if boost.device != device:
        raise ValueError(f"recommend: boost is on {boost.device}, the queries on {device}")


def popularity_boost(counts: torch.Tensor, strength: float) -> torch.Tensor:
    """A popularity penalty for topk_rows' boost=: float32 [M] on counts' device,
    -strength * log1p(counts) / log1p(counts.max()), formed in float64 and rounded once. It is 0 for
    an item nobody has touched and -strength for the most popular one, the logarithm in between (the
    counts of a catalogue span orders of magnitude). strength is on the cosine's scale, [-1, 1]: 0.2
    takes a fifth of the score range off the most popular item; a negative strength lifts popular
    items instead. counts: interaction counts per item, any real dtype, non-negative (the lengths of
    seen_csr(..., by="item") rows). An all-zero counts gives zeros. Plain torch ops; nothing is read on
    the host."""
    if not isinstance(counts, torch.Tensor) or counts.dim() != 1 or counts.dtype == torch.bool or counts.is_complex():
        raise TypeError("popularity_boost: counts must be a 1-D tensor of counts")
    strength = float(strength)
    if strength != strength:
        raise ValueError("popularity_boost: strength is NaN")
    if counts.numel() == 0:
        return torch.zeros(0, dtype=torch.float32, device=counts.device)
    logs = torch.log1p(counts.detach().to(torch.float64))
    top = logs.max()
    share = torch.where(top > 0, logs / top.clamp(min=torch.finfo(torch.float64).tiny), torch.zeros_like(logs))
    return (-strength * share).to(torch.float32)


def candidate_csr(lists, device=None):
    """The ``among=`` CSR of per-query candidate lists: (ptr int64 [Q + 1], idx int32), row q holding
    query q's candidate indices ascending and deduplicated. lists: a sequence of integer sequences
    (or 1-D tensors), or an integer tensor [Q, N] whose negative entries are padding; negative
    entries are dropped, an empty row stays an empty row. Plain torch ops, on ``device`` (default:
    the tensor's own, the CPU for sequences)."""
    if torch.is_tensor(lists):
        if lists.dim() != 2 or lists.dtype.is_floating_point or lists.dtype.is_complex or lists.dtype == torch.bool:
            raise TypeError("candidate_csr: a tensor of lists must be an integer tensor [Q, N]")
        t = lists.detach().to(torch.int64)
        if device is not None:
            t = t.to(device)
        Q = t.shape[0]
        rows = torch.arange(Q, device=t.device).repeat_interleave(t.shape[1])
        cols = t.reshape(-1)
    else:
        lists = [torch.as_tensor(r).reshape(-1) for r in lists]
        for r in lists:
            if r.numel() and (r.dtype.is_floating_point or r.dtype.is_complex or r.dtype == torch.bool):
                raise TypeError(f"candidate_csr: candidate indices must be integers, got {r.dtype}")
        dev = torch.device("cpu") if device is None else torch.device(device)
        Q = len(lists)
        lens = torch.tensor([r.numel() for r in lists], dtype=torch.int64)
        rows = torch.arange(Q).repeat_interleave(lens).to(dev)
        cols = torch.cat([r.to(device=dev, dtype=torch.int64) for r in lists] + [torch.zeros(0, dtype=torch.int64, device=dev)])
    keep = cols >= 0
    rows, cols = rows[keep], cols[keep]
    if cols.numel() and int(cols.max()) > torch.iinfo(torch.int32).max:
        raise ValueError("candidate_csr: a candidate index does not fit int32")
    C = int(cols.max()) + 1 if cols.numel() else 1
    key = torch.unique(rows * C + cols, sorted=True)
    ptr = torch.zeros(Q + 1, dtype=torch.int64, device=cols.device)
    if Q > 0:
        ptr[1:] = torch.cumsum(torch.bincount(key // C, minlength=Q), 0)
    return ptr, (key % C).to(torch.int32)


def group_csr(groups, device=None):
    """The groups of topk_groups as a CSR: (ptr int64 [G + 1], idx int32), row g holding group g's
    member indices (rows of the query table) in the order given — the order is the association of
    the "average" strategy's sum — and as often as given: a member named twice counts twice. groups: a
    sequence of integer sequences (or 1-D tensors), or an integer tensor [G, N] whose negative
    entries are padding; negative entries are dropped, an empty row stays an empty group. Plain torch
    ops, on ``device`` (default: the tensor's own, the CPU for sequences)."""
    if torch.is_tensor(groups):
        if groups.dim() != 2 or groups.dtype.is_floating_point or groups.dtype.is_complex or groups.dtype == torch.bool:
            raise TypeError("group_csr: a tensor of groups must be an integer tensor [G, N]")
        t = groups.detach().to(torch.int64)
        if device is not None:
            t = t.to(device)
        keep = t >= 0
        lens, cols = keep.sum(1), t[keep]  # boolean indexing walks row by row: member order is kept
    else:
        rows = [torch.as_tensor(r).reshape(-1) for r in groups]
        for r in rows:
            if r.numel() and (r.dtype.is_floating_point or r.dtype.is_complex or r.dtype == torch.bool):
                raise TypeError(f"group_csr: member indices must be integers, got {r.dtype}")
        dev = torch.device("cpu") if device is None else torch.device(device)
        rows = [r.to(torch.int64) for r in rows]
        rows = [r[r >= 0] for r in rows]
        lens = torch.tensor([r.numel() for r in rows], dtype=torch.int64, device=dev)
        cols = torch.cat(rows + [torch.zeros(0, dtype=torch.int64)]).to(dev)
    if cols.numel() and int(cols.max()) > torch.iinfo(torch.int32).max:
        raise ValueError("group_csr: a member index does not fit int32")
    ptr = torch.zeros(lens.numel() + 1, dtype=torch.int64, device=cols.device)
    ptr[1:] = torch.cumsum(lens, 0)
    return ptr, cols.to(torch.int32)


def _groups_arg(groups, device=None):
    """(ptr, idx) of a groups argument: group_csr's own output (ptr int64, idx int32) as it is, anything
    else through group_csr."""
    if isinstance(groups, tuple) and len(groups) == 2 and all(torch.is_tensor(t) and t.dim() == 1 for t in groups) \
            and groups[0].dtype == torch.int64 and groups[1].dtype == torch.int32 and groups[0].numel() >= 1:
        return groups if device is None else (groups[0].to(device), groups[1].to(device))
    return group_csr(groups, device=device)


def group_seen_csr(seen, groups, by: str = "any"):
    """The exclusion CSR of groups from the users' seen CSR: (ptr int64 [G + 1], idx int32), row g
    holding what group g has seen, ascending and deduplicated — by="any": the union of its members'
    rows (nobody is served something they know), by="all": their intersection (only what everybody
    knows is left out). seen: seen_csr(..., by="user"), row u being user u's; groups: group_csr's
    output, or what it takes. A member named twice counts once here; a member with an empty row
    empties the intersection, and an empty group has an empty row under both. A member outside the
    seen CSR's rows is a ValueError. Plain torch ops on seen's device: plumbing, not the hot path."""
    if by not in ("any", "all"):
        raise ValueError(f"group_seen_csr: by must be 'any' or 'all', got {by!r}")
    sptr, sidx = _serving.csr_arg("group_seen_csr", "seen", seen)[:2]
    dev = sptr.device
    gptr, gidx = _groups_arg(groups, device=dev)
    G, U = gptr.numel() - 1, sptr.numel() - 1
    mem = gidx.to(torch.int64)
    if mem.numel() and (int(mem.min()) < 0 or int(mem.max()) >= U):
        raise ValueError(f"group_seen_csr: a member index lies outside the seen CSR's {U} rows")
    grp = torch.repeat_interleave(torch.arange(G, device=dev), gptr[1:] - gptr[:-1])
    pair = torch.unique(grp * max(U, 1) + mem, sorted=True)  # each (group, member) once
    grp, mem = pair // max(U, 1), pair % max(U, 1)
    n = sptr[mem + 1] - sptr[mem]
    row = torch.repeat_interleave(torch.arange(pair.numel(), device=dev), n)
    at = sptr[mem][row] + torch.arange(row.numel(), device=dev) - (torch.cumsum(n, 0) - n)[row]
    items = sidx[at].to(torch.int64)
    C = int(items.max()) + 1 if items.numel() else 1
    key, count = torch.unique(grp[row] * C + items, sorted=True, return_counts=True)
    if by == "all":  # seen rows are deduplicated: the count is the number of members that have the item
        key = key[count == torch.bincount(grp, minlength=G)[key // C]]
    ptr = torch.zeros(G + 1, dtype=torch.int64, device=dev)
    if G > 0:
        ptr[1:] = torch.cumsum(torch.bincount(key // C, minlength=G), 0)
    return ptr, (key % C).to(torch.int32)


class _Group(NamedTuple):
    """_Plan's group mode: S member rows per group, the aggregate (_ffi.GROUP_*), the groups' sizes
    (int32 on the device) and their floors (f32 on the device, or None)."""
    S: int
    agg: int
    size: torch.Tensor
    floor: torch.Tensor | None


def _among_blocks(lengths, k: int, block_bytes: int):
    """[(a, b, capacity)] over queries sorted longest row first (lengths: the sorted row lengths, a
    host sequence): a block's capacity is max(k, its longest row = its first) and it holds at most
    block_bytes // (8 * capacity) queries, at least one."""
    blocks, a, Q = [], 0, len(lengths)
    while a < Q:
        cap = max(k, int(lengths[a]))
        b = min(Q, a + max(1, block_bytes // (8 * cap)))
        blocks.append((a, b, cap))
        a = b
    return blocks


class _Plan:
    """One topk_rows call, prepared for whichever block strategy runs it: the library, stream and
    device; D, M, k, Q and the query order (None: the caller's; else the among sort, every per-query
    array below being in that order); the unit rows Qn [Qpad, D] and Cn (one normalize each); the
    output buffers [Qpad, k]; the exclusion CSR on the device (eptr None: nothing is excluded, which an
    empty idx means too); the attribute words and the mask table (wh None: no filter). A strategy
    brings the list buffers (lists) and issues the two calls a block is made of: filter and select.
    Group mode (group: a _Group; topk_groups): a "query" is a group of S member rows. picked then holds
    S member rows per group, Qn is [Qpad * S, D], Q and Qpad count groups (Qpad a multiple of
    128 // S), and filter calls lgcn_score_filter_groups; lists, thresholds, the exclusion rows, the
    mask table and the outputs are per group, and select and the strategies run as they are."""

    def __init__(self, lib, queries, picked, candidates, k: int, D: int, Qpad: int, excl, masks, attrs, order=None,
                 group=None, Cn=None, boost=None):
        dev = queries.device
        self.lib, self.dev, self.s = lib, dev, _ffi.stream_of(dev)
        self.group, self.rows = group, 1 if group is None else group.S  # member rows per query
        self.boost = None if boost is None else boost.detach().contiguous()  # f32 [M]: filter's and _run_among's
        self.qmul = _serving.QUERY_MULTIPLE // self.rows
        self.k, self.D, self.Qpad, self.M, self.order = k, D, Qpad, candidates.shape[0], order
        self.Q = picked.numel() // self.rows
        Q, M = self.Q, self.M
        self.eptr = self.eidx = self.erow = None
        if excl is not None and excl[1].numel():  # an empty idx: nothing to exclude anywhere
            self.eptr, self.eidx, self.erow = _serving.csr_on(dev, *excl)
        if order is not None:
            picked = picked[order].contiguous()
            if self.eptr is not None:
                self.erow = _serving.rows_in(order, self.erow)
        self.Qn = _serving.unit_queries(lib, queries, picked, D, Qpad * self.rows, False, self.s)
        self.Cn = Cn  # an earlier plan's, over the same candidates (topk_groups: one plan per size class)
        if Cn is None:
            self.Cn = torch.empty((max(M, 1), D), dtype=torch.float32, device=dev)
            _serving.normalize_into(lib, candidates.detach(), None, M, self.Cn.data_ptr(), D, M, self.s)
        self.out_idx = torch.empty((Qpad, k), dtype=torch.int32, device=dev)
        self.out_score = torch.empty((Qpad, k), dtype=torch.float32, device=dev)
        self.out_n = torch.empty(Qpad, dtype=torch.int32, device=dev)
        self.wh = self.attrs = None
        if masks is not None:  # the kernels' [Qpad, 3] table (padding queries' rows are never read) and attribute words
            if order is not None:
                self.wh = masks.to(dev)[order].contiguous()
            else:
                self.wh = torch.zeros((Qpad, 3), dtype=torch.int32, device=dev)
                self.wh[:Q] = masks.to(dev)
            self.attrs = attrs.detach().contiguous()

    def lists(self, slots: int) -> None:
        """The list workspace (key + index per slot) that filter fills and select reads."""
        self.lkey = torch.empty(slots, dtype=torch.int32, device=self.dev)
        self.lidx = torch.empty(slots, dtype=torch.int32, device=self.dev)

    def blocks(self, cap: int) -> list:
        """[(q0, nb, qv)] of the padded queries in blocks of at most BLOCK_BYTES of list workspace at
        ``cap`` slots per query (nb queries from q0 on, the first qv of them real), and that workspace."""
        qmul, Qpad = self.qmul, self.Qpad
        blk = min(Qpad, max(qmul, (BLOCK_BYTES // (8 * cap)) // qmul * qmul))
        self.lists(blk * cap)
        if self.group is not None and self.group.floor is not None:  # dense rows become lists: see filter
            self.fthr = torch.zeros(blk, dtype=torch.int32, device=self.dev)
            self.fcnt = torch.zeros(blk, dtype=torch.int32, device=self.dev)
        # Q >= 1 and Qpad - Q < qmul (128 for queries), while a block starts at a multiple of qmul below
        # Qpad (or at 0): q0 <= Qpad - qmul < Q, so every block holds a real query (qv >= 1)
        return [(q0, min(blk, Qpad - q0), min(blk, self.Q - q0)) for q0 in range(0, Qpad, blk)]

    def filter(self, q0: int, nb: int, qv: int, n: int, stride: int, cap: int, what: str, thr=None, counts=None) -> None:
        """Score the block's queries against n candidates ``stride`` apart into the lists: every score
        in candidate order (thr None), or the scores at or above the thresholds, counted; under an
        attribute filter only candidates that pass enter a thresholded list. With a boost every one of
        these passes is lgcn_score_filter_boost's (labelled as ``what`` with the _boost name).
        Group mode: the group keys of lgcn_score_filter_groups. It does not know the attribute predicate
        (select alone applies it), and under a floor "every score" is a list under zero thresholds,
        counted in fcnt, which select then reads in place of dense rows: a dense row cannot say that a
        candidate fell under the floor."""
        if self.group is not None:
            g = self.group
            floor = None
            if g.floor is not None:
                floor = g.floor.data_ptr() + q0 * 4
                if thr is None:
                    self.fcnt.zero_()
                    thr, counts = self.fthr.data_ptr(), self.fcnt.data_ptr()
            _ffi.check(self.lib.lgcn_score_filter_groups(
                self.Qn.data_ptr() + q0 * g.S * self.D * 4, nb, qv, g.S, g.size.data_ptr() + q0 * 4, g.agg, floor,
                self.Cn.data_ptr(), n, stride, self.D, thr, self.lkey.data_ptr(), self.lidx.data_ptr(), counts, cap,
                self.s), "lgcn_score_filter_groups")
            return
        qptr = self.Qn.data_ptr() + q0 * self.D * 4
        args = (qptr, nb, qv, self.Cn.data_ptr(), n, stride, self.D, thr, self.lkey.data_ptr(), self.lidx.data_ptr(),
                counts, cap)
        if self.boost is not None:  # every pass forms boosted keys; dense rows take no attribute filter
            wh = (None, None) if thr is None or self.wh is None else (self.attrs.data_ptr(), self.wh.data_ptr() + q0 * 12)
            _ffi.check(self.lib.lgcn_score_filter_boost(*args, *wh, self.boost.data_ptr(), self.s),
                       what.replace("lgcn_score_filter", "lgcn_score_filter_boost"))
        elif thr is None or self.wh is None:
            _ffi.check(self.lib.lgcn_score_filter(*args, self.s), what)
        else:
            _ffi.check(self.lib.lgcn_score_filter_attr(*args, self.attrs.data_ptr(), self.wh.data_ptr() + q0 * 12, self.s),
                       "lgcn_score_filter_attr")

    def select(self, q0: int, nb: int, qv: int, counts, dense_n: int, cap: int, thr_out=None, emit: bool = False) -> None:
        """The ranked selection over the block's lists (counts: their lengths; None: dense rows of
        dense_n), eligible entries only: the k-th best key into thr_out, or the ranked lists into the
        outputs' rows from q0 on (emit)."""
        k = self.k
        if counts is None and self.group is not None and self.group.floor is not None:
            counts, dense_n = self.fcnt.data_ptr(), 0  # filter's lists under zero thresholds
        ex = _serving.csr_at(self.eptr, self.eidx, self.erow, q0)
        outs = (self.out_idx.data_ptr() + q0 * k * 4, self.out_score.data_ptr() + q0 * k * 4,
                self.out_n.data_ptr() + q0 * 4) if emit else (None, None, None)
        args = (self.lkey.data_ptr(), self.lidx.data_ptr(), counts, dense_n, cap, k, nb, qv, *ex, thr_out, *outs)
        if self.wh is None:
            _ffi.check(self.lib.lgcn_select_topk_ranked(*args, self.s), "lgcn_select_topk_ranked")
        else:
            _ffi.check(self.lib.lgcn_select_topk_ranked_attr(*args, self.attrs.data_ptr(), self.wh.data_ptr() + q0 * 12,
                                                             self.s), "lgcn_select_topk_ranked_attr")

    def finish(self, index_dtype):
        """(idx, score) of the Q real queries, in the caller's order."""
        idx, score = self.out_idx[:self.Q], self.out_score[:self.Q]
        if self.order is None:
            score = score.clone()
        else:
            idx, score = _serving.in_caller_order(self.order, idx), _serving.in_caller_order(self.order, score)
        return (idx.to(torch.int64) if index_dtype == torch.int64 else idx), score


def _run_dense(plan: _Plan) -> None:
    """M <= cap: every score of a block, then the ranked emit. No host read."""
    M, cap = plan.M, max(plan.M, plan.k)  # a dense row needs M slots
    for q0, nb, qv in plan.blocks(cap):
        plan.filter(q0, nb, qv, M, 1, cap, "lgcn_score_filter(dense)")
        plan.select(q0, nb, qv, None, M, cap, emit=True)


def _run_filtered(plan: _Plan, cap: int, subset: int) -> None:
    """M > cap: first thresholds from a strided subset, then lists of the scores at or above them,
    tightened while a list overflows (at most 8 rounds). One host read per block and round."""
    M, k, dev = plan.M, plan.k, plan.dev
    stride = max(1, -(-M // min(subset, cap)))
    S = -(-M // stride)
    blocks = plan.blocks(cap)
    lcnt = torch.zeros(blocks[0][1], dtype=torch.int32, device=dev)
    thr = torch.empty(blocks[0][1], dtype=torch.int32, device=dev)
    # a row outside the CSR excludes nothing, as in the kernel
    taken = None if plan.eptr is None else _serving.row_lengths(plan.eptr, plan.erow, plan.Q)
    for q0, nb, qv in blocks:
        # eligible candidates of the block's poorest query, read with the first overflow check
        fewest = torch.full((), M, dtype=torch.int64, device=dev) if taken is None else M - taken[q0:q0 + qv].max()
        # first thresholds: the k-th best eligible entry of a strided subset
        plan.filter(q0, nb, qv, S, stride, cap, "lgcn_score_filter(subset)")
        plan.select(q0, nb, qv, None, S, cap, thr_out=thr.data_ptr())
        for _ in range(8):
            lcnt.zero_()
            plan.filter(q0, nb, qv, M, 1, cap, "lgcn_score_filter", thr=thr.data_ptr(), counts=lcnt.data_ptr())
            longest, few = torch.stack([lcnt[:qv].max().to(torch.int64), fewest]).tolist()  # the block's host read
            if few < k:
                raise ValueError(f"recommend: a query has {few} eligible candidates, fewer than k={k} "
                                 f"(M={M} is above the dense capacity {cap}, which pads such rows)")
            if longest <= cap:
                plan.select(q0, nb, qv, lcnt.data_ptr(), 0, cap, emit=True)
                break
            # a list overflowed: its kept entries are real candidates, so the k-th best eligible one
            # among them is a valid, tighter threshold; filter again
            plan.select(q0, nb, qv, lcnt.data_ptr(), 0, cap, thr_out=thr.data_ptr())
        else:
            raise RuntimeError("recommend: candidate lists kept overflowing (scores too concentrated for the capacity"
                               + ("" if plan.wh is None else f", or more than cap={cap} candidates pass the filter of a "
                                                             f"query that cannot fill k={k}") + ")")


def _run_among(plan: _Plan, among, blocks) -> None:
    """Each query's own row as its list (queries longest row first, ``blocks`` of _among_blocks), then
    the ranked emit; unpadded (Qpad == nb). No filter runs and nothing is read on the host here."""
    aptr, aidx, arow = _serving.csr_on(plan.dev, *among)
    arow = _serving.rows_in(plan.order, arow)
    lcnt = torch.empty(plan.Q, dtype=torch.int32, device=plan.dev)
    plan.lists(max((b - a) * cap for a, b, cap in blocks))  # one pair of list buffers serves every block
    for a, b, cap in blocks:
        counts = lcnt.data_ptr() + a * 4
        args = (plan.Qn.data_ptr() + a * plan.D * 4, b - a, plan.Cn.data_ptr(), plan.M, plan.D,
                *_serving.csr_at(aptr, aidx, arow, a), plan.lkey.data_ptr(), plan.lidx.data_ptr(), counts, cap)
        if plan.boost is None:
            _ffi.check(plan.lib.lgcn_score_lists(*args, plan.s), "lgcn_score_lists")
        else:
            _ffi.check(plan.lib.lgcn_score_lists_boost(*args, plan.boost.data_ptr(), plan.s), "lgcn_score_lists_boost")
        plan.select(a, b - a, b - a, counts, _ffi.RANKED_REPEATS, cap, emit=True)


def topk_rows(queries: torch.Tensor, picked: torch.Tensor, candidates: torch.Tensor, k: int, excl=None,
              cap: int | None = None, subset: int | None = None, index_dtype: torch.dtype = torch.int64,
              attrs: torch.Tensor | None = None, where=None, among=None, boost: torch.Tensor | None = None):
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
    first Q rows of this call's padded buffer, which lives as long as the view does.
    attrs / where: an attribute filter, tested on the device where the score is tested (both or
    neither). attrs is int32 [M] on the device, one 32-bit attribute word per candidate (attr_bits
    makes them from labels); where is (any, all, none), each member an int — [0, 2**32) is taken as
    the bit pattern, bit 31 being the int32's sign — or an integer tensor / sequence with one mask
    per query, None for 0. Candidate j passes for query q when attrs[j] & none == 0,
    attrs[j] & all == all and (any == 0 or attrs[j] & any != 0); only candidates that pass and are
    not excluded are ranked. Under a filter a query short of k eligible candidates is padded with
    -1 / -inf above ``cap`` too, as long as the candidates that pass for it fit ``cap`` (RuntimeError
    otherwise); the ValueError above is left for M minus the excluded falling below k. topk_items,
    topk_users, topk_rows_diverse and metrics.evaluate_ranking hand both on.
    among: None, or a candidate set per query as a CSR, (ptr, idx) — row q is query q's — or
    (ptr, idx, rows) with rows[q] naming the CSR row of query q (candidate_csr builds one): query q
    ranks only the entries of its row that lie in [0, M), are not in its excl row and pass ``where``,
    by the same rule on the same keys, so its list is its full ranking restricted to the row, bit for
    bit. Entries may come in any order; an entry named twice is ranked twice (two adjacent slots of
    the list: pass candidate_csr's deduplicated rows to avoid it), an entry outside [0, M) names
    nothing. A query with fewer than k such entries is padded with -1 / -inf; a missing or empty row
    gives an all-padding list, never an error. The cost follows the sum of the row lengths, not M:
    the candidates are normalised once, each row is scored by lgcn_score_lists, no score filter
    runs. Queries are processed longest row first in blocks whose list capacity is
    max(k, the block's longest row), at most BLOCK_BYTES // (8 * capacity) queries each, and come
    back in the caller's order; the row lengths are read on the host once per call. A row longer
    than _ffi.RANKED_MAX_CAP is a ValueError naming the length; cap= and subset= have no meaning
    with among and passing either is a ValueError.
    boost: None, or a float32 tensor [M] on the queries' device, one value per candidate, shared by all
    queries (a per-query weight is the caller's scaling of the vector): candidate j is ranked by
    score + boost[j], ONE f32 addition on the score the unboosted call gives the pair, and that sum is
    the score returned. It is added where the key is formed, before any threshold, so a boosted
    candidate is found wherever it stood before; everything else — the order, excl, attrs / where,
    among, the padding, cap's meaning — is unchanged, on the boosted scores. -0.0 is the exact identity
    (the unboosted lists, bit for bit, at the boosted kernels' cost); -inf ranks a candidate last among
    the eligible, where it still fills a slot when fewer than k others exist; +inf ranks it above every
    finite score; NaN first. Nothing is checked on the values and no host read is added. Any other
    dtype, shape or device is a ValueError before anything is launched. With boost=None the library
    calls are exactly those above. popularity_boost makes a popularity penalty from interaction counts.
    topk_items, topk_users, topk_rows_diverse, topk_rows_calibrated and metrics.evaluate_ranking hand
    boost= on; topk_groups and metrics.rank_positions / evaluate_auc do not take one."""
    k = int(k)
    if index_dtype not in (torch.int64, torch.int32):
        raise ValueError(f"recommend: index_dtype must be torch.int64 or torch.int32, got {index_dtype}")
    if k < 1 or k > MAX_K:
        raise ValueError(f"recommend: k={k} outside [1, {MAX_K}]")
    Q = torch.as_tensor(picked).numel()
    if among is not None:
        if cap is not None or subset is not None:
            raise ValueError("recommend: cap= and subset= have no meaning with among= (a block's capacity is its "
                             "longest row)")
        among = _serving.csr_arg("recommend", "among", among, Q)[:3]
    else:
        cap = CAP if cap is None else int(cap)
        if cap < k:
            raise ValueError(f"recommend: k={k} exceeds the list capacity {cap}")
        if cap > _ffi.RANKED_MAX_CAP:
            raise ValueError(f"recommend: cap={cap} exceeds {_ffi.RANKED_MAX_CAP}")
        subset = max(SUBSET_MIN, SUBSET_PER_K * k) if subset is None else int(subset)
        if subset < 1:
            raise ValueError(f"recommend: subset={subset}")
    masks = _where_arg(attrs, where, candidates.shape[0], Q)
    _boost_arg(boost, candidates.shape[0], queries.device)
    if excl is not None:
        excl = _serving.csr_arg("recommend", "excl", excl, Q)[:3]
    order = blocks = None
    if among is not None:
        # longest row first. The one host read of the call: the sorted row lengths, which give every
        # block's boundaries and capacity at once (and the refusal of a row the selection cannot hold,
        # before anything is loaded)
        lens, order = _serving.longest_first(_serving.row_lengths(among[0], among[2], Q))
        lengths = lens.cpu().numpy()
        if Q and int(lengths[0]) > _ffi.RANKED_MAX_CAP:
            raise ValueError(f"recommend: an among row has {int(lengths[0])} entries, above the ranked selection's "
                             f"capacity {_ffi.RANKED_MAX_CAP}")
        blocks = _among_blocks(lengths, k, BLOCK_BYTES)
    lib = _ffi.load()
    for t in (queries, candidates) if masks is None else (queries, candidates, attrs):
        _ffi.require_device(t, "recommend")
    dev = queries.device
    if candidates.shape[1] != queries.shape[1]:
        raise ValueError("recommend: queries and candidates must have the same width")
    D = _serving.width("recommend", queries.shape[1])
    picked = torch.as_tensor(picked).to(device=dev, dtype=torch.int64).contiguous().view(-1)
    if Q == 0:
        return (torch.empty((0, k), dtype=index_dtype, device=dev),
                torch.empty((0, k), dtype=torch.float32, device=dev))
    if among is not None:  # unpadded: a block is launched for its own queries only
        plan = _Plan(lib, queries, picked, candidates, k, D, Q, excl, masks, attrs, order.to(dev), boost=boost)
        _run_among(plan, among, blocks)
    else:
        plan = _Plan(lib, queries, picked, candidates, k, D, _serving.padded(Q), excl, masks, attrs, boost=boost)
        if candidates.shape[0] <= cap:
            _run_dense(plan)
        else:
            _run_filtered(plan, cap, subset)
    return plan.finish(index_dtype)


STRATEGIES = {"least_misery": _ffi.GROUP_MIN, "most_pleasure": _ffi.GROUP_MAX, "average": _ffi.GROUP_MEAN}


def topk_groups(queries: torch.Tensor, groups, candidates: torch.Tensor, k: int, strategy: str = "least_misery",
                floor=None, excl=None, cap: int | None = None, subset: int | None = None,
                index_dtype: torch.dtype = torch.int64, attrs: torch.Tensor | None = None, where=None, among=None):
    """(idx [G, k] of ``index_dtype``, score f32 [G, k]) on the device: ONE ranked list per group of
    query rows — "what do the four of us watch tonight?". groups: group_csr's output, or what it
    takes (lists of member indices into ``queries``, or a padded tensor with -1 padding); at most
    _ffi.GROUP_MAX_MEMBERS members per group (ValueError naming the size), an empty group gets an
    all-padding list. A candidate's group score is formed from its members' cosine scores — exactly
    the scores topk_rows ranks each member by — on the device, before anything is listed
    (lgcn_score_filter_groups), and the lists are ranked as topk_rows ranks a query's (score
    descending, candidate index ascending, NaN first; -1 / -inf in the slots a short list cannot fill):
      strategy="least_misery"   the minimum of the members' scores;
      strategy="most_pleasure"  the maximum;
      strategy="average"        the f32 sum of the members' scores in member order, one addition at a
                                time, over the member count (one f32 division);
    a NaN member score makes the group's score NaN under all three, and a member named twice counts
    twice. A group of one has that member's topk_rows list, bit for bit.
    floor ("average without misery" with strategy="average"; works with every strategy): None, a float
    for all groups, or one value per group; a candidate that SOME member scores below the group's
    floor is not eligible (a NaN score is not below anything). NaN is a ValueError. A group left with
    fewer than k candidates is padded, above ``cap`` too.
    excl: topk_rows', with one row per GROUP (group_seen_csr builds it from the users' seen rows) or
    (ptr, idx, rows). cap, subset, index_dtype: topk_rows'. attrs / where: topk_rows' attribute filter
    with one mask row per group (or one for all); the group filter does not know the predicate — the
    ranked selection alone applies it — so above ``cap`` candidates a group's list must also hold the
    non-passing candidates that score above its k-th eligible one, as it must the excluded ones
    (RuntimeError after eight tightening rounds otherwise; a group that cannot fill k with passing
    candidates would need all M slots). among= is not supported with groups (ValueError).
    Groups are bucketed by size class S (the next power of two >= the size, at least 2), one plan run
    per class over S member rows per group, and come back in the caller's order; the group sizes are
    read on the host once per call."""
    k = int(k)
    if among is not None:
        raise ValueError("recommend: among= is not supported with groups")
    if strategy not in STRATEGIES:
        raise ValueError(f"recommend: strategy must be one of {sorted(STRATEGIES)}, got {strategy!r}")
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
    gptr, gidx = (t.cpu() for t in _groups_arg(groups))
    G = gptr.numel() - 1
    sizes = gptr[1:] - gptr[:-1]  # the host read of the call: the classes and their padded member rows
    if G and int(sizes.max()) > _ffi.GROUP_MAX_MEMBERS:
        raise ValueError(f"recommend: a group has {int(sizes.max())} members, above {_ffi.GROUP_MAX_MEMBERS}")
    if gidx.numel() and (int(gidx.min()) < 0 or int(gidx.max()) >= queries.shape[0]):
        raise ValueError(f"recommend: a group member lies outside the {queries.shape[0]} query rows")
    if floor is not None:
        floor = torch.as_tensor(floor, dtype=torch.float32).detach().reshape(-1)
        if floor.numel() not in (1, G):
            raise ValueError(f"recommend: floor has {floor.numel()} values for {G} groups")
        if bool(torch.isnan(floor).any()):
            raise ValueError("recommend: floor is NaN")
        floor = floor.expand(G)
    masks = _where_arg(attrs, where, candidates.shape[0], G)
    if excl is not None:
        excl = _serving.csr_arg("recommend", "excl", excl, G)[:3]
    lib = _ffi.load()
    for t in (queries, candidates) if masks is None else (queries, candidates, attrs):
        _ffi.require_device(t, "recommend")
    dev = queries.device
    if candidates.shape[1] != queries.shape[1]:
        raise ValueError("recommend: queries and candidates must have the same width")
    D = _serving.width("recommend", queries.shape[1])
    out_idx = torch.full((G, k), -1, dtype=torch.int32, device=dev)
    out_score = torch.full((G, k), float("-inf"), dtype=torch.float32, device=dev)
    cls = torch.where(sizes > 0, torch.maximum(sizes, torch.full_like(sizes, 2)), torch.zeros_like(sizes))
    cls = torch.where(cls > 0, 2 ** torch.ceil(torch.log2(cls.clamp(min=1).double())).long(), cls)  # 0: empty
    Cn = None  # the candidates' unit rows: normalised by the first class's plan, shared by the rest
    for S in (2, 4, 8, 16, 32):
        sel = torch.nonzero(cls == S).view(-1)  # the class's groups, in the caller's order
        Gc = sel.numel()
        if Gc == 0:
            continue
        # [Gc, S] member rows: a group's own in order, its first member in the padding slots (rows the
        # kernel never takes: it goes by the sizes)
        slot = torch.arange(S)[None, :]
        n = sizes[sel][:, None]
        members = gidx.to(torch.int64)[gptr[sel][:, None] + torch.where(slot < n, slot, torch.zeros_like(slot))]
        sel_d = sel.to(dev)
        group = _Group(S, STRATEGIES[strategy], sizes[sel].to(device=dev, dtype=torch.int32).contiguous(),
                       None if floor is None else floor.to(dev)[sel_d].contiguous())
        excl_c = None if excl is None else (excl[0], excl[1], sel if excl[2] is None else excl[2].to("cpu")[sel])
        gm = _serving.QUERY_MULTIPLE // S
        plan = _Plan(lib, queries, members.reshape(-1).to(dev).contiguous(), candidates, k, D, -(-Gc // gm) * gm, excl_c,
                     None if masks is None else masks.to(dev)[sel_d], attrs, group=group, Cn=Cn)
        Cn = plan.Cn
        if candidates.shape[0] <= cap:
            _run_dense(plan)
        else:
            _run_filtered(plan, cap, subset)
        idx, score = plan.finish(torch.int32)
        out_idx[sel_d], out_score[sel_d] = idx, score
    return (out_idx.to(torch.int64) if index_dtype == torch.int64 else out_idx), out_score


class Reranked(NamedTuple):
    """lgcn_rerank_mmr's outputs for Q queries and k picks, on the device."""
    idx: torch.Tensor    # [Q, k], the pool's index dtype: the picks in pick order, -1 in unfilled slots
    score: torch.Tensor  # f32 [Q, k]: each pick's relevance as the pool gave it, -inf in unfilled slots
    pair: torch.Tensor   # f32 [Q, k]: each pick's summed similarity to the picks before it, 0 in unfilled slots
    n: torch.Tensor      # int32 [Q]: filled slots


def _diversity(diversity) -> float:
    d = float(diversity)
    if not 0.0 <= d <= 1.0:  # NaN fails both comparisons
        raise ValueError(f"recommend: diversity={d} outside [0, 1]")
    return d


def rerank_mmr(pool_idx: torch.Tensor, pool_score: torch.Tensor, candidates: torch.Tensor, k: int, diversity: float,
               normalized: bool = False) -> Reranked:
    """Greedy Maximal Marginal Relevance over per-query pools, on the device (lgcn_rerank_mmr).

    pool_idx [Q, N] int32 or int64 and pool_score [Q, N] f32: each query's pool in the caller's
    order (topk_rows' output in practice; rows may be a column slice of a wider tensor), entries
    distinct; an entry outside [0, M) — the -1 of a short list — is skipped. candidates [M, d]: the
    rows the similarities are cosines of, normalised once here; with normalized=True they are taken
    as unit rows already and only zero-padded to the kernel's width.
    Step by step the pick is the unpicked entry with the largest
    (1 - diversity) * score - diversity * (largest cosine to a pick so far), the lowest pool
    position among equal values; so diversity=0 returns the pool's first k eligible entries and the
    list for a smaller k is a prefix. Returns Reranked(idx, score, pair, n); intra_list_diversity
    turns pair and n into ILD@c.
    Limits: 1 <= k <= N <= MMR_MAX_POOL and N * D * 4 <= MMR_MAX_LDS_BYTES, D the padded width
    (ValueError before anything is loaded)."""
    k, diversity = int(k), _diversity(diversity)
    if pool_idx.dim() != 2 or pool_score.shape != pool_idx.shape:
        raise ValueError("rerank_mmr: pool_idx and pool_score must both be [Q, N]")
    _serving.require_index_dtype("rerank_mmr", "pool_idx", pool_idx)
    if pool_score.dtype != torch.float32:
        raise TypeError(f"rerank_mmr: pool_score must be float32, got {pool_score.dtype}")
    if candidates.dim() != 2 or candidates.dtype != torch.float32:
        raise TypeError("rerank_mmr: candidates must be 2-D float32")
    Q, N = pool_idx.shape
    M, d = candidates.shape
    if k < 1 or k > N:
        raise ValueError(f"rerank_mmr: k={k} outside [1, N={N}]")
    if N > MMR_MAX_POOL:
        raise ValueError(f"rerank_mmr: a pool of {N} entries exceeds MMR_MAX_POOL={MMR_MAX_POOL}")
    D = _serving.width("recommend", d)
    if N * D * 4 > MMR_MAX_LDS_BYTES:
        raise ValueError(f"rerank_mmr: {N} pool rows of width {D} take {N * D * 4} bytes, above "
                         f"MMR_MAX_LDS_BYTES={MMR_MAX_LDS_BYTES} (at most {MMR_MAX_LDS_BYTES // (4 * D)} rows)")
    lib = _ffi.load()
    for t in (pool_idx, pool_score, candidates):
        _ffi.require_device(t, "rerank_mmr")
    dev = pool_idx.device
    index_dtype = pool_idx.dtype
    pool_idx, ld = _serving.index_list(pool_idx)
    pool_score = pool_score.detach()
    if pool_score.stride(1) != 1 or (Q > 1 and pool_score.stride(0) != ld):  # one leading dimension serves both
        pool_idx, pool_score, ld = pool_idx.contiguous(), pool_score.contiguous(), N
    s = _ffi.stream_of(dev)
    Cn = _serving.unit_rows(lib, candidates, D, normalized, s)
    out_idx = torch.empty((Q, k), dtype=torch.int32, device=dev)
    out_score = torch.empty((Q, k), dtype=torch.float32, device=dev)
    out_pair = torch.empty((Q, k), dtype=torch.float32, device=dev)
    out_n = torch.empty(Q, dtype=torch.int32, device=dev)
    if Q:
        _ffi.check(lib.lgcn_rerank_mmr(pool_idx.data_ptr(), pool_score.data_ptr(), ld, N, Q, Cn.data_ptr(), M, D, k,
                                       diversity, out_idx.data_ptr(), out_score.data_ptr(), out_pair.data_ptr(),
                                       out_n.data_ptr(), s), "lgcn_rerank_mmr")
    return Reranked(out_idx.to(index_dtype), out_score, out_pair, out_n)


def topk_rows_diverse(queries: torch.Tensor, picked: torch.Tensor, candidates: torch.Tensor, k: int, diversity: float,
                      pool: int | None = None, excl=None, **kw) -> Reranked:
    """topk_rows for a relevance pool of ``pool`` entries per query, then rerank_mmr down to k:
    Reranked(idx, score, pair, n), score staying the cosine relevance.

    pool: default max(4 * k, 64); whatever is asked for is clamped to what exists and what the
    re-rank kernel holds, min(M, MMR_MAX_POOL, MMR_MAX_LDS_BYTES // (4 * D)) with D the padded
    width, and a pool that ends up below k is a ValueError. excl and kw (cap, subset, index_dtype,
    attrs, where, among, boost) are topk_rows'; under a filter a query's pool holds passing candidates
    only, and with among= entries of the query's row only (a pool wider than a row is padded, and the
    picks all lie in the row). With boost= the pool is the boosted ranking's and the relevance MMR
    weighs — and ``score`` — is the boosted score."""
    k, diversity = int(k), _diversity(diversity)
    if k < 1:
        raise ValueError(f"recommend: k={k} outside [1, {MMR_MAX_POOL}]")
    if queries.dim() != 2 or candidates.dim() != 2:
        raise ValueError("recommend: queries and candidates must be 2-D")
    M, D = candidates.shape[0], _serving.width("recommend", candidates.shape[1])
    want = max(4 * k, 64) if pool is None else int(pool)
    limits = {"the candidate count M": M, "MMR_MAX_POOL": MMR_MAX_POOL,
              f"MMR_MAX_LDS_BYTES // (4 * D) at D={D}": MMR_MAX_LDS_BYTES // (4 * D)}
    name = min(limits, key=limits.get)
    pool = min(want, limits[name])
    if pool < k:
        if want < k:
            raise ValueError(f"recommend: pool={want} is below k={k}")
        raise ValueError(f"recommend: k={k} exceeds the largest pool, {limits[name]} ({name})")
    index_dtype = kw.pop("index_dtype", torch.int64)
    if index_dtype not in (torch.int64, torch.int32):
        raise ValueError(f"recommend: index_dtype must be torch.int64 or torch.int32, got {index_dtype}")
    idx, score = topk_rows(queries, picked, candidates, pool, excl=excl, index_dtype=torch.int32, **kw)
    out = rerank_mmr(idx, score, candidates, k, diversity)
    return out if index_dtype == torch.int32 else out._replace(idx=out.idx.to(torch.int64))


def intra_list_diversity(pair: torch.Tensor, n: torch.Tensor, ks) -> torch.Tensor:
    """ILD@c of re-ranked lists, float64 [Q, C] for the sorted distinct cutoffs of ``ks``: one minus
    the mean pairwise cosine among a list's first c' = min(c, n) items,
    1 - 2 * sum(pair[:c']) / (c' * (c' - 1)), NaN where c' < 2. pair and n are Reranked's (pair[t]
    is pick t's summed cosine to picks 0 .. t - 1). Plain torch on the tensors' device; CPU tensors
    work too."""
    if pair.dim() != 2 or n.shape != pair.shape[:1]:
        raise ValueError(f"intra_list_diversity: pair {tuple(pair.shape)} / n {tuple(n.shape)} are not [Q, k] / [Q]")
    cs = sorted({int(c) for c in ks})
    if not cs or cs[0] < 1 or cs[-1] > pair.shape[1]:
        raise ValueError(f"intra_list_diversity: cutoffs {cs} outside [1, k={pair.shape[1]}]")
    f64 = torch.float64
    csum = torch.cat([torch.zeros((pair.shape[0], 1), dtype=f64, device=pair.device),
                      torch.cumsum(pair.to(f64), 1)], 1)
    c = torch.tensor(cs, dtype=torch.int64, device=pair.device)
    cp = torch.minimum(n.to(torch.int64).clamp(min=0)[:, None], c[None, :])
    pairs = (cp * (cp - 1)).to(f64)
    ild = 1.0 - 2.0 * csum.gather(1, cp) / pairs.clamp(min=1.0)
    return torch.where(cp >= 2, ild, torch.full((), float("nan"), dtype=f64, device=pair.device))


class Calibrated(NamedTuple):
    """lgcn_rerank_calibrated's outputs for Q queries and k picks, on the device."""
    idx: torch.Tensor    # [Q, k], the pool's index dtype: the picks in pick order, -1 in unfilled slots
    score: torch.Tensor  # f32 [Q, k]: each pick's relevance as the pool gave it, -inf in unfilled slots
    kl: torch.Tensor     # f32 [Q, k]: KL(target || the list up to and including the pick), 0 in unfilled slots
    n: torch.Tensor      # int32 [Q]: filled slots


def _calibration(calibration) -> float:
    c = float(calibration)
    if not 0.0 <= c <= 1.0:  # NaN fails both comparisons
        raise ValueError(f"recommend: calibration={c} outside [0, 1]")
    return c


def _alpha(alpha) -> float:
    a = float(alpha)
    if not 0.0 < a < 1.0:
        raise ValueError(f"recommend: alpha={a} outside (0, 1)")
    return a


def _attr_words(who: str, attrs, M: int | None = None) -> None:
    if not isinstance(attrs, torch.Tensor) or attrs.dtype != torch.int32 or attrs.dim() != 1:
        raise TypeError(f"{who}: attrs must be an int32 tensor [M] (see attr_bits)")
    if M is not None and attrs.numel() != M:
        raise ValueError(f"{who}: attrs has {attrs.numel()} entries for {M} candidates")


def attr_profile(history, attrs: torch.Tensor, rows=None, weights: torch.Tensor | None = None):
    """(p f32 [Q, 32], w f32 [Q]) on the device: each history's target distribution over the 32 bits
    of the attribute words (lgcn_attr_profile). An item's own distribution is uniform over the set
    bits of attrs[i]; p is the weighted mean of those of the history's items, formed in float64 and
    rounded once, w the weight it was formed from. An entry outside [0, M), one whose word is 0
    (movies.csv's "(no genres listed)") or whose weight is not > 0 (NaN included) is skipped; a
    history with nothing left gives 32 zeros and w = 0, which rerank_calibrated reads as "no target".

    history: the CSR (ptr int64 [R + 1], idx int32) — one output row per CSR row — or (ptr, idx, rows);
    rows= names the CSR row of each output beside a 2-tuple (a row outside the CSR is an empty
    history). attrs: int32 [M] on the device (attr_bits). weights: f32, one per CSR entry; None: 1.
    The same history gives the same bits alone or in a batch, at any position, and run to run.
    ValueError / TypeError for bad arguments before anything is loaded."""
    if rows is not None:
        if history is None or len(history) != 2:
            raise ValueError("attr_profile: rows= goes with a history of (ptr, idx)")
        history = (history[0], history[1], rows)
    ptr, hidx, hrow, Q = _serving.csr_arg("attr_profile", "history", history)
    _attr_words("attr_profile", attrs)
    _serving.check_weights("attr_profile", weights, hidx.numel())
    lib = _ffi.load()
    for t in (attrs,) + (() if weights is None else (weights,)):
        _ffi.require_device(t, "attr_profile")
    dev = attrs.device
    p = torch.empty((Q, CALIB_GENRES), dtype=torch.float32, device=dev)
    w = torch.empty(Q, dtype=torch.float32, device=dev)
    M = attrs.numel()
    if Q == 0 or hidx.numel() == 0 or M == 0:  # nothing to sum (and no device address to pass)
        return p.zero_(), w.zero_()
    ptr, hidx, hrow = _serving.csr_on(dev, ptr, hidx, hrow)
    weights = None if weights is None else weights.detach().contiguous()
    _ffi.check(lib.lgcn_attr_profile(ptr.data_ptr(), hidx.data_ptr(), _ffi.ptr(weights), _ffi.ptr(hrow), ptr.numel() - 1,
                                     Q, attrs.detach().contiguous().data_ptr(), M, p.data_ptr(), w.data_ptr(),
                                     _ffi.stream_of(dev)), "lgcn_attr_profile")
    return p, w


def rerank_calibrated(pool_idx: torch.Tensor, pool_score: torch.Tensor, attrs: torch.Tensor, target: torch.Tensor,
                      k: int, calibration: float, alpha: float = 0.01) -> Calibrated:
    """Greedy calibrated re-ranking over per-query pools, on the device (lgcn_rerank_calibrated).

    pool_idx [Q, N] int32 or int64 and pool_score [Q, N] f32: each query's pool in the caller's order
    (topk_rows' output in practice; rows may be a column slice of a wider tensor), entries distinct;
    an entry outside [0, M) — the -1 of a short list — is skipped. attrs int32 [M]: the candidates'
    attribute words, a bit per genre. target f32 [Q, 32]: each query's genre distribution p
    (attr_profile's). With l = calibration, the list's distribution q (the mean of its items' own,
    items without a word left out) and q~ = (1 - alpha) * q + alpha * p, step by step the pick is the
    unpicked entry with the largest (1 - l) * score - l * KL(p || q~ of the list with it), the lowest
    pool position among equal values; so calibration=0 returns the pool's first k eligible entries,
    the list for a smaller k is a prefix, and a target row of zeros gives the pool order with kl = 0.
    Returns Calibrated(idx, score, kl, n); miscalibration turns kl and n into C_KL@c.
    Limits: 1 <= k <= N <= CALIB_MAX_POOL (ValueError before anything is loaded)."""
    k, calibration, alpha = int(k), _calibration(calibration), _alpha(alpha)
    if pool_idx.dim() != 2 or pool_score.shape != pool_idx.shape:
        raise ValueError("rerank_calibrated: pool_idx and pool_score must both be [Q, N]")
    _serving.require_index_dtype("rerank_calibrated", "pool_idx", pool_idx)
    if pool_score.dtype != torch.float32:
        raise TypeError(f"rerank_calibrated: pool_score must be float32, got {pool_score.dtype}")
    _attr_words("rerank_calibrated", attrs)
    Q, N = pool_idx.shape
    if not isinstance(target, torch.Tensor) or target.dtype != torch.float32:
        raise TypeError("rerank_calibrated: target must be a float32 tensor [Q, 32]")
    if tuple(target.shape) != (Q, CALIB_GENRES):
        raise ValueError(f"rerank_calibrated: target is {tuple(target.shape)} for {Q} queries, not [{Q}, {CALIB_GENRES}]")
    if k < 1 or k > N:
        raise ValueError(f"rerank_calibrated: k={k} outside [1, N={N}]")
    if N > CALIB_MAX_POOL:
        raise ValueError(f"rerank_calibrated: a pool of {N} entries exceeds CALIB_MAX_POOL={CALIB_MAX_POOL}")
    lib = _ffi.load()
    for t in (pool_idx, pool_score, attrs, target):
        _ffi.require_device(t, "rerank_calibrated")
    dev = pool_idx.device
    index_dtype = pool_idx.dtype
    pool_idx, ld = _serving.index_list(pool_idx)
    pool_score = pool_score.detach()
    if pool_score.stride(1) != 1 or (Q > 1 and pool_score.stride(0) != ld):  # one leading dimension serves both
        pool_idx, pool_score, ld = pool_idx.contiguous(), pool_score.contiguous(), N
    out_idx = torch.empty((Q, k), dtype=torch.int32, device=dev)
    out_score = torch.empty((Q, k), dtype=torch.float32, device=dev)
    out_kl = torch.empty((Q, k), dtype=torch.float32, device=dev)
    out_n = torch.empty(Q, dtype=torch.int32, device=dev)
    if Q:
        words = attrs.detach().contiguous()
        if words.numel() == 0:  # the library wants an address; no entry is eligible
            words = torch.zeros(1, dtype=torch.int32, device=dev)
        _ffi.check(lib.lgcn_rerank_calibrated(pool_idx.data_ptr(), pool_score.data_ptr(), ld, N, Q, words.data_ptr(),
                                              attrs.numel(), target.detach().contiguous().data_ptr(), k, calibration,
                                              alpha, out_idx.data_ptr(), out_score.data_ptr(), out_kl.data_ptr(),
                                              out_n.data_ptr(), _ffi.stream_of(dev)), "lgcn_rerank_calibrated")
    return Calibrated(out_idx.to(index_dtype), out_score, out_kl, out_n)


def topk_rows_calibrated(queries: torch.Tensor, picked: torch.Tensor, candidates: torch.Tensor, k: int,
                         calibration: float, attrs: torch.Tensor | None = None, history=None,
                         target: torch.Tensor | None = None, pool: int | None = None, excl=None, alpha: float = 0.01,
                         **kw) -> Calibrated:
    """topk_rows for a relevance pool of ``pool`` entries per query, then rerank_calibrated down to k:
    Calibrated(idx, score, kl, n), score staying the cosine relevance.

    attrs: the candidates' attribute words, int32 [M] on the device (required; the same words serve a
    where= filter). Exactly one of history — a CSR (ptr, idx), row q being query q's, or
    (ptr, idx, rows), profiled here by attr_profile — and target (f32 [Q, 32]) says what to
    calibrate to. pool: default max(4 * k, 64); whatever is asked for is clamped to what exists and
    what the re-rank kernel holds, min(M, CALIB_MAX_POOL), and a pool that ends up below k is a
    ValueError. excl and kw (where, among, boost, cap, subset, index_dtype) are topk_rows'; under a filter
    a query's pool holds passing candidates only, and with among= entries of the query's row only. With
    boost= the pool is the boosted ranking's and the relevance the calibration weighs — and ``score`` —
    is the boosted score."""
    k, calibration, alpha = int(k), _calibration(calibration), _alpha(alpha)
    if k < 1:
        raise ValueError(f"recommend: k={k} outside [1, {CALIB_MAX_POOL}]")
    if queries.dim() != 2 or candidates.dim() != 2:
        raise ValueError("recommend: queries and candidates must be 2-D")
    if attrs is None:
        raise ValueError("recommend: a calibrated list needs attrs (the candidates' attribute words)")
    M = candidates.shape[0]
    _attr_words("recommend", attrs, M)
    if (history is None) == (target is None):
        raise ValueError("recommend: exactly one of history= and target= says what to calibrate to")
    Q = torch.as_tensor(picked).numel()
    if history is not None:
        history = _serving.csr_arg("recommend", "history", history, Q)[:3]
    want = max(4 * k, 64) if pool is None else int(pool)
    limits = {"the candidate count M": M, "CALIB_MAX_POOL": CALIB_MAX_POOL}
    name = min(limits, key=limits.get)
    pool = min(want, limits[name])
    if pool < k:
        if want < k:
            raise ValueError(f"recommend: pool={want} is below k={k}")
        raise ValueError(f"recommend: k={k} exceeds the largest pool, {limits[name]} ({name})")
    index_dtype = kw.pop("index_dtype", torch.int64)
    if index_dtype not in (torch.int64, torch.int32):
        raise ValueError(f"recommend: index_dtype must be torch.int64 or torch.int32, got {index_dtype}")
    if kw.get("where") is not None:
        kw["attrs"] = attrs
    idx, score = topk_rows(queries, picked, candidates, pool, excl=excl, index_dtype=torch.int32, **kw)
    if target is None:
        target = attr_profile(history if history[2] is not None else (history[0], history[1], torch.arange(Q)), attrs)[0]
    out = rerank_calibrated(idx, score, attrs, target, k, calibration, alpha)
    return out if index_dtype == torch.int32 else out._replace(idx=out.idx.to(torch.int64))


def miscalibration(kl: torch.Tensor, n: torch.Tensor, ks) -> torch.Tensor:
    """C_KL@c of calibrated lists, float64 [Q, C] for the sorted distinct cutoffs of ``ks``: the KL
    divergence between the target and the list's first c' = min(c, n) items, kl[:, c' - 1]; NaN where
    n == 0. kl and n are Calibrated's. Plain torch on the tensors' device; CPU tensors work too."""
    if kl.dim() != 2 or n.shape != kl.shape[:1]:
        raise ValueError(f"miscalibration: kl {tuple(kl.shape)} / n {tuple(n.shape)} are not [Q, k] / [Q]")
    cs = sorted({int(c) for c in ks})
    if not cs or cs[0] < 1 or cs[-1] > kl.shape[1]:
        raise ValueError(f"miscalibration: cutoffs {cs} outside [1, k={kl.shape[1]}]")
    c = torch.tensor(cs, dtype=torch.int64, device=kl.device)
    cp = torch.minimum(n.to(torch.int64).clamp(min=0)[:, None], c[None, :])
    got = kl.to(torch.float64).gather(1, (cp - 1).clamp(min=0))
    return torch.where(cp >= 1, got, torch.full((), float("nan"), dtype=torch.float64, device=kl.device))


def topk_items(user_emb: torch.Tensor, item_emb: torch.Tensor, users, k: int, seen=None, among=None, **kw):
    """The k best items for each user index in ``users``; seen: seen_csr(..., by="user") over all
    users (row u is user u's), whose items are left out. Returns topk_rows' (idx, score). kw: topk_rows'
    cap, subset, index_dtype, attrs and where (the items' attribute words; one filter per user or one for all)
    and boost (one f32 per item).
    among: topk_rows' candidate sets with seen's convention — a 2-tuple (ptr, idx) is a CSR over all
    users, row u being user u's set; a 3-tuple names each query's row."""
    users = torch.as_tensor(users).view(-1)
    if among is not None and len(among) == 2:
        among = (among[0], among[1], users)
    return topk_rows(user_emb, users, item_emb, k, excl=None if seen is None else (seen[0], seen[1], users),
                     among=among, **kw)


def topk_users(user_emb: torch.Tensor, item_emb: torch.Tensor, items, k: int, seen=None, among=None, **kw):
    """The k best users for each item index in ``items``; seen: seen_csr(..., by="item"); kw as
    topk_items' (attrs are then the users' attribute words); among: a 2-tuple is a CSR over all items,
    row i being item i's set of users, a 3-tuple names each query's row."""
    items = torch.as_tensor(items).view(-1)
    if among is not None and len(among) == 2:
        among = (among[0], among[1], items)
    return topk_rows(item_emb, items, user_emb, k, excl=None if seen is None else (seen[0], seen[1], items),
                     among=among, **kw)
