"""BPR negatives drawn on the device (lgcn_sample_negatives in csrc/lgcn_negatives.hip): per triplet
an item its user has no train edge to, exactly uniform over the unseen items and without rejection,
or the hardest of n such draws — the one the model's tables currently score highest by cosine
(dynamic negative sampling).

    sample_negatives   users + the seen CSR (+ tables) -> negatives, one call
    NegativeSampler    the seen CSR of a training edge set built once, a step counter, device stats;
                       FusedTrainStep's neg_sampler, and utils.helpers.set_negative_sampler's

The draw is a counter hash of (seed, step, the triplet's global index, the candidate's number),
spelled out in include/lgcn.h: it uses no torch generator, the same triplet gets the same negative
in any batch split and run to run, and a host checker reproduces it to the bit.

Hardest-of-n under the row-lazy Adam (lgcn_amd.optim.RowLazyAdam, the harness's fast path): with
``model=`` the sampler reads the two embedding tables as they are in memory at each draw. The lazy
optimizer brings a row up to date only when a step touches it, so a row not touched lately lags its
dense value by the moment-only updates of the steps since. That affects only which of the n
candidates counts as the hardest — every candidate is an unseen item either way, and the step itself
reads current rows — and it is not corrected.
"""
from __future__ import annotations

import torch

from . import _ffi, _serving

MAX_CANDIDATES = _ffi.NEGATIVES_MAX_N  # n of hardest-of-n
MAX_D = _ffi.NEGATIVES_MAX_D           # columns of a table row

_SEED_MASK = (1 << 64) - 1


def _check_tables(tables, num_items: int):
    if not isinstance(tables, (tuple, list)) or len(tables) != 2:
        raise ValueError("negatives: tables is (user rows [U, d], item rows [I, d])")
    uw, iw = tables
    for t, nm in ((uw, "user"), (iw, "item")):
        if not torch.is_tensor(t) or t.dim() != 2 or t.dtype != torch.float32:
            raise TypeError(f"negatives: the {nm} table must be a 2-D float32 tensor")
    d = uw.shape[1]
    if iw.shape[1] != d:
        raise ValueError(f"negatives: table widths differ: {d} vs {iw.shape[1]}")
    if d < 4 or d % 4 != 0 or d > MAX_D:
        raise ValueError(f"negatives: rows of {d} columns (multiples of 4 from 4 to {MAX_D} are supported)")
    if iw.shape[0] != num_items:
        raise ValueError(f"negatives: the item table has {iw.shape[0]} rows for {num_items} items")
    if uw.device != iw.device:
        raise ValueError(f"negatives: the tables are on {uw.device} and {iw.device}")
    return uw, iw


def _aligned_rows(t: torch.Tensor):
    """(t, ld) with 16-byte aligned rows: t as it is when its rows already are, else a copy."""
    t, ld = _serving.row_view(t.detach())
    if ld % 4 != 0 or t.data_ptr() % 16 != 0:
        t = t.clone(memory_format=torch.contiguous_format)
        ld = t.shape[1]
    return t, ld


def sample_negatives(users: torch.Tensor, seen, num_items: int, *, seed: int, step: int, candidates: int = 1,
                     tables=None, first: int = 0, out: torch.Tensor | None = None, return_score: bool = False,
                     stats: torch.Tensor | None = None):
    """int64 [B] on the device: a negative for every triplet (with return_score: also f32 [B], the
    pick's cosine; 0 when candidates == 1), lgcn_sample_negatives' rule (include/lgcn.h).

    users: int64 [B] on the device. seen: the CSR (ptr int64 [R + 1], idx int32) of
    recommend.seen_csr(..., by="user") — row u the items of user u, ascending and deduplicated —
    or None to exclude nothing; a user outside the CSR has seen nothing. num_items: I; every
    negative is in [0, I). A user whose row holds every item gets a uniform draw over all items.
    seed, step: the draw's counters (seed taken mod 2^64). first: the global index of users[0], so
    that a slice of a longer list draws what the whole list draws there.
    candidates = n in [1, MAX_CANDIDATES]; n > 1 needs tables = (user rows [U, d], item rows [I, d]),
    f32 on users' device, d a multiple of 4 up to MAX_D: the pick is the candidate of the highest
    cosine, the lowest-numbered among equals, NaN ranking last. A user outside [0, U) reads no row
    and takes candidate 0. Row-strided views with 16-byte aligned rows are read in place.
    out: int64 [B] contiguous on the device, written and returned. stats: int64 [2] on the device,
    added to — [0] triplets whose user has seen every item, [1] users outside [0, U) (n > 1).
    ValueError / TypeError for bad arguments before anything is loaded; no CPU fallback."""
    if not torch.is_tensor(users) or users.dim() != 1 or users.dtype != torch.int64:
        raise TypeError("negatives: users must be a 1-D int64 tensor")
    B = users.numel()
    I = int(num_items)
    if I < 1 or I > torch.iinfo(torch.int32).max:
        raise ValueError(f"negatives: num_items={num_items}")
    n = int(candidates)
    if n < 1 or n > MAX_CANDIDATES:
        raise ValueError(f"negatives: candidates={candidates} (1 to {MAX_CANDIDATES} are supported)")
    if int(first) < 0:
        raise ValueError(f"negatives: first={first}")
    ptr = idx = None
    if seen is not None:
        ptr, idx, rows, _ = _serving.csr_arg("negatives", "seen", seen)
        if rows is not None:
            raise ValueError("negatives: seen is (ptr, idx): row u belongs to user u")
    if (n > 1) != (tables is not None):
        raise ValueError(f"negatives: tables are needed exactly when candidates > 1 (candidates={n})")
    uw = iw = None
    if tables is not None:
        uw, iw = _check_tables(tables, I)
        if uw.device != users.device:
            raise ValueError(f"negatives: the tables are on {uw.device}, users on {users.device}")
    if out is not None:
        if not torch.is_tensor(out) or out.dtype != torch.int64 or out.shape != (B,) or not out.is_contiguous():
            raise TypeError(f"negatives: out must be a contiguous int64 tensor of {B} elements")
        if out.device != users.device:
            raise ValueError(f"negatives: out is on {out.device}, users on {users.device}")
    if stats is not None:
        if not torch.is_tensor(stats) or stats.dtype != torch.int64 or stats.shape != (2,) or not stats.is_contiguous():
            raise TypeError("negatives: stats must be a contiguous int64 tensor of 2 elements")
        if stats.device != users.device:
            raise ValueError(f"negatives: stats is on {stats.device}, users on {users.device}")
    _ffi.require_device(users, "negatives")
    lib = _ffi.load()
    dev = users.device
    users = users.contiguous()
    if out is None:
        out = torch.empty(B, dtype=torch.int64, device=dev)
    score = torch.empty(B, dtype=torch.float32, device=dev) if return_score else None
    if stats is None:
        stats = torch.zeros(2, dtype=torch.int64, device=dev)
    if B > 0:
        R = 0
        if idx is not None and idx.numel() > 0:  # an empty CSR excludes nothing (and has no address)
            ptr, idx, R = ptr.to(dev).contiguous(), idx.to(dev).contiguous(), ptr.numel() - 1
        else:
            ptr = idx = None
        ldu = ldi = U = d = 0
        if uw is not None:
            U, d = uw.shape
            uw, ldu = _aligned_rows(uw)
            iw, ldi = _aligned_rows(iw)
        _ffi.check(lib.lgcn_sample_negatives(users.data_ptr(), B, int(first), _ffi.ptr(ptr), _ffi.ptr(idx), R, I,
                                             int(seed) & _SEED_MASK, int(step), n, _ffi.ptr(uw), ldu, U,
                                             _ffi.ptr(iw), ldi, d, out.data_ptr(), _ffi.ptr(score), stats.data_ptr(),
                                             _ffi.stream_of(dev)), "lgcn_sample_negatives")
    return (out, score) if return_score else out


class NegativeSampler:
    """Negatives for the triplets of one training edge set: never an item the user has a train edge
    to, and with candidates > 1 the hardest of that many draws.

    train_edge_index: the training edges in the project's global numbering (items at num_users + i,
    either or both directions), on the device the triplets will be on; its seen CSR is built once
    (recommend.seen_csr(..., by="user")). tables = (user rows, item rows) or model= (a LightGCN:
    its user_embedding.weight and item_embedding.weight, read as they are in memory at every draw —
    see the module docstring for what that means under the row-lazy Adam) give the scores for
    candidates > 1.

    As FusedTrainStep(neg_sampler=...) it draws step k's negatives straight into the batch's buffer
    (draw_triplets); installed with utils.helpers.set_negative_sampler it serves the reference's
    get_triplets_indices and the harness's fused train() alike."""

    def __init__(self, train_edge_index: torch.Tensor, num_users: int, num_items: int, candidates: int = 1,
                 seed: int = 0, tables=None, model=None):
        from .recommend import seen_csr

        self.num_users, self.num_items = int(num_users), int(num_items)
        self.candidates = int(candidates)
        if self.candidates < 1 or self.candidates > MAX_CANDIDATES:
            raise ValueError(f"negatives: candidates={candidates} (1 to {MAX_CANDIDATES} are supported)")
        if tables is not None and model is not None:
            raise ValueError("negatives: pass tables or model, not both")
        if (self.candidates > 1) != (tables is not None or model is not None):
            raise ValueError(f"negatives: tables or a model are needed exactly when candidates > 1 "
                             f"(candidates={self.candidates})")
        if tables is not None:
            _check_tables(tables, self.num_items)
        if not torch.is_tensor(train_edge_index) or train_edge_index.dim() != 2 or train_edge_index.shape[0] != 2:
            raise TypeError("negatives: train_edge_index must be a [2, E] tensor")
        _ffi.require_device(train_edge_index, "negatives")
        self.seed = int(seed)
        self.tables, self.model = tables, model
        self.seen = seen_csr(train_edge_index, self.num_users, self.num_items, by="user")
        self._stats = torch.zeros(2, dtype=torch.int64, device=train_edge_index.device)
        self.calls = 0   # draws made
        self._step = 0   # the step of the next draw that names none

    def _tables(self):
        if self.model is not None:
            return self.model.user_embedding.weight, self.model.item_embedding.weight
        return self.tables

    def draw_triplets(self, out: torch.Tensor, users: torch.Tensor, pos: torch.Tensor, step: int | None = None):
        """out[b] = the negative of triplet (users[b], pos[b]) at ``step`` (None: this sampler's own
        counter, advanced by every call that names none). pos is not read: a positive is a train
        edge, so the seen row excludes it already."""
        if step is None:
            step = self._step
            self._step += 1
        self.calls += 1
        return sample_negatives(users, self.seen, self.num_items, seed=self.seed, step=int(step),
                                candidates=self.candidates, tables=self._tables(), out=out, stats=self._stats)

    def __call__(self, users: torch.Tensor, pos: torch.Tensor) -> torch.Tensor:
        out = torch.empty(users.shape[0], dtype=torch.int64, device=users.device)
        return self.draw_triplets(out, users, pos)

    def stats(self) -> dict:
        """{"all_seen": triplets whose user had seen every item (drawn over all items), "bad_users":
        users outside the user table (candidates > 1)} over every draw so far; one host read."""
        a, b = self._stats.tolist()
        return {"all_seen": a, "bad_users": b}
