"""Shared by tests/test_owner_kernels.py (CPU) and tests/test_gpu_owner_kernels.py /
tests/test_gpu_exchange.py (GPU): a sequential numpy restatement of the row-exchange contracts of
include/lgcn.h (the lgcn_rows_* and lgcn_owner_* block) and of the comments of
csrc/lgcn_exchange.hip, which the kernels are held to bitwise.

A send buffer is `world` destination blocks of `blk` floats:
  [gradient ids: 2*cap floats (int64, -1 = empty) | gradient rows: cap*d | pad |
   request ids at float offset req_off: 2*rcap floats (int64, -1 = empty) | pad]
Row r goes to destination r % world. Slots are taken with atomics, so the order of the slots
inside a block is not part of the contract: blocks are compared on their valid entries sorted
by id (block_entries / block_requests), which also check that the valid slots are the block's
first ones and, where the contract says each row travels once, that the ids are distinct.

The rank-ordered mean's bar against a float64 mean (mean_bar): W - 1 float32 additions and one
division are off by at most 2^-24 * sum_r |g_r[row]| to first order (each partial sum is at most
the sum of the magnitudes; the quotient's own half ulp is 2^-24 of at most that sum / W, and the
W - 1 additions' errors arrive divided by W); the bar is twice that, for the higher-order terms.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
WIDTHS = (8, 16, 32, 64, 128, 256, 512)  # LGCN_EX_DISPATCH of csrc/lgcn_exchange.hip
MEAN_EPS = 2.0 ** -23


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same_bits(a, b) -> bool:
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---- the listed rows ---------------------------------------------------------------------------

def listed_rows(rows_a, keys_b, off_b: int = 0, first_b=None, skip_b=None) -> np.ndarray:
    """The rows a (rows_a, keys_b) list carries, in list order (int64): every rows_a entry, then
    keys_b[j] + off_b where first_b[j] is set and skip_b[row] is not (either filter may be None)."""
    out = [] if rows_a is None else [int(r) for r in np.asarray(rows_a).ravel()]
    keys = [] if keys_b is None else np.asarray(keys_b).ravel()
    for j, k in enumerate(keys):
        row = int(k) + int(off_b)
        if first_b is not None and not first_b[j]:
            continue
        if skip_b is not None and skip_b[row]:
            continue
        out.append(row)
    return np.asarray(out, np.int64)


def owner_blocks(rows, g, world: int, cap: int):
    """(blocks, overflow): blocks[o] = (ids, vals) is the multiset of (row, g[row]) owed to
    destination o = row % world, sorted by row (int64 [n_o], float32 [n_o, d]); overflow: some
    destination is owed more than cap rows."""
    rows = np.asarray(rows, np.int64).ravel()
    g = np.asarray(g, F32)
    blocks, overflow = [], False
    for o in range(world):
        ids = np.sort(rows[rows % world == o], kind="stable")
        blocks.append((ids, g[ids].reshape(len(ids), g.shape[1])))
        overflow = overflow or len(ids) > cap
    return blocks, overflow


def even_capacity(counts) -> int:
    """The tests' slots per block: the largest destination count, rounded up to even, plus 2."""
    m = max([int(c) for c in counts] or [0])
    return m + m % 2 + 2


# ---- send buffers ------------------------------------------------------------------------------

def block_floats(cap: int, d: int, rcap: int, gap: int = 0, tail: int = 0):
    """(req_off, blk) of a block with `gap` floats (even) between the gradient rows and the request
    ids and at least `tail` floats after them; blk a multiple of 4 (OwnerExchange: gap = tail = 0)."""
    req_off = 2 * cap + cap * d + gap
    blk = req_off + 2 * rcap + tail
    return req_off, blk + (-blk) % 4


def parse_send(send, world: int, blk: int, cap: int, req_off: int, rcap: int, d: int):
    """A send (or received) buffer, float32 [world * blk], as per-destination slot arrays
    (grad_ids int64 [cap], grad_rows float32 [cap, d], req_ids int64 [rcap]): the ids are int64
    viewed over float32 pairs, as OwnerExchange.unpack reads them."""
    b = np.ascontiguousarray(send, F32).reshape(world, blk)
    out = []
    for o in range(world):
        gid = np.ascontiguousarray(b[o, :2 * cap]).view(np.int64)
        rows = b[o, 2 * cap:2 * cap + cap * d].reshape(cap, d)
        rid = np.ascontiguousarray(b[o, req_off:req_off + 2 * rcap]).view(np.int64)
        out.append((gid.copy(), rows.copy(), rid.copy()))
    return out


def _valid_prefix(ids, what: str) -> int:
    """The number of valid slots: they are the first ones (a slot is the destination's counter at
    the time it was taken), every later one holds -1."""
    ids = np.asarray(ids, np.int64)
    n = int((ids >= 0).sum())
    assert (ids[:n] >= 0).all() and (ids[n:] == -1).all(), f"{what}: valid slots are not the first {n}: {ids}"
    return n


def block_entries(grad_ids, grad_rows, distinct: bool, what: str = "block"):
    """(ids, rows) of a block's valid gradient slots sorted by id (stable)."""
    n = _valid_prefix(grad_ids, what)
    order = np.argsort(grad_ids[:n], kind="stable")
    ids = np.asarray(grad_ids[:n], np.int64)[order]
    if distinct:
        assert len(np.unique(ids)) == len(ids), f"{what}: a row travels twice: {ids}"
    return ids, np.asarray(grad_rows, F32)[:n][order]


def block_requests(req_ids, distinct: bool, what: str = "block") -> np.ndarray:
    """A block's valid request ids, sorted."""
    n = _valid_prefix(req_ids, what)
    ids = np.sort(np.asarray(req_ids[:n], np.int64), kind="stable")
    if distinct:
        assert len(np.unique(ids)) == len(ids), f"{what}: a row is requested twice: {ids}"
    return ids


def reset_image(image, world: int, blk: int, cap: int, req_off: int, rcap: int) -> np.ndarray:
    """lgcn_owner_reset on the host image of a send buffer: every id slot := -1, all else kept."""
    img = np.array(image, F32).reshape(world, blk)
    minus1 = np.full(2, -1, np.int32).view(F32)
    for o in range(world):
        img[o, :2 * cap] = np.tile(minus1, cap)
        img[o, req_off:req_off + 2 * rcap] = np.tile(minus1, rcap)
    return img.reshape(-1)


def packed_image(image, world: int, blk: int, cap: int, d: int, slots, g) -> np.ndarray:
    """A reset image with gradient slots filled: slots[o] = the ids of destination o's first
    len(slots[o]) slots, each followed into the row area by g[id]. Everything else kept."""
    img = np.array(image, F32).reshape(world, blk)
    g = np.asarray(g, F32)
    for o in range(world):
        ids = np.asarray(slots[o], np.int64)
        n = len(ids)
        assert n <= cap
        img[o, :2 * n] = ids.view(F32)
        img[o, 2 * cap:2 * cap + n * d] = g[ids].reshape(-1)
    return img.reshape(-1)


def requested_image(image, world: int, blk: int, req_off: int, slots) -> np.ndarray:
    """A reset image with request slots filled: slots[o] = the ids of o's first request slots."""
    img = np.array(image, F32).reshape(world, blk)
    for o in range(world):
        ids = np.asarray(slots[o], np.int64)
        img[o, req_off:req_off + 2 * len(ids)] = ids.view(F32)
    return img.reshape(-1)


# ---- requests ----------------------------------------------------------------------------------

def requests(rows_a, keys_b, off_b: int, claim, stamp: int, world: int = 1):
    """The rows requested per destination (sorted int64 arrays), entries rows_a then keys_b + off_b.
    With a claim array (int32 [N], updated in place): each distinct row whose claim[row] != stamp is
    requested exactly once and claim[row] becomes stamp. Without: every entry, duplicates included."""
    rows = listed_rows(rows_a, keys_b, off_b)
    out = [[] for _ in range(world)]
    for row in rows:
        row = int(row)
        if claim is not None:
            if claim[row] == stamp:
                continue
            claim[row] = stamp
        out[row % world].append(row)
    return [np.sort(np.asarray(x, np.int64)) for x in out]


# ---- the rank-ordered mean ---------------------------------------------------------------------

def rank_ordered_mean(ids_all, rows_all, world: int, cap: int, div: float):
    """(first, ref) of lgcn_rows_mark_first + lgcn_rows_accumulate: the slots [world * cap] walked
    in rank order; the first occurrence of a row stores its float32 row, later ones add to it in
    float32; then every row is divided by div once (div > 0; else the sums stay undivided).
    first: uint8 [world * cap], 1 on the lowest slot holding each row; ref: {row: float32 [d]}."""
    ids_all = np.asarray(ids_all, np.int64).ravel()
    rows_all = np.asarray(rows_all, F32).reshape(world * cap, -1)
    assert ids_all.size == world * cap
    first = np.zeros(world * cap, np.uint8)
    ref: dict = {}
    for i, r in enumerate(ids_all):
        r = int(r)
        if r < 0:
            continue
        if r not in ref:
            first[i] = 1
            ref[r] = rows_all[i].copy()
        else:
            ref[r] = ref[r] + rows_all[i]
        assert ref[r].dtype == F32
    if div > 0:
        ref = {r: v / F32(div) for r, v in ref.items()}
    return first, ref


def slots_of(blocks_per_rank, cap: int, d: int):
    """(ids_all [W * cap], rows_all [W * cap, d]) from each rank's (ids, vals) block for one owner,
    -1 padded: what that owner's lgcn_rows_accumulate reads, up to the order inside a rank's slots
    (which the rank-ordered mean does not depend on: a row appears at most once per rank)."""
    W = len(blocks_per_rank)
    ids_all = np.full(W * cap, -1, np.int64)
    rows_all = np.zeros((W * cap, d), F32)
    for r, (ids, vals) in enumerate(blocks_per_rank):
        assert len(ids) <= cap and len(np.unique(ids)) == len(ids)
        ids_all[r * cap:r * cap + len(ids)] = ids
        rows_all[r * cap:r * cap + len(ids)] = vals
    return ids_all, rows_all


def dense_mean64(tables, listing, div: float):
    """(mean, mag): float64 sum over the ranks r that list the row (listing[r]: bool [N]) of
    tables[r][row], / div, and the sum of the magnitudes; rows nobody lists: 0."""
    N, d = tables[0].shape
    total = np.zeros((N, d), np.float64)
    mag = np.zeros((N, d), np.float64)
    for t, m in zip(tables, listing):
        t64 = np.asarray(t, np.float64) * np.asarray(m, bool)[:, None]
        total += t64
        mag += np.abs(t64)
    return total / float(div), mag


def mean_bar(mag) -> np.ndarray:
    """|rank-ordered float32 mean - float64 mean| <= 2^-23 * sum_r |g_r[row]|, elementwise."""
    return MEAN_EPS * np.asarray(mag, np.float64)


# ---- input recipes -----------------------------------------------------------------------------

def rank_list(rng, N: int, I: int, n_a: int = 90, n_b: int = 120):
    """One rank's gradient list, the recipe of the replicated test: about n_a distinct rows_a over
    the N rows, n_b keys_b over the I items with duplicates, first_b marking their first
    occurrences, skip_b the mask of rows_a. -> (rows_a int32, keys_b int64, first_b, skip_b uint8)."""
    rows_a = np.unique(rng.integers(0, N, n_a)).astype(np.int32)
    keys_b = rng.integers(0, I, n_b).astype(np.int64)
    first_b = np.zeros(n_b, np.uint8)
    first_b[np.unique(keys_b, return_index=True)[1]] = 1
    skip_b = np.zeros(N, np.uint8)
    skip_b[rows_a] = 1
    return rows_a, keys_b, first_b, skip_b
