"""Hub chunks dealt to the XCDs by source window (lgcn_slice_schedule_build_xcd, tuning
slice_hub_xcd): a permutation of each slice's full hub chunks and of nothing else, the deal the
header describes, and bitwise the results of the undealt schedule. Small graphs with chunk = 8
reach hundreds of full chunks per slice."""
import numpy as np
import pytest
import torch

import graphs
from lgcn_amd import synth

pytestmark = pytest.mark.gpu

CHUNK = 8
GROUPS = {32: 32, 64: 16, 128: 8}  # items per workgroup of the item pass at width d


def _edges(U, I, rows, seed):
    """rows[i] = the users of item i (the hub rows); every further item gets 3 users dealt from a
    permutation, so no user gains more than one edge from them."""
    rng = np.random.default_rng(seed)
    users, items = [np.asarray(r, np.int64) for r in rows], [np.full(len(r), i, np.int64) for i, r in enumerate(rows)]
    perm = rng.permutation(U)
    for k, i in enumerate(range(len(rows), I)):
        users.append(perm[(3 * k + np.arange(3)) % U])
        items.append(np.full(3, i, np.int64))
    return synth.undirected_from_pairs(np.concatenate(users), np.concatenate(items), U, I)


def _dealt_rows(U, n_chunks, seed):
    """Hub item rows holding n_chunks full chunks in all (rows of up to 30 chunks, each with a tail
    of 1..7 edges), their users dealt from one cyclic permutation so user degrees stay below CHUNK
    (the item-table slice then has no hub and no row item of exactly CHUNK edges)."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(U)
    rows, cur, left, h = [], 0, n_chunks, 0
    while left > 0:
        c = min(left, 30 - (h % 5))
        deg = CHUNK * c + 1 + h % 7
        assert deg <= U
        rows.append(np.sort(perm[(cur + np.arange(deg)) % U]))
        cur += deg
        left -= c
        h += 1
    assert cur <= 4 * U
    return rows


def _plan(ei, N, dev, U):
    from lgcn_amd.plan import PropagationPlan

    return PropagationPlan(torch.from_numpy(ei).to(dev), N, CHUNK, side_split=U)


def _build(plan, N, bounds, d, on, tune, row_mask=None):
    from lgcn_amd.sliced import build_sliced

    tune(slice_hub_xcd=on)
    return build_sliced(plan.fwd, N, bounds, CHUNK, row_mask=row_mask, d=d)


def _decode(items):
    it = items.cpu().numpy()
    beg, word = it[:, 0], it[:, 1]
    return beg, (word & 0xFFFFFFFF).astype(np.int64), (word >> 32).astype(np.int64)


def _expected(beg, ln, dst, col, G):
    """The dealt order of one slice's items, from the undealt order (include/lgcn.h)."""
    P = np.nonzero((dst < 0) & (ln == CHUNK))[0]
    n = len(P)
    mid = col[beg[P] + CHUNK // 2]
    order = np.argsort(mid, kind="stable")
    lo = [x * n // 8 for x in range(9)]
    rounds = (n // 8) // G
    ptr, seq = lo[:8], []
    for j in range(8 * rounds):
        x = j % 8
        seq.extend(order[ptr[x]:ptr[x] + G])
        ptr[x] += G
    for x in range(8):
        seq.extend(order[ptr[x]:lo[x + 1]])
    idx = np.arange(len(beg))
    idx[P] = P[np.asarray(seq, np.int64)] if n else P
    return idx, P, mid, order, rounds


def _check_pair(off, on, col, G):
    """Permutation only, the old order when off, the specified deal when on. Returns the number of
    full chunks of every slice."""
    assert (on.n_splits, on.n_partials) == (off.n_splits, off.n_partials)
    assert list(on.host_offsets) == list(off.host_offsets)
    assert torch.equal(on.splits[: on.n_splits], off.splits[: off.n_splits])
    ns = []
    for (a, na), (b, nb) in zip(off.launches, on.launches):
        assert na == nb
        beg, ln, dst = _decode(a)
        # off: longest first, stable in CSR order
        plain = np.where(dst >= 0, ln & 0x1FFFFFFF, ln)
        key = list(zip(-plain, beg))
        assert key == sorted(key)
        idx, P, mid, order, rounds = _expected(beg, ln, dst, col, G)
        got = b.cpu().numpy()
        want = a.cpu().numpy()[idx]
        rest = np.setdiff1d(np.arange(na), P)
        assert np.array_equal(got[rest], a.cpu().numpy()[rest])  # everything but full chunks in place
        assert sorted(map(tuple, got)) == sorted(map(tuple, a.cpu().numpy()))
        assert np.array_equal(got, want)
        ns.append(len(P))
    return ns


def _check_deal(off_items, on_items, col, G):
    """The deal itself on a slice whose full chunks are a prefix: block j < 8 * rounds holds G
    chunks of group j % 8; groups' midpoint ranges ascend without overlap; a group's blocks ascend."""
    beg, ln, dst = _decode(off_items)
    _, P, mid, order, rounds = _expected(beg, ln, dst, col, G)
    n = len(P)
    assert np.array_equal(P, np.arange(n))
    rank = np.empty(n, np.int64)
    rank[order] = np.arange(n)
    rank_of_beg = dict(zip(beg[P].tolist(), rank.tolist()))
    gbeg, gln, gdst = _decode(on_items)
    assert np.all((gdst[:n] < 0) & (gln[:n] == CHUNK))
    r = np.array([rank_of_beg[b] for b in gbeg[:n].tolist()])
    lo = np.array([x * n // 8 for x in range(9)])
    group = np.searchsorted(lo, r, side="right") - 1
    gmid = col[gbeg[:n] + CHUNK // 2]
    last = {}
    for j in range(8 * rounds):
        blk = slice(j * G, (j + 1) * G)
        assert np.all(group[blk] == j % 8)
        assert np.array_equal(r[blk], r[j * G] + np.arange(G))
        assert np.all(np.diff(gmid[blk]) >= 0)
        if j % 8 in last:
            assert r[j * G] == last[j % 8] + 1
        last[j % 8] = r[(j + 1) * G - 1]
    tail = r[8 * rounds * G:]
    assert np.all(np.diff(tail) > 0)  # leftovers (or, below 8 * G chunks, everything) in midpoint order
    if rounds:
        dealt = slice(0, 8 * rounds * G)
        lows = [gmid[dealt][group[dealt] == x].min() for x in range(8)]
        highs = [gmid[dealt][group[dealt] == x].max() for x in range(8)]
        for x in range(7):
            assert highs[x] <= lows[x + 1]
    return n, rounds


@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("case", ["below", "exact", "remainder"])
def test_deal_by_group_size(gpu, tune, d, case):
    G = GROUPS[d]
    n = {"below": 8 * G - 1, "exact": 8 * G, "remainder": 2 * 8 * G + 13}[case]
    U, I = 1500, 160
    ei = _edges(U, I, _dealt_rows(U, n, seed=d), seed=1)
    N = U + I
    plan = _plan(ei, N, gpu, U)
    col = plan.fwd.col.cpu().numpy()
    bounds = [0, U, N]
    off = _build(plan, N, bounds, d, False, tune)
    on = _build(plan, N, bounds, d, True, tune)
    ns = _check_pair(off, on, col, G)
    assert ns == [n, 0]  # the item-table slice has no hub: nothing to deal
    assert torch.equal(on.launches[1][0], off.launches[1][0])
    got_n, rounds = _check_deal(off.launches[0][0], on.launches[0][0], col, G)
    assert (got_n, rounds) == (n, {"below": 0, "exact": 1, "remainder": 2}[case])
    changed = not torch.equal(on.launches[0][0], off.launches[0][0])
    assert changed  # a stable sort by midpoint alone already reorders these rows' chunks


def test_equal_midpoints_keep_their_order(gpu, tune):
    """Every full chunk has the same midpoint source: the sort is stable, so the deal is of the
    current order."""
    d, G = 128, 8
    U, I = 600, 8 * G + 3 + 40
    rows = [np.arange(10) for _ in range(8 * G + 3)]  # one full chunk (midpoint user 4) + 2 edges each
    ei = _edges(U, I, rows, seed=2)
    N = U + I
    plan = _plan(ei, N, gpu, U)
    col = plan.fwd.col.cpu().numpy()
    bounds = [0, U, N]
    off = _build(plan, N, bounds, d, False, tune)
    on = _build(plan, N, bounds, d, True, tune)
    ns = _check_pair(off, on, col, G)
    assert ns[0] == 8 * G + 3
    beg, ln, dst = _decode(off.launches[0][0])
    full = (dst < 0) & (ln == CHUNK)
    assert np.all(col[beg[full] + CHUNK // 2] == 4)
    _check_deal(off.launches[0][0], on.launches[0][0], col, G)


def _mixed_graph():
    """Hubs on both sides, several slices: items rated by hundreds of users, users with hundreds of
    items, over a sparse background."""
    U, I = 1200, 700
    rng = np.random.default_rng(5)
    rows = [np.sort(rng.choice(U, int(k), replace=False)) for k in rng.integers(300, 900, 20)]
    ei = _edges(U, I, rows, seed=3)
    heavy_u = np.repeat(np.arange(6), 400)
    heavy_i = np.concatenate([rng.choice(I, 400, replace=False) for _ in range(6)])
    extra = synth.undirected_from_pairs(heavy_u, heavy_i, U, I)
    N = U + I
    key = np.unique(np.concatenate([ei[0] * N + ei[1], extra[0] * N + extra[1]]))
    return U, I, np.stack([key // N, key % N])


@pytest.mark.parametrize("d", [32, 64, 128])
def test_permutation_only_over_several_slices(gpu, tune, d):
    U, I, ei = _mixed_graph()
    N = U + I
    plan = _plan(ei, N, gpu, U)
    col = plan.fwd.col.cpu().numpy()
    bounds = [0, U // 3, 2 * U // 3, U, U + I // 2, N]
    off = _build(plan, N, bounds, d, False, tune)
    on = _build(plan, N, bounds, d, True, tune)
    ns = _check_pair(off, on, col, GROUPS[d])
    assert max(ns) >= 8 * GROUPS[d]  # at least one slice is really dealt
    # without a width the builder keeps the old order whatever the switch says
    from lgcn_amd.sliced import build_sliced

    plain = build_sliced(plan.fwd, N, bounds, CHUNK)
    assert torch.equal(plain.items[: plain.host_offsets[-1]], off.items[: off.host_offsets[-1]])


@pytest.mark.parametrize("d", [32, 64, 128])
def test_results_bitwise(gpu, tune, d):
    """K = 3 forward and one LGConv layer over the dealt and the undealt schedule: the same bits,
    with the riding combine and without, twice per call."""
    from lgcn_amd import propagate_forward
    from lgcn_amd.propagate import lgconv_forward
    from lgcn_amd.sliced import SlicedDirection

    U, I, ei = _mixed_graph()
    N, K = U + I, 3
    tune(slice_mb=N * d * 4 / 5 / 2**20)
    plans = {}
    for on in (False, True):
        tune(slice_hub_xcd=on)
        plans[on] = _plan(ei, N, gpu, U)
        assert isinstance(plans[on].schedule("fwd", d), SlicedDirection)
    a, b = plans[False].schedule("fwd", d), plans[True].schedule("fwd", d)
    assert len(a.launches) >= 3
    assert not torch.equal(a.items[: a.host_offsets[-1]], b.items[: b.host_offsets[-1]])
    uw, iw = graphs.embeddings(U, I, d, seed=d)
    uw_t, iw_t = torch.from_numpy(uw).to(gpu), torch.from_numpy(iw).to(gpu)
    x = torch.cat([uw_t, iw_t])
    for ride in (True, False):
        tune(slice_ride=ride)
        want = propagate_forward(uw_t, iw_t, plans[False], K).cpu()
        for _ in range(2):
            assert torch.equal(propagate_forward(uw_t, iw_t, plans[True], K).cpu(), want)
    want = lgconv_forward(x, plans[False]).cpu()
    for _ in range(2):
        assert torch.equal(lgconv_forward(x, plans[True]).cpu(), want)


def test_unchanged_paths(gpu, tune):
    """An uncoalesced edge_index still gets no sliced schedule, and a row_mask schedule (a rank's
    share of a sharded plan) keeps the old order."""
    from lgcn_amd.plan import CsrDirection

    U, I, ei = graphs.shuffled()
    N, d = U + I, 64
    plan = _plan(ei, N, gpu, U)
    assert _build(plan, N, [0, U, N], d, True, tune) is None
    tune(slice_mb=0.005)
    assert isinstance(plan.schedule("fwd", d), CsrDirection)

    U, I, ei = _mixed_graph()
    N = U + I
    plan = _plan(ei, N, gpu, U)
    mask = (torch.arange(N, device=gpu) % 2 == 0).to(torch.uint8)
    bounds = [0, U // 2, U, N]
    off = _build(plan, N, bounds, d, False, tune, row_mask=mask)
    on = _build(plan, N, bounds, d, True, tune, row_mask=mask)
    assert list(on.host_offsets) == list(off.host_offsets)
    assert torch.equal(on.items[: on.host_offsets[-1]], off.items[: off.host_offsets[-1]])
    assert torch.equal(on.splits[: on.n_splits], off.splits[: off.n_splits])
