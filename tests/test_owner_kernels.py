"""The CPU reference of the row-exchange kernels (tests/owner_checker.py) against independent
statements of the same contracts: the rank-ordered float32 mean against a float64 dense mean, the
owner blocks as a partition of the listed rows, and the request dedupe's stamp."""
import numpy as np
import pytest

import owner_checker as oc

F32 = np.float32


def _ranks(W, N, d, cap, seed):
    """W ranks' gradient tables and slot lists (each rank lists about half the rows, in a random
    order, -1 padded to cap)."""
    rng = np.random.default_rng(seed)
    tables, listing = [], []
    ids_all = np.full(W * cap, -1, np.int64)
    rows_all = np.zeros((W * cap, d), F32)
    for r in range(W):
        # magnitudes across six decades and both signs: sums that cancel and sums that do not
        t = (rng.standard_normal((N, d)) * 10.0 ** rng.integers(-3, 3, (N, 1))).astype(F32)
        rows = rng.permutation(N)[:rng.integers(N // 3, cap + 1)]
        m = np.zeros(N, bool)
        m[rows] = True
        ids_all[r * cap:r * cap + len(rows)] = rows
        rows_all[r * cap:r * cap + len(rows)] = t[rows]
        tables.append(t)
        listing.append(m)
    return tables, listing, ids_all, rows_all


@pytest.mark.parametrize("W", [1, 2, 3, 8])
def test_rank_ordered_mean_within_bar_of_float64_mean(W):
    """|out - mean64| <= 2^-23 * sum_r |g_r[row]| elementwise, on exactly the listed rows."""
    N, d, cap = 97, 16, 70
    tables, listing, ids_all, rows_all = _ranks(W, N, d, cap, seed=W)
    first, ref = oc.rank_ordered_mean(ids_all, rows_all, W, cap, float(W))
    mean, mag = oc.dense_mean64(tables, listing, float(W))
    union = np.flatnonzero(np.any(listing, axis=0))
    assert sorted(ref) == list(union)
    assert int(first.sum()) == len(union)
    worst = 0.0
    for row, v in ref.items():
        assert v.dtype == F32
        err, bar = np.abs(v.astype(np.float64) - mean[row]), oc.mean_bar(mag[row])
        assert (err <= bar).all(), (row, err.max(), bar.min())
        worst = max(worst, float((err / np.maximum(bar, 1e-300)).max()))
    print(f"W={W}: worst error / bar {worst:.3f}")
    # one listing rank: the row itself / W, exactly one rounding
    for row in union:
        who = [r for r in range(W) if listing[r][row]]
        if len(who) == 1:
            assert oc.same_bits(ref[row], tables[who[0]][row] / F32(W))


def test_rank_ordered_mean_first_is_lowest_slot_and_div_zero_keeps_sums():
    ids = np.array([5, -1, 3, 3, 5, 7, -1, 5, 3], np.int64)  # W = 3, cap = 3
    rows = np.arange(9 * 4, dtype=F32).reshape(9, 4) + F32(0.1)
    first, ref = oc.rank_ordered_mean(ids, rows, 3, 3, 0.0)
    assert first.tolist() == [1, 0, 1, 0, 0, 1, 0, 0, 0]
    assert oc.same_bits(ref[5], (rows[0] + rows[4]) + rows[7])
    assert oc.same_bits(ref[3], (rows[2] + rows[3]) + rows[8])
    assert oc.same_bits(ref[7], rows[5])
    _, mean = oc.rank_ordered_mean(ids, rows, 3, 3, 3.0)
    assert all(oc.same_bits(mean[r], ref[r] / F32(3)) for r in ref)


@pytest.mark.parametrize("world", [1, 3, 8])
def test_owner_blocks_partition_the_listed_rows(world):
    """The per-destination lists are a disjoint cover of listed_rows; the order of rows_a and
    keys_b does not change the sorted result; every value is g[row]."""
    U, I, d = 500, 300, 8
    N = U + I
    rng = np.random.default_rng(world)
    g = rng.standard_normal((N, d)).astype(F32)
    rows_a, keys_b, first_b, skip_b = oc.rank_list(rng, N, I)
    listed = oc.listed_rows(rows_a, keys_b, U, first_b, skip_b)
    # the filters: rows_a whole, then each key not in rows_a once
    want = set(rows_a.tolist()) | {int(k) + U for k in keys_b}
    assert len(listed) == len(want) and set(listed.tolist()) == want
    assert listed[:len(rows_a)].tolist() == rows_a.tolist()
    assert listed.min() < U <= listed.max()
    blocks, over = oc.owner_blocks(listed, g, world, cap=len(listed))
    assert not over and len(blocks) == world
    for o, (ids, vals) in enumerate(blocks):
        assert (ids % world == o).all() and (np.diff(ids) > 0).all()
        assert oc.same_bits(vals, g[ids])
    assert np.array_equal(np.sort(np.concatenate([b[0] for b in blocks])), np.sort(listed))
    # another order of the same lists (first_b follows its keys)
    pa, pb = rng.permutation(len(rows_a)), rng.permutation(len(keys_b))
    first_p = np.zeros(len(keys_b), np.uint8)
    first_p[np.unique(keys_b[pb], return_index=True)[1]] = 1
    again, _ = oc.owner_blocks(oc.listed_rows(rows_a[pa], keys_b[pb], U, first_p, skip_b), g, world, cap=len(listed))
    for (a, va), (b, vb) in zip(blocks, again):
        assert np.array_equal(a, b) and oc.same_bits(va, vb)
    # without a filter the duplicates travel
    every = oc.listed_rows(rows_a, keys_b, U, None, skip_b)
    assert len(every) == len(rows_a) + int((skip_b[keys_b + U] == 0).sum()) > len(listed)
    both = oc.listed_rows(rows_a, keys_b, U, first_b, None)
    assert len(both) == len(rows_a) + int(first_b.sum()) > len(listed)
    # the overflow report: the fullest destination decides
    most = max(len(b[0]) for b in blocks)
    assert oc.owner_blocks(listed, g, world, most)[1] is False
    assert oc.owner_blocks(listed, g, world, most - 1)[1] is True


@pytest.mark.parametrize("world", [1, 3, 8])
def test_requests_stamp(world):
    """With a claim array: each distinct row once, to its owner; the same stamp again requests
    nothing; the next stamp requests the full distinct set again. Without: every entry."""
    U, I = 152, 48
    rng = np.random.default_rng(10 + world)
    rows_a = np.unique(rng.integers(0, U + I, 60)).astype(np.int32)
    keys_b = rng.integers(0, I, 3000).astype(np.int64)
    distinct = np.unique(np.concatenate([rows_a.astype(np.int64), keys_b + U]))
    assert np.intersect1d(rows_a, keys_b + U).size  # some rows come through both lists
    claim = np.full(U + I, -1, np.int32)
    got = oc.requests(rows_a, keys_b, U, claim, 1, world)
    assert len(got) == world
    for o, ids in enumerate(got):
        assert np.array_equal(ids, distinct[distinct % world == o])
    assert np.array_equal(np.flatnonzero(claim == 1), distinct) and ((claim == 1) | (claim == -1)).all()
    assert all(len(x) == 0 for x in oc.requests(rows_a, keys_b, U, claim, 1, world))
    again = oc.requests(rows_a, keys_b, U, claim, 2, world)
    assert all(np.array_equal(a, b) for a, b in zip(got, again))
    assert np.array_equal(np.flatnonzero(claim == 2), distinct)
    every = oc.requests(rows_a, keys_b, U, None, 7, world)
    assert sum(len(x) for x in every) == len(rows_a) + len(keys_b)
    assert np.array_equal(np.sort(np.concatenate(every)),
                          np.sort(np.concatenate([rows_a.astype(np.int64), keys_b + U])))
    for o, ids in enumerate(every):
        assert (ids % world == o).all()


def test_parse_send_round_trips_an_image():
    """parse_send reads what packed_image / requested_image / reset_image lay out."""
    world, cap, rcap, d = 3, 4, 6, 8
    req_off, blk = oc.block_floats(cap, d, rcap, gap=2, tail=3)
    assert req_off == 2 * cap + cap * d + 2 and blk % 4 == 0 and blk >= req_off + 2 * rcap + 3
    rng = np.random.default_rng(0)
    g = rng.standard_normal((20, d)).astype(F32)
    pre = np.full(world * blk, np.nan, F32)
    img = oc.reset_image(pre, world, blk, cap, req_off, rcap)
    slots = [np.array([3, 0], np.int64), np.array([], np.int64), np.array([2, 17, 5], np.int64)]
    reqs = [np.array([9], np.int64), np.array([1, 4, 10], np.int64), np.array([], np.int64)]
    img = oc.requested_image(oc.packed_image(img, world, blk, cap, d, slots, g), world, blk, req_off, reqs)
    for o, (gid, rows, rid) in enumerate(oc.parse_send(img, world, blk, cap, req_off, rcap, d)):
        ids, vals = oc.block_entries(gid, rows, True)
        assert np.array_equal(ids, np.sort(slots[o])) and oc.same_bits(vals, g[ids])
        assert np.array_equal(oc.block_requests(rid, True), np.sort(reqs[o]))
        assert np.isnan(rows[len(slots[o]):]).all()
    # the gap, the tail and nothing else keep the pre-fill
    b = img.reshape(world, blk)
    assert np.isnan(b[:, req_off - 2:req_off]).all() and np.isnan(b[:, req_off + 2 * rcap:]).all()
    with pytest.raises(AssertionError):
        oc.block_requests(np.array([4, -1, 5], np.int64), True)
    with pytest.raises(AssertionError):
        oc.block_requests(np.array([4, 4, -1], np.int64), True)
