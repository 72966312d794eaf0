"""Group recommendation on the GPU (lgcn_amd.recommend.topk_groups, utils.recommend.recommend_for_groups;
lgcn_score_filter_groups of csrc/lgcn_recall_group.hip).

The oracle is tests/group_checker.py on the members' own score rows, and those come from the public
path: topk_rows(every user, k = M) in dense mode, scattered by index, so they are the filter's keys.
The group key is a contract to the bit (include/lgcn.h), so every comparison is torch.equal on the
indices and on the scores' bits; there is no tolerance.

Shapes: 200 users, d in {5, 64, 100, 256}; M = 300 (dense) and M = 1000 above a capacity of 128 (the
subset thresholds and the list path); k in {1, 10, 100}. At M = 1000, k = 100 runs with cap = 512:
under cap = 128 the first thresholds (the 100th best of the 125 subset entries) let about 800 entries
through and every tightening round keeps 100 / 128 of them, so the eight rounds _run_filtered allows
end near 140 > 128 — its documented RuntimeError, whatever the kernel. Groups: sizes 1, 2, 3, 4, 5, 8, 9,
16, 17, 32 (both sides of every size class and of each four-row lane boundary), an empty group, more
groups per class than one 128-row block holds, and counts that leave padding groups."""
import functools

import numpy as np
import pandas as pd
import pytest
import torch

import group_checker as gc

pytestmark = pytest.mark.gpu

U = 200
PER_SIZE = {1: 35, 2: 35, 3: 17, 4: 17, 5: 9, 8: 9, 9: 5, 16: 5, 17: 3, 32: 3}  # 70 / 34 / 18 / 10 / 6 per class
KS = {300: [(1, {}), (10, {}), (100, {})], 1000: [(1, dict(cap=128)), (10, dict(cap=128)), (100, dict(cap=512))]}


def _emb(rng, n, d):
    return rng.standard_normal((n, d)).astype(np.float32)


def _groups(rng):
    """139 groups in shuffled order: PER_SIZE of each size, distinct members except in every fifth
    group (a member named twice counts twice), and one empty group."""
    groups = []
    for n, count in PER_SIZE.items():
        for c in range(count):
            g = rng.choice(U, n, replace=False)
            if n > 1 and c % 5 == 4:
                g[-1] = g[0]
            groups.append(g.tolist())
    groups.append([])
    return [groups[i] for i in rng.permutation(len(groups))]


@functools.lru_cache(maxsize=None)
def _case(d, M, variant="plain"):
    """(users, cands, groups) as numpy; variant "dup": 20 distinct candidate rows, repeated (equal
    group keys, ranked by index); "nan": candidate 7 is a NaN row."""
    rng = np.random.default_rng(d * 1009 + M + len(variant))
    users, cands = _emb(rng, U, d), _emb(rng, M, d)
    if variant == "dup":
        cands = _emb(rng, 20, d)[rng.integers(0, 20, M)]
    if variant == "nan":
        cands[7] = np.nan
    return users, cands, _groups(rng)


@functools.lru_cache(maxsize=None)
def _device_case(d, M, variant="plain"):
    """(users, cands on the device, groups, table): table [U, M] f32 holds every user's score row as
    the filter gives it (topk_rows in dense mode, k = M), computed once per case and never changed."""
    from lgcn_amd.recommend import topk_rows

    dev = torch.device("cuda:0")
    users, cands, groups = _case(d, M, variant)
    Ut, Ct = torch.from_numpy(users).to(dev), torch.from_numpy(cands).to(dev)
    idx, score = topk_rows(Ut, torch.arange(U), Ct, M)
    assert bool((idx >= 0).all())
    table = np.empty((U, M), dtype=np.float32)
    table[np.arange(U)[:, None], idx.cpu().numpy()] = score.cpu().numpy()
    table.setflags(write=False)
    return Ut, Ct, groups, table


def _same(got, want):
    """Indices equal and scores equal to the bit (NaN included); want is the checker's numpy pair."""
    gi, gs = got[0].cpu().numpy().astype(np.int64), got[1].cpu().numpy()
    return np.array_equal(gi, want[0]) and np.array_equal(gs.view(np.uint32), want[1].view(np.uint32))


def _csr(rows, dev):
    ptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    idx = np.concatenate([np.asarray(r, np.int32) for r in rows] + [np.zeros(0, np.int32)])
    return torch.from_numpy(ptr).to(dev), torch.from_numpy(idx).to(dev)


@pytest.mark.parametrize("strategy", gc.STRATEGIES)
@pytest.mark.parametrize("M", [300, 1000])
@pytest.mark.parametrize("d", [5, 64, 100, 256])
def test_every_strategy_equals_the_checker(gpu, d, M, strategy):
    from lgcn_amd.recommend import group_csr, topk_groups

    Ut, Ct, groups, table = _device_case(d, M)
    for k, kw in KS[M]:
        got = topk_groups(Ut, groups, Ct, k, strategy=strategy, **kw)
        assert got[0].shape == (len(groups), k) and got[0].dtype == torch.int64 and got[1].dtype == torch.float32
        assert _same(got, gc.rank_groups(table, groups, k, strategy)), k
    empty = groups.index([])
    assert (got[0][empty] == -1).all() and torch.isneginf(got[1][empty]).all()
    # the CSR and the padded tensor name the same groups
    k, kw = KS[M][1]
    want = gc.rank_groups(table, groups, k, strategy)
    assert _same(topk_groups(Ut, group_csr(groups), Ct, k, strategy=strategy, **kw), want)
    padded = torch.full((len(groups), 32), -1, dtype=torch.int64)
    for g, members in enumerate(groups):
        padded[g, :len(members)] = torch.tensor(members, dtype=torch.int64)
    assert _same(topk_groups(Ut, padded.to(gpu), Ct, k, strategy=strategy, **kw), want)


@pytest.mark.parametrize("M", [300, 1000])
@pytest.mark.parametrize("d", [64, 100])
def test_floor(gpu, d, M):
    from lgcn_amd.recommend import topk_groups

    Ut, Ct, groups, table = _device_case(d, M)
    G, k = len(groups), 10
    kw = KS[M][1][1]
    rng = np.random.default_rng(5)
    lowest = [table[g].min(0) if g else np.zeros(M, np.float32) for g in groups]  # each candidate's worst member score
    # per group: a floor between scores, and for every third group one that exactly five candidates pass
    per_group = rng.uniform(-0.3, 0.05, G).astype(np.float32)
    few = np.array([np.sort(lowest[g])[-5] for g in range(G)], dtype=np.float32)
    tight = np.where(np.arange(G) % 3 == 0, few, per_group).astype(np.float32)
    for strategy in gc.STRATEGIES:
        for floor in (np.float32(-0.05), per_group, tight, np.float32(2.0)):
            arg = float(floor) if np.ndim(floor) == 0 else torch.from_numpy(floor)
            got = topk_groups(Ut, groups, Ct, k, strategy=strategy, floor=arg, **kw)
            assert _same(got, gc.rank_groups(table, groups, k, strategy, floor=floor)), (strategy, floor)
    gi = got[0].cpu().numpy()
    assert (gi == -1).all()  # nothing passes a floor of 2
    got = topk_groups(Ut, groups, Ct, k, strategy="average", floor=torch.from_numpy(tight).to(gpu), **kw)
    gi = got[0].cpu().numpy()
    for g in range(0, G, 3):  # a padded tail behind the five that pass
        if groups[g]:
            assert (gi[g, :5] >= 0).all() and (gi[g, 5:] == -1).all() and torch.isneginf(got[1][g, 5:]).all(), g
    assert _same(got, gc.rank_groups(table, groups, k, "average", floor=tight))


@pytest.mark.parametrize("strategy", gc.STRATEGIES)
def test_equal_keys_rank_by_index_and_overflow_tightens(gpu, monkeypatch, strategy):
    from lgcn_amd import _ffi
    from lgcn_amd.recommend import topk_groups

    d, k, cap = 64, 20, 128
    for M in (300, 1000):
        Ut, Ct, groups, table = _device_case(d, M, "dup")
        want = gc.rank_groups(table, groups, k, strategy)
        if M == 1000:
            # on the CPU first: the first thresholds (the k-th best of every 8th candidate) let more than
            # cap keys through for some group, or the case tests nothing
            stride = -(-M // cap)
            over = 0
            for members in groups:
                if members:
                    keys = gc.group_keys(table[members], strategy)
                    thr = np.sort(keys[::stride])[-k]
                    over += int((keys >= thr).sum() > cap)
            assert over > 0
            calls = []
            check = _ffi.check
            monkeypatch.setattr(_ffi, "check", lambda rc, what: (calls.append(what), check(rc, what))[1])
        got = topk_groups(Ut, groups, Ct, k, strategy=strategy, **({} if M == 300 else dict(cap=cap)))
        assert _same(got, want), M
    # per class: one subset pass and at least one list pass; some class went round again
    assert calls.count("lgcn_score_filter_groups") > 2 * 5
    gi = got[0].cpu().numpy()
    for g, members in enumerate(groups):  # equal keys stand together in ascending index order
        if members:
            s = got[1][g].cpu().numpy().view(np.uint32)
            for a in range(k - 1):
                assert s[a] != s[a + 1] or gi[g, a] < gi[g, a + 1]


@pytest.mark.parametrize("M,kw", [(300, {}), (1000, dict(cap=128))])
def test_a_nan_candidate_ranks_first(gpu, M, kw):
    from lgcn_amd.recommend import topk_groups

    Ut, Ct, groups, table = _device_case(64, M, "nan")
    assert np.isnan(table[:, 7]).all()
    for strategy in gc.STRATEGIES:
        got = topk_groups(Ut, groups, Ct, 10, strategy=strategy, **kw)
        assert _same(got, gc.rank_groups(table, groups, 10, strategy))
        some = torch.tensor([g for g, m in enumerate(groups) if m], device=gpu)
        assert (got[0][some, 0] == 7).all() and torch.isnan(got[1][some, 0]).all()
        # a floor does not drop it: a NaN is not below anything
        got = topk_groups(Ut, groups, Ct, 10, strategy=strategy, floor=-0.1, **kw)
        assert _same(got, gc.rank_groups(table, groups, 10, strategy, floor=np.float32(-0.1)))
        assert (got[0][some, 0] == 7).all()


@pytest.mark.parametrize("M,kw", [(300, {}), (1000, dict(cap=128))])
@pytest.mark.parametrize("d", [5, 64, 256])
def test_groups_of_one_user(gpu, d, M, kw):
    from lgcn_amd.recommend import topk_groups, topk_rows

    Ut, Ct, _, table = _device_case(d, M)
    who = torch.arange(0, U, 3)
    own = topk_rows(Ut, who, Ct, 10, **kw)
    for strategy in gc.STRATEGIES:  # a group of one is that user's list, bit for bit
        got = topk_groups(Ut, [[u] for u in who.tolist()], Ct, 10, strategy=strategy, **kw)
        assert torch.equal(got[0], own[0]) and torch.equal(got[1].view(torch.int32), own[1].view(torch.int32))
    # a user named n times: the user's own list for the minimum and the maximum, the checker's for the mean
    reps = [1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 31, 32]
    groups = [[u] * reps[i % len(reps)] for i, u in enumerate(who.tolist())]
    for strategy in ("least_misery", "most_pleasure"):
        got = topk_groups(Ut, groups, Ct, 10, strategy=strategy, **kw)
        assert torch.equal(got[0], own[0]) and torch.equal(got[1].view(torch.int32), own[1].view(torch.int32))
    assert _same(topk_groups(Ut, groups, Ct, 10, strategy="average", **kw), gc.rank_groups(table, groups, 10, "average"))


@pytest.mark.parametrize("M,kw,most", [(300, {}, 30), (1000, dict(cap=128), 5)])
def test_exclusion_rows_and_the_attribute_filter(gpu, M, kw, most):
    from lgcn_amd.recommend import group_seen_csr, topk_groups

    Ut, Ct, groups, table = _device_case(64, M)
    G, k = len(groups), 10
    rng = np.random.default_rng(21)
    seen = [np.sort(rng.choice(M, int(n), replace=False)) for n in rng.integers(0, most + 1, U)]
    seen[groups[0][0] if groups[0] else 0] = np.zeros(0, np.int64)
    want_rows = {"any": [], "all": []}
    for members in groups:
        sets = [set(seen[u].tolist()) for u in members]
        want_rows["any"].append(sorted(set().union(*sets)))
        want_rows["all"].append(sorted(set.intersection(*sets)) if sets else [])
    for by in ("any", "all"):
        excl = group_seen_csr(_csr(seen, gpu), groups, by=by)
        assert [excl[1][excl[0][g]:excl[0][g + 1]].tolist() for g in range(G)] == want_rows[by]
        for strategy in gc.STRATEGIES:
            got = topk_groups(Ut, groups, Ct, k, strategy=strategy, excl=excl, **kw)
            assert _same(got, gc.rank_groups(table, groups, k, strategy, excl=want_rows[by])), (by, strategy)
    # (ptr, idx, rows): the groups reversed name their rows
    back = list(range(G))[::-1]
    got = topk_groups(Ut, [groups[g] for g in back], Ct, k, excl=(*excl, torch.tensor(back)), **kw)
    want = gc.rank_groups(table, groups, k, "least_misery", excl=want_rows["all"])
    assert _same(got, (want[0][back], want[1][back]))
    # where=: one mask row per group; the ranked selection alone applies it
    attr = rng.integers(0, 16, M).astype(np.int32)
    any_ = rng.integers(0, 16, G)
    if M == 300:
        any_[::9] = 1 << 20  # a bit no candidate has: nothing passes
    else:
        # above the capacity the group filter's lists hold non-passing candidates too, so a group that
        # cannot fill k would need all M slots (topk_groups' docstring): every mask here lets at least a
        # quarter of the candidates pass (`any` = 8 alone contradicts `none` = 8)
        any_[any_ == 8] = 9
    passes = ((attr[None, :] & 8) == 0) & ((any_[:, None] == 0) | ((attr[None, :] & any_[:, None]) != 0))
    where = (torch.from_numpy(any_), 0, 8)
    at = torch.from_numpy(attr).to(gpu)
    for strategy in gc.STRATEGIES:
        got = topk_groups(Ut, groups, Ct, k, strategy=strategy, attrs=at, where=where, **kw)
        assert _same(got, gc.rank_groups(table, groups, k, strategy, passes=passes)), strategy
    assert M != 300 or (got[0][::9] == -1).all()
    got = topk_groups(Ut, groups, Ct, k, strategy="average", floor=-0.2, excl=excl, attrs=at, where=where, **kw)
    assert _same(got, gc.rank_groups(table, groups, k, "average", floor=np.float32(-0.2), excl=want_rows["all"],
                                     passes=passes))


@pytest.mark.parametrize("M,kw", [(300, {}), (1000, dict(cap=128))])
def test_permutations_reruns_and_int32_indices(gpu, M, kw):
    from lgcn_amd.recommend import topk_groups

    Ut, Ct, groups, _ = _device_case(100, M)
    rng = np.random.default_rng(33)
    perm = rng.permutation(len(groups))
    shuffled = [rng.permutation(g).tolist() for g in groups]
    for strategy in gc.STRATEGIES:
        base = topk_groups(Ut, groups, Ct, 10, strategy=strategy, **kw)
        again = topk_groups(Ut, groups, Ct, 10, strategy=strategy, **kw)
        assert torch.equal(base[0], again[0]) and torch.equal(base[1].view(torch.int32), again[1].view(torch.int32))
        moved = topk_groups(Ut, [groups[g] for g in perm], Ct, 10, strategy=strategy, **kw)
        at = torch.from_numpy(perm).to(gpu)
        assert torch.equal(moved[0], base[0][at]) and torch.equal(moved[1].view(torch.int32), base[1][at].view(torch.int32))
        if strategy != "average":  # the minimum and the maximum do not depend on the member order
            other = topk_groups(Ut, shuffled, Ct, 10, strategy=strategy, **kw)
            assert torch.equal(other[0], base[0]) and torch.equal(other[1].view(torch.int32), base[1].view(torch.int32))
        i32 = topk_groups(Ut, groups, Ct, 10, strategy=strategy, index_dtype=torch.int32, **kw)
        assert i32[0].dtype == torch.int32 and torch.equal(i32[0].to(torch.int64), base[0])
        assert torch.equal(i32[1].view(torch.int32), base[1].view(torch.int32))
    idx, score = topk_groups(Ut, [], Ct, 4)
    assert idx.shape == (0, 4) and idx.dtype == torch.int64 and score.shape == (0, 4)
    idx, score = topk_groups(Ut, [[], []], Ct, 4)
    assert (idx == -1).all() and torch.isneginf(score).all() and idx.shape == (2, 4)


def test_raw_entry_point_lists_and_counts(gpu):
    """lgcn_score_filter_groups itself, S = 4 and S = 16: dense rows hold the checker's keys; under zero
    thresholds a list names every candidate once and its count runs past a small capacity; with a floor
    it names the candidates that pass; empty and padding groups take nothing."""
    from lgcn_amd import _ffi, _serving

    lib = _ffi.load()
    Ut, Ct, _, table = _device_case(64, 300)
    M, D = 300, 64
    s = _ffi.stream_of(gpu)
    Cn = _serving.unit_rows(lib, Ct, D, False, s)
    rng = np.random.default_rng(41)
    for S, Gpad in ((4, 32), (16, 8)):
        sizes = rng.integers(1, S + 1, Gpad - 2).tolist()
        sizes[1] = 0  # an empty group; the last two groups are padding
        Gv = len(sizes)
        members = np.zeros((Gpad, S), dtype=np.int64)
        for g, n in enumerate(sizes):
            members[g, :n] = rng.choice(U, n, replace=False)
            members[g, n:] = members[g, 0]
        Qn = _serving.unit_queries(lib, Ut, torch.from_numpy(members[:Gv].reshape(-1)).to(gpu), D, Gpad * S, False, s)
        gsize = torch.tensor(sizes, dtype=torch.int32, device=gpu)
        floors = np.full(Gv, -0.1, dtype=np.float32)
        for agg, strategy in enumerate(gc.STRATEGIES):
            want = [gc.group_keys(table[members[g, :n]], strategy) if n else None for g, n in enumerate(sizes)]
            dkey = torch.full((Gpad, M), 0x5A5A5A5A, dtype=torch.int32, device=gpu)
            didx = torch.full((Gpad, M), -99, dtype=torch.int32, device=gpu)
            _ffi.check(lib.lgcn_score_filter_groups(Qn.data_ptr(), Gpad, Gv, S, gsize.data_ptr(), agg, None, Cn.data_ptr(),
                                                    M, 1, D, None, dkey.data_ptr(), didx.data_ptr(), None, M, s), "dense")
            for cap, floor in ((M, None), (16, None), (M, floors)):
                lkey = torch.full((Gpad, cap), 0x5A5A5A5A, dtype=torch.int32, device=gpu)
                lidx = torch.full((Gpad, cap), -99, dtype=torch.int32, device=gpu)
                ln = torch.zeros(Gpad, dtype=torch.int32, device=gpu)
                thr = torch.zeros(Gpad, dtype=torch.int32, device=gpu)
                fl = None if floor is None else torch.from_numpy(floor).to(gpu)
                _ffi.check(lib.lgcn_score_filter_groups(Qn.data_ptr(), Gpad, Gv, S, gsize.data_ptr(), agg, _ffi.ptr(fl),
                                                        Cn.data_ptr(), M, 1, D, thr.data_ptr(), lkey.data_ptr(),
                                                        lidx.data_ptr(), ln.data_ptr(), cap, s), "lists")
                torch.cuda.synchronize()
                for g in range(Gpad):
                    n = sizes[g] if g < Gv else 0
                    if n == 0:  # nothing written, nothing counted
                        assert int(ln[g]) == 0 and (lidx[g] == -99).all() and (didx[g] == -99).all()
                        continue
                    assert np.array_equal(dkey[g].cpu().numpy().view(np.uint32), want[g])
                    assert didx[g].tolist() == list(range(M))
                    ok = np.ones(M, bool) if floor is None else gc.eligible(table[members[g, :n]], floor=floor[g])
                    assert int(ln[g]) == int(ok.sum())  # entries past cap are counted
                    kept = min(cap, int(ok.sum()))
                    li = lidx[g, :kept].cpu().numpy()
                    assert len(set(li.tolist())) == kept and ok[li].all()
                    assert np.array_equal(lkey[g, :kept].cpu().numpy().view(np.uint32), want[g][li])
                    assert (lidx[g, kept:] == -99).all()
                    if kept == int(ok.sum()):
                        assert sorted(li.tolist()) == np.nonzero(ok)[0].tolist()


class _Handler:
    """40 movies (ids 100, 103, ...) with a genre each, 30 users with five training edges each (global
    numbering, both directions): the synthetic MovieLens handler of tests/test_gpu_recommend_among.py."""

    def __init__(self):
        rng = np.random.default_rng(51)
        ids = [100 + 3 * i for i in range(40)]
        self.user_id_map = {1000 + u: u for u in range(30)}
        self.movie_id_map = {m: 30 + i for i, m in enumerate(ids)}
        self.movies = pd.DataFrame({"movieId": ids, "title": [f"Movie {m}" for m in ids],
                                    "genres": [["Comedy", "Horror", "Drama", "Romance"][i % 4] for i in range(40)]})
        drawn = np.stack([rng.choice(40, 7, replace=False) for _ in range(30)]) + 30
        u = np.repeat(np.arange(30), 5)
        i = drawn[:, :5].reshape(-1)
        self.seen = [set((drawn[v, :5] - 30).tolist()) for v in range(30)]
        self.edge_index = torch.from_numpy(np.stack([np.concatenate([u, i]), np.concatenate([i, u])])).long()


def test_harness_serves_groups(gpu):
    from lgcn_amd.recommend import topk_groups
    from models.light_gcn import LightGCN
    from utils import recommend as R

    h = _Handler()
    torch.manual_seed(5)
    model = LightGCN(30, 40, num_layers=2, dim_h=32).to(gpu)
    model.eval()
    groups = [[1003, 1001, 1017, 1009], [1002, 1002, 1005], [1004, -1], [], [1029]]
    members = [[h.user_id_map[u] for u in g] for g in (groups[0], groups[1], groups[3], groups[4])]
    with torch.no_grad():
        user_emb, item_emb = model.get_embeddings(user_indices=torch.arange(30, device=gpu),
                                                  item_indices=torch.arange(40, device=gpu))
    movie_of = lambda i: 100 + 3 * i
    for strategy, floor in (("least_misery", None), ("most_pleasure", None), ("average", None), ("average", -0.05)):
        got = R.recommend_for_groups(model, groups, h, k=8, strategy=strategy, floor=floor, seen_by=None)
        assert got[2] == {"error": "Invalid user ID"} and got[3] == []
        idx, score = topk_groups(user_emb, members, item_emb, 8, strategy=strategy, floor=floor)
        for slot, g in ((0, 0), (1, 1), (4, 3)):
            want = [(movie_of(i), s) for i, s in zip(idx[g].tolist(), score[g].tolist()) if i >= 0]
            assert [(x["movie_id"], x["score"]) for x in got[slot]] == want
            assert all(x["title"] == f"Movie {x['movie_id']}" for x in got[slot]) and (got[slot] or floor is not None)
        assert R.recommend_for_group(model, groups[0], h, k=8, strategy=strategy, floor=floor, seen_by=None) == got[0]
    # seen_by: what any member has seen, what every member has seen, nothing
    ranked = lambda **kw: [x["movie_id"] for x in R.recommend_for_group(model, groups[0], h, k=40, **kw)]
    seen = [h.seen[u] for u in members[0]]
    everything = ranked(seen_by=None)
    assert len(everything) == 40
    union, common = set().union(*seen), set.intersection(*seen)
    assert ranked() == ranked(seen_by="any") == [m for m in everything if (m - 100) // 3 not in union]
    assert ranked(seen_by="all") == [m for m in everything if (m - 100) // 3 not in common]
    assert len(union) > len(common)
    pair = [1000, 1000]  # one user twice: what "all" leaves out is what that user has seen
    got = [x["movie_id"] for x in R.recommend_for_group(model, pair, h, k=40, seen_by="all")]
    assert len(got) == 35 and not {(m - 100) // 3 for m in got} & h.seen[0]
    # genres=
    comedies = ranked(seen_by=None, genres=["Comedy"])
    assert comedies == [m for m in everything if ((m - 100) // 3) % 4 == 0] and len(comedies) == 10
    assert R.recommend_for_group(model, [1001, 5], h) == {"error": "Invalid user ID"}
