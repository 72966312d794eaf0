"""Group recommendation without a GPU: group_csr and group_seen_csr, the argument errors of
lgcn_amd.recommend.topk_groups (all raised before the library is loaded), lgcn_score_filter_groups'
argument checks (codes and messages, no device touched), the binding's names, the host oracle of the
GPU tests on hand-made cases, and the harness's answers that need no model."""
import numpy as np
import pandas as pd
import pytest
import torch

import group_checker as gc


def _no_load(monkeypatch):
    from lgcn_amd import _ffi

    def no_load(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(_ffi, "load", no_load)


def test_group_csr_keeps_order_and_repeats():
    from lgcn_amd.recommend import group_csr

    ptr, idx = group_csr([[5, 1, 5, 3], [], (2,), torch.tensor([7, -1, 0, 7]), [-4]])
    assert ptr.dtype == torch.int64 and idx.dtype == torch.int32 and ptr.device.type == "cpu"
    assert ptr.tolist() == [0, 4, 4, 5, 8, 8]  # empty groups kept, negatives dropped
    assert idx.tolist() == [5, 1, 5, 3, 2, 7, 0, 7]  # the order given, a member named twice twice
    padded = torch.tensor([[5, 1, 5, 3], [-1, -1, -1, -1], [2, -1, -1, -1], [7, -1, 0, 7]], dtype=torch.int32)
    p2, i2 = group_csr(padded)
    assert p2.tolist() == [0, 4, 4, 5, 8] and i2.tolist() == [5, 1, 5, 3, 2, 7, 0, 7] and i2.dtype == torch.int32
    p3, i3 = group_csr([])
    assert p3.tolist() == [0] and i3.numel() == 0
    p4, i4 = group_csr(torch.zeros((3, 0), dtype=torch.int64))
    assert p4.tolist() == [0, 0, 0, 0] and i4.numel() == 0
    with pytest.raises(TypeError, match="integer"):
        group_csr(torch.zeros((2, 2)))
    with pytest.raises(TypeError, match="integers"):
        group_csr([[0.5, 1.0]])
    with pytest.raises(ValueError, match="int32"):
        group_csr([[2 ** 31]])


def _csr(rows):
    ptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    idx = np.concatenate([np.asarray(r, np.int32) for r in rows] + [np.zeros(0, np.int32)])
    return torch.from_numpy(ptr), torch.from_numpy(idx)


def test_group_seen_csr_is_the_union_or_the_intersection():
    from lgcn_amd.recommend import group_csr, group_seen_csr

    rng = np.random.default_rng(3)
    U, I = 12, 40
    seen = [np.sort(rng.choice(I, int(n), replace=False)) for n in rng.integers(3, 25, U)]
    seen[4] = np.zeros(0, np.int64)  # a member who has seen nothing
    seen[9] = np.arange(I)
    groups = [[0, 1, 2], [3], [], [5, 4, 6], [7, 7, 8], [9, 10], [11, 0, 11, 0, 2], [4], [4, 4]]
    want = {"any": [], "all": []}
    for g in groups:
        sets = [set(seen[u].tolist()) for u in g]
        want["any"].append(sorted(set().union(*sets)))
        want["all"].append(sorted(set.intersection(*sets)) if sets else [])
    assert want["all"][3] == [] and want["any"][3] != []  # the empty row empties the intersection only
    assert want["all"][4] == sorted(set(seen[7]) & set(seen[8]))  # the repeated member counts once
    assert want["all"][5] == sorted(seen[10].tolist()) and len(want["any"][5]) == I
    for by in ("any", "all"):
        for arg in (groups, group_csr(groups)):
            ptr, idx = group_seen_csr(_csr(seen), arg, by=by)
            assert ptr.dtype == torch.int64 and idx.dtype == torch.int32
            got = [idx[ptr[g]:ptr[g + 1]].tolist() for g in range(len(groups))]
            assert got == want[by], by
    ptr, idx = group_seen_csr(_csr(seen), [], by="any")
    assert ptr.tolist() == [0] and idx.numel() == 0
    ptr, idx = group_seen_csr(_csr([[], []]), [[0, 1], [1]], by="all")
    assert ptr.tolist() == [0, 0, 0] and idx.numel() == 0
    with pytest.raises(ValueError, match="by must be 'any' or 'all'"):
        group_seen_csr(_csr(seen), groups, by="most")
    with pytest.raises(ValueError, match="outside the seen CSR's 12 rows"):
        group_seen_csr(_csr(seen), [[0, 12]])


def test_topk_groups_argument_errors_come_before_the_library(monkeypatch):
    from lgcn_amd import _ffi
    from lgcn_amd.recommend import topk_groups

    _no_load(monkeypatch)
    q, c = torch.randn(40, 8), torch.randn(6, 8)
    groups = [[0, 1], [2, 3, 4]]
    with pytest.raises(ValueError, match="a group has 33 members, above 32"):
        topk_groups(q, [[0, 1], list(range(33))], c, 2)
    with pytest.raises(ValueError, match="strategy must be one of"):
        topk_groups(q, groups, c, 2, strategy="mean")
    with pytest.raises(ValueError, match="floor is NaN"):
        topk_groups(q, groups, c, 2, floor=float("nan"))
    with pytest.raises(ValueError, match="floor is NaN"):
        topk_groups(q, groups, c, 2, floor=torch.tensor([0.1, float("nan")]))
    with pytest.raises(ValueError, match="floor has 3 values for 2 groups"):
        topk_groups(q, groups, c, 2, floor=[0.1, 0.2, 0.3])
    ptr, idx = torch.tensor([0, 1, 2], dtype=torch.int64), torch.tensor([1, 4], dtype=torch.int32)
    with pytest.raises(ValueError, match="among= is not supported with groups"):
        topk_groups(q, groups, c, 2, among=(ptr, idx))
    with pytest.raises(ValueError, match="a group member lies outside the 40 query rows"):
        topk_groups(q, [[0, 40]], c, 2)
    with pytest.raises(ValueError, match="k=0 outside"):
        topk_groups(q, groups, c, 0)
    with pytest.raises(ValueError, match="k=5 exceeds the list capacity 4"):
        topk_groups(q, groups, c, 5, cap=4)
    with pytest.raises(ValueError, match="index_dtype"):
        topk_groups(q, groups, c, 2, index_dtype=torch.int16)
    with pytest.raises(ValueError, match="excl has 1 rows for 2 queries"):
        topk_groups(q, groups, c, 2, excl=(ptr[:2], idx))
    with pytest.raises(ValueError, match="where needs attrs"):
        topk_groups(q, groups, c, 2, where=(1, 0, 0))
    with pytest.raises(AssertionError, match="the library was loaded"):  # a good call gets that far
        topk_groups(q, groups, c, 2, floor=[0.1, -0.2], strategy="average")


def test_the_binding_carries_the_new_names():
    from lgcn_amd import _ffi

    assert "lgcn_recall_group.hip" in _ffi.SOURCES and "lgcn_score_filter_groups" in _ffi.EXPORTED
    assert _ffi.ABI_VERSION == 11
    assert (_ffi.GROUP_MIN, _ffi.GROUP_MAX, _ffi.GROUP_MEAN, _ffi.GROUP_MAX_MEMBERS) == (0, 1, 2, 32)
    header = (_ffi.INCLUDE / "lgcn.h").read_text()
    for line in ("#define LGCN_GROUP_MIN 0", "#define LGCN_GROUP_MAX 1", "#define LGCN_GROUP_MEAN 2",
                 "#define LGCN_GROUP_MAX_MEMBERS 32", "#define LGCN_ABI_VERSION 11"):
        assert line in header, line


def test_score_filter_groups_checks_its_arguments_without_a_device():
    """One case per argument error of the C entry point. Like lgcn_score_lists' (tests/test_recommend_among.py)
    it runs on host addresses: a check must come back before anything reads them, so no device is needed."""
    from lgcn_amd import _ffi

    lib = _ffi.load()
    buf = torch.zeros(512, dtype=torch.int32)
    p = buf.data_ptr()
    names = ["Qn", "gsize", "floor", "Cn", "thr", "list_key", "list_idx", "list_n"]

    def call(null=(), S=4, agg=_ffi.GROUP_MIN, Gpad=32, Gvalid=3, M=10, cap=16, D=64):
        a = {n: (None if n in null else p) for n in names}
        return lib.lgcn_score_filter_groups(a["Qn"], Gpad, Gvalid, S, a["gsize"], agg, a["floor"], a["Cn"], M, 1, D,
                                            a["thr"], a["list_key"], a["list_idx"], a["list_n"], cap, None)

    err = lambda: lib.lgcn_last_error().decode()
    for S in (0, 1, 3, 6, 64, -2):
        assert call(S=S) == _ffi.E_ARG and f"lgcn_score_filter_groups: S={S}" in err()
    for agg in (-1, 3):
        assert call(agg=agg) == _ffi.E_ARG and f"lgcn_score_filter_groups: agg={agg}" in err()
    for S, Gpad in ((4, 31), (2, 32), (32, 3), (8, 0)):
        assert call(S=S, Gpad=Gpad) == _ffi.E_ARG and "not a multiple of 128 rows" in err()
    for n in ("gsize", "list_key", "list_idx"):
        assert call(null=(n,)) == _ffi.E_ARG and f"lgcn_score_filter_groups: {n} is null" in err()
    assert call(null=("list_n",)) == _ffi.E_ARG and "list_n is null while thr is set" in err()
    assert call(null=("thr",)) == _ffi.E_ARG and "thr is null while floor is set" in err()
    assert call(null=("thr", "floor"), M=20) == _ffi.E_ARG and "dense mode needs M <= cap" in err()
    for kw in (dict(null=("Qn",)), dict(null=("Cn",)), dict(Gvalid=33), dict(Gvalid=-1), dict(M=-1), dict(cap=0)):
        assert call(**kw) == _ffi.E_ARG and "lgcn_score_filter_groups: bad args" in err(), kw
    assert call(D=48) == _ffi.E_UNSUPPORTED and "D=48" in err()
    assert call(Gvalid=0) == 0 and call(M=0) == 0  # nothing to do: no launch, nothing read


def test_checker_on_hand_made_cases():
    f = lambda *rows: np.array(rows, dtype=np.float32)
    bits = lambda a: np.asarray(a, np.float32).view(np.uint32).tolist()
    # keys: order-preserving, -0 just below +0, NaN highest, and back to the score's bits
    s = f([-np.inf, -1.5, -0.0, 0.0, 1e-40, 2.0, np.inf, np.nan])[0]
    k = gc.score_key(s)
    assert (np.diff(k.astype(np.int64)) > 0).all() and k[-1] == 0xFFFFFFFF and k[3] == k[2] + 1
    assert bits(gc.key_score(k))[:-1] == bits(s)[:-1] and np.isnan(gc.key_score(k)[-1])
    # -0 / +0: the minimum is -0 and the maximum +0, whichever member holds which
    for rows in (f([-0.0], [0.0]), f([0.0], [-0.0])):
        assert bits(gc.key_score(gc.group_keys(rows, "least_misery"))) == bits([-0.0])
        assert bits(gc.key_score(gc.group_keys(rows, "most_pleasure"))) == bits([0.0])
        assert bits(gc.key_score(gc.group_keys(rows, "average"))) == bits([0.0])  # -0 + 0 = +0
    assert bits(gc.key_score(gc.group_keys(f([-0.0], [-0.0]), "average"))) == bits([-0.0])
    # a NaN member score: the NaN key under every strategy, ranked first; the floor does not drop it
    rows = f([0.5, np.nan, 0.1, -0.2], [0.4, 0.9, 0.3, 0.8])
    for strategy in gc.STRATEGIES:
        idx, score = gc.rank_group(rows, 3, strategy, floor=0.2)
        assert idx[0] == 1 and np.isnan(score[0]) and idx.tolist() == [1, 0, -1] and np.isneginf(score[2])
    # the mean is the sequential f32 sum in member order, then one division: the order matters
    rows = f([1e8], [1.0], [-1e8], [1.0])
    assert gc.key_score(gc.group_keys(rows, "average"))[0] == np.float32(0.25)  # ((1e8 + 1) - 1e8) + 1 = 1
    assert gc.key_score(gc.group_keys(rows[[0, 2, 1, 3]], "average"))[0] == np.float32(0.5)
    third = gc.key_score(gc.group_keys(f([0.1], [0.2], [0.3]), "average"))[0]
    assert third == np.float32(np.float32(np.float32(0.1) + np.float32(0.2)) + np.float32(0.3)) / np.float32(3)
    # min / max, ties by index, exclusion and the predicate, the padded tail
    rows = f([0.9, 0.2, 0.5, 0.5, 0.1], [0.3, 0.8, 0.5, 0.5, 0.7])
    assert gc.rank_group(rows, 5, "least_misery")[0].tolist() == [2, 3, 0, 1, 4]
    assert gc.rank_group(rows, 5, "most_pleasure")[0].tolist() == [0, 1, 4, 2, 3]
    assert gc.rank_group(rows, 5, "least_misery", floor=0.25)[0].tolist() == [2, 3, 0, -1, -1]
    assert gc.rank_group(rows, 2, "least_misery", excl=[2])[0].tolist() == [3, 0]
    assert gc.rank_group(rows, 5, "most_pleasure", passes=[True, False, False, True, True])[0].tolist() == [0, 4, 3, -1, -1]
    # n = 1: the member's own ranking, under all three, to the bit; n = 0: all padding
    rng = np.random.default_rng(1)
    one = rng.standard_normal((1, 50)).astype(np.float32)
    one[0, [3, 9]] = [-0.0, 0.0]
    own = np.lexsort((np.arange(50), -gc.score_key(one[0]).astype(np.int64)))[:10]
    for strategy in gc.STRATEGIES:
        idx, score = gc.rank_group(one, 10, strategy)
        assert idx.tolist() == own.tolist() and bits(score) == bits(one[0, own])
    idx, score = gc.rank_group(one[:0], 4, "average")
    assert (idx == -1).all() and np.isneginf(score).all()
    # rank_groups: per-group floors, rows and predicates
    table = rng.standard_normal((6, 30)).astype(np.float32)
    groups = [[0, 1], [], [5, 5, 2]]
    idx, score = gc.rank_groups(table, groups, 4, "average", floor=np.array([-0.5, 0.0, -9.0], np.float32),
                                excl=[[1], [], [0, 2]], passes=np.arange(30) % 3 != 0)
    assert (idx[1] == -1).all() and 1 not in idx[0] and not set(idx[2]) & {0, 2} and (idx[2] % 3 != 0).all()
    want = gc.rank_group(table[[5, 5, 2]], 4, "average", floor=-9.0, excl=[0, 2], passes=np.arange(30) % 3 != 0)
    assert idx[2].tolist() == want[0].tolist() and bits(score[2]) == bits(want[1])


class _Handler:
    user_id_map = {7: 0, 8: 1, 9: 2}
    movie_id_map = {30: 3, 10: 4, 50: 5, 20: 6, 40: 7}
    movies = pd.DataFrame({"movieId": [10, 20, 30, 40, 50], "title": list("abcde"), "genres": ["Comedy"] * 5})


def test_harness_answers_unknown_users_without_the_model_and_the_cli_options():
    from utils import recommend as R

    bad = {"error": "Invalid user ID"}
    assert R.recommend_for_groups(None, [[7, 1], [999]], _Handler) == [bad, bad]
    assert R.recommend_for_group(None, [8, 9, 5], _Handler, strategy="average", floor=0.2) == bad
    assert R.recommend_for_users(None, [1], _Handler) == [bad]  # the same answer
    with pytest.raises(ValueError, match="seen_by must be 'any', 'all' or None"):
        R.recommend_for_groups(None, [[7]], _Handler, seen_by="most")
    with pytest.raises(ValueError, match="unknown genre 'Opera'"):
        R.recommend_for_groups(None, [[7]], _Handler, genres=["Opera"])
    argv = ["recommend.py", "--group", "1, 5,9", "--strategy", "average", "--floor", "0.2"]
    assert R._cli_ids(R._cli_option(argv, "--group")) == [1, 5, 9]
    assert R._cli_option(argv, "--strategy") == ["average"] and R._cli_option(argv, "--floor") == ["0.2"]
    assert argv == ["recommend.py"]
