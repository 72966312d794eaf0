"""Per-item score boosts without a GPU: the numpy checker of the contract against a brute-force sort on
hand-made cases, the ABI bookkeeping, the argument checks of lgcn_score_filter_boost and
lgcn_score_lists_boost (codes and messages, no device touched), topk_rows' refusals of a bad boost=
(before the library is loaded), popularity_boost against float64, and the harness's boost forms."""
import numpy as np
import pandas as pd
import pytest
import torch

import boost_checker as bc


def _no_load(monkeypatch):
    from lgcn_amd import _ffi

    def no_load(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(_ffi, "load", no_load)


def test_keys_order_floats_with_nan_first_and_minus_zero_below_zero():
    vals = np.array([-np.inf, -3.5, -1e-40, -0.0, 0.0, 1e-40, 0.25, np.inf, np.nan], np.float32)
    keys = bc.score_key(vals)
    assert (np.diff(keys.astype(np.int64)) > 0).all()  # strictly ascending, -0 below +0, NaN last (the highest)
    assert keys[-1] == 0xFFFFFFFF and (keys != 0).all()
    back = bc.key_score(keys)
    assert (back[:-1].view(np.uint32) == vals[:-1].view(np.uint32)).all() and np.isnan(back[-1])
    assert bc.score_key(np.array([-np.nan], np.float32))[0] == 0xFFFFFFFF  # every NaN, whatever its sign


def test_checker_agrees_with_a_brute_force_sort_on_hand_made_cases():
    inf, nan = np.inf, np.nan
    scores = np.array([[0.5, 0.25, 0.5, -0.0, 0.0, 0.75, -0.25, 0.5, 0.1, 0.1],
                       [0.0, -0.0, 0.0, -0.0, 1.0, -1.0, 0.5, 0.5, 0.5, nan],
                       [0.3, 0.3, 0.3, 0.3, 0.3, 0.3, 0.3, 0.3, 0.3, 0.3]], np.float32)
    cases = {
        "identity": np.full(10, -0.0, np.float32),
        "plus_zero": np.zeros(10, np.float32),  # turns a -0 score into +0: a different key
        "ties": np.array([0.0, 0.25, 0.0, 0.5, 0.5, -0.25, 0.75, 0.0, 0.4, 0.4], np.float32),
        "infinities": np.array([-inf, 0.0, inf, -inf, 0.0, 0.0, inf, -0.0, 0.0, -inf], np.float32),
        "nan": np.array([0.0, nan, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, inf], np.float32),
    }
    for name, boost in cases.items():
        for k in (1, 4, 10, 12):
            gi, gs = bc.boosted_topk(scores, boost, k)
            wi, ws = bc.brute_force(scores, boost, k)
            assert (gi == wi).all() and bc.same_bits(gs, ws), (name, k)
    # the facts the cases were made for
    gi, gs = bc.boosted_topk(scores, cases["identity"], 10)
    with np.errstate(invalid="ignore"):
        assert (bc.boosted_keys(scores, cases["identity"]) == bc.score_key(scores)).all()
    assert gi[2].tolist() == list(range(10))  # all equal: by index
    assert gi[0].tolist()[:4] == [5, 0, 2, 7] and gi[0].tolist()[-3:] == [4, 3, 6]  # +0 above -0
    assert gi[1, 0] == 9 and np.isnan(gs[1, 0])  # NaN first
    gi, gs = bc.boosted_topk(scores, cases["plus_zero"], 10)
    assert gi[0].tolist()[-3:] == [3, 4, 6]  # -0 + +0 = +0: the two zeros now tie, by index
    gi, gs = bc.boosted_topk(scores, cases["infinities"], 10)
    assert gi[2].tolist() == [2, 6, 1, 4, 5, 7, 8, 0, 3, 9]
    assert np.isposinf(gs[2, :2]).all() and np.isneginf(gs[2, -3:]).all()
    assert gi[1, 0] == 9 and np.isnan(gs[1, 0])  # NaN + -inf is NaN
    gi, gs = bc.boosted_topk(scores, cases["nan"], 3)
    assert gi[0].tolist() == [1, 9, 5] and gi[1].tolist() == [1, 9, 4]  # two NaN keys tie by index, then +inf


def test_checker_options_exclusion_predicate_among_and_padding():
    scores = np.array([[0.9, 0.8, 0.7, 0.6, 0.5, 0.4]], np.float32)
    boost = np.array([-0.0, 0.0, 0.5, -np.inf, 0.0, 0.0], np.float32)
    gi, gs = bc.boosted_topk(scores, boost, 4, excl=[np.array([2])])
    assert gi.tolist() == [[0, 1, 4, 5]]
    passes = np.array([[True, False, True, True, False, False]])
    gi, gs = bc.boosted_topk(scores, boost, 4, passes=passes)
    assert gi.tolist() == [[2, 0, 3, -1]] and np.isneginf(gs[0, 2:]).all()  # the -inf filler, then padding
    gi, gs = bc.boosted_topk(scores, boost, 6, among=[np.array([5, 1, 9, -1, 1, 6, 3])])
    assert gi.tolist() == [[1, 1, 5, 3, -1, -1]]  # named twice: ranked twice; 9, -1 and 6 name nothing
    gi, gs = bc.boosted_topk(scores, boost, 3, among=[np.array([4, 2, 0, 2])], excl=[np.array([0])], passes=passes)
    assert gi.tolist() == [[2, 2, -1]] and gs[0, 0] == np.float32(0.7) + np.float32(0.5)


def test_abi_lists_the_boost_exports_and_the_new_source():
    from lgcn_amd import _ffi

    assert _ffi.ABI_VERSION == 11
    assert "lgcn_score_filter_boost" in _ffi.EXPORTED and "lgcn_score_lists_boost" in _ffi.EXPORTED
    assert "lgcn_recall_boost.hip" in _ffi.SOURCES and "lgcn_recall_among.h" in _ffi.HEADERS
    lib = _ffi.load()
    assert lib.lgcn_abi_version() == 11
    assert len(_ffi._SIGS["lgcn_score_filter_boost"][0]) == len(_ffi._SIGS["lgcn_score_filter_attr"][0]) + 1
    assert len(_ffi._SIGS["lgcn_score_lists_boost"][0]) == len(_ffi._SIGS["lgcn_score_lists"][0]) + 1


def test_boost_entry_points_check_their_arguments_without_a_device():
    from lgcn_amd import _ffi

    lib = _ffi.load()
    buf = torch.zeros(512, dtype=torch.int32)
    p = buf.data_ptr()  # a host address: an argument check must come back before anything reads it

    def filt(thr=p, attr=None, where=None, boost=p, M=10, cap=16):
        return lib.lgcn_score_filter_boost(p, 128, 4, p, M, 1, 64, thr, p, p, p, cap, attr, where, boost, None)

    def err():
        return lib.lgcn_last_error()

    assert filt(boost=None) == _ffi.E_ARG and b"lgcn_score_filter_boost: boost is null" in err()
    assert filt(thr=None, boost=None) == _ffi.E_ARG and b"boost is null" in err()
    assert filt(attr=p) == _ffi.E_ARG and b"lgcn_score_filter_boost: where is null" in err()
    assert filt(where=p) == _ffi.E_ARG and b"lgcn_score_filter_boost: attr is null" in err()
    assert filt(thr=None, attr=p, where=p) == _ffi.E_ARG
    assert b"lgcn_score_filter_boost: attr is set while thr is null" in err()
    assert filt(thr=None, M=20) == _ffi.E_ARG and b"dense mode needs M <= cap" in err()
    assert filt(M=0) == 0 and filt(M=0, attr=p, where=p) == 0 and filt(thr=None, M=0) == 0  # nothing to score: no launch
    assert lib.lgcn_score_filter_boost(p, 128, 4, p, 10, 1, 48, p, p, p, p, 16, None, None, p, None) == _ffi.E_UNSUPPORTED

    names = ["Qn", "Cn", "among_ptr", "among_idx", "list_key", "list_idx", "list_n", "boost"]

    def lists(null=None, D=64, cap=16, Q=4):
        a = {n: (None if n == null else p) for n in names}
        return lib.lgcn_score_lists_boost(a["Qn"], Q, a["Cn"], 10, D, a["among_ptr"], a["among_idx"], None, 3,
                                          a["list_key"], a["list_idx"], a["list_n"], cap, a["boost"], None)

    for n in names:
        assert lists(null=n) == _ffi.E_ARG
        assert f"lgcn_score_lists_boost: {n} is null".encode() in err()
    assert lists(cap=0) == _ffi.E_ARG and b"lgcn_score_lists_boost: cap=0" in err()
    assert lists(D=100) == _ffi.E_ARG and b"lgcn_score_lists_boost: D=100" in err()
    assert lists(Q=0) == 0
    assert lists(Q=0, null="boost") == _ffi.E_ARG  # a null boost is refused even where nothing would launch


def test_topk_rows_refuses_a_bad_boost_before_the_library(monkeypatch):
    from lgcn_amd.recommend import topk_items, topk_rows, topk_rows_diverse

    _no_load(monkeypatch)
    q, c = torch.randn(3, 8), torch.randn(6, 8)
    call = lambda boost, **kw: topk_rows(q, torch.arange(3), c, 2, boost=boost, **kw)
    for bad in (torch.zeros(6, dtype=torch.float64), torch.zeros(6, dtype=torch.float16), torch.zeros(6, dtype=torch.int32),
                [0.0] * 6, np.zeros(6, np.float32)):
        with pytest.raises(ValueError, match="^recommend: boost must be a float32 tensor"):
            call(bad)
    for bad in (torch.zeros(5), torch.zeros(7), torch.zeros((6, 1)), torch.zeros((1, 6)), torch.zeros(())):
        with pytest.raises(ValueError, match=r"^recommend: boost has shape .* for 6 candidates"):
            call(bad)
    with pytest.raises(ValueError, match="^recommend: boost is on meta, the queries on cpu"):
        call(torch.zeros(6, device="meta"))
    ptr, idx = torch.tensor([0, 2, 2, 5], dtype=torch.int64), torch.tensor([1, 4, 0, 2, 3], dtype=torch.int32)
    with pytest.raises(ValueError, match="boost has shape"):
        call(torch.zeros(5), among=(ptr, idx))
    with pytest.raises(ValueError, match="boost must be a float32"):
        topk_items(q, c, [0, 1], 2, boost=torch.zeros(6, dtype=torch.float64))
    with pytest.raises(ValueError, match="boost has shape"):
        topk_rows_diverse(q, torch.arange(3), c, 2, 0.5, pool=4, boost=torch.zeros(3))
    with pytest.raises(AssertionError, match="the library was loaded"):  # a good boost gets that far
        call(torch.zeros(6))


def test_popularity_boost_against_float64():
    from lgcn_amd.recommend import popularity_boost

    rng = np.random.default_rng(5)
    counts = np.concatenate([[0, 0, 1, 2, 81531], rng.integers(0, 50000, 400), rng.integers(0, 5, 100)])
    want = np.log1p(counts.astype(np.float64)) / np.log1p(float(counts.max()))
    for strength in (0.2, 1.0, -0.35, 0.0):
        for t in (torch.from_numpy(counts), torch.from_numpy(counts).to(torch.int32), torch.from_numpy(counts).float()):
            got = popularity_boost(t, strength)
            assert got.dtype == torch.float32 and got.shape == (len(counts),)
            assert np.array_equal(got.numpy(), (-strength * want).astype(np.float32))
    got = popularity_boost(torch.from_numpy(counts), 0.2).numpy()
    assert got[0] == 0 and got[4] == np.float32(-0.2) and (got <= 0).all() and (got >= np.float32(-0.2)).all()
    assert got[2] < 0 and got[3] < got[2]  # monotone in the count
    zeros = popularity_boost(torch.zeros(7, dtype=torch.int64), 0.5)
    assert zeros.dtype == torch.float32 and (zeros == 0).all() and not torch.isnan(zeros).any()
    assert popularity_boost(torch.zeros(0), 0.5).shape == (0,)
    with pytest.raises(TypeError):
        popularity_boost([1, 2, 3], 0.2)
    with pytest.raises(ValueError, match="NaN"):
        popularity_boost(torch.ones(3), float("nan"))


class _Handler:
    user_id_map = {7: 0, 8: 1, 9: 2}
    movie_id_map = {30: 3, 10: 4, 50: 5, 20: 6, 40: 7}
    movies = pd.DataFrame({"movieId": [10, 20, 30, 40, 50], "title": list("abcde"), "genres": ["Comedy"] * 5})


def test_harness_boost_forms_and_the_cli_option():
    from lgcn_amd.recommend import popularity_boost
    from utils import recommend as R

    cpu = torch.device("cpu")
    never = lambda: (_ for _ in ()).throw(AssertionError("the counts were asked for without less_popular"))
    assert R._boost_vector("x", _Handler, None, None, never, cpu) == {}
    got = R._boost_vector("x", _Handler, {10: 0.5, 40: float("-inf"), 999: 3.0}, None, never, cpu)["boost"]
    assert got.dtype == torch.float32 and got.tolist() == [-0.0, 0.5, -0.0, -0.0, float("-inf")]  # item order: 30 10 50 20 40
    assert torch.signbit(got[[0, 2, 3]]).all()  # unnamed movies: -0.0, the exact identity
    vec = torch.tensor([0.1, 0.2, 0.3, 0.4, 0.5], dtype=torch.float64)
    got = R._boost_vector("x", _Handler, vec, None, never, cpu)["boost"]
    assert got.dtype == torch.float32 and torch.equal(got, vec.float())
    counts = torch.tensor([0, 3, 1, 9, 0])
    got = R._boost_vector("x", _Handler, None, 0.3, lambda: counts, cpu)["boost"]
    assert torch.equal(got, popularity_boost(counts, 0.3))
    got = R._boost_vector("x", _Handler, vec, 0.3, lambda: counts, cpu)["boost"]
    assert torch.equal(got, vec.float() + popularity_boost(counts, 0.3))
    with pytest.raises(ValueError, match="boost has 4 values for 5 movies"):
        R._boost_vector("x", _Handler, torch.zeros(4), None, never, cpu)
    for bad in (torch.zeros(5, dtype=torch.int64), [0.0] * 5, torch.zeros((5, 1))):
        with pytest.raises(ValueError, match="boost is a float tensor over the items or a mapping"):
            R._boost_vector("x", _Handler, bad, None, never, cpu)
    # unknown users and histories are answered without the model, boosted or not
    assert R.recommend_for_users_boosted(None, [1], _Handler, less_popular=0.2, boost={10: 1.0}) == [{"error": "Invalid user ID"}]
    assert R.recommend_for_histories_boosted(None, [[999]], _Handler, less_popular=0.2) == [{"error": "No known movie IDs"}]
    argv = ["recommend.py", "5", "--less-popular", "0.2", "--genres", "Comedy"]
    assert R._cli_option(argv, "--less-popular") == ["0.2"] and argv == ["recommend.py", "5", "--genres", "Comedy"]


def test_the_boosted_calls_declare_the_two_arguments_and_the_batch_calls_their_own():
    """recommend_for_users_boosted, recommend_for_histories_boosted and evaluate_ranking_boosted are the
    three calls with boost= and less_popular= declared after the positional arguments, None by default, and
    every parameter of the call they extend, with its default; the extended calls keep their own lists."""
    import inspect

    from utils import ranking_eval
    from utils import recommend as R

    def params(f):
        return [(n, p.default) for n, p in inspect.signature(f).parameters.items()]

    for plain, boosted, lead in ((R.recommend_for_users, R.recommend_for_users_boosted, 3),
                                 (R.recommend_for_histories, R.recommend_for_histories_boosted, 3),
                                 (ranking_eval.evaluate_ranking, ranking_eval.evaluate_ranking_boosted, 4)):
        old, new = params(plain), params(boosted)
        assert new == old[:lead] + [("boost", None), ("less_popular", None)] + old[lead:]
        assert "boost" not in dict(old) and not hasattr(plain, "__wrapped__") and not hasattr(boosted, "__wrapped__")
