"""Attribute-filtered top-k without a GPU: attr_bits and genre_table (vocabulary, bits, zero rows), the
argument errors of lgcn_amd.recommend.topk_rows' attrs / where and of utils.recommend's genre
arguments (all raised before the library is loaded), the int32 image of masks in [2**31, 2**32), and
the two new entry points' argument checks (codes and messages, no device touched)."""
import pandas as pd
import pytest
import torch


def _no_load(monkeypatch):
    from lgcn_amd import _ffi

    def no_load(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(_ffi, "load", no_load)


def test_attr_bits():
    from lgcn_amd.recommend import attr_bits

    vocab = ["Action", "Comedy", "Drama"]
    got = attr_bits([["Comedy"], [], ("Drama", "Action"), {"Comedy", "Drama"}, ["Comedy", "Comedy"]], vocab)
    assert got.dtype == torch.int32 and got.device.type == "cpu" and got.tolist() == [2, 0, 5, 6, 2]
    assert attr_bits([], vocab).shape == (0,)
    wide = [f"g{b}" for b in range(32)]
    got = attr_bits([["g31"], ["g0", "g31"], wide], wide)  # bit 31 is the sign bit
    assert got.tolist() == [-2 ** 31, -2 ** 31 + 1, -1]
    with pytest.raises(ValueError, match="33 labels"):
        attr_bits([[]], wide + ["g32"])
    with pytest.raises(ValueError, match="'Horror'"):
        attr_bits([["Comedy"], ["Horror"]], vocab)


class _Handler:
    """Five movies of movie_id_map (ids 10, 20, 30, 40, 50 at items 0..4 behind 3 users); 50 has no row
    in movies, 60 has a row and no index."""
    user_id_map = {7: 0, 8: 1, 9: 2}
    movie_id_map = {30: 3, 10: 4, 50: 5, 20: 6, 40: 7}
    movies = pd.DataFrame({"movieId": [10, 20, 30, 40, 60, 10],
                           "title": list("abcdef"),
                           "genres": ["Comedy|Romance", "(no genres listed)", "Horror", float("nan"), "Western",
                                      "Drama"]})


def test_genre_table():
    from utils.recommend import genre_table

    vocab, attrs = genre_table(_Handler)
    assert vocab == ["Comedy", "Horror", "Romance", "Western"]  # sorted; the placeholder is no label; the first row of an id counts
    assert attrs.dtype == torch.int32 and attrs.device.type == "cpu"
    # item order: 30 (Horror), 10 (Comedy|Romance), 50 (no row), 20 (placeholder), 40 (missing value)
    assert attrs.tolist() == [2, 5, 0, 0, 0]

    class NoColumn(_Handler):
        movies = _Handler.movies[["movieId", "title"]]

    with pytest.raises(ValueError, match="no 'genres' column"):
        genre_table(NoColumn)


def test_handler_keeps_the_genres_column(tmp_path):
    from data.dataset_handler import MovieLensDataHandler, write_synthetic_movielens
    from utils.recommend import genre_table

    rp, mp = write_synthetic_movielens(str(tmp_path), 20, 15, 200, seed=1)
    h = MovieLensDataHandler(rp, mp, device=torch.device("cpu"))
    assert list(h.movies.columns) == ["movieId", "title", "genres"]
    vocab, attrs = genre_table(h)
    assert vocab == ["Drama"] and attrs.tolist() == [1] * len(h.movie_id_map)


def test_topk_rows_filter_errors_come_before_the_library(monkeypatch):
    from lgcn_amd.recommend import topk_rows

    _no_load(monkeypatch)
    q, c = torch.randn(4, 8), torch.randn(6, 8)
    attrs = torch.zeros(6, dtype=torch.int32)
    picked = torch.arange(4)
    with pytest.raises(ValueError, match="where needs attrs"):
        topk_rows(q, picked, c, 2, where=(1, 0, 0))
    with pytest.raises(ValueError, match="attrs needs where"):
        topk_rows(q, picked, c, 2, attrs=attrs)
    with pytest.raises(TypeError, match="attrs must be an int32 tensor"):
        topk_rows(q, picked, c, 2, attrs=attrs.to(torch.int64), where=(1, 0, 0))
    with pytest.raises(TypeError, match="attrs must be an int32 tensor"):
        topk_rows(q, picked, c, 2, attrs=attrs.tolist(), where=(1, 0, 0))
    with pytest.raises(ValueError, match="attrs has 5 entries for 6 candidates"):
        topk_rows(q, picked, c, 2, attrs=attrs[:5], where=(1, 0, 0))
    for bad in ((1, 0), 5, "abc", torch.zeros(3, dtype=torch.int32)):
        with pytest.raises(ValueError, match=r"where is \(any, all, none\)"):
            topk_rows(q, picked, c, 2, attrs=attrs, where=bad)
    with pytest.raises(ValueError, match="any mask has 3 entries for 4 queries"):
        topk_rows(q, picked, c, 2, attrs=attrs, where=([1, 2, 3], 0, 0))
    with pytest.raises(ValueError, match="none mask has 5 entries for 4 queries"):
        topk_rows(q, picked, c, 2, attrs=attrs, where=(None, None, torch.zeros(5, dtype=torch.int32)))
    for bad in (2 ** 32, -2 ** 31 - 1, 2 ** 70):
        with pytest.raises(ValueError, match="outside 32 bits"):
            topk_rows(q, picked, c, 2, attrs=attrs, where=(0, bad, 0))
    with pytest.raises(ValueError, match="outside 32 bits"):
        topk_rows(q, picked, c, 2, attrs=attrs, where=(0, [0, 0, 2 ** 32, 0], 0))
    for bad in (1.0, True, torch.ones(4), [1.0, 2.0, 3.0, 4.0], torch.ones(4, dtype=torch.bool)):
        with pytest.raises(TypeError, match="all mask must be an int or integers"):
            topk_rows(q, picked, c, 2, attrs=attrs, where=(0, bad, 0))


def test_masks_become_the_twos_complement_int32():
    from lgcn_amd.recommend import _where_arg

    attrs = torch.zeros(6, dtype=torch.int32)
    got = _where_arg(attrs, (2 ** 31, 2 ** 32 - 1, None), 6, 3)
    assert got.dtype == torch.int32 and got.shape == (3, 3)
    assert got.tolist() == [[-2 ** 31, -1, 0]] * 3
    got = _where_arg(attrs, ([1, 2 ** 31 + 5, 2 ** 31 - 1], torch.tensor([2 ** 32 - 2, 0, 7]), -2 ** 31), 6, 3)
    assert got.tolist() == [[1, -2, -2 ** 31], [-2 ** 31 + 5, 0, -2 ** 31], [2 ** 31 - 1, 7, -2 ** 31]]
    got = _where_arg(attrs, (torch.tensor([-1, 3, 0], dtype=torch.int32), 0, torch.tensor([4, 5, 6], dtype=torch.uint8)),
                     6, 3)
    assert got.tolist() == [[-1, 0, 4], [3, 0, 5], [0, 0, 6]]
    assert _where_arg(attrs, (1, 2, 3), 6, 0).shape == (0, 3)
    assert _where_arg(None, None, 6, 3) is None
    # the bit pattern is what the kernels read as uint32
    assert got.numpy().view("uint32")[0, 0] == 2 ** 32 - 1


def test_harness_genre_errors_come_before_the_library(monkeypatch):
    from utils import recommend as R

    _no_load(monkeypatch)
    for kw in (dict(genres=["Comedy", "Sci-Fi"]), dict(genres_all=["Sci-Fi"]), dict(without_genres=["Sci-Fi"])):
        with pytest.raises(ValueError, match=r"recommend_for_users: unknown genre 'Sci-Fi'.*\['Comedy', 'Horror', "
                                             r"'Romance', 'Western'\]"):
            R.recommend_for_users(None, [7], _Handler, **kw)
        with pytest.raises(ValueError, match=r"recommend_for_histories: unknown genre 'Sci-Fi'.*\['Comedy'"):
            R.recommend_for_histories(None, [[10]], _Handler, **kw)
    assert R._genre_filter("x", _Handler, None, None, None) == {}
    flt = R._genre_filter("x", _Handler, ["Comedy", "Western"], ["Romance"], "Horror")
    assert flt["where"] == (1 | 8, 4, 2) and flt["attrs"].tolist() == [2, 5, 0, 0, 0]
    # unknown ids are still answered without the model or the GPU
    assert R.recommend_for_users(None, [1], _Handler, genres=["Comedy"]) == [{"error": "Invalid user ID"}]
    assert R.recommend_for_histories(None, [[999]], _Handler, genres=["Comedy"]) == [{"error": "No known movie IDs"}]


def test_new_entry_points_check_their_arguments_without_a_device():
    from lgcn_amd import _ffi

    lib = _ffi.load()
    buf = torch.zeros(512, dtype=torch.int32)
    p = buf.data_ptr()  # a host address: an argument check must come back before anything reads it
    filt = lambda thr, attr, where: lib.lgcn_score_filter_attr(p, 128, 4, p, 10, 1, 64, thr, p, p, p, 16, attr, where,
                                                               None)
    assert filt(None, p, p) == _ffi.E_ARG
    msg = lib.lgcn_last_error()
    assert b"lgcn_score_filter_attr" in msg and b"thr is null" in msg
    assert filt(p, None, p) == _ffi.E_ARG and b"lgcn_score_filter_attr: attr is null" in lib.lgcn_last_error()
    assert filt(p, p, None) == _ffi.E_ARG and b"lgcn_score_filter_attr: where is null" in lib.lgcn_last_error()
    assert lib.lgcn_score_filter_attr(p, 128, 4, p, 10, 1, 64, p, p, p, None, 16, p, p, None) == _ffi.E_ARG  # list_n
    assert b"bad args" in lib.lgcn_last_error()
    assert lib.lgcn_score_filter_attr(p, 100, 4, p, 10, 1, 64, p, p, p, p, 16, p, p, None) == _ffi.E_ARG
    assert b"not a multiple of 128" in lib.lgcn_last_error()
    assert lib.lgcn_score_filter_attr(p, 128, 4, p, 10, 1, 48, p, p, p, p, 16, p, p, None) == _ffi.E_UNSUPPORTED
    assert lib.lgcn_score_filter_attr(p, 128, 4, p, 0, 1, 64, p, p, p, p, 16, p, p, None) == 0  # no candidates: no launch
    ranked = lambda attr, where, k=4: lib.lgcn_select_topk_ranked_attr(p, p, None, 8, 16, k, 128, 4, None, None, None, 0,
                                                                       p, None, None, None, attr, where, None)
    assert ranked(None, p) == _ffi.E_ARG and b"lgcn_select_topk_ranked_attr: attr is null" in lib.lgcn_last_error()
    assert ranked(p, None) == _ffi.E_ARG and b"lgcn_select_topk_ranked_attr: where is null" in lib.lgcn_last_error()
    assert ranked(p, p, k=0) == _ffi.E_ARG and b"lgcn_select_topk_ranked_attr: k=0" in lib.lgcn_last_error()
    # the unfiltered entry point keeps its own name in its messages
    assert lib.lgcn_select_topk_ranked(p, p, None, 8, 16, 0, 128, 4, None, None, None, 0, p, None, None, None,
                                       None) == _ffi.E_ARG
    assert b"lgcn_select_topk_ranked: k=0" in lib.lgcn_last_error()
