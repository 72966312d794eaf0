"""Fold-in without a GPU: the float64 rule of foldin_checker.py agrees with a hand-computed case,
lgcn_foldin_rows checks its arguments before any HIP call, lgcn_amd.foldin refuses bad arguments
before loading anything and CPU tensors after, inv_sqrt_degree is plain torch, and
utils.recommend.recommend_for_histories answers histories without a known id without touching the
model."""
import ctypes
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from foldin_checker import exact32, foldin64, scale64, sums64


def test_checker_agrees_with_a_hand_computed_case():
    """Three queries: one empty; one with an entry outside [0, M) (skipped, its weight with it) and a
    repeated entry (counted twice); one through every factor."""
    table = np.array([[1.0, 2.0], [3.0, -4.0], [0.5, 8.0]])
    isd = np.array([0.5, 1.0, 0.25])
    ptr = np.array([0, 0, 4, 6])
    idx = np.array([1, 7, 1, 0, 2, -1], np.int32)
    w = np.array([2.0, 100.0, 1.0, 0.5, 4.0, 9.0])
    total, absum, n = sums64(ptr, idx, w, None, 3, table, isd)
    assert n.tolist() == [0, 3, 1]
    # query 1: 2 * 1 * row1 + 1 * 1 * row1 + 0.5 * 0.5 * row0 = (9.25, -11.5); query 2: 4 * 0.25 * row2
    assert total.tolist() == [[0.0, 0.0], [9.25, -11.5], [0.5, 8.0]]
    assert absum.tolist() == [[0.0, 0.0], [9.25, 12.5], [0.5, 8.0]]
    assert scale64(n).tolist() == [0.0, 1.0 / np.sqrt(3.0), 1.0]
    out, n2, bound = foldin64(ptr, idx, w, None, 3, table, isd)
    assert (n2 == n).all() and out[0].tolist() == [0.0, 0.0] and out[2].tolist() == [0.5, 8.0]
    np.testing.assert_allclose(out[1], [9.25 / 3 ** 0.5, -11.5 / 3 ** 0.5], rtol=1e-15)
    np.testing.assert_allclose(bound[1], [11 * 2.0 ** -24 * 9.25 / 3 ** 0.5, 11 * 2.0 ** -24 * 12.5 / 3 ** 0.5], rtol=1e-15)
    assert bound[0].tolist() == [0.0, 0.0]
    # without the factors, through rows: query 0 -> row 2, query 1 -> a row outside the CSR
    out, n3, _ = foldin64(ptr, idx, None, np.array([2, 5]), 2, table, None)
    assert n3.tolist() == [1, 0] and out.tolist() == [[0.5, 8.0], [0.0, 0.0]]
    # the exact form: f32(sum) * f32(s)
    e, _ = exact32(ptr, idx, w, None, 3, table, isd)
    assert e.dtype == np.float32 and e[1].tolist() == [np.float32(9.25) * np.float32(1 / np.sqrt(3.0)),
                                                       np.float32(-11.5) * np.float32(1 / np.sqrt(3.0))]


def _args(**over):
    """A well-formed lgcn_foldin_rows argument list over a host buffer (never launched: every call
    below fails validation first, or has Q = 0), with some arguments replaced."""
    buf = (ctypes.c_char * 256)()
    p = ctypes.addressof(buf)
    a = dict(hist_ptr=p, hist_idx=p, hist_w=p, hist_row=p, hist_rows=4, Q=4, table=p, M=1000, d=64, ldt=64, isd=p,
             out=p, ldo=64, out_n=p, stream=None)
    a.update(over)
    return buf, list(a.values())


@pytest.mark.parametrize("over,word", [
    (dict(hist_ptr=None), b"hist_ptr"),
    (dict(hist_idx=None), b"hist_idx"),
    (dict(table=None), b"table"),
    (dict(out=None), b"out is null"),
    (dict(Q=-1), b"Q=-1"),
    (dict(M=-1), b"M=-1"),
    (dict(hist_rows=-1), b"hist_rows=-1"),
    (dict(d=0), b"d=0"),
    (dict(d=-3), b"d=-3"),
    (dict(ldt=63), b"ldt=63"),
    (dict(ldo=63), b"ldo=63"),
    (dict(d=100, ldt=100, ldo=99), b"ldo=99"),
    (dict(ldt=2**31), b"ldt=2147483648"),
    (dict(Q=2**31), b"Q=2147483648"),
])
def test_foldin_rows_refuses_bad_arguments(over, word):
    from lgcn_amd import _ffi

    lib = _ffi.load()
    keep, args = _args(**over)
    assert lib.lgcn_foldin_rows(*args) == _ffi.E_ARG
    msg = lib.lgcn_last_error()
    assert b"lgcn_foldin_rows" in msg and word in msg, msg


def test_foldin_rows_limit_and_optional_nulls():
    """d = 257 is unsupported; d = 256 passes every check and with Q = 0 returns OK without a launch,
    so this runs on a machine without a GPU. hist_w, hist_row, isd and out_n may be NULL."""
    from lgcn_amd import _ffi

    lib = _ffi.load()
    keep, args = _args(d=257, ldt=300, ldo=300)
    assert lib.lgcn_foldin_rows(*args) == _ffi.E_UNSUPPORTED
    msg = lib.lgcn_last_error()
    assert b"lgcn_foldin_rows" in msg and b"LGCN_FOLDIN_MAX_D" in msg, msg
    keep, args = _args(d=256, ldt=256, ldo=300, Q=0)
    assert lib.lgcn_foldin_rows(*args) == 0
    keep, args = _args(d=1, ldt=1, ldo=1, Q=0, hist_w=None, hist_row=None, isd=None, out_n=None, hist_rows=0, M=0)
    assert lib.lgcn_foldin_rows(*args) == 0


def test_symbol_and_constants_match_the_header():
    from lgcn_amd import _ffi, foldin

    text = (ROOT / "include" / "lgcn.h").read_text()
    assert "lgcn_foldin_rows" in _ffi.EXPORTED and "lgcn_foldin.hip" in _ffi.SOURCES and _ffi.ABI_VERSION == 11
    for name, value in (("MAX_D", _ffi.FOLDIN_MAX_D), ("LONG", _ffi.FOLDIN_LONG), ("CHUNK", _ffi.FOLDIN_CHUNK)):
        assert int(re.search(rf"#define LGCN_FOLDIN_{name} (\d+)", text).group(1)) == value
    assert (foldin.MAX_D, foldin.LONG, foldin.CHUNK) == (256, _ffi.FOLDIN_LONG, _ffi.FOLDIN_CHUNK)
    assert _ffi.FOLDIN_LONG >= 64 and _ffi.FOLDIN_CHUNK % 64 == 0


def _case(Q=3, M=50, d=16):
    g = torch.Generator().manual_seed(0)
    ptr = torch.arange(0, 4 * (Q + 1), 4, dtype=torch.int64)
    idx = torch.cat([torch.randperm(M, generator=g)[:4] for _ in range(Q)]).to(torch.int32)
    return (ptr, idx), torch.randn(M, d, generator=g)


def test_python_argument_errors_come_before_the_library(monkeypatch):
    from lgcn_amd import _ffi
    from lgcn_amd.foldin import fold_in, fold_in_rows, layer_tables

    hist, table = _case()
    ptr, idx = hist

    def no_load(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")

    with monkeypatch.context() as m:
        m.setattr(_ffi, "load", no_load)
        for f in (fold_in_rows, fold_in):
            with pytest.raises(ValueError, match="history is"):
                f((ptr,), table)
            with pytest.raises(ValueError, match="history is"):
                f(None, table)
            with pytest.raises(TypeError, match="ptr int64"):
                f((ptr.to(torch.int32), idx), table)
            with pytest.raises(TypeError, match="ptr int64"):
                f((ptr, idx.to(torch.int64)), table)
            with pytest.raises(TypeError, match="rows must be integers"):
                f((ptr, idx, torch.tensor([0.5])), table)
            with pytest.raises(TypeError, match="table"):
                f(hist, table.double())
            with pytest.raises(TypeError, match="table"):
                f(hist, table[0])
            with pytest.raises(ValueError, match="257 columns"):
                f(hist, torch.zeros(50, 257))
            with pytest.raises(TypeError, match="weights"):
                f(hist, table, weights=torch.ones(12, dtype=torch.float64))
            with pytest.raises(ValueError, match="11 weights for 12"):
                f(hist, table, weights=torch.ones(11))
        with pytest.raises(TypeError, match="isd"):
            fold_in_rows(hist, table, isd=torch.ones(50, dtype=torch.float64))
        with pytest.raises(ValueError, match="49 isd factors for 50"):
            fold_in_rows(hist, table, isd=torch.ones(49))
        with pytest.raises(ValueError, match="count"):
            fold_in(hist, table, count=torch.ones(49))
        with pytest.raises(ValueError, match="count"):
            fold_in(hist, table, count=torch.ones(50, 1))
        with pytest.raises(ValueError, match="K=0"):
            layer_tables(table[:20], table[20:], None, 0)
        with pytest.raises(TypeError, match="user_w"):
            layer_tables(table[:20].double(), table[20:], None, 2)
        with pytest.raises(ValueError, match="widths differ"):
            layer_tables(table[:20, :8], table[20:], None, 2)

        class Plan:
            num_nodes = 49

        with pytest.raises(ValueError, match="49 nodes"):
            layer_tables(table[:20], table[20:], Plan, 2)
    # well-formed, but on the CPU: no fallback
    with pytest.raises(_ffi.LgcnError, match="ROCm device"):
        fold_in_rows(hist, table)
    with pytest.raises(_ffi.LgcnError, match="ROCm device"):
        fold_in(hist, table, count=torch.ones(50), weights=torch.ones(12))
    Plan.num_nodes = 50
    with pytest.raises(_ffi.LgcnError, match="ROCm device"):
        layer_tables(table[:20], table[20:], Plan, 2)


def test_inv_sqrt_degree():
    from lgcn_amd.foldin import inv_sqrt_degree

    count = torch.tensor([0, 1, 3, 8, 58571])
    got = inv_sqrt_degree(count)
    assert got.dtype == torch.float32 and got.shape == (5,)
    want = (1.0 / np.sqrt(np.array([1, 2, 4, 9, 58572], np.float64))).astype(np.float32)
    assert got.numpy().tolist() == want.tolist()
    bare = inv_sqrt_degree(count, new_edge=False)
    assert bare[0] == 0 and bare[1:].numpy().tolist() == \
        (1.0 / np.sqrt(np.array([1, 3, 8, 58571], np.float64))).astype(np.float32).tolist()
    assert inv_sqrt_degree(torch.tensor([3.0, 0.0]), new_edge=False).tolist() == [np.float32(1 / np.sqrt(3.0)), 0.0]
    assert inv_sqrt_degree(torch.zeros(0, dtype=torch.int64)).shape == (0,)
    with pytest.raises(ValueError, match="1-D"):
        inv_sqrt_degree(torch.ones(2, 2))


class _NoModel:
    """Stands where a model would: any use of it is an error."""

    def __getattr__(self, name):
        raise AssertionError(f"the model was touched ({name})")


def _handler(U=4, I=80):
    import pandas as pd

    class H:
        user_id_map = {10 + u: u for u in range(U)}
        movie_id_map = {100 + i: U + i for i in range(I)}
        movies = pd.DataFrame({"movieId": [100 + i for i in range(I)], "title": [f"m{i}" for i in range(I)]})
        edge_index = torch.tensor([[0, 1], [U + 2, U + 3]])

    return H


def test_recommend_for_histories_answers_unknown_ids_without_the_model():
    from lgcn_amd import _ffi
    from models.light_gcn import LightGCN
    from utils import recommend as R

    H = _handler()
    err = {"error": "No known movie IDs"}
    assert R.recommend_for_histories(_NoModel(), [[1, 2, 3], [], [99, 180]], H, k=5, explain=3) == [err] * 3
    assert R.recommend_for_histories(_NoModel(), [], H) == []
    assert R.recommend_for_histories(_NoModel(), [[7]], H, embeddings="propagated", diversity=0.5, pool=20) == [err]
    with pytest.raises(ValueError, match="embeddings"):
        R.recommend_for_histories(_NoModel(), [[100]], H, embeddings="cooked")
    with pytest.raises(ValueError, match="pool"):
        R.recommend_for_histories(_NoModel(), [[100]], H, pool=20)
    for bad in (0, 9):
        with pytest.raises(ValueError, match="explain="):
            R.recommend_for_histories(_NoModel(), [[100]], H, explain=bad)
    with pytest.raises(ValueError, match="1 weight lists for 2"):
        R.recommend_for_histories(_NoModel(), [[100], [101]], H, weights=[[1.0]])
    with pytest.raises(ValueError, match="2 ids and 1 weights"):
        R.recommend_for_histories(_NoModel(), [[100, 101]], H, weights=[[1.0]])
    model = LightGCN(4, 80, num_layers=1, dim_h=8)
    with pytest.raises(_ffi.LgcnError, match="ROCm device"):  # a known id needs the device
        R.recommend_for_histories(model, [[1], [100, 105]], H, k=5)


def test_evaluate_fold_in_checks_its_mode_first():
    from utils.ranking_eval import evaluate_fold_in

    with pytest.raises(ValueError, match="embeddings"):
        evaluate_fold_in(_NoModel(), None, None, None, "cpu", embeddings="cooked")
