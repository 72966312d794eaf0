"""Explanations without a GPU: lgcn_explain_topr checks its arguments before any HIP call,
lgcn_amd.explain refuses bad arguments before loading anything and CPU tensors after,
history_weights is plain torch (checked on CPU tensors against numpy), and the float64 rule of
explain_checker.py has the properties the GPU tests rely on."""
import ctypes
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from explain_checker import check_lists, explain64, ranked64


def _args(**over):
    """A well-formed lgcn_explain_topr argument list over a host buffer (never launched: every call
    below fails validation first, or has Q = 0), with some arguments replaced."""
    buf = (ctypes.c_char * 256)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16  # Cn must be 16-byte aligned
    a = dict(rec_idx=p, ld=10, k=10, Q=4, hist_ptr=p, hist_idx=p, hist_w=p, hist_row=p, hist_rows=4, Cn=p, M=1000,
             D=64, r=3, out_idx=p, out_val=p, out_n=p, out_sum=p, stream=None)
    a.update(over)
    return buf, list(a.values())


@pytest.mark.parametrize("over,word", [
    (dict(rec_idx=None), b"rec_idx"),
    (dict(hist_ptr=None), b"hist_ptr"),
    (dict(hist_idx=None), b"hist_idx"),
    (dict(Cn=None), b"Cn"),
    (dict(out_idx=None), b"out_idx"),
    (dict(out_val=None), b"out_val"),
    (dict(out_n=None), b"out_n"),
    (dict(k=0), b"k=0"),
    (dict(k=11), b"k=11"),
    (dict(r=0), b"r=0"),
    (dict(r=-2), b"r=-2"),
    (dict(Q=-1), b"Q=-1"),
    (dict(M=-1), b"M=-1"),
    (dict(hist_rows=-1), b"hist_rows=-1"),
    (dict(D=0), b"D=0"),
    (dict(D=6), b"D=6"),
    (dict(D=260), b"D=260"),
])
def test_explain_topr_refuses_bad_arguments(over, word):
    from lgcn_amd import _ffi

    lib = _ffi.load()
    keep, args = _args(**over)
    assert lib.lgcn_explain_topr(*args) == _ffi.E_ARG
    msg = lib.lgcn_last_error()
    assert b"lgcn_explain_topr" in msg and word in msg, msg


def test_explain_topr_refuses_a_misaligned_table():
    from lgcn_amd import _ffi

    lib = _ffi.load()
    keep, args = _args()
    args[9] += 4
    assert lib.lgcn_explain_topr(*args) == _ffi.E_ARG and b"aligned" in lib.lgcn_last_error()


@pytest.mark.parametrize("over,word", [
    (dict(k=65, ld=65), b"LGCN_EXPLAIN_MAX_K"),
    (dict(k=65, ld=100), b"LGCN_EXPLAIN_MAX_K"),
    (dict(r=9), b"LGCN_EXPLAIN_MAX_R"),
])
def test_explain_topr_limits(over, word):
    from lgcn_amd import _ffi

    lib = _ffi.load()
    keep, args = _args(**over)
    assert lib.lgcn_explain_topr(*args) == _ffi.E_UNSUPPORTED
    msg = lib.lgcn_last_error()
    assert b"lgcn_explain_topr" in msg and word in msg, msg


def test_explain_topr_accepts_the_limits_exactly_and_the_optional_nulls():
    """k = 64, r = 8, D = 256 pass every check; with Q = 0 the call then returns OK without a
    launch, so this runs on a machine without a GPU. hist_w, hist_row and out_sum may be NULL."""
    from lgcn_amd import _ffi

    lib = _ffi.load()
    keep, args = _args(k=64, ld=64, r=8, D=256, Q=0)
    assert lib.lgcn_explain_topr(*args) == 0
    keep, args = _args(k=64, ld=64, r=8, D=256, Q=0, hist_w=None, hist_row=None, out_sum=None, hist_rows=0, M=0)
    assert lib.lgcn_explain_topr(*args) == 0


def test_symbol_and_limits_match_the_header():
    from lgcn_amd import _ffi, explain

    text = (ROOT / "include" / "lgcn.h").read_text()
    assert "lgcn_explain_topr" in _ffi.EXPORTED and "lgcn_explain.hip" in _ffi.SOURCES and _ffi.ABI_VERSION == 11
    assert int(re.search(r"#define LGCN_EXPLAIN_MAX_K (\d+)", text).group(1)) == _ffi.EXPLAIN_MAX_K == 64
    assert int(re.search(r"#define LGCN_EXPLAIN_MAX_R (\d+)", text).group(1)) == _ffi.EXPLAIN_MAX_R == 8
    assert (explain.MAX_K, explain.MAX_R) == (64, 8)


def _case(Q=3, k=5, M=50, d=16, dtype=torch.int64):
    g = torch.Generator().manual_seed(0)
    rec = torch.stack([torch.randperm(M, generator=g)[:k] for _ in range(Q)]).to(dtype)
    ptr = torch.arange(0, 4 * (Q + 1), 4, dtype=torch.int64)
    idx = torch.cat([torch.sort(torch.randperm(M, generator=g)[:4]).values for _ in range(Q)]).to(torch.int32)
    return rec, (ptr, idx), torch.randn(M, d, generator=g)


def test_explain_rows_python_argument_errors():
    from lgcn_amd import _ffi
    from lgcn_amd.explain import explain_items, explain_rows

    rec, hist, cands = _case()
    ptr, idx = hist
    with pytest.raises(ValueError, match=r"\[Q, k\]"):
        explain_rows(rec[0], hist, cands)
    with pytest.raises(TypeError, match="rec_idx"):
        explain_rows(rec.to(torch.int16), hist, cands)
    with pytest.raises(TypeError, match="candidates"):
        explain_rows(rec, hist, cands.double())
    with pytest.raises(ValueError, match="k=65"):
        explain_rows(torch.zeros((2, 65), dtype=torch.int32), hist, cands)
    with pytest.raises(ValueError, match="k=0"):
        explain_rows(torch.zeros((2, 0), dtype=torch.int32), hist, cands)
    for r in (0, 9):
        with pytest.raises(ValueError, match=f"r={r}"):
            explain_rows(rec, hist, cands, r=r)
    with pytest.raises(ValueError, match="columns"):
        explain_rows(rec, hist, torch.randn(50, 257))
    # the history, as recommend._excl_args checks excl
    with pytest.raises(ValueError, match="history is"):
        explain_rows(rec, (ptr,), cands)
    with pytest.raises(ValueError, match="history is"):
        explain_rows(rec, None, cands)
    with pytest.raises(TypeError, match="ptr int64"):
        explain_rows(rec, (ptr.to(torch.int32), idx), cands)
    with pytest.raises(TypeError, match="ptr int64"):
        explain_rows(rec, (ptr, idx.to(torch.int64)), cands)
    with pytest.raises(ValueError, match="2 rows for 3 queries"):
        explain_rows(rec, (ptr[:3], idx), cands)
    with pytest.raises(ValueError, match="rows has 2 entries for 3 queries"):
        explain_rows(rec, (ptr, idx, torch.tensor([0, 1])), cands)
    with pytest.raises(TypeError, match="weights"):
        explain_rows(rec, hist, cands, weights=torch.ones(12, dtype=torch.float64))
    with pytest.raises(ValueError, match="11 weights for 12"):
        explain_rows(rec, hist, cands, weights=torch.ones(11))
    for dtype in (torch.int64, torch.int32):  # well-formed, but on the CPU: no fallback
        with pytest.raises(_ffi.LgcnError, match="ROCm device"):
            explain_rows(rec.to(dtype), hist, cands, weights=torch.ones(12))
        with pytest.raises(_ffi.LgcnError, match="ROCm device"):
            explain_rows(rec.to(dtype), hist, cands, r=8, normalized=True)
        with pytest.raises(_ffi.LgcnError, match="ROCm device"):
            explain_items(cands, torch.arange(3), rec.to(dtype), hist)


def test_history_weights_match_numpy():
    from lgcn_amd.explain import history_weights

    rng = np.random.default_rng(2)
    rows = [np.sort(rng.choice(30, n, replace=False)) for n in (0, 1, 7, 30, 0, 3)]
    ptr = np.cumsum([0] + [len(x) for x in rows]).astype(np.int64)
    idx = np.concatenate(rows).astype(np.int32)
    got = history_weights((torch.from_numpy(ptr), torch.from_numpy(idx)))
    assert got.dtype == torch.float32 and got.shape == (idx.size,)
    count = np.bincount(idx, minlength=30)
    want = np.concatenate([1.0 / np.sqrt(len(x) * count[x].astype(np.float64)) for x in rows])
    np.testing.assert_allclose(got.numpy(), want.astype(np.float32), rtol=1e-7)
    # literal: two users sharing item 0, one of them with a second item
    lit = history_weights((torch.tensor([0, 2, 3]), torch.tensor([0, 5], dtype=torch.int32).repeat(2)[:3]))
    assert lit.tolist() == pytest.approx([0.5, 2 ** -0.5, 2 ** -0.5])
    empty = history_weights((torch.zeros(4, dtype=torch.int64), torch.zeros(0, dtype=torch.int32)))
    assert empty.shape == (0,) and empty.dtype == torch.float32


def test_recommend_for_users_explain_answers_unknown_ids_without_a_gpu():
    import pandas as pd

    from lgcn_amd import _ffi
    from models.light_gcn import LightGCN
    from utils import recommend as R

    U, I = 4, 80
    model = LightGCN(U, I, num_layers=1, dim_h=8)

    class H:
        user_id_map = {10 + u: u for u in range(U)}
        movie_id_map = {100 + i: U + i for i in range(I)}
        movies = pd.DataFrame({"movieId": [100 + i for i in range(I)], "title": [f"m{i}" for i in range(I)]})
        edge_index = torch.tensor([[0, 1], [U + 2, U + 3]])

    assert R.recommend_for_users(model, [-1, 99], H, k=5, explain=3) == [{"error": "Invalid user ID"}] * 2
    for bad in (0, 9):
        with pytest.raises(ValueError, match="explain="):
            R.recommend_for_users(model, [-1], H, k=5, explain=bad)
    with pytest.raises(_ffi.LgcnError, match="ROCm device"):  # a known id needs the device
        R.recommend_for_users(model, [10], H, k=5, explain=3)


def test_float64_rule_properties():
    """What the GPU tests lean on, shown on the rule itself (rows with entries k / 8: every dot is
    exact): the list for a smaller r is a prefix, an item is never a reason for itself and is not
    in the total, equal contributions come in ascending item order, NaN ranks last, and the rule's
    own lists pass check_lists, which refuses two reasons swapped, twins out of index order, a
    better item left out and a wrong count."""
    C = np.zeros((41, 8))
    C[30] = [1, 0, 0, 0, 0, 0, 0, 0]
    for i, x in {2: 0.25, 5: 0.75, 9: 0.5, 11: 0.75, 17: -0.125, 23: 0.75, 30: 1.0, 33: 0.375}.items():
        C[i, 0] = x
    items = np.array([2, 5, 9, 11, 17, 23, 30, 41, -3])  # two entries outside [0, M)
    w = np.ones(items.size)
    i8, v8, n8, tot8 = explain64(items, w, C, 30, 8)
    assert n8 == 6 and i8.tolist() == [5, 11, 23, 9, 2, 17, -1, -1]  # 30 itself is not a reason
    assert v8[:6].tolist() == [0.75, 0.75, 0.75, 0.5, 0.25, -0.125] and np.isneginf(v8[6:]).all()
    assert tot8 == 0.75 * 3 + 0.5 + 0.25 - 0.125
    i3, v3, n3, tot3 = explain64(items, w, C, 30, 3)
    assert n3 == 3 and (i3 == i8[:3]).all() and (v3 == v8[:3]).all() and tot3 == tot8
    assert explain64(items, w, C, 41, 3)[2:] == (0, 0.0) and explain64(items, w, C, -1, 3)[2:] == (0, 0.0)
    half = np.where(items == 5, 0.5, 1.0)  # a weight breaks the tie
    assert explain64(items, half, C, 30, 4)[0].tolist() == [11, 23, 9, 5]
    Cn = C.copy()
    Cn[9] = np.nan
    it, c = ranked64(items, w, Cn, 30)
    assert it[-1] == 9 and np.isnan(c[-1]) and np.isnan(explain64(items, w, Cn, 30, 8)[3])
    # check_lists on the rule's own output: slots 30 (in the history), 33 (not in it), 41 (empty)
    ptr, idx = np.array([0, items.size]), items.astype(np.int32)
    rec = np.array([[30, 33, 41]])
    outs = [explain64(items, w, C, j, 5) for j in rec[0]]
    gi = np.stack([o[0] for o in outs])[None]
    gv = np.stack([o[1] for o in outs])[None].astype(np.float32)
    gn = np.array([[o[2] for o in outs]])
    gt = np.array([[o[3] for o in outs]], np.float32)
    assert gn.tolist() == [[5, 5, 0]] and gi[0, 1].tolist() == [30, 5, 11, 23, 9]
    dec, listed = check_lists(rec, ptr, idx, None, None, C, 5, gi, gv, gn, gt)
    assert (dec, listed) == (4, 10)  # the twins are exact ties: not decided, the lower index first

    def refused(**change):
        out = dict(gi=gi.copy(), gv=gv.copy(), gn=gn.copy(), gt=gt.copy())
        for name, (at, value) in change.items():
            out[name][at] = value
        with pytest.raises(AssertionError):
            check_lists(rec, ptr, idx, None, None, C, 5, out["gi"], out["gv"], out["gn"], out["gt"])

    refused(gi=((0, 0, [3, 4]), [2, 9]), gv=((0, 0, [3, 4]), [0.25, 0.5]))  # two reasons swapped
    refused(gi=((0, 0, [0, 1]), [11, 5]))                                  # twins out of index order
    refused(gi=((0, 0, 4), 17), gv=((0, 0, 4), -0.125))                    # a better item (2) left out
    refused(gi=((0, 0, 4), 30), gv=((0, 0, 4), 1.0))                       # the slot's own item listed
    refused(gn=((0, 0), 4))
    refused(gt=((0, 1), float(gt[0, 1]) + 1e-3))
    refused(gi=((0, 2, 0), 5))                                             # an empty slot with an entry

