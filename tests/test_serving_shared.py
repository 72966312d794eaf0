"""The pieces lgcn_amd._serving shares between recall, recommend and metrics, without a GPU: row
lengths as the kernels read them, a CSR argument's device tensors and block addresses, the host
image of lgcn_recall_width, the longest-first order and its way back; that topk_rows checks excl
before the library on every path; and that utils.recommend's two batch calls keep their refusals."""
import ctypes

import pandas as pd
import pytest
import torch


def _csr():
    return torch.tensor([0, 2, 2, 5], dtype=torch.int64), torch.tensor([1, 4, 0, 2, 3], dtype=torch.int32)


def _no_load(monkeypatch):
    from lgcn_amd import _ffi

    def no_load(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(_ffi, "load", no_load)


def test_row_lengths():
    from lgcn_amd._serving import row_lengths

    ptr, _ = _csr()
    got = row_lengths(ptr, None, 3)
    assert got.dtype == torch.int64 and got.tolist() == [2, 0, 3]
    assert row_lengths(ptr, None, 2).tolist() == [2, 0]  # fewer queries than CSR rows
    # rows outside the CSR (-1, R) are empty; a row named twice counts for both queries
    for rows in (torch.tensor([-1, 3, 2, 2, 0]), torch.tensor([-1, 3, 2, 2, 0], dtype=torch.int32)):
        got = row_lengths(ptr, rows, 5)
        assert got.dtype == torch.int64 and got.tolist() == [0, 0, 3, 3, 2]
    none = torch.zeros(1, dtype=torch.int64)  # R == 0: every query's row is outside
    assert row_lengths(none, None, 4).tolist() == [0] * 4
    assert row_lengths(none, torch.tensor([0, -1, 7]), 3).tolist() == [0] * 3
    assert row_lengths(ptr, None, 0).tolist() == []


@pytest.mark.parametrize("a", [0, 128])
def test_csr_at_forms_the_block_addresses(a):
    from lgcn_amd._serving import csr_at

    R = 300
    ptr = torch.arange(R + 1, dtype=torch.int64)
    idx = torch.zeros(R, dtype=torch.int32)
    rows = torch.arange(R, dtype=torch.int64)
    assert csr_at(ptr, idx, rows, a) == (ptr.data_ptr(), idx.data_ptr(), rows.data_ptr() + 8 * a, R)
    assert csr_at(ptr, idx, None, a) == (ptr.data_ptr() + 8 * a, idx.data_ptr(), None, R - a)
    assert csr_at(None, None, None, a) == (None, None, None, 0)  # an absent argument


def test_csr_on_gives_the_library_an_address_and_int64_rows():
    from lgcn_amd._serving import csr_on

    ptr, idx = _csr()
    cpu = torch.device("cpu")
    p, i, r = csr_on(cpu, ptr, idx, None)
    assert p.data_ptr() == ptr.data_ptr() and i.data_ptr() == idx.data_ptr() and r is None  # nothing to move or copy
    p, i, r = csr_on(cpu, torch.zeros(4, dtype=torch.int64), idx[:0], None)
    assert i.numel() == 1 and i.dtype == torch.int32 and p.tolist() == [0] * 4
    strided = torch.tensor([[2, 9], [-1, 9], [0, 9]], dtype=torch.int32)[:, 0]
    assert not strided.is_contiguous()
    p, i, r = csr_on(cpu, ptr, idx, strided)
    assert r.dtype == torch.int64 and r.is_contiguous() and r.tolist() == [2, -1, 0]
    wide = torch.arange(12, dtype=torch.int64)[::2][:4]  # a strided ptr comes back contiguous
    assert csr_on(cpu, wide, idx, None)[0].is_contiguous()


def test_width_and_padded_are_lgcn_recall_width():
    """The library loads without a device; lgcn_recall_width touches none."""
    from lgcn_amd import _ffi, _serving

    lib = _ffi.load()
    for d in range(1, 257):
        D, qm = ctypes.c_int32(0), ctypes.c_int32(0)
        _ffi.check(lib.lgcn_recall_width(d, ctypes.byref(D), ctypes.byref(qm)), "lgcn_recall_width")
        assert (_serving.width("x", d), _serving.QUERY_MULTIPLE) == (D.value, qm.value), d
    assert [_serving.padded(Q) for Q in (0, 1, 127, 128, 129, 256, 300)] == [128, 128, 128, 128, 256, 256, 384]


def test_longest_first_is_stable_and_comes_back():
    from lgcn_amd._serving import in_caller_order, longest_first, rows_in

    lens = torch.tensor([3, 7, 3, 0, 7, 1])
    sorted_lens, order = longest_first(lens)
    assert sorted_lens.tolist() == [7, 7, 3, 3, 1, 0] and order.tolist() == [1, 4, 0, 2, 5, 3]  # equal rows keep their order
    assert rows_in(order, None) is order  # row q is query q's: the order names the rows
    rows = torch.tensor([10, 11, 12, 13, 14, 15])
    assert rows_in(order, rows).tolist() == [11, 14, 10, 12, 15, 13] and rows_in(order, rows).is_contiguous()
    per_query = torch.arange(12).view(6, 2)[order]  # results in the sorted order ...
    assert torch.equal(in_caller_order(order, per_query), torch.arange(12).view(6, 2))  # ... and back


def test_unit_queries_zero_pads_given_unit_rows():
    from lgcn_amd._serving import unit_queries

    q = torch.arange(12, dtype=torch.float32).view(4, 3)
    got = unit_queries(None, q, torch.tensor([2, 0, 2]), 8, 5, True, None)  # normalized: the library is not called
    assert got.shape == (5, 8) and got.dtype == torch.float32
    assert torch.equal(got[:3, :3], q[[2, 0, 2]]) and not got[:3, 3:].any() and not got[3:].any()


def test_excl_is_checked_before_the_library_on_every_path(monkeypatch):
    from lgcn_amd.recommend import topk_rows

    _no_load(monkeypatch)
    q, c = torch.randn(3, 8), torch.randn(6, 8)
    ptr, idx = _csr()
    attrs = torch.zeros(6, dtype=torch.int32)
    # dense, filtered and attribute-filtered calls, and the among path as before
    for kw in ({}, dict(cap=4, subset=2), dict(attrs=attrs, where=(1, 0, 0)), dict(among=(ptr, idx))):
        call = lambda excl: topk_rows(q, torch.arange(3), c, 2, excl=excl, **kw)
        for bad in ((ptr,), (ptr, idx, None, None)):
            with pytest.raises(ValueError, match=r"^recommend: excl is \(ptr, idx\) or \(ptr, idx, rows\)"):
                call(bad)
        for bad in ((ptr.to(torch.int32), idx), (ptr, idx.to(torch.int64)), (ptr[:0], idx), (ptr.view(2, 2), idx),
                    (ptr, idx.view(5, 1)), (ptr.tolist(), idx), (ptr, idx.numpy())):
            with pytest.raises(TypeError, match=r"^recommend: excl needs ptr int64 \[R \+ 1\] and idx int32"):
                call(bad)
        for rows in (torch.tensor([0.0, 1.0, 2.0]), [0.5, 1.0, 2.0], torch.tensor([True, False, True])):
            with pytest.raises(TypeError, match="^recommend: excl rows must be integers"):
                call((ptr, idx, rows))
        with pytest.raises(ValueError, match="^recommend: excl rows has 2 entries for 3 queries"):
            call((ptr, idx, [0, 1]))
        with pytest.raises(ValueError, match=r"^recommend: excl has 2 rows for 3 queries"):
            call((ptr[:3], idx))
        with pytest.raises(AssertionError, match="the library was loaded"):  # a well-formed excl gets that far
            call((ptr, idx))


class _Handler:
    user_id_map = {7: 0, 8: 1, 9: 2}
    movie_id_map = {30: 3, 10: 4, 50: 5, 20: 6, 40: 7}
    movies = pd.DataFrame({"movieId": [10, 20, 30, 40, 50], "title": list("abcde"), "genres": ["Comedy"] * 5})


def test_batch_calls_keep_their_refusals_and_answer_unknown_ids_without_the_model(monkeypatch):
    from lgcn_amd import explain
    from utils import recommend as R

    _no_load(monkeypatch)
    calls = {"recommend_for_users": lambda **kw: R.recommend_for_users(None, [7], _Handler, **kw),
             "recommend_for_histories": lambda **kw: R.recommend_for_histories(None, [[10]], _Handler, **kw)}
    for who, call in calls.items():
        with pytest.raises(ValueError, match=f"^{who}: pool is the re-rank's pool and needs diversity$"):
            call(pool=32)
        for r in (0, explain.MAX_R + 1):
            with pytest.raises(ValueError, match=rf"^{who}: explain={r} outside \[1, {explain.MAX_R}\]$"):
                call(explain=r)
        assert R._check_options(who, None, None, None) is None and R._check_options(who, 0.5, 32, "3") == 3
    # unknown ids: answered on the host whatever else is asked for (the model is None)
    opts = dict(diversity=0.3, pool=32, explain=2, genres=["Comedy"], among=[10])
    assert R.recommend_for_users(None, [1, 2], _Handler, **opts) == [{"error": "Invalid user ID"}] * 2
    assert R.recommend_for_histories(None, [[999], []], _Handler, **opts) == [{"error": "No known movie IDs"}] * 2
