"""lgcn_amd._serving without a GPU and without the library: the one ragged-CSR argument check behind
recommend's excl, explain's and fold-in's history and rank_metrics' truth + rows, and the one int32
image of an index list behind rerank_mmr, explain_rows and rank_metrics."""
import pytest
import torch

# (message prefix, argument name, the caller's Q for a CSR of 3 rows; None: fold-in derives it)
CALLERS = [("recommend", "excl", 3), ("explain", "history", 3), ("fold_in", "history", None), ("rank_metrics", "truth", 3)]


def _csr():
    return torch.tensor([0, 2, 2, 5], dtype=torch.int64), torch.tensor([1, 4, 0, 2, 3], dtype=torch.int32)


@pytest.mark.parametrize("who,name,Q", CALLERS)
def test_csr_arg_refusals_carry_the_callers_prefix(who, name, Q):
    from lgcn_amd._serving import csr_arg

    ptr, idx = _csr()
    for bad in (None, (ptr,), (ptr, idx, None, None)):
        with pytest.raises(ValueError, match=rf"^{who}: {name} is \(ptr, idx\) or \(ptr, idx, rows\)"):
            csr_arg(who, name, bad, Q)
    for bad in ((ptr.to(torch.int32), idx), (ptr, idx.to(torch.int64)), (ptr[:0], idx), (ptr.view(2, 2), idx),
                (ptr, idx.view(5, 1)), (ptr.tolist(), idx), (ptr, idx.numpy())):  # the last two: not tensors
        with pytest.raises(TypeError, match=rf"^{who}: {name} needs ptr int64 \[R \+ 1\] and idx int32"):
            csr_arg(who, name, bad, Q)
    for rows in (torch.tensor([0.0, 1.0, 2.0]), [0.5, 1.0, 2.0], torch.tensor([True, False, True])):
        with pytest.raises(TypeError, match=rf"^{who}: {name} rows must be integers"):
            csr_arg(who, name, (ptr, idx, rows), Q)


@pytest.mark.parametrize("who,name,Q", [c for c in CALLERS if c[2] is not None])
def test_csr_arg_counts_rows_against_the_queries(who, name, Q):
    from lgcn_amd._serving import csr_arg

    ptr, idx = _csr()
    with pytest.raises(ValueError, match=rf"^{who}: {name} rows has 2 entries for 3 queries"):
        csr_arg(who, name, (ptr, idx, [0, 1]), Q)
    with pytest.raises(ValueError, match=rf"^{who}: {name} has 2 rows for 3 queries \(pass the row of each query\)"):
        csr_arg(who, name, (ptr[:3], idx), Q)
    # rank_metrics' contract: queries past the end of the truth CSR have empty rows
    assert csr_arg(who, name, (ptr[:3], idx), Q, short=True)[3] == 3
    with pytest.raises(ValueError, match="rows has 2 entries"):
        csr_arg(who, name, (ptr, idx, [0, 1]), Q, short=True)


def test_csr_arg_returns_the_parts_and_the_query_count():
    from lgcn_amd._serving import csr_arg

    ptr, idx = _csr()
    got = csr_arg("explain", "history", (ptr, idx), 2)  # more CSR rows than queries is fine
    assert got[0] is ptr and got[1] is idx and got[2] is None and got[3] == 2
    assert csr_arg("fold_in", "history", (ptr, idx))[2:] == (None, 3)  # Q derived: every CSR row
    strided = torch.tensor([[2, 9], [-1, 9], [7, 9], [0, 9]], dtype=torch.int32)[:, 0]
    for rows in ([2, -1, 7, 0], (2, -1, 7, 0), strided, torch.tensor([[2, -1], [7, 0]])):
        p, i, r, Q = csr_arg("fold_in", "history", (ptr, idx, rows))  # Q derived: the rows named
        assert p is ptr and i is idx and Q == 4 and r.dim() == 1 and r.tolist() == [2, -1, 7, 0]
        assert not r.dtype.is_floating_point
    assert csr_arg("recommend", "excl", [ptr, idx, strided], 4)[3] == 4  # a list serves as the tuple


def test_float_rows_and_non_tensor_ptr_are_refused_before_the_library(monkeypatch):
    """The two refusals that were fold-in's alone, through a public function whose history check
    comes before the library is loaded."""
    from lgcn_amd import _ffi
    from lgcn_amd.explain import explain_rows

    def no_load(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(_ffi, "load", no_load)
    ptr, idx = _csr()
    rec, cands = torch.zeros((3, 4), dtype=torch.int32), torch.randn(6, 8)
    with pytest.raises(TypeError, match="explain: history rows must be integers"):
        explain_rows(rec, (ptr, idx, torch.tensor([0.0, 1.0, 2.0])), cands)
    with pytest.raises(TypeError, match="explain: history needs ptr int64"):
        explain_rows(rec, (ptr.tolist(), idx), cands)


def test_index_list_sends_values_outside_int32_to_minus_one():
    from lgcn_amd._serving import index_list

    t = torch.tensor([[0, 2 ** 31, -5, 2 ** 31 - 1], [7, 2 ** 32 + 7, -(2 ** 32) + 3, -1]], dtype=torch.int64)
    got, ld = index_list(t)
    assert got.dtype == torch.int32 and ld == 4
    assert got.tolist() == [[0, -1, -1, 2 ** 31 - 1], [7, -1, -1, -1]]
    t32 = torch.tensor([[3, -5, 9]], dtype=torch.int32)  # int32 lists pass as they are, negatives included
    got, ld = index_list(t32)
    assert got is t32 and ld == 3


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_index_list_keeps_row_strided_views_and_copies_the_rest(dtype):
    from lgcn_amd._serving import index_list

    wide = torch.arange(40, dtype=dtype).view(4, 10)
    got, ld = index_list(wide[:, 2:7])  # a column slice: a view of the (converted) wide rows
    assert got.dtype == torch.int32 and got.tolist() == wide[:, 2:7].tolist()
    if dtype == torch.int32:
        assert ld == 10 and got.data_ptr() == wide[:, 2:7].data_ptr() and got.stride() == (10, 1)
    else:  # the int32 image is a new tensor; whatever its layout, ld describes it
        assert got.stride(1) == 1 and ld == got.stride(0) >= 5
    got, ld = index_list(wide[1:2, 2:7])  # one row: its stride means nothing
    assert ld == 5 and got.tolist() == wide[1:2, 2:7].tolist()
    tr = wide.t()  # [10, 4] with adjacent rows, not columns: copied
    got, ld = index_list(tr)
    assert ld == 4 and got.is_contiguous() and got.tolist() == tr.tolist()
    if dtype == torch.int32:
        assert got.data_ptr() != tr.data_ptr()
    got, ld = index_list(wide[:, ::2])  # columns two apart: copied
    assert ld == 5 and got.is_contiguous() and got.tolist() == wide[:, ::2].tolist()
    got, ld = index_list(wide[:0])  # no rows
    assert got.shape == (0, 10) and ld == 10


def test_width_and_weights_checks():
    from lgcn_amd._serving import check_weights, require_index_dtype, width

    assert [width("explain", d) for d in (1, 8, 9, 24, 64, 65, 256)] == [8, 8, 16, 32, 64, 128, 256]
    for d in (0, 257):
        with pytest.raises(ValueError, match=f"^recommend: rows of {d} columns"):
            width("recommend", d)
    check_weights("explain", None, 5)
    check_weights("fold_in", torch.ones(5), 5)
    for bad in (torch.ones(5, dtype=torch.float64), torch.ones(5, 1), [1.0] * 5):
        with pytest.raises(TypeError, match="^fold_in: weights must be 1-D float32"):
            check_weights("fold_in", bad, 5)
    with pytest.raises(ValueError, match="^explain: 4 weights for 5 history entries"):
        check_weights("explain", torch.ones(4), 5)
    require_index_dtype("rerank_mmr", "pool_idx", torch.zeros(1, dtype=torch.int64))
    with pytest.raises(TypeError, match="^rerank_mmr: pool_idx must be int32 or int64, got torch.int16"):
        require_index_dtype("rerank_mmr", "pool_idx", torch.zeros(1, dtype=torch.int16))
