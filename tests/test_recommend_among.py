"""Per-query candidate sets without a GPU: candidate_csr, the argument errors of
lgcn_amd.recommend.topk_rows' among (all raised before the library is loaded), lgcn_score_lists'
argument checks (codes and messages, no device touched), the block plan, and the CLI's --among."""
import pandas as pd
import pytest
import torch


def _no_load(monkeypatch):
    from lgcn_amd import _ffi

    def no_load(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(_ffi, "load", no_load)


def test_candidate_csr_from_sequences_and_from_a_padded_tensor():
    from lgcn_amd.recommend import candidate_csr

    ptr, idx = candidate_csr([[5, 1, 5, 3], [], (2,), torch.tensor([7, -1, 0, 7]), [-4]])
    assert ptr.dtype == torch.int64 and idx.dtype == torch.int32 and ptr.device.type == "cpu"
    assert ptr.tolist() == [0, 3, 3, 4, 6, 6]  # empty rows kept, negatives dropped
    assert idx.tolist() == [1, 3, 5, 2, 0, 7]  # ascending and deduplicated within a row
    padded = torch.tensor([[5, 1, 5, 3], [-1, -1, -1, -1], [2, -1, -1, -1], [7, -1, 0, 7]], dtype=torch.int32)
    p2, i2 = candidate_csr(padded)
    assert p2.tolist() == [0, 3, 3, 4, 6] and i2.tolist() == [1, 3, 5, 2, 0, 7] and i2.dtype == torch.int32
    p3, i3 = candidate_csr([])
    assert p3.tolist() == [0] and i3.numel() == 0
    p4, i4 = candidate_csr(torch.zeros((3, 0), dtype=torch.int64))
    assert p4.tolist() == [0, 0, 0, 0] and i4.numel() == 0
    with pytest.raises(TypeError, match="integer"):
        candidate_csr(torch.zeros((2, 2)))
    with pytest.raises(TypeError, match="integers"):
        candidate_csr([[0.5, 1.0]])
    with pytest.raises(ValueError, match="int32"):
        candidate_csr([[2 ** 31]])


def test_among_argument_errors_come_before_the_library(monkeypatch):
    from lgcn_amd import _ffi
    from lgcn_amd.recommend import topk_rows

    _no_load(monkeypatch)
    q, c = torch.randn(3, 8), torch.randn(6, 8)
    ptr, idx = torch.tensor([0, 2, 2, 5], dtype=torch.int64), torch.tensor([1, 4, 0, 2, 3], dtype=torch.int32)
    call = lambda among, **kw: topk_rows(q, torch.arange(3), c, 2, among=among, **kw)
    for bad in ((ptr,), (ptr, idx, None, None)):
        with pytest.raises(ValueError, match=r"^recommend: among is \(ptr, idx\) or \(ptr, idx, rows\)"):
            call(bad)
    for bad in ((ptr.to(torch.int32), idx), (ptr, idx.to(torch.int64)), (ptr.tolist(), idx), (ptr, idx.view(5, 1))):
        with pytest.raises(TypeError, match=r"^recommend: among needs ptr int64 \[R \+ 1\] and idx int32"):
            call(bad)
    with pytest.raises(TypeError, match="^recommend: among rows must be integers"):
        call((ptr, idx, torch.tensor([0.0, 1.0, 2.0])))
    with pytest.raises(ValueError, match="^recommend: among rows has 2 entries for 3 queries"):
        call((ptr, idx, [0, 1]))
    with pytest.raises(ValueError, match=r"^recommend: among has 2 rows for 3 queries"):
        call((ptr[:3], idx))
    for kw in (dict(cap=64), dict(subset=16), dict(cap=64, subset=16)):
        with pytest.raises(ValueError, match="cap= and subset= have no meaning with among="):
            call((ptr, idx), **kw)
    # a row the ranked selection cannot hold: the length is named (a CSR of lengths only; idx is never read)
    n = _ffi.RANKED_MAX_CAP + 1
    long_ptr = torch.tensor([0, 3, 3 + n, 3 + n], dtype=torch.int64)
    long_idx = torch.zeros(3 + n, dtype=torch.int32)
    with pytest.raises(ValueError, match=f"among row has {n} entries"):
        call((long_ptr, long_idx))
    with pytest.raises(ValueError, match=f"among row has {n} entries"):
        call((long_ptr, long_idx, [0, 1, 1]))
    with pytest.raises(AssertionError, match="the library was loaded"):  # queries that avoid the long row get that far
        call((long_ptr, long_idx, [0, 2, 0]))
    with pytest.raises(ValueError, match=r"k=0 outside"):
        topk_rows(q, torch.arange(3), c, 0, among=(ptr, idx))


def test_block_plan_follows_the_sorted_lengths():
    from lgcn_amd.recommend import _among_blocks

    # capacity = max(k, the block's first = longest row); at most bytes // (8 * capacity) queries, at least one
    assert _among_blocks([4097, 33, 33, 31, 1, 0], 10, 8 * 33 * 2) == [(0, 1, 4097), (1, 3, 33), (3, 5, 31), (5, 6, 10)]
    assert _among_blocks([4097, 33, 33, 31, 1, 0], 10, 1 << 30) == [(0, 6, 4097)]
    assert _among_blocks([], 10, 1 << 30) == []
    assert _among_blocks([5, 5, 5], 100, 8 * 100 * 2) == [(0, 2, 100), (2, 3, 100)]


def test_score_lists_checks_its_arguments_without_a_device():
    from lgcn_amd import _ffi

    assert "lgcn_recall_among.hip" in _ffi.SOURCES and "lgcn_score_lists" in _ffi.EXPORTED
    lib = _ffi.load()
    buf = torch.zeros(512, dtype=torch.int32)
    p = buf.data_ptr()  # a host address: an argument check must come back before anything reads it
    names = ["Qn", "Cn", "among_ptr", "among_idx", "list_key", "list_idx", "list_n"]

    def call(null=None, D=64, cap=16, Q=4):
        a = {n: (None if n == null else p) for n in names}
        return lib.lgcn_score_lists(a["Qn"], Q, a["Cn"], 10, D, a["among_ptr"], a["among_idx"], None, 3, a["list_key"],
                                    a["list_idx"], a["list_n"], cap, None)

    for n in names:
        assert call(null=n) == _ffi.E_ARG
        assert f"lgcn_score_lists: {n} is null".encode() in lib.lgcn_last_error()
    for cap in (0, -3):
        assert call(cap=cap) == _ffi.E_ARG and f"lgcn_score_lists: cap={cap}".encode() in lib.lgcn_last_error()
    for D in (0, 7, 48, 100, 512):
        assert call(D=D) == _ffi.E_ARG and f"lgcn_score_lists: D={D}".encode() in lib.lgcn_last_error()
    assert call(Q=-1) == _ffi.E_ARG and b"Qvalid=-1" in lib.lgcn_last_error()
    assert call(Q=0) == 0  # no queries: no launch, nothing read


class _Handler:
    user_id_map = {7: 0, 8: 1, 9: 2}
    movie_id_map = {30: 3, 10: 4, 50: 5, 20: 6, 40: 7}
    movies = pd.DataFrame({"movieId": [10, 20, 30, 40, 50], "title": list("abcde"), "genres": ["Comedy"] * 5})


def test_harness_among_forms_and_the_cli_option():
    from utils import recommend as R

    served = [(0, 7), (2, 9)]  # users 7 and 9 of the inputs [7, 999, 9]
    assert R._among_csr("x", None, 3, served, _Handler, None) == {}
    ptr, idx, rows = R._among_csr("x", [40, 10, 10, 77], 3, served, _Handler, None)["among"]  # shared; 77 unknown
    assert ptr.tolist() == [0, 2] and idx.tolist() == [1, 4] and rows.tolist() == [0, 0]
    ptr, idx = R._among_csr("x", {9: [20, 30], 8: [10]}, 3, served, _Handler, None)["among"]  # 7 is missing: empty
    assert ptr.tolist() == [0, 0, 2] and idx.tolist() == [0, 3]
    ptr, idx = R._among_csr("x", [[50], [10], (40, 40, 999)], 3, served, _Handler, None)["among"]  # aligned with the inputs
    assert ptr.tolist() == [0, 1, 2] and idx.tolist() == [2, 4]
    with pytest.raises(ValueError, match="among holds 2 sets for 3 entries"):
        R._among_csr("x", [[50], [10]], 3, served, _Handler, None)
    assert R._among_csr("x", [], 3, served, _Handler, None)["among"][0].tolist() == [0, 0]  # an empty shared set
    # unknown users and histories are answered without the model, among or not
    assert R.recommend_for_users(None, [1], _Handler, among=[10]) == [{"error": "Invalid user ID"}]
    assert R.recommend_for_histories(None, [[999]], _Handler, among=[10]) == [{"error": "No known movie IDs"}]
    argv = ["recommend.py", "5", "--among", "1, 296,318", "--genres", "Comedy"]
    assert R._cli_ids(R._cli_option(argv, "--among")) == [1, 296, 318]
    assert argv == ["recommend.py", "5", "--genres", "Comedy"]
    assert R._cli_option(argv, "--among") is None and R._cli_ids(None) is None
    assert R._cli_option(argv, "--genres") == ["Comedy"] and argv == ["recommend.py", "5"]
