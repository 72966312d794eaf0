"""Exact ranking positions without a GPU: the numpy checker on hand-made cases,
lgcn_amd.metrics.summarize_positions on CPU tensors against it, the closed-form AUC against pair
counting, rank_positions' refusals (before the library is loaded) and lgcn_rank_positions' argument
checks (before any HIP call)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from rank_position_checker import auc_by_pairs, key_scores, positions_from_keys, summaries64

NAN_KEY = 0xFFFFFFFF


def test_checker_on_hand_made_cases():
    #            0   1   2   3   4   5
    keys = np.array([[50, 90, 50, 10, 90, 50],              # ties: 1 4 | 0 2 5 | 3
                     [7, NAN_KEY, 9, 9, 1, NAN_KEY],        # NaN keys rank first: 1 5 | 2 3 | 0 | 4
                     [5, 4, 3, 2, 1, 6],                    # everything but one candidate seen
                     [1, 2, 3, 4, 5, 6]], dtype=np.uint32)  # empty truth row
    truth = [[5, 0, 3, 1], [5, 2, 0, 7, -1, 3], [4, 2], []]
    seen = [[], [3], [0, 1, 2, 3, 5, 9], [1]]
    ptr, pos, key, eligible = positions_from_keys(keys, lambda q: truth[q], lambda q: seen[q])
    assert ptr.tolist() == [0, 4, 10, 12, 12]
    assert pos[0:4].tolist() == [4, 2, 5, 0]  # equal keys go by index
    # query 1: 3 is seen (never ranked, and it no longer stands above 0); 7 and -1 are out of range
    assert pos[4:10].tolist() == [1, 2, 3, -1, -1, -1]
    assert key[4:10].tolist() == [NAN_KEY, 9, 7, 0, 0, 9]
    assert pos[10:12].tolist() == [0, -1]  # the only eligible candidate; a seen target
    assert eligible.tolist() == [6, 5, 1, 5]  # seen entry 9 is outside [0, M) and takes nothing away
    assert pos.dtype == np.int32 and key.dtype == np.uint32 and eligible.dtype == np.int32
    s = summaries64(ptr, pos, eligible, ks=(1, 3))
    # query 2 has N_neg = 0 (its one eligible candidate is its one ranked target), query 3 no truth
    assert s["users"] == 2
    # query 0: positions {0, 2, 4, 5} of 6: negatives at 1 and 3; correct pairs 2 + 1 + 0 + 0 of 8
    # query 1: positions {1, 2, 3} of 5: negatives at 0 and 4; correct pairs 1 + 1 + 1 of 6
    assert s["auc"] == pytest.approx((3 / 8 + 3 / 6) / 2, abs=1e-15)
    assert s["mrr"] == pytest.approx((1.0 + 0.5) / 2) and s["mean_rank"] == pytest.approx((11 / 4 + 2.0) / 2)
    assert s["mpr"] == pytest.approx((11 / 4 / 5 + 2.0 / 4) / 2)
    assert s["recall@1"] == pytest.approx((1 / 4 + 0) / 2) and s["hit_rate@3"] == 1.0
    assert s["recall@3"] == pytest.approx((2 / 4 + 2 / 6) / 2)  # T is the whole truth row
    assert s["mrr@1"] == pytest.approx(0.5) and s["mrr@3"] == pytest.approx(0.75)
    idcg3 = 1 + 1 / math.log2(3) + 0.5
    assert s["ndcg@3"] == pytest.approx(((1 + 0.5) / idcg3 + (1 / math.log2(3) + 0.5) / idcg3) / 2)
    assert key_scores(np.array([NAN_KEY], np.uint32))[0] != key_scores(np.array([NAN_KEY], np.uint32))[0]  # NaN
    assert key_scores(np.array([0xBF800000], np.uint32))[0] == 1.0


def test_checker_with_no_user_at_all():
    ptr, pos, key, eligible = positions_from_keys(np.zeros((2, 3), np.uint32) + 5, lambda q: [], lambda q: [])
    s = summaries64(ptr, pos, eligible, ks=(2,))
    assert s["users"] == 0 and all(math.isnan(v) for k, v in s.items() if k != "users")
    assert pos.shape == (0,) and eligible.tolist() == [3, 3]


def _random_positions(rng, Q, M):
    """Positions as a ranking would give them: distinct per user, inside [0, eligible), some -1."""
    ptr, pos, eligible = [0], [], []
    for q in range(Q):
        E = int(rng.integers(1, M + 1))
        n = int(rng.integers(0, min(E, 12) + 1))
        if q % 9 == 4:
            n = E = min(E, 6)  # every eligible candidate is a ranked target: N_neg = 0
        row = list(rng.choice(E, n, replace=False)) + [-1] * int(rng.integers(0, 3))
        rng.shuffle(row)
        pos += row
        ptr.append(len(pos))
        eligible.append(E)
    return np.array(ptr, np.int64), np.array(pos, np.int32), np.array(eligible, np.int32)


@pytest.mark.parametrize("ks", [(), (1, 5, 2000), tuple(range(1, 25, 2)), (7, 7, 3)])
def test_summarize_positions_on_cpu_tensors_equals_the_checker(ks):
    from lgcn_amd.metrics import RankPositions, summarize_positions

    rng = np.random.default_rng(len(ks) + 17)
    ptr, pos, eligible = _random_positions(rng, 150, 3000)
    want = summaries64(ptr, pos, eligible, ks)
    got = summarize_positions(RankPositions(torch.from_numpy(ptr), torch.from_numpy(pos),
                                            torch.zeros(len(pos)), torch.from_numpy(eligible)), ks)
    assert len(set(ks)) != 12 or len(want) == 5 + 5 * 12  # twelve cutoffs: above rank_metrics' eight
    assert set(got) == set(want) and got["users"] == want["users"] and 0 < want["users"] < 150
    for name, w in want.items():
        assert abs(got[name] - w) <= 1e-12, (name, got[name], w)
    if 2000 in ks:  # below the ranked lists' cap nothing of this could be seen
        assert want["recall@2000"] > want["recall@5"] and (pos > 1024).any()


def test_summarize_positions_with_nobody_and_bad_cutoffs():
    from lgcn_amd.metrics import RankPositions, summarize_positions

    none = RankPositions(torch.zeros(3, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), torch.zeros(0),
                         torch.tensor([4, 4], dtype=torch.int32))
    s = summarize_positions(none, (3,))
    assert s["users"] == 0 and math.isnan(s["auc"]) and math.isnan(s["recall@3"])
    assert summarize_positions(RankPositions(torch.zeros(1, dtype=torch.int64), none.pos, none.score,
                                             none.eligible[:0]))["users"] == 0
    with pytest.raises(ValueError, match="summarize_positions: cutoffs"):
        summarize_positions(none, (0, 5))


def test_closed_form_auc_equals_pair_counting():
    rng = np.random.default_rng(5)
    for _ in range(200):
        E = int(rng.integers(2, 400))
        n = int(rng.integers(1, min(E, 30)))
        p = rng.choice(E, n, replace=False)
        closed = 1.0 - (p.sum() - n * (n - 1) / 2) / (n * (E - n))
        assert abs(closed - auc_by_pairs(p, E)) <= 1e-12


def _csr():
    return torch.tensor([0, 2, 2, 5], dtype=torch.int64), torch.tensor([1, 4, 0, 2, 3], dtype=torch.int32)


def test_rank_positions_refusals_come_before_the_library(monkeypatch):
    from lgcn_amd import _ffi
    from lgcn_amd.metrics import rank_positions

    def no_load(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(_ffi, "load", no_load)
    ptr, idx = _csr()
    q, c, picked = torch.randn(3, 8), torch.randn(6, 8), torch.arange(3)
    with pytest.raises(TypeError, match="^rank_positions: truth needs ptr int64"):
        rank_positions(q, picked, c, (ptr.tolist(), idx))
    with pytest.raises(ValueError, match=r"^rank_positions: truth is \(ptr, idx\)"):
        rank_positions(q, picked, c, (ptr, idx, picked))
    with pytest.raises(TypeError, match="^rank_positions: truth rows must be integers"):
        rank_positions(q, picked, c, (ptr, idx), rows=torch.tensor([0.0, 1.0, 2.0]))
    with pytest.raises(ValueError, match="^rank_positions: truth rows has 2 entries for 3 queries"):
        rank_positions(q, picked, c, (ptr, idx), rows=[0, 1])
    with pytest.raises(ValueError, match=r"^rank_positions: seen is \(ptr, idx\) or \(ptr, idx, rows\)"):
        rank_positions(q, picked, c, (ptr, idx), seen=(ptr,))
    with pytest.raises(ValueError, match="^rank_positions: seen has 2 rows for 3 queries"):
        rank_positions(q, picked, c, (ptr, idx), seen=(ptr[:3], idx))
    with pytest.raises(ValueError, match="^rank_positions: rows of 300 columns"):
        rank_positions(torch.randn(3, 300), picked, torch.randn(6, 300), (ptr, idx))
    with pytest.raises(ValueError, match="^rank_positions: queries and candidates must have the same width"):
        rank_positions(q, picked, torch.randn(6, 9), (ptr, idx))
    with pytest.raises(TypeError, match="^rank_positions: picked must be integers"):
        rank_positions(q, torch.tensor([0.0, 1.0, 2.0]), c, (ptr, idx))
    monkeypatch.undo()
    with pytest.raises(_ffi.LgcnError, match="rank_positions: the MI355X LightGCN path needs ROCm device tensors"):
        rank_positions(q, picked, c, (ptr, idx))


def test_binding_names_the_entry():
    from lgcn_amd import _ffi

    assert "lgcn_rank_positions" in _ffi.EXPORTED and "lgcn_rank_positions_workspace_size" in _ffi.EXPORTED
    assert "lgcn_rankpos.hip" in _ffi.SOURCES
    assert _ffi.ABI_VERSION == 11


def _args(**over):
    """Host buffers standing in for device memory: every call below is refused, or returns, before
    anything would read them."""
    Q, Qpad, M, D, nnz = 3, 128, 6, 8, 5
    keep = dict(Qn=np.zeros((Qpad, D), np.float32), Cn=np.zeros((M + 1, D), np.float32),
                truth_ptr=np.array([0, 2, 2, 5], np.int64), truth_idx=np.array([1, 4, 0, 2, 3], np.int32),
                seen_ptr=np.array([0, 1, 1, 2], np.int64), seen_idx=np.array([0, 5], np.int32),
                out_ptr=np.array([0, 2, 2, 5], np.int64), pos=np.zeros(nnz, np.int32), key=np.zeros(nnz, np.uint32),
                eligible=np.zeros(Q, np.int32), ws=np.zeros(4096, np.uint8))
    a = {k: v.ctypes.data for k, v in keep.items()}
    a.update(Q=Q, Qpad=Qpad, M=M, D=D, nnz=nnz, truth_row=None, truth_rows=3, seen_row=None, seen_rows=3, ws_bytes=2048, stages=7)
    a["ws"] = (a["ws"] + 255) // 256 * 256
    a.update(over)
    order = ("Qn", "Qpad", "Q", "Cn", "M", "D", "truth_ptr", "truth_idx", "truth_row", "truth_rows", "seen_ptr",
             "seen_idx", "seen_row", "seen_rows", "out_ptr", "nnz", "pos", "key", "eligible", "ws", "ws_bytes", "stages")
    return keep, [a[k] for k in order] + [None]


@pytest.mark.parametrize("over,word", [
    (dict(Qn=None), b"Qn is null"), (dict(Cn=None), b"Cn is null"), (dict(truth_ptr=None), b"truth_ptr is null"),
    (dict(truth_idx=None), b"truth_idx is null"), (dict(seen_idx=None), b"seen_idx is null"),
    (dict(out_ptr=None), b"out_ptr is null"), (dict(pos=None), b"pos_out is null"), (dict(key=None), b"key_out is null"),
    (dict(eligible=None), b"eligible_out is null"), (dict(Qpad=100), b"multiple of 128"), (dict(Q=-1), b"Q=-1"),
    (dict(Q=200), b"Qpad=128"), (dict(M=-2), b"M=-2"), (dict(nnz=-1), b"nnz=-1"), (dict(truth_rows=-1), b"truth_rows=-1"),
    (dict(seen_rows=-1), b"seen_rows=-1"), (dict(stages=0), b"stages=0"), (dict(stages=8), b"stages=8"),
])
def test_entry_refuses_bad_arguments(over, word):
    from lgcn_amd import _ffi

    lib = _ffi.load()
    keep, args = _args(**over)
    assert lib.lgcn_rank_positions(*args) == _ffi.E_ARG
    msg = lib.lgcn_last_error()
    assert b"lgcn_rank_positions" in msg and word in msg, msg


def test_entry_refuses_a_misaligned_table_an_odd_width_and_a_short_workspace():
    from lgcn_amd import _ffi

    lib = _ffi.load()
    keep, args = _args()
    args[3] += 4
    assert lib.lgcn_rank_positions(*args) == _ffi.E_ARG and b"Cn is not 16-byte aligned" in lib.lgcn_last_error()
    for D in (24, 0, 512):
        keep, args = _args(D=D)
        assert lib.lgcn_rank_positions(*args) == _ffi.E_UNSUPPORTED
        assert f"lgcn_rank_positions: D={D}".encode() in lib.lgcn_last_error()
    need = ctypes.c_size_t(0)
    assert lib.lgcn_rank_positions_workspace_size(3, 5, ctypes.byref(need)) == 0 and need.value >= 20
    assert lib.lgcn_rank_positions_workspace_size(3, -1, ctypes.byref(need)) == _ffi.E_ARG
    for over in (dict(ws_bytes=8), dict(ws=None)):
        keep, args = _args(**over)
        assert lib.lgcn_rank_positions(*args) == _ffi.E_WORKSPACE and b"workspace" in lib.lgcn_last_error()


def test_entry_returns_without_a_launch_for_no_queries_and_no_truth():
    from lgcn_amd import _ffi

    lib = _ffi.load()
    for over in (dict(Q=0), dict(nnz=0), dict(Q=0, Qpad=0, seen_ptr=None, seen_idx=None, truth_row=None)):
        keep, args = _args(**over)
        assert lib.lgcn_rank_positions(*args) == 0
