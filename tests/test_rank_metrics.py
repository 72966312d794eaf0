"""Full-ranking evaluation without a GPU: lgcn_rank_metrics checks its arguments before any HIP
call, lgcn_amd.metrics.summarize is plain torch (checked on CPU tensors against literal numbers
and a float64 numpy restatement), and rank_metrics refuses bad cutoffs and CPU tensors."""
import ctypes
import math

import numpy as np
import pytest
import torch

from rank_metrics_checker import summarize64


def _metric_args(values=(5, 10), **over):
    """A well-formed lgcn_rank_metrics argument list over host buffers (never launched: every call
    below must fail validation first, or has Q = 0), with some arguments replaced."""
    buf = (ctypes.c_int64 * 16)()
    p = ctypes.addressof(buf)
    cut = (ctypes.c_int32 * max(len(values), 1))(*values)
    a = dict(ranked_idx=p, ld=10, k=10, Q=4, truth_ptr=p, truth_idx=p, truth_row=None, truth_rows=4,
             cutoffs=ctypes.addressof(cut), n_cutoffs=len(values), hits_out=p, dcg_out=p, first_out=p, ntruth_out=p,
             stream=None)
    a.update(over)
    return (buf, cut), list(a.values())


@pytest.mark.parametrize("over,word", [
    (dict(ranked_idx=None), b"ranked_idx"),
    (dict(truth_ptr=None), b"truth_ptr"),
    (dict(truth_idx=None), b"truth_idx"),
    (dict(cutoffs=None), b"cutoffs"),
    (dict(hits_out=None), b"hits_out"),
    (dict(dcg_out=None), b"dcg_out"),
    (dict(first_out=None), b"first_out"),
    (dict(ntruth_out=None), b"ntruth_out"),
    (dict(k=0, ld=0), b"k=0"),
    (dict(k=1025, ld=1025), b"k=1025"),
    (dict(ld=9), b"ld=9"),
    (dict(Q=-1), b"Q=-1"),
    (dict(truth_rows=-1), b"truth_rows=-1"),
    (dict(n_cutoffs=0), b"n_cutoffs=0"),
    (dict(n_cutoffs=9), b"n_cutoffs=9"),
])
def test_rank_metrics_refuses_bad_arguments(over, word):
    from lgcn_amd import _ffi

    lib = _ffi.load()
    keep, args = _metric_args(**over)
    assert lib.lgcn_rank_metrics(*args) == _ffi.E_ARG
    msg = lib.lgcn_last_error()
    assert b"lgcn_rank_metrics" in msg and word in msg, msg


@pytest.mark.parametrize("cutoffs", [[5, 5], [10, 5], [0], [11]], ids=["equal", "descending", "zero", "k+1"])
def test_rank_metrics_refuses_bad_cutoffs(cutoffs):
    from lgcn_amd import _ffi

    lib = _ffi.load()
    keep, args = _metric_args(values=cutoffs)
    assert lib.lgcn_rank_metrics(*args) == _ffi.E_ARG
    msg = lib.lgcn_last_error()
    assert b"lgcn_rank_metrics" in msg and b"cutoffs" in msg, msg


def test_rank_metrics_symbol_limits_and_empty_call():
    from lgcn_amd import _ffi, metrics

    lib = _ffi.load()
    assert "lgcn_rank_metrics" in _ffi.EXPORTED and _ffi.ABI_VERSION == 11
    assert metrics.MAX_CUTOFFS == _ffi.METRICS_MAX_CUTOFFS == 8
    keep, args = _metric_args(Q=0)
    assert lib.lgcn_rank_metrics(*args) == 0  # no launch: this machine may have no GPU
    keep, args = _metric_args(values=list(range(1, 9)))  # eight cutoffs are accepted (Q = 0)
    args[3] = 0
    assert lib.lgcn_rank_metrics(*args) == 0


def _counts(hits, dcg, first, n_truth):
    from lgcn_amd.metrics import RankCounts

    return RankCounts(torch.tensor(hits, dtype=torch.int32), torch.tensor(dcg, dtype=torch.float32),
                      torch.tensor(first, dtype=torch.int32), torch.tensor(n_truth, dtype=torch.int32))


def test_summarize_literal_numbers():
    """Ranked [3, 7, 1, 9] against truth {4, 7, 9} at c = 4: hits at ranks 1 and 3."""
    from lgcn_amd.metrics import summarize

    dcg = 1 / math.log2(3) + 1 / math.log2(5)
    idcg = 1 + 1 / math.log2(3) + 1 / 2
    assert dcg == pytest.approx(1.0616064, abs=1e-7) and idcg == pytest.approx(2.1309298, abs=1e-7)
    out = summarize(_counts([[2]], [[dcg]], [1], [3]), [4])
    assert out["users"] == 1
    assert out["recall@4"] == pytest.approx(2 / 3, rel=1e-12)
    assert out["precision@4"] == 0.5
    assert out["hit_rate@4"] == 1.0
    assert out["mrr@4"] == 0.5
    assert out["ndcg@4"] == pytest.approx(0.4981893, abs=1e-7)
    assert out["ndcg@4"] == pytest.approx(float(np.float32(dcg)) / idcg, rel=1e-12)
    assert set(out) == {"users", "recall@4", "precision@4", "hit_rate@4", "ndcg@4", "mrr@4"}


def _random_counts(rng, Q, cs, empty_share):
    """Hand-made counts that a ranking could have produced: hit ranks drawn first, counts from them."""
    k = cs[-1]
    hits, dcg, first, n_truth = [], [], [], []
    for _ in range(Q):
        T = 0 if rng.random() < empty_share else int(rng.integers(1, 2 * k))
        ranks = np.sort(rng.choice(k, rng.integers(0, min(T, k) + 1), replace=False)) if T else np.zeros(0, np.int64)
        hits.append([int((ranks < c).sum()) for c in cs])
        dcg.append([float((1 / np.log2(ranks[ranks < c] + 2.0)).sum()) for c in cs])
        first.append(int(ranks[0]) if ranks.size else -1)
        n_truth.append(T)
    return _counts(hits, dcg, first, n_truth)


@pytest.mark.parametrize("cs", [(1,), (5, 10, 20), (1, 2, 3, 5, 8, 13, 21, 34)])
def test_summarize_matches_float64_numpy(cs):
    from lgcn_amd.metrics import summarize

    counts = _random_counts(np.random.default_rng(len(cs)), 300, cs, empty_share=0.2)
    assert 0 < int((counts.n_truth == 0).sum()) < 300
    got = summarize(counts, cs)
    want = summarize64(*[t.numpy() for t in counts], cs)
    assert got["users"] == want["users"] == int((counts.n_truth > 0).sum())  # empty truth rows are left out
    assert set(got) == set(want)
    for key, w in want.items():
        assert got[key] == pytest.approx(w, rel=1e-12), key
    # cutoffs in any order, repeated: the sorted distinct ones
    assert summarize(counts, list(cs[::-1]) + [cs[0]]) == got


def test_summarize_leaves_out_empty_truth_rows():
    from lgcn_amd.metrics import summarize

    # the second query has no truth: whatever its counts say, it is not averaged
    out = summarize(_counts([[1], [0]], [[1.0], [0.0]], [0, -1], [1, 0]), [3])
    assert out == {"users": 1, "recall@3": 1.0, "precision@3": 1 / 3, "hit_rate@3": 1.0, "ndcg@3": 1.0, "mrr@3": 1.0}
    # a first hit at or past the cutoff does not count for mrr at that cutoff
    out = summarize(_counts([[0, 1]], [[0.0, 0.5]], [2], [1]), [2, 3])
    assert out["mrr@2"] == 0.0 and out["mrr@3"] == pytest.approx(1 / 3, rel=1e-12)
    assert out["hit_rate@2"] == 0.0 and out["hit_rate@3"] == 1.0


@pytest.mark.parametrize("Q", [0, 3])
def test_summarize_without_truth_is_nan(Q):
    from lgcn_amd.metrics import summarize

    out = summarize(_counts(np.zeros((Q, 2), np.int32), np.zeros((Q, 2), np.float32), [-1] * Q, [0] * Q), [5, 10])
    assert out.pop("users") == 0
    assert len(out) == 10 and all(math.isnan(v) for v in out.values())


def test_summarize_refuses_mismatched_cutoffs():
    from lgcn_amd.metrics import summarize

    with pytest.raises(ValueError):
        summarize(_counts([[1, 1]], [[1.0, 1.0]], [0], [1]), [5])
    with pytest.raises(ValueError, match="first"):  # first / n_truth must have one entry per query
        summarize(_counts([[1], [0]], [[1.0], [0.0]], [0], [1, 1]), [5])
    with pytest.raises(ValueError, match="n_truth"):
        summarize(_counts([[1], [0]], [[1.0], [0.0]], [0, -1], [1]), [5])


def test_rank_metrics_refuses_bad_cutoffs_and_cpu_tensors():
    from lgcn_amd import _ffi
    from lgcn_amd.metrics import evaluate_ranking, rank_metrics

    ranked = torch.zeros((2, 10), dtype=torch.int32)
    truth = (torch.zeros(3, dtype=torch.int64), torch.zeros(0, dtype=torch.int32))
    for ks in ([], [0], [11], [-3, 5], range(1, 10)):  # none, below 1, above k, nine of them
        with pytest.raises(ValueError):
            rank_metrics(ranked, truth, ks)
    with pytest.raises(ValueError):
        rank_metrics(ranked, truth, [5], rows=[0])  # one row id for two queries
    with pytest.raises(ValueError):
        rank_metrics(ranked, truth, [5], rows=torch.zeros((3, 2), dtype=torch.int64)[:, 0])  # strided, three ids
    with pytest.raises(TypeError):
        rank_metrics(ranked, (truth[0].to(torch.int32), truth[1]), [5])
    with pytest.raises(_ffi.LgcnError, match="ROCm device"):  # no CPU fallback
        rank_metrics(ranked, truth, [5])
    with pytest.raises(_ffi.LgcnError, match="ROCm device"):
        evaluate_ranking(torch.randn(2, 8), torch.randn(10, 8), truth, ks=(5,))
