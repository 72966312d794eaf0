"""MMR re-ranking without a GPU: lgcn_rerank_mmr checks its arguments before any HIP call,
lgcn_amd.recommend refuses bad arguments before loading anything and CPU tensors after,
intra_list_diversity is plain torch (checked on CPU tensors against the float64 numpy restatement),
and the float64 rule itself has the properties the GPU tests rely on."""
import ctypes
import math
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from rerank_checker import check_lists, ild64, mmr64, unit_rows64


def _mmr_args(**over):
    """A well-formed lgcn_rerank_mmr argument list over a host buffer (never launched: every call
    below fails validation first, or has Q = 0), with some arguments replaced."""
    buf = (ctypes.c_char * 256)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16  # Cn must be 16-byte aligned
    a = dict(pool_idx=p, pool_score=p, ld=100, N=100, Q=4, Cn=p, M=1000, D=64, k=10, diversity=0.5, out_idx=p,
             out_score=p, out_pair=p, out_n=p, stream=None)
    a.update(over)
    return buf, list(a.values())


@pytest.mark.parametrize("over,word", [
    (dict(pool_idx=None), b"pool_idx"),
    (dict(pool_score=None), b"pool_score"),
    (dict(Cn=None), b"Cn"),
    (dict(out_idx=None), b"out_idx"),
    (dict(out_score=None), b"out_score"),
    (dict(out_pair=None), b"out_pair"),
    (dict(out_n=None), b"out_n"),
    (dict(k=0), b"k=0"),
    (dict(k=101), b"k=101"),
    (dict(ld=99), b"ld=99"),
    (dict(Q=-1), b"Q=-1"),
    (dict(M=-1), b"M=-1"),
    (dict(D=0), b"D=0"),
    (dict(D=6), b"D=6"),
    (dict(diversity=-0.125), b"diversity"),
    (dict(diversity=1.5), b"diversity"),
    (dict(diversity=float("nan")), b"diversity"),
])
def test_rerank_mmr_refuses_bad_arguments(over, word):
    from lgcn_amd import _ffi

    lib = _ffi.load()
    keep, args = _mmr_args(**over)
    assert lib.lgcn_rerank_mmr(*args) == _ffi.E_ARG
    msg = lib.lgcn_last_error()
    assert b"lgcn_rerank_mmr" in msg and word in msg, msg


def test_rerank_mmr_refuses_a_misaligned_table():
    from lgcn_amd import _ffi

    lib = _ffi.load()
    keep, args = _mmr_args()
    args[5] += 4
    assert lib.lgcn_rerank_mmr(*args) == _ffi.E_ARG and b"aligned" in lib.lgcn_last_error()


@pytest.mark.parametrize("N,D,word", [
    (513, 8, b"LGCN_MMR_MAX_POOL"),
    (129, 256, b"LGCN_MMR_MAX_LDS_BYTES"),   # one row past 128 * 256 * 4 == 131072
    (512, 128, b"LGCN_MMR_MAX_LDS_BYTES"),
    (257, 128, b"LGCN_MMR_MAX_LDS_BYTES"),
])
def test_rerank_mmr_pool_limits(N, D, word):
    from lgcn_amd import _ffi

    lib = _ffi.load()
    keep, args = _mmr_args(N=N, ld=N, D=D)
    assert lib.lgcn_rerank_mmr(*args) == _ffi.E_UNSUPPORTED
    msg = lib.lgcn_last_error()
    assert b"lgcn_rerank_mmr" in msg and word in msg, msg


@pytest.mark.parametrize("N,D", [(128, 256), (256, 128), (512, 64), (512, 8)])
def test_rerank_mmr_accepts_the_limit_exactly(N, D):
    """N * D * 4 == 131072 (and N == 512) pass every check; with Q = 0 the call then returns OK
    without a launch, so this runs on a machine without a GPU."""
    from lgcn_amd import _ffi

    lib = _ffi.load()
    keep, args = _mmr_args(N=N, ld=N, D=D, k=N, Q=0)
    assert N * D * 4 <= 131072 and lib.lgcn_rerank_mmr(*args) == 0


def test_symbol_and_limits_match_the_header():
    from lgcn_amd import _ffi, recommend

    text = (ROOT / "include" / "lgcn.h").read_text()
    assert "lgcn_rerank_mmr" in _ffi.EXPORTED and "lgcn_rerank.hip" in _ffi.SOURCES and _ffi.ABI_VERSION == 11
    assert int(re.search(r"#define LGCN_MMR_MAX_POOL (\d+)", text).group(1)) == _ffi.MMR_MAX_POOL == 512
    assert int(re.search(r"#define LGCN_MMR_MAX_LDS_BYTES (\d+)", text).group(1)) == _ffi.MMR_MAX_LDS_BYTES == 131072
    assert (recommend.MMR_MAX_POOL, recommend.MMR_MAX_LDS_BYTES) == (512, 131072)


def _pool(Q=3, N=20, M=50, d=16, dtype=torch.int64):
    g = torch.Generator().manual_seed(0)
    idx = torch.stack([torch.randperm(M, generator=g)[:N] for _ in range(Q)]).to(dtype)
    return idx, torch.randn(Q, N, generator=g), torch.randn(M, d, generator=g)


def test_rerank_mmr_python_argument_errors():
    from lgcn_amd import _ffi
    from lgcn_amd.recommend import rerank_mmr

    idx, score, cands = _pool()
    for k in (0, 21):
        with pytest.raises(ValueError, match="k="):
            rerank_mmr(idx, score, cands, k, 0.5)
    for bad in (-0.1, 1.01, float("nan")):
        with pytest.raises(ValueError, match="diversity"):
            rerank_mmr(idx, score, cands, 5, bad)
    with pytest.raises(ValueError, match=r"\[Q, N\]"):
        rerank_mmr(idx, score[:, :19], cands, 5, 0.5)
    with pytest.raises(ValueError, match=r"\[Q, N\]"):
        rerank_mmr(idx[0], score[0], cands, 5, 0.5)
    with pytest.raises(TypeError, match="pool_idx"):
        rerank_mmr(idx.to(torch.int16), score, cands, 5, 0.5)
    with pytest.raises(TypeError, match="pool_score"):
        rerank_mmr(idx, score.double(), cands, 5, 0.5)
    with pytest.raises(TypeError, match="candidates"):
        rerank_mmr(idx, score, cands.double(), 5, 0.5)
    with pytest.raises(ValueError, match="MMR_MAX_POOL"):
        rerank_mmr(torch.zeros((1, 513), dtype=torch.int32), torch.zeros((1, 513)), cands, 5, 0.5)
    with pytest.raises(ValueError, match="MMR_MAX_LDS_BYTES"):  # 129 rows at the padded width 256
        rerank_mmr(torch.zeros((1, 129), dtype=torch.int32), torch.zeros((1, 129)), torch.randn(300, 200), 5, 0.5)
    with pytest.raises(ValueError, match="columns"):
        rerank_mmr(idx, score, torch.randn(50, 257), 5, 0.5)
    for dtype in (torch.int64, torch.int32):  # well-formed, but on the CPU: no fallback
        with pytest.raises(_ffi.LgcnError, match="ROCm device"):
            rerank_mmr(idx.to(dtype), score, cands, 5, 0.5)
        with pytest.raises(_ffi.LgcnError, match="ROCm device"):
            rerank_mmr(idx.to(dtype), score, cands, 5, 0.0, normalized=True)


def test_topk_rows_diverse_pool_rules():
    from lgcn_amd import _ffi
    from lgcn_amd.recommend import topk_rows_diverse

    q, picked = torch.randn(4, 16), torch.arange(4)
    with pytest.raises(ValueError, match="pool=5 is below k=10"):
        topk_rows_diverse(q, picked, torch.randn(100, 16), 10, 0.5, pool=5)
    with pytest.raises(ValueError, match="candidate count"):  # 8 candidates cannot fill k = 10
        topk_rows_diverse(q, picked, torch.randn(8, 16), 10, 0.5)
    with pytest.raises(ValueError, match="MMR_MAX_POOL"):
        topk_rows_diverse(q, picked, torch.randn(2000, 16), 600, 0.5)
    with pytest.raises(ValueError, match=r"MMR_MAX_LDS_BYTES // \(4 \* D\) at D=256"):  # 128 rows at most
        topk_rows_diverse(torch.randn(4, 200), picked, torch.randn(2000, 200), 129, 0.5)
    with pytest.raises(ValueError, match="diversity"):
        topk_rows_diverse(q, picked, torch.randn(100, 16), 10, 2.0)
    with pytest.raises(ValueError, match="k=0"):
        topk_rows_diverse(q, picked, torch.randn(100, 16), 0, 0.5)
    with pytest.raises(_ffi.LgcnError, match="ROCm device"):
        topk_rows_diverse(q, picked, torch.randn(100, 16), 10, 0.5)


def test_intra_list_diversity_matches_numpy():
    from lgcn_amd.recommend import intra_list_diversity

    rng = np.random.default_rng(3)
    pair = rng.standard_normal((50, 12)).astype(np.float32)
    n = rng.integers(0, 13, 50).astype(np.int32)
    n[:4] = [0, 1, 2, 12]
    for q in range(50):
        pair[q, n[q]:] = 0  # the kernel's tails
    cs = [1, 2, 5, 12]
    got = intra_list_diversity(torch.from_numpy(pair), torch.from_numpy(n), cs + [5])
    assert got.dtype == torch.float64 and got.shape == (50, 4)
    want = ild64(pair, n, cs)
    np.testing.assert_allclose(got.numpy(), want, rtol=1e-12, atol=1e-12, equal_nan=True)
    assert torch.isnan(got[:, 0]).all()               # one item has no pair
    assert torch.isnan(got[:2]).all()                 # lists of 0 and 1 items: c' < 2 at every cutoff
    assert not torch.isnan(got[2, 1:]).any()          # a list of two items counts from c = 2 on
    assert got[2, 1] == got[2, 3]                     # and c' = min(c, n) stays 2
    # literal: three items with cosines 0.5, 0.25, 0.75 between them -> mean 0.5 -> ILD 0.5
    lit = intra_list_diversity(torch.tensor([[0.0, 0.5, 1.0]]), torch.tensor([3]), [2, 3])
    assert lit.tolist() == [[0.5, 0.5]]
    for ks in ([], [0], [13]):
        with pytest.raises(ValueError):
            intra_list_diversity(torch.from_numpy(pair), torch.from_numpy(n), ks)
    with pytest.raises(ValueError):
        intra_list_diversity(torch.from_numpy(pair), torch.from_numpy(n[:49]), [5])


def test_harness_entry_points_refuse_cpu_tensors_when_diversity_is_set():
    import pandas as pd

    from lgcn_amd import _ffi
    from lgcn_amd.metrics import evaluate_ranking
    from models.light_gcn import LightGCN
    from utils import ranking_eval
    from utils import recommend as R

    truth = (torch.tensor([0, 1, 2], dtype=torch.int64), torch.tensor([3, 4], dtype=torch.int32))
    with pytest.raises(_ffi.LgcnError, match="ROCm device"):
        evaluate_ranking(torch.randn(2, 8), torch.randn(100, 8), truth, ks=(5,), diversity=0.5)
    with pytest.raises(ValueError, match="diversity"):
        evaluate_ranking(torch.randn(2, 8), torch.randn(100, 8), truth, ks=(5,), diversity=1.5)
    with pytest.raises(ValueError, match="needs diversity"):
        evaluate_ranking(torch.randn(2, 8), torch.randn(100, 8), truth, ks=(5,), pool=50)
    U, I = 4, 80
    model = LightGCN(U, I, num_layers=1, dim_h=8)

    class H:
        user_id_map = {10 + u: u for u in range(U)}
        movie_id_map = {100 + i: U + i for i in range(I)}
        movies = pd.DataFrame({"movieId": [100 + i for i in range(I)], "title": [f"m{i}" for i in range(I)]})
        edge_index = torch.tensor([[0, 1], [U + 2, U + 3]])

    with pytest.raises(_ffi.LgcnError, match="ROCm device"):
        R.recommend_for_users(model, [10, 11], H, k=5, diversity=0.5)
    with pytest.raises(ValueError, match="needs diversity"):
        R.recommend_for_users(model, [10, 11], H, k=5, pool=50)
    assert R.recommend_for_users(model, [-1], H, k=5, diversity=0.5) == [{"error": "Invalid user ID"}]
    ei = torch.tensor([[0, 1], [U + 2, U + 3]])
    with pytest.raises(_ffi.LgcnError, match="ROCm device"):
        ranking_eval.evaluate_ranking(model, ei, ei, "cpu", ks=(5,), diversity=0.0, pool=20)


def test_float64_rule_properties():
    """What the GPU tests lean on, shown on the rule itself: diversity 0 keeps the pool order and
    skips ineligible entries, a smaller k gives a prefix, a duplicate of the first pick is pushed
    down, and the rule's own lists pass check_lists, which refuses two picks swapped."""
    rng = np.random.default_rng(4)
    cands = rng.standard_normal((60, 8)).astype(np.float32)
    cands[7] = cands[3]  # a duplicate row
    U = unit_rows64(cands)
    pidx = np.array([3, 7, 60, 11, -1, 20, 2**31 - 1, 5, 9, 30])
    r = np.array([0.9, 0.9, 0.95, 0.8, 0.99, 0.7, 0.98, 0.6, 0.5, 0.4], np.float32)
    idx, score, pair, n = mmr64(pidx, r, U, 8, 0.0)
    assert n == 7 and idx.tolist() == [3, 7, 11, 20, 5, 9, 30, -1] and math.isinf(score[7]) and pair[7] == 0
    idx5, score5, pair5, n5 = mmr64(pidx, r, U, 5, 0.5)
    idx8, score8, pair8, n8 = mmr64(pidx, r, U, 8, 0.5)
    assert n5 == 5 and (idx8[:5] == idx5).all() and (pair8[:5] == pair5).all()
    assert idx8[0] == 3 and idx8[1] != 7  # the twin of pick 0 has cosine 1 to it: 0.45 - 0.5 < 0.4 - 0.5 * cos
    assert pair8[0] == 0 and abs(pair8[1] - float(U[idx8[1]] @ U[3])) < 1e-12
    dec, steps = check_lists(pidx[None], r[None], U, 8, 0.5, idx8[None], score8[None], pair8[None], np.array([n8]))
    assert steps == 7 and dec == 6  # step 0 is the exact tie of the twins: not decided, the lower position wins
    bad = idx8.copy()
    bad[[0, 1]] = bad[[1, 0]]
    with pytest.raises(AssertionError):
        check_lists(pidx[None], r[None], U, 8, 0.5, bad[None], score8[None], pair8[None], np.array([n8]))
