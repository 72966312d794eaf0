"""Calibrated re-ranking without a GPU: lgcn_attr_profile and lgcn_rerank_calibrated check their
arguments before any HIP call, lgcn_amd.recommend refuses bad arguments before loading anything and
CPU tensors after, miscalibration is plain torch (checked against numpy), the float64 rule of
calibrate_checker.py agrees with a direct restatement in Python floats, and nothing existing changed
its signature."""
import ctypes
import inspect
import math
import re

import numpy as np
import pytest
import torch

from calibrate_checker import calibrate64, check_lists, ckl64, profile64
from conftest import ROOT


def _no_load(monkeypatch):
    from lgcn_amd import _ffi

    def no_load(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(_ffi, "load", no_load)


def _calib_args(**over):
    """A well-formed lgcn_rerank_calibrated argument list over a host buffer (never launched: every
    call below fails validation first, or has Q = 0), with some arguments replaced."""
    buf = (ctypes.c_char * 256)()
    p = ctypes.addressof(buf)
    a = dict(pool_idx=p, pool_score=p, ld=100, N=100, Q=4, attr=p, M=1000, target=p, k=10, lam=0.5, alpha=0.01,
             out_idx=p, out_score=p, out_kl=p, out_n=p, stream=None)
    a.update(over)
    return buf, list(a.values())


@pytest.mark.parametrize("over,word", [
    (dict(pool_idx=None), b"pool_idx"),
    (dict(pool_score=None), b"pool_score"),
    (dict(attr=None), b"attr"),
    (dict(target=None), b"target"),
    (dict(out_idx=None), b"out_idx"),
    (dict(out_score=None), b"out_score"),
    (dict(out_kl=None), b"out_kl"),
    (dict(out_n=None), b"out_n"),
    (dict(k=0), b"k=0"),
    (dict(k=101), b"k=101"),
    (dict(ld=99), b"ld=99"),
    (dict(Q=-1), b"Q=-1"),
    (dict(M=-1), b"M=-1"),
    (dict(lam=-0.125), b"lambda"),
    (dict(lam=1.5), b"lambda"),
    (dict(lam=float("nan")), b"lambda"),
    (dict(alpha=0.0), b"alpha"),
    (dict(alpha=1.0), b"alpha"),
    (dict(alpha=-0.5), b"alpha"),
    (dict(alpha=float("nan")), b"alpha"),
])
def test_rerank_calibrated_refuses_bad_arguments(over, word):
    from lgcn_amd import _ffi

    lib = _ffi.load()
    keep, args = _calib_args(**over)
    assert lib.lgcn_rerank_calibrated(*args) == _ffi.E_ARG
    msg = lib.lgcn_last_error()
    assert b"lgcn_rerank_calibrated" in msg and word in msg, msg


def test_rerank_calibrated_pool_limit_and_no_queries():
    from lgcn_amd import _ffi

    lib = _ffi.load()
    keep, args = _calib_args(N=1025, ld=1025)
    assert lib.lgcn_rerank_calibrated(*args) == _ffi.E_UNSUPPORTED and b"LGCN_CALIB_MAX_POOL" in lib.lgcn_last_error()
    for lam in (0.0, 1.0):  # the limits pass every check; Q = 0 then returns OK without a launch
        keep, args = _calib_args(N=1024, ld=1024, k=1024, Q=0, lam=lam)
        assert lib.lgcn_rerank_calibrated(*args) == 0


def _profile_args(**over):
    buf = (ctypes.c_char * 256)()
    p = ctypes.addressof(buf)
    a = dict(hist_ptr=p, hist_idx=p, hist_w=None, hist_row=None, hist_rows=3, Q=3, attr=p, M=10, out_p=p, out_w=p,
             stream=None)
    a.update(over)
    return buf, list(a.values())


@pytest.mark.parametrize("over,word", [
    (dict(hist_ptr=None), b"hist_ptr"),
    (dict(hist_idx=None), b"hist_idx"),
    (dict(attr=None), b"attr"),
    (dict(out_p=None), b"out_p"),
    (dict(out_w=None), b"out_w"),
    (dict(Q=-1), b"Q=-1"),
    (dict(M=-1), b"M=-1"),
    (dict(hist_rows=-1), b"hist_rows=-1"),
])
def test_attr_profile_refuses_bad_arguments(over, word):
    from lgcn_amd import _ffi

    lib = _ffi.load()
    keep, args = _profile_args(**over)
    assert lib.lgcn_attr_profile(*args) == _ffi.E_ARG
    msg = lib.lgcn_last_error()
    assert b"lgcn_attr_profile" in msg and word in msg, msg
    keep, args = _profile_args(Q=0)
    assert lib.lgcn_attr_profile(*args) == 0


def test_symbols_and_constants_match_the_header():
    from lgcn_amd import _ffi, recommend

    text = (ROOT / "include" / "lgcn.h").read_text()
    assert "lgcn_rerank_calibrated" in _ffi.EXPORTED and "lgcn_attr_profile" in _ffi.EXPORTED
    assert "lgcn_calibrate.hip" in _ffi.SOURCES and _ffi.ABI_VERSION == 11
    define = lambda name: int(re.search(rf"#define {name} (\d+)", text).group(1))
    assert define("LGCN_CALIB_GENRES") == _ffi.CALIB_GENRES == recommend.CALIB_GENRES == 32
    assert define("LGCN_CALIB_MAX_POOL") == _ffi.CALIB_MAX_POOL == recommend.CALIB_MAX_POOL == 1024 == _ffi.RANKED_MAX_K
    assert define("LGCN_PROFILE_LONG") == _ffi.PROFILE_LONG == 512
    assert define("LGCN_PROFILE_CHUNK") == _ffi.PROFILE_CHUNK == 512
    assert define("LGCN_ABI_VERSION") == 11


def _pool(Q=3, N=20, M=50, dtype=torch.int64):
    g = torch.Generator().manual_seed(0)
    idx = torch.stack([torch.randperm(M, generator=g)[:N] for _ in range(Q)]).to(dtype)
    attrs = torch.randint(0, 1 << 18, (M,), generator=g).to(torch.int32)
    target = torch.full((Q, 32), 1 / 32)
    return idx, torch.randn(Q, N, generator=g), attrs, target


def test_python_argument_errors_come_before_the_library(monkeypatch):
    from lgcn_amd import _ffi
    from lgcn_amd.recommend import attr_profile, rerank_calibrated, topk_rows_calibrated

    idx, score, attrs, target = _pool()
    _no_load(monkeypatch)
    for k in (0, 21):
        with pytest.raises(ValueError, match="k="):
            rerank_calibrated(idx, score, attrs, target, k, 0.5)
    for bad in (-0.1, 1.01, float("nan")):
        with pytest.raises(ValueError, match="calibration"):
            rerank_calibrated(idx, score, attrs, target, 5, bad)
    for bad in (0.0, 1.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            rerank_calibrated(idx, score, attrs, target, 5, 0.5, alpha=bad)
    with pytest.raises(ValueError, match=r"\[Q, N\]"):
        rerank_calibrated(idx, score[:, :19], attrs, target, 5, 0.5)
    with pytest.raises(TypeError, match="pool_idx"):
        rerank_calibrated(idx.to(torch.int16), score, attrs, target, 5, 0.5)
    with pytest.raises(TypeError, match="pool_score"):
        rerank_calibrated(idx, score.double(), attrs, target, 5, 0.5)
    with pytest.raises(TypeError, match="attrs"):
        rerank_calibrated(idx, score, attrs.to(torch.int64), target, 5, 0.5)
    with pytest.raises(TypeError, match="target"):
        rerank_calibrated(idx, score, attrs, target.double(), 5, 0.5)
    with pytest.raises(ValueError, match="target"):
        rerank_calibrated(idx, score, attrs, target[:, :18], 5, 0.5)
    with pytest.raises(ValueError, match="CALIB_MAX_POOL"):
        rerank_calibrated(torch.zeros((1, 1025), dtype=torch.int32), torch.zeros((1, 1025)), attrs, target[:1], 5, 0.5)
    # the profile
    ptr, hidx = torch.tensor([0, 2, 3]), torch.tensor([1, 2, 3], dtype=torch.int32)
    with pytest.raises(TypeError, match="ptr int64"):
        attr_profile((ptr.to(torch.int32), hidx), attrs)
    with pytest.raises(TypeError, match="attrs"):
        attr_profile((ptr, hidx), attrs.float())
    with pytest.raises(ValueError, match="weights"):
        attr_profile((ptr, hidx), attrs, weights=torch.ones(2))
    with pytest.raises(TypeError, match="weights"):
        attr_profile((ptr, hidx), attrs, weights=torch.ones(3, dtype=torch.float64))
    with pytest.raises(ValueError, match="rows="):
        attr_profile((ptr, hidx, torch.tensor([0])), attrs, rows=torch.tensor([0]))
    # the pool rules of topk_rows_calibrated
    q, picked, cands = torch.randn(4, 16), torch.arange(4), torch.randn(50, 16)
    hist = (torch.tensor([0, 1, 2, 3, 3]), hidx)
    with pytest.raises(ValueError, match="pool=5 is below k=10"):
        topk_rows_calibrated(q, picked, cands, 10, 0.5, attrs=attrs, history=hist, pool=5)
    with pytest.raises(ValueError, match="candidate count"):
        topk_rows_calibrated(q, picked, cands[:8], 10, 0.5, attrs=attrs[:8], history=hist)
    with pytest.raises(ValueError, match="CALIB_MAX_POOL"):
        topk_rows_calibrated(q, picked, torch.randn(3000, 16), 1025, 0.5, attrs=torch.zeros(3000, dtype=torch.int32),
                             history=hist)
    with pytest.raises(ValueError, match="exactly one of history= and target="):
        topk_rows_calibrated(q, picked, cands, 10, 0.5, attrs=attrs)
    with pytest.raises(ValueError, match="exactly one of history= and target="):
        topk_rows_calibrated(q, picked, cands, 10, 0.5, attrs=attrs, history=hist, target=torch.zeros(4, 32))
    with pytest.raises(ValueError, match="needs attrs"):
        topk_rows_calibrated(q, picked, cands, 10, 0.5, history=hist)
    with pytest.raises(ValueError, match="attrs has 49 entries"):
        topk_rows_calibrated(q, picked, cands, 10, 0.5, attrs=attrs[:49], history=hist)
    with pytest.raises(ValueError, match="calibration"):
        topk_rows_calibrated(q, picked, cands, 10, 2.0, attrs=attrs, history=hist)
    with pytest.raises(ValueError, match="k=0"):
        topk_rows_calibrated(q, picked, cands, 0, 0.5, attrs=attrs, history=hist)
    monkeypatch.undo()
    for dtype in (torch.int64, torch.int32):  # well-formed, but on the CPU: no fallback
        with pytest.raises(_ffi.LgcnError, match="ROCm device"):
            rerank_calibrated(idx.to(dtype), score, attrs, target, 5, 0.5)
    with pytest.raises(_ffi.LgcnError, match="ROCm device"):
        attr_profile((ptr, hidx), attrs)
    with pytest.raises(_ffi.LgcnError, match="ROCm device"):
        topk_rows_calibrated(q, picked, cands, 10, 0.5, attrs=attrs, history=hist)


def test_harness_refusals_come_before_the_library(monkeypatch):
    from lgcn_amd import metrics
    from utils import recommend as R

    _no_load(monkeypatch)
    emb = torch.randn(4, 8)
    truth = (torch.tensor([0, 1, 2, 3, 4]), torch.tensor([0, 1, 2, 3], dtype=torch.int32))
    attrs = torch.ones(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="calibration and diversity"):
        metrics.evaluate_ranking(emb, emb, truth, calibration=0.5, diversity=0.5, attrs=attrs, seen=truth)
    with pytest.raises(ValueError, match="calibration=1.5"):
        metrics.evaluate_ranking(emb, emb, truth, calibration=1.5, attrs=attrs, seen=truth)
    with pytest.raises(ValueError, match="needs history= or seen="):
        metrics.evaluate_ranking(emb, emb, truth, calibration=0.5, attrs=attrs)
    with pytest.raises(ValueError, match="needs attrs"):
        metrics.evaluate_ranking(emb, emb, truth, calibration=0.5, seen=truth)
    with pytest.raises(ValueError, match="needs calibration"):
        metrics.evaluate_ranking(emb, emb, truth, history=truth)
    with pytest.raises(ValueError, match="pool is the re-rank's pool"):
        metrics.evaluate_ranking(emb, emb, truth, pool=10)
    for who in ("recommend_for_users", "recommend_for_histories"):
        with pytest.raises(ValueError, match=f"^{who}: diversity and calibration are two re-ranks; one per call$"):
            R._check_options(who, 0.5, None, None, 0.5)
        with pytest.raises(ValueError, match="calibration=-1.0"):
            R._check_options(who, None, None, None, -1.0)
        assert R._check_options(who, None, 32, 2, 0.5) == 2  # pool serves the calibrated re-rank too


def test_calibration_none_leaves_the_signatures_as_they_are():
    """The new keywords are appended with None defaults; every parameter that was there keeps its place
    and default."""
    from lgcn_amd import metrics
    from utils import ranking_eval
    from utils import recommend as R

    def params(f):
        return [(n, p.default) for n, p in inspect.signature(f).parameters.items()]

    E = inspect.Parameter.empty
    users = params(R.recommend_for_users)
    assert users[:13] == [("model", E), ("user_ids", E), ("data_handler", E), ("k", 10), ("exclude_seen", True),
                          ("train_edge_index", None), ("diversity", None), ("pool", None), ("explain", None),
                          ("genres", None), ("genres_all", None), ("without_genres", None), ("among", None)]
    assert users[13:] == [("calibration", None)]
    hist = params(R.recommend_for_histories)
    assert [n for n, _ in hist[:15]] == ["model", "histories", "data_handler", "k", "exclude_history", "train_edge_index",
                                        "embeddings", "weights", "diversity", "pool", "explain", "genres", "genres_all",
                                        "without_genres", "among"]
    assert hist[15:] == [("calibration", None)]
    ev = params(metrics.evaluate_ranking)
    assert ev[:8] == [("user_emb", E), ("item_emb", E), ("truth", E), ("ks", (20,)), ("seen", None), ("users", None),
                      ("diversity", None), ("pool", None)]
    assert ev[8:] == [("calibration", None), ("attrs", None), ("history", None), ("topk_kw", E)]
    re_ = params(ranking_eval.evaluate_ranking)
    assert re_[:8] == [("model", E), ("train_edge_index", E), ("heldout_edge_index", E), ("device", E), ("ks", (20,)),
                       ("embeddings", "raw"), ("diversity", None), ("pool", None)]
    assert re_[8:] == [("calibration", None), ("data_handler", None), ("attrs", None)]


def test_miscalibration_matches_numpy():
    from lgcn_amd.recommend import miscalibration

    rng = np.random.default_rng(3)
    kl = rng.random((7, 12)).astype(np.float32)
    n = np.array([12, 0, 1, 5, 12, 11, 3], np.int32)
    ks = (10, 1, 5, 12, 5)
    got = miscalibration(torch.from_numpy(kl), torch.from_numpy(n), ks)
    assert got.dtype == torch.float64 and got.shape == (7, 4)
    want = ckl64(kl, n, ks)
    np.testing.assert_array_equal(got.numpy(), want)
    assert np.isnan(want[1]).all() and want[2, 3] == np.float64(kl[2, 0]) and want[3, 0] == np.float64(kl[3, 0])
    for bad in ((), (0,), (13,)):
        with pytest.raises(ValueError, match="cutoffs"):
            miscalibration(torch.from_numpy(kl), torch.from_numpy(n), bad)
    with pytest.raises(ValueError, match=r"\[Q, k\]"):
        miscalibration(torch.from_numpy(kl), torch.from_numpy(n[:3]), (1,))


def _brute_profile(idx, weights, attr):
    p, W = [0.0] * 32, 0.0
    for e, i in enumerate(idx):
        w = 1.0 if weights is None else float(np.float32(weights[e]))
        if not (0 <= i < len(attr)) or int(attr[i]) & 0xFFFFFFFF == 0 or not w > 0:
            continue
        word = int(attr[i]) & 0xFFFFFFFF
        pc = bin(word).count("1")
        for g in range(32):
            if word >> g & 1:
                p[g] += w / pc
        W += w
    return ([x / W for x in p] if W > 0 else p), W


def _brute_kl(p, picks, attr, alpha):
    mass, m = [0.0] * 32, 0
    for i in picks:
        word = int(attr[i]) & 0xFFFFFFFF
        if word:
            m += 1
            pc = bin(word).count("1")
            for g in range(32):
                if word >> g & 1:
                    mass[g] += 1.0 / pc
    kl = 0.0
    for g in range(32):
        if p[g] > 0:
            qt = (1 - alpha) * mass[g] / max(1, m) + alpha * p[g]
            kl += p[g] * math.log(p[g] / qt)
    return kl


def _brute_rerank(pidx, pscore, attr, p, k, lam, alpha):
    lam, alpha = float(np.float32(lam)), float(np.float32(alpha))
    picks, left = [], [c for c, i in enumerate(pidx) if 0 <= i < len(attr)]
    out = []
    while left and len(out) < k:
        best, bv, bkl = None, None, None
        for c in left:
            kl = _brute_kl(p, picks + [pidx[c]], attr, alpha)
            v = (1 - lam) * float(pscore[c]) - lam * kl
            if math.isnan(v):
                v = -math.inf
            if best is None or v > bv:
                best, bv, bkl = c, v, kl
        left.remove(best)
        picks.append(pidx[best])
        out.append((int(pidx[best]), float(pscore[best]), bkl))
    return out


def test_checker_agrees_with_a_direct_restatement():
    rng = np.random.default_rng(11)
    for case in range(12):
        M, N = 40, 12
        attr = rng.integers(0, 1 << 6, M).astype(np.uint32)
        attr[rng.random(M) < 0.15] = 0
        if case == 0:
            attr[5] = 0xFFFFFFFF  # every genre at once, bit 31 included
        hist = rng.integers(-2, M + 2, 9)
        weights = None if case % 2 else rng.choice([1.0, 2.5, 0.0, -1.0, np.nan], 9).astype(np.float32)
        p64, W = profile64(hist, weights, attr)
        bp, bW = _brute_profile(hist.tolist(), weights, attr)
        np.testing.assert_allclose(p64, bp, rtol=1e-14, atol=0)
        assert W == pytest.approx(bW, rel=1e-14) and (W == 0 or abs(p64.sum() - 1) < 1e-12)
        p = p64.astype(np.float32)
        pidx = rng.permutation(M)[:N].astype(np.int64)
        pidx[rng.integers(0, N)] = -1
        pidx[rng.integers(0, N)] = M
        pscore = np.sort(rng.standard_normal(N).astype(np.float32))[::-1].copy()
        if case == 3:
            pscore[2] = np.nan
        k, lam = [1, 5, N][case % 3], [0.0, 0.3, 0.7, 1.0][case % 4]
        idx, score, kl, n = calibrate64(pidx, pscore, attr, p, k, lam, 0.01)
        want = _brute_rerank(pidx.tolist(), pscore, attr, p.astype(np.float64).tolist(), k, lam, 0.01)
        assert n == len(want) == min(k, N - 2)
        assert idx[:n].tolist() == [w[0] for w in want]
        np.testing.assert_array_equal(score[:n].view(np.uint32), np.array([w[1] for w in want], np.float32).view(np.uint32))
        np.testing.assert_allclose(kl[:n], [w[2] for w in want], rtol=1e-12, atol=1e-14)
        assert (idx[n:] == -1).all() and np.isneginf(score[n:]).all() and (kl[n:] == 0).all()
        # the rule's own output passes its checker, and the stated consequences hold
        dec, steps, worst = check_lists(pidx[None], pscore[None], attr, p[None], k, lam, 0.01, idx[None], score[None],
                                        kl.astype(np.float32)[None], np.array([n]))
        assert steps == n and worst["kl"] <= 1.0 and worst["value"] <= 4.0
        if lam == 0.0 and case != 3:
            assert idx[:n].tolist() == [i for i in pidx.tolist() if 0 <= i < M][:n]
        short = calibrate64(pidx, pscore, attr, p, 1, lam, 0.01)
        assert short[0][0] == idx[0] and short[2][0] == kl[0]
        none = calibrate64(pidx, pscore, attr, np.zeros(32, np.float32), k, lam, 0.01)
        if case != 3:
            assert none[0][:n].tolist() == [i for i in pidx.tolist() if 0 <= i < M][:n] and (none[2] == 0).all()


def test_checker_refuses_a_wrong_list():
    rng = np.random.default_rng(5)
    M, N, k = 30, 10, 4
    attr = (1 << rng.integers(0, 4, M)).astype(np.uint32)
    p = np.zeros(32, np.float32)
    p[:4] = [0.7, 0.1, 0.1, 0.1]
    pidx = rng.permutation(M)[:N].astype(np.int64)
    pscore = np.linspace(1.0, 0.9, N).astype(np.float32)
    idx, score, kl, n = calibrate64(pidx, pscore, attr, p, k, 0.7, 0.01)
    args = (pidx[None], pscore[None], attr, p[None], k, 0.7, 0.01)
    check_lists(*args, idx[None], score[None], kl.astype(np.float32)[None], np.array([n]))
    assert idx.tolist() != pidx[:k].tolist()  # the re-rank did something, so the pool prefix is a wrong answer
    with pytest.raises(AssertionError):
        check_lists(*args, pidx[None, :k], pscore[None, :k], kl.astype(np.float32)[None], np.array([n]))
    with pytest.raises(AssertionError):
        check_lists(*args, idx[None], score[None], (kl * (1 + 1e-4)).astype(np.float32)[None], np.array([n]))
    with pytest.raises(AssertionError):
        check_lists(*args, idx[None], score[None], kl.astype(np.float32)[None], np.array([n - 1]))
