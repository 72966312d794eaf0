"""The device negative sampler without a GPU: the host checker's own rules (r-th unseen item against
brute force, the hash's uniformity), the argument refusals of lgcn_amd.negatives before the library
is loaded, the ABI bookkeeping, and that nothing changes while no sampler is installed."""
import numpy as np
import pytest
import torch

import negatives_checker as NC


def test_rth_unseen_matches_enumeration():
    rng = np.random.default_rng(0)
    cases = [(np.zeros(0, np.int32), 7), (np.arange(9, dtype=np.int32), 9)]  # the empty row, the full row
    for _ in range(200):
        I = int(rng.integers(1, 60))
        c = int(rng.integers(0, I + 1))
        cases.append((np.sort(rng.choice(I, c, replace=False)).astype(np.int32), I))
    for row, I in cases:
        want = NC.unseen_brute(row, I)
        assert len(want) == I - len(row)
        assert [NC.rth_unseen(row, r) for r in range(len(want))] == want, (row, I)


def test_candidates_are_unseen_and_fall_back_when_nothing_is():
    ptr = np.array([0, 0, 5, 9], np.int64)
    idx = np.array([0, 1, 2, 3, 4, 0, 1, 3, 4], np.int32)  # user 0: none, user 1: all of 5, user 2: all but 2
    users = np.array([0, 1, 2, 7, -1] * 40, np.int64)
    cand, all_seen = NC.candidates(users, ptr, idx, 5, seed=3, step=2, n=4)
    assert all_seen == 40
    assert (cand >= 0).all() and (cand < 5).all()
    assert (cand[users == 2] == 2).all()  # the one unseen item, always
    assert len(np.unique(cand[users == 0])) == 5 and len(np.unique(cand[users == 1])) == 5
    # a sub-range drawn with first = b0 is the slice of the whole
    part, _ = NC.candidates(users[50:90], ptr, idx, 5, seed=3, step=2, n=4, first=50)
    assert np.array_equal(part, cand[50:90])


def _chi2(draws, bins):
    count = np.bincount(draws, minlength=bins).astype(np.float64)
    e = len(draws) / bins
    return float(((count - e) ** 2 / e).sum())


@pytest.mark.parametrize("vary", ["b", "j", "step"])
def test_draw_is_uniform(vary):
    """200,000 draws over 50 bins, varied over one counter: chi^2 < 100 at 49 degrees of freedom
    (the 99.99 % point is 91)."""
    N, bins = 200_000, 50
    if vary == "b":
        draws = [NC.umul64hi(NC.draw_hash(11, 5, b, 0), bins) for b in range(N)]
    elif vary == "j":
        draws = [NC.umul64hi(NC.draw_hash(11, 5, 123, j), bins) for j in range(N)]
    else:
        draws = [NC.umul64hi(NC.draw_hash(11, s, 123, 0), bins) for s in range(N)]
    chi2 = _chi2(np.asarray(draws), bins)
    print(f"chi2 over {vary}: {chi2:.1f}")
    assert chi2 < 100


def test_pick_hardest_tie_and_nan_rule():
    s = np.array([[0.1, 0.5, 0.5, np.nan], [np.nan, np.nan, np.nan, np.nan], [np.nan, -0.9, np.nan, -0.9],
                  [-0.0, 0.0, -1.0, np.nan]])
    assert NC.pick_hardest(s).tolist() == [1, 0, 1, 0]
    assert NC.top_gap(s).tolist()[:2] == [0.4, np.inf]


def _no_load(monkeypatch):
    from lgcn_amd import _ffi

    def no_load(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(_ffi, "load", no_load)


def test_argument_refusals_come_before_the_library(monkeypatch):
    from lgcn_amd import _ffi
    from lgcn_amd.negatives import MAX_CANDIDATES, MAX_D, NegativeSampler, sample_negatives

    _no_load(monkeypatch)
    users = torch.tensor([0, 1, 2], dtype=torch.int64)
    ptr, idx = torch.tensor([0, 2, 2, 3], dtype=torch.int64), torch.tensor([1, 4, 0], dtype=torch.int32)
    seen = (ptr, idx)
    uw, iw = torch.randn(3, 8), torch.randn(6, 8)
    kw = dict(seed=1, step=0)
    with pytest.raises(TypeError, match="^negatives: users must be a 1-D int64"):
        sample_negatives(users.to(torch.int32), seen, 6, **kw)
    with pytest.raises(TypeError, match="^negatives: users must be a 1-D int64"):
        sample_negatives(users.view(3, 1), seen, 6, **kw)
    with pytest.raises(ValueError, match="^negatives: num_items=0"):
        sample_negatives(users, seen, 0, **kw)
    for n in (0, MAX_CANDIDATES + 1):
        with pytest.raises(ValueError, match=f"^negatives: candidates={n}"):
            sample_negatives(users, seen, 6, candidates=n, tables=(uw, iw), **kw)
    with pytest.raises(ValueError, match="^negatives: first=-1"):
        sample_negatives(users, seen, 6, first=-1, **kw)
    with pytest.raises(TypeError, match=r"^negatives: seen needs ptr int64 \[R \+ 1\] and idx int32"):
        sample_negatives(users, (ptr, idx.to(torch.int64)), 6, **kw)
    with pytest.raises(ValueError, match=r"^negatives: seen is \(ptr, idx\) or"):
        sample_negatives(users, (ptr,), 6, **kw)
    with pytest.raises(ValueError, match=r"^negatives: seen is \(ptr, idx\): row u"):
        sample_negatives(users, (ptr, idx, [0, 1, 2]), 6, **kw)
    with pytest.raises(ValueError, match="^negatives: tables are needed exactly when candidates > 1"):
        sample_negatives(users, seen, 6, candidates=4, **kw)
    with pytest.raises(ValueError, match="^negatives: tables are needed exactly when candidates > 1"):
        sample_negatives(users, seen, 6, candidates=1, tables=(uw, iw), **kw)
    with pytest.raises(ValueError, match="^negatives: tables is "):
        sample_negatives(users, seen, 6, candidates=2, tables=(uw,), **kw)
    with pytest.raises(TypeError, match="^negatives: the item table must be a 2-D float32"):
        sample_negatives(users, seen, 6, candidates=2, tables=(uw, iw.double()), **kw)
    with pytest.raises(ValueError, match="^negatives: table widths differ"):
        sample_negatives(users, seen, 6, candidates=2, tables=(uw, torch.randn(6, 12)), **kw)
    for d in (6, MAX_D + 4):
        with pytest.raises(ValueError, match=f"^negatives: rows of {d} columns"):
            sample_negatives(users, seen, 6, candidates=2, tables=(torch.randn(3, d), torch.randn(6, d)), **kw)
    with pytest.raises(ValueError, match="^negatives: the item table has 5 rows for 6 items"):
        sample_negatives(users, seen, 6, candidates=2, tables=(uw, iw[:5]), **kw)
    with pytest.raises(TypeError, match="^negatives: out must be a contiguous int64 tensor of 3"):
        sample_negatives(users, seen, 6, out=torch.zeros(4, dtype=torch.int64), **kw)
    with pytest.raises(TypeError, match="^negatives: stats must be a contiguous int64 tensor of 2"):
        sample_negatives(users, seen, 6, stats=torch.zeros(2, dtype=torch.int32), **kw)
    # well-formed arguments on the host: no CPU fallback, and still nothing loaded
    with pytest.raises(_ffi.LgcnError, match="ROCm device"):
        sample_negatives(users, seen, 6, **kw)
    ei = torch.tensor([[0, 1], [3, 4]])
    with pytest.raises(ValueError, match="^negatives: candidates=33"):
        NegativeSampler(ei, 3, 6, candidates=33, tables=(uw, iw))
    with pytest.raises(ValueError, match="^negatives: tables or a model are needed exactly when"):
        NegativeSampler(ei, 3, 6, candidates=4)
    with pytest.raises(ValueError, match="^negatives: pass tables or model, not both"):
        NegativeSampler(ei, 3, 6, candidates=4, tables=(uw, iw), model=object())
    with pytest.raises(_ffi.LgcnError, match="ROCm device"):
        NegativeSampler(ei, 3, 6)


def test_entry_point_is_declared_and_checks_its_arguments():
    import ctypes
    import re

    from conftest import ROOT
    from lgcn_amd import _ffi

    assert "lgcn_sample_negatives" in _ffi.EXPORTED and "lgcn_negatives.hip" in _ffi.SOURCES and _ffi.ABI_VERSION == 11
    text = (ROOT / "include" / "lgcn.h").read_text()
    assert int(re.search(r"#define LGCN_NEGATIVES_MAX_N (\d+)", text).group(1)) == _ffi.NEGATIVES_MAX_N == 32
    assert int(re.search(r"#define LGCN_NEGATIVES_MAX_D (\d+)", text).group(1)) == _ffi.NEGATIVES_MAX_D == 512
    lib = _ffi.load()
    buf = (ctypes.c_int64 * 8)()
    p = ctypes.addressof(buf)
    f = (ctypes.c_float * 64)()
    t = (ctypes.addressof(f) + 15) // 16 * 16

    def call(users=p, B=0, first=0, sp=None, si=None, R=0, I=5, n=1, uw=None, ldu=0, U=0, iw=None, ldi=0, d=0, out=p,
             stats=p):
        return lib.lgcn_sample_negatives(users, B, first, sp, si, R, I, 1, 0, n, uw, ldu, U, iw, ldi, d, out, None,
                                         stats, None)

    assert call() == 0  # B == 0: no launch, no device needed
    for bad, word in ((dict(B=-1), b"B=-1"), (dict(first=-2), b"first=-2"), (dict(I=0), b"I=0"), (dict(I=1 << 31), b"I="),
                      (dict(n=0), b"n=0"), (dict(users=None), b"users is null"), (dict(out=None), b"out is null"),
                      (dict(stats=None), b"stats is null"), (dict(sp=p), b"seen_ptr and seen_idx"),
                      (dict(R=-1), b"seen_rows=-1"), (dict(n=2), b"user_rows is null"),
                      (dict(n=2, uw=t), b"item_rows is null"), (dict(n=2, uw=t, iw=t, d=6, ldu=8, ldi=8), b"d=6"),
                      (dict(n=2, uw=t, iw=t, d=8, ldu=4, ldi=8), b"ldu=4"),
                      (dict(n=2, uw=t, iw=t, d=8, ldu=8, ldi=10), b"ldi=10"),
                      (dict(n=2, uw=t, iw=t + 4, d=8, ldu=8, ldi=8), b"not 16-byte aligned"),
                      (dict(n=2, uw=t, iw=t, d=8, ldu=8, ldi=8, U=-1), b"U=-1")):
        assert call(**bad) == _ffi.E_ARG, bad
        msg = lib.lgcn_last_error()
        assert b"lgcn_sample_negatives" in msg and word in msg, (bad, msg)
    for bad, word in ((dict(n=33), b"LGCN_NEGATIVES_MAX_N"),
                      (dict(n=2, uw=t, iw=t, d=516, ldu=516, ldi=516), b"LGCN_NEGATIVES_MAX_D")):
        assert call(**bad) == _ffi.E_UNSUPPORTED, bad
        assert word in lib.lgcn_last_error()


def test_default_draw_is_untouched_without_a_sampler():
    """No sampler installed: get_triplets_indices draws torch.randint(0, I, (B,)) from the global
    generator, the same values and the same generator state afterwards."""
    from utils import helpers

    assert helpers.negative_sampler() is None
    U, I = 6, 9
    ei = torch.tensor([[0, 1, 5, 6, 9, 2], [7, 8, 14, 0, 3, 6]])
    torch.manual_seed(123)
    want = torch.randint(0, I, (4,))
    state = torch.get_rng_state()
    torch.manual_seed(123)
    users, pos, neg = helpers.get_triplets_indices(ei, U, I, "cpu")
    assert users.tolist() == [0, 1, 5, 2] and pos.tolist() == [1, 2, 8, 0]
    assert torch.equal(neg, want) and torch.equal(torch.get_rng_state(), state)


def test_set_negative_sampler_installs_and_restores():
    from utils import helpers

    U, I = 6, 9
    ei = torch.tensor([[0, 1, 5, 6, 9, 2], [7, 8, 14, 0, 3, 6]])
    seen = []

    def sampler(users, pos):
        seen.append((users.tolist(), pos.tolist()))
        return torch.full_like(pos, 4)

    try:
        helpers.set_negative_sampler(sampler)
        assert helpers.negative_sampler() is sampler
        torch.manual_seed(5)
        state = torch.get_rng_state()
        neg = helpers.get_triplets_indices(ei, U, I, "cpu")[2]
        assert neg.tolist() == [4, 4, 4, 4] and seen == [([0, 1, 5, 2], [1, 2, 8, 0])]
        assert torch.equal(torch.get_rng_state(), state)  # the installed sampler draws, not torch.randint
        with pytest.raises(TypeError, match="set_negative_sampler"):
            helpers.set_negative_sampler(3)
        assert helpers.negative_sampler() is sampler
    finally:
        helpers.set_negative_sampler(None)
    assert helpers.negative_sampler() is None
    torch.manual_seed(123)
    want = torch.randint(0, I, (4,))
    torch.manual_seed(123)
    assert torch.equal(helpers.get_triplets_indices(ei, U, I, "cpu")[2], want)
    assert helpers.sample_negative is helpers.REFERENCE_SAMPLE_NEGATIVE


def test_harness_sampler_dispatch():
    """harness._Sampler.draw_triplets: the installed sampler's draw_triplets (on the sampler's own
    counter), a plain callable's result copied, else the default draw_into."""
    from lgcn_amd.harness import _Sampler
    from utils import helpers

    s = _Sampler(9, "cpu")
    users, pos = torch.tensor([0, 1, 2]), torch.tensor([3, 4, 5])
    out = torch.empty(3, dtype=torch.int64)
    torch.manual_seed(9)
    want = torch.randint(0, 9, (3,))
    torch.manual_seed(9)
    s.draw_triplets(out, users, pos, 0)
    assert torch.equal(out, want)

    class Fake:
        calls = []

        def draw_triplets(self, out, users, pos, step=None):
            self.calls.append(step)
            out.fill_(7)

        def __call__(self, users, pos):
            raise AssertionError("the in-place draw is preferred")

    try:
        fake = Fake()
        helpers.set_negative_sampler(fake)
        s.draw_triplets(out, users, pos, 5)
        assert out.tolist() == [7, 7, 7] and fake.calls == [None]
        helpers.set_negative_sampler(lambda u, p: u + p)
        s.draw_triplets(out, users, pos, 6)
        assert out.tolist() == [3, 5, 7]
    finally:
        helpers.set_negative_sampler(None)
