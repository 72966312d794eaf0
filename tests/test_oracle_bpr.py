"""oracle/bpr_ref.py, the float64 per-triplet contract of the BPR kernels, checked on the CPU:
against float64 torch autograd through utils.train_test.bpr_loss, against the older float64 loss
restatement, and the conditioning of the bars tests/test_gpu_bpr_kernels.py holds the kernels to."""
import numpy as np
import pytest

import bpr_checker as BC
from oracle import bpr_ref, lgconv_ref


def _small_case(d, B=64, seed=0):
    rng = np.random.default_rng(seed + d)
    U, I = 11, 17
    F = rng.standard_normal((U + I, d)) * 0.1
    W = rng.standard_normal((U + I, d)) * 0.1
    u = rng.integers(0, 5, B)  # 64 triplets over 5 users: every user many times
    p, n = rng.integers(0, I, B), rng.integers(0, I, B)
    n[::7] = p[::7]            # some triplets whose negative is their positive
    return F, W, U, u, p, n


@pytest.mark.parametrize("d", [8, 64])
def test_ref_equals_float64_autograd(d):
    """Loss, du/dp/dn and the reg rows == torch autograd in float64 through the harness's own
    bpr_loss, rtol 1e-12 per row (duplicated users and p == n triplets included; their du is
    exactly zero on both sides)."""
    import torch

    from utils import train_test as TT

    coeff = 5e-3
    F, W, U, u, p, n = _small_case(d)
    ref = bpr_ref.bpr_triplet_ref(F, W, U, u, p, n, coeff)
    rows = [torch.tensor(t[r], dtype=torch.float64, requires_grad=True)
            for t, r in ((F, u), (W, u), (F, U + p), (W, U + p), (F, U + n), (W, U + n))]
    loss = TT.bpr_loss(*rows, bpr_coeff=coeff)
    loss.backward()
    assert abs(ref.loss(coeff) - loss.item()) <= 1e-12 * abs(loss.item())
    for name, got, want in (("du", ref.du, rows[0].grad), ("reg_u", ref.reg_u, rows[1].grad),
                            ("dp", ref.dp, rows[2].grad), ("reg_p", ref.reg_p, rows[3].grad),
                            ("dn", ref.dn, rows[4].grad), ("reg_n", ref.reg_n, rows[5].grad)):
        BC.parity.assert_rows_close(got, want.numpy(), rtol=1e-12, what=name)
    assert (ref.du[::7] == 0).all() and (ref.du[1::7] != 0).any()
    # the uncancelled scales bound the rows they belong to
    for g, S in ((ref.du, ref.S_u), (ref.dp, ref.S_p), (ref.dn, ref.S_n)):
        assert (np.abs(g).max(axis=1) <= S * (1 + 1e-12)).all()


@pytest.mark.parametrize("d", [8, 64])
def test_ref_loss_equals_bpr_loss_np(d):
    coeff = 5e-3
    F, W, U, u, p, n = _small_case(d, seed=3)
    ref = bpr_ref.bpr_triplet_ref(F, W, U, u, p, n, coeff)
    want = lgconv_ref.bpr_loss_np(F[u], W[u], F[U + p], W[U + p], F[U + n], W[U + n], coeff)
    assert abs(ref.loss(coeff) - want) <= 1e-12 * abs(want)
    np.testing.assert_allclose(ref.sums[:, 5], ref.sreg, rtol=0, atol=0)
    assert ref.sums.shape == (64, 6)


def test_softplus_threshold():
    """F.softplus(beta=1, threshold=20): z itself and slope 1 above 20, log1p(exp(z)) up to it."""
    import torch

    z = np.array([-800.0, -20.0, -1e-3, 0.0, 1e-3, 19.999999, 20.0, 20.000001, 35.0])
    sp, sg = bpr_ref.softplus(z)
    t = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.softplus(t)
    y.sum().backward()
    np.testing.assert_allclose(sp, y.detach().numpy(), rtol=1e-14, atol=0)
    np.testing.assert_allclose(sg, t.grad.numpy(), rtol=1e-14, atol=0)


def test_effective_F_is_two_float32_roundings():
    rng = np.random.default_rng(1)
    F = rng.standard_normal((9, 8)).astype(np.float32)
    W = rng.standard_normal((9, 8)).astype(np.float32)
    t = np.array([1, 0, 1, 0, 0, 1, 1, 0, 1], np.uint8)
    F_nan = F.copy()
    F_nan[t == 0] = np.nan
    mul = np.float32(1 / 3)
    got = bpr_ref.effective_F(F_nan, W, t, 3.0, mul)
    assert got.dtype == np.float32 and np.isfinite(got).all()
    assert np.array_equal(got[t == 1], F[t == 1])
    want = np.float32(np.float64(np.float32(np.float64(W[t == 0]) / 3.0)) * np.float64(mul))  # each step rounded once
    assert np.array_equal(got[t == 0], want)
    assert np.array_equal(bpr_ref.effective_F(F, W, None, 3.0, mul), F)


@pytest.mark.parametrize("d", BC.WIDTHS)
@pytest.mark.parametrize("family", BC.FAMILIES)
def test_bars_are_reachable_in_float32(family, d):
    """Conditioning of the GPU bars: the same formula restated in plain float32 numpy stays under
    a QUARTER of every bar of tests/test_gpu_bpr_kernels.py, on every input family and width it
    uses (B = 1001 and B = 1). So float32 alone reaches the bars with room to spare: they cannot
    excuse a wrong kernel, and a correct float32 kernel is not at their mercy."""
    for B in (1001, 1):
        F, W, u, p, n = BC.make_case(family, d, B)
        cf, terms = BC.f32_restatement(F, W, u, p, n)
        BC.assert_bars(BC.bar_ratios(cf, terms, BC.case_ref(family, d, B), family), f"{family} d={d} B={B}", limit=0.25)


def test_bars_catch_a_wrong_row():
    """The bars can fail: one element off by 1e-4 of its row's scale, a NaN row, or one softplus
    term off by 1e-4 relative is over them."""
    family, d, B = "normal", 64, 1001
    F, W, u, p, n = BC.make_case(family, d, B)
    ref = BC.case_ref(family, d, B)
    cf, terms = BC.f32_restatement(F, W, u, p, n)
    bad = cf.copy()
    bad[B + 17, 5] += np.float32(1e-4 * ref.S_p[17])
    with pytest.raises(AssertionError):
        BC.assert_bars(BC.bar_ratios(bad, terms, ref, family), "perturbed")
    bad = cf.copy()
    bad[3] = np.nan
    with pytest.raises(AssertionError):
        BC.assert_bars(BC.bar_ratios(bad, terms, ref, family), "nan")
    t2 = terms.copy()
    t2[40] *= np.float32(1 + 1e-4)
    with pytest.raises(AssertionError):
        BC.assert_bars(BC.bar_ratios(cf, t2, ref, family), "term")
