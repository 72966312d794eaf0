"""oracle/adam_ref.py, the float64 contract of the clip-norm and Adam kernels, checked on the CPU:
against torch.optim.Adam + clip_grad_norm_ in float64, and the conditioning of the bars
tests/test_gpu_optim_kernels.py holds the kernels to (tests/adam_checker.py)."""
import numpy as np
import pytest

import adam_checker as AC
from oracle import adam_ref


def test_trajectory_ref_equals_torch_float64():
    """adam_trajectory_ref == clip_grad_norm_(1) + torch.optim.Adam, both in float64, on 3 tensors
    for 20 steps (clip active and inactive), to 1e-12 relative; the norms too."""
    import torch

    rng = np.random.default_rng(0)
    shapes = [(13, 8), (5, 3), (7,)]
    w0 = [rng.standard_normal(s) * 0.1 for s in shapes]
    grads = [[rng.standard_normal(s) * (3.0 if t % 2 else 0.02) for s in shapes] for t in range(20)]
    for max_norm in (1.0, None):
        w, m, v, norms = adam_ref.adam_trajectory_ref(w0, grads, 1e-3, (0.9, 0.999), 1e-8, max_norm)
        ps = [torch.nn.Parameter(torch.tensor(x, dtype=torch.float64)) for x in w0]
        opt = torch.optim.Adam(ps, lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
        for t, gs in enumerate(grads):
            for p, g in zip(ps, gs):
                p.grad = torch.tensor(g, dtype=torch.float64)
            if max_norm is not None:
                n = torch.nn.utils.clip_grad_norm_(ps, max_norm=max_norm).item()
                assert abs(norms[t] - n) <= 1e-12 * n
            opt.step()
        assert max_norm is None or (min(norms) < 1.0 < max(norms))
        for k, p in enumerate(ps):
            st = opt.state[p]
            for got, want, what in ((w[k], p, "p"), (m[k], st["exp_avg"], "exp_avg"), (v[k], st["exp_avg_sq"], "exp_avg_sq")):
                want = want.detach().numpy()
                assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (max_norm, k, what)


def test_step_ref_is_one_trajectory_step():
    """adam_step_ref with the double constants of step t == the trajectory's step t."""
    rng = np.random.default_rng(1)
    w0 = [rng.standard_normal((6, 4))]
    grads = [[rng.standard_normal((6, 4))] for _ in range(3)]
    w2, m2, v2, _ = adam_ref.adam_trajectory_ref(w0, grads[:2])
    w3, m3, v3, _ = adam_ref.adam_trajectory_ref(w0, grads)
    one = adam_ref.adam_step_ref(w2[0], grads[2][0], m2[0], v2[0], 1.0, -(1e-3 / (1 - 0.9 ** 3)),
                                 np.sqrt(1 - 0.999 ** 3), 1 - 0.9, 0.999, 1 - 0.999, 1e-8)
    for got, want in ((one.p, w3[0]), (one.m, m3[0]), (one.v, v3[0])):
        assert np.abs(got - want).max() <= 1e-14 * np.abs(want).max()
    norm, coef = adam_ref.clip_ref([np.array([3.0, 4.0]), None, np.zeros(0)], 1.0)
    assert norm == 5.0 and coef == 1.0 / (5.0 + 1e-6)
    assert adam_ref.clip_ref([np.zeros(4)], 1.0) == (0.0, 1.0)


@pytest.mark.parametrize("family", AC.FAMILIES)
def test_bars_are_attainable_in_float32(family):
    """adam_elem's operations in numpy float32, each correctly rounded, stay inside the one-step
    bars on every family, step and clip coefficient the GPU test uses: a correct float32 kernel
    passes them. (They are tight: p' alone spends up to its own half ulp, EPS |p'|, of its bar.)"""
    hyp = AC.hyper()
    worst = {}
    for t in AC.STEPS:
        ss, bc2 = AC.host_consts(t)
        for coef in (1.0, AC.CLIP_COEF):
            p, g, m, v = AC.make_family(family, 20000, coef, seed=t)
            got = AC.emulate_adam_elem(p, g, m, v, coef, ss, bc2, *hyp)
            ref = adam_ref.adam_step_ref(p, g, m, v, np.float32(coef), ss, bc2, *hyp)
            assert all(np.isfinite(a).all() for a in got)
            # every intermediate a normal float32 (the families' promise)
            tiny = np.finfo(np.float32).tiny
            for x in (ref.g * ref.g * float(hyp[2]), ref.v, np.abs(ref.m), np.abs(ref.upd)):
                assert ((x == 0) | (x >= tiny)).all() and (x < 1e38).all()
            r = AC.step_ratios(got, ref, m, ss)
            AC.assert_bars(r, f"{family} t={t} coef={coef}")
            for k, x in r.items():
                worst[k] = max(worst.get(k, 0.0), x)
    print(family, worst)
    assert worst["p"] > 0.05, "the p' bar is far from what float32 does: not the bar the issue states?"


def test_bars_catch_a_wrong_step():
    """The bars can fail: one element of m', v' or p' off by 1e-6 relative, a step taken with the
    neighbouring step's constants, or a clip coefficient that was not applied is over them."""
    hyp = AC.hyper()
    t = 10
    ss, bc2 = AC.host_consts(t)
    p, g, m, v = AC.make_family("normal", 4096, AC.CLIP_COEF)
    ref = adam_ref.adam_step_ref(p, g, m, v, np.float32(AC.CLIP_COEF), ss, bc2, *hyp)
    good = AC.emulate_adam_elem(p, g, m, v, AC.CLIP_COEF, ss, bc2, *hyp)
    AC.assert_bars(AC.step_ratios(good, ref, m, ss), "good")
    for k in range(4):
        bad = [a.copy() for a in good]
        bad[k][17] *= np.float32(1 + 1e-6)
        with pytest.raises(AssertionError):
            AC.assert_bars(AC.step_ratios(bad, ref, m, ss), "perturbed")
    for wrong in (AC.emulate_adam_elem(p, g, m, v, AC.CLIP_COEF, *AC.host_consts(t + 1), *hyp),
                  AC.emulate_adam_elem(p, g, m, v, 1.0, ss, bc2, *hyp)):
        with pytest.raises(AssertionError):
            AC.assert_bars(AC.step_ratios(wrong, ref, m, ss), "wrong")


def test_norm_chain_lengths():
    """The chain lengths the norm bar is built from, on cases small enough to count by hand."""
    # one block of 256 threads: 1 float4 iteration (4) + 6 shuffles + 4 waves; finish 1 + 6 + 4
    assert AC.norm_chain_dense([4]) == 4 + 10 + 11
    assert AC.norm_chain_dense([5]) == 4 + 1 + 10 + 11                      # + the scalar tail
    assert AC.norm_chain_dense([5], [False]) == 1 + 10 + 11                 # scalar path
    assert AC.dense_norm_blocks([1023, 1025, 7, 0]) == 9
    # past 1024 blocks * 256 threads * 4: a second float4 iteration for some threads, and a tail
    assert AC.norm_chain_dense([1048576 + 4099]) == 8 + 1 + 10 + (4 + 10)
    assert AC.norm_chain_dense([1048576 + 4099], [False]) == 5 + 10 + (4 + 10)
    assert AC.lanes(8) == (2, 1) and AC.lanes(256) == (64, 1) and AC.lanes(512) == (64, 2)
    # d = 512: 4 rows per block, 8192 rows per sweep, two float4 per lane
    assert AC.norm_chain_rows(8192 + 37, 512) == 2 * 8 + 10 + (8 + 10)
    assert AC.norm_chain_rows(262144 + 5, 8) == 2 * 4 + 10 + (8 + 10)
    assert AC.norm_chain_rows(66, 64, ranks=3) == 4 + 10 + (24 + 10)


def test_trajectory_bar_on_the_cpu():
    """The trajectory bar is attainable and can fail: adam_elem's float32 emulation, stepped with
    host constants, stays within it of the float64 trajectory (clip on and off), and the same
    emulation with every step's constants taken one step late misses it."""
    T, d = 12, 8
    w0, grads = AC.trajectory_case(T, d)
    hyp = AC.hyper()
    for clip in (None, 1.0):
        ref, yard, _ = AC.trajectory_refs(T, d, clip)
        for shift in (0, 1):
            st = [[w.copy(), np.zeros_like(w), np.zeros_like(w)] for w in w0]
            for t, gs in enumerate(grads, 1):
                coef = 1.0
                if clip is not None:
                    norm = np.sqrt(np.float32(sum(float((g.astype(np.float32) ** 2).sum(dtype=np.float32)) for g in gs)))
                    coef = AC.coef_f32(norm, clip)
                for s, g in zip(st, gs):
                    s[0], _, s[1], s[2] = AC.emulate_adam_elem(s[0], g, s[1], s[2], coef, *AC.host_consts(t + shift), *hyp)
            ratio = AC.trajectory_ratios([s[0] for s in st], yard, ref)
            assert (ratio <= 1.0) == (shift == 0), (clip, shift, ratio)
