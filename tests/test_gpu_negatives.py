"""The device negative sampler on the GPU (lgcn_sample_negatives in csrc/lgcn_negatives.hip,
lgcn_amd.negatives) against the host checker of negatives_checker.py.

The integer part — which items the candidates are — is specified to the bit and compared exactly.
The hardest-of-n pick compares f32 cosines, so it is held to the project's per-row bar: the pick's
float64 cosine within 1e-5 of the float64 best of its own n candidates, with at most 0.1 % of the
picks differing from the float64 argmax at all (so the tolerance cannot hide a wrong argmax), and
exactly wherever the best score is clear of the others.

Shapes: batches below, at and above one workgroup (256 triplets at n = 1, 16 at n > 1) and one wave;
n at one batch of candidates (2, 8) and two (32); rows of one lane (d = 4), a few lanes (16, 20),
one pass (64) and several (128, 256, 512), d = 20 leaving lanes idle in a pass."""
import functools

import numpy as np
import pytest
import torch

import negatives_checker as NC

pytestmark = pytest.mark.gpu

U1, I1 = 37, 53


def _csr(rows):
    ptr = np.cumsum([0] + [len(x) for x in rows]).astype(np.int64)
    return ptr, np.concatenate(list(rows) + [np.zeros(0, np.int64)]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _seen_small():
    """U1 users over I1 items: user 0 has seen nothing, user 1 everything, user 2 all but item 17."""
    rng = np.random.default_rng(1)
    rows = [np.zeros(0, np.int64), np.arange(I1), np.delete(np.arange(I1), 17)]
    for _ in range(3, U1):
        rows.append(np.sort(rng.choice(I1, int(rng.integers(0, 41)), replace=False)))
    return _csr(rows)


def _users_small(B, seed=2):
    rng = np.random.default_rng(seed)
    users = rng.integers(0, U1, B).astype(np.int64)
    special = np.array([0, 1, 2, -1, U1 + 5], np.int64)
    users[:min(B, 5)] = special[:min(B, 5)]
    return users


def _dev(gpu, *arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in arrays]


def _in_row(ptr, idx, users, items):
    """bool [B]: items[b] is in users[b]'s row."""
    return np.array([int(i) in set(NC.user_row(ptr, idx, int(u)).tolist()) for u, i in zip(users, items)], bool)


@pytest.mark.parametrize("B", [0, 1, 3, 1000, 4097])
def test_uniform_draw_is_the_checkers_exactly(gpu, B):
    from lgcn_amd.negatives import sample_negatives

    ptr, idx = _seen_small()
    users = _users_small(B)
    tptr, tidx, tusers = _dev(gpu, ptr, idx, users)
    stats = torch.zeros(2, dtype=torch.int64, device=gpu)
    out, score = sample_negatives(tusers, (tptr, tidx), I1, seed=77, step=3, stats=stats, return_score=True)
    want, all_seen = NC.candidates(users, ptr, idx, I1, 77, 3, 1)
    out = out.cpu().numpy()
    assert out.dtype == np.int64 and out.shape == (B,)
    assert np.array_equal(out, want[:, 0])
    assert stats.tolist() == [all_seen, 0] and all_seen == int((users == 1).sum())
    assert (score.cpu().numpy() == 0).all()
    assert not _in_row(ptr, idx, users, out)[users != 1].any()
    assert (out[users == 2] == 17).all()  # the one unseen item
    # stats are added to, the draw repeats bit for bit, and out= is written in place
    buf = torch.full((B,), -1, dtype=torch.int64, device=gpu)
    got = sample_negatives(tusers, (tptr, tidx), I1, seed=77, step=3, stats=stats, out=buf)
    assert got is buf and np.array_equal(buf.cpu().numpy(), out)
    assert stats.tolist() == [2 * all_seen, 0]
    # no CSR: nothing is excluded, the draw is umul64hi(h2, I)
    free = sample_negatives(tusers, None, I1, seed=77, step=3).cpu().numpy()
    assert free.tolist() == [NC.umul64hi(NC.draw_hash(77, 3, b, 0), I1) for b in range(B)]


def test_uniform_draw_covers_exactly_the_unseen_items(gpu):
    """One user 20,000 times: every unseen item is drawn, no seen one, about equally often."""
    from lgcn_amd.negatives import sample_negatives

    ptr, idx = _seen_small()
    u = 5
    row = NC.user_row(ptr, idx, u)
    unseen = NC.unseen_brute(row, I1)
    tptr, tidx = _dev(gpu, ptr, idx)
    out = sample_negatives(torch.full((20000,), u, dtype=torch.int64, device=gpu), (tptr, tidx), I1, seed=1, step=0)
    count = np.bincount(out.cpu().numpy(), minlength=I1)
    assert sorted(np.flatnonzero(count).tolist()) == unseen
    e = 20000 / len(unseen)
    chi2 = float(((count[unseen] - e) ** 2 / e).sum())
    print(f"chi2 {chi2:.1f} at {len(unseen) - 1} degrees of freedom")
    # chi^2 has mean df and deviation sqrt(2 df): 2 df + 40 is over 5 deviations out for df <= 52
    assert chi2 < 2 * len(unseen) + 40


@pytest.mark.parametrize("n", [1, 4])
def test_draw_does_not_depend_on_the_launch(gpu, n):
    """Sub-ranges drawn with first = b0 are slices of the whole draw; a repeat is bitwise the same;
    another seed or step draws something else."""
    from lgcn_amd.negatives import sample_negatives

    ptr, idx = _seen_small()
    B = 1000
    users = _users_small(B, seed=8)
    users[users >= U1] = 3
    users[users < 0] = 4
    tptr, tidx, tusers = _dev(gpu, ptr, idx, users)
    g = torch.Generator().manual_seed(3)
    tables = None
    if n > 1:
        tables = (0.1 * torch.randn(U1, 20, generator=g).to(gpu), 0.1 * torch.randn(I1, 20, generator=g).to(gpu))
    kw = dict(candidates=n, tables=tables, return_score=True)
    whole, score = sample_negatives(tusers, (tptr, tidx), I1, seed=9, step=4, **kw)
    for b0, b1 in ((0, 17), (17, 400), (400, 1000)):
        part, ps = sample_negatives(tusers[b0:b1], (tptr, tidx), I1, seed=9, step=4, first=b0, **kw)
        assert torch.equal(part, whole[b0:b1]) and torch.equal(ps, score[b0:b1])
    again, s2 = sample_negatives(tusers, (tptr, tidx), I1, seed=9, step=4, **kw)
    assert torch.equal(again, whole) and torch.equal(s2, score)
    for seed, step in ((10, 4), (9, 5)):
        other = sample_negatives(tusers, (tptr, tidx), I1, seed=seed, step=step, candidates=n, tables=tables)
        assert (other != whole).float().mean().item() > 0.5


# ---- hardest of n ---------------------------------------------------------------------------------
U2, I2, B2 = 64, 500, 2048


@functools.lru_cache(maxsize=None)
def _seen_mid():
    rng = np.random.default_rng(4)
    rows = [np.sort(rng.choice(I2, int(rng.integers(0, 300)), replace=False)) for _ in range(U2)]
    rows[0] = np.zeros(0, np.int64)
    return _csr(rows)


@functools.lru_cache(maxsize=None)
def _users_mid():
    return np.random.default_rng(6).integers(0, U2, B2).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _cand_mid(n):
    ptr, idx = _seen_mid()
    return NC.candidates(_users_mid(), ptr, idx, I2, 21, 6, n)[0]


_PARITY = {}


@pytest.mark.parametrize("d", [4, 16, 20, 64, 128, 256, 512])
@pytest.mark.parametrize("n", [2, 8, 32])
def test_hardest_of_n_matches_float64(gpu, n, d):
    from lgcn_amd.negatives import sample_negatives
    from parity import record_stats

    ptr, idx = _seen_mid()
    users = _users_mid()
    cand = _cand_mid(n)
    g = torch.Generator().manual_seed(100 + d)
    # the rows sit inside wider tensors (ld = d + 8, 16 bytes in): read in place; and contiguous
    wide_u = 0.1 * torch.randn(U2, d + 8, generator=g)
    wide_i = 0.1 * torch.randn(I2, d + 8, generator=g)
    uw, iw = wide_u[:, 4:4 + d], wide_i[:, 4:4 + d]
    scores = NC.cosines(users, cand, uw.numpy(), iw.numpy())
    j64 = NC.pick_hardest(scores)
    want = cand[np.arange(B2), j64]
    tptr, tidx, tusers = _dev(gpu, ptr, idx, users)
    du, di = wide_u.to(gpu)[:, 4:4 + d], wide_i.to(gpu)[:, 4:4 + d]
    assert du.stride(0) == d + 8 and du.data_ptr() % 16 == 0
    stats = torch.zeros(2, dtype=torch.int64, device=gpu)
    out, score = sample_negatives(tusers, (tptr, tidx), I2, seed=21, step=6, candidates=n, tables=(du, di),
                                  return_score=True, stats=stats)
    out2, score2 = sample_negatives(tusers, (tptr, tidx), I2, seed=21, step=6, candidates=n,
                                    tables=(du.contiguous(), di.contiguous()), return_score=True)
    assert torch.equal(out, out2) and torch.equal(score, score2)  # the view changes no bit
    out, score = out.cpu().numpy(), score.cpu().numpy().astype(np.float64)
    assert stats.tolist() == [0, 0]
    hit = cand == out[:, None]
    assert hit.any(axis=1).all(), "a pick that is none of its triplet's candidates"
    picked = scores[np.arange(B2), hit.argmax(axis=1)]  # the same item scores the same at any j
    best = scores[np.arange(B2), j64]
    gap = float((best - picked).max())
    differ = float((out != want).mean())
    score_err = float(np.abs(score - picked).max())
    _PARITY[f"n{n}_d{d}"] = {"worst_gap": gap, "differing_share": differ, "score_err": score_err}
    record_stats("negatives", _PARITY)
    print(f"n={n} d={d}: worst gap {gap:.3g}, differing share {differ:.3g}, score error {score_err:.3g}")
    assert gap <= 1e-5
    assert differ <= 1e-3
    assert score_err <= 1e-5
    clear = NC.top_gap(scores) > 1e-5  # a best score clear of the rest is picked exactly
    assert np.array_equal(out[clear], want[clear])
    assert not _in_row(ptr, idx, users, out).any()


def test_tie_and_nan_rule(gpu):
    from lgcn_amd.negatives import sample_negatives

    U, I, B, n, d = 20, 40, 512, 8, 16
    rng = np.random.default_rng(12)
    ptr, idx = _csr([np.sort(rng.choice(I, int(rng.integers(0, 12)), replace=False)) for _ in range(U)])
    users = rng.integers(0, U, B).astype(np.int64)
    users[::7] = 3        # user 3's row is zero below
    users[5::31] = U + 2  # outside the user table (and the CSR)
    users[6::31] = -1
    cand, _ = NC.candidates(users, ptr, idx, I, 5, 1, n)
    tptr, tidx, tusers = _dev(gpu, ptr, idx, users)
    uw = (0.1 * rng.standard_normal((U, d))).astype(np.float32)
    uw[3] = 0
    outside = (users < 0) | (users >= U)
    zero_user = users == 3

    def run(iw):
        stats = torch.zeros(2, dtype=torch.int64, device=gpu)
        out, score = sample_negatives(tusers, (tptr, tidx), I, seed=5, step=1, candidates=n,
                                      tables=_dev(gpu, uw, iw), return_score=True, stats=stats)
        assert stats.tolist() == [0, int(outside.sum())]
        return out.cpu().numpy(), score.cpu().numpy()

    # identical item rows: every score of a triplet is the same, the lowest j wins
    out, score = run(np.tile((0.1 * rng.standard_normal(d)).astype(np.float32), (I, 1)))
    assert np.array_equal(out, cand[:, 0])
    assert np.isnan(score[outside | zero_user]).all() and not np.isnan(score[~(outside | zero_user)]).any()
    # zero and NaN item rows rank last: never picked unless all n are such, then candidate 0
    iw = (0.1 * rng.standard_normal((I, d))).astype(np.float32)
    bad = np.zeros(I, bool)
    bad[rng.choice(I, 30, replace=False)] = True
    kinds = np.flatnonzero(bad)
    iw[kinds[::2]] = 0
    iw[kinds[1::2], 3] = np.nan
    out, score = run(iw)
    all_bad = bad[cand].all(axis=1)
    normal = ~(outside | zero_user)
    assert all_bad[normal].any() and (~all_bad[normal]).any()
    assert not bad[out[normal & ~all_bad]].any()
    assert np.array_equal(out[all_bad], cand[all_bad, 0])
    assert np.array_equal(out[outside | zero_user], cand[outside | zero_user, 0])
    want, stats, _, scores, _ = NC.hardest(users, ptr, idx, I, 5, 1, n, uw, iw)
    assert stats == [0, int(outside.sum())]
    clear = NC.top_gap(scores) > 1e-5
    assert np.array_equal(out[clear], want[clear])
    ok = normal & ~all_bad
    picked = scores[np.arange(B), (cand == out[:, None]).argmax(axis=1)]
    assert np.abs(score[ok] - picked[ok]).max() <= 1e-5 and np.isnan(score[~ok]).all()


# ---- through the training step and the harness -----------------------------------------------------
class _Batch:
    def __init__(self, ei):
        self.edge_index = ei

    def to(self, device):
        return _Batch(self.edge_index.to(device))


@functools.lru_cache(maxsize=None)
def _planted():
    from lgcn_amd import synth

    g, _ = synth.planted_bipartite(40, 30, 3, degree=5, seed=2)
    return g.num_users, g.num_items, g.edge_index


@pytest.mark.parametrize("graphs", [False, True])
@pytest.mark.parametrize("n", [1, 4])
def test_fused_step_trains_on_the_samplers_negatives(gpu, n, graphs):
    """Three steps of FusedTrainStep(lazy=True) with a NegativeSampler, bitwise a twin stepped
    through the plain neg_sampler hook with the negatives the checker computes from the tables as
    they are in memory at each draw."""
    from lgcn_amd.negatives import NegativeSampler
    from lgcn_amd.optim import RowLazyAdam
    from lgcn_amd.train_step import FusedTrainStep
    from models.light_gcn import LightGCN

    U, I, ei_np = _planted()
    ei = torch.from_numpy(ei_np).to(gpu)
    users = ei_np[0][ei_np[0] < U]
    sptr, sidx = [t.cpu().numpy() for t in NegativeSampler(ei, U, I).seen]
    assert np.array_equal(sptr[1:] - sptr[:-1], [len(set(ei_np[1][ei_np[0] == u].tolist())) for u in range(U)])
    batch = _Batch(ei)
    seed = 5

    def run(make):
        torch.manual_seed(0)
        m = LightGCN(U, I, num_layers=2, dim_h=16).to(gpu)
        opt = RowLazyAdam(m.user_embedding.weight.data, m.item_embedding.weight.data, lr=1e-2, max_grad_norm=1.0)
        step = FusedTrainStep(m, opt, graphs=graphs, lazy=True, neg_sampler=make(m))
        losses, negs = [], []
        for _ in range(3):
            losses.append(step.step(batch).item())
            negs.append(step.state(ei).neg.cpu().numpy().copy())
        step.sync()
        return losses, m.user_embedding.weight.detach().clone(), m.item_embedding.weight.detach().clone(), negs

    samplers = []

    def device_sampler(m):
        samplers.append(NegativeSampler(ei, U, I, candidates=n, seed=seed, model=m if n > 1 else None))
        return samplers[-1]

    def checker_hook(m):
        k = [0]

        def hook(pos):
            if n == 1:
                out = NC.candidates(users, sptr, sidx, I, seed, k[0], 1)[0][:, 0]
            else:
                out, _, _, scores, _ = NC.hardest(users, sptr, sidx, I, seed, k[0], n,
                                                  m.user_embedding.weight.detach().cpu().numpy(),
                                                  m.item_embedding.weight.detach().cpu().numpy())
                assert NC.top_gap(scores).min() > 1e-6, "the planted data leaves a pick to rounding"
            k[0] += 1
            return torch.from_numpy(out).to(pos.device)

        return hook

    got = run(device_sampler)
    ref = run(checker_hook)
    assert samplers[0].calls == 3 and samplers[0].stats() == {"all_seen": 0, "bad_users": 0}
    for a, b in zip(got[3], ref[3]):
        assert np.array_equal(a, b)
        assert not _in_row(sptr, sidx, users, a).any()
    assert got[0] == ref[0]
    assert torch.equal(got[1], ref[1]) and torch.equal(got[2], ref[2])


def test_harness_trains_through_an_installed_sampler(gpu, tune):
    """helpers.set_negative_sampler + the unchanged train(): the fused path, one draw per step; with
    the sampler removed the default draws and today's loss are back, bit for bit."""
    from lgcn_amd.negatives import NegativeSampler
    from models.light_gcn import LightGCN
    from utils import helpers
    from utils import train_test as TT

    tune(harness_fused=True)
    U, I, ei_np = _planted()
    ei = torch.from_numpy(ei_np).to(gpu)
    src, dst = ei_np
    low = np.where(src < U, src, dst) < 20  # the edges of users 0..19, both directions, and the rest
    loader = [_Batch(torch.from_numpy(np.ascontiguousarray(ei_np[:, sel])).to(gpu)) for sel in (low, ~low)]

    def run(make):
        torch.manual_seed(0)
        model = LightGCN(U, I, num_layers=2, dim_h=16).to(gpu)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        sampler = make(model) if make else None
        helpers.set_negative_sampler(sampler)
        try:
            torch.manual_seed(41)
            losses = []
            for _ in range(2):
                losses.append(TT.train(model, opt, loader, gpu))
                assert TT.LAST_TRAIN_PATH == "fused", TT.LAST_TRAIN_PATH
        finally:
            helpers.set_negative_sampler(None)
        return losses, sampler

    base, _ = run(None)
    hard, sampler = run(lambda m: NegativeSampler(ei, U, I, candidates=4, model=m))
    assert sampler.calls == 2 * len(loader)
    assert sampler.stats() == {"all_seen": 0, "bad_users": 0}
    assert all(np.isfinite(x) for x in hard) and hard != base
    assert helpers.negative_sampler() is None
    again, _ = run(None)
    assert again == base
