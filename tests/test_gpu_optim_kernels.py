"""The clip-norm and Adam kernels of csrc/lgcn_optim.hip and csrc/lgcn_rowadam.hip called directly
through the C ABI and held to the float64 contract of oracle/adam_ref.py (bars and chain lengths:
tests/adam_checker.py), plus what must be bitwise: the scalar against the float4 path, host
against device constants, lgcn_adam_prologue against lgcn_adam_consts, the row-lazy replays against
the dense kernel. Every pointer is inside a live allocation and every id in range; the NaN rows are
the ones a kernel must never read.

Worst error / bar measured on an MI355X (parity.stats_dir() / "optim_kernels.json", copied to
profiles/optim_kernels/): see the docstrings of the tests below.
"""
import functools

import numpy as np
import pytest
import torch

import adam_checker as AC
from oracle import adam_ref

pytestmark = pytest.mark.gpu

F32 = np.float32
U, I = 37, 29
N = U + I


def _dev(gpu, a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(gpu)


# ---- (a) lgcn_grad_norm against float64 --------------------------------------------------------

NORM_LISTS = {"n1": (1,), "n3": (3,), "n4_5": (4, 5), "mixed_null": (1023, 1025, 7, 0),
              "eight": (5, 64, 1, 300, 2, 1027, 4, 33)}
NORM_FAMILIES = ("normal", "zero", "1e-15", "1e15", "active", "inactive", "near")


def _norm_grads(numels, family, seed=0):
    rng = np.random.default_rng(AC._seed("norm", numels, family, seed))
    scale = {"zero": 0.0, "1e-15": 1e-15, "1e15": 1e15}.get(family, 1.0)
    return [AC._mag(rng, n, scale).astype(F32) if n else None for n in numels]


def _check_norm(gpu, grads, max_norm, L, key, family, misaligned=()):
    slabs = [None if g is None else AC.Slab(gpu, g, k in misaligned) for k, g in enumerate(grads)]
    out = AC.grad_norm(gpu, slabs, max_norm)
    ratios = AC.norm_ratios(out, grads, F32(max_norm), L)
    print(key, family, "max_norm", max_norm, "out", out, "L", L, ratios)
    AC.record("lgcn_grad_norm", f"{key}/{family}", ratios)
    AC.assert_bars(ratios, f"{key} {family}")
    AC.same_bits(out[1], AC.coef_f32(out[0], max_norm), "coef from the stored norm")
    AC.same_bits(AC.grad_norm(gpu, slabs, max_norm), out, "second call")
    for k, s in enumerate(slabs):
        if s is not None:
            AC.same_bits(s.read(f"grad {k}"), grads[k], "the gradient itself")
    return out


@pytest.mark.parametrize("family", NORM_FAMILIES)
@pytest.mark.parametrize("name", NORM_LISTS)
def test_grad_norm_matches_float64(gpu, name, family):
    """out[0] within (L + 4) 2^-24 of the float64 norm, out[1] bitwise min(max_norm / (out[0] +
    1e-6f), 1) and within the bar of the float64 coefficient, a second call bitwise the first.
    Lists of 1, 2, 4 (one of numel 0 and a null grad) and 8 tensors; all-zero gradients give norm 0
    and coefficient 1 exactly; `near` puts max_norm within two ulp of norm + 1e-6 on either side.

    Worst error / bar on an MI355X over the five lists and seven families: norm 0.021,
    coefficient 0.041 (all-zero: 0 / 0; `near`: 0.012 / 0.029)."""
    numels = NORM_LISTS[name]
    grads = _norm_grads(numels, family)
    norm64, _ = adam_ref.clip_ref(grads, 1.0)
    L = AC.norm_chain_dense(numels)
    if family == "active":
        max_norms = [0.37 * norm64]
    elif family == "inactive":
        max_norms = [3.0 * norm64]
    elif family == "near":
        mid = F32(norm64 + 1e-6)
        max_norms = [mid]
        for _ in range(2):
            max_norms = [np.nextafter(max_norms[0], F32(0)), *max_norms, np.nextafter(max_norms[-1], F32(np.inf))]
    else:
        max_norms = [1.0]
    for mn in max_norms:
        out = _check_norm(gpu, grads, float(mn), L, name, family)
        if family == "zero":
            assert out[0] == 0.0 and out[1] == 1.0
        if family == "active":
            assert out[1] < 0.5
        if family == "inactive":
            assert out[1] == 1.0


def test_grad_norm_grid_wrap_and_scalar_path(gpu):
    """1,048,576 + 4,099 elements: past 1024 blocks x 256 threads x 4, so the float4 loop wraps
    for some threads, and as an interior view one float off alignment, where the scalar loop
    wraps four times. A second list mixes a misaligned tensor with aligned ones. The aligned and
    the misaligned results are within the bar of float64 and of each other.

    Worst error / bar on an MI355X, norm / coefficient: wrap 0.0098 / 0.012 aligned, 0.011 /
    0.013 on the scalar path; second list 0.0033 / 0.010 and 0.0040 / 0.012."""
    for key, numels, mis in (("wrap", (1048576 + 4099,), (0,)), ("offset_view", (1027, 5, 64), (0, 2))):
        grads = _norm_grads(numels, "normal", seed=1)
        al = [k not in mis for k in range(len(numels))]
        La, Lm = AC.norm_chain_dense(numels), AC.norm_chain_dense(numels, al)
        a = _check_norm(gpu, grads, 1.0, La, key, "aligned")
        m = _check_norm(gpu, grads, 1.0, Lm, key, "misaligned", misaligned=mis)
        norm64, _ = adam_ref.clip_ref(grads, 1.0)
        assert abs(float(a[0]) - float(m[0])) <= AC.norm_bar(max(La, Lm)) * norm64


# ---- (b) lgcn_adam_step, one step against float64 ----------------------------------------------

STEP_NUMELS = ((1,), (3,), (4,), (5,), (1023,), (5, 64, 1, 300, 2, 1027, 4, 33))


def _clip_tensor(gpu, coef):
    return None if coef is None else torch.tensor([123.0, coef], dtype=torch.float32, device=gpu)


def _run_step(gpu, arrays, hyp, ss, bc2, *, coef=None, dev=False, write_grad=1, misalign=None):
    """arrays: per tensor (p, g, m, v) float32; -> the same after lgcn_adam_step. dev: the step's
    two constants from a device pair (host arguments 0 and 1); misalign: index into (P, G, M, V)."""
    slabs = [tuple(AC.Slab(gpu, a, misaligned=(j == misalign)) for j, a in enumerate(t)) for t in arrays]
    scal = torch.tensor([float(ss), float(bc2)], dtype=torch.float32, device=gpu) if dev else None
    AC.adam_step(gpu, slabs, hyp, 0.0 if dev else ss, 1.0 if dev else bc2, clip=_clip_tensor(gpu, coef),
                 dev_scalars=scal, write_grad=write_grad)
    return [tuple(s.read(f"tensor {k} {'PGMV'[j]}") for j, s in enumerate(t)) for k, t in enumerate(slabs)]


def _judge_step(got, arrays, coef, hyp, ss, bc2, key, family, what):
    worst = {}
    for (p, g, m, v), out in zip(arrays, got):
        c = F32(1.0 if coef is None else coef)
        ref = adam_ref.adam_step_ref(p, g, m, v, c, ss, bc2, *hyp)
        r = AC.step_ratios(out, ref, m, ss)
        AC.same_bits(out[1], g * c, what + ": the clipped gradient")
        for k, x in r.items():
            worst[k] = x if k not in worst or not x <= worst[k] else worst[k]
    AC.record("lgcn_adam_step", f"{key}/{family}", worst)
    AC.assert_bars(worst, what)
    return worst


@pytest.mark.parametrize("t", AC.STEPS)
@pytest.mark.parametrize("family", AC.FAMILIES)
def test_adam_step_matches_float64(gpu, family, t):
    """p', g', m', v' of one lgcn_adam_step within the one-step bars of tests/adam_checker.py, from
    float32 state and the float32 constants of step t, for numel 1, 3, 4, 5, 1023 and a list of 8
    mixed tensors, with clip = NULL and clip = [x, 0.3712]; g' bitwise fl(g * coef); the floats
    around every tensor untouched.

    Worst error / bar on an MI355X over the steps, sizes and both clips, per family:
      family    g'      m'      v'      p'
      normal    0.981   0.193   0.313   0.971
      tiny      0.996   0.204   0.302   0.998
      huge      0.964   0.191   0.303   0.971
      zero_g    0       0.228   0.164   0.972
      first     0.985   0.042   0.551   0.966
      cancel    0.983   0.134   0.292   0.967
      stale     0.980   0.041   0.592   0.828
    (g' is one correctly rounded product, so it reaches its half ulp; p' spends up to its own.)"""
    hyp = AC.hyper()
    ss, bc2 = AC.host_consts(t)
    for coef in (None, AC.CLIP_COEF):
        for numels in STEP_NUMELS:
            arrays = [AC.make_family(family, n, coef or 1.0, seed=(t, k)) for k, n in enumerate(numels)]
            got = _run_step(gpu, arrays, hyp, ss, bc2, coef=coef)
            w = _judge_step(got, arrays, coef, hyp, ss, bc2, "small", family, f"{family} t={t} coef={coef} {numels}")
            print(family, t, coef, numels, w)


@pytest.mark.parametrize("numels", [(5,), (1023,), STEP_NUMELS[-1]])
def test_adam_step_paths_are_bitwise_one(gpu, numels):
    """The same step taken with write_grad = 0 (gradient bitwise untouched, p / m / v the same),
    with the two constants read from a device pair, and with each of P, G, M, V in turn one float
    off alignment (the scalar loop) is bitwise the aligned float4 step with host constants."""
    hyp = AC.hyper()
    ss, bc2 = AC.host_consts(10)
    for coef in (None, AC.CLIP_COEF):
        arrays = [AC.make_family("normal", n, coef or 1.0, seed=("paths", k)) for k, n in enumerate(numels)]
        want = _run_step(gpu, arrays, hyp, ss, bc2, coef=coef)
        _judge_step(want, arrays, coef, hyp, ss, bc2, "paths", "normal", f"aligned {numels}")
        variants = {"write_grad=0": dict(write_grad=0), "dev_scalars": dict(dev=True)}
        variants.update({f"misaligned {'PGMV'[j]}": dict(misalign=j) for j in range(4)})
        for name, kw in variants.items():
            got = _run_step(gpu, arrays, hyp, ss, bc2, coef=coef, **kw)
            for k, (w, o, a) in enumerate(zip(want, got, arrays)):
                for j in (0, 2, 3):
                    AC.same_bits(o[j], w[j], f"{name}: tensor {k} {'PGMV'[j]}")
                AC.same_bits(o[1], a[1] if name == "write_grad=0" else w[1], f"{name}: tensor {k} grad")


def test_adam_step_grid_wrap(gpu):
    """8,388,608 + 7 elements: past 8192 blocks x 256 threads of float4, so the grid-stride loop
    wraps (and the scalar tail follows it); every element is held to the one-step bars.

    Worst error / bar on an MI355X: g' 0.9994, m' 0.211, v' 0.330, p' 0.990."""
    n = 8388608 + 7
    assert n // 4 > AC.ADAM_MAX_BLOCKS * AC.K_BLOCK
    hyp = AC.hyper()
    ss, bc2 = AC.host_consts(10)
    arrays = [AC.make_family("normal", n, AC.CLIP_COEF, seed="wrap")]
    got = _run_step(gpu, arrays, hyp, ss, bc2, coef=AC.CLIP_COEF)
    print(_judge_step(got, arrays, AC.CLIP_COEF, hyp, ss, bc2, "wrap", "normal", "grid wrap"))


# ---- (c) lgcn_adam_prologue --------------------------------------------------------------------

@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.8, 0.99)])
def test_adam_prologue_is_the_consts_table(gpu, betas):
    """Steps 1..4096, then the device counter set to 19,990 and 20 more: every (step_size,
    bc2_sqrt) pair the prologue writes is bitwise the lgcn_adam_consts row of the same t (what
    "row-lazy == dense, bitwise" rests on) and within one float32 ulp of the host's double
    formula; the counter ends at exactly the number of calls.

    On an MI355X every pair equals the host's (0 ulp), for both betas."""
    from lgcn_amd import _ffi

    lib, s = _ffi.load(), _ffi.stream_of(gpu)
    first, jump, more = 4096, 19990, 20
    ts = np.concatenate([np.arange(1, first + 1), np.arange(jump + 1, jump + more + 1)])
    table = torch.full((len(ts), 2), float("nan"), dtype=torch.float32, device=gpu)
    step = torch.zeros(1, dtype=torch.float64, device=gpu)
    for i in range(len(ts)):  # a fresh slot per call: no sync in the loop
        if i == first:
            assert step.item() == float(first)
            step.fill_(float(jump))
        _ffi.check(lib.lgcn_adam_prologue(step.data_ptr(), AC.LR, betas[0], betas[1], table.data_ptr() + 8 * i, s),
                   "lgcn_adam_prologue")
    assert step.item() == float(jump + more)
    consts = torch.zeros((jump + more + 2, 4), dtype=torch.float32, device=gpu)
    _ffi.check(lib.lgcn_adam_consts(consts.data_ptr(), 1, jump + more + 1, AC.LR, betas[0], betas[1], s),
               "lgcn_adam_consts")
    got, rows = table.cpu().numpy(), consts.cpu().numpy()
    AC.same_bits(got, rows[ts, :2], "prologue pairs against the consts rows")
    AC.same_bits(rows[ts, 2], F32(1.0) / rows[ts, 1], "consts.z = fl(1 / bc2_sqrt)")
    assert rows[0, 0] == (1.0 if betas[1] == 0.999 else 0.0)  # the Markstein flag
    host = np.array([AC.host_consts(int(t), AC.LR, betas) for t in ts], F32)
    ulps = np.abs(got.astype(np.float64) - host.astype(np.float64)) / np.spacing(np.abs(host)).astype(np.float64)
    AC.record("lgcn_adam_prologue", f"betas={betas}", {"ulp_to_host_double": float(ulps.max())})
    assert ulps.max() <= 1.0, (ulps.max(), ts[ulps.max(axis=1).argmax()])


# ---- (d) the row clip norms --------------------------------------------------------------------

def _row_lists(gpu, rng, n_users=U, n_items=I):
    """List a (unique rows, with 0, U - 1, U, N - 1) + list b (item keys with off_b = U, duplicates
    marked by first_b = 0 and overwritten with the exchange's -1 padding, rows of list a marked in
    skip_b). -> (device args, the rows that count)."""
    n = n_users + n_items
    rows_a = np.unique(np.concatenate([[0, n_users - 1, n_users, n - 1], rng.integers(0, n, 9)])).astype(np.int32)
    keys = rng.integers(0, n_items, 24).astype(np.int64)
    keys[:3] = (n_items - 1, keys[3], 0)  # row N - 1 of list a, a duplicate, row U of list a
    first = np.zeros(len(keys), np.uint8)
    first[np.unique(keys, return_index=True)[1]] = 1
    skip = np.zeros(n, np.uint8)
    skip[rows_a] = 1
    listed_b = [int(k) + n_users for k, f in zip(keys, first) if f and not skip[int(k) + n_users]]
    assert listed_b and (first == 0).any() and any(skip[int(k) + n_users] for k in keys[first == 1])
    keys[first == 0] = -1
    live = np.concatenate([rows_a, listed_b]).astype(np.int64)
    assert len(np.unique(live)) == len(live)
    return dict(rows_a=_dev(gpu, rows_a), keys_b=_dev(gpu, keys), off_b=n_users, first_b=_dev(gpu, first),
                skip_b=_dev(gpu, skip)), live


def _nan_outside(g, live):
    out = np.full_like(g, np.nan)
    out[live] = g[live]
    return out


def _row_norm(rt, lists, max_norm, step=None):
    ws = torch.full((AC.ROW_NORM_BLOCKS,), float("nan"), dtype=torch.float32, device=rt.gpu)
    out = torch.full((2,), float("nan"), dtype=torch.float32, device=rt.gpu)
    rt.ffi.check(rt.lib.lgcn_row_grad_norm(*rt.norm_args(**lists), float(max_norm), ws.data_ptr(), out.data_ptr(),
                                           rt.ffi.ptr(step), rt.stream), "lgcn_row_grad_norm")
    return out.cpu().numpy()


def _row_partials(rt, lists):
    part = torch.full((AC.ROW_NORM_BLOCKS,), float("nan"), dtype=torch.float32, device=rt.gpu)
    rt.ffi.check(rt.lib.lgcn_row_grad_sqnorm(*rt.norm_args(**lists), part.data_ptr(), rt.stream), "lgcn_row_grad_sqnorm")
    return part


def _row_finish(rt, partials, max_norm, step=None):
    out = torch.full((2,), float("nan"), dtype=torch.float32, device=rt.gpu)
    rt.ffi.check(rt.lib.lgcn_row_grad_norm_finish(partials.data_ptr(), partials.numel(), float(max_norm), out.data_ptr(),
                                                  rt.ffi.ptr(step), rt.stream), "lgcn_row_grad_norm_finish")
    return out.cpu().numpy()


def _norm_only_tables(gpu, n_users, n_items, d, g):
    return AC.RowTables(gpu, n_users, n_items, d, None, g, None, None, last=np.zeros(n_users + n_items), step=0, max_t=4)


@pytest.mark.parametrize("d", AC.WIDTHS)
def test_row_grad_norm_matches_float64(gpu, d):
    """lgcn_row_grad_norm over list a + list b (off_b, first_b, skip_b, -1 padding) of two tables
    (U = 37, I = 29; rows 0, U - 1, U, N - 1 listed) against float64 over the rows that count; the
    gradient rows outside them are NaN and the result finite. step_advance moves by exactly 1 and
    NULL leaves it. lgcn_row_grad_sqnorm + lgcn_row_grad_norm_finish over one rank's partials is
    bitwise lgcn_row_grad_norm; over three ranks' concatenated partials within the bar of float64.

    Worst error / bar on an MI355X over the widths: norm 0.024, coefficient 0.021 (one rank);
    0.021 / 0.032 (three ranks)."""
    rng = np.random.default_rng(d)
    lists, live = _row_lists(gpu, rng)
    entries = lists["rows_a"].numel() + lists["keys_b"].numel()
    ranks = [AC._mag(rng, N * d, 1.0).astype(F32).reshape(N, d) for _ in range(3)]
    rts = [_norm_only_tables(gpu, U, I, d, _nan_outside(g, live)) for g in ranks]
    rt = rts[0]
    step = torch.tensor([41], dtype=torch.int64, device=gpu)
    out = _row_norm(rt, lists, 1.0, step)
    assert step.item() == 42
    assert np.isfinite(out).all()
    ratios = AC.norm_ratios(out, [ranks[0][live]], F32(1.0), AC.norm_chain_rows(entries, d))
    print(d, out, ratios)
    AC.record("lgcn_row_grad_norm", f"d={d}", ratios)
    AC.assert_bars(ratios, f"row norm d={d}")
    AC.same_bits(out[1], AC.coef_f32(out[0], 1.0), "coef from the stored norm")
    AC.same_bits(_row_norm(rt, lists, 1.0, None), out, "step_advance = NULL")
    assert step.item() == 42
    parts = [_row_partials(r, lists) for r in rts]
    assert all(bool(torch.isfinite(p).all().item()) for p in parts)
    AC.same_bits(_row_finish(rt, parts[0], 1.0, step), out, "sqnorm + finish, one rank")
    assert step.item() == 43
    out3 = _row_finish(rt, torch.cat(parts), 1.0, None)
    assert step.item() == 43
    ratios3 = AC.norm_ratios(out3, [g[live] for g in ranks], F32(1.0), AC.norm_chain_rows(entries, d, ranks=3))
    AC.record("lgcn_row_grad_norm_finish", f"d={d} ranks=3", ratios3)
    AC.assert_bars(ratios3, f"three ranks d={d}")
    AC.same_bits(out3[1], AC.coef_f32(out3[0], 1.0), "coef from the stored norm, three ranks")


@pytest.mark.parametrize("d,entries", [(512, 8192 + 37), (8, 262144 + 5)])
def test_row_grad_norm_grid_wrap(gpu, d, entries):
    """More entries than 2048 blocks x (256 / LPR) lane groups: the entry loop of k_row_sqnorm
    wraps. One list a over every row of two tables, shuffled.

    Worst error / bar on an MI355X, norm / coefficient: 0.010 / 0.022 (d = 512), 0.011 / 0.016
    (d = 8)."""
    rng = np.random.default_rng(entries)
    n_users = entries // 3
    g = AC._mag(rng, entries * d, 1.0).astype(F32).reshape(entries, d)
    rt = _norm_only_tables(gpu, n_users, entries - n_users, d, g)
    lists = dict(rows_a=_dev(gpu, rng.permutation(entries).astype(np.int32)), keys_b=None, off_b=0, first_b=None,
                 skip_b=None)
    lpr, _ = AC.lanes(d)
    assert entries > AC.ROW_NORM_BLOCKS * (AC.K_BLOCK // lpr)
    out = _row_norm(rt, lists, 1.0)
    ratios = AC.norm_ratios(out, [g], F32(1.0), AC.norm_chain_rows(entries, d))
    print(d, out, ratios)
    AC.record("lgcn_row_grad_norm", f"d={d} wrap", ratios)
    AC.assert_bars(ratios, f"row norm wrap d={d}")
    AC.same_bits(_row_finish(rt, _row_partials(rt, lists), 1.0), out, "sqnorm + finish")


# ---- (e) lgcn_row_adam update, gap 0 -----------------------------------------------------------

@pytest.mark.parametrize("family", ["normal", "first", "cancel", "tiny"])
@pytest.mark.parametrize("mode", [1, 3])
@pytest.mark.parametrize("d", AC.WIDTHS)
def test_row_adam_update_matches_float64(gpu, d, mode, family):
    """One update of the listed rows (every row current: gap 0) within the one-step bars, with the
    float32 constants of the table's row t + 1; mode 1 (no clip, advances the device step) and
    mode 3 (clip = [x, 0.3712], the norm's finish has advanced it). Rows outside the list keep
    every bit of p, m, v and last (their gradient rows are NaN); last[row] == t + 1 for the rest.

    Worst error / bar on an MI355X over the widths and both modes:
      family    m'      v'      p'
      normal    0.194   0.315   0.979
      first     0.042   0.617   0.980
      cancel    0.135   0.316   0.966
      tiny      0.212   0.317   0.762"""
    t = 10
    coef = AC.CLIP_COEF if mode == 3 else None
    rng = np.random.default_rng(d + mode)
    lists, live = _row_lists(gpu, rng)
    p, g, m, v = (a.reshape(N, d) for a in AC.make_family(family, N * d, coef or 1.0, seed=(d, mode)))
    rt = AC.RowTables(gpu, U, I, d, p, _nan_outside(g, live), m, v, last=np.full(N, t), step=t + (mode == 3), max_t=32)
    rt.row_adam(mode, clip=_clip_tensor(gpu, coef), **lists)
    p1, m1, v1, last1 = rt.state()
    assert rt.step.item() == t + 1
    ss, bc2 = rt.consts.cpu().numpy()[t + 1, :2]
    AC.same_bits(np.array([ss, bc2]), np.array(AC.host_consts(t + 1)), "the table's row against the host")
    hyp = AC.hyper()
    ref = adam_ref.adam_step_ref(p[live], g[live], m[live], v[live], F32(coef or 1.0), ss, bc2, *hyp)
    ratios = AC.step_ratios((p1[live], g[live] * F32(coef or 1.0), m1[live], v1[live]), ref, m[live], ss)
    del ratios["g"]  # the update does not store the clipped gradient
    print(d, mode, family, ratios)
    AC.record("lgcn_row_adam", f"d={d}/{family}", ratios)
    AC.assert_bars(ratios, f"row update d={d} mode={mode} {family}")
    rest = np.setdiff1d(np.arange(N), live)
    assert len(rest) > 10
    for got, was, what in ((p1, p, "p"), (m1, m, "m"), (v1, v, "v")):
        AC.same_bits(got[rest], was[rest], f"{what} of the rows outside the list")
    assert (last1[rest] == t).all() and (last1[live] == t + 1).all()


# ---- (f) lgcn_row_adam replays, bitwise the dense kernel ---------------------------------------

GAPS = (0, 1, 2, 3, 7, 300)
T_NOW = 310
VARIANTS = {"fast": ((0.9, 0.999), 1e-8), "markstein": ((0.9, 0.999), 1e-13), "ieee": ((0.9, 0.99), 1e-8)}


def _replay_state(d):
    """[N, d] p, m, v and each row's gap (row r: GAPS[r % 6]). Row r's state pattern is (r // 6) %
    6: ordinary; |m| just above 2^-40 (crosses it mid-replay); |m| below 2^-40; v just above 2^-96
    (crosses); v below 2^-96; exact zeros. m = +-sqrt(v) * uniform(0.3, 1) elementwise, so each
    row also mixes signs; every third element of the ordinary rows is an exact zero pair."""
    rng = np.random.default_rng(d)
    gap = np.array([GAPS[r % 6] for r in range(N)])
    vscale = np.array([1e-4, 2.0 ** -78, 2.0 ** -90, 2.0 ** -95, 1e-33, 0.0])[(np.arange(N) // 6) % 6]
    v = vscale[:, None] * rng.uniform(1.0, 2.0, (N, d))
    m = np.sqrt(v) * rng.uniform(0.3, 1.0, (N, d)) * rng.choice([-1.0, 1.0], (N, d))
    zero = ((np.arange(N) // 6) % 6 == 0)[:, None] & (np.arange(d) % 3 == 0)[None, :]
    v[zero], m[zero] = 0.0, 0.0
    p = rng.standard_normal((N, d)) * 0.1
    p, m, v = (np.ascontiguousarray(a, F32) for a in (p, m, v))
    assert (np.abs(m[m != 0]) > 2.0 ** -40).any() and (np.abs(m[m != 0]) < 2.0 ** -40).any()
    assert (v[v != 0] > 2.0 ** -96).any() and (v[v != 0] < 2.0 ** -96).any() and (m < 0).any() and (v == 0).any()
    assert (v[v != 0] >= np.finfo(F32).tiny * 1e3).all()
    return p, m, v, gap


@functools.lru_cache(maxsize=None)
def _replay_reference(d, variant):
    """The dense kernel applied once per missed step: lgcn_adam_step with a zero gradient and
    dev_scalars at that step's consts row, rows not yet due restored after each step. ->
    (p, m, v) after the catch-up to T_NOW, (p, m, v) after one more step with the gradient g, g."""
    from lgcn_amd import _ffi

    gpu = torch.device("cuda:0")
    betas, eps = VARIANTS[variant]
    p, m, v, gap = _replay_state(d)
    rt = AC.RowTables(gpu, U, I, d, p, np.zeros((N, d), F32), m, v, last=T_NOW - gap, step=T_NOW, betas=betas, eps=eps,
                      max_t=T_NOW + 8)
    hyp = AC.hyper(betas, eps)
    lib, s = _ffi.load(), _ffi.stream_of(gpu)

    def dense(step):
        arr = (_ffi.AdamTensor * 1)(_ffi.AdamTensor(rt.p.data_ptr(), rt.g.data_ptr(), rt.m.data_ptr(), rt.v.data_ptr(), N * d))
        _ffi.check(lib.lgcn_adam_step(arr, 1, float(hyp[0]), float(hyp[1]), float(hyp[2]), float(hyp[3]), 0.0, 1.0, None,
                                      rt.consts.data_ptr() + 16 * step, 0, s), "lgcn_adam_step")

    gap_dev = _dev(gpu, gap)
    for step in range(T_NOW - max(GAPS) + 1, T_NOW + 1):
        idle = (gap_dev < T_NOW - step + 1)[:, None]  # rows whose last step is this one or later
        keep = [t.clone() for t in (rt.p, rt.m, rt.v)]
        dense(step)
        for t, k in zip((rt.p, rt.m, rt.v), keep):
            t.copy_(torch.where(idle, k, t))
    caught = tuple(t.cpu().numpy() for t in (rt.p, rt.m, rt.v))
    g = (np.random.default_rng(d + 1).standard_normal((N, d)) * 1e-3).astype(F32)
    rt.g.copy_(_dev(gpu, g))
    dense(T_NOW + 1)
    stepped = tuple(t.cpu().numpy() for t in (rt.p, rt.m, rt.v))
    assert all(np.isfinite(a).all() for a in (*caught, *stepped))
    return caught, stepped, g


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("d", AC.WIDTHS)
def test_row_adam_replays_bitwise_dense(gpu, d, mode, variant):
    """Rows 0, 1, 2, 3, 7 and 300 steps behind, brought up to date by lgcn_row_adam, are bitwise
    lgcn_adam_step applied once per missed step (held to float64 by the tests above). mode 0: a
    list with duplicates in both halves; mode 2: the flush of rows [0, 53), no multiple of any
    width's rows per block; mode 1: catch-up, then the step's own update. `fast`: beta2 = 0.999,
    eps = 1e-8, the shortened replay arithmetic while the row stays in its range; `markstein`: eps
    = 1e-13 turns that off and keeps the corrected division; `ieee`: beta2 = 0.99, the plain
    division. Rows outside the list (or past n_rows) keep every bit."""
    betas, eps = VARIANTS[variant]
    p, m, v, gap = _replay_state(d)
    caught, stepped, g = _replay_reference(d, variant)
    rng = np.random.default_rng(d + mode)
    out_of_list = np.arange(N) % 5 == 4
    live = np.flatnonzero(~out_of_list) if mode != 2 else np.arange(53)
    rest = np.setdiff1d(np.arange(N), live)
    assert all(set(GAPS) == set(gap[x]) for x in (live, rest)) and 53 % (AC.K_BLOCK // AC.lanes(d)[0]) != 0
    rt = AC.RowTables(gpu, U, I, d, p, _nan_outside(g, live), m, v, last=T_NOW - gap, step=T_NOW, betas=betas, eps=eps,
                      max_t=T_NOW + 8)
    assert rt.consts[0, 0].item() == (1.0 if variant != "ieee" else 0.0)
    if mode == 0:
        a = live[live < 40]
        b = live[live >= 40] - U
        rows_a = rng.permutation(np.concatenate([a, a[::2], a[::3]])).astype(np.int32)
        keys_b = rng.permutation(np.concatenate([b, b, b[::2]])).astype(np.int64)
        assert (b >= 0).all()
        rt.row_adam(0, rows_a=_dev(gpu, rows_a), keys_b=_dev(gpu, keys_b), off_b=U)
    elif mode == 1:
        rt.row_adam(1, rows_a=_dev(gpu, rng.permutation(live).astype(np.int32)))
    else:
        rt.row_adam(2, n_rows=53)
    p1, m1, v1, last1 = rt.state()
    want = stepped if mode == 1 else caught
    for got, ref, was, what in ((p1, want[0], p, "p"), (m1, want[1], m, "m"), (v1, want[2], v, "v")):
        for gp in GAPS:
            sel = live[gap[live] == gp]
            AC.same_bits(got[sel], ref[sel], f"{what}, rows {gp} steps behind")
        AC.same_bits(got[rest], was[rest], f"{what} of the rows outside the list")
    assert (last1[live] == T_NOW + (mode == 1)).all() and (last1[rest] == (T_NOW - gap)[rest]).all()
    assert rt.step.item() == T_NOW + (mode == 1)
    moved = gap[live] > 0
    assert (p1[live][moved] != p[live][moved]).any()


# ---- (g) trajectories --------------------------------------------------------------------------

def _fused_trajectory(gpu, w0, grads, clip, capturable):
    from lgcn_amd.optim import FusedAdam

    ps = [torch.nn.Parameter(_dev(gpu, w)) for w in w0]
    opt = FusedAdam(ps, lr=AC.LR, betas=AC.BETAS, eps=AC.ADAM_EPS, max_grad_norm=clip, capturable=capturable)
    dev_grads = [[_dev(gpu, g) for g in gs] for gs in grads]
    norms = []
    for gs in dev_grads:
        for p, g in zip(ps, gs):
            p.grad = g
        opt.step()
        if clip is not None:
            norms.append(opt.last_norm.clone())
    return [p.detach().cpu().numpy() for p in ps], [float(n[0].item()) for n in norms]


def _lazy_trajectory(gpu, w0, grads, clip):
    from lgcn_amd.optim import RowLazyAdam

    uw, iw = (_dev(gpu, w) for w in w0)
    opt = RowLazyAdam(uw, iw, lr=AC.LR, betas=AC.BETAS, eps=AC.ADAM_EPS, max_grad_norm=clip, max_steps=128)
    deferred = 0
    for gu, gi in grads:
        rows = np.flatnonzero(np.concatenate([np.abs(gu).max(axis=1), np.abs(gi).max(axis=1)]) > 0).astype(np.int32)
        deferred += uw.shape[0] + iw.shape[0] - len(rows)
        ra = _dev(gpu, rows)
        opt.catch_up(ra)
        opt.gu.copy_(_dev(gpu, gu))
        opt.gi.copy_(_dev(gpu, gi))
        opt.step_rows(ra)
    assert deferred > 0.4 * len(grads) * (uw.shape[0] + iw.shape[0])
    opt.flush()
    return [uw.cpu().numpy(), iw.cpu().numpy()]


@pytest.mark.parametrize("d", [8, 64])
@pytest.mark.parametrize("clip", [None, 1.0])
@pytest.mark.parametrize("T", [12, 60])
@pytest.mark.parametrize("kind", ["host", "capturable", "row_lazy"])
def test_trajectory_matches_float64(gpu, kind, T, clip, d):
    """FusedAdam (host constants, device constants) and RowLazyAdam + flush() over T steps on 64 +
    40 rows, 60 % of them idle at each step, row gradient scales 1, 1e-2 and 1e-12, against plain
    float64 Adam (oracle/adam_ref.py). The yardstick is torch.optim.Adam in float32 on the CPU
    (+ clip_grad_norm_) on the same inputs: per row the optimizer may be off by at most 4 x
    max(torch's own error on that row, 2^-24 max|p| of the row). A step count off by one, or
    another step's constants, misses by about 1e-3, four orders above it.

    Worst row ratio (error / that bar) on an MI355X: host 0.40, capturable 0.43, row_lazy 0.43
    (0.25 is a row on which the optimizer is exactly as far off as torch's float32, or within the
    2^-24 floor)."""
    w0, grads = AC.trajectory_case(T, d)
    ref, yard, norms = AC.trajectory_refs(T, d, clip)
    if kind == "row_lazy":
        got = _lazy_trajectory(gpu, w0, grads, clip)
    else:
        got, got_norms = _fused_trajectory(gpu, w0, grads, clip, kind == "capturable")
        if clip is not None:
            np.testing.assert_allclose(got_norms, norms, rtol=1e-5, atol=0)
    ratio = AC.trajectory_ratios(got, yard, ref)
    print(kind, T, clip, d, ratio)
    AC.record("trajectory", f"{kind}/T={T}/clip={clip}/d={d}", {"row_ratio": ratio})
    assert ratio <= 1.0, ratio


# ---- (h) more parameters than one launch takes -------------------------------------------------

MANY_SHAPES = ((5, 8), (3,), (17,), (4, 4), (1,), (9, 2), (6,), (2, 3), (33,), (7,), (10,))


@pytest.mark.parametrize("capturable", [False, True])
@pytest.mark.parametrize("active", [True, False])
def test_fused_adam_clips_by_the_global_norm(gpu, active, capturable):
    """11 parameters (two launches of at most 8) with max_grad_norm = 1 == clip_grad_norm_ over
    all of them + Adam: last_norm[0] is the global norm to 1e-5 at every step, the parameters are
    held to the trajectory bar, with the clip active (norms 3.6 .. 7.4) and inactive (a thousandth
    of that). Clipping each launch's parameters by their own norm instead misses both (measured:
    6,100 x the parameter bar with the clip active, and a reported norm 70 % off either way).

    Worst row ratio on an MI355X: 0.25 in all four cases (no row further off than torch's
    float32 or the 2^-24 floor)."""
    T, scale = 4, (1.0 if active else 1e-3)
    assert len(MANY_SHAPES) == 11
    w0, grads = AC.trajectory_case(T, 0, MANY_SHAPES, 0, scale)
    ref, yard, norms = AC.trajectory_refs(T, 0, 1.0, MANY_SHAPES, 0, scale)
    assert all((n > 2.0) == active and (n < 0.5) != active for n in norms)
    got, got_norms = _fused_trajectory(gpu, w0, grads, 1.0, capturable)
    ratio = AC.trajectory_ratios(got, yard, ref)
    norm_err = float(np.max(np.abs(np.array(got_norms) - norms) / norms))
    print(active, capturable, ratio, norm_err)
    AC.record("trajectory", f"11 parameters/active={active}/capturable={capturable}", {"row_ratio": ratio})
    assert ratio <= 1.0 and norm_err <= 1e-5, (ratio, norm_err)
