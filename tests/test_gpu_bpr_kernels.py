"""The BPR loss kernels of csrc/lgcn_bpr.hip called directly through the C ABI and held to the
float64 per-triplet contract of oracle/bpr_ref.py (bars: tests/bpr_checker.py), plus what must
be bitwise: the reg rows, permutation equivariance, the column-sharded form against the fused one,
the segment sum against its sequential restatement. Every case is tiny; ids are always in range."""
import math

import numpy as np
import pytest
import torch

import bpr_checker as BC
from oracle import bpr_ref

pytestmark = pytest.mark.gpu

F32 = np.float32
DIV, MUL = 3.0, float(F32(1 / 3))  # the untouched rows' (W / div) * mul
SPEC_MAX_B = 49152                 # kBprSpecMaxB: speculative F loads below it


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _same_bits(a, b, what):
    assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), f"{what}: not bitwise equal"


def _judge(cf, cw, terms, F_eff, W, u, p, n, family, d, what, group="fused", ref=None, d_full=None):
    """The bars of (a) on one launch's outputs; cw bitwise; the worst ratios recorded."""
    ref = ref if ref is not None else bpr_ref.bpr_triplet_ref(F_eff, W, BC.U, u, p, n, BC.COEFF)
    ratios = BC.bar_ratios(cf, terms, ref, family)
    BC.record(d_full or d, ratios, group)
    BC.assert_bars(ratios, what)
    if cw is not None:
        _same_bits(cw, BC.cw_expected(W, u, p, n, BC.COEFF, d_full or d), what + " cw")
    return ref


# ---- (a) lgcn_bpr_fused against float64 --------------------------------------------------------

@pytest.mark.parametrize("family", BC.FAMILIES)
@pytest.mark.parametrize("B", [1, 1001])
@pytest.mark.parametrize("d", BC.WIDTHS)
def test_bpr_fused_matches_float64(gpu, d, B, family):
    """Every cf row within 1e-5 of its uncancelled scale (normal / scaled: also of its own max),
    both terms, cw bitwise kreg * W, cw = NULL changes no bit of cf / terms. B = 1001 leaves the
    last block partial at every width (2..128 triplets per block).

    Worst error / bar measured on an MI355X over the seven families and both B, per width
    (tests/bpr_checker.py records them in parity.stats_dir() / "bpr_kernels.json", group "fused"):
      d      cf rows (scale bar)   cf rows (plain bar)   terms[b]   terms[B + b]
      8            0.15                  0.24              0.11        0.015
      16           0.12                  0.18              0.097       0.014
      32           0.10                  0.11              0.097       0.014
      64           0.067                 0.079             0.095       0.014
      128          0.053                 0.059             0.095       0.014
      256          0.041                 0.047             0.093       0.018
      512          0.041                 0.042             0.095       0.014
    (untouched rows, test_bpr_fused_untouched_rows: at most 0.21 / 0.29 / 0.14 / 0.016, at d = 8).
    """
    F, W, u, p, n = BC.make_case(family, d, B)
    run = BC.Launch(gpu, F, W, u, p, n)
    cf, cw, terms = run.fused()
    _judge(cf, cw, terms, F, W, u, p, n, family, d, f"{family} d={d} B={B}", ref=BC.case_ref(family, d, B))
    cf0, none, terms0 = run.fused(with_cw=False)
    assert none is None
    _same_bits(cf0, cf, "cf without cw")
    _same_bits(terms0, terms, "terms without cw")
    if family == "equal":  # the same sums feed both cosines and dcp == -dcn: du is exactly 0
        assert not cf[:B].any()
        ln2 = F32(math.log(2.0))
        assert np.all(np.abs(terms[:B] - ln2) <= np.spacing(ln2))  # log1pf(expf(0)), within 1 ulp of ln 2
        _same_bits(terms[:B], np.full(B, terms[0], F32), "softplus(0) of every triplet")


@pytest.mark.parametrize("d", [64, 512])
def test_bpr_fused_single_table(gpu, d):
    """f_hi = NULL with f_split = N: bitwise the two-tensor launch."""
    F, W, u, p, n = BC.make_case("normal", d, 1001)
    one = BC.Launch(gpu, F, W, u, p, n, f_split=BC.N).fused()
    two = BC.Launch(gpu, F, W, u, p, n).fused()
    for a, b, what in zip(one, two, ("cf", "cw", "terms")):
        _same_bits(a, b, what)


# ---- (b) untouched rows, both load strategies --------------------------------------------------

def _untouched_case(d, B, family="normal"):
    F, W, u, p, n = BC.make_case(family, d, B)
    touched = BC.touched_mask()
    F_nan = F.copy()
    F_nan[touched == 0] = np.nan  # a kernel that reads the F row of an untouched entry shows it
    return F_nan, bpr_ref.effective_F(F_nan, W, touched, DIV, MUL), W, u, p, n, touched


@pytest.mark.parametrize("d,B", [(d, 1001) for d in BC.WIDTHS] +
                         [(d, B) for d in (8, 64) for B in (SPEC_MAX_B - 1, SPEC_MAX_B)])
def test_bpr_fused_untouched_rows(gpu, d, B):
    """touched[r] == 0: the row is (W[r] / div) * mul, its F row (NaN here) never reaches an
    output. B < 49152 is the speculative-load instantiation, 49152 the first that is not."""
    F_nan, F_eff, W, u, p, n, touched = _untouched_case(d, B)
    assert np.isfinite(F_eff).all() and 0.3 < touched.mean() < 0.7
    cf, cw, terms = BC.Launch(gpu, F_nan, W, u, p, n, touched=touched, div=DIV, mul=MUL).fused()
    assert np.isfinite(cf).all() and np.isfinite(terms).all()
    _judge(cf, cw, terms, F_eff, W, u, p, n, "normal", d, f"untouched d={d} B={B}", group="untouched")


@pytest.mark.parametrize("d", [8, 64, 512])
def test_bpr_fused_all_touched_equals_null_mask(gpu, d):
    F, W, u, p, n = BC.make_case("normal", d, 1001)
    ones = BC.Launch(gpu, F, W, u, p, n, touched=np.ones(BC.N, np.uint8), div=DIV, mul=MUL).fused()
    null = BC.Launch(gpu, F, W, u, p, n, div=DIV, mul=MUL).fused()
    for a, b, what in zip(ones, null, ("cf", "cw", "terms")):
        _same_bits(a, b, what)


# ---- (c) equivariance and determinism, bitwise -------------------------------------------------

@pytest.mark.parametrize("d", [8, 64, 512])
def test_bpr_fused_permutation_equivariant_and_deterministic(gpu, d):
    """Permuting the triplets permutes cf / cw / terms bit for bit (a lane-group or block
    indexing error that a tolerance hides does not survive this); two runs are bitwise equal."""
    B = 1001
    F, W, u, p, n = BC.make_case("normal", d, B)
    run = BC.Launch(gpu, F, W, u, p, n)
    cf, cw, terms = run.fused()
    for a, b, what in zip(run.fused(), (cf, cw, terms), ("cf", "cw", "terms")):
        _same_bits(a, b, what + " rerun")
    perm = np.random.default_rng(11).permutation(B)
    cf2, cw2, terms2 = BC.Launch(gpu, F, W, u[perm], p[perm], n[perm]).fused()
    for k in range(3):
        _same_bits(cf2[k * B:(k + 1) * B], cf[k * B:(k + 1) * B][perm], f"cf block {k}")
        _same_bits(cw2[k * B:(k + 1) * B], cw[k * B:(k + 1) * B][perm], f"cw block {k}")
    for k in range(2):
        _same_bits(terms2[k * B:(k + 1) * B], terms[k * B:(k + 1) * B][perm], f"terms block {k}")


# ---- (d) lgcn_bpr_fused_cols -------------------------------------------------------------------

def _full(shape, gpu, value=BC.SENTINEL):
    return torch.full(shape, value, dtype=torch.float32, device=gpu)


@pytest.mark.parametrize("shares,with_touched", [((32, 16, 8, 8), False), ((32, 16, 8, 8), True), ((64, 32), False),
                                                 ((512,), False)])
def test_bpr_fused_cols_shares(gpu, shares, with_touched):
    """d_full split into unequal column shares, each in tensors of its own. Phase 1 writes this
    share's six partial sums and nothing else; phase 2, given the shares' sums added in float32 in
    share order (the all-reduce), writes columns that concatenate to rows meeting the bars of the
    full-width float64 reference, cw with the FULL width's reg scale, the same terms everywhere."""
    d_full, B = sum(shares), 1001
    rng = np.random.default_rng(d_full + with_touched)
    F = (rng.standard_normal((BC.N, d_full)) * 0.1).astype(F32)
    W = (rng.standard_normal((BC.N, d_full)) * 0.1).astype(F32)
    u, p, n = rng.integers(0, BC.U, B), rng.integers(0, BC.I, B), rng.integers(0, BC.I, B)
    touched, F_eff = None, F
    if with_touched:
        touched = BC.touched_mask(1)
        F_eff = bpr_ref.effective_F(F, W, touched, DIV, MUL)
        F = F.copy()
        F[touched == 0] = np.nan
    ref = bpr_ref.bpr_triplet_ref(F_eff, W, BC.U, u, p, n, BC.COEFF)
    runs, partials, c0 = [], [], 0
    for ds in shares:
        sl = slice(c0, c0 + ds)
        c0 += ds
        run = BC.Launch(gpu, F[:, sl], W[:, sl], u, p, n, touched=touched, div=DIV if with_touched else 1.0,
                        mul=MUL if with_touched else 1.0)
        sums = _full((B, 6), gpu)
        cf, cw, terms = run.outputs()
        run.cols(d_full, 1, sums, cf, cw, terms)
        for t, what in ((cf, "cf"), (cw, "cw"), (terms, "terms")):  # phase 1 writes nothing else
            assert bool((t == BC.SENTINEL).all().item()), f"phase 1 wrote {what}"
        got = sums.cpu().numpy()
        part = bpr_ref.bpr_triplet_ref(F_eff[:, sl], W[:, sl], BC.U, u, p, n, BC.COEFF, d_full=d_full)
        ratios = {}
        for k, name in enumerate(("suu", "spp", "snn")):
            ratios["sum_" + name] = BC._ratio(np.abs(got[:, k] - part.sums[:, k]), BC.parity.RTOL * part.sums[:, k])
        ratios["sum_sreg"] = BC._ratio(np.abs(got[:, 5] - part.sreg), BC.parity.RTOL * part.sreg)
        ratios["sum_sup"] = BC._ratio(np.abs(got[:, 3] - part.sup), BC.parity.RTOL * part.abs_up)
        ratios["sum_sun"] = BC._ratio(np.abs(got[:, 4] - part.sun), BC.parity.RTOL * part.abs_un)
        BC.record(d_full, ratios, "cols_phase1")
        BC.assert_bars(ratios, f"phase 1 share {sl}")
        runs.append(run)
        partials.append(got)
    total = partials[0].copy()
    for q in partials[1:]:
        total = (total + q).astype(F32)
    cols_cf, cols_cw, all_terms = [], [], []
    for run in runs:
        sums = torch.from_numpy(total).to(gpu)
        cf, cw, terms = run.outputs()
        run.cols(d_full, 2, sums, cf, cw, terms)
        _same_bits(sums.cpu().numpy(), total, "phase 2 must not write sums")
        cols_cf.append(cf.cpu().numpy())
        cols_cw.append(cw.cpu().numpy())
        all_terms.append(terms.cpu().numpy())
    for t in all_terms[1:]:
        _same_bits(t, all_terms[0], "terms of every share")
    _judge(np.concatenate(cols_cf, axis=1), np.concatenate(cols_cw, axis=1), all_terms[0], F_eff, W, u, p, n, "normal",
           None, f"cols {shares}", group="cols_phase2", ref=ref, d_full=d_full)


@pytest.mark.parametrize("d", [64, 512])
def test_bpr_fused_cols_single_share_bitwise_fused(gpu, d):
    """d == d_full: phase 1 then phase 2 is lgcn_bpr_fused bit for bit (no contraction in the
    build, and the six sums pass through memory unrounded)."""
    F, W, u, p, n = BC.make_case("normal", d, 1001)
    run = BC.Launch(gpu, F, W, u, p, n)
    want = run.fused()
    sums = _full((1001, 6), gpu)
    cf, cw, terms = run.outputs()
    run.cols(d, 1, sums, None, None, None)
    run.cols(d, 2, sums, cf, cw, terms)
    for a, b, what in zip((cf, cw, terms), want, ("cf", "cw", "terms")):
        _same_bits(a.cpu().numpy(), b, what)


# ---- (e) lgcn_bpr_loss, lgcn_loss_accumulate ---------------------------------------------------

LOSS_D, LOSS_COEFF = 64, 2.0 ** -8  # a coefficient float32 holds exactly


def _loss_terms(B, mixed):
    rng = np.random.default_rng(B + mixed)
    if mixed:
        return (rng.standard_normal(2 * B) * 3).astype(F32)
    t0 = np.logaddexp(0.0, rng.standard_normal(B) * 3)          # softplus-like, positive
    t1 = (rng.standard_normal((B, 3)) ** 2).sum(1) * LOSS_D * 0.01  # sums of squares
    return np.concatenate([t0, t1]).astype(F32)


def _loss_bound(t, B):
    """Reference and error bound of the loss sum.

    The kernel adds float32 numbers in a fixed tree and closes with a few more operations; each
    operation has relative error <= 2^-24, so (to first order) the result is off by at most
    (operations on the longest path) * 2^-24 * (the value the same expression has on |terms|).
    Longest path, single block of 1024 threads: a thread adds its ceil(B / 1024) strided terms one
    after another, then 6 shuffle steps across the wave and 16 wave sums in thread 0: at most
    ceil(B / 1024) + 22 additions; the close adds (x / B) / 10 or coeff * (x / (B * d)) (3
    operations) and the final sum (1): ceil(B / 1024) + 26. Two stages: stage one is a block of
    256 threads over ceil(B / 256) terms (ceil(B / 65536) per thread, 6 shuffles, 4 wave sums),
    stage two the single block over 256 partial sums (1 + 6 + 16): shorter than the single block's
    path for every B. ceil(B / 1024) + 32 covers both with the second-order terms."""
    t0, t1 = t[:B].astype(np.float64), t[B:].astype(np.float64)
    want = -(t0.sum() / B) / 10.0 + LOSS_COEFF * t1.sum() / (B * LOSS_D)
    bound = (math.ceil(B / 1024) + 32) * 2.0 ** -24 * (np.abs(t0).sum() / (10.0 * B)
                                                       + abs(LOSS_COEFF) * np.abs(t1).sum() / (B * LOSS_D))
    return want, bound


@pytest.mark.parametrize("B,mixed", [(B, False) for B in (1, 63, 1024, 8193, 16383, 16384, 16385, 50001)] +
                         [(63, True), (16385, True)])
def test_bpr_loss_matches_float64(gpu, B, mixed):
    """lgcn_bpr_loss against the value the loss has: single block (partial = NULL) at every B,
    two stages (a 2 * LGCN_LOSS_PARTS scratch) from B = LGCN_LOSS_FUSED_MAX_B; below it the
    scratch changes no bit. mixed: first halves of both signs, as the scatter test's terms."""
    from lgcn_amd import _ffi

    lib, s = _ffi.load(), _ffi.stream_of(gpu)
    assert _ffi.LOSS_FUSED_MAX_B == 16384 and _ffi.LOSS_PARTS == 256
    t = _loss_terms(B, mixed)
    terms = torch.from_numpy(t).to(gpu)
    want, bound = _loss_bound(t, B)
    got = {}
    for name in ("single", "scratch"):
        loss = torch.full((1,), float("nan"), dtype=torch.float32, device=gpu)
        part = torch.full((2 * _ffi.LOSS_PARTS,), float("nan"), dtype=torch.float32, device=gpu) if name == "scratch" else None
        _ffi.check(lib.lgcn_bpr_loss(terms.data_ptr(), B, LOSS_D, LOSS_COEFF, loss.data_ptr(), _ffi.ptr(part), s),
                   "lgcn_bpr_loss")
        got[name] = loss.cpu().numpy()
        err = abs(float(got[name][0]) - want)
        BC.record("loss", {f"{name}_B={B}" + ("_mixed" if mixed else ""): err / bound}, "bound")
        assert err <= bound, (name, B, float(got[name][0]), want, err, bound)
        if name == "scratch":
            used = bool(torch.isfinite(part).all().item())
            assert used == (B >= _ffi.LOSS_FUSED_MAX_B), "two stages exactly from LGCN_LOSS_FUSED_MAX_B"
    if B < _ffi.LOSS_FUSED_MAX_B:
        _same_bits(got["single"], got["scratch"], "the scratch below LGCN_LOSS_FUSED_MAX_B")


def test_bpr_loss_empty_batch_is_nan(gpu):
    """B = 0 is OK and writes NaN, as torch's mean of nothing (documented in the kernel)."""
    from lgcn_amd import _ffi

    loss = torch.zeros(1, dtype=torch.float32, device=gpu)
    _ffi.check(_ffi.load().lgcn_bpr_loss(None, 0, 64, 5e-3, loss.data_ptr(), None, _ffi.stream_of(gpu)), "lgcn_bpr_loss")
    assert math.isnan(loss.item())


def test_loss_accumulate_is_the_python_float_sum(gpu):
    from lgcn_amd import _ffi

    lib, s = _ffi.load(), _ffi.stream_of(gpu)
    acc = torch.full((1,), 0.1, dtype=torch.float64, device=gpu)
    want = 0.1
    for value, w in ((-0.0693147, 4803.0), (0.3333333, 7.0), (-1.2345678e-3, 162001.0)):
        loss = torch.tensor([value], dtype=torch.float32, device=gpu)
        _ffi.check(lib.lgcn_loss_accumulate(loss.data_ptr(), w, acc.data_ptr(), s), "lgcn_loss_accumulate")
        want += float(F32(value)) * w
    assert acc.cpu().numpy().tobytes() == np.float64(want).tobytes()


# ---- (f) lgcn_segment_rows ---------------------------------------------------------------------

SEG_N, SEG_E, SEG_SPLIT = 203, 3000, 101


def _segment_ref(rowptr, perm, C, out0, add, mul, div):
    """Sequential float32: the rows in the order listed, then (acc * mul) / div."""
    out = out0.copy()
    mul, div = F32(mul), F32(div)
    for r in range(len(rowptr) - 1):
        beg, end = int(rowptr[r]), int(rowptr[r + 1])
        if add and beg == end:
            continue
        acc = np.zeros(C.shape[1], F32)
        for e in range(beg, end):
            acc = (acc + C[perm[e]]).astype(F32)
        v = ((acc * mul).astype(F32) / div).astype(F32)
        out[r] = (out[r] + v).astype(F32) if add else v
    return out


def _segment_run(gpu, rowptr, perm, C, out0, add, mul, div, n_rows, split):
    from lgcn_amd import _ffi

    d = C.shape[1]
    lo, hi = torch.from_numpy(out0[:split].copy()).to(gpu), torch.from_numpy(out0[split:].copy()).to(gpu)
    Cg = torch.from_numpy(C).to(gpu)
    _ffi.check(_ffi.load().lgcn_segment_rows(rowptr.data_ptr(), perm.data_ptr(), Cg.data_ptr(), n_rows, d, lo.data_ptr(),
                                             hi.data_ptr(), split, add, mul, div, _ffi.stream_of(gpu)),
               "lgcn_segment_rows")
    return torch.cat([lo, hi]).cpu().numpy()


@pytest.mark.parametrize("d", BC.WIDTHS)
def test_segment_rows_bitwise_sequential(gpu, d):
    """N = 203 rows (no multiple of any width's rows per block), 3,000 contributions grouped by
    lgcn_csr_build: one hub row with 1,500 of them, many empty rows; out in two tensors.
    add = 0 writes every row (exact 0 where empty, over a NaN prefill); add = 1 adds and leaves
    rows without contributions bit for bit."""
    from lgcn_amd import _ffi

    lib, s = _ffi.load(), _ffi.stream_of(gpu)
    rng = np.random.default_rng(d)
    keys_np = np.concatenate([np.full(SEG_E // 2, 77), rng.choice(np.arange(0, SEG_N, 3), SEG_E - SEG_E // 2)])
    rng.shuffle(keys_np)
    keys = torch.from_numpy(keys_np.astype(np.int64)).to(gpu)
    rowptr = torch.empty(SEG_N + 1, dtype=torch.int64, device=gpu)
    col = torch.empty(SEG_E, dtype=torch.int32, device=gpu)
    perm = torch.empty(SEG_E, dtype=torch.int32, device=gpu)
    err = torch.zeros(1, dtype=torch.int64, device=gpu)
    nb = _ffi._sz(0)
    _ffi.check(lib.lgcn_csr_workspace_size(SEG_E, SEG_N, nb), "ws")
    ws = torch.empty(max(1, nb.value), dtype=torch.uint8, device=gpu)
    _ffi.check(lib.lgcn_csr_build(keys.data_ptr(), keys.data_ptr(), SEG_E, SEG_N, rowptr.data_ptr(), col.data_ptr(),
                                  perm.data_ptr(), err.data_ptr(), ws.data_ptr(), ws.numel(), s), "csr")
    assert int(err.item()) == 0
    rp, pm = rowptr.cpu().numpy(), perm.cpu().numpy()
    counts = np.diff(rp)
    assert counts[77] >= SEG_E // 2 and (counts == 0).sum() > SEG_N // 2 and rp[-1] == SEG_E
    np.testing.assert_array_equal(pm, np.argsort(keys_np, kind="stable"))
    C = rng.standard_normal((SEG_E, d)).astype(F32)
    for add in (0, 1):
        out0 = np.full((SEG_N, d), np.nan, F32) if add == 0 else rng.standard_normal((SEG_N, d)).astype(F32)
        got = _segment_run(gpu, rowptr, perm, C, out0, add, MUL, DIV, SEG_N, SEG_SPLIT)
        want = _segment_ref(rp, pm, C, out0, add, MUL, DIV)
        _same_bits(got, want, f"add={add}")
        if add == 0:
            assert np.isfinite(got).all() and not got[counts == 0].any()
        else:
            _same_bits(got[counts == 0], out0[counts == 0], "rows without contributions")
            assert (got[counts > 0] != out0[counts > 0]).any()


def test_segment_rows_order_is_as_listed(gpu):
    """A hand-made perm that is not sorted within a row: the rows are added in the listed order
    (float32 addition does not commute across three terms of mixed size)."""
    d = 16
    rowptr_np = np.array([0, 3, 3, 7, 8], np.int64)
    perm_np = np.array([5, 0, 3, 7, 6, 1, 2, 4], np.int32)
    C = (np.random.default_rng(2).standard_normal((8, d)) * 10.0 ** np.arange(-3, 5)[:, None]).astype(F32)
    rowptr, perm = torch.from_numpy(rowptr_np).to(gpu), torch.from_numpy(perm_np).to(gpu)
    for add in (0, 1):
        out0 = np.full((4, d), 0.5, F32)
        got = _segment_run(gpu, rowptr, perm, C, out0, add, 1.0, 1.0, 4, 2)
        _same_bits(got, _segment_ref(rowptr_np, perm_np, C, out0, add, 1.0, 1.0), f"add={add}")
    sorted_perm = np.array([0, 3, 5, 1, 2, 6, 7, 4], np.int32)
    assert not np.array_equal(_segment_ref(rowptr_np, sorted_perm, C, out0, 0, 1.0, 1.0),
                              _segment_ref(rowptr_np, perm_np, C, out0, 0, 1.0, 1.0)), "the case cannot tell the orders apart"


# ---- (g) argument errors: refused before any launch --------------------------------------------

def test_argument_errors(gpu):
    from lgcn_amd import _ffi

    lib, s = _ffi.load(), _ffi.stream_of(gpu)
    buf = torch.zeros(4096, dtype=torch.float32, device=gpu)  # every pointer below is valid device memory
    ids = torch.zeros(8, dtype=torch.int64, device=gpu)
    P, Q, K = buf.data_ptr(), buf.data_ptr() + 4, ids.data_ptr()

    def fused(f_lo=P, B=4, d=8, cf=P):
        return lib.lgcn_bpr_fused(f_lo, None, 4, P, None, 4, 2, K, K, K, B, d, None, 1.0, 1.0, 5e-3, cf, P, P, s)

    def cols(f_lo=P, B=4, d=8, d_full=8, phase=2, cf=P):
        return lib.lgcn_bpr_fused_cols(f_lo, None, 4, P, None, 4, 2, K, K, K, B, d, d_full, None, 1.0, 1.0, 5e-3, P,
                                       phase, cf, P, P, s)

    def seg(out=P, d=8, C=P):
        return lib.lgcn_segment_rows(K, K, C, 1, d, out, None, 1, 0, 1.0, 1.0, s)

    assert fused(d=12) == cols(d=12, d_full=12) == seg(d=12) == _ffi.E_UNSUPPORTED
    assert fused(f_lo=Q) == cols(f_lo=Q) == fused(cf=Q) == cols(cf=Q) == _ffi.E_UNSUPPORTED
    assert seg(out=Q) == seg(C=Q) == _ffi.E_UNSUPPORTED
    assert seg(d=12) == _ffi.E_UNSUPPORTED and "8..512" in lib.lgcn_last_error().decode()
    assert fused(B=-1) == cols(B=-1) == _ffi.E_ARG
    assert cols(phase=0) == cols(phase=3) == _ffi.E_ARG
    assert cols(d=16, d_full=8) == _ffi.E_ARG
    null = (None, None, 0, None, None, 0, 0, None, None, None, 0, 8)
    assert lib.lgcn_bpr_fused(*null, None, 1.0, 1.0, 5e-3, None, None, None, s) == 0
    assert lib.lgcn_bpr_fused_cols(*null, 8, None, 1.0, 1.0, 5e-3, None, 1, None, None, None, s) == 0
    torch.cuda.synchronize()
    assert not buf.any().item()  # nothing was launched: the buffer every pointer aimed at is untouched
