"""Shared by tests/test_oracle_bpr.py (CPU) and tests/test_gpu_bpr_kernels.py (GPU): the input
families, the bars of the per-triplet BPR contract (oracle/bpr_ref.py) and the direct C-ABI
launches of lgcn_bpr_fused / lgcn_bpr_fused_cols.

The bars (every row of every output is judged, none exempt):
  cf rows (u | p | n)  max|got - ref| <= RTOL * S_row, S_row the uncancelled scale of the row
                       (oracle/bpr_ref.py); for `normal` and `scaled` inputs also the plain
                       parity bar, RTOL of the row's max|ref|;
  terms[b]             |got - ref| <= RTOL * (sp_ref + sg_ref): softplus' = sg, so an error dz in
                       z moves sp by sg * dz;
  terms[B + b]         RTOL relative (a sum of squares).
"""
from __future__ import annotations

import functools

import numpy as np

import parity
from oracle import bpr_ref

U, I = 37, 53
N = U + I
F_SPLIT = 41   # the propagated table's split, inside the item range
PAIRED = 26    # users 0..25 own item 2k (their "positive partner") and item 2k + 1 ("negative")
WIDTHS = (8, 16, 32, 64, 128, 256, 512)
FAMILIES = ("normal", "scaled", "nearP", "nearN", "equal", "extreme+", "extreme-")
PLAIN_ROW_BAR = ("normal", "scaled")  # families also held to RTOL of the row's own max|ref|
COEFF = 5e-3
F32 = np.float32


def _seed(*parts) -> int:
    return int.from_bytes(repr(parts).encode(), "little") % (2**63)


@functools.lru_cache(maxsize=None)
def make_case(family: str, d: int, B: int):
    """(F, W, u, p, n): float32 [N, d] tables (rows of std 0.1 unless the family says otherwise)
    and int64 [B] ids, all in range; users and items repeat, so one table row serves many
    triplets. The arrays are shared between tests and read-only."""
    rng = np.random.default_rng(_seed(family, d))
    F = (rng.standard_normal((N, d)) * 0.1).astype(F32)
    W = (rng.standard_normal((N, d)) * 0.1).astype(F32)
    users, items = F[:U], F[U:]
    k = np.arange(PAIRED)
    noise = lambda: (rng.standard_normal((PAIRED, d)) * 0.1).astype(F32)
    sloppy = (k % 2 == 1)[:, None]  # every other pair carries noise, the rest is exact
    if family == "scaled":
        users *= (F32(10.0) ** rng.integers(-3, 4, U).astype(F32))[:, None]
        items[0::2] *= F32(1e-3)  # positives are drawn from the even items,
        items[1::2] *= F32(1e3)   # negatives from the odd ones
    elif family == "nearP":
        items[2 * k] = F32(2.0) * users[k] + F32(1e-3) * noise()
    elif family == "nearN":
        items[2 * k + 1] = F32(-0.5) * users[k] + F32(1e-4) * noise()
    elif family in ("extreme+", "extreme-"):
        same, opposite = (2 * k, 2 * k + 1) if family == "extreme+" else (2 * k + 1, 2 * k)
        items[same] = F32(3.0) * users[k] + np.where(sloppy, F32(1e-4) * noise(), F32(0.0))
        items[opposite] = -users[k] + np.where(sloppy, F32(1e-4) * noise(), F32(0.0))
    ids = np.random.default_rng(_seed(family, d, B, "ids"))
    if family in ("normal", "equal"):
        u, p, n = ids.integers(0, U, B), ids.integers(0, I, B), ids.integers(0, I, B)
        if family == "equal":
            n = p.copy()
    elif family == "scaled":
        u, p, n = ids.integers(0, U, B), 2 * ids.integers(0, (I + 1) // 2, B), 2 * ids.integers(0, I // 2, B) + 1
    else:
        u = ids.integers(0, PAIRED, B)
        p = 2 * u if family != "nearN" else ids.integers(0, I, B)
        n = 2 * u + 1 if family != "nearP" else ids.integers(0, I, B)
    out = (F, W, u.astype(np.int64), p.astype(np.int64), n.astype(np.int64))
    for a in out:
        a.setflags(write=False)
    assert 0 <= out[2].min() and out[2].max() < U and 0 <= min(out[3].min(), out[4].min())
    assert max(out[3].max(), out[4].max()) < I
    return out


@functools.lru_cache(maxsize=None)
def case_ref(family: str, d: int, B: int) -> bpr_ref.BprRef:
    F, W, u, p, n = make_case(family, d, B)
    return bpr_ref.bpr_triplet_ref(F, W, U, u, p, n, COEFF)


def touched_mask(seed: int = 0) -> np.ndarray:
    """uint8[N], about half the rows 0 (both users and items on either side)."""
    return (np.random.default_rng(_seed("touched", seed)).random(N) < 0.5).astype(np.uint8)


def kreg_f32(coeff, B, d_full) -> np.float32:
    """k_bpr_fused's float expression: coeff * 2.0f / (float(B) * float(d_full))."""
    return F32(F32(coeff) * F32(2.0)) / (F32(B) * F32(d_full))


def cw_expected(W, u, p, n, coeff, d_full) -> np.ndarray:
    """[3B, d] float32, bit for bit what the kernel stores: float32(kreg) * W[row]."""
    k = kreg_f32(coeff, len(u), d_full)
    rows = np.concatenate([u, U + p, U + n])
    return (k * np.asarray(W, F32)[rows]).astype(F32)


def f32_restatement(F, W, u, p, n):
    """The kernel's formula in plain float32 numpy (numpy's own summation order): (cf [3B, d],
    terms [2B]). What the bars must leave room for; used by the CPU conditioning check."""
    F, W = np.asarray(F, F32), np.asarray(W, F32)
    B = len(u)
    eu, ep, en = F[u], F[U + p], F[U + n]
    wu, wp, wn = W[u], W[U + p], W[U + n]
    dot = lambda x, y: (x * y).sum(1, dtype=F32)
    suu, spp, snn, sup, sun = dot(eu, eu), dot(ep, ep), dot(en, en), dot(eu, ep), dot(eu, en)
    sreg = (dot(wu, wu) + dot(wp, wp) + dot(wn, wn)).astype(F32)
    nu, np_, nn = np.sqrt(suu), np.sqrt(spp), np.sqrt(snn)
    cp, cn = sup / (nu * np_), sun / (nu * nn)
    z = F32(10.0) * (cp - cn)
    with np.errstate(over="ignore"):
        sp = np.where(z > F32(20.0), z, np.log1p(np.exp(z))).astype(F32)
        sg = np.where(z > F32(20.0), F32(1.0), F32(1.0) / (F32(1.0) + np.exp(-z))).astype(F32)
    inv_b = F32(1.0) / F32(B)
    dcp, dcn = (-sg * inv_b)[:, None], (sg * inv_b)[:, None]
    inu, inp, inn = (F32(1.0) / nu)[:, None], (F32(1.0) / np_)[:, None], (F32(1.0) / nn)[:, None]
    a, b, c = eu * inu, ep * inp, en * inn
    cp, cn = cp[:, None], cn[:, None]
    du = (dcp * (b - cp * a) + dcn * (c - cn * a)) * inu
    dp = dcp * (a - cp * b) * inp
    dn = dcn * (a - cn * c) * inn
    out = np.concatenate([du, dp, dn]).astype(F32), np.concatenate([sp, sreg]).astype(F32)
    assert out[0].dtype == F32 and out[1].dtype == F32
    return out


def _ratio(err, bar):
    """max over the entries of err / bar (bar 0: the entry must be exact); nan if anything is."""
    err, bar = np.asarray(err, np.float64), np.asarray(bar, np.float64)
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), np.where(err == 0, 0.0, np.inf))
    r = np.where(np.isnan(err), np.nan, r)
    return float(np.max(r))


def bar_ratios(cf, terms, ref: bpr_ref.BprRef, family: str) -> dict:
    """Worst error / bar of each output (<= 1 passes) against the float64 reference; every row
    counts. Non-finite outputs give nan, which no bar accepts."""
    cf, terms = np.asarray(cf, np.float64), np.asarray(terms, np.float64)
    B = ref.sp.shape[0]
    assert cf.shape == (3 * B, ref.du.shape[1]) and terms.shape == (2 * B,)
    out = {}
    for name, blk, want, S in (("cf_u", cf[:B], ref.du, ref.S_u), ("cf_p", cf[B:2 * B], ref.dp, ref.S_p),
                               ("cf_n", cf[2 * B:], ref.dn, ref.S_n)):
        out[name] = _ratio(np.abs(blk - want).max(axis=1), parity.RTOL * S)
        if family in PLAIN_ROW_BAR:
            out[name + "_plain"] = _ratio(np.abs(blk - want).max(axis=1), parity.RTOL * np.abs(want).max(axis=1))
    out["term_sp"] = _ratio(np.abs(terms[:B] - ref.sp), parity.RTOL * (ref.sp + ref.sg))
    out["term_reg"] = _ratio(np.abs(terms[B:] - ref.sreg), parity.RTOL * ref.sreg)
    return out


def assert_bars(ratios: dict, what: str, limit: float = 1.0) -> None:
    bad = {k: v for k, v in ratios.items() if not v <= limit}
    assert not bad, f"{what}: error / bar over {limit:g}: {bad} (all: {ratios})"


# ---- worst ratios per width, written to parity.stats_dir() / "bpr_kernels.json" ----------------
_WORST: dict = {}


def record(d, ratios: dict, group: str = "fused") -> None:
    slot = _WORST.setdefault(d if isinstance(d, str) else f"d={d}", {}).setdefault(group, {})
    for k, v in ratios.items():
        slot[k] = v if k not in slot or not v <= slot[k] else slot[k]
    parity.record_stats("bpr_kernels", _WORST)


# ---- direct launches through the C ABI ---------------------------------------------------------
SENTINEL = -12345.5


class Launch:
    """One table set on the device: F split at f_split (f_split == N: one tensor, f_hi NULL),
    W split at U, the ids, and the optional touched mask."""

    def __init__(self, gpu, F, W, u, p, n, *, f_split: int = F_SPLIT, touched=None, div: float = 1.0, mul: float = 1.0,
                 coeff: float = COEFF):
        import torch

        from lgcn_amd import _ffi

        assert 0 < f_split <= N and F.shape == W.shape == (N, F.shape[1])
        assert 0 <= min(u.min(), p.min(), n.min()) and u.max() < U and max(p.max(), n.max()) < I  # never out of range
        self.ffi, self.lib, self.gpu, self.torch = _ffi, _ffi.load(), gpu, torch
        up = lambda a: torch.from_numpy(np.array(a)).to(gpu)  # a contiguous, writable copy
        self.d, self.B = int(F.shape[1]), int(len(u))
        self.f_lo, self.f_hi = up(F[:f_split]), (up(F[f_split:]) if f_split < N else None)
        self.w_lo, self.w_hi = up(W[:U]), up(W[U:])
        self.f_split = f_split
        self.u, self.p, self.n = up(u), up(p), up(n)
        self.touched = None if touched is None else up(np.asarray(touched, np.uint8))
        self.div, self.mul, self.coeff = float(div), float(mul), float(coeff)
        self.stream = _ffi.stream_of(gpu)

    def _tables(self):
        ptr = self.ffi.ptr
        return (self.f_lo.data_ptr(), ptr(self.f_hi), self.f_split, self.w_lo.data_ptr(), self.w_hi.data_ptr(), U, U,
                self.u.data_ptr(), self.p.data_ptr(), self.n.data_ptr(), self.B, self.d)

    def outputs(self, with_cw: bool = True):
        t = self.torch
        full = lambda *s: t.full(s, SENTINEL, dtype=t.float32, device=self.gpu)
        return full(3 * self.B, self.d), (full(3 * self.B, self.d) if with_cw else None), full(2 * self.B)

    def fused(self, with_cw: bool = True):
        """lgcn_bpr_fused -> (cf, cw or None, terms) as numpy."""
        cf, cw, terms = self.outputs(with_cw)
        self.ffi.check(self.lib.lgcn_bpr_fused(*self._tables(), self.ffi.ptr(self.touched), self.div, self.mul,
                                               self.coeff, cf.data_ptr(), self.ffi.ptr(cw), terms.data_ptr(),
                                               self.stream), "lgcn_bpr_fused")
        return cf.cpu().numpy(), (None if cw is None else cw.cpu().numpy()), terms.cpu().numpy()

    def cols(self, d_full: int, phase: int, sums, cf, cw, terms) -> None:
        """lgcn_bpr_fused_cols on device tensors the caller owns."""
        self.ffi.check(self.lib.lgcn_bpr_fused_cols(*self._tables(), d_full, self.ffi.ptr(self.touched), self.div,
                                                    self.mul, self.coeff, sums.data_ptr(), phase, self.ffi.ptr(cf),
                                                    self.ffi.ptr(cw), self.ffi.ptr(terms), self.stream),
                       f"lgcn_bpr_fused_cols phase {phase}")
