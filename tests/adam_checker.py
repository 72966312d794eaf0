"""Shared by tests/test_oracle_adam.py (CPU) and tests/test_gpu_optim_kernels.py (GPU): the bars
the clip-norm and Adam kernels (csrc/lgcn_optim.hip, csrc/lgcn_rowadam.hip) are held to against
the float64 contract of oracle/adam_ref.py, the input families, and the direct C-ABI launches.

One-step bars, EPS = 2^-24 (half a float32 ulp, relative), reference quantities in float64:
  g'   EPS |g'|                      one multiplication (and bitwise fl(g * coef))
  m'   4 EPS (|m| + |g'|)            g' (1), g' - m (1), omb1 * (1), m + (1)
  v'   6 EPS v'                      v * beta2 (1), g' (2, squared), g' * g' (1), omb2 * (1), + (1)
  p'   |step_size| bar_m / denom + 9 EPS |upd| + EPS |p'|
                                     m' through the quotient; v' through the square root (3),
                                     sqrt, / bc2_sqrt, + eps, m / denom, step_size * (5), slack 1;
                                     the half ulp of p' itself
The clip norm: relative (L + 4) EPS, L the float32 additions on the longest chain into the sum
(norm_chain_dense / norm_chain_rows below: nonnegative summands, so the sum is off by at most
L EPS relative to first order; the 4 covers the square's own rounding, the square root and the
second-order terms).
"""
from __future__ import annotations

import ctypes
import functools
import math

import numpy as np

import parity
from bpr_checker import _ratio, _seed
from oracle import adam_ref

F32 = np.float32
EPS = 2.0 ** -24
K_BLOCK = 256            # kBlock of csrc/lgcn_common.h
DENSE_NORM_BLOCKS = 1024  # kNormBlocks (lgcn_grad_norm_workspace_floats)
ROW_NORM_BLOCKS = 2048    # kRowNormBlocks (lgcn_row_grad_norm_workspace_floats)
ADAM_MAX_BLOCKS = 8192    # lgcn_adam_step's grid cap
WIDTHS = (8, 16, 32, 64, 128, 256, 512)
FAMILIES = ("normal", "tiny", "huge", "zero_g", "first", "cancel", "stale")
STEPS = (1, 2, 10, 1000, 20000)
CLIP_COEF = 0.3712
LR, BETAS, ADAM_EPS = 1e-3, (0.9, 0.999), 1e-8
SENTINEL = -12345.5
GUARD = 8


def lanes(d: int) -> tuple[int, int]:
    """(LPR, NV) of the row kernels' instantiation for width d (LGCN_ROW_DISPATCH)."""
    return (min(d // 4, 64), 2 if d == 512 else 1)


# ---- the step's constants ----------------------------------------------------------------------

def host_consts(t: int, lr: float = LR, betas=BETAS) -> tuple[np.float32, np.float32]:
    """(step_size, bc2_sqrt) of step t: the double formulas of lgcn_adam_prologue on the host
    (lr as the float32 the ABI takes), rounded to float32 once."""
    lr = float(F32(lr))
    bc1 = 1.0 - float(betas[0]) ** t
    bc2 = 1.0 - float(betas[1]) ** t
    return F32(-(lr / bc1)), F32(math.sqrt(bc2))


def hyper(betas=BETAS, eps: float = ADAM_EPS) -> tuple[np.float32, np.float32, np.float32, np.float32]:
    """(omb1, beta2, omb2, eps) as the float32 values the ABI receives from FusedAdam's doubles."""
    return F32(1 - betas[0]), F32(betas[1]), F32(1 - betas[1]), F32(eps)


# ---- input families ----------------------------------------------------------------------------

def _mag(rng, n, scale, signed=True):
    """scale * uniform(0.5, 2), random sign: nothing near zero, so no square goes subnormal."""
    x = scale * rng.uniform(0.5, 2.0, n)
    return x * rng.choice([-1.0, 1.0], n) if signed else x


def make_family(family: str, n: int, coef: float = 1.0, seed=0):
    """(p, g, m, v) float32 [n]. Every intermediate of the update stays a normal float32."""
    rng = np.random.default_rng(_seed("adam", family, n, seed))
    p = _mag(rng, n, 0.1)
    gs, ms, vs = {"normal": (1.0, 1.0, 1.0), "tiny": (1e-14, 1e-14, 1e-28), "huge": (1e8, 1e8, 1e16),
                  "zero_g": (0.0, 1e-3, 1e-6), "first": (1.0, 0.0, 0.0), "cancel": (1.0, 1.0, 1.0),
                  "stale": (1e-3, 1e-20, 1e-30)}[family]
    g, m, v = _mag(rng, n, gs), _mag(rng, n, ms), _mag(rng, n, vs, signed=False)
    if family == "first":  # any gradient: magnitudes from 1e-10 to 1e6
        g = g * 10.0 ** rng.integers(-10, 7, n)
    if family == "cancel":  # g * coef == m to about 1e-6: the first moment's difference cancels
        g = F32(m).astype(np.float64) / coef * (1.0 + 1e-6 * rng.standard_normal(n))
    out = tuple(np.ascontiguousarray(a, F32) for a in (p, g, m, v))
    for a in out:
        a.setflags(write=False)
    return out


def emulate_adam_elem(p, g, m, v, coef, step_size, bc2_sqrt, omb1, beta2, omb2, eps):
    """adam_elem (csrc/lgcn_optim.hip) in numpy float32: the same operations in the same order,
    each correctly rounded (no contraction, IEEE sqrt and division, as the build has them)."""
    p, g, m, v = (np.asarray(a, F32) for a in (p, g, m, v))
    coef, step_size, bc2_sqrt, omb1, beta2, omb2, eps = (F32(x) for x in (coef, step_size, bc2_sqrt, omb1, beta2,
                                                                          omb2, eps))
    g = g * coef
    m = m + omb1 * (g - m)
    v = v * beta2
    v = v + omb2 * (g * g)
    denom = np.sqrt(v) / bc2_sqrt + eps
    p = p + step_size * (m / denom)
    assert p.dtype == g.dtype == m.dtype == v.dtype == F32
    return p, g, m, v


def step_ratios(got, ref: adam_ref.AdamStep, m_in, step_size) -> dict:
    """Worst error / bar of g', m', v', p' (got: the four float32 arrays after the step)."""
    p, g, m, v = (np.asarray(a, np.float64) for a in got)
    bar_m = 4 * EPS * (np.abs(np.asarray(m_in, np.float64)) + np.abs(ref.g))
    bar_p = abs(float(step_size)) * bar_m / ref.denom + 9 * EPS * np.abs(ref.upd) + EPS * np.abs(ref.p)
    return {"g": _ratio(np.abs(g - ref.g), EPS * np.abs(ref.g)), "m": _ratio(np.abs(m - ref.m), bar_m),
            "v": _ratio(np.abs(v - ref.v), 6 * EPS * ref.v), "p": _ratio(np.abs(p - ref.p), bar_p)}


def assert_bars(ratios: dict, what: str, limit: float = 1.0) -> None:
    bad = {k: v for k, v in ratios.items() if not v <= limit}
    assert not bad, f"{what}: error / bar over {limit:g}: {bad} (all: {ratios})"


# ---- the clip norm's bar -----------------------------------------------------------------------

def _ceil(a: int, b: int) -> int:
    return -(-a // b)


def norm_chain_finish(nparts: int) -> int:
    """k_norm_finish / k_norm_finish_rows, one block of K_BLOCK threads over nparts partials: a
    thread adds its ceil(nparts / K_BLOCK) partials in turn, 6 shuffle steps across the wave, then
    thread 0 adds the K_BLOCK / 64 wave sums."""
    return _ceil(nparts, K_BLOCK) + 6 + K_BLOCK // 64


def dense_norm_blocks(numels) -> int:
    return min(DENSE_NORM_BLOCKS, max(1, _ceil(sum(numels), K_BLOCK)))


def norm_chain_dense(numels, aligned=None) -> int:
    """L of lgcn_grad_norm. A thread of k_sqnorm_partial walks every tensor with the stride of the
    whole grid: per float4 it adds three times inside the float4 and once into its accumulator
    (counted 4 per iteration), then at most one scalar-tail element of an aligned tensor (the
    tail is shorter than the stride), or ceil(numel / stride) single elements of a tensor whose
    gradient is not 16-byte aligned; then 6 shuffle steps, the sum over the block's waves, and the
    finish over the blocks' partials."""
    aligned = [True] * len(numels) if aligned is None else aligned
    blocks = dense_norm_blocks(numels)
    stride = blocks * K_BLOCK
    per_thread = 0
    for n, al in zip(numels, aligned):
        if al:
            per_thread += 4 * _ceil(n // 4, stride) + (1 if n % 4 else 0)
        else:
            per_thread += _ceil(n, stride)
    return per_thread + 6 + K_BLOCK // 64 + norm_chain_finish(blocks)


def norm_chain_rows(n_entries: int, d: int, ranks: int = 1) -> int:
    """L of lgcn_row_grad_norm (ranks = 1) or of lgcn_row_grad_sqnorm on each of `ranks` ranks +
    lgcn_row_grad_norm_finish over their concatenated partials. k_row_sqnorm runs ROW_NORM_BLOCKS
    blocks of K_BLOCK / LPR lane groups; a lane adds NV float4 (4 additions each, as above) per
    entry its group meets, ceil(entries / (blocks * groups)) of them."""
    lpr, nv = lanes(d)
    per_thread = 4 * nv * _ceil(n_entries, ROW_NORM_BLOCKS * (K_BLOCK // lpr))
    return per_thread + 6 + K_BLOCK // 64 + norm_chain_finish(ROW_NORM_BLOCKS * ranks)


def norm_bar(L: int) -> float:
    """relative, on the norm (and on the clip coefficient: its sum and quotient add 2 EPS to a
    norm that is really off by at most (L / 2 + 1.5) EPS, the square root halving the sum's error)."""
    return (L + 4) * EPS


def coef_f32(norm_f32, max_norm) -> np.float32:
    """k_norm_finish's float expression on the norm it stored."""
    c = F32(max_norm) / (F32(norm_f32) + F32(1e-6))
    return c if c < F32(1.0) else F32(1.0)


def norm_ratios(out, grads, max_norm, L: int) -> dict:
    """out = (norm, coef) float32 of a norm kernel against float64 over `grads`."""
    norm, coef = adam_ref.clip_ref(grads, max_norm)
    bar = norm_bar(L)
    return {"norm": _ratio(abs(float(out[0]) - norm), bar * norm), "coef": _ratio(abs(float(out[1]) - coef), bar * coef)}


# ---- trajectories ------------------------------------------------------------------------------
TRAJ_ROWS = (64, 40)
TRAJ_HEADROOM = 4.0  # two float32 runs of one formula


@functools.lru_cache(maxsize=None)
def trajectory_case(T: int, d: int, shapes=None, seed: int = 0, scale_grad: float = 1.0):
    """(w0, grads): float32 parameter arrays and grads[t][k]; 60 % of the rows of every array have
    an exactly zero gradient at each step, row gradient scales cycle through 1, 1e-2, 1e-12."""
    shapes = tuple((r, d) for r in TRAJ_ROWS) if shapes is None else shapes
    rng = np.random.default_rng(_seed("trajectory", T, d, shapes, seed))
    w0 = tuple((rng.standard_normal(s) * 0.1).astype(F32) for s in shapes)
    grads = []
    for _ in range(T):
        gs = []
        for s in shapes:
            rows = s[0]
            scale = np.array([1.0, 1e-2, 1e-12])[np.arange(rows) % 3] * scale_grad
            g = rng.standard_normal(s) * scale.reshape((rows,) + (1,) * (len(s) - 1))
            g[rng.random(rows) < 0.6] = 0.0
            gs.append(g.astype(F32))
        grads.append(tuple(gs))
    for a in (*w0, *(g for gs in grads for g in gs)):
        a.setflags(write=False)
    return w0, tuple(grads)


def torch_adam_fp32(w0, grads, lr, betas, eps, max_norm):
    """The yardstick: torch.optim.Adam in float32 on the CPU, clip_grad_norm_ before each step."""
    import torch

    ps = [torch.nn.Parameter(torch.from_numpy(np.array(w, F32))) for w in w0]
    opt = torch.optim.Adam(ps, lr=lr, betas=betas, eps=eps)
    norms = []
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = torch.from_numpy(np.array(g, F32))
        if max_norm is not None:
            norms.append(float(torch.nn.utils.clip_grad_norm_(ps, max_norm=max_norm)))
        opt.step()
    return [p.detach().numpy().copy() for p in ps], norms


@functools.lru_cache(maxsize=None)
def trajectory_refs(T: int, d: int, clip, shapes=None, seed: int = 0, scale_grad: float = 1.0):
    """(float64 reference weights, torch-float32 weights, float64 norms) of trajectory_case."""
    w0, grads = trajectory_case(T, d, shapes, seed, scale_grad)
    ref, _, _, norms = adam_ref.adam_trajectory_ref(w0, grads, LR, BETAS, ADAM_EPS, clip)
    yard, _ = torch_adam_fp32(w0, grads, LR, BETAS, ADAM_EPS, clip)
    return ref, yard, norms


def trajectory_ratios(got, yard, ref) -> float:
    """Worst row of: the optimizer's error / (TRAJ_HEADROOM * max(torch-float32's error on that
    row, EPS * max|p| of the row)), errors against the float64 trajectory, max over the row."""
    worst = 0.0
    for a, y, r in zip(got, yard, ref):
        r = np.asarray(r, np.float64).reshape(r.shape[0], -1) if r.ndim > 1 else np.asarray(r, np.float64).reshape(1, -1)
        a = np.asarray(a, np.float64).reshape(r.shape)
        y = np.asarray(y, np.float64).reshape(r.shape)
        bar = TRAJ_HEADROOM * np.maximum(np.abs(y - r).max(axis=1), EPS * np.abs(r).max(axis=1))
        worst = max(worst, _ratio(np.abs(a - r).max(axis=1), bar))
    return worst


# ---- worst ratios, written to parity.stats_dir() / "optim_kernels.json" ------------------------
_WORST: dict = {}


def record(kernel: str, key: str, ratios: dict) -> None:
    """kernel: the ABI entry; key: width / family (or the case's name)."""
    slot = _WORST.setdefault(kernel, {}).setdefault(key, {})
    for k, v in ratios.items():
        slot[k] = v if k not in slot or not v <= slot[k] else slot[k]
    parity.record_stats("optim_kernels", _WORST)


# ---- direct launches through the C ABI ---------------------------------------------------------

def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), f"{what}: not bitwise equal"


class Slab:
    """A float32 array as an interior view of a larger device allocation filled with SENTINEL:
    16-byte aligned (4 floats in) or off by one float (5 in), GUARD sentinels after its end."""

    def __init__(self, gpu, data, misaligned: bool = False):
        import torch

        data = np.asarray(data, F32).ravel()
        self.n, self.lead = data.size, 5 if misaligned else 4
        host = np.full(self.lead + self.n + GUARD, SENTINEL, F32)
        host[self.lead:self.lead + self.n] = data
        self.buf = torch.from_numpy(host).to(gpu)
        self.ptr = self.buf.data_ptr() + 4 * self.lead
        assert (self.ptr % 16 != 0) == misaligned

    def read(self, what: str = "") -> np.ndarray:
        """The array, after checking that the floats around it are untouched."""
        host = self.buf.cpu().numpy()
        around = np.concatenate([host[:self.lead], host[self.lead + self.n:]])
        same_bits(around, np.full(around.size, SENTINEL, F32), f"{what}: the floats around the tensor")
        return host[self.lead:self.lead + self.n].copy()


def adam_tensors(slabs):
    """lgcn_adam_tensor_t[] over (P, G, M, V) slab tuples (G alone for the norm; None: no grad)."""
    from lgcn_amd import _ffi

    arr = (_ffi.AdamTensor * len(slabs))()
    for k, s in enumerate(slabs):
        if not isinstance(s, tuple):
            arr[k] = _ffi.AdamTensor(None, None if s is None else s.ptr, None, None, 0 if s is None else s.n)
        else:
            arr[k] = _ffi.AdamTensor(s[0].ptr, s[1].ptr, s[2].ptr, s[3].ptr, s[0].n)
    return arr


def grad_norm(gpu, slabs, max_norm: float) -> np.ndarray:
    """lgcn_grad_norm over gradient slabs -> float32 [norm, coef]; the workspace is NaN-filled."""
    import torch

    from lgcn_amd import _ffi

    lib = _ffi.load()
    ws = torch.full((lib.lgcn_grad_norm_workspace_floats(),), float("nan"), dtype=torch.float32, device=gpu)
    out = torch.full((2,), float("nan"), dtype=torch.float32, device=gpu)
    _ffi.check(lib.lgcn_grad_norm(adam_tensors(slabs), len(slabs), float(max_norm), ws.data_ptr(), out.data_ptr(),
                                  _ffi.stream_of(gpu)), "lgcn_grad_norm")
    return out.cpu().numpy()


def adam_step(gpu, slabs, hyp, step_size, bc2_sqrt, clip=None, dev_scalars=None, write_grad: int = 1) -> None:
    """lgcn_adam_step on (P, G, M, V) slab tuples; clip / dev_scalars: device tensors or None."""
    from lgcn_amd import _ffi

    omb1, beta2, omb2, eps = hyp
    _ffi.check(_ffi.load().lgcn_adam_step(adam_tensors(slabs), len(slabs), float(omb1), float(beta2), float(omb2),
                                          float(eps), float(step_size), float(bc2_sqrt), _ffi.ptr(clip),
                                          _ffi.ptr(dev_scalars), int(write_grad), _ffi.stream_of(gpu)),
               "lgcn_adam_step")


class RowTables:
    """The two-table state of the row kernels on the device, [N, d] tensors split at U: parameters,
    gradients, both moments, last, claim, the device step and the constants' table."""

    def __init__(self, gpu, U: int, I: int, d: int, p, g, m, v, *, last, step: int, betas=BETAS, eps=ADAM_EPS,
                 lr: float = LR, max_t: int = 512):
        import torch

        from lgcn_amd import _ffi

        self.ffi, self.lib, self.gpu, self.torch = _ffi, _ffi.load(), gpu, torch
        self.U, self.I, self.N, self.d = U, I, U + I, d
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(gpu)
        self.p, self.g, self.m, self.v = (None if a is None else up(a, F32) for a in (p, g, m, v))
        self.last = up(last, np.int32)
        self.claim = torch.full((self.N,), -1, dtype=torch.int32, device=gpu)
        self.step = torch.tensor([step], dtype=torch.int64, device=gpu)
        self.betas, self.eps, self.lr = betas, eps, lr
        self.consts = torch.zeros((max_t + 2, 4), dtype=torch.float32, device=gpu)
        self.stream = _ffi.stream_of(gpu)
        _ffi.check(self.lib.lgcn_adam_consts(self.consts.data_ptr(), 1, max_t + 1, lr, float(betas[0]),
                                             float(betas[1]), self.stream), "lgcn_adam_consts")

    def _halves(self, t):
        if t is None:
            return None, None
        return t.data_ptr(), t.data_ptr() + 4 * self.U * self.d  # rows U.. of the same allocation

    def row_adam(self, mode: int, rows_a=None, keys_b=None, off_b: int = 0, first_b=None, skip_b=None,
                 n_rows: int = 0, clip=None) -> None:
        ptr = self.ffi.ptr
        omb1, beta2, omb2, eps = hyper(self.betas, self.eps)
        with_grad = mode in (1, 3)
        self.ffi.check(self.lib.lgcn_row_adam(
            *self._halves(self.p), *self._halves(self.g if with_grad else None), *self._halves(self.m),
            *self._halves(self.v), self.U, self.d, ptr(rows_a), 0 if rows_a is None else rows_a.numel(), ptr(keys_b),
            0 if keys_b is None else keys_b.numel(), off_b, ptr(first_b), ptr(skip_b), n_rows, self.last.data_ptr(),
            self.claim.data_ptr(), self.step.data_ptr(), self.consts.data_ptr(), float(omb1), float(beta2),
            float(omb2), float(eps), ptr(clip), mode, self.stream), f"lgcn_row_adam mode {mode}")

    def norm_args(self, rows_a, keys_b, off_b, first_b, skip_b):
        ptr = self.ffi.ptr
        return (*self._halves(self.g), self.U, self.d, ptr(rows_a), 0 if rows_a is None else rows_a.numel(),
                ptr(keys_b), 0 if keys_b is None else keys_b.numel(), off_b, ptr(first_b), ptr(skip_b))

    def state(self):
        """(p, m, v, last) as numpy."""
        return tuple(t.cpu().numpy() for t in (self.p, self.m, self.v, self.last))
