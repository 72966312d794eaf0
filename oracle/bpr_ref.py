"""ORACLE — test infrastructure, not product code (numpy only).

The per-triplet contract of the fused cosine-BPR kernels (csrc/lgcn_bpr.hip: lgcn_bpr_fused,
lgcn_bpr_fused_cols) in float64: what the six sums, the two loss terms and the gradient rows of
ONE triplet (u, p, n) must be, independent of the scatter, the backward and the optimizer that
consume them.

  loss = -mean_b softplus(z_b) / 10 + coeff * mean_{b,c} (wu^2 + wp^2 + wn^2),
  z_b  = 10 (cos(u_b, p_b) - cos(u_b, n_b))          (utils.train_test.bpr_loss)

with the cosines on the propagated rows F and the squares on the layer-0 rows W. User u is row u
of a table, item i is row U + i. softplus is F.softplus(beta=1, threshold=20): z itself above 20,
and its derivative there is 1.

With a = u/|u|, b = p/|p|, c = n/|n|, cp = a.b, cn = a.c, sg = softplus'(z) and s = sg / B:

  du = s * (-(b - cp a) + (c - cn a)) / |u|
  dp = -s * (a - cp b) / |p|
  dn =  s * (a - cn c) / |n|

Each of these is a difference of terms that nearly cancel when the rows are nearly parallel, so a
float32 evaluation is accurate relative to the terms, not to the result. The "uncancelled scale"
of a row is the size of those terms (max norm over the columns):

  S_u = s * ((max|b| + |cp| max|a|) + (max|c| + |cn| max|a|)) / |u|
  S_p = s * (max|a| + |cp| max|b|) / |p|
  S_n = s * (max|a| + |cn| max|c|) / |n|
"""
from __future__ import annotations

import dataclasses

import numpy as np

SOFTPLUS_THRESHOLD = 20.0


@dataclasses.dataclass
class BprRef:
    """Everything float64; [B] unless stated."""
    suu: np.ndarray
    spp: np.ndarray
    snn: np.ndarray
    sup: np.ndarray
    sun: np.ndarray
    sreg: np.ndarray    # sum of squares of the three layer-0 rows
    abs_up: np.ndarray  # sum_c |u_c p_c|: the scale a float32 dot product is accurate to
    abs_un: np.ndarray
    cp: np.ndarray
    cn: np.ndarray
    z: np.ndarray
    sp: np.ndarray      # softplus(z), threshold 20
    sg: np.ndarray      # its derivative
    du: np.ndarray      # [B, d]
    dp: np.ndarray      # [B, d]
    dn: np.ndarray      # [B, d]
    S_u: np.ndarray
    S_p: np.ndarray
    S_n: np.ndarray
    reg_u: np.ndarray   # [B, d] coeff * 2 / (B * d_full) * W[row]
    reg_p: np.ndarray   # [B, d]
    reg_n: np.ndarray   # [B, d]
    d_full: int

    @property
    def sums(self) -> np.ndarray:
        """[B, 6] in the kernels' order: |u|^2, |p|^2, |n|^2, u.p, u.n, reg squares."""
        return np.stack([self.suu, self.spp, self.snn, self.sup, self.sun, self.sreg], axis=1)

    def loss(self, coeff: float) -> float:
        B = self.sp.shape[0]
        return float(-self.sp.mean() / 10.0 + coeff * self.sreg.sum() / (B * self.d_full))


def effective_F(F, W, touched, div, mul) -> np.ndarray:
    """The propagated table a sparse batch plan stands for: rows with touched[r] == 0 were not
    propagated and are (W[r] / float32(div)) * float32(mul), two correctly rounded float32
    operations (the kernel's own); touched rows are F's. touched None: F itself."""
    F = np.asarray(F, np.float32)
    if touched is None:
        return F
    W = np.asarray(W, np.float32)
    t = np.asarray(touched).astype(bool)
    sub = ((W / np.float32(div)).astype(np.float32) * np.float32(mul)).astype(np.float32)
    return np.where(t[:, None], F, sub).astype(np.float32)


def softplus(z: np.ndarray):
    """(softplus(z), its derivative) as F.softplus(beta=1, threshold=20) defines them."""
    z = np.asarray(z, np.float64)
    over = z > SOFTPLUS_THRESHOLD
    zc = np.where(over, 0.0, z)
    sp = np.where(over, z, np.logaddexp(0.0, zc))
    e = np.exp(-np.abs(zc))  # sigmoid without overflow or cancellation on either side
    sg = np.where(over, 1.0, np.where(zc >= 0, 1.0 / (1.0 + e), e / (1.0 + e)))
    return sp, sg


def bpr_triplet_ref(F, W, U, u, p, n, coeff, d_full=None) -> BprRef:
    """F, W: [N, d] propagated and layer-0 tables; u, p, n: [B] user / item ids (item i is row
    U + i); d_full: the width the reg mean is taken over (d when None; wider when F and W are a
    column share of a wider table)."""
    F = np.asarray(F, np.float64)
    W = np.asarray(W, np.float64)
    u, p, n = (np.asarray(x, np.int64) for x in (u, p, n))
    B, d = u.shape[0], F.shape[1]
    d_full = d if d_full is None else int(d_full)
    ru, rp, rn = u, U + p, U + n
    eu, ep, en = F[ru], F[rp], F[rn]
    wu, wp, wn = W[ru], W[rp], W[rn]
    suu, spp, snn = (eu * eu).sum(1), (ep * ep).sum(1), (en * en).sum(1)
    sup, sun = (eu * ep).sum(1), (eu * en).sum(1)
    sreg = (wu * wu).sum(1) + (wp * wp).sum(1) + (wn * wn).sum(1)
    nu, np_, nn = np.sqrt(suu), np.sqrt(spp), np.sqrt(snn)
    a, b, c = eu / nu[:, None], ep / np_[:, None], en / nn[:, None]
    cp, cn = (a * b).sum(1), (a * c).sum(1)
    z = 10.0 * (cp - cn)
    sp, sg = softplus(z)
    s = sg / B
    col = lambda v: v[:, None]
    du = (-col(s) * (b - col(cp) * a) + col(s) * (c - col(cn) * a)) / col(nu)
    dp = -col(s) * (a - col(cp) * b) / col(np_)
    dn = col(s) * (a - col(cn) * c) / col(nn)
    ma, mb, mc = np.abs(a).max(1), np.abs(b).max(1), np.abs(c).max(1)
    S_u = s * ((mb + np.abs(cp) * ma) + (mc + np.abs(cn) * ma)) / nu
    S_p = s * (ma + np.abs(cp) * mb) / np_
    S_n = s * (ma + np.abs(cn) * mc) / nn
    kreg = coeff * 2.0 / (B * d_full)
    return BprRef(suu=suu, spp=spp, snn=snn, sup=sup, sun=sun, sreg=sreg,
                  abs_up=np.abs(eu * ep).sum(1), abs_un=np.abs(eu * en).sum(1),
                  cp=cp, cn=cn, z=z, sp=sp, sg=sg, du=du, dp=dp, dn=dn, S_u=S_u, S_p=S_p, S_n=S_n,
                  reg_u=kreg * wu, reg_p=kreg * wp, reg_n=kreg * wn, d_full=d_full)
