"""ORACLE — test infrastructure, not product code (numpy only).

The contract of the clip-norm and Adam kernels (csrc/lgcn_optim.hip, csrc/lgcn_rowadam.hip) in
float64: torch.nn.utils.clip_grad_norm_(max_norm) followed by torch.optim.Adam's default update
(no weight decay, no amsgrad), per element

  g' = g * coef                        coef = min(max_norm / (||g||_2 + 1e-6), 1)
  m' = m + (1 - beta1) (g' - m)
  v' = beta2 v + (1 - beta2) g'^2
  p' = p + step_size * m' / (sqrt(v') / bc2_sqrt + eps)
       step_size = -lr / (1 - beta1^t),  bc2_sqrt = sqrt(1 - beta2^t)

adam_step_ref takes the step's constants as given (float32 values, the kernels' inputs: whether
they are the right constants for step t is lgcn_adam_prologue's / lgcn_adam_consts' business);
adam_trajectory_ref is the whole optimizer from t = 1 with double hyper-parameters.
"""
from __future__ import annotations

import dataclasses

import numpy as np

CLIP_EPS = 1e-6  # clip_grad_norm_'s


def clip_ref(grads, max_norm):
    """(norm, coef) of the gradients taken together (None entries: no gradient), float64."""
    sq = 0.0
    for g in grads:
        if g is not None:
            g = np.asarray(g, np.float64)
            sq += float(np.sum(g * g))
    norm = float(np.sqrt(sq))
    return norm, min(float(max_norm) / (norm + CLIP_EPS), 1.0)


@dataclasses.dataclass
class AdamStep:
    """One element-wise step, everything float64 and of the inputs' shape."""
    p: np.ndarray
    g: np.ndarray      # the clipped gradient g * coef
    m: np.ndarray
    v: np.ndarray
    denom: np.ndarray  # sqrt(v') / bc2_sqrt + eps
    upd: np.ndarray    # step_size * m' / denom


def adam_step_ref(p, g, m, v, coef, step_size, bc2_sqrt, omb1, beta2, omb2, eps) -> AdamStep:
    """One step in float64 from the given state and constants (each converted to float64 as it
    stands: float32 inputs are taken at their float32 values)."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    coef, step_size, bc2_sqrt, omb1, beta2, omb2, eps = (float(x) for x in (coef, step_size, bc2_sqrt, omb1, beta2,
                                                                            omb2, eps))
    g1 = g * coef
    m1 = m + omb1 * (g1 - m)
    v1 = v * beta2 + omb2 * (g1 * g1)
    denom = np.sqrt(v1) / bc2_sqrt + eps
    upd = step_size * (m1 / denom)
    return AdamStep(p + upd, g1, m1, v1, denom, upd)


def adam_trajectory_ref(w0, grads, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_norm=None):
    """Plain Adam in float64. w0: the parameter arrays; grads[t - 1][k]: parameter k's gradient at
    step t = 1..T (None: it has none at that step and neither moves nor counts in the norm; a
    parameter's own step count then lags, as torch's does). Returns (w, m, v, norms): the arrays
    after T steps and the T pre-clip norms (None without max_norm)."""
    beta1, beta2 = (float(b) for b in betas)
    w = [np.array(x, np.float64) for x in w0]
    m = [np.zeros_like(x) for x in w]
    v = [np.zeros_like(x) for x in w]
    steps = [0] * len(w)
    norms = []
    for gs in grads:
        assert len(gs) == len(w)
        coef = 1.0
        if max_norm is not None:
            norm, coef = clip_ref(gs, max_norm)
            norms.append(norm)
        for k, g in enumerate(gs):
            if g is None:
                continue
            steps[k] += 1
            t = steps[k]
            g = np.asarray(g, np.float64) * coef
            m[k] = m[k] + (1.0 - beta1) * (g - m[k])
            v[k] = beta2 * v[k] + (1.0 - beta2) * (g * g)
            bc1 = 1.0 - beta1 ** t
            bc2 = 1.0 - beta2 ** t
            w[k] = w[k] - (lr / bc1) * (m[k] / (np.sqrt(v[k]) / np.sqrt(bc2) + eps))
    return w, m, v, (norms if max_norm is not None else None)
