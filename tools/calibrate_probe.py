"""Probe: calibrated serving for every user at C2 shape (162,541 users x 59,047 items, d = 64): a
relevance pool of 100 per user, seen items excluded, re-ranked to k = 10 at calibration 0.5 towards
the genre mix of the user's own history. Genre words are synthetic: 18 genres, 0 to 3 per item with
probabilities .05 / .35 / .4 / .2 (the distribution the tests use).

python tools/calibrate_probe.py [--reps 5] [--scale 1.0] [--pool 100] [--k 10] [--calibration 0.5] [--out FILE]

Timings, each the median of --reps after a warm-up with its fastest and slowest run, the arms
alternating in one process, host clock around a device synchronise:
  top10          lgcn_amd.recommend.topk_rows(k = 10) for all users: the unfiltered list, as a check
                 that nothing existing moved (compare with the parent commit in the same session)
  topk           lgcn_amd.recommend.topk_rows(k = pool) alone
  calibrated     lgcn_amd.recommend.topk_rows_calibrated end to end (profile, pool, re-rank)
  profile        lgcn_amd.recommend.attr_profile over every user's seen row, against
  torch_profile  a torch formulation on the same device: per block of 2 M entries index_select of the
                 words, the [E, 32] item distributions, index_add_ into [U, 32], then the division
  rerank         the re-rank stage alone on the same pools, lgcn_amd.recommend.rerank_calibrated, against
  torch_rerank   the batched torch formulation on the same device and pools: per block of 8,192 users
                 the [B, N, 32] item distributions, then k steps of candidate distributions, the
                 [B, N, 32] log, values, masked argmax, state update
The last line is one JSON record: the medians and ranges, the ratios torch / kernel, the share of
slots on which the two re-rank arms picked the same item, the largest difference between the two
profiles, and the mean C_KL@k of the relevance lists and of the re-ranked ones. The kernels' own
times come from a kernel trace in a run of its own
(rocprofv3 --kernel-trace --stats -- python tools/calibrate_probe.py --reps 1).
"""
import torch

import _probe

TORCH_BLOCK = 8192        # users per block of the torch re-rank: a 105 MB [B, N, 32] at pool 100
PROFILE_BLOCK = 1 << 21   # history entries per block of the torch profile: a 268 MB [E, 32]
GENRES = 18


def genre_words(items: int, seed: int, device) -> torch.Tensor:
    """int32 [items]: 0 to 3 distinct genres of GENRES per item with probabilities .05 / .35 / .4 / .2."""
    gen = torch.Generator().manual_seed(seed)
    count = torch.multinomial(torch.tensor([.05, .35, .4, .2]), items, replacement=True, generator=gen)
    order = torch.argsort(torch.rand(items, GENRES, generator=gen), 1)  # a random permutation per item
    chosen = torch.arange(GENRES)[None, :] < count[:, None]              # its first ``count`` genres
    words = (chosen.to(torch.int64) << order).sum(1)
    return words.to(torch.int32).to(device)


def item_dists(words: torch.Tensor) -> torch.Tensor:
    """f32 [..., 32]: uniform over the set bits of each word, zeros for a zero word."""
    bits = ((words.to(torch.int64)[..., None] >> torch.arange(32, device=words.device)) & 1).to(torch.float32)
    return bits / bits.sum(-1, keepdim=True).clamp(min=1.0)


def torch_profile(ptr, idx, attrs, users):
    """The target distributions [U, 32] in torch ops (unit weights, every index in range)."""
    rows = torch.repeat_interleave(torch.arange(users, device=idx.device), ptr[1:] - ptr[:-1])
    out = torch.zeros((users, 32), dtype=torch.float32, device=idx.device)
    weight = torch.zeros(users, dtype=torch.float32, device=idx.device)
    for e0 in range(0, idx.numel(), PROFILE_BLOCK):
        words = attrs.index_select(0, idx[e0:e0 + PROFILE_BLOCK].to(torch.int64))
        r = rows[e0:e0 + PROFILE_BLOCK]
        out.index_add_(0, r, item_dists(words))
        weight.index_add_(0, r, (words != 0).to(torch.float32))
    return out / weight.clamp(min=1.0)[:, None]


def torch_calibrated(pool_idx, pool_score, attrs, target, k, lam, alpha):
    """Greedy calibrated re-ranking in batched torch ops: (idx [Q, k], kl [Q, k]). Pools are full."""
    out_i, out_k = [], []
    for q0 in range(0, pool_idx.shape[0], TORCH_BLOCK):
        pi, r, p = pool_idx[q0:q0 + TORCH_BLOCK], pool_score[q0:q0 + TORCH_BLOCK], target[q0:q0 + TORCH_BLOCK]
        words = attrs[pi]                               # [B, N]
        dist = item_dists(words)                        # [B, N, 32]
        has = (words != 0).to(torch.float32)
        B, N = pi.shape
        pos = (p > 0)[:, None, :]
        plogp = torch.where(p > 0, p * torch.log(p.clamp(min=1e-38)), torch.zeros_like(p)).sum(1)  # [B]
        mass = torch.zeros_like(p)
        m = torch.zeros(B, device=p.device)
        taken = torch.zeros_like(r, dtype=torch.bool)
        ar = torch.arange(B, device=r.device)
        picks, kls = [], []
        for _ in range(k):
            q = (mass[:, None, :] + dist) / (m[:, None] + has).clamp(min=1.0)[..., None]
            qt = (1.0 - alpha) * q + alpha * p[:, None, :]
            cross = torch.where(pos, p[:, None, :] * torch.log(qt), torch.zeros((), device=p.device)).sum(2)
            kl = plogp[:, None] - cross                 # [B, N]
            v = ((1.0 - lam) * r - lam * kl).masked_fill(taken, float("-inf"))
            w = torch.argmax(v, dim=1)
            picks.append(pi[ar, w])
            kls.append(kl[ar, w])
            taken[ar, w] = True
            mass = mass + dist[ar, w]
            m = m + has[ar, w]
        out_i.append(torch.stack(picks, 1))
        out_k.append(torch.stack(kls, 1))
    return torch.cat(out_i), torch.cat(out_k)


def main():
    ap = _probe.parser(reps=5)
    ap.add_argument("--pool", type=int, default=100)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--calibration", type=float, default=0.5)
    ap.add_argument("--alpha", type=float, default=0.01)
    args = ap.parse_args()
    dev = _probe.device("calibrate_probe")
    from lgcn_amd import recommend, synth

    g = synth.ml25m_shaped(seed=0, scale=args.scale)
    U, I = g.num_users, g.num_items
    seen = recommend.seen_csr(torch.from_numpy(g.edge_index).to(dev), U, I, by="user")
    gen = torch.Generator(device=dev).manual_seed(0)
    user_emb = torch.randn(U, args.dim, device=dev, generator=gen)
    item_emb = torch.randn(I, args.dim, device=dev, generator=gen)
    attrs = genre_words(I, 0, dev)
    users = torch.arange(U, device=dev)
    excl = (seen[0], seen[1], users)
    k, N, lam, alpha = args.k, args.pool, args.calibration, args.alpha
    pool_idx, pool_score = recommend.topk_rows(user_emb, users, item_emb, N, excl=excl, index_dtype=torch.int32)
    pool_idx64 = pool_idx.to(torch.int64)
    target = recommend.attr_profile(seen, attrs)[0]
    arms = {"top10": lambda: recommend.topk_rows(user_emb, users, item_emb, 10, excl=excl, index_dtype=torch.int32),
            "topk": lambda: recommend.topk_rows(user_emb, users, item_emb, N, excl=excl, index_dtype=torch.int32),
            "calibrated": lambda: recommend.topk_rows_calibrated(user_emb, users, item_emb, k, lam, attrs=attrs,
                                                                 history=seen, pool=N, excl=excl, alpha=alpha,
                                                                 index_dtype=torch.int32),
            "profile": lambda: recommend.attr_profile(seen, attrs),
            "torch_profile": lambda: torch_profile(seen[0], seen[1], attrs, U),
            "rerank": lambda: recommend.rerank_calibrated(pool_idx, pool_score, attrs, target, k, lam, alpha),
            "torch_rerank": lambda: torch_calibrated(pool_idx64, pool_score, attrs, target, k, lam, alpha)}
    results, times = _probe.run_arms(arms, args.reps, 2)
    rec = dict(users=U, items=I, dim=args.dim, pool=N, k=k, calibration=lam, alpha=alpha, genres=GENRES,
               seen_entries=int(seen[1].numel()), longest_history=int((seen[0][1:] - seen[0][:-1]).max()), reps=args.reps)
    _probe.put_times(rec, times, 2, spread=True)
    rec["torch_over_rerank"] = round(rec["torch_rerank_ms"] / rec["rerank_ms"], 3)
    rec["torch_over_profile"] = round(rec["torch_profile_ms"] / rec["profile_ms"], 3)
    rec["calibrated_over_topk"] = round(rec["calibrated_ms"] / rec["topk_ms"], 3)
    ours, (t_idx, t_kl) = results["rerank"], results["torch_rerank"]
    rec["same_pick_share"] = round(float((ours.idx.to(torch.int64) == t_idx).float().mean()), 6)
    rec["calibrated_equals_rerank"] = bool(torch.equal(results["calibrated"].idx, ours.idx))
    rec["profile_max_abs_diff"] = float((results["profile"][0] - results["torch_profile"]).abs().max())
    relevance = recommend.rerank_calibrated(pool_idx, pool_score, attrs, target, k, 0.0, alpha)
    has = results["profile"][1] > 0
    mean = lambda kl, n: round(float(recommend.miscalibration(kl, n, [k])[has].mean()), 6)
    rec["users_with_target"] = int(has.sum())
    rec[f"ckl@{k}_relevance"] = mean(relevance.kl, relevance.n)
    rec[f"ckl@{k}_reranked"] = mean(ours.kl, ours.n)
    rec[f"ckl@{k}_torch"] = mean(t_kl, torch.full((t_kl.shape[0],), k, device=dev))
    _probe.emit(rec, args.out)


if __name__ == "__main__":
    main()
