"""Probe: diversity-aware serving for every user at C2 shape (162,541 users x 59,047 items, d = 64):
a relevance pool of 100 per user, seen items excluded, re-ranked by greedy MMR to k = 10 at
diversity 0.5.

python tools/rerank_probe.py [--reps 3] [--scale 1.0] [--pool 100] [--k 10] [--diversity 0.5] [--out FILE]

Three timings, each the median of --reps after a warm-up, the arms alternating in one process, host
clock around a device synchronise:
  topk        lgcn_amd.recommend.topk_rows(k = pool) alone
  diverse     lgcn_amd.recommend.topk_rows_diverse end to end (pool, normalise, re-rank)
  rerank      the re-rank stage alone on the same pools, lgcn_amd.recommend.rerank_mmr, against
  torch       the batched torch formulation on the same device and pools: per block of 8,192 users
              a [B, N, D] gather of unit rows, a torch.bmm Gram [B, N, N], then k steps of values,
              masked argmax, maximum update (both arms normalise the candidates inside the timing)
The last line is one JSON record: the medians, the ratio torch / rerank, the share of slots on which
the two arms picked the same item, and the mean ILD@k of the relevance lists and of the re-ranked
ones. The kernel's own time comes from a kernel trace in a run of its own
(rocprofv3 --kernel-trace --stats -- python tools/rerank_probe.py --reps 1).
"""
import torch

import _probe

TORCH_BLOCK = 8192  # users per block: a 210 MB gather and a 328 MB Gram at pool 100, d = 64


def torch_mmr(pool_idx, pool_score, candidates, k, diversity):
    """Greedy MMR in batched torch ops: (idx [Q, k], pair [Q, k]). Pools are full (no -1 entries)."""
    cn = candidates / torch.norm(candidates, dim=1, keepdim=True)
    keep, out_i, out_p = 1.0 - diversity, [], []
    for q0 in range(0, pool_idx.shape[0], TORCH_BLOCK):
        pi, r = pool_idx[q0:q0 + TORCH_BLOCK], pool_score[q0:q0 + TORCH_BLOCK]
        rows = cn[pi]                                  # [B, N, D]
        gram = torch.bmm(rows, rows.transpose(1, 2))   # [B, N, N]
        B, N = pi.shape
        m = torch.zeros_like(r)
        a = torch.zeros_like(r)
        taken = torch.zeros_like(r, dtype=torch.bool)
        picks, pairs = [], []
        ar = torch.arange(B, device=r.device)
        for t in range(k):
            v = (keep * r - diversity * m).masked_fill(taken, float("-inf"))
            w = torch.argmax(v, dim=1)
            picks.append(pi[ar, w])
            pairs.append(a[ar, w])
            taken[ar, w] = True
            s = gram[ar, w]                            # [B, N]: every position against the pick
            m = s if t == 0 else torch.maximum(m, s)
            a = a + s
        out_i.append(torch.stack(picks, 1))
        out_p.append(torch.stack(pairs, 1))
    return torch.cat(out_i), torch.cat(out_p)


def main():
    ap = _probe.parser(reps=3)
    ap.add_argument("--pool", type=int, default=100)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--diversity", type=float, default=0.5)
    args = ap.parse_args()
    dev = _probe.device("rerank_probe")
    from lgcn_amd import recommend, synth

    g = synth.ml25m_shaped(seed=0, scale=args.scale)
    U, I = g.num_users, g.num_items
    seen = recommend.seen_csr(torch.from_numpy(g.edge_index).to(dev), U, I, by="user")
    gen = torch.Generator(device=dev).manual_seed(0)
    user_emb = torch.randn(U, args.dim, device=dev, generator=gen)
    item_emb = torch.randn(I, args.dim, device=dev, generator=gen)
    users = torch.arange(U, device=dev)
    excl = (seen[0], seen[1], users)
    k, N, delta = args.k, args.pool, args.diversity
    pool_idx, pool_score = recommend.topk_rows(user_emb, users, item_emb, N, excl=excl, index_dtype=torch.int32)
    pool_idx64 = pool_idx.to(torch.int64)
    arms = {"topk": lambda: recommend.topk_rows(user_emb, users, item_emb, N, excl=excl, index_dtype=torch.int32),
            "diverse": lambda: recommend.topk_rows_diverse(user_emb, users, item_emb, k, delta, pool=N, excl=excl,
                                                           index_dtype=torch.int32),
            "rerank": lambda: recommend.rerank_mmr(pool_idx, pool_score, item_emb, k, delta),
            "torch": lambda: torch_mmr(pool_idx64, pool_score, item_emb, k, delta)}
    results, times = _probe.run_arms(arms, args.reps, 1)
    rec = dict(users=U, items=I, dim=args.dim, pool=N, k=k, diversity=delta, seen_entries=int(seen[1].numel()),
               reps=args.reps)
    _probe.put_times(rec, times, 2)
    rec["torch_over_rerank"] = round(rec["torch_ms"] / rec["rerank_ms"], 3)
    ours, (t_idx, t_pair) = results["rerank"], results["torch"]
    rec["same_pick_share"] = round(float((ours.idx.to(torch.int64) == t_idx).float().mean()), 6)
    rec["diverse_equals_rerank"] = bool(torch.equal(results["diverse"].idx, ours.idx))
    ks = [k]
    relevance = recommend.rerank_mmr(pool_idx, pool_score, item_emb, k, 0.0)
    rec[f"ild@{k}_relevance"] = round(float(recommend.intra_list_diversity(relevance.pair, relevance.n, ks).mean()), 6)
    rec[f"ild@{k}_reranked"] = round(float(recommend.intra_list_diversity(ours.pair, ours.n, ks).mean()), 6)
    n_t = torch.full((t_pair.shape[0],), k, device=dev)
    rec[f"ild@{k}_torch"] = round(float(recommend.intra_list_diversity(t_pair, n_t, ks).mean()), 6)
    _probe.emit(rec, args.out)


if __name__ == "__main__":
    main()
