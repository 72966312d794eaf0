"""Probe: the device negative sampler (lgcn_amd.negatives) at C3 shape — the ML-25M-shaped graph's
train split (162,541 users, 59,047 items), its 1024-part / 32-parts-per-batch Cluster-GCN batches
(about 10k triplets each), K = 3, d = 128 — and at the planted graph's batch size (180,000 triplets).

python tools/negatives_probe.py [--reps 5] [--scale 1.0] [--dim 128] [--batches 8] [--out FILE]

Timings, each the median of --reps after a warm-up (all repetitions printed and kept, the range
reported), the arms alternating in one process, host clock around a device synchronise:
  draw    for B = one C3 batch's triplets and B = 180,000 (the users of that many random train
          edges), n = 1, 4, 8: sample_negatives against a torch formulation on the same device and
          users —
            n = 1: torch.randint, membership by searchsorted over the seen CSR's (user, item) keys,
                   redraw of the hits until none is left (one host read per round);
            n > 1: torch.randint [B, n] (nothing excluded: the cheaper task), the [B, n, d] gather
                   of the candidate rows, bmm with the user rows, the two norms, argmax.
  step    the C3 step (FusedTrainStep, row-lazy Adam, captured, over the first --batches batches)
          with the default sampler (torch.randint, today's step), and with a NegativeSampler at
          n = 1, 4 and 8 (model=), in the same run.
Quality: the share of the default sampler's draws that are items the user has a train edge to, over
every train triplet once (C2-shaped data) and over the heaviest 1 % of users' triplets.
The last line is one JSON record.
"""
import numpy as np
import torch

import _probe


def torch_uniform_unseen(users, keys, I):
    """n = 1 in torch ops: draw, test membership, redraw the hits. Returns (negatives, rounds)."""
    neg = torch.randint(0, I, (users.numel(),), device=users.device)
    rounds = 0
    while True:
        rounds += 1
        q = users * I + neg
        at = torch.searchsorted(keys, q).clamp_(max=keys.numel() - 1)
        hit = keys[at] == q
        n_hit = int(hit.sum().item())
        if n_hit == 0 or rounds >= 64:
            return neg, rounds
        neg[hit] = torch.randint(0, I, (n_hit,), device=users.device)


def torch_hardest(users, uw, iw, n):
    """n > 1 in torch ops (no exclusion): gather, bmm, norms, argmax."""
    cand = torch.randint(0, iw.shape[0], (users.numel(), n), device=users.device)
    u = uw[users]
    c = iw[cand]
    s = torch.bmm(c, u.unsqueeze(2)).squeeze(2) / (c.norm(dim=2) * u.norm(dim=1, keepdim=True))
    return cand.gather(1, s.argmax(1, keepdim=True)).squeeze(1)


def seen_share(users, neg, keys, I):
    q = users * I + neg
    at = torch.searchsorted(keys, q).clamp_(max=keys.numel() - 1)
    return float((keys[at] == q).float().mean().item())


def main():
    ap = _probe.parser(reps=5)
    ap.set_defaults(dim=128)
    ap.add_argument("--batches", type=int, default=8, help="C3 batches each step arm cycles over")
    ap.add_argument("--big", type=int, default=180000, help="the planted graph's batch size")
    args = ap.parse_args()
    dev = _probe.device("negatives_probe")
    from lgcn_amd import cluster, recommend, synth
    from lgcn_amd.negatives import NegativeSampler, sample_negatives
    from lgcn_amd.optim import RowLazyAdam
    from lgcn_amd.train_step import FusedTrainStep
    from models.light_gcn import LightGCN

    g = synth.ml25m_shaped(seed=0, scale=args.scale)
    U, I, N = g.num_users, g.num_items, g.num_nodes
    train_np = synth.train_split(g.edge_index, 0.9, seed=0)
    _, _, lists = cluster.cluster_batches(train_np, N, 1024, 32)
    lists = lists[:args.batches]
    train_ei = torch.from_numpy(train_np).to(dev)
    seen = recommend.seen_csr(train_ei, U, I, by="user")
    ptr, sidx = seen
    length = ptr[1:] - ptr[:-1]
    keys = torch.repeat_interleave(torch.arange(U, device=dev), length) * I + sidx.to(torch.int64)
    d, K = args.dim, 3
    gen = torch.Generator(device=dev).manual_seed(0)
    uw = 0.1 * torch.randn(U, d, device=dev, generator=gen)
    iw = 0.1 * torch.randn(I, d, device=dev, generator=gen)
    rec = dict(users=U, items=I, dim=d, layers=K, train_pairs=int(sidx.numel()), mean_row=round(float(length.float().mean()), 2),
               longest_row=int(length.max()), reps=args.reps)

    # --- quality of the default draw: every train triplet once --------------------------------------
    all_users = train_ei[0][train_ei[0] < U]
    torch.manual_seed(0)
    rec["default_seen_share_all_triplets"] = seen_share(all_users, torch.randint(0, I, (all_users.numel(),), device=dev),
                                                        keys, I)
    cut = torch.quantile(length.float(), 0.99).item()
    heavy = all_users[length[all_users] >= cut]
    rec["default_seen_share_heaviest_1pct_users"] = seen_share(heavy, torch.randint(0, I, (heavy.numel(),), device=dev),
                                                               keys, I)
    rec["triplets_of_heaviest_1pct_users_share"] = round(heavy.numel() / all_users.numel(), 4)

    # --- draw time ----------------------------------------------------------------------------------
    first = torch.from_numpy(lists[0]).to(dev)
    pick = torch.randperm(all_users.numel(), device=dev, generator=gen)[:args.big]
    for label, users in (("c3", first[0][first[0] < U].contiguous()), ("big", all_users[pick].contiguous())):
        B = users.numel()
        rec[f"{label}_triplets"] = B
        step = [0]

        def ours(n):
            def fn():
                step[0] += 1
                return sample_negatives(users, seen, I, seed=1, step=step[0], candidates=n,
                                        tables=(uw, iw) if n > 1 else None)
            return fn

        arms = {"hip_n1": ours(1), "torch_n1": lambda: torch_uniform_unseen(users, keys, I)[0]}
        for n in (4, 8):
            arms[f"hip_n{n}"] = ours(n)
            arms[f"torch_n{n}"] = (lambda n: lambda: torch_hardest(users, uw, iw, n))(n)
        results, times = _probe.run_arms(arms, args.reps, 4, inner=20, label=f"{label} ")
        _probe.put_times(rec, {f"{label}_{k}": v for k, v in times.items()}, 4, spread=True)
        for n in (1, 4, 8):
            rec[f"{label}_torch_over_hip_n{n}"] = round(rec[f"{label}_torch_n{n}_ms"] / rec[f"{label}_hip_n{n}_ms"], 2)
        rec[f"{label}_torch_n1_rounds"] = torch_uniform_unseen(users, keys, I)[1]
        rec[f"{label}_hip_seen_share"] = max(seen_share(users, results[f"hip_n{n}"], keys, I) for n in (1, 4, 8))
        rec[f"{label}_default_seen_share"] = seen_share(users, torch.randint(0, I, (B,), device=dev), keys, I)

    # --- step cost ----------------------------------------------------------------------------------
    class Batch:
        def __init__(self, ei):
            self.edge_index = ei

    batches = [Batch(torch.from_numpy(x).to(dev)) for x in lists]
    rec["step_batches"] = len(batches)
    rec["step_mean_triplets"] = float(np.mean([int((x[0] < U).sum()) for x in lists]))
    arms, samplers = {}, {}
    for name, n in (("default", 0), ("n1", 1), ("n4", 4), ("n8", 8)):
        torch.manual_seed(0)
        m = LightGCN(U, I, num_layers=K, dim_h=d).to(dev)
        opt = RowLazyAdam(m.user_embedding.weight.data, m.item_embedding.weight.data, lr=1e-3, max_grad_norm=1)
        if n:
            samplers[name] = NegativeSampler(train_ei, U, I, candidates=n, seed=3, model=m if n > 1 else None)
        fused = FusedTrainStep(m, opt, graphs=True, lazy=True, neg_sampler=samplers.get(name))

        def epoch(fused=fused):
            for b in batches:
                fused.step(b)
            fused.sync()

        epoch()  # every batch's plan and captured graph
        arms[f"step_{name}"] = epoch
    _, times = _probe.run_arms(arms, args.reps, 3, inner=4)
    per_step = {k: [t / len(batches) for t in v] for k, v in times.items()}
    _probe.put_times(rec, per_step, 4, spread=True)
    for name in ("n1", "n4", "n8"):
        rec[f"step_{name}_over_default"] = round(rec[f"step_{name}_ms"] / rec["step_default_ms"], 4)
        rec[f"step_{name}_stats"] = samplers[name].stats()
    _probe.emit(rec, args.out)


if __name__ == "__main__":
    main()
