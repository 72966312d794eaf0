"""Probe: top-k recommendation for every user at C2 shape (162,541 users x 59,047 items, d = 64,
k = 10), each user's exclusion row drawn from the ML-25M-shaped synthetic graph.

python tools/recommend_probe.py [--reps 3] [--scale 1.0] [--only ours|torch] [--out FILE]

Times lgcn_amd.recommend.topk_items over all users against the batched torch formulation on the
same device and inputs, in query blocks: normalise, torch.mm, index_put_ of -inf on the seen
entries, torch.topk. Both are timed end to end (host clock around a device synchronise, the
exclusion CSR built beforehand for both), alternating, after a warm-up of each; the last line is
one JSON record (ms per 1,000 users of each, their ratio, and how many of the two index lists
agree). The split between the score filter and the ranked selection comes from a kernel trace of
`--only ours` in a run of its own (rocprofv3 --kernel-trace --stats -- python tools/...).
"""
import torch

import _probe

TORCH_BLOCK = 8192  # users per torch.mm block: a 1.9 GB score block at 59,047 items


def torch_topk(user_emb, item_emb, users, k, seen):
    ptr, idx = seen
    cn = item_emb / torch.norm(item_emb, dim=1, keepdim=True)
    out_i, out_s = [], []
    for q0 in range(0, users.numel(), TORCH_BLOCK):
        u = users[q0:q0 + TORCH_BLOCK]
        q = user_emb[u]
        scores = torch.mm(q / torch.norm(q, dim=1, keepdim=True), cn.t())
        beg, cnt = ptr[u], ptr[u + 1] - ptr[u]
        rows = torch.repeat_interleave(torch.arange(u.numel(), device=u.device), cnt)
        offs = torch.arange(rows.numel(), device=u.device) - torch.repeat_interleave(torch.cumsum(cnt, 0) - cnt, cnt)
        cols = idx[torch.repeat_interleave(beg, cnt) + offs].long()
        scores.index_put_((rows, cols), torch.tensor(float("-inf"), device=u.device))
        s, i = torch.topk(scores, k, dim=1)
        out_i.append(i)
        out_s.append(s)
    return torch.cat(out_i), torch.cat(out_s)


def main():
    ap = _probe.parser(reps=3)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--only", choices=["ours", "torch"], default=None)
    args = ap.parse_args()
    dev = _probe.device("recommend_probe")
    from lgcn_amd import recommend, synth

    g = synth.ml25m_shaped(seed=0, scale=args.scale)
    U, I = g.num_users, g.num_items
    seen = recommend.seen_csr(torch.from_numpy(g.edge_index).to(dev), U, I, by="user")
    gen = torch.Generator(device=dev).manual_seed(0)
    user_emb = torch.randn(U, args.dim, device=dev, generator=gen)
    item_emb = torch.randn(I, args.dim, device=dev, generator=gen)
    users = torch.arange(U, device=dev)
    arms = {"ours": lambda: recommend.topk_items(user_emb, item_emb, users, args.k, seen=seen),
            "torch": lambda: torch_topk(user_emb, item_emb, users, args.k, seen)}
    if args.only:
        arms = {args.only: arms[args.only]}
    results, times = _probe.run_arms(arms, args.reps, 1)
    rec = dict(users=U, items=I, dim=args.dim, k=args.k, seen_entries=int(seen[1].numel()), reps=args.reps)
    for name, ts in times.items():
        rec[f"{name}_ms_per_1000_users"] = round(_probe.median(ts) / U * 1000, 4)
        rec[f"{name}_ms_all"] = [round(t, 1) for t in ts]
    if len(arms) == 2:
        rec["torch_over_ours"] = round(rec["torch_ms_per_1000_users"] / rec["ours_ms_per_1000_users"], 3)
        rec["same_index_share"] = round(float((results["ours"][0] == results["torch"][0]).float().mean()), 6)
        diff = (results["ours"][1] - results["torch"][1]).abs()
        rec["max_score_diff"] = float(diff[torch.isfinite(diff)].max())
    _probe.emit(rec, args.out)


if __name__ == "__main__":
    main()
