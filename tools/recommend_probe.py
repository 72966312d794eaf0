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
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "movie-recommender-system-with-gnns_amd"))

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
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--only", choices=["ours", "torch"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("recommend_probe needs a ROCm device (a CPU timing says nothing here)")
    from lgcn_amd import recommend, synth

    dev = torch.device("cuda")
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

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t) * 1e3

    results, times = {}, {name: [] for name in arms}
    for name, fn in arms.items():  # warm-up: code objects, allocator pools
        results[name], _ = timed(fn)
    for _ in range(args.reps):
        for name, fn in arms.items():
            _, ms = timed(fn)
            times[name].append(ms)
            print(f"{name}: {ms:.1f} ms", flush=True)
    rec = dict(users=U, items=I, dim=args.dim, k=args.k, seen_entries=int(seen[1].numel()), reps=args.reps)
    for name, ts in times.items():
        rec[f"{name}_ms_per_1000_users"] = round(sorted(ts)[len(ts) // 2] / U * 1000, 4)
        rec[f"{name}_ms_all"] = [round(t, 1) for t in ts]
    if len(arms) == 2:
        rec["torch_over_ours"] = round(rec["torch_ms_per_1000_users"] / rec["ours_ms_per_1000_users"], 3)
        rec["same_index_share"] = round(float((results["ours"][0] == results["torch"][0]).float().mean()), 6)
        diff = (results["ours"][1] - results["torch"][1]).abs()
        rec["max_score_diff"] = float(diff[torch.isfinite(diff)].max())
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
