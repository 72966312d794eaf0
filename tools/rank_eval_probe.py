"""Probe: full-ranking evaluation of every user at C2 shape (162,541 users x 59,047 items, d = 64,
cutoffs 5 / 10 / 20), five items per user held out of the ML-25M-shaped synthetic graph and the
rest (about 77 per user) excluded as seen.

python tools/rank_eval_probe.py [--reps 5] [--scale 1.0] [--out FILE]

Times two things, host clock around a device synchronise, after a warm-up of each:
  * the whole lgcn_amd.metrics.evaluate_ranking (ranking, counts, means, its one host read);
  * the metric stage alone — lgcn_amd.metrics.rank_metrics (one lgcn_rank_metrics launch) against a
    torch formulation on the same device and the same ranked lists: composite keys row * M + idx
    for the lists and the truth CSR, torch.searchsorted into the sorted truth keys, cumulative sums
    read at each cutoff. The two alternate, `--inner` calls per timing.
The last line is one JSON record (the medians, the ratio, whether the two agree, the metrics).
(tools/eval_probe.py is the older probe of the reference-style evaluate().)
"""
import torch

import _probe

KS = (5, 10, 20)
HELD_OUT = 5


def split_edges(ptr, idx, U, gen):
    """(train, held-out) edge lists of a user CSR: HELD_OUT random entries of every row that has
    more than HELD_OUT, global numbering (items at U + i)."""
    deg = ptr[1:] - ptr[:-1]
    row = torch.repeat_interleave(torch.arange(U, device=ptr.device), deg)
    order = torch.argsort(row.double() + torch.rand(row.numel(), device=ptr.device, generator=gen, dtype=torch.float64))
    rank = torch.arange(row.numel(), device=ptr.device) - ptr[row]  # row is sorted: position within the row
    held = torch.zeros(row.numel(), dtype=torch.bool, device=ptr.device)
    held[order] = (rank < HELD_OUT) & (deg[row] > HELD_OUT)
    edges = torch.stack([row, idx.long() + U])
    return edges[:, ~held], edges[:, held]


def torch_counts(ranked, truth, rows, cs, M):
    """rank_metrics' outputs by torch ops: [Q * k] int64 keys, searchsorted, cumulative sums."""
    ptr, idx = truth
    R, (Q, k) = ptr.numel() - 1, ranked.shape
    dev = ranked.device
    deg = ptr[1:] - ptr[:-1]
    tkeys = torch.repeat_interleave(torch.arange(R, device=dev), deg) * M + idx.long()  # sorted: rows, then idx
    keys = (rows[:, None] * M + ranked.long()).view(-1)
    pos = torch.searchsorted(tkeys, keys).clamp(max=tkeys.numel() - 1)
    hit = ((tkeys[pos] == keys) & (ranked.view(-1) >= 0)).view(Q, k)
    disc = 1.0 / torch.log2(torch.arange(2, k + 2, device=dev, dtype=torch.float64))
    at = torch.tensor(cs, device=dev) - 1
    hits = hit.cumsum(1, dtype=torch.int32)[:, at]
    dcg = (hit * disc).cumsum(1)[:, at].float()
    first = torch.where(hit.any(1), hit.int().argmax(1), torch.full((), -1, device=dev)).int()
    return hits, dcg, first, deg[rows].int()


def main():
    ap = _probe.parser(reps=5)
    ap.add_argument("--inner", type=int, default=10)
    args = ap.parse_args()
    dev = _probe.device("rank_eval_probe")
    from lgcn_amd import metrics, recommend, synth

    g = synth.ml25m_shaped(seed=0, scale=args.scale)
    U, I = g.num_users, g.num_items
    gen = torch.Generator(device=dev).manual_seed(0)
    every = recommend.seen_csr(torch.from_numpy(g.edge_index).to(dev), U, I, by="user")
    train, held = split_edges(*every, U, gen)
    seen, truth = recommend.seen_csr(train, U, I), recommend.seen_csr(held, U, I)
    user_emb = torch.randn(U, args.dim, device=dev, generator=gen)
    item_emb = torch.randn(I, args.dim, device=dev, generator=gen)
    users = torch.nonzero(truth[0][1:] > truth[0][:-1]).view(-1)

    whole = {"evaluate_ranking": lambda: metrics.evaluate_ranking(user_emb, item_emb, truth, ks=KS, seen=seen)}
    result, t_whole = (d["evaluate_ranking"] for d in _probe.run_arms(whole, args.reps, 2))

    ranked, _ = recommend.topk_items(user_emb, item_emb, users, KS[-1], seen=seen, index_dtype=torch.int32)
    arms = {"kernel": lambda: metrics.rank_metrics(ranked, truth, KS, rows=users),
            "torch": lambda: torch_counts(ranked, truth, users, KS, I)}
    outs, times = _probe.run_arms(arms, args.reps, 3, inner=args.inner, label="metric stage, ")
    med = _probe.median
    a, b = outs["kernel"], outs["torch"]
    rec = dict(users=U, items=I, dim=args.dim, ks=list(KS), evaluated_users=int(users.numel()),
               seen_entries=int(seen[1].numel()), truth_entries=int(truth[1].numel()), reps=args.reps,
               evaluate_ranking_ms=round(med(t_whole), 2), evaluate_ranking_ms_all=[round(t, 2) for t in t_whole],
               metric_kernel_ms=round(med(times["kernel"]), 4), metric_torch_ms=round(med(times["torch"]), 4),
               metric_kernel_ms_all=[round(t, 4) for t in times["kernel"]],
               metric_torch_ms_all=[round(t, 4) for t in times["torch"]])
    rec["torch_over_kernel"] = round(rec["metric_torch_ms"] / rec["metric_kernel_ms"], 3)
    rec["counts_equal"] = bool(torch.equal(a.hits, b[0]) and torch.equal(a.first, b[2]) and torch.equal(a.n_truth, b[3]))
    rec["max_dcg_diff"] = float((a.dcg - b[1]).abs().max())
    rec["metrics"] = {key: round(v, 6) for key, v in result.items()}
    _probe.emit(rec, args.out)


if __name__ == "__main__":
    main()
