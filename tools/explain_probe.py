"""Probe: "because you watched" explanations for every user at C2 shape (162,541 users x 59,047
items, d = 64): each user's top 10 with seen items excluded, then the 3 history items that point
most strongly at each of the 10.

python tools/explain_probe.py [--reps 5] [--scale 1.0] [--k 10] [--r 3] [--out FILE]

Timings, each the median of --reps after a warm-up (all repetitions are printed and kept), the arms
alternating in one process, host clock around a device synchronise:
  topk        lgcn_amd.recommend.topk_items(k) alone
  served      topk_items then lgcn_amd.explain.explain_items: what turning explanations on costs
  explain     the explain stage alone on the same lists, lgcn_amd.explain.explain_items, against
  torch       the batched torch formulation on the same device and lists: users bucketed by history
              length (powers of two), per bucket and block a padded [B, L, D] gather of unit rows,
              torch.bmm against the [B, D, k] recommended rows, the pad and the item itself masked,
              torch.topk over the history (both arms normalise the items inside the timing; the
              bucketing is built once outside it)
  longest     explain_items for the single user with the longest history: one wave, the floor of
              the explain stage whatever else runs
The last line is one JSON record: the timings, the ratio torch / explain, and the share of
(user, slot, position) entries on which the two arms name the same item. The kernel's own time
comes from a kernel trace in a run of its own
(rocprofv3 --kernel-trace --stats -- python tools/explain_probe.py --reps 1).
"""
import torch

import _probe

TORCH_BLOCK_BYTES = 1 << 30  # the padded gather of one block: B * L * D * 4


def torch_buckets(ptr, users):
    """[(L, users of history length in (L / 2, L])], L a power of two; users without history left out."""
    length = (ptr[1:] - ptr[:-1])[users]
    out, L = [], 1
    top = int(length.max())
    while True:
        pick = (length <= L) & (length > L // 2)
        if pick.any():
            out.append((L, torch.nonzero(pick).view(-1)))
        if L >= top:
            return out
        L <<= 1


def torch_explain(buckets, ptr, idx, users, rec_idx, item_emb, r):
    """The r best history items per slot in batched torch ops: idx [Q, k, r] (-1 unfilled)."""
    cn = item_emb / torch.norm(item_emb, dim=1, keepdim=True)
    Q, k = rec_idx.shape
    D = cn.shape[1]
    out = torch.full((Q, k, r), -1, dtype=torch.int64, device=rec_idx.device)
    for L, who in buckets:
        step = max(1, TORCH_BLOCK_BYTES // (L * D * 4))
        ar = torch.arange(L, device=rec_idx.device)
        for b0 in range(0, who.numel(), step):
            qs = who[b0:b0 + step]
            beg = ptr[users[qs]]
            n = ptr[users[qs] + 1] - beg
            real = ar[None, :] < n[:, None]                                   # [B, L]
            hist = idx[(beg[:, None] + ar[None, :]).clamp(max=idx.numel() - 1)].to(torch.int64)
            hist = torch.where(real, hist, torch.zeros_like(hist))
            rec = rec_idx[qs]                                                 # [B, k]
            c = torch.bmm(cn[hist], cn[rec].transpose(1, 2))                  # [B, L, k]
            dead = ~real[:, :, None] | (hist[:, :, None] == rec[:, None, :])
            c = c.masked_fill(dead, float("-inf"))
            val, pos = torch.topk(c, min(r, L), dim=1)                        # [B, r', k]
            got = torch.gather(hist, 1, pos.reshape(qs.numel(), -1)).view(pos.shape)
            got = torch.where(torch.isneginf(val), torch.full_like(got, -1), got)
            out[qs, :, :got.shape[1]] = got.transpose(1, 2)
    return out


def main():
    ap = _probe.parser(reps=5)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--r", type=int, default=3)
    args = ap.parse_args()
    dev = _probe.device("explain_probe")
    from lgcn_amd import explain, recommend, synth

    g = synth.ml25m_shaped(seed=0, scale=args.scale)
    U, I = g.num_users, g.num_items
    seen = recommend.seen_csr(torch.from_numpy(g.edge_index).to(dev), U, I, by="user")
    ptr, sidx = seen
    gen = torch.Generator(device=dev).manual_seed(0)
    user_emb = torch.randn(U, args.dim, device=dev, generator=gen)
    item_emb = torch.randn(I, args.dim, device=dev, generator=gen)
    users = torch.arange(U, device=dev)
    k, r = args.k, args.r
    rec32, _ = recommend.topk_items(user_emb, item_emb, users, k, seen=seen, index_dtype=torch.int32)
    rec64 = rec32.to(torch.int64)
    length = ptr[1:] - ptr[:-1]
    heavy = torch.argmax(length).view(1)
    buckets = torch_buckets(ptr, users)

    def served():
        idx, _ = recommend.topk_items(user_emb, item_emb, users, k, seen=seen, index_dtype=torch.int32)
        return explain.explain_items(item_emb, users, idx, seen, r=r)

    arms = {"topk": lambda: recommend.topk_items(user_emb, item_emb, users, k, seen=seen, index_dtype=torch.int32),
            "served": served,
            "explain": lambda: explain.explain_items(item_emb, users, rec32, seen, r=r),
            "torch": lambda: torch_explain(buckets, ptr, sidx, users, rec64, item_emb, r),
            "longest": lambda: explain.explain_items(item_emb, heavy, rec32[heavy], seen, r=r)}
    results, times = _probe.run_arms(arms, args.reps, 2)
    rec = dict(users=U, items=I, dim=args.dim, k=k, r=r, seen_entries=int(sidx.numel()),
               longest_history=int(length.max()), mean_history=round(float(length.float().mean()), 2), reps=args.reps)
    _probe.put_times(rec, times, 3)
    rec["torch_over_explain"] = round(rec["torch_ms"] / rec["explain_ms"], 3)
    rec["explain_cost_ms"] = round(rec["served_ms"] - rec["topk_ms"], 3)
    ours, theirs = results["explain"], results["torch"]
    rec["same_item_share"] = round(float((ours.idx.to(torch.int64) == theirs).float().mean()), 6)
    rec["served_equals_explain"] = bool(torch.equal(results["served"].idx, ours.idx))
    rec["filled_share"] = round(float((ours.idx >= 0).float().mean()), 6)
    _probe.emit(rec, args.out)


if __name__ == "__main__":
    main()
