"""Probe: per-item score boosts at C2 shape (162,541 users x 59,047 items, d = 64): every user's k = 10
best unseen items of the ML-25M-shaped synthetic graph, unboosted and under boosts.

python tools/boost_probe.py [--reps 5] [--scale 1.0] [--dim 64] [--unboosted-only] [--skip-torch] [--out FILE]

Times, host clock around a device synchronise, after a warm-up of each, medians of --reps with the
range, the arms taken in turn, of lgcn_amd.recommend.topk_items:
  (a) unboosted                          today's call
  (b) boost = -0.0 everywhere            the boosted kernels when they change nothing: (b) - (a) is what the
                                         boost costs, reported beside (a)'s own run-to-run range
  (c) popularity_boost(counts, 0.2)      "show less of what everybody has seen"; counts: the items' training
                                         interaction counts
  (d) a genre filter, any = a bit on about 20 % of the items, unboosted
  (e) (c) and (d) together
  (f) among= with 100 candidates per user, unboosted      (g) (f) with the penalty of (c)
(c) also against the batched torch formulation on the same device and unit rows: blocks of 8,192 users,
mm, an add over the [Q, M] block, -inf on the seen pairs, topk; with the share of lists equal to torch's
(mm sums in another order: near-ties may fall the other way). It reports the mean training popularity of
the served top-10 before and after the penalty, and whether (b) returns (a)'s lists bit for bit.
--unboosted-only runs (a), (d) and (f) alone: the arms a tree without boost= has, for a before / after
comparison of the unchanged paths. The last line is one JSON record."""
import torch

import _probe

BLOCK = 8192
K = 10
BETA = 0.2
AMONG = 100


def torch_topk(Qn, Cn, users, seen, boost):
    """(idx, score) by dense torch ops, BLOCK users at a time; boost: None or f32 [M]."""
    ptr, sidx = seen
    dev = Qn.device
    out_i = torch.empty((users.numel(), K), dtype=torch.int64, device=dev)
    out_s = torch.empty((users.numel(), K), dtype=torch.float32, device=dev)
    ninf = torch.full((), float("-inf"), device=dev)
    for b0 in range(0, users.numel(), BLOCK):
        u = users[b0:b0 + BLOCK]
        B = u.numel()
        S = Qn[b0:b0 + B] @ Cn.t()
        if boost is not None:
            S += boost[None, :]
        n = ptr[u + 1] - ptr[u]
        row = torch.repeat_interleave(torch.arange(B, device=dev), n)
        at = torch.repeat_interleave(ptr[u] - torch.cumsum(n, 0) + n, n) + torch.arange(row.numel(), device=dev)
        S.index_put_((row, sidx[at].long()), ninf)
        out_s[b0:b0 + B], out_i[b0:b0 + B] = torch.topk(S, K, dim=1)
    return out_i, out_s


def strided_sets(U, I, n, gen, dev):
    """(ptr, idx): n distinct candidates per user, start + t * stride mod I with n * stride < I."""
    start = torch.randint(0, I, (U, 1), device=dev, generator=gen)
    stride = torch.randint(1, max(2, I // n), (U, 1), device=dev, generator=gen)
    idx = (start + torch.arange(n, device=dev)[None, :] * stride) % I
    return torch.arange(U + 1, device=dev) * n, idx.reshape(-1).to(torch.int32)


def main():
    ap = _probe.parser(reps=5)
    ap.add_argument("--unboosted-only", action="store_true")
    ap.add_argument("--skip-torch", action="store_true")
    args = ap.parse_args()
    dev = _probe.device("boost_probe")
    from lgcn_amd import recommend, synth

    g = synth.ml25m_shaped(seed=0, scale=args.scale)
    U, I = g.num_users, g.num_items
    gen = torch.Generator(device=dev).manual_seed(0)
    seen = recommend.seen_csr(torch.from_numpy(g.edge_index).to(dev), U, I, by="user")
    user_emb = torch.randn(U, args.dim, device=dev, generator=gen)
    item_emb = torch.randn(I, args.dim, device=dev, generator=gen)
    users = torch.arange(U, device=dev)
    attr = (torch.rand(I, device=dev, generator=gen) < 0.2).to(torch.int32)
    among = strided_sets(U, I, AMONG, gen, dev)
    counts = torch.bincount(seen[1].long(), minlength=I)
    rec = dict(users=U, items=I, dim=args.dim, k=K, reps=args.reps, beta=BETA, among=AMONG,
               seen_entries=int(seen[1].numel()), items_with_bit=int(attr.sum()), unboosted_only=args.unboosted_only)

    def ours(boost=None, genre=False, sets=False):
        kw = {} if boost is None else dict(boost=boost)
        if genre:
            kw.update(attrs=attr, where=(1, 0, 0))
        if sets:
            return recommend.topk_rows(user_emb, users, item_emb, K, among=among, **kw)
        return recommend.topk_items(user_emb, item_emb, users, K, seen=seen, **kw)

    arms = {"a_unboosted": lambda: ours(), "d_genre": lambda: ours(genre=True), "f_among": lambda: ours(sets=True)}
    if not args.unboosted_only:
        zero = torch.full((I,), -0.0, dtype=torch.float32, device=dev)
        penalty = recommend.popularity_boost(counts, BETA)
        arms.update({"b_minus_zero": lambda: ours(zero), "c_penalty": lambda: ours(penalty),
                     "e_penalty_genre": lambda: ours(penalty, genre=True), "g_among_penalty": lambda: ours(penalty, sets=True)})
    arms = dict(sorted(arms.items()))
    results, times = _probe.run_arms(arms, args.reps, 2)
    _probe.put_times(rec, times, 2, spread=True)
    popularity = lambda idx: round(float(counts[idx.clamp(min=0)].double().mean()), 2)
    rec["a_mean_popularity_of_top10"] = popularity(results["a_unboosted"][0])
    if not args.unboosted_only:
        lo, hi = rec["a_unboosted_ms_range"]
        rec["a_own_range_ms"] = round(hi - lo, 2)
        for name, base in (("b_minus_zero", "a_unboosted"), ("c_penalty", "a_unboosted"), ("e_penalty_genre", "d_genre"),
                           ("g_among_penalty", "f_among")):
            rec[f"{name}_over_{base}_ms"] = round(rec[f"{name}_ms"] - rec[f"{base}_ms"], 2)
            rec[f"{name}_over_{base}_pct"] = round(100.0 * (rec[f"{name}_ms"] / rec[f"{base}_ms"] - 1.0), 2)
        a, b = results["a_unboosted"], results["b_minus_zero"]
        rec["minus_zero_equals_unboosted"] = bool(torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32),
                                                                                          b[1].view(torch.int32)))
        rec["c_mean_popularity_of_top10"] = popularity(results["c_penalty"][0])
        rec["c_lists_changed"] = round(float((results["c_penalty"][0] != a[0]).any(1).double().mean()), 6)
        if not args.skip_torch:
            Qn = torch.nn.functional.normalize(user_emb, dim=1)
            Cn = torch.nn.functional.normalize(item_emb, dim=1)
            tarms = {"a_unboosted_torch": lambda: torch_topk(Qn, Cn, users, seen, None),
                     "c_penalty_torch": lambda: torch_topk(Qn, Cn, users, seen, penalty)}
            touts, ttimes = _probe.run_arms(tarms, args.reps, 2)
            _probe.put_times(rec, ttimes, 2, spread=True)
            for name in ("a_unboosted", "c_penalty"):
                rec[f"{name}_torch_over_ours"] = round(rec[f"{name}_torch_ms"] / rec[f"{name}_ms"], 3)
                same = (touts[f"{name}_torch"][0] == results[name][0]).all(1)
                rec[f"{name}_lists_equal_to_torch"] = round(float(same.double().mean()), 6)
    _probe.emit(rec, args.out)


if __name__ == "__main__":
    main()
