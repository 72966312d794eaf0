"""Probe: attribute-filtered top-k at C2 shape (162,541 users x 59,047 items, d = 64): every user's
k = 10 best unseen items of the ML-25M-shaped synthetic graph, under no filter and four filters.

python tools/filter_probe.py [--reps 5] [--scale 1.0] [--dim 64] [--excl-users 8192] [--out FILE]

Times, host clock around a device synchronise, after a warm-up of each, medians of --reps with the
range, of lgcn_amd.recommend.topk_items:
  (a) unfiltered                        today's call
  (b) an all-pass filter (0, 0, 0)      the filtered kernels with nothing to drop: (b) - (a) is what the
                                        epilogue costs, reported beside (a)'s own run-to-run range
  (c) any = a bit on about 20 % of the items
  (d) any = a bit on about 0.5 %
  (e) per-user masks drawn from a palette of eight filters
each against the batched torch formulation on the same device and unit rows: blocks of 8,192 users,
mm, -inf on the seen pairs and where the predicate fails, topk. For (c) and (d) the same request is
also written as exclusion rows (a user's seen items joined with every item that fails) and run
through the unfiltered path, on the first --excl-users users (the rows of all users do not fit a
device: 0.8 x 59,047 entries each at 20 %), beside the filtered call on the same users; it reports
whether that completes at all. The last line is one JSON record."""
import torch

import _probe

BLOCK = 8192
K = 10
# (any, all, none) over bits 0 (20 %), 1 (0.5 %), 2 (50 %), 3 (10 %)
PALETTE = [(0, 0, 0), (1, 0, 0), (2, 0, 0), (4, 0, 0), (0, 4 | 8, 0), (0, 0, 1), (1 | 8, 0, 4), (4, 1, 8)]


def passes(attr, any_, all_, none):
    """The predicate on int32 words; the masks broadcast against attr."""
    return ((attr & none) == 0) & ((attr & all_) == all_) & ((any_ == 0) | ((attr & any_) != 0))


def torch_topk(Qn, Cn, users, seen, attr, where):
    """(idx, score) by dense torch ops, BLOCK users at a time; where: None, or three ints / int32 [Q]."""
    ptr, sidx = seen
    dev = Qn.device
    out_i = torch.empty((users.numel(), K), dtype=torch.int64, device=dev)
    out_s = torch.empty((users.numel(), K), dtype=torch.float32, device=dev)
    ninf = torch.full((), float("-inf"), device=dev)
    for b0 in range(0, users.numel(), BLOCK):
        u = users[b0:b0 + BLOCK]
        B = u.numel()
        S = Qn[b0:b0 + B] @ Cn.t()
        n = ptr[u + 1] - ptr[u]
        row = torch.repeat_interleave(torch.arange(B, device=dev), n)
        at = torch.repeat_interleave(ptr[u] - torch.cumsum(n, 0) + n, n) + torch.arange(row.numel(), device=dev)
        S.index_put_((row, sidx[at].long()), ninf)
        if where is not None:
            m = [w[b0:b0 + B, None] if torch.is_tensor(w) else w for w in where]
            S.masked_fill_(~passes(attr[None, :], *m), float("-inf"))
        out_s[b0:b0 + B], out_i[b0:b0 + B] = torch.topk(S, K, dim=1)
    return out_i, out_s


def union_rows(seen, users, fails):
    """The exclusion CSR (ptr, idx) of ``users``: a user's seen items joined with every failing item."""
    ptr, sidx = seen
    dev = users.device
    B = users.numel()
    drop = fails[None, :].repeat(B, 1)
    n = ptr[users + 1] - ptr[users]
    row = torch.repeat_interleave(torch.arange(B, device=dev), n)
    at = torch.repeat_interleave(ptr[users] - torch.cumsum(n, 0) + n, n) + torch.arange(row.numel(), device=dev)
    drop[row, sidx[at].long()] = True
    out_ptr = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    out_ptr[1:] = torch.cumsum(drop.sum(1), 0)
    return out_ptr, torch.nonzero(drop)[:, 1].to(torch.int32)


def main():
    ap = _probe.parser(reps=5)
    ap.add_argument("--excl-users", type=int, default=8192)
    ap.add_argument("--skip-torch", action="store_true")
    args = ap.parse_args()
    dev = _probe.device("filter_probe")
    from lgcn_amd import recommend, synth

    g = synth.ml25m_shaped(seed=0, scale=args.scale)
    U, I = g.num_users, g.num_items
    gen = torch.Generator(device=dev).manual_seed(0)
    seen = recommend.seen_csr(torch.from_numpy(g.edge_index).to(dev), U, I, by="user")
    user_emb = torch.randn(U, args.dim, device=dev, generator=gen)
    item_emb = torch.randn(I, args.dim, device=dev, generator=gen)
    users = torch.arange(U, device=dev)
    draw = torch.rand((4, I), device=dev, generator=gen)
    attr = torch.zeros(I, dtype=torch.int32, device=dev)
    for b, p in enumerate((0.2, 0.005, 0.5, 0.1)):
        attr |= (draw[b] < p).to(torch.int32) << b
    pal = torch.tensor(PALETTE, dtype=torch.int32, device=dev)[torch.randint(0, len(PALETTE), (U,), device=dev, generator=gen)]
    cases = {"a_unfiltered": None, "b_all_pass": (0, 0, 0), "c_20pct": (1, 0, 0), "d_half_pct": (2, 0, 0),
             "e_palette": tuple(pal[:, c].contiguous() for c in range(3))}
    rec = dict(users=U, items=I, dim=args.dim, k=K, reps=args.reps, seen_entries=int(seen[1].numel()),
               items_with_bit=[int(((attr >> b) & 1).sum()) for b in range(4)])

    def ours(where, who=users, excl=None):
        if excl is not None:
            return recommend.topk_rows(user_emb, who, item_emb, K, excl=excl)
        kw = {} if where is None else dict(attrs=attr, where=where)
        return recommend.topk_items(user_emb, item_emb, who, K, seen=seen, **kw)

    arms = {name: (lambda w=w: ours(w)) for name, w in cases.items()}
    results, times = _probe.run_arms(arms, args.reps, 2)
    _probe.put_times(rec, times, 2, spread=True)
    lo, hi = rec["a_unfiltered_ms_range"]
    rec["epilogue_ms"] = round(rec["b_all_pass_ms"] - rec["a_unfiltered_ms"], 2)
    rec["a_own_range_ms"] = round(hi - lo, 2)
    rec["epilogue_exceeds_a_range"] = bool(abs(rec["epilogue_ms"]) > hi - lo)
    rec["all_pass_equals_unfiltered"] = bool(torch.equal(results["a_unfiltered"][0], results["b_all_pass"][0]))
    for name in cases:
        rec[f"{name}_filled"] = round(float((results[name][0] >= 0).double().mean()), 6)
    if not args.skip_torch:
        Qn = torch.nn.functional.normalize(user_emb, dim=1)
        Cn = torch.nn.functional.normalize(item_emb, dim=1)
        tarms = {f"{name}_torch": (lambda w=w: torch_topk(Qn, Cn, users, seen, attr, w)) for name, w in cases.items()}
        touts, ttimes = _probe.run_arms(tarms, args.reps, 2)
        _probe.put_times(rec, ttimes, 2, spread=True)
        for name in cases:
            rec[f"{name}_torch_over_ours"] = round(rec[f"{name}_torch_ms"] / rec[f"{name}_ms"], 3)
            # torch.mm sums in another order: near-ties may fall the other way
            rec[f"{name}_torch_agreement"] = round(float((touts[f"{name}_torch"][0] == results[name][0]).double().mean()), 6)
    # (c) and (d) written as exclusion rows through the unfiltered path, on the first users
    who = users[:min(args.excl_users, U)]
    rec["excl_users"] = int(who.numel())
    for name in ("c_20pct", "d_half_pct"):
        w = cases[name]
        rows = union_rows(seen, who, ~passes(attr, *w))
        rec[f"{name}_excl_entries"] = int(rows[1].numel())
        try:
            got, ms = _probe.timed(lambda: ours(None, who, rows))
            got, ms = _probe.timed(lambda: ours(None, who, rows))  # the second call: warm
            want = ours(w, who)
            rec[f"{name}_as_exclusion"] = dict(completes=True, ms=round(ms, 2), equal=bool(torch.equal(got[0], want[0])))
        except (RuntimeError, ValueError) as e:
            rec[f"{name}_as_exclusion"] = dict(completes=False, error=f"{type(e).__name__}: {e}"[:200])
        _, ms = _probe.timed(lambda: ours(w, who))
        rec[f"{name}_filtered_same_users_ms"] = round(ms, 2)
    _probe.emit(rec, args.out)


if __name__ == "__main__":
    main()
