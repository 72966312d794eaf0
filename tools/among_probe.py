"""Probe: per-query candidate sets at C2 shape (162,541 users x 59,047 items, d = 64, k = 10): every
user ranks ITS candidates and nothing else (lgcn_amd.recommend.topk_rows' among=), on three workloads:
  w100      100 candidates per user      the 1 + 99 sampled-negative protocol
  w1000     1,000 candidates per user    a retrieval stage's output
  history   each user's own history of the ML-25M-shaped synthetic graph (mean 77, longest 31,703)

python tools/among_probe.py [--reps 5] [--scale 1.0] [--dim 64] [--excl-users 8192] [--out FILE]

Per workload, host clock around a device synchronise, after a warm-up of each, medians of --reps with
the range:
  <w>                 topk_rows(among=) end to end
  <w>_score_ms / <w>_select_ms   lgcn_score_lists' and the ranked selection's share of one more call
                      (each library call between two synchronises), pairs/s and the gathered bytes/s
                      (pairs x D x 4) that share implies
  <w>_torch           the batched torch formulation on the same device and unit rows: rows bucketed
                      by length (powers of two), padded gather, bmm, -inf on the padding, topk
  <w>_torch_agreement the share of users whose lists agree (bmm sums in another order: near-ties may
                      fall the other way)
For the first --excl-users users of w100 the same request is also written as complement exclusion
rows (every item outside the set) through today's path; it reports whether that completes at all.
The last line is one JSON record."""
import torch

import _probe

K = 10
GATHER_FLOATS = 1 << 28  # floats of one padded gather of the torch formulation (1 GiB)


def strided_sets(U, I, n, gen, dev):
    """(ptr, idx): n distinct candidates per user, start + t * stride mod I with n * stride < I."""
    start = torch.randint(0, I, (U, 1), device=dev, generator=gen)
    stride = torch.randint(1, max(2, I // n), (U, 1), device=dev, generator=gen)
    idx = (start + torch.arange(n, device=dev)[None, :] * stride) % I
    return torch.arange(U + 1, device=dev) * n, idx.reshape(-1).to(torch.int32)


def torch_among(Qn, Cn, csr):
    """(idx, score) [U, K] by dense torch ops: rows of a length bucket gathered padded, bmm, topk."""
    ptr, idx = csr
    dev, U, D = Qn.device, Qn.shape[0], Qn.shape[1]
    out_i = torch.full((U, K), -1, dtype=torch.int64, device=dev)
    out_s = torch.full((U, K), float("-inf"), dtype=torch.float32, device=dev)
    lens = ptr[1:] - ptr[:-1]
    bucket = torch.where(lens > 0, torch.ceil(torch.log2(lens.clamp(min=1).double())).long(), torch.full_like(lens, -1))
    order = torch.argsort(bucket, stable=True)
    counts = torch.bincount(bucket + 1, minlength=2).tolist()  # the host read: rows per bucket
    at = counts[0]  # empty rows keep their padding
    for b, n in enumerate(counts[1:]):
        L = 1 << b
        step = max(1, GATHER_FLOATS // (L * D))
        for r0 in range(at, at + n, step):
            r = order[r0:min(r0 + step, at + n)]
            t = torch.arange(L, device=dev)[None, :]
            valid = t < lens[r][:, None]
            j = idx[(ptr[r][:, None] + t).clamp(max=idx.numel() - 1)].long()
            S = torch.bmm(Cn[j], Qn[r].unsqueeze(2)).squeeze(2)
            S.masked_fill_(~valid, float("-inf"))
            s, p = torch.topk(S, min(K, L), dim=1)
            got = torch.where(torch.isinf(s) & (s < 0), torch.full_like(p, -1), j.gather(1, p))
            out_i[r, :got.shape[1]] = got
            out_s[r, :s.shape[1]] = s
        at += n
    return out_i, out_s


class Shares:
    """The milliseconds lgcn_score_lists and the ranked selections take within the calls made while
    it is active: each library call between two device synchronises."""

    def __init__(self, lib):
        self.lib, self.ms, self.real = lib, {"score": 0.0, "select": 0.0}, {}

    def __enter__(self):
        for name, what in (("lgcn_score_lists", "score"), ("lgcn_select_topk_ranked", "select")):
            self.real[name] = getattr(self.lib, name)

            def timing(*a, fn=self.real[name], what=what):
                rc, ms = _probe.timed(lambda: fn(*a))
                self.ms[what] += ms
                return rc

            setattr(self.lib, name, timing)
        return self

    def __exit__(self, *exc):
        for name, fn in self.real.items():
            setattr(self.lib, name, fn)


def complement_rows(csr, users, I):
    """The exclusion CSR of ``users``: every item outside the user's set."""
    ptr, idx = csr
    dev, B = users.device, users.numel()
    drop = torch.ones((B, I), dtype=torch.bool, device=dev)
    n = ptr[users + 1] - ptr[users]
    row = torch.repeat_interleave(torch.arange(B, device=dev), n)
    at = torch.repeat_interleave(ptr[users] - torch.cumsum(n, 0) + n, n) + torch.arange(row.numel(), device=dev)
    drop[row, idx[at].long()] = False
    out_ptr = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    out_ptr[1:] = torch.cumsum(drop.sum(1), 0)
    return out_ptr, torch.nonzero(drop)[:, 1].to(torch.int32)


def main():
    ap = _probe.parser(reps=5)
    ap.add_argument("--excl-users", type=int, default=8192)
    ap.add_argument("--skip-torch", action="store_true")
    args = ap.parse_args()
    dev = _probe.device("among_probe")
    from lgcn_amd import _ffi, _serving, recommend, synth

    g = synth.ml25m_shaped(seed=0, scale=args.scale)
    U, I = g.num_users, g.num_items
    gen = torch.Generator(device=dev).manual_seed(0)
    user_emb = torch.randn(U, args.dim, device=dev, generator=gen)
    item_emb = torch.randn(I, args.dim, device=dev, generator=gen)
    users = torch.arange(U, device=dev)
    work = {"w100": strided_sets(U, I, 100, gen, dev), "w1000": strided_sets(U, I, 1000, gen, dev),
            "history": recommend.seen_csr(torch.from_numpy(g.edge_index).to(dev), U, I, by="user")}
    D = _serving.width("among_probe", args.dim)
    rec = dict(users=U, items=I, dim=args.dim, k=K, reps=args.reps)
    lib = _ffi.load()
    ours = lambda csr: recommend.topk_rows(user_emb, users, item_emb, K, among=csr)
    arms = {name: (lambda csr=csr: ours(csr)) for name, csr in work.items()}
    results, times = _probe.run_arms(arms, args.reps, 2)
    _probe.put_times(rec, times, 2, spread=True)
    for name, csr in work.items():
        lens = csr[0][1:] - csr[0][:-1]
        pairs = int(csr[1].numel())
        rec[f"{name}_pairs"], rec[f"{name}_longest"] = pairs, int(lens.max())
        with Shares(lib) as sh:
            ours(csr)
        rec[f"{name}_score_ms"], rec[f"{name}_select_ms"] = round(sh.ms["score"], 3), round(sh.ms["select"], 3)
        rec[f"{name}_pairs_per_s"] = round(pairs / (sh.ms["score"] * 1e-3), -6)
        rec[f"{name}_gathered_TB_per_s"] = round(pairs * D * 4 / (sh.ms["score"] * 1e-3) / 1e12, 3)
    if not args.skip_torch:
        Qn = torch.nn.functional.normalize(user_emb, dim=1)
        Cn = torch.nn.functional.normalize(item_emb, dim=1)
        tarms = {f"{name}_torch": (lambda csr=csr: torch_among(Qn, Cn, csr)) for name, csr in work.items()}
        touts, ttimes = _probe.run_arms(tarms, args.reps, 2)
        _probe.put_times(rec, ttimes, 2, spread=True)
        for name in work:
            rec[f"{name}_torch_over_ours"] = round(rec[f"{name}_torch_ms"] / rec[f"{name}_ms"], 3)
            same = (touts[f"{name}_torch"][0] == results[name][0]).all(1)
            rec[f"{name}_torch_agreement"] = round(float(same.double().mean()), 6)
    # w100 written as complement exclusion rows through today's path, on the first users
    who = users[:min(args.excl_users, U)]
    rec["excl_users"] = int(who.numel())
    rows = complement_rows(work["w100"], who, I)
    rec["w100_excl_entries"] = int(rows[1].numel())
    sub = (work["w100"][0], work["w100"][1], who)
    try:
        today = lambda: recommend.topk_rows(user_emb, who, item_emb, K, excl=rows)
        got, ms = _probe.timed(today)
        got, ms = _probe.timed(today)  # the second call: warm
        want = recommend.topk_rows(user_emb, who, item_emb, K, among=sub)
        rec["w100_as_exclusion"] = dict(completes=True, ms=round(ms, 2), equal=bool(torch.equal(got[0], want[0])))
    except (RuntimeError, ValueError) as e:
        rec["w100_as_exclusion"] = dict(completes=False, error=f"{type(e).__name__}: {e}"[:200])
    _, ms = _probe.timed(lambda: recommend.topk_rows(user_emb, who, item_emb, K, among=sub))
    _, ms = _probe.timed(lambda: recommend.topk_rows(user_emb, who, item_emb, K, among=sub))
    rec["w100_among_same_users_ms"] = round(ms, 2)
    _probe.emit(rec, args.out)


if __name__ == "__main__":
    main()
