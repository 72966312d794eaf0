"""Probe: group recommendation at C2 shape (162,541 users x 59,047 items, d = 64, k = 10): all users of
the ML-25M-shaped synthetic graph put into groups, one list per group
(lgcn_amd.recommend.topk_groups), on two workloads:
  four    groups of four consecutive users (40,635 groups), what ANY member has seen left out
          (group_seen_csr(by="any"))
  mixed   groups of 2 to 8 consecutive users, sizes drawn uniformly, the same exclusion

python tools/group_probe.py [--reps 5] [--scale 1.0] [--dim 64] [--floor -0.1] [--skip-torch] [--out FILE]

Per workload, host clock around a device synchronise, after a warm-up of each, medians of --reps with
the range:
  <w>_<strategy>          topk_groups end to end: least_misery, most_pleasure, average, and
                          average_floor (average without anything a member scores under --floor)
  <w>_rows                the parent's unchanged path over the same member rows as independent queries:
                          topk_rows for every member with the member's own seen row left out — the same
                          MFMA work, S times the lists and the selections
  <w>_<strategy>_torch    the batched torch formulation on the same device and unit rows: blocks of
                          groups (a [B, S, M] score block of at most 2^28 floats), mm for the members,
                          amin / amax / mean over the member axis with the padding members masked, -inf
                          on the excluded entries and under the floor, topk
  <w>_padded_rows         the member rows after padding every group to its size class (what the MFMA tile
                          works on, against <w>_member_rows for the independent queries)
  <w>_<strategy>_torch_agreement   the share of groups whose lists agree (mm and mean sum in another
                          order: near-ties may fall the other way)
and <w>_filter_ms / <w>_select_ms: lgcn_score_filter_groups' and the ranked selection's share of one more
least_misery call (each library call between two synchronises). The last line is one JSON record."""
import torch

import _probe

K = 10
BLOCK_FLOATS = 1 << 28  # floats of one [B, S, M] score block of the torch formulation (1 GiB)
STRATEGIES = ("least_misery", "most_pleasure", "average")


def consecutive_groups(U, sizes):
    """Padded member tensor [G, max size] (-1 padding) of consecutive users cut into ``sizes``."""
    ptr = torch.zeros(sizes.numel() + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(sizes, 0)
    keep = ptr[1:] <= U
    ptr, sizes = ptr[:int(keep.sum()) + 1], sizes[keep]
    slot = torch.arange(int(sizes.max()))[None, :]
    return torch.where(slot < sizes[:, None], ptr[:-1, None] + slot, torch.full_like(slot, -1))


def torch_groups(Qn, Cn, members, excl, strategy, floor):
    """(idx, score) [G, K] by dense torch ops, blocks of groups; members [G, S] with -1 padding."""
    eptr, eidx = excl
    dev, (G, S), M = Qn.device, members.shape, Cn.shape[0]
    out_i = torch.empty((G, K), dtype=torch.int64, device=dev)
    out_s = torch.empty((G, K), dtype=torch.float32, device=dev)
    ninf = torch.full((), float("-inf"), device=dev)
    step = max(1, BLOCK_FLOATS // (S * M))
    for b0 in range(0, G, step):
        m = members[b0:b0 + step]
        B = m.shape[0]
        valid = (m >= 0)[:, :, None]
        sc = (Qn[m.clamp(min=0).reshape(-1)] @ Cn.t()).view(B, S, M)
        if strategy == "least_misery":
            red = sc.masked_fill(~valid, float("inf")).amin(1)
        elif strategy == "most_pleasure":
            red = sc.masked_fill(~valid, float("-inf")).amax(1)
        else:
            red = sc.masked_fill(~valid, 0.0).sum(1) / valid.sum(1).to(torch.float32)
        if floor is not None:
            red.masked_fill_((sc.masked_fill(~valid, float("inf")) < floor).any(1), float("-inf"))
        n = eptr[b0 + 1:b0 + B + 1] - eptr[b0:b0 + B]
        row = torch.repeat_interleave(torch.arange(B, device=dev), n)
        red.index_put_((row, eidx[eptr[b0]:eptr[b0 + B]].long()), ninf)
        s, p = torch.topk(red, K, dim=1)
        out_s[b0:b0 + B], out_i[b0:b0 + B] = s, torch.where(torch.isinf(s) & (s < 0), torch.full_like(p, -1), p)
    return out_i, out_s


class Shares:
    """The milliseconds lgcn_score_filter_groups and the ranked selection take within the calls made
    while it is active: each library call between two device synchronises."""

    def __init__(self, lib):
        self.lib, self.ms, self.real = lib, {"filter": 0.0, "select": 0.0}, {}

    def __enter__(self):
        for name, what in (("lgcn_score_filter_groups", "filter"), ("lgcn_select_topk_ranked", "select")):
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


def main():
    ap = _probe.parser(reps=5)
    ap.add_argument("--floor", type=float, default=-0.1)
    ap.add_argument("--skip-torch", action="store_true")
    args = ap.parse_args()
    dev = _probe.device("group_probe")
    from lgcn_amd import _ffi, recommend, synth

    g = synth.ml25m_shaped(seed=0, scale=args.scale)
    U, I = g.num_users, g.num_items
    gen = torch.Generator(device=dev).manual_seed(0)
    seen = recommend.seen_csr(torch.from_numpy(g.edge_index).to(dev), U, I, by="user")
    user_emb = torch.randn(U, args.dim, device=dev, generator=gen)
    item_emb = torch.randn(I, args.dim, device=dev, generator=gen)
    cpu_gen = torch.Generator().manual_seed(0)
    work = {"four": consecutive_groups(U, torch.full((U // 4,), 4, dtype=torch.int64)),
            "mixed": consecutive_groups(U, torch.randint(2, 9, (U // 2,), generator=cpu_gen))}
    rec = dict(users=U, items=I, dim=args.dim, k=K, reps=args.reps, floor=args.floor)
    lib = _ffi.load()
    arms, tarms, shapes = {}, {}, {}
    Qn = torch.nn.functional.normalize(user_emb, dim=1)
    Cn = torch.nn.functional.normalize(item_emb, dim=1)
    for name, padded in work.items():
        csr = recommend.group_csr(padded)
        excl = recommend.group_seen_csr(seen, csr, by="any")
        members = csr[1].to(torch.int64).to(dev)
        rec[f"{name}_groups"], rec[f"{name}_member_rows"] = int(padded.shape[0]), int(members.numel())
        rec[f"{name}_excl_entries"] = int(excl[1].numel())
        sizes = (csr[0][1:] - csr[0][:-1]).clamp(min=2).double()
        # the rows the tile works on: every group padded to its size class, the next power of two
        rec[f"{name}_padded_rows"] = int((2 ** torch.ceil(torch.log2(sizes))).sum())
        pd = padded.to(dev)
        for strategy, floor in [(s, None) for s in STRATEGIES] + [("average", args.floor)]:
            arm = f"{name}_{strategy}" + ("" if floor is None else "_floor")
            arms[arm] = lambda csr=csr, excl=excl, strategy=strategy, floor=floor: recommend.topk_groups(
                user_emb, csr, item_emb, K, strategy=strategy, floor=floor, excl=excl)
            tarms[f"{arm}_torch"] = lambda pd=pd, excl=excl, strategy=strategy, floor=floor: torch_groups(
                Qn, Cn, pd, excl, strategy, floor)
        arms[f"{name}_rows"] = lambda members=members: recommend.topk_rows(
            user_emb, members, item_emb, K, excl=(seen[0], seen[1], members))
        shapes[name] = (csr, excl)
    results, times = _probe.run_arms(arms, args.reps, 2)
    _probe.put_times(rec, times, 2, spread=True)
    for name in work:
        lo, hi = rec[f"{name}_rows_ms_range"]
        for arm in [a for a in arms if a.startswith(name) and not a.endswith("_rows")]:
            glo, ghi = rec[f"{arm}_ms_range"]
            rec[f"{arm}_over_rows"] = round(rec[f"{arm}_ms"] / rec[f"{name}_rows_ms"], 3)
            # expectation one: not slower than the independent rows by more than the two calls' own ranges
            rec[f"{arm}_slower_than_rows_beyond_ranges"] = bool(
                rec[f"{arm}_ms"] - rec[f"{name}_rows_ms"] > (hi - lo) + (ghi - glo))
            rec[f"{arm}_filled"] = round(float((results[arm][0] >= 0).double().mean()), 6)
        csr, excl = shapes[name]
        with Shares(lib) as sh:
            recommend.topk_groups(user_emb, csr, item_emb, K, strategy="least_misery", excl=excl)
        rec[f"{name}_filter_ms"], rec[f"{name}_select_ms"] = round(sh.ms["filter"], 3), round(sh.ms["select"], 3)
    if not args.skip_torch:
        touts, ttimes = _probe.run_arms(tarms, args.reps, 2)
        _probe.put_times(rec, ttimes, 2, spread=True)
        for arm in tarms:
            ours = arm[:-len("_torch")]
            rec[f"{arm}_over_ours"] = round(rec[f"{arm}_ms"] / rec[f"{ours}_ms"], 3)
            same = (touts[arm][0] == results[ours][0]).all(1)
            rec[f"{arm}_agreement"] = round(float(same.double().mean()), 6)
    _probe.emit(rec, args.out)


if __name__ == "__main__":
    main()
