"""Probe: fold-in for every history at C2 shape (162,541 histories over 59,047 items, d = 64, mean
77 entries, longest 31,703): each user's row rebuilt from their item history as if the model had
never seen them, then their top 10 with the history excluded.

python tools/foldin_probe.py [--reps 5] [--scale 1.0] [--k 10] [--out FILE]

Timings, each the median of --reps after a warm-up (all repetitions are printed and kept, the range
is reported), the arms alternating in one process, host clock around a device synchronise:
  foldin      lgcn_amd.foldin.fold_in_rows over all histories (table, isd = 1 / sqrt(degree + 1)), against
  torch       the torch formulation on the same device and inputs: index_select of every entry's row
              (an [E, d] intermediate), a multiply by isd[i] / sqrt(n), index_add_ into [Q, d] (float
              atomics: its bits change from run to run)
  topk        lgcn_amd.recommend.topk_rows(k) of the folded rows with the histories excluded, alone
  served      fold_in_rows then topk_rows: what serving unseen users costs over serving known ones
  longest     fold_in_rows for the single longest history (both launches, eight waves on that row):
              its share of ``foldin`` bounds what the heavy tail costs
The last line is one JSON record: the timings, the ratio torch / foldin, the largest difference
between the two arms relative to the row's largest entry, and whether two fold-in runs agree bit
for bit. The kernels' own times come from a kernel trace in a run of its own
(rocprofv3 --kernel-trace --stats -- python tools/foldin_probe.py --reps 1).
"""
import torch

import _probe


def torch_foldin(ptr, idx, table, isd):
    """The same rows in plain torch ops: gather, scale, scatter-add."""
    Q = ptr.numel() - 1
    length = ptr[1:] - ptr[:-1]
    row = torch.repeat_interleave(torch.arange(Q, device=ptr.device), length)
    i = idx.to(torch.int64)
    scale = torch.rsqrt(length.clamp(min=1).to(torch.float32))
    terms = table.index_select(0, i) * (isd[i] * scale[row])[:, None]
    return torch.zeros((Q, table.shape[1]), dtype=torch.float32, device=ptr.device).index_add_(0, row, terms)


def main():
    ap = _probe.parser(reps=5)
    ap.add_argument("--k", type=int, default=10)
    args = ap.parse_args()
    dev = _probe.device("foldin_probe")
    from lgcn_amd import foldin, recommend, synth

    g = synth.ml25m_shaped(seed=0, scale=args.scale)
    U, I = g.num_users, g.num_items
    ei = torch.from_numpy(g.edge_index).to(dev)
    seen = recommend.seen_csr(ei, U, I, by="user")
    ptr, sidx = seen
    by_item = recommend.seen_csr(ei, U, I, by="item")[0]
    isd = foldin.inv_sqrt_degree(by_item[1:] - by_item[:-1])
    gen = torch.Generator(device=dev).manual_seed(0)
    table = torch.randn(I, args.dim, device=dev, generator=gen)
    length = ptr[1:] - ptr[:-1]
    heavy = torch.argmax(length).view(1)
    k = args.k
    picked = torch.arange(U, device=dev)
    rows = foldin.fold_in_rows(seen, table, isd=isd).rows

    def served():
        q = foldin.fold_in_rows(seen, table, isd=isd).rows
        return recommend.topk_rows(q, picked, table, k, excl=seen, index_dtype=torch.int32)

    arms = {"foldin": lambda: foldin.fold_in_rows(seen, table, isd=isd).rows,
            "torch": lambda: torch_foldin(ptr, sidx, table, isd),
            "topk": lambda: recommend.topk_rows(rows, picked, table, k, excl=seen, index_dtype=torch.int32),
            "served": served,
            "longest": lambda: foldin.fold_in_rows((ptr, sidx, heavy), table, isd=isd).rows}
    results, times = _probe.run_arms(arms, args.reps, 3)
    rec = dict(histories=U, items=I, dim=args.dim, k=k, entries=int(sidx.numel()), longest_history=int(length.max()),
               mean_history=round(float(length.float().mean()), 2),
               long_histories=int((length > foldin.LONG).sum()), reps=args.reps)
    _probe.put_times(rec, times, 3, spread=True)
    rec["torch_over_foldin"] = round(rec["torch_ms"] / rec["foldin_ms"], 3)
    rec["foldin_cost_ms"] = round(rec["served_ms"] - rec["topk_ms"], 3)
    rec["longest_share_of_foldin"] = round(rec["longest_ms"] / rec["foldin_ms"], 3)
    rec["gather_gb_per_s"] = round(sidx.numel() * args.dim * 4 / rec["foldin_ms"] / 1e6, 1)
    ours, theirs = results["foldin"], results["torch"]
    top = theirs.abs().amax(1).clamp(min=1e-30)
    rec["max_row_relative_difference"] = float(((ours - theirs).abs().amax(1) / top).max())
    rec["foldin_bitwise_repeatable"] = bool(torch.equal(ours, rows))
    rec["torch_bitwise_repeatable"] = bool(torch.equal(theirs, torch_foldin(ptr, sidx, table, isd)))
    rec["longest_equals_batch_row"] = bool(torch.equal(results["longest"][0], ours[heavy[0]]))
    rec["served_equals_topk"] = bool(torch.equal(results["served"][0], results["topk"][0]))
    _probe.emit(rec, args.out)


if __name__ == "__main__":
    main()
