"""Probe: exact full-ranking positions and AUC of every user at C2 shape (162,541 users x 59,047
items, d = 64), five items per user held out of the ML-25M-shaped synthetic graph and the rest
(about 77 per user) excluded as seen — rank_eval_probe's workload.

python tools/rank_position_probe.py [--reps 5] [--scale 1.0] [--dim 64] [--out FILE]

Times, host clock around a device synchronise, after a warm-up of each, medians of --reps with the
range:
  * the whole lgcn_amd.metrics.evaluate_auc, and evaluate_ranking at ks=(20,) beside it;
  * lgcn_rank_positions' three stages on their own (its stages mask): the targets' keys, the dense
    count, the seen correction;
  * lgcn_score_filter alone over the same Q x M with a threshold nothing passes (+inf): the MFMA
    floor — the dense count runs the same matrix instructions, so its ratio to this is the price of
    the counting epilogue;
  * a batched torch formulation on the same device and the same unit rows: blocks of 8,192 users,
    mm, index_put_ of -inf on the seen pairs, a gather of the targets' scores, then
    (scores > t) | ((scores == t) & (index < j)) summed per target; and the share of (user, item)
    pairs on which it gives the kernel's position (torch.mm sums in another order, so near-ties
    may fall the other way).
A second row repeats the kernel's timings with 20 % of every user's items held out: long truth rows,
many passes of the dense count. The last line is one JSON record."""
import ctypes

import torch

import _probe
from rank_eval_probe import split_edges

BLOCK = 8192


def split_fraction(ptr, idx, U, gen, share):
    """(train, held-out) edge lists of a user CSR: a random ``share`` of every row (rounded down)."""
    deg = ptr[1:] - ptr[:-1]
    row = torch.repeat_interleave(torch.arange(U, device=ptr.device), deg)
    order = torch.argsort(row.double() + torch.rand(row.numel(), device=ptr.device, generator=gen, dtype=torch.float64))
    rank = torch.arange(row.numel(), device=ptr.device) - ptr[row]
    held = torch.zeros(row.numel(), dtype=torch.bool, device=ptr.device)
    held[order] = rank < (deg[row].double() * share).long()
    edges = torch.stack([row, idx.long() + U])
    return edges[:, ~held], edges[:, held]


class Staged:
    """rank_positions' buffers, kept, so that lgcn_rank_positions can be issued stage by stage."""

    def __init__(self, lib, user_emb, item_emb, users, truth, seen):
        from lgcn_amd import _ffi, _serving, metrics

        dev = user_emb.device
        self.lib, self.s = lib, _ffi.stream_of(dev)
        self.Q, self.M, d = users.numel(), item_emb.shape[0], user_emb.shape[1]
        self.D = _serving.width("probe", d)
        self.Qpad = _serving.padded(self.Q)
        self.Cn = _serving.unit_rows(lib, item_emb, self.D, False, self.s)
        # longest truth row first, as rank_positions hands its queries over
        users = users[_serving.longest_first(_serving.row_lengths(truth[0], users, self.Q)).indices]
        self.users, self.truth, self.seen = users, truth, seen
        self.Qn = _serving.unit_queries(lib, user_emb, users, self.D, self.Qpad, False, self.s)
        self.out_ptr = torch.zeros(self.Q + 1, dtype=torch.int64, device=dev)
        self.out_ptr[1:] = torch.cumsum(_serving.row_lengths(truth[0], users, self.Q), 0)
        lens = self.out_ptr[1:] - self.out_ptr[:-1]
        self.nnz = int(self.out_ptr[-1])
        self.tiers = metrics._tiers(self.Q, [int((lens > n).sum()) for n in metrics.TIER_LENGTHS])
        self.pos = torch.empty(self.nnz, dtype=torch.int32, device=dev)
        self.key = torch.empty(self.nnz, dtype=torch.int32, device=dev)
        self.eligible = torch.empty(self.Q, dtype=torch.int32, device=dev)
        need = ctypes.c_size_t(0)
        _ffi.check(lib.lgcn_rank_positions_workspace_size(self.Q, self.nnz, ctypes.byref(need)), "workspace_size")
        self.ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        # the filter-only floor: one list slot per query, thresholds at +inf (key 0xFF800000)
        self.lkey = torch.empty(self.Qpad, dtype=torch.int32, device=dev)
        self.lidx = torch.empty(self.Qpad, dtype=torch.int32, device=dev)
        self.lcnt = torch.zeros(self.Qpad, dtype=torch.int32, device=dev)
        self.thr = torch.full((self.Qpad,), 0xFF800000 - (1 << 32), dtype=torch.int32, device=dev)

    def stage(self, mask):
        from lgcn_amd import metrics

        t, sn = self.truth, self.seen
        metrics._issue_positions(self.lib, self.tiers, self.Qn, self.D, self.Cn, self.M, t[0], t[1], self.users, sn[0],
                                 sn[1], self.users, self.out_ptr, self.nnz, self.pos, self.key, self.eligible, self.ws,
                                 mask, self.s)

    def floor(self):
        from lgcn_amd import _ffi

        _ffi.check(self.lib.lgcn_score_filter(self.Qn.data_ptr(), self.Qpad, self.Q, self.Cn.data_ptr(), self.M, 1,
                                              self.D, self.thr.data_ptr(), self.lkey.data_ptr(), self.lidx.data_ptr(),
                                              self.lcnt.data_ptr(), 1, self.s), "lgcn_score_filter")


def torch_positions(st: Staged):
    """int32 [nnz]: the positions by dense torch ops on st's unit rows, BLOCK users at a time."""
    dev = st.Qn.device
    tptr, tidx = st.truth
    sptr, sidx = st.seen
    Cn = st.Cn[:, :]
    out = torch.empty(st.nnz, dtype=torch.int32, device=dev)
    col = torch.arange(st.M, device=dev)[None, :]
    for b0 in range(0, st.Q, BLOCK):
        u = st.users[b0:b0 + BLOCK]
        B = u.numel()
        S = st.Qn[b0:b0 + B] @ Cn.t()
        slen = sptr[u + 1] - sptr[u]
        srow = torch.repeat_interleave(torch.arange(B, device=dev), slen)
        sat = torch.repeat_interleave(sptr[u] - torch.cumsum(slen, 0) + slen, slen) + torch.arange(srow.numel(), device=dev)
        tlen = tptr[u + 1] - tptr[u]
        trow = torch.repeat_interleave(torch.arange(B, device=dev), tlen)
        nth = torch.arange(trow.numel(), device=dev) - (torch.cumsum(tlen, 0) - tlen)[trow]
        tj = tidx[tptr[u][trow] + nth].long()
        S.index_put_((srow, sidx[sat].long()), torch.full((), float("-inf"), device=dev))
        tscore = S[trow, tj]
        was_seen = torch.isinf(tscore) & (tscore < 0)
        base = int(st.out_ptr[b0])
        got = torch.empty(trow.numel(), dtype=torch.int32, device=dev)
        for n in range(int(tlen.max()) if B else 0):  # the n-th target of every user that has one
            pick = nth == n
            r, j, t = trow[pick], tj[pick], tscore[pick]
            rows = S[r]
            above = (rows > t[:, None]) | ((rows == t[:, None]) & (col < j[:, None]))
            got[pick] = above.sum(1, dtype=torch.int32)
        out[base:base + trow.numel()] = torch.where(was_seen, torch.full_like(got, -1), got)
    return out


def main():
    ap = _probe.parser(reps=5)
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--skip-long", action="store_true")
    args = ap.parse_args()
    dev = _probe.device("rank_position_probe")
    from lgcn_amd import _ffi, metrics, recommend, synth

    lib = _ffi.load()
    g = synth.ml25m_shaped(seed=0, scale=args.scale)
    U, I = g.num_users, g.num_items
    gen = torch.Generator(device=dev).manual_seed(0)
    every = recommend.seen_csr(torch.from_numpy(g.edge_index).to(dev), U, I, by="user")
    user_emb = torch.randn(U, args.dim, device=dev, generator=gen)
    item_emb = torch.randn(I, args.dim, device=dev, generator=gen)
    rec = dict(users=U, items=I, dim=args.dim, reps=args.reps)

    def row(tag, train, held, with_torch):
        seen, truth = recommend.seen_csr(train, U, I), recommend.seen_csr(held, U, I)
        users = torch.nonzero(truth[0][1:] > truth[0][:-1]).view(-1)
        tl = truth[0][1:] - truth[0][:-1]
        rec[f"{tag}evaluated_users"], rec[f"{tag}truth_entries"] = int(users.numel()), int(truth[1].numel())
        rec[f"{tag}seen_entries"], rec[f"{tag}longest_truth_row"] = int(seen[1].numel()), int(tl.max())
        rec[f"{tag}rows_above_{metrics.TIER_LENGTHS[0]}"] = int((tl > metrics.TIER_LENGTHS[0]).sum())
        rec[f"{tag}rows_above_{metrics.TIER_LENGTHS[1]}"] = int((tl > metrics.TIER_LENGTHS[1]).sum())
        whole = {"evaluate_auc": lambda: metrics.evaluate_auc(user_emb, item_emb, truth, seen=seen, users=users, ks=(20,))}
        if with_torch:
            whole["evaluate_ranking"] = lambda: metrics.evaluate_ranking(user_emb, item_emb, truth, ks=(20,), seen=seen,
                                                                         users=users)
        results, times = _probe.run_arms(whole, args.reps, 2, label=tag)
        st = Staged(lib, user_emb, item_emb, users, truth, seen)
        st.stage(_ffi.RANKPOS_ALL)
        kernel_pos = st.pos.clone()
        arms = {"stage_keys": lambda: st.stage(_ffi.RANKPOS_KEYS), "stage_count": lambda: st.stage(_ffi.RANKPOS_COUNT),
                "stage_finish": lambda: st.stage(_ffi.RANKPOS_FINISH), "filter_floor": st.floor}
        if with_torch:
            arms["torch"] = lambda: torch_positions(st)
        outs, stage_times = _probe.run_arms(arms, args.reps, 3, label=tag)
        times.update(stage_times)
        _probe.put_times(rec, {f"{tag}{k}": v for k, v in times.items()}, 3, spread=True)
        rec[f"{tag}count_over_floor"] = round(rec[f"{tag}stage_count_ms"] / rec[f"{tag}filter_floor_ms"], 3)
        rec[f"{tag}floor_passed"] = int(st.lcnt.max())  # 0: the floor stored nothing
        if with_torch:
            rec[f"{tag}torch_over_evaluate_auc"] = round(rec[f"{tag}torch_ms"] / rec[f"{tag}evaluate_auc_ms"], 3)
            rec[f"{tag}torch_agreement"] = float((outs["torch"] == kernel_pos).double().mean())
            rec[f"{tag}torch_max_position_diff"] = int((outs["torch"] - kernel_pos).abs().max())
        rec[f"{tag}metrics"] = {k: round(v, 6) for k, v in results["evaluate_auc"].items()}

    row("", *split_edges(*every, U, gen), not args.skip_torch)
    if not args.skip_long:
        row("split20_", *split_fraction(*every, U, gen, 0.2), False)
    _probe.emit(rec, args.out)


if __name__ == "__main__":
    main()
