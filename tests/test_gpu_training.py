"""Training path on the GPU: the harness mirror driving the HIP LightGCN vs the same harness
driving the CPU oracle model, with identical negatives (the sampler is patched to draw on the
CPU so both runs see the same draws)."""
import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle.lgconv_torch import OracleLightGCN
from parity import assert_rows_close

pytestmark = pytest.mark.gpu

G = np.load(GOLDEN / "harness.npz")


class _Batch:
    def __init__(self, ei):
        self.edge_index = ei

    def to(self, device):
        return _Batch(self.edge_index.to(device))


@pytest.fixture
def cpu_negatives(monkeypatch):
    from utils import helpers

    state = {"g": None}

    def sample_negative(pos_idx, num_items, device):
        return torch.randint(0, num_items, (pos_idx.shape[0],), generator=state["g"]).to(device)

    monkeypatch.setattr(helpers, "sample_negative", sample_negative)

    def reseed(s):
        state["g"] = torch.Generator().manual_seed(s)

    return reseed


def _models(gpu):
    from models.light_gcn import LightGCN

    U, I = int(G["train_U"]), int(G["train_I"])
    hip = LightGCN(U, I, num_layers=3, dim_h=64).to(gpu)
    ref = OracleLightGCN(U, I, num_layers=3, dim_h=64)
    for m in (hip, ref):
        with torch.no_grad():
            m.user_embedding.weight.copy_(torch.from_numpy(G["train_init_user_w"]))
            m.item_embedding.weight.copy_(torch.from_numpy(G["train_init_item_w"]))
    return hip, ref


def test_first_step_loss_and_grads_match(gpu, cpu_negatives):
    from utils import train_test as TT

    hip, ref = _models(gpu)
    b = torch.from_numpy(G["train_batch0"])
    out = {}
    for name, m, dev in (("hip", hip, gpu), ("ref", ref, torch.device("cpu"))):
        cpu_negatives(5)
        loss = TT.bpr_loss(*TT.compute_embeddings(m, _Batch(b).to(dev), dev))
        loss.backward()
        out[name] = (loss.item(), m.user_embedding.weight.grad.cpu().numpy(), m.item_embedding.weight.grad.cpu().numpy())
    assert abs(out["hip"][0] - out["ref"][0]) <= 1e-5 * abs(out["ref"][0])
    for name, a, r in zip(("grad_user", "grad_item"), out["hip"][1:], out["ref"][1:]):
        assert_rows_close(a, r, what=name)  # per row: 1e-5 of that row's max |ref|


def test_epoch_matches_oracle_harness(gpu, cpu_negatives):
    from utils import train_test as TT

    hip, ref = _models(gpu)
    batches = [torch.from_numpy(G[f"train_batch{p}"]) for p in range(3)]
    res = {}
    for name, m, dev in (("hip", hip, gpu), ("ref", ref, torch.device("cpu"))):
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        cpu_negatives(9)
        loss = TT.train(m, opt, [_Batch(x) for x in batches], dev)
        st = opt.state[m.user_embedding.weight]
        res[name] = (loss, m.user_embedding.weight.detach().cpu().numpy(), st["exp_avg"].cpu().numpy(),
                     st["exp_avg_sq"].cpu().numpy())
    assert abs(res["hip"][0] - res["ref"][0]) <= 1e-5 * abs(res["ref"][0])
    # three Adam steps: the weights per row within 1e-5 of that row's max |ref| (measured
    # 2e-7). The first moments mix the three steps' gradients, and steps 2 and 3 differentiate at
    # weights that already differ by rounding, so a row whose gradients nearly cancel carries that
    # difference at its own (small) scale: per row within 1e-4 (measured 2.2e-5; the first step's
    # gradients themselves are held to 1e-5 per row by test_first_step_loss_and_grads_match). A
    # row whose moments are exactly 0 on the reference side must be exactly 0 here.
    rw, _ = assert_rows_close(res["hip"][1], res["ref"][1], what="weights after 3 Adam steps")
    rm, _ = assert_rows_close(res["hip"][2], res["ref"][2], rtol=1e-4, what="exp_avg after 3 Adam steps")
    print(f"3 Adam steps: weights row-rel {rw:.3g}, exp_avg row-rel {rm:.3g}")


def test_cluster_training_converges_on_gpu(gpu):
    """End to end: synthetic MovieLens CSV -> handler -> Cluster-GCN loader -> train_model."""
    import tempfile

    from data.dataset_handler import MovieLensDataHandler, write_synthetic_movielens
    from models.light_gcn import LightGCN
    from utils import train_test as TT

    d = tempfile.mkdtemp()
    rp, mp = write_synthetic_movielens(d, 600, 300, 20000, seed=3)
    h = MovieLensDataHandler(rp, mp, device=gpu)
    loader, val, test = h.get_data_training(num_train_clusters=8, clusters_per_batch=2,
                                            indexes_path=d + "/indexes", random_state=0)
    U, I = h.get_num_users_items()
    torch.manual_seed(0)
    model = LightGCN(U, I, num_layers=3, dim_h=32).to(gpu)
    np.random.seed(0)
    _, tr, vl, vr = TT.train_model(model, loader, val, test, gpu, epochs=4, lr=1e-2, checkpoint=None)
    assert all(np.isfinite(tr)) and tr[-1] < tr[0]
    assert all(0.0 <= r <= 1.0 for r in vr)


def test_fused_adam_matches_torch(gpu):
    """FusedAdam(max_grad_norm=1) == clip_grad_norm_(1) + torch Adam, to fp32 rounding."""
    from lgcn_amd.optim import FusedAdam

    torch.manual_seed(0)
    shapes = [(1000, 64), (333, 64), (7, 3)]
    a = [torch.randn(s, device=gpu) * 0.01 for s in shapes]
    b = [t.clone() for t in a]
    pa = [torch.nn.Parameter(t) for t in a]
    pb = [torch.nn.Parameter(t) for t in b]
    oa = torch.optim.Adam(pa, lr=1e-3)
    ob = FusedAdam(pb, lr=1e-3, max_grad_norm=1)
    for step in range(6):
        scale = 10.0 if step % 2 == 0 else 0.01  # clipping active / inactive
        gs = [torch.randn(s, device=gpu) * scale for s in shapes]
        for p, g in zip(pa, gs):
            p.grad = g.clone()
        for p, g in zip(pb, gs):
            p.grad = g.clone()
        norm = torch.nn.utils.clip_grad_norm_(pa, max_norm=1)
        oa.step()
        ob.step()
        assert abs(ob.last_norm[0].item() - norm.item()) <= 1e-5 * norm.item()
        for x, y in zip(pa, pb):
            assert torch.allclose(x.grad, y.grad, rtol=1e-5, atol=1e-9)
            assert (x - y).abs().max().item() <= 1e-6 * max(1.0, x.abs().max().item()) + 1e-8


@pytest.mark.parametrize("K,d,cluster", [(3, 64, False), (2, 128, False), (1, 32, False), (3, 64, True),
                                         (1, 64, True), (4, 128, True)])
def test_fused_train_step_matches_autograd(gpu, K, d, cluster):
    """lgcn_amd.train_step (no autograd: fused BPR kernel + sorted scatter + sparse HIP backward) ==
    the reference harness on the HIP model with autograd, same negatives (same CUDA seed).
    cluster=True: the batch is one Cluster-GCN part of 8, so most rows (and most negatives) are
    untouched by the batch edges — the sparse-plan paths."""
    from lgcn_amd.train_step import FusedTrainStep
    from models.light_gcn import LightGCN
    from utils import train_test as TT

    import graphs

    U, I, ei = graphs.subsampled(U=400, I=250, pairs=5000, seed=K)
    if cluster:
        from lgcn_amd import cluster as C

        part = C.partition_nodes(ei, U + I, 8)
        ei = C.intra_part_edges(ei, part, 8)[3]
        assert 0 < ei.shape[1] < 0.3 * 5000
    torch.manual_seed(1)
    a = LightGCN(U, I, num_layers=K, dim_h=d).to(gpu)
    b = LightGCN(U, I, num_layers=K, dim_h=d).to(gpu)
    b.load_state_dict(a.state_dict())
    batch = _Batch(torch.from_numpy(ei).to(gpu))
    torch.cuda.manual_seed(7)
    loss_ref = TT.bpr_loss(*TT.compute_embeddings(a, batch, gpu))
    loss_ref.backward()
    step = FusedTrainStep(b, optimizer=None)
    torch.cuda.manual_seed(7)
    loss = step.compute_grads(batch)
    assert abs(loss.item() - loss_ref.item()) <= 2e-6 * max(1.0, abs(loss_ref.item()))
    for wa, wb in ((a.user_embedding.weight, b.user_embedding.weight), (a.item_embedding.weight, b.item_embedding.weight)):
        ga, gb = wa.grad.cpu().numpy(), wb.grad.cpu().numpy()
        assert np.abs(ga - gb).max() <= 1e-5 * np.abs(ga).max()
        # and row by row, each row against its own max: a wrong small row does not hide behind the
        # table's largest. Both sides are float32 runs, so both round: the worst row measured on an
        # MI355X is 5.3e-7 of its max (the six cases, both tables; rows autograd leaves exactly 0,
        # up to 351 of 400 users in the cluster cases, are exactly 0 here), held with 4x headroom.
        assert_rows_close(gb, ga, rtol=2.2e-6, what="fused step gradient rows")


def test_fused_train_step_deterministic(gpu):
    from lgcn_amd.train_step import FusedTrainStep
    from models.light_gcn import LightGCN

    import graphs

    U, I, ei = graphs.sym()
    torch.manual_seed(1)
    m = LightGCN(U, I, num_layers=3, dim_h=64).to(gpu)
    step = FusedTrainStep(m, optimizer=None)
    batch = _Batch(torch.from_numpy(ei).to(gpu))
    res = []
    for _ in range(2):
        torch.cuda.manual_seed(3)
        step.compute_grads(batch)
        res.append((m.user_embedding.weight.grad.clone(), m.item_embedding.weight.grad.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_graph_replay_equals_eager(gpu):
    """A hipGraph-replayed fused step (capturable FusedAdam) == the eager fused step, bitwise,
    given the same CUDA seed before each step."""
    from lgcn_amd import cluster as C
    from lgcn_amd.optim import FusedAdam
    from lgcn_amd.train_step import FusedTrainStep
    from models.light_gcn import LightGCN

    import graphs

    U, I, ei = graphs.subsampled(U=500, I=300, pairs=6000, seed=4)
    part = C.partition_nodes(ei, U + I, 4)
    batches = [_Batch(torch.from_numpy(x).to(gpu)) for x in C.intra_part_edges(ei, part, 4)]
    res = []
    for use_graphs in (False, True):
        torch.manual_seed(0)
        m = LightGCN(U, I, num_layers=3, dim_h=64).to(gpu)
        opt = FusedAdam(m.parameters(), lr=1e-2, max_grad_norm=1, capturable=True)
        step = FusedTrainStep(m, opt, graphs=use_graphs)
        losses = []
        for i in range(12):
            torch.cuda.manual_seed(100 + i)
            losses.append(step.step(batches[i % 4]).item())
        res.append((losses, m.user_embedding.weight.detach().clone(), m.item_embedding.weight.detach().clone()))
    assert res[0][0] == res[1][0]
    assert torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])


@pytest.mark.parametrize("clip,d,betas", [(None, 64, (0.9, 0.999)), (1.0, 64, (0.9, 0.999)),
                                           (None, 128, (0.8, 0.99)), (None, 512, (0.9, 0.999))])
def test_row_lazy_adam_matches_dense_fused_adam(gpu, clip, d, betas):
    """RowLazyAdam (deferred rows replayed when touched, flush at the end) == dense
    FusedAdam(capturable=True) on the same sparse gradients: bitwise without clipping (the
    replays are the dense kernel's arithmetic with its per-step constants); with clipping the
    norm is summed over other rows in another order, so to fp32 rounding of the clip coef. betas
    (0.8, 0.99): the step-constant division takes the IEEE division instead of the Markstein
    shortcut (proven for beta2 = 0.999 only); d = 512: two float4 per lane."""
    from lgcn_amd.optim import FusedAdam, RowLazyAdam

    U, I = 300, 200
    N = U + I
    torch.manual_seed(0)
    w0 = [torch.randn(U, d, device=gpu) * 0.1, torch.randn(I, d, device=gpu) * 0.1]
    dense = [torch.nn.Parameter(t.clone()) for t in w0]
    lazy = [t.clone() for t in w0]
    od = FusedAdam(dense, lr=1e-2, betas=betas, max_grad_norm=clip, capturable=True)
    ol = RowLazyAdam(lazy[0], lazy[1], lr=1e-2, betas=betas, max_grad_norm=clip)
    rng = np.random.default_rng(1)
    for step in range(15):
        rows = np.unique(rng.integers(0, N, rng.integers(1, 120)))
        negs = rng.integers(0, I, 40)  # list b: item ids, duplicates and overlaps allowed
        gfull = torch.zeros(N, d, device=gpu)
        live = np.unique(np.concatenate([rows, negs + U]))
        gfull[torch.from_numpy(live).to(gpu)] = torch.randn(len(live), d, device=gpu) * (3.0 if step % 3 else 0.05)
        dense[0].grad, dense[1].grad = gfull[:U].clone(), gfull[U:].clone()
        ra = torch.from_numpy(rows.astype(np.int32)).to(gpu)
        nb = torch.from_numpy(negs).to(gpu)
        ol.catch_up(ra, nb, U)
        ol.gu.copy_(gfull[:U])
        ol.gi.copy_(gfull[U:])
        first = np.zeros(len(negs), np.uint8)
        _, idx = np.unique(negs, return_index=True)
        first[idx] = 1
        skip = np.zeros(N, np.uint8)
        skip[rows] = 1
        ol.step_rows(ra, nb, U, first_b=torch.from_numpy(first).to(gpu), skip_b=torch.from_numpy(skip).to(gpu))
        od.step()
    ol.flush()
    for a, b in zip(dense, lazy):
        if clip is None:
            assert torch.equal(a.detach(), b)
        else:
            assert (a.detach() - b).abs().max().item() <= 1e-6 * a.abs().max().item()


@pytest.mark.parametrize("d", [64, 128])
def test_row_lazy_adam_long_gaps_bitwise_dense(gpu, d):
    """Rows left untouched for ~300 steps are bitwise the dense FusedAdam after their catch-up and
    the flush: the zero-gradient replays take csrc/lgcn_exact.h's shortened sqrt / division only
    while a per-row bound keeps |m| >= 2^-40 and v >= 2^-96, and the full sequences after. The
    rows are chosen to cross that bound mid-replay (touched at the first and last step only: |m|
    from ~1e-3 decays by 0.9 a step, past 2^-40 after ~200 steps; a flush at step 160 splits the
    gap), to start below it (first gradient ~1e-14: |m| ~1e-15), to stay at exact zero (no
    nonzero gradient ever), and to be touched every step or at random."""
    from lgcn_amd.optim import FusedAdam, RowLazyAdam

    U, I = 40, 24
    N = U + I
    torch.manual_seed(3)
    w0 = [torch.randn(U, d, device=gpu) * 0.1, torch.randn(I, d, device=gpu) * 0.1]
    dense = [torch.nn.Parameter(t.clone()) for t in w0]
    lazy = [t.clone() for t in w0]
    od = FusedAdam(dense, lr=1e-2, max_grad_norm=None, capturable=True)
    ol = RowLazyAdam(lazy[0], lazy[1], lr=1e-2, max_grad_norm=None, max_steps=1024)
    rng = np.random.default_rng(2)
    steps = 320
    scale = np.ones(N)
    scale[0:10] = 1e-2      # ordinary rows
    scale[10:20] = 1e-14    # |m| below the fast range from the start
    scale[20:24] = 0.0      # never a nonzero gradient: m = v = 0 throughout
    busy = np.array([30, 31, U + 3, U + 4])  # touched every step
    for step in range(steps):
        if step == 0 or step == steps - 1:
            rows = np.arange(N)
        else:
            rows = np.unique(np.concatenate([busy, rng.integers(24, N, 3)]))  # rows 0..23 idle
        gfull = torch.zeros(N, d, device=gpu)
        gr = torch.randn(len(rows), d, device=gpu) * torch.from_numpy(scale[rows]).float().to(gpu)[:, None]
        gfull[torch.from_numpy(rows).to(gpu)] = gr
        dense[0].grad, dense[1].grad = gfull[:U].clone(), gfull[U:].clone()
        ra = torch.from_numpy(rows.astype(np.int32)).to(gpu)
        ol.catch_up(ra)
        ol.gu.copy_(gfull[:U])
        ol.gi.copy_(gfull[U:])
        ol.step_rows(ra)
        od.step()
        if step == steps // 2:  # a mid-run flush: every row current, then the gaps resume
            ol.flush()
            for a, b in zip(dense, lazy):
                assert torch.equal(a.detach(), b)
    ol.flush()
    for a, b in zip(dense, lazy):
        assert torch.equal(a.detach(), b)


@pytest.mark.parametrize("use_graphs,clip,whole", [(False, float("inf"), False), (True, float("inf"), False),
                                                   (False, 1e6, False), (True, 1e6, True), (False, 1.0, False)])
def test_lazy_train_step_matches_dense_step(gpu, use_graphs, clip, whole):
    """FusedTrainStep(lazy=True) + RowLazyAdam == FusedTrainStep + dense capturable FusedAdam on
    the same Cluster-GCN batches and negatives. Whenever the clip coefficient is exactly 1 —
    no clipping (max_norm = inf), or a finite max_norm the norm stays under (1e6: the norm and
    clamp run on both sides) — bitwise, every loss and every parameter (eager and
    hipGraph-replayed). With an active clip_grad_norm_(1) the two norms sum the same squares in
    different orders, so the coefficients can differ in their last bit: after ONE step (same
    gradients, coefficient off by <= 1 ulp) the parameters agree per row to 1e-5 of the row's
    scale; over 20 steps the losses agree to 1e-5 (the parameters then drift apart where Adam's
    sign-like step meets noise-level gradients; that drift is printed, not asserted)."""
    from lgcn_amd import cluster as C
    from lgcn_amd.optim import FusedAdam, RowLazyAdam
    from lgcn_amd.train_step import FusedTrainStep
    from models.light_gcn import LightGCN

    import graphs

    U, I, ei = graphs.subsampled(U=2000, I=1000, pairs=8000, seed=4)
    part = C.partition_nodes(ei, U + I, 8)
    batches = [_Batch(torch.from_numpy(x).to(gpu)) for x in C.intra_part_edges(ei, part, 8)]
    assert all(2 * int((b.edge_index[0] < U).sum()) <= U + I for b in batches)
    if whole:  # one batch = the whole graph: 2B > N (big intra-part batches of structured graphs)
        batches = [_Batch(torch.from_numpy(ei).to(gpu))] * 8
        assert 2 * int((batches[0].edge_index[0] < U).sum()) > U + I
    res, first = [], []
    for lazy in (False, True):
        torch.manual_seed(0)
        m = LightGCN(U, I, num_layers=3, dim_h=64).to(gpu)
        if lazy:
            opt = RowLazyAdam(m.user_embedding.weight.data, m.item_embedding.weight.data, lr=1e-2,
                              max_grad_norm=clip)
        else:
            opt = FusedAdam(m.parameters(), lr=1e-2, max_grad_norm=clip, capturable=True)
        step = FusedTrainStep(m, opt, graphs=use_graphs, lazy=lazy)
        losses = []
        for i in range(20):
            torch.cuda.manual_seed(100 + i)
            losses.append(step.step(batches[i % 8]).item())
            if i == 0:
                step.sync()
                first.append((m.user_embedding.weight.detach().cpu().numpy().copy(),
                              m.item_embedding.weight.detach().cpu().numpy().copy()))
        step.sync()
        res.append((losses, m.user_embedding.weight.detach().clone(), m.item_embedding.weight.detach().clone()))
    if clip != 1.0:
        assert res[0][0] == res[1][0]
        assert torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])
        return
    for name, a, b in zip(("user", "item"), first[0], first[1]):
        assert_rows_close(b, a, what=f"{name} table after one clipped step")
    for a, b in zip(res[0][0], res[1][0]):
        assert abs(a - b) <= 1e-5 * max(1.0, abs(a))
    for name, x, y in (("user", res[0][1], res[1][1]), ("item", res[0][2], res[1][2])):
        print(f"clip 1, 20 steps: {name} table max |dense - lazy| = {(x - y).abs().max().item():.3g} "
              f"of max |w| {x.abs().max().item():.3g}")


def test_recall20_parity_after_training(gpu, cpu_negatives):
    """BASELINE.json: Recall@20 within ±0.002 of the reference. The reference harness
    (utils/train_test.py train + evaluate) trains the HIP model on the GPU and the oracle model
    (PyG 2.4.0 LGConv restated, oracle/lgconv_torch.py) on the CPU for 5 epochs over the
    golden Cluster-GCN batches, same negatives; then Recall@20 and Recall@100 on the golden
    validation edges with the same numpy seed. A path check of the reference harness on the
    golden 300 x 200 graph, not Recall evidence: its validation set is a few hundred edges, so one
    hit moves Recall by ~0.002 (measured 0.0018 / 0.0013 at k = 20 / 100 — a hit or two). The
    Recall parity evidence is test_recall_parity_c1_size (BASELINE configs[0]'s size) and the
    data-parallel comparison in tests/test_gpu_dp_recall.py; with identical embeddings the hit
    counts are exact (tests/test_gpu_recall.py)."""
    from utils import train_test as TT

    hip, ref = _models(gpu)
    batches = [torch.from_numpy(G[f"train_batch{p}"]) for p in range(3)]
    val = torch.from_numpy(G["val_edge_index"])
    out = {}
    for name, m, dev in (("hip", hip, gpu), ("ref", ref, torch.device("cpu"))):
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)  # the reference's learning rate
        cpu_negatives(21)
        for _ in range(5):
            TT.train(m, opt, [_Batch(x) for x in batches], dev)
        with torch.no_grad():
            embs = TT.compute_embeddings(m, _Batch(val).to(dev), dev)
            rec = {}
            for k in (20, 100):
                np.random.seed(5)
                rec[k] = TT.compute_recall_at_k((embs[1], embs[3], embs[5]), k=k)
        out[name] = rec
    for k in (20, 100):
        assert abs(out["hip"][k] - out["ref"][k]) <= 0.002, (k, out)  # BASELINE.json north star


def test_recall_parity_c1_size(gpu, tune):
    """Recall parity at BASELINE configs[0]'s size (tests/c1_harness.py: 4 Cluster-GCN parts, one per
    step, 5 epochs of the reference harness, the same CPU-drawn negatives on both sides): the HIP
    model trained on the GPU (the fused harness step) against the oracle model on the CPU.

    * Training: the two tables give the SAME Recall through one scorer — both scored by the CPU
      reference formula, and both by the GPU path — equal to the bit.
    * End to end (GPU evaluate vs CPU reference evaluate): with recall_ties="cpu" (CPU torch.topk's
      choice among equal scores) the GPU Recall equals the CPU reference's; the bar is VERDICT r5's
      max(1e-3 relative, 2 x the oracle's own spread under a second summation order), the spread
      measured here (tests/test_noise_floor.py: 0 at this size).
    * The default tie rule ("index", torch.topk on a GPU): scored against the oracle tables through
      the same rule, the same bar; against the CPU reference it differs by the tie rule alone
      (validation candidates repeat: ~8 rows per item), held to the north star's +-0.002."""
    import c1_harness as C
    from parity import record_stats

    cpu = torch.device("cpu")
    data = C.c1_data()
    init = C.init_state()
    m_ref, gs, _ = C.train_c1(cpu, data=data, init=init)
    w_ref = C.tables(m_ref)
    m_hip, gs_hip, path = C.train_c1(gpu, data=data, init=init)
    assert path == "fused", path
    assert torch.equal(gs_hip, gs)  # the same negatives
    w_hip = C.tables(m_hip)
    m_2, gs_2, _ = C.train_c1(cpu, order_seed=1, data=data, init=init)
    ref_cpu = C.recall(w_ref, cpu, gs, data=data)
    spread = {k: abs(C.recall(C.tables(m_2), cpu, gs, data=data)[k] - ref_cpu[k]) for k in (20, 100)}
    bar = {k: max(1e-3 * ref_cpu[k], 2 * spread[k]) for k in (20, 100)}
    hip_cpu_scored = C.recall(w_hip, cpu, gs, data=data)
    tune(recall_ties="cpu")
    hip_cpu_ties = C.recall(w_hip, gpu, gs, data=data)
    ref_cpu_ties = C.recall(w_ref, gpu, gs, data=data)
    tune(recall_ties="index")
    hip_index = C.recall(w_hip, gpu, gs, data=data)
    ref_index = C.recall(w_ref, gpu, gs, data=data)
    stats = {"oracle_cpu": ref_cpu, "spread": spread, "bar": bar, "hip_scored_on_cpu": hip_cpu_scored,
             "hip_gpu_cpu_ties": hip_cpu_ties, "oracle_gpu_cpu_ties": ref_cpu_ties, "hip_gpu_index": hip_index,
             "oracle_gpu_index": ref_index}
    record_stats("recall_parity_c1", stats)
    for k in (20, 100):
        print(f"C1 Recall@{k}: oracle (CPU) {ref_cpu[k]:.8f}; HIP tables scored on CPU {hip_cpu_scored[k]:.8f}; "
              f"GPU evaluate, cpu ties {hip_cpu_ties[k]:.8f}; index ties {hip_index[k]:.8f} vs oracle tables "
              f"{ref_index[k]:.8f}; noise floor {spread[k]:.2e}, bar {bar[k]:.2e}")
        assert hip_cpu_scored[k] == ref_cpu[k], (k, stats)  # training: same Recall through one scorer
        assert ref_cpu_ties[k] == ref_cpu[k], (k, stats)    # the GPU scorer with CPU ties == the CPU scorer
        assert abs(hip_cpu_ties[k] - ref_cpu[k]) <= bar[k], (k, stats)
        assert abs(hip_index[k] - ref_index[k]) <= bar[k], (k, stats)
        assert abs(hip_index[k] - ref_cpu[k]) <= 0.002, (k, stats)  # BASELINE.json north star


@pytest.mark.parametrize("lazy,grouping", [(False, "count"), (True, "count"), (True, "radix")])
def test_sorted_negatives_path_bitwise_range_path(gpu, tune, lazy, grouping):
    """The large-B negatives path (the keys grouped by row — lgcn_group_keys, or one radix sort
    with tuning neg_grouping="radix" — then lgcn_sorted_scatter_add, taken from
    sorted_scatter_min_b triplets) gives bitwise the range-scatter path's losses and
    parameters over 12 hipGraph-replayed steps (dense FusedAdam and row-lazy Adam)."""
    tune(neg_grouping=grouping)
    from lgcn_amd import cluster as C
    from lgcn_amd.optim import FusedAdam, RowLazyAdam
    from lgcn_amd.train_step import FusedTrainStep
    from models.light_gcn import LightGCN

    import graphs

    U, I, ei = graphs.subsampled(U=2000, I=1000, pairs=8000, seed=4)
    part = C.partition_nodes(ei, U + I, 4)
    batches = [_Batch(torch.from_numpy(x).to(gpu)) for x in C.intra_part_edges(ei, part, 4)]
    batches.append(_Batch(torch.from_numpy(ei).to(gpu)))  # one 2B > N batch
    res = []
    for min_b in (1000000000, 1):
        tune(sorted_scatter_min_b=min_b)
        torch.manual_seed(0)
        m = LightGCN(U, I, num_layers=3, dim_h=64).to(gpu)
        if lazy:
            opt = RowLazyAdam(m.user_embedding.weight.data, m.item_embedding.weight.data, lr=1e-2, max_grad_norm=1.0)
        else:
            opt = FusedAdam(m.parameters(), lr=1e-2, max_grad_norm=1.0, capturable=True)
        step = FusedTrainStep(m, opt, graphs=True, lazy=lazy)
        losses = []
        for i in range(12):
            torch.cuda.manual_seed(50 + i)
            losses.append(step.step(batches[i % len(batches)]).item())
        step.sync()
        st = step.state(batches[-1].edge_index)
        assert (st.neg_rowptr is not None) == (min_b == 1)
        res.append((losses, m.user_embedding.weight.detach().clone(), m.item_embedding.weight.detach().clone()))
    assert res[0][0] == res[1][0]
    assert torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])


@pytest.mark.parametrize("min_b,clip,graphs_on", [(1000000000, 1.0, True), (1000000000, None, False),
                                                   (1, 1.0, True), (1, None, True)])
def test_reg_rows_in_update_bitwise_separate_passes(gpu, tune, min_b, clip, graphs_on):
    """ABI 10: the single-GPU lazy step forms the BPR reg-gradient rows inside the clip norm and the
    Adam update from their occurrence counts (lgcn_row_grad_norm_reg / lgcn_row_adam_reg; the range
    scatter writes the negatives' counts, the sorted path's grouping has them) instead of adding them
    to g in two passes after the backward. Bitwise the separate passes — losses, tables, Adam
    moments and clip norms — over 12 steps on the range and the sorted negatives paths, an active
    clip (the norm sums the same squares in the same order) and none, eager and hipGraph-replayed,
    including a 2B > N batch."""
    from lgcn_amd import cluster as C
    from lgcn_amd.optim import RowLazyAdam
    from lgcn_amd.train_step import FusedTrainStep
    from models.light_gcn import LightGCN

    import graphs

    U, I, ei = graphs.subsampled(U=2000, I=1000, pairs=8000, seed=4)
    part = C.partition_nodes(ei, U + I, 4)
    batches = [_Batch(torch.from_numpy(x).to(gpu)) for x in C.intra_part_edges(ei, part, 4)]
    batches.append(_Batch(torch.from_numpy(ei).to(gpu)))  # one 2B > N batch
    tune(sorted_scatter_min_b=min_b)
    res = []
    for in_update in (False, True):
        tune(reg_in_update=in_update)
        torch.manual_seed(0)
        m = LightGCN(U, I, num_layers=3, dim_h=64).to(gpu)
        opt = RowLazyAdam(m.user_embedding.weight.data, m.item_embedding.weight.data, lr=1e-2, max_grad_norm=clip)
        step = FusedTrainStep(m, opt, graphs=graphs_on, lazy=True)
        assert step.reg_in_update == in_update
        losses, norms = [], []
        for i in range(12):
            torch.cuda.manual_seed(50 + i)
            losses.append(step.step(batches[i % len(batches)]).item())
            norms.append(opt.last_norm.cpu().clone())
        step.sync()
        st = step.state(batches[0].edge_index)
        assert (st.neg_rowptr is not None) == (min_b == 1)
        res.append((losses, norms, [t.detach().clone() for t in (m.user_embedding.weight, m.item_embedding.weight,
                                                                   *opt.m, *opt.v)]))
    assert res[0][0] == res[1][0]
    assert all(torch.equal(a, b) for a, b in zip(res[0][1], res[1][1]))
    for a, b in zip(res[0][2], res[1][2]):
        assert torch.equal(a, b)


def test_reg_rows_in_update_unfused_loss_batch(gpu, tune):
    """The counted range scatter without the fused loss (LGCN_LOSS_FUSED_MAX_B <= B < the sorted
    path's threshold: lgcn_range_scatter_add_counts with terms = NULL, the loss in its own launch):
    bitwise the separate reg passes over 4 captured steps."""
    from lgcn_amd import _ffi, synth
    from lgcn_amd.optim import RowLazyAdam
    from lgcn_amd.train_step import FusedTrainStep, loss_fused
    from models.light_gcn import LightGCN

    U, I = 30000, 8000
    g = synth.bipartite(U, I, 20000, seed=5)
    batch = _Batch(torch.from_numpy(g.edge_index).to(gpu))
    res = []
    for in_update in (False, True):
        tune(reg_in_update=in_update)
        torch.manual_seed(0)
        m = LightGCN(U, I, num_layers=3, dim_h=64).to(gpu)
        opt = RowLazyAdam(m.user_embedding.weight.data, m.item_embedding.weight.data, lr=1e-2, max_grad_norm=1.0)
        step = FusedTrainStep(m, opt, graphs=True, lazy=True)
        losses = []
        for i in range(4):
            torch.cuda.manual_seed(90 + i)
            losses.append(step.step(batch).item())
        step.sync()
        st = step.state(batch.edge_index)
        assert st.neg_rowptr is None and st.B >= _ffi.LOSS_FUSED_MAX_B and not loss_fused(st, I)
        res.append((losses, m.user_embedding.weight.detach().clone(), m.item_embedding.weight.detach().clone()))
    assert res[0][0] == res[1][0]
    assert torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])


@pytest.mark.parametrize("lazy", [False, True])
def test_planted_shape_captured_step_bitwise_range_path(gpu, tune, lazy):
    """The captured training step at the planted-graph shape (VERDICT r02 missing #4; the shape
    whose step faulted with the first grouping attempt): one batch of B = 180,000 (user, item)
    pairs over the full ML-25M id space (U = 162,541, I = 59,047; 2B = 360k > N = 221,588), K = 3,
    d = 128, every step after the first replayed from its hipGraph. The sorted path with the
    counting-sort grouping (the default from 49,152 triplets) and with the radix sort give bitwise
    the range-scatter path's losses and tables."""
    from lgcn_amd import synth
    from lgcn_amd.optim import FusedAdam, RowLazyAdam
    from lgcn_amd.train_step import FusedTrainStep
    from models.light_gcn import LightGCN

    U, I = synth.ML25M_USERS, synth.ML25M_ITEMS
    g = synth.bipartite(U, I, 180000, seed=11)
    batch = _Batch(torch.from_numpy(g.edge_index).to(gpu))
    B = int((g.edge_index[0] < U).sum())
    assert 2 * B > U + I
    res = []
    for min_b, grouping in ((1000000000, "count"), (1, "count"), (1, "radix")):
        tune(sorted_scatter_min_b=min_b, neg_grouping=grouping)
        torch.manual_seed(0)
        m = LightGCN(U, I, num_layers=3, dim_h=128).to(gpu)
        if lazy:
            opt = RowLazyAdam(m.user_embedding.weight.data, m.item_embedding.weight.data, lr=1e-3, max_grad_norm=1.0)
        else:
            opt = FusedAdam(m.parameters(), lr=1e-3, max_grad_norm=1.0, capturable=True)
        step = FusedTrainStep(m, opt, graphs=True, lazy=lazy)
        losses = []
        for i in range(5):
            torch.cuda.manual_seed(70 + i)
            losses.append(step.step(batch).item())
        step.sync()
        st = step.state(batch.edge_index)
        assert (st.neg_rowptr is not None) == (min_b == 1)
        if st.neg_rowptr is not None:
            assert int(st.neg_err.item()) == 0
            assert int(st.neg_rowptr[-1].item()) == B
        res.append((losses, m.user_embedding.weight.detach().clone(), m.item_embedding.weight.detach().clone()))
        del step, opt, m
        torch.cuda.synchronize()
    for other in res[1:]:
        assert other[0] == res[0][0]
        assert torch.equal(other[1], res[0][1]) and torch.equal(other[2], res[0][2])

