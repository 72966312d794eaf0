"""The row-exchange kernels of csrc/lgcn_exchange.hip called directly through the C ABI and held
bitwise to the sequential restatement of their contracts in tests/owner_checker.py: the
owner-sharded family (lgcn_owner_reset, lgcn_owner_pack_rows, lgcn_owner_pack_requests,
lgcn_rows_gather in both modes, lgcn_rows_mark), the replicated family's edges, and one
owner-sharded step of W simulated ranks in one process (the all_to_alls are transposes).

Every output buffer is an interior view of a larger allocation pre-filled with NaN (floats), -7
(ints) or 7 (bytes); Buf.host() checks the guard on both sides. Send buffers are compared as
whole images: what the contract writes, over the pre-fill everywhere else. The tables are two
allocations (lo, hi) split at U, strictly inside the range of the listed rows."""
import inspect
from collections import namedtuple

import numpy as np
import pytest
import torch

import owner_checker as oc

pytestmark = pytest.mark.gpu

F32 = np.float32
PAD = 16  # guard elements on either side (a multiple of 16 bytes for every dtype used)
FILL = {torch.float32: float("nan"), torch.int64: -7, torch.int32: -7, torch.uint8: 7}
NP = {torch.float32: np.float32, torch.int64: np.int64, torch.int32: np.int32, torch.uint8: np.uint8}
INT_MAX = 2**31 - 1
U, I = 500, 300
N = U + I

Layout = namedtuple("Layout", "world cap rcap d req_off blk")


def layout(world, cap, rcap, d, gap=0, tail=0):
    req_off, blk = oc.block_floats(cap, d, rcap, gap, tail)
    return Layout(world, cap, rcap, d, req_off, blk)


class Buf:
    """n elements of a device allocation pre-filled with the dtype's fill, PAD guard elements on
    either side (lead = PAD + 1: a float32 view 4 bytes off the 16-byte alignment)."""

    def __init__(self, gpu, n, dtype, data=None, lead=PAD):
        self.n, self.lead, self.dtype = int(n), lead, dtype
        self.full = torch.full((lead + self.n + PAD,), FILL[dtype], dtype=dtype, device=gpu)
        self.t = self.full[lead:lead + self.n]
        if data is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(data, NP[dtype]).reshape(-1)))
        self.ptr = self.t.data_ptr()
        assert (self.ptr % 16 == 0) == (lead == PAD)

    def host(self) -> np.ndarray:
        """The view's content, after checking the guards on both sides."""
        h = self.full.cpu().numpy()
        guard = np.concatenate([h[:self.lead], h[self.lead + self.n:]])
        assert guard.tobytes() == np.full(guard.size, FILL[self.dtype], NP[self.dtype]).tobytes(), "guard overwritten"
        return h[self.lead:self.lead + self.n].copy()


class Table:
    """An [n, d] float32 table as two allocations split at row `split`."""

    def __init__(self, gpu, data, split=U):
        data = np.asarray(data, F32)
        self.shape, self.split = data.shape, split
        d = data.shape[1]
        self.lo = Buf(gpu, split * d, torch.float32, data[:split])
        self.hi = Buf(gpu, (data.shape[0] - split) * d, torch.float32, data[split:])
        self.args = (self.lo.ptr, self.hi.ptr, split, d)

    def host(self) -> np.ndarray:
        return np.concatenate([self.lo.host(), self.hi.host()]).reshape(self.shape)


def up(gpu, a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).to(gpu)


def ptr(t):
    return None if t is None else t.data_ptr()


@pytest.fixture(scope="module")
def ffi(gpu):
    from lgcn_amd import _ffi

    return _ffi, _ffi.load(), _ffi.stream_of(gpu)


def same_image(got, want, what):
    assert got.shape == want.shape
    bad = np.flatnonzero(oc.bits(got) != oc.bits(want))
    assert bad.size == 0, f"{what}: {bad.size} floats differ, first at {bad[:8]}"


def owner_reset(ffi, L, send, counts):
    return ffi[1].lgcn_owner_reset(send.ptr, L.world, L.blk, L.cap, L.req_off, L.rcap, counts.ptr, ffi[2])


def pack_rows(ffi, L, tab, rows_a, keys_b, off_b, first_b, skip_b, counts, send, overflow, d=None, blk=None):
    lo, hi, split, dd = tab.args
    return ffi[1].lgcn_owner_pack_rows(lo, hi, split, dd if d is None else d, ptr(rows_a),
                                       0 if rows_a is None else rows_a.numel(), ptr(keys_b),
                                       0 if keys_b is None else keys_b.numel(), off_b, ptr(first_b), ptr(skip_b),
                                       L.world, L.cap, L.blk if blk is None else blk, counts.ptr, send.ptr,
                                       overflow.ptr, ffi[2])


def pack_requests(ffi, L, rows_a, keys_b, off_b, counts, send, mine, overflow, claim, stamp):
    return ffi[1].lgcn_owner_pack_requests(ptr(rows_a), 0 if rows_a is None else rows_a.numel(), ptr(keys_b),
                                           0 if keys_b is None else keys_b.numel(), off_b, L.world, L.rcap, L.blk,
                                           L.req_off, counts.ptr, send.ptr, mine.ptr, overflow.ptr,
                                           None if claim is None else claim.ptr, stamp, ffi[2])


def gather(ffi, tab, ids_ptr, n, rows_ptr, scatter, d=None):
    lo, hi, split, dd = tab.args
    return ffi[1].lgcn_rows_gather(lo, hi, split, dd if d is None else d, ids_ptr, n, rows_ptr, scatter, ffi[2])


# ---- a. lgcn_owner_reset -----------------------------------------------------------------------

@pytest.mark.parametrize("world,cap,rcap,d", [(1, 2, 2, 8), (3, 10, 6, 64), (8, 260, 260, 128), (64, 4, 4, 16),
                                              (8, 70000, 70000, 8)])
def test_owner_reset(gpu, ffi, world, cap, rcap, d):
    """Every gradient-id and request-id slot := -1, counts[0 : 2 * world] := 0; the row area, the
    pad (2 floats before the request ids, 4 or more after) and the counts past 2 * world keep their
    pre-fill. The last case has 1.12 M id slots: the grid-stride loop runs (4096 x 256 threads)."""
    L = layout(world, cap, rcap, d, gap=2, tail=4)
    assert (world, cap) != (8, 70000) or world * (cap + rcap) > 4096 * 256
    send = Buf(gpu, world * L.blk, torch.float32)
    counts = Buf(gpu, 2 * world + 3, torch.int32)
    pre = send.host()
    ffi[0].check(owner_reset(ffi, L, send, counts), "lgcn_owner_reset")
    img = send.host()
    for gid, rows, rid in oc.parse_send(img, world, L.blk, cap, L.req_off, rcap, d):
        assert (gid == -1).all() and (rid == -1).all()
        assert np.isnan(rows).all()
    same_image(img, oc.reset_image(pre, world, L.blk, cap, L.req_off, rcap), "after reset")
    c = counts.host()
    assert (c[:2 * world] == 0).all() and (c[2 * world:] == -7).all()


def test_owner_reset_rejects_bad_layouts(gpu, ffi):
    """E_ARG, and nothing written, for: 65 ranks, odd cap, request ids overlapping the gradient ids,
    odd req_off, a block that is no multiple of 4 floats, a block shorter than its request ids."""
    good = dict(world=3, block_floats=112, cap=10, req_off=100, rcap=6)
    send = Buf(gpu, 65 * 120, torch.float32)
    counts = Buf(gpu, 140, torch.int32)
    pre = send.host()

    def call(**kw):
        a = dict(good, **kw)
        return ffi[1].lgcn_owner_reset(send.ptr, a["world"], a["block_floats"], a["cap"], a["req_off"], a["rcap"],
                                       counts.ptr, ffi[2])

    for bad in (dict(world=65), dict(cap=9), dict(req_off=18), dict(req_off=101, block_floats=116),
                dict(block_floats=114), dict(block_floats=108)):
        assert call(**bad) == ffi[0].E_ARG, bad
        same_image(send.host(), pre, f"rejected {bad}")
        assert (counts.host() == -7).all(), bad
    assert call() == 0  # the layout they were derived from is accepted
    assert (counts.host()[:6] == 0).all()


# ---- b. lgcn_owner_pack_rows -------------------------------------------------------------------

def check_packed(L, img, reset_img, counts, blocks, g, distinct, full=None, owed=None):
    """A send image after reset + pack_rows against the owner blocks; `full`: the destination that
    overflowed (holds exactly cap of the rows in owed, distinct). Returns nothing; asserts."""
    slots = []
    for o, (gid, rows, rid) in enumerate(oc.parse_send(img, L.world, L.blk, L.cap, L.req_off, L.rcap, L.d)):
        ids, vals = oc.block_entries(gid, rows, distinct or o == full, f"destination {o}")
        if o == full:
            assert len(ids) == L.cap and np.isin(ids, owed).all()
            assert counts[o] >= L.cap
        else:
            assert np.array_equal(ids, blocks[o][0]), f"destination {o}"
            assert oc.same_bits(vals, blocks[o][1]), f"destination {o}"
            assert counts[o] == len(ids)
        assert oc.same_bits(vals, g[ids])
        assert (gid[len(ids):] == -1).all() and (rid == -1).all()
        slots.append(gid[:len(ids)])
    same_image(img, oc.packed_image(reset_img, L.world, L.blk, L.cap, L.d, slots, g), "after pack_rows")


@pytest.mark.parametrize("world", [1, 3, 8])
@pytest.mark.parametrize("d", oc.WIDTHS)
def test_owner_pack_rows(gpu, ffi, d, world):
    """reset + pack_rows: every block's valid (id, row) pairs, sorted by id, are the owner blocks
    of the reference (ids equal, rows bitwise g[id]); unused slots, the request ids and the pad
    keep -1 / the pre-fill; overflow stays 0; counts[o] = the block's valid ids. Then without
    first_b (duplicate keys travel) and without skip_b (rows listed on both sides travel twice)."""
    rng = np.random.default_rng(1000 * world + d)
    g = rng.standard_normal((N, d)).astype(F32)
    tab = Table(gpu, g)
    rows_a, keys_b, first_b, skip_b = oc.rank_list(rng, N, I)
    ra, kb, fb, sb = up(gpu, rows_a, np.int32), up(gpu, keys_b, np.int64), up(gpu, first_b, np.uint8), up(gpu, skip_b, np.uint8)
    sizes = []
    for no_first, no_skip in ((False, False), (True, False), (False, True)):
        listed = oc.listed_rows(rows_a, keys_b, U, None if no_first else first_b, None if no_skip else skip_b)
        assert listed.min() < U < listed.max()
        sizes.append(len(listed))
        blocks, _ = oc.owner_blocks(listed, g, world, 0)
        cap = oc.even_capacity(len(b[0]) for b in blocks)
        L = layout(world, cap, 4, d, gap=0, tail=4)
        send = Buf(gpu, world * L.blk, torch.float32)
        counts = Buf(gpu, 2 * world + 3, torch.int32)
        overflow = Buf(gpu, 1, torch.int32, [0])
        reset_img = oc.reset_image(send.host(), world, L.blk, cap, L.req_off, L.rcap)
        ffi[0].check(owner_reset(ffi, L, send, counts), "lgcn_owner_reset")
        ffi[0].check(pack_rows(ffi, L, tab, ra, kb, U, None if no_first else fb, None if no_skip else sb, counts, send,
                               overflow), "lgcn_owner_pack_rows")
        c = counts.host()
        check_packed(L, send.host(), reset_img, c, blocks, g, distinct=not (no_first or no_skip))
        assert (c[world:2 * world] == 0).all() and (c[2 * world:] == -7).all()
        assert overflow.host()[0] == 0
    assert sizes[0] < sizes[1] and sizes[0] < sizes[2]
    same_image(tab.host(), g, "the gradient table")


@pytest.mark.parametrize("d", [8, 64, 512])
def test_owner_pack_rows_overflow(gpu, ffi, d):
    """Destination 1 of 3 is owed cap + 5 rows, the others fewer than cap: overflow & 1; the full
    block holds exactly cap distinct rows of those owed to it, each with its g row; the others are
    complete; the request ids right after the row area and the next block keep their contents
    (the whole image is compared), so nothing went past slot cap - 1."""
    world, cap, full = 3, 10, 1
    rng = np.random.default_rng(d)
    n, split = 120, 60
    g = rng.standard_normal((n, d)).astype(F32)
    tab = Table(gpu, g, split)
    chosen = np.concatenate([rng.permutation(np.arange(o, n, world))[:cap + 5 if o == full else 6] for o in range(world)])
    chosen = rng.permutation(chosen)
    owed = chosen[chosen % world == full]
    assert len(owed) == cap + 5 and owed.min() < split < owed.max()
    hi_rows = chosen[chosen >= split]
    keys_b = hi_rows[::2] - split  # half of the rows past the split come as keys
    rows_a = np.setdiff1d(chosen, keys_b + split).astype(np.int32)
    listed = oc.listed_rows(rows_a, keys_b, split)
    blocks, over = oc.owner_blocks(listed, g, world, cap)
    assert over and sorted(listed.tolist()) == sorted(chosen.tolist())
    L = layout(world, cap, 4, d)  # the request ids start right after the row area
    assert L.req_off == 2 * cap + cap * d
    send = Buf(gpu, world * L.blk, torch.float32)
    counts = Buf(gpu, 2 * world + 3, torch.int32)
    overflow = Buf(gpu, 1, torch.int32, [0])
    reset_img = oc.reset_image(send.host(), world, L.blk, cap, L.req_off, L.rcap)
    ra, kb = up(gpu, rows_a, np.int32), up(gpu, keys_b, np.int64)
    ffi[0].check(owner_reset(ffi, L, send, counts), "lgcn_owner_reset")
    ffi[0].check(pack_rows(ffi, L, tab, ra, kb, split, None, None, counts, send, overflow), "lgcn_owner_pack_rows")
    assert overflow.host()[0] & 1
    check_packed(L, send.host(), reset_img, counts.host(), blocks, g, distinct=True, full=full, owed=owed)


def test_owner_pack_rows_argument_checks(gpu, ffi):
    """Unsupported widths and a send buffer off the 16-byte alignment: E_UNSUPPORTED; a block
    shorter than its ids and rows: E_ARG; an empty list: OK. Nothing is written in any of them."""
    _ffi = ffi[0]
    g = np.random.default_rng(0).standard_normal((8, 1024)).astype(F32)
    tab = Table(gpu, g, 4)
    send = Buf(gpu, 4096, torch.float32)
    off = Buf(gpu, 4096, torch.float32, lead=PAD + 1)
    counts = Buf(gpu, 5, torch.int32, [0, 0, -7, -7, -7])
    overflow = Buf(gpu, 1, torch.int32, [0])
    rows_a = up(gpu, [1, 6], np.int32)
    pre, pre_off = send.host(), off.host()
    L = Layout(1, 2, 0, 64, 0, 4096)
    assert pack_rows(ffi, L, tab, rows_a, None, 0, None, None, counts, send, overflow, d=24) == _ffi.E_UNSUPPORTED
    assert pack_rows(ffi, L, tab, rows_a, None, 0, None, None, counts, send, overflow, d=1024) == _ffi.E_UNSUPPORTED
    assert pack_rows(ffi, L, tab, rows_a, None, 0, None, None, counts, off, overflow, d=64) == _ffi.E_UNSUPPORTED
    assert pack_rows(ffi, L, tab, rows_a, None, 0, None, None, counts, send, overflow, d=64,
                     blk=2 * 66 - 4) == _ffi.E_ARG
    assert pack_rows(ffi, L, tab, None, None, 0, None, None, counts, send, overflow, d=64) == 0
    same_image(send.host(), pre, "send")
    same_image(off.host(), pre_off, "misaligned send")
    assert counts.host().tolist() == [0, 0, -7, -7, -7] and overflow.host()[0] == 0
    # the same call with a supported width and the aligned buffer packs
    _ffi.check(pack_rows(ffi, L, tab, rows_a, None, 0, None, None, counts, send, overflow, d=64), "lgcn_owner_pack_rows")
    assert counts.host()[0] == 2


# ---- c. lgcn_owner_pack_requests ---------------------------------------------------------------
RU, RI = 152, 48  # the dense-batch shape scaled down: many more keys than items
RN = RU + RI


def request_lists(seed, n_b=3000):
    rng = np.random.default_rng(seed)
    rows_a = np.unique(rng.integers(0, RN, 60)).astype(np.int32)
    keys_b = rng.integers(0, RI, n_b).astype(np.int64)
    assert np.intersect1d(rows_a, keys_b + RU).size and rows_a.min() < RU
    return rows_a, keys_b


def check_requested(L, img, reset_img, counts, mine, want, distinct, mine_fill, full=None, owed=None):
    slots = []
    mine = mine.reshape(L.world, L.rcap)
    for o, (gid, rows, rid) in enumerate(oc.parse_send(img, L.world, L.blk, L.cap, L.req_off, L.rcap, L.d)):
        ids = oc.block_requests(rid, distinct or o == full, f"destination {o}")
        if o == full:
            assert len(ids) == L.rcap and np.isin(ids, owed).all()
            assert counts[L.world + o] >= L.rcap
        else:
            assert np.array_equal(ids, want[o]), f"destination {o}"
            assert counts[L.world + o] == len(ids)
        n = len(ids)
        assert np.array_equal(mine[o, :n], rid[:n]), f"mine, destination {o}"
        assert (mine[o, n:] == mine_fill).all(), f"mine past the requests of destination {o}"
        slots.append(rid[:n])
    same_image(img, oc.requested_image(reset_img, L.world, L.blk, L.req_off, slots), "after pack_requests")


@pytest.mark.parametrize("world", [1, 3, 8])
def test_owner_pack_requests_claim(gpu, ffi, world):
    """With claim = -1 and stamp 1: each distinct row once in its owner's request slots, mine equal
    to the send block slot for slot (mine pre-filled -1 as _step_owner does), counts[world + o]
    the requests, counts[0 : world] untouched, claim == stamp exactly on the requested rows. The
    same stamp again (after a reset): nothing. Stamp 2: the full set again, into a mine pre-filled
    with -7, whose unused entries keep it (the kernel does not reset mine)."""
    _ffi = ffi[0]
    rows_a, keys_b = request_lists(world)
    ra, kb = up(gpu, rows_a, np.int32), up(gpu, keys_b, np.int64)
    claim_ref = np.full(RN, -1, np.int32)
    want = oc.requests(rows_a, keys_b, RU, claim_ref, 1, world)
    L = layout(world, 2, oc.even_capacity(len(x) for x in want), 8, gap=0, tail=4)
    send = Buf(gpu, world * L.blk, torch.float32)
    counts = Buf(gpu, 2 * world + 3, torch.int32)
    overflow = Buf(gpu, 1, torch.int32, [0])
    claim = Buf(gpu, RN, torch.int32, np.full(RN, -1))
    mine = Buf(gpu, world * L.rcap, torch.int64, np.full(world * L.rcap, -1))
    reset_img = oc.reset_image(send.host(), world, L.blk, L.cap, L.req_off, L.rcap)
    mark = np.arange(world) + 5

    def run(m, stamp):
        _ffi.check(owner_reset(ffi, L, send, counts), "lgcn_owner_reset")
        counts.t[:world] = torch.from_numpy(mark.astype(np.int32)).to(gpu)
        _ffi.check(pack_requests(ffi, L, ra, kb, RU, counts, send, m, overflow, claim, stamp), "lgcn_owner_pack_requests")
        c = counts.host()
        assert np.array_equal(c[:world], mark) and (c[2 * world:] == -7).all()
        assert overflow.host()[0] == 0
        return c

    c = run(mine, 1)
    m = mine.host()
    check_requested(L, send.host(), reset_img, c, m, want, True, -1)
    for o, (_, _, rid) in enumerate(oc.parse_send(send.host(), world, L.blk, L.cap, L.req_off, L.rcap, L.d)):
        assert np.array_equal(m.reshape(world, L.rcap)[o], rid)  # every slot, the unused ones included
    assert np.array_equal(claim.host(), claim_ref)
    assert set(np.flatnonzero(claim_ref == 1)) == set(np.concatenate(want))
    # the kernel relies on its caller for mine's -1: _step_owner fills it before the call
    from lgcn_amd.train_step import FusedTrainStep

    src = inspect.getsource(FusedTrainStep._step_owner)
    assert 0 <= src.index("ex.mine.fill_(-1)") < src.index("lgcn_owner_pack_requests")

    mine7 = Buf(gpu, world * L.rcap, torch.int64)
    c = run(mine7, 1)
    assert all(len(x) == 0 for x in oc.requests(rows_a, keys_b, RU, claim_ref, 1, world))
    same_image(send.host(), reset_img, "the same stamp again")
    assert (c[world:2 * world] == 0).all() and (mine7.host() == -7).all()
    assert np.array_equal(claim.host(), claim_ref)

    c = run(mine7, 2)
    again = oc.requests(rows_a, keys_b, RU, claim_ref, 2, world)
    assert all(np.array_equal(a, b) for a, b in zip(want, again))
    check_requested(L, send.host(), reset_img, c, mine7.host(), again, True, -7)
    assert np.array_equal(claim.host(), claim_ref)


@pytest.mark.parametrize("world", [1, 3, 8])
def test_owner_pack_requests_without_claim(gpu, ffi, world):
    """claim = NULL: every entry is requested, duplicates included (the multiset per destination)."""
    rows_a, keys_b = request_lists(20 + world, n_b=400)
    ra, kb = up(gpu, rows_a, np.int32), up(gpu, keys_b, np.int64)
    want = oc.requests(rows_a, keys_b, RU, None, 0, world)
    assert sum(len(x) for x in want) == len(rows_a) + len(keys_b)
    L = layout(world, 2, oc.even_capacity(len(x) for x in want), 8, gap=0, tail=4)
    send = Buf(gpu, world * L.blk, torch.float32)
    counts = Buf(gpu, 2 * world + 3, torch.int32)
    overflow = Buf(gpu, 1, torch.int32, [0])
    mine = Buf(gpu, world * L.rcap, torch.int64)
    reset_img = oc.reset_image(send.host(), world, L.blk, L.cap, L.req_off, L.rcap)
    ffi[0].check(owner_reset(ffi, L, send, counts), "lgcn_owner_reset")
    ffi[0].check(pack_requests(ffi, L, ra, kb, RU, counts, send, mine, overflow, None, 0), "lgcn_owner_pack_requests")
    check_requested(L, send.host(), reset_img, counts.host(), mine.host(), want, False, -7)
    assert overflow.host()[0] == 0
    # a claim array with a negative stamp is refused, nothing written
    claim = Buf(gpu, RN, torch.int32, np.full(RN, -1))
    before, cb, mb = send.host(), counts.host(), mine.host()
    assert pack_requests(ffi, L, ra, kb, RU, counts, send, mine, overflow, claim, -1) == ffi[0].E_ARG
    same_image(send.host(), before, "refused call")
    assert np.array_equal(counts.host(), cb) and np.array_equal(mine.host(), mb) and (claim.host() == -1).all()


def test_owner_pack_requests_overflow(gpu, ffi):
    """Destination 1 of 3 is owed rcap + 3 distinct rows (drawn many times): overflow & 2; exactly
    rcap of its request slots are valid, a distinct subset of the rows owed to it; mine agrees
    with the send block on them; the floats after the request ids and the next block are intact."""
    world, rcap, full = 3, 6, 1
    rng = np.random.default_rng(3)
    owed = rng.permutation(np.arange(full, RN, world))[:rcap + 3]
    others = np.concatenate([rng.permutation(np.arange(o, RN, world))[:4] for o in (0, 2)])
    rows = np.concatenate([owed, others])
    hi = rows[rows >= RU]
    assert hi.size and (rows < RU).any()
    rows_a = rows[rows < RU].astype(np.int32)
    keys_b = rng.permutation(np.repeat(hi - RU, 40)).astype(np.int64)
    claim_ref = np.full(RN, -1, np.int32)
    want = oc.requests(rows_a, keys_b, RU, claim_ref, 9, world)
    assert [len(x) for x in want] == [4, rcap + 3, 4]
    L = layout(world, 2, rcap, 8, gap=0, tail=4)
    send = Buf(gpu, world * L.blk, torch.float32)
    counts = Buf(gpu, 2 * world + 3, torch.int32)
    overflow = Buf(gpu, 1, torch.int32, [0])
    claim = Buf(gpu, RN, torch.int32, np.full(RN, -1))
    mine = Buf(gpu, world * rcap, torch.int64)
    ra, kb = up(gpu, rows_a, np.int32), up(gpu, keys_b, np.int64)
    reset_img = oc.reset_image(send.host(), world, L.blk, L.cap, L.req_off, rcap)
    ffi[0].check(owner_reset(ffi, L, send, counts), "lgcn_owner_reset")
    ffi[0].check(pack_requests(ffi, L, ra, kb, RU, counts, send, mine, overflow, claim, 9), "lgcn_owner_pack_requests")
    assert overflow.host()[0] & 2
    check_requested(L, send.host(), reset_img, counts.host(), mine.host(), want, True, -7, full=full, owed=np.sort(owed))
    claim.host()  # guards


def test_owner_pack_requests_grid_stride(gpu, ffi):
    """1.2 M keys over 48 items (more entries than the 4096 x 256 threads of the launch) with a
    claim array: the 48 distinct rows once each. The last 8 items are drawn only past entry
    4096 x 256, where a thread is on its second turn of the loop."""
    world, n_b, once = 3, 1_200_000, 4096 * 256
    assert n_b > once
    rng = np.random.default_rng(4)
    keys_b = np.concatenate([rng.integers(0, RI - 8, once), rng.integers(0, RI, n_b - once)]).astype(np.int64)
    assert np.unique(keys_b[:once]).size == RI - 8 and np.unique(keys_b).size == RI
    kb = up(gpu, keys_b, np.int64)
    rows = np.arange(RU, RN)
    want = [rows[rows % world == o] for o in range(world)]
    L = layout(world, 2, oc.even_capacity(len(x) for x in want), 8, gap=0, tail=4)
    send = Buf(gpu, world * L.blk, torch.float32)
    counts = Buf(gpu, 2 * world + 3, torch.int32)
    overflow = Buf(gpu, 1, torch.int32, [0])
    claim = Buf(gpu, RN, torch.int32, np.full(RN, -1))
    mine = Buf(gpu, world * L.rcap, torch.int64)
    reset_img = oc.reset_image(send.host(), world, L.blk, L.cap, L.req_off, L.rcap)
    ffi[0].check(owner_reset(ffi, L, send, counts), "lgcn_owner_reset")
    ffi[0].check(pack_requests(ffi, L, None, kb, RU, counts, send, mine, overflow, claim, 1), "lgcn_owner_pack_requests")
    check_requested(L, send.host(), reset_img, counts.host(), mine.host(), want, True, -7)
    assert overflow.host()[0] == 0
    c = claim.host()
    assert (c[RU:] == 1).all() and (c[:RU] == -1).all()


# ---- d. lgcn_rows_gather -----------------------------------------------------------------------

@pytest.mark.parametrize("d", oc.WIDTHS)
def test_rows_gather_and_scatter(gpu, ffi, d):
    """gather: out[i] = table[ids[i]] bitwise, -1 slots keep their pre-fill, the table is only
    read; scatter: the listed rows := rows[i], every other row untouched; gather then scatter of
    the same distinct ids is the identity."""
    _ffi = ffi[0]
    rng = np.random.default_rng(d)
    p = rng.standard_normal((N, d)).astype(F32)
    n = 150
    ids = rng.permutation(N)[:n].astype(np.int64)
    ids[rng.permutation(n)[:20]] = -1
    ok = ids >= 0
    assert ids[ok].min() < U < ids[ok].max()
    idt = up(gpu, ids, np.int64)
    tab = Table(gpu, p)
    out = Buf(gpu, n * d, torch.float32)
    _ffi.check(gather(ffi, tab, idt.data_ptr(), n, out.ptr, 0), "lgcn_rows_gather")
    want = np.full((n, d), np.nan, F32)
    want[ok] = p[ids[ok]]
    same_image(out.host().reshape(n, d), want, "gathered rows")
    same_image(tab.host(), p, "the table after a gather")
    # scatter other rows in
    x = rng.standard_normal((n, d)).astype(F32)
    rows = Buf(gpu, n * d, torch.float32, x)
    _ffi.check(gather(ffi, tab, idt.data_ptr(), n, rows.ptr, 1), "lgcn_rows_gather(scatter)")
    q = p.copy()
    q[ids[ok]] = x[ok]
    same_image(tab.host(), q, "the table after a scatter")
    same_image(rows.host().reshape(n, d), x, "the scattered rows")
    # round trip
    back = Buf(gpu, n * d, torch.float32)
    _ffi.check(gather(ffi, tab, idt.data_ptr(), n, back.ptr, 0), "lgcn_rows_gather")
    _ffi.check(gather(ffi, tab, idt.data_ptr(), n, back.ptr, 1), "lgcn_rows_gather(scatter)")
    same_image(tab.host(), q, "the table after gather + scatter")


def test_rows_gather_argument_checks(gpu, ffi):
    _ffi = ffi[0]
    p = np.random.default_rng(1).standard_normal((8, 64)).astype(F32)
    tab = Table(gpu, p, 4)
    ids = up(gpu, [5, 2], np.int64)
    out = Buf(gpu, 2 * 64, torch.float32)
    off = Buf(gpu, 2 * 64, torch.float32, lead=PAD + 1)
    assert gather(ffi, tab, None, 0, None, 0) == 0
    assert gather(ffi, tab, ids.data_ptr(), 0, out.ptr, 1) == 0
    assert gather(ffi, tab, ids.data_ptr(), 2, off.ptr, 0) == _ffi.E_UNSUPPORTED
    assert gather(ffi, tab, ids.data_ptr(), 2, out.ptr, 0, d=24) == _ffi.E_UNSUPPORTED
    assert np.isnan(out.host()).all() and np.isnan(off.host()).all()
    same_image(tab.host(), p, "the table")


# ---- e. lgcn_rows_mark -------------------------------------------------------------------------

def test_rows_mark(gpu, ffi):
    """mask[ids[i]] = value for ids[i] >= 0 (and first[i], if given); -1 ids skipped; the other
    bytes unchanged; marked with 0 and then with 1, an all-ones mask is itself again (the pair of
    calls _owner_reduce makes around the clip norm)."""
    _ffi, lib, s = ffi
    rng = np.random.default_rng(5)
    n = 300
    ids = rng.integers(0, N, n).astype(np.int64)
    ids[rng.permutation(n)[:40]] = -1
    first = (rng.random(n) < 0.5).astype(np.uint8)
    idt, ft = up(gpu, ids, np.int64), up(gpu, first, np.uint8)
    ok = ids >= 0
    assert (first[~ok] == 1).any()  # a -1 id with first set is skipped all the same
    ones = Buf(gpu, N, torch.uint8, np.ones(N))
    _ffi.check(lib.lgcn_rows_mark(idt.data_ptr(), ft.data_ptr(), n, ones.ptr, 0, s), "lgcn_rows_mark")
    want = np.ones(N, np.uint8)
    want[ids[ok & (first == 1)]] = 0
    assert 0 < int((want == 0).sum()) < int(np.unique(ids[ok]).size)
    assert np.array_equal(ones.host(), want)
    _ffi.check(lib.lgcn_rows_mark(idt.data_ptr(), ft.data_ptr(), n, ones.ptr, 1, s), "lgcn_rows_mark")
    assert (ones.host() == 1).all()
    # first = NULL: every non-negative id; over a mask of other bytes
    orig = rng.integers(2, 200, N).astype(np.uint8)
    mask = Buf(gpu, N, torch.uint8, orig)
    _ffi.check(lib.lgcn_rows_mark(idt.data_ptr(), None, n, mask.ptr, 0, s), "lgcn_rows_mark")
    want = orig.copy()
    want[ids[ok]] = 0
    assert np.array_equal(mask.host(), want)
    _ffi.check(lib.lgcn_rows_mark(idt.data_ptr(), None, n, mask.ptr, 1, s), "lgcn_rows_mark")
    want[ids[ok]] = 1
    assert np.array_equal(mask.host(), want)
    assert lib.lgcn_rows_mark(None, None, 0, None, 1, s) == 0
    assert np.array_equal(mask.host(), want)


# ---- f. the replicated kernels' edges ----------------------------------------------------------

def replicated_slots(rng, W, cap, n, d):
    """W ranks' slots over n rows: distinct rows per rank, -1 padded, in a random order."""
    ids_all = np.full(W * cap, -1, np.int64)
    rows_all = rng.standard_normal((W * cap, d)).astype(F32)
    for r in range(W):
        k = int(rng.integers(cap // 2, cap + 1))
        ids_all[r * cap + rng.permutation(cap)[:k]] = rng.permutation(n)[:k]
    return ids_all, rows_all


@pytest.mark.parametrize("d", oc.WIDTHS)
def test_rows_accumulate_without_division(gpu, ffi, d):
    """div = 0.0 leaves the rank-ordered sums undivided; rows outside the union are untouched."""
    _ffi, lib, s = ffi
    W, cap, n, split = 3, 20, 60, 30
    rng = np.random.default_rng(d + 1)
    ids_all, rows_all = replicated_slots(rng, W, cap, n, d)
    first_ref, ref = oc.rank_ordered_mean(ids_all, rows_all, W, cap, 0.0)
    idt = up(gpu, ids_all, np.int64)
    rows = Buf(gpu, W * cap * d, torch.float32, rows_all)
    claim = Buf(gpu, n, torch.int32, np.full(n, INT_MAX))
    first = Buf(gpu, W * cap, torch.uint8)
    _ffi.check(lib.lgcn_rows_mark_first(idt.data_ptr(), W * cap, claim.ptr, first.ptr, s), "lgcn_rows_mark_first")
    assert np.array_equal(first.host(), first_ref) and (claim.host() == INT_MAX).all()
    g = Table(gpu, np.full((n, d), np.nan, F32), split)
    _ffi.check(lib.lgcn_rows_accumulate(idt.data_ptr(), rows.ptr, W, cap, cap * d, first.ptr, g.lo.ptr, g.hi.ptr,
                                        split, d, 0.0, s), "lgcn_rows_accumulate")
    want = np.full((n, d), np.nan, F32)
    for r, v in ref.items():
        want[r] = v
    assert min(ref) < split <= max(ref) and len(ref) < n
    same_image(g.host(), want, "undivided sums")
    same_image(rows.host(), rows_all.reshape(-1), "the rows")


def test_replicated_kernels_argument_checks(gpu, ffi):
    """rank_stride no multiple of 4: E_UNSUPPORTED; rank_stride < cap * d: E_ARG;
    lgcn_rows_mark_first with n = 2^31: E_ARG before any pointer is read; cap = 0 and n = 0: no-ops."""
    _ffi, lib, s = ffi
    W, cap, n, d, split = 2, 4, 12, 8, 6
    rng = np.random.default_rng(7)
    ids_all, rows_all = replicated_slots(rng, W, cap, n, d)
    idt = up(gpu, ids_all, np.int64)
    # room for the widest stride tried, so that a check that let it through would stay in bounds
    rows = Buf(gpu, W * (cap * d + 4), torch.float32, np.resize(rows_all, W * (cap * d + 4)))
    first = Buf(gpu, W * cap, torch.uint8)
    claim = Buf(gpu, n, torch.int32, np.full(n, INT_MAX))
    g = Table(gpu, np.full((n, d), np.nan, F32), split)

    def acc(cap_, stride):
        return lib.lgcn_rows_accumulate(idt.data_ptr(), rows.ptr, W, cap_, stride, first.ptr, g.lo.ptr, g.hi.ptr, split,
                                        d, float(W), s)

    assert acc(cap, cap * d + 2) == _ffi.E_UNSUPPORTED
    assert acc(cap, cap * d - 4) == _ffi.E_ARG
    assert acc(0, 0) == 0
    assert lib.lgcn_rows_mark_first(idt.data_ptr(), 2**31, claim.ptr, first.ptr, s) == _ffi.E_ARG
    assert lib.lgcn_rows_mark_first(idt.data_ptr(), 0, claim.ptr, first.ptr, s) == 0
    assert lib.lgcn_rows_mark_first(None, 0, None, None, s) == 0
    assert np.isnan(g.host()).all() and (first.host() == 7).all() and (claim.host() == INT_MAX).all()
    # accepted: the padded stride that is a multiple of 4
    _ffi.check(lib.lgcn_rows_mark_first(idt.data_ptr(), W * cap, claim.ptr, first.ptr, s), "lgcn_rows_mark_first")
    _ffi.check(acc(cap, cap * d + 4), "lgcn_rows_accumulate")
    rows_h = rows.host().reshape(W, cap * d + 4)[:, :cap * d].reshape(W * cap, d)
    first_ref, ref = oc.rank_ordered_mean(ids_all, rows_h, W, cap, float(W))
    assert np.array_equal(first.host(), first_ref)
    gh = g.host()
    for r, v in ref.items():
        assert oc.same_bits(gh[r], v), r
    assert np.isnan(np.delete(gh, sorted(ref), axis=0)).all()


# ---- g. one simulated owner-sharded step -------------------------------------------------------
SU, SI = 120, 80
SN = SU + SI


@pytest.mark.parametrize("d", [8, 64, 512])
@pytest.mark.parametrize("W", [2, 3, 8])
def test_simulated_owner_step(gpu, ffi, W, d):
    """W ranks in one process, the all_to_alls as transposes of the [W, W, block] buffers: every
    rank resets, packs its gradient rows and its (deduped) requests; every owner unpacks as
    OwnerExchange.unpack does, marks first occurrences, accumulates the rank-ordered mean from the
    received blocks (rank_stride = block) into a NaN table, marks its not-in-union mask and gathers
    the requested parameter rows; every rank scatters the replies through its `mine`.
    The owner's table: bitwise the checker's rank-ordered mean on exactly its rows of the union
    (NaN elsewhere), within 2^-23 * sum |g_r| of the float64 mean; the mask 0 exactly there; each
    rank's table equals P_{row % W}[row] on every row it requested and is unchanged elsewhere."""
    _ffi, lib, s = ffi
    rng = np.random.default_rng(100 * W + d)
    grads = [rng.standard_normal((SN, d)).astype(F32) for _ in range(W)]
    lists = [oc.rank_list(rng, SN, SI, n_a=40, n_b=60) for _ in range(W)]
    listed = [oc.listed_rows(ra, kb, SU, fb, sb) for ra, kb, fb, sb in lists]
    reqs = [(np.unique(rng.integers(0, SN, 40)).astype(np.int32), rng.integers(0, SI, 200).astype(np.int64))
            for _ in range(W)]
    blocks = [oc.owner_blocks(listed[r], grads[r], W, 0)[0] for r in range(W)]
    wanted = [oc.requests(ra, kb, SU, np.full(SN, -1, np.int32), 1, W) for ra, kb in reqs]
    cap = oc.even_capacity(len(b[0]) for bl in blocks for b in bl)
    rcap = oc.even_capacity(len(x) for w in wanted for x in w)
    L = layout(W, cap, rcap, d)  # OwnerExchange's block: no gap, padded to 4 floats
    assert all(x.min() < SU < x.max() for x in listed)

    # 1. every rank packs
    keep, sends, mines = [], [], []
    for r in range(W):
        tab = Table(gpu, grads[r], SU)
        send = Buf(gpu, W * L.blk, torch.float32)
        counts = Buf(gpu, 2 * W, torch.int32)
        overflow = Buf(gpu, 1, torch.int32, [0])
        claim = Buf(gpu, SN, torch.int32, np.full(SN, -1))
        mine = Buf(gpu, W * rcap, torch.int64, np.full(W * rcap, -1))
        dev = [up(gpu, a, t) for a, t in zip(lists[r], (np.int32, np.int64, np.uint8, np.uint8))]
        rq = [up(gpu, reqs[r][0], np.int32), up(gpu, reqs[r][1], np.int64)]
        _ffi.check(owner_reset(ffi, L, send, counts), "lgcn_owner_reset")
        _ffi.check(pack_rows(ffi, L, tab, dev[0], dev[1], SU, dev[2], dev[3], counts, send, overflow),
                   "lgcn_owner_pack_rows")
        _ffi.check(pack_requests(ffi, L, rq[0], rq[1], SU, counts, send, mine, overflow, claim, 1),
                   "lgcn_owner_pack_requests")
        keep.append((tab, counts, overflow, claim, dev, rq))
        sends.append(send)
        mines.append(mine)
    for r in range(W):
        tab, counts, overflow, claim, _, _ = keep[r]
        assert overflow.host()[0] == 0
        c = counts.host()
        assert c[:W].tolist() == [len(b[0]) for b in blocks[r]] and c[W:].tolist() == [len(x) for x in wanted[r]]
        same_image(tab.host(), grads[r], f"rank {r}'s gradient table")
        sends[r].host()  # guards
    # 2. the all_to_all
    recv = torch.stack([b.t for b in sends]).view(W, W, L.blk).transpose(0, 1).contiguous()
    # 3. every owner reduces and replies
    params = [rng.standard_normal((SN, d)).astype(F32) for _ in range(W)]
    listing = [np.isin(np.arange(SN), x) for x in listed]
    mean64, mag = oc.dense_mean64(grads, listing, float(W))
    replies = []
    for o in range(W):
        ro = recv[o]
        ids_all = Buf(gpu, W * cap, torch.int64)
        req_all = Buf(gpu, W * rcap, torch.int64)
        ids_all.t.view(W, cap).copy_(ro[:, :2 * cap].view(torch.int64))
        req_all.t.view(W, rcap).copy_(ro[:, L.req_off:L.req_off + 2 * rcap].view(torch.int64))
        first = Buf(gpu, W * cap, torch.uint8)
        claim = Buf(gpu, SN, torch.int32, np.full(SN, INT_MAX))
        _ffi.check(lib.lgcn_rows_mark_first(ids_all.ptr, W * cap, claim.ptr, first.ptr, s), "lgcn_rows_mark_first")
        g = Table(gpu, np.full((SN, d), np.nan, F32), SU)
        _ffi.check(lib.lgcn_rows_accumulate(ids_all.ptr, ro.data_ptr() + 8 * cap, W, cap, L.blk, first.ptr, g.lo.ptr,
                                            g.hi.ptr, SU, d, float(W), s), "lgcn_rows_accumulate")
        not_union = Buf(gpu, SN, torch.uint8, np.ones(SN))
        _ffi.check(lib.lgcn_rows_mark(ids_all.ptr, first.ptr, W * cap, not_union.ptr, 0, s), "lgcn_rows_mark")
        P = Table(gpu, params[o], SU)
        reply = Buf(gpu, W * rcap * d, torch.float32)
        _ffi.check(gather(ffi, P, req_all.ptr, W * rcap, reply.ptr, 0), "lgcn_rows_gather(replies)")
        replies.append(reply)

        # what arrived: rank r's block for o, whatever its slot order
        ids_h = ids_all.host().reshape(W, cap)
        for r in range(W):
            got, _ = oc.block_entries(ids_h[r], np.zeros((cap, 1), F32), True, f"owner {o}, rank {r}")
            assert np.array_equal(got, blocks[r][o][0])
        _, ref = oc.rank_ordered_mean(*oc.slots_of([blocks[r][o] for r in range(W)], cap, d), W, cap, float(W))
        union = np.unique(np.concatenate(listed))
        mine_rows = union[union % W == o]
        assert sorted(ref) == mine_rows.tolist() and mine_rows.min() < SU < mine_rows.max()
        want = np.full((SN, d), np.nan, F32)
        for row, v in ref.items():
            want[row] = v
        gh = g.host()
        same_image(gh, want, f"owner {o}'s accumulated table")
        err = np.abs(gh[mine_rows].astype(np.float64) - mean64[mine_rows])
        assert (err <= oc.mean_bar(mag[mine_rows])).all(), f"owner {o}: off the float64 mean by {err.max()}"
        assert int(first.host().sum()) == len(mine_rows) and (claim.host() == INT_MAX).all()
        nu = np.ones(SN, np.uint8)
        nu[mine_rows] = 0
        assert np.array_equal(not_union.host(), nu)
        same_image(P.host(), params[o], f"owner {o}'s parameters")
    # 4. the replies travel back
    back = torch.stack([b.t for b in replies]).view(W, W, rcap * d).transpose(0, 1).contiguous()
    for b in replies:
        b.host()  # guards
    # 5. every rank writes the rows it asked for
    for r in range(W):
        t0 = rng.standard_normal((SN, d)).astype(F32)
        T = Table(gpu, t0, SU)
        _ffi.check(gather(ffi, T, mines[r].ptr, W * rcap, back[r].data_ptr(), 1), "lgcn_rows_gather(scatter replies)")
        want = t0.copy()
        asked = np.concatenate(wanted[r])
        assert asked.min() < SU < asked.max() and len(np.unique(asked)) == len(asked)
        for row in asked:
            want[row] = params[row % W][row]
        same_image(T.host(), want, f"rank {r}'s table after the replies")
        m = mines[r].host().reshape(W, rcap)
        for o in range(W):
            assert np.array_equal(np.sort(m[o][m[o] >= 0]), wanted[r][o])
