"""The spectral-norm kernels (csrc/spectral_norm.hip) held to exact values and derived bounds through the C ABI; operands, references,
conditions and the comparison: tests/sn_exact_util.py, checked against itself on the CPU by tests/test_sn_harness.py.

The tables are built with the structs of _lib.py at the offsets, padding and alignment ops.SpectralNormBank._build gives them.  Every
buffer the kernels write lies between canary regions and starts as NaN (the pack arena: 0xFF bytes, a NaN in every storage type): the
scratch, the pack arena, u, v, grads / bias_grads, dot_partials.  After each call whatever the contract does not own is bit-identical
to what it was: scal[2], scal[3] and the padding of the scratch, the gaps between the layers' pack slices, the tails behind grads."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import exact_util as X
import sn_exact_util as S
from semantic_pyramid_for_image_generation_amd import _lib as L, ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16, F16 = S.F32, S.BF16, S.F16
CANARY, PAD, NAN = -1536.0, 64, float("nan")
SP_ERR_INVALID = -1
DT_IDS = [S.NAME[dt] for dt in S.DTYPES]
TABLES = {"ragged": S.RAGGED, "capped": S.CAPPED}
THIRD = float(np.float32(1.0) / np.float32(3.0))


class Guarded:
    """[PAD canaries][n elements = `body`][PAD canaries] on the device; .t is the body (16-byte aligned)."""

    def __init__(self, n, dtype=F32, body=NAN):
        self.n = n
        self.canary = 0xA5 if dtype == torch.uint8 else CANARY
        host = torch.full((PAD + n + PAD,), self.canary, dtype=dtype)
        if isinstance(body, torch.Tensor):
            host[PAD:PAD + n] = body.to(dtype)
        else:
            host[PAD:PAD + n] = body
        self.init = host[PAD:PAD + n].clone()
        self.buf = host.to(DEV)
        self.t = self.buf[PAD:PAD + n]
        assert self.t.data_ptr() % 16 == 0

    def host(self, what):
        h = self.buf.cpu()
        edge = torch.cat((h[:PAD], h[PAD + self.n:]))
        assert bool((edge == self.canary).all()), (what, "a canary next to the buffer was overwritten")
        return h[PAD:PAD + self.n]


def bits(t):
    return t.view(torch.int32) if t.dtype == F32 else t


def untouched(now, init, mask, what):
    """Where `mask` holds, `now` carries the bits of `init`."""
    bad = (bits(now) != bits(init)) & mask
    assert not bool(bad.any()), (what, "%d elements outside what the call owns changed, first at %d" % (int(bad.sum()), int(bad.nonzero()[0])))


class Bank:
    """The operands of a case on the device: W (flat), u and v (guarded), the forward and backward tables."""

    def __init__(self, c):
        self.c, self.lay = c, c.lay
        lay = c.lay
        w, u, v = torch.zeros(lay.w_floats), torch.full((lay.u_floats,), NAN), torch.full((lay.v_floats,), NAN)
        for Lr in c.layers:
            e = Lr.ent
            w[e.w_off:e.w_off + e.rows * e.cols] = Lr.W.float().reshape(-1)
            u[e.u_off:e.u_off + e.rows] = Lr.u0.float()
            v[e.v_off:e.v_off + e.cols] = Lr.v0.float()
        self.w = w.to(DEV)
        self.u, self.v = Guarded(lay.u_floats, F32, u), Guarded(lay.v_floats, F32, v)
        self.table = self.fwd_table()
        btab = (L.SpSnBwdLayer * len(lay.entries))()
        for b, e in zip(btab, lay.entries):
            b.w = self.w.data_ptr() + 4 * e.w_off
            b.dw_off, b.dot_off, b.scratch_off, b.grad_off = e.dw_off, e.dot_off, e.scratch_off, e.grad_off
            b.rows, b.cols, b.cin, b.taps, b.cin_p, b.plain = e.rows, e.cols, e.cin, e.taps, e.cin_p, e.kind
            b.db_off, b.bias_off = e.db_off, e.bias_off
        self.bwd_table = torch.frombuffer(bytearray(bytes(btab)), dtype=torch.uint8).to(DEV)

    def host_table(self, block0=None):
        tab = (L.SpSnLayer * len(self.lay.entries))()
        for i, (t, e) in enumerate(zip(tab, self.lay.entries)):
            t.w = self.w.data_ptr() + 4 * e.w_off
            t.u, t.v = self.u.t.data_ptr() + 4 * e.u_off, self.v.t.data_ptr() + 4 * e.v_off
            assert t.w % 16 == 0 and t.u % 16 == 0 and t.v % 16 == 0 and e.scratch_off % 4 == 0 and e.part_off % 4 == 0
            t.scratch_off, t.part_off, t.fwd_off, t.dgrad_off = e.scratch_off, e.part_off, e.fwd_off, e.dgrad_off
            t.rows, t.cols, t.cin, t.taps, t.cin_p, t.cout_p, t.kind = e.rows, e.cols, e.cin, e.taps, e.cin_p, e.cout_p, e.kind
            assert t.taps <= 9
            t.pack_block0 = e.pack_block0 if block0 is None else block0[i]
        return tab

    def fwd_table(self, block0=None):
        return torch.frombuffer(bytearray(bytes(self.host_table(block0))), dtype=torch.uint8).to(DEV)

    def unpacked_table(self, skip):
        """(device table, pack_blocks) from ops.SpectralNormBank._unpacked_table itself, on a bank that carries this case's table."""
        bank = ops.SpectralNormBank.__new__(ops.SpectralNormBank)
        bank._table_host = self.host_table()
        bank.specs, bank.entries = list(self.lay.entries), [bank._table_host[i] for i in range(len(self.lay.entries))]
        bank.pack_blocks, bank.table_dev = self.lay.pack_blocks, self.table
        return bank._unpacked_table(frozenset(skip))


class Forward:
    """One sp_sn_forward call on a bank: fresh guarded scratch and pack arena, the ownership checks, the per-layer results."""

    def __init__(self, bank, power_iter=True, pack="flat", table=None, blocks=None, packed=None):
        c, lay = bank.c, bank.lay
        self.bank, self.c, self.power_iter = bank, c, power_iter
        self.scratch, self.arena = Guarded(lay.scratch_floats), Guarded(lay.pack_bytes, torch.uint8, 0xFF)
        if blocks is None:
            blocks = lay.pack_blocks if pack == "flat" else 0
        L.call("sp_sn_forward", ops.ptr(table if table is not None else bank.table), len(lay.entries), lay.max_rows, lay.max_cols, lay.max_pack,
               ops.ptr(self.scratch.t), lay.scratch_floats, ops.ptr(self.arena.t), int(power_iter), ops.sp_dtype(c.dtype), blocks, ops.stream())
        torch.cuda.synchronize()
        what = (c.what, "forward")
        self.s, self.a = self.scratch.host(what), self.arena.host(what)
        self.u, self.v = bank.u.host(what), bank.v.host(what)
        own = S.scratch_owned(lay, power_iter)
        untouched(self.s, self.scratch.init, ~own, (what, "scratch"))
        assert not bool(self.s[own].isnan().any()), (what, "a scratch element the call owns was not written")
        self.packed = set(range(len(lay.entries))) if packed is None else packed

    def got(self, i) -> S.Case:
        Lr, dt = self.c.layers[i], self.c.dtype
        e, s = Lr.ent, self.s
        o = e.scratch_off
        g = S.Case(v=s[o:o + e.cols], s=s[o + e.cols:o + e.cols + e.rows], usnap=s[o + e.cols + e.rows:o + e.cols + 2 * e.rows],
                   sigma=s[o + e.cols + 2 * e.rows], inv_sigma=s[o + e.cols + 2 * e.rows + 1],
                   u_out=self.u[e.u_off:e.u_off + e.rows], v_out=self.v[e.v_off:e.v_off + e.cols])
        if self.power_iter:
            g.parts = s[e.part_off:e.part_off + e.slabs * e.cols]
        g.fwd = self.a[e.fwd_off:e.fwd_off + e.fwd_bytes].view(F32 if e.kind else dt)
        g.dgrad = self.a[e.dgrad_off:e.dgrad_off + e.dgrad_bytes].view(dt) if e.dgrad_off >= 0 else None
        return g

    def arena_owned(self):
        """Mask over the arena's bytes of the slices of the layers that were packed."""
        own = torch.zeros(self.a.numel(), dtype=torch.bool)
        for i in self.packed:
            e = self.c.layers[i].ent
            own[e.fwd_off:e.fwd_off + e.fwd_bytes] = True
            if e.dgrad_off >= 0:
                own[e.dgrad_off:e.dgrad_off + e.dgrad_bytes] = True
        return own

    def check(self, parts=None):
        """Every layer's checks, then every byte of the arena outside the packed layers' slices (gaps and skipped slices) unchanged."""
        c, worst = self.c, {}
        for i, Lr in enumerate(c.layers):
            g = self.got(i)
            names = [k for k in Lr.checks if (parts is None or k in parts) and (i in self.packed or k not in ("fwd", "dgrad"))]
            for k in names:
                w = S.compare(Lr, g, (k,))
                if Lr.checks[k][0] == "within":
                    worst[k] = max(worst.get(k, 0.0), w)
        # (the slices are compared as numbers above: a negative sigma - eval mode with any u, v - leaves -0.0 in the padding)
        untouched(self.a, self.arena.init, ~self.arena_owned(), (c.what, "the pack arena between the packed slices"))
        return worst


@functools.lru_cache(maxsize=4)
def built(regime, table, dt, power_iter=True, count=0):
    specs = TABLES[table] if table in TABLES else [S.MANY] * count
    return S.sn_case(regime, specs, dt, 0, power_iter)


def report(tag, worst):
    print("%s: error / bound %s" % (tag, " ".join("%s %.3f" % kv for kv in sorted(worst.items())) or "- (all exact)"))


# ------------------------------------------------------------------------------------------------------------------------------------
# batched backward
# ------------------------------------------------------------------------------------------------------------------------------------
def run_backward(fwd, seed=0, entry="plain", scale=1.0, accumulate=None, bias=True, lo=0, hi=None, zero=()):
    """One batched backward of layers lo .. hi on the snapshots of `fwd`.  accumulate: None | "alias" | "separate"; zero: layers
    whose dW slot stays zero.  Returns the worst error / bound per check."""
    bank, c, lay = fwd.bank, fwd.c, fwd.bank.lay
    hi = len(lay.entries) if hi is None else hi
    g = X.gen(77 + seed)
    arena = torch.zeros(lay.arena_floats)
    ops_in, prev_host = [], torch.full((lay.flat_floats,), NAN)
    for i, Lr in enumerate(c.layers):
        e = Lr.ent
        G, db = S.grad_bias(Lr, g, i not in zero)
        arena[e.dw_off:e.dw_off + e.n_dw] = S.pack_dw(Lr, G)
        arena[e.db_off:e.db_off + e.rows] = db.float()
        pw, pb = X.integers(Lr.W.shape, 16, g), X.integers((e.rows,), 16, g)
        pw[pw == 0] = 5.0
        if lo <= i < hi:
            prev_host[e.grad_off:e.grad_off + e.rows * e.cols] = pw.float().reshape(-1)
            prev_host[e.bias_off:e.bias_off + e.rows] = pb.float()
        ops_in.append((G, db, pw, pb))
    arena_g = Guarded(lay.arena_floats, F32, arena)
    flat = Guarded(lay.flat_floats, F32, prev_host if accumulate == "alias" else NAN)
    prev = flat if accumulate == "alias" else Guarded(lay.flat_floats, F32, prev_host) if accumulate == "separate" else None
    n = hi - lo
    dots = Guarded(n * S.DOT_BLOCKS)
    table = ctypes.c_void_p(bank.bwd_table.data_ptr() + lo * ctypes.sizeof(L.SpSnBwdLayer))
    args = (table, n, lay.max_elems, ops.ptr(arena_g.t), ops.ptr(fwd.scratch.t), ops.ptr(flat.t), ops.ptr(prev.t) if prev else None,
            ops.ptr(flat.t) if bias else None, ops.ptr(dots.t))
    keep = None
    if entry == "plain":
        assert scale == 1.0
        L.call("sp_sn_backward_batched", *args, ops.stream())
    elif entry == "scaled":
        L.call("sp_sn_backward_batched_scaled", *args, scale, ops.stream())
    else:
        keep = torch.tensor([scale], dtype=torch.float32, device=DEV)
        L.call("sp_sn_backward_batched_dscaled", *args, ops.ptr(keep), ops.stream())
    torch.cuda.synchronize()
    what = (c.what, "backward", entry, accumulate, lo, hi)
    out, dp = flat.host(what), dots.host(what)
    untouched(arena_g.host(what), arena_g.init, torch.ones(lay.arena_floats, dtype=torch.bool), (what, "the gradient arena"))
    untouched(fwd.scratch.host(what), fwd.s, torch.ones(lay.scratch_floats, dtype=torch.bool), (what, "the forward's scratch"))
    if accumulate == "separate":
        untouched(prev.host(what), prev.init, torch.ones(lay.flat_floats, dtype=torch.bool), (what, "accumulate_from"))
    own = torch.zeros(lay.flat_floats, dtype=torch.bool)
    grid_x = min(S.DOT_BLOCKS, (lay.max_elems + 1023) // 1024)
    worst = {}
    for i in range(lo, hi):
        Lr, e = c.layers[i], c.layers[i].ent
        G, db, pw, pb = ops_in[i]
        own[e.grad_off:e.grad_off + e.rows * e.cols] = True
        if bias:
            own[e.bias_off:e.bias_off + e.rows] = True
        depth = S.dot_depth(e.rows, e.cols, e.cin, e.taps, e.kind, grid_x)
        checks = S.backward_checks(Lr, fwd.got(i), G, depth, scale, pw if accumulate else None)
        nb = min(grid_x, (e.rows * e.cols + 1023) // 1024)
        mine = dp[(i - lo) * S.DOT_BLOCKS:(i - lo + 1) * S.DOT_BLOCKS]
        assert not bool(mine[:nb].isnan().any()) and bool(mine[nb:].isnan().all()), (what, i, "dot_partials: %d entries are this layer's" % nb)
        got = S.Case(grad=out[e.grad_off:e.grad_off + e.rows * e.cols], dot=mine[:nb].double().sum().to(checks["dot"][1].dtype))
        for k in checks:
            w = S.compare(Lr, got, (k,), checks) if not (k == "dot" and checks[k][0] == "within") else S.assert_within(
                got.dot.double(), checks[k][1], checks[k][2], "%s dot" % (what,))
            if checks[k][0] == "within":
                worst[k] = max(worst.get(k, 0.0), w)
        if i in zero:                                       # exact zeros, or accumulate_from as it was
            S.assert_exact(got.grad, pw.float().reshape(-1) if accumulate else torch.zeros(e.rows * e.cols), "%s layer %d: a zero dW slot" % (what, i))
        if bias:
            S.assert_exact(out[e.bias_off:e.bias_off + e.rows], S.bias_want(db, scale, pb if accumulate else None), "%s layer %d bias" % (what, i))
    untouched(out, flat.init, ~own, (what, "grads outside the layers' ranges"))
    return worst


# ------------------------------------------------------------------------------------------------------------------------------------
# the three regimes on the ragged tables
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", S.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("table", list(TABLES))
@pytest.mark.parametrize("regime", ("blocks", "integer", "dense"))
def test_forward_and_batched_backward(regime, table, dt):
    """One power iteration and the packings of a ragged table in one call, then the batched backward on its snapshots: copied, scaled
    onto an aliased and onto a separate accumulate_from, and with the factor read from device memory.  blocks: torch.equal throughout."""
    c = built(regime, table, dt)
    bank = Bank(c)
    fwd = Forward(bank)
    worst = fwd.check()
    wb = run_backward(fwd, 0)
    for k, v in run_backward(fwd, 1, "scaled", 0.5, "alias").items():
        wb[k] = max(wb.get(k, 0.0), v)
    for k, v in run_backward(fwd, 2, "scaled", 2.0, "separate", bias=False).items():
        wb[k] = max(wb.get(k, 0.0), v)
    for k, v in run_backward(fwd, 3, "dscaled", 0.25 if regime != "dense" else THIRD, "alias").items():
        wb[k] = max(wb.get(k, 0.0), v)
    assert (regime == "blocks") == (not worst and "grad" not in wb)
    report("sn %s %s %s forward" % (regime, table, S.NAME[dt]), worst)
    report("sn %s %s %s backward" % (regime, table, S.NAME[dt]), wb)


@pytest.mark.parametrize("dt", S.DTYPES, ids=DT_IDS)
def test_pack_grids_agree(dt):
    """pack_blocks = 0 (2-D grid) and pack_blocks > 0 (flat) give identical arenas - in eval mode, where two calls on one table see
    the same u and v: byte for byte, the scratch included."""
    c = built("integer", "ragged", dt, False)
    bank = Bank(c)
    flat, grid = Forward(bank, False, "flat"), Forward(bank, False, "grid")
    flat.check()
    grid.check()
    assert torch.equal(flat.a, grid.a) and torch.equal(bits(flat.s), bits(grid.s))


@pytest.mark.parametrize("regime,dt", [("blocks", F32), ("integer", BF16), ("dense", F16)], ids=["blocks-fp32", "integer-bf16", "dense-fp16"])
def test_a_table_of_256_layers(regime, dt):
    """1280 wtu units and 1280 wv units against a grid of 1024 blocks: the stride loop of sn_for_each_unit and the full LDS prefix."""
    c = built(regime, "many", dt, True, S.MAX_LAYERS)
    fwd = Forward(Bank(c))
    worst = fwd.check()
    report("sn %s 256 layers %s forward" % (regime, S.NAME[dt]), worst)
    report("sn %s 256 layers %s backward" % (regime, S.NAME[dt]), run_backward(fwd, 4, "scaled", 0.5, "alias"))


@pytest.mark.parametrize("dt", S.DTYPES, ids=DT_IDS)
def test_eval_mode_leaves_u_and_v_alone(dt):
    """power_iter = 0: u and v untouched bit for bit, sigma = u . (W v) (exact integers here), the packings use it, the snapshots
    equal the stored vectors, and the slab partials are not written."""
    c = built("integer", "ragged", dt, False)
    fwd = Forward(Bank(c), False)
    assert fwd.check() == {}
    for Lr in c.layers:
        e = Lr.ent
        assert bool(fwd.s[e.part_off:e.part_off + e.slabs * e.cols].isnan().all())


@pytest.mark.parametrize("dt", S.DTYPES, ids=DT_IDS)
def test_two_consecutive_forwards_keep_their_own_snapshots(dt):
    """The second scratch holds the second iteration's snapshots (referred to the u the first one left), the first scratch is
    unchanged, and the backward of the FIRST forward still meets its references afterwards."""
    c = built("integer", "ragged", dt)
    bank = Bank(c)
    first = Forward(bank)
    first.check()
    layers = []
    for i, Lr in enumerate(c.layers):
        nxt = S.Case(Lr)
        nxt.update(u0=first.got(i).u_out.double(), v0=first.got(i).v_out.double(), regime="dense")
        layers.append(S.finish_layer(nxt, dt))
    bank.c = S.Case(c)
    bank.c.update(layers=layers, what=c.what + ("second forward",))
    second = Forward(bank)                                   # (a Forward keeps the case it was made with)
    report("sn second forward %s" % S.NAME[dt], second.check())
    untouched(first.scratch.host("first scratch"), first.s, torch.ones_like(first.s, dtype=torch.bool), "the first forward's scratch")
    assert all(not torch.equal(first.got(i).usnap, second.got(i).usnap) for i in range(len(layers)))
    run_backward(first, 5)
    run_backward(second, 5)


SKIPS = {"first": [0], "middle": [3], "last": [len(S.RAGGED) - 1], "every": list(range(len(S.RAGGED)))}


@pytest.mark.parametrize("which", list(SKIPS))
def test_skip_pack_tables(which):
    """ops.SpectralNormBank._unpacked_table: the skipped layers' slices keep their 0xFF prefill, the others equal the full pack."""
    c = built("integer", "ragged", BF16, False)
    bank = Bank(c)
    full = Forward(bank, False)
    full.check()
    table, blocks = bank.unpacked_table(SKIPS[which])
    assert (blocks > 0) == (which != "every")
    part = Forward(bank, False, table=table, blocks=blocks, packed=set(range(len(S.RAGGED))) - set(SKIPS[which]))
    part.check()
    for i, Lr in enumerate(c.layers):
        e = Lr.ent
        for off, size in ((e.fwd_off, e.fwd_bytes), (e.dgrad_off, e.dgrad_bytes)):
            if size:
                mine = part.a[off:off + size]
                assert bool((mine == 0xFF).all()) if i in SKIPS[which] else torch.equal(mine, full.a[off:off + size]), (which, i)


def test_no_input_gradient_packing_where_dgrad_off_is_minus_one():
    c = S.sn_case("integer", S.RAGGED, BF16, 1, True, False)
    assert all(Lr.ent.dgrad_off == -1 for Lr in c.layers)
    Forward(Bank(c)).check()


@pytest.mark.parametrize("accumulate", [None, "alias"], ids=["copy", "accumulate"])
def test_group_sub_tables_and_zero_slots(accumulate):
    """Layers lo .. hi of a larger table with the grads base unchanged: every other layer's range keeps its bits.  A layer whose dW
    slot is all zero yields exact zeros, or leaves accumulate_from as it was."""
    c = S.sn_case("integer", S.RAGGED, F32, 2, True, True, [(0, 2), (2, 5), (5, len(S.RAGGED))])
    fwd = Forward(Bank(c))
    fwd.check()
    for lo, hi in c.lay.groups:
        run_backward(fwd, 6, "scaled", 0.5, accumulate, lo=lo, hi=hi, zero=(1, 3, 6))


# ------------------------------------------------------------------------------------------------------------------------------------
# the single-layer entry
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ("blocks", "integer", "dense"))
def test_single_layer_backward_in_all_four_dot_modes(regime):
    """sp_sn_backward: dot_ready 0 (memset here) and 3 (zero-filled by the caller) sum through a float atomic - exact where the
    products are integers; 1 takes <dWsn, W>, 2 takes <dWsn, W / sigma>."""
    c = built(regime, "ragged", F32)
    bank = Bank(c)
    fwd = Forward(bank)
    g = X.gen(11)
    worst = {}
    for i, Lr in enumerate(c.layers):
        e = Lr.ent
        G, _ = S.grad_bias(Lr, g)
        snap = fwd.got(i)
        dw = S.pack_dw(Lr, G).to(DEV)
        dot64 = float((G * Lr.W).sum())
        given = {0: NAN, 3: 0.0, 1: float(np.float32(dot64)), 2: float(np.float32(dot64 * float(snap.inv_sigma.double())))}
        for mode in (0, 3, 1, 2):
            grad, dot = Guarded(e.rows * e.cols), Guarded(1, F32, given[mode])
            L.call("sp_sn_backward", ops.ptr(dw), ctypes.c_void_p(bank.w.data_ptr() + 4 * e.w_off), ctypes.c_void_p(fwd.scratch.t.data_ptr() + 4 * e.scratch_off),
                   e.rows, e.cols, e.cin, e.taps, e.cin_p, e.kind, ops.ptr(dot.t), mode, ops.ptr(grad.t), ops.stream())
            torch.cuda.synchronize()
            what = "%s layer %d dot_ready %d" % (c.what, i, mode)
            depth = S.dot_depth_single(e.rows, e.cols) if mode in (0, 3) else 1
            checks = S.backward_checks(Lr, snap, G, depth, 1.0, None, given[2] if mode == 2 else None)
            got = S.Case(grad=grad.host(what), dot=dot.host(what).reshape(()))
            if mode in (1, 2):
                S.assert_exact(got.dot, torch.tensor(given[mode], dtype=torch.float32), what + ": the given dot is read only")
                checks.pop("dot")
            elif checks["dot"][0] == "within":
                worst["dot"] = max(worst.get("dot", 0.0), S.assert_within(got.dot.double(), checks["dot"][1], checks["dot"][2], what))
                checks.pop("dot")
            w = S.compare(Lr, got, None, checks)
            if checks["grad"][0] == "within":
                worst["grad"] = max(worst.get("grad", 0.0), w)
    report("sn %s sp_sn_backward" % regime, worst)


# ------------------------------------------------------------------------------------------------------------------------------------
# sp_sn_pair_scales, refusals
# ------------------------------------------------------------------------------------------------------------------------------------
def test_pair_scales_come_from_the_two_scratches():
    c = built("dense", "ragged", BF16)
    bank = Bank(c)
    a, b = Forward(bank), Forward(bank)
    n = len(c.layers)
    out = Guarded(2 * n)
    L.call("sp_sn_pair_scales", ops.ptr(bank.table), n, ops.ptr(a.scratch.t), ops.ptr(b.scratch.t), ops.ptr(out.t), ops.stream())
    torch.cuda.synchronize()
    got = out.host("pair scales").view(n, 2)
    want = torch.stack([torch.stack((torch.tensor(1.0), a.got(i).sigma * b.got(i).inv_sigma)) for i in range(n)])
    S.assert_exact(got, want, "sp_sn_pair_scales")
    assert not torch.equal(want[:, 1], torch.ones(n))


def test_refusals_write_nothing():
    """Host argument checks: an error code, the entry's name in the message, nothing launched."""
    c = built("integer", "ragged", F32, False)
    bank, lay, lib = Bank(c), c.lay, L.lib()
    scratch, arena = Guarded(lay.scratch_floats), Guarded(lay.pack_bytes, torch.uint8, 0xFF)
    n = len(lay.entries)

    def fwd(table=ops.ptr(bank.table), n_layers=n, s=ops.ptr(scratch.t), a=ops.ptr(arena.t), dtype=L.SP_F32, blocks=lay.pack_blocks):
        return lib.sp_sn_forward(table, n_layers, lay.max_rows, lay.max_cols, lay.max_pack, s, lay.scratch_floats, a, 1, dtype, blocks, ops.stream())

    off4 = ctypes.c_void_p(scratch.t.data_ptr() + 4)
    for rc in (fwd(n_layers=0), fwd(n_layers=S.MAX_LAYERS + 1), fwd(table=None), fwd(s=None), fwd(a=None), fwd(dtype=L.SP_F8), fwd(dtype=7),
               fwd(blocks=-2), fwd(s=off4), fwd(a=ctypes.c_void_p(arena.t.data_ptr() + 8))):
        assert rc == SP_ERR_INVALID and b"sp_sn_forward" in lib.sp_last_error_string()
    p = ops.ptr(scratch.t)
    btab = ops.ptr(bank.bwd_table)
    assert lib.sp_sn_backward_batched(btab, 0, lay.max_elems, p, p, p, None, None, p, ops.stream()) == SP_ERR_INVALID
    assert lib.sp_sn_backward_batched(None, n, lay.max_elems, p, p, p, None, None, p, ops.stream()) == SP_ERR_INVALID
    assert lib.sp_sn_backward_batched_dscaled(btab, n, lay.max_elems, p, p, p, None, None, p, None, ops.stream()) == SP_ERR_INVALID
    assert lib.sp_sn_backward(p, p, p, 4, 8, 3, 3, 4, 0, p, 0, p, ops.stream()) == SP_ERR_INVALID          # cin x taps != cols
    assert lib.sp_sn_backward(p, p, p, 4, 8, 8, 1, 8, 0, None, 0, p, ops.stream()) == SP_ERR_INVALID
    assert lib.sp_sn_pair_scales(ops.ptr(bank.table), 0, p, p, p, ops.stream()) == SP_ERR_INVALID
    torch.cuda.synchronize()
    what = "refusals"
    untouched(scratch.host(what), scratch.init, torch.ones(lay.scratch_floats, dtype=torch.bool), what)
    assert bool((arena.host(what) == 0xFF).all())
    untouched(bank.u.host(what), bank.u.init, torch.ones(lay.u_floats, dtype=torch.bool), what)
    untouched(bank.v.host(what), bank.v.init, torch.ones(lay.v_floats, dtype=torch.bool), what)
