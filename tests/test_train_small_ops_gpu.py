"""GPU: the kernels of the training step that tests/test_train_ops_gpu.py, test_recurrent_ops_gpu.py and test_criterion_gpu.py
do not reach -- GlobalContext (pool node, broadcast add, the fused inference block), embedding forward / backward, the
Philox dropout masks, the bicubic resize of the learned position table and its transpose, mean over the height, the (2,1)
max-pool, GELU / ReLU, and the small row movers -- ONE AT A TIME through the d2t_op_* test entries, against references
written in float64 from each operation's definition at the kernels' layouts (tests/train_small_refs.py, pinned to
oracle.restatement, F.interpolate and the Philox known answers by tests/test_train_small_refs_cpu.py).

Outputs are pre-filled with NaN (floats) / 0xFF (bytes) and allocated with a guard tail: an element a kernel should have
written and did not fails, and so does a write behind the specified region.

Tolerances (none of them taken from the code under test):
  exact     bit for bit: masks against the integer restatement; apply_mask (one fp32 multiply); token_rows; the forward
            values of the pools and of ReLU; the broadcast add (one fp32 add) and its dx (a copy); padding rows and absent
            tokens; mean_h_bwd = dy * fl32(1 / H); embed_bwd against an fp32 host sum of the hit rows in ascending row order
            followed by one multiply by scale (the order the kernel's comment promises), and two launches against each other.
  measured  err = max |y - y64| <= 8 e32 + 1e-6 max |y64|, e32 = the largest max |y32 - y64| over three fp32 CPU evaluations
            of the same function on the same inputs (torch's own, every reduction reversed, every reduction in 16 chunks
            summed left to right).  For the table resize the three are fp32 F.interpolate and a dense fp32
            tap-matrix product in both association orders.  Operations without a reduction (GELU, embedding rows) have one
            fp32 evaluation.  Backward references are torch.autograd on the float64 forward.
  derived   dbg, the gradient of GlobalContext's attention bias, is zero in exact arithmetic (a softmax ignores a shift of its
            logits): only |dbg| <= (HW + B + 4) 2^-24 sum |dl64| is asserted, dl64 the float64 logit gradients.
  1e-6      the (2,1) max-pool's backward against autograd, relative to max |dx64|, as test_train_ops_gpu.py holds the 2x2 one.
Every figure is printed (`FIG ...` lines, pytest -s) before it is asserted; DESIGN.md 5.5b has the table from an MI355X.

Shown to fail when a kernel is made subtly wrong (scratch builds, one mutation at a time, every address in range, each build
run once on an MI355X; the numbers are those of DESIGN.md 5.5b):
   2 embed_bwd: waves of a pass listed in reverse      -> test_embed_bwd_exact_in_ascending_row_order (the 8 cases with > 1 row)
   3 gc_pool: staging bound 512 on the ragged round     -> test_gc_pool_node, test_global_context_fused_block (all but HW 512)
  4b gc_wpool: idle pixel phase accumulates and is reduced -> test_gc_pool_node, test_gc_bcast_add_node at (1,9,11,192), (2,7,37,68)
   6 Philox key bump constants swapped                  -> test_dropout_mask_is_philox (16 of 18)
   7 draw lane order high half first                    -> test_dropout_mask_is_philox (13 of 18)
   9 bicubic transpose scanning oy < gh - 1             -> test_bicubic_table_and_its_transpose (all 7)
  10 mean_h_bwd: b from C * W only                      -> test_mean_h (B > 1 and H > 1)
NOT caught: 1 (flush at n > CAP: equivalent, the list has room for the delayed pass), 4 (nph + 1 phases alone: the idle phase
holds zeros), 5 (da = dctx . x, not against ctx: the same gradient, and how fp32 autograd itself evaluates it -- inside e32 by
construction), 8 (i0 clamped to n_in: dead for scale = G / (g + 0.1)).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_small_refs as TR
from doc2tex_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL = 1  # include/d2t.h D2T_EINVAL
U = 2.0 ** -24
NAN = float("nan")
GUARD = 64
F64 = torch.float64


def _fig(name, **kv):
    print("FIG " + name + " " + " ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in kv.items()))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _d(t):
    return None if t is None else t.contiguous().to(DEV)


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


class Buf:
    """a device output of `shape` filled with a sentinel (NaN / 0xFF bytes), with a guard tail behind it; `init`: the contents of
    an in-place operand instead of the sentinel (the tail keeps it)"""

    def __init__(self, *shape, dtype=torch.float32, init=None):
        self.shape, self.n, self.f = shape, int(np.prod(shape)), dtype == torch.float32
        self.t = torch.full((self.n + GUARD,), NAN if self.f else 0xFF, dtype=dtype, device=DEV)
        if init is not None:
            self.t[:self.n] = init.reshape(-1).to(DEV)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def _clean(self, c):
        return bool(torch.isnan(c).all()) if self.f else bool((c == 0xFF).all())

    def untouched(self):
        return self._clean(self.t.cpu())

    def get(self):
        c = self.t.cpu()
        assert self._clean(c[self.n:]), "a kernel wrote behind its output"
        return c[:self.n].view(*self.shape)


def _p(x):
    return None if x is None else (x.ptr if isinstance(x, Buf) else x.data_ptr())


def _call(name, *args):
    """the entry on the current stream (always the last argument), then a synchronize"""
    lib = _lib.require_device()
    rc = getattr(lib, name)(*[_p(a) if isinstance(a, (Buf, torch.Tensor)) or a is None else a for a in args],
                            C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def _rule(name, y, y64, e32, **kv):
    """the measured rule; returns err / e32"""
    assert not torch.isnan(y).any(), f"{name}: unwritten / NaN elements"
    err = float((y.double() - y64).abs().max())
    mx = float(y64.abs().max())
    ratio = err / e32 if e32 > 0 else 0.0
    _fig(name, e32=e32, err=err, ratio=ratio, max=mx, **kv)
    assert err <= 8.0 * e32 + 1e-6 * mx, f"{name}: |y - y64| = {err:.3e}, e32 = {e32:.3e}, max |y64| = {mx:.3e}"
    return ratio


def _exact(name, y, want, **kv):
    bad = int((_bits(y) != _bits(want)).sum()) if y.shape == want.shape else -1
    _fig(name, differing=bad, n=want.numel(), **kv)
    assert bad == 0, f"{name}: {bad} of {want.numel()} elements differ"


# =====================================================================================================================
# GlobalContext
# =====================================================================================================================
GC_SHAPES = [(1, 1, 1, 128),     # one position: a = 1, dwg = 0, dx = dctx exactly
             (2, 1, 7, 128),     # below one wave; empty gc_wpool chunks
             (3, 7, 73, 256),    # HW 511
             (2, 16, 32, 512),   # HW 512
             (2, 19, 27, 512),   # HW 513
             (1, 10, 103, 64),   # HW 1030: two full staging rounds + 6
             (2, 29, 53, 128),   # HW 1537
             (2, 3, 5, 192),     # C/4 = 48 does not divide 256
             (2, 3, 5, 68),      # C/4 = 17 does not divide 256
             # ... and with more pixels per gc_wpool chunk than pixel phases, so that the idle phase has pixels it could take
             # (at HW 15 a chunk is one pixel and phase 0 alone works): 5 phases, 7 pixels; 15 phases, 17 pixels
             (1, 9, 11, 192), (2, 7, 37, 68)]
GC_HOT = (3, 7, 73, 256, True)   # bg = 90, logits over 90 +- 20: exp overflows fp32 without the max subtraction
GC_CASES = [s + (False,) for s in GC_SHAPES] + [GC_HOT]
_gc_id = lambda c: "x".join(map(str, c[:4])) + ("-hot" if c[4] else "")


@functools.lru_cache(maxsize=None)
def _gc_case(B, H, W, Cc, hot):
    g = _gen(1000 + 7 * B + 11 * H + 13 * W + Cc + hot)
    HW = H * W
    x = torch.randn(B, HW, Cc, generator=g)
    P = TR.gc_params(Cc, seed=Cc + HW)  # wg ~ N(0, 2 / C), fc2.weight random: the ConvMLP and its gradient are alive
    if hot:
        l = x.double() @ P["wg"].double()
        P["wg"] = (P["wg"].double() * (20.0 / float(l.abs().max()))).float()
        P["bg"] = torch.tensor([90.0])
    dctx, dout = torch.randn(B, Cc, generator=g), torch.randn(B, HW, Cc, generator=g)
    pool64, pool32 = TR.e32_of(lambda dt, m: TR.gc_pool_bwd_ref(x.to(dt), P["wg"].to(dt), P["bg"].to(dt), dctx.to(dt), m))
    add64, add32 = TR.e32_of(lambda dt, m: TR.bcast_add_ref(x.to(dt), dctx.to(dt), dout.to(dt), m))
    blk64, blk32 = TR.e32_of(lambda dt, m: TR.global_context_ref(x.to(dt), P, m))
    return dict(x=x, P=P, dctx=dctx, dout=dout, pool64=pool64, pool32=pool32, add64=add64, add32=add32, blk64=blk64, blk32=blk32)


def _gc_pool(x, wg, bg, dctx, B, H, W, Cc):
    ctx, dx, dwg, dbg = Buf(B, Cc), Buf(B, H * W, Cc), Buf(Cc), Buf(1)
    keep = [_d(t) for t in (x, wg, bg, dctx)]
    rc = _call("d2t_op_train_gc_pool", *keep, ctx, dx, dwg, dbg, B, H, W, Cc)
    return rc, ctx, dx, dwg, dbg


@pytest.mark.parametrize("case", GC_CASES, ids=_gc_id)
def test_gc_pool_node(case):
    """Tr::gc_pool + Tr::bwd_gc_pool: gc_logits, gc_pool, gc_pool_bwd_weights, gc_pool_bwd_dx, gc_wpool (weighted), colsum"""
    B, H, W, Cc, hot = case
    k = _gc_case(*case)
    rc, ctx, dx, dwg, dbg = _gc_pool(k["x"], k["P"]["wg"], k["P"]["bg"], k["dctx"], B, H, W, Cc)
    assert rc == 0
    y64, e32 = k["pool64"], k["pool32"]
    if hot:
        lg = k["x"].double() @ k["P"]["wg"].double() + 90.0
        _fig("gc_hot_logits", lo=float(lg.min()), hi=float(lg.max()))
        assert float(lg.max()) > 100.0 and float(lg.min()) < 80.0  # exp(l) itself is inf in fp32 from l = 88.8
    tag = dict(B=B, HW=H * W, C=Cc, hot=int(hot))
    _rule("gc_ctx", ctx.get(), y64["ctx"], e32["ctx"], **tag)
    _rule("gc_dx", dx.get(), y64["dx"], e32["dx"], **tag)
    _rule("gc_dwg", dwg.get(), y64["dwg"], e32["dwg"], **tag)
    bound = (H * W + B + 4) * U * float(y64["dl"].abs().sum())
    got = float(dbg.get().abs().max())
    _fig("gc_dbg", got=got, bound=bound, ref=float(y64["dbg"].abs().max()), **tag)
    assert not torch.isnan(dbg.get()).any() and got <= bound
    if H * W == 1:  # one position: the softmax is 1, nothing depends on the logit
        _exact("gc_ctx_one_position", ctx.get(), k["x"].reshape(B, Cc))
        _exact("gc_dx_one_position", dx.get().reshape(B, Cc), k["dctx"])
        _exact("gc_dwg_one_position", dwg.get(), torch.zeros(Cc))


@pytest.mark.parametrize("case", GC_CASES[:-1], ids=_gc_id)
def test_gc_bcast_add_node(case):
    """Tr::bcast_add + its backward: gc_bcast_add, gc_wpool without weights (empty chunks when HW < 16), the dx copy"""
    B, H, W, Cc, _ = case
    k = _gc_case(*case)
    HW = H * W
    out, dx, dy = Buf(B, HW, Cc), Buf(B, HW, Cc), Buf(B, Cc)
    keep = [_d(t) for t in (k["x"], k["dctx"], k["dout"])]
    assert _call("d2t_op_train_bcast_add", *keep, out, dx, dy, B, HW, Cc) == 0
    _exact("bcast_out", out.get(), k["x"] + k["dctx"][:, None])  # one fp32 add
    _exact("bcast_dx", dx.get(), k["dout"])
    _rule("bcast_dy", dy.get(), k["add64"]["dy"], k["add32"]["dy"], B=B, HW=HW, C=Cc)


@pytest.mark.parametrize("case", GC_CASES, ids=_gc_id)
def test_global_context_fused_block(case):
    """launch_global_context in place, fc2.weight random (the reference's zero initialisation would silence the ConvMLP):
    against float64, and its pooled vector against the pool node's on the same input"""
    B, H, W, Cc, hot = case
    k = _gc_case(*case)
    P, HW = k["P"], H * W
    x = Buf(B, HW, Cc, init=k["x"])
    ctx = Buf(B, Cc)
    w = [_d(P[n]) for n in ("wg", "bg", "w1", "b1", "ln_g", "ln_b", "w2", "b2")]
    assert _call("d2t_op_global_context", x, *w, ctx, B, HW, Cc) == 0
    tag = dict(B=B, HW=HW, C=Cc, hot=int(hot))
    assert float((k["blk64"]["out"] - k["x"].double()).abs().max()) > 0.1  # the block adds something
    _rule("gcf_out", x.get(), k["blk64"]["out"], k["blk32"]["out"], **tag)
    _rule("gcf_ctx", ctx.get(), k["blk64"]["ctx"], k["blk32"]["ctx"], **tag)
    rc, node_ctx, *_ = _gc_pool(k["x"], P["wg"], P["bg"], k["dctx"], B, H, W, Cc)
    assert rc == 0
    _rule("gcf_ctx_vs_node", ctx.get(), node_ctx.get().double(), k["blk32"]["ctx"], **tag)


@pytest.mark.parametrize("Cc", (516, 66, 0))
def test_gc_refusals(Cc):
    """C above 512 (thread = channel) and C % 4 != 0 (float4 rows): D2T_EINVAL from all three entries, nothing written"""
    B, H, W = 2, 3, 5
    n = max(Cc, 4)
    x, v, m = torch.zeros(B, H * W, n, device=DEV), torch.zeros(B, n, device=DEV), torch.zeros(n, n, device=DEV)
    outs = [Buf(B, n), Buf(B, H * W, n), Buf(n), Buf(1)]
    assert _call("d2t_op_train_gc_pool", x, v, v, v, *outs, B, H, W, Cc) == EINVAL
    assert all(o.untouched() for o in outs)
    outs = [Buf(B, H * W, n), Buf(B, H * W, n), Buf(B, n)]
    assert _call("d2t_op_train_bcast_add", x, v, x, *outs, B, H * W, Cc) == EINVAL
    assert all(o.untouched() for o in outs)
    xin, ctx = Buf(B, H * W, n), Buf(B, n)
    assert _call("d2t_op_global_context", xin, v, v, m, v, v, v, m, v, ctx, B, H * W, Cc) == EINVAL
    assert xin.untouched() and ctx.untouched()


# =====================================================================================================================
# embedding
# =====================================================================================================================
EMB_CASES = [(1, 5, 256, 0, "random"),      # single row
             (255, 93, 256, 0, "random"), (256, 93, 256, 0, "random"), (257, 93, 256, 0, "random"),  # around one listing pass
             (1023, 7, 512, -1, "same"),    # every row the same token: one below CAP
             (1024, 7, 512, -1, "same"),    # at CAP: the in-loop flush
             (1025, 7, 512, -1, "same"),    # one past CAP
             (2600, 11, 1024, -1, "mostly"),  # one token on 2300 interleaved rows: two in-loop flushes and a remainder, four column groups
             (300, 9, 260, 0, "random")]    # the c < D guard


@functools.lru_cache(maxsize=None)
def _emb_case(rows, V, D, pad_id, pattern):
    g = _gen(rows * 7 + V + D)
    if pattern == "same":
        tok = torch.full((rows,), 3, dtype=torch.int64)
    else:
        tok = torch.randint(0, V - 1, (rows,), generator=g)  # token V - 1 is absent
        if pattern == "mostly":
            tok[tok == 4] = 5
            tok[torch.randperm(rows, generator=g)[:2300]] = 4
            assert int((tok == 4).sum()) == 2300
    dx = torch.randn(rows, D, generator=g)
    if pad_id >= 0:
        tok[rows // 2] = pad_id if rows > 1 else 2
        dx[tok == pad_id] *= 1e30  # must not leak into any row, least of all as inf * 0
    scale = float(np.float32(np.sqrt(np.float32(D))))
    return tok, dx, scale, TR.embed_bwd_ordered_fp32(dx, tok, V, scale, pad_id)


def _embed_bwd(dx, tok, rows, V, D, scale, pad_id):
    dE = Buf(V, D)
    keep = [_d(dx), _d(tok)]
    rc = _call("d2t_op_embed_bwd", *keep, dE, rows, V, D, C.c_float(scale), pad_id)
    return rc, dE


@pytest.mark.parametrize("rows,V,D,pad_id,pattern", EMB_CASES)
def test_embed_bwd_exact_in_ascending_row_order(rows, V, D, pad_id, pattern):
    tok, dx, scale, want = _emb_case(rows, V, D, pad_id, pattern)
    rc, dE = _embed_bwd(dx, tok, rows, V, D, scale, pad_id)
    assert rc == 0
    got = dE.get()
    _exact("embed_bwd", got, want, rows=rows, V=V, D=D, most=int(torch.bincount(tok, minlength=V).max()))
    absent = [v for v in range(V) if v != pad_id and not bool((tok == v).any())]
    assert V - 1 in absent and float(got[absent].abs().max()) == 0.0 and float(got.abs().max()) > 0.0
    if pad_id >= 0:
        assert float(got[pad_id].abs().max()) == 0.0
    rc2, dE2 = _embed_bwd(dx, tok, rows, V, D, scale, pad_id)
    assert rc2 == 0 and _same(dE2.get(), got)  # a fixed order: two launches agree bit for bit


def test_embed_bwd_refusal():
    dx, tok = torch.zeros(4, 1028, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV)
    dE = Buf(3, 1028)
    assert _call("d2t_op_embed_bwd", dx, tok, dE, 4, 3, 1028, C.c_float(1.0), 0) == EINVAL  # four columns per thread of 256
    assert dE.untouched()


@pytest.mark.parametrize("rows,V,D", [(255, 93, 256), (300, 9, 260)])
def test_embed_train_forward(rows, V, D):
    """x[r] = E[tok[r]] * sqrt(D) + pe[r % L] with L = 7, which divides neither row count"""
    L = 7
    tok, _, scale, _ = _emb_case(rows, V, D, 0, "random")
    g = _gen(rows + D)
    E, pe = torch.randn(V, D, generator=g), torch.randn(L + 2, D, generator=g)
    y64, e32 = TR.e32_of(lambda dt, m: TR.embed_ref(E.to(dt), pe.to(dt), tok, L, scale))
    x = Buf(rows, D)
    keep = [_d(E), _d(pe), _d(tok)]
    assert _call("d2t_op_embed_train", *keep, x, rows, L, V, D, C.c_float(scale)) == 0
    _rule("embed_train", x.get(), y64, e32, rows=rows, D=D)
    bad = tok.clone()
    bad[rows - 1] = V  # a token behind the table is refused before the launch
    x2 = Buf(rows, D)
    keep[2] = _d(bad)
    assert _call("d2t_op_embed_train", *keep, x2, rows, L, V, D, C.c_float(scale)) == EINVAL and x2.untouched()


# =====================================================================================================================
# dropout
# =====================================================================================================================
_SEEDS = (0, 0x0123456789ABCDEF)
_STREAMS = (0, (3 << 16) | 5, (1 << 40) + 1)
DROP_CASES = [(n, p, _SEEDS[(i + j) % 2], _STREAMS[(i + 2 * j) % 3])
              for i, n in enumerate((1, 7, 8, 9, 2049, 100003)) for j, p in enumerate((0.1, 0.25, 0.5))]


@pytest.mark.parametrize("n,p,seed,stream_id", DROP_CASES)
def test_dropout_mask_is_philox(n, p, seed, stream_id):
    """every byte against the integer restatement of Philox4x32-10 (known-answer vectors: test_train_small_refs_cpu.py)"""
    mask = Buf(n, dtype=torch.uint8)
    assert _call("d2t_op_dropout_mask", mask, n, C.c_float(p), seed, stream_id) == 0
    got = mask.get()  # the byte behind n is part of the guard
    want = TR.dropout_mask_ref(n, p, seed, stream_id)
    _exact("dropout_mask", got, want, p=p, seed=seed, stream=stream_id, kept=int(got.sum()))


@pytest.mark.parametrize("n,p", [(9, 0.5), (100003, 0.1)])
def test_apply_mask_exact(n, p):
    g = _gen(n)
    a = torch.randn(n, generator=g)
    m = TR.dropout_mask_ref(n, p, 7, 1)
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    out = Buf(n)
    keep = [_d(a), _d(m)]
    assert _call("d2t_op_apply_mask", keep[0], keep[1], C.c_float(scale), out, n) == 0
    want = torch.where(m.bool(), a * torch.tensor(scale, dtype=torch.float32), torch.zeros(()))
    _exact("apply_mask", out.get(), want, p=p)


def test_dropout_refusals():
    mask = Buf(16, dtype=torch.uint8)
    for p in (1.0, -0.1, NAN):
        assert _call("d2t_op_dropout_mask", mask, 16, C.c_float(p), 0, 0) == EINVAL
    assert _call("d2t_op_dropout_mask", mask, 0, C.c_float(0.5), 0, 0) == EINVAL
    assert mask.untouched()


# =====================================================================================================================
# the learned position table resized to a crop's grid
# =====================================================================================================================
TABLE_CASES = [(6, 40, 3, 17, 256), (6, 40, 6, 33, 256), (6, 40, 5, 40, 256),
               (6, 40, 1, 1, 64),   # a one-cell crop
               (1, 9, 1, 5, 64),    # a one-row table: every vertical tap is clamped to it
               (4, 4, 7, 9, 32),    # upsampling: several destination cells per source cell
               (2, 3, 2, 2, 8)]


@functools.lru_cache(maxsize=None)
def _table_case(GH, GW, gh, gw, D):
    g = _gen(GH * 100 + GW + gh * 7 + gw)
    src, grad = torch.randn(GH * GW, D, generator=g), torch.randn(gh * gw, D, generator=g)
    sh, sw = TR.pos_scales(GH, GW, gh, gw)
    return (src, grad, sh, sw) + TR.bicubic_e32(src, grad, GH, GW, gh, gw, sh, sw)


@pytest.mark.parametrize("GH,GW,gh,gw,D", TABLE_CASES)
def test_bicubic_table_and_its_transpose(GH, GW, gh, gw, D):
    src, grad, sh, sw, y64, ey, d64, ed = _table_case(GH, GW, gh, gw, D)
    # floor() of a source coordinate cannot differ between fp32 and float64: none is near an integer
    margin = min(float((c - c.round()).abs().min()) for c in (TR.source_coords(sh, gh), TR.source_coords(sw, gw)))
    _fig("bicubic_coord_margin", margin=margin)
    assert margin >= 1e-4
    tag = dict(GH=GH, GW=GW, gh=gh, gw=gw, D=D)
    sd, gd = _d(src), _d(grad)
    dst, dsrc = Buf(gh * gw, D), Buf(GH * GW, D)
    assert _call("d2t_op_bicubic_table", sd, dst, GH, GW, gh, gw, D, C.c_float(sh), C.c_float(sw), 0) == 0
    _rule("bicubic_fwd", dst.get(), y64, ey, **tag)
    assert _call("d2t_op_bicubic_table", gd, dsrc, GH, GW, gh, gw, D, C.c_float(sh), C.c_float(sw), 1) == 0
    _rule("bicubic_bwd", dsrc.get(), d64, ed, **tag)
    # the adjoint identity <bwd(g), s> = <g, fwd(s)> on the kernels' own results, summed in float64
    lhs, rhs = float((dsrc.get().double() * src.double()).sum()), float((grad.double() * dst.get().double()).sum())
    scale = float((grad.double().abs() * dst.get().double().abs()).sum())
    _fig("bicubic_adjoint", lhs=lhs, rhs=rhs, rel=abs(lhs - rhs) / scale, **tag)
    assert abs(lhs - rhs) <= 1e-5 * scale


def test_bicubic_refusals():
    s, dst = torch.zeros(24, 8, device=DEV), Buf(24, 8)
    for a in ((0, 3, 2, 2, 8, 1.0, 1.0), (2, 3, 0, 2, 8, 1.0, 1.0), (2, 3, 2, 2, 0, 1.0, 1.0), (2, 3, 2, 2, 8, 0.0, 1.0),
              (2, 3, 2, 2, 8, 1.0, NAN)):
        for tr in (0, 1):
            assert _call("d2t_op_bicubic_table", s, dst, *a[:5], C.c_float(a[5]), C.c_float(a[6]), tr) == EINVAL
    assert dst.untouched()


# =====================================================================================================================
# mean over the height, the (2,1) max-pool, GELU / ReLU
# =====================================================================================================================
@pytest.mark.parametrize("B,H,W,Cc", [(1, 1, 1, 4), (2, 3, 37, 256), (3, 6, 129, 512)])
def test_mean_h(B, H, W, Cc):
    g = _gen(B + H + W)
    x, dy = torch.randn(B, H, W, Cc, generator=g), torch.randn(B, W, Cc, generator=g)
    y64, e32 = TR.e32_of(lambda dt, m: TR.mean_h_ref(x.to(dt), m))
    y, dx = Buf(B, W, Cc), Buf(B, H, W, Cc)
    keep = [_d(x), _d(dy)]
    assert _call("d2t_op_train_mean_h", *keep, y, dx, B, H, W, Cc) == 0
    _rule("mean_h", y.get(), y64, e32, B=B, H=H, W=W, C=Cc)
    inv = torch.tensor(float(np.float32(1.0) / np.float32(H)), dtype=torch.float32)
    _exact("mean_h_bwd", dx.get(), (dy * inv)[:, None].expand(B, H, W, Cc).contiguous(), B=B, H=H)


@pytest.mark.parametrize("B,H,W,Cc", [(2, 8, 17, 256), (1, 7, 5, 64)])  # odd H: floor
def test_maxpool_2x1(B, H, W, Cc):
    """VGG's MaxPool2d((2,1), (2,1)): maxpool_k_kernel and maxpool_bwd with KW = 1; post-ReLU input, ties at zero take the
    first maximum"""
    x = torch.relu(torch.randn(B, Cc, H, W, generator=_gen(50 + H)))
    assert int((x == 0).sum()) > x.numel() // 4
    OH = (H - 2) // 2 + 1
    dy = torch.randn(B, Cc, OH, W, generator=_gen(51))
    xd = x.double().requires_grad_(True)
    yr = F.max_pool2d(xd, (2, 1), (2, 1))
    assert yr.shape == (B, Cc, OH, W)
    (gx,) = torch.autograd.grad(yr, [xd], dy.double())
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    y, dx = Buf(B, OH, W, Cc), Buf(B, H, W, Cc)
    keep = [_d(nhwc(x)), _d(nhwc(dy))]
    assert _call("d2t_op_train_maxpool_w", *keep, y, dx, B, H, W, Cc, 1, 2, 1, 0, 0) == 0
    _exact("maxpool_2x1", y.get(), nhwc(yr.detach().float()))
    got = dx.get()
    assert not torch.isnan(got).any()
    rel = float((got.double() - nhwc(gx)).abs().max() / gx.abs().max())
    _fig("maxpool_2x1_bwd", rel=rel)
    assert rel <= 1e-6


def test_maxpool_w_is_the_2x2_entry_and_refuses():
    """KW = 2 is d2t_op_train_maxpool; a window the kernels do not have, C % 4 != 0 and padding above half the window are refused"""
    B, H, W, Cc = 2, 9, 13, 64
    x, dy = torch.relu(torch.randn(B, H, W, Cc, generator=_gen(3))), torch.randn(B, 4, 6, Cc, generator=_gen(4))
    xd, dyd = _d(x), _d(dy)
    y, dx, y2, dx2 = Buf(B, 4, 6, Cc), Buf(B, H, W, Cc), Buf(B, 4, 6, Cc), Buf(B, H, W, Cc)
    assert _call("d2t_op_train_maxpool_w", xd, dyd, y, dx, B, H, W, Cc, 2, 2, 2, 0, 0) == 0
    assert _call("d2t_op_train_maxpool", xd, dyd, y2, dx2, B, H, W, Cc, 2, 2, 0, 0) == 0
    assert _same(y.get(), y2.get()) and _same(dx.get(), dx2.get())
    y, dx = Buf(B, 4, 6, Cc), Buf(B, H, W, Cc)
    for a in ((B, H, W, Cc, 3, 2, 2, 0, 0), (B, H, W, 62, 1, 2, 1, 0, 0), (B, H, W, Cc, 1, 2, 1, 0, 1), (B, H, W, Cc, 1, 0, 1, 0, 0),
              (B, 1, W, Cc, 1, 2, 1, 0, 0)):
        assert _call("d2t_op_train_maxpool_w", xd, dyd, y, dx, *a) == EINVAL
    assert y.untouched() and dx.untouched()


@pytest.mark.parametrize("n", (4, 1028, 100004))
@pytest.mark.parametrize("op", (0, 1), ids=("gelu", "relu"))
def test_gelu_relu(op, n):
    """ew_kernel's EW_GELU / EW_GELU_BWD / EW_RELU / EW_RELU_BWD on a grid over [-8, 8] plus random values (no reduction: the
    three fp32 evaluations of the measured rule coincide)"""
    g = _gen(n + op)
    x = torch.cat([torch.linspace(-8, 8, n // 2), torch.randn(n - n // 2, generator=g) * 2])
    dy = torch.randn(n, generator=g)
    y64, d64 = TR.ew_ref(x.double(), dy, op)
    y32, d32 = TR.ew_ref(x, dy, op)
    y, dx = Buf(n), Buf(n)
    keep = [_d(x), _d(dy)]
    assert _call("d2t_op_train_ew", *keep, y, dx, n, op) == 0
    if op == 1:
        _exact("relu", y.get(), y32)
        _exact("relu_bwd", dx.get(), d32)
    else:
        _rule("gelu", y.get(), y64, float((y32.double() - y64).abs().max()), n=n)
        _rule("gelu_bwd", dx.get(), d64, float((d32.double() - d64).abs().max()), n=n)


def test_ew_refusals():
    x = torch.zeros(16, device=DEV)
    y, dx = Buf(16), Buf(16)
    for n, op in ((6, 0), (7, 1), (0, 0), (8, 2)):
        assert _call("d2t_op_train_ew", x, x, y, dx, n, op) == EINVAL
    assert y.untouched() and dx.untouched()


# =====================================================================================================================
# row movers and small sums of the ViT token node
# =====================================================================================================================
@pytest.mark.parametrize("B,stride,n", [(3, 1001, 997), (1, 77, 77)])
def test_sum_over_batch(B, stride, n):
    x = torch.randn(B * stride, generator=_gen(stride))
    y64, e32 = TR.e32_of(lambda dt, m: TR.sum_over_batch_ref(x.to(dt), stride, n, m))
    out = Buf(n)
    xd = _d(x)
    assert _call("d2t_op_sum_over_batch", xd, out, B, stride, n) == 0
    _rule("sum_over_batch", out.get(), y64, e32, B=B, n=n)
    if B == 1:
        _exact("sum_over_batch_one", out.get(), x[:n])
    o2 = Buf(n)
    assert _call("d2t_op_sum_over_batch", xd, o2, B, n - 1, n) == EINVAL and _call("d2t_op_sum_over_batch", xd, o2, 0, stride, n) == EINVAL
    assert o2.untouched()


@pytest.mark.parametrize("B,n,D", [(3, 37, 33), (1, 5, 8)])
def test_token_rows_both_directions(B, n, D):
    skip = 1
    src = torch.randn(B * n, D, generator=_gen(n))
    full = torch.randn(B * (n + skip), D, generator=_gen(n + 1))
    sc, ga = Buf(B * (n + skip), D), Buf(B * n, D)
    sd, fd = _d(src), _d(full)
    assert _call("d2t_op_token_rows", sd, sc, B, n, skip, D, 1) == 0
    _exact("token_rows_scatter", sc.get(), TR.token_rows_ref(src, B, n, skip, True))
    assert float(sc.get().reshape(B, n + skip, D)[:, 0].abs().max()) == 0.0  # the cls rows
    assert _call("d2t_op_token_rows", fd, ga, B, n, skip, D, 0) == 0
    _exact("token_rows_gather", ga.get(), TR.token_rows_ref(full, B, n, skip, False))
    o = Buf(B * n, D)
    assert _call("d2t_op_token_rows", fd, o, B, 0, skip, D, 0) == EINVAL and _call("d2t_op_token_rows", fd, o, B, n, -1, D, 0) == EINVAL
    assert o.untouched()


@pytest.mark.parametrize("B,stride_rows,row,D", [(3, 38, 0, 131), (3, 38, 5, 131), (1, 6, 0, 256)])
def test_sum_rows_strided(B, stride_rows, row, D):
    x = torch.randn(B * stride_rows, D, generator=_gen(stride_rows + row))
    y64, e32 = TR.e32_of(lambda dt, m: TR.sum_rows_strided_ref(x.to(dt), stride_rows, row, m))
    out = Buf(D)
    xd = _d(x)
    assert _call("d2t_op_sum_rows_strided", xd, out, B, stride_rows, row, D) == 0
    _rule("sum_rows_strided", out.get(), y64, e32, B=B, D=D, row=row)
    if B == 1:
        _exact("sum_rows_strided_one", out.get(), x[row])
    o2 = Buf(D)
    assert _call("d2t_op_sum_rows_strided", xd, o2, B, stride_rows, stride_rows, D) == EINVAL
    assert o2.untouched()
