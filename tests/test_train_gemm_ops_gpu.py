"""GPU: the kernels that carry most of a training step -- launch_wgrad (three GEMM kernels, five record tiles),
launch_wgrad_reduce (both kernels), launch_colreduce (four modes) and its final pass, BatchNorm finalize / apply / backward
apply, ln_train / ln_bwd, the stem's forward and weight gradient, dilate / flip_oihw / pad_cols / copy2d -- ONE LAUNCHER AT A
TIME through the d2t_op_* entries of include/d2t.h, on caller tensors in the kernels' own layouts, against float64 references
written from each operation's definition (tests/train_gemm_refs.py, pinned to torch.autograd by
tests/test_train_gemm_refs_cpu.py).  S, chunk, lda / ldb, accumulate and `add` are arguments here, so the launcher branches
that Tr::wgrad's own choice never reaches at a small shape are reached.

Every output is pre-filled with NaN (floats) / 0xFF (records) and allocated with a guard tail that must come back untouched.

Rules (none taken from the code under test; every figure is printed as a `FIG ...` line before it is asserted):
  exact     bit for bit: wgrad_reduce against the documented orders restated in numpy fp32 (grid-stride kernel: z ascending;
            one-block-per-output kernel: every 256th partial per thread, then the halving tree), then one fp32 add of dst where
            accumulate is set; the four movers; bn_bwd_apply's gout; ReLU zeros; the records bn_apply / bn_bwd_apply write,
            which must be the host split of the fp32 output the SAME launch wrote; colreduce_final with accumulate against
            prev + the non-accumulating result; guard tails; refusals (D2T_EINVAL, nothing written).
  measured  err = max |y - y64| <= 8 e32 + 1e-6 max |y64|, e32 = the largest max |y32 - y64| over three fp32 CPU evaluations of
            the same function on the same inputs (torch's own reductions, every reduction reversed, every reduction in 16
            chunks).  For the split-bf16 kernels y64 and the fp32 evaluations are of the three split products
            lo*hi + hi*lo + hi*hi of the path's own operand split, so that the split's error and the accumulation's are held
            apart.  For the BatchNorm chain torch's own evaluation of y is F.batch_norm in fp32.
  derived   the split-bf16 result against the UNSPLIT float64 product (in place of test_train_ops_gpu.py's 2e-4 of the maximum):
            Both splits -- the records' (conv_common.h split_f32) and wgrad_bf16x3_kernel's split4_bf16 -- are the same function
            (pinned bit for bit on the CPU): hi = x truncated to bf16's 8 significant bits, so r = x - hi has |r| < 2^-7 |x| and
            is exact in fp32; lo = bf16 round-to-nearest of r, |r - lo| <= 2^-8 |r| < 2^-15 |x| and |lo| <= (1 + 2^-8) 2^-7 |x|.
            With xs = hi + lo:  a b - (al bh + ah bl + ah bh) = (a b - as bs) + al bl, and
              |a b - as bs| <= |a - as| |b| + |as| |b - bs| <= (2^-15 + (1 + 2^-15) 2^-15) |a||b| < 1.001 * 2^-14 |a||b|,
              |al bl| <= (1 + 2^-8)^2 2^-14 |a||b| < 1.008 * 2^-14 |a||b|,
            so the three products miss the exact one by less than 1.005 * 2^-13 |a||b| per term.  The products of two bf16
            values are exact in fp32; adding the n = 3 * (rows of the chunk) of them into one fp32 accumulator costs at most one
            rounding of 2^-23 (truncating adder allowed for) per addition on a running sum of at most 1.02 sum |a||b|.  Bound:
              |part - part64| <= (1.005 * 2^-13 + 1.02 * (3 rows + 8) * 2^-23) * sum_p |a[p][m]| |b[src(p)][n]|   per element.

Shown to fail when a kernel is made subtly wrong (scratch builds, one mutation each, every address in range, each build run
once on an MI355X on the tests of its area):
   1 wgrad_rec_kernel without the ah * bl product            -> test_wgrad_records_and_equivalence (all 56)
   2 issue(1) skipped when the K loop has 2 steps            -> test_wgrad_records_and_equivalence (21: the cases with a chunk of 17 ... 32 rows)
   3 the pow_ carry as `if`                                  -> test_wgrad_records_and_equivalence (7: OW 5 with chunk 48)
   4 wgrad_src_row with kh and kw swapped                    -> test_wgrad_plain_geometries (15 of 21: all but 1x1)
   5 wgrad_reduce_small_kernel's tree started at 64          -> test_wgrad_reduce_exact_in_documented_order (6), the stem (4)
   6 layout 1 indexed (m N + n) + tap M N                    -> test_wgrad_reduce_exact_in_documented_order (14), the stem (8)
   7 CR_BN_BWD reading rstd[c] for mean[c]                   -> test_colreduce_modes (10), the BatchNorm chain (18)
   8 store_split4 writing lo at dst + 16                     -> the BatchNorm chain's record comparison (all 10 with records)
   9 ln_bwd without the xh * bsum term                       -> test_layernorm_forward_backward (all 12)
  10 dilate ignoring offw                                    -> test_dilate (the 3 cases with offw != 0)
  11 bn_finalize not adding the shift back to the mean       -> the BatchNorm chain (19 of 20)
  12 CR_SUM_SQ squaring the raw value beside the shifted sum -> the BatchNorm chain (19), test_colreduce_modes (5)
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_record_refs as CR
import train_gemm_refs as G
from doc2tex_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL = 1  # include/d2t.h D2T_EINVAL
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


class Buf:
    """a device output of `shape` filled with a sentinel (NaN / 0xFF), with a guard tail behind it; `init`: the contents of an
    in-place operand instead of the sentinel (the tail keeps it)"""

    def __init__(self, *shape, dtype=torch.float32, init=None):
        self.shape, self.n, self.f = shape, int(np.prod(shape)), dtype == torch.float32
        fill = NAN if self.f else (0xFF if dtype == torch.uint8 else -1)
        self.t = torch.full((self.n + GUARD,), fill, dtype=dtype, device=DEV)
        if init is not None:
            self.t[:self.n] = init.reshape(-1).to(DEV)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def _clean(self, c):
        return bool(torch.isnan(c).all()) if self.f else bool((c == (0xFF if c.dtype == torch.uint8 else -1)).all())

    def untouched(self):
        return self._clean(self.t.cpu())

    def get(self):
        c = self.t.cpu()
        assert self._clean(c[self.n:]), "a kernel wrote behind its output"
        return c[:self.n].view(*self.shape)


def _p(x):
    return None if x is None else (x.ptr if isinstance(x, Buf) else x.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _call(name, *args):
    """the entry on the current stream (always the last argument), then a synchronize"""
    lib = _lib.require_device()
    rc = getattr(lib, name)(*[_p(a) if isinstance(a, (Buf, torch.Tensor)) or a is None else a for a in args], _stream())
    torch.cuda.synchronize()
    return rc


def _rule(name, y, y64, e32, **kv):
    """the measured rule; returns err / e32"""
    assert y.shape == y64.shape and not torch.isnan(y).any(), f"{name}: unwritten / NaN elements"
    err = float((y.double() - y64).abs().max())
    mx = float(y64.abs().max())
    ratio = err / e32 if e32 > 0 else 0.0
    _fig(name, e32=e32, err=err, ratio=ratio, max=mx, **kv)
    assert err <= 8.0 * e32 + 1e-6 * mx, f"{name}: |y - y64| = {err:.3e}, e32 = {e32:.3e}, max |y64| = {mx:.3e}"
    return ratio


def _exact(name, y, want, **kv):
    want = torch.as_tensor(want)
    bad = int((_bits(y) != _bits(want)).sum()) if y.shape == want.shape else -1
    _fig(name, differing=bad, n=want.numel(), **kv)
    assert bad == 0, f"{name}: {bad} of {want.numel()} elements differ"


# =====================================================================================================================
# launch_wgrad
# =====================================================================================================================
def _wgrad(a, b, M, N, S, chunk, conv=None, bf16x3=0, records=0):
    """conv: None or (B, H, W, geom).  Returns (rc, part Buf, (bm, bn))."""
    lib = _lib.require_device()
    taps = 1 if conv is None else conv[3][0] * conv[3][1]
    part = Buf(S, taps, M, N)
    tile = (C.c_int32 * 2)(-1, -1)
    ad, bd = _d(a), _d(b)
    A = _lib.D2TOpWgradArgs()
    A.a, A.b, A.part, A.tile = ad.data_ptr(), bd.data_ptr(), part.ptr, C.cast(tile, C.c_void_p).value
    A.P, A.M, A.N, A.lda, A.ldb = a.shape[0], M, N, a.shape[1], b.shape[1]
    if conv is not None:
        B, H, W, geom = conv
        A.geom, A.B, A.H, A.W = 1, B, H, W
        A.OH, A.OW = G.out_size(H, W, geom)
        A.KH, A.KW, A.SH, A.SW, A.PH, A.PW = geom
    A.S, A.chunk, A.bf16x3, A.records = S, chunk, bf16x3, records
    rc = lib.d2t_op_wgrad(C.byref(A), _stream())
    torch.cuda.synchronize()
    return rc, part, (tile[0], tile[1])


@functools.lru_cache(maxsize=None)
def _wg_operands(P, brows, lda, ldb, seed):
    g = _gen(seed)
    return torch.randn(P, lda, generator=g), torch.randn(brows, ldb, generator=g)


@functools.lru_cache(maxsize=None)
def _wg_ref(P, brows, M, N, lda, ldb, S, chunk, conv, split, seed):
    """(y64, e32, abs64, exact64): split: references of the three split products (abs64 / exact64: the derived bound's scale and
    the unsplit float64 product)"""
    a, b = _wg_operands(P, brows, lda, ldb, seed)
    src = None if conv is None else G.src_rows(*conv)
    if not split:
        y64, e32 = G.e32_of(lambda dt, m: G.wgrad_ref(a.to(dt), b.to(dt), M, N, S, chunk, src, m))
        return y64, e32, None, None
    ahl = tuple(torch.from_numpy(v) for v in G.split4_bf16(a.numpy()))
    bhl = tuple(torch.from_numpy(v) for v in G.split4_bf16(b.numpy()))
    y64, e32 = G.e32_of(lambda dt, m: G.wgrad_split_ref(tuple(v.to(dt) for v in ahl), tuple(v.to(dt) for v in bhl), M, N, S,
                                                        chunk, src, m))
    return y64, e32, G.abs_product(a, b, M, N, S, chunk, src), G.wgrad_ref(a.double(), b.double(), M, N, S, chunk, src)


def _derived(name, y, abs64, exact64, rows, **kv):
    bound = (1.005 * 2.0 ** -13 + 1.02 * (3 * rows + 8) * 2.0 ** -23) * abs64
    err = (y.double() - exact64).abs()
    worst = float((err / bound.clamp(min=1e-300)).max())
    _fig(name, err=float(err.max()), bound=float(bound.max()), worst_ratio=worst, rel_max=float(err.max() / exact64.abs().max()), **kv)
    assert bool((err <= bound).all()), f"{name}: split-bf16 error {float(err.max()):.3e} above the derived bound (x{worst:.2f})"


def _check_wgrad(name, kernel, P, brows, M, N, lda, ldb, S, chunk, conv, seed=1, want_tile=None):
    """kernel: 'f32' | 'bf16x3' | 'rec'"""
    split = kernel != "f32"
    a, b = _wg_operands(P, brows, lda, ldb, seed)
    y64, e32, abs64, exact64 = _wg_ref(P, brows, M, N, lda, ldb, S, chunk, conv, split, seed)
    rc, part, tile = _wgrad(a, b, M, N, S, chunk, conv, bf16x3=int(split), records=int(kernel == "rec"))
    assert rc == 0
    if want_tile:
        assert tile == want_tile, tile
    y = part.get()
    tag = dict(kernel=kernel, tile="x".join(map(str, tile)), M=M, N=N, P=P, S=S, chunk=chunk)
    _rule(name, y, y64, e32, **tag)
    if split:
        _derived(name + "_derived", y, abs64, exact64, chunk, **tag)
    return y


# (M, N, lda, ldb) per plain kernel: ragged against the tile, the vocabulary's 500, M = 4, lda > M, ldb > N
WG_WIDTHS = {"f32_64": [(4, 500, 8, 504), (64, 36, 64, 36)],        # wgrad_kernel<64, 64>: M <= 64 or N <= 64
             "f32_128": [(500, 68, 504, 72), (68, 132, 68, 132)],   # wgrad_kernel<128, 128>
             "bf16x3": [(500, 68, 504, 72), (68, 132, 68, 132)]}    # wgrad_bf16x3_kernel (M, N > 64)
WG_ROWS = [(1, 32),    # one row: a K step with 31 (15) zero rows
           (31, 32),   # one short K step
           (32, 32),   # exactly one K step of the fp32 kernels (two of the bf16 one)
           (33, 32),   # a last chunk of one row
           (97, 48)]   # three chunks, chunk not a multiple of the fp32 K step, last chunk of one row


@pytest.mark.parametrize("P, chunk", WG_ROWS, ids=lambda v: str(v))
@pytest.mark.parametrize("kernel, wi", [(k, i) for k in WG_WIDTHS for i in range(2)], ids=lambda v: str(v))
def test_wgrad_plain_rows(kernel, wi, P, chunk):
    M, N, lda, ldb = WG_WIDTHS[kernel][wi]
    S = (P + chunk - 1) // chunk
    tile = (64, 64) if kernel == "f32_64" else (128, 128)
    _check_wgrad("wgrad_rows", "bf16x3" if kernel == "bf16x3" else "f32", P, P, M, N, lda, ldb, S, chunk, None, seed=P, want_tile=tile)


WG_CONVS = [("3x3p1", 3, 4, 5),      # OW 5, padding taps on every side
            ("3x3p1", 2, 3, 1),      # OW 1: two of three kw taps read padding only
            ("2x2s21p01", 3, 4, 4),  # stride (2,1), pad (0,1): OW 5
            ("2x2s2", 3, 4, 10),     # stride 2: OW 5
            ("2x2s2", 2, 4, 2),      # OW 1
            ("1x1", 3, 2, 5), ("1x1", 2, 3, 1)]


@pytest.mark.parametrize("name, B, H, W", WG_CONVS, ids=lambda v: str(v))
@pytest.mark.parametrize("kernel", list(WG_WIDTHS))
def test_wgrad_plain_geometries(kernel, name, B, H, W):
    M, N, lda, ldb = WG_WIDTHS[kernel][1]
    geom = G.GEOMS[name]
    OH, OW = G.out_size(H, W, geom)
    P, chunk = B * OH * OW, 32
    _check_wgrad("wgrad_geom", "bf16x3" if kernel == "bf16x3" else "f32", P, B * H * W, M, N, lda, ldb, (P + chunk - 1) // chunk,
                 chunk, (B, H, W, geom), seed=H * W)


REC_TILES = [(256, 256), (256, 128), (128, 128), (128, 64), (64, 32)]
REC_SHAPES = [(t, t) for t in REC_TILES] + [((384, 128), (128, 128)),   # three blocks of 128 x 128
                                            ((512, 256), (256, 256))]   # two blocks of 256 x 256
REC_CASES = [  # geometry, B, H, W, chunk
    ("3x3p1", 3, 3, 5, 16),      # P 45 (not a multiple of 16), OW 5 < 16: the carry runs more than once; K loop of 1 step; chunks
                                 # begin mid-row (16 = image 1, row 0, column 1) and mid-image
    ("3x3p1", 3, 3, 5, 48),      # the same in one chunk: K loop of 3 steps, first use of stage 2, carry over image boundaries
    ("3x3p1", 3, 2, 17, 32),     # OW 17, P 102: K loops of 2 steps (no LDS-DMA inside the loop), last chunk 6 rows
    ("3x3p1", 3, 2, 17, 48),     # 3 steps
    ("3x3p1", 3, 2, 17, 80),     # 5 steps: the steady state, every stage reused
    ("2x2s21p01", 3, 2, 15, 32), # stride (2,1), pad (0,1): OW 16 = the K step
    ("2x2s2", 3, 6, 2, 16),      # OW 1: sixteen carries per step
    ("2x2s2", 3, 4, 10, 16)]     # stride 2: OW 5, P 30


@pytest.mark.parametrize("case", REC_CASES, ids=lambda c: "-".join(map(str, c)))
@pytest.mark.parametrize("shape, tile", REC_SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_wgrad_records_and_equivalence(shape, tile, case):
    """wgrad_rec_kernel on records the entry builds, and (M, N > 64) wgrad_bf16x3_kernel on the same operands, S and chunk:
    both inside the measured rule against the same float64 sum of the three split products"""
    M, N = shape
    name, B, H, W, chunk = case
    geom = G.GEOMS[name]
    OH, OW = G.out_size(H, W, geom)
    P = B * OH * OW
    S = (P + chunk - 1) // chunk
    args = (P, B * H * W, M, N, M, N, S, chunk, (B, H, W, geom))
    y_rec = _check_wgrad("wgrad_rec", "rec", *args, seed=7, want_tile=tile)
    if M > 64 and N > 64 and shape == tile:
        y_b = _check_wgrad("wgrad_rec_vs_bf16x3", "bf16x3", *args, seed=7, want_tile=(128, 128))
        _fig("wgrad_rec_minus_bf16x3", diff=float((y_rec - y_b).abs().max()), M=M, N=N, chunk=chunk)


WG_REFUSED = [dict(M=6, N=64),                                    # M % 4
              dict(M=64, N=64, lda=66),                           # lda % 4
              dict(M=64, N=64, ldb=70),                           # ldb % 4
              dict(M=128, N=128, records=1, chunk=24),            # records: chunk % 16
              dict(M=96, N=96, records=1),                        # records: no tile
              dict(M=128, N=128, records=1, bf16x3=0),            # records need split-bf16 arithmetic
              dict(M=128, N=128, records=1, conv=False),          # records need a geometry
              dict(M=64, N=64, S=1),                              # S * chunk < P
              dict(M=64, N=64, S=4)]                              # an empty chunk


@pytest.mark.parametrize("kw", WG_REFUSED, ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()))
def test_wgrad_refusals_write_nothing(kw):
    M, N = kw["M"], kw["N"]
    B, H, W, geom = 2, 4, 6, G.GEOMS["3x3p1"]
    P, chunk = 48, kw.get("chunk", 16)
    a = torch.randn(P, kw.get("lda", M), generator=_gen(1))
    b = torch.randn(B * H * W, kw.get("ldb", N), generator=_gen(2))
    conv = (B, H, W, geom) if kw.get("conv", True) else None
    if conv is None:
        b = b[:P].contiguous()
    S = kw.get("S", (P + chunk - 1) // chunk)
    lib = _lib.require_device()
    taps = 9 if conv else 1
    part = Buf(max(S, 3), taps, M, N)
    ad, bd = _d(a), _d(b)
    A = _lib.D2TOpWgradArgs()
    A.a, A.b, A.part, A.tile = ad.data_ptr(), bd.data_ptr(), part.ptr, None
    A.P, A.M, A.N, A.lda, A.ldb = P, M, N, a.shape[1], b.shape[1]
    if conv:
        A.geom, A.B, A.H, A.W, A.OH, A.OW = 1, B, H, W, H, W
        A.KH, A.KW, A.SH, A.SW, A.PH, A.PW = geom
    A.S, A.chunk, A.bf16x3, A.records = S, chunk, kw.get("bf16x3", 1), kw.get("records", 0)
    rc = lib.d2t_op_wgrad(C.byref(A), _stream())
    torch.cuda.synchronize()
    assert rc == EINVAL and part.untouched()


# =====================================================================================================================
# launch_wgrad_reduce
# =====================================================================================================================
def _small_kernel(total, S):
    """include/d2t.h d2t_op_wgrad_reduce: when the one-block-per-output kernel is taken"""
    return (total <= 4096 and S >= 256) or (total <= 65536 and S >= 128)


RED_CASES = [  # taps, M, N, layout, S
    (9, 32, 1, 1, 256), (9, 32, 1, 1, 255),            # total 288: tree from S = 256 on
    (1, 64, 64, 0, 128), (1, 64, 64, 0, 127),          # total 4096: tree from S = 128 on
    (4, 128, 128, 1, 128),                             # total 65536: the last size the tree takes
    (1, 5, 13108, 0, 128),                             # total 65540: grid-stride
    (1, 12, 20, 1, 3), (4, 12, 20, 1, 3), (9, 12, 20, 1, 3),   # layout 1 with 1, 4, 9 taps
    (9, 8, 4, 1, 300),                                 # the tree with a second round of partials per thread
    (1, 12, 20, 0, 1), (9, 12, 20, 1, 1)]              # S = 1


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("taps, M, N, layout, S", RED_CASES, ids=lambda v: str(v))
def test_wgrad_reduce_exact_in_documented_order(taps, M, N, layout, S, accumulate):
    total = taps * M * N
    rng = np.random.default_rng(total + S)
    part = rng.standard_normal((S, taps, M, N)).astype(np.float32)
    prev = rng.standard_normal((M, N, taps) if layout == 1 else (M, N)).astype(np.float32)
    small = _small_kernel(total, S)
    want = (G.reduce_tree_fp32 if small else G.reduce_ordered_fp32)(part, layout, prev if accumulate else None)
    other = (G.reduce_ordered_fp32 if small else G.reduce_tree_fp32)(part, layout, prev if accumulate else None)
    dst = Buf(*prev.shape, init=torch.from_numpy(prev) if accumulate else None)
    pd = _d(torch.from_numpy(part))
    assert _call("d2t_op_wgrad_reduce", pd, dst, S, taps, M, N, layout, accumulate) == 0
    _fig("wgrad_reduce_orders_differ", n=int((want.view(np.int32) != other.view(np.int32)).sum()), small=int(small), S=S, total=total)
    _exact("wgrad_reduce", dst.get(), torch.from_numpy(want), small=int(small), S=S, total=total, layout=layout, acc=accumulate)
    y64 = G.reduce_ref(torch.from_numpy(part).double(), layout, torch.from_numpy(prev).double() if accumulate else None)
    assert float((dst.get().double() - y64).abs().max()) <= (S + 1) * 2.0 ** -24 * float(np.abs(part).sum(0).max() + np.abs(prev).max())


def test_wgrad_reduce_refusals():
    part, dst = _d(torch.zeros(2 * 9 * 4 * 4)), Buf(4, 4, 9)
    for S, taps, M, N, layout in [(0, 9, 4, 4, 1), (2, 9, 4, 4, 0), (2, 9, 4, 4, 2), (2, 0, 4, 4, 1), (2, 9, 0, 4, 1)]:
        assert _call("d2t_op_wgrad_reduce", part, dst, S, taps, M, N, layout, 0) == EINVAL
    assert dst.untouched()


# =====================================================================================================================
# launch_colreduce / launch_colreduce_final
# =====================================================================================================================
def _colreduce(cmode, a, y, z, mean, rstd, R, Cc):
    lib = _lib.require_device()
    n = C.c_int32(-1)
    assert lib.d2t_op_colreduce(cmode, None, None, None, None, None, None, R, Cc, C.byref(n), None) == 0 and n.value >= 1
    part = Buf(n.value, 2, Cc)
    keep = [_d(t) for t in (a, y, z, mean, rstd)]
    n2 = C.c_int32(-1)
    rc = lib.d2t_op_colreduce(cmode, *[_p(t) for t in keep], part.ptr, R, Cc, C.byref(n2), _stream())
    torch.cuda.synchronize()
    assert n2.value == n.value
    return rc, part, n.value


COL_R = [1, 127, 128, 129, 300]  # 300: three chunks of at least 128 rows, the last one ragged (asserted below)


@pytest.mark.parametrize("Cc", [4, 60, 64, 68, 512])
@pytest.mark.parametrize("cmode, with_y", [(0, False), (1, False), (2, False), (2, True), (3, False)],
                         ids=["sum", "sum_sq", "bn_bwd", "bn_bwd_relu", "ln_bwd"])
def test_colreduce_modes(cmode, with_y, Cc):
    for R in COL_R:
        g = _gen(1000 * cmode + Cc + R)
        a = torch.randn(R, Cc, generator=g)
        z = torch.randn(R, Cc, generator=g) + 1.0 if cmode >= 2 else None
        y = torch.randn(R, Cc, generator=g) if with_y else None
        nstat = Cc if cmode == 2 else R
        mean = torch.randn(nstat, generator=g) if cmode >= 2 else None
        rstd = torch.rand(nstat, generator=g) + 0.5 if cmode >= 2 else None   # (distinct from mean: swapping them shows)
        y64, e32 = G.e32_of(lambda dt, m: dict(zip(("s0", "s1"), G.colsums_ref(
            cmode, *[None if t is None else t.to(dt) for t in (a, y, z, mean, rstd)], mode=m))))
        rc, part, chunks = _colreduce(cmode, a, y, z, mean, rstd, R, Cc)
        assert rc == 0
        if R == 300:
            assert chunks >= 2, "no shape with several chunks"
        p = part.get()
        tag = dict(mode=cmode, relu=int(with_y), R=R, C=Cc, chunks=chunks)
        _rule("colreduce_s0", p[:, 0].double().sum(0).float(), y64["s0"], e32["s0"], **tag)
        if cmode == 0:
            pass  # (the second sum of CR_SUM is never read: colsum passes out1 = nullptr)
        else:
            _rule("colreduce_s1", p[:, 1].double().sum(0).float(), y64["s1"], e32["s1"], **tag)
        # the final pass: plain, without out1, accumulating
        o0, o1 = Buf(Cc), Buf(Cc)
        assert _call("d2t_op_colreduce_final", part, chunks, Cc, o0, o1, 0) == 0
        _rule("colreduce_final_s0", o0.get(), y64["s0"], e32["s0"], **tag)
        if cmode != 0:
            _rule("colreduce_final_s1", o1.get(), y64["s1"], e32["s1"], **tag)
        q0, q1 = Buf(Cc), Buf(Cc)
        assert _call("d2t_op_colreduce_final", part, chunks, Cc, q0, None, 0) == 0
        _exact("colreduce_final_out1_null", q0.get(), o0.get(), **tag)
        assert q1.untouched()
        prev = torch.randn(2, Cc, generator=g)
        r0, r1 = Buf(Cc, init=prev[0]), Buf(Cc, init=prev[1])
        assert _call("d2t_op_colreduce_final", part, chunks, Cc, r0, r1, 1) == 0
        _exact("colreduce_final_accumulate_s0", r0.get(), prev[0] + o0.get(), **tag)
        if cmode != 0:
            _exact("colreduce_final_accumulate_s1", r1.get(), prev[1] + o1.get(), **tag)


def test_colreduce_refusals():
    lib = _lib.require_device()
    a, part = _d(torch.zeros(8 * 64)), Buf(4 * 2 * 64)
    n = C.c_int32(-7)
    for cmode, R, Cc in [(0, 8, 6), (0, 8, 2), (0, 0, 8), (4, 8, 8), (-1, 8, 8), (2, 8, 8)]:  # C % 4, C < 4, R, mode, operands of mode 2
        assert lib.d2t_op_colreduce(cmode, a.data_ptr(), None, None, None, None, part.ptr, R, Cc, C.byref(n), _stream()) == EINVAL
    torch.cuda.synchronize()
    assert part.untouched()


# =====================================================================================================================
# BatchNorm: finalize + apply + backward apply, chained on caller tensors
# =====================================================================================================================
EPS, MOM = 1e-5, 0.1


@functools.lru_cache(maxsize=None)
def _bn_case(R, Cc, offset, with_res, relu):
    """inputs and references.  Channel c has mean about +-offset standard deviations and a standard deviation between 0.5 and 2."""
    g = _gen(31 * R + Cc + 7 * int(offset) + 2 * with_res + relu)
    std = 0.5 + 1.5 * torch.rand(Cc, generator=g)
    sign = torch.where(torch.arange(Cc) % 2 == 0, 1.0, -1.0)
    z = torch.randn(R, Cc, generator=g) * std + sign * offset * std
    gamma, beta = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g) * 0.5
    res = torch.randn(R, Cc, generator=g) if with_res else None
    dy = torch.randn(R, Cc, generator=g)
    rm, rv = torch.randn(Cc, generator=g), torch.rand(Cc, generator=g) + 0.5
    if relu:  # keep every pre-activation 1e-3 clear of the kink (test_train_ops_gpu.py): move the residual, or drop dy there
        st = G.bn_stats_ref(z.double(), EPS)
        t = G.bn_apply_ref(z.double(), st["mean"], st["rstd"], gamma.double(), beta.double(), None if res is None else res.double())
        near = t.abs() < 1e-3
        if with_res:
            res = res + torch.where(near, torch.where(t >= 0, 4e-3, -4e-3), 0.0).float()
        else:
            dy = dy.masked_fill(near, 0.0)

    def run(dt, m):
        k = G.bn_chain_ref(z.to(dt), gamma.to(dt), beta.to(dt), None if res is None else res.to(dt), relu, dy.to(dt), EPS, MOM,
                           rm.to(dt), rv.to(dt), m)
        if dt == torch.float32 and m == "plain" and R > 1:  # torch's own evaluation of the forward
            t = F.batch_norm(z.t()[None], None, None, gamma, beta, training=True, momentum=MOM, eps=EPS)[0].t()
            t = t if res is None else t + res
            k["y"] = torch.relu(t) if relu else t
        return k

    y64, e32 = G.e32_of(run)
    t64 = G.bn_apply_ref(z.double(), y64["mean"], y64["rstd"], gamma.double(), beta.double(), None if res is None else res.double())
    if relu:
        assert with_res is False or float(t64.abs().min()) >= 1e-3
    return dict(z=z, gamma=gamma, beta=beta, res=res, dy=dy, rm=rm, rv=rv, y64=y64, e32=e32, t64=t64)


def _bn_chain_gpu(k, R, Cc, relu, planes):
    """the six launches on caller tensors; returns the outputs on the host"""
    z, gamma, beta, res, dy = (_d(k[n]) for n in ("z", "gamma", "beta", "res", "dy"))
    rc, part, chunks = _colreduce(G.CR_SUM_SQ, k["z"], None, None, None, None, R, Cc)
    assert rc == 0
    mean, rstd = Buf(Cc), Buf(Cc)
    rm, rv = Buf(Cc, init=k["rm"]), Buf(Cc, init=k["rv"])
    assert _call("d2t_op_bn_finalize", part, chunks, Cc, R, C.c_float(EPS), C.c_float(MOM), z, mean, rstd, rm, rv) == 0
    y, ypl = Buf(R, Cc), Buf(R * Cc * 2, dtype=torch.int16) if planes else None
    assert _call("d2t_op_bn_apply", z, mean, rstd, gamma, beta, res, y, ypl, R, Cc, int(relu)) == 0
    lib = _lib.require_device()
    n = C.c_int32()
    part2 = Buf(chunks, 2, Cc)
    assert lib.d2t_op_colreduce(G.CR_BN_BWD, dy.data_ptr(), y.ptr if relu else None, z.data_ptr(), mean.ptr, rstd.ptr, part2.ptr, R, Cc,
                                C.byref(n), _stream()) == 0 and n.value == chunks
    s0, s1 = Buf(Cc), Buf(Cc)
    assert _call("d2t_op_colreduce_final", part2, chunks, Cc, s0, s1, 0) == 0
    dz, gout, dpl = Buf(R, Cc), Buf(R, Cc), Buf(R * Cc * 2, dtype=torch.int16) if planes else None
    assert _call("d2t_op_bn_bwd_apply", dy, y if relu else None, z, mean, rstd, gamma, s0, s1, dz, gout, dpl, R, Cc) == 0
    out = dict(mean=mean.get(), rstd=rstd.get(), run_mean=rm.get(), run_var=rv.get(), y=y.get(), s0=s0.get(), s1=s1.get(),
               dz=dz.get(), g=gout.get())
    if planes:
        out["y_planes"], out["dz_planes"] = ypl.get(), dpl.get()
    return out


def _check_bn(R, Cc, offset, with_res, relu, planes):
    k = _bn_case(R, Cc, offset, with_res, relu)
    o = _bn_chain_gpu(k, R, Cc, relu, planes)
    y64, e32 = k["y64"], k["e32"]
    tag = dict(R=R, C=Cc, offset=offset, res=int(with_res), relu=int(relu))
    ratios = {n: _rule("bn_" + n, o[n], y64[n], e32[n], **tag) for n in ("mean", "rstd", "run_mean", "run_var", "y", "s0", "s1", "dz")}
    # exact: gout = dy where the kernel's own y is positive (dy without ReLU); ReLU zeros; the records of the same launch
    want_g = torch.where(o["y"] > 0, k["dy"], torch.zeros(())) if relu else k["dy"]
    _exact("bn_gout", o["g"], want_g, **tag)
    if relu:
        neg = k["t64"] <= -1e-3
        _exact("bn_relu_zeros", o["y"][neg], torch.zeros(int(neg.sum())), **tag)
    if planes:
        for n in ("y", "dz"):
            want = torch.from_numpy(CR.records_of(o[n].numpy(), CR.REC_BF16).view(np.int16))
            _exact(f"bn_{n}_records", o[n + "_planes"], want, **tag)
    return ratios


BN_SHAPES = [(300, 64, True),    # three row chunks (the last ragged), one column block, records
             (129, 36, False)]   # two chunks, a ragged column block, C % 32 != 0: no records


@pytest.mark.parametrize("relu", [False, True], ids=["lin", "relu"])
@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("offset", [0.0, 2.0])
@pytest.mark.parametrize("R, Cc, planes", BN_SHAPES, ids=lambda v: str(v))
def test_batchnorm_chain(R, Cc, planes, offset, with_res, relu):
    _check_bn(R, Cc, offset, with_res, relu, planes)


def test_batchnorm_one_row():
    """R = 1: the variance is 0, rstd = 1 / sqrt(eps), y = beta, and the unbiased factor R / (R - 1) is guarded"""
    Cc = 32
    k = _bn_case(1, Cc, 2.0, False, False)
    o = _bn_chain_gpu(k, 1, Cc, False, True)
    _exact("bn_one_row_mean", o["mean"], k["z"][0])
    _exact("bn_one_row_rstd", o["rstd"], torch.full((Cc,), float(np.float32(1.0 / np.sqrt(np.float64(np.float32(EPS)))))))
    _exact("bn_one_row_y", o["y"], k["beta"][None, :].clone())
    _rule("bn_one_row_run_var", o["run_var"], k["y64"]["run_var"], k["e32"]["run_var"])
    _rule("bn_one_row_run_mean", o["run_mean"], k["y64"]["run_mean"], k["e32"]["run_mean"])
    assert float(o["dz"].abs().max()) <= 1e-3 * float(k["dy"].abs().max())  # one sample per channel carries no gradient


@pytest.mark.parametrize("offset", [8.0, 32.0])
def test_batchnorm_offset_channels(offset):
    """Channels whose mean lies 8 (32) standard deviations from zero, R = 720, C = 64, under the same measured rule: the bound's
    reference is the error of torch's fp32 batch_norm (and of the two re-associated fp32 evaluations), not the kernel.
    Measured on an MI355X.  With var = E[z^2] - mean^2 from raw fp32 sums rstd missed the rule: 4.8e-6 against
    e32 = 1.7e-7 (28.8 e32) at 8 standard deviations, 7.3e-5 (435 e32) at 32.  With the sums taken about the channel's value in
    row 0 (CR_SUM_SQ, bn_finalize): 3.2e-7 (1.9 e32) and 1.9e-7 (1.1 e32); every other output of the chain below 1.5 e32."""
    r = _check_bn(720, 64, offset, False, False, True)
    _fig("bn_offset_ratio", offset=offset, **{n: float(v) for n, v in r.items()})


def test_batchnorm_refusals():
    Cc, R = 48, 8
    z = _d(torch.randn(R, Cc))
    v = _d(torch.ones(Cc))
    y, pl = Buf(R, Cc), Buf(R * Cc * 2, dtype=torch.int16)
    assert _call("d2t_op_bn_apply", z, v, v, v, v, None, y, pl, R, Cc, 0) == EINVAL          # planes with C % 32 != 0
    assert _call("d2t_op_bn_bwd_apply", z, None, z, v, v, v, v, v, y, None, pl, R, Cc) == EINVAL
    assert _call("d2t_op_bn_apply", z, v, v, v, v, None, y, None, R, 46, 0) == EINVAL        # C % 4
    assert _call("d2t_op_bn_finalize", z, 1, Cc, R, C.c_float(EPS), C.c_float(MOM), z, y, y, y, None) == EINVAL  # one running statistic
    assert y.untouched() and pl.untouched()


# =====================================================================================================================
# LayerNorm
# =====================================================================================================================
LN_ROWS = [1, 3, 4, 5, 522]  # four rows per block: below, at and above one block; 131 blocks with a ragged last one


@pytest.mark.parametrize("with_add", [False, True], ids=["noadd", "add"])
@pytest.mark.parametrize("hot", [False, True], ids=["centred", "mean50"])
@pytest.mark.parametrize("D", [128, 256, 512])
def test_layernorm_forward_backward(D, hot, with_add):
    for rows in LN_ROWS:
        g = _gen(D + rows + hot)
        x = torch.randn(rows, D, generator=g) + (50.0 if hot else 0.0)
        gamma, beta = torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g)
        dy = torch.randn(rows, D, generator=g)
        add = torch.randn(rows, D, generator=g) if with_add else None

        def run(dt, m):
            k = G.ln_ref(x.to(dt), gamma.to(dt), beta.to(dt), 1e-5, m)
            k["dx"] = G.ln_bwd_ref(dy.to(dt), x.to(dt), k["mean"], k["rstd"], gamma.to(dt), None if add is None else add.to(dt), m)
            return k

        y64, e32 = G.e32_of(run)
        if hot:  # torch's own fp32 layer_norm as the plain evaluation's y as well
            e32["y"] = max(e32["y"], float((F.layer_norm(x, (D,), gamma, beta, 1e-5).double() - y64["y"]).abs().max()))
        xd, gd, bd, dyd, addd = (_d(t) for t in (x, gamma, beta, dy, add))
        y, mean, rstd, dx = Buf(rows, D), Buf(rows), Buf(rows), Buf(rows, D)
        assert _call("d2t_op_ln_train", xd, gd, bd, y, mean, rstd, rows, D, C.c_float(1e-5)) == 0
        assert _call("d2t_op_ln_bwd", dyd, xd, mean, rstd, gd, addd, dx, rows, D) == 0
        tag = dict(rows=rows, D=D, hot=int(hot), add=int(with_add))
        for n, b in (("y", y), ("mean", mean), ("rstd", rstd), ("dx", dx)):
            _rule("ln_" + n, b.get(), y64[n], e32[n], **tag)


def test_layernorm_refusals():
    x, v = _d(torch.randn(4, 384)), _d(torch.ones(384))
    y, m = Buf(4, 384), Buf(4)
    assert _call("d2t_op_ln_train", x, v, v, y, m, m, 4, 384, C.c_float(1e-5)) == EINVAL
    assert _call("d2t_op_ln_bwd", x, x, v, v, v, None, y, 4, 384) == EINVAL
    assert _call("d2t_op_ln_train", x, v, v, y, m, m, 0, 128, C.c_float(1e-5)) == EINVAL
    assert y.untouched() and m.untouched()


# =====================================================================================================================
# stem: forward and weight gradient
# =====================================================================================================================
STEM_IMAGES = [(2, 5, 7, (32, 1)),      # 70 pixels: chunks of 32 (last one 6 rows) and of one pixel
               (2, 20, 36, (1024, 1))]  # 1440 pixels: a ragged second chunk; 1440 chunks of one pixel -> the tree reduction


@pytest.mark.parametrize("B, H, W, chunks", STEM_IMAGES, ids=lambda v: str(v))
@pytest.mark.parametrize("Cout, Cin", [(32, 1), (32, 3), (64, 1), (64, 3)])
def test_stem_forward_and_weight_gradient(Cout, Cin, B, H, W, chunks):
    g = _gen(Cout + Cin + H)
    img = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * 0.3
    dz = torch.randn(B * H * W, Cout, generator=g)
    imgd, wd, dzd = _d(img), _d(w), _d(dz)
    z = Buf(B * H * W, Cout)
    assert _call("d2t_op_stem_raw", imgd, wd, z, B, Cin, H, W, Cout) == 0
    y64, e32 = G.e32_of(lambda dt, m: G.stem_ref(img.to(dt), w.to(dt), m))
    tag = dict(Cout=Cout, Cin=Cin, H=H, W=W)
    _rule("stem_raw", z.get(), y64, e32, **tag)
    K, P = 9 * Cin, B * H * W
    for chunk in chunks:
        n = (P + chunk - 1) // chunk
        part = Buf(n, K, Cout)
        assert _call("d2t_op_stem_wgrad", imgd, dzd, part, B, Cin, H, W, Cout, chunk, n) == 0
        p64, pe = G.e32_of(lambda dt, m: G.stem_wgrad_ref(img.to(dt), dz.to(dt), chunk, m))
        _rule("stem_wgrad_part", part.get(), p64, pe, chunk=chunk, n=n, **tag)
        # reduced as the step does it: M = Cout, N = 1, layout 1 -> OIHW
        dw = Buf(Cout, Cin, 3, 3)
        assert _call("d2t_op_wgrad_reduce", part, dw, n, K, Cout, 1, 1, 0) == 0
        d64, de = G.e32_of(lambda dt, m: G.reduce_ref(G.stem_wgrad_ref(img.to(dt), dz.to(dt), chunk, m).reshape(n, K, Cout, 1), 1,
                                                      mode=m).reshape(Cout, Cin, 3, 3))
        _rule("stem_dw", dw.get(), d64, de, chunk=chunk, n=n, small=int(_small_kernel(K * Cout, n)), **tag)
        want = (G.reduce_tree_fp32 if _small_kernel(K * Cout, n) else G.reduce_ordered_fp32)(
            part.get().numpy().reshape(n, K, Cout, 1), 1)
        _exact("stem_dw_order", dw.get(), torch.from_numpy(want).reshape(Cout, Cin, 3, 3), chunk=chunk, **tag)


def test_stem_refusals():
    img, w = _d(torch.randn(1, 1, 4, 4)), _d(torch.randn(64 * 9))
    z = Buf(16, 64)
    assert _call("d2t_op_stem_raw", img, w, z, 1, 1, 4, 4, 48) == EINVAL          # Cout = 48
    assert _call("d2t_op_stem_wgrad", img, w, z, 1, 1, 4, 4, 48, 16, 1) == EINVAL
    assert _call("d2t_op_stem_raw", img, w, z, 1, 2, 4, 4, 32) == EINVAL          # Cin = 2
    assert _call("d2t_op_stem_wgrad", img, w, z, 1, 1, 4, 4, 32, 8, 1) == EINVAL  # chunks do not cover the pixels
    assert _call("d2t_op_stem_wgrad", img, w, z, 1, 1, 4, 4, 32, 8, 3) == EINVAL  # an empty chunk
    assert z.untouched()


# =====================================================================================================================
# movers (exact)
# =====================================================================================================================
DILATE_CASES = [  # B, OH, OW, C, DH, DW, SH, SW, offh, offw
    (2, 3, 4, 8, 6, 5, 2, 1, 1, 0),     # stride (2,1), offset in h; DH exactly the dilated extent + offset
    (2, 3, 4, 8, 8, 9, 2, 2, 1, 1),     # stride (2,2), both offsets
    (1, 2, 3, 5, 9, 11, 2, 2, 0, 2),    # DH / DW larger than the dilated extent: zero rows and columns behind
    (3, 4, 5, 4, 4, 5, 1, 1, 0, 0),     # stride 1: a copy
    (1, 3, 3, 4, 4, 4, 2, 2, 0, 1)]     # DH / DW smaller than the dilated extent: the rest is dropped


@pytest.mark.parametrize("case", DILATE_CASES, ids=lambda c: "-".join(map(str, c)))
def test_dilate(case):
    B, OH, OW, Cc, DH, DW, SH, SW, offh, offw = case
    src = torch.randn(B, OH, OW, Cc, generator=_gen(OH * OW))
    dst = Buf(B, DH, DW, Cc)
    assert _call("d2t_op_dilate", _d(src), dst, B, OH, OW, Cc, DH, DW, SH, SW, offh, offw) == 0
    _exact("dilate", dst.get(), G.dilate_ref(src, DH, DW, SH, SW, offh, offw))


@pytest.mark.parametrize("Cout, Cin, KH, KW", [(5, 3, 2, 2), (7, 4, 3, 3), (64, 32, 3, 3), (3, 2, 1, 1), (2, 3, 2, 3)])
def test_flip_oihw(Cout, Cin, KH, KW):
    w = torch.randn(Cout, Cin, KH, KW, generator=_gen(Cout))
    out = Buf(Cin, Cout, KH, KW)
    assert _call("d2t_op_flip_oihw", _d(w), out, Cout, Cin, KH, KW) == 0
    _exact("flip_oihw", out.get(), G.flip_oihw_ref(w))


@pytest.mark.parametrize("rows, Cs, Cd", [(7, 500, 512), (5, 64, 64), (1, 1, 3)])
def test_pad_cols(rows, Cs, Cd):
    src = torch.randn(rows, Cs, generator=_gen(Cs))
    dst = Buf(rows, Cd)
    assert _call("d2t_op_pad_cols", _d(src), dst, rows, Cs, Cd) == 0
    _exact("pad_cols", dst.get(), G.pad_cols_ref(src, Cd))


@pytest.mark.parametrize("rows, cols, lds, ldd", [(5, 12, 20, 16), (5, 12, 12, 20), (3, 7, 7, 7), (300, 33, 40, 35)])
def test_copy2d(rows, cols, lds, ldd):
    src = torch.randn(rows, lds, generator=_gen(cols))
    prev = torch.randn(rows, ldd, generator=_gen(cols + 1))
    dst = Buf(rows, ldd, init=prev)
    assert _call("d2t_op_copy2d", _d(src), lds, dst, ldd, rows, cols) == 0
    _exact("copy2d", dst.get(), G.copy2d_ref(src, prev, cols))


def test_mover_refusals():
    src, dst = _d(torch.randn(64)), Buf(64)
    assert _call("d2t_op_dilate", src, dst, 1, 2, 2, 4, 4, 4, 2, 2, -1, 0) == EINVAL
    assert _call("d2t_op_dilate", src, dst, 1, 2, 2, 4, 4, 4, 0, 2, 0, 0) == EINVAL
    assert _call("d2t_op_pad_cols", src, dst, 4, 8, 4) == EINVAL
    assert _call("d2t_op_copy2d", src, 4, dst, 8, 4, 6) == EINVAL
    assert _call("d2t_op_flip_oihw", src, dst, 0, 2, 2, 2) == EINVAL
    assert dst.untouched()
