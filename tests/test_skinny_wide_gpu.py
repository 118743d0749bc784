"""GPU: the wide form of the decode step's skinny GEMM (csrc/decode_gemm.hip skinny_wide_kernel, block tile 32 x 64 at K = 256,
32 x 32 for N <= 512 and at K = 512, 32 x 16 at K = 1024) against the split-K form, through d2t_op_skinny_form (form 0
split-K, 1 wide).

The wide form claims the split-K form's BITS for every output element: the same 16x16x4 MFMA chain per K slice, the slices
summed in ascending order from zero, the same LayerNorm association.  So the comparison is torch.equal on y and ln_out, at
row counts around the tile edges and the dispatch threshold (16, 64, 128, 384) and column counts that are no multiple of the
tile's 64, 32 or 16 columns.
The split-K form is held to float64 by tests/test_decode_ops_gpu.py; one direct float64 check of the wide form (the derived
bound of that file: |y - y64| <= (K + 4) 2^-24 (|x| |w|^T + |bias| + |res|)) guards against both being wrong alike.
Outputs are pre-filled with NaN: an element a kernel should have written and did not fails, and so does one written
outside the [M][N] block.  The last test crosses launch_skinny's dispatch threshold end to end."""
import pytest
import torch

from conftest import engine_model
from doc2tex_amd import _lib, synth
from oracle import restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL = 1  # include/d2t.h D2T_EINVAL
U = 2.0 ** -24
NAN = float("nan")
SKINNY_WIDE_MIN_M = 384  # csrc/kernels.h

MS = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 130, 383, 384, 385)
KN = ((256, 768), (256, 1024), (256, 500), (256, 16), (256, 520), (512, 512), (512, 528), (1024, 256), (1024, 40))
OPTS = ((True, True, 1), (False, False, 0), (True, False, 0), (False, True, 1))  # bias, residual, act (1 = ReLU)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


class _Problem:
    """seeded Gaussian operands for 385 rows, on the device once; a case takes the first M rows"""

    def __init__(self, K, N, shifted=False):
        g = _gen(K * 3 + N)
        self.K, self.N = K, N
        self.x = torch.randn(385, K, generator=g) + (100.0 if shifted else 0.0)
        self.w = torch.randn(N, K, generator=g) * K ** -0.5
        self.bias = torch.randn(N, generator=g) * 0.5
        self.res = torch.randn(385, N, generator=g)
        self.lg, self.lb = 1.0 + 0.2 * torch.randn(K, generator=g), 0.2 * torch.randn(K, generator=g)
        self.d = {k: getattr(self, k).to(DEV) for k in ("x", "w", "bias", "res", "lg", "lb")}


def _call(P, form, M, use_bias, use_res, act, ln=False, ldx=None, ldy=None, step=None, nsteps=1):
    """returns rc, y [nsteps][M][ldy], ln_out [M][K] or None (device tensors)"""
    lib = _lib.require_device()
    K, N = P.K, P.N
    ldx, ldy = ldx or K, ldy or N
    if ldx == K:
        xd = P.d["x"][:M].contiguous()
    else:
        xd = torch.full((M, ldx), 7.0, device=DEV)  # the padding columns must not matter
        xd[:, :K] = P.d["x"][:M]
    rd = P.d["res"][:M].contiguous() if use_res else None
    y = torch.full((nsteps, M, ldy), NAN, device=DEV)
    lo = torch.full((M, K), NAN, device=DEV) if ln and N >= K else None
    st = torch.tensor([step], dtype=torch.int32, device=DEV) if step is not None else None
    rc = lib.d2t_op_skinny_form(_lib.ptr(xd), _lib.ptr(P.d["w"]), _lib.ptr(P.d["bias"] if use_bias else None), _lib.ptr(rd),
                                _lib.ptr(P.d["lg"] if ln else None), _lib.ptr(P.d["lb"] if ln else None), 1e-5, _lib.ptr(y),
                                _lib.ptr(lo), M, K, N, ldx, ldy, act, _lib.ptr(st), M * ldy, form, _lib.stream_of(xd))
    torch.cuda.synchronize()
    return rc, y, lo


def _same(a, b):
    """bitwise, NaN fill included"""
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _compare(P, M, use_bias, use_res, act, **kw):
    rc0, y0, lo0 = _call(P, 0, M, use_bias, use_res, act, **kw)
    rc1, y1, lo1 = _call(P, 1, M, use_bias, use_res, act, **kw)
    what = (P.K, P.N, M, use_bias, use_res, act, kw)
    assert rc0 == 0 and rc1 == 0, what
    s = kw.get("step") or 0
    assert not torch.isnan(y0[s, :, :P.N]).any(), what
    assert _same(y1, y0), what  # the NaN fill outside [M][N] of step s included: nothing else is written
    if lo0 is not None:
        assert not torch.isnan(lo0).any() and _same(lo1, lo0), what


@pytest.mark.parametrize("K,N", KN)
def test_wide_form_equals_splitk_form_bitwise(K, N):
    P = _Problem(K, N)
    for M in MS:
        for use_bias, use_res, act in OPTS:
            _compare(P, M, use_bias, use_res, act)


@pytest.mark.parametrize("K,N", [(256, 768), (256, 1024), (512, 512), (512, 528)])
def test_wide_form_layernorm_prologue_and_ln_out_bitwise(K, N):
    """rows of mean 100, sigma 1 (what a one-pass variance gets wrong), ln_out requested (N >= K)"""
    P = _Problem(K, N, shifted=True)
    for M in MS:
        for use_bias, use_res, act in OPTS[:2]:
            _compare(P, M, use_bias, use_res, act, ln=True)


@pytest.mark.parametrize("K,N,ln", [(256, 500, True), (256, 520, True), (1024, 40, True), (512, 528, False)])
def test_wide_form_strides_and_step_offset_bitwise(K, N, ln):
    """ldx > K, ldy > N (the logits' strided store), the step-offset output base; LayerNorm without ln_out (N < K too)"""
    P = _Problem(K, N, shifted=ln)
    for M in (17, 130, 385):
        for step in (0, 3):
            _compare(P, M, True, False, 0, ln=ln, ldx=K + 4, ldy=N + 8, step=step, nsteps=4)
        _compare(P, M, True, True, 1, ln=ln, ldx=K + 8)


def test_wide_form_vs_float64():
    M, K, N = 384, 256, 768
    P = _Problem(K, N)
    rc, y, _ = _call(P, 1, M, True, True, 0)
    assert rc == 0
    x, w, bias, res = P.x[:M].double(), P.w.double(), P.bias.double(), P.res[:M].double()
    ref = x @ w.T + bias + res
    tol = (K + 4) * U * (x.abs() @ w.abs().T + bias.abs() + res.abs())
    got = y[0].cpu().double()
    assert not torch.isnan(got).any(), "unwritten output elements"
    err = (got - ref).abs()
    print(f"FIG skinny_wide M={M} K={K} N={N} err={float(err.max()):.3e} tol_min={float(tol.min()):.3e}")
    assert float((err - tol).max()) <= 0


def test_wide_form_refuses_what_launch_skinny_refuses():
    lib = _lib.require_device()
    xd, wd = torch.zeros(8, 512, device=DEV), torch.zeros(64, 512, device=DEV)
    g, lo = torch.ones(512, device=DEV), torch.full((8, 512), NAN, device=DEV)
    y = torch.full((8, 128), NAN, device=DEV)
    # (K, N, ldx, ln, ln_out, form): K the wide form does not serve, ldx % 4, ln_out with N < K, no such form
    for K, N, ldx, ln, want_lo, form in ((48, 64, 48, False, False, 1), (208, 64, 208, False, False, 1), (128, 64, 128, False, False, 1),
                                         (256, 64, 258, False, False, 1), (512, 64, 512, True, True, 1), (256, 64, 256, False, False, 2),
                                         (256, 64, 256, False, False, -1)):
        rc = lib.d2t_op_skinny_form(_lib.ptr(xd), _lib.ptr(wd), None, None, _lib.ptr(g if ln else None), _lib.ptr(g if ln else None),
                                    1e-5, _lib.ptr(y), _lib.ptr(lo if want_lo else None), 4, K, N, ldx, 64, 0, None, 0, form,
                                    _lib.stream_of(xd))
        torch.cuda.synchronize()
        assert rc == EINVAL and torch.isnan(y).all() and torch.isnan(lo).all(), (K, N, ldx, ln, want_lo, form)


def test_rows_do_not_depend_on_the_dispatch_threshold():
    """T2, bf16x3 default, 12 steps: 2 * SKINNY_WIDE_MIN_M rows -- two seeded 48 x 64 crops repeated -- in ONE greedy call run
    the wide form; the two crops alone (B = 2) run the split-K form.  Tokens and logits of every row are bitwise those of
    its crop in the B = 2 call."""
    B = 2 * SKINNY_WIDE_MIN_M
    _, m = engine_model("T2", 12)
    two = synth.synth_images(2, 48, 64, seed=1000).cuda()
    many = two.repeat(B // 2, 1, 1, 1)
    with torch.no_grad():
        p2, l2, _ = m(two, torch.full((2, 1), R.GO, dtype=torch.long, device=DEV), is_train=False)
        pb, lb, _ = m(many, torch.full((B, 1), R.GO, dtype=torch.long, device=DEV), is_train=False)
    torch.cuda.synchronize()
    assert pb.shape == (B,) + tuple(p2.shape[1:]) and lb.shape == (B,) + tuple(l2.shape[1:])
    assert torch.equal(pb, p2.repeat(B // 2, 1))
    assert _same(lb.contiguous(), l2.repeat(B // 2, 1, 1).contiguous())
