"""GPU: the decode step's kernels (csrc/decode.hip, decode_gemm.hip, decode_row.hip, decode_beam.hip) ONE AT A TIME
through the d2t_op_* test entries, against references written here in float64 from each operation's definition -- the skinny split-K GEMM and its LayerNorm prologue, the
fused decoder-row kernels (kinds 0-5 of d2t_op_decoder_row), argmax + embed with its end-of-sequence bookkeeping, the
beam top-k, the device-side Beam.advance, the ancestry table and the cache gather.

Outputs are pre-filled with NaN (floats) / -1 (ints): an element a kernel should have written and did not fails.

Tolerances (none of them taken from the code under test):
  exact     integers, copies, indices under exact ties.
  derived   one dot product deep: |y - y64| <= (K + 4) 2^-24 (|x| |w|^T + |bias| + |res|), the textbook bound of any
            summation order; ReLU is 1-Lipschitz, GELU <= 1.13, plus 4 ulp of the result for erff.
            x = emb sqrt(d) + pe: 2 * 2^-24 (|emb sqrt(d)| + |pe|).
  measured  chained operators: e32 = max |y32 - y64| of a plain fp32 PyTorch CPU evaluation of the same operation on the
            same inputs; the kernel gets max |y - y64| <= 8 e32 + 1e-6 max |y64| (split-K over eight waves, MFMA
            accumulation order, expf / rsqrtf within a few ulp, online softmax: reorderings a sequential fp32
            evaluation does not sample; a dropped key, tile tail or bias is orders of magnitude above).
  split-bf16 row kernels (kinds 3, 4): (a) the measured rule against a float64 evaluation in which the memory rows, the
            absorbed queries and the probabilities are hi + lo and the lo * lo product is left out -- queries and
            probabilities as the kernels split them in registers (hi = upper 16 bits, lo = bf16_rne(x - hi)), the memory
            planes as launch_split_bf16 makes them (hi = bf16_rne(x), lo = bf16_rne(x - hi)); (b) 1e-3 max |y64| against
            plain float64.
Every figure is printed (`FIG ...` lines, pytest -s) before it is asserted.  Measured on an MI355X (DESIGN.md 5.3a has the
table): the kernels' error is 0.1 ... 1.9 e32 for the fp32 kinds, the LayerNorm prologue and the top-k values, and
0.7 ... 7.4 e32 for the split-bf16 kinds against the split evaluation (5e-7 ... 2.4e-5 relative against plain float64).

Shown to fail when the kernel is made subtly wrong (scratch builds, one mutation at a time, every address in range):
  `idx < bi` -> `idx > bi` in the top-k lane scan; the top-k cross-wave tie-break removed
        -> test_beam_topk_exact_ties_take_the_lower_flat_index, test_beam_topk_vs_float64, ..._rows_with_minus_inf_logits
  `i < bi` dropped from argmax_embed_kernel -> test_argmax_first_maximum_under_ties, test_argmax_embed_bookkeeping_over_steps
  the last wave's partial left out of the split-K sum -> all four test_skinny_* value tests
  LayerNorm prologue with a one-pass variance -> test_skinny_layernorm_prologue (the mean-100 rows)
  the two-row kernels storing the second row at the first row's place -> test_decoder_row_projected_d512_vs_float64,
        ..._two_row_build_equals_one_row_build_d512 (d 512); test_decoder_row_vs_float64, ..._one_row_against_two_row_build
        (absorbed); test_decoder_row_result_does_not_depend_on_the_launch (both)
  one key tile skipped when T % 16 != 0 -> test_decoder_row_vs_float64, test_decoder_row_ancestry
  `n_par[q]` read as `n_par[0]` in pass 3 of beam_dev_advance_kernel -> test_beam_advance_matches_the_python_restatement
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from doc2tex_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL = 1  # include/d2t.h D2T_EINVAL
U = 2.0 ** -24
NAN = float("nan")


def _fig(name, **kv):
    print("FIG " + name + " " + " ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in kv.items()))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _d(t):
    return None if t is None else t.contiguous().to(DEV)


def _i32(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.int32)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _measured(name, y, y64, y32=None, e32=None, factor=8.0, **kv):
    """the measured rule (e32 from the fp32 evaluation y32 of the same inputs unless given); returns (e32, err)"""
    assert not torch.isnan(y).any(), f"{name}: unwritten / NaN elements"
    if e32 is None:
        e32 = float((y32.double() - y64).abs().max())
    err = float((y.double() - y64).abs().max())
    mx = float(y64.abs().max())
    _fig(name, e32=e32, err=err, ratio=err / e32 if e32 > 0 else 0.0, max=mx, **kv)
    assert err <= factor * e32 + 1e-6 * mx, f"{name}: |y - y64| = {err:.3e}, e32 = {e32:.3e}, max |y64| = {mx:.3e}"
    return e32, err


# =====================================================================================================================
# skinny GEMM
# =====================================================================================================================
def _skinny_call(x, w, bias, res, ln, M, K, N, ldx, ldy, act, step=None, nsteps=1, want_ln_out=False):
    """x [M][K] is laid out with row stride ldx, y with ldy; returns rc, y [nsteps][M][ldy], ln_out [M][K]"""
    lib = _lib.require_device()
    xd = torch.full((M, ldx), 7.0)  # the padding columns must not matter
    xd[:, :K] = x
    xd = _d(xd)
    wd, bd, rd = _d(w), _d(bias), _d(res)
    g, b = (_d(ln[0]), _d(ln[1])) if ln else (None, None)
    y = torch.full((nsteps, M, ldy), NAN, device=DEV)
    lo = torch.full((M, K), NAN, device=DEV) if want_ln_out else None
    st = _d(_i32([step])) if step is not None else None
    rc = lib.d2t_op_skinny(_lib.ptr(xd), _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(rd), _lib.ptr(g), _lib.ptr(b), 1e-5, _lib.ptr(y),
                           _lib.ptr(lo), M, K, N, ldx, ldy, act, _lib.ptr(st), M * ldy, _lib.stream_of(xd))
    torch.cuda.synchronize()
    return rc, y.cpu(), None if lo is None else lo.cpu()


def _act(v, act):
    return F.relu(v) if act == 1 else F.gelu(v) if act == 2 else v


def _skinny_inputs(M, K, N, seed, use_bias, use_res):
    g = _gen(seed)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) * K ** -0.5
    bias = torch.randn(N, generator=g) * 0.5 if use_bias else None
    res = torch.randn(M, N, generator=g) if use_res else None
    return x, w, bias, res


def _check_skinny_plain(M, K, N, act, use_bias, use_res, seed, ldx=None, ldy=None, step=None, nsteps=1):
    ldx, ldy = ldx or K, ldy or N
    x, w, bias, res = _skinny_inputs(M, K, N, seed, use_bias, use_res)
    rc, y, _ = _skinny_call(x, w, bias, res, None, M, K, N, ldx, ldy, act, step, nsteps)
    assert rc == 0
    pre = x.double() @ w.double().T
    mag = x.double().abs() @ w.double().abs().T
    if bias is not None:
        pre, mag = pre + bias.double(), mag + bias.double().abs()
    if res is not None:
        pre, mag = pre + res.double(), mag + res.double().abs()
    ref = _act(pre, act)
    tol = (K + 4) * U * mag * (1.13 if act == 2 else 1.0) + (4 * 2.0 ** -23 * ref.abs() if act == 2 else 0.0)
    s = step or 0
    got = y[s, :, :N].double()
    assert not torch.isnan(got).any(), "unwritten output elements"
    over = ((got - ref).abs() - tol).max()
    _fig("skinny", M=M, K=K, N=N, act=act, err=float((got - ref).abs().max()), tol_min=float(tol.min()))
    assert over <= 0, f"|y - y64| exceeds the derived bound by {float(over):.3e}"
    y[s, :, :N] = NAN  # everything else -- padding columns, other steps' slabs -- must be untouched
    assert torch.isnan(y).all(), "the kernel wrote outside its [M][N] block"


_SK_M = (1, 15, 16, 17, 31, 33, 64, 65, 130)
_SK_N = (16, 500, 512, 513, 768, 1536)
SKINNY_CASES = []
for _ki, _K in enumerate((256, 512, 1024)):
    for _ni, _N in enumerate(_SK_N):
        _c = _ki * 6 + _ni
        SKINNY_CASES.append((_SK_M[(_c * 2 + _ki) % 9], _K, _N, _c % 3, bool(_c & 1), bool(_c & 2)))
# both sides of the N <= 512 tile switch with the same rows, around the 16- / 32-row tile edges
for _K, _M in ((256, 33), (512, 17), (1024, 65), (256, 31), (512, 130), (1024, 16)):
    for _N in (512, 513):
        SKINNY_CASES.append((_M, _K, _N, (_M + _N) % 3, True, _M % 2 == 1))
SKINNY_CASES += [(64, 256, 1536, 1, True, False), (64, 512, 1536, 2, False, True), (130, 1024, 768, 0, True, True),
                 (1, 1024, 1536, 1, True, True), (15, 512, 16, 2, True, True), (64, 1024, 500, 0, False, False)]


@pytest.mark.parametrize("M,K,N,act,use_bias,use_res", SKINNY_CASES)
def test_skinny_splitk_vs_float64(M, K, N, act, use_bias, use_res):
    _check_skinny_plain(M, K, N, act, use_bias, use_res, seed=M * 7 + K + N)


@pytest.mark.parametrize("M", _SK_M)
@pytest.mark.parametrize("K,N", [(512, 768), (256, 16)])
def test_skinny_every_row_count_on_both_tile_heights(M, K, N):
    """32-row tiles (N > 512) and 16-row tiles at every row count of the list: ragged last tiles, one and several tiles"""
    _check_skinny_plain(M, K, N, 0, True, True, seed=M + N)


@pytest.mark.parametrize("M,K,N,act,use_bias,use_res", [
    (1, 48, 16, 0, False, False), (17, 48, 500, 1, True, False), (65, 48, 513, 2, True, True), (130, 48, 768, 0, False, True),
    (15, 208, 16, 1, True, True), (33, 208, 512, 2, False, True), (64, 208, 1536, 0, True, False), (130, 208, 513, 1, True, True)])
def test_skinny_generic_vs_float64(M, K, N, act, use_bias, use_res):
    _check_skinny_plain(M, K, N, act, use_bias, use_res, seed=M + K + N)


@pytest.mark.parametrize("M,K,N,ldx,ldy,step,nsteps", [
    (17, 256, 500, 260, 500, None, 1), (33, 512, 93, 512, 100, None, 1), (64, 1024, 513, 1028, 520, None, 1),
    (5, 256, 93, 256, 93, 0, 3), (17, 512, 500, 516, 504, 2, 3), (33, 1024, 768, 1024, 768, 1, 3), (65, 208, 93, 212, 96, 3, 4),
    (64, 256, 16384, 256, 16384, 1, 2)])
def test_skinny_strides_and_step_offset(M, K, N, ldx, ldy, step, nsteps):
    """ldx > K, ldy > N (the logits' strided store) and the step-offset output base"""
    _check_skinny_plain(M, K, N, 0, True, False, seed=M + N, ldx=ldx, ldy=ldy, step=step, nsteps=nsteps)


@pytest.mark.parametrize("M,K,N,act,shifted,use_res", [
    (1, 256, 512, 0, True, False), (17, 256, 768, 1, True, False), (33, 256, 1536, 0, False, True), (64, 256, 513, 2, True, True),
    (15, 512, 512, 1, True, False), (31, 512, 1536, 0, True, True), (64, 512, 513, 0, False, False), (65, 512, 768, 2, True, False),
    (130, 256, 256, 0, True, False), (16, 1024, 1024, 1, True, False), (33, 1024, 1536, 0, False, True)])
def test_skinny_layernorm_prologue(M, K, N, act, shifted, use_res):
    """rows of mean 100, sigma 1 are what a one-pass variance gets wrong; ln_out (N >= K) is checked too"""
    x, w, bias, res = _skinny_inputs(M, K, N, 11 + M + K + N, True, use_res)
    if shifted:
        x = x + 100.0
    g = _gen(5)
    lg, lb = 1.0 + 0.2 * torch.randn(K, generator=g), 0.2 * torch.randn(K, generator=g)
    rc, y, lo = _skinny_call(x, w, bias, res, (lg, lb), M, K, N, K, N, act, want_ln_out=True)
    assert rc == 0

    def ref(dt):
        a = F.layer_norm(x.to(dt), (K,), lg.to(dt), lb.to(dt), 1e-5)
        v = a @ w.to(dt).T + bias.to(dt)
        if res is not None:
            v = v + res.to(dt)
        return a, _act(v, act)
    a64, y64 = ref(torch.float64)
    a32, y32 = ref(torch.float32)
    _measured("skinny_ln_out", lo, a64, a32, K=K, N=N, M=M, shifted=int(shifted))
    _measured("skinny_ln_y", y[0], y64, y32, K=K, N=N, M=M, shifted=int(shifted))


def test_skinny_refuses_what_it_does_not_serve():
    x, w, bias, _ = _skinny_inputs(4, 512, 256, 1, True, False)
    g = (torch.ones(512), torch.zeros(512))
    rc, y, lo = _skinny_call(x, w, bias, None, g, 4, 512, 256, 512, 256, 0, want_ln_out=True)  # ln_out with N < K
    assert rc == EINVAL and torch.isnan(y).all() and torch.isnan(lo).all()
    for K in (48, 208):  # LayerNorm with a K the prologue does not serve
        x, w, bias, _ = _skinny_inputs(4, K, 64, 1, True, False)
        rc, y, _ = _skinny_call(x, w, bias, None, (torch.ones(K), torch.zeros(K)), 4, K, 64, K, 64, 0)
        assert rc == EINVAL and torch.isnan(y).all()
    # sizes the kernels do not take; the buffers are large enough for whatever a launch would have touched
    lib = _lib.require_device()
    xd, wd = _d(torch.zeros(8, 512)), _d(torch.zeros(64, 512))
    y = torch.full((8, 128), NAN, device=DEV)
    neg = _d(_i32([-1]))
    for M, K, N, ldx, ldy, act, step in ((4, 40, 64, 40, 64, 0, None), (4, 256, 64, 254, 64, 0, None), (4, 256, 64, 258, 64, 0, None),
                                         (4, 256, 64, 256, 60, 0, None), (4, 256, 64, 256, 64, 3, None), (4, 256, 64, 256, 64, 0, neg),
                                         (0, 256, 64, 256, 64, 0, None), (4, 256, 0, 256, 64, 0, None)):
        rc = lib.d2t_op_skinny(_lib.ptr(xd), _lib.ptr(wd), None, None, None, None, 1e-5, _lib.ptr(y), None, M, K, N, ldx, ldy, act,
                               _lib.ptr(step), 0, _lib.stream_of(xd))
        torch.cuda.synchronize()
        assert rc == EINVAL and torch.isnan(y).all(), (M, K, N, ldx, ldy, act)


# =====================================================================================================================
# decoder row
# =====================================================================================================================
H = 8
ROW_KEYS = ("ca_in_w", "ca_in_b", "sa_out_w", "sa_out_b", "ca_out_w", "ca_out_b", "ln_g", "ln_b")


def _row_weights(D, seed=77):
    g = _gen(seed)
    rn = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale
    return dict(ca_in_w=rn(3 * D, D, scale=D ** -0.5), ca_in_b=rn(3 * D, scale=0.2), sa_out_w=rn(D, D, scale=D ** -0.5),
                sa_out_b=rn(D, scale=0.2), ca_out_w=rn(D, D, scale=D ** -0.5), ca_out_b=rn(D, scale=0.2),
                ln_g=1.0 + 0.2 * rn(D), ln_b=0.2 * rn(D))


def _row_problem(M, D, T, Lmax, step, samples=None, row_map=None, rows=None, anc=None, seed=0, mode="gauss", counts=None):
    """one layer's row step: inputs of M rows at position `step`.  Cache positions >= step hold NaN (uninitialised memory
    in production), earlier ones seeded values.  counts (kind 5): live hypotheses per sample -> seg + row_map."""
    g = _gen(1000 + seed)
    rn = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale
    hd = D // H
    if counts is not None:
        samples = len(counts)
        row_map = [n for n, c in enumerate(counts) for _ in range(c)]
        assert len(row_map) == M
    samples = samples or M
    rows = rows or M
    P = dict(_row_weights(D), M=M, D=D, T=T, Lmax=Lmax, step=step, samples=samples, rows=rows, counts=counts)
    P["qkv"], P["xres"] = rn(M, 3 * D), rn(M, D)
    P["sk"], P["sv"] = rn(rows, H, Lmax, hd), rn(rows, H, Lmax, hd)
    P["mem"] = rn(samples, T, D)
    if mode == "saturate":  # scores spread over about +-60: the softmax saturates to one key
        P["mem"] = P["mem"] * 20.0
        P["sk"] = P["sk"] * 10.0
    elif mode == "uniform":  # all memory rows of a sample equal: uniform attention
        P["mem"] = P["mem"][:, :1, :].expand(samples, T, D).clone()
    P["sk"][:, :, step:, :] = NAN
    P["sv"][:, :, step:, :] = NAN
    P["row_map"] = None if row_map is None else _i32(row_map)
    P["anc"] = None if anc is None else _i32(anc)
    return P


def _take_rows(P, idx):
    """the same problem restricted to / reordered as rows idx (each keeps its cache row, sample and ancestry)"""
    Q = dict(P)
    idx = list(idx)
    Q["M"] = Q["rows"] = len(idx)
    for k in ("qkv", "xres", "sk", "sv"):
        Q[k] = P[k][idx].clone()
    rm = P["row_map"] if P["row_map"] is not None else torch.arange(P["M"], dtype=torch.int32)
    Q["row_map"] = rm[idx].clone()
    if P["counts"] is not None:  # kind 5: rows stay grouped by sample, in sample order
        s = sorted(set(int(v) for v in Q["row_map"]))
        assert [int(v) for v in Q["row_map"]] == sorted(int(v) for v in Q["row_map"])
        Q["counts"] = [int((Q["row_map"] == n).sum()) for n in range(max(s) + 1)]
        Q["samples"] = len(Q["counts"])
        Q["mem"] = P["mem"][:Q["samples"]]
    assert P["anc"] is None
    return Q


def _split16(x32):
    """what the kernels split in registers (absorbed queries, probabilities): hi = upper 16 bits, lo = bf16_rne(x - hi)"""
    hi = (_bits(x32) & -65536).view(torch.float32)
    lo = (x32 - hi).to(torch.bfloat16).float()
    return hi.double(), lo.double()


def _split_planes(x32):
    """the memory planes (launch_split_bf16, csrc/kernels.h): hi = bf16_rne(x), lo = bf16_rne(x - hi)"""
    hi = x32.to(torch.bfloat16).float()
    lo = (x32 - hi).to(torch.bfloat16).float()
    return hi.double(), lo.double()


def _row_ref(P, dt, split=False):
    """nn.TransformerDecoderLayer (post-norm) up to the cross-attention block's residual sum, newest position only"""
    M, D, T, t = P["M"], P["D"], P["T"], P["step"]
    hd = D // H
    c = lambda k: P[k].to(dt)
    q, k, v = c("qkv").split(D, dim=1)
    sk, sv = c("sk"), c("sv")
    a = torch.zeros(M, D, dtype=dt)
    pos = torch.arange(t)
    for b in range(M):
        src = P["anc"][b, :t].long() if P["anc"] is not None else torch.full((t,), b, dtype=torch.long)
        K = torch.cat([sk[src, :, pos, :].permute(1, 0, 2), k[b].view(H, 1, hd)], 1)  # [H][t + 1][hd]
        V = torch.cat([sv[src, :, pos, :].permute(1, 0, 2), v[b].view(H, 1, hd)], 1)
        p = torch.softmax(torch.einsum("he,hje->hj", q[b].view(H, hd), K) / math.sqrt(hd), -1)
        a[b] = torch.einsum("hj,hje->he", p, V).reshape(D)
    x1 = F.layer_norm(a @ c("sa_out_w").T + c("sa_out_b") + c("xres"), (D,), c("ln_g"), c("ln_b"), 1e-5)
    wq, wk, wv = c("ca_in_w").split(D, dim=0)
    bq, bk, bv = c("ca_in_b").split(D)
    q2 = x1 @ wq.T + bq
    rm = P["row_map"].long() if P["row_map"] is not None else torch.arange(M)
    a2 = torch.zeros(M, D, dtype=dt)
    kv = {}
    for b in range(M):
        s = int(rm[b])
        if not split:
            if s not in kv:
                mem = c("mem")[s]
                kv[s] = ((mem @ wk.T + bk).view(T, H, hd), (mem @ wv.T + bv).view(T, H, hd))
            K2, V2 = kv[s]
            p = torch.softmax(torch.einsum("he,jhe->hj", q2[b].view(H, hd), K2) / math.sqrt(hd), -1)
            a2[b] = torch.einsum("hj,jhe->he", p, V2).reshape(D)
        else:  # absorbed form on hi + lo operands without the lo * lo product; float64 otherwise
            if s not in kv:
                kv[s] = _split_planes(P["mem"][s])
            mh, ml = kv[s]
            qp = torch.einsum("he,hec->hc", q2[b].view(H, hd), wk.view(H, hd, D)) / math.sqrt(hd)  # q'_h = W_k,h^T q_h
            qh, ql = _split16(qp.float())
            sc = qh @ mh.T + ql @ mh.T + qh @ ml.T  # [H][T]; b_k cancels in the softmax
            pr = torch.exp(sc - sc.max(-1, keepdim=True).values)
            ph, pl = _split16(pr.float())
            ctx = (ph @ mh + ph @ ml + pl @ mh) / pr.sum(-1, keepdim=True)  # [H][D]
            a2[b] = (torch.einsum("hc,hec->he", ctx, wv.view(H, hd, D)) + bv.view(H, hd)).reshape(D)
    return a2 @ c("ca_out_w").T + c("ca_out_b") + x1


def _row_run(kind, P, one_row=0, check_cache=True):
    """launch; returns y2 [M][D] (CPU).  The caches must be their old contents bit for bit except position `step` of the
    launched rows, which holds this step's k / v exactly."""
    lib = _lib.require_device()
    M, D = P["M"], P["D"]
    dv = {k: _d(P[k]) for k in ROW_KEYS + ("qkv", "xres", "sk", "sv", "mem", "row_map", "anc")}
    y2 = torch.full((M, D), NAN, device=DEV)
    step = _d(_i32([P["step"]]))
    seg, nseg = None, 0
    if kind == 5:
        first = np.concatenate([[0], np.cumsum(P["counts"])[:-1]])
        seg = _d(_i32(np.stack([first, P["counts"], np.zeros_like(first)], 1)))
        nseg = len(P["counts"])
    anc_stride = P["anc"].shape[1] if P["anc"] is not None else 0
    p = _lib.ptr
    rc = lib.d2t_op_decoder_row(kind, p(dv["qkv"]), p(dv["xres"]), p(dv["sk"]), p(dv["sv"]), p(dv["mem"]), p(dv["ca_in_w"]),
                                p(dv["ca_in_b"]), p(dv["sa_out_w"]), p(dv["sa_out_b"]), p(dv["ca_out_w"]), p(dv["ca_out_b"]),
                                p(dv["ln_g"]), p(dv["ln_b"]), 1e-5, p(y2), p(step), M, D, P["T"], P["Lmax"], P["rows"],
                                P["samples"], one_row, p(dv["row_map"]), p(dv["anc"]), anc_stride, p(seg), nseg,
                                _lib.stream_of(y2))
    torch.cuda.synchronize()
    assert rc == 0, f"d2t_op_decoder_row kind {kind}: rc {rc}"
    if check_cache:
        hd = D // H
        for name, off in (("sk", D), ("sv", 2 * D)):
            want = P[name].clone()
            want[:M, :, P["step"], :] = P["qkv"][:, off:off + D].view(M, H, hd)
            assert torch.equal(_bits(dv[name].cpu()), _bits(want)), f"{name}: cache differs from (old contents + this step's row)"
    return y2.cpu()


_REF_CACHE = {}


def _row_refs(key, P, split=False):
    if key not in _REF_CACHE:
        _REF_CACHE[key] = (_row_ref(P, torch.float64), _row_ref(P, torch.float32))
    r = _REF_CACHE[key]
    if split and len(r) == 2:
        r = _REF_CACHE[key] = r + (_row_ref(P, torch.float64, split=True),)
    return r


def _row_check(kind, P, key, one_row=0, name=None):
    name = name or f"row_kind{kind}"
    y = _row_run(kind, P, one_row)
    bx3 = kind in (3, 4)
    refs = _row_refs(key, P, split=bx3)
    y64, y32 = refs[0], refs[1]
    info = dict(M=P["M"], T=P["T"], step=P["step"], D=P["D"])
    if bx3:
        e32 = float((y32.double() - y64).abs().max())  # of the plain evaluation
        _measured(name + "_vs_split64", y, refs[2], e32=e32, **info)
        rel = float((y.double() - y64).abs().max() / y64.abs().max())
        _fig(name + "_vs_plain64", rel=rel, **info)
        assert rel <= 1e-3, f"{name}: {rel:.3e} relative to max |y64| against plain float64"
    else:
        _measured(name, y, y64, y32, **info)
    return y


def _perm_map(M, samples, seed):
    """rows -> samples with repeats and out of order"""
    r = np.random.RandomState(seed)
    m = r.randint(0, samples, size=M)
    m[: min(M, samples)] = r.permutation(samples)[: min(M, samples)]
    return m.tolist()


# (M, step, T, Lmax, samples (None: row b -> sample b), mode): every M, step, T of the issue's lists at least once
ROW_CASES = [
    (1, 0, 1, 64, None, "gauss"),
    (2, 1, 15, 64, None, "gauss"),
    (3, 63, 16, 64, None, "gauss"),       # step = Lmax - 1
    (5, 127, 17, 128, 3, "gauss"),        # step = Lmax - 1, repeated / permuted samples
    (64, 63, 261, 152, 7, "gauss"),
    (5, 1, 513, 64, None, "gauss"),
    (3, 0, 1695, 64, 2, "gauss"),
    (64, 1, 1695, 64, 3, "gauss"),
    (3, 63, 261, 152, None, "saturate"),
    (2, 5, 17, 64, None, "uniform"),
    (5, 0, 16, 64, 5, "gauss"),
    (1, 151, 513, 152, None, "gauss"),
]


def _case_problem(case, D=256, seed_off=0):
    M, step, T, Lmax, samples, mode = case
    rm = _perm_map(M, samples, M + T) if samples else None
    return _row_problem(M, D, T, Lmax, step, samples=samples, row_map=rm, seed=M * 31 + T + step + seed_off, mode=mode)


@pytest.mark.parametrize("kind", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("ci", range(len(ROW_CASES)))
def test_decoder_row_vs_float64(kind, ci):
    P = _case_problem(ROW_CASES[ci])
    _row_check(kind, P, ("c", ci), one_row=0)


@pytest.mark.parametrize("one_row", [0, 1])
@pytest.mark.parametrize("ci", [0, 1, 2, 3, 4, 5, 8, 9])
def test_decoder_row_projected_d512_vs_float64(one_row, ci):
    P = _case_problem(ROW_CASES[ci], D=512)
    _row_check(0, P, ("c512", ci), one_row=one_row, name=f"row_kind0_d512_{'one' if one_row else 'two'}")


# kind 5: live hypotheses per sample (1-6, unequal, a finished sample with none), step, T, Lmax, mode
BEAM_ROW_CASES = [
    ([1], 0, 1, 64, "gauss"),
    ([2], 1, 15, 64, "gauss"),
    ([3], 63, 16, 64, "gauss"),
    ([5], 127, 17, 128, "gauss"),
    ([6, 1, 4], 1, 261, 152, "gauss"),
    ([2, 0, 3], 5, 513, 64, "gauss"),
    ([5, 6, 1, 4, 2, 3, 6, 5, 0, 4, 6, 3, 5, 2, 6, 6], 63, 1695, 64, "gauss"),  # 64 rows
    ([1, 2], 0, 1695, 64, "gauss"),
    ([3, 2], 63, 261, 152, "saturate"),
    ([2, 4], 3, 17, 64, "uniform"),
]


@pytest.mark.parametrize("ci", range(len(BEAM_ROW_CASES)))
def test_decoder_row_beam_split_vs_float64(ci):
    counts, step, T, Lmax, mode = BEAM_ROW_CASES[ci]
    P = _row_problem(sum(counts), 256, T, Lmax, step, counts=counts, seed=50 + ci, mode=mode)
    _row_check(5, P, ("b", ci))


@pytest.mark.parametrize("kind", [2, 4])
@pytest.mark.parametrize("step", [0, 1, 63, 511])
def test_decoder_row_ancestry(kind, step):
    """every earlier position of a hypothesis lives in some other cache row (Lmax = ANC_MAX = 512)"""
    M, rows, Lmax = 5, 12, 512
    r = np.random.RandomState(step)
    anc = r.randint(0, rows, size=(M, Lmax))
    P = _row_problem(M, 256, 261, Lmax, step, samples=3, row_map=_perm_map(M, 3, 9), rows=rows, anc=anc, seed=step)
    _row_check(kind, P, ("anc", step), name=f"row_kind{kind}_anc")


def test_decoder_row_two_row_build_equals_one_row_build_d512():
    """decoder_row2_kernel: 'per row bit-identical to the one-row kernel'"""
    for ci in (0, 1, 3, 4):
        P = _case_problem(ROW_CASES[ci], D=512)
        y2 = _row_run(0, P, one_row=0)
        y1 = _row_run(0, P, one_row=1)
        assert torch.equal(_bits(y2), _bits(y1)), f"case {ci}: two-row and one-row builds differ"


@pytest.mark.parametrize("kind", [0, 1, 2, 3, 4, 5, "0_d512"])
def test_decoder_row_result_does_not_depend_on_the_launch(kind):
    """a row's y2 is the same bits alone (M = 1) and inside M = 2, 5 and 64, at the first and at the last position"""
    D = 512 if kind == "0_d512" else 256
    k = 0 if kind == "0_d512" else kind
    if k == 5:
        counts = [5, 6, 1, 4, 2, 3, 6, 5, 1, 4, 6, 3, 5, 2, 5, 6]  # 64 rows; row 0 = sample 0, row 63 = sample 15
        base = _row_problem(64, D, 261, 64, 7, counts=counts, seed=3)
    else:
        base = _row_problem(64, D, 261, 64, 7, samples=5, row_map=_perm_map(64, 5, 4), seed=3)
    y_all = _row_run(k, base)
    for probe in (0, 63):
        alone = _row_run(k, _take_rows(base, [probe]))
        assert torch.equal(_bits(alone[0]), _bits(y_all[probe])), f"row {probe}: M = 1 differs from M = 64"
        others = [r for r in (9, 20, 33, 47) if r != probe]
        for idx in ([probe] + others, others + [probe], [probe, 33], [33, probe]):
            if k == 5:
                idx = sorted(idx)
            y = _row_run(k, _take_rows(base, idx))
            assert torch.equal(_bits(y[idx.index(probe)]), _bits(alone[0])), f"row {probe} inside rows {idx} differs from M = 1"


@pytest.mark.parametrize("pair", [(1, 2), (3, 4)])
def test_decoder_row_absorbed_one_row_against_two_row_build(pair):
    """the absorbed one-row and two-row builds sum their GEMV groups in a different association and promise agreement to
    fp32 rounding only.  Measured on an MI355X: max |difference| 9.5e-7 ... 1.4e-6 (kinds 1 / 2) and 1.2e-6 ... 3.8e-6
    (kinds 3 / 4) on outputs of magnitude 4-5 -- not zero, so the measured rule stays."""
    worst = 0.0
    for ci in (1, 3, 4, 6):
        P = _case_problem(ROW_CASES[ci])
        ya, yb = _row_run(pair[0], P), _row_run(pair[1], P)
        y64, y32 = _row_refs(("c", ci), P)[:2]
        e32 = float((y32.double() - y64).abs().max())
        diff = float((ya - yb).abs().max())
        worst = max(worst, diff)
        _fig(f"row_kind{pair[0]}_vs_kind{pair[1]}", diff=diff, e32=e32, M=P["M"], T=P["T"])
        assert diff <= 8 * e32 + 1e-6 * float(y64.abs().max())
    _fig(f"row_kind{pair[0]}_vs_kind{pair[1]}_worst", diff=worst)


def test_decoder_row_refuses_out_of_range_arguments():
    P = _case_problem(ROW_CASES[1])
    lib = _lib.require_device()

    def rc_of(kind, **kw):
        Q = dict(P)
        Q.update(kw)
        dv = {k: _d(Q[k]) for k in ROW_KEYS + ("qkv", "xres", "sk", "sv", "mem")}
        y2 = torch.full((Q["M"], Q["D"]), NAN, device=DEV)
        step = _d(_i32([Q["step"]]))
        rm, anc, seg = _d(Q.get("row_map")), _d(Q.get("anc")), _d(Q.get("seg"))
        p = _lib.ptr
        rc = lib.d2t_op_decoder_row(kind, p(dv["qkv"]), p(dv["xres"]), p(dv["sk"]), p(dv["sv"]), p(dv["mem"]), p(dv["ca_in_w"]),
                                    p(dv["ca_in_b"]), p(dv["sa_out_w"]), p(dv["sa_out_b"]), p(dv["ca_out_w"]), p(dv["ca_out_b"]),
                                    p(dv["ln_g"]), p(dv["ln_b"]), 1e-5, p(y2), p(step), Q["M"], Q["D"], Q["T"], Q["Lmax"],
                                    Q["rows"], Q["samples"], 0, p(rm), p(anc), Q.get("anc_stride", 0), p(seg), Q.get("nseg", 0),
                                    _lib.stream_of(y2))
        torch.cuda.synchronize()
        assert torch.isnan(y2).all()
        return rc
    assert rc_of(1, step=64) == EINVAL and rc_of(1, step=-1) == EINVAL          # beyond the cache
    assert rc_of(1, row_map=_i32([0, 2])) == EINVAL                            # a sample that does not exist
    assert rc_of(1, samples=1) == EINVAL                                       # row 1 has no sample
    assert rc_of(1, D=512) == EINVAL and rc_of(6) == EINVAL and rc_of(0, D=384) == EINVAL
    assert rc_of(1, anc=_i32(np.zeros((2, 64))), anc_stride=64) == EINVAL      # ancestry: one-row absorbed builds only
    assert rc_of(2, anc=_i32(np.full((2, 64), 2)), anc_stride=64) == EINVAL    # a cache row that does not exist
    assert rc_of(5, row_map=_i32([0, 0]), seg=_i32([[0, 7, 0]]), nseg=1) == EINVAL   # more than 6 hypotheses / rows != M
    assert rc_of(5, row_map=_i32([0, 1]), seg=_i32([[0, 2, 0]]), nseg=1) == EINVAL   # row_map disagrees with seg


# =====================================================================================================================
# argmax + embed
# =====================================================================================================================
def _grid_logits(shape, g):
    """random multiples of 1/4 in [-10, 10]: ties are exact in any arithmetic, non-tied values 1/4 apart"""
    return torch.randint(-40, 41, shape, generator=g).float() / 4.0


class _ArgmaxState:
    """device state of launch_argmax_embed + the Python model of one launch"""

    def __init__(self, B, S, V, d, end, rpb=0, nb=0, with_stop=True, seed=0):
        g = _gen(seed)
        self.B, self.S, self.V, self.d, self.end, self.rpb, self.nb = B, S, V, d, end, rpb, nb
        self.emb = torch.randn(V, d, generator=g)
        self.pe = torch.randn(S + 1, d, generator=g)
        self.m = dict(tokens=np.full((B, S), -1, np.int64), ended=np.zeros(B, np.int32), end_count=np.zeros(1, np.int32),
                      steps_done=np.zeros(1, np.int32), step=np.zeros(1, np.int32), done_count=np.zeros(1, np.int32))
        if nb:
            self.m.update(bec=np.zeros(nb, np.int32), bsd=np.zeros(nb, np.int32), bdone=np.zeros(1, np.int32))
            if with_stop:
                self.m["stop_at"] = np.zeros(1, np.int32)
        self.x_model = np.full((B, d), np.nan)
        self.x_tol = np.zeros((B, d))
        self.dv = {k: torch.as_tensor(v).to(DEV) for k, v in self.m.items()}
        self.x = torch.full((B, d), NAN, device=DEV)
        self.emb_d, self.pe_d = _d(self.emb), _d(self.pe)

    def model_step(self, logits):  # logits [B][S][V] numpy
        m = self.m
        t = int(m["step"][0])
        if "stop_at" in m and m["stop_at"][0] and t >= m["stop_at"][0]:
            return
        for b in range(self.B):
            tok = int(np.argmax(logits[b, t]))  # first maximum
            m["tokens"][b, t] = tok
            if tok == self.end and not m["ended"][b]:
                m["ended"][b] = 1
                m["end_count"][0] += 1
                if m["end_count"][0] == self.B:
                    m["steps_done"][0] = t + 1
                if self.nb:
                    k = b // self.rpb
                    m["bec"][k] += 1
                    if m["bec"][k] == self.rpb:
                        m["bsd"][k] = t + 1
                        m["bdone"][0] += 1
                        if m["bdone"][0] == self.nb and "stop_at" in m:
                            m["stop_at"][0] = t + 1
            e, pe = self.emb[tok].double().numpy() * math.sqrt(self.d), self.pe[t + 1].double().numpy()
            self.x_model[b] = e + pe
            self.x_tol[b] = 2 * U * (np.abs(e) + np.abs(pe))
        m["step"][0] = t + 1

    def launch(self, logits_d):
        lib = _lib.require_device()
        p, dv = _lib.ptr, self.dv
        rc = lib.d2t_op_argmax_embed(p(logits_d), self.S, p(dv["tokens"]), p(dv["ended"]), p(dv["end_count"]), p(dv["steps_done"]),
                                     p(dv["step"]), p(dv["done_count"]), p(dv.get("bec")), p(dv.get("bsd")), p(dv.get("bdone")),
                                     p(dv.get("stop_at")), p(self.emb_d), p(self.pe_d), p(self.x), self.B, self.V, self.d, self.end,
                                     self.rpb, self.nb, _lib.stream_of(self.x))
        torch.cuda.synchronize()
        assert rc == 0

    def compare(self, where):
        for k, v in self.m.items():
            got = self.dv[k].cpu().numpy()
            assert np.array_equal(got, v), f"{where}: {k} = {got.tolist()} but the model has {v.tolist()}"
        x = self.x.cpu().double().numpy()
        assert not np.isnan(x).any() or np.isnan(self.x_model).all(), f"{where}: x has unwritten elements"
        if not np.isnan(self.x_model).all():
            assert (np.abs(x - self.x_model) <= self.x_tol).all(), f"{where}: x = emb sqrt(d) + pe beyond 2 * 2^-24 (|.| + |.|)"


@pytest.mark.parametrize("V", [64, 93, 500, 1000, 16384])
def test_argmax_first_maximum_under_ties(V):
    g = _gen(V)
    rows = []  # (logit row, expected token)

    def base():
        return _grid_logits((V,), g)
    if V > 64:
        for i in (0, 5, V - 65):  # the maximum twice in one lane's stride
            r = base(); r[i] = r[i + 64] = 11.0; rows.append((r, i))
        r = base(); r[3] = r[3 + 64] = r[3 + 128 if V > 131 else 3] = 11.0; rows.append((r, 3))
    for i, j in ((2, 7), (0, 63), (31, 32), (V - 2, V - 1)):  # in two lanes of one wave
        r = base(); r[i] = r[j] = 11.0; rows.append((r, i))
    r = base(); r[V - 1] = r[0] = 11.0; rows.append((r, 0))
    r = base(); r[V - 1] = 11.0; rows.append((r, V - 1))
    rows.append((torch.full((V,), 2.5), 0))  # all equal
    r = torch.full((V,), -math.inf); r[V // 2] = -3.0; rows.append((r, V // 2))
    r = torch.full((V,), -math.inf); r[V - 1] = -50.0; rows.append((r, V - 1))
    r = base(); r[V // 3] = math.inf; rows.append((r, V // 3))
    r = base(); r[V - 1] = r[7] = math.inf; rows.append((r, 7))
    for _ in range(3):  # the grid alone: the largest level occurs many times in a long row
        r = base(); rows.append((r, int(np.argmax(r.numpy()))))
    B, S = len(rows), 2
    logits = torch.zeros(B, S, V)
    for b, (r, _) in enumerate(rows):
        logits[b, 0] = r
        logits[b, 1] = r.flip(0)  # second step: the mirrored rows
    st = _ArgmaxState(B, S, V, 64, end=V - 1 if V > 64 else 1, seed=V)
    ld, ln = _d(logits), logits.numpy()
    for t in range(S):
        st.model_step(ln)
        st.launch(ld)
        st.compare(f"V = {V}, step {t}")
    assert st.m["tokens"][:, 0].tolist() == [e for _, e in rows]  # the model itself: lowest index
    for b, (r, _) in enumerate(rows):
        f = r.flip(0).numpy()
        assert st.m["tokens"][b, 1] == int(np.flatnonzero(f == f.max())[0])


@pytest.mark.parametrize("B,S,V,rpb,nb,with_stop", [
    (5, 8, 93, 0, 0, False), (64, 8, 16384, 0, 0, False), (6, 8, 500, 3, 2, True), (12, 8, 1000, 4, 3, True),
    (6, 8, 64, 2, 3, False), (64, 6, 93, 32, 2, True), (1, 4, 93, 1, 1, True)])
def test_argmax_embed_bookkeeping_over_steps(B, S, V, rpb, nb, with_stop):
    """rows end at chosen steps (some twice, some never); every integer after every launch equals the Python model; after
    stop_at a launch leaves everything alone"""
    g = _gen(B * 100 + V)
    end = 1
    logits = _grid_logits((B, S, V), g)
    logits[:, :, end] = -20.0
    end_at = torch.randint(0, S - 2, (B,), generator=g)  # every row ends before the last two steps ...
    if not with_stop:
        end_at[0] = S + 5  # ... unless nothing stops the loop: then one row never does
    for b in range(B):
        for t in (int(end_at[b]), int(end_at[b]) + 1 if b % 3 == 0 else -1):  # every third row emits [s] again
            if 0 <= t < S:
                logits[b, t, end] = 20.0
    st = _ArgmaxState(B, S, V, 256, end, rpb, nb, with_stop, seed=B + V)
    ld, ln = _d(logits), logits.numpy()
    stopped_seen = False
    for t in range(S):
        before = int(st.m["step"][0])
        st.model_step(ln)
        st.launch(ld)
        st.compare(f"launch {t}")
        if int(st.m["step"][0]) == before:
            stopped_seen = True
    if with_stop:
        assert stopped_seen and st.m["stop_at"][0] == int(end_at.max()) + 1 and st.m["bdone"][0] == nb
    else:
        assert st.m["step"][0] == S
        assert (st.m["steps_done"][0] == 0) == bool(end_at.max() >= S)


def test_argmax_embed_refuses_a_step_beyond_its_buffers():
    st = _ArgmaxState(2, 2, 93, 64, 1)
    ld = _d(_grid_logits((2, 2, 93), _gen(0)))
    st.dv["step"].fill_(2)
    lib = _lib.require_device()
    p, dv = _lib.ptr, st.dv
    rc = lib.d2t_op_argmax_embed(p(ld), 2, p(dv["tokens"]), p(dv["ended"]), p(dv["end_count"]), p(dv["steps_done"]), p(dv["step"]),
                                 p(dv["done_count"]), None, None, None, None, p(st.emb_d), p(st.pe_d), p(st.x), 2, 93, 64, 1, 0, 0,
                                 _lib.stream_of(st.x))
    assert rc == EINVAL and (dv["tokens"].cpu() == -1).all()


# =====================================================================================================================
# beam top-k
# =====================================================================================================================
def _topk_segment(m, V, g, dup_rows=(), plant=(), ninf=0.0):
    """logits [m][V] on the 1/4 grid and scores = fp32(lse64 + a/4 + pi/64): candidates of different rows are >= 1/64
    apart, equal ones are exactly equal.  dup_rows: (i, j) row j becomes a copy of row i with the same score.
    plant: (row, column) entries raised to 10.25 (above the grid).  ninf: share of -inf logits."""
    lg = _grid_logits((m, V), g)
    if ninf:
        lg[torch.rand(m, V, generator=g) < ninf] = -math.inf
        lg[:, 0] = torch.where(torch.isinf(lg[:, 0]), torch.zeros(m), lg[:, 0])  # every row keeps a finite entry
    for r, c in plant:
        lg[r, c] = 10.25
    for i, j in dup_rows:
        lg[j] = lg[i]
    lse = torch.logsumexp(lg.double(), 1)
    a = torch.randint(-8, 9, (m,), generator=g).double()
    pi = torch.randperm(m, generator=g).double()
    for r, _ in plant:  # the planted rows lead
        a[r] = 9.0
    for i, j in dup_rows:
        a[j], pi[j] = a[i], pi[i]
    sc = (lse + a / 4 + pi / 64).float()
    for i, j in dup_rows:
        assert sc[i] == sc[j]
    return lg, sc


def _topk_expected(lg, sc, k, tol_factor=8.0):
    """float64 candidates, their k best by (value descending, flat index ascending), the value tolerance of the measured
    rule, and the gap condition: ranks 1 .. k + 1 are exact ties or further apart than ten tolerances"""
    c64 = (sc.double()[:, None] + F.log_softmax(lg.double(), 1)).reshape(-1)
    c32 = (sc[:, None] + F.log_softmax(lg, 1)).reshape(-1)
    fin = torch.isfinite(c64)
    e32 = float((c32.double() - c64)[fin].abs().max())
    tol = tol_factor * e32 + 1e-6 * float(c64[fin].abs().max())
    v = c64.numpy()
    order = np.lexsort((np.arange(v.size), -v))[: k + 1]
    top = v[order]
    with np.errstate(invalid="ignore"):  # -inf next to -inf: an exact tie
        gaps = top[:-1] - top[1:]
        ok = (top[:-1] == top[1:]) | (gaps > 10 * tol)
    assert ok.all(), f"test construction: candidates closer than ten tolerances ({gaps.min():.3e} vs {tol:.3e})"
    return order[:k], top[:k], tol, e32


def _tie_shapes(idx, val):
    """which stages of the kernel's reduction the exact ties among the selected candidates exercise"""
    s = set()
    for a in range(len(idx)):
        for b in range(a + 1, len(idx)):
            if val[a] == val[b]:
                ta, tb = idx[a] % 256, idx[b] % 256  # idx[a] < idx[b]: the expected order
                if ta == tb:
                    s.add("same_thread")
                elif ta // 64 == tb // 64:
                    s.add("same_wave")
                elif tb // 64 < ta // 64:
                    s.add("later_index_in_earlier_wave")
                else:
                    s.add("other_wave")
    return s


def _run_topk(segs, V, kmax, rows_total, logits, scores):
    lib = _lib.require_device()
    N = len(segs)
    ld, sd, sg = _d(logits), _d(scores), _d(_i32(segs))
    topv = torch.full((N, kmax), NAN, device=DEV)
    topi = torch.full((N, kmax), -1, dtype=torch.int32, device=DEV)
    rc = lib.d2t_op_beam_topk(_lib.ptr(ld), _lib.ptr(sd), _lib.ptr(sg), N, rows_total, V, kmax, _lib.ptr(topv), _lib.ptr(topi),
                              _lib.stream_of(ld))
    torch.cuda.synchronize()
    assert rc == 0
    return topv.cpu().numpy(), topi.cpu().numpy()


def _check_topk(parts, V, kmax, want_shapes=()):
    """parts: per segment (logits [m][V] or None, scores, k)"""
    segs, lgs, scs, off = [], [], [], 0
    for lg, sc, k in parts:
        m = 0 if lg is None else lg.shape[0]
        segs.append((off, m, k))
        if m:
            lgs.append(lg); scs.append(sc)
        off += m
    topv, topi = _run_topk(segs, V, kmax, off, torch.cat(lgs), torch.cat(scs))
    shapes, worst = set(), (0.0, 0.0)
    for n, (lg, sc, k) in enumerate(parts):
        if lg is None or k == 0:
            assert np.isnan(topv[n]).all() and (topi[n] == -1).all(), f"segment {n} (no rows or k = 0) was written"
            continue
        idx, val, tol, e32 = _topk_expected(lg, sc, k)
        got_i, got_v = topi[n, :k], topv[n, :k].astype(np.float64)
        assert len(set(got_i.tolist())) == k and (got_i >= 0).all() and (got_i < lg.numel()).all(), f"segment {n}: indices {got_i}"
        assert np.array_equal(got_i, idx), f"segment {n}: indices {got_i.tolist()} expected {idx.tolist()}"
        fin = np.isfinite(val)
        assert np.array_equal(got_v[~fin], val[~fin])
        err = float(np.abs(got_v[fin] - val[fin]).max()) if fin.any() else 0.0
        assert err <= tol, f"segment {n}: values off by {err:.3e} (tolerance {tol:.3e})"
        if err > worst[0]:
            worst = (err, e32)
        assert np.isnan(topv[n, k:]).all() and (topi[n, k:] == -1).all(), f"segment {n}: slots beyond k were written"
        shapes |= _tie_shapes(idx.tolist(), val.tolist())
    _fig("beam_topk", V=V, N=len(parts), err=worst[0], e32=worst[1], ratio=worst[0] / worst[1] if worst[1] else 0.0)
    for s in want_shapes:
        assert s in shapes, f"test construction: no exact tie of kind {s} among the selected candidates ({shapes})"


def _planted_columns(V, m):
    """columns of the leading row such that ties fall in one thread (flat index 256 apart), in two lanes of a wave and
    in two waves with the later index in the earlier wave"""
    if V >= 500:
        return [(0, 70), (0, 71), (0, 70 + 256), (0, 260), (0, 130)]  # threads 70, 71, 70 again, 4 (wave 0 after wave 1), 130
    return []


@pytest.mark.parametrize("V", [93, 500, 16384])
@pytest.mark.parametrize("N", [1, 7, 64])
def test_beam_topk_vs_float64(V, N):
    g = _gen(V * 100 + N)
    parts = []
    for n in range(N):
        m = (1, 16, 5, 10, 2, 7, 13)[n % 7] if N > 1 else 16
        k = (16, 5, 1, 10, 3, 16, 8)[(n + n // 7) % 7] if N > 1 else 16
        if V == 16384 and N == 64 and n % 4:
            m = min(m, 3)  # the expensive size a few times, not 64 times
        if n % 9 == 4:
            parts.append((None, None, k))  # no rows
            continue
        if n % 9 == 6:
            k = 0
        lg, sc = _topk_segment(m, V, g)
        parts.append((lg, sc, min(k, m * V)))
    _check_topk(parts, V, 16)


@pytest.mark.parametrize("V", [93, 500, 16384])
def test_beam_topk_exact_ties_take_the_lower_flat_index(V):
    g = _gen(V + 1)
    parts = []
    if V >= 500:
        # one leading row with its maximum five times: ties inside one thread's scan, one wave's shuffles, across waves
        lg, sc = _topk_segment(16, V, g, plant=_planted_columns(V, 16))
        parts.append((lg, sc, 16))
    # whole rows duplicated with equal scores (rows 1 / 3 / 4, 2 / 5 and 0 / 15), the maximum planted twice in each of the
    # leading three: at V = 93 their flat indices 100, 123 | 286, 309 | 379, 402 sit in threads 100, 123 | 30, 53 | 123, 146
    plant = [(1, 30), (1, 7)] if V == 93 else [(1, 30), (1, 286)]
    lg, sc = _topk_segment(16, V, g, dup_rows=[(1, 3), (1, 4), (2, 5), (0, 15)], plant=plant)
    parts.append((lg, sc, 16))
    lg, sc = _topk_segment(7, V, g, dup_rows=[(0, 6), (0, 3)])
    parts.append((lg, sc, 9))
    lg, sc = _topk_segment(2, V, g, dup_rows=[(0, 1)])
    parts.append((lg, sc, 16))
    _check_topk(parts, V, 16, want_shapes=("same_thread", "same_wave", "later_index_in_earlier_wave"))


@pytest.mark.parametrize("V", [93, 500])
def test_beam_topk_rows_with_minus_inf_logits(V):
    g = _gen(V + 2)
    parts = []
    lg = torch.full((1, V), -math.inf)
    lg[0, [3, 50, 51, 77, 92]] = torch.tensor([1.0, 2.5, 2.5, -4.0, 0.25])  # five finite candidates, k = 16
    parts.append((lg, torch.tensor([0.5]), 16))
    for m, k in ((4, 16), (16, 16), (2, 7)):
        lg, sc = _topk_segment(m, V, g, ninf=0.5)
        parts.append((lg, sc, k))
    lg = torch.full((3, V), -math.inf)
    lg[:, 0] = 0.0  # one finite candidate per row
    parts.append((lg, torch.tensor([0.0, 0.25, -0.25]), 8))
    _check_topk(parts, V, 16)


def test_beam_topk_refuses_out_of_range_segments():
    lib = _lib.require_device()
    lg, sc = _d(torch.zeros(4, 93)), _d(torch.zeros(4))
    for seg, kmax in (([[0, 17, 1]], 16), ([[2, 3, 1]], 16), ([[0, 4, 9]], 8), ([[0, 1, 1]], 17), ([[-1, 2, 1]], 16)):
        topv = torch.full((1, 16), NAN, device=DEV)
        topi = torch.full((1, 16), -1, dtype=torch.int32, device=DEV)
        sg = _d(_i32(seg))
        rc = lib.d2t_op_beam_topk(_lib.ptr(lg), _lib.ptr(sc), _lib.ptr(sg), 1, 4, 93, kmax, _lib.ptr(topv), _lib.ptr(topi),
                                  _lib.stream_of(lg))
        torch.cuda.synchronize()
        assert rc == EINVAL and torch.isnan(topv).all(), seg


# =====================================================================================================================
# device-side Beam.advance
# =====================================================================================================================
class _BeamModel:
    """Beam.advance (tools/beam.py) for N samples at once, as csrc/kernels.h documents struct BeamDev: written from the
    documented behaviour, as oracle/restatement.py:tfm_beam restates it for one sample"""
    INT = ("ctrl", "map", "prev", "seg", "comp_n", "fin", "comp_t", "comp_par", "hist_par", "hist_tok")

    def __init__(self, N, beam, cap, S, V, end, go):
        self.N, self.beam, self.cap, self.S, self.V, self.end = N, beam, cap, S, V, end
        a = self.a = dict(ctrl=np.full(4, -1, np.int32), tok=np.full(cap, -1, np.int64), scores=np.full(cap, np.nan, np.float32),
                          map=np.full(cap, -1, np.int32), prev=np.full(cap, -1, np.int32), seg=np.full((N, 3), -1, np.int32),
                          comp_n=np.full(N, -1, np.int32), fin=np.full(N, -1, np.int32), comp_t=np.full((N, beam), -1, np.int32),
                          comp_par=np.full((N, beam), -1, np.int32), comp_score=np.full((N, beam), np.nan, np.float32),
                          hist_par=np.full((S, cap), -1, np.int32), hist_tok=np.full((S, cap), -1, np.int32))
        self.dv = {k: torch.as_tensor(v).to(DEV) for k, v in a.items()}
        # init
        a["seg"][:, 0] = np.arange(N); a["seg"][:, 1] = 1; a["seg"][:, 2] = beam
        a["tok"][:N] = go; a["scores"][:N] = 0; a["map"][:N] = np.arange(N); a["prev"][:N] = np.arange(N)
        a["comp_n"][:] = 0; a["fin"][:] = 0
        a["ctrl"][:] = (0, N, 0, 0)
        self.go = go

    def advance(self, topv, topi):
        a, beam, V = self.a, self.beam, self.V
        t = int(a["ctrl"][0])
        if a["ctrl"][2] and t >= a["ctrl"][2]:
            return
        new = []
        for i in range(self.N):
            rows = []
            if not a["fin"][i] and a["seg"][i, 1] > 0:
                off, live, cn = int(a["seg"][i, 0]), int(a["seg"][i, 2]), int(a["comp_n"][i])
                for r in range(live):
                    idx = int(topi[i, r]); prev, word = idx // V, idx % V
                    if word == self.end:  # a completed hypothesis: (step, parent row, score)
                        a["comp_t"][i, cn], a["comp_par"][i, cn], a["comp_score"][i, cn] = t, off + prev, topv[i, r]
                        cn += 1
                    else:
                        rows.append((off + prev, word, topv[i, r]))
                a["comp_n"][i] = cn
                if cn == beam:  # Beam.done
                    a["fin"][i] = 1
                    rows = []
            new.append(rows)
        run = 0
        for i, rows in enumerate(new):  # rows stay compact, in sample order
            for j, (par, word, val) in enumerate(rows):
                row = run + j
                a["tok"][row], a["scores"][row], a["map"][row], a["prev"][row] = word, val, i, par
                a["hist_par"][t, row], a["hist_tok"][t, row] = par, word
            a["seg"][i] = (run, len(rows), 0 if a["fin"][i] else beam - a["comp_n"][i])
            run += len(rows)
        a["ctrl"][0] = a["ctrl"][3] = t + 1
        a["ctrl"][1] = run
        if run == 0:
            a["ctrl"][2] = t + 1

    def launch(self, init, topv=None, topi=None):
        lib = _lib.require_device()
        p, d = _lib.ptr, self.dv
        tv = None if topv is None else _d(torch.as_tensor(topv))
        ti = None if topi is None else _d(torch.as_tensor(topi))
        rc = lib.d2t_op_beam_advance(init, self.go, p(d["ctrl"]), p(d["tok"]), p(d["scores"]), p(d["map"]), p(d["prev"]), p(d["seg"]),
                                     p(d["comp_n"]), p(d["fin"]), p(d["comp_t"]), p(d["comp_par"]), p(d["comp_score"]),
                                     p(d["hist_par"]), p(d["hist_tok"]), p(tv), p(ti), self.N, self.beam, self.cap, self.V, self.S,
                                     self.end, _lib.stream_of(d["ctrl"]))
        torch.cuda.synchronize()
        assert rc == 0

    def compare(self, where):
        for k, v in self.a.items():
            got = self.dv[k].cpu().numpy()
            same = np.array_equal(got, v) if k in self.INT or k == "tok" else np.array_equal(got.view(np.int32), v.view(np.int32))
            if not same:
                bad = np.argwhere(got != v)[:5].tolist() if k in self.INT or k == "tok" else "(bits)"
                raise AssertionError(f"{where}: {k} differs from the Python restatement at {bad}")


@pytest.mark.parametrize("N", [1, 5, 256, 257, 700, 1024])
@pytest.mark.parametrize("beam", [1, 5, 16])
def test_beam_advance_matches_the_python_restatement(N, beam):
    V, S, end, steps = 93, 16, 1, 14
    r = np.random.RandomState(N * 17 + beam)
    bm = _BeamModel(N, beam, N * beam, S, V, end, go=2)
    bm.launch(1)
    bm.compare("init")
    rate = r.choice([1.0, 0.5, 0.15, 0.0], size=N, p=[0.1, 0.3, 0.4, 0.2])  # some samples finish at the first step
    finished_at = set()
    for t in range(steps):
        a = bm.a
        topv = np.full((N, beam), np.nan, np.float32)
        topi = np.full((N, beam), -1, np.int32)
        for i in range(N):
            m, live = int(a["seg"][i, 1]), int(a["seg"][i, 2])
            if a["fin"][i] or m <= 0:
                continue
            par = r.randint(0, m, size=live)
            word = r.randint(2, V, size=live)
            word[r.rand(live) < (1.0 if t >= 10 else rate[i])] = end  # from step 10 on everything ends
            topi[i, :live] = par * V + word
            topv[i, :live] = np.sort(r.randn(live).astype(np.float32) - t)[::-1]
        bm.advance(topv, topi)
        bm.launch(0, topv, topi)
        bm.compare(f"step {t}")
        if bm.a["ctrl"][2]:
            finished_at.add(int(bm.a["ctrl"][2]))
    assert bm.a["fin"].all() and bm.a["ctrl"][1] == 0 and len(finished_at) == 1 and bm.a["ctrl"][2] <= 12
    if N >= 256:
        first = np.array([bm.a["comp_t"][i].max() for i in range(N)])
        assert (first == 0).any() and len(set(first.tolist())) > 3  # samples finished at different steps, some at once
    # nothing is left: a further launch is a no-op
    topv = np.zeros((N, beam), np.float32)
    topi = np.full((N, beam), 5, np.int32)
    bm.advance(topv, topi)
    bm.launch(0, topv, topi)
    bm.compare("after the end")


def test_beam_advance_refuses_out_of_range_state():
    bm = _BeamModel(3, 4, 12, 4, 93, 1, go=2)
    bm.launch(1)
    lib = _lib.require_device()
    p, d = _lib.ptr, bm.dv

    def rc_of(topi, N=3, beam=4):
        tv, ti = _d(torch.zeros(3, 4)), _d(_i32(topi))
        rc = lib.d2t_op_beam_advance(0, 2, p(d["ctrl"]), p(d["tok"]), p(d["scores"]), p(d["map"]), p(d["prev"]), p(d["seg"]),
                                     p(d["comp_n"]), p(d["fin"]), p(d["comp_t"]), p(d["comp_par"]), p(d["comp_score"]),
                                     p(d["hist_par"]), p(d["hist_tok"]), p(tv), p(ti), N, beam, 12 if N == 3 else N * beam, 93, 4, 1,
                                     _lib.stream_of(tv))
        torch.cuda.synchronize()
        return rc
    ok = np.full((3, 4), 7)
    bad = ok.copy(); bad[1, 2] = 93 + 7  # parent 1 of a sample with one live row
    assert rc_of(bad) == EINVAL and rc_of(-ok) == EINVAL
    assert rc_of(ok, N=1025) == EINVAL and rc_of(ok, beam=17) == EINVAL
    bm.compare("after refused launches")  # nothing ran


# =====================================================================================================================
# ancestry table, cache gather
# =====================================================================================================================
@pytest.mark.parametrize("rows,stride,step,rows_live,stop", [
    (7, 64, 0, None, None), (7, 64, 1, None, None), (7, 64, 2, None, None), (7, 64, 63, None, None), (7, 64, 64, None, None),
    (640, 512, 511, None, None), (640, 152, 77, 333, None), (12, 64, 5, 0, None), (12, 64, 5, 12, 0), (12, 64, 5, None, 5),
    (12, 64, 5, None, 6), (12, 64, 5, 4, 3), (1, 16, 15, None, None)])
def test_beam_ancestry_exact(rows, stride, step, rows_live, stop):
    lib = _lib.require_device()
    r = np.random.RandomState(rows + step)
    old = r.randint(0, rows, size=(rows, stride)).astype(np.int32)
    prev = r.randint(0, rows, size=rows).astype(np.int32)
    want = np.full((rows, stride), -1, np.int32)
    stopped = stop is not None and stop != 0 and step >= stop
    if step >= 1 and not stopped:
        for row in range(rows if rows_live is None else rows_live):
            want[row, : step - 1] = old[prev[row], : step - 1]
            want[row, step - 1] = prev[row]
    od, nd, pd = _d(torch.as_tensor(old)), _d(torch.as_tensor(want * 0 - 1)), _d(torch.as_tensor(prev))
    sin, sout = _d(_i32([step])), _d(_i32([-1]))
    rp = None if rows_live is None else _d(_i32([rows_live]))
    sp = None if stop is None else _d(_i32([stop]))
    rc = lib.d2t_op_beam_ancestry(_lib.ptr(od), _lib.ptr(nd), _lib.ptr(pd), rows, stride, _lib.ptr(sin), _lib.ptr(sout), _lib.ptr(rp),
                                  _lib.ptr(sp), _lib.stream_of(od))
    torch.cuda.synchronize()
    assert rc == 0
    assert int(sout.cpu()) == step  # the step is published whatever the guards say
    assert np.array_equal(nd.cpu().numpy(), want)
    assert np.array_equal(od.cpu().numpy(), old)


def test_beam_ancestry_refuses_bad_parents_and_steps():
    lib = _lib.require_device()
    od, nd = _d(_i32(np.zeros((4, 8)))), _d(_i32(np.full((4, 8), -1)))
    for prev, step in (([0, 1, 2, 4], 3), ([0, -1, 2, 3], 3), ([0, 1, 2, 3], 9), ([0, 1, 2, 3], -1)):
        pd, sin, sout = _d(_i32(prev)), _d(_i32([step])), _d(_i32([-1]))
        rc = lib.d2t_op_beam_ancestry(_lib.ptr(od), _lib.ptr(nd), _lib.ptr(pd), 4, 8, _lib.ptr(sin), _lib.ptr(sout), None, None,
                                      _lib.stream_of(od))
        torch.cuda.synchronize()
        assert rc == EINVAL and (nd.cpu() == -1).all() and int(sout.cpu()) == -1


@pytest.mark.parametrize("slabs,cap,M,heads,Lmax,hd,rows", [
    (2, 5, 5, 8, 16, 32, 1), (2, 5, 3, 8, 16, 32, 7), (12, 10, 7, 8, 24, 32, 24), (2, 6, 6, 8, 152, 64, 152), (1, 1, 1, 1, 4, 4, 3),
    (4, 64, 64, 8, 64, 32, 7)])
def test_cache_gather_exact(slabs, cap, M, heads, Lmax, hd, rows):
    lib = _lib.require_device()
    g = _gen(cap + rows)
    src = torch.randn(slabs, cap, heads, Lmax, hd, generator=g)
    src[:, :, :, rows:, :] = NAN  # positions beyond `rows` are not copied, whatever they hold
    prev = torch.randint(0, cap, (M,), generator=g).int()
    want = torch.full_like(src, NAN)
    want[:, :M, :, :rows, :] = src[:, prev.long(), :, :rows, :]
    sd, dd, pd = _d(src), _d(torch.full_like(src, NAN)), _d(prev)
    rc = lib.d2t_op_cache_gather(_lib.ptr(sd), _lib.ptr(dd), _lib.ptr(pd), slabs, cap, M, heads, Lmax, hd, rows, _lib.stream_of(sd))
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.equal(_bits(dd.cpu()), _bits(want))
    assert torch.equal(_bits(sd.cpu()), _bits(src))
    bad = _d(_i32([cap] * M))
    rc = lib.d2t_op_cache_gather(_lib.ptr(sd), _lib.ptr(dd), _lib.ptr(bad), slabs, cap, M, heads, Lmax, hd, rows, _lib.stream_of(sd))
    assert rc == EINVAL
    rc = lib.d2t_op_cache_gather(_lib.ptr(sd), _lib.ptr(dd), _lib.ptr(pd), slabs, cap, M, heads, Lmax, hd, Lmax + 1, _lib.stream_of(sd))
    assert rc == EINVAL
