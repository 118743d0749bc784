// libd2t engine: the d2t_op_* entries of the C-ABI -- single kernels behind argument checks, for the operator tests and tools.
#include <climits>

#include "engine_impl.h"

extern "C" {

int d2t_op_conv2d(const float* x, const float* w, const float* bias, const float* residual, float* y, int32_t B,
                  int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KH, int32_t KW, int32_t SH, int32_t SW,
                  int32_t PH, int32_t PW, int32_t act, d2t_stream stream) {
  if (!x || !w || !y || SH < 1 || SW < 1) return D2T_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (Cin == 1 || Cin == 3) {  // the stem kernels: x is the image as the encoder takes it, NCHW planar [B][Cin][H][W]
    if (KH != 3 || KW != 3 || SH != 1 || SW != 1 || PH != 1 || PW != 1 || residual) return D2T_EINVAL;
    return launch_stem(x, w, bias, y, B, Cin, H, W, Cout, act, s) == hipSuccess ? D2T_OK : D2T_EHIP;
  }
  if (Cin % 32) return D2T_EINVAL;
  float* wp = nullptr;  // the kernel's K order (test entry point: temporary repack, synchronous)
  if (hipMalloc(reinterpret_cast<void**>(&wp), (size_t)Cout * KH * KW * Cin * 4) != hipSuccess) return D2T_ENOMEM;
  ConvP p{};
  p.in = x; p.w = wp; p.bias = bias; p.res = residual; p.out = y;
  conv_shape(p, B, H, W, Cin, Cout, KH, KW, SH, SW, PH, PW);
  p.act = act;
  hipError_t e = launch_repack_ohwi(w, wp, Cout, KH, KW, Cin, s);
  if (e == hipSuccess) e = launch_conv(p, s);
  hipStreamSynchronize(s);
  hipFree(wp);
  return e == hipSuccess ? D2T_OK : D2T_EHIP;
}

int d2t_op_conv2d_bf16x3(const float* x, const float* w, const float* bias, const float* residual, float* y, int32_t B,
                         int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KH, int32_t KW, int32_t SH, int32_t SW,
                         int32_t PH, int32_t PW, int32_t act, d2t_stream stream) {
  if (!x || !w || !y || SH < 1 || SW < 1 || Cin % 32) return D2T_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)Cout * KH * KW * Cin;
  uint16_t *hi = nullptr, *lo = nullptr;
  float* wp = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&hi), n * 2) != hipSuccess) return D2T_ENOMEM;
  if (hipMalloc(reinterpret_cast<void**>(&lo), n * 2) != hipSuccess) { hipFree(hi); return D2T_ENOMEM; }
  if (hipMalloc(reinterpret_cast<void**>(&wp), n * 4) != hipSuccess) { hipFree(hi); hipFree(lo); return D2T_ENOMEM; }
  ConvP p{};
  p.in = x; p.w = wp; p.w_hi = hi; p.w_lo = lo; p.bias = bias; p.res = residual; p.out = y;
  conv_shape(p, B, H, W, Cin, Cout, KH, KW, SH, SW, PH, PW);
  p.act = act;
  hipError_t e = launch_repack_ohwi(w, wp, Cout, KH, KW, Cin, s);
  if (e == hipSuccess) e = launch_split_bf16(wp, hi, lo, n, s);
  if (e == hipSuccess) e = launch_conv_bf16x3(p, s);
  hipStreamSynchronize(s);
  hipFree(hi);
  hipFree(lo);
  hipFree(wp);
  return e == hipSuccess ? D2T_OK : D2T_EHIP;
}

// kernel selection of d2t_op_conv2d_bf16x3_split (process-wide; op-level tests and tools/conv_bench.py only)
static int g_op_conv_kind = 3, g_op_reserved_cus = 0;
int d2t_op_set_conv_kernel(int32_t kind, int32_t reserved_cus) {
  if ((kind != 0 && kind != 3 && kind != 8) || reserved_cus < 0 || reserved_cus > 128) return D2T_EINVAL;  // 0 / 3 as d2t_set_conv_kernel; 8: kind 3 in fp16x2 arithmetic (ConvP::f16)
  g_op_conv_kind = kind;
  g_op_reserved_cus = reserved_cus;
  return D2T_OK;
}

// The split-activation kernel: input, residual and output travel as bf16 hi / lo (conv kind 8: fp16) records.
// pool: with the fused 2x2 / stride 2 max-pool (ConvP::pool2, conv kernel 3 only); y is the POOLED map [B][OH/2][OW/2][Cout]
static int op_conv_split(bool pool, const float* x, const float* w, const float* bias, const float* residual, float* y, int B, int H,
                         int W, int Cin, int Cout, int KH, int KW, int SH, int SW, int PH, int PW, int act, hipStream_t s) {
  if (!x || !w || !y || SH < 1 || SW < 1 || Cin % 32 || Cout % 32 || (pool && Cout > 64 && Cout < 128)) return D2T_EINVAL;
  const int OH = (H + 2 * PH - KH) / SH + 1, OW = (W + 2 * PW - KW) / SW + 1;
  const size_t nw = (size_t)Cout * KH * KW * Cin, rx = (size_t)B * H * W, ry = (size_t)B * OH * OW;
  const size_t nx = rx * Cin, ny = ry * Cout, rp = (size_t)B * (OH / 2) * (OW / 2);
  void* buf = nullptr;
  const size_t bytes = nw * 4 + nw * 4 + nx * 4 + ny * 4 + (residual ? ny * 4 : 0) + 256;
  if (hipMalloc(&buf, bytes) != hipSuccess) return D2T_ENOMEM;
  char* q = (char*)buf;
  float* wp = (float*)q; q += nw * 4;
  uint16_t* whi = (uint16_t*)q; q += nw * 2;
  uint16_t* wlo = (uint16_t*)q; q += nw * 2;
  uint16_t* xs = (uint16_t*)q; q += nx * 4;
  uint16_t* ys = (uint16_t*)q; q += ny * 4;
  uint16_t* rs = nullptr;
  if (residual) { rs = (uint16_t*)q; q += ny * 4; }
  void* zero = q;
  ConvP p{};
  p.w = wp; p.w_hi = whi; p.w_lo = wlo; p.bias = bias;
  p.in_hi = xs; p.out_hi = ys; p.res_hi = rs; p.zero16 = zero;
  const int f16 = g_op_conv_kind == 8;  // fp16 records, fp16 hi / lo weights, two MFMAs per product
  p.f16 = f16;
  p.pipelined = (f16 || pool) ? 3 : g_op_conv_kind; p.reserved_cus = g_op_reserved_cus; p.split_tail = !pool;
  conv_shape(p, B, H, W, Cin, Cout, KH, KW, SH, SW, PH, PW);
  p.act = act;
  if (pool) { p.pool2 = 1; p.M = (int)(4 * rp); }  // rows in pooled order
  hipError_t e = hipMemsetAsync(zero, 0, 256, s);
  if (e == hipSuccess) e = launch_repack_ohwi(w, wp, Cout, KH, KW, Cin, s);
  if (e == hipSuccess) e = f16 ? launch_split_f16(wp, whi, wlo, nw, s) : launch_split_bf16(wp, whi, wlo, nw, s);
  if (e == hipSuccess) e = launch_split_act(x, xs, rx, Cin, s, f16);
  if (e == hipSuccess && residual) e = launch_split_act(residual, rs, ry, Cout, s, f16);
  if (e == hipSuccess) e = launch_conv_bf16x3(p, s);
  if (e == hipSuccess) e = launch_merge_act(ys, y, pool ? rp : ry, Cout, s, f16);
  hipStreamSynchronize(s);
  hipFree(buf);
  return e == hipSuccess ? D2T_OK : D2T_EHIP;
}

int d2t_op_conv2d_bf16x3_split(const float* x, const float* w, const float* bias, const float* residual, float* y,
                               int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KH, int32_t KW,
                               int32_t SH, int32_t SW, int32_t PH, int32_t PW, int32_t act, d2t_stream stream) {
  return op_conv_split(false, x, w, bias, residual, y, B, H, W, Cin, Cout, KH, KW, SH, SW, PH, PW, act, (hipStream_t)stream);
}

int d2t_op_conv2d_bf16x3_split_pool(const float* x, const float* w, const float* bias, float* y,
                               int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KH, int32_t KW,
                               int32_t SH, int32_t SW, int32_t PH, int32_t PW, int32_t act, d2t_stream stream) {
  return op_conv_split(true, x, w, bias, nullptr, y, B, H, W, Cin, Cout, KH, KW, SH, SW, PH, PW, act, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------
// the encoder's record path one kernel at a time (test infrastructure; see include/d2t.h): the engine's own launchers and
// its weight concatenation on caller buffers.  Sizes are checked here; what a launcher itself refuses (hipErrorInvalidValue,
// before it launches anything) comes back as D2T_EINVAL.
// ---------------------------------------------------------------------------
namespace {
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
bool rec_fmt_ok(int f) { return f >= 0 && f <= 2; }  // conv_common.h REC_BF16, REC_F16, REC_F16_PAIR
// the stream drained, the temporary freed, the launches' status as a return code
int rec_op_finish(hipStream_t s, void* buf, hipError_t e) {
  const hipError_t e2 = hipStreamSynchronize(s);
  if (buf) hipFree(buf);
  return e != hipSuccess ? op_status(e) : op_status(e2);
}
}  // namespace

int d2t_op_records_split(const float* x, uint16_t* planes, int64_t rows, int32_t C, int32_t fmt, d2t_stream stream) {
  if (!x || !planes || rows < 1 || C < 32 || C % 32 || !rec_fmt_ok(fmt) || rows * C > (1LL << 31)) return D2T_EINVAL;
  if ((reinterpret_cast<uintptr_t>(x) & 3) || !aligned16(planes)) return D2T_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  return rec_op_finish(s, nullptr, launch_split_act(x, planes, (size_t)rows, C, s, fmt));
}

int d2t_op_records_merge(const uint16_t* planes, float* x, int64_t rows, int32_t C, int32_t fmt, d2t_stream stream) {
  if (!x || !planes || rows < 1 || C < 32 || C % 32 || !rec_fmt_ok(fmt) || rows * C > (1LL << 31)) return D2T_EINVAL;
  if ((reinterpret_cast<uintptr_t>(x) & 3) || (reinterpret_cast<uintptr_t>(planes) & 1)) return D2T_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  return rec_op_finish(s, nullptr, launch_merge_act(planes, x, (size_t)rows, C, s, fmt));
}

int d2t_op_conv_records(const d2t_op_conv_records_args* a, d2t_stream stream) {
  if (!a || !a->w) return D2T_EINVAL;
  const bool rec_in = rec_fmt_ok(a->in_fmt);
  if (rec_in ? (!a->x_rec || a->x_f32) : ((a->in_fmt != 3 && a->in_fmt != 4) || !a->x_f32 || a->x_rec)) return D2T_EINVAL;
  if ((a->out_rec != nullptr) == (a->out_f32 != nullptr) || (a->res_rec && a->res_f32)) return D2T_EINVAL;
  if ((a->out_rec && !rec_fmt_ok(a->out_fmt)) || (a->res_rec && !rec_fmt_ok(a->res_fmt))) return D2T_EINVAL;
  if (a->B < 1 || a->H < 1 || a->W < 1 || a->Cin < 32 || a->Cin % 32 || a->Cout < 32 || a->Cout % 32 || a->KH < 1 || a->KW < 1 ||
      a->KH * a->KW > 16 || a->SH < 1 || a->SW < 1 || a->PH < 0 || a->PW < 0 || a->PH >= a->KH || a->PW >= a->KW)
    return D2T_EINVAL;
  if (a->act < ACT_NONE || a->act > ACT_GELU || (a->kind != 0 && a->kind != 3) || a->out_rows < 1) return D2T_EINVAL;
  if (a->max_blocks < 0 || a->reserved_cus < 0) return D2T_EINVAL;
  if (a->in_fmt == 3 && a->Cout < 64) return D2T_EINVAL;  // (launch_conv sends fp32 rows with fewer channels to the fp32 kernel)
  if (a->H + 2 * a->PH < a->KH || a->W + 2 * a->PW < a->KW) return D2T_EINVAL;
  const int OH = a->OH >= 0 ? a->OH : (a->H + 2 * a->PH - a->KH) / a->SH + 1;
  const int OW = a->OW >= 0 ? a->OW : (a->W + 2 * a->PW - a->KW) / a->SW + 1;
  // an overridden grid: every window still starts inside the image or its padding (the taps beyond read the zero page)
  if (OH < 1 || OW < 1 || (long long)(OH - 1) * a->SH - a->PH >= a->H || (long long)(OW - 1) * a->SW - a->PW >= a->W) return D2T_EINVAL;
  const long long M = a->pool2 ? 4LL * a->B * (OH / 2) * (OW / 2) : (long long)a->B * OH * OW;
  if (M < 1 || M > (1 << 24) || (long long)a->B * a->H * a->W * a->Cin * 2 > INT_MAX) return D2T_EINVAL;
  const bool second = a->x2_rec || a->w2 || a->bias2 || a->Cin2;
  if (second) {  // (Cin2 % 32 and the layer shapes this mode serves: the launcher's own refusals)
    if (!rec_in || !a->x2_rec || !a->w2 || !a->bias || !a->bias2 || a->Cin2 < 1) return D2T_EINVAL;
    if (M * a->Cin2 * 2 > INT_MAX) return D2T_EINVAL;  // DmaIssuer::a_off2 is an int
  }
  // the rows the launch writes, and the table rows it reads
  long long last_row;
  if (a->rows_per_img < 0 || a->row_add_off < 0) return D2T_EINVAL;
  if (a->rows_per_img > 0) {
    if (a->pool2 || a->row_off < 0 || (long long)a->row_off + a->rows_per_img > a->img_stride || M % a->rows_per_img) return D2T_EINVAL;
    last_row = (M / a->rows_per_img - 1) * a->img_stride + a->row_off + a->rows_per_img - 1;
  } else {
    last_row = (a->pool2 ? M / 4 : M) - 1;
  }
  if (last_row >= a->out_rows) return D2T_EINVAL;
  if (a->row_add && (a->pool2 || (long long)a->row_add_off + (a->rows_per_img > 0 ? a->rows_per_img : 1) > a->row_add_rows)) return D2T_EINVAL;
  if (!aligned16(a->x_rec) || !aligned16(a->x_f32) || !aligned16(a->x2_rec) || !aligned16(a->res_rec) || !aligned16(a->res_f32) ||
      !aligned16(a->row_add) || !aligned16(a->out_rec) || !aligned16(a->out_f32) || !aligned16(a->bias) || !aligned16(a->bias2))
    return D2T_EINVAL;

  hipStream_t s = (hipStream_t)stream;
  const int K1 = a->KH * a->KW * a->Cin, K2 = second ? a->Cin2 : 0, Co = a->Cout;
  const size_t n1 = (size_t)Co * K1, n = (size_t)Co * (K1 + K2);
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  void* buf = nullptr;
  if (hipMalloc(&buf, up(n1 * 4) + up(n * 4) + up((size_t)Co * 4) + 2 * up(n * 2) + 256) != hipSuccess) return D2T_ENOMEM;
  char* q = (char*)buf;
  float* wp = (float*)q; q += up(n1 * 4);     // w in the kernels' K order
  float* wcat = (float*)q; q += up(n * 4);    // [w | w2] along K
  float* bcat = (float*)q; q += up((size_t)Co * 4);
  uint16_t* whi = (uint16_t*)q; q += up(n * 2);
  uint16_t* wlo = (uint16_t*)q; q += up(n * 2);
  void* zero = q;
  const int f16 = rec_in && a->in_fmt != 0;  // fp16 records in: the two-MFMA arithmetic, as conv_operands
  ConvP p{};
  hipError_t e = hipMemsetAsync(zero, 0, 256, s);
  if (e == hipSuccess) e = launch_repack_ohwi(a->w, wp, Co, a->KH, a->KW, a->Cin, s);
  if (second) {  // (a 1x1 layer's K order is plain)
    if (e == hipSuccess) e = eng::concat_k(wp, a->bias, K1, a->w2, a->bias2, K2, Co, wcat, bcat, whi, wlo, s);
    p.w = wcat; p.bias = bcat; p.in2_hi = a->x2_rec; p.Cin2 = K2;
  } else {
    if (e == hipSuccess && a->in_fmt != 4) e = launch_split_bf16(wp, whi, wlo, n, s);
    p.w = wp; p.bias = a->bias;
  }
  if (e == hipSuccess && f16) e = launch_split_f16(p.w, whi, wlo, n, s);  // as eng::f16_planes
  if (a->in_fmt != 4) { p.w_hi = whi; p.w_lo = wlo; }
  if (rec_in) { p.in_hi = a->x_rec; p.zero16 = zero; p.f16 = f16; } else p.in = a->x_f32;
  p.pipelined = a->kind; p.split_tail = a->split_tail != 0;
  p.max_blocks = a->max_blocks; p.reserved_cus = a->reserved_cus;
  p.res = a->res_f32;
  if (a->res_rec) { p.res_hi = a->res_rec; p.res_fmt = 1 + a->res_fmt; }
  if (a->out_rec) { p.out_hi = a->out_rec; p.out_fmt = 1 + a->out_fmt; } else p.out = a->out_f32;
  conv_shape(p, a->B, a->H, a->W, a->Cin, Co, a->KH, a->KW, a->SH, a->SW, a->PH, a->PW, OH, OW);
  p.K += K2;
  p.act = a->act;
  if (a->pool2) { p.pool2 = 1; p.M = (int)M; }
  p.row_add = a->row_add; p.rows_per_img = a->rows_per_img; p.img_stride = a->img_stride; p.row_off = a->row_off;
  p.row_add_off = a->row_add_off;
  if (e == hipSuccess) e = launch_conv(p, s);
  return rec_op_finish(s, buf, e);
}

int d2t_op_linear_kv(const float* x, const float* w, const float* bias, float* y, int32_t K, int32_t N, int32_t kv_B, int32_t kv_T,
                     int32_t heads, int32_t hd, int32_t bf16x3, d2t_stream stream) {
  if (!x || !w || !y || K < 32 || K % 32 || N < 1 || kv_B < 1 || kv_T < 1 || heads < 1 || hd < 1) return D2T_EINVAL;
  const long long d = (long long)heads * hd, M = (long long)kv_B * kv_T;
  if (d > N || N % d || M > (1 << 24) || N > (1 << 20) || (bf16x3 && N < 64)) return D2T_EINVAL;
  if (!aligned16(x) || !aligned16(w) || !aligned16(bias) || !aligned16(y)) return D2T_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  ConvP p{};
  p.in = x; p.w = w; p.bias = bias; p.out = y;
  linear_shape(p, (int)M, K, N);
  p.store_mode = STORE_KV; p.kv_T = kv_T; p.kv_heads = heads; p.kv_hd = hd; p.kv_B = kv_B;
  void* buf = nullptr;
  hipError_t e = hipSuccess;
  if (bf16x3) {
    const size_t n = (size_t)N * K;
    if (hipMalloc(&buf, n * 4) != hipSuccess) return D2T_ENOMEM;
    uint16_t* hi = (uint16_t*)buf;
    p.w_hi = hi; p.w_lo = hi + n;
    e = launch_split_bf16(w, hi, hi + n, n, s);
  }
  if (e == hipSuccess) e = launch_conv(p, s);
  return rec_op_finish(s, buf, e);
}

int d2t_op_maxpool_records(const uint16_t* x, uint16_t* y, int32_t B, int32_t H, int32_t W, int32_t C, int32_t SH, int32_t SW,
                           int32_t PH, int32_t PW, int32_t fmt, d2t_stream stream) {
  if (!x || !y || x == y || B < 1 || H < 1 || W < 1 || C < 32 || C % 32 || SH < 1 || SW < 1 || !rec_fmt_ok(fmt)) return D2T_EINVAL;
  // padding below the window size: every window holds at least one pixel of the map
  if (PH < 0 || PH > 1 || PW < 0 || PW > 1 || H + 2 * PH < 2 || W + 2 * PW < 2) return D2T_EINVAL;
  if ((long long)B * H * W * C > (1LL << 31) || !aligned16(x) || !aligned16(y)) return D2T_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  return rec_op_finish(s, nullptr, launch_maxpool_split(x, y, B, H, W, C, SH, SW, PH, PW, s, fmt));
}

int d2t_op_stem_records(const float* img, const float* w, const float* bias, uint16_t* out, int32_t B, int32_t Cin, int32_t H,
                        int32_t W, int32_t act, int32_t fmt, d2t_stream stream) {
  if (!img || !w || !out || B < 1 || H < 1 || W < 1 || (Cin != 1 && Cin != 3) || (act != ACT_NONE && act != ACT_RELU)) return D2T_EINVAL;
  if ((fmt != 0 && fmt != 1) || (long long)B * H * W * 32 > (1LL << 31) || !aligned16(out)) return D2T_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  return rec_op_finish(s, nullptr, launch_stem_split(img, w, bias, out, B, Cin, H, W, 32, act, s, fmt));
}

int d2t_op_pack_conv(const float* w_oihw, const float* conv_bias, const float* bn_w, const float* bn_b, const float* bn_mean,
                     const float* bn_var, float eps, float* w_out, float* bias_out, uint16_t* bf16_hi, uint16_t* bf16_lo,
                     uint16_t* f16_hi, uint16_t* f16_lo, int32_t Cout, int32_t Cin, int32_t KH, int32_t KW, d2t_stream stream) {
  if (!w_oihw || !w_out || !bias_out || !bf16_hi || !bf16_lo || !f16_hi || !f16_lo || w_oihw == w_out) return D2T_EINVAL;
  if (Cout < 1 || Cin < 1 || KH < 1 || KW < 1 || (long long)Cout * Cin * KH * KW > (1LL << 28)) return D2T_EINVAL;
  const int nbn = (bn_w != nullptr) + (bn_b != nullptr) + (bn_mean != nullptr) + (bn_var != nullptr);
  if (nbn != 0 && nbn != 4) return D2T_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)Cout * Cin * KH * KW;
  hipError_t e = launch_pack_conv(w_oihw, conv_bias, bn_w, bn_b, bn_mean, bn_var, eps, w_out, bias_out, Cout, Cin, KH, KW, s);
  if (e == hipSuccess) e = launch_split_bf16(w_out, bf16_hi, bf16_lo, n, s);
  if (e == hipSuccess) e = launch_split_f16(w_out, f16_hi, f16_lo, n, s);
  return rec_op_finish(s, nullptr, e);
}

int d2t_op_linear(const float* x, const float* w, const float* bias, const float* residual, float* y, int32_t M,
                  int32_t K, int32_t N, int32_t act, d2t_stream stream) {
  if (!x || !w || !y || K % 16) return D2T_EINVAL;
  LinW lw{w, bias, N, K};
  return linear_any(nullptr, (hipStream_t)stream, x, lw, residual, y, M, act) == hipSuccess ? D2T_OK : D2T_EHIP;
}

int d2t_op_maxpool2x2(const float* x, float* y, int32_t B, int32_t H, int32_t W, int32_t C, int32_t SH, int32_t SW,
                      int32_t PH, int32_t PW, d2t_stream stream) {
  if (!x || !y) return D2T_EINVAL;
  return launch_maxpool(x, y, B, H, W, C, SH, SW, PH, PW, (hipStream_t)stream) == hipSuccess ? D2T_OK : D2T_EHIP;
}

int d2t_op_layernorm(const float* x, const float* gamma, const float* beta, float* y, int32_t rows, int32_t D,
                     float eps, d2t_stream stream) {
  if (!x || !gamma || !beta || !y) return D2T_EINVAL;
  return launch_layernorm(x, gamma, beta, y, rows, D, eps, (hipStream_t)stream) == hipSuccess ? D2T_OK : D2T_EHIP;
}

// The fused GlobalContext block as the encoder runs it (engine.hip, the end of a ResNet stage): one temporary workspace laid out
// like the engine's gc_ws, logits [B*HW] | ctx [B][C] | y [B][C] without padding in between
int d2t_op_global_context(float* x, const float* wg, const float* bg, const float* w1, const float* b1, const float* ln_g,
                          const float* ln_b, const float* w2, const float* b2, float* ctx_out, int32_t B, int32_t HW, int32_t C,
                          d2t_stream stream) {
  if (!x || !wg || !bg || !w1 || !b1 || !ln_g || !ln_b || !w2 || !b2) return D2T_EINVAL;
  if (B < 1 || B > 65535 || HW < 1 || HW > (1 << 24) || C < 4 || C > 512 || C % 4) return D2T_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const size_t nl = (size_t)B * HW, nc = (size_t)B * C;
  float* buf = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&buf), (nl + 2 * nc) * 4) != hipSuccess) return D2T_ENOMEM;
  float *logits = buf, *ctx = buf + nl, *y = ctx + nc;
  const GCParams w{wg, bg, w1, b1, ln_g, ln_b, w2, b2};
  hipError_t e = launch_global_context(x, w, logits, ctx, y, B, HW, C, s);
  if (e == hipSuccess && ctx_out) e = hipMemcpyAsync(ctx_out, ctx, nc * 4, hipMemcpyDeviceToDevice, s);
  hipStreamSynchronize(s);
  hipFree(buf);
  return op_status(e);
}

int d2t_op_vit_attention(const float* qkv, float* y, int32_t B, int32_t N, int32_t heads, d2t_stream stream) {
  if (!qkv || !y) return D2T_EINVAL;
  return launch_vit_attention(qkv, y, B, N, heads, (hipStream_t)stream) == hipSuccess ? D2T_OK : D2T_EHIP;
}

int d2t_op_vit_attention_probs(const float* qkv, float* y, float* probs, int32_t B, int32_t N, int32_t heads,
                               d2t_stream stream) {
  if (!qkv || !y || !probs || B < 1 || N < 1 || heads < 1) return D2T_EINVAL;
  return launch_vit_attention_probs(qkv, y, probs, B, N, heads, (hipStream_t)stream) == hipSuccess ? D2T_OK : D2T_EHIP;
}

int d2t_op_decode_attention(const float* q, const float* k, const float* v, float* y, int32_t B, int32_t heads,
                            int32_t hd, int32_t L, int32_t Lmax, d2t_stream stream) {
  if (!q || !k || !v || !y || L > Lmax) return D2T_EINVAL;
  DecAttnP p{};
  p.q = q; p.q_stride = heads * hd; p.k = const_cast<float*>(k); p.v = const_cast<float*>(v);
  p.y = y; p.y_stride = heads * hd; p.B = B; p.heads = heads; p.hd = hd; p.Lmax = Lmax; p.L = L;
  p.kv_batch_stride = (long long)heads * Lmax * hd;
  return launch_decode_attention(p, (hipStream_t)stream) == hipSuccess ? D2T_OK : D2T_EHIP;
}

// ---------------------------------------------------------------------------
// decode-step kernels one at a time (test infrastructure; see include/d2t.h).  Every entry checks its sizes -- and the
// device-side integers a kernel would index with, read back first -- against the kernel's limits before it launches.
// ---------------------------------------------------------------------------
namespace {
// the stream's earlier work has finished; n ints of device memory on the host
bool fetch_ints(hipStream_t s, const int* dev, size_t n, std::vector<int>* out) {
  out->resize(n);
  if (hipStreamSynchronize(s) != hipSuccess) return false;
  return n == 0 || hipMemcpy(out->data(), dev, n * sizeof(int), hipMemcpyDeviceToHost) == hipSuccess;
}
}  // namespace

namespace {
int op_skinny(const float* x, const float* w, const float* bias, const float* res, const float* ln_g, const float* ln_b,
              float ln_eps, float* y, float* ln_out, int32_t M, int32_t K, int32_t N, int32_t ldx, int32_t ldy, int32_t act,
              const int32_t* step, int64_t out_step_stride, int form, d2t_stream stream) {
  if (!x || !w || !y || M < 1 || M > 65535 * 16 || N < 1 || K < 16 || K % 16 || ldx < K || ldx % 4 || ldy < N) return D2T_EINVAL;
  if (act != ACT_NONE && act != ACT_RELU && act != ACT_GELU) return D2T_EINVAL;
  if ((ln_g == nullptr) != (ln_b == nullptr) || (ln_out && !ln_g)) return D2T_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (step) {
    std::vector<int> t;
    if (out_step_stride < 0 || !fetch_ints(s, step, 1, &t) || t[0] < 0) return D2T_EINVAL;
  }
  SkinnyP p{};
  p.x = x; p.w = w; p.bias = bias; p.res = res; p.y = y;
  p.M = M; p.K = K; p.N = N; p.ldx = ldx; p.ldy = ldy; p.ldres = N; p.act = act;
  p.step_ptr = step; p.out_step_stride = out_step_stride;
  p.ln_g = ln_g; p.ln_b = ln_b; p.ln_eps = ln_eps; p.ln_out = ln_out;
  const hipError_t e = launch_skinny_form(p, form, s);
  return op_status(e);
}
}  // namespace

int d2t_op_skinny(const float* x, const float* w, const float* bias, const float* res, const float* ln_g, const float* ln_b,
                  float ln_eps, float* y, float* ln_out, int32_t M, int32_t K, int32_t N, int32_t ldx, int32_t ldy, int32_t act,
                  const int32_t* step, int64_t out_step_stride, d2t_stream stream) {
  return op_skinny(x, w, bias, res, ln_g, ln_b, ln_eps, y, ln_out, M, K, N, ldx, ldy, act, step, out_step_stride, SKINNY_FORM_AUTO,
                   stream);
}

int d2t_op_skinny_form(const float* x, const float* w, const float* bias, const float* res, const float* ln_g,
                       const float* ln_b, float ln_eps, float* y, float* ln_out, int32_t M, int32_t K, int32_t N, int32_t ldx,
                       int32_t ldy, int32_t act, const int32_t* step, int64_t out_step_stride, int32_t form,
                       d2t_stream stream) {
  if (form != SKINNY_FORM_SPLITK && form != SKINNY_FORM_WIDE) return D2T_EINVAL;
  return op_skinny(x, w, bias, res, ln_g, ln_b, ln_eps, y, ln_out, M, K, N, ldx, ldy, act, step, out_step_stride, form, stream);
}

namespace {
// Set-up the decoder-row operator entries share: one temporary buffer [W_o^T | W_q^T | W_co^T | W_v^T | extra bytes] with the
// four transposes enqueued, and the DecRowP fields every kind sets alike.  *buf is allocated here (nullptr on D2T_ENOMEM)
// and freed by the caller after its stream has drained.
struct RowOpTmp { float* buf; float* wv_t; float* ext; };
int row_op_setup(const float* qkv, const float* xres, float* sk, float* sv, const float* ca_in_w, const float* ca_in_b,
                 const float* sa_out_w, const float* sa_out_b, const float* ca_out_w, const float* ca_out_b, const float* ln1_g,
                 const float* ln1_b, float eps, float* y2, const int32_t* step, int M, int D, int Lmax, size_t extra,
                 hipStream_t s, RowOpTmp* t, DecRowP* r, hipError_t* e) {
  const size_t dd = (size_t)D * D;
  t->buf = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&t->buf), 4 * dd * 4 + extra) != hipSuccess) return D2T_ENOMEM;
  float *wo_t = t->buf, *wq_t = t->buf + dd, *wco_t = t->buf + 2 * dd;
  t->wv_t = t->buf + 3 * dd; t->ext = t->buf + 4 * dd;
  *e = launch_transpose(sa_out_w, wo_t, D, D, s);
  if (*e == hipSuccess) *e = launch_transpose(ca_in_w, wq_t, D, D, s);
  if (*e == hipSuccess) *e = launch_transpose(ca_out_w, wco_t, D, D, s);
  if (*e == hipSuccess) *e = launch_transpose(ca_in_w + 2 * dd, t->wv_t, D, D, s);
  *r = DecRowP{};
  r->qkv = qkv; r->qkv_stride = 3 * D; r->xres = xres;
  r->sk = sk; r->sv = sv; r->s_batch_stride = (long long)Lmax * D; r->s_Lmax = Lmax;
  r->wo_t = wo_t; r->bo = sa_out_b; r->ln1_g = ln1_g; r->ln1_b = ln1_b; r->eps = eps;
  r->wq_t = wq_t; r->bq = ca_in_b; r->wco_t = wco_t; r->bco = ca_out_b;
  r->y2 = y2; r->step_ptr = step; r->M = M; r->D = D; r->heads = 8;
  return D2T_OK;
}
// The device-side integers a row kernel indexes with, read back: the step (a cache position), the row map (optional: samples)
// and the ancestry rows (optional: cache rows at positions below the step).
static int row_op_check(hipStream_t s, const int32_t* step, int Lmax, const int32_t* row_map, int M, int samples, const int32_t* anc,
                 int anc_stride, int rows) {
  std::vector<int> h;
  if (!fetch_ints(s, step, 1, &h)) return D2T_EHIP;
  const int t = h[0];
  if (t < 0 || t >= Lmax) return D2T_EINVAL;
  if (row_map) {
    if (!fetch_ints(s, row_map, M, &h)) return D2T_EHIP;
    for (int v : h) if (v < 0 || v >= samples) return D2T_EINVAL;
  }
  if (anc) {
    if (!fetch_ints(s, anc, (size_t)M * anc_stride, &h)) return D2T_EHIP;
    for (int b = 0; b < M; ++b)
      for (int j = 0; j < t; ++j)
        if (h[(size_t)b * anc_stride + j] < 0 || h[(size_t)b * anc_stride + j] >= rows) return D2T_EINVAL;
  }
  return D2T_OK;
}
// every (row0, len) slice of a ragged table lies inside the packed memory and within the kernels' longest memory
static bool ragged_slices_ok(const int32_t* row0, const int32_t* len, int n, int mem_rows) {
  for (int i = 0; i < n; ++i)
    if (row0[i] < 0 || len[i] < 1 || len[i] > 4096 || (long long)row0[i] + len[i] > mem_rows) return false;
  return true;
}
// the stream drained, the temporaries freed, the launches' status as a return code
static int row_op_finish(hipStream_t s, float* buf, hipError_t e) {
  const hipError_t e2 = hipStreamSynchronize(s);
  hipFree(buf);
  return e == hipErrorInvalidValue ? D2T_EINVAL : (e == hipSuccess && e2 == hipSuccess) ? D2T_OK : D2T_EHIP;
}
}  // namespace

int d2t_op_decoder_row(int32_t kind, const float* qkv, const float* xres, float* sk, float* sv, const float* mem,
                       const float* ca_in_w, const float* ca_in_b, const float* sa_out_w, const float* sa_out_b,
                       const float* ca_out_w, const float* ca_out_b, const float* ln1_g, const float* ln1_b, float eps, float* y2,
                       const int32_t* step, int32_t M, int32_t D, int32_t T, int32_t Lmax, int32_t rows, int32_t samples,
                       int32_t one_row, const int32_t* row_map, const int32_t* anc, int32_t anc_stride, const int32_t* seg,
                       int32_t nsamples, d2t_stream stream) {
  if (!qkv || !xres || !sk || !sv || !mem || !ca_in_w || !ca_in_b || !sa_out_w || !sa_out_b || !ca_out_w || !ca_out_b ||
      !ln1_g || !ln1_b || !y2 || !step)
    return D2T_EINVAL;
  if (kind < 0 || kind > 5 || M < 1 || M > 65535 || rows < M || samples < 1 || T < 1 || T > 4096 || Lmax < 1 || Lmax > 4096)
    return D2T_EINVAL;
  if (kind == 0 ? (D != 256 && D != 512) : D != 256) return D2T_EINVAL;
  if (!row_map && samples < M) return D2T_EINVAL;  // row b attends over sample b
  if (anc && ((kind != 2 && kind != 4) || Lmax > 512 || anc_stride < Lmax)) return D2T_EINVAL;  // one-row absorbed builds only
  if (kind == 5 && (!seg || !row_map || nsamples < 1 || nsamples > samples)) return D2T_EINVAL;
  if (kind != 5 && seg) return D2T_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = row_op_check(s, step, Lmax, row_map, M, samples, anc, anc_stride, rows)) return rc;
  if (kind == 5) {  // compact segments in sample order, at most 6 live hypotheses each, every row in exactly one
    std::vector<int> h, rm;
    if (!fetch_ints(s, seg, (size_t)nsamples * 3, &h) || !fetch_ints(s, row_map, M, &rm)) return D2T_EHIP;
    int next = 0;
    for (int n = 0; n < nsamples; ++n) {
      const int first = h[3 * n], cnt = h[3 * n + 1];
      if (cnt < 0 || cnt > 6 || (cnt > 0 && first != next)) return D2T_EINVAL;
      for (int r = 0; r < cnt; ++r) if (rm[next + r] != n) return D2T_EINVAL;
      next += cnt;
    }
    if (next != M) return D2T_EINVAL;
  }
  const size_t dd = (size_t)D * D, memn = (size_t)samples * T * D;
  // temporaries: three transposed projections, W_v^T; then projected K / V (kind 0), bf16 planes (3, 4), q' + x1 (5)
  size_t extra = 0;
  if (kind == 0) extra = 2 * memn * 4;
  else if (kind == 3 || kind == 4) extra = memn * 4;
  else if (kind == 5) extra = (size_t)M * 9 * D * 4;
  RowOpTmp tmp;
  DecRowP r;
  hipError_t e = hipSuccess;
  if (int rc = row_op_setup(qkv, xres, sk, sv, ca_in_w, ca_in_b, sa_out_w, sa_out_b, ca_out_w, ca_out_b, ln1_g, ln1_b, eps, y2, step,
                            M, D, Lmax, extra, s, &tmp, &r, &e))
    return rc;
  float *const buf = tmp.buf, *const wv_t = tmp.wv_t, *const ext = tmp.ext;
  r.c_row_map = row_map; r.T = T;
  r.anc = anc; r.anc_stride = anc_stride;
  const float *wk = ca_in_w + dd, *bv = ca_in_b + 2 * D;
  if (e != hipSuccess) {  // (nothing more to launch)
  } else if (kind == 0) {  // K / V of the memory rows as cross_kv projects them: [2][samples][8][T][D / 8]
    ConvP p{};
    p.in = mem; p.w = wk; p.bias = ca_in_b + D; p.out = ext;
    linear_shape(p, samples * T, D, 2 * D);
    p.store_mode = STORE_KV; p.kv_T = T; p.kv_heads = 8; p.kv_hd = D / 8; p.kv_B = samples;
    e = launch_conv(p, s);
    r.ck = ext; r.cv = ext + memn; r.c_batch_stride = (long long)T * D;
    r.one_row = one_row != 0;
    if (e == hipSuccess) e = launch_decoder_row(r, s);
  } else if (kind == 5) {
    r.one_row = 1;
    e = launch_decoder_row_beam(r, mem, (long long)T * D, wk, wv_t, bv, ext, ext + (size_t)M * 8 * D, seg, nsamples, s);
  } else {
    r.one_row = kind == 2 || kind == 4;
    uint16_t *hi = nullptr, *lo = nullptr;
    if (kind >= 3) {
      hi = reinterpret_cast<uint16_t*>(ext); lo = hi + memn;
      e = launch_split_bf16(mem, hi, lo, memn, s);
    }
    if (e == hipSuccess) e = launch_decoder_row_absorbed(r, mem, (long long)T * D, wk, wv_t, bv, s, hi, lo);
  }
  return row_op_finish(s, buf, e);
}

// cross_attn_probs_kernel alone (decode_maps.hip): the probabilities of M query rows, row b over its own T projected keys
int d2t_op_cross_attn_probs(const float* q, const float* keys, int32_t M, int32_t D, int32_t T, int32_t per_head, float* out,
                            d2t_stream stream) {
  if (!q || !keys || !out || M < 1 || M > 65535 || T < 1 || T > 4096 || (D != 256 && D != 512)) return D2T_EINVAL;
  CrossProbsP p{};
  p.q = q; p.q_stride = D; p.ck = keys; p.c_batch_stride = (long long)T * D; p.M = M; p.D = D; p.T = T;
  p.out = out; p.out_head_stride = per_head ? T : 0; p.out_row_stride = (long long)(per_head ? 8 : 1) * T;
  hipStream_t s = (hipStream_t)stream;
  const hipError_t e = launch_cross_attn_probs(p, s);
  return row_op_finish(s, nullptr, e);
}

// The ragged builds of the greedy absorbed row kernels (kind as d2t_op_decoder_row: 1 / 2 = fp32 MFMA two-row / one-row,
// 3 / 4 = split-bf16 two-row / one-row): mem is ONE packed [mem_rows][256] buffer, row b attends over the len[b] rows from
// row0[b] on (host arrays, validated here, uploaded for the launch).
int d2t_op_decoder_row_ragged(int32_t kind, const float* qkv, const float* xres, float* sk, float* sv, const float* mem,
                              const float* ca_in_w, const float* ca_in_b, const float* sa_out_w, const float* sa_out_b,
                              const float* ca_out_w, const float* ca_out_b, const float* ln1_g, const float* ln1_b, float eps,
                              float* y2, const int32_t* step, int32_t M, int32_t Lmax, int32_t rows, int32_t mem_rows,
                              const int32_t* row0_host, const int32_t* len_host, d2t_stream stream) {
  if (!qkv || !xres || !sk || !sv || !mem || !ca_in_w || !ca_in_b || !sa_out_w || !sa_out_b || !ca_out_w || !ca_out_b ||
      !ln1_g || !ln1_b || !y2 || !step || !row0_host || !len_host)
    return D2T_EINVAL;
  if (kind < 1 || kind > 4 || M < 1 || M > 65535 || rows < M || mem_rows < 1 || mem_rows > (1 << 22) || Lmax < 1 || Lmax > 4096)
    return D2T_EINVAL;
  if (!ragged_slices_ok(row0_host, len_host, M, mem_rows)) return D2T_EINVAL;
  constexpr int D = 256;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = row_op_check(s, step, Lmax, nullptr, M, 0, nullptr, 0, rows)) return rc;
  const size_t dd = (size_t)D * D, memn = (size_t)mem_rows * D;
  const size_t extra = kind >= 3 ? memn * 4 : 0;
  RowOpTmp tmp;
  DecRowP r;
  hipError_t e = hipSuccess;
  if (int rc = row_op_setup(qkv, xres, sk, sv, ca_in_w, ca_in_b, sa_out_w, sa_out_b, ca_out_w, ca_out_b, ln1_g, ln1_b, eps, y2, step,
                            M, D, Lmax, extra + (size_t)2 * M * 4, s, &tmp, &r, &e))
    return rc;
  float *const buf = tmp.buf, *const wv_t = tmp.wv_t, *const ext = tmp.ext;
  int* tab = reinterpret_cast<int*>(reinterpret_cast<char*>(ext) + extra);  // [row0 | len] behind the bf16 planes
  if (e == hipSuccess) e = hipMemcpyAsync(tab, row0_host, (size_t)M * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(tab + M, len_host, (size_t)M * 4, hipMemcpyHostToDevice, s);
  r.T = 1;  // (unused by the ragged builds)
  r.one_row = kind == 2 || kind == 4;
  uint16_t *hi = nullptr, *lo = nullptr;
  if (e == hipSuccess && kind >= 3) {
    hi = reinterpret_cast<uint16_t*>(ext); lo = hi + memn;
    e = launch_split_bf16(mem, hi, lo, memn, s);
  }
  if (e == hipSuccess) e = launch_decoder_row_absorbed(r, mem, 0, ca_in_w + dd, wv_t, ca_in_b + 2 * D, s, hi, lo, tab, tab + M);
  return row_op_finish(s, buf, e);
}

// The per-sample ragged builds of the one-row absorbed kernel (ragged beam search; kind 2 = fp32 MFMA, 4 = split-bf16): mem is
// ONE packed [mem_rows][256] buffer, row b attends over the len[row_map[b]] rows from row0[row_map[b]] on.  row0 / len: host
// arrays [samples]; row_map (required) and anc (optional, the hypotheses' ancestry rows): device arrays as d2t_op_decoder_row.
int d2t_op_decoder_row_ragged_beam(int32_t kind, const float* qkv, const float* xres, float* sk, float* sv, const float* mem,
                                   const float* ca_in_w, const float* ca_in_b, const float* sa_out_w, const float* sa_out_b,
                                   const float* ca_out_w, const float* ca_out_b, const float* ln1_g, const float* ln1_b, float eps,
                                   float* y2, const int32_t* step, int32_t M, int32_t Lmax, int32_t rows, int32_t mem_rows,
                                   int32_t samples, const int32_t* row0_host, const int32_t* len_host, const int32_t* row_map,
                                   const int32_t* anc, int32_t anc_stride, d2t_stream stream) {
  if (!qkv || !xres || !sk || !sv || !mem || !ca_in_w || !ca_in_b || !sa_out_w || !sa_out_b || !ca_out_w || !ca_out_b ||
      !ln1_g || !ln1_b || !y2 || !step || !row0_host || !len_host || !row_map)
    return D2T_EINVAL;
  if ((kind != 2 && kind != 4) || M < 1 || M > 65535 || rows < M || samples < 1 || samples > 65535 || mem_rows < 1 ||
      mem_rows > (1 << 22) || Lmax < 1 || Lmax > 4096)
    return D2T_EINVAL;
  if (!ragged_slices_ok(row0_host, len_host, samples, mem_rows)) return D2T_EINVAL;
  if (anc && (Lmax > 512 || anc_stride < Lmax)) return D2T_EINVAL;
  constexpr int D = 256;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = row_op_check(s, step, Lmax, row_map, M, samples, anc, anc_stride, rows)) return rc;
  const size_t dd = (size_t)D * D, memn = (size_t)mem_rows * D;
  const size_t extra = kind == 4 ? memn * 4 : 0;
  RowOpTmp tmp;
  DecRowP r;
  hipError_t e = hipSuccess;
  if (int rc = row_op_setup(qkv, xres, sk, sv, ca_in_w, ca_in_b, sa_out_w, sa_out_b, ca_out_w, ca_out_b, ln1_g, ln1_b, eps, y2, step,
                            M, D, Lmax, extra + (size_t)2 * samples * 4, s, &tmp, &r, &e))
    return rc;
  float *const buf = tmp.buf, *const wv_t = tmp.wv_t, *const ext = tmp.ext;
  int* tab = reinterpret_cast<int*>(reinterpret_cast<char*>(ext) + extra);  // [row0 | len] behind the bf16 planes
  if (e == hipSuccess) e = hipMemcpyAsync(tab, row0_host, (size_t)samples * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(tab + samples, len_host, (size_t)samples * 4, hipMemcpyHostToDevice, s);
  r.T = 1;  // (unused by the ragged builds)
  r.one_row = true;
  r.c_row_map = row_map;
  r.anc = anc; r.anc_stride = anc_stride;
  uint16_t *hi = nullptr, *lo = nullptr;
  if (e == hipSuccess && kind == 4) {
    hi = reinterpret_cast<uint16_t*>(ext); lo = hi + memn;
    e = launch_split_bf16(mem, hi, lo, memn, s);
  }
  if (e == hipSuccess) e = launch_decoder_row_absorbed(r, mem, 0, ca_in_w + dd, wv_t, ca_in_b + 2 * D, s, hi, lo, tab, tab + samples);
  return row_op_finish(s, buf, e);
}

int d2t_op_argmax_embed(const float* logits, int32_t S, int64_t* tokens, int32_t* ended, int32_t* end_count, int32_t* steps_done,
                        int32_t* step, int32_t* done_count, int32_t* batch_end_count, int32_t* batch_steps_done,
                        int32_t* batches_done, int32_t* stop_at, const float* emb, const float* pe, float* x, int32_t B, int32_t V,
                        int32_t d, int32_t end_token, int32_t rows_per_batch, int32_t n_batches, d2t_stream stream) {
  if (!logits || !tokens || !ended || !end_count || !steps_done || !step || !done_count || B < 1 || B > 65535 || V < 1 || S < 1)
    return D2T_EINVAL;
  if (end_token < 0 || end_token >= V) return D2T_EINVAL;
  if (x && (!emb || !pe || d < 1)) return D2T_EINVAL;
  if (n_batches < 0 || n_batches > 64) return D2T_EINVAL;
  if (n_batches > 0 && (rows_per_batch < 1 || (long long)rows_per_batch * n_batches != B || !batch_end_count || !batch_steps_done ||
                        !batches_done))
    return D2T_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  std::vector<int> t;
  if (!fetch_ints(s, step, 1, &t)) return D2T_EHIP;
  if (t[0] < 0 || t[0] >= S) return D2T_EINVAL;  // logits / tokens hold S steps, pe S + 1 rows
  ArgmaxP p{};
  p.logits = logits; p.row_stride = (long long)S * V; p.step_stride = V;
  p.tokens = tokens; p.tok_stride = S;
  p.ended = ended; p.end_count = end_count; p.steps_done = steps_done; p.step_ptr = step; p.done_count = done_count;
  p.B = B; p.V = V; p.end_token = end_token;
  p.emb = emb; p.pe = pe; p.x = x; p.d = d;
  p.rows_per_batch = rows_per_batch; p.n_batches = n_batches;
  p.batch_end_count = batch_end_count; p.batch_steps_done = batch_steps_done; p.batches_done = batches_done; p.stop_at = stop_at;
  return launch_argmax_embed(p, s) == hipSuccess ? D2T_OK : D2T_EHIP;
}

int d2t_op_beam_topk(const float* logits, const float* scores, const int32_t* seg, int32_t N, int32_t rows, int32_t V, int32_t kmax,
                     float* topv, int32_t* topi, d2t_stream stream) {
  if (!logits || !scores || !seg || !topv || !topi || N < 1 || N > 65535 || rows < 1 || V < 1 || kmax < 1 || kmax > 16)
    return D2T_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  std::vector<int> h;
  if (!fetch_ints(s, seg, (size_t)N * 3, &h)) return D2T_EHIP;
  for (int n = 0; n < N; ++n) {
    const int off = h[3 * n], m = h[3 * n + 1], k = h[3 * n + 2];
    if (m <= 0 || k <= 0) continue;  // the kernel leaves such a segment alone
    if (off < 0 || m > 16 || off + m > rows || k > kmax || (long long)k > (long long)m * V || (long long)m * V > 0x7fffffffLL)
      return D2T_EINVAL;
  }
  const hipError_t e = launch_beam_topk_batch(logits, scores, seg, N, V, kmax, topv, topi, s);
  return op_status(e);
}

int d2t_op_beam_advance(int32_t init, int64_t go_token, int32_t* ctrl, int64_t* tok, float* scores, int32_t* map, int32_t* prev,
                        int32_t* seg, int32_t* comp_n, int32_t* fin, int32_t* comp_t, int32_t* comp_par, float* comp_score,
                        int32_t* hist_par, int32_t* hist_tok, const float* topv, const int32_t* topi, int32_t N, int32_t beam,
                        int32_t cap, int32_t V, int32_t S, int32_t end_token, d2t_stream stream) {
  if (!ctrl || !tok || !scores || !map || !prev || !seg || !comp_n || !fin || !comp_t || !comp_par || !comp_score || !hist_par ||
      !hist_tok)
    return D2T_EINVAL;
  if (N < 1 || N > 1024 || beam < 1 || beam > 16 || (long long)cap < (long long)N * beam || V < 1 || S < 1 || end_token < 0 ||
      end_token >= V)
    return D2T_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  BeamDev b{};
  b.ctrl = ctrl; b.tok = tok; b.scores = scores; b.map = map; b.prev = prev; b.seg = seg; b.comp_n = comp_n; b.fin = fin;
  b.comp_t = comp_t; b.comp_par = comp_par; b.comp_score = comp_score; b.hist_par = hist_par; b.hist_tok = hist_tok;
  b.topv = topv; b.topi = topi; b.N = N; b.beam = beam; b.cap = cap; b.V = V; b.S = S; b.end_token = end_token;
  if (init) return launch_beam_dev_init(b, go_token, s) == hipSuccess ? D2T_OK : D2T_EHIP;
  if (!topv || !topi) return D2T_EINVAL;
  // the state as the kernel will read it: the step indexes the history, the candidates index rows of their segment
  std::vector<int> c, sg, cn, fi, ti;
  if (!fetch_ints(s, ctrl, 4, &c) || !fetch_ints(s, seg, (size_t)N * 3, &sg) || !fetch_ints(s, comp_n, N, &cn) ||
      !fetch_ints(s, fin, N, &fi) || !fetch_ints(s, topi, (size_t)N * beam, &ti))
    return D2T_EHIP;
  if (c[0] < 0 || c[2] < 0) return D2T_EINVAL;
  if (!(c[2] && c[0] >= c[2])) {  // the launch will do work
    if (c[0] >= S) return D2T_EINVAL;
    for (int i = 0; i < N; ++i) {
      if (fi[i] || sg[3 * i + 1] <= 0) continue;
      const int live = sg[3 * i + 2], m = sg[3 * i + 1];
      if (live < 0 || live > beam || cn[i] < 0 || cn[i] + live > beam || sg[3 * i] < 0 || sg[3 * i] + m > cap) return D2T_EINVAL;
      for (int r = 0; r < live; ++r) {
        const int idx = ti[(size_t)i * beam + r];
        if (idx < 0 || idx / V >= m) return D2T_EINVAL;
      }
    }
  }
  const hipError_t e = launch_beam_dev_advance(b, s);
  return op_status(e);
}

int d2t_op_beam_ancestry(const int32_t* anc_old, int32_t* anc_new, const int32_t* prev, int32_t rows, int32_t stride,
                         const int32_t* step_in, int32_t* step_out, const int32_t* rows_ptr, const int32_t* stop,
                         d2t_stream stream) {
  if (!anc_old || !anc_new || !prev || !step_in || !step_out || rows < 1 || rows > 65535 || stride < 1) return D2T_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  std::vector<int> t, pv;
  if (!fetch_ints(s, step_in, 1, &t) || !fetch_ints(s, prev, rows, &pv)) return D2T_EHIP;
  if (t[0] < 0 || t[0] > stride) return D2T_EINVAL;  // positions 0 .. t - 1 of a row are written
  for (int v : pv) if (v < 0 || v >= rows) return D2T_EINVAL;
  const hipError_t e = launch_beam_ancestry(anc_old, anc_new, prev, rows, stride, step_in, step_out, s, rows_ptr, stop);
  return op_status(e);
}

int d2t_op_cache_gather(const float* src, float* dst, const int32_t* prev, int32_t slabs, int32_t cap, int32_t M, int32_t heads,
                        int32_t Lmax, int32_t hd, int32_t rows, d2t_stream stream) {
  if (!src || !dst || !prev || src == dst || slabs < 1 || cap < 1 || M < 1 || M > cap || M > 65535 || heads < 1 || heads > 65535 ||
      Lmax < 1 || hd < 4 || hd % 4 || rows < 1 || rows > Lmax)
    return D2T_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  std::vector<int> pv;
  if (!fetch_ints(s, prev, M, &pv)) return D2T_EHIP;
  for (int v : pv) if (v < 0 || v >= cap) return D2T_EINVAL;
  return launch_cache_gather(src, dst, prev, slabs, cap, M, heads, Lmax, hd, rows, s) == hipSuccess ? D2T_OK : D2T_EHIP;
}

// ---------------------------------------------------------------------------
// recurrent kernels one at a time (test infrastructure; see include/d2t.h): the launchers of recurrent.hip on caller
// tensors in the kernels' own layouts, behind the same checks.  Asynchronous unless an integer table has to be read back.
// ---------------------------------------------------------------------------
namespace {
// n 64-bit token ids of device memory, each in [0, V)?  (the stream's earlier work has finished)  0 / D2T_EINVAL / D2T_EHIP
int tokens_in_range(hipStream_t s, const int64_t* dev, size_t n, int V) {
  std::vector<int64_t> h(n);
  if (hipStreamSynchronize(s) != hipSuccess) return D2T_EHIP;
  if (n && hipMemcpy(h.data(), dev, n * sizeof(int64_t), hipMemcpyDeviceToHost) != hipSuccess) return D2T_EHIP;
  for (int64_t v : h) if (v < 0 || v >= V) return D2T_EINVAL;
  return D2T_OK;
}
// the device tables of a greedy decode group (AttnDecP::grp_*) and where its per-batch step counts go
struct OpAttnGroup { const int32_t *row0, *len, *row_batch, *batch_rows; int n_batches; int32_t* steps_dev; };
int op_attn_decode(const d2t_op_attn_decode_args* a, bool ragged, const int32_t* smp_row0, const int32_t* smp_T, int st_ld,
                   d2t_stream stream, const OpAttnGroup* grp = nullptr);
}  // namespace

int d2t_op_bilstm(const float* g, const float* whh_t, float* out, float* sv_gates, float* sv_c, int32_t B, int32_t T,
                  int32_t H, d2t_stream stream) {
  if (!g || !whh_t || !out || (sv_gates == nullptr) != (sv_c == nullptr)) return D2T_EINVAL;
  if (H != 256 || B < 1 || B > 65535 * 4 || T < 1) return D2T_EINVAL;  // grid.y blocks of four rows
  hipStream_t s = (hipStream_t)stream;
  return op_status(sv_gates ? launch_bilstm_train_fwd(g, whh_t, out, sv_gates, sv_c, B, T, H, s) : launch_bilstm(g, whh_t, out, B, T, H, s));
}

int d2t_op_bilstm_hprev(const float* out, float* hprev_fwd, float* hprev_rev, int32_t B, int32_t T, int32_t H,
                        d2t_stream stream) {
  if (!out || !hprev_fwd || !hprev_rev || B < 1 || T < 1 || H < 1) return D2T_EINVAL;
  return op_status(launch_bilstm_hprev(out, hprev_fwd, hprev_rev, B, T, H, (hipStream_t)stream));
}

int d2t_op_attn_decode(const d2t_op_attn_decode_args* a, d2t_stream stream) {
  return op_attn_decode(a, false, nullptr, nullptr, 0, stream);
}

int d2t_op_attn_decode_ragged(const d2t_op_attn_decode_args* a, const int32_t* smp_row0, const int32_t* smp_T, int32_t st_ld,
                              d2t_stream stream) {
  return op_attn_decode(a, true, smp_row0, smp_T, st_ld, stream);
}

int d2t_op_attn_decode_group(const d2t_op_attn_decode_args* a, const int32_t* row0, const int32_t* len, const int32_t* row_batch,
                             const int32_t* batch_rows, int32_t n_batches, int32_t* steps_dev, d2t_stream stream) {
  const OpAttnGroup grp{row0, len, row_batch, batch_rows, n_batches, steps_dev};
  return op_attn_decode(a, false, nullptr, nullptr, 0, stream, &grp);
}

namespace {
// d2t_op_attn_decode, and with `ragged` its ragged step: mem / kp packed, the per-sample device tables smp_row0 / smp_T
// [a->samples] read back and checked against a->T (the largest length), the packed row total (the sum of the lengths) and st_ld
// grp: the group build of the loop -- mem / kp packed, the per-row and per-batch device tables read back and checked: every
// length in range and a->T the largest, every row's slice inside the packed rows (their total: the sum of the rows' lengths),
// the rows in batch order and batch_rows their counts; a->exit_state is then one word per batch, and the per-batch finalize
// kernel follows the loop
int op_attn_decode(const d2t_op_attn_decode_args* a, bool ragged, const int32_t* smp_row0, const int32_t* smp_T, int st_ld,
                   d2t_stream stream, const OpAttnGroup* grp) {
  if (!a || !a->mem || !a->kp || !a->wq_t || !a->bq || !a->wloc || !a->bloc || !a->wscore || !a->wx_t || !a->bx || !a->wg_t ||
      !a->bg || !a->probs || !a->tokens || !a->end_step)
    return D2T_EINVAL;
  if (a->B < 1 || a->B > 65535 || a->S < 1 || a->V < 1 || a->V > D2T_ATTN_MAX_CLASSES || a->taps < 1 || a->taps > 11 ||
      a->key_off < 0 || a->key_off > 1 || a->init_mode < 0 || a->init_mode > 2 || a->T - a->key_off < 1 ||
      a->T - a->key_off > 4096 || a->end_token < 0 || a->end_token >= a->V)
    return D2T_EINVAL;
  if ((a->emb == nullptr) == (a->tokgate == nullptr)) return D2T_EINVAL;
  if (a->init_mode != 0 && (!a->wih_t || !a->bih || !a->wic_t || !a->bic)) return D2T_EINVAL;
  if ((a->sv_hprev == nullptr) != (a->sv_cprev == nullptr)) return D2T_EINVAL;
  if ((a->sv_gates == nullptr) != (a->sv_hafter == nullptr) || (a->sv_gates == nullptr) != (a->sv_cafter == nullptr)) return D2T_EINVAL;
  if ((a->use_teacher || a->sv_tok) && !a->teacher) return D2T_EINVAL;
  if (a->exit_state && ((!grp && !a->steps_dev) || a->step_mode || a->teacher)) return D2T_EINVAL;
  if ((!a->exit_state || grp) && a->steps_dev) return D2T_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (grp) {
    if (!grp->row0 || !grp->len || !grp->row_batch || !grp->batch_rows || !grp->steps_dev || grp->n_batches < 1 ||
        grp->n_batches > 64 || grp->n_batches > a->B || a->B > 1024)
      return D2T_EINVAL;
    if (a->step_mode || a->teacher || a->use_teacher || a->out_dropmask || a->sv_tok || a->sv_hprev || a->sv_gates || a->sv_alpha ||
        a->sv_hq || a->sv_x)
      return D2T_EINVAL;
    std::vector<int> r0, len, rb, br;
    if (!fetch_ints(s, grp->row0, a->B, &r0) || !fetch_ints(s, grp->len, a->B, &len) || !fetch_ints(s, grp->row_batch, a->B, &rb) ||
        !fetch_ints(s, grp->batch_rows, grp->n_batches, &br))
      return D2T_EHIP;
    long long total = 0;
    int longest = 0;
    for (int v : len) {
      if (v - a->key_off < 1 || v - a->key_off > 4096) return D2T_EINVAL;
      total += v;
      longest = std::max(longest, v);
    }
    if (longest != a->T) return D2T_EINVAL;
    std::vector<int> count(grp->n_batches, 0);
    for (int b = 0; b < a->B; ++b) {
      if (r0[b] < 0 || (long long)r0[b] + len[b] > total) return D2T_EINVAL;
      if (rb[b] < 0 || rb[b] >= grp->n_batches || rb[b] != (b ? rb[b - 1] + (rb[b] != rb[b - 1]) : 0)) return D2T_EINVAL;
      ++count[rb[b]];
    }
    for (int k = 0; k < grp->n_batches; ++k)
      if (br[k] != count[k] || count[k] < 1) return D2T_EINVAL;
  }
  if (a->step_mode) {
    if (a->S != 1 || a->teacher || a->samples < 1 || !a->st_h_out || !a->st_c_out || !a->st_mem_out) return D2T_EINVAL;
    if (!a->first && (!a->st_h_in || !a->st_c_in || !a->st_mem_in || !a->tok_in)) return D2T_EINVAL;
    if (a->row_sample) {
      std::vector<int> h;
      if (!fetch_ints(s, a->row_sample, a->B, &h)) return D2T_EHIP;
      for (int v : h) if (v < 0 || v >= a->samples) return D2T_EINVAL;
    }
    if (!a->first)
      if (int rc = tokens_in_range(s, a->tok_in, a->B, a->V)) return rc;
  } else if (a->samples != a->B || a->row_sample || a->tok_in) {
    return D2T_EINVAL;
  }
  if (a->teacher)
    if (int rc = tokens_in_range(s, a->teacher, (size_t)a->B * a->S, a->V)) return rc;
  if (ragged) {
    if (!a->step_mode || !smp_row0 || !smp_T || st_ld < 1 || st_ld > 4096) return D2T_EINVAL;
    std::vector<int> r0, len;
    if (!fetch_ints(s, smp_row0, a->samples, &r0) || !fetch_ints(s, smp_T, a->samples, &len)) return D2T_EHIP;
    long long total = 0;
    int longest = 0;
    for (int v : len) {
      if (v - a->key_off < 1 || v - a->key_off > 4096 || v - a->key_off > st_ld) return D2T_EINVAL;
      total += v;
      longest = std::max(longest, v);
    }
    if (longest != a->T) return D2T_EINVAL;
    for (int i = 0; i < a->samples; ++i)
      if (r0[i] < 0 || (long long)r0[i] + len[i] > total) return D2T_EINVAL;
  }
  AttnDecP p{};
  p.mem = a->mem; p.T = a->T; p.D = 256; p.key_off = a->key_off; p.init_mode = a->init_mode;
  p.kp = a->kp; p.wq_t = a->wq_t; p.bq = a->bq; p.wloc = a->wloc; p.bloc = a->bloc; p.taps = a->taps;
  p.wscore = a->wscore; p.bscore = a->bscore; p.wx_t = a->wx_t; p.bx = a->bx; p.wg_t = a->wg_t; p.bg = a->bg;
  p.wih_t = a->wih_t; p.bih = a->bih; p.wic_t = a->wic_t; p.bic = a->bic; p.emb = a->emb; p.tokgate = a->tokgate;
  p.probs = a->probs; p.tokens = a->tokens; p.end_step = a->end_step;
  p.B = a->B; p.S = a->S; p.V = a->V; p.H = 256; p.E = 256; p.coverage = a->coverage != 0; p.end_token = a->end_token;
  p.step_mode = a->step_mode != 0; p.first = a->first != 0;
  p.st_h_in = a->st_h_in; p.st_c_in = a->st_c_in; p.st_mem_in = a->st_mem_in;
  p.st_h_out = a->st_h_out; p.st_c_out = a->st_c_out; p.st_mem_out = a->st_mem_out;
  p.tok_in = a->tok_in; p.row_sample = a->row_sample;
  p.teacher = a->teacher; p.use_teacher = a->use_teacher; p.out_dropmask = a->out_dropmask; p.out_dropscale = a->out_dropscale;
  p.sv_tok = a->sv_tok; p.sv_hprev = a->sv_hprev; p.sv_cprev = a->sv_cprev; p.sv_hafter = a->sv_hafter; p.sv_cafter = a->sv_cafter;
  p.sv_gates = a->sv_gates; p.sv_alpha = a->sv_alpha; p.sv_hq = a->sv_hq; p.sv_x = a->sv_x;
  p.exit_state = reinterpret_cast<unsigned long long*>(a->exit_state);
  if (ragged) { p.smp_row0 = smp_row0; p.smp_T = smp_T; p.st_ld = st_ld; }
  if (grp) { p.grp_row0 = grp->row0; p.grp_len = grp->len; p.grp_row_batch = grp->row_batch; p.grp_batch_rows = grp->batch_rows; }
  hipError_t e = hipMemsetAsync(a->end_step, 0xFF, (size_t)a->B * 4, s);  // -1 = never emitted the end token
  if (e == hipSuccess && a->exit_state) e = hipMemsetAsync(a->exit_state, 0, grp ? (size_t)grp->n_batches * 8 : 8, s);
  if (e == hipSuccess) e = launch_attn_decode(p, s);
  if (e == hipSuccess && grp)
    return op_status(launch_attn_decode_finalize_group(p.exit_state, grp->steps_dev, grp->row_batch, grp->batch_rows, grp->n_batches,
                                                       a->B, a->S, a->V, a->tokens, a->probs, s));
  if (e == hipSuccess && a->exit_state)
    e = launch_attn_decode_finalize(p.exit_state, a->steps_dev, a->B, a->S, a->V, a->T - a->key_off, a->tokens, a->probs,
                                    a->sv_alpha, s);
  return op_status(e);
}
}  // namespace

int d2t_op_attn_decode_finalize(const uint64_t* exit_state, int32_t* steps_dev, int32_t B, int32_t S, int32_t V, int32_t Tk,
                                int64_t* tokens, float* probs, float* alpha, d2t_stream stream) {
  if (!exit_state || !steps_dev || !tokens || !probs || B < 1 || S < 1 || V < 1 || Tk < 1) return D2T_EINVAL;
  return op_status(launch_attn_decode_finalize(reinterpret_cast<const unsigned long long*>(exit_state), steps_dev, B, S, V, Tk,
                                               tokens, probs, alpha, (hipStream_t)stream));
}

int d2t_op_attn_alpha_gather(const float* hist, const int32_t* path, const int32_t* len, float* out, int32_t N, int32_t S,
                             int32_t cap, int32_t Tk, d2t_stream stream) {
  if (!hist || !path || !len || !out || N < 1 || S < 1 || cap < 1 || Tk < 1) return D2T_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  std::vector<int> l, pt;
  if (!fetch_ints(s, len, N, &l) || !fetch_ints(s, path, (size_t)N * S, &pt)) return D2T_EHIP;
  for (int i = 0; i < N; ++i) {
    if (l[i] < 0 || l[i] > S) return D2T_EINVAL;
    for (int j = 0; j < l[i]; ++j)
      if (pt[(size_t)i * S + j] < 0 || pt[(size_t)i * S + j] >= cap) return D2T_EINVAL;
  }
  return op_status(launch_attn_alpha_gather(hist, path, len, out, N, S, cap, Tk, s));
}

namespace {
// the caller's record as the kernels and the host functions take it; false: a missing array or a size they refuse (max_n:
// the kernels' sample limit; the host functions have none)
static bool attn_beam_rec(const d2t_op_attn_beam_rec* r, AttnBeamDev* b, int max_n = 1024) {  // (static: we are inside extern "C")
  if (!r || !r->ctrl || !r->tok || !r->scores || !r->map || !r->idx_h || !r->idx_m || !r->seg || !r->comp_n || !r->fin ||
      !r->last_completed || !r->comp_t || !r->comp_par || !r->comp_score || !r->hist_par || !r->hist_tok)
    return false;
  if (r->N < 1 || r->N > max_n || r->beam < 1 || r->beam > 16 || (long long)r->cap < (long long)r->N * r->beam || r->V < 1 ||
      r->S < 1 || r->end_token < 0 || r->end_token >= r->V)
    return false;
  *b = AttnBeamDev{};
  b->ctrl = r->ctrl; b->tok = r->tok; b->scores = r->scores; b->map = r->map; b->idx_h = r->idx_h; b->idx_m = r->idx_m;
  b->seg = r->seg; b->comp_n = r->comp_n; b->fin = r->fin; b->last_completed = r->last_completed; b->comp_t = r->comp_t;
  b->comp_par = r->comp_par; b->comp_score = r->comp_score; b->hist_par = r->hist_par; b->hist_tok = r->hist_tok;
  b->topv = r->topv; b->topi = r->topi;
  b->N = r->N; b->beam = r->beam; b->cap = r->cap; b->V = r->V; b->S = r->S; b->end_token = r->end_token;
  return true;
}
// The state as one step of the bookkeeping will read it, h's ctrl, seg, comp_n, fin and topi being HOST arrays: the step
// indexes the history, the candidates index rows of their segment.
static bool attn_beam_advance_ok(const AttnBeamDev& h) {
  const int* c = h.ctrl;
  if (c[0] < 0 || c[2] < 0) return false;
  if (c[2] && c[0] >= c[2]) return true;  // stopped: the step does nothing
  if (c[0] >= h.S) return false;
  for (int i = 0; i < h.N; ++i) {
    if (h.fin[i]) continue;
    const int off = h.seg[3 * i], m = h.seg[3 * i + 1], k = h.seg[3 * i + 2];
    if (k < 1 || k > h.beam || m < 1 || m > h.beam || off < 0 || off + std::max(m, k) > h.cap || h.comp_n[i] < 0 ||
        h.comp_n[i] + k > h.beam)
      return false;
    for (int q = 0; q < k; ++q) {
      const int idx = h.topi[(size_t)i * h.beam + q];
      if (idx < 0 || idx / h.V >= m) return false;
    }
  }
  return true;
}
// The walk the final pick will take, h's ctrl, seg, comp_n, last_completed, comp_t, comp_par and the first ctrl[3] steps of
// hist_par being HOST arrays: every row it reads must lie inside the record.
static bool attn_beam_finish_ok(const AttnBeamDev& h) {
  const int steps = h.ctrl[3];
  if (steps < 0 || steps > h.S) return false;
  for (int i = 0; i < h.N; ++i) {
    int t = -1, row = 0;
    if (!h.last_completed[i]) {
      if (h.seg[3 * i + 1] > 0) { t = steps - 1; row = h.seg[3 * i]; }
    } else {
      if (h.comp_n[i] < 1 || h.comp_n[i] > h.beam) return false;
      for (int j = 0; j < h.comp_n[i]; ++j) {  // any of them may be the best
        const int tj = h.comp_t[(size_t)i * h.beam + j], pj = h.comp_par[(size_t)i * h.beam + j];
        if (tj < 0 || tj >= steps || pj < 0 || pj >= h.cap) return false;
        for (int u = tj - 1, rw = pj; u >= 0; --u) {
          rw = h.hist_par[(size_t)u * h.cap + rw];
          if (rw < 0 || rw >= h.cap) return false;
        }
      }
    }
    for (; t >= 0; --t) {
      if (row < 0 || row >= h.cap) return false;
      row = h.hist_par[(size_t)t * h.cap + row];
    }
    if (row < 0 || row >= h.cap) return false;
  }
  return true;
}
}  // namespace

int d2t_op_attn_beam_advance(const d2t_op_attn_beam_rec* r, int32_t init, int64_t go_token, d2t_stream stream) {
  AttnBeamDev b;
  if (!attn_beam_rec(r, &b)) return D2T_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (init) return op_status(launch_attn_beam_dev_init(b, go_token, s));
  if (!b.topv || !b.topi) return D2T_EINVAL;
  std::vector<int> c, sg, cn, fi, ti;
  if (!fetch_ints(s, b.ctrl, 4, &c) || !fetch_ints(s, b.seg, (size_t)b.N * 3, &sg) || !fetch_ints(s, b.comp_n, b.N, &cn) ||
      !fetch_ints(s, b.fin, b.N, &fi) || !fetch_ints(s, b.topi, (size_t)b.N * b.beam, &ti))
    return D2T_EHIP;
  AttnBeamDev h = b;
  h.ctrl = c.data(); h.seg = sg.data(); h.comp_n = cn.data(); h.fin = fi.data(); h.topi = ti.data();
  if (!attn_beam_advance_ok(h)) return D2T_EINVAL;
  return op_status(launch_attn_beam_dev_advance(b, s));
}

int d2t_op_attn_beam_finish(const d2t_op_attn_beam_rec* r, int64_t* seq, int32_t* len, float* score, int32_t* path, int32_t* plen,
                            d2t_stream stream) {
  AttnBeamDev b;
  if (!attn_beam_rec(r, &b) || !seq || !len || !score || (path != nullptr) != (plen != nullptr)) return D2T_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  std::vector<int> c, sg, cn, lc, ct, cp, hp;
  if (!fetch_ints(s, b.ctrl, 4, &c)) return D2T_EHIP;
  if (c[3] < 0 || c[3] > b.S) return D2T_EINVAL;  // (the steps of the history to fetch)
  if (!fetch_ints(s, b.seg, (size_t)b.N * 3, &sg) || !fetch_ints(s, b.comp_n, b.N, &cn) || !fetch_ints(s, b.last_completed, b.N, &lc) ||
      !fetch_ints(s, b.comp_t, (size_t)b.N * b.beam, &ct) || !fetch_ints(s, b.comp_par, (size_t)b.N * b.beam, &cp) ||
      !fetch_ints(s, b.hist_par, (size_t)c[3] * b.cap, &hp))
    return D2T_EHIP;
  AttnBeamDev h = b;
  h.ctrl = c.data(); h.seg = sg.data(); h.comp_n = cn.data(); h.last_completed = lc.data(); h.comp_t = ct.data();
  h.comp_par = cp.data(); h.hist_par = hp.data();
  if (!attn_beam_finish_ok(h)) return D2T_EINVAL;
  return op_status(launch_attn_beam_dev_finish(b, seq, len, score, path, plen, s));
}

// The same two operators on the host functions of attn_beam_host.h, which the host loop of the search runs: every pointer
// is a host pointer, there is no device and no context, and N has no upper limit.
int d2t_op_attn_beam_host_advance(const d2t_op_attn_beam_rec* r, int32_t init, int64_t go_token) {
  AttnBeamDev b;
  if (!attn_beam_rec(r, &b, INT_MAX)) return D2T_EINVAL;
  if (init) { attn_beam_host_init(b, go_token); return D2T_OK; }
  if (!b.topv || !b.topi || !attn_beam_advance_ok(b)) return D2T_EINVAL;
  attn_beam_host_advance(b, b.topv, b.topi);
  return D2T_OK;
}

int d2t_op_attn_beam_host_finish(const d2t_op_attn_beam_rec* r, int64_t* seq, int32_t* len, float* score, int32_t* path,
                                 int32_t* plen) {
  AttnBeamDev b;
  if (!attn_beam_rec(r, &b, INT_MAX) || !seq || !len || !score || (path != nullptr) != (plen != nullptr)) return D2T_EINVAL;
  if (!attn_beam_finish_ok(b)) return D2T_EINVAL;
  attn_beam_host_finish(b, seq, len, score, path, plen);
  return D2T_OK;
}

}  // extern "C"
