// Training step of the recognizer: Model.forward under module.train() and its backward.
//
//   d2t_train_forward   image, teacher tokens -> logits [B][L][V]; BatchNorm on batch statistics (running statistics
//                       updated in the engine's copies), teacher-forced decoder pass with causal + PAD key-padding
//                       masks (prediction_head/tfm.py:103-118); every intermediate the backward needs stays on a tape
//   d2t_train_backward  dlogits -> gradient of every trainable parameter (what loss.backward() leaves in .grad,
//                       engine/training.py:137); read back with d2t_train_grad
//
// Supported stack: HybridViT (ResNet backbone + ViTEncoderV3) or ResNet+None encoders with the TFM head; dropout 0.
// All arithmetic fp32: GEMMs and convolutions (forward and data gradients) on the fp32-MFMA implicit-GEMM kernel
// (conv_mfma.hip), weight gradients on the fp32-MFMA TN kernel (train_wgrad.hip).
//
// This file: the builder's core (tape memory, gradient buffers, GEMMs, reductions), then every operation of the tape as
// a forward builder with its backward directly behind it, then the reverse walk.  The networks built from the operations
// are in train_models.hip, the C entries in train_abi.hip, the types in train_tape.h.
#include "train_tape.h"

namespace tape {

// ---------------- core ----------------
int Tr::alloc(float** p, size_t floats) {
  *p = st->tape.alloc(floats);
  if (!*p) return fail(c, D2T_ENOMEM, "training tape: hipMalloc failed");
  if (st->poison) TCHK(hipMemsetAsync(*p, 0xFF, floats * 4, s));
  return D2T_OK;
}
int Tr::zeros(float** p, size_t floats) {
  RC(alloc(p, floats));
  TCHK(hipMemsetAsync(*p, 0, floats * 4, s));
  return D2T_OK;
}
int Tr::new_tensor(long long rows, int cols, int* id, int B, int H, int W, float* into) {
  TT x;
  x.rows = rows; x.cols = cols; x.B = B; x.H = H; x.W = W;
  if (into) x.p = into; else RC(alloc(&x.p, (size_t)rows * cols));
  st->t.push_back(x);
  *id = (int)st->t.size() - 1;
  return D2T_OK;
}
int Tr::raw(const std::string& k, const float** p, size_t numel) {
  const RawW* r;
  RC(need(c, k, &r));
  if (numel && r->numel != numel) return fail(c, D2T_EINVAL, "weight '%s' has %zu elements, expected %zu", k.c_str(), r->numel, numel);
  *p = r->p;
  return D2T_OK;
}
int Tr::grad_buf(const std::string& k, float** p) {
  st->touched.push_back(k);
  auto it = st->grads.find(k);
  if (it != st->grads.end()) { *p = it->second; return D2T_OK; }
  const RawW* r;
  RC(need(c, k, &r));
  void* q;
  RC(dev_alloc(c, &q, r->numel * 4));
  TCHK(hipMemsetAsync(q, 0, r->numel * 4, s));
  st->grads[k] = (float*)q;
  hipEvent_t ev;
  TCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  st->ready[k] = ev;
  *p = (float*)q;
  return D2T_OK;
}
int Tr::ensure_part(size_t floats) { return ensure(c, &st->part, &st->part_cap, floats * 4); }

// the parameter names of a layer `key`: nn.MultiheadAttention calls its packed projection in_proj_weight / in_proj_bias,
// every other layer has key.weight / key.bias
static std::string param_key(const std::string& key, const char* what) {
  return key + (key.find("in_proj") != std::string::npos ? "_" : ".") + what;
}

// out[M][N] = act(a[M][K] @ w[N][K]^T + bias) + res      (fp32 MFMA GEMM; K % 32 == 0)
int Tr::gemm_nt(const float* a, const float* w, const float* bias, const float* res, float* out, long long M, int N, int K,
                int act) {
  ConvP p{};
  p.in = a; p.w = w; p.bias = bias; p.res = res; p.out = out;
  linear_shape(p, (int)M, K, N);
  p.act = act;
  TCHK(d2t_internal_conv_timed(c, p, s));
  return D2T_OK;
}
// dx[M][K] = g[M][N] @ W[N][K]  ->  NT GEMM against W^T [K][N], whose reduction dimension N must be a multiple of 32: a
// vocabulary-sized N is padded with zeros
int Tr::gemm_gw(const float* g, long long M, int N, int K, const float* w, float** dx) {
  const int Np = (N + 31) / 32 * 32;
  float *t, *gpad = nullptr;
  RC(alloc(&t, (size_t)K * Np));
  if (Np != N) {
    float* wpad;
    RC(alloc(&gpad, (size_t)M * Np));
    RC(alloc(&wpad, (size_t)Np * K));
    TCHK(hipMemsetAsync(wpad, 0, (size_t)Np * K * 4, s));
    TCHK(launch_copy(w, wpad, (size_t)N * K, s));
    TCHK(launch_transpose(wpad, t, Np, K, s));
    TCHK(launch_pad_cols(g, gpad, (size_t)M, N, Np, s));
  } else {
    TCHK(launch_transpose(w, t, N, K, s));
  }
  RC(alloc(dx, (size_t)M * K));
  return gemm_nt(gpad ? gpad : g, t, nullptr, nullptr, *dx, M, K, Np, ACT_NONE);
}
// split-bf16 mode: hand the convolution its input as hi / lo records (a copy in the step's arena), which moves it from
// the kernel that splits fp32 activations inside its K loop to the LDS-DMA kernels (conv_bf16x3p.hip: ~25 % faster; the
// copy costs one pass over the input).  Same split, same three-MFMA products.
bool Tr::want_planes(long long rows, int C) const {
  static const bool off = D2T_PROBE_ENV_STR("D2T_TRAIN_SPLIT_INPUT") && D2T_PROBE_ENV("D2T_TRAIN_SPLIT_INPUT") == 0;
  return !off && c->conv_bf16x3 && c->zero_page && C % 32 == 0 && rows * C * 2 <= 0x7fffffffLL;
}
// records written by the producer of a tensor (BatchNorm apply kernels), or nullptr
int Tr::new_planes(long long rows, int C, uint16_t** out) {
  *out = nullptr;
  if (!want_planes(rows, C)) return D2T_OK;
  float* pl;
  RC(alloc(&pl, (size_t)rows * C));
  *out = reinterpret_cast<uint16_t*>(pl);
  return D2T_OK;
}
int Tr::split_input(ConvP* p, const float* x, long long rows, int C, const uint16_t* ready) {
  if (!want_planes(rows, C) || p->KH * p->KW > 16) return D2T_OK;
  if (!ready) {
    float* planes;
    RC(alloc(&planes, (size_t)rows * C));
    TCHK(launch_split_act(x, reinterpret_cast<uint16_t*>(planes), (size_t)rows, C, s));
    ready = reinterpret_cast<const uint16_t*>(planes);
  }
  p->in = nullptr;
  p->in_hi = ready;
  p->zero16 = c->zero_page;
  p->pipelined = c->conv_pipelined;
  p->split_tail = 1;
  return D2T_OK;
}
// A convolution weight of wn = O * I * KH * KW elements for the kernel, in a caller buffer of packed_floats(wn, O):
// pack_weight: raw OIHW -> the kernel's packed OHWI order (no BN folding in training mode) ...
static size_t packed_floats(size_t wn, int O) { return 2 * wn + O + 64; }
int Tr::pack_weight(const float* w, int O, int I, int KH, int KW, float* buf) {
  TCHK(launch_pack_conv(w, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, buf, buf + (size_t)O * I * KH * KW, O, I, KH, KW, s));
  return D2T_OK;
}
// ... weight_operand: p reads it; in bf16x3 mode also its bf16 hi / lo planes (behind it in the buffer), which make
// launch_conv take the split-bf16 kernel (fp32 activations split on the fly)
int Tr::weight_operand(float* buf, size_t wn, int O, ConvP* p) {
  p->w = buf;
  if (!c->conv_bf16x3) return D2T_OK;
  uint16_t* hi = reinterpret_cast<uint16_t*>(buf + wn + O + 16);
  TCHK(launch_split_bf16(buf, hi, hi + wn, wn, s));
  p->w_hi = hi; p->w_lo = hi + wn;
  return D2T_OK;
}
// the column reduction p describes (a, y, z, mean, rstd, R, C, mode) into per-chunk partials in st->part; *chunks: how many
int Tr::colreduce_part(ColRedP p, int* chunks) {
  *chunks = colreduce_chunks(p.R, p.C);
  RC(ensure_part((size_t)*chunks * 2 * p.C));
  p.part = st->part;
  TCHK(launch_colreduce(p, s));
  return D2T_OK;
}
// ... and its two sums per column into out0[C], out1[C] (out1 nullable)
int Tr::colreduce2(const ColRedP& p, float* out0, float* out1) {
  int chunks;
  RC(colreduce_part(p, &chunks));
  TCHK(launch_colreduce_final(st->part, chunks, p.C, out0, out1, 0, s));
  return D2T_OK;
}
// dst[c] = column sums of a[R][C]
int Tr::colsum(const float* a, long long R, int C, float* dst) {
  ColRedP p{};
  p.a = a; p.R = R; p.C = C; p.mode = CR_SUM;
  return colreduce2(p, dst, nullptr);
}
// The split of a weight gradient's P rows into S chunks of `chunk` rows (rec: the record kernel's tile, or nullptr for the
// plain kernels).  chunk % 32 == 0, no chunk is empty, S <= 64 on the plain path.
WgradPlan wgrad_plan(long long P, int M, int N, int taps, const WgradRecTile* rec) {
  const int tile = (M <= 64 || N <= 64) ? 64 : 128;
  const long long tiles = rec ? (long long)(M / rec->bm) * (N / rec->bn) * taps
                              : (long long)((M + tile - 1) / tile) * ((N + tile - 1) / tile) * taps;
  // split the rows into S chunks so that tiles * S blocks fill whole rounds of the block slots (two 64 KB-LDS blocks per
  // CU on 256 CUs; the record kernel: one to eight per CU by tile shape): among the S that give >= ~2 rounds pick the
  // one wasting least of its last round
  const long long slots = rec ? rec->slots : 512;
  const long long smax = std::max<long long>(1, (P + 511) / 512);
  long long S = 1;
  double best = -1.0;
  for (long long cand = 1; cand <= std::min<long long>(smax, 64); ++cand) {
    const long long blocks = tiles * cand, rounds = (blocks + slots - 1) / slots;
    double eff = (double)blocks / (double)(rounds * slots);
    if (blocks < 2 * slots && cand < smax) eff *= 0.5;  // prefer enough blocks to hide the tile prologue / epilogue
    if (eff > best + 1e-9) { best = eff; S = cand; }
  }
  // the record kernel's K loops are cheap to keep long and every extra split is another [taps][M][N] partial to write
  // and sum: one round of blocks (measured against 2 ... 4 rounds and the rule above: 113.8 vs 114.2 ... 117.8 ms per step)
  static const int rec_rounds = D2T_PROBE_ENV_STR("D2T_WGRAD_ROUNDS") ? std::max(1, D2T_PROBE_ENV("D2T_WGRAD_ROUNDS")) : 1;
  if (rec) S = std::max<long long>(1, std::min<long long>(smax, rec_rounds * slots / tiles));
  long long chunk = ((P + S - 1) / S + 31) / 32 * 32;
  S = (P + chunk - 1) / chunk;
  return WgradPlan{S, chunk};
}
// dW[M][N](taps) = a^T (x) b  with the split-K two-pass reduction
int Tr::wgrad(const float* a, int lda, const float* b, int ldb, long long P, int M, int N, int taps, const Node::Conv* geom,
              const TT* xin, const TT* yout, float* dst, int layout, const uint16_t* a_rec, const uint16_t* b_rec) {
  // both operands exist as split-bf16 records (a convolution between BatchNorm layers): the LDS-DMA kernel
  static const bool rec_off = D2T_PROBE_ENV_STR("D2T_WGRAD_REC") && D2T_PROBE_ENV("D2T_WGRAD_REC") == 0;
  const WgradRecTile* rec =
      !rec_off && a_rec && b_rec && geom && c->conv_bf16x3 && c->zero_page && lda == M && ldb == N ? wgrad_rec_tile(M, N) : nullptr;
  const WgradPlan plan = wgrad_plan(P, M, N, taps, rec);
  const long long S = plan.S, chunk = plan.chunk;
  RC(ensure_part((size_t)S * taps * M * N));
  WgradP p{};
  p.a = a; p.b = b; p.part = st->part; p.P = P; p.M = M; p.N = N; p.lda = lda; p.ldb = ldb; p.taps = taps;
  p.KW = 1; p.S = (int)S; p.chunk = (int)chunk;
  p.bf16x3 = c->conv_bf16x3 ? 1 : 0;
  if (rec) { p.a_rec = a_rec; p.b_rec = b_rec; p.zero = c->zero_page; }
  if (geom) {
    p.geom = 1; p.H = xin->H; p.W = xin->W; p.OH = yout->H; p.OW = yout->W;
    p.KW = geom->KW; p.SH = geom->SH; p.SW = geom->SW; p.PH = geom->PH; p.PW = geom->PW;
  }
  TCHK(launch_wgrad(p, s));
  TCHK(launch_wgrad_reduce(st->part, dst, (int)S, taps, M, N, layout, 0, s));
  return D2T_OK;
}
// The gradients of a Linear's parameters from its output gradient g (P rows, row stride ldg) and its input x (row stride
// ldx): d wk[woff : woff + N] = g^T x (sums over the rows of outer products -> one TN GEMM), d bk[woff : woff + N] = the
// column sums of g (bk empty: no bias; needs ldg == N).  bias_first: the reduction ahead of the GEMM (bwd_linear's order).
int Tr::linear_grads(const std::string& wk, const std::string& bk, const float* g, int ldg, const float* x, int ldx, long long P,
                     int N, int K, int woff, bool bias_first) {
  float *dW, *db = nullptr;
  RC(grad_buf(wk, &dW));
  if (!bk.empty()) RC(grad_buf(bk, &db));
  if (db && bias_first) RC(colsum(g, P, N, db + woff));
  RC(wgrad(g, ldg, x, ldx, P, N, K, 1, nullptr, nullptr, nullptr, dW + (size_t)woff * K, 0));
  if (db && !bias_first) RC(colsum(g, P, N, db + woff));
  return D2T_OK;
}
// out[i] = a[i] + b[i] over n elements for each of B batch elements (strides lda for a and out, ldb for b: 0 = one table
// for all), one launch each
hipError_t Tr::add_rows_each(const float* a, size_t lda, const float* b, size_t ldb, float* out, int B, int n) {
  for (int i = 0; i < B; ++i)
    if (hipError_t e = launch_add_rows(a + i * lda, b + i * ldb, out + i * lda, n, s)) return e;
  return hipSuccess;
}
// tensor gradient accumulation: first contribution takes the buffer, later ones add
int Tr::add_grad(int id, float* g) {
  TT& x = st->t[id];
  if (!x.grad) { x.grad = g; return D2T_OK; }
  TCHK(launch_ew(x.grad, g, x.grad, (size_t)x.rows * x.cols, EW_ADD, s));
  return D2T_OK;
}
// gradient of tensor `id` from one launch: a fresh dx of the tensor's n elements, launch(dx, n) fills it, then add_grad
template <class F>
int Tr::grad_to(int id, F launch) {
  const size_t n = (size_t)st->t[id].rows * st->t[id].cols;
  float* dx;
  RC(alloc(&dx, n));
  TCHK(launch(dx, n));
  return add_grad(id, dx);
}
int Tr::own_grad(int id) {  // make sure tensor `id` has a gradient buffer (contents unspecified)
  TT& x = st->t[id];
  if (!x.grad) RC(alloc(&x.grad, (size_t)x.rows * x.cols));
  return D2T_OK;
}
// a fresh keep mask of n elements (nullptr when dropout is off)
int Tr::new_mask(size_t n, const uint8_t** m, float p) {
  *m = nullptr;
  if (p < 0.f) p = st->drop_p;
  if (p <= 0.f) return D2T_OK;
  float* raw;
  RC(alloc(&raw, n / 4 + 2));
  uint8_t* mk = reinterpret_cast<uint8_t*>(raw);
  TCHK(launch_dropout_mask(mk, n, p, st->drop_seed, (st->drop_calls << 16) | st->drop_site, s));
  ++st->drop_site;
  st->masks.push_back({mk, n});
  *m = mk;
  return D2T_OK;
}
static Node node(Kind kind, int in, int in2 = -1) {
  Node n;
  n.kind = kind; n.in = in; n.in2 = in2;
  return n;
}
int Tr::push(Node& n, int out) {  // the node, with output tensor `out`, onto the tape
  n.out = out;
  st->nodes.push_back(n);
  return D2T_OK;
}
// a node whose output has the shape of its input n.in (the same map: B / H / W carry over): the output tensor,
// launch(x, y, elements), the node on the tape
template <class F>
int Tr::map_node(Node n, int* out, F launch) {
  const TT x = st->t[n.in];
  RC(new_tensor(x.rows, x.cols, out, x.B, x.H, x.W));
  TCHK(launch(x.p, st->t[*out].p, (size_t)x.rows * x.cols));
  return push(n, *out);
}

// ---------------- operations: forward builder, then its backward ----------------
// conv (+BN batch stats) (+res) (+relu).  bnkey empty: bias from wkey + ".bias", no normalisation.
int Tr::conv_bn(int in, const std::string& wkey, const std::string& bnkey, int Cout, int KH, int KW, int SH, int SW, int PH,
                int PW, bool relu, int res, int* out, int OH, int OW) {
  const TT x = st->t[in];
  if (OH < 0) { OH = (x.H + 2 * PH - KH) / SH + 1; OW = (x.W + 2 * PW - KW) / SW + 1; }
  const long long P = (long long)x.B * OH * OW;
  Node n = node(N_CONV, in, res);
  Node::Conv& cv = n.conv;
  cv.wkey = wkey; cv.bnkey = bnkey; cv.Cin = x.cols; cv.Cout = Cout;
  cv.KH = KH; cv.KW = KW; cv.SH = SH; cv.SW = SW; cv.PH = PH; cv.PW = PW; cv.relu = relu;
  const float* w;
  const size_t wn = (size_t)Cout * x.cols * KH * KW;
  RC(raw(wkey + ".weight", &w, wn));
  RC(ensure(c, &st->scratch, &st->scratch_cap, packed_floats(wn, Cout) * 4));
  const float* bias = nullptr;
  if (bnkey.empty()) RC(raw(wkey + ".bias", &bias, Cout));
  RC(pack_weight(w, Cout, x.cols, KH, KW, st->scratch));
  RC(alloc(&cv.z, (size_t)P * Cout));
  ConvP p{};
  RC(weight_operand(st->scratch, wn, Cout, &p));
  p.in = x.p; p.bias = bias; p.out = cv.z;
  conv_shape(p, x.B, x.H, x.W, x.cols, Cout, KH, KW, SH, SW, PH, PW, OH, OW);
  RC(split_input(&p, x.p, x.rows, x.cols, x.planes));
  if (p.in_hi && !x.planes) st->t[in].planes = p.in_hi;  // records made here: the weight gradient reads them again
  TCHK(d2t_internal_conv_timed(c, p, s));
  if (bnkey.empty()) {
    RC(new_tensor(P, Cout, out, x.B, OH, OW, cv.z));
  } else {
    RC(bn_forward(cv, P));
    RC(new_tensor(P, Cout, out, x.B, OH, OW));
    const float *g, *b;
    RC(raw(bnkey + ".weight", &g, Cout));
    RC(raw(bnkey + ".bias", &b, Cout));
    uint16_t* pl;  // the next convolution's operand records, written by the same pass
    RC(new_planes(P, Cout, &pl));
    TCHK(launch_bn_apply(cv.z, cv.mean, cv.rstd, g, b, res >= 0 ? st->t[res].p : nullptr, st->t[*out].p, P, Cout, relu, s, pl));
    st->t[*out].planes = pl;
  }
  return push(n, *out);
}
int Tr::bn_forward(Node::Conv& n, long long P) {
  const int C = n.Cout;
  RC(alloc(&n.mean, C));
  RC(alloc(&n.rstd, C));
  ColRedP p{};
  p.a = n.z; p.R = P; p.C = C; p.mode = CR_SUM_SQ;
  int chunks;
  RC(colreduce_part(p, &chunks));
  const RawW *rm, *rv;
  RC(need(c, n.bnkey + ".running_mean", &rm));
  RC(need(c, n.bnkey + ".running_var", &rv));
  TCHK(launch_bn_finalize(st->part, chunks, C, P, 1e-5f, 0.1f, n.z, n.mean, n.rstd, rm->p, rv->p, s));
  return D2T_OK;
}
// The first layer, a 3x3 convolution of the image's one or three channels on kernels of its own (weight gradient
// included): with BatchNorm + ReLU (ResNet, resnet.py:205-207), or -- bnkey empty -- with a bias and the ReLU as a node of
// its own (VGG, vgg.py:17).
int Tr::stem(const float* img, int B, int Cin, int H, int W, int Cout, const std::string& wkey, const std::string& bnkey, int* out) {
  const long long P = (long long)B * H * W;
  const bool bn = !bnkey.empty();
  Node n = node(N_CONV, -1);
  Node::Conv& cv = n.conv;
  cv.stem = true; cv.wkey = wkey; cv.bnkey = bnkey; cv.relu = bn; cv.Cin = Cin; cv.Cout = Cout;
  cv.KH = cv.KW = 3; cv.PH = cv.PW = 1;
  const float *w, *b;
  RC(raw(wkey + ".weight", &w, (size_t)Cout * 9 * Cin));
  if (bn) {
    RC(alloc(&cv.z, (size_t)P * Cout));
  } else {
    RC(raw(wkey + ".bias", &b, Cout));
    RC(new_tensor(P, Cout, out, B, H, W));
    cv.z = st->t[*out].p;
  }
  TCHK(launch_stem_raw(img, w, cv.z, B, Cin, H, W, Cout, s));
  if (bn) {
    RC(bn_forward(cv, P));
    RC(new_tensor(P, Cout, out, B, H, W));
    const float* g;
    RC(raw(bnkey + ".weight", &g, Cout));
    RC(raw(bnkey + ".bias", &b, Cout));
    TCHK(launch_bn_apply(cv.z, cv.mean, cv.rstd, g, b, nullptr, st->t[*out].p, P, Cout, 1, s));
  } else {
    TCHK(launch_bias_add(cv.z, b, P, Cout, s));
  }
  RC(push(n, *out));
  return bn ? D2T_OK : relu(*out, out);
}
int Tr::bwd_conv(const Node& n) {
  const Node::Conv& cv = n.conv;
  const TT& y = st->t[n.out];
  const long long P = y.rows;
  const int Cout = cv.Cout;
  const float* dz = y.grad;
  uint16_t* dz_planes = nullptr;
  float *dW;
  RC(grad_buf(cv.wkey + ".weight", &dW));
  if (!cv.bnkey.empty()) {
    const float* gamma;
    RC(raw(cv.bnkey + ".weight", &gamma));
    float *dgam, *dbet, *dzb, *gres = nullptr;
    RC(grad_buf(cv.bnkey + ".weight", &dgam));
    RC(grad_buf(cv.bnkey + ".bias", &dbet));
    ColRedP p{};
    p.a = y.grad; p.y = cv.relu ? y.p : nullptr; p.z = cv.z; p.mean = cv.mean; p.rstd = cv.rstd;
    p.R = P; p.C = Cout; p.mode = CR_BN_BWD;
    RC(colreduce2(p, dbet, dgam));
    RC(alloc(&dzb, (size_t)P * Cout));
    if (n.in2 >= 0) RC(alloc(&gres, (size_t)P * Cout));
    if (!cv.stem) RC(new_planes(P, Cout, &dz_planes));  // the data-gradient convolution's operand records
    TCHK(launch_bn_bwd_apply(y.grad, cv.relu ? y.p : nullptr, cv.z, cv.mean, cv.rstd, gamma, dbet, dgam, dzb, gres, P, Cout, s, dz_planes));
    if (n.in2 >= 0) RC(add_grad(n.in2, gres));
    dz = dzb;
  } else {
    float* db;
    RC(grad_buf(cv.wkey + ".bias", &db));
    RC(colsum(dz, P, Cout, db));
  }
  if (cv.stem) {
    const int chunk = 1024, nch = (int)((P + chunk - 1) / chunk), K = 9 * cv.Cin;
    RC(ensure_part((size_t)nch * K * Cout));
    TCHK(launch_stem_wgrad(st->image, dz, st->part, st->B, cv.Cin, st->H, st->W, Cout, chunk, nch, s));
    TCHK(launch_wgrad_reduce(st->part, dW, nch, K, Cout, 1, 1, 0, s));
    return D2T_OK;
  }
  const TT& x = st->t[n.in];
  RC(wgrad(dz, Cout, x.p, x.cols, P, Cout, x.cols, cv.KH * cv.KW, &cv, &x, &y, dW, 1, dz_planes, x.planes));
  // data gradient: stride-1 convolution of the (zero-dilated) dz with the flipped, transposed filter
  const float* w;
  RC(raw(cv.wkey + ".weight", &w));
  const int Cin = x.cols;
  const size_t wn = (size_t)Cin * cv.KH * cv.KW * Cout;
  float *wf, *wp, *dx;
  RC(alloc(&wf, wn));
  RC(alloc(&wp, packed_floats(wn, Cin)));
  TCHK(launch_flip_oihw(w, wf, Cout, Cin, cv.KH, cv.KW, s));                      // [Cin][Cout][KH][KW]
  RC(pack_weight(wf, Cin, Cout, cv.KH, cv.KW, wp));
  const float* src = dz;
  int DH = y.H, DW = y.W;
  if (cv.SH != 1 || cv.SW != 1 || DH != x.H + 2 * cv.PH - cv.KH + 1 || DW != x.W + 2 * cv.PW - cv.KW + 1) {
    DH = std::max(x.H + 2 * cv.PH - cv.KH + 1, (y.H - 1) * cv.SH + 1);
    DW = std::max(x.W + 2 * cv.PW - cv.KW + 1, (y.W - 1) * cv.SW + 1);
    float* dil;
    RC(alloc(&dil, (size_t)x.B * DH * DW * Cout));
    TCHK(launch_dilate(dz, dil, x.B, y.H, y.W, Cout, DH, DW, cv.SH, cv.SW, 0, 0, s));
    src = dil;
  }
  RC(alloc(&dx, (size_t)x.rows * Cin));
  ConvP p{};
  RC(weight_operand(wp, wn, Cin, &p));
  p.in = src; p.out = dx;
  conv_shape(p, x.B, DH, DW, Cout, Cin, cv.KH, cv.KW, 1, 1, cv.KH - 1 - cv.PH, cv.KW - 1 - cv.PW, x.H, x.W);
  RC(split_input(&p, src, (long long)x.B * DH * DW, Cout, src == dz ? dz_planes : nullptr));
  TCHK(d2t_internal_conv_timed(c, p, s));
  return add_grad(n.in, dx);
}

int Tr::pool(int in, int SH, int SW, int PH, int PW, int* out, int KW) {  // window 2 x KW
  const TT x = st->t[in];
  const int OH = (x.H + 2 * PH - 2) / SH + 1, OW = (x.W + 2 * PW - KW) / SW + 1;
  RC(new_tensor((long long)x.B * OH * OW, x.cols, out, x.B, OH, OW));
  if (KW == 2) TCHK(launch_maxpool(x.p, st->t[*out].p, x.B, x.H, x.W, x.cols, SH, SW, PH, PW, s));
  else TCHK(launch_maxpool_k(x.p, st->t[*out].p, x.B, x.H, x.W, x.cols, 2, KW, SH, SW, PH, PW, s));
  Node n = node(N_POOL, in);
  n.pool.SH = SH; n.pool.SW = SW; n.pool.PH = PH; n.pool.PW = PW; n.pool.KW = KW;
  return push(n, *out);
}
int Tr::bwd_pool(const Node& n) {
  const TT& x = st->t[n.in];
  const Node::Pool& q = n.pool;
  return grad_to(n.in, [&](float* dx, size_t) {
    return launch_maxpool_bwd(x.p, st->t[n.out].grad, dx, x.B, x.H, x.W, x.cols, q.SH, q.SW, q.PH, q.PW, s, q.KW);
  });
}

// AdaptiveAvgPool2d((None, 1)) over the height of the permuted map (recognizers/build_feat.py:50-55): [B,H,W,C] -> [B,W,C]
int Tr::mean_h(int in, int* out) {
  const TT x = st->t[in];
  RC(new_tensor((long long)x.B * x.W, x.cols, out, x.B, 1, x.W));
  TCHK(launch_mean_h(x.p, st->t[*out].p, x.B, x.H, x.W, x.cols, s));
  Node n = node(N_MEANH, in);
  return push(n, *out);
}
int Tr::bwd_mean_h(const Node& n) {
  const TT& x = st->t[n.in];
  return grad_to(n.in, [&](float* dx, size_t) { return launch_mean_h_bwd(st->t[n.out].grad, dx, x.B, x.H, x.W, x.cols, s); });
}

// out = act(in @ W[woff:woff+N]^T + b[woff:woff+N]) + res;  `into`: write the result into caller memory
int Tr::linear(int in, const std::string& key, int N, int K, int woff, int act, int res, int* out, float* into, bool bias) {
  const TT x = st->t[in];
  if (x.cols != K) return fail(c, D2T_EINVAL, "linear '%s': input has %d columns, expected %d", key.c_str(), x.cols, K);
  const float *w, *b = nullptr;
  RC(raw(param_key(key, "weight"), &w));
  if (bias) RC(raw(param_key(key, "bias"), &b));
  RC(new_tensor(x.rows, N, out, 0, 0, 0, into));
  RC(gemm_nt(x.p, w + (size_t)woff * K, b ? b + woff : nullptr, res >= 0 ? st->t[res].p : nullptr, st->t[*out].p, x.rows, N, K, act));
  Node n = node(N_LINEAR, in, res);
  n.lin.key = key; n.lin.N = N; n.lin.K = K; n.lin.woff = woff; n.lin.relu = act == ACT_RELU; n.lin.nobias = !bias;
  return push(n, *out);
}
int Tr::bwd_linear(const Node& n) {
  const Node::Linear& l = n.lin;
  const TT& y = st->t[n.out];
  const TT& x = st->t[n.in];
  const float* g = y.grad;
  if (n.in2 >= 0) RC(add_grad(n.in2, y.grad));  // the residual branch takes the incoming gradient as is
  if (l.relu) {
    float* m;
    RC(alloc(&m, (size_t)y.rows * y.cols));
    TCHK(launch_ew(y.grad, y.p, m, (size_t)y.rows * y.cols, EW_RELU_BWD, s));
    g = m;
  }
  const std::string wk = param_key(l.key, "weight");
  RC(linear_grads(wk, l.nobias ? std::string() : param_key(l.key, "bias"), g, l.N, x.p, l.K, y.rows, l.N, l.K, l.woff, true));
  const float* w;
  RC(raw(wk, &w));
  float* dx;
  RC(gemm_gw(g, y.rows, l.N, l.K, w + (size_t)l.woff * l.K, &dx));
  return add_grad(n.in, dx);
}

int Tr::layernorm(int in, const std::string& key, float eps, int* out, float* into) {
  const TT x = st->t[in];
  const float *g, *b;
  RC(raw(key + ".weight", &g, x.cols));
  RC(raw(key + ".bias", &b, x.cols));
  Node n = node(N_LN, in);
  n.ln.key = key;
  RC(alloc(&n.ln.mean, x.rows));
  RC(alloc(&n.ln.rstd, x.rows));
  RC(new_tensor(x.rows, x.cols, out, 0, 0, 0, into));
  TCHK(launch_ln_train(x.p, g, b, st->t[*out].p, n.ln.mean, n.ln.rstd, (int)x.rows, x.cols, eps, s));
  return push(n, *out);
}
int Tr::bwd_ln(const Node& n) {
  const Node::LayerNorm& l = n.ln;
  const TT& y = st->t[n.out];
  const TT& x = st->t[n.in];
  const float* g;
  RC(raw(l.key + ".weight", &g));
  float *dg, *db;
  RC(grad_buf(l.key + ".weight", &dg));
  RC(grad_buf(l.key + ".bias", &db));
  ColRedP p{};
  p.a = y.grad; p.z = x.p; p.mean = l.mean; p.rstd = l.rstd; p.R = x.rows; p.C = x.cols; p.mode = CR_LN_BWD;
  RC(colreduce2(p, db, dg));
  return grad_to(n.in, [&](float* dx, size_t) { return launch_ln_bwd(y.grad, x.p, l.mean, l.rstd, g, nullptr, dx, (int)x.rows, x.cols, s); });
}

int Tr::attention(int qt, int qoff, int kvt, int koff, int voff, int nb, int Lq, int Lk, int heads, int hd, int causal,
                  const int64_t* keytok, int* out, bool attn_dropout, const uint8_t* given_mask, float given_scale) {
  Node n = node(N_ATTN, qt, kvt);
  Node::Attn& a = n.attn;
  a.qoff = qoff; a.koff = koff; a.voff = voff; a.nb = nb; a.Lq = Lq; a.Lk = Lk; a.heads = heads; a.hd = hd;
  RC(alloc(&a.probs, (size_t)nb * heads * Lq * Lk));
  if (attn_dropout) {  // nn.MultiheadAttention(dropout=p): on the softmax probabilities
    RC(new_mask((size_t)nb * heads * Lq * Lk, &a.drop.mask));
    a.drop.scale = 1.f / (1.f - st->drop_p);
  }
  if (given_mask) {  // a caller's keep mask instead of a drawn one (d2t_op_train_attention_ex)
    a.drop.mask = given_mask;
    a.drop.scale = given_scale;
  }
  RC(new_tensor((long long)nb * Lq, heads * hd, out));
  AttnTrainP p{};
  p.dropmask = a.drop.mask; p.dropscale = a.drop.scale;
  p.q = st->t[qt].p + qoff; p.k = st->t[kvt].p + koff; p.v = st->t[kvt].p + voff; p.o = st->t[*out].p; p.probs = a.probs;
  p.keytok = keytok; p.B = nb; p.heads = heads; p.hd = hd; p.Lq = Lq; p.Lk = Lk;
  p.ldq = st->t[qt].cols; p.ldk = p.ldv = st->t[kvt].cols; p.ldo = heads * hd; p.causal = causal; p.pad_id = 0;
  TCHK(launch_attn_train_fwd(p, s));
  return push(n, *out);
}
int Tr::bwd_attn(const Node& n) {
  const Node::Attn& a = n.attn;
  RC(own_grad(n.in));
  RC(own_grad(n.in2));
  const TT& y = st->t[n.out];
  AttnTrainP p{};
  p.q = st->t[n.in].p + a.qoff; p.k = st->t[n.in2].p + a.koff; p.v = st->t[n.in2].p + a.voff;
  p.o = y.grad; p.probs = a.probs;
  p.dq = st->t[n.in].grad + a.qoff; p.dk = st->t[n.in2].grad + a.koff; p.dv = st->t[n.in2].grad + a.voff;
  p.B = a.nb; p.heads = a.heads; p.hd = a.hd; p.Lq = a.Lq; p.Lk = a.Lk;
  p.ldq = st->t[n.in].cols; p.ldk = p.ldv = st->t[n.in2].cols; p.ldo = a.heads * a.hd;
  p.dropmask = a.drop.mask; p.dropscale = a.drop.scale;
  TCHK(launch_attn_train_bwd(p, s));
  return D2T_OK;
}

// nn.Dropout(p): out = in * mask / (1 - p); identity (no node) when p == 0
int Tr::dropout(int in, int* out, float p) {  // p < 0: the decoder's configured rate (d2t_train_set_dropout)
  if (p < 0.f) p = st->drop_p;
  if (p <= 0.f) { *out = in; return D2T_OK; }
  Node n = node(N_DROPOUT, in);
  n.drop.scale = 1.f / (1.f - p);
  RC(new_mask((size_t)st->t[in].rows * st->t[in].cols, &n.drop.mask, p));
  return map_node(n, out, [&](const float* x, float* y, size_t k) { return launch_apply_mask(x, n.drop.mask, n.drop.scale, y, k, s); });
}
int Tr::bwd_dropout(const Node& n) {
  return grad_to(n.in, [&](float* dx, size_t k) { return launch_apply_mask(st->t[n.out].grad, n.drop.mask, n.drop.scale, dx, k, s); });
}

int Tr::add(int a, int b, int* out) {
  return map_node(node(N_ADD, a, b), out, [&](const float* x, float* y, size_t k) { return launch_ew(x, st->t[b].p, y, k, EW_ADD, s); });
}
int Tr::bwd_add(const Node& n) {  // both operands receive the gradient; the second gets its own copy unless it only accumulates
  float* g = st->t[n.out].grad;
  RC(add_grad(n.in, g));
  if (!st->t[n.in2].grad) {
    const TT& y = st->t[n.out];
    float* cp;
    RC(alloc(&cp, (size_t)y.rows * y.cols));
    TCHK(launch_copy(g, cp, (size_t)y.rows * y.cols, s));
    g = cp;
  }
  return add_grad(n.in2, g);
}

int Tr::gelu(int in, int* out) {
  return map_node(node(N_GELU, in), out, [&](const float* x, float* y, size_t k) { return launch_ew(x, nullptr, y, k, EW_GELU, s); });
}
int Tr::bwd_gelu(const Node& n) {
  return grad_to(n.in, [&](float* dx, size_t k) { return launch_ew(st->t[n.out].grad, st->t[n.in].p, dx, k, EW_GELU_BWD, s); });
}

int Tr::relu(int in, int* out) {
  return map_node(node(N_RELU, in), out, [&](const float* x, float* y, size_t k) { return launch_ew(x, nullptr, y, k, EW_RELU, s); });
}
int Tr::bwd_relu(const Node& n) {
  return grad_to(n.in, [&](float* dx, size_t k) { return launch_ew(st->t[n.out].grad, st->t[n.out].p, dx, k, EW_RELU_BWD, s); });
}

// out[b] = in[b] + table  (PositionalEncoding2D of the ResNet+None encoder, recognizers/build_seq.py:69-76)
int Tr::add_const(int in, const float* table, int* out) {
  const int B = st->t[in].B;
  return map_node(node(N_ADDCONST, in), out, [&](const float* x, float* y, size_t k) { return add_rows_each(x, k / B, table, 0, y, B, (int)(k / B)); });
}
int Tr::bwd_add_const(const Node& n) { return add_grad(n.in, st->t[n.out].grad); }

// The two nodes of GlobalContext.forward (addon_module/visual_attention.py:147-165; train_models.hip global_context) that
// are no ordinary layers.  gc_pool: a 1x1-conv attention map over the H*W positions, softmax, the attention-pooled
// channel vector: ctx[b] = sum_p a[b][p] x[b][p], a = softmax_p(x . wg + bg); key: "...global_cxt".
int Tr::gc_pool(int in, const std::string& key, int* out) {
  const TT x = st->t[in];
  const int B = x.B, HW = x.H * x.W, C = x.cols;
  const float *wg, *bg;
  RC(raw(key + ".weight", &wg, C));
  RC(raw(key + ".bias", &bg, 1));
  Node n = node(N_GCPOOL, in);
  n.gcpool.key = key;
  RC(alloc(&n.gcpool.logits, (size_t)B * HW));  // kept for the backward pass
  TCHK(launch_gc_logits(x.p, wg, bg, n.gcpool.logits, (long long)B * HW, C, s));
  RC(new_tensor(B, C, out));
  TCHK(launch_gc_pool(x.p, n.gcpool.logits, st->t[*out].p, B, HW, C, s));
  return push(n, *out);
}
int Tr::bwd_gc_pool(const Node& n) {
  const TT& x = st->t[n.in];
  const int B = x.B, HW = x.H * x.W, C = x.cols;
  const float* dctx = st->t[n.out].grad;
  const float* wg;
  RC(raw(n.gcpool.key + ".weight", &wg, C));
  float *a, *dl, *sdl, *dx, *dwg_b, *dwg, *dbg;
  RC(alloc(&a, (size_t)B * HW));
  RC(alloc(&dl, (size_t)B * HW));
  RC(alloc(&sdl, B));
  TCHK(launch_gc_pool_bwd_weights(x.p, n.gcpool.logits, dctx, st->t[n.out].p, a, dl, sdl, B, HW, C, s));
  RC(alloc(&dx, (size_t)x.rows * C));
  TCHK(launch_gc_pool_bwd_dx(a, dl, dctx, wg, dx, B, HW, C, s));
  RC(add_grad(n.in, dx));
  // d wg[c] = sum_b sum_p dl[b][p] x[b][p][c]; d bg = sum dl (zero up to rounding: a softmax ignores a shift)
  RC(alloc(&dwg_b, (size_t)B * C));
  RC(ensure_part((size_t)B * GC_CHUNKS * C));
  TCHK(launch_gc_wpool(x.p, dl, st->part, dwg_b, B, HW, C, s));
  RC(grad_buf(n.gcpool.key + ".weight", &dwg));
  RC(colsum(dwg_b, B, C, dwg));
  RC(grad_buf(n.gcpool.key + ".bias", &dbg));
  TCHK(launch_sum_small(sdl, B, dbg, s));
  return D2T_OK;
}

// bcast_add: out[b][p] = in[b][p] + y[b], the block's result added to every position
int Tr::bcast_add(int in, int y, int* out) {
  const TT x = st->t[in];
  RC(new_tensor(x.rows, x.cols, out, x.B, x.H, x.W));
  TCHK(launch_gc_bcast_add(x.p, st->t[y].p, st->t[*out].p, x.B, x.H * x.W, x.cols, s));
  Node n = node(N_BCAST, in, y);
  return push(n, *out);
}
int Tr::bwd_bcast_add(const Node& n) {  // dx = dout; dy[b][c] = sum over the image's positions
  const TT& x = st->t[n.in];
  const TT& o = st->t[n.out];
  const int B = x.B, HW = x.H * x.W, C = x.cols;
  float *dy, *dx;
  RC(alloc(&dy, (size_t)B * C));
  RC(ensure_part((size_t)B * GC_CHUNKS * C));
  TCHK(launch_gc_wpool(o.grad, nullptr, st->part, dy, B, HW, C, s));
  RC(add_grad(n.in2, dy));
  RC(alloc(&dx, (size_t)x.rows * C));
  TCHK(hipMemcpyAsync(dx, o.grad, (size_t)x.rows * C * 4, hipMemcpyDeviceToDevice, s));
  return add_grad(n.in, dx);
}

// The ViT's token rows from the gh x gw patch tokens (vit_encoder.py:249-262): [cls + pos[0] | patch + pos[1:]]; p: the
// encoder's key prefix
int Tr::tokens(int patch, const std::string& p, int gh, int gw, int* out) {
  const d2t_config& g = c->cfg;
  const int D = g.vit_dim, B = st->t[patch].B, n = gh * gw;
  const float *cls, *pos;
  RC(raw(p + "cls_token", &cls, D));
  const RawW* pr;
  RC(need(c, p + "pos_embed", &pr));
  pos = pr->p;
  // ViTEncoder (learned table, vit_encoder.py:58-95): a crop whose patch grid is not max_dimension's reads the table through a
  // bicubic resize, rebuilt every step (the table is being trained)
  int GH = 0, GW = 0;
  if (d2t_encoder_shape(c, g.max_h, g.max_w, nullptr, nullptr, &GH, &GW, nullptr, nullptr) || (long long)pr->numel != (long long)(GH * GW + 1) * D)
    return fail(c, D2T_EINVAL, "pos_embed does not match max_dimension's patch grid");
  const PosGrid pg = pos_grid(g, GH, GW, gh, gw);
  if (pg.interp) {
    float* tbl;
    RC(alloc(&tbl, (size_t)(n + 1) * D));
    TCHK(launch_copy(pos, tbl, (size_t)D, s));
    TCHK(launch_bicubic_table(pos + D, tbl + D, GH, GW, gh, gw, D, pg.sh, pg.sw, s));
    pos = tbl;
  } else if ((long long)pr->numel < (long long)(n + 1) * D) {
    return fail(c, D2T_EINVAL, "pos_embed too small for %d tokens", n + 1);
  }
  RC(new_tensor((long long)B * (n + 1), D, out));
  float* x = st->t[*out].p;
  TCHK(launch_token_rows(st->t[patch].p, x, B, n, 1, D, 1, s));          // scatter, cls rows zero
  TCHK(launch_fill_cls(cls, x, B, (long long)(n + 1) * D, D, s));
  // + pos_embed[:, :n+1] (flat prefix slice, vit_encoder.py:260), broadcast over the batch
  TCHK(add_rows_each(x, (size_t)(n + 1) * D, pos, 0, x, B, (n + 1) * D));
  Node tn = node(N_TOKENS, patch);
  tn.tokens.ntok = n; tn.tokens.cls_key = p + "cls_token";
  tn.tokens.table_h = GH; tn.tokens.table_w = GW; tn.tokens.crop_h = gh; tn.tokens.crop_w = gw;
  // a learned table receives a gradient (ViTEncoderV3's is frozen, :235-237)
  if (g.vit_pos != D2T_VIT_POS_SINCOS_PREFIX) tn.tokens.pos_key = p + "pos_embed";
  return push(tn, *out);
}
int Tr::bwd_tokens(const Node& n) {
  const Node::Tokens& k = n.tokens;
  const TT& y = st->t[n.out];
  const TT& x = st->t[n.in];
  const int D = y.cols, nb = (int)(y.rows / (k.ntok + 1));
  float *dcls, *dx;
  RC(grad_buf(k.cls_key, &dcls));
  TCHK(launch_sum_rows_strided(y.grad, dcls, nb, k.ntok + 1, 0, D, s));
  RC(alloc(&dx, (size_t)x.rows * D));
  TCHK(launch_token_rows(y.grad, dx, nb, k.ntok, 1, D, 0, s));
  if (!k.pos_key.empty()) {
    // d pos_embed: the table is broadcast over the batch, so its gradient is the sum of the token gradients over the batch --
    // written to the first ntok + 1 rows (prefix slice / table as is) or, for a resized table, pulled back through the
    // transpose of the bicubic resize; rows the crop did not read get zero
    const PosGrid pg = pos_grid(c->cfg, k.table_h, k.table_w, k.crop_h, k.crop_w);
    float* dpos;
    RC(grad_buf(k.pos_key, &dpos));
    const size_t rows = (size_t)k.ntok + 1, all = (size_t)k.table_h * k.table_w + 1;
    if (!pg.interp) {
      TCHK(launch_sum_over_batch(y.grad, dpos, nb, (long long)(rows * D), (long long)(rows * D), s));
      if (all > rows) TCHK(hipMemsetAsync(dpos + rows * D, 0, (all - rows) * D * 4, s));
    } else {
      float* dt;
      RC(alloc(&dt, rows * D));
      TCHK(launch_sum_over_batch(y.grad, dt, nb, (long long)(rows * D), (long long)(rows * D), s));
      TCHK(launch_copy(dt, dpos, (size_t)D, s));
      TCHK(launch_bicubic_table_bwd(dt + D, dpos + D, k.table_h, k.table_w, k.crop_h, k.crop_w, D, pg.sh, pg.sw, s));
    }
  }
  return add_grad(n.in, dx);
}

// The TFM head's input rows: word_embed[tgt] * sqrt(D) + pos_enc (tfm.py:103-106); p: the head's key prefix
int Tr::embed(const int64_t* tgt, int B, int L, const std::string& p, int* out) {
  const d2t_config& g = c->cfg;
  const int D = g.dec_dim;
  const float *E, *pe;
  RC(raw(p + "word_embed.weight", &E, (size_t)g.vocab * D));
  RC(raw(p + "pos_enc.pe", &pe));
  RC(new_tensor((long long)B * L, D, out));
  TCHK(launch_embed_train(E, pe, tgt, st->t[*out].p, B * L, L, D, sqrtf((float)D), s));
  Node n = node(N_EMBED, -1);
  n.embed.key = p + "word_embed.weight";
  return push(n, *out);
}
int Tr::bwd_embed(const Node& n) {
  float* dE;
  RC(grad_buf(n.embed.key, &dE));
  const d2t_config& g = c->cfg;
  TCHK(launch_embed_bwd(st->t[n.out].grad, st->tgt, dE, st->B * st->L, g.vocab, g.dec_dim, sqrtf((float)g.dec_dim), 0, s));
  return D2T_OK;
}

// nn.LSTM(bidirectional, batch_first) of a BidirectionalLSTM (seq_modeling/bilstm.py:14-24; key: "...rnn.").  The input
// projection of both directions is one GEMM on the engine's packed copies (c->lstm[i]: finalized weights).
int Tr::bilstm(int in, int layer, const std::string& key, int B, int T, int* out) {
  const TT x = st->t[in];
  const int Hh = c->cfg.bilstm_hidden;
  const BiLstmW& L = c->lstm[layer];
  if (!c->finalized || !L.wih_cat || x.cols != L.in) return fail(c, D2T_ESTATE, "BiLSTM weights are not finalized");
  Node n = node(N_BILSTM, in);
  Node::BiLstm& b = n.bilstm;
  b.key = key; b.layer = layer; b.in_width = L.in; b.B = B; b.T = T;
  float* gates;
  RC(alloc(&gates, (size_t)B * T * 8 * Hh));
  RC(gemm_nt(x.p, L.wih_cat, L.bias_cat, nullptr, gates, (long long)B * T, 8 * Hh, L.in, ACT_NONE));
  RC(alloc(&b.gates, (size_t)B * T * 8 * Hh));
  RC(alloc(&b.cells, (size_t)B * T * 2 * Hh));
  RC(new_tensor((long long)B * T, 2 * Hh, out));
  TCHK(launch_bilstm_train_fwd(gates, L.whh_t, st->t[*out].p, b.gates, b.cells, B, T, Hh, s));
  return push(n, *out);
}
int Tr::bwd_bilstm(const Node& n) {
  const Node::BiLstm& b = n.bilstm;
  const int B = b.B, T = b.T, Hh = c->cfg.bilstm_hidden, in = b.in_width;
  const long long R = (long long)B * T;
  const TT& x = st->t[n.in];
  const TT& rec = st->t[n.out];
  const float *whh_f, *whh_r;
  RC(raw(b.key + "weight_hh_l0", &whh_f, (size_t)4 * Hh * Hh));
  RC(raw(b.key + "weight_hh_l0_reverse", &whh_r, (size_t)4 * Hh * Hh));
  float *dgates, *hpf, *hpr;
  RC(alloc(&dgates, (size_t)R * 8 * Hh));
  TCHK(launch_bilstm_train_bwd(rec.grad, b.gates, b.cells, whh_f, whh_r, dgates, B, T, Hh, s));
  RC(alloc(&hpf, (size_t)R * Hh));
  RC(alloc(&hpr, (size_t)R * Hh));
  TCHK(launch_bilstm_hprev(rec.p, hpf, hpr, B, T, Hh, s));
  float *bsum, *g;
  RC(alloc(&bsum, (size_t)8 * Hh));
  RC(colsum(dgates, R, 8 * Hh, bsum));
  const char* sfx[2] = {"", "_reverse"};
  for (int d = 0; d < 2; ++d) {
    const float* dg = dgates + (size_t)d * 4 * Hh;
    RC(linear_grads(b.key + "weight_ih_l0" + sfx[d], "", dg, 8 * Hh, x.p, in, R, 4 * Hh, in));
    RC(linear_grads(b.key + "weight_hh_l0" + sfx[d], "", dg, 8 * Hh, d == 0 ? hpf : hpr, Hh, R, 4 * Hh, Hh));
    RC(grad_buf(b.key + "bias_ih_l0" + sfx[d], &g));
    TCHK(launch_copy(bsum + (size_t)d * 4 * Hh, g, (size_t)4 * Hh, s));
    RC(grad_buf(b.key + "bias_hh_l0" + sfx[d], &g));
    TCHK(launch_copy(bsum + (size_t)d * 4 * Hh, g, (size_t)4 * Hh, s));
  }
  // dx = dgates @ [W_ih ; W_ih_reverse]  ([R][8H] x [8H][in])
  float* dx;
  RC(gemm_gw(dgates, R, 8 * Hh, in, c->lstm[b.layer].wih_cat, &dx));
  return add_grad(n.in, dx);
}

// Attention / AttentionV2.forward_greedy under is_train with teacher_forcing = 1 (seq2seq.py:224-331) over the memory
// `mem` and its key projection `kp`: the whole loop is one launch of the greedy kernel fed with the label tokens; its
// per-step state is kept for bwd_lstm.
int Tr::lstm_head(int mem, int kp, const int64_t* tgt, int B, int S, float* logits, int* out) {
  const d2t_config& g = c->cfg;
  const int Hh = g.attn_hidden, V = g.vocab, T = (int)(st->t[mem].rows / B);
  const int key_off = g.attn_keys == D2T_ATTN_KEYS_NOCLS_INIT_CLS ? 1 : 0, Tk = T - key_off;
  Node n = node(N_LSTM, mem, kp);
  Node::Lstm& L = n.lstm;
  L.B = B; L.S = S; L.T = T; L.key_off = key_off;
  const size_t BS = (size_t)B * S;
  RC(alloc(&L.h_prev, BS * Hh));
  RC(alloc(&L.c_prev, BS * Hh));
  RC(alloc(&L.h_after, BS * Hh));
  RC(alloc(&L.c_after, BS * Hh));
  RC(alloc(&L.gates, BS * 4 * Hh));
  RC(alloc(&L.alpha, BS * Tk));
  RC(alloc(&L.hq, BS * Hh));
  RC(alloc(&L.ctx_emb, BS * 2 * Hh));
  float *dummy, *tokbuf;
  RC(alloc(&dummy, BS * 2 + B + 16));  // tokens (int64) and end_step scratch
  RC(alloc(&tokbuf, BS * 2 + 2));      // input token per (row, step), int64
  L.tokens = reinterpret_cast<const int64_t*>(tokbuf);
  RC(new_tensor((long long)BS, V, out, 0, 0, 0, logits));
  if (st->drop_p > 0.f) {  // nn.Dropout(droprate) on the generator output of every step (seq2seq.py:298)
    RC(new_mask(BS * V, &L.drop.mask));
    L.drop.scale = 1.f / (1.f - st->drop_p);
  }
  const uint8_t* d_flags = nullptr;
  if (!st->teacher_flags.empty()) {
    if ((int)st->teacher_flags.size() != S) return fail(c, D2T_EINVAL, "teacher flags: %zu entries for %d steps", st->teacher_flags.size(), S);
    float* fb;
    RC(alloc(&fb, S / 4 + 2));
    TCHK(hipMemcpyAsync(fb, st->teacher_flags.data(), S, hipMemcpyHostToDevice, s));
    TCHK(hipStreamSynchronize(s));  // the host vector may change before an asynchronous copy would run
    d_flags = reinterpret_cast<const uint8_t*>(fb);
  }
  L.init_mode = !g.attn_enc_init ? 0 : (g.attn_keys == D2T_ATTN_KEYS_ALL_INIT_MEAN ? 1 : 2);
  AttnDecP p{};
  p.mem = st->t[mem].p; p.T = T; p.D = Hh; p.key_off = key_off; p.init_mode = L.init_mode;
  p.kp = st->t[kp].p; p.wq_t = c->attn.wq_t; p.bq = c->attn.bq; p.wloc = c->attn.wloc; p.bloc = c->attn.bloc;
  p.taps = c->attn.taps; p.wscore = c->attn.wscore; p.bscore = c->attn.bscore;
  p.wx_t = c->attn.wx_t; p.bx = c->attn.bx; p.wg_t = c->attn.wg_t; p.bg = c->attn.bg;
  p.wih_t = c->attn.wih_t; p.bih = c->attn.bih; p.wic_t = c->attn.wic_t; p.bic = c->attn.bic;
  p.emb = c->attn.emb; p.tokgate = c->attn.tokgate; p.probs = logits; p.tokens = reinterpret_cast<int64_t*>(dummy);
  p.end_step = reinterpret_cast<int*>(dummy + BS * 2);
  p.B = B; p.S = S; p.V = V; p.H = Hh; p.E = Hh; p.coverage = g.attn_coverage; p.end_token = 1;
  p.teacher = tgt; p.use_teacher = d_flags; p.out_dropmask = L.drop.mask; p.out_dropscale = L.drop.scale;
  p.sv_tok = reinterpret_cast<int64_t*>(tokbuf);
  p.sv_hprev = L.h_prev; p.sv_cprev = L.c_prev; p.sv_hafter = L.h_after; p.sv_cafter = L.c_after;
  p.sv_gates = L.gates; p.sv_alpha = L.alpha; p.sv_hq = L.hq; p.sv_x = L.ctx_emb;
  TCHK(launch_attn_decode(p, s));
  return push(n, *out);
}
int Tr::bwd_lstm(const Node& n) {
  const Node::Lstm& L = n.lstm;
  const d2t_config& g = c->cfg;
  const int B = L.B, S = L.S, T = L.T, Hh = g.attn_hidden, V = g.vocab, key_off = L.key_off;
  const int taps = c->attn.taps, kd = g.attn_kernel_dim;
  const long long BS = (long long)B * S;
  const std::string pp = "predicter.Prediction.", ac = pp + "attention_cell.";
  const TT& mem = st->t[n.in];
  const TT& kp = st->t[n.in2];
  const float* dl = st->t[n.out].grad;
  if (L.drop.mask) {  // output dropout: everything upstream sees the masked, rescaled gradient
    float* dlm;
    RC(alloc(&dlm, (size_t)BS * V));
    TCHK(launch_apply_mask(dl, L.drop.mask, L.drop.scale, dlm, (size_t)BS * V, s));
    dl = dlm;
  }
  // Bahdanau cell: h2h is the query projection, no location layers, no score bias (the kernel's location filter is the
  // zero filter the forward pass used).  One-hot targets: rnn.weight_ih is [4H][H + V]; the kernel gets its context
  // columns beside a zero "embedding" block, and the token columns' gradients are gathered per token below.
  const bool bahdanau = g.attn_cell == D2T_ATTN_CELL_BAHDANAU, onehot = g.attn_onehot != 0;
  const std::string qk = ac + (bahdanau ? "attn.h2h" : "attn.query_proj");
  const float *wih, *whh, *wq, *cw = nullptr, *cb = nullptr, *pw = nullptr;
  RC(raw(ac + "rnn.weight_ih", &wih));
  RC(raw(ac + "rnn.weight_hh", &whh));
  RC(raw(qk + ".weight", &wq));
  if (!bahdanau) {
    RC(raw(ac + "attn.loc_conv.weight", &cw));
    RC(raw(ac + "attn.loc_conv.bias", &cb));
    RC(raw(ac + "attn.loc_proj.weight", &pw));
  }
  if (onehot) {
    float* wc;
    RC(zeros(&wc, (size_t)4 * Hh * 2 * Hh));
    TCHK(launch_copy2d(wih, Hh + V, wc, 2 * Hh, (size_t)4 * Hh, Hh, s));
    wih = wc;
  }
  AttnTrainBwdP p{};
  p.dlogits = dl; p.mem = mem.p; p.T = T; p.D = Hh; p.key_off = key_off; p.kp = kp.p;
  p.wg_t = c->attn.wg_t; p.wih_raw = wih; p.whh_raw = whh; p.wq_raw = wq; p.wloc = c->attn.wloc; p.bloc = c->attn.bloc;
  p.wscore = c->attn.wscore; p.taps = taps;
  p.sv_cprev = L.c_prev; p.sv_cafter = L.c_after; p.sv_gates = L.gates; p.sv_alpha = L.alpha; p.sv_hq = L.hq;
  float *dmem, *dkp, *dgates, *dhq, *demb, *dh0, *dc0, *dwloc, *dbloc, *dwscore, *dbscore;
  RC(zeros(&dmem, (size_t)mem.rows * mem.cols));
  RC(zeros(&dkp, (size_t)kp.rows * kp.cols));
  RC(alloc(&dgates, (size_t)BS * 4 * Hh));
  RC(alloc(&dhq, (size_t)BS * Hh));
  RC(alloc(&demb, (size_t)BS * Hh));
  RC(alloc(&dh0, (size_t)B * Hh));
  RC(alloc(&dc0, (size_t)B * Hh));
  RC(alloc(&dwloc, (size_t)B * Hh * taps));
  RC(alloc(&dbloc, (size_t)B * Hh));
  RC(alloc(&dwscore, (size_t)B * Hh));
  RC(alloc(&dbscore, (size_t)B + 16));
  p.dmem = dmem; p.dkp = dkp; p.dgates = dgates; p.dhq = dhq; p.dh0 = dh0; p.dc0 = dc0;
  p.dwloc = dwloc; p.dbloc = dbloc; p.dwscore = dwscore; p.dbscore = dbscore;
  p.B = B; p.S = S; p.V = V; p.H = Hh; p.E = Hh; p.coverage = g.attn_coverage;
  // The two products that do not take part in the recurrence leave the sequential kernel (each cost its weight matrix
  // per row and step from L2): dlogits . generator.weight for all (row, step) as one GEMM before it ...
  static const bool hoist = !(D2T_PROBE_ENV_STR("D2T_LSTM_BWD_HOIST") && D2T_PROBE_ENV("D2T_LSTM_BWD_HOIST") == 0);
  if (hoist) {
    const int Vp = (V + 31) / 32 * 32;
    float *gpad, *wgp, *dhl;
    RC(alloc(&gpad, (size_t)BS * Vp));
    RC(alloc(&wgp, (size_t)Hh * Vp));
    RC(alloc(&dhl, (size_t)BS * Hh));
    TCHK(launch_pad_cols(dl, gpad, (size_t)BS, V, Vp, s));
    TCHK(launch_pad_cols(c->attn.wg_t, wgp, (size_t)Hh, V, Vp, s));
    RC(gemm_nt(gpad, wgp, nullptr, nullptr, dhl, BS, Hh, Vp, ACT_NONE));
    p.dhl = dhl;
    p.demb = nullptr;
  } else {
    p.demb = demb;
  }
  TCHK(launch_attn_train_lstm_bwd(p, s));
  // ... and the gradient of the embedded target, dgates . W_ih[:, H:], as one GEMM after it (not needed with one-hot targets)
  if (hoist && !onehot) RC(gemm_nt(dgates, c->attn.wx_t + (size_t)Hh * 4 * Hh, nullptr, nullptr, demb, BS, Hh, 4 * Hh, ACT_NONE));
  float *gW, *gB, *gB2;
  RC(linear_grads(ac + "generator.weight", ac + "generator.bias", dl, V, L.h_after, Hh, BS, V, Hh));
  if (!onehot) {
    RC(linear_grads(ac + "rnn.weight_ih", "", dgates, 4 * Hh, L.ctx_emb, 2 * Hh, BS, 4 * Hh, 2 * Hh));
  } else {  // columns [0, H): the context part; column H + v: the sum of the gate gradients of the steps fed token v
    float *gc, *gt, *gtt;
    RC(grad_buf(ac + "rnn.weight_ih", &gW));
    RC(alloc(&gc, (size_t)4 * Hh * Hh));
    RC(alloc(&gt, (size_t)V * 4 * Hh));
    RC(alloc(&gtt, (size_t)4 * Hh * V));
    RC(wgrad(dgates, 4 * Hh, L.ctx_emb, 2 * Hh, BS, 4 * Hh, Hh, 1, nullptr, nullptr, nullptr, gc, 0));
    TCHK(launch_copy2d(gc, Hh, gW, Hh + V, (size_t)4 * Hh, Hh, s));
    TCHK(launch_embed_bwd(dgates, L.tokens, gt, (int)BS, V, 4 * Hh, 1.f, -1, s));
    TCHK(launch_transpose(gt, gtt, V, 4 * Hh, s));
    TCHK(launch_copy2d(gtt, V, gW + Hh, Hh + V, (size_t)4 * Hh, V, s));
  }
  RC(linear_grads(ac + "rnn.weight_hh", "", dgates, 4 * Hh, L.h_prev, Hh, BS, 4 * Hh, Hh));
  RC(grad_buf(ac + "rnn.bias_ih", &gB));
  RC(grad_buf(ac + "rnn.bias_hh", &gB2));
  RC(colsum(dgates, BS, 4 * Hh, gB));
  TCHK(launch_copy(gB, gB2, (size_t)4 * Hh, s));
  RC(linear_grads(qk + ".weight", qk + ".bias", dhq, Hh, L.h_prev, Hh, BS, Hh, Hh));
  RC(grad_buf(ac + "attn.score.weight", &gW));
  TCHK(launch_sum_over_rows(dwscore, gW, B, Hh, s));
  if (!bahdanau) {
    RC(grad_buf(ac + "attn.score.bias", &gB));
    TCHK(launch_sum_over_rows(dbscore, gB, B, 1, s));
    float *gcw, *gcb, *gpw, *gpb;
    RC(grad_buf(ac + "attn.loc_conv.weight", &gcw));
    RC(grad_buf(ac + "attn.loc_conv.bias", &gcb));
    RC(grad_buf(ac + "attn.loc_proj.weight", &gpw));
    RC(grad_buf(ac + "attn.loc_proj.bias", &gpb));
    TCHK(launch_loc_unfold_bwd(dwloc, dbloc, B, cw, cb, pw, Hh, kd, taps, gcw, gcb, gpw, gpb, s));
  }
  if (!onehot) {
    RC(grad_buf(pp + "embedding.weight", &gW));
    TCHK(launch_embed_bwd(demb, L.tokens, gW, (int)BS, V, Hh, 1.f, 0, s));  // padding_idx = [GO] = 0 (seq2seq.py:33-35)
  }
  if (g.attn_enc_init) {  // h0 / c0 = proj_init_{h,c}(memory[:, 0]) or, on a BiLSTM encoder, of the mean over the tokens
    const bool mean = L.init_mode == 1;
    const float* initv = mem.p;  // row b = memory[b][0] with a row stride of T * Hh
    int ldi = T * Hh;
    if (mean) {
      float *sums, *mv;
      RC(alloc(&sums, (size_t)B * Hh));
      RC(alloc(&mv, (size_t)B * Hh));
      RC(ensure_part((size_t)B * GC_CHUNKS * Hh));
      TCHK(launch_gc_wpool(mem.p, nullptr, st->part, sums, B, T, Hh, s));
      TCHK(launch_scale(sums, mv, (size_t)B * Hh, 1.f / T, s));
      initv = mv;
      ldi = Hh;
    }
    RC(linear_grads(pp + "proj_init_h.weight", pp + "proj_init_h.bias", dh0, Hh, initv, ldi, B, Hh, Hh));
    RC(linear_grads(pp + "proj_init_c.weight", pp + "proj_init_c.bias", dc0, Hh, initv, ldi, B, Hh, Hh));
    float *t1, *dinit;
    RC(alloc(&t1, (size_t)B * Hh));
    RC(alloc(&dinit, (size_t)B * Hh));
    RC(gemm_nt(dh0, c->attn.wih_t, nullptr, nullptr, t1, B, Hh, Hh, ACT_NONE));
    RC(gemm_nt(dc0, c->attn.wic_t, nullptr, t1, dinit, B, Hh, Hh, ACT_NONE));
    if (mean) {  // every token carries 1 / T of the initial state's gradient
      float *dsc, *dmem2;
      RC(alloc(&dsc, (size_t)B * Hh));
      TCHK(launch_scale(dinit, dsc, (size_t)B * Hh, 1.f / T, s));
      RC(alloc(&dmem2, (size_t)mem.rows * mem.cols));
      TCHK(launch_gc_bcast_add(dmem, dsc, dmem2, B, T, Hh, s));
      dmem = dmem2;
    } else {
      TCHK(add_rows_each(dmem, (size_t)T * Hh, dinit, Hh, dmem, B, Hh));
    }
  }
  RC(add_grad(n.in, dmem));
  RC(add_grad(n.in2, dkp));
  return D2T_OK;
}

// ---------------- backward ----------------
int Tr::backward() {
  for (int i = (int)st->nodes.size() - 1; i >= 0; --i) {
    const Node& n = st->nodes[i];
    if (!st->t[n.out].grad) continue;
    switch (n.kind) {
      case N_CONV: RC(bwd_conv(n)); break;
      case N_POOL: RC(bwd_pool(n)); break;
      case N_MEANH: RC(bwd_mean_h(n)); break;
      case N_LINEAR: RC(bwd_linear(n)); break;
      case N_LN: RC(bwd_ln(n)); break;
      case N_ATTN: RC(bwd_attn(n)); break;
      case N_DROPOUT: RC(bwd_dropout(n)); break;
      case N_ADD: RC(bwd_add(n)); break;
      case N_GELU: RC(bwd_gelu(n)); break;
      case N_RELU: RC(bwd_relu(n)); break;
      case N_ADDCONST: RC(bwd_add_const(n)); break;
      case N_GCPOOL: RC(bwd_gc_pool(n)); break;
      case N_BCAST: RC(bwd_bcast_add(n)); break;
      case N_TOKENS: RC(bwd_tokens(n)); break;
      case N_EMBED: RC(bwd_embed(n)); break;
      case N_BILSTM: RC(bwd_bilstm(n)); break;
      case N_LSTM: RC(bwd_lstm(n)); break;
    }
    // gradients this node wrote are final once the stream reaches this point (a parameter written by several
    // nodes is re-recorded by each): d2t_train_grad on another stream waits for exactly this
    for (const std::string& k : st->touched) TCHK(hipEventRecord(st->ready[k], s));
    st->touched.clear();
  }
  return D2T_OK;
}

}  // namespace tape
