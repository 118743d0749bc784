// libd2t engine: context life cycle, weight packing, the decode-stream pool, backbone and encoders, setters and profiling
// of the C-ABI declared in include/d2t.h (the decodes: engine_tfm.hip, engine_attn.hip; the d2t_op_* entries:
// engine_ops.hip).  Host code only launches the kernels of the other .hip files on the caller's HIP stream; there is no
// CPU compute path and no fallback.
#include "engine_impl.h"
#include <mutex>

namespace {

int pack_conv(d2t_ctx* c, const std::string& conv, const std::string& bn, ConvW* out, hipStream_t s) {
  const RawW *w, *g = nullptr, *b = nullptr, *mu = nullptr, *var = nullptr;
  int rc = need(c, conv + ".weight", &w);
  if (rc) return rc;
  if (w->shape.size() != 4) return fail(c, D2T_EINVAL, "conv weight '%s' is not 4-D", conv.c_str());
  const RawW* cb = find(c, conv + ".bias");
  if (!bn.empty()) {
    if ((rc = need(c, bn + ".weight", &g)) || (rc = need(c, bn + ".bias", &b)) ||
        (rc = need(c, bn + ".running_mean", &mu)) || (rc = need(c, bn + ".running_var", &var)))
      return rc;
  }
  out->Cout = (int)w->shape[0]; out->Cin = (int)w->shape[1]; out->KH = (int)w->shape[2]; out->KW = (int)w->shape[3];
  void *pw, *pb;
  if ((rc = dev_alloc(c, &pw, w->numel * 4)) || (rc = dev_alloc(c, &pb, (size_t)out->Cout * 4))) return rc;
  c->owned.push_back(pw);
  c->owned.push_back(pb);
  out->w = (float*)pw;
  out->bias = (float*)pb;
  HIPCHK(c, launch_pack_conv(w->p, cb ? cb->p : nullptr, g ? g->p : nullptr, b ? b->p : nullptr, mu ? mu->p : nullptr,
                             var ? var->p : nullptr, 1e-5f, out->w, out->bias, out->Cout, out->Cin, out->KH, out->KW,
                             s));
  out->w_h16 = out->w_l16 = nullptr;  // fp16 hi / lo planes: made on first use (f16_planes), only the two-MFMA modes read them
  if (out->Cin % 32 == 0) {  // bf16 hi/lo planes of the folded weights (bf16x3 kernel)
    void *ph = nullptr, *pl = nullptr;
    if ((rc = dev_alloc(c, &ph, w->numel * 2))) return rc;
    c->owned.push_back(ph);
    if ((rc = dev_alloc(c, &pl, w->numel * 2))) return rc;
    c->owned.push_back(pl);
    out->w_hi = (uint16_t*)ph;
    out->w_lo = (uint16_t*)pl;
    HIPCHK(c, launch_split_bf16(out->w, out->w_hi, out->w_lo, w->numel, s));
  }
  return D2T_OK;
}
// fp16 hi / lo planes of a packed convolution weight (fp16x2 / mixed precision), created the first time a launch needs them:
// contexts that never leave split-bf16 (the default; training; fp32) do not pay their memory
int f16_planes(d2t_ctx* c, ConvW& w, hipStream_t s) {
  if (w.w_h16) return D2T_OK;
  if (!w.w || w.Cin % 32) return fail(c, D2T_ESTATE, "no fp16 planes for this layer");
  const size_t n = (size_t)w.Cout * w.KH * w.KW * w.Cin + (size_t)w.Cout * w.K2;
  void *qh = nullptr, *ql = nullptr;
  int rc;
  if ((rc = dev_alloc(c, &qh, n * 2))) return rc;
  c->owned.push_back(qh);
  if ((rc = dev_alloc(c, &ql, n * 2))) return rc;
  c->owned.push_back(ql);
  HIPCHK(c, launch_split_f16(w.w, (uint16_t*)qh, (uint16_t*)ql, n, s));
  w.w_h16 = (uint16_t*)qh;
  w.w_l16 = (uint16_t*)ql;
  return D2T_OK;
}
int get_lin(d2t_ctx* c, const std::string& k, LinW* out, int N, int K, bool bias = true) {
  const RawW *w, *b = nullptr;
  int rc;
  if ((rc = need(c, k + ".weight", &w, {N, K})) || (bias && (rc = need(c, k + ".bias", &b, {N})))) return rc;
  *out = LinW{w->p, b ? b->p : nullptr, N, K};
  return D2T_OK;
}
// bf16 hi/lo planes of a Linear's weight for the bf16x3 GEMM kernel (K % 32 == 0)
int split_planes(d2t_ctx* c, const float* w, size_t n, const uint16_t** hi, const uint16_t** lo, hipStream_t s) {
  void *ph, *pl;
  int rc;
  if ((rc = dev_alloc(c, &ph, n * 2)) || (rc = dev_alloc(c, &pl, n * 2))) return rc;
  c->owned.push_back(ph);
  c->owned.push_back(pl);
  HIPCHK(c, launch_split_bf16(w, (uint16_t*)ph, (uint16_t*)pl, n, s));
  *hi = (const uint16_t*)ph;
  *lo = (const uint16_t*)pl;
  return D2T_OK;
}
int split_lin(d2t_ctx* c, LinW* l, hipStream_t s) {
  if (l->K % 32) return D2T_OK;
  return split_planes(c, l->w, (size_t)l->N * l->K, &l->w_hi, &l->w_lo, s);
}

int get_ln(d2t_ctx* c, const std::string& k, LNW* out, int D) {
  const RawW *g, *b;
  int rc;
  if ((rc = need(c, k + ".weight", &g, {D})) || (rc = need(c, k + ".bias", &b, {D}))) return rc;
  *out = LNW{g->p, b->p};
  return D2T_OK;
}

void free_packed(d2t_ctx* c) {
  for (void* p : c->owned) hipFree(p);
  c->owned.clear();
  c->pos_interp.clear();  // resized copies of the previous position table (owned buffers)
  for (int i = 0; i < 4; ++i) c->layers[i].clear();
  c->vit.clear();
  c->dec.clear();
  c->finalized = false;
}

// spatial size after the backbone (resnet.py:205-245) for an H x W crop
void backbone_hw(int H, int W, int* oh, int* ow) {
  int h = H / 2, w = W / 2;          // maxpool1
  h /= 2; w /= 2;                    // maxpool2
  h = (h - 2) / 2 + 1; w = w + 1;    // maxpool3 k2 s(2,1) p(0,1)
  h = (h - 2) / 2 + 1; w = w + 1;    // conv4_1  k2 s(2,1) p(0,1)
  *oh = h - 1; *ow = w - 1;          // conv4_2  k2 s1 p0
}

// launch_conv, bracketed by HIP events on `s` while profiling is enabled
hipError_t conv_timed(d2t_ctx* c, const ConvP& p, hipStream_t s) {
  if (!c->profiling) return launch_conv(p, s);
  d2t_ctx::ProfRec r{p.M, p.Cout, p.K, nullptr, nullptr};
  hipError_t e;
  if ((e = hipEventCreate(&r.a)) != hipSuccess || (e = hipEventCreate(&r.b)) != hipSuccess) return e;
  if ((e = hipEventRecord(r.a, s)) != hipSuccess) return e;
  e = launch_conv(p, s);
  hipError_t e2 = hipEventRecord(r.b, s);
  c->prof.push_back(r);
  return e != hipSuccess ? e : e2;
}

// How a convolution behind the stem is routed (conv() and the patch embedding): split-record input brings the zero page and
// the block cap; fp16 records in select the two-MFMA kernels (x16 * w_lo + x16 * w_hi) on the layer's fp16 hi / lo weight
// planes, made on first use; the pipelined kernel's switches come from the context.
int conv_route(d2t_ctx* c, hipStream_t s, ConvP& p, ConvW& w, bool split_in, bool f16_in) {
  if (split_in) { p.zero16 = c->zero_page; p.max_blocks = c->conv_max_blocks; }
  if (split_in && f16_in) {
    if (int rc = f16_planes(c, w, s)) return rc;
    p.f16 = 1;
    p.w_hi = w.w_h16; p.w_lo = w.w_l16;
  }
  p.pipelined = c->conv_pipelined; p.reserved_cus = c->reserved_cus;
  p.split_tail = !c->decode_in_flight || D2T_PROBE_ENV("D2T_CONV_TAIL_ALWAYS");
  return D2T_OK;
}

// One convolution of the backbone.  `res` may be nullptr; `out_split` asks for split-bf16 output planes
// (only meaningful on the bf16x3 path; the consumer must be another bf16x3 convolution or the split pool).
// pool2: fuse the 2x2 / stride 2 max-pool that follows (split-record path only: see ConvP::pool2); y is then the POOLED map.
Act conv(d2t_ctx* c, hipStream_t s, hipError_t* err, const Act& x, const ConvW& w, int sh, int sw, int ph, int pw,
         int act, const Act* res, float* outbuf, const ConvP* extra = nullptr, bool out_split = false, bool pool2 = false,
         int out_fmt = -1) {
  // out_fmt: record format of a split output (conv_common.h REC_*); -1 = the input's (fp16x2 mode: one fp16; else bf16 hi | lo)
  Act y{outbuf, x.B, (x.H + 2 * ph - w.KH) / sh + 1, (x.W + 2 * pw - w.KW) / sw + 1, w.Cout};
  y.split = out_split;
  ConvP p{};
  if (extra) p = *extra;
  p.w = w.w; p.bias = w.bias;
  if (c->conv_bf16x3) { p.w_hi = w.w_hi; p.w_lo = w.w_lo; }
  if (x.split) p.in_hi = x.planes(); else p.in = x.p;
  if (conv_route(c, s, p, const_cast<ConvW&>(w), x.split, x.fmt != 0) != D2T_OK) {  // (w lives in *c)
    if (*err == hipSuccess) *err = hipErrorOutOfMemory;
    return y;
  }
  if (out_split) {
    y.fmt = out_fmt >= 0 ? out_fmt : (x.split ? (x.fmt ? 1 : 0) : (c->conv_f16 ? 1 : 0));
    p.out_fmt = 1 + y.fmt;
  }
  if (res && res->split) p.res_fmt = 1 + res->fmt;
  if (out_split) { p.out_hi = y.planes(); } else { p.out = outbuf; }
  if (res) {
    if (res->split) { p.res_hi = res->planes(); } else { p.res = res->p; }
  }
  conv_shape(p, x.B, x.H, x.W, x.C, w.Cout, w.KH, w.KW, sh, sw, ph, pw);
  p.K += p.Cin2;  // (a second 1x1 input from `extra`)
  p.act = act;
  if (pool2) {  // rows in pooled order (floor: a last odd row / column belongs to no window and is never computed)
    p.pool2 = 1;
    p.M = 4 * y.B * (y.H / 2) * (y.W / 2);
    y.H /= 2;
    y.W /= 2;
  }
  hipError_t e = conv_timed(c, p, s);
  if (e != hipSuccess && *err == hipSuccess) *err = e;
  return y;
}

// pick a rotating activation buffer that is not in `live`
float* pick(d2t_ctx* c, std::initializer_list<const float*> live) {
  for (int i = 0; i < 4; ++i) {
    bool used = false;
    for (const float* l : live) used |= (l == c->act[i]);
    if (!used) return c->act[i];
  }
  return nullptr;
}

// ResNet.forward (feature_extractor/resnet.py:205-245).  On the bf16x3 path every activation between the
// stem and the last convolution lives as split-bf16 planes; `final_split` says whether the returned map
// does too (a bf16x3 consumer follows) or is fp32 (final_out / any other consumer).
int run_backbone(d2t_ctx* c, hipStream_t s, const float* img, int B, int H, int W, Act* out, float* final_out,
                 const ConvP* final_extra, bool final_split) {
  hipError_t err = hipSuccess;
  // GlobalContext blocks read and update whole fp32 maps, so with gcb the activations stay fp32 (the convolutions still
  // take the split-bf16 kernel in bf16x3 mode, splitting their input on the fly)
  const bool sp = c->conv_bf16x3 && !c->cfg.gcb;
  Act x{pick(c, {}), B, H, W, c->stem.Cout};
  x.split = sp;
  const int f16 = sp && c->conv_f16;  // fp16 records between the stem and the last convolution
  x.fmt = f16;
  // mixed precision (ctx.h mixed_units): unit u of [layer3.1 .. layer3.4, conv3, layer4.0 .. layer4.2] runs the two-MFMA
  // arithmetic; a tensor that a mixed unit consumes is written as fp16 hi | lo pairs (its MFMAs read the hi half, the
  // residual add both), the map between a mixed block's two convolutions as one fp16
  const int nmix = (sp && !f16 && c->conv_pipelined == 3) ? c->mixed_units : 0;
  auto mixed = [&](int u) { return u >= 0 && u < nmix; };
  auto fmt_for = [&](int consumer_unit) { return mixed(consumer_unit) ? 2 : -1; };
  if (sp) HIPCHK(c, launch_stem_split(img, c->stem.w, c->stem.bias, x.planes(), B, c->stem.Cin, H, W, c->stem.Cout, ACT_RELU, s, f16));
  else HIPCHK(c, launch_stem(img, c->stem.w, c->stem.bias, x.p, B, c->stem.Cin, H, W, c->stem.Cout, ACT_RELU, s));
  // the two 2x2 / stride 2 max-pools (resnet.py:94,106) run inside the epilogue of the convolution in front of them on the
  // split-record path with the 16x16x32 kernels: conv0_2 writes 268 MB instead of 1.07 GB and no pool kernel re-reads it
  const bool fuse_pool = sp && c->conv_pipelined == 3 && !c->no_pool_fusion;
  x = conv(c, s, &err, x, c->conv0_2, 1, 1, 1, 1, ACT_RELU, nullptr, pick(c, {x.p}), nullptr, sp, fuse_pool);
  auto pool = [&](const Act& a, int sh, int sw, int ph, int pw) {
    Act y{pick(c, {a.p}), a.B, (a.H + 2 * ph - 2) / sh + 1, (a.W + 2 * pw - 2) / sw + 1, a.C};
    y.split = a.split;
    y.fmt = a.fmt;
    hipError_t e = a.split ? launch_maxpool_split(a.planes(), y.planes(), a.B, a.H, a.W, a.C, sh, sw, ph, pw, s, f16)
                           : launch_maxpool(a.p, y.p, a.B, a.H, a.W, a.C, sh, sw, ph, pw, s);
    if (e != hipSuccess && err == hipSuccess) err = e;
    return y;
  };
  auto stage = [&](int li) {
    int bi = -1;
    for (const Block& b : c->layers[li]) {
      ++bi;
      // this block's unit and the unit that consumes its output (layer3.4 -> conv3 = unit 4; layer4.2 -> conv4_1: never mixed)
      const int unit = li == 2 ? bi - 1 : li == 3 ? 5 + bi : -1;
      const int next = li == 2 ? bi : li == 3 ? (bi < 2 ? 6 + bi : -1) : -1;
      if (mixed(unit) && !b.has_down) {
        Act t = conv(c, s, &err, x, b.c1, 1, 1, 1, 1, ACT_RELU, nullptr, pick(c, {x.p}), nullptr, sp, false, 1);
        x = conv(c, s, &err, t, b.c2, 1, 1, 1, 1, ACT_RELU, &x, pick(c, {x.p, t.p}), nullptr, sp, false, mixed(next) ? 2 : 0);
        continue;
      }
      Act t = conv(c, s, &err, x, b.c1, 1, 1, 1, 1, ACT_RELU, nullptr, pick(c, {x.p}), nullptr, sp);
      if (b.has_down && b.c2cat.w && sp && c->conv_pipelined == 3 && b.c2.Cout >= 128 && !c->no_shortcut_fusion) {
        // the 1x1 shortcut inside conv2's launch: K-steps over x appended behind the taps over t, one accumulator, no residual
        ConvP ex{};
        ex.in2_hi = x.planes();
        ex.Cin2 = x.C;
        x = conv(c, s, &err, t, b.c2cat, 1, 1, 1, 1, ACT_RELU, nullptr, pick(c, {x.p, t.p}), &ex, sp, false, fmt_for(next));
        continue;
      }
      Act r = x;
      if (b.has_down) r = conv(c, s, &err, x, b.down, 1, 1, 0, 0, ACT_NONE, nullptr, pick(c, {x.p, t.p}), nullptr, sp);
      x = conv(c, s, &err, t, b.c2, 1, 1, 1, 1, ACT_RELU, &r, pick(c, {x.p, t.p, r.p}), nullptr, sp, false, fmt_for(next));
    }
    if (c->cfg.gcb) {  // resnet.py:200-201: GlobalContext closes the stage
      const int HW = x.H * x.W;
      float* ws = c->gc_ws;  // logits [B*HW] | ctx [B][C] | y [B][C]
      hipError_t e = launch_global_context(x.p, c->gc[li], ws, ws + (size_t)x.B * HW, ws + (size_t)x.B * HW + (size_t)x.B * x.C,
                                           x.B, HW, x.C, s);
      if (e != hipSuccess && err == hipSuccess) err = e;
    }
  };
  if (c->cfg.gcb) {
    const int rc = ensure(c, &c->gc_ws, &c->gc_ws_cap, ((size_t)B * (H / 2) * (W / 2) + 2 * (size_t)B * 512 + 64) * 4);
    if (rc) return rc;
  }
  if (!fuse_pool) x = pool(x, 2, 2, 0, 0);
  stage(0);
  const bool fuse_pool2 = fuse_pool && c->conv1.Cout >= 128;  // (the pipelined 16x16x32 kernel takes layers with >= 128 channels)
  x = conv(c, s, &err, x, c->conv1, 1, 1, 1, 1, ACT_RELU, nullptr, pick(c, {x.p}), nullptr, sp, fuse_pool2);
  if (!fuse_pool2) x = pool(x, 2, 2, 0, 0);
  stage(1);
  x = conv(c, s, &err, x, c->conv2, 1, 1, 1, 1, ACT_RELU, nullptr, pick(c, {x.p}), nullptr, sp);
  x = pool(x, 2, 1, 0, 1);
  stage(2);
  x = conv(c, s, &err, x, c->conv3, 1, 1, 1, 1, ACT_RELU, nullptr, pick(c, {x.p}), nullptr, sp, false, mixed(5) ? 2 : x.fmt == 2 ? 0 : -1);
  stage(3);
  x = conv(c, s, &err, x, c->conv4_1, 2, 1, 0, 1, ACT_RELU, nullptr, pick(c, {x.p}), nullptr, sp);
  x = conv(c, s, &err, x, c->conv4_2, 1, 1, 0, 0, ACT_RELU, nullptr, final_out ? final_out : pick(c, {x.p}),
           final_extra, sp && final_split && !final_out);
  if (err != hipSuccess) return fail(c, D2T_EHIP, "backbone launch: %s", hipGetErrorString(err));
  *out = x;
  return D2T_OK;
}

// Position rows a crop with patch grid gh x gw adds to its tokens ([1 + gh*gw][D], row 0 = the cls row): the loaded table,
// or -- ViTEncoder, D2T_VIT_POS_LEARNED_INTERP -- its bicubic resize (vit_encoder.py:58-95), built once per grid
int pos_table_for(d2t_ctx* c, int gh, int gw, hipStream_t s, const float** out) {
  const PosGrid pg = pos_grid(c->cfg, c->pos_GH, c->pos_GW, gh, gw);
  if (!pg.interp) { *out = c->pos_embed; return D2T_OK; }
  const int D = c->cfg.vit_dim;
  d2t_ctx::PosTab& t = c->pos_interp[std::make_pair(gh, gw)];
  if (!t.p) {
    void* p;
    if (int rc = dev_alloc(c, &p, (size_t)(gh * gw + 1) * D * 4)) return rc;
    c->owned.push_back(p);
    t.p = (float*)p;
    t.valid = false;
  }
  if (!t.valid) {
    HIPCHK(c, launch_copy(c->pos_embed, t.p, (size_t)D, s));  // class_pos_embedding is kept (:69,:93-95)
    HIPCHK(c, launch_bicubic_table(c->pos_embed + D, t.p + D, c->pos_GH, c->pos_GW, gh, gw, D, pg.sh, pg.sw, s));
    t.valid = true;
  }
  *out = t.p;
  return D2T_OK;
}

// PositionalEncoding2D crop [h][w][C] (common/postional_encoding.py:105-134,146-157)
int get_pe2d(d2t_ctx* c, int h, int w, int C, hipStream_t s, const float** out) {
  auto key = std::make_pair(h, w);
  auto it = c->pe2d.find(key);
  if (it != c->pe2d.end()) { *out = it->second; return D2T_OK; }
  const int half = C / 2;
  std::vector<float> div(half / 2);
  for (int i = 0; i < half / 2; ++i) div[i] = expf((float)(2 * i) * (float)(-std::log(10000.0) / (double)half));
  std::vector<float> host((size_t)h * w * C);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      float* o = host.data() + ((size_t)y * w + x) * C;
      for (int i = 0; i < half / 2; ++i) {
        o[2 * i] = sinf((float)y * div[i]);
        o[2 * i + 1] = cosf((float)y * div[i]);
        o[half + 2 * i] = sinf((float)x * div[i]);
        o[half + 2 * i + 1] = cosf((float)x * div[i]);
      }
    }
  void* d;
  int rc = dev_alloc(c, &d, host.size() * 4);
  if (rc) return rc;
  HIPCHK(c, hipMemcpy(d, host.data(), host.size() * 4, hipMemcpyHostToDevice));
  c->pe2d[key] = (float*)d;
  *out = (float*)d;
  return D2T_OK;
}

}  // namespace

int d2t_internal_pe2d(d2t_ctx* c, int h, int w, int C, hipStream_t s, const float** out) { return get_pe2d(c, h, w, C, s, out); }
hipError_t d2t_internal_conv_timed(d2t_ctx* c, const ConvP& p, hipStream_t s) { return conv_timed(c, p, s); }

// Process-wide pool of the engine's decode streams.  The first streams a process creates get hardware queues of their own;
// streams created after others were destroyed can end up sharing one (measured: the SECOND context of a process decoded its
// three chains at the rate of ~2.4: 2830 instead of 3810 formulas/s on config C1).  A destroyed context's streams are
// therefore kept and handed, in the same roles, to the next context of that device and priority.
namespace {
std::mutex g_stream_mu;
std::map<std::pair<int, int>, std::vector<hipStream_t>> g_stream_pool;
hipError_t acquire_stream(int device, int prio, hipStream_t* out) {
  {
    std::lock_guard<std::mutex> lk(g_stream_mu);
    auto& v = g_stream_pool[std::make_pair(device, prio)];
    if (!v.empty()) {
      *out = v.back();
      v.pop_back();
      return hipSuccess;
    }
  }
  return hipStreamCreateWithPriority(out, hipStreamNonBlocking, prio);
}
void release_stream(int device, int prio, hipStream_t st) {
  hipStreamSynchronize(st);
  std::lock_guard<std::mutex> lk(g_stream_mu);
  g_stream_pool[std::make_pair(device, prio)].push_back(st);
}
}  // namespace

// ===========================================================================
// C-ABI
// ===========================================================================
extern "C" {

int d2t_device_available(void) {
  int n = 0;
  return hipGetDeviceCount(&n) == hipSuccess && n > 0;
}

int d2t_create(const d2t_config* cfg, d2t_ctx** out) {
  if (!cfg || !out) return D2T_EINVAL;
  *out = nullptr;
  d2t_ctx* c = new d2t_ctx();
  c->cfg = *cfg;
  *out = c;  // returned even on error so that d2t_last_error works; caller destroys it
  if (cfg->in_channels != 1 && cfg->in_channels != 3)
    return fail(c, D2T_EINVAL, "in_channels must be 1 (grey crops) or 3 (rgb crops), got %d", cfg->in_channels);
  if (cfg->backbone_out != 512) return fail(c, D2T_EINVAL, "backbone output_channel must be 512");
  if (cfg->encoder == D2T_ENC_HYBRID_VIT) {
    if (cfg->vit_dim != 256 && cfg->vit_dim != 512) return fail(c, D2T_EINVAL, "ViT hidden_size must be 256 or 512");
    if (cfg->vit_dim / cfg->vit_heads != 32) return fail(c, D2T_EINVAL, "ViT head_dim must be 32");
    if (cfg->patch_h < 1 || cfg->patch_w < 1) return fail(c, D2T_EINVAL, "bad patch size");
  } else if (cfg->encoder != D2T_ENC_RESNET && cfg->encoder != D2T_ENC_VGG_BILSTM &&
             cfg->encoder != D2T_ENC_RESNET_BILSTM) {
    return fail(c, D2T_EINVAL, "unknown encoder %d", cfg->encoder);
  }
  if (cfg->decoder == D2T_DEC_TFM) {
    const int hd = cfg->dec_heads > 0 ? cfg->dec_dim / cfg->dec_heads : 0;
    if (cfg->dec_dim != 256 && cfg->dec_dim != 512) return fail(c, D2T_EINVAL, "decoder d_model must be 256 or 512");
    if (hd != 32 && hd != 64) return fail(c, D2T_EINVAL, "decoder head_dim must be 32 or 64");
    if (cfg->dec_heads != 8) return fail(c, D2T_EINVAL, "decoder nhead must be 8");
    if (cfg->dec_ff % 64) return fail(c, D2T_EINVAL, "dim_feedforward must be a multiple of 64");
    if (cfg->max_seq_len + 2 > 512) return fail(c, D2T_EINVAL, "max_seq_len must be <= 510");
    if (cfg->encoder == D2T_ENC_VGG_BILSTM || cfg->encoder == D2T_ENC_RESNET_BILSTM)
      return fail(c, D2T_EINVAL, "BiLSTM encoders are paired with the Attn decoder only");
  } else if (cfg->decoder == D2T_DEC_ATTN) {
    if (cfg->attn_hidden != 256) return fail(c, D2T_EINVAL, "Attn hidden_size / input_size must be 256");
    if (cfg->attn_kernel_size < 0 || cfg->attn_kernel_size > 5) return fail(c, D2T_EINVAL, "Attn kernel_size must be <= 5");
    if (cfg->vocab > D2T_ATTN_MAX_CLASSES)
      return fail(c, D2T_EINVAL, "Attn decoder supports num_class <= %d, got %d", D2T_ATTN_MAX_CLASSES, cfg->vocab);
    if (cfg->batch_max_length < 1) return fail(c, D2T_EINVAL, "batch_max_length must be >= 1");
    if (cfg->encoder == D2T_ENC_RESNET) return fail(c, D2T_EINVAL, "Feat=ResNet+Seq=None is paired with the TFM decoder only");
    if (cfg->encoder == D2T_ENC_HYBRID_VIT && cfg->vit_dim != 256) return fail(c, D2T_EINVAL, "Attn over ViT needs hidden_size 256");
    if ((cfg->encoder == D2T_ENC_VGG_BILSTM || cfg->encoder == D2T_ENC_RESNET_BILSTM) && cfg->bilstm_hidden != 256)
      return fail(c, D2T_EINVAL, "BiLSTM hidden_size must be 256");
  } else {
    return fail(c, D2T_EINVAL, "unknown decoder %d", cfg->decoder);
  }
  if (!d2t_device_available()) return fail(c, D2T_EHIP, "no HIP device visible");
  HIPCHK(c, hipGetDevice(&c->device));  // the calling thread's current device becomes the context's device
  c->cross_fp32 = D2T_PROBE_ENV("D2T_DECODE_CROSS_FP32") != 0;  // probe builds, A/B: the greedy cross-attention on the fp32 MFMA
  {  // the decode stream carries a latency-bound chain of small kernels: give it the highest priority so its
     // workgroups are placed first whenever the encoder of the next batch is filling the chip
    int lo = 0, hi = 0;
    HIPCHK(c, hipDeviceGetStreamPriorityRange(&lo, &hi));
    c->stream_prio = D2T_PROBE_ENV_STR("D2T_NO_PRIO") ? lo : hi;
    for (int i = 0; i < d2t_ctx::MAXC; ++i) HIPCHK(c, acquire_stream(c->device, c->stream_prio, &c->chains[i].stream));
  }
  HIPCHK(c, hipEventCreateWithFlags(&c->ev_in, hipEventDisableTiming));
  for (int i = 0; i < d2t_ctx::MAXC; ++i) HIPCHK(c, hipEventCreateWithFlags(&c->ev_done[i], hipEventDisableTiming));
  HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&c->h_pinned), 64, hipHostMallocDefault));
  HIPCHK(c, hipMalloc(&c->zero_page, 256));
  HIPCHK(c, hipMemset(c->zero_page, 0, 256));
  return D2T_OK;
}

void d2t_destroy(d2t_ctx* c) {
  DevGuard dg_(c);
  if (!c) return;
  hipDeviceSynchronize();
  d2t_train_release(c);
  for (auto& ge : c->graphs) hipGraphExecDestroy(ge.exec);
  c->graphs.clear();
  free_packed(c);
  for (auto& kv : c->raw) hipFree(kv.second.p);
  for (auto& kv : c->pe2d) hipFree(kv.second);
  for (int i = 0; i < 4; ++i) if (c->act[i]) hipFree(c->act[i]);
  for (int i = 0; i < d2t_ctx::MAXC; ++i) {
    if (c->ckv2[i]) hipFree(c->ckv2[i]);
    if (c->ev_done[i]) hipEventDestroy(c->ev_done[i]);
    if (c->rg_tab[i]) hipFree(c->rg_tab[i]);
    if (c->rg_host[i]) hipHostFree(c->rg_host[i]);
    if (c->rg_ev[i]) hipEventDestroy(c->rg_ev[i]);
  }
  if (c->skv_alt) hipFree(c->skv_alt);
  if (c->beam_ws) hipFree(c->beam_ws);
  if (c->beam_hist) hipFree(c->beam_hist);
  if (c->h_beam) hipHostFree(c->h_beam);
  if (c->beam_qp) hipFree(c->beam_qp);
  if (c->h_pinned) hipHostFree(c->h_pinned);
  if (c->zero_page) hipFree(c->zero_page);
  if (c->gc_ws) hipFree(c->gc_ws);
  if (c->ev_in) hipEventDestroy(c->ev_in);
  if (c->brg_tab) hipFree(c->brg_tab);
  if (c->brg_host) hipHostFree(c->brg_host);
  if (c->h_steps) hipHostFree(c->h_steps);
  for (hipEvent_t ev : c->ticket_ev) if (ev) hipEventDestroy(ev);
  for (d2t_ctx::Chain& o : c->chains) {
    if (o.skv) hipFree(o.skv);
    if (o.dws) hipFree(o.dws);
    if (o.dstate) hipFree(o.dstate);
    if (o.out) hipFree(o.out);
  }
  // the streams go back to the process-wide pool, last acquired first (the next context takes them in the same roles)
  for (int i = d2t_ctx::MAXC - 1; i >= 0; --i)
    if (c->chains[i].stream) release_stream(c->device, c->stream_prio, c->chains[i].stream);
  delete c;
}

const char* d2t_last_error(const d2t_ctx* c) { return c ? c->err.c_str() : "null ctx"; }

int d2t_device_of(const d2t_ctx* c) { return c ? c->device : -1; }

int d2t_load_weight(d2t_ctx* c, const char* name, const float* dev, const int64_t* shape, int32_t ndim,
                    d2t_stream stream) {
  DevGuard dg_(c);
  if (!c || !name || !dev || ndim < 0 || (ndim > 0 && !shape)) return fail(c, D2T_EINVAL, "bad argument");
  if (int rc = check_dev_ptr(c, dev, name)) return rc;
  size_t n = 1;
  std::vector<int64_t> shp(shape, shape + ndim);
  for (auto v : shp) n *= (size_t)v;
  RawW& r = c->raw[name];
  if (r.p && r.numel != n) { hipDeviceSynchronize(); hipFree(r.p); r.p = nullptr; }
  if (!r.p) {
    void* p;
    int rc = dev_alloc(c, &p, n * 4);
    if (rc) return rc;
    r.p = (float*)p;
  }
  r.shape = shp;
  r.numel = n;
  HIPCHK(c, hipMemcpyAsync(r.p, dev, n * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return D2T_OK;
}

int d2t_finalize_weights(d2t_ctx* c, d2t_stream stream) {
  DevGuard dg_(c);
  if (!c) return D2T_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  hipDeviceSynchronize();
  for (auto& ge : c->graphs) hipGraphExecDestroy(ge.exec);
  c->graphs.clear();
  free_packed(c);
  const d2t_config& g = c->cfg;
  int rc;
  const bool vit = g.encoder == D2T_ENC_HYBRID_VIT;
  const std::string sm = "seqmodeler.SequenceModeling.";
  c->bb = vit ? sm + "patch_embed.backbone.ConvNet." : "featextractor.FeatureExtraction.ConvNet.";
  const std::string& bb = c->bb;
  const bool is_vgg = g.encoder == D2T_ENC_VGG_BILSTM;
  const bool has_lstm = is_vgg || g.encoder == D2T_ENC_RESNET_BILSTM;
  if (is_vgg) {
    // VGG_FeatureExtractor (feature_extractor/vgg.py:16-41): nn.Sequential indices of the convs / BNs
    const char* convs[7] = {"0", "3", "6", "8", "11", "14", "18"};
    const char* bns[7] = {"", "", "", "", "12", "15", ""};
    for (int i = 0; i < 7; ++i)
      if ((rc = pack_conv(c, bb + convs[i], bns[i][0] ? bb + bns[i] : std::string(), &c->vgg[i], s))) return rc;
    if (c->vgg[0].Cin != g.in_channels || c->vgg[0].KH != 3 || c->vgg[0].KW != 3 || c->vgg[6].KH != 2 || c->vgg[6].Cout != 512)
      return fail(c, D2T_EINVAL, "unexpected VGG_FeatureExtractor shapes");
  }
  if (!is_vgg) {
  if ((rc = pack_conv(c, bb + "conv0_1", bb + "bn0_1", &c->stem, s))) return rc;
  if (c->stem.Cin != g.in_channels || c->stem.KH != 3 || c->stem.KW != 3)
    return fail(c, D2T_EINVAL, "conv0_1 must be %d-channel 3x3 (the config's in_channels), got %d channels %dx%d", g.in_channels,
                c->stem.Cin, c->stem.KH, c->stem.KW);
  if ((rc = pack_conv(c, bb + "conv0_2", bb + "bn0_2", &c->conv0_2, s))) return rc;
  for (int li = 0; li < 4; ++li) {
    for (int bi = 0; bi < RESNET_LAYERS[li]; ++bi) {
      const std::string p = bb + "layer" + std::to_string(li + 1) + "." + std::to_string(bi);
      Block b;
      if ((rc = pack_conv(c, p + ".conv1", p + ".bn1", &b.c1, s))) return rc;
      if ((rc = pack_conv(c, p + ".conv2", p + ".bn2", &b.c2, s))) return rc;
      if (find(c, p + ".downsample.0.weight")) {
        b.has_down = true;
        if ((rc = pack_conv(c, p + ".downsample.0", p + ".downsample.1", &b.down, s))) return rc;
        if (b.c2.w_hi && b.down.w_hi && b.down.KH == 1 && b.down.KW == 1 && b.down.Cout == b.c2.Cout) {
          // conv2 | shortcut concatenated along K (both already folded and in the kernels' K order: a 1x1 layer's is plain)
          const int Co = b.c2.Cout, K2 = b.c2.KH * b.c2.KW * b.c2.Cin, Kd = b.down.Cin;
          void* bufs[4] = {nullptr, nullptr, nullptr, nullptr};
          const size_t n = (size_t)Co * (K2 + Kd);
          const size_t bytes[4] = {n * 4, (size_t)Co * 4, n * 2, n * 2};
          for (int q = 0; q < 4; ++q) {  // (each buffer is owned as soon as it exists: nothing leaks when a later one fails)
            if ((rc = dev_alloc(c, &bufs[q], bytes[q]))) return rc;
            c->owned.push_back(bufs[q]);
          }
          void *pw = bufs[0], *pb = bufs[1], *ph = bufs[2], *pl = bufs[3];
          b.c2cat = b.c2;
          b.c2cat.w = (float*)pw; b.c2cat.bias = (float*)pb; b.c2cat.w_hi = (uint16_t*)ph; b.c2cat.w_lo = (uint16_t*)pl;
          b.c2cat.w_h16 = b.c2cat.w_l16 = nullptr; b.c2cat.K2 = Kd;  // (K2: the K rows of the second, 1x1 input)
          HIPCHK(c, hipMemcpy2DAsync(pw, (size_t)(K2 + Kd) * 4, b.c2.w, (size_t)K2 * 4, (size_t)K2 * 4, Co, hipMemcpyDeviceToDevice, s));
          HIPCHK(c, hipMemcpy2DAsync((float*)pw + K2, (size_t)(K2 + Kd) * 4, b.down.w, (size_t)Kd * 4, (size_t)Kd * 4, Co,
                                     hipMemcpyDeviceToDevice, s));
          HIPCHK(c, launch_add_rows(b.c2.bias, b.down.bias, b.c2cat.bias, Co, s));
          HIPCHK(c, launch_split_bf16(b.c2cat.w, b.c2cat.w_hi, b.c2cat.w_lo, n, s));
        } else {
          b.c2cat.w = nullptr;
        }
      }
      c->layers[li].push_back(b);
    }
    if (c->cfg.gcb) {  // GlobalContext(planes) appended to the stage (visual_attention.py:105-165)
      const std::string p = bb + "layer" + std::to_string(li + 1) + "." + std::to_string(RESNET_LAYERS[li]) + ".";
      const int C = c->layers[li].back().c2.Cout;
      const RawW *wg, *bg, *w1, *b1, *lg, *lb, *w2, *b2;
      if ((rc = need(c, p + "global_cxt.weight", &wg, {1, C, 1, 1})) || (rc = need(c, p + "global_cxt.bias", &bg, {1})) ||
          (rc = need(c, p + "bottleneck_add.fc1.weight", &w1, {C, C, 1, 1})) ||
          (rc = need(c, p + "bottleneck_add.fc1.bias", &b1, {C})) ||
          (rc = need(c, p + "bottleneck_add.norm.weight", &lg, {C})) || (rc = need(c, p + "bottleneck_add.norm.bias", &lb, {C})) ||
          (rc = need(c, p + "bottleneck_add.fc2.weight", &w2, {C, C, 1, 1})) ||
          (rc = need(c, p + "bottleneck_add.fc2.bias", &b2, {C})))
        return rc;
      c->gc[li] = GCParams{wg->p, bg->p, w1->p, b1->p, lg->p, lb->p, w2->p, b2->p};
    }
  }
  if ((rc = pack_conv(c, bb + "conv1", bb + "bn1", &c->conv1, s))) return rc;
  if ((rc = pack_conv(c, bb + "conv2", bb + "bn2", &c->conv2, s))) return rc;
  if ((rc = pack_conv(c, bb + "conv3", bb + "bn3", &c->conv3, s))) return rc;
  if ((rc = pack_conv(c, bb + "conv4_1", bb + "bn4_1", &c->conv4_1, s))) return rc;
  if ((rc = pack_conv(c, bb + "conv4_2", bb + "bn4_2", &c->conv4_2, s))) return rc;
  }  // !is_vgg

  if (has_lstm) {
    // 2x BidirectionalLSTM (seq_modeling/bilstm.py:6-24, build_seq.py:20-23): nn.LSTM(bidirectional) + Linear
    const int Hh = g.bilstm_hidden, G4 = 4 * Hh;
    int in = 512;
    for (int i = 0; i < 2; ++i) {
      const std::string lp = sm + std::to_string(i) + ".";
      BiLstmW& L = c->lstm[i];
      L.in = in;
      void *a, *b2, *t;
      if ((rc = dev_alloc(c, &a, (size_t)2 * G4 * in * 4)) || (rc = dev_alloc(c, &b2, (size_t)2 * G4 * 4)) ||
          (rc = dev_alloc(c, &t, (size_t)2 * Hh * G4 * 4)))
        return rc;
      c->owned.push_back(a); c->owned.push_back(b2); c->owned.push_back(t);
      L.wih_cat = (float*)a; L.bias_cat = (float*)b2; L.whh_t = (float*)t;
      const char* sfx[2] = {"", "_reverse"};
      for (int dirn = 0; dirn < 2; ++dirn) {
        const RawW *wi, *wh, *bi, *bh;
        if ((rc = need(c, lp + "rnn.weight_ih_l0" + sfx[dirn], &wi, {G4, in})) ||
            (rc = need(c, lp + "rnn.weight_hh_l0" + sfx[dirn], &wh, {G4, Hh})) ||
            (rc = need(c, lp + "rnn.bias_ih_l0" + sfx[dirn], &bi, {G4})) ||
            (rc = need(c, lp + "rnn.bias_hh_l0" + sfx[dirn], &bh, {G4})))
          return rc;
        HIPCHK(c, launch_copy(wi->p, L.wih_cat + (size_t)dirn * G4 * in, (size_t)G4 * in, s));
        HIPCHK(c, launch_add_rows(bi->p, bh->p, L.bias_cat + (size_t)dirn * G4, G4, s));
        HIPCHK(c, launch_transpose_into(wh->p, G4, Hh, L.whh_t + (size_t)dirn * Hh * G4, G4, 0, s));
      }
      if ((rc = get_lin(c, lp + "linear", &L.lin, Hh, 2 * Hh))) return rc;
      in = Hh;
    }
  }

  if (vit) {
    const int D = g.vit_dim;
    if ((rc = pack_conv(c, sm + "patch_embed.proj", "", &c->patch, s))) return rc;
    if (c->patch.Cout != D || c->patch.KH != g.patch_h || c->patch.KW != g.patch_w)
      return fail(c, D2T_EINVAL, "patch_embed.proj shape does not match the config");
    const RawW *pos, *cls;
    if ((rc = need(c, sm + "pos_embed", &pos)) || (rc = need(c, sm + "cls_token", &cls, {1, 1, D}))) return rc;
    if (pos->shape.size() != 3 || pos->shape[2] != D) return fail(c, D2T_EINVAL, "pos_embed must be [1,N,%d]", D);
    c->pos_embed = pos->p;
    c->pos_rows = (int)pos->shape[1];
    if (g.vit_pos < D2T_VIT_POS_SINCOS_PREFIX || g.vit_pos > D2T_VIT_POS_LEARNED_PREFIX) return fail(c, D2T_EINVAL, "vit_pos %d", g.vit_pos);
    if (d2t_encoder_shape(c, g.max_h, g.max_w, nullptr, nullptr, &c->pos_GH, &c->pos_GW, nullptr, nullptr))
      return fail(c, D2T_EINVAL, "max_dimension %dx%d leaves no backbone output", g.max_h, g.max_w);
    if (c->pos_rows != c->pos_GH * c->pos_GW + 1)
      return fail(c, D2T_EINVAL, "pos_embed has %d rows, max_dimension %dx%d gives a %dx%d patch grid", c->pos_rows, g.max_h,
                  g.max_w, c->pos_GH, c->pos_GW);
    void* p;
    if ((rc = dev_alloc(c, &p, (size_t)D * 4))) return rc;
    c->owned.push_back(p);
    c->cls_row = (float*)p;
    HIPCHK(c, launch_add_rows(cls->p, pos->p, c->cls_row, D, s));
    for (int i = 0; i < g.vit_depth; ++i) {
      const std::string b = sm + "blocks." + std::to_string(i) + ".";
      VitBlock vb;
      if ((rc = get_ln(c, b + "norm1", &vb.n1, D)) || (rc = get_ln(c, b + "norm2", &vb.n2, D)) ||
          (rc = get_lin(c, b + "attn.qkv", &vb.qkv, 3 * D, D)) || (rc = get_lin(c, b + "attn.proj", &vb.proj, D, D)))
        return rc;
      const RawW* f1;
      if ((rc = need(c, b + "mlp.fc1.weight", &f1))) return rc;
      const int hid = (int)f1->shape[0];
      if ((rc = get_lin(c, b + "mlp.fc1", &vb.fc1, hid, D)) || (rc = get_lin(c, b + "mlp.fc2", &vb.fc2, D, hid)))
        return rc;
      if ((rc = split_lin(c, &vb.qkv, s)) || (rc = split_lin(c, &vb.proj, s)) || (rc = split_lin(c, &vb.fc1, s)) ||
          (rc = split_lin(c, &vb.fc2, s)))
        return rc;
      c->vit.push_back(vb);
    }
    if ((rc = get_ln(c, sm + "norm", &c->vit_norm, D))) return rc;
    if (g.decoder == D2T_DEC_TFM && g.dec_dim != D)
      return fail(c, D2T_EINVAL, "decoder d_model must equal the ViT hidden_size");
  } else if (g.decoder == D2T_DEC_TFM && g.dec_dim != c->conv4_2.Cout) {
    return fail(c, D2T_EINVAL, "decoder d_model must equal the backbone output_channel");
  }

  const std::string pp = "predicter.Prediction.";
  if (g.decoder == D2T_DEC_ATTN) {
    // Attention.__init__ (prediction_head/seq2seq.py:11-68) + LocationAwareAttention (attention1D.py:121-133,203-214)
    const int Hh = g.attn_hidden, V = g.vocab, taps = 2 * g.attn_kernel_size + 1, kd = g.attn_kernel_dim;
    const std::string ac = pp + "attention_cell.";
    AttnW& A = c->attn;
    A = AttnW{};
    A.taps = taps;
    const RawW *emb = nullptr, *lcw = nullptr, *lcb = nullptr, *lpw = nullptr, *lpb = nullptr, *qw, *qb, *sw, *sb = nullptr,
               *wih, *whh, *bih, *bhh, *gw, *gb;
    const bool bahdanau = g.attn_cell == D2T_ATTN_CELL_BAHDANAU, onehot = g.attn_onehot != 0;
    const int Ein = onehot ? V : Hh;  // width of the decoder-input part of rnn.weight_ih
    if (!onehot && (rc = need(c, pp + "embedding.weight", &emb, {V, Hh}))) return rc;
    if (bahdanau) {  // BahdanauAttentionCell (attention1D.py:71-85): i2h without bias, h2h, score without bias
      if ((rc = need(c, ac + "attn.h2h.weight", &qw, {Hh, Hh})) || (rc = need(c, ac + "attn.h2h.bias", &qb, {Hh})) ||
          (rc = get_lin(c, ac + "attn.i2h", &A.key, Hh, Hh, /*bias=*/false)) ||
          (rc = need(c, ac + "attn.score.weight", &sw, {1, Hh})))
        return rc;
    } else if ((rc = need(c, ac + "attn.loc_conv.weight", &lcw, {kd, 1, taps})) ||
               (rc = need(c, ac + "attn.loc_conv.bias", &lcb, {kd})) ||
               (rc = need(c, ac + "attn.loc_proj.weight", &lpw, {Hh, kd})) ||
               (rc = need(c, ac + "attn.loc_proj.bias", &lpb, {Hh})) ||
               (rc = need(c, ac + "attn.query_proj.weight", &qw, {Hh, Hh})) ||
               (rc = need(c, ac + "attn.query_proj.bias", &qb, {Hh})) ||
               (rc = get_lin(c, ac + "attn.key_proj", &A.key, Hh, Hh)) ||
               (rc = need(c, ac + "attn.score.weight", &sw, {1, Hh})) || (rc = need(c, ac + "attn.score.bias", &sb, {1}))) {
      return rc;
    }
    if ((rc = need(c, ac + "rnn.weight_ih", &wih, {4 * Hh, Hh + Ein})) ||
        (rc = need(c, ac + "rnn.weight_hh", &whh, {4 * Hh, Hh})) || (rc = need(c, ac + "rnn.bias_ih", &bih, {4 * Hh})) ||
        (rc = need(c, ac + "rnn.bias_hh", &bhh, {4 * Hh})) || (rc = need(c, ac + "generator.weight", &gw, {V, Hh})) ||
        (rc = need(c, ac + "generator.bias", &gb, {V})))
      return rc;
    A.emb = emb ? emb->p : nullptr; A.bq = qb->p; A.wscore = sw->p; A.bg = gb->p;
    auto alloc = [&](float** dst, size_t n) -> int {
      void* q;
      int r2 = dev_alloc(c, &q, n * 4);
      if (r2) return r2;
      c->owned.push_back(q);
      *dst = (float*)q;
      return D2T_OK;
    };
    if ((rc = alloc(&A.wq_t, (size_t)Hh * Hh)) || (rc = alloc(&A.wloc, (size_t)Hh * taps)) ||
        (rc = alloc(&A.bloc, Hh)) || (rc = alloc(&A.wx_t, (size_t)3 * Hh * 4 * Hh)) || (rc = alloc(&A.bx, 4 * Hh)) ||
        (rc = alloc(&A.wg_t, (size_t)Hh * V)))
      return rc;
    HIPCHK(c, launch_transpose_into(qw->p, Hh, Hh, A.wq_t, Hh, 0, s));
    if (!onehot) {
      HIPCHK(c, launch_transpose_into(wih->p, 4 * Hh, 2 * Hh, A.wx_t, 4 * Hh, 0, s));       // rows [ctx ; emb]
    } else {
      // one-hot decoder input (seq2seq.py:72-78): W_ih . [ctx ; onehot(tok)] = W_ih[:, :H] . ctx + W_ih[:, H + tok]; the
      // kernel keeps its [ctx ; emb ; h] layout with zero "emb" rows and adds row `tok` of the transposed tail of W_ih
      float* full;  // W_ih^T [H + V][4H]
      if ((rc = alloc(&full, (size_t)(Hh + V) * 4 * Hh))) return rc;
      HIPCHK(c, launch_transpose_into(wih->p, 4 * Hh, Hh + V, full, 4 * Hh, 0, s));
      HIPCHK(c, hipMemcpyAsync(A.wx_t, full, (size_t)Hh * 4 * Hh * 4, hipMemcpyDeviceToDevice, s));
      HIPCHK(c, hipMemsetAsync(A.wx_t + (size_t)Hh * 4 * Hh, 0, (size_t)Hh * 4 * Hh * 4, s));
      A.tokgate = full + (size_t)Hh * 4 * Hh;
    }
    HIPCHK(c, launch_transpose_into(whh->p, 4 * Hh, Hh, A.wx_t, 4 * Hh, 2 * Hh, s));      // rows h
    HIPCHK(c, launch_add_rows(bih->p, bhh->p, A.bx, 4 * Hh, s));
    HIPCHK(c, launch_transpose_into(gw->p, V, Hh, A.wg_t, V, 0, s));
    if (bahdanau) {  // no location term, no score bias: a zero one-tap filter
      HIPCHK(c, hipMemsetAsync(A.wloc, 0, (size_t)Hh * taps * 4, s));
      HIPCHK(c, hipMemsetAsync(A.bloc, 0, (size_t)Hh * 4, s));
      A.bscore = 0.f;
    } else {  // fold loc_proj o loc_conv (attention1D.py:150-152) into one [H][taps] filter on the host
      std::vector<float> hcw((size_t)kd * taps), hcb(kd), hpw((size_t)Hh * kd), hpb(Hh), hsb(1);
      HIPCHK(c, hipStreamSynchronize(s));
      HIPCHK(c, hipMemcpy(hcw.data(), lcw->p, hcw.size() * 4, hipMemcpyDeviceToHost));
      HIPCHK(c, hipMemcpy(hcb.data(), lcb->p, hcb.size() * 4, hipMemcpyDeviceToHost));
      HIPCHK(c, hipMemcpy(hpw.data(), lpw->p, hpw.size() * 4, hipMemcpyDeviceToHost));
      HIPCHK(c, hipMemcpy(hpb.data(), lpb->p, hpb.size() * 4, hipMemcpyDeviceToHost));
      HIPCHK(c, hipMemcpy(hsb.data(), sb->p, 4, hipMemcpyDeviceToHost));
      std::vector<float> w((size_t)Hh * taps), b(Hh);
      for (int n = 0; n < Hh; ++n) {
        double bb2 = hpb[n];
        for (int m = 0; m < kd; ++m) bb2 += (double)hpw[(size_t)n * kd + m] * hcb[m];
        b[n] = (float)bb2;
        for (int j = 0; j < taps; ++j) {
          double a = 0.0;
          for (int m = 0; m < kd; ++m) a += (double)hpw[(size_t)n * kd + m] * hcw[(size_t)m * taps + j];
          w[(size_t)n * taps + j] = (float)a;
        }
      }
      HIPCHK(c, hipMemcpy(A.wloc, w.data(), w.size() * 4, hipMemcpyHostToDevice));
      HIPCHK(c, hipMemcpy(A.bloc, b.data(), b.size() * 4, hipMemcpyHostToDevice));
      A.bscore = hsb[0];
    }
    if (g.attn_enc_init) {
      const RawW *hw, *hb, *cw, *cb;
      if ((rc = need(c, pp + "proj_init_h.weight", &hw, {Hh, Hh})) || (rc = need(c, pp + "proj_init_h.bias", &hb, {Hh})) ||
          (rc = need(c, pp + "proj_init_c.weight", &cw, {Hh, Hh})) || (rc = need(c, pp + "proj_init_c.bias", &cb, {Hh})))
        return rc;
      if ((rc = alloc(&A.wih_t, (size_t)Hh * Hh)) || (rc = alloc(&A.wic_t, (size_t)Hh * Hh))) return rc;
      HIPCHK(c, launch_transpose_into(hw->p, Hh, Hh, A.wih_t, Hh, 0, s));
      HIPCHK(c, launch_transpose_into(cw->p, Hh, Hh, A.wic_t, Hh, 0, s));
      A.bih = hb->p; A.bic = cb->p;
    }
    HIPCHK(c, hipStreamSynchronize(s));
    c->finalized = true;
    return D2T_OK;
  }

  // decoder (prediction_head/tfm.py:36-72)
  const int d = g.dec_dim, V = g.vocab;
  const RawW *we, *pe;
  if ((rc = need(c, pp + "word_embed.weight", &we, {V, d})) || (rc = need(c, pp + "pos_enc.pe", &pe))) return rc;
  if (pe->shape.size() != 2 || pe->shape[1] != d || pe->shape[0] < g.max_seq_len + 2)
    return fail(c, D2T_EINVAL, "pos_enc.pe must be [>=%d,%d]", g.max_seq_len + 2, d);
  c->word_embed = we->p;
  c->word_pe = pe->p;
  c->word_pe_rows = (int)pe->shape[0];
  void *kw, *kb;
  if ((rc = dev_alloc(c, &kw, (size_t)g.dec_layers * 2 * d * d * 4)) ||
      (rc = dev_alloc(c, &kb, (size_t)g.dec_layers * 2 * d * 4)))
    return rc;
  c->owned.push_back(kw);
  c->owned.push_back(kb);
  c->ckv_w = (float*)kw;
  c->ckv_b = (float*)kb;
  for (int i = 0; i < g.dec_layers; ++i) {
    const std::string l = pp + "model.layers." + std::to_string(i) + ".";
    DecLayer dl;
    const RawW *siw, *sib, *ciw, *cib;
    if ((rc = need(c, l + "self_attn.in_proj_weight", &siw, {3 * d, d})) ||
        (rc = need(c, l + "self_attn.in_proj_bias", &sib, {3 * d})) ||
        (rc = need(c, l + "multihead_attn.in_proj_weight", &ciw, {3 * d, d})) ||
        (rc = need(c, l + "multihead_attn.in_proj_bias", &cib, {3 * d})))
      return rc;
    dl.sa_in = LinW{siw->p, sib->p, 3 * d, d};
    dl.ca_q = LinW{ciw->p, cib->p, d, d};
    HIPCHK(c, launch_copy(ciw->p + (size_t)d * d, c->ckv_w + (size_t)i * 2 * d * d, (size_t)2 * d * d, s));
    HIPCHK(c, launch_copy(cib->p + d, c->ckv_b + (size_t)i * 2 * d, (size_t)2 * d, s));
    if ((rc = get_lin(c, l + "self_attn.out_proj", &dl.sa_out, d, d)) ||
        (rc = get_lin(c, l + "multihead_attn.out_proj", &dl.ca_out, d, d)) ||
        (rc = get_lin(c, l + "linear1", &dl.l1, g.dec_ff, d)) || (rc = get_lin(c, l + "linear2", &dl.l2, d, g.dec_ff)) ||
        (rc = get_ln(c, l + "norm1", &dl.n1, d)) || (rc = get_ln(c, l + "norm2", &dl.n2, d)) ||
        (rc = get_ln(c, l + "norm3", &dl.n3, d)))
      return rc;
    for (auto pr : {std::make_pair(&dl.sa_out_t, dl.sa_out.w), std::make_pair(&dl.ca_q_t, dl.ca_q.w),
                    std::make_pair(&dl.ca_out_t, dl.ca_out.w)}) {
      void* tp;
      if ((rc = dev_alloc(c, &tp, (size_t)d * d * 4))) return rc;
      c->owned.push_back(tp);
      *pr.first = (float*)tp;
      HIPCHK(c, launch_transpose(pr.second, *pr.first, d, d, s));
    }
    {  // absorbed cross-attention: W_k as stored, W_v transposed (read from the engine's stacked copy), b_v
      void* tp;
      if ((rc = dev_alloc(c, &tp, (size_t)d * d * 4))) return rc;
      c->owned.push_back(tp);
      dl.ca_v_t = (float*)tp;
      dl.ca_wk = c->ckv_w + (size_t)i * 2 * d * d;
      dl.ca_bv = c->ckv_b + (size_t)i * 2 * d + d;
      HIPCHK(c, launch_transpose(c->ckv_w + (size_t)i * 2 * d * d + (size_t)d * d, dl.ca_v_t, d, d, s));
    }
    c->dec.push_back(dl);
  }
  if ((rc = get_lin(c, pp + "proj", &c->out_proj, V, d))) return rc;
  {  // bf16 split of the stacked cross-attention K/V projection (one large-M GEMM per batch)
    const uint16_t *hi = nullptr, *lo = nullptr;
    if (d % 32 == 0 && (rc = split_planes(c, c->ckv_w, (size_t)g.dec_layers * 2 * d * d, &hi, &lo, s))) return rc;
    c->ckv_hi = const_cast<uint16_t*>(hi);
    c->ckv_lo = const_cast<uint16_t*>(lo);
  }
  c->dec_absorbed = d == 256 && g.dec_heads == 8 && !D2T_PROBE_ENV_STR("D2T_DECODE_PROJECTED_KV");
  HIPCHK(c, hipStreamSynchronize(s));
  c->finalized = true;
  return D2T_OK;
}

int d2t_encoder_shape(const d2t_ctx* c, int32_t H, int32_t W, int32_t* T, int32_t* d, int32_t* grid_h,
                      int32_t* grid_w, int32_t* pad_w, int32_t* pad_h) {
  if (!c) return D2T_EINVAL;
  if (H < 4 || W < 4) return D2T_EINVAL;
  int fh, fw;
  if (c->cfg.encoder == D2T_ENC_VGG_BILSTM) {  // vgg.py:16-41: pools (2,2),(2,2),(2,1),(2,1), final 2x2 conv
    fh = H / 2 / 2 / 2 / 2 - 1;
    fw = W / 2 / 2 - 1;
  } else {
    backbone_hw(H, W, &fh, &fw);
  }
  if (fh < 1 || fw < 1) return D2T_EINVAL;
  int gh = fh, gw = fw, pw = 0, ph = 0, t, dim = c->cfg.backbone_out;
  if (c->cfg.encoder == D2T_ENC_VGG_BILSTM || c->cfg.encoder == D2T_ENC_RESNET_BILSTM) {
    t = fw;  // the height is averaged away (build_feat.py:50-55)
    dim = c->cfg.bilstm_hidden;
  } else if (c->cfg.encoder == D2T_ENC_HYBRID_VIT) {
    ph = (c->cfg.patch_h - fh % c->cfg.patch_h) % c->cfg.patch_h;
    pw = (c->cfg.patch_w - fw % c->cfg.patch_w) % c->cfg.patch_w;
    gh = (fh + ph) / c->cfg.patch_h;
    gw = (fw + pw) / c->cfg.patch_w;
    t = gh * gw + 1;
    dim = c->cfg.vit_dim;
  } else {
    t = fh * fw;
  }
  if (T) *T = t;
  if (d) *d = dim;
  if (grid_h) *grid_h = gh;
  if (grid_w) *grid_w = gw;
  if (pad_w) *pad_w = pw;
  if (pad_h) *pad_h = ph;
  return D2T_OK;
}

int d2t_encode(d2t_ctx* c, const float* image, int32_t B, int32_t H, int32_t W, float* memory, d2t_stream stream) {
  return d2t_encode_attn(c, image, B, H, W, memory, nullptr, 0, stream);
}

int d2t_encode_attn(d2t_ctx* c, const float* image, int32_t B, int32_t H, int32_t W, float* memory, float* const* maps_dev,
                    int32_t n_maps, d2t_stream stream) {
  DevGuard dg_(c);
  if (!c || !image || !memory || B < 1) return fail(c, D2T_EINVAL, "bad argument");
  if (!c->finalized) return fail(c, D2T_ESTATE, "weights not finalized");
  if (int rc = check_dev_ptr(c, image, "image")) return rc;
  if (int rc = check_dev_ptr(c, memory, "memory")) return rc;
  hipStream_t s = (hipStream_t)stream;
  const d2t_config& g = c->cfg;
  if (n_maps < 0 || (n_maps > 0 && !maps_dev)) return fail(c, D2T_EINVAL, "bad attention-map list (%d entries)", n_maps);
  for (int i = 0; i < n_maps; ++i) {
    if (!maps_dev[i]) continue;
    if (g.encoder != D2T_ENC_HYBRID_VIT) return fail(c, D2T_EINVAL, "attention maps need the ViT encoder (this one has no self-attention)");
    if (int rc = check_dev_ptr(c, maps_dev[i], "attention map")) return rc;
  }
  if (g.encoder == D2T_ENC_HYBRID_VIT && n_maps > 0 && n_maps != (int)c->vit.size())
    return fail(c, D2T_EINVAL, "%d attention maps for a ViT of depth %d (pass 0 or one per block)", n_maps, (int)c->vit.size());
  int T, dim, gh, gw, pw, ph;
  if (d2t_encoder_shape(c, H, W, &T, &dim, &gh, &gw, &pw, &ph))
    return fail(c, D2T_EINVAL, "unsupported crop %dx%d (backbone output would be empty)", H, W);
  const bool vit = g.encoder == D2T_ENC_HYBRID_VIT;
  if (vit && g.vit_pos != D2T_VIT_POS_LEARNED_INTERP && T > c->pos_rows)  // the prefix slice would run off the table
    return fail(c, D2T_EINVAL, "crop %dx%d exceeds max_dimension (pos_embed rows %d)", H, W, c->pos_rows);
  if (T > memory_cap(c)) return fail(c, D2T_EINVAL, "memory length %d > %d unsupported", T, memory_cap(c));
  // largest activation: conv0_2 output B*H*W*64 floats; ViT needs B*T*max(3*dim, hidden)
  size_t need_floats = (size_t)B * H * W * 64;
  if (vit) {
    size_t hid = c->vit.empty() ? 0 : (size_t)c->vit[0].fc1.N;
    size_t v = (size_t)B * T * (hid > 3 * (size_t)dim ? hid : 3 * (size_t)dim);
    if (v > need_floats) need_floats = v;
  }
  const bool lstm_enc = g.encoder == D2T_ENC_VGG_BILSTM || g.encoder == D2T_ENC_RESNET_BILSTM;
  if (lstm_enc && (size_t)B * T * 8 * g.bilstm_hidden > need_floats) need_floats = (size_t)B * T * 8 * g.bilstm_hidden;
  if (c->act_cap < need_floats * 4) {
    hipDeviceSynchronize();
    for (int i = 0; i < 4; ++i) {
      if (c->act[i]) hipFree(c->act[i]);
      c->act[i] = nullptr;
      void* p;
      int rc = dev_alloc(c, &p, need_floats * 4);
      if (rc) { c->act_cap = 0; return rc; }
      c->act[i] = (float*)p;
    }
    c->act_cap = need_floats * 4;
  }
  Act f{};
  int rc;
  if (lstm_enc) {
    hipError_t err = hipSuccess;
    if (g.encoder == D2T_ENC_VGG_BILSTM) {
      // VGG_FeatureExtractor.forward (feature_extractor/vgg.py:16-44)
      Act x{pick(c, {}), B, H, W, c->vgg[0].Cout};
      HIPCHK(c, launch_stem(image, c->vgg[0].w, c->vgg[0].bias, x.p, B, c->vgg[0].Cin, H, W, x.C, ACT_RELU, s));
      auto pool = [&](const Act& a, int kh, int kw) {
        Act y{pick(c, {a.p}), a.B, (a.H - kh) / kh + 1, (a.W - kw) / kw + 1, a.C};
        hipError_t e = launch_maxpool_k(a.p, y.p, a.B, a.H, a.W, a.C, kh, kw, kh, kw, 0, 0, s);
        if (e != hipSuccess && err == hipSuccess) err = e;
        return y;
      };
      x = pool(x, 2, 2);
      x = conv(c, s, &err, x, c->vgg[1], 1, 1, 1, 1, ACT_RELU, nullptr, pick(c, {x.p}));
      x = pool(x, 2, 2);
      x = conv(c, s, &err, x, c->vgg[2], 1, 1, 1, 1, ACT_RELU, nullptr, pick(c, {x.p}));
      x = conv(c, s, &err, x, c->vgg[3], 1, 1, 1, 1, ACT_RELU, nullptr, pick(c, {x.p}));
      x = pool(x, 2, 1);
      x = conv(c, s, &err, x, c->vgg[4], 1, 1, 1, 1, ACT_RELU, nullptr, pick(c, {x.p}));
      x = conv(c, s, &err, x, c->vgg[5], 1, 1, 1, 1, ACT_RELU, nullptr, pick(c, {x.p}));
      x = pool(x, 2, 1);
      f = conv(c, s, &err, x, c->vgg[6], 1, 1, 0, 0, ACT_RELU, nullptr, pick(c, {x.p}));
      if (err != hipSuccess) return fail(c, D2T_EHIP, "VGG launch: %s", hipGetErrorString(err));
    } else if ((rc = run_backbone(c, s, image, B, H, W, &f, nullptr, nullptr, false))) {
      return rc;
    }
    if (f.W != T || f.C != 512) return fail(c, D2T_EINVAL, "unexpected feature map %dx%dx%d", f.H, f.W, f.C);
    // AdaptiveAvgPool2d((None,1)) over the height (build_feat.py:50-55), then 2x BidirectionalLSTM
    float* seq = pick(c, {f.p});
    HIPCHK(c, launch_mean_h(f.p, seq, B, f.H, f.W, f.C, s));
    const int Hh = g.bilstm_hidden;
    for (int i = 0; i < 2; ++i) {
      const BiLstmW& L = c->lstm[i];
      float* gates = pick(c, {seq});
      float* rec = pick(c, {seq, gates});
      LinW ih{L.wih_cat, L.bias_cat, 8 * Hh, L.in};
      HIPCHK(c, linear_any(c, s, seq, ih, nullptr, gates, B * T, ACT_NONE));
      HIPCHK(c, launch_bilstm(gates, L.whh_t, rec, B, T, Hh, s));
      float* out = i == 1 ? memory : pick(c, {rec});
      HIPCHK(c, linear_any(c, s, rec, L.lin, nullptr, out, B * T, ACT_NONE));
      seq = out;
    }
    return D2T_OK;
  }
  if (!vit) {
    // Feat=ResNet, Seq=None: PositionalEncoding2D add, [B,C,H,W] -> [B,HW,C] (build_seq.py:69-76)
    int fh, fw;
    backbone_hw(H, W, &fh, &fw);
    const float* pe;
    if ((rc = get_pe2d(c, fh, fw, g.backbone_out, s, &pe))) return rc;
    ConvP ex{};
    ex.row_add = pe; ex.rows_per_img = fh * fw; ex.img_stride = fh * fw; ex.row_off = 0; ex.row_add_off = 0;
    return run_backbone(c, s, image, B, H, W, &f, memory, &ex, false);
  }
  if ((rc = run_backbone(c, s, image, B, H, W, &f, nullptr, nullptr, true))) return rc;
  // HybridEmbed.forward (patchembed.py:115-141): zero-pad right/bottom + Conv2d(k=s=patch) as one
  // implicit GEMM whose out-of-range taps read zero; epilogue adds pos_embed[1+i] (flat prefix
  // slice, vit_encoder.py:260) and leaves row 0 of every image for the cls token.
  hipError_t err = hipSuccess;
  float* X = pick(c, {f.p});
  {
    Act y{X, f.B, gh, gw, dim};
    ConvP p{};
    p.w = c->patch.w; p.bias = c->patch.bias; p.out = X;
    if (c->conv_bf16x3) { p.w_hi = c->patch.w_hi; p.w_lo = c->patch.w_lo; }
    if (f.split) p.in_hi = f.planes(); else p.in = f.p;
    if ((rc = conv_route(c, s, p, c->patch, f.split, f.fmt != 0))) return rc;  // (fp16 records from the backbone)
    conv_shape(p, f.B, f.H, f.W, f.C, dim, g.patch_h, g.patch_w, g.patch_h, g.patch_w, 0, 0, gh, gw);
    const float* pos;
    if ((rc = pos_table_for(c, gh, gw, s, &pos))) return rc;
    p.row_add = pos; p.rows_per_img = gh * gw; p.img_stride = T; p.row_off = 1; p.row_add_off = 1;
    HIPCHK(c, conv_timed(c, p, s));
    HIPCHK(c, launch_fill_cls(c->cls_row, X, B, (long long)T * dim, dim, s));
  }
  const int M = B * T;
  float* Hn = pick(c, {X});
  float* Q = pick(c, {X, Hn});
  float* X2 = pick(c, {X, Hn, Q});
  for (size_t i = 0; i < c->vit.size(); ++i) {
    const VitBlock& vb = c->vit[i];
    // Block.forward (vision_transformer.py:119-122), LayerNorm eps 1e-6 (:175)
    HIPCHK(c, launch_layernorm(X, vb.n1.g, vb.n1.b, Hn, M, dim, 1e-6f, s));
    HIPCHK(c, linear_any(c, s, Hn, vb.qkv, nullptr, Q, M, ACT_NONE));
    float* map = i < (size_t)n_maps ? maps_dev[i] : nullptr;  // the block's attn_drop input [B][heads][T][T]
    if (map) HIPCHK(c, launch_vit_attention_probs(Q, Hn, map, B, T, g.vit_heads, s));
    else HIPCHK(c, launch_vit_attention(Q, Hn, B, T, g.vit_heads, s));
    HIPCHK(c, linear_any(c, s, Hn, vb.proj, X, X2, M, ACT_NONE));
    HIPCHK(c, launch_layernorm(X2, vb.n2.g, vb.n2.b, Hn, M, dim, 1e-6f, s));
    HIPCHK(c, linear_any(c, s, Hn, vb.fc1, nullptr, Q, M, ACT_GELU));
    HIPCHK(c, linear_any(c, s, Q, vb.fc2, X2, X, M, ACT_NONE));
  }
  HIPCHK(c, launch_layernorm(X, c->vit_norm.g, c->vit_norm.b, memory, M, dim, 1e-6f, s));
  (void)err;
  return D2T_OK;
}

int d2t_set_reserved_blocks(d2t_ctx* c, int32_t blocks) {
  DevGuard dg_(c);
  if (!c || blocks < 0) return fail(c, D2T_EINVAL, "bad argument");
  if (!c->num_cus) {
    hipDeviceProp_t prop;
    int dev = 0;
    HIPCHK(c, hipGetDevice(&dev));
    HIPCHK(c, hipGetDeviceProperties(&prop, dev));
    c->num_cus = prop.multiProcessorCount;
  }
  const int slots = 2 * c->num_cus;  // the convolution runs two blocks per CU
  if (blocks >= slots) return fail(c, D2T_EINVAL, "cannot reserve %d of %d block slots", blocks, slots);
  c->conv_max_blocks = blocks ? slots - blocks : 0;
  return D2T_OK;
}

int d2t_set_reserved_cus(d2t_ctx* c, int32_t cus) {
  DevGuard dg_(c);
  if (!c || cus < 0 || cus > 128) return fail(c, D2T_EINVAL, "reserved CUs must be in [0, 128]");
  c->reserved_cus = cus;
  return D2T_OK;
}

int d2t_set_conv_kernel(d2t_ctx* c, int32_t kind) {
  DevGuard dg_(c);
  if (!c || (kind != 0 && kind != 3))
    return fail(c, D2T_EINVAL, "conv kernel must be 3 (pipelined 256x128 on 16x16x32 MFMAs, one block per CU) or 0 (128x128 on 32x32x16 MFMAs, two blocks per CU)");
  if ((c->conv_f16 || c->mixed_units) && kind != 3) return fail(c, D2T_ESTATE, "the fp16x2 convolutions exist for conv kernel 3 only");
  c->conv_pipelined = kind;
  return D2T_OK;
}

int d2t_set_beam_shared_tile(d2t_ctx* c, int32_t on) {
  DevGuard dg_(c);
  if (!c) return D2T_EINVAL;
  c->beam_shared_tile = on != 0;
  return D2T_OK;
}

int d2t_set_conv_fusion(d2t_ctx* c, int32_t pools, int32_t shortcuts) {
  DevGuard dg_(c);
  if (!c) return D2T_EINVAL;
  c->no_pool_fusion = pools == 0;
  c->no_shortcut_fusion = shortcuts == 0;
  return D2T_OK;
}

int d2t_set_decode_chains(d2t_ctx* c, int32_t chains) {
  DevGuard dg_(c);
  if (!c || chains < 1 || chains > d2t_ctx::MAXC) return fail(c, D2T_EINVAL, "decode chains must be 1 .. %d", d2t_ctx::MAXC);
  c->n_chains = chains;
  return D2T_OK;
}

int d2t_set_conv_precision(d2t_ctx* c, int32_t mode) {
  DevGuard dg_(c);
  if (!c || (mode != D2T_CONV_FP32 && mode != D2T_CONV_BF16X3 && mode != D2T_CONV_FP16X2 && mode != D2T_CONV_MIXED))
    return fail(c, D2T_EINVAL, "unknown conv precision %d", mode);
  if ((mode == D2T_CONV_FP16X2 || mode == D2T_CONV_MIXED) && c->conv_pipelined != 3)
    return fail(c, D2T_ESTATE, "the fp16x2 convolutions exist for conv kernel 3 (pipelined 256x128 on 16x16x32 MFMAs) only");
  c->conv_bf16x3 = mode != D2T_CONV_FP32;
  c->conv_f16 = mode == D2T_CONV_FP16X2;
  c->mixed_units = mode == D2T_CONV_MIXED ? D2T_MIXED_UNITS_DEFAULT : 0;
  return D2T_OK;
}

int d2t_set_mixed_units(d2t_ctx* c, int32_t units) {
  DevGuard dg_(c);
  if (!c || units < 0 || units > 8) return fail(c, D2T_EINVAL, "mixed units must be 0 .. 8");
  if (units > 0 && (!c->conv_bf16x3 || c->conv_f16 || c->conv_pipelined != 3))
    return fail(c, D2T_ESTATE, "mixed units need the split-bf16 arithmetic on conv kernel 3");
  c->mixed_units = units;
  return D2T_OK;
}

int d2t_profile_enable(d2t_ctx* c, int32_t on) {
  DevGuard dg_(c);
  if (!c) return D2T_EINVAL;
  c->profiling = on != 0;
  return D2T_OK;
}

int d2t_profile_read(d2t_ctx* c, int32_t max_records, int32_t* n, int32_t* M, int32_t* N, int32_t* K, float* ms) {
  DevGuard dg_(c);
  if (!c || !n) return D2T_EINVAL;
  HIPCHK(c, hipDeviceSynchronize());
  int out = 0;
  for (auto& r : c->prof) {
    if (out < max_records && M && N && K && ms) {
      float t = 0.f;
      if (hipEventElapsedTime(&t, r.a, r.b) != hipSuccess) t = -1.f;
      M[out] = r.M; N[out] = r.N; K[out] = r.K; ms[out] = t;
      ++out;
    }
    hipEventDestroy(r.a);
    hipEventDestroy(r.b);
  }
  c->prof.clear();
  *n = out;
  return D2T_OK;
}

}  // extern "C"
