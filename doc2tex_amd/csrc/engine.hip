// libd2t engine: context life cycle, the decode-stream pool, backbone and encoders (one function per network), setters and
// profiling of the C-ABI declared in include/d2t.h (the weights: engine_weights.hip; the decodes: engine_tfm.hip,
// engine_attn.hip; the d2t_op_* entries: engine_ops.hip).  Host code only launches the kernels of the other .hip files on the
// caller's HIP stream; there is no CPU compute path and no fallback.
#include "engine_impl.h"
#include <mutex>

// (ConvOpts is filled with designated initializers: C++20, which hipcc's clang takes in C++17 too)
#pragma clang diagnostic ignored "-Wc++20-designator"

namespace {

// spatial size after the VGG (vgg.py:16-41) for an H x W crop: pools (2,2), (2,2), (2,1), (2,1), then the 2x2 convolution
void vgg_hw(int H, int W, int* oh, int* ow) {
  *oh = H / 2 / 2 / 2 / 2 - 1;
  *ow = W / 2 / 2 - 1;
}
bool vgg_encoder(const d2t_config& g) { return g.encoder == D2T_ENC_VGG_BILSTM || g.encoder == D2T_ENC_VGG; }
bool lstm_encoder(const d2t_config& g) { return g.encoder == D2T_ENC_VGG_BILSTM || g.encoder == D2T_ENC_RESNET_BILSTM; }

// mean_height False: proj_feat = Linear(3 * C -> C) reads the whole height of the feature map, which must be 3 (build_feat.py:
// 38-40,56-61; the reference fails in the matrix product otherwise)
int proj_height_check(d2t_ctx* c, int fh) {
  if (fh == 3) return D2T_OK;
  return fail(c, D2T_EINVAL, "mean_height False: proj_feat reads a feature map of height 3 (64-pixel crops), this crop gives "
              "height %d", fh);
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

// A layer's operands in a ConvP (Net::conv and the patch embedding): the folded weights, with their bf16 planes in bf16x3
// mode, the input as fp32 or as split records, and how a convolution behind the stem is routed: split-record input brings the
// zero page and the block cap; fp16 records in select the two-MFMA kernels (x16 * w_lo + x16 * w_hi) on the layer's fp16
// hi / lo weight planes, made on first use; the pipelined kernel's switches come from the context.
int conv_operands(d2t_ctx* c, hipStream_t s, ConvP& p, const ConvW& w, const Act& x) {
  p.w = w.w; p.bias = w.bias;
  if (c->conv_bf16x3) { p.w_hi = w.w_hi; p.w_lo = w.w_lo; }
  if (x.split) { p.in_hi = x.planes(); p.zero16 = c->zero_page; p.max_blocks = c->conv_max_blocks; }
  else p.in = x.p;
  if (x.split && x.fmt != 0) {
    if (int rc = eng::f16_planes(c, const_cast<ConvW&>(w), s)) return rc;  // (w lives in *c)
    p.f16 = 1;
    p.w_hi = w.w_h16; p.w_lo = w.w_l16;
  }
  p.pipelined = c->conv_pipelined; p.reserved_cus = c->reserved_cus;
  p.split_tail = !c->decode_in_flight || D2T_PROBE_ENV("D2T_CONV_TAIL_ALWAYS");
  return D2T_OK;
}

// How one convolution differs from the common one: 3x3, stride 1, padding 1, ReLU, no residual, output in the network's own
// representation, in a rotating buffer that holds neither the input nor the residual
struct ConvOpts {
  int sh = 1, sw = 1, ph = 1, pw = 1;
  int act = ACT_RELU;
  const Act* res = nullptr;
  const ConvP* extra = nullptr;  // fields set beforehand: a second 1x1 input (in2_hi, Cin2), a row table added in the epilogue
  float* out = nullptr;          // nullptr: Net::pick({input, residual})
  // split-record output planes (only meaningful on the bf16x3 path; the consumer must be another bf16x3 convolution or the
  // split pool); -1: as the network's activations (Net::split)
  int out_split = -1;
  // fuse the 2x2 / stride 2 max-pool that follows (split-record path only: see ConvP::pool2); the result is then the POOLED map
  bool pool2 = false;
  // record format of a split output (conv_common.h REC_*); -1 = the input's (fp16x2 mode: one fp16; else bf16 hi | lo)
  int out_fmt = -1;
};

// Launches the layers of one network on one stream.  A failed launch does not stop the network: the first error is kept and
// the caller reports it once, behind the last layer.
struct Net {
  d2t_ctx* c;
  hipStream_t s;
  bool split = false;  // the activations between the first and the last layer are split records, not fp32
  hipError_t err = hipSuccess;

  void note(hipError_t e) { if (e != hipSuccess && err == hipSuccess) err = e; }

  // a rotating activation buffer that is not in `live`
  float* pick(std::initializer_list<const float*> live) const {
    for (int i = 0; i < 4; ++i) {
      bool used = false;
      for (const float* l : live) used |= (l == c->act[i]);
      if (!used) return c->act[i];
    }
    return nullptr;
  }

  Act conv(const Act& x, const ConvW& w, const ConvOpts& o = {}) {
    const bool out_split = o.out_split < 0 ? split : o.out_split != 0;
    Act y{o.out ? o.out : pick({x.p, o.res ? o.res->p : nullptr}), x.B, (x.H + 2 * o.ph - w.KH) / o.sh + 1,
          (x.W + 2 * o.pw - w.KW) / o.sw + 1, w.Cout};
    y.split = out_split;
    ConvP p{};
    if (o.extra) p = *o.extra;
    if (conv_operands(c, s, p, w, x) != D2T_OK) {  // (the fp16 planes could not be made)
      note(hipErrorOutOfMemory);
      return y;
    }
    if (out_split) {
      y.fmt = o.out_fmt >= 0 ? o.out_fmt : (x.split ? (x.fmt ? 1 : 0) : (c->conv_f16 ? 1 : 0));
      p.out_fmt = 1 + y.fmt;
      p.out_hi = y.planes();
    } else {
      p.out = y.p;
    }
    if (o.res && o.res->split) { p.res_fmt = 1 + o.res->fmt; p.res_hi = o.res->planes(); }
    else if (o.res) p.res = o.res->p;
    conv_shape(p, x.B, x.H, x.W, x.C, w.Cout, w.KH, w.KW, o.sh, o.sw, o.ph, o.pw);
    p.K += p.Cin2;  // (a second 1x1 input from `extra`)
    p.act = o.act;
    if (o.pool2) {  // rows in pooled order (floor: a last odd row / column belongs to no window and is never computed)
      p.pool2 = 1;
      p.M = 4 * y.B * (y.H / 2) * (y.W / 2);
      y.H /= 2;
      y.W /= 2;
    }
    note(conv_timed(c, p, s));
    return y;
  }

  // 2x2 max-pool over an fp32 map or over split records (of the same format on both sides)
  Act pool(const Act& a, int sh, int sw, int ph, int pw) {
    Act y{pick({a.p}), a.B, (a.H + 2 * ph - 2) / sh + 1, (a.W + 2 * pw - 2) / sw + 1, a.C};
    y.split = a.split;
    y.fmt = a.fmt;
    note(a.split ? launch_maxpool_split(a.planes(), y.planes(), a.B, a.H, a.W, a.C, sh, sw, ph, pw, s, a.fmt)
                 : launch_maxpool(a.p, y.p, a.B, a.H, a.W, a.C, sh, sw, ph, pw, s));
    return y;
  }
  // kh x kw max-pool with the window as its stride, fp32 (VGG)
  Act pool_k(const Act& a, int kh, int kw) {
    Act y{pick({a.p}), a.B, (a.H - kh) / kh + 1, (a.W - kw) / kw + 1, a.C};
    note(launch_maxpool_k(a.p, y.p, a.B, a.H, a.W, a.C, kh, kw, kh, kw, 0, 0, s));
    return y;
  }
};

// Mixed precision (ctx.h mixed_units): the first `mixed_units` of the backbone's eight plain 512 -> 512 units
//   0 layer3.1   1 layer3.2   2 layer3.3   3 layer3.4   4 conv3   5 layer4.0   6 layer4.1   7 layer4.2
// run the two-MFMA arithmetic.  A tensor that a mixed unit consumes is written as fp16 hi | lo pairs (its MFMAs read the hi
// half, the residual add both), the map between a mixed block's two convolutions as one fp16.
// mixed_unit: the unit that block bi of stage li (both from 0) is, or -1 (layer3.0 has a shortcut; layer1, layer2 are narrower)
int mixed_unit(int li, int bi) {
  if (li == 2) return bi - 1;
  if (li == 3) return 5 + bi;
  return -1;
}
// the unit that consumes that block's output, or -1: layer3.4 feeds conv3 (unit 4); layer4.2 feeds conv4_1, which is never mixed
int consumer_unit(int li, int bi) {
  if (li == 2) return bi;
  if (li == 3 && bi < 2) return 6 + bi;
  return -1;
}

// BasicBlock.forward (feature_extractor/resnet.py:28-45).  mixed: the block is a mixed unit; mixed_next: its consumer is one.
Act basic_block(Net& n, const Block& b, const Act& x, bool mixed, bool mixed_next) {
  d2t_ctx* c = n.c;
  if (mixed && !b.has_down) {
    Act t = n.conv(x, b.c1, {.out_fmt = 1});
    return n.conv(t, b.c2, {.res = &x, .out_fmt = mixed_next ? 2 : 0});
  }
  const int fmt = mixed_next ? 2 : -1;
  Act t = n.conv(x, b.c1);
  float* out = n.pick({x.p, t.p});
  if (b.has_down && b.c2cat.w && n.split && c->conv_pipelined == 3 && b.c2.Cout >= 128 && !c->no_shortcut_fusion) {
    // the 1x1 shortcut inside conv2's launch: K-steps over x appended behind the taps over t, one accumulator, no residual
    ConvP ex{};
    ex.in2_hi = x.planes();
    ex.Cin2 = x.C;
    return n.conv(t, b.c2cat, {.extra = &ex, .out = out, .out_fmt = fmt});
  }
  if (!b.has_down) return n.conv(t, b.c2, {.res = &x, .out = out, .out_fmt = fmt});
  Act r = n.conv(x, b.down, {.ph = 0, .pw = 0, .act = ACT_NONE, .out = out});
  return n.conv(t, b.c2, {.res = &r, .out = n.pick({x.p, t.p, r.p}), .out_fmt = fmt});
}

// One stage of the ResNet: its blocks and, with gcb, the GlobalContext that closes it (resnet.py:200-201), in place
Act run_stage(Net& n, int li, Act x, int nmix) {
  d2t_ctx* c = n.c;
  auto mixed = [&](int u) { return u >= 0 && u < nmix; };
  int bi = 0;
  for (const Block& b : c->layers[li]) {
    x = basic_block(n, b, x, mixed(mixed_unit(li, bi)), mixed(consumer_unit(li, bi)));
    ++bi;
  }
  if (c->cfg.gcb) {
    const int HW = x.H * x.W;
    float* ws = c->gc_ws;  // logits [B*HW] | ctx [B][C] | y [B][C]
    n.note(launch_global_context(x.p, c->gc[li], ws, ws + (size_t)x.B * HW, ws + (size_t)x.B * HW + (size_t)x.B * x.C, x.B, HW,
                                 x.C, n.s));
  }
  return x;
}

// ResNet.forward (feature_extractor/resnet.py:205-245).  On the bf16x3 path every activation between the
// stem and the last convolution lives as split-bf16 planes; `final_split` says whether the returned map
// does too (a bf16x3 consumer follows) or is fp32 (final_out / any other consumer).
int run_backbone(d2t_ctx* c, hipStream_t s, const float* img, int B, int H, int W, Act* out, float* final_out,
                 const ConvP* final_extra, bool final_split) {
  // GlobalContext blocks read and update whole fp32 maps, so with gcb the activations stay fp32 (the convolutions still
  // take the split-bf16 kernel in bf16x3 mode, splitting their input on the fly)
  const bool sp = c->conv_bf16x3 && !c->cfg.gcb;
  Net n{c, s, sp};
  Act x{n.pick({}), B, H, W, c->stem.Cout};
  x.split = sp;
  const int f16 = sp && c->conv_f16;  // fp16 records between the stem and the last convolution
  x.fmt = f16;
  const int nmix = (sp && !f16 && c->conv_pipelined == 3) ? c->mixed_units : 0;
  if (sp) HIPCHK(c, launch_stem_split(img, c->stem.w, c->stem.bias, x.planes(), B, c->stem.Cin, H, W, c->stem.Cout, ACT_RELU, s, f16));
  else HIPCHK(c, launch_stem(img, c->stem.w, c->stem.bias, x.p, B, c->stem.Cin, H, W, c->stem.Cout, ACT_RELU, s));
  // the two 2x2 / stride 2 max-pools (resnet.py:94,106) run inside the epilogue of the convolution in front of them on the
  // split-record path with the 16x16x32 kernels: conv0_2 writes 268 MB instead of 1.07 GB and no pool kernel re-reads it
  const bool fuse_pool = sp && c->conv_pipelined == 3 && !c->no_pool_fusion;
  const bool fuse_pool2 = fuse_pool && c->conv1.Cout >= 128;  // (the pipelined 16x16x32 kernel takes layers with >= 128 channels)
  x = n.conv(x, c->conv0_2, {.pool2 = fuse_pool});
  if (c->cfg.gcb) {
    const int rc = ensure(c, &c->gc_ws, &c->gc_ws_cap, ((size_t)B * (H / 2) * (W / 2) + 2 * (size_t)B * 512 + 64) * 4);
    if (rc) return rc;
  }
  if (!fuse_pool) x = n.pool(x, 2, 2, 0, 0);
  x = run_stage(n, 0, x, nmix);
  x = n.conv(x, c->conv1, {.pool2 = fuse_pool2});
  if (!fuse_pool2) x = n.pool(x, 2, 2, 0, 0);
  x = run_stage(n, 1, x, nmix);
  x = n.conv(x, c->conv2);
  x = n.pool(x, 2, 1, 0, 1);
  x = run_stage(n, 2, x, nmix);
  x = n.conv(x, c->conv3, {.out_fmt = 5 < nmix ? 2 : x.fmt == 2 ? 0 : -1});  // (its consumer, layer4.0, is unit 5)
  x = run_stage(n, 3, x, nmix);
  x = n.conv(x, c->conv4_1, {.sh = 2, .ph = 0});
  x = n.conv(x, c->conv4_2, {.ph = 0, .pw = 0, .extra = final_extra, .out = final_out, .out_split = sp && final_split && !final_out});
  if (n.err != hipSuccess) return fail(c, D2T_EHIP, "backbone launch: %s", hipGetErrorString(n.err));
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
    if (int rc = owned_alloc(c, &t.p, (size_t)(gh * gw + 1) * D)) return rc;
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

// The four rotating activation buffers, each as large as the largest activation of an encode of B crops H x W (memory
// [B][T][dim]): conv0_2's output B*H*W*64 floats; a ViT needs B*T*max(3*dim, mlp hidden), a BiLSTM B*T*8*hidden (its gates)
int ensure_activations(d2t_ctx* c, int B, int H, int W, int T, int dim) {
  const d2t_config& g = c->cfg;
  size_t need_floats = (size_t)B * H * W * 64;
  if (g.encoder == D2T_ENC_HYBRID_VIT) {
    size_t hid = c->vit.empty() ? 0 : (size_t)c->vit[0].fc1.N;
    size_t v = (size_t)B * T * (hid > 3 * (size_t)dim ? hid : 3 * (size_t)dim);
    if (v > need_floats) need_floats = v;
  }
  if (lstm_encoder(g) && (size_t)B * T * 8 * g.bilstm_hidden > need_floats) need_floats = (size_t)B * T * 8 * g.bilstm_hidden;
  if (c->act_cap >= need_floats * 4) return D2T_OK;
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
  return D2T_OK;
}

// VGG_FeatureExtractor.forward (feature_extractor/vgg.py:16-44).  final_out / final_extra: the last convolution (2x2, bias,
// ReLU, no BatchNorm) writes there, with a row table added behind its ReLU (encode_vgg_flat)
int encode_vgg(d2t_ctx* c, hipStream_t s, const float* image, int B, int H, int W, Act* out, float* final_out = nullptr,
               const ConvP* final_extra = nullptr) {
  Net n{c, s};
  Act x{n.pick({}), B, H, W, c->vgg[0].Cout};
  HIPCHK(c, launch_stem(image, c->vgg[0].w, c->vgg[0].bias, x.p, B, c->vgg[0].Cin, H, W, x.C, ACT_RELU, s));
  x = n.pool_k(x, 2, 2);
  x = n.conv(x, c->vgg[1]);
  x = n.pool_k(x, 2, 2);
  x = n.conv(x, c->vgg[2]);
  x = n.conv(x, c->vgg[3]);
  x = n.pool_k(x, 2, 1);
  x = n.conv(x, c->vgg[4]);
  x = n.conv(x, c->vgg[5]);
  x = n.pool_k(x, 2, 1);
  x = n.conv(x, c->vgg[6], {.ph = 0, .pw = 0, .extra = final_extra, .out = final_out});
  if (n.err != hipSuccess) return fail(c, D2T_EHIP, "VGG launch: %s", hipGetErrorString(n.err));
  *out = x;
  return D2T_OK;
}

// Behind either feature extractor's map f: AdaptiveAvgPool2d((None,1)) over the height (build_feat.py:50-55) -- or, with
// mean_height False, proj_feat over the [b, w, c * h] flattening of a map of height 3 (:56-61), which is a convolution with
// window (3, 1) over the NHWC map (pack_proj_feat) -- then 2x BidirectionalLSTM (seq_modeling/bilstm.py:6-24); the second
// one's Linear writes the memory [B][T][hidden]
int encode_bilstm_tail(d2t_ctx* c, hipStream_t s, const Act& f, int T, float* memory) {
  if (f.W != T || f.C != 512) return fail(c, D2T_EINVAL, "unexpected feature map %dx%dx%d", f.H, f.W, f.C);
  Net n{c, s};
  const int B = f.B, Hh = c->cfg.bilstm_hidden;
  float* seq;
  if (c->cfg.proj_height) {
    if (int rc = proj_height_check(c, f.H)) return rc;
    const Act y = n.conv(f, c->proj_feat, {.ph = 0, .pw = 0, .act = ACT_NONE, .out_split = 0});
    if (n.err != hipSuccess) return fail(c, D2T_EHIP, "proj_feat launch: %s", hipGetErrorString(n.err));
    seq = y.p;
  } else {
    seq = n.pick({f.p});
    HIPCHK(c, launch_mean_h(f.p, seq, B, f.H, f.W, f.C, s));
  }
  for (int i = 0; i < 2; ++i) {
    const BiLstmW& L = c->lstm[i];
    float* gates = n.pick({seq});
    float* rec = n.pick({seq, gates});
    LinW ih{L.wih_cat, L.bias_cat, 8 * Hh, L.in};
    HIPCHK(c, linear_any(c, s, seq, ih, nullptr, gates, B * T, ACT_NONE));
    HIPCHK(c, launch_bilstm(gates, L.whh_t, rec, B, T, Hh, s));
    float* out = i == 1 ? memory : n.pick({rec});
    HIPCHK(c, linear_any(c, s, rec, L.lin, nullptr, out, B * T, ACT_NONE));
    seq = out;
  }
  return D2T_OK;
}

// Feat=ResNet, Seq=None: PositionalEncoding2D add, [B,C,H,W] -> [B,HW,C] (build_seq.py:69-76), both in the epilogue of the
// backbone's last convolution, which writes the memory
int encode_resnet_flat(d2t_ctx* c, hipStream_t s, const float* image, int B, int H, int W, float* memory) {
  int fh, fw;
  backbone_hw(H, W, &fh, &fw);
  const float* pe;
  if (int rc = get_pe2d(c, fh, fw, c->cfg.backbone_out, s, &pe)) return rc;
  ConvP ex{};
  ex.row_add = pe; ex.rows_per_img = fh * fw; ex.img_stride = fh * fw; ex.row_off = 0; ex.row_add_off = 0;
  Act f{};
  return run_backbone(c, s, image, B, H, W, &f, memory, &ex, false);
}

// Feat=VGG, Seq=None: as encode_resnet_flat, in the epilogue of the VGG's last convolution (bias, ReLU, then the table's row)
int encode_vgg_flat(d2t_ctx* c, hipStream_t s, const float* image, int B, int H, int W, float* memory) {
  int fh, fw;
  vgg_hw(H, W, &fh, &fw);
  const float* pe;
  if (int rc = get_pe2d(c, fh, fw, c->cfg.backbone_out, s, &pe)) return rc;
  ConvP ex{};
  ex.row_add = pe; ex.rows_per_img = fh * fw; ex.img_stride = fh * fw; ex.row_off = 0; ex.row_add_off = 0;
  Act f{};
  return encode_vgg(c, s, image, B, H, W, &f, memory, &ex);
}

// HybridEmbed.forward (patchembed.py:115-141) over the backbone's map f: zero-pad right/bottom + Conv2d(k=s=patch) as one
// implicit GEMM whose out-of-range taps read zero; epilogue adds pos_embed[1+i] (flat prefix
// slice, vit_encoder.py:260) and leaves row 0 of every image for the cls token.  X: the tokens [B][T = 1 + gh*gw][dim]
int patch_embed(d2t_ctx* c, hipStream_t s, const Act& f, int gh, int gw, int dim, float* X) {
  const d2t_config& g = c->cfg;
  const int T = gh * gw + 1;
  ConvP p{};
  p.out = X;
  if (int rc = conv_operands(c, s, p, c->patch, f)) return rc;  // (f may hold fp16 records from the backbone)
  conv_shape(p, f.B, f.H, f.W, f.C, dim, g.patch_h, g.patch_w, g.patch_h, g.patch_w, 0, 0, gh, gw);
  const float* pos;
  if (int rc = pos_table_for(c, gh, gw, s, &pos)) return rc;
  p.row_add = pos; p.rows_per_img = gh * gw; p.img_stride = T; p.row_off = 1; p.row_add_off = 1;
  HIPCHK(c, conv_timed(c, p, s));
  HIPCHK(c, launch_fill_cls(c->cls_row, X, f.B, (long long)T * dim, dim, s));
  return D2T_OK;
}

// Hybrid ViT: the backbone, the patch embedding and ViTEncoder's blocks; block i's attn_drop input [B][heads][T][T] goes to
// maps_dev[i] where that is set
int encode_vit(d2t_ctx* c, hipStream_t s, const float* image, int B, int H, int W, int gh, int gw, int dim, float* memory,
               float* const* maps_dev, int n_maps) {
  Act f{};
  if (int rc = run_backbone(c, s, image, B, H, W, &f, nullptr, nullptr, true)) return rc;
  const Net n{c, s};
  float* X = n.pick({f.p});
  if (int rc = patch_embed(c, s, f, gh, gw, dim, X)) return rc;
  const int T = gh * gw + 1, M = B * T;
  float* Hn = n.pick({X});
  float* Q = n.pick({X, Hn});
  float* X2 = n.pick({X, Hn, Q});
  for (size_t i = 0; i < c->vit.size(); ++i) {
    const VitBlock& vb = c->vit[i];
    // Block.forward (vision_transformer.py:119-122), LayerNorm eps 1e-6 (:175)
    HIPCHK(c, launch_layernorm(X, vb.n1.g, vb.n1.b, Hn, M, dim, 1e-6f, s));
    HIPCHK(c, linear_any(c, s, Hn, vb.qkv, nullptr, Q, M, ACT_NONE));
    float* map = i < (size_t)n_maps ? maps_dev[i] : nullptr;
    if (map) HIPCHK(c, launch_vit_attention_probs(Q, Hn, map, B, T, c->cfg.vit_heads, s));
    else HIPCHK(c, launch_vit_attention(Q, Hn, B, T, c->cfg.vit_heads, s));
    HIPCHK(c, linear_any(c, s, Hn, vb.proj, X, X2, M, ACT_NONE));
    HIPCHK(c, launch_layernorm(X2, vb.n2.g, vb.n2.b, Hn, M, dim, 1e-6f, s));
    HIPCHK(c, linear_any(c, s, Hn, vb.fc1, nullptr, Q, M, ACT_GELU));
    HIPCHK(c, linear_any(c, s, Q, vb.fc2, X2, X, M, ACT_NONE));
  }
  HIPCHK(c, launch_layernorm(X, c->vit_norm.g, c->vit_norm.b, memory, M, dim, 1e-6f, s));
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
  } else if (cfg->encoder != D2T_ENC_RESNET && cfg->encoder != D2T_ENC_VGG && !lstm_encoder(*cfg)) {
    return fail(c, D2T_EINVAL, "unknown encoder %d", cfg->encoder);
  }
  if (lstm_encoder(*cfg) && cfg->bilstm_hidden != 256) return fail(c, D2T_EINVAL, "BiLSTM hidden_size must be 256");
  if (cfg->proj_height && !lstm_encoder(*cfg))
    return fail(c, D2T_EINVAL, "proj_height (mean_height False) is read by the BiLSTM encoders only");
  if (cfg->decoder == D2T_DEC_TFM) {
    const int hd = cfg->dec_heads > 0 ? cfg->dec_dim / cfg->dec_heads : 0;
    if (cfg->dec_dim != 256 && cfg->dec_dim != 512) return fail(c, D2T_EINVAL, "decoder d_model must be 256 or 512");
    if (hd != 32 && hd != 64) return fail(c, D2T_EINVAL, "decoder head_dim must be 32 or 64");
    if (cfg->dec_heads != 8) return fail(c, D2T_EINVAL, "decoder nhead must be 8");
    if (cfg->dec_ff % 64) return fail(c, D2T_EINVAL, "dim_feedforward must be a multiple of 64");
    if (cfg->max_seq_len + 2 > 512) return fail(c, D2T_EINVAL, "max_seq_len must be <= 510");
    if (lstm_encoder(*cfg) && cfg->dec_dim != cfg->bilstm_hidden)
      return fail(c, D2T_EINVAL, "a TFM decoder behind the BiLSTM needs d_model = the BiLSTM hidden_size (256), got %d", cfg->dec_dim);
  } else if (cfg->decoder == D2T_DEC_ATTN) {
    if (cfg->attn_hidden != 256) return fail(c, D2T_EINVAL, "Attn hidden_size / input_size must be 256");
    if (cfg->attn_kernel_size < 0 || cfg->attn_kernel_size > 5) return fail(c, D2T_EINVAL, "Attn kernel_size must be <= 5");
    if (cfg->vocab > D2T_ATTN_MAX_CLASSES)
      return fail(c, D2T_EINVAL, "Attn decoder supports num_class <= %d, got %d", D2T_ATTN_MAX_CLASSES, cfg->vocab);
    if (cfg->batch_max_length < 1) return fail(c, D2T_EINVAL, "batch_max_length must be >= 1");
    if (cfg->encoder == D2T_ENC_RESNET || cfg->encoder == D2T_ENC_VGG)
      return fail(c, D2T_EINVAL, "Feat=ResNet|VGG + Seq=None is paired with the TFM decoder only");
    if (cfg->encoder == D2T_ENC_HYBRID_VIT && cfg->vit_dim != 256) return fail(c, D2T_EINVAL, "Attn over ViT needs hidden_size 256");
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
  eng::free_packed(c);
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
  if (c->maps_ws) hipFree(c->maps_ws);
  if (c->h_pinned) hipHostFree(c->h_pinned);
  if (c->zero_page) hipFree(c->zero_page);
  if (c->gc_ws) hipFree(c->gc_ws);
  if (c->ev_in) hipEventDestroy(c->ev_in);
  if (c->brg_tab) hipFree(c->brg_tab);
  if (c->brg_host) hipHostFree(c->brg_host);
  if (c->h_steps) hipHostFree(c->h_steps);
  for (int i = 0; i < d2t_ctx::ABEAM_TABS; ++i) {
    if (c->abeam_tab_host[i]) hipHostFree(c->abeam_tab_host[i]);
    if (c->abeam_tab_ev[i]) hipEventDestroy(c->abeam_tab_ev[i]);
  }
  for (hipEvent_t ev : c->ticket_ev) if (ev) hipEventDestroy(ev);
  for (d2t_ctx::Chain& o : c->chains) {
    if (o.skv) hipFree(o.skv);
    if (o.dws) hipFree(o.dws);
    if (o.dstate) hipFree(o.dstate);
    if (o.out) hipFree(o.out);
    if (o.abeam_ws) hipFree(o.abeam_ws);
    if (o.abeam_mem) hipFree(o.abeam_mem);
    if (o.abeam_hist) hipFree(o.abeam_hist);
    for (int i = 0; i < 2; ++i) {
      if (o.agrp_host[i]) hipHostFree(o.agrp_host[i]);
      if (o.agrp_ev[i]) hipEventDestroy(o.agrp_ev[i]);
    }
  }
  // the streams go back to the process-wide pool, last acquired first (the next context takes them in the same roles)
  for (int i = d2t_ctx::MAXC - 1; i >= 0; --i)
    if (c->chains[i].stream) release_stream(c->device, c->stream_prio, c->chains[i].stream);
  delete c;
}

const char* d2t_last_error(const d2t_ctx* c) { return c ? c->err.c_str() : "null ctx"; }

int d2t_device_of(const d2t_ctx* c) { return c ? c->device : -1; }


int d2t_encoder_shape(const d2t_ctx* c, int32_t H, int32_t W, int32_t* T, int32_t* d, int32_t* grid_h,
                      int32_t* grid_w, int32_t* pad_w, int32_t* pad_h) {
  if (!c) return D2T_EINVAL;
  if (H < 4 || W < 4) return D2T_EINVAL;
  int fh, fw;
  if (vgg_encoder(c->cfg)) vgg_hw(H, W, &fh, &fw);
  else backbone_hw(H, W, &fh, &fw);
  if (fh < 1 || fw < 1) return D2T_EINVAL;
  int gh = fh, gw = fw, pw = 0, ph = 0, t, dim = c->cfg.backbone_out;
  if (lstm_encoder(c->cfg)) {
    t = fw;  // the height is averaged (build_feat.py:50-55) or projected (:56-61) away
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
  if (g.encoder == D2T_ENC_HYBRID_VIT && g.vit_pos != D2T_VIT_POS_LEARNED_INTERP && T > c->pos_rows)  // the prefix slice would run off the table
    return fail(c, D2T_EINVAL, "crop %dx%d exceeds max_dimension (pos_embed rows %d)", H, W, c->pos_rows);
  if (T > memory_cap(c)) return fail(c, D2T_EINVAL, "memory length %d > %d unsupported", T, memory_cap(c));
  if (g.proj_height) {  // refused before anything is launched: the caller's memory stays as it is
    int fh, fw;
    if (vgg_encoder(g)) vgg_hw(H, W, &fh, &fw);
    else backbone_hw(H, W, &fh, &fw);
    if (int rc = proj_height_check(c, fh)) return rc;
  }
  if (int rc = ensure_activations(c, B, H, W, T, dim)) return rc;
  Act f{};
  switch (g.encoder) {
    case D2T_ENC_VGG_BILSTM:
      if (int rc = encode_vgg(c, s, image, B, H, W, &f)) return rc;
      return encode_bilstm_tail(c, s, f, T, memory);
    case D2T_ENC_RESNET_BILSTM:
      if (int rc = run_backbone(c, s, image, B, H, W, &f, nullptr, nullptr, false)) return rc;
      return encode_bilstm_tail(c, s, f, T, memory);
    case D2T_ENC_HYBRID_VIT:
      return encode_vit(c, s, image, B, H, W, gh, gw, dim, memory, maps_dev, n_maps);
    case D2T_ENC_VGG:
      return encode_vgg_flat(c, s, image, B, H, W, memory);
    default:  // D2T_ENC_RESNET (d2t_create admits no other)
      return encode_resnet_flat(c, s, image, B, H, W, memory);
  }
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
