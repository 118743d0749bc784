// libd2t engine, the weights: d2t_load_weight keeps a state dict's tensors on the device, d2t_finalize_weights packs them into
// the layouts the kernels read -- one pack_* function per network, each beside the reference lines it restates.  Host code
// only: copies and the packing kernels of ops.hip on the caller's stream.
#include "engine_impl.h"

namespace {

// kh > 0: the weight is a Linear's [Cout][Cin * kh * kw] read as the OIHW filter [Cout][Cin][kh][kw] (pack_proj_feat)
int pack_conv(d2t_ctx* c, const std::string& conv, const std::string& bn, ConvW* out, hipStream_t s, int kh = 0, int kw = 0) {
  const RawW *w, *g = nullptr, *b = nullptr, *mu = nullptr, *var = nullptr;
  int rc = need(c, conv + ".weight", &w);
  if (rc) return rc;
  if (kh > 0) {
    if (w->shape.size() != 2 || w->shape[1] % (kh * kw))
      return fail(c, D2T_EINVAL, "linear weight '%s' is not [out][in * %d]", conv.c_str(), kh * kw);
  } else if (w->shape.size() != 4) {
    return fail(c, D2T_EINVAL, "conv weight '%s' is not 4-D", conv.c_str());
  }
  const RawW* cb = find(c, conv + ".bias");
  if (!bn.empty()) {
    if ((rc = need(c, bn + ".weight", &g)) || (rc = need(c, bn + ".bias", &b)) ||
        (rc = need(c, bn + ".running_mean", &mu)) || (rc = need(c, bn + ".running_var", &var)))
      return rc;
  }
  out->Cout = (int)w->shape[0];
  if (kh > 0) { out->Cin = (int)w->shape[1] / (kh * kw); out->KH = kh; out->KW = kw; }
  else { out->Cin = (int)w->shape[1]; out->KH = (int)w->shape[2]; out->KW = (int)w->shape[3]; }
  if ((rc = owned_alloc(c, &out->w, w->numel)) || (rc = owned_alloc(c, &out->bias, (size_t)out->Cout))) return rc;
  HIPCHK(c, launch_pack_conv(w->p, cb ? cb->p : nullptr, g ? g->p : nullptr, b ? b->p : nullptr, mu ? mu->p : nullptr,
                             var ? var->p : nullptr, 1e-5f, out->w, out->bias, out->Cout, out->Cin, out->KH, out->KW,
                             s));
  out->w_h16 = out->w_l16 = nullptr;  // fp16 hi / lo planes: made on first use (f16_planes), only the two-MFMA modes read them
  if (out->Cin % 32 == 0) {  // bf16 hi/lo planes of the folded weights (bf16x3 kernel)
    if ((rc = owned_alloc(c, &out->w_hi, w->numel)) || (rc = owned_alloc(c, &out->w_lo, w->numel))) return rc;
    HIPCHK(c, launch_split_bf16(out->w, out->w_hi, out->w_lo, w->numel, s));
  }
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
  uint16_t *ph, *pl;
  int rc;
  if ((rc = owned_alloc(c, &ph, n)) || (rc = owned_alloc(c, &pl, n))) return rc;
  HIPCHK(c, launch_split_bf16(w, ph, pl, n, s));
  *hi = ph;
  *lo = pl;
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

// VGG_FeatureExtractor (feature_extractor/vgg.py:16-41): nn.Sequential indices of the convs / BNs
int pack_vgg(d2t_ctx* c, hipStream_t s) {
  const char* convs[7] = {"0", "3", "6", "8", "11", "14", "18"};
  const char* bns[7] = {"", "", "", "", "12", "15", ""};
  for (int i = 0; i < 7; ++i)
    if (int rc = pack_conv(c, c->bb + convs[i], bns[i][0] ? c->bb + bns[i] : std::string(), &c->vgg[i], s)) return rc;
  if (c->vgg[0].Cin != c->cfg.in_channels || c->vgg[0].KH != 3 || c->vgg[0].KW != 3 || c->vgg[6].KH != 2 || c->vgg[6].Cout != 512)
    return fail(c, D2T_EINVAL, "unexpected VGG_FeatureExtractor shapes");
  return D2T_OK;
}

// proj_feat (recognizers/build_feat.py:38-40,56-61): Linear(3 * C -> C) over visual_feature.permute(0, 3, 1, 2).flatten(-2),
// whose column c * 3 + h is channel c at height h.  weight.view(C, C, 3, 1) therefore is the OIHW filter of a convolution with
// window (3, 1), stride 1 and no padding over the [B][3][W][C] map, and its output [B][1][W][C] is the BiLSTM's input
int pack_proj_feat(d2t_ctx* c, hipStream_t s) {
  const int C = c->cfg.backbone_out;
  if (int rc = pack_conv(c, "featextractor.proj_feat", "", &c->proj_feat, s, 3, 1)) return rc;
  if (c->proj_feat.Cout != C || c->proj_feat.Cin != C || !c->proj_feat.bias || !find(c, "featextractor.proj_feat.bias"))
    return fail(c, D2T_EINVAL, "featextractor.proj_feat must be Linear(%d -> %d) with a bias", 3 * C, C);
  return D2T_OK;
}

// One BasicBlock (feature_extractor/resnet.py:12-45) under the key prefix p.  A block with a 1x1 shortcut of conv2's width also
// gets conv2 | shortcut concatenated along K (Block::c2cat): both are already folded and in the kernels' K order (a 1x1
// layer's is plain)
int pack_block(d2t_ctx* c, const std::string& p, Block* b, hipStream_t s) {
  int rc;
  if ((rc = pack_conv(c, p + ".conv1", p + ".bn1", &b->c1, s))) return rc;
  if ((rc = pack_conv(c, p + ".conv2", p + ".bn2", &b->c2, s))) return rc;
  if (!find(c, p + ".downsample.0.weight")) return D2T_OK;
  b->has_down = true;
  if ((rc = pack_conv(c, p + ".downsample.0", p + ".downsample.1", &b->down, s))) return rc;
  if (!(b->c2.w_hi && b->down.w_hi && b->down.KH == 1 && b->down.KW == 1 && b->down.Cout == b->c2.Cout)) return D2T_OK;
  const int Co = b->c2.Cout, K2 = b->c2.KH * b->c2.KW * b->c2.Cin, Kd = b->down.Cin;
  const size_t n = (size_t)Co * (K2 + Kd);
  ConvW& cat = b->c2cat;
  cat = b->c2;
  cat.w_h16 = cat.w_l16 = nullptr; cat.K2 = Kd;  // (K2: the K rows of the second, 1x1 input)
  if ((rc = owned_alloc(c, &cat.w, n)) || (rc = owned_alloc(c, &cat.bias, (size_t)Co)) || (rc = owned_alloc(c, &cat.w_hi, n)) ||
      (rc = owned_alloc(c, &cat.w_lo, n)))
    return rc;
  HIPCHK(c, eng::concat_k(b->c2.w, b->c2.bias, K2, b->down.w, b->down.bias, Kd, Co, cat.w, cat.bias, cat.w_hi, cat.w_lo, s));
  return D2T_OK;
}

// GlobalContext(planes) appended to a stage (visual_attention.py:105-165), C channels, under the key prefix p
int pack_global_context(d2t_ctx* c, const std::string& p, int C, GCParams* out) {
  const RawW *wg, *bg, *w1, *b1, *lg, *lb, *w2, *b2;
  int rc;
  if ((rc = need(c, p + "global_cxt.weight", &wg, {1, C, 1, 1})) || (rc = need(c, p + "global_cxt.bias", &bg, {1})) ||
      (rc = need(c, p + "bottleneck_add.fc1.weight", &w1, {C, C, 1, 1})) ||
      (rc = need(c, p + "bottleneck_add.fc1.bias", &b1, {C})) ||
      (rc = need(c, p + "bottleneck_add.norm.weight", &lg, {C})) || (rc = need(c, p + "bottleneck_add.norm.bias", &lb, {C})) ||
      (rc = need(c, p + "bottleneck_add.fc2.weight", &w2, {C, C, 1, 1})) ||
      (rc = need(c, p + "bottleneck_add.fc2.bias", &b2, {C})))
    return rc;
  *out = GCParams{wg->p, bg->p, w1->p, b1->p, lg->p, lb->p, w2->p, b2->p};
  return D2T_OK;
}

// ResNet (feature_extractor/resnet.py:205-245, layers :262), in the order of its forward
int pack_resnet(d2t_ctx* c, hipStream_t s) {
  const d2t_config& g = c->cfg;
  const std::string& bb = c->bb;
  int rc;
  if ((rc = pack_conv(c, bb + "conv0_1", bb + "bn0_1", &c->stem, s))) return rc;
  if (c->stem.Cin != g.in_channels || c->stem.KH != 3 || c->stem.KW != 3)
    return fail(c, D2T_EINVAL, "conv0_1 must be %d-channel 3x3 (the config's in_channels), got %d channels %dx%d", g.in_channels,
                c->stem.Cin, c->stem.KH, c->stem.KW);
  if ((rc = pack_conv(c, bb + "conv0_2", bb + "bn0_2", &c->conv0_2, s))) return rc;
  for (int li = 0; li < 4; ++li) {
    const std::string layer = bb + "layer" + std::to_string(li + 1) + ".";
    for (int bi = 0; bi < RESNET_LAYERS[li]; ++bi) {
      Block b;
      if ((rc = pack_block(c, layer + std::to_string(bi), &b, s))) return rc;
      c->layers[li].push_back(b);
    }
    if (g.gcb && (rc = pack_global_context(c, layer + std::to_string(RESNET_LAYERS[li]) + ".", c->layers[li].back().c2.Cout, &c->gc[li])))
      return rc;
  }
  if ((rc = pack_conv(c, bb + "conv1", bb + "bn1", &c->conv1, s))) return rc;
  if ((rc = pack_conv(c, bb + "conv2", bb + "bn2", &c->conv2, s))) return rc;
  if ((rc = pack_conv(c, bb + "conv3", bb + "bn3", &c->conv3, s))) return rc;
  if ((rc = pack_conv(c, bb + "conv4_1", bb + "bn4_1", &c->conv4_1, s))) return rc;
  return pack_conv(c, bb + "conv4_2", bb + "bn4_2", &c->conv4_2, s);
}

// 2x BidirectionalLSTM (seq_modeling/bilstm.py:6-24, build_seq.py:20-23): nn.LSTM(bidirectional) + Linear, under the key
// prefix sm
int pack_bilstm(d2t_ctx* c, const std::string& sm, hipStream_t s) {
  const int Hh = c->cfg.bilstm_hidden, G4 = 4 * Hh;
  int in = 512, rc;
  for (int i = 0; i < 2; ++i) {
    const std::string lp = sm + std::to_string(i) + ".";
    BiLstmW& L = c->lstm[i];
    L.in = in;
    if ((rc = owned_alloc(c, &L.wih_cat, (size_t)2 * G4 * in)) || (rc = owned_alloc(c, &L.bias_cat, (size_t)2 * G4)) ||
        (rc = owned_alloc(c, &L.whh_t, (size_t)2 * Hh * G4)))
      return rc;
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
  return D2T_OK;
}

// HybridEmbed's projection + ViTEncoder (patchembed.py:115-141, vit_encoder.py, vision_transformer.py:119-122), under the key
// prefix sm
int pack_vit(d2t_ctx* c, const std::string& sm, hipStream_t s) {
  const d2t_config& g = c->cfg;
  const int D = g.vit_dim;
  int rc;
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
  if ((rc = owned_alloc(c, &c->cls_row, (size_t)D))) return rc;
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
  if (g.decoder == D2T_DEC_TFM && g.dec_dim != D) return fail(c, D2T_EINVAL, "decoder d_model must equal the ViT hidden_size");
  return D2T_OK;
}

// loc_proj o loc_conv (attention1D.py:150-152) as one filter w [H][taps] with bias b [H] (both sized by the caller), accumulated in double:
// conv_w [kd][taps], conv_b [kd], proj_w [H][kd], proj_b [H]
void fold_location_filter(const std::vector<float>& conv_w, const std::vector<float>& conv_b, const std::vector<float>& proj_w,
                          const std::vector<float>& proj_b, int H, int kd, int taps, std::vector<float>* w,
                          std::vector<float>* b) {
  for (int n = 0; n < H; ++n) {
    double bn = proj_b[n];
    for (int m = 0; m < kd; ++m) bn += (double)proj_w[(size_t)n * kd + m] * conv_b[m];
    (*b)[n] = (float)bn;
    for (int j = 0; j < taps; ++j) {
      double a = 0.0;
      for (int m = 0; m < kd; ++m) a += (double)proj_w[(size_t)n * kd + m] * conv_w[(size_t)m * taps + j];
      (*w)[(size_t)n * taps + j] = (float)a;
    }
  }
}

// The location term of the score (A.wloc [H][taps], A.bloc [H], A.bscore).  LocationAwareAttention: the folded filter, computed
// on the host from the weights as they lie on the device once the stream has drained.  Bahdanau (loc == nullptr): no
// location term and no score bias, a zero filter
struct LocW { const RawW *conv_w, *conv_b, *proj_w, *proj_b, *score_b; };
int pack_location_term(d2t_ctx* c, AttnW& A, const LocW* loc, int H, int kd, hipStream_t s) {
  if (!loc) {
    HIPCHK(c, hipMemsetAsync(A.wloc, 0, (size_t)H * A.taps * 4, s));
    HIPCHK(c, hipMemsetAsync(A.bloc, 0, (size_t)H * 4, s));
    A.bscore = 0.f;
    return D2T_OK;
  }
  std::vector<float> hcw((size_t)kd * A.taps), hcb(kd), hpw((size_t)H * kd), hpb(H), hsb(1), w((size_t)H * A.taps), b(H);
  HIPCHK(c, hipStreamSynchronize(s));
  HIPCHK(c, hipMemcpy(hcw.data(), loc->conv_w->p, hcw.size() * 4, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(hcb.data(), loc->conv_b->p, hcb.size() * 4, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(hpw.data(), loc->proj_w->p, hpw.size() * 4, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(hpb.data(), loc->proj_b->p, hpb.size() * 4, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(hsb.data(), loc->score_b->p, 4, hipMemcpyDeviceToHost));
  fold_location_filter(hcw, hcb, hpw, hpb, H, kd, A.taps, &w, &b);
  HIPCHK(c, hipMemcpy(A.wloc, w.data(), w.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(A.bloc, b.data(), b.size() * 4, hipMemcpyHostToDevice));
  A.bscore = hsb[0];
  return D2T_OK;
}

// Attention.__init__ (prediction_head/seq2seq.py:11-68) + LocationAwareAttention (attention1D.py:121-133,203-214) or
// BahdanauAttentionCell (attention1D.py:71-85: i2h without bias, h2h, score without bias), under the key prefix pp
int pack_attn_head(d2t_ctx* c, const std::string& pp, hipStream_t s) {
  const d2t_config& g = c->cfg;
  const int Hh = g.attn_hidden, V = g.vocab, taps = 2 * g.attn_kernel_size + 1, kd = g.attn_kernel_dim;
  const std::string ac = pp + "attention_cell.";
  AttnW& A = c->attn;
  A = AttnW{};
  A.taps = taps;
  int rc;
  const RawW *emb = nullptr, *qw, *qb, *sw, *wih, *whh, *bih, *bhh, *gw, *gb;
  LocW loc{};
  const bool bahdanau = g.attn_cell == D2T_ATTN_CELL_BAHDANAU, onehot = g.attn_onehot != 0;
  const int Ein = onehot ? V : Hh;  // width of the decoder-input part of rnn.weight_ih
  if (!onehot && (rc = need(c, pp + "embedding.weight", &emb, {V, Hh}))) return rc;
  if (bahdanau) {
    if ((rc = need(c, ac + "attn.h2h.weight", &qw, {Hh, Hh})) || (rc = need(c, ac + "attn.h2h.bias", &qb, {Hh})) ||
        (rc = get_lin(c, ac + "attn.i2h", &A.key, Hh, Hh, /*bias=*/false)) ||
        (rc = need(c, ac + "attn.score.weight", &sw, {1, Hh})))
      return rc;
  } else if ((rc = need(c, ac + "attn.loc_conv.weight", &loc.conv_w, {kd, 1, taps})) ||
             (rc = need(c, ac + "attn.loc_conv.bias", &loc.conv_b, {kd})) ||
             (rc = need(c, ac + "attn.loc_proj.weight", &loc.proj_w, {Hh, kd})) ||
             (rc = need(c, ac + "attn.loc_proj.bias", &loc.proj_b, {Hh})) ||
             (rc = need(c, ac + "attn.query_proj.weight", &qw, {Hh, Hh})) ||
             (rc = need(c, ac + "attn.query_proj.bias", &qb, {Hh})) ||
             (rc = get_lin(c, ac + "attn.key_proj", &A.key, Hh, Hh)) ||
             (rc = need(c, ac + "attn.score.weight", &sw, {1, Hh})) ||
             (rc = need(c, ac + "attn.score.bias", &loc.score_b, {1}))) {
    return rc;
  }
  if ((rc = need(c, ac + "rnn.weight_ih", &wih, {4 * Hh, Hh + Ein})) ||
      (rc = need(c, ac + "rnn.weight_hh", &whh, {4 * Hh, Hh})) || (rc = need(c, ac + "rnn.bias_ih", &bih, {4 * Hh})) ||
      (rc = need(c, ac + "rnn.bias_hh", &bhh, {4 * Hh})) || (rc = need(c, ac + "generator.weight", &gw, {V, Hh})) ||
      (rc = need(c, ac + "generator.bias", &gb, {V})))
    return rc;
  A.emb = emb ? emb->p : nullptr; A.bq = qb->p; A.wscore = sw->p; A.bg = gb->p;
  if ((rc = owned_alloc(c, &A.wq_t, (size_t)Hh * Hh)) || (rc = owned_alloc(c, &A.wloc, (size_t)Hh * taps)) ||
      (rc = owned_alloc(c, &A.bloc, (size_t)Hh)) || (rc = owned_alloc(c, &A.wx_t, (size_t)3 * Hh * 4 * Hh)) ||
      (rc = owned_alloc(c, &A.bx, (size_t)4 * Hh)) || (rc = owned_alloc(c, &A.wg_t, (size_t)Hh * V)))
    return rc;
  HIPCHK(c, launch_transpose_into(qw->p, Hh, Hh, A.wq_t, Hh, 0, s));
  if (!onehot) {
    HIPCHK(c, launch_transpose_into(wih->p, 4 * Hh, 2 * Hh, A.wx_t, 4 * Hh, 0, s));       // rows [ctx ; emb]
  } else {
    // one-hot decoder input (seq2seq.py:72-78): W_ih . [ctx ; onehot(tok)] = W_ih[:, :H] . ctx + W_ih[:, H + tok]; the
    // kernel keeps its [ctx ; emb ; h] layout with zero "emb" rows and adds row `tok` of the transposed tail of W_ih
    float* full;  // W_ih^T [H + V][4H]
    if ((rc = owned_alloc(c, &full, (size_t)(Hh + V) * 4 * Hh))) return rc;
    HIPCHK(c, launch_transpose_into(wih->p, 4 * Hh, Hh + V, full, 4 * Hh, 0, s));
    HIPCHK(c, hipMemcpyAsync(A.wx_t, full, (size_t)Hh * 4 * Hh * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(c, hipMemsetAsync(A.wx_t + (size_t)Hh * 4 * Hh, 0, (size_t)Hh * 4 * Hh * 4, s));
    A.tokgate = full + (size_t)Hh * 4 * Hh;
  }
  HIPCHK(c, launch_transpose_into(whh->p, 4 * Hh, Hh, A.wx_t, 4 * Hh, 2 * Hh, s));      // rows h
  HIPCHK(c, launch_add_rows(bih->p, bhh->p, A.bx, 4 * Hh, s));
  HIPCHK(c, launch_transpose_into(gw->p, V, Hh, A.wg_t, V, 0, s));
  if ((rc = pack_location_term(c, A, bahdanau ? nullptr : &loc, Hh, kd, s))) return rc;
  if (g.attn_enc_init) {
    const RawW *hw, *hb, *cw, *cb;
    if ((rc = need(c, pp + "proj_init_h.weight", &hw, {Hh, Hh})) || (rc = need(c, pp + "proj_init_h.bias", &hb, {Hh})) ||
        (rc = need(c, pp + "proj_init_c.weight", &cw, {Hh, Hh})) || (rc = need(c, pp + "proj_init_c.bias", &cb, {Hh})))
      return rc;
    if ((rc = owned_alloc(c, &A.wih_t, (size_t)Hh * Hh)) || (rc = owned_alloc(c, &A.wic_t, (size_t)Hh * Hh))) return rc;
    HIPCHK(c, launch_transpose_into(hw->p, Hh, Hh, A.wih_t, Hh, 0, s));
    HIPCHK(c, launch_transpose_into(cw->p, Hh, Hh, A.wic_t, Hh, 0, s));
    A.bih = hb->p; A.bic = cb->p;
  }
  return D2T_OK;
}

// [k][n] copy of a d x d projection [n][k] for the row kernels
int transposed_copy(d2t_ctx* c, const float* w, float** out, int d, hipStream_t s) {
  if (int rc = owned_alloc(c, out, (size_t)d * d)) return rc;
  HIPCHK(c, launch_transpose(w, *out, d, d, s));
  return D2T_OK;
}

// The transformer decoder (prediction_head/tfm.py:36-72), under the key prefix pp
int pack_tfm_head(d2t_ctx* c, const std::string& pp, hipStream_t s) {
  const d2t_config& g = c->cfg;
  const int d = g.dec_dim, V = g.vocab;
  const RawW *we, *pe;
  int rc;
  if ((rc = need(c, pp + "word_embed.weight", &we, {V, d})) || (rc = need(c, pp + "pos_enc.pe", &pe))) return rc;
  if (pe->shape.size() != 2 || pe->shape[1] != d || pe->shape[0] < g.max_seq_len + 2)
    return fail(c, D2T_EINVAL, "pos_enc.pe must be [>=%d,%d]", g.max_seq_len + 2, d);
  c->word_embed = we->p;
  c->word_pe = pe->p;
  c->word_pe_rows = (int)pe->shape[0];
  if ((rc = owned_alloc(c, &c->ckv_w, (size_t)g.dec_layers * 2 * d * d)) ||
      (rc = owned_alloc(c, &c->ckv_b, (size_t)g.dec_layers * 2 * d)))
    return rc;
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
    float* ckv_w = c->ckv_w + (size_t)i * 2 * d * d;  // this layer's rows of the stacked K | V projection
    float* ckv_b = c->ckv_b + (size_t)i * 2 * d;
    HIPCHK(c, launch_copy(ciw->p + (size_t)d * d, ckv_w, (size_t)2 * d * d, s));
    HIPCHK(c, launch_copy(cib->p + d, ckv_b, (size_t)2 * d, s));
    if ((rc = get_lin(c, l + "self_attn.out_proj", &dl.sa_out, d, d)) ||
        (rc = get_lin(c, l + "multihead_attn.out_proj", &dl.ca_out, d, d)) ||
        (rc = get_lin(c, l + "linear1", &dl.l1, g.dec_ff, d)) || (rc = get_lin(c, l + "linear2", &dl.l2, d, g.dec_ff)) ||
        (rc = get_ln(c, l + "norm1", &dl.n1, d)) || (rc = get_ln(c, l + "norm2", &dl.n2, d)) ||
        (rc = get_ln(c, l + "norm3", &dl.n3, d)))
      return rc;
    // absorbed cross-attention: W_k as stored, W_v transposed (read from the engine's stacked copy), b_v
    dl.ca_wk = ckv_w;
    dl.ca_bv = ckv_b + d;
    if ((rc = transposed_copy(c, dl.sa_out.w, &dl.sa_out_t, d, s)) || (rc = transposed_copy(c, dl.ca_q.w, &dl.ca_q_t, d, s)) ||
        (rc = transposed_copy(c, dl.ca_out.w, &dl.ca_out_t, d, s)) ||
        (rc = transposed_copy(c, ckv_w + (size_t)d * d, &dl.ca_v_t, d, s)))
      return rc;
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
  return D2T_OK;
}

}  // namespace

namespace eng {

hipError_t concat_k(const float* w1, const float* b1, int K1, const float* w2, const float* b2, int K2, int Co, float* w,
                    float* bias, uint16_t* w_hi, uint16_t* w_lo, hipStream_t s) {
  const size_t ld = (size_t)(K1 + K2) * 4;
  hipError_t e = hipMemcpy2DAsync(w, ld, w1, (size_t)K1 * 4, (size_t)K1 * 4, Co, hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess) e = hipMemcpy2DAsync(w + K1, ld, w2, (size_t)K2 * 4, (size_t)K2 * 4, Co, hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess) e = launch_add_rows(b1, b2, bias, Co, s);
  if (e == hipSuccess) e = launch_split_bf16(w, w_hi, w_lo, (size_t)Co * (K1 + K2), s);
  return e;
}

// fp16 hi / lo planes of a packed convolution weight (fp16x2 / mixed precision), created the first time a launch needs them:
// contexts that never leave split-bf16 (the default; training; fp32) do not pay their memory
int f16_planes(d2t_ctx* c, ConvW& w, hipStream_t s) {
  if (w.w_h16) return D2T_OK;
  if (!w.w || w.Cin % 32) return fail(c, D2T_ESTATE, "no fp16 planes for this layer");
  const size_t n = (size_t)w.Cout * w.KH * w.KW * w.Cin + (size_t)w.Cout * w.K2;
  uint16_t *qh, *ql;  // (the layer takes them only once both exist and are filled)
  int rc;
  if ((rc = owned_alloc(c, &qh, n)) || (rc = owned_alloc(c, &ql, n))) return rc;
  HIPCHK(c, launch_split_f16(w.w, qh, ql, n, s));
  w.w_h16 = qh;
  w.w_l16 = ql;
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

}  // namespace eng

extern "C" {

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
  eng::free_packed(c);
  const d2t_config& g = c->cfg;
  const bool vit = g.encoder == D2T_ENC_HYBRID_VIT, is_vgg = g.encoder == D2T_ENC_VGG_BILSTM || g.encoder == D2T_ENC_VGG;
  const bool has_lstm = g.encoder == D2T_ENC_VGG_BILSTM || g.encoder == D2T_ENC_RESNET_BILSTM;
  const std::string sm = "seqmodeler.SequenceModeling.", pp = "predicter.Prediction.";
  c->bb = vit ? sm + "patch_embed.backbone.ConvNet." : "featextractor.FeatureExtraction.ConvNet.";
  int rc;
  if ((rc = is_vgg ? pack_vgg(c, s) : pack_resnet(c, s))) return rc;
  if (has_lstm && g.proj_height && (rc = pack_proj_feat(c, s))) return rc;
  if (has_lstm && (rc = pack_bilstm(c, sm, s))) return rc;
  if (vit && (rc = pack_vit(c, sm, s))) return rc;
  if (has_lstm && g.decoder == D2T_DEC_TFM && g.dec_dim != g.bilstm_hidden)
    return fail(c, D2T_EINVAL, "decoder d_model must equal the BiLSTM hidden_size");
  if (!vit && !has_lstm && g.decoder == D2T_DEC_TFM && g.dec_dim != (is_vgg ? c->vgg[6].Cout : c->conv4_2.Cout))
    return fail(c, D2T_EINVAL, "decoder d_model must equal the backbone output_channel");
  if ((rc = g.decoder == D2T_DEC_ATTN ? pack_attn_head(c, pp, s) : pack_tfm_head(c, pp, s))) return rc;
  HIPCHK(c, hipStreamSynchronize(s));
  c->finalized = true;
  return D2T_OK;
}

}  // extern "C"
