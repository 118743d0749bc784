// The networks of the training step, built from the tape's operations (train.hip): the feature extractors, the
// sequence models and the two prediction heads, and the two entries that run them, d2t_train_forward / d2t_train_backward.
#include "train_tape.h"

namespace tape {

// GlobalContext.forward (addon_module/visual_attention.py:147-165, use_attn + fuse_add): the attention-pooled channel
// vector (gc_pool), ConvMLP (fc1 -> LayerNorm2d -> ReLU -> fc2) on it, added to every position (bcast_add)
int Tr::global_context(int in, const std::string& key, int* out) {
  const int C = st->t[in].cols;
  int ctx, h, y;
  RC(gc_pool(in, key + ".global_cxt", &ctx));
  const std::string m = key + ".bottleneck_add.";
  RC(linear(ctx, m + "fc1", C, C, 0, ACT_NONE, -1, &h));
  RC(layernorm(h, m + "norm", 1e-5f, &h));
  RC(relu(h, &h));
  RC(dropout(h, &h, 0.25f));  // ConvMLP's nn.Dropout(drop=0.25), hard-wired (visual_attention.py:86,94,100)
  RC(linear(h, m + "fc2", C, C, 0, ACT_NONE, -1, &y));
  return bcast_add(in, y, out);
}

int Tr::backbone(const float* img, int B, int H, int W, const std::string& p, int* out) {
  int x;
  RC(stem(img, B, c->cfg.in_channels, H, W, 32, p + "conv0_1", p + "bn0_1", &x));
  RC(conv_bn(x, p + "conv0_2", p + "bn0_2", 64, 3, 3, 1, 1, 1, 1, true, -1, &x));
  RC(pool(x, 2, 2, 0, 0, &x));
  const int chans[4] = {128, 256, 512, 512};
  auto stage = [&](int li) -> int {
    for (int i = 0; i < RESNET_LAYERS[li]; ++i) {
      const std::string bp = p + "layer" + std::to_string(li + 1) + "." + std::to_string(i);
      int t, r = x;
      RC(conv_bn(x, bp + ".conv1", bp + ".bn1", chans[li], 3, 3, 1, 1, 1, 1, true, -1, &t));
      if (find(c, bp + ".downsample.0.weight"))
        RC(conv_bn(x, bp + ".downsample.0", bp + ".downsample.1", chans[li], 1, 1, 1, 1, 0, 0, false, -1, &r));
      RC(conv_bn(t, bp + ".conv2", bp + ".bn2", chans[li], 3, 3, 1, 1, 1, 1, true, r, &x));
    }
    if (c->cfg.gcb)  // a GlobalContext block closes the stage (resnet.py:200-201): Sequential index = number of blocks
      RC(global_context(x, p + "layer" + std::to_string(li + 1) + "." + std::to_string(RESNET_LAYERS[li]), &x));
    return D2T_OK;
  };
  RC(stage(0));
  RC(conv_bn(x, p + "conv1", p + "bn1", 128, 3, 3, 1, 1, 1, 1, true, -1, &x));
  RC(pool(x, 2, 2, 0, 0, &x));
  RC(stage(1));
  RC(conv_bn(x, p + "conv2", p + "bn2", 256, 3, 3, 1, 1, 1, 1, true, -1, &x));
  RC(pool(x, 2, 1, 0, 1, &x));
  RC(stage(2));
  RC(conv_bn(x, p + "conv3", p + "bn3", 512, 3, 3, 1, 1, 1, 1, true, -1, &x));
  RC(stage(3));
  RC(conv_bn(x, p + "conv4_1", p + "bn4_1", 512, 2, 2, 2, 1, 0, 1, true, -1, &x));
  RC(conv_bn(x, p + "conv4_2", p + "bn4_2", 512, 2, 2, 1, 1, 0, 0, true, -1, &x));
  *out = x;
  return D2T_OK;
}

// VGG_FeatureExtractor.forward (feature_extractor/vgg.py:16-44): Conv2d(1, 64) + ReLU, pool, Conv2d(64, 128) + ReLU, pool,
// two convolutions + ReLU, (2,1) pool, two bias-free convolutions with BatchNorm + ReLU, (2,1) pool, a 2x2 convolution + ReLU
int Tr::vgg(const float* img, int B, int H, int W, const std::string& p, int* out) {
  int x;
  RC(stem(img, B, c->cfg.in_channels, H, W, 64, p + "0", "", &x));
  auto cr = [&](const char* key, const char* bn, int Cout, int k, int pad) -> int {
    RC(conv_bn(x, p + key, bn ? p + bn : std::string(), Cout, k, k, 1, 1, pad, pad, bn != nullptr, -1, &x));
    if (!bn) RC(relu(x, &x));
    return D2T_OK;
  };
  RC(pool(x, 2, 2, 0, 0, &x));
  RC(cr("3", nullptr, 128, 3, 1));
  RC(pool(x, 2, 2, 0, 0, &x));
  RC(cr("6", nullptr, 256, 3, 1));
  RC(cr("8", nullptr, 256, 3, 1));
  RC(pool(x, 2, 1, 0, 0, &x, 1));
  RC(cr("11", "12", 512, 3, 1));
  RC(cr("14", "15", 512, 3, 1));
  RC(pool(x, 2, 1, 0, 0, &x, 1));
  RC(cr("18", nullptr, 512, 2, 0));
  *out = x;
  return D2T_OK;
}

// BidirectionalLSTM (seq_modeling/bilstm.py:14-24): nn.LSTM(bidirectional, batch_first) + Linear(2H -> H)
int Tr::bilstm_layer(int in, int layer, const std::string& key, int B, int T, int* out) {
  const int Hh = c->cfg.bilstm_hidden;
  int rec;
  RC(bilstm(in, layer, key + "rnn.", B, T, &rec));
  return linear(rec, key + "linear", Hh, 2 * Hh, 0, ACT_NONE, -1, out);
}

// ViTEncoderV3 on top of the backbone (vit_encoder.py:249-268, patchembed.py:115-141)
int Tr::vit(int feat, const std::string& p, int* out, float* into) {
  const d2t_config& g = c->cfg;
  const TT f = st->t[feat];
  const int D = g.vit_dim, gh = (f.H + g.patch_h - 1) / g.patch_h, gw = (f.W + g.patch_w - 1) / g.patch_w, n = gh * gw;
  // (memories beyond about 600 tokens: the training attention kernels read K / V from global memory, train_attn.hip GKV)
  if (n + 1 > 4096) return fail(c, D2T_EINVAL, "training step: memory length %d > 4096 unsupported", n + 1);
  int patch, x;
  // zero padding right / bottom = out-of-image taps of the strided convolution
  RC(conv_bn(feat, p + "patch_embed.proj", "", D, g.patch_h, g.patch_w, g.patch_h, g.patch_w, 0, 0, false, -1, &patch, gh, gw));
  RC(tokens(patch, p, gh, gw, &x));
  const int rows_b = n + 1;
  for (int i = 0; i < g.vit_depth; ++i) {
    const std::string bp = p + "blocks." + std::to_string(i) + ".";
    int h, qkv, a, x1, h2, u, ge, x2;
    RC(layernorm(x, bp + "norm1", 1e-6f, &h));
    RC(linear(h, bp + "attn.qkv", 3 * D, D, 0, ACT_NONE, -1, &qkv));
    RC(attention(qkv, 0, qkv, D, 2 * D, f.B, rows_b, rows_b, g.vit_heads, D / g.vit_heads, 0, nullptr, &a));
    RC(linear(a, bp + "attn.proj", D, D, 0, ACT_NONE, x, &x1));
    RC(layernorm(x1, bp + "norm2", 1e-6f, &h2));
    RC(linear(h2, bp + "mlp.fc1", 4 * D, D, 0, ACT_NONE, -1, &u));
    RC(gelu(u, &ge));
    RC(linear(ge, bp + "mlp.fc2", D, 4 * D, 0, ACT_NONE, x1, &x2));
    x = x2;
  }
  return layernorm(x, p + "norm", 1e-6f, out, into);
}

// out = res + dropout(linear(in)) of a post-norm decoder layer: without dropout the residual add rides in the GEMM epilogue
int Tr::linear_res(int in, const std::string& key, int N, int K, int res, int* out) {
  if (st->drop_p <= 0.f) return linear(in, key, N, K, 0, ACT_NONE, res, out);
  int z, d;
  RC(linear(in, key, N, K, 0, ACT_NONE, -1, &z));
  RC(dropout(z, &d));
  return add(res, d, out);
}
// TransformerPrediction teacher-forced pass (tfm.py:103-118), post-norm nn.TransformerDecoderLayer
int Tr::decoder(int mem, const int64_t* tgt, int B, int L, const std::string& p, float* logits, int* out) {
  const d2t_config& g = c->cfg;
  const int D = g.dec_dim, heads = g.dec_heads, hd = D / heads, T = (int)(st->t[mem].rows / B);
  int x;
  RC(embed(tgt, B, L, p, &x));
  const bool dp = st->drop_p > 0.f;
  for (int l = 0; l < g.dec_layers; ++l) {
    const std::string lp = p + "model.layers." + std::to_string(l) + ".";
    int qkv, a, y1, x1, q2, kv, a2, y2, x2, f, fd, y3;
    RC(linear(x, lp + "self_attn.in_proj", 3 * D, D, 0, ACT_NONE, -1, &qkv));
    RC(attention(qkv, 0, qkv, D, 2 * D, B, L, L, heads, hd, 1, tgt, &a, dp));
    RC(linear_res(a, lp + "self_attn.out_proj", D, D, x, &y1));  // x + dropout1(self_attn(x))
    RC(layernorm(y1, lp + "norm1", 1e-5f, &x1));
    RC(linear(x1, lp + "multihead_attn.in_proj", D, D, 0, ACT_NONE, -1, &q2));
    RC(linear(mem, lp + "multihead_attn.in_proj", 2 * D, D, D, ACT_NONE, -1, &kv));
    RC(attention(q2, 0, kv, 0, D, B, L, T, heads, hd, 0, nullptr, &a2, dp));
    RC(linear_res(a2, lp + "multihead_attn.out_proj", D, D, x1, &y2));
    RC(layernorm(y2, lp + "norm2", 1e-5f, &x2));
    RC(linear(x2, lp + "linear1", g.dec_ff, D, 0, ACT_RELU, -1, &f));
    RC(dropout(f, &fd));
    RC(linear_res(fd, lp + "linear2", D, g.dec_ff, x2, &y3));  // x + dropout3(linear2(dropout(relu(linear1(x)))))
    RC(layernorm(y3, lp + "norm3", 1e-5f, &x));
  }
  return linear(x, p + "proj", g.vocab, D, 0, ACT_NONE, -1, out, logits);
}

// The LSTM-attention heads (Attn / Attnv2): the key projection of the memory, then the teacher-forced loop (lstm_head)
int Tr::lstm_decoder(int mem, const int64_t* tgt, int B, int S, float* logits, int* out) {
  const int Hh = c->cfg.attn_hidden;
  if (!c->finalized) return fail(c, D2T_ESTATE, "the Attn training step needs finalized weights");
  // key_proj of the location-aware cell, i2h (no bias) of the Bahdanau cell (attention1D.py:77-82)
  const bool bahdanau = c->cfg.attn_cell == D2T_ATTN_CELL_BAHDANAU;
  int kp;
  RC(linear(mem, std::string("predicter.Prediction.attention_cell.attn.") + (bahdanau ? "i2h" : "key_proj"), Hh, Hh, 0, ACT_NONE, -1,
            &kp, nullptr, !bahdanau));
  return lstm_head(mem, kp, tgt, B, S, logits, out);
}

}  // namespace tape

using tape::Tr;

extern "C" {

int d2t_train_forward(d2t_ctx* c, const float* image, int32_t B, int32_t H, int32_t W, const int64_t* tgt, int32_t L,
                      float* logits, d2t_stream stream) {
  DevGuard dg_(c);
  if (!c || !image || !tgt || !logits || B < 1 || H < 1 || W < 1 || L < 1) return fail(c, D2T_EINVAL, "bad argument");
  if (int rc = check_dev_ptr(c, image, "image")) return rc;
  if (int rc = check_dev_ptr(c, logits, "logits")) return rc;
  const d2t_config& g = c->cfg;
  const bool lstm = g.decoder == D2T_DEC_ATTN;
  const bool lstm_enc = g.encoder == D2T_ENC_VGG_BILSTM || g.encoder == D2T_ENC_RESNET_BILSTM;
  const bool flat_enc = g.encoder == D2T_ENC_RESNET || g.encoder == D2T_ENC_VGG;
  if (lstm && flat_enc) return fail(c, D2T_ESTATE, "the Attn training step needs the HybridViT or a BiLSTM encoder");
  if (lstm && L != g.batch_max_length + 1) return fail(c, D2T_EINVAL, "the Attn head trains on batch_max_length + 1 = %d steps", g.batch_max_length + 1);
  if (!lstm && L > g.max_seq_len + 1) return fail(c, D2T_EINVAL, "teacher sequence longer than max_seq_len + 1");
  if (lstm_enc && g.proj_height) {  // refused before anything is launched, as d2t_encode does
    int32_t fh = 0;
    if (d2t_encoder_shape(c, H, W, nullptr, nullptr, &fh, nullptr, nullptr, nullptr) || fh != 3)
      return fail(c, D2T_EINVAL, "mean_height False: proj_feat reads a feature map of height 3 (64-pixel crops), this crop gives "
                  "height %d", fh);
  }
  if (!c->train) c->train = new d2t_train_state();
  d2t_train_state* st = c->train;
  st->tape.reset();
  st->t.clear();
  st->nodes.clear();
  st->have_forward = false;
  st->masks.clear();
  st->drop_site = 0;
  ++st->drop_calls;
  st->tgt = tgt; st->image = image; st->B = B; st->H = H; st->W = W; st->L = L;
  Tr tr{c, st, (hipStream_t)stream};
  int feat, mem, out;
  if (g.encoder == D2T_ENC_HYBRID_VIT) {
    const std::string sp = "seqmodeler.SequenceModeling.";
    RC(tr.backbone(image, B, H, W, sp + "patch_embed.backbone.ConvNet.", &feat));
    RC(tr.vit(feat, sp, &mem, nullptr));
  } else if (lstm_enc) {  // VGG | ResNet -> mean over the height | proj_feat -> 2 x BidirectionalLSTM (build_feat.py:50-61, build_seq.py)
    const std::string fp = "featextractor.FeatureExtraction.ConvNet.";
    if (g.encoder == D2T_ENC_VGG_BILSTM) RC(tr.vgg(image, B, H, W, fp, &feat));
    else RC(tr.backbone(image, B, H, W, fp, &feat));
    int seq;
    if (g.proj_height) {
      // mean_height False: Linear(3 * C -> C) over the [b, w, c * h] flattening = a (3, 1) convolution over the NHWC map whose
      // OIHW filter is the weight as it lies in memory (engine_weights.hip pack_proj_feat); so is its gradient
      RC(tr.conv_bn(feat, "featextractor.proj_feat", "", g.backbone_out, 3, 1, 1, 1, 0, 0, false, -1, &seq));
    } else {
      RC(tr.mean_h(feat, &seq));
    }
    const int T = st->t[feat].W;
    RC(tr.bilstm_layer(seq, 0, "seqmodeler.SequenceModeling.0.", B, T, &seq));
    RC(tr.bilstm_layer(seq, 1, "seqmodeler.SequenceModeling.1.", B, T, &mem));
  } else {  // Feat=ResNet | VGG, Seq=None: + PositionalEncoding2D, [B,C,H,W] -> [B,HW,C] (already the NHWC row layout)
    const std::string fp = "featextractor.FeatureExtraction.ConvNet.";
    if (g.encoder == D2T_ENC_VGG) RC(tr.vgg(image, B, H, W, fp, &feat));
    else RC(tr.backbone(image, B, H, W, fp, &feat));
    const tape::TT f = st->t[feat];
    const float* pe;
    RC(d2t_internal_pe2d(c, f.H, f.W, f.cols, (hipStream_t)stream, &pe));
    RC(tr.add_const(feat, pe, &mem));
  }
  if (lstm) RC(tr.lstm_decoder(mem, tgt, B, L, logits, &out));
  else RC(tr.decoder(mem, tgt, B, L, "predicter.Prediction.", logits, &out));
  st->logits_id = out;
  st->have_forward = true;
  return D2T_OK;
}

int d2t_train_backward(d2t_ctx* c, const float* dlogits, d2t_stream stream) {
  DevGuard dg_(c);
  if (!c || !dlogits) return fail(c, D2T_EINVAL, "bad argument");
  d2t_train_state* st = c->train;
  if (!st || !st->have_forward) return fail(c, D2T_ESTATE, "d2t_train_backward without a preceding d2t_train_forward");
  Tr tr{c, st, (hipStream_t)stream};
  st->t[st->logits_id].grad = const_cast<float*>(dlogits);
  st->have_forward = false;  // the tape is consumed (the attention probabilities are overwritten)
  st->touched.clear();
  return tr.backward();
}

}  // extern "C"
