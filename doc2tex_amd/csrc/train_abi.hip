// The C entries of the training step other than the forward / backward pair (train_models.hip): gradients and weights in
// and out of the engine, dropout and teacher-forcing controls, what the last forward saved (masks, alignments, decisions),
// the fused cross-entropy, and the op-level test entries.
#include "train_tape.h"

using namespace tape;

extern "C" {

int d2t_train_grad(d2t_ctx* c, const char* name, float* dst, int64_t numel, d2t_stream stream) {
  DevGuard dg_(c);
  if (!c || !name || !dst) return fail(c, D2T_EINVAL, "bad argument");
  d2t_train_state* st = c->train;
  if (!st) return fail(c, D2T_ESTATE, "no training step has run");
  auto it = st->grads.find(name);
  if (it == st->grads.end()) return fail(c, D2T_ESTATE, "no gradient for '%s'", name);
  const RawW* r = find(c, name);
  if (!r || (int64_t)r->numel != numel) return fail(c, D2T_EINVAL, "gradient '%s': size mismatch", name);
  // ordered after the backward kernels that produce this gradient, whichever stream `stream` is
  HIPCHK(c, hipStreamWaitEvent((hipStream_t)stream, st->ready[name], 0));
  HIPCHK(c, hipMemcpyAsync(dst, it->second, (size_t)numel * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return D2T_OK;
}

// launch one multi-copy kernel over `table` on stream s; the table travels through a pinned block of the gather ring
static int run_copy_table(d2t_ctx* c, d2t_train_state* st, const std::vector<CopyChunk>& table, hipStream_t s) {
  if (table.empty()) return D2T_OK;
  const size_t bytes = table.size() * sizeof(CopyChunk);
  d2t_train_state::GatherStage& g = st->gather[st->gather_calls++ & 3];
  if (g.pending) {
    HIPCHK(c, hipEventSynchronize(g.ev));
    g.pending = false;
  }
  if (bytes > g.cap) {
    if (g.h) { HIPCHK(c, hipHostFree(g.h)); HIPCHK(c, hipFree(g.d)); }
    g.h = g.d = nullptr;
    g.cap = 0;
    HIPCHK(c, hipHostMalloc(&g.h, bytes * 2, hipHostMallocDefault));
    HIPCHK(c, hipMalloc(&g.d, bytes * 2));
    g.cap = bytes * 2;
    if (!g.ev) HIPCHK(c, hipEventCreateWithFlags(&g.ev, hipEventDisableTiming));
  }
  memcpy(g.h, table.data(), bytes);
  HIPCHK(c, hipMemcpyAsync(g.d, g.h, bytes, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipEventRecord(g.ev, s));
  g.pending = true;
  HIPCHK(c, launch_multi_copy(reinterpret_cast<const CopyChunk*>(g.d), (int)table.size(), s));
  return D2T_OK;
}

int d2t_train_gather(d2t_ctx* c, int32_t source, int32_t n, const char* const* names, const int64_t* offsets,
                     const int64_t* numels, float* flat, d2t_stream stream) {
  DevGuard dg_(c);
  if (!c || n < 0 || (n && (!names || !offsets || !numels || !flat)) || (source != 0 && source != 1)) return fail(c, D2T_EINVAL, "bad argument");
  d2t_train_state* st = c->train;
  if (source == 0 && !st) return fail(c, D2T_ESTATE, "no training step has run");
  if (!st) st = c->train = new d2t_train_state();
  if (int rc = check_dev_ptr(c, flat, "flat")) return rc;
  hipStream_t s = (hipStream_t)stream;
  constexpr long long CHUNK = 1 << 16;  // floats per block
  std::vector<CopyChunk> table;
  for (int i = 0; i < n; ++i) {
    const RawW* r = find(c, names[i]);
    if (!r || (int64_t)r->numel != numels[i]) return fail(c, D2T_EINVAL, "tensor '%s': unknown or size mismatch", names[i]);
    const float* src = r->p;
    if (source == 0) {
      auto it = st->grads.find(names[i]);
      if (it == st->grads.end()) return fail(c, D2T_ESTATE, "no gradient for '%s'", names[i]);
      src = it->second;
      HIPCHK(c, hipStreamWaitEvent(s, st->ready[names[i]], 0));  // (the same stream as the backward: no-ops)
    }
    for (long long o = 0; o < numels[i]; o += CHUNK)
      table.push_back(CopyChunk{src + o, flat + offsets[i] + o, std::min<long long>(CHUNK, numels[i] - o)});
  }
  return run_copy_table(c, st, table, s);
}

/* Refresh the engine's copies of tensors that are already loaded (same names, same sizes) from device memory, all in one
 * kernel: what the step after optimizer.step() needs -- every parameter changed, and one d2t_load_weight per tensor
 * is ~400 four-microsecond device copies.  Anything not loaded yet (or resized) is an error: use d2t_load_weight. */
int d2t_reload_weights(d2t_ctx* c, int32_t n, const char* const* names, const float* const* srcs, const int64_t* numels,
                       d2t_stream stream) {
  DevGuard dg_(c);
  if (!c || n < 0 || (n && (!names || !srcs || !numels))) return fail(c, D2T_EINVAL, "bad argument");
  if (!c->train) c->train = new d2t_train_state();
  hipStream_t s = (hipStream_t)stream;
  constexpr long long CHUNK = 1 << 16;
  std::vector<CopyChunk> table;
  for (int i = 0; i < n; ++i) {
    auto it = c->raw.find(names[i]);
    if (it == c->raw.end() || !it->second.p || (int64_t)it->second.numel != numels[i])
      return fail(c, D2T_EINVAL, "tensor '%s': not loaded or size mismatch", names[i]);
    if (int rc = check_dev_ptr(c, srcs[i], names[i])) return rc;
    for (long long o = 0; o < numels[i]; o += CHUNK)
      table.push_back(CopyChunk{srcs[i] + o, it->second.p + o, std::min<long long>(CHUNK, numels[i] - o)});
  }
  return run_copy_table(c, c->train, table, s);
}

int d2t_read_weight(d2t_ctx* c, const char* name, float* dst, int64_t numel, d2t_stream stream) {
  DevGuard dg_(c);
  if (!c || !name || !dst) return fail(c, D2T_EINVAL, "bad argument");
  const RawW* r = find(c, name);
  if (!r) return fail(c, D2T_ESTATE, "unknown tensor '%s'", name);
  if ((int64_t)r->numel != numel) return fail(c, D2T_EINVAL, "tensor '%s': size mismatch", name);
  HIPCHK(c, hipMemcpyAsync(dst, r->p, (size_t)numel * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return D2T_OK;
}

// where d2t_read_weight copies from: the fused optimizer writes the stepped parameter here as well (optim.hip)
int d2t_weight_ptr(d2t_ctx* c, const char* name, float** ptr_out, int64_t* numel_out) {
  if (!c || !name || !ptr_out || !numel_out) return fail(c, D2T_EINVAL, "bad argument");
  const RawW* r = find(c, name);
  if (!r || !r->p) return fail(c, D2T_ESTATE, "unknown tensor '%s'", name);
  *ptr_out = r->p;
  *numel_out = (int64_t)r->numel;
  return D2T_OK;
}

int d2t_train_set_dropout(d2t_ctx* c, float p, uint64_t seed) {
  DevGuard dg_(c);
  if (!c || !(p >= 0.f) || p >= 1.f) return fail(c, D2T_EINVAL, "dropout probability must be in [0, 1)");
  if (!c->train) c->train = new d2t_train_state();
  if (c->train->drop_seed != seed) c->train->drop_calls = 0;
  c->train->drop_p = p;
  c->train->drop_seed = seed;
  return D2T_OK;
}

int d2t_train_set_teacher_flags(d2t_ctx* c, const uint8_t* flags, int32_t n) {
  DevGuard dg_(c);
  if (!c || n < 0 || (n > 0 && !flags)) return fail(c, D2T_EINVAL, "bad argument");
  if (!c->train) c->train = new d2t_train_state();
  c->train->teacher_flags.assign(flags, flags + n);
  return D2T_OK;
}

int d2t_train_read_mask(d2t_ctx* c, int32_t index, uint8_t* dst, int64_t numel, d2t_stream stream) {
  DevGuard dg_(c);
  if (!c || !dst) return fail(c, D2T_EINVAL, "bad argument");
  d2t_train_state* st = c->train;
  if (!st || index < 0 || (size_t)index >= st->masks.size()) return fail(c, D2T_EINVAL, "no dropout mask %d", index);
  if ((int64_t)st->masks[index].second != numel) return fail(c, D2T_EINVAL, "mask %d has %zu elements", index, st->masks[index].second);
  HIPCHK(c, hipMemcpyAsync(dst, st->masks[index].first, (size_t)numel, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return D2T_OK;
}

// The alignments the last training forward saved for its backward pass (LSTM-attention heads): [B][S][Tk].
int d2t_train_read_attn_alpha(d2t_ctx* c, float* dst, int64_t numel, d2t_stream stream) {
  DevGuard dg_(c);
  if (!c || !dst) return fail(c, D2T_EINVAL, "bad argument");
  if (c->cfg.decoder != D2T_DEC_ATTN) return fail(c, D2T_ESTATE, "the TFM head has no alignment maps");
  d2t_train_state* st = c->train;
  if (!st || !st->have_forward) return fail(c, D2T_ESTATE, "no training forward to read the alignments of");
  for (const Node& n : st->nodes) {
    if (n.kind != N_LSTM) continue;
    const int64_t want = (int64_t)n.lstm.B * n.lstm.S * (n.lstm.T - n.lstm.key_off);
    if (numel != want) return fail(c, D2T_EINVAL, "the saved alignments have %lld elements, not %lld", (long long)want, (long long)numel);
    HIPCHK(c, hipMemcpyAsync(dst, n.lstm.alpha, (size_t)numel * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return D2T_OK;
  }
  return fail(c, D2T_ESTATE, "the last training forward ran no LSTM-attention decoder");
}

int d2t_train_mask_count(d2t_ctx* c) { return c && c->train ? (int)c->train->masks.size() : 0; }

// The discrete decisions of the last training forward, in network order: one entry per ReLU (convolution + BatchNorm
// [+ residual] + ReLU nodes, decoder linear1) and per max-pool.  A test replays them in the oracle (ReLU -> multiply by the
// keep mask, max-pool -> gather of the recorded window element), which makes oracle and engine evaluate the SAME smooth
// function: gradients then agree to rounding everywhere, with no "a tie may have flipped" allowance.  (Which nodes are
// decisions: Node::is_decision.)
int d2t_train_decision_count(d2t_ctx* c) {
  if (!c || !c->train) return 0;
  int k = 0;
  for (const Node& n : c->train->nodes) k += n.is_decision();
  return k;
}

// index-th decision: is_pool_out = 1 for a max-pool (bytes = window element kh*2+kw per output element, NHWC), 0 for a
// ReLU keep mask (bytes = y > 0 per element, rows x cols); numel_out = its element count.  dst may be NULL (query only).
int d2t_train_read_decision(d2t_ctx* c, int32_t index, uint8_t* dst, int64_t numel, int32_t* is_pool_out, int64_t* numel_out,
                            d2t_stream stream) {
  DevGuard dg_(c);
  if (!c || !c->train) return fail(c, D2T_ESTATE, "no training forward has run");
  d2t_train_state* st = c->train;
  int k = 0;
  for (const Node& n : st->nodes) {
    if (!n.is_decision()) continue;
    if (k++ != index) continue;
    const TT& y = st->t[n.out];
    const int64_t ne = (int64_t)y.rows * y.cols;
    if (is_pool_out) *is_pool_out = n.kind == N_POOL;
    if (numel_out) *numel_out = ne;
    if (!dst) return D2T_OK;
    if (numel != ne) return fail(c, D2T_EINVAL, "decision %d has %lld elements", index, (long long)ne);
    if (n.kind == N_POOL) {
      const TT& x = st->t[n.in];
      HIPCHK(c, launch_pool_argmax(x.p, dst, x.B, x.H, x.W, x.cols, n.pool.SH, n.pool.SW, n.pool.PH, n.pool.PW, (hipStream_t)stream, n.pool.KW));
    } else {
      HIPCHK(c, launch_relu_mask(y.p, dst, (size_t)ne, (hipStream_t)stream));
    }
    return D2T_OK;
  }
  return fail(c, D2T_EINVAL, "no decision %d", index);
}

void d2t_train_release(d2t_ctx* c) {
  DevGuard dg_(c);
  if (c && c->train) {
    hipDeviceSynchronize();
    delete c->train;
    c->train = nullptr;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Op-level test entry points: ONE node of the training tape, forward + backward, on caller tensors (row-major
// [rows][cols], NHWC maps).  They drive exactly the builders / backward functions the full step uses (a throw-away
// context holds the operands under fake keys), so tests/test_ops_gpu.py can hold every backward kernel -- data gradients,
// weight gradients in both arithmetic modes, BatchNorm / LayerNorm / attention / max-pool backward -- against float64
// torch autograd one op at a time.  Synchronous; not on any hot path.
// ---------------------------------------------------------------------------------------------------------------------
namespace {
struct OpCtx {
  d2t_ctx c;
  d2t_train_state st;
  Tr tr;
  OpCtx(int bf16x3, hipStream_t s) : tr{&c, &st, s} {
    c.conv_bf16x3 = bf16x3 != 0;
    hipGetDevice(&c.device);
    if (hipMalloc(&c.zero_page, 256) == hipSuccess) hipMemset(c.zero_page, 0, 256);  // out-of-image taps of the LDS-DMA kernels
  }
  ~OpCtx() {
    if (c.zero_page) hipFree(c.zero_page);
    c.zero_page = nullptr;
  }
  void put(const char* key, const float* p, std::vector<int64_t> shape) {
    RawW r;
    r.p = const_cast<float*>(p);
    r.shape = shape;
    r.numel = 1;
    for (auto v : shape) r.numel *= (size_t)v;
    c.raw[key] = r;
  }
  int out(float* dst, const float* src, size_t n) {
    if (!dst) return D2T_OK;
    if (!src) return hipMemsetAsync(dst, 0, n * 4, tr.s) == hipSuccess ? D2T_OK : D2T_EHIP;
    return hipMemcpyAsync(dst, src, n * 4, hipMemcpyDeviceToDevice, tr.s) == hipSuccess ? D2T_OK : D2T_EHIP;
  }
  int grad(float* dst, const char* key, size_t n) {
    auto it = st.grads.find(key);
    return out(dst, it == st.grads.end() ? nullptr : it->second, n);
  }
  int finish(int rc) {
    hipStreamSynchronize(tr.s);
    c.raw.clear();  // caller memory: nothing to free
    return rc;
  }
};
}  // namespace

// Fused cross-entropy, reduction 'none' (the criterion of engine/training.py:50-53): no context needed.
int d2t_ce_forward(const float* logits, const int64_t* target, float* loss, float* lse, int32_t rows, int32_t V,
                   int64_t ignore_index, d2t_stream stream) {
  if (!logits || !target || !loss || !lse || rows < 0 || V < 1) return D2T_EINVAL;
  return launch_ce_fwd(logits, target, loss, lse, rows, V, ignore_index, (hipStream_t)stream) == hipSuccess ? D2T_OK : D2T_EHIP;
}
int d2t_ce_backward(const float* logits, const int64_t* target, const float* lse, const float* dloss, float* dlogits,
                    int32_t rows, int32_t V, int64_t ignore_index, d2t_stream stream) {
  if (!logits || !target || !lse || !dloss || !dlogits || rows < 0 || V < 1) return D2T_EINVAL;
  return launch_ce_bwd(logits, target, lse, dloss, dlogits, rows, V, ignore_index, (hipStream_t)stream) == hipSuccess ? D2T_OK : D2T_EHIP;
}
// The same with class weights and / or label smoothing (nn.CrossEntropyLoss(weight, label_smoothing)), and the reference's
// LabelSmoothingLoss (modules/loss/labelsmoothing.py): include/d2t.h.
int d2t_ce_smooth_forward(const float* logits, const int64_t* target, const float* weight, float* loss, float* lse, float* mass,
                          int32_t rows, int32_t V, int64_t ignore_index, float on, float off, int32_t mode, int64_t pad_index,
                          d2t_stream stream) {
  if (!logits || !target || !loss || !lse || !mass || rows < 0 || V < 1) return D2T_EINVAL;
  if ((mode != D2T_CE_TORCH && mode != D2T_CE_REFERENCE) || (mode == D2T_CE_REFERENCE && weight)) return D2T_EINVAL;
  return launch_ce_smooth_fwd(logits, target, weight, loss, lse, mass, rows, V, ignore_index, on, off, mode == D2T_CE_REFERENCE,
                              pad_index, (hipStream_t)stream) == hipSuccess ? D2T_OK : D2T_EHIP;
}
int d2t_ce_smooth_backward(const float* logits, const int64_t* target, const float* weight, const float* lse, const float* mass,
                           const float* dloss, float* dlogits, int32_t rows, int32_t V, int64_t ignore_index, float on,
                           float off, int32_t mode, int64_t pad_index, d2t_stream stream) {
  if (!logits || !target || !lse || !mass || !dloss || !dlogits || rows < 0 || V < 1) return D2T_EINVAL;
  if ((mode != D2T_CE_TORCH && mode != D2T_CE_REFERENCE) || (mode == D2T_CE_REFERENCE && weight)) return D2T_EINVAL;
  return launch_ce_smooth_bwd(logits, target, weight, lse, mass, dloss, dlogits, rows, V, ignore_index, on, off,
                              mode == D2T_CE_REFERENCE, pad_index, (hipStream_t)stream) == hipSuccess ? D2T_OK : D2T_EHIP;
}

int d2t_op_train_conv(const float* x, const float* w, const float* bias, const float* gamma, const float* beta,
                      const float* residual, const float* dy, float* y, float* dx, float* dw, float* dbias,
                      float* dgamma, float* dbeta, float* dres, int32_t B, int32_t H, int32_t W, int32_t Cin,
                      int32_t Cout, int32_t KH, int32_t KW, int32_t SH, int32_t SW, int32_t PH, int32_t PW, int32_t relu,
                      int32_t bf16x3, d2t_stream stream) {
  if (!x || !w || !dy || (gamma && !beta) || (!gamma && !bias && Cin != 1 && Cin != 3) || SH < 1 || SW < 1) return D2T_EINVAL;
  if (Cin != 1 && Cin != 3 && Cin % 32) return D2T_EINVAL;
  OpCtx o(bf16x3, (hipStream_t)stream);
  Tr& tr = o.tr;
  o.put("w.weight", w, {Cout, Cin, KH, KW});
  if (bias) o.put("w.bias", bias, {Cout});
  float *rm = nullptr, *rv = nullptr;
  if (gamma) {
    o.put("bn.weight", gamma, {Cout});
    o.put("bn.bias", beta, {Cout});
    RC(tr.zeros(&rm, Cout));
    RC(tr.zeros(&rv, Cout));
    o.put("bn.running_mean", rm, {Cout});
    o.put("bn.running_var", rv, {Cout});
  }
  int xin = -1, res = -1, out = -1;
  auto run = [&]() -> int {
    if (Cin == 1 || Cin == 3) {  // the stem: 3x3, stride 1, pad 1, BatchNorm + ReLU (resnet.py:205-207); x is the image, NCHW planar
      if (KH != 3 || KW != 3 || SH != 1 || SW != 1 || PH != 1 || PW != 1 || !gamma || residual || !relu || Cout != 32)
        return fail(&o.c, D2T_EINVAL, "stem geometry");
      o.st.image = x; o.st.B = B; o.st.H = H; o.st.W = W;
      RC(tr.stem(x, B, Cin, H, W, Cout, "w", "bn", &out));
    } else {
      RC(tr.new_tensor((long long)B * H * W, Cin, &xin, B, H, W, const_cast<float*>(x)));
      const int OH = (H + 2 * PH - KH) / SH + 1, OW = (W + 2 * PW - KW) / SW + 1;
      if (residual) RC(tr.new_tensor((long long)B * OH * OW, Cout, &res, B, OH, OW, const_cast<float*>(residual)));
      RC(tr.conv_bn(xin, "w", gamma ? "bn" : "", Cout, KH, KW, SH, SW, PH, PW, relu != 0, res, &out));
    }
    const TT yo = o.st.t[out];
    RC(o.out(y, yo.p, (size_t)yo.rows * yo.cols));
    o.st.t[out].grad = const_cast<float*>(dy);
    RC(tr.backward());
    if (xin >= 0) RC(o.out(dx, o.st.t[xin].grad, (size_t)B * H * W * Cin));
    if (res >= 0) RC(o.out(dres, o.st.t[res].grad, (size_t)yo.rows * yo.cols));
    RC(o.grad(dw, "w.weight", (size_t)Cout * Cin * KH * KW));
    if (bias && !gamma) RC(o.grad(dbias, "w.bias", Cout));
    if (gamma) { RC(o.grad(dgamma, "bn.weight", Cout)); RC(o.grad(dbeta, "bn.bias", Cout)); }
    return D2T_OK;
  };
  return o.finish(run());
}

int d2t_op_train_linear(const float* x, const float* w, const float* bias, const float* residual, const float* dy, float* y,
                        float* dx, float* dw, float* dbias, float* dres, int32_t M, int32_t K, int32_t N, int32_t relu,
                        int32_t bf16x3, d2t_stream stream) {
  if (!x || !w || !bias || !dy || K % 32) return D2T_EINVAL;
  OpCtx o(bf16x3, (hipStream_t)stream);
  Tr& tr = o.tr;
  o.put("l.weight", w, {N, K});
  o.put("l.bias", bias, {N});
  auto run = [&]() -> int {
    int xin, res = -1, out;
    RC(tr.new_tensor(M, K, &xin, 0, 0, 0, const_cast<float*>(x)));
    if (residual) RC(tr.new_tensor(M, N, &res, 0, 0, 0, const_cast<float*>(residual)));
    RC(tr.linear(xin, "l", N, K, 0, relu ? ACT_RELU : ACT_NONE, res, &out));
    RC(o.out(y, o.st.t[out].p, (size_t)M * N));
    o.st.t[out].grad = const_cast<float*>(dy);
    RC(tr.backward());
    RC(o.out(dx, o.st.t[xin].grad, (size_t)M * K));
    if (res >= 0) RC(o.out(dres, o.st.t[res].grad, (size_t)M * N));
    RC(o.grad(dw, "l.weight", (size_t)N * K));
    RC(o.grad(dbias, "l.bias", N));
    return D2T_OK;
  };
  return o.finish(run());
}

int d2t_op_train_layernorm(const float* x, const float* gamma, const float* beta, const float* dy, float* y, float* dx,
                           float* dgamma, float* dbeta, int32_t rows, int32_t D, float eps, d2t_stream stream) {
  if (!x || !gamma || !beta || !dy) return D2T_EINVAL;
  OpCtx o(0, (hipStream_t)stream);
  Tr& tr = o.tr;
  o.put("n.weight", gamma, {D});
  o.put("n.bias", beta, {D});
  auto run = [&]() -> int {
    int xin, out;
    RC(tr.new_tensor(rows, D, &xin, 0, 0, 0, const_cast<float*>(x)));
    RC(tr.layernorm(xin, "n", eps, &out));
    RC(o.out(y, o.st.t[out].p, (size_t)rows * D));
    o.st.t[out].grad = const_cast<float*>(dy);
    RC(tr.backward());
    RC(o.out(dx, o.st.t[xin].grad, (size_t)rows * D));
    RC(o.grad(dgamma, "n.weight", D));
    RC(o.grad(dbeta, "n.bias", D));
    return D2T_OK;
  };
  return o.finish(run());
}

// One attention node, forward + backward, for both attention entries (include/d2t.h).  poison: the tape's blocks start as NaN
// and the operands' gradient buffers are left to Tr::bwd_attn (own_grad); otherwise the gradients start as zeros.
static int run_op_attention(const d2t_op_train_attention_args& a, bool poison, hipStream_t s) {
  OpCtx o(0, s);
  Tr& tr = o.tr;
  o.st.poison = poison;
  auto run = [&]() -> int {
    const int D = a.heads * a.hd;
    const size_t nprobs = (size_t)a.nb * a.heads * a.Lq * a.Lk;
    int qt, kt, out;
    if (a.layout == 1) {  // one packed tensor as both operands: the call of Tr::vit and of the decoder's self-attention
      RC(tr.new_tensor((long long)a.nb * a.Lq, 3 * D, &qt, 0, 0, 0, const_cast<float*>(a.qkv)));
      kt = qt;
      RC(tr.attention(qt, 0, qt, D, 2 * D, a.nb, a.Lq, a.Lk, a.heads, a.hd, a.causal, a.keytok, &out, false, a.dropmask, a.dropscale));
    } else {
      RC(tr.new_tensor((long long)a.nb * a.Lq, D, &qt, 0, 0, 0, const_cast<float*>(a.q)));
      RC(tr.new_tensor((long long)a.nb * a.Lk, 2 * D, &kt, 0, 0, 0, const_cast<float*>(a.kv)));
      RC(tr.attention(qt, 0, kt, 0, D, a.nb, a.Lq, a.Lk, a.heads, a.hd, a.causal, a.keytok, &out, false, a.dropmask, a.dropscale));
    }
    float* saved = o.st.nodes.back().attn.probs;
    RC(o.out(a.y, o.st.t[out].p, (size_t)a.nb * a.Lq * D));
    RC(o.out(a.probs, saved, nprobs));
    float* g;  // the tape hands a node's output gradient on as a mutable buffer: give it a private copy
    RC(tr.alloc(&g, (size_t)a.nb * a.Lq * D));
    RC(o.out(g, a.dy, (size_t)a.nb * a.Lq * D));
    o.st.t[out].grad = g;
    if (!poison) {
      RC(tr.zeros(&o.st.t[qt].grad, (size_t)a.nb * a.Lq * D));
      RC(tr.zeros(&o.st.t[kt].grad, (size_t)a.nb * a.Lk * 2 * D));
    }
    RC(tr.backward());
    RC(o.out(a.ds, saved, nprobs));
    if (a.layout == 1) {
      RC(o.out(a.dqkv, o.st.t[qt].grad, (size_t)a.nb * a.Lq * 3 * D));
    } else {
      RC(o.out(a.dq, o.st.t[qt].grad, (size_t)a.nb * a.Lq * D));
      RC(o.out(a.dkv, o.st.t[kt].grad, (size_t)a.nb * a.Lk * 2 * D));
    }
    return D2T_OK;
  };
  return o.finish(run());
}

// q [nb*Lq][heads*hd], kv [nb*Lk][2*heads*hd] (keys in the first half of a row, values in the second); keytok: optional
// [nb][Lk] token ids whose PAD (0) entries are masked out (tgt_key_padding_mask, tfm.py:107-110); causal: additive -inf mask
int d2t_op_train_attention(const float* q, const float* kv, const int64_t* keytok, const float* dy, float* y, float* dq,
                           float* dkv, int32_t nb, int32_t Lq, int32_t Lk, int32_t heads, int32_t hd, int32_t causal,
                           d2t_stream stream) {
  if (!q || !kv || !dy) return D2T_EINVAL;
  d2t_op_train_attention_args a{};
  a.q = q; a.kv = kv; a.keytok = keytok; a.dy = dy; a.y = y; a.dq = dq; a.dkv = dkv;
  a.nb = nb; a.Lq = Lq; a.Lk = Lk; a.heads = heads; a.hd = hd; a.causal = causal;
  return run_op_attention(a, false, (hipStream_t)stream);
}

int d2t_op_train_attention_ex(const d2t_op_train_attention_args* a, d2t_stream stream) {
  if (!a || !a->dy || (a->layout != 0 && a->layout != 1)) return D2T_EINVAL;
  if (a->layout == 0 ? (!a->q || !a->kv) : (!a->qkv || a->Lq != a->Lk)) return D2T_EINVAL;
  if ((a->hd != 32 && a->hd != 64) || a->nb < 1 || a->Lq < 1 || a->Lk < 1 || a->heads < 1) return D2T_EINVAL;
  if ((long long)a->nb * a->heads > 0x7fffffffll) return D2T_EINVAL;                            // one block per (batch, head)
  if ((long long)a->nb * std::max(a->Lq, a->Lk) * 3 * a->heads * a->hd > (1ll << 31)) return D2T_EINVAL;
  if ((long long)a->nb * a->heads * a->Lq * a->Lk > (1ll << 31)) return D2T_EINVAL;
  if (a->dropmask && !(std::isfinite(a->dropscale) && a->dropscale > 0.f)) return D2T_EINVAL;
  if (a->plan) {
    const AttnTrainPlan pl = attn_train_plan(a->hd, a->Lq, a->Lk);
    a->plan[0] = pl.fwd_form; a->plan[1] = pl.fwd_waves; a->plan[2] = pl.bwd_form; a->plan[3] = pl.bwd_waves;
  }
  return run_op_attention(*a, true, (hipStream_t)stream);
}

int d2t_op_train_maxpool(const float* x, const float* dy, float* y, float* dx, int32_t B, int32_t H, int32_t W, int32_t C,
                         int32_t SH, int32_t SW, int32_t PH, int32_t PW, d2t_stream stream) {
  if (!x || !dy) return D2T_EINVAL;
  OpCtx o(0, (hipStream_t)stream);
  Tr& tr = o.tr;
  auto run = [&]() -> int {
    int xin, out;
    RC(tr.new_tensor((long long)B * H * W, C, &xin, B, H, W, const_cast<float*>(x)));
    RC(tr.pool(xin, SH, SW, PH, PW, &out));
    const TT yo = o.st.t[out];
    RC(o.out(y, yo.p, (size_t)yo.rows * C));
    o.st.t[out].grad = const_cast<float*>(dy);
    RC(tr.backward());
    RC(o.out(dx, o.st.t[xin].grad, (size_t)B * H * W * C));
    return D2T_OK;
  };
  return o.finish(run());
}

// The recurrent backward kernels one at a time (include/d2t.h): train_recurrent.hip's launchers on caller tensors in the
// kernels' own layouts, asynchronous on the stream.
int d2t_op_bilstm_bwd(const float* dout, const float* sv_gates, const float* sv_c, const float* whh_fwd, const float* whh_rev,
                      float* dgates, int32_t B, int32_t T, int32_t H, d2t_stream stream) {
  if (!dout || !sv_gates || !sv_c || !whh_fwd || !whh_rev || !dgates) return D2T_EINVAL;
  if (H != 256 || B < 1 || B > 65535 * 4 || T < 1) return D2T_EINVAL;  // grid.y blocks of four rows
  return op_status(launch_bilstm_train_bwd(dout, sv_gates, sv_c, whh_fwd, whh_rev, dgates, B, T, H, (hipStream_t)stream));
}

int d2t_op_attn_lstm_bwd(const d2t_op_attn_lstm_bwd_args* a, d2t_stream stream) {
  if (!a || !a->dlogits || !a->mem || !a->kp || !a->wih_raw || !a->whh_raw || !a->wq_raw || !a->wloc || !a->bloc || !a->wscore ||
      !a->sv_cprev || !a->sv_cafter || !a->sv_gates || !a->sv_alpha || !a->sv_hq || !a->dmem || !a->dkp || !a->dgates || !a->dhq ||
      !a->dh0 || !a->dc0 || !a->dwloc || !a->dbloc || !a->dwscore || !a->dbscore)
    return D2T_EINVAL;
  if (!a->dhl && (!a->wg_t || a->V > 1024)) return D2T_EINVAL;  // the in-kernel generator product stages 1024 classes
  if (a->B < 1 || a->B > 65535 || a->S < 1 || a->V < 1 || a->V > D2T_ATTN_MAX_CLASSES || a->taps < 1 || a->taps > 11 ||
      a->key_off < 0 || a->key_off > 1 || a->T - a->key_off < 1 || a->T - a->key_off > 4096)
    return D2T_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  AttnTrainBwdP p{};
  p.dlogits = a->dlogits; p.mem = a->mem; p.T = a->T; p.D = 256; p.key_off = a->key_off; p.kp = a->kp;
  p.wg_t = a->wg_t; p.wih_raw = a->wih_raw; p.whh_raw = a->whh_raw; p.wq_raw = a->wq_raw;
  p.wloc = a->wloc; p.bloc = a->bloc; p.wscore = a->wscore; p.taps = a->taps;
  p.sv_cprev = a->sv_cprev; p.sv_cafter = a->sv_cafter; p.sv_gates = a->sv_gates; p.sv_alpha = a->sv_alpha; p.sv_hq = a->sv_hq;
  p.dmem = a->dmem; p.dkp = a->dkp; p.dgates = a->dgates; p.dhq = a->dhq; p.demb = a->demb; p.dhl = a->dhl;
  p.dh0 = a->dh0; p.dc0 = a->dc0; p.dwloc = a->dwloc; p.dbloc = a->dbloc; p.dwscore = a->dwscore; p.dbscore = a->dbscore;
  p.B = a->B; p.S = a->S; p.V = a->V; p.H = 256; p.E = 256; p.coverage = a->coverage != 0;
  const size_t n = (size_t)a->B * a->T * 256 * sizeof(float);
  hipError_t e = hipMemsetAsync(a->dmem, 0, n, s);
  if (e == hipSuccess) e = hipMemsetAsync(a->dkp, 0, n, s);
  if (e == hipSuccess) e = launch_attn_train_lstm_bwd(p, s);
  return op_status(e);
}

int d2t_op_loc_unfold_bwd(const float* dwloc, const float* dbloc, int32_t B, const float* conv_w, const float* conv_b,
                          const float* proj_w, int32_t H, int32_t kd, int32_t taps, float* d_conv_w, float* d_conv_b,
                          float* d_proj_w, float* d_proj_b, d2t_stream stream) {
  if (!dwloc || !dbloc || !conv_w || !conv_b || !proj_w || !d_conv_w || !d_conv_b || !d_proj_w || !d_proj_b) return D2T_EINVAL;
  if (B < 1 || H < 1 || kd < 1 || taps < 1 || (long long)H * (taps + 1) * 4 > 64 * 1024) return D2T_EINVAL;  // one block's LDS
  return op_status(launch_loc_unfold_bwd(dwloc, dbloc, B, conv_w, conv_b, proj_w, H, kd, taps, d_conv_w, d_conv_b, d_proj_w,
                                             d_proj_b, (hipStream_t)stream));
}

// The remaining kernels of the step one at a time (include/d2t.h): nodes of the tape through an OpCtx, launchers as they are.
static bool gc_width(int C) { return C >= 4 && C <= 512 && C % 4 == 0; }  // thread = channel / float4 rows of the gc_* kernels

int d2t_op_train_gc_pool(const float* x, const float* wg, const float* bg, const float* dctx, float* ctx, float* dx, float* dwg,
                         float* dbg, int32_t B, int32_t H, int32_t W, int32_t C, d2t_stream stream) {
  if (!x || !wg || !bg || !dctx) return D2T_EINVAL;
  if (B < 1 || B > 65535 || H < 1 || W < 1 || (long long)H * W > (1 << 24) || !gc_width(C)) return D2T_EINVAL;
  OpCtx o(0, (hipStream_t)stream);
  Tr& tr = o.tr;
  o.put("g.weight", wg, {C});
  o.put("g.bias", bg, {1});
  auto run = [&]() -> int {
    int xin, out;
    RC(tr.new_tensor((long long)B * H * W, C, &xin, B, H, W, const_cast<float*>(x)));
    RC(tr.gc_pool(xin, "g", &out));
    RC(o.out(ctx, o.st.t[out].p, (size_t)B * C));
    o.st.t[out].grad = const_cast<float*>(dctx);
    RC(tr.backward());
    RC(o.out(dx, o.st.t[xin].grad, (size_t)B * H * W * C));
    RC(o.grad(dwg, "g.weight", C));
    RC(o.grad(dbg, "g.bias", 1));
    return D2T_OK;
  };
  return o.finish(run());
}

int d2t_op_train_bcast_add(const float* x, const float* y, const float* dout, float* out, float* dx, float* dy, int32_t B,
                           int32_t HW, int32_t C, d2t_stream stream) {
  if (!x || !y || !dout) return D2T_EINVAL;
  if (B < 1 || B > 65535 || HW < 1 || HW > (1 << 24) || !gc_width(C)) return D2T_EINVAL;
  OpCtx o(0, (hipStream_t)stream);
  Tr& tr = o.tr;
  auto run = [&]() -> int {
    int xin, yin, res;
    RC(tr.new_tensor((long long)B * HW, C, &xin, B, 1, HW, const_cast<float*>(x)));
    RC(tr.new_tensor(B, C, &yin, 0, 0, 0, const_cast<float*>(y)));
    RC(tr.bcast_add(xin, yin, &res));
    RC(o.out(out, o.st.t[res].p, (size_t)B * HW * C));
    o.st.t[res].grad = const_cast<float*>(dout);
    RC(tr.backward());
    RC(o.out(dx, o.st.t[xin].grad, (size_t)B * HW * C));
    RC(o.out(dy, o.st.t[yin].grad, (size_t)B * C));
    return D2T_OK;
  };
  return o.finish(run());
}

int d2t_op_train_mean_h(const float* x, const float* dy, float* y, float* dx, int32_t B, int32_t H, int32_t W, int32_t C,
                        d2t_stream stream) {
  if (!x || !dy || B < 1 || H < 1 || W < 1 || C < 1 || (long long)B * H * W * C > (1ll << 31)) return D2T_EINVAL;
  OpCtx o(0, (hipStream_t)stream);
  Tr& tr = o.tr;
  auto run = [&]() -> int {
    int xin, out;
    RC(tr.new_tensor((long long)B * H * W, C, &xin, B, H, W, const_cast<float*>(x)));
    RC(tr.mean_h(xin, &out));
    RC(o.out(y, o.st.t[out].p, (size_t)B * W * C));
    o.st.t[out].grad = const_cast<float*>(dy);
    RC(tr.backward());
    RC(o.out(dx, o.st.t[xin].grad, (size_t)B * H * W * C));
    return D2T_OK;
  };
  return o.finish(run());
}

int d2t_op_train_maxpool_w(const float* x, const float* dy, float* y, float* dx, int32_t B, int32_t H, int32_t W, int32_t C,
                           int32_t KW, int32_t SH, int32_t SW, int32_t PH, int32_t PW, d2t_stream stream) {
  if (!x || !dy || (KW != 1 && KW != 2) || B < 1 || H < 1 || W < 1 || C < 4 || C % 4 || SH < 1 || SW < 1) return D2T_EINVAL;
  if (PH < 0 || PH > 1 || PW < 0 || PW > KW / 2 || H + 2 * PH < 2 || W + 2 * PW < KW) return D2T_EINVAL;  // nn.MaxPool2d's own rule
  if ((long long)B * H * W * C > (1ll << 31)) return D2T_EINVAL;
  OpCtx o(0, (hipStream_t)stream);
  Tr& tr = o.tr;
  auto run = [&]() -> int {
    int xin, out;
    RC(tr.new_tensor((long long)B * H * W, C, &xin, B, H, W, const_cast<float*>(x)));
    RC(tr.pool(xin, SH, SW, PH, PW, &out, KW));
    const TT yo = o.st.t[out];
    RC(o.out(y, yo.p, (size_t)yo.rows * C));
    o.st.t[out].grad = const_cast<float*>(dy);
    RC(tr.backward());
    RC(o.out(dx, o.st.t[xin].grad, (size_t)B * H * W * C));
    return D2T_OK;
  };
  return o.finish(run());
}

int d2t_op_train_ew(const float* x, const float* dy, float* y, float* dx, int64_t n, int32_t op, d2t_stream stream) {
  if (!x || !dy || n < 4 || n % 4 || n > (1ll << 31) || (op != 0 && op != 1)) return D2T_EINVAL;
  OpCtx o(0, (hipStream_t)stream);
  Tr& tr = o.tr;
  auto run = [&]() -> int {
    int xin, out;
    RC(tr.new_tensor(n / 4, 4, &xin, 0, 0, 0, const_cast<float*>(x)));
    RC(op == 0 ? tr.gelu(xin, &out) : tr.relu(xin, &out));
    RC(o.out(y, o.st.t[out].p, (size_t)n));
    o.st.t[out].grad = const_cast<float*>(dy);
    RC(tr.backward());
    RC(o.out(dx, o.st.t[xin].grad, (size_t)n));
    return D2T_OK;
  };
  return o.finish(run());
}

int d2t_op_embed_train(const float* E, const float* pe, const int64_t* tok, float* x, int32_t rows, int32_t L, int32_t V,
                       int32_t D, float scale, d2t_stream stream) {
  if (!E || !pe || !tok || !x || rows < 1 || L < 1 || V < 1 || D < 1) return D2T_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  std::vector<int64_t> h((size_t)rows);  // the kernel indexes E by the token
  if (hipMemcpyAsync(h.data(), tok, (size_t)rows * 8, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
    return D2T_EHIP;
  for (int64_t t : h)
    if (t < 0 || t >= V) return D2T_EINVAL;
  return op_status(launch_embed_train(E, pe, tok, x, rows, L, D, scale, s));
}

int d2t_op_embed_bwd(const float* dx, const int64_t* tok, float* dE, int32_t rows, int32_t V, int32_t D, float scale,
                     int32_t pad_id, d2t_stream stream) {
  if (!dx || !tok || !dE || rows < 1 || V < 1 || D < 1 || D > 1024) return D2T_EINVAL;  // four columns per thread of 256
  return op_status(launch_embed_bwd(dx, tok, dE, rows, V, D, scale, pad_id, (hipStream_t)stream));
}

int d2t_op_dropout_mask(uint8_t* mask, int64_t n, float p, uint64_t seed, uint64_t stream_id, d2t_stream stream) {
  if (!mask || n < 1 || !(p >= 0.f) || p >= 1.f) return D2T_EINVAL;
  return op_status(launch_dropout_mask(mask, (size_t)n, p, seed, stream_id, (hipStream_t)stream));
}

int d2t_op_apply_mask(const float* a, const uint8_t* mask, float scale, float* out, int64_t n, d2t_stream stream) {
  if (!a || !mask || !out || n < 1) return D2T_EINVAL;
  return op_status(launch_apply_mask(a, mask, scale, out, (size_t)n, (hipStream_t)stream));
}

int d2t_op_bicubic_table(const float* src, float* dst, int32_t GH, int32_t GW, int32_t gh, int32_t gw, int32_t D, float scale_h,
                         float scale_w, int32_t transpose, d2t_stream stream) {
  if (!src || !dst || src == dst || GH < 1 || GW < 1 || gh < 1 || gw < 1 || D < 1) return D2T_EINVAL;
  if ((long long)GH * GW * D > (1ll << 31) || (long long)gh * gw * D > (1ll << 31)) return D2T_EINVAL;
  if (!(scale_h > 0.f) || !(scale_w > 0.f) || !(scale_h * (float)gh < 1e9f) || !(scale_w * (float)gw < 1e9f)) return D2T_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  return op_status(transpose ? launch_bicubic_table_bwd(src, dst, GH, GW, gh, gw, D, scale_h, scale_w, s)
                             : launch_bicubic_table(src, dst, GH, GW, gh, gw, D, scale_h, scale_w, s));
}

int d2t_op_sum_over_batch(const float* x, float* out, int32_t B, int64_t stride, int64_t n, d2t_stream stream) {
  if (!x || !out || B < 1 || n < 1 || stride < n) return D2T_EINVAL;
  return op_status(launch_sum_over_batch(x, out, B, stride, n, (hipStream_t)stream));
}

int d2t_op_token_rows(const float* src, float* dst, int32_t B, int32_t n, int32_t skip, int32_t D, int32_t scatter,
                      d2t_stream stream) {
  if (!src || !dst || src == dst || B < 1 || n < 1 || skip < 0 || D < 1 || (long long)B * ((long long)n + skip) * D > (1ll << 31))
    return D2T_EINVAL;
  return op_status(launch_token_rows(src, dst, B, n, skip, D, scatter != 0, (hipStream_t)stream));
}

int d2t_op_sum_rows_strided(const float* x, float* out, int32_t B, int64_t stride_rows, int32_t row, int32_t D,
                            d2t_stream stream) {
  if (!x || !out || B < 1 || D < 1 || stride_rows < 1 || row < 0 || row >= stride_rows) return D2T_EINVAL;
  return op_status(launch_sum_rows_strided(x, out, B, stride_rows, row, D, (hipStream_t)stream));
}

// The weight-gradient, BatchNorm, LayerNorm, stem and data-movement launchers one at a time (include/d2t.h): caller tensors
// in the kernels' own layouts, asynchronous on the stream, every size checked first.
static const long long OP_MAX_ELEMS = 1ll << 31;

int d2t_op_wgrad_plan(int64_t P, int32_t M, int32_t N, int32_t taps, int32_t records, int64_t* out) {
  if (!out || P < 1 || M < 1 || N < 1 || taps < 1) return D2T_EINVAL;
  const WgradRecTile* rec = records ? wgrad_rec_tile(M, N) : nullptr;
  if (records && !rec) return D2T_EINVAL;
  const WgradPlan pl = wgrad_plan(P, M, N, taps, rec);
  const int plain = (M <= 64 || N <= 64) ? 64 : 128;
  out[0] = pl.S; out[1] = pl.chunk; out[2] = rec ? rec->bm : plain; out[3] = rec ? rec->bn : plain;
  return D2T_OK;
}

int d2t_op_wgrad(const d2t_op_wgrad_args* a, d2t_stream stream) {
  if (!a || !a->a || !a->b || !a->part) return D2T_EINVAL;
  if (a->P < 1 || a->M < 1 || a->N < 1 || a->lda < a->M || a->ldb < a->N || a->S < 1 || a->chunk < 1) return D2T_EINVAL;
  if (a->M % 4 || a->N % 4 || a->lda % 4 || a->ldb % 4) return D2T_EINVAL;  // 16-byte operand loads
  if ((long long)a->S * a->chunk < a->P || (long long)(a->S - 1) * a->chunk >= a->P || a->S > 65535) return D2T_EINVAL;
  int taps = 1;
  long long brows = a->P;
  if (a->geom) {
    if (a->B < 1 || a->H < 1 || a->W < 1 || a->OH < 1 || a->OW < 1 || a->KH < 1 || a->KW < 1 || a->SH < 1 || a->SW < 1 ||
        a->PH < 0 || a->PW < 0 || a->KH * a->KW > 65535)
      return D2T_EINVAL;
    if ((long long)a->B * a->OH * a->OW != a->P) return D2T_EINVAL;
    taps = a->KH * a->KW;
    brows = (long long)a->B * a->H * a->W;
  }
  if (a->P * a->lda > OP_MAX_ELEMS || brows * a->ldb > OP_MAX_ELEMS || (long long)a->S * taps * a->M * a->N > OP_MAX_ELEMS)
    return D2T_EINVAL;
  const WgradRecTile* rec = nullptr;
  if (a->records) {
    rec = wgrad_rec_tile(a->M, a->N);
    if (!rec || !a->geom || !a->bf16x3 || a->lda != a->M || a->ldb != a->N || a->chunk % 16) return D2T_EINVAL;
  }
  hipStream_t s = (hipStream_t)stream;
  WgradP p{};
  p.a = a->a; p.b = a->b; p.part = a->part; p.P = a->P; p.M = a->M; p.N = a->N; p.lda = a->lda; p.ldb = a->ldb; p.taps = taps;
  p.KW = 1; p.S = a->S; p.chunk = a->chunk; p.bf16x3 = a->bf16x3 ? 1 : 0;
  if (a->geom) {
    p.geom = 1; p.H = a->H; p.W = a->W; p.OH = a->OH; p.OW = a->OW;
    p.KW = a->KW; p.SH = a->SH; p.SW = a->SW; p.PH = a->PH; p.PW = a->PW;
  }
  if (a->tile) {
    const int plain = (a->M <= 64 || a->N <= 64) ? 64 : 128;
    a->tile[0] = rec ? rec->bm : plain; a->tile[1] = rec ? rec->bn : plain;
  }
  if (!rec) return op_status(launch_wgrad(p, s));
  // record operands: [row][32 x hi | 32 x lo] per 32 columns = as many bytes as the fp32 rows; 256 zero bytes for the padding taps
  void *ar = nullptr, *br = nullptr, *zero = nullptr;
  hipError_t e = hipMalloc(&ar, (size_t)a->P * a->M * 4);
  if (e == hipSuccess) e = hipMalloc(&br, (size_t)brows * a->N * 4);
  if (e == hipSuccess) e = hipMalloc(&zero, 256);
  if (e == hipSuccess) e = hipMemsetAsync(zero, 0, 256, s);
  if (e == hipSuccess) e = launch_split_act(a->a, reinterpret_cast<uint16_t*>(ar), (size_t)a->P, a->M, s, 0);
  if (e == hipSuccess) e = launch_split_act(a->b, reinterpret_cast<uint16_t*>(br), (size_t)brows, a->N, s, 0);
  if (e == hipSuccess) {
    p.a_rec = reinterpret_cast<const uint16_t*>(ar); p.b_rec = reinterpret_cast<const uint16_t*>(br); p.zero = zero;
    e = launch_wgrad(p, s);
  }
  const hipError_t e2 = hipStreamSynchronize(s);  // the operand records are the entry's own
  if (ar) hipFree(ar);
  if (br) hipFree(br);
  if (zero) hipFree(zero);
  return e != hipSuccess ? op_status(e) : op_status(e2);
}

int d2t_op_wgrad_reduce(const float* part, float* dst, int32_t S, int32_t taps, int32_t M, int32_t N, int32_t layout,
                        int32_t accumulate, d2t_stream stream) {
  if (!part || !dst || S < 1 || taps < 1 || M < 1 || N < 1 || (layout != 0 && layout != 1) || (layout == 0 && taps != 1))
    return D2T_EINVAL;
  if ((long long)S * taps * M * N > OP_MAX_ELEMS) return D2T_EINVAL;
  return op_status(launch_wgrad_reduce(part, dst, S, taps, M, N, layout, accumulate != 0, (hipStream_t)stream));
}

int d2t_op_colreduce(int32_t mode, const float* a, const float* y, const float* z, const float* mean, const float* rstd,
                     float* part, int64_t R, int32_t C, int32_t* chunks, d2t_stream stream) {
  if (mode < CR_SUM || mode > CR_LN_BWD || R < 1 || C < 4 || C % 4 || R * C > OP_MAX_ELEMS) return D2T_EINVAL;
  if (chunks) *chunks = colreduce_chunks(R, C);
  if (!part) return chunks ? D2T_OK : D2T_EINVAL;
  if (!a || (mode >= CR_BN_BWD && (!z || !mean || !rstd)) || (y && mode != CR_BN_BWD)) return D2T_EINVAL;
  ColRedP p{};
  p.a = a; p.y = y; p.z = z; p.mean = mean; p.rstd = rstd; p.part = part; p.R = R; p.C = C; p.mode = mode;
  return op_status(launch_colreduce(p, (hipStream_t)stream));
}

int d2t_op_colreduce_final(const float* part, int32_t chunks, int32_t C, float* out0, float* out1, int32_t accumulate,
                           d2t_stream stream) {
  if (!part || !out0 || chunks < 1 || C < 1 || (long long)chunks * 2 * C > OP_MAX_ELEMS) return D2T_EINVAL;
  return op_status(launch_colreduce_final(part, chunks, C, out0, out1, accumulate != 0, (hipStream_t)stream));
}

int d2t_op_bn_finalize(const float* part, int32_t chunks, int32_t C, int64_t R, float eps, float momentum, const float* z,
                       float* mean, float* rstd, float* run_mean, float* run_var, d2t_stream stream) {
  if (!part || !z || !mean || !rstd || chunks < 1 || C < 1 || R < 1 || (long long)chunks * 2 * C > OP_MAX_ELEMS) return D2T_EINVAL;
  if (!(eps >= 0.f) || !(momentum >= 0.f && momentum <= 1.f) || (run_mean == nullptr) != (run_var == nullptr)) return D2T_EINVAL;
  return op_status(launch_bn_finalize(part, chunks, C, R, eps, momentum, z, mean, rstd, run_mean, run_var, (hipStream_t)stream));
}

int d2t_op_bn_apply(const float* z, const float* mean, const float* rstd, const float* gamma, const float* beta, const float* res,
                    float* y, uint16_t* planes, int64_t R, int32_t C, int32_t relu, d2t_stream stream) {
  if (!z || !mean || !rstd || !gamma || !beta || !y || R < 1 || C < 4 || C % 4 || R * C > OP_MAX_ELEMS) return D2T_EINVAL;
  if (planes && C % 32) return D2T_EINVAL;
  return op_status(launch_bn_apply(z, mean, rstd, gamma, beta, res, y, R, C, relu != 0, (hipStream_t)stream, planes));
}

int d2t_op_bn_bwd_apply(const float* dy, const float* y, const float* z, const float* mean, const float* rstd,
                        const float* gamma, const float* s0, const float* s1, float* dz, float* gout, uint16_t* planes, int64_t R,
                        int32_t C, d2t_stream stream) {
  if (!dy || !z || !mean || !rstd || !gamma || !s0 || !s1 || !dz || R < 1 || C < 4 || C % 4 || R * C > OP_MAX_ELEMS)
    return D2T_EINVAL;
  if (planes && C % 32) return D2T_EINVAL;
  return op_status(launch_bn_bwd_apply(dy, y, z, mean, rstd, gamma, s0, s1, dz, gout, R, C, (hipStream_t)stream, planes));
}

static bool ln_width(int D) { return D == 128 || D == 256 || D == 512; }  // one wave per row, D / 64 elements per lane

int d2t_op_ln_train(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, int32_t rows,
                    int32_t D, float eps, d2t_stream stream) {
  if (!x || !gamma || !beta || !y || !mean || !rstd || rows < 1 || !ln_width(D) || !(eps >= 0.f)) return D2T_EINVAL;
  if ((long long)rows * D > OP_MAX_ELEMS) return D2T_EINVAL;
  return op_status(launch_ln_train(x, gamma, beta, y, mean, rstd, rows, D, eps, (hipStream_t)stream));
}

int d2t_op_ln_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma, const float* add,
                  float* dx, int32_t rows, int32_t D, d2t_stream stream) {
  if (!dy || !x || !mean || !rstd || !gamma || !dx || rows < 1 || !ln_width(D)) return D2T_EINVAL;
  if ((long long)rows * D > OP_MAX_ELEMS) return D2T_EINVAL;
  return op_status(launch_ln_bwd(dy, x, mean, rstd, gamma, add, dx, rows, D, (hipStream_t)stream));
}

static bool stem_shape(int B, int Cin, int H, int W, int Cout) {
  return B >= 1 && H >= 1 && W >= 1 && (Cin == 1 || Cin == 3) && (Cout == 32 || Cout == 64) &&
         (long long)B * H * W * Cout <= OP_MAX_ELEMS;
}

int d2t_op_stem_raw(const float* img, const float* w, float* z, int32_t B, int32_t Cin, int32_t H, int32_t W, int32_t Cout,
                    d2t_stream stream) {
  if (!img || !w || !z || !stem_shape(B, Cin, H, W, Cout)) return D2T_EINVAL;
  return op_status(launch_stem_raw(img, w, z, B, Cin, H, W, Cout, (hipStream_t)stream));
}

int d2t_op_stem_wgrad(const float* img, const float* dz, float* part, int32_t B, int32_t Cin, int32_t H, int32_t W, int32_t Cout,
                      int32_t chunk, int32_t nchunks, d2t_stream stream) {
  if (!img || !dz || !part || !stem_shape(B, Cin, H, W, Cout) || chunk < 1 || nchunks < 1) return D2T_EINVAL;
  const long long P = (long long)B * H * W;
  if ((long long)nchunks * chunk < P || (long long)(nchunks - 1) * chunk >= P) return D2T_EINVAL;
  if ((long long)nchunks * 9 * Cin * Cout > OP_MAX_ELEMS) return D2T_EINVAL;
  return op_status(launch_stem_wgrad(img, dz, part, B, Cin, H, W, Cout, chunk, nchunks, (hipStream_t)stream));
}

int d2t_op_dilate(const float* src, float* dst, int32_t B, int32_t OH, int32_t OW, int32_t C, int32_t DH, int32_t DW, int32_t SH,
                  int32_t SW, int32_t offh, int32_t offw, d2t_stream stream) {
  if (!src || !dst || src == dst || B < 1 || OH < 1 || OW < 1 || C < 1 || DH < 1 || DW < 1 || SH < 1 || SW < 1 || offh < 0 || offw < 0)
    return D2T_EINVAL;
  if ((long long)B * OH * OW * C > OP_MAX_ELEMS || (long long)B * DH * DW * C > OP_MAX_ELEMS) return D2T_EINVAL;
  return op_status(launch_dilate(src, dst, B, OH, OW, C, DH, DW, SH, SW, offh, offw, (hipStream_t)stream));
}

int d2t_op_flip_oihw(const float* w, float* out, int32_t Cout, int32_t Cin, int32_t KH, int32_t KW, d2t_stream stream) {
  if (!w || !out || w == out || Cout < 1 || Cin < 1 || KH < 1 || KW < 1 || (long long)Cout * Cin * KH * KW > OP_MAX_ELEMS)
    return D2T_EINVAL;
  return op_status(launch_flip_oihw(w, out, Cout, Cin, KH, KW, (hipStream_t)stream));
}

int d2t_op_pad_cols(const float* src, float* dst, int64_t rows, int32_t Cs, int32_t Cd, d2t_stream stream) {
  if (!src || !dst || src == dst || rows < 1 || Cs < 1 || Cd < Cs || rows * Cd > OP_MAX_ELEMS) return D2T_EINVAL;
  return op_status(launch_pad_cols(src, dst, (size_t)rows, Cs, Cd, (hipStream_t)stream));
}

int d2t_op_copy2d(const float* src, int32_t lds, float* dst, int32_t ldd, int64_t rows, int32_t cols, d2t_stream stream) {
  if (!src || !dst || src == dst || rows < 1 || cols < 1 || lds < cols || ldd < cols) return D2T_EINVAL;
  if (rows * lds > OP_MAX_ELEMS || rows * ldd > OP_MAX_ELEMS) return D2T_EINVAL;
  return op_status(launch_copy2d(src, lds, dst, ldd, (size_t)rows, cols, (hipStream_t)stream));
}

}  // extern "C"
