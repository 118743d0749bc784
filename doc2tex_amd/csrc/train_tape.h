// The tape of the training step, shared between train.hip (the operations), train_models.hip (the networks) and
// train_abi.hip (the C entries): tensors, nodes, the per-context state and the builder `Tr`.  Internal to libd2t.
//
// The network is recorded as a tape of nodes over row-major [rows][cols] tensors (NHWC maps are [B*H*W][C]); the backward
// walks it in reverse and accumulates into tensor gradients, so residual fan-out needs no special cases.
#pragma once
#include "ctx.h"

// (hidden: these types cross the three files, but none of their symbols belongs to the library's surface)
#pragma GCC visibility push(hidden)
namespace tape {

struct Arena {
  struct Blk { char* p; size_t cap; };
  std::vector<Blk> blks;
  size_t cur = 0, off = 0;
  void reset() { cur = 0; off = 0; }
  float* alloc(size_t floats) {
    const size_t bytes = (floats * 4 + 255) & ~(size_t)255;
    while (cur < blks.size() && off + bytes > blks[cur].cap) { ++cur; off = 0; }
    if (cur == blks.size()) {
      const size_t cap = std::max(bytes, (size_t)256 << 20);
      void* q = nullptr;
      if (hipMalloc(&q, cap) != hipSuccess) return nullptr;
      blks.push_back({(char*)q, cap});
      off = 0;
    }
    float* r = reinterpret_cast<float*>(blks[cur].p + off);
    off += bytes;
    return r;
  }
  void release() {
    for (auto& b : blks) hipFree(b.p);
    blks.clear();
    reset();
  }
};

struct TT {  // tensor on the tape
  float* p = nullptr;
  long long rows = 0;
  int cols = 0;
  int B = 0, H = 0, W = 0;  // NHWC maps: rows = B*H*W
  float* grad = nullptr;
  const uint16_t* planes = nullptr;  // split-bf16 records of p, when the producing kernel wrote them alongside (bf16x3 mode)
};

enum Kind { N_CONV, N_POOL, N_LINEAR, N_LN, N_ATTN, N_GELU, N_EMBED, N_TOKENS, N_ADDCONST, N_DROPOUT, N_ADD, N_LSTM, N_RELU,
            N_GCPOOL, N_BCAST, N_MEANH, N_BILSTM };

// What a node's forward builder saves for its backward: `kind`, the tensor ids, and the member group named after the kind
// (by convention a builder fills its own group and a backward reads only that one; the other groups keep their defaults).
// N_GELU, N_RELU, N_ADD, N_ADDCONST, N_BCAST and N_MEANH need nothing beyond the tensors.
struct Node {
  Kind kind;
  int in = -1, in2 = -1, out = -1;  // tensor ids (in2: residual / second operand)
  struct Drop {  // keep mask (bytes, nullptr: no dropout) and 1 / (1 - p)
    const uint8_t* mask = nullptr;
    float scale = 1.f;
  };
  struct Conv {  // conv (+ BatchNorm, or a bias when bnkey is empty) (+ residual in2) (+ ReLU); stem: the image's own kernels
    std::string wkey, bnkey;
    int Cin = 0, Cout = 0, KH = 0, KW = 0, SH = 1, SW = 1, PH = 0, PW = 0;
    float *z = nullptr, *mean = nullptr, *rstd = nullptr;  // the convolution's output; BatchNorm's batch statistics
    bool relu = false, stem = false;
  } conv;
  struct Pool { int KW = 2, SH = 1, SW = 1, PH = 0, PW = 0; } pool;  // max-pool, window 2 x KW
  struct Linear {  // out = act(in @ W[woff : woff+N]^T + b) (+ in2)
    std::string key;
    int N = 0, K = 0, woff = 0;
    bool relu = false, nobias = false;  // nobias: nn.Linear(..., bias=False)
  } lin;
  struct LayerNorm {
    std::string key;
    float *mean = nullptr, *rstd = nullptr;  // per row
  } ln;
  struct Attn {  // q / k / v column offsets inside tensors in (q) and in2 (k, v)
    int qoff = 0, koff = 0, voff = 0, heads = 0, hd = 0, Lq = 0, Lk = 0, nb = 0;
    float* probs = nullptr;
    Drop drop;  // nn.MultiheadAttention(dropout=p): on the softmax probabilities
  } attn;
  Drop drop;  // N_DROPOUT
  struct Embed { std::string key; } embed;
  struct Tokens {  // out[b][0] = cls + pos[0], out[b][1+i] = in[b][i] + pos[1+i]   (in = patch tokens)
    std::string cls_key, pos_key;  // pos_key empty: a frozen table
    int ntok = 0;
    int table_h = 0, table_w = 0, crop_h = 0, crop_w = 0;  // patch grids of the learned table and of this crop
  } tokens;
  struct GcPool {
    std::string key;
    float* logits = nullptr;  // attention logits over the positions
  } gcpool;
  struct Lstm {  // teacher-forced LSTM-attention decoder: in = memory, in2 = key projection, out = logits; per (row, step)
    float *h_prev = nullptr, *c_prev = nullptr, *h_after = nullptr, *c_after = nullptr, *gates = nullptr, *alpha = nullptr,
          *hq = nullptr, *ctx_emb = nullptr;  // ctx_emb: [context | embedded input token]
    const int64_t* tokens = nullptr;  // the input token
    int init_mode = 0;                // how the initial state was formed (AttnDecP::init_mode)
    int B = 0, S = 0, T = 0, key_off = 0;
    Drop drop;  // nn.Dropout on the generator output of every step
  } lstm;
  struct BiLstm {
    std::string key;  // "...rnn."
    float *gates = nullptr, *cells = nullptr;  // gates after their nonlinearities, cell states
    int layer = 0, in_width = 0, B = 0, T = 0;
  } bilstm;

  // A discrete decision of the forward pass (d2t_train_read_decision): every max-pool and every ReLU, fused or on its own.
  bool is_decision() const {
    return kind == N_POOL || kind == N_RELU || (kind == N_CONV && conv.relu) || (kind == N_LINEAR && lin.relu);
  }
};

// how Tr::wgrad splits the P rows of a weight gradient: S chunks of `chunk` rows each (train.hip; reported by the test entry
// d2t_op_wgrad_plan)
struct WgradPlan { long long S, chunk; };
WgradPlan wgrad_plan(long long P, int M, int N, int taps, const WgradRecTile* rec);

struct Tr {  // builder / runner bound to one context and stream
  d2t_ctx* c;
  d2t_train_state* st;
  hipStream_t s;

  // ---- core (train.hip): tape memory, parameters and their gradient buffers, GEMMs, reductions
  int alloc(float** p, size_t floats);
  int zeros(float** p, size_t floats);
  int new_tensor(long long rows, int cols, int* id, int B = 0, int H = 0, int W = 0, float* into = nullptr);
  int raw(const std::string& k, const float** p, size_t numel = 0);
  int grad_buf(const std::string& k, float** p);
  int ensure_part(size_t floats);
  int gemm_nt(const float* a, const float* w, const float* bias, const float* res, float* out, long long M, int N, int K, int act);
  int gemm_gw(const float* g, long long M, int N, int K, const float* w, float** dx);
  bool want_planes(long long rows, int C) const;
  int new_planes(long long rows, int C, uint16_t** out);
  int split_input(ConvP* p, const float* x, long long rows, int C, const uint16_t* ready = nullptr);
  int pack_weight(const float* w, int O, int I, int KH, int KW, float* buf);
  int weight_operand(float* buf, size_t wn, int O, ConvP* p);
  int colreduce_part(ColRedP p, int* chunks);
  int colreduce2(const ColRedP& p, float* out0, float* out1);
  int colsum(const float* a, long long R, int C, float* dst);
  int wgrad(const float* a, int lda, const float* b, int ldb, long long P, int M, int N, int taps, const Node::Conv* geom,
            const TT* xin, const TT* yout, float* dst, int layout, const uint16_t* a_rec = nullptr,
            const uint16_t* b_rec = nullptr);
  int linear_grads(const std::string& wk, const std::string& bk, const float* g, int ldg, const float* x, int ldx, long long P,
                   int N, int K, int woff = 0, bool bias_first = false);
  hipError_t add_rows_each(const float* a, size_t lda, const float* b, size_t ldb, float* out, int B, int n);
  int add_grad(int id, float* g);
  int own_grad(int id);
  int new_mask(size_t n, const uint8_t** m, float p = -1.f);
  template <class F> int grad_to(int id, F launch);
  int push(Node& n, int out);
  template <class F> int map_node(Node n, int* out, F launch);

  // ---- operations (train.hip): each forward builder appends one node; its bwd_* follows it in the file
  int conv_bn(int in, const std::string& wkey, const std::string& bnkey, int Cout, int KH, int KW, int SH, int SW, int PH,
              int PW, bool relu, int res, int* out, int OH = -1, int OW = -1);
  int stem(const float* img, int B, int Cin, int H, int W, int Cout, const std::string& wkey, const std::string& bnkey, int* out);
  int bn_forward(Node::Conv& n, long long P);
  int bwd_conv(const Node& n);
  int pool(int in, int SH, int SW, int PH, int PW, int* out, int KW = 2);
  int bwd_pool(const Node& n);
  int mean_h(int in, int* out);
  int bwd_mean_h(const Node& n);
  int linear(int in, const std::string& key, int N, int K, int woff, int act, int res, int* out, float* into = nullptr,
             bool bias = true);
  int bwd_linear(const Node& n);
  int layernorm(int in, const std::string& key, float eps, int* out, float* into = nullptr);
  int bwd_ln(const Node& n);
  int attention(int qt, int qoff, int kvt, int koff, int voff, int nb, int Lq, int Lk, int heads, int hd, int causal,
                const int64_t* keytok, int* out, bool attn_dropout = false, const uint8_t* given_mask = nullptr,
                float given_scale = 1.f);
  int bwd_attn(const Node& n);
  int dropout(int in, int* out, float p = -1.f);
  int bwd_dropout(const Node& n);
  int add(int a, int b, int* out);
  int bwd_add(const Node& n);
  int gelu(int in, int* out);
  int bwd_gelu(const Node& n);
  int relu(int in, int* out);
  int bwd_relu(const Node& n);
  int add_const(int in, const float* table, int* out);
  int bwd_add_const(const Node& n);
  int gc_pool(int in, const std::string& key, int* out);
  int bwd_gc_pool(const Node& n);
  int bcast_add(int in, int y, int* out);
  int bwd_bcast_add(const Node& n);
  int tokens(int patch, const std::string& p, int gh, int gw, int* out);
  int bwd_tokens(const Node& n);
  int embed(const int64_t* tgt, int B, int L, const std::string& p, int* out);
  int bwd_embed(const Node& n);
  int bilstm(int in, int layer, const std::string& key, int B, int T, int* out);
  int bwd_bilstm(const Node& n);
  int lstm_head(int mem, int kp, const int64_t* tgt, int B, int S, float* logits, int* out);
  int bwd_lstm(const Node& n);
  int backward();

  // ---- networks (train_models.hip)
  int global_context(int in, const std::string& key, int* out);
  int backbone(const float* img, int B, int H, int W, const std::string& p, int* out);
  int vgg(const float* img, int B, int H, int W, const std::string& p, int* out);
  int bilstm_layer(int in, int layer, const std::string& key, int B, int T, int* out);
  int vit(int feat, const std::string& p, int* out, float* into);
  int linear_res(int in, const std::string& key, int N, int K, int res, int* out);
  int decoder(int mem, const int64_t* tgt, int B, int L, const std::string& p, float* logits, int* out);
  int lstm_decoder(int mem, const int64_t* tgt, int B, int S, float* logits, int* out);
};

}  // namespace tape
#pragma GCC visibility pop

struct d2t_train_state {
  // d2t_train_gather: copy-table staging (pinned + device mirror), four sets in rotation so that the host waits for an
  // upload queued four calls ago, never for the work just ahead of it
  struct GatherStage { void *h = nullptr, *d = nullptr; size_t cap = 0; hipEvent_t ev = nullptr; bool pending = false; } gather[4];
  unsigned gather_calls = 0;
  tape::Arena tape;
  std::vector<tape::TT> t;
  std::vector<tape::Node> nodes;
  std::map<std::string, float*> grads;  // persistent, one buffer per trainable parameter
  std::map<std::string, hipEvent_t> ready;  // recorded on the compute stream after the last kernel that writes a gradient
  std::vector<std::string> touched;         // gradients written by the node being processed
  float* part = nullptr; size_t part_cap = 0;   // wgrad / column-reduction partial sums
  float* scratch = nullptr; size_t scratch_cap = 0;
  const int64_t* tgt = nullptr;
  const float* image = nullptr;
  // dropout of nn.TransformerDecoderLayer (d2t_train_set_dropout): Philox masks keyed by (seed, forward call, site)
  float drop_p = 0.f;
  unsigned long long drop_seed = 0, drop_calls = 0, drop_site = 0;
  std::vector<uint8_t> teacher_flags;  // d2t_train_set_teacher_flags (scheduled sampling of the LSTM head); empty = all teacher
  std::vector<std::pair<const uint8_t*, size_t>> masks;  // in creation order (d2t_train_read_mask)
  int B = 0, H = 0, W = 0, L = 0;
  int logits_id = -1;
  bool have_forward = false;
  bool poison = false;  // test entries: every Tr::alloc block starts as 0xFF bytes (NaN), filled on the stream
  ~d2t_train_state() {
    tape.release();
    for (auto& kv : grads) hipFree(kv.second);
    for (auto& kv : ready) hipEventDestroy(kv.second);
    for (auto& g : gather) {
      if (g.h) hipHostFree(g.h);
      if (g.d) hipFree(g.d);
      if (g.ev) hipEventDestroy(g.ev);
    }
    if (part) hipFree(part);
    if (scratch) hipFree(scratch);
  }
};

#define TCHK(expr)                                                                               \
  do {                                                                                           \
    hipError_t e_ = (expr);                                                                      \
    if (e_ != hipSuccess) return fail(c, D2T_EHIP, "%s: %s", #expr, hipGetErrorString(e_));      \
  } while (0)
#define RC(expr)            \
  do {                      \
    int rc_ = (expr);       \
    if (rc_) return rc_;    \
  } while (0)
