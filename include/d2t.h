/*
 * libd2t -- C-ABI of the MI355X (gfx950) recognizer engine.
 *
 * Drop-in boundary for the doc2tex `modules.recognizers` forward pass.  The
 * reference is 100 % Python and has no FFI of its own; the entry
 * points below are what a ctypes binding for that path binds, one per reference
 * call site (citations relative to /root/reference/doc2tex/):
 *
 *   d2t_create / d2t_load_weight / d2t_finalize_weights
 *        <- Model.__init__            modules/build_model.py:8-34
 *           load_checkpoint           utils/model_utils.py:136-237 (state_dict names)
 *   d2t_encoder_shape / d2t_encode
 *        <- Model.forward_encoder     modules/build_model.py:36-43
 *           (ResNet.forward resnet.py:205-245, HybridEmbed.forward patchembed.py:115-141,
 *            ViTEncoderV3.forward vit_encoder.py:249-268, SeqModelingBuilder.forward
 *            recognizers/build_seq.py:42-83)
 *   d2t_decode_greedy
 *        <- TransformerPrediction.forward_greedy (eval)  prediction_head/tfm.py:119-143
 *   d2t_decode_attn_greedy
 *        <- Attention.forward_greedy seq2seq.py:224-331, AttentionV2.forward_greedy seq2seq_v2.py:176-293
 *   d2t_decode_beam
 *        <- TransformerPrediction.forward_beam tfm.py:145-186 + Beam tools/beam.py:38-140
 *   d2t_decode_attn_beam
 *        <- Attention.forward_beam seq2seq.py:83-222, AttentionV2.forward_beam seq2seq_v2.py:12-174
 *   d2t_train_forward / d2t_train_backward / d2t_train_grad (+ dropout, scheduled-sampling setters)
 *        <- Model.forward under module.train() and loss.backward(): forward_step / train_one_step
 *           engine/training.py:76-164 (tfm.py:103-118, seq2seq.py:224-331 with is_train)
 *   d2t_decode_greedy_async / d2t_decode_greedy_submit / d2t_decode_attn_greedy_submit[_ragged] / d2t_decode_wait,
 *   d2t_set_reserved_blocks / d2t_set_decode_chains, d2t_decode_beam_batch[_ragged] / d2t_decode_attn_beam_batch
 *        -- serving extensions without a reference counterpart (cross-batch pipelining, batched beam search);
 *           their results equal the corresponding reference-shaped calls bit for bit
 *   d2t_op_*  -- single-kernel entry points used by the parity tests.
 *
 * Conventions
 *   - plain C, no C++ types, no exceptions across the boundary;
 *   - every pointer named *dev* / marked [device] is a raw HIP device pointer
 *     owned by the CALLER (e.g. a torch tensor's data_ptr()); the engine writes
 *     outputs in place and keeps its own packed copies of the weights;
 *   - all tensors fp32, token ids int64; arithmetic fp32 on the matrix cores, or (d2t_set_conv_precision) large
 *     convolutions / GEMMs as three bf16 MFMAs per product with fp32 accumulation (tokens bit-exact, logits within 1e-3);
 *   - every launch goes to the caller's hipStream_t (`stream`, may be NULL for
 *     the default stream); calls are asynchronous unless they return host
 *     scalars (d2t_decode_greedy's steps_out, d2t_decode_beam);
 *   - return value 0 = D2T_OK, otherwise an error code; d2t_last_error(ctx)
 *     gives the message.  The library never aborts and never falls back to
 *     the CPU;
 *   - a ctx is not thread-safe: one ctx per device per process.
 */
#ifndef D2T_H
#define D2T_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct d2t_ctx d2t_ctx;
typedef void* d2t_stream; /* hipStream_t */

enum {
  D2T_OK = 0,
  D2T_EINVAL = 1, /* bad argument / unsupported configuration */
  D2T_ENOMEM = 2, /* device allocation failed */
  D2T_EHIP = 3,   /* HIP runtime error */
  D2T_ESTATE = 4  /* call order (weights missing / not finalized) */
};

enum {
  D2T_ENC_RESNET = 0,        /* Feat=ResNet, Seq=None (+PositionalEncoding2D)          -> TFM decoder   */
  D2T_ENC_HYBRID_VIT = 1,    /* Seq=ViT over the ResNet backbone (HybridEmbed)                          */
  D2T_ENC_VGG_BILSTM = 2,    /* Feat=VGG,    height-mean | proj_feat, 2x BidirectionalLSTM -> Attn | TFM (d_model 256) */
  D2T_ENC_RESNET_BILSTM = 3, /* Feat=ResNet, height-mean | proj_feat, 2x BidirectionalLSTM                          */
  D2T_ENC_VGG = 4            /* Feat=VGG, Seq=None (+PositionalEncoding2D)              -> TFM decoder   */
};
enum { D2T_DEC_TFM = 0, D2T_DEC_ATTN = 1 };
/* d2t_config.attn_keys: which memory tokens the LSTM-attention decoder attends to / starts from */
enum {
  D2T_ATTN_KEYS_ALL_INIT_MEAN = 0,  /* Attention / AttentionV2 on a BiLSTM encoder (seq2seq.py:229-233)     */
  D2T_ATTN_KEYS_NOCLS_INIT_CLS = 1, /* AttentionV2 with seqmodel='TFM' (seq2seq_v2.py:182-199): shipped YAMLs */
  D2T_ATTN_KEYS_ALL_INIT_FIRST = 2  /* Attention (v1) on a non-BiLSTM encoder (seq2seq.py:234-236)          */
};

/* Activation codes of d2t_op_conv2d. */
enum { D2T_ACT_NONE = 0, D2T_ACT_RELU = 1, D2T_ACT_GELU = 2 };

enum { D2T_ATTN_CELL_LOCATION = 0, D2T_ATTN_CELL_BAHDANAU = 1 };
/* How the ViT encoder's position table meets a crop whose patch grid differs from max_dimension's
 * (create_vit_modeling, seq_modeling/vit_encoder.py:295-302):
 *   SINCOS_PREFIX   fix_embed: True -> ViTEncoderV3 (:229-268): frozen sincos table, flat prefix slice pos_embed[:, :N+1]
 *   LEARNED_INTERP  default -> ViTEncoder (:22-118): learned table, resized to the crop's grid by bicubic interpolation
 *                   (F.interpolate, align_corners False, scale factors (gh + 0.1) / GH, (gw + 0.1) / GW, :58-95); the table
 *                   itself when the grids agree (or the token counts agree and the padded feature map is square, :66-67)
 *   LEARNED_PREFIX  interpolate_embed: False -> ViTEncoderV2 (:207-226): learned table, flat prefix slice
 * The first and the last are the same arithmetic in inference; in training the learned tables receive gradients. */
enum { D2T_VIT_POS_SINCOS_PREFIX = 0, D2T_VIT_POS_LEARNED_INTERP = 1, D2T_VIT_POS_LEARNED_PREFIX = 2 };

typedef struct d2t_config {
  int32_t encoder;      /* D2T_ENC_*: Feat=ResNet+Seq=None  |  Seq=ViT (hybrid) */
  int32_t in_channels;  /* 1 (grey crops) or 3 (rgb: True) */
  int32_t backbone_out; /* ResNet output_channel, 512 */
  int32_t vit_depth, vit_heads, vit_dim; /* ViT blocks / heads / hidden_size */
  int32_t patch_h, patch_w;              /* patch_size */
  int32_t max_h, max_w;                  /* max_dimension: sizes the sincos pos-embed grid */
  int32_t dec_dim, dec_heads, dec_layers, dec_ff; /* TFM d_model / nhead / layers / dim_feedforward */
  int32_t vocab;        /* num_class */
  int32_t max_seq_len;  /* Prediction.params.max_seq_len */
  /* appended in v2 of the struct: recurrent model family */
  int32_t decoder;          /* D2T_DEC_* */
  int32_t attn_hidden;      /* Attn hidden_size (= input_size = embed dim), 256 */
  int32_t attn_kernel_size; /* location filter half width: Conv1d kernel = 2*k+1 */
  int32_t attn_kernel_dim;  /* location filter channels */
  int32_t attn_keys;        /* D2T_ATTN_KEYS_* */
  int32_t attn_enc_init;    /* enc_init: initial (h,c) projected from the encoder output */
  int32_t attn_coverage;    /* 1 = attn_type 'coverage' (accumulated alignment), 0 = 'loc_aware' */
  int32_t bilstm_hidden;    /* SequenceModeling.params.hidden_size of the BiLSTM, 256 */
  int32_t batch_max_length; /* Attn decoders run batch_max_length + 1 steps */
  int32_t gcb;              /* 1: GlobalContext blocks close the four ResNet stages (gcb: True) */
  /* appended in v3: the other cells / inputs of Attention.__init__ (prediction_head/seq2seq.py:31-53) */
  int32_t attn_cell;        /* D2T_ATTN_CELL_*: location-aware (attn_type 'coverage' | 'loc_aware') or Bahdanau
                               (attention1D.py:71-118: keys "attn.i2h / attn.h2h / attn.score", no alignment memory) */
  int32_t attn_onehot;      /* 1 = embed_target False: the decoder input is the one-hot vector of the previous token
                               (seq2seq.py:72-78), rnn.weight_ih is [4H][H + num_class] and there is no embedding table */
  /* appended in v4: the ViT encoder variants beside ViTEncoderV3 */
  int32_t vit_pos;          /* D2T_VIT_POS_* */
  /* appended in v5: mean_height False (recognizers/build_feat.py:16,33-40,56-61) */
  int32_t proj_height;      /* 1: a BiLSTM encoder reads proj_feat = Linear(3 * C -> C) over the [b, w, c * h] flattening of the
                               feature map (its height must be 3: 64-pixel crops) instead of the mean over the height */
} d2t_config;

/* Largest num_class (d2t_config.vocab) of the LSTM-attention decoders: d2t_create refuses more.  probs [B][S][vocab] fp32
 * stays caller memory (2.1 GB at B = 64, S = 501 and this cap). */
#define D2T_ATTN_MAX_CLASSES 16384

/* ---- lifecycle ----------------------------------------------------------
 * d2t_create binds the context to the HIP device that is current for the calling thread (the reference picks its
 * device from the string opt["device"], build_pred.py:17 -- the Python layer above translates "cuda:N" into
 * hipSetDevice(N) around this call).  Every stream, event and buffer of the context lives on that device and every
 * later call switches to it on entry and restores the caller's device on return, so two contexts on two GPUs can be
 * driven from one thread.  Caller buffers on another device are rejected with D2T_EINVAL. */
int d2t_create(const d2t_config* cfg, d2t_ctx** out);
void d2t_destroy(d2t_ctx* ctx);
const char* d2t_last_error(const d2t_ctx* ctx);
/* HIP device index the context was created on (-1 for a null ctx). */
int d2t_device_of(const d2t_ctx* ctx);
/* 1 if a HIP device is usable from this process, else 0 (no ctx needed). */
int d2t_device_available(void);

/* ---- weights -------------------------------------------------------------
 * One call per state_dict entry, `name` being the reference's key (e.g.
 * "seqmodeler.SequenceModeling.blocks.0.attn.qkv.weight").  `dev` is fp32
 * [device], contiguous, `shape[ndim]` its torch shape.  Integer entries
 * (num_batches_tracked) and tables the engine rebuilds itself are ignored.
 * d2t_finalize_weights folds eval-BatchNorm into the convolutions, packs
 * everything into the engine's layouts and fails if an entry is missing.  It
 * may be called again after further d2t_load_weight calls (re-pack). */
int d2t_load_weight(d2t_ctx* ctx, const char* name, const float* dev, const int64_t* shape, int32_t ndim,
                    d2t_stream stream);
int d2t_finalize_weights(d2t_ctx* ctx, d2t_stream stream);

/* ---- encoder -------------------------------------------------------------
 * d2t_encoder_shape: host-only; token count T, feature dim d, patch grid
 * (grid_h, grid_w; the backbone feature map size for the ResNet encoder) and
 * HybridEmbed's (pad_w, pad_h) for an H x W crop.
 * d2t_encode: image [B,in_channels,H,W] fp32 in [-1,1] [device] (NCHW planar; in_channels
 * is the config's, 1 or 3) -> memory [B,T,d] [device, caller-allocated].  d2t_encode_attn
 * and d2t_train_forward take the same image layout. */
int d2t_encoder_shape(const d2t_ctx* ctx, int32_t H, int32_t W, int32_t* T, int32_t* d, int32_t* grid_h,
                      int32_t* grid_w, int32_t* pad_w, int32_t* pad_h);
int d2t_encode(d2t_ctx* ctx, const float* image_dev, int32_t B, int32_t H, int32_t W, float* memory_dev,
               d2t_stream stream);
/* d2t_encode plus the ViT self-attention probabilities of chosen blocks (what the reference's `attn_drop` modules see,
 * vision_transformer.py:74-76): maps_dev (host array) holds n_maps = 0 or vit_depth device pointers; entry i, if not
 * NULL, receives block i's softmax(q k^T / sqrt(32)) as contiguous fp32 [B][heads][T][T] (key innermost, caller-allocated,
 * B*heads*T*T*4 bytes).  NULL entries cost nothing; memory is bitwise the same as without maps.  A non-NULL entry on an
 * encoder without self-attention (ResNet, VGG / ResNet + BiLSTM) is refused with D2T_EINVAL.  n_maps 0 = d2t_encode. */
int d2t_encode_attn(d2t_ctx* ctx, const float* image_dev, int32_t B, int32_t H, int32_t W, float* memory_dev,
                    float* const* maps_dev, int32_t n_maps, d2t_stream stream);

/* ---- greedy decode -------------------------------------------------------
 * memory [B,T,d]; start_tokens [B] int64 ([GO]).  Runs up to max_seq_len+1
 * steps with a KV cache; rows that emitted [s] keep generating until the whole
 * batch has ended (reference semantics).  If is_test != 0 the step count is
 * the first step at which every row has emitted [s] (tfm.py:138-140),
 * otherwise max_seq_len+1.
 * tokens_dev [B, max_seq_len+1] int64 and logits_dev [B, max_seq_len+1, vocab]
 * fp32 are written for steps [0, *steps_out); entries beyond are unspecified.
 * Synchronises `stream` before returning (steps_out is a host scalar). */
int d2t_decode_greedy(d2t_ctx* ctx, const float* memory_dev, int32_t B, int32_t T, const int64_t* start_tokens_dev,
                      int32_t is_test, int64_t* tokens_dev, float* logits_dev, int32_t* steps_out,
                      d2t_stream stream);

/* ---- LSTM-attention greedy decode (Attn / Attnv2 heads, eval mode) ----------
 * Attention.forward_greedy (prediction_head/seq2seq.py:224-331), AttentionV2.forward_greedy
 * (seq2seq_v2.py:176-293) with is_train = False.  memory [B,T,256]; runs batch_max_length+1 steps in one
 * launch.  tokens_dev [B,S] int64, probs_dev [B,S,V] fp32 (S = batch_max_length+1) are always full size;
 * with is_test != 0 everything after the first step at which all rows emitted [s] is zeroed, as the
 * reference leaves its pre-zeroed `probs` untouched after the early break. */
int d2t_decode_attn_greedy(d2t_ctx* ctx, const float* memory_dev, int32_t B, int32_t T, int32_t is_test,
                           int64_t* tokens_dev, float* probs_dev, int32_t* steps_out, d2t_stream stream);

/* d2t_decode_attn_greedy plus the alignment of every step (the reference's `alpha_stores` with viz_attn,
 * seq2seq.py:267-272,300-301): alpha_dev [B][S][Tk] fp32, Tk = T - 1 for the Attnv2 + TFM key mode (the cls row is not
 * a key) and T otherwise.  With is_test the steps after the early exit are zeroed like probs.  alpha_dev NULL =
 * d2t_decode_attn_greedy. */
int d2t_decode_attn_greedy_alpha(d2t_ctx* ctx, const float* memory_dev, int32_t B, int32_t T, int32_t is_test,
                                 int64_t* tokens_dev, float* probs_dev, float* alpha_dev, int32_t* steps_out,
                                 d2t_stream stream);

/* Pipelined variant: always runs max_seq_len+1 steps (is_test = 0 semantics) and returns as soon as the
 * work is enqueued, so the caller can start encoding the next batch while this one decodes (the decode
 * loop is latency-bound and leaves most CUs idle).  tokens_dev / logits_dev / start_tokens_dev must stay
 * alive and untouched until d2t_decode_wait: it makes `stream` wait for every outstanding decode
 * (and, if host_sync != 0, blocks the host until they are complete). */
/* Decode groups: B need not be one encoder batch.  A serving loop may collect the memories of several consecutive batches
 * in one buffer and decode their rows with ONE call -- the step loop's duration hardly depends on the row count, and every
 * row's result is bit-identical to its single-batch decode (doc2tex_amd.Model.decode_group does exactly this).  Two forms:
 *   d2t_decode_greedy_submit         UNIFORM group: every batch has the same row count (rows_per_batch) and the same memory
 *                                    length T; memory_dev is [B][T][d];
 *   d2t_decode_greedy_submit_ragged  RAGGED group: batch i has batch_rows[i] rows and memory length batch_T[i] (crops of
 *                                    different sizes); memory_dev is the batches' memories packed back to back,
 *                                    [sum_i batch_rows[i] * batch_T[i]][d] (Model.decode_group_mixed). */
int d2t_decode_greedy_async(d2t_ctx* ctx, const float* memory_dev, int32_t B, int32_t T,
                            const int64_t* start_tokens_dev, int64_t* tokens_dev, float* logits_dev, d2t_stream stream);
int d2t_decode_wait(d2t_ctx* ctx, d2t_stream stream, int32_t host_sync);
/* Serving tickets.  Every d2t_decode_greedy_async call is numbered 1, 2, 3, ... (d2t_decode_last_ticket returns the
 * number of the most recent one, 0 before the first).  d2t_decode_wait_ticket orders `stream` (and the host, if
 * host_sync != 0) after THAT decode only -- a consumer of batch i need not wait for batches i+1, i+2 that are already
 * in flight; d2t_decode_query polls: 1 complete, 0 still running, < 0 error (-D2T_E*).  The output buffers of a decode
 * belong to the engine until its ticket is complete: a caller that recycles buffers checks the ticket first. */
/* The general asynchronous entry point: as d2t_decode_greedy_async, plus
 *   is_test != 0       the reference's early exit (tfm.py:138-140) decided ON THE DEVICE: the whole step loop is still one
 *                      graph launch, but once every batch of the group has emitted [s] in all its rows the remaining
 *                      kernels return at their first instruction; d2t_decode_steps then reports, per batch, the first step
 *                      at which all ITS rows had ended (entries of tokens / logits beyond it are unspecified);
 *   rows_per_batch     > 0: the B rows are B / rows_per_batch encoder batches of that many rows (a decode group, at most
 *                      64 batches); 0: one batch.
 * *ticket_out (optional) receives the decode's ticket. */
int d2t_decode_greedy_submit(d2t_ctx* ctx, const float* memory_dev, int32_t B, int32_t T, const int64_t* start_tokens_dev,
                             int32_t is_test, int32_t rows_per_batch, int64_t* tokens_dev, float* logits_dev,
                             d2t_stream stream, int64_t* ticket_out);
/* A decode group whose batches differ in row count and memory length (d_model 256 / 8 heads, the absorbed cross-attention:
 * each row reads its own slice of the packed memory rows, so it is bit-identical to its single-batch decode).
 *   memory_dev         [sum_i batch_rows[i] * batch_T[i]][d], batch after batch, each batch [rows][T][d];
 *   batch_rows/batch_T HOST arrays [n_batches] (1 .. 64 batches, every entry >= 1, batch_T[i] <= 4096); read before the call
 *                      returns;
 *   start_tokens_dev   [B], tokens_dev [B][S], logits_dev [B][S][V] with B = sum_i batch_rows[i], rows in batch order.
 * is_test, tickets, d2t_decode_steps (one entry per batch) and the PAD / zero output behind the group's stop step are those
 * of d2t_decode_greedy_submit.  The captured step loop depends on B alone: lengths, offsets and the batch layout are read
 * from engine-owned device tables (filled on `stream` by an asynchronous copy), so any mix with the same row total replays
 * one graph.  Refused before anything is enqueued (D2T_EINVAL unless stated): no batch / no row, more than 64 batches, a
 * batch without rows, a memory length < 1 or > 4096, a pointer of another device; a context without the TFM decoder
 * (D2T_ESTATE); a decoder with projected cross K/V (d_model 512: D2T_ESTATE -- its K/V layout depends on T; decode such
 * batches with d2t_decode_greedy_submit, one group per size). */
int d2t_decode_greedy_submit_ragged(d2t_ctx* ctx, const float* memory_dev, int32_t n_batches, const int32_t* batch_rows,
                                    const int32_t* batch_T, const int64_t* start_tokens_dev, int32_t is_test,
                                    int64_t* tokens_dev, float* logits_dev, d2t_stream stream, int64_t* ticket_out);
/* 1 if this context decodes ragged groups (d2t_decode_greedy_submit_ragged: TFM decoder whose cross-attention reads the
 * encoder memory itself), 0 if that entry point refuses (LSTM-attention heads; projected cross K/V, d_model 512).  Valid
 * once the weights are finalized. */
int32_t d2t_decode_supports_ragged(const d2t_ctx* ctx);
/* Captured decode loops the context currently holds (at most 40, least recently used evicted). */
int32_t d2t_decode_graph_count(const d2t_ctx* ctx);
/* The LSTM-attention heads (Attn / Attnv2) through the same serving machinery: d2t_decode_attn_greedy[_alpha] without
 * the wait.  The key projection, the one-launch step loop and a small finalize kernel are enqueued on the stream of one of
 * the d2t_set_decode_chains chains (they take turns), ordered behind `stream` by an event; the call returns once that is
 * done and never synchronises the host.  Every chain has its own key-projection workspace and state block, so up to
 * `chains` decodes are in flight side by side.
 *   is_test != 0   the reference's early exit (seq2seq.py:224-331, seq2seq_v2.py:176-293), decided inside the kernel: a
 *                  block stops once ALL rows have emitted [s] and its next step lies beyond the largest end step, and the
 *                  finalize kernel zeroes tokens / probs / alpha of the steps behind the exit -- the outputs are those of
 *                  the synchronous call bit for bit, whatever the buffers held before;
 *   alpha_dev      NULL, or [B][S][Tk] as for d2t_decode_attn_greedy_alpha.
 * The decode takes the next ticket of the counter above: d2t_decode_query / d2t_decode_wait_ticket / d2t_decode_wait /
 * d2t_decode_last_ticket work unchanged, and d2t_decode_steps reports ONE entry, the reference's step count
 * (batch_max_length + 1 without is_test, or when some row never emitted [s]).  memory_dev, tokens_dev, probs_dev and
 * alpha_dev belong to the engine until the ticket is complete.  Refuses what the synchronous call refuses (a TFM context:
 * D2T_ESTATE; an unsupported memory length: D2T_EINVAL) before anything is enqueued. */
int d2t_decode_attn_greedy_submit(d2t_ctx* ctx, const float* memory_dev, int32_t B, int32_t T, int32_t is_test,
                                  int64_t* tokens_dev, float* probs_dev, float* alpha_dev, d2t_stream stream,
                                  int64_t* ticket_out);
/* d2t_decode_attn_greedy_submit for SEVERAL encoder batches of different row counts and memory lengths in ONE launch: the
 * one-launch step loop has one block per row, so a bucket of 8 crops keeps 8 compute units busy for the whole loop; the rows
 * of all collected batches fill the chip with the same blocks.  Rows never interact, so every row's tokens and probs are
 * those of its own batch's d2t_decode_attn_greedy_submit call bit for bit.
 *   memory_dev         [sum_i batch_rows[i] * batch_T[i]][256], batch after batch, each batch [rows][T][256];
 *   batch_rows/batch_T HOST arrays [n_batches], read before the call returns;
 *   tokens_dev         [B][S], probs_dev [B][S][V] with B = sum_i batch_rows[i], rows in batch order; no alignment maps.
 * is_test != 0: the early exit is decided per BATCH inside the kernel (one exit word per batch): a batch's rows stop at that
 * batch's stop step whatever the other batches of the launch do, the finalize kernel zeroes tokens / probs of batch k's rows
 * behind ITS stop step, and d2t_decode_steps reports one entry per batch (one entry, batch_max_length + 1, without is_test).
 * The next chain in turn, ordered behind `stream` by an event; one key projection over all packed rows, one loop launch, one
 * finalize launch, one ticket.  The call does not wait for the decode; it may wait for an earlier table upload of the same
 * chain (each chain has two small pinned staging slots that take turns, and a slot is rewritten only once its last upload
 * has run: that upload stands in front of the chain's loop before last).  Refused before anything is enqueued (D2T_EINVAL unless stated): no batch or more
 * than 64 batches, a batch without rows, more than 1024 rows in total, a memory length whose key count lies outside
 * [1, 4096], a pointer of another device, a vocabulary over D2T_ATTN_MAX_CLASSES; a context without the Attn decoder
 * (D2T_ESTATE).  d2t_decode_greedy_submit_ragged and d2t_decode_supports_ragged keep refusing / answering 0 for an Attn
 * context: the two heads' groups are separate entries. */
int d2t_decode_attn_greedy_submit_ragged(d2t_ctx* ctx, const float* memory_dev, int32_t n_batches, const int32_t* batch_rows,
                                         const int32_t* batch_T, int32_t is_test, int64_t* tokens_dev, float* probs_dev,
                                         d2t_stream stream, int64_t* ticket_out);
/* 1 if d2t_decode_attn_greedy_submit_ragged serves this context (a finalized LSTM-attention head), 0 if it refuses. */
int32_t d2t_decode_attn_supports_ragged_greedy(const d2t_ctx* ctx);
/* Step counts of the batches of one asynchronous decode (blocks until it is complete). */
int d2t_decode_steps(d2t_ctx* ctx, int64_t ticket, int32_t* steps_out, int32_t max_batches, int32_t* n_out);
int64_t d2t_decode_last_ticket(const d2t_ctx* ctx);
int d2t_decode_query(d2t_ctx* ctx, int64_t ticket);
int d2t_decode_wait_ticket(d2t_ctx* ctx, int64_t ticket, d2t_stream stream, int32_t host_sync);

/* ---- beam decode (one sample, fresh beam state per call) ------------------
 * memory [1,T,d].  seq_out: HOST buffer of max_seq_len+1 int64; *len_out its
 * used length; *score_out the hypothesis score (tools/beam.py semantics:
 * best = argmax score/len over completed hypotheses).
 * Every single-sample beam call is its batched call with N = 1 (d2t_decode_beam = d2t_decode_beam_batch,
 * d2t_decode_attn_beam = d2t_decode_attn_beam_batch); which loop runs depends on the decoder.  d_model 256 (round 4):
 * Beam.advance (tools/beam.py:68-105) runs on the device -- candidate walk, completed set, row compaction and a
 * (parent, token) history per step in one single-block kernel -- and the whole max_seq_len + 1 step loop is ONE captured
 * graph per (N, T, beam); the host copies one result block back and walks the best hypothesis through the history.  Other
 * TFM decoders (d_model 512), d2t_set_beam_shared_tile(1) and the LSTM-attention heads run a host-side loop with one
 * round trip per step. */
int d2t_decode_beam(d2t_ctx* ctx, const float* memory_dev, int32_t T, int32_t beam_size, int64_t* seq_out,
                    int32_t* len_out, float* score_out, d2t_stream stream);

/* d2t_decode_attn_beam for N samples in one step loop (extension, like d2t_decode_beam_batch).  memory [N][T][256];
 * seq_out (host) [N][batch_max_length + 1]; len_out, score_out (host) [N]. */
int d2t_decode_attn_beam_batch(d2t_ctx* ctx, const float* memory, int32_t N, int32_t T, int32_t beam_size, int64_t* seq_out,
                               int32_t* len_out, float* score_out, d2t_stream stream);
/* ... plus each returned hypothesis's alignment map (the reference's decoder_attn with viz_attn, seq2seq.py:174-221):
 * alpha_dev [N][S][Tk] fp32 (device, 16-byte aligned), row j < len_out[i] = the alignment of step j in the row that was the
 * hypothesis's parent at that step, zeros beyond.  The search keeps every step's alignments in a history of
 * S * N * beam_size * Tk floats beside its workspace; a call whose history would exceed D2T_ATTN_MAP_BUDGET bytes is
 * refused with D2T_EINVAL (split the batch).  alpha_dev NULL = d2t_decode_attn_beam_batch. */
#define D2T_ATTN_MAP_BUDGET (256ull << 20)
int d2t_decode_attn_beam_batch_alpha(d2t_ctx* ctx, const float* memory, int32_t N, int32_t T, int32_t beam_size,
                                     int64_t* seq_out, int32_t* len_out, float* score_out, float* alpha_dev,
                                     d2t_stream stream);

/* d2t_decode_attn_beam_batch[_alpha] for N samples whose memories have DIFFERENT lengths (crops of different sizes), in one
 * step loop: memory_packed_dev [T[0] + .. + T[N-1]][256], sample i's rows behind sample i-1's; T: HOST array [N]; seq_out,
 * len_out, score_out as d2t_decode_attn_beam_batch.  Every sample's sequence, length and score are those of its own
 * d2t_decode_attn_beam_batch call, bit for bit; the loop's batch_max_length + 1 host round trips are paid once for all
 * lengths.  The key projection runs once over the packed rows, the per-sample tables (first row, length) are uploaded once
 * in front of the loop, and the step kernel's ragged build reads them through the row map.
 * alpha_dev: NULL, or [N][S][max Tk] fp32 (device, 16-byte aligned; Tk = T[i], less one where the head drops the cls token
 * from its keys): sample i's map as d2t_decode_attn_beam_batch_alpha returns it in columns [0, Tk_i), zeros behind.  The
 * history is S * N * beam_size * max Tk floats and held to D2T_ATTN_MAP_BUDGET.
 * Refused before anything is enqueued (D2T_EINVAL unless stated): N < 1 or N > 1024, a length with Tk < 1 or Tk > 4096,
 * beam_size outside [1, 16], a history over the budget, a pointer of another device; a context without the Attn decoder
 * (D2T_ESTATE); the 'loc_aware' cell (D2T_ESTATE, as the uniform call). */
int d2t_decode_attn_beam_batch_ragged(d2t_ctx* ctx, const float* memory_packed_dev, int32_t N, const int32_t* T,
                                      int32_t beam_size, int64_t* seq_out, int32_t* len_out, float* score_out, float* alpha_dev,
                                      d2t_stream stream);
/* 1 if d2t_decode_attn_beam_batch_ragged serves this context, 0 if it refuses with D2T_ESTATE.  Valid once the weights are
 * finalized. */
int32_t d2t_decode_attn_supports_ragged_beam(const d2t_ctx* ctx);

/* Beam search for N samples at once (not in the reference, whose forward_beam is single-sample): the same results as
 * N calls of d2t_decode_beam, with the hypotheses of all samples advanced by one shared step loop.  memory [N][T][d];
 * seq_out (host) [N][max_seq_len + 1]; len_out, score_out (host) [N]. */
int d2t_decode_beam_batch(d2t_ctx* ctx, const float* memory, int32_t N, int32_t T, int32_t beam_size, int64_t* seq_out,
                          int32_t* len_out, float* score_out, d2t_stream stream);

/* d2t_decode_beam_batch for N samples whose memories have DIFFERENT lengths (crops of different sizes), in one step loop:
 * memory_packed_dev [T[0] + .. + T[N-1]][d], sample i's rows behind sample i-1's; T: HOST array [N]; outputs as
 * d2t_decode_beam_batch.  Every sample's sequence, length and score are those of its own d2t_decode_beam call, bit for bit.
 * The captured loop depends on N and beam_size alone: lengths and offsets are read from engine-owned per-sample device
 * tables (filled on `stream` by an asynchronous copy in front of the loop), so any mix of lengths with the same N and beam
 * replays one graph.  Refused before anything is enqueued (D2T_EINVAL unless stated): N < 1 or N > 1024, a length < 1 or
 * > 4096, beam_size outside [1, 16], beam_size * vocab over d2t_decode_beam_batch's cap, a pointer of another device; a
 * context without the TFM decoder (D2T_ESTATE); a context whose beam search does not run on the device -- d_model 512,
 * d2t_set_beam_shared_tile(1), max_seq_len + 2 > 512 (D2T_ESTATE: call d2t_decode_beam_batch once per length). */
int d2t_decode_beam_batch_ragged(d2t_ctx* ctx, const float* memory_packed_dev, int32_t N, const int32_t* T, int32_t beam_size,
                                 int64_t* seq_out, int32_t* len_out, float* score_out, d2t_stream stream);
/* 1 if d2t_decode_beam_batch_ragged serves this context, 0 if it refuses with D2T_ESTATE.  Valid once the weights are
 * finalized; follows d2t_set_beam_shared_tile. */
int32_t d2t_decode_supports_ragged_beam(const d2t_ctx* ctx);
/* The table arithmetic of d2t_decode_beam_batch_ragged (host only, no context): row0_out[i] = T[0] + .. + T[i-1],
 * len_out[i] = T[i] (either may be NULL); returns the packed row total. */
int64_t d2t_ragged_beam_tables(int32_t N, const int32_t* T, int32_t* row0_out, int32_t* len_out);

/* Cross-attention maps of the TFM decoder: which memory tokens every generated token looked at.  A teacher-forced replay
 * of the step loop over tokens the caller already has (a greedy decode's, a beam hypothesis'): step t < S is fed
 * tokens_in[b][t] (device, [B][S]; column 0 = the start token) instead of an argmax, and the softmax(q . K^T / sqrt(hd))
 * of its cross-attention query over the T memory tokens is written as row t -- the attention of the query that produced
 * token t + 1.  No early exit; every id must lie inside the vocabulary (read back and checked).
 *   per_head == 0: maps [B][nl][S][T], the mean over the 8 heads summed in head order (torch's average_attn_weights)
 *   per_head != 0: maps [B][nl][8][S][T]
 * nl = popcount(layer_mask), the chosen layers (bit l = decoder layer l) in ascending order.  fp32; rows sum to 1.
 * The replay always runs the projected-K/V form of the row work, in fp32 throughout (the K / V projection of the memory too,
 * whatever d2t_set_conv_precision says), in buffers of its own and with plain launches on `stream`:
 * it changes no setting, memory slot or captured loop of the context, so decodes before and after it are what they are
 * without it; it does not wait for decodes in flight either (it shares nothing with them).  Synchronous: returns once the
 * maps are complete.  Roughly the cost of one more decode of S steps, without its vocabulary GEMM.
 * Refused before anything is enqueued: a context without the TFM decoder (D2T_ESTATE); S outside [1, max_seq_len + 1], T
 * outside d2t_decode_greedy's range, B > 65535, an empty layer_mask or a bit at or above dec_layers, a pointer of another
 * device, maps larger than D2T_ATTN_MAP_BUDGET bytes ("split the batch"), a token id outside the vocabulary (D2T_EINVAL). */
int d2t_decode_cross_attention(d2t_ctx* ctx, const float* memory_dev, int32_t B, int32_t T, const int64_t* tokens_in_dev,
                               int32_t S, uint32_t layer_mask, int32_t per_head, float* maps_dev, d2t_stream stream);

/* LSTM-attention beam search for ONE sample (reference: Attention.forward_beam, prediction_head/seq2seq.py:83-222;
 * AttentionV2.forward_beam, seq2seq_v2.py:12-174 -- what config/test.yaml runs with beam_size 5 / 10).  Coverage
 * attention only.  memory [1][T][256]; seq_out (host, >= batch_max_length + 1 entries) receives the token ids without
 * the leading [GO]; *score_out the reference's returned score.  1 <= beam_size <= 16.  d2t_decode_attn_beam_batch with
 * N = 1. */
int d2t_decode_attn_beam(d2t_ctx* ctx, const float* memory, int32_t T, int32_t beam_size, int64_t* seq_out,
                         int32_t* len_out, float* score_out, d2t_stream stream);

/* ---- LSTM-attention beam search with the bookkeeping on the device ----------------------------------------------
 * The searches above run a host loop: one device -> host copy, one synchronisation and one upload per step.  The
 * device-side loop keeps the reference's hypothesis bookkeeping in a record on the device (AttnBeamDev), runs the step
 * kernel for all N x beam row slots under a guard on the live row count, and is one captured graph per (N, beam, row
 * stride capacity, maps on / off) -- no host round trip inside the search, so it can also be SUBMITTED.  Same results as the
 * host loop, bit for bit.  The row stride of its state and history is the largest Tk rounded up to 256, so searches whose
 * longest memories share that capacity replay one graph.
 *
 * d2t_decode_attn_supports_device_beam: 1 for an Attn context whose beam search exists (coverage / Bahdanau cells).
 * d2t_set_attn_beam_device(ctx, 1): d2t_decode_attn_beam, _batch, _batch_alpha and _batch_ragged run the device-side loop
 * (default 0: the host loop).  D2T_ESTATE where the context has no device-side search.
 * d2t_decode_attn_beam_device_runs: searches this context has run on the device-side loop (synchronous or submitted).
 *
 * d2t_decode_attn_beam_batch_submit: d2t_decode_attn_beam_batch_ragged without the wait (equal lengths are the uniform
 * case).  packed [sum T][256] and every output are DEVICE buffers: seq_dev [N][S] (zeros beyond a sample's length),
 * len_dev [N], score_dev [N], alpha_dev NULL or [N][S][max Tk]; T is a host array.  The decode chains take turns
 * (d2t_set_decode_chains); the search runs on its chain's stream behind the caller's stream and the call returns once it is
 * enqueued.  The outputs are complete once *ticket_out is (d2t_decode_query / d2t_decode_wait_ticket); d2t_decode_steps then
 * reports ONE entry, the steps the search executed.  `packed` may be released once the call has returned and the caller's
 * stream work in front of it has run (the search reads its own copy).  Refusals are those of
 * d2t_decode_attn_beam_batch_ragged, made before anything is enqueued; the context stays usable. */
int32_t d2t_decode_attn_supports_device_beam(const d2t_ctx* ctx);
int d2t_set_attn_beam_device(d2t_ctx* ctx, int32_t on);
int64_t d2t_decode_attn_beam_device_runs(const d2t_ctx* ctx);
int d2t_decode_attn_beam_batch_submit(d2t_ctx* ctx, const float* packed, int32_t N, const int32_t* T, int32_t beam_size,
                                      int64_t* seq_dev, int32_t* len_dev, float* score_dev, float* alpha_dev, d2t_stream stream,
                                      int64_t* ticket_out);

/* ---- convolution arithmetic ------------------------------------------------
 * D2T_CONV_FP32   exact fp32 on v_mfma_f32_32x32x2_f32.
 * D2T_CONV_BF16X3 (default of d2t_create, as of doc2tex_amd.Model) backbone / patch-embed convolutions on the bf16 matrix cores with each fp32 operand
 *                 split into two bf16 (a_hi*b_hi + a_hi*b_lo + a_lo*b_hi, fp32 accumulate): ~2^-17 relative
 *                 product error, measured logits error 2.4e-5 against the 1e-3 budget.  Takes effect at the
 *                 next d2t_encode.
 * D2T_CONV_FP16X2 (opt-in) the backbone's feature maps are kept as fp16 (11 significant bits, rounded once where a layer stores
 *                 them) and its split-record convolutions multiply them with the weights split into fp16 hi + fp16 lo
 *                 (x*w_lo + x*w_hi, fp32 accumulate): two matrix instructions per product instead of three.  Greedy tokens
 *                 exact and |dlogit| <= 1e-3 on the reference fixtures of the HybridViT / LSTM-head stacks (measured
 *                 1.2e-4 .. 2.1e-4 on the benchmark configs), with a 5x instead of a 20x margin -- and NOT on the ResNet-only
 *                 stacks (up to 9e-3): DESIGN.md section 3.  Everything that takes fp32 input (ViT linears, decoder) is as in
 *                 D2T_CONV_BF16X3.  Needs conv kernel 3 (d2t_set_conv_kernel).
 * D2T_CONV_MIXED  (round 4, opt-in) D2T_CONV_BF16X3 with the two-MFMA fp16 arithmetic of D2T_CONV_FP16X2 in the first
 *                 D2T_MIXED_UNITS_DEFAULT of the backbone's eight plain 512 -> 512 units [layer3.1, layer3.2, layer3.3,
 *                 layer3.4, conv3, layer4.0, layer4.1, layer4.2] (resnet.py:32-48, 205-245; the K = 4608 layers) and nothing
 *                 else.  The tensors entering / leaving those units are stored as fp16 hi | fp16 lo pairs (22 bits), so the
 *                 residual stream keeps its precision and only the MFMA's activation operand is rounded to 11 bits.  The error
 *                 of the logits grows with the square root of the number of two-MFMA layers (DESIGN.md section 3,
 *                 tools/probe/fp16x2_sim.py); d2t_set_mixed_units changes the count (0 .. 8; 0 = D2T_CONV_BF16X3). */
enum { D2T_CONV_FP32 = 0, D2T_CONV_BF16X3 = 1, D2T_CONV_FP16X2 = 2, D2T_CONV_MIXED = 3 };
#define D2T_MIXED_UNITS_DEFAULT 3
int d2t_set_conv_precision(d2t_ctx* ctx, int32_t mode);
int d2t_set_mixed_units(d2t_ctx* ctx, int32_t units);

/* Pipelined serving: the split-bf16 convolution is a persistent kernel; capping its grid at
 * (2 x CUs - blocks) leaves `blocks` block slots free at all times, into which the latency-bound decode
 * kernels of the previous batch (running on the engine's high-priority stream) are placed without waiting
 * for a convolution block to retire.  0 (default) = use every slot. */
int d2t_set_reserved_blocks(d2t_ctx* ctx, int32_t blocks);

/* The split-bf16 convolution kernel of the layers with at least 128 output channels.  kind 3 (default): the pipelined
 * 256x128 kernel on v_mfma_f32_16x16x32_bf16 -- ONE persistent block per CU holding three LDS stages, LDS-DMA two K-steps
 * ahead behind counted waits, grid = (CUs - d2t_set_reserved_cus) -- with the fused max-pools / shortcuts and the fp16x2 /
 * mixed arithmetic built on it.  kind 0: the 128x128 kernel on 32x32x16 MFMAs with two blocks per CU (the kernel of the
 * narrower layers; d2t_set_reserved_blocks applies to it).  Same three products per element in the same order in both; the
 * sum inside an MFMA spans 32 k in kind 3 and 16 in kind 0, so the two agree to fp32 rounding, not bit for bit; all rows of
 * a layer always run on one kind.  (Rounds 1-3 exported five more variants here; they were A/B arms and left in round 4.) */
int d2t_set_conv_kernel(d2t_ctx* ctx, int32_t kind);
/* Validation switches (tests): pools = 0 runs the two 2x2 max-pools as their own kernels instead of inside the epilogue of the
 * convolution in front of them, shortcuts = 0 the BasicBlocks' 1x1 shortcuts as their own launches instead of inside conv2's.
 * Pooled values are bit-identical either way; the shortcut sum forms in another order (fp32 rounding).  Default: both fused. */
int d2t_set_conv_fusion(d2t_ctx* ctx, int32_t pools, int32_t shortcuts);
/* Beam search of the d_model-256 TFM decoder, cross-attention: 0 (default) one block per hypothesis row, each reading its
 * sample's memory rows; 1: one block per SAMPLE that stages the sample's memory tiles in LDS once per layer and step for
 * all its live hypotheses (beam <= 6; decode_beam.hip beam_cross_kernel).  Same results to fp32 summation order. */
int d2t_set_beam_shared_tile(d2t_ctx* ctx, int32_t on);
int d2t_set_reserved_cus(d2t_ctx* ctx, int32_t cus);
/* Number of decode chains (1 .. 4, default 1) d2t_decode_greedy_async alternates between.  Each chain has
 * its own stream, self-attention cache and workspace, so with 2 the step loops of two consecutive batches
 * run side by side (the loop is a dependent chain of small kernels that cannot fill the chip alone). */
int d2t_set_decode_chains(d2t_ctx* ctx, int32_t chains);

/* ---- training step (engine/training.py:76-164) ----------
 * d2t_train_forward runs Model.forward under module.train() for the HybridViT + TFM stack: BatchNorm on batch
 * statistics (the engine's copies of running_mean / running_var are updated with momentum 0.1; read them back
 * with d2t_read_weight), teacher-forced decoder pass over tgt [B][L] (= text[:, :-1]; PAD = 0 keys masked,
 * causal), dropout 0.  logits [B][L][vocab] is caller memory.  Weights are the ones last given to
 * d2t_load_weight (no finalize needed).  d2t_train_backward takes dL/dlogits [B][L][vocab] and leaves the
 * gradient of every trainable parameter in engine memory; d2t_train_grad copies one out by its state_dict key.
 * d2t_train_grad may be given ANY stream: the copy is ordered (by an event) after the last backward kernel that
 * writes that gradient, so a communication stream can pick up early gradients (decoder, ViT, deep backbone layers)
 * and all-reduce them while the rest of the backward still runs on the compute stream.
 * One forward may be followed by at most one backward.  All pointers are device pointers. */
int d2t_train_forward(d2t_ctx* ctx, const float* image, int32_t B, int32_t H, int32_t W, const int64_t* tgt, int32_t L,
                      float* logits, d2t_stream stream);
int d2t_train_backward(d2t_ctx* ctx, const float* dlogits, d2t_stream stream);
int d2t_train_grad(d2t_ctx* ctx, const char* name, float* dst, int64_t numel, d2t_stream stream);
/* All of them at once (the single-process step: what loss.backward() leaves in .grad): gradient `names[i]` is written to
 * flat[offsets[i] .. offsets[i] + numels[i]) by ONE kernel ordered after the whole backward, instead of one device copy per
 * parameter (378 of them for the headline model: ~3 ms of 4-us copies).  source = 0: gradients; 1: the engine's current
 * copy of loaded tensors (the BatchNorm running statistics after a training forward, as d2t_read_weight). */
int d2t_train_gather(d2t_ctx* ctx, int32_t source, int32_t n, const char* const* names, const int64_t* offsets,
                     const int64_t* numels, float* flat, d2t_stream stream);
/* The other direction, after optimizer.step(): refresh the engine's copies of tensors that are ALREADY loaded (same names and
 * sizes as the d2t_load_weight calls that created them) from device memory, in one kernel.  Folded / packed inference
 * weights are not rebuilt: call d2t_finalize_weights before the next inference forward (the training step reads the raw copies). */
int d2t_reload_weights(d2t_ctx* ctx, int32_t n, const char* const* names, const float* const* srcs, const int64_t* numels,
                       d2t_stream stream);
/* copy the engine's current copy of a loaded tensor (e.g. BatchNorm running statistics after a training forward) */
int d2t_read_weight(d2t_ctx* ctx, const char* name, float* dst, int64_t numel, d2t_stream stream);
/* Dropout of nn.TransformerDecoderLayer(dropout=p) in the training step: on the attention probabilities of both
 * attentions, after each of the three sub-layers (dropout1/2/3) and inside the feed-forward block.  Keep masks are
 * Philox4x32-10 draws keyed by (seed, number of training forwards since the seed was set, site index): statistically
 * the same as torch's dropout, not the same random stream.  p = 0 (default) disables it.  The masks of the last
 * forward can be read back (creation order = the order torch draws them) for verification. */
int d2t_train_set_dropout(d2t_ctx* ctx, float p, uint64_t seed);
/* LSTM-attention head only.  (a) d2t_train_set_dropout's p is the head's `droprate`: dropout on the generator output
 * of every step (seq2seq.py:298), one [B][S][V] mask.  (b) Scheduled sampling (seq2seq.py:311-316): flags[t] (host
 * bytes, n = batch_max_length + 1 of them; flags[0] is ignored) says whether step t is fed the label token (1) or the
 * arg-max of step t-1's output (0).  n = 0 restores "always the label".  The flags apply to the following forwards. */
int d2t_train_set_teacher_flags(d2t_ctx* ctx, const uint8_t* flags, int32_t n);
int d2t_train_mask_count(d2t_ctx* ctx);
/* The discrete decisions of the last d2t_train_forward, in network order: one entry per ReLU (keep mask, y > 0, one byte per
 * element of the [rows][cols] output) and per max-pool (the window element kh*2+kw that holds the first maximum, one byte
 * per NHWC output element).  Test instrument: replayed in the CPU oracle they pin both sides to the same smooth function.
 * dst may be NULL to query *is_pool_out / *numel_out only. */
int d2t_train_decision_count(d2t_ctx* ctx);
int d2t_train_read_decision(d2t_ctx* ctx, int32_t index, uint8_t* dst, int64_t numel, int32_t* is_pool_out,
                            int64_t* numel_out, d2t_stream stream);
int d2t_train_read_mask(d2t_ctx* ctx, int32_t index, uint8_t* dst, int64_t numel, d2t_stream stream);
/* The alignments of the last d2t_train_forward of an LSTM-attention head, [B][S][Tk] (S = batch_max_length + 1), copied
 * into dst (device).  D2T_ESTATE for the TFM head and before any forward (or after its backward consumed it). */
int d2t_train_read_attn_alpha(d2t_ctx* ctx, float* dst, int64_t numel, d2t_stream stream);
/* free the training tape, gradient buffers and workspace */
void d2t_train_release(d2t_ctx* ctx);

/* ---- in-engine kernel timing (bench.py roofline leg) ------------------------
 * While enabled, d2t_encode brackets every implicit-GEMM (MFMA) launch with a
 * pair of HIP events on the launch stream.  d2t_profile_read synchronises,
 * returns up to max_records launches in issue order as GEMM shape (M,N,K) and
 * elapsed milliseconds, and clears the log.  *n receives the number written. */
int d2t_profile_enable(d2t_ctx* ctx, int32_t on);
int d2t_profile_read(d2t_ctx* ctx, int32_t max_records, int32_t* n, int32_t* M, int32_t* N, int32_t* K, float* ms);

/* ---- single-kernel entry points (parity tests) ----------------------------
 * All tensors [device] fp32.  Activations are NHWC / row-major [rows, features].
 */
/* y = act(conv2d(x, w) + bias + residual).  x [B,H,W,Cin] NHWC, w [Cout,KH,KW,Cin]
 * (OHWI), bias [Cout] or NULL, residual [B,OH,OW,Cout] or NULL, y [B,OH,OW,Cout].
 * Out-of-range taps read as zero.  Cin must be 1 or 3 (direct stem kernels, 3x3 pad 1 only;
 * x is then the image as d2t_encode takes it, NCHW planar [B,Cin,H,W], w still OHWI)
 * or a multiple of 32 (MFMA implicit GEMM). */
int d2t_op_conv2d(const float* x, const float* w, const float* bias, const float* residual, float* y, int32_t B,
                  int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KH, int32_t KW, int32_t SH, int32_t SW,
                  int32_t PH, int32_t PW, int32_t act, d2t_stream stream);
/* Same contract on the bf16x3 kernel (Cin % 32 == 0); splits w internally (test entry point, synchronous). */
int d2t_op_conv2d_bf16x3(const float* x, const float* w, const float* bias, const float* residual, float* y, int32_t B,
                         int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KH, int32_t KW, int32_t SH,
                         int32_t SW, int32_t PH, int32_t PW, int32_t act, d2t_stream stream);
/* Same again on the split-activation kernel: x, residual and y cross the kernel boundary as bf16 hi/lo
 * planes (split / merged around the launch by this test entry point). */
/* which split-bf16 kernel d2t_op_conv2d_bf16x3_split launches (d2t_set_conv_kernel / d2t_set_reserved_cus of a context,
 * but process-wide: tests and tools only) */
int d2t_op_set_conv_kernel(int32_t kind, int32_t reserved_cus);
/* the same with the 2x2 / stride 2 max-pool that follows fused into the epilogue (ConvP::pool2; no residual): y is the pooled
 * map [B][OH/2][OW/2][Cout].  Layers with <= 64 or >= 128 output channels (the two kernels that carry the fused form). */
int d2t_op_conv2d_bf16x3_split_pool(const float* x, const float* w, const float* bias, float* y, int32_t B, int32_t H, int32_t W,
                                    int32_t Cin, int32_t Cout, int32_t KH, int32_t KW, int32_t SH, int32_t SW, int32_t PH,
                                    int32_t PW, int32_t act, d2t_stream stream);
int d2t_op_conv2d_bf16x3_split(const float* x, const float* w, const float* bias, const float* residual, float* y,
                               int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KH, int32_t KW,
                               int32_t SH, int32_t SW, int32_t PH, int32_t PW, int32_t act, d2t_stream stream);
/* y[M,N] = act(x[M,K] @ w[N,K]^T + bias + residual); any M (skinny path for M<=64). */
int d2t_op_linear(const float* x, const float* w, const float* bias, const float* residual, float* y, int32_t M,
                  int32_t K, int32_t N, int32_t act, d2t_stream stream);
/* 2x2 max-pool, NHWC, stride (SH,SW), padding (PH,PW) with -inf semantics. */
int d2t_op_maxpool2x2(const float* x, float* y, int32_t B, int32_t H, int32_t W, int32_t C, int32_t SH, int32_t SW,
                      int32_t PH, int32_t PW, d2t_stream stream);
/* y = LayerNorm(x) * gamma + beta over the last dim (D = 256 or 512). */
int d2t_op_layernorm(const float* x, const float* gamma, const float* beta, float* y, int32_t rows, int32_t D,
                     float eps, d2t_stream stream);
/* ViT self-attention.  qkv [B,N,3,heads,32] -> y [B,N,heads*32]; softmax(q k^T / sqrt(32)) v. */
int d2t_op_vit_attention(const float* qkv, float* y, int32_t B, int32_t N, int32_t heads, d2t_stream stream);
/* ... plus the softmax probabilities, probs [B,heads,N,N] fp32 (key innermost); y is bitwise d2t_op_vit_attention's. */
int d2t_op_vit_attention_probs(const float* qkv, float* y, float* probs, int32_t B, int32_t N, int32_t heads,
                               d2t_stream stream);
/* Single-query attention (decoder step).  q [B,heads*hd]; k,v [B,heads,Lmax,hd];
 * attends over the first L keys; y [B,heads*hd].  hd = 32 or 64. */
int d2t_op_decode_attention(const float* q, const float* k, const float* v, float* y, int32_t B, int32_t heads,
                            int32_t hd, int32_t L, int32_t Lmax, d2t_stream stream);

/* ---- the decode step's kernels, one at a time ------------------------------------------------------------------
 * TEST INFRASTRUCTURE (tests/test_decode_ops_gpu.py): the serving paths never call these.  No context; tensors are
 * device pointers in the layouts PyTorch has (weights [N][K] as stored); whatever transposition / splitting a kernel
 * wants happens in temporary device memory.  Every size -- and every device-side integer a kernel indexes with (step
 * counters, row maps, ancestry, segments, parents), read back before the launch -- is checked against the kernel's limits:
 * D2T_EINVAL and nothing launched otherwise.  The entries synchronise the stream for that check. */
/* Skinny GEMM (launch_skinny): y[M][ldy] (first N columns) = act(A @ w[N][K]^T + bias + res[M][N]), A = x[M][ldx] or, with
 * ln_g / ln_b, LayerNorm(x) * ln_g + ln_b (K = 256, 512, 1024); ln_out (optional, needs N >= K) receives A [M][K].
 * step (optional, device): the output base is advanced by *step * out_step_stride floats. */
int d2t_op_skinny(const float* x, const float* w, const float* bias, const float* res, const float* ln_g, const float* ln_b,
                  float ln_eps, float* y, float* ln_out, int32_t M, int32_t K, int32_t N, int32_t ldx, int32_t ldy, int32_t act,
                  const int32_t* step, int64_t out_step_stride, d2t_stream stream);
/* The same with the kernel form named instead of chosen from M: form 0 the split-K kernel (block tile 16 / 32 rows x 16
 * columns), form 1 the wide kernel of the decode groups (K = 256, 512, 1024 only).  The two give bitwise equal results. */
int d2t_op_skinny_form(const float* x, const float* w, const float* bias, const float* res, const float* ln_g,
                       const float* ln_b, float ln_eps, float* y, float* ln_out, int32_t M, int32_t K, int32_t N, int32_t ldx,
                       int32_t ldy, int32_t act, const int32_t* step, int64_t out_step_stride, int32_t form,
                       d2t_stream stream);
/* The fused row step of one post-norm decoder layer for M rows at position t = *step (8 heads):
 *   a = SelfAttn(q, cache[0 .. t-1] + this step's k, v);  x1 = LN1(a @ sa_out_w^T + sa_out_b + xres)
 *   y2 = CrossAttn(x1, mem of the row's sample) @ ca_out_w^T + ca_out_b + x1          (pre-LN2)
 * kind: 0 projected K/V (D = 256 or 512; one_row != 0 selects the one-row-per-block build at D = 512), 1 absorbed two rows
 * per block, 2 absorbed one row, 3 / 4 the same two on split-bf16 MFMAs, 5 beam search's pre / per-sample cross / post
 * split (D = 256 for 1-5).  qkv [M][3D] (self-attention in-projection of this step), xres [M][D]; sk / sv
 * [rows][8][Lmax][D/8], read and written (row b's k, v are stored at position t); mem [samples][T][D]; ca_in_w [3D][D] /
 * ca_in_b [3D] the cross-attention in-projection; row_map (optional) [M]: the sample of a row (default: row b -> sample b);
 * anc (kinds 2, 4, Lmax <= 512) [M][anc_stride]: the cache row that holds position j < t of row b; seg (kind 5)
 * [nsamples][3] = (first row, rows <= 6, -) of sample n, compact and in row order, row_map agreeing with it. */
int d2t_op_decoder_row(int32_t kind, const float* qkv, const float* xres, float* sk, float* sv, const float* mem,
                       const float* ca_in_w, const float* ca_in_b, const float* sa_out_w, const float* sa_out_b,
                       const float* ca_out_w, const float* ca_out_b, const float* ln1_g, const float* ln1_b, float eps, float* y2,
                       const int32_t* step, int32_t M, int32_t D, int32_t T, int32_t Lmax, int32_t rows, int32_t samples,
                       int32_t one_row, const int32_t* row_map, const int32_t* anc, int32_t anc_stride, const int32_t* seg,
                       int32_t nsamples, d2t_stream stream);
/* The ragged builds of the greedy absorbed row kernels (D = 256; kind 1 - 4 as above): mem is ONE packed [mem_rows][256]
 * buffer and row b attends over the len[b] rows from row row0[b] on (HOST arrays [M]; 1 <= len[b] <= 4096,
 * row0[b] + len[b] <= mem_rows).  Everything else as d2t_op_decoder_row.  With row0[b] = b * T and len[b] = T the result
 * equals d2t_op_decoder_row's bit for bit. */
int d2t_op_decoder_row_ragged(int32_t kind, const float* qkv, const float* xres, float* sk, float* sv, const float* mem,
                              const float* ca_in_w, const float* ca_in_b, const float* sa_out_w, const float* sa_out_b,
                              const float* ca_out_w, const float* ca_out_b, const float* ln1_g, const float* ln1_b, float eps,
                              float* y2, const int32_t* step, int32_t M, int32_t Lmax, int32_t rows, int32_t mem_rows,
                              const int32_t* row0, const int32_t* len, d2t_stream stream);
/* The per-sample ragged builds of the one-row absorbed kernel (ragged beam search; kind 2 = fp32 MFMA, 4 = split-bf16):
 * mem is ONE packed [mem_rows][256] buffer, row b attends over the len[row_map[b]] rows from row row0[row_map[b]] on.
 * row0 / len: HOST arrays [samples] (1 <= len[i] <= 4096, row0[i] + len[i] <= mem_rows); row_map (required, device [M],
 * values < samples); anc (optional, Lmax <= 512) as d2t_op_decoder_row.  A sample's rows equal d2t_op_decoder_row's on
 * that sample's memory alone bit for bit. */
int d2t_op_decoder_row_ragged_beam(int32_t kind, const float* qkv, const float* xres, float* sk, float* sv, const float* mem,
                                   const float* ca_in_w, const float* ca_in_b, const float* sa_out_w, const float* sa_out_b,
                                   const float* ca_out_w, const float* ca_out_b, const float* ln1_g, const float* ln1_b, float eps,
                                   float* y2, const int32_t* step, int32_t M, int32_t Lmax, int32_t rows, int32_t mem_rows,
                                   int32_t samples, const int32_t* row0, const int32_t* len, const int32_t* row_map,
                                   const int32_t* anc, int32_t anc_stride, d2t_stream stream);
/* The map kernel of d2t_decode_cross_attention alone (8 heads, D = 256 or 512, 1 <= T <= 4096, M <= 65535):
 * P[b][h][j] = softmax_j(q[b][h] . keys[b][h][j] / sqrt(D / 8)).  q [M][D] (the cross-attention queries, bias included, not
 * scaled); keys [M][8][T][D / 8] (row b's projected keys).  per_head != 0: out [M][8][T] = P; 0: out [M][T], the mean over
 * the heads summed in head order.  Writes exactly those floats. */
int d2t_op_cross_attn_probs(const float* q, const float* keys, int32_t M, int32_t D, int32_t T, int32_t per_head, float* out,
                            d2t_stream stream);
/* One greedy step (launch_argmax_embed) at t = *step < S: tokens[b][t] = first maximum of logits[b][t][:V] (logits [B][S][V],
 * tokens [B][S]); end-of-sequence bookkeeping in ended [B], end_count, steps_done; *step becomes t + 1, done_count (zero
 * before the first launch) is back at zero afterwards; x [B][d] (optional) = emb[token] * sqrt(d) + pe[t + 1] (pe [S + 1][d]).
 * n_batches > 0: rows are n_batches groups of rows_per_batch with batch_end_count / batch_steps_done [n_batches],
 * batches_done [1] and stop_at [1] (optional; once *stop_at != 0 and t >= *stop_at a launch changes nothing). */
int d2t_op_argmax_embed(const float* logits, int32_t S, int64_t* tokens, int32_t* ended, int32_t* end_count, int32_t* steps_done,
                        int32_t* step, int32_t* done_count, int32_t* batch_end_count, int32_t* batch_steps_done,
                        int32_t* batches_done, int32_t* stop_at, const float* emb, const float* pe, float* x, int32_t B, int32_t V,
                        int32_t d, int32_t end_token, int32_t rows_per_batch, int32_t n_batches, d2t_stream stream);
/* Beam candidates (launch_beam_topk_batch): segment n = seg[n] = (first row, rows <= 16, k <= kmax <= 16) of logits [rows][V] /
 * scores [rows]; its k best of score[i] + log_softmax(logits[i])[v] (value descending, flat index i * V + v ascending on ties)
 * at topv / topi [n][kmax].  A segment with no rows or k = 0 leaves its slots untouched. */
int d2t_op_beam_topk(const float* logits, const float* scores, const int32_t* seg, int32_t N, int32_t rows, int32_t V, int32_t kmax,
                     float* topv, int32_t* topi, d2t_stream stream);
/* Device-side Beam.advance for N <= 1024 samples, beam <= 16 (struct BeamDev of csrc/kernels.h: ctrl [4], tok / scores / map /
 * prev [cap], seg [N][3], comp_n / fin [N], comp_t / comp_par / comp_score [N][beam], hist_par / hist_tok [S][cap]).  init != 0:
 * launch_beam_dev_init (topv / topi unused); else one launch_beam_dev_advance over the candidates topv / topi [N][beam]. */
int d2t_op_beam_advance(int32_t init, int64_t go_token, int32_t* ctrl, int64_t* tok, float* scores, int32_t* map, int32_t* prev,
                        int32_t* seg, int32_t* comp_n, int32_t* fin, int32_t* comp_t, int32_t* comp_par, float* comp_score,
                        int32_t* hist_par, int32_t* hist_tok, const float* topv, const int32_t* topi, int32_t N, int32_t beam,
                        int32_t cap, int32_t V, int32_t S, int32_t end_token, d2t_stream stream);
/* anc_new[row][0 .. t-2] = anc_old[prev[row]][...], anc_new[row][t-1] = prev[row], t = *step_in <= stride, published to
 * *step_out; rows >= *rows_ptr are skipped and nothing is written once *stop != 0 and t >= *stop (both optional). */
int d2t_op_beam_ancestry(const int32_t* anc_old, int32_t* anc_new, const int32_t* prev, int32_t rows, int32_t stride,
                         const int32_t* step_in, int32_t* step_out, const int32_t* rows_ptr, const int32_t* stop,
                         d2t_stream stream);
/* dst[slab][i][head][0 .. rows)[:] = src[slab][prev[i]][head][0 .. rows)[:] for i < M; caches [slabs][cap][heads][Lmax][hd]. */
int d2t_op_cache_gather(const float* src, float* dst, const int32_t* prev, int32_t slabs, int32_t cap, int32_t M, int32_t heads,
                        int32_t Lmax, int32_t hd, int32_t rows, d2t_stream stream);

/* ---- the encoder's record path, one kernel at a time ---------------------------------------------------------------
 * TEST INFRASTRUCTURE (tests/test_conv_records_gpu.py): the serving paths never call these.  No context, device pointers,
 * synchronous; every size is checked before anything is launched (D2T_EINVAL), and what a kernel's own launcher refuses
 * comes back as D2T_EINVAL with nothing launched on the caller's buffers.
 * RECORDS: an activation [rows][C], C % 32 == 0, as raw uint16 planes -- per row and 32-channel group one 128-byte record
 * [32 x hi | 32 x lo].  Formats: 0 = bf16 hi | lo, 1 = ONE fp16 in the hi half, 2 = fp16 hi | fp16 lo. */
/* fp32 [rows][C] -> records (a source that is not 16-byte aligned takes the scalar kernel), and back */
int d2t_op_records_split(const float* x, uint16_t* planes, int64_t rows, int32_t C, int32_t fmt, d2t_stream stream);
int d2t_op_records_merge(const uint16_t* planes, float* x, int64_t rows, int32_t C, int32_t fmt, d2t_stream stream);
/* One launch_conv with every field of the record path settable.
 * Input: x_rec, records [B*H*W][Cin] of format in_fmt (1 and 2 select the two-MFMA arithmetic on fp16 hi / lo weights, whose
 * MFMAs read the hi half alone) -- or x_f32, fp32 rows, with in_fmt 3 (split-bf16 kernel, split on the fly; Cout >= 64)
 * or 4 (fp32 kernel).  w [Cout][KH][KW][Cin] (OHWI), bias [Cout] or NULL.
 * Second input (records only): x2_rec [M][Cin2] in the format of x_rec, w2 [Cout][Cin2], bias2 [Cout]; bias is then
 * required, and the launch adds bias + bias2.
 * Residual: res_rec (records, res_fmt 0/1/2) or res_f32, rows indexed like the output's; never both.
 * Output: out_rec (records, out_fmt 0/1/2) or out_f32, a buffer of out_rows rows that the CALLER allocates and prefills:
 * the entry never clears it.  Without a remap the launch writes rows [0, M) (pool2: the M / 4 pooled rows).
 * OH / OW < 0: what the convolution formula gives; otherwise the patch embedding's override.  M = B * OH * OW, with
 * pool2 4 * B * (OH/2) * (OW/2) rows in pooled order.
 * Remap (rows_per_img > 0): GEMM row m goes to output row (m / rows_per_img) * img_stride + row_off + m % rows_per_img.
 * row_add [row_add_rows][Cout] (optional): row row_add_off + m % rows_per_img (row_add_off without a remap) is added
 * behind the activation.
 * kind: 0 / 3 as d2t_set_conv_kernel; split_tail: ConvP::split_tail.
 * max_blocks > 0: at most that many (persistent) blocks of the 128-row record kernels; reserved_cus > 0: the pipelined kernel
 * runs one block on each of (CUs - reserved_cus) CUs, at least 8 (ConvP::max_blocks / reserved_cus).  Negative: refused. */
typedef struct d2t_op_conv_records_args {
  const uint16_t* x_rec; const float* x_f32; const uint16_t* x2_rec;
  const float* w; const float* w2; const float* bias; const float* bias2;
  const uint16_t* res_rec; const float* res_f32; const float* row_add;
  uint16_t* out_rec; float* out_f32;
  int32_t in_fmt, res_fmt, out_fmt;
  int32_t B, H, W, Cin, Cin2, Cout, KH, KW, SH, SW, PH, PW, OH, OW, act, pool2;
  int32_t rows_per_img, img_stride, row_off, row_add_off, row_add_rows, out_rows;
  int32_t kind, split_tail;
  int32_t max_blocks, reserved_cus;
} d2t_op_conv_records_args;
int d2t_op_conv_records(const d2t_op_conv_records_args* a, d2t_stream stream);
/* The head-split K / V store of cross_kv (STORE_KV): y [slabs][kv_B][heads][kv_T][hd] from x [M = kv_B * kv_T][K] @ w [N][K]^T
 * + bias, N = slabs * heads * hd, K % 32 == 0; bf16x3 != 0: the split-bf16 kernel (N >= 64), else the fp32 kernel. */
int d2t_op_linear_kv(const float* x, const float* w, const float* bias, float* y, int32_t K, int32_t N, int32_t kv_B, int32_t kv_T,
                     int32_t heads, int32_t hd, int32_t bf16x3, d2t_stream stream);
/* 2x2 max-pool over records of format fmt, [B][H][W][C] -> [B][OH][OW][C], stride >= 1, padding 0 or 1 */
int d2t_op_maxpool_records(const uint16_t* x, uint16_t* y, int32_t B, int32_t H, int32_t W, int32_t C, int32_t SH, int32_t SW,
                           int32_t PH, int32_t PW, int32_t fmt, d2t_stream stream);
/* The stem (3x3, padding 1) writing records [B*H*W][32] of format 0 or 1: img NCHW planar [B][Cin][H][W], Cin 1 or 3,
 * w [32][3][3][Cin], bias [32] or NULL */
int d2t_op_stem_records(const float* img, const float* w, const float* bias, uint16_t* out, int32_t B, int32_t Cin, int32_t H,
                        int32_t W, int32_t act, int32_t fmt, d2t_stream stream);
/* Weight packing as d2t_finalize_weights does it: w_oihw [Cout][Cin][KH][KW] with the optional convolution bias [Cout] and the
 * optional eval-BatchNorm (all four of bn_w, bn_b, bn_mean, bn_var, or none) folded in -> w_out in the kernels' K order
 * (Cin % 32 == 0; plain OHWI otherwise), bias_out [Cout], and the bf16 (RNE hi) and fp16 hi / lo planes of w_out. */
int d2t_op_pack_conv(const float* w_oihw, const float* conv_bias, const float* bn_w, const float* bn_b, const float* bn_mean,
                     const float* bn_var, float eps, float* w_out, float* bias_out, uint16_t* bf16_hi, uint16_t* bf16_lo,
                     uint16_t* f16_hi, uint16_t* f16_lo, int32_t Cout, int32_t Cin, int32_t KH, int32_t KW, d2t_stream stream);

/* ---- the recurrent kernels, one at a time ------------------------------------------------------------------------
 * TEST INFRASTRUCTURE (tests/test_recurrent_ops_gpu.py): the BiLSTM recurrence, the LSTM-attention decoder loop and their
 * small helpers (csrc/recurrent.hip), behind the same rules as the decode-step entries above -- no context, device
 * pointers, every size and every device-side integer table checked before anything is launched (D2T_EINVAL otherwise).
 * Unlike those entries the tensors are in the KERNELS' OWN layouts (transposed weights, the folded location filter, gates
 * [B*T][8H]): what the engine hands its launchers.  H = D = E = 256.  The backward kernels' entries are further down, next
 * to the d2t_op_train_* entries. */
/* One bidirectional LSTM layer from its input projection: g [B*T][2*4H] (forward | reverse gates i, f, g, o, biases
 * included), whh_t [2][H][4H] (W_hh^T per direction); out [B][T][2H] = [h_fwd | h_rev].  sv_gates [B*T][2*4H] and sv_c
 * [B*T][2H] (both or neither): the training forward, which keeps the gates AFTER their nonlinearities and the cell state. */
int d2t_op_bilstm(const float* g, const float* whh_t, float* out, float* sv_gates, float* sv_c, int32_t B, int32_t T,
                  int32_t H, d2t_stream stream);
/* The h_prev operands of the W_hh gradient GEMMs: hprev_fwd[b][t] = out[b][t-1][:H], hprev_rev[b][t] = out[b][t+1][H:]
 * (zeros at the ends); out [B][T][2H], both results [B*T][H]. */
int d2t_op_bilstm_hprev(const float* out, float* hprev_fwd, float* hprev_rev, int32_t B, int32_t T, int32_t H,
                        d2t_stream stream);
/* The LSTM-attention decoder loop (launch_attn_decode; struct AttnDecP of csrc/kernels.h, whose field names these are).
 * Required: mem [samples][T][256], kp [samples][T][256], wq_t [256][256], bq, wloc [256][taps], bloc, wscore, wx_t [768][1024],
 * bx [1024], wg_t [256][V], bg [V], probs [B][S][V], tokens [B][S], end_step [B] (set to -1 by the entry first, as the engine
 * does); exactly one of emb [V][256] / tokgate [V][1024]; wih_t / bih / wic_t / bic when init_mode != 0.
 * samples = B outside step mode.  Step mode (S = 1): st_*_out required, st_*_in and tok_in [B] unless first; row_sample
 * (optional) [B] < samples.  teacher [B][S] < V (not in step mode) with use_teacher [S], sv_tok; out_dropmask [B][S][V];
 * the sv_* buffers are optional (hprev + cprev together; gates + hafter + cafter together).
 * exit_state (needs steps_dev; neither step mode nor teacher): the early-exit build -- the word is zeroed, the loop runs, and
 * the finalize kernel follows on the stream, as the engine's greedy is_test path. */
typedef struct d2t_op_attn_decode_args {
  const float *mem, *kp, *wq_t, *bq, *wloc, *bloc, *wscore, *wx_t, *bx, *wg_t, *bg, *wih_t, *bih, *wic_t, *bic, *emb, *tokgate;
  float* probs;
  int64_t* tokens;
  int32_t* end_step;
  const float *st_h_in, *st_c_in, *st_mem_in;
  float *st_h_out, *st_c_out, *st_mem_out;
  const int64_t* tok_in;
  const int32_t* row_sample;
  const int64_t* teacher;
  const uint8_t *use_teacher, *out_dropmask;
  int64_t* sv_tok;
  float *sv_hprev, *sv_cprev, *sv_hafter, *sv_cafter, *sv_gates, *sv_alpha, *sv_hq, *sv_x;
  uint64_t* exit_state;
  int32_t* steps_dev;
  float bscore, out_dropscale;
  int32_t B, T, S, V, taps, key_off, init_mode, coverage, end_token, step_mode, first, samples;
} d2t_op_attn_decode_args;
int d2t_op_attn_decode(const d2t_op_attn_decode_args* a, d2t_stream stream);
/* The ragged build of the step (step mode only; AttnDecP::smp_row0 / smp_T / st_ld): mem and kp are ONE packed
 * [sum of lengths][256] buffer each, and row b's sample i = row_sample[b] (0 without a map) owns the smp_T[i] rows from row
 * smp_row0[i] on.  smp_row0 / smp_T: DEVICE arrays [samples], read back and checked before the launch: 1 <= smp_T[i] -
 * key_off <= st_ld, smp_row0[i] >= 0, smp_row0[i] + smp_T[i] <= the sum of the lengths; a->T is the largest length.
 * st_mem_in / st_mem_out [B][st_ld] and sv_alpha [B][1][st_ld], 1 <= st_ld <= 4096: row b's first Tk_i elements are read /
 * written, sv_alpha is zero on [Tk_i, st_ld), st_mem_out untouched there.  Everything else as d2t_op_attn_decode; a row's
 * outputs equal d2t_op_attn_decode's on its sample's memory alone bit for bit. */
int d2t_op_attn_decode_ragged(const d2t_op_attn_decode_args* a, const int32_t* smp_row0, const int32_t* smp_T, int32_t st_ld,
                              d2t_stream stream);
/* The group build of the loop (loop mode only: neither step mode nor teacher; AttnDecP::grp_*): the a->B <= 1024 rows are the
 * rows of n_batches <= 64 batches in batch order, mem and kp ONE packed buffer each, and row b owns the len[b] rows from row
 * row0[b] on.  row0 / len / row_batch: DEVICE arrays [B], batch_rows: DEVICE array [n_batches], read back and checked before
 * the launch: 1 <= len[b] - key_off <= 4096, a->T the largest length, row0[b] >= 0, row0[b] + len[b] <= the sum of the rows'
 * lengths, row_batch non-decreasing from 0 to n_batches - 1 in steps of one, batch_rows[k] the rows of batch k.  a->exit_state
 * (optional) is ONE WORD PER BATCH [n_batches], zeroed by the entry; a->steps_dev must be NULL and no sv_* / mask / teacher
 * field set.  The per-batch finalize kernel follows: steps_dev[k] (device [n_batches], required) = batch k's step count, and
 * tokens / probs of its rows are zeroed behind it; without exit words every entry is S and nothing is zeroed.  A row's
 * tokens, probs and end_step equal d2t_op_attn_decode's on its batch alone bit for bit. */
int d2t_op_attn_decode_group(const d2t_op_attn_decode_args* a, const int32_t* row0, const int32_t* len, const int32_t* row_batch,
                             const int32_t* batch_rows, int32_t n_batches, int32_t* steps_dev, d2t_stream stream);
/* The finalize kernel alone on a caller-given exit word {rows ended : high 32 bits, largest end step : low 32 bits}:
 * *steps_dev = largest end step + 1 if all B rows ended and that is below S, else S; tokens [B][S], probs [B][S][V] and
 * alpha [B][S][Tk] (optional) zeroed for the steps [steps, S) of every row. */
int d2t_op_attn_decode_finalize(const uint64_t* exit_state, int32_t* steps_dev, int32_t B, int32_t S, int32_t V, int32_t Tk,
                                int64_t* tokens, float* probs, float* alpha, d2t_stream stream);
/* out [N][S][Tk] = hist[j][path[i*S + j]][:] for j < len[i], zeros for len[i] <= j < S; hist [S][cap][Tk], path [N][S]
 * (values < cap where j < len[i]), len [N] in [0, S].  out must be 16-byte aligned. */
int d2t_op_attn_alpha_gather(const float* hist, const int32_t* path, const int32_t* len, float* out, int32_t N, int32_t S,
                             int32_t cap, int32_t Tk, d2t_stream stream);
/* The record of the LSTM-attention beam search (csrc/attn_beam_host.h AttnBeamDev), every array a device buffer of the
 * caller: ctrl [4] = {step, live rows, stop-at step, steps run}; tok (int64), scores, map, idx_h, idx_m [cap]; seg [N][3] =
 * {first row, rows ranked, candidates wanted}; comp_n, fin, last_completed [N]; comp_t, comp_par, comp_score [N][beam];
 * hist_par, hist_tok [S][cap]; topv, topi [N][beam] the step's candidates (d2t_op_beam_topk).  cap >= N * beam, N <= 1024,
 * beam <= 16.
 * d2t_op_attn_beam_advance: init != 0 lays out step 0 (beam rows per sample from go_token, seg = {i * beam, 1, beam});
 * init == 0 is ONE step of the bookkeeping on the record (a stopped record is left alone).  D2T_EINVAL for a record whose
 * step, segments or candidates would index outside it.
 * d2t_op_attn_beam_finish: the final pick of every sample: seq [N][S] (zeros beyond the length), len [N], score [N], and with
 * path / plen (both or neither) the chosen launch rows path [N][S] and their count plen [N]. */
typedef struct d2t_op_attn_beam_rec {
  int32_t* ctrl; int64_t* tok; float* scores;
  int32_t *map, *idx_h, *idx_m, *seg, *comp_n, *fin, *last_completed, *comp_t, *comp_par;
  float* comp_score;
  int32_t *hist_par, *hist_tok;
  const float* topv; const int32_t* topi;
  int32_t N, beam, cap, V, S, end_token;
} d2t_op_attn_beam_rec;
int d2t_op_attn_beam_advance(const d2t_op_attn_beam_rec* r, int32_t init, int64_t go_token, d2t_stream stream);
int d2t_op_attn_beam_finish(const d2t_op_attn_beam_rec* r, int64_t* seq, int32_t* len, float* score, int32_t* path, int32_t* plen,
                            d2t_stream stream);
/* The same two operators as the HOST loop of the search runs them (csrc/attn_beam_host.h): every array of the record and
 * every output is a host array, nothing touches a device or a context, and N has no upper limit.  They write what the device
 * operators write, array for array, and refuse the same records with D2T_EINVAL, writing nothing. */
int d2t_op_attn_beam_host_advance(const d2t_op_attn_beam_rec* r, int32_t init, int64_t go_token);
int d2t_op_attn_beam_host_finish(const d2t_op_attn_beam_rec* r, int64_t* seq, int32_t* len, float* score, int32_t* path,
                                 int32_t* plen);

/* ---- fused cross-entropy ------------------------------------------------------------------------------------------
 * The criterion of the reference's training step -- nn.CrossEntropyLoss(ignore_index = PAD, reduction = 'none') on
 * preds.view(-1, V) / target.view(-1) (engine/training.py:50-53, 83, 90; modules/loss/builder.py:18-24) -- as one kernel
 * each way instead of torch's log_softmax + nll_loss pair.  logits [rows][V] fp32, target [rows] int64; loss [rows] and
 * lse [rows] (log-sum-exp, kept for the backward) are written; rows whose target equals ignore_index give loss 0 and a
 * zero gradient.  dloss [rows] is the incoming gradient of the per-row losses (1 / rows for the reference's .mean()). */
int d2t_ce_forward(const float* logits, const int64_t* target, float* loss, float* lse, int32_t rows, int32_t V,
                   int64_t ignore_index, d2t_stream stream);
int d2t_ce_backward(const float* logits, const int64_t* target, const float* lse, const float* dloss, float* dlogits,
                    int32_t rows, int32_t V, int64_t ignore_index, d2t_stream stream);
/* The other criteria modules/loss/builder.py can build, as a second kernel pair (the plain pair above is untouched).  A
 * live row with target t puts the mass  m[v] = on * w[t] * [v == t] + off * w[v] * [v in S]  on class v:
 *     loss = sum_v m[v] * (lse - x[v]),      dlogits[v] = dloss * (M * exp(x[v] - lse) - m[v]),      M = sum_v m[v].
 *   D2T_CE_TORCH      nn.CrossEntropyLoss(weight, ignore_index, label_smoothing = e): on = 1 - e, off = e / V, S = every
 *                     class, w = weight [V] (NULL: all ones); pad_index is not read.
 *   D2T_CE_REFERENCE  LabelSmoothingLoss(reduction, classes, ignore_index, smoothing = s) (modules/loss/labelsmoothing.py):
 *                     on = 1 - s, off = s / (classes - 2), S = every class except t and column pad_index, weight NULL;
 *                     the row mass M is then not 1.
 * The forward writes loss [rows], lse [rows] and mass [rows] (M; lse and mass feed the backward, which repeats no
 * reduction).  Rows whose target equals ignore_index or lies outside [0, V) give loss 0 and a zero gradient row.  One pass
 * over the logits each way. */
#define D2T_CE_TORCH 0
#define D2T_CE_REFERENCE 1
int d2t_ce_smooth_forward(const float* logits, const int64_t* target, const float* weight, float* loss, float* lse, float* mass,
                          int32_t rows, int32_t V, int64_t ignore_index, float on, float off, int32_t mode, int64_t pad_index,
                          d2t_stream stream);
int d2t_ce_smooth_backward(const float* logits, const int64_t* target, const float* weight, const float* lse, const float* mass,
                           const float* dloss, float* dlogits, int32_t rows, int32_t V, int64_t ignore_index, float on,
                           float off, int32_t mode, int64_t pad_index, d2t_stream stream);

/* ---- fused optimizer step ----------------------------------------------------------------------------------------
 * What follows loss.backward() in the reference's training step (engine/training.py:139-150): clip_grad_norm_(max_norm)
 * and Adam / AdamW .step(), as multi-tensor kernels over a table of chunks (one block = one run of at most
 * D2T_OPTIM_CHUNK elements of one tensor; 16-byte accesses where all of a chunk's pointers allow, scalar ones otherwise):
 *   1. norm = sqrt(sum over every record of g * g): one fp32 sum per thread, all above it in double and in a fixed order
 *      (bit-reproducible, no atomics); coef = min(1, max_grad_norm / (norm + 1e-6)) stays in device memory;
 *   2. per element, in fp32 and in torch's order of operations:
 *        g' = g * coef;   decoupled (AdamW): p *= 1 - lr * wd;   otherwise (Adam): g' += wd * p;
 *        m += (g' - m) * (1 - beta1);   v = beta2 * v + (1 - beta2) * g' * g';
 *        p -= (lr / bc1) * (m / (sqrt(v) / sqrt_bc2 + eps));
 *      p, m, v are stored in place and, where the record has a mirror, the new p there as well.  The gradients are read
 *      only: they stay unclipped.
 * The mirror is the engine's raw copy of the parameter (d2t_weight_ptr): with it the engine's weights follow the step
 * and the next d2t_train_forward needs no d2t_reload_weights.  Finalized (folded / packed) inference weights are not
 * rebuilt: d2t_finalize_weights before the next inference forward.
 * The scalars of a record are doubles: bc1 = 1 - beta1^step and sqrt_bc2 = sqrt(1 - beta2^step) of that parameter's own
 * step count, formed by the caller; the products above (1 - lr * wd, lr / bc1, 1 - beta) are formed from them in double
 * and rounded to fp32 once, as torch's Python scalars are.
 * A d2t_optim owns the staging buffers of the table, the partial sums and the coefficient; it lives on the HIP device
 * that is current at d2t_optim_create, needs no d2t_ctx, and is not thread-safe.  d2t_optim_step enqueues at most three
 * launches and one host-to-device copy on `stream` and never waits for the device.  max_grad_norm <= 0: no clipping, the
 * norm is not computed and norm_dev (may be NULL) is not written; otherwise norm_dev [device float] receives the norm
 * before clipping.  Every pointer of every record (and norm_dev) must be device memory of the optimizer's device, and
 * every size non-negative: D2T_EINVAL before anything is enqueued otherwise, with a message in d2t_optim_last_error.
 * Records must not overlap one another. */
#define D2T_OPTIM_CHUNK 32768
typedef struct d2t_optim d2t_optim;
typedef struct d2t_optim_tensor {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  float* mirror; /* NULL: none */
  int64_t numel;
  double lr, weight_decay, beta1, beta2, eps, bc1, sqrt_bc2;
} d2t_optim_tensor;
int d2t_optim_create(d2t_optim** out);
void d2t_optim_destroy(d2t_optim* opt);
const char* d2t_optim_last_error(d2t_optim* opt);
int32_t d2t_optim_chunk(void); /* D2T_OPTIM_CHUNK, for bindings */
int d2t_optim_step(d2t_optim* opt, const d2t_optim_tensor* tensors, int32_t n, int32_t decoupled, float max_grad_norm,
                   float* norm_dev, d2t_stream stream);
/* ---- the optimizer family: LAMB, AdamP, MADGRAD, Lookahead (csrc/optim_family.hip) -----------------------------------
 * The other optimizers of the reference's builder (modules/optim/builder.py:76-94) on the same pattern and the same
 * d2t_optim object: a table of chunks through its staging rotation, 16-byte accesses where all of a chunk's pointers allow
 * and scalar ones otherwise.  For every entry point below:
 *   - it enqueues on `stream` and never waits for the device (the first call allocates scratch);
 *   - every sum above one element (p^2, u^2, the per-row dot products) is a double, added in a fixed order without
 *     atomics; the global gradient norm is d2t_optim_step's (one fp32 sum per thread, double above it).  Results are
 *     bit-reproducible for the same pointers' alignment;
 *   - every pointer of every record must be device memory of the optimizer's device, sizes non-negative and scalars
 *     finite: D2T_EINVAL before anything is enqueued otherwise, with a message in d2t_optim_last_error;
 *   - the new parameter is stored to `param` and, where given, to `mirror` (the engine's raw copy, d2t_weight_ptr); the
 *     gradients are only read.  Records must not overlap one another.  Scalars are doubles, rounded to fp32 once.
 *
 * d2t_optim_lamb_step (reference optim/lamb.py:113-216), four launches: norm = sqrt(sum g^2) over all records [norm_dev,
 * may be NULL]; divisor = norm / max_grad_norm where norm > max_grad_norm (> 0, required), else 1 -- LAMB's own rule,
 * without clip_grad_norm_'s 1e-6; then per element g' = g / divisor, m = beta1 m + beta3 g', v = beta2 v + (1 - beta2) g'^2,
 * u = (m / bc1) / (sqrt(v) / sqrt_bc2 + eps) [+ weight_decay p where weight_decay != 0].  With `adapt` (the caller sets it
 * where weight_decay != 0 or always_adapt): trust = |p| / |u| over the tensor if both are > 0, else 1, min(trust, 1) under
 * trust_clip; otherwise trust = 1.  p -= lr (u trust).  u is formed in both passes from the new m, v and the old p; the
 * per-chunk sums of p^2 and u^2 are added per tensor in chunk order by every block of the apply pass.  bc1 = sqrt_bc2 = 1
 * is bias_correction=False; beta3 = 1 is grad_averaging=False. */
typedef struct d2t_optim_lamb_tensor {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  float* mirror; /* NULL: none */
  int64_t numel;
  double lr, weight_decay, beta1, beta2, beta3, eps, bc1, sqrt_bc2;
  int32_t adapt, trust_clip;
} d2t_optim_lamb_tensor;
int d2t_optim_lamb_step(d2t_optim* opt, const d2t_optim_lamb_tensor* tensors, int32_t n, float max_grad_norm, float* norm_dev,
                        d2t_stream stream);
/* d2t_optim_adamp_step (reference optim/adamp.py:25-40, 66-129), three launches plus the two of the norm when
 * max_grad_norm > 0 (d2t_optim_step's clip: g' = g coef, norm_dev required then):
 *   1. m = beta1 m + (1 - beta1) g', v = beta2 v + (1 - beta2) g'^2; perturb = (beta1 m + (1 - beta1) g') / denom under
 *      nesterov, else m / denom, denom = sqrt(v) / sqrt_bc2 + eps; for a record with rows > 0 (a tensor of more than one
 *      dimension, rows = size(0), row length numel / rows) the sums g'.p, g'.g', p.p and p.perturb of every row;
 *   2. one block per record: cos(x, y) = x.y / (max(|x|, eps) max(|y|, eps)) as F.cosine_similarity; mode 1 (channel) where
 *      max over rows of |cos(g'_i, p_i)| < delta / sqrt(row length), else mode 2 (layer) where |cos(g', p)| over the whole
 *      tensor < delta / sqrt(numel), else 0; written to *mode [device int32, may be NULL] -- no host read;
 *   3. in a projecting mode perturb -= p_n (p.perturb) / (|p| + eps), p_n = p / (|p| + eps), over the row (mode 1) or the
 *      tensor (mode 2); p *= 1 - lr weight_decay (wd_ratio if projected, else 1) where weight_decay > 0;
 *      p -= (lr / bc1) perturb.
 * A record with rows > 0 holds at most 2^31 - 1 elements. */
typedef struct d2t_optim_adamp_tensor {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  float* mirror; /* NULL: none */
  int32_t* mode; /* NULL: the decision is not reported */
  int64_t numel, rows;
  double lr, weight_decay, beta1, beta2, eps, bc1, sqrt_bc2, delta, wd_ratio;
  int32_t nesterov, pad_;
} d2t_optim_adamp_tensor;
int d2t_optim_adamp_step(d2t_optim* opt, const d2t_optim_adamp_tensor* tensors, int32_t n, float max_grad_norm, float* norm_dev,
                         d2t_stream stream);
/* d2t_optim_madgrad_step (reference optim/madgrad.py:102-195, dense path), one launch plus the two of the norm when
 * max_grad_norm > 0 (as above).  lamb = (lr + eps) sqrt(step), formed by the caller.  Per element: where weight_decay != 0,
 * p *= 1 - lr weight_decay under decoupled_decay, else g' += weight_decay p; x = x0 where momentum != 0 (x0 is read only),
 * else p + s / (cbrt(grad_sum_sq) + eps), rebuilt before the accumulators move (x0 is not touched, may be NULL);
 * grad_sum_sq += lamb g'^2; s += lamb g'; z = x - s / (cbrt(grad_sum_sq) + eps); p = z where momentum == 0, else
 * (1 - ck) p + ck z with ck = 1 - momentum. */
typedef struct d2t_optim_madgrad_tensor {
  float* param;
  const float* grad;
  float* grad_sum_sq;
  float* s;
  float* x0;     /* used where momentum != 0 */
  float* mirror; /* NULL: none */
  int64_t numel;
  double lr, weight_decay, momentum, eps, lamb;
  int32_t decoupled_decay, pad_;
} d2t_optim_madgrad_tensor;
int d2t_optim_madgrad_step(d2t_optim* opt, const d2t_optim_madgrad_tensor* tensors, int32_t n, float max_grad_norm,
                           float* norm_dev, d2t_stream stream);
/* d2t_optim_lookahead_sync (reference optim/lookahead.py:30-41), one launch: slow += alpha (fast - slow), then fast = slow
 * and, where given, mirror = slow.  0 <= alpha <= 1. */
typedef struct d2t_optim_lookahead_tensor {
  float* fast;
  float* slow;
  float* mirror; /* NULL: none */
  int64_t numel;
} d2t_optim_lookahead_tensor;
int d2t_optim_lookahead_sync(d2t_optim* opt, const d2t_optim_lookahead_tensor* tensors, int32_t n, float alpha,
                             d2t_stream stream);
/* Device pointer and element count of the engine's raw copy of a loaded tensor, by state_dict key: what d2t_read_weight
 * copies from and d2t_reload_weights writes to.  Valid until the tensor is loaded again with another size or the context
 * is destroyed.  D2T_ESTATE with a message for a name that is not loaded. */
int d2t_weight_ptr(d2t_ctx* ctx, const char* name, float** ptr_out, int64_t* numel_out);

/* ---- validation metrics -------------------------------------------------------------------------------------------
 * The quadratic half of the reference's validation_step (engine/inferencing.py:133-134,226: Levenshtein distances and
 * BLEU's clipped n-gram counts) as two kernels (csrc/metrics.hip).  Stateless like the criterion: no ctx, device
 * pointers and a stream in, asynchronous, integers out, one result per sample and no atomics.
 *
 * d2t_metric_edit_distance: dist[p] = Levenshtein distance (insert, delete, substitute, each 1) of the int32 symbol
 * strings a_sym[a_off[p] .. a_off[p+1]) and b_sym[b_off[p] .. b_off[p+1]), p < N; symbols are compared as integers.
 * a_off / b_off hold N + 1 int64 each; a_total / b_total are the element counts of a_sym / b_sym (a symbol pointer may be
 * NULL where its count is 0).  One block per pair runs an anti-diagonal wavefront over three rolling diagonals as long as
 * the pair's SHORTER string + 1: in LDS while that string has at most D2T_METRIC_ED_LDS_LEN symbols, otherwise in the
 * caller's workspace.  max_len is the caller's bound on every string of the call, since the lengths themselves are device
 * data: max_len > D2T_METRIC_ED_MAX_LEN, or a workspace smaller than d2t_metric_edit_distance_workspace(N, max_len)
 * reports (0 bytes for max_len <= D2T_METRIC_ED_LDS_LEN; workspace may then be NULL), is D2T_EINVAL and nothing is
 * launched.  Nothing is ever truncated: a pair whose offsets decrease, leave [0, total] or span more than max_len gets
 * dist -1 and none of its symbols is read. */
#define D2T_METRIC_ED_MAX_LEN 32768
#define D2T_METRIC_ED_LDS_LEN 4095
int d2t_metric_edit_distance_workspace(int32_t N, int64_t max_len, int64_t* bytes_out);
int d2t_metric_edit_distance(const int32_t* a_sym, const int64_t* a_off, int64_t a_total, const int32_t* b_sym,
                             const int64_t* b_off, int64_t b_total, int32_t* dist, int32_t N, int64_t max_len,
                             void* workspace, int64_t workspace_bytes, d2t_stream stream);
/* d2t_metric_bleu_counts: candidate rows cand [N][cand_cols] and reference rows ref [N][ref_cols], int64 tokens.  A row's
 * length is the position of its first end_token, or the whole row without one (converter.detokenize).  out [N][2 + max_n]
 * int64 = cand_len, ref_len, clipped_1 .. clipped_max_n, where clipped_n = sum over the distinct n-grams of min(count in
 * the candidate, count in the reference) (modules/metrics/bleu.py:96-105 with one reference), counted without a hash
 * table: candidate n-gram i counts when fewer equal candidate n-grams precede it than the reference holds.  One block per
 * sample, both rows in LDS.  1 <= max_n <= 4; 1 <= cols <= D2T_METRIC_BLEU_MAX_COLS each: D2T_EINVAL and nothing launched
 * otherwise. */
#define D2T_METRIC_BLEU_MAX_COLS 2048
int d2t_metric_bleu_counts(const int64_t* cand, int32_t cand_cols, const int64_t* ref, int32_t ref_cols, int32_t N,
                           int64_t end_token, int32_t max_n, int64_t* out, d2t_stream stream);

/* ---- op-level TRAINING test entry points ---------------------------------------------------------------------
 * One node of the training tape, forward + backward, on caller tensors (fp32, device, row-major [rows][cols]; maps
 * NHWC; convolution weights OIHW as in the state_dict).  They run the very builders / backward functions of
 * d2t_train_forward / d2t_train_backward, so the backward kernels can be checked one op at a time.  Output pointers may
 * be NULL.  bf16x3 != 0: split-bf16 arithmetic for the convolution / data-gradient / weight-gradient GEMMs.
 * Synchronous (the call returns after the stream has drained). */
/* y = [relu]( BN_batchstats( conv(x, w) ) [+ residual] )  (gamma != NULL)   or   conv(x, w) + bias  (gamma == NULL).
 * Cin == 1 or 3 selects the stem (3x3, pad 1, BN + ReLU, 32 output channels: resnet.py:205-207); x is then the image,
 * NCHW planar [B,Cin,H,W], and no dx is written (the image needs no gradient). */
int d2t_op_train_conv(const float* x, const float* w, const float* bias, const float* gamma, const float* beta,
                      const float* residual, const float* dy, float* y, float* dx, float* dw, float* dbias,
                      float* dgamma, float* dbeta, float* dres, int32_t B, int32_t H, int32_t W, int32_t Cin,
                      int32_t Cout, int32_t KH, int32_t KW, int32_t SH, int32_t SW, int32_t PH, int32_t PW, int32_t relu,
                      int32_t bf16x3, d2t_stream stream);
/* y = [relu](x @ w^T + bias) [+ residual];  x [M][K], w [N][K] */
int d2t_op_train_linear(const float* x, const float* w, const float* bias, const float* residual, const float* dy, float* y,
                        float* dx, float* dw, float* dbias, float* dres, int32_t M, int32_t K, int32_t N, int32_t relu,
                        int32_t bf16x3, d2t_stream stream);
int d2t_op_train_layernorm(const float* x, const float* gamma, const float* beta, const float* dy, float* y, float* dx,
                           float* dgamma, float* dbeta, int32_t rows, int32_t D, float eps, d2t_stream stream);
/* nn.MultiheadAttention core: q [nb*Lq][heads*hd], kv [nb*Lk][2*heads*hd] (keys | values); keytok (optional) [nb][Lk]
 * token ids whose PAD (0) entries are masked (tgt_key_padding_mask); causal != 0 adds the causal mask. */
int d2t_op_train_attention(const float* q, const float* kv, const int64_t* keytok, const float* dy, float* y, float* dq,
                           float* dkv, int32_t nb, int32_t Lq, int32_t Lk, int32_t heads, int32_t hd, int32_t causal,
                           d2t_stream stream);
/* The same node with everything the training step passes it (Tr::attention + Tr::bwd_attn themselves; tests/test_train_attn_ops_gpu.py).
 * layout 0, separate: q [nb*Lq][D], kv [nb*Lk][2D] as above (D = heads*hd); gradients dq, dkv.
 * layout 1, packed: qkv [nb*L][3D], one tape tensor passed as both operands with column offsets 0 / D / 2D, the call of the ViT
 *   blocks and of the decoder's self-attention; needs Lq == Lk; gradient dqkv [nb*L][3D].
 * dropmask (optional): keep mask [nb][heads][Lq][Lk], bytes, of nn.MultiheadAttention's dropout on the probabilities, used
 *   with dropscale (finite, > 0) instead of a drawn mask.
 * Outputs, each optional: y [nb*Lq][D]; dq / dkv or dqkv; probs [nb][heads][Lq][Lk], the saved softmax, copied on the stream
 *   between forward and backward; ds, the same shape, what the backward left in its place.
 * plan (optional, host): {forward form, forward waves, backward form, backward waves} as the launchers select them; forward
 *   0 = K / V in LDS, 1 = K / V from global memory; backward 0 = coalesced "fast", 1 = plain LDS, 2 = global K / V; waves 0 =
 *   the launcher refuses the shape.
 * Every tape buffer of the entry (y, probs, the gradients of q / kv / qkv) starts as 0xFF bytes, so an element no kernel
 * writes comes back NaN.  Every size is checked before anything is launched: D2T_EINVAL with nothing written (plan included).
 * A shape the launchers refuse (Lk > 10240) is a non-zero status with plan filled and no other buffer touched. */
typedef struct d2t_op_train_attention_args {
  const float *q, *kv, *qkv, *dy;
  const int64_t* keytok;
  const uint8_t* dropmask;
  float *y, *dq, *dkv, *dqkv, *probs, *ds;
  int32_t* plan;
  float dropscale;
  int32_t layout, nb, Lq, Lk, heads, hd, causal;
} d2t_op_train_attention_args;
int d2t_op_train_attention_ex(const d2t_op_train_attention_args* a, d2t_stream stream);
int d2t_op_train_maxpool(const float* x, const float* dy, float* y, float* dx, int32_t B, int32_t H, int32_t W, int32_t C,
                         int32_t SH, int32_t SW, int32_t PH, int32_t PW, d2t_stream stream);
/* The backward kernels of the recurrent paths one at a time (csrc/train_recurrent.hip; test infrastructure with the rules of
 * d2t_op_bilstm above: kernel layouts, asynchronous on the stream, H = D = E = 256).
 * BiLSTM through time: dout [B][T][2H]; sv_gates / sv_c as d2t_op_bilstm saved them; whh_fwd / whh_rev [4H][H] as stored;
 * dgates [B*T][2*4H] = the gradient of the pre-activation gates. */
int d2t_op_bilstm_bwd(const float* dout, const float* sv_gates, const float* sv_c, const float* whh_fwd, const float* whh_rev,
                      float* dgates, int32_t B, int32_t T, int32_t H, d2t_stream stream);
/* Backward of the teacher-forced LSTM-attention loop (launch_attn_train_lstm_bwd; struct AttnTrainBwdP of csrc/kernels.h).
 * dlogits [B][S][V]; mem / kp [B][T][256]; wg_t [256][V]; wih_raw [1024][512], whh_raw [1024][256], wq_raw [256][256] as stored;
 * the sv_* of the forward.  dmem / dkp [B][T][256] are zeroed by the entry, then accumulated into.  Per-(row, step) factors:
 * dgates [B][S][1024], dhq [B][S][256], demb [B][S][256] (optional); dh0 / dc0 [B][256]; per-row partials dwloc [B][256][taps],
 * dbloc / dwscore [B][256], dbscore [B].  dhl (optional) [B][S][256] = dlogits . generator.weight; required when V > 1024. */
typedef struct d2t_op_attn_lstm_bwd_args {
  const float *dlogits, *mem, *kp, *wg_t, *wih_raw, *whh_raw, *wq_raw, *wloc, *bloc, *wscore;
  const float *sv_cprev, *sv_cafter, *sv_gates, *sv_alpha, *sv_hq, *dhl;
  float *dmem, *dkp, *dgates, *dhq, *demb, *dh0, *dc0, *dwloc, *dbloc, *dwscore, *dbscore;
  int32_t B, T, S, V, taps, key_off, coverage;
} d2t_op_attn_lstm_bwd_args;
int d2t_op_attn_lstm_bwd(const d2t_op_attn_lstm_bwd_args* a, d2t_stream stream);
/* Gradients of loc_conv.weight [kd][taps], loc_conv.bias [kd], loc_proj.weight [H][kd], loc_proj.bias [H] from the per-row
 * partials of the folded filter, dwloc [B][H][taps] and dbloc [B][H]. */
int d2t_op_loc_unfold_bwd(const float* dwloc, const float* dbloc, int32_t B, const float* conv_w, const float* conv_b,
                          const float* proj_w, int32_t H, int32_t kd, int32_t taps, float* d_conv_w, float* d_conv_b,
                          float* d_proj_w, float* d_proj_b, d2t_stream stream);

/* ---- the remaining kernels of the training step one at a time (test infrastructure; tests/test_train_small_ops_gpu.py) ----
 * Thin: each entry launches exactly what the tape (csrc/train.hip) or the engine launches, on caller tensors (fp32, device,
 * maps NHWC).  Every size is checked before anything is launched; what a kernel does not serve is D2T_EINVAL with nothing
 * written.  The d2t_op_train_* entries run one node of the tape, forward + backward, and are synchronous as the ones above
 * (output pointers may be NULL); the others are asynchronous on the stream unless stated. */
/* GlobalContext's pooling node (Tr::gc_pool / Tr::bwd_gc_pool): ctx[b] = sum_p softmax_p(x[b] . wg + bg)[p] x[b][p].
 * x [B][H*W][C], wg [C], bg [1], dctx [B][C] -> ctx [B][C], dx as x, dwg [C], dbg [1].  C % 4 == 0, 4 <= C <= 512. */
int d2t_op_train_gc_pool(const float* x, const float* wg, const float* bg, const float* dctx, float* ctx, float* dx, float* dwg,
                         float* dbg, int32_t B, int32_t H, int32_t W, int32_t C, d2t_stream stream);
/* GlobalContext's closing node (Tr::bcast_add): out[b][p] = x[b][p] + y[b].  x, dout, out, dx [B][HW][C]; y, dy [B][C].
 * C % 4 == 0, 4 <= C <= 512. */
int d2t_op_train_bcast_add(const float* x, const float* y, const float* dout, float* out, float* dx, float* dy, int32_t B,
                           int32_t HW, int32_t C, d2t_stream stream);
/* The fused GlobalContext block of the inference path (launch_global_context), in place on x [B][HW][C]: x += fc2(relu(
 * LayerNorm(fc1(ctx)))), eps 1e-5.  wg [C], bg [1], w1 / w2 [C][C], b1 / ln_g / ln_b / b2 [C]; ctx_out (optional) [B][C]
 * receives the pooled vector.  C % 4 == 0, 4 <= C <= 512.  Synchronous (temporary buffers). */
int d2t_op_global_context(float* x, const float* wg, const float* bg, const float* w1, const float* b1, const float* ln_g,
                          const float* ln_b, const float* w2, const float* b2, float* ctx_out, int32_t B, int32_t HW, int32_t C,
                          d2t_stream stream);
/* x[r] = E[tok[r]] * scale + pe[r % L]: E [V][D], pe [>= L][D], tok [rows], x [rows][D].  The tokens are copied to the host and
 * checked against V first (the entry synchronises the stream for that). */
int d2t_op_embed_train(const float* E, const float* pe, const int64_t* tok, float* x, int32_t rows, int32_t L, int32_t V,
                       int32_t D, float scale, d2t_stream stream);
/* dE[v] = scale * sum_{r: tok[r] == v} dx[r], rows added in ascending order; zero for v == pad_id and for absent tokens.
 * dx [rows][D], dE [V][D], 1 <= D <= 1024. */
int d2t_op_embed_bwd(const float* dx, const int64_t* tok, float* dE, int32_t rows, int32_t V, int32_t D, float scale,
                     int32_t pad_id, d2t_stream stream);
/* Philox4x32-10 keep mask (bytes, n of them) and its application out = mask ? a * scale : 0.  0 <= p < 1. */
int d2t_op_dropout_mask(uint8_t* mask, int64_t n, float p, uint64_t seed, uint64_t stream_id, d2t_stream stream);
int d2t_op_apply_mask(const float* a, const uint8_t* mask, float scale, float* out, int64_t n, d2t_stream stream);
/* ViTEncoder's learned table resized by ATen's bicubic rule (csrc/posembed.hip); scale_h / scale_w = 1 / scale_factor.
 * transpose == 0: src [GH*GW][D] -> dst [gh*gw][D];  transpose != 0 (the gradient): src [gh*gw][D] -> dst [GH*GW][D]. */
int d2t_op_bicubic_table(const float* src, float* dst, int32_t GH, int32_t GW, int32_t gh, int32_t gw, int32_t D, float scale_h,
                         float scale_w, int32_t transpose, d2t_stream stream);
/* out[i] = sum_b x[b * stride + i], i < n <= stride */
int d2t_op_sum_over_batch(const float* x, float* out, int32_t B, int64_t stride, int64_t n, d2t_stream stream);
/* scatter == 0: dst [B][n][D] = rows skip ... skip + n - 1 of every image of src [B][n + skip][D];  scatter != 0: the inverse,
 * src [B][n][D] -> dst [B][n + skip][D] with zero skip rows */
int d2t_op_token_rows(const float* src, float* dst, int32_t B, int32_t n, int32_t skip, int32_t D, int32_t scatter,
                      d2t_stream stream);
/* out[c] = sum_b x[(b * stride_rows + row) * D + c],  0 <= row < stride_rows */
int d2t_op_sum_rows_strided(const float* x, float* out, int32_t B, int64_t stride_rows, int32_t row, int32_t D,
                            d2t_stream stream);
/* Tr::mean_h: y[b][w] = mean_h x[b][h][w].  x, dx [B][H][W][C]; y, dy [B][W][C]. */
int d2t_op_train_mean_h(const float* x, const float* dy, float* y, float* dx, int32_t B, int32_t H, int32_t W, int32_t C,
                        d2t_stream stream);
/* Tr::pool with a 2 x KW window, KW 1 (VGG's (2,1) pools) or 2; otherwise as d2t_op_train_maxpool.  C % 4 == 0,
 * PH <= 1, PW <= KW / 2. */
int d2t_op_train_maxpool_w(const float* x, const float* dy, float* y, float* dx, int32_t B, int32_t H, int32_t W, int32_t C,
                           int32_t KW, int32_t SH, int32_t SW, int32_t PH, int32_t PW, d2t_stream stream);
/* Tr::gelu (op 0) or Tr::relu (op 1) over n elements, n % 4 == 0: y = f(x), dx = dy f'(x) */
int d2t_op_train_ew(const float* x, const float* dy, float* y, float* dx, int64_t n, int32_t op, d2t_stream stream);

/* ---- the weight-gradient, BatchNorm, LayerNorm, stem and data-movement kernels of the training step one LAUNCHER at a time
 * (test infrastructure; tests/test_train_gemm_ops_gpu.py) ----
 * Each entry calls one launcher of csrc/train_wgrad.hip / train_kernels.hip on caller tensors in the kernel's own layout
 * (fp32, device, row-major, maps NHWC), asynchronously on the stream, so that a NaN pre-fill and a guard tail of the caller's
 * buffers speak about the kernel itself.  Every size is checked before anything is launched; what a launcher does not serve is
 * D2T_EINVAL with nothing written. */
/* launch_wgrad: part[z][tap][m][n] = sum_{p in chunk z} a[p][m] * b[src(p, tap)][n], z < S, chunk z = rows [z chunk, (z+1) chunk).
 * a [P][lda], part [S][taps][M][N].  geom == 0: b [P][ldb], src(p) = p, taps = 1.  geom != 0: b is the NHWC map [B][H][W][ldb],
 * row p = output pixel (b, oh, ow) of [B][OH][OW], tap = kh * KW + kw reads (oh * SH - PH + kh, ow * SW - PW + kw), zero in the
 * padding; taps = KH * KW and P = B * OH * OW.  S * chunk >= P > (S - 1) * chunk.  M, N, lda, ldb % 4 == 0.
 * bf16x3: split-bf16 arithmetic where the launcher has it (M, N > 64).  records != 0: the entry builds both operand records
 * (launch_split_act, format 0) in buffers of its own with a zero page of its own and passes them; that needs geom, bf16x3,
 * lda == M, ldb == N, chunk % 16 == 0 and a tile for (M, N), and the entry then waits for the stream before it returns.
 * tile (optional, host): [2] receives the block tile taken -- bm, bn of the record kernel, or 64, 64 / 128, 128. */
typedef struct d2t_op_wgrad_args {
  const float *a, *b;
  float* part;
  int32_t* tile;
  int64_t P;
  int32_t M, N, lda, ldb, geom, B, H, W, OH, OW, KH, KW, SH, SW, PH, PW, S, chunk, bf16x3, records;
} d2t_op_wgrad_args;
int d2t_op_wgrad(const d2t_op_wgrad_args* a, d2t_stream stream);
/* Host only: the S / chunk Tr::wgrad chooses for P rows of an M x N gradient with `taps` filter taps; records != 0: for the
 * record kernel (EINVAL where (M, N) has no tile).  out [4] = S, chunk, tile bm, tile bn. */
int d2t_op_wgrad_plan(int64_t P, int32_t M, int32_t N, int32_t taps, int32_t records, int64_t* out);
/* launch_wgrad_reduce: dst = (accumulate ? dst : 0) + sum_z part[z][tap][m][n]; layout 0: dst [M][N] (taps == 1), layout 1:
 * OIHW dst [M][N][taps].  The kernel with one block per output is taken for (taps M N <= 4096 and S >= 256) or
 * (taps M N <= 65536 and S >= 128). */
int d2t_op_wgrad_reduce(const float* part, float* dst, int32_t S, int32_t taps, int32_t M, int32_t N, int32_t layout,
                        int32_t accumulate, d2t_stream stream);
/* launch_colreduce: per-chunk column sums of [R][C] matrices into part [chunks][2][C] (mode 0: sum a | 0;  1: the sums about
 * the channel's value in row 0, sum (a - a[0][c]) | sum (a - a[0][c])^2;
 * 2 (BatchNorm backward): g = dy (y > 0 where y is given) -> sum g | sum g (z - mean[c]) rstd[c];  3 (LayerNorm backward):
 * sum a | sum a (z - mean[r]) rstd[r]).  *chunks (host) receives colreduce_chunks(R, C); with part == NULL nothing else happens.
 * C % 4 == 0. */
int d2t_op_colreduce(int32_t mode, const float* a, const float* y, const float* z, const float* mean, const float* rstd,
                     float* part, int64_t R, int32_t C, int32_t* chunks, d2t_stream stream);
/* launch_colreduce_final: out0[c] = (accumulate ? out0[c] : 0) + sum_k part[k][0][c], out1 (optional) from part[k][1][c] */
int d2t_op_colreduce_final(const float* part, int32_t chunks, int32_t C, float* out0, float* out1, int32_t accumulate,
                           d2t_stream stream);
/* launch_bn_finalize: part [chunks][2][C] of mode 1 over z [R][C] (the same z: its row 0 is the shift of the sums) -> mean,
 * rstd = 1 / sqrt(biased variance + eps); run_mean / run_var (both or neither) updated in place with `momentum` and the
 * unbiased variance (the biased one where R == 1) */
int d2t_op_bn_finalize(const float* part, int32_t chunks, int32_t C, int64_t R, float eps, float momentum, const float* z,
                       float* mean, float* rstd, float* run_mean, float* run_var, d2t_stream stream);
/* launch_bn_apply: y = act((z - mean) rstd gamma + beta (+ res)), [R][C], C % 4 == 0; planes (optional, C % 32 == 0): the
 * split-bf16 records of y, R * C * 2 uint16 */
int d2t_op_bn_apply(const float* z, const float* mean, const float* rstd, const float* gamma, const float* beta, const float* res,
                    float* y, uint16_t* planes, int64_t R, int32_t C, int32_t relu, d2t_stream stream);
/* launch_bn_bwd_apply: g = dy (y > 0 where y is given); dz = gamma rstd (g - s0 / R - xhat s1 / R); gout (optional) = g;
 * planes (optional, C % 32 == 0): the records of dz */
int d2t_op_bn_bwd_apply(const float* dy, const float* y, const float* z, const float* mean, const float* rstd,
                        const float* gamma, const float* s0, const float* s1, float* dz, float* gout, uint16_t* planes, int64_t R,
                        int32_t C, d2t_stream stream);
/* launch_ln_train / launch_ln_bwd: LayerNorm over rows of D = 128, 256 or 512 with saved mean / rstd [rows];
 * dx = rstd (dy gamma - mean_c(dy gamma) - xhat mean_c(dy gamma xhat)) (+ add) */
int d2t_op_ln_train(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, int32_t rows,
                    int32_t D, float eps, d2t_stream stream);
int d2t_op_ln_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma, const float* add,
                  float* dx, int32_t rows, int32_t D, d2t_stream stream);
/* launch_stem_raw: z [B][H][W][Cout] = conv3x3, pad 1 of the NCHW image [B][Cin][H][W] with raw OIHW weights, no bias.
 * launch_stem_wgrad: part [nchunks][9 Cin][Cout], tap = (ci * 3 + kh) * 3 + kw, over pixel chunks of `chunk` rows of
 * dz [B H W][Cout]; nchunks * chunk >= B H W > (nchunks - 1) * chunk.  Cin 1 or 3, Cout 32 or 64. */
int d2t_op_stem_raw(const float* img, const float* w, float* z, int32_t B, int32_t Cin, int32_t H, int32_t W, int32_t Cout,
                    d2t_stream stream);
int d2t_op_stem_wgrad(const float* img, const float* dz, float* part, int32_t B, int32_t Cin, int32_t H, int32_t W, int32_t Cout,
                      int32_t chunk, int32_t nchunks, d2t_stream stream);
/* dst [B][DH][DW][C]: dst[b][oh SH + offh][ow SW + offw] = src[b][oh][ow] where that lies inside, zero elsewhere */
int d2t_op_dilate(const float* src, float* dst, int32_t B, int32_t OH, int32_t OW, int32_t C, int32_t DH, int32_t DW, int32_t SH,
                  int32_t SW, int32_t offh, int32_t offw, d2t_stream stream);
/* out [Cin][Cout][KH][KW] = w [Cout][Cin][KH - 1 - kh][KW - 1 - kw] */
int d2t_op_flip_oihw(const float* w, float* out, int32_t Cout, int32_t Cin, int32_t KH, int32_t KW, d2t_stream stream);
/* dst [rows][Cd] = src [rows][Cs] zero-padded on the right, Cd >= Cs */
int d2t_op_pad_cols(const float* src, float* dst, int64_t rows, int32_t Cs, int32_t Cd, d2t_stream stream);
/* dst[r][0 .. cols) = src[r][0 .. cols), row strides lds, ldd >= cols; the rest of dst is not written */
int d2t_op_copy2d(const float* src, int32_t lds, float* dst, int32_t ldd, int64_t rows, int32_t cols, d2t_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* D2T_H */
