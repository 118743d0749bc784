"""Thin Python owner of a libd2t context: config marshalling, weight upload,
encode / decode calls on torch ROCm tensors.  No compute happens here."""
import ctypes as C

import torch

from . import _lib


def config_from_opt(opt):
    """Flat reference config dict (config/train.yaml schema) -> D2TConfig.  FeatureExtraction.params.mean_height is read
    where it is present: FeatExtractorBuilder pops it from the caller's dict (build_feat.py:16), so a Model hands its engine
    Model.engine_opt(), which carries the popped value."""
    feat = opt["FeatureExtraction"]["name"]
    seq = opt["SequenceModeling"]["name"]
    pred = opt["Prediction"]
    pp = pred["params"]
    cfg = _lib.D2TConfig()
    max_dim = opt.get("max_dimension") or [0, 0]
    if opt.get("imgH"):
        max_dim = (opt["imgH"], max_dim[1])  # vit_encoder.py:292-294
    cfg.max_h, cfg.max_w = int(max_dim[0]), int(max_dim[1])
    cfg.backbone_out = 512
    cfg.in_channels = 1
    if seq == "ViT":
        sp = opt["SequenceModeling"]["params"]
        bbp = sp.get("backbone") or {}
        if bbp.get("name") != "resnet":
            raise NotImplementedError("ViT without the resnet hybrid backbone cannot run in the reference either "
                                      "(PatchEmbed returns a 3-tuple, SURVEY.md 3 notes)")
        if sp.get("patching_style") != "2d":
            raise NotImplementedError("patching_style '1d' (TRIGBaseEncoder) crashes in the reference: HybridEmbed1D has no "
                                      "patch_size attribute for build_seq.py:63-66 to read")
        # create_vit_modeling, vit_encoder.py:295-302
        if sp.get("fix_embed", False):
            cfg.vit_pos = _lib.VIT_POS_SINCOS_PREFIX       # ViTEncoderV3
        elif not sp.get("interpolate_embed", True):
            cfg.vit_pos = _lib.VIT_POS_LEARNED_PREFIX      # ViTEncoderV2
        else:
            cfg.vit_pos = _lib.VIT_POS_LEARNED_INTERP      # ViTEncoder
        cfg.gcb = int(bool(bbp.get("gcb", False)))
        cfg.encoder = _lib.ENC_HYBRID_VIT
        cfg.in_channels = int(bbp["input_channel"])
        cfg.backbone_out = int(bbp["output_channel"])
        cfg.vit_depth, cfg.vit_heads, cfg.vit_dim = int(sp["depth"]), int(sp["num_heads"]), int(sp["hidden_size"])
        ps = sp["patch_size"]
        ps = (ps, ps) if isinstance(ps, int) else tuple(ps)
        cfg.patch_h, cfg.patch_w = int(ps[0]), int(ps[1])
    elif feat in ("ResNet", "VGG") and seq in ("None", "BiLSTM"):
        fp = opt["FeatureExtraction"]["params"]
        if fp.get("gcb", False) and feat == "VGG":
            raise NotImplementedError("gcb is a ResNet option")
        cfg.gcb = int(bool(fp.get("gcb", False))) if feat == "ResNet" else 0
        cfg.in_channels = int(fp["input_channel"])
        cfg.backbone_out = int(fp["output_channel"])
        if seq == "BiLSTM":
            cfg.encoder = _lib.ENC_VGG_BILSTM if feat == "VGG" else _lib.ENC_RESNET_BILSTM
            cfg.bilstm_hidden = int(opt["SequenceModeling"]["params"]["hidden_size"])
            if opt["SequenceModeling"]["params"].get("pos_enc", False):
                raise NotImplementedError("BiLSTM pos_enc crashes in the reference (self.gated undefined, build_seq.py:55)")
            if cfg.bilstm_hidden != 256:
                raise NotImplementedError(f"BiLSTM hidden_size must be 256 (the recurrent kernels are built for it), got "
                                          f"{cfg.bilstm_hidden}")
            if pred["name"] == "TFM" and int(pp["d_model"]) != cfg.bilstm_hidden:
                raise NotImplementedError(f"a TFM head behind the BiLSTM needs d_model = the BiLSTM hidden_size = 256, got d_model "
                                          f"{int(pp['d_model'])} (the reference fails in cross-attention when the two differ)")
            # mean_height False (build_feat.py:33-40,56-61): proj_feat over the flattened height instead of its mean
            cfg.proj_height = int(not fp.get("mean_height", True))
        elif pred["name"] != "TFM":
            raise NotImplementedError(f"Feat={feat} with Seq=None and Pred={pred['name']} crashes in the reference: "
                                      "SeqModelingBuilder.forward reads self.AdaptiveAvgPool, which only FeatExtractorBuilder "
                                      "has (build_seq.py:78; Attnv2 matches neither branch and leaves the result unbound)")
        else:  # + PositionalEncoding2D, [B,C,H,W] -> [B,HW,C] (build_seq.py:69-76); proj_feat, if built, is never used
            cfg.encoder = _lib.ENC_RESNET if feat == "ResNet" else _lib.ENC_VGG
    else:
        raise NotImplementedError(f"Feat={feat} Seq={seq} is not on the accelerated path")
    cfg.vocab = int(opt["num_class"])
    cfg.batch_max_length = int(opt.get("batch_max_length", 0))
    if pred["name"] == "TFM":
        cfg.decoder = _lib.DEC_TFM
        cfg.dec_dim, cfg.dec_heads = int(pp["d_model"]), int(pp["nhead"])
        cfg.dec_layers, cfg.dec_ff = int(pp["num_decoder_layers"]), int(pp["dim_feedforward"])
        cfg.max_seq_len = int(pp["max_seq_len"])
    elif pred["name"] in ("Attn", "Attnv2"):
        cfg.decoder = _lib.DEC_ATTN
        cfg.attn_hidden = int(pp["hidden_size"])
        cfg.attn_kernel_size, cfg.attn_kernel_dim = int(pp["kernel_size"]), int(pp["kernel_dim"])
        cfg.attn_enc_init = int(bool(pp.get("enc_init", False)))
        attn_type = pp.get("attn_type", "coverage")
        if attn_type == "luong":  # constructs in the reference, but no forward can run (build_model raises before any engine exists)
            raise AttributeError("'LuongAttention' object has no attribute 'reset_mem'")
        cfg.attn_coverage = int(attn_type == "coverage")
        cfg.attn_cell = _lib.ATTN_CELL_LOCATION if attn_type in ("coverage", "loc_aware") else _lib.ATTN_CELL_BAHDANAU
        cfg.attn_onehot = int(not pp.get("embed_target", False))
        if cfg.attn_cell == _lib.ATTN_CELL_BAHDANAU:
            cfg.attn_kernel_size, cfg.attn_kernel_dim = 0, 1  # no location filter
        sm = pp.get("seqmodel", "ViT")
        if pred["name"] == "Attnv2":  # seq2seq_v2.py:182-199
            if sm in ("BiLSTM", "VIG"):
                cfg.attn_keys = _lib.ATTN_KEYS_ALL_INIT_MEAN
            elif sm == "TFM":
                cfg.attn_keys = _lib.ATTN_KEYS_NOCLS_INIT_CLS
            else:
                raise ValueError("seqmodel must be either BiLSTM or TFM option")
        else:  # seq2seq.py:229-238
            cfg.attn_keys = _lib.ATTN_KEYS_ALL_INIT_MEAN if sm == "BiLSTM" else _lib.ATTN_KEYS_ALL_INIT_FIRST
    else:
        raise NotImplementedError(f"Prediction '{pred['name']}' is not on the accelerated path")
    return cfg


def device_index(device):
    """opt["device"] as the reference passes it around ('cuda', 'cuda:1', a torch.device, None) -> HIP device index."""
    if device is None or (isinstance(device, str) and device in ("", "cpu")):
        return torch.cuda.current_device()  # the engine has no CPU path; 'cpu' configs get the current GPU
    d = torch.device(device)
    if d.type != "cuda":
        raise RuntimeError(f"doc2tex_amd: device '{device}' is not a ROCm (cuda) device; the engine has no CPU path")
    return torch.cuda.current_device() if d.index is None else int(d.index)


def ragged_tables(layout):
    """The tables of a ragged decode group, as the engine writes them for its kernels: layout = [(rows_i, T_i)] per batch ->
    dict(row0, len, row_batch, batch_rows, rows, mem_rows).  Row b (batch order) attends over the len[b] memory rows that
    start at row row0[b] of the packed [sum rows_i * T_i][d] buffer; row_batch[b] is its batch, batch_rows[k] the rows of
    batch k.  Pure host arithmetic (lists of ints)."""
    row0, length, row_batch, batch_rows = [], [], [], []
    base = 0
    for k, (rows, T) in enumerate(layout):
        rows, T = int(rows), int(T)
        if rows < 1 or T < 1:
            raise ValueError(f"batch {k} of the group has {rows} rows of memory length {T}")
        for i in range(rows):
            row0.append(base + i * T)
            length.append(T)
            row_batch.append(k)
        batch_rows.append(rows)
        base += rows * T
    return {"row0": row0, "len": length, "row_batch": row_batch, "batch_rows": batch_rows, "rows": len(row0), "mem_rows": base}


def ragged_beam_tables(lengths):
    """The per-SAMPLE tables of a ragged beam search, as the engine writes them (d2t_ragged_beam_tables): sample i's memory
    occupies the lengths[i] rows from row0[i] on of the packed [sum lengths][d] buffer -> dict(row0, len, mem_rows).  Pure
    host arithmetic (lists of ints)."""
    row0, base = [], 0
    for i, T in enumerate(lengths):
        T = int(T)
        if T < 1:
            raise ValueError(f"sample {i} has memory length {T}")
        row0.append(base)
        base += T
    return {"row0": row0, "len": [int(T) for T in lengths], "mem_rows": base}


def pack_memories(memories):
    """Encoder memories [n_i, T_i, d] of different lengths -> (packed [sum n_i * T_i, d], lengths): the samples' rows one
    behind the other in input order, lengths[j] the memory length of flat sample j."""
    d = memories[0].shape[-1]
    lengths = []
    for m in memories:
        if m.dim() != 3 or m.shape[-1] != d:
            raise ValueError(f"expected memories [n, T, {d}], got {tuple(m.shape)}")
        lengths += [int(m.shape[1])] * int(m.shape[0])
    packed = torch.cat([m.float().reshape(-1, d) for m in memories], 0).contiguous()
    return packed, lengths


_LATE_PRECISIONS = ("fp16x2", "mixed")  # they need the pipelined16 kernel, so they follow the kernel choice

# The engine settings Model.engine() keeps in step with the model's switches, in the order they are sent:
# (name, Engine method, what a fresh context already has (None: unknown, always sent), condition or None).  A setting is
# sent when the wanted value differs from the applied one AND its condition holds; the condition is only evaluated for a
# value that differs.  A wanted tuple is passed as the method's arguments.
SETTINGS = (
    ("reserved_blocks", "set_reserved_blocks", None, None),
    ("reserved_cus", "set_reserved_cus", None, None),
    # 'fp32' / 'bf16x3' go before a change of the kernel, the others after it (below)
    ("conv_precision", "set_conv_precision", None, lambda eng, want, finalize: want["conv_precision"] not in _LATE_PRECISIONS),
    ("conv_kernel", "set_conv_kernel", None, None),
    ("beam_shared_tile", "set_beam_shared_tile", None, None),
    # only a context with finalized weights can say whether it has the device-side search
    ("attn_beam_device", "set_attn_beam_device", False, lambda eng, want, finalize: finalize and eng.supports_device_attn_beam()),
    ("conv_fusion", "set_conv_fusion", None, None),
    ("decode_chains", "set_decode_chains", None, None),
    ("conv_precision", "set_conv_precision", None, lambda eng, want, finalize: want["conv_precision"] in _LATE_PRECISIONS),
    ("mixed_units", "set_mixed_units", None, lambda eng, want, finalize: want["conv_precision"] == "mixed"),
)


def apply_settings(eng, want, finalize=True):
    """Send the settings of SETTINGS whose wanted value (want[name]) is not the one `eng.applied` records.  A value is
    recorded only after its setter returned, so one that raised is sent again by the next call."""
    for name, setter, fresh, when in SETTINGS:
        value = want[name]
        if eng.applied.get(name, fresh) == value or (when is not None and not when(eng, want, finalize)):
            continue
        getattr(eng, setter)(*(value if isinstance(value, tuple) else (value,)))
        eng.applied[name] = value
        if name == "conv_precision":  # the units are sent again with the next 'mixed'
            eng.applied.pop("mixed_units", None)


def beam_arrays(N, S):
    """Host result arrays of a beam search over N samples of up to S tokens: (seq [N * S] int64, len [N] int32, score [N]
    float).  Never empty, so that an empty list of samples still reaches the C side with valid pointers."""
    return (C.c_int64 * max(1, N * S))(), (C.c_int32 * max(1, N))(), (C.c_float * max(1, N))()


def beam_results(seq, n, score, N, S, tensor_score, alpha=None, keys=None):
    """The filled arrays of a beam search (flat seq [N * S], len [N], score [N]; anything that indexes like a list) ->
    [(LongTensor [1, len] on the CPU, score)] per sample.  The score is a Python float for the TFM head and a 0-dim tensor
    for the LSTM-attention heads, as in the reference.  alpha [N, S, >= max keys]: each entry also carries its alignment
    map, a view cut to [len, keys[i]]."""
    out = []
    for i in range(N):
        r = (torch.LongTensor(list(seq[i * S: i * S + n[i]])).unsqueeze(0),
             torch.tensor(float(score[i])) if tensor_score else float(score[i]))
        out.append(r if alpha is None else r + (alpha[i, :n[i], :keys[i]],))
    return out


def packed_rows(packed, lengths):
    """A packed memory and the lengths of its samples as the C side takes them: (fp32 contiguous [sum lengths, d], [int],
    int32 array of the lengths -- never empty, like beam_arrays)."""
    packed = packed.float().contiguous()
    lengths = [int(T) for T in lengths]
    if packed.dim() != 2 or packed.shape[0] != sum(lengths):
        raise ValueError(f"packed memory {tuple(packed.shape)} does not hold the {sum(lengths)} rows of `lengths`")
    return packed, lengths, (C.c_int32 * max(1, len(lengths)))(*lengths)


class Engine:
    def __init__(self, opt, device=None):
        self.ctx = None
        self.lib = _lib.require_device()
        self.cfg = config_from_opt(opt)
        # the context lives on ONE device: opt["device"] (build_pred.py:17) unless the module has been moved since
        self.device = device_index(opt.get("device") if device is None else device)
        if not 0 <= self.device < torch.cuda.device_count():
            raise RuntimeError(f"doc2tex_amd: no HIP device {self.device} (visible: {torch.cuda.device_count()})")
        self.ctx = C.c_void_p()
        with torch.cuda.device(self.device):
            rc = self.lib.d2t_create(C.byref(self.cfg), C.byref(self.ctx))
        try:
            self._check(rc, "d2t_create")
        except RuntimeError:
            self.__del__()
            raise
        assert self.lib.d2t_device_of(self.ctx) == self.device
        # the upload signature (None forces an upload), the one the finalized weights were built from, the shapes loaded last
        self._sig, self._fin_sig, self._loaded_shapes = None, None, None
        self.weight_uploads = 0  # sync_weights calls that moved tensors into the engine (load or reload)
        self._load_epoch = object()  # replaced whenever d2t_load_weight may have re-allocated the raw copies (weight_ptr)
        self.applied = {}  # settings sent to the context so far (apply_settings): name -> value
        self._train_keep = None  # (image, tgt) of a training forward until its backward has read them
        # submitted decodes: [(ticket, tensors)] referenced until the ticket completes, ticket -> per-batch step counts, the
        # device whose current stream decode_wait orders (None before the first submission)
        self._held, self._steps_cache, self._wait_dev = [], {}, None

    def _on_device(self, t, what):
        """Tensors handed to the context must live on its device (the C side checks the raw pointers too).  Which calls
        check here is uneven -- the TFM greedy calls, the submitted calls and the ragged group do; the synchronous greedy
        call of the LSTM-attention heads and the synchronous beam searches leave it to the C side -- and stays so: unifying
        it would change the exception their callers see."""
        if not t.is_cuda:
            raise RuntimeError(f"doc2tex_amd: {what} must be a ROCm (cuda) tensor; the engine has no CPU path")
        if t.device.index != self.device:
            raise RuntimeError(f"doc2tex_amd: {what} is on {t.device} but this model's engine lives on cuda:{self.device}; "
                               "move the input, or the Model with .to(device), so that they agree")

    def __del__(self):
        ctx, self.ctx = getattr(self, "ctx", None), None  # (an object whose __init__ never ran has no ctx)
        if ctx:
            try:
                self.lib.d2t_destroy(ctx)
            except Exception:
                pass

    def _check(self, rc, what):
        _lib.check(rc, self.ctx, what)

    # ---- weights ---------------------------------------------------------
    def sync_weights(self, module, finalize=True):
        """Upload the module's state if any tensor changed since last time; finalize=True also folds / packs it
        for inference (the training step reads the raw copies and skips that)."""
        items = []
        for name, t in list(module.named_parameters()) + list(module.named_buffers()):
            if not t.is_floating_point() or name.endswith("image_positional_encoder.pe"):
                continue
            items.append((name, t))
        sig = tuple((n, t.data_ptr(), t._version, tuple(t.shape)) for n, t in items)
        if sig == self._sig:
            if finalize and self._fin_sig != sig:
                self._check(self.lib.d2t_finalize_weights(self.ctx, _lib.stream_of(items[0][1])), "finalize_weights")
                self._fin_sig = sig
            return
        stream = None
        tds = []
        for name, t in items:
            if not t.is_cuda:
                raise RuntimeError(f"doc2tex_amd: parameter '{name}' is on {t.device}; move the Model to the GPU")
            self._on_device(t, f"parameter '{name}'")
            td = t.detach()
            if td.dtype != torch.float32 or not td.is_contiguous():
                td = td.float().contiguous()
            tds.append(td)
            stream = _lib.stream_of(td)
        shapes = tuple((n, tuple(t.shape)) for n, t in items)
        if shapes == self._loaded_shapes:
            # same tensors as last time with new contents (an optimizer step): one copy kernel instead of one copy each
            n = len(items)
            self._check(self.lib.d2t_reload_weights(
                self.ctx, n, (C.c_char_p * n)(*[nm.encode() for nm, _ in items]),
                (C.c_void_p * n)(*[td.data_ptr() for td in tds]), (C.c_int64 * n)(*[td.numel() for td in tds]), stream),
                "reload_weights")
        else:
            for (name, _), td in zip(items, tds):
                shape = (C.c_int64 * td.dim())(*td.shape)
                self._check(self.lib.d2t_load_weight(self.ctx, name.encode(), _lib.ptr(td), shape, td.dim(), stream),
                            f"load_weight({name})")
            self._loaded_shapes = shapes
            self._load_epoch = object()
        self.weight_uploads += 1
        self._fin_sig = None
        if finalize:
            self._check(self.lib.d2t_finalize_weights(self.ctx, stream), "finalize_weights")
            self._fin_sig = sig
        self._sig = sig

    def weight_ptr(self, name):
        """(device pointer, numel) of the engine's raw copy of a loaded tensor (d2t_weight_ptr), None if it is not loaded.
        The pointer holds until the tensors are loaded afresh (`_load_epoch` is then another object)."""
        p, n = C.c_void_p(), C.c_int64(0)
        if self.lib.d2t_weight_ptr(self.ctx, name.encode(), C.byref(p), C.byref(n)) != _lib.D2T_OK:
            return None
        return p.value, int(n.value)

    def weights_current(self, module, names):
        """The caller states that the engine's RAW copies of the tensors `names` already hold the module's present values
        (the fused optimizer wrote both; a training forward produced the running statistics it copied out): their
        entries of the upload signature are re-taken from the module, so the next sync_weights does not upload on their
        account.  Every other tensor keeps its old entry and is still re-uploaded if it changed.  The finalized (folded /
        packed) weights are stale either way and are rebuilt by the next sync_weights that asks for them."""
        self._fin_sig = None
        if self._sig is None:
            return
        names = set(names)
        cur = {n: t for n, t in list(module.named_parameters()) + list(module.named_buffers()) if n in names}
        self._sig = tuple((e[0], cur[e[0]].data_ptr(), cur[e[0]]._version, tuple(cur[e[0]].shape)) if e[0] in cur else e
                          for e in self._sig)

    # ---- training step -------------------------------------------------------
    def train_forward(self, image, tgt):
        """Model.forward under module.train(): logits [B,L,V] of the teacher-forced pass (BatchNorm on batch
        statistics; the engine's running statistics are updated, see read_weight)."""
        self._on_device(image, "input")
        if image.dim() != 4 or image.shape[1] != self.cfg.in_channels:
            raise ValueError(f"expected image [B,{self.cfg.in_channels},H,W], got {tuple(image.shape)}")
        image = image.float().contiguous()
        tgt = tgt.to(device=image.device, dtype=torch.int64).contiguous()
        B, _, H, W = image.shape
        L = tgt.shape[1]
        logits = torch.empty((B, L, self.cfg.vocab), dtype=torch.float32, device=image.device)
        self._train_keep = (image, tgt)  # the backward pass reads them
        self._check(self.lib.d2t_train_forward(self.ctx, _lib.ptr(image), B, H, W, _lib.ptr(tgt), L, _lib.ptr(logits),
                                               _lib.stream_of(image)), "train_forward")
        return logits

    def read_attn_alpha(self, B, L, Tk, device):
        """The alignments of the last training forward of an LSTM-attention head, [B, L, Tk] (a fresh tensor: no autograd
        history)."""
        a = torch.empty((B, L, Tk), dtype=torch.float32, device=device)
        self._check(self.lib.d2t_train_read_attn_alpha(self.ctx, _lib.ptr(a), a.numel(), _lib.stream_of(a)), "train_read_attn_alpha")
        return a

    def set_dropout(self, p, seed):
        """Dropout probability of the decoder layers in the training step and the seed of its Philox masks."""
        self._check(self.lib.d2t_train_set_dropout(self.ctx, float(p), int(seed) & 0xFFFFFFFFFFFFFFFF), "train_set_dropout")

    def set_teacher_flags(self, flags):
        """Scheduled sampling of the LSTM-attention head: flags[t] = 1 feeds the label at step t, 0 the model's own
        arg-max (seq2seq.py:311-316).  None / empty = always the label."""
        data = bytes(bytearray(int(bool(f)) for f in flags)) if flags else b""
        self._check(self.lib.d2t_train_set_teacher_flags(self.ctx, data, len(data)), "train_set_teacher_flags")

    def mask_count(self):
        return int(self.lib.d2t_train_mask_count(self.ctx))

    def read_mask(self, index, numel):
        m = torch.empty(int(numel), dtype=torch.uint8, device=f"cuda:{self.device}")
        self._check(self.lib.d2t_train_read_mask(self.ctx, int(index), _lib.ptr(m), int(numel), _lib.stream_of(m)), "train_read_mask")
        return m

    def train_backward(self, dlogits):
        dlogits = dlogits.float().contiguous()
        self._check(self.lib.d2t_train_backward(self.ctx, _lib.ptr(dlogits), _lib.stream_of(dlogits)), "train_backward")
        self._train_keep = None

    def train_grad(self, name, like):
        g = torch.empty_like(like, dtype=torch.float32, memory_format=torch.contiguous_format)
        self._check(self.lib.d2t_train_grad(self.ctx, name.encode(), _lib.ptr(g), g.numel(), _lib.stream_of(g)),
                    f"train_grad({name})")
        return g

    def train_gather(self, names, likes, source="grad"):
        """All gradients (source "grad") or the engine's copies of loaded tensors (source "weight": the BatchNorm running
        statistics after a training forward) in ONE kernel: returns fp32 tensors shaped like `likes`, views of one flat
        buffer (as DistributedDataParallel's gradient_as_bucket_view hands them out)."""
        n = len(names)
        numels = [int(t.numel()) for t in likes]
        offs, total = [], 0
        for m in numels:  # 16-byte aligned starts: the copy kernel moves float4s
            offs.append(total)
            total += (m + 3) & ~3
        if n == 0:
            return []
        flat = torch.empty(max(total, 1), dtype=torch.float32, device=likes[0].device)
        arr = (C.c_char_p * n)(*[s.encode() for s in names])
        self._check(self.lib.d2t_train_gather(self.ctx, 0 if source == "grad" else 1, n, arr, (C.c_int64 * n)(*offs),
                                              (C.c_int64 * n)(*numels), _lib.ptr(flat), _lib.stream_of(flat)),
                    "train_gather")
        return [flat[o:o + m].view(t.shape) for o, m, t in zip(offs, numels, likes)]

    def train_grad_into(self, name, dst):
        """Copy the gradient of `name` into the flat fp32 view `dst` on the current stream (ordered after the
        kernels that produce it, whichever stream that is)."""
        self._check(self.lib.d2t_train_grad(self.ctx, name.encode(), _lib.ptr(dst), dst.numel(), _lib.stream_of(dst)),
                    f"train_grad({name})")

    def read_weight(self, name, dst):
        """Copy the engine's current copy of a loaded tensor into `dst` (fp32, contiguous, same size)."""
        self._check(self.lib.d2t_read_weight(self.ctx, name.encode(), _lib.ptr(dst), dst.numel(), _lib.stream_of(dst)),
                    f"read_weight({name})")

    # ---- encoder -----------------------------------------------------------
    def encoder_shape(self, H, W):
        v = [C.c_int32() for _ in range(6)]
        self._check(self.lib.d2t_encoder_shape(self.ctx, H, W, *[C.byref(x) for x in v]), "encoder_shape")
        T, d, gh, gw, pw, ph = [x.value for x in v]
        return T, d, gh, gw, pw, ph

    def encode(self, image, attn_maps=None):
        """image [B,in_channels,H,W] (1 grey plane or 3 colour planes, as the config says) -> (memory [B,T,d], (grid_h, grid_w), (pad_w, pad_h)).  attn_maps (ViT encoders): a list of
        vit_depth entries, each None or a caller-allocated contiguous fp32 tensor [B, heads, T, T] on the image's device
        that receives that block's self-attention probabilities (the reference's attn_drop input); memory is bitwise the
        same with or without them."""
        self._on_device(image, "input")
        if image.dim() != 4 or image.shape[1] != self.cfg.in_channels:
            raise ValueError(f"expected image [B,{self.cfg.in_channels},H,W], got {tuple(image.shape)}")
        image = image.float().contiguous()
        B, _, H, W = image.shape
        T, d, gh, gw, pw, ph = self.encoder_shape(H, W)
        memory = torch.empty((B, T, d), dtype=torch.float32, device=image.device)
        if attn_maps is None:
            self._check(self.lib.d2t_encode(self.ctx, _lib.ptr(image), B, H, W, _lib.ptr(memory),
                                            _lib.stream_of(image)), "encode")
            return memory, (gh, gw), (pw, ph)
        n = len(attn_maps)
        shape = (B, self.cfg.vit_heads, T, T)
        for i, a in enumerate(attn_maps):
            if a is None:
                continue
            self._on_device(a, f"attn_maps[{i}]")
            if a.dtype != torch.float32 or tuple(a.shape) != shape or not a.is_contiguous():
                raise ValueError(f"attn_maps[{i}] must be a contiguous float32 tensor of shape {shape}, got "
                                 f"{a.dtype} {tuple(a.shape)}")
        ptrs = (C.c_void_p * max(n, 1))(*[None if a is None else _lib.ptr(a) for a in attn_maps])
        self._check(self.lib.d2t_encode_attn(self.ctx, _lib.ptr(image), B, H, W, _lib.ptr(memory), ptrs, n,
                                             _lib.stream_of(image)), "encode_attn")
        return memory, (gh, gw), (pw, ph)

    def set_conv_precision(self, mode):
        """'fp32' (exact), 'bf16x3' (split-bf16 matrix-core path for the convolutions: three products per element) or 'fp16x2'
        (fp16 feature maps times fp16 hi / lo weights in the backbone: two products per element), or 'mixed' ('bf16x3' with the
        'fp16x2' arithmetic in the first few 512 -> 512 units of the backbone only: set_mixed_units)."""
        code = {"fp32": _lib.CONV_FP32, "bf16x3": _lib.CONV_BF16X3, "fp16x2": _lib.CONV_FP16X2, "mixed": _lib.CONV_MIXED}[mode]
        self._check(self.lib.d2t_set_conv_precision(self.ctx, code), "set_conv_precision")

    def set_mixed_units(self, units):
        """'mixed' precision: how many of the backbone's eight plain 512 -> 512 units run the two-MFMA fp16 arithmetic (0 .. 8)."""
        self._check(self.lib.d2t_set_mixed_units(self.ctx, int(units)), "set_mixed_units")

    def set_reserved_blocks(self, blocks):
        self._check(self.lib.d2t_set_reserved_blocks(self.ctx, int(blocks)), "set_reserved_blocks")

    def set_reserved_cus(self, cus):
        self._check(self.lib.d2t_set_reserved_cus(self.ctx, int(cus)), "set_reserved_cus")

    def set_conv_kernel(self, kind):
        """'pipelined16' (256x128 tile, one block per CU, three LDS stages, 16x16x32 MFMAs; default) or 'classic' (128x128 on
        32x32x16 MFMAs, two blocks per CU)."""
        if kind not in ("classic", "pipelined16"):
            raise ValueError(f"conv kernel must be 'pipelined16' or 'classic', not {kind!r}")
        self._check(self.lib.d2t_set_conv_kernel(self.ctx, {"classic": 0, "pipelined16": 3}[kind]), "set_conv_kernel")

    def set_beam_shared_tile(self, on):
        """Beam search: one cross-attention block per sample serving all its hypotheses from one staged memory tile (beam <= 6)."""
        self._check(self.lib.d2t_set_beam_shared_tile(self.ctx, int(bool(on))), "set_beam_shared_tile")

    def set_conv_fusion(self, pools=True, shortcuts=True):
        """Validation switches: run the 2x2 max-pools / the BasicBlocks' 1x1 shortcuts as their own kernels (False) instead of
        inside the neighbouring convolution's launch (True, default)."""
        self._check(self.lib.d2t_set_conv_fusion(self.ctx, int(bool(pools)), int(bool(shortcuts))), "set_conv_fusion")

    def set_decode_chains(self, chains):
        self._check(self.lib.d2t_set_decode_chains(self.ctx, int(chains)), "set_decode_chains")

    # ---- kernel timing -------------------------------------------------------
    def profile(self, on):
        self._check(self.lib.d2t_profile_enable(self.ctx, int(bool(on))), "profile_enable")

    def profile_read(self, max_records=4096):
        """[(M, N, K, ms)] for every MFMA implicit-GEMM launch since the last read."""
        n = C.c_int32(0)
        M, N, K = [(C.c_int32 * max_records)() for _ in range(3)]
        ms = (C.c_float * max_records)()
        self._check(self.lib.d2t_profile_read(self.ctx, max_records, C.byref(n), M, N, K, ms), "profile_read")
        return [(M[i], N[i], K[i], ms[i]) for i in range(n.value)]

    # ---- decoder -----------------------------------------------------------
    def _greedy_outputs(self, memory, S, alloc):
        """(tokens [B, S] int64, logits / probs [B, S, V] fp32) of a greedy decode beside its memory.  alloc: torch.zeros for
        the synchronous calls (what lies behind an is_test exit is read as zeros), torch.empty for the submitted ones."""
        B = memory.shape[0]
        return (alloc((B, S), dtype=torch.int64, device=memory.device),
                alloc((B, S, self.cfg.vocab), dtype=torch.float32, device=memory.device))

    def decode_greedy(self, memory, start_tokens, is_test):
        self._on_device(memory, "memory")
        memory = memory.float().contiguous()
        B, T, _ = memory.shape
        start = start_tokens.to(device=memory.device, dtype=torch.int64).contiguous()
        tokens, logits = self._greedy_outputs(memory, self.cfg.max_seq_len + 1, torch.zeros)
        steps = C.c_int32(0)
        self._check(self.lib.d2t_decode_greedy(self.ctx, _lib.ptr(memory), B, T, _lib.ptr(start), int(bool(is_test)),
                                               _lib.ptr(tokens), _lib.ptr(logits), C.byref(steps),
                                               _lib.stream_of(memory)), "decode_greedy")
        s = steps.value
        return tokens[:, :s], logits[:, :s]

    def cross_attention_layers(self, layers=None):
        """The decoder layers a map request names, ascending and without repeats: None = all, negative indices from the end."""
        n = self.cfg.dec_layers
        if layers is None:
            return list(range(n))
        out = set()
        for l in layers:
            l = int(l)
            if not -n <= l < n:
                raise ValueError(f"doc2tex_amd: decoder layer {l} of a cross-attention map request; the decoder has {n} layers")
            out.add(l % n)
        if not out:
            raise ValueError("doc2tex_amd: a cross-attention map request names no layer")
        return sorted(out)

    def cross_attention_bytes(self, B, S, T, n_layers, per_head):
        """Bytes of the maps decode_cross_attention returns for B rows of S steps over T memory tokens."""
        return int(B) * int(n_layers) * (self.cfg.dec_heads if per_head else 1) * int(S) * int(T) * 4

    def decode_cross_attention(self, memory, tokens_in, layers=None, per_head=False):
        """Cross-attention maps of the TFM decoder over tokens that are already known (d2t_decode_cross_attention): a
        teacher-forced replay of the step loop.  memory [B, T, d]; tokens_in [B, S] int64, column 0 the start token, column t
        the token fed at step t.  Returns fp32 [B, nl, S, T] (the mean over the heads) or, per_head, [B, nl, H, S, T]: row t is
        the attention of the query that produced token t + 1; nl counts `layers` (None: all; negative indices allowed), kept
        in ascending order.  Maps beyond _lib.ATTN_MAP_BUDGET bytes raise ValueError before any device work."""
        if self.cfg.decoder != _lib.DEC_TFM:
            raise RuntimeError("doc2tex_amd: decode_cross_attention needs the TFM head (the LSTM-attention heads return their "
                               "maps from the decode itself: return_alpha)")
        chosen = self.cross_attention_layers(layers)
        if memory.dim() != 3 or tokens_in.dim() != 2 or tokens_in.shape[0] != memory.shape[0]:
            raise ValueError(f"doc2tex_amd: memory {tuple(memory.shape)} / tokens_in {tuple(tokens_in.shape)}: expected [B, T, d] and [B, S]")
        B, T, _ = memory.shape
        S = tokens_in.shape[1]
        if not 1 <= S <= self.cfg.max_seq_len + 1:
            raise ValueError(f"doc2tex_amd: {S} replay steps; the decoder runs 1 .. max_seq_len + 1 = {self.cfg.max_seq_len + 1}")
        need = self.cross_attention_bytes(B, S, T, len(chosen), per_head)
        if need > _lib.ATTN_MAP_BUDGET:
            raise ValueError(f"doc2tex_amd: cross-attention maps of {need} bytes ({B} rows x {len(chosen)} layers x "
                             f"{self.cfg.dec_heads if per_head else 1} x {S} steps x {T} tokens) exceed the "
                             f"{_lib.ATTN_MAP_BUDGET}-byte budget: split the batch")
        self._on_device(memory, "memory")
        memory = memory.float().contiguous()
        tokens_in = tokens_in.to(device=memory.device, dtype=torch.int64).contiguous()
        shape = (B, len(chosen)) + ((self.cfg.dec_heads,) if per_head else ()) + (S, T)
        maps = torch.empty(shape, dtype=torch.float32, device=memory.device)
        mask = sum(1 << l for l in chosen)
        self._check(self.lib.d2t_decode_cross_attention(self.ctx, _lib.ptr(memory), B, T, _lib.ptr(tokens_in), S, mask,
                                                        int(bool(per_head)), _lib.ptr(maps), _lib.stream_of(memory)),
                    "decode_cross_attention")
        return maps

    def attn_keys(self, T):
        """Keys the LSTM-attention decoder attends over in a memory of T tokens (AttentionV2 + TFM drops the cls row)."""
        return T - (1 if self.cfg.attn_keys == _lib.ATTN_KEYS_NOCLS_INIT_CLS else 0)

    def decode_attn_greedy(self, memory, is_test, return_alpha=False):
        """Attention/AttentionV2.forward_greedy in eval mode: full-size (preds_index [B,S], probs [B,S,V]); with
        return_alpha also the alignment of every step, [B,S,Tk] (zeros after an is_test early exit)."""
        memory = memory.float().contiguous()
        B, T, _ = memory.shape
        S = self.cfg.batch_max_length + 1
        tokens, probs = self._greedy_outputs(memory, S, torch.zeros)
        steps = C.c_int32(0)
        if not return_alpha:
            self._check(self.lib.d2t_decode_attn_greedy(self.ctx, _lib.ptr(memory), B, T, int(bool(is_test)),
                                                        _lib.ptr(tokens), _lib.ptr(probs), C.byref(steps),
                                                        _lib.stream_of(memory)), "decode_attn_greedy")
            return tokens, probs
        alpha = torch.empty((B, S, self.attn_keys(T)), dtype=torch.float32, device=memory.device)
        self._check(self.lib.d2t_decode_attn_greedy_alpha(self.ctx, _lib.ptr(memory), B, T, int(bool(is_test)),
                                                          _lib.ptr(tokens), _lib.ptr(probs), _lib.ptr(alpha), C.byref(steps),
                                                          _lib.stream_of(memory)), "decode_attn_greedy_alpha")
        return tokens, probs, alpha

    def decode_attn_greedy_async(self, memory, is_test, return_alpha=False):
        """decode_attn_greedy without the wait (d2t_decode_attn_greedy_submit): returns (tokens [B,S], probs [B,S,V]
        [, alpha [B,S,Tk]], ticket).  The tensors are fresh allocations that one of the engine's decode streams is still
        writing; they are complete -- zeros after an is_test early exit included -- once `ticket` is (wait_ticket /
        decode_wait / ticket_done), and decode_steps(ticket) is then [the reference's step count].  `memory` and the
        outputs stay referenced here until the ticket completes."""
        self._on_device(memory, "memory")
        memory = memory.float().contiguous()
        B, T, _ = memory.shape
        S = self.cfg.batch_max_length + 1
        tokens, probs = self._greedy_outputs(memory, S, torch.empty)
        alpha = torch.empty((B, S, self.attn_keys(T)), dtype=torch.float32, device=memory.device) if return_alpha else None
        t = C.c_int64(0)
        self._check(self.lib.d2t_decode_attn_greedy_submit(self.ctx, _lib.ptr(memory), B, T, int(bool(is_test)),
                                                           _lib.ptr(tokens), _lib.ptr(probs),
                                                           None if alpha is None else _lib.ptr(alpha),
                                                           _lib.stream_of(memory), C.byref(t)), "decode_attn_greedy_submit")
        ticket = self._hold(int(t.value), memory, (memory, tokens, probs, alpha))
        return (tokens, probs, ticket) if alpha is None else (tokens, probs, alpha, ticket)

    def decode_attn_greedy_ragged_into(self, packed, layout, tokens, probs, is_test=False):
        """d2t_decode_attn_greedy_submit_ragged on caller-held buffers: packed [sum rows_i * T_i, 256] holds the batches'
        memories back to back, layout = [(rows_i, T_i)], tokens [B, S], probs [B, S, V] with B = sum rows_i, rows in batch
        order.  One launch decodes all rows; every row equals its own batch's decode_attn_greedy_async bit for bit.  Returns
        the ticket; decode_steps(ticket) has one entry per batch with is_test (one entry, S, without)."""
        self._on_device(packed, "memory")
        n = len(layout)
        tab = ragged_tables(layout) if n else {"rows": 0, "mem_rows": 0}
        d, S, V, B = self.cfg.attn_hidden, self.cfg.batch_max_length + 1, self.cfg.vocab, tab["rows"]
        if tuple(packed.shape) != (tab["mem_rows"], d) or not packed.is_contiguous() or packed.dtype != torch.float32:
            raise ValueError(f"packed memory must be a contiguous float32 [{tab['mem_rows']}, {d}] tensor, got "
                             f"{packed.dtype} {tuple(packed.shape)}")
        for what, t, shape, dtype in (("tokens", tokens, (B, S), torch.int64), ("probs", probs, (B, S, V), torch.float32)):
            self._on_device(t, what)
            if tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous():
                raise ValueError(f"{what} must be a contiguous {dtype} tensor of shape {shape}, got {t.dtype} {tuple(t.shape)}")
        rows = (C.c_int32 * max(n, 1))(*[int(r) for r, _ in layout])
        Ts = (C.c_int32 * max(n, 1))(*[int(t) for _, t in layout])
        t = C.c_int64(0)
        self._check(self.lib.d2t_decode_attn_greedy_submit_ragged(self.ctx, _lib.ptr(packed), n, rows, Ts, int(bool(is_test)),
                                                                  _lib.ptr(tokens), _lib.ptr(probs), _lib.stream_of(packed),
                                                                  C.byref(t)), "decode_attn_greedy_submit_ragged")
        return self._hold(int(t.value), packed, (packed, tokens, probs))

    def supports_ragged_attn_greedy(self):
        """Whether this context decodes greedy groups of the LSTM-attention heads (d2t_decode_attn_supports_ragged_greedy);
        the context itself answers, once the weights are finalized."""
        return bool(self.lib.d2t_decode_attn_supports_ragged_greedy(self.ctx))

    def decode_greedy_async(self, memory, start_tokens, is_test=False):
        """Pipelined greedy decode (max_seq_len+1 steps; with is_test the device stops early): returns (tokens, logits, ticket).  The tensors are fresh
        allocations written by the engine's decode stream; they are valid once `ticket` is complete (wait_ticket /
        decode_wait) and are never recycled behind the caller's back -- the engine keeps them alive until then."""
        self._on_device(memory, "memory")
        memory = memory.float().contiguous()
        start = start_tokens.to(device=memory.device, dtype=torch.int64).contiguous()
        tokens, logits = self._greedy_outputs(memory, self.cfg.max_seq_len + 1, torch.empty)
        ticket = self.decode_greedy_async_into(memory, start, tokens, logits, is_test=is_test)
        return tokens, logits, ticket

    def decode_greedy_async_into(self, memory, start, tokens, logits, is_test=False, rows_per_batch=0):
        """d2t_decode_greedy_submit on caller-held buffers; returns the decode's ticket.  The buffers are referenced here
        until the ticket completes, so dropping them early cannot hand their memory to another allocation mid-write.
        rows_per_batch: the rows are several encoder batches of that size (a decode group)."""
        B, T, _ = memory.shape
        t = C.c_int64(0)
        self._check(self.lib.d2t_decode_greedy_submit(self.ctx, _lib.ptr(memory), B, T, _lib.ptr(start), int(bool(is_test)),
                                                      int(rows_per_batch), _lib.ptr(tokens), _lib.ptr(logits),
                                                      _lib.stream_of(memory), C.byref(t)), "decode_greedy_submit")
        return self._hold(int(t.value), memory, (memory, start, tokens, logits))

    def decode_greedy_ragged_into(self, memory, layout, start, tokens, logits, is_test=False):
        """d2t_decode_greedy_submit_ragged on caller-held buffers: memory [sum rows_i * T_i, d] holds the batches' memories
        back to back, layout = [(rows_i, T_i)], start [B], tokens [B, S], logits [B, S, V] with B = sum rows_i.  Returns the
        ticket; decode_steps(ticket) has one entry per batch."""
        self._on_device(memory, "memory")
        n = len(layout)
        tab = ragged_tables(layout) if n else {"rows": 0, "mem_rows": 0}
        d, S, V, B = self.cfg.dec_dim, self.cfg.max_seq_len + 1, self.cfg.vocab, tab["rows"]
        if tuple(memory.shape) != (tab["mem_rows"], d) or not memory.is_contiguous() or memory.dtype != torch.float32:
            raise ValueError(f"packed memory must be a contiguous float32 [{tab['mem_rows']}, {d}] tensor, got "
                             f"{memory.dtype} {tuple(memory.shape)}")
        for what, t, shape, dtype in (("start", start, (B,), torch.int64), ("tokens", tokens, (B, S), torch.int64),
                                      ("logits", logits, (B, S, V), torch.float32)):
            self._on_device(t, what)
            if tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous():
                raise ValueError(f"{what} must be a contiguous {dtype} tensor of shape {shape}, got {t.dtype} {tuple(t.shape)}")
        rows = (C.c_int32 * max(n, 1))(*[int(r) for r, _ in layout])
        Ts = (C.c_int32 * max(n, 1))(*[int(t) for _, t in layout])
        t = C.c_int64(0)
        self._check(self.lib.d2t_decode_greedy_submit_ragged(self.ctx, _lib.ptr(memory), n, rows, Ts, _lib.ptr(start),
                                                             int(bool(is_test)), _lib.ptr(tokens), _lib.ptr(logits),
                                                             _lib.stream_of(memory), C.byref(t)), "decode_greedy_submit_ragged")
        return self._hold(int(t.value), memory, (memory, start, tokens, logits))

    def supports_ragged_groups(self):
        """Whether this context decodes ragged groups (TFM head on the absorbed cross-attention: d_model 256, 8 heads); the
        context itself answers (d2t_decode_supports_ragged), once the weights are finalized."""
        return bool(self.lib.d2t_decode_supports_ragged(self.ctx))

    def graph_count(self):
        return int(self.lib.d2t_decode_graph_count(self.ctx))

    def _hold(self, ticket, memory, tensors):
        """Keep the buffers of the asynchronous decode `ticket` referenced until it completes; returns the ticket."""
        self._wait_dev = memory.device
        held = self._held
        held.append((ticket, tensors))
        while held and self.ticket_done(held[0][0]):  # tickets complete in order per chain; at most a few stay pending
            self.decode_steps(held.pop(0)[0])  # keep its step counts past the C side's 64-entry ring
        if len(held) > 48:  # the C side keeps 64 ticket events: never let a live ticket fall out of its ring
            self.wait_ticket(held[0][0], host_sync=True)
        return ticket

    def decode_steps(self, ticket):
        """Per-batch step counts of an asynchronous decode (waits for it): [steps of batch 0, batch 1, ...]; ONE entry
        (max_seq_len + 1) for a decode without early exit.  Remembered on this side, so a handle consumed more than 64
        decodes later still learns its length."""
        cache = self._steps_cache
        ticket = int(ticket)
        if ticket not in cache:
            out = (C.c_int32 * 64)()
            n = C.c_int32(0)
            self._check(self.lib.d2t_decode_steps(self.ctx, ticket, out, 64, C.byref(n)), "decode_steps")
            cache[ticket] = [int(out[i]) for i in range(n.value)]
            for old in [t for t in cache if t <= ticket - 4096]:
                del cache[old]
        return cache[ticket]

    def ticket_done(self, ticket):
        r = int(self.lib.d2t_decode_query(self.ctx, int(ticket)))
        if r < 0:
            self._check(-r, "decode_query")
        return r == 1

    def wait_ticket(self, ticket, host_sync=False):
        """Order the current stream (and the host, if asked) after the decode with this ticket -- and only that one."""
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        self._check(self.lib.d2t_decode_wait_ticket(self.ctx, int(ticket), stream, int(bool(host_sync))), "decode_wait_ticket")

    def decode_wait(self, host_sync=False):
        if self._wait_dev is None:
            return
        stream = C.c_void_p(torch.cuda.current_stream(self._wait_dev).cuda_stream)
        self._check(self.lib.d2t_decode_wait(self.ctx, stream, int(bool(host_sync))), "decode_wait")
        if host_sync:
            for t, _ in self._held:
                self.decode_steps(t)
            self._held = []

    def decode_attn_beam(self, memory, beam_size):
        """Attention.forward_beam / AttentionV2.forward_beam for one sample: (LongTensor [1, n] on the CPU, score)."""
        memory = memory.float().contiguous()
        assert memory.shape[0] == 1  # seq2seq.py:90
        S = self.cfg.batch_max_length + 1
        seq, n, score = beam_arrays(1, S)
        self._check(self.lib.d2t_decode_attn_beam(self.ctx, _lib.ptr(memory), memory.shape[1], int(beam_size), seq,
                                                  n, score, _lib.stream_of(memory)), "decode_attn_beam")
        return beam_results(seq, n, score, 1, S, True)[0]

    def decode_attn_beam_batch(self, memory, beam_size, return_alpha=False):
        """LSTM-attention beam search for every sample of memory [N,T,256] in one step loop.  return_alpha: each entry
        also carries the returned hypothesis's alignment map [len, Tk] (the reference's seqs_alpha[best][1:]), on the
        memory's device; the call is refused when the step history exceeds _lib.ATTN_MAP_BUDGET bytes."""
        memory = memory.float().contiguous()
        N, T, S = memory.shape[0], memory.shape[1], self.cfg.batch_max_length + 1
        seq, n, score = beam_arrays(N, S)
        if not return_alpha:
            self._check(self.lib.d2t_decode_attn_beam_batch(self.ctx, _lib.ptr(memory), N, T, int(beam_size), seq,
                                                            n, score, _lib.stream_of(memory)), "decode_attn_beam_batch")
            return beam_results(seq, n, score, N, S, True)
        alpha = torch.empty((N, S, self.attn_keys(T)), dtype=torch.float32, device=memory.device)
        self._check(self.lib.d2t_decode_attn_beam_batch_alpha(self.ctx, _lib.ptr(memory), N, T, int(beam_size), seq, n, score,
                                                              _lib.ptr(alpha), _lib.stream_of(memory)),
                    "decode_attn_beam_batch_alpha")
        return beam_results(seq, n, score, N, S, True, alpha, [alpha.shape[2]] * N)

    def decode_attn_beam_batch_ragged(self, packed, lengths, beam_size, return_alpha=False):
        """decode_attn_beam_batch for samples whose memories have different lengths: packed [sum lengths, 256] holds sample
        i's lengths[i] rows behind sample i-1's (pack_memories).  One shared step loop, so its batch_max_length + 1 host round
        trips are paid once: [(LongTensor [1,len], score)] per sample, each equal to decode_attn_beam_batch on that sample
        alone.  return_alpha: each entry also carries its alignment map cut to [len, Tk_i]; the call is refused when the
        step history (at the longest sample's stride) exceeds _lib.ATTN_MAP_BUDGET bytes."""
        packed, lengths, Ts = packed_rows(packed, lengths)
        N, S = len(lengths), self.cfg.batch_max_length + 1
        seq, n, score = beam_arrays(N, S)
        ld = self.attn_keys(max(lengths)) if lengths else 0
        alpha = torch.empty((N, S, max(ld, 1)), dtype=torch.float32, device=packed.device) if return_alpha else None
        self._check(self.lib.d2t_decode_attn_beam_batch_ragged(self.ctx, _lib.ptr(packed), N, Ts, int(beam_size), seq, n, score,
                                                               _lib.ptr(alpha), _lib.stream_of(packed)),
                    "decode_attn_beam_batch_ragged")
        return beam_results(seq, n, score, N, S, True, alpha, [self.attn_keys(T) for T in lengths])

    def supports_ragged_attn_beam(self):
        """Whether decode_attn_beam_batch_ragged serves this context (an LSTM-attention head with the coverage or the
        Bahdanau cell); the context itself answers, once the weights are finalized."""
        return bool(self.lib.d2t_decode_attn_supports_ragged_beam(self.ctx))

    def supports_device_attn_beam(self):
        """Whether this context has the device-side LSTM-attention beam search (set_attn_beam_device,
        decode_attn_beam_batch_async): an LSTM-attention head with the coverage or the Bahdanau cell."""
        return bool(self.lib.d2t_decode_attn_supports_device_beam(self.ctx))

    def set_attn_beam_device(self, on):
        """on: decode_attn_beam / _batch / _batch_ragged keep the hypothesis bookkeeping on the device (one captured graph
        per search, no host round trip per step) and return the same results; off (default): the host loop."""
        self._check(self.lib.d2t_set_attn_beam_device(self.ctx, int(bool(on))), "set_attn_beam_device")

    def attn_beam_device_runs(self):
        """Searches this context has run on the device-side loop."""
        return int(self.lib.d2t_decode_attn_beam_device_runs(self.ctx))

    def decode_attn_beam_batch_async(self, packed, lengths, beam_size, return_alpha=False):
        """decode_attn_beam_batch_ragged without the wait (d2t_decode_attn_beam_batch_submit): returns
        (seq [N,S] int64, len [N] int32, score [N] float32[, alpha [N,S,max Tk]], ticket), tensors on the memory's device that
        one of the engine's decode streams is still writing.  They are complete once `ticket` is (wait_ticket / ticket_done);
        decode_steps(ticket) is then [the steps the search executed].  Sample i's result is seq[i, :len[i]], score[i] and
        alpha[i, :len[i], :attn_keys(lengths[i])].  `packed` and the outputs stay referenced here until the ticket
        completes."""
        self._on_device(packed, "memory")
        packed, lengths, Ts = packed_rows(packed, lengths)
        N, S = len(lengths), self.cfg.batch_max_length + 1
        dev = packed.device
        seq = torch.empty((max(N, 1), S), dtype=torch.int64, device=dev)
        n = torch.empty((max(N, 1),), dtype=torch.int32, device=dev)
        score = torch.empty((max(N, 1),), dtype=torch.float32, device=dev)
        ld = self.attn_keys(max(lengths)) if lengths else 0
        alpha = torch.empty((max(N, 1), S, max(ld, 1)), dtype=torch.float32, device=dev) if return_alpha else None
        t = C.c_int64(0)
        self._check(self.lib.d2t_decode_attn_beam_batch_submit(self.ctx, _lib.ptr(packed), N, Ts, int(beam_size), _lib.ptr(seq),
                                                               _lib.ptr(n), _lib.ptr(score), _lib.ptr(alpha),
                                                               _lib.stream_of(packed), C.byref(t)),
                    "decode_attn_beam_batch_submit")
        ticket = self._hold(int(t.value), packed, (packed, seq, n, score, alpha))
        return (seq, n, score, ticket) if alpha is None else (seq, n, score, alpha, ticket)

    def attn_map_bytes(self, T, beam_size):
        """Bytes of alignment history one sample adds to a beam search with maps (d2t_decode_attn_beam_batch_alpha)."""
        return (self.cfg.batch_max_length + 1) * int(beam_size) * self.attn_keys(T) * 4

    def decode_beam_batch(self, memory, beam_size):
        """Beam search for every sample of memory [N,T,d] in one shared step loop: [(LongTensor [1,len], score)] * N,
        each equal to decode_beam on that sample alone."""
        memory = memory.float().contiguous()
        N, S = memory.shape[0], self.cfg.max_seq_len + 1
        seq, n, score = beam_arrays(N, S)
        self._check(self.lib.d2t_decode_beam_batch(self.ctx, _lib.ptr(memory), N, memory.shape[1], int(beam_size), seq, n,
                                                   score, _lib.stream_of(memory)), "decode_beam_batch")
        return beam_results(seq, n, score, N, S, False)

    def decode_beam_batch_ragged(self, packed, lengths, beam_size):
        """decode_beam_batch for samples whose memories have different lengths: packed [sum lengths, d] holds sample i's
        lengths[i] rows behind sample i-1's.  One shared step loop (one captured graph per sample count and beam width,
        whatever the lengths): [(LongTensor [1,len], score)] per sample, each equal to decode_beam on that sample alone."""
        packed, lengths, Ts = packed_rows(packed, lengths)
        N, S = len(lengths), self.cfg.max_seq_len + 1
        seq, n, score = beam_arrays(N, S)
        self._check(self.lib.d2t_decode_beam_batch_ragged(self.ctx, _lib.ptr(packed), N, Ts, int(beam_size), seq, n, score,
                                                          _lib.stream_of(packed)), "decode_beam_batch_ragged")
        return beam_results(seq, n, score, N, S, False)

    def supports_ragged_beam(self):
        """Whether decode_beam_batch_ragged serves this context (the device-side beam loop: TFM head, d_model 256 on the
        absorbed cross-attention, no beam_shared_tile); the context itself answers, once the weights are finalized."""
        return bool(self.lib.d2t_decode_supports_ragged_beam(self.ctx))

    def decode_beam(self, memory, beam_size):
        memory = memory.float().contiguous()
        if memory.shape[0] != 1:
            raise AssertionError(
                f"beam search should only have signle source, encounter with batch size: {memory.shape[0]}")
        S = self.cfg.max_seq_len + 1
        seq, n, score = beam_arrays(1, S)
        self._check(self.lib.d2t_decode_beam(self.ctx, _lib.ptr(memory), memory.shape[1], int(beam_size), seq, n, score,
                                             _lib.stream_of(memory)), "decode_beam")
        return beam_results(seq, n, score, 1, S, False)[0]
