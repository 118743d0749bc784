"""Drop-in `Model(opt)` for doc2tex's recognizer (reference:
doc2tex/modules/build_model.py:7-79 and doc2tex/modules/recognizers/*).

Same constructor argument (the flat config dict), same attributes
(.stages/.featextractor/.seqmodeler/.predicter), same forward signatures and
return tuples, same state_dict key names and shapes -- but every forward runs
in libd2t (hand-written gfx950 HIP kernels) through ctypes.  There is no CPU or
eager-PyTorch fallback: on a machine without the built library or without a
HIP device the forward raises.
"""
import os

import torch
import torch.nn as nn

from . import _lib
from . import params as P
from .engine import Engine, apply_settings, beam_results, pack_memories


def decoder_attn_outputs(stages, decoder_attn, output_shape, feat_pad):
    """The alignment-map entries Model.forward adds to addition_outputs (reference build_model.py:66-77): none unless
    the decoder returned a map (beam search with viz_attn) AND the encoder reports a feature grid (ViT).
    An Attn (v1) head on the ViT attends over the cls row too, and so does the TFM head (whose map is the last decoder
    layer's head-mean cross-attention, Model._tfm_maps); that row is dropped before the map is laid on the grid.
    The key names are the reference's: "feat_width" is output_shape[0], "feat_height" output_shape[1]."""
    if decoder_attn is None or output_shape is None:
        return {}
    if stages["Pred"] in ("Attn", "TFM") and stages["Seq"] == "ViT":
        decoder_attn = decoder_attn[:, 1:]
    decoder_attn = decoder_attn.reshape(-1, output_shape[0], output_shape[1])
    return {"decoder_attn": decoder_attn, "feat_width": output_shape[0], "feat_height": output_shape[1], "feat_pad": feat_pad}


class FeatExtractorBuilder(nn.Module):
    """recognizers/build_feat.py:8-63 (parameter tree; ResNet or VGG; for Seq=BiLSTM the height-mean -- or, with
    mean_height False, proj_feat over the flattened height -- runs inside the engine)."""

    def __init__(self, flow, config):
        super().__init__()
        self.config = config
        self.flow = flow
        self.feat_name = flow["Feat"]
        if self.feat_name != "None":
            self.mean_height = bool(config["FeatureExtraction"]["params"].pop("mean_height", True))  # build_feat.py:16
            if self.feat_name == "VGG":
                self.FeatureExtraction = P.VGGFeatureExtractorParams(**config["FeatureExtraction"]["params"])
            elif self.feat_name == "ResNet":
                self.FeatureExtraction = P.ResNetFeatureExtractorParams(**config["FeatureExtraction"]["params"])
            else:
                raise NotImplementedError(f"FeatureExtraction '{self.feat_name}' is not on the accelerated path")
            self.FeatureExtraction_output = config["FeatureExtraction"]["params"]["output_channel"]
            if not self.mean_height:
                # build_feat.py:37-40: created whatever Seq is; only Seq=BiLSTM reads it (:56-61), over a feature map of
                # height 3.  The engine runs it as a (3, 1) convolution over the NHWC map
                self.proj_feat = nn.Linear(self.FeatureExtraction_output * 3, self.FeatureExtraction_output)
        else:
            if flow["Seq"] != "ViT":
                raise Exception("No FeatureExtraction module specified")
            self.FeatureExtraction = nn.Identity()


class SeqModelingBuilder(nn.Module):
    """recognizers/build_seq.py:7-40 (parameter tree; ViT hybrid, BiLSTM or None)."""

    def __init__(self, flow, config, FeatureExtraction_output):
        super().__init__()
        self.config = config
        self.flow = flow
        if flow["Seq"] == "ViT":
            assert config["max_dimension"] is not None, \
                "ViT encoder require exact height or max height and max width"
            sp = config["SequenceModeling"]["params"]
            bb = sp["backbone"]
            backbone = P.ResNetFeatureExtractorParams(bb["input_channel"], bb["output_channel"], bb["gcb"])
            max_dimension = ((config["imgH"], config["max_dimension"][1]) if config["imgH"]
                             else config["max_dimension"])  # vit_encoder.py:292-294
            ps = sp["patch_size"]
            ps = (ps, ps) if isinstance(ps, int) else tuple(ps)
            if sp.get("patching_style") != "2d":
                raise NotImplementedError("patching_style '1d' (TRIGBaseEncoder) crashes in the reference: HybridEmbed1D has "
                                          "no patch_size attribute for build_seq.py:63-66 to read")
            # create_vit_modeling (vit_encoder.py:295-302): fix_embed -> ViTEncoderV3 (frozen sincos table); otherwise a
            # learned table, read through bicubic interpolation (ViTEncoder) or -- interpolate_embed False -- a prefix slice
            # (ViTEncoderV2)
            self.SequenceModeling = P.ViTEncoderParams(
                img_size=tuple(max_dimension), patch_size=ps, in_chans=sp["input_channel"], depth=sp["depth"],
                embed_dim=sp["hidden_size"], num_heads=sp["num_heads"], hybrid_backbone=backbone,
                fix_embed=bool(sp.get("fix_embed", False)))
        elif flow["Seq"] == "BiLSTM":  # build_seq.py:13-25
            hidden_size = config["SequenceModeling"]["params"]["hidden_size"]
            self.SequenceModeling = nn.Sequential(
                P.BidirectionalLSTMParams(FeatureExtraction_output, hidden_size, hidden_size),
                P.BidirectionalLSTMParams(hidden_size, hidden_size, hidden_size))
            self.SequenceModeling_output = hidden_size
        elif flow["Seq"] == "None":
            if flow["Pred"] == "TFM":
                self.image_positional_encoder = P.PositionalEncoding2DParams(FeatureExtraction_output)
            self.SequenceModeling_output = FeatureExtraction_output
        else:
            raise NotImplementedError(f"SequenceModeling '{flow['Seq']}' is not on the accelerated path")


class PredictBuilder(nn.Module):
    """recognizers/build_pred.py:9-26 (parameter tree; TFM, Attn, Attnv2)."""

    def __init__(self, flow, config, SequenceModeling_output):
        super().__init__()
        self.flow = flow
        self.config = config
        if flow["Pred"] not in ("TFM", "Attn", "Attnv2"):
            raise NotImplementedError(f"Prediction '{flow['Pred']}' is not on the accelerated path")
        config["Prediction"]["params"]["num_classes"] = config["num_class"]  # build_pred.py:16-17
        config["Prediction"]["params"]["device"] = config["device"]
        if flow["Pred"] == "TFM":
            self.Prediction = P.TransformerPredictionParams(**config["Prediction"]["params"])
        else:  # Attention and AttentionV2 share parameters (seq2seq_v2.py:11)
            self.Prediction = P.AttentionParams(**config["Prediction"]["params"])


class DecodeHandle:
    """Completion handle of a pipelined forward (addition_outputs["decode"]): the forward's tokens / logits are views the
    engine's decode stream is still writing.  `wait()` orders the current stream (optionally the host) after exactly that
    decode -- launching the group first if it is still collecting batches -- and `done()` polls without blocking.
    `result()` waits and returns (prediction, logits) as the synchronous call would: with is_test they are cut at the
    first step at which every row of THIS batch had emitted [s] (tfm.py:138-140).

    LSTM-attention heads (full_size): `result()` returns the FULL-SIZE tensors, zeros after the exit step, because that
    is what their synchronous forward -- and the reference (seq2seq.py:224-331) -- returns; `steps()` is the reference's
    step count."""

    def __init__(self, model, eng, ticket=None, index=0, tensors=None, full_size=False):
        self._model, self._eng, self.ticket = model, eng, ticket
        self._index, self._tensors = index, tensors  # position of this batch inside its decode group; full-size views
        self._steps = None
        self._full_size = full_size

    def steps(self):
        """Valid length of this batch's tokens / logits (blocks the host until its decode is complete).  Cached: the
        C side keeps the step counts of the last 64 decodes only."""
        if self._steps is None:
            self._launch()
            per_batch = self._eng.decode_steps(self.ticket)
            # a decode without early exit reports ONE entry (all max_seq_len + 1 steps) whatever the group size
            self._steps = per_batch[self._index] if len(per_batch) > 1 else per_batch[0]
        return self._steps

    def result(self):
        n = self.steps()  # blocks the host until the decode is complete
        p, l = self._tensors
        if self._full_size:
            return p, l
        return p[:, :n], l[:, :n]

    def _launch(self):
        if self.ticket is None:  # the group this forward belongs to has not been launched yet
            self._model.launch_decode_group()
        assert self.ticket is not None

    def done(self):
        if self.ticket is None:
            return False
        return self._eng.ticket_done(self.ticket)

    def wait(self, host_sync=False):
        self._launch()
        self._eng.wait_ticket(self.ticket, host_sync=host_sync)


class BeamSearchHandle:
    """Completion handle of Model.beam_search_batch_async: the search runs on one of the engine's decode streams.
    `done()` polls without blocking, `wait()` orders the current stream (optionally the host) after exactly this search,
    `steps()` is the number of steps it executed, and `result()` waits and returns what beam_search_batch returns for the
    same input: [(LongTensor [1, len], score)] per sample, with return_attn also each sample's map [len, Tk_i]."""

    def __init__(self, eng, ticket, tensors, lengths, return_attn):
        self._eng, self.ticket, self._tensors, self._lengths, self._attn = eng, ticket, tensors, lengths, return_attn
        self._result = [] if ticket is None else None  # (an empty list of inputs: nothing was submitted)

    def done(self):
        return self.ticket is None or self._eng.ticket_done(self.ticket)

    def wait(self, host_sync=False):
        if self.ticket is not None:
            self._eng.wait_ticket(self.ticket, host_sync=host_sync)

    def steps(self):
        return 0 if self.ticket is None else self._eng.decode_steps(self.ticket)[0]

    def result(self):
        if self._result is None:
            self.wait(host_sync=True)
            seq, n, score = (t.cpu() for t in self._tensors[:3])
            self._result = beam_results(seq.flatten().tolist(), n.tolist(), score.tolist(), len(self._lengths), seq.shape[1], True,
                                        self._tensors[3] if self._attn else None, [self._eng.attn_keys(T) for T in self._lengths])
        return self._result


class DecodeGroup:
    """The forwards of a pipelined head that share ONE step loop (TFM: Model.decode_group > 1; LSTM-attention heads:
    Model.attn_decode_group > 1, always the mixed layout, no start tokens): their memories lie back to back
    in one packed [memory rows, d] buffer and their outputs are views of one tokens / logits pair.  Every group writes into
    fresh tensors (no ring to overrun): the views handed out stay valid for as long as the caller keeps them, and become
    readable once the group's ticket -- shared by its handles -- is complete.  Two layouts of the same object:
      uniform (row_budget 0)  every batch has the first one's (B, T), which are part of the key; room for `batches` of them;
                              launched through decode_greedy_async_into(rows_per_batch=B);
      mixed (row_budget > 0)  batches of any (B, T) -- Model.decode_group_mixed -- up to max(row_budget, first B) rows; the
                              packed memory grows as needed; launched through decode_greedy_ragged_into with the layout
                              (attn: decode_attn_greedy_ragged_into; the handles are full-size ones)."""

    @staticmethod
    def steps_of(eng, attn=False):
        """Steps of the head's loop: the second dimension of its tokens / logits."""
        return (eng.cfg.batch_max_length if attn else eng.cfg.max_seq_len) + 1

    @staticmethod
    def key_of(eng, memory, is_test, batches, mixed, attn=False):
        """What the batches of one group have in common; a batch with another key launches what has been collected."""
        B, T, d = memory.shape
        tail = (d, DecodeGroup.steps_of(eng, attn), eng.cfg.vocab, memory.device, bool(is_test))
        return ("mixed",) + tail if mixed else (batches, B, T) + tail

    def __init__(self, model, eng, memory, is_test, batches, row_budget=0, attn=False):
        B, T, d = memory.shape
        S, V, dev = self.steps_of(eng, attn), eng.cfg.vocab, memory.device
        self._model, self._eng, self.is_test, self.attn = model, eng, bool(is_test), bool(attn)
        self.key = self.key_of(eng, memory, is_test, batches, row_budget > 0, attn)
        self.rows_per_batch = 0 if row_budget else B
        if row_budget:
            self.cap = max(row_budget, B)  # a single batch beyond the row budget is a group of its own
            # the packed memory starts at what `batches` batches like this one need and grows with longer / larger ones
            mem_rows = min(self.cap, max(1, batches) * B) * T
        else:
            self.cap, mem_rows = batches * B, batches * B * T
        self.layout, self.handles, self.rows, self.mem_rows = [], [], 0, 0  # [(B, T)] per batch; output / memory rows in use
        self.mem = torch.empty((mem_rows, d), dtype=torch.float32, device=dev)
        self.start = None if attn else torch.empty((self.cap,), dtype=torch.int64, device=dev)
        self.tokens = torch.empty((self.cap, S), dtype=torch.int64, device=dev)
        self.logits = torch.empty((self.cap, S, V), dtype=torch.float32, device=dev)

    def fits(self, key, B):
        """Whether a batch of B rows with this key joins the group; if not, the group is launched first."""
        return key == self.key and self.rows + B <= self.cap

    def full(self, batches):
        return len(self.layout) >= batches

    def add(self, memory, start=None):
        """Copy a batch in; returns (tokens view, logits view, handle) of its rows."""
        B, T, d = memory.shape
        r0, m0 = self.rows, self.mem_rows
        if m0 + B * T > self.mem.shape[0]:  # (mixed) longer memories than the first batch's: grow the packed buffer
            grown = torch.empty((max(2 * self.mem.shape[0], m0 + B * T), d), dtype=torch.float32, device=memory.device)
            grown[:m0].copy_(self.mem[:m0])
            self.mem = grown
        self.mem[m0:m0 + B * T].copy_(memory.reshape(B * T, d))
        if self.start is not None:
            self.start[r0:r0 + B].copy_(start.to(device=memory.device, dtype=torch.int64))
        views = self.tokens[r0:r0 + B], self.logits[r0:r0 + B]
        handle = DecodeHandle(self._model, self._eng, None, len(self.layout), views, full_size=self.attn)
        self.handles.append(handle)
        self.layout.append((B, T))
        self.rows, self.mem_rows = r0 + B, m0 + B * T
        return views + (handle,)

    def launch(self, eng):
        """Submit the collected rows as one decode; its ticket goes to every handle."""
        r, m = self.rows, self.mem_rows
        if self.attn:
            ticket = eng.decode_attn_greedy_ragged_into(self.mem[:m], self.layout, self.tokens[:r], self.logits[:r],
                                                        is_test=self.is_test)
        elif self.rows_per_batch:
            ticket = eng.decode_greedy_async_into(self.mem[:m].view(r, self.layout[0][1], -1), self.start[:r], self.tokens[:r],
                                                  self.logits[:r], is_test=self.is_test, rows_per_batch=self.rows_per_batch)
        else:
            ticket = eng.decode_greedy_ragged_into(self.mem[:m], self.layout, self.start[:r], self.tokens[:r], self.logits[:r],
                                                   is_test=self.is_test)
        for h in self.handles:
            h.ticket = ticket


class Model(nn.Module):
    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        stages = {
            "Feat": opt["FeatureExtraction"]["name"],
            "Seq": opt["SequenceModeling"]["name"],
            "Pred": opt["Prediction"]["name"],
        }
        self.stages = stages
        if stages["Seq"].__contains__("Vi"):
            assert stages["Feat"] == "None"
        self.featextractor = FeatExtractorBuilder(stages, opt)
        self.seqmodeler = SeqModelingBuilder(stages, opt, getattr(self.featextractor, "FeatureExtraction_output", None))
        self.predicter = PredictBuilder(stages, opt, getattr(self.seqmodeler, "SequenceModeling_output", None))
        self._engine = None
        # Opt-in software pipelining across consecutive forward() calls (eval, greedy, is_test=False):
        # forward returns while the latency-bound decode loop still runs on the engine's stream, so the
        # next batch's encoder overlaps it.  Results are valid after synchronize().
        self.pipelined = False
        # pipelined mode: block slots the persistent convolution leaves free for the decode stream
        self.reserved_blocks = 64
        # split-bf16 convolution kernel: 'pipelined16' (256x128 tile, one block per CU, three LDS stages, 16x16x32 MFMAs;
        # default) or 'classic' (128x128 on 32x32x16 MFMAs, two blocks per CU)
        self.conv_kernel = "pipelined16"
        # pipelined serving: compute units the pipelined kernel's grid leaves to the decode streams
        self.reserved_cus = 0
        # validation switches (tests): the 2x2 max-pools / 1x1 shortcuts inside the neighbouring convolution's launch (default)
        self.conv_fusion = (True, True)
        # beam search (TFM, d_model 256, beam <= 6): one cross-attention block per sample for all its hypotheses (default: per row)
        self.beam_shared_tile = False
        # beam search of the LSTM-attention heads (coverage / Bahdanau cells): keep the hypothesis bookkeeping on the device --
        # one captured graph per search instead of a host round trip per step, same results.  Off by
        # default; heads without that search ignore it.  beam_search_batch_async always runs the device-side search.
        self.attn_beam_device = False
        # pipelined mode: decode loops in flight side by side (1 .. 4)
        self.decode_chains = 1
        # (LSTM-attention heads: each of the chains holds one forward's whole loop, key projection and state block)
        # pipelined mode, TFM head: decode the rows of this many consecutive forward() calls in ONE step loop.  Ignored by the
        # LSTM-attention heads, whose loop already is one launch with one block per row and whose early exit is decided over
        # the forward's own batch (their groups have a switch of their own, attn_decode_group below).  The decode step is a
        # chain of small latency-bound kernels whose duration barely depends on the row count, so two batches per loop halve
        # the launches (and the interference with the next encoders) per formula.  Rows are independent and every kernel is
        # dispatched by layer shape only, so each row's tokens / logits are bit-identical to an ungrouped decode.  Results
        # of a group become valid after synchronize() (which also launches a group that is still incomplete).
        self.decode_group = 1
        # decode groups over crops of DIFFERENT sizes (opt-in; TFM head with d_model 256, the absorbed cross-attention): a
        # group then takes consecutive forward() calls of any (rows, memory length) -- every row reads its own slice of one
        # packed memory buffer and stays bit-identical to its single-batch decode -- and is launched when it holds
        # `decode_group` batches or the next batch would exceed `decode_group_rows` rows (the row count up to which the step
        # loop's duration stays flat).  Off: a change of the row count or memory length launches the
        # group collected so far, as before.  Other decoders (d_model 512) keep that behaviour whatever the switch says.
        self.decode_group_mixed = False
        self.decode_group_rows = 384
        # pipelined mode, LSTM-attention heads (opt-in): decode the rows of up to this many consecutive greedy forward() calls
        # -- crops of any size -- in ONE launch of the step loop.  That loop has one 1024-thread block per row, so a bucket of
        # 8 crops keeps 8 compute units busy for all of its steps; the rows of several batches fill the chip with the same
        # blocks, each bit-identical to its own batch's decode, and each batch keeps its own is_test exit step (DESIGN.md
        # section 5.4e).  A group is launched when it holds `attn_decode_group` batches (at most 64), when the next batch
        # would exceed `attn_decode_group_rows` rows (one block per compute unit on a 256-CU part; at most 1024), when is_test
        # changes, on synchronize() and on a handle's wait().  A forward with viz_attn on launches what has been collected
        # and runs alone.  1: one launch per forward, as before.  Beam search and synchronous forwards are untouched.
        self.attn_decode_group = 1
        self.attn_decode_group_rows = 256
        self._group = None  # the DecodeGroup that is still collecting forwards
        # Arithmetic of the backbone / large GEMMs:
        #   'bf16x3'  (default) split-bf16: 3 bf16 MFMAs per product, fp32 accumulate; max |dlogit| ~5e-5 against the 1e-3 bar
        #             on every fixture and on fresh seeds (tools/probe/fp16x2_margin.py);
        #   'fp16x2'  (opt-in, +21 % formulas/s behind a ViT encoder) fp16 feature-map records x fp16 hi / lo weights in the
        #             backbone: 2 MFMAs per product.  Tokens exact and logits within 1e-3 on every HybridViT / LSTM-head fixture
        #             (C2: ~2e-4, C4: ~1.5e-4), but the margin is 5x, not 20x: the tiny test stack T2 reaches 5e-4 .. 1.05e-3 on
        #             fresh seeds, a near-tie between two tokens flips ~5x as often, and Feat=ResNet + Seq=None stacks (their
        #             decoder reads the backbone's output directly) move by up to 9e-3.  Needs conv_kernel = 'pipelined16';
        #   'mixed'   (round 4, opt-in) 'bf16x3' with the two-MFMA arithmetic in the first `mixed_units` of the backbone's eight
        #             plain 512 -> 512 units only (layer3.1 .. layer3.4, conv3, layer4.0 .. layer4.2: the K = 4608 layers); the error
        #             grows with the square root of the number of such layers;
        #   'fp32'    exact fp32 matrix-core arithmetic.
        # D2T_CONV_PRECISION=auto|bf16x3|fp16x2|mixed|fp32 overrides the default; 'auto' is 'bf16x3'.
        # The reference's --amp (api/infer.py:120-124,157-161; engine/inferencing.py:68-72,149-153) wraps the model call in
        # torch.autocast: its convolutions and linears then run on fp16 operands and return fp16 (measured on the reference
        # itself, CPU autocast(float16): max |dlogit| 3e-3 on C2, 7e-3 on T2 against its own fp32 path).  A forward of an
        # eval()-mode HybridViT stack that the caller runs under torch.autocast("cuda") therefore takes `amp_conv_precision`
        # ('fp16x2': 2e-4 on C2, 17x closer to fp32 than the reference's AMP path; None: autocast changes nothing) -- outputs
        # stay fp32.  An explicit conv_precision / D2T_CONV_PRECISION always wins, and training steps keep their arithmetic.
        self.amp_conv_precision = "fp16x2"
        prec = os.environ.get("D2T_CONV_PRECISION", "auto")
        self._precision_auto = prec == "auto"
        if prec == "auto":
            prec = "bf16x3"
        self._conv_precision = prec
        self.mixed_units = 3  # conv_precision 'mixed': units on the two-MFMA arithmetic (0 .. 8; 3 keeps |dlogit| <= 1e-4 on C2 / C4 / S0)
        # data-parallel training: a doc2tex_amd.dist.GradSync makes loss.backward() return all-reduced (mean) gradients
        self.grad_sync = None

    def beam_search_batch(self, input, beam_size=None, return_attn=False):
        """Extension (the reference's beam search takes one sample per call, tfm.py:146-148): encode the whole batch
        and advance the hypotheses of all samples in one step loop.  Returns [(LongTensor [1, len], score)] per
        sample, each identical to `forward(input[i:i+1], ...)` with `beam_size` set.

        input may also be a list or tuple of image tensors of different sizes: one search over all of them
        (_beam_search_mixed), the results as one flat list in input order.

        return_attn (LSTM-attention heads): [(seq, score, decoder_attn)] per sample, decoder_attn [len, Tk] being what
        forward_decoder returns for that sample alone with viz_attn set (decoder_attn_outputs lays it on the feature grid).
        A batch whose alignment history would exceed _lib.ATTN_MAP_BUDGET bytes is searched in several parts.
        TFM head, with return_attn or Prediction.viz_attn set: the same triple, decoder_attn [len, T] being the last decoder
        layer's head-mean cross-attention of the returned hypothesis (one row per generated token, the cls row of a ViT
        memory included), from a teacher-forced replay per sample after the search (_tfm_maps)."""
        beam = int(beam_size or self.opt.get("beam_size", 1))
        if self.stages["Pred"] == "TFM" and getattr(self.predicter.Prediction, "viz_attn", False):
            return_attn = True
        if isinstance(input, (list, tuple)):
            return self._beam_search_mixed(input, beam, return_attn)  # (TFM head with maps: tensor by tensor)
        memory, _, _ = self.forward_encoder(input)
        if self.stages["Pred"] == "TFM":
            eng, memory = self.engine(), memory.contiguous()
            results = eng.decode_beam_batch(memory, beam)
            if not return_attn:
                return results
            # with return_attn, or viz_attn set on the head: every sample's hypothesis replayed on its own (their lengths
            # differ) -> (seq, score, decoder_attn [len, T]), the last layer's head-mean cross-attention
            exact = self._exact_memory(input, memory)
            eng = self.engine()  # (the model's own precision again)
            return [r + (self._tfm_maps(eng, exact[i:i + 1], None, r[0])[0][0],) for i, r in enumerate(results)]
        eng = self.engine()
        if not return_attn:
            return eng.decode_attn_beam_batch(memory.contiguous(), beam)
        per = max(1, _lib.ATTN_MAP_BUDGET // max(1, eng.attn_map_bytes(memory.shape[1], beam)))
        out = []
        for a in range(0, memory.shape[0], per):
            out += eng.decode_attn_beam_batch(memory[a:a + per].contiguous(), beam, return_alpha=True)
        return out

    def beam_search_batch_async(self, input, beam_size=None, return_attn=False):
        """beam_search_batch without the wait, for the LSTM-attention heads whose search the engine keeps on the device
        (Engine.supports_device_attn_beam): the encoders run on the current stream, the search is submitted to one of the
        engine's decode chains (decode_chains of them take turns) and the call returns a BeamSearchHandle -- so the next
        input's encoder can run beside the search.  input: a tensor, or a list / tuple of tensors of different sizes.
        handle.result() is exactly what beam_search_batch returns for the same input.

        Never falls back to a blocking search: a head without the device-side search (TFM, the 'loc_aware' cell) raises
        NotImplementedError, and a return_attn input whose alignment history exceeds _lib.ATTN_MAP_BUDGET bytes raises
        RuntimeError (submit fewer samples per call)."""
        beam = int(beam_size or self.opt.get("beam_size", 1))
        if self.stages["Pred"] == "TFM":
            raise NotImplementedError("beam_search_batch_async: the TFM head's beam search cannot be submitted; use "
                                      "beam_search_batch")
        eng = self.engine()
        if not eng.supports_device_attn_beam():
            raise NotImplementedError("beam_search_batch_async: this head has no device-side beam search (the 'loc_aware' "
                                      "cell has no beam search in the engine at all); use beam_search_batch")
        inputs = list(input) if isinstance(input, (list, tuple)) else [input]
        if len(inputs) == 0:
            return BeamSearchHandle(eng, None, (), [], return_attn)
        packed, lengths = pack_memories([self.forward_encoder(x)[0] for x in inputs])
        if return_attn:
            need = len(lengths) * eng.attn_map_bytes(max(lengths), beam)
            if need > _lib.ATTN_MAP_BUDGET:
                raise RuntimeError(f"beam_search_batch_async: the alignment history of {len(lengths)} samples ({need} bytes at "
                                   f"the longest memory's stride) exceeds the {_lib.ATTN_MAP_BUDGET}-byte budget; submit fewer "
                                   "samples per call")
        out = eng.decode_attn_beam_batch_async(packed, lengths, beam, return_alpha=return_attn)
        return BeamSearchHandle(eng, out[-1], out[:-1], lengths, return_attn)

    def _beam_search_mixed(self, inputs, beam, return_attn=False):
        """beam_search_batch for a list of image tensors [n_i, C, H_i, W_i] (crops of different sizes, e.g. the buckets of
        Preprocessor.batch): every tensor is encoded on its own, the memories are packed and ONE search advances the
        hypotheses of all samples (TFM head: Engine.decode_beam_batch_ragged; Attn / Attnv2: Engine.decode_attn_beam_batch_ragged,
        whose host-side loop then pays its batch_max_length + 1 round trips once instead of once per tensor).  Returns the flat
        list of results in input order, each identical to the single-tensor call on its tensor; with return_attn (LSTM-attention
        heads) every sample's map is cut to its own [len, Tk_i].  Where the engine has no ragged beam search (d_model 512,
        beam_shared_tile, the 'loc_aware' cell) the tensors are searched one after the other by that call -- and so is a
        return_attn list whose alignment history, at the longest memory's stride, would exceed _lib.ATTN_MAP_BUDGET bytes."""
        if len(inputs) == 0:
            return []
        eng = self.engine()
        tfm = self.stages["Pred"] == "TFM"
        if (return_attn and tfm) or not (eng.supports_ragged_beam() if tfm else eng.supports_ragged_attn_beam()):
            return self._beam_search_each(inputs, beam, return_attn)
        packed, lengths = pack_memories([self.forward_encoder(x)[0] for x in inputs])
        if tfm:
            return eng.decode_beam_batch_ragged(packed, lengths, beam)
        if return_attn:
            if len(lengths) * eng.attn_map_bytes(max(lengths), beam) > _lib.ATTN_MAP_BUDGET:
                del packed
                return self._beam_search_each(inputs, beam, return_attn)  # (which splits each tensor's batch as it needs)
        return eng.decode_attn_beam_batch_ragged(packed, lengths, beam, return_alpha=return_attn)

    def _beam_search_each(self, inputs, beam, return_attn):
        out = []
        for x in inputs:
            out += self.beam_search_batch(x, beam, return_attn)
        return out

    def _collect_decode(self, eng, memory, start, is_test=False, attn=False):
        """pipelined + decode_group > 1: collect the encoder memories of consecutive calls, launch one decode per group --
        when it holds decode_group batches, or when the next batch does not fit it (another key; decode_group_mixed: more
        rows than decode_group_rows).  attn: the LSTM-attention heads' groups (attn_decode_group / attn_decode_group_rows),
        always mixed, within the engine's 64 batches and 1024 rows per launch."""
        if attn:
            G, mixed = min(64, int(self.attn_decode_group)), True
            budget = min(1024, max(1, int(self.attn_decode_group_rows)))
        else:
            G = int(self.decode_group)
            mixed = bool(self.decode_group_mixed and eng.supports_ragged_groups())
            budget = max(1, int(self.decode_group_rows)) if mixed else 0
        if self._group is not None and not self._group.fits(DecodeGroup.key_of(eng, memory, is_test, G, mixed, attn), memory.shape[0]):
            self.launch_decode_group()
        if self._group is None:
            self._group = DecodeGroup(self, eng, memory, is_test, G, budget, attn)
        out = self._group.add(memory, start)
        if self._group.full(G):
            self.launch_decode_group()
        return out

    def launch_decode_group(self):
        """Launch the decode group that is still collecting forwards, if there is one."""
        group, self._group = self._group, None
        if group is not None:
            group.launch(self._engine)

    def drop_decode_group(self):
        """Forget the collected forwards without decoding them (their handles never complete)."""
        self._group = None

    def synchronize(self, host_sync=True, flush=True):
        """Order the current stream (and optionally the host) after every outstanding pipelined decode.  `flush` also
        launches a decode group that is still incomplete (decode_group > 1); a serving loop that only wants to order a
        consumer stream after the groups already launched passes flush=False."""
        if self._engine is not None:
            if flush:
                self.launch_decode_group()
            self._engine.decode_wait(host_sync=host_sync)

    # -- engine plumbing -----------------------------------------------------
    def engine_opt(self):
        """The config the engine is built from: self.opt, except that a `mean_height: False` FeatExtractorBuilder popped from it
        (build_feat.py:16) is put back -- into a copy of the two dicts above the key, never into the caller's."""
        if getattr(self.featextractor, "mean_height", True):
            return self.opt
        fe = self.opt["FeatureExtraction"]
        return {**self.opt, "FeatureExtraction": {**fe, "params": {**fe["params"], "mean_height": False}}}

    def engine(self, finalize=True):
        """The libd2t context of this model, with the current weights uploaded (and packed for inference)."""
        # the context lives where the parameters live (model.to("cuda:1") moves the engine with them); before the first
        # .to() the reference's own device string, opt["device"] (build_pred.py:17), decides
        p0 = next(self.parameters())
        dev = p0.device if p0.is_cuda else None
        if self._engine is not None and dev is not None and self._engine.device != dev.index:
            self.synchronize()
            self._engine, self._group = None, None  # parameters were moved to another GPU: a fresh context there
        if self._engine is None:
            self._engine = Engine(self.engine_opt(), device=dev)
        self._engine.sync_weights(self, finalize=finalize)
        # what the context should run with; engine.SETTINGS holds the order and the conditions of the set_* calls
        apply_settings(self._engine, {
            "reserved_blocks": self.reserved_blocks if self.pipelined else 0,
            "reserved_cus": self.reserved_cus if self.pipelined else 0,
            "conv_precision": self.effective_conv_precision(),
            "conv_kernel": self.conv_kernel,
            "beam_shared_tile": bool(self.beam_shared_tile),
            "attn_beam_device": bool(self.attn_beam_device),
            "conv_fusion": tuple(self.conv_fusion),
            "decode_chains": self.decode_chains,
            "mixed_units": int(self.mixed_units)}, finalize)
        return self._engine

    @property
    def conv_precision(self):
        return self._conv_precision

    @conv_precision.setter
    def conv_precision(self, mode):
        if mode not in ("fp32", "bf16x3", "fp16x2", "mixed"):
            raise ValueError(f"conv_precision must be 'fp32', 'bf16x3', 'fp16x2' or 'mixed', not {mode!r}")
        self._conv_precision = mode
        self._precision_auto = False

    def _under_amp(self):
        """True when the caller's torch.autocast("cuda") asks for reduced precision and this model may follow it."""
        if not (self._precision_auto and self.amp_conv_precision) or self.training or self.stages["Seq"] != "ViT":
            return False
        try:
            return bool(torch.is_autocast_enabled("cuda"))
        except TypeError:  # older signature: no device argument, CUDA implied
            return bool(torch.is_autocast_enabled())

    def effective_conv_precision(self):
        """The arithmetic the next forward runs in (an 'auto' fp16x2 steps back to bf16x3 for other convolution kernels;
        under the caller's torch.autocast an 'auto' model takes amp_conv_precision)."""
        if self._under_amp() and self.conv_kernel == "pipelined16":
            if self.amp_conv_precision not in ("fp16x2", "mixed", "bf16x3"):
                raise ValueError(f"amp_conv_precision must be 'fp16x2', 'mixed', 'bf16x3' or None, not {self.amp_conv_precision!r}")
            return self.amp_conv_precision
        if self._precision_auto and self._conv_precision in ("fp16x2", "mixed") and self.conv_kernel != "pipelined16":
            return "bf16x3"
        return self._conv_precision

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        if self._engine is not None:
            self._engine._sig = None  # tensors moved: re-upload on next use
        return out

    # -- reference API -------------------------------------------------------
    def _hooked_attn_drops(self):
        """The ViT blocks whose attn_drop carries a forward hook or forward pre-hook: [(block index, module)]."""
        if self.stages["Seq"] != "ViT":
            return []
        return [(i, blk.attn.attn_drop) for i, blk in enumerate(self.seqmodeler.SequenceModeling.blocks)
                if blk.attn.attn_drop._forward_hooks or blk.attn.attn_drop._forward_pre_hooks]

    def _refuse_train_attn_hooks(self):
        if self.training and self._hooked_attn_drops():
            raise NotImplementedError(
                "forward hooks on attn_drop read the ViT attention maps of the inference encoder only: the training step's "
                "attention kernels (attn_train_fwd_kernel / attn_train_bwd_kernel) do not write the probabilities.  Call "
                "model.eval() for the maps, or remove the hooks before training")

    def forward_encoder(self, input, *args, **kwargs):
        """build_model.py:36-43 -> (contextual_feature [B,T,d], output_shape, feat_pad).

        ViT encoders: when a block's attn.attn_drop has a forward hook or pre-hook (as the reference's attention rollout
        registers, tools/interpretation/vit_visualize.py:26-93), the encoder also writes that block's attention
        probabilities [B, heads, T, T] and then calls attn_drop on them in block order, so the hooks see what they see in
        the reference.  Only hooked blocks are allocated; without hooks the encoder runs exactly as before."""
        self._refuse_train_attn_hooks()
        hooked = self._hooked_attn_drops()
        eng = self.engine()
        if not hooked:
            memory, grid, pad = eng.encode(input)
        else:
            B, _, H, W = input.shape
            T = eng.encoder_shape(H, W)[0]
            maps = [None] * eng.cfg.vit_depth
            for i, _ in hooked:
                maps[i] = torch.empty((B, eng.cfg.vit_heads, T, T), dtype=torch.float32, device=input.device)
            memory, grid, pad = eng.encode(input, attn_maps=maps)
            for i, mod in hooked:
                # eval: Dropout returns its input.  A hook (or pre-hook) handing back another tensor would change the rest
                # of the reference's forward, but the engine has already used the unmodified probabilities
                if mod(maps[i]) is not maps[i]:
                    raise RuntimeError(
                        f"a hook on seqmodeler.SequenceModeling.blocks.{i}.attn.attn_drop returned a replacement tensor: the "
                        "HIP encoder computes attention in one kernel and has already used the unmodified probabilities, so "
                        "hooks on attn_drop may read the maps but not replace them")
        if self.stages["Seq"] == "ViT":
            return memory, grid, pad  # build_seq.py:59-66
        return memory, None, None  # build_seq.py:69-76

    def forward_decoder(self, contextual_feature, text, is_train=True, is_test=False, rtl_text=None, maps_memory=None):
        """build_model.py:45-53 / build_pred.py:28-50 / tfm.py:188-195.

        maps_memory (TFM head with viz_attn; an extension): the memory the cross-attention maps are replayed over, where it is
        not the one decoded -- Model.forward passes the crop's memory encoded in exact fp32 (_exact_memory).  None: the maps
        are taken over contextual_feature itself."""
        beam_size = self.opt.get("beam_size", 1)  # read on every call, build_pred.py:31
        self._luong_check()
        eng = self.engine()
        if self.stages["Pred"] in ("Attn", "Attnv2"):
            # build_pred.py:36-44 -> Attention.forward (seq2seq.py:333-347)
            if self.training or is_train:
                raise NotImplementedError(
                    "forward_decoder() is the inference entry point of the HIP engine (greedy / beam decoding of an encoder "
                    "memory): call model.eval() and pass is_train=False (engine/inferencing.py:70-76).  The teacher-forced "
                    "training pass of the LSTM-attention head runs through Model.forward() under model.train(), which keeps "
                    "the whole step on one autograd node")
            pred = self.predicter.Prediction
            viz = bool(getattr(pred, "viz_attn", False))  # read on every call, like the reference (seq2seq.py:124,267)
            if beam_size > 1:  # seq2seq.py:333-347 -> forward_beam (one sample, returns (seq, score, alphas or None))
                if not viz:
                    prediction, logits = eng.decode_attn_beam(contextual_feature.contiguous(), beam_size)
                    return prediction, logits, None, {}
                if contextual_feature.shape[0] != 1:
                    raise AssertionError("forward_beam takes one sample (seq2seq.py:90)")
                prediction, logits, alphas = eng.decode_attn_beam_batch(contextual_feature.contiguous(), beam_size,
                                                                        return_alpha=True)[0]
                return prediction, logits, alphas, {}
            if self.pipelined and int(self.attn_decode_group) > 1:
                # several forwards, one launch (attn_decode_group): the rows join a DecodeGroup; a forward with viz_attn on,
                # with more rows than one launch takes, or with a memory length the engine refuses (the refusal is then this
                # forward's alone, not its group's) sends what has been collected first and runs alone below
                memory = contextual_feature.contiguous()
                if (not viz and memory.shape[0] <= 1024 and 1 <= eng.attn_keys(memory.shape[1]) <= 4096
                        and eng.supports_ragged_attn_greedy()):
                    prediction, logits, handle = self._collect_decode(eng, memory, None, is_test, attn=True)
                    return prediction, logits, None, {"decode": handle}
                self.launch_decode_group()
            if self.pipelined:
                # the forward returns while the loop runs on one of the engine's decode streams; tensors are full size as in
                # the synchronous call and complete (zeros after an is_test exit included) once the handle is
                out = eng.decode_attn_greedy_async(contextual_feature.contiguous(), is_test, return_alpha=viz)
                prediction, logits, ticket = out[0], out[1], out[-1]
                if viz:  # set at call time, complete with the handle (seq2seq.py:267-272,300-301)
                    pred.alpha_stores = out[2].unsqueeze(-1)
                handle = DecodeHandle(self, eng, ticket, 0, (prediction, logits), full_size=True)
                return prediction, logits, None, {"decode": handle}
            if not viz:
                prediction, logits = eng.decode_attn_greedy(contextual_feature.contiguous(), is_test)
                return prediction, logits, None, {}
            # greedy: the alignments go to Prediction.alpha_stores [B, S, Tk, 1] (seq2seq.py:267-272,300-301), not to the
            # return value
            prediction, logits, alpha = eng.decode_attn_greedy(contextual_feature.contiguous(), is_test, return_alpha=True)
            pred.alpha_stores = alpha.unsqueeze(-1)
            return prediction, logits, None, {}
        if self.training:
            raise NotImplementedError(
                "forward_decoder() is the inference entry point of the HIP engine (greedy / beam decoding of an encoder "
                "memory): call model.eval() first.  The teacher-forced training pass (tfm.py:103-118) runs through "
                "Model.forward() under model.train(), encoder and decoder on one autograd node, so that loss.backward() "
                "reaches the backbone")
        # viz_attn on the TFM head (an attribute read on every call, like the LSTM heads'; absent = off): the decode itself is
        # what it always is, and a teacher-forced replay over its tokens writes the cross-attention maps afterwards (_tfm_maps)
        viz = bool(getattr(self.predicter.Prediction, "viz_attn", False))
        if beam_size > 1:
            memory = contextual_feature.contiguous()
            prediction, logits = eng.decode_beam(memory, beam_size)
            if viz:  # one row per generated token; the last layer's head mean is the decoder_attn Model.forward lays on the grid
                last, cross = self._tfm_maps(eng, memory if maps_memory is None else maps_memory, None, prediction)
                return prediction, logits, last[0], {"cross_attn": cross}
        else:
            if text.dim() != 2 or text.shape[1] != 1:
                raise ValueError("eval decoding expects text = [B,1] start tokens ([GO])")
            if viz:
                # a pipelined or grouped forward with the flag on sends what has been collected, waits for every decode in
                # flight and runs alone, synchronously (no handle): the greedy maps go to Prediction.alpha_stores [B, steps, T, 1]
                # as the LSTM heads' do (seq2seq.py:267-272), the full request to addition_outputs["cross_attn"]
                if self.pipelined:
                    self.synchronize()
                memory = contextual_feature.contiguous()
                prediction, logits = eng.decode_greedy(memory, text[:, 0], is_test)
                last, cross = self._tfm_maps(eng, memory if maps_memory is None else maps_memory, text[:, 0], prediction)
                self.predicter.Prediction.alpha_stores = last.unsqueeze(-1)
                return prediction, logits, None, {"cross_attn": cross}
            # pipelined: the forward returns while the step loop runs on an engine stream.  With is_test the early exit is
            # taken on the device; prediction / logits are then FULL-SIZE tensors whose valid length is only known once the
            # decode is complete -- addition_outputs["decode"].result() waits and returns them cut as the reference does
            if self.pipelined and int(self.decode_group) > 1:
                prediction, logits, handle = self._collect_decode(eng, contextual_feature.contiguous(), text[:, 0], is_test)
                return prediction, logits, None, {"decode": handle}
            elif self.pipelined:
                prediction, logits, ticket = eng.decode_greedy_async(contextual_feature.contiguous(), text[:, 0], is_test)
                return prediction, logits, None, {"decode": DecodeHandle(self, eng, ticket, 0, (prediction, logits))}
            else:
                prediction, logits = eng.decode_greedy(contextual_feature.contiguous(), text[:, 0], is_test)
        return prediction, logits, None, {}

    def _exact_memory(self, input, memory):
        """The encoder memory of `input` in exact fp32 arithmetic, for the map replay of the TFM head: `memory` itself when that
        is what the model runs in, else the crop encoded once more with conv_precision 'fp32' (no hooks fire; the model's own
        precision is back with the next engine() call, so the decode is what it is without the flag).  Why: attention
        probabilities amplify the memory's rounding -- on a ResNet memory read by a d_model-512 decoder the split-bf16
        backbone moves them by up to 2.9e-4, the fp32 one by 2e-5.  Pipelined: waits for the decodes
        in flight first, as the flagged forward does anyway."""
        if self.effective_conv_precision() == "fp32":
            return memory
        if self.pipelined:
            self.synchronize()
        saved = self._conv_precision, self._precision_auto
        self._conv_precision, self._precision_auto = "fp32", False
        try:
            return self.engine().encode(input)[0]
        finally:
            self._conv_precision, self._precision_auto = saved

    def _tfm_maps(self, eng, memory, start, generated):
        """Cross-attention maps of a finished TFM decode (Engine.decode_cross_attention): the step loop replayed over
        [start | generated[:, :-1]], so that row t is the attention of the query that produced generated[:, t].
        start [B] (None: [GO], as the beam search starts); generated [B, steps] on any device.
        Returns (last [B, steps, T], cross): `last` the last decoder layer's mean over the heads; `cross` what the head asks
        for -- Prediction.viz_attn_layers (default all; negative indices allowed) as [B, nl, steps, T], or with
        Prediction.viz_attn_heads [B, nl, H, steps, T].  Rows beyond the maps budget per call are replayed in parts."""
        pred = self.predicter.Prediction
        per_head = bool(getattr(pred, "viz_attn_heads", False))
        want = eng.cross_attention_layers(getattr(pred, "viz_attn_layers", None))
        top = eng.cfg.dec_layers - 1
        layers = want if top in want else want + [top]
        B, T = memory.shape[0], memory.shape[1]
        generated = generated.to(device=memory.device, dtype=torch.int64)
        if start is None:
            start = torch.full((B,), _lib.TOK_GO, dtype=torch.int64, device=memory.device)
        tokens_in = torch.cat([start.to(device=memory.device, dtype=torch.int64).reshape(B, 1), generated[:, :-1]], dim=1)
        per = _lib.ATTN_MAP_BUDGET // max(1, eng.cross_attention_bytes(1, tokens_in.shape[1], T, len(layers), per_head))
        if per < 1:
            raise ValueError(f"the cross-attention maps of ONE sample ({len(layers)} layers, {tokens_in.shape[1]} steps, {T} memory "
                             f"tokens) exceed the {_lib.ATTN_MAP_BUDGET}-byte budget: ask for fewer layers (viz_attn_layers) or "
                             "the head mean (viz_attn_heads off)")
        maps = torch.cat([eng.decode_cross_attention(memory[a:a + per], tokens_in[a:a + per], layers, per_head)
                          for a in range(0, B, per)], dim=0)
        last = maps[:, -1].mean(dim=1) if per_head else maps[:, -1]
        return last, (maps if top in want else maps[:, :len(want)])

    def _luong_check(self):
        """attn_type 'luong': Attention.forward_greedy / forward_beam call `self.attention_cell.reset_mem()` first thing
        (seq2seq.py:114,285; seq2seq_v2.py:65,247) and LuongAttention has no such method, so in the reference every forward
        of such a model -- training or evaluation -- ends in this AttributeError.  Same here, before any GPU work."""
        if self.stages["Pred"] in ("Attn", "Attnv2") and self.opt["Prediction"]["params"].get("attn_type", "coverage") == "luong":
            raise AttributeError("'LuongAttention' object has no attribute 'reset_mem'")

    def forward(self, input, text, is_train=True, is_test=False, rtl_text=None):
        self._luong_check()
        if self.training:
            # module.train(): teacher-forced pass with BatchNorm on batch statistics (tfm.py:103-118 / seq2seq.py:224-331
            # with is_train), one autograd node over the whole network so that loss.backward() (engine/training.py:137)
            # fills every .grad
            from .train import train_forward
            self._refuse_train_attn_hooks()
            if self.stages["Pred"] != "TFM" and self.stages["Seq"] not in ("ViT", "BiLSTM"):  # Attn / Attnv2
                raise NotImplementedError("training the LSTM-attention head is implemented on the HybridViT and BiLSTM encoders")
            logits = train_forward(self, input, text)
            return logits.argmax(dim=2), logits, {}
        contextual_feature, output_shape, feat_pad = self.forward_encoder(input)
        extra = {}
        if self.stages["Pred"] == "TFM" and getattr(self.predicter.Prediction, "viz_attn", False):
            extra["maps_memory"] = self._exact_memory(input, contextual_feature)
        prediction, logits, decoder_attn, addition_outputs = self.forward_decoder(
            contextual_feature, text=text, is_train=is_train, is_test=is_test, rtl_text=rtl_text, **extra)
        # decoder_attn is None for greedy decoding, and for the TFM head (build_pred.py:34,46-49) unless its viz_attn is set
        addition_outputs.update(decoder_attn_outputs(self.stages, decoder_attn, output_shape, feat_pad))
        return prediction, logits, addition_outputs
