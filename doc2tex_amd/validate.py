"""`validation_step` of the reference's training loop (doc2tex/engine/inferencing.py:12-247) on the engine.

Same signature, same 11-tuple in the same order.  What differs from the reference is where the work happens:

  * the strings of a batch come from one `LabelDecoder.to_latex` call per tensor (decode, the cut at "[s]" -- with the
    reference's `find() == -1` quirk, which drops the last character of a row without "[s]" -- and the whitespace
    clean-up, in native code) instead of per-sample Python;
  * exact match, character NED, word NED and BLEU go through `metrics.ValidationMetrics`: the edit distances and the
    clipped n-gram counts are computed by kernels on the current stream, their integers stay on the device, and ONE
    download at the end of the run feeds the reference's closing arithmetic.  The per-sample losses are kept on the
    device the same way;
  * `export_csv` rows are written at the end from the downloaded records (same columns, same order, same file name);
  * the reference's "confidence score" block (inferencing.py:98-106,175-183) is dead code -- its running product starts
    from zeros and the result is never used -- and is not reproduced;
  * the loop is synchronous: one forward, then that batch's strings.  Overlapping the two (`model.pipelined`) is not
    done here.
"""
import time

import torch

from . import _lib
from .metrics import ValidationMetrics
from .postprocess import LabelDecoder


def _label_decoder(converter):
    """The converter itself if it is a LabelDecoder, otherwise one over the same vocabulary (the reference's converters
    list their special tokens first: [PAD] [GO] [s] [UNK] for TFM, [GO] [s] [UNK] for Attn)."""
    if isinstance(converter, LabelDecoder):
        return converter
    character = list(converter.character)
    if character[:1] == ["[PAD]"]:
        return LabelDecoder(character[4:], "TFM")
    return LabelDecoder(character[3:], "Attn")


def validation_step(model, augment, criterion, evaluation_loader, converter, config, args, device):
    """validation or evaluation: returns (all_loss, total_names, averaged loss, accuracy, bleu_score, norm_ED, word_ED,
    total_preds, total_labels, infer_time, length_of_data).  `criterion`: a `reduction="none"` criterion of
    doc2tex_amd.loss; `converter`: the reference's TFMLabelConverter / AttnLabelConverter or a LabelDecoder."""
    _lib.require_device()
    head = config["Prediction"]["name"]
    attn = "Attn" in head
    if not attn and head != "TFM":
        raise NotImplementedError(f"validation_step: Prediction '{head}' (the reference serves the Attn heads and TFM)")
    token_level = config.get("token_level", "word")
    postprocess = bool(config.get("postprocess", True))
    decoder = _label_decoder(converter)
    metrics = ValidationMetrics(converter.dict["[s]"], token_level)

    length_of_data = 0
    infer_time = 0
    loss_sum, loss_count = 0, 0
    batch_costs, total_names = [], []

    for image_tensors, labels, img_names in evaluation_loader:
        if image_tensors is None and labels is None and img_names is None:
            break
        batch_size = image_tensors.size(0)
        length_of_data = length_of_data + batch_size
        assert image_tensors.device.type == device

        if augment:
            image_tensors = torch.clamp(image_tensors, min=0.0, max=255.0)
            image_tensors = image_tensors.div(255.0)
            image_tensors = getattr(augment, "normalize")(image_tensors)

        start_time = time.time()
        if attn:
            text_for_pred = torch.LongTensor(batch_size, config["batch_max_length"] + 1).fill_(0).to(device)
            kwargs = {"is_train": False}
        else:
            text_for_pred = torch.LongTensor(batch_size, 1).fill_(converter.dict["[GO]"]).to(device)
            kwargs = {}
        text_for_loss, _ = converter.encode(labels, batch_max_length=config["batch_max_length"])
        if config["use_amp"]:
            with torch.autocast(device_type=device):
                preds_index, preds, _ = model(image_tensors, text_for_pred, **kwargs)
        else:
            preds_index, preds, _ = model(image_tensors, text_for_pred, **kwargs)
        infer_time += time.time() - start_time

        target = text_for_loss[:, 1:]  # without [GO] Symbol
        costs = criterion(preds.contiguous().view(-1, preds.shape[-1]), target.contiguous().view(-1))
        costs = costs.view(batch_size, -1).mean(dim=1)
        loss_count += costs.data.numel()  # the reference's Averager: running sum of the tensors' sums over their element count
        loss_sum = loss_sum + costs.data.sum()
        batch_costs.append(costs.detach())

        pred_strs = decoder.to_latex(preds_index, token_level, postprocess)
        gt_strs = decoder.to_latex(target, token_level, postprocess)
        metrics.update(preds_index, target, pred_strs, gt_strs)
        total_names += list(img_names)

        if config["sanity_check"]:
            break

    result = metrics.compute()  # the one metrics download; divides by zero on an empty loader as the reference does
    all_loss = torch.cat(batch_costs).cpu().numpy().tolist()
    total_preds = [r["pred"] for r in result["records"]]
    total_labels = [r["gt"] for r in result["records"]]

    if config["export_csv"]:
        import csv

        eval_data = config["eval_data"].split("/")[-1]
        save_path = f"./result/{config['exp_name']}/{args.log_path[:-4]}_{eval_data}.csv"
        with open(save_path, "wt") as fo:
            writer = csv.writer(fo)
            for cost, img_name, r in zip(all_loss, total_names, result["records"]):
                writer.writerow((cost, img_name, r["pred"], r["gt"], 1 if r["correct"] else 0))

    valid_loss = loss_sum / float(loss_count) if loss_count != 0 else 0
    return (all_loss, total_names, valid_loss, result["accuracy"], result["bleu"], result["norm_ED"], result["word_ED"],
            total_preds, total_labels, infer_time, length_of_data)
