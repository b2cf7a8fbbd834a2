"""Configuration bag with the reference's field names (reference src/config.py:71-170).

``get_config`` mirrors the reference's argparse flags for the hot path; dataset paths, wandb names and the BERT
switch are out of scope.  ``optimizer``/``activation`` are looked up by name like the reference
does (config.py:24-27), but resolve to this package's HIP-backed classes / activation ids.
"""
from __future__ import annotations

import argparse
from datetime import datetime

ACTIVATIONS = ("elu", "hardshrink", "hardtanh", "leakyrelu", "prelu", "relu", "rrelu", "tanh")      # reference config.py:25-27


def str2bool(v):
    """reference config.py:61-68"""
    if isinstance(v, bool):
        return v
    if v.lower() in ("yes", "true", "t", "y", "1"):
        return True
    if v.lower() in ("no", "false", "f", "n", "0"):
        return False
    raise argparse.ArgumentTypeError("Boolean value expected.")


def _json_object(text):
    import json
    value = json.loads(text)
    if not isinstance(value, dict):
        raise argparse.ArgumentTypeError("a JSON object is expected")
    if "betas" in value:
        value["betas"] = tuple(value["betas"])
    return value


def _pos_weight(text):
    """--pos_weight balanced, or a JSON list: --pos_weight '[1, 4, 4, 11, 5, 9]'"""
    import json
    if text.strip().lower() == "balanced":
        return "balanced"
    if text.strip().lower() in ("none", ""):
        return None
    try:
        value = json.loads(text)
    except ValueError:
        value = None
    if not isinstance(value, list) or not all(isinstance(x, (int, float)) and not isinstance(x, bool) for x in value):
        raise argparse.ArgumentTypeError("'balanced' or a JSON list of numbers is expected")
    return [float(x) for x in value]


class Config(object):
    """Attribute bag (reference config.py:71-96).  'optimizer' names resolve to mmda_amd.optim classes."""

    def __init__(self, **kwargs):
        for key, value in kwargs.items():
            if key == "optimizer" and isinstance(value, str):
                from . import optim
                value = optim.optimizer_dict[value]
            if key == "activation":
                value = activation_name(value)
            setattr(self, key, value)

    def __str__(self):
        import pprint
        return "Configurations\n" + pprint.pformat(self.__dict__)


def activation_name(act) -> str:
    """Accepts the reference's forms: a name ('leakyrelu'), an nn.Module class (nn.LeakyReLU, config.py:25-27) or
    an instance; returns the lower-case name."""
    if isinstance(act, str):
        name = act.lower()
    else:
        cls = act if isinstance(act, type) else type(act)
        name = cls.__name__.lower()
    if name not in ACTIVATIONS:
        raise ValueError(f"unknown activation '{name}'")
    return name


DEFAULTS = dict(
    mode="train", runs=5, use_confidNet=False, device="cuda", eval_mode="macro",
    use_bert=False, use_cmd_sim=True, data="mosei", name="run",
    num_classes=6, batch_size=64, eval_batch_size=10, n_epoch=40, patience=6,
    diff_weight=0.3, sim_weight=0.7, sp_weight=0.0, recon_weight=0.7, conf_weight=0.3,
    learning_rate=1e-4, optimizer="Adam", clip=1.0, weight_decay=0.1,
    extractor="lstm", rnncell="lstm", embedding_size=300, hidden_size=128, dropout=0.1,
    reverse_grad_weight=1.0, activation="leakyrelu", threshold=0.35, model="MISA",
    # added for the MI355X build (not reference flags)
    visual_size=35, acoustic_size=74, vocab_size=20000, precision="bf16", seq_len=50, pretrained_emb=None,
    fusion_fp8=False, dp_global_stats=False,
    # how embed.weight trains: "dense" (Adam over the whole table: what the reference does), "sparse" (torch.optim.SparseAdam on the
    # rows a batch touches) or "frozen" (fixed pretrained vectors: what the reference's `embed.requires_grad = False` meant to do)
    # ... or "deferred": dense Adam's weights bit for bit, with the update of a row the batch does not touch applied when the row is next
    # needed (or by MISA.flush_embedding()) instead of by a pass over the table every step; embed_deferred_window: steps between the
    # full flushes that bound how far a row can fall behind
    embed_update="dense", embed_deferred_window=256,
    # optimizer steps made from this many consecutive batches each (gradient accumulation with data-parallel semantics: the mean over
    # micro-batches of their gradients, then clip + Adam -- what that many ranks would compute); 1 = the reference's loop
    accum_steps=1,
    # the optimizer beyond its name and lr: optimizer_kwargs go to its constructor (betas, eps, weight_decay ...); clip_norm is
    # torch.nn.utils.clip_grad_norm_'s max_norm, applied in front of `clip` (None = off).  optimizer="AdamW" without a weight_decay among
    # its kwargs takes the weight_decay above -- the reference's flag, which optimizer="Adam" keeps ignoring as the reference does.
    optimizer_kwargs={}, clip_norm=None,
    # after the last epoch of Solver.train(): "global" / "per_class" sweep the decision cut-off(s) over the dev split with the best
    # checkpoint (mmda_amd/calibrate.py; objective: what eval_mode names) and the final test evaluation decides with them; "none": the
    # reference's loop, which decides with `threshold` throughout
    calibrate="none",
    # the classification criterion beyond the reference's plain BCE: pos_weight -- None, one weight per class on the
    # positive term (BCEWithLogitsLoss's convention), or "balanced", which Solver.build() resolves to (N - n_c) / n_c from the training
    # set's labels -- and the focal exponent focal_gamma (0, or 1 .. 8).  The defaults are the reference's criterion, bit for bit.
    pos_weight=None, focal_gamma=0.0,
    # which dev figure Solver.train() keeps the best checkpoint by: "valid_loss" (the reference's loop: the lowest dev loss), or the
    # highest "map" / "auroc" -- macro average precision / macro AUROC of the dev scores (mmda_amd/ranking.py), figures
    # that move neither with `threshold` nor with the criterion's weights
    select_by="valid_loss",
    # which of a MOSEI sample's two targets the model's head is trained on: "emotion" -- the six-class multi-label
    # classifier, the reference's published configuration -- or "sentiment": the (-3, 3) regression target, one output column
    # (num_classes=1) without the sigmoid, under senti_loss "l1" (the reference's commented nn.L1Loss, config.py's criterion_dict['mosi'])
    # or "mse"; evaluation then reports the reference's eval_mosei_senti table
    task="emotion", senti_loss="l1",
    # after the last epoch of Solver.train(), in front of `calibrate`: "temperature" / "platt" fit one logit scaling q = sigmoid(a z + b)
    # of the scores (a alone / a and b; mmda_amd/reliability.py) on the dev split with the best checkpoint; the cut-offs
    # of `calibrate` are then chosen on, and the final test evaluation scores with, the scaled scores; "none": raw scores throughout
    scaling="none",
    # after the final test pass of Solver.train(): N > 0 runs MC dropout with N draws per sample over the test split with the best
    # checkpoint (mmda_amd/uncertainty.py) and prints how each confidence -- maximum class probability, the MC-dropout
    # figures, ConfidNet's tcp -- ranks the right decisions above the wrong ones; 0: nothing happens
    mc_passes=0,
    # after the final test pass of Solver.train(), behind `scaling` / `calibrate`: R > 0 resamples the test split R times (1 .. 8192)
    # with the best checkpoint (mmda_amd/bootstrap.py) and prints every figure of the cut-off and ranking reports as
    # `figure  point  [lo, hi]`, with calibrated cut-offs also their paired difference to `threshold`; 0: nothing happens
    bootstrap=0,
    # after the final test pass of Solver.train(), next to `mc_passes`' table: N > 0 (1 .. 16) fits the Trust Score on the hidden
    # vectors of the training split with the best checkpoint (mmda_amd/neighbours.py), N the neighbour count of its
    # density filter and `trust_alpha` in [0, 1) the share of each label's rows the filter drops, and prints how it ranks the right
    # decisions of the test split above the wrong ones beside maximum class probability and ConfidNet's tcp; 0: nothing happens
    trust_k=0,
    trust_alpha=0.0,
)


def get_config(parse=True, **optional_kwargs):
    """reference config.py:99-170 (same flags, same defaults except use_bert which is fixed False: the BERT branch
    needs a hub download and is out of scope)."""
    parser = argparse.ArgumentParser()
    for k, v in DEFAULTS.items():
        if isinstance(v, bool):
            parser.add_argument(f"--{k}", type=str2bool, default=v)
        elif k == "optimizer_kwargs":                          # a JSON object: --optimizer_kwargs '{"betas": [0.9, 0.98]}'
            parser.add_argument(f"--{k}", type=_json_object, default=dict(v))
        elif k == "clip_norm":
            parser.add_argument(f"--{k}", type=float, default=None)
        elif k == "pos_weight":
            parser.add_argument(f"--{k}", type=_pos_weight, default=None)
        elif k == "calibrate":
            parser.add_argument(f"--{k}", choices=("none", "global", "per_class"), default=v)
        elif k == "select_by":
            parser.add_argument(f"--{k}", choices=("valid_loss", "map", "auroc"), default=v)
        elif k == "task":
            parser.add_argument(f"--{k}", choices=("emotion", "sentiment"), default=v)
        elif k == "senti_loss":
            parser.add_argument(f"--{k}", choices=("l1", "mse"), default=v)
        elif k == "scaling":
            parser.add_argument(f"--{k}", choices=("none", "temperature", "platt"), default=v)
        elif v is None:
            parser.add_argument(f"--{k}", default=None)
        else:
            parser.add_argument(f"--{k}", type=type(v), default=v)
    if parse:
        kwargs = vars(parser.parse_args())
    else:
        kwargs = vars(parser.parse_known_args()[0])
    if kwargs.get("name") == "run":
        kwargs["name"] = datetime.now().strftime("%Y-%m-%d_%H:%M:%S")
    kwargs.update(optional_kwargs)
    if kwargs.get("use_bert"):
        raise NotImplementedError("use_bert=True needs bert-base-uncased from the hub; only the GloVe/LSTM text branch is built")
    if "word2id" not in kwargs:
        kwargs["word2id"] = range(kwargs["vocab_size"])        # only len() is read (reference models.py:47)
    return Config(**kwargs)


def make_config(**kw):
    """Programmatic construction with the reference's defaults."""
    d = dict(DEFAULTS, optimizer_kwargs={})
    d.update(kw)
    if "word2id" not in d:
        d["word2id"] = range(d["vocab_size"])
    return Config(**d)
