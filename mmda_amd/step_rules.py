"""What no optimizer step does, in one place: a pure function over plain values (no torch, no library).  ``Solver.build``, the ``MISA``
step methods, ``Adam.step``, ``RMSprop.step`` and ``clip_grad_norm_`` compute their own booleans -- what counts as a gradient exchange
differs between them -- and ask here.  DESIGN.md ("what no step does") gives the reason for each rule."""
from __future__ import annotations

from ._lib import MMDAError

ROWS = ("sparse", "deferred")            # the table's rows are updated where their gradient sums become final
_X = "a gradient exchange (grad_sync / data parallel)"

# (name, text) in the order in which they are looked at: the first rule that applies is the one raised
RULES = (
    ("rows_optimizer", "embed_update='{eu}' is built for Adam / AdamW only, not {opt} (torch has no sparse RMSprop to match)"),
    ("rows_exchange", "embed_update='{eu}' with " + _X + " is not built yet (use 'dense' or 'frozen')"),
    ("accum_optimizer", "accum_steps > 1 with optimizer {opt} is not built: Adam / AdamW only"),
    ("accum_exchange", "accum_steps > 1 together with " + _X + " is not built yet"),
    ("accum_deferred", "accum_steps > 1 with embed_update='deferred' is not built: the mode's contract is dense Adam's bits, which one "
                       "rows update over the micro-batches' concatenated list does not give (use 'dense': the same weights)"),
    ("accum_no_adam", "accum_steps > 1 with do_adam=False: the accumulated step ends in its optimizer step"),
    ("decay_deferred", "weight_decay > 0 with embed_update='deferred' is not built: the replay ring keeps two scalars per update and a "
                       "decayed zero-gradient step needs a third (use 'dense' or 'sparse')"),
    ("norm_value", "clip_norm must be >= 0 (None or 0: off), not {clip_norm}"),
    ("norm_optimizer", "clip_norm with optimizer {opt} is not built: Adam / AdamW only"),
    ("norm_rows", "clip_norm with embed_update='{eu}' is not built: the table's rows are updated where their gradient sums become final, "
                  "before a norm of the whole gradient exists (use 'dense' or 'frozen')"),
    ("norm_exchange", "clip_norm with " + _X + " is not built: the early step updates a prefix before the whole gradient exists"),
    ("frozen_exchange", "frozen parameters (requires_grad=False) together with " + _X + " are not built yet"),
    ("encoded_exchange", "a step from the encoder cache with a gradient exchange (grad_sync / a process group) is not built"),
    ("encoded_accum", "a step from the encoder cache with gradient accumulation (accum_steps > 1, accum_index, accum_count) is not built"),
)


# What the classification criterion refuses.  These are refusals of a SETTING, raised where it is made (MISA.set_cls_loss,
# bce_sum_over_classes, DeviceEval.add_cls_loss), not of a step: the criterion combines with every step form, so RULES has no entry for it.
CLS_MAX_CLASSES = 16
CLS_RULES = (
    ("cls_gamma", "focal_gamma must be 0 or between 1 and 8, not {gamma}: for 0 < gamma < 1 the gradient's (1-s)^(gamma-1) diverges where "
                  "the loss vanishes"),
    ("cls_weight_count", "pos_weight has {n} entries, the model {ncls} classes"),
    ("cls_weight_classes", "pos_weight is built for at most 16 classes, not {ncls}"),
    ("cls_weight_value", "pos_weight must be finite and >= 0, not {bad} (class {c})"),
)


def cls_verdict(pos_weight, focal_gamma, num_classes: int):
    """(rule, format values) of the first rule that refuses the setting, or None.  ``pos_weight``: None or a sequence of numbers."""
    try:
        g = float(focal_gamma)
    except (TypeError, ValueError):
        return "cls_gamma", dict(gamma=repr(focal_gamma))
    if not (g == 0.0 or 1.0 <= g <= 8.0):
        return "cls_gamma", dict(gamma=focal_gamma)
    if pos_weight is None:
        return None
    w = list(pos_weight)
    if len(w) != num_classes:
        return "cls_weight_count", dict(n=len(w), ncls=num_classes)
    if num_classes > CLS_MAX_CLASSES:
        return "cls_weight_classes", dict(ncls=num_classes)
    for c, x in enumerate(w):
        x = float(x)
        if not (0.0 <= x < float("inf")):
            return "cls_weight_value", dict(bad=x, c=c)
    return None


def cls_setting(pos_weight, focal_gamma, num_classes: int):
    """The setting as the native side takes it, (weights tuple or None, gamma), or MMDAError with the text of the rule that refuses it.
    Weights that are all 1 are passed down as None: with gamma = 0 that is the plain criterion, whose bits are the reference's."""
    hit = cls_verdict(pos_weight, focal_gamma, num_classes)
    if hit is not None:
        raise MMDAError(dict(CLS_RULES)[hit[0]].format(**hit[1]))
    w = None if pos_weight is None else tuple(float(x) for x in pos_weight)
    if w is not None and all(x == 1.0 for x in w):
        w = None
    return w, float(focal_gamma)


# What the sentiment task refuses.  Like CLS_RULES these are refusals of a SETTING, raised where it is made (MISA.__init__,
# MISA.set_task, MISA.set_cls_loss, Solver.build, Solver.calibrate, Solver.rank) with nothing changed: the task combines with every step
# form -- the target reaches the step through the pointer the labels came through -- so RULES has no entry for it either.
TASKS = ("emotion", "sentiment")
SENTI_LOSSES = ("l1", "mse")
SENTI_RULES = (
    ("task_name", "task must be 'emotion' or 'sentiment', not {task!r}"),
    ("senti_loss", "senti_loss must be 'l1' or 'mse', not {loss!r}"),
    ("senti_classes", "task='sentiment' has one regression output: num_classes must be 1, not {ncls}"),
    ("senti_confid", "task='sentiment' with use_confidNet is not built: the confidence target truth * pred is defined for labels in {{0, 1}}"),
    ("senti_pos_weight", "task='sentiment' with pos_weight is not built: the weight belongs to the positive term of the classification "
                         "criterion"),
    ("senti_focal", "task='sentiment' with focal_gamma = {gamma} is not built: the focal factor belongs to the classification criterion "
                    "(focal_gamma must be 0)"),
    ("senti_calibrate", "task='sentiment' with threshold calibration (Solver.calibrate, calibrate={how!r}) is not built: the cut-off "
                        "figures are classification figures"),
    ("senti_rank", "task='sentiment' with Solver.rank is not built: AUROC and average precision are classification figures"),
    ("senti_select_by", "task='sentiment' with select_by={select_by!r} is not built: the ranking figures are classification figures (the "
                        "best checkpoint is the one with the lowest dev loss: the dev MAE under senti_loss='l1')"),
)


def task_verdict(task="emotion", senti_loss="l1", num_classes=1, use_confidNet=False, pos_weight=None, focal_gamma=0.0,
                 calibrate="none", select_by="valid_loss", rank=False):
    """(rule, format values) of the first rule of SENTI_RULES that refuses the setting, or None.  ``calibrate``: config.calibrate, or any
    other value than "none" for a call of Solver.calibrate; ``rank``: a call of Solver.rank.  Under task='emotion' nothing is looked at
    but the task's name."""
    if task not in TASKS:
        return "task_name", dict(task=task)
    if task == "emotion":
        return None
    if senti_loss not in SENTI_LOSSES:
        return "senti_loss", dict(loss=senti_loss)
    if isinstance(num_classes, bool) or num_classes != 1:
        return "senti_classes", dict(ncls=num_classes)
    if use_confidNet:
        return "senti_confid", {}
    if pos_weight is not None:
        return "senti_pos_weight", {}
    try:
        zero = float(focal_gamma) == 0.0
    except (TypeError, ValueError):
        zero = False
    if not zero:
        return "senti_focal", dict(gamma=focal_gamma)
    if calibrate not in (None, "none"):
        return "senti_calibrate", dict(how=calibrate)
    if rank:
        return "senti_rank", {}
    if select_by not in (None, "valid_loss"):
        return "senti_select_by", dict(select_by=select_by)
    return None


def task_check(task="emotion", senti_loss="l1", **values) -> None:
    """Raises MMDAError with the text of the rule that refuses the setting (``task_verdict``'s arguments)."""
    hit = task_verdict(task, senti_loss, **values)
    if hit is not None:
        raise MMDAError(dict(SENTI_RULES)[hit[0]].format(**hit[1]))


# What modality masking refuses.  A keep set is an operation on a batch's INPUTS, made where the batch is made; a path
# that has no inputs left to mask refuses it where the keep set is given (MISA.forward_encoded, InferencePass, Solver.eval / infer /
# modalities), with nothing run.
MODALITY_RULES = (
    ("modality_encoded", "a keep set ({keep}) on the encoder cache (EncodedLoader / forward_encoded) is not built: the cache holds the "
                         "encoder outputs of whole samples, and a masked input needs the encoders run again (use the DeviceLoader the "
                         "cache was built from)"),
)


def modality_verdict(keep=None, encoded: bool = False):
    """(rule, format values) of the first rule of MODALITY_RULES that refuses the setting, or None.  ``keep``: None or the keep set's
    three bits (7 keeps everything and is refused nowhere); ``encoded``: the batches come from the encoder cache."""
    if encoded and keep is not None and int(keep) != 7:
        return "modality_encoded", dict(keep=int(keep))
    return None


def modality_check(keep=None, encoded: bool = False) -> None:
    """Raises MMDAError with the text of the rule that refuses the setting (``modality_verdict``'s arguments)."""
    hit = modality_verdict(keep, encoded)
    if hit is not None:
        raise MMDAError(dict(MODALITY_RULES)[hit[0]].format(**hit[1]))


# What reliability and logit scaling refuse: both read a score as the probability of a label, and the sentiment task's
# one output column is a regression value.  Refused where it is asked for (config.scaling at Solver.build, Solver.reliability /
# fit_scaling, a scaling handed to Solver.eval / calibrate), with nothing run.
SCALING_RULES = (
    ("senti_scaling", "task='sentiment' with {what} is not built: reliability and logit scaling read a score as the probability of a "
                      "label, and the sentiment output is a regression value"),
)


def scaling_verdict(task="emotion", scaling="none", reliability=False):
    """(rule, format values) of the first rule of SCALING_RULES that refuses the setting, or None.  ``scaling``: config.scaling, or any
    other value than "none" / None for a scaling fitted or applied by a call; ``reliability``: a call of Solver.reliability."""
    if task == "sentiment" and (reliability or scaling not in (None, "none")):
        return "senti_scaling", dict(what="Solver.reliability" if reliability else f"logit scaling (scaling={scaling!r})")
    return None


def scaling_check(task="emotion", scaling="none", reliability=False) -> None:
    """Raises MMDAError with the text of the rule that refuses the setting (``scaling_verdict``'s arguments)."""
    hit = scaling_verdict(task, scaling, reliability)
    if hit is not None:
        raise MMDAError(dict(SCALING_RULES)[hit[0]].format(**hit[1]))


# What the bootstrap refuses.  Refused where it is asked for (config.bootstrap at Solver.build, Solver.bootstrap, the
# Bootstrap class and its calls), with nothing run.  The limits are those of csrc/bootstrap.hip.
BOOT_MAX_REPLICATES, BOOT_MAX_ROWS, BOOT_MAX_CLASSES, BOOT_RANK_MAX_ROWS = 8192, 1 << 20, 16, 16384
BOOTSTRAP_RULES = (
    ("boot_sentiment", "task='sentiment' with the bootstrap (Solver.bootstrap, bootstrap={replicates}) is not built: the resampled "
                       "figures are classification figures"),
    ("boot_sharded", "the bootstrap resamples each rank's own {mode} loader and exchanges nothing: under a process group the {mode} loader "
                     "must not be sharded (shard={shard}); give every rank the whole split or set bootstrap=0"),
    ("boot_replicates", "replicates must be an integer in 1 .. 8192 (one workgroup sorts a figure's replicates in LDS), not {replicates!r}"),
    ("boot_rows", "a bootstrap over n = {n} rows is outside 1 .. 2^20 = 1048576 rows"),
    ("boot_classes", "a bootstrap table must have 1 .. 16 classes (a row is packed into 16 + 16 bits), not C = {C}"),
    ("boot_rank_rows", "a ranking bootstrap over n = {n} rows is over the limit of 16384 rows: a replicate's row weights and their scan "
                       "stay in 128 KiB of LDS"),
    ("boot_compare", "compare needs two results of the same Bootstrap over the same figures: {why}"),
)


def bootstrap_verdict(task="emotion", replicates=1, n=1, C=1, rank=False, sharded=None, mode="test", compare=None):
    """(rule, format values) of the first rule of BOOTSTRAP_RULES that refuses the setting, or None.  ``rank``: the ranking figures
    are asked for; ``sharded``: the shard of the split's loader under a process group, or None; ``compare``: None, or why two results
    cannot be compared."""
    if task == "sentiment":
        return "boot_sentiment", dict(replicates=replicates)
    if sharded is not None:
        return "boot_sharded", dict(mode=mode, shard=sharded)
    if isinstance(replicates, bool) or not isinstance(replicates, int) or not 1 <= replicates <= BOOT_MAX_REPLICATES:
        return "boot_replicates", dict(replicates=replicates)
    if not 1 <= n <= BOOT_MAX_ROWS:
        return "boot_rows", dict(n=n)
    if not 1 <= C <= BOOT_MAX_CLASSES:
        return "boot_classes", dict(C=C)
    if rank and n > BOOT_RANK_MAX_ROWS:
        return "boot_rank_rows", dict(n=n)
    if compare is not None:
        return "boot_compare", dict(why=compare)
    return None


def bootstrap_check(**values) -> None:
    """Raises MMDAError with the text of the rule that refuses the setting (``bootstrap_verdict``'s arguments)."""
    hit = bootstrap_verdict(**values)
    if hit is not None:
        raise MMDAError(dict(BOOTSTRAP_RULES)[hit[0]].format(**hit[1]))


# What the Trust Score refuses.  Refused where it is asked for (config.trust_k at Solver.build, Solver.trust,
# TrustIndex.fit), with nothing run.
TRUST_RULES = (
    ("trust_sentiment", "task='sentiment' with the Trust Score (Solver.trust, trust_k={k}) is not built: its sets are the training rows "
                        "of each label, and the sentiment task's one output column is a regression value"),
)


def trust_verdict(task="emotion", k=10):
    """(rule, format values) of the first rule of TRUST_RULES that refuses the setting, or None."""
    if task == "sentiment":
        return "trust_sentiment", dict(k=k)
    return None


def trust_check(**values) -> None:
    """Raises MMDAError with the text of the rule that refuses the setting (``trust_verdict``'s arguments)."""
    hit = trust_verdict(**values)
    if hit is not None:
        raise MMDAError(dict(TRUST_RULES)[hit[0]].format(**hit[1]))


def verdict(embed_update: str = "dense", optimizer: str | None = None, weight_decay: float = 0.0, clip_norm=None,
            exchange: bool = False, accumulate: bool = False, encoded: bool = False, frozen: bool = False,
            do_adam: bool = True) -> str | None:
    """The name of the first rule that refuses the step, or None.  ``optimizer``: "adam" (Adam, AdamW), "other", or None (the native
    step's own Adam).  ``frozen``: parameters beyond the table have requires_grad=False."""
    rows, other = embed_update in ROWS, optimizer == "other"
    cn = 0.0 if clip_norm is None else float(clip_norm)
    applies = (rows and other, rows and exchange,
               accumulate and other, accumulate and exchange, accumulate and embed_update == "deferred", accumulate and not do_adam,
               weight_decay > 0 and embed_update == "deferred",
               not cn >= 0.0, cn > 0 and other, cn > 0 and rows, cn > 0 and exchange,
               frozen and exchange, encoded and exchange, encoded and accumulate)
    for (name, _), hit in zip(RULES, applies):
        if hit:
            return name
    return None


def text(rule: str, embed_update: str = "dense", optimizer_name: str = "", clip_norm=None) -> str:
    return dict(RULES)[rule].format(eu=embed_update, opt=optimizer_name, clip_norm=clip_norm)


def check(embed_update: str = "dense", optimizer: str | None = None, optimizer_name: str = "", clip_norm=None, **values) -> None:
    """Raises MMDAError with the text of the rule that refuses the step (``verdict``'s arguments; ``optimizer_name`` is for the text)."""
    rule = verdict(embed_update, optimizer, clip_norm=clip_norm, **values)
    if rule is not None:
        raise MMDAError(text(rule, embed_update, optimizer_name, clip_norm))
