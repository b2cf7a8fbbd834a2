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
