"""CPU: mmda_amd/step_rules.py -- the one table of what no optimizer step does -- over its full grid, and the callers that ask it."""
import itertools

import pytest
import torch

from mmda_amd import MISA, _lib, make_config, optim, step_rules
from mmda_amd.solver import Solver

# one letter per rule, in the order in which the rules are looked at ('.': the step is allowed)
LETTER = {"A": "rows_optimizer", "B": "rows_exchange", "C": "accum_optimizer", "D": "accum_exchange", "E": "accum_deferred",
          "F": "accum_no_adam", "G": "decay_deferred", "H": "norm_value", "I": "norm_optimizer", "J": "norm_rows", "K": "norm_exchange",
          "L": "frozen_exchange", "M": "encoded_exchange", "N": "encoded_accum", ".": None}
OPTIMIZERS = {"none": (None, 0.0), "Adam": ("adam", 0.0), "AdamW": ("adam", 0.1), "RMSprop": ("other", 0.0)}
# EXPECTED[embed_update][optimizer]: 16 verdicts, clip_norm (None, 1.0) x exchange (off, on) x accumulation (off, on) x encoded (off, on),
# the last one fastest.  Written out by hand from the rule list ("what no step does"): the first rule that applies, in order.
_PLAIN = "...N.MDD" "...NKKDD"          # no rows mode, Adam or the native default
_PLAIN_RMS = "..CC.MCC" "IICCIICC"
EXPECTED = {
    "dense": {"none": _PLAIN, "Adam": _PLAIN, "AdamW": _PLAIN, "RMSprop": _PLAIN_RMS},
    "frozen": {"none": _PLAIN, "Adam": _PLAIN, "AdamW": _PLAIN, "RMSprop": _PLAIN_RMS},
    "sparse": {"none": "...NBBBB" "JJJJBBBB", "Adam": "...NBBBB" "JJJJBBBB", "AdamW": "...NBBBB" "JJJJBBBB", "RMSprop": "A" * 16},
    "deferred": {"none": "..EEBBBB" "JJEEBBBB", "Adam": "..EEBBBB" "JJEEBBBB", "AdamW": "GGEEBBBB" "GGEEBBBB", "RMSprop": "A" * 16},
}


def test_the_full_grid_against_the_hand_written_verdicts():
    assert [n for n, _ in step_rules.RULES] == [LETTER[c] for c in "ABCDEFGHIJKLMN"]
    seen = 0
    for eu, per_opt in EXPECTED.items():
        for opt, verdicts in per_opt.items():
            kind, wd = OPTIMIZERS[opt]
            grid = itertools.product((None, 1.0), (False, True), (False, True), (False, True))
            for letter, (clip_norm, exchange, accumulate, encoded) in zip(verdicts, grid, strict=True):
                case = dict(embed_update=eu, optimizer=kind, weight_decay=wd, clip_norm=clip_norm, exchange=exchange,
                            accumulate=accumulate, encoded=encoded)
                assert step_rules.verdict(**case) == LETTER[letter], case
                if letter == ".":
                    step_rules.check(optimizer_name=opt, **case)
                else:
                    with pytest.raises(_lib.MMDAError) as e:
                        step_rules.check(optimizer_name=opt, **case)
                    assert str(e.value) == step_rules.text(LETTER[letter], eu, opt, clip_norm), case
                seen += 1
    assert seen == 256


def test_the_rules_outside_the_grid_and_the_words_callers_match():
    assert step_rules.verdict(accumulate=True, do_adam=False) == "accum_no_adam"
    assert step_rules.verdict(frozen=True, exchange=True) == "frozen_exchange"
    assert step_rules.verdict(frozen=True) is None and step_rules.verdict(embed_update="frozen", exchange=True) is None
    for bad in (-1.0, float("nan")):
        assert step_rules.verdict(clip_norm=bad) == "norm_value"
    assert step_rules.verdict(clip_norm=0.0, exchange=True, optimizer="other", embed_update="sparse") == "rows_optimizer"
    assert step_rules.verdict(clip_norm=0.0, exchange=True) is None
    words = {"rows_optimizer": ["RMSprop"], "rows_exchange": ["gradient exchange", "grad_sync", "not built yet", "embed_update='sparse'"],
             "accum_optimizer": ["RMSprop", "not built"], "accum_exchange": ["grad_sync", "not built yet"], "accum_deferred": ["deferred"],
             "decay_deferred": ["weight_decay", "deferred"], "norm_value": ["clip_norm"], "norm_optimizer": ["clip_norm", "RMSprop"],
             "norm_rows": ["clip_norm", "embed_update='sparse'"], "norm_exchange": ["clip_norm", "gradient exchange"],
             "frozen_exchange": ["not built yet", "gradient exchange"], "encoded_exchange": ["gradient exchange", "not built"],
             "encoded_accum": ["not built"]}
    for rule, subs in words.items():
        t = step_rules.text(rule, "sparse", "RMSprop", -1.0)
        assert all(w in t for w in subs), (rule, t)


def _solver(**kw):
    cfg = make_config(vocab_size=32, **kw)
    return Solver(cfg, cfg, cfg, [], [], [], is_train=True, model=MISA(cfg)), cfg


def _optimizer(model, name):
    if name is None:
        return None
    kw = dict(weight_decay=0.1) if name == "AdamW" else {}
    return getattr(optim, name)(list(model.parameters()), lr=1e-3, **kw).attach(model)


# (rule, config, the optimizer handed to the step, further arguments of the step)
SAME_TEXT = [("rows_optimizer", dict(embed_update="sparse", optimizer="RMSprop"), "RMSprop", {}),
             ("rows_optimizer", dict(embed_update="deferred", optimizer="RMSprop"), "RMSprop", {}),
             ("decay_deferred", dict(embed_update="deferred", optimizer="AdamW"), "AdamW", {}),
             ("norm_optimizer", dict(optimizer="RMSprop", clip_norm=1.0), "RMSprop", dict(clip_norm=1.0)),
             ("norm_rows", dict(embed_update="sparse", clip_norm=1.0), "Adam", dict(clip_norm=1.0)),
             ("accum_optimizer", dict(optimizer="RMSprop", accum_steps=2), "RMSprop", dict(accum_index=0, accum_count=2)),
             ("accum_deferred", dict(embed_update="deferred", accum_steps=2), "Adam", dict(accum_index=0, accum_count=2))]


@pytest.mark.parametrize("case", SAME_TEXT, ids=[f"{c[0]}-{c[1].get('embed_update', 'dense')}" for c in SAME_TEXT])
def test_solver_build_and_the_step_raise_the_same_rules_text(case):
    rule, ckw, opt_name, skw = case
    s, cfg = _solver(**ckw)
    want = step_rules.text(rule, cfg.embed_update, opt_name, skw.get("clip_norm"))
    with pytest.raises(_lib.MMDAError) as e:
        s.build()
    assert str(e.value) == want
    m = MISA(cfg)
    with pytest.raises(_lib.MMDAError) as e:
        m.train_step(None, None, None, None, None, lr=1e-3, clip=1.0, optimizer=_optimizer(m, opt_name), **skw)
    assert str(e.value) == want
    assert m._step == 0 and m._seed == MISA(cfg)._seed and m._acc_next == 0


@pytest.mark.parametrize("eu, kw, rule", [("sparse", {}, "rows_exchange"), ("deferred", {}, "rows_exchange"),
                                          ("dense", dict(clip_norm=1.0), "norm_exchange"),
                                          ("dense", dict(accum_index=0, accum_count=2), "accum_exchange")])
def test_a_refused_exchange_is_never_called(eu, kw, rule):
    """(what the step methods refuse with a grad_sync, they refuse in front of the step: no seed drawn, no step counted, no call)"""
    m = MISA(make_config(vocab_size=32, embed_update=eu))
    calls = []
    seed = m._seed
    with pytest.raises(_lib.MMDAError) as e:
        m.train_step(None, None, None, None, None, lr=1e-3, clip=1.0, grad_sync=lambda g, n: calls.append(1) or 1.0, **kw)
    assert str(e.value) == step_rules.text(rule, eu, "", kw.get("clip_norm"))
    assert "not built" in str(e.value) and "gradient exchange" in str(e.value)
    assert not calls and m._step == 0 and m._seed == seed


def test_the_unfused_callers_ask_the_same_table(monkeypatch):
    m = MISA(make_config(vocab_size=32, embed_update="sparse"))
    m._G = torch.zeros(4)                                    # (clip_grad_norm_ looks for a bucket and a stream before it asks)
    monkeypatch.setattr(_lib, "stream_ptr", lambda: None)
    with pytest.raises(_lib.MMDAError) as e:
        optim.clip_grad_norm_(m, 1.0)
    assert str(e.value) == step_rules.text("norm_rows", "sparse", "", 1.0)
    with pytest.raises(_lib.MMDAError) as e:
        m._push_adam(None, 1.0)
    assert str(e.value) == step_rules.text("norm_rows", "sparse", "", 1.0)
    d = MISA(make_config(vocab_size=32))
    d.freeze("trnn1")
    with pytest.raises(_lib.MMDAError) as e:
        d._sync_trainable(exchange=True)
    assert str(e.value) == step_rules.text("frozen_exchange")
