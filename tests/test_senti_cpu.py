"""The sentiment task without a GPU: the collector's numpy restatement against the reference's fixture, the rules table,
the two configuration flags, and the criterion's torch restatement against torch's own l1_loss / mse_loss and their autograd.
tests/test_gpu_senti.py holds the device to the same restatements."""
import sys

import numpy as np
import pytest
import torch

import senti_cases as sc
from mmda_amd import _lib, step_rules
from mmda_amd.config import DEFAULTS, get_config, make_config

FIX = sc.load_fixture()


# ------------------------------------------------------------------------------------------------ collector restatement vs the fixture
def test_fixture_covers_the_cases_it_is_for():
    nan = lambda n, k: np.isnan(FIX[n][2][k])
    assert all((t != 0).any() for _, t, _ in FIX.values())                       # the reference runs on each
    assert max(p.size for p, _, _ in FIX.values()) <= 700
    assert any((t == 0).any() for _, t, _ in FIX.values())
    assert any((p == 0).any() for p, _, _ in FIX.values())                       # >= 0 against > 0
    assert nan("no_extreme_64", "mae_intensity") and nan("const_pred_50", "corr") and nan("one_row", "corr")
    assert not nan("one_row", "mae_intensity") and nan("one_row_wrong_sign", "mae_intensity")
    p = FIX["half_even_clips_22"][0]
    assert {0.5, -0.5, 1.5, -1.5, 2.5, -2.5}.issubset(set(p.tolist())) and p.max() > 3 and p.min() < -3
    assert (FIX["all_positive_pred_80"][0] > 0).all() and (FIX["all_negative_pred_80"][0] < 0).all()
    for n, (_, _, f) in FIX.items():                                             # 'mult' is Acc-7 again
        assert f["mult"] == f["acc7"], n


@pytest.mark.parametrize("split", sc.SPLITS, ids=lambda s: f"batch{s}")
@pytest.mark.parametrize("name", list(FIX))
def test_restatement_matches_the_fixture(name, split):
    pred, truth, want = FIX[name]
    counts, sums = sc.state_numpy(pred, truth, split)
    lines = []
    bad = sc.check_figures(name, sc.finish_numpy(counts, sums), pred, truth, want, lines)
    print("\n".join(lines))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", list(FIX))
def test_counts_do_not_depend_on_the_split(name):
    pred, truth, _ = FIX[name]
    whole = sc.state_numpy(pred, truth, None)[0]
    for split in sc.SPLITS[1:]:
        assert (sc.state_numpy(pred, truth, split)[0] == whole).all(), split
    n = pred.size
    assert whole[0] == n and whole[4:8].sum() == n and whole[8:12].sum() == whole[1] and whole[12] == (np.abs(truth) > 2).sum()


def test_half_to_even_and_the_two_clips():
    # 0.5 -> 0, 1.5 -> 2, 2.5 -> 2; 3.5 clips to 3 (Acc-7) and 2 (Acc-5); 2.7 rounds to 3 under the first clip and clips to 2 under the second
    p = np.array([0.5, 1.5, 2.5, 3.5, 2.7, -2.5], np.float32)
    c7, _ = sc.state_numpy(p, np.array([0, 2, 2, 3, 3, -2], np.float32))
    assert c7[2] == 6
    c5, _ = sc.state_numpy(p, np.array([0, 2, 2, 2, 2, -2], np.float32))
    assert c5[3] == 6
    c, _ = sc.state_numpy(p, np.array([1, 1, 3, 2, 2, -3], np.float32))
    assert c[2] == 0


def test_no_nonzero_truth_gives_nan_by_definition():
    c, s = sc.state_numpy(np.array([0.3, -0.2], np.float32), np.zeros(2, np.float32))
    f = sc.finish_numpy(c, s)
    assert np.isnan(f["acc2_non0"]) and np.isnan(f["f1_non0"]) and f["acc2"] == 0.5


# ------------------------------------------------------------------------------------------------ rules
@pytest.mark.parametrize("kw,rule", sc.REFUSED, ids=[f"{r}-{i}" for i, (_, r) in enumerate(sc.REFUSED)])
def test_each_refusal_by_name_and_text(kw, rule):
    kw = dict(dict(task="sentiment"), **kw)
    hit = step_rules.task_verdict(**kw)
    assert hit is not None and hit[0] == rule
    text = dict(step_rules.SENTI_RULES)[rule].format(**hit[1])
    with pytest.raises(_lib.MMDAError) as e:
        step_rules.task_check(**kw)
    assert str(e.value) == text
    if rule != "task_name":
        assert "sentiment" in text or "senti_loss" in text


@pytest.mark.parametrize("kw", sc.ALLOWED, ids=[str(i) for i in range(len(sc.ALLOWED))])
def test_nothing_else_is_refused(kw):
    assert step_rules.task_verdict("sentiment", **kw) is None
    step_rules.task_check("sentiment", **kw)


def test_emotion_task_looks_at_nothing_but_its_name():
    # today's behaviour: every combination the classifier allows stays allowed
    assert step_rules.task_verdict("emotion", senti_loss="huber", num_classes=6, use_confidNet=True, pos_weight=[1.0] * 6, focal_gamma=2.0,
                                   calibrate="per_class", select_by="map", rank=True) is None
    assert step_rules.task_verdict() is None


def test_rules_table_is_complete_and_ordered():
    names = [n for n, _ in step_rules.SENTI_RULES]
    assert len(set(names)) == len(names)
    assert set(r for _, r in sc.REFUSED) == set(names)
    # the first rule that applies is the one raised
    assert step_rules.task_verdict("sentiment", senti_loss="huber", num_classes=6, use_confidNet=True)[0] == "senti_loss"
    assert step_rules.task_verdict("sentiment", num_classes=6, use_confidNet=True)[0] == "senti_classes"
    # the step rules know nothing of the task: it combines with every step form
    assert not any("sentiment" in t for _, t in step_rules.RULES)


# ------------------------------------------------------------------------------------------------ configuration
def test_config_defaults_are_todays_behaviour(monkeypatch):
    assert DEFAULTS["task"] == "emotion" and DEFAULTS["senti_loss"] == "l1"
    monkeypatch.setattr(sys, "argv", ["train.py"])
    cfg = get_config(parse=True)
    assert cfg.task == "emotion" and cfg.senti_loss == "l1" and cfg.num_classes == 6
    assert make_config().task == "emotion"


def test_config_parses_the_two_flags(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["train.py", "--task", "sentiment", "--senti_loss", "mse", "--num_classes", "1"])
    cfg = get_config(parse=True)
    assert (cfg.task, cfg.senti_loss, cfg.num_classes) == ("sentiment", "mse", 1)
    for bad in (["--task", "regression"], ["--senti_loss", "huber"]):
        monkeypatch.setattr(sys, "argv", ["train.py"] + bad)
        with pytest.raises(SystemExit):
            get_config(parse=True)


def test_binding_constants():
    assert _lib.TASK == {"emotion": 0, "sentiment": 1} and _lib.SENTI_LOSS == {"l1": 0, "mse": 1}
    assert (_lib.SENTI_STATE_WORDS, _lib.SENTI_FIGURES) == (sc.WORDS, len(sc.FIGURES))
    for name in ("mmda_misa_set_task", "mmda_heads_fwd_task", "mmda_heads_bwd_task", "mmda_loss_reg", "mmda_senti_accumulate",
                 "mmda_senti_finish"):
        assert name in _lib.SIGNATURES


# ------------------------------------------------------------------------------------------------ criterion restatement vs torch
@pytest.mark.parametrize("kind", sc.KINDS)
@pytest.mark.parametrize("dtype", (torch.float32, torch.float64))
@pytest.mark.parametrize("B", sc.OP_BATCHES)
def test_criterion_restatement_is_torchs(B, dtype, kind):
    z, y = sc.op_inputs(B, 0)
    s = z[:, 6:].to(dtype).clone()
    s[::3, 0] = y[::3].to(dtype)                                   # s == y exactly: sign(0) = 0
    s.requires_grad_(True)
    fn = torch.nn.functional.l1_loss if kind == "l1" else torch.nn.functional.mse_loss
    ref = fn(s.reshape(-1), y.to(dtype), reduction="mean")
    (g,) = torch.autograd.grad(ref, s)
    tol = 4 * torch.finfo(dtype).eps
    assert abs(float(sc.reg_value(s.detach(), y, kind)) - float(ref.detach())) <= tol * max(1.0, abs(float(ref.detach())))
    mine = sc.reg_grad(s.detach(), y, kind)
    if kind == "l1":
        assert torch.equal(mine, g)                                # +-1/B or 0, bit for bit
        one = float(torch.tensor(1.0, dtype=dtype) / B)
        assert (mine[::3] == 0).all() and set(mine.unique().tolist()) <= {-one, 0.0, one}
    else:
        assert (mine - g).abs().max() <= tol * g.abs().max().clamp(min=1.0)
        assert (mine[::3] == 0).all()
    assert torch.equal(sc.reg_grad(s.detach(), y, kind, scale=0.5), 0.5 * mine)


def test_head_restatement_has_no_sigmoid():
    z, _ = sc.op_inputs(5, 1)
    z = z.double().requires_grad_(True)
    mask = torch.tensor([[2.0], [0.0], [2.0], [2.0], [0.0]], dtype=torch.float64)
    tcp, s, lab = sc.head_fwd(z, mask, 0.35)
    assert torch.equal(s, z[:, 6:] * mask) and torch.equal(lab, (s > 0.35).double())
    g = torch.Generator().manual_seed(3)
    dt, ds = torch.randn(5, 6, dtype=torch.float64, generator=g), torch.randn(5, 1, dtype=torch.float64, generator=g)
    (gz,) = torch.autograd.grad((tcp * dt).sum() + (s * ds).sum(), z)
    assert torch.allclose(sc.head_bwd(tcp.detach(), mask, dt, ds), gz, rtol=1e-14, atol=0)
