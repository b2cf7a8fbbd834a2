"""CPU: the class-weighted / focal classification criterion without a launch -- the float64 restatement the device tests compare with
(tests/cls_loss_cases.py), the two config fields and their flags, every refusal by name and by error code, and class_pos_weight on host
tensors."""
import ctypes
import math
import os
import subprocess
import sys
import tempfile
import textwrap

import pytest
import torch
import torch.nn.functional as TF

import cls_loss_cases as cc
from mmda_amd import MISA, _lib, class_pos_weight, get_config, make_config, step_rules
from mmda_amd.solver import Solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("B", (1, 5, 33))
def test_restatement_is_bce_at_the_defaults_and_the_weight_form_at_gamma_0(B):
    s, y = cc.inputs(B, 6, "-cpu")
    s = s.double()
    plain = sum(TF.binary_cross_entropy(s[:, c], y[:, c].double()) for c in range(6))
    assert abs(float(cc.value(s, y)) - float(plain)) <= 1e-14 * abs(float(plain))
    assert abs(float(cc.value(s, y, [1.0] * 6, 0.0)) - float(plain)) <= 1e-14 * abs(float(plain))
    w = torch.tensor(cc.WEIGHTS, dtype=torch.float64)
    yd = y.double()
    weighted = sum(TF.binary_cross_entropy(s[:, c], yd[:, c], weight=yd[:, c] * w[c] + (1 - yd[:, c])) for c in range(6))
    assert abs(float(cc.value(s, y, cc.WEIGHTS, 0.0)) - float(weighted)) <= 1e-14 * abs(float(weighted))
    # the plain gradient: torch's (s - y) / max(s (1 - s), 1e-12) / B
    g = cc.grad_closed(s, y)
    assert torch.allclose(g, (s - yd) / (s * (1 - s)).clamp(min=1e-12) / B, rtol=1e-13, atol=0)


@pytest.mark.parametrize("g", cc.GAMMAS)
@pytest.mark.parametrize("B", (1, 5, 33))
def test_closed_form_gradient_is_autograd_of_the_unclamped_expression(B, g):
    s, y = cc.inputs(B, 6, "-cpu")
    for w in (None, cc.WEIGHTS):
        sd = s.double().requires_grad_(True)
        cc.value(sd, y, w, g, clamp=False).backward()
        closed = cc.grad_closed(s.double(), y, w, g)
        assert torch.allclose(closed, sd.grad, rtol=1e-12, atol=1e-15), (B, g, w)


def test_focal_form_at_unit_weights_and_saturated_scores_are_finite():
    s, y = cc.inputs(5, 6, "-cpu")
    sd, yd = s.double(), y.double()
    pt = torch.where(yd > 0, sd, 1 - sd)
    focal = (-(1 - pt) ** 2.0 * torch.log(pt)).mean(0).sum()
    assert abs(float(cc.value(sd, y, None, 2.0)) - float(focal)) <= 1e-14 * abs(float(focal))
    s0, y0 = cc.saturated()
    for g in cc.GAMMAS:
        for dtype in (torch.float32, torch.float64):
            assert math.isfinite(float(cc.value(s0.to(dtype), y0, cc.WEIGHTS, g)))
            assert torch.isfinite(cc.grad_closed(s0.to(dtype), y0, cc.WEIGHTS, g)).all()


# ------------------------------------------------------------------------------------------------ config, flags, model
def test_config_defaults_and_model_setting():
    cfg = make_config(vocab_size=32)
    assert cfg.pos_weight is None and cfg.focal_gamma == 0.0
    m = MISA(cfg)
    assert m.cls_loss == dict(pos_weight=None, focal_gamma=0.0)
    m2 = MISA(make_config(vocab_size=32, pos_weight=cc.WEIGHTS, focal_gamma=2))
    assert m2.cls_loss == dict(pos_weight=tuple(cc.WEIGHTS), focal_gamma=2.0)
    assert m2.set_cls_loss([1] * 6, 0.0) == dict(pos_weight=None, focal_gamma=0.0)          # all ones: passed down as none
    assert m2.set_cls_loss([1] * 6, 2.0) == dict(pos_weight=None, focal_gamma=2.0)
    assert m2.set_cls_loss() == dict(pos_weight=None, focal_gamma=0.0)
    bal = MISA(make_config(vocab_size=32, pos_weight="balanced", focal_gamma=1.0))            # resolved by Solver.build()
    assert bal.cls_loss == dict(pos_weight=None, focal_gamma=1.0)
    with pytest.raises(ValueError, match="pos_weight"):
        MISA(make_config(vocab_size=32, pos_weight="inverse"))


def test_cli_flags(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["prog", "--pos_weight", "[1, 4, 4, 11, 5, 9]", "--focal_gamma", "2"])
    cfg = get_config()
    assert cfg.pos_weight == [1.0, 4.0, 4.0, 11.0, 5.0, 9.0] and cfg.focal_gamma == 2.0
    monkeypatch.setattr(sys, "argv", ["prog", "--pos_weight", "balanced"])
    cfg = get_config()
    assert cfg.pos_weight == "balanced" and cfg.focal_gamma == 0.0
    monkeypatch.setattr(sys, "argv", ["prog"])
    cfg = get_config()
    assert cfg.pos_weight is None and cfg.focal_gamma == 0.0
    for bad in ("[1, \"a\"]", "{\"a\": 1}", "heavy"):
        monkeypatch.setattr(sys, "argv", ["prog", "--pos_weight", bad])
        with pytest.raises(SystemExit):
            get_config()


# ------------------------------------------------------------------------------------------------ refusals
REFUSED = [("cls_gamma", dict(focal_gamma=0.5)), ("cls_gamma", dict(focal_gamma=9)), ("cls_gamma", dict(focal_gamma=float("nan"))),
           ("cls_gamma", dict(focal_gamma=-1.0)),
           ("cls_weight_value", dict(pos_weight=[1, 1, 1, 1, 1, -0.5])), ("cls_weight_value", dict(pos_weight=[1, float("nan"), 1, 1, 1, 1])),
           ("cls_weight_value", dict(pos_weight=[1, 1, float("inf"), 1, 1, 1])),
           ("cls_weight_count", dict(pos_weight=[1, 2, 3])), ("cls_weight_count", dict(pos_weight=[1] * 7))]


@pytest.mark.parametrize("rule, kw", REFUSED, ids=[f"{r}-{i}" for i, (r, _) in enumerate(REFUSED)])
def test_every_refusal_is_raised_by_name_and_changes_nothing(rule, kw):
    assert step_rules.cls_verdict(kw.get("pos_weight"), kw.get("focal_gamma", 0.0), 6)[0] == rule
    m = MISA(make_config(vocab_size=32, pos_weight=cc.WEIGHTS, focal_gamma=2.0))
    before = dict(m.cls_loss)
    with pytest.raises(_lib.MMDAError) as e:
        m.set_cls_loss(**kw)
    hit = step_rules.cls_verdict(kw.get("pos_weight"), kw.get("focal_gamma", 0.0), 6)
    assert str(e.value) == dict(step_rules.CLS_RULES)[rule].format(**hit[1])
    assert m.cls_loss == before
    with pytest.raises(_lib.MMDAError):
        MISA(make_config(vocab_size=32, **kw))


def test_more_than_sixteen_classes_take_no_weights():
    assert step_rules.cls_verdict([1.0] * 17, 0.0, 17)[0] == "cls_weight_classes"
    assert step_rules.cls_verdict(None, 2.0, 17) is None
    with pytest.raises(_lib.MMDAError, match="16 classes"):
        step_rules.cls_setting([2.0] * 17, 0.0, 17)
    assert [n for n, _ in step_rules.CLS_RULES] == ["cls_gamma", "cls_weight_count", "cls_weight_classes", "cls_weight_value"]
    assert step_rules.cls_setting([1.0] * 6, 0.0, 6) == (None, 0.0)
    assert step_rules.cls_setting((2.0, 1, 1, 1, 1, 1), 1, 6) == ((2.0, 1.0, 1.0, 1.0, 1.0, 1.0), 1.0)


def _opts(g=0.0, w=()):
    return _lib.ClsOpts(focal_gamma=g, n_weights=len(w), pos_weight=(ctypes.c_float * 16)(*w))


def test_native_error_codes_without_gpu():
    """mmda_misa_set_cls_loss keeps numbers only: no device is needed.  The op entries refuse in front of their launch."""
    lib = _lib.load()
    model, model17 = MISA(make_config(vocab_size=32)), MISA(make_config(vocab_size=32, num_classes=17))     # (kept: they own the handles)
    h, h17 = model._h, model17._h
    assert lib.mmda_misa_set_cls_loss(None, ctypes.byref(_opts())) == EINVAL
    for bad in (_opts(0.5), _opts(9.0), _opts(float("nan")), _opts(-1.0), _opts(0.0, [1, 1, 1, 1, 1, -1.0]),
                _opts(0.0, [1, 1, 1, float("nan"), 1, 1]), _opts(0.0, [1, 1, 1, 1, 1, float("inf")]), _opts(2.0, [1, 2, 3]),
                _opts(0.0, [1.0] * 7)):
        assert lib.mmda_misa_set_cls_loss(h, ctypes.byref(bad)) == EINVAL
    wide = _lib.ClsOpts(focal_gamma=0.0, n_weights=17)
    assert lib.mmda_misa_set_cls_loss(h17, ctypes.byref(wide)) == EINVAL                  # ncls = 17 with weights
    assert lib.mmda_misa_set_cls_loss(h17, ctypes.byref(_opts(2.0))) == 0                   # ... without: any class count
    for ok in (_opts(), _opts(1.0), _opts(8.0), _opts(3.5, cc.WEIGHTS), _opts(0.0, [0.0] * 6)):
        assert lib.mmda_misa_set_cls_loss(h, ctypes.byref(ok)) == 0
    assert lib.mmda_misa_set_cls_loss(h, None) == 0                                         # NULL: the plain criterion
    p = 1 << 20
    assert lib.mmda_loss_cls_opts(p, p, 4, 6, 1.0, p, p, ctypes.byref(_opts(0.5)), None) == EINVAL
    assert lib.mmda_loss_cls_opts(p, p, 4, 6, 1.0, p, p, ctypes.byref(_opts(2.0, [1, 2])), None) == EINVAL
    assert lib.mmda_loss_cls_opts(None, p, 4, 6, 1.0, p, p, None, None) == EINVAL
    assert lib.mmda_loss_misc_opts(p, p, p, 4, 6, p, p, 1, 1, 1.0, p, p, 8, 1.0, p, p, p, 0.3, 0.7, 0.7, 0.3, 0,
                                   ctypes.byref(_opts(9.0)), None) == EINVAL
    assert lib.mmda_label_counts(None, 4, 6, p, None) == EINVAL
    assert lib.mmda_label_counts(p, 4, 6, None, None) == EINVAL
    assert lib.mmda_label_counts(p, 4, 17, p, None) == EINVAL
    assert lib.mmda_label_counts(p, 4, 0, p, None) == EINVAL
    assert lib.mmda_label_counts(p, -1, 6, p, None) == EINVAL
    assert lib.mmda_label_counts(p, 4, 6, p + 4, None) == EINVAL                           # 64-bit counts
    assert lib.mmda_label_counts(p, 0, 6, p, None) == 0                                    # nothing to count: no launch


def test_cls_opts_size_matches_c_layout():
    code = textwrap.dedent("""
        #include <stdio.h>
        #include <stddef.h>
        #include "mmda_hip.h"
        int main(){printf("%zu %zu %zu\\n", sizeof(mmda_cls_opts), offsetof(mmda_cls_opts, n_weights), offsetof(mmda_cls_opts, pos_weight));
                   return 0;}""")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(code)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")], check=True)
        out = subprocess.run([os.path.join(d, "s")], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out] == [ctypes.sizeof(_lib.ClsOpts), _lib.ClsOpts.n_weights.offset, _lib.ClsOpts.pos_weight.offset]


# ------------------------------------------------------------------------------------------------ class_pos_weight
def test_class_pos_weight_on_cpu_tensors():
    y = torch.zeros(10, 4)
    y[:5, 0] = 1.0              # 5 of 10 -> 1
    y[:1, 1] = 1.0              # 1 of 10 -> 9
    y[:, 2] = 0.7               # every row (an entry counts when > 0) -> 0
    w = class_pos_weight(y)     # class 3: no positive -> 1
    assert w.dtype == torch.float64 and w.tolist() == [1.0, 9.0, 0.0, 1.0]
    assert class_pos_weight(y, cap=4.0).tolist() == [1.0, 4.0, 0.0, 1.0]
    y[0, 3] = -1.0                                                       # not > 0
    assert class_pos_weight(y).tolist()[3] == 1.0
    assert class_pos_weight(torch.ones(3, 1)).tolist() == [0.0]
    with pytest.raises(ValueError):
        class_pos_weight(torch.zeros(4))
    with pytest.raises(ValueError):
        class_pos_weight(y, cap=0.0)


def test_solver_resolves_balanced_from_a_host_dataset():
    """(a loader that is not device-resident: one host pass over loader.dataset's labels; the samples are the reference's triples)"""
    import numpy as np

    class Loader(list):
        pass

    lab = np.zeros((8, 1, 7), dtype=np.float32)
    lab[:4, 0, 1] = 1.0          # class 0: 4 of 8 -> 1
    lab[:2, 0, 2] = 2.0          # class 1: 2 of 8 -> 3
    lab[:, 0, 0] = 5.0           # the sentiment column is not a class
    loader = Loader()
    loader.dataset = [((None, None, None, None), lab[i], f"seg{i}") for i in range(8)]
    cfg = make_config(vocab_size=32, pos_weight="balanced", focal_gamma=2.0, device="cpu")
    s = Solver(cfg, cfg, cfg, loader, [], [], is_train=False, model=MISA(cfg)).build()
    assert s.cls_pos_weight == [1.0, 3.0, 1.0, 1.0, 1.0, 1.0]
    assert s.model.cls_loss == dict(pos_weight=(1.0, 3.0, 1.0, 1.0, 1.0, 1.0), focal_gamma=2.0)
    assert s._cls_setting() == s.model.cls_loss
    with pytest.raises(ValueError, match="balanced"):                     # nothing to resolve it from
        Solver(cfg, cfg, cfg, None, [], [], is_train=False, model=MISA(cfg)).build()
    plain = Solver(cfg, cfg, cfg, loader, [], [], is_train=False, model=MISA(make_config(vocab_size=32)))
    plain.train_config = make_config(vocab_size=32)
    assert plain.build().cls_pos_weight is None and plain.model.cls_loss == dict(pos_weight=None, focal_gamma=0.0)
