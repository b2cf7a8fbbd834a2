"""CPU: the optimizer settings that need no launch -- constructors, the param-group rule, the config names, the error codes of the new
entry points and the ctypes mirror of mmda_adam_opts."""
import ctypes
import os
import subprocess
import tempfile
import textwrap

import pytest
import torch

from mmda_amd import MISA, _lib, make_config, optim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def _params():
    return [torch.nn.Parameter(torch.zeros(4))]


def test_adam_takes_weight_decay_and_adamw_exists():
    a = optim.Adam(_params(), lr=1e-3, weight_decay=0.1)
    assert a.settings() == (0.9, 0.999, 1e-8, 0.1, False)
    assert a.defaults["weight_decay"] == 0.1 and a.defaults["decoupled_weight_decay"] is False
    d = optim.Adam(_params(), betas=(0.8, 0.95), eps=1e-6, weight_decay=0.2, decoupled_weight_decay=True)
    assert d.settings() == (0.8, 0.95, 1e-6, 0.2, True)
    w = optim.AdamW(_params())
    assert isinstance(w, optim.Adam)
    assert w.settings() == (0.9, 0.999, 1e-8, 1e-2, True)          # torch.optim.AdamW's defaults
    assert w.param_groups[0]["weight_decay"] == 1e-2 and w.param_groups[0]["decoupled_weight_decay"] is True
    assert optim.optimizer_dict["AdamW"] is optim.AdamW
    assert optim.optimizer_dict["Adam"] is optim.Adam and optim.optimizer_dict["RMSprop"] is optim.RMSprop
    plain = optim.Adam(_params())
    assert plain.settings() == (0.9, 0.999, 1e-8, 0.0, False)


def test_bad_settings_are_refused_at_construction():
    for kw in (dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)), dict(eps=-1.0), dict(weight_decay=-0.1)):
        with pytest.raises(ValueError):
            optim.Adam(_params(), **kw)


def test_rmsprop_still_refuses_what_it_does_not_do():
    for kw in (dict(weight_decay=0.1), dict(momentum=0.9), dict(centered=True)):
        with pytest.raises(NotImplementedError):
            optim.RMSprop(_params(), **kw)


def test_config_resolves_adamw_and_carries_the_new_fields():
    cfg = make_config(optimizer="AdamW", vocab_size=32)
    assert cfg.optimizer is optim.AdamW
    assert cfg.optimizer_kwargs == {} and cfg.clip_norm is None
    cfg2 = make_config(vocab_size=32, optimizer_kwargs=dict(betas=(0.9, 0.98)), clip_norm=1.0)
    assert cfg2.optimizer is optim.Adam and cfg2.optimizer_kwargs["betas"] == (0.9, 0.98) and cfg2.clip_norm == 1.0
    assert make_config(vocab_size=32).optimizer_kwargs is not cfg.optimizer_kwargs       # (no shared default dict)


def test_second_param_group_on_an_attached_optimizer_raises_by_name():
    model = MISA(make_config(vocab_size=32))
    ps = list(model.parameters())
    opt = optim.AdamW(ps[:3], lr=1e-3).attach(model)
    with pytest.raises(_lib.MMDAError, match="param group"):
        opt.add_param_group(dict(params=ps[3:5], weight_decay=0.0))
    assert len(opt.param_groups) == 1
    two = optim.Adam([dict(params=ps[:3]), dict(params=ps[3:5], weight_decay=0.0)], lr=1e-3, weight_decay=0.1)
    two.attach(model)
    with pytest.raises(_lib.MMDAError, match="param group"):
        two.settings()
    # not attached: torch's rule, any number of groups
    free = optim.Adam([dict(params=ps[:3]), dict(params=ps[3:5])], lr=1e-3)
    free.add_param_group(dict(params=ps[5:6]))
    assert len(free.param_groups) == 3


def test_model_refuses_settings_by_name_before_anything_runs():
    """(the refusals that need no device: they are raised before the batch is looked at)"""
    model = MISA(make_config(vocab_size=32, embed_update="sparse"))
    opt = optim.Adam(list(model.parameters()), lr=1e-3).attach(model)
    with pytest.raises(_lib.MMDAError, match="clip_norm"):
        model._push_adam(opt, 1.0)
    with pytest.raises(_lib.MMDAError, match="clip_norm"):
        model._push_adam(opt, -1.0)
    dense = MISA(make_config(vocab_size=32))
    with pytest.raises(_lib.MMDAError, match="gradient exchange"):
        dense._push_adam(None, 1.0, exchange=True)
    rms = optim.RMSprop(list(dense.parameters()), lr=1e-3).attach(dense)
    with pytest.raises(_lib.MMDAError, match="RMSprop"):
        dense._push_adam(rms, 1.0)
    assert dense._adam_pushed == (0.9, 0.999, 1e-8, 0.0, False, 0.0)
    # what is allowed reaches the handle (no device needed: the handle only keeps the numbers)
    w = optim.AdamW(list(dense.parameters()), lr=1e-3, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.1).attach(dense)
    assert dense._push_adam(w, 2.0) == (0.8, 0.95, 1e-6, 0.1, True, 2.0)
    assert dense._adam_pushed == (0.8, 0.95, 1e-6, 0.1, True, 2.0)
    assert dense._push_adam(None, None) == (0.9, 0.999, 1e-8, 0.0, False, 0.0)


def _opts(**kw):
    d = dict(beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, decoupled=0, scale_dev=None)
    d.update(kw)
    return _lib.AdamOpts(**d)


BAD_OPTS = (dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.0), dict(beta2=-1e-3), dict(eps=-1e-8), dict(weight_decay=-0.1),
            dict(beta1=float("nan")))


def test_set_adam_error_codes_without_gpu():
    lib = _lib.load()
    model = MISA(make_config(vocab_size=32))
    h = model._h
    assert lib.mmda_misa_set_adam(None, ctypes.byref(_opts()), 0.0) == EINVAL
    for bad in BAD_OPTS:
        assert lib.mmda_misa_set_adam(h, ctypes.byref(_opts(**bad)), 0.0) == EINVAL, bad
    assert lib.mmda_misa_set_adam(h, ctypes.byref(_opts()), -1.0) == EINVAL
    assert lib.mmda_misa_set_adam(h, ctypes.byref(_opts()), float("nan")) == EINVAL
    assert lib.mmda_misa_set_adam(h, ctypes.byref(_opts(beta1=0.0, beta2=0.0, eps=0.0, weight_decay=0.5, decoupled=1)), 3.0) == 0
    assert lib.mmda_misa_set_adam(h, None, 0.0) == 0                   # NULL: the defaults


def test_op_entries_error_codes_without_gpu():
    """NULL or bad arguments are MMDA_EINVAL in front of any launch (the pointers are never dereferenced: no device is needed)."""
    lib = _lib.load()
    p = 1 << 20                                                       # a 16-byte aligned "pointer"
    ok = ctypes.byref(_opts())
    assert lib.mmda_clamp_adam_opts(p, None, p, p, p, 8, None, 0, 0, 1e-3, 1.0, 1.0, 1, None, None) == EINVAL           # no opts
    assert lib.mmda_clamp_adam_opts(None, None, p, p, p, 8, None, 0, 0, 1e-3, 1.0, 1.0, 1, ok, None) == EINVAL          # no p
    assert lib.mmda_clamp_adam_opts(p, None, p, p, p, 8, None, 0, 0, 1e-3, 1.0, 1.0, 0, ok, None) == EINVAL             # step 0
    assert lib.mmda_clamp_adam_opts(p, None, p, p, p, -1, None, 0, 0, 1e-3, 1.0, 1.0, 1, ok, None) == EINVAL            # n < 0
    assert lib.mmda_clamp_adam_opts(p + 4, None, p, p, p, 8, None, 0, 0, 1e-3, 1.0, 1.0, 1, ok, None) == EINVAL         # alignment
    assert lib.mmda_clamp_adam_opts(p, None, p, p, p, 0, None, 2, 5, 1e-3, 1.0, 1.0, 1, ok, None) == EINVAL             # runs missing
    for bad in BAD_OPTS:
        assert lib.mmda_clamp_adam_opts(p, None, p, p, p, 8, None, 0, 0, 1e-3, 1.0, 1.0, 1, ctypes.byref(_opts(**bad)), None) == EINVAL
        assert lib.mmda_clamp_adam_rows_opts(p, p, p, p, 4, 8, p, 1, 1e-3, 1.0, 1.0, 1, ctypes.byref(_opts(**bad)), None) == EINVAL
    assert lib.mmda_clamp_adam_opts(p, None, p, p, p, 0, None, 0, 0, 1e-3, 1.0, 1.0, 1, ok, None) == 0                  # nothing to do
    assert lib.mmda_clamp_adam_rows_opts(p, p, p, p, 4, 8, p, 1, 1e-3, 1.0, 1.0, 1, None, None) == EINVAL
    assert lib.mmda_clamp_adam_rows_opts(p, p, p, p, 4, 8, None, 1, 1e-3, 1.0, 1.0, 1, ok, None) == EINVAL              # no mask
    assert lib.mmda_clamp_adam_rows_opts(p, p, p, p, 4, 0, p, 1, 1e-3, 1.0, 1.0, 1, ok, None) == EINVAL                 # dim 0
    assert lib.mmda_clamp_adam_rows_opts(p, p, p, p, 0, 8, p, 1, 1e-3, 1.0, 1.0, 1, ok, None) == 0

    assert lib.mmda_grad_norm_partials(-1) == EINVAL
    assert lib.mmda_grad_norm_partials(0) == 1 and lib.mmda_grad_norm_partials(1031) == 5
    assert lib.mmda_grad_norm_partials(2048 * 256 * 4 + 1031) == 2048 and lib.mmda_grad_norm_partials(1 << 62) == 2048
    assert lib.mmda_grad_norm(None, None, 8, None, 0, 0, 1.0, 1.0, p, 8, p, None) == EINVAL                             # no g
    assert lib.mmda_grad_norm(p, None, 8, None, 0, 0, 1.0, 1.0, None, 8, p, None) == EINVAL                             # no partials
    assert lib.mmda_grad_norm(p, None, 8, None, 0, 0, 1.0, 1.0, p, 8, None, None) == EINVAL                             # no out
    assert lib.mmda_grad_norm(p, None, 8, None, 0, 0, -1.0, 1.0, p, 8, p, None) == EINVAL                               # max_norm < 0
    assert lib.mmda_grad_norm(p, None, -8, None, 0, 0, 1.0, 1.0, p, 8, p, None) == EINVAL
    assert lib.mmda_grad_norm(p + 4, None, 8, None, 0, 0, 1.0, 1.0, p, 8, p, None) == EINVAL                            # alignment
    assert lib.mmda_grad_norm(p, None, 8, None, 0, 0, 1.0, 1.0, p + 4, 8, p, None) == EINVAL                            # doubles
    assert lib.mmda_grad_norm(p, None, 4096, None, 0, 0, 1.0, 1.0, p, 3, p, None) == EINVAL                             # 4 blocks, room for 3
    assert lib.mmda_grad_norm(p, None, 0, None, 2, 5, 1.0, 1.0, p, 8, p, None) == EINVAL                                # runs missing
    assert lib.mmda_grad_scale(None, 8, None, 0, 0, p, None) == EINVAL
    assert lib.mmda_grad_scale(p, 8, None, 0, 0, None, None) == EINVAL
    assert lib.mmda_grad_scale(p, -1, None, 0, 0, p, None) == EINVAL
    assert lib.mmda_grad_scale(p + 4, 8, None, 0, 0, p, None) == EINVAL
    assert lib.mmda_grad_scale(p, 0, None, 2, 5, p, None) == EINVAL
    assert lib.mmda_grad_scale(p, 0, None, 0, 0, p, None) == 0


def test_adam_opts_size_matches_c_layout():
    code = textwrap.dedent("""
        #include <stdio.h>
        #include <stddef.h>
        #include "mmda_hip.h"
        int main(){printf("%zu %zu %zu\\n", sizeof(mmda_adam_opts), offsetof(mmda_adam_opts, decoupled), offsetof(mmda_adam_opts, scale_dev));
                   return 0;}""")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(code)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")], check=True)
        out = subprocess.run([os.path.join(d, "s")], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out] == [ctypes.sizeof(_lib.AdamOpts), _lib.AdamOpts.decoupled.offset, _lib.AdamOpts.scale_dev.offset]
