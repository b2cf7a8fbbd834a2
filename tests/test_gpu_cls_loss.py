"""MI355X: the class-weighted / focal classification criterion (mmda_amd/csrc/loss_terms.h) at its three device sites --
mmda_loss_cls_opts, role 0 of mmda_loss_misc_opts and the seed the forward stretch stores -- against the float64 restatement of
tests/cls_loss_cases.py, bit identity with the plain criterion and between step forms, mmda_label_counts, and Solver with
pos_weight="balanced".

Op-level bound: 8 x the error of the float32 CPU restatement on the same inputs (cls_loss_cases.py); every figure is printed before
it is asserted.  With MMDA_CLS_LOSS_RATIOS_OUT set to a path, the measured kernel error / e32 of every row is written there as JSON
(tests/golden/cls_loss_error_ratios.json is such a run)."""
import ctypes as C
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cls_loss_cases as cc
from golden_util import SIDE, batch_of, load_case
from model_compare import rel
from mmda_amd import _lib
from mmda_amd.utils import functions as F
from oracle import misa_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _ratios_file():
    yield
    path = os.environ.get("MMDA_CLS_LOSS_RATIOS_OUT")
    if path:
        with open(path, "w") as f:
            json.dump(RATIOS, f, indent=0, sort_keys=True)


def _opts(w, g):
    return _lib.cls_opts(None if w is None else tuple(w), float(g))


def _assert_ok(name, got, ref32):
    bad = cc.check(name, got, ref32, RATIOS.setdefault(name, {}))
    assert not bad, "\n".join(bad)


def _settings(ncls):
    return [(w, g) for g in cc.GAMMAS for w in (None, cc.weights_for(ncls))]


def _tag(w, g):
    return f"g{g}-{'w' if w is not None else 'nw'}"


# ------------------------------------------------------------------------------------------------ mmda_loss_cls_opts
@pytest.mark.parametrize("B, ncls", cc.SHAPES, ids=[f"B{B}-n{n}" for B, n in cc.SHAPES])
def test_loss_cls_opts_against_float64(B, ncls):
    """value + gradient into a cleared buffer; gradient alone (loss = NULL) at scale 0.3 onto a pre-filled buffer; value alone"""
    lib = _lib.load()
    s, y = cc.inputs(B, ncls)
    sd, yd = s.to(DEV), y.to(DEV)
    pre = cc.prefill(B, ncls)
    st = _lib.stream_ptr()
    for w, g in _settings(ncls):
        o = _opts(w, g)
        name = f"cls-B{B}-n{ncls}-{_tag(w, g)}"
        loss = torch.zeros((), device=DEV); ds = torch.zeros(B, ncls, device=DEV)
        assert lib.mmda_loss_cls_opts(sd.data_ptr(), yd.data_ptr(), B, ncls, 1.0, loss.data_ptr(), ds.data_ptr(), o, st) == 0
        _assert_ok(name, cc.errors(loss.cpu(), ds, s, y, w, g), cc.e32(s, y, w, g))
        ds2 = pre.to(DEV)
        assert lib.mmda_loss_cls_opts(sd.data_ptr(), yd.data_ptr(), B, ncls, 0.3, None, ds2.data_ptr(), o, st) == 0
        _assert_ok(name + "-prefill", cc.errors(None, ds2, s, y, w, g, 0.3, pre), cc.e32(s, y, w, g, 0.3, pre, want_value=False))
        loss3 = torch.zeros((), device=DEV)
        assert lib.mmda_loss_cls_opts(sd.data_ptr(), yd.data_ptr(), B, ncls, 1.0, loss3.data_ptr(), None, o, st) == 0
        _assert_ok(name + "-no_ds", cc.errors(loss3.cpu(), None, s, y, w, g), cc.e32(s, y, w, g, want_grad=False))
        assert torch.equal(loss3.cpu(), loss.cpu())                               # (the value does not depend on the gradient's presence)


# ------------------------------------------------------------------------------------------------ role 0 of mmda_loss_misc_opts
def _misc(lib, sd, td, yd, B, ncls, d_scores, with_conf, o):
    """the launch with a small recon part, conf computed (with_conf) but seeding nothing: d_scores receives the classification term only"""
    L = torch.zeros(8, device=DEV)
    L[1], L[2] = 0.37, 1.21
    rec = torch.arange(8, dtype=torch.float32, device=DEV) / 8.0
    org = torch.zeros(8, device=DEV)
    d_tcp = torch.zeros(B, ncls, device=DEV) if d_scores is not None else None
    rc = lib.mmda_loss_misc_opts(sd.data_ptr(), td.data_ptr(), yd.data_ptr(), B, ncls, _lib.ptr(d_scores), _lib.ptr(d_tcp), with_conf, 0, 0.9,
                                 rec.data_ptr(), org.data_ptr(), 8, 0.6, None, None, L.data_ptr(), 0.3, 0.8, 0.6, 0.9, 0, o, _lib.stream_ptr())
    assert rc == 0
    if d_tcp is not None:
        assert float(d_tcp.abs().max()) == 0.0
    return L.cpu()


@pytest.mark.parametrize("B, ncls", cc.SHAPES, ids=[f"B{B}-n{n}" for B, n in cc.SHAPES])
def test_loss_misc_opts_role_0_against_float64(B, ncls):
    lib = _lib.load()
    s, y = cc.inputs(B, ncls)
    t = torch.sigmoid(torch.randn(B, ncls, generator=torch.Generator().manual_seed(B)))
    sd, td, yd = s.to(DEV), t.to(DEV), y.to(DEV)
    pre = cc.prefill(B, ncls)
    recon = float((torch.arange(8, dtype=torch.float64) / 8.0).pow(2).mean())
    for w, g in _settings(ncls):
        o = _opts(w, g)
        for with_conf in ((0, 1) if ncls == 6 else (0,)):
            name = f"misc-B{B}-n{ncls}-{_tag(w, g)}-c{with_conf}"
            ds = pre.to(DEV)
            L = _misc(lib, sd, td, yd, B, ncls, ds, with_conf, o)
            _assert_ok(name, cc.errors(L[0], ds, s, y, w, g, 1.0, pre), cc.e32(s, y, w, g, 1.0, pre))
            # the weighted total of the same launch: cls + 0.3 L1 + 0.8 L2 + 0.6 recon (use_conf = 0), to float32 rounding of the sum
            want = float(L[0]) + 0.3 * 0.37 + 0.8 * 1.21 + 0.6 * recon
            assert abs(float(L[5]) - want) <= 1e-6 * abs(want), (name, float(L[5]), want)
        L = _misc(lib, sd, td, yd, B, ncls, None, 0, o)
        _assert_ok(f"misc-B{B}-n{ncls}-{_tag(w, g)}-no_ds", cc.errors(L[0], None, s, y, w, g), cc.e32(s, y, w, g, want_grad=False))


# ------------------------------------------------------------------------------------------------ saturated scores
@pytest.mark.parametrize("g", cc.GAMMAS)
def test_saturated_scores_are_finite_and_equal_the_restatement(g):
    """scores exactly 0 and 1 against both labels: finite, the four saturated gradient elements equal to the float32 restatement's
    (their arithmetic is exact but for one division), value and the interior elements within the op-level bound"""
    lib = _lib.load()
    s, y = cc.saturated()
    w = cc.WEIGHTS
    sd, yd = s.to(DEV), y.to(DEV)
    td = torch.full((1, 6), 0.5, device=DEV)
    want32 = cc.grad_closed(s, y, w, g)
    for site in ("cls", "misc"):
        ds = torch.zeros(1, 6, device=DEV)
        if site == "cls":
            loss = torch.zeros((), device=DEV)
            assert lib.mmda_loss_cls_opts(sd.data_ptr(), yd.data_ptr(), 1, 6, 1.0, loss.data_ptr(), ds.data_ptr(), _opts(w, g),
                                          _lib.stream_ptr()) == 0
            val = loss.cpu()
        else:
            val = _misc(lib, sd, td, yd, 1, 6, ds, 0, _opts(w, g))[0]
        assert torch.isfinite(val).all() and torch.isfinite(ds).all()
        print(f"saturated {site} g={g}: value {float(val):.6f} grad {ds.cpu().tolist()} restatement {want32.tolist()}")
        assert torch.equal(ds.cpu()[:, :4], want32[:, :4]), (site, ds.cpu().tolist(), want32.tolist())
        _assert_ok(f"saturated-{site}-g{g}", cc.errors(val, ds, s, y, w, g), cc.e32(s, y, w, g))


# ------------------------------------------------------------------------------------------------ bit identity with the plain criterion
def test_unit_weights_and_gamma_0_are_the_plain_entry_points_bit_for_bit():
    from mmda_amd.utils.eval import DeviceEval
    lib = _lib.load()
    s, y = cc.inputs(43, 6)
    sd, yd = s.to(DEV), y.to(DEV)
    out = []
    for kw in ({}, dict(pos_weight=[1] * 6, focal_gamma=0.0)):
        gs = sd.clone().requires_grad_(True)
        v = F.bce_sum_over_classes(gs, yd, **kw)
        v.backward()
        ev = DeviceEval(6, torch.device(DEV))
        ev.add_cls_loss(sd, yd, **kw)
        out.append((v.detach().cpu(), gs.grad.cpu(), ev.loss_sum.cpu()))
    for a, b in zip(*out):
        assert torch.equal(a, b)
    assert torch.equal(out[0][0].reshape(1), out[0][2])
    # ... and differ from a criterion that is on
    assert not torch.equal(F.bce_sum_over_classes(sd, yd, pos_weight=cc.WEIGHTS).cpu(), out[0][0])
    # the C ABI: a NULL mmda_cls_opts* and {0, 0} run mmda_loss_cls / mmda_loss_misc
    td = torch.sigmoid(torch.randn(43, 6)).to(DEV)
    plain_l = torch.zeros((), device=DEV); plain_d = torch.zeros(43, 6, device=DEV)
    assert lib.mmda_loss_cls(sd.data_ptr(), yd.data_ptr(), 43, 6, 0.7, plain_l.data_ptr(), plain_d.data_ptr(), _lib.stream_ptr()) == 0
    for o in (None, C.byref(_lib.ClsOpts())):
        l = torch.zeros((), device=DEV); d = torch.zeros(43, 6, device=DEV)
        assert lib.mmda_loss_cls_opts(sd.data_ptr(), yd.data_ptr(), 43, 6, 0.7, l.data_ptr(), d.data_ptr(), o, _lib.stream_ptr()) == 0
        assert torch.equal(l.cpu(), plain_l.cpu()) and torch.equal(d.cpu(), plain_d.cpu())
    L = torch.zeros(8, device=DEV); dsc = torch.zeros(43, 6, device=DEV); dt = torch.zeros(43, 6, device=DEV)
    rec = torch.randn(8).to(DEV); org = torch.randn(8).to(DEV)
    assert lib.mmda_loss_misc(sd.data_ptr(), td.data_ptr(), yd.data_ptr(), 43, 6, dsc.data_ptr(), dt.data_ptr(), 1, 0, 0.9, rec.data_ptr(),
                              org.data_ptr(), 8, 0.6, None, None, L.data_ptr(), 0.3, 0.8, 0.6, 0.9, 0, _lib.stream_ptr()) == 0
    ds2 = torch.zeros(43, 6, device=DEV)
    L2 = _misc_plain_again(lib, sd, td, yd, ds2, rec, org)
    assert torch.equal(L.cpu()[:6], L2[:6]) and torch.equal(dsc.cpu(), ds2.cpu())


def _misc_plain_again(lib, sd, td, yd, ds, rec, org):
    L = torch.zeros(8, device=DEV); dt = torch.zeros(43, 6, device=DEV)
    assert lib.mmda_loss_misc_opts(sd.data_ptr(), td.data_ptr(), yd.data_ptr(), 43, 6, ds.data_ptr(), dt.data_ptr(), 1, 0, 0.9, rec.data_ptr(),
                                   org.data_ptr(), 8, 0.6, None, None, L.data_ptr(), 0.3, 0.8, 0.6, 0.9, 0, None, _lib.stream_ptr()) == 0
    return L.cpu()


def _fixture_model(name, precision, use_confidNet=None, **kw):
    from mmda_amd import MISA, make_config
    z, meta, cfg = load_case(name)
    if use_confidNet is not None:
        cfg = SimpleNamespace(**dict(vars(cfg), use_confidNet=use_confidNet))
    m = MISA(make_config(precision=precision, device=DEV, **kw, **vars(cfg)))
    P = orc.synth_params(cfg, meta["seed"])
    m.load_state_dict(P, strict=True)
    m.to(DEV)
    batch = batch_of(z)
    b = {k: (v.to(DEV) if k != "l" else v) for k, v in batch.items()}
    return m, cfg, P, batch, b, meta


@pytest.mark.parametrize("name", ["tiny_cmd_ragged", "real_b8_t12_ragged"])
def test_a_train_step_with_unit_weights_is_the_default_step_bit_for_bit(name):
    """(real_b8_t12_ragged: hidden 128, where the forward stretch stores the seed; the tiny fixture: the loss launch seeds)"""
    state = []
    for kw in ({}, dict(pos_weight=[1.0] * 6, focal_gamma=0.0)):
        m, cfg, P, batch, b, meta = _fixture_model(name, "fp32", **kw)
        m.train_step(b["t"], b["v"], b["a"], b["l"], b["emo"], lr=1e-3, clip=cfg.clip, training=False)
        torch.cuda.synchronize()
        state.append([x.detach().cpu().clone() for x in m.flat_buckets()] + [m._ws_view("losses", (8,)).cpu().clone()])
        assert not m.cluster_aborted()
    for x, y in zip(*state):
        assert torch.equal(x, y)
    assert not torch.equal(state[0][0], P_flat_start(name))


def P_flat_start(name):
    m, *_ = _fixture_model(name, "fp32")
    m._materialize(torch.device(DEV))
    return m.flat_buckets()[0].detach().cpu().clone()


# ------------------------------------------------------------------------------------------------ a train step against the oracle
W, G = cc.WEIGHTS, 2.0


def _oracle_step(P, cfg, batch, emulate=False):
    """oracle.loss_and_grads with the classification term swapped: total = L.total - L.cls + new_cls(o.scores, emo)"""
    leaves = {k: p.detach().clone().requires_grad_(True) for k, p in P.items()}
    for k in leaves:
        if k.endswith("activation.weight"):
            leaves[k] = leaves[orc.PRELU_KEY]
    if emulate:
        from oracle import bf16_emul as emu
        o = emu.forward(leaves, cfg, batch["t"], batch["v"], batch["a"], batch["l"], True, True)
    else:
        o = orc.forward(leaves, cfg, batch["t"], batch["v"], batch["a"], batch["l"])
    L = orc.all_losses(o, batch["emo"], cfg)
    new = cc.oracle_cls(o.scores, batch["emo"], W, G)
    L.total = L.total - L.cls + new
    L.cls = new
    L.total.backward()
    return o, L, {k: (None if p.grad is None else p.grad.detach()) for k, p in leaves.items()}


def _check_losses(m, L, tol):
    got = m.read_losses()
    for k in ("cls", "diff", "sim", "recon", "conf", "total"):
        ref = float(getattr(L, k).detach())
        print(f"loss {k}: step {got[k]:.8f} oracle {ref:.8f}")
        assert abs(got[k] - ref) < tol * abs(ref) + 1e-7, (k, got[k], ref)


@pytest.mark.parametrize("confid", [False, True], ids=["seed_fwd", "confidnet"])
@pytest.mark.parametrize("name", ["tiny_cmd_ragged", "real_b8_t12_ragged"])
def test_fp32_train_step_matches_autograd_through_the_oracle(name, confid):
    """tests/test_gpu_model.py's bounds for these fixtures: losses 1e-4, every gradient 2e-4 of its tensor's largest element; a
    gradient the oracle leaves None is exactly zero.  Without ConfidNet the forward stretch stores the seed (hidden 128: the real
    fixture; at the tiny fixture's hidden 16 the loss launch seeds it), with ConfidNet role 0 of the loss launch adds it atomically."""
    m, cfg, P, batch, b, meta = _fixture_model(name, "fp32", use_confidNet=confid, pos_weight=W, focal_gamma=G)
    assert m.cls_loss == dict(pos_weight=tuple(W), focal_gamma=G)
    m.train_step(b["t"], b["v"], b["a"], b["l"], b["emo"], lr=cfg.learning_rate, clip=cfg.clip, do_adam=False, training=False)
    assert not m.cluster_aborted()
    o, L, Gr = _oracle_step(P, cfg, batch)
    plain = float(orc.cls_loss(o.scores.detach(), batch["emo"]))
    assert abs(float(L.cls.detach()) - plain) > 1e-2 * plain                       # (the criterion is on: another number)
    pub = m._public()
    assert rel(pub["scores"], o.scores.detach()) < 1e-4 and rel(pub["tcp"], o.tcp.detach()) < 1e-4
    _check_losses(m, L, 1e-4)
    m._assign_grad_views()
    for k, p in m.named_parameters():
        if Gr[k] is None:
            assert float(p.grad.abs().max()) == 0.0, k
            continue
        g, ref = p.grad.cpu(), Gr[k]
        gmax = float(ref.abs().max())
        if k.endswith("self_attn.in_proj_bias"):                                    # (the key part is zero in exact arithmetic)
            hs = cfg.hidden_size
            keep = torch.ones(3 * hs, dtype=torch.bool); keep[hs:2 * hs] = False
            g, ref = g[keep], ref[keep]
        e = float((g - ref).abs().max() / max(gmax, 1e-6))
        assert e < 2e-4, f"{k}: rel err {e:.3e}"


def _bf16_step_against_the_emulating_oracle(name):
    """tests/test_gpu_model.py's bf16 bounds against the bf16-emulating oracle: outputs 1e-3, losses 1e-4, every gradient 1e-2 (L2)"""
    m, cfg, P, batch, b, meta = _fixture_model(name, "bf16", pos_weight=W, focal_gamma=G)
    m.train_step(b["t"], b["v"], b["a"], b["l"], b["emo"], lr=cfg.learning_rate, clip=cfg.clip, do_adam=False, training=False)
    assert not m.cluster_aborted()
    o, L, Gr = _oracle_step(P, cfg, batch, emulate=True)
    pub = m._public()
    assert rel(pub["scores"], o.scores.detach()) < 1e-3 and rel(pub["tcp"], o.tcp.detach()) < 1e-3
    for s_ in SIDE:
        assert rel(pub[s_], getattr(o, s_).detach()) < 1e-3, s_
    _check_losses(m, L, 1e-4)
    m._assign_grad_views()
    for k, p in m.named_parameters():
        if Gr[k] is None:
            assert float(p.grad.abs().max()) == 0.0, k
            continue
        g, ref = p.grad.cpu().double(), Gr[k].double()
        if k.endswith("self_attn.in_proj_bias"):
            hs = cfg.hidden_size
            keep = torch.ones(3 * hs, dtype=torch.bool); keep[hs:2 * hs] = False
            g, ref = g[keep], ref[keep]
        l2 = float((g - ref).norm() / ref.norm().clamp_min(1e-30))
        print(f"bf16 {name} {k}: relative L2 error {l2:.3e}")
        assert l2 <= 1e-2, f"{k}: relative L2 error vs the bf16-emulating oracle {l2:.3e}"


def test_bf16_train_step_matches_the_emulating_oracle_hidden_128():
    _bf16_step_against_the_emulating_oracle("real_b8_t12_ragged")


# ------------------------------------------------------------------------------------------------ bit equality between step forms
def _turn_on(*models):
    for m in models:
        m.set_cls_loss(W, G)


@pytest.mark.parametrize("confid", [False, True])
def test_encoded_step_equals_the_cut_step_under_the_criterion(confid):
    import test_gpu_encoded as enc
    a, cfg = enc._model("fp32", use_confidNet=confid)
    e, _ = enc._model("fp32", use_confidNet=confid)
    _turn_on(a, e)
    warm = orc.synth_batch(cfg, 8, 12, 60, ragged=True)
    for m in (a, e):
        enc._cut_step(m, warm, seed=900)
    # (it is the criterion's step: the plain one from the same state on the same batch reports another classification loss)
    p, _ = enc._model("fp32", use_confidNet=confid)
    enc._cut_step(p, warm, seed=900)
    assert p.read_losses()["cls"] != a.read_losses()["cls"] and p.read_losses()["diff"] == a.read_losses()["diff"]
    b = orc.synth_batch(cfg, 6, 9, 71, ragged=True)
    before = enc._state(e)
    eb = enc._encoded_batch(e, b)
    enc._cut_step(a, b, seed=1001)
    e.train_step_encoded(eb, lr=enc.LR, clip=enc.CLIP, seed=1001)
    enc._assert_same_step(a, e, before, 6, ("criterion", confid))
    assert not a.cluster_aborted() and not e.cluster_aborted()


def test_accumulated_step_equals_the_manual_mean_of_gradients_under_the_criterion():
    import test_gpu_accum as acc
    m, cfg = acc._model("fp32")
    twin, _ = acc._model("fp32")
    _turn_on(m, twin)
    batches = [orc.synth_batch(cfg, B, T, 50 + i, ragged=True) for i, (B, T) in enumerate([(8, 9), (6, 12)])]
    losses = []
    for k, b in enumerate(batches):
        acc._step(m, b, seed=100 + k, accum_index=k, accum_count=2)
        losses.append(m._ws_view("losses", (8,)).cpu().clone())
    Gs = []
    for k, b in enumerate(batches):
        acc._step(twin, b, seed=100 + k, do_adam=False)
        Gs.append(twin.flat_buckets()[1].clone())
        assert torch.equal(twin._ws_view("losses", (8,)).cpu()[:6], losses[k][:6]), k
    twin.flat_buckets()[1].copy_(Gs[0] + Gs[1])
    acc._adam_step(twin, 0.5, 1)
    acc._assert_state_equal(acc._state(m), acc._state(twin))
    assert m._step == 1 and not m.cluster_aborted() and not twin.cluster_aborted()


# ------------------------------------------------------------------------------------------------ mmda_label_counts
@pytest.mark.parametrize("C_", (1, 6, 16))
@pytest.mark.parametrize("N", (1, 63, 64, 65, 4097))
def test_label_counts_equal_an_integer_sum_and_repeat(N, C_):
    lib = _lib.load()
    gen = torch.Generator().manual_seed(N * 17 + C_)
    lab = torch.randn(N, C_, generator=gen)
    lab[torch.rand(N, C_, generator=gen) < 0.5] = 0.0                               # zeros and negatives do not count
    d = lab.to(DEV)
    runs = []
    for _ in range(2):
        counts = torch.zeros(C_, dtype=torch.int64, device=DEV)
        assert lib.mmda_label_counts(d.data_ptr(), N, C_, counts.data_ptr(), _lib.stream_ptr()) == 0
        runs.append(counts.cpu())
    assert torch.equal(runs[0], (lab > 0).sum(dim=0).to(torch.int64))
    assert torch.equal(runs[0], runs[1])
    counts = torch.full((C_,), 5, dtype=torch.int64, device=DEV)                      # (added into what is there)
    assert lib.mmda_label_counts(d.data_ptr(), N, C_, counts.data_ptr(), _lib.stream_ptr()) == 0
    assert torch.equal(counts.cpu(), runs[0] + 5)


def test_class_pos_weight_on_the_device_equals_the_host():
    from mmda_amd import class_pos_weight
    lab = (torch.rand(300, 6, generator=torch.Generator().manual_seed(4)) < torch.tensor([0.5, 0.2, 0.2, 0.08, 0.15, 0.0])).float()
    host = class_pos_weight(lab)
    assert host[5] == 1.0                                                            # no positive
    assert torch.equal(class_pos_weight(lab.to(DEV)), host)
    assert torch.equal(class_pos_weight(lab.to(DEV), cap=3.0), host.clamp(max=3.0))


# ------------------------------------------------------------------------------------------------ Solver, pos_weight="balanced"
def test_solver_resolves_balanced_trains_and_evaluates_with_it():
    import test_gpu_encoded as enc
    from mmda_amd import DeviceDataset, DeviceLoader, MISA, class_pos_weight, make_config
    from mmda_amd.solver import Solver
    lengths = np.random.default_rng(3).integers(1, 10, size=40)
    samples = enc.make_samples(lengths, 35, 74, seed=5)
    ds = DeviceDataset.from_samples(samples, DEV)
    cfg = orc.default_config(vocab_size=120, learning_rate=1e-3)
    c = make_config(precision="fp32", device=DEV, pos_weight="balanced", focal_gamma=2.0, **vars(cfg))
    m = MISA(c)
    m.load_state_dict(orc.synth_params(cfg, 21))
    solver = Solver(c, c, c, DeviceLoader(ds, 8), DeviceLoader(ds, 10), enc.ListLoader([]), is_train=True, model=m).build()
    emo = ds.emo.cpu()
    n = (emo > 0).sum(dim=0).double()
    want = torch.where(n > 0, (40 - n) / n.clamp(min=1), torch.ones_like(n))
    assert solver.cls_pos_weight == want.tolist() == class_pos_weight(ds).tolist()
    assert m.cls_loss == dict(pos_weight=tuple(want.tolist()), focal_gamma=2.0)
    tr = solver.train_epoch()
    assert all(np.isfinite(v) for v in tr.values()) and m._step == 5
    loss, acc, y_pred, y_true = solver.eval("dev")
    per_batch, per_batch64 = [], []
    for scores, truth in solver._eval_batches(solver.dev_data_loader):
        per_batch.append(float(solver.get_cls_loss(scores, truth)))
        per_batch64.append(float(cc.value(scores.detach().cpu().double(), truth.cpu(), want.tolist(), 2.0)))
    assert len(per_batch) == 4
    print(f"eval loss {loss:.8f}  get_cls_loss {np.mean(per_batch):.8f}  float64 {np.mean(per_batch64):.8f}")
    assert abs(loss - np.mean(per_batch)) <= 1e-6 * abs(loss)
    assert abs(loss - np.mean(per_batch64)) <= 1e-5 * abs(loss)
    plain = float(np.mean([float(F.bce_sum_over_classes(s_, t_)) for s_, t_ in solver._eval_batches(solver.dev_data_loader)]))
    assert abs(plain - loss) > 1e-2 * abs(loss)
    assert not m.cluster_aborted()


# ------------------------------------------------------------------------------------------------ the tiny fixture in bf16
def test_bf16_train_step_matches_the_emulating_oracle_tiny_fixture():
    """(the same step as the fp32 one above at tiny_cmd_ragged: hidden 16, encoders of 12 / 5 / 7 units)"""
    _bf16_step_against_the_emulating_oracle("tiny_cmd_ragged")
