"""Training mode (dropout on) on a real MI355X against an exact reference.  The dropout masks are a pure function of (seed, site,
element index): oracle/dropout_rng.py restates them on the host, so the attention and head kernels with dropout, and one whole
training step, have a float64 / masked-oracle reference instead of a comparison with themselves.

Op tests: float64 torch plus the host masks, gradients from autograd; the error is per element, relative to the tensor's max
magnitude (model_compare.rel), so a single wrong row shows: 1e-5 forward, 1e-4 backward, the bounds of test_attention_fwd_bwd and
test_layernorm_fwd_bwd.  Model tests: tests/dropout_cases.py lists the configurations; tests/test_dropout_oracle_cpu.py proves on the
CPU that at each of them every site's mask moves the step by at least 100 of the tolerances applied here."""
import contextlib
import math
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from dropout_cases import CASES, grad_bounds, reference
from model_compare import assert_outputs_and_losses_match_oracle, rel, statement_order_losses
from oracle import dropout_rng as drng

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1                                                   # MMDA_EINVAL (include/mmda_hip.h)
OP_SEED = 0x9E3779B97F4A7C15                                  # a seed that needs all 64 bits


# ------------------------------------------------------------------------------------------------ attention
def _attn_reference(qkv, dctx, mask, S, B, E, nh, dtype):
    """ctx, the un-dropped softmax rows and d_qkv of dropout(softmax(q k' / sqrt(hd))) v in ``dtype``"""
    hd = E // nh
    x = qkv.to(dtype).requires_grad_(True)
    q, k, v = x.view(S, B, 3 * E).split(E, dim=-1)
    h = lambda z: z.reshape(S, B, nh, hd).permute(1, 2, 0, 3)
    att = torch.softmax(h(q) @ h(k).transpose(-1, -2) / math.sqrt(hd), -1)
    ctx = ((att * mask.to(dtype)) @ h(v)).permute(2, 0, 1, 3).reshape(S * B, E)
    ctx.backward(dctx.to(dtype))
    return ctx.detach(), att.detach(), x.grad


ATTN_SHAPES = [(6, 7, 128, 2), (6, 1, 64, 1), (6, 5, 256, 4),           # head width 64, six tokens: the register kernel
               (6, 7, 16, 2), (8, 3, 128, 2), (1, 4, 32, 2), (5, 70, 24, 3)]      # the generic kernel: S = MAXS at hd = 64, S = 1, hd = 8
# + one case per kernel with qkv scaled by 30: logits in the hundreds, max-subtraction at work, saturated rows
ATTN_CASES = [(s, p, 1.0) for s in ATTN_SHAPES for p in (0.0, 0.25, 0.5)] + [((6, 7, 128, 2), 0.25, 30.0), ((6, 7, 16, 2), 0.25, 30.0)]


@pytest.mark.parametrize("shape,p,scale", ATTN_CASES, ids=[f"S{s[0]}-B{s[1]}-E{s[2]}-h{s[3]}-p{p}-x{int(k)}" for s, p, k in ATTN_CASES])
def test_attention_with_dropout_against_float64(shape, p, scale):
    """ctx (with dropout), the stashed probabilities (without) and d_qkv: 1e-5 forward, 1e-4 backward, at every case.  At the scaled
    cases one fp32 ulp of a logit (6e-5 at 512) is that much relative error in every unsaturated probability, whoever computes it: the
    same reference run in float32 lies 1.4e-6 (forward) and 2.7e-5 / 4.0e-5 (backward, hd 64 / hd 8) from its float64 run, which the
    bounds still cover, so they stay.  There, elements whose float64 gradient is below 1e-30 are left out of the backward comparison
    (fp32 underflows where float64 keeps a value)."""
    from mmda_amd import ops
    S, B, E, nh = shape
    g = torch.Generator().manual_seed(S * 1000 + B * 10 + nh)
    qkv = torch.randn(S * B, 3 * E, generator=g) * scale
    dctx = torch.randn(S * B, E, generator=g)
    mask = torch.from_numpy(drng.mask(p, OP_SEED, drng.SITE_ATTN, (B, nh, S, S)))
    if p > 0 and B * nh * S * S >= 36:
        assert bool((mask == 0).any()) and bool((mask != 0).any())
    ctx, att, dqkv = _attn_reference(qkv, dctx, mask, S, B, E, nh, torch.float64)
    tol_f, tol_b = 1e-5, 1e-4
    if scale != 1.0:
        assert float(att.max(-1).values.min()) > 0.5 and float(att.max()) > 0.999        # the rows do saturate
    d = torch.device(DEV)
    c, pr = ops.attn_fwd(qkv.to(d), S, B, E, nh, drop_p=p, seed=OP_SEED, site=drng.SITE_ATTN)
    e_ctx, e_pr = rel(c, ctx), rel(pr, att)
    dq = ops.attn_bwd(qkv.to(d), pr, dctx.to(d), S, B, E, nh, drop_p=p, seed=OP_SEED, site=drng.SITE_ATTN).cpu().double()
    ref = dqkv
    if scale != 1.0:
        keep = dqkv.abs() >= 1e-30
        dq, ref = dq[keep], dqkv[keep]
    e_dq = rel(dq, ref)
    print(f"attention {shape} p={p} x{scale}: ctx {e_ctx:.2e} probs {e_pr:.2e} (bound {tol_f:.1e}), d_qkv {e_dq:.2e} (bound {tol_b:.1e})")
    assert e_ctx < tol_f and e_pr < tol_f
    assert e_dq < tol_b


def test_attention_rejects_shapes_it_has_no_kernel_for():
    from mmda_amd import _lib
    lib = _lib.load()
    buf = lambda *s: torch.zeros(*s, device=DEV)
    for S, B, E, nh in ((9, 2, 32, 2), (6, 2, 34, 4)):        # S above MAXS = 8; E no multiple of nhead
        qkv, ctx, probs, dctx = buf(S * B, 3 * E), buf(S * B, E), buf(B, nh, S, S), buf(S * B, E)
        s = _lib.stream_ptr()
        assert lib.mmda_attn_fwd(qkv.data_ptr(), S, B, E, nh, ctx.data_ptr(), probs.data_ptr(), 0.25, 1, 1, s) == EINVAL, (S, E, nh)
        assert lib.mmda_attn_bwd(qkv.data_ptr(), probs.data_ptr(), dctx.data_ptr(), S, B, E, nh, torch.zeros_like(qkv).data_ptr(), 0.25, 1, 1,
                                 s) == EINVAL, (S, E, nh)


# ------------------------------------------------------------------------------------------------ heads
THR = 0.35


def _heads_inputs(B, ncls):
    """logits (B, 6 + ncls) ~ 3 N(0, 1) with +-40 planted in both heads (the sigmoid saturates), and the two upstream gradients.
    Seeds: 20 + B + ncls.  No float64 score of any case below lies within 1e-6 of the threshold (asserted)."""
    g = torch.Generator().manual_seed(20 + B + ncls)
    z = torch.randn(B, 6 + ncls, generator=g) * 3.0
    z[0, 1], z[0, 4], z[0, 6], z[-1, 6 + ncls - 1], z[B // 2, 7] = 40.0, -40.0, 40.0, -40.0, -40.0
    return z, torch.randn(B, 6, generator=g), torch.randn(B, ncls, generator=g)


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("ncls", [6, 3])
@pytest.mark.parametrize("B", [1, 5, 70])
def test_heads_fwd_bwd_against_float64(B, ncls, p):
    """tcp = sigmoid(confidence logits), scores = sigmoid(classifier logits * mask), labels = scores > threshold; d_logits with either
    upstream gradient absent.  Forward 1e-5, backward 1e-4 of the tensor's max; labels exact (no reference score within 1e-6 of the
    threshold at these seeds, so none is excused; the allowance is 1 %)."""
    from mmda_amd import ops
    z, dtcp, dsc = _heads_inputs(B, ncls)
    seed = OP_SEED + (2 if B == 1 else 0)                    # B = 1, six or three elements: a seed whose mask drops and keeps
    mask = torch.from_numpy(drng.mask(p, seed, drng.SITE_CLS, (B, ncls)))
    if p > 0:
        assert bool((mask == 0).any()) and bool((mask != 0).any()), "choose another seed"
    x = z.double().requires_grad_(True)
    tcp = torch.sigmoid(x[:, :6])
    sc = torch.sigmoid(x[:, 6:] * mask)
    near = (sc.detach() - THR).abs() < 1e-6
    assert not bool(near.any()), "choose another seed: a reference score sits on the threshold"
    d = torch.device(DEV)
    t_g, s_g, l_g = ops.heads_fwd(z.to(d), ncls, THR, drop_p=p, seed=seed, site=drng.SITE_CLS)
    assert rel(t_g, tcp) < 1e-5 and rel(s_g, sc) < 1e-5
    assert float((s_g.cpu().double() - sc.detach()).abs().max()) < 1e-6              # and absolutely: scores are probabilities
    wrong = (l_g.cpu().double() != (sc.detach() > THR).double()) & ~near
    assert not bool(wrong.any()) and float(near.double().mean()) <= 0.01
    assert set(l_g.unique().tolist()) <= {0.0, 1.0}
    for use_t, use_s in ((True, True), (True, False), (False, True), (False, False)):
        x.grad = None
        loss = (tcp * dtcp.double()).sum() * float(use_t) + (sc * dsc.double()).sum() * float(use_s)
        loss.backward(retain_graph=True)
        got = ops.heads_bwd(t_g, s_g, dtcp.to(d) if use_t else None, dsc.to(d) if use_s else None, ncls, drop_p=p, seed=seed,
                            site=drng.SITE_CLS).cpu()
        if use_t or use_s:
            assert rel(got, x.grad) < 1e-4, (use_t, use_s)
        # an absent head's columns must be exactly zero, not "small"
        if not use_t:
            assert float(got[:, :6].abs().max()) == 0.0
        if not use_s:
            assert float(got[:, 6:].abs().max()) == 0.0
        if p > 0 and use_s:
            assert bool((got[:, 6:][mask == 0] == 0).all())                          # a dropped logit has no gradient


# ------------------------------------------------------------------------------------------------ one training step
@contextlib.contextmanager
def _fusion_dropout(p):
    """mmda_amd.models.FUSION_DROPOUT (read when a model is made) at ``p`` for the block"""
    import mmda_amd.models as mm
    old = mm.FUSION_DROPOUT
    try:
        mm.FUSION_DROPOUT = p
        yield
    finally:
        mm.FUSION_DROPOUT = old


def _make_model(case, cfg, P):
    from mmda_amd import make_config, MISA
    with _fusion_dropout(case.p_tf):
        m = MISA(make_config(precision=case.precision, device=DEV, **vars(cfg)))
    missing = m.load_state_dict(P, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    m.to(DEV)
    return m


def _to_dev(batch):
    return {k: (v.to(DEV) if k != "l" else v) for k, v in batch.items()}


def _assert_grads(grads, cfg, case, skip=()):
    """``grads`` {name: gradient} against the oracle's (dropout_cases.grad_bounds: the reference and each tensor's bound).  fp32: max
    error relative to the tensor's max magnitude, as test_gpu_model._check_grads (key part of in_proj_bias: identically zero in exact
    arithmetic, compared absolutely); bf16: relative L2, as test_bf16_path_within_1e2.  A gradient the oracle leaves None must be
    exactly zero.  A gradient that is not finite in the oracle itself (B = 1: everything in front of CMD's sqrt(0)) has no value to
    agree with and is left out; every other tensor is compared.  Returns the number compared."""
    G, bounds = grad_bounds(case)
    checked = 0
    for k, g in grads.items():
        if k in skip or (G[k] is not None and not bool(torch.isfinite(G[k]).all())):
            continue
        g = torch.as_tensor(g).detach().cpu().double()
        assert bool(torch.isfinite(g).all()), k
        if G[k] is None:
            assert float(g.abs().max()) == 0.0, f"{k}: the reference leaves this gradient None; ours must be exactly zero"
            continue
        ref = G[k].double()
        if k.endswith("self_attn.in_proj_bias"):
            hs = cfg.hidden_size
            keep = torch.ones(3 * hs, dtype=torch.bool); keep[hs:2 * hs] = False
            assert float(g[~keep].abs().max()) < 1e-5
            g, ref = g[keep], ref[keep]
        if case.precision == "fp32":
            e = float((g - ref).abs().max() / ref.abs().max().clamp_min(1e-6))
        else:
            e = float((g - ref).norm() / ref.norm().clamp_min(1e-30))
        if e > 0.25 * bounds[k]:
            print(f"{case.name} {k}: gradient error {e:.3e} (bound {bounds[k]:.1e})")
        assert e < bounds[k], f"{case.name} {k}: gradient error {e:.3e} (bound {bounds[k]:.1e})"
        checked += 1
    return checked


def _assert_step(case, scores, tcp, losses, grads, skip=()):
    cfg, P, batch, masks, (o, L, G) = reference(case)
    if case.precision == "fp32":
        assert_outputs_and_losses_match_oracle(scores, tcp, losses, o, L, case.tol_out)
    else:                                                     # bf16: outputs 1e-3, losses 1e-4 (test_bf16_path_within_1e2, part 1)
        assert rel(scores, o.scores.detach()) < case.tol_out and rel(tcp, o.tcp.detach()) < case.tol_out
        for k in ("cls", "diff", "sim", "recon", "conf", "total"):
            ref = float(getattr(L, k).detach())
            assert abs(losses[k] - ref) < case.tol_loss * abs(ref) + 1e-7, (k, losses[k], ref)
    if case.B == 1:
        # one sample: CMD's gradient is NaN in the reference itself (test_degenerate_shapes_against_the_oracle), and with it every
        # gradient behind the shared projections.  The fusion layer's and the classifier's own gradients (and those of the private and
        # reconstruction layers) are finite and are compared: the backward pass of one sample per workgroup with every mask on
        finite = [k for k, g in G.items() if g is not None and bool(torch.isfinite(g).all())]
        assert any(g is not None and not torch.isfinite(g).all() for g in G.values())
        assert sum(k.startswith(("transformer_encoder.", "classifier.")) for k in finite) == 14, finite      # (+ private_*, recon_*)
        assert _assert_grads(grads, cfg, case, skip) >= len(finite)
        return
    assert _assert_grads(grads, cfg, case, skip) > 20


def _native_step(case, model=None):
    cfg, P, batch, masks, _ = reference(case)
    model = model or _make_model(case, cfg, P)
    b = _to_dev(batch)
    model.train_step(b["t"], b["v"], b["a"], b["l"], b["emo"], lr=cfg.learning_rate, clip=cfg.clip, do_adam=False, training=True,
                     seed=case.seed)
    assert not model.cluster_aborted()
    pub = model._public()
    model._assign_grad_views()
    return model, pub, {k: p.grad for k, p in model.named_parameters()}


@pytest.mark.parametrize("name", ["fused_b5", "fused_b1", "fused_b5_p01", "adv_confid_b6", "generic_b260", "bf16_b8"])
def test_training_step_matches_the_masked_oracle(name):
    """One fused training step (dropout on, explicit seed, no optimizer) against loss_and_grads(masks=site_masks(seed)): scores, tcp,
    the six losses and every parameter gradient, at the dropout-off bounds of the same path.  fused_b5 / fused_b1: the fused per-sample
    stretches; fused_b5_p01: FUSION_DROPOUT at its default 0.1; adv_confid_b6: the stand-alone launches, the discriminator's dropout,
    live confidence gradients; generic_b260: the tiled GEMM epilogue's mask index; bf16_b8: bf16 encoders in front of the same block."""
    case = CASES[name]
    model, pub, grads = _native_step(case)
    _assert_step(case, pub["scores"], pub["tcp"], model.read_losses(), grads)
    # a second step with the same seed reproduces the first; another seed does not
    s1 = pub["scores"].clone()
    model2, pub2, _ = _native_step(case, model)
    assert rel(pub2["scores"], s1) < 1e-5
    b = _to_dev(reference(case)[2])
    cfg = reference(case)[0]
    model.train_step(b["t"], b["v"], b["a"], b["l"], b["emo"], lr=cfg.learning_rate, clip=cfg.clip, do_adam=False, training=True,
                     seed=case.seed + 1)
    assert rel(model._public()["scores"], s1) > 1e-3


_CHILD = r'''
import sys, numpy as np, torch
sys.path.insert(0, %r); sys.path.insert(0, %r)
import mmda_amd.models as mm
from dropout_cases import CASES, inputs_of
from mmda_amd import make_config, MISA
case = CASES["fused_b5"]
cfg, P, b = inputs_of(case)
mm.FUSION_DROPOUT = case.p_tf
m = MISA(make_config(precision="fp32", device="cuda:0", **vars(cfg))); m.load_state_dict(P); m.to("cuda:0")
m.train_step(b["t"].cuda(), b["v"].cuda(), b["a"].cuda(), b["l"], b["emo"].cuda(), lr=0.0, clip=1.0, do_adam=False, training=True, seed=case.seed)
torch.cuda.synchronize()
assert not m.cluster_aborted()
m._assign_grad_views()
L = m.read_losses()
out = {"g::" + k: p.grad.cpu().numpy() for k, p in m.named_parameters()}
out.update({"o::" + k: m._public()[k].cpu().numpy() for k in ("scores", "tcp")})
out.update({"l::" + k: np.float64(v) for k, v in L.items()})
np.savez(sys.argv[1], **out)
'''


@pytest.mark.parametrize("switches", [{"MMDA_ROW_FUSE": "0"}, {"MMDA_FFN_FUSE": "0"}], ids=["stand_alone_fusion_launches", "skinny_feed_forward"])
def test_replaced_launches_match_the_masked_oracle_in_a_fresh_process(switches):
    """The launches the fused stretches replaced (MMDA_ROW_FUSE=0: stand-alone LayerNorm / attention / heads kernels;
    MMDA_FFN_FUSE=0: the row-skinny GEMM's dropout epilogue and the gated backward), one switch per fresh process, each against the
    ORACLE of fused_b5 -- not against the default path, which would carry the same masks and the same mistakes."""
    case = CASES["fused_b5"]
    code = _CHILD % (ROOT, os.path.join(ROOT, "tests"))
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, "o.npz")
        r = subprocess.run([sys.executable, "-c", code, f], env=dict(os.environ, **switches), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        z = np.load(f)
        got = {k: z[k] for k in z.files}
    _assert_step(case, got["o::scores"], got["o::tcp"], {k[3:]: float(v) for k, v in got.items() if k.startswith("l::")},
                 {k[3:]: v for k, v in got.items() if k.startswith("g::")})


def test_autograd_entry_in_training_mode_matches_the_masked_oracle():
    """model.train(); model(...); the reference's getters; total.backward(): the seed is the model's own draw -- predicted here from
    MISA._seed by the LCG of MISA._next_seed, which is also the seed of the case's masks."""
    from mmda_amd.solver import Solver
    case = CASES["autograd_b5"]
    cfg, P, batch, masks, _ = reference(case)
    model = _make_model(case, cfg, P)
    b = _to_dev(batch)
    predicted = (model._seed * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
    assert predicted == case.seed
    model.train()
    c = model.config
    solver = Solver(c, c, c, None, None, None, is_train=True, model=model)
    scores, labels = model(b["t"], b["v"], b["a"], b["l"], None, None, None)
    assert model._seed == predicted, "the forward drew another seed than the LCG predicts"
    L, total = statement_order_losses(solver, cfg, scores, b["emo"])
    losses = {k: float(v.detach()) for k, v in L.items()}
    losses["total"] = float(total.detach())
    model.zero_grad()
    total.backward()
    _assert_step(case, scores, model.tcp, losses, {k: p.grad for k, p in model.named_parameters()})


def _samples_of(b):
    """The columns of an ``orc.synth_batch`` as reference-style samples: sample i is column i cut to its length"""
    out = []
    for i, n in enumerate(b["l"].tolist()):
        lab = np.concatenate([[0.0], b["emo"][i].numpy()]).astype(np.float32)[None]
        out.append(((b["t"][:n, i].numpy(), b["v"][:n, i].numpy(), b["a"][:n, i].numpy(), ["w"] * n), lab, f"seg{i}"))
    return out


def test_train_step_encoded_matches_the_masked_oracle():
    """The same batch through the encoder cache (encoders frozen, the step starts at the projections): the masks of the fusion block and
    the heads do not depend on the entry point, so outputs, losses and the gradients of everything behind the encoders go against the
    numbers of fused_b5."""
    from mmda_amd import DeviceDataset, EncodedLoader, EncoderCache
    case = CASES["fused_b5"]
    cfg, P, batch, masks, _ = reference(case)
    model = _make_model(case, cfg, P)
    model._materialize(torch.device(DEV))
    model.freeze("trnn1", "trnn2", "vrnn1", "vrnn2", "arnn1", "arnn2", "tlayer_norm", "vlayer_norm", "alayer_norm", "embed")
    frozen = set(model.frozen_names())
    cache = EncoderCache.build(model, DeviceDataset.from_samples(_samples_of(batch), DEV), case.B, order="dataset")
    (eb,) = list(EncodedLoader(cache, case.B))
    assert eb.rows.tolist() == list(range(case.B))
    model.train_step_encoded(eb, lr=cfg.learning_rate, clip=cfg.clip, do_adam=False, training=True, seed=case.seed)
    pub = model._public()
    model._assign_grad_views()
    grads = {k: p.grad for k, p in model.named_parameters() if k not in frozen}
    assert all(g is not None for g in grads.values()) and len(grads) > 30
    _assert_step(case, pub["scores"], pub["tcp"], model.read_losses(), grads)
