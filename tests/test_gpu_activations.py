"""Every activation id at every kernel site that applies one, on a real MI355X, against the same operation in torch on the CPU in
FLOAT64 (gradients from autograd).  One act_fwd / act_bwd pair (csrc/common.h) serves the GEMM epilogues, the LayerNorm kernels,
the fused per-sample backward and the discriminator's element-wise kernels; PReLU's slope gradient and RReLU's replayed slopes have
their own code at each site.  Inputs carry the kinks -1, -0.5, 0, 0.5, 1 exactly: float64 torch has the conventions common.h
encodes (relu'(0) = 0, leaky'(0) = 0.01, elu'(0) = 1, hardtanh'(+-1) = 0, hardshrink(+-0.5) = hardshrink'(+-0.5) = 0, prelu'(0) =
slope, rrelu eval slope (lo + hi) / 2), so the reference alone judges them.  DESIGN.md section 4b has the id x site table."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import misa_oracle as orc
from model_compare import assert_grads_match_oracle, assert_outputs_and_losses_match_oracle, statement_order_losses


def dev():
    return torch.device("cuda:0")


def relerr(got, ref):
    got = got.detach().float().cpu(); ref = ref.detach().float().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all(), "non-finite values in HIP output"
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-6))


TOL = {"fp32": 1e-4, "bf16": 1e-2}          # as tests/test_gpu_ops.py: relative to the tensor's maximum

PLAIN = ["none", "relu", "sigmoid", "leakyrelu", "tanh", "elu", "hardtanh", "hardshrink"]      # ids 0..7: no parameters
ALL = PLAIN + ["prelu", "rrelu"]
SELECTS = ("none", "relu", "hardtanh", "hardshrink")           # the output is x, 0 or +-1: exact in any precision
CONST_DERIVATIVE = SELECTS + ("leakyrelu", "prelu")            # the derivative is one of 0, 1, 0.01, the slope
KINKS = (-1.0, -0.5, 0.0, 0.5, 1.0)
SLOPE = 0.25                                                   # PReLU's on the device (exact in fp32)
LO, HI = 1.0 / 8.0, 1.0 / 3.0                                  # nn.RReLU's defaults


def act64(name, x, slope=None):
    if name == "none": return x
    if name == "relu": return F.relu(x)
    if name == "sigmoid": return torch.sigmoid(x)
    if name == "leakyrelu": return F.leaky_relu(x, 0.01)
    if name == "tanh": return torch.tanh(x)
    if name == "elu": return F.elu(x)
    if name == "hardtanh": return F.hardtanh(x)
    if name == "hardshrink": return F.hardshrink(x)
    if name == "prelu": return F.prelu(x, slope)
    if name == "rrelu": return F.rrelu(x, LO, HI, training=False)
    raise KeyError(name)


def planted(shape, seed):
    """randn with every 7th element (flat order) overwritten cyclically by the kinks"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    flat = x.view(-1)
    k = flat[::7].numel()
    flat[::7] = torch.tensor(KINKS).repeat(k // len(KINKS) + 1)[:k]
    return x


def act_kw(name, d, rand=0, seed=0, site=0, dslope_fill=None):
    """keywords of the ops wrappers for the parametrised activations; returns (kw for forward, kw for backward, dslope tensor)"""
    if name == "prelu":
        slope = torch.full((1,), SLOPE, device=d)
        dslope = None if dslope_fill is None else torch.full((1,), dslope_fill, device=d)
        return dict(slope=slope), dict(slope=slope, dslope=dslope), dslope
    if name == "rrelu":
        kw = dict(rrelu=(LO, HI, rand, seed, site))
        return kw, dict(kw), None
    return {}, {}, None


# ------------------------------------------------------------------------------------------------ A. element-wise site
@pytest.mark.parametrize("n", [1000, 600001])                  # 600 001: odd and above 2048 * 256, the grid-stride loop wraps
@pytest.mark.parametrize("act", ALL)
def test_act_dropout_fwd_bwd_all_ids(act, n):
    from mmda_amd import ops
    d = dev()
    x = planted((n,), 20)
    dh = torch.randn(n, generator=torch.Generator().manual_seed(21))
    slope64 = torch.tensor([SLOPE], dtype=torch.float64, requires_grad=True)
    xd, dhd = x.to(d), dh.to(d)
    for p, seed, site in ((0.0, 0, 0), (0.25, 77, 5)):
        mask = ops.dropout_mask_via_act(n, p, seed, site, d).cpu().double() if p > 0 else torch.ones(n, dtype=torch.float64)
        x64 = x.double().requires_grad_(True)
        slope64.grad = None
        ref = act64(act, x64, slope64) * mask
        ref.backward(dh.double())
        fkw, bkw, dslope = act_kw(act, d, dslope_fill=3.0)
        h = ops.act_dropout_fwd(xd, act, p, seed, site, **fkw)
        dz = ops.act_dropout_bwd(dhd, xd, act, p, seed, site, **bkw)
        if p == 0.0 and act in SELECTS:
            assert torch.equal(h.cpu(), ref.detach().float())
        assert relerr(h, ref) < TOL["fp32"], (act, p)
        assert relerr(dz, x64.grad) < TOL["fp32"], (act, p)
        if act == "prelu":
            gz = (dh.double() * mask * x.double())[x <= 0]
            want, allowed = 3.0 + float(gz.sum()), 1e-4 * float(gz.abs().sum())
            assert abs(want - (3.0 + float(slope64.grad))) <= 1e-9 * float(gz.abs().sum())      # autograd's is the same sum
            got = float(dslope.cpu())
            print(f"prelu dslope n={n} p={p}: got {got:.6f} want {want:.6f} allowed {allowed:.3e}")
            assert abs(got - want) <= allowed, (got, want, allowed)
        if p == 0.0 and act in CONST_DERIVATIVE:                # dh = 1: dz is the derivative itself
            x64 = x.double().requires_grad_(True)
            act64(act, x64, slope64).sum().backward()
            _, bkw1, _ = act_kw(act, d)
            dz1 = ops.act_dropout_bwd(torch.ones(n, device=d), xd, act, 0.0, 0, 0, **bkw1)
            assert torch.equal(dz1.cpu(), x64.grad.float()), act
        if p == 0.0 and act == "elu":
            # measured, not asserted: act_fwd computes exp(x) - 1 where torch has expm1; against the tensor's maximum that passes,
            # per element it cannot be accurate near 0 (DESIGN.md section 4b records the figure)
            near = (x < 0) & (x >= -1e-3)
            if bool(near.any()):
                r = ref.detach()[near]
                e = float(((h.cpu().double()[near] - r) / r).abs().max())
                print(f"elu forward, {int(near.sum())} elements with x in [-1e-3, 0): worst per-element relative error {e:.3e}")


@pytest.mark.parametrize("n", [1000, 600001])
def test_rrelu_training_draws_are_uniform_and_replayed_elementwise(n):
    """rand = 1 with z = -1 and dh = 1: h = -slope, so every h lies in (-hi, -lo], their mean is (lo + hi) / 2 within three standard
    errors of a uniform variable (sd (hi - lo) / sqrt(12)), the backward pass replays the draws bit for bit, another seed draws others."""
    from mmda_amd import ops
    d = dev()
    z = torch.full((n,), -1.0, device=d); one = torch.ones(n, device=d)
    lo, hi = float(torch.tensor(LO, dtype=torch.float32)), float(torch.tensor(HI, dtype=torch.float32))
    h = ops.act_dropout_fwd(z, "rrelu", 0.0, 0, 0, rrelu=(LO, HI, 1, 1234, 3))
    dz = ops.act_dropout_bwd(one, z, "rrelu", 0.0, 0, 0, rrelu=(LO, HI, 1, 1234, 3))
    hc = h.cpu().double()
    assert bool(((hc > -hi) & (hc <= -lo)).all()), (float(hc.min()), float(hc.max()))
    mean = float((-hc).mean())
    print(f"rrelu n={n}: mean slope {mean:.6f}, (lo + hi) / 2 = {(lo + hi) / 2:.6f}, bound {3 / math.sqrt(12 * n) * (hi - lo):.3e}")
    assert abs(mean - (lo + hi) / 2) <= 3 / math.sqrt(12 * n) * (hi - lo)
    assert torch.equal(dz, -h)
    h2 = ops.act_dropout_fwd(z, "rrelu", 0.0, 0, 0, rrelu=(LO, HI, 1, 1235, 3))
    assert not torch.equal(h2, h)


# ------------------------------------------------------------------------------------------------ B. LayerNorm sites
def _ln_reference(act, x, res, mask, g, b, dy, permute=None):
    """float64 autograd of layer_norm(act(x) + res * mask) (res may be None).  dy in the output's layout."""
    n = x.shape[-1]
    x64 = x.double().requires_grad_(True); g64 = g.double().requires_grad_(True); b64 = b.double().requires_grad_(True)
    r64 = None if res is None else res.double().requires_grad_(True)
    slope64 = torch.tensor([SLOPE], dtype=torch.float64, requires_grad=True)
    a = act64(act, x64, slope64)
    a.retain_grad()
    pre = a if res is None else a + r64 * mask
    y = F.layer_norm(pre, (n,), g64, b64, 1e-5)
    if permute:
        y = y.view(permute[0], permute[1], n).permute(1, 0, 2).contiguous()
    y.backward(dy.double())
    mean = pre.detach().mean(-1)
    rstd = 1.0 / torch.sqrt(pre.detach().var(-1, unbiased=False) + 1e-5)
    za = (a.grad * x.double())[x <= 0]                        # PReLU: d(slope) = sum of d(act output) * z over z <= 0
    return dict(y=y.detach(), mean=mean, rstd=rstd, dx=x64.grad, dres=None if res is None else r64.grad, dg=g64.grad, db=b64.grad,
                dslope=float(za.sum()), dslope_abs=float(za.abs().sum()),
                dslope_autograd=None if slope64.grad is None else float(slope64.grad))


def _check_dslope(got, ref, filled, what):
    want, allowed = filled + ref["dslope"], 1e-4 * ref["dslope_abs"]
    assert abs(ref["dslope"] - ref["dslope_autograd"]) <= 1e-9 * ref["dslope_abs"]
    print(f"prelu dslope {what}: got {got:.6f} want {want:.6f} allowed {allowed:.3e}")
    assert abs(got - want) <= allowed, (what, got, want, allowed)


# (n, rows): two 64-lane passes with masked lanes; the fusion width; wide rows, few of them.  One case permuted (S, B) -> (B, S).
LN_CASES = [(70, 33, None), (128, 192, None), (600, 5, None), (128, 192, (6, 32))]


@pytest.mark.parametrize("n,rows,permute", LN_CASES)
@pytest.mark.parametrize("act", ALL)
def test_layernorm_sites_all_ids(act, n, rows, permute):
    """Stand-alone forward and backward with a dropped-out residual, then the same row through the multi-problem launches and the
    separate parameter-gradient pass (no residual there).  Bounds as test_layernorm_fwd_bwd (tests/test_gpu_ops.py): 1e-5 on y,
    1e-4 on gradients; mean and rstd are sums of the same n terms as y and get y's bound."""
    from mmda_amd import ops
    d = dev()
    gen = torch.Generator().manual_seed(31)
    x = planted((rows, n), 30)
    res = torch.randn(rows, n, generator=gen); g = torch.randn(n, generator=gen); b = torch.randn(n, generator=gen)
    dy = torch.randn((permute[1], permute[0], n) if permute else (rows, n), generator=gen)
    p, seed, site = 0.25, 91, 7
    mask = ops.dropout_mask_via_act(rows * n, p, seed, site, d).cpu().double().view(rows, n)
    ref = _ln_reference(act, x, res, mask, g, b, dy, permute)
    xd, rd, gd, bd, dyd = x.to(d), res.to(d), g.to(d), b.to(d), dy.to(d)
    fkw, bkw, dslope = act_kw(act, d, dslope_fill=3.0)
    y, mean, rstd = ops.layernorm_fwd(xd, gd, bd, res=rd, act=act, drop_p=p, seed=seed, site=site, permute=permute, **fkw)
    assert relerr(y, ref["y"]) < 1e-5 and relerr(mean, ref["mean"]) < 1e-5 and relerr(rstd, ref["rstd"]) < 1e-5
    dx, dres, dg, db = ops.layernorm_bwd(dyd, xd, gd, mean, rstd, res=rd, act=act, drop_p=p, seed=seed, site=site, permute=permute,
                                         want_dres=True, **bkw)
    assert relerr(dx, ref["dx"]) < 1e-4 and relerr(dres, ref["dres"]) < 1e-4
    assert relerr(dg, ref["dg"]) < 1e-4 and relerr(db, ref["db"]) < 1e-4
    if act == "prelu":
        _check_dslope(float(dslope.cpu()), ref, 3.0, f"layernorm_bwd n={n} rows={rows}")
    if permute:
        return                                               # (the multi wrapper takes no permutation)
    ref = _ln_reference(act, x, None, None, g, b, dy)
    fkw, bkw, dslope = act_kw(act, d, dslope_fill=3.0)
    (y, dx, dg, db), = ops.layernorm_multi([xd], [gd], [bd], [dyd], acts=[act], **bkw)
    assert relerr(y, ref["y"]) < 1e-5 and relerr(dx, ref["dx"]) < 1e-4
    assert relerr(dg, ref["dg"]) < 1e-4 and relerr(db, ref["db"]) < 1e-4
    if act == "prelu":
        _check_dslope(float(dslope.cpu()), ref, 3.0, f"layernorm_multi n={n} rows={rows}")


@pytest.mark.parametrize("rows,n", [(5, 128), (128, 5)])
def test_layernorm_multi_three_activations_share_one_slope(rows, n):
    """Three problems with three activations in one launch each way, PReLU among them twice: all share one slope / dslope pointer, as
    the model's three projections do, and dslope must hold the sum over the problems."""
    from mmda_amd import ops
    d = dev()
    acts = ["prelu", "hardshrink", "prelu"]
    gen = torch.Generator().manual_seed(41)
    xs = [planted((rows, n), 40 + i) for i in range(3)]
    gs = [torch.randn(n, generator=gen) for _ in range(3)]; bs = [torch.randn(n, generator=gen) for _ in range(3)]
    dys = [torch.randn(rows, n, generator=gen) for _ in range(3)]
    refs = [_ln_reference(a, x, None, None, g, b, dy) for a, x, g, b, dy in zip(acts, xs, gs, bs, dys)]
    _, bkw, dslope = act_kw("prelu", d, dslope_fill=3.0)
    got = ops.layernorm_multi([t.to(d) for t in xs], [t.to(d) for t in gs], [t.to(d) for t in bs], [t.to(d) for t in dys], acts=acts, **bkw)
    for ref, (y, dx, dg, db) in zip(refs, got):
        assert relerr(y, ref["y"]) < 1e-5 and relerr(dx, ref["dx"]) < 1e-4
        assert relerr(dg, ref["dg"]) < 1e-4 and relerr(db, ref["db"]) < 1e-4
    total = dict(dslope=refs[0]["dslope"] + refs[2]["dslope"], dslope_abs=refs[0]["dslope_abs"] + refs[2]["dslope_abs"],
                 dslope_autograd=refs[0]["dslope_autograd"] + refs[2]["dslope_autograd"])
    _check_dslope(float(dslope.cpu()), total, 3.0, f"three problems rows={rows} n={n}")


@pytest.mark.parametrize("n,rows", [(70, 33), (600, 5)])
def test_rrelu_training_draws_at_the_layernorm_site_are_the_elementwise_ones(n, rows):
    """rand = 1 ties the LayerNorm kernels' RNG index (row * n + column) to the element-wise kernels' flat index, forward and backward."""
    from mmda_amd import ops
    d = dev()
    gen = torch.Generator().manual_seed(51)
    x = planted((rows, n), 50).to(d)
    g = torch.randn(n, generator=gen).to(d); b = torch.randn(n, generator=gen).to(d); dy = torch.randn(rows, n, generator=gen).to(d)
    rr = (LO, HI, 1, 4321, 9)
    y1, mean1, rstd1 = ops.layernorm_fwd(x, g, b, act="rrelu", rrelu=rr)
    a = ops.act_dropout_fwd(x.view(-1), "rrelu", 0.0, 0, 0, rrelu=rr).view(rows, n)
    assert not torch.equal(a, ops.act_dropout_fwd(x.view(-1), "rrelu", 0.0, 0, 0, rrelu=(LO, HI, 0, 0, 0)).view(rows, n))     # draws, not the mean
    y2, mean2, rstd2 = ops.layernorm_fwd(a, g, b)
    assert relerr(y1, y2) < 1e-6
    dx1, _, _, _ = ops.layernorm_bwd(dy, x, g, mean1, rstd1, act="rrelu", rrelu=rr)
    dx2, _, _, _ = ops.layernorm_bwd(dy, a, g, mean2, rstd2)
    want = ops.act_dropout_bwd(dx2.view(-1), x.view(-1), "rrelu", 0.0, 0, 0, rrelu=rr).view(rows, n)
    assert relerr(dx1, want) < 1e-6


# ------------------------------------------------------------------------------------------------ C. GEMM epilogues
# Operands are integers in [-4, 4] over 4, the bias integers in [-16, 16] over 16, alpha = 0.25 where the entry point has one: every
# product is a multiple of 1/64 and every partial sum fits in 24 bits, so the pre-activation is the SAME fp32 number in any summation
# order -- and with bf16 operands, which hold these values exactly, and in MX e4m3 (k/4 * 2^8 or 2^9 <= 384 is representable).  The
# output must then be act64(exact pre-activation): bit for bit where the activation selects, to the fp32 tolerance where it computes.
# The seeds are chosen (on the CPU) so that at least four pre-activations sit exactly on each kink.
GEMM_SEEDS = {(33, 70, 35): 0, (70, 144, 160): 0, (96, 128, 128): 0, (37, 48, 128): 0}


def exact_problem(M, N, K, alpha):
    gen = torch.Generator().manual_seed(GEMM_SEEDS[(M, N, K)])
    A = torch.randint(-4, 5, (M, K), generator=gen).float() / 4
    W = torch.randint(-4, 5, (N, K), generator=gen).float() / 4
    bias = torch.randint(-16, 17, (N,), generator=gen).float() / 16
    pre = (A.double() @ W.double().t()) * alpha + bias.double()
    assert torch.equal(((A @ W.t()) * alpha + bias).double(), pre)                 # exact in fp32 too: the premise of this section
    for k in KINKS:
        assert int((pre == k).sum()) >= 4, f"the inputs put only {int((pre == k).sum())} pre-activations on {k}"
    return A, W, bias, pre


def check_epilogue(out, act, pre):
    ref = act64(act, pre)
    if act in SELECTS:
        assert torch.equal(out.cpu(), ref.float()), act
    else:
        assert relerr(out, ref) < TOL["fp32"], act


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("M,N,K", [(33, 70, 35), (70, 144, 160)])      # the few-k-tile class; the general 64-tile class
@pytest.mark.parametrize("act", PLAIN)
def test_gemm_epilogue_on_exact_preactivations(act, M, N, K, mode):
    from mmda_amd import ops
    A, W, bias, pre = exact_problem(M, N, K, 0.25)
    out = ops.gemm(A.to(dev()), W.to(dev()), mode=mode, bias=bias.to(dev()), act=act, alpha=0.25)
    check_epilogue(out, act, pre)


@pytest.mark.parametrize("M,N,K", [(33, 70, 35), (96, 128, 128)])      # scalar operand loads; float4 loads
@pytest.mark.parametrize("act", PLAIN)
def test_gemm_skinny_epilogue_on_exact_preactivations(act, M, N, K):
    from mmda_amd import ops
    A, W, bias, pre = exact_problem(M, N, K, 0.25)
    out, = ops.gemm_skinny([dict(A=A.to(dev()), B=W.to(dev()), bias=bias.to(dev()), act=act, alpha=0.25)])
    check_epilogue(out, act, pre)


@pytest.mark.parametrize("act", PLAIN)
def test_gemm_mx8_epilogue_on_exact_preactivations(act):
    from mmda_amd import ops
    A, W, bias, pre = exact_problem(37, 48, 128, 1.0)            # (mmda_mx8_args has no alpha)
    out = ops.gemm_mx8(A.to(dev()), W.to(dev()), bias=bias.to(dev()), act=act)
    check_epilogue(out, act, pre)


# ------------------------------------------------------------------------------------------------ D. whole model
# The activations no fixture covers, against the live oracle, hidden size 128 (the fused-row kernels apply) and the adversarial branch on
# (the discriminator's act_drop kernels run).  The projections and the discriminator's first layer are scaled up in BOTH sides'
# parameters: unscaled, the projections' pre-activations stay within +-0.33, where hardtanh never saturates and hardshrink zeroes
# everything.  Scaled: projections span +-1.3, the discriminator -2.5 .. 1.8.
MODEL_KINKS = {"hardtanh": (-1.0, 1.0), "hardshrink": (-0.5, 0.5)}       # where the VALUE or the derivative jumps by a constant
_MODEL_CASES = {}


def model_case(act):
    """(cfg, P, batch, o, L, G): built once per activation and shared, never changed"""
    if act not in _MODEL_CASES:
        cfg = orc.default_config(vocab_size=40, use_cmd_sim=False, use_confidNet=True, activation=act)
        P = orc.synth_params(cfg, 3)
        for m in "tva":
            for s in ("weight", "bias"):
                P[f"project_{m}.project_{m}.{s}"] = P[f"project_{m}.project_{m}.{s}"] * 4
        for s in ("weight", "bias"):
            P[f"discriminator.discriminator_layer_1.{s}"] = P[f"discriminator.discriminator_layer_1.{s}"] * 2
        batch = orc.synth_batch(cfg, 8, 6, 11, ragged=True)
        o, L, G = orc.loss_and_grads(P, cfg, batch)
        # precondition, on the oracle's own pre-activations: nothing within 1e-4 of a jump (~100x the fp32 rounding of a 512-term sum of
        # order 1), so no element may legitimately land on the other side on the device, and nothing is masked
        with torch.no_grad():
            zp = torch.cat([orc._linear(getattr(o, f"utterance_{m}"), P, f"project_{m}.project_{m}") for m in "tva"])
            zd = torch.cat([orc._linear(getattr(o, f"utt_shared_{m}"), P, "discriminator.discriminator_layer_1") for m in "tva"])
        for z in (zp, zd):
            for k in MODEL_KINKS.get(act, ()):
                assert float((z - k).abs().min()) >= 1e-4, (act, k)
        if act == "hardtanh":
            assert bool((zp.abs() > 1).any()) and bool((zd.abs() > 1).any())
        if act == "hardshrink":
            assert 0.05 < float((zp.abs() > 0.5).float().mean()) < 0.95
        _MODEL_CASES[act] = (cfg, P, batch, o, L, G)
    return _MODEL_CASES[act]


def load_model(cfg, P, precision):
    from mmda_amd import make_config, MISA
    c = make_config(precision=precision, device="cuda:0", **vars(cfg))
    m = MISA(c)
    missing = m.load_state_dict(P, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    m.to("cuda:0")
    return m, c


def to_dev(batch):
    return {k: (v.to("cuda:0") if k != "l" else v) for k, v in batch.items()}


@pytest.mark.parametrize("path", ["fused", "statement_order"])
@pytest.mark.parametrize("act", ["leakyrelu", "elu", "tanh", "hardtanh", "hardshrink"])       # leakyrelu: the control
def test_whole_model_fp32_each_unparametrised_activation(act, path):
    cfg, P, batch, o, L, G = model_case(act)
    model, c = load_model(cfg, P, "fp32")
    b = to_dev(batch)
    if path == "fused":
        model.train_step(b["t"], b["v"], b["a"], b["l"], b["emo"], lr=cfg.learning_rate, clip=cfg.clip, do_adam=False, training=False)
        assert not model.cluster_aborted()
        pub = model._public()
        assert_outputs_and_losses_match_oracle(pub["scores"], pub["tcp"], model.read_losses(), o, L, 1e-4)
        model._assign_grad_views()
    else:
        from mmda_amd.solver import Solver
        model.eval()
        solver = Solver(c, c, c, None, None, None, is_train=True, model=model)
        scores, _ = model(b["t"], b["v"], b["a"], b["l"], None, None, None)
        Lt, total = statement_order_losses(solver, cfg, scores, b["emo"])
        losses = {k: v.item() for k, v in Lt.items()}
        losses["total"] = total.item()
        assert_outputs_and_losses_match_oracle(scores, model.tcp, losses, o, L, 1e-4)
        model.zero_grad()
        total.backward()
    assert_grads_match_oracle(model, G, 2e-4)


@pytest.mark.parametrize("act", ["leakyrelu", "elu", "tanh"])
def test_whole_model_bf16_each_smooth_activation(act):
    """Bounds as test_degenerate_shapes_against_the_oracle: 1e-2 on outputs and losses, 2e-1 relative L2 on gradients.  hardtanh and
    hardshrink are left out on purpose: a pre-activation error of 1e-2 moves dozens of elements across a jump of 0.5, which is the
    activation's nature and no kernel's error."""
    cfg, P, batch, o, L, G = model_case(act)
    model, c = load_model(cfg, P, "bf16")
    b = to_dev(batch)
    model.train_step(b["t"], b["v"], b["a"], b["l"], b["emo"], lr=cfg.learning_rate, clip=cfg.clip, do_adam=False, training=False)
    assert not model.cluster_aborted()
    pub = model._public()
    assert_outputs_and_losses_match_oracle(pub["scores"], pub["tcp"], model.read_losses(), o, L, 1e-2)
    model._assign_grad_views()
    assert_grads_match_oracle(model, G, 2e-1)
