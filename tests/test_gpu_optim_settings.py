"""GPU: the optimizer you constructed is the optimizer that steps -- betas, eps, weight decay (L2 and decoupled), a changing lr and
clip_grad_norm_, from the launches up to ``Solver``.  The reference for the arithmetic is torch.optim.Adam / AdamW /
torch.nn.utils.clip_grad_norm_ on the CPU, run here; between two paths of this package that run the same functor on the same
gradients the comparison is torch.equal.  Op-level inputs follow tests/golden/gen_optim_bits.py: n in {1031, 3, 4}, gradients uniform
in +-3, grad_scale 0.5, clip 1, p ~ N(0, 1)."""
import importlib.util
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import misa_oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("gen_optim_bits", os.path.join(GOLDEN, "gen_optim_bits.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

DEV = "cuda:0"
LR, CLIP, SCALE = gen.LR, gen.CLIP, gen.SCALE
TOL = 2e-6                                                   # what tests/test_gpu_ops.py holds plain Adam to against torch fp32
ULP = 2.0 ** -23
# (name, weight_decay, decoupled, betas, eps, lr)
DECAY_CASES = [("l2", 0.1, False, (0.9, 0.999), 1e-8, 1e-3), ("decoupled", 0.1, True, (0.9, 0.999), 1e-8, 1e-3),
               ("l2_betas", 0.1, False, (0.8, 0.95), 1e-6, 3e-3), ("decoupled_betas", 0.1, True, (0.8, 0.95), 1e-6, 3e-3)]


def _inputs(n, steps, seed):
    rng = np.random.default_rng(seed)
    f32 = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    p = f32(rng.standard_normal(n))
    g = [f32(rng.uniform(-3.0, 3.0, n)) for _ in range(steps)]
    acc = f32(rng.uniform(-3.0, 3.0, n))
    return p, g, acc


def _torch_opt(p, wd, decoupled, betas, eps, lr):
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    return cls([p], lr=lr, betas=betas, eps=eps, weight_decay=wd)


# ================================================================================================ 1: arithmetic against torch
@pytest.mark.parametrize("case", DECAY_CASES, ids=[c[0] for c in DECAY_CASES])
@pytest.mark.parametrize("n", gen.DENSE_N)
def test_decayed_adam_against_torch(n, case):
    """Six steps, lr halved every two; parameters and both moments within 2e-6 of torch's fp32 optimizer on the CPU."""
    from mmda_amd import ops
    _, wd, decoupled, betas, eps, lr0 = case
    p0, gs, _ = _inputs(n, 6, 100 + n)
    ref = torch.nn.Parameter(p0.clone())
    opt = _torch_opt(ref, wd, decoupled, betas, eps, lr0)
    p, m, v = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    for s in range(1, 7):
        lr = lr0 * 0.5 ** ((s - 1) // 2)
        opt.param_groups[0]["lr"] = lr
        ref.grad = (gs[s - 1] * SCALE).clamp(-CLIP, CLIP)
        opt.step()
        ops.clamp_adam_opts(p, gs[s - 1].to(DEV), m, v, lr, s, clip=CLIP, grad_scale=SCALE, betas=betas, eps=eps, weight_decay=wd,
                            decoupled=decoupled)
    st = opt.state[ref]
    for name, got, want in (("p", p, ref.detach()), ("m", m, st["exp_avg"]), ("v", v, st["exp_avg_sq"])):
        err = float((got.cpu() - want).abs().max())
        print(f"{case[0]} n={n} {name}: max err {err:.3e}")
        assert err < TOL, (name, err)
    # decay did something: the undecayed rule ends elsewhere
    q, m2, v2 = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    for s in range(1, 7):
        ops.clamp_adam_opts(q, gs[s - 1].to(DEV), m2, v2, lr0 * 0.5 ** ((s - 1) // 2), s, clip=CLIP, grad_scale=SCALE, betas=betas, eps=eps)
    assert not torch.equal(q, p)


def test_no_decay_no_scale_is_the_plain_launch():
    """weight_decay = 0 and no device scale through the new entry: the bits of mmda_clamp_adam / _sum."""
    from mmda_amd import ops
    n = 1031
    p0, gs, acc = _inputs(n, 1, 7)
    for a in (None, acc.to(DEV)):
        x = [p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)]
        y = [p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)]
        ops.clamp_adam_opts(x[0], gs[0].to(DEV), x[1], x[2], LR, 2, clip=CLIP, grad_scale=SCALE, betas=(0.8, 0.95), eps=1e-6, acc=a)
        ops.clamp_adam_sum(y[0], a, gs[0].to(DEV), y[1], y[2], LR, 2, clip=CLIP, grad_scale=SCALE, betas=(0.8, 0.95), eps=1e-6)
        assert all(torch.equal(s, t) for s, t in zip(x, y))


# ================================================================================================ 2: layouts agree
def _kw(decoupled, scale_dev):
    return dict(clip=CLIP, grad_scale=SCALE, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.1, decoupled=decoupled, scale_dev=scale_dev)


@pytest.mark.parametrize("decoupled", [False, True], ids=["l2", "decoupled"])
@pytest.mark.parametrize("n", gen.DENSE_N)
def test_dense_and_full_run_table_agree(n, decoupled):
    from mmda_amd import ops
    p0, gs, acc = _inputs(n, 1, 200 + n)
    g, acc = gs[0].to(DEV), acc.to(DEV)
    coef = torch.tensor([0.625], device=DEV)
    runs = ops.runs_table([(0, n)], n, DEV)
    for a in (None, acc):
        for sd in (None, coef):
            x = [p0.to(DEV), torch.full((n,), 0.05, device=DEV), torch.full((n,), 1e-3, device=DEV)]
            y = [t.clone() for t in x]
            ops.clamp_adam_opts(x[0], g, x[1], x[2], LR, 3, acc=a, **_kw(decoupled, sd))
            ops.clamp_adam_opts(y[0], g, y[1], y[2], LR, 3, acc=a, runs=runs, **_kw(decoupled, sd))
            assert all(torch.equal(s, t) for s, t in zip(x, y)), (a is not None, sd is not None)
            assert not torch.equal(x[0].cpu(), p0)
    # the device scale is a factor of grad_scale, rounded once: the host-side product gives the same launch
    x = [p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)]
    y = [t.clone() for t in x]
    ops.clamp_adam_opts(x[0], g, x[1], x[2], LR, 1, **_kw(decoupled, coef))
    kw = _kw(decoupled, None)
    kw["grad_scale"] = float(np.float32(SCALE) * np.float32(0.625))
    ops.clamp_adam_opts(y[0], g, y[1], y[2], LR, 1, **kw)
    assert all(torch.equal(s, t) for s, t in zip(x, y))


@pytest.mark.parametrize("decoupled", [False, True], ids=["l2", "decoupled"])
@pytest.mark.parametrize("D", [300, 7])
def test_rows_form_with_every_row_agrees_with_dense(D, decoupled):
    """width 300: whole quads, a lane takes two; width 7: the scalar form.  mask all ones, want 1: every row; want 0: nothing."""
    from mmda_amd import ops
    V = 37
    rng = np.random.default_rng(D)
    f32 = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)
    p0, g = f32(rng.standard_normal((V, D))), f32(rng.uniform(-3.0, 3.0, (V, D)))
    m0, v0 = f32(0.1 * rng.standard_normal((V, D))), f32(rng.uniform(0.0, 1e-2, (V, D)))
    coef = torch.tensor([0.625], device=DEV)
    mask = torch.ones(V, dtype=torch.uint8, device=DEV)
    for sd in (None, coef):
        x = [p0.clone(), m0.clone(), v0.clone()]
        y = [p0.clone(), m0.clone(), v0.clone()]
        ops.clamp_adam_opts(x[0].view(-1), g.view(-1), x[1].view(-1), x[2].view(-1), LR, 3, **_kw(decoupled, sd))
        ops.clamp_adam_rows_opts(y[0], g, y[1], y[2], mask, 0, LR, 3, **_kw(decoupled, sd))
        assert torch.equal(y[0], p0) and torch.equal(y[1], m0) and torch.equal(y[2], v0)
        ops.clamp_adam_rows_opts(y[0], g, y[1], y[2], mask, 1, LR, 3, **_kw(decoupled, sd))
        assert all(torch.equal(s, t) for s, t in zip(x, y)), sd is not None
        assert not torch.equal(x[0], p0)


@pytest.mark.parametrize("decoupled", [False, True], ids=["l2", "decoupled"])
def test_run_ranges_touch_nothing_outside(decoupled):
    """gen_optim_bits.run_ranges(1063), NaN in p, g, acc, m, v outside the runs: the dense launch's bits inside, NaN still outside."""
    from mmda_amd import ops
    n = gen.RUNS_N
    ranges = gen.run_ranges(n)
    mask = torch.zeros(n, dtype=torch.bool)
    for b, l in ranges:
        mask[b:b + l] = True
    mask = mask.to(DEV)
    assert 0 < int(mask.sum()) < n
    p0, gs, acc = _inputs(n, 1, 300)
    runs = ops.runs_table(ranges, n, DEV)
    coef = torch.tensor([0.625], device=DEV)
    nan = torch.full((n,), float("nan"), device=DEV)
    hole = lambda t: torch.where(mask, t.to(DEV), nan)
    for with_acc in (False, True):
        a = acc.to(DEV) if with_acc else None
        x = [p0.to(DEV), torch.full((n,), 0.05, device=DEV), torch.full((n,), 1e-3, device=DEV)]
        y = [hole(t) for t in x]
        g_nan, a_nan = hole(gs[0]), (hole(acc) if with_acc else None)
        ops.clamp_adam_opts(x[0], gs[0].to(DEV), x[1], x[2], LR, 3, acc=a, **_kw(decoupled, coef))
        ops.clamp_adam_opts(y[0], g_nan, y[1], y[2], LR, 3, acc=a_nan, runs=runs, **_kw(decoupled, coef))
        for s, t in zip(x, y):
            assert torch.equal(s[mask], t[mask]) and bool(torch.isnan(t[~mask]).all()) and not bool(torch.isnan(t[mask]).any())


# ================================================================================================ 3: the norm
def _norm_ref(x, gscale, max_norm):
    ref = gscale * float(x.double().pow(2).sum().sqrt())
    return ref, min(1.0, max_norm / (ref + 1e-6))


def _check_norm(out, x, gscale, max_norm, what):
    ref, cref = _norm_ref(x, gscale, max_norm)
    got, coef = (float(t) for t in out.cpu())
    print(f"{what}: norm {got!r} ref {ref!r} rel {abs(got - ref) / ref:.3e}; coef {coef!r} ref {cref!r}")
    assert abs(got - ref) <= ULP * ref, (what, got, ref)
    assert abs(coef - cref) <= 4 * ULP * cref, (what, coef, cref)
    return coef


def _norm_inputs(n):
    if n == gen.LARGE_N:
        _, acc, g, _, _ = gen.large_inputs(n)                # exact small integers over 1024
        return g, acc
    _, gs, acc = _inputs(n, 1, 400 + n)
    return gs[0].to(DEV), acc.to(DEV)


@pytest.mark.parametrize("gscale", [1.0, 0.5])
@pytest.mark.parametrize("n", gen.DENSE_N + (gen.LARGE_N,))
def test_norm_dense(n, gscale):
    """within one fp32 ulp of the float64 norm of the same fp32 inputs (double accumulation of exact squares, one final rounding); the
    coefficient within 4 ulps; one max_norm that clips and one that does not; two launches give equal bits"""
    from mmda_amd import ops
    g, acc = _norm_inputs(n)
    for what, a, x in (("g", None, g), ("acc+g", acc, acc + g)):
        ref, _ = _norm_ref(x, gscale, 1.0)
        out = ops.grad_norm(g, 0.5 * ref, grad_scale=gscale, acc=a)
        assert _check_norm(out, x, gscale, 0.5 * ref, f"n={n} {what} clipping") < 1.0
        again = ops.grad_norm(g, 0.5 * ref, grad_scale=gscale, acc=a)
        assert torch.equal(out.view(torch.int32), again.view(torch.int32))
        out = ops.grad_norm(g, 2.0 * ref, grad_scale=gscale, acc=a)
        assert _check_norm(out, x, gscale, 2.0 * ref, f"n={n} {what} not clipping") == 1.0


@pytest.mark.parametrize("gscale", [1.0, 0.5])
@pytest.mark.parametrize("n", [gen.RUNS_N, gen.LARGE_N])
def test_norm_over_runs_ignores_what_lies_outside(n, gscale):
    from mmda_amd import ops
    ranges = gen.run_ranges(n)
    mask = torch.zeros(n, dtype=torch.bool, device=DEV)
    for b, l in ranges:
        mask[b:b + l] = True
    runs = ops.runs_table(ranges, n, DEV)
    g, acc = _norm_inputs(n)
    nan = torch.full((n,), float("nan"), device=DEV)
    g_nan, a_nan = torch.where(mask, g, nan), torch.where(mask, acc, nan)
    for what, a, x in (("g", None, g[mask]), ("acc+g", a_nan, (acc + g)[mask])):
        ref, _ = _norm_ref(x, gscale, 1.0)
        out = ops.grad_norm(g_nan, 0.5 * ref, grad_scale=gscale, acc=a, runs=runs)
        assert _check_norm(out, x, gscale, 0.5 * ref, f"runs n={n} {what} clipping") < 1.0
        again = ops.grad_norm(g_nan, 0.5 * ref, grad_scale=gscale, acc=a, runs=runs)
        assert torch.equal(out.view(torch.int32), again.view(torch.int32))
        out = ops.grad_norm(g_nan, 2.0 * ref, grad_scale=gscale, acc=a, runs=runs)
        assert _check_norm(out, x, gscale, 2.0 * ref, f"runs n={n} {what} not clipping") == 1.0


@pytest.mark.parametrize("n", gen.DENSE_N)
def test_norm_of_a_zero_gradient(n):
    """norm 0, coefficient 1 -- for zeros, and for a run table with nothing in it (nothing trains: no float is loaded)"""
    from mmda_amd import ops
    assert ops.grad_norm(torch.zeros(n, device=DEV), 1.0).cpu().tolist() == [0.0, 1.0]
    empty = ops.runs_table([], n, DEV)
    assert ops.grad_norm(torch.full((n,), float("nan"), device=DEV), 1.0, runs=(empty[0], 0, 0)).cpu().tolist() == [0.0, 1.0]


@pytest.mark.parametrize("n", [gen.DENSE_N[0], gen.RUNS_N])
def test_grad_scale_in_place(n):
    """g *= coef: torch's g.mul_(clip_coef); over runs, nothing outside them is touched"""
    from mmda_amd import ops
    _, gs, _ = _inputs(n, 1, 500 + n)
    g = gs[0].to(DEV)
    coef = torch.tensor([7.0, 0.3], device=DEV)
    if n == gen.RUNS_N:
        ranges = gen.run_ranges(n)
        mask = torch.zeros(n, dtype=torch.bool, device=DEV)
        for b, l in ranges:
            mask[b:b + l] = True
        x = torch.where(mask, g, torch.full_like(g, float("nan")))
        ops.grad_scale_(x, coef[1:], runs=ops.runs_table(ranges, n, DEV))
        assert torch.equal(x[mask], (g * coef[1])[mask]) and bool(torch.isnan(x[~mask]).all())
    else:
        x = g.clone()
        ops.grad_scale_(x, coef[1:])
        assert torch.equal(x, g * coef[1])


# ================================================================================================ 4: clip_grad_norm_ + step against torch
@pytest.mark.parametrize("n", gen.DENSE_N)
def test_norm_clip_then_adamw_against_torch(n):
    """torch: clip_grad_norm_, clip_grad_value_, AdamW.step() on the CPU; here: the norm launch, then the update with the coefficient
    read from device memory.  Three steps, the bound of test 1.  The in-place scale followed by the plain launch gives the same bits."""
    from mmda_amd import ops
    wd, betas, eps = 0.1, (0.9, 0.999), 1e-8
    p0, gs, _ = _inputs(n, 3, 600 + n)
    max_norm = 0.35 * float(gs[0].norm())                  # clips the norm; the value clip at 1 then still bites on some elements
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([ref], lr=LR, betas=betas, eps=eps, weight_decay=wd)
    x = [p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)]
    y = [t.clone() for t in x]
    for s in (1, 2, 3):
        ref.grad = gs[s - 1].clone()
        total = torch.nn.utils.clip_grad_norm_([ref], max_norm)
        assert float(total) > max_norm
        torch.nn.utils.clip_grad_value_([ref], CLIP)
        opt.step()
        g = gs[s - 1].to(DEV)
        out = ops.grad_norm(g, max_norm)
        assert abs(float(out[0]) - float(total)) <= 64 * ULP * float(total)        # (torch's norm is an fp32 sum)
        ops.clamp_adam_opts(x[0], g, x[1], x[2], LR, s, clip=CLIP, betas=betas, eps=eps, weight_decay=wd, decoupled=True, scale_dev=out[1:])
        g2 = g.clone()
        ops.grad_scale_(g2, out[1:])
        ops.clamp_adam_opts(y[0], g2, y[1], y[2], LR, s, clip=CLIP, betas=betas, eps=eps, weight_decay=wd, decoupled=True)
        assert all(torch.equal(a, b) for a, b in zip(x, y)), s
    st = opt.state[ref]
    for name, got, want in (("p", x[0], ref.detach()), ("m", x[1], st["exp_avg"]), ("v", x[2], st["exp_avg_sq"])):
        err = float((got.cpu() - want).abs().max())
        print(f"n={n} {name}: max err {err:.3e}")
        assert err < TOL, (name, err)


# ================================================================================================ model level
class ListLoader:
    def __init__(self, batches):
        self.batches = batches
        self.dataset = self

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


def _tuple_of(b):
    B = b["t"].shape[1]
    z = torch.zeros(B, b["t"].shape[0] + 2, dtype=torch.int64)
    return (b["t"], b["v"], b["a"], torch.zeros(B), b["emo"], b["l"], z, z, z, [f"s{i}" for i in range(B)])


def _model(precision="fp32", **kw):
    from mmda_amd import make_config, MISA
    cfg = orc.default_config(vocab_size=120)
    m = MISA(make_config(precision=precision, device=DEV, **kw, **vars(cfg)))
    m.load_state_dict(orc.synth_params(cfg, 21))
    m.to(DEV)
    m._materialize(torch.device(DEV))
    return m, cfg


def _step(m, b, lr=LR, **kw):
    kw.setdefault("training", True)
    m.train_step(b["t"].to(DEV), b["v"].to(DEV), b["a"].to(DEV), b["l"], b["emo"].to(DEV), lr=lr, clip=CLIP, **kw)


def _state(m):
    P, _, M, V = m.flat_buckets()
    torch.cuda.synchronize()
    return [x.detach().cpu().clone() for x in (P, M, V)]


def _assert_state_equal(a, b, what=""):
    for name, x, y in zip("PMV", a, b):
        bad = int((x != y).sum())
        assert bad == 0, (what, name, bad, float((x - y).abs().max()))


def _opt(m, cls_name, **kw):
    from mmda_amd import optim
    return getattr(optim, cls_name)([p for p in m.parameters() if p.requires_grad], lr=LR, **kw).attach(m)


def _batches(cfg, k=3, seed=60):
    shapes = [(6, 6), (8, 6), (5, 6), (7, 6)]
    return [orc.synth_batch(cfg, B, T, seed + i, ragged=True) for i, (B, T) in enumerate(shapes[:k])]


def _bucket_norm(m, b):
    """the gradient norm of batch ``b`` at the model's current weights (a step without its optimizer on a throw-away twin)"""
    from mmda_amd import ops
    _step(m, b, do_adam=False, seed=5)
    return float(ops.grad_norm(m.flat_buckets()[1], 1.0)[0])


def _unfused_step(m, opt, b, seed, k, clip_norm, lr=LR):
    """the reference's order, by hand: backward, clip_grad_norm_, clip_grad_value_ + step (one fused launch)"""
    from mmda_amd import optim
    _step(m, b, do_adam=False, seed=seed)
    norm = None
    if clip_norm is not None:
        norm = optim.clip_grad_norm_(m, clip_norm)
    m._step = k - 1                                          # (the step without its optimizer counted itself: this is update k)
    opt.param_groups[0]["lr"] = lr
    opt.step(clip_value=CLIP)
    return norm


# (name, optimizer class, its kwargs, whether the norm is clipped)
FUSED_CASES = [("default", "Adam", {}, False), ("betas", "Adam", dict(betas=(0.8, 0.95), eps=1e-6), False),
               ("l2", "Adam", dict(weight_decay=0.1), False), ("adamw", "AdamW", dict(weight_decay=0.1), False),
               ("norm", "Adam", {}, True), ("adamw_norm", "AdamW", dict(weight_decay=0.1), True)]


# ------------------------------------------------------------------------------------------------ 5: fused = unfused
@pytest.mark.parametrize("case", FUSED_CASES, ids=[c[0] for c in FUSED_CASES])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_fused_step_equals_unfused_step(precision, case):
    """Three train_step(optimizer=..., clip_norm=...) against three train_step(do_adam=False) + clip_grad_norm_ + optimizer.step() on a
    twin: the same functor on the same deterministic gradient bucket, so parameters and both moments are equal bit for bit.  'default'
    is plain Adam, which holds this without any of the new settings (the launches it makes are the ones it has always made)."""
    _, cls, kw, clipped = case
    m, cfg = _model(precision)
    twin, _ = _model(precision)
    batches = _batches(cfg)
    clip_norm = None
    if clipped:
        probe, _ = _model(precision)
        clip_norm = 0.5 * _bucket_norm(probe, batches[0])
        del probe
    om, ot = _opt(m, cls, **kw), _opt(twin, cls, **kw)
    start = _state(m)
    for k, b in enumerate(batches, 1):
        _step(m, b, optimizer=om, clip_norm=clip_norm, seed=70 + k)
        norm = _unfused_step(twin, ot, b, 70 + k, k, clip_norm)
        assert m._step == twin._step == k
        if clipped:
            assert torch.equal(m.grad_norm().cpu(), norm.cpu())
            assert k > 1 or float(norm) > clip_norm          # (it bites: the first batch by construction)
        _assert_state_equal(_state(m), _state(twin), (case[0], k))
    assert not torch.equal(_state(m)[0], start[0]) and not m.cluster_aborted()
    if case[0] != "default":
        # ... and the setting reached the fused step: plain Adam from the same start ends elsewhere
        plain, _ = _model(precision)
        for k, b in enumerate(batches, 1):
            _step(plain, b, seed=70 + k)
        assert not torch.equal(_state(plain)[0], _state(m)[0])


# (name, model kwargs, parameters frozen by requires_grad, whether the norm is clipped)
TAIL_CASES = [("dense", {}, (), False), ("dense_norm", {}, (), True), ("sparse", dict(embed_update="sparse"), (), False),
              ("frozen", dict(embed_update="frozen"), (), False), ("frozen_norm", dict(embed_update="frozen"), (), True),
              ("masked", {}, ("trnn1", "project_v"), False), ("masked_norm", {}, ("trnn1", "project_v"), True)]


@pytest.mark.parametrize("case", TAIL_CASES, ids=[c[0] for c in TAIL_CASES])
def test_the_three_native_tails_give_the_same_bits(case):
    """One batch at B = 8, T = 12 through each native entry that issues the optimizer part of a step: the fused train_step; train_step
    without its optimizer, then mmda_misa_adam_step; the same, then mmda_misa_adam_step_accumulated with no accumulator.  The update is
    an element function of the same gradient bucket (where the bucket is split between the early pass and the rest does not enter it),
    and the sparse table's rows sum in list order on every path: parameters and both moments are equal bit for bit."""
    from mmda_amd import _lib
    _, mkw, frozen, clipped = case
    models = [_model("fp32", **mkw) for _ in range(3)]
    cfg = models[0][1]
    fused, stepped, closed = (m for m, _ in models)
    b = orc.synth_batch(cfg, 8, 12, 64, ragged=True)
    for m in (fused, stepped, closed):
        if frozen:
            m.freeze(*frozen)
    clip_norm = None
    if clipped:
        probe, _ = _model("fp32", **mkw)
        clip_norm = 0.5 * _bucket_norm(probe, b)
        del probe
    start = _state(fused)
    _step(fused, b, clip_norm=clip_norm, seed=9)
    lib, s = fused._lib, _lib.stream_ptr()
    _step(stepped, b, clip_norm=clip_norm, do_adam=False, seed=9)
    _lib.check(lib.mmda_misa_adam_step(stepped._h, LR, CLIP, 1.0, 1, s), "adam_step")
    _step(closed, b, clip_norm=clip_norm, do_adam=False, seed=9)
    ids = rows = None
    R = b["t"].numel()
    if closed.embed_update == "sparse":
        ids = torch.empty(R, dtype=torch.int64, device=DEV)
        rows = torch.empty(R, closed.embed.weight.shape[1], dtype=torch.float32, device=DEV)
    _lib.check(lib.mmda_misa_adam_step_accumulated(closed._h, None, _lib.ptr(ids), _lib.ptr(rows), 0, R if ids is not None else 0,
                                                   LR, CLIP, 1.0, 1, s), "adam_step_accumulated")
    assert fused._step == stepped._step == closed._step == 1
    for other, what in ((stepped, "adam_step"), (closed, "adam_step_accumulated")):
        _assert_state_equal(_state(fused), _state(other), (case[0], what))
        if clipped:
            assert torch.equal(fused.grad_norm().cpu(), other.grad_norm().cpu()) and float(fused.grad_norm()) > clip_norm
    assert not torch.equal(_state(fused)[0], start[0]) and not fused.cluster_aborted()


# ------------------------------------------------------------------------------------------------ 6: the other paths
def test_accumulated_steps_through_solver():
    """accum_steps = 2 over three batches (steps of 2 and 1) with AdamW and a norm clip, dropout on, against the manual path: the
    micro-batches without their optimizer, their sum written into the bucket by torch, the norm of that sum scaled by 1/N, one launch."""
    from mmda_amd import make_config, models, ops
    from mmda_amd.solver import Solver
    cfg = orc.default_config(vocab_size=120, learning_rate=LR, clip=CLIP)
    train = _batches(cfg)
    probe, _ = _model("fp32")
    clip_norm = 0.5 * _bucket_norm(probe, train[2])
    c = make_config(precision="fp32", device=DEV, n_epoch=1, name="optset", accum_steps=2, optimizer="AdamW",
                    optimizer_kwargs=dict(betas=(0.8, 0.95), eps=1e-6), weight_decay=0.1, clip_norm=clip_norm, **vars(cfg))
    m = models.MISA(c)
    m.load_state_dict(orc.synth_params(cfg, 21))
    s = Solver(c, c, c, ListLoader([_tuple_of(b) for b in train]), ListLoader([]), ListLoader([]), is_train=True, model=m).build()
    assert s.optimizer.settings() == (0.8, 0.95, 1e-6, 0.1, True)       # AdamW takes cfg.weight_decay
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    s.train_epoch()
    assert m._step == 2

    hand = models.MISA(c)
    hand.load_state_dict(sd)
    hand.to(DEV)
    hand._materialize(torch.device(DEV))
    oh = _opt(hand, "AdamW", betas=(0.8, 0.95), eps=1e-6, weight_decay=0.1)
    G = hand.flat_buckets()[1]
    for k, group in enumerate(([train[0], train[1]], [train[2]]), 1):
        total = None
        for b in group:
            _step(hand, b, do_adam=False)                    # (draws the seed the solver's micro-batch drew)
            total = G.clone() if total is None else total + G
        G.copy_(total)
        out = ops.grad_norm(G, clip_norm, grad_scale=1.0 / len(group))
        hand._step = k - 1
        oh.step(clip_value=CLIP, grad_scale=1.0 / len(group), scale_dev=out[1:])
        if k == 2:
            assert torch.equal(m.grad_norm().cpu(), out[0].cpu()) and float(out[0]) > clip_norm
    _assert_state_equal(_state(m), _state(hand))


CUT = ("trnn1", "trnn2", "vrnn1", "vrnn2", "arnn1", "arnn2", "tlayer_norm", "vlayer_norm", "alayer_norm", "embed")


def _tensor_ranges(m, frozen):
    names = m._native_names
    offs = [m._layout[n][0] for n in names] + [m._flat_floats]
    return [(n, offs[i], offs[i + 1]) for i, n in enumerate(names) if m._get(n).requires_grad != frozen]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_encoder_cut_decays_and_measures_trainable_runs_only(precision):
    """freeze(...) with AdamW and a norm clip: frozen tensors and their moments keep their bits, and NaN in their gradient slots does
    not reach the norm."""
    from mmda_amd import optim
    m, cfg = _model(precision)
    twin, _ = _model(precision)
    for x in (m, twin):
        assert x.freeze(*CUT)
    batches = _batches(cfg)
    probe, _ = _model(precision)
    probe.freeze(*CUT)
    clip_norm = 0.5 * _bucket_norm(probe, batches[0])
    om, ot = _opt(m, "AdamW", weight_decay=0.1), _opt(twin, "AdamW", weight_decay=0.1)
    start = _state(m)
    frozen, live = _tensor_ranges(m, True), _tensor_ranges(m, False)
    assert frozen and live
    for k, b in enumerate(batches, 1):
        _step(m, b, optimizer=om, clip_norm=clip_norm, seed=80 + k)
        _step(twin, b, do_adam=False, seed=80 + k)
        G = twin.flat_buckets()[1]
        for _, b0, e0 in frozen:
            G[b0:e0] = float("nan")
        norm = optim.clip_grad_norm_(twin, clip_norm)
        assert torch.isfinite(norm) and torch.equal(norm.cpu(), m.grad_norm().cpu())
        assert bool(torch.isnan(G[frozen[0][1]:frozen[0][2]]).all())                  # the scale touched nothing outside the runs
        twin._step = k - 1
        ot.step(clip_value=CLIP)
        _assert_state_equal(_state(m), _state(twin), k)
    end = _state(m)
    for _, b0, e0 in frozen:
        assert all(torch.equal(x[b0:e0], y[b0:e0]) for x, y in zip(end, start))
    assert sum(not torch.equal(end[0][b0:e0], start[0][b0:e0]) for _, b0, e0 in live) > len(live) // 2
    assert not any(bool(torch.isnan(x).any()) for x in end)


def _samples_of(b):
    out = []
    for i, L in enumerate(b["l"].tolist()):
        lab = np.concatenate([[0.0], b["emo"][i].numpy()]).astype(np.float32)[None]
        out.append(((b["t"][:L, i].numpy(), b["v"][:L, i].numpy(), b["a"][:L, i].numpy(), ["w"] * L), lab, f"seg{i}"))
    return out


def test_step_from_the_encoder_cache_takes_the_settings():
    """train_step_encoded against the cut step from the batch itself, both with AdamW, other betas and a norm clip: equal bits"""
    from mmda_amd import DeviceDataset, EncodedLoader, EncoderCache
    m, cfg = _model("bf16")
    twin, _ = _model("bf16")
    for x in (m, twin):
        x.freeze(*CUT)
    b = _batches(cfg)[1]
    B = b["t"].shape[1]
    probe, _ = _model("bf16")
    probe.freeze(*CUT)
    clip_norm = 0.5 * _bucket_norm(probe, b)
    kw = dict(betas=(0.8, 0.95), eps=1e-6, weight_decay=0.1)
    om, ot = _opt(m, "AdamW", **kw), _opt(twin, "AdamW", **kw)
    cache = EncoderCache.build(m, DeviceDataset.from_samples(_samples_of(b), DEV), B, order="dataset")
    (eb,) = list(EncodedLoader(cache, B))
    for k in (1, 2):
        m.train_step_encoded(eb, lr=LR, clip=CLIP, optimizer=om, clip_norm=clip_norm, seed=90 + k, training=False)
        _step(twin, b, optimizer=ot, clip_norm=clip_norm, seed=90 + k, training=False)
        assert torch.equal(m.grad_norm().cpu(), twin.grad_norm().cpu()) and (k > 1 or float(m.grad_norm()) > clip_norm)
        _assert_state_equal(_state(m), _state(twin), k)
    plain, _ = _model("bf16")
    plain.freeze(*CUT)
    for k in (1, 2):
        _step(plain, b, seed=90 + k, training=False)
    assert not torch.equal(_state(plain)[0], _state(m)[0])


@pytest.mark.parametrize("cls", ["Adam", "AdamW"])
def test_sparse_table_is_not_decayed(cls):
    """embed_update='sparse' with decay: the dense prefix decays, the table's rows follow SparseAdam, which has none -- after one step
    from the same start the table and its moments equal the run without decay bit for bit, and the prefix does not."""
    m, cfg = _model("fp32", embed_update="sparse")
    ref, _ = _model("fp32", embed_update="sparse")
    b = _batches(cfg)[0]
    _step(m, b, optimizer=_opt(m, cls, weight_decay=0.1), seed=3)
    _step(ref, b, optimizer=_opt(ref, "Adam"), seed=3)
    off = m._layout["embed.weight"][0]
    a, r = _state(m), _state(ref)
    for x, y in zip(a, r):
        assert torch.equal(x[off:], y[off:])
    assert not torch.equal(a[0][:off], r[0][:off])
    assert not torch.equal(a[0][off:], _state(_model("fp32", embed_update="sparse")[0])[0][off:])       # (rows did move)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_deferred_table_with_other_betas_and_a_changing_lr(precision):
    """embed_update='deferred' replays with the optimizer's betas / eps and each update's own step_size: after a flush the whole state
    equals embed_update='dense' under the same settings."""
    m, cfg = _model(precision, embed_update="deferred")
    dense, _ = _model(precision)
    kw = dict(betas=(0.8, 0.95), eps=1e-6)
    om, od = _opt(m, "Adam", **kw), _opt(dense, "Adam", **kw)
    for k, b in enumerate(_batches(cfg, 4), 1):
        lr = LR * 0.5 ** (k - 1)
        _step(m, b, lr=lr, optimizer=om, seed=20 + k)
        _step(dense, b, lr=lr, optimizer=od, seed=20 + k)
    m.flush_embedding()
    _assert_state_equal(_state(m), _state(dense))
    plain, _ = _model(precision)
    for k, b in enumerate(_batches(cfg, 4), 1):
        _step(plain, b, lr=LR * 0.5 ** (k - 1), seed=20 + k)
    assert not torch.equal(_state(plain)[0], _state(dense)[0])


# ------------------------------------------------------------------------------------------------ 7: schedules
def test_a_torch_scheduler_on_the_solvers_optimizer_sets_the_steps_lr():
    """StepLR(solver.optimizer, 1, 0.5) stepped after each of three epochs of two batches against explicit train_step(lr=...) with the
    halved values."""
    from mmda_amd import make_config, models
    from mmda_amd.solver import Solver
    cfg = orc.default_config(vocab_size=120, learning_rate=LR, clip=CLIP)
    train = _batches(cfg, 2)
    c = make_config(precision="bf16", device=DEV, n_epoch=1, name="sched", **vars(cfg))
    m = models.MISA(c)
    m.load_state_dict(orc.synth_params(cfg, 21))
    s = Solver(c, c, c, ListLoader([_tuple_of(b) for b in train]), ListLoader([]), ListLoader([]), is_train=True, model=m).build()
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    sched = torch.optim.lr_scheduler.StepLR(s.optimizer, 1, 0.5)
    lrs = []
    for _ in range(3):
        lrs.append(s.optimizer.param_groups[0]["lr"])
        s.train_epoch()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                  # (torch's "scheduler before optimizer.step()": the fused step is the step)
            sched.step()
    assert lrs == [LR, LR * 0.5, LR * 0.25] and m._step == 6

    hand = models.MISA(c)
    hand.load_state_dict(sd)
    hand.to(DEV)
    for lr in lrs:
        for b in train:
            _step(hand, b, lr=lr)
    _assert_state_equal(_state(m), _state(hand))
    flat = models.MISA(c)                                    # the schedule did something
    flat.load_state_dict(sd)
    flat.to(DEV)
    for _ in lrs:
        for b in train:
            _step(flat, b)
    assert not torch.equal(_state(flat)[0], _state(hand)[0])


# ------------------------------------------------------------------------------------------------ 8: refusals
REFUSALS = [("decay_deferred", dict(embed_update="deferred"), "AdamW", dict(weight_decay=0.1), None, False, "weight_decay"),
            ("norm_sparse", dict(embed_update="sparse"), "Adam", {}, 1.0, False, "clip_norm"),
            ("norm_deferred", dict(embed_update="deferred"), "Adam", {}, 1.0, False, "clip_norm"),
            ("norm_exchange", {}, "Adam", {}, 1.0, True, "gradient exchange")]


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_refusals_name_the_setting_and_leave_a_usable_model(case):
    from mmda_amd import _lib
    _, mkw, cls, okw, clip_norm, exchange, word = case
    m, cfg = _model("fp32", **mkw)
    never, _ = _model("fp32", **mkw)
    b = _batches(cfg)[0]
    before = _state(m)
    sync = (lambda G, n: 1.0) if exchange else None
    with pytest.raises(_lib.MMDAError, match=word):
        _step(m, b, optimizer=_opt(m, cls, **okw), clip_norm=clip_norm, grad_sync=sync, seed=1)
    assert m._step == 0
    _assert_state_equal(_state(m), before)
    _step(m, b, seed=2)
    _step(never, b, seed=2)
    for x in (m, never):
        if x.embed_update == "deferred":
            x.flush_embedding()
    _assert_state_equal(_state(m), _state(never))
    assert not torch.equal(_state(m)[0], before[0])


def test_native_step_refuses_before_any_launch():
    """the same combinations set on the handle directly: MMDA_EINVAL from the stepping entries, nothing changed, and NULL restores"""
    import ctypes
    from mmda_amd import _lib
    m, cfg = _model("fp32", embed_update="deferred")
    never, _ = _model("fp32", embed_update="deferred")
    b = _batches(cfg)[0]
    lib = _lib.load()
    for opts, clip_norm in ((_lib.AdamOpts(0.9, 0.999, 1e-8, 0.1, 1, None), 0.0), (_lib.AdamOpts(0.9, 0.999, 1e-8, 0.0, 0, None), 1.0)):
        before = _state(m)
        assert lib.mmda_misa_set_adam(m._h, ctypes.byref(opts), clip_norm) == 0
        with pytest.raises(_lib.MMDAError, match="-1"):
            _step(m, b, seed=1)
        _assert_state_equal(_state(m), before)
        m._step = 0
        assert lib.mmda_misa_set_adam(m._h, None, 0.0) == 0
    _step(m, b, seed=2)
    _step(never, b, seed=2)
    m.flush_embedding(); never.flush_embedding()
    _assert_state_equal(_state(m), _state(never))


def test_solver_build_refuses_by_name():
    from mmda_amd import _lib, make_config, models
    from mmda_amd.solver import Solver
    cfg = orc.default_config(vocab_size=120, learning_rate=LR, clip=CLIP)

    def solver(**kw):
        c = make_config(precision="fp32", device=DEV, n_epoch=1, name="refuse", **kw, **vars(cfg))
        return Solver(c, c, c, ListLoader([]), ListLoader([]), ListLoader([]), is_train=True, model=models.MISA(c))

    with pytest.raises(_lib.MMDAError, match="weight_decay"):
        solver(embed_update="deferred", optimizer="AdamW").build()
    with pytest.raises(_lib.MMDAError, match="clip_norm"):
        solver(embed_update="sparse", clip_norm=1.0).build()
    with pytest.raises(_lib.MMDAError, match="clip_norm"):
        solver(embed_update="deferred", clip_norm=1.0).build()
    with pytest.raises(_lib.MMDAError, match="clip_norm"):
        solver(optimizer="RMSprop", clip_norm=1.0).build()
    s = solver(embed_update="sparse", optimizer="AdamW").build()              # allowed: the prefix decays
    assert s.optimizer.settings()[3:] == (0.1, True)
    assert solver().build().optimizer.settings() == (0.9, 0.999, 1e-8, 0.0, False)     # optimizer="Adam" ignores cfg.weight_decay
