"""MI355X: the sentiment task -- the one-launch collector against the reference's fixture, the head / criterion entry
points against float64 torch, and the step under the task against an oracle composed from oracle/misa_oracle.py (its forward up to
`o.h`, the classifier's parameters and the `cls` mask, its own diff / sim / recon terms; torch autograd gives the gradients).

Bounds (none is made from what the kernels give):
  collector   counts equal; the float64 sums equal tests/senti_cases.py's restatement of the kernel's summation order bit for bit; figures
              as senti_cases.check_figures holds them (ratios of counts: 1 ulp; mae, mae_intensity, corr: 8 x float64 numpy's own distance
              from the longdouble definition, floored at 4 ulp -- the rule of tests/test_gpu_losses.py)
  ops         scores and the score column's d_logits are products by 0, 1 or 2: bit for bit; tcp 1e-5 / its d_logits 1e-4 of the tensor's
              max (tests/test_gpu_dropout_parity.py's head test); the l1 seed bit for bit; values and the mse seed 8 x max(e32, 2^-24),
              e32 the float32 torch restatement's error against float64 on the same inputs (tests/cls_loss_cases.py's rule)
  fp32 step   outputs and losses 1e-4, gradients 2e-4 of the tensor's max, three clip+Adam steps by the three criteria of
              tests/test_gpu_model.py::test_fp32_fused_step_matches_golden
  bf16 step   scores 1e-2 x max(1, max |score|) against the float oracle (test_bf16_path_within_1e2, part 2); the criterion
              differentially from the step's own stored scores
  paths       fused step, unfused epoch and autograd: every gradient 2e-4 of the tensor's max, the bound each path is held to
With MMDA_SENTI_RATIOS_OUT set to a path the measured error / e32 of the op tests is written there (tests/golden/senti_error_ratios.json
is such a run)."""
import contextlib
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import senti_cases as sc
from model_compare import rel
from oracle import dropout_rng as drng
from oracle import misa_oracle as orc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EINVAL = -1
THR = 0.35
LR, CLIP = 1e-3, 1.0
FIX = sc.load_fixture()
RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _ratios_file():
    yield
    path = os.environ.get("MMDA_SENTI_RATIOS_OUT")
    if path:
        with open(path, "w") as f:
            json.dump(RATIOS, f, indent=0, sort_keys=True)


@pytest.fixture(scope="module", autouse=True)
def _global_generators_as_found():
    """Solver.build() draws weight_hh* from torch's global generator (orthogonal_), and so do tests of other files: this module hands
    the global generators back as it found them, so what runs behind it sees the state it saw before this file existed."""
    cpu = torch.get_rng_state()
    cuda = torch.cuda.get_rng_state_all() if torch.cuda.is_available() else None
    yield
    torch.set_rng_state(cpu)
    if cuda is not None:
        torch.cuda.set_rng_state_all(cuda)


def _lib():
    from mmda_amd import _lib as L
    return L, L.load()


# ================================================================================================ collector
def _collect(pred, truth, split):
    """(counts, sums, figures dict, raw state) of the device collector over the batches of `split` rows"""
    from mmda_amd import SentimentEval
    ev = SentimentEval(DEV)
    p, t = torch.from_numpy(np.asarray(pred)).to(DEV), torch.from_numpy(np.asarray(truth)).to(DEV)
    for lo, hi in sc.batches(p.numel(), split):
        ev.update(p[lo:hi], t[lo:hi])
    fig = dict(zip(sc.FIGURES, ev.figures().cpu().tolist()))
    st = ev.state.cpu()
    return st[:sc.NI].numpy().copy(), st[sc.F0:sc.F0 + sc.NF].view(torch.float64).numpy().copy(), fig, st


@pytest.mark.parametrize("split", sc.SPLITS, ids=lambda s: f"batch{s}")
@pytest.mark.parametrize("name", list(FIX))
def test_collector_against_the_fixture(name, split):
    pred, truth, want = FIX[name]
    counts, sums, fig, st = _collect(pred, truth, split)
    want_counts, want_sums = sc.state_numpy(pred, truth, split)
    assert (counts == want_counts).all(), (counts, want_counts)
    assert (counts == sc.state_numpy(pred, truth, None)[0]).all()                 # ... whatever the split
    assert int(st[13]) == 0 and not st[14:16].any() and int(st[23]) == 0          # the ticket is back at 0, the spare words untouched
    assert sums.tobytes() == want_sums.tobytes(), (sums, want_sums)               # the kernel's summation order, bit for bit
    lines = []
    bad = sc.check_figures(f"{name}/{split}", fig, pred, truth, want, lines)
    print("\n".join(lines))
    assert not bad, "\n".join(bad)
    for k in sc.FIGURES:                                                           # NaN where the fixture has NaN, and nowhere else
        assert np.isnan(fig[k]) == np.isnan(want[k]), k
    # a second run over the same batches: the same bits
    _, _, fig2, st2 = _collect(pred, truth, split)
    assert torch.equal(st, st2)
    assert np.array([fig[k] for k in sc.FIGURES]).tobytes() == np.array([fig2[k] for k in sc.FIGURES]).tobytes()


@pytest.mark.parametrize("n", [1, 257, 8192 + 300])
def test_collector_sizes_around_the_launch_forms(n):
    """one row; one row past a workgroup; past GRID_CAP workgroups, where a workgroup strides (the restatement is held to the fixture by
    tests/test_senti_cpu.py; here the device is held to the restatement and to the definition)"""
    rng = np.random.default_rng(n)
    grid = (np.arange(-9, 10) / 3.0).astype(np.float32)
    truth = rng.choice(grid, size=n)
    pred = (truth + rng.normal(0, 1.0, n)).astype(np.float32)
    counts, sums, fig, _ = _collect(pred, truth, None)
    want_counts, want_sums = sc.state_numpy(pred, truth, None)
    assert (counts == want_counts).all() and sums.tobytes() == want_sums.tobytes()
    want = sc.finish_numpy(want_counts, want_sums)
    for k in sc.FIGURES:
        if np.isnan(want[k]):
            assert np.isnan(fig[k]), k
        elif k in sc.SUMMED:
            d = sc.definition(pred, truth, np.longdouble)[k]
            d64 = sc.definition(pred, truth, np.float64)[k]
            bound = sc.FACTOR * max(abs(float(np.longdouble(d64) - d)), sc.FLOOR_ULP * sc.ulp(float(d)))
            err = abs(float(np.longdouble(fig[k]) - d))
            print(f"n={n} {k}: err {err:.3e} bound {bound:.3e}")
            assert err <= bound, (k, err, bound)
        else:
            assert abs(fig[k] - want[k]) <= sc.RATIO_ULP * sc.ulp(want[k]), k


def test_sentiment_metrics_surface():
    from mmda_amd import SentimentEval, sentiment_metrics
    from mmda_amd import sentiment as S
    L, lib = _lib()
    pred, truth, want = FIX["random_300"]
    p, t = torch.from_numpy(pred).to(DEV), torch.from_numpy(truth).to(DEV)
    ev = sentiment_metrics(p.view(-1, 1), t)                                       # (N, 1) against (N,)
    d = ev.as_dict()
    assert set(S.REFERENCE_KEYS) <= set(d) and "f1_non0" in d and d["mult"] == d["acc7"]
    assert not sc.check_figures("surface", d, pred, truth, want)
    c = ev.counts()
    assert c["n"] == 300 and c["n_nonzero"] == int((truth != 0).sum()) and c["n_extreme"] == int((np.abs(truth) > 2).sum())
    assert "MAE:" in S.format_table(d, c["n"], c["n_nonzero"])
    with pytest.raises(L.MMDAError):
        SentimentEval("cpu")
    with pytest.raises(L.MMDAError):
        SentimentEval(DEV).update(p.cpu(), t.cpu())
    with pytest.raises(ValueError):
        SentimentEval(DEV).update(p[:5], t[:4])
    # the entry points refuse what they cannot run, before any launch
    st = torch.zeros(sc.WORDS + 1, dtype=torch.int64, device=DEV)
    out = torch.zeros(9, dtype=torch.float64, device=DEV)
    s = L.stream_ptr()
    assert lib.mmda_senti_accumulate(None, t.data_ptr(), 4, st.data_ptr(), s) == EINVAL
    assert lib.mmda_senti_accumulate(p.data_ptr(), t.data_ptr(), -1, st.data_ptr(), s) == EINVAL
    assert lib.mmda_senti_accumulate(p.data_ptr(), t.data_ptr(), 4, st.data_ptr() + 4, s) == EINVAL
    assert lib.mmda_senti_accumulate(p.data_ptr(), t.data_ptr(), 0, st.data_ptr(), s) == 0
    assert lib.mmda_senti_finish(None, out.data_ptr(), s) == EINVAL and lib.mmda_senti_finish(st.data_ptr(), None, s) == EINVAL
    assert not st.cpu().any()


# ================================================================================================ ops
def _op_case(B, p):
    z, y = sc.op_inputs(B, int(p * 10))
    seed = 0x9E3779B97F4A7C15 + (2 if B == 1 else 0)
    mask = torch.from_numpy(drng.mask(p, seed, drng.SITE_CLS, (B, 1)))
    if p > 0 and B > 1:
        assert bool((mask == 0).any()) and bool((mask != 0).any()), "choose another seed"
    return z, y, seed, mask


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("B", sc.OP_BATCHES)
def test_heads_task_against_float64(B, p):
    L, lib = _lib()
    z, y, seed, mask = _op_case(B, p)
    g = torch.Generator().manual_seed(B)
    dtcp, dsc = torch.randn(B, 6, generator=g), torch.randn(B, 1, generator=g)
    tcp64, s64, lab64 = sc.head_fwd(z.double(), mask, THR)
    zd = z.to(DEV)
    tcp, s, lab = (torch.empty(B, n, device=DEV) for n in (6, 1, 1))
    st = L.stream_ptr()
    fwd = lambda task, a, b, c: lib.mmda_heads_fwd_task(zd.data_ptr(), B, 1, THR, a.data_ptr(), b.data_ptr(), c.data_ptr(), p, seed,
                                                        drng.SITE_CLS, task, st)
    assert fwd(1, tcp, s, lab) == 0
    assert torch.equal(s.cpu().double(), s64)                                       # z * {0, 1, 2}: exact in float32
    assert torch.equal(lab.cpu().double(), lab64) and rel(tcp, tcp64) < 1e-5
    dz = torch.empty(B, 7, device=DEV)
    bwd = lambda task, dt, ds, out: lib.mmda_heads_bwd_task(tcp.data_ptr(), s.data_ptr(), None if dt is None else dt.data_ptr(),
                                                            None if ds is None else ds.data_ptr(), B, 1, out.data_ptr(), p, seed,
                                                            drng.SITE_CLS, task, st)
    dtd, dsd = dtcp.to(DEV), dsc.to(DEV)
    assert bwd(1, dtd, dsd, dz) == 0
    ref = sc.head_bwd(tcp64, mask, dtcp.double(), dsc.double())
    assert torch.equal(dz[:, 6:].cpu().double(), ref[:, 6:])                        # no s (1 - s): the seed times the mask
    assert rel(dz[:, :6], ref[:, :6]) < 1e-4
    assert bwd(1, None, dsd, dz) == 0 and float(dz[:, :6].abs().max()) == 0.0 and torch.equal(dz[:, 6:].cpu().double(), ref[:, 6:])
    assert bwd(1, dtd, None, dz) == 0 and float(dz[:, 6:].abs().max()) == 0.0
    # task 0 through the same entry is the classifier's call, bit for bit
    a0, b0, c0 = (torch.empty(B, n, device=DEV) for n in (6, 1, 1))
    a1, b1, c1 = (torch.empty(B, n, device=DEV) for n in (6, 1, 1))
    assert fwd(0, a0, b0, c0) == 0
    assert lib.mmda_heads_fwd(zd.data_ptr(), B, 1, THR, a1.data_ptr(), b1.data_ptr(), c1.data_ptr(), p, seed, drng.SITE_CLS, st) == 0
    assert torch.equal(a0, a1) and torch.equal(b0, b1) and torch.equal(c0, c1) and torch.equal(a0, tcp)
    assert float(b0.max()) <= 1.0 and float(b0.min()) >= 0.0
    keep = b0.clone()
    assert fwd(2, a0, b0, c0) == EINVAL and fwd(-1, a0, b0, c0) == EINVAL and bwd(2, dtd, dsd, dz) == EINVAL
    assert torch.equal(b0, keep)


def _metric(got, ref):
    ref = ref.double().reshape(-1); got = got.double().reshape(-1)
    return float((got - ref).norm() / ref.norm().clamp_min(1e-300))


@pytest.mark.parametrize("kind", sc.KINDS)
@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("B", sc.OP_BATCHES)
def test_loss_reg_against_float64(B, p, kind):
    L, lib = _lib()
    z, y, seed, mask = _op_case(B, p)
    s = (z[:, 6:] * mask.float()).contiguous()
    s[::3, 0] = y[::3]                                                              # rows with s == y: the seed is exactly 0 there
    k = L.SENTI_LOSS[kind]
    name = f"reg-B{B}-p{p}-{kind}"
    sd, yd = s.to(DEV), y.to(DEV)
    loss, ds = torch.zeros((), device=DEV), torch.zeros(B, 1, device=DEV)
    st = L.stream_ptr()
    assert lib.mmda_loss_reg(sd.data_ptr(), yd.data_ptr(), B, 1, k, 1.0, loss.data_ptr(), ds.data_ptr(), st) == 0
    v64, g64 = sc.reg_value(s.double(), y, kind), sc.reg_grad(s.double(), y, kind)
    v32, g32 = sc.reg_value(s, y, kind), sc.reg_grad(s, y, kind)
    den = abs(float(v64)) or 1.0                                                     # (B = 1: the one row is planted, the value exactly 0)
    e_v = max(abs(float(v32) - float(v64)) / den, sc.E32_FLOOR)
    err_v = abs(float(loss) - float(v64)) / den
    assert float(v64) != 0.0 or float(loss) == 0.0
    RATIOS[name] = {"value": round(err_v / e_v, 3)}
    print(f"{name}: value err {err_v:.3e} e32 {e_v:.3e}")
    assert err_v <= sc.FACTOR * e_v
    assert bool((ds[::3] == 0).all())
    if kind == "l1":
        assert torch.equal(ds.cpu(), g32)                                           # +-1/B or 0, bit for bit
        one = float(torch.tensor(1.0) / B)
        assert set(ds.cpu().unique().tolist()) <= {-one, 0.0, one}
    else:
        e_g = max(_metric(g32, g64), sc.E32_FLOOR)
        err_g = _metric(ds.cpu(), g64)
        RATIOS[name]["grad.whole"] = round(err_g / e_g, 3)
        print(f"{name}: seed err {err_g:.3e} e32 {e_g:.3e}")
        assert err_g <= sc.FACTOR * e_g
    # gradients accumulate, scaled; the value is added, unscaled; either output may be absent
    pre = torch.randn(B, 1, generator=torch.Generator().manual_seed(B + 1))
    ds2 = pre.to(DEV)
    assert lib.mmda_loss_reg(sd.data_ptr(), yd.data_ptr(), B, 1, k, 0.5, loss.data_ptr(), ds2.data_ptr(), st) == 0
    want = pre.double() + sc.reg_grad(s.double(), y, kind, 0.5)
    e_a = max(_metric(pre + sc.reg_grad(s, y, kind, 0.5), want), sc.E32_FLOOR)
    assert _metric(ds2.cpu(), want) <= sc.FACTOR * e_a
    assert abs(float(loss) - 2 * float(v64)) <= 2 * sc.FACTOR * e_v * abs(float(v64))
    assert lib.mmda_loss_reg(sd.data_ptr(), yd.data_ptr(), B, 1, k, 1.0, None, None, st) == 0
    keep = ds2.clone()
    for bad in ((2, B), (-1, B), (k, 0)):
        assert lib.mmda_loss_reg(sd.data_ptr(), yd.data_ptr(), bad[1], 1, bad[0], 1.0, loss.data_ptr(), ds2.data_ptr(), st) == EINVAL
    assert lib.mmda_loss_reg(None, yd.data_ptr(), B, 1, k, 1.0, loss.data_ptr(), ds2.data_ptr(), st) == EINVAL
    assert torch.equal(ds2, keep)


def test_senti_loss_function_is_the_op_with_autograd():
    from mmda_amd.utils import functions as F
    z, y = sc.op_inputs(33, 3)
    for kind in sc.KINDS:
        s = z[:, 6:].clone().to(DEV).requires_grad_(True)
        loss = F.senti_loss(s, y.to(DEV), kind)
        (3.0 * loss).backward()
        assert abs(float(loss.detach()) - float(sc.reg_value(z[:, 6:].double(), y, kind))) <= 1e-5 * float(loss.detach())
        assert rel(s.grad, 3.0 * sc.reg_grad(z[:, 6:].double(), y, kind)) < 1e-5


# ================================================================================================ the step
TINY = dict(embedding_size=12, visual_size=5, acoustic_size=7, hidden_size=16, vocab_size=30)       # the tiny fixtures' widths
CONFIGS = {
    "tiny": dict(TINY),                                                  # hidden 16: the stand-alone head and loss launches
    "mosei": dict(vocab_size=80),                                        # MOSEI widths: the fused row-local stretches
    "mosei_adv": dict(vocab_size=80, use_cmd_sim=False),                 # the adversarial branch: stand-alone launches at hidden 128
    "mosei_gru": dict(vocab_size=80, rnncell="gru"),
}
T = 6


def _cfg(name, **kw):
    return orc.default_config(num_classes=1, **dict(CONFIGS[name], **kw))


def _targets(B, seed):
    g = torch.Generator().manual_seed(900 + 13 * B + seed)
    y = torch.randint(-9, 10, (B,), generator=g).float() / 3.0
    y[torch.rand(B, generator=g) < 0.15] = 0.0
    return y


def _batch(cfg, B, seed):
    b = orc.synth_batch(cfg, B, T, seed, ragged=True)
    b["y"] = _targets(B, seed)
    return b


@contextlib.contextmanager
def _fusion_dropout(p):
    import mmda_amd.models as mm
    old = mm.FUSION_DROPOUT
    try:
        mm.FUSION_DROPOUT = p
        yield
    finally:
        mm.FUSION_DROPOUT = old


def _model(cfg, precision="fp32", wseed=31, p_tf=0.0, task="sentiment", senti_loss="l1", **kw):
    from mmda_amd import MISA, make_config
    with _fusion_dropout(p_tf):
        m = MISA(make_config(precision=precision, device=DEV, task=task, senti_loss=senti_loss, **kw, **vars(cfg)))
    missing = m.load_state_dict(orc.synth_params(cfg, wseed), strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    m.to(DEV)
    m._materialize(torch.device(DEV))
    return m


def _step(m, b, target="y", **kw):
    kw.setdefault("training", False)
    kw.setdefault("lr", LR)
    kw.setdefault("clip", CLIP)
    m.train_step(b["t"].to(DEV), b["v"].to(DEV), b["a"].to(DEV), b["l"], b[target].to(DEV), **kw)


def _state(m):
    P, _, M, V = m.flat_buckets()
    torch.cuda.synchronize()
    return [x.detach().cpu().clone() for x in (P, M, V)]


def _assert_state_equal(a, b, what="", model=None):
    for name, x, y in zip("PMV", a, b):
        bad = int((x != y).sum())
        where = []
        if bad and model is not None:                             # which tensors: the failure names them
            offs = [model._layout[n][0] for n in model._native_names] + [model._flat_floats]
            where = [(n, int((x[offs[i]:offs[i + 1]] != y[offs[i]:offs[i + 1]]).sum())) for i, n in enumerate(model._native_names)]
            where = [w for w in where if w[1]]
        assert bad == 0, (what, name, bad, float((x - y).abs().max()), where)


def senti_oracle(P, cfg, b, kind, masks=None, dtype=torch.float32):
    """(o with .scores, L, G) of one step under the task: oracle.misa_oracle.forward up to o.h, the regression output from the
    classifier's parameters and the `cls` mask, the criterion's restatement, the oracle's own diff / sim / recon terms; autograd."""
    old = torch.get_default_dtype()
    try:
        torch.set_default_dtype(dtype)                            # (the encoders' nn.LSTM modules are made inside the oracle)
        leaves = {k: p.detach().clone().to(dtype).requires_grad_(True) for k, p in P.items()}
        o = orc.forward(leaves, cfg, b["t"], b["v"].to(dtype), b["a"].to(dtype), b["l"], None, masks)
        s = o.h @ leaves["classifier.classifier_layer.weight"].t() + leaves["classifier.classifier_layer.bias"]
        if masks is not None:
            s = s * masks["cls"].to(dtype)
        o.scores = s
        L = SimpleNamespace(cls=sc.reg_value(s, b["y"], kind), diff=orc.diff_loss(o), recon=orc.recon_loss(o),
                            sim=orc.cmd_loss(o) if cfg.use_cmd_sim else orc.domain_loss(o))
        L.total = L.cls + cfg.diff_weight * L.diff + cfg.sim_weight * L.sim + cfg.recon_weight * L.recon
        L.total.backward()
        G = {k: (None if p.grad is None else p.grad.detach()) for k, p in leaves.items()}
        return o, L, G
    finally:
        torch.set_default_dtype(old)


def _assert_outputs_losses(m, B, o, L, tol):
    pub = m._public()
    assert rel(pub["scores"], o.scores.detach()) < tol and rel(pub["tcp"], o.tcp.detach()) < tol
    got = m.read_losses()
    for k in ("cls", "diff", "sim", "recon", "total"):
        ref = float(getattr(L, k).detach())
        print(f"loss {k}: {got[k]!r} oracle {ref!r}")
        assert abs(got[k] - ref) <= tol * abs(ref) + 1e-7, (k, got[k], ref)
    assert got["conf"] == 0.0                                     # no confidence loss under the task (one column)
    labels = pub["labels"].cpu()
    near = (o.scores.detach() - cfg_threshold(m)).abs() < 1e-4
    assert bool(((labels.double() == (o.scores.detach() > cfg_threshold(m)).double()) | near).all())


def cfg_threshold(m):
    return float(m.config.threshold)


def _assert_grads(grads, G, cfg, tol, what):
    n = 0
    for k, g in grads.items():
        g = torch.as_tensor(g).detach().cpu().double()
        assert bool(torch.isfinite(g).all()), k
        if G[k] is None:
            assert float(g.abs().max()) == 0.0, f"{k}: the oracle leaves this gradient None; ours must be exactly zero"
            continue
        ref = G[k].double()
        if k.endswith("self_attn.in_proj_bias"):
            hs = cfg.hidden_size
            keep = torch.ones(3 * hs, dtype=torch.bool); keep[hs:2 * hs] = False
            assert float(g[~keep].abs().max()) < 1e-5
            g, ref = g[keep], ref[keep]
        e = float((g - ref).abs().max() / ref.abs().max().clamp_min(1e-6))
        if e > 0.25 * tol:
            print(f"{what} {k}: gradient error {e:.3e} (bound {tol:.1e})")
        assert e < tol, f"{what} {k}: gradient error {e:.3e} (bound {tol:.1e})"
        n += 1
    assert n > 20
    return n


def _grads_of(m):
    m._assign_grad_views()
    return {k: p.grad for k, p in m.named_parameters()}


FP32_CASES = [("tiny", 5), ("tiny", 33), ("mosei", 5), ("mosei", 33), ("mosei_adv", 5), ("mosei_gru", 5)]


@pytest.mark.parametrize("kind", sc.KINDS)
@pytest.mark.parametrize("name,B", FP32_CASES, ids=[f"{n}-B{b}" for n, b in FP32_CASES])
def test_fp32_step_matches_the_composed_oracle(name, B, kind):
    cfg = _cfg(name)
    b = _batch(cfg, B, 17)
    P = orc.synth_params(cfg, 31)
    m = _model(cfg, senti_loss=kind)
    assert m.task == "sentiment" and m.senti_loss == kind
    _step(m, b, do_adam=False)
    assert not m.cluster_aborted()
    o, L, G = senti_oracle(P, cfg, b, kind, dtype=torch.float64)
    _assert_outputs_losses(m, B, o, L, 1e-4)
    _assert_grads(_grads_of(m), G, cfg, 2e-4, f"{name}-B{B}-{kind}")
    if kind == "mse" and B == 33:
        return                                                    # (the optimizer part does not depend on the criterion: l1 and one mse case)
    # three clip + Adam steps from the same start against the oracle's loop
    m = _model(cfg, senti_loss=kind)
    Pr = {k: v.clone() for k, v in P.items()}
    opt = orc.AdamState(Pr, LR)
    n = 3
    for s in range(n):
        bs = _batch(cfg, B, 40 + s)
        _step(m, bs)
        _, Ls, Gs = senti_oracle(Pr, cfg, bs, kind)
        opt.step(Pr, {k: (None if g is None else g.clamp(-CLIP, CLIP)) for k, g in Gs.items()})
        tot = m.read_losses()["total"]
        assert abs(tot - float(Ls.total)) < 2e-4 * abs(float(Ls.total)), s
    for k, p in m.state_dict().items():
        got, ref, base = p.detach().cpu().numpy(), Pr[k].numpy(), P[k].numpy()
        if k.endswith("self_attn.in_proj_bias"):
            hs = cfg.hidden_size
            keep = np.ones(3 * hs, bool); keep[hs:2 * hs] = False
            got, ref, base = got[keep], ref[keep], base[keep]
        d = np.abs(got - ref)
        assert d.max() <= 2 * n * LR + 1e-7, k
        assert (d <= 0.01 * n * LR).mean() >= 0.99, (k, float((d <= 0.01 * n * LR).mean()))
        upd_ref = (ref - base).astype(np.float64); upd = (got - base).astype(np.float64)
        if np.linalg.norm(upd_ref) > 0:
            assert np.linalg.norm(upd - upd_ref) <= 2e-2 * np.linalg.norm(upd_ref), (k, np.linalg.norm(upd - upd_ref) / np.linalg.norm(upd_ref))
        else:
            assert np.abs(upd).max() == 0.0, k


TRAIN_CASES = [("tiny", 5, 0x1D0A5EF0), ("mosei", 5, 0x1D0A5EF0), ("mosei", 33, 0x2B0B0001), ("mosei_adv", 5, 0x3C0C0002)]


@pytest.mark.parametrize("kind", sc.KINDS)
@pytest.mark.parametrize("name,B,seed", TRAIN_CASES, ids=[f"{n}-B{b}" for n, b, _ in TRAIN_CASES])
def test_training_mode_step_matches_the_masked_oracle(name, B, seed, kind):
    """dropout on: p = 0.25 at the fusion layer's four sites, 0.5 at the output column (and in the discriminator), the masks of
    oracle/dropout_rng.py; the bounds of the dropout-off step (a mask multiplies by 0 or by a constant: no new rounding)"""
    p_tf, p_cls = 0.25, 0.5
    cfg = _cfg(name, dropout=p_cls)
    b = _batch(cfg, B, 17)
    P = orc.synth_params(cfg, 31)
    masks = drng.site_masks(cfg, B, seed, p_tf, p_cls)
    assert masks["cls"].shape == (B, 1) and bool((masks["cls"] == 0).any()) and bool((masks["cls"] != 0).any())
    m = _model(cfg, p_tf=p_tf, senti_loss=kind)
    _step(m, b, do_adam=False, training=True, seed=seed)
    assert not m.cluster_aborted()
    o, L, G = senti_oracle(P, cfg, b, kind, masks=masks, dtype=torch.float64)
    _assert_outputs_losses(m, B, o, L, 1e-4)
    dropped = masks["cls"][:, 0] == 0
    assert bool((m._public()["scores"].cpu()[dropped] == 0).all())                  # a dropped output is exactly 0
    _assert_grads(_grads_of(m), G, cfg, 2e-4, f"train-{name}-B{B}-{kind}")


@pytest.mark.parametrize("kind", sc.KINDS)
@pytest.mark.parametrize("B", [5, 33])
def test_bf16_step_criterion_is_fp32_behind_the_scores(B, kind):
    """bf16 encoders in front of the same block: the criterion is fp32 arithmetic behind the logits, so it is checked from the step's own
    stored scores -- the l1 seed in the workspace bit for bit, the loss at the op test's bound; the scores themselves against the float
    oracle at the bf16 output bound"""
    p_tf, p_cls, seed = 0.25, 0.5, 0x5E0E04F5
    cfg = _cfg("mosei", dropout=p_cls)
    b = _batch(cfg, B, 17)
    m = _model(cfg, precision="bf16", p_tf=p_tf, senti_loss=kind)
    _step(m, b, do_adam=False, training=True, seed=seed)
    assert not m.cluster_aborted()
    s = m._public()["scores"].cpu().clone()
    ds = m._ws_view("d_scores", (B, 1)).cpu().clone()
    y = b["y"]
    g32, g64 = sc.reg_grad(s, y, kind), sc.reg_grad(s.double(), y, kind)
    if kind == "l1":
        assert torch.equal(ds, g32)
    else:
        assert _metric(ds, g64) <= sc.FACTOR * max(_metric(g32, g64), sc.E32_FLOOR)
    v64 = float(sc.reg_value(s.double(), y, kind))
    e_v = max(abs(float(sc.reg_value(s, y, kind)) - v64) / abs(v64), sc.E32_FLOOR)
    got = m.read_losses()["cls"]
    print(f"bf16 B={B} {kind}: cls {got!r} float64 of the stored scores {v64!r} e32 {e_v:.2e}")
    assert abs(got - v64) <= sc.FACTOR * e_v * abs(v64)
    masks = drng.site_masks(cfg, B, seed, p_tf, p_cls)
    o, _, _ = senti_oracle(orc.synth_params(cfg, 31), cfg, b, kind, masks=masks)
    ref = o.scores.detach()
    err = float((s - ref).abs().max())
    print(f"bf16 B={B}: scores err {err:.3e} max |score| {float(ref.abs().max()):.3f}")
    assert err <= 1e-2 * max(1.0, float(ref.abs().max()))
    # the backward pass behind the seed: the classifier's gradient from the step's own stored tensors (d_logits = d_scores * mask)
    gw = _grads_of(m)["classifier.classifier_layer.bias"].cpu()
    want = (ds.double() * masks["cls"]).sum(0)
    assert abs(float(gw) - float(want)) <= 1e-5 * max(1.0, abs(float(want)))


# ------------------------------------------------------------------------------------------------ the three paths
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
    return (b["t"], b["v"], b["a"], b["y"], b["emo"], b["l"], z, z, z, [f"s{i}" for i in range(B)])


@pytest.mark.parametrize("kind", sc.KINDS)
@pytest.mark.parametrize("name", ["tiny", "mosei"])
def test_fused_unfused_and_autograd_gradients_agree(name, kind):
    """one batch, dropout off (config.dropout = 0, the fusion layer's 0.1 patched to 0): the fused step, Solver.train_epoch_unfused and
    model(...) + the getters + backward()"""
    from mmda_amd.solver import Solver
    cfg = _cfg(name, dropout=0.0, clip=100.0, learning_rate=LR)
    b = _batch(cfg, 5, 17)
    fused = _model(cfg, senti_loss=kind)
    _step(fused, b, do_adam=False, training=True, clip=100.0)
    G = {"fused": {k: g.detach().cpu().clone() for k, g in _grads_of(fused).items()}}
    auto = _model(cfg, senti_loss=kind)
    auto.train()
    solver = Solver(auto.config, auto.config, auto.config, None, None, None, is_train=True, model=auto)
    auto.zero_grad()
    scores, _ = auto(b["t"].to(DEV), b["v"].to(DEV), b["a"].to(DEV), b["l"], None, None, None)
    assert scores.shape == (5, 1)
    total = (solver.get_cls_loss(scores, b["y"].to(DEV)) + cfg.diff_weight * solver.get_diff_loss()
             + cfg.sim_weight * solver.get_cmd_loss() + cfg.recon_weight * solver.get_recon_loss())
    total.backward()
    G["autograd"] = {k: p.grad.detach().cpu().clone() for k, p in auto.named_parameters()}
    assert abs(float(total) - fused.read_losses()["total"]) <= 1e-4 * abs(float(total))
    unf = _model(cfg, senti_loss=kind)
    s = Solver(unf.config, unf.config, unf.config, ListLoader([_tuple_of(b)]), None, None, is_train=True, model=unf)
    s.optimizer = unf.config.optimizer([p for p in unf.parameters() if p.requires_grad], lr=LR).attach(unf)
    out = s.train_epoch_unfused()
    assert abs(out["total"] - float(total)) <= 1e-4 * abs(float(total))
    G["unfused"] = {k: p.grad.detach().cpu().clone() for k, p in unf.named_parameters()}
    for a_, b_ in (("fused", "autograd"), ("fused", "unfused"), ("autograd", "unfused")):
        worst = 0.0
        for k in G[a_]:
            x, y = G[a_][k].double(), G[b_][k].double()
            if k.endswith("self_attn.in_proj_bias"):
                continue
            e = float((x - y).abs().max() / y.abs().max().clamp_min(1e-6))
            worst = max(worst, e)
            assert e < 2e-4, (a_, b_, k, e)
        print(f"{name}-{kind}: {a_} vs {b_}: worst gradient difference {worst:.3e} of the tensor's max")


# ------------------------------------------------------------------------------------------------ switching, default bits
def test_set_task_switches_between_steps_on_one_handle():
    """a one-column model: the emotion classifier and the regression on the same handle, each step equal bit for bit to a model that was
    built for it"""
    cfg = _cfg("mosei")
    b = _batch(cfg, 5, 17)
    b["emo1"] = (b["y"] > 0).float().view(-1, 1)
    m = _model(cfg, task="emotion")
    senti, emo = _model(cfg, task="sentiment", senti_loss="mse"), _model(cfg, task="emotion")
    for task, twin, target in (("sentiment", senti, "y"), ("emotion", emo, "emo1"), ("sentiment", senti, "y")):
        assert m.set_task(task, "mse") == task
        for x in (m, twin):
            _step(x, b, target=target, do_adam=False, training=True, seed=77)
        assert torch.equal(m.flat_buckets()[1], twin.flat_buckets()[1]), task
        assert torch.equal(m._ws_view("losses", (8,)), twin._ws_view("losses", (8,))), task
        assert torch.equal(m._public()["scores"], twin._public()["scores"]), task
    assert not torch.equal(senti.flat_buckets()[1], emo.flat_buckets()[1])
    s = emo._public()["scores"]
    assert float(s.min()) >= 0.0 and float(s.max()) <= 1.0


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_default_task_step_is_bit_identical_to_a_model_that_never_heard_of_it(precision):
    """two optimizer steps, dropout on, of a model whose configuration has no `task` at all and of one that was told "emotion": the
    same parameters, moments, losses and scores.  (bf16: a resident recurrence that gave up on its cluster -- DESIGN.md section 5's
    open item -- invalidates a step whatever the task, so the abort flag is looked at before the bits.)"""
    from mmda_amd import MISA, make_config
    cfg = orc.default_config(vocab_size=80)                                          # six classes: the default model
    b = orc.synth_batch(cfg, 8, T, 17, ragged=True)

    def build(strip):
        c = make_config(precision=precision, device=DEV, **vars(cfg))
        if strip:
            del c.task, c.senti_loss
        m = MISA(c)
        m.load_state_dict(orc.synth_params(cfg, 31))
        m.to(DEV)
        m._materialize(torch.device(DEV))
        return m

    plain, told = build(True), build(False)
    told.set_task("emotion")
    for k in range(2):
        for m in (plain, told):
            _step(m, b, target="emo", training=True, seed=500 + k)
        sp, st = _state(plain), _state(told)
        assert not plain.cluster_aborted() and not told.cluster_aborted()            # (a recurrence that gave up is no statement about the task)
        _assert_state_equal(sp, st, k, plain)
        assert torch.equal(plain._ws_view("losses", (8,)), told._ws_view("losses", (8,)))
        assert torch.equal(plain._public()["scores"], told._public()["scores"])


# ------------------------------------------------------------------------------------------------ accumulation, encoded step
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_two_micro_batches_are_the_manual_mean(precision):
    """accum_steps = 2 under the task: bit-identical to two steps without their optimizer, the gradient buckets added in order, and the
    native Adam step at scale 1/2 (the property tests/test_gpu_accum.py asserts for emotion, asserted the same way)"""
    from mmda_amd import _lib as L
    cfg = _cfg("mosei")
    m, twin = _model(cfg, precision), _model(cfg, precision)
    start = _state(m)
    batches = [_batch(cfg, 8, 60), _batch(cfg, 5, 61)]
    for k, b in enumerate(batches):
        _step(m, b, training=True, seed=300 + k, accum_index=k, accum_count=2)
    G = []
    for k, b in enumerate(batches):
        _step(twin, b, training=True, seed=300 + k, do_adam=False)
        G.append(twin.flat_buckets()[1].clone())
    twin.flat_buckets()[1].copy_(G[0] + G[1])
    L.check(twin._lib.mmda_misa_adam_step(twin._h, LR, CLIP, 0.5, 1, L.stream_ptr()), "adam_step")
    _assert_state_equal(_state(m), _state(twin))
    assert m._step == 1 and not torch.equal(_state(m)[0], start[0]) and not m.cluster_aborted()


CUT = ("trnn1", "trnn2", "vrnn1", "vrnn2", "arnn1", "arnn2", "tlayer_norm", "vlayer_norm", "alayer_norm", "embed")


def _samples_of(b):
    out = []
    for i, n in enumerate(b["l"].tolist()):
        lab = np.concatenate([[float(b["y"][i])], b["emo"][i].numpy()]).astype(np.float32)[None]
        out.append(((b["t"][:n, i].numpy(), b["v"][:n, i].numpy(), b["a"][:n, i].numpy(), ["w"] * n), lab, f"seg{i}"))
    return out


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_encoded_step_gives_the_bits_of_the_cut_step(precision):
    from mmda_amd import DeviceDataset, EncodedLoader, EncoderCache, _lib as L
    cfg = _cfg("mosei")
    a, e = _model(cfg, precision), _model(cfg, precision)
    for m in (a, e):
        m.freeze(*CUT)
    for i, B in enumerate((8, 5)):
        b = _batch(cfg, B, 70 + i)
        ds = DeviceDataset.from_samples(_samples_of(b), DEV)
        cache = EncoderCache.build(e, ds, B, order="dataset")
        assert cache.task == "sentiment" and cache.emo.shape == (B, 1) and torch.equal(cache.emo[:, 0], ds.sentiment)
        assert torch.equal(cache.emo[:, 0].cpu(), b["y"])
        (eb,) = list(EncodedLoader(cache, B))
        before = _state(e)
        _step(a, b, training=True, seed=1000 + i)
        e.train_step_encoded(eb, lr=LR, clip=CLIP, seed=1000 + i)
        sa, se = _state(a), _state(e)
        _assert_state_equal(se, sa, (precision, i))
        assert not torch.equal(se[0], before[0])
        assert torch.equal(e._ws_view("losses", (8,)).cpu(), a._ws_view("losses", (8,)).cpu())
        assert torch.equal(e._ws_view("scores", (B, 1)).cpu(), a._ws_view("scores", (B, 1)).cpu())
    # a cache stored under the other task is refused by name, nothing launched
    other = _model(cfg, precision, task="emotion")
    other.freeze(*CUT)
    stale = EncoderCache.build(other, ds, B, order="dataset")
    assert stale.task == "emotion" and stale.emo.shape == (B, 6)
    (sb,) = list(EncodedLoader(stale, B))
    keep = _state(e)
    with pytest.raises(L.MMDAError, match="task"):
        e.train_step_encoded(sb, lr=LR, clip=CLIP)
    _assert_state_equal(_state(e), keep)


# ------------------------------------------------------------------------------------------------ Solver
def _corpus(cfg, n=40):
    rng = np.random.default_rng(5)
    grid = (np.arange(-9, 10) / 3.0).astype(np.float32)
    out = []
    for i in range(n):
        ln = int(rng.integers(1, T + 1))
        lab = np.zeros((1, 7), np.float32)
        lab[0, 0] = 0.0 if i % 7 == 0 else rng.choice(grid)
        lab[0, 1:] = rng.random(6) > 0.6
        out.append(((rng.integers(2, cfg.vocab_size, ln), rng.standard_normal((ln, cfg.visual_size)).astype(np.float32),
                     rng.standard_normal((ln, cfg.acoustic_size)).astype(np.float32), ["w"] * ln), lab, f"seg{i}"))
    return out


def _solver(cfg, ds, name, **kw):
    from mmda_amd import DeviceLoader, MISA, make_config
    from mmda_amd.solver import Solver
    c = make_config(precision="fp32", device=DEV, task="sentiment", n_epoch=2, optimizer="Adam", name=name, batch_size=16,
                    **dict(vars(cfg), **kw))
    m = MISA(c)
    m.load_state_dict(orc.synth_params(cfg, 9))
    gen = torch.Generator().manual_seed(3)
    s = Solver(c, c, c, DeviceLoader(ds, 16, shuffle=True, generator=gen), DeviceLoader(ds, 16), DeviceLoader(ds, 16), is_train=True,
               model=m).build()
    m._materialize(torch.device(DEV))                        # (the flat buckets are made lazily: the test reads them before the first step)
    return s


def test_solver_trains_evaluates_prints_and_checkpoints(tmp_path, monkeypatch, capsys):
    from mmda_amd import DeviceDataset, sentiment_metrics
    from mmda_amd import sentiment as S
    monkeypatch.chdir(tmp_path)
    cfg = _cfg("mosei", learning_rate=LR)
    ds = DeviceDataset.from_samples(_corpus(cfg), DEV)
    s = _solver(cfg, ds, "senti")
    before = _state(s.model)
    hist = s.train()
    assert len(hist) == 2 and s.model._step == 6 and not torch.equal(_state(s.model)[0], before[0])
    out = capsys.readouterr().out
    for line in ("MAE:", "Correlation Coefficient:", "mult_acc_7:", "mult_acc_5:", "F1 score all/non0:", "Accuracy all/non0:",
                 "Extreme Intensity MAE:"):
        assert sum(x.startswith(line) for x in out.splitlines()) == 3, line        # two dev passes and the test pass
    assert os.path.exists("checkpoints/model_senti.std") and os.path.exists("checkpoints/optim_senti.std")
    loss, acc, preds, truths = s.eval("dev")
    assert preds.shape == (40,) and truths.shape == (40,) and preds.dtype == np.float32
    assert sorted(truths.tolist()) == sorted(ds.sentiment.cpu().tolist())
    last = s.last_sentiment
    assert set(S.REFERENCE_KEYS) <= set(last) and acc == last["acc2_non0"]
    one = sentiment_metrics(torch.from_numpy(preds).to(DEV), torch.from_numpy(truths).to(DEV))
    whole = one.as_dict()
    c1, c2 = one.counts(), s.last_sentiment_counts
    assert all(c1[k] == c2[k] for k in S.COUNTS)
    for k in S.FIGURES:
        if k in sc.SUMMED:
            assert abs(last[k] - whole[k]) <= 1e-12 * max(1.0, abs(whole[k])), k   # the same rows in three batches: another order of the sums
        else:
            assert last[k] == whole[k] or (np.isnan(last[k]) and np.isnan(whole[k])), k
    # the dev loss is the mean of the batches' MAE under l1, and what the best checkpoint was chosen by
    bounds = [(0, 16), (16, 32), (32, 40)]
    assert abs(loss - np.mean([np.abs(preds[a:b] - truths[a:b]).mean() for a, b in bounds])) <= 1e-5 * loss
    assert all(h["valid_acc"] == h["valid_acc"] and h["valid_loss"] > 0 for h in hist)
    # the checkpoint round-trips: a fresh model that loads it evaluates to the same predictions, bit for bit
    s2 = _solver(cfg, ds, "senti")
    s2.model.load_state_dict(torch.load("checkpoints/model_senti.std", weights_only=True))
    s2.model.to(DEV)
    s.model.load_state_dict(torch.load("checkpoints/model_senti.std", weights_only=True))
    p1, p2 = s.eval("dev")[2], s2.eval("dev")[2]
    assert np.array_equal(p1, p2)
    assert not s.model.cluster_aborted()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_raise_by_name_and_leave_the_handle_unchanged(monkeypatch):
    from mmda_amd import MISA, make_config, step_rules
    from mmda_amd import _lib as L
    from mmda_amd.solver import Solver
    rules = dict(step_rules.SENTI_RULES)
    text = lambda r, **kw: rules[r].format(**kw)

    def raises(fn, want):
        with pytest.raises(L.MMDAError) as e:
            fn()
        assert str(e.value) == want, (str(e.value), want)

    # --- a sentiment model: every refused setting, then a step equal to an untouched twin's
    cfg = _cfg("mosei")
    m, twin = _model(cfg), _model(cfg)
    raises(lambda: m.set_cls_loss([2.0], 0.0), text("senti_pos_weight"))
    raises(lambda: m.set_cls_loss(None, 2.0), text("senti_focal", gamma=2.0))
    raises(lambda: m.set_task("sentiment", "huber"), text("senti_loss", loss="huber"))
    raises(lambda: m.set_task("regression"), text("task_name", task="regression"))
    s = Solver(m.config, m.config, m.config, ListLoader([]), ListLoader([]), ListLoader([]), is_train=False, model=m)
    raises(lambda: s.calibrate("dev"), text("senti_calibrate", how="Solver.calibrate"))
    raises(lambda: s.rank("dev"), text("senti_rank"))
    for kw, want in ((dict(calibrate="global"), text("senti_calibrate", how="global")),
                     (dict(select_by="map"), text("senti_select_by", select_by="map")),
                     (dict(select_by="auroc"), text("senti_select_by", select_by="auroc"))):
        c = make_config(precision="fp32", device=DEV, task="sentiment", **dict(vars(cfg), **kw))
        raises(lambda: Solver(c, c, c, None, None, None, is_train=True, model=m).build(), want)
    h = m._h
    st = L.stream_ptr()
    assert m._lib.mmda_misa_set_task(h, 1, 2) == EINVAL and m._lib.mmda_misa_set_task(h, 2, 0) == EINVAL
    assert m._lib.mmda_misa_set_task(None, 1, 0) == EINVAL
    opts = L.ClsOpts(focal_gamma=2.0, n_weights=0)
    import ctypes as C
    assert m._lib.mmda_misa_set_cls_loss(h, C.byref(opts)) == EINVAL
    assert m.task == "sentiment" and m.senti_loss == "l1" and m.cls_loss == dict(pos_weight=None, focal_gamma=0.0)
    b = _batch(cfg, 5, 17)
    for x in (m, twin):
        _step(x, b, training=True, seed=9)
    _assert_state_equal(_state(m), _state(twin), "sentiment handle")
    assert torch.equal(m._ws_view("losses", (8,)), twin._ws_view("losses", (8,)))
    with pytest.raises(ValueError, match="sentiment column"):
        _step(m, b, target="emo")
    # --- construction: num_classes, use_confidNet, pos_weight, focal_gamma under the task
    mk = lambda **kw: MISA(make_config(precision="fp32", device=DEV, task="sentiment", **dict(vars(cfg), **kw)))
    raises(lambda: mk(num_classes=6), text("senti_classes", ncls=6))
    raises(lambda: mk(use_confidNet=True), text("senti_confid"))
    raises(lambda: mk(pos_weight=[3.0]), text("senti_pos_weight"))
    raises(lambda: mk(focal_gamma=2.0), text("senti_focal", gamma=2.0))
    raises(lambda: mk(senti_loss="huber"), text("senti_loss", loss="huber"))
    c6 = make_config(precision="fp32", device=DEV, task="sentiment", **dict(vars(cfg), num_classes=6))
    raises(lambda: Solver(c6, c6, c6, None, None, None, is_train=True, model=twin).build(), text("senti_classes", ncls=6))
    # --- a default six-class model: the task is refused, the next default step's bits are what they were
    cfg6 = orc.default_config(vocab_size=80)
    d, dtwin = _model(cfg6, task="emotion"), _model(cfg6, task="emotion")
    raises(lambda: d.set_task("sentiment"), text("senti_classes", ncls=6))
    assert d._lib.mmda_misa_set_task(d._h, 1, 0) == EINVAL
    d.set_cls_loss([1.0, 2.0, 1.0, 1.0, 3.0, 1.0], 2.0)
    d.set_cls_loss(None, 0.0)
    assert d.task == "emotion"
    b6 = orc.synth_batch(cfg6, 5, T, 17, ragged=True)
    for x in (d, dtwin):
        _step(x, b6, target="emo", training=True, seed=9)
    _assert_state_equal(_state(d), _state(dtwin), "default handle")
    assert torch.equal(d._ws_view("losses", (8,)), dtwin._ws_view("losses", (8,)))


def test_inference_pass_returns_the_raw_outputs():
    from mmda_amd import DeviceDataset, InferencePass, sentiment_metrics
    cfg = _cfg("mosei")
    m = _model(cfg)
    ds = DeviceDataset.from_samples(_corpus(cfg, 20), DEV)
    res = InferencePass(m, ("scores",)).run(ds, 8, "dataset")
    s = res.scores
    assert s.shape == (20, 1) and (float(s.max()) > 1.0 or float(s.min()) < 0.0)
    d = sentiment_metrics(s, ds.sentiment).as_dict()
    want = float((s[:, 0].double() - ds.sentiment.double()).abs().mean())
    assert abs(d["mae"] - want) <= 1e-12 * want
