"""GPU: frozen parameters (requires_grad = False) -- the run-table optimizer launches against the dense ones, then the model: a frozen
tensor and its optimizer state keep their bits, every trainable tensor gets the bits of the same step with nothing frozen, ``.grad`` of a
frozen tensor is None, and under the encoder cut (all six recurrent layers, the three inter-layer LayerNorms and the table frozen) the
backward pass stops in front of the encoders while the forward pass, which then keeps no encoder stash, still gives the unfrozen step's
scores and losses bit for bit.  References: the dense launches for the ops, the unfrozen step of the same build for bits,
``oracle.misa_oracle`` (gradients None for frozen names) for the fp32 model."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import misa_oracle as orc

DEV = "cuda:0"
LR, CLIP = 1e-3, 1.0
RNN = ("trnn1", "trnn2", "vrnn1", "vrnn2", "arnn1", "arnn2")
LNS = ("tlayer_norm", "vlayer_norm", "alayer_norm")
SET_B = ("trnn1", "embed")                                   # some of the encoders: every gradient is still computed
SET_C = RNN + LNS + ("embed",)                               # the encoder cut


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


def _model(precision="fp32", vocab=120, **kw):
    from mmda_amd import make_config, MISA
    cfg = orc.default_config(vocab_size=vocab)
    m = MISA(make_config(precision=precision, device=DEV, **kw, **vars(cfg)))
    m.load_state_dict(orc.synth_params(cfg, 21))
    m.to(DEV)
    m._materialize(torch.device(DEV))                        # (the flat buckets are made lazily: the tests read them before the first step)
    return m, cfg


def _step(m, b, **kw):
    kw.setdefault("training", False)
    m.train_step(b["t"].to(DEV), b["v"].to(DEV), b["a"].to(DEV), b["l"], b["emo"].to(DEV), lr=LR, clip=CLIP, **kw)


def _state(m):
    P, _, M, V = m.flat_buckets()
    torch.cuda.synchronize()
    return [x.detach().cpu().clone() for x in (P, M, V)]


def _set_state(m, state, step):
    for x, y in zip((m.flat_buckets()[0], m.flat_buckets()[2], m.flat_buckets()[3]), state):
        x.copy_(y)
    m._step = step


def _ranges(m, frozen: bool):
    """[(name, begin, end)] of the frozen / the trainable tensors; a tensor's range runs up to the next tensor (alignment padding)"""
    names = m._native_names
    offs = [m._layout[n][0] for n in names] + [m._flat_floats]
    return [(n, offs[i], offs[i + 1]) for i, n in enumerate(names) if m._get(n).requires_grad != frozen]


def _assert_frozen_untouched(m, got, before, what=""):
    fr = _ranges(m, True)
    assert fr
    for name, b, e in fr:
        for tag, x, y in zip("PMV", got, before):
            assert torch.equal(x[b:e], y[b:e]), (what, name, tag)


def _assert_trainable_equal(m, got, want, what=""):
    tr = _ranges(m, False)
    assert tr
    for name, b, e in tr:
        for tag, x, y in zip("PMV", got, want):
            assert torch.equal(x[b:e], y[b:e]), (what, name, tag, float((x[b:e] - y[b:e]).abs().max()))


# ------------------------------------------------------------------------------------------------ 1: the run-table launches
def _op_ranges(n):
    """runs of length 1, 3, 4 and 5, begins at offsets = 1, 2, 3, 0 mod 4, a whole quad, long runs, a run that ends at n; the first
    element is frozen.  n = 5: a run of one float and a run of two that ends at n."""
    if n == 5:
        return [(1, 1), (3, 2)]
    r = [(1, 1), (6, 3), (11, 4), (16, 5), (24, 4), (33, 1000), (1037, 2), (1041, n - 1041 - 9), (n - 7, 7)]
    assert r[-2][1] > 0 and r[-1][0] + r[-1][1] == n
    return r


@pytest.mark.parametrize("n", [5, 4099, 2 ** 21 + 4003])
def test_run_table_ops_equal_the_dense_ops_inside_the_runs_and_touch_nothing_else(n):
    """2^21 + 4003: more items than the capped grid of 2048 x 256 lanes holds, so lanes take a second trip through the stride loop.  The
    gradient (and the accumulator) hold NaN wherever nothing trains: a frozen float that was read would show in a trainable result or,
    written back, in P, M or V."""
    from mmda_amd import ops
    gen = torch.Generator().manual_seed(n)
    ranges = _op_ranges(n)
    runs = ops.runs_table(ranges, n, DEV)
    assert runs[1] == len(ranges)
    assert runs[2] == sum((b + l - 1) // 4 - b // 4 + 1 for b, l in ranges)
    if n > 2 ** 21:
        assert runs[2] > 2048 * 256
    mask = torch.zeros(n, dtype=torch.bool)
    for b, l in ranges:
        mask[b:b + l] = True
    assert not mask[0] and mask[n - 1] and 0 < int(mask.sum()) < n
    mask = mask.to(DEV)
    nan = torch.full((n,), float("nan"), device=DEV)

    def rnd(scale=1.0, positive=False):
        x = torch.rand(n, generator=gen) if positive else torch.randn(n, generator=gen)
        return (x * scale).to(DEV)

    p0, g, a, m0, v0 = rnd(), rnd(2.5), rnd(2.5), rnd(0.1), rnd(0.01, positive=True)
    g_nan, a_nan = torch.where(mask, g, nan), torch.where(mask, a, nan)
    if n > 5:
        assert 0 < int(((g * 0.5).abs() > CLIP)[mask].sum()) < int(mask.sum())      # some trainable elements are clamped, not all

    def check(got, ref, start, what):
        for tag, x, y, x0 in zip("PMV", got, ref, start):
            assert torch.equal(x[mask], y[mask]), (what, tag)
            assert torch.equal(x[~mask], x0[~mask]), (what, tag, "frozen")
            assert not torch.equal(x[mask], x0[mask]), (what, tag, "nothing moved")

    ref = [p0.clone(), m0.clone(), v0.clone()]
    got = [p0.clone(), m0.clone(), v0.clone()]
    ops.clamp_adam(ref[0], g, ref[1], ref[2], LR, 3, clip=CLIP, grad_scale=0.5)
    ops.clamp_adam_runs(got[0], g_nan, got[1], got[2], runs, LR, 3, clip=CLIP, grad_scale=0.5)
    check(got, ref, (p0, m0, v0), "adam")

    ref = [p0.clone(), m0.clone(), v0.clone()]
    got = [p0.clone(), m0.clone(), v0.clone()]
    ops.clamp_adam_sum(ref[0], a, g, ref[1], ref[2], LR, 2, clip=CLIP, grad_scale=1.0 / 3.0)
    ops.clamp_adam_sum_runs(got[0], a_nan, g_nan, got[1], got[2], runs, LR, 2, clip=CLIP, grad_scale=1.0 / 3.0)
    check(got, ref, (p0, m0, v0), "adam over acc + g")
    assert torch.equal(a_nan[mask], a[mask]) and torch.equal(g_nan[mask], g[mask])      # neither operand is written

    ref = [p0.clone(), v0.clone()]
    got = [p0.clone(), v0.clone()]
    ops.clamp_rmsprop(ref[0], g, ref[1], 1e-2, clip=CLIP, grad_scale=0.5)
    ops.clamp_rmsprop_runs(got[0], g_nan, got[1], runs, 1e-2, clip=CLIP, grad_scale=0.5)
    for tag, x, y, x0 in zip(("P", "square_avg"), got, ref, (p0, v0)):
        assert torch.equal(x[mask], y[mask]), ("rmsprop", tag)
        assert torch.equal(x[~mask], x0[~mask]), ("rmsprop", tag, "frozen")
    assert not any(bool(torch.isnan(x).any()) for x in got)

    # a slice of the table that starts at a later run: its own item count, the runs in front are left alone
    if n > 5:
        table, k, items = runs
        first = [int(x) for x in table[:, 2].tolist()]
        got = [p0.clone(), m0.clone(), v0.clone()]
        ref = [p0.clone(), m0.clone(), v0.clone()]
        ops.clamp_adam(ref[0], g, ref[1], ref[2], LR, 1, clip=CLIP)
        ops.clamp_adam_runs(got[0], g_nan, got[1], got[2], (table[3:], k - 3, items - first[3]), LR, 1, clip=CLIP)
        tail = mask.clone(); tail[:ranges[3][0]] = False
        for tag, x, y, x0 in zip("PMV", got, ref, (p0, m0, v0)):
            assert torch.equal(x[tail], y[tail]) and torch.equal(x[~tail], x0[~tail]), ("slice", tag)


# ------------------------------------------------------------------------------------------------ 2: one step, bits
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_one_step_is_bit_identical_on_the_trainable_tensors_and_leaves_the_frozen_ones(precision):
    """Two unfrozen steps (M and V are non-zero), then one step with the same seed, dropout on, on (a) nothing frozen, (b) trnn1.* and
    the table, (c) the cut set -- at (B, T) = (8, 12) and again, from (a)'s state, at (6, 9), so that the shape changes between steps of
    a model that has frozen tensors.  (c)'s forward keeps no encoder stash: its scores and six losses are (a)'s."""
    models = {}
    for k in "abc":
        models[k], cfg = _model(precision)
    warm = [orc.synth_batch(cfg, 8, 12, 60 + i, ragged=True) for i in range(2)]
    for m in models.values():
        for i, b in enumerate(warm):
            _step(m, b, training=True, seed=900 + i)
    assert models["b"].freeze(*SET_B) and models["c"].freeze(*SET_C)
    assert not models["b"].trainable_info()[2]
    step = 2
    for B, T in ((8, 12), (6, 9)):
        snap = _state(models["a"])
        assert float(snap[1].abs().max()) > 0 and float(snap[2].abs().max()) > 0
        for k in "bc":
            _set_state(models[k], snap, step)
        batch = orc.synth_batch(cfg, B, T, 70 + B, ragged=True)
        out = {}
        for k, m in models.items():
            _step(m, batch, training=True, seed=1000 + B)
            out[k] = (_state(m), m._ws_view("scores", (B, cfg.num_classes)).cpu().clone(), m.read_losses())
        step += 1
        assert models["c"].trainable_info()[2] and models["c"]._trainable_sends == 1
        assert not torch.equal(out["a"][0][0], snap[0])
        for k in "bc":
            _assert_frozen_untouched(models[k], out[k][0], snap, (k, B, T))
            _assert_trainable_equal(models[k], out[k][0], out["a"][0], (k, B, T))
            assert torch.equal(out[k][1], out["a"][1]), (k, "scores")
            assert out[k][2] == out["a"][2], (k, out[k][2], out["a"][2])
        # (a)'s frozen-in-(c) tensors did move: the comparison above is not vacuous
        name, b0, e0 = _ranges(models["c"], True)[0]
        assert not torch.equal(out["a"][0][0][b0:e0], snap[0][b0:e0]), name
    for m in models.values():
        assert not m.cluster_aborted()


def test_cut_step_with_the_stashing_forward_gives_the_same_bits():
    """set_frozen_forward(True): the cut step stashes all the same (what tools/bench_frozen.py measures the no-stash forward against)"""
    a, cfg = _model("bf16")
    b, _ = _model("bf16")
    for m in (a, b):
        m.freeze(*SET_C)
    b.set_frozen_forward(True)
    for i in range(2):
        batch = orc.synth_batch(cfg, 8, 12, 80 + i, ragged=True)
        _step(a, batch, training=True, seed=50 + i); _step(b, batch, training=True, seed=50 + i)
        assert a.read_losses() == b.read_losses()
    for x, y in zip(_state(a), _state(b)):
        assert torch.equal(x, y)
    assert not a.cluster_aborted() and not b.cluster_aborted()


# ------------------------------------------------------------------------------------------------ 3: fp32 against the oracle
@pytest.mark.parametrize("which", ["b", "c"])
def test_model_fp32_three_steps_match_the_oracle_with_none_gradients(which):
    """The per-step criteria of tests/test_gpu_accum.py::test_model_fp32_two_micro_batches_match_oracle_mean_gradient; the oracle's
    AdamState skips a None gradient as torch does."""
    m, cfg = _model("fp32")
    frozen = set(m.freeze(*(SET_B if which == "b" else SET_C)))
    P = orc.synth_params(cfg, 21)
    P0 = {k: v.clone() for k, v in P.items()}
    opt = orc.AdamState(P, LR)
    for i in range(3):
        batch = orc.synth_batch(cfg, 6, 9, 30 + i, ragged=True)
        _step(m, batch)
        G = orc.loss_and_grads(P, cfg, batch)[2]
        opt.step(P, {k: (None if g is None or k in frozen else g.clamp(-CLIP, CLIP)) for k, g in G.items()})
        torch.cuda.synchronize()
        got_sd = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
        for k, p in P.items():
            ref, got = p.numpy(), got_sd[k]
            if k in frozen:
                assert np.array_equal(got, P0[k].numpy()), (i, k)
                continue
            if k.endswith("self_attn.in_proj_bias"):
                hs = cfg.hidden_size
                keep = np.ones(3 * hs, bool); keep[hs:2 * hs] = False
                ref, got = ref[keep], got[keep]
            d = np.abs(got - ref)
            assert d.max() <= 2 * LR + 1e-7, (i, k)             # one Adam step moves an element by at most lr
            assert (d <= 0.02 * LR).mean() >= 0.99, (i, k, float((d <= 0.02 * LR).mean()))
    assert m._step == 3 and not m.cluster_aborted()


# ------------------------------------------------------------------------------------------------ 4: the unfused path
def _solver(optimizer="Adam", precision="fp32", batches=1, n_epoch=1, dev=0):
    from mmda_amd import make_config, models
    from mmda_amd.solver import Solver
    cfg = orc.default_config(vocab_size=120, learning_rate=LR, clip=CLIP)
    c = make_config(precision=precision, device=DEV, n_epoch=n_epoch, optimizer=optimizer, name="frozen", **vars(cfg))
    train = [orc.synth_batch(cfg, B, T, 90 + i, ragged=True) for i, (B, T) in enumerate([(6, 9), (8, 12), (6, 5)][:batches])]
    devb = [orc.synth_batch(cfg, 6, 9, 190 + i, ragged=True) for i in range(dev)]
    m = models.MISA(c)
    m.load_state_dict(orc.synth_params(cfg, 21))
    s = Solver(c, c, c, ListLoader([_tuple_of(b) for b in train]), ListLoader([_tuple_of(b) for b in devb]), ListLoader([]),
               is_train=True, model=m)
    return s, train


@pytest.mark.parametrize("optimizer", ["Adam", "RMSprop"])
def test_unfused_step_leaves_frozen_tensors_and_equals_the_unfrozen_step_elsewhere(optimizer):
    """forward, the six getters, loss.backward(), clip_grad_value_, optimizer.step() (Solver.train_epoch_unfused, one batch, dropout on:
    both models draw the same seed) with set (b) against the same step with nothing frozen.  The optimizer state starts non-zero."""
    res = {}
    for frozen in (False, True):
        s, _ = _solver(optimizer)
        m = s.model
        if frozen:
            m.freeze(*SET_B)
        torch.manual_seed(7)
        s.build()
        m._materialize(torch.device(DEV))
        gen = torch.Generator().manual_seed(3)
        second = torch.rand(m._flat_floats, generator=gen).mul_(1e-3).to(DEV)
        if optimizer == "Adam":
            m.flat_buckets()[2].copy_(torch.randn(m._flat_floats, generator=gen).mul_(1e-2).to(DEV))
            m.flat_buckets()[3].copy_(second)
            m._step = 2
            state = lambda: _state(m)
        else:
            s.optimizer._square_avg(m.flat_buckets()[0]).copy_(second)
            state = lambda: [m.flat_buckets()[0].detach().cpu().clone(), s.optimizer._square_avg(m.flat_buckets()[0]).detach().cpu().clone()]
        before = state()
        s.train_epoch_unfused()
        torch.cuda.synchronize()
        res[frozen] = (m, before, state())
        for name, p in m.named_parameters():
            if name == "embed.weight" or name.startswith("trnn1."):
                assert (p.grad is None) == frozen, name
            else:
                assert p.grad is not None, name
        assert not m.cluster_aborted()
    m, before, after = res[True]
    assert len(s.optimizer.param_groups[0]["params"]) == len(list(m.parameters())) - 9      # the reference's filtered list
    _assert_frozen_untouched(m, after, before, optimizer)
    _assert_trainable_equal(m, after, res[False][2], optimizer)
    for x, y in zip(res[False][2], res[False][1]):
        name, b0, e0 = _ranges(m, True)[0]
        assert not torch.equal(x[b0:e0], y[b0:e0])              # ... which the unfrozen step did move


# ------------------------------------------------------------------------------------------------ 5: accumulation
def test_accumulated_step_under_the_cut_equals_the_manual_path_on_the_trainable_tensors():
    """accum_steps = 3 with the (8, 9), (8, 12), (6, 9) micro-batches of tests/test_gpu_accum.py and set (c), against that file's manual
    path on an unfrozen twin -- train_step(do_adam=False) per micro-batch, the sum written into the bucket, mmda_misa_adam_step --
    restricted to the trainable tensors."""
    from mmda_amd import _lib
    m, cfg = _model("bf16")
    twin, _ = _model("bf16")
    warm = orc.synth_batch(cfg, 8, 12, 41, ragged=True)
    for x in (m, twin):
        _step(x, warm, training=True, seed=5)
    m.freeze(*SET_C)
    before = _state(m)
    batches = [orc.synth_batch(cfg, B, T, 50 + i, ragged=True) for i, (B, T) in enumerate([(8, 9), (8, 12), (6, 9)])]
    G = []
    for k, b in enumerate(batches):
        _step(m, b, seed=100 + k, accum_index=k, accum_count=3)
        _step(twin, b, seed=100 + k, do_adam=False)
        G.append(twin.flat_buckets()[1].clone())
    twin.flat_buckets()[1].copy_((G[0] + G[1]) + G[2])
    _lib.check(twin._lib.mmda_misa_adam_step(twin._h, LR, CLIP, 1.0 / 3.0, 2, _lib.stream_ptr()), "adam_step")
    got = _state(m)
    assert m._step == 2
    _assert_frozen_untouched(m, got, before, "accum")
    _assert_trainable_equal(m, got, _state(twin), "accum")
    assert not torch.equal(got[0], before[0])
    assert not m.cluster_aborted() and not twin.cluster_aborted()


# ------------------------------------------------------------------------------------------------ 6: the flags change between steps
def test_freeze_step_unfreeze_step():
    m, cfg = _model("bf16")
    ref, _ = _model("bf16")
    b1, b2 = (orc.synth_batch(cfg, 8, 12, 20 + i, ragged=True) for i in range(2))
    assert m._trainable_sends == 0
    m.freeze(*SET_C)
    _step(m, b1, training=True, seed=1)
    _step(m, b1, training=True, seed=2)
    assert m._trainable_sends == 1                             # the same set twice: sent once
    mid = _state(m)
    m.unfreeze(*SET_C)
    _set_state(ref, mid, 2)
    _step(m, b2, training=True, seed=3)
    _step(ref, b2, training=True, seed=3)
    assert m._trainable_sends == 2 and ref._trainable_sends == 0
    for x, y, x0 in zip(_state(m), _state(ref), mid):
        assert torch.equal(x, y)
    off = m._layout["embed.weight"][0]
    assert m.frozen_names() == [] and not torch.equal(_state(m)[0][off:], mid[0][off:])        # the table trains again
    assert not m.cluster_aborted()


# ------------------------------------------------------------------------------------------------ 7: refusals
def _free_port():
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def test_refusals_leave_a_usable_model():
    from mmda_amd import _lib
    import torch.distributed as dist
    m, cfg = _model("fp32")
    fresh, _ = _model("fp32")
    b = orc.synth_batch(cfg, 6, 9, 30, ragged=True)
    for x in (m, fresh):
        x.freeze("trnn1")
    with pytest.raises(_lib.MMDAError, match="not built yet"):
        _step(m, b, grad_sync=lambda g, n: 1.0)
    assert m._step == 0
    _step(m, b); _step(fresh, b)
    for x, y in zip(_state(m), _state(fresh)):
        assert torch.equal(x, y)

    for mode in ("sparse", "deferred"):
        e, _ = _model("fp32", embed_update=mode)
        efresh, _ = _model("fp32", embed_update=mode)
        e.embed.weight.requires_grad_(False)
        with pytest.raises(_lib.MMDAError, match=r'set_embed_update\("frozen"\)'):
            _step(e, b)
        assert e._step == 0
        e.embed.weight.requires_grad_(True)
        _step(e, b); _step(efresh, b)
        e.flush_embedding(); efresh.flush_embedding()
        for x, y in zip(_state(e), _state(efresh)):
            assert torch.equal(x, y)

    # Solver.build() under an initialised process group (one rank, gloo)
    s, train = _solver()
    s.model.freeze("trnn1")
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1)
    try:
        with pytest.raises(_lib.MMDAError, match="not built yet"):
            s.build()
    finally:
        dist.destroy_process_group()
    s.build()                                                  # ... and without the group it builds and trains
    s.train_epoch()
    assert s.model._step == 1 and not s.model.cluster_aborted()


# ------------------------------------------------------------------------------------------------ 8: Solver
def test_solver_trains_the_heads_of_a_frozen_encoder():
    s, train = _solver(precision="bf16", batches=3, n_epoch=2, dev=2)
    m = s.model
    names = m.freeze("trnn", "vrnn", "arnn", "tlayer_norm", "vlayer_norm", "alayer_norm", "embed")
    assert len(names) == 48 + 6 + 1
    torch.manual_seed(11)
    s.build()
    assert len(s.optimizer.param_groups[0]["params"]) == len(list(m.parameters())) - len(names)
    m._materialize(torch.device(DEV))
    before = _state(m)
    for e in range(2):
        out = s.train_epoch()
        assert all(np.isfinite(v) for v in out.values())
        loss, acc, _, _ = s.eval("dev")
        assert np.isfinite(loss)
    assert m._step == 6 and m.trainable_info()[2] and m._trainable_sends == 1
    after = _state(m)
    _assert_frozen_untouched(m, after, before, "solver")
    moved = {n: (b0, e0) for n, b0, e0 in _ranges(m, False)}
    for name in ("classifier.classifier_layer.weight", "project_t.project_t.weight", "shared.shared_1.weight",
                 "transformer_encoder.layers.0.linear1.weight", "recon_a.recon_a_1.bias"):
        b0, e0 = moved[name]
        assert not torch.equal(after[0][b0:e0], before[0][b0:e0]), name
    # the optimizer state round-trips
    sd = s.optimizer.state_dict()
    assert sd["step"] == 6
    keep = {k: sd[k].clone() for k in ("exp_avg", "exp_avg_sq")}
    m.flat_buckets()[2].zero_(); m.flat_buckets()[3].zero_(); m._step = 0
    s.optimizer.load_state_dict(sd)
    assert m._step == 6
    for k, x in zip(("exp_avg", "exp_avg_sq"), m.flat_buckets()[2:]):
        assert torch.equal(x.cpu(), keep[k])
    s.train_epoch()                                            # ... and training goes on
    _assert_frozen_untouched(m, _state(m), before, "solver, resumed")
    assert not m.cluster_aborted()
