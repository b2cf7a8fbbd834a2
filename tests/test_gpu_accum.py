"""GPU: config.accum_steps -- one optimizer step from N micro-batches with data-parallel semantics (A = ((G_0 + G_1) + G_2) + ...,
one fp32 add per element, then clip + Adam on A / N), from the three op-level launches up to ``Solver.train_epoch``.  References: torch's
own fp32 adds for the ops; ``oracle.misa_oracle`` (AdamState on the clamped mean gradient) for the fp32 model; and, for bit identity, the
path that existed before -- ``train_step(do_adam=False)`` per micro-batch, the sum written into the bucket by torch, then
``mmda_misa_adam_step``.  Dropout is off (training=False) unless a test says otherwise."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import misa_oracle as orc

DEV = "cuda:0"
LR, CLIP = 1e-3, 1.0


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


def _accum_step(m, batches, **kw):
    for k, b in enumerate(batches):
        _step(m, b, accum_index=k, accum_count=len(batches), **kw)


def _state(m):
    """(P, M, V) of the whole flat buckets, on the CPU"""
    P, _, M, V = m.flat_buckets()
    torch.cuda.synchronize()
    return [x.detach().cpu().clone() for x in (P, M, V)]


def _assert_state_equal(a, b, upto=None):
    for name, x, y in zip("PMV", a, b):
        x, y = (x, y) if upto is None else (x[:upto], y[:upto])
        bad = int((x != y).sum())
        assert bad == 0, (name, bad, float((x - y).abs().max()))


def _adam_step(m, scale, step):
    from mmda_amd import _lib
    _lib.check(m._lib.mmda_misa_adam_step(m._h, LR, CLIP, scale, step, _lib.stream_ptr()), "adam_step")


def _valid(b):
    T, B = b["t"].shape
    return torch.arange(T).unsqueeze(1) < b["l"].unsqueeze(0)


# ------------------------------------------------------------------------------------------------ 1: the accumulate op
@pytest.mark.parametrize("n", [1, 3, 4, 5, 4099, 2 ** 20 + 5, 2 ** 21 + 4 * 1000 + 3])
def test_accumulate_op_is_exact(n):
    """tail only (1, 3), float4 body only (4), both (5, 4099), over a thousand blocks (2^20 + 5), and more float4 than the capped grid of
    2048 x 256 lanes holds, so that lanes take a second trip through the stride loop (2^21 + 4003)."""
    from mmda_amd import ops
    gen = torch.Generator().manual_seed(n)
    g0, g1, g2 = (torch.randn(n, generator=gen).to(DEV) for _ in range(3))
    acc = torch.full((n,), float("nan"), device=DEV)
    ops.grad_accumulate(acc, g0, first=True)
    assert torch.equal(acc, g0)                              # a copy, whatever was there
    ops.grad_accumulate(acc, g1)
    ops.grad_accumulate(acc, g2)
    assert torch.equal(acc, (g0 + g1) + g2)
    assert not torch.isnan(acc).any()


# ------------------------------------------------------------------------------------------------ 2: the closing-step op
def test_closing_step_op_equals_accumulate_then_clamp_adam():
    from mmda_amd import ops
    n, scale = 4099, 1.0 / 3.0
    gen = torch.Generator().manual_seed(5)
    p0 = torch.randn(n, generator=gen)
    a = [p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)]           # accumulate, then mmda_clamp_adam
    b = [p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)]           # mmda_clamp_adam_sum
    c = [p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)]           # acc = None against mmda_clamp_adam
    d = [p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)]
    acc_a = torch.empty(n, device=DEV)
    acc_b = torch.empty(n, device=DEV)
    for step in (1, 2, 3):
        g = [(torch.randn(n, generator=gen) * 2.5).to(DEV) for _ in range(3)]
        total = (g[0] + g[1]) + g[2]
        clipped = int(((total * scale).abs() > CLIP).sum())
        assert 0 < clipped < n                               # some elements are clamped, not all
        ops.grad_accumulate(acc_a, g[0], first=True); ops.grad_accumulate(acc_a, g[1]); ops.grad_accumulate(acc_a, g[2])
        ops.clamp_adam(a[0], acc_a, a[1], a[2], LR, step, clip=CLIP, grad_scale=scale)
        ops.grad_accumulate(acc_b, g[0], first=True); ops.grad_accumulate(acc_b, g[1])
        keep, last = acc_b.clone(), g[2].clone()
        ops.clamp_adam_sum(b[0], acc_b, g[2], b[1], b[2], LR, step, clip=CLIP, grad_scale=scale)
        assert torch.equal(acc_b, keep) and torch.equal(g[2], last)                    # neither operand is written
        for x, y in zip(a, b):
            assert torch.equal(x, y), step
        ops.clamp_adam_sum(c[0], None, g[0], c[1], c[2], LR, step, clip=CLIP, grad_scale=scale)
        ops.clamp_adam(d[0], g[0], d[1], d[2], LR, step, clip=CLIP, grad_scale=scale)
        for x, y in zip(c, d):
            assert torch.equal(x, y), step
    assert not torch.equal(a[0].cpu(), p0) and not torch.equal(a[0], c[0])


@pytest.mark.parametrize("D", [300, 7])
def test_rows_append_op(D):
    """16-byte form (D % 4 == 0) and scalar form; padding positions become id -1; what lies outside the appended range is untouched"""
    from mmda_amd import ops
    gen = torch.Generator().manual_seed(D)
    cap = 200
    ids_out = torch.full((cap,), -7, dtype=torch.int64, device=DEV)
    rows_out = torch.full((cap, D), 9.0, device=DEV)
    used, want_ids, want_rows = 3, [], []
    for T, B in ((9, 8), (12, 6)):
        ids = torch.randint(0, 50, (T, B), generator=gen)
        rows = torch.randn(T * B, D, generator=gen)
        lengths = torch.randint(1, T + 1, (B,), generator=gen).to(torch.int32)
        new = ops.embed_rows_append(ids_out, rows_out, used, ids.to(DEV), rows.to(DEV), lengths.to(DEV))
        assert new == used + T * B
        used = new
        pad = torch.arange(T).unsqueeze(1) >= lengths.unsqueeze(0)
        want_ids.append(torch.where(pad, torch.full_like(ids, -1), ids).reshape(-1)); want_rows.append(rows)
    assert torch.equal(ids_out[3:used].cpu(), torch.cat(want_ids)) and torch.equal(rows_out[3:used].cpu(), torch.cat(want_rows))
    assert bool((ids_out[:3] == -7).all()) and bool((ids_out[used:] == -7).all())
    assert bool((rows_out[:3] == 9.0).all()) and bool((rows_out[used:] == 9.0).all())
    from mmda_amd import _lib
    with pytest.raises(_lib.MMDAError):                      # does not fit: refused, nothing launched
        ops.embed_rows_append(ids_out, rows_out, used, ids.to(DEV), rows.to(DEV), lengths.to(DEV))


# ------------------------------------------------------------------------------------------------ 3: fp32 model against the oracle
def test_model_fp32_two_micro_batches_match_oracle_mean_gradient():
    """The criteria of tests/test_gpu_dp.py::test_two_rank_dp_step_matches_oracle_mean_gradient, on the same quantity: the parameters
    after one step from the clamped mean of the two micro-batch gradients."""
    m, cfg = _model("fp32")
    batches = [orc.synth_batch(cfg, 6, 9, 30 + r, ragged=True) for r in range(2)]
    _accum_step(m, batches)
    torch.cuda.synchronize()
    assert m._step == 1 and not m.cluster_aborted()
    got_sd = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    P = orc.synth_params(cfg, 21)
    grads = [orc.loss_and_grads(P, cfg, b)[2] for b in batches]
    mean = {k: (None if grads[0][k] is None else sum(g[k] for g in grads) / 2) for k in grads[0]}
    mean = {k: (None if g is None else g.clamp(-CLIP, CLIP)) for k, g in mean.items()}
    opt = orc.AdamState(P, LR)
    opt.step(P, mean)
    for k, p in P.items():
        ref = p.numpy(); got = got_sd[k]
        if k.endswith("self_attn.in_proj_bias"):
            hs = cfg.hidden_size
            keep = np.ones(3 * hs, bool); keep[hs:2 * hs] = False
            ref, got = ref[keep], got[keep]
        d = np.abs(got - ref)
        assert d.max() <= 2 * LR + 1e-7, k                     # one Adam step moves an element by at most lr
        assert (d <= 0.02 * LR).mean() >= 0.99, (k, float((d <= 0.02 * LR).mean()))


# ------------------------------------------------------------------------------------------------ 4: bit identity with the manual path
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_model_is_bit_identical_to_the_manual_path(precision):
    """N = 3 with (B, T) = (8, 9), (8, 12), (6, 9): T changes, then B, so the workspace is re-carved between micro-batches (B = 8: the
    bf16 production kernel forms).  Two accumulated steps; the second reuses the accumulator."""
    m, cfg = _model(precision)
    twin, _ = _model(precision)
    n = m.grad_floats
    start = _state(m)
    assert n == m.flat_buckets()[0].numel()
    for step in (1, 2):
        batches = [orc.synth_batch(cfg, B, T, 40 + 10 * step + i, ragged=True) for i, (B, T) in enumerate([(8, 9), (8, 12), (6, 9)])]
        seeds = [100 * step + i for i in range(3)]
        for k, b in enumerate(batches):
            _step(m, b, seed=seeds[k], accum_index=k, accum_count=3)
            assert m._step == (step if k == 2 else step - 1)
        G = []
        for k, b in enumerate(batches):
            _step(twin, b, seed=seeds[k], do_adam=False)
            G.append(twin.flat_buckets()[1].clone())
        assert not torch.equal(G[0], G[1])
        twin.flat_buckets()[1].copy_((G[0] + G[1]) + G[2])
        _adam_step(twin, 1.0 / 3.0, step)
        _assert_state_equal(_state(m), _state(twin))
        assert m._step == step and m._acc is not None and m._acc.numel() == n
        if step == 1:
            acc_ptr = m._acc.data_ptr()
            assert not torch.equal(_state(m)[0], start[0])
        else:
            assert m._acc.data_ptr() == acc_ptr
    assert not m.cluster_aborted() and not twin.cluster_aborted()


# ------------------------------------------------------------------------------------------------ 5: accum_count = 1
def test_count_one_is_todays_step():
    """dropout on: both models draw the same seeds from the same start"""
    a, cfg = _model("fp32")
    b, _ = _model("fp32")
    start = _state(a)
    for i in range(2):
        batch = orc.synth_batch(cfg, 6, 9, 70 + i, ragged=True)
        _step(a, batch, training=True, accum_index=0, accum_count=1)
        _step(b, batch, training=True)
    _assert_state_equal(_state(a), _state(b))
    assert a._acc is None and a._acc_list is None and a._step == 2 and b._step == 2
    assert not torch.equal(_state(a)[0], start[0])


# ------------------------------------------------------------------------------------------------ 6: sparse
def _table(m):
    off, (V, D) = m._layout["embed.weight"]
    return off, V, D


def test_sparse_rows_update_runs_once_on_the_concatenated_list():
    from mmda_amd import ops
    m, cfg = _model("fp32", vocab=80, embed_update="sparse")
    twin, _ = _model("fp32", vocab=80, embed_update="sparse")
    batches = [orc.synth_batch(cfg, 8, 12, 81, ragged=True), orc.synth_batch(cfg, 8, 9, 82, ragged=True)]
    touched = [set(b["t"][_valid(b)].tolist()) for b in batches]
    seen = [set(b["t"].reshape(-1).tolist()) for b in batches]
    both = touched[0] & touched[1]
    pad_only = (seen[0] | seen[1]) - (touched[0] | touched[1])
    neither = sorted(set(range(80)) - (touched[0] | touched[1]))
    assert both and pad_only and (touched[0] - touched[1]) and (touched[1] - touched[0]) and set(pad_only) <= set(neither)
    start = _state(m)
    off, V, D = _table(m)
    n = m.grad_floats
    assert n == m.dense_floats == off

    _accum_step(m, batches)
    assert m._step == 1 and not m._rows_pending

    ids, rows, G = [], [], []
    for b in batches:
        _step(twin, b, do_adam=False)
        i, r = twin.embedding_grad_rows()
        ids.append(i.clone()); rows.append(r.clone()); G.append(twin.flat_buckets()[1][:n].clone())
    P, _, M, Vv = twin.flat_buckets()
    ops.embed_rows_sparse_adam(P[off:off + V * D].view(V, D), M[off:off + V * D].view(V, D), Vv[off:off + V * D].view(V, D),
                               torch.cat(ids), torch.cat(rows), LR, 1, lengths=None, clip=CLIP, grad_scale=0.5)
    ops.clamp_adam(P[:n], G[0] + G[1], M[:n], Vv[:n], LR, 1, clip=CLIP, grad_scale=0.5)
    got, want = _state(m), _state(twin)
    _assert_state_equal(got, want)
    rest = torch.tensor(neither)
    hit = torch.tensor(sorted(touched[0] | touched[1]))
    for x, x0 in zip(got, start):
        t, t0 = x[off:].view(V, D), x0[off:].view(V, D)
        assert torch.equal(t[rest], t0[rest])                # rows no micro-batch touched (padding included): bit for bit
        assert not torch.equal(t[hit], t0[hit])
    # a plain optimizer step behind it applies no stale rows: the table and its moments stay
    _adam_step(m, 1.0, 2)
    after = _state(m)
    for x, y in zip(got, after):
        assert torch.equal(x[off:], y[off:])
    assert not torch.equal(got[0][:off], after[0][:off])
    assert not m.cluster_aborted()


# ------------------------------------------------------------------------------------------------ 7: frozen
def test_frozen_table_stays_and_the_rest_equals_dense():
    batches = None
    out = {}
    for mode in ("dense", "frozen"):
        m, cfg = _model("fp32", vocab=80, embed_update=mode)
        if batches is None:
            batches = [orc.synth_batch(cfg, 8, 12, 81, ragged=True), orc.synth_batch(cfg, 8, 9, 82, ragged=True)]
        start = _state(m)
        _accum_step(m, batches)
        out[mode] = _state(m)
        off = m.dense_floats
        if mode == "frozen":
            assert m._acc.numel() == off
            for x, x0 in zip(out[mode], start):
                assert torch.equal(x[off:], x0[off:])        # the table and its (zero) moments
        else:
            assert m._acc.numel() == m.flat_buckets()[0].numel() and not torch.equal(out[mode][0][off:], start[0][off:])
    _assert_state_equal(out["dense"], out["frozen"], upto=off)
    assert not torch.equal(out["frozen"][0][:off], start[0][:off])


# ------------------------------------------------------------------------------------------------ 8: Solver
def test_solver_groups_the_loader_into_steps():
    """Five batches, accum_steps = 2: steps of 2, 2 and 1 micro-batches.  Dropout is on (train_epoch trains): the hand-issued sequence
    draws the same per-micro-batch seeds from the same start."""
    from mmda_amd import make_config, models
    from mmda_amd.solver import Solver
    cfg = orc.default_config(vocab_size=120, learning_rate=LR, clip=CLIP)
    c = make_config(precision="fp32", device=DEV, n_epoch=1, name="accum", accum_steps=2, **vars(cfg))
    shapes = [(6, 9), (4, 12), (6, 5), (6, 9), (4, 7)]
    train = [orc.synth_batch(cfg, B, T, 90 + i, ragged=True) for i, (B, T) in enumerate(shapes)]
    m = models.MISA(c)
    m.load_state_dict(orc.synth_params(cfg, 21))
    s = Solver(c, c, c, ListLoader([_tuple_of(b) for b in train]), ListLoader([]), ListLoader([]), is_train=True, model=m)
    s.build()
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}          # (build() re-initialised weight_hh*)
    out = s.train_epoch()
    assert m._step == 3

    hand = models.MISA(c)
    hand.load_state_dict(sd)
    hand.to(DEV)
    losses = []
    for (k, cnt), b in zip([(0, 2), (1, 2), (0, 2), (1, 2), (0, 1)], train):
        _step(hand, b, training=True, accum_index=k, accum_count=cnt)
        losses.append(hand.read_losses())
    assert hand._step == 3
    _assert_state_equal(_state(m), _state(hand))
    for k in out:
        ref = float(np.mean([l[k] for l in losses]))
        # fp32 sum of five terms on the device against a float64 mean: a few roundings of 2^-24 each
        assert abs(out[k] - ref) <= 1e-5 * abs(ref) + 1e-7, (k, out[k], ref)
    assert not m.cluster_aborted()


# ------------------------------------------------------------------------------------------------ 9: refusals
def test_refusals_leave_a_usable_model():
    from mmda_amd import _lib, make_config, MISA
    m, cfg = _model("fp32")
    fresh, _ = _model("fp32")
    b = orc.synth_batch(cfg, 6, 9, 30, ragged=True)
    with pytest.raises(_lib.MMDAError):
        _step(m, b, accum_index=1, accum_count=2)            # out of order
    _step(m, b, accum_index=0, accum_count=3)
    with pytest.raises(_lib.MMDAError):
        _step(m, b, accum_index=1, accum_count=2)            # the count changes mid-step
    _step(m, b, accum_index=0, accum_count=2)                # (the sequence was reset: a new one starts)
    with pytest.raises(_lib.MMDAError):
        _step(m, b, accum_index=0, accum_count=2)            # index 1 was due
    _step(m, b, accum_index=0, accum_count=2)
    with pytest.raises(_lib.MMDAError):
        _step(m, b)                                          # a plain step in the middle of an accumulated one
    with pytest.raises(_lib.MMDAError, match="grad_sync"):
        _step(m, b, accum_index=0, accum_count=2, grad_sync=lambda g, n: 1.0)
    with pytest.raises(_lib.MMDAError):
        _step(m, b, accum_index=2, accum_count=2)
    assert m._step == 0
    _step(m, b)
    _step(fresh, b)
    _assert_state_equal(_state(m), _state(fresh))
    assert m._step == 1

    with pytest.raises(ValueError):
        MISA(make_config(vocab_size=120, accum_steps=0))

    d, _ = _model("fp32", embed_update="deferred")
    dfresh, _ = _model("fp32", embed_update="deferred")
    with pytest.raises(_lib.MMDAError, match="deferred"):
        _step(d, b, accum_index=0, accum_count=2)
    _step(d, b)
    _step(dfresh, b)
    d.flush_embedding(); dfresh.flush_embedding()
    _assert_state_equal(_state(d), _state(dfresh))


def _accum_solver(**kw):
    from mmda_amd import make_config, models
    from mmda_amd.solver import Solver
    cfg = orc.default_config(vocab_size=120, learning_rate=LR, clip=CLIP)
    c = make_config(precision="fp32", device=DEV, n_epoch=1, name="accum", accum_steps=2, **kw, **vars(cfg))
    train = [orc.synth_batch(cfg, 6, 9, 90 + i, ragged=True) for i in range(2)]
    m = models.MISA(c)
    m.load_state_dict(orc.synth_params(cfg, 21))
    return Solver(c, c, c, ListLoader([_tuple_of(b) for b in train]), ListLoader([]), ListLoader([]), is_train=True, model=m)


def test_solver_refusals():
    from mmda_amd import _lib
    with pytest.raises(_lib.MMDAError, match="RMSprop"):
        _accum_solver(optimizer="RMSprop").build()
    with pytest.raises(_lib.MMDAError, match="deferred"):
        _accum_solver(embed_update="deferred").build()
    s = _accum_solver().build()
    with pytest.raises(_lib.MMDAError, match="train_epoch_unfused"):
        s.train_epoch_unfused()
    assert s.model._step == 0
    s.train_epoch()                                          # ... and the fused path still trains
    assert s.model._step == 1 and not s.model.cluster_aborted()
