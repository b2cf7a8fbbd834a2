"""GPU: config.embed_update = 'deferred' -- dense Adam on embed.weight with the update of the rows a batch does not touch applied when a
row is next needed, or by a flush, instead of by a pass over the table every step.  The oracle is the dense path itself: the same
adam1() runs on the same operands in the same order, so after a flush the table and its two moments are compared with torch.equal --
no tolerance anywhere in this file.  Gradient rows of the op-level tests are multiples of 1/8 in [-8, 8]: every summation order is
exact, so index_add_ is a reference for the sums bit for bit."""
import os
import socket

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import misa_oracle as orc

DEV = "cuda:0"
SHAPES = [(6, 9), (4, 12), (6, 5), (7, 9), (5, 10), (6, 8)]        # (B, T): six ragged batches around 6 x 9
MORE = [(6, 9), (3, 11), (8, 7), (5, 9)]                           # ten steps with the above: window 4 wraps and flushes at steps 4 and 8


# ================================================================================================ op level
def _op_problem(V, D, n, steps, with_lengths):
    """Initial (P, M, V) with non-zero moments, per-step (ids, rows, lengths, lr).  Rows 0..3 are never touched, rows 4 and 5 at steps
    1 and 6 only; every list repeats ids and holds ids < 0 and ids >= V."""
    g = torch.Generator().manual_seed(1000 * D + n)
    P0 = torch.randn(V, D, generator=g)
    M0 = torch.randn(V, D, generator=g) * 0.1
    V0 = torch.rand(V, D, generator=g) * 0.01 + 1e-4
    B = 8 if with_lengths else 0
    out = []
    for s in range(1, steps + 1):
        ids = torch.randint(6, V, (n,), generator=g)
        ids[::7] = ids[3]                                    # repeats, spread over the list
        if s in (1, 6):
            ids[1] = 4; ids[n // 2] = 5; ids[n - 2] = 4
        ids[2] = -1; ids[n // 3] = V; ids[n - 1] = V + 5; ids[5] = -7
        rows = torch.randint(-64, 65, (n, D), generator=g).float() / 8.0
        lengths = None
        if with_lengths:
            T = n // B
            lengths = torch.randint(1, T + 1, (B,), generator=g).sort(descending=True).values.int()
            lengths[0] = T
        out.append((ids, rows, lengths, 1e-3 * (1.0 + 0.37 * s)))
    return (P0, M0, V0), out


def _valid_positions(ids, lengths, V):
    ok = (ids >= 0) & (ids < V)
    if lengths is not None:
        B = lengths.numel()
        p = torch.arange(ids.numel())
        ok &= (p // B) < lengths.long()[p % B]
    return ok


def _step_number(s):
    """Adam step number of the s-th update: 1, 3, 4, 6, 7, 9 ... -- numbers may skip (an optimizer whose counter other calls advance),
    and dense Adam only ever sees the numbers it is given."""
    return s + s // 2


def _dense_reference(state0, steps, clip, gscale):
    from mmda_amd import ops
    P, M, Vv = [x.clone().to(DEV) for x in state0]
    V = P.shape[0]
    for s, (ids, rows, lengths, lr) in enumerate(steps, 1):
        ok = _valid_positions(ids, lengths, V)
        G = torch.zeros_like(P)
        G.index_add_(0, ids[ok].to(DEV), rows[ok].to(DEV))
        ops.clamp_adam(P.view(-1), G.view(-1), M.view(-1), Vv.view(-1), lr, _step_number(s), clip=clip, grad_scale=gscale)
    return [x.cpu() for x in (P, M, Vv)]


def _deferred_run(state0, steps, clip, gscale, window):
    from mmda_amd import ops
    P, M, Vv = [x.clone().to(DEV) for x in state0]
    st = ops.embed_deferred_state(P.shape[0], window)
    for s, (ids, rows, lengths, lr) in enumerate(steps, 1):
        ops.embed_rows_dense_adam(P, M, Vv, st, ids.to(DEV), rows.to(DEV), lr, _step_number(s),
                                  lengths=None if lengths is None else lengths.to(DEV), clip=clip, grad_scale=gscale)
    before = [x.cpu().clone() for x in (P, M, Vv)]
    ops.embed_rows_flush(P, M, Vv, st)
    after = [x.cpu().clone() for x in (P, M, Vv)]
    ops.embed_rows_flush(P, M, Vv, st)                      # nothing stale: nothing is written
    again = [x.cpu().clone() for x in (P, M, Vv)]
    return before, after, again, st.row_step.cpu()


@pytest.mark.parametrize("with_lengths", [False, True])
@pytest.mark.parametrize("window", [256, 4, 1])
@pytest.mark.parametrize("D", [300, 20])
def test_op_rows_update_then_flush_equals_dense_adam(D, window, with_lengths):
    V, n, nsteps = 64, 40, 7
    state0, steps = _op_problem(V, D, n, nsteps, with_lengths)
    touched = [set(ids[_valid_positions(ids, l, V)].tolist()) for ids, _, l, _ in steps]
    assert all(not (t & {0, 1, 2, 3}) for t in touched)
    if not with_lengths:
        assert all(({4, 5} <= t) == (i in (0, 5)) and (not (t & {4, 5}) or i in (0, 5)) for i, t in enumerate(touched))
    assert all(len(ids.unique()) < n and int(ids.min()) < 0 and int(ids.max()) >= V for ids, _, _, _ in steps)
    clip, gscale = 3.0, 0.5
    ref = _dense_reference(state0, steps, clip, gscale)
    before, after, again, row_step = _deferred_run(state0, steps, clip, gscale, window)
    for name, r, a, a2 in zip("PMV", ref, after, again):
        assert torch.equal(r, a), (name, int((r != a).sum()))
        assert torch.equal(a, a2), name
    assert torch.equal(row_step, torch.full((V,), nsteps, dtype=torch.int32))
    if window > nsteps:
        # no table-sized pass ran: rows no list touched hold their initial bits until the flush (and dense Adam moved them)
        for name, b, s0, r in zip("PMV", before, state0, ref):
            assert torch.equal(b[:4], s0[:4]), name
            assert not torch.equal(r[:4], s0[:4]), name
    # the same steps on a fresh copy: the same bits (no float atomics, one writer per row)
    _, after2, _, _ = _deferred_run(state0, steps, clip, gscale, window)
    for a, a2 in zip(after, after2):
        assert torch.equal(a, a2)


def test_op_sorted_list_form_equals_dense_adam():
    """3200 positions: the stable sort and the two-level list-order sum (segments spanning several 64-position runs)."""
    V, D, n = 64, 20, 3200
    state0, steps = _op_problem(V, D, n, 3, True)
    ref = _dense_reference(state0, steps, 2.0, 1.0)
    _, after, _, _ = _deferred_run(state0, steps, 2.0, 1.0, 256)
    for name, r, a in zip("PMV", ref, after):
        assert torch.equal(r, a), (name, int((r != a).sum()))


def test_op_catch_up_brings_listed_rows_only():
    """Rows listed at non-padding positions hold dense Adam's bits after a catch-up; the other rows are not written."""
    from mmda_amd import ops
    V, D = 64, 300
    state0, steps = _op_problem(V, D, 40, 5, False)
    ref = _dense_reference(state0, steps, 3.0, 1.0)
    P, M, Vv = [x.clone().to(DEV) for x in state0]
    st = ops.embed_deferred_state(V, 256)
    for s, (ids, rows, _, lr) in enumerate(steps, 1):
        ops.embed_rows_dense_adam(P, M, Vv, st, ids.to(DEV), rows.to(DEV), lr, _step_number(s), clip=3.0)
    ids = torch.tensor([[0, 2, -1, 2], [V, 1, 3, 0]], dtype=torch.int64)          # (T, B) = (2, 4); lengths leave out row 3
    lengths = torch.tensor([2, 2, 1, 1], dtype=torch.int32)
    ops.embed_rows_catch_up(P, M, Vv, st, ids.to(DEV), lengths=lengths.to(DEV))
    for name, got, r, s0 in zip("PMV", (P, M, Vv), ref, state0):
        got = got.cpu()
        assert torch.equal(got[:3], r[:3]), name
        assert torch.equal(got[3], s0[3]), name
    assert st.row_step.cpu()[:4].tolist() == [5, 5, 5, 0]


# ================================================================================================ model level
def _model(mode, precision, vocab, window=256, seed=9):
    from mmda_amd import make_config, MISA
    cfg = orc.default_config(vocab_size=vocab)                 # dropout on (0.1, and the fusion layer's own)
    P = orc.synth_params(cfg, seed)
    m = MISA(make_config(precision=precision, device=DEV, embed_update=mode, embed_deferred_window=window, **vars(cfg)))
    m.load_state_dict(P); m.to(DEV)
    return m, cfg, P


def _step(m, b, lr=1e-3, clip=1.0, **kw):
    m.train_step(b["t"].to(DEV), b["v"].to(DEV), b["a"].to(DEV), b["l"], b["emo"].to(DEV), lr=lr, clip=clip, **kw)


def _batches(cfg, shapes, seed=50):
    return [orc.synth_batch(cfg, B, T, seed + i, ragged=True) for i, (B, T) in enumerate(shapes)]


def _touched(b):
    T, B = b["t"].shape
    return torch.unique(b["t"][torch.arange(T).unsqueeze(1) < b["l"].unsqueeze(0)])


def _raw_table(m):
    off, (V, D) = m._layout["embed.weight"]
    P, _, M, Vv = m.flat_buckets()
    return [x[off:off + V * D].view(V, D).detach().cpu().clone() for x in (P, M, Vv)]


def _assert_models_equal(dense, deferred, what=""):
    deferred.flush_embedding()
    torch.cuda.synchronize()
    a, b = dense.state_dict(), deferred.state_dict()
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k, int((a[k] != b[k]).sum()))
    for i, name in ((2, "M"), (3, "V")):
        x, y = dense.flat_buckets()[i], deferred.flat_buckets()[i]
        assert torch.equal(x, y), (what, name, int((x != y).sum()))
    assert not dense.cluster_aborted() and not deferred.cluster_aborted()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("window", [256, 4])
def test_fused_steps_equal_dense_after_flush(precision, window):
    """Same state, batches, seeds and per-step learning rates.  window = 4 over ten steps wraps the ring twice and forces the flushes of
    steps 4 and 8."""
    shapes = SHAPES if window == 256 else SHAPES + MORE
    dense, cfg, P0 = _model("dense", precision, 120)
    deferred, _, _ = _model("deferred", precision, 120, window)
    train = _batches(cfg, shapes)
    never = sorted(set(range(120)) - set().union(*[set(_touched(b).tolist()) for b in train]))
    assert never
    for i, b in enumerate(train):
        for m in (dense, deferred):
            _step(m, b, lr=1e-3 * (1 + 0.25 * i), seed=900 + i)
    assert deferred.embed.weight.grad is None
    ids_a, rows_a = dense.embedding_grad_rows()
    ids_b, rows_b = deferred.embedding_grad_rows()
    assert torch.equal(ids_a, ids_b) and torch.equal(rows_a, rows_b)
    assert dense.read_losses() == deferred.read_losses()
    if window == 256:
        # before the flush a row touched in step 1 and never again still holds the moments step 1 left (dense Adam has decayed them
        # five times since): no pass over the table ran
        later = set().union(*[set(_touched(b).tolist()) for b in train[1:]])
        once = sorted(set(_touched(train[0]).tolist()) - later)
        assert once
        raw, ref = _raw_table(deferred), _raw_table(dense)
        assert not torch.equal(raw[1][once], ref[1][once]) and not torch.equal(raw[2][once], ref[2][once])
        assert float(raw[1][never].abs().max()) == 0.0 and torch.equal(raw[0][never], P0["embed.weight"][never])
    _assert_models_equal(dense, deferred, f"{precision} window {window}")
    before = _raw_table(deferred)
    deferred._df_dirty = True                                 # a flush with nothing stale changes nothing
    deferred.flush_embedding()
    for x, y in zip(before, _raw_table(deferred)):
        assert torch.equal(x, y)


def test_sorted_list_steps_equal_dense_after_flush():
    """B = 64, T = 50: 3200 positions take the sorted path (segments span 64-position runs), bf16."""
    dense, cfg, _ = _model("dense", "bf16", 500)
    deferred, _, _ = _model("deferred", "bf16", 500)
    for i in range(3):
        b = orc.synth_batch(cfg, 64, 50, 70 + i, ragged=True)
        for m in (dense, deferred):
            _step(m, b, lr=1e-3 * (1 + i), seed=40 + i)
    _assert_models_equal(dense, deferred, "sorted")


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


def _solver(mode, precision="fp32", optimizer="Adam", window=256, build=True):
    from mmda_amd import make_config, models
    from mmda_amd.solver import Solver
    cfg = orc.default_config(vocab_size=120, learning_rate=1e-3)
    c = make_config(precision=precision, device=DEV, n_epoch=1, optimizer=optimizer, name="df", embed_update=mode,
                    embed_deferred_window=window, **vars(cfg))
    train = _batches(cfg, SHAPES)
    dev = _batches(cfg, SHAPES[:2], seed=150)
    m = models.MISA(c)
    m.load_state_dict(orc.synth_params(cfg, 9))
    s = Solver(c, c, c, ListLoader([_tuple_of(b) for b in train]), ListLoader([_tuple_of(b) for b in dev]),
               ListLoader([_tuple_of(b) for b in dev]), is_train=True, model=m)
    if build:
        torch.manual_seed(1234)                                # build() draws weight_hh (orthogonal_) from torch's generator
        s.build()
    return s, train, dev


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_unfused_order_equals_dense(precision):
    """forward, the six getters, loss.backward(), clip_grad_value_, optimizer.step(): the rows update runs in optimizer.step()."""
    a, _, _ = _solver("dense", precision)
    b, _, _ = _solver("deferred", precision)
    la = a.train_epoch_unfused()
    lb = b.train_epoch_unfused()
    assert la == lb
    assert b.model.embed.weight.grad is None
    _assert_models_equal(a.model, b.model, "unfused")


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_gradient_step_then_clip_then_optimizer_step_equals_dense(precision):
    """train_step(do_adam=False), clip_grad_value_, optimizer.step(): both calls advance the model's step counter, so the Adam step
    numbers run 2, 4, 6 ... and dense Adam never sees the odd ones; the deferred table must not replay them either.  Then a gradient-only
    step that no optimizer step follows, between fused steps."""
    from mmda_amd import optim
    a, train, _ = _solver("dense", precision)
    b, _, _ = _solver("deferred", precision, window=4)
    for s in (a, b):
        m = s.model
        for i, bt in enumerate(train):
            _step(m, bt, do_adam=False, seed=700 + i)
            optim.clip_grad_value_(m, 1.0)
            s.optimizer.step()
        assert m._step == 2 * len(train)
        _step(m, train[0], seed=800, optimizer=s.optimizer)
        _step(m, train[1], do_adam=False, seed=801)           # its gradient is dropped: the next step clears the bucket
        _step(m, train[2], seed=802, optimizer=s.optimizer)
    assert b.model.embed.weight.grad is None
    _assert_models_equal(a.model, b.model, "do_adam=False, clip, step")


def test_native_adam_step_applies_the_pending_rows():
    """mmda_misa_adam_step behind a gradient-only step (the C-level order; Python steps through optim.Adam): dense against deferred."""
    from mmda_amd import _lib
    dense, cfg, _ = _model("dense", "fp32", 120)
    deferred, _, _ = _model("deferred", "fp32", 120)
    train = _batches(cfg, SHAPES[:4])
    for m in (dense, deferred):
        for i, bt in enumerate(train):
            _step(m, bt, do_adam=False, seed=600 + i)
            _lib.check(m._lib.mmda_misa_adam_step(m._h, 1e-3 * (1 + i), 1.0, 1.0, m._step, _lib.stream_ptr()), "adam_step")
            m._rows_pending = False
        m._df_dirty = True
    _assert_models_equal(dense, deferred, "mmda_misa_adam_step")


def test_eval_between_steps_equals_dense():
    """Solver.eval() between epochs reads rows the training batches left stale: catch-up runs inside every forward."""
    a, _, dev = _solver("dense")
    b, _, _ = _solver("deferred")
    for s in (a, b):
        s.train_epoch()
    ra, rb = a.eval("dev"), b.eval("dev")
    assert ra[0] == rb[0] and ra[1] == rb[1] and np.array_equal(ra[2], rb[2])
    d = dev[0]
    with torch.no_grad():
        sa, _ = a.model(d["t"].to(DEV), d["v"].to(DEV), d["a"].to(DEV), d["l"])
        sb, _ = b.model(d["t"].to(DEV), d["v"].to(DEV), d["a"].to(DEV), d["l"])
    assert torch.equal(sa, sb)
    for s in (a, b):
        s.train_epoch()
    _assert_models_equal(a.model, b.model, "eval between epochs")


def test_checkpoints_cross_the_modes():
    """state_dict() / optimizer.state_dict() of a deferred run hold the flushed table without an explicit flush; a checkpoint written in
    either mode loads in the other, and two further steps give equal results."""
    saved = {}
    for mode in ("dense", "deferred"):
        s, train, _ = _solver(mode)
        for i, b in enumerate(train[:3]):
            _step(s.model, b, seed=300 + i, optimizer=s.optimizer)
        sd = {k: v.detach().cpu().clone() for k, v in s.model.state_dict().items()}          # (no flush_embedding() here)
        saved[mode] = (sd, s.optimizer.state_dict())
    for k in saved["dense"][0]:
        assert torch.equal(saved["dense"][0][k], saved["deferred"][0][k]), k
    for k in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(saved["dense"][1][k], saved["deferred"][1][k]), k
    assert saved["deferred"][1]["step"] == 3
    models = []
    for written, loaded in (("deferred", "dense"), ("dense", "deferred"), ("deferred", "deferred")):
        s, train, _ = _solver(loaded)
        sd, osd = saved[written]
        s.model.load_state_dict(sd); s.model.to(DEV)
        b0 = train[3]
        s.model._prepare(b0["t"].to(DEV), b0["v"].to(DEV), b0["a"].to(DEV), b0["l"])
        s.optimizer.load_state_dict(osd)
        assert s.model._step == 3
        for i, b in enumerate(train[3:5]):
            _step(s.model, b, seed=400 + i, optimizer=s.optimizer)
        models.append(s.model)
    _assert_models_equal(models[0], models[1], "deferred -> dense against dense -> deferred")
    _assert_models_equal(models[0], models[2], "deferred -> dense against deferred -> deferred")


def test_switching_the_mode_flushes_first():
    dense, cfg, _ = _model("dense", "fp32", 120)
    m, _, _ = _model("deferred", "fp32", 120)
    train = _batches(cfg, SHAPES)
    for i, b in enumerate(train[:3]):
        _step(dense, b, seed=i); _step(m, b, seed=i)
    m.set_embed_update("dense")
    for i, b in enumerate(train[3:5]):
        _step(dense, b, seed=10 + i); _step(m, b, seed=10 + i)
    m.set_embed_update("deferred")
    _step(dense, train[5], seed=20); _step(m, train[5], seed=20)
    _assert_models_equal(dense, m, "dense <-> deferred")


def test_rmsprop_raises_at_build():
    from mmda_amd import _lib
    s, _, _ = _solver("deferred", optimizer="RMSprop", build=False)
    with pytest.raises(_lib.MMDAError):
        s.build()


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _dp_worker(rank, world, port, q):
    import sys
    import torch.distributed as dist
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from mmda_amd import make_config, MISA, _lib
        from mmda_amd.solver import Solver
        c = make_config(precision="fp32", device="cuda:0", embed_update="deferred", **vars(orc.default_config(vocab_size=120)))
        s = Solver(c, c, c, ListLoader([]), ListLoader([]), ListLoader([]), is_train=True, model=MISA(c))
        try:
            s.build()
            q.put((rank, "built"))
        except _lib.MMDAError as e:
            q.put((rank, "MMDAError: " + str(e)))
    finally:
        dist.destroy_process_group()


def test_two_ranks_raise_at_build():
    import torch.multiprocessing as mp
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = dict(q.get(timeout=150) for _ in range(world))
    finally:
        for p in procs:
            p.join(timeout=120)
            if p.is_alive():
                p.kill()
    for r in range(world):
        assert res[r].startswith("MMDAError") and "not built yet" in res[r], res[r]
