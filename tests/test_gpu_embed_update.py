"""GPU: config.embed_update = 'sparse' (torch.optim.SparseAdam on the rows a batch touches, fused with the coalescing of the
gradient rows) and 'frozen' (the table never changes and no gradient for it is computed), from the op-level entry point up to
``Solver``.  Oracles: torch.optim.SparseAdam on the CPU fed the clipped coalesced rows; ``oracle.misa_oracle`` with
``G["embed.weight"] = None`` for everything else.  Touched rows = distinct ids at non-padding positions of the (T, B) id tensor.
Dropout is off wherever the CPU oracle is the reference (as in test_gpu_solver.py)."""
import os
import socket

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import misa_oracle as orc

DEV = "cuda:0"
SHAPES = [(6, 9), (4, 12), (6, 5)] * 2          # (B, T) of consecutive batches; six steps: rows are touched, skipped, touched again
LOSS_KEYS = ("cls", "diff", "sim", "recon", "conf", "total")
EPS23 = 2.0 ** -23


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


def _solver(monkeypatch, embed_update, precision="fp32", shapes=SHAPES, seed=50, optimizer="Adam", lr=1e-3, clip=1.0, build=True):
    from mmda_amd import make_config, models
    from mmda_amd.solver import Solver
    monkeypatch.setattr(models, "FUSION_DROPOUT", 0.0)
    cfg = orc.default_config(vocab_size=80, dropout=0.0, learning_rate=lr, clip=clip)
    c = make_config(precision=precision, device=DEV, n_epoch=1, optimizer=optimizer, name="eu", embed_update=embed_update, **vars(cfg))
    train = [orc.synth_batch(cfg, B, T, seed + i, ragged=True) for i, (B, T) in enumerate(shapes)]
    dev = [orc.synth_batch(cfg, B, T, seed + 100 + i, ragged=True) for i, (B, T) in enumerate(shapes[:2])]
    m = models.MISA(c)
    m.load_state_dict(orc.synth_params(cfg, 9))
    s = Solver(c, c, c, ListLoader([_tuple_of(b) for b in train]), ListLoader([_tuple_of(b) for b in dev]),
               ListLoader([_tuple_of(b) for b in dev]), is_train=True, model=m)
    if not build:
        return s, cfg, None, train, dev
    s.build()
    P = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    return s, cfg, P, train, dev


def _assert_params_match(model, P_ref, P0, cfg, steps, lr):
    """The bounds of tests/test_gpu_solver.py::_assert_params_match, taken over unchanged: hard bound 2 steps lr, 99 % of the elements
    within 0.01 steps lr, update within 2e-2 relative L2."""
    for k, p in model.state_dict().items():
        got, ref, base = p.detach().cpu().numpy(), P_ref[k].numpy(), P0[k].numpy()
        if k.endswith("self_attn.in_proj_bias"):
            hs = cfg.hidden_size
            keep = np.ones(3 * hs, bool); keep[hs:2 * hs] = False
            got, ref, base = got[keep], ref[keep], base[keep]
        d = np.abs(got - ref)
        frac = float((d <= 0.01 * steps * lr).mean())
        upd_ref = (ref - base).astype(np.float64); upd = (got - base).astype(np.float64)
        rel = float(np.linalg.norm(upd - upd_ref) / np.linalg.norm(upd_ref)) if np.linalg.norm(upd_ref) > 0 else 0.0
        if k == "embed.weight":
            print(f"embed.weight: max |d| {d.max():.3e} (bound {2 * steps * lr:.1e}), bulk {frac:.4f}, update rel L2 {rel:.3e}")
        assert d.max() <= 2 * steps * lr + 1e-7, k
        assert frac >= 0.99, (k, frac)
        if np.linalg.norm(upd_ref) > 0:
            assert rel <= 2e-2, (k, rel)
        else:
            assert np.abs(upd).max() == 0.0, k


def _valid(b):
    """(T, B) bool: the non-padding positions of a batch"""
    T, B = b["t"].shape
    return torch.arange(T).unsqueeze(1) < b["l"].unsqueeze(0)


def _touched(b):
    return torch.unique(b["t"][_valid(b)])


def _pad_only(b):
    """ids that occur in the batch's id tensor at padded positions only"""
    pad_ids = torch.unique(b["t"][~_valid(b)])
    return pad_ids[~torch.isin(pad_ids, _touched(b))]


def _oracle_loop(P0, cfg, train, mode):
    """fwd, losses, bwd, clamp; embed.weight's gradient is taken out (G = None: AdamState skips it) and, in 'sparse' mode, fed as
    the rows of the touched ids to torch.optim.SparseAdam.  Returns (P, per-step losses, table elements clamped per step)."""
    P = {k: v.clone() for k, v in P0.items()}
    opt = orc.AdamState(P, cfg.learning_rate)
    emb = P["embed.weight"].clone().requires_grad_(True)
    sopt = torch.optim.SparseAdam([emb], lr=cfg.learning_rate)
    losses, clamped = [], []
    for b in train:
        P["embed.weight"] = emb.detach()
        _, L, G = orc.loss_and_grads(P, cfg, b)
        losses.append({k: float(getattr(L, k)) for k in LOSS_KEYS})
        clamped.append(int((G["embed.weight"].abs() > cfg.clip).sum()))
        G = {k: (None if g is None else g.clamp(-cfg.clip, cfg.clip)) for k, g in G.items()}
        Ge = G["embed.weight"]
        G["embed.weight"] = None
        opt.step(P, G)
        if mode == "sparse":
            ids = _touched(b)
            # (no gradient flows through padding: outside the touched rows the oracle's dense gradient is exactly zero)
            rest = torch.ones(Ge.shape[0], dtype=torch.bool); rest[ids] = False
            assert float(Ge[rest].abs().max()) == 0.0
            emb.grad = torch.sparse_coo_tensor(ids.unsqueeze(0), Ge[ids], Ge.shape)
            sopt.step()
    P["embed.weight"] = emb.detach()
    return P, losses, clamped


def _table_state(m):
    off, (V, D) = m._layout["embed.weight"]
    P, _, M, Vv = m.flat_buckets()
    return [x[off:off + V * D].view(V, D).detach().cpu().clone() for x in (P, M, Vv)]


def _check_batch_properties(train, vocab):
    """What the six batches are chosen for, asserted from the ids and lengths: rows touched / skipped / touched again, rows never
    touched, and in every batch ids that occur at padded positions only."""
    touched = [set(_touched(b).tolist()) for b in train]
    again = [r for r in set().union(*touched)
             if any(r in touched[i] and r not in touched[j] and r in touched[k]
                    for i in range(len(train)) for j in range(i + 1, len(train)) for k in range(j + 1, len(train)))]
    never = sorted(set(range(vocab)) - set().union(*touched))
    assert len(again) >= 5 and len(never) >= 2
    assert len({b["t"].shape for b in train}) >= 2 and len(train) >= 6
    for b in train:
        assert _pad_only(b).numel() > 0 and int(b["l"].min()) < b["t"].shape[0]
    return never


# ------------------------------------------------------------------------------------------------ 1: the op, both list lengths
def _op_inputs(T, B, V, step, heavy):
    g = torch.Generator().manual_seed(1000 * T + step)
    ids = torch.randint(0, V, (T, B), generator=g)
    # a few ids many times: the owner's four quarters (short lists); segments that span several 64-position runs (sorted lists)
    for k, (idv, cnt) in enumerate(heavy):
        pos = torch.randperm(T * B, generator=g)[:cnt]
        ids.view(-1)[pos] = idv + step                   # (another row every step: touched, then skipped)
    lengths = torch.randint(1, T + 1, (B,), generator=g).sort(descending=True).values
    lengths[0] = T
    rows = torch.randn(T * B, 300, generator=g) * 3
    return ids, rows, lengths.to(torch.int32)


def _sparse_adam_reference(P, steps, lr, clip, scale=1.0):
    """torch.optim.SparseAdam on the CPU: per step sparse_coo(unique valid ids, clamp(scale * index_add sum)).  Returns
    (P, M, V, touched mask, largest |g|, largest multiplicity)."""
    p = P.clone().requires_grad_(True)
    opt = torch.optim.SparseAdam([p], lr=lr)
    touched = torch.zeros(P.shape[0], dtype=torch.bool)
    gmax, rmax = 0.0, 0
    for ids, rows, lengths in steps:
        T, B = ids.shape
        valid = (torch.arange(T).unsqueeze(1) < lengths.unsqueeze(0)).reshape(-1) & (ids.reshape(-1) >= 0)
        vid = ids.reshape(-1)[valid]
        dense = torch.zeros_like(P).index_add_(0, vid, rows[valid])
        uniq, counts = torch.unique(vid, return_counts=True)
        g = (dense[uniq] * scale).clamp(-clip, clip)
        p.grad = torch.sparse_coo_tensor(uniq.unsqueeze(0), g, P.shape)
        opt.step()
        touched[uniq] = True
        gmax = max(gmax, float(g.abs().max())); rmax = max(rmax, int(counts.max()))
    st = opt.state[p]
    return p.detach(), st["exp_avg"], st["exp_avg_sq"], touched, gmax, rmax


def _assert_rows_match(got, ref, init, touched, gmax, rmax, what=""):
    """Untouched rows: bit for bit their initial values.  Touched rows of P: the project's bound for its dense kernel against torch over
    three steps (test_gpu_ops.py::test_clamp_adam_matches_torch_adam_three_steps), 2e-6.  Touched rows of M / V: at most three fp32
    roundings per element on either side plus the roundings of the row sum, whose order differs (four quarters then combined / list
    order runs against the CPU's index_add), and the two terms of a moment can cancel -- hence absolute:
    (4 + r) 2^-23 max(|M_ref|, |g|), r = the most valid positions one id has; with g^2 for V."""
    (P, M, V), (Pr, Mr, Vr), (P0, M0, V0) = got, ref, init
    for a, a0 in ((P, P0), (M, M0), (V, V0)):
        assert torch.equal(a[~touched], a0[~touched]), what
    dP = float((P[touched] - Pr[touched]).abs().max())
    bM = (4 + rmax) * EPS23 * max(float(Mr.abs().max()), gmax)
    bV = (4 + rmax) * EPS23 * max(float(Vr.abs().max()), gmax * gmax)
    dM = float((M[touched] - Mr[touched]).abs().max()); dV = float((V[touched] - Vr[touched]).abs().max())
    print(f"{what}: touched rows {int(touched.sum())}, r {rmax}, |g|max {gmax:.3g}: dP {dP:.3e} (< 2e-6), dM {dM:.3e} (<= {bM:.3e}), "
          f"dV {dV:.3e} (<= {bV:.3e})")
    assert dP < 2e-6, (what, dP)
    assert dM <= bM, (what, dM, bM)
    assert dV <= bV, (what, dV, bV)


@pytest.mark.parametrize("T,B,heavy", [(20, 16, [(5, 90), (40, 7)]), (50, 64, [(5, 400), (40, 70), (90, 7)])])
def test_op_matches_torch_sparse_adam_three_steps(T, B, heavy):
    """ops.embed_rows_sparse_adam, a list below and one above the length where the sorted path takes over (3072 positions)"""
    from mmda_amd import ops
    V, lr, clip = 997, 1e-3, 1.0
    assert (T * B >= 3072) == (B == 64)
    g = torch.Generator().manual_seed(7)
    P0 = torch.randn(V, 300, generator=g); M0 = torch.randn(V, 300, generator=g) * 0.01; V0 = torch.rand(V, 300, generator=g) * 0.01
    steps = [_op_inputs(T, B, V, k, heavy) for k in range(3)]
    # SparseAdam starts its moments at zero: so does this comparison; the non-zero start is used for the untouched-rows check below
    Pr, Mr, Vr, touched, gmax, rmax = _sparse_adam_reference(P0, steps, lr, clip)
    assert rmax >= (64 if B == 64 else 8) and 0 < int(touched.sum()) < V
    assert any(int((ids >= 0).sum()) > 0 for ids, _, _ in steps)
    runs = []
    for rep in range(2):
        p, m, v = P0.to(DEV), torch.zeros(V, 300, device=DEV), torch.zeros(V, 300, device=DEV)
        for k, (ids, rows, lengths) in enumerate(steps):
            ops.embed_rows_sparse_adam(p, m, v, ids.to(DEV), rows.to(DEV), lr, k + 1, lengths=lengths.to(DEV), clip=clip)
        runs.append((p.cpu(), m.cpu(), v.cpu()))
    _assert_rows_match(runs[0], (Pr, Mr, Vr), (P0, torch.zeros_like(P0), torch.zeros_like(P0)), touched, gmax, rmax, f"op T={T} B={B}")
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)                            # no float atomics: the same bits on a repeat
    # untouched rows keep parameter AND both (non-zero) moments bit for bit; ids < 0 and ids >= V are skipped, as is padding
    ids, rows, lengths = steps[0]
    ids = ids.clone(); ids[0, 1] = -1; ids[1, 0] = V + 3
    p, m, v = P0.to(DEV), M0.to(DEV), V0.to(DEV)
    ops.embed_rows_sparse_adam(p, m, v, ids.to(DEV), rows.to(DEV), lr, 1, lengths=lengths.to(DEV), clip=clip)
    valid = (torch.arange(T).unsqueeze(1) < lengths.unsqueeze(0)) & (ids >= 0) & (ids < V)
    t1 = torch.zeros(V, dtype=torch.bool); t1[ids[valid]] = True
    for a, a0 in ((p, P0), (m, M0), (v, V0)):
        assert torch.equal(a.cpu()[~t1], a0[~t1])
        assert not torch.equal(a.cpu()[t1], a0[t1])


# ------------------------------------------------------------------------------------------------ 2, 6, 10: sparse, fp32
@pytest.mark.parametrize("path", ["train_epoch", "train_epoch_unfused"])
def test_sparse_fp32_matches_the_oracle_loop(monkeypatch, path):
    """clip = 0.004: small enough to clamp some coalesced table rows on every step (asserted from the oracle), so the unfused order --
    clip_grad_value_ first, optimizer.step() after -- is checked to clamp the COALESCED sum inside the rows update."""
    s, cfg, P0, train, _ = _solver(monkeypatch, "sparse", clip=0.004)
    never = _check_batch_properties(train, cfg.vocab_size)
    m = s.model
    out = getattr(s, path)()
    P, losses, clamped = _oracle_loop(P0, cfg, train, "sparse")
    print("table elements clamped per step (oracle):", clamped)
    assert all(c > 0 for c in clamped)
    for k in out:
        ref = float(np.mean([l[k] for l in losses]))
        assert abs(out[k] - ref) <= 2e-4 * abs(ref) + 1e-7, (k, out[k], ref)
    _assert_params_match(m, P, P0, cfg, len(train), cfg.learning_rate)
    Pt, Mt, Vt = _table_state(m)
    assert torch.equal(Pt[never], P0["embed.weight"][never])
    assert float(Mt[never].abs().max()) == 0.0 and float(Vt[never].abs().max()) == 0.0
    every = sorted(set().union(*[set(_touched(b).tolist()) for b in train]))
    assert float(Mt[every].abs().max()) > 0.0 and not torch.equal(Pt[every], P0["embed.weight"][every])
    assert m.embed.weight.grad is None and m.embed.weight.requires_grad
    assert not m.cluster_aborted()


def _step(m, b, lr=1e-3, clip=1.0, **kw):
    m.train_step(b["t"].to(DEV), b["v"].to(DEV), b["a"].to(DEV), b["l"], b["emo"].to(DEV), lr=lr, clip=clip, **kw)


def test_sparse_mode_is_applied_and_pad_only_rows_stay(monkeypatch):
    """Config stores unknown keys silently: a build without the feature would train densely.  After step 2 a row touched in step 1
    and not in step 2 has the first moment step 1 left (dense Adam would have decayed it); a row whose id occurs only at padded
    positions of a step keeps parameter and both moments through it."""
    s, cfg, P0, train, _ = _solver(monkeypatch, "sparse")
    m = s.model
    t1, t2 = set(_touched(train[0]).tolist()), set(_touched(train[1]).tolist())
    only1 = sorted(t1 - t2)
    assert only1
    before = [P0["embed.weight"], torch.zeros_like(P0["embed.weight"]), torch.zeros_like(P0["embed.weight"])]
    for i, b in enumerate(train[:3]):
        pad_only = _pad_only(b)
        assert pad_only.numel() > 0
        _step(m, b)
        after = _table_state(m)
        for x, y in zip(before, after):
            assert torch.equal(x[pad_only], y[pad_only]), i
        if i == 0:
            M1 = after[1].clone()
            assert float(M1[only1].abs().max()) > 0.0
        if i == 1:
            assert torch.equal(after[1][only1], M1[only1]) and torch.equal(after[2][only1], before[2][only1])
            assert torch.equal(after[0][only1], before[0][only1])
        before = after


# ------------------------------------------------------------------------------------------------ 3: sparse, bf16, both list lengths
@pytest.mark.parametrize("B,T,vocab", [(8, 12, 80), (64, 50, 500)])
def test_sparse_bf16_step_applies_sparse_adam_to_its_own_gradient_rows(monkeypatch, B, T, vocab):
    """One fused bf16 step; the model's own embedding_grad_rows() (existing gradient code) and the batch's lengths through CPU
    SparseAdam give the table, within the op-level bounds: pins the update inside the bf16 step (short and sorted list) without
    leaning on bf16 gradient tolerances."""
    from mmda_amd import make_config, models
    monkeypatch.setattr(models, "FUSION_DROPOUT", 0.0)
    cfg = orc.default_config(vocab_size=vocab, dropout=0.0)
    m = models.MISA(make_config(precision="bf16", device=DEV, embed_update="sparse", **vars(cfg)))
    P = orc.synth_params(cfg, 9)
    m.load_state_dict(P); m.to(DEV)
    b = orc.synth_batch(cfg, B, T, 61, ragged=True)
    assert (T * B >= 3072) == (B == 64)
    lr, clip = 1e-3, 1.0
    _step(m, b, lr=lr, clip=clip)
    ids, rows = m.embedding_grad_rows()
    ids, rows = ids.cpu().view(T, B), rows.cpu().clone()
    assert torch.equal(ids >= 0, _valid(b))
    Pr, Mr, Vr, touched, gmax, rmax = _sparse_adam_reference(P["embed.weight"], [(ids, rows, b["l"])], lr, clip)
    assert torch.equal(torch.nonzero(touched).view(-1), _touched(b))
    z = torch.zeros_like(P["embed.weight"])
    _assert_rows_match(_table_state(m), (Pr, Mr, Vr), (P["embed.weight"], z, z), touched, gmax, rmax, f"bf16 B={B} T={T}")
    assert not m.cluster_aborted()


# ------------------------------------------------------------------------------------------------ 4: frozen, fp32
@pytest.mark.parametrize("path", ["train_epoch", "train_epoch_unfused"])
def test_frozen_fp32_matches_the_oracle_loop(monkeypatch, path):
    s, cfg, P0, train, _ = _solver(monkeypatch, "frozen")
    m = s.model
    assert all(p is not m.embed.weight for g in s.optimizer.param_groups for p in g["params"])
    out = getattr(s, path)()
    P, losses, _ = _oracle_loop(P0, cfg, train, "frozen")
    for k in out:
        ref = float(np.mean([l[k] for l in losses]))
        assert abs(out[k] - ref) <= 2e-4 * abs(ref) + 1e-7, (k, out[k], ref)
    Pt, Mt, Vt = _table_state(m)
    assert torch.equal(Pt, P0["embed.weight"]) and torch.equal(m.embed.weight.detach().cpu(), P0["embed.weight"])
    assert m.embed.weight.requires_grad is False and m.embed.weight.grad is None
    assert float(Mt.abs().max()) == 0.0 and float(Vt.abs().max()) == 0.0
    _assert_params_match(m, P, P0, cfg, len(train), cfg.learning_rate)
    assert not m.cluster_aborted()


# ------------------------------------------------------------------------------------------------ 5: one step against dense
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("B,T,ragged", [(32, 50, False), (8, 12, True)])
@pytest.mark.parametrize("mode", ["frozen", "sparse"])
def test_one_step_leaves_every_other_parameter_as_dense_does(mode, B, T, ragged, precision):
    """Same parameters, same batch, same seed, dropout ON: the step-1 gradients of the other parameters do not depend on how the
    table is updated and the step is deterministic, so every non-embedding parameter (and its moments) is equal bit for bit: skipping
    the dX / scatter / clear work altered nothing else.  (T B < 8192: above it the grouped GEMM launches split K by a target that
    depends on what else is in the launch, and equality would hold only up to that reordering.)"""
    from mmda_amd import make_config, MISA
    assert T * B < 8192
    cfg = orc.default_config(vocab_size=300)
    P = orc.synth_params(cfg, 9)
    b = orc.synth_batch(cfg, B, T, 77, ragged=ragged)
    got = {}
    for mo in ("dense", mode):
        m = MISA(make_config(precision=precision, device=DEV, embed_update=mo, **vars(cfg)))
        m.load_state_dict(P); m.to(DEV)
        _step(m, b, lr=1e-3, clip=1.0, seed=1234)
        torch.cuda.synchronize()
        assert not m.cluster_aborted()
        n = m.dense_floats
        got[mo] = [x[:n].cpu().clone() for x in (m.flat_buckets()[0], m.flat_buckets()[2], m.flat_buckets()[3])] + [_table_state(m)[0]]
        losses = m.read_losses()
        got[mo].append(losses)
    for k, (a, c) in enumerate(zip(got["dense"][:3], got[mode][:3])):
        bad = int((a != c).sum())
        assert bad == 0, (("P", "M", "V")[k], bad, float((a - c).abs().max()))
    assert got["dense"][4] == got[mode][4]
    assert not torch.equal(got["dense"][3], P["embed.weight"])
    if mode == "frozen":
        assert torch.equal(got[mode][3], P["embed.weight"])
    else:
        touched = _touched(b)
        rest = torch.ones(cfg.vocab_size, dtype=torch.bool); rest[touched] = False
        assert torch.equal(got[mode][3][rest], P["embed.weight"][rest])
        assert not torch.equal(got[mode][3][touched], P["embed.weight"][touched])


# ------------------------------------------------------------------------------------------------ 7: checkpoints across modes
def test_checkpoint_across_modes(monkeypatch):
    s, cfg, P0, train, _ = _solver(monkeypatch, "sparse")
    m = s.model
    for b in train[:3]:
        _step(m, b, optimizer=s.optimizer)
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    osd = s.optimizer.state_dict()
    assert len(sd) == 99 and osd["mmda_flat"] and osd["step"] == 3 and osd["exp_avg"].numel() == m.flat_buckets()[0].numel()
    _step(m, train[3], optimizer=s.optimizer)
    want = [x.cpu().clone() for x in (m.flat_buckets()[0], m.flat_buckets()[2], m.flat_buckets()[3])]
    for mode in ("sparse", "dense", "frozen"):
        s2, _, _, _, _ = _solver(monkeypatch, mode)
        s2.model.load_state_dict(sd); s2.model.to(DEV)
        b0 = train[3]
        s2.model._prepare(b0["t"].to(DEV), b0["v"].to(DEV), b0["a"].to(DEV), b0["l"])
        s2.optimizer.load_state_dict(osd)
        assert s2.model._step == 3
        assert torch.equal(s2.model.flat_buckets()[2].cpu(), osd["exp_avg"])        # (frozen: the table's moments are carried)
        _step(s2.model, b0, optimizer=s2.optimizer)
        have = [x.cpu() for x in (s2.model.flat_buckets()[0], s2.model.flat_buckets()[2], s2.model.flat_buckets()[3])]
        assert all(bool(torch.isfinite(x).all()) for x in have)
        if mode == "sparse":
            for a, c in zip(want, have):
                assert torch.equal(a, c)
        if mode == "frozen":
            assert torch.equal(_table_state(s2.model)[0], sd["embed.weight"])
        assert len(s2.model.state_dict()) == 99


# ------------------------------------------------------------------------------------------------ 8: errors, data parallelism
def test_sparse_with_rmsprop_raises_at_build(monkeypatch):
    from mmda_amd import _lib
    s, _, _, _, _ = _solver(monkeypatch, "sparse", optimizer="RMSprop", build=False)
    with pytest.raises(_lib.MMDAError):
        s.build()
    s, _, _, _, _ = _solver(monkeypatch, "frozen", optimizer="RMSprop", build=False)
    s.build()
    s.train_epoch()
    assert s.model.embed.weight.grad is None


@pytest.mark.parametrize("mode", ["sparse", "deferred"])
def test_a_grad_sync_is_refused_in_front_of_the_step(mode):
    """train_step(grad_sync=...) under a rows mode: refused before anything changes -- the exchange is never called, no seed is drawn,
    no step is counted and the parameters keep their bits -- and the model then steps as one that was never asked."""
    from mmda_amd import _lib, make_config, models
    cfg = orc.default_config(vocab_size=120)
    c = make_config(precision="fp32", device=DEV, embed_update=mode, **vars(cfg))
    b = orc.synth_batch(cfg, 8, 12, 61, ragged=True)
    m, never = models.MISA(c), models.MISA(c)
    for x in (m, never):
        x.load_state_dict(orc.synth_params(cfg, 9))
        x.to(DEV)
    _step(m, b, seed=1); _step(never, b, seed=1)             # (buckets, workspace and moments exist)
    calls = []

    def sync(G, n):
        calls.append(n)
        return 1.0

    step_no, seed, params = m._step, m._seed, m.flat_buckets()[0].clone()
    with pytest.raises(_lib.MMDAError, match="not built yet"):
        _step(m, b, grad_sync=sync)
    assert not calls
    assert m._step == step_no and m._seed == seed
    assert torch.equal(m.flat_buckets()[0], params)
    _step(m, b); _step(never, b)
    for x, y in zip(m.flat_buckets(), never.flat_buckets()):
        assert torch.equal(x, y)


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _dp_worker(rank, world, port, q, mode):
    import sys
    import torch.distributed as dist
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from oracle import misa_oracle as orc
        from mmda_amd import make_config, MISA, _lib
        from mmda_amd.solver import Solver
        cfg = orc.default_config(vocab_size=120)
        P = orc.synth_params(cfg, 21)
        c = make_config(precision="fp32", device="cuda:0", embed_update=mode, **vars(cfg))
        m = MISA(c)
        if rank == 0:
            m.load_state_dict(P)
        s = Solver(c, c, c, ListLoader([]), ListLoader([]), ListLoader([]), is_train=True, model=m)
        if mode == "sparse":
            try:
                s.build()
                q.put((rank, "built"))
            except _lib.MMDAError as e:
                q.put((rank, "MMDAError: " + str(e)))
            return
        batch = orc.synth_batch(cfg, 6, 9, 30 + rank, ragged=True)
        d = {k: (v.to("cuda:0") if k != "l" else v) for k, v in batch.items()}
        s.build()                                      # (moves the model to the GPU and broadcasts rank 0's parameters)
        dp = s.dp
        exchanged = []
        dp._exchange_embedding_rows = lambda model: exchanged.append(1)
        for _ in range(2):
            m.train_step(d["t"], d["v"], d["a"], d["l"], d["emo"], lr=1e-3, clip=1.0, training=False, grad_sync=dp.sync,
                         optimizer=s.optimizer)
        torch.cuda.synchronize()
        sd = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
        q.put((rank, (sd, len(exchanged), float(m.flat_buckets()[2][m.dense_floats:].abs().max()))))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("mode", ["frozen", "sparse"])
def test_two_ranks(mode):
    """frozen: replicas stay bit-identical, embed.weight is untouched, no embedding exchange is issued, the rest trains.
    sparse: Solver.build() raises on every rank (not built yet)."""
    import torch.multiprocessing as mp
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, world, port, q, mode)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = dict(q.get(timeout=150) for _ in range(world))
    finally:
        for p in procs:
            p.join(timeout=120)
            if p.is_alive():
                p.kill()
    for p in procs:
        assert p.exitcode == 0
    if mode == "sparse":
        for r in range(world):
            assert res[r].startswith("MMDAError") and "not built yet" in res[r], res[r]
        return
    cfg = orc.default_config(vocab_size=120)
    P = orc.synth_params(cfg, 21)
    (sd0, ex0, mom0), (sd1, ex1, mom1) = res[0], res[1]
    assert ex0 == 0 and ex1 == 0 and mom0 == 0.0 and mom1 == 0.0
    for k in sd0:
        np.testing.assert_array_equal(sd0[k], sd1[k], err_msg=k)
    np.testing.assert_array_equal(sd0["embed.weight"], P["embed.weight"].numpy())
    moved = [k for k in sd0 if k != "embed.weight" and "weight_hh" not in k and not np.array_equal(sd0[k], P[k].numpy())]
    assert len(moved) > 50


# ------------------------------------------------------------------------------------------------ 9: evaluation
@pytest.mark.parametrize("mode", ["sparse", "frozen"])
def test_eval_does_not_depend_on_the_mode(monkeypatch, mode):
    s, cfg, P0, train, dev = _solver(monkeypatch, mode)
    s.train_epoch()
    loss, acc, pred, truth = s.eval("dev")
    sd = {k: v.detach().cpu().clone() for k, v in s.model.state_dict().items()}
    s2, _, _, _, _ = _solver(monkeypatch, "dense")
    s2.model.load_state_dict(sd); s2.model.to(DEV)
    loss2, acc2, pred2, truth2 = s2.eval("dev")
    assert loss == loss2 and acc == acc2
    assert np.array_equal(pred, pred2) and np.array_equal(truth, truth2)
