"""GPU: the encoder cache -- ``mmda_encoded_gather`` / ``mmda_encoded_collect`` against torch indexing, ``EncoderCache.build`` against the
workspace of an evaluation forward and against the fp32 oracle's encoders, and a step that starts behind the encoders
(``MISA.train_step_encoded``) against the step under the encoder cut on the same batch: bit for bit, since from the projections on the
two issue the same launches.  Then the oracle behind the encoders, the Solver, the absence of synchronisation, staleness and refusals.
Tolerances are those of tests/test_gpu_model.py (max error relative to the tensor's max magnitude, 1e-4 in fp32, 1e-2 in bf16) and of
tests/test_gpu_frozen.py (one Adam step moves an element by at most lr)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from model_compare import assert_outputs_and_losses_match_oracle, rel
from oracle import misa_oracle as orc

DEV = "cuda:0"
LR, CLIP = 1e-3, 1.0
RNN = ("trnn1", "trnn2", "vrnn1", "vrnn2", "arnn1", "arnn2")
LNS = ("tlayer_norm", "vlayer_norm", "alayer_norm")
CUT = RNN + LNS + ("embed",)
N = 21


class ListLoader:
    def __init__(self, batches):
        self.batches = batches
        self.dataset = self

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


def _model(precision="fp32", freeze=True, **kw):
    from mmda_amd import make_config, MISA
    cfg = orc.default_config(vocab_size=120, **kw)
    m = MISA(make_config(precision=precision, device=DEV, **vars(cfg)))
    m.load_state_dict(orc.synth_params(cfg, 21))
    m.to(DEV)
    m._materialize(torch.device(DEV))
    if freeze:
        m.freeze(*CUT)
    return m, cfg


def _samples_of(b):
    """The columns of an ``orc.synth_batch`` as reference-style samples: sample i is column i cut to its length"""
    out = []
    for i, L in enumerate(b["l"].tolist()):
        lab = np.concatenate([[0.0], b["emo"][i].numpy()]).astype(np.float32)[None]
        out.append(((b["t"][:L, i].numpy(), b["v"][:L, i].numpy(), b["a"][:L, i].numpy(), ["w"] * L), lab, f"seg{i}"))
    return out


def _dataset_of(b):
    from mmda_amd import DeviceDataset
    return DeviceDataset.from_samples(_samples_of(b), DEV)


def _cut_step(m, b, **kw):
    kw.setdefault("training", True)
    m.train_step(b["t"].to(DEV), b["v"].to(DEV), b["a"].to(DEV), b["l"], b["emo"].to(DEV), lr=LR, clip=CLIP, **kw)


def _encoded_batch(m, b):
    """The one batch of an EncodedLoader over a cache built from exactly the batch ``b`` (its columns in their order)"""
    from mmda_amd import EncodedLoader, EncoderCache
    B = b["t"].shape[1]
    cache = EncoderCache.build(m, _dataset_of(b), B, order="dataset")
    (eb,) = list(EncodedLoader(cache, B))
    assert eb.rows.tolist() == list(range(B)) and eb.B == B
    return eb


def _state(m):
    P, _, M, V = m.flat_buckets()
    torch.cuda.synchronize()
    return [x.detach().cpu().clone() for x in (P, M, V)]


def _ranges(m, frozen):
    names = m._native_names
    offs = [m._layout[n][0] for n in names] + [m._flat_floats]
    return [(n, offs[i], offs[i + 1]) for i, n in enumerate(names) if m._get(n).requires_grad != frozen]


def _assert_same_step(a, e, before, B, what):
    """model ``a`` took the cut step, ``e`` the encoded one, both from ``before``"""
    sa, se = _state(a), _state(e)
    tr, fr = _ranges(e, False), _ranges(e, True)
    assert tr and fr
    for name, b0, e0 in tr:
        for tag, x, y in zip("PMV", se, sa):
            assert torch.equal(x[b0:e0], y[b0:e0]), (what, name, tag, float((x[b0:e0] - y[b0:e0]).abs().max()))
    for name, b0, e0 in fr:
        for tag, x, y in zip("PMV", se, before):
            assert torch.equal(x[b0:e0], y[b0:e0]), (what, name, tag, "frozen")
    assert torch.equal(e._ws_view("losses", (8,)).cpu(), a._ws_view("losses", (8,)).cpu()), (what, e.read_losses(), a.read_losses())
    nc = e.config.num_classes
    assert torch.equal(e._ws_view("scores", (B, nc)).cpu(), a._ws_view("scores", (B, nc)).cpu()), (what, "scores")
    assert not torch.equal(se[0], before[0]), (what, "nothing moved")
    return se


# ------------------------------------------------------------------------------------------------ 1: the two row movers
def _tables(n, widths, offset, gen):
    """tables of n rows with a canary row in front of and behind each; ``offset``: the table's base lies that many floats off 16 bytes"""
    out = []
    for w in widths:
        buf = torch.empty((n + 2) * w + 8, device=DEV)
        buf.copy_(torch.randn(buf.shape, generator=gen))
        assert buf.data_ptr() % 16 == 0
        out.append((buf, buf[offset + w:offset + w + n * w].view(n, w)))
    return out


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("B", [1, 5, 67])
@pytest.mark.parametrize("widths", [(1200, 140, 296), (20, 12, 7)])
def test_gather_and_collect_equal_torch_indexing(widths, B, offset):
    """(20, 12, 7): 7 is a 4-byte-lane row; offset 1: a 16-byte-lane width on a base that is not 16-byte aligned.  67 columns: 17
    workgroups, the last with one live wave."""
    from mmda_amd import _lib
    lib = _lib.load()
    gen = torch.Generator().manual_seed(B * 10 + offset)
    n = 80
    tabs = _tables(n, widths + (6,), offset, gen)
    rows = torch.randint(0, n, (B,), generator=gen).to(torch.int32)
    if B > 1:
        rows[-1] = rows[0]                                           # a repeated row: the gather only reads the tables
    rows_dev = rows.to(DEV)
    outs = _tables(B, widths + (6,), 0, gen)
    before = [buf.clone() for buf, _ in outs]
    s = _lib.stream_ptr()
    _lib.check(lib.mmda_encoded_gather(*(t.data_ptr() for _, t in tabs[:3]), *widths, tabs[3][1].data_ptr(), 6, rows_dev.data_ptr(), B,
                                       *(o.data_ptr() for _, o in outs[:3]), outs[3][1].data_ptr(), s), "gather")
    for (tbuf, t), (obuf, o), b0, w in zip(tabs, outs, before, widths + (6,)):
        assert torch.equal(o, t.index_select(0, rows_dev.long())), w
        assert torch.equal(obuf[:w], b0[:w]) and torch.equal(obuf[w + B * w:], b0[w + B * w:]), (w, "canary")
    # without the labels: three segments, the label output untouched
    keep = outs[3][0].clone()
    outs[0][1].zero_()
    _lib.check(lib.mmda_encoded_gather(*(t.data_ptr() for _, t in tabs[:3]), *widths, None, 6, rows_dev.data_ptr(), B,
                                       *(o.data_ptr() for _, o in outs[:3]), None, s), "gather")
    assert torch.equal(outs[0][1], tabs[0][1].index_select(0, rows_dev.long())) and torch.equal(outs[3][0], keep)

    # collect: a permuted dst, then dst = NULL with base = 3
    src = [o.clone() for _, o in outs[:3]]
    dst = torch.randperm(n, generator=gen)[:B].to(torch.int32)
    for dst_dev, base, at in ((dst.to(DEV), 0, dst.long()), (None, 3, torch.arange(3, 3 + B))):
        want = []
        for tbuf, t in tabs[:3]:
            tbuf.copy_(torch.randn(tbuf.shape, generator=gen))
            want.append(tbuf.clone())
        _lib.check(lib.mmda_encoded_collect(*(x.data_ptr() for x in src), *widths, *(t.data_ptr() for _, t in tabs[:3]),
                                            None if dst_dev is None else dst_dev.data_ptr(), base, B, s), "collect")
        for x, (tbuf, t), full, w in zip(src, tabs[:3], want, widths):
            ref = full[offset + w:offset + w + n * w].view(n, w)    # (a view of the copy: the indexed assignment lands in `full`)
            ref[at.to(DEV)] = x
            assert torch.equal(tbuf, full), (w, base)                # the rows, and nothing but the rows: canaries included


# ------------------------------------------------------------------------------------------------ 2: the cache is the workspace
def make_samples(lengths, dv, da, seed=0):
    """Reference-style samples (as tests/test_gpu_inference.py makes them); every sample has a class at a positive score and any eight
    consecutive samples hold every class, so a training step's losses stay finite."""
    rng = np.random.default_rng(seed)
    out = []
    for i, L in enumerate(lengths):
        lab = rng.normal(size=(1, 7)).astype(np.float32)
        lab[0, 1 + i % 6] = 1.0
        lab[0, 1 + (i + 3) % 6] = 0.5
        out.append(((rng.integers(2, 50, size=L), rng.normal(size=(L, dv)).astype(np.float32),
                     rng.normal(size=(L, da)).astype(np.float32), ["w"] * L), lab, f"seg{i}"))
    return out


@pytest.fixture(scope="module")
def corpus():
    from mmda_amd import DeviceDataset
    lengths = np.random.default_rng(8).integers(1, 13, size=N)
    lengths[0], lengths[1] = 12, 1
    samples = make_samples(lengths, 35, 74, seed=2)
    return samples, DeviceDataset.from_samples(samples, DEV)


@pytest.fixture(scope="module")
def oracle_utt(corpus):
    """orc.encode_modality over the 21 samples as one padded batch, rows put back at their sample index; computed once, never written"""
    from mmda_amd.data import collate_fn
    samples, _ = corpus
    cfg = orc.default_config(vocab_size=120)
    P = orc.synth_params(cfg, 21)
    t, v, a, _, _, l, _, _, _, ids = collate_fn(list(samples))
    at = torch.tensor([int(s[3:]) for s in ids])
    out = {}
    with torch.no_grad():
        for m, x, d in (("t", P["embed.weight"][t], cfg.embedding_size), ("v", v, cfg.visual_size), ("a", a, cfg.acoustic_size)):
            u = orc.encode_modality(x, l.cpu(), P, m, d)
            out[m] = torch.empty_like(u)
            out[m][at] = u
    return out


@pytest.mark.parametrize("order", ["length", "dataset"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_cache_rows_are_the_workspace_rows_of_an_evaluation_forward(corpus, oracle_utt, precision, order):
    from mmda_amd import DeviceLoader, EncoderCache, inference_plan
    samples, ds = corpus
    m, cfg = _model(precision, freeze=False)
    m.eval()
    seed0 = m._seed
    cache = EncoderCache.build(m, ds, 8, order)
    assert len(cache) == N and cache.widths == (1200, 140, 296) and cache.utt_t.shape == (N, 1200)
    assert all(getattr(cache, f"utt_{k}").data_ptr() % 16 == 0 for k in "tva")
    assert torch.equal(cache.emo, ds.emo) and cache.lengths.tolist() == list(ds.lengths) and list(cache.segments) == list(ds.segments)
    plan, bounds = inference_plan(ds.lengths, 8, order)
    n_batches = len(bounds) - 1
    for _ in range(n_batches):                                        # one seed per batch, as one model(...) call per batch draws
        seed0 = (seed0 * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
    assert m._seed == seed0
    seen = 0
    for batch in DeviceLoader(ds, 8, sampler=plan.tolist()):          # the plan's own batches (batch_plan sorts them the same way)
        with torch.no_grad():
            m(batch[0], batch[1], batch[2], batch[5])
        at = torch.tensor([int(s[3:]) for s in batch[9]], device=DEV)
        B = len(batch[9])
        for k, w in zip("tva", cache.widths):
            assert torch.equal(getattr(cache, f"utt_{k}")[at], m._ws_view(f"utt_{k}", (B, w))), (k, seen)
        seen += B
    assert seen == N
    tol = 1e-4 if precision == "fp32" else 1e-2
    for k in "tva":
        assert rel(getattr(cache, f"utt_{k}"), oracle_utt[k]) < tol, k
    from mmda_amd.encoded import encoder_ranges
    bits = m._P.view(torch.int32)
    assert cache.fingerprint == sum(int(bits[b:e].sum(dtype=torch.int64)) for b, e in encoder_ranges(m))
    cache.check(m)
    assert not m.cluster_aborted()


# ------------------------------------------------------------------------------------------------ 3: bit equality with the cut step
def _bits(precision, shapes, rmsprop=False, **kw):
    """Two models from one state under the cut: ``a`` takes train_step, ``e`` train_step_encoded over a cache of exactly that batch,
    same seed, dropout on; one warm step each first (a (B, T) step: M and V are non-zero, and ``e``'s workspace is re-carved)."""
    from mmda_amd import optim
    a, cfg = _model(precision, **kw)
    e, _ = _model(precision, **kw)
    opt = {}
    if rmsprop:
        for k, m in (("a", a), ("e", e)):
            opt[k] = optim.RMSprop([p for p in m.parameters() if p.requires_grad], lr=1e-2)
            opt[k].attach(m)
    warm = orc.synth_batch(cfg, 8, 12, 60, ragged=True)
    for k, m in (("a", a), ("e", e)):
        _cut_step(m, warm, seed=900, optimizer=opt.get(k))
    assert a.trainable_info()[2] and e.trainable_info()[2]
    for i, (B, T) in enumerate(shapes):
        b = orc.synth_batch(cfg, B, T, 70 + i, ragged=True)
        before = _state(e)
        for x, y in zip(before, _state(a)):
            assert torch.equal(x, y)
        eb = _encoded_batch(e, b)
        _cut_step(a, b, seed=1000 + i, optimizer=opt.get("a"))
        e.train_step_encoded(eb, lr=LR, clip=CLIP, seed=1000 + i, optimizer=opt.get("e"))
        assert e._ws_shape == (B, 1)
        _assert_same_step(a, e, before, B, (precision, i, B, T))
        if rmsprop:
            assert torch.equal(opt["a"]._square_avg(a.flat_buckets()[0]).cpu(), opt["e"]._square_avg(e.flat_buckets()[0]).cpu())
    assert a._step == e._step
    assert not a.cluster_aborted() and not e.cluster_aborted()
    return a, e


@pytest.mark.parametrize("confid", [False, True])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_three_encoded_steps_equal_three_cut_steps_bit_for_bit(precision, confid):
    _bits(precision, [(8, 12), (6, 9), (8, 12)], use_confidNet=confid)


def test_encoded_steps_equal_cut_steps_with_gru_encoders():
    _bits("bf16", [(8, 12), (6, 9)], rnncell="gru")


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_encoded_steps_equal_cut_steps_with_rmsprop_behind_do_adam_false(precision):
    a, e = _bits(precision, [(8, 12), (6, 9)], rmsprop=True)
    assert a._step == e._step


# ------------------------------------------------------------------------------------------------ 4: the other forms of the fusion block
def test_stand_alone_skinny_launches():
    _bits("fp32", [(8, 12)], hidden_size=64)                         # hidden != 128: no fused row-local stretches


def test_tiled_fusion_block():
    _bits("fp32", [(260, 3)])                                        # B > SKINNY_MAX_B = 256


# ------------------------------------------------------------------------------------------------ 5: against the oracle
def test_three_fp32_steps_from_a_cache_match_the_oracle_behind_the_encoders():
    """The cache is built at batch_size = 4 and trained at B = 8 (the encoders saw other batches than the step would have).  Oracle:
    orc.encode_modality once (frozen encoders), then per step orc.fusion_from_utterances + the losses, gradients None for the frozen
    names, orc.AdamState.  Per step: scores, tcp and the six losses within 1e-4, the parameters by the criteria of
    tests/test_gpu_frozen.py::test_model_fp32_three_steps_match_the_oracle_with_none_gradients."""
    from mmda_amd import EncodedLoader, EncoderCache
    m, cfg = _model("fp32")
    frozen = set(m.frozen_names())
    b = orc.synth_batch(cfg, 8, 12, 33, ragged=True)
    cache = EncoderCache.build(m, _dataset_of(b), 4)
    loader = EncodedLoader(cache, 8, shuffle=True, generator=torch.Generator().manual_seed(4))
    P = orc.synth_params(cfg, 21)
    P0 = {k: v.clone() for k, v in P.items()}
    with torch.no_grad():
        utt = {"t": orc.encode_modality(P["embed.weight"][b["t"]], b["l"], P, "t", cfg.embedding_size),
               "v": orc.encode_modality(b["v"], b["l"], P, "v", cfg.visual_size),
               "a": orc.encode_modality(b["a"], b["l"], P, "a", cfg.acoustic_size)}
    opt = orc.AdamState(P, LR)
    for i in range(3):
        (eb,) = list(loader)
        rows = eb.rows.cpu().long()
        assert sorted(rows.tolist()) == list(range(8))
        m.train_step_encoded(eb, lr=LR, clip=CLIP, training=False)
        leaves = {k: p.detach().clone().requires_grad_(True) for k, p in P.items()}
        o = orc.fusion_from_utterances(leaves, cfg, {k: u[rows] for k, u in utt.items()})
        L = orc.all_losses(o, b["emo"][rows], cfg)
        L.total.backward()
        G = {k: (None if p.grad is None or k in frozen else p.grad.detach().clamp(-CLIP, CLIP)) for k, p in leaves.items()}
        opt.step(P, G)
        torch.cuda.synchronize()
        assert_outputs_and_losses_match_oracle(m._ws_view("scores", (8, 6)), m._ws_view("tcp", (8, 6)), m.read_losses(), o, L, 1e-4)
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
            assert d.max() <= 2 * LR + 1e-7, (i, k)                 # one Adam step moves an element by at most lr
            assert (d <= 0.02 * LR).mean() >= 0.99, (i, k, float((d <= 0.02 * LR).mean()))
    assert m._step == 3 and not m.cluster_aborted()


# ------------------------------------------------------------------------------------------------ 6: Solver
def _solver(train, dev, n_epoch=2):
    from mmda_amd import make_config, models
    from mmda_amd.solver import Solver
    cfg = orc.default_config(vocab_size=120, learning_rate=LR, clip=CLIP)
    c = make_config(precision="fp32", device=DEV, n_epoch=n_epoch, name="encoded", **vars(cfg))
    m = models.MISA(c)
    m.load_state_dict(orc.synth_params(cfg, 21))
    m.freeze(*CUT)
    torch.manual_seed(0)
    return Solver(c, c, c, train, dev, ListLoader([]), is_train=True, model=m).build()


def test_solver_trains_and_evaluates_from_the_cache(corpus, tmp_path, monkeypatch):
    """Two epochs of train() over encoded train and dev loaders against the same Solver over DeviceLoaders under the cut, the same
    sampler seed.  The cache is built in length order, the DeviceLoader's batches are shuffled ones: the encoders saw other batches, so
    the comparison is the fp32 bound, not bits -- 12 Adam steps move an element by at most 12 lr, and 99 % of the elements agree within
    2 % of that."""
    from mmda_amd import DeviceLoader, EncodedLoader, EncoderCache
    monkeypatch.chdir(tmp_path)
    samples, ds = corpus
    gen = lambda: torch.Generator().manual_seed(5)
    ref = _solver(DeviceLoader(ds, 8, shuffle=True, generator=gen()), DeviceLoader(ds, 8))
    enc = _solver(DeviceLoader(ds, 8, shuffle=True, generator=gen()), DeviceLoader(ds, 8))
    cache = enc.encode("dev")
    direct = EncoderCache.build(enc.model, ds, 8)
    for k in "tva":
        assert torch.equal(getattr(cache, f"utt_{k}"), getattr(direct, f"utt_{k}")), k
    assert cache.fingerprint == direct.fingerprint
    # evaluation from the cache against evaluation from the DeviceLoader, before any training
    want = enc.eval("dev")
    enc.dev_data_loader = EncodedLoader(cache, 8)
    got = enc.eval("dev")
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])          # predicted labels, truths
    assert abs(got[0] - want[0]) <= 1e-4 * abs(want[0]) and got[1] == want[1]
    enc.train_data_loader = EncodedLoader(cache, 8, shuffle=True, generator=gen())
    from mmda_amd import _lib
    with pytest.raises(_lib.MMDAError, match="EncodedLoader"):
        enc.train_epoch_unfused()
    hist = {}
    for name, s in (("ref", ref), ("enc", enc)):
        s.model._seed = 0x5EED                                       # (the evaluation passes above drew seeds)
        hist[name] = s.train()
        torch.cuda.synchronize()
    assert ref.model._step == enc.model._step == 6
    steps = 6
    for (n0, b0, e0) in _ranges(enc.model, False):
        x, y = enc.model._P[b0:e0].cpu().numpy(), ref.model._P[b0:e0].cpu().numpy()
        if n0.endswith("self_attn.in_proj_bias"):
            continue
        d = np.abs(x - y)
        assert d.max() <= 2 * LR * steps + 1e-7, n0
        assert (d <= 0.02 * LR * steps).mean() >= 0.99, (n0, float((d <= 0.02 * LR * steps).mean()))
    for he, hr in zip(hist["enc"], hist["ref"]):
        assert abs(he["valid_loss"] - hr["valid_loss"]) <= 1e-4 * abs(hr["valid_loss"]), (he, hr)
        assert abs(he["valid_acc"] - hr["valid_acc"]) <= 1e-4, (he, hr)
    assert not enc.model.cluster_aborted() and not ref.model.cluster_aborted()


# ------------------------------------------------------------------------------------------------ 7: no hidden waits
def test_a_warm_encoded_epoch_does_not_synchronise(corpus):
    """The epoch's steps, its upload of the order and the enqueued fingerprint run with torch's synchronisation check armed; the epoch's
    one read-back -- the fingerprint's, behind the last batch -- comes after the check is switched off."""
    from mmda_amd import EncodedLoader, EncoderCache
    samples, ds = corpus
    m, cfg = _model("bf16")
    cache = EncoderCache.build(m, ds, 8)
    loader = EncodedLoader(cache, 8, shuffle=True, generator=torch.Generator().manual_seed(9))
    m.train()

    def epoch(it, sums=None):
        for _ in range(len(loader)):
            m.train_step_encoded(next(it), lr=LR, clip=CLIP)
            L = m._ws_view("losses", (8,))
            sums = L.clone() if sums is None else sums + L
        return sums

    it = iter(loader)
    epoch(it)
    assert next(it, None) is None                                    # warm: allocator blocks, side stream, run table
    probe = torch.ones(1, device=DEV)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()                                             # the check is live in this build
        it = iter(loader)
        sums = epoch(it)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert next(it, None) is None                                    # the fingerprint's read-back: the cache is current
    assert all(np.isfinite(sums.tolist())) and m._step == 2 * len(loader) and not m.cluster_aborted()


# ------------------------------------------------------------------------------------------------ 8: staleness and refusals
def test_refusals_leave_a_usable_model_and_a_stale_cache_is_named():
    from mmda_amd import _lib, EncodedLoader, EncoderCache
    m, cfg = _model("fp32")
    twin, _ = _model("fp32")
    b = orc.synth_batch(cfg, 8, 12, 44, ragged=True)
    cache = EncoderCache.build(m, _dataset_of(b), 8, order="dataset")
    loader = EncodedLoader(cache, 8)
    (eb,) = list(loader)
    m._seed = twin._seed
    m.unfreeze("trnn1")
    with pytest.raises(_lib.MMDAError, match="trnn1.weight_ih_l0"):
        m.train_step_encoded(eb, lr=LR, clip=CLIP)
    with pytest.raises(_lib.MMDAError, match="encoder cut"):
        with torch.no_grad():
            m.forward_encoded(eb)
    assert m._step == 0 and m._seed == twin._seed
    # ... and so does the native entry point, handed a good batch and a workspace carved for it: MMDA_EINVAL, nothing launched
    import ctypes
    m._carve(8, 1, torch.device(DEV))
    nb = _lib.EncodedBatch(tab_t=cache.utt_t.data_ptr(), tab_v=cache.utt_v.data_ptr(), tab_a=cache.utt_a.data_ptr(),
                           tab_emo=cache.emo.data_ptr(), rows=eb.rows_ptr, B=8)
    emo_out = torch.full((8, 6), -1.0, device=DEV)
    P0 = _state(m)
    assert m._lib.mmda_misa_train_step_encoded(m._h, ctypes.byref(nb), emo_out.data_ptr(), 1, 7, 1, LR, CLIP, 1, _lib.stream_ptr()) == -1
    nb.B = 6                                                         # (under the cut, but not the B of the carve)
    m.freeze("trnn1"); m._sync_trainable()
    assert m._lib.mmda_misa_train_step_encoded(m._h, ctypes.byref(nb), emo_out.data_ptr(), 1, 7, 1, LR, CLIP, 1, _lib.stream_ptr()) == -1
    m.unfreeze("trnn1")
    assert bool((emo_out == -1.0).all()) and all(torch.equal(x, y) for x, y in zip(_state(m), P0))
    twin.unfreeze("trnn1")
    _cut_step(m, b); _cut_step(twin, b)                              # ... and an ordinary step works
    for x, y in zip(_state(m), _state(twin)):
        assert torch.equal(x, y)
    # that step trained trnn1: the cache is stale, and the next epoch says so
    m.freeze("trnn1")
    with pytest.raises(_lib.MMDAError, match="stale"):
        cache.check(m)
    with pytest.raises(_lib.MMDAError, match="stale"):
        for eb2 in loader:
            m.train_step_encoded(eb2, lr=LR, clip=CLIP)
    # a write from outside
    fresh, _ = _model("fp32")
    c2 = EncoderCache.build(fresh, _dataset_of(b), 8)
    c2.check(fresh)
    with torch.no_grad():
        fresh.trnn1.weight_ih_l0[3, 5] += 0.5
    with pytest.raises(_lib.MMDAError, match="stale"):
        list(EncodedLoader(c2, 8))
    # the other refusals, each before any launch
    ok, _ = _model("fp32")
    c3 = EncoderCache.build(ok, _dataset_of(b), 8)
    (e3,) = list(EncodedLoader(c3, 8))
    step0, seed0 = ok._step, ok._seed
    with pytest.raises(_lib.MMDAError, match="gradient exchange"):
        ok.train_step_encoded(e3, lr=LR, clip=CLIP, grad_sync=lambda g, n: 1.0)
    for kw in (dict(accum_index=1, accum_count=2), dict(accum_count=2)):
        with pytest.raises(_lib.MMDAError, match="not built"):
            ok.train_step_encoded(e3, lr=LR, clip=CLIP, **kw)
    with pytest.raises(_lib.MMDAError, match="autograd"):
        ok.forward_encoded(e3)
    small, _ = _model("fp32", visual_size=20)
    with pytest.raises(_lib.MMDAError, match="wide"):
        small.train_step_encoded(e3, lr=LR, clip=CLIP)
    assert ok._step == step0 and ok._seed == seed0
    ok.train_step_encoded(e3, lr=LR, clip=CLIP)
    assert ok._step == step0 + 1 and not ok.cluster_aborted()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_steps_of_both_kinds_in_one_process(precision):
    """(B, T) step, encoded step, (B, T) step against the same three steps with the middle one done as a cut step: the workspace is
    re-carved (8, 12) -> (8, 1) -> (6, 9), and what a step leaves behind for the next (K-major weight copies, side-stream flags) is
    consumed across the two kinds."""
    a, cfg = _model(precision)
    e, _ = _model(precision)
    bs = [orc.synth_batch(cfg, B, T, 20 + i, ragged=True) for i, (B, T) in enumerate([(8, 12), (8, 12), (6, 9)])]
    before = _state(e)
    _cut_step(a, bs[0], seed=1); _cut_step(e, bs[0], seed=1)
    eb = _encoded_batch(e, bs[1])
    _cut_step(a, bs[1], seed=2)
    e.train_step_encoded(eb, lr=LR, clip=CLIP, seed=2)
    _cut_step(a, bs[2], seed=3); _cut_step(e, bs[2], seed=3)
    _assert_same_step(a, e, before, 6, precision)
    # forward_encoded: the scores of model(...) on the same batch, the side-channel attributes set
    a.eval(); e.eval()
    eb = _encoded_batch(e, bs[1])
    with torch.no_grad():
        want = a(bs[1]["t"].to(DEV), bs[1]["v"].to(DEV), bs[1]["a"].to(DEV), bs[1]["l"])
        got = e.forward_encoded(eb)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert torch.equal(e.utt_shared_a, a.utt_shared_a) and torch.equal(e.tcp, a.tcp) and e.domain_label_t is None
    assert torch.equal(eb.emo(), bs[1]["emo"].to(DEV))
    assert not a.cluster_aborted() and not e.cluster_aborted()
