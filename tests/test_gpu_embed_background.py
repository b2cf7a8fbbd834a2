"""GPU: the background pass over the embedding table (MISA.set_embed_background).  In plain dense mode the rows a
batch does not index take their zero-gradient Adam step from a few workgroups on a low-priority stream beside the forward pass, and
the step's closing launch walks only the rows the batch does index.  The oracle is the same step with the pass switched off -- the one
dense launch over the whole table: the same functor on the same operands, so everything is compared BIT for bit (int32 views:
torch.equal on floats would equate +0 and -0), with no tolerance anywhere in this file."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import misa_oracle as orc

DEV = "cuda:0"
LR, CLIP = 1e-3, 1.0


def _model(on, precision="bf16", vocab=512, seed=9, embed_update="dense", **kw):
    from mmda_amd import make_config, MISA
    cfg = orc.default_config(vocab_size=vocab, **kw)            # dropout on (0.1, and the fusion layer's own)
    m = MISA(make_config(precision=precision, device=DEV, embed_update=embed_update, **vars(cfg)))
    m.load_state_dict(orc.synth_params(cfg, seed)); m.to(DEV)
    m.set_embed_background(on)
    return m, cfg


def _step(m, b, lr=LR, **kw):
    m.train_step(b["t"].to(DEV), b["v"].to(DEV), b["a"].to(DEV), b["l"], b["emo"].to(DEV), lr=lr, clip=CLIP, **kw)


def _batches(cfg, shapes, seed=50):
    return [orc.synth_batch(cfg, B, T, seed + i, ragged=True) for i, (B, T) in enumerate(shapes)]


def _ids(b):
    return set(b["t"].flatten().tolist())                         # every position of the (T, B) tensor, padding included


def _bits(x):
    return x.detach().contiguous().view(torch.int32).cpu()


def _assert_same_bits(on, off, what=""):
    torch.cuda.synchronize()
    for name, x, y in zip("PGMV", on.flat_buckets(), off.flat_buckets()):
        bx, by = _bits(x), _bits(y)
        assert torch.equal(bx, by), (what, name, int((bx != by).sum()))
    lx, ly = _bits(on._ws_view("losses", (8,))[:6]), _bits(off._ws_view("losses", (8,))[:6])
    assert torch.equal(lx, ly), (what, "losses", lx.tolist(), ly.tolist())
    on._assign_grad_views(); off._assign_grad_views()
    gx, gy = on.embed.weight.grad, off.embed.weight.grad
    if gx is not None or gy is not None:
        assert torch.equal(_bits(gx), _bits(gy)), (what, "embed.weight.grad")
    assert not on.cluster_aborted() and not off.cluster_aborted()


def _pair(shapes, vocab=512, precision="bf16", step_kw=None, opt=None, active=True, seed=50, **model_kw):
    """The same model, batches, seeds and learning rates with the pass on and off; returns (on, off, batches)."""
    on, cfg = _model(True, precision, vocab, **model_kw)
    off, _ = _model(False, precision, vocab, **model_kw)
    train = _batches(cfg, shapes, seed)
    opts = {id(m): opt(m) for m in (on, off)} if opt else {}
    for i, b in enumerate(train):
        for m in (on, off):
            kw = dict(step_kw or {})
            if opt:
                kw["optimizer"] = opts[id(m)]
            _step(m, b, lr=LR * (1 + 0.25 * i), seed=900 + i, **kw)
            assert m.embed_background_active() == (active and m is on), (i, m is on)
    return on, off, train


def test_one_step_on_equals_one_step_off():
    """The first step with the pass, once, against one without: (B, T, V) = (4, 5, 64)."""
    on, off, _ = _pair([(4, 5)], vocab=64)
    _assert_same_bits(on, off, "first step")


def _opt(cls, **kw):
    def make(m):
        from mmda_amd import optim
        return getattr(optim, cls)([p for p in m.parameters() if p.requires_grad], lr=LR, **kw).attach(m)
    return make


CASES = {
    "most rows indexed": dict(shapes=[(4, 5)] * 3, vocab=64),
    "ragged, padding positions": dict(shapes=[(4, 6)] * 3, vocab=512),
    "bf16": dict(shapes=[(8, 12)] * 3, vocab=2000),
    "fp32: event join": dict(shapes=[(8, 12)] * 3, vocab=2000, precision="fp32"),
    "gru": dict(shapes=[(4, 6)] * 3, vocab=512, rnncell="gru"),
    "sorted list form": dict(shapes=[(64, 48)] * 3, vocab=2000),
    "L2 decay": dict(shapes=[(4, 6)] * 3, vocab=512, opt=_opt("Adam", weight_decay=0.05)),
    "decoupled decay": dict(shapes=[(4, 6)] * 3, vocab=512, opt=_opt("AdamW", weight_decay=0.05)),
    "(B, T) changes between steps": dict(shapes=[(4, 5), (6, 9), (3, 7), (6, 9)], vocab=512),
}


@pytest.mark.parametrize("case", list(CASES))
def test_steps_with_the_pass_equal_steps_without(case):
    kw = dict(CASES[case])
    on, off, train = _pair(kw.pop("shapes"), **kw)
    if kw.get("vocab", 512) >= 512:
        # a row indexed in step 1 and not in step 2 has non-zero moments when the pass steps it: it really moves
        assert _ids(train[0]) - _ids(train[1])
        # ... and padding positions index rows that no valid position does: they are stamped all the same
        b = train[0]
        T = b["t"].shape[0]
        valid = set(b["t"][torch.arange(T).unsqueeze(1) < b["l"].unsqueeze(0)].tolist())
        assert _ids(b) - valid
    _assert_same_bits(on, off, case)
    a, b = on.state_dict(), off.state_dict()
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), (case, k)


def test_an_evaluation_forward_right_behind_a_step_reads_finished_rows():
    """The join: scores over ids the step did not index, issued straight behind the step, equal the off path's bit for bit."""
    on, off, train = _pair([(8, 12)] * 3, vocab=2000)
    cfg = orc.default_config(vocab_size=2000)
    ev = orc.synth_batch(cfg, 8, 12, 777, ragged=True)
    assert _ids(ev) - _ids(train[-1])
    extra = orc.synth_batch(cfg, 8, 12, 51, ragged=True)
    out = []
    for m in (on, off):
        _step(m, extra, seed=77)                                # no synchronisation between the step and the forward
        with torch.no_grad():
            s, _ = m(ev["t"].to(DEV), ev["v"].to(DEV), ev["a"].to(DEV), ev["l"])
        out.append(_bits(s))
    assert on.embed_background_active() and not off.embed_background_active()
    assert torch.equal(out[0], out[1])
    _assert_same_bits(on, off, "after the evaluation forward")


def test_load_state_dict_between_two_steps_is_honoured():
    on, off, train = _pair([(4, 6)] * 2, vocab=512)
    cfg = orc.default_config(vocab_size=512)
    other = orc.synth_params(cfg, 31)
    for m in (on, off):
        m.load_state_dict(other)
        _step(m, train[0], seed=5)
    assert on.embed_background_active() and not off.embed_background_active()
    _assert_same_bits(on, off, "load_state_dict between steps")
    assert not torch.equal(_bits(on.state_dict()["embed.weight"]), _bits(other["embed.weight"]))


def _ineligible(step_kw=None, opt=None, prepare=None, after=None, **model_kw):
    """A configuration in which the pass may not run: switched on all the same, it reports inactive and the steps match the off path."""
    on, cfg = _model(True, **model_kw)
    off, _ = _model(False, **model_kw)
    train = _batches(cfg, [(4, 6)] * 3)
    for m in (on, off):
        if prepare:
            prepare(m)
        o = opt(m) if opt else None
        for i, b in enumerate(train):
            kw = dict(step_kw(i) if callable(step_kw) else (step_kw or {}))
            if o is not None:
                kw["optimizer"] = o
            _step(m, b, seed=300 + i, **kw)
            assert not m.embed_background_active()
            if after:
                after(m, o)
    if model_kw.get("embed_update") == "deferred":
        on.flush_embedding(); off.flush_embedding()
    _assert_same_bits(on, off, str(model_kw))


def test_ineligible_clip_norm():
    _ineligible(step_kw=dict(clip_norm=0.5))


def test_ineligible_accumulated_step():
    _ineligible(step_kw=lambda i: dict(accum_index=i, accum_count=3))


@pytest.mark.parametrize("mode", ["deferred", "sparse", "frozen"])
def test_ineligible_embed_update_modes(mode):
    _ineligible(embed_update=mode)


def test_ineligible_frozen_parameter():
    _ineligible(prepare=lambda m: (m._materialize(torch.device(DEV)), m.freeze("project_v")))


def test_ineligible_gradient_step_then_optimizer_step():
    def after(m, o):
        from mmda_amd import optim
        optim.clip_grad_value_(m, CLIP)
        o.step()
    _ineligible(step_kw=dict(do_adam=False), opt=_opt("Adam"), after=after)


def test_ineligible_gradient_exchange():
    _ineligible(step_kw=dict(grad_sync=lambda g, n: 1.0))


def test_ineligible_step_from_the_encoder_cache():
    from mmda_amd import DeviceDataset, EncodedLoader, EncoderCache
    import numpy as np
    cut = ("trnn1", "trnn2", "vrnn1", "vrnn2", "arnn1", "arnn2", "tlayer_norm", "vlayer_norm", "alayer_norm", "embed")
    on, cfg = _model(True, "fp32", 120)
    off, _ = _model(False, "fp32", 120)
    b = orc.synth_batch(cfg, 4, 6, 11, ragged=True)
    samples = []
    for i, L in enumerate(b["l"].tolist()):
        lab = np.concatenate([[0.0], b["emo"][i].numpy()]).astype(np.float32)[None]
        samples.append(((b["t"][:L, i].numpy(), b["v"][:L, i].numpy(), b["a"][:L, i].numpy(), ["w"] * L), lab, f"seg{i}"))
    for m in (on, off):
        m._materialize(torch.device(DEV))
        m.freeze(*cut)
        cache = EncoderCache.build(m, DeviceDataset.from_samples(samples, DEV), 4, order="dataset")
        (eb,) = list(EncodedLoader(cache, 4))
        for i in range(2):
            m.train_step_encoded(eb, lr=LR, clip=CLIP, seed=40 + i)
            assert not m.embed_background_active()
    _assert_same_bits(on, off, "train_step_encoded")
