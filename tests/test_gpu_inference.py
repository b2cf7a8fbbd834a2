"""GPU: the inference pass -- ``mmda_infer_collect`` (one launch per batch), ``InferencePass.run`` / ``run_loader``, ``Solver.infer`` and
the ``utils.tools`` files -- against torch indexing of the same sources, against ``model(...)`` on the same batches (bit for bit: the
pass only copies what that forward computes) and against the fp32 oracle (``hidden`` and ``attention``, which ``model(...)`` does not
expose).  Tolerances are those of tests/test_gpu_model.py: max error relative to the tensor's max magnitude, 1e-4 in fp32, 1e-2 in bf16."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from model_compare import rel
from oracle import misa_oracle as orc

DEV = "cuda:0"
MOSEI = (35, 74)
N = 21
ALL = ("scores", "labels", "tcp", "hidden", "utterance", "attention")


def make_samples(lengths, dv, da, seed=0):
    """Reference-style samples (as tests/test_gpu_device_loader.py makes them); every sample has a class at a positive score and any
    eight consecutive samples hold every class, so a training step's losses stay finite."""
    rng = np.random.default_rng(seed)
    out = []
    for i, L in enumerate(lengths):
        lab = rng.normal(size=(1, 7)).astype(np.float32)
        lab[0, 1 + i % 6] = 1.0
        lab[0, 1 + (i + 3) % 6] = 0.5
        out.append(((rng.integers(2, 50, size=L), rng.normal(size=(L, dv)).astype(np.float32),
                     rng.normal(size=(L, da)).astype(np.float32), ["w"] * L), lab, f"seg{i}"))
    return out


class ListLoader:
    def __init__(self, batches):
        self.batches = batches
        self.dataset = self

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


@pytest.fixture(scope="module")
def corpus():
    from mmda_amd import DeviceDataset
    lengths = np.random.default_rng(8).integers(1, 10, size=N)
    samples = make_samples(lengths, *MOSEI, seed=2)
    return samples, DeviceDataset.from_samples(samples, DEV)


def _cfg():
    return orc.default_config(vocab_size=120)


def _model(precision):
    from mmda_amd import MISA, make_config
    cfg = _cfg()
    m = MISA(make_config(precision=precision, device=DEV, **vars(cfg)))
    m.load_state_dict(orc.synth_params(cfg, 21))
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def model_fp32():
    return _model("fp32")


@pytest.fixture(scope="module")
def model_bf16():
    return _model("bf16")


@pytest.fixture
def model(request, model_fp32, model_bf16):
    return model_fp32 if request.param == "fp32" else model_bf16


both = pytest.mark.parametrize("model", ["fp32", "bf16"], indirect=True)


@pytest.fixture(scope="module")
def oracle(corpus):
    """The fp32 oracle over the 21 samples as ONE padded batch, rows put back at their sample index (evaluation outputs do not depend on
    the batch a sample sits in); computed once and never written.  ``attention``: the head average of the softmax of
    ``oracle.misa_oracle.fusion_layer``, restated on the oracle's own six utterance vectors."""
    from mmda_amd.data import collate_fn
    samples, _ = corpus
    cfg, P = _cfg(), orc.synth_params(_cfg(), 21)
    t, v, a, _, _, l, _, _, _, ids = collate_fn(list(samples))
    with torch.no_grad():
        o = orc.forward(P, cfg, t, v, a, l)
        x = torch.stack((o.utt_private_t, o.utt_private_v, o.utt_private_a, o.utt_shared_t, o.utt_shared_v, o.utt_shared_a), dim=0)
        te = "transformer_encoder.layers.0."
        S, B, E = x.shape
        hd = E // orc.NHEAD
        qkv = x @ P[te + "self_attn.in_proj_weight"].t() + P[te + "self_attn.in_proj_bias"]
        q, k, _ = qkv.split(E, dim=-1)
        heads = lambda z: z.reshape(S, B, orc.NHEAD, hd).permute(1, 2, 0, 3)
        att = torch.softmax((heads(q) @ heads(k).transpose(-1, -2)) / math.sqrt(hd), dim=-1)        # (B, NHEAD, 6, 6)
        fields = dict(scores=o.scores, tcp=o.tcp, hidden=o.h, utterance=x.permute(1, 0, 2), attention=att.sum(1) / orc.NHEAD)
    at = torch.tensor([int(s[3:]) for s in ids])                       # batch row -> sample index
    out = {}
    for k_, val in fields.items():
        tab = torch.empty_like(val)
        tab[at] = val
        out[k_] = tab
    return out


def _forward_fields(model, batch):
    """What ``model(...)`` returns and sets for one batch, under no_grad: scores, labels, tcp and the six utterance vectors."""
    with torch.no_grad():
        scores, labels = model(batch[0], batch[1], batch[2], batch[5])
    utt = torch.stack([model.utt_private_t, model.utt_private_v, model.utt_private_a, model.utt_shared_t, model.utt_shared_v,
                       model.utt_shared_a], dim=1)
    return dict(scores=scores, labels=labels, tcp=model.tcp.clone(), utterance=utt)


def _same_result(a, b):
    """every table of two results, bit for bit (the flat buffer under them has uninitialised padding between tables)"""
    a, b = a.cpu(), b.cpu()
    assert a.fields == b.fields and len(a) == len(b)
    for f in a.fields:
        assert torch.equal(a[f], b[f]) and not bool(torch.isnan(a[f]).any()), f


# ------------------------------------------------------------------------------------------------ 1: the launch, no model
def _sources(B, hs, nhead, C=6, seed=0):
    g = torch.Generator().manual_seed(1000 * B + 10 * hs + nhead + seed)
    src = dict(scores=torch.rand(B, C, generator=g), labels=(torch.rand(B, C, generator=g) > 0.5).float(), tcp=torch.rand(B, 6, generator=g),
               hfused=torch.randn(B, 6 * hs, generator=g), x6=torch.randn(6, B, hs, generator=g),
               probs=torch.softmax(torch.randn(B, nhead, 6, 6, generator=g), dim=-1))
    want = dict(scores=src["scores"], labels=src["labels"], tcp=src["tcp"], hidden=src["hfused"], utterance=src["x6"].permute(1, 0, 2),
                attention=src["probs"].sum(1) / nhead)                  # (heads in head order; exact for one and two heads)
    return {k: v.to(DEV) for k, v in src.items()}, want


def _nan_tables(rows, hs, C=6, fields=ALL):
    shapes = dict(scores=(rows, C), labels=(rows, C), tcp=(rows, 6), hidden=(rows, 6 * hs), utterance=(rows, 6, hs), attention=(rows, 6, 6))
    return {f: torch.full(shapes[f], float("nan"), device=DEV) for f in fields}


def _check_tables(out, want, rows):
    rows = torch.as_tensor(rows)
    for f, tab in out.items():
        got = tab.cpu()
        assert torch.equal(got[rows], want[f].contiguous()), f
        rest = torch.ones(got.shape[0], dtype=torch.bool)
        rest[rows] = False
        assert int(rest.sum()) == 3 and bool(torch.isnan(got[rest]).all()), f          # the launch wrote nothing else


@pytest.mark.parametrize("nhead", [1, 2])
@pytest.mark.parametrize("hs", [128, 6])
@pytest.mark.parametrize("B", [1, 5, 8, 67])
def test_collect_equals_torch_indexing(B, hs, nhead):
    """B = 5, 67: not a multiple of the four columns of a workgroup; 8, 67: more than one workgroup.  hs = 128 takes the 16-byte rows,
    hs = 6 the 4-byte ones (its utterance rows are no whole float4s; its 36-float hidden row is, and sits at 16-byte multiples)."""
    from mmda_amd import ops
    src, want = _sources(B, hs, nhead)
    rng = np.random.default_rng(B + hs)
    dst = rng.permutation(B + 3)[:B]
    if B > 1:
        assert not np.array_equal(dst, np.arange(B))
    else:
        dst = np.array([2])
    out = _nan_tables(B + 3, hs)
    ops.infer_collect(**src, out=out, dst=torch.from_numpy(dst.astype(np.int32)).to(DEV))
    _check_tables(out, want, dst)


@pytest.mark.parametrize("hs", [128, 6])
def test_collect_by_base_and_with_tables_left_out(hs):
    from mmda_amd import ops
    B = 5
    src, want = _sources(B, hs, 2, seed=1)
    out = _nan_tables(B + 3, hs)
    ops.infer_collect(**src, out=out, base=2)                           # dst = NULL: rows base .. base + B - 1
    _check_tables(out, want, np.arange(2, 2 + B))
    for keep in (("hidden",), ("attention", "labels"), ("utterance", "tcp", "scores")):
        out = _nan_tables(B + 3, hs, fields=keep)                       # the other tables are NULL: skipped
        ops.infer_collect(**src, out=out, base=0)
        _check_tables(out, want, np.arange(B))
    out = _nan_tables(B + 3, hs, fields=("hidden",))                    # ... and so may the sources they would read be
    ops.infer_collect(hfused=src["hfused"], out=out, base=3)
    _check_tables(out, want, np.arange(3, 3 + B))


def test_collect_takes_unaligned_tables_through_the_4_byte_rows():
    """A table that starts 4 bytes off a 16-byte boundary: the wide rows fall back to 4-byte lanes."""
    from mmda_amd import ops
    B, hs = 5, 128
    src, want = _sources(B, hs, 2, seed=2)
    rows = B + 3
    flat_h = torch.full((rows * 6 * hs + 1,), float("nan"), device=DEV)
    flat_u = torch.full((rows * 6 * hs + 1,), float("nan"), device=DEV)
    out = dict(hidden=flat_h[1:].view(rows, 6 * hs), utterance=flat_u[1:].view(rows, 6, hs))
    assert out["hidden"].data_ptr() % 16 == 4
    ops.infer_collect(**src, out=out, base=1)
    _check_tables(out, want, np.arange(1, 1 + B))
    assert bool(torch.isnan(flat_h[0])) and bool(torch.isnan(flat_u[0]))


# ------------------------------------------------------------------------------------------------ 2: run_loader against the forward
@both
@pytest.mark.parametrize("bs", [8, 4])
def test_run_loader_equals_the_forward_of_the_same_batches(corpus, model, bs):
    """Batches of 8, 8, 5 -- or of four, ending on a batch of ONE sample."""
    from mmda_amd import DeviceLoader, InferencePass
    samples, ds = corpus
    batches = list(DeviceLoader(ds, bs))
    assert [b[0].shape[1] for b in batches] == ([8, 8, 5] if bs == 8 else [4] * 5 + [1])
    ref = [_forward_fields(model, b) for b in batches]
    res = InferencePass(model, ALL).run_loader(DeviceLoader(ds, bs))
    assert len(res) == N and res.fields == ALL
    for f in ("scores", "labels", "tcp", "utterance"):
        want = torch.cat([r[f] for r in ref])
        assert res[f].shape == want.shape and torch.equal(res[f], want), f
    assert res.hidden.shape == (N, 768) and res.attention.shape == (N, 6, 6)
    assert list(res.segments) == [s for b in batches for s in b[9]]
    assert torch.equal(res.lengths, torch.cat([b[5] for b in batches]))
    assert not model.cluster_aborted()


@both
def test_run_loader_sizes_its_tables_from_a_counting_pass_over_a_list(corpus, model):
    """A loader without a dataset of its own (a list of tuples, host tensors among them) is counted first."""
    from mmda_amd import DeviceLoader, InferencePass
    samples, ds = corpus
    batches = [tuple(x.cpu() if torch.is_tensor(x) and i < 3 else x for i, x in enumerate(b)) for b in DeviceLoader(ds, 8)][:2]
    want = InferencePass(model, ("scores",)).run_loader(DeviceLoader(ds, 8)).scores[:16]
    for loader in (batches, ListLoader(batches)):
        res = InferencePass(model, ("scores",)).run_loader(loader)
        assert len(res) == 16 and res.tcp is None and torch.equal(res.scores, want)


# ------------------------------------------------------------------------------------------------ 3: run(), row i = sample i
@both
@pytest.mark.parametrize("order", ["length", "dataset"])
def test_run_puts_row_i_at_sample_i(corpus, model, order):
    """The expected tables: the same plan replayed through DeviceLoader(sampler=plan) and model(...), rows placed by torch indexing."""
    from mmda_amd import DeviceLoader, InferencePass, inference_plan
    samples, ds = corpus
    plan, bounds = inference_plan(ds.lengths, 8, order)
    if order == "length":
        assert not np.array_equal(plan, np.arange(N))
    want = {}
    for k, b in enumerate(DeviceLoader(ds, 8, sampler=plan.tolist())):
        idx = torch.from_numpy(plan[bounds[k]:bounds[k + 1]]).to(DEV)
        assert b[9] == [f"seg{i}" for i in idx.tolist()]               # the replay visits the plan's batches
        for f, val in _forward_fields(model, b).items():
            if f not in want:
                want[f] = torch.full((N,) + tuple(val.shape[1:]), float("nan"), device=DEV)
            want[f][idx] = val
    res = InferencePass(model, ALL).run(ds, 8, order=order)
    for f in want:
        assert torch.equal(res[f], want[f]), (order, f)
    assert list(res.segments) == [s[2] for s in samples] and res.lengths.tolist() == ds.lengths.tolist()


# ------------------------------------------------------------------------------------------------ 4: against the oracle
@pytest.mark.parametrize("order", ["length", "dataset"])
def test_fp32_pass_matches_the_oracle(corpus, model_fp32, oracle, order):
    """fp32 bound of tests/test_gpu_model.py: 1e-4 of the tensor's max magnitude.  Labels are not compared here: one score of this corpus
    lies 1.5e-4 from the threshold; the bit comparison with model(...)'s labels above is the label test."""
    from mmda_amd import InferencePass
    res = InferencePass(model_fp32, ALL).run(corpus[1], 8, order=order).cpu()
    for f in ("hidden", "scores", "tcp", "utterance", "attention"):
        e = rel(res[f], oracle[f])
        print(f"fp32 {order} {f}: rel {e:.3e}")
        assert e < 1e-4, (f, e)
    assert bool(((res.labels == 0) | (res.labels == 1)).all())
    assert torch.allclose(res.attention.sum(-1), torch.ones(N, 6), atol=1e-5)


@pytest.mark.parametrize("order", ["length", "dataset"])
def test_bf16_hidden_and_attention_within_1e2_of_the_oracle(corpus, model_bf16, oracle, order):
    """The project's bf16 output bound (1e-2 of the tensor's max magnitude, as tests/test_gpu_model.py applies it) on the two fields
    that only the pass exposes."""
    from mmda_amd import InferencePass
    res = InferencePass(model_bf16, ALL).run(corpus[1], 8, order=order).cpu()
    for f in ("hidden", "attention", "scores", "tcp", "utterance"):
        e = rel(res[f], oracle[f])
        print(f"bf16 {order} {f}: rel {e:.3e}")
        assert e < 1e-2, (f, e)


# ------------------------------------------------------------------------------------------------ 5: dropout and mode
@both
def test_passes_repeat_bit_for_bit_and_ignore_the_training_flag(corpus, model):
    from mmda_amd import InferencePass
    p = InferencePass(model, ALL)
    a = p.run(corpus[1], 8)
    b = p.run(corpus[1], 8)
    _same_result(a, b)
    model.train()
    try:
        c = p.run(corpus[1], 8)                                         # dropout stays off: the pass is an evaluation pass
        assert model.training
        d = p.run_loader(ListLoader([]))                                # (an empty loader: no rows, no launch)
        assert model.training and len(d) == 0 and d.scores.shape == (0, 6)
    finally:
        model.eval()
    _same_result(a, c)
    p.run(corpus[1], 8)
    assert not model.training


# ------------------------------------------------------------------------------------------------ 6: no synchronisation
@both
def test_a_warm_pass_does_not_synchronise(corpus, model):
    from mmda_amd import DeviceLoader, InferencePass
    samples, ds = corpus
    p = InferencePass(model, ALL)
    warm = p.run(ds, 8), p.run_loader(DeviceLoader(ds, 8))
    probe = torch.ones(1, device=DEV)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()                                                 # the check is live in this build
        got = p.run(ds, 8), p.run_loader(DeviceLoader(ds, 8))
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    for w, g in zip(warm, got):
        _same_result(w, g)


# ------------------------------------------------------------------------------------------------ 7: training is undisturbed
def _solver(train, dev, precision):
    from mmda_amd import make_config, models
    from mmda_amd.solver import Solver
    cfg = orc.default_config(vocab_size=120, learning_rate=1e-3, clip=1.0)
    c = make_config(precision=precision, device=DEV, n_epoch=1, name="inference", **vars(cfg))
    m = models.MISA(c)
    m.load_state_dict(orc.synth_params(cfg, 21))
    torch.manual_seed(0)                                             # build() draws the orthogonal recurrent weights
    return Solver(c, c, c, train, dev, ListLoader([]), is_train=True, model=m).build()


def _state(m):
    P, _, M, V = m.flat_buckets()
    torch.cuda.synchronize()
    return [x.detach().cpu().clone() for x in (P, M, V)]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_training_after_a_pass_equals_training_after_as_many_evaluation_forwards(corpus, precision):
    from mmda_amd import DeviceLoader, InferencePass
    samples, ds = corpus
    batches = list(DeviceLoader(ds, 8))
    a, b = _solver(ListLoader([]), ListLoader([]), precision), _solver(ListLoader([]), ListLoader([]), precision)

    def train(s, batch):
        s.model.train()
        s.model.train_step(batch[0], batch[1], batch[2], batch[5], batch[4], lr=1e-3, clip=1.0, optimizer=s.optimizer)

    train(a, batches[0]); train(b, batches[0])
    for x, y in zip(_state(a.model), _state(b.model)):
        assert torch.equal(x, y)                                     # the same state going in
    start = _state(a.model)[0]
    res = InferencePass(a.model).run_loader(DeviceLoader(ds, 8))     # (a) a pass of three batches, the model left in train()
    assert a.model.training and len(res) == N
    b.model.eval()                                                   # (b) three plain evaluation forwards
    for batch in batches:
        _forward_fields(b.model, batch)
    train(a, batches[1]); train(b, batches[1])
    assert a.model._seed == b.model._seed and a.model._step == b.model._step == 2
    for name, x, y in zip("PMV", _state(a.model), _state(b.model)):
        assert torch.equal(x, y), (name, int((x != y).sum()))
    assert not torch.equal(start, _state(a.model)[0]) and not a.model.cluster_aborted()


# ------------------------------------------------------------------------------------------------ 8: Solver.infer and the files
def test_solver_infer_and_the_saved_files(corpus, tmp_path, monkeypatch):
    from mmda_amd import DeviceLoader, InferencePass
    from mmda_amd.utils import tools
    samples, ds = corpus
    s = _solver(ListLoader([]), DeviceLoader(ds, 8), "fp32")
    by_loader = s.infer("dev")                                       # order="loader": the loader's batches, rows as it yields them
    assert by_loader.fields == ("scores", "labels", "tcp", "hidden") and by_loader.attention is None
    at = torch.tensor([int(x[3:]) for x in by_loader.segments], device=DEV)
    assert sorted(at.tolist()) == list(range(N)) and at.tolist() != list(range(N))
    by_dataset = s.infer("dev", order="dataset")                     # the same batches, rows at their sample index
    by_length = s.infer("dev", fields=("hidden", "tcp", "attention"), order="length")
    assert list(by_dataset.segments) == list(by_length.segments) == [x[2] for x in samples]
    for f in by_loader.fields:
        assert torch.equal(by_dataset[f][at], by_loader[f]), f
    direct = InferencePass(s.model, ("hidden", "tcp", "attention")).run(ds, 8, "length")
    assert by_length.scores is None
    _same_result(by_length, direct)
    assert rel(by_length.hidden, by_dataset.hidden) < 2e-4 and rel(by_length.tcp, by_dataset.tcp) < 2e-4   # (each within 1e-4 of the oracle)
    assert s.infer("test").scores.shape == (0, 6)                    # an empty split

    monkeypatch.chdir(tmp_path)
    host = by_length.cpu()
    for confid in (False, True):
        s.train_config.use_confidNet = confid
        tools.save_hidden(s.train_config, by_length.hidden, dataset="dev")          # device tensors are saved as host tensors
        tools.save_tcp(s.train_config, host.tcp, dataset="dev")
        h, tcp = tools.load_hidden(s.train_config, dataset="dev"), tools.load_tcp(s.train_config, dataset="dev")
        assert not h.is_cuda and torch.equal(h, host.hidden) and torch.equal(tcp, host.tcp)
    assert sorted(p.name for p in (tmp_path / "hidden_vectors").iterdir()) == ["MISA_C_dev.pt", "MISA_dev.pt"]

    s.dev_data_loader = ListLoader(list(DeviceLoader(ds, 8)))
    with pytest.raises(ValueError, match="DeviceLoader"):
        s.infer("dev", order="length")
    assert torch.equal(s.infer("dev").scores, by_loader.scores)      # ... which order="loader" takes
