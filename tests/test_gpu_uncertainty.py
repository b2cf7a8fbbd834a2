"""GPU: the MC-dropout pass end to end (mmda_amd/uncertainty.py) on the small configuration of tests/uncertainty_cases.py -- default
hidden size, T = 4, ragged, n = 7 -- against the masked oracle: the host restates every mask (oracle/dropout_rng.py), so EVERY DRAW has a
reference, not only the statistics.  The oracle starts from the utterance rows the GPU cached, so encoder error does not enter and the
bound is the dropout-off bound of the fusion block (``tol_out`` = 1e-4 of the tensor's max) in both precisions.
tests/test_uncertainty_cpu.py proves that this comparison can tell a pass that ignores the column index from a correct one, and that
the case's seed keeps every oracle draw away from the decision threshold."""
import contextlib
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import uncertainty_cases as uc
from model_compare import rel

DEV = "cuda:0"
TABLES = ("mean", "var", "entropy", "expected_entropy", "mutual_info", "vote", "tcp_mean", "tcp_var", "draws", "tcp_draws")


@contextlib.contextmanager
def _fusion_dropout(p):
    """mmda_amd.models.FUSION_DROPOUT (read when a model is made) at ``p`` for the block"""
    import mmda_amd.models as mm
    old = mm.FUSION_DROPOUT
    try:
        mm.FUSION_DROPOUT = p
        yield
    finally:
        mm.FUSION_DROPOUT = old


def _model(precision):
    from mmda_amd import MISA, make_config
    with _fusion_dropout(uc.P_TF):
        m = MISA(make_config(precision=precision, device=DEV, **vars(uc.config())))
    m.load_state_dict(uc.params())
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def samples():
    return uc.make_samples()


@pytest.fixture(scope="module")
def dataset(samples):
    from mmda_amd import DeviceDataset
    return DeviceDataset.from_samples(samples, DEV)


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


def _bits(x):
    return x.contiguous().view(torch.int64 if x.dtype == torch.float64 else torch.int32)


def _same(a, b, names=TABLES):
    for k in names:
        x, y = getattr(a, k), getattr(b, k)
        assert (x is None) == (y is None), k
        if x is not None:
            assert torch.equal(_bits(x), _bits(y)), k


def _against_oracle(res, K, model, vote_everywhere):
    """Every draw of ``scores`` and ``tcp`` and every statistic of ``res`` against the masked oracle over the rows the GPU cached."""
    cfg = uc.config()
    n = len(res)
    utt = {m: getattr(res.cache, f"utt_{m}").cpu() for m in "tva"}
    S, Q = uc.oracle_draws(utt, res.chunks, res.seeds, K)
    assert S.shape == (n, K, 6) and res.draws.shape == (n, K, 6) and res.tcp_draws.shape == (n, K, 6)
    e_s, e_q = rel(res.draws, S), rel(res.tcp_draws, Q)
    print(f"K={K}: draws of scores {e_s:.2e}, of tcp {e_q:.2e} (bound {uc.TOL_OUT:.0e})")
    assert e_s < uc.TOL_OUT and e_q < uc.TOL_OUT
    assert bool((res.draws == 0.5).any()) and bool((res.draws != 0.5).any())            # dropped and kept logits
    thr = np.float32(cfg.threshold)
    ref = uc.mc_reference(S.reshape(n * K, 6).numpy(), K, thr)
    bounds = uc.stat_bounds(S)
    for k, bound in bounds.items():
        e = float(np.abs(getattr(res, k).cpu().numpy() - ref[k]).max())
        print(f"  {k}: {e:.2e} (bound {bound:.2e})")
        assert e < bound, (k, e, bound)
    reft = uc.mc_reference(Q.reshape(n * K, 6).numpy(), K, None, bernoulli=False)
    for k in ("mean", "var"):
        e = float(np.abs(getattr(res, "tcp_" + k).cpu().numpy() - reft[k]).max())
        assert e < uc.TOL_OUT, ("tcp_" + k, e)
    # the vote: compared wherever no oracle draw lies within 10 tol_out of the threshold
    near = ((S.double() - float(thr)).abs() < 10 * uc.TOL_OUT).any(dim=1).numpy()
    vote = res.vote.cpu().numpy()
    assert np.array_equal(vote[~near], ref["vote"][~near])
    if vote_everywhere:
        assert int(near.sum()) == 0, "an oracle draw sits on the threshold: choose another MC_SEED (tests/test_uncertainty_cpu.py)"
    # ... and it is exactly the count over the GPU's own draws, everywhere
    # (numpy's count / K is the correctly rounded quotient; a device tensor divided by a scalar may be multiplied by 1 / K instead)
    own = (res.draws.cpu().numpy() > thr).sum(axis=1) / float(K)
    assert np.array_equal(own, vote)


@both
def test_every_draw_and_statistic_against_the_oracle(model, dataset):
    """K = 3, columns = 16: chunks of 5 and of 2 samples under seeds[0] and seeds[1]."""
    from mmda_amd import MCDropoutPass
    from mmda_amd.uncertainty import chunk_seeds
    res = MCDropoutPass(model, passes=uc.K_SMALL, seed=uc.MC_SEED, columns=uc.COLUMNS_SMALL, keep_draws=True).run(dataset, 4)
    assert [c.tolist() for c in res.chunks] == [[0, 1, 2, 3, 4], [5, 6]] and res.seeds == chunk_seeds(uc.MC_SEED, 2)
    assert res.passes == uc.K_SMALL and len(res) == uc.N
    assert all(getattr(res, k).is_cuda for k in TABLES) and res.mean.dtype == torch.float64 and res.draws.dtype == torch.float32
    assert res.lengths.tolist() == [int(x) for x in dataset.lengths] and list(res.segments) == [f"seg{i}" for i in range(uc.N)]
    _against_oracle(res, uc.K_SMALL, model, vote_everywhere=True)
    assert not model.cluster_aborted()


@pytest.mark.parametrize("K,columns,sizes", [(65, 260, [4, 3]), (256, 256, [1] * 7)], ids=["K65-260cols", "K256-1sample"])
def test_the_wide_form_against_the_oracle(model_fp32, dataset, K, columns, sizes):
    """K = 65, four samples per chunk: 260 columns, above SKINNY_MAX_B = 256 -- the tiled GEMMs' mask index.  K = 256 at columns = 256:
    one sample per chunk, seven seeds.  (Thousands of draws: some do sit near the threshold, and only there the vote is left out.)"""
    from mmda_amd import MCDropoutPass
    res = MCDropoutPass(model_fp32, passes=K, seed=uc.MC_SEED + 1, columns=columns, keep_draws=True).run(dataset, 7, order="dataset")
    assert [len(c) for c in res.chunks] == sizes and len(set(res.seeds)) == len(sizes)
    _against_oracle(res, K, model_fp32, vote_everywhere=False)


def test_identities(model_fp32, dataset):
    from mmda_amd import EncoderCache, InferencePass, MCDropoutPass
    m = model_fp32
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    seed_state, training = m._seed, m.training
    p = MCDropoutPass(m, passes=uc.K_SMALL, seed=uc.MC_SEED, columns=uc.COLUMNS_SMALL, keep_draws=True)
    a = p.run(dataset, 2, order="length")
    # the model: its seed sequence, training flag and parameters are what they were
    assert m._seed == seed_state and m.training is training
    after = m.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)
    # the deterministic tables: InferencePass's, bit for bit
    inf = InferencePass(m, ("scores", "labels", "tcp")).run(dataset, 4)
    _same(a, inf, ("scores", "labels", "tcp"))
    m._seed = seed_state
    # batch size and order shape phase A only
    b = p.run(dataset, 7, order="dataset")
    _same(a, b)
    _same(a, b, ("scores", "labels", "tcp"))
    # phase B alone over a cache built separately; and with the deterministic tables handed in
    cache = EncoderCache.build(m, dataset, 4)
    c = p.run_cache(cache)
    _same(a, c)
    _same(a, c, ("scores", "labels", "tcp"))
    d = p.run_cache(cache, deterministic=inf)
    _same(a, d)
    assert d.scores is inf.scores
    m._seed = seed_state
    # two runs; another seed; keep_draws only adds tables
    _same(a, p.run(dataset, 2, order="length"))
    other = MCDropoutPass(m, passes=uc.K_SMALL, seed=uc.MC_SEED + 1, columns=uc.COLUMNS_SMALL, keep_draws=True).run(dataset, 4)
    assert float((other.draws - a.draws).abs().max()) > 100 * uc.TOL_OUT and not torch.equal(other.mean, a.mean)
    _same(a, other, ("scores", "labels", "tcp"))
    plain = MCDropoutPass(m, passes=uc.K_SMALL, seed=uc.MC_SEED, columns=uc.COLUMNS_SMALL).run(dataset, 4)
    assert plain.draws is None and plain.tcp_draws is None
    _same(a, plain, TABLES[:8])
    # mc_statistics over the kept draws is the pass's own reduction
    from mmda_amd import mc_statistics
    st = mc_statistics(a.draws.reshape(uc.N * uc.K_SMALL, 6), uc.K_SMALL, thresholds=uc.config().threshold)
    for k in ("mean", "var", "entropy", "expected_entropy", "mutual_info", "vote"):
        assert torch.equal(_bits(st[k]), _bits(getattr(a, k))), k
    # cpu() / as_dict()
    h = a.cpu()
    assert not h.mean.is_cuda and torch.equal(h.mean, a.mean.cpu()) and h.seeds == a.seeds
    dct = a.as_dict()
    assert dct["passes"] == uc.K_SMALL and np.array_equal(dct["var"], a.var.cpu().numpy()) and dct["draws"].shape == (uc.N, uc.K_SMALL, 6)
    m._seed = seed_state


def test_refusals_on_the_device(model_fp32, dataset):
    from mmda_amd import EncoderCache, MCDropoutPass, MISA, make_config
    from mmda_amd._lib import MMDAError
    p = MCDropoutPass(model_fp32, passes=2, columns=4)
    cpu_model = MISA(make_config(precision="fp32", device="cpu", **vars(uc.config())))
    with pytest.raises(MMDAError, match="MCDropoutPass: the model is on cpu"):
        MCDropoutPass(cpu_model, passes=2).run(dataset, 4)
    cache = EncoderCache.build(model_fp32, dataset, 4)
    narrow = EncoderCache(cache.flat, tuple(w - 4 for w in cache.widths), cache.n, None, cache.lengths, cache.segments, 0)
    with pytest.raises(MMDAError, match="encoder cache: its rows are"):
        p.run_cache(narrow)
    host = EncoderCache(cache.flat.cpu(), cache.widths, cache.n, None, cache.lengths, cache.segments, cache.fingerprint)
    with pytest.raises(MMDAError, match="encoder cache: the cache is on cpu"):
        p.run_cache(host)
    stale = EncoderCache(cache.flat, cache.widths, cache.n, None, cache.lengths, cache.segments, cache.fingerprint + 1)
    with pytest.raises(MMDAError, match="encoder cache is stale"):
        p.run_cache(stale)
    with pytest.raises(TypeError, match="EncoderCache"):
        p.run_cache(dataset)
    # the native entry: the carve's B must be a multiple of K, `which` 0 or 1, tcp without entropy tables
    import ctypes as C
    from mmda_amd import _lib
    m = model_fp32
    rows = torch.arange(6, dtype=torch.int32, device=DEV)
    m._forward_encoded_raw(cache, rows.data_ptr(), 6, True, 1)
    t = torch.full((3, 6), -1.0, dtype=torch.float64, device=DEV)
    out = _lib.McOut(mean=t.data_ptr())
    s = _lib.stream_ptr()
    assert m._lib.mmda_misa_mc_reduce(m._h, 4, 0, None, C.byref(out), None, 0, s) == -1          # 6 % 4
    assert m._lib.mmda_misa_mc_reduce(m._h, 2, 2, None, C.byref(out), None, 0, s) == -1          # which
    assert m._lib.mmda_misa_mc_reduce(m._h, 0, 0, None, C.byref(out), None, 0, s) == -1
    ent = _lib.McOut(entropy=t.data_ptr())
    assert m._lib.mmda_misa_mc_reduce(m._h, 2, 1, None, C.byref(ent), None, 0, s) == -1          # tcp is no probability of a label
    torch.cuda.synchronize()
    assert bool((t == -1.0).all())
    assert m._lib.mmda_misa_mc_reduce(m._h, 2, 0, None, C.byref(out), None, 0, s) == 0
    sc = m._public()["scores"].double().reshape(3, 2, 6)
    assert float((t - sc.sum(1) / 2).abs().max()) <= 1e-12


def test_failure_table_on_a_planted_case():
    """Tables planted by hand: every kind's AUROC equals ``failure_prediction`` called by hand on ``confidence(kind)``, against the same
    ``correct`` of the deterministic decision; the confidences are the documented transformations."""
    import math
    from mmda_amd import failure_prediction
    from mmda_amd.uncertainty import KINDS, MCDropoutResult
    g = torch.Generator().manual_seed(4)
    n, C = 40, 6
    u = lambda *s: torch.rand(*s, generator=g)
    scores, tcp = u(n, C), u(n, C)
    mean = u(n, C).double()
    h = lambda q: -q * torch.log(q) - (1 - q) * torch.log(1 - q)
    tables = dict(scores=scores, labels=(scores > 0.35).float(), tcp=tcp, mean=mean, var=u(n, C).double() * 0.25, entropy=h(mean),
                  expected_entropy=h(mean) * 0.5, mutual_info=h(mean) * 0.5, vote=u(n, C).double(), tcp_mean=u(n, C).double(),
                  tcp_var=u(n, C).double())
    res = MCDropoutResult({k: v.to(DEV) for k, v in tables.items()}, 8, [0], [np.arange(n)], None, None)
    truth = (u(n, C) > 0.5).float().to(DEV)
    correct = ((res.labels > 0) == (truth > 0)).float()
    assert 0 < float(correct.mean()) < 1
    table = res.failure_table(truth)
    assert tuple(table) == KINDS
    want = dict(mcp=torch.maximum(res.scores, 1 - res.scores), mc_mean=torch.maximum(res.mean, 1 - res.mean).float(),
                entropy=(1 - res.entropy / math.log(2.0)).float(), mutual_info=(-res.mutual_info).float(), variance=(-res.var).float(),
                tcp=res.tcp, tcp_mean=res.tcp_mean.float())
    for k in KINDS:
        conf = res.confidence(k)
        assert conf.dtype == torch.float32 and conf.shape == (n, C) and torch.equal(conf, want[k]), k
        by_hand = failure_prediction(conf, correct)
        assert torch.equal(_bits(table[k].table), _bits(by_hand.table)), k
        assert table[k].as_dict()["auroc"] == by_hand.as_dict()["auroc"]
    assert float(res.confidence("entropy").min()) >= -1e-6 and float(res.confidence("mcp").min()) >= 0.5
    assert set(res.failure_table(truth, kinds=("mcp", "tcp"))) == {"mcp", "tcp"}
    with pytest.raises(ValueError, match="unknown kind"):
        res.confidence("margin")


# ------------------------------------------------------------------------------------------------ solver and command line
class ListLoader:
    def __init__(self, batches):
        self.batches = batches
        self.dataset = self

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


def _solver(train, dev, test, name="mc", n_epoch=1, drop=(), **extra):
    from mmda_amd import make_config, models
    from mmda_amd.solver import Solver
    cfg = uc.config()
    cfg.learning_rate, cfg.clip = 1e-3, 1.0
    c = make_config(precision="fp32", device=DEV, n_epoch=n_epoch, name=name, **vars(cfg), **extra)
    for key in drop:                                                 # a configuration from before the option existed
        delattr(c, key)
    m = models.MISA(c)
    m.load_state_dict(uc.params())
    torch.manual_seed(0)                                             # build() draws the orthogonal recurrent weights
    return Solver(c, c, c, train, dev, test, is_train=True, model=m).build()


def test_solver_uncertainty_fills_last_uncertainty(dataset, capsys):
    from mmda_amd import DeviceLoader, MCDropoutPass
    from mmda_amd._lib import MMDAError
    s = _solver(ListLoader([]), DeviceLoader(dataset, 4), ListLoader([]))
    res = s.uncertainty("dev", passes=4, to_print=True)
    table = s.last_uncertainty
    assert tuple(table) == ("mcp", "mc_mean", "entropy", "mutual_info", "variance", "tcp", "tcp_mean")       # use_confidNet
    assert all(set(r) == {"auroc", "aupr_success", "aupr_error", "fpr_at_95tpr"} for r in table.values())
    want = res.failure_table(dataset.emo)
    for k, r in table.items():
        assert r["auroc"] == want[k].as_dict()["macro_auroc"], k
    text = capsys.readouterr().out
    assert "AUROC" in text and "mutual_info" in text and "4 MC-dropout draws" in text
    direct = MCDropoutPass(s.model, passes=4).run(dataset, 4)
    _same(res, direct, TABLES[:8])
    assert s.uncertainty("dev").passes == 32                          # config.mc_passes = 0: the pass's default
    with pytest.raises(ValueError, match="mode must be"):
        s.uncertainty("train")
    with pytest.raises(MMDAError, match="passes must be"):
        s.uncertainty("dev", passes=300)
    with pytest.raises(ValueError, match="must be a DeviceLoader"):
        s.uncertainty("test", passes=2)


def test_mc_passes_0_is_the_loop_without_the_option(dataset, tmp_path, monkeypatch, capsys):
    """train() with mc_passes = 0, and with a configuration from before the option existed: the same history, the same checkpoint
    bytes, the same printed text, no uncertainty pass.  With mc_passes = 3 the table follows the final test pass and nothing else moves."""
    from mmda_amd import DeviceLoader
    runs = {}
    for where, extra in (("with", dict(mc_passes=0)), ("without", dict(drop=("mc_passes",))), ("three", dict(mc_passes=3))):
        os.makedirs(tmp_path / where)
        monkeypatch.chdir(tmp_path / where)
        gen = torch.Generator().manual_seed(5)
        s = _solver(DeviceLoader(dataset, 4, shuffle=True, generator=gen), DeviceLoader(dataset, 4), DeviceLoader(dataset, 4), name="mc",
                    **extra)
        assert hasattr(s.train_config, "mc_passes") == (where != "without")
        capsys.readouterr()
        history = s.train()
        text = capsys.readouterr().out
        files = {f: open(tmp_path / where / "checkpoints" / f, "rb").read() for f in ("model_mc.std", "optim_mc.std")}
        runs[where] = (history, files, text)
        assert hasattr(s, "last_uncertainty") == (where == "three")
        if where == "three":
            assert set(s.last_uncertainty) >= {"mcp", "mutual_info", "tcp"} and "3 MC-dropout draws" in text
    assert runs["with"][0] == runs["without"][0] == runs["three"][0]
    assert runs["with"][1] == runs["without"][1] == runs["three"][1]
    assert runs["with"][2] == runs["without"][2] and "MC-dropout" not in runs["with"][2]


def test_a_train_step_after_the_pass_is_the_train_step_without_it(samples, dataset):
    """Two models with the same parameters and the same seed state take the same training step (dropout on, the seed drawn from the
    model's own sequence), one of them behind an MC-dropout pass: the same losses and the same parameters, bit for bit."""
    from mmda_amd import MCDropoutPass
    from mmda_amd.data import collate_fn
    t, v, a, _, emo, l, _, _, _, _ = collate_fn(list(samples))
    t, v, a, emo = (x.to(DEV) for x in (t, v, a, emo))
    out = []
    for with_pass in (True, False):
        m = _model("fp32").train()
        if with_pass:
            MCDropoutPass(m, passes=uc.K_SMALL, seed=3, columns=uc.COLUMNS_SMALL).run(dataset, 4)
            assert m.training
        m.train_step(t, v, a, l, emo, lr=1e-3, clip=1.0, training=True)
        torch.cuda.synchronize()
        out.append((m.read_losses(), {k: p.detach().clone() for k, p in m.state_dict().items()}))
    assert out[0][0] == out[1][0]
    assert all(torch.equal(out[0][1][k], out[1][1][k]) for k in out[1][1])
    assert any(not torch.equal(out[1][1][k].cpu(), uc.params()[k]) for k in out[1][1])        # the step did move the parameters
