"""GPU: the Trust Score chain (mmda_amd/neighbours.py) -- ``TrustIndex.fit`` / ``.score``, ``NeighbourIndex.vote``,
``mmda_trust_score`` -- against the numpy definitions of tests/knn_cases.py, and ``Solver.trust`` on the tiny synthetic solver of
tests/test_gpu_solver.py.  With real-valued tables the definitions are fed the kernel's own distances (the search itself is
tests/test_gpu_knn.py's subject) and everything behind them must agree bit for bit: the kept-member masks, and ``trust``, whose sqrt and
division are correctly rounded in float64.  With an integer-valued table the distances are exact too, so the whole chain equals the
int64 reference bit for bit."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import knn_cases as kc

DEV = "cuda:0"
N, NQ, D, K = 300, 65, 48, 10


def _tables(C, integer=False, seed=0):
    rng = np.random.default_rng(77 + seed + C)
    if integer:
        base, query = (rng.integers(-8, 9, size=(r, D)).astype(np.float32) for r in (N, NQ))
        query[::4] = base[:NQ:4]                                      # exact zeros and ties
    else:
        base, query = (rng.standard_normal((r, D)).astype(np.float32) for r in (N, NQ))
    truth = rng.integers(0, 2, size=(N, C)).astype(np.float32)
    labels = rng.integers(0, 2, size=(NQ, C)).astype(np.float32)
    return base, query, truth, labels


def _dev(*arrays):
    return [torch.tensor(a).to(DEV) for a in arrays]


def _bits(x):
    return x.contiguous().view(torch.int64 if x.dtype == torch.float64 else torch.int32)


@pytest.mark.parametrize("alpha", [0.0, 0.25])
@pytest.mark.parametrize("C", [6, 1])
def test_fit_and_score_are_the_definition_on_the_kernels_distances(C, alpha):
    from mmda_amd import TrustIndex, knn_search
    base, query, truth, labels = _tables(C)
    b, q, t, lab = _dev(base, query, truth, labels)
    index = TrustIndex.fit(b, t, k=K, alpha=alpha)
    inside = ((kc.ref_members(truth)[:, None] >> np.arange(2 * C)[None, :]) & 1).astype(bool)
    if alpha == 0.0:
        assert index.radius is None
        want_kept = inside
    else:
        own, _ = knn_search(b, b, K, member=torch.tensor(kc.ref_members(truth)).to(DEV), sets=2 * C)
        radius = np.where(inside, own[:, :, K - 1].cpu().numpy(), np.inf)
        assert np.array_equal(index.radius.cpu().numpy(), radius)
        want_kept = kc.ref_density_filter(radius, inside, K, alpha)
        assert want_kept.sum() < inside.sum()
        for s in range(2 * C):                                        # the nearest-rank quantile keeps ceil((1 - alpha) m), ties aside
            assert want_kept[:, s].sum() >= int(np.ceil((1 - alpha) * inside[:, s].sum()))
    assert np.array_equal(index.kept.cpu().numpy(), want_kept)
    want_members = (want_kept.astype(np.int64) << np.arange(2 * C)[None, :]).sum(axis=1).astype(np.int32)
    assert np.array_equal(index.members.cpu().numpy(), want_members)
    res = index.score(q, lab)
    dist, idx = knn_search(q, b, 1, member=torch.tensor(want_members).to(DEV), sets=2 * C)
    want, p, o = kc.ref_trust(dist.cpu().numpy(), labels)
    assert res.trust.dtype == torch.float64 and tuple(res.trust.shape) == (NQ, C)
    assert np.array_equal(res.trust.cpu().numpy().view(np.int64), want.view(np.int64))
    assert np.array_equal(res.d_pred.cpu().numpy(), p) and np.array_equal(res.d_other.cpu().numpy(), o)
    y = (labels > 0).astype(np.int64)
    first = idx[:, :, 0].cpu().numpy()
    cols = 2 * np.arange(C)[None, :]
    assert np.array_equal(res.nearest_pred.cpu().numpy(), np.take_along_axis(first, cols + y, axis=1))
    assert np.array_equal(res.nearest_other.cpu().numpy(), np.take_along_axis(first, cols + 1 - y, axis=1))
    assert res.confidence().dtype == torch.float32 and torch.equal(res.confidence(), res.trust.to(torch.float32))
    host = res.cpu()
    assert not host.trust.is_cuda and set(res.as_dict()) == set(res.TABLES) | {"k", "alpha"}


@pytest.mark.parametrize("alpha", [0.0, 0.25])
def test_integer_table_the_whole_chain_is_the_reference(alpha):
    from mmda_amd import TrustIndex
    C = 6
    base, query, truth, labels = _tables(C, integer=True)
    b, q, t, lab = _dev(base, query, truth, labels)
    members = kc.ref_members(truth)
    inside = ((members[:, None] >> np.arange(2 * C)[None, :]) & 1).astype(bool)
    kept = inside
    if alpha > 0:
        own, _, _ = kc.ref_knn(kc.pair_distances(base, base, integer=True), members, 2 * C, K)
        kept = kc.ref_density_filter(np.where(inside, own[:, :, K - 1], np.inf), inside, K, alpha)
    members = (kept.astype(np.int64) << np.arange(2 * C)[None, :]).sum(axis=1).astype(np.int32)
    dist, idx, _ = kc.ref_knn(kc.pair_distances(query, base, integer=True), members, 2 * C, 1)
    want, p, o = kc.ref_trust(dist, labels)
    index = TrustIndex.fit(b, t, k=K, alpha=alpha)
    res = index.score(q, lab)
    assert np.array_equal(index.kept.cpu().numpy(), kept)
    assert np.array_equal(res.trust.cpu().numpy().view(np.int64), want.view(np.int64))
    assert np.array_equal(res.d_pred.cpu().numpy(), p.astype(np.float32))
    assert np.array_equal(res.d_other.cpu().numpy(), o.astype(np.float32))
    hit = (p == 0) & (o > 0)                                         # queries that are base rows: 1e-12 keeps the ratio finite
    assert hit.any() and np.all(want[hit] > 1e11) and np.all(np.isfinite(want))


def test_vote_is_a_numpy_gather():
    from mmda_amd import NeighbourIndex
    base, query, truth, _ = _tables(6)
    b, q, t = _dev(base, query, truth)
    ni = NeighbourIndex(b, t)
    _, index = ni.search(q, 7)
    vote = ni.vote(q, 7)
    assert vote.dtype == torch.float32 and tuple(vote.shape) == (NQ, 6)
    assert np.array_equal(vote.cpu().numpy(), kc.ref_vote(index.cpu().numpy(), truth))
    few = NeighbourIndex(b[:3], t[:3])                                # fewer rows than k: the share among the three there are
    assert np.array_equal(few.vote(q, 7).cpu().numpy(), kc.ref_vote(few.search(q, 7)[1].cpu().numpy(), truth[:3]))
    with pytest.raises(ValueError, match="truth"):
        NeighbourIndex(b).vote(q, 3)


def test_a_class_that_is_never_positive():
    from mmda_amd import TrustIndex
    base, query, truth, labels = _tables(6)
    truth = truth.copy()
    truth[:, 2] = 0.0
    b, q, t, lab = _dev(base, query, truth, labels)
    res = TrustIndex.fit(b, t, k=K, alpha=0.25).score(q, lab)
    trust, y = res.trust.cpu().numpy(), labels[:, 2] > 0
    assert y.any() and (~y).any()
    assert np.all(trust[y, 2] == 0.0) and np.all(np.isposinf(trust[~y, 2]))                # decided positive: no such row; else no other
    assert np.all(res.nearest_pred.cpu().numpy()[y, 2] == -1) and np.all(res.nearest_other.cpu().numpy()[~y, 2] == -1)
    assert np.all(np.isfinite(np.delete(trust, 2, axis=1)))


# ---------------------------------------------------------------------------------------------- Solver.trust
def _figures(fp):
    d = fp.as_dict()
    return dict(auroc=d["macro_auroc"], aupr_success=d["macro_aupr_success"], aupr_error=d["macro_aupr_error"],
                fpr_at_95tpr=d["macro_fpr_at_95tpr"])


def test_solver_trust_is_the_manual_composition(monkeypatch, capsys):
    from test_gpu_solver import _solver
    from mmda_amd import Bootstrap, InferencePass, TrustIndex, failure_prediction
    s, cfg, _, train, dev = _solver(monkeypatch)
    res = s.trust("dev", k=3, alpha=0.25, to_print=True)
    text = capsys.readouterr().out
    base = InferencePass(s.model, ("hidden",)).run_loader(s.train_data_loader)
    got = InferencePass(s.model, ("scores", "labels", "tcp", "hidden")).run_loader(s.dev_data_loader)
    fit_truth = torch.cat([b["emo"] for b in train], 0).to(DEV)
    truth = torch.cat([b["emo"] for b in dev], 0).to(DEV)
    index = TrustIndex.fit(base.hidden, fit_truth, k=3, alpha=0.25)
    want = index.score(got.hidden, got.labels)
    assert torch.equal(_bits(res.trust), _bits(want.trust))
    correct = ((got.labels > 0) == (truth > 0)).to(torch.float32)
    kinds = ("mcp", "trust") + (("tcp",) if getattr(s.train_config, "use_confidNet", False) else ())
    assert tuple(s.last_trust) == kinds
    conf = dict(mcp=torch.maximum(got.scores, 1.0 - got.scores), trust=want.confidence(), tcp=got.tcp)
    for kind in kinds:
        assert np.array_equal(np.array(list(s.last_trust[kind].values())),
                              np.array(list(_figures(failure_prediction(conf[kind], correct)).values())), equal_nan=True), kind
        assert kind in text
    assert "Trust Score against the train split (k = 3, alpha = 0.25" in text and "AUROC" in text
    assert s.last_trust_bootstrap is None
    n = int(truth.shape[0])
    s.trust("dev", k=3, bootstrap=Bootstrap(n, 40, 0, DEV))
    assert tuple(s.last_trust_bootstrap) == tuple(k for k in ("trust", "mcp", "tcp") if k in kinds)
    for kind, row in s.last_trust_bootstrap.items():
        assert set(row) == {"result", "summary", "vs_tcp"} and row["summary"] is not None
        assert (row["vs_tcp"] is not None) == ("tcp" in kinds)
    with pytest.raises(ValueError, match="mode must be"):
        s.trust("train")
    with pytest.raises(ValueError, match="k must be"):
        s.trust("dev", k=17)
    with pytest.raises(ValueError, match="alpha must be"):
        s.trust("dev", alpha=1.0)


def test_trust_k_0_is_the_loop_without_the_option(monkeypatch, tmp_path, capsys):
    """train() with trust_k = 0, and with a configuration from before the option existed: the same history, the same checkpoint bytes,
    the same printed text, no Trust Score pass.  With trust_k = 3 the table follows the final test pass and nothing else moves."""
    from test_gpu_solver import _solver
    runs = {}
    for where in ("with", "without", "three"):
        os.makedirs(tmp_path / where)
        monkeypatch.chdir(tmp_path / where)
        torch.manual_seed(0)
        s, *_ = _solver(monkeypatch, name="tr")
        assert s.train_config.trust_k == 0 and s.train_config.trust_alpha == 0.0
        if where == "without":
            delattr(s.train_config, "trust_k")
            delattr(s.train_config, "trust_alpha")
        if where == "three":
            s.train_config.trust_k = 3
        capsys.readouterr()
        history = s.train()
        text = capsys.readouterr().out
        files = {f: open(tmp_path / where / "checkpoints" / f, "rb").read() for f in ("model_tr.std", "optim_tr.std")}
        runs[where] = (history, files, text)
        assert hasattr(s, "last_trust") == (where == "three")
        if where == "three":
            assert set(s.last_trust) >= {"mcp", "trust"} and "Trust Score against the train split (k = 3" in text
    assert runs["with"][0] == runs["without"][0] == runs["three"][0]
    assert runs["with"][1] == runs["without"][1] == runs["three"][1]
    assert runs["with"][2] == runs["without"][2] and "Trust Score" not in runs["with"][2]
