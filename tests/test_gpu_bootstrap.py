"""GPU: the bootstrap kernels (csrc/bootstrap.hip) against the host's MATERIALISED resamples -- every replicate's rows gathered with
``resample_indices`` and run through the existing ``get_metrics`` and ``rank_counts_host`` + ``figures_from_counts`` -- and
``Solver.bootstrap``, ``config.bootstrap`` and the two joins end to end on the tiny model of tests/uncertainty_cases.py (the
configuration of tests/test_gpu_inference.py with the confidence head, n = 7).

Shapes (bootstrap_cases.gpu_shapes; tests/test_bootstrap_cpu.py proves which form each reaches): (1, 1), (2, 1), (37, 6), (300, 16),
the count kernel's threads per workgroup - 1 / + 0 / + 1 at six classes, and the LDS edge (16384, 6) / (16385, 6): the ranking call
refuses the second by name, the decision call takes the global form.  R in {1, 2, 65} on the small shapes, 3 on the two large ones; a
replicate does not depend on R, so the host yardstick is made once per shape at the largest R.  Bounds: tests/bootstrap_cases.py; a
summary is compared with ``summary_host`` of the device's own figure table: the same bits, but ``std``, whose division and square
root are the device's own (2 ulp)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bootstrap_cases as bc
import uncertainty_cases as uc
from mmda_amd import bootstrap as bt

DEV = "cuda:0"
SHAPES = bc.gpu_shapes()
RUNS = [(s, R) for s in SHAPES for R in bc.replicates(s)]
ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


@pytest.fixture(scope="module")
def cases():
    """Per shape: the tables on both sides and, for the largest R, the materialised yardstick per replicate (computed once, never
    written): integer states, get_metrics dicts and ranking tables; index R is the identity's."""
    out = {}
    for shape in SHAPES:
        n, C = shape
        case, R = bc.case(n, C), max(bc.replicates(shape))
        j = list(bt.resample_indices(bc.SEED, R, n)) + [np.arange(n)]
        case["decisions"] = [bc.materialised_decisions(case["labels"], case["truth_d"], rows) for rows in j]
        case["ranking"] = [bc.materialised_ranking(case["scores"], case["truth"], rows) for rows in j] if n <= bt.RANK_MAX_ROWS else None
        case["dev"] = {k: torch.from_numpy(case[k]).to(DEV) for k in ("scores", "truth", "labels", "truth_d")}
        case["R"] = R
        out[shape] = case
    return out


def _rows(case, R):
    """the yardstick's indices of a run with R replicates: replicates 0 .. R - 1, then the identity"""
    return list(range(R)) + [case["R"]]


# ------------------------------------------------------------------------------------------------ 1: decisions
@pytest.mark.parametrize("shape,R", RUNS, ids=ids)
def test_decision_states_and_figures_equal_the_materialised_resample(cases, shape, R):
    from mmda_amd.utils.eval import DeviceEval
    n, C = shape
    case, d = cases[shape], cases[shape]["dev"]
    bs = bt.Bootstrap(n, R, bc.SEED, DEV)
    forms = ("auto", "lds", "global") if n <= 16384 else ("auto", "global")
    res = {form: bs.decisions(d["labels"], d["truth_d"], form=form) for form in forms}
    auto = res["auto"]
    assert auto.state.shape == (R + 1, 3 * C + 2) and auto.state.dtype == torch.int64 and auto.state.is_cuda
    assert auto.figures.shape == (R + 1, 10 + 3 * C) and auto.figures.dtype == torch.float64 and auto.names == bt.decision_names(C)
    for form in forms[1:]:                                          # integer adds only: the form does not show
        assert torch.equal(res[form].state, auto.state) and torch.equal(res[form].figures.view(torch.int64), auto.figures.view(torch.int64))
    state, figures = auto.state.cpu().numpy(), auto.figures.cpu().numpy()
    for row, at in enumerate(_rows(case, R)):
        want_state, want = case["decisions"][at]
        assert np.array_equal(state[row], want_state), row
        bc.check_decision_figures(figures[row], want_state, want, C)
    if n <= 16384:
        with pytest.raises(ValueError, match="form must be"):
            bs.decisions(d["labels"], d["truth_d"], form="registers")
    else:
        from mmda_amd._lib import MMDAError
        with pytest.raises(MMDAError, match="mmda_boot_counts"):
            bs.decisions(d["labels"], d["truth_d"], form="lds")
    ev = DeviceEval(C, DEV)                                         # the identity row: the unresampled counts
    ev.update(d["labels"], d["truth_d"])
    st = ev.state.cpu().numpy()
    assert np.array_equal(state[R, :3 * C].astype(np.float64), st[:3 * C]) and state[R, 3 * C + 1] == st[3 * C + 1] == n
    assert abs(state[R, 3 * C] / bt.LCM - st[3 * C]) <= n * bc.EPS * max(1.0, st[3 * C])


# ------------------------------------------------------------------------------------------------ 2: ranking
@pytest.mark.parametrize("shape,R", RUNS, ids=ids)
def test_ranking_tables_equal_the_materialised_resample(cases, shape, R):
    from mmda_amd import ranking_metrics
    from mmda_amd._lib import MMDAError
    n, C = shape
    case, d = cases[shape], cases[shape]["dev"]
    bs = bt.Bootstrap(n, R, bc.SEED, DEV)
    if n > bt.RANK_MAX_ROWS:
        with pytest.raises(MMDAError, match="over the limit of 16384 rows"):
            bs.ranking(d["scores"], d["truth"])
        return
    res = bs.ranking(d["scores"], d["truth"], tpr=0.95)
    assert res.figures.shape == (R + 1, 6 * (C + 1)) and res.figures.dtype == torch.float64 and res.figures.is_cuda
    assert res.names == bt.ranking_names(C) and res.state is None
    table = res.table.cpu().numpy()
    assert table.shape == (R + 1, C + 1, 6)
    for row, at in enumerate(_rows(case, R)):
        bc.check_rank_table(table[row], case["ranking"][at], C)
    bc.check_rank_table(table[R], ranking_metrics(d["scores"], d["truth"], tpr=0.95).table.cpu().numpy(), C)
    if shape == (37, 6):                                            # another level, and the failure-prediction names
        res = bs.ranking(d["scores"], d["truth"], tpr=0.5, failure=True)
        want = bc.materialised_ranking(case["scores"], case["truth"], bt.resample_indices(bc.SEED, 1, n)[0], tpr=0.5)
        bc.check_rank_table(res.table.cpu().numpy()[0], want, C)
        assert res.names[-1] == "macro_fpr_at_50tpr"
        with pytest.raises(ValueError, match="tpr must be"):
            bs.ranking(d["scores"], d["truth"], tpr=0.0)


# ------------------------------------------------------------------------------------------------ 3: summary and compare
def _check_summary(got, want):
    assert got.shape == want.shape
    for k in range(want.shape[1]):
        if k != 2:
            bad = [(f, got[f, k].hex(), want[f, k].hex()) for f in range(want.shape[0]) if not bc.same_bits(got[f, k], want[f, k])]
            assert not bad, (bt.COMPARE_COLUMNS[k], bad)
    assert np.array_equal(np.isnan(got[:, 2]), np.isnan(want[:, 2]))
    assert (np.nan_to_num(np.abs(got[:, 2] - want[:, 2])) <= 2.0 ** -51 * np.nan_to_num(np.abs(want[:, 2]))).all()


@pytest.mark.parametrize("R", [1, 2, 3, 64, 65, 2000, 8192])
def test_summary_and_compare_of_planted_tables(R):
    bs = bt.Bootstrap(1, R, 0, DEV)
    a, b = bc.summary_table(R, 9, seed=1), bc.summary_table(R, 9, seed=2)
    da, db = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    names = tuple(f"f{k}" for k in range(9))
    s = bs._summary(da, None, names, 0.05)
    assert s.table.shape == (9, 6) and s.table.is_cuda and s.columns == bt.SUMMARY_COLUMNS
    _check_summary(s.table.cpu().numpy(), bt.summary_host(a, 0.05))
    c = bs._summary(da, db, names, 0.1)
    assert c.table.shape == (9, 9) and c.columns == bt.COMPARE_COLUMNS
    _check_summary(c.table.cpu().numpy(), bt.summary_host(a, 0.1, other=b))
    assert set(s.as_dict()["f0"]) == set(bt.SUMMARY_COLUMNS) and set(c.as_dict()["f6"]) == set(bt.COMPARE_COLUMNS)


@pytest.mark.parametrize("shape", [(37, 6), (300, 16)], ids=ids)
def test_summary_and_compare_of_the_devices_own_figures(cases, shape):
    from mmda_amd._lib import MMDAError
    n, C = shape
    d = cases[shape]["dev"]
    bs = bt.Bootstrap(n, 65, bc.SEED, DEV)
    m, r = bs.decisions(d["labels"], d["truth_d"]), bs.ranking(d["scores"], d["truth"])
    for res in (m, r):
        _check_summary(res.summary(0.05).table.cpu().numpy(), bt.summary_host(res.figures.cpu().numpy(), 0.05))
    assert np.isnan(r.summary().table.cpu().numpy()[:, 1]).any()    # the class without positives: no replicate defines its AUROC
    other = bs.decisions((d["scores"] > 0.5).float(), d["truth_d"])
    cmp = bs.compare(m, other, alpha=0.1)
    _check_summary(cmp.table.cpu().numpy(), bt.summary_host(m.figures.cpu().numpy(), 0.1, other=other.figures.cpu().numpy()))
    same = bs.compare(m, m).table.cpu().numpy()
    assert (same[:, :5] == 0).all() and (same[:, 5] == 65).all() and (same[:, 6:] == 1).all()
    with pytest.raises(MMDAError, match="figure sets differ"):
        bs.compare(m, r)
    with pytest.raises(MMDAError, match="different Bootstrap"):
        bs.compare(m, bt.Bootstrap(n, 65, bc.SEED, DEV).decisions(d["labels"], d["truth_d"]))
    with pytest.raises(ValueError, match="resamples n = 37|resamples n = 300"):
        bs.decisions(d["labels"][:-1], d["truth_d"][:-1])


# ------------------------------------------------------------------------------------------------ 4: reproducibility
@pytest.mark.parametrize("shape", [(300, 16), (16384, 6)], ids=ids)
def test_two_runs_on_fresh_buffers_give_the_same_bits(cases, shape):
    n, C = shape
    case, runs = cases[shape], []
    for _ in range(2):
        d = {k: torch.from_numpy(case[k]).to(DEV) for k in ("scores", "truth", "labels", "truth_d")}
        bs = bt.Bootstrap(n, 3 if n > 4096 else 65, bc.SEED, DEV)
        m, r = bs.decisions(d["labels"], d["truth_d"]), bs.ranking(d["scores"], d["truth"])
        runs.append([m.state, m.figures, r.figures, m.summary().table, r.summary().table, bs.compare(m, m).table])
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))


# ------------------------------------------------------------------------------------------------ 5: solver, flag and joins
def _solver(train, dev, test, name="boot", n_epoch=1, drop=(), **extra):
    from mmda_amd import make_config, models
    from mmda_amd.solver import Solver
    cfg = uc.config()
    cfg.learning_rate, cfg.clip = 1e-3, 1.0
    c = make_config(precision="fp32", device=DEV, n_epoch=n_epoch, name=name, **vars(cfg), **extra)
    for key in drop:
        delattr(c, key)
    m = models.MISA(c)
    m.load_state_dict(uc.params())
    torch.manual_seed(0)
    return Solver(c, c, c, train, dev, test, is_train=True, model=m).build()


class ListLoader:
    def __init__(self, batches):
        self.batches, self.dataset = batches, self

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


@pytest.fixture(scope="module")
def dataset():
    from mmda_amd import DeviceDataset
    return DeviceDataset.from_samples(uc.make_samples(), DEV)


def test_solver_bootstrap_end_to_end(dataset, capsys):
    from mmda_amd import DeviceLoader
    from mmda_amd._lib import MMDAError
    from mmda_amd.calibrate import Thresholds
    from mmda_amd.utils.eval import KEYS
    s = _solver(ListLoader([]), DeviceLoader(dataset, 4), ListLoader([]))
    C, n = 6, len(dataset)
    out = s.bootstrap("dev", replicates=65, to_print=True)
    assert out is s.last_bootstrap and out["vs_default"] is None and out["bootstrap"].n == n
    text = capsys.readouterr().out
    assert "65 replicates" in text and "macro_auroc" in text and "weighted_recall" in text and "[" in text
    s.eval("dev")
    metrics = out["summaries"]["metrics"].as_dict()
    assert abs(metrics["acc"]["point"] - s.last_eval_metrics["acc"]) <= 0.5e-4 + bc.EPS
    for key in KEYS[1:]:
        assert abs(metrics[key]["point"] - s.last_eval_metrics[key]) <= (C + 2) * bc.EPS, key
    ranked = s.rank("dev")
    for kind, res in (("ranking", ranked["scores"]), ("confidence", ranked["confidence"])):
        assert out[kind] is not None
        bc.check_rank_table(out[kind].table[65].cpu().numpy(), res.table.cpu().numpy(), C)
        t = out["summaries"][kind].table.cpu().numpy()
        ok = ~np.isnan(t[:, 3])
        assert (t[ok, 3] <= t[ok, 4]).all() and (t[:, 5] <= 65).all() and (t[:, 5] >= 0).all()
    assert out["confidence"].names[2] == "auroc[0]" and out["confidence"].names[-1] == "macro_fpr_at_95tpr"
    t = out["summaries"]["metrics"].table.cpu().numpy()
    assert (t[:, 3] <= t[:, 4]).all() and (t[:, 5] == 65).all()
    fixed = Thresholds([float(s.train_config.threshold)] * C, [0] * C)
    again = s.bootstrap("dev", replicates=65, thresholds=fixed)
    vs = again["vs_default"].table.cpu().numpy()
    assert vs.shape == (10 + 3 * C, 9) and (vs[:, :5] == 0).all() and (vs[:, 8] == 1).all()
    assert s.bootstrap("dev", replicates=65, confidence=False)["confidence"] is None
    with pytest.raises(MMDAError, match="replicates must be an integer"):
        s.bootstrap("dev", replicates=0)
    with pytest.raises(ValueError, match="mode must be"):
        s.bootstrap("train", replicates=5)


def test_bootstrap_0_is_the_loop_without_the_option(dataset, tmp_path, monkeypatch, capsys):
    """train() with bootstrap = 0, and with a configuration from before the option existed: the same history, checkpoint bytes and
    printed text.  With bootstrap = 5 the table follows the final test pass and nothing else moves."""
    from mmda_amd import DeviceLoader
    runs = {}
    for where, extra in (("with", dict(bootstrap=0)), ("without", dict(drop=("bootstrap",))), ("five", dict(bootstrap=5))):
        os.makedirs(tmp_path / where)
        monkeypatch.chdir(tmp_path / where)
        gen = torch.Generator().manual_seed(5)
        s = _solver(DeviceLoader(dataset, 4, shuffle=True, generator=gen), DeviceLoader(dataset, 4), DeviceLoader(dataset, 4), **extra)
        capsys.readouterr()
        history = s.train()
        text = capsys.readouterr().out
        files = {f: open(tmp_path / where / "checkpoints" / f, "rb").read() for f in ("model_boot.std", "optim_boot.std")}
        runs[where] = (history, files, text)
        assert hasattr(s, "last_bootstrap") == (where == "five")
        if where == "five":
            assert "5 replicates" in text and s.last_bootstrap["metrics"].figures.shape[0] == 6
    assert runs["with"][0] == runs["without"][0] == runs["five"][0]
    assert runs["with"][1] == runs["without"][1] == runs["five"][1]
    assert runs["with"][2] == runs["without"][2] and "replicates" not in runs["with"][2]


def test_the_two_joins(dataset):
    from mmda_amd import MCDropoutPass, ModalityPass
    from mmda_amd.utils.eval import KEYS
    s = _solver(ListLoader([]), ListLoader([]), ListLoader([]))
    C, n = 6, len(dataset)
    res = ModalityPass(s.model).run(dataset, 4)
    boot = res.bootstrap(replicates=65, seed=3)
    F = 10 + 3 * C
    assert boot["summary"].shape == (8, F, 6) and boot["vs_full"].shape == (8, F, 9) and len(boot["names"]) == F and len(boot["results"]) == 8
    summary, plain = boot["summary"].cpu().numpy(), res.metrics()
    for k in range(8):
        assert abs(summary[k, 0, 0] - plain[k]["acc"]) <= 0.5e-4 + bc.EPS
        for f, key in enumerate(KEYS[1:], start=1):
            assert abs(summary[k, f, 0] - plain[k][key]) <= (C + 2) * bc.EPS, (k, key)
    vs = boot["vs_full"].cpu().numpy()
    assert (vs[7, :, :5] == 0).all() and (vs[7, :, 8] == 1).all()
    assert bc.same_bits(vs[:, :, 0], summary[:, :, 0] - summary[7:8, :, 0])
    mc = MCDropoutPass(s.model, passes=4).run(dataset, 4)
    plain = mc.failure_table(dataset.emo)
    bs = bt.Bootstrap(n, 65, 0, DEV)
    table = mc.failure_table(dataset.emo, bootstrap=bs)
    assert set(table) == set(plain) and "tcp" in table
    for kind, row in table.items():
        assert row["summary"].table.shape == (6 * (C + 1), 6) and row["vs_tcp"].table.shape == (6 * (C + 1), 9)
        bc.check_rank_table(row["result"].table[65].cpu().numpy(), plain[kind].table.cpu().numpy(), C)
        assert bc.same_bits(row["summary"].table[:, 0].cpu().numpy(), row["result"].figures[65].cpu().numpy())
    own = table["tcp"]["vs_tcp"].table.cpu().numpy()
    ok = ~np.isnan(own[:, 0])
    assert (own[ok, 0] == 0).all() and (own[:, 8] == 1).all()
    assert set(mc.failure_table(dataset.emo, kinds=("mcp",), bootstrap=bs)["mcp"]) == {"result", "summary", "vs_tcp"}
    assert mc.failure_table(dataset.emo, kinds=("mcp",), bootstrap=bs)["mcp"]["vs_tcp"] is None
