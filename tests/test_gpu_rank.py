"""GPU: ranking metrics -- ``mmda_rank_counts`` against the host ``rank_counts_host`` (integer equality; the host sorts, the kernel
compares every pair), ``mmda_rank_finish`` against ``figures_from_counts``, ``mmda_rank_rows_accumulate`` against ``label_ranking_host``,
and ``Solver.rank`` / ``failure_prediction`` / ``config.select_by`` end to end on the tiny model of tests/test_gpu_inference.py.

Shapes (rank_cases.gpu_shapes; tests/test_rank_cpu.py proves which plan form each reaches): (1, 1), (2, 1), (37, 6), (300, 16), rows per
workgroup - 1 / + 0 / + 1 and j-tile - 1 / + 0 / + 1 with six classes each, one above the size where a 16-class table stops being
split, and (20001, 6).  Every table of six classes or more holds every value class (rank_cases.value_case; tests/test_rank_cpu.py
checks that from the tables), the two single-class shapes what one column can hold.

Bounds: counts and the row state are integers, compared for equality.  ``auroc`` and ``fpr_at_tpr`` are an integer reduction and one
fp64 division on both sides: the same bits.  ``ap`` / ``ap_neg`` add P (Nn) quotients of integers, each in [0, 1] and each the same
bits on both sides, in two different orders: either sum is within (P - 1) 2^-53 P of the exact one, so they differ by at most
P^2 2^-52, and by P 2^-52 after the division by P.  The macro row adds C <= 16 such figures in class order on both sides; it is held
to C 2^-52 against the nan-mean of the device's own class rows."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import misa_oracle as orc
from rank_cases import gpu_shapes, value_case

DEV = "cuda:0"
MOSEI = (35, 74)
SHAPES = gpu_shapes()
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def cases():
    """Per shape: host inputs, the host counts, table and row state (the yardstick; computed once, never written), the device copies."""
    from mmda_amd import ranking as rk
    out = {}
    for shape in SHAPES:
        s, t = value_case(*shape)
        counts = rk.rank_counts_host(s, t)
        out[shape] = dict(scores=s, truth=t, counts=counts, table=rk.figures_from_counts(counts, t, 0.95),
                          rows=rk.label_ranking_host(s, t), s_dev=torch.from_numpy(s).to(DEV), t_dev=torch.from_numpy(t).to(DEV))
    return out


def same_bits(a, b):
    """equal values, NaN where the other is NaN"""
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


def check_table(got, want, C):
    """a device table against the yardstick's: the rules of the module docstring"""
    assert got.shape == want.shape == (C + 1, 6)
    assert np.array_equal(np.isnan(got), np.isnan(want))        # NaN exactly where a figure is undefined
    assert np.array_equal(got[:C, :2], want[:C, :2])
    assert same_bits(got[:C, 2], want[:C, 2]) and same_bits(got[:C, 5], want[:C, 5])
    P, Nn = want[:C, 0], want[:C, 1]
    for col, n in ((3, P), (4, Nn)):
        diff = np.abs(got[:C, col] - want[:C, col])
        print("column", col, "largest difference", np.nanmax(diff, initial=0.0), "bound at that class", n[np.nanargmax(np.nan_to_num(diff))] * EPS)
        assert (np.nan_to_num(diff) <= n * EPS).all(), col
    assert np.array_equal(got[C, :2], want[C, :2])
    for f in range(2, 6):                                       # the macro row: nan-mean of the device's own class rows, in class order
        vals = [v for v in got[:C, f] if not np.isnan(v)]
        if not vals:
            assert np.isnan(got[C, f])
        else:
            total = 0.0
            for v in vals:
                total += v
            assert abs(got[C, f] - total / len(vals)) <= C * EPS, f
            assert abs(got[C, f] - np.nanmean(got[:C, f])) <= C * EPS, f


# ------------------------------------------------------------------------------------------------ 1: counts, table, row state
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_counts_table_and_rows_equal_the_host(cases, shape):
    from mmda_amd import ranking as rk
    N, C = shape
    case = cases[shape]
    counts = rk.rank_counts(case["s_dev"], case["t_dev"])
    assert counts.shape == (N, C, 4) and counts.dtype == torch.int32
    got = counts.cpu().numpy().view(np.uint32)
    assert np.array_equal(got, case["counts"])
    res = rk.ranking_metrics(case["s_dev"], case["t_dev"], tpr=0.95)
    assert res.table.is_cuda and res.table.dtype == torch.float64 and res.rows.is_cuda
    assert torch.equal(res.counts, counts)
    check_table(res.table.cpu().numpy(), case["table"], C)
    # the row state: integers; streamed in two halves == in one call
    assert np.array_equal(res.rows.cpu().numpy(), case["rows"])
    halves = rk.RowRanking(C, DEV)
    halves.update(case["s_dev"][:N // 2], case["t_dev"][:N // 2])
    halves.update(case["s_dev"][N // 2:], case["t_dev"][N // 2:])
    assert torch.equal(halves.state, res.rows)
    want = rk.label_ranking_figures(case["rows"], C)
    d = res.as_dict()
    assert all(same_bits(d[k], want[k]) for k in ("lrap", "ranking_loss", "coverage_error"))
    assert same_bits(d["macro_auroc"], res.table[C, 2].item()) and same_bits(d["map"], res.table[C, 3].item())
    assert len(d["auroc"]) == C and d["tpr"] == 0.95
    # a second run gives the same bits
    again = rk.ranking_metrics(case["s_dev"], case["t_dev"], tpr=0.95)
    assert torch.equal(again.counts, res.counts) and torch.equal(again.rows, res.rows)
    assert torch.equal(again.table.view(torch.int64), res.table.view(torch.int64))


@pytest.mark.parametrize("shape", [(37, 6), (300, 16)], ids=lambda s: "x".join(map(str, s)))
def test_other_levels_and_the_pooled_figures(cases, shape):
    from mmda_amd import ranking as rk
    N, C = shape
    case = cases[shape]
    for level in (0.5, 1.0):
        res = rk.ranking_metrics(case["s_dev"], case["t_dev"], tpr=level, label_ranking=False)
        assert res.rows is None
        check_table(res.table.cpu().numpy(), rk.figures_from_counts(case["counts"], case["truth"], level), C)
    res = rk.ranking_metrics(case["s_dev"], case["t_dev"], micro=True)
    s1, t1 = case["scores"].reshape(N * C, 1), case["truth"].reshape(N * C, 1)
    check_table(res.micro.cpu().numpy(), rk.figures_from_counts(rk.rank_counts_host(s1, t1), t1, 0.95), 1)
    d = res.as_dict()
    assert same_bits(d["micro_auroc"], res.micro[0, 2].item()) and same_bits(d["micro_ap"], res.micro[0, 3].item())
    host = res.cpu()
    assert not host.table.is_cuda and host.counts is None and torch.equal(host.rows, res.rows.cpu())


def test_refusals_and_the_empty_table(cases):
    from mmda_amd import _lib, ranking as rk
    case = cases[(37, 6)]
    with pytest.raises(_lib.MMDAError, match="ranking_metrics"):
        rk.ranking_metrics(torch.from_numpy(case["scores"]), case["t_dev"])
    with pytest.raises(ValueError, match=r"\(N, C\)"):
        rk.ranking_metrics(case["s_dev"][:, :5], case["t_dev"])
    with pytest.raises(ValueError, match="tpr"):
        rk.ranking_metrics(case["s_dev"], case["t_dev"], tpr=1.5)
    with pytest.raises(ValueError, match=r"2\^20"):             # refused by its size, before any launch
        rk.ranking_metrics(torch.empty((1 << 20) + 1, 1, device=DEV), torch.empty((1 << 20) + 1, 1, device=DEV))
    res = rk.ranking_metrics(case["s_dev"][:0], case["t_dev"][:0])
    t = res.table.cpu().numpy()
    assert np.isnan(t[:, 2:]).all() and (t[:, :2] == 0).all() and int(res.rows.sum()) == 0
    assert all(np.isnan(res.as_dict()[k]) for k in ("map", "macro_auroc", "lrap", "ranking_loss", "coverage_error"))


# ------------------------------------------------------------------------------------------------ 2: end to end
N_SAMPLES = 21


class ListLoader:
    def __init__(self, batches):
        self.batches = batches
        self.dataset = self

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


def make_samples(lengths, dv, da, seed=0):
    """Reference-style samples, as tests/test_gpu_inference.py makes them."""
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
def dataset():
    from mmda_amd import DeviceDataset
    lengths = np.random.default_rng(8).integers(1, 10, size=N_SAMPLES)
    return DeviceDataset.from_samples(make_samples(lengths, *MOSEI, seed=2), DEV)


def _solver(train, dev, test, name="rank", n_epoch=1, drop=(), **extra):
    from mmda_amd import make_config, models
    from mmda_amd.solver import Solver
    cfg = orc.default_config(vocab_size=120, learning_rate=1e-3, clip=1.0)
    c = make_config(precision="fp32", device=DEV, n_epoch=n_epoch, name=name, **vars(cfg), **extra)
    for key in drop:                                                 # a configuration from before the option existed
        delattr(c, key)
    m = models.MISA(c)
    m.load_state_dict(orc.synth_params(cfg, 21))
    torch.manual_seed(0)                                             # build() draws the orthogonal recurrent weights
    return Solver(c, c, c, train, dev, test, is_train=True, model=m).build()


def test_solver_rank_equals_the_metrics_of_the_inferred_tables(dataset):
    from mmda_amd import DeviceLoader, failure_prediction, ranking as rk, ranking_metrics
    s = _solver(ListLoader([]), DeviceLoader(dataset, 8), ListLoader([]))
    out = s.rank("dev")
    assert out is s.last_ranking and set(out) == {"scores", "confidence"}
    assert out["scores"].table.is_cuda and out["confidence"].table.is_cuda
    # the truth table from the loop rank() itself runs; infer's rows are in the same order: the same scores, row by row
    batches = list(s._eval_batches(s.dev_data_loader))
    truth = torch.cat([t for _, t in batches], 0).contiguous()
    res = s.infer("dev")
    assert torch.equal(torch.cat([sc for sc, _ in batches], 0), res.scores) and res.scores.unique(dim=0).shape[0] == N_SAMPLES
    want = ranking_metrics(res.scores, truth)
    bits = lambda x: x.contiguous().view(torch.int64)
    assert torch.equal(bits(out["scores"].table), bits(want.table)) and torch.equal(out["scores"].rows, want.rows)
    assert torch.equal(out["scores"].counts, want.counts)
    # the confidence head: tcp against "was the decision correct", device == device and device == yardstick on the read-back table
    correct = ((res.labels > 0) == (truth > 0)).float()
    conf = failure_prediction(res.tcp, correct)
    assert torch.equal(bits(out["confidence"].table), bits(conf.table))
    tcp_h, cor_h = res.tcp.cpu().numpy(), correct.cpu().numpy()
    check_table(conf.table.cpu().numpy(), rk.figures_from_counts(rk.rank_counts_host(tcp_h, cor_h), cor_h, 0.95), 6)
    d = conf.as_dict()
    t = conf.table.cpu().numpy()
    assert same_bits(d["auroc"], t[:6, 2]) and same_bits(d["aupr_success"], t[:6, 3]) and same_bits(d["aupr_error"], t[:6, 4])
    assert same_bits(d["fpr_at_95tpr"], t[:6, 5]) and d["n_correct"] == cor_h.sum(0).tolist()
    with pytest.raises(ValueError, match="mode must be"):
        s.rank("train")


def test_select_by_map_keeps_the_epoch_with_the_higher_dev_map(dataset, tmp_path, monkeypatch):
    from mmda_amd import DeviceLoader
    monkeypatch.chdir(tmp_path)
    gen = torch.Generator().manual_seed(5)
    s = _solver(DeviceLoader(dataset, 8, shuffle=True, generator=gen), DeviceLoader(dataset, 8), DeviceLoader(dataset, 8), name="sel",
                n_epoch=2, select_by="map")
    assert s.train_config.dropout > 0
    snaps, figures, rank = [], [], s.rank

    def spy(mode, **kw):                                              # train() ranks the dev split once per epoch: the weights then
        snaps.append({k: v.detach().clone() for k, v in s.model.state_dict().items()})
        out = rank(mode, **kw)
        figures.append(out["scores"].as_dict()["map"])
        return out

    s.rank = spy
    history = s.train()
    assert len(history) == len(snaps) == 2 and [h["valid_map"] for h in history] == figures
    assert all(0.0 < f <= 1.0 for f in figures)
    best = 1 if figures[1] >= figures[0] else 0
    saved = torch.load(tmp_path / "checkpoints" / "model_sel.std", weights_only=True)
    assert saved.keys() == snaps[best].keys()
    assert all(torch.equal(saved[k].to(DEV), snaps[best][k]) for k in saved)
    assert any(not torch.equal(snaps[0][k], snaps[1][k]) for k in saved)         # the two epochs are two different models
    if figures[0] != figures[1]:
        assert any(not torch.equal(saved[k].to(DEV), snaps[1 - best][k]) for k in saved)


def test_select_by_valid_loss_is_the_loop_without_the_option(dataset, tmp_path, monkeypatch):
    from mmda_amd import DeviceLoader
    runs = {}
    for where, extra in (("with", dict(select_by="valid_loss")), ("without", dict(drop=("select_by",)))):
        os.makedirs(tmp_path / where)
        monkeypatch.chdir(tmp_path / where)
        gen = torch.Generator().manual_seed(5)
        s = _solver(DeviceLoader(dataset, 8, shuffle=True, generator=gen), DeviceLoader(dataset, 8), DeviceLoader(dataset, 8),
                    name="sel", n_epoch=2, **extra)
        assert hasattr(s.train_config, "select_by") == (where == "with")
        history = s.train()
        runs[where] = (history, {f: open(tmp_path / where / "checkpoints" / f, "rb").read() for f in ("model_sel.std", "optim_sel.std")})
        assert not hasattr(s, "last_ranking")                         # valid_loss ranks nothing
    assert runs["with"][0] == runs["without"][0] and all("valid_map" not in h for h in runs["with"][0])
    assert runs["with"][1] == runs["without"][1]
