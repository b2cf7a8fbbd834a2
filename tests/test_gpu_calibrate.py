"""GPU: threshold calibration -- ``mmda_calib_accumulate`` against the host ``sweep_counts`` (integer equality), ``mmda_calib_select``
against ``select_from_counts`` / ``table_from_counts``, ``mmda_eval_accumulate_thr`` against ``DeviceEval`` over torch-made labels,
and ``Solver.calibrate`` / ``Solver.eval(thresholds=...)`` end to end on the tiny model of tests/test_gpu_inference.py.

Bounds: counts are integers and compared for equality.  Per-class F1 and micro-F1 are single IEEE divisions of integers, so their arg
max is compared exactly; macro / weighted / acc add several such terms (the host adds them in numpy's order, the kernel in class
order), so the chosen cut-off must attain the host's maximum within 1e-12, the bound of the table itself."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import misa_oracle as orc

DEV = "cuda:0"
MOSEI = (35, 74)
SHAPES = [(1, 6, 1), (37, 6, 99), (300, 1, 7), (301, 6, 99), (1000, 16, 256), (70001, 6, 99)]


def make_case(N, C, K, seed=0):
    """The value classes of tests/golden/calib/calib_sweep.npz at any shape: informative scores, rows exactly on grid values, the row
    [0, 1, NaN, 0.35, 0.35, 1] (as far as C reaches), a class with no positives, all-negative rows, a class capped at 0.6."""
    from mmda_amd import calibrate as cal
    rng = np.random.default_rng(seed + 1000 * K + C)
    grid = cal.default_grid() if K == 99 else (np.arange(1, K + 1, dtype=np.float64) / (K + 1)).astype(np.float32)
    truth = (rng.random((N, C)) < np.linspace(0.5, 0.05, C)).astype(np.float32)
    scores = np.clip(0.5 * truth + rng.normal(0.3, 0.2, (N, C)), 0.0, 1.0).astype(np.float32)
    on = min(40, N // 2)
    scores[:on] = grid[rng.integers(0, K, (on, C))]
    special = np.array([0.0, 1.0, np.nan, 0.35, 0.35, 1.0], dtype=np.float32)
    scores[N // 2, :min(C, 6)] = special[:C]
    if C > 2:
        truth[:, 2] = 0.0
    truth[N // 3:N // 3 + 5] = 0.0
    scores[:, C - 1] = np.minimum(scores[:, C - 1], np.float32(0.6))
    return scores, truth, grid


@pytest.fixture(scope="module")
def cases():
    """Per shape: host inputs, the host counts (the yardstick; computed once, never written) and the device copies."""
    from mmda_amd import calibrate as cal
    out = {}
    for shape in SHAPES:
        s, t, g = make_case(*shape)
        hist, pairs = cal.sweep_counts(s, t, g)
        out[shape] = dict(scores=s, truth=t, grid=g, hist=hist, pairs=pairs, s_dev=torch.from_numpy(s).to(DEV),
                          t_dev=torch.from_numpy(t).to(DEV))
    return out


def _sweep(case, C, pairs=True):
    from mmda_amd import ThresholdSweep
    return ThresholdSweep(C, case["grid"], DEV, pairs=pairs)


# ------------------------------------------------------------------------------------------------ 1: the counts
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_counts_equal_the_host_sweep(cases, shape):
    N, C, K = shape
    case = cases[shape]
    sw = _sweep(case, C)
    sw.update(case["s_dev"], case["t_dev"])
    hist, pairs = sw.counts()
    assert hist.dtype == np.int64 and np.array_equal(hist, case["hist"])
    assert np.array_equal(pairs, case["pairs"])
    # without the pair counts: the same histogram
    only = _sweep(case, C, pairs=False)
    only.update(case["s_dev"], case["t_dev"])
    h2, p2 = only.counts()
    assert p2 is None and np.array_equal(h2, case["hist"])
    # two calls over halves add up to one call over the whole; a second run gives the same bits
    halves = _sweep(case, C)
    halves.update(case["s_dev"][:N // 2], case["t_dev"][:N // 2])
    halves.update(case["s_dev"][N // 2:], case["t_dev"][N // 2:])
    again = _sweep(case, C)
    again.update(case["s_dev"], case["t_dev"])
    assert torch.equal(halves._counts, sw._counts) and torch.equal(again._counts, sw._counts)


def test_update_refuses_host_tensors_and_wrong_shapes(cases):
    from mmda_amd import _lib
    case = cases[(37, 6, 99)]
    sw = _sweep(case, 6)
    with pytest.raises(_lib.MMDAError, match="ThresholdSweep.update"):
        sw.update(torch.from_numpy(case["scores"]), case["t_dev"])
    with pytest.raises(ValueError, match=r"\(N, 6\)"):
        sw.update(case["s_dev"][:, :5], case["t_dev"][:, :5])
    assert int(sw._counts.sum()) == 0


# ------------------------------------------------------------------------------------------------ 2: the selection
@pytest.mark.parametrize("shape", [(37, 6, 99), (301, 6, 99), (1000, 16, 256), (300, 1, 7)], ids=lambda s: "x".join(map(str, s)))
def test_select_and_table_equal_the_host(cases, shape):
    from mmda_amd import calibrate as cal
    from mmda_amd.utils.eval import KEYS
    N, C, K = shape
    case = cases[shape]
    sw = _sweep(case, C)
    sw.update(case["s_dev"], case["t_dev"])
    want_table = cal.table_from_counts(case["hist"], case["pairs"], N)
    table = sw.table()
    assert table.shape == (K, 10) and np.abs(table - want_table).max() <= 1e-12
    for objective in ("f1", "weighted_f1"):                     # exact: each class's F1 is one division of integers
        thr = sw.select(objective, per_class=True)
        want_thr, want_k = cal.select_from_counts(case["hist"], case["pairs"], case["grid"], objective, True)
        assert thr.values.is_cuda and thr.k.dtype == torch.int32
        assert np.array_equal(thr.k.cpu().numpy(), want_k) and np.array_equal(thr.values.cpu().numpy(), want_thr)
    thr = sw.select("micro_f1", per_class=False)                # exact: one division of integers
    want_thr, want_k = cal.select_from_counts(case["hist"], case["pairs"], case["grid"], "micro_f1", False)
    assert np.array_equal(thr.k.cpu().numpy(), want_k) and np.array_equal(thr.values.cpu().numpy(), want_thr)
    for objective in ("f1", "weighted_f1", "acc"):              # sums of several terms: the chosen cut-off attains the host's maximum
        thr = sw.select(objective, per_class=False)
        k = thr.k.cpu().numpy()
        col = want_table[:, KEYS.index(objective)]
        assert (k == k[0]).all() and abs(col[k[0]] - col.max()) <= 1e-12, objective
        assert np.array_equal(thr.values.cpu().numpy(), case["grid"][k])
        first = int(np.argmax(table[:, KEYS.index(objective)]))  # ties go to the lowest k of the kernel's own column
        assert k[0] == first


def test_select_without_pairs_and_refusals(cases):
    from mmda_amd import _lib, calibrate as cal
    case = cases[(301, 6, 99)]
    sw = _sweep(case, 6, pairs=False)
    sw.update(case["s_dev"], case["t_dev"])
    table = sw.table()
    want = cal.table_from_counts(case["hist"], None, 301)
    assert np.isnan(table[:, 0]).all() and np.abs(table[:, 1:] - want[:, 1:]).max() <= 1e-12
    lib = _lib.load()
    out_t, out_k = torch.zeros(6, device=DEV), torch.zeros(6, dtype=torch.int32, device=DEV)
    full = _sweep(case, 6)
    args = lambda s, objective, per_class: (s._counts.data_ptr(), s._pairs_ptr, 6, 99, s.grid_dev.data_ptr(), objective, per_class,
                                            out_t.data_ptr(), out_k.data_ptr(), None, _lib.stream_ptr())
    assert lib.mmda_calib_select(*args(full, 1, 1)) == -1       # micro-F1 per class
    assert lib.mmda_calib_select(*args(full, 3, 1)) == -1       # acc per class
    assert lib.mmda_calib_select(*args(sw, 3, 0)) == -1         # acc without the pair counts
    assert lib.mmda_calib_select(*args(sw, 0, 1)) == 0
    with pytest.raises(ValueError, match="per_class=False"):
        full.select("micro_f1", per_class=True)
    with pytest.raises(ValueError, match="pair counts"):
        sw.select("acc", per_class=False)


# ------------------------------------------------------------------------------------------------ 3: evaluation from scores
@pytest.mark.parametrize("N", [1, 37, 301])
def test_eval_accumulate_thr_equals_device_eval_over_torch_labels(cases, N):
    from mmda_amd import _lib
    from mmda_amd.utils.eval import DeviceEval
    case = cases[(301, 6, 99)]
    s, t = case["s_dev"][:N].contiguous(), case["t_dev"][:N].contiguous()
    thr = torch.tensor([0.35, 0.2, 0.01, 0.5, 0.6, 0.99], device=DEV)
    want_labels = (s > thr).float()
    ref = DeviceEval(6, DEV)
    ref.update(want_labels, t)
    got = DeviceEval(6, DEV)
    labels = torch.full_like(s, -1.0)
    lib = _lib.load()
    for out in (labels.data_ptr(), None):                       # with and without labels_out: two batches of the same rows
        _lib.check(lib.mmda_eval_accumulate_thr(s.data_ptr(), t.data_ptr(), N, 6, thr.data_ptr(), out, got.state.data_ptr(),
                                                _lib.stream_ptr()), "mmda_eval_accumulate_thr")
    ref.update(want_labels, t)
    a, b = got.state.cpu().numpy(), ref.state.cpu().numpy()
    assert torch.equal(labels, want_labels)
    assert np.array_equal(a[:18], b[:18]) and a[19] == b[19] == 2 * N
    assert abs(a[18] - b[18]) <= 1e-9


def test_confidence_curve_counts(cases):
    from mmda_amd import confidence_curve
    case = cases[(301, 6, 99)]
    tcp = torch.nan_to_num(case["s_dev"], nan=0.0)
    correct = case["t_dev"]                                     # any 0/1 table
    cut = np.array([0.25, 0.5, 0.75], dtype=np.float32)
    kept, kept_correct = confidence_curve(tcp, correct, cut)
    assert kept.shape == kept_correct.shape == (6, 3) and kept.is_cuda
    for k, c in enumerate(cut):
        keep = tcp > float(c)
        assert torch.equal(kept[:, k], keep.sum(0)) and torch.equal(kept_correct[:, k], (keep & (correct > 0)).sum(0))


# ------------------------------------------------------------------------------------------------ 4: end to end
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


CUT = ("trnn1", "trnn2", "vrnn1", "vrnn2", "arnn1", "arnn2", "tlayer_norm", "vlayer_norm", "alayer_norm", "embed")


def _solver(train, dev, test, precision, name="calibrate", freeze=(), **extra):
    from mmda_amd import make_config, models
    from mmda_amd.solver import Solver
    cfg = orc.default_config(vocab_size=120, learning_rate=1e-3, clip=1.0)
    c = make_config(precision=precision, device=DEV, n_epoch=1, name=name, **vars(cfg), **extra)
    m = models.MISA(c)
    m.load_state_dict(orc.synth_params(cfg, 21))
    if freeze:
        m.freeze(*freeze)
    torch.manual_seed(0)                                             # build() draws the orthogonal recurrent weights
    return Solver(c, c, c, train, dev, test, is_train=True, model=m).build()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_calibrated_eval_equals_host_metrics_of_the_inferred_scores(dataset, precision):
    from mmda_amd import DeviceLoader
    from mmda_amd.utils.eval import KEYS, get_metrics
    s = _solver(ListLoader([]), DeviceLoader(dataset, 8), ListLoader([]), precision)
    thr = s.calibrate("dev")
    assert thr is s.thresholds and thr.values.is_cuda and thr.per_class and thr.objective == "f1"       # eval_mode = macro
    table = s.last_calibration["table"]
    loss, acc, y_pred, y_true = s.eval("dev", thresholds=thr)
    got = dict(s.last_eval_metrics)
    res = s.infer("dev")                                             # the loader's own batches and row order, as eval's
    scores = res.scores.cpu().numpy()
    want_pred = scores > thr.cpu().values.numpy()
    assert np.array_equal(y_pred > 0, want_pred)
    want = get_metrics(y_true, want_pred)
    for k in KEYS:
        assert abs(got[k] - want[k]) <= 1e-12, k
    assert acc == want["acc"]
    # the sweep's row at float32(0.35) is what plain eval reports: both count the same comparisons
    plain_loss, plain_acc, _, _ = s.eval("dev")
    plain = dict(s.last_eval_metrics)
    at = int(np.flatnonzero(s.last_calibration["grid"] == np.float32(0.35))[0])
    assert at == 34
    for i, k in enumerate(KEYS[1:], start=1):
        assert abs(table[at, i] - plain[k]) <= 1e-12, k
    assert round(table[at, 0], 4) == plain["acc"] == plain_acc and abs(plain_loss - loss) <= 1e-6 * abs(loss)
    # 0.35 is on the grid, so per-class cut-offs cannot do worse in macro-F1 on the split they were chosen on
    assert got["f1"] >= plain["f1"]
    with pytest.raises(ValueError, match="per_class=False"):
        s.calibrate("dev", objective="micro_f1")
    glob = s.calibrate("dev", objective="micro_f1", per_class=False)
    assert len(set(glob.k.tolist())) == 1 and s.thresholds is glob


def test_encoded_dev_loader_gives_the_same_thresholds(dataset):
    from mmda_amd import DeviceLoader, EncodedLoader
    s = _solver(ListLoader([]), DeviceLoader(dataset, 8), ListLoader([]), "fp32", freeze=CUT)   # the cache needs the encoder cut
    want = s.calibrate("dev")
    want_table = s.last_calibration["table"]
    s.dev_data_loader = EncodedLoader(s.encode("dev"), 8)
    got = s.calibrate("dev")
    assert torch.equal(got.k, want.k) and torch.equal(got.values, want.values)
    assert np.array_equal(s.last_calibration["table"], want_table)


def test_train_with_calibrate_per_class_saves_and_uses_the_thresholds(dataset, tmp_path, monkeypatch):
    from mmda_amd import DeviceLoader, Thresholds
    from mmda_amd.utils.eval import KEYS
    monkeypatch.chdir(tmp_path)
    gen = torch.Generator().manual_seed(5)
    s = _solver(DeviceLoader(dataset, 8, shuffle=True, generator=gen), DeviceLoader(dataset, 8), DeviceLoader(dataset, 8), "fp32",
                name="cal", calibrate="per_class")
    s.train()
    final = dict(s.last_eval_metrics)                                # of train()'s last act: the test pass under the thresholds
    path = tmp_path / "checkpoints" / "thresholds_cal.pt"
    assert path.exists()
    loaded = Thresholds.load(path, DEV)
    assert torch.equal(loaded.values, s.thresholds.values) and loaded.per_class is True
    s.eval("test", thresholds=loaded)
    for k in KEYS:
        assert s.last_eval_metrics[k] == final[k], k
    # calibrate = "none" writes nothing and decides with config.threshold
    plain = _solver(DeviceLoader(dataset, 8), DeviceLoader(dataset, 8), DeviceLoader(dataset, 8), "fp32", name="plain")
    plain.train()
    assert not (tmp_path / "checkpoints" / "thresholds_plain.pt").exists() and not hasattr(plain, "thresholds")
