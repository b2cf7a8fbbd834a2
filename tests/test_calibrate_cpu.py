"""CPU: threshold calibration's host functions (mmda_amd/calibrate.py: sweep_counts, table_from_counts, select_from_counts) against the
reference's own get_metrics at every cut-off (tests/golden/calib/calib_sweep.npz, written by tests/golden/gen_golden_calib.py) and against
a brute-force arg max over the project's get_metrics; grid validation, configuration, the Thresholds file and the native entry
points' argument checks (no launch: no GPU here)."""
import os
import sys

import numpy as np
import pytest
import torch

from mmda_amd import _lib, calibrate as cal
from mmda_amd.utils.eval import KEYS, get_metrics

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden():
    d = np.load(os.path.join(HERE, "golden", "calib", "calib_sweep.npz"))
    return {k: d[k] for k in d.files}


@pytest.fixture(scope="module")
def informative():
    """scores = clip(0.5 truth + noise): a cut-off matters; class 2 has no positives.  With the brute-force figures of get_metrics at
    every cut-off (per-class F1 restated from the same tp / fp / fn), computed once."""
    rng = np.random.default_rng(5)
    truth = (rng.random((257, 6)) < np.array([0.5, 0.3, 0.0, 0.2, 0.1, 0.4])).astype(np.float32)
    scores = np.clip(0.5 * truth + rng.normal(0.3, 0.2, truth.shape), 0, 1).astype(np.float32)
    grid = cal.default_grid()
    brute = np.array([[get_metrics(truth, scores > t)[k] for k in KEYS] for t in grid])
    f1c = np.zeros((grid.shape[0], 6))
    for k, t in enumerate(grid):
        p, y = scores > t, truth > 0
        tp, fp, fn = (p & y).sum(0), (p & ~y).sum(0), (~p & y).sum(0)
        den = (2 * tp + fp + fn).astype(np.float64)
        f1c[k] = np.where(den > 0, 2 * tp / np.where(den > 0, den, 1), 0.0)
    return truth, scores, grid, brute, f1c


def test_default_grid_holds_the_reference_threshold_bit_for_bit():
    g = cal.default_grid()
    assert g.dtype == np.float32 and g.shape == (99,) and (np.diff(g) > 0).all()
    assert g[34].tobytes() == np.float32(0.35).tobytes()


def test_sweep_table_equals_the_reference_at_every_cutoff(golden):
    hist, pairs = cal.sweep_counts(golden["scores"], golden["truth"], golden["grid"])
    n, C = golden["scores"].shape
    assert hist.shape == (C, 100, 2) and pairs.shape == (99, C + 1, C + 1)
    assert (hist.sum(axis=(1, 2)) == n).all() and (pairs.sum(axis=(1, 2)) == n).all()
    assert list(golden["keys"]) == KEYS
    table = cal.table_from_counts(hist, pairs, n)
    want = golden["metrics"]
    assert np.abs(table[:, 1:] - want[:, 1:]).max() <= 1e-12
    # the reference adds the rows' ratios one by one in floating point and rounds to 4 places; the sweep's acc is exact and unrounded
    assert np.abs(np.round(table[:, 0], 4) - want[:, 0]).max() <= 1.0001e-4


def test_sweep_counts_edge_values(golden):
    """a score ON a grid value is not above it; NaN is above nothing; 0 and 1 fall in the first and the last bin"""
    grid = golden["grid"]
    s = np.array([[0.0, 1.0, np.nan, 0.35, 0.35, 1.0]], dtype=np.float32)
    t = np.array([[1, 1, 0, 1, 0, 0]], dtype=np.float32)
    hist, pairs = cal.sweep_counts(s, t, grid)
    bins = [int(np.argwhere(hist[c].sum(1))[0, 0]) for c in range(6)]
    assert bins == [0, 99, 0, 34, 34, 99]                       # 0.35 == grid[34]: above grid[0 .. 33] only
    # positives: columns 0, 1, 3.  At 0.34 columns 1, 3, 4, 5 are predicted (2 of them positive, union of 5); at 0.35 only 1 and 5
    assert pairs[33, 2, 5] == 1 and pairs[34, 1, 4] == 1


def test_without_pairs_the_accuracy_column_is_nan(golden):
    hist, _ = cal.sweep_counts(golden["scores"], golden["truth"], golden["grid"])
    table = cal.table_from_counts(hist, None, 301)
    assert np.isnan(table[:, 0]).all() and np.abs(table[:, 1:] - golden["metrics"][:, 1:]).max() <= 1e-12


def test_select_equals_brute_force(informative):
    truth, scores, grid, brute, f1c = informative
    hist, pairs = cal.sweep_counts(scores, truth, grid)
    # per class: F1 is one IEEE division of integers, so the arg max is exact; the same k under both per-class objectives
    for objective in ("f1", "weighted_f1"):
        thr, k = cal.select_from_counts(hist, pairs, grid, objective, per_class=True)
        assert k.dtype == np.int32 and thr.dtype == np.float32
        assert np.array_equal(k, f1c.argmax(0)) and np.array_equal(thr, grid[k])
    assert k[2] == 0                                            # no positives: F1 is 0 everywhere and the tie goes to the lowest k
    thr, k = cal.select_from_counts(hist, pairs, grid, "micro_f1", per_class=False)
    assert (k == brute[:, KEYS.index("micro_f1")].argmax()).all() and np.array_equal(thr, grid[k])
    for objective in ("f1", "weighted_f1", "acc"):
        _, k = cal.select_from_counts(hist, pairs, grid, objective, per_class=False)
        assert (k == k[0]).all()
        col = KEYS.index(objective)
        table = cal.table_from_counts(hist, pairs, truth.shape[0])
        if objective == "acc":                                  # brute force rounds acc to 4 places: compare what the sweep maximises
            assert table[k[0], col] == table[:, col].max() and abs(round(table[k[0], col], 4) - brute[:, col].max()) <= 1.0001e-4
        else:
            assert abs(brute[k[0], col] - brute[:, col].max()) <= 1e-12
    # macro-F1 of the per-class choice is at least that of any single cut-off
    _, kc = cal.select_from_counts(hist, pairs, grid, "f1", per_class=True)
    assert f1c[kc, np.arange(6)].mean() >= brute[:, KEYS.index("f1")].max() - 1e-15


def test_ties_go_to_the_lowest_cutoff():
    grid = np.array([0.2, 0.4, 0.6, 0.8], dtype=np.float32)
    scores = np.array([[0.9, 0.1], [0.1, 0.9], [0.9, 0.5]], dtype=np.float32)
    truth = np.array([[1, 0], [0, 0], [1, 0]], dtype=np.float32)
    hist, pairs = cal.sweep_counts(scores, truth, grid)
    thr, k = cal.select_from_counts(hist, pairs, grid, "f1", per_class=True)
    assert k.tolist() == [0, 0]                                 # class 0: F1 = 1 at every cut-off; class 1: F1 = 0 at every cut-off
    # one cut-off for both: macro-F1 is 1/2 and weighted-F1 (class 1 has no support) is 1 at every cut-off -> k = 0; class 1's false
    # positive at 0.5 is gone from 0.6 on, so micro-F1 (4/5) and acc (2/3) are best at k = 2 AND k = 3 -> k = 2
    for objective, want in (("f1", 0), ("micro_f1", 2), ("weighted_f1", 0), ("acc", 2)):
        _, k = cal.select_from_counts(hist, pairs, grid, objective, per_class=False)
        assert k.tolist() == [want, want], objective


def test_grid_validation_names_the_rule():
    with pytest.raises(ValueError, match="1-D"):
        cal.check_grid(np.zeros((2, 2)))
    with pytest.raises(ValueError, match="1 <= K <= 256"):
        cal.check_grid(np.zeros((0,)))
    with pytest.raises(ValueError, match="1 <= K <= 256"):
        cal.check_grid(np.linspace(0, 1, 257))
    with pytest.raises(ValueError, match="finite"):
        cal.check_grid([0.1, np.inf])
    with pytest.raises(ValueError, match="strictly increasing"):
        cal.check_grid([0.1, 0.1])
    with pytest.raises(ValueError, match="strictly increasing as fp32"):
        cal.check_grid(np.array([0.5, 0.5 + 1e-12]))            # distinct doubles, one float
    assert cal.check_grid(np.linspace(0, 1, 256)).dtype == np.float32


def test_objectives():
    assert cal.objective_for("macro", True) == "f1" and cal.objective_for("weighted", True) == "weighted_f1"
    assert cal.objective_for("micro", False) == "micro_f1"
    with pytest.raises(ValueError, match="per_class=False"):
        cal.objective_for("micro", True)
    with pytest.raises(ValueError, match="per_class=False"):
        cal.check_objective("acc", True)
    with pytest.raises(ValueError, match="objective"):
        cal.check_objective("accuracy", False)
    with pytest.raises(ValueError, match="eval_mode"):
        cal.objective_for("samples", False)


def test_calibrate_flag_parses_and_defaults_to_none(monkeypatch):
    from mmda_amd import get_config, make_config
    assert make_config().calibrate == "none"
    monkeypatch.setattr(sys, "argv", ["prog"])
    assert get_config().calibrate == "none"
    monkeypatch.setattr(sys, "argv", ["prog", "--calibrate", "per_class"])
    assert get_config().calibrate == "per_class"
    monkeypatch.setattr(sys, "argv", ["prog", "--calibrate", "sometimes"])
    with pytest.raises(SystemExit):
        get_config()


def test_solver_refusals_come_before_any_device_work(monkeypatch):
    from types import SimpleNamespace
    from mmda_amd import make_config
    from mmda_amd.solver import Solver
    from mmda_amd.utils import convert
    monkeypatch.setattr(convert, "_DEVICE", convert._DEVICE)    # a Solver sets the process-wide device: put it back afterwards

    def solver(**kw):
        c = make_config(device="cpu", vocab_size=32, **kw)
        return Solver(c, c, c, [], SimpleNamespace(shard=(0, 2)), [], is_train=False, model=None)

    s = solver(eval_mode="micro")
    with pytest.raises(ValueError, match="per_class=False"):     # eval_mode = micro names no per-class objective
        s.calibrate("dev")
    with pytest.raises(ValueError, match="mode must be"):
        s.calibrate("train", per_class=False)
    assert s._calibrate_after_training(False) is None            # calibrate = "none": nothing happens
    s = solver(calibrate="per_class")
    s.dp = SimpleNamespace(rank=1)                               # under a process group, a sharded dev loader is refused by name
    with pytest.raises(ValueError, match="must not be sharded"):
        s._calibrate_after_training(False)
    s = solver(calibrate="sometimes")
    with pytest.raises(ValueError, match="config.calibrate"):
        s._calibrate_after_training(False)


def test_thresholds_round_trip(tmp_path):
    thr = cal.Thresholds(torch.tensor([0.35, 0.2, 0.01, 0.5, 0.6, 0.99]), torch.tensor([34, 19, 0, 49, 59, 98]), cal.default_grid(),
                         "f1", True)
    path = tmp_path / "thresholds.pt"
    thr.save(path)
    got = cal.Thresholds.load(path, "cpu")
    assert torch.equal(got.values, thr.values) and got.values.dtype == torch.float32
    assert torch.equal(got.k, thr.k) and got.k.dtype == torch.int32
    assert np.array_equal(got.grid, thr.grid) and got.objective == "f1" and got.per_class is True and len(got) == 6
    assert torch.equal(thr.cpu().values, thr.values)
    with pytest.raises(ValueError, match="one entry per class"):
        cal.Thresholds(torch.zeros(6), torch.zeros(5))


def test_sweep_refuses_the_cpu_by_name():
    with pytest.raises(_lib.MMDAError, match="ThresholdSweep"):
        cal.ThresholdSweep(6, device="cpu")
    with pytest.raises(_lib.MMDAError, match="confidence_curve"):
        cal.confidence_curve(torch.zeros(4, 6), torch.zeros(4, 6), [0.5])


def test_native_argument_checks_without_gpu():
    """MMDA_EINVAL (-1) before any launch; N == 0 is MMDA_OK with no launch.  Pointers are never dereferenced on the host."""
    lib = _lib.load()
    p = 4096                                                    # a non-NULL, 8-byte aligned stand-in: never read
    assert lib.mmda_calib_accumulate(None, None, 1, 6, None, 99, None, None, None) == -1
    for hole in range(4):
        args = [p, p, p, p]
        args[hole] = None
        assert lib.mmda_calib_accumulate(args[0], args[1], 1, 6, args[2], 99, args[3], None, None) == -1
    assert lib.mmda_calib_accumulate(p, p, 1, 6, p, 0, p, p, None) == -1
    assert lib.mmda_calib_accumulate(p, p, 1, 6, p, 257, p, p, None) == -1
    assert lib.mmda_calib_accumulate(p, p, 1, 17, p, 99, p, p, None) == -1
    assert lib.mmda_calib_accumulate(p, p, 1, 0, p, 99, p, p, None) == -1
    assert lib.mmda_calib_accumulate(p, p, -1, 6, p, 99, p, p, None) == -1
    assert lib.mmda_calib_accumulate(p, p, 0, 6, p, 99, p, p, None) == 0
    assert lib.mmda_calib_accumulate(p, p, 0, 16, p, 256, p, None, None) == 0
    # select: per-class needs a per-class objective; acc needs the pair counts
    assert lib.mmda_calib_select(None, None, 6, 99, p, 0, 0, p, p, None, None) == -1
    assert lib.mmda_calib_select(p, p, 6, 99, p, 1, 1, p, p, None, None) == -1
    assert lib.mmda_calib_select(p, p, 6, 99, p, 3, 1, p, p, None, None) == -1
    assert lib.mmda_calib_select(p, None, 6, 99, p, 3, 0, p, p, None, None) == -1
    assert lib.mmda_calib_select(p, p, 6, 99, p, 4, 0, p, p, None, None) == -1
    assert lib.mmda_calib_select(p, p, 6, 257, p, 0, 0, p, p, None, None) == -1
    assert lib.mmda_eval_accumulate_thr(p, p, 4, 6, None, None, p, None) == -1
    assert lib.mmda_eval_accumulate_thr(p, p, 4, 17, p, None, p, None) == -1
    assert lib.mmda_eval_accumulate_thr(p, p, 0, 6, p, None, p, None) == 0
