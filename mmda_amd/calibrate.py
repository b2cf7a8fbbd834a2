"""Threshold calibration: every cut-off of a grid swept on the device in one launch per batch, the best one -- or the best one per
class -- selected on the device, and handed back to ``Solver.eval``.

The model decides ``labels = scores > threshold`` (reference models.py:249): one scalar for all classes, 0.35 by default, a
hyper-parameter that costs the reference a whole run per candidate.  Everything ``get_metrics`` reports is a function of per-class
tp / fp / fn, and ``get_accuracy`` of the rows' (|y & p|, |y | p|) pairs; for a grid ``thr[0..K)`` both follow, at EVERY cut-off, from

  ``hist[c][j][p]``   rows with ``bin(scores[i,c]) == j`` and ``(truth[i,c] > 0) == p``, ``bin(s) = #{k : s > thr[k]}`` (NaN: 0)
  ``pairs[k][a][b]``  rows with ``|y & p| == a`` and ``|y | p| == b`` at cut-off k, where "predicted" is ``s > thr[k]``

which are integers: the sweep is exact and bit-reproducible.  The host functions below (plain numpy, like ``get_metrics``) define the
quantities and are the yardstick of the tests; ``ThresholdSweep`` computes the same on the device (``mmda_calib_accumulate``,
``mmda_calib_select``).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .utils.eval import KEYS, LCM, host_tables, metrics_from_counts

MAX_CLASSES, MAX_GRID = 16, 256
OBJECTIVES = {"f1": 0, "micro_f1": 1, "weighted_f1": 2, "acc": 3}
PER_CLASS_OBJECTIVES = ("f1", "weighted_f1")
EVAL_MODE_OBJECTIVE = {"macro": "f1", "micro": "micro_f1", "weighted": "weighted_f1"}
_COLUMN = {name: KEYS.index(name) for name in OBJECTIVES}


def default_grid():
    """float32(k / 100), k = 1 .. 99; entry 34 is float32(0.35) bit for bit, the reference's own operating point."""
    return (np.arange(1, 100, dtype=np.float64) / 100.0).astype(np.float32)


def check_grid(grid):
    """The grid as a float32 array; ValueError naming the rule it breaks: 1-D, 1 <= K <= 256, finite, strictly increasing as fp32."""
    if isinstance(grid, torch.Tensor):
        grid = grid.detach().cpu().numpy()
    g = np.asarray(grid)
    if g.ndim != 1:
        raise ValueError(f"grid must be 1-D, not of shape {g.shape}")
    if not 1 <= g.shape[0] <= MAX_GRID:
        raise ValueError(f"grid must have 1 <= K <= {MAX_GRID} cut-offs, not {g.shape[0]}")
    g = g.astype(np.float32)
    if not np.isfinite(g).all():
        raise ValueError("grid must be finite")
    if not (np.diff(g) > 0).all():
        raise ValueError("grid must be strictly increasing as fp32")
    return np.ascontiguousarray(g)


def objective_name(objective):
    if objective not in OBJECTIVES:
        raise ValueError(f"objective must be one of {tuple(OBJECTIVES)}, not {objective!r}")
    return objective


def objective_for(eval_mode, per_class):
    """config.eval_mode -> objective: macro -> f1, micro -> micro_f1, weighted -> weighted_f1."""
    if eval_mode not in EVAL_MODE_OBJECTIVE:
        raise ValueError(f"eval_mode must be one of {tuple(EVAL_MODE_OBJECTIVE)}, not {eval_mode!r}")
    return check_objective(EVAL_MODE_OBJECTIVE[eval_mode], per_class)


def check_objective(objective, per_class):
    objective_name(objective)
    if per_class and objective not in PER_CLASS_OBJECTIVES:
        raise ValueError(f"objective {objective!r} is not a combination of per-class figures, so per-class cut-offs cannot be chosen "
                         f"class by class: use per_class=False (or one of {PER_CLASS_OBJECTIVES})")
    return objective


# ---------------------------------------------------------------------------------------------------- host (numpy)
def _bins(scores, grid):
    s = np.asarray(scores, dtype=np.float32)
    b = np.searchsorted(grid, s, side="left")                   # #{k : grid[k] < s}
    b[np.isnan(s)] = 0                                          # a NaN is greater than nothing
    return b


def sweep_counts(scores, truth, grid):
    """(hist (C, K+1, 2), pairs (K, C+1, C+1)), int64, of host arrays scores / truth (N, C)."""
    grid = check_grid(grid)
    s, pos = host_tables(scores, truth, "scores and truth")
    N, C = s.shape
    K = grid.shape[0]
    bins = _bins(s, grid)
    hist = np.zeros((C, K + 1, 2), dtype=np.int64)
    for c in range(C):
        hist[c] = np.bincount(bins[:, c] * 2 + pos[:, c], minlength=2 * (K + 1)).reshape(K + 1, 2)
    pairs = np.zeros((K, C + 1, C + 1), dtype=np.int64)
    for k in range(K):
        pred = bins > k
        a = (pred & pos).sum(1)
        b = (pred | pos).sum(1)
        pairs[k] = np.bincount(a * (C + 1) + b, minlength=(C + 1) ** 2).reshape(C + 1, C + 1)
    return hist, pairs


def counts_from_hist(hist):
    """tp, fp, fn (K, C) int64: tp[k][c] = sum_{j > k} hist[c][j][1], fp likewise from [0], fn = positives - tp."""
    hist = np.asarray(hist, dtype=np.int64)
    suffix = hist[:, ::-1].cumsum(axis=1)[:, ::-1]              # suffix[c][j] = sum_{j' >= j}
    tp = suffix[:, 1:, 1].T
    fp = suffix[:, 1:, 0].T
    fn = suffix[:, 0, 1][None, :] - tp
    return tp, fp, fn


def exact_accuracy(pairs_k, n):
    """mean_i |y_i & p_i| / max(|y_i | p_i|, 1) from one cut-off's pair counts: an integer sum and one division."""
    if n <= 0:
        return 0.0
    C1 = pairs_k.shape[0]
    num = 0
    for a in range(1, C1):
        for b in range(a, C1):
            num += int(pairs_k[a, b]) * a * (LCM // b)
    return num / (LCM * int(n))


def table_from_counts(hist, pairs, n):
    """(K, 10) float64: utils.eval.KEYS with one cut-off k for all classes; acc unrounded, NaN where pairs is None."""
    tp, fp, fn = counts_from_hist(hist)
    K = tp.shape[0]
    out = np.zeros((K, len(KEYS)), dtype=np.float64)
    for k in range(K):
        acc = exact_accuracy(np.asarray(pairs[k]), n) if pairs is not None else float("nan")
        m = metrics_from_counts(tp[k], fp[k], fn[k], acc)
        out[k] = [m[key] for key in KEYS]
    return out


def select_from_counts(hist, pairs, grid, objective="f1", per_class=True):
    """(thr (C,) float32, k (C,) int32): the cut-offs that maximise ``objective``, ties to the lowest k."""
    grid = check_grid(grid)
    check_objective(objective, per_class)
    hist = np.asarray(hist, dtype=np.int64)
    C = hist.shape[0]
    if per_class:
        tp, fp, fn = (x.astype(np.float64) for x in counts_from_hist(hist))
        den = 2 * tp + fp + fn
        f1 = np.where(den > 0, 2 * tp / np.where(den > 0, den, 1.0), 0.0)
        k = f1.argmax(axis=0).astype(np.int32)                  # the first maximum
    else:
        if objective == "acc" and pairs is None:
            raise ValueError("objective 'acc' needs the pair counts")
        n = int(hist[0].sum())
        col = table_from_counts(hist, pairs, n)[:, _COLUMN[objective]]
        k = np.full(C, int(col.argmax()), dtype=np.int32)
    return grid[k], k


# ---------------------------------------------------------------------------------------------------- device
class Thresholds:
    """One cut-off per class: ``values`` (C,) float32 and ``k`` (C,) int32, their indices into ``grid``; on the device when they come
    from ``ThresholdSweep.select``.  ``Solver.eval(mode, thresholds=...)`` decides with them."""

    def __init__(self, values, k, grid=None, objective=None, per_class=None):
        self.values = torch.as_tensor(values, dtype=torch.float32).reshape(-1)
        self.k = torch.as_tensor(k, dtype=torch.int32).reshape(-1)
        if self.values.shape != self.k.shape:
            raise ValueError(f"values and k must have one entry per class each, not {tuple(self.values.shape)} and {tuple(self.k.shape)}")
        self.grid = None if grid is None else np.asarray(grid, dtype=np.float32)
        self.objective, self.per_class = objective, per_class

    def __len__(self):
        return int(self.values.shape[0])

    def to(self, device):
        return Thresholds(self.values.to(device), self.k.to(device), self.grid, self.objective, self.per_class)

    def cpu(self):
        """The same on the host (two small device-to-host copies: the one wait of a calibration besides ``table()``)."""
        return self.to("cpu")

    def save(self, path):
        torch.save(dict(values=self.values.cpu(), k=self.k.cpu(), grid=None if self.grid is None else torch.from_numpy(self.grid.copy()),
                        objective=self.objective, per_class=self.per_class), path)

    @classmethod
    def load(cls, path, device="cpu"):
        d = torch.load(path, map_location="cpu", weights_only=True)
        grid = None if d.get("grid") is None else d["grid"].numpy()
        return cls(d["values"], d["k"], grid, d.get("objective"), d.get("per_class")).to(device)


class ThresholdSweep:
    """``ThresholdSweep(num_classes, grid=None, device=...)``: ``update(scores, truth)`` per batch (one launch, no synchronisation),
    then ``select(objective, per_class)`` -> ``Thresholds`` on the device (one launch, no read-back); ``table()`` and ``counts()`` read
    back once each."""

    def __init__(self, num_classes, grid=None, device="cuda", pairs=True):
        self.C = int(num_classes)
        if not 1 <= self.C <= MAX_CLASSES:
            raise ValueError(f"num_classes must be in 1 .. {MAX_CLASSES}, not {num_classes}")
        self.grid = check_grid(default_grid() if grid is None else grid)
        self.K = int(self.grid.shape[0])
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.MMDAError(f"ThresholdSweep counts on the GPU only (the HIP path has no CPU fallback), not on {self.device}")
        self._lib = _lib.load()
        self.grid_dev = torch.from_numpy(self.grid).to(self.device)
        nh, npairs = self.C * (self.K + 1) * 2, (self.K * (self.C + 1) ** 2 if pairs else 0)
        self._counts = torch.zeros(nh + npairs, dtype=torch.int64, device=self.device)      # one buffer: counts() is one read-back
        self._nh = nh
        self._pairs_ptr = self._counts.data_ptr() + 8 * nh if pairs else None
        self._table = torch.empty(self.K, len(KEYS), dtype=torch.float64, device=self.device)

    def reset(self):
        self._counts.zero_()

    def _accumulate(self, s, t):
        if s.dim() != 2 or s.shape[1] != self.C or t.shape != s.shape:
            raise ValueError(f"scores and truth must both be (N, {self.C}), not {tuple(s.shape)} and {tuple(t.shape)}")
        if s.shape[0] == 0:                                          # an empty batch (its tensors have no storage to point at)
            return
        _lib.check(self._lib.mmda_calib_accumulate(s.data_ptr(), t.data_ptr(), s.shape[0], self.C, self.grid_dev.data_ptr(), self.K,
                                                   self._counts.data_ptr(), self._pairs_ptr, _lib.stream_ptr()),
                   "mmda_calib_accumulate")

    def update(self, scores, truth):
        """scores, truth: (N, C) on the device; no synchronisation."""
        self._accumulate(*_lib.device_tables(scores, truth, "ThresholdSweep.update"))      # (_accumulate checks the shapes)

    def update_result(self, result, truth):
        """The ``scores`` table of an ``InferenceResult`` against ``truth`` (n, C), rows in the result's order."""
        if getattr(result, "scores", None) is None:
            raise ValueError("the InferenceResult has no scores table: collect the 'scores' field")
        self.update(result.scores, truth)

    def _select(self, objective, per_class, out_thr, out_k):
        _lib.check(self._lib.mmda_calib_select(self._counts.data_ptr(), self._pairs_ptr, self.C, self.K, self.grid_dev.data_ptr(),
                                               OBJECTIVES[objective], int(bool(per_class)), out_thr.data_ptr(), out_k.data_ptr(),
                                               self._table.data_ptr(), _lib.stream_ptr()), "mmda_calib_select")

    def select(self, objective="f1", per_class=True):
        """``Thresholds`` on the device: no read-back."""
        check_objective(objective, per_class)
        if objective == "acc" and self._pairs_ptr is None:
            raise ValueError("objective 'acc' needs the pair counts: ThresholdSweep(..., pairs=True)")
        values = torch.empty(self.C, dtype=torch.float32, device=self.device)
        k = torch.empty(self.C, dtype=torch.int32, device=self.device)
        self._select(objective, per_class, values, k)
        return Thresholds(values, k, self.grid, objective, bool(per_class))

    def table(self):
        """(K, 10) float64 on the host, columns ``utils.eval.KEYS``, one cut-off for all classes per row: one read-back."""
        self.select("f1", per_class=False)
        return self._table.cpu().numpy()

    def counts(self):
        """(hist (C, K+1, 2), pairs (K, C+1, C+1) or None) as int64 on the host: one read-back."""
        flat = self._counts.cpu().numpy()
        hist = flat[:self._nh].reshape(self.C, self.K + 1, 2)
        pairs = flat[self._nh:].reshape(self.K, self.C + 1, self.C + 1) if self._pairs_ptr is not None else None
        return hist, pairs


def confidence_curve(tcp, correct, cutoffs):
    """ConfidNet's ``tcp`` (n, C) against ``correct = (labels == truth)`` (n, C), both on the device, by the sweep's kernel: per class
    and cut-off, (kept, kept_correct) -- how many decisions have ``tcp > cutoffs[k]`` and how many of those are correct -- as two (C, K)
    int64 device tensors (suffix sums of the histogram and nothing more; no read-back)."""
    t, c = _lib.device_tables(tcp, correct, "confidence_curve")
    sweep = ThresholdSweep(t.shape[1] if t.dim() == 2 else 0, cutoffs, t.device, pairs=False)
    sweep._accumulate(t, c)
    hist = sweep._counts.view(sweep.C, sweep.K + 1, 2)
    suffix = hist.flip(1).cumsum(1).flip(1)[:, 1:]              # [c][k] = sum_{j > k}
    return suffix.sum(2), suffix[:, :, 1].contiguous()
