#!/usr/bin/env python3
"""Generate tests/golden/calib/calib_sweep.npz: scores, truth, the default grid of cut-offs and, for every cut-off k, the REFERENCE's own
src/utils/eval.py get_metrics(truth, scores > grid[k]).  Run in the build container only; the file is loaded by path (the reference's
`utils` package __init__ is not needed).

Usage:  python tests/golden/gen_golden_calib.py
"""
import importlib.util
import os
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
spec = importlib.util.spec_from_file_location("ref_eval", "/root/reference/src/utils/eval.py")
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)

KEYS = ["acc", "f1", "precision", "recall", "micro_f1", "micro_precision", "micro_recall", "weighted_f1", "weighted_precision",
        "weighted_recall"]
N, C = 301, 6
grid = (np.arange(1, 100, dtype=np.float64) / 100.0).astype(np.float32)
rng = np.random.default_rng(23)

truth = (rng.random((N, C)) < np.array([0.5, 0.3, 0.2, 0.15, 0.1, 0.05])).astype(np.float32)      # imbalanced, like MOSEI's emotions
scores = np.clip(0.5 * truth + rng.normal(0.3, 0.2, (N, C)), 0.0, 1.0).astype(np.float32)        # informative scores
scores[:40] = grid[rng.integers(0, grid.shape[0], (40, C))]       # exactly on grid values: the comparison is a strict >
scores[40] = np.array([0.0, 1.0, np.nan, 0.35, 0.35, 1.0], dtype=np.float32)
truth[40] = np.array([1, 1, 0, 1, 0, 0], dtype=np.float32)
truth[:, 2] = 0.0                                                 # a class with no positives
truth[50:55] = 0.0                                                # all-negative rows
scores[:, 4] = np.minimum(scores[:, 4], np.float32(0.6))          # a class that is never predicted at high cut-offs

metrics = np.zeros((grid.shape[0], len(KEYS)), dtype=np.float64)
with warnings.catch_warnings():
    warnings.simplefilter("ignore")                               # sklearn's zero-division warnings: the value (0.0) is what is pinned
    for k, t in enumerate(grid):
        pred = (scores > t).astype(np.float32)                    # NaN > t is False
        m = ref.get_metrics(truth, pred)
        metrics[k] = [m[key] for key in KEYS]

np.savez_compressed(os.path.join(HERE, "calib", "calib_sweep.npz"), scores=scores, truth=truth, grid=grid, metrics=metrics, keys=np.array(KEYS))
print("wrote", grid.shape[0], "cut-offs")
