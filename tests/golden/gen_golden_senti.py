#!/usr/bin/env python3
"""Generate tests/golden/senti/senti_cases.npz from the REFERENCE's own src/utils/eval_metrics.py (eval_mosei_senti), run in the build
container only (it needs scikit-learn, which the reference's function calls).  The file is loaded by path, as gen_golden_eval.py
loads eval.py.  Inputs are float32 values -- what the device collector reads -- handed to the reference as float64, so every figure is
the reference's float64 arithmetic on exactly those values.

Per case: pred, truth (float32) and `figures`, float64 in the order of KEYS: the nine keys eval_mosei_senti returns, then 'f1_non0',
which it computes and prints but does not return (made here by the same sklearn call on the same arrays).

Usage:  python tests/golden/gen_golden_senti.py
"""
import contextlib
import importlib.util
import io
import os
import warnings

import numpy as np
from sklearn.metrics import f1_score

HERE = os.path.dirname(os.path.abspath(__file__))
spec = importlib.util.spec_from_file_location("ref_eval_metrics", "/root/reference/src/utils/eval_metrics.py")
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)

KEYS = ["mae", "corr", "mult", "f1", "acc2", "acc2_non0", "acc7", "acc5", "mae_intensity", "f1_non0"]
rng = np.random.default_rng(11)
GRID = (np.arange(-9, 10) / 3.0).astype(np.float32)          # MOSEI's sentiment grid: thirds in [-3, 3], 0 exactly
cases = {}


def add(name, pred, truth):
    pred, truth = np.asarray(pred, np.float32), np.asarray(truth, np.float32)
    assert pred.shape == truth.shape and pred.ndim == 1 and (truth != 0).any(), name      # the reference fails without a non-zero truth
    p64, t64 = pred.astype(np.float64), truth.astype(np.float64)
    with warnings.catch_warnings(), np.errstate(all="ignore"), contextlib.redirect_stdout(io.StringIO()):
        warnings.simplefilter("ignore")                # numpy's empty-mean / zero-variance and sklearn's zero-division warnings
        m = ref.eval_mosei_senti(p64, t64)
        nz = t64 != 0
        m["f1_non0"] = f1_score(t64[nz] > 0, p64[nz] > 0, average="weighted")
    cases[name] = (pred, truth, np.array([m[k] for k in KEYS], dtype=np.float64))


def grid_truth(n, zeros=0.15):
    t = rng.choice(GRID, size=n)
    t[rng.random(n) < zeros] = 0.0
    return t


# random predictions around truths on the grid, exact zeros among the truths; 700 rows: three workgroups of the collector, the last partial
t = grid_truth(300); add("random_300", t + rng.normal(0, 0.9, 300), t)
t = grid_truth(700); add("random_700", t + rng.normal(0, 1.2, 700), t)
# predictions exactly 0 (and -0.0): >= 0 counts them positive, > 0 negative
t = grid_truth(96); p = (t + rng.normal(0, 0.7, 96)).astype(np.float32); p[::3] = 0.0; p[1::12] = -0.0
add("pred_zero_96", p, t)
# half-to-even at +-0.5, +-1.5, +-2.5; beyond +-3 and between 2 and 3: the two clips differ
p = np.array([0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 3.5, -3.5, 4.0, -7.25, 2.2, 2.7, -2.2, -2.7, 2.0, -2.0, 3.0, -3.0, 0.49999997, 1.5000001,
              2.4999998, -0.50000006], np.float32)
t = np.array([0.0, 0.0, 2.0, -2.0, 2.0, -3.0, 3.0, -3.0, 3.0, -3.0, 2.0, 3.0, -2.0, -3.0, 2.3333333, -2.6666667, 2.6666667, -2.3333333,
              0.0, 1.0, 2.0, -1.0], np.float32)
add("half_even_clips_22", p, t)
# no |truth| > 2: the extreme MAE is numpy's mean of an empty array, NaN
t = np.clip(grid_truth(64), -2.0, 2.0); add("no_extreme_64", t + rng.normal(0, 0.5, 64), t)
# constant predictions (0.5: every sum of them is exact, so numpy's variance is exactly 0): corr is 0 / 0
t = grid_truth(50); add("const_pred_50", np.full(50, 0.5, np.float32), t)
# one polarity absent from the predictions: a label with no predicted row in the weighted F1
t = grid_truth(80); add("all_positive_pred_80", np.abs(t + rng.normal(0, 0.8, 80)) + 0.1, t)
t = grid_truth(80); add("all_negative_pred_80", -np.abs(t + rng.normal(0, 0.8, 80)) - 0.1, t)
# a single row (corr: NaN; an extreme truth, so mae_intensity is a number)
add("one_row", np.array([2.2], np.float32), np.array([2.6666667], np.float32))
add("one_row_wrong_sign", np.array([-0.4], np.float32), np.array([1.0], np.float32))

out = {}
for k, (p, t, m) in cases.items():
    out[k + "/pred"] = p; out[k + "/truth"] = t; out[k + "/figures"] = m
out["keys"] = np.array(KEYS)
out["names"] = np.array(list(cases))
os.makedirs(os.path.join(HERE, "senti"), exist_ok=True)
np.savez_compressed(os.path.join(HERE, "senti", "senti_cases.npz"), **out)
for k, (p, t, m) in cases.items():
    print(f"{k:24s}", " ".join(f"{x:.6g}" for x in m))
print("wrote", len(cases), "cases")
