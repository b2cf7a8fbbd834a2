#!/usr/bin/env python3
"""Generate tests/golden/rank/rank_cases.npz: small (scores, truth) tables with scikit-learn's own figures -- per class
roc_auc_score, average_precision_score in both senses (the positives under the score; the negatives under the negated score) and the
false-positive rate of the first roc_curve point whose true-positive rate reaches 0.95; per table
label_ranking_average_precision_score, label_ranking_loss and coverage_error.  Needs scikit-learn (the tests do not).

Where a class has no positive (or no negative) the figures our definitions leave undefined are stored as NaN: roc_auc_score raises
there and average_precision_score returns 0 with a warning.  NaN and infinite scores are kept out (sklearn refuses them); -0.0 is in.

FPR cases: in the random tables no class has a number of positives P with 0.95 P within 1e-9 of an integer (the table is drawn again
otherwise).  Two single-class tables have P = 20 and P = 40, where 0.95 P is exactly 19 and 38: there sklearn's tpr is 19/20 and
38/40, both the double nearest to 0.95, so `tpr >= 0.95` holds at the 19th (38th) positive and roc_curve gives the false-positive
rate at that point -- the same element that need = ceil(0.95 * 20.0) = 19 (ceil(0.95 * 40.0) = 38: both products round to the
integer) selects.

Usage:  python tests/golden/gen_golden_rank.py
"""
import os
import warnings

import numpy as np
from sklearn.metrics import (average_precision_score, coverage_error, label_ranking_average_precision_score, label_ranking_loss,
                             roc_auc_score, roc_curve)

HERE = os.path.dirname(os.path.abspath(__file__))
TPR = 0.95
rng = np.random.default_rng(41)


def fpr_at(y, s):
    fpr, tpr, _ = roc_curve(y, s, drop_intermediate=False)
    return float(fpr[np.argmax(tpr >= TPR)])


def class_figures(s, y):
    out = np.full(4, np.nan)
    P, Nn = int(y.sum()), int((1 - y).sum())
    if P and Nn:
        out[0] = roc_auc_score(y, s)
        out[3] = fpr_at(y, s)
    if P:
        out[1] = average_precision_score(y, s)
    if Nn:
        out[2] = average_precision_score(1 - y, -s.astype(np.float64))
    return out


def near_integer(P):
    return abs(TPR * P - round(TPR * P)) <= 1e-9


def draw(N, C, ties, rate):
    while True:
        truth = (rng.random((N, C)) < rate).astype(np.float32)
        if not any(near_integer(int(p)) and p > 0 for p in truth.sum(0)):
            break
    scores = (0.4 * truth + rng.normal(0.3, 0.25, (N, C))).astype(np.float32)
    if ties == "quarters":
        scores = (np.round(scores * 4) / 4).astype(np.float32)
    elif ties == "halves":
        scores = (np.round(scores * 2) / 2).astype(np.float32)
        zero = scores == 0
        scores[zero] = np.where(rng.random(int(zero.sum())) < 0.5, np.float32(-0.0), np.float32(0.0))   # some zeros negative: -0 == +0
    return scores, truth


cases = []
for N in (2, 5, 17, 33, 64, 120):
    for C in (1, 3, 6):
        for ties in ("none", "quarters", "halves"):
            cases.append(draw(N, C, ties, rng.uniform(0.1, 0.6, C)))
# value classes: an all-equal column, a class with no positives, a class with no negatives, empty and full rows
s, t = draw(41, 6, "quarters", np.full(6, 0.3))
s[:, 1] = np.float32(0.5); t[:, 2] = 0.0; t[:, 3] = 1.0; t[5] = 0.0; t[6] = 1.0
cases.append((s, t))
s, t = draw(9, 16, "none", np.full(16, 0.4))
cases.append((s, t))
# 0.95 P exactly an integer: P = 20 and P = 40, one class, every score distinct (then with ties)
for P, N, ties in ((20, 55, False), (40, 90, False), (20, 55, True), (40, 90, True)):
    t = np.zeros((N, 1), dtype=np.float32)
    t[rng.permutation(N)[:P]] = 1.0
    s = (0.3 * t + rng.normal(0.3, 0.25, (N, 1))).astype(np.float32)
    if ties:
        s = (np.round(s * 8) / 8).astype(np.float32)
    cases.append((s, t))

out = {"n_cases": np.int64(len(cases)), "tpr": np.float64(TPR)}
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    for k, (s, t) in enumerate(cases):
        assert np.isfinite(s).all()
        N, C = s.shape
        per_class = np.stack([class_figures(s[:, c], t[:, c]) for c in range(C)])            # (C, 4): auroc, ap, ap_neg, fpr
        rows = np.full(3, np.nan)
        if C > 1:                                                                               # sklearn wants a multilabel table
            rows[:] = [label_ranking_average_precision_score(t, s), label_ranking_loss(t, s), coverage_error(t, s)]
        out[f"scores_{k}"], out[f"truth_{k}"], out[f"classes_{k}"], out[f"rows_{k}"] = s, t, per_class, rows

os.makedirs(os.path.join(HERE, "rank"), exist_ok=True)
np.savez_compressed(os.path.join(HERE, "rank", "rank_cases.npz"), **out)
print("wrote", len(cases), "cases")
