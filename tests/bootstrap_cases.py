"""The tables, shapes and bounds of the bootstrap tests (tests/test_bootstrap_cpu.py, tests/test_gpu_bootstrap.py).

Tables: ``rank_cases.value_case(n, C)`` for scores and truth -- heavy ties, an all-equal column, a class with no positives, one with
no negatives, +-inf, NaN and -0 -- and labels ``scores > 0.35``.  The DECISION tables (labels, truth_d) have one row cleared in both,
for the ``max(union, 1)`` branch of the Jaccard accuracy; the ranking tables keep value_case's truth, whose column 3 has no negatives.

Bounds (EPS = 2^-52):
  states            integers: equality.
  decision figures  quotients of integers below 2^53 and sums of at most C <= 16 of them, each in [0, 1], added in class order on the
                    device and by numpy's unrolled sum on the host: every figure is within (C + 2) 2^-53 of the exact one on either
                    side, so the two differ by at most (C + 2) EPS.
  auroc, fpr        an integer reduction and one fp64 division on both sides: the same bits.
  ap, ap_neg        P_w (Nn_w) terms w_i q_i against the materialised sum of the same q_i, each w_i times, in another order: as in
                    tests/test_gpu_rank.py, P_w EPS after the division by P_w.
"""
import numpy as np

from mmda_amd import bootstrap as bt
from mmda_amd import ranking as rk
from mmda_amd.utils.eval import KEYS, get_metrics
from rank_cases import value_case

EPS = 2.0 ** -52
THRESHOLD = 0.35
SMALL_R = (1, 2, 65)
LARGE_R = (3,)
SEED = 20261021


def gpu_shapes():
    """(n, C) of the GPU test: the small and odd ends, the count kernel's threads per workgroup - 1 / + 0 / + 1 at six classes, and the
    LDS edge (at 16385 the ranking call refuses and the decision call takes the global form)."""
    p = bt.boot_plan(1, 1, 1)
    T, L = p.threads, p.lds_rows
    return [(1, 1), (2, 1), (37, 6), (300, 16), (T - 1, 6), (T, 6), (T + 1, 6), (L, 6), (L + 1, 6)]


def replicates(shape):
    return LARGE_R if shape[0] > 4096 else SMALL_R


def case(n, C):
    """dict(scores, truth, labels, truth_d): see the module docstring"""
    scores, truth = value_case(n, C)
    with np.errstate(invalid="ignore"):
        labels = (scores > np.float32(THRESHOLD)).astype(np.float32)
    truth_d = truth.copy()
    labels[n // 5] = 0.0
    truth_d[n // 5] = 0.0
    return dict(scores=scores, truth=truth, labels=labels, truth_d=truth_d)


SWEEP_SHAPES = [(2, 1), (37, 6), (300, 16)]                     # (300, 16): the longest class sums
SWEEP_GRID = np.array([0.1, 0.25, THRESHOLD, 0.5, 0.8], dtype=np.float32)


def sweep_case(n, C):
    """(scores, truth_d, labels per cut-off of SWEEP_GRID) for the tests that hold a threshold sweep against the bootstrap's identity
    replicate: ``case``'s decision tables with row n // 5 cleared in the SCORES too, so that it predicts nothing at any cut-off and
    takes the ``max(union, 1)`` branch on both sides; the NaN and +-inf of ``value_case`` go through ``s > t`` on both."""
    c = case(n, C)
    scores = c["scores"].copy()
    scores[n // 5] = 0.0
    with np.errstate(invalid="ignore"):
        labels = [(scores > t).astype(np.float32) for t in SWEEP_GRID]
    return scores, c["truth_d"], labels


def materialised_decisions(labels, truth, j):
    """(state int64 [3 C + 2], get_metrics' dict) of the rows ``j`` of the decision tables"""
    p, y = labels[j] > 0, truth[j] > 0
    C = p.shape[1]
    inter, union = (p & y).sum(1), np.maximum((p | y).sum(1), 1)
    state = np.concatenate([(p & y).sum(0), (p & ~y).sum(0), (~p & y).sum(0), [int(((bt.LCM // union) * inter).sum()), len(j)]])
    assert state.shape == (3 * C + 2,)
    return state.astype(np.int64), get_metrics(truth[j], labels[j])


def materialised_ranking(scores, truth, j, tpr=0.95):
    return rk.figures_from_counts(rk.rank_counts_host(scores[j], truth[j]), truth[j], tpr)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


def check_decision_figures(got, state, metrics, C):
    """one row of a figure table against the materialised resample's state and get_metrics dict"""
    assert got.shape == (10 + 3 * C,)
    n = float(state[3 * C + 1])
    exact_acc = float(state[3 * C]) / (bt.LCM * n)
    assert abs(got[0] - exact_acc) <= EPS and abs(got[0] - metrics["acc"]) <= 0.5e-4 + EPS      # get_accuracy rounds to four places
    for k, key in enumerate(KEYS[1:], start=1):
        assert abs(got[k] - metrics[key]) <= (C + 2) * EPS, key
    tp, fp, fn = (state[k * C:(k + 1) * C].astype(np.float64) for k in range(3))
    div = lambda a, b: np.where(b > 0, a / np.where(b > 0, b, 1.0), 0.0)
    assert same_bits(got[10:10 + C], div(2 * tp, 2 * tp + fp + fn))
    assert same_bits(got[10 + C:10 + 2 * C], div(tp, tp + fp)) and same_bits(got[10 + 2 * C:], div(tp, tp + fn))


def check_rank_table(got, want, C):
    """tests/test_gpu_rank.py's check_table, with P_w and Nn_w (the table's own first two columns) for P and Nn"""
    assert got.shape == want.shape == (C + 1, 6)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got[:C, :2], want[:C, :2])
    assert same_bits(got[:C, 2], want[:C, 2]) and same_bits(got[:C, 5], want[:C, 5])
    for col, n in ((3, want[:C, 0]), (4, want[:C, 1])):
        diff = np.nan_to_num(np.abs(got[:C, col] - want[:C, col]))
        assert (diff <= n * EPS).all(), (col, diff.max())
    assert np.array_equal(got[C, :2], want[C, :2])
    for f in range(2, 6):
        vals = [v for v in got[:C, f] if not np.isnan(v)]
        if not vals:
            assert np.isnan(got[C, f])
        else:
            total = 0.0
            for v in vals:
                total += v
            assert abs(got[C, f] - total / len(vals)) <= C * EPS, f


def summary_table(R, F, seed=0):
    """an (R + 1, F) figure table for the summary tests: column 0 all defined, 1 a third NaN, 2 all NaN, 3 one defined value, 4 two,
    5 constant, 6 signed with exact zeros; the rest random"""
    rng = np.random.default_rng(seed + 31 * R + F)
    x = rng.normal(0.4, 0.2, (R + 1, F))
    if F > 1:
        x[rng.random(R + 1) < 1 / 3, 1] = np.nan
    if F > 2:
        x[:, 2] = np.nan
    if F > 3:
        x[1:, 3] = np.nan
    if F > 4:
        x[2:, 4] = np.nan
    if F > 5:
        x[:, 5] = 0.25
    if F > 6:
        x[:, 6] = np.round(rng.normal(0.0, 1.0, R + 1))
    return x
