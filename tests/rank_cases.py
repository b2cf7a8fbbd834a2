"""The tables of the ranking-metric tests (tests/test_rank_cpu.py, tests/test_gpu_rank.py): the shapes the GPU test runs, taken from the
plan's own numbers, and one table per shape that holds every value class the shape has columns for: all of them from six classes on
(``value_classes`` names which column holds which), so every shape but (1, 1) and (2, 1), which the issue fixes, has six or more."""
import numpy as np

from mmda_amd import ranking as rk


def gpu_shapes():
    """The (N, C) of tests/test_gpu_rank.py, from the plan's own numbers: the fixed ones, rows-per-workgroup and j-tile -1 / +0 / +1
    (six classes each, so that every value class sits on those edges), one above the size at which a 16-class table stops being
    split, and the largest (split, several tiles per split)."""
    p = rk.rank_plan(1, 1)
    R, T = p.rows_per_wg, p.tile
    shapes = [(1, 1), (2, 1), (37, 6), (300, 16)]
    shapes += [(R - 1, 6), (R, 6), (R + 1, 6), (T - 1, 6), (T, 6), (T + 1, 6)]
    n = T
    while rk.rank_plan(n, 16).splits > 1 or rk.rank_plan(n, 16).tiles < 2:
        n += R
    shapes += [(n + 1, 16), (20001, 6)]
    return shapes


def value_case(N, C, seed=0):
    """Every value class of the GPU test in one table, as far as C reaches (all of them at C >= 6): column 0 rounded to quarters (heavy
    ties, both kinds of rows); column 1 all equal (1.0); column 2 a class with no positives; column 3 one with no negatives (in quarters);
    columns 4 and 5 informative and untied, both kinds of rows; the row [0, 1, NaN, -0.0, +inf, -inf] at N // 2; a real -inf in the last
    column at N // 3; a NaN in the last row, first and last column, for the tile tail."""
    rng = np.random.default_rng(seed + 7919 * N + C)
    truth = (rng.random((N, C)) < np.linspace(0.5, 0.08, C)).astype(np.float32)
    scores = (0.4 * truth + rng.normal(0.3, 0.25, (N, C))).astype(np.float32)
    scores[:, 0::3] = np.round(scores[:, 0::3] * 4) / 4
    if C > 1:
        scores[:, 1] = np.float32(1.0)                          # all equal, the special row's 1 included
    if C > 2:
        truth[:, 2] = 0.0
    if C > 3:
        truth[:, 3] = 1.0
    special = np.array([0.0, 1.0, np.nan, -0.0, np.inf, -np.inf], dtype=np.float32)
    scores[N // 2, :min(C, 6)] = special[:C]
    if N > 2:
        scores[N // 3, C - 1] = -np.inf                         # a real -inf: ties with the NaNs
    scores[N - 1, 0] = np.nan
    scores[N - 1, C - 1] = np.nan
    return scores, truth


def value_classes(scores, truth):
    """Which value classes a table holds: what ``value_case`` promises at C >= 6, restated from the table itself."""
    s, pos = np.asarray(scores), np.asarray(truth) > 0
    N, C = s.shape
    fin = np.where(np.isfinite(s), s, 0.0)
    both = pos.any(0) & (~pos).any(0)
    distinct = np.array([np.unique(fin[:, c]).size for c in range(C)])
    special = s[N // 2, :min(C, 6)]
    return dict(no_positives=bool((~pos.any(0)).any()), no_negatives=bool(pos.all(0).any()), all_equal=bool((distinct == 1).any()),
                heavy_ties=bool((both & (distinct > 1) & (distinct <= 16)).any()), untied=bool((both & (distinct >= 0.99 * (N - 3))).any()),
                special_row=bool(C >= 6 and special[0] == 0 and not np.signbit(special[0]) and special[1] == 1 and np.isnan(special[2])
                                 and special[3] == 0 and np.signbit(special[3]) and special[4] == np.inf and special[5] == -np.inf),
                real_neg_inf=bool(N > 2 and s[N // 3, C - 1] == -np.inf), nan_in_last_row=bool(np.isnan(s[N - 1]).any()))
