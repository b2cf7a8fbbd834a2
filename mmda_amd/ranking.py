"""Ranking metrics: how well a score table RANKS, before any cut-off is chosen.

Per class, over the rows of a split: AUROC, average precision (``ap``: of the positives; ``ap_neg``: of the negatives under the negated
score) and the false-positive rate at a true-positive level.  Per row, over the classes: label-ranking average precision, ranking loss
and coverage error.  The same table over ConfidNet's ``tcp`` against "was the decision correct" is the failure-prediction report of
the paper the confidence head comes from (AUROC, AUPR-Success, AUPR-Error, FPR at 95 % TPR).

Everything follows from integers.  With scores compared as fp32 (``-0 == +0``; a NaN counts as ``-inf``) and
``pos(i,c) = truth[i,c] > 0``, per element ``(i, c)`` over the rows ``j`` of class ``c``:

  ``gp, gn``   positives / negatives with ``s_j > s_i``
  ``ep, en``   positives / negatives with ``s_j == s_i``, row ``i`` itself included

and with ``P, Nn`` the class totals, ``ln = Nn - gn - en``, ``lp = P - gp - ep``:

  ``auroc``       ``(2 sum_{i pos} ln_i + sum_{i pos} en_i) / (2 P Nn)``                       NaN when ``P == 0`` or ``Nn == 0``
  ``ap``          ``(1/P) sum_{i pos} (gp+ep) / (gp+ep+gn+en)``                                NaN when ``P == 0``
  ``ap_neg``      ``(1/Nn) sum_{i neg} (ln+en) / (ln+en+lp+ep)``                               NaN when ``Nn == 0``
  ``fpr_at_tpr``  ``min{gn_i+en_i : i pos, gp_i+ep_i >= max(1, ceil(level P))} / Nn``          NaN when ``P == 0`` or ``Nn == 0``

(sklearn's ``roc_auc_score``, ``average_precision_score`` and the first ``roc_curve`` point at or above the level, ties grouped).  Per
row, with ``Y`` its positives, ``rank_j = #{k : s_k >= s_j}`` and ``L_j = #{k in Y : s_k >= s_j}``, the row state adds
``sum_{j in Y} L_j (720720 / rank_j)``, ``sum_{j in Y} (rank_j - L_j)`` and ``max_{j in Y} rank_j`` by ``|Y|``: about 3 C integers
from which the three means follow exactly (sklearn's ``label_ranking_average_precision_score``, ``label_ranking_loss``,
``coverage_error``).

The host functions below (plain numpy; the counts by SORTING, where the kernel compares every pair) define the quantities and are the
yardstick of the tests; ``ranking_metrics`` / ``failure_prediction`` compute the same on the device (``mmda_rank_counts``,
``mmda_rank_finish``, ``mmda_rank_rows_accumulate``).
"""
from __future__ import annotations

import ctypes
import math
from fractions import Fraction

import numpy as np
import torch

from . import _lib
from .utils.eval import LCM, host_tables

MAX_CLASSES = 16
MAX_ROWS = 1 << 20                                               # rows of one table: the count launch is quadratic
MAX_PAIRS = 1 << 42                                              # N^2 C comparisons of one table
COLUMNS = ("n_pos", "n_neg", "auroc", "ap", "ap_neg", "fpr_at_tpr")
SELECT_BY = {"valid_loss": None, "map": "map", "auroc": "macro_auroc"}


def check_select_by(select_by, process_group=False):
    """config.select_by: which dev figure ``Solver.train`` keeps the best checkpoint by.  Under a process group only ``valid_loss``:
    the ranks settle one scalar loss between them (``dist.DataParallelSync.agree``) and nothing more."""
    if select_by not in SELECT_BY:
        raise ValueError(f"select_by must be one of {tuple(SELECT_BY)}, not {select_by!r}")
    if process_group and select_by != "valid_loss":
        raise ValueError(f"select_by={select_by!r} ranks each process's own dev scores and exchanges nothing: under a process group only "
                         "select_by='valid_loss' is supported")
    return select_by


def max_rows(C):
    """The most rows of C classes one native call takes: both limits (the row entry shares the counts' refusals)."""
    return min(MAX_ROWS, math.isqrt(MAX_PAIRS // C))


def check_size(N, C):
    """ValueError naming the limit a table of N rows and C classes breaks."""
    if not 1 <= C <= MAX_CLASSES:
        raise ValueError(f"a score table must have 1 .. {MAX_CLASSES} classes, not {C}")
    if N > MAX_ROWS:
        raise ValueError(f"a score table of {N} rows is over the limit of 2^20 = {MAX_ROWS} rows (the count is quadratic in the rows)")
    if N * N * C > MAX_PAIRS:
        raise ValueError(f"a score table of {N} rows and {C} classes needs {N * N * C} comparisons, over the limit of 2^42 = {MAX_PAIRS}")


# ---------------------------------------------------------------------------------------------------- host (numpy)
def score_keys(scores):
    """fp32 scores -> uint32 keys with the order of this module: a < b <=> key(a) < key(b), equal scores <=> equal keys.  NaN -> the
    key of -inf, -0 -> +0, then negatives bit-inverted and the others given the top bit."""
    u = np.ascontiguousarray(np.asarray(scores, dtype=np.float32)).view(np.uint32).copy()
    u[(u & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)] = np.uint32(0xff800000)
    u[u == np.uint32(0x80000000)] = np.uint32(0)
    neg = (u & np.uint32(0x80000000)) != 0
    return np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def rank_counts_host(scores, truth):
    """(N, C, 4) uint32 {gp, gn, ep, en} of host arrays scores / truth (N, C), by sorting each class's keys: O(N log N)."""
    s, pos = host_tables(scores, truth, "scores and truth")
    N, C = s.shape
    keys = score_keys(s)
    out = np.zeros((N, C, 4), dtype=np.uint32)
    for c in range(C):
        k = keys[:, c]
        for col, sel in ((0, pos[:, c]), (1, ~pos[:, c])):
            srt = np.sort(k[sel])
            lo, hi = np.searchsorted(srt, k, side="left"), np.searchsorted(srt, k, side="right")
            out[:, c, col] = srt.shape[0] - hi                  # greater
            out[:, c, col + 2] = hi - lo                        # equal
    return out


def figures_from_counts(counts, truth, tpr=0.95):
    """(C + 1, 6) float64, columns ``COLUMNS``: the class rows from the counts, then the means over the classes where a figure is
    defined, added in class order (NaN where none is), whose first two columns are the number of classes in ``auroc`` and ``ap``."""
    counts = np.asarray(counts).astype(np.int64)
    pos = np.asarray(truth) > 0
    N, C = pos.shape
    if not 0.0 < tpr <= 1.0:
        raise ValueError(f"tpr must be in (0, 1], not {tpr}")
    out = np.full((C + 1, 6), np.nan, dtype=np.float64)
    for c in range(C):
        gp, gn, ep, en = (counts[:, c, k] for k in range(4))
        y = pos[:, c]
        P = int(y.sum())
        Nn = N - P
        ln, lp = Nn - gn - en, P - gp - ep
        out[c, 0], out[c, 1] = P, Nn
        if P > 0:
            out[c, 3] = ((gp + ep)[y] / (gp + ep + gn + en)[y]).sum() / float(P)
        if Nn > 0:
            out[c, 4] = ((ln + en)[~y] / (ln + en + lp + ep)[~y]).sum() / float(Nn)
        if P > 0 and Nn > 0:
            out[c, 2] = float(2 * int(ln[y].sum()) + int(en[y].sum())) / float(2 * P * Nn)
            need = max(1, int(np.ceil(np.float64(tpr) * np.float64(P))))
            out[c, 5] = float(int((gn + en)[y & (gp + ep >= need)].min())) / float(Nn)
    for f in range(2, 6):
        total, n = 0.0, 0
        for c in range(C):
            if not np.isnan(out[c, f]):
                total, n = total + out[c, f], n + 1
        out[C, f] = total / n if n else np.nan
        if f < 4:
            out[C, f - 2] = n
    return out


def state_words(C):
    return 2 + 3 * (C + 1)


def label_ranking_host(scores, truth):
    """The row state of host arrays scores / truth (N, C) as int64 [2 + 3 (C + 1)]: rows, coverage_sum, rows_by_P[C + 1],
    lrap_num[C + 1], bad_sum[C + 1]."""
    s, pos = host_tables(scores, truth, "scores and truth")
    N, C = s.shape
    if not 1 <= C <= MAX_CLASSES:
        raise ValueError(f"a score table must have 1 .. {MAX_CLASSES} classes, not {C}")
    keys = score_keys(s).astype(np.int64)
    ge = keys[:, None, :] >= keys[:, :, None]                   # [i, j, k]: s_k >= s_j
    rank = ge.sum(2)
    L = (ge & pos[:, None, :]).sum(2)
    P = pos.sum(1)
    state = np.zeros(state_words(C), dtype=np.int64)
    state[0] = N
    state[1] = np.where(pos, rank, 0).max(1, initial=0).sum() if N else 0
    lrap = np.where(pos, L * (LCM // np.maximum(rank, 1)), 0).sum(1)
    bad = np.where(pos, rank - L, 0).sum(1)
    state[2:2 + C + 1] = np.bincount(P, minlength=C + 1)
    state[2 + (C + 1):2 + 2 * (C + 1)] = [int(lrap[P == p].sum()) for p in range(C + 1)]
    state[2 + 2 * (C + 1):] = [int(bad[P == p].sum()) for p in range(C + 1)]
    return state


def label_ranking_figures(state, C):
    """{"lrap", "ranking_loss", "coverage_error"} from a row state: exact rationals, one division each.  A row with no positive, or
    with nothing but positives, counts 1 in LRAP and 0 in the ranking loss; one with no positive covers 0.  NaN without rows."""
    st = [int(x) for x in np.asarray(state).reshape(-1)]
    if len(st) != state_words(C):
        raise ValueError(f"a row state of {C} classes has {state_words(C)} words, not {len(st)}")
    rows, cover = st[0], st[1]
    by_p, lrap_num, bad = st[2:2 + C + 1], st[2 + (C + 1):2 + 2 * (C + 1)], st[2 + 2 * (C + 1):]
    if rows == 0:
        return dict(lrap=float("nan"), ranking_loss=float("nan"), coverage_error=float("nan"))
    lrap = Fraction(by_p[0] + by_p[C])
    loss = Fraction(0)
    for p in range(1, C):
        lrap += Fraction(lrap_num[p], LCM * p)
        loss += Fraction(bad[p], p * (C - p))
    return dict(lrap=float(lrap / rows), ranking_loss=float(loss / rows), coverage_error=float(Fraction(cover, rows)))


# ---------------------------------------------------------------------------------------------------- device
def rank_plan(N, C):
    """``_lib.RankPlan`` of a shape: what ``mmda_rank_counts`` launches for it (host code only)."""
    plan = _lib.RankPlan()
    _lib.check(_lib.load().mmda_rank_plan_describe(int(N), int(C), ctypes.byref(plan)), "mmda_rank_plan_describe")
    return plan


def _counts(s, t):
    """the counts of device tables already checked: the one place that launches mmda_rank_counts"""
    N, C = s.shape
    check_size(N, C)
    counts = torch.empty(N, C, 4, dtype=torch.int32, device=s.device)
    if N:
        _lib.check(_lib.load().mmda_rank_counts(s.data_ptr(), t.data_ptr(), N, C, counts.data_ptr(), _lib.stream_ptr()), "mmda_rank_counts")
    return counts


def rank_counts(scores, truth):
    """(N, C, 4) int32 on the device, the bits of the uint32 counts {gp, gn, ep, en}: one launch (and a clear where the plan splits)."""
    return _counts(*_lib.device_tables(scores, truth, "rank_counts", "scores and truth"))


def _table(s, t, tpr):
    """the (C + 1, 6) table of device tables already checked; no read-back"""
    N, C = s.shape
    check_size(N, C)
    if not 0.0 < tpr <= 1.0:
        raise ValueError(f"tpr must be in (0, 1], not {tpr}")
    if N == 0:                                                   # an empty split: nothing is defined, no class enters a mean
        table = torch.full((C + 1, 6), float("nan"), dtype=torch.float64, device=s.device)
        table[:, :2] = 0.0
        return table, None
    counts = _counts(s, t)
    table = torch.empty(C + 1, 6, dtype=torch.float64, device=s.device)
    _lib.check(_lib.load().mmda_rank_finish(counts.data_ptr(), t.data_ptr(), N, C, float(tpr), table.data_ptr(), _lib.stream_ptr()),
               "mmda_rank_finish")
    return table, counts


class RowRanking:
    """The label-ranking state of a stream of batches: ``update(scores, truth)`` per batch (one launch, no synchronisation), ``state``
    on the device, ``figures()`` after one read-back."""

    def __init__(self, num_classes, device="cuda"):
        self.C = int(num_classes)
        if not 1 <= self.C <= MAX_CLASSES:
            raise ValueError(f"num_classes must be in 1 .. {MAX_CLASSES}, not {num_classes}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.MMDAError(f"RowRanking counts on the GPU only (the HIP path has no CPU fallback), not on {self.device}")
        self.state = torch.zeros(state_words(self.C), dtype=torch.int64, device=self.device)

    def update(self, scores, truth):
        s, t = _lib.device_tables(scores, truth, "RowRanking.update", "scores and truth")
        if s.shape[1] != self.C:
            raise ValueError(f"scores and truth must both be (N, {self.C}), not {tuple(s.shape)}")
        step = max_rows(self.C)                                  # what one call takes: the row cap and the comparison cap
        for at in range(0, s.shape[0], step):
            a, b = s[at:at + step], t[at:at + step]
            _lib.check(_lib.load().mmda_rank_rows_accumulate(a.data_ptr(), b.data_ptr(), a.shape[0], self.C, self.state.data_ptr(),
                                                             _lib.stream_ptr()), "mmda_rank_rows_accumulate")

    def figures(self):
        return label_ranking_figures(self.state.cpu().numpy(), self.C)


class RankingResult:
    """``table`` (C + 1, 6) float64, columns ``COLUMNS``, row C the means; ``micro`` (2, 6) or None: the same over all (row, class)
    elements pooled; ``rows`` int64 [2 + 3 (C + 1)] or None: the label-ranking state.  On the device as ``ranking_metrics`` returns
    it; ``cpu()`` reads back, ``as_dict()`` names the figures."""

    def __init__(self, table, micro=None, rows=None, tpr=0.95, counts=None):
        self.table, self.micro, self.rows, self.tpr, self.counts = table, micro, rows, float(tpr), counts

    @property
    def C(self):
        return int(self.table.shape[0]) - 1

    def cpu(self):
        """The same on the host (one small device-to-host copy per table held); the per-element counts are dropped."""
        host = lambda x: None if x is None else x.cpu()
        return RankingResult(host(self.table), host(self.micro), host(self.rows), self.tpr)

    def as_dict(self):
        """Per-class lists under ``COLUMNS``' names, ``macro_auroc``, ``map``, ``macro_ap_neg``, ``macro_fpr_at_tpr``; with the row
        state ``lrap``, ``ranking_loss``, ``coverage_error``; with the pooled table ``micro_auroc``, ``micro_ap``, ``micro_ap_neg``,
        ``micro_fpr_at_tpr``.  Reads back what is still on the device."""
        r = self.cpu()
        t, C = r.table.numpy(), self.C
        out = {name: t[:C, k].tolist() for k, name in enumerate(COLUMNS)}
        out.update(tpr=self.tpr, macro_auroc=float(t[C, 2]), map=float(t[C, 3]), macro_ap_neg=float(t[C, 4]),
                   macro_fpr_at_tpr=float(t[C, 5]))
        if r.rows is not None:
            out.update(label_ranking_figures(r.rows.numpy(), C))
        if r.micro is not None:
            m = r.micro.numpy()
            out.update(micro_auroc=float(m[0, 2]), micro_ap=float(m[0, 3]), micro_ap_neg=float(m[0, 4]), micro_fpr_at_tpr=float(m[0, 5]))
        return out


def ranking_metrics(scores, truth, tpr=0.95, micro=False, label_ranking=True):
    """``RankingResult`` of device tables scores / truth (N, C): the per-class table and its means (two launches), the label-ranking
    state (one launch) and, ``micro=True``, the pooled figures by a second pass over the (N C, 1) view.  No read-back."""
    s, t = _lib.device_tables(scores, truth, "ranking_metrics", "scores and truth")
    N, C = s.shape
    table, counts = _table(s, t, tpr)
    pooled = None
    if micro:
        pooled, _ = _table(s.reshape(N * C, 1), t.reshape(N * C, 1), tpr)
    rows = None
    if label_ranking:
        acc = RowRanking(C, s.device)
        acc.update(s, t)
        rows = acc.state
    return RankingResult(table, pooled, rows, tpr, counts)


class FailurePrediction(RankingResult):
    """``RankingResult`` over a confidence table against "was the decision correct", with the names of the failure-prediction
    literature in ``as_dict()``: ``auroc``, ``aupr_success`` (= ap), ``aupr_error`` (= ap_neg), ``fpr_at_95tpr`` (at ``tpr``)."""

    def as_dict(self):
        t, C = self.table.cpu().numpy(), self.C
        fpr = "fpr_at_%dtpr" % round(100 * self.tpr)
        out = dict(n_correct=t[:C, 0].tolist(), n_wrong=t[:C, 1].tolist(), auroc=t[:C, 2].tolist(), aupr_success=t[:C, 3].tolist(),
                   aupr_error=t[:C, 4].tolist(), tpr=self.tpr)
        out[fpr] = t[:C, 5].tolist()
        out.update(macro_auroc=float(t[C, 2]), macro_aupr_success=float(t[C, 3]), macro_aupr_error=float(t[C, 4]))
        out["macro_" + fpr] = float(t[C, 5])
        return out


def failure_prediction(tcp, correct, tpr=0.95):
    """ConfidNet's ``tcp`` (n, C) against ``correct = (labels == truth)`` (n, C), both on the device: does the confidence rank the
    correct decisions above the wrong ones.  ``FailurePrediction``, on the device."""
    s, t = _lib.device_tables(tcp, correct, "failure_prediction", "scores and truth")
    table, counts = _table(s, t, tpr)
    return FailurePrediction(table, None, None, tpr, counts)
