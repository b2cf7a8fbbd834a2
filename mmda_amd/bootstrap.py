"""Bootstrap intervals and paired tests for every report: how far a figure would move on another draw of the split.

The non-parametric bootstrap over the n rows of a split.  Replicate ``r`` in ``0 .. R - 1`` draws n rows with replacement: for
``k`` in ``0 .. n - 1``

  ``u = rng_u32(seed, 12, (r << 32) + k)``  (``csrc/common.h``'s generator at the site ``SITE_BOOTSTRAP``),  ``j(r, k) = (u * n) >> 32``

and row ``i`` has the weight ``w_r[i] = #{k : j(r, k) = i}``; the weights of a replicate sum to n.  The multiply-high map is
non-uniform by at most ``n / 2^32`` (under 2.5e-4 at the row limit, 4e-7 at MOSEI's dev split).  A replicate depends on ``(seed, r, n)``
alone -- not on R, on C, on the table or on which report is resampled -- so two reports over the same ``(seed, n)`` see the same
resamples: a PAIRED comparison.  One more replicate, the identity (``w = 1``, row R of every table), gives each figure's point
estimate through the same kernels.  ``resample_indices`` restates the draws in numpy.

What is resampled:

  decisions  everything ``utils.eval.get_metrics`` is a function of.  Per replicate one integer state ``tp[C], fp[C], fn[C], acc_num,
             n`` (``acc_num = sum over the draws of 720720 |y & p| / max(|y | p|, 1)``, an integer), from it the ten ``KEYS`` by
             ``metrics_from_counts``' arithmetic (``acc`` not rounded to four places) and ``f1 / precision / recall`` per class.
  ranking    everything ``ranking.figures_from_counts`` returns: with ``GP, GN, EP, EN`` the counts of the ``ranking.py`` docstring
             under the replicate's weights (a row's own full weight in its ``E*``), over the rows with ``w_i > 0``:
             ``auroc = (2 sum_{pos} w_i LN_i + sum_{pos} w_i EN_i) / (2 P_w Nn_w)``, ``ap = (1/P_w) sum_{pos} w_i (GP+EP)/(GP+EP+GN+EN)``,
             ``ap_neg`` likewise, ``fpr_at_tpr = min{GN_i+EN_i : i pos, GP_i+EP_i >= max(1, ceil(tpr P_w))} / Nn_w`` -- the figures of
             the materialised resample ``figures_from_counts(rank_counts_host(s[j_r], t[j_r]), t[j_r], tpr)``, NaN by the same rules.

``summary`` turns an ``(R + 1, F)`` figure table into ``point, mean, std, lo, hi, defined`` per figure (percentile interval over the
replicates where the figure is defined); ``Bootstrap.compare`` summarises the replicate-wise difference of two results and adds
``p_le, p_ge, p_two``.  The host functions (plain numpy) define the quantities and are the yardstick of the tests; ``Bootstrap``
computes the same on the device (``csrc/bootstrap.hip``) with no read-back.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib, step_rules
from .modality import _rng_u32
from .utils.eval import LCM

SITE_BOOTSTRAP = 12                      # the next free id after modality.SITE_MODALITY
MAX_REPLICATES = step_rules.BOOT_MAX_REPLICATES
MAX_ROWS = step_rules.BOOT_MAX_ROWS
MAX_CLASSES = step_rules.BOOT_MAX_CLASSES
RANK_MAX_ROWS = step_rules.BOOT_RANK_MAX_ROWS
SUMMARY_COLUMNS = ("point", "mean", "std", "lo", "hi", "defined")
COMPARE_COLUMNS = SUMMARY_COLUMNS + ("p_le", "p_ge", "p_two")
FORMS = {"auto": 0, "lds": 1, "global": 2}


# ---------------------------------------------------------------------------------------------------- names
def decision_names(C):
    """The columns of a decision figure table: the ten ``utils.eval.KEYS``, then f1 / precision / recall per class."""
    from .utils.eval import KEYS
    return tuple(KEYS) + tuple(f"{k}[{c}]" for k in ("f1", "precision", "recall") for c in range(C))


def ranking_names(C, failure=False, tpr=0.95):
    """The columns of a ranking figure table, the ``(C + 1, 6)`` table row by row: per class ``ranking.COLUMNS`` (``failure``: the
    names of ``FailurePrediction.as_dict``), then the macro row, whose first two entries count the classes in ``auroc`` and ``ap``."""
    if failure:
        fpr = "fpr_at_%dtpr" % round(100 * tpr)
        cols = ("n_correct", "n_wrong", "auroc", "aupr_success", "aupr_error", fpr)
        macro = ("classes_in_auroc", "classes_in_aupr", "macro_auroc", "macro_aupr_success", "macro_aupr_error", "macro_" + fpr)
    else:
        from .ranking import COLUMNS as cols
        macro = ("classes_in_auroc", "classes_in_ap", "macro_auroc", "map", "macro_ap_neg", "macro_fpr_at_tpr")
    return tuple(f"{k}[{c}]" for c in range(C) for k in cols) + macro


# ---------------------------------------------------------------------------------------------------- host (numpy)
def resample_indices(seed, R, n):
    """(R, n) int64: ``j(r, k)`` of the module docstring, every entry in ``[0, n)``.  Row r does not depend on R."""
    R, n = int(R), int(n)
    r = np.arange(R, dtype=np.uint64)[:, None] << np.uint64(32)
    k = np.arange(n, dtype=np.uint64)[None, :]
    u = _rng_u32(seed, SITE_BOOTSTRAP, r + k).astype(np.uint64)
    return ((u * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def resample_weights(seed, R, n):
    """(R + 1, n) int64: ``w_r[i]``, row R the identity's ones."""
    j = resample_indices(seed, R, n)
    w = np.ones((int(R) + 1, int(n)), dtype=np.int64)
    for r in range(int(R)):
        w[r] = np.bincount(j[r], minlength=int(n))
    return w


def _check_host(n, C, R, rank=False):
    step_rules.bootstrap_check(replicates=R, n=int(n), C=int(C), rank=rank)


def figures_from_states(state, C):
    """(rows, 10 + 3 C) float64 from integer states (rows, 3 C + 2): ``metrics_from_counts`` per row, ``acc = acc_num / (LCM n)``."""
    from .utils.eval import KEYS, _div, metrics_from_counts
    state = np.asarray(state, dtype=np.int64).reshape(-1, 3 * C + 2)
    out = np.empty((state.shape[0], 10 + 3 * C), dtype=np.float64)
    for r, st in enumerate(state):
        tp, fp, fn = (st[k * C:(k + 1) * C].astype(np.float64) for k in range(3))
        acc = float(st[3 * C]) / (float(LCM) * float(st[3 * C + 1])) if st[3 * C + 1] > 0 else float("nan")
        m = metrics_from_counts(tp, fp, fn, acc)
        out[r, :10] = [m[k] for k in KEYS]
        out[r, 10:10 + C] = _div(2 * tp, 2 * tp + fp + fn)
        out[r, 10 + C:10 + 2 * C] = _div(tp, tp + fp)
        out[r, 10 + 2 * C:] = _div(tp, tp + fn)
    return out


def decisions_host(labels, truth, seed, R):
    """``(state (R + 1, 3 C + 2) int64, figures (R + 1, 10 + 3 C) float64)`` of host tables labels / truth (n, C): the weighted
    restatement of ``mmda_boot_counts`` / ``mmda_boot_figures``."""
    p, y = np.asarray(labels) > 0, np.asarray(truth) > 0
    if p.ndim != 2 or p.shape != y.shape:
        raise ValueError(f"labels and truth must both be (n, C), not {p.shape} and {y.shape}")
    n, C = p.shape
    _check_host(n, C, R)
    w = resample_weights(seed, R, n)                                      # (R + 1, n)
    inter, union = (p & y).sum(1), np.maximum((p | y).sum(1), 1)
    row_acc = (LCM // union) * inter                                      # an integer per row
    state = np.empty((R + 1, 3 * C + 2), dtype=np.int64)
    state[:, :C] = w @ (p & y).astype(np.int64)
    state[:, C:2 * C] = w @ (p & ~y).astype(np.int64)
    state[:, 2 * C:3 * C] = w @ (~p & y).astype(np.int64)
    state[:, 3 * C] = w @ row_acc.astype(np.int64)
    state[:, 3 * C + 1] = w.sum(1)
    return state, figures_from_states(state, C)


def ranking_host(scores, truth, seed, R, tpr=0.95):
    """(R + 1, C + 1, 6) float64 of host tables scores / truth (n, C): the weighted restatement of ``mmda_boot_rank``.  Per class the
    keys are sorted once; a replicate's weighted counts are prefix sums of its weights over that order."""
    from .ranking import score_keys
    s = np.asarray(scores, dtype=np.float32)
    pos = np.asarray(truth) > 0
    if s.ndim != 2 or pos.shape != s.shape:
        raise ValueError(f"scores and truth must both be (n, C), not {s.shape} and {pos.shape}")
    if not 0.0 < tpr <= 1.0:
        raise ValueError(f"tpr must be in (0, 1], not {tpr}")
    n, C = s.shape
    _check_host(n, C, R, rank=True)
    w_all = resample_weights(seed, R, n)
    keys = score_keys(s)
    out = np.full((R + 1, C + 1, 6), np.nan, dtype=np.float64)
    for c in range(C):
        order = np.argsort(keys[:, c], kind="stable")                     # ascending
        ks, y = keys[order, c], pos[order, c]
        lo, hi = np.searchsorted(ks, ks, side="left"), np.searchsorted(ks, ks, side="right")
        for r in range(R + 1):
            w = w_all[r][order]
            cp = np.concatenate([[0], np.cumsum(np.where(y, w, 0))])      # weight of the positives among the first k sorted rows
            cn = np.concatenate([[0], np.cumsum(np.where(y, 0, w))])
            P, Nn = int(cp[-1]), int(cn[-1])
            gp, gpep = P - cp[hi], P - cp[lo]                             # greater; greater or equal
            gn, gnen = Nn - cn[hi], Nn - cn[lo]
            live_p, live_n = y & (w > 0), ~y & (w > 0)
            row = out[r, c]
            row[0], row[1] = P, Nn
            if P > 0:                                                     # added in descending-score order, as the positions are
                terms = (w * (gpep / np.maximum(gpep + gnen, 1)))[live_p][::-1]
                row[3] = float(np.cumsum(terms)[-1]) / float(P)
            if Nn > 0:
                lnen, lpep = Nn - gn, P - gp
                terms = (w * (lnen / np.maximum(lnen + lpep, 1)))[live_n][::-1]
                row[4] = float(np.cumsum(terms)[-1]) / float(Nn)
            if P > 0 and Nn > 0:
                num = int((w * (2 * (Nn - gnen) + (gnen - gn)))[live_p].sum())
                row[2] = float(num) / float(2 * P * Nn)
                need = max(1, int(np.ceil(np.float64(tpr) * np.float64(P))))
                row[5] = float(int(gnen[live_p & (gpep >= need)].min())) / float(Nn)
    for r in range(R + 1):
        for f in range(2, 6):
            total, k = 0.0, 0
            for c in range(C):
                if not np.isnan(out[r, c, f]):
                    total, k = total + out[r, c, f], k + 1
            out[r, C, f] = total / k if k else np.nan
            if f < 4:
                out[r, C, f - 2] = k
    return out


def _percentile(x, q):
    m = x.shape[0]
    h = np.float64(m - 1) * np.float64(q)
    a = min(max(int(np.floor(h)), 0), m - 1)
    b = min(a + 1, m - 1)
    return x[a] + (h - np.float64(a)) * (x[b] - x[a])


def summary_host(figures, alpha=0.05, other=None):
    """``mmda_boot_summary``'s arithmetic in numpy: ``figures`` (R + 1, F) -> (F, 6) float64, columns ``SUMMARY_COLUMNS``.  With
    ``other`` (R + 1, F) the rows are the differences ``figures - other`` (NaN where either is) and the result is (F, 9), columns
    ``COMPARE_COLUMNS``.  Per figure the m defined replicate values are sorted; ``mean`` and the two-pass ``std`` (ddof 1) are added in
    sorted order, one addition after the other; the percentiles at ``q = alpha / 2`` and ``1 - alpha / 2`` interpolate linearly at
    ``h = (m - 1) q``: ``x[a] + (h - a) (x[min(a + 1, m - 1)] - x[a])``, ``a = floor(h)``.  ``m < 2``: ``std`` NaN; ``m == 0``: ``mean``,
    ``std``, ``lo``, ``hi`` NaN."""
    q_lo, q_hi = _quantiles(alpha)
    x = np.asarray(figures, dtype=np.float64)
    if other is not None:
        x = x - np.asarray(other, dtype=np.float64)
    R, F = x.shape[0] - 1, x.shape[1]
    out = np.full((F, 6 if other is None else 9), np.nan, dtype=np.float64)
    for f in range(F):
        v = x[:R, f]
        v = np.sort(v[~np.isnan(v)])
        m = v.shape[0]
        out[f, 0], out[f, 5] = x[R, f], m
        if m > 0:
            mean = np.cumsum(v)[-1] / np.float64(m)                      # cumsum: one addition after the other
            out[f, 1] = mean
            if m > 1:
                d = v - mean
                out[f, 2] = np.sqrt(np.cumsum(d * d)[-1] / np.float64(m - 1))
            out[f, 3], out[f, 4] = _percentile(v, q_lo), _percentile(v, q_hi)
        if other is not None:
            p_le, p_ge = (1 + int((v <= 0).sum())) / (m + 1), (1 + int((v >= 0).sum())) / (m + 1)
            out[f, 6], out[f, 7], out[f, 8] = p_le, p_ge, min(1.0, 2.0 * min(p_le, p_ge))
    return out


def _quantiles(alpha):
    alpha = float(alpha)
    if not 0.0 < alpha < 1.0:
        raise ValueError(f"alpha must be in (0, 1), not {alpha}")
    return alpha / 2.0, 1.0 - alpha / 2.0


# ---------------------------------------------------------------------------------------------------- device
def boot_plan(n, C, R):
    """``_lib.BootPlan`` of a shape: the form ``mmda_boot_counts`` gives it and the limits of the entry points (host code only)."""
    plan = _lib.BootPlan()
    _lib.check(_lib.load().mmda_boot_plan_describe(int(n), int(C), int(R), ctypes.byref(plan)), "mmda_boot_plan_describe")
    return plan


class BootstrapSummary:
    """``table`` (F, 6) float64 -- or (F, 9) for a comparison -- on the device, ``names`` its rows, ``columns`` its columns;
    ``as_dict()`` reads back and names: ``{figure: {column: value}}``."""

    def __init__(self, table, names, columns, alpha):
        self.table, self.names, self.columns, self.alpha = table, tuple(names), tuple(columns), float(alpha)

    def cpu(self):
        return BootstrapSummary(self.table.cpu(), self.names, self.columns, self.alpha)

    def as_dict(self):
        t = self.table.cpu().numpy()
        return {name: {col: float(t[f, k]) for k, col in enumerate(self.columns)} for f, name in enumerate(self.names)}

    def format(self, only=None):
        """Lines ``figure  point  [lo, hi]`` (a comparison: and ``p_two``); ``only``: the names to print (None: all)."""
        d = self.as_dict()
        lines = []
        for name in (self.names if only is None else only):
            r = d[name]
            line = f"{name:<24}{r['point']:10.4f}  [{r['lo']:.4f}, {r['hi']:.4f}]"
            if "p_two" in r:
                line += f"  p = {r['p_two']:.4f}"
            lines.append(line)
        return "\n".join(lines)


class BootstrapResult:
    """``figures`` (R + 1, F) float64 on the device, row R the point estimate; ``names`` the F figures; ``state`` the integer states
    (R + 1, 3 C + 2) of a decision result (None for a ranking result); ``owner`` the ``Bootstrap`` that made it."""

    def __init__(self, owner, kind, figures, names, state=None, shape=None):
        self.owner, self.kind, self.figures, self.names, self.state, self.shape = owner, kind, figures, tuple(names), state, shape

    @property
    def table(self):
        """the figures in their report's own shape: (R + 1, C + 1, 6) for a ranking result"""
        return self.figures if self.shape is None else self.figures.view(self.figures.shape[0], *self.shape)

    def summary(self, alpha=0.05):
        """``BootstrapSummary`` (F, 6): one ``mmda_boot_summary`` launch, nothing read back."""
        return self.owner._summary(self.figures, None, self.names, alpha)


class Bootstrap:
    """``Bootstrap(n, replicates=2000, seed=0, device="cuda")``: R resamples of n rows.  ``decisions(labels, truth)`` and
    ``ranking(scores, truth)`` resample a report over tables of n rows, ``compare(a, b)`` two results of THIS object over the same
    figures, replicate by replicate.  Every call queues its launches and returns device tensors; nothing is read back."""

    def __init__(self, n, replicates=2000, seed=0, device="cuda"):
        import torch
        step_rules.bootstrap_check(replicates=replicates, n=int(n))
        self.n, self.R, self.seed = int(n), int(replicates), int(seed) & ((1 << 64) - 1)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.MMDAError(f"Bootstrap resamples on the GPU only (the HIP path has no CPU fallback), not on {self.device}")

    def _tables(self, a, b, who, rank=False):
        a, b = _lib.device_tables(a, b, who, f"{who}: the two tables", "(n, C)")
        if a.shape[0] != self.n:
            raise ValueError(f"{who}: the tables have {a.shape[0]} rows, this Bootstrap resamples n = {self.n}")
        step_rules.bootstrap_check(replicates=self.R, n=self.n, C=int(a.shape[1]), rank=rank)
        return a, b

    def decisions(self, labels, truth, form="auto"):
        """The decision figures of labels / truth (n, C) on the device under every replicate: a pack launch, the count launch
        (``form``: "auto", "lds" or "global" -- the states do not depend on it) and the figure launch."""
        import torch
        if form not in FORMS:
            raise ValueError(f"form must be one of {tuple(FORMS)}, not {form!r}")
        p, y = self._tables(labels, truth, "Bootstrap.decisions")
        C, lib, st = int(p.shape[1]), _lib.load(), _lib.stream_ptr()
        codes = torch.empty(self.n, dtype=torch.int32, device=p.device)
        state = torch.empty(self.R + 1, 3 * C + 2, dtype=torch.int64, device=p.device)
        figures = torch.empty(self.R + 1, 10 + 3 * C, dtype=torch.float64, device=p.device)
        _lib.check(lib.mmda_boot_pack(p.data_ptr(), y.data_ptr(), self.n, C, codes.data_ptr(), st), "mmda_boot_pack")
        _lib.check(lib.mmda_boot_counts(codes.data_ptr(), self.n, C, self.R, self.seed, FORMS[form], state.data_ptr(), st), "mmda_boot_counts")
        _lib.check(lib.mmda_boot_figures(state.data_ptr(), C, self.R, figures.data_ptr(), st), "mmda_boot_figures")
        return BootstrapResult(self, ("decisions", C), figures, decision_names(C), state)

    @staticmethod
    def sorted_tables(s, t):
        """Once per table, torch plumbing on the device: the int32 (C, n) tables ``mmda_boot_rank`` reads -- ``inv`` (row -> sorted
        position, descending score in ``ranking.score_keys``' order: a NaN counts as -inf, -0 == +0), ``first`` / ``last`` (the tie
        group of every position) and ``pos`` (the row at the position is a positive)."""
        import torch
        n, C = s.shape
        s = torch.where(torch.isnan(s), torch.full_like(s, float("-inf")), s) + 0.0        # NaN -> -inf, -0 -> +0
        vals, perm = torch.sort(s, dim=0, descending=True, stable=True)
        idx = torch.arange(n, device=s.device).unsqueeze(1).expand(n, C)
        new = torch.ones(n, C, dtype=torch.bool, device=s.device)
        new[1:] = vals[1:] != vals[:-1]
        end = torch.ones(n, C, dtype=torch.bool, device=s.device)
        end[:-1] = new[1:]
        first = torch.cummax(torch.where(new, idx, torch.zeros_like(idx)), dim=0).values
        last = torch.cummin(torch.where(end, idx, torch.full_like(idx, n - 1)).flip(0), dim=0).values.flip(0)
        inv = torch.empty_like(idx, memory_format=torch.contiguous_format)
        inv.scatter_(0, perm, idx.contiguous())
        pos = torch.gather(t > 0, 0, perm)
        return tuple(x.t().to(torch.int32).contiguous() for x in (inv, first, last, pos))

    def ranking(self, scores, truth, tpr=0.95, failure=False):
        """The ranking figures of scores / truth (n, C) under every replicate, n <= 16384: the sort (once per table), then one
        workgroup per (replicate, class).  ``failure=True``: the table is a confidence table against "was the decision correct" and the
        figures take ``FailurePrediction.as_dict``'s names."""
        import torch
        s, t = self._tables(scores, truth, "Bootstrap.ranking", rank=True)
        if not 0.0 < tpr <= 1.0:
            raise ValueError(f"tpr must be in (0, 1], not {tpr}")
        C = int(s.shape[1])
        inv, first, last, pos = self.sorted_tables(s, t)
        out = torch.empty(self.R + 1, C + 1, 6, dtype=torch.float64, device=s.device)
        _lib.check(_lib.load().mmda_boot_rank(inv.data_ptr(), first.data_ptr(), last.data_ptr(), pos.data_ptr(), self.n, C, self.R, self.seed,
                                              float(tpr), out.data_ptr(), _lib.stream_ptr()), "mmda_boot_rank")
        kind = ("failure" if failure else "ranking", C, float(tpr))
        return BootstrapResult(self, kind, out.view(self.R + 1, (C + 1) * 6), ranking_names(C, failure, tpr), None, (C + 1, 6))

    def _summary(self, a, b, names, alpha):
        import torch
        q_lo, q_hi = _quantiles(alpha)
        F, ncols = int(a.shape[1]), 6 if b is None else 9
        out = torch.empty(F, ncols, dtype=torch.float64, device=a.device)
        _lib.check(_lib.load().mmda_boot_summary(a.data_ptr(), None if b is None else b.data_ptr(), self.R, F, q_lo, q_hi, ncols,
                                                 out.data_ptr(), _lib.stream_ptr()), "mmda_boot_summary")
        return BootstrapSummary(out, names, SUMMARY_COLUMNS if b is None else COMPARE_COLUMNS, alpha)

    def compare(self, a, b, alpha=0.05):
        """The paired comparison of two results of this object over the same figures: ``BootstrapSummary`` (F, 9) of ``delta_r = a_r -
        b_r`` (NaN where either side is), with ``p_le = (1 + #{delta <= 0}) / (m + 1)``, ``p_ge`` likewise and ``p_two = min(1, 2
        min(p_le, p_ge))`` over the m defined deltas."""
        why = None
        if not (isinstance(a, BootstrapResult) and isinstance(b, BootstrapResult)):
            why = "both arguments must be BootstrapResults"
        elif a.owner is not self or b.owner is not self:
            why = "a result comes from a different Bootstrap (its resamples are not these)"
        elif a.kind != b.kind or a.names != b.names:
            why = f"the figure sets differ ({a.kind} and {b.kind})"
        step_rules.bootstrap_check(replicates=self.R, n=self.n, compare=why)
        return self._summary(a.figures, b.figures, a.names, alpha)
