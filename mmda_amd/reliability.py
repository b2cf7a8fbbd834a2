"""Probability calibration: are the numbers of a score table probabilities.

**Reliability** (the report).  ``prob`` (N, C) fp32, ``y = target > 0``.  A NaN counts in ``n_nan[c]`` and nowhere else; any other
value is clamped to [0, 1].  Its bin of ``M`` is ``j = min(M - 1, int(p * float32(M)))``: one fp32 multiply, truncated.  Per (class,
bin) three unsigned integers -- ``cnt``, ``pos`` and ``sum_p = sum rint(p 2^40)`` -- and per class two float64 sums, ``sum_sq = sum
(p - y)^2`` and ``sum_nll = -sum [y max(log p, -100) + (1 - y) max(log(1 - p), -100)]`` (``BCELoss``'s clamp).  From them, per class,
as the mean over the classes (row C) and over all classes pooled (row C + 1), the columns ``FIGURES``:

  ``ece``  ``sum_j |pos_j 2^40 - sum_p_j| / (2^40 n)``        ``mce``  ``max_j |pos_j 2^40 - sum_p_j| / (2^40 cnt_j)``

exact integers and one division, so with the diagram ``(C, M, 3) = {cnt, pos / cnt, sum_p / (2^40 cnt)}`` they do not depend on the
order of arrival or on how the rows are split into batches.  ``brier = sum_sq / n``, ``nll = sum_nll / n``; ``n = 0`` gives NaN.

**Scaling** (the fit).  ``q = sigmoid(a z + b)`` with ``z = log p' - log1p(-p')`` in float64 of the fp32 score clamped to
``[2^-23, 1 - 2^-23]``.  ``how="temperature"`` fits ``a`` alone (Guo et al.'s 1 / T), ``"platt"`` ``a`` and ``b``; ``per_class``: one
group per class, else one group of all classes.  A group's parameters minimise its mean NLL (convex) by a damped Newton iteration
whose state stays on the device; ``status`` 0 converged (``max |d NLL / d theta| <= 1e-12``), 1 degenerate (no positive or no
negative: ``(1, 0)``), 2 not converged in ``max_iter`` (separable data drifts to infinity; the last accepted point).

The host functions (plain numpy float64) define the quantities and are the yardstick of the tests; ``ReliabilityEval`` /
``reliability_metrics`` / ``fit_scaling`` / ``Scaling.apply`` compute the same on the device (``mmda_reliab_accumulate``,
``mmda_reliab_finish``, ``mmda_scaling_fit``, ``mmda_scaling_apply``) and read nothing back.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .utils.eval import host_tables

MAX_CLASSES, MAX_BINS, MAX_ROWS = 16, 64, 1 << 20
FIX = 1 << 40
FIGURES = ("n", "n_nan", "base_rate", "mean_p", "ece", "mce", "brier", "nll")
HOWS = tuple(_lib.SCALING_HOW)
STATUS = {0: "converged", 1: "degenerate", 2: "not converged"}
ROWS_PER_WG = 16                                                 # reliab.hip: a workgroup is 16 rows x 16 class lanes
P_LO, P_HI = np.float32(2.0 ** -23), np.float32(1.0 - 2.0 ** -23)
G_TOL, LAM0, LAM_MIN_UP, DIAG_FLOOR, RISE = 1e-12, 1e-2, 1e-3, 1e-6, 2.0 ** -43   # reliab.hip: SC_*


def state_words(C, M):
    """MMDA_RELIAB_STATE_WORDS"""
    return 2 + 3 * C + 3 * C * M


def check_shape(C, M=None):
    if not 1 <= C <= MAX_CLASSES:
        raise ValueError(f"a probability table must have 1 .. {MAX_CLASSES} classes, not {C}")
    if M is not None and not 1 <= M <= MAX_BINS:
        raise ValueError(f"bins must be in 1 .. {MAX_BINS}, not {M}")


def check_how(how):
    if how not in _lib.SCALING_HOW:
        raise ValueError(f"how must be one of {HOWS}, not {how!r}")
    return how


# ---------------------------------------------------------------------------------------------------- host (numpy): the report
def clean(prob):
    """(p float32 clamped to [0, 1] with -0 -> 0 and NaN -> 0, nan mask)"""
    p = np.asarray(prob, dtype=np.float32)
    nan = np.isnan(p)
    p = np.where(nan | ~(p > 0), np.float32(0), np.minimum(p, np.float32(1))).astype(np.float32)
    return p, nan


def bin_index(p32, M):
    return np.minimum(M - 1, (np.asarray(p32, np.float32) * np.float32(M)).astype(np.int32))


def elementwise_host(prob, target):
    """(sq, nll) float64 (N, C): the terms of the two sums, 0 at a NaN."""
    p32, y = host_tables(prob, target, "prob and target")
    p32, nan = clean(p32)
    p = p32.astype(np.float64)
    with np.errstate(divide="ignore"):
        term = -np.maximum(np.where(y, np.log(p), np.log(1.0 - p)), -100.0)
    d = p - y.astype(np.float64)
    return np.where(nan, 0.0, d * d), np.where(nan, 0.0, term)


def state_host(prob, target, bins=15):
    """The state of host arrays as a dict: ``cnt``, ``pos``, ``sum_p`` (C, M) uint64, ``n_nan`` (C,) uint64, ``sum_sq``, ``sum_nll``
    (C,) float64 (numpy's own summation order)."""
    p32, y = host_tables(prob, target, "prob and target")
    N, C = p32.shape
    check_shape(C, bins)
    p32, nan = clean(p32)
    j = bin_index(p32, bins)
    fixed = np.rint(p32.astype(np.float64) * float(FIX)).astype(np.uint64)
    cnt, pos, sum_p = (np.zeros((C, bins), dtype=np.uint64) for _ in range(3))
    for c in range(C):
        ok = ~nan[:, c]
        cnt[c] = np.bincount(j[ok, c], minlength=bins)
        pos[c] = np.bincount(j[ok & y[:, c], c], minlength=bins)
        for b in range(bins):
            sum_p[c, b] = fixed[ok & (j[:, c] == b), c].sum(dtype=np.uint64)
    sq, nll = elementwise_host(prob, target)
    return dict(cnt=cnt, pos=pos, sum_p=sum_p, n_nan=nan.sum(0).astype(np.uint64), sum_sq=sq.sum(0), sum_nll=nll.sum(0))


def unpack_state(words, C, M):
    """The device state (int64 words read back) as ``state_host``'s dict, and the ticket."""
    w = np.ascontiguousarray(np.asarray(words).reshape(-1)).view(np.uint64)
    if w.shape[0] != state_words(C, M):
        raise ValueError(f"a state of {C} classes and {M} bins has {state_words(C, M)} words, not {w.shape[0]}")
    cells = w[2 + 3 * C:].reshape(C, M, 3)
    sums = w[2 + C:2 + 3 * C].view(np.float64)
    return dict(cnt=cells[..., 0].copy(), pos=cells[..., 1].copy(), sum_p=cells[..., 2].copy(), n_nan=w[2:2 + C].copy(),
                sum_sq=sums[:C].copy(), sum_nll=sums[C:].copy()), int(w[0])


def ordered_sum(terms, state=None):
    """(C,) float64: ``state + `` the sum of ``terms`` (N, C) over the rows in the order ``mmda_reliab_accumulate`` adds one batch --
    thread (r, c) of workgroup b adds rows ``16 (b + k grid) + r`` in row order, a class's row lanes are added ``(r0 + r1) + (r2 + r3)``
    per wave and the four waves in order, the workgroups' partials in workgroup order."""
    t = np.asarray(terms, dtype=np.float64)
    N, C = t.shape
    out = np.zeros(C) if state is None else np.asarray(state, dtype=np.float64).copy()
    if N == 0:
        return out
    grid = min(_lib.RELIAB_GRID_CAP, -(-N // ROWS_PER_WG))
    stride = grid * ROWS_PER_WG
    K = -(-N // stride)
    pad = np.zeros((K * stride, C))
    pad[:N] = t
    pad = pad.reshape(K, grid, ROWS_PER_WG, C)
    thread = np.zeros((grid, ROWS_PER_WG, C))
    for k in range(K):
        thread = thread + pad[k]
    wave = (thread[:, 0::4] + thread[:, 1::4]) + (thread[:, 2::4] + thread[:, 3::4])      # [:, w]: the row lanes 4 w + {0, 1, 2, 3} of wave w
    part = np.zeros((grid, C))
    for w in range(4):
        part = part + wave[:, w]
    total = np.zeros(C)
    for b in range(grid):
        total = total + part[b]
    return out + total


def _row(cnt, pos, sum_p, n_nan, sum_sq, sum_nll):
    cnt, pos, sum_p = ([int(x) for x in v] for v in (cnt, pos, sum_p))
    n, npos, sp = sum(cnt), sum(pos), sum(sum_p)
    nan = float("nan")
    if n == 0:
        return [0.0, float(n_nan)] + [nan] * 6
    gaps = [abs(a * FIX - b) for a, b in zip(pos, sum_p)]
    mce = max(float(d) / float(FIX * k) for d, k in zip(gaps, cnt) if k)
    return [float(n), float(n_nan), float(npos) / float(n), float(sp) / float(FIX * n), float(sum(gaps)) / float(FIX * n), mce,
            float(sum_sq) / float(n), float(sum_nll) / float(n)]


def figures_from_state(st):
    """``(figures (C + 2, 8), diagram (C, M, 3))`` float64 from a state dict: the class rows, the means over the classes where a column
    is not NaN (added in class order; NaN where none is), the pooled row."""
    C, M = st["cnt"].shape
    fig = np.full((C + 2, len(FIGURES)), np.nan)
    for c in range(C):
        fig[c] = _row(st["cnt"][c], st["pos"][c], st["sum_p"][c], st["n_nan"][c], st["sum_sq"][c], st["sum_nll"][c])
    for f in range(len(FIGURES)):
        total, k = 0.0, 0
        for c in range(C):
            if not np.isnan(fig[c, f]):
                total, k = total + fig[c, f], k + 1
        fig[C, f] = total / k if k else np.nan
    pool = lambda key: [sum(int(st[key][c, j]) for c in range(C)) for j in range(M)]
    sq = nll = 0.0
    for c in range(C):
        sq, nll = sq + float(st["sum_sq"][c]), nll + float(st["sum_nll"][c])
    fig[C + 1] = _row(pool("cnt"), pool("pos"), pool("sum_p"), sum(int(x) for x in st["n_nan"]), sq, nll)
    diagram = np.full((C, M, 3), np.nan)
    for c in range(C):
        for j in range(M):
            k = int(st["cnt"][c, j])
            diagram[c, j, 0] = float(k)
            if k:
                diagram[c, j, 1] = float(int(st["pos"][c, j])) / float(k)
                diagram[c, j, 2] = float(int(st["sum_p"][c, j])) / float(FIX * k)
    return fig, diagram


def reliability_host(prob, target, bins=15):
    """``(figures, diagram)`` of host arrays: the definition."""
    return figures_from_state(state_host(prob, target, bins))


# ---------------------------------------------------------------------------------------------------- host (numpy): the fit
def logit_host(scores):
    """z float64 of fp32 scores; NaN stays NaN."""
    p = np.asarray(scores, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        pc = np.where(np.isnan(p), p, np.minimum(np.maximum(p, P_LO), P_HI)).astype(np.float64)
    return np.log(pc) - np.log1p(-pc)


def nll_sums_host(z, y, a, b):
    """(NLL, g_a, g_b, H_aa, H_ab, H_bb) SUMS over the elements z (float64, no NaN), y (bool) at (a, b)."""
    t = a * z + b
    e = np.exp(-np.abs(t))
    d = 1.0 / (1.0 + e)
    q = np.where(t >= 0.0, d, e * d)
    w = e * d * d
    r = q - y.astype(np.float64)
    loss = np.maximum(np.where(y, -t, t), 0.0) + np.log1p(e)
    return np.array([loss.sum(), (r * z).sum(), r.sum(), (w * z * z).sum(), (w * z).sum(), w.sum()])


def _groups(scores, truth, per_class):
    s, y = host_tables(scores, truth, "prob and target")
    z = logit_host(s)
    cols = [[c] for c in range(s.shape[1])] if per_class else [list(range(s.shape[1]))]
    out = []
    for g in cols:
        zz, yy = z[:, g].reshape(-1), y[:, g].reshape(-1)
        ok = ~np.isnan(zz)
        out.append((g, zz[ok], yy[ok]))
    return out


def mean_nll_host(scores, truth, a, b, per_class):
    """Per group ``(mean NLL, gradient (2,), Hessian (2, 2))`` at the per-class parameters ``a``, ``b`` (a group's first class's)."""
    out = []
    for g, z, y in _groups(scores, truth, per_class):
        f, ga, gb, haa, hab, hbb = nll_sums_host(z, y, float(a[g[0]]), float(b[g[0]])) / max(1, z.shape[0])
        out.append((f, np.array([ga, gb]), np.array([[haa, hab], [hab, hbb]])))
    return out


def _lm_update(s, tot, n, platt):
    """reliab.hip: scaling_update -- one damped Newton step of a group from the sums at its trial point."""
    f, ga, gb, haa, hab, hbb = (float(x) / n for x in tot)
    s["iterations"] += 1
    if f <= s["nll"] + abs(s["nll"]) * RISE:
        s.update(a=s["ta"], b=s["tb"], nll=f, g=(ga, gb), h=(haa, hab, hbb), lam=s["lam"] * 0.1)
        if (max(abs(ga), abs(gb)) if platt else abs(ga)) <= G_TOL:
            s["status"] = 0
            return
    else:
        s["lam"] = max(s["lam"] * 10.0, LAM_MIN_UP)
    lam, (ga, gb), (haa, hab, hbb) = s["lam"], s["g"], s["h"]
    daa = haa + lam * max(haa, DIAG_FLOOR)
    if not platt:
        s["ta"] = s["a"] - ga / daa
        return
    dbb = hbb + lam * max(hbb, DIAG_FLOOR)
    det = daa * dbb - hab * hab
    if det > 0.0:
        da, db = (dbb * ga - hab * gb) / det, (daa * gb - hab * ga) / det
    else:
        da, db = ga / daa, gb / dbb
    s["ta"], s["tb"] = s["a"] - da, s["b"] - db


def fit_scaling_host(scores, truth, how="temperature", per_class=False, max_iter=64):
    """``(a, b float64 (C,), status, iterations int32 (C,))`` of host arrays: the iteration of ``mmda_scaling_fit`` in numpy (its sums
    in numpy's order)."""
    check_how(how)
    s32, _ = host_tables(scores, truth, "prob and target")
    C = s32.shape[1]
    a, b = np.ones(C), np.zeros(C)
    status, iters = np.ones(C, np.int32), np.zeros(C, np.int32)
    for g, z, y in _groups(scores, truth, per_class):
        n, npos = z.shape[0], int(y.sum())
        st = dict(ta=1.0, tb=0.0, a=1.0, b=0.0, nll=float("inf"), lam=LAM0, g=(0.0, 0.0), h=(0.0, 0.0, 0.0), iterations=0,
                  status=1 if npos in (0, n) else 2)
        for _ in range(max_iter):
            if st["status"] != 2:
                break
            _lm_update(st, nll_sums_host(z, y, st["ta"], st["tb"]), float(n), how == "platt")
        a[g], b[g], status[g], iters[g] = st["a"], st["b"], st["status"], st["iterations"]
    return a, b, status, iters


def apply_host(scores, a, b):
    """float64 ``sigmoid(a_c z + b_c)`` of host arrays; NaN stays NaN."""
    t = np.asarray(a, np.float64)[None, :] * logit_host(scores) + np.asarray(b, np.float64)[None, :]
    with np.errstate(invalid="ignore"):
        e = np.exp(-np.abs(t))
        return np.where(t >= 0.0, 1.0 / (1.0 + e), e / (1.0 + e))


# ---------------------------------------------------------------------------------------------------- device
class ReliabilityResult:
    """``figures`` (C + 2, 8) float64, columns ``FIGURES``: the class rows, row C their means, row C + 1 all classes pooled;
    ``diagram`` (C, M, 3) float64 ``{cnt, pos / cnt, mean p}`` per bin.  On the device as ``ReliabilityEval.result`` returns it;
    ``cpu()`` reads back, ``as_dict()`` names the figures."""

    def __init__(self, figures, diagram):
        self.figures, self.diagram = figures, diagram

    @property
    def C(self):
        return int(self.figures.shape[0]) - 2

    @property
    def bins(self):
        return int(self.diagram.shape[1])

    def cpu(self):
        return ReliabilityResult(self.figures.cpu(), self.diagram.cpu())

    def as_dict(self):
        """Per-class lists under ``FIGURES``' names, ``macro_<figure>`` and ``pooled_<figure>``, ``bins`` and the ``diagram`` as nested
        lists.  Reads back what is still on the device."""
        r = self.cpu()
        f, C = r.figures.numpy(), self.C
        out = {name: f[:C, k].tolist() for k, name in enumerate(FIGURES)}
        for k, name in enumerate(FIGURES):
            out["macro_" + name], out["pooled_" + name] = float(f[C, k]), float(f[C + 1, k])
        out.update(bins=self.bins, diagram=r.diagram.tolist())
        return out


class ReliabilityEval:
    """The reliability state of a stream of batches: ``update(prob, target)`` per batch (one launch, no synchronisation),
    ``result()`` -> ``ReliabilityResult`` on the device (one launch, nothing read back)."""

    def __init__(self, num_classes, bins=15, device="cuda"):
        self.C, self.bins = int(num_classes), int(bins)
        check_shape(self.C, self.bins)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.MMDAError(f"ReliabilityEval counts on the GPU only (the HIP path has no CPU fallback), not on {self.device}")
        self._lib = _lib.load()
        self.state = torch.zeros(state_words(self.C, self.bins), dtype=torch.int64, device=self.device)
        self.rows = 0

    def reset(self):
        self.state.zero_()
        self.rows = 0
        return self

    def update(self, prob, target):
        p, t = _lib.device_tables(prob, target, "ReliabilityEval.update", "prob and target")
        if p.shape[1] != self.C:
            raise ValueError(f"prob and target must both be (N, {self.C}), not {tuple(p.shape)}")
        if self.rows + p.shape[0] > MAX_ROWS:
            raise ValueError(f"a reliability state takes at most 2^20 = {MAX_ROWS} rows, not {self.rows} + {p.shape[0]}")
        if p.shape[0]:                                               # an empty batch has no storage to point at, and adds nothing
            _lib.check(self._lib.mmda_reliab_accumulate(p.data_ptr(), t.data_ptr(), p.shape[0], self.C, self.bins, self.state.data_ptr(),
                                                        _lib.stream_ptr()), "mmda_reliab_accumulate")
        self.rows += int(p.shape[0])
        return self

    def update_result(self, result, truth):
        """The ``scores`` of an ``InferenceResult`` against ``truth`` (n, C)."""
        if result.scores is None:
            raise ValueError("update_result needs an InferenceResult with its 'scores' field")
        return self.update(result.scores, truth)

    def result(self):
        fig = torch.empty(self.C + 2, _lib.RELIAB_FIGURES, dtype=torch.float64, device=self.device)
        dia = torch.empty(self.C, self.bins, 3, dtype=torch.float64, device=self.device)
        _lib.check(self._lib.mmda_reliab_finish(self.state.data_ptr(), self.C, self.bins, fig.data_ptr(), dia.data_ptr(), _lib.stream_ptr()),
                   "mmda_reliab_finish")
        return ReliabilityResult(fig, dia)


def reliability_metrics(prob, target, bins=15):
    """``ReliabilityResult`` of device tables prob / target (N, C): two launches, no read-back."""
    p, t = _lib.device_tables(prob, target, "reliability_metrics", "prob and target")
    return ReliabilityEval(p.shape[1], bins, p.device).update(p, t).result()


class Scaling:
    """``q = sigmoid(a_c logit(p) + b_c)``: ``a``, ``b`` (C,) float64, ``status``, ``iterations`` (C,) int32 (a group's values repeated
    for its classes); on the device when they come from ``fit_scaling``.  ``Solver.eval(mode, scaling=...)`` scores with them."""

    def __init__(self, a, b, status=None, iterations=None, how=None, per_class=None):
        self.a = torch.as_tensor(a, dtype=torch.float64).reshape(-1)
        self.b = torch.as_tensor(b, dtype=torch.float64).reshape(-1)
        if self.a.shape != self.b.shape:
            raise ValueError(f"a and b must have one entry per class each, not {tuple(self.a.shape)} and {tuple(self.b.shape)}")
        zeros = lambda: torch.zeros(self.a.shape, dtype=torch.int32, device=self.a.device)
        self.status = zeros() if status is None else torch.as_tensor(status, dtype=torch.int32).reshape(-1)
        self.iterations = zeros() if iterations is None else torch.as_tensor(iterations, dtype=torch.int32).reshape(-1)
        self.how, self.per_class = how, per_class

    def __len__(self):
        return int(self.a.shape[0])

    def to(self, device):
        return Scaling(self.a.to(device), self.b.to(device), self.status.to(device), self.iterations.to(device), self.how, self.per_class)

    def cpu(self):
        return self.to("cpu")

    def save(self, path):
        torch.save(dict(a=self.a.cpu(), b=self.b.cpu(), status=self.status.cpu(), iterations=self.iterations.cpu(), how=self.how,
                        per_class=self.per_class), path)

    @classmethod
    def load(cls, path, device="cpu"):
        d = torch.load(path, map_location="cpu", weights_only=True)
        return cls(d["a"], d["b"], d.get("status"), d.get("iterations"), d.get("how"), d.get("per_class")).to(device)

    def apply(self, scores):
        """The scaled scores (N, C) fp32 of a device table, out of place: one launch."""
        if not (isinstance(scores, torch.Tensor) and scores.is_cuda):
            raise _lib.MMDAError("Scaling.apply needs a device tensor (the HIP path has no CPU fallback)")
        if scores.dim() != 2 or scores.shape[1] != len(self):
            raise ValueError(f"scores must be (N, {len(self)}), not {tuple(scores.shape)}")
        if scores.shape[0] > MAX_ROWS:
            raise ValueError(f"a score table of {scores.shape[0]} rows is over the limit of 2^20 = {MAX_ROWS} rows")
        s = scores.detach().to(torch.float32).contiguous()
        a, b = self.a.to(s.device).contiguous(), self.b.to(s.device).contiguous()
        out = torch.empty_like(s)
        if s.shape[0]:
            _lib.check(_lib.load().mmda_scaling_apply(s.data_ptr(), a.data_ptr(), b.data_ptr(), s.shape[0], s.shape[1], out.data_ptr(),
                                                      _lib.stream_ptr()), "mmda_scaling_apply")
        return out


def fit_scaling(scores, truth, how="temperature", per_class=False, max_iter=64):
    """``Scaling`` on the device that minimises the mean NLL of ``truth > 0`` under ``sigmoid(a logit(scores) + b)``: a clear, a
    prepare launch and ``max_iter`` iteration launches on the current stream, nothing read back."""
    check_how(how)
    if isinstance(max_iter, bool) or not 1 <= int(max_iter) <= _lib.SCALING_MAX_ITER:
        raise ValueError(f"max_iter must be in 1 .. {_lib.SCALING_MAX_ITER}, not {max_iter!r}")
    s, t = _lib.device_tables(scores, truth, "fit_scaling", "prob and target")
    N, C = s.shape
    check_shape(C)
    if N > MAX_ROWS:
        raise ValueError(f"a score table of {N} rows is over the limit of 2^20 = {MAX_ROWS} rows")
    if N == 0:                                                       # no row: every group is degenerate, nothing is launched
        one = torch.ones(C, dtype=torch.float64, device=s.device)
        return Scaling(one, torch.zeros_like(one), torch.ones(C, dtype=torch.int32, device=s.device), None, how, bool(per_class))
    lib = _lib.load()
    nbytes = lib.mmda_scaling_work_bytes(N, C)
    work = torch.empty(nbytes // 8, dtype=torch.float64, device=s.device)
    a, b = torch.ones(C, dtype=torch.float64, device=s.device), torch.zeros(C, dtype=torch.float64, device=s.device)
    status, iters = torch.ones(C, dtype=torch.int32, device=s.device), torch.zeros(C, dtype=torch.int32, device=s.device)
    _lib.check(lib.mmda_scaling_fit(s.data_ptr(), t.data_ptr(), N, C, _lib.SCALING_HOW[how], int(bool(per_class)), int(max_iter),
                                    work.data_ptr(), nbytes, a.data_ptr(), b.data_ptr(), status.data_ptr(), iters.data_ptr(),
                                    _lib.stream_ptr()), "mmda_scaling_fit")
    return Scaling(a, b, status, iters, how, bool(per_class))
