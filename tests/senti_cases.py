"""The sentiment task: restatements, case tables and bounds of tests/test_senti_cpu.py and tests/test_gpu_senti.py.
Importable without a GPU.

The collector (mmda_amd/csrc/senti.hip) restated in numpy:
  state_numpy      the state of mmda_senti_accumulate over a sequence of batches, the float64 sums added in the kernel's own order --
                   thread (row stride 256 x workgroups), the wave's xor butterfly (a balanced pairwise tree), waves in order, workgroups in
                   order -- so that a device state can be compared with it bit for bit
  finish_numpy     mmda_senti_finish's arithmetic on a state
The definition, for the bounds of the three figures that are sums of rounded terms (mae, mae_intensity, corr):
  definition(pred, truth, dtype)   np.mean / np.corrcoef's formulas in `dtype`; np.longdouble is the truth, np.float64 numpy's own
  bound = FACTOR * max(|definition_f64 - truth|, FLOOR_ULP ulp of the value)       (tests/test_gpu_losses.py's rule: 8 x the reference's
  own error; the floor keeps a zero yardstick from demanding exactness)
The ratio figures (acc7, acc5, acc2, acc2_non0, f1, f1_non0) are functions of integer counts: one IEEE division (the F1s: two divisions,
two products, one sum and one division), held to RATIO_ULP ulp of the fixture's float64.

The criterion and the head (mmda_amd/csrc/loss_terms.h) restated in torch, in whatever dtype the inputs have:
  reg_value / reg_grad     mean_b |s - y| or (s - y)^2 and its gradient sign(s - y) / B (0 at s == y) or 2 (s - y) / B
  head_fwd / head_bwd      tcp = sigmoid(z[:, :6]); scores = z[:, 6:] * mask (no sigmoid); dz = d * mask (no s (1 - s))
"""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "senti", "senti_cases.npz")
RATIOS_JSON = os.path.join(HERE, "golden", "senti_error_ratios.json")

FIGURES = ("mae", "corr", "acc7", "acc5", "acc2", "f1", "acc2_non0", "f1_non0", "mae_intensity")
SUMMED = ("mae", "corr", "mae_intensity")                  # held by the yardstick; the others are ratios of counts
FACTOR, FLOOR_ULP, RATIO_ULP = 8.0, 4.0, 1.0
THREADS, GRID_CAP, WAVE = 256, 32, 64
NI, NF, F0, WORDS = 13, 7, 16, 24
SPLITS = (None, 1, 7, 64)                                  # one batch; batches of 1, 7 and 64 rows, the last one partial


def load_fixture():
    """{name: (pred f32, truth f32, {figure: float64})} in the fixture's order"""
    z = np.load(FIXTURE)
    keys = [str(k) for k in z["keys"]]
    return {str(n): (z[f"{n}/pred"], z[f"{n}/truth"], dict(zip(keys, z[f"{n}/figures"].tolist()))) for n in z["names"]}


def batches(n, size):
    return [(0, n)] if size is None else [(lo, min(lo + size, n)) for lo in range(0, n, size)]


# ------------------------------------------------------------------------------------------------ the collector
def _row_terms(p32, t32):
    p, t = p32.astype(np.float64), t32.astype(np.float64)
    ad = np.abs(p - t)
    ext = np.abs(t32) > 2
    return np.stack([ad, np.where(ext, ad, 0.0), p, t, p * p, t * t, p * t])


def _counts(p32, t32):
    c = np.zeros(NI, dtype=np.int64)
    non0 = t32 != 0
    c[0], c[1] = p32.size, non0.sum()
    r = lambda x, lim: np.rint(np.clip(x, -lim, lim))
    c[2] = (r(p32, 3.0) == r(t32, 3.0)).sum()
    c[3] = (r(p32, 2.0) == r(t32, 2.0)).sum()
    for tb in (0, 1):
        for pb in (0, 1):
            c[4 + 2 * tb + pb] = (((t32 >= 0) == bool(tb)) & ((p32 >= 0) == bool(pb))).sum()
            c[8 + 2 * tb + pb] = (non0 & ((t32 > 0) == bool(tb)) & ((p32 > 0) == bool(pb))).sum()
    c[12] = (np.abs(t32) > 2).sum()
    return c


def _launch_sums(p32, t32):
    """the seven float64 sums one launch adds to the state, in the kernel's order"""
    n = p32.size
    blocks = min((n + THREADS - 1) // THREADS, GRID_CAP)
    terms = _row_terms(p32, t32)
    total = np.zeros(NF)
    for b in range(blocks):
        thread = np.zeros((NF, THREADS))
        for i0 in range(b * THREADS, n, blocks * THREADS):          # a thread adds its rows in row order
            w = min(THREADS, n - i0)
            thread[:, :w] = thread[:, :w] + terms[:, i0:i0 + w]
        part = np.zeros(NF)
        for wv in range(THREADS // WAVE):                            # waves in order, each a balanced pairwise tree over its lanes
            v = thread[:, wv * WAVE:(wv + 1) * WAVE]
            while v.shape[1] > 1:
                v = v[:, 0::2] + v[:, 1::2]
            part = part + v[:, 0]
        total = total + part                                         # workgroups in order
    return total


def state_numpy(pred, truth, split=None):
    """(counts int64 (13,), sums float64 (7,)) after the batches of `split` rows each"""
    p32, t32 = np.asarray(pred, np.float32).reshape(-1), np.asarray(truth, np.float32).reshape(-1)
    c, f = np.zeros(NI, dtype=np.int64), np.zeros(NF)
    for lo, hi in batches(p32.size, split):
        c += _counts(p32[lo:hi], t32[lo:hi])
        f = f + _launch_sums(p32[lo:hi], t32[lo:hi])
    return c, f


def _weighted_f1(T):
    tn, fp, fn, tp = (float(x) for x in T)
    true0, true1 = tn + fp, fn + tp
    den0, den1 = true0 + (tn + fn), true1 + (fp + tp)
    f0 = 2.0 * tn / den0 if den0 > 0 else 0.0
    f1 = 2.0 * tp / den1 if den1 > 0 else 0.0
    with np.errstate(all="ignore"):
        return float(np.float64(f0 * true0 + f1 * true1) / np.float64(true0 + true1))


def finish_numpy(counts, sums):
    """the nine figures from a state, mmda_senti_finish's expressions in float64"""
    c = [float(x) for x in counts]
    s = [np.float64(x) for x in sums]
    n, n0, next_ = np.float64(c[0]), np.float64(c[1]), np.float64(c[12])
    with np.errstate(all="ignore"):
        num = n * s[6] - s[2] * s[3]
        vp, vt = n * s[4] - s[2] * s[2], n * s[5] - s[3] * s[3]
        r = num / (np.sqrt(vp) * np.sqrt(vt))
        r = min(r, 1.0) if r > 1.0 else max(r, -1.0) if r < -1.0 else r
        out = dict(mae=s[0] / n, corr=r, acc7=np.float64(c[2]) / n, acc5=np.float64(c[3]) / n, acc2=np.float64(c[4] + c[7]) / n,
                   f1=_weighted_f1(counts[4:8]), acc2_non0=np.float64(c[8] + c[11]) / n0, f1_non0=_weighted_f1(counts[8:12]),
                   mae_intensity=s[1] / next_)
    return {k: float(v) for k, v in out.items()}


def definition(pred, truth, dtype):
    """mae, mae_intensity, corr by eval_mosei_senti's definitions (np.mean, np.corrcoef's centred products) evaluated in `dtype`"""
    p, t = np.asarray(pred, np.float32).astype(dtype), np.asarray(truth, np.float32).astype(dtype)
    with np.errstate(all="ignore"):
        ad = np.abs(p - t)
        ext = np.abs(t) > 2
        mae = ad.sum() / dtype(p.size)
        mae_i = ad[ext].sum() / dtype(ext.sum()) if ext.any() else dtype(np.nan)
        dp, dt = p - p.sum() / dtype(p.size), t - t.sum() / dtype(t.size)
        corr = (dp * dt).sum() / np.sqrt((dp * dp).sum() * (dt * dt).sum()) if p.size > 1 else dtype(np.nan)
    return dict(mae=mae, mae_intensity=mae_i, corr=corr)


def ulp(x):
    return float(np.spacing(np.abs(np.float64(x)))) if np.isfinite(x) else float("nan")


def summed_bound(pred, truth, key, fixture_value):
    """(truth in longdouble, bound): FACTOR x float64 numpy's distance from the longdouble definition, floored at FLOOR_ULP ulp.  The
    float64 side is the fixture's own figure: the reference's np.mean / np.corrcoef on these rows."""
    tr = definition(pred, truth, np.longdouble)[key]
    e = abs(float(np.longdouble(fixture_value) - tr))
    return tr, FACTOR * max(e, FLOOR_ULP * ulp(float(tr)))


def check_figures(name, got, pred, truth, want, lines=None):
    """every figure of `got` against the fixture's `want`; returns the list of failures (each figure is appended to `lines` first)"""
    bad = []
    for k in FIGURES:
        g, w = float(got[k]), float(want[k])
        if np.isnan(w) or np.isnan(g):
            ok, note = bool(np.isnan(w) and np.isnan(g)), "nan"
        elif k in SUMMED:
            tr, bound = summed_bound(pred, truth, k, w)
            err = abs(float(np.longdouble(g) - tr))
            ok, note = err <= bound, f"err {err:.3e} bound {bound:.3e}"
        else:
            err = abs(g - w)
            ok, note = err <= RATIO_ULP * ulp(w), f"err {err / ulp(w) if w else err:.2f} ulp"
        if lines is not None:
            lines.append(f"{name:28s} {k:14s} got {g!r:24} want {w!r:24} {note}")
        if not ok:
            bad.append(f"{name}: {k} = {g!r}, the fixture has {w!r} ({note})")
    return bad


# ------------------------------------------------------------------------------------------------ criterion and head
KINDS = ("l1", "mse")


def reg_value(s, y, kind):
    d = s.reshape(-1) - y.reshape(-1).to(s.dtype)
    return (d.abs() if kind == "l1" else d * d).mean()


def reg_grad(s, y, kind, scale=1.0):
    """scale * d reg_value / d s by the closed form, in s.dtype (sign(0) = 0: torch's l1_loss backward)"""
    d = s - y.reshape(s.shape).to(s.dtype)
    g = torch.sign(d) if kind == "l1" else 2.0 * d
    return scale * g / s.numel()


def head_fwd(z, mask, threshold):
    """(tcp, scores, labels) of logits (B, 6 + ncls) under the class-score dropout multipliers `mask` (B, ncls)"""
    tcp = torch.sigmoid(z[:, :6])
    scores = z[:, 6:] * mask.to(z.dtype)
    return tcp, scores, (scores > threshold).to(z.dtype)


def head_bwd(tcp, mask, dtcp, dscores):
    return torch.cat([dtcp * tcp * (1.0 - tcp), dscores * mask.to(dscores.dtype)], dim=1)


OP_BATCHES = (1, 5, 33, 300)                               # under a wave; a partial block; B (6 + 1) = 2100 elements: nine blocks of 256
E32_FLOOR = 2.0 ** -24


def op_inputs(B, seed):
    """logits (B, 7) float32, targets (B,) on the thirds grid, with rows planted so that the output equals the target exactly"""
    g = torch.Generator().manual_seed(4100 + 7 * B + seed)
    z = torch.randn(B, 7, generator=g) * 1.5
    y = torch.randint(-9, 10, (B,), generator=g).float() / 3.0
    y[torch.rand(B, generator=g) < 0.15] = 0.0
    return z, y


# ------------------------------------------------------------------------------------------------ the rules table (section 1 of the issue)
# (keyword arguments of step_rules.task_verdict under task='sentiment', the rule that must refuse them)
REFUSED = [
    (dict(task="regression"), "task_name"),
    (dict(senti_loss="huber"), "senti_loss"),
    (dict(num_classes=6), "senti_classes"),
    (dict(num_classes=2), "senti_classes"),
    (dict(use_confidNet=True), "senti_confid"),
    (dict(pos_weight=[2.0]), "senti_pos_weight"),
    (dict(pos_weight="balanced"), "senti_pos_weight"),
    (dict(focal_gamma=2.0), "senti_focal"),
    (dict(calibrate="global"), "senti_calibrate"),
    (dict(calibrate="per_class"), "senti_calibrate"),
    (dict(rank=True), "senti_rank"),
    (dict(select_by="map"), "senti_select_by"),
    (dict(select_by="auroc"), "senti_select_by"),
]
ALLOWED = [dict(), dict(senti_loss="mse"), dict(focal_gamma=0), dict(focal_gamma=0.0, pos_weight=None), dict(calibrate="none"),
           dict(select_by="valid_loss"), dict(rank=False)]
