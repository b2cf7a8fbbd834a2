"""The case rows and generators shared by tests/test_reliability_cpu.py and tests/test_gpu_reliability.py (not a test file)."""
import numpy as np

from mmda_amd import reliability as rel

GRID_STRIDE = 16 * 32                                            # rows one launch covers before a workgroup strides
COLLECTOR_N = (1, 63, 64, 65, 255, 256, 257, GRID_STRIDE - 1, GRID_STRIDE, GRID_STRIDE + 1)
COLLECTOR_C = (1, 6, 16)
COLLECTOR_M = (1, 2, 15, 64)
FIT_N = (4, 65, 257, 1871)
FIT_C = (1, 6)
FIT_TRUE = ((1.0, 0.0), (0.5, 0.7), (2.5, -1.0), (0.2, 0.0))     # (a0, b0): scores = sigmoid((z* - b0) / a0)
FIT_COMBOS = (("temperature", False), ("temperature", True), ("platt", False), ("platt", True))
SPECIALS = np.array([0.0, 1.0, -0.0, np.nan, -0.25, 1.5], dtype=np.float32)


def edge_values(M):
    """every fp32 bin edge float32(k / M), k = 0 .. M, and its two fp32 neighbours"""
    e = (np.arange(M + 1, dtype=np.float64) / M).astype(np.float32)
    return np.concatenate([e, np.nextafter(e, np.float32(-1)), np.nextafter(e, np.float32(2))]).astype(np.float32)


def prob_table(N, C, M, seed):
    """(prob (N, C) fp32, target (N, C) fp32): uniform draws mixed with the bin edges and their neighbours, the special values and
    values below 2^-17; targets of both kinds written in several ways (> 0 is the positive)."""
    rng = np.random.default_rng(seed)
    p = rng.random((N, C), dtype=np.float32)
    pool = np.concatenate([edge_values(M), SPECIALS, (rng.random(8) * 2.0 ** -18).astype(np.float32),
                           np.array([1e-30, 2.0 ** -17, 2.0 ** -41, 1e-45], dtype=np.float32)])
    pick = rng.random((N, C)) < 0.45
    p[pick] = pool[rng.integers(0, pool.shape[0], int(pick.sum()))]
    t = rng.choice(np.array([0.0, 1.0, -1.0, 2.0, 0.5], dtype=np.float32), size=(N, C), p=[0.45, 0.35, 0.05, 0.05, 0.10])
    return p, t.astype(np.float32)


def ragged_splits(N, seed):
    """row ranges that cover 0 .. N in order, ragged, with one empty range among them"""
    rng = np.random.default_rng(seed)
    cuts = sorted(set(rng.integers(0, N + 1, 3).tolist()) | {0, N})
    ranges = [(a, b) for a, b in zip(cuts[:-1], cuts[1:])]
    ranges.insert(len(ranges) // 2, (ranges[0][1], ranges[0][1]))
    return ranges


def _separable(z, y):
    if y.all() or not y.any():
        return True
    return z[y].min() >= z[~y].max() or z[~y].min() >= z[y].max()


def min_eigenvalue(scores, truth, a, b, how, per_class):
    """the smallest eigenvalue, over the groups, of the mean-NLL Hessian in the fitted parameters at (a, b)"""
    out = np.inf
    for _, _, H in rel.mean_nll_host(scores, truth, a, b, per_class):
        out = min(out, float(H[0, 0]) if how == "temperature" else float(np.linalg.eigvalsh(H)[0]))
    return out


def fit_table(N, C, true, how, per_class, seed):
    """(scores (N, C) fp32, truth (N, C) fp32): y ~ Bernoulli(sigmoid(z*)), scores = sigmoid((z* - b0) / a0); the first draw in which
    no group is single-class or separable in z and the mean-NLL Hessian at the host optimum has no eigenvalue below 1e-3."""
    a0, b0 = true
    rng = np.random.default_rng(seed)
    for _ in range(4000):
        zs = rng.normal(0.0, 1.5, (N, C))
        y = rng.random((N, C)) < 1.0 / (1.0 + np.exp(-zs))
        s = (1.0 / (1.0 + np.exp(-(zs - b0) / a0))).astype(np.float32)
        z = rel.logit_host(s)
        groups = [(z[:, c], y[:, c]) for c in range(C)] if per_class else [(z.reshape(-1), y.reshape(-1))]
        if any(_separable(zz, yy) for zz, yy in groups):
            continue
        t = y.astype(np.float32)
        a, b, status, _ = rel.fit_scaling_host(s, t, how, per_class, 256)
        if (status == 0).all() and min_eigenvalue(s, t, a, b, how, per_class) >= 1e-3:
            return s, t
    raise AssertionError(f"no admissible draw for N={N} C={C} true={true} how={how} per_class={per_class}")


def fit_cases():
    """(N, C, true, how, per_class, seed) rows: every size and combination, the true parameters in turn"""
    rows, k = [], 0
    for N in FIT_N:
        for C in FIT_C:
            for how, per_class in FIT_COMBOS:
                rows.append((N, C, FIT_TRUE[k % len(FIT_TRUE)], how, per_class, 100 + k))
                k += 1
    return rows


def degenerate_table(seed=7, N=65):
    """(scores, truth, expected status) of three classes: an ordinary one (0), an all-negative one (1), a separable one (2)"""
    s, t = fit_table(N, 1, (0.5, 0.7), "platt", True, seed)
    rng = np.random.default_rng(seed)
    s1 = rng.random(N, dtype=np.float32)
    s2 = rng.random(N, dtype=np.float32) * 0.8 + 0.1
    scores = np.stack([s[:, 0], s1, s2], 1).astype(np.float32)
    truth = np.stack([t[:, 0], np.zeros(N, np.float32), (s2 > 0.5).astype(np.float32)], 1)
    return scores, truth, np.array([0, 1, 2], dtype=np.int32)


def scipy_fit(scores, truth, how, per_class):
    """(a, b) (C,) float64 by scipy's trust-exact with the analytic gradient and Hessian, from (1, 0)"""
    from scipy.optimize import minimize
    C = scores.shape[1]
    a, b = np.ones(C), np.zeros(C)
    y = np.asarray(truth) > 0
    z = rel.logit_host(scores)
    for g in ([[c] for c in range(C)] if per_class else [list(range(C))]):
        zz, yy = z[:, g].reshape(-1), y[:, g].reshape(-1)
        ok = ~np.isnan(zz)
        zz, yy, n = zz[ok], yy[ok], float(ok.sum())
        if how == "temperature":
            fun = lambda x: rel.nll_sums_host(zz, yy, x[0], 0.0)[0] / n
            jac = lambda x: rel.nll_sums_host(zz, yy, x[0], 0.0)[1:2] / n
            hess = lambda x: rel.nll_sums_host(zz, yy, x[0], 0.0)[3:4].reshape(1, 1) / n
            x = minimize(fun, [1.0], jac=jac, hess=hess, method="trust-exact", options=dict(gtol=1e-14)).x
            a[g] = x[0]
        else:
            def parts(x):
                return rel.nll_sums_host(zz, yy, x[0], x[1]) / n
            fun = lambda x: parts(x)[0]
            jac = lambda x: parts(x)[1:3]
            hess = lambda x: np.array([[parts(x)[3], parts(x)[4]], [parts(x)[4], parts(x)[5]]])
            x = minimize(fun, [1.0, 0.0], jac=jac, hess=hess, method="trust-exact", options=dict(gtol=1e-14)).x
            a[g], b[g] = x[0], x[1]
    return a, b
