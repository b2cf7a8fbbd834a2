"""What the MC-dropout tests share (tests/test_uncertainty_cpu.py, tests/test_gpu_mc_reduce.py, tests/test_gpu_uncertainty.py): the
numpy float64 restatement of the seven figures ``mmda_mc_reduce`` computes, the input tables the reduce kernel is tested on, and the
small model / dataset / seeds of the end-to-end pass with the oracle's draws for it -- one table, so the files cannot drift apart.

The end-to-end configuration is the one of tests/dropout_cases.py (default hidden_size, T = 4, ragged, ``p_tf`` = 0.25 at the four
fusion-layer sites, ``p_cls`` = 0.5 on the classifier logits) with n = 7 samples.  ``MC_SEED`` is a constant chosen on the CPU
(test_uncertainty_cpu.py re-checks it): with it no draw of the fp32 oracle, at K = 3 and ``columns`` = 16, lies within ``VOTE_MARGIN`` of
the decision threshold, so the GPU's vote can be compared at every element."""
import numpy as np
import torch

from oracle import dropout_rng as drng
from oracle import misa_oracle as orc

STATS = ("mean", "var", "entropy", "expected_entropy", "mutual_info", "vote")
ENTROPY = ("entropy", "expected_entropy", "mutual_info")


# ------------------------------------------------------------------------------------------------ the seven figures, in numpy float64
def bernoulli_entropy(q):
    """h(q) = -q ln q - (1 - q) ln(1 - q) in nats, h(0) = h(1) = 0; a NaN stays a NaN."""
    q = np.asarray(q, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        h = -q * np.log(q) - (1.0 - q) * np.log(1.0 - q)
    return np.where((q == 0.0) | (q == 1.0), 0.0, h)


def mc_reference(p, K, thr=None, bernoulli=True):
    """``p`` fp32 (B K, W), row b K + k = draw k of sample b -> dict of (B, W) float64 tables (and ``draws`` (B, K, W) fp32).  mean and
    the population variance over the draws widened to float64; ``vote``: the share of draws with p > thr in fp32, a NaN draw counting
    as not above (left out without ``thr``); ``bernoulli``: entropy = h(mean), expected_entropy = mean h(p_k), mutual_info =
    max(0, entropy - expected_entropy).  A NaN draw makes every figure of its element but the vote NaN."""
    p = np.ascontiguousarray(p, dtype=np.float32)
    W = p.shape[1]
    B = p.shape[0] // K
    assert B * K == p.shape[0]
    draws = p.reshape(B, K, W)
    d = draws.astype(np.float64)
    out = {"draws": draws}
    with np.errstate(invalid="ignore"):
        mean = d.sum(axis=1) / K
        out["mean"] = mean
        out["var"] = ((d - mean[:, None, :]) ** 2).sum(axis=1) / K
        if thr is not None:
            t = np.broadcast_to(np.asarray(thr, dtype=np.float32), (W,))
            out["vote"] = (draws > t[None, None, :]).sum(axis=1) / float(K)
        if bernoulli:
            out["entropy"] = bernoulli_entropy(mean)
            out["expected_entropy"] = bernoulli_entropy(d).sum(axis=1) / K
            diff = out["entropy"] - out["expected_entropy"]
            out["mutual_info"] = np.where(np.isnan(diff), np.nan, np.maximum(0.0, diff))
    return out


# ------------------------------------------------------------------------------------------------ inputs of the reduce kernel's test
REDUCE_SHAPES = [(1, 1, 6), (1, 2, 1), (5, 3, 6), (3, 64, 6), (2, 65, 6), (2, 256, 6), (7, 32, 1), (33, 8, 6), (4, 5, 64)]
DENORMAL = float(np.float32(1e-42))
ALMOST_ONE = float(np.float32(1.0) - np.float32(2.0 ** -24))
PLANTED = (0.0, 1.0, ALMOST_ONE, DENORMAL, float("nan"))


def reduce_input(B, K, W, seed=None):
    """(p (B K, W) fp32, thr (W,) fp32): uniform draws in [0, 1) with exact 0, exact 1, 1 - 2^-24, a denormal and one NaN planted at
    distinct random positions (in that order, as many as the table has room for: (1, 2, 1) holds two values), and one column's
    threshold set to an exact draw of that column."""
    rng = np.random.default_rng(1000 * B + 10 * K + W if seed is None else seed)
    p = rng.random((B * K, W), dtype=np.float32)
    at = rng.permutation(B * K * W)[:len(PLANTED)]
    flat = p.reshape(-1)
    for pos, val in zip(at, PLANTED):
        flat[pos] = np.float32(val)
    thr = (0.2 + 0.6 * rng.random(W)).astype(np.float32)
    # one column's threshold is an exact draw of that column: `>` must be strict
    w0 = int(rng.integers(0, W))
    col = p[:, w0]
    finite = col[np.isfinite(col)]
    if finite.size:
        thr[w0] = finite[0]
    return p, thr


# ------------------------------------------------------------------------------------------------ the end-to-end case
N, T, K_SMALL, COLUMNS_SMALL = 7, 4, 3, 16
P_TF, P_CLS = 0.25, 0.5
WSEED, DSEED = 31, 5
MC_SEED = 0x6D0C0075                 # of 0x6D0C0000 + 0 .. 399 the seed whose nearest fp32-oracle draw lies farthest (0.032) from the threshold
VOTE_MARGIN = 2e-2                   # every fp32-oracle draw keeps this far from the threshold: 20 times the 10 x tol_out the GPU test skips at
TOL_OUT = 1e-4                       # dropout_cases' fp32 bound on scores / tcp, relative to the tensor's max (model_compare.rel)
MOSEI = (35, 74)


def config():
    return orc.default_config(vocab_size=80, dropout=P_CLS, use_confidNet=True)


def make_samples(n=N, seed=DSEED):
    """Reference-style samples of lengths 1 .. T (ragged), as tests/test_gpu_inference.py makes them."""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(1, T + 1, size=n)
    lengths[0], lengths[-1] = T, 1
    out = []
    for i, L in enumerate(lengths):
        L = int(L)
        lab = rng.normal(size=(1, 7)).astype(np.float32)
        lab[0, 1 + i % 6] = 1.0
        lab[0, 1 + (i + 3) % 6] = 0.5
        out.append(((rng.integers(2, 50, size=L), rng.normal(size=(L, MOSEI[0])).astype(np.float32),
                     rng.normal(size=(L, MOSEI[1])).astype(np.float32), ["w"] * L), lab, f"seg{i}"))
    return out


def params():
    return orc.synth_params(config(), WSEED)


def oracle_utterances(samples):
    """The fp32 oracle's three utterance tables (n, 4 H_i), row i = sample i: the encoders over the samples as ONE padded batch
    (evaluation outputs do not depend on the batch a sample sits in), rows put back at their sample index."""
    from mmda_amd.data import collate_fn
    cfg, P = config(), params()
    t, v, a, _, _, l, _, _, _, ids = collate_fn(list(samples))
    with torch.no_grad():
        o = orc.forward(P, cfg, t, v, a, l)
    at = torch.tensor([int(s[3:]) for s in ids])
    out = {}
    for m in "tva":
        val = getattr(o, f"utterance_{m}")
        tab = torch.empty_like(val)
        tab[at] = val
        out[m] = tab
    return out


def tiled_masks(cfg, B, K, seed):
    """What a pass that IGNORED the column index would apply: the masks of (seed, B) with every column repeated K times."""
    m = drng.site_masks(cfg, B, seed, P_TF, P_CLS)
    return {k: v.repeat_interleave(K, dim=0 if k in ("attn", "cls") else 1) for k, v in m.items()}


def oracle_chunk(utt, idx, K, seed, masks=None):
    """The oracle's draws of one chunk: ``utt`` {"t","v","a"} -> (n, 4 H) tables, ``idx`` the chunk's sample indices; each row repeated
    K times, one training-mode fusion block under ``site_masks(cfg, len(idx) K, seed)``.  -> (scores (c, K, C), tcp (c, K, 6))."""
    cfg, P = config(), params()
    rows = torch.as_tensor(np.asarray(idx), dtype=torch.int64).repeat_interleave(K)
    rep = {m: utt[m][rows] for m in "tva"}
    if masks is None:
        masks = drng.site_masks(cfg, len(idx) * K, seed, P_TF, P_CLS)
    with torch.no_grad():
        o = orc.fusion_from_utterances(P, cfg, rep, masks=masks)
    c = len(idx)
    return o.scores.reshape(c, K, -1), o.tcp.reshape(c, K, 6)


def oracle_draws(utt, chunks, seeds, K):
    """(scores (n, K, C), tcp (n, K, 6)) fp32 of the whole pass: ``oracle_chunk`` per (chunk, seed), rows in sample order."""
    S, Q = zip(*(oracle_chunk(utt, idx, K, seed) for idx, seed in zip(chunks, seeds)))
    return torch.cat(S, 0), torch.cat(Q, 0)


def threshold_margin(scores, thr):
    """The distance of the nearest draw from the threshold."""
    return float((scores.double() - float(np.float32(thr))).abs().min())


def entropy_slope(scores, pad=TOL_OUT):
    """max |h'(q)| = max |ln((1 - q) / q)| over the draws (n, K, C) and their per-sample means, each moved by ``pad`` away from 1/2
    first (so the figure holds on the whole interval an error of ``pad`` can reach): the Lipschitz constant that turns an error of
    the scores into one of the entropy figures."""
    q = torch.cat([scores.double().reshape(-1), scores.double().mean(dim=1).reshape(-1)])
    q = torch.where(q < 0.5, q - pad, q + pad).clamp(1e-300, 1.0 - 1e-16)
    return float(torch.log((1.0 - q) / q).abs().max())


def stat_bounds(scores):
    """{figure: absolute bound} on the GPU's statistics of the score draws against the oracle's, given draws within ``TOL_OUT``
    (absolute; scores are at most 1, so the relative bound on the draws implies it).  mean: an average of K errors, TOL_OUT.  var =
    mean(p^2) - mean^2: its derivative in p_k is 2 (p_k - mean) / K, and sum_k |.| <= 2 * mean|p_k - mean| <= 1, so TOL_OUT.  entropy
    = h(mean) and expected_entropy = mean h(p_k): L * TOL_OUT with L = ``entropy_slope`` of the ORACLE's draws (the issue's 2 x tol_out
    assumes L <= 2; it is 2.0 .. 2.8 at these cases -- a kept logit is doubled by the classifier's p = 0.5 dropout -- so the derived
    figure is used where it is the larger one).  mutual_info, their clipped difference: both errors, 2 L * TOL_OUT (the issue's
    2 x tol_out is L <= 1)."""
    L = entropy_slope(scores)
    return dict(mean=TOL_OUT, var=TOL_OUT, entropy=max(2.0, L) * TOL_OUT, expected_entropy=max(2.0, L) * TOL_OUT,
                mutual_info=max(2.0, 2.0 * L) * TOL_OUT)
