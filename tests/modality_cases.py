"""Shared by tests/test_modality_cpu.py and tests/test_gpu_modality.py: references for modality masking that restate the DEFINITIONS, not
the code under test -- the Shapley value as the average marginal contribution over the six orders in which three players can join (float64),
and the mask of a collated batch from its LENGTHS (the device recognises padding by the id; the reference does not)."""
import itertools

import numpy as np

PAD, UNK = 1, 0
LENGTH_LISTS = {"B1_T1": [1], "B1_T9": [9], "B4_T9_ties": [9, 4, 9, 4], "B8_T9_ragged": [3, 9, 1, 5, 2, 7, 1, 4],
                "B5_partial_block": [2, 6, 6, 1, 3]}
WIDTHS = [(35, 74), (1, 130)]            # the lane loop of a row runs zero (1 of 64 lanes), one and three times
ATTRIB_N = (1, 63, 64, 65, 257)
ATTRIB_C = (1, 6, 16)


def shapley_ref(V):
    """``V (8, ...)`` -> ``phi (3, ...)`` float64: player m's marginal contribution V[S + m] - V[S], S = the players before m, averaged
    over the 3! orders.  (Equal to the subset form with weights 1/3, 1/6, 1/6, 1/3: a set of size 0 or 2 precedes m in two orders,
    each set of size 1 in one.)"""
    V = np.asarray(V, dtype=np.float64)
    phi = np.zeros((3,) + V.shape[1:], dtype=np.float64)
    for order in itertools.permutations(range(3)):
        S = 0
        for m in order:
            phi[m] += V[S | 1 << m] - V[S]
            S |= 1 << m
    return phi / 6.0


def loo_ref(V):
    V = np.asarray(V, dtype=np.float64)
    return np.stack([V[7] - V[7 & ~(1 << m)] for m in range(3)])


def dominant_ref(phi):
    """``phi (n, 3, C)`` (the device's own fp32 values) -> (dominant (n, C) int32, counts (3, C) int64): the lowest m among the phi_m
    that are not NaN and attain their maximum, -1 where all three are NaN."""
    phi = np.asarray(phi)
    n, _, C = phi.shape
    dom = np.full((n, C), -1, dtype=np.int32)
    for i in range(n):
        for c in range(C):
            best = None
            for m in range(3):
                x = phi[i, m, c]
                if x != x:
                    continue
                if best is None or x > best:
                    best, dom[i, c] = x, m
    counts = np.stack([(dom == m).sum(0) for m in range(3)]).astype(np.int64)
    return dom, counts


def attrib_bound(V):
    """2^-19 max(1, max |V|): at most eleven fp32 roundings (four differences, four products, three sums; the two weights' own
    rounding is below that) on magnitudes <= 2 max |V|, i.e. 11 * 2^-24 * 2 max|V| < 2^-19 max|V|."""
    finite = np.abs(np.asarray(V, dtype=np.float64))
    finite = finite[np.isfinite(finite)]
    return 2.0 ** -19 * max(1.0, float(finite.max()) if finite.size else 1.0)


def attrib_values(n, C, seed, lo=0.0, hi=1.0):
    rng = np.random.default_rng(seed)
    return rng.uniform(lo, hi, size=(8, n, C)).astype(np.float32)


def mask_ref(ids, v, a, lengths, keep):
    """Masked copies of a collated batch (numpy: ids (T, B) int64, v (T, B, dv), a (T, B, da); lengths (B,)) under ``keep``, an int
    or B keep sets: text -> UNK at t < len, visual / acoustic rows -> 0."""
    ids, v, a = np.array(ids), np.array(v), np.array(a)
    T, B = ids.shape
    keep = np.broadcast_to(np.asarray(keep, dtype=np.int64), (B,))
    for b in range(B):
        L = int(lengths[b])
        if not keep[b] & 1:
            ids[:L, b] = UNK
        if not keep[b] & 2:
            v[:, b] = 0.0
        if not keep[b] & 4:
            a[:, b] = 0.0
    return ids, v, a


def make_samples(lengths, dv, da, seed=0):
    """Reference-style samples; every sample has a class at a positive score and any six consecutive samples hold every class."""
    rng = np.random.default_rng(seed)
    out = []
    for i, L in enumerate(lengths):
        lab = rng.normal(size=(1, 7)).astype(np.float32)
        lab[0, 1 + i % 6] = 1.0
        lab[0, 1 + (i + 3) % 6] = 0.5
        out.append(((rng.integers(2, 50, size=L), rng.normal(size=(L, dv)).astype(np.float32),
                     rng.normal(size=(L, da)).astype(np.float32), ["w"] * L), lab, f"seg{i}"))
    return out
