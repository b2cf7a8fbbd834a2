"""Helpers of the nearest-neighbour tests (tests/test_knn_cases_cpu.py, tests/test_gpu_knn.py, tests/test_gpu_trust.py): the case table
and a brute-force reference in numpy -- int64 for the integer cases, float64 otherwise -- with the (distance, row number) order, the
padding rule, and the Trust Score and density-filter definitions of mmda_amd/neighbours.py.

Integer cases: rows are integer-valued and small enough that every squared distance, every row norm and every partial sum of either
distance form is an integer below 2^24, so fp32 computes them exactly in ANY summation order and the kernel must return the reference's
distances and row numbers bit for bit.  Ties are frequent there (at D = 6 most adjacent ranks tie), duplicated base rows are planted, and
the self-search cases plant a duplicate of a row: the duplicate stays eligible at distance 0, the row itself does not.

Real-valued cases: standard normal rows; a clustered case (32 centres plus 1e-3 noise, the queries beside the centres), where the dot
form cancels to nothing; a scaled case (rows x 30).

The shapes are the smallest that reach every edge: Q in {1, tile - 1, tile, tile + 1}, N in {1, k - 1, slab - 1, slab, slab + 1,
2 slab + 3} with tile and slab taken from ``ops.knn_plan``, D in {6, 42, 768, 770}, k in {1, 10, 16}, S in {1, 12, 16}; an empty set, a
row in no set, a set smaller than k, and one NaN row in the base."""
import functools
from dataclasses import dataclass

import numpy as np

U = 2.0 ** -24
KINDS_REAL = ("normal", "clustered", "scaled")


@dataclass(frozen=True)
class Case:
    name: str
    kind: str                # "int" or one of KINDS_REAL
    q: str                   # "1", "tile-1", "tile", "tile+1", "self" (the query table is the base)
    n: str                   # "1", "k-1", "slab-1", "slab", "slab+1", "2slab+3"
    D: int
    k: int
    S: int
    span: int = 8            # integer cases: entries drawn from -span .. span
    exclude_self: bool = False
    nan_row: bool = False    # one base row holds a NaN
    seed: int = 0


CASES = (
    Case("int_d768_merged", "int", "tile+1", "2slab+3", 768, 10, 12, seed=1),
    Case("int_d42_self", "int", "self", "slab+1", 42, 10, 12, exclude_self=True, seed=2),
    Case("int_d6_ties_narrow_tile", "int", "tile", "slab", 6, 16, 16, span=2, seed=3),
    Case("int_d6_self_ties", "int", "self", "slab-1", 6, 10, 1, span=2, exclude_self=True, seed=4),
    Case("int_one_by_one", "int", "1", "1", 6, 1, 1, span=2, seed=5),
    Case("int_d42_small_base", "int", "tile-1", "k-1", 42, 10, 12, seed=6),
    Case("int_d770_k1", "int", "tile-1", "slab-1", 770, 1, 16, seed=7),
    Case("normal_d768_nan", "normal", "tile+1", "2slab+3", 768, 10, 12, nan_row=True, seed=8),
    Case("clustered_d768", "clustered", "tile", "2slab+3", 768, 10, 12, seed=9),
    Case("scaled_d770_narrow_tile", "scaled", "tile+1", "slab+1", 770, 16, 16, seed=10),
    Case("normal_d42_k1", "normal", "1", "slab", 42, 1, 1, seed=11),
    Case("normal_d6_one_set", "normal", "tile-1", "slab-1", 6, 10, 1, nan_row=True, seed=12),
    Case("clustered_d42_small_base", "clustered", "tile", "k-1", 42, 16, 12, seed=13),
)
BY_NAME = {c.name: c for c in CASES}


def shape(case):
    """(Q, N, tile, slab) of a case: tile and slab are what ``ops.knn_plan`` gives its (D, S, k)"""
    from mmda_amd import ops
    plan = ops.knn_plan(1, 4096, case.D, case.S, case.k)
    tile, slab = plan["tile_q"], plan["slab_rows"]
    N = {"1": 1, "k-1": case.k - 1, "slab-1": slab - 1, "slab": slab, "slab+1": slab + 1, "2slab+3": 2 * slab + 3}[case.n]
    Q = N if case.q == "self" else {"1": 1, "tile-1": tile - 1, "tile": tile, "tile+1": tile + 1}[case.q]
    assert N >= 1, case
    return Q, N, tile, slab


def members(N, S, rng):
    """(N,) int32 set bits.  S > 1: S // 2 classes of random labels, bit 2 c + v (an odd S keeps its last bit for every third row);
    then set S - 1 is emptied, set S - 2 is cut to its first three rows, and every 17th row is taken out of every set.  S == 1: every
    row in set 0 but each 17th."""
    m = np.zeros(N, dtype=np.int64)
    if S == 1:
        m[:] = 1
    else:
        truth = rng.integers(0, 2, size=(N, S // 2))
        for c in range(S // 2):
            m |= 1 << (2 * c + truth[:, c])
        if S % 2:
            m[::3] |= 1 << (S - 1)
        m &= ~(1 << (S - 1))                                   # an empty set
        has = np.flatnonzero(m & (1 << (S - 2)))
        m[has[3:]] &= ~(1 << (S - 2))                          # a set smaller than k
    if N > 17:
        m[16::17] = 0                                          # rows in no set
    return m.astype(np.int32)


@functools.lru_cache(maxsize=None)
def tables(name):
    """(query, base, member) of a case: fp32 (Q, D), fp32 (N, D), int32 (N,); read-only (shared between tests)."""
    case = BY_NAME[name]
    Q, N, _, _ = shape(case)
    rng = np.random.default_rng(1000 + case.seed)
    D = case.D
    if case.kind == "int":
        base = rng.integers(-case.span, case.span + 1, size=(N, D)).astype(np.float32)
        for i in range(3, N, 7):                               # duplicated base rows: exact ties at every distance
            base[i] = base[i - 2]
        query = base if case.q == "self" else rng.integers(-case.span, case.span + 1, size=(Q, D)).astype(np.float32)
        if case.q != "self" and N > 4:
            query[::5] = base[(np.arange(0, Q, 5) * 3) % N]    # queries that ARE base rows: distance 0, and tied with their duplicates
    else:
        if case.kind == "clustered":
            centres = rng.standard_normal((32, D))
            base = centres[rng.integers(0, 32, size=N)] + 1e-3 * rng.standard_normal((N, D))
            query = centres[np.arange(Q) % 32] + 1e-3 * rng.standard_normal((Q, D))
        else:
            scale = 30.0 if case.kind == "scaled" else 1.0
            base = scale * rng.standard_normal((N, D))
            query = scale * rng.standard_normal((Q, D))
        base, query = base.astype(np.float32), query.astype(np.float32)
        if case.nan_row:
            base[N // 2, D // 2] = np.nan
    member = members(N, case.S, rng)
    for a in (query, base, member):
        a.setflags(write=False)
    return query, base, member


def pair_distances(query, base, integer=False):
    """(Q, N) squared distances as sum (q_i - b_i)^2: int64 for integer tables, float64 otherwise (NaN where a row holds one)"""
    dt = np.int64 if integer else np.float64
    q, b = query.astype(dt), base.astype(dt)
    out = np.empty((q.shape[0], b.shape[0]), dtype=dt)
    for i in range(q.shape[0]):
        diff = b - q[i]
        out[i] = (diff * diff).sum(axis=1)
    return out


def ref_knn(d, member, S, k, exclude_self=False):
    """The definition over a (Q, N) distance matrix ``d``: per (query row, set) the k least (distance, row number) among the set's rows
    whose distance is finite, query row i leaving out base row i under ``exclude_self``; the tail +inf / -1.  -> (dist (Q, S, k)
    float64, index (Q, S, k) int32, eligible (Q, S) counts)"""
    Q, N = d.shape
    df = d.astype(np.float64)
    dist = np.full((Q, S, k), np.inf)
    index = np.full((Q, S, k), -1, dtype=np.int32)
    eligible = np.zeros((Q, S), dtype=np.int64)
    rows = np.arange(N)
    for i in range(Q):
        ok = np.isfinite(df[i])
        if exclude_self:
            ok = ok & (rows != i)
        for s in range(S):
            cand = rows[ok & ((member >> s) & 1).astype(bool)]
            eligible[i, s] = cand.size
            order = cand[np.lexsort((cand, d[i, cand]))][:k]
            dist[i, s, :order.size] = df[i, order]
            index[i, s, :order.size] = order
    return dist, index, eligible


@functools.lru_cache(maxsize=None)
def reference(name):
    """(d (Q, N), dist, index, eligible) of a case, computed once"""
    case = BY_NAME[name]
    query, base, member = tables(name)
    d = pair_distances(query, base, integer=case.kind == "int")
    dist, index, eligible = ref_knn(d, member, case.S, case.k, case.exclude_self)
    for a in (d, dist, index, eligible):
        a.setflags(write=False)
    return d, dist, index, eligible


def reported_bound(D, d64):
    """The worst-case error of a direct-form fp32 sum of D squares in any order, on the float64 distance d64"""
    return 2.0 * (D + 2) * U * d64


def selection_bound(D, qn, bn_max):
    """Twice the worst-case error of the dot form |q|^2 + |b|^2 - 2 q.b in fp32: all a selection by it can move"""
    g = (D + 3) * U / (1.0 - (D + 3) * U)
    return 4.0 * g * (qn + bn_max)


def dot_form_fp32(query, base):
    """An fp32 restatement of the dot form with torch on the host: (Q, N) fp32"""
    import torch
    q, b = torch.tensor(query), torch.tensor(base)
    qn, bn = (q * q).sum(dim=1, keepdim=True), (b * b).sum(dim=1).unsqueeze(0)
    return ((qn + bn) - 2.0 * (q @ b.t())).numpy()


# ---------------------------------------------------------------------------------------------- Trust Score, density filter
def ref_members(truth):
    """(N,) int32: bit 2 c + v where truth[i, c] == v"""
    pos = (np.asarray(truth) > 0).astype(np.int64)
    m = np.zeros(pos.shape[0], dtype=np.int64)
    for c in range(pos.shape[1]):
        m |= 1 << (2 * c + pos[:, c])
    return m.astype(np.int32)


def ref_trust(dist, labels):
    """trust[i, c] = sqrt(dist[i, 2 c + 1 - y, 0]) / (sqrt(dist[i, 2 c + y, 0]) + 1e-12), y = labels[i, c] > 0, in float64 from the
    squared distances as they are given; an empty decided set (inf) gives 0, else an empty other set gives inf.
    -> (trust, d_pred, d_other) (n, C)"""
    y = (np.asarray(labels) > 0).astype(np.int64)
    n, C = y.shape
    first = np.asarray(dist)[:, :, 0]
    cols = 2 * np.arange(C)[None, :]
    p = np.take_along_axis(first, cols + y, axis=1)
    o = np.take_along_axis(first, cols + 1 - y, axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.sqrt(o.astype(np.float64)) / (np.sqrt(p.astype(np.float64)) + 1e-12)
    return np.where(np.isinf(p), 0.0, t), p, o


def ref_density_filter(radius, inside, k, alpha):
    """The stated rule: a set of m members keeps those whose radius is <= the ceil((1 - alpha) m)-th smallest radius of the set; a set
    with fewer than k members is kept whole.  radius, inside: (N, S).  -> kept (N, S) bool"""
    kept = np.zeros_like(inside, dtype=bool)
    for s in range(inside.shape[1]):
        rows = np.flatnonzero(inside[:, s])
        m = rows.size
        if m < k:
            kept[rows, s] = True
            continue
        rank = int(np.ceil((1.0 - alpha) * float(m)))
        thr = np.sort(radius[rows, s])[rank - 1]
        kept[rows[radius[rows, s] <= thr], s] = True
    return kept


def ref_vote(index, truth):
    """(n, C) fp32: the share of positive truth among the valid rows of index (n, k)"""
    pos = (np.asarray(truth) > 0).astype(np.float32)
    valid = index >= 0
    rows = pos[np.maximum(index, 0)] * valid[..., None].astype(np.float32)
    return rows.sum(axis=1, dtype=np.float32) / np.maximum(valid.sum(axis=1, keepdims=True), 1).astype(np.float32)
