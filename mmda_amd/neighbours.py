"""Exact nearest neighbours between device tables, and the Trust Score built on them.

The paper the confidence head comes from judges ConfidNet's ``tcp`` against three baselines.  Maximum class probability and MC dropout
read the network's own output (mmda_amd/uncertainty.py); the third, Trust Score (Jiang et al. 2018), reads the TRAINING SET: for each
decision, the distance from the sample's hidden vector to the nearest training example of the other label, divided by the distance to
the nearest training example of the decided label.  Underneath is one operation, ``mmda_knn_sets`` (csrc/knn.hip): per (query row,
set of base rows) the k nearest members, exact, from a distance GEMM on the f32-input MFMA whose Q x N matrix never reaches memory.

  knn_search      the operation over two device tables
  NeighbourIndex  a table of hidden vectors: the nearest training examples of a sample, and their k-NN vote
  TrustIndex      the 2 C sets {truth[:, c] == v} of a table, optionally thinned to their alpha-high-density subsets; ``score``
  TrustResult     the tables of a scored split; ``failure_table`` puts ``trust`` beside ``mcp`` / ``tcp`` in the failure-prediction report

Nothing here reads back or waits: shapes are host integers, everything else stays on the device.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, ops
from .ranking import failure_prediction

MAX_K, MAX_SETS, MAX_D, MAX_CLASSES = _lib.KNN_MAX_K, _lib.KNN_MAX_SETS, _lib.KNN_MAX_D, _lib.TRUST_MAX_CLASSES
MIN_DIST = 1e-12          # the published implementation's min_dist (csrc/knn.hip carries the same constant)


# ---------------------------------------------------------------------------------------------- refusals, by name
def _int_in(name, v, lo, hi, why):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError(f"{name} must be an int in {lo} .. {hi} ({why}), not {v!r}")
    return int(v)


def _table(name, t, who, cols=None):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise _lib.MMDAError(f"{who} needs device tensors (the HIP path has no CPU fallback): {name} is not one")
    if t.dim() != 2:
        raise ValueError(f"{name} must be 2-D (rows, D), not {tuple(t.shape)}")
    if cols is not None and int(t.shape[1]) != cols:
        raise ValueError(f"{name} has {int(t.shape[1])} columns, the table it is searched against {cols}")
    if not 1 <= int(t.shape[1]) <= MAX_D:
        raise ValueError(f"{name} must have D in 1 .. {MAX_D} columns, not {int(t.shape[1])}")
    return t.detach().to(torch.float32).contiguous()


def check_trust_settings(k=10, alpha=0.0, classes=1, task="emotion"):
    """Everything ``TrustIndex.fit`` and ``Solver.trust`` refuse before any launch, each by the name of its setting."""
    from . import step_rules
    step_rules.trust_check(task=task, k=k)
    _int_in("k", k, 1, MAX_K, "the entries one list of mmda_knn_sets holds")
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float, np.floating, np.integer)) or not 0.0 <= float(alpha) < 1.0:
        raise ValueError(f"alpha must be a number in [0, 1) (the share of each set the density filter drops), not {alpha!r}")
    if not 1 <= int(classes) <= MAX_CLASSES:
        raise ValueError(f"truth must have 1 .. {MAX_CLASSES} classes (two sets per class, {MAX_SETS} sets per search), not {int(classes)}")


# ---------------------------------------------------------------------------------------------- the operation
def knn_search(query, base, k, member=None, sets=1, exclude_self=False):
    """Per (query row, set) the ``k`` nearest member rows of ``base``: ``(dist, index)``, device tensors (Q, sets, k) fp32 / int32.

    ``query`` (Q, D) and ``base`` (N, D) are device tables of one width D in 1 .. 1024; ``member`` (N,) integers whose bit s says
    that base row is in set s (None: every row in set 0), ``sets`` in 1 .. 16, ``k`` in 1 .. 16.  ``dist`` holds SQUARED Euclidean
    distances, ascending, equal distances by lower row number, recomputed as sum (q_i - b_i)^2 for the rows the search selected (a
    query equal to a base row reports exactly 0); where a set has fewer than k eligible rows the tail is +inf / -1; a pair whose
    distance is not finite is never selected.  ``exclude_self``: query row i ignores base row i, by row number (the self-search of a
    table).  A call over Q rows gives the bits of Q calls over one row each."""
    q = _table("query", query, "knn_search")
    b = _table("base", base, "knn_search", cols=int(q.shape[1]))
    k = _int_in("k", k, 1, MAX_K, "the entries one list holds")
    sets = _int_in("sets", sets, 1, MAX_SETS, "the bits of member that are read")
    if int(b.shape[0]) < 1:
        raise ValueError("base must have at least one row")
    if b.device != q.device:
        raise ValueError(f"query is on {q.device}, base on {b.device}")
    if member is None:
        m = torch.ones(int(b.shape[0]), dtype=torch.int32, device=b.device)
    else:
        if not (isinstance(member, torch.Tensor) and member.is_cuda):
            raise _lib.MMDAError("knn_search needs device tensors (the HIP path has no CPU fallback): member is not one")
        if member.dim() != 1 or int(member.shape[0]) != int(b.shape[0]) or member.dtype.is_floating_point:
            raise ValueError(f"member must be ({int(b.shape[0])},) integers, one per base row, not {tuple(member.shape)} {member.dtype}")
        m = member.detach().to(torch.int32).contiguous()
    return ops.knn_sets(q, b, m, sets, k, exclude_self)


class NeighbourIndex:
    """``NeighbourIndex(vectors, truth=None, segments=None)`` over a device table of hidden vectors (N, D).  ``search(query, k)``:
    the ``k`` nearest rows of each query, ``(dist, index)`` (n, k) -- an explanation by example: ``segments[index]`` names them.
    ``vote(query, k)``: (n, C) fp32, the share of positive ``truth`` among the k nearest (among as many as there are where N < k): the
    k-NN classifier on the fused representation."""

    def __init__(self, vectors, truth=None, segments=None):
        self.vectors = _table("vectors", vectors, "NeighbourIndex")
        self.n = int(self.vectors.shape[0])
        self.truth = None
        if truth is not None:
            truth = torch.as_tensor(truth).to(self.vectors.device)
            if truth.dim() != 2 or int(truth.shape[0]) != self.n:
                raise ValueError(f"truth must be ({self.n}, C), one row per vector, not {tuple(truth.shape)}")
            self.truth = (truth > 0).to(torch.float32)
        self.segments = segments

    def search(self, query, k, exclude_self=False):
        dist, index = knn_search(query, self.vectors, k, exclude_self=exclude_self)
        return dist[:, 0], index[:, 0]

    def vote(self, query, k, exclude_self=False):
        if self.truth is None:
            raise ValueError("vote needs the truth table the index was built without")
        _, index = self.search(query, k, exclude_self)
        valid = (index >= 0)
        rows = self.truth[index.clamp_min(0).to(torch.int64)] * valid.unsqueeze(-1).to(torch.float32)      # (n, k, C)
        return rows.sum(dim=1) / valid.sum(dim=1, keepdim=True).clamp_min(1).to(torch.float32)


# ---------------------------------------------------------------------------------------------- Trust Score
def set_members(truth):
    """(N,) int32: bit 2 c + v of row i is set where ``truth[i, c] == v`` (v = 1: > 0)"""
    pos = (truth > 0).to(torch.int32)
    C = int(truth.shape[1])
    shifts = torch.arange(C, dtype=torch.int32, device=truth.device) * 2
    return torch.bitwise_left_shift(torch.ones_like(pos), shifts.unsqueeze(0) + pos).sum(dim=1).to(torch.int32)


class TrustResult:
    """Device tables of a scored split, row i = sample i, column c = class c: ``trust`` (n, C) float64 =
    sqrt(d_other) / (sqrt(d_pred) + 1e-12); ``d_pred`` / ``d_other`` (n, C) fp32, the SQUARED distance to the nearest kept training row
    whose label in class c is / is not the decided one (+inf where there is none: ``trust`` is then 0 / +inf); ``nearest_pred`` /
    ``nearest_other`` (n, C) int32 their row numbers in the fitted table (-1 where there is none); ``labels`` (n, C) the decisions."""

    TABLES = ("trust", "d_pred", "d_other", "nearest_pred", "nearest_other", "labels")

    def __init__(self, tables, k=1, alpha=0.0):
        for name in self.TABLES:
            setattr(self, name, tables.get(name))
        self.k, self.alpha = int(k), float(alpha)
        self.n = int(self.trust.shape[0])

    def __len__(self):
        return self.n

    def _tables(self):
        return {name: getattr(self, name) for name in self.TABLES if getattr(self, name) is not None}

    def confidence(self):
        """``trust`` as an fp32 table: larger means more confident."""
        return self.trust.to(torch.float32)

    def failure_table(self, truth, others=None, tpr=0.95, bootstrap=None):
        """``{"trust": failure_prediction(confidence(), correct), name: failure_prediction(table, correct) ...}`` for the tables of
        ``others`` (a dict such as ``{"mcp": ..., "tcp": ...}``, larger = more confident, of the decisions' shape), every row against
        the same ``correct = (labels == truth)``.  ``bootstrap``: None, or a ``Bootstrap`` over this result's n rows: the table is
        then ``{kind: dict(result, summary, vs_tcp)}`` as ``MCDropoutResult.failure_table`` gives it -- the resampled figures, their
        intervals and the paired difference ``kind - tcp`` over the same resamples (None where ``tcp`` is not among the rows)."""
        truth = torch.as_tensor(truth).to(self.labels.device)
        if truth.shape != self.labels.shape:
            raise ValueError(f"truth must be {tuple(self.labels.shape)}, the decisions' shape, not {tuple(truth.shape)}")
        correct = ((self.labels > 0) == (truth > 0)).to(torch.float32)
        rows = {"trust": self.confidence()}
        for name, t in (others or {}).items():
            if name == "trust" or tuple(t.shape) != tuple(self.labels.shape):
                raise ValueError(f"others[{name!r}] must be a {tuple(self.labels.shape)} table under another name than 'trust'")
            rows[name] = t.detach().to(torch.float32)
        if bootstrap is not None:
            res = {name: bootstrap.ranking(t, correct, tpr=tpr, failure=True) for name, t in rows.items()}
            return {name: dict(result=r, summary=r.summary(), vs_tcp=bootstrap.compare(r, res["tcp"]) if "tcp" in res else None)
                    for name, r in res.items()}
        return {name: failure_prediction(t, correct, tpr=tpr) for name, t in rows.items()}

    def cpu(self):
        """The same result on the host (one device-to-host copy per table)."""
        return TrustResult({name: t.cpu() for name, t in self._tables().items()}, self.k, self.alpha)

    def as_dict(self):
        """Every table as a numpy array under its name, plus ``k`` and ``alpha``.  Reads back what is still on the device."""
        out = {name: t.cpu().numpy() for name, t in self._tables().items()}
        out.update(k=self.k, alpha=self.alpha)
        return out


class TrustIndex:
    """``TrustIndex.fit(vectors, truth, k=10, alpha=0.0)`` then ``.score(vectors, labels)`` -> ``TrustResult``.

    The 2 C sets of the fitted table are the rows with ``truth[:, c] == v``, numbered s = 2 c + v.  ``alpha > 0`` thins each set to its
    alpha-high-density subset: a member's radius is its distance to its k-th nearest member of the same set, the row itself counting
    as the first (as in the published implementation) -- one self-search with ``mmda_knn_sets`` --, and a set of m members keeps those
    whose radius is <= the ceil((1 - alpha) m)-th smallest radius of the set, the nearest-rank quantile.  The published code
    interpolates the percentile linearly (``np.percentile``); the nearest-rank rule is deterministic, needs no interpolation between
    two radii, and is the same at alpha = 0, where both keep every member.  A set with fewer than k members is kept whole.  The
    threshold comes from one ``torch.sort`` on the device (fit time, at most 16 columns).  Nothing is read back.

    ``members`` (N,) int32: the set bits of the kept rows; ``kept`` (N, 2 C) bool; ``radius`` (N, 2 C) fp32, the squared radii (+inf
    outside a row's sets; None at alpha = 0)."""

    def __init__(self, vectors, members, kept, classes, k, alpha, radius=None):
        self.vectors, self.members, self.kept, self.radius = vectors, members, kept, radius
        self.classes, self.k, self.alpha = int(classes), int(k), float(alpha)

    @classmethod
    def fit(cls, vectors, truth, k=10, alpha=0.0):
        v = _table("vectors", vectors, "TrustIndex.fit")
        if not (isinstance(truth, torch.Tensor) and truth.is_cuda):
            raise _lib.MMDAError("TrustIndex.fit needs device tensors (the HIP path has no CPU fallback): truth is not one")
        if truth.dim() != 2 or int(truth.shape[0]) != int(v.shape[0]):
            raise ValueError(f"truth must be ({int(v.shape[0])}, C), one row per vector, not {tuple(truth.shape)}")
        C = int(truth.shape[1])
        check_trust_settings(k, alpha, C)
        if int(v.shape[0]) < 1:
            raise ValueError("vectors must have at least one row")
        k, alpha, S = int(k), float(alpha), 2 * C
        members = set_members(truth)
        bits = torch.arange(S, dtype=torch.int32, device=v.device).unsqueeze(0)
        inside = (torch.bitwise_right_shift(members.unsqueeze(1), bits) & 1).to(torch.bool)              # (N, S)
        radius = None
        if alpha > 0.0:
            dist, _ = ops.knn_sets(v, v, members, S, k, False)
            inf = torch.full((), float("inf"), dtype=torch.float32, device=v.device)
            radius = torch.where(inside, dist[:, :, k - 1], inf)                                          # (N, S)
            m = inside.sum(dim=0)                                                                         # (S,) members per set
            rank = torch.ceil((1.0 - alpha) * m.to(torch.float64)).to(torch.int64)                        # nearest rank, 1-based
            ordered, _ = torch.sort(radius, dim=0)
            thr = ordered.gather(0, (rank - 1).clamp_(0, int(v.shape[0]) - 1).unsqueeze(0))               # (1, S)
            inside = inside & ((radius <= thr) | (m < k).unsqueeze(0))
            members = (inside.to(torch.int32) << bits).sum(dim=1).to(torch.int32)
        return cls(v, members.contiguous(), inside, C, k, alpha, radius)

    def score(self, vectors, labels):
        """``vectors`` (n, D) hidden vectors and ``labels`` (n, C) the decisions made for them -> ``TrustResult``: one search at k = 1
        over the 2 C kept sets and one ``mmda_trust_score`` launch."""
        q = _table("vectors", vectors, "TrustIndex.score", cols=int(self.vectors.shape[1]))
        if not (isinstance(labels, torch.Tensor) and labels.is_cuda):
            raise _lib.MMDAError("TrustIndex.score needs device tensors (the HIP path has no CPU fallback): labels is not one")
        if tuple(labels.shape) != (int(q.shape[0]), self.classes):
            raise ValueError(f"labels must be ({int(q.shape[0])}, {self.classes}), not {tuple(labels.shape)}")
        lab = (labels.detach() > 0).to(torch.float32).contiguous()
        dist, index = ops.knn_sets(q, self.vectors, self.members, 2 * self.classes, 1, False)
        trust, d_pred, d_other, n_pred, n_other = ops.trust_score(dist, lab, index, tables=True)
        return TrustResult(dict(trust=trust, d_pred=d_pred, d_other=d_other, nearest_pred=n_pred, nearest_other=n_other, labels=lab),
                           self.k, self.alpha)
