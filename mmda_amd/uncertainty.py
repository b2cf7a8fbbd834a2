"""MC-dropout uncertainty: K stochastic draws per sample in ONE forward pass, reduced on the device.

The paper the confidence head comes from judges ConfidNet's ``tcp`` against two baselines: the maximum class probability, and
Monte-Carlo dropout -- the mean, entropy and mutual information of the scores over K stochastic forward passes.  Here both fall out of
two properties of the model:

  * every dropout site lies behind the encoders (four in the fusion layer, one on the classifier logits, one in the discriminator), so a
    sample's three utterance vectors are the same in every draw: the encoders, 98 % of the FLOPs, run once (phase A, the loop of
    ``InferencePass`` / ``EncoderCache.build``) and the draws start at the projections from the cached rows;
  * a mask is a pure function of (seed, site, element index) and the element index contains the batch column, so K draws of a sample
    need not be K launches of the fusion block: each sample's row is gathered K times into B K columns and ONE training-mode forward
    with one seed gives the K copies K independent masks (phase B).  No existing kernel changes.

One launch per table (``mmda_misa_mc_reduce``) then reduces the B K columns to per-sample float64 tables.  The host can restate every
mask (oracle/dropout_rng.py), so every single draw has a reference, not only the statistics.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib, ops
from .encoded import MODALITIES, EncoderCache, encoder_widths
from .inference import InferencePass, InferenceResult, _model_device, _pass_device, dataset_pass, inference_plan
from .ranking import failure_prediction

KINDS = ("mcp", "mc_mean", "entropy", "mutual_info", "variance", "tcp", "tcp_mean")
STATS = ("mean", "var", "entropy", "expected_entropy", "mutual_info", "vote")
SEED_MUL, SEED_ADD, SEED_MASK = 6364136223846793005, 1442695040888963407, 0xFFFFFFFFFFFFFFFF      # MISA._next_seed's LCG


# ---------------------------------------------------------------------------------------------- host side: seeds, chunks, refusals
def chunk_seeds(seed, chunks):
    """``seeds[0] = seed``, ``seeds[i + 1] = seeds[i] * 6364136223846793005 + 1442695040888963407 mod 2^64``: the LCG of
    ``MISA._next_seed`` with a state of its own, so a pass never draws from the model's sequence."""
    out, s = [], int(seed) & SEED_MASK
    for _ in range(int(chunks)):
        out.append(s)
        s = (s * SEED_MUL + SEED_ADD) & SEED_MASK
    return out


def chunk_plan(n, passes, columns):
    """The samples 0 .. n-1 in index order, cut into chunks of ``max(1, columns // passes)``: a list of int64 index arrays.  A chunk of
    c samples is one forward at c * passes columns."""
    per = max(1, int(columns) // int(passes))
    return [np.arange(lo, min(lo + per, int(n)), dtype=np.int64) for lo in range(0, int(n), per)]


def check_settings(passes, columns=None, task="emotion"):
    """Everything a pass refuses before any launch, each by the name of its setting."""
    if task == "sentiment":
        raise _lib.MMDAError("MC-dropout uncertainty under task='sentiment' is not built: the entropy reads a score as the probability "
                             "of a label, and the sentiment task's one output column is a regression value")
    if isinstance(passes, bool) or not isinstance(passes, (int, np.integer)) or not 1 <= int(passes) <= _lib.MC_MAX_PASSES:
        raise _lib.MMDAError(f"passes must be an int in 1 .. {_lib.MC_MAX_PASSES} (the draws one reduce launch takes), not {passes!r}")
    if columns is not None:
        if isinstance(columns, bool) or not isinstance(columns, (int, np.integer)) or int(columns) < int(passes):
            raise _lib.MMDAError(f"columns must be an int >= passes (= {int(passes)}): one sample's draws share a forward, not {columns!r}")


def _thresholds(thresholds, W, dev):
    if thresholds is None:
        return None
    t = torch.as_tensor(thresholds, dtype=torch.float32, device=dev).reshape(-1)
    if t.numel() == 1:
        t = t.expand(W)
    if t.numel() != W:
        raise ValueError(f"thresholds: one cut-off, or one per column ({W}), not {t.numel()}")
    return t.contiguous()


def _mc_out(tables, draws=None):
    out = _lib.McOut()
    for k in STATS:
        setattr(out, k, _lib.ptr(tables.get(k)))
    out.draws = _lib.ptr(draws)
    return out


# ---------------------------------------------------------------------------------------------- the reduction alone
def mc_statistics(p, passes, thresholds=None, bernoulli=True, keep_draws=False):
    """The reduction over any device table ``p`` (B K, W) fp32 whose row b K + k is draw k of sample b (``mmda_mc_reduce``, one launch,
    no read-back): a dict of (B, W) float64 device tables ``mean``, ``var`` (population form), ``vote`` (the share of draws above
    ``thresholds`` -- one cut-off or one per column; left out without them) and, ``bernoulli=True``, ``entropy`` = h(mean),
    ``expected_entropy`` = mean of h(p_k) and ``mutual_info`` = max(0, their difference), h in nats; ``keep_draws=True`` adds ``draws``
    (B, K, W) fp32.  The summation order is a function of K alone: the same bits on every run and at every B."""
    check_settings(passes)
    K = int(passes)
    if not (isinstance(p, torch.Tensor) and p.is_cuda):
        raise _lib.MMDAError("mc_statistics needs a device tensor (the HIP path has no CPU fallback)")
    if p.dim() != 2 or p.shape[0] == 0 or p.shape[0] % K != 0 or not 1 <= p.shape[1] <= _lib.MC_MAX_WIDTH:
        raise ValueError(f"p must be (B * passes, W) with B >= 1 and W in 1 .. {_lib.MC_MAX_WIDTH}, not {tuple(p.shape)} at passes = {K}")
    p = p.detach().to(torch.float32).contiguous()
    B, W = p.shape[0] // K, p.shape[1]
    thr = _thresholds(thresholds, W, p.device)
    names = [k for k in STATS if (k != "vote" or thr is not None) and (bernoulli or k not in ("entropy", "expected_entropy", "mutual_info"))]
    flat = torch.empty(len(names), B, W, dtype=torch.float64, device=p.device)
    tables = {k: flat[i] for i, k in enumerate(names)}
    draws = torch.empty(B, K, W, dtype=torch.float32, device=p.device) if keep_draws else None
    out = _mc_out(tables, draws)
    _lib.check(_lib.load().mmda_mc_reduce(p.data_ptr(), B, K, W, _lib.ptr(thr), int(bool(bernoulli)), C.byref(out), None, 0,
                                          _lib.stream_ptr()), "mmda_mc_reduce")
    if keep_draws:
        tables["draws"] = draws
    return tables


# ---------------------------------------------------------------------------------------------- the result
class MCDropoutResult:
    """Device tables, row i = sample i.  Deterministic (one evaluation forward): ``scores``, ``labels`` (n, C), ``tcp`` (n, 6), fp32.
    Over the score draws, float64 (n, C): ``mean``, ``var``, ``entropy``, ``expected_entropy``, ``mutual_info``, ``vote`` (the share of
    draws above the model's ``threshold``).  Over the ``tcp`` draws, float64 (n, 6): ``tcp_mean``, ``tcp_var``.  ``keep_draws``:
    ``draws`` (n, K, C) and ``tcp_draws`` (n, K, 6), fp32, else None.  Bookkeeping on the host: ``passes``, ``seeds`` (one per chunk),
    ``chunks`` (the sample indices of each chunk), ``lengths``, ``segments``; ``cache``: the ``EncoderCache`` the draws started from."""

    TABLES = ("scores", "labels", "tcp") + STATS + ("tcp_mean", "tcp_var", "draws", "tcp_draws")

    def __init__(self, tables, passes, seeds, chunks, lengths, segments, cache=None):
        for k in self.TABLES:
            setattr(self, k, tables.get(k))
        self.passes, self.seeds, self.chunks = int(passes), list(seeds), list(chunks)
        self.lengths, self.segments, self.cache = lengths, segments, cache
        self.n = int(self.mean.shape[0])

    def __len__(self):
        return self.n

    def _tables(self):
        return {k: getattr(self, k) for k in self.TABLES if getattr(self, k) is not None}

    def confidence(self, kind):
        """An fp32 table in which LARGER means MORE confident -- (n, C), or (n, 6) for the two ``tcp`` kinds.  "mcp": max(s, 1 - s) of
        the deterministic scores; "mc_mean": max(mean, 1 - mean); "entropy": 1 - entropy / ln 2; "mutual_info": -mutual_info;
        "variance": -var; "tcp": the deterministic ``tcp``; "tcp_mean": the mean of ``tcp`` over the draws."""
        if kind == "mcp":
            return torch.maximum(self.scores, 1.0 - self.scores).to(torch.float32)
        if kind == "mc_mean":
            return torch.maximum(self.mean, 1.0 - self.mean).to(torch.float32)
        if kind == "entropy":
            return (1.0 - self.entropy / math.log(2.0)).to(torch.float32)
        if kind == "mutual_info":
            return (-self.mutual_info).to(torch.float32)
        if kind == "variance":
            return (-self.var).to(torch.float32)
        if kind == "tcp":
            return self.tcp.to(torch.float32)
        if kind == "tcp_mean":
            return self.tcp_mean.to(torch.float32)
        raise ValueError(f"unknown kind {kind!r}: the kinds are {KINDS}")

    def failure_table(self, truth, kinds=None, tpr=0.95, bootstrap=None):
        """``{kind: failure_prediction(confidence(kind), correct)}`` with ``correct = (labels == truth)`` of the DETERMINISTIC decision
        for every kind, so the rows of the table differ in the confidence only.  ``kinds=None``: every kind whose table has the
        decisions' shape (the ``tcp`` kinds need six classes).  ``bootstrap``: None, or a ``Bootstrap`` over this result's n rows
        (mmda_amd/bootstrap.py): the table is then ``{kind: dict(result, summary, vs_tcp)}`` -- the kind's resampled failure-prediction
        figures (``BootstrapResult``, row R the unresampled table), their intervals (``BootstrapSummary`` (F, 6)) and the paired
        difference ``kind - tcp`` over the same resamples ((F, 9); None where ``tcp`` is not among the kinds)."""
        if kinds is None:
            kinds = tuple(k for k in KINDS if not k.startswith("tcp") or self.tcp.shape == self.labels.shape)
        truth = torch.as_tensor(truth).to(self.labels.device)
        correct = ((self.labels > 0) == (truth > 0)).to(torch.float32)
        if bootstrap is not None:
            res = {k: bootstrap.ranking(self.confidence(k), correct, tpr=tpr, failure=True) for k in kinds}
            return {k: dict(result=r, summary=r.summary(), vs_tcp=bootstrap.compare(r, res["tcp"]) if "tcp" in res else None)
                    for k, r in res.items()}
        return {k: failure_prediction(self.confidence(k), correct, tpr=tpr) for k in kinds}

    def cpu(self):
        """The same result on the host (one device-to-host copy per table held)."""
        return MCDropoutResult({k: v.cpu() for k, v in self._tables().items()}, self.passes, self.seeds, self.chunks, self.lengths,
                               self.segments)

    def as_dict(self):
        """Every table as a numpy array under its name, plus ``passes`` and ``seeds``.  Reads back what is still on the device."""
        out = {k: v.cpu().numpy() for k, v in self._tables().items()}
        out.update(passes=self.passes, seeds=list(self.seeds))
        return out


# ---------------------------------------------------------------------------------------------- the pass
class MCDropoutPass:
    """``MCDropoutPass(model, passes=32, seed=0, columns=256, keep_draws=False).run(dataset, batch_size, order)`` or
    ``.run_cache(cache)`` -> ``MCDropoutResult``.

    A result depends on (seed, passes, columns, n) and on nothing else -- not on ``batch_size`` or ``order``, which shape phase A
    only.  The reason: the column index is part of the mask index.  Draw k of sample i sits in column (i - lo) * passes + k of the chunk
    that starts at sample lo, chunks are cut from the samples in INDEX order by ``columns // passes`` alone, and chunk c runs under
    ``seeds[c]``; so which mask a draw sees is fixed by those four numbers, while phase A only decides in which batch a sample's
    (deterministic, batch-independent) encoder rows were computed.  For the same reason a sample's draws DO depend on the chunk it
    falls in (on ``columns``): making them independent of it would need the mask index changed inside the kernels.

    The pass leaves ``model.training``, the precision and the model's seed sequence as it found them (phase A draws one seed per batch
    as every evaluation pass does; the sequence is put back) and every later entry point sets ``set_inference`` itself, as after an
    ``InferencePass``; the next step re-carves the workspace as usual.  Nothing is read back and the host never waits inside the
    pass: the recurrences' abort words are sticky across the re-carve, ``model.check_cluster`` (or ``Solver.uncertainty``) reads them."""

    def __init__(self, model, passes=32, seed=0, columns=256, keep_draws=False):
        check_settings(passes, columns, getattr(model, "task", "emotion"))
        self.model, self.passes, self.columns = model, int(passes), int(columns)
        self.seed, self.keep_draws = int(seed) & SEED_MASK, bool(keep_draws)

    # ------------------------------------------------------------------ phase A: one evaluation forward per batch, two collects
    def run(self, dataset, batch_size, order="length"):
        """Phase A over ``dataset`` (a ``DeviceDataset``) batched by ``inference_plan`` -- per batch one gather, the evaluation
        forward, ``mmda_misa_infer_collect`` (scores, labels, tcp) and ``mmda_misa_encoded_collect`` (the utterance rows) -- then
        phase B over the rows just cached."""
        m = self.model
        plan, bounds = inference_plan(dataset.lengths, batch_size, order)
        dev = _pass_device(m, dataset, "MCDropoutPass")
        n, widths = len(dataset), encoder_widths(m)
        lengths = torch.from_numpy(np.array(dataset.lengths, dtype=np.int64))
        segments = np.array(dataset.segments, dtype=object)
        flat, layout, out = InferencePass(m, ("scores", "labels", "tcp"))._tables(n, dev)
        cache = EncoderCache(torch.empty(sum((n * w + 3) // 4 * 4 for w in widths), dtype=torch.float32, device=dev), widths, n, None,
                             lengths, segments, 0, m, getattr(m, "task", "emotion"))
        tabs = tuple(getattr(cache, f"utt_{k}").data_ptr() for k in MODALITIES)
        lib, h = m._lib, m._h

        def collect(dst_ptr):
            ops.misa_infer_collect(m, out, dst_ptr, 0)
            _lib.check(lib.mmda_misa_encoded_collect(h, *tabs, dst_ptr, 0, _lib.stream_ptr()), "mmda_misa_encoded_collect")

        seed_state = m._seed
        try:
            dataset_pass(m, dataset, plan, bounds, batch_size, dev, collect)
        finally:
            m._seed = seed_state
        det = InferenceResult(flat, layout, n, lengths, segments)
        return self._phase_b(cache, det)

    # ------------------------------------------------------------------ phase B alone
    def run_cache(self, cache, deterministic=None):
        """Phase B over an existing ``EncoderCache``.  Its ``_refuse`` applies before any launch (another device, other widths) and its
        fingerprint is enqueued in front of the first forward and read behind the last one -- this entry's one wait, the rule of an
        ``EncodedLoader`` epoch -- raising ``MMDAError`` when the encoders are not the ones the rows were made with.  ``deterministic``:
        anything with ``scores``, ``labels`` and ``tcp`` tables of the cache's samples (an ``InferenceResult``); None: one
        evaluation-mode forward from the cached rows per ``columns`` samples, collected by ``mmda_misa_infer_collect``."""
        m = self.model
        _model_device(m, "MCDropoutPass")
        if not isinstance(cache, EncoderCache):
            raise TypeError(f"run_cache takes an EncoderCache, not {type(cache).__name__}")
        pending = cache._fingerprint_issue(m)                # (_refuse first)
        n, dev = cache.n, cache.device
        if deterministic is None:
            flat, layout, out = InferencePass(m, ("scores", "labels", "tcp"))._tables(n, dev)
            rows = torch.arange(n, dtype=torch.int32, device=dev)
            for lo in range(0, n, self.columns):
                cnt = min(self.columns, n - lo)
                m._forward_encoded_raw(cache, rows.data_ptr() + 4 * lo, cnt, False, 0)
                ops.misa_infer_collect(m, out, None, lo)
            deterministic = InferenceResult(flat, layout, n, cache.lengths, cache.segments)
        res = self._phase_b(cache, deterministic)
        cache._fingerprint_verify(pending)
        return res

    def _phase_b(self, cache, det):
        m, K, n, dev = self.model, self.passes, cache.n, cache.device
        cfg = m.config
        nc = int(cfg.num_classes)
        chunks = chunk_plan(n, K, self.columns)
        seeds = chunk_seeds(self.seed, len(chunks))
        flat = torch.empty(n * (len(STATS) * nc + 2 * 6), dtype=torch.float64, device=dev)
        tables, cur = dict(scores=det.scores, labels=det.labels, tcp=det.tcp), 0
        for k, w in [(k, nc) for k in STATS] + [("tcp_mean", 6), ("tcp_var", 6)]:
            tables[k] = flat[cur:cur + n * w].view(n, w)
            cur += n * w
        if self.keep_draws:
            tables["draws"] = torch.empty(n, K, nc, dtype=torch.float32, device=dev)
            tables["tcp_draws"] = torch.empty(n, K, 6, dtype=torch.float32, device=dev)
        out_s = _mc_out(tables, tables.get("draws"))
        out_t = _mc_out(dict(mean=tables["tcp_mean"], var=tables["tcp_var"]), tables.get("tcp_draws"))
        thr = torch.full((nc,), float(cfg.threshold), dtype=torch.float32, device=dev)
        # each index `passes` times, int32, on the device: chunk c is the slice [lo K, hi K) of it
        rows = torch.arange(n, dtype=torch.int32, device=dev).repeat_interleave(K)
        lib, h = m._lib, m._h
        for idx, seed in zip(chunks, seeds):
            lo, cnt = int(idx[0]), int(idx.shape[0])
            m._forward_encoded_raw(cache, rows.data_ptr() + 4 * lo * K, cnt * K, True, seed)
            _lib.check(lib.mmda_misa_mc_reduce(h, K, 0, thr.data_ptr(), C.byref(out_s), None, lo, _lib.stream_ptr()), "mmda_misa_mc_reduce")
            _lib.check(lib.mmda_misa_mc_reduce(h, K, 1, None, C.byref(out_t), None, lo, _lib.stream_ptr()), "mmda_misa_mc_reduce")
        return MCDropoutResult(tables, K, seeds, chunks, cache.lengths, cache.segments, cache)
