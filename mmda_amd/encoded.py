"""Encoder cache: train the fusion block and the heads from stored encoder outputs.

When nothing behind the fusion block trains -- the six recurrent layers, the three ``{t,v,a}layer_norm`` between them and the embedding
table are frozen, the *encoder cut* of ``MISA.freeze`` -- the three utterance vectors ``utt_t (4 H_t)``, ``utt_v (4 H_v)``,
``utt_a (4 H_a)`` of a sample are constants: the encoders have no dropout (``nn.LSTM`` / ``nn.GRU``, one layer each, reference
``models.py:48-55``), and nothing behind them reads anything else of them.  ``EncoderCache.build`` runs the evaluation forward once over
a ``DeviceDataset`` and keeps those rows on the device, row i = sample i; ``EncodedLoader`` then makes a batch an index list, and
``MISA.train_step_encoded`` / ``MISA.forward_encoded`` gather the batch's rows straight into the workspace (one launch) and start at
the projections: no embedding conversion, no input GEMM, no recurrence.  From the projections on such a step issues the launches of a
step under the cut, so parameters, moments and losses get the same bits.  DESIGN.md 4g.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .data import _kept, batch_plan
from .inference import _pass_device, dataset_pass, inference_plan

MODALITIES = ("t", "v", "a")
ENCODER_PREFIXES = ("trnn1", "trnn2", "vrnn1", "vrnn2", "arnn1", "arnn2", "tlayer_norm", "vlayer_norm", "alayer_norm", "embed")


def encoder_widths(model):
    """(4 H_t, 4 H_v, 4 H_a): the widths of the rows the fusion block reads of the encoders (final h of two layers x two directions)."""
    return tuple(4 * int(h) for h in model.hidden_sizes)


def encoder_ranges(model):
    """The ranges (begin, end) of the flat parameter bucket that the encoders read: the recurrent layers -- from the first of them up to
    the table, which follows them --, the three inter-layer LayerNorm pairs, and the table."""
    lay = model._layout
    size = lambda n: int(np.prod(lay[n][1]))
    rnn = [n for n in model._native_names if n.split(".")[0] in ENCODER_PREFIXES[:6]]
    embed = lay["embed.weight"][0]
    out = [(min(lay[n][0] for n in rnn), embed)]
    assert all(out[0][0] <= lay[n][0] and lay[n][0] + size(n) <= embed for n in rnn)
    for m in MODALITIES:
        for k in ("weight", "bias"):
            n = f"{m}layer_norm.{k}"
            out.append((lay[n][0], lay[n][0] + size(n)))
    out.append((embed, embed + size("embed.weight")))
    return out


def _fingerprint_tensor(model):
    """int64 sum over the int32 view of ``encoder_ranges`` -- a tensor of one element on the model's device, nothing read back.  A model
    whose parameters are not in their flat bucket yet (before its first step) is summed tensor by tensor: the same number, since the
    alignment padding between tensors is zero."""
    if model._views_valid():
        bits = model._P.view(torch.int32)
        parts = [bits[b:e] for b, e in encoder_ranges(model)]
    else:
        parts = [model._get(n).detach().reshape(-1).view(torch.int32) for n in model._native_names if n.split(".")[0] in ENCODER_PREFIXES]
    return torch.stack([x.sum(dtype=torch.int64) for x in parts]).sum()


class EncoderCache:
    """``utt_t``, ``utt_v``, ``utt_a``: (n, 4 H_i) views of one flat 16-byte aligned buffer; ``emo`` (n, 6) or None; ``lengths`` (n,)
    int64 and ``segments`` on the host; ``fingerprint``, the int64 sum over the int32 view of every parameter the encoders read, taken
    when the rows were made.  Row i is sample i of the ``DeviceDataset`` the cache was built from."""

    def __init__(self, flat, widths, n, emo, lengths, segments, fingerprint, model=None, task="emotion"):
        self.task = task                         # what ``emo`` holds: the emotion labels, or (task="sentiment") the (n, 1) sentiment column
        self.flat, self.widths, self.n = flat, tuple(int(w) for w in widths), int(n)
        self.emo, self.lengths, self.segments, self.fingerprint = emo, lengths, segments, int(fingerprint)
        self.model = model                       # the model the fingerprint was last taken of (EncodedLoader checks against it)
        self.device = flat.device
        cur = 0
        for m, w in zip(MODALITIES, self.widths):
            setattr(self, f"utt_{m}", flat[cur:cur + self.n * w].view(self.n, w))
            cur += self._stride(w)

    def _stride(self, w):
        return (self.n * w + 3) // 4 * 4         # every table starts 16-byte aligned

    def __len__(self):
        return self.n

    @classmethod
    def build(cls, model, dataset, batch_size, order="length"):
        """One evaluation pass of ``model`` over ``dataset`` (a ``DeviceDataset``), batched by ``inference_plan`` -- the loop of
        ``InferencePass.run``: one gather, one seed drawn, the evaluation forward and ONE collect launch
        (``mmda_misa_encoded_collect``) per batch.  The pass does not need the cut (an evaluation forward trains nothing); training from
        the cache does."""
        plan, bounds = inference_plan(dataset.lengths, batch_size, order)
        dev = _pass_device(model, dataset, "EncoderCache")
        n, widths = len(dataset), encoder_widths(model)
        flat = torch.empty(sum((n * w + 3) // 4 * 4 for w in widths), dtype=torch.float32, device=dev)
        task = getattr(model, "task", "emotion")
        # the label table the steps gather from: under the sentiment task the dataset's sentiment column, one float per sample
        labels = dataset.sentiment.reshape(n, 1).clone() if task == "sentiment" else None if dataset.emo is None else dataset.emo.clone()
        cache = cls(flat, widths, n, labels, torch.from_numpy(np.array(dataset.lengths, dtype=np.int64)),
                    np.array(dataset.segments, dtype=object), 0, model, task)
        tabs = tuple(getattr(cache, f"utt_{m}").data_ptr() for m in MODALITIES)
        lib, h = model._lib, model._h
        dataset_pass(model, dataset, plan, bounds, batch_size, dev, lambda dst_ptr: _lib.check(
            lib.mmda_misa_encoded_collect(h, *tabs, dst_ptr, 0, _lib.stream_ptr()), "mmda_misa_encoded_collect"))
        model.check_cluster("encoder cache")
        cache.fingerprint = int(_fingerprint_tensor(model).item())         # (off the hot path: the build's one read-back)
        return cache

    # ------------------------------------------------------------------ staleness
    def _refuse(self, model):
        dev = next(model.parameters()).device
        if dev != self.device:
            raise _lib.MMDAError(f"encoder cache: the cache is on {self.device}, the model on {dev}")
        if encoder_widths(model) != self.widths:
            raise _lib.MMDAError(f"encoder cache: its rows are {self.widths} floats wide, the model's encoders give {encoder_widths(model)}")

    def _fingerprint_issue(self, model):
        """The fingerprint of ``model`` as a device tensor: enqueued, not read."""
        self._refuse(model)
        return _fingerprint_tensor(model)

    def _fingerprint_verify(self, pending):
        got = int(pending.item())
        if got != self.fingerprint:
            raise _lib.MMDAError(f"encoder cache is stale: the parameters the encoders read (recurrent layers, inter-layer LayerNorms, "
                                 f"embedding table) have fingerprint {got}, the cache was built at {self.fingerprint}: rebuild it "
                                 f"(EncoderCache.build)")

    def check(self, model):
        """Recompute the fingerprint of ``model`` (torch ops, one read-back) and raise ``MMDAError`` naming the cache as stale when it
        differs from the one the rows were made at.  Remembers ``model`` as the one an ``EncodedLoader`` checks against."""
        self._fingerprint_verify(self._fingerprint_issue(model))
        self.model = model
        return self

    # ------------------------------------------------------------------ files
    def save(self, path):
        """Plain tensors and Python scalars (``torch.load(..., weights_only=True)`` reads them); segments are saved as ``str``."""
        torch.save(dict(flat=self.flat.cpu(), widths=list(self.widths), n=self.n, emo=None if self.emo is None else self.emo.cpu(),
                        lengths=self.lengths.cpu(), segments=[str(s) for s in self.segments], fingerprint=self.fingerprint), path)

    @classmethod
    def load(cls, path, device):
        """The cache of ``save`` on ``device``.  It knows no model yet: ``cache.check(model)`` before training from it.  (The file's keys
        are what they were: a label table one column wide is the sentiment column, the dataset's emotion table has six.)"""
        d = torch.load(path, weights_only=True, map_location="cpu")
        seg = np.empty(len(d["segments"]), dtype=object)
        for i, s in enumerate(d["segments"]):
            seg[i] = s
        return cls(d["flat"].to(device), d["widths"], d["n"], None if d["emo"] is None else d["emo"].to(device), d["lengths"], seg,
                   d["fingerprint"], task="sentiment" if d["emo"] is not None and d["emo"].shape[1] == 1 else "emotion")


class EncodedBatch:
    """A batch of cached rows: an index list.  ``rows`` (B,) int32 on the cache's device names the samples (``rows_ptr`` its address);
    ``lengths`` (B,) int64 and ``segments`` come in the same order.  The gather happens inside the step."""

    def __init__(self, cache, rows, B, lengths, segments):
        self.cache, self.rows, self.rows_ptr, self.B, self.lengths, self.segments = cache, rows, rows.data_ptr(), int(B), lengths, segments

    def emo(self):
        """The batch's labels (B, 6) -- under the sentiment task the (B, 1) sentiment column --: a torch gather, for callers outside the fused step (which gathers them itself)."""
        if self.cache.emo is None:
            raise _lib.MMDAError("encoder cache: the dataset it was built from has no emotion labels")
        return self.cache.emo.index_select(0, self.rows)


class EncodedLoader:
    """``DeviceLoader``'s rules over an ``EncoderCache``: an epoch draws its index sequence (``sampler``, else ``torch.randperm(n,
    generator=generator)`` when ``shuffle``, else 0 .. n-1), plans its batches with ``batch_plan`` over the cache's OWN lengths -- so the
    batches, and the order of the samples inside each, are those of a ``DeviceLoader`` over the dataset the cache was built from --
    and uploads the int32 order once; a batch is a slice of it.

    Staleness: an epoch enqueues the fingerprint of ``cache.model`` before its first batch and reads it back behind its last one -- the
    epoch's one synchronisation, next to the loss read-back every epoch ends with -- raising ``MMDAError`` when the encoders' parameters
    are not the ones the cache was built at.  (Inside an epoch the cut guarantees that no launch writes them; a consumer that leaves
    the loop early is not checked.)"""

    def __init__(self, cache, batch_size, shuffle=False, sampler=None, generator=None, drop_last=False):
        if sampler is not None and shuffle:
            raise ValueError("sampler option is mutually exclusive with shuffle")
        self.cache, self.batch_size, self.shuffle, self.sampler, self.generator = cache, int(batch_size), bool(shuffle), sampler, generator
        self.drop_last = bool(drop_last)
        _kept(0, self.batch_size, self.drop_last)

    def __len__(self):
        m = len(self.sampler) if self.sampler is not None else len(self.cache)
        return _kept(m, self.batch_size, self.drop_last)[2]

    def _indices(self):
        if self.sampler is not None:
            return np.fromiter(iter(self.sampler), dtype=np.int64)
        if self.shuffle:
            return torch.randperm(len(self.cache), generator=self.generator).numpy()
        return np.arange(len(self.cache), dtype=np.int64)

    def plan(self):
        """(order, bounds) of the next epoch, as ``batch_plan`` returns them (draws the epoch's index sequence)."""
        return batch_plan(self.cache.lengths.numpy(), self._indices(), self.batch_size, self.drop_last)

    def __iter__(self):
        c = self.cache
        order, bounds = self.plan()
        if order.size == 0:
            return
        if c.model is None:
            raise _lib.MMDAError("encoder cache: it was loaded from a file and has not been checked against a model: cache.check(model)")
        pending = c._fingerprint_issue(c.model)
        order_dev = torch.from_numpy(order.astype(np.int32))
        if c.device.type == "cuda":
            order_dev = order_dev.pin_memory().to(c.device, non_blocking=True)
        lens_all = c.lengths[torch.from_numpy(order)]
        segs_all = c.segments[order]
        for lo, hi in zip(bounds[:-1].tolist(), bounds[1:].tolist()):
            yield EncodedBatch(c, order_dev[lo:hi], hi - lo, lens_all[lo:hi].clone(), segs_all[lo:hi].tolist())
        c._fingerprint_verify(pending)
