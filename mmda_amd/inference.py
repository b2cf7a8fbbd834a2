"""Inference pass: a trained (and usually frozen) MISA run once over a split, with the per-sample class scores, thresholded labels,
ConfidNet confidence (``tcp``), fused hidden vector ``h``, the six utterance vectors and the fusion layer's attention map kept ON THE
DEVICE in tables of one row per sample -- the inputs of the reference's second stage (``src/inference.py`` is a TODO there,
``utils/tools.py`` has ``save_hidden`` / ``load_hidden`` for exactly these rows, ``models.py:159`` asks for the attention scores).

Per batch the pass is the evaluation forward plus ONE collect launch (``mmda_misa_infer_collect``) on the same stream: no clone of the
workspace views, no read-back, no synchronisation.  In evaluation mode a sample's outputs do not depend on its batch companions, so
``InferencePass.run`` is free to batch a ``DeviceDataset`` by length -- fewer recurrent time steps than dataset order -- and still puts
row i at sample i: the plan's int32 order, uploaded once, is both what ``mmda_collate_gather`` gathers a batch by and where the collect
launch writes its rows.  DESIGN.md 4f.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, ops
from .data import PAD, UNK, batch_plan
from .modality import parse_keep

FIELDS = ("scores", "labels", "tcp", "hidden", "utterance", "attention")
ORDERS = ("length", "dataset")


def inference_plan(lengths, batch_size, order="length"):
    """(order, bounds) as ``batch_plan`` returns them, over all samples once.  ``order="length"``: the samples sorted by length
    descending (stable) and cut into batches -- the first batch is the longest, so the workspace is carved once at its largest and never
    grows mid-pass, and a batch pads almost nothing.  ``order="dataset"``: samples 0 .. n-1 cut into batches, each sorted as collate_fn
    sorts it (what ``DeviceLoader(dataset, batch_size)`` yields)."""
    if not isinstance(order, str) or order not in ORDERS:
        raise ValueError(f"order must be one of {ORDERS}, not {order!r}")
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    seq = np.argsort(-lengths, kind="stable") if order == "length" else np.arange(lengths.shape[0], dtype=np.int64)
    return batch_plan(lengths, seq, batch_size)


def _model_device(model, who):
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise _lib.MMDAError(f"{who}: the model is on {dev}; the pass runs on the GPU only (model.to('cuda'))")
    return dev


def _pass_device(model, dataset, who):
    """The device a pass of ``model`` over ``dataset`` (a ``DeviceDataset``) runs on; refuses, by ``who``'s name, anything off the GPU."""
    if torch.device(dataset.device).type != "cuda":
        raise _lib.MMDAError(f"{who}: the dataset is on {dataset.device}; the pass runs on the GPU only")
    dev = _model_device(model, who)
    if torch.device(dataset.device) != dev:
        raise _lib.MMDAError(f"{who}: the dataset is on {dataset.device}, the model on {dev}")
    return dev


def _eval_batch(m, t, v, a, lengths):
    """One batch of a pass: ``_prepare``, one seed drawn, the evaluation forward (dropout off, no stash)."""
    t, v, a, len_dev = m._prepare(t, v, a, lengths)
    m._forward_raw(t, v, a, len_dev, False, m._next_seed(), inference=True)


def dataset_pass(m, ds, plan, bounds, batch_size, dev, collect, keeps=None):
    """The loop of a pass over a device-resident dataset, shared by ``InferencePass.run``, ``EncoderCache.build``
    (mmda_amd/encoded.py) and ``ModalityPass.run`` (mmda_amd/modality.py): the plan's int32 order is uploaded once; every batch is one
    ``mmda_collate_gather`` into buffers sized once for the longest batch, ``_eval_batch``, and ``collect(dst_ptr)`` -- the caller's one
    launch, which copies what the forward left in the workspace to the rows the B int32 indices at ``dst_ptr`` name (the batch's
    samples).  No read-back, no synchronisation.  ``keeps``: keep sets (ints 0 .. 7); every batch is then gathered,
    evaluated and collected once per keep set k -- ``mmda_collate_gather_masked`` in the plain gather's place, ``collect(dst_ptr, k)``."""
    n = len(ds)
    if not n:
        return
    lib = m._lib
    order_dev = torch.from_numpy(plan.astype(np.int32)).pin_memory().to(dev, non_blocking=True)
    lens_np = np.asarray(ds.lengths, dtype=np.int64)[plan]
    lens_all = torch.from_numpy(lens_np)
    Bmax, Tmax = int(min(int(batch_size), n)), int(lens_np.max())
    ids_buf = torch.empty(Tmax * Bmax, dtype=torch.int64, device=dev)
    v_buf = torch.empty(Tmax * Bmax * ds.dv, device=dev)
    a_buf = torch.empty(Tmax * Bmax * ds.da, device=dev)
    y_buf = torch.empty(Bmax, device=dev)
    src = tuple(_lib.ptr(x) for x in (ds.words, ds.visual, ds.acoustic, ds.offsets, ds.emo, ds.sentiment))
    order_ptr = order_dev.data_ptr()
    no_drop = _lib.ModalityP()
    for lo, hi in zip(bounds[:-1].tolist(), bounds[1:].tolist()):
        B, T = hi - lo, int(lens_np[lo])
        ids, v, a = ids_buf[:T * B].view(T, B), v_buf[:T * B * ds.dv].view(T, B, ds.dv), a_buf[:T * B * ds.da].view(T, B, ds.da)
        if keeps is None:
            _lib.check(lib.mmda_collate_gather(*src, order_ptr + 4 * lo, B, T, ds.dv, ds.da, PAD, ids.data_ptr(), v.data_ptr(),
                                               a.data_ptr(), None, y_buf.data_ptr(), _lib.stream_ptr()), "mmda_collate_gather")
            _eval_batch(m, ids, v, a, lens_all[lo:hi])
            collect(order_ptr + 4 * lo)
            continue
        for k in keeps:
            _lib.check(lib.mmda_collate_gather_masked(*src, order_ptr + 4 * lo, B, T, ds.dv, ds.da, PAD, int(k), no_drop, 0, UNK,
                                                      ids.data_ptr(), v.data_ptr(), a.data_ptr(), None, y_buf.data_ptr(), None,
                                                      _lib.stream_ptr()), "mmda_collate_gather_masked")
            _eval_batch(m, ids, v, a, lens_all[lo:hi])
            collect(order_ptr + 4 * lo, k)


def _check_fields(fields):
    if isinstance(fields, str):
        fields = (fields,)
    fields = tuple(fields)
    if not fields:
        raise ValueError(f"fields is empty: name at least one of {FIELDS}")
    bad = [f for f in fields if not isinstance(f, str) or f not in FIELDS]
    if bad:
        raise ValueError(f"unknown field(s) {bad}: the fields are {FIELDS}")
    return tuple(f for f in FIELDS if f in fields)


class InferenceResult:
    """One tensor per requested field, row i = sample i: ``scores`` (n, C), ``labels`` (n, C) in {0, 1}, ``tcp`` (n, 6), ``hidden``
    (n, 6 hs) -- the reference's ``h = cat(h[0..5], dim=1)`` --, ``utterance`` (n, 6, hs) = [private t, v, a, shared t, v, a] and
    ``attention`` (n, 6, 6), the fusion layer's softmax averaged over its heads; a field that was not requested is None.  ``lengths``
    (n,) int64 on the host and ``segments`` (the samples' ids) come in the same order.  The tables are views of one flat buffer, so
    ``cpu()`` is one read-back of everything."""

    def __init__(self, flat, layout, n, lengths, segments):
        self._flat, self._layout, self.n = flat, layout, int(n)
        self.lengths, self.segments = lengths, segments
        self.fields = tuple(layout)
        for f in FIELDS:
            setattr(self, f, None)
        for f, (off, shape) in layout.items():
            setattr(self, f, flat[off:off + int(np.prod(shape))].view(shape)[:self.n])

    def __getitem__(self, field):
        if field not in self._layout:
            raise KeyError(field)
        return getattr(self, field)

    def __len__(self):
        return self.n

    def cpu(self):
        """The same result on the host: one device-to-host copy (and the one synchronisation of a pass)."""
        return InferenceResult(self._flat.cpu(), self._layout, self.n, self.lengths, self.segments)


class InferencePass:
    """``InferencePass(model, fields).run(dataset, batch_size, order)`` or ``.run_loader(loader)`` -> ``InferenceResult``.

    Every batch is ``model._prepare``, one seed drawn, the evaluation forward (dropout off whatever ``model.training`` says, no stash)
    and one collect launch.  ``model.training`` is not touched; the seed counter advances as one ``model(...)`` call per batch would
    advance it, so training that goes on after a pass is bit-identical to training after as many evaluation forwards.  The cluster
    status of the recurrences is read once, at the end (``check_cluster("inference")``, the pass's only wait besides ``cpu()``)."""

    def __init__(self, model, fields=("scores", "labels", "tcp", "hidden")):
        self.model = model
        self.fields = _check_fields(fields)

    # ------------------------------------------------------------------ tables
    def _device(self):
        return _model_device(self.model, "InferencePass")

    def _tables(self, rows, dev):
        cfg = self.model.config
        hs, nc = int(cfg.hidden_size), int(cfg.num_classes)
        shapes = dict(scores=(rows, nc), labels=(rows, nc), tcp=(rows, 6), hidden=(rows, 6 * hs), utterance=(rows, 6, hs),
                      attention=(rows, 6, 6))
        layout, cur = {}, 0
        for f in self.fields:
            layout[f] = (cur, shapes[f])
            cur += (int(np.prod(shapes[f])) + 3) // 4 * 4        # every table starts 16-byte aligned
        flat = torch.empty(cur, dtype=torch.float32, device=dev)
        out = _lib.InferOut()
        for f, (off, _) in layout.items():
            setattr(out, f, flat.data_ptr() + 4 * off)
        return flat, layout, out

    def _batch(self, t, v, a, lengths, out, dst_ptr, base):
        _eval_batch(self.model, t, v, a, lengths)
        ops.misa_infer_collect(self.model, out, dst_ptr, base)

    # ------------------------------------------------------------------ over a device-resident dataset
    def run(self, dataset, batch_size, order="length", keep=None):
        """Row i of every table is sample i of ``dataset`` (a ``DeviceDataset``), whatever ``order`` the batches are visited in
        (``inference_plan``).  Batches are gathered by ``mmda_collate_gather`` into buffers sized once for the longest batch.
        ``keep``: a keep set (``modality.parse_keep``) -- the batches are then gathered by
        ``mmda_collate_gather_masked`` with the other modalities blanked; None is the plain pass."""
        keeps = None if keep is None else (parse_keep(keep),)
        plan, bounds = inference_plan(dataset.lengths, batch_size, order)
        dev = _pass_device(self.model, dataset, "InferencePass")
        m, ds, n = self.model, dataset, len(dataset)
        flat, layout, out = self._tables(n, dev)
        lengths = torch.from_numpy(np.array(ds.lengths, dtype=np.int64))
        dataset_pass(m, ds, plan, bounds, batch_size, dev, lambda dst_ptr, k=None: ops.misa_infer_collect(m, out, dst_ptr, 0), keeps)
        m.check_cluster("inference")
        return InferenceResult(flat, layout, n, lengths, np.array(ds.segments, dtype=object))

    # ------------------------------------------------------------------ over any loader of the reference's tuples
    def run_loader(self, loader, keep=None):
        """``loader``: any iterable of the reference's 10-tuples (``DataLoader`` + ``collate_fn``, ``DevicePrefetcher``,
        ``DeviceLoader``, a list).  Rows come in the order the loader yields samples; ``segments`` is the tuples' last slot, ``lengths``
        their sixth, concatenated.

        Sizing the tables: ``len(loader.dataset)`` is used, as an upper bound on the samples one pass yields (a sampler, ``drop_last`` or
        a shard may yield fewer; the result is cut to the rows written), when the loader has a ``dataset`` with a length that is not the
        loader itself.  Otherwise -- a plain list, or a stand-in loader whose ``dataset`` is the loader -- a first counting pass over the
        batches' ``lengths`` sizes them, so such a loader must yield the same number of samples twice.

        ``keep``: a keep set (``modality.parse_keep``) -- every batch is masked, out of place, by one
        ``mmda_modality_mask`` launch in front of ``_prepare``; None is the plain pass.  A loader over the encoder cache is refused."""
        from . import step_rules
        from .encoded import EncodedLoader
        keep = None if keep is None else parse_keep(keep)
        step_rules.modality_check(keep, encoded=isinstance(loader, EncodedLoader))
        dev = self._device()
        m = self.model
        ds = getattr(loader, "dataset", None)
        if ds is not None and ds is not loader and hasattr(ds, "__len__"):
            rows = len(ds)
        else:
            rows = sum(int(len(batch[5])) for batch in loader)
        flat, layout, out = self._tables(rows, dev)
        lengths, segments, done = [], [], 0
        for batch in loader:
            t, v, a, l, ids = batch[0], batch[1], batch[2], batch[5], batch[9]
            l = torch.as_tensor(l).cpu()
            B = int(l.numel())
            if done + B > rows:
                raise _lib.MMDAError(f"InferencePass: the loader yields more than the {rows} samples its tables were sized for")
            t, v, a = (x if x.is_cuda else x.to(dev) for x in (t, v, a))
            if keep is not None:
                t, v, a = ops.modality_mask(t.contiguous(), v.contiguous().float(), a.contiguous().float(), keep)
            self._batch(t, v, a, l, out, None, done)
            lengths.append(l.to(torch.int64))
            segments.extend(list(ids))
            done += B
        m.check_cluster("inference")
        lengths = torch.cat(lengths) if lengths else torch.zeros(0, dtype=torch.int64)
        seg = np.empty(len(segments), dtype=object)
        for i, x in enumerate(segments):
            seg[i] = x
        return InferenceResult(flat, layout, done, lengths, seg)
