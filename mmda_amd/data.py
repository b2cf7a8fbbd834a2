"""Synthetic MOSEI-shaped batches with the reference's 10-tuple contract (reference data_loader.py:59-122).

Real CMU-MOSEI needs the mmsdk ETL and data that are not in this environment, so the loaders
here generate tensors of the same shapes, dtypes and ordering rules: batch sorted by length descending, time-major
``pad_sequence`` layout, PAD id 1 past each sample's length (create_dataset.py:25-27: <unk>=0, <pad>=1), emotion labels
binarised to {0,1} float32, CPU int64 ``lengths``.  The three BERT tensors are returned as zeros of shape (B, T+2):
they are ignored when use_bert=False.

For real samples (the reference's dataset items): ``collate_fn`` builds the same tuple on the host, ``DevicePrefetcher`` copies it one
batch ahead, and ``DeviceDataset`` / ``DeviceLoader`` keep the whole dataset on the device and gather each batch there in one launch.
"""
from __future__ import annotations

import torch

PAD, UNK = 1, 0


def synth_batch(config, B: int, T: int, seed: int, ragged: bool = False, device="cpu"):
    g = torch.Generator().manual_seed(1234 + seed)
    V = len(config.word2id)
    if ragged:
        lengths = torch.sort(torch.randint(1, T + 1, (B,), generator=g), descending=True).values
        lengths[0] = T
    else:
        lengths = torch.full((B,), T, dtype=torch.int64)
    t = torch.randint(2, V, (T, B), generator=g)
    v = torch.randn(T, B, config.visual_size, generator=g)
    a = torch.randn(T, B, config.acoustic_size, generator=g)
    mask = torch.arange(T).unsqueeze(1) >= lengths.unsqueeze(0)          # (T,B) True on padding
    t[mask] = PAD
    v[mask] = 0.0
    a[mask] = 0.0
    emo = (torch.rand(B, 6, generator=g) > 0.6).float()
    for c in range(6):                    # every class >= 1 positive so conf-loss' /nnz is finite (solver.py:459)
        if emo[:, c].sum() == 0:
            emo[c % B, c] = 1.0
    y = torch.randn(B, generator=g)
    bert = torch.zeros(B, T + 2, dtype=torch.int64)
    ids = [f"synthetic_{seed}_{i}" for i in range(B)]
    dev = torch.device(device)
    if dev.type != "cpu":
        t, v, a, y, emo = (x.to(dev) for x in (t, v, a, y, emo))
    return t, v, a, y, emo, lengths, bert, bert, bert, ids


class SyntheticLoader:
    """Iterable of pre-generated batches (a stand-in for DataLoader(MSADataset, collate_fn))."""

    def __init__(self, config, n_batches: int, batch_size: int, seq_len: int, seed: int = 0, ragged: bool = True, device="cpu"):
        self.batches = [synth_batch(config, batch_size, seq_len, seed * 1000 + i, ragged, device) for i in range(n_batches)]
        self.dataset = self
        self.batch_size = batch_size

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


def get_loader(config, shuffle=True, n_batches=8, seed=0, ragged=True, device="cpu"):
    """Same name as the reference's factory (data_loader.py:50); synthetic data."""
    config.data_len = n_batches * config.batch_size
    return SyntheticLoader(config, n_batches, config.batch_size, getattr(config, "seq_len", 50), seed, ragged, device)


# ---------------------------------------------------------------------------------------------- collate (reference data_loader.py:59-122)
def collate_fn(batch, use_bert: bool = False):
    """The reference's collate for samples ``((word_ids, visual (L,dv), acoustic (L,da), words), label (1,7) | (1,1), segment)``:
    sort by length descending, time-major zero/PAD padding, MOSEI labels (1,7) = [sentiment, 6 emotion scores] -> ``labels``
    (B,) sentiment and ``emo_labels`` (B,6) float32 {0,1} (score > 0), NaNs in labels replaced by 0, int64 CPU ``lengths``.
    Vectorised: one pass per tensor instead of the reference's per-sample pad_sequence / torch.cat calls.  Without BERT
    (``use_bert=False``, the branch this build covers) the three BERT tensors are zeros of shape (B, T+2): the reference
    tokenises every sample here even when the model ignores the result."""
    import numpy as np
    batch = sorted(batch, key=lambda x: np.asarray(x[0][0]).shape[0], reverse=True)      # stable, like the reference
    B = len(batch)
    lens = [int(np.asarray(s[0][0]).shape[0]) for s in batch]
    T = lens[0] if B else 0
    dv = np.asarray(batch[0][0][1]).shape[1]; da = np.asarray(batch[0][0][2]).shape[1]
    sent = np.full((T, B), PAD, dtype=np.int64)
    vis = np.zeros((T, B, dv), dtype=np.float32)
    aco = np.zeros((T, B, da), dtype=np.float32)
    for b, s in enumerate(batch):
        L = lens[b]
        sent[:L, b] = np.asarray(s[0][0], dtype=np.int64)
        vis[:L, b] = np.asarray(s[0][1], dtype=np.float32)
        aco[:L, b] = np.asarray(s[0][2], dtype=np.float32)
    lab = np.stack([np.nan_to_num(np.asarray(s[1], dtype=np.float64))[0] for s in batch]) if B else np.zeros((0, 1))
    if lab.shape[1] == 7:
        emo = (lab[:, 1:] > 0.0).astype(np.float32)
        labels = lab[:, 0].astype(np.float32)
        emo_t = torch.from_numpy(emo)
    else:
        labels = lab[:, 0].astype(np.float32)
        emo_t = None
    ids = [s[2] for s in batch]
    bert = torch.zeros(B, T + 2, dtype=torch.int64)
    return (torch.from_numpy(sent), torch.from_numpy(vis), torch.from_numpy(aco), torch.from_numpy(labels), emo_t,
            torch.tensor(lens, dtype=torch.int64), bert, bert, bert, ids)


class DevicePrefetcher:
    """Wraps a loader of reference-style host batches and copies each batch to the device ONE BATCH AHEAD on a dedicated HIP
    stream, so the copies of batch i+1 run beside the kernels of batch i and the training loop only ever sees device tensors.
    ``lengths`` stays on the host like the reference (pack_padded_sequence wants it there); ids pass through.

    Source tensors are copied as they are: pageable ones through the runtime's own staging (the call returns when the data has
    left the tensor), page-locked ones asynchronously.  Staging through our own page-locked buffers was measured and dropped:
    CPU writes into hipHostMalloc memory ran at ~0.2 GB/s on the MI355X hosts (3.3 ms for a 0.75 MB batch), against 0.35 ms
    for the plain pageable copies of the same batch.
    """

    def __init__(self, loader, device):
        self.loader = loader
        self.device = torch.device(device)
        self.stream = torch.cuda.Stream(device=self.device) if self.device.type == "cuda" else None

    def __len__(self):
        return len(self.loader)

    def _stage(self, batch):
        if self.stream is None:
            return batch, None
        out = []
        with torch.cuda.stream(self.stream):
            for i, x in enumerate(batch):
                if torch.is_tensor(x) and i != 5 and not x.is_cuda:        # index 5 = lengths: host side
                    out.append(x.to(self.device, non_blocking=x.is_pinned()))
                else:
                    out.append(x)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        return tuple(out), ev

    def __iter__(self):
        it = iter(self.loader)
        try:
            nxt = self._stage(next(it))
        except StopIteration:
            return
        for batch in it:
            cur, ev = nxt
            nxt = self._stage(batch)                  # the next batch's copies run beside this batch's compute
            yield self._hand_over(cur, ev)
        yield self._hand_over(*nxt)

    def _hand_over(self, cur, ev):
        """Make the compute stream wait for the copies and tell the caching allocator that the compute stream uses these
        tensors: they were allocated on the copy stream, and without record_stream their memory could be handed to the next
        batch's copy while kernels of this step (the host runs several steps ahead of the GPU) have not read them yet."""
        if ev is not None:
            cs = torch.cuda.current_stream(self.device)
            cs.wait_event(ev)
            for x in cur:
                if torch.is_tensor(x) and x.is_cuda:
                    x.record_stream(cs)
        return cur


# ---------------------------------------------------------------------------------------------- device-resident dataset
class DeviceDataset:
    """A whole dataset of reference-style samples on the device, uploaded once: the samples' time positions back to back (``words`` int32
    (P,), ``visual`` (P, dv), ``acoustic`` (P, da)), ``offsets`` int64 (n + 1,), and per sample ``sentiment`` (n,) and ``emo`` (n, 6) or
    None.  A batch is then a pure function of B sample indices: ``DeviceLoader`` gathers it with one launch.  ``lengths`` (int64) and
    ``segments`` (object) stay on the host: the batch plan is made from the one, the batch's id list from the other."""

    def __init__(self, words, visual, acoustic, offsets, emo, sentiment, lengths, segments):
        self.words, self.visual, self.acoustic, self.offsets, self.emo, self.sentiment = words, visual, acoustic, offsets, emo, sentiment
        self.lengths, self.segments = lengths, segments
        self.device = words.device
        self.dv, self.da = int(visual.shape[1]), int(acoustic.shape[1])

    def __len__(self):
        return int(self.lengths.shape[0])

    @classmethod
    def from_samples(cls, samples, device):
        """``samples[i]`` is what the reference's ``MSADataset[i]`` returns: ``((word_ids, visual (L, dv), acoustic (L, da), words),
        label (1, 7) | (1, 1), segment)``.  The label columns are made with collate_fn's own numpy operations, so a gathered batch
        equals a collated one bit for bit; (1, 1) labels mean no emotion table."""
        import numpy as np
        from ._lib import MMDAError
        device = torch.device(device)
        if device.type != "cuda":
            raise MMDAError(f"DeviceDataset lives on the GPU (device={device}): there is no CPU path, use DataLoader + collate_fn")
        n = len(samples)
        if n == 0:
            raise ValueError("DeviceDataset: the dataset is empty")
        words = [np.asarray(s[0][0], dtype=np.int64).reshape(-1) for s in samples]
        visual = [np.asarray(s[0][1], dtype=np.float32) for s in samples]
        acoustic = [np.asarray(s[0][2], dtype=np.float32) for s in samples]
        lengths = np.array([w.shape[0] for w in words], dtype=np.int64)
        if int(lengths.min()) <= 0:
            raise ValueError(f"DeviceDataset: sample {int(lengths.argmin())} has length zero")
        for i, (v, a) in enumerate(zip(visual, acoustic)):
            if v.ndim != 2 or a.ndim != 2 or v.shape[0] != lengths[i] or a.shape[0] != lengths[i]:
                raise ValueError(f"DeviceDataset: sample {i}: visual / acoustic must be (L, d) with the L of its word ids")
            if v.shape[1] != visual[0].shape[1] or a.shape[1] != acoustic[0].shape[1]:
                raise ValueError(f"DeviceDataset: sample {i} has feature widths ({v.shape[1]}, {a.shape[1]}), sample 0 has "
                                 f"({visual[0].shape[1]}, {acoustic[0].shape[1]})")
        if visual[0].shape[1] == 0 or acoustic[0].shape[1] == 0:
            raise ValueError("DeviceDataset: zero feature width")
        flat_w = np.concatenate(words)
        if flat_w.min() < -2 ** 31 or flat_w.max() >= 2 ** 31:
            raise ValueError("DeviceDataset: word ids must fit int32")
        lab = np.stack([np.nan_to_num(np.asarray(s[1], dtype=np.float64))[0] for s in samples])            # as collate_fn does
        emo = (lab[:, 1:] > 0.0).astype(np.float32) if lab.shape[1] == 7 else None
        sentiment = lab[:, 0].astype(np.float32)
        offsets = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(lengths, out=offsets[1:])
        segments = np.empty(n, dtype=object)
        for i, s in enumerate(samples):
            segments[i] = s[2]
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(device)
        return cls(up(flat_w.astype(np.int32)), up(np.concatenate(visual)), up(np.concatenate(acoustic)), up(offsets),
                   None if emo is None else up(emo), up(sentiment), lengths, segments)


def class_pos_weight(labels, cap=None):
    """Per-class positive weights ``(N - n_c) / n_c`` of an (N, C) label table (``BCEWithLogitsLoss``'s ``pos_weight`` convention),
    n_c the rows with an entry > 0 in class c: what ``config.pos_weight = "balanced"`` resolves to.  ``labels``: a tensor, or a
    ``DeviceDataset`` (its ``emo`` table).  On the device the counts are one ``mmda_label_counts`` launch, exact 64-bit integers; a CPU
    tensor is counted with a torch sum.  A class with no positive gets 1.0; ``cap`` clips from above.  Returns C float64 values on the
    host."""
    from . import _lib
    if isinstance(labels, DeviceDataset):
        if labels.emo is None:
            raise ValueError("class_pos_weight: the dataset has no emotion labels")
        labels = labels.emo
    if not torch.is_tensor(labels) or labels.dim() != 2 or labels.shape[1] < 1:
        raise ValueError("class_pos_weight: an (N, C) label tensor or a DeviceDataset is expected")
    if cap is not None and not float(cap) > 0.0:
        raise ValueError(f"class_pos_weight: cap must be > 0, not {cap}")
    N, C = int(labels.shape[0]), int(labels.shape[1])
    if labels.is_cuda:
        lab = labels.detach().to(torch.float32).contiguous()
        counts = torch.zeros(C, dtype=torch.int64, device=lab.device)
        _lib.check(_lib.load().mmda_label_counts(lab.data_ptr(), N, C, counts.data_ptr(), _lib.stream_ptr()), "mmda_label_counts")
        n = counts.cpu()
    else:
        n = (labels.detach() > 0).sum(dim=0).to(torch.int64)
    n = n.to(torch.float64)
    w = torch.where(n > 0, (N - n) / n.clamp(min=1.0), torch.ones_like(n))
    return w if cap is None else w.clamp(max=float(cap))


def host_labels(dataset):
    """One host pass over a dataset's labels -> (N, C) float tensor of 0 / 1, for loaders whose data is not resident on the device.  An
    item is a reference-style sample ``(features, label (1, 7), segment)`` -- columns 1.. of the label, as collate_fn reads them -- or an
    already collated batch (its fifth entry is the emotion table)."""
    import numpy as np
    rows = []
    for item in dataset:
        if len(item) == 3:
            lab = np.nan_to_num(np.asarray(item[1], dtype=np.float64)).reshape(1, -1)
            if lab.shape[1] < 2:
                raise ValueError("pos_weight='balanced': the dataset's samples carry no emotion labels")
            rows.append(torch.from_numpy((lab[:, 1:] > 0.0).astype(np.float32)))
        else:
            rows.append((torch.as_tensor(item[4]).detach().cpu().float() > 0).float())
    if not rows:
        raise ValueError("pos_weight='balanced': the training set is empty")
    return torch.cat(rows, 0)


def _kept(m, batch_size, drop_last=False, shard=None):
    """How much of an index sequence of ``m`` entries one rank batches, as ``(prefix, per_rank, batches)``: the sequence is cut to its
    first ``prefix`` entries (a multiple of ``world * batch_size`` under ``drop_last``, else of ``world``; all of it without a shard),
    the rank keeps ``per_rank`` of them -- less the short tail under ``drop_last`` -- in ``batches`` batches.  The one place that knows
    the rule: ``batch_plan`` cuts by it and ``DeviceLoader.__len__`` counts by it; it validates ``batch_size`` and ``shard`` too."""
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError("batch_size must be positive")
    world = 1
    if shard is not None:
        rank, world = int(shard[0]), int(shard[1])
        if world < 1 or not 0 <= rank < world:
            raise ValueError(f"shard=(rank, world)={tuple(shard)} needs 0 <= rank < world")
    unit = world * batch_size if (drop_last and shard is not None) else world
    prefix = m // unit * unit
    per_rank = prefix // world
    if drop_last:
        per_rank = per_rank // batch_size * batch_size
    return prefix, per_rank, (per_rank + batch_size - 1) // batch_size


def batch_plan(lengths, indices, batch_size, drop_last=False, shard=None):
    """The batches ``DataLoader(batch_size=..., collate_fn=collate_fn)`` makes of the index sequence ``indices``, as two int64 arrays:
    ``order``, the sample indices of all batches back to back, each batch sorted by length descending (stable, as collate_fn's
    ``sorted(..., reverse=True)``), and ``bounds`` (batches + 1,): batch k is ``order[bounds[k]:bounds[k + 1]]``, its T is the length of its
    first sample.  ``shard=(rank, world)``: the sequence is first cut to a multiple of ``world * batch_size`` (``drop_last``) or of
    ``world``, then rank r keeps ``indices[r::world]`` -- every rank gets the same number of batches of the same sizes, so the collectives
    of data-parallel training line up."""
    import numpy as np
    lengths = np.asarray(lengths, dtype=np.int64)
    idx = np.asarray(indices)
    if idx.size and idx.dtype.kind not in "iu":
        raise TypeError("batch_plan: indices must be integers")
    idx = idx.astype(np.int64).reshape(-1)
    batch_size = int(batch_size)
    prefix, per_rank, _ = _kept(idx.size, batch_size, drop_last, shard)
    n = lengths.shape[0]
    if idx.size and (int(idx.min()) < 0 or int(idx.max()) >= n):
        raise IndexError(f"batch_plan: sample index outside [0, {n})")
    if shard is not None:
        idx = idx[:prefix][int(shard[0])::int(shard[1])]
    idx = idx[:per_rank]
    starts = np.arange(0, idx.size, batch_size, dtype=np.int64)
    bounds = np.append(starts, idx.size).astype(np.int64)
    order = np.empty_like(idx)
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        chunk = idx[lo:hi]
        order[lo:hi] = chunk[np.argsort(-lengths[chunk], kind="stable")]
    return order, bounds


class DeviceLoader:
    """Drop-in for ``DataLoader(dataset, batch_size, collate_fn=collate_fn)`` over a ``DeviceDataset``: the same 10-tuples, bit for bit,
    for the same index sequence, with the batch tensors made on the device.  An epoch draws its index sequence (``sampler``, else
    ``torch.randperm(n, generator=generator)`` when ``shuffle``, else 0 .. n-1), plans its batches on the host (``batch_plan``) and uploads
    the order once; a batch is then five ``torch.empty`` and one ``mmda_collate_gather`` launch on the current stream -- no copy in either
    direction, no synchronisation.  The outputs belong to the stream they were made on (the caching allocator's stream ordering keeps them
    valid while the host runs ahead): consume a batch on the stream that was current when it was yielded.  Every tensor of a yielded
    tuple is the batch's own, as with ``collate_fn`` -- except the three BERT slots, which are one cached all-zero CPU tensor per shape
    (``use_bert=False``: nothing reads them), shared by the three slots, by every batch of that shape and across epochs: do not write
    into it.

    Modality masking (mmda_amd/modality.py).  ``modality_dropout=(p_t, p_v, p_a)``: every sample's text / visual /
    acoustic input is blanked with that probability (never all three), a function of (seed, the sample's dataset index) and so
    independent of batch size and order; ``keep``: a fixed keep set (an int 0 .. 7 or modality names) ANDed with the random one.  With
    either given, every batch is one ``mmda_collate_gather_masked`` launch in the plain launch's place, under the seed
    ``(modality_seed + epoch) mod 2^64``; ``epoch`` counts the ``__iter__`` calls from 0 (``set_epoch(e)`` sets the next one), and
    ``last_keep`` is the device uint8 (B,) of the keep sets of the batch just yielded.  With all three at their defaults the loader
    calls ``mmda_collate_gather`` exactly as it always has (``last_keep`` stays None)."""

    def __init__(self, dataset, batch_size, shuffle=False, sampler=None, generator=None, drop_last=False, shard=None,
                 modality_dropout=None, modality_seed=0, keep=None):
        from .modality import parse_dropout, parse_keep
        if sampler is not None and shuffle:
            raise ValueError("sampler option is mutually exclusive with shuffle")
        self.dataset, self.batch_size, self.shuffle, self.sampler, self.generator = dataset, int(batch_size), bool(shuffle), sampler, generator
        self.drop_last, self.shard = bool(drop_last), shard
        _kept(0, self.batch_size, self.drop_last, shard)            # refuses a bad batch_size / shard here, not at the first epoch
        self._bert = {}                      # (B, T + 2) -> the zero tensor the three BERT slots share (use_bert=False)
        self.modality_dropout = parse_dropout(modality_dropout)
        if isinstance(modality_seed, bool) or not isinstance(modality_seed, int):
            raise ValueError(f"modality_seed must be an int, not {modality_seed!r}")
        self.modality_seed = modality_seed
        self.keep = None if keep is None else parse_keep(keep)
        self.epoch, self.last_keep = 0, None

    def set_epoch(self, epoch):
        """The epoch number the next ``__iter__`` runs under (the random keep sets' seed is ``modality_seed + epoch``)."""
        if isinstance(epoch, bool) or not isinstance(epoch, int) or epoch < 0:
            raise ValueError(f"epoch must be an int >= 0, not {epoch!r}")
        self.epoch = epoch

    @property
    def masked(self):
        return self.modality_dropout is not None or self.keep is not None

    def __len__(self):
        m = len(self.sampler) if self.sampler is not None else len(self.dataset)
        return _kept(m, self.batch_size, self.drop_last, self.shard)[2]

    def _indices(self):
        import numpy as np
        if self.sampler is not None:
            return np.fromiter(iter(self.sampler), dtype=np.int64)
        if self.shuffle:
            return torch.randperm(len(self.dataset), generator=self.generator).numpy()
        return np.arange(len(self.dataset), dtype=np.int64)

    def __iter__(self):
        import numpy as np
        from . import _lib
        ds = self.dataset
        epoch, self.epoch = self.epoch, self.epoch + 1
        order, bounds = batch_plan(ds.lengths, self._indices(), self.batch_size, self.drop_last, self.shard)
        if order.size == 0:
            return
        lib = _lib.load()
        masked = self.masked
        if masked:
            keep_const = 7 if self.keep is None else self.keep
            p = _lib.ModalityP((_lib.C.c_float * 3)(*(self.modality_dropout or (0.0, 0.0, 0.0))))
            seed = (self.modality_seed + epoch) % (1 << 64)
        # the epoch's one host-to-device copy, from page-locked memory so that it does not wait for the device either
        order_dev = torch.from_numpy(order.astype(np.int32)).pin_memory().to(ds.device, non_blocking=True)
        lens_np = ds.lengths[order]
        lens_all = torch.from_numpy(lens_np)
        segs_all = ds.segments[order]
        src = tuple(_lib.ptr(x) for x in (ds.words, ds.visual, ds.acoustic, ds.offsets, ds.emo, ds.sentiment))
        order_ptr, dev, dv, da = order_dev.data_ptr(), ds.device, ds.dv, ds.da
        for lo, hi in zip(bounds[:-1].tolist(), bounds[1:].tolist()):
            B, T = hi - lo, int(lens_np[lo])
            ids = torch.empty(T, B, dtype=torch.int64, device=dev)
            v = torch.empty(T, B, dv, device=dev)
            a = torch.empty(T, B, da, device=dev)
            emo = torch.empty(B, 6, device=dev) if ds.emo is not None else None
            y = torch.empty(B, device=dev)
            if masked:
                self.last_keep = kept = torch.empty(B, dtype=torch.uint8, device=dev)
                _lib.check(lib.mmda_collate_gather_masked(*src, order_ptr + 4 * lo, B, T, dv, da, PAD, keep_const, p, seed, UNK,
                                                          ids.data_ptr(), v.data_ptr(), a.data_ptr(), _lib.ptr(emo), y.data_ptr(),
                                                          kept.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
                           "mmda_collate_gather_masked")
            else:
                _lib.check(lib.mmda_collate_gather(*src, order_ptr + 4 * lo, B, T, dv, da, PAD, ids.data_ptr(), v.data_ptr(),
                                                   a.data_ptr(), _lib.ptr(emo), y.data_ptr(),
                                                   torch.cuda.current_stream(dev).cuda_stream), "mmda_collate_gather")
            bert = self._bert.get((B, T + 2))
            if bert is None:
                bert = self._bert[(B, T + 2)] = torch.zeros(B, T + 2, dtype=torch.int64)
            yield ids, v, a, y, emo, lens_all[lo:hi].clone(), bert, bert, bert, segs_all[lo:hi].tolist()
