"""Modality masking: what each of the three inputs -- 0 = text, 1 = visual, 2 = acoustic -- contributes, per sample and per class, and
training with an input blanked at random (modality dropout).  The reference leaves the question as a stub (``utils/tools.py`` has a
broken ``random_shuffle`` and ``# TODO: Implement tcp saving``, ``inference.py`` is one TODO line).  DESIGN.md 4n.

A *keep set* is three bits, bit m set = modality m is kept; 7 keeps everything, 0 nothing.  Masking a column of a batch: every word id
at ``t < len`` becomes ``UNK`` (padding keeps ``PAD``), the column's visual / acoustic rows become 0.0; lengths, labels and segments do
not change and nothing is rescaled (input blanking, not inverted dropout).

The random keep set of SAMPLE s is a function of its dataset index, not of its batch position: with
``u_m = (float)(rng_u32(seed, 11, 3 s + m) >> 8) * 2^-24`` (``csrc/common.h``'s generator at the site ``SITE_MODALITY``), modality m is
dropped iff ``p_m > 0 and u_m < p_m`` in fp32; a draw that would drop all three drops none.  ``keep_bits`` restates that in numpy.

On the device (``csrc/modality.hip``): ``mmda_collate_gather_masked`` makes a masked batch in the one launch that gathers it,
``mmda_modality_mask`` masks a batch that exists already, out of place, and ``mmda_modality_attrib`` turns the values under the eight
keep sets into exact Shapley values.  ``ModalityPass`` runs a model over a split under all eight keep sets with no read-back.
"""
from __future__ import annotations

import numpy as np

MODALITIES = ("text", "visual", "acoustic")
SITE_MODALITY = 11                       # the next free id after csrc/misa.hip's dropout sites
KEEP_ALL = 7
VALUES = ("scores", "tcp")

_M64 = (1 << 64) - 1
_GOLD = np.uint64(0x9E3779B97F4A7C15)
_STRIDE = np.uint64(0xD6E8FEB86659FD93)
_MIX1 = np.uint64(0xFF51AFD7ED558CCD)
_MIX2 = np.uint64(0xC4CEB9FE1A85EC53)
_S33 = np.uint64(33)


def _rng_u32(seed: int, site: int, idx) -> np.ndarray:
    """``common.h: rng_u32`` in uint64 arithmetic modulo 2^64: murmur3 fmix64 of seed + GOLD (site + 1) + idx STRIDE, bits 16 .. 47."""
    idx = np.asarray(idx, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(int(seed) & _M64) + _GOLD * np.uint64(site + 1) + idx * _STRIDE
        z = z ^ (z >> _S33); z = z * _MIX1
        z = z ^ (z >> _S33); z = z * _MIX2
        z = z ^ (z >> _S33)
    return ((z >> np.uint64(16)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def parse_dropout(modality_dropout):
    """None, or the three drop rates (p_t, p_v, p_a) as Python floats, each in [0, 1)."""
    if modality_dropout is None:
        return None
    try:
        p = tuple(float(x) for x in modality_dropout)
    except TypeError:
        raise ValueError(f"modality_dropout must be None or three rates (p_t, p_v, p_a), not {modality_dropout!r}") from None
    if len(p) != 3:
        raise ValueError(f"modality_dropout must be None or three rates (p_t, p_v, p_a), not {modality_dropout!r}")
    for m, x in zip(MODALITIES, p):
        if not 0.0 <= x < 1.0:
            raise ValueError(f"modality_dropout: the rate of {m} must lie in [0, 1), not {x}")
    return p


def parse_keep(keep) -> int:
    """A keep set as its three bits.  ``keep``: None (everything, 7), an int 0 .. 7, one of the names ``"text"``, ``"visual"``,
    ``"acoustic"``, or a collection of them (duplicates are fine, an empty collection keeps nothing)."""
    if keep is None:
        return KEEP_ALL
    if isinstance(keep, bool):
        raise ValueError(f"keep must be an int 0 .. 7 or modality names {MODALITIES}, not {keep!r}")
    if isinstance(keep, (int, np.integer)):
        if not 0 <= int(keep) <= 7:
            raise ValueError(f"keep = {int(keep)} is outside 0 .. 7 (bit m set = modality m of {MODALITIES} is kept)")
        return int(keep)
    names = (keep,) if isinstance(keep, str) else tuple(keep)
    bits = 0
    for name in names:
        if not isinstance(name, str) or name not in MODALITIES:
            raise ValueError(f"keep names {name!r}: the modalities are {MODALITIES}")
        bits |= 1 << MODALITIES.index(name)
    return bits


def keep_names(bits: int):
    return tuple(m for i, m in enumerate(MODALITIES) if bits >> i & 1)


def keep_bits(seed: int, p, sample_indices) -> np.ndarray:
    """The random keep sets of the samples ``sample_indices`` (dataset indices) under the drop rates ``p = (p_t, p_v, p_a)`` and
    ``seed``: uint8, same shape.  The device computes the same bits (``csrc/modality.hip: random_keep``)."""
    s = np.asarray(sample_indices, dtype=np.uint64)
    drop = np.zeros(s.shape, dtype=np.uint8)
    with np.errstate(over="ignore"):
        for m in range(3):
            p32 = np.float32(p[m])
            if not p32 > np.float32(0.0):
                continue
            u = (_rng_u32(seed, SITE_MODALITY, s * np.uint64(3) + np.uint64(m)) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
            drop |= (u < p32).astype(np.uint8) << np.uint8(m)
    drop[drop == 7] = 0                   # a sample is never emptied by chance
    return (np.uint8(7) & ~drop).astype(np.uint8)


def mask_batch(ids, v, a, keep, pad_id=None, unk_id=None):
    """The mask on the host, for tests and for loaders that are lists of host batches: numpy arrays ``ids (T, B)``, ``v (T, B, dv)``,
    ``a (T, B, da)`` and ``keep``, an int or B keep sets -> masked copies.  Padding is recognised by ``ids == PAD``."""
    from .data import PAD, UNK
    pad_id, unk_id = PAD if pad_id is None else pad_id, UNK if unk_id is None else unk_id
    ids, v, a = np.array(ids), np.array(v), np.array(a)
    k = np.broadcast_to(np.asarray(keep, dtype=np.uint8), (ids.shape[1],))
    ids[(ids != pad_id) & ((k & 1) == 0)[None, :]] = unk_id
    v[:, (k & 2) == 0] = 0.0
    a[:, (k & 4) == 0] = 0.0
    return ids, v, a


def shapley3(V):
    """float64 restatement of ``mmda_modality_attrib``'s two tables: ``V (8, ...)`` -> ``phi (3, ...)``, ``loo (3, ...)``."""
    V = np.asarray(V, dtype=np.float64)
    phi, loo = np.zeros((3,) + V.shape[1:]), np.zeros((3,) + V.shape[1:])
    for m in range(3):
        bit = 1 << m
        for S in range(8):
            if S & bit:
                continue
            w = (1.0 / 3.0, 1.0 / 6.0, 1.0 / 3.0)[bin(S).count("1")]
            phi[m] += w * (V[S | bit] - V[S])
        loo[m] = V[7] - V[7 ^ bit]
    return phi, loo


# ---------------------------------------------------------------------------------------------- the pass
class ModalityResult:
    """The values of a split under the eight keep sets, on the device, row i = sample i: ``scores (8, n, C)`` and ``tcp (8, n, 6)``
    (None where not collected); ``lengths`` (n,) int64 on the host, ``segments``, and ``truth (n, C)``, the split's labels, when the
    pass knew them.  Slice k is what the model gives with keep set k: 7 is the whole input, 0 an input of which only the lengths are left."""

    def __init__(self, scores, tcp, lengths, segments, truth=None, threshold=0.5, task="emotion"):
        self.scores, self.tcp, self.lengths, self.segments, self.truth = scores, tcp, lengths, segments, truth
        self.threshold, self.task = threshold, task
        self.n = int((scores if scores is not None else tcp).shape[1])

    def __len__(self):
        return self.n

    def _value(self, which):
        if which not in VALUES:
            raise ValueError(f"attribution of {which!r}: the values are {VALUES}")
        V = getattr(self, which)
        if V is None:
            raise ValueError(f"attribution of {which!r}: the pass did not collect it (ModalityPass(model, values=...))")
        return V

    def attribution(self, which="scores"):
        """``dict(phi (n, 3, C), loo (n, 3, C), dominant (n, C) int32, counts (3, C) int64)`` of ``scores`` or ``tcp`` from one
        ``mmda_modality_attrib`` launch: the exact Shapley value of each modality, the leave-one-out difference ``V[7] - V[7 without
        m]``, the modality with the largest Shapley value and how many rows each modality dominates per class."""
        from . import ops
        return dict(zip(("phi", "loo", "dominant", "counts"), ops.modality_attrib(self._value(which))))

    def metrics(self, truth=None, threshold=None):
        """The reference's ``get_metrics`` figures (and ``acc``, ``keep``, ``kept``) per keep set, a list of eight dicts, counted on the
        device by ``DeviceEval`` from ``scores[k] > threshold``.  ``truth (n, C)``: the labels, row i = sample i (None: the pass's
        own).  ``threshold``: None (the model's ``config.threshold``), a number, C numbers, or a ``Thresholds`` from ``calibrate``."""
        import torch
        from . import _lib
        from .utils.eval import DeviceEval
        if self.task == "sentiment":
            raise _lib.MMDAError("ModalityResult.metrics under task='sentiment' is not built: the figures are classification figures")
        S = self._value("scores")
        truth = self.truth if truth is None else truth
        if truth is None:
            raise ValueError("metrics: the pass has no labels of its own; give truth (n, C)")
        C = int(S.shape[2])
        truth = torch.as_tensor(truth).to(device=S.device, dtype=torch.float32).contiguous()
        if tuple(truth.shape) != (self.n, C):
            raise ValueError(f"metrics: truth is {tuple(truth.shape)}, the scores are {(self.n, C)}")
        thr = self.threshold if threshold is None else getattr(threshold, "values", threshold)
        thr = torch.as_tensor(thr, dtype=torch.float32).reshape(-1).to(S.device)
        if thr.numel() == 1:
            thr = thr.expand(C)
        if thr.numel() != C:
            raise ValueError(f"metrics: threshold has {thr.numel()} entries, the scores {C} classes")
        thr, lib, out = thr.contiguous(), _lib.load(), []
        for k in range(8):
            ev = DeviceEval(C, S.device)
            _lib.check(lib.mmda_eval_accumulate_thr(S[k].data_ptr(), truth.data_ptr(), self.n, C, thr.data_ptr(), None,
                                                    ev.state.data_ptr(), _lib.stream_ptr()), "mmda_eval_accumulate_thr")
            m = ev.result()[2]
            out.append(dict(m, keep=k, kept=keep_names(k)))
        return out

    def bootstrap(self, truth=None, threshold=None, replicates=2000, seed=0, alpha=0.05):
        """The eight keep sets' decision figures with bootstrap intervals (mmda_amd/bootstrap.py), the same resamples for all eight:
        ``dict(bootstrap, names, results, summary, vs_full)`` -- ``results`` the eight ``BootstrapResult``s (labels
        ``scores[k] > threshold``, as ``metrics`` makes them), ``summary`` their (8, F, 6) table of point, mean, std, lo, hi, defined on
        the device, ``vs_full`` the (8, F, 9) paired differences ``keep set k - keep set 7``; F = 10 + 3 C, named by ``names``.
        ``truth`` / ``threshold``: as for ``metrics``."""
        import torch
        from . import _lib
        from .bootstrap import Bootstrap
        if self.task == "sentiment":
            raise _lib.MMDAError("ModalityResult.bootstrap under task='sentiment' is not built: the figures are classification figures")
        S = self._value("scores")
        truth = self.truth if truth is None else truth
        if truth is None:
            raise ValueError("bootstrap: the pass has no labels of its own; give truth (n, C)")
        C = int(S.shape[2])
        truth = torch.as_tensor(truth).to(device=S.device, dtype=torch.float32).contiguous()
        if tuple(truth.shape) != (self.n, C):
            raise ValueError(f"bootstrap: truth is {tuple(truth.shape)}, the scores are {(self.n, C)}")
        thr = self.threshold if threshold is None else getattr(threshold, "values", threshold)
        thr = torch.as_tensor(thr, dtype=torch.float32).reshape(-1).to(S.device)
        if thr.numel() == 1:
            thr = thr.expand(C)
        if thr.numel() != C:
            raise ValueError(f"bootstrap: threshold has {thr.numel()} entries, the scores {C} classes")
        thr, lib = thr.contiguous(), _lib.load()
        bs = Bootstrap(self.n, replicates, seed, S.device)
        results = []
        for k in range(8):
            labels = torch.empty(self.n, C, dtype=torch.float32, device=S.device)
            scratch = torch.zeros(3 * C + 2, dtype=torch.float64, device=S.device)
            _lib.check(lib.mmda_eval_accumulate_thr(S[k].data_ptr(), truth.data_ptr(), self.n, C, thr.data_ptr(), labels.data_ptr(),
                                                    scratch.data_ptr(), _lib.stream_ptr()), "mmda_eval_accumulate_thr")
            results.append(bs.decisions(labels, truth))
        return dict(bootstrap=bs, names=results[7].names, results=results,
                    summary=torch.stack([r.summary(alpha).table for r in results]),
                    vs_full=torch.stack([bs.compare(r, results[7], alpha).table for r in results]))

    def cpu(self):
        """The same result on the host."""
        mv = lambda x: None if x is None else x.cpu()
        return ModalityResult(mv(self.scores), mv(self.tcp), self.lengths, self.segments, mv(self.truth), self.threshold, self.task)

    def as_dict(self):
        """Host numpy arrays: scores, tcp (where collected), and per collected value ``phi_*``, ``loo_*``, ``dominant_*``, ``counts_*``."""
        out = dict(lengths=np.asarray(self.lengths), segments=self.segments)
        for which in VALUES:
            V = getattr(self, which)
            if V is None:
                continue
            out[which] = V.cpu().numpy()
            if V.is_cuda:
                for k, x in self.attribution(which).items():
                    out[f"{k}_{which}"] = x.cpu().numpy()
        return out


class ModalityPass:
    """``ModalityPass(model, values=("scores", "tcp")).run(dataset, batch_size, order="length")`` -> ``ModalityResult``.

    Per batch: eight ``mmda_collate_gather_masked`` launches (keep sets 0 .. 7) into one set of buffers, eight evaluation forwards
    (dropout off whatever ``model.training`` says, no stash) and eight ``mmda_misa_infer_collect`` launches that write row i = sample i
    of slice k of the ``(8, n, C)`` / ``(8, n, 6)`` tables.  No read-back, no synchronisation but the cluster check at the end.  ONE
    SEED IS DRAWN PER FORWARD, eight per batch: the seed counter advances as eight ``model(...)`` calls per batch would advance it, so
    training that goes on after a pass is bit-identical to training after as many evaluation forwards (as for ``InferencePass``).
    Under ``task="sentiment"`` the pass works on the one score column and ``tcp`` is refused."""

    def __init__(self, model, values=VALUES):
        from . import _lib, step_rules
        values = (values,) if isinstance(values, str) else tuple(values)
        bad = [x for x in values if x not in VALUES]
        if bad or not values:
            raise ValueError(f"values {values!r}: name at least one of {VALUES}")
        self.model = model
        self.values = tuple(x for x in VALUES if x in values)
        self.task = getattr(model, "task", "emotion")
        if self.task == "sentiment" and "tcp" in self.values:
            raise _lib.MMDAError("ModalityPass(values='tcp'): " + dict(step_rules.SENTI_RULES)["senti_confid"])

    def _result(self, scores, tcp, lengths, segments, truth):
        return ModalityResult(scores, tcp, lengths, segments, truth, float(self.model.config.threshold), self.task)

    def run(self, dataset, batch_size, order="length"):
        import torch
        from . import _lib, ops
        from .inference import _pass_device, dataset_pass, inference_plan
        plan, bounds = inference_plan(dataset.lengths, batch_size, order)
        dev = _pass_device(self.model, dataset, "ModalityPass")
        m, n, nc = self.model, len(dataset), int(self.model.config.num_classes)
        scores = torch.empty(8, n, nc, device=dev) if "scores" in self.values else None
        tcp = torch.empty(8, n, 6, device=dev) if "tcp" in self.values else None
        outs = []
        for k in range(8):
            o = _lib.InferOut()
            o.scores = None if scores is None else scores[k].data_ptr()
            o.tcp = None if tcp is None else tcp[k].data_ptr()
            outs.append(o)
        dataset_pass(m, dataset, plan, bounds, batch_size, dev, lambda dst_ptr, k: ops.misa_infer_collect(m, outs[k], dst_ptr, 0),
                     keeps=range(8))
        m.check_cluster("modalities")
        truth = dataset.sentiment.reshape(n, 1) if self.task == "sentiment" else dataset.emo
        return self._result(scores, tcp, torch.from_numpy(np.array(dataset.lengths, dtype=np.int64)),
                            np.array(dataset.segments, dtype=object), truth)

    def run_loader(self, loader):
        """The same tables from any loader of the reference's 10-tuples: eight ``InferencePass.run_loader(loader, keep=k)`` passes, each
        batch masked by one ``mmda_modality_mask`` launch in front of the forward.  Slower than ``run`` -- the loader is walked eight
        times and every batch is copied once more -- but the tables are the same; rows come in the order the loader yields samples,
        so the loader must yield the same samples in the same order every time."""
        import torch
        from .inference import InferencePass
        p = InferencePass(self.model, self.values)
        res = [p.run_loader(loader, keep=k) for k in range(8)]
        if len({r.n for r in res}) != 1 or any(list(r.segments) != list(res[0].segments) for r in res[1:]):
            from . import _lib
            raise _lib.MMDAError("ModalityPass.run_loader: the loader did not yield the same samples in the same order eight times")
        stack = lambda f: torch.stack([getattr(r, f) for r in res]) if f in self.values else None
        col = 3 if self.task == "sentiment" else 4
        lab = [b[col] for b in loader]
        truth = None
        if lab and all(x is not None for x in lab):
            dev = res[0]._flat.device
            truth = torch.cat([torch.as_tensor(x).to(dev).float().reshape(len(x), -1) for x in lab])
        return self._result(stack("scores"), stack("tcp"), res[0].lengths, res[0].segments, truth)


def format_table(metrics, tcp, phi, classes=None):
    """One table: per keep set acc / F1 / mean tcp, then per class the mean Shapley value of each modality.  ``metrics``: the list of
    ``ModalityResult.metrics`` (or None); ``tcp``: eight means or None; ``phi``: (3, C) means."""
    lines = [f"{'keep':<24}{'acc':>8}{'f1':>8}{'tcp':>8}"]
    for k in range(8):
        name = "+".join(keep_names(k)) or "(none)"
        acc = f"{metrics[k]['acc']:8.4f}" if metrics else f"{'-':>8}"
        f1 = f"{metrics[k]['f1']:8.4f}" if metrics else f"{'-':>8}"
        q = f"{tcp[k]:8.4f}" if tcp is not None else f"{'-':>8}"
        lines.append(f"{k} {name:<22}{acc}{f1}{q}")
    C = phi.shape[1]
    classes = classes or [f"class{c}" for c in range(C)]
    lines.append(f"{'mean phi':<24}" + "".join(f"{m:>10}" for m in MODALITIES))
    for c in range(C):
        lines.append(f"{classes[c]:<24}" + "".join(f"{phi[m, c]:10.4f}" for m in range(3)))
    return "\n".join(lines)
