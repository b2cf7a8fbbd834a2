"""The sentiment table on the device: the figures of the reference's ``eval_mosei_senti``
(``src/utils/eval_metrics.py``) -- MAE, Pearson correlation, Acc-7, Acc-5, Acc-2 and weighted F1 with and without the zero-labelled
rows, MAE over the extreme rows -- from one device state that a launch per batch adds to (``mmda_senti_accumulate``), turned into the
figures on the device (``mmda_senti_finish``).  Nothing is read back until the caller asks (``as_dict``, ``counts``).

    ev = SentimentEval(device)
    for scores, y in batches: ev.update(scores, y)      # any device tensors of equal size: an InferenceResult's scores, for one
    ev.as_dict()                                        # the reference's keys (+ 'f1_non0', which it prints and does not return)

The integer part of the state does not depend on how the rows are split into batches; the float64 sums are added in a fixed order, so
the same batches give the same bits on every run.  NaN where numpy gives NaN (``corr`` of a constant column or a single row,
``mae_intensity`` without a row of ``|truth| > 2``); without a row of ``truth != 0`` the reference itself fails, and the two ``non0``
figures are NaN here.
"""
from __future__ import annotations

import torch

from . import _lib

# mmda_senti_finish's order
FIGURES = ("mae", "corr", "acc7", "acc5", "acc2", "f1", "acc2_non0", "f1_non0", "mae_intensity")
# the integer words of the state, in order ("has0": the (truth >= 0, pred >= 0) table over all rows, "non0": (truth > 0, pred > 0) over the
# rows with truth != 0; a table is [tn, fp, fn, tp] = index 2 * truth bit + pred bit), and the float64 words from F0 on
COUNTS = ("n", "n_nonzero", "acc7_hits", "acc5_hits", "has0_tn", "has0_fp", "has0_fn", "has0_tp", "non0_tn", "non0_fp", "non0_fn", "non0_tp",
          "n_extreme")
SUMS = ("abs_err", "abs_err_extreme", "p", "t", "pp", "tt", "pt")
F0 = 16
# eval_mosei_senti's returned keys ('mult' is Acc-7 again)
REFERENCE_KEYS = ("mae", "corr", "mult", "f1", "acc2", "acc2_non0", "acc7", "acc5", "mae_intensity")


class SentimentEval:
    """Accumulates the state over the batches of an evaluation pass; no synchronisation until a result is read."""

    def __init__(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.MMDAError(f"SentimentEval counts on the GPU (device={device}): the HIP path has no CPU fallback")
        self.state = torch.zeros(_lib.SENTI_STATE_WORDS, dtype=torch.int64, device=device)
        self.loss_sum = torch.zeros(1, dtype=torch.float32, device=device)
        self.batches = 0
        self._lib = _lib.load()

    def update(self, pred: torch.Tensor, truth: torch.Tensor):
        """``pred``, ``truth``: device tensors of N elements each ((N,) or (N, 1)); one launch on the current stream."""
        if not (pred.is_cuda and truth.is_cuda):
            raise _lib.MMDAError("SentimentEval.update needs device tensors (the HIP path has no CPU fallback)")
        p = pred.detach().to(torch.float32).contiguous().reshape(-1)
        t = truth.detach().to(torch.float32).contiguous().reshape(-1)
        if p.numel() != t.numel():
            raise ValueError(f"SentimentEval.update: {p.numel()} predictions, {t.numel()} truths")
        _lib.check(self._lib.mmda_senti_accumulate(p.data_ptr(), t.data_ptr(), p.numel(), self.state.data_ptr(), _lib.stream_ptr()),
                   "mmda_senti_accumulate")
        return self

    def add_loss(self, pred: torch.Tensor, truth: torch.Tensor, senti_loss: str):
        """adds this batch's criterion (``senti_loss``: 'l1' or 'mse', the mean over the batch's rows) to the running sum, on the
        device: ``DeviceEval.add_cls_loss`` for the sentiment task.  ``pred``, ``truth``: as ``update`` takes them."""
        p = pred.detach().to(torch.float32).contiguous().reshape(-1)
        t = truth.detach().to(torch.float32).contiguous().reshape(-1)
        if not (p.is_cuda and t.is_cuda) or p.numel() != t.numel():
            raise _lib.MMDAError("SentimentEval.add_loss needs device tensors of equal size (the HIP path has no CPU fallback)")
        _lib.check(self._lib.mmda_loss_reg(p.data_ptr(), t.data_ptr(), p.numel(), 1, _lib.SENTI_LOSS[senti_loss], 1.0,
                                           self.loss_sum.data_ptr(), None, _lib.stream_ptr()), "mmda_loss_reg")
        self.batches += 1

    def mean_loss(self) -> float:
        """the mean of the batches' losses: one read-back"""
        return float(self.loss_sum.item()) / max(self.batches, 1)

    def figures(self) -> torch.Tensor:
        """(9,) float64 on the device, in the order of ``FIGURES``: one launch, nothing read back."""
        out = torch.empty(_lib.SENTI_FIGURES, dtype=torch.float64, device=self.state.device)
        _lib.check(self._lib.mmda_senti_finish(self.state.data_ptr(), out.data_ptr(), _lib.stream_ptr()), "mmda_senti_finish")
        return out

    def counts(self) -> dict:
        """The state read back: the integer counts and the float64 sums by name."""
        st = self.state.cpu()
        out = {k: int(st[i]) for i, k in enumerate(COUNTS)}
        out.update({k: float(x) for k, x in zip(SUMS, st[F0:F0 + len(SUMS)].view(torch.float64).tolist())})
        return out

    def as_dict(self) -> dict:
        """The figures read back under the reference's keys, and 'f1_non0'."""
        f = dict(zip(FIGURES, self.figures().tolist()))
        f["mult"] = f["acc7"]
        return f


def sentiment_metrics(pred: torch.Tensor, truth: torch.Tensor) -> SentimentEval:
    """The table of one set of predictions: a ``SentimentEval`` that has seen them (``.as_dict()`` reads the figures back)."""
    return SentimentEval(pred.device).update(pred, truth)


def format_table(f: dict, n: int = None, n_non0: int = None) -> str:
    """The lines eval_mosei_senti prints, from ``as_dict()``."""
    over = "" if n is None else f" over {n}/{n_non0}"
    return "\n".join(["-" * 50, f"MAE:  {f['mae']}", f"Correlation Coefficient:  {f['corr']}", f"mult_acc_7:  {f['acc7']}",
                      f"mult_acc_5:  {f['acc5']}", f"F1 score all/non0: {round(f['f1'], 4)}/{round(f['f1_non0'], 4)}{over}",
                      f"Accuracy all/non0: {round(f['acc2'], 4)}/{round(f['acc2_non0'], 4)}",
                      f"Extreme Intensity MAE:  {f['mae_intensity']}", "-" * 50])
