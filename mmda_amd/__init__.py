"""mmda_amd - MI355X-native (gfx950) hot path of SoyeonHH/MMDA's MISA training step.

Public surface mirrors the reference's modules: ``models.MISA`` (alias ``Model``), ``solver.Solver``,
``config.get_config``, ``utils.{DiffLoss, CMD, ReverseLayerF, getBinaryTensor, to_gpu, to_cpu}``; the input side is in ``data``
(``collate_fn``, ``DevicePrefetcher``; the device-resident ``DeviceDataset`` / ``DeviceLoader`` and their host core ``batch_plan`` are
exported here too), the output side in ``inference`` (``InferencePass``: per-sample scores, confidence and hidden vectors kept on the
device) and ``utils.tools`` (their files); ``encoded`` holds the encoder cache (``EncoderCache``, ``EncodedLoader``: training the
fusion block and the heads of a model with frozen encoders from stored encoder outputs); ``calibrate`` sweeps the decision cut-off
(``ThresholdSweep``, ``Thresholds``: every candidate threshold counted on the device in one launch per batch); ``ranking`` measures
how a score table ranks before any cut-off (``ranking_metrics``: exact per-class AUROC / AP and the label-ranking figures;
``failure_prediction``: the same over ConfidNet's ``tcp``); ``sentiment`` holds the table of the second task (``config.task =
"sentiment"``): ``sentiment_metrics`` / ``SentimentEval``, the figures of the reference's ``eval_mosei_senti`` from one device state;
``modality`` masks inputs (``DeviceLoader(modality_dropout=..., keep=...)``, ``keep_bits``: the random keep sets restated in numpy) and
attributes a value to the three modalities (``ModalityPass`` / ``ModalityResult``: the split under all eight keep sets, exact Shapley
values from one launch); ``reliability`` asks whether the scores are probabilities (``reliability_metrics`` / ``ReliabilityEval``: the
reliability diagram, ECE, MCE, Brier score and NLL per class from one integer state a launch per batch adds to) and fits the monotone
rescaling that makes them so (``fit_scaling`` -> ``Scaling``: temperature or Platt scaling of the logits, per class or shared, by a
damped Newton iteration whose state never leaves the device; ``config.scaling``); ``uncertainty`` gives ``tcp`` its baselines
(``MCDropoutPass`` / ``MCDropoutResult``: K dropout draws per sample from ONE forward of the fusion block over rows repeated K times,
reduced on the device to mean, variance, entropy and mutual information; ``mc_statistics``: that reduction over any table;
``config.mc_passes``); ``bootstrap`` says how far any of those figures would move on another draw of the split (``Bootstrap``: the rows
resampled R times on the device by a counter-based generator, percentile intervals per figure and paired comparisons over the same
resamples; ``resample_indices``: the draws restated in numpy; ``config.bootstrap``); ``neighbours`` searches one device table for the
nearest rows of another, exactly (``knn_search``, ``NeighbourIndex``: a distance GEMM on the f32-input MFMA whose matrix is never
written) and builds ``tcp``'s third baseline on it (``TrustIndex`` / ``TrustResult``: the Trust Score, the distance to the nearest
training example of the other label over that to the nearest of the decided one; ``config.trust_k``).
"""
from . import _lib  # noqa: F401
from .models import MISA, Model  # noqa: F401
from .config import Config, get_config, make_config  # noqa: F401
from .data import DeviceDataset, DeviceLoader, batch_plan, class_pos_weight  # noqa: F401
from .inference import FIELDS, InferencePass, InferenceResult, inference_plan  # noqa: F401
from .encoded import EncodedBatch, EncodedLoader, EncoderCache  # noqa: F401
from .calibrate import ThresholdSweep, Thresholds, confidence_curve, default_grid  # noqa: F401
from .ranking import RankingResult, failure_prediction, rank_plan, ranking_metrics  # noqa: F401
from .sentiment import SentimentEval, sentiment_metrics  # noqa: F401
from .modality import MODALITIES, ModalityPass, ModalityResult, keep_bits, parse_keep  # noqa: F401
from .reliability import ReliabilityEval, ReliabilityResult, Scaling, fit_scaling, reliability_metrics  # noqa: F401
from .uncertainty import MCDropoutPass, MCDropoutResult, mc_statistics  # noqa: F401
from .bootstrap import Bootstrap, BootstrapResult, BootstrapSummary, boot_plan, resample_indices  # noqa: F401
from .neighbours import NeighbourIndex, TrustIndex, TrustResult, knn_search  # noqa: F401
