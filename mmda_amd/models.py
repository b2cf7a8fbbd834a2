"""MISA model with the reference's call surface, computed by hand-written HIP kernels (gfx950).

Mirrors reference ``src/models.py:15-285``: same constructor (``MISA(config)``), same ``forward`` signature and return
value, same post-forward side-channel attributes the solver reads (``utt_shared_*``, ``utt_private_*``,
``utt_*_orig``, ``utt_*_recon``, ``domain_label_*``, ``tcp``), same ``state_dict`` keys.  ``Model`` is an alias
(BASELINE.json's north star names it so).

What is different by design: there are no ``nn.LSTM``/``nn.Linear`` submodules.  Every parameter is a view into ONE
flat fp32 device bucket (gradients and Adam moments likewise), the layout of which is defined by the native runtime
(``mmda_misa_param_info``); all arithmetic happens in ``libmmda_hip.so`` through the C ABI in ``include/mmda_hip.h``.
PyTorch only owns the memory and the autograd tape entry.  There is no CPU fallback: forward on a CPU tensor raises.
"""
from __future__ import annotations

import ctypes as C
import math
import operator
import os
from typing import Dict, List, Tuple

import torch
import torch.nn as nn

from . import _lib, step_rules
from . import optim as _optim
from .config import activation_name

FFN_DIM = 2048          # torch default dim_feedforward of nn.TransformerEncoderLayer (reference models.py:160)
FUSION_DROPOUT = 0.1    # torch default dropout of nn.TransformerEncoderLayer (not a reference flag)

_TOP_ORDER = ["activation", "embed", "trnn1", "trnn2", "vrnn1", "vrnn2", "arnn1", "arnn2", "project_t", "project_v", "project_a",
              "private_t", "private_v", "private_a", "shared", "recon_t", "recon_v", "recon_a", "discriminator",
              "sp_discriminator", "confidence", "classifier", "tlayer_norm", "vlayer_norm", "alayer_norm",
              "transformer_encoder"]
_RNN_ORDER = ["weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0", "weight_ih_l0_reverse", "weight_hh_l0_reverse",
              "bias_ih_l0_reverse", "bias_hh_l0_reverse"]

# outputs of the autograd entry, in order (labels last, non-differentiable)
_PUB = ["scores", "tcp", "utt_t_orig", "utt_v_orig", "utt_a_orig", "utt_private_t", "utt_private_v", "utt_private_a",
        "utt_shared_t", "utt_shared_v", "utt_shared_a", "utt_t_recon", "utt_v_recon", "utt_a_recon",
        "domain_label_t", "domain_label_v", "domain_label_a"]


_SIG_CACHE: Dict[int, bool] = {}
_REQUIRES_GRAD = operator.attrgetter("requires_grad")


# Adam as the native step runs it until told otherwise: (beta1, beta2, eps, weight_decay, decoupled, clip_norm)
_ADAM_DEFAULTS = (0.9, 0.999, 1e-8, 0.0, False, 0.0)


def _takes_model(fn) -> bool:
    """True if ``fn`` accepts a third positional argument (the model)."""
    import inspect
    key = id(getattr(fn, "__func__", fn))
    if key not in _SIG_CACHE:
        try:
            ps = list(inspect.signature(fn).parameters.values())
            npos = sum(p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD) for p in ps)
            _SIG_CACHE[key] = npos >= 3 or any(p.kind == p.VAR_POSITIONAL for p in ps)
        except (TypeError, ValueError):
            _SIG_CACHE[key] = True
    return _SIG_CACHE[key]


class _Bag(nn.Module):
    """Parameter container; exists only to reproduce the reference's dotted state_dict names."""


def _reference_sort_key(name: str):
    top = name.split(".")[0]
    rest = name[len(top) + 1:]
    sub = _RNN_ORDER.index(rest) if rest in _RNN_ORDER else 0
    return (_TOP_ORDER.index(top), sub)


# mmda_misa_set_embed_update ('deferred' is dense plus mmda_misa_set_embed_deferred: the same weights, no pass over the table per step)
EMBED_UPDATE = {"dense": 0, "sparse": 1, "frozen": 2, "deferred": 0}


class MISA(nn.Module):
    """MISA for CMU-MOSEI emotion multi-label classification (reference models.py:15-17), HIP-backed."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.text_size = config.embedding_size
        self.visual_size = config.visual_size
        self.acoustic_size = config.acoustic_size
        self.input_sizes = [self.text_size, self.visual_size, self.acoustic_size]
        self.hidden_sizes = [int(self.text_size), int(self.visual_size), int(self.acoustic_size)]
        self.output_size = config.num_classes
        self.dropout_rate = config.dropout
        if getattr(config, "extractor", "lstm") == "transformer":
            # the reference prints a TODO and calls exit() here (models.py:33-36)
            raise NotImplementedError("extractor='transformer' is a TODO in the reference as well")
        # reference models.py:39: nn.LSTM if config.rnncell == 'lstm' else nn.GRU
        self.rnncell = "lstm" if getattr(config, "rnncell", "lstm") == "lstm" else "gru"
        if getattr(config, "use_bert", False):
            raise NotImplementedError("use_bert=True needs a hub download; the GloVe/LSTM text branch is the hot path")
        self.activation_name = activation_name(config.activation)
        self.precision = getattr(config, "precision", "bf16")
        if self.precision not in ("bf16", "fp32"):
            raise ValueError("config.precision must be 'bf16' or 'fp32'")

        self.embed_update = getattr(config, "embed_update", "dense")
        if not isinstance(self.embed_update, str) or self.embed_update not in EMBED_UPDATE:
            raise ValueError("config.embed_update must be 'dense', 'sparse', 'frozen' or 'deferred'")
        # deferred: updates between full flushes (MMDA_EMBED_WINDOW overrides the configuration); read by that mode only
        self.embed_window = 0
        if self.embed_update == "deferred":
            self.embed_window = int(os.environ.get("MMDA_EMBED_WINDOW", 0) or getattr(config, "embed_deferred_window", 256))
            if self.embed_window < 1:
                raise ValueError("config.embed_deferred_window must be at least 1")

        # optimizer steps from this many micro-batches each (Solver.train_epoch groups the loader's batches; train_step takes the position)
        self.accum_steps = getattr(config, "accum_steps", 1)
        if isinstance(self.accum_steps, bool) or not isinstance(self.accum_steps, int) or self.accum_steps < 1:
            raise ValueError("config.accum_steps must be an int >= 1")

        # what the sentiment task refuses (step_rules.SENTI_RULES), by name and before the native model exists
        step_rules.task_check(getattr(config, "task", "emotion"), getattr(config, "senti_loss", "l1"), num_classes=self.output_size,
                              use_confidNet=bool(getattr(config, "use_confidNet", False)), pos_weight=getattr(config, "pos_weight", None),
                              focal_gamma=getattr(config, "focal_gamma", 0.0))

        lib = _lib.load()
        cc = _lib.MisaConfig(
            vocab=len(config.word2id), d_t=self.text_size, d_v=self.visual_size, d_a=self.acoustic_size,
            hidden=config.hidden_size, ncls=config.num_classes, act=_lib.ACT[self.activation_name],
            use_cmd_sim=int(bool(config.use_cmd_sim)), use_confidNet=int(bool(getattr(config, "use_confidNet", False))),
            dropout=float(config.dropout), fusion_dropout=FUSION_DROPOUT, threshold=float(config.threshold),
            reverse_grad_weight=float(getattr(config, "reverse_grad_weight", 1.0)),
            diff_weight=float(getattr(config, "diff_weight", 0.3)), sim_weight=float(getattr(config, "sim_weight", 0.7)),
            recon_weight=float(getattr(config, "recon_weight", 0.7)), conf_weight=float(getattr(config, "conf_weight", 0.3)),
            mode=_lib.BF16 if self.precision == "bf16" else _lib.F32, rnncell=_lib.CELL[self.rnncell])
        h = C.c_void_p()
        _lib.check(lib.mmda_misa_create(C.byref(cc), C.byref(h)), "mmda_misa_create")
        self._h = h
        self._lib = lib
        # BASELINE configs[4]: the fusion layer's feed-forward products on block-scaled fp8 (forward only; off by default)
        self.fusion_fp8 = bool(getattr(config, "fusion_fp8", False))
        if self.fusion_fp8:
            _lib.check(lib.mmda_misa_set_fusion_fp8(h, 1), "set_fusion_fp8")
        _lib.check(lib.mmda_misa_set_embed_update(h, EMBED_UPDATE[self.embed_update]), "set_embed_update")
        # the classification criterion (config.pos_weight, config.focal_gamma).  "balanced" needs the training set's
        # labels: Solver.build() resolves it and calls set_cls_loss; until then the weights are off
        pw = getattr(config, "pos_weight", None)
        if isinstance(pw, str) and pw != "balanced":
            raise ValueError("config.pos_weight must be None, a list of num_classes floats or 'balanced'")
        self.task, self.senti_loss = "emotion", "l1"
        self.set_cls_loss(None if isinstance(pw, str) else pw, getattr(config, "focal_gamma", 0.0))
        # the task (config.task, config.senti_loss): under "sentiment" the one output column is the regression output
        self.set_task(getattr(config, "task", "emotion"), getattr(config, "senti_loss", "l1"))
        self._layout: Dict[str, Tuple[int, Tuple[int, ...]]] = {}
        self._native_names: List[str] = []                  # mmda_misa_param_info order = ascending bucket offset
        for i in range(lib.mmda_misa_num_params(h)):
            name, off, rows, cols = C.c_char_p(), C.c_int64(), C.c_int(), C.c_int()
            _lib.check(lib.mmda_misa_param_info(h, i, C.byref(name), C.byref(off), C.byref(rows), C.byref(cols)))
            shape = (rows.value, cols.value) if cols.value > 0 else (rows.value,)
            self._layout[name.value.decode()] = (off.value, shape)
            self._native_names.append(name.value.decode())
        self._flat_floats = lib.mmda_misa_flat_floats(h)
        self._dense_floats = lib.mmda_misa_dense_floats(h)
        self._names: List[str] = sorted(self._layout, key=_reference_sort_key)
        # config.activation = prelu: the reference instantiates ONE nn.PReLU() (models.py:30) and adds that module to the three
        # projections and to the discriminator, so its slope shows up in state_dict() under every one of those names: aliases of the
        # single native parameter "activation.weight", registered as the same nn.Parameter
        self._aliases: Dict[str, str] = {}
        if "activation.weight" in self._layout:
            after = {f"project_{m_}.project_{m_}.bias": f"project_{m_}.project_{m_}_activation.weight" for m_ in "tva"}
            after["discriminator.discriminator_layer_1.bias"] = "discriminator.discriminator_layer_1_activation.weight"
            names = []
            for n_ in self._names:
                names.append(n_)
                if n_ in after:
                    names.append(after[n_])
                    self._aliases[after[n_]] = "activation.weight"
            self._names = names
        for name in self._names:
            if name in self._aliases:
                self._layout[name] = self._layout[self._aliases[name]]
                self._register(name, None, shared=self._get(self._aliases[name]))
            else:
                self._register(name, self._layout[name][1])
        self._plist = [(n, self._get(n)) for n in self._names]
        self.reset_parameters()
        if self.embed_update == "frozen":
            # what the reference's `self.model.embed.requires_grad = False` (solver.py:86) meant: the optimizer's
            # filter(lambda p: p.requires_grad, ...) then leaves the table out
            self.embed.weight.requires_grad_(False)
        # frozen parameters: the requires_grad flags (native order) the native side was last told -- it starts with every flag set --, how
        # often it was told, and the device table of trainable runs the unfused optimizers step through (made when first needed)
        self._native_params = [self._get(n) for n in self._native_names]
        self._embed_index = self._native_names.index("embed.weight")
        self._trainable_sent = (True,) * len(self._native_names)
        self._trainable_sends = 0
        self._runs_cache = None
        self._cut_flags = None                              # the flags under which the native side last reported the encoder cut on
        self._rules_passed = None                           # the last case step_rules let pass (MISA._rules)
        self._adam_pushed = _ADAM_DEFAULTS                  # (beta1, beta2, eps, weight_decay, decoupled, clip_norm) the native side holds
        # deferred mode: per-row step counts and the ring of step scalars (device, made with the flat buckets), and whether a step has
        # been taken since the last flush
        self._df_row_step = self._df_ring = None
        self._df_dirty = False
        # sparse / deferred mode: a backward whose rows update is still to be applied (the next optimizer step consumes it), and the clip value
        # optim.clip_grad_value_ recorded for it (the clamp applies to the coalesced rows, which exist only inside that update)
        self._rows_pending = False
        self._rows_clip = None
        self._rows_keep = None

        # accumulated steps (train_step(accum_count > 1)): the second gradient bucket and, in sparse mode, the (ids, rows) list of the
        # step's micro-batches -- host-owned, outside the workspace (which is re-carved when a micro-batch changes T or B), made on
        # first use, grown when a micro-batch needs more, kept across steps; the position the next call must have, and the step's count
        self._acc = None
        self._acc_list = None
        self._acc_used = 0
        self._acc_next = 0
        self._acc_count = 1

        # device state (created lazily on the first forward / .to())
        self._P = self._G = self._M = self._V = None
        self._ws = None
        self._ws_shape = None
        self._len_dev = None
        self._len_cache = None
        self._fwd_id = 0
        self._step = 0
        self._seed = 0x5EED
        self._anchor = None
        self._last = {}
        self._abort_seen = False
        self._seg_work = None

    # ------------------------------------------------------------------ parameters
    def _register(self, dotted: str, shape, shared=None):
        mod = self
        parts = dotted.split(".")
        for p in parts[:-1]:
            if not hasattr(mod, p):
                mod.add_module(p, _Bag())
            mod = getattr(mod, p)
        mod.register_parameter(parts[-1], shared if shared is not None else nn.Parameter(torch.empty(shape, dtype=torch.float32)))

    def _get(self, dotted: str) -> nn.Parameter:
        mod = self
        for p in dotted.split("."):
            mod = getattr(mod, p)
        return mod

    @torch.no_grad()
    def reset_parameters(self):
        """Same distributions as the torch modules the reference instantiates (nn.LSTM, nn.Linear, nn.LayerNorm,
        nn.Embedding, nn.MultiheadAttention); the reference's solver then applies orthogonal_ to weight_hh*."""
        for name, p in self._plist:
            if name.endswith("activation.weight"):
                p.fill_(0.25)                               # nn.PReLU() default
            elif name == "embed.weight":
                p.normal_(0.0, 1.0)
            elif "rnn" in name.split(".")[0]:
                h = self._layout[name.rsplit(".", 1)[0] + ".weight_hh_l0"][1][1]
                k = 1.0 / math.sqrt(h)
                p.uniform_(-k, k)
            elif "layer_norm" in name or ".norm1." in name or ".norm2." in name:
                p.fill_(1.0 if name.endswith("weight") else 0.0)
            elif name.endswith("in_proj_weight"):
                nn.init.xavier_uniform_(p)
            elif name.endswith("in_proj_bias") or name.endswith("out_proj.bias"):
                p.zero_()
            elif name.endswith("weight"):
                k = 1.0 / math.sqrt(p.shape[1])
                p.uniform_(-k, k)
            else:   # Linear bias: U(-1/sqrt(fan_in), 1/sqrt(fan_in))
                w = self._get(name[:-4] + "weight")
                k = 1.0 / math.sqrt(w.shape[1])
                p.uniform_(-k, k)

    def _apply(self, fn, *args, **kwargs):
        self.flush_embedding()   # (deferred: the copies made below must hold current rows)
        out = super()._apply(fn, *args, **kwargs)
        self._P = None           # parameter storages were replaced: re-flatten lazily
        return out

    def _views_valid(self) -> bool:
        if self._P is None:
            return False
        base = self._P.data_ptr()
        for name, p in self._plist:
            if p.data_ptr() != base + 4 * self._layout[name][0]:
                return False
        return True

    @torch.no_grad()
    def _materialize(self, device):
        """(Re)build the flat device buckets and point every Parameter at its slice."""
        if device.type != "cuda":
            raise _lib.MMDAError("mmda_amd.MISA runs on an MI355X only (no CPU fallback); move the model with .to('cuda')")
        P = torch.zeros(self._flat_floats, dtype=torch.float32, device=device)
        for name, p in self._plist:
            off, shape = self._layout[name]
            n = p.numel()
            P[off:off + n].copy_(p.data.reshape(-1))
            p.data = P[off:off + n].view(shape)
        self._P = P
        if self._G is None or self._G.device != device:
            self._G = torch.zeros_like(P)
            self._M = torch.zeros_like(P)
            self._V = torch.zeros_like(P)
        for name, p in self._plist:
            off, shape = self._layout[name]
            p.grad = None
        _lib.check(self._lib.mmda_misa_bind(self._h, P.data_ptr(), self._G.data_ptr(), self._M.data_ptr(), self._V.data_ptr()),
                   "mmda_misa_bind")
        self._ws_shape = None
        if self.embed_update == "deferred":
            self._bind_deferred()

    def _bind_deferred(self):
        """(Re)bind the deferred state with every row current (the table holds flushed rows: new, loaded, or flushed by the caller);
        the native side counts the updates from here."""
        V = self._layout["embed.weight"][1][0]
        dev = self._P.device
        if self._df_row_step is None or self._df_row_step.device != dev:
            self._df_row_step = torch.zeros(V, dtype=torch.int32, device=dev)
            self._df_ring = torch.zeros(int(self._lib.mmda_embed_deferred_scalar_floats(self.embed_window)), dtype=torch.float32, device=dev)
        _lib.check(self._lib.mmda_misa_set_embed_deferred(self._h, self._df_row_step.data_ptr(), self._df_ring.data_ptr(), self.embed_window,
                                                          _lib.stream_ptr()), "set_embed_deferred")
        self._df_dirty = False

    def flush_embedding(self):
        """embed_update='deferred': every row of embed.weight (and of its Adam moments) takes the optimizer steps it has not taken yet.
        Required before embed.weight is read directly (p.data, flat_buckets()); state_dict(), checkpointing, .to() and load_state_dict()
        call it themselves.  With no step since the last flush, and in every other mode, nothing is launched."""
        if self.embed_update != "deferred" or not self._df_dirty or self._P is None or not self._views_valid():
            return
        _lib.check(self._lib.mmda_misa_embed_flush(self._h, _lib.stream_ptr()), "embed_flush")
        self._df_dirty = False

    def state_dict(self, *args, **kwargs):
        self.flush_embedding()
        return super().state_dict(*args, **kwargs)

    def load_state_dict(self, state_dict, *args, **kwargs):
        # deferred: the moments of stale rows catch up before the table under them changes; the loaded rows are current at this step
        self.flush_embedding()
        out = super().load_state_dict(state_dict, *args, **kwargs)
        if self.embed_update == "deferred" and self._P is not None and self._views_valid():
            self._bind_deferred()
        return out

    def set_embed_update(self, mode: str):
        """Switch how embed.weight trains (config.embed_update) between steps; a deferred table is flushed first."""
        if not isinstance(mode, str) or mode not in EMBED_UPDATE:
            raise ValueError("embed_update must be 'dense', 'sparse', 'frozen' or 'deferred'")
        self.flush_embedding()
        bound = self._P is not None and self._views_valid()
        if self.embed_update == "deferred":
            _lib.check(self._lib.mmda_misa_set_embed_deferred(self._h, None, None, 0, _lib.stream_ptr()), "set_embed_deferred")
        _lib.check(self._lib.mmda_misa_set_embed_update(self._h, EMBED_UPDATE[mode]), "set_embed_update")
        self.embed_update = mode
        if mode == "deferred" and self.embed_window < 1:
            self.embed_window = int(os.environ.get("MMDA_EMBED_WINDOW", 0) or getattr(self.config, "embed_deferred_window", 256))
        self._rows_pending = False
        self._rows_clip = None
        self._cut_flags = None
        self.embed.weight.requires_grad_(mode != "frozen")
        if mode != "dense":
            self.embed.weight.grad = None
        if mode == "deferred" and bound:
            self._bind_deferred()

    def set_cls_loss(self, pos_weight=None, focal_gamma: float = 0.0):
        """The classification criterion of every step and loss of this model from now on: ``pos_weight`` -- None or one
        weight >= 0 per class on the positive term -- and the focal exponent ``focal_gamma`` (0, or 1 .. 8).  What is refused is raised
        by name (step_rules.CLS_RULES) with nothing changed.  ``self.cls_loss`` reports the setting in force; weights that are all 1
        count as none, so with ``focal_gamma = 0`` the step is the default one."""
        w, g = step_rules.cls_setting(pos_weight, focal_gamma, self.output_size)
        step_rules.task_check(self.task, self.senti_loss, num_classes=self.output_size, pos_weight=w, focal_gamma=g)
        _lib.check(self._lib.mmda_misa_set_cls_loss(self._h, _lib.cls_opts(w, g)), "mmda_misa_set_cls_loss")
        self.cls_loss = dict(pos_weight=w, focal_gamma=g)
        return self.cls_loss

    def set_task(self, task: str = "emotion", senti_loss: str = "l1"):
        """Which target the head is trained on, from the next step on.  ``"emotion"``: the classifier.  ``"sentiment"``:
        the model's one score column (``num_classes == 1``) is a regression output -- no sigmoid in ``forward``, ``scores`` are the raw
        outputs, ``labels = scores > threshold`` as ever -- and the loss every step calls ``cls`` is the batch mean of ``|s - y|``
        (``senti_loss="l1"``) or ``(s - y)^2`` (``"mse"``) against the ``(B,)`` or ``(B, 1)`` sentiment column given where the emotion
        labels were.  What is refused is raised by name (step_rules.SENTI_RULES) with nothing changed."""
        step_rules.task_check(task, senti_loss, num_classes=self.output_size,
                              use_confidNet=bool(getattr(self.config, "use_confidNet", False)),
                              pos_weight=self.cls_loss["pos_weight"], focal_gamma=self.cls_loss["focal_gamma"])
        _lib.check(self._lib.mmda_misa_set_task(self._h, _lib.TASK[task], _lib.SENTI_LOSS[senti_loss if task == "sentiment" else "l1"]),
                   "mmda_misa_set_task")
        self.task, self.senti_loss = task, (senti_loss if task == "sentiment" else self.senti_loss)
        return self.task

    # ------------------------------------------------------------------ frozen parameters
    def _match(self, prefixes) -> List[str]:
        names = []
        for pre in prefixes:
            hit = [n for n in self._names if n.startswith(pre)]
            if not isinstance(pre, str) or not pre or not hit:
                raise ValueError(f"no parameter of the state dict begins with {pre!r}")
            names += [n for n in hit if n not in names]
        return [n for n in self._names if n in names]

    def freeze(self, *prefixes: str) -> List[str]:
        """requires_grad_(False) on every parameter whose state-dict name begins with one of ``prefixes`` (``"trnn1"``, ``"embed"``,
        ``"project_t.project_t.weight"``); returns those names.  Nothing else happens here: the flags are read when the next step begins,
        as PyTorch's are -- a frozen tensor and its optimizer state then keep their bits, its ``.grad`` is None, and when nothing behind
        the fusion block trains (all six recurrent layers, the three ``*layer_norm`` between them and the table) the backward pass
        stops in front of the encoders."""
        names = self._match(prefixes)
        for n in names:
            self._get(n).requires_grad_(False)
        return names

    def unfreeze(self, *prefixes: str) -> List[str]:
        """The opposite of freeze().  A table frozen by embed_update='frozen' is thawed by set_embed_update(), not here."""
        names = self._match(prefixes)
        if "embed.weight" in names and self.embed_update == "frozen":
            raise _lib.MMDAError("embed.weight is frozen by embed_update='frozen': switch the mode with set_embed_update('dense')")
        for n in names:
            self._get(n).requires_grad_(True)
        return names

    def _trainable_flags(self) -> Tuple[bool, ...]:
        # (read at every step: the Parameter objects are looked up once, they stay the same objects through .to() and _materialize)
        flags = tuple(map(_REQUIRES_GRAD, self._native_params))
        if self.embed_update == "frozen" and flags[self._embed_index]:
            flags = flags[:self._embed_index] + (False,) + flags[self._embed_index + 1:]
        return flags

    def frozen_names(self, beyond_embed_update: bool = False) -> List[str]:
        """State-dict names of the parameters with requires_grad = False (``beyond_embed_update``: the table that embed_update='frozen'
        froze is not listed)."""
        out = [n for n in self._names if not self._get(n).requires_grad]
        if beyond_embed_update and self.embed_update == "frozen":
            out = [n for n in out if n != "embed.weight"]
        return out

    def _sync_trainable(self, exchange: bool = False) -> Tuple[bool, ...]:
        """Read the requires_grad flags (a step begins) and tell the native side when they differ from what it was last told.
        ``exchange``: a gradient exchange is part of the step."""
        flags = self._trainable_flags()
        if flags == self._trainable_sent and not exchange and (flags[self._embed_index] or self.embed_update not in ("sparse", "deferred")):
            return flags                                    # (the steady state: one tuple compare)
        frozen = [n for n, f in zip(self._native_names, flags) if not f]
        if "embed.weight" in frozen and self.embed_update in ("sparse", "deferred"):
            raise _lib.MMDAError(f"embed.weight.requires_grad=False under embed_update='{self.embed_update}': freeze the table with "
                                 "set_embed_update(\"frozen\")")
        step_rules.check(frozen=any(not (n == "embed.weight" and self.embed_update == "frozen") for n in frozen), exchange=exchange)
        if flags != self._trainable_sent:
            _lib.check(self._lib.mmda_misa_set_trainable(self._h, bytes(bytearray(int(f) for f in flags)), len(flags)), "set_trainable")
            self._trainable_sent = flags
            self._trainable_sends += 1
        return flags

    def trainable_info(self):
        """(runs, trainable_floats, encoder_cut) as the native side holds them: runs = [(begin, length), ...] of the flat buckets, sorted,
        disjoint, a tensor's range taken up to the next tensor (alignment padding included)."""
        cap = len(self._native_names) + 1
        runs = (_lib.Run * cap)()
        n, floats, cut = C.c_int(), C.c_int64(), C.c_int()
        _lib.check(self._lib.mmda_misa_trainable_info(self._h, runs, cap, C.byref(n), C.byref(floats), C.byref(cut)), "trainable_info")
        return [(int(runs[i].begin), int(runs[i].len)) for i in range(n.value)], int(floats.value), bool(cut.value)

    def _trainable_runs(self):
        """None when every float of [0, grad_floats) trains; else (device table of mmda_run, runs, items) for the unfused optimizers'
        run-table launches over that range.  Reads the flags (optimizer.step() begins a step of its own)."""
        flags = self._sync_trainable()
        n_floats = self.grad_floats
        offs = [self._layout[n][0] for n in self._native_names] + [self._flat_floats]
        live = [(offs[i], offs[i + 1] - offs[i], f) for i, f in enumerate(flags) if offs[i] < n_floats]
        if all(f for _, _, f in live):
            return None
        key = (flags, n_floats, self._P.device)
        if self._runs_cache is None or self._runs_cache[0] != key:
            from . import ops
            self._runs_cache = (key,) + ops.runs_table([(b, l) for b, l, f in live if f], n_floats, self._P.device)      # (once per change)
        return self._runs_cache[1:]

    def set_frozen_forward(self, stash: bool):
        """A step under the encoder cut keeps no encoder stash in its forward pass (default); ``stash=True`` runs the stashing forward
        all the same (tools/bench_frozen.py measures both)."""
        _lib.check(self._lib.mmda_misa_set_cut_forward(self._h, int(bool(stash))), "set_cut_forward")

    def _assign_grad_views(self):
        for name, p in self._plist:
            if name == "embed.weight" and self.embed_update != "dense":
                continue                                    # no dense gradient exists: see embedding_grad_rows()
            if not p.requires_grad:
                p.grad = None                               # frozen: what its range of the bucket holds is unspecified
                continue
            if p.grad is None:
                off, shape = self._layout[name]
                p.grad = self._G[off:off + p.numel()].view(shape)

    def zero_grad(self, set_to_none: bool = False):
        """Zeroes the flat gradient bucket with one memset (the reference calls model.zero_grad() per batch,
        solver.py:139).  Gradients stay views of the bucket."""
        if self._G is not None and self._P is not None:
            _lib.check(self._lib.mmda_misa_zero_grad(self._h, _lib.stream_ptr()), "zero_grad")
        else:
            super().zero_grad(set_to_none=True)

    # ------------------------------------------------------------------ device plumbing
    def _prepare(self, sentences, video, acoustic, lengths):
        dev = sentences.device
        if dev.type != "cuda":
            raise _lib.MMDAError("inputs are on the CPU: mmda_amd.MISA has no CPU path (HIP kernels only)")
        if not self._views_valid():
            self._materialize(dev)
        T, B = sentences.shape
        if video.shape[0] != T or video.shape[1] != B or acoustic.shape[0] != T or acoustic.shape[1] != B:
            raise ValueError("sentences/video/acoustic must share (T, B)")
        if video.shape[2] != self.visual_size or acoustic.shape[2] != self.acoustic_size:
            raise ValueError("feature width does not match config.visual_size / acoustic_size")
        lens = torch.as_tensor(lengths)
        if lens.numel() != B:
            raise ValueError("lengths must have B entries")
        lmin, lmax = int(lens.min()), int(lens.max())
        if lmin <= 0:
            raise RuntimeError("Length of all samples has to be greater than 0")     # pack_padded_sequence's rule
        if lmax > T:
            raise RuntimeError("a length exceeds the padded sequence length")
        self._carve(B, T, dev)
        # lengths arrive on the CPU (reference: l = to_cpu(l), solver.py:149).  Convert on the host, stage through a pinned
        # buffer and copy asynchronously; an unchanged batch (benchmark loops) reuses the device copy.
        lens32 = lens.to(device="cpu", dtype=torch.int32)
        cached = self._len_cache
        if cached is not None and cached[0].shape == lens32.shape and torch.equal(cached[0], lens32) and cached[1].device == dev:
            len_dev = cached[1]
        else:
            pin = torch.empty(B, dtype=torch.int32, pin_memory=True)
            pin.copy_(lens32)
            len_dev = pin.to(device=dev, non_blocking=True)
            self._len_cache = (lens32.clone(), len_dev, pin)
        t = sentences.contiguous()
        if t.dtype != torch.int64:
            t = t.long()
        v = video.contiguous().float()
        a = acoustic.contiguous().float()
        return t, v, a, len_dev

    def _carve(self, B: int, T: int, dev):
        """The workspace laid out for (B, T) batches, grown when it has to be."""
        if self._ws_shape != (B, T):
            need = self._lib.mmda_misa_workspace_floats(self._h, B, T)
            if self._ws is None or self._ws.numel() < need or self._ws.device != dev:
                if self._ws is not None and self._ws_shape is not None:
                    # the old buffer's sticky abort words would be lost with it (the native side never touches a buffer it was
                    # not handed): look at them first.  Buffers only grow, so this synchronous read happens a few times per run.
                    self._abort_seen = self._abort_seen or self.cluster_aborted()
                self._ws = torch.zeros(need, dtype=torch.float32, device=dev)
            _lib.check(self._lib.mmda_misa_set_workspace_async(self._h, self._ws.data_ptr(), self._ws.numel(), B, T, _lib.stream_ptr()),
                       "set_workspace")
            self._ws_shape = (B, T)

    def _off(self, name: str) -> int:
        o = self._lib.mmda_misa_tensor_offset(self._h, name.encode())
        if o < 0:
            raise KeyError(name)
        return o

    def _ws_view(self, name: str, shape):
        n = 1
        for s in shape:
            n *= s
        o = self._off(name)
        return self._ws[o:o + n].view(shape)

    def _public(self) -> Dict[str, torch.Tensor]:
        """Views (into the workspace) of everything the reference's solver reads after a forward."""
        B, _ = self._ws_shape
        hs, nc = self.config.hidden_size, self.config.num_classes
        x6 = self._ws_view("x6", (6, B, hs))
        orig = self._ws_view("orig", (3, B, hs))
        recon = self._ws_view("recon", (3, B, hs))
        out = {"scores": self._ws_view("scores", (B, nc)), "tcp": self._ws_view("tcp", (B, 6)),
               "labels": self._ws_view("labels", (B, nc))}
        for i, m in enumerate("tva"):
            out[f"utt_{m}_orig"] = orig[i]
            out[f"utt_private_{m}"] = x6[i]
            out[f"utt_shared_{m}"] = x6[3 + i]
            out[f"utt_{m}_recon"] = recon[i]
        if not self.config.use_cmd_sim:
            dom = self._ws_view("dom", (3, B, 3))
            for i, m in enumerate("tva"):
                out[f"domain_label_{m}"] = dom[i]
        return out

    def _grad_slots(self) -> Dict[str, torch.Tensor]:
        B, _ = self._ws_shape
        hs, nc = self.config.hidden_size, self.config.num_classes
        dx6 = self._ws_view("d_x6", (6, B, hs))
        dorig = self._ws_view("d_orig", (3, B, hs))
        drec = self._ws_view("d_recon", (3, B, hs))
        out = {"scores": self._ws_view("d_scores", (B, nc)), "tcp": self._ws_view("d_tcp", (B, 6))}
        for i, m in enumerate("tva"):
            out[f"utt_{m}_orig"] = dorig[i]
            out[f"utt_private_{m}"] = dx6[i]
            out[f"utt_shared_{m}"] = dx6[3 + i]
            out[f"utt_{m}_recon"] = drec[i]
        if not self.config.use_cmd_sim:
            ddom = self._ws_view("d_dom", (3, B, 3))
            for i, m in enumerate("tva"):
                out[f"domain_label_{m}"] = ddom[i]
        return out

    def _next_seed(self) -> int:
        self._seed = (self._seed * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        return self._seed

    def _forward_raw(self, t, v, a, len_dev, training: bool, seed: int, inference: bool = False):
        # inference: a forward that no backward will follow (torch.no_grad()): no stash, no backward-only operand copies
        if not inference:
            self._sync_trainable()                          # (a step begins: the pass is planned with the set the backward will find)
        _lib.check(self._lib.mmda_misa_set_inference(self._h, int(inference)), "set_inference")
        _lib.check(self._lib.mmda_misa_forward(self._h, t.data_ptr(), v.data_ptr(), a.data_ptr(), len_dev.data_ptr(),
                                               int(training), seed, _lib.stream_ptr()), "mmda_misa_forward")
        self._fwd_id += 1
        self._last = dict(t=t, v=v, a=a, len_dev=len_dev)

    # ------------------------------------------------------------------ reference call surface
    def alignment(self, sentences, visual, acoustic, lengths, bert_sent=None, bert_sent_type=None, bert_sent_mask=None):
        """reference models.py:182-250 (whole encoder + fusion + heads in one native call)."""
        t, v, a, len_dev = self._prepare(sentences, visual, acoustic, lengths)
        seed = self._next_seed()
        if torch.is_grad_enabled():
            if self._anchor is None or self._anchor.device != t.device:
                self._anchor = torch.zeros(1, device=t.device, requires_grad=True)
            outs = _MISAFn.apply(self._anchor, self, t, v, a, len_dev, self.training, seed)
            return self._publish(dict(zip(_PUB, outs[:-1])), outs[-1])
        self._forward_raw(t, v, a, len_dev, self.training, seed, inference=True)
        return self._publish_workspace()

    def _publish(self, named, labels):
        """Sets the side-channel attributes the getters read (every name of ``_PUB`` but ``scores``; the domain labels are None under
        ``use_cmd_sim``) from ``named`` and returns (scores, labels)."""
        for k in _PUB:
            if k == "scores":
                continue
            val = named.get(k)
            if k.startswith("domain_label") and self.config.use_cmd_sim:
                val = None
            setattr(self, k, val)
        return named["scores"], labels

    def _publish_workspace(self):
        """What a forward under ``no_grad`` left in the workspace, published: one clone per tensor of ``_PUB`` in its order, then the
        labels -- the workspace is overwritten by the next forward, the attributes must not be."""
        pub = self._public()
        named = {k: pub[k].clone() if k in pub else None for k in _PUB}
        return self._publish(named, pub["labels"].clone())

    def forward(self, sentences, video, acoustic, lengths, bert_sent=None, bert_sent_type=None, bert_sent_mask=None):
        """reference models.py:282-285: returns (predicted_scores (B,6), predicted_labels (B,6) in {0,1})."""
        return self.alignment(sentences, video, acoustic, lengths, bert_sent, bert_sent_type, bert_sent_mask)

    # written-but-unread attributes of the reference (models.py:234-237,256-258), materialised on demand with the HIP GEMM
    @property
    def utt_t(self):
        return self.utt_private_t + self.utt_shared_t

    @property
    def utt_v(self):
        return self.utt_private_v + self.utt_shared_v

    @property
    def utt_a(self):
        return self.utt_private_a + self.utt_shared_a

    # sp_discriminator outputs (models.py:234-237): the reference computes them every forward and never reads them (no loss uses
    # them), so the hot path skips the dead GEMMs; the attributes are materialised on demand on the HIP GEMM.
    def _sp_disc(self, x):
        from . import ops
        w = self.sp_discriminator.sp_discriminator_layer_1.weight
        b = self.sp_discriminator.sp_discriminator_layer_1.bias
        return ops.gemm(x.detach().contiguous(), w.detach(), mode="fp32", bias=b.detach())

    @property
    def shared_or_private_p_t(self):
        return self._sp_disc(self.utt_private_t)

    @property
    def shared_or_private_p_v(self):
        return self._sp_disc(self.utt_private_v)

    @property
    def shared_or_private_p_a(self):
        return self._sp_disc(self.utt_private_a)

    @property
    def shared_or_private_s(self):
        return self._sp_disc((self.utt_shared_t + self.utt_shared_v + self.utt_shared_a) / 3.0)

    # ------------------------------------------------------------------ fused fast path (Solver.train_epoch)
    def train_step(self, sentences, video, acoustic, lengths, emo_label, lr: float, clip: float, do_adam: bool = True,
                   training: bool = True, seed=None, grad_sync=None, optimizer=None, accum_index: int = 0, accum_count: int = 1,
                   clip_norm=None):
        """One reference loop iteration (solver.py:139-186) in native code: zero_grad, forward, six losses, backward,
        clip + Adam.  ``grad_sync(flat_grad_bucket, dense_floats, model)`` is called between backward and Adam for the
        data-parallel all-reduce (mmda_amd/dist.py) and must return the gradient scale (1/world).
        ``optimizer``: an mmda_amd.optim optimizer attached to this model.  Adam (or None) is stepped by the native fused
        clamp+Adam with ``lr`` and the optimizer's own ``betas``, ``eps`` and weight decay (``optimizer=None``: Adam's defaults, no
        decay); any other (RMSprop, config.py:24) by its own fused kernel after the gradient exchange.
        ``clip_norm``: ``torch.nn.utils.clip_grad_norm_(clip_norm)`` in front of the value clip, on the device; ``grad_norm()`` then
        holds the step's norm.
        Losses stay on the device (read them with ``read_losses()``; one sync, not six).
        ``accum_index`` / ``accum_count``: this batch is micro-batch ``accum_index`` of an optimizer step made from ``accum_count``
        consecutive calls (0, 1, ... count - 1, the same count in each): the gradients of the micro-batches are summed in that order and
        the last call takes one clip + Adam step with their mean -- what ``accum_count`` data-parallel ranks would compute."""
        if accum_count != 1 or accum_index != 0 or self._acc_next:
            return self._accum_micro_step(sentences, video, acoustic, lengths, emo_label, lr, clip, do_adam, training, seed, grad_sync,
                                          optimizer, accum_index, accum_count, clip_norm)
        (t, v, a, len_dev), emo, seed, custom, adam = self._step_begin((sentences, video, acoustic, lengths), emo_label, optimizer, clip_norm,
                                                                       do_adam, seed, exchange=grad_sync is not None)
        s = _lib.stream_ptr()
        fused_adam = do_adam and grad_sync is None and not custom
        gs_owner = getattr(grad_sync, "__self__", None)
        global_stats = getattr(gs_owner, "global_stats", False) and (gs_owner.world > 1 or gs_owner.force_collectives)
        if global_stats:
            self._global_stats_step(t, v, a, len_dev, emo, training, seed, gs_owner)
        else:
            _lib.check(self._lib.mmda_misa_train_step(self._h, t.data_ptr(), v.data_ptr(), a.data_ptr(), len_dev.data_ptr(),
                                                      emo.data_ptr(), int(training), seed, int(fused_adam), lr, clip, max(self._step, 1), s),
                       "mmda_misa_train_step")
        rows = self.embed_update in ("sparse", "deferred") and not fused_adam     # (pending: the native side holds t, len_dev until then)
        self._step_end(dict(t=t, v=v, a=a, len_dev=len_dev, emo=emo), rows, (t, len_dev) if rows else None, forwarded=not global_stats)
        self._df_dirty = self._df_dirty or (self.embed_update == "deferred" and fused_adam)
        if not do_adam or fused_adam:
            return
        step_no = max(self._step, 1)
        early = None
        if not custom:
            # A DataParallelSync (dist.py) steps the early-reduced prefix on its communication stream; the rest here, behind the exchange
            def early(n_floats, stream, _gs=1.0 / float(getattr(gs_owner, "world", 1))):
                self._adam_range(0, int(n_floats), lr, clip, _gs, step_no, stream.cuda_stream, adam, "adam(early)")
        scale, done = self._exchange(grad_sync, early) if grad_sync is not None else (1.0, 0)
        if custom:
            optimizer.step(clip_value=clip, grad_scale=scale)
        elif done > 0:
            self._adam_range(done, self.grad_floats - done, lr, clip, scale, step_no, s, adam, "adam(rest)")
        else:
            _lib.check(self._lib.mmda_misa_adam_step(self._h, lr, clip, scale, self._step, s), "adam_step")

    # ------------------------------------------------------------------ what the step methods share
    def _step_begin(self, batch, emo_label, optimizer, clip_norm, do_adam, seed, exchange=False, accumulate=False, encoded=False):
        """The beginning of a step: what no step does is refused (step_rules), by name and before anything changes; the optimizer's
        settings and the trainable set reach the native side; the batch -- (sentences, video, acoustic, lengths) or an EncodedBatch -- is
        prepared; then a seed is drawn and the step counted (a custom optimizer counts its own steps on the same counter, an accumulated
        step is counted by its closing micro-batch).  Returns (io, labels, seed, custom, Adam settings)."""
        if encoded:
            io, adam = self._encoded_begin(batch, "train_step_encoded", optimizer, clip_norm, exchange, accumulate, do_adam)
            if batch.cache.emo is None:
                raise _lib.MMDAError("train_step_encoded: the cache has no emotion labels (its dataset had none)")
            if batch.cache.task != self.task:
                raise _lib.MMDAError(f"train_step_encoded: the cache's label table was stored under task='{batch.cache.task}', the model's "
                                     f"task is '{self.task}': rebuild it (EncoderCache.build)")
            self._send_adam(adam)
            emo = torch.empty(batch.B, self.config.num_classes, dtype=torch.float32, device=batch.cache.device)
        else:
            adam = self._send_adam(self._rules(optimizer, clip_norm, exchange, accumulate, False, do_adam))
            self._sync_trainable(exchange=exchange)
            io = self._prepare(*batch)
            emo = emo_label.to(device=io[0].device, dtype=torch.float32).contiguous()
            if self.task == "sentiment" and emo.numel() != io[0].shape[1]:
                raise ValueError(f"task='sentiment' takes the (B,) or (B, 1) sentiment column: the target has {emo.numel()} entries, the "
                                 f"batch {io[0].shape[1]} samples")
        if seed is None:
            seed = self._next_seed()
        custom = do_adam and optimizer is not None and not isinstance(optimizer, _optim.Adam)
        if not custom and not accumulate:
            self._step += 1
        return io, emo, seed, custom, adam

    def _step_end(self, last, rows_pending=False, rows_keep=None, forwarded=True):
        """The end of a native step: what the autograd path, the rows updates and the next step read of it."""
        if forwarded:
            self._fwd_id += 1
        self._last = last
        self._rows_pending, self._rows_clip, self._rows_keep = rows_pending, None, rows_keep

    def _exchange(self, grad_sync, early=None):
        """The step's one gradient exchange: ``grad_sync(bucket, dense_floats, model)`` or a plain ``(bucket, dense_floats)`` callable --
        decided from its signature, never by retrying after a TypeError, which could come from behind an issued collective.  ``early``:
        a DataParallelSync's early-step hook for the call.  Returns (gradient scale, floats of the bucket prefix the hook stepped)."""
        owner = getattr(grad_sync, "__self__", None)
        hook = early is not None and all(hasattr(owner, x) for x in ("early_step", "early_stepped", "world"))
        if hook:
            owner.early_step = early
        try:
            scale = grad_sync(self._G, self._dense_floats, self) if _takes_model(grad_sync) else grad_sync(self._G, self._dense_floats)
        finally:
            if hook:
                owner.early_step = None
        return float(scale), (int(owner.early_stepped) if hook else 0)

    # ------------------------------------------------------------------ the optimizer's settings
    def _rules(self, optimizer=None, clip_norm=None, exchange=False, accumulate=False, encoded=False, do_adam=True):
        """The Adam settings of a step -- the attached optimizer's betas, eps, weight decay and decay kind (``None`` or another optimizer
        class: Adam's defaults) and ``clip_norm`` -- once step_rules lets the step pass (the steady state: one tuple compare)."""
        key = optimizer.settings() if isinstance(optimizer, _optim.Adam) else _ADAM_DEFAULTS[:5]
        case = (self.embed_update, type(optimizer), key[3], clip_norm, exchange, accumulate, encoded, do_adam)
        if case != self._rules_passed:
            kind, name = _optim.rule_kind(optimizer)
            step_rules.check(embed_update=self.embed_update, optimizer=kind, optimizer_name=name, weight_decay=key[3], clip_norm=clip_norm,
                             exchange=exchange, accumulate=accumulate, encoded=encoded, do_adam=do_adam)
            self._rules_passed = case
        return key + (0.0 if clip_norm is None else float(clip_norm),)

    def _send_adam(self, key):
        """``mmda_misa_set_adam`` when the settings differ from what was sent last (the steady state: one tuple compare)."""
        if key != self._adam_pushed:
            if self.embed_update == "deferred" and key[:3] != self._adam_pushed[:3]:
                self.flush_embedding()                      # stale rows replay the steps they missed under the betas those were made with
            opts = _lib.AdamOpts(beta1=key[0], beta2=key[1], eps=key[2], weight_decay=key[3], decoupled=int(key[4]), scale_dev=None)
            _lib.check(self._lib.mmda_misa_set_adam(self._h, C.byref(opts), key[5]), "mmda_misa_set_adam")
            self._adam_pushed = key
        return key

    def _push_adam(self, optimizer, clip_norm, exchange: bool = False):
        """The Adam settings of the step about to run, on the handle; raises, by name and before anything changes, for what no step does"""
        return self._send_adam(self._rules(optimizer, clip_norm, exchange))

    def _adam_range(self, first: int, n: int, lr, clip, grad_scale, step, stream, adam, what: str):
        """clamp + Adam over floats [first, first + n) of the flat buckets with the settings ``adam`` (the data-parallel step's launches)."""
        ptrs = [x.data_ptr() + first * 4 for x in (self._P, self._G, self._M, self._V)]
        _optim.clamp_adam(self._lib, *ptrs, n, None, lr, clip, grad_scale, step, adam, None, stream, what)

    def grad_norm(self) -> torch.Tensor:
        """The gradient norm of the last step taken with ``clip_norm`` (what ``clip_grad_norm_`` returns), as a 0-d view of device
        memory: reading it costs no sync until the caller asks for its value."""
        if self._ws is None:
            raise _lib.MMDAError("grad_norm(): no step has run yet")
        return self._ws_view("grad_norm", (2,))[0]

    # ------------------------------------------------------------------ steps that start behind the encoders (mmda_amd/encoded.py)
    def _encoded_begin(self, batch, what: str, optimizer=None, clip_norm=None, exchange=False, accumulate=False, do_adam=True):
        """Everything a step from the encoder cache refuses, by name and before any launch; then the workspace carved at (B, 1) --
        nothing such a step runs depends on T -- and the native batch, with the step's Adam settings."""
        from .encoded import EncodedBatch
        if not isinstance(batch, EncodedBatch):
            raise TypeError(f"{what} takes an EncodedBatch (EncodedLoader yields them), not {type(batch).__name__}")
        dist = torch.distributed
        adam = self._rules(optimizer, clip_norm, exchange or (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1),
                           accumulate or self.accum_steps > 1 or bool(self._acc_next), True, do_adam)
        cache = batch.cache
        cache._refuse(self)                                  # another device, other widths
        flags = self._sync_trainable()
        if flags != self._cut_flags:                        # (the steady state: one tuple compare)
            if not self.trainable_info()[2]:
                from .encoded import ENCODER_PREFIXES
                live = [n for n, f in zip(self._native_names, flags) if f and n.split(".")[0] in ENCODER_PREFIXES]
                if self.embed_update in ("sparse", "deferred"):
                    live.append(f"embed.weight (embed_update='{self.embed_update}' trains the table through its rows)")
                raise _lib.MMDAError(f"{what} needs the encoder cut -- every recurrent layer, the three inter-layer LayerNorms and the "
                                     f"table frozen (MISA.freeze): the cached rows are constants only then.  Still trainable: {live}")
            self._cut_flags = flags
        if cache.device.type != "cuda":
            raise _lib.MMDAError(f"{what}: the cache is on {cache.device}: mmda_amd.MISA has no CPU path (HIP kernels only)")
        if not self._views_valid():
            self._materialize(cache.device)
        self._carve(batch.B, 1, cache.device)
        return _lib.EncodedBatch(tab_t=cache.utt_t.data_ptr(), tab_v=cache.utt_v.data_ptr(), tab_a=cache.utt_a.data_ptr(),
                                 tab_emo=_lib.ptr(cache.emo), rows=batch.rows_ptr, B=batch.B), adam

    def train_step_encoded(self, batch, lr: float, clip: float, do_adam: bool = True, training: bool = True, seed=None, optimizer=None,
                           grad_sync=None, accum_index: int = 0, accum_count: int = 1, clip_norm=None):
        """``train_step`` from the encoder cache: ``batch`` is an ``EncodedBatch``; the step gathers its rows (and labels) in one launch
        and starts at the projections.  Needs the encoder cut; seeds, the step counter and ``optimizer`` are ``train_step``'s (a
        custom optimizer, RMSprop, is stepped by its own kernel behind the native step without its Adam).  ``grad_sync`` and the
        accumulation arguments exist to be refused by name."""
        eb, emo, seed, custom, _ = self._step_begin(batch, None, optimizer, clip_norm, do_adam, seed, exchange=grad_sync is not None,
                                                    accumulate=accum_index != 0 or accum_count != 1, encoded=True)
        _lib.check(self._lib.mmda_misa_train_step_encoded(self._h, C.byref(eb), emo.data_ptr(), int(training), seed, int(do_adam and not custom),
                                                          lr, clip, max(self._step, 1), _lib.stream_ptr()), "mmda_misa_train_step_encoded")
        self._step_end(dict(encoded=batch, emo=emo))
        if custom:
            optimizer.step(clip_value=clip, grad_scale=1.0)

    def forward_encoded(self, batch, keep=None):
        """``model(...)`` under ``torch.no_grad()`` from the encoder cache: (scores, labels) of the batch, the side-channel attributes
        set as ``alignment`` sets them.  Draws one seed, as ``model(...)`` does.  ``keep`` exists to be refused by name: a keep set
        other than 7 (mmda_amd/modality.py) needs the encoders run on the masked input, and the cache holds whole samples."""
        if keep is not None:
            from .modality import parse_keep
            step_rules.modality_check(parse_keep(keep), encoded=True)
        if torch.is_grad_enabled():
            raise _lib.MMDAError("autograd through forward_encoded is not built: call it under torch.no_grad() (train with train_step_encoded)")
        eb, _ = self._encoded_begin(batch, "forward_encoded")
        eb.tab_emo = None
        seed = self._next_seed()
        _lib.check(self._lib.mmda_misa_set_inference(self._h, 1), "set_inference")
        _lib.check(self._lib.mmda_misa_forward_encoded(self._h, C.byref(eb), int(self.training), seed, _lib.stream_ptr()),
                   "mmda_misa_forward_encoded")
        self._fwd_id += 1
        self._last = dict(encoded=batch)
        return self._publish_workspace()

    def _forward_encoded_raw(self, cache, rows_ptr: int, B: int, training: bool, seed: int):
        """A forward from ``B`` cached rows (``rows_ptr``: their int32 indices on the device, repeats allowed) that no backward will
        follow: ``mmda_misa_set_inference(1)`` and ``mmda_misa_forward_encoded`` at the carve (B, 1), with the seed it is GIVEN -- none
        is drawn.  Unlike ``_encoded_begin`` it does not ask for the encoder cut: an inference forward trains nothing, so the cached
        rows only have to be those of the current encoders (the caller's concern: ``EncoderCache`` fingerprints).  Results stay in
        the workspace (mmda_amd/uncertainty.py reduces them there)."""
        cache._refuse(self)                                  # another device, other widths
        if cache.device.type != "cuda":
            raise _lib.MMDAError(f"the cache is on {cache.device}: mmda_amd.MISA has no CPU path (HIP kernels only)")
        if not self._views_valid():
            self._materialize(cache.device)
        self._carve(int(B), 1, cache.device)
        eb = _lib.EncodedBatch(tab_t=cache.utt_t.data_ptr(), tab_v=cache.utt_v.data_ptr(), tab_a=cache.utt_a.data_ptr(), tab_emo=None,
                               rows=rows_ptr, B=int(B))
        _lib.check(self._lib.mmda_misa_set_inference(self._h, 1), "set_inference")
        _lib.check(self._lib.mmda_misa_forward_encoded(self._h, C.byref(eb), int(training), int(seed) & 0xFFFFFFFFFFFFFFFF, _lib.stream_ptr()),
                   "mmda_misa_forward_encoded")
        self._fwd_id += 1
        self._last = dict(encoded=cache)

    def _accum_micro_step(self, sentences, video, acoustic, lengths, emo_label, lr, clip, do_adam, training, seed, grad_sync, optimizer,
                          index, count, clip_norm=None) -> None:
        """Micro-batch ``index`` of an optimizer step made from ``count``: the native step without its optimizer part, then either the
        add into the second bucket or -- behind the last one -- clip + Adam on (accumulated + this micro-batch's gradients) / count."""
        expected, self._acc_next = self._acc_next, 0           # (any refusal below leaves the sequence reset)
        self._acc_used = 0 if expected == 0 else self._acc_used
        for x in (index, count):
            if isinstance(x, bool) or not isinstance(x, int):
                raise _lib.MMDAError("accum_index / accum_count must be ints")
        if count < 1 or not 0 <= index < count:
            raise _lib.MMDAError(f"accum_index {index} is outside [0, accum_count = {count})")
        if index != expected or (index > 0 and count != self._acc_count):
            raise _lib.MMDAError(f"accumulated step: micro-batch {index} of {count} arrived where {expected} of "
                                 f"{self._acc_count if expected else count} was due (indices run 0 .. count - 1 with one count); "
                                 "the sequence starts over")
        (t, v, a, len_dev), emo, seed, _, _ = self._step_begin((sentences, video, acoustic, lengths), emo_label, optimizer, clip_norm, do_adam,
                                                               seed, exchange=grad_sync is not None, accumulate=True)
        s = _lib.stream_ptr()
        lib, h = self._lib, self._h
        _lib.check(lib.mmda_misa_train_step(h, t.data_ptr(), v.data_ptr(), a.data_ptr(), len_dev.data_ptr(), emo.data_ptr(), int(training),
                                            seed, 0, lr, clip, max(self._step, 1), s), "mmda_misa_train_step")
        self._step_end(dict(t=t, v=v, a=a, len_dev=len_dev, emo=emo))       # (sparse: the rows go to the list below, nothing stays pending)
        closing = index == count - 1
        n = self.grad_floats
        if count > 1 and (self._acc is None or self._acc.numel() < n or self._acc.device != t.device):
            if index > 0:
                raise _lib.MMDAError("accumulated step: the gradient bucket changed size or device between micro-batches")
            self._acc = torch.empty(n, dtype=torch.float32, device=t.device)
        ids_p = rows_p = None
        cap = 0
        if self.embed_update == "sparse":
            D = self._layout["embed.weight"][1][1]
            need = self._acc_used + t.numel()
            old = self._acc_list
            if old is None or old[0].numel() < need or old[0].device != t.device:
                room = max(need, count * t.numel())            # (equal micro-batches: the step's whole list at once)
                ids = torch.empty(room, dtype=torch.int64, device=t.device)
                rows = torch.empty((room, D), dtype=torch.float32, device=t.device)
                if old is not None and self._acc_used > 0:
                    ids[:self._acc_used].copy_(old[0][:self._acc_used])
                    rows[:self._acc_used].copy_(old[1][:self._acc_used])
                self._acc_list = (ids, rows)
            ids_p, rows_p, cap = self._acc_list[0].data_ptr(), self._acc_list[1].data_ptr(), self._acc_list[0].numel()
        if not closing:
            _lib.check(lib.mmda_misa_grad_accumulate(h, self._acc.data_ptr(), int(index == 0), ids_p, rows_p, self._acc_used, cap, s),
                       "mmda_misa_grad_accumulate")
            self._acc_used += t.numel()
            self._acc_next, self._acc_count = index + 1, count
            return
        self._step += 1
        _lib.check(lib.mmda_misa_adam_step_accumulated(h, self._acc.data_ptr() if count > 1 else None, ids_p, rows_p, self._acc_used, cap,
                                                       lr, clip, 1.0 / count, self._step, s), "mmda_misa_adam_step_accumulated")
        self._acc_used = 0

    def _global_stats_step(self, t, v, a, len_dev, emo, training: bool, seed: int, dp) -> None:
        """forward + losses + backward of one step with the batch-statistic losses on the batch of ALL ranks (DataParallelSync
        global_stats=True).  Reference: on one device DiffLoss (utils/functions.py:64-76), CMD (:89-108) and the
        confidence loss (solver.py:451-462) see the whole batch; here every rank gathers the (6, B, hs) private / shared utterance
        vectors -- and scores, tcp, labels for the confidence loss -- of all ranks, runs the SAME loss entry points on the gathered
        batch, keeps the loss sums and adds ITS rows of the gradients, times the world size (the gradient exchange averages over
        ranks; cls and recon are means over samples, for which the average of the shard gradients already is the global gradient).
        Equal batch shapes on all ranks."""
        lib, h, cfg = self._lib, self._h, self.config
        if not cfg.use_cmd_sim:
            raise NotImplementedError("global_stats: the CMD similarity branch only (config.use_cmd_sim)")
        s = _lib.stream_ptr()
        W, r = int(dp.world), int(dp.rank)
        _lib.check(lib.mmda_misa_zero_grad(h, s), "zero_grad")
        self._forward_raw(t, v, a, len_dev, training, seed, inference=False)
        _lib.check(lib.mmda_misa_zero_act_grads(h, s), "zero_act_grads")
        B, _ = self._ws_shape
        hs, nc = int(cfg.hidden_size), int(cfg.num_classes)
        Bg = W * B
        L = self._ws_view("losses", (8,))
        X = dp.gather_rows(self._ws_view("x6", (6, B, hs)), dim=1)                    # (6, W B, hs): rank r at rows [r B, (r + 1) B)
        dX = torch.zeros_like(X)
        work = torch.empty(int(lib.mmda_loss_diff_work_floats(Bg, hs)), dtype=torch.float32, device=X.device)
        _lib.check(lib.mmda_loss_diff(X.data_ptr(), Bg * hs, Bg, hs, float(getattr(cfg, "diff_weight", 0.3)), L.data_ptr() + 4, dX.data_ptr(),
                                      work.data_ptr(), s), "loss_diff(global)")
        _lib.check(lib.mmda_loss_cmd(X[3:].data_ptr(), Bg * hs, Bg, hs, float(getattr(cfg, "sim_weight", 0.7)), L.data_ptr() + 8,
                                     dX[3:].data_ptr(), s), "loss_cmd(global)")
        self._ws_view("d_x6", (6, B, hs)).add_(dX[:, r * B:(r + 1) * B], alpha=float(W))
        if nc == 6:
            S = dp.gather_rows(self._ws_view("scores", (B, nc)))
            Tc = dp.gather_rows(self._ws_view("tcp", (B, 6)))
            E = dp.gather_rows(emo)
            with_g = bool(getattr(cfg, "use_confidNet", False))
            dS = torch.zeros_like(S) if with_g else None
            dT = torch.zeros_like(Tc) if with_g else None
            _lib.check(lib.mmda_loss_conf(S.data_ptr(), Tc.data_ptr(), E.data_ptr(), Bg, nc, float(getattr(cfg, "conf_weight", 0.3)),
                                          L.data_ptr() + 16, dS.data_ptr() if with_g else None, dT.data_ptr() if with_g else None, s),
                       "loss_conf(global)")
            if with_g:
                self._ws_view("d_scores", (B, nc)).add_(dS[r * B:(r + 1) * B], alpha=float(W))
                self._ws_view("d_tcp", (B, 6)).add_(dT[r * B:(r + 1) * B], alpha=float(W))
        _lib.check(lib.mmda_misa_set_external_batch_losses(h, 1), "set_external_batch_losses")
        try:
            _lib.check(lib.mmda_misa_losses(h, emo.data_ptr(), 1, s), "mmda_misa_losses")
        finally:
            lib.mmda_misa_set_external_batch_losses(h, 0)
        _lib.check(lib.mmda_misa_backward(h, t.data_ptr(), v.data_ptr(), a.data_ptr(), len_dev.data_ptr(), s), "mmda_misa_backward")
        # (keep the gathered tensors alive until the stream has run the launches that read them)
        self._gs_keep = (X, dX, work)

    # ------------------------------------------------------------------ early part of the gradient bucket (data parallel)
    def early_grad_floats(self) -> int:
        """Length of the gradient-bucket prefix (fusion block, LayerNorms, layer-2 recurrent layers) whose gradients are final
        beside the layer-1 backward recurrence of the step that was just issued; 0 if nothing is early."""
        return int(self._lib.mmda_misa_early_grad_floats(self._h))

    def wait_early_grads(self, stream) -> None:
        """Make ``stream`` (a torch.cuda.Stream) wait for the event after which that prefix may be read."""
        _lib.check(self._lib.mmda_misa_wait_early_grads(self._h, stream.cuda_stream), "wait_early_grads")

    # ------------------------------------------------------------------ sparse view of the embedding gradient (data parallel)
    def embedding_grad_rows(self):
        """(ids (R,) int64, rows (R, d_t) fp32) of the last backward: embed.weight.grad == sum over the list of rows[p] into row
        ids[p].  The dense gradient is non-zero in at most R = T*B of its V rows, so data-parallel ranks exchange these instead of
        V x d_t.  Positions past a sample's length carry id -1 (their rows are exactly zero: no gradient flows through padding)."""
        if self.embed_update == "frozen":
            raise _lib.MMDAError("embed_update='frozen': no gradient with respect to the embedding rows is computed")
        t = self._last["t"]
        T, B = t.shape
        R = T * B
        pad = torch.arange(T, device=t.device, dtype=torch.int32).unsqueeze(1) >= self._last["len_dev"].unsqueeze(0)
        ids = torch.where(pad, torch.full_like(t, -1), t)
        return ids.reshape(R), self._ws_view("d_x_t", (R, self._layout["embed.weight"][1][1]))

    def embedding_rows_per_step(self):
        """T * B of the last step: the rows the (ids, rows) form of the embedding gradient holds (None before the first step)."""
        return None if not getattr(self, "_last", None) else int(self._last["t"].numel())

    def embedding_table_rows(self):
        """V: the rows a dense exchange of embed.weight.grad moves."""
        return int(self._layout["embed.weight"][1][0])

    def scatter_embedding_rows(self, ids: torch.Tensor, rows: torch.Tensor):
        """embed.weight.grad[ids] += rows with the native atomic scatter-add (summation order not fixed; ids < 0 not allowed)."""
        if ids.numel() == 0:
            return
        off, (V, D) = self._layout["embed.weight"]
        g = self._G[off:off + V * D]
        _lib.check(self._lib.mmda_embed_scatter_add(g.data_ptr(), ids.contiguous().data_ptr(), ids.numel(), D,
                                                    rows.contiguous().data_ptr(), _lib.stream_ptr()), "embed_scatter_add")

    def set_embedding_grad_rows(self, ids: torch.Tensor, rows: torch.Tensor):
        """embed.weight.grad[id] = sum of rows[p] over the positions with ids[p] == id, added in list order by the native
        deterministic segment sum (rows of ids that occur are overwritten, ids < 0 skipped): what every data-parallel rank runs on
        the same all-gathered list, so that replicas stay bit-identical."""
        n = ids.numel()
        if n == 0:
            return
        off, (V, D) = self._layout["embed.weight"]
        g = self._G[off:off + V * D]
        need = int(self._lib.mmda_embed_segment_sum_work_bytes(n, D))
        if self._seg_work is None or self._seg_work.numel() < need or self._seg_work.device != g.device:
            self._seg_work = torch.empty(need, dtype=torch.uint8, device=g.device)
        _lib.check(self._lib.mmda_embed_segment_sum(g.data_ptr(), ids.contiguous().data_ptr(), n, D, rows.contiguous().data_ptr(),
                                                    self._seg_work.data_ptr(), self._seg_work.numel(), _lib.stream_ptr()),
                   "embed_segment_sum")

    def read_losses(self) -> Dict[str, float]:
        """cls, diff, sim, recon, conf, total of the last losses pass (one device->host sync); under task='sentiment' cls is the
        regression loss."""
        L = self._ws_view("losses", (8,)).tolist()
        return dict(cls=L[0], diff=L[1], sim=L[2], recon=L[3], conf=L[4], total=L[5])

    def flat_buckets(self):
        """(params, grads, adam_m, adam_v) flat fp32 device tensors; the first `dense_floats` entries exclude embed.weight."""
        return self._P, self._G, self._M, self._V

    @property
    def dense_floats(self) -> int:
        return self._dense_floats

    @property
    def grad_floats(self) -> int:
        """Floats of the flat buckets that carry a dense gradient and take the dense optimizer launch: everything, or (embed_update
        'sparse' / 'frozen' / 'deferred') the prefix in front of embed.weight."""
        return self._flat_floats if self.embed_update == "dense" else self._dense_floats

    def apply_sparse_rows(self, lr: float, step: int, clip: float, grad_scale: float = 1.0, betas=(0.9, 0.999), eps: float = 1e-8) -> bool:
        """embed_update='sparse': the SparseAdam update of the rows the last backward touched (coalesce, scale, clamp, update: one fused
        native pass over d_x_t), once per backward.  Returns False when no backward is pending."""
        if self.embed_update != "sparse" or not self._rows_pending:
            return False
        from . import ops
        off, (V, D) = self._layout["embed.weight"]
        t = self._last["t"]
        ops.embed_rows_sparse_adam(self._P[off:off + V * D].view(V, D), self._M[off:off + V * D].view(V, D),
                                   self._V[off:off + V * D].view(V, D), t, self._ws_view("d_x_t", (t.numel(), D)), lr, step,
                                   lengths=self._last["len_dev"], clip=clip, grad_scale=grad_scale, betas=betas, eps=eps)
        self._rows_pending = False
        self._rows_clip = None
        return True

    def apply_deferred_rows(self, lr: float, step: int, clip: float, grad_scale: float = 1.0, betas=(0.9, 0.999), eps: float = 1e-8) -> bool:
        """embed_update='deferred': dense Adam's step `step` for the rows the last backward touched, with the sums the dense scatter
        would have left in embed.weight.grad (one fused native pass over d_x_t), once per backward; every other row takes the step when it
        is next needed.  Returns False when no backward is pending."""
        if self.embed_update != "deferred" or not self._rows_pending:
            return False
        # (the model-level entry: the native model counts the updates of this path and of the fused step in one place; it runs
        # mmda_embed_rows_dense_adam on the ids, lengths and d_x_t of that backward, which self._rows_keep keeps alive)
        _lib.check(self._lib.mmda_misa_embed_deferred_step(self._h, lr, betas[0], betas[1], eps, clip, grad_scale, int(step),
                                                           _lib.stream_ptr()), "embed_deferred_step")
        self._rows_pending = False
        self._rows_clip = None
        self._rows_keep = None
        self._df_dirty = True
        return True

    def cluster_aborted(self) -> bool:
        """True if a resident-weights recurrence ever timed out waiting for its cluster (results are invalid after that).
        Synchronous device->host read: call it off the step path."""
        import ctypes
        if self._ws is None or self._ws_shape is None:
            return self._abort_seen
        flag = ctypes.c_int(0)
        _lib.check(self._lib.mmda_misa_cluster_status(self._h, ctypes.byref(flag)), "cluster_status")
        self._abort_seen = self._abort_seen or bool(flag.value)
        self._abort_bits = getattr(self, "_abort_bits", 0) | int(flag.value)
        return self._abort_seen

    def check_cluster(self, where: str = ""):
        """Raises MMDAError if a recurrence ever gave up waiting for its cluster (every result since then is invalid).
        One synchronous device->host read: Solver calls it once per epoch / evaluation pass and before saving a checkpoint."""
        if self.cluster_aborted():
            # The hand-off tags every published bf16 value with its epoch in a spare bit: a NaN / an overflowing activation reads as a tag
            # that never matches, so a DIVERGED run ends here too (the reference would print NaN losses).  Say which one it was.
            nonfinite = False
            try:
                L = self._ws_view("losses", (8,)).tolist()
                nonfinite = any(x != x or abs(x) == float("inf") for x in L[:6]) or not bool(torch.isfinite(self._P).all())
            except Exception:
                pass
            what = ("non-finite values reached a recurrence (diverged run: NaN / inf in the losses or parameters), which its data-tagged "
                    "hand-off reports as a cluster time-out" if nonfinite else
                    "a resident-weights recurrence timed out waiting for its workgroup cluster")
            if not nonfinite and (getattr(self, "_abort_bits", 0) & 2):
                what = ("a kernel of the fused training step timed out waiting on the device for the side stream's chain (flag join): are "
                        "kernel dispatches being serialised (profiler counters)?  Run such tools with MMDA_FLAG_JOIN=0 MMDA_SORT_EARLY=0")
            raise _lib.MMDAError(what + (f" ({where})" if where else "") + ": results since then are invalid")

    def set_recurrence(self, resident_weights: bool):
        """bf16 recurrences: W_hh resident in LDS across a workgroup cluster (default) or streamed from L2 per step."""
        _lib.check(self._lib.mmda_misa_set_recurrence(self._h, int(resident_weights)), "set_recurrence")

    def set_gemm_operands(self, bf16_copies: bool):
        """bf16 mode: LSTM-sized GEMMs on bf16 operand copies (default) or on fp32 tensors staged through the generic kernel."""
        _lib.check(self._lib.mmda_misa_set_gemm_operands(self._h, int(bf16_copies)), "set_gemm_operands")

    def set_fusion_fp8(self, on: bool):
        """Forward feed-forward products of the fusion transformer layer (linear1 / linear2, reference models.py:160-161) on
        block-scaled fp8 MFMA operands; the backward pass stays exact (straight-through)."""
        self.fusion_fp8 = bool(on)
        _lib.check(self._lib.mmda_misa_set_fusion_fp8(self._h, int(on)), "set_fusion_fp8")

    def set_embed_background(self, on: bool, workgroups: int = 0):
        """Plain dense mode: the Adam step of the table rows a batch does not index runs as a throttled background pass beside the
        forward pass of the fused step (the bits of the one dense launch).  ``on=True``: in every eligible step (a model left alone runs
        it where it pays, at batches of up to 32 samples); ``workgroups``: the throttle, 0 = the default.  Overrides MMDA_EMBED_BG /
        MMDA_EMBED_BG_WGS for this model."""
        _lib.check(self._lib.mmda_misa_set_embed_background(self._h, int(bool(on)), int(workgroups)), "set_embed_background")

    def embed_background_active(self) -> bool:
        """Whether the last fused training step ran the background pass over the embedding table."""
        return self._lib.mmda_misa_embed_background_active(self._h) == 1

    def set_precision(self, precision: str):
        self.precision = precision
        _lib.check(self._lib.mmda_misa_set_mode(self._h, _lib.BF16 if precision == "bf16" else _lib.F32), "set_mode")

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._lib.mmda_misa_destroy(self._h)
                self._h = None
        except Exception:
            pass


class _MISAFn(torch.autograd.Function):
    """Autograd tape entry for the compat path: forward and backward are single native calls; the anchor input only
    exists so that the outputs require grad.  Parameter gradients are ACCUMULATED into the flat bucket (and exposed as
    ``p.grad`` views), like ``loss.backward()`` accumulates in the reference."""

    @staticmethod
    def forward(ctx, anchor, model, t, v, a, len_dev, training, seed):
        model._forward_raw(t, v, a, len_dev, training, seed)
        pub = model._public()
        outs = []
        for k in _PUB:
            outs.append(pub[k].clone() if k in pub else torch.zeros(0, device=t.device))
        labels = pub["labels"].clone()
        ctx.model = model
        ctx.fwd_id = model._fwd_id
        ctx.io = (t, v, a, len_dev)
        ctx.mark_non_differentiable(labels)
        return tuple(outs) + (labels,)

    @staticmethod
    def backward(ctx, *grads):
        model = ctx.model
        if ctx.fwd_id != model._fwd_id:
            raise RuntimeError("backward through a stale MISA forward: activations live in a per-model workspace that the "
                               "next forward overwrites (run forward -> backward in order, as the reference loop does)")
        lib = model._lib
        s = _lib.stream_ptr()
        _lib.check(lib.mmda_misa_zero_act_grads(model._h, s), "zero_act_grads")
        slots = model._grad_slots()
        for k, g in zip(_PUB, grads[:-1]):
            if g is not None and k in slots and g.numel() > 0:
                slots[k].copy_(g)
        t, v, a, len_dev = ctx.io
        model._sync_trainable()
        _lib.check(lib.mmda_misa_backward(model._h, t.data_ptr(), v.data_ptr(), a.data_ptr(), len_dev.data_ptr(), s),
                   "mmda_misa_backward")
        model._rows_pending = model.embed_update in ("sparse", "deferred")
        model._rows_clip = None
        model._rows_keep = (t, len_dev) if model._rows_pending else None   # (the native side holds these pointers until the rows update)
        model._assign_grad_views()
        return (torch.zeros_like(model._anchor),) + (None,) * 7


Model = MISA   # BASELINE.json north_star: "keeping the Model(config) constructor"
