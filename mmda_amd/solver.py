"""Solver with the reference's surface (reference src/solver.py:42-462): ``Solver(train_config, dev_config, test_config,
train_dl, dev_dl, test_dl, is_train, model)``, ``build()``, ``train()``, ``eval(mode)`` and the six ``get_*_loss``
getters - plus ``train_epoch()`` (the body of solver.py:127-197), which is what ``train()`` calls.

Two ways through a batch, same kernels underneath:
  * ``train_epoch()``           - fused native step (``MISA.train_step``): zero_grad, forward, six losses, backward,
                                  [RCCL gradient all-reduce], clip + Adam; losses are read back once per epoch.
  * ``train_epoch_unfused()``   - the reference's statement order verbatim (forward, six getters on the module's
                                  side-channel attributes, ``loss.backward()``, clip, ``optimizer.step()``) through autograd.
``train_epoch()`` and ``eval()`` also take loaders that yield ``EncodedBatch`` (``mmda_amd/encoded.py``: ``EncodedLoader`` over an
``EncoderCache``, which ``encode(mode)`` builds): steps that start behind the frozen encoders.
wandb / hypertune / tqdm / sklearn reports of the reference are logging only and are not reproduced.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import models, step_rules
from . import optim as _optim
from .dist import DataParallelSync
from .encoded import EncodedBatch, EncodedLoader, EncoderCache
from .utils import to_gpu, to_cpu, set_device
from .utils import functions as F


from .utils.eval import get_accuracy, get_metrics, DeviceEval      # reference utils/eval.py

DEV_TEST = ("dev", "test")                # the splits a report takes, and the splits a loader-wide pass (infer, encode) takes
SPLITS = ("train", "dev", "test")


class Solver(object):
    def __init__(self, train_config, dev_config, test_config, train_data_loader, dev_data_loader, test_data_loader,
                 is_train=True, model=None):
        self.train_config = train_config
        self.epoch_i = 0
        self.train_data_loader = train_data_loader
        self.dev_data_loader = dev_data_loader
        self.test_data_loader = test_data_loader
        self.is_train = is_train
        self.model = model
        if torch.cuda.is_available():
            self.device = torch.device(train_config.device)
        else:
            self.device = torch.device("cpu")
        set_device(self.device)
        self.dp = None
        self.loss_diff = F.DiffLoss()
        self.loss_cmd = F.CMD()

    # ------------------------------------------------------------------ build (solver.py:60-100)
    def build(self, cuda=True):
        cfg = self.train_config
        from .ranking import check_select_by
        check_select_by(getattr(cfg, "select_by", "valid_loss"),
                        process_group=torch.distributed.is_available() and torch.distributed.is_initialized())
        # what the sentiment task refuses (step_rules.SENTI_RULES), here rather than at the first batch or behind the last epoch
        step_rules.task_check(getattr(cfg, "task", "emotion"), getattr(cfg, "senti_loss", "l1"), num_classes=cfg.num_classes,
                              use_confidNet=bool(getattr(cfg, "use_confidNet", False)), pos_weight=getattr(cfg, "pos_weight", None),
                              focal_gamma=getattr(cfg, "focal_gamma", 0.0), calibrate=getattr(cfg, "calibrate", "none"),
                              select_by=getattr(cfg, "select_by", "valid_loss"))
        if getattr(cfg, "scaling", "none") not in ("none", "temperature", "platt"):
            raise ValueError(f"config.scaling must be 'none', 'temperature' or 'platt', not {cfg.scaling!r}")
        step_rules.scaling_check(getattr(cfg, "task", "emotion"), getattr(cfg, "scaling", "none"))
        if int(getattr(cfg, "bootstrap", 0) or 0) != 0:        # (0, the default: nothing is looked at)
            step_rules.bootstrap_check(task=getattr(cfg, "task", "emotion"), replicates=int(cfg.bootstrap))
        if int(getattr(cfg, "trust_k", 0) or 0) != 0:          # (0, the default: nothing is looked at)
            from .neighbours import check_trust_settings
            check_trust_settings(int(cfg.trust_k), float(getattr(cfg, "trust_alpha", 0.0) or 0.0), cfg.num_classes,
                                 getattr(cfg, "task", "emotion"))
        if self.model is None:
            self.model = getattr(models, cfg.model)(cfg)
        for name, param in self.model.named_parameters():
            if "weight_hh" in name:
                torch.nn.init.orthogonal_(param)
        if not getattr(cfg, "use_bert", False):
            if getattr(cfg, "pretrained_emb", None) is not None:
                self.model.embed.weight.data = cfg.pretrained_emb
            # (the reference writes `self.model.embed.requires_grad = False` here, solver.py:86: an attribute on the module that
            # freezes nothing.  Whether the table trains is config.embed_update: 'dense' (what the reference does), 'sparse', 'frozen')
        eu = getattr(self.model, "embed_update", "dense")
        opt_kwargs = dict(getattr(cfg, "optimizer_kwargs", None) or {})
        if cfg.optimizer is _optim.AdamW and "weight_decay" not in opt_kwargs:
            opt_kwargs["weight_decay"] = cfg.weight_decay
        clip_norm = getattr(cfg, "clip_norm", None)
        dp_on = torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1
        if self.is_train:
            # what no step does (step_rules.py), refused here rather than at the first batch.  An exchange: a process group of more than
            # one rank; for frozen parameters, any initialised process group
            kind, name = _optim.rule_kind(cfg.optimizer)
            step_rules.check(embed_update=eu, optimizer=kind, optimizer_name=name, weight_decay=float(opt_kwargs.get("weight_decay", 0) or 0),
                             clip_norm=clip_norm, exchange=dp_on, accumulate=int(getattr(cfg, "accum_steps", 1)) > 1)
            step_rules.check(frozen=bool(hasattr(self.model, "frozen_names") and self.model.frozen_names(beyond_embed_update=True)),
                             exchange=torch.distributed.is_available() and torch.distributed.is_initialized())
        self.model.to(self.device)
        self.cls_pos_weight = None
        if isinstance(getattr(cfg, "pos_weight", None), str):
            self.cls_pos_weight = self._balanced_pos_weight()
            self.model.set_cls_loss(self.cls_pos_weight, getattr(cfg, "focal_gamma", 0.0))
        if self.is_train:
            self.optimizer = cfg.optimizer([p for p in self.model.parameters() if p.requires_grad], lr=cfg.learning_rate, **opt_kwargs)
            if hasattr(self.optimizer, "attach"):
                self.optimizer.attach(self.model)
        if dp_on:
            # config.dp_global_stats (not a reference option: the reference is single-device): the batch-statistic losses on the
            # batch of all ranks instead of DDP semantics (mmda_amd/dist.py)
            self.dp = DataParallelSync(global_stats=bool(getattr(cfg, "dp_global_stats", False)))
            self.dp.broadcast_parameters(self.model)
        return self

    def _balanced_pos_weight(self):
        """config.pos_weight = "balanced": (N - n_c) / n_c per class from the training set's labels -- one launch over the label table
        where that is resident on the device (DeviceLoader, EncodedLoader), one host pass over ``loader.dataset`` otherwise."""
        from .data import DeviceLoader, class_pos_weight, host_labels
        cfg, loader = self.train_config, self.train_data_loader
        if cfg.pos_weight != "balanced":
            raise ValueError("config.pos_weight must be None, a list of num_classes floats or 'balanced'")
        if loader is None or (not isinstance(loader, EncodedLoader) and not hasattr(loader, "dataset")):
            raise ValueError("pos_weight='balanced' is resolved from the training set: the solver has no training loader with a dataset "
                             "(give the weights as a list, or mmda_amd.class_pos_weight(labels))")
        if isinstance(loader, DeviceLoader):
            labels = loader.dataset
        elif isinstance(loader, EncodedLoader):
            labels = loader.cache.emo
            if labels is None:
                raise ValueError("pos_weight='balanced': the encoder cache holds no emotion labels")
        else:
            labels = host_labels(loader.dataset)
        return [float(x) for x in class_pos_weight(labels)]

    def _sentiment(self):
        """the model's task is the sentiment regression (the step's target is the batch's ``y`` column, evaluation the sentiment table)"""
        return getattr(self.model, "task", "emotion") == "sentiment"

    def _cls_setting(self):
        """the model's classification criterion, as keyword arguments of bce_sum_over_classes / DeviceEval.add_cls_loss"""
        return dict(getattr(self.model, "cls_loss", None) or {})

    # ------------------------------------------------------------------ train (solver.py:103-307)
    def _micro_batches(self):
        """The loader's batches as (batch, accum_index, accum_count): optimizer steps of cfg.accum_steps consecutive batches each, the
        last one of an epoch of whatever is left (steps never straddle epochs).  A step's count must be known when its first
        micro-batch is issued, so the loader is read one step ahead; accum_steps = 1 reads it batch by batch as ever."""
        N = int(getattr(self.train_config, "accum_steps", 1))
        if N <= 1:
            for batch in self.train_data_loader:
                yield batch, 0, 1
            return
        group = []
        for batch in self.train_data_loader:
            group.append(batch)
            if len(group) == N:
                for k, b in enumerate(group):
                    yield b, k, N
                group = []
        for k, b in enumerate(group):
            yield b, k, len(group)

    def train_epoch(self):
        """Fused path.  Returns the epoch's mean losses (dict)."""
        cfg = self.train_config
        self.model.train()
        sums = None
        n = 0
        optimizer = getattr(self, "optimizer", None)
        clip_norm = getattr(cfg, "clip_norm", None)
        senti = self._sentiment()
        for batch, k, count in self._micro_batches():
            accum = dict(accum_index=k, accum_count=count) if count > 1 else {}
            if clip_norm is not None:
                accum["clip_norm"] = clip_norm
            # the optimizer's own lr: cfg.learning_rate as build() set it, until a torch.optim.lr_scheduler on self.optimizer or a
            # loaded checkpoint changes it
            lr = optimizer.param_groups[0]["lr"] if optimizer is not None else cfg.learning_rate
            step = dict(lr=lr, clip=cfg.clip, grad_sync=self.dp.sync if self.dp is not None else None,
                        optimizer=getattr(self, "optimizer", None), **accum)
            if isinstance(batch, EncodedBatch):                  # an index list into the encoder cache: the step gathers it
                self.model.train_step_encoded(batch, **step)
            else:
                t, v, a, y, emo_label, l, bert_sent, bert_sent_type, bert_sent_mask, ids = batch
                t = to_gpu(t); v = to_gpu(v); a = to_gpu(a); emo_label = to_gpu(y if senti else emo_label)
                l = to_cpu(l)
                self.model.train_step(t, v, a, l, emo_label, **step)
            L = self.model._ws_view("losses", (8,))
            sums = L.clone() if sums is None else sums + L       # stays on the device; one sync per epoch
            n += 1
        out = (sums / max(n, 1)).tolist() if sums is not None else [0.0] * 8
        # the read-back above synchronised anyway: a recurrence that gave up on its cluster invalidates the whole epoch
        self._check_cluster("train_epoch")
        return dict(cls=out[0], diff=out[1], sim=out[2], recon=out[3], conf=out[4], total=out[5])

    def train_epoch_unfused(self):
        """The reference's loop body, statement for statement (solver.py:138-193), through autograd."""
        cfg = self.train_config
        if int(getattr(cfg, "accum_steps", 1)) > 1:
            from . import _lib
            raise _lib.MMDAError("train_epoch_unfused() is the reference's loop, one optimizer step per batch: accum_steps > 1 runs "
                                 "through train_epoch()")
        if isinstance(self.train_data_loader, EncodedLoader):
            from . import _lib
            raise _lib.MMDAError("train_epoch_unfused() is the reference's loop through autograd, which a step from the encoder cache "
                                 "does not go through: an EncodedLoader runs through train_epoch()")
        self.model.train()
        train_loss = []
        for batch in self.train_data_loader:
            self.model.zero_grad()
            t, v, a, y, emo_label, l, bert_sent, bert_sent_type, bert_sent_mask, ids = batch
            t = to_gpu(t); v = to_gpu(v); a = to_gpu(a); y = to_gpu(y); emo_label = to_gpu(emo_label)
            l = to_cpu(l)
            predicted_scores, predicted_labels = self.model(t, v, a, l, bert_sent, bert_sent_type, bert_sent_mask)
            emo_label = (y if self._sentiment() else emo_label).type(torch.float)
            cls_loss = self.get_cls_loss(predicted_scores, emo_label)
            diff_loss = self.get_diff_loss()
            domain_loss = self.get_domain_loss()
            recon_loss = self.get_recon_loss()
            cmd_loss = self.get_cmd_loss()
            conf_loss = self.get_conf_loss(predicted_scores, emo_label) if cfg.use_confidNet or not self._sentiment() else 0.0
            similarity_loss = cmd_loss if cfg.use_cmd_sim else domain_loss
            loss = cls_loss + cfg.diff_weight * diff_loss + cfg.sim_weight * similarity_loss + cfg.recon_weight * recon_loss
            if cfg.use_confidNet:
                loss = loss + cfg.conf_weight * conf_loss
            loss.backward()
            if getattr(cfg, "clip_norm", None) is not None:
                _optim.clip_grad_norm_(self.model, cfg.clip_norm)
            _optim.clip_grad_value_(self.model, cfg.clip)
            self.optimizer.step()
            train_loss.append(loss.item())
        self._check_cluster("train_epoch_unfused")
        return dict(total=float(np.mean(train_loss)) if train_loss else 0.0)

    def _check_cluster(self, where):
        if hasattr(self.model, "check_cluster"):
            self.model.check_cluster(where)

    def _check_cluster_all_ranks(self, where):
        """Data parallel: every rank reads its own status, the ranks agree (one MAX all-reduce) and ALL of them raise -- a rank
        that raised alone would leave its peers waiting in the next collective."""
        if self.dp is None:
            return self._check_cluster(where)
        bad = bool(self.model.cluster_aborted()) if hasattr(self.model, "cluster_aborted") else False
        if self.dp.any_rank(bad):
            from . import _lib
            raise _lib.MMDAError(f"a resident-weights recurrence timed out waiting for its workgroup cluster on "
                                 f"{'this rank' if bad else 'another rank'} ({where}): results since then are invalid")

    def train(self):
        cfg = self.train_config
        best_valid_loss = float("inf")
        # config.select_by != "valid_loss": the best checkpoint is the one with the HIGHEST dev figure of Solver.rank (build() has
        # refused that under a process group); "valid_loss" takes none of these branches
        select_by = getattr(cfg, "select_by", "valid_loss")
        best_figure = float("-inf")
        best_epoch = -1
        history = []
        for e in range(cfg.n_epoch):
            self.epoch_i = e
            tr = self.train_epoch()
            print(f"Training loss: {round(tr['total'], 4)}")
            valid_loss, valid_acc, preds, truths = self.eval(mode="dev")
            print("-" * 100)
            print("Epochs: {}, Valid loss: {}, Valid acc: {}".format(e, valid_loss, valid_acc))
            print("-" * 100)
            if self._sentiment():
                self._print_sentiment()
            # Data parallel: whether this epoch is the best one is decided ONCE, from rank 0's dev loss (a sharded dev loader, or one
            # ULP of difference between ranks, must not send one rank into the checkpoint barrier and another into the next epoch's
            # all-reduce), and the cluster check in front of the save is collective, so an error is raised on every rank.
            extra = {}
            if select_by == "valid_loss":
                decided = self.dp.agree(valid_loss) if self.dp is not None else valid_loss
                is_best = decided <= best_valid_loss
                if is_best:
                    best_valid_loss = decided
            else:
                from .ranking import SELECT_BY
                figure = self.rank("dev", confidence=False)["scores"].as_dict()[SELECT_BY[select_by]]
                print(f"Valid {select_by}: {figure}")
                is_best = figure >= best_figure                 # a NaN (no class with both kinds of rows) is never the best
                if is_best:
                    best_figure = figure
                extra = {f"valid_{select_by}": figure}
            if is_best:
                best_epoch = e
                print("Found new best model on dev set!")
                self._check_cluster_all_ranks("before saving the checkpoint")  # never save weights a failed exchange produced
                if self.dp is None or self.dp.rank == 0:
                    os.makedirs("checkpoints", exist_ok=True)
                    torch.save(self.model.state_dict(), f"checkpoints/model_{cfg.name}.std")
                    torch.save(self.optimizer.state_dict(), f"checkpoints/optim_{cfg.name}.std")     # solver.py:220
            if self.dp is not None:
                torch.distributed.barrier()               # every epoch, on every rank: nobody reads the checkpoint before rank 0 has written it
            history.append(dict(epoch=e, train=tr, valid_loss=valid_loss, valid_acc=valid_acc, **extra))
        scaling = self._scale_after_training(best_epoch >= 0)
        thresholds = self._calibrate_after_training(best_epoch >= 0, scaling)
        test_loss, acc, _, _ = self.eval(mode="test", to_print=best_epoch >= 0, thresholds=thresholds, scaling=scaling)
        if self._sentiment():
            self._print_sentiment()
        if int(getattr(cfg, "mc_passes", 0) or 0) > 0:     # (0, the default: nothing below runs)
            if best_epoch >= 0:
                self._load_best_checkpoint()
            self.uncertainty("test", passes=int(cfg.mc_passes), to_print=True)
        if int(getattr(cfg, "trust_k", 0) or 0) > 0:       # (0, the default: nothing below runs)
            if best_epoch >= 0:
                self._load_best_checkpoint()
            self.trust("test", k=int(cfg.trust_k), alpha=float(getattr(cfg, "trust_alpha", 0.0) or 0.0), to_print=True)
        if int(getattr(cfg, "bootstrap", 0) or 0) > 0:    # (0, the default: nothing below runs)
            if best_epoch >= 0:
                self._load_best_checkpoint()
            self.bootstrap("test", replicates=int(cfg.bootstrap), thresholds=thresholds, scaling=scaling, to_print=True)
        print("=" * 50)
        print(f"Best epoch: {best_epoch}")
        print(f"Accuracy: {acc}")
        return history

    # ------------------------------------------------------------------ eval (solver.py:311-370; the passes: DESIGN.md 4s)
    def _load_best_checkpoint(self):
        path = f"checkpoints/model_{self.train_config.name}.std"
        if os.path.exists(path):
            self.model.load_state_dict(torch.load(path, weights_only=True))

    def _split(self, mode, among=None):
        """The ``mode`` split's loader.  ``among``: None -- ``eval``'s rule, anything but "dev" is the test split -- or the splits the
        caller takes (``DEV_TEST``, ``SPLITS``): any other mode is refused by name."""
        if among is None:
            return self.dev_data_loader if mode == "dev" else self.test_data_loader
        if mode not in among:
            raise ValueError(f"mode must be {', '.join(map(repr, among[:-1]))} or {among[-1]!r}, not {mode!r}")
        return getattr(self, f"{mode}_data_loader")

    def _begin_pass(self, mode, to_print):
        """An evaluation pass begins: the printed test pass runs on the best checkpoint, where there is one.  -> the split's loader"""
        if mode == "test" and to_print:
            self._load_best_checkpoint()
        return self._split(mode)

    def _keep(self, keep, dataloader):
        """A keep set (mmda_amd/modality.py) as its three bits, or None; refused by name over the encoder cache (step_rules.MODALITY_RULES)"""
        if keep is None:
            return None
        from .modality import parse_keep
        keep = parse_keep(keep)
        step_rules.modality_check(keep, encoded=isinstance(dataloader, EncodedLoader))
        return keep

    @staticmethod
    def _mask(t, v, a, keep):
        """the batch's inputs under a keep set: masked copies from one launch, the loader's tensors untouched (None: the inputs)"""
        if keep is None:
            return t, v, a
        from . import ops
        return ops.modality_mask(t.contiguous(), v.contiguous().float(), a.contiguous().float(), keep)

    def _eval_batches(self, dataloader, confidence=False, keep=None, scaling=None):
        """The one walk over an evaluation split: (scores, truth) of every batch, on the device, under ``model.eval()`` and ``no_grad``,
        one forward per batch; ``confidence=True``: (scores, truth, labels, tcp) -- the model's own decisions and ConfidNet's confidence
        in them.  ``truth`` is the batch's ``y`` column under the sentiment task and its emotion labels otherwise.  ``keep``: None or a
        keep set's three bits (``_keep``).  ``scaling``: None, or a ``Scaling``: the scores are its ``apply`` of the model's (one launch
        per batch); the decisions and ``tcp`` stay the model's own."""
        self.model.eval()
        with torch.no_grad():
            for batch in dataloader:
                if isinstance(batch, EncodedBatch):
                    predicted_scores, predicted_labels = self.model.forward_encoded(batch, keep=keep)
                    emo_label = batch.emo()
                else:
                    t, v, a, y, emo_label, l, bert_sent, bert_sent_type, bert_sent_mask, ids = batch
                    t = to_gpu(t); v = to_gpu(v); a = to_gpu(a); emo_label = to_gpu(y if self._sentiment() else emo_label)
                    t, v, a = self._mask(t, v, a, keep)
                    l = to_cpu(l)
                    predicted_scores, predicted_labels = self.model(t, v, a, l, bert_sent, bert_sent_type, bert_sent_mask)
                if scaling is not None:
                    predicted_scores = scaling.apply(predicted_scores)
                if confidence:
                    yield predicted_scores, emo_label.type(torch.float), predicted_labels, self.model.tcp
                else:
                    yield predicted_scores, emo_label.type(torch.float)

    def eval(self, mode=None, to_print=False, thresholds=None, keep=None, scaling=None):
        """``thresholds``: None -- the model's own labels (``scores > config.threshold``) -- or a ``Thresholds`` (mmda_amd/calibrate.py):
        labels and counts then come from ``scores > thresholds.values`` class by class, and the returned ``y_pred`` are those labels.
        ``keep``: None, or a keep set (an int 0 .. 7 or modality names, mmda_amd/modality.py): the split is evaluated with the other
        modalities blanked -- one ``mmda_modality_mask`` launch per batch in front of the forward; None is the plain pass.
        ``scaling``: None, or a ``Scaling`` (mmda_amd/reliability.py): the scores of every batch are scaled behind the forward pass (one
        ``mmda_scaling_apply`` launch), and labels, counts and the loss come from the scaled scores -- under ``thresholds``, or under
        ``config.threshold`` in every class without them."""
        assert mode is not None
        keep = self._keep(keep, self._split(mode))
        if self._sentiment():
            if thresholds is not None:
                step_rules.task_check("sentiment", self.model.senti_loss, calibrate="thresholds")
            if scaling is not None:
                step_rules.scaling_check("sentiment", scaling="Solver.eval")
            return self._eval_sentiment(mode, to_print, keep)
        return self._eval_emotion(mode, to_print, thresholds, keep, scaling)

    def _eval_emotion(self, mode, to_print, thresholds=None, keep=None, scaling=None):
        """``eval`` of the emotion labels.  Predictions, the per-batch classification loss and the metric counts stay on the GPU: one
        read-back at the end of the pass instead of three per batch (solver.py:350-360 calls .item()/.cpu() per batch).  Without
        ``thresholds`` and ``scaling`` the model's own labels are counted (``DeviceEval.update``); otherwise the labels are cut from the
        (scaled) scores in the launch that counts them (``DeviceEval.update_thr``; ``thresholds=None``: ``config.threshold`` in every
        class).  These are two launches and two label tensors, not one path with a default."""
        from . import _lib
        dataloader = self._begin_pass(mode, to_print)
        own = thresholds is None and scaling is None
        if own:
            thr = None
        elif thresholds is None:
            thr = torch.full((int(self.train_config.num_classes),), float(self.train_config.threshold), dtype=torch.float32,
                             device=self.device)
        else:
            thr = thresholds.values.to(device=self.device, dtype=torch.float32).contiguous()
        acc_dev = None
        y_true, y_pred = [], []
        for scores, emo_label, labels, _ in self._eval_batches(dataloader, confidence=True, keep=keep, scaling=scaling):
            if not scores.is_cuda:
                raise _lib.MMDAError(f"{'eval()' if own else 'eval(thresholds=...)'} counts on the GPU only (the HIP path has no CPU fallback)")
            if acc_dev is None:
                acc_dev = DeviceEval(scores.shape[1], scores.device)
            if own:
                acc_dev.update(labels, emo_label)
            else:
                labels = acc_dev.update_thr(scores, emo_label, thr)
            acc_dev.add_cls_loss(scores, emo_label, **self._cls_setting())
            y_pred.append(labels.detach())
            y_true.append(emo_label.detach())
        y_true = torch.cat(y_true, 0).cpu().numpy().squeeze() if y_true else np.zeros((0,))
        y_pred = torch.cat(y_pred, 0).cpu().numpy().squeeze() if y_pred else np.zeros((0,))
        self._check_cluster(f"eval({mode})")
        if acc_dev is None:
            self.last_eval_metrics = get_metrics(y_true, y_pred)
            return 0.0, get_accuracy(y_true, y_pred), y_pred, y_true
        loss, acc, self.last_eval_metrics = acc_dev.result()
        return loss, acc, y_pred, y_true

    # ------------------------------------------------------------------ the sentiment task (mmda_amd/sentiment.py)
    def _eval_sentiment(self, mode, to_print, keep=None):
        """``eval`` under task='sentiment': (mean batch loss, acc2_non0, preds (N,), truths (N,)).  Per batch one collector launch
        (``SentimentEval.update``) and one loss launch adding into a device sum (``SentimentEval.add_loss``), nothing read back until the
        pass is over.  ``self.last_sentiment``: the reference's eval_mosei_senti keys (and 'f1_non0'), all from the one collector state."""
        from . import _lib
        from .sentiment import SentimentEval
        dataloader = self._begin_pass(mode, to_print)
        ev = None
        preds, truths = [], []
        for scores, y in self._eval_batches(dataloader, keep=keep):
            if not scores.is_cuda:
                raise _lib.MMDAError("eval() under task='sentiment' counts on the GPU only (the HIP path has no CPU fallback)")
            s, t = scores.detach().to(torch.float32).contiguous().reshape(-1), y.contiguous().reshape(-1)
            if ev is None:
                ev = SentimentEval(s.device)
            ev.update(s, t)
            ev.add_loss(s, t, self.model.senti_loss)
            preds.append(s); truths.append(t)
        self._check_cluster(f"eval({mode})")
        if ev is None:
            self.last_sentiment = None
            return 0.0, float("nan"), np.zeros((0,), np.float32), np.zeros((0,), np.float32)
        self.last_sentiment = ev.as_dict()
        self.last_sentiment_counts = ev.counts()
        return ev.mean_loss(), self.last_sentiment["acc2_non0"], torch.cat(preds).cpu().numpy(), torch.cat(truths).cpu().numpy()

    def _print_sentiment(self):
        from .sentiment import format_table
        if getattr(self, "last_sentiment", None):
            c = self.last_sentiment_counts
            print(format_table(self.last_sentiment, c["n"], c["n_nonzero"]))

    # ------------------------------------------------------------------ threshold calibration (mmda_amd/calibrate.py)
    def calibrate(self, mode="dev", grid=None, objective=None, per_class=True, scaling=None):
        """Sweeps every cut-off of ``grid`` (default 0.01 .. 0.99) over the ``mode`` split in one pass -- ``_eval_batches`` with
        ``ThresholdSweep.update`` per batch -- and selects, on the device, the cut-off (``per_class=False``) or the
        cut-off per class that maximises ``objective`` ("f1", "micro_f1", "weighted_f1", "acc"; None: what ``config.eval_mode`` names).
        Sets and returns ``self.thresholds``; the sweep's table of the ten figures per cut-off is kept in ``self.last_calibration``.
        ``scaling``: None, or a ``Scaling``: the cut-offs are chosen on the scaled scores (``eval`` must then be given both)."""
        from .calibrate import ThresholdSweep, check_objective, objective_for
        if self._sentiment():
            step_rules.task_check("sentiment", self.model.senti_loss, calibrate="Solver.calibrate")
            if scaling is not None:
                step_rules.scaling_check("sentiment", scaling="Solver.calibrate")
        if objective is None:
            objective = objective_for(getattr(self.train_config, "eval_mode", "macro"), per_class)
        check_objective(objective, per_class)
        dataloader = self._split(mode, DEV_TEST)
        sweep = ThresholdSweep(int(self.train_config.num_classes), grid, self.device)
        for scores, emo_label in self._eval_batches(dataloader, scaling=scaling):
            sweep.update(scores, emo_label)
        self._check_cluster(f"calibrate({mode})")
        self.thresholds = sweep.select(objective, per_class)
        self.last_calibration = dict(table=sweep.table(), grid=sweep.grid, objective=objective, per_class=bool(per_class))
        return self.thresholds

    def _calibrate_after_training(self, have_checkpoint, scaling=None):
        """config.calibrate != "none": the best checkpoint's cut-offs from the dev split, saved by rank 0, for the final test pass."""
        how = getattr(self.train_config, "calibrate", "none")
        if how == "none":
            return None
        if how not in ("global", "per_class"):
            raise ValueError(f"config.calibrate must be 'none', 'global' or 'per_class', not {how!r}")
        if self.dp is not None and getattr(self.dev_data_loader, "shard", None) is not None:
            raise ValueError(f"calibrate={how!r} sweeps each rank's own dev loader and exchanges nothing: the dev loader must not be "
                             f"sharded (shard={self.dev_data_loader.shard}); give every rank the whole dev split or set calibrate='none'")
        if have_checkpoint:
            self._load_best_checkpoint()
        thresholds = self.calibrate("dev", per_class=how == "per_class", scaling=scaling)
        if self.dp is None or self.dp.rank == 0:
            os.makedirs("checkpoints", exist_ok=True)
            thresholds.save(f"checkpoints/thresholds_{self.train_config.name}.pt")
        return thresholds

    # ------------------------------------------------------------------ reliability and logit scaling (mmda_amd/reliability.py)
    def _score_tables(self, mode, who, confidence, scaling=None):
        """(scores, truth, labels, tcp or None) of the ``mode`` split, concatenated on the device: the one gather, behind
        ``rank``, ``reliability``, ``fit_scaling`` and ``bootstrap`` (``who``, for the messages).  ``tcp`` is None where it is not asked
        for (``confidence``) or the model has no confidence column per class."""
        from . import _lib
        dataloader = self._split(mode, DEV_TEST)
        S, T, L, Q = [], [], [], []
        for scores, emo_label, labels, tcp in self._eval_batches(dataloader, confidence=True, scaling=scaling):
            if not scores.is_cuda:
                raise _lib.MMDAError(f"{who}() counts on the GPU only (the HIP path has no CPU fallback)")
            S.append(scores.detach()); T.append(emo_label.detach()); L.append(labels.detach())
            Q.append(None if tcp is None else tcp.detach())
        self._check_cluster(f"{who}({mode})")
        if not S:
            raise ValueError(f"{who}({mode!r}): the {mode} loader yields no batch")
        tcp = torch.cat(Q, 0) if confidence and all(q is not None and q.shape == l.shape for q, l in zip(Q, L)) else None
        return torch.cat(S, 0), torch.cat(T, 0), torch.cat(L, 0), tcp

    def reliability(self, mode="dev", bins=15, scaling=None):
        """Whether the numbers of the ``mode`` split ("dev" or "test") are probabilities: ``{"scores": reliability_metrics(scores,
        truth), "confidence": reliability_metrics(tcp, labels == truth)}`` -- ``ReliabilityResult``s on the device, in the shape of
        ``rank``; ``confidence`` is None where the model has no confidence column per class.  ``scaling``: None, or a ``Scaling`` the
        scores pass through first (the model's decisions and ``tcp`` do not).  Sets and returns ``self.last_reliability``."""
        from .reliability import reliability_metrics
        if self._sentiment():
            step_rules.scaling_check("sentiment", reliability=True)
        scores, truth, labels, tcp = self._score_tables(mode, "reliability", True, scaling)
        out = {"scores": reliability_metrics(scores, truth, bins), "confidence": None}
        if tcp is not None:
            correct = (labels > 0) == (truth > 0)
            out["confidence"] = reliability_metrics(tcp, correct.to(torch.float32), bins)
        self.last_reliability = out
        return out

    def fit_scaling(self, mode="dev", how="temperature", per_class=False, max_iter=64):
        """Fits the logit scaling of the ``mode`` split's scores (``reliability.fit_scaling``: the iteration runs on the device, nothing
        is read back).  Sets and returns ``self.scaling``."""
        from .reliability import fit_scaling
        if self._sentiment():
            step_rules.scaling_check("sentiment", scaling=how)
        scores, truth, _, _ = self._score_tables(mode, "fit_scaling", False)
        self.scaling = fit_scaling(scores, truth, how=how, per_class=per_class, max_iter=max_iter)
        return self.scaling

    def _scale_after_training(self, have_checkpoint):
        """config.scaling != "none": the best checkpoint's logit scaling from the dev split, saved by rank 0, for the cut-offs of
        ``_calibrate_after_training`` and the final test pass."""
        how = getattr(self.train_config, "scaling", "none")
        if how == "none":
            return None
        if how not in ("temperature", "platt"):
            raise ValueError(f"config.scaling must be 'none', 'temperature' or 'platt', not {how!r}")
        if self.dp is not None and getattr(self.dev_data_loader, "shard", None) is not None:
            raise ValueError(f"scaling={how!r} fits on each rank's own dev loader and exchanges nothing: the dev loader must not be "
                             f"sharded (shard={self.dev_data_loader.shard}); give every rank the whole dev split or set scaling='none'")
        if have_checkpoint:
            self._load_best_checkpoint()
        scaling = self.fit_scaling("dev", how=how)
        if self.dp is None or self.dp.rank == 0:
            os.makedirs("checkpoints", exist_ok=True)
            scaling.save(f"checkpoints/scaling_{self.train_config.name}.pt")
        return scaling

    # ------------------------------------------------------------------ ranking metrics (mmda_amd/ranking.py)
    def rank(self, mode="dev", tpr=0.95, confidence=True):
        """How the model RANKS the ``mode`` split ("dev" or "test"), before any cut-off: ``_score_tables`` keeps scores, truth, the
        model's decisions and ``model.tcp`` of every batch on the device, then ``{"scores": ranking_metrics(scores, truth),
        "confidence": failure_prediction(tcp, labels == truth)}`` -- both ``RankingResult``s on the device; ``confidence`` is None
        where it is not asked for or the model has no confidence column per class.  Sets and returns ``self.last_ranking``.  Waits for
        nothing but the cluster check; reading a result back (``.cpu()``, ``.as_dict()``) is the caller's."""
        from .ranking import failure_prediction, ranking_metrics
        if self._sentiment():
            step_rules.task_check("sentiment", self.model.senti_loss, rank=True)
        scores, truth, labels, tcp = self._score_tables(mode, "rank", confidence)
        out = {"scores": ranking_metrics(scores, truth, tpr=tpr), "confidence": None}
        if tcp is not None:
            correct = (labels > 0) == (truth > 0)
            out["confidence"] = failure_prediction(tcp, correct.to(torch.float32), tpr=tpr)
        self.last_ranking = out
        return out

    # ------------------------------------------------------------------ inference (the reference's src/inference.py is a TODO)
    def infer(self, mode, fields=None, order="loader", keep=None):
        """One inference pass over the ``mode`` split ("train", "dev" or "test") -> ``InferenceResult`` (mmda_amd/inference.py): the
        per-sample tables stay on the device.  ``order="loader"``: the loader's own batches, rows in the order it yields samples.
        ``order="length"`` / ``"dataset"``: the loader must be a ``DeviceLoader``; its dataset is batched by ``inference_plan`` at the
        loader's batch size and row i is sample i of the dataset.  ``keep``: None, or a keep set (mmda_amd/modality.py) -- the pass
        runs with the other modalities blanked (``InferencePass.run`` / ``run_loader`` with that ``keep``)."""
        from .data import DeviceLoader
        from .inference import ORDERS, InferencePass
        loader = self._split(mode, SPLITS)
        if order != "loader" and order not in ORDERS:
            raise ValueError(f"order must be 'loader', 'length' or 'dataset', not {order!r}")
        if order != "loader" and not isinstance(loader, DeviceLoader):
            raise ValueError(f"order={order!r} re-batches a device-resident dataset: the {mode} loader must be a DeviceLoader "
                             f"(it is a {type(loader).__name__}); use order='loader'")
        p = InferencePass(self.model, fields) if fields is not None else InferencePass(self.model)
        keep = self._keep(keep, loader)
        if order == "loader":
            return p.run_loader(loader, keep=keep)
        return p.run(loader.dataset, loader.batch_size, order, keep=keep)

    # ------------------------------------------------------------------ modality attribution (mmda_amd/modality.py)
    def modalities(self, mode="dev", values=None, to_print=False):
        """The ``mode`` split ("dev" or "test") under all eight keep sets -> ``ModalityResult``, kept in ``self.last_modalities``: what
        the model scores, and how confident ConfidNet is, with every subset of {text, visual, acoustic} blanked; its ``attribution``
        gives each modality's exact Shapley value per sample and class.  ``values``: None -- ("scores", "tcp"), under task='sentiment'
        ("scores",) -- or a subset.  Over a ``DeviceLoader`` the pass is ``ModalityPass.run`` on its dataset at its batch size: eight
        masked gathers per batch, row i = sample i.  Any other loader of the reference's tuples is walked eight times
        (``ModalityPass.run_loader``: ``InferencePass.run_loader(loader, keep=k)`` for k = 0 .. 7), which is slower -- every batch is
        copied once more by the mask launch and the loader's own work is done eight times -- but gives the same tables, rows in the
        loader's order.  A loader over the encoder cache is refused by name.  ``to_print``: one table, per keep set acc / F1 / mean
        tcp and per class the mean Shapley value of each modality (read back for the print)."""
        from .data import DeviceLoader
        from .modality import ModalityPass, format_table
        loader = self._split(mode, DEV_TEST)
        step_rules.modality_check(0, encoded=isinstance(loader, EncodedLoader))
        if values is None:
            values = ("scores",) if self._sentiment() else ("scores", "tcp")
        p = ModalityPass(self.model, values)
        res = p.run(loader.dataset, loader.batch_size) if isinstance(loader, DeviceLoader) else p.run_loader(loader)
        self.last_modalities = res
        if to_print:
            metrics = None if self._sentiment() or res.truth is None or res.scores is None else res.metrics()
            which = "scores" if res.scores is not None else "tcp"
            phi = res.attribution(which)["phi"].mean(dim=0).cpu().numpy()
            tcp = None if res.tcp is None else res.tcp.mean(dim=(1, 2)).cpu().numpy()
            print(format_table(metrics, tcp, phi))
        return res

    # ------------------------------------------------------------------ MC-dropout uncertainty (mmda_amd/uncertainty.py)
    def uncertainty(self, mode="dev", passes=None, to_print=False, seed=0, columns=256):
        """MC dropout over the ``mode`` split ("dev" or "test") -> ``MCDropoutResult``, on the device: ``passes`` draws per sample
        (None: ``config.mc_passes``, or 32 where that is 0) from one forward of the fusion block per chunk.  A ``DeviceLoader``'s
        dataset is used as it is, an ``EncodedLoader``'s cache goes through ``run_cache``, and any other loader's ``dataset`` of the
        reference's samples is uploaded once (``DeviceDataset.from_samples``).  ``self.last_uncertainty``: per kind of confidence --
        maximum class probability, the MC-dropout figures and, with ConfidNet, ``tcp`` and its mean over the draws -- the macro
        AUROC, AUPR-Success, AUPR-Error and FPR@95TPR of "does it rank the right decisions above the wrong ones", every kind against
        the same deterministic decisions (this read-back and the cluster check are the call's waits; the pass itself has none).
        ``to_print``: that table."""
        from .data import DeviceDataset, DeviceLoader
        from .uncertainty import KINDS, MCDropoutPass, check_settings
        loader = self._split(mode, DEV_TEST)
        cfg = self.train_config
        if passes is None:
            passes = int(getattr(cfg, "mc_passes", 0) or 0) or 32
        check_settings(passes, columns, getattr(cfg, "task", "emotion"))
        p = MCDropoutPass(self.model, passes=passes, seed=seed, columns=columns)
        if isinstance(loader, EncodedLoader):
            res, truth = p.run_cache(loader.cache), loader.cache.emo
        else:
            ds = loader.dataset if isinstance(loader, DeviceLoader) else None
            if ds is None:
                src = getattr(loader, "dataset", None)
                if src is None or src is loader or not hasattr(src, "__len__"):
                    raise ValueError(f"uncertainty({mode!r}) re-batches the split's samples: the {mode} loader must be a DeviceLoader, an "
                                     f"EncodedLoader or have a `dataset` of the reference's samples (it is a {type(loader).__name__})")
                ds = DeviceDataset.from_samples([src[i] for i in range(len(src))], next(self.model.parameters()).device)
            res, truth = p.run(ds, getattr(loader, "batch_size", None) or cfg.batch_size), ds.emo
        self._check_cluster(f"uncertainty({mode})")
        self.last_uncertainty = None
        if truth is not None and truth.shape == res.labels.shape:
            kinds = tuple(k for k in KINDS if not k.startswith("tcp") or
                          (bool(getattr(cfg, "use_confidNet", False)) and res.tcp.shape == res.labels.shape))
            table = {}
            for k, fp in res.failure_table(truth, kinds).items():
                d = fp.as_dict()
                table[k] = dict(auroc=d["macro_auroc"], aupr_success=d["macro_aupr_success"], aupr_error=d["macro_aupr_error"],
                                fpr_at_95tpr=d["macro_fpr_at_95tpr"])
            self.last_uncertainty = table
            if to_print:
                print(f"failure prediction on the {mode} split, {res.passes} MC-dropout draws per sample (macro over classes)")
                print(f"{'confidence':<12} {'AUROC':>8} {'AUPR-Succ':>10} {'AUPR-Err':>9} {'FPR@95TPR':>10}")
                for k, r in table.items():
                    print(f"{k:<12} {r['auroc']:8.4f} {r['aupr_success']:10.4f} {r['aupr_error']:9.4f} {r['fpr_at_95tpr']:10.4f}")
        return res

    # ------------------------------------------------------------------ Trust Score (mmda_amd/neighbours.py)
    def _sample_tables(self, mode, fields, who):
        """(``InferenceResult`` with ``fields``, truth (n, C) on the device) of the ``mode`` split ("train", "dev" or "test"), row i of
        both the same sample.  A ``DeviceLoader``'s dataset is walked as it is (``InferencePass.run``: row i = sample i, whatever the
        loader shuffles or masks); a loader with a ``dataset`` of the reference's samples has it uploaded once
        (``DeviceDataset.from_samples``) and walked the same way; a plain list of the reference's tuples, or a stand-in whose
        ``dataset`` is itself, is walked by ``InferencePass.run_loader`` and once more for the tuples' emotion labels, so it must yield
        the same batches twice.  A loader over the encoder cache is refused by name."""
        from .data import DeviceDataset, DeviceLoader
        from .inference import InferencePass
        loader = self._split(mode, SPLITS)
        if isinstance(loader, EncodedLoader):
            raise ValueError(f"{who}({mode!r}) reads the hidden vectors of the split's samples: the {mode} loader must not be an "
                             f"EncodedLoader (the encoder cache holds utterance rows, not samples)")
        p = InferencePass(self.model, fields)
        ds = loader.dataset if isinstance(loader, DeviceLoader) else None
        src = getattr(loader, "dataset", None)
        if ds is None and src is not None and src is not loader and hasattr(src, "__len__") and hasattr(src, "__getitem__"):
            ds = DeviceDataset.from_samples([src[i] for i in range(len(src))], next(self.model.parameters()).device)
        if ds is not None:
            return p.run(ds, getattr(loader, "batch_size", None) or self.train_config.batch_size), ds.emo
        res = p.run_loader(loader)
        truth = [torch.as_tensor(batch[4]) for batch in loader]
        if not truth:
            raise ValueError(f"{who}({mode!r}): the {mode} loader yields no batch")
        return res, torch.cat(truth, 0).to(res._flat.device)

    def trust(self, mode="dev", k=10, alpha=0.0, fit="train", to_print=False, bootstrap=None):
        """The Trust Score of the ``mode`` split's decisions ("dev" or "test") against the ``fit`` split ("train", "dev" or "test") ->
        ``TrustResult``, on the device: one ``InferencePass`` over ``fit`` for its hidden vectors, one over ``mode`` (scores, decisions,
        ``tcp``, hidden vectors), ``TrustIndex.fit(hidden, truth, k, alpha)`` and ``.score``.  The splits are taken the way
        ``uncertainty`` takes them (a ``DeviceLoader``'s dataset as it is, any other loader's ``dataset`` uploaded once), row i = sample
        i.  ``self.last_trust``: per kind of confidence -- ``mcp``, ``trust`` and, with ConfidNet, ``tcp`` -- the macro AUROC,
        AUPR-Success, AUPR-Error and FPR@95TPR of "does it rank the right decisions above the wrong ones", every kind against the same
        deterministic decisions (this read-back and the cluster check are the call's waits).  ``bootstrap``: None, or a ``Bootstrap``
        over the split's rows -- ``self.last_trust_bootstrap`` is then ``TrustResult.failure_table(..., bootstrap=bootstrap)``: per
        kind the resampled figures, their intervals and the paired ``vs_tcp`` difference.  ``to_print``: the table."""
        from .neighbours import TrustIndex, check_trust_settings
        cfg = self.train_config
        self._split(mode, DEV_TEST)
        self._split(fit, SPLITS)
        check_trust_settings(k, alpha, cfg.num_classes, getattr(cfg, "task", "emotion"))
        base, fit_truth = self._sample_tables(fit, ("hidden",), "trust")
        res, truth = self._sample_tables(mode, ("scores", "labels", "tcp", "hidden"), "trust")
        self._check_cluster(f"trust({mode})")
        if fit_truth is None or truth is None or truth.shape != res.labels.shape or fit_truth.shape[0] != base.hidden.shape[0]:
            raise ValueError(f"trust({mode!r}, fit={fit!r}) needs the emotion labels of both splits")
        index = TrustIndex.fit(base.hidden, fit_truth.to(base.hidden.device), k=k, alpha=alpha)
        out = index.score(res.hidden, res.labels)
        others = {"mcp": torch.maximum(res.scores, 1.0 - res.scores)}
        if bool(getattr(cfg, "use_confidNet", False)) and res.tcp.shape == res.labels.shape:
            others["tcp"] = res.tcp
        table = {}
        for kind, fp in out.failure_table(truth, others).items():
            d = fp.as_dict()
            table[kind] = dict(auroc=d["macro_auroc"], aupr_success=d["macro_aupr_success"], aupr_error=d["macro_aupr_error"],
                               fpr_at_95tpr=d["macro_fpr_at_95tpr"])
        self.last_trust = {kind: table[kind] for kind in ("mcp", "trust", "tcp") if kind in table}
        self.last_trust_bootstrap = None if bootstrap is None else out.failure_table(truth, others, bootstrap=bootstrap)
        if to_print:
            print(f"failure prediction on the {mode} split, Trust Score against the {fit} split (k = {int(k)}, alpha = {float(alpha):g}; "
                  f"macro over classes)")
            print(f"{'confidence':<12} {'AUROC':>8} {'AUPR-Succ':>10} {'AUPR-Err':>9} {'FPR@95TPR':>10}")
            for kind, r in self.last_trust.items():
                print(f"{kind:<12} {r['auroc']:8.4f} {r['aupr_success']:10.4f} {r['aupr_error']:9.4f} {r['fpr_at_95tpr']:10.4f}")
        return out

    # ------------------------------------------------------------------ bootstrap intervals (mmda_amd/bootstrap.py)
    def bootstrap(self, mode="test", replicates=2000, seed=0, alpha=0.05, thresholds=None, scaling=None, confidence=True, to_print=False):
        """How far the figures of the ``mode`` split ("dev" or "test") would move on another draw of it: the split is gathered once
        (``_score_tables``) and resampled ``replicates`` times on the device.  Sets and returns ``self.last_bootstrap``:
        ``metrics`` -- the cut-off figures of ``eval`` under the same ``thresholds`` / ``scaling`` (the model's own decisions where
        both are None) --, ``ranking`` (``rank``'s score table), ``confidence`` (its failure-prediction table, None where the model has
        no confidence column per class or it is not asked for) and, with ``thresholds``, ``vs_default``: the paired comparison of those
        cut-offs against ``config.threshold`` in every class, same resamples on both sides.  The first three are ``BootstrapResult``s
        (``summary(alpha)`` gives point, mean, std, lo, hi), kept on the device; ``summaries`` holds their ``BootstrapSummary``s at
        ``alpha``.  ``to_print``: ``figure  point  [lo, hi]`` for the ten cut-off figures and the macro ranking figures."""
        from .bootstrap import Bootstrap
        from .utils.eval import KEYS
        cfg = self.train_config
        sharded = getattr(self._split(mode), "shard", None) if self.dp is not None else None
        step_rules.bootstrap_check(task="sentiment" if self._sentiment() else "emotion", replicates=replicates, sharded=sharded, mode=mode)
        scores, truth, labels, tcp = self._score_tables(mode, "bootstrap", confidence, scaling)
        n, C = int(scores.shape[0]), int(scores.shape[1])
        bs = Bootstrap(n, replicates, seed, scores.device)
        s32 = scores.to(torch.float32)
        cut = lambda thr: (s32 > thr.to(device=s32.device, dtype=torch.float32).reshape(1, -1)).to(torch.float32)
        default_thr = torch.full((C,), float(cfg.threshold), dtype=torch.float32)
        if thresholds is not None:
            if thresholds.values.numel() != C:
                raise ValueError(f"thresholds has {thresholds.values.numel()} entries, the model {C} classes")
            decided = cut(thresholds.values)
        else:
            decided = labels if scaling is None else cut(default_thr)
        out = dict(bootstrap=bs, alpha=float(alpha), metrics=bs.decisions(decided, truth), ranking=bs.ranking(scores, truth),
                   confidence=None, vs_default=None)
        if tcp is not None:
            correct = ((labels > 0) == (truth > 0)).to(torch.float32)
            out["confidence"] = bs.ranking(tcp, correct, failure=True)
        if thresholds is not None:
            out["vs_default"] = bs.compare(out["metrics"], bs.decisions(cut(default_thr), truth), alpha)
        out["summaries"] = {k: out[k].summary(alpha) for k in ("metrics", "ranking", "confidence") if out[k] is not None}
        self.last_bootstrap = out
        if to_print:
            print(f"bootstrap of the {mode} split: {n} rows, {replicates} replicates, {100 * (1 - alpha):g} % percentile intervals")
            print(out["summaries"]["metrics"].format(KEYS))
            print(out["summaries"]["ranking"].format(("macro_auroc", "map", "macro_ap_neg", "macro_fpr_at_tpr")))
            if out["confidence"] is not None:
                names = out["confidence"].names[-4:]
                print("failure prediction (tcp)")
                print(out["summaries"]["confidence"].format(names))
            if out["vs_default"] is not None:
                print(f"calibrated cut-offs minus threshold = {cfg.threshold}")
                print(out["vs_default"].format(KEYS))
        return out

    # ------------------------------------------------------------------ encoder cache (mmda_amd/encoded.py)
    def encode(self, mode, batch_size=None, order="length"):
        """The ``EncoderCache`` of the ``mode`` split ("train", "dev" or "test"), whose loader must be a ``DeviceLoader``: one evaluation
        pass over its dataset at ``batch_size`` (default: the loader's).  Wrap it in an ``EncodedLoader`` and hand that to the solver
        in the split's place to train, or evaluate, from the stored encoder outputs."""
        from .data import DeviceLoader
        loader = self._split(mode, SPLITS)
        if not isinstance(loader, DeviceLoader):
            raise ValueError(f"encode({mode!r}) reads a device-resident dataset: the {mode} loader must be a DeviceLoader "
                             f"(it is a {type(loader).__name__})")
        return EncoderCache.build(self.model, loader.dataset, loader.batch_size if batch_size is None else batch_size, order)

    # ------------------------------------------------------------------ getters (solver.py:373-462)
    def get_cls_loss(self, predicted_scores, emo_label):
        if self._sentiment():                             # the task's criterion against the sentiment column
            return F.senti_loss(predicted_scores, emo_label.type(torch.float), self.model.senti_loss)
        return F.bce_sum_over_classes(predicted_scores, emo_label.type(torch.float), **self._cls_setting())

    def get_domain_loss(self):
        if self.train_config.use_cmd_sim:
            return 0.0
        m = self.model
        return F.domain_loss(m.domain_label_t, m.domain_label_v, m.domain_label_a)

    def get_cmd_loss(self):
        if not self.train_config.use_cmd_sim:
            return 0.0
        m = self.model
        # (t,v) + (t,a) + (a,v), /3  - one fused launch instead of three CMD() calls
        return F.cmd_loss_multi([m.utt_shared_t, m.utt_shared_v, m.utt_shared_a], [(0, 1), (0, 2), (2, 1)], 5, 1.0 / 3.0)

    def get_diff_loss(self):
        m = self.model
        ts = [m.utt_private_t, m.utt_private_v, m.utt_private_a, m.utt_shared_t, m.utt_shared_v, m.utt_shared_a]
        # (p_t,s_t) (p_v,s_v) (p_a,s_a) (p_a,p_t) (p_a,p_v) (p_t,p_v)   solver.py:432-439
        return F.diff_loss_multi(ts, [(0, 3), (1, 4), (2, 5), (2, 0), (2, 1), (0, 1)])

    def get_recon_loss(self):
        m = self.model
        return F.recon_loss([m.utt_t_recon, m.utt_v_recon, m.utt_a_recon], [m.utt_t_orig, m.utt_v_orig, m.utt_a_orig])

    def get_conf_loss(self, pred, truth):
        return F.conf_loss(pred, self.model.tcp, truth)
