"""Optimizers.  ``Adam`` / ``RMSprop`` keep the torch.optim constructors (the reference builds its optimizer as
``config.optimizer(params, lr=...)`` out of ``optimizer_dict = {'RMSprop', 'Adam'}``, config.py:24, solver.py:97-99) but step
with the fused HIP clamp+update kernels.  ``Adam`` takes torch's ``betas``, ``eps`` and ``weight_decay`` (L2, or decoupled with
``decoupled_weight_decay=True``); ``AdamW`` is that with torch.optim.AdamW's defaults.  What the optimizer was constructed with is what
steps, on the fused path (``MISA.train_step(optimizer=...)``) as through ``step()``.  ``clip_grad_norm_`` is
torch.nn.utils.clip_grad_norm_ on the flat gradient bucket, without a read-back.

When every parameter is a view into one flat bucket whose gradient/moment buckets are laid out identically (that is
how mmda_amd.models.MISA allocates them) the whole model is ONE kernel launch; otherwise one launch per tensor.
``state_dict()`` / ``load_state_dict()`` of an attached optimizer carry the flat moment buckets and the step count, so a
run can be resumed from ``checkpoints/optim_{name}.std`` (solver.py:220 saves it beside the model).
"""
from __future__ import annotations

import torch

from . import _lib, step_rules


def rule_kind(optimizer):
    """(kind, class name) of an optimizer, an optimizer class or None, as step_rules takes them"""
    if optimizer is None:
        return None, ""
    cls = optimizer if isinstance(optimizer, type) else type(optimizer)
    return ("adam" if issubclass(cls, Adam) else "other"), cls.__name__


def clamp_adam(lib, p, g, m, v, n, runs, lr, clip, grad_scale, step, settings, scale_dev, stream, what):
    """One clamp + Adam launch over n floats, or over ``runs`` = (table, n_runs, items), with ``settings`` = (beta1, beta2, eps, weight_decay,
    decoupled).  Always mmda_clamp_adam_opts: without decay and device scale it launches what the plain entries launch (mmda_hip.h)."""
    b1, b2, eps, wd, dec = settings[:5]
    table, n_runs, items = runs if runs is not None else (None, 0, 0)
    opts = _lib.AdamOpts(beta1=b1, beta2=b2, eps=eps, weight_decay=wd, decoupled=int(dec), scale_dev=_lib.ptr(scale_dev))
    _lib.check(lib.mmda_clamp_adam_opts(p, None, g, m, v, n, _lib.ptr(table), n_runs, items, lr, clip, grad_scale, step,
                                        _lib.C.byref(opts), stream), what)


class _FlatOptimizer(torch.optim.Optimizer):
    """Shared plumbing: binding to a MISA model's flat buckets, the step counter, (de)serialisation of the flat state."""

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        self._model = None
        self._t = 0

    def attach(self, model):
        """Bind to a MISA model so the step is one fused launch over its flat buckets (and shares the model's step counter
        with the native fused train step)."""
        self._model = model
        return self

    def _flat(self):
        m = self._model
        if m is not None and m._P is not None and m._views_valid():
            return m
        return None

    def _next_step(self) -> int:
        m = self._model
        if m is not None:
            m._step += 1
            self._t = m._step
        else:
            self._t += 1
        return self._t

    # ---- checkpointing (solver.py:220: torch.save(self.optimizer.state_dict(), 'checkpoints/optim_{name}.std'))
    def _flat_state(self):
        return {}

    def _load_flat_state(self, st):
        pass

    def state_dict(self):
        m = self._flat()
        if m is None:
            return super().state_dict()
        if hasattr(m, "flush_embedding"):
            m.flush_embedding()                             # embed_update 'deferred': the moment buckets hold current rows
        groups = [{k: v for k, v in g.items() if k != "params"} for g in self.param_groups]
        # the moment buckets are raw images of the flat bucket: its (name, offset, shape) layout travels with them, so that a checkpoint
        # written under another bucket order (another configuration or build) is re-ordered by name on load instead of loading wrongly
        layout = [[k, int(off), [int(x) for x in shape]] for k, (off, shape) in m._layout.items()]
        out = {"mmda_flat": 2, "step": int(m._step), "param_groups": groups, "layout": layout}
        out.update({k: v.detach().cpu().clone() for k, v in self._flat_state().items()})
        return out

    def load_state_dict(self, sd):
        m = self._flat()
        if m is None or getattr(m, "embed_update", "dense") != "deferred":
            return self._load_state_dict(sd, m)
        # embed_update 'deferred': the table takes the steps it is behind under the moments it has; the loaded moments, and the loaded
        # step count, then find every row current
        m.flush_embedding()
        out = self._load_state_dict(sd, m)
        m._bind_deferred()
        return out

    def _load_state_dict(self, sd, m):
        if not (isinstance(sd, dict) and sd.get("mmda_flat")):
            if m is not None:
                # a torch-format state (the reference writes one, solver.py:220): the attached fused step never reads self.state, so
                # the moments would be dropped silently -- scatter them into the flat buckets by parameter order instead
                return self._load_torch_state(sd, m)
            return super().load_state_dict(sd)
        if m is None:
            raise _lib.MMDAError("load_state_dict of a flat optimizer state needs the optimizer attached to a MISA model on the GPU")
        for g, saved in zip(self.param_groups, sd["param_groups"]):
            g.update(saved)
        m._step = int(sd["step"]); self._t = m._step
        mine = {k: (int(off), tuple(int(x) for x in shape)) for k, (off, shape) in m._layout.items()}
        saved = sd.get("layout")
        if saved is None:                                   # version 1: no layout recorded -- only safe when nothing else can differ
            for v in self._flat_state().values():
                for k, t in sd.items():
                    if torch.is_tensor(t) and t.numel() != v.numel():
                        raise _lib.MMDAError("flat optimizer state of another size (and without a layout map): cannot be loaded")
            return self._load_flat_state(sd)
        theirs = {k: (int(off), tuple(shape)) for k, off, shape in saved}
        if theirs == mine:
            return self._load_flat_state(sd)
        if set(theirs) != set(mine) or any(theirs[k][1] != mine[k][1] for k in mine):
            raise _lib.MMDAError("flat optimizer state belongs to a model with other parameters / shapes")
        # same parameters, another bucket order: move every tensor's moments to its offset here
        remapped = {}
        for name, img in sd.items():
            if not torch.is_tensor(img) or name not in self._flat_state():
                continue
            out = torch.zeros_like(img)
            for k, (off, shape) in mine.items():
                n = 1
                for x in shape:
                    n *= x
                o2 = theirs[k][0]
                out[off:off + n] = img[o2:o2 + n]
            remapped[name] = out
        self._load_flat_state(dict(sd, **remapped))

    def _load_torch_state(self, sd, m):
        names = [k for k, _ in m.named_parameters()]
        params = [p for g in self.param_groups for p in g["params"]]
        if len(sd.get("param_groups", [{}])[0].get("params", [])) != len(params):
            raise _lib.MMDAError("torch-format optimizer state with another number of parameters")
        by_id = {id(p): k for k, p in m.named_parameters()}
        flat = self._flat_state()
        keymap = {"exp_avg": "exp_avg", "exp_avg_sq": "exp_avg_sq", "square_avg": "square_avg"}
        step = 0
        for idx, p in zip(sd["param_groups"][0]["params"], params):
            st = sd["state"].get(idx)
            if not st:
                continue
            off, shape = m._layout[by_id[id(p)]]
            for src, dst in keymap.items():
                if src in st and dst in flat:
                    flat[dst][off:off + p.numel()].copy_(st[src].reshape(-1).to(flat[dst].device))
            step = max(step, int(st.get("step", 0)))
        for g, saved in zip(self.param_groups, sd["param_groups"]):
            g.update({k: v for k, v in saved.items() if k != "params"})
        m._step = step; self._t = step
        del names


class Adam(_FlatOptimizer):
    """torch.optim.Adam's constructor (no amsgrad).  ``weight_decay``: L2, added to the clipped gradient as torch.optim.Adam does, or
    -- ``decoupled_weight_decay=True`` -- torch.optim.AdamW's ``p -= lr * weight_decay * p``.  Attached to a model the bucket is one
    param group: per-tensor decay exclusions are not built.  With ``embed_update='sparse'`` the decay covers the dense prefix; the
    table's rows follow SparseAdam, which has none."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, clip_value=None, decoupled_weight_decay=False):
        b1, b2 = betas
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ValueError(f"betas must lie in [0, 1): {betas}")
        if not eps >= 0.0:
            raise ValueError(f"eps must be >= 0: {eps}")
        if not weight_decay >= 0.0:
            raise ValueError(f"weight_decay must be >= 0: {weight_decay}")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                      decoupled_weight_decay=bool(decoupled_weight_decay), clip_value=clip_value))

    def settings(self):
        """(beta1, beta2, eps, weight_decay, decoupled) of the one param group an attached optimizer may have"""
        if self._model is not None and len(self.param_groups) != 1:
            raise _lib.MMDAError(f"{type(self).__name__} attached to a MISA model has {len(self.param_groups)} param groups: the flat bucket "
                                 "is one group (per-tensor settings such as decay exclusions are not built)")
        g0 = self.param_groups[0]
        b1, b2 = g0["betas"]
        return (float(b1), float(b2), float(g0["eps"]), float(g0.get("weight_decay", 0.0)), bool(g0.get("decoupled_weight_decay", False)))

    def add_param_group(self, param_group):
        if getattr(self, "_model", None) is not None and len(self.param_groups) >= 1:
            raise _lib.MMDAError(f"{type(self).__name__} is attached to a MISA model: a second param group is not built (the flat bucket "
                                 "is one group)")
        return super().add_param_group(param_group)

    def _flat_state(self):
        _, _, M, V = self._model.flat_buckets()
        return {"exp_avg": M, "exp_avg_sq": V}

    def _load_flat_state(self, sd):
        _, _, M, V = self._model.flat_buckets()
        M.copy_(sd["exp_avg"].to(M.device)); V.copy_(sd["exp_avg_sq"].to(V.device))

    @torch.no_grad()
    def step(self, closure=None, clip_value=None, grad_scale=1.0, scale_dev=None):
        """``scale_dev``: a one-element device tensor that multiplies ``grad_scale`` inside the launch (a clip coefficient that the
        host never reads), or None."""
        lib = _lib.load()
        cfg = self.settings()
        g0 = self.param_groups[0]
        m = self._flat()
        if m is not None and hasattr(m, "_push_adam"):
            # the native side replays a deferred table's rows with the handle's betas and eps: they are this optimizer's (and what no
            # step does is refused here, by name, before the step is counted)
            m._push_adam(self, m._adam_pushed[5])
        t = self._next_step()
        s = _lib.stream_ptr()
        clip = clip_value if clip_value is not None else g0["clip_value"]
        clip = float("inf") if clip is None else float(clip)
        b1, b2 = g0["betas"]
        if m is not None:
            P, G, M, V = m.flat_buckets()
            # embed_update 'sparse' / 'frozen': the dense launch ends in front of embed.weight; 'sparse' then updates the rows the last
            # backward touched, clamped by what clip_grad_value_ recorded for them (the unfused order clips before it steps)
            n = getattr(m, "grad_floats", P.numel())
            # frozen parameters (requires_grad=False): the same update over the trainable runs of the bucket only
            runs = m._trainable_runs() if hasattr(m, "_trainable_runs") else None
            clamp_adam(lib, P.data_ptr(), G.data_ptr(), M.data_ptr(), V.data_ptr(), n, runs, g0["lr"], clip, grad_scale, t, cfg, scale_dev,
                       s, "mmda_clamp_adam_runs" if runs is not None else "mmda_clamp_adam")
            if getattr(m, "embed_update", "dense") == "sparse":
                rows_clip = clip if m._rows_clip is None else min(clip, float(m._rows_clip))
                m.apply_sparse_rows(g0["lr"], t, rows_clip, grad_scale, betas=(b1, b2), eps=g0["eps"])
            elif getattr(m, "embed_update", "dense") == "deferred":
                # dense Adam's step for the rows of the last backward (two clamps in a row are one clamp at the smaller value)
                rows_clip = clip if m._rows_clip is None else min(clip, float(m._rows_clip))
                m.apply_deferred_rows(g0["lr"], t, rows_clip, grad_scale, betas=(b1, b2), eps=g0["eps"])
            return None
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.device.type != "cuda":
                    raise _lib.MMDAError("mmda_amd.optim.Adam steps on the GPU only")
                st = self.state[p]
                if not st:
                    st["m"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["v"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                g = p.grad.contiguous()
                ok = all(x.data_ptr() % 16 == 0 for x in (p, g, st["m"], st["v"])) and p.is_contiguous()
                if not ok:
                    raise _lib.MMDAError("parameter storage is not 16-byte aligned/contiguous")
                gb1, gb2 = group["betas"]
                gst = (float(gb1), float(gb2), float(group["eps"]), float(group.get("weight_decay", 0.0)),
                       bool(group.get("decoupled_weight_decay", False)))
                clamp_adam(lib, p.data_ptr(), g.data_ptr(), st["m"].data_ptr(), st["v"].data_ptr(), p.numel(), None, group["lr"], clip,
                           grad_scale, t, gst, scale_dev, s, "mmda_clamp_adam")
        return None


class AdamW(Adam):
    """torch.optim.AdamW's constructor and defaults: decoupled weight decay, 1e-2"""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, clip_value=None):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, clip_value=clip_value,
                         decoupled_weight_decay=True)


class RMSprop(_FlatOptimizer):
    """torch.optim.RMSprop(params, lr) with torch's defaults (alpha 0.99, eps 1e-8, no momentum, not centered, no weight decay):
    the form the reference can construct (config.py:24, solver.py:97-99)."""

    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0, momentum=0, centered=False, clip_value=None):
        if weight_decay != 0 or momentum != 0 or centered:
            raise NotImplementedError("the reference passes lr only (solver.py:97-99)")
        super().__init__(params, dict(lr=lr, alpha=alpha, eps=eps, clip_value=clip_value))
        self._sq = None

    def _square_avg(self, like):
        if self._sq is None or self._sq.shape != like.shape or self._sq.device != like.device:
            self._sq = torch.zeros_like(like)
        return self._sq

    def _flat_state(self):
        return {"square_avg": self._square_avg(self._model.flat_buckets()[0])}

    def _load_flat_state(self, sd):
        sq = self._square_avg(self._model.flat_buckets()[0])
        sq.copy_(sd["square_avg"].to(sq.device))

    @torch.no_grad()
    def step(self, closure=None, clip_value=None, grad_scale=1.0):
        lib = _lib.load()
        self._next_step()
        s = _lib.stream_ptr()
        g0 = self.param_groups[0]
        clip = clip_value if clip_value is not None else g0["clip_value"]
        clip = float("inf") if clip is None else float(clip)
        m = self._flat()
        if m is not None:
            step_rules.check(embed_update=getattr(m, "embed_update", "dense"), optimizer="other", optimizer_name=type(self).__name__)
            P, G, _, _ = m.flat_buckets()
            sq = self._square_avg(P)
            runs = m._trainable_runs() if hasattr(m, "_trainable_runs") else None
            if runs is not None:                            # frozen parameters: the trainable runs only
                table, n_runs, items = runs
                _lib.check(lib.mmda_clamp_rmsprop_runs(P.data_ptr(), G.data_ptr(), sq.data_ptr(), table.data_ptr(), n_runs, items, g0["lr"],
                                                       g0["alpha"], g0["eps"], clip, grad_scale, s), "mmda_clamp_rmsprop_runs")
                return None
            _lib.check(lib.mmda_clamp_rmsprop(P.data_ptr(), G.data_ptr(), sq.data_ptr(), getattr(m, "grad_floats", P.numel()), g0["lr"], g0["alpha"], g0["eps"],
                                              clip, grad_scale, s), "mmda_clamp_rmsprop")
            return None
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.device.type != "cuda":
                    raise _lib.MMDAError("mmda_amd.optim.RMSprop steps on the GPU only")
                st = self.state[p]
                if not st:
                    st["square_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                g = p.grad.contiguous()
                _lib.check(lib.mmda_clamp_rmsprop(p.data_ptr(), g.data_ptr(), st["square_avg"].data_ptr(), p.numel(), group["lr"],
                                                  group["alpha"], group["eps"], clip, grad_scale, s), "mmda_clamp_rmsprop")
        return None


def clip_grad_value_(model_or_params, clip_value):
    """torch.nn.utils.clip_grad_value_ on the flat gradient bucket (solver.py:185)."""
    lib = _lib.load()
    m = model_or_params
    if hasattr(m, "flat_buckets") and m._G is not None:
        # embed_update 'sparse' / 'frozen': the bucket ends in front of embed.weight.  'sparse': the table's gradient rows are not yet
        # coalesced (clip_grad_value_ clamps the coalesced gradient), so the value is recorded for the pending rows update
        _lib.check(lib.mmda_clamp(m._G.data_ptr(), getattr(m, "grad_floats", m._G.numel()), float(clip_value), _lib.stream_ptr()),
                   "mmda_clamp")
        if getattr(m, "embed_update", "dense") in ("sparse", "deferred") and m._rows_pending:
            m._rows_clip = float(clip_value) if m._rows_clip is None else min(float(m._rows_clip), float(clip_value))
        return
    for p in m:
        if p.grad is not None:
            _lib.check(lib.mmda_clamp(p.grad.data_ptr(), p.grad.numel(), float(clip_value), _lib.stream_ptr()), "mmda_clamp")


def clip_grad_norm_(model_or_params, max_norm):
    """torch.nn.utils.clip_grad_norm_(..., max_norm) (L2) on the device: the norm of the flat gradient bucket -- of its trainable runs
    when parameters are frozen -- then the bucket scaled in place by min(1, max_norm / (norm + 1e-6)).  Returns the norm as a 0-d device
    tensor; nothing is read back.  A list of parameters takes one norm launch per tensor and a sum on the device."""
    lib = _lib.load()
    s = _lib.stream_ptr()
    max_norm = float(max_norm)
    if not max_norm >= 0.0:
        raise ValueError(f"max_norm must be >= 0: {max_norm}")
    m = model_or_params
    if hasattr(m, "flat_buckets") and m._G is not None:
        step_rules.check(embed_update=getattr(m, "embed_update", "dense"), clip_norm=1.0)      # (any norm of the whole gradient)
        G = m._G
        n = getattr(m, "grad_floats", G.numel())
        runs = m._trainable_runs() if hasattr(m, "_trainable_runs") else None
        table, n_runs, items = runs if runs is not None else (None, 0, 0)
        cap = int(lib.mmda_grad_norm_partials(items if runs is not None else n))
        parts = torch.empty(max(cap, 1), dtype=torch.float64, device=G.device)
        out = torch.empty(2, dtype=torch.float32, device=G.device)
        _lib.check(lib.mmda_grad_norm(G.data_ptr(), None, n, _lib.ptr(table), n_runs, items, max_norm, 1.0, parts.data_ptr(), cap,
                                      out.data_ptr(), s), "mmda_grad_norm")
        _lib.check(lib.mmda_grad_scale(G.data_ptr(), n, _lib.ptr(table), n_runs, items, out.data_ptr() + 4, s), "mmda_grad_scale")
        return out[0]
    grads = [p.grad for p in m if p.grad is not None]
    if not grads:
        return torch.zeros(())
    dev = grads[0].device
    sq = torch.zeros((), dtype=torch.float64, device=dev)
    for g in grads:
        if not (g.is_contiguous() and g.data_ptr() % 16 == 0):
            raise _lib.MMDAError("gradient storage is not 16-byte aligned/contiguous")
        cap = int(lib.mmda_grad_norm_partials(g.numel()))
        parts = torch.empty(max(cap, 1), dtype=torch.float64, device=dev)
        out = torch.empty(2, dtype=torch.float32, device=dev)
        _lib.check(lib.mmda_grad_norm(g.data_ptr(), None, g.numel(), None, 0, 0, max_norm, 1.0, parts.data_ptr(), cap, out.data_ptr(), s),
                   "mmda_grad_norm")
        sq = sq + out[0].double() ** 2
    norm = sq.sqrt().float()
    coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0).reshape(1).contiguous()
    for g in grads:
        _lib.check(lib.mmda_grad_scale(g.data_ptr(), g.numel(), None, 0, 0, coef.data_ptr(), s), "mmda_grad_scale")
    return norm


optimizer_dict = {"RMSprop": RMSprop, "Adam": Adam, "AdamW": AdamW}       # reference config.py:24, and AdamW
