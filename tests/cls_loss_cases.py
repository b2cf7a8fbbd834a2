"""The class-weighted / focal classification criterion (mmda_amd/csrc/loss_terms.h): its restatement in torch, the case
table of the device tests and their metrics.  Importable without a GPU.

Restatement, in whatever dtype the scores have (float64: the reference; float32: the yardstick of the bounds):
  lp = max(log s, -100), lq = max(log1p(-s), -100)
  l(s, y)  = -( w_c y (1-s)^g lp + (1-y) s^g lq )                  cls = sum_c (1/B) sum_b l
  dl/ds    = - w_c y ( (1-s)^g / max(s, 1e-12) - g (1-s)^(g-1) lp ) + (1-y) ( s^g / max(1-s, 1e-12) - g s^(g-1) lq )

Metrics of a result against the float64 restatement:
  value        |v - ref| / |ref|
  grad.whole   ||g - ref|| / ||ref||
  grad.worst   the worst element of |g - ref| / (|t| + |p|), t the element's own gradient term (scale * dl/ds / B) and p what the buffer
               held before the call (gradients accumulate): the scale at which the element's last addition rounds.  Relative to the
               element, not to the tensor: under a focal exponent the elements span seven decades, and a wrong small one would vanish
               in a norm.

Bound of a metric: 8 * max(e32, 2^-24), e32 the same metric of the float32 CPU restatement against the float64 one on the same inputs --
the rule of tests/losses_cases.py.  The kernel evaluates the same float32 expression; it differs in the library's logf / log1pf / powf
and in the order of the value's sum (256 strided partials, wave sums)."""
import zlib

import torch

FACTOR = 8.0
E32_FLOOR = 2.0 ** -24
WEIGHTS = [1.0, 2.5, 4.0, 11.0, 0.5, 7.0]
GAMMAS = (0.0, 1.0, 2.0, 3.5)
# B * ncls on each side of the 256-thread stride and at its smallest: 6 B crosses 256 between 42 and 43, 16 B between 16 and 17
SHAPES = [(1, 6), (5, 6), (42, 6), (43, 6), (300, 6), (16, 16), (17, 16), (257, 1)]


def weights_for(ncls):
    return [WEIGHTS[c % len(WEIGHTS)] for c in range(ncls)]


def _w(w, like):
    return torch.ones(like.shape[1], dtype=like.dtype) if w is None else torch.as_tensor(w, dtype=like.dtype)


def elementwise(s, y, w=None, g=0.0, clamp=True):
    """l(s, y) per element, in s.dtype, from differentiable torch operations (clamp=False: the unclamped expression)"""
    y = y.to(s.dtype)
    lp, lq = torch.log(s), torch.log1p(-s)
    if clamp:
        lp, lq = lp.clamp(min=-100.0), lq.clamp(min=-100.0)
    fp = (1.0 - s) ** g if g != 0.0 else torch.ones_like(s)
    fq = s ** g if g != 0.0 else torch.ones_like(s)
    return -(_w(w, s) * y * fp * lp + (1.0 - y) * fq * lq)


def value(s, y, w=None, g=0.0, clamp=True):
    """cls = sum_c (1/B) sum_b l"""
    return elementwise(s, y, w, g, clamp).mean(dim=0).sum()


def grad_closed(s, y, w=None, g=0.0):
    """d cls / d s by the closed form, in s.dtype"""
    y = y.to(s.dtype)
    lp, lq = torch.log(s).clamp(min=-100.0), torch.log1p(-s).clamp(min=-100.0)
    q = 1.0 - s
    one, zero = torch.ones_like(s), torch.zeros_like(s)
    fp, fq = (q ** g, s ** g) if g != 0.0 else (one, one)
    gp, gq = (g * q ** (g - 1.0), g * s ** (g - 1.0)) if g != 0.0 else (zero, zero)
    d = -_w(w, s) * y * (fp / s.clamp(min=1e-12) - gp * lp) + (1.0 - y) * (fq / q.clamp(min=1e-12) - gq * lq)
    return d / s.shape[0]


def oracle_cls(scores, emo, w=None, g=0.0):
    """the term in the scores' own dtype with autograd through it: what replaces oracle.misa_oracle's L.cls in a step's total"""
    return value(scores, emo, w, g)


# ------------------------------------------------------------------------------------------------ inputs
def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()) & 0x7FFFFFFF)


def inputs(B, ncls, tag=""):
    """scores = sigmoid(logits), logits uniform in [-3, 3] (float32 itself is accurate there), labels Bernoulli(0.3); float32"""
    gen = _gen(f"cls-B{B}-n{ncls}{tag}")
    s = torch.sigmoid(torch.rand(B, ncls, generator=gen) * 6.0 - 3.0)
    y = (torch.rand(B, ncls, generator=gen) < 0.3).float()
    return s, y


def prefill(B, ncls):
    return torch.randn(B, ncls, generator=_gen(f"cls-prefill-B{B}-n{ncls}"))


def saturated():
    """one row of six: scores exactly 0 and 1 against both labels, and two interior ones"""
    return torch.tensor([[0.0, 0.0, 1.0, 1.0, 0.25, 0.75]]), torch.tensor([[0.0, 1.0, 0.0, 1.0, 1.0, 0.0]])


# ------------------------------------------------------------------------------------------------ reference and metrics
def reference(s, y, w, g, scale=1.0, pre=None, dtype=torch.float64):
    """(value, gradient buffer after the call, the call's own term) with the float32 inputs widened exactly"""
    sd = s.to(dtype)
    v = value(sd, y, w, g)
    term = scale * grad_closed(sd, y, w, g)
    return v, (term if pre is None else term + pre.to(dtype)), term


def errors(val, grad, s, y, w, g, scale=1.0, pre=None):
    """the metrics of (val, grad) -- either may be None -- against the float64 restatement"""
    v64, g64, t64 = reference(s, y, w, g, scale, pre)
    out = {}
    if val is not None:
        out["value"] = abs(float(val) - float(v64)) / abs(float(v64))
    if grad is not None:
        got = grad.detach().cpu().double()
        assert torch.isfinite(got).all(), "non-finite values in the gradient"
        d = (got - g64).abs()
        denom = t64.abs() + (pre.double().abs() if pre is not None else 0.0)
        out["grad.whole"] = float(d.norm() / g64.norm())
        # (an element whose term and prefill are both exactly 0 -- a saturated score on the side its label switches off -- must be 0)
        inf = torch.full_like(d, float("inf"))
        out["grad.worst"] = float(torch.where(denom > 0, d / denom.clamp(min=1e-300), torch.where(d == 0, torch.zeros_like(d), inf)).max())
    return out


def e32(s, y, w, g, scale=1.0, pre=None, want_value=True, want_grad=True):
    """the same metrics of the float32 CPU restatement"""
    v32, g32, _ = reference(s, y, w, g, scale, pre, dtype=torch.float32)
    return errors(v32 if want_value else None, g32 if want_grad else None, s, y, w, g, scale, pre)


def bound(e):
    return FACTOR * max(e, E32_FLOOR)


def check(name, got, ref32, ratios=None):
    """every metric of `got` within 8 x the float32 restatement's; prints each figure first.  Returns the misses."""
    bad = []
    for k in sorted(got):
        e = max(ref32[k], E32_FLOOR)
        print(f"cls-loss-error {name} {k}: kernel {got[k]:.3e}  e32 {ref32[k]:.3e}  ratio {got[k] / e:.2f}  bound {bound(ref32[k]):.3e}")
        if ratios is not None:
            ratios[k] = round(got[k] / e, 3)
        if not got[k] <= bound(ref32[k]):
            bad.append(f"{name} {k}: {got[k]:.3e} > {bound(ref32[k]):.3e} (e32 {ref32[k]:.3e})")
    return bad
