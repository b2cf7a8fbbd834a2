"""The case table of the loss kernels (mmda_amd/csrc/losses.hip) and their float64 reference.  Importable without a GPU.

A loss call picks one of several kernel forms by its shape (ops.loss_forms reports which).  Every row below names the form it is
meant for; tests/test_losses_cases_cpu.py proves from the form query that the rows land there and that together they reach every
form, and tests/test_gpu_losses.py runs them on the device.

Reference: the dtype-agnostic functions of oracle/misa_oracle.py, evaluated in float64 with autograd on the float32 inputs the kernel
gets (widened exactly), generalised here to any pair list, 1..5 moments and a value scale.

Metrics of a result against the float64 reference:
  value        |v - ref| / |ref|
  grad.whole   ||g - ref|| / ||ref||, the worst error over the call's gradient tensors against the largest reference norm among them
  grad.rows    the largest row of g - ref (L2), relative to the RMS row norm of ref (a row's own norm can be as small as one likes where
  grad.cols    the gradient changes sign; a wrong tail row is off by a whole row norm and stands out against the RMS); same for columns

Bound of a metric: 8 * e32, where e32 is the same metric of the float32 CPU oracle against the float64 one, on the same inputs.  The
kernels accumulate in float32 as that oracle does; they differ from it in reduction order (eight row groups, wave sums) and send the
Gram products through the f32 GEMM; the factor 8 is the allowance for that.  e32 is taken as at least 2^-24: a float32 result carries
half an ulp of its own, and an oracle that happens to land closer than that did so by coincidence.  The bound is never looser than what
tests/test_gpu_ops.py asserts for the quantity (PRESENT)."""
import zlib

import torch

from oracle import misa_oracle as orc

PROD_DIFF = [(0, 3), (1, 4), (2, 5), (2, 0), (2, 1), (0, 1)]           # mmda_loss_diff / solver.py:432-439
PROD_CMD = [(0, 1), (0, 2), (2, 1)]                                    # mmda_loss_cmd / solver.py:415-417
FACTOR = 8.0
E32_FLOOR = 2.0 ** -24
# what tests/test_gpu_ops.py asserts today, per (kind, value or gradient)
PRESENT = {("diff", "value"): 1e-4, ("diff", "grad"): 2e-4, ("cmd", "value"): 1e-4, ("cmd", "grad"): 2e-4,
           ("conf", "value"): 1e-5, ("conf", "grad"): 1e-4, ("cls", "value"): 1e-5, ("cls", "grad"): 1e-5,
           ("domain", "value"): 1e-5, ("domain", "grad"): 1e-5, ("recon", "value"): 1e-5, ("recon", "grad"): 1e-5,
           ("misc", "value"): 1e-5, ("misc", "grad"): 1e-5, ("misc", "grad_conf"): 1e-4}


# ------------------------------------------------------------------------------------------------ the float64 reference
def diff_ref(ts, pairs):
    return sum(orc.diff_pair(ts[i], ts[j]) for i, j in pairs)


def cmd_ref(ts, pairs, n_moments=5, value_scale=1.0):
    return value_scale * sum(orc.cmd_pair(ts[i], ts[j], n_moments) for i, j in pairs)


def recon_ref(recs, origs):
    """mean over the tensors of MSE_mean (orc.recon_loss for three)"""
    return sum(((r - o) ** 2).mean() for r, o in zip(recs, origs)) / len(recs)


def domain_ref(doms):
    from types import SimpleNamespace
    return orc.domain_loss(SimpleNamespace(domain_label_t=doms[0], domain_label_v=doms[1], domain_label_a=doms[2]))


def evaluate(fn, inputs, dtype, n_grad=None):
    """fn over the inputs widened to dtype: (value, gradients of the first n_grad inputs), as dtype tensors"""
    n_grad = len(inputs) if n_grad is None else n_grad
    xs = [x.detach().to(dtype).requires_grad_(i < n_grad) for i, x in enumerate(inputs)]
    v = fn(xs)
    v.backward()
    return v.detach(), [x.grad if x.grad is not None else torch.zeros_like(x) for x in xs[:n_grad]]


# ------------------------------------------------------------------------------------------------ metrics and bounds
def _rms(v):
    return float((v.double() ** 2).mean().sqrt())


def grad_errors(got, ref):
    """{whole, rows, cols}: the absolute error figures of a 2-D gradient against the float64 one, and the reference's own figures"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape and got.dim() == 2, (got.shape, ref.shape)
    assert torch.isfinite(got).all(), "non-finite values in the gradient"
    d = got - ref
    return (dict(whole=float(d.norm()), rows=float(d.norm(dim=1).max()), cols=float(d.norm(dim=0).max())),
            dict(whole=float(ref.norm()), rows=_rms(ref.norm(dim=1)), cols=_rms(ref.norm(dim=0))))


def errors(value, grads, ref_value, ref_grads, group="grad"):
    """The metrics of one call: value (None: not taken) and the worst of each gradient metric over the call's tensors.  A tensor's
    error is taken relative to the largest reference figure among the call's tensors: the exact gradient of one tensor can cancel to
    nothing (CMD at D = 1 is a sum of signs over the pairs), the call's scale cannot."""
    out = {}
    if value is not None:
        v, r = float(value), float(ref_value)
        out["value"] = abs(v - r) / abs(r) if r != 0.0 else (0.0 if v == 0.0 else float("inf"))
    per = [grad_errors(g, r) for g, r in zip(grads, ref_grads)]
    for k in ("whole", "rows", "cols"):
        if per:
            scale = max(r[k] for _, r in per)
            worst = max(e[k] for e, _ in per)
            out[f"{group}.{k}"] = worst / scale if scale > 0.0 else (0.0 if worst == 0.0 else float("inf"))
    return out


def bound(kind, metric, e32):
    present = PRESENT[(kind, metric.split(".")[0])]
    return min(FACTOR * max(e32, E32_FLOOR), present)


def check(kind, name, got, e32, ratios=None):
    """Every metric of `got` within its bound; prints each figure first.  Returns the list of misses (strings).  ratios: a dict that
    receives kernel error / e32 per metric."""
    bad = []
    for k in sorted(got):
        e = max(e32[k], E32_FLOOR)
        b = bound(kind, k, e32[k])
        print(f"losses-error {name} {k}: kernel {got[k]:.3e}  e32 {e32[k]:.3e}  ratio {got[k] / e:.2f}  bound {b:.3e}")
        if ratios is not None:
            ratios[k] = round(got[k] / e, 3)
        if not got[k] <= b:
            bad.append(f"{name} {k}: {got[k]:.3e} > {b:.3e} (e32 {e32[k]:.3e}, ratio {got[k] / e:.2f})")
    return bad


# ------------------------------------------------------------------------------------------------ inputs
def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()) & 0x7FFFFFFF)


def side_inputs(c):
    """nt (B, D) tensors of sigmoid(randn), as the present tests make them; c['nan']: (tensor, row, column) set to NaN"""
    g = _gen(c["name"])
    ts = [torch.sigmoid(torch.randn(c["B"], c["D"], generator=g)) for _ in range(c["nt"])]
    for t, r, col in c.get("nan", ()):
        ts[t][r, col] = float("nan")
    return ts


def head_inputs(c):
    """scores, tcp (B, ncls) in (0, 1) and 0/1 labels with a positive in every class"""
    g = _gen(c["name"])
    B, n = c["B"], c["ncls"]
    s = torch.sigmoid(torch.randn(B, n, generator=g))
    t = torch.sigmoid(torch.randn(B, n, generator=g))
    y = (torch.rand(B, n, generator=g) > 0.6).float()
    y[0] = 1.0
    return s, t, y


def domain_inputs(c):
    g = _gen(c["name"])
    return [torch.randn(c["B"], 3, generator=g) for _ in range(3)]


def recon_inputs(c):
    g = _gen(c["name"])
    return ([torch.randn(c["B"], c["D"], generator=g) for _ in range(3)], [torch.randn(c["B"], c["D"], generator=g) for _ in range(3)])


def misc_inputs(c):
    g = _gen(c["name"])
    s, t, y = head_inputs(c)
    n = c["n_recon"]
    return dict(s=s, t=t, y=y, rec=torch.randn(1, n, generator=g), org=torch.randn(1, n, generator=g),
                L1=0.37, L2=1.21, dw=0.3, sw=0.8, rw=0.6, cw=0.9, conf_scale=0.9, recon_scale=0.6)


def side_fn(c):
    if c["kind"] == "diff":
        return lambda xs: diff_ref(xs, c["pairs"])
    return lambda xs: cmd_ref(xs, c["pairs"], c["n_moments"], c["value_scale"])


def side_reference(c, ts=None):
    """(value64, grads64, e32) of a diff or cmd case"""
    ts = side_inputs(c) if ts is None else ts
    v64, g64 = evaluate(side_fn(c), ts, torch.float64)
    v32, g32 = evaluate(side_fn(c), ts, torch.float32)
    return v64, g64, errors(v32, g32, v64, g64)


# ------------------------------------------------------------------------------------------------ DiffLoss
# the fast form by row count (D <= 128): rows per thread 4 / 8 / 16 / 32, generic beyond 256 rows
_DIFF_B = {2: "fast4", 7: "fast4", 8: "fast4", 9: "fast4", 32: "fast4", 33: "fast8", 64: "fast8", 65: "fast16", 128: "fast16",
           129: "fast32", 256: "fast32", 257: "generic"}
_DIFF_D = (3, 63, 64, 65, 127, 128, 129)


def _diff(B, D, form, nt=6, pairs=PROD_DIFF, tag="", **kw):
    few = B <= 256
    return dict(kind="diff", name=f"diff-B{B}-D{D}{tag}", B=B, D=D, nt=nt, pairs=list(pairs),
                expect=dict(diff=form, diff_products="skinny" if few else "batched", diff_loss_sum="finish" if few else "own_launch"), **kw)


DIFF_SHAPES = [_diff(B, D, f) for D in (65, 128) for B, f in _DIFF_B.items()]
DIFF_SHAPES += [_diff(B, D, "generic" if D > 128 else _DIFF_B[B]) for B in (9, 33) for D in _DIFF_D if D not in (65, 128)]
DIFF_SHAPES += [_diff(257, 129, "generic"), _diff(2, 3, "fast4")]

_DIFF_LISTS = (("nt2", 2, [(0, 1)]), ("nt4", 4, [(3, 0), (1, 2)]), ("nt6", 6, PROD_DIFF), ("unused", 4, [(0, 1), (1, 3)]),
               ("self", 3, [(1, 1), (0, 2)]), ("repeat", 3, [(0, 1), (0, 1), (2, 1)]))
DIFF_LISTS = [_diff(B, 65, f, nt, pairs, tag=f"-{tag}") for B, f in ((9, "fast4"), (257, "generic")) for tag, nt, pairs in _DIFF_LISTS]

# a few NaN elements, in the fast and in the generic prep: first and last row, the column at a wave's edge, the last column
DIFF_NAN = [_diff(9, 65, "fast4", tag="-nan", nan=[(0, 0, 0), (1, 8, 64), (3, 4, 63), (5, 8, 0)]),
            _diff(257, 129, "generic", tag="-nan", nan=[(0, 0, 0), (1, 256, 128), (3, 100, 64), (5, 256, 0)])]


# ------------------------------------------------------------------------------------------------ CMD
_CMD_B = {3: "fast4", 7: "fast4", 8: "fast4", 9: "fast4", 32: "fast4", 33: "fast8", 64: "fast8", 65: "stream", 129: "stream",
          257: "stream"}
_CMD_D = (1, 2, 63, 64, 65, 127, 128, 129, 160)


def _cmd(B, D, form, nt=3, pairs=PROD_CMD, n_moments=5, value_scale=1.0 / 3.0, tag=""):
    return dict(kind="cmd", name=f"cmd-B{B}-D{D}{tag}", B=B, D=D, nt=nt, pairs=list(pairs), n_moments=n_moments, value_scale=value_scale,
                expect=dict(cmd=form, cmd_grid=nt if form == "stream" else 1))


CMD_SHAPES = [_cmd(B, D, f) for D in (65, 128) for B, f in _CMD_B.items()]
CMD_SHAPES += [_cmd(B, D, "serial" if D > 128 else _CMD_B[B]) for B in (9, 33) for D in _CMD_D if D not in (65, 128)]
CMD_SHAPES += [_cmd(3, 512, "serial"), _cmd(65, 1, "stream"), _cmd(129, 63, "stream"), _cmd(257, 129, "serial")]
CMD_REJECT = dict(kind="cmd", name="cmd-B3-D513-reject", B=3, D=513, nt=3, pairs=PROD_CMD, n_moments=5, value_scale=1.0 / 3.0,
                  expect=dict(cmd="reject", cmd_grid=0))

CMD_FORM_REPS = ((9, 65, "fast4"), (33, 65, "fast8"), (65, 65, "stream"), (9, 160, "serial"))
CMD_ARGS = []
for _B, _D, _f in CMD_FORM_REPS:
    CMD_ARGS += [_cmd(_B, _D, _f, n_moments=k, tag=f"-nm{k}") for k in (1, 2, 3, 4)]           # (5: every row of CMD_SHAPES)
    CMD_ARGS += [_cmd(_B, _D, _f, nt=2, pairs=[(0, 1)], value_scale=1.0, tag="-nt2"),
                 _cmd(_B, _D, _f, nt=2, pairs=[(1, 0)], value_scale=1.0, tag="-reversed"),
                 _cmd(_B, _D, _f, value_scale=1.0, tag="-vs1")]                                 # (nt = 3 at 1/3: CMD_SHAPES)

# more pairs than the three the model uses: both orders of each pair
NP4 = [(0, 1), (1, 0), (0, 2), (2, 0)]
NP6 = [(0, 1), (1, 0), (0, 2), (2, 0), (2, 1), (1, 2)]
CMD_LISTS = [_cmd(B, D, f, pairs=pairs, tag=f"-np{len(pairs)}") for B, D, f in CMD_FORM_REPS for pairs in (NP4, NP6)]


# ------------------------------------------------------------------------------------------------ cls, conf, domain, recon
def _head(kind, B, ncls=6):
    return dict(kind=kind, name=f"{kind}-B{B}-n{ncls}", B=B, ncls=ncls)


CLS_CASES = [_head("cls", B) for B in (1, 255, 256, 257)] + [_head("cls", 41, n) for n in (1, 7)]
CONF_CASES = [_head("conf", B) for B in (1, 63, 64, 65, 257)]
DOMAIN_CASES = [dict(kind="domain", name=f"domain-B{B}", B=B) for B in (1, 85, 86, 257)]          # 3B crosses 256 between 85 and 86
# recon: 3 * B * D elements over ceil(n / 256) workgroups, 64 at the most
RECON_CASES = [dict(kind="recon", name=f"recon-B{B}-D{D}", B=B, D=D, expect=dict(recon_blocks=rb))
               for B, D, rb in ((1, 1, 1), (5, 17, 1), (5, 103, 7), (43, 127, 64), (129, 128, 64))]


# ------------------------------------------------------------------------------------------------ mmda_loss_misc
def _misc(B, n_recon, rb, ncls=6, with_conf=1, conf_grads=1, use_conf=1):
    return dict(kind="misc", name=f"misc-B{B}-n{ncls}-r{n_recon}-w{with_conf}g{conf_grads}u{use_conf}", B=B, ncls=ncls, n_recon=n_recon,
                with_conf=with_conf, conf_grads=conf_grads, use_conf=use_conf, expect=dict(misc_recon_blocks=rb),
                grid=1 + (ncls if with_conf else 0) + rb)


MISC_RECON = ((1, 1), (2047, 1), (2048, 1), (2049, 2), (17 * 2048, 17), (64 * 2048 + 5, 64))
MISC_CASES = [_misc(5, 2049, 2, with_conf=w, conf_grads=g, use_conf=u) for w in (0, 1) for g in (0, 1) for u in (0, 1)]
MISC_CASES += [_misc(5, n, rb) for n, rb in MISC_RECON if n != 2049]
MISC_CASES += [_misc(257, 1, 1), _misc(257, 64 * 2048 + 5, 64)]
MISC_CASES += [_misc(B, 2049, 2, ncls=4, with_conf=0, conf_grads=0, use_conf=0) for B in (5, 257)]


def misc_reference(c, inp, dtype, pre=None):
    """L[0], L[3], L[4], L[5] and the four gradient buffers (pre: what they held before, added to) of a misc case"""
    conf_on = bool(c["with_conf"])
    grads_on = conf_on and bool(c["conf_grads"])
    s = inp["s"].to(dtype).requires_grad_(True); t = inp["t"].to(dtype).requires_grad_(True); y = inp["y"].to(dtype)
    rec = inp["rec"].to(dtype).requires_grad_(True); org = inp["org"].to(dtype).requires_grad_(True)
    cls = orc.cls_loss(s, y)
    conf = orc.conf_loss(s, t, y) if conf_on else torch.zeros((), dtype=dtype)
    recon = ((rec - org) ** 2).mean()
    seed = cls + inp["recon_scale"] * recon + (inp["conf_scale"] * conf if grads_on else 0.0)
    seed.backward()
    total = cls + inp["dw"] * inp["L1"] + inp["sw"] * inp["L2"] + inp["rw"] * recon + (inp["cw"] * conf if c["use_conf"] else 0.0)
    g = dict(d_scores=s.grad, d_tcp=t.grad if t.grad is not None else torch.zeros_like(t), d_recon=rec.grad, d_orig=org.grad)
    if pre is not None:
        g = {k: v + pre[k].to(dtype) for k, v in g.items()}
    return dict(cls=cls.detach(), recon=recon.detach(), conf=conf.detach(), total=total.detach()), g


# ------------------------------------------------------------------------------------------------ the call contract
# once per form: scale = 0.3 onto pre-filled loss and dx; loss = NULL; dx = NULL; stride = B * D + 8 with NaN in the gaps of x and a
# canary in the gaps of dx
VARIANTS = ("scale_prefill", "no_loss", "no_dx", "stride")
_CONTRACT_DIFF = ((9, 65, "fast4"), (33, 65, "fast8"), (65, 65, "fast16"), (129, 65, "fast32"), (9, 129, "generic"), (257, 65, "generic"))


def _contract(base, variant):
    c = dict(base, name=f"{base['name']}-{variant}", variant=variant, have_loss=variant != "no_loss", have_dx=variant != "no_dx")
    e = dict(base.get("expect", {}))
    if c["kind"] == "diff":
        e["diff_loss_sum"] = None if not c["have_loss"] else ("finish" if c["have_dx"] and c["B"] <= 256 else "own_launch")
    if c["kind"] == "cmd" and e["cmd"] == "stream":
        e["cmd_grid"] = c["nt"] if c["have_dx"] else 1
    if c["kind"] == "recon" and variant == "stride":
        e["recon_blocks"] = c["stride_blocks"]                      # three launches of B * D elements each
    c["expect"] = e
    return c


CONTRACT = [_contract(_diff(B, D, f), v) for B, D, f in _CONTRACT_DIFF for v in VARIANTS]
CONTRACT += [_contract(_cmd(B, D, f), v) for B, D, f in CMD_FORM_REPS for v in VARIANTS]
CONTRACT += [_contract(dict(kind="recon", name="recon-B5-D103", B=5, D=103, expect=dict(recon_blocks=7), stride_blocks=3), v)
             for v in VARIANTS]
CONTRACT += [_contract(dict(kind="recon", name="recon-B43-D127", B=43, D=127, expect=dict(recon_blocks=64), stride_blocks=22), v)
             for v in VARIANTS]
CONTRACT += [_contract(_head(k, 41), v) for k in ("cls", "conf") for v in VARIANTS[:3]]
CONTRACT += [_contract(dict(kind="domain", name="domain-B41", B=41), v) for v in VARIANTS[:3]]

# the loss value has the same bits in two runs on the same input (partials are added in block order)
REPRO = [_diff(257, 65, "generic", tag="-repro"), dict(kind="recon", name="recon-B129-D128-repro", B=129, D=128),
         dict(_misc(5, 64 * 2048 + 5, 64), name="misc-r64-repro")]

SIDE_CASES = DIFF_SHAPES + DIFF_LISTS + CMD_SHAPES + CMD_ARGS + CMD_LISTS
ALL_FORM_ROWS = SIDE_CASES + DIFF_NAN + [CMD_REJECT] + RECON_CASES + MISC_CASES + CONTRACT


def forms_of(c):
    """what ops.loss_forms says about the call a row makes"""
    from mmda_amd import ops
    n_recon = c.get("n_recon", 0)
    if c["kind"] == "recon" and c.get("variant") == "stride":
        n_recon = c["B"] * c["D"]                                  # three launches of one tensor each
    return ops.loss_forms(c["B"], c.get("D", 1), have_loss=c.get("have_loss", True), have_dx=c.get("have_dx", True),
                          cmd_nt=c.get("nt", 3) if c["kind"] == "cmd" else 3, n_recon=n_recon)
