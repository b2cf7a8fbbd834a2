"""MI355X: every launch form of the loss kernels (mmda_amd/csrc/losses.hip) at its edges against the float64 reference.

The rows, the reference, the metrics and the bounds are in tests/losses_cases.py; tests/test_losses_cases_cpu.py proves which kernel
form each row reaches.  A bound is 8 x the error of the float32 CPU oracle on the same inputs (computed here, per row and metric),
never looser than what tests/test_gpu_ops.py asserts.  Every figure is printed before it is asserted.  With MMDA_LOSSES_RATIOS_OUT set
to a path, the measured kernel error / e32 of every row is written there as JSON (tests/golden/losses_error_ratios.json is such a run).

Findings of the first run against float64, kept here because they explain what a reader of the figures will see:
  * the factor 8 held at every row; the worst ratio was 6.0 (the value of diff-B256-D128, 6.7e-7: one thread adds the 256 block partials
    of the combine launch one after the other).
  * the fast and the stream form of CMD summed only the first three pairs of a list (the cmd-*-np4 / -np6 rows at D = 65 were off by
    25 % and 50 % in the value); the serial form at D = 160 took all six.  Fixed in the kernels: every form takes up to six pairs.
  * the DiffLoss prep kernels replace NaN by 0 as torch.nan_to_num does, but the gradient they leave AT a NaN position is the gradient
    with respect to that substituted 0 (autograd through nan_to_num gives exactly 0 there).  test_diff_nan_to_num prints both and asserts
    the finite positions only."""
import ctypes as C
import json
import os

import pytest
import torch

import losses_cases as lc
from mmda_amd import _lib
from mmda_amd.utils import functions as F
from oracle import misa_oracle as orc

pytestmark = pytest.mark.gpu
EINVAL = -1
RATIOS = {}


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _ratios_file():
    yield
    path = os.environ.get("MMDA_LOSSES_RATIOS_OUT")
    if path:
        with open(path, "w") as f:
            json.dump(RATIOS, f, indent=0, sort_keys=True)


def _ids(cases):
    return [c["name"] for c in cases]


def _assert_ok(c, got, e32, suffix=""):
    bad = lc.check(c["kind"], c["name"] + suffix, got, e32, RATIOS.setdefault(c["name"] + suffix, {}))
    assert not bad, "\n".join(bad)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ DiffLoss and CMD through functions.py
def _run_side(c, ts):
    gts = [t.to(dev()).requires_grad_(True) for t in ts]
    if c["kind"] == "diff":
        got = F.diff_loss_multi(gts, c["pairs"])
    else:
        got = F.cmd_loss_multi(gts, c["pairs"], c["n_moments"], c["value_scale"])
    got.backward()
    return got.detach().cpu(), [g.grad.cpu() for g in gts]


@pytest.mark.parametrize("c", lc.SIDE_CASES, ids=_ids(lc.SIDE_CASES))
def test_diff_and_cmd_rows(c):
    ts = lc.side_inputs(c)
    v64, g64, e32 = lc.side_reference(c, ts)
    v, g = _run_side(c, ts)
    _assert_ok(c, lc.errors(v, g, v64, g64), e32)
    used = {i for p in c["pairs"] for i in p}
    for k in range(c["nt"]):
        if k not in used:
            assert float(g64[k].abs().max()) == 0.0 and float(g[k].abs().max()) == 0.0, f"tensor {k} is in no pair"


@pytest.mark.parametrize("c", lc.DIFF_NAN, ids=_ids(lc.DIFF_NAN))
def test_diff_nan_to_num(c):
    ts = lc.side_inputs(c)
    v64, g64, e32 = lc.side_reference(c, ts)
    v, g = _run_side(c, ts)
    # what the kernel leaves at the NaN positions, beside the gradient with respect to the 0 that replaced the NaN
    zeroed = [torch.nan_to_num(t) for t in ts]
    _, g0 = lc.evaluate(lambda xs: sum(_diff_pair_plain(xs[i], xs[j]) for i, j in c["pairs"]), zeroed, torch.float64)
    for t, r, col in c["nan"]:
        assert float(g64[t][r, col]) == 0.0
        print(f"losses-nan {c['name']} tensor {t} [{r},{col}]: kernel {float(g[t][r, col]):.6e}  autograd through nan_to_num 0  "
              f"gradient w.r.t. the substituted 0: {float(g0[t][r, col]):.6e}")
        g[t][r, col] = 0.0
    _assert_ok(c, lc.errors(v, g, v64, g64), e32)


def _diff_pair_plain(x1, x2):
    """orc.diff_pair without the nan_to_num (inputs already finite): the gradient flows to every element"""
    x1 = x1 - x1.mean(dim=0, keepdim=True)
    x2 = x2 - x2.mean(dim=0, keepdim=True)
    n1 = x1.norm(dim=1, keepdim=True).detach() + 1e-6
    n2 = x2.norm(dim=1, keepdim=True).detach() + 1e-6
    g = (x1 / n1).t() @ (x2 / n2)
    return (g * g).mean()


# ------------------------------------------------------------------------------------------------ raw calls (the C ABI through _lib)
class Call:
    """One loss call on buffers of our own: the logical (rows, cols) tensors that get gradients, grouped into the stacked buffers the
    entry point takes (pad floats behind each tensor of a group: stride = rows * cols + pad), and the tensors it only reads."""

    def __init__(self, c, pad=0):
        self.c, self.pad, k = c, pad, c["kind"]
        if k in ("diff", "cmd"):
            ts = lc.side_inputs(c)
            self.groups, self.consts, self.fn = [ts], [], lc.side_fn(c)
        elif k == "recon":
            rec, org = lc.recon_inputs(c)
            self.groups, self.consts, self.fn = [rec, org], [], (lambda xs: lc.recon_ref(xs[:3], xs[3:]))
        elif k == "domain":
            self.groups, self.consts, self.fn = [lc.domain_inputs(c)], [], lc.domain_ref
        else:
            s, t, y = lc.head_inputs(c)
            if k == "cls":
                self.groups, self.consts, self.fn = [[s]], [y], (lambda xs: orc.cls_loss(xs[0], y.to(xs[0].dtype)))
            else:
                self.groups, self.consts, self.fn = [[s], [t]], [y], (lambda xs: orc.conf_loss(xs[0], xs[1], y.to(xs[0].dtype)))
        assert pad == 0 or k in ("diff", "cmd", "recon")
        self.logical = [t for g in self.groups for t in g]

    def stack(self, group, body, fill):
        """(tensors of the group, body + pad) buffer: `body` tensors in front, `fill` in the gaps"""
        m = body[0].numel()
        buf = torch.full((len(group), m + self.pad), fill, dtype=torch.float32)
        buf[:, :m] = torch.stack([t.reshape(-1).float() for t in body])
        return buf

    def unstack(self, bufs):
        """the logical tensors out of the group buffers, and the gap floats"""
        out, gaps = [], []
        for group, buf in zip(self.groups, bufs):
            m = group[0].numel()
            buf = buf.cpu()
            out += [buf[i, :m].reshape(group[0].shape) for i in range(len(group))]
            gaps.append(buf[:, m:])
        return out, gaps

    def launch(self, scale, loss, gbufs):
        c, lib, s = self.c, _lib.load(), _lib.stream_ptr()
        p = lambda t: None if t is None else t.data_ptr()
        x = [self.stack(g, g, float("nan")).to(dev()) for g in self.groups]
        k = [t.to(dev()) for t in self.consts]
        g = gbufs if gbufs is not None else [None] * len(self.groups)
        B, D = c["B"], c.get("D", 0)
        stride = B * D + self.pad
        if c["kind"] == "diff":
            arr, n = F._pairs(c["pairs"])
            work = torch.empty(lib.mmda_loss_diff_work_floats(B, D), device=dev())
            rc = lib.mmda_loss_diff_pairs(p(x[0]), stride, c["nt"], n, arr, B, D, scale, p(loss), p(g[0]), p(work), s)
        elif c["kind"] == "cmd":
            arr, n = F._pairs(c["pairs"])
            rc = lib.mmda_loss_cmd_pairs(p(x[0]), stride, c["nt"], n, arr, c["n_moments"], B, D, scale, c["value_scale"], p(loss), p(g[0]), s)
        elif c["kind"] == "recon":
            rc = lib.mmda_loss_recon(p(x[0]), p(x[1]), stride, B, D, scale, p(loss), p(g[0]), p(g[1]), s)
        elif c["kind"] == "domain":
            rc = lib.mmda_loss_domain(p(x[0]), B, scale, p(loss), p(g[0]), s)
        elif c["kind"] == "cls":
            rc = lib.mmda_loss_cls(p(x[0]), p(k[0]), B, c["ncls"], scale, p(loss), p(g[0]), s)
        else:
            rc = lib.mmda_loss_conf(p(x[0]), p(x[1]), p(k[0]), B, c["ncls"], scale, p(loss), p(g[0]), p(g[1]), s)
        torch.cuda.synchronize()
        return rc


CANARY = -12345.678


def _run_variant(c, variant):
    """One raw call in a variant of the contract; asserts every metric against float64 at 8 x the float32 oracle's error."""
    call = Call(c, pad=8 if variant == "stride" else 0)
    scale = 0.3 if variant == "scale_prefill" else 1.0
    have_loss, have_dx = variant != "no_loss", variant != "no_dx"
    v64, g64 = lc.evaluate(call.fn, call.logical, torch.float64)
    v32, g32 = lc.evaluate(call.fn, call.logical, torch.float32)
    gen = torch.Generator().manual_seed(5)
    if variant == "scale_prefill":              # non-zero, of the size of what is added: the sum is held to the bound
        loss0 = float(torch.tensor(0.5 * float(v64), dtype=torch.float32))
        pre = [(torch.randn(t.shape, generator=gen) * max(lc._rms(scale * g), 1e-30)).float() for t, g in zip(call.logical, g64)]
    else:
        loss0, pre = 0.0, [torch.zeros_like(t) for t in call.logical]
    loss = torch.tensor([loss0], device=dev()) if have_loss else None
    gbufs, at = None, 0
    if have_dx:
        gbufs = []
        for group in call.groups:
            gbufs.append(call.stack(group, pre[at:at + len(group)], CANARY).to(dev()))
            at += len(group)
    assert call.launch(scale, loss, gbufs) == 0, _lib.load().mmda_last_error()
    want_v = loss0 + v64                        # the value is NOT scaled
    got_v = loss.cpu()[0] if have_loss else None
    got_g, want_g, ref32_g = [], [], []
    if have_dx:
        got_g, gaps = call.unstack(gbufs)
        want_g = [p.double() + scale * g for p, g in zip(pre, g64)]
        ref32_g = [p + scale * g for p, g in zip(pre, g32)]
        for gap in gaps:
            assert torch.equal(_bits(gap), _bits(torch.full_like(gap, CANARY))), "the gap floats of dx were written"
    e32 = lc.errors(torch.tensor(loss0) + v32 if have_loss else None, ref32_g, want_v, want_g)
    _assert_ok(c, lc.errors(got_v, got_g, want_v, want_g), e32)


@pytest.mark.parametrize("c", lc.CONTRACT, ids=_ids(lc.CONTRACT))
def test_call_contract(c):
    _run_variant(c, c["variant"])


PLAIN = lc.CLS_CASES + lc.CONF_CASES + lc.DOMAIN_CASES + lc.RECON_CASES


@pytest.mark.parametrize("c", PLAIN, ids=_ids(PLAIN))
def test_cls_conf_domain_recon_rows(c):
    _run_variant(c, "plain")


def test_diff_dx_of_a_tensor_in_no_pair_keeps_its_bits():
    for c in (c for c in lc.DIFF_LISTS if "unused" in c["name"]):
        call = Call(c)
        gen = torch.Generator().manual_seed(6)
        pre = [torch.randn(t.shape, generator=gen) for t in call.logical]
        gbufs = [call.stack(call.groups[0], pre, CANARY).to(dev())]
        assert call.launch(1.0, torch.zeros(1, device=dev()), gbufs) == 0
        got, _ = call.unstack(gbufs)
        assert torch.equal(_bits(got[2]), _bits(pre[2])), c["name"]
        assert not torch.equal(got[0], pre[0])


def test_cmd_rejects_more_than_512_columns_and_leaves_loss_and_dx_alone():
    c = lc.CMD_REJECT
    call = Call(c)
    loss = torch.tensor([0.625], device=dev())
    pre = [torch.full(t.shape, 0.5) for t in call.logical]
    gbufs = [call.stack(call.groups[0], pre, CANARY).to(dev())]
    assert call.launch(1.0, loss, gbufs) == EINVAL
    assert float(loss.cpu()[0]) == 0.625 and torch.equal(gbufs[0].cpu(), call.stack(call.groups[0], pre, CANARY))
    with pytest.raises(_lib.MMDAError):
        F.cmd_loss_multi([t.to(dev()) for t in call.logical], c["pairs"], 5, 1.0)


def test_cmd_loss_multi_computes_the_callers_list_or_raises():
    """up to six pairs are computed in every form (the np rows of the table); a seventh is refused, not dropped"""
    ts = [t.to(dev()) for t in lc.side_inputs(lc.CMD_LISTS[0])]
    with pytest.raises(_lib.MMDAError):
        F.cmd_loss_multi(ts, lc.NP6 + [(0, 1)], 5, 1.0)
    with pytest.raises(_lib.MMDAError):
        F.cmd_loss_multi(ts + ts[:1], lc.PROD_CMD, 5, 1.0)              # four tensors: more than any CMD form holds


def test_bce_saturated_scores_value_and_gradient():
    """BCELoss clamps log at -100 and its backward divides by max(s(1-s), 1e-12): scores of exactly 0/1 stay finite."""
    s = torch.tensor([[0.0, 1.0, 0.5, 1.0, 0.0, 0.25]]); y = torch.tensor([[1.0, 0.0, 1.0, 1.0, 0.0, 0.0]])
    ref = torch.nn.BCELoss()(s[0], y[0]) * 6
    gs = s.to(dev()).requires_grad_(True)
    got = F.bce_sum_over_classes(gs, y.to(dev()))
    got.backward()
    assert abs(got.item() - ref.item()) < 1e-4 * ref.item()
    sd, yd = s.double(), y.double()
    want = (sd - yd) / torch.clamp(sd * (1 - sd), min=1e-12) / 1
    err = ((gs.grad.cpu().double() - want).abs() / want.abs().clamp_min(1e-30)).max()
    print(f"losses-error cls-saturated grad: worst element {float(err):.3e}  bound 1.000e-05")
    assert torch.equal(gs.grad.cpu() == 0, want == 0) and float(err) <= 1e-5


# ------------------------------------------------------------------------------------------------ mmda_loss_misc, directly
def _run_misc(c, inp, pre):
    d, lib = dev(), _lib.load()
    s, t, y, rec, org = (inp[k].to(d) for k in ("s", "t", "y", "rec", "org"))
    L = torch.zeros(8, device=d)
    L[1] = inp["L1"]; L[2] = inp["L2"]
    g = {k: v.clone().to(d) for k, v in pre.items()}
    rc = lib.mmda_loss_misc(s.data_ptr(), t.data_ptr(), y.data_ptr(), c["B"], c["ncls"], g["d_scores"].data_ptr(), g["d_tcp"].data_ptr(),
                            c["with_conf"], c["conf_grads"], inp["conf_scale"], rec.data_ptr(), org.data_ptr(), c["n_recon"],
                            inp["recon_scale"], g["d_recon"].data_ptr(), g["d_orig"].data_ptr(), L.data_ptr(), inp["dw"], inp["sw"],
                            inp["rw"], inp["cw"], c["use_conf"], _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, lib.mmda_last_error()
    return L.cpu(), {k: v.cpu() for k, v in g.items()}


def _misc_pre(c, inp):
    gen = torch.Generator().manual_seed(7)
    B, n = c["B"], c["ncls"]
    return dict(d_scores=torch.randn(B, n, generator=gen) / B, d_tcp=torch.randn(B, n, generator=gen) / B,
                d_recon=torch.randn(1, c["n_recon"], generator=gen) / c["n_recon"], d_orig=torch.randn(1, c["n_recon"], generator=gen) / c["n_recon"])


@pytest.mark.parametrize("c", lc.MISC_CASES, ids=_ids(lc.MISC_CASES))
def test_misc_rows(c):
    inp = lc.misc_inputs(c)
    pre = _misc_pre(c, inp)
    L64, g64 = lc.misc_reference(c, inp, torch.float64, pre)
    L32, g32 = lc.misc_reference(c, inp, torch.float32, pre)
    L, g = _run_misc(c, inp, pre)
    assert int(_bits(L)[7]) == c["grid"], "the ticket counts the workgroups"
    assert float(L[1]) == float(torch.tensor(inp["L1"])) and float(L[2]) == float(torch.tensor(inp["L2"])) and float(L[6]) == 0.0
    conf_on = bool(c["with_conf"])
    grads_on = conf_on and bool(c["conf_grads"])
    got, e32 = {}, {}
    for name, i in (("cls", 0), ("recon", 3), ("conf", 4), ("total", 5)):
        if name == "conf" and not conf_on:
            assert float(L[4]) == 0.0
            continue
        got["value." + name] = lc.errors(L[i], [], L64[name], [])["value"]
        e32["value." + name] = lc.errors(L32[name], [], L64[name], [])["value"]
    head = "grad_conf" if grads_on else "grad"
    for group, keys in ((head, ("d_scores",) + (("d_tcp",) if grads_on else ())), ("grad", ("d_recon", "d_orig"))):
        a = lc.errors(None, [g[k] for k in keys], None, [g64[k] for k in keys], group)
        b = lc.errors(None, [g32[k] for k in keys], None, [g64[k] for k in keys], group)
        for m in a:
            got[f"{m}@{keys[0]}"] = a[m]; e32[f"{m}@{keys[0]}"] = b[m]
    if not grads_on:
        assert torch.equal(_bits(g["d_tcp"]), _bits(pre["d_tcp"])), "d_tcp written without conf gradients"
    _assert_ok(c, got, e32)


# ------------------------------------------------------------------------------------------------ the same bits in two runs
def test_loss_values_have_the_same_bits_in_two_runs():
    for c in lc.REPRO:
        runs = []
        for _ in range(2):
            if c["kind"] == "misc":
                inp = lc.misc_inputs(c)
                L, _g = _run_misc(c, inp, _misc_pre(c, inp))
                runs.append(_bits(L)[[0, 3, 4, 5]])
            else:
                call = Call(c)
                loss = torch.zeros(1, device=dev())
                gbufs = [call.stack(g, [torch.zeros_like(t) for t in g], 0.0).to(dev()) for g in call.groups]
                assert call.launch(1.0, loss, gbufs) == 0
                runs.append(_bits(loss))
        assert torch.equal(runs[0], runs[1]), c["name"]
