"""GPU: the heads and the three small losses (cls, conf, recon) give the bits that tests/golden/losses_bits.npz recorded from the build
before their element terms (loss_terms.h) and block-level bodies (losses.hip) replaced the copies that each launch carried.  The other
bitwise tests hold the launches of one build to each other (fused seeds == the loss launch, fused heads == stand-alone heads), so a
mistake the copies share would pass them all; this one holds each entry point to a recording.  tests/golden/gen_losses_bits.py made the
fixture and owns the list of calls: replay() runs it here on the build under test, once for the whole module.  Reference: the recorded
outputs, compared bit pattern by bit pattern -- no tolerance.

The last test holds the one-launch entry (mmda_loss_misc) to the stand-alone entries (mmda_loss_cls, mmda_loss_conf, mmda_loss_recon)
on the build under test: they run the same bodies, so from cleared buffers they leave the same bits -- but for d_scores, which two
terms add into (see there)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import losses_cases as lc
from mmda_amd import _lib, ops

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("gen_losses_bits", os.path.join(GOLDEN, "gen_losses_bits.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def bits():
    z = np.load(gen.FIXTURE, allow_pickle=False)
    inp = {k[4:]: z[k] for k in z.files if k.startswith("in::")}
    want = {k[5:]: z[k] for k in z.files if k.startswith("out::")}
    got = gen.replay(inp)
    assert set(got) == set(want) | set(gen.DERIVED)
    return inp, want, got


def _same_bits(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape and a.dtype.itemsize in (4, 8)
    as_int = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int32 if x.dtype.itemsize == 4 else np.int64))
    return torch.equal(as_int(a), as_int(b))


def _assert_equal(bits, prefix, expect):
    _, want, got = bits
    keys = sorted(k for k in want if k.startswith(prefix))
    assert len(keys) == expect, keys
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert _same_bits(got[k], want[k]), (k, int((got[k] != want[k]).sum()))


@pytest.mark.parametrize("B, ncls", gen.CLS_SHAPES)
def test_loss_cls_gives_the_recorded_bits(bits, B, ncls):
    """plain and weighted / focal, scale 0.7: value and gradient onto pre-filled buffers, the gradient alone, the value alone"""
    _assert_equal(bits, f"cls{B}x{ncls}::", 2 * (2 + 1 + 1))
    inp, _, got = bits
    k = f"cls{B}x{ncls}"
    for tag in ("plain", "opts"):
        assert _same_bits(got[f"{k}::{tag}::no_loss::ds"], got[f"{k}::{tag}::ds"]) and _same_bits(got[f"{k}::{tag}::no_ds::loss"], got[f"{k}::{tag}::loss"])
        assert not np.array_equal(got[f"{k}::{tag}::ds"], inp[f"{k}::pre"])
    assert not np.array_equal(got[f"{k}::plain::ds"], got[f"{k}::opts::ds"])


@pytest.mark.parametrize("B", gen.CONF_B)
def test_loss_conf_gives_the_recorded_bits(bits, B):
    """scale 0.3 onto pre-filled gradients of the scores and of tcp; the value alone"""
    _assert_equal(bits, f"conf{B}::", 3 + 1)
    _, _, got = bits
    assert _same_bits(got[f"conf{B}::no_grads::loss"], got[f"conf{B}::loss"])


def test_loss_recon_gives_the_recorded_bits(bits):
    """contiguous at 3, 258 and 16386 elements (one, two and the capped 64 workgroups) and three strided launches, onto pre-filled
    gradients; the gaps of the strided buffers keep what they held"""
    shapes = gen.RECON_SHAPES + (gen.RECON_FORMULA,)
    for B, D in shapes:
        _assert_equal(bits, f"recon{B}x{D}::", 3)
    _assert_equal(bits, "recon_strided::", 3)
    inp, _, got = bits
    B, D, stride = gen.RECON_STRIDED
    for name in ("rec", "org"):
        g, pre = got[f"recon_strided::d_{name}"], inp[f"recon_strided::pre_{name}"]
        gap = (np.arange(3 * stride) % stride) >= B * D
        assert gap.sum() == 3 * (stride - B * D) and np.array_equal(g[gap], pre[gap]) and not (g[~gap] == pre[~gap]).any()


def test_loss_misc_gives_the_recorded_bits(bits):
    """every (with_conf, conf_grads, use_conf) at two recon workgroups, n_recon = 1 and 2048, the weighted / focal criterion, and the
    capped grid's second trip (d_recon / d_orig as wrap-around sums of their bit patterns)"""
    first = 3 + 2
    _assert_equal(bits, "misc2049::", first + 3 * (len(gen.MISC_COMBOS) - 1) + 3)
    for n in gen.MISC_N:
        _assert_equal(bits, f"misc{n}::", 3 + 2)
    _assert_equal(bits, "misc_large::", 3 + 1)
    _, _, got = bits
    for k in gen.DERIVED:                                 # the recon role sees neither the conf switches nor the criterion
        assert _same_bits(got[k], got[gen.MISC_FIRST + k[k.rindex("::"):]]), k
    total = lambda tag: got[f"misc2049::{tag}::L"][5]
    assert total("w1g1u1") != total("w1g1u0") and total("w0g0u1") == total("w0g0u0")
    assert not got["misc2049::w1g0u1::d_tcp"].any() and got["misc2049::w1g1u1::d_tcp"].any()
    assert gen.MISC_LARGE_N > 64 * 2048


@pytest.mark.parametrize("B, ncls", gen.HEAD_SHAPES)
def test_heads_give_the_recorded_bits(bits, B, ncls):
    """tcp, scores, labels and d_logits (with and without d_tcp), class-score dropout off and at 0.5"""
    _assert_equal(bits, f"heads{B}x{ncls}::", len(gen.HEAD_DROP) * (3 + 1 + 1))
    _, _, got = bits
    k = f"heads{B}x{ncls}"
    (p0, _, _), (p1, _, _) = gen.HEAD_DROP
    assert _same_bits(got[f"{k}::p{p0}::fwd::tcp"], got[f"{k}::p{p1}::fwd::tcp"])           # dropout is on the class scores only
    assert not np.array_equal(got[f"{k}::p{p0}::fwd::scores"], got[f"{k}::p{p1}::fwd::scores"])
    assert not got[f"{k}::p{p1}::bwd_no_dtcp::dlogits"][:, :6].any()


# ------------------------------------------------------------------------------------------------ one launch == the stand-alone entries
# n_recon = 3 D over one (B = 1, D) tensor triple.  192: one recon workgroup in either entry; 131079: 64 in either (the capped grids),
# the large formula case at the nearest multiple of three (mmda_loss_recon takes three tensors of equal size).
@pytest.mark.parametrize("D", [64, 43693])
def test_the_one_launch_entry_and_the_stand_alone_entries_give_the_same_bits(bits, D):
    lib = _lib.load()
    p, st = _lib.ptr, _lib.stream_ptr()
    B, ncls, n = gen.MISC_B, gen.MISC_NCLS, 3 * D
    f = ops.loss_forms(1, D, n_recon=n)
    assert f["recon_blocks"] == f["misc_recon_blocks"] == (1 if D == 64 else 64)
    inp = bits[0]
    dev = lambda name: torch.from_numpy(inp[name]).to(gen.DEV)
    s, t, y = dev("misc::s"), dev("misc::t"), dev("misc::y")
    rec, org, _, _ = gen.formula_inputs(n)
    c, r = gen.MISC_W["conf_scale"], gen.MISC_W["recon_scale"]
    zeros = lambda: (torch.zeros_like(s), torch.zeros_like(t), torch.zeros_like(rec), torch.zeros_like(org), torch.zeros(8, device=gen.DEV))
    one = zeros()
    gen.misc_call(lib, s, t, y, one[0], one[1], 1, 1, 1, rec, org, one[2], one[3], one[4])
    sep = zeros()
    L = sep[4].data_ptr()
    _lib.check(lib.mmda_loss_cls(p(s), p(y), B, ncls, 1.0, L, p(sep[0]), st), "mmda_loss_cls")
    _lib.check(lib.mmda_loss_conf(p(s), p(t), p(y), B, ncls, c, L + 16, p(sep[0]), p(sep[1]), st), "mmda_loss_conf")
    _lib.check(lib.mmda_loss_recon(p(rec), p(org), D, 1, D, r, L + 12, p(sep[2]), p(sep[3]), st), "mmda_loss_recon")
    torch.cuda.synchronize()
    for name, a, b in list(zip(("d_scores", "d_tcp", "d_recon", "d_orig"), one, sep))[1:]:
        assert a.abs().max() > 0 and torch.equal(a.view(torch.int32), b.view(torch.int32)), name
    # d_scores: cls and conf both add into it.  The stand-alone conf kernel's `+=` contracts scale * g + d_scores into one fma; the one
    # launch adds the rounded product atomically.  Measured at the commit before the shared bodies (and after them): 6 of 30 elements
    # differ, by one unit in the last place each.  So this field is held to the float64 bound of losses_cases.check instead, in both entries.
    ulps = (one[0].view(torch.int32) - sep[0].view(torch.int32)).abs()
    print(f"losses-bits d_scores D={D}: {int((ulps != 0).sum())} of {ulps.numel()} elements differ, by at most {int(ulps.max())} ulp")
    ref_inp = dict(gen.MISC_W, s=s.cpu(), t=t.cpu(), y=y.cpu(), rec=rec.cpu()[None], org=org.cpu()[None])
    case = dict(with_conf=1, conf_grads=1, use_conf=1)
    g64 = lc.misc_reference(case, ref_inp, torch.float64)[1]["d_scores"]
    g32 = lc.misc_reference(case, ref_inp, torch.float32)[1]["d_scores"]
    e32 = lc.errors(None, [g32], None, [g64], "grad_conf")
    for tag, a in (("one-launch", one[0]), ("stand-alone", sep[0])):
        bad = lc.check("misc", f"bits-D{D}-d_scores-{tag}", lc.errors(None, [a], None, [g64], "grad_conf"), e32)
        assert not bad, "\n".join(bad)
    for i, name in ((0, "cls"), (4, "conf"), (3, "recon")):
        print(f"losses-bits L[{i}] ({name}) D={D}: one launch {float(one[4][i])!r}  stand-alone {float(sep[4][i])!r}")
        assert one[4][i] != 0 and torch.equal(one[4][i].view(torch.int32), sep[4][i].view(torch.int32)), name
