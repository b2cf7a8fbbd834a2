"""The fp32-operand GEMMs at their edges, on the MI355X: every case of tests/gemm_f32_cases.py (one kernel instance, one k-slice
pattern, one tile edge, one reduce form or one epilogue feature each -- test_gemm_f32_plan_cpu.py proves from the launch plan what each
case reaches) against a float64 reference of the values the kernel multiplies.  mmda_gemm, mmda_gemm_grouped, the split-K reduce
behind them, mmda_gemm_skinny and mmda_colsum.

Every operand and output sits inside a larger buffer.  The output's surroundings (columns N .. ldc, rows below M, the floats before an
offset base, bias-gradient entries past M) are pre-filled with a sentinel that must still be there afterwards, bit for bit.  Three
input families:
  a  integer-valued operands in [-8, 8], small-integer C0 / biases, alpha in {1, -0.5, 0}, gate scale and dropout multiplier 2: every
     partial sum is a multiple of a small binary fraction below 2^24, in fp32 and in bf16 mode, so the result is EXACT in any summation
     order and the assertion is torch.equal -- one dropped k element, a k-tile counted twice, a stale prefetch stage or a wrong
     ones-column entry flips bits;
  b  randn operands (bf16 mode: the reference multiplies the bf16-rounded values), per element |got - ref| <= min(F sqrt(n) u,
     n u / (1 - n u)) mag with n = K + 8 (column sums: M + 8), u = 2^-24, F = 8 and mag the same expression on absolute values;
  c  family a with NaN in every element the contract says is never read (columns past K up to the leading dimension, rows past M / N,
     k-rows past K of the transposed layouts, A2 and gate padding; the gather array is M entries long and followed by an out-of-range
     index): still exact, no NaN in the window.
Each case runs twice on fresh outputs and must give the same bits.  Dropout masks come from oracle/dropout_rng.py."""
import ctypes as C

import pytest
import torch

import gemm_f32_cases as gc

pytestmark = pytest.mark.gpu
DEVICE = "cuda:0"


def _bits(t):
    return t.view(torch.int32)


def _compare(tag, what, got, ref, mag, family, terms, fails):
    """got, ref, mag: (nb, rows, cols) or (nb, n) float64.  Returns the largest error / working bar (family b), else 0"""
    if not bool(torch.isfinite(got).all()):
        at = torch.nonzero(~torch.isfinite(got))[0].tolist()
        fails.append(f"{tag}: {what} holds {int((~torch.isfinite(got)).sum())} non-finite values, first at (batch, row, column) {at}")
        return 0.0
    if family != "b":
        if not torch.equal(got, ref):
            wrong = torch.nonzero(got != ref)
            at = tuple(wrong[0].tolist())
            fails.append(f"{tag}: {what} differs from the exact result in {len(wrong)} elements, first at (batch, row, column) {list(at)}: "
                         f"got {got[at].item()!r}, want {ref[at].item()!r}")
        return 0.0
    work, ceil = gc.bars(terms, mag)
    err = (got - ref).abs()
    ratio = float((err / work.clamp_min(1e-300)).max()) if err.numel() else 0.0
    bad = err > torch.minimum(work, ceil)
    if bool(bad.any()):
        at = tuple(torch.nonzero(bad)[0].tolist())
        fails.append(f"{tag}: {what} error / working bar = {ratio:.3f}, error / hard ceiling = {float((err / ceil.clamp_min(1e-300)).max()):.3f}, "
                     f"first at (batch, row, column) {list(at)}: got {got[at].item()!r}, want {ref[at].item()!r}")
    return ratio


def _window_check(tag, what, buf, flat, fails):
    """The window of an output buffer as float64, after checking that everything around it still holds the sentinel"""
    outside = buf.outside()
    bad = outside & (_bits(flat) != gc.SENTINEL_BITS)
    if bool(bad.any()):
        first = int(torch.nonzero(bad)[0])
        rel = (first - buf.off) % buf.stride if buf.nb > 1 else first - buf.off
        fails.append(f"{tag}: {int(bad.sum())} floats of {what} outside the {buf.rows} x {buf.cols} window were written, first at flat offset "
                     f"{first} (row {rel // buf.ld}, column {rel % buf.ld} of its matrix)")
    return buf.window(flat).double()


def _vector_check(tag, what, got, n, fails):
    if bool((_bits(got)[:, n:] != gc.SENTINEL_BITS).any()):
        fails.append(f"{tag}: {what} written past entry {n}")
    return got[:, :n].double()


def _upload(d, names, dev):
    out = {}
    for n in names:
        v = d.get(n + "buf") if n != "gather" else d.get("gather")
        if v is not None:
            out[n] = (v.flat if isinstance(v, gc.Buf) else v).to(dev)
    return out


def _addr(tensors):
    return {n: t.data_ptr() for n, t in tensors.items()}


def launch(case, probs, datas, addrs, fresh):
    """The call of a case on the device buffers at `addrs` (one {buffer name: address} per problem)"""
    from mmda_amd import _lib
    lib = _lib.load()
    if case["call"] in ("gemm", "grouped"):
        arr = (_lib.GemmArgs * len(probs))(*[gc.gemm_args(p, a) for p, a in zip(probs, addrs)])
        if case["call"] == "grouped":
            _lib.check(lib.mmda_gemm_grouped(arr, len(probs), _lib.stream_ptr()), "mmda_gemm_grouped")
        else:
            for g in arr:
                _lib.check(lib.mmda_gemm(C.byref(g), _lib.stream_ptr()), "mmda_gemm")
    elif case["call"] == "skinny":
        for p, a in zip(probs, addrs):
            assert gc.skinny_forms(p, a) == (p["expect"]["form"], p["expect"]["second"]), "the device buffers' alignment gives another form"
        arr = (_lib.SkinnyArgs * len(probs))(*[gc.skinny_args(p, a) for p, a in zip(probs, addrs)])
        _lib.check(lib.mmda_gemm_skinny(arr, len(probs), _lib.stream_ptr()), "mmda_gemm_skinny")
    else:
        for p, d, a in zip(probs, datas, addrs):
            _lib.check(lib.mmda_colsum(a["X"], d["Xbuf"].ld, p["M"], p["N"], a["out"], a.get("out2"), _lib.stream_ptr()), "mmda_colsum")


def run_case(case, family):
    """One call, twice on fresh outputs.  Returns (failures, {instance: largest |got - ref| / working bar}) -- family b only."""
    dev = torch.device(DEVICE)
    probs = case["problems"]
    make = {"gemm": gc.make_gemm, "skinny": gc.make_skinny, "colsum": gc.make_colsum}
    datas = [make[p["kind"]](p, family, gc.seed_of(case, k, family)) for k, p in enumerate(probs)]
    ins = {"gemm": ("A", "A2", "B", "bias", "bias2", "gate", "gather"), "skinny": ("A", "A2", "B", "A_2nd", "B_2nd", "bias", "gate", "dsig", "dsig2"),
           "colsum": ("X",)}
    outs = {"gemm": ("C", "bias_grad", "bias_grad2"), "skinny": ("C", "C2"), "colsum": ("out", "out2")}
    operands = [_upload(d, ins[p["kind"]], dev) for p, d in zip(probs, datas)]
    runs = []
    for _ in range(2):
        fresh = [_upload(d, outs[p["kind"]], dev) for p, d in zip(probs, datas)]
        addrs = [dict(_addr(o), **_addr(f)) for o, f in zip(operands, fresh)]
        launch(case, probs, datas, addrs, fresh)
        torch.cuda.synchronize()
        runs.append([{n: t.cpu() for n, t in f.items()} for f in fresh])
    fails, ratios = [], {}
    for k, (p, d) in enumerate(zip(probs, datas)):
        M, N = p["M"], p["N"]
        tag = f"problem {k} ({p['kind']} {p.get('mode', '')} {p.get('form', '')} {M}x{N}x{p.get('K', '')}" + (f" batch {p['batch']})" if p.get("batch", 1) > 1 else ")")
        r1, r2 = runs[0][k], runs[1][k]
        if any(not torch.equal(_bits(r1[n]), _bits(r2[n])) for n in r1):
            fails.append(f"{tag}: two runs differ in their bits")
        terms = gc.terms_of(p)
        checks = []
        if p["kind"] == "gemm":
            inst = p["expect"]["inst"]
            C_ref, mag, grads = gc.ref_gemm(p, d)
            checks.append(("C", _window_check(tag, "C", d["Cbuf"], r1["C"], fails), C_ref, mag))
            for n, (g, gm) in grads.items():
                checks.append((n, _vector_check(tag, n, r1[n], M, fails), g, gm))
        elif p["kind"] == "skinny":
            inst = f"skinny/{'nt' if p['tb'] else 'nn'}/{p['expect']['form']}"
            C_ref, mag, C2_ref, mag2 = gc.ref_skinny(p, d)
            checks.append(("C", _window_check(tag, "C", d["Cbuf"], r1["C"], fails), C_ref, mag))
            if C2_ref is not None:
                checks.append(("C2", _window_check(tag, "C2", d["C2buf"], r1["C2"], fails), C2_ref, mag2))
        else:
            inst = "colsum"
            for n, (v, vm) in gc.ref_colsum(p, d).items():
                checks.append((n, _vector_check(tag, n, r1[n], N, fails), v[None], vm[None]))
        if inst is None:
            continue
        for what, got, ref, mg in checks:
            ratio = _compare(tag, what, got, ref, mg, family, terms, fails)
            if family == "b":
                ratios[inst] = max(ratios.get(inst, 0.0), ratio)
    return fails, ratios


PARAMS = [(c, f) for c in gc.CASES for f in gc.families_of(c)]


@pytest.mark.parametrize("case,family", PARAMS, ids=[f"{c['name']}-{f}" for c, f in PARAMS])
def test_gemm_f32_edge(case, family):
    try:
        fails, ratios = run_case(case, family)
    except AssertionError:
        raise
    except Exception as e:                               # a launch or the device failed: start nothing more on this GPU
        pytest.exit(f"{case['name']}-{family}: {type(e).__name__}: {e}", returncode=3)
    for inst, ratio in ratios.items():
        print(f"f32-edge-ratio {inst} {case['name']} {ratio:.4f}")
    assert not fails, "\n".join(fails)
