"""The resident-weights recurrences in every form the launch plan can pick, on the MI355X: each case of tests/lstm_forms_cases.py
(test_lstm_plan_cpu.py proves from the plan which form, waves per block, launch count and kernel instances it reaches) against
torch.nn.LSTM / nn.GRU in float64 and against the bf16-emulating oracle with the partial-dh rounding of the instance that ran
(tile_partials = 32 for a PAIR = 1 instance, True otherwise).

Per case: the plan the device reports must be the case's `expect` (the test fails instead of testing another form); no exchange may
time out; hseq / final h within 1e-2 of the exact reference and 1e-3 of the oracle (max-norm relative); every gradient -- float64 host
products of the kernel's own dG (or dg_bf16 where only that is written) and hseq, no GEMM kernel -- within 3e-2 of the exact reference
and 1e-2 relative L2 of the oracle; dg_bf16 == round(dG) bit for bit; zeros at padded positions; no NaN left in a window; sentinels
around every buffer intact; the other layer's final-h slots untouched; forward_only = 1 within 1e-5 of the stash run; two runs on fresh
buffers identical in their bits; where a case has a pairing pass, dX of every backward pass nearer to the oracle of its own partial-dh
rounding than to the other's; several descriptors in one launch within 1e-5 of each alone where the plan gives both the same form
and waves per block.  The bounds are test_lstm_fwd_bwd_vs_nn_lstm's.  Cases under MMDA_LSTM_NO_QUAD=1 (read once per process) run
together in one fresh child process.

Not done: the fp32 `gates` cannot start NaN-filled (they carry the input projection into the forward pass); hseq and dg_bf16 do."""
import json
import os
import subprocess
import sys
import traceback

import pytest
import torch

import lstm_forms_cases as lc

pytestmark = pytest.mark.gpu
TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
CHILD_TIMEOUT = 300                                  # seconds, for the child process of a switch set
TOL = 1e-2                                           # tests/test_gpu_ops.py: TOL["bf16"]
SAME = 1e-5                                          # two instances of the same arithmetic


def _rel(got, ref):
    got, ref = got.double(), ref.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-6))


def _l2(got, ref):
    got, ref = got.double(), ref.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float((got - ref).norm() / ref.norm().clamp_min(1e-30))


class Report:
    def __init__(self, name):
        self.name, self.fails, self.margins = name, [], {}

    def bound(self, kernel, what, value, limit):
        """value must be below limit; the worst value / limit per kernel instance and kind of bound -- against the exact reference,
        the oracle, or another instance of the same arithmetic -- is kept for the margin table"""
        kind = "exact" if " against nn." in what else ("oracle" if "oracle" in what else "same")
        ratio = value / limit
        if ratio > self.margins.setdefault(kernel, {}).get(kind, (-1.0, ""))[0]:
            self.margins[kernel][kind] = (ratio, what)
        if not value < limit:
            self.fails.append(f"{what} [{kernel}]: {value:.3e} is not below {limit:.0e}")

    def check(self, ok, what):
        if not ok:
            self.fails.append(what)


def _run_all(c, prep, len_dev, inputs, dev, no_quad):
    return {p: lc.run_pass(c, p, prep, len_dev, inputs, dev, no_quad=no_quad) for p in lc.passes_of(c) if p != "fwd"}


def run_case(c):
    """Every pass of the case, twice.  Returns (failures, {kernel instance: {kind of bound: (worst observed / bound, which check)}})."""
    dev = torch.device("cuda:0")
    no_quad = c["switches"] == lc.NO_QUAD
    R = Report(c["name"])
    inputs, lengths = lc.inputs_of(c["name"])
    prep, len_dev = lc.prepare(c, inputs, lengths, dev)
    T, B, e = c["T"], c["B"], c["expect"]
    first, second = (_run_all(c, prep, len_dev, inputs, dev, no_quad) for _ in range(2))
    mask = torch.arange(T)[:, None] < lengths[None, :]                         # (T, B): inside the sequence
    # 1. the plan the device reports is the one the case is meant for; no exchange timed out
    for p, res in first.items():
        if p.startswith("bwd"):
            R.fails += lc.plan_mismatch(c, "fwd", res["plans"]["fwd"]) + lc.plan_mismatch(c, p, res["plans"]["bwd"])
            R.check(not res["aborted_bwd"], f"{p}: a cluster exchange timed out in the backward call")
        else:
            R.fails += lc.plan_mismatch(c, p, res["plans"]["fwd"])
        R.check(not res["aborted_fwd"], f"{p}: a cluster exchange timed out in the forward call")
    if R.fails:
        return R.fails, R.margins                                              # another form ran, or nothing finished: no numbers
    k_fwd, k_only = e["kernels"]["fwd"], e["kernels"]["fwd_only"]
    for i, inp in enumerate(inputs):
        H, tag = inp["H"], f"descriptor {i} (H = {inp['H']})"
        exact = lc.exact_reference(c, inp, lengths)
        emul = {}

        def oracle(pair):
            tp = 32 if pair else True
            if tp not in emul:
                emul[tp] = lc.emul_reference(c, inp, lengths, tp)
            return emul[tp]

        layer = i % 2
        for p, res in first.items():
            r, r2 = res["descs"][i], second[p]["descs"][i]
            kf = k_only if p == "fwd_only" else k_fwd
            # 3. forward against both references (5.: the forward_only run is held to the same bounds)
            R.bound(kf, f"{tag} {p}: hseq against nn.{c['cell'].upper()}", _rel(r["hseq"], exact["hseq"]), TOL)
            R.bound(kf, f"{tag} {p}: hseq against the oracle", _rel(r["hseq"], oracle(False)["hseq"]), 1e-3)
            for d in range(2):
                R.bound(kf, f"{tag} {p}: final h, direction {d}, against nn.{c['cell'].upper()}", _rel(r["utt"][:, 2 * d + layer], exact["hn"][d]), TOL)
                R.bound(kf, f"{tag} {p}: final h, direction {d}, against the oracle", _rel(r["utt"][:, 2 * d + layer], oracle(False)["hn"][d]), 1e-3)
                # 4. the other layer's slots
                R.check(bool((r["utt"][:, 2 * d + 1 - layer] == lc.UTT_FILL).all()), f"{tag} {p}: final-h slots of the other layer were written")
            R.check(bool((r["hseq"][~mask] == 0).all()), f"{tag} {p}: hseq is not zero at padded positions")
            R.check(not r["broken"], f"{tag} {p}: sentinels overwritten around {r['broken']}")
            if p != "fwd_only":
                R.check(bool(torch.isfinite(r["stash"]).all()) and bool(torch.isfinite(r["cstash"]).all()), f"{tag} {p}: NaN in the stash")
            # 6. two runs, the same bits
            same = ["hseq", "utt"] + (["cstash", "stash"] if p != "fwd_only" else []) + [k for k in ("dG_raw", "dg16_bits") if k in r]
            for k in same:
                a, b = (t.view(torch.int32) if t.dtype == torch.float32 else t for t in (r[k], r2[k]))
                R.check(torch.equal(a, b), f"{tag} {p}: {k} differs between two runs on fresh buffers")
            if not p.startswith("bwd"):
                continue
            kb, key = e["kernels"][p], "nodh" if p == "bwd16_nodh" else "dh"
            mT = mask.reshape(T, B)
            if "dG" in r:
                R.check(bool(torch.isfinite(r["dG"]).all()), f"{tag} {p}: NaN in dG")
                R.check(bool((r["dG"][~mT] == 0).all()), f"{tag} {p}: dG is not zero at padded positions")
            if "dg16" in r:
                R.check(bool(torch.isfinite(r["dg16"]).all()), f"{tag} {p}: NaN left in dg_bf16")
                R.check(bool((r["dg16"][~mT] == 0).all()), f"{tag} {p}: dg_bf16 is not zero at padded positions")
            if "dG" in r and "dg16" in r:
                R.check(torch.equal(r["dg16_bits"], r["dG_raw"].to(torch.bfloat16).view(torch.int16)), f"{tag} {p}: dg_bf16 is not round(dG)")
            # 2. / 3. gradients from the kernel's own outputs
            got = lc.host_gradients(c, inp, r["dG"] if "dG" in r else r["dg16"], r["hseq"])
            orc = oracle(e["pair"][p])["grads"][key]
            for name, g in got.items():
                R.bound(kb, f"{tag} {p}: {name} against nn.{c['cell'].upper()}", _rel(g, exact["grads"][key][name]), 3 * TOL)
                R.bound(kb, f"{tag} {p}: {name} against the oracle (relative L2)", _l2(g, orc[name]), 1e-2)
            # The 1e-2 above is wider than the distance between the two roundings of the partial dh (test_lstm_plan_cpu.py prints it:
            # ~1e-3 at the largest hidden size), so it alone cannot tell a pairing instance from one that does not pair.  A correct
            # instance differs from its own oracle by summation order only: it must be nearer to that than to the other rounding.
            if any(e["pair"].values()) and H == max(c["Hs"]):
                other = oracle(not e["pair"][p])["grads"][key]["dX"]
                own_d, other_d = _l2(got["dX"], orc["dX"]), _l2(got["dX"], other)
                print(f"lstm-forms-own-oracle {c['name']} {p} H={H}: dX is {own_d:.2e} from its own oracle, {other_d:.2e} from the other")
                R.check(own_d < other_d, f"{tag} {p}: dX is nearer to the oracle of the other partial-dh rounding ({other_d:.2e}) than to "
                                         f"its own ({own_d:.2e}) [{kb}]")
        # 5. forward_only = 1 against the stash run: two instances of the same arithmetic
        a, b = first["fwd_only"]["descs"][i], first["bwd"]["descs"][i]
        R.bound(k_only, f"{tag}: hseq, forward_only against the stash run", _rel(a["hseq"], b["hseq"]), SAME)
        R.bound(k_only, f"{tag}: final h, forward_only against the stash run", _rel(a["utt"], b["utt"]), SAME)
        # 7. the same descriptor launched alone, where the plan gives it the same form and waves per block
        if len(inputs) > 1:
            alone = lc.run_pass(c, "bwd", prep, len_dev, inputs, dev, only=i, no_quad=no_quad)
            R.check(not (alone["aborted_fwd"] or alone["aborted_bwd"]), f"{tag}: a cluster exchange timed out in the launch of its own")
            for call, keys, kernel in (("fwd", ("hseq", "utt", "cstash"), k_fwd), ("bwd", ("dG",), e["kernels"]["bwd"])):
                mine, theirs = alone["plans"][call], first["bwd"]["plans"][call]
                if (mine["form"], mine["wpb"]) != (theirs["form"], theirs["wpb"]):
                    print(f"lstm-forms-alone {c['name']} {tag} {call}: alone it runs {mine['form']} at {mine['wpb']}, not compared")
                    continue
                for k in keys:
                    R.bound(kernel, f"{tag}: {k}, one launch against a launch of its own", _rel(b[k], alone["descs"][0][k]), SAME)
    return R.fails, R.margins


def child_main(switch_name):
    """Runs in the fresh process of a switch set: every case of the set, one JSON line each.  Stops at the first error that is not a
    wrong number (nothing more is started on a GPU that may have faulted)."""
    for c in lc.cases_of(switch_name):
        try:
            fails, margins = run_case(c)
        except BaseException:
            traceback.print_exc()
            sys.exit(1)
        print(json.dumps(dict(case=c["name"], fails=fails, margins=margins)), flush=True)


_children = {}


def child_results(switches):
    if switches not in _children:
        code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_lstm_forms as t; t.child_main(%r)" % (ROOT, TESTS, switches)
        try:
            r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **lc.ENV[switches]), capture_output=True, text=True,
                               timeout=CHILD_TIMEOUT)
            out, tail = r.stdout, f"exit status {r.returncode}\n{r.stderr[-3000:]}"
        except subprocess.TimeoutExpired as e:
            out = e.stdout.decode() if isinstance(e.stdout, bytes) else (e.stdout or "")
            tail = f"no end after {CHILD_TIMEOUT} s"
        lines = {}
        for line in out.splitlines():
            if line.startswith("{"):
                rec = json.loads(line)
                lines[rec["case"]] = rec
        _children[switches] = (lines, tail)
    return _children[switches]


@pytest.mark.parametrize("c", lc.CASES, ids=[c["name"] for c in lc.CASES])
def test_lstm_form(c):
    if c["switches"] == lc.DEFAULT:
        try:
            fails, margins = run_case(c)
        except Exception as e:                           # a launch or the device failed: start nothing more on this GPU
            pytest.exit(f"{c['name']}: {type(e).__name__}: {e}", returncode=3)
    else:
        lines, tail = child_results(c["switches"])
        rec = lines.get(c["name"])
        assert rec is not None, f"the {c['switches']} child process printed no result for this case: {tail}"
        fails, margins = rec["fails"], rec["margins"]
    for kernel, kinds in sorted(margins.items()):
        for kind, (ratio, what) in sorted(kinds.items()):
            print(f"lstm-forms-margin {kernel} | {kind} | {ratio:.3f} of the bound | {c['name']} {what}")
    assert not fails, "\n".join(fails)
