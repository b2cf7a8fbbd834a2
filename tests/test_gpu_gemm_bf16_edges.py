"""The bf16 grouped GEMM at its edges, on the MI355X: every case of tests/gemm_bf16_cases.py (one kernel instance, one k-slice
pattern, one tile edge or one epilogue pair each -- test_gemm_bf16_plan_cpu.py proves from the launch plan what each case reaches)
against a float64 reference of the same bf16 values.

Every operand and output sits inside a larger buffer.  The output's surroundings (columns N .. ldc, rows below M, bias-gradient
entries past M) are pre-filled with a sentinel that must still be there afterwards, bit for bit.  Three input families:
  a  integer-valued operands: every partial sum is an integer below 2^24, so the result is EXACT in any summation order and the
     assertion is torch.equal -- a k-tile multiplied twice, a stale ring stage, a dropped tail element or a misplaced ones-column
     flips bits;
  b  randn operands, per element |got - ref| <= min(F sqrt(n) u, n u / (1 - n u)) mag with n = K + 8, u = 2^-24, F = 8 and mag the
     same expression on absolute values (an error confined to small outputs or to one element does not hide behind the largest);
  c  family a with NaN in every operand element the contract says is never read (k past the 8-padded depth, tn columns outside
     the windows, k-rows past K): still exact, no NaN in the window.
Each run happens twice on fresh outputs and must give the same bits (deterministic split-K).  Cases under non-default switches
(MMDA_GEMM_DMA_STAGES=3, MMDA_GEMM_DMA_TALL=1: read once per process) run in one fresh child process per switch set."""
import json
import os
import subprocess
import sys
import traceback

import pytest
import torch

import gemm_bf16_cases as gc

pytestmark = pytest.mark.gpu
TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
CHILD_TIMEOUT = 600                                  # seconds, per child process


def families_of(case):
    return ("a", "b", "c") if any(p.get("poison") for p in case["problems"]) else ("a", "b")


def _bits(t):
    return t.view(torch.int32)


def run_case(case, family):
    """One call, twice on fresh outputs.  Returns (failures, {instance: largest |got - ref| / working bar}) -- family b only."""
    from mmda_amd import ops
    dev = torch.device("cuda:0")
    probs = case["problems"]
    datas = [gc.make_data(p, family, gc.seed_of(case, k, family)) for k, p in enumerate(probs)]
    operands = [(d["Abuf"].to(dev), d["Bbuf"].to(dev), {k: d[k].to(dev) for k in ("bias", "bias2") if d[k] is not None}) for d in datas]
    runs = []
    for _ in range(2):
        call, outs = [], []
        for p, d, (Ab, Bb, biases) in zip(probs, datas, operands):
            lay = gc.layout(p)
            M, N = p["M"], p["N"]
            Cd = d["Cbuf"].to(dev)
            grads = {k: d[k + "buf"].to(dev) for k in ("bias_grad", "bias_grad2") if d[k + "buf"] is not None}
            q = dict(K=p["K"], out=Cd[:M, :N], accumulate=bool(p.get("accumulate")), alpha=p.get("alpha", 1.0),
                     perm_n_H=p.get("perm_n_H", 0), perm_m_H=p.get("perm_m_H", 0), **biases, **grads)
            if p["form"] == "nt":
                q.update(A=Ab, B=Bb)
            else:
                q.update(A=Ab[:, lay["a0"]:], B=Bb[:, lay["b0"]:], M=M, N=N, tn=True)
            call.append(q); outs.append((Cd, grads))
        ops.gemm_bf16_grouped(call)
        torch.cuda.synchronize()
        runs.append(outs)
    fails, ratios = [], {}
    for k, (p, d) in enumerate(zip(probs, datas)):
        M, N, inst = p["M"], p["N"], p["expect"]["inst"]
        tag = f"problem {k} ({p['form']} {M}x{N}x{p['K']})"
        (C1, g1), (C2, g2) = runs[0][k], runs[1][k]
        if not torch.equal(_bits(C1), _bits(C2)) or any(not torch.equal(_bits(g1[n]), _bits(g2[n])) for n in g1):
            fails.append(f"{tag}: two runs differ in their bits")
        C_ref, mag, g_ref, _ = gc.reference(p, d)
        got = C1.cpu()
        outside = torch.ones(got.shape, dtype=torch.bool); outside[:M, :N] = False
        bad = int((_bits(got)[outside] != gc.SENTINEL_BITS).sum())
        if bad:
            where = torch.nonzero(outside & (_bits(got) != gc.SENTINEL_BITS))[:4].tolist()
            fails.append(f"{tag}: {bad} elements outside the {M} x {N} window were written, first at (row, column) {where}")
        checks = [("C", got[:M, :N].double(), C_ref, mag)]
        for n, buf in g1.items():
            b = buf.cpu()
            if bool((_bits(b)[M:] != gc.SENTINEL_BITS).any()):
                fails.append(f"{tag}: {n} written past entry M")
            checks.append((n, b[:M].double(), g_ref[n][0], g_ref[n][1]))
        for what, x, ref, mg in checks:
            if not bool(torch.isfinite(x).all()):
                fails.append(f"{tag}: {what} holds {int((~torch.isfinite(x)).sum())} non-finite values")
            elif family != "b":
                if not torch.equal(x, ref):
                    wrong = torch.nonzero(x != ref)
                    fails.append(f"{tag}: {what} differs from the exact result in {len(wrong)} elements, first at {wrong[:4].tolist()}: "
                                 f"got {x[tuple(wrong[0].tolist())].item()}, want {ref[tuple(wrong[0].tolist())].item()}")
            else:
                work, ceil = gc.bars(p["K"], mg, inst)
                err = (x - ref).abs()
                ratio = float((err / work.clamp_min(1e-300)).max())
                ratios[inst] = max(ratios.get(inst, 0.0), ratio)
                if not bool((err <= torch.minimum(work, ceil)).all()):
                    at = tuple(torch.nonzero(err > torch.minimum(work, ceil))[0].tolist())
                    fails.append(f"{tag}: {what} error / working bar = {ratio:.3f}, error / hard ceiling = {float((err / ceil.clamp_min(1e-300)).max()):.3f}, "
                                 f"first at {at}: got {x[at].item()!r}, want {ref[at].item()!r}")
    return fails, ratios


def child_main(switch_name):
    """Runs in the fresh process of a switch set: every case and family of the set, one JSON line each.  Stops at the first error that
    is not a wrong number (nothing more is started on a GPU that may have faulted)."""
    switches = {v: k for k, v in gc.SWITCH_NAME.items()}[switch_name]
    for case in gc.cases_of(switches):
        for family in families_of(case):
            try:
                fails, ratios = run_case(case, family)
            except BaseException:
                traceback.print_exc()
                sys.exit(1)
            print(json.dumps(dict(case=case["name"], family=family, fails=fails, ratios=ratios)), flush=True)


_children = {}


def child_results(switches):
    if switches not in _children:
        name = gc.SWITCH_NAME[switches]
        code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_gemm_bf16_edges as t; t.child_main(%r)" % (ROOT, TESTS, name)
        try:
            r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **gc.ENV[switches]), capture_output=True, text=True,
                               timeout=CHILD_TIMEOUT)
            out, tail = r.stdout, f"exit status {r.returncode}\n{r.stderr[-3000:]}"
        except subprocess.TimeoutExpired as e:
            out = e.stdout.decode() if isinstance(e.stdout, bytes) else (e.stdout or "")
            tail = f"no end after {CHILD_TIMEOUT} s"
        lines = {}
        for line in out.splitlines():
            if line.startswith("{"):
                rec = json.loads(line)
                lines[(rec["case"], rec["family"])] = rec
        _children[switches] = (lines, tail)
    return _children[switches]


PARAMS = [(c, f) for c in gc.CASES for f in families_of(c)]


@pytest.mark.parametrize("case,family", PARAMS, ids=[f"{c['name']}-{f}" for c, f in PARAMS])
def test_gemm_bf16_edge(case, family):
    if case["switches"] == gc.DEFAULT:
        try:
            fails, ratios = run_case(case, family)
        except Exception as e:                           # a launch or the device failed: start nothing more on this GPU
            pytest.exit(f"{case['name']}-{family}: {type(e).__name__}: {e}", returncode=3)
    else:
        lines, tail = child_results(case["switches"])
        rec = lines.get((case["name"], family))
        assert rec is not None, f"the {gc.SWITCH_NAME[case['switches']]} child process printed no result for this case: {tail}"
        fails, ratios = rec["fails"], rec["ratios"]
    for inst, ratio in ratios.items():
        print(f"bf16-edge-ratio {inst} {case['name']} {ratio:.4f}")
    assert not fails, "\n".join(fails)
