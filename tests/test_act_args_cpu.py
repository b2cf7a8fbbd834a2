"""CPU: the host-side argument checks of every entry point that takes an activation id (include/mmda_hip.h) and of the fp32
GEMM's K.  Each bad call must return MMDA_EINVAL (-1) BEFORE any launch: pointers are dummy non-null integers that are never
dereferenced, and no GPU is needed (a call that got as far as a launch would come back as MMDA_ELAUNCH, -2, here).

Every family runs in a child process: a call that kills the process (the K == 0 division in the launch planner) then reads as a failed
assertion on the child's return code instead of a dead pytest."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PRELUDE = r"""
import ctypes as C, sys
from mmda_amd import _lib
lib = _lib.load()
EINVAL, D = -1, 0x1000                       # D: a non-null, 16-byte aligned pointer that nothing may read
NONE, HARDSHRINK, PRELU, RRELU = (_lib.ACT[k] for k in ("none", "hardshrink", "prelu", "rrelu"))
bad = []
def expect(what, rc):
    if rc != EINVAL:
        bad.append((what, rc))
def done():
    print("BAD", bad) if bad else print("OK")
    sys.exit(1 if bad else 0)
def actp_cases():
    # (name, act, fill(actp)) for every activation argument the LayerNorm / act_dropout entries must refuse
    def rr(lo, hi):
        def f(p): p.lo = lo; p.hi = hi
        return f
    nothing = lambda p: None
    return [("prelu, slope NULL", PRELU, nothing), ("rrelu, zeroed params", RRELU, nothing), ("rrelu, lo > hi", RRELU, rr(0.5, 0.25)),
            ("rrelu, lo < 0", RRELU, rr(-0.125, 0.25)), ("rrelu, nan", RRELU, rr(float("nan"), 0.25)),
            ("act -1", -1, nothing), ("act 10", 10, nothing), ("act 42", 42, nothing)]
"""

LAYERNORM = PRELUDE + r"""
def ln_fwd():
    a = _lib.LnArgs()
    a.rows = 4; a.n = 128; a.x = D; a.gamma = D; a.beta = D; a.y = D; a.mean = D; a.rstd = D; a.eps = 1e-5
    return a
def ln_bwd():
    b = _lib.LnBwdArgs()
    b.rows = 4; b.n = 128; b.dy = D; b.x = D; b.gamma = D; b.mean = D; b.rstd = D; b.d_x = D; b.dgamma = D; b.dbeta = D
    return b
for name, act, fill in actp_cases():
    a = ln_fwd(); a.act = act; fill(a.actp)
    expect("layernorm_fwd: " + name, lib.mmda_layernorm_fwd(C.byref(a), None))
    arr = (_lib.LnArgs * 2)(ln_fwd(), a)                     # a good problem first: the bad one must still stop the launch
    expect("layernorm_fwd_multi: " + name, lib.mmda_layernorm_fwd_multi(arr, 2, None))
    b = ln_bwd(); b.act = act; fill(b.actp)
    expect("layernorm_bwd: " + name, lib.mmda_layernorm_bwd(C.byref(b), None))
    arr = (_lib.LnBwdArgs * 2)(ln_bwd(), b)
    expect("layernorm_bwd_multi: " + name, lib.mmda_layernorm_bwd_multi(arr, 2, None))
    expect("layernorm_param_grads: " + name, lib.mmda_layernorm_param_grads(arr, 2, None))
done()
"""

ACT_DROPOUT = PRELUDE + r"""
for name, act, fill in actp_cases():
    p = _lib.ActParams(); fill(p)
    expect("act_dropout_fwd_p: " + name, lib.mmda_act_dropout_fwd_p(D, D, 256, act, C.byref(p), 0.0, 0, 0, None))
    expect("act_dropout_bwd_p: " + name, lib.mmda_act_dropout_bwd_p(D, D, D, 256, act, C.byref(p), 0.0, 0, 0, None))
for act in (PRELU, RRELU, -1, 10, 42):                       # the unparametrised entries pass no parameters at all
    expect("act_dropout_fwd: act %d" % act, lib.mmda_act_dropout_fwd(D, D, 256, act, 0.0, 0, 0, None))
    expect("act_dropout_bwd: act %d" % act, lib.mmda_act_dropout_bwd(D, D, D, 256, act, 0.0, 0, 0, None))
done()
"""

GEMM_HEAD = PRELUDE + r"""
def gemm(act=NONE, K=32, M=16):
    g = _lib.GemmArgs()
    g.mode = _lib.F32; g.transB = 1; g.M = M; g.N = 16; g.K = K; g.batch = 1
    g.A = D; g.lda = 32; g.B = D; g.ldb = 32; g.C = D; g.ldc = 16; g.act = act
    return g
"""

GEMM_ACT = GEMM_HEAD + r"""
def skinny(act):
    g = _lib.SkinnyArgs()
    g.M = 16; g.N = 16; g.K = 32; g.transB = 1; g.A = D; g.lda = 32; g.B = D; g.ldb = 32; g.C = D; g.ldc = 16; g.act = act
    return g
def mx8(act):
    g = _lib.Mx8Args()
    g.M = 16; g.N = 16; g.K = 128; g.Aq = D; g.As = D; g.Bq = D; g.Bs = D; g.C = D; g.ldc = 16; g.act = act
    return g
for act in (PRELU, RRELU, -1, 42):
    for mode in (_lib.F32, _lib.BF16):
        g = gemm(act); g.mode = mode
        expect("gemm mode %d: act %d" % (mode, act), lib.mmda_gemm(C.byref(g), None))
        arr = (_lib.GemmArgs * 2)(gemm(), g)
        expect("gemm_grouped mode %d: act %d" % (mode, act), lib.mmda_gemm_grouped(arr, 2, None))
    arr = (_lib.SkinnyArgs * 2)(skinny(NONE), skinny(act))
    expect("gemm_skinny: act %d" % act, lib.mmda_gemm_skinny(arr, 2, None))
    m = mx8(act)
    expect("gemm_mx8: act %d" % act, lib.mmda_gemm_mx8(C.byref(m), None))
done()
"""

GEMM_K0 = GEMM_HEAD + r"""
for K in (0, -1):
    g = gemm(K=K)
    expect("gemm: K = %d" % K, lib.mmda_gemm(C.byref(g), None))
    arr = (_lib.GemmArgs * 2)(gemm(), gemm(K=K))
    expect("gemm_grouped: K = %d" % K, lib.mmda_gemm_grouped(arr, 2, None))
# an EMPTY problem keeps what it returned before: nothing to compute is MMDA_OK, whatever its K
g = gemm(K=0, M=0)
if lib.mmda_gemm(C.byref(g), None) != 0:
    bad.append(("gemm: empty problem with K = 0 is MMDA_OK", None))
arr = (_lib.GemmArgs * 1)(g)
if lib.mmda_gemm_grouped(arr, 1, None) != 0:
    bad.append(("gemm_grouped: empty problem with K = 0 is MMDA_OK", None))
done()
"""


def run_child(code):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=ROOT)
    assert r.returncode == 0, f"child returned {r.returncode}\n{r.stdout}\n{r.stderr[-2000:]}"


@pytest.mark.parametrize("family", ["LAYERNORM", "ACT_DROPOUT", "GEMM_ACT", "GEMM_K0"])
def test_bad_activation_arguments_and_k_are_refused_before_any_launch(family):
    run_child(globals()[family])
