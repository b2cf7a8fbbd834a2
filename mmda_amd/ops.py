"""Thin per-operator wrappers over the C ABI (one function per entry point of include/mmda_hip.h).

These take/return torch CUDA tensors purely as device-memory handles; all arithmetic is in libmmda_hip.so.
Used by the parity tests (tests/test_gpu_ops.py) and available to callers who want single kernels.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import ACT, BF16, F32, check, load, ptr, stream_ptr

MODE = {"fp32": F32, "bf16": BF16, F32: F32, BF16: BF16}


def _f(t):
    assert t.is_cuda and t.dtype == torch.float32 and (t.is_contiguous() or (t.dim() == 2 and t.stride(1) == 1)), \
        "expect contiguous (or row-strided 2-D) fp32 CUDA tensors"
    return t


def _buf(t):
    """Device pointer of an fp32 operand; an empty view (a problem with no rows) still names the buffer it was sliced from."""
    return ptr(_f(t)) or t.untyped_storage().data_ptr() + 4 * t.storage_offset()


def _gemm_args(A, B, *, mode="fp32", transA=False, transB=True, bias=None, bias2=None, out=None, accumulate=False, act="none",
               A2=None, gather=None, alpha=1.0, drop_p=0.0, seed=0, site=0, gate=None, gate_scale=1.0, bias_grad=None, bias_grad2=None):
    """The mmda_gemm_args of one problem and its output tensor (allocated here unless given)."""
    batched = A.dim() == 3
    Ab = A if batched else A.unsqueeze(0)
    Bb = B if B.dim() == 3 else B.unsqueeze(0)
    nb = max(Ab.shape[0], Bb.shape[0])
    if gather is not None:
        M = gather.numel(); K = Ab.shape[2]
    elif transA:
        K, M = Ab.shape[1], Ab.shape[2]
    else:
        M, K = Ab.shape[1], Ab.shape[2]
    N = Bb.shape[1] if transB else Bb.shape[2]
    if out is None:
        out = torch.zeros((nb, max(M, 1), N), device=A.device, dtype=torch.float32)[:, :M]
        if not batched and B.dim() == 2:
            out = out[0]
    Cb = out if out.dim() == 3 else out.unsqueeze(0)
    g = _lib.GemmArgs()
    g.mode = MODE[mode]; g.transA = int(transA); g.transB = int(transB); g.M = M; g.N = N; g.K = K; g.batch = nb
    g.A = _buf(Ab); g.lda = Ab.shape[2]; g.strideA = Ab.stride(0) if Ab.shape[0] > 1 else 0
    g.A2 = ptr(A2); g.gather = ptr(gather)
    g.B = _buf(Bb); g.ldb = Bb.shape[2]; g.strideB = Bb.stride(0) if Bb.shape[0] > 1 else 0
    g.C = _buf(Cb); g.ldc = N; g.strideC = Cb.stride(0) if Cb.shape[0] > 1 else 0
    g.bias = ptr(bias); g.bias2 = ptr(bias2)
    g.strideBias = (bias.stride(0) if (bias is not None and bias.dim() == 2) else 0)
    g.accumulate = int(accumulate); g.act = ACT[act]
    g.drop_p = drop_p; g.drop_seed = seed; g.drop_site = site
    g.gate = ptr(gate); g.ldgate = N; g.gate_scale = gate_scale; g.alpha = alpha
    g.bias_grad = ptr(bias_grad); g.bias_grad2 = ptr(bias_grad2)
    if bias_grad is not None and bias_grad.dim() == 2:
        g.strideBias = bias_grad.stride(0)
    return g, out


def gemm(A, B, **kw):
    """C = act(alpha * opA(A (+A2)) @ opB(B) + bias + bias2 (+C)).  A,B 2-D or 3-D (batched, uniform strides).
    Keywords: see _gemm_args."""
    g, out = _gemm_args(A, B, **kw)
    check(load().mmda_gemm(C.byref(g), stream_ptr()), "mmda_gemm")
    return out


def gemm_grouped(problems):
    """mmda_gemm_grouped: independent GEMMs (any shapes, layouts, modes) in one launch per 16.  problems: list of dicts with A, B
    and the keywords of gemm().  Returns the outputs."""
    built = [_gemm_args(p["A"], p["B"], **{k: v for k, v in p.items() if k not in ("A", "B")}) for p in problems]
    arr = (_lib.GemmArgs * len(built))(*[g for g, _ in built])
    check(load().mmda_gemm_grouped(arr, len(built), stream_ptr()), "mmda_gemm_grouped")
    return [out for _, out in built]


GEMM_CLASSES = ("Tile64", "Tile64Tiny", "Tile128", "GroupSlot")
GEMM_REDUCE = (None, "scalar", "vector")


def gemm_plan(problems, grouped=False):
    """What mmda_gemm (each problem a call of its own) or, grouped, mmda_gemm_grouped would launch for these problems
    (mmda_gemm_plan_describe: host code only, works without a GPU).  problems: _lib.GemmArgs structures, or dicts of their field names
    (pointer fields as integers: only their alignment matters; batch defaults to 1, A / B / C to an aligned address).  Returns (rows,
    launches): one dict per problem -- cls (a name of GEMM_CLASSES, None for an empty problem), mode, ta, tb, tx, ty, sk, per, last, ldn,
    blocks, launch, slab_off, reduce (None, "scalar" or "vector") -- and the number of GEMM launches."""
    arr = (_lib.GemmArgs * max(1, len(problems)))()
    for k, p in enumerate(problems):
        if isinstance(p, _lib.GemmArgs):
            C.memmove(C.byref(arr[k]), C.byref(p), C.sizeof(_lib.GemmArgs))
            continue
        g = arr[k]
        g.batch = 1; g.A = g.B = g.C = 1 << 20
        for name, v in p.items():
            setattr(g, name, v)
    rows = (_lib.GemmPlanRow * max(1, len(problems)))()
    n = load().mmda_gemm_plan_describe(arr, len(problems), int(bool(grouped)), rows, len(problems))
    if n < 0:
        check(n, "mmda_gemm_plan_describe")
    return [dict(cls=GEMM_CLASSES[r.cls] if r.cls >= 0 else None, mode=r.mode, ta=bool(r.ta), tb=bool(r.tb), tx=r.tx, ty=r.ty, sk=r.sk,
                 per=r.per, last=r.last, ldn=r.ldn, blocks=r.blocks, launch=r.launch, slab_off=r.slab_off, reduce=GEMM_REDUCE[r.reduce])
            for r in rows[:len(problems)]], n


def convert_bf16(jobs):
    """jobs: list of (src[rows, cols] fp32 or bf16, gather or None, want_plain, want_transposed) -> list of (plain, transposed) bf16 tensors.

    plain is [rows, round_up(cols, 8)], transposed is [cols, round_up(rows, 8)], both zero padded; one launch for all jobs."""
    lib = load()
    arr = (_lib.ConvertJob * len(jobs))()
    outs = []
    for j, (src, gather, want_p, want_t) in zip(arr, jobs):
        rows = gather.numel() if gather is not None else src.shape[0]
        cols = src.shape[1]
        ldp, ldt = (cols + 7) // 8 * 8, (rows + 7) // 8 * 8
        # filled with NaN patterns so that a padding element the kernel forgot shows up in the tests
        P = torch.full((rows, ldp), float("nan"), device=src.device, dtype=torch.bfloat16) if want_p else None
        T = torch.full((cols, ldt), float("nan"), device=src.device, dtype=torch.bfloat16) if want_t else None
        if src.dtype == torch.bfloat16:                 # re-layout of an existing bf16 matrix (row stride = its leading dimension)
            assert src.is_cuda and src.stride(1) == 1
            j.src = ptr(src); j.ld = src.stride(0); j.src_bf16 = 1
        else:
            j.src = ptr(_f(src)); j.ld = src.shape[1]
        j.rows = rows; j.cols = cols; j.gather = ptr(gather)
        j.plain = ptr(P); j.ldp = ldp; j.transposed = ptr(T); j.ldt = ldt
        outs.append((P, T))
    check(lib.mmda_convert_bf16(arr, len(jobs), stream_ptr()), "mmda_convert_bf16")
    return outs


def _gemm_bf16_args(problems, plan_only=False):
    """The mmda_gemm_bf16_args array of a call and its output tensors (allocated here unless given).  plan_only: nothing is allocated,
    and a problem may stand in for its operands by shape alone -- lda / ldb instead of A / B, optional A_addr / B_addr / C_addr / ldc
    (integers; only their alignment matters), True for a bias / bias_grad that would be given."""
    FAKE = 1 << 20

    def addr(t):
        if plan_only and (t is None or isinstance(t, (bool, int))):
            return (FAKE if t is True else int(t)) if t else None
        return ptr(t)

    arr = (_lib.GemmBf16Args * len(problems))()
    outs = []
    for g, p in zip(arr, problems):
        A, B = p.get("A"), p.get("B")
        tn = bool(p.get("tn", False))
        if plan_only and A is None:
            M, N, K, lda, ldb = p["M"], p["N"], p["K"], p["lda"], p["ldb"]
            g.A = p.get("A_addr", FAKE); g.B = p.get("B_addr", FAKE)
        else:
            assert A.dtype == torch.bfloat16 and B.dtype == torch.bfloat16 and (tn or (A.is_contiguous() and B.is_contiguous()))
            # tn: A is (K, lda) with M <= lda columns in use, B is (K, ldb): C = A[:K, :M]^T @ B[:K, :N]
            M, N, K = (p["M"], p["N"], p["K"]) if tn else (A.shape[0], B.shape[0], p["K"])
            lda, ldb = (A.stride(0), B.stride(0)) if tn else (A.shape[1], B.shape[1])
            g.A = ptr(A); g.B = ptr(B)
        g.tn = int(tn); g.perm_m_H = int(p.get("perm_m_H", 0)); g.perm_n_H = int(p.get("perm_n_H", 0))
        out = p.get("out")
        if out is None and not plan_only:
            out = torch.zeros((M, N), device=A.device, dtype=torch.float32)
        g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb
        if out is None:
            g.C = p.get("C_addr", FAKE); g.ldc = p.get("ldc", N)
        else:
            # `out` may be an (M, N) window of a wider buffer: its row stride is the leading dimension
            g.C = ptr(out if plan_only else _f(out)); g.ldc = out.stride(0) if M > 1 else max(N, out.stride(0))
        g.bias = addr(p.get("bias")); g.bias2 = addr(p.get("bias2"))
        g.bias_grad = addr(p.get("bias_grad")); g.bias_grad2 = addr(p.get("bias_grad2"))
        g.accumulate = int(p.get("accumulate", False)); g.alpha = p.get("alpha", 1.0)
        outs.append(out)
    return arr, outs


def gemm_bf16_grouped(problems):
    """problems: list of dicts A[M, lda] bf16, B[N, ldb] bf16 (both K-major), K, optional out/bias/bias2/bias_grad/bias_grad2/accumulate/
    alpha/perm_n_H/perm_m_H.  C = alpha * A[:, :K] @ B[:, :K]^T + bias + bias2 (+C); bias_grad[m] += sum_k A[m, k].  `out` may be a
    row-strided (M, N) window of a larger buffer.  One launch per 16 problems."""
    arr, outs = _gemm_bf16_args(problems)
    check(load().mmda_gemm_bf16_grouped(arr, len(problems), stream_ptr()), "mmda_gemm_bf16_grouped")
    return outs


BF16_CLASSES = ("Reg64", "Reg128", "Dma128", "Dma256")


def gemm_bf16_plan(problems, switches=None):
    """What gemm_bf16_grouped(problems) would launch (mmda_gemm_bf16_plan_describe: host code only, works without a GPU).  switches:
    (dma_on, dma_stages, dma_min_rows, dma_tall) in place of the MMDA_GEMM_DMA* environment, None = the defaults (1, 2, 8192, 0).
    Returns (rows, launches): one dict per problem -- cls (a name of BF16_CLASSES, None for an empty problem), mixed, tx, ty, sk, per,
    last, launch -- and the number of GEMM launches.  Problems may be given by shape alone (see _gemm_bf16_args)."""
    arr, _ = _gemm_bf16_args(problems, plan_only=True)
    rows = (_lib.GemmBf16PlanRow * max(1, len(problems)))()
    sw = None if switches is None else (C.c_int * 4)(*[int(x) for x in switches])
    n = load().mmda_gemm_bf16_plan_describe(arr, len(problems), sw, rows, len(problems))
    if n < 0:
        check(n, "mmda_gemm_bf16_plan_describe")
    return [dict(cls=BF16_CLASSES[r.cls] if r.cls >= 0 else None, mixed=bool(r.mixed), tx=r.tx, ty=r.ty, sk=r.sk, per=r.per,
                 last=r.last, launch=r.launch) for r in rows[:len(problems)]], n


def gemm_skinny(problems):
    """Row-skinny exact-f32 GEMMs, up to 8 problems per launch.  Each problem is a dict: A[M,K], B ([N,K] if transB else [K,N]),
    optional A2, second product (A_2nd, B_2nd), out/out2, bias, accumulate, alpha, act, drop_p/seed/site, gate/gate_scale,
    dsig/dsig2.  Returns the list of outputs (out2 tensors are updated in place)."""
    lib = load()
    arr = (_lib.SkinnyArgs * len(problems))()
    outs = []
    for g, p in zip(arr, problems):
        A, B = _f(p["A"]), _f(p["B"])
        tb = bool(p.get("transB", True))
        M, K = A.shape
        N = B.shape[0] if tb else B.shape[1]
        out = p.get("out")
        if out is None:
            out = torch.zeros((M, N), device=A.device, dtype=torch.float32)
        g.M = M; g.N = N; g.K = K; g.transB = int(tb)
        g.A = ptr(A); g.A2 = ptr(p.get("A2")); g.lda = A.stride(0); g.B = ptr(B); g.ldb = B.stride(0)
        if p.get("A_2nd") is not None:
            A2n, B2n = p["A_2nd"], p["B_2nd"]
            g.K2 = A2n.shape[1]; g.A_2nd = ptr(A2n); g.lda_2nd = A2n.stride(0); g.B_2nd = ptr(B2n); g.ldb_2nd = B2n.stride(0)
        g.C = ptr(out); g.ldc = out.stride(0)
        if p.get("out2") is not None:
            g.C2 = ptr(p["out2"]); g.ldc2 = p["out2"].stride(0)
        g.bias = ptr(p.get("bias")); g.accumulate = int(p.get("accumulate", False)); g.alpha = p.get("alpha", 1.0)
        g.act = ACT[p.get("act", "none")]
        g.drop_p = p.get("drop_p", 0.0); g.drop_seed = p.get("seed", 0); g.drop_site = p.get("site", 0)
        if p.get("gate") is not None:
            g.gate = ptr(p["gate"]); g.ldgate = p["gate"].stride(0); g.gate_scale = p.get("gate_scale", 1.0)
        if p.get("dsig") is not None:
            g.dsig = ptr(p["dsig"]); g.lddsig = p["dsig"].stride(0)
        g.dsig2 = ptr(p.get("dsig2"))
        outs.append(out)
    check(lib.mmda_gemm_skinny(arr, len(problems), stream_ptr()), "mmda_gemm_skinny")
    return outs


def transpose_f32(mats):
    """fp32 transposes of several matrices in one launch."""
    lib = load()
    arr = (_lib.TransposeJob * len(mats))()
    outs = []
    for j, x in zip(arr, mats):
        r, c = x.shape
        o = torch.full((c, r), float("nan"), device=x.device)
        j.src = ptr(_f(x)); j.rows = r; j.cols = c; j.ld = x.stride(0); j.dst = ptr(o); j.ldd = r
        outs.append(o)
    check(lib.mmda_transpose_f32(arr, len(mats), stream_ptr()), "mmda_transpose_f32")
    return outs

def colsum(X, out=None, out2=None):
    lib = load()
    M, N = X.shape
    if out is None:
        out = torch.zeros(N, device=X.device)
    check(lib.mmda_colsum(ptr(_f(X)), N, M, N, ptr(out), ptr(out2), stream_ptr()), "mmda_colsum")
    return out


def embed_gather(W, ids):
    lib = load()
    rows, dim = ids.numel(), W.shape[1]
    out = torch.empty(tuple(ids.shape) + (dim,), device=W.device)
    check(lib.mmda_embed_gather(ptr(_f(W)), ptr(ids.contiguous()), rows, dim, ptr(out), stream_ptr()), "embed_gather")
    return out


def embed_scatter_add(dW, ids, dX):
    lib = load()
    check(lib.mmda_embed_scatter_add(ptr(_f(dW)), ptr(ids.contiguous()), ids.numel(), dW.shape[1], ptr(_f(dX)), stream_ptr()),
          "embed_scatter_add")
    return dW


def mx8_quant(x):
    """fp32 (rows, K) -> (element bytes (rows * K,) uint8 in MFMA operand order, scale bytes (rows * K / 32,) uint8): mmda_mx8_quant."""
    lib = load()
    rows, K = x.shape
    q = torch.empty(rows * K, dtype=torch.uint8, device=x.device)
    s = torch.empty(rows * K // 32 + 16, dtype=torch.uint8, device=x.device)
    j = (_lib.Mx8QuantJob * 1)()
    j[0].src = ptr(_f(x)); j[0].ld = K; j[0].rows = rows; j[0].K = K; j[0].q = ptr(q); j[0].s = ptr(s)
    check(lib.mmda_mx8_quant(j, 1, stream_ptr()), "mmda_mx8_quant")
    return q, s


def gemm_mx8(A, B, *, bias=None, act="none", drop_p=0.0, seed=0, site=0):
    """act(A (M, K) @ B (N, K)^T + bias) * dropout with both operands quantised to block-scaled fp8 (OCP MX e4m3): mmda_gemm_mx8."""
    lib = load()
    M, K = A.shape
    N = B.shape[0]
    Aq, As = mx8_quant(A)
    Bq, Bs = mx8_quant(B)
    out = torch.empty(M, N, dtype=torch.float32, device=A.device)
    g = _lib.Mx8Args()
    g.M = M; g.N = N; g.K = K; g.Aq = ptr(Aq); g.As = ptr(As); g.Bq = ptr(Bq); g.Bs = ptr(Bs); g.C = ptr(out); g.ldc = N
    g.bias = ptr(bias); g.act = ACT[act]; g.drop_p = drop_p; g.drop_seed = seed; g.drop_site = site
    check(lib.mmda_gemm_mx8(C.byref(g), stream_ptr()), "mmda_gemm_mx8")
    return out


def embed_segment_sum(dW, ids, rows):
    """dW[id] = list-order sum of rows[p] over ids[p] == id (overwrites those rows; ids < 0 skipped): mmda_embed_segment_sum."""
    lib = load()
    n, D = rows.shape
    need = int(lib.mmda_embed_segment_sum_work_bytes(n, D))
    work = torch.empty(max(need, 256), dtype=torch.uint8, device=dW.device)
    check(lib.mmda_embed_segment_sum(ptr(_f(dW)), ptr(ids), n, D, ptr(_f(rows)), ptr(work), work.numel(), stream_ptr()), "mmda_embed_segment_sum")
    return dW


def _fill_actp(ap, slope=None, dslope=None, rrelu=None):
    """mmda_act_params: slope / dslope are one-element device tensors (PReLU), rrelu = (lo, hi, rand, seed, site) (RReLU)."""
    ap.slope = ptr(slope); ap.dslope = ptr(dslope)
    if rrelu is not None:
        ap.lo, ap.hi, ap.rand, ap.seed, ap.site = rrelu[0], rrelu[1], int(rrelu[2]), rrelu[3], rrelu[4]
    return ap


def layernorm_fwd(x, gamma, beta, *, res=None, act="none", drop_p=0.0, seed=0, site=0, permute=None, eps=1e-5, slope=None, rrelu=None):
    lib = load()
    n = x.shape[-1]
    rows = x.numel() // n
    y = torch.empty_like(x)
    mean = torch.empty(rows, device=x.device); rstd = torch.empty(rows, device=x.device)
    a = _lib.LnArgs()
    a.rows = rows; a.n = n; a.x = ptr(_f(x)); a.res = ptr(res); a.gamma = ptr(gamma); a.beta = ptr(beta)
    a.y = ptr(y); a.mean = ptr(mean); a.rstd = ptr(rstd); a.act = ACT[act]
    a.drop_p = drop_p; a.drop_seed = seed; a.drop_site = site
    a.permute_S, a.permute_B = permute if permute else (0, 0)
    a.eps = eps
    _fill_actp(a.actp, slope, None, rrelu)
    check(lib.mmda_layernorm_fwd(C.byref(a), stream_ptr()), "layernorm_fwd")
    if permute:
        y = y.view(permute[1], permute[0], n)
    return y, mean, rstd


def layernorm_bwd(dy, x, gamma, mean, rstd, *, res=None, act="none", drop_p=0.0, seed=0, site=0, permute=None,
                  want_dres=False, slope=None, dslope=None, rrelu=None):
    """dslope (PReLU, one element) is accumulated into."""
    lib = load()
    n = x.shape[-1]
    rows = x.numel() // n
    dx = torch.empty_like(x)
    dres = torch.empty_like(x) if want_dres else None
    dg = torch.zeros(n, device=x.device); db = torch.zeros(n, device=x.device)
    a = _lib.LnBwdArgs()
    a.rows = rows; a.n = n; a.dy = ptr(_f(dy)); a.x = ptr(_f(x)); a.res = ptr(res); a.gamma = ptr(gamma)
    a.mean = ptr(mean); a.rstd = ptr(rstd); a.d_x = ptr(dx); a.accumulate_dx = 0; a.d_res = ptr(dres)
    a.dgamma = ptr(dg); a.dbeta = ptr(db); a.act = ACT[act]
    a.drop_p = drop_p; a.drop_seed = seed; a.drop_site = site
    a.permute_S, a.permute_B = permute if permute else (0, 0)
    _fill_actp(a.actp, slope, dslope, rrelu)
    check(lib.mmda_layernorm_bwd(C.byref(a), stream_ptr()), "layernorm_bwd")
    return dx, dres, dg, db


def layernorm_multi(xs, gammas, betas, dys, acts=None, slope=None, dslope=None, rrelu=None):
    """Several LayerNorms through the multi-problem launches: forward, input gradients (no parameter gradients) and the
    separate parameter-gradient pass.  Returns per problem (y, dx, dgamma, dbeta).  acts: one activation name per problem (default
    none); slope / dslope / rrelu are shared by all problems, as in the model (dslope is accumulated into by the input-gradient pass)."""
    lib = load()
    k = len(xs)
    fa = (_lib.LnArgs * k)(); ba = (_lib.LnBwdArgs * k)()
    keep = []
    for a, b, x, g, be, dy, act in zip(fa, ba, xs, gammas, betas, dys, acts or ["none"] * k):
        rows, n = x.shape
        y = torch.empty_like(x); mean = torch.empty(rows, device=x.device); rstd = torch.empty(rows, device=x.device)
        dx = torch.empty_like(x); dg = torch.zeros(n, device=x.device); db = torch.zeros(n, device=x.device)
        a.rows = rows; a.n = n; a.x = ptr(_f(x)); a.gamma = ptr(g); a.beta = ptr(be); a.y = ptr(y); a.mean = ptr(mean); a.rstd = ptr(rstd)
        a.eps = 1e-5; a.act = ACT[act]
        _fill_actp(a.actp, slope, None, rrelu)
        b.rows = rows; b.n = n; b.dy = ptr(_f(dy)); b.x = ptr(x); b.gamma = ptr(g); b.mean = ptr(mean); b.rstd = ptr(rstd); b.d_x = ptr(dx)
        b.act = ACT[act]
        _fill_actp(b.actp, slope, dslope, rrelu)
        keep.append((y, dx, dg, db, mean, rstd))
    check(lib.mmda_layernorm_fwd_multi(fa, k, stream_ptr()), "layernorm_fwd_multi")
    check(lib.mmda_layernorm_bwd_multi(ba, k, stream_ptr()), "layernorm_bwd_multi")      # dgamma/dbeta NULL: dx only
    for b, (y, dx, dg, db, mean, rstd) in zip(ba, keep):
        b.dgamma = ptr(dg); b.dbeta = ptr(db); b.d_x = None
    check(lib.mmda_layernorm_param_grads(ba, k, stream_ptr()), "layernorm_param_grads")
    return [(y, dx, dg, db) for (y, dx, dg, db, _, _) in keep]


def act_dropout_fwd(z, act, p=0.0, seed=0, site=0, slope=None, rrelu=None):
    """h = dropout(act(z)) element-wise, any of the ten activations: mmda_act_dropout_fwd_p."""
    lib = load()
    h = torch.empty_like(z)
    ap = _fill_actp(_lib.ActParams(), slope, None, rrelu)
    check(lib.mmda_act_dropout_fwd_p(ptr(_f(z)), ptr(h), z.numel(), ACT[act], C.byref(ap), p, seed, site, stream_ptr()), "act_dropout_fwd")
    return h


def act_dropout_bwd(dh, z, act, p=0.0, seed=0, site=0, slope=None, rrelu=None, dslope=None):
    """dz = dh * dropmask * act'(z); dslope (PReLU, one element) is accumulated into: mmda_act_dropout_bwd_p."""
    lib = load()
    dz = torch.empty_like(z)
    ap = _fill_actp(_lib.ActParams(), slope, dslope, rrelu)
    check(lib.mmda_act_dropout_bwd_p(ptr(_f(dh)), ptr(_f(z)), ptr(dz), z.numel(), ACT[act], C.byref(ap), p, seed, site, stream_ptr()),
          "act_dropout_bwd")
    return dz


def lstm_pack(whh, mode):
    """Returns (packed_fwd, packed_bwd) byte tensors for one direction's W_hh (4H,H)."""
    lib = load()
    H = whh.shape[1]
    md = MODE[mode]
    pf = torch.empty(lib.mmda_lstm_packed_bytes(md, H, 0), dtype=torch.uint8, device=whh.device)
    pb = torch.empty(lib.mmda_lstm_packed_bytes(md, H, 1), dtype=torch.uint8, device=whh.device)
    check(lib.mmda_lstm_pack_whh(md, H, ptr(_f(whh)), ptr(pf), ptr(pb), stream_ptr()), "lstm_pack")
    return pf, pb


def lstm_pack_cluster(whh):
    """Cluster-backward packing (bf16) of one direction's W_hh."""
    lib = load()
    H = whh.shape[1]
    pc = torch.empty(lib.mmda_lstm_packed_bytes(BF16, H, 2), dtype=torch.uint8, device=whh.device)
    check(lib.mmda_lstm_pack_whh_cluster(H, ptr(_f(whh)), ptr(pc), stream_ptr()), "lstm_pack_cluster")
    return pc


def _desc(H, gates, cstash, hseq, wp0, wp1, utt, layer, d_hseq=None, xchg=None, epoch_base=0, wc0=None, wc1=None):
    d = _lib.LstmDesc()
    d.H = H; d.gates = ptr(gates); d.cstash = ptr(cstash); d.hseq = ptr(hseq)
    d.wpack[0] = ptr(wp0); d.wpack[1] = ptr(wp1)
    d.wpack_c[0] = ptr(wc0); d.wpack_c[1] = ptr(wc1)
    d.utt = ptr(utt); d.layer = layer; d.d_hseq = ptr(d_hseq)
    d.xchg = ptr(xchg); d.epoch_base = epoch_base
    return d


def lstm_xchg(H, B, device):
    """Zeroed cluster-exchange buffer (None when the shape has no resident-weights plan)."""
    n = load().mmda_lstm_xchg_bytes(H, B)
    return torch.zeros(n, dtype=torch.uint8, device=device) if n > 0 else None


LSTM_FORMS = ("barrier", "wave", "quad")
LSTM_DHSEQ = ("run-time", "absent", "present")


def lstm_kernel_names():
    """The C++ names of the resident recurrences' kernel instances, in the order of the MMDA_LSTM_K_* enum"""
    lib, out = load(), []
    while (s := lib.mmda_lstm_kernel_name(len(out))) is not None:
        out.append(s.decode())
    return out


def lstm_plan(descs, B, T, backward=False, no_quad=False, quad_cap=0):
    """What mmda_lstm_fwd / mmda_lstm_bwd would run for these descriptors on the resident-weights kernels (mmda_lstm_plan_describe:
    host code only; without a GPU give quad_cap > 0).  descs: an array of _lib.LstmDesc as the real call takes it, or a list of dicts
    by shape alone -- H and optionally cell ('lstm' / 'gru'), gate_minor, forward_only, d_hseq, dg_bf16, dg_bf16_only, xchg, wpack_c (the
    last five as booleans: only whether a pointer is NULL matters; xchg and wpack_c default to present).  no_quad stands for
    MMDA_LSTM_NO_QUAD; quad_cap > 0 replaces the occupancy query behind the quad form's limit, 0 asks the runtime as a launch does.
    Returns a dict: ok, form (a name of LSTM_FORMS), wpb, groups, groups_per_launch, launches, wg_per_group, wg_per_desc, gru,
    gate_minor, no_stash, dhseq (a name of LSTM_DHSEQ), pair, kernel (the instance's C++ name); ok = False: the streaming
    kernels run and the other entries are None."""
    if not isinstance(descs, C.Array):
        arr = (_lib.LstmDesc * max(1, len(descs)))()
        for d, p in zip(arr, descs):
            fake = lambda on: 4096 if on else None           # never followed
            d.H = p["H"]; d.cell = _lib.CELL[p.get("cell", "lstm")]; d.gate_minor = int(p.get("gate_minor", False))
            d.forward_only = int(p.get("forward_only", False)); d.dg_bf16_only = int(p.get("dg_bf16_only", False))
            d.xchg = fake(p.get("xchg", True)); d.d_hseq = fake(p.get("d_hseq", False)); d.dg_bf16 = fake(p.get("dg_bf16", False))
            d.wpack_c[0] = d.wpack_c[1] = fake(p.get("wpack_c", True))
        n = len(descs)
    else:
        arr, n = descs, len(descs)
    plan = _lib.LstmPlan()
    sw = (C.c_int * 2)(int(no_quad), int(quad_cap))
    check(load().mmda_lstm_plan_describe(n, arr, B, T, int(backward), sw, C.byref(plan)), "mmda_lstm_plan_describe")
    keys = ("form", "wpb", "groups", "groups_per_launch", "launches", "wg_per_group", "wg_per_desc", "gru", "gate_minor", "no_stash",
            "dhseq", "pair", "kernel")
    if not plan.ok:
        return dict({k: None for k in keys}, ok=False)
    return dict(ok=True, form=LSTM_FORMS[plan.form], wpb=plan.wpb, groups=plan.groups, groups_per_launch=plan.groups_per_launch,
                launches=plan.launches, wg_per_group=plan.wg_per_group, wg_per_desc=list(plan.wg_per_desc)[:n], gru=bool(plan.gru),
                gate_minor=bool(plan.gate_minor), no_stash=bool(plan.no_stash), dhseq=LSTM_DHSEQ[plan.dhseq],
                pair=bool(plan.pair), kernel=load().mmda_lstm_kernel_name(plan.kernel).decode())


def step_plan(handle, B, T, *, fused=False, labels=False, opt_step=False, enc_cached=False, switches=None):
    """The plan a forward pass over (B, T) batches gets on a model handle as it is set now (mmda_misa_plan_describe: host code only,
    works without a GPU, a workspace or bound buffers).  fused / labels / opt_step / enc_cached: what the pass is asked to be -- part of
    train_step, with labels, with an optimizer step that may run the background table pass behind it, starting behind the encoders.
    switches: None for the defaults (the process's environment is NOT read), or a dict from names of _lib.STEP_SWITCHES to values, the
    rest at their defaults.  Returns a dict with one entry per field of _lib.STEP_PLAN_FIELDS: bools, but for the ints gm,
    embed_update, embed_bg_wgs and embed_bg_lds."""
    req = _lib.MisaStepRequest(int(fused), int(labels), int(opt_step), int(enc_cached))
    sw = None
    if switches is not None:
        assert set(switches) <= set(_lib.STEP_SWITCHES), sorted(set(switches) - set(_lib.STEP_SWITCHES))
        sw = (C.c_int * len(_lib.STEP_SWITCHES))(*dict(_lib.STEP_SWITCHES, **switches).values())
    plan = _lib.MisaStepPlan()
    check(load().mmda_misa_plan_describe(handle, int(B), int(T), C.byref(req), sw, len(_lib.STEP_SWITCHES), C.byref(plan)),
          "mmda_misa_plan_describe")
    ints = ("gm", "embed_update", "embed_bg_wgs", "embed_bg_lds")
    return {k: getattr(plan, k) if k in ints else bool(getattr(plan, k)) for k in _lib.STEP_PLAN_FIELDS}


LOSS_DIFF_FORMS = ("generic", "fast4", "fast8", "fast16", "fast32")
LOSS_DIFF_PRODUCTS = ("skinny", "batched")
LOSS_DIFF_SUMS = (None, "finish", "own_launch")
LOSS_CMD_FORMS = ("fast4", "fast8", "stream", "serial", "reject")


def loss_forms(B, D, have_loss=True, have_dx=True, cmd_nt=3, n_recon=0):
    """Which kernel form the loss entry points pick for (B, D) tensors (mmda_loss_forms_describe: host code only, no GPU; the
    launchers read the same decision).  have_loss / have_dx: whether the call passes `loss` / `dx`; cmd_nt: tensors of the CMD call;
    n_recon: elements of the recon call (0: 3 * B * D).  Returns a dict: diff (a name of LOSS_DIFF_FORMS), diff_products
    ('skinny' / 'batched'), diff_loss_sum ('finish' / 'own_launch', None without `loss`), diff_combine_blocks, cmd (a name of
    LOSS_CMD_FORMS), cmd_grid, recon_blocks (mmda_loss_recon), misc_recon_blocks (mmda_loss_misc)."""
    f = _lib.LossForms()
    check(load().mmda_loss_forms_describe(int(B), int(D), int(bool(have_loss)), int(bool(have_dx)), int(cmd_nt), int(n_recon),
                                          C.byref(f)), "mmda_loss_forms_describe")
    return dict(diff=LOSS_DIFF_FORMS[f.diff_form], diff_products=LOSS_DIFF_PRODUCTS[f.diff_products],
                diff_loss_sum=LOSS_DIFF_SUMS[f.diff_loss_sum], diff_combine_blocks=f.diff_combine_blocks,
                cmd=LOSS_CMD_FORMS[f.cmd_form], cmd_grid=f.cmd_grid, recon_blocks=f.recon_blocks,
                misc_recon_blocks=f.misc_recon_blocks)


def _to_gate_minor(x, H):
    """(..., 4H) [gate][unit] -> [unit][gate] (the resident-weights kernels' 16-byte layout)"""
    return x.reshape(*x.shape[:-1], 4, H).transpose(-1, -2).reshape(*x.shape[:-1], 4 * H).contiguous()


def _from_gate_minor(x, H):
    return x.reshape(*x.shape[:-1], H, 4).transpose(-1, -2).reshape(*x.shape[:-1], 4 * H).contiguous()


def gru_pad(rnn_params, H, D, device):
    """torch nn.GRU(bidirectional) parameters -> the four-slot layout (mmda_gru_pad_params).  rnn_params: dict with
    weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0 and their _reverse twins.  Returns (job, padded dict); the job can be
    handed to gru_unpad_grads with gradient tensors of the same shapes."""
    lib = load()
    t = {k: _f(v.detach().to(device)) for k, v in rnn_params.items()}
    pad = dict(w_ih=torch.full((8 * H, D), float("nan"), device=device), w_hh_f=torch.full((4 * H, H), float("nan"), device=device),
               w_hh_r=torch.full((4 * H, H), float("nan"), device=device), b_ih=torch.full((8 * H,), float("nan"), device=device),
               b_hh=torch.full((8 * H,), float("nan"), device=device))
    check(lib.mmda_gru_pad_params((_lib.GruPadJob * 1)(_gru_job(t, pad, H, D)), 1, stream_ptr()), "gru_pad_params")
    return pad, t


def _gru_job(t, pad, H, D):
    j = _lib.GruPadJob()
    j.H, j.D = H, D
    for d, sfx in enumerate(("", "_reverse")):
        j.w_ih[d] = ptr(t["weight_ih_l0" + sfx]); j.w_hh[d] = ptr(t["weight_hh_l0" + sfx])
        j.b_ih[d] = ptr(t["bias_ih_l0" + sfx]); j.b_hh[d] = ptr(t["bias_hh_l0" + sfx])
    j.pw_ih = ptr(pad["w_ih"]); j.pw_hh[0] = ptr(pad["w_hh_f"]); j.pw_hh[1] = ptr(pad["w_hh_r"])
    j.pb_ih = ptr(pad["b_ih"]); j.pb_hh = ptr(pad["b_hh"]) if pad.get("b_hh") is not None else None
    return j


def gru_unpad_grads(grads, pad_grads, H, D):
    """grads (torch-layout dict, accumulated into) += pad_grads (four-slot: w_ih, w_hh_f, w_hh_r, b_ih = gate-gradient column
    sums); pad_grads are zeroed."""
    lib = load()
    check(lib.mmda_gru_unpad_grads((_lib.GruPadJob * 1)(_gru_job(grads, dict(pad_grads, b_hh=None), H, D)), 1, stream_ptr()),
          "gru_unpad_grads")


def lstm_bidir_fwd(pre, whh_f, whh_r, lengths, *, mode="fp32", layer=0, utt=None, resident=False, gate_minor=False, cell="lstm"):
    """pre: (T,B,2,4H) = x W_ih^T + b_ih + b_hh per direction.  Returns dict(hseq, gates, cstash, utt, packs).
    gate_minor (resident only): the kernels see `gates` as [dir][unit][gate]; inputs/outputs here stay in torch's order.
    cell="gru": pre / whh_* are in the four-slot layout (gru_pad)."""
    lib = load()
    T, B, _, G4 = pre.shape
    H = G4 // 4
    gates = _to_gate_minor(pre, H) if gate_minor else pre.clone().contiguous()
    # torch layout (T,B,2,H); the gate-minor kernels keep it batch-minor-by-4, (T, ceil(B/4), 2, H, 4): rows rounded up
    cst = torch.zeros(T, (B + 3) // 4, 2, H, 4, device=pre.device) if gate_minor else torch.zeros(T, B, 2, H, device=pre.device)
    hseq = torch.full((T, B, 2 * H), float("nan"), device=pre.device)
    if utt is None:
        utt = torch.zeros(B, 4 * H, device=pre.device)
    pf0, pb0 = lstm_pack(whh_f, mode)
    pf1, pb1 = lstm_pack(whh_r, mode)
    len_dev = lengths.to(device=pre.device, dtype=torch.int32)
    xchg = lstm_xchg(H, B, pre.device) if resident else None
    pcs = (lstm_pack_cluster(whh_f), lstm_pack_cluster(whh_r)) if (resident and MODE[mode] == BF16) else (None, None)
    d = (_lib.LstmDesc * 1)(_desc(H, gates, cst, hseq, pf0, pf1, utt, layer, None, xchg, 0))
    d[0].gate_minor = int(gate_minor)
    d[0].cell = _lib.CELL[cell]
    check(lib.mmda_lstm_fwd(MODE[mode], 1, d, B, T, ptr(len_dev), stream_ptr()), "lstm_fwd")
    return dict(hseq=hseq, gates=gates, cstash=cst, utt=utt, packs=(pf0, pb0, pf1, pb1), len_dev=len_dev, xchg=xchg, T=T, pcs=pcs,
                gate_minor=bool(gate_minor), H=H, cell=cell)


def lstm_bidir_bwd(fw, d_utt, d_hseq, *, mode="fp32", layer=0, dg_bf16_only=False):
    """Consumes the dict returned by lstm_bidir_fwd; returns dG (T,B,2,4H) (overwrites fw['gates'])."""
    lib = load()
    gates = fw["gates"]
    T, B, _, G4 = gates.shape
    H = G4 // 4
    pf0, pb0, pf1, pb1 = fw["packs"]
    pc0, pc1 = fw.get("pcs", (None, None))
    d = (_lib.LstmDesc * 1)(_desc(H, gates, fw["cstash"], fw["hseq"], pb0, pb1, d_utt, layer, d_hseq, fw.get("xchg"), T + 2, pc0, pc1))
    d[0].gate_minor = int(fw.get("gate_minor", False))
    d[0].cell = _lib.CELL[fw.get("cell", "lstm")]
    if MODE[mode] == BF16 and lib.mmda_lstm_bwd_emits_dg_bf16(BF16, 1, d, B, T):
        # the resident gate-minor kernel also emits dG rounded to bf16 (kernel column order); NaN-filled to expose gaps
        fw["dg_bf16"] = torch.full((T * B, 2 * G4), float("nan"), device=gates.device, dtype=torch.bfloat16)
        d[0].dg_bf16 = ptr(fw["dg_bf16"])
        d[0].dg_bf16_only = int(dg_bf16_only)
    check(lib.mmda_lstm_bwd(MODE[mode], 1, d, B, T, ptr(fw["len_dev"]), stream_ptr()), "lstm_bwd")
    return _from_gate_minor(gates, H) if fw.get("gate_minor") else gates


def lstm_aborted(fw):
    """True if a cluster exchange timed out (sticky abort word at the start of the exchange buffer)."""
    x = fw.get("xchg")
    return False if x is None else bool(x[:4].view(torch.int32).item() != 0)


def attn_fwd(qkv, S, B, E, nhead, drop_p=0.0, seed=0, site=0):
    lib = load()
    ctx = torch.empty(S * B, E, device=qkv.device)
    probs = torch.empty(B, nhead, S, S, device=qkv.device)
    check(lib.mmda_attn_fwd(ptr(_f(qkv)), S, B, E, nhead, ptr(ctx), ptr(probs), drop_p, seed, site, stream_ptr()), "attn_fwd")
    return ctx, probs


def attn_bwd(qkv, probs, dctx, S, B, E, nhead, drop_p=0.0, seed=0, site=0):
    lib = load()
    dqkv = torch.empty_like(qkv)
    check(lib.mmda_attn_bwd(ptr(_f(qkv)), ptr(_f(probs)), ptr(_f(dctx)), S, B, E, nhead, ptr(dqkv), drop_p, seed, site,
                            stream_ptr()), "attn_bwd")
    return dqkv


def clamp_adam(p, g, m, v, lr, step, clip=float("inf"), grad_scale=1.0, betas=(0.9, 0.999), eps=1e-8):
    lib = load()
    check(lib.mmda_clamp_adam(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), lr, betas[0], betas[1], eps, clip, grad_scale, step,
                              stream_ptr()), "clamp_adam")


def grad_accumulate(acc, g, first=False):
    """acc = g (first) or acc += g, elementwise fp32, in place: one micro-batch's gradients into the accumulator of an accumulated step."""
    lib = load()
    assert acc.numel() == g.numel() and acc.dtype == g.dtype == torch.float32 and acc.is_contiguous() and g.is_contiguous()
    check(lib.mmda_grad_accumulate(ptr(acc), ptr(g), acc.numel(), int(bool(first)), stream_ptr()), "grad_accumulate")


def clamp_adam_sum(p, acc, g, m, v, lr, step, clip=float("inf"), grad_scale=1.0, betas=(0.9, 0.999), eps=1e-8):
    """clamp_adam with the gradient acc + g (neither is written); acc = None: clamp_adam itself."""
    lib = load()
    assert acc is None or (acc.numel() == p.numel() and acc.is_contiguous())
    check(lib.mmda_clamp_adam_sum(ptr(p), ptr(acc), ptr(g), ptr(m), ptr(v), p.numel(), lr, betas[0], betas[1], eps, clip, grad_scale, step,
                                  stream_ptr()), "clamp_adam_sum")


def runs_table(ranges, bucket_floats, device="cuda"):
    """Frozen parameters: the device table of trainable runs for the run-table launches below, from (begin, length) ranges of a flat
    bucket -- ascending and disjoint; empty ones are dropped, touching ones merged.  Returns (table, runs, items); build it once per
    change of the set."""
    lib = load()
    k = len(ranges)
    begin = (C.c_int64 * max(k, 1))(*[int(b) for b, _ in ranges])
    length = (C.c_int64 * max(k, 1))(*[int(l) for _, l in ranges])
    out = (_lib.Run * max(k, 1))()
    n = C.c_int()
    items = int(lib.mmda_runs_build(begin, length, k, int(bucket_floats), out, C.byref(n)))
    if items < 0:
        raise _lib.MMDAError("mmda_runs_build: the ranges must be ascending, disjoint and inside the bucket")
    rows = [[out[i].begin, out[i].len, out[i].first] for i in range(n.value)] or [[0, 0, 0]]
    return torch.tensor(rows, dtype=torch.int64).to(device), int(n.value), items


def clamp_adam_runs(p, g, m, v, runs, lr, step, clip=float("inf"), grad_scale=1.0, betas=(0.9, 0.999), eps=1e-8):
    """clamp_adam over the trainable runs (runs_table) of the flat buffers only: nothing between the runs is read or written."""
    lib = load()
    table, n, items = runs
    check(lib.mmda_clamp_adam_runs(ptr(p), ptr(g), ptr(m), ptr(v), ptr(table), n, items, lr, betas[0], betas[1], eps, clip, grad_scale, step,
                                   stream_ptr()), "clamp_adam_runs")


def clamp_adam_sum_runs(p, acc, g, m, v, runs, lr, step, clip=float("inf"), grad_scale=1.0, betas=(0.9, 0.999), eps=1e-8):
    """clamp_adam_sum over the trainable runs only."""
    lib = load()
    table, n, items = runs
    assert acc is None or (acc.numel() == p.numel() and acc.is_contiguous())
    check(lib.mmda_clamp_adam_sum_runs(ptr(p), ptr(acc), ptr(g), ptr(m), ptr(v), ptr(table), n, items, lr, betas[0], betas[1], eps, clip,
                                       grad_scale, step, stream_ptr()), "clamp_adam_sum_runs")


def clamp_rmsprop(p, g, sq, lr, alpha=0.99, eps=1e-8, clip=float("inf"), grad_scale=1.0):
    lib = load()
    check(lib.mmda_clamp_rmsprop(ptr(p), ptr(g), ptr(sq), p.numel(), lr, alpha, eps, clip, grad_scale, stream_ptr()), "clamp_rmsprop")


def clamp_rmsprop_runs(p, g, sq, runs, lr, alpha=0.99, eps=1e-8, clip=float("inf"), grad_scale=1.0):
    """clamp_rmsprop over the trainable runs only."""
    lib = load()
    table, n, items = runs
    check(lib.mmda_clamp_rmsprop_runs(ptr(p), ptr(g), ptr(sq), ptr(table), n, items, lr, alpha, eps, clip, grad_scale, stream_ptr()),
          "clamp_rmsprop_runs")


def _adam_opts(betas, eps, weight_decay, decoupled, scale_dev):
    assert scale_dev is None or (scale_dev.dtype == torch.float32 and scale_dev.is_cuda and scale_dev.numel() >= 1)
    return _lib.AdamOpts(beta1=betas[0], beta2=betas[1], eps=eps, weight_decay=weight_decay, decoupled=int(bool(decoupled)),
                         scale_dev=ptr(scale_dev))


def clamp_adam_opts(p, g, m, v, lr, step, clip=float("inf"), grad_scale=1.0, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                    decoupled=False, scale_dev=None, acc=None, runs=None):
    """clamp_adam / _sum / _runs / _sum_runs with the settings of mmda_adam_opts: L2 (torch.optim.Adam) or decoupled (torch.optim.AdamW)
    weight decay, and ``scale_dev``, a device float that multiplies ``grad_scale`` inside the launch.  acc: the gradient is acc + g;
    runs (runs_table): the trainable runs only."""
    lib = load()
    table, n, items = runs if runs is not None else (None, 0, 0)
    assert acc is None or (acc.numel() == p.numel() and acc.is_contiguous())
    opts = _adam_opts(betas, eps, weight_decay, decoupled, scale_dev)
    check(lib.mmda_clamp_adam_opts(ptr(p), ptr(acc), ptr(g), ptr(m), ptr(v), p.numel(), ptr(table), n, items, lr, clip, grad_scale, step,
                                   C.byref(opts), stream_ptr()), "clamp_adam_opts")


def clamp_adam_rows_opts(p, g, m, v, mask, want, lr, step, clip=float("inf"), grad_scale=1.0, betas=(0.9, 0.999), eps=1e-8,
                         weight_decay=0.0, decoupled=False, scale_dev=None):
    """clamp_adam_rows with the settings of mmda_adam_opts."""
    lib = load()
    rows, dim = p.shape
    opts = _adam_opts(betas, eps, weight_decay, decoupled, scale_dev)
    check(lib.mmda_clamp_adam_rows_opts(ptr(p), ptr(g), ptr(m), ptr(v), rows, dim, ptr(mask), int(want), lr, clip, grad_scale, step,
                                        C.byref(opts), stream_ptr()), "clamp_adam_rows_opts")


def grad_norm(g, max_norm, grad_scale=1.0, acc=None, runs=None):
    """The global L2 norm of the flat gradient g (acc + g; over the runs of a runs_table only) and clip_grad_norm_'s coefficient:
    a (2,) device tensor [grad_scale * norm, min(1, max_norm / (that + 1e-6))].  Deterministic; nothing is read back."""
    lib = load()
    table, n, items = runs if runs is not None else (None, 0, 0)
    assert g.dtype == torch.float32 and g.is_contiguous() and (acc is None or (acc.numel() == g.numel() and acc.is_contiguous()))
    cap = int(lib.mmda_grad_norm_partials(items if runs is not None else g.numel()))
    parts = torch.empty(max(cap, 1), dtype=torch.float64, device=g.device)
    out = torch.empty(2, dtype=torch.float32, device=g.device)
    check(lib.mmda_grad_norm(ptr(g), ptr(acc), g.numel(), ptr(table), n, items, max_norm, grad_scale, ptr(parts), cap, ptr(out),
                             stream_ptr()), "grad_norm")
    return out


def grad_scale_(g, scale_dev, runs=None):
    """g *= scale_dev[0] in place (over the runs of a runs_table only); scale_dev: a device float, e.g. grad_norm(...)[1:]."""
    lib = load()
    table, n, items = runs if runs is not None else (None, 0, 0)
    assert g.dtype == torch.float32 and g.is_contiguous() and scale_dev.dtype == torch.float32 and scale_dev.is_cuda
    check(lib.mmda_grad_scale(ptr(g), g.numel(), ptr(table), n, items, ptr(scale_dev), stream_ptr()), "grad_scale")


def embed_rows_append(ids_out, rows_out, offset, ids, rows, lengths=None):
    """A micro-batch's (T, B) ids and (T * B, D) gradient rows appended at position `offset` of the list (ids_out (cap,) int64, rows_out
    (cap, D) fp32); positions past a sample's length (lengths: (B,) int32 on the device) get id -1.  Returns the list's new length."""
    lib = load()
    n = ids.numel()
    cap, D = rows_out.shape
    assert ids.dtype == ids_out.dtype == torch.int64 and ids.is_contiguous() and ids_out.is_contiguous() and ids_out.numel() == cap
    assert rows.shape == (n, D) and rows.is_contiguous() and rows_out.is_contiguous()
    B = 0
    if lengths is not None:
        assert lengths.dtype == torch.int32 and lengths.is_cuda and lengths.is_contiguous() and n % lengths.numel() == 0
        B = lengths.numel()
    check(lib.mmda_embed_rows_append(ptr(ids_out), ptr(rows_out), int(offset), cap, ptr(ids), ptr(rows), n, D, ptr(lengths), B,
                                     stream_ptr()), "embed_rows_append")
    return int(offset) + n


def mark_rows(ids, rows):
    """uint8 mask of `rows` bytes: 1 where the row id occurs in `ids` (int64, device)."""
    lib = load()
    mask = torch.empty(rows, dtype=torch.uint8, device=ids.device)
    check(lib.mmda_mark_rows(ptr(mask), rows, ptr(ids), ids.numel(), stream_ptr()), "mark_rows")
    return mask


def clamp_adam_rows(p, g, m, v, mask, want, lr, step, clip=float("inf"), grad_scale=1.0, betas=(0.9, 0.999), eps=1e-8):
    """clip + Adam over the rows of the (rows, dim) table p whose mask byte equals `want` (in place)."""
    lib = load()
    rows, dim = p.shape
    check(lib.mmda_clamp_adam_rows(ptr(p), ptr(g), ptr(m), ptr(v), rows, dim, ptr(mask), int(want), lr, betas[0], betas[1], eps, clip,
                                   grad_scale, step, stream_ptr()), "clamp_adam_rows")


def embed_rows_sparse_adam(p, m, v, ids, rows, lr, step, lengths=None, clip=float("inf"), grad_scale=1.0, betas=(0.9, 0.999), eps=1e-8):
    """torch.optim.SparseAdam on the rows of the (V, D) table p (moments m, v; in place) that the id list touches: per distinct id at a
    non-padding position, g = clamp(grad_scale * position-order sum of rows[pos], +-clip), then the update.  ids: (n,) or (T, B) int64;
    rows: (n, D) fp32; lengths: (B,) int32 on the device or None (position t * B + b is padding when t >= lengths[b])."""
    lib = load()
    V, D = p.shape
    n = ids.numel()
    assert ids.dtype == torch.int64 and ids.is_cuda and ids.is_contiguous() and rows.shape == (n, D)
    assert p.is_contiguous() and m.is_contiguous() and v.is_contiguous()
    B = 0
    if lengths is not None:
        assert lengths.dtype == torch.int32 and lengths.is_cuda and lengths.is_contiguous() and n % lengths.numel() == 0
        B = lengths.numel()
    check(lib.mmda_embed_rows_sparse_adam(ptr(_f(p)), ptr(_f(m)), ptr(_f(v)), ptr(ids), n, D, ptr(_f(rows)), ptr(lengths), B, V, lr,
                                          betas[0], betas[1], eps, clip, grad_scale, step, stream_ptr()), "embed_rows_sparse_adam")


class DeferredState:
    """Device state of the deferred dense update of one (table_rows, D) table -- row_step (int32 per row) and the ring of step scalars
    -- and, on the host, the count of updates applied (`seq`) and the count at the last full flush.  The counting is done here, so a
    caller cannot hand the kernels an update number that is not the last one + 1."""

    def __init__(self, table_rows, window, device="cuda"):
        lib = load()
        if window < 1:
            raise ValueError("window must be at least 1")
        self.window = int(window)
        self.row_step = torch.empty(table_rows, dtype=torch.int32, device=device)
        self.ring = torch.zeros(int(lib.mmda_embed_deferred_scalar_floats(self.window)), dtype=torch.float32, device=device)
        self.reset()

    def reset(self):
        """Every row current, no update counted (a new or a loaded table)."""
        check(load().mmda_embed_deferred_reset(ptr(self.row_step), self.row_step.numel(), stream_ptr()), "embed_deferred_reset")
        self.seq = 0
        self.flushed = 0


def embed_deferred_state(table_rows, window, device="cuda"):
    return DeferredState(table_rows, window, device)


def embed_rows_dense_adam(p, m, v, state, ids, rows, lr, step, lengths=None, clip=float("inf"), grad_scale=1.0, betas=(0.9, 0.999),
                          eps=1e-8):
    """The next update of dense Adam (clamp_adam's arithmetic, bias corrections of step number `step`) on the rows of the (V, D) table p
    (moments m, v; in place) that the id list touches, with g = the position-order sum of rows[pos]; every other row takes the update
    when it is next caught up or flushed (`state`: a DeferredState, which counts the updates).  Arguments as embed_rows_sparse_adam."""
    lib = load()
    V, D = p.shape
    n = ids.numel()
    assert state.row_step.numel() == V
    assert ids.dtype == torch.int64 and ids.is_cuda and ids.is_contiguous() and rows.shape == (n, D)
    assert p.is_contiguous() and m.is_contiguous() and v.is_contiguous()
    B = 0
    if lengths is not None:
        assert lengths.dtype == torch.int32 and lengths.is_cuda and lengths.is_contiguous() and n % lengths.numel() == 0
        B = lengths.numel()
    seq = state.seq + 1
    check(lib.mmda_embed_rows_dense_adam(ptr(_f(p)), ptr(_f(m)), ptr(_f(v)), ptr(state.row_step), ptr(state.ring), state.window, ptr(ids), n,
                                         D, ptr(_f(rows)), ptr(lengths), B, V, lr, betas[0], betas[1], eps, clip, grad_scale, seq, step,
                                         stream_ptr()), "embed_rows_dense_adam")
    if seq % state.window == 0:
        state.flushed = seq - 1                              # (that update flushed first)
    state.seq = seq


def embed_rows_catch_up(p, m, v, state, ids, lengths=None, betas=(0.9, 0.999), eps=1e-8):
    """The rows of p (and m, v) at the non-padding positions of the id list take the updates they missed: run it before reading those
    rows."""
    lib = load()
    V, D = p.shape
    assert state.row_step.numel() == V
    assert ids.dtype == torch.int64 and ids.is_cuda and ids.is_contiguous()
    B = 0
    if lengths is not None:
        assert lengths.dtype == torch.int32 and lengths.is_cuda and lengths.is_contiguous() and ids.numel() % lengths.numel() == 0
        B = lengths.numel()
    check(lib.mmda_embed_rows_catch_up(ptr(_f(p)), ptr(_f(m)), ptr(_f(v)), ptr(state.row_step), ptr(state.ring), state.window, ptr(ids),
                                       ids.numel(), D, ptr(lengths), B, V, betas[0], betas[1], eps, state.seq, stream_ptr()),
          "embed_rows_catch_up")


def embed_rows_flush(p, m, v, state, betas=(0.9, 0.999), eps=1e-8):
    """Every stale row of p (and m, v) takes the updates it missed: afterwards the three hold what dense Adam over the table gives.
    With no update since the last flush nothing is launched."""
    lib = load()
    V, D = p.shape
    assert state.row_step.numel() == V
    if state.flushed == state.seq:
        return
    check(lib.mmda_embed_rows_flush(ptr(_f(p)), ptr(_f(m)), ptr(_f(v)), ptr(state.row_step), ptr(state.ring), state.window, D, V, betas[0],
                                    betas[1], eps, state.seq, stream_ptr()), "embed_rows_flush")
    state.flushed = state.seq


def heads_fwd(logits, ncls, threshold=0.35, drop_p=0.0, seed=0, site=0):
    lib = load()
    B = logits.shape[0]
    tcp = torch.empty(B, 6, device=logits.device); sc = torch.empty(B, ncls, device=logits.device)
    lab = torch.empty(B, ncls, device=logits.device)
    check(lib.mmda_heads_fwd(ptr(_f(logits)), B, ncls, threshold, ptr(tcp), ptr(sc), ptr(lab), drop_p, seed, site, stream_ptr()),
          "heads_fwd")
    return tcp, sc, lab


def heads_bwd(tcp, scores, dtcp, dscores, ncls, drop_p=0.0, seed=0, site=0):
    """d_logits (B, 6 + ncls) of the two sigmoid heads; ``dtcp`` / ``dscores`` may be None (that head's columns come out zero)."""
    lib = load()
    B = tcp.shape[0]
    dlogits = torch.empty(B, 6 + ncls, device=tcp.device)
    check(lib.mmda_heads_bwd(ptr(_f(tcp)), ptr(_f(scores)), ptr(None if dtcp is None else _f(dtcp)),
                             ptr(None if dscores is None else _f(dscores)), B, ncls, ptr(dlogits), drop_p, seed, site, stream_ptr()),
          "heads_bwd")
    return dlogits


def dropout_mask_via_act(n, p, seed, site, device):
    """Exposes the counter-based dropout multipliers (for the statistical tests): h = dropout(identity(1))."""
    lib = load()
    z = torch.ones(n, device=device); h = torch.empty(n, device=device)
    check(lib.mmda_act_dropout_fwd(ptr(z), ptr(h), n, ACT["none"], p, seed, site, stream_ptr()), "act_dropout_fwd")
    return h


def collate_gather(words, visual, acoustic, offsets, emo, sentiment, order, T, pad_id=1, out=None):
    """One batch of ``data.collate_fn`` gathered from a device-resident dataset in one launch: words int32 (P,), visual (P, dv), acoustic
    (P, da), offsets int64 (n + 1,), emo (n, 6) or None, sentiment (n,), all on the device; order int32 (B,) on the device, sample
    indices in batch order, every one in [0, n) (nothing on the device checks them).  Returns (ids int64 (T, B), visual (T, B, dv),
    acoustic (T, B, da), emo (B, 6) or None, sentiment (B,)), padding written by the launch itself.  ``out``: the same five tensors to
    write into (None in the emo slot when emo is None) instead of fresh ``torch.empty`` ones."""
    lib = load()
    B, dv, da = order.numel(), visual.shape[1], acoustic.shape[1]
    assert words.dtype == order.dtype == torch.int32 and offsets.dtype == torch.int64
    assert all(x.is_cuda and x.is_contiguous() for x in (words, visual, acoustic, offsets, sentiment, order) + (() if emo is None else (emo,)))
    assert words.numel() == visual.shape[0] == acoustic.shape[0] and offsets.numel() == sentiment.numel() + 1
    assert emo is None or (emo.dtype == torch.float32 and tuple(emo.shape) == (sentiment.numel(), 6))
    _f(visual); _f(acoustic); _f(sentiment)
    dev = words.device
    if out is None:
        out = (torch.empty(T, B, dtype=torch.int64, device=dev), torch.empty(T, B, dv, device=dev), torch.empty(T, B, da, device=dev),
               None if emo is None else torch.empty(B, 6, device=dev), torch.empty(B, device=dev))
    ids, v, a, e, y = out
    assert ids.dtype == torch.int64 and tuple(ids.shape) == (T, B) and tuple(v.shape) == (T, B, dv) and tuple(a.shape) == (T, B, da)
    assert tuple(y.shape) == (B,) and (e is None or tuple(e.shape) == (B, 6))
    assert all(x.is_cuda and x.is_contiguous() for x in (ids, v, a, y) + (() if e is None else (e,)))
    check(lib.mmda_collate_gather(ptr(words), ptr(visual), ptr(acoustic), ptr(offsets), ptr(emo), ptr(sentiment), ptr(order), B, int(T), dv,
                                  da, int(pad_id), ptr(ids), ptr(v), ptr(a), ptr(e), ptr(y), stream_ptr()), "collate_gather")
    return ids, v, a, e, y


def infer_collect(scores=None, labels=None, tcp=None, hfused=None, x6=None, probs=None, *, out, dst=None, base=0):
    """One batch of forward results copied into per-sample tables in one launch (``mmda_infer_collect``).  Sources, B columns: scores /
    labels (B, C), tcp (B, 6), hfused (B, 6 hs), x6 (6, B, hs), probs (B, nhead, 6, 6).  ``out``: dict of tables (n rows) by field name --
    scores, labels, tcp, hidden (n, 6 hs), utterance (n, 6, hs), attention (n, 6, 6); a missing field is skipped.  Column b goes to row
    ``dst[b]`` (int32 device tensor of B distinct rows in [0, n)), or to ``base + b``; nothing on the device checks the rows."""
    lib = load()
    srcs = dict(scores=scores, labels=labels, tcp=tcp, hfused=hfused, x6=x6, probs=probs)
    given = [t for t in srcs.values() if t is not None]
    assert given and all(t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 for t in given)
    cols = [t.shape[1] if k == "x6" else t.shape[0] for k, t in srcs.items() if t is not None]
    B = cols[0]
    assert all(c == B for c in cols)
    ncls = next((t.shape[1] for t in (scores, labels) if t is not None), 1)
    hs = x6.shape[2] if x6 is not None else (hfused.shape[1] // 6 if hfused is not None else 1)
    nhead = probs.shape[1] if probs is not None else 1
    unknown = set(out) - {"scores", "labels", "tcp", "hidden", "utterance", "attention"}
    assert not unknown, unknown
    n = None
    for t in out.values():
        assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float32
        n = t.shape[0] if n is None else n
        assert t.shape[0] == n
    if dst is not None:
        assert dst.dtype == torch.int32 and dst.is_cuda and dst.is_contiguous() and dst.numel() == B
    else:
        assert n is None or 0 <= base and base + B <= n
    s = _lib.InferSrc(ptr(scores), ptr(labels), ptr(tcp), ptr(hfused), ptr(x6), ptr(probs), int(ncls), int(hs), int(nhead))
    o = _lib.InferOut(*(ptr(out.get(k)) for k in ("scores", "labels", "tcp", "hidden", "utterance", "attention")))
    check(lib.mmda_infer_collect(C.byref(s), C.byref(o), ptr(dst), int(base), int(B), stream_ptr()), "infer_collect")
    return out


def misa_infer_collect(model, out, dst_ptr=None, base=0):
    """``mmda_misa_infer_collect``: the same with the sources taken from ``model``'s workspace as its last forward left them.  ``out``: an
    ``_lib.InferOut``; ``dst_ptr``: device address of the batch's int32 rows, or None for rows ``base .. base + B - 1``."""
    check(model._lib.mmda_misa_infer_collect(model._h, C.byref(out), dst_ptr, int(base), stream_ptr()), "misa_infer_collect")


# ---------------------------------------------------------------------------------------------- modality masking
def collate_gather_masked(words, visual, acoustic, offsets, emo, sentiment, order, T, keep=None, p=None, seed=0, pad_id=1, unk_id=0,
                          out=None, out_keep=None):
    """``collate_gather`` under a keep set, in the same one launch (``mmda_collate_gather_masked``).  ``keep``: the constant keep set
    (``modality.parse_keep``: None = everything, an int 0 .. 7 or modality names); ``p``: None or the drop rates (p_t, p_v, p_a) of the
    random keep set, a function of (``seed``, sample index); column b gets ``random_keep(order[b]) & keep``.  Returns ``collate_gather``'s
    five tensors and the columns' keep sets, uint8 (B,) (``out_keep``: the tensor to write them into)."""
    from .modality import parse_dropout, parse_keep
    lib = load()
    keep_const, p = parse_keep(keep), parse_dropout(p) or (0.0, 0.0, 0.0)
    B, dv, da = order.numel(), visual.shape[1], acoustic.shape[1]
    assert words.dtype == order.dtype == torch.int32 and offsets.dtype == torch.int64
    assert all(x.is_cuda and x.is_contiguous() for x in (words, visual, acoustic, offsets, sentiment, order) + (() if emo is None else (emo,)))
    assert words.numel() == visual.shape[0] == acoustic.shape[0] and offsets.numel() == sentiment.numel() + 1
    assert emo is None or (emo.dtype == torch.float32 and tuple(emo.shape) == (sentiment.numel(), 6))
    _f(visual); _f(acoustic); _f(sentiment)
    dev = words.device
    if out is None:
        out = (torch.empty(T, B, dtype=torch.int64, device=dev), torch.empty(T, B, dv, device=dev), torch.empty(T, B, da, device=dev),
               None if emo is None else torch.empty(B, 6, device=dev), torch.empty(B, device=dev))
    if out_keep is None:
        out_keep = torch.empty(B, dtype=torch.uint8, device=dev)
    ids, v, a, e, y = out
    assert ids.dtype == torch.int64 and tuple(ids.shape) == (T, B) and tuple(v.shape) == (T, B, dv) and tuple(a.shape) == (T, B, da)
    assert tuple(y.shape) == (B,) and (e is None or tuple(e.shape) == (B, 6))
    assert out_keep.dtype == torch.uint8 and tuple(out_keep.shape) == (B,)
    assert all(x.is_cuda and x.is_contiguous() for x in (ids, v, a, y, out_keep) + (() if e is None else (e,)))
    check(lib.mmda_collate_gather_masked(ptr(words), ptr(visual), ptr(acoustic), ptr(offsets), ptr(emo), ptr(sentiment), ptr(order), B,
                                         int(T), dv, da, int(pad_id), keep_const, _lib.ModalityP((C.c_float * 3)(*p)),
                                         int(seed) & 0xFFFFFFFFFFFFFFFF, int(unk_id), ptr(ids), ptr(v), ptr(a), ptr(e), ptr(y),
                                         ptr(out_keep), stream_ptr()), "collate_gather_masked")
    return ids, v, a, e, y, out_keep


def modality_mask(ids, v, a, keep, out=None, pad_id=1, unk_id=0):
    """Masked copies of a batch that exists already, in one launch (``mmda_modality_mask``): ids int64 (T, B), v (T, B, dv), a (T, B, da)
    on the device are read and never written.  ``keep``: a keep set for every column (``modality.parse_keep``) or a uint8 (B,) device
    tensor of one keep set per column.  An id equal to ``pad_id`` stays.  ``out``: the three tensors to write into (not the inputs)."""
    from .modality import parse_keep
    lib = load()
    assert ids.dim() == 2 and v.dim() == 3 and a.dim() == 3
    T, B = ids.shape
    dv, da = v.shape[2], a.shape[2]
    assert ids.dtype == torch.int64 and tuple(v.shape[:2]) == (T, B) and tuple(a.shape[:2]) == (T, B)
    _f(v); _f(a)
    assert all(x.is_cuda and x.is_contiguous() for x in (ids, v, a))
    if torch.is_tensor(keep):
        assert keep.dtype == torch.uint8 and keep.is_cuda and keep.is_contiguous() and tuple(keep.shape) == (B,)
        keep_ptr, keep_const = keep.data_ptr(), 7
    else:
        keep_ptr, keep_const = None, parse_keep(keep)
    if out is None:
        out = (torch.empty_like(ids), torch.empty_like(v), torch.empty_like(a))
    oi, ov, oa = out
    for x, y in zip(out, (ids, v, a)):
        assert x.is_cuda and x.is_contiguous() and x.dtype == y.dtype and x.shape == y.shape and x.data_ptr() != y.data_ptr()
    check(lib.mmda_modality_mask(ptr(ids), ptr(v), ptr(a), int(T), int(B), int(dv), int(da), keep_ptr, keep_const, int(pad_id), int(unk_id),
                                 ptr(oi), ptr(ov), ptr(oa), stream_ptr()), "modality_mask")
    return oi, ov, oa


def modality_attrib(V):
    """``V (8, n, C)`` fp32 on the device, V[k] = a value under keep set k -> ``(phi (n, 3, C), loo (n, 3, C), dominant (n, C) int32,
    counts (3, C) int64)`` from one ``mmda_modality_attrib`` launch: exact Shapley values of the three modalities, the leave-one-out
    differences, the modality with the largest Shapley value (-1 where all three are NaN) and the rows each modality dominates."""
    lib = load()
    assert V.dim() == 3 and V.shape[0] == 8 and V.is_cuda
    _f(V)
    V = V.contiguous()
    n, nc = int(V.shape[1]), int(V.shape[2])
    phi, loo = torch.empty(n, 3, nc, device=V.device), torch.empty(n, 3, nc, device=V.device)
    dominant = torch.empty(n, nc, dtype=torch.int32, device=V.device)
    counts = torch.empty(3, nc, dtype=torch.int64, device=V.device)
    check(lib.mmda_modality_attrib(ptr(V), n, nc, ptr(phi), ptr(loo), ptr(dominant), ptr(counts), stream_ptr()), "modality_attrib")
    return phi, loo, dominant, counts


KNN_PLAN_FIELDS = ("tile_q", "tile_b", "slab_rows", "slabs", "merge", "launches", "grid_x", "grid_y", "threads", "lds_bytes",
                   "vector_loads", "max_slabs", "work_bytes")


def knn_plan(Q, N, D, S=1, k=1):
    """The launches ``mmda_knn_sets`` gives a shape (mmda_knn_plan_describe: host code only, no GPU; the launcher reads the same
    function), as a dict: ``tile_q`` / ``tile_b`` (query / base rows of a distance tile), ``slab_rows`` and ``slabs`` (how the base is
    cut across workgroups), ``merge`` (whether the last launch merges more than one slab's lists), ``launches``, ``grid_x`` /
    ``grid_y`` / ``threads`` / ``lds_bytes`` of the search launch, ``vector_loads``, ``max_slabs`` and ``work_bytes`` (the buffer the
    caller allocates).  A shape outside the limits raises ``MMDAError``."""
    p = _lib.KnnPlan()
    check(load().mmda_knn_plan_describe(int(Q), int(N), int(D), int(S), int(k), C.byref(p)), "mmda_knn_plan_describe")
    return {f: bool(getattr(p, f)) if f in ("merge", "vector_loads") else int(getattr(p, f)) for f in KNN_PLAN_FIELDS}


def knn_sets(query, base, member, S, k, exclude_self=False, work=None):
    """``mmda_knn_sets`` over device tables: query (Q, D), base (N, D) fp32 contiguous, member (N,) int32 (bit s = row in set s) ->
    (dist (Q, S, k) fp32, index (Q, S, k) int32).  ``work``: None (allocated here, ``knn_plan``'s ``work_bytes``) or a uint8 device
    buffer of at least that size."""
    _f(query), _f(base)
    assert query.is_contiguous() and base.is_contiguous() and query.dim() == 2 and base.dim() == 2 and query.shape[1] == base.shape[1]
    assert member.is_cuda and member.dtype == torch.int32 and member.is_contiguous() and member.numel() == base.shape[0]
    Q, D, N = int(query.shape[0]), int(query.shape[1]), int(base.shape[0])
    plan = knn_plan(Q, N, D, S, k)
    if work is None:
        work = torch.empty(plan["work_bytes"], dtype=torch.uint8, device=query.device)
    dist = torch.empty(Q, int(S), int(k), dtype=torch.float32, device=query.device)
    index = torch.empty(Q, int(S), int(k), dtype=torch.int32, device=query.device)
    check(load().mmda_knn_sets(ptr(query) or ptr(base), ptr(base), ptr(member), Q, N, D, int(S), int(k), int(bool(exclude_self)),
                               ptr(dist) or ptr(base), ptr(index) or ptr(base), ptr(work), int(work.numel()), stream_ptr()),
          "mmda_knn_sets")
    return dist, index


def trust_score(dist, labels, index=None, tables=False):
    """``mmda_trust_score``: dist (n, 2 C, k) fp32 and the decisions labels (n, C) fp32 -> trust (n, C) float64; ``tables=True``
    (needs ``index`` (n, 2 C, k) int32): ``(trust, d_pred, d_other, nearest_pred, nearest_other)``."""
    _f(dist), _f(labels)
    n, C = int(labels.shape[0]), int(labels.shape[1])
    assert dist.is_contiguous() and labels.is_contiguous() and dist.dim() == 3 and dist.shape[0] == n and dist.shape[1] == 2 * C
    k = int(dist.shape[2])
    dev = dist.device
    trust = torch.empty(n, C, dtype=torch.float64, device=dev)
    extra = [None] * 4
    if tables:
        assert index is not None and index.dtype == torch.int32 and index.is_contiguous() and index.shape == dist.shape
        extra = [torch.empty(n, C, dtype=dt, device=dev) for dt in (torch.float32, torch.float32, torch.int32, torch.int32)]
    if n:
        check(load().mmda_trust_score(ptr(dist), ptr(index), ptr(labels), n, C, k, ptr(trust), *[ptr(t) for t in extra], stream_ptr()),
              "mmda_trust_score")
    return (trust, *extra) if tables else trust
