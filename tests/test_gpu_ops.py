"""Per-kernel parity on a real MI355X: every C-ABI operator against the same op computed by PyTorch on the CPU
(fp32).  fp32 mode tolerance 1e-4 (north_star), bf16 mode 1e-2, both relative to the tensor's max magnitude."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from oracle import misa_oracle as orc


def dev():
    return torch.device("cuda:0")


def relerr(got, ref):
    got = got.detach().float().cpu(); ref = ref.detach().float().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all(), "non-finite values in HIP output"
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-6))


TOL = {"fp32": 1e-4, "bf16": 1e-2}


# ------------------------------------------------------------------------------------------------ GEMM
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("M,N,K", [(1600, 2400, 300), (64, 64, 32), (33, 70, 35), (7, 12, 768), (192, 2048, 128), (100, 140, 74)])
def test_gemm_nt_bias(mode, M, N, K):
    from mmda_amd import ops
    torch.manual_seed(0)
    A = torch.randn(M, K); W = torch.randn(N, K) / math.sqrt(K); b = torch.randn(N); b2 = torch.randn(N)
    ref = A @ W.t() + b + b2
    out = ops.gemm(A.to(dev()), W.to(dev()), mode=mode, bias=b.to(dev()), bias2=b2.to(dev()))
    assert relerr(out, ref) < TOL[mode]


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_gemm_nn_tn_accumulate_alpha(mode):
    from mmda_amd import ops
    torch.manual_seed(1)
    M, N, K = 150, 300, 1200
    dY = torch.randn(M, N); W = torch.randn(N, K) / math.sqrt(N); X = torch.randn(M, K)
    # dX = dY W  (NN)
    out = ops.gemm(dY.to(dev()), W.to(dev()), mode=mode, transB=False)
    assert relerr(out, dY @ W) < TOL[mode]
    # dW += dY^T X (TN, accumulate) with alpha
    C0 = torch.randn(N, K)
    out = ops.gemm(dY.to(dev()), X.to(dev()), mode=mode, transA=True, transB=False, out=C0.clone().to(dev()), accumulate=True,
                   alpha=-0.5)
    assert relerr(out, C0 - 0.5 * dY.t() @ X) < TOL[mode]


# ------------------------------------------------------------------------------------------------ bf16-operand GEMM + conversion
def test_convert_bf16_plain_transposed_gather_padding():
    """fp32 -> bf16 copies (plain / transposed / gathered) are the round-to-nearest-even values with zero padding."""
    from mmda_amd import ops
    torch.manual_seed(3)
    X = torch.randn(130, 37); W = torch.randn(1200, 300); E = torch.randn(50, 300)
    ids = torch.randint(0, 50, (77,))
    (Xp, Xt), (Wp, Wt), (Gp, Gt), (_, Tt) = ops.convert_bf16([
        (X.to(dev()), None, True, True), (W.to(dev()), None, True, True), (E.to(dev()), ids.to(dev()), True, True),
        (X.to(dev()), None, False, True)])
    for src, P, T in ((X, Xp, Xt), (W, Wp, Wt), (E[ids], Gp, Gt), (X, None, Tt)):
        ref = src.to(torch.bfloat16)
        r, c = src.shape
        if P is not None:
            assert torch.equal(P.cpu()[:, :c], ref) and bool((P.cpu()[:, c:] == 0).all())
        assert torch.equal(T.cpu()[:, :r], ref.t()) and bool((T.cpu()[:, r:] == 0).all())
    # bf16 source (re-layout only): transpose of a bf16 matrix with a padded leading dimension
    Sb = torch.randn(130, 40).to(torch.bfloat16).to(dev())
    (Pb, Tb), = ops.convert_bf16([(Sb[:, :37], None, True, True)])
    assert torch.equal(Pb.cpu()[:, :37], Sb.cpu()[:, :37]) and bool((Pb.cpu()[:, 37:] == 0).all())
    assert torch.equal(Tb.cpu()[:, :130], Sb.cpu()[:, :37].t()) and bool((Tb.cpu()[:, 130:] == 0).all())


@pytest.mark.parametrize("rows,cols", [(130, 300), (77, 148), (1601, 600), (50, 12), (3, 4), (257, 2400), (64, 64)])
def test_convert_bf16_16_byte_form(rows, cols):
    """Shapes that take the 16-byte form of the conversion (16-byte-aligned rows, columns a multiple of 4 / 8): plain, transposed,
    gathered and bf16-source jobs in one launch, odd row counts, the 4-element padding of a 300-wide plain copy."""
    from mmda_amd import ops
    torch.manual_seed(rows * 7 + cols)
    X = torch.randn(rows, cols)
    E = torch.randn(40, cols); ids = torch.randint(0, 40, (rows,))
    c8 = cols // 8 * 8
    Sb = torch.randn(rows, cols + 8).to(torch.bfloat16).to(dev())          # bf16 source inside a wider (16-byte-aligned) buffer
    jobs = [(X.to(dev()), None, True, True), (X.to(dev()), None, False, True), (X.to(dev()), None, True, False),
            (E.to(dev()), ids.to(dev()), True, True)]
    if c8 >= 8:
        jobs.append((Sb[:, :c8], None, True, True))
    outs = ops.convert_bf16(jobs)
    refs = [X, X, X, E[ids]] + ([Sb.cpu()[:, :c8].float()] if c8 >= 8 else [])
    for (P, T), src in zip(outs, refs):
        ref = src.to(torch.bfloat16)
        r, c = src.shape
        if P is not None:
            assert torch.equal(P.cpu()[:, :c], ref) and bool((P.cpu()[:, c:] == 0).all())
        if T is not None:
            assert torch.equal(T.cpu()[:, :r], ref.t()) and bool((T.cpu()[:, r:] == 0).all())


@pytest.mark.parametrize("M,N,K", [(1600, 2400, 300), (1600, 1200, 300), (128, 128, 64), (33, 70, 35), (7, 12, 768), (1600, 140, 40),
                                   (300, 128, 1600), (8320, 2400, 300), (8200, 600, 1100), (8200, 300, 2400)])
def test_gemm_bf16_operands_nt_bias(M, N, K):
    """C = A B^T + b + b2 on bf16 K-major operands: exact against fp32 matmul of the same bf16-rounded values (up to fp32
    summation order), so the bar is the fp32 one.  The shapes with >= 8192 rows take the LDS-DMA pipelined kernel (round 3), rows /
    columns / depth off the tile grid (128 x 128 tiles; the 256 x 128 class for K >= 1024 is off by default:
    test_gemm_bf16_tall_class_in_a_fresh_process)."""
    from mmda_amd import ops
    torch.manual_seed(4)
    A = torch.randn(M, K); W = torch.randn(N, K) / math.sqrt(K); b = torch.randn(N); b2 = torch.randn(N)
    (Ap, _), (Wp, _) = ops.convert_bf16([(A.to(dev()), None, True, False), (W.to(dev()), None, True, False)])
    ref = A.bfloat16().float() @ W.bfloat16().float().t() + b + b2
    out, = ops.gemm_bf16_grouped([dict(A=Ap, B=Wp, K=K, bias=b.to(dev()), bias2=b2.to(dev()))])
    assert relerr(out, ref) < TOL["fp32"]


def test_gemm_bf16_grouped_backward_forms_bias_grad_accumulate():
    """The three products of one LSTM layer's backward in one grouped launch, all in NT form on converted copies:
    dX = dG W (B = W^T copy), dW += dG^T X (A = dG^T copy, B = X^T copy, bias gradient as the ones row, accumulate, alpha),
    and a sub-matrix (row offset) operand as used by the time-shifted dW_hh product."""
    from mmda_amd import ops
    torch.manual_seed(5)
    R, G4, I = 1600, 280, 35
    dG = torch.randn(R, G4); W = torch.randn(G4, I) / 6; X = torch.randn(R, I); C0 = torch.randn(G4, I)
    (dGp, dGt), (_, Wt), (_, Xt) = ops.convert_bf16([(dG.to(dev()), None, True, True), (W.to(dev()), None, False, True),
                                                     (X.to(dev()), None, False, True)])
    dGb, Wb, Xb = dG.bfloat16().float(), W.bfloat16().float(), X.bfloat16().float()
    bg = torch.zeros(G4, device=dev()); bg2 = torch.ones(G4, device=dev())
    shift = 64                                        # rows [shift, R) of dG against rows [0, R - shift) of X
    outs = ops.gemm_bf16_grouped([
        dict(A=dGp, B=Wt, K=G4),
        dict(A=dGt, B=Xt, K=R, out=C0.clone().to(dev()), accumulate=True, alpha=-0.5, bias_grad=bg, bias_grad2=bg2),
        dict(A=dGt[:, shift:].contiguous(), B=Xt[:, :Xt.shape[1] - shift].contiguous(), K=R - shift),
    ])
    assert relerr(outs[0], dGb @ Wb) < TOL["fp32"]
    assert relerr(outs[1], C0 - 0.5 * dGb.t() @ Xb) < TOL["fp32"]
    assert relerr(bg, dGb.sum(0)) < TOL["fp32"] and relerr(bg2, 1 + dGb.sum(0)) < TOL["fp32"]
    assert relerr(outs[2], dGb[shift:].t() @ Xb[:R - shift]) < TOL["fp32"]


@pytest.mark.parametrize("M,N,K,lda,ldb,a0,b0", [(2400, 300, 1600, 2400, 304, 0, 0), (140, 35, 1550, 280, 80, 140, 40),
                                                  (1200, 300, 12750, 2400, 608, 1200, 304), (64, 64, 64, 64, 64, 0, 0),
                                                  (296, 74, 490, 592, 160, 296, 80)])
def test_gemm_bf16_tn_form_weight_gradient(M, N, K, lda, ldb, a0, b0):
    """tn form: C = A^T B on (K, M)- and (K, N)-major operands (dW = dG^T X on the tensors as they lie; transposing LDS reads), with
    the bias gradient as a virtual ones-column, accumulate, column windows that start off the 16-byte grid (the reverse direction's
    half of dG for a 35-wide LSTM: a0 = 280 bytes; b0: the per-direction bf16 copy of hseq) and split-K -- against an fp32 matmul of the same bf16 values."""
    from mmda_amd import ops
    torch.manual_seed(M + N + K)
    A = (torch.randn(K, lda) * 0.5).to(torch.bfloat16).to(dev())
    Bm = (torch.randn(K, ldb) * 0.5).to(torch.bfloat16).to(dev())
    C0 = torch.randn(M, N)
    bg = torch.zeros(M, device=dev())
    out, = ops.gemm_bf16_grouped([dict(A=A[:, a0:], B=Bm[:, b0:], M=M, N=N, K=K, tn=True, out=C0.clone().to(dev()), accumulate=True,
                                       bias_grad=bg)])
    Af, Bf = A.float().cpu()[:, a0:a0 + M], Bm.float().cpu()[:, b0:b0 + N]
    want = C0 + Af.t() @ Bf
    tol = 3e-5 * float(want.abs().max()) * max(1.0, (K / 1600) ** 0.5)
    assert float((out.cpu() - want).abs().max()) < tol, (M, N, K)
    assert float((bg.cpu() - Af.sum(0)).abs().max()) < 3e-5 * float(Af.sum(0).abs().max()) * max(1.0, (K / 1600) ** 0.5)


def test_gemm_bf16_split_k_is_bitwise_reproducible():
    """Split-K combines through per-slice slabs summed in slice order by a reduce launch (splitk.hip), not through float atomics: the
    weight-gradient launch of an LSTM layer (tn form, bias-gradient column, accumulate) twice on the same inputs gives the same bits.
    What runs, by ops.gemm_bf16_plan (test_gemm_bf16_plan_cpu.py pins it): at K = 1600 both problems stay whole on the register-staged
    64 x 64 mixed instance (25 k-tiles: no split below 128); at K = 12800 the first is split in 9 on the LDS-DMA kernel and the second,
    whose hseq window starts off the 16-byte grid, in 10 on the register-staged one -- both split policies behind one reduce launch."""
    from mmda_amd import ops
    torch.manual_seed(77)
    for K in (1600, 12800):
        A = (torch.randn(K, 2400) * 0.5).to(torch.bfloat16).to(dev()); Bm = (torch.randn(K, 304) * 0.5).to(torch.bfloat16).to(dev())
        H = (torch.randn(K, 600) * 0.5).to(torch.bfloat16).to(dev())
        outs = []
        for _ in range(2):
            C = torch.ones(2400, 300, device=dev()); C2 = torch.ones(1200, 300, device=dev()); bg = torch.zeros(2400, device=dev())
            ops.gemm_bf16_grouped([dict(A=A, B=Bm, M=2400, N=300, K=K, tn=True, out=C, accumulate=True, bias_grad=bg),
                                   dict(A=A[:, 1200:], B=H[:, 300:], M=1200, N=300, K=K, tn=True, out=C2, accumulate=True)])
            outs.append((C.clone(), C2.clone(), bg.clone()))
        for x, y in zip(*outs):
            assert torch.equal(x, y)
        ref = 1 + A.float().t() @ Bm.float()[:, :300]
        assert float((outs[0][0] - ref).abs().max()) < 3e-5 * float(ref.abs().max()) * max(1.0, (K / 1600) ** 0.5)
        assert relerr(outs[0][2], A.float().sum(0)) < TOL["fp32"]


def _tn_bar(want, K):
    """test_gemm_bf16_tn_form_weight_gradient's bar: absolute, against the largest expected magnitude"""
    return 3e-5 * float(want.abs().max()) * max(1.0, (K / 1600) ** 0.5)


def test_gemm_bf16_grouped_more_problems_than_a_launch_holds():
    """18 problems in one call, nt and tn mixed: one kernel class whose problems are cut into a launch of 16 and a launch of 2 (the cut
    falls in the middle of the class's K-ordered list), and nt problems that run on the mixed (tn-capable) instance.  Shapes of the
    tests above, every output at the bar its shape has there."""
    from mmda_amd import ops
    torch.manual_seed(18)
    problems, checks = [], []
    for i in range(18):
        kind = i % 5
        if kind < 3:
            M, N, K = ((33, 70, 35), (7, 12, 768), (128, 128, 64))[kind]
            A = torch.randn(M, K); W = torch.randn(N, K) / math.sqrt(K)
            (Ap, _), (Wp, _) = ops.convert_bf16([(A.to(dev()), None, True, False), (W.to(dev()), None, True, False)])
            p = dict(A=Ap, B=Wp, K=K)
            want = A.bfloat16().float() @ W.bfloat16().float().t()
            if kind == 2:
                b = torch.randn(N)
                p["bias"] = b.to(dev()); want = want + b
            checks.append(("nt", K, want, None, None))
        elif kind == 3:
            M = N = K = 64
            A = (torch.randn(K, M) * 0.5).to(torch.bfloat16).to(dev()); Bm = (torch.randn(K, N) * 0.5).to(torch.bfloat16).to(dev())
            p = dict(A=A, B=Bm, M=M, N=N, K=K, tn=True)
            checks.append(("tn", K, A.float().cpu().t() @ Bm.float().cpu(), None, None))
        else:
            M, N, K, lda, ldb, a0, b0 = 140, 35, 96, 280, 80, 140, 40
            A = (torch.randn(K, lda) * 0.5).to(torch.bfloat16).to(dev()); Bm = (torch.randn(K, ldb) * 0.5).to(torch.bfloat16).to(dev())
            C0 = torch.randn(M, N); bg = torch.zeros(M, device=dev())
            p = dict(A=A[:, a0:], B=Bm[:, b0:], M=M, N=N, K=K, tn=True, out=C0.clone().to(dev()), accumulate=True, bias_grad=bg)
            Af, Bf = A.float().cpu()[:, a0:a0 + M], Bm.float().cpu()[:, b0:b0 + N]
            checks.append(("tn", K, C0 + Af.t() @ Bf, bg, Af.sum(0)))
        problems.append(p)
    outs = ops.gemm_bf16_grouped(problems)
    for i, (out, (form, K, want, bg, want_bg)) in enumerate(zip(outs, checks)):
        if form == "nt":
            assert relerr(out, want) < TOL["fp32"], i
        else:
            assert float((out.cpu() - want).abs().max()) < _tn_bar(want, K), i
        if bg is not None:
            assert float((bg.cpu() - want_bg).abs().max()) < _tn_bar(want_bg, K), i


def test_gemm_bf16_grouped_classes_and_both_split_policies_in_one_call():
    """One call whose problems land in two kernel classes and are split by both policies: a tn weight gradient in the LDS-DMA class
    (the call holds >= 8192 k-rows; split into equal-length pieces), a tn weight gradient of one 64 x 64 tile walking 129 k-tiles
    (register-staged class, split because nk >= 128) and a small unsplit nt product -- the slabs of two classes behind one reduce
    launch.  Against the fp32 matmul of the same bf16 values; twice on fresh outputs, same bits."""
    from mmda_amd import ops
    torch.manual_seed(8256)
    K = 8256
    A1 = (torch.randn(K, 256) * 0.5).to(torch.bfloat16).to(dev()); B1 = (torch.randn(K, 96) * 0.5).to(torch.bfloat16).to(dev())
    A2 = (torch.randn(K, 64) * 0.5).to(torch.bfloat16).to(dev()); B2 = (torch.randn(K, 64) * 0.5).to(torch.bfloat16).to(dev())
    A3 = torch.randn(33, 35); W3 = torch.randn(70, 35) / math.sqrt(35); b3 = torch.randn(70)
    (A3p, _), (W3p, _) = ops.convert_bf16([(A3.to(dev()), None, True, False), (W3.to(dev()), None, True, False)])
    C1 = torch.randn(256, 96); C2 = torch.randn(64, 64)
    runs = []
    for _ in range(2):
        bg = torch.zeros(256, device=dev())
        outs = ops.gemm_bf16_grouped([
            dict(A=A1, B=B1, M=256, N=96, K=K, tn=True, out=C1.clone().to(dev()), accumulate=True, bias_grad=bg),
            dict(A=A2, B=B2, M=64, N=64, K=K, tn=True, out=C2.clone().to(dev()), accumulate=True),
            dict(A=A3p, B=W3p, K=35, bias=b3.to(dev()))])
        runs.append([o.cpu() for o in outs] + [bg.cpu()])
    for x, y in zip(*runs):
        assert torch.equal(x, y)
    o1, o2, o3, bg = runs[0]
    want1 = C1 + A1.float().cpu().t() @ B1.float().cpu()
    want2 = C2 + A2.float().cpu().t() @ B2.float().cpu()
    want_bg = A1.float().cpu().sum(0)
    assert float((o1 - want1).abs().max()) < _tn_bar(want1, K)
    assert float((bg - want_bg).abs().max()) < _tn_bar(want_bg, K)
    assert float((o2 - want2).abs().max()) < _tn_bar(want2, K)
    assert relerr(o3, A3.bfloat16().float() @ W3.bfloat16().float().t() + b3) < TOL["fp32"]


def test_gemm_bf16_gate_interleave():
    """The gate-minor layout end to end at GEMM level: W_ih rows interleaved by the conversion, bias read through the
    interleave (forward); dW rows and bias gradients written back through it (backward)."""
    from mmda_amd import ops, _lib
    import ctypes as C
    torch.manual_seed(12)
    R, H, D = 96, 35, 40
    X = torch.randn(R, D); W = torch.randn(8 * H, D) / 6; b = torch.randn(8 * H)
    perm = torch.tensor([(j // (4 * H)) * 4 * H + (j % 4) * H + (j % (4 * H)) // 4 for j in range(8 * H)])
    lib = _lib.load()
    d = dev()
    Xd, Wd = X.to(d), W.to(d)
    ldD = (D + 7) // 8 * 8; ldR = (R + 7) // 8 * 8
    Xb = torch.zeros(R, ldD, device=d, dtype=torch.bfloat16); XbT = torch.zeros(D, ldR, device=d, dtype=torch.bfloat16)
    Wb = torch.zeros(8 * H, ldD, device=d, dtype=torch.bfloat16)
    jobs = (_lib.ConvertJob * 2)()
    jobs[0].src = Xd.data_ptr(); jobs[0].ld = D; jobs[0].rows = R; jobs[0].cols = D; jobs[0].plain = Xb.data_ptr(); jobs[0].ldp = ldD
    jobs[0].transposed = XbT.data_ptr(); jobs[0].ldt = ldR
    jobs[1].src = Wd.data_ptr(); jobs[1].ld = D; jobs[1].rows = 8 * H; jobs[1].cols = D; jobs[1].plain = Wb.data_ptr(); jobs[1].ldp = ldD
    jobs[1].row_perm_H = H
    _lib.check(lib.mmda_convert_bf16(jobs, 2, _lib.stream_ptr()), "convert")
    assert torch.equal(Wb.cpu()[:, :D], W[perm].bfloat16())
    # forward: gates (interleaved columns) = X W'^T + b[orig]
    gates = torch.zeros(R, 8 * H, device=d)
    g = (_lib.GemmBf16Args * 1)()
    g[0].M = R; g[0].N = 8 * H; g[0].K = D; g[0].A = Xb.data_ptr(); g[0].lda = ldD; g[0].B = Wb.data_ptr(); g[0].ldb = ldD
    g[0].C = gates.data_ptr(); g[0].ldc = 8 * H; bd = b.to(d); g[0].bias = bd.data_ptr(); g[0].perm_n_H = H
    _lib.check(lib.mmda_gemm_bf16_grouped(g, 1, _lib.stream_ptr()), "gemm fwd")
    ref = X.bfloat16().float() @ W.bfloat16().float().t() + b
    assert relerr(gates, ref[:, perm]) < TOL["fp32"]
    # backward: dW[orig(m)] += dG'^T X, bias gradient likewise
    dG = torch.randn(R, 8 * H)                       # in interleaved column order
    (_, dGT), = ops.convert_bf16([(dG.to(d), None, False, True)])
    dW = torch.zeros(8 * H, D, device=d); db = torch.zeros(8 * H, device=d)
    g[0] = _lib.GemmBf16Args()
    g[0].M = 8 * H; g[0].N = D; g[0].K = R; g[0].A = dGT.data_ptr(); g[0].lda = dGT.shape[1]; g[0].B = XbT.data_ptr(); g[0].ldb = ldR
    g[0].C = dW.data_ptr(); g[0].ldc = D; g[0].accumulate = 1; g[0].bias_grad = db.data_ptr(); g[0].perm_m_H = H
    _lib.check(lib.mmda_gemm_bf16_grouped(g, 1, _lib.stream_ptr()), "gemm bwd")
    ref_dW = torch.zeros(8 * H, D); ref_dW[perm] = dG.bfloat16().float().t() @ X.bfloat16().float()
    ref_db = torch.zeros(8 * H); ref_db[perm] = dG.bfloat16().float().sum(0)
    assert relerr(dW, ref_dW) < TOL["fp32"] and relerr(db, ref_db) < TOL["fp32"]


def test_gemm_bf16_rejects_misaligned_operands():
    from mmda_amd import ops, _lib
    A = torch.zeros(16, 24, device=dev(), dtype=torch.bfloat16); B = torch.zeros(16, 24, device=dev(), dtype=torch.bfloat16)
    with pytest.raises(_lib.MMDAError):
        ops.gemm_bf16_grouped([dict(A=A, B=B, K=30)])            # K beyond the padded leading dimension



# ------------------------------------------------------------------------------------------------ row-skinny f32 GEMM (fusion block)
@pytest.mark.parametrize("M,N,K", [(32, 128, 1200), (32, 128, 140), (32, 128, 296), (96, 128, 128), (192, 384, 128), (192, 2048, 128),
                                   (192, 128, 2048), (32, 12, 768), (7, 5, 3), (33, 17, 70), (1, 128, 16)])
def test_gemm_skinny_nt_bias_act(M, N, K):
    """y = act(x W^T + b): every forward Linear of the fusion block, plus ragged shapes that take the scalar-load path."""
    from mmda_amd import ops
    torch.manual_seed(6)
    A = torch.randn(M, K); W = torch.randn(N, K) / math.sqrt(K); b = torch.randn(N)
    for act, f in (("none", lambda t: t), ("sigmoid", torch.sigmoid), ("relu", torch.relu)):
        out, = ops.gemm_skinny([dict(A=A.to(dev()), B=W.to(dev()), bias=b.to(dev()), act=act)])
        assert relerr(out, f(A @ W.t() + b)) < TOL["fp32"], act


@pytest.mark.parametrize("M,N,K", [(32, 768, 12), (192, 2048, 128), (192, 128, 2048), (192, 128, 384), (32, 1200, 128), (96, 128, 3),
                                   (33, 70, 17)])
def test_gemm_skinny_nn_accumulate_alpha(M, N, K):
    """dx (+)= alpha * dy W (W is (K, N), n contiguous): every input gradient of the fusion block."""
    from mmda_amd import ops
    torch.manual_seed(7)
    dY = torch.randn(M, K); W = torch.randn(K, N) / math.sqrt(K); C0 = torch.randn(M, N)
    out, = ops.gemm_skinny([dict(A=dY.to(dev()), B=W.to(dev()), transB=False)])
    assert relerr(out, dY @ W) < TOL["fp32"]
    out, = ops.gemm_skinny([dict(A=dY.to(dev()), B=W.to(dev()), transB=False, out=C0.clone().to(dev()), accumulate=True, alpha=-0.25)])
    assert relerr(out, C0 - 0.25 * dY @ W) < TOL["fp32"]


def test_gemm_skinny_grouped_epilogues():
    """One launch, several problems: A + A2 operand, two products into one output, second destination with its own sigmoid
    factor, relu gate, unaligned operand bases (scalar path) next to aligned ones; the launch is bitwise reproducible."""
    from mmda_amd import ops
    torch.manual_seed(8)
    B_, hs = 32, 128
    priv = torch.rand(B_, hs); shared = torch.rand(B_, hs); Wr = torch.randn(hs, hs) / 11; br = torch.randn(hs)
    d1 = torch.randn(B_, hs); W1 = torch.randn(hs, hs) / 11; d2 = torch.randn(B_, hs); W2 = torch.randn(hs, hs) / 11; C0 = torch.randn(B_, hs)
    dr = torch.randn(B_, hs); s1 = torch.rand(B_, hs); s2 = torch.rand(B_, hs); ca = torch.randn(B_, hs); cb = torch.randn(B_, hs)
    df2 = torch.randn(192, hs); W_l2 = torch.randn(hs, 2048) / 11; f1 = torch.relu(torch.randn(192, 2048))
    big = torch.randn(hs * hs + 1, device=dev())
    W_un = big[1:].view(hs, hs)                          # 4-byte aligned only: scalar-load path
    xs = torch.randn(B_, hs)

    def run():
        ca_d, cb_d = ca.clone().to(dev()), cb.clone().to(dev())
        outs = ops.gemm_skinny([
            dict(A=priv.to(dev()), A2=shared.to(dev()), B=Wr.to(dev()), bias=br.to(dev())),
            dict(A=d1.to(dev()), B=W1.to(dev()), A_2nd=d2.to(dev()), B_2nd=W2.to(dev()), transB=False, out=C0.clone().to(dev()),
                 accumulate=True),
            dict(A=dr.to(dev()), B=Wr.to(dev()), transB=False, out=ca_d, out2=cb_d, accumulate=True, dsig=s1.to(dev()), dsig2=s2.to(dev())),
            dict(A=df2.to(dev()), B=W_l2.to(dev()), transB=False, gate=f1.to(dev()), gate_scale=1.25),
            dict(A=xs.to(dev()), B=W_un),
        ])
        return outs + [cb_d]

    o = run()
    assert relerr(o[0], (priv + shared) @ Wr.t() + br) < TOL["fp32"]
    assert relerr(o[1], C0 + d1 @ W1 + d2 @ W2) < TOL["fp32"]
    assert relerr(o[2], (ca + dr @ Wr) * s1 * (1 - s1)) < TOL["fp32"]
    assert relerr(o[5], (cb + dr @ Wr) * s2 * (1 - s2)) < TOL["fp32"]
    assert relerr(o[3], (df2 @ W_l2) * (f1 > 0) * 1.25) < TOL["fp32"]
    assert relerr(o[4], xs @ W_un.cpu().t()) < TOL["fp32"]
    o2 = run()
    for x, y in zip(o, o2):
        assert torch.equal(x, y), "fixed-order reduction must be bitwise reproducible"


def test_gemm_skinny_dropout_matches_generic_kernel_mask():
    """Same (seed, site, m*N+n) stream as mmda_gemm: the FFN's dropout mask does not depend on which kernel computed it."""
    from mmda_amd import ops
    torch.manual_seed(9)
    x = torch.randn(192, 128, device=dev()); W = torch.randn(2048, 128, device=dev()) / 11; b = torch.randn(2048, device=dev())
    a = ops.gemm(x, W, mode="fp32", bias=b, act="relu", drop_p=0.1, seed=77, site=3)
    s, = ops.gemm_skinny([dict(A=x, B=W, bias=b, act="relu", drop_p=0.1, seed=77, site=3)])
    assert torch.equal(a == 0, s == 0)
    assert relerr(s, a) < TOL["fp32"]



@pytest.mark.parametrize("shape", ["tn_dwih", "nn_dx", "tn_dwhh_offsets", "nt_small_k"])
def test_gemm_128_tile_kernel_lstm_shapes(shape):
    """The aligned bf16 fast kernel (128x128 tile, 16-byte staging) on the LSTM-sized GEMMs of the backward pass,
    including split-K and sub-matrix (row/column offset) operands."""
    from mmda_amd import ops, _lib
    import ctypes as C
    torch.manual_seed(13)
    d = dev()
    T, B, H, D = 50, 32, 300, 600
    R = T * B
    if shape == "tn_dwih":          # dW_ih (8H, D) += dG^T X
        dG = torch.randn(R, 8 * H) * 0.1; X = torch.randn(R, D)
        C0 = torch.randn(8 * H, D)
        out = ops.gemm(dG.to(d), X.to(d), mode="bf16", transA=True, transB=False, out=C0.clone().to(d), accumulate=True)
        assert relerr(out, C0 + dG.t() @ X) < 1e-2
    elif shape == "nn_dx":          # dX (R, D) = dG W_ih
        dG = torch.randn(R, 8 * H) * 0.1; W = torch.randn(8 * H, D) / math.sqrt(D)
        out = ops.gemm(dG.to(d), W.to(d), mode="bf16", transB=False)
        assert relerr(out, dG @ W) < 1e-2
    elif shape == "nt_small_k":     # gates = X W^T + b, K = 300 (9 full k-tiles + 12)
        X = torch.randn(R, 300); W = torch.randn(8 * H, 300) / math.sqrt(300); b = torch.randn(8 * H)
        out = ops.gemm(X.to(d), W.to(d), mode="bf16", bias=b.to(d))
        assert relerr(out, X @ W.t() + b) < 1e-2
    else:                           # dW_hh: dG[1:, :, fwd] with hseq[:-1, :, :H]; and the reverse pairing, in place on views
        dG = (torch.randn(T, B, 2, 4 * H) * 0.1); hs = torch.randn(T, B, 2 * H)
        ref_f = dG[1:, :, 0].reshape(-1, 4 * H).t() @ hs[:-1, :, :H].reshape(-1, H)
        ref_r = dG[:-1, :, 1].reshape(-1, 4 * H).t() @ hs[1:, :, H:].reshape(-1, H)
        dGd, hsd = dG.to(d), hs.to(d)
        lib = _lib.load()
        for ref, a_off, b_off in ((ref_f, B * 8 * H, 0), (ref_r, 4 * H, B * 2 * H + H)):
            out = torch.zeros(4 * H, H, device=d)
            g = _lib.GemmArgs()
            g.mode = 1; g.transA = 1; g.transB = 0; g.M = 4 * H; g.N = H; g.K = (T - 1) * B; g.batch = 1
            g.A = dGd.data_ptr() + 4 * a_off; g.lda = 8 * H; g.B = hsd.data_ptr() + 4 * b_off; g.ldb = 2 * H
            g.C = out.data_ptr(); g.ldc = H; g.accumulate = 1
            _lib.check(lib.mmda_gemm(C.byref(g), _lib.stream_ptr()))
            assert relerr(out, ref) < 1e-2


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("M,N,K", [(1600, 2400, 300), (192, 128, 128), (32, 12, 768), (96, 128, 2048)])
def test_gemm_weight_grad_with_fused_bias_grad(mode, M, N, K):
    """dW += dY^T X and db += colsum(dY) (also db2) out of ONE GEMM: the bias gradient is a virtual all-ones column of X.
    N multiple of 64 (extra tile column), split-K and non-split shapes."""
    from mmda_amd import ops
    torch.manual_seed(14)
    dY = torch.randn(M, N) * 0.3; X = torch.randn(M, K)
    dW0 = torch.randn(N, K); db0 = torch.randn(N); db20 = torch.zeros(N)
    d = dev()
    db = db0.clone().to(d); db2 = db20.clone().to(d)
    out = ops.gemm(dY.to(d), X.to(d), mode=mode, transA=True, transB=False, out=dW0.clone().to(d), accumulate=True, bias_grad=db,
                   bias_grad2=db2)
    assert relerr(out, dW0 + dY.t() @ X) < TOL[mode]
    assert relerr(db, db0 + dY.sum(0)) < TOL[mode] and relerr(db2, dY.sum(0)) < TOL[mode]


def _grouped_problems(d):
    """18 small problems for one mmda_gemm_grouped call: (layout, mode, M, N, K, extras).  K = 768 is 24 k-tiles (splits unless the
    epilogue forbids it), K = 35 is two (never splits).  Returns a maker of fresh problem lists and the float64 references."""
    spec = [("nt", "fp32", 33, 70, 768, {}), ("nt", "bf16", 70, 35, 768, {}), ("nn", "fp32", 35, 33, 768, {}),
            ("nn", "bf16", 140, 70, 35, {}), ("tn", "fp32", 70, 33, 768, {"bias_grad": True, "accumulate": True}),
            ("tn", "bf16", 35, 140, 768, {}), ("nt", "fp32", 7, 12, 35, {}), ("nt", "fp32", 0, 33, 768, {}),
            ("nt", "bf16", 64, 64, 768, {"act": "relu"}), ("nn", "fp32", 65, 129, 35, {}), ("tn", "fp32", 33, 35, 35, {}),
            ("nt", "bf16", 128, 33, 35, {}), ("nn", "bf16", 33, 65, 768, {}), ("tn", "bf16", 70, 70, 35, {}),
            ("nt", "fp32", 140, 140, 768, {"alpha": -0.5}), ("nn", "fp32", 1, 70, 768, {}),
            ("tn", "bf16", 33, 70, 768, {}), ("nt", "fp32", 35, 7, 35, {})]
    g = torch.Generator().manual_seed(21)
    data, refs = [], []
    for lay, mode, M, N, K, ex in spec:
        A = torch.randn((K, M) if lay == "tn" else (M, K), generator=g)
        B = torch.randn((N, K) if lay == "nt" else (K, N), generator=g) / math.sqrt(K)
        C0 = torch.randn(M, N, generator=g); bg0 = torch.randn(M, generator=g)
        opA = A.double().t() if lay == "tn" else A.double(); opB = B.double().t() if lay == "nt" else B.double()
        ref = ex.get("alpha", 1.0) * (opA @ opB)
        if ex.get("accumulate"):
            ref = ref + C0.double()
        if ex.get("act") == "relu":
            ref = ref.clamp_min(0)
        data.append((A.to(d), B.to(d), C0, bg0))
        refs.append((ref, bg0.double() + opA.sum(1)))

    def make():
        probs = []
        for (lay, mode, M, N, K, ex), (A, B, C0, bg0) in zip(spec, data):
            # (a problem without rows still names real buffers: empty views of one-row tensors)
            p = dict(A=A if M else torch.zeros(1, K, device=d)[:0], B=B, mode=mode, transA=lay == "tn", transB=lay == "nt")
            if ex.get("accumulate"):
                p.update(out=C0.clone().to(d), accumulate=True)
            if ex.get("bias_grad"):
                p.update(bias_grad=bg0.clone().to(d))
            p.update({k: v for k, v in ex.items() if k in ("act", "alpha")})
            probs.append(p)
        return probs
    return spec, make, refs


def test_gemm_grouped_two_launches_layouts_modes_split_and_not():
    """fp32-operand mmda_gemm_grouped: more problems than one launch holds (GROUP_MAX = 16), nt / nn / tn, both modes, odd sizes,
    split-K and unsplit slots side by side, bias gradient with accumulate, an activation (no split), an empty problem (no slot).
    Every result against a float64 product; the same call twice gives the same bits (the split-K sums have a fixed order)."""
    from mmda_amd import ops
    spec, make, refs = _grouped_problems(dev())
    first = make(); outs = ops.gemm_grouped(first)
    again = make(); outs2 = ops.gemm_grouped(again)
    for (lay, mode, M, N, K, ex), p, p2, out, out2, (ref, bg_ref) in zip(spec, first, again, outs, outs2, refs):
        assert out.shape == (M, N) and torch.equal(out, out2), (lay, mode, M, N, K)
        if M == 0:
            continue
        assert relerr(out, ref) < TOL[mode], (lay, mode, M, N, K)
        if ex.get("bias_grad"):
            assert relerr(p["bias_grad"], bg_ref) < TOL[mode] and torch.equal(p["bias_grad"], p2["bias_grad"])


def test_gemm_batched_strided_and_act_gather():
    from mmda_amd import ops
    torch.manual_seed(2)
    A = torch.randn(3, 20, 16); W = torch.randn(3, 16, 16); b = torch.randn(3, 16)
    ref = torch.sigmoid(torch.einsum("bmk,bnk->bmn", A, W) + b[:, None, :])
    out = ops.gemm(A.to(dev()), W.to(dev()), bias=b.to(dev()), act="sigmoid")
    assert relerr(out, ref) < 1e-5
    # broadcast A over the batch (strideA = 0)
    out = ops.gemm(A[0].to(dev()), W.to(dev()))
    assert relerr(out, torch.einsum("mk,bnk->bmn", A[0], W)) < 1e-5
    # gather rows (embedding lookup fused into the A operand)
    E = torch.randn(50, 16); ids = torch.randint(0, 50, (37,))
    out = ops.gemm(E.to(dev()), W[0].to(dev()), gather=ids.to(dev()))
    assert relerr(out, E[ids] @ W[0].t()) < 1e-5
    # relu/dropout-backward gate
    G = torch.randn(20, 16)
    out = ops.gemm(A[0].to(dev()), W[0].to(dev()), gate=G.to(dev()), gate_scale=2.0)
    assert relerr(out, (A[0] @ W[0].t()) * (G > 0).float() * 2.0) < 1e-5


def test_gemm_sub_matrix_views_for_whh_grad():
    """dW_hh pairs dG[t] with h[t-1] (fwd) / h[t+1] (rev): row- and column-offset views with big leading dims."""
    from mmda_amd import _lib, ops
    import ctypes as C
    torch.manual_seed(3)
    T, B, H = 5, 4, 6
    dG = torch.randn(T, B, 2, 4 * H); hs = torch.randn(T, B, 2 * H)
    ref_f = sum(dG[t, :, 0].t() @ hs[t - 1, :, :H] for t in range(1, T))
    ref_r = sum(dG[t, :, 1].t() @ hs[t + 1, :, H:] for t in range(T - 1))
    dGd, hsd = dG.to(dev()), hs.to(dev())
    lib = _lib.load()
    for ref, a_off, b_off in ((ref_f, B * 8 * H, 0), (ref_r, 4 * H, B * 2 * H + H)):
        out = torch.zeros(4 * H, H, device=dev())
        g = _lib.GemmArgs()
        g.mode = 0; g.transA = 1; g.transB = 0; g.M = 4 * H; g.N = H; g.K = (T - 1) * B; g.batch = 1
        g.A = dGd.data_ptr() + 4 * a_off; g.lda = 8 * H; g.B = hsd.data_ptr() + 4 * b_off; g.ldb = 2 * H
        g.C = out.data_ptr(); g.ldc = H; g.accumulate = 1
        _lib.check(lib.mmda_gemm(C.byref(g), _lib.stream_ptr()))
        assert relerr(out, ref) < 1e-5


def test_colsum_and_embedding():
    from mmda_amd import ops
    torch.manual_seed(4)
    X = torch.randn(1000, 70)
    o1 = torch.zeros(70, device=dev()); o2 = torch.ones(70, device=dev())
    ops.colsum(X.to(dev()), o1, o2)
    assert relerr(o1, X.sum(0)) < 1e-5 and relerr(o2, X.sum(0) + 1) < 1e-5
    W = torch.randn(40, 300); ids = torch.randint(0, 40, (7, 5))
    out = ops.embed_gather(W.to(dev()), ids.to(dev()))
    assert torch.equal(out.cpu(), W[ids])
    dX = torch.randn(7, 5, 300)
    dW = ops.embed_scatter_add(torch.zeros(40, 300, device=dev()), ids.to(dev()), dX.to(dev()))
    ref = torch.zeros(40, 300).index_add_(0, ids.reshape(-1), dX.reshape(-1, 300))
    assert relerr(dW, ref) < 1e-5


# ------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("n,rows", [(600, 130), (70, 33), (148, 64), (128, 192), (16, 5), (150, 33), (300, 64)])
def test_layernorm_fwd_bwd(n, rows):
    from mmda_amd import ops
    torch.manual_seed(5)
    x = torch.randn(rows, n, requires_grad=True); g = torch.randn(n, requires_grad=True); b = torch.randn(n, requires_grad=True)
    y = torch.nn.functional.layer_norm(x, (n,), g, b, 1e-5)
    dy = torch.randn(rows, n)
    y.backward(dy)
    yh, mean, rstd = ops.layernorm_fwd(x.detach().to(dev()), g.detach().to(dev()), b.detach().to(dev()))
    assert relerr(yh, y) < 1e-5
    dx, _, dg, db = ops.layernorm_bwd(dy.to(dev()), x.detach().to(dev()), g.detach().to(dev()), mean, rstd)
    assert relerr(dx, x.grad) < 1e-4 and relerr(dg, g.grad) < 1e-4 and relerr(db, b.grad) < 1e-4


def test_layernorm_act_residual_permute():
    from mmda_amd import ops
    torch.manual_seed(6)
    S, B, n = 6, 5, 128
    x = torch.randn(S * B, n, requires_grad=True); r = torch.randn(S * B, n, requires_grad=True)
    g = torch.randn(n, requires_grad=True); b = torch.randn(n, requires_grad=True)
    y = torch.nn.functional.layer_norm(torch.nn.functional.leaky_relu(x, 0.01) + r, (n,), g, b, 1e-5)
    yp = y.view(S, B, n).permute(1, 0, 2).contiguous()          # (B,S,n) = cat(h[0..5], dim=1)
    dyp = torch.randn(B, S, n)
    yp.backward(dyp)
    d = dev()
    yh, mean, rstd = ops.layernorm_fwd(x.detach().to(d), g.detach().to(d), b.detach().to(d), res=r.detach().to(d), act="leakyrelu",
                                       permute=(S, B))
    assert relerr(yh, yp) < 1e-5
    dx, dres, dg, db = ops.layernorm_bwd(dyp.to(d), x.detach().to(d), g.detach().to(d), mean, rstd, res=r.detach().to(d),
                                         act="leakyrelu", permute=(S, B), want_dres=True)
    assert relerr(dx, x.grad) < 1e-4 and relerr(dres, r.grad) < 1e-4 and relerr(dg, g.grad) < 1e-4 and relerr(db, b.grad) < 1e-4


def test_layernorm_multi_launch_and_split_param_grads():
    """The three inter-layer LayerNorms (rows = T*B, n = 2H = 600/70/148) in one launch each way; input gradients without
    parameter gradients, parameter gradients from the separate column-strip pass."""
    from mmda_amd import ops
    torch.manual_seed(15)
    shapes = [(1600, 600), (1600, 70), (1600, 148), (33, 128), (5, 1024)]
    xs = [torch.randn(r, n, requires_grad=True) for r, n in shapes]
    gs = [torch.randn(n, requires_grad=True) for _, n in shapes]; bs = [torch.randn(n, requires_grad=True) for _, n in shapes]
    dys = [torch.randn(r, n) for r, n in shapes]
    d = dev()
    got = ops.layernorm_multi([x.detach().to(d) for x in xs], [g.detach().to(d) for g in gs], [b.detach().to(d) for b in bs],
                              [t.to(d) for t in dys])
    for x, g, b, dy, (y, dx, dg, db) in zip(xs, gs, bs, dys, got):
        ref = torch.nn.functional.layer_norm(x, x.shape[-1:], g, b, 1e-5)
        ref.backward(dy)
        assert relerr(y, ref) < 1e-5
        assert relerr(dx, x.grad) < 1e-4 and relerr(dg, g.grad) < 1e-4 and relerr(db, b.grad) < 1e-4


# ------------------------------------------------------------------------------------------------ LSTM

def _l2(got, ref):
    got = got.detach().double().cpu(); ref = ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((got - ref).norm() / ref.norm().clamp_min(1e-30))


def _emul_layer(rnn, x, lengths, d_out, d_hn, cell, tile_partials):
    """The same layer on the bf16-emulating oracle (oracle/bf16_emul.py: explicit fp32 loops rounding to bf16 where the kernels
    do): returns (hseq, h_n, dX, {torch parameter name: gradient})."""
    from oracle import bf16_emul as emu
    leaves = {"r." + k: p.detach().clone().requires_grad_(True) for k, p in rnn.named_parameters()}
    xe = x.detach().clone().requires_grad_(True)
    oe, hne = emu.birnn(xe, lengths, leaves, "r", cell, True, tile_partials)
    ((oe * d_out).sum() + (hne * d_hn).sum()).backward()
    return oe.detach(), hne.detach(), xe.grad, {k[2:]: v.grad for k, v in leaves.items()}

def _lstm_case(T, B, H, D, ragged, seed):
    torch.manual_seed(seed)
    rnn = torch.nn.LSTM(D, H, bidirectional=True)
    with torch.no_grad():
        k = 2.0 / math.sqrt(H)            # twice torch's default init range (1/sqrt(H)): harsher than a fresh model
        for p in rnn.parameters():
            p.uniform_(-k, k)
    x = torch.randn(T, B, D, requires_grad=True)
    if ragged:
        lengths = torch.sort(torch.randint(1, T + 1, (B,)), descending=True).values
        lengths[0] = T
    else:
        lengths = torch.full((B,), T)
    return rnn, x, lengths


@pytest.mark.parametrize("mode", ["fp32", "bf16", "bf16-resident", "bf16-resident-gateminor"])
@pytest.mark.parametrize("T,B,H,ragged", [(9, 5, 6, True), (12, 16, 35, True), (7, 20, 74, True), (10, 32, 300, False),
                                          (6, 3, 300, True), (5, 17, 128, True), (8, 70, 300, True),
                                          # sequences shorter than the hand-off's flag-announced prologue (three steps) and just past it
                                          (1, 8, 300, False), (2, 8, 300, True), (3, 8, 74, True), (4, 8, 300, True),
                                          # barrier-synchronised form (H > 320; 21 hidden tiles: the backward's LDS-resident variant)
                                          (4, 8, 336, True),
                                          # a launch chunked over batch groups: barrier form, 11 groups at 10 per launch
                                          (3, 330, 336, True),
                                          # ... and wave form at four waves per block, 13 groups at 12 per launch; gate-minor: the
                                          # dg_bf16_only call pairs, the other does not (tests/test_gpu_lstm_forms.py has more)
                                          (3, 400, 300, True)])
def test_lstm_fwd_bwd_vs_nn_lstm(mode, T, B, H, ragged):
    """Three implementations of the recurrence behind one entry point: exact f32-MFMA streaming kernel, bf16 streaming kernel,
    and the bf16 kernel with W_hh resident in LDS across a cluster of workgroups (per-step h / dG all-gather)."""
    from mmda_amd import ops
    resident = "resident" in mode
    gate_minor = mode.endswith("gateminor")      # `gates` as [dir][unit][gate]: 16-byte stash accesses in the resident kernels
    mode = mode.split("-")[0]
    D = H if H < 100 else 40
    rnn, x, lengths = _lstm_case(T, B, H, D, ragged, 7)
    pk = torch.nn.utils.rnn.pack_padded_sequence(x, lengths, enforce_sorted=False)
    out, (hn, _) = rnn(pk)
    pad, _ = torch.nn.utils.rnn.pad_packed_sequence(out, total_length=T)
    d_out = torch.randn(T, B, 2 * H); d_hn = torch.randn(2, B, H)
    (pad * d_out).sum().add((hn * d_hn).sum()).backward()
    d = dev()
    # time-batched input projection for both directions on the HIP GEMM: (T*B, D) x (8H, D)^T + b_ih + b_hh
    wih = torch.cat((rnn.weight_ih_l0, rnn.weight_ih_l0_reverse), 0).detach()
    bih = torch.cat((rnn.bias_ih_l0, rnn.bias_ih_l0_reverse), 0).detach()
    bhh = torch.cat((rnn.bias_hh_l0, rnn.bias_hh_l0_reverse), 0).detach()
    pre = ops.gemm(x.detach().reshape(T * B, D).to(d), wih.to(d), mode=mode, bias=bih.to(d), bias2=bhh.to(d)).view(T, B, 2, 4 * H)
    fw = ops.lstm_bidir_fwd(pre, rnn.weight_hh_l0.detach().to(d), rnn.weight_hh_l0_reverse.detach().to(d), lengths, mode=mode, layer=1,
                            resident=resident, gate_minor=gate_minor)
    assert not ops.lstm_aborted(fw), "cluster exchange timed out in forward"
    tol = TOL[mode]
    assert relerr(fw["hseq"], pad) < tol
    utt = fw["utt"].cpu().view(B, 4, H)     # [h1_fwd, h2_fwd, h1_bwd, h2_bwd]; layer=1 fills slots 1 and 3
    assert relerr(utt[:, 1], hn[0]) < tol and relerr(utt[:, 3], hn[1]) < tol
    assert float(utt[:, 0].abs().max()) == 0.0 and float(utt[:, 2].abs().max()) == 0.0
    # backward
    d_utt = torch.zeros(B, 4, H); d_utt[:, 1] = d_hn[0]; d_utt[:, 3] = d_hn[1]
    dG = ops.lstm_bidir_bwd(fw, d_utt.view(B, 4 * H).to(d), d_out.to(d), mode=mode, layer=1).view(T * B, 8 * H)
    assert not ops.lstm_aborted(fw), "cluster exchange timed out in backward"
    mask = (torch.arange(T)[:, None] < lengths[None, :]).reshape(T * B)
    assert float(dG.cpu()[~mask].abs().max() if (~mask).any() else 0.0) == 0.0, "dG must be zero at padded positions"
    pair, others = False, []                    # further (dG, hseq, oracle form) to hold to the bounds below
    if "dg_bf16" in fw:
        # the kernel's own bf16 copy of dG (kernel column order [dir][unit][gate]) == the fp32 dG rounded, zeros at padding
        want = ops._to_gate_minor(dG.view(T, B, 2, 4 * H), H).reshape(T * B, 8 * H).to(torch.bfloat16)
        assert torch.equal(fw["dg_bf16"].view(torch.int16), want.view(torch.int16)), "bf16 dG copy differs from round(dG)"
        # production form: only the bf16 copy is written (the fp32 stores are what the kernel's memory pipeline is busy with)
        fw2 = ops.lstm_bidir_fwd(pre, rnn.weight_hh_l0.detach().to(d), rnn.weight_hh_l0_reverse.detach().to(d), lengths, mode=mode,
                                 layer=1, resident=resident, gate_minor=gate_minor)
        ops.lstm_bidir_bwd(fw2, d_utt.view(B, 4 * H).to(d), d_out.to(d), mode=mode, layer=1, dg_bf16_only=True)
        assert not ops.lstm_aborted(fw2)
        # The two calls may run different instances: at four waves per block the dg_bf16_only call takes a PAIR = 1 instance, which
        # adds two fp32 partial-dh tiles before the one bf16 rounding, the other call the run-time instance, which rounds each tile.
        # Both are legitimate roundings (oracle/bf16_emul.py: tile_partials=32 / True).  Same pairing: the same bits.  Otherwise each
        # call is held to its own oracle below.
        shape = dict(H=H, gate_minor=True, d_hseq=True, dg_bf16=True)
        pair, pair2 = (ops.lstm_plan([dict(shape, dg_bf16_only=o)], B, T, backward=True)["pair"] for o in (False, True))
        if pair2 == pair:
            assert torch.equal(fw2["dg_bf16"].view(torch.int16), fw["dg_bf16"].view(torch.int16))
        else:
            dG2 = ops._from_gate_minor(fw2["dg_bf16"].float().view(T, B, 2, 4 * H), H).view(T * B, 8 * H)
            assert float(dG2.cpu()[~mask].abs().max() if (~mask).any() else 0.0) == 0.0, "dg_bf16 must be zero at padded positions"
            assert relerr(fw2["hseq"], pad) < tol
            others.append((dG2, fw2["hseq"], 32 if pair2 else resident))
    btol = tol * (3 if mode == "bf16" else 1)
    emul = {}
    for dG, hseq, tile_partials in [(dG, fw["hseq"], 32 if pair else resident)] + others:
        dx = ops.gemm(dG, wih.to(d), mode=mode, transB=False).view(T, B, D)
        assert relerr(dx, x.grad) < btol
        dwih = ops.gemm(dG, x.detach().reshape(T * B, D).to(d), mode=mode, transA=True, transB=False)
        assert relerr(dwih, torch.cat((rnn.weight_ih_l0.grad, rnn.weight_ih_l0_reverse.grad), 0)) < btol
        db = ops.colsum(dG)
        assert relerr(db, torch.cat((rnn.bias_ih_l0.grad, rnn.bias_ih_l0_reverse.grad), 0)) < btol
        hseq = hseq.view(T * B, 2 * H)
        if T > 1:
            dG3 = dG.view(T, B, 8 * H); hs3 = hseq.view(T, B, 2 * H)
            dwf = ops.gemm(dG3[1:, :, :4 * H].reshape(-1, 4 * H).contiguous(), hs3[:-1, :, :H].reshape(-1, H).contiguous(), mode=mode,
                           transA=True, transB=False)
            dwr = ops.gemm(dG3[:-1, :, 4 * H:].reshape(-1, 4 * H).contiguous(), hs3[1:, :, H:].reshape(-1, H).contiguous(), mode=mode,
                           transA=True, transB=False)
            assert relerr(dwf, rnn.weight_hh_l0.grad) < btol
            assert relerr(dwr, rnn.weight_hh_l0_reverse.grad) < btol
        if mode == "bf16":
            # The bounds above are against exact fp32 nn.LSTM, i.e. they include the quantisation of the operands.  Against the
            # bf16-emulating loops (same rounding points: x, W_ih, W_hh, h, dG and -- resident kernels -- the per-tile partial dh)
            # what is left is summation order and the v_exp/v_rcp activations: hidden states within 1e-3 of the max magnitude,
            # every gradient within 1e-2 relative L2 (north_star's bf16 bound; measured 1e-3 .. 3e-3).
            if tile_partials not in emul:
                emul[tile_partials] = _emul_layer(rnn, x, lengths, d_out, d_hn, "lstm", tile_partials=tile_partials)
            oe, hne, dxe, ge = emul[tile_partials]
            assert relerr(hseq.view(T, B, 2 * H), oe) < 1e-3
            assert relerr(utt[:, 1], hne[0]) < 1e-3 and relerr(utt[:, 3], hne[1]) < 1e-3
            assert _l2(dx, dxe) < 1e-2
            assert _l2(dwih, torch.cat((ge["weight_ih_l0"], ge["weight_ih_l0_reverse"]), 0)) < 1e-2
            assert _l2(db, torch.cat((ge["bias_ih_l0"], ge["bias_ih_l0_reverse"]), 0)) < 1e-2
            if T > 1:
                assert _l2(dwf, ge["weight_hh_l0"]) < 1e-2 and _l2(dwr, ge["weight_hh_l0_reverse"]) < 1e-2

@pytest.mark.parametrize("mode,T,B,H,ragged", [("fp32", 6, 5, 20, True), ("fp32", 9, 33, 74, True), ("bf16", 9, 33, 74, True),
                                               ("fp32", 5, 16, 300, False), ("bf16", 12, 32, 300, True), ("fp32", 1, 3, 35, False),
                                               ("bf16-resident", 12, 32, 300, True), ("bf16-resident-gateminor", 12, 32, 300, True),
                                               ("bf16-resident-gateminor", 9, 40, 74, True), ("bf16-resident", 7, 19, 35, False)])
def test_gru_fwd_bwd_vs_nn_gru(mode, T, B, H, ragged):
    """rnncell='gru' (reference models.py:39): nn.GRU's three gate blocks padded into the four-slot layout the LSTM machinery
    works on (mmda_gru_pad_params), the GRU cell in the streaming recurrent kernels, gradients folded back by
    mmda_gru_unpad_grads.  Checked against nn.GRU on packed sequences + autograd."""
    from mmda_amd import ops
    resident = "resident" in mode                # the wave-autonomous resident-weights kernels (W_hh fragments in registers)
    gate_minor = mode.endswith("gateminor")
    mode = mode.split("-")[0]
    D = H if H < 100 else 40
    torch.manual_seed(11)
    rnn = torch.nn.GRU(D, H, bidirectional=True)
    with torch.no_grad():
        k = 2.0 / math.sqrt(H)
        for p in rnn.parameters():
            p.uniform_(-k, k)
    x = torch.randn(T, B, D, requires_grad=True)
    lengths = torch.full((B,), T)
    if ragged:
        lengths = torch.sort(torch.randint(1, T + 1, (B,)), descending=True).values
        lengths[0] = T
    pk = torch.nn.utils.rnn.pack_padded_sequence(x, lengths, enforce_sorted=False)
    out, hn = rnn(pk)
    pad, _ = torch.nn.utils.rnn.pad_packed_sequence(out, total_length=T)
    d_out = torch.randn(T, B, 2 * H); d_hn = torch.randn(2, B, H)
    (pad * d_out).sum().add((hn * d_hn).sum()).backward()
    d = dev()
    params = dict(rnn.named_parameters())
    P, _ = ops.gru_pad(params, H, D, d)
    # the pad kernel against its definition: W_ih rows [r; z; n; 0], W_hh rows [r; z; 0; n] per direction
    for dr, sfx in enumerate(("", "_reverse")):
        wi, wh = params["weight_ih_l0" + sfx].detach(), params["weight_hh_l0" + sfx].detach()
        bi, bh = params["bias_ih_l0" + sfx].detach(), params["bias_hh_l0" + sfx].detach()
        z2, z1 = torch.zeros(H, D), torch.zeros(H)
        assert torch.equal(P["w_ih"].cpu()[dr * 4 * H:(dr + 1) * 4 * H], torch.cat((wi, z2), 0))
        assert torch.equal(P["w_hh_r" if dr else "w_hh_f"].cpu(), torch.cat((wh[:2 * H], torch.zeros(H, H), wh[2 * H:]), 0))
        assert torch.equal(P["b_ih"].cpu()[dr * 4 * H:(dr + 1) * 4 * H], torch.cat((bi, z1), 0))
        assert torch.equal(P["b_hh"].cpu()[dr * 4 * H:(dr + 1) * 4 * H], torch.cat((bh[:2 * H], z1, bh[2 * H:]), 0))
    xd = x.detach().reshape(T * B, D).to(d)
    pre = ops.gemm(xd, P["w_ih"], mode=mode, bias=P["b_ih"], bias2=P["b_hh"]).view(T, B, 2, 4 * H)
    fw = ops.lstm_bidir_fwd(pre, P["w_hh_f"], P["w_hh_r"], lengths, mode=mode, layer=0, cell="gru", resident=resident,
                            gate_minor=gate_minor)
    assert not ops.lstm_aborted(fw), "cluster exchange timed out in forward"
    if resident:
        from mmda_amd import _lib
        d0 = (_lib.LstmDesc * 1)(ops._desc(H, fw["gates"], fw["cstash"], fw["hseq"], fw["packs"][0], fw["packs"][2], fw["utt"], 0, None,
                                           fw["xchg"], 0))
        d0[0].cell = 1; d0[0].gate_minor = int(gate_minor)
        assert _lib.load().mmda_lstm_resident_applicable(_lib.BF16, 1, d0, B, T, 0) == 1, "expected the resident-weights kernel to run"
    tol = TOL[mode]
    assert relerr(fw["hseq"], pad) < tol
    utt = fw["utt"].cpu().view(B, 4, H)
    assert relerr(utt[:, 0], hn[0]) < tol and relerr(utt[:, 2], hn[1]) < tol
    # backward: four-slot gate gradients -> padded weight gradients -> torch layout
    d_utt = torch.zeros(B, 4, H); d_utt[:, 0] = d_hn[0]; d_utt[:, 2] = d_hn[1]
    dG = ops.lstm_bidir_bwd(fw, d_utt.view(B, 4 * H).to(d), d_out.to(d), mode=mode, layer=0).view(T * B, 8 * H)
    mask = (torch.arange(T)[:, None] < lengths[None, :]).reshape(T * B)
    assert float(dG.cpu()[~mask].abs().max() if (~mask).any() else 0.0) == 0.0, "dG must be zero at padded positions"
    btol = tol * (3 if mode == "bf16" else 1)
    dx = ops.gemm(dG, P["w_ih"], mode=mode, transB=False).view(T, B, D)
    assert relerr(dx, x.grad) < btol
    G = dict(w_ih=ops.gemm(dG, xd, mode=mode, transA=True, transB=False), b_ih=ops.colsum(dG),
             w_hh_f=torch.zeros(4 * H, H, device=d), w_hh_r=torch.zeros(4 * H, H, device=d))
    if T > 1:
        dG3 = dG.view(T, B, 8 * H); hs3 = fw["hseq"].view(T, B, 2 * H)
        G["w_hh_f"] = ops.gemm(dG3[1:, :, :4 * H].reshape(-1, 4 * H).contiguous(), hs3[:-1, :, :H].reshape(-1, H).contiguous(), mode=mode,
                               transA=True, transB=False)
        G["w_hh_r"] = ops.gemm(dG3[:-1, :, 4 * H:].reshape(-1, 4 * H).contiguous(), hs3[1:, :, H:].reshape(-1, H).contiguous(), mode=mode,
                               transA=True, transB=False)
    # accumulate semantics: start the torch-layout gradients at 1 and expect 1 + grad
    grads = {n: torch.ones_like(p, device=d) for n, p in params.items()}
    ops.gru_unpad_grads(grads, G, H, D)
    for n, p in params.items():
        if T == 1 and "weight_hh" in n:
            assert float((grads[n] - 1).abs().max()) == 0.0
            continue
        assert relerr(grads[n] - 1, p.grad) < btol, n
    if mode == "bf16":         # against the bf16-emulating loops: see test_lstm_fwd_bwd_vs_nn_lstm
        oe, hne, dxe, ge = _emul_layer(rnn, x, lengths, d_out, d_hn, "gru", tile_partials=resident)
        assert relerr(fw["hseq"], oe) < 1e-3
        assert relerr(utt[:, 0], hne[0]) < 1e-3 and relerr(utt[:, 2], hne[1]) < 1e-3
        assert _l2(dx, dxe) < 1e-2
        for n, p in params.items():
            if T == 1 and "weight_hh" in n:
                continue
            assert _l2(grads[n] - 1, ge[n]) < 1e-2, n
    for v in G.values():
        assert float(v.abs().max()) == 0.0, "unpad must leave the padded gradients zeroed"


def test_lstm_three_modalities_one_launch_matches_separate():
    """The production launch packs text/visual/acoustic into one grid; results must equal per-modality launches."""
    from mmda_amd import _lib, ops
    import ctypes as C
    d = dev()
    T, B = 8, 19
    torch.manual_seed(8)
    lengths = torch.sort(torch.randint(1, T + 1, (B,)), descending=True).values
    lengths[0] = T
    singles, descs, keep = [], [], []
    for H in (300, 35, 74):
        pre = torch.randn(T, B, 2, 4 * H, device=d)
        wf = (torch.rand(4 * H, H, device=d) - 0.5) * 0.4; wr = (torch.rand(4 * H, H, device=d) - 0.5) * 0.4
        singles.append(ops.lstm_bidir_fwd(pre, wf, wr, lengths, mode="bf16"))
        gates = pre.clone(); cst = torch.zeros(T, B, 2, H, device=d); hseq = torch.zeros(T, B, 2 * H, device=d)
        utt = torch.zeros(B, 4 * H, device=d)
        pf0, _ = ops.lstm_pack(wf, "bf16"); pf1, _ = ops.lstm_pack(wr, "bf16")
        keep.append((gates, cst, hseq, utt, pf0, pf1))
        descs.append(ops._desc(H, gates, cst, hseq, pf0, pf1, utt, 0))
    arr = (_lib.LstmDesc * 3)(*descs)
    len_dev = lengths.to(device=d, dtype=torch.int32)
    _lib.check(_lib.load().mmda_lstm_fwd(_lib.BF16, 3, arr, B, T, len_dev.data_ptr(), _lib.stream_ptr()))
    for s, k in zip(singles, keep):
        # same arithmetic, but the kernel is instantiated for a different tile count per wave, so last-bit differences in
        # the compiler's fma contraction are allowed; an indexing error would be O(1)
        assert relerr(k[2], s["hseq"]) < 1e-5 and relerr(k[3], s["utt"]) < 1e-5 and relerr(k[1], s["cstash"]) < 1e-5


# ------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("E", [128, 16])
def test_attention_fwd_bwd(E):
    from mmda_amd import ops
    torch.manual_seed(9)
    S, B, nh = 6, 7, 2
    hd = E // nh
    qkv = torch.randn(S * B, 3 * E, requires_grad=True)
    q, k, v = qkv.view(S, B, 3 * E).split(E, dim=-1)
    h = lambda z: z.reshape(S, B, nh, hd).permute(1, 2, 0, 3)
    att = torch.softmax(h(q) @ h(k).transpose(-1, -2) / math.sqrt(hd), -1)
    ctx = (att @ h(v)).permute(2, 0, 1, 3).reshape(S * B, E)
    dctx = torch.randn(S * B, E)
    ctx.backward(dctx)
    d = dev()
    c, p = ops.attn_fwd(qkv.detach().to(d), S, B, E, nh)
    assert relerr(c, ctx) < 1e-5 and relerr(p, att) < 1e-5
    dq = ops.attn_bwd(qkv.detach().to(d), p, dctx.to(d), S, B, E, nh)
    assert relerr(dq, qkv.grad) < 1e-4


# ------------------------------------------------------------------------------------------------ losses
def _side(B, D, seed):
    torch.manual_seed(seed)
    return [torch.sigmoid(torch.randn(B, D)).requires_grad_(True) for _ in range(6)]


@pytest.mark.parametrize("B,D", [(32, 128), (5, 16), (70, 128), (41, 100), (64, 128), (130, 128), (256, 128), (300, 128), (5, 160)])
def test_diff_cmd_recon_losses_and_grads(B, D):
    from types import SimpleNamespace
    from mmda_amd.utils import functions as F
    ts = _side(B, D, 10)
    o = SimpleNamespace(utt_private_t=ts[0], utt_private_v=ts[1], utt_private_a=ts[2], utt_shared_t=ts[3], utt_shared_v=ts[4],
                        utt_shared_a=ts[5])
    d = dev()
    # diff
    ref = orc.diff_loss(o); ref.backward()
    gts = [t.detach().to(d).requires_grad_(True) for t in ts]
    got = F.diff_loss_multi(gts, [(0, 3), (1, 4), (2, 5), (2, 0), (2, 1), (0, 1)]); got.backward()
    assert abs(got.item() - ref.item()) < 1e-4 * abs(ref.item()) + 1e-8
    for g, t in zip(gts, ts):
        assert relerr(g.grad, t.grad) < 2e-4
    # single-pair module form
    a, b = ts[0].detach(), ts[3].detach()
    assert abs(F.DiffLoss()(a.to(d), b.to(d)).item() - orc.diff_pair(a, b).item()) < 1e-4 * orc.diff_pair(a, b).item() + 1e-8
    # cmd
    for t in ts:
        t.grad = None
    ref = orc.cmd_loss(o); ref.backward()
    gts = [t.detach().to(d).requires_grad_(True) for t in ts[3:]]
    got = F.cmd_loss_multi(gts, [(0, 1), (0, 2), (2, 1)], 5, 1.0 / 3.0); got.backward()
    assert abs(got.item() - ref.item()) < 1e-4 * abs(ref.item())
    for g, t in zip(gts, ts[3:]):
        assert relerr(g.grad, t.grad) < 2e-4
    assert abs(F.CMD()(a.to(d), b.to(d), 5).item() - orc.cmd_pair(a, b).item()) < 1e-4 * orc.cmd_pair(a, b).item()
    # recon
    rec = [torch.randn(B, D, requires_grad=True) for _ in range(3)]
    org = [torch.randn(B, D, requires_grad=True) for _ in range(3)]
    oo = SimpleNamespace(utt_t_recon=rec[0], utt_v_recon=rec[1], utt_a_recon=rec[2], utt_t_orig=org[0], utt_v_orig=org[1], utt_a_orig=org[2])
    ref = orc.recon_loss(oo); ref.backward()
    grec = [t.detach().to(d).requires_grad_(True) for t in rec]; gorg = [t.detach().to(d).requires_grad_(True) for t in org]
    got = F.recon_loss(grec, gorg); got.backward()
    assert abs(got.item() - ref.item()) < 1e-5 * abs(ref.item())
    for g, t in zip(grec + gorg, rec + org):
        assert relerr(g.grad, t.grad) < 1e-5


@pytest.mark.parametrize("B", [32, 5, 300])
def test_cls_conf_domain_losses_and_grads(B):
    from types import SimpleNamespace
    from mmda_amd.utils import functions as F
    torch.manual_seed(11)
    s = torch.sigmoid(torch.randn(B, 6)).requires_grad_(True)
    t = torch.sigmoid(torch.randn(B, 6)).requires_grad_(True)
    y = (torch.rand(B, 6) > 0.6).float(); y[0] = 1.0
    d = dev()
    ref = orc.cls_loss(s, y); ref.backward()
    gs = s.detach().to(d).requires_grad_(True)
    got = F.bce_sum_over_classes(gs, y.to(d)); got.backward()
    assert abs(got.item() - ref.item()) < 1e-5 * abs(ref.item()) and relerr(gs.grad, s.grad) < 1e-5
    s.grad = None
    ref = orc.conf_loss(s, t, y); ref.backward()
    gs = s.detach().to(d).requires_grad_(True); gt = t.detach().to(d).requires_grad_(True)
    got = F.conf_loss(gs, gt, y.to(d)); got.backward()
    assert abs(got.item() - ref.item()) < 1e-5 * abs(ref.item())
    assert relerr(gs.grad, s.grad) < 1e-4 and relerr(gt.grad, t.grad) < 1e-4
    dom = [torch.randn(B, 3, requires_grad=True) for _ in range(3)]
    ref = orc.domain_loss(SimpleNamespace(domain_label_t=dom[0], domain_label_v=dom[1], domain_label_a=dom[2])); ref.backward()
    gd = [x.detach().to(d).requires_grad_(True) for x in dom]
    got = F.domain_loss(*gd); got.backward()
    assert abs(got.item() - ref.item()) < 1e-5 * abs(ref.item())
    for g, x in zip(gd, dom):
        assert relerr(g.grad, x.grad) < 1e-5


def test_bce_clamp_at_saturated_scores():
    """BCELoss clamps log at -100 and its backward divides by max(s(1-s), 1e-12): scores of exactly 0/1 stay finite."""
    from mmda_amd.utils import functions as F
    s = torch.tensor([[0.0, 1.0, 0.5, 1.0, 0.0, 0.25]]); y = torch.tensor([[1.0, 0.0, 1.0, 1.0, 0.0, 0.0]])
    ref = torch.nn.BCELoss()(s[0], y[0]) * 6
    got = F.bce_sum_over_classes(s.to(dev()), y.to(dev()))
    assert abs(got.item() - ref.item()) < 1e-4 * ref.item()


# ------------------------------------------------------------------------------------------------ optimizer, dropout
def test_clamp_adam_rows_in_two_passes_equals_the_dense_update():
    """Untouched rows first (zero gradient), touched rows after the scatter: bit-identical to one dense clip + Adam pass."""
    from mmda_amd import ops
    torch.manual_seed(3)
    V, D = 997, 300
    ids = torch.randint(0, V, (160,))
    ids[0] = V - 1
    p = torch.randn(V, D); m = torch.randn(V, D) * 1e-2; v = torch.rand(V, D) * 1e-3
    g = torch.zeros(V, D); g.index_add_(0, ids, torch.randn(160, D) * 3.0)
    ref = [t.clone().to(dev()) for t in (p, m, v)]
    ops.clamp_adam(ref[0].view(-1), g.to(dev()).view(-1), ref[1].view(-1), ref[2].view(-1), 1e-3, 4, clip=1.0)
    got = [t.clone().to(dev()) for t in (p, m, v)]
    mask = ops.mark_rows(ids.to(dev()), V)
    assert int(mask.sum()) == len(set(ids.tolist())) and set(mask.nonzero().flatten().tolist()) == set(ids.tolist())
    gz = torch.zeros(V, D, device=dev())                 # what the gradient bucket holds before the scatter
    ops.clamp_adam_rows(got[0], gz, got[1], got[2], mask, 0, 1e-3, 4, clip=1.0)
    ops.clamp_adam_rows(got[0], g.to(dev()), got[1], got[2], mask, 1, 1e-3, 4, clip=1.0)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)


def test_clamp_adam_matches_torch_adam_three_steps():
    from mmda_amd import ops
    torch.manual_seed(12)
    n = 10007
    p0 = torch.randn(n); ref = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=1e-3)
    p = p0.clone().to(dev()); m = torch.zeros(n, device=dev()); v = torch.zeros(n, device=dev())
    for step in range(1, 4):
        g = torch.randn(n) * 3
        ref.grad = g.clone()
        torch.nn.utils.clip_grad_value_([ref], 1.0)
        opt.step()
        ops.clamp_adam(p, g.to(dev()), m, v, 1e-3, step, clip=1.0)
    assert float((p.cpu() - ref.detach()).abs().max()) < 2e-6


def test_dropout_rng_statistics_and_replay():
    from mmda_amd import ops
    n, p = 1_000_000, 0.1
    h = ops.dropout_mask_via_act(n, p, seed=123, site=3, device=dev())
    keep = (h > 0).float().mean().item()
    assert abs(keep - (1 - p)) < 2e-3                                  # keep-rate
    assert abs(h.mean().item() - 1.0) < 5e-3                           # inverted scaling 1/(1-p)
    u = torch.unique(h).cpu().tolist()
    assert len(u) == 2 and u[0] == 0.0 and abs(u[1] - 1 / (1 - p)) < 1e-5
    h2 = ops.dropout_mask_via_act(n, p, seed=123, site=3, device=dev())
    assert torch.equal(h, h2)                                          # same (seed, site, index) -> same mask (fwd/bwd replay)
    h3 = ops.dropout_mask_via_act(n, p, seed=124, site=3, device=dev())
    assert (h != h3).float().mean().item() > 0.1                       # a new seed decorrelates
    # adjacent elements are uncorrelated
    k = (h > 0).float()
    c = ((k[1:] - k.mean()) * (k[:-1] - k.mean())).mean().item()
    assert abs(c) < 1e-3


# ------------------------------------------------------------------------------------------------ evaluation metrics on the device
def test_device_eval_counts_match_reference_golden():
    """mmda_eval_accumulate over the batches of an evaluation pass -> accuracy and the nine P/R/F1 figures of the reference's
    get_metrics (golden vectors from src/utils/eval.py), exact counts, one read-back."""
    import os
    from mmda_amd.utils.eval import DeviceEval, KEYS
    from oracle import eval_oracle as ev
    G = np.load(os.path.join(os.path.dirname(__file__), "golden", "eval_metrics.npz"))
    for c in sorted({k.split("/")[0] for k in G.files if "/" in k}):
        y = torch.from_numpy(G[c + "/y"]).to(dev()); p = torch.from_numpy(G[c + "/pred"]).to(dev())
        acc = DeviceEval(y.shape[1], dev())
        for s in range(0, y.shape[0], 50):                      # ragged last batch
            acc.update(p[s:s + 50], y[s:s + 50])
        _, a, m = acc.result()
        for k, r in zip(KEYS, G[c + "/metrics"]):
            assert abs(m[k] - r) < 1e-12, (c, k, m[k], r)
        assert a == G[c + "/metrics"][0] == ev.get_accuracy(G[c + "/y"], G[c + "/pred"])
    # full-size property check: 2**18 samples, counts are exact integers and add up
    torch.manual_seed(0)
    N = 1 << 18
    y = (torch.rand(N, 6, device=dev()) > 0.7).float(); p = (torch.rand(N, 6, device=dev()) > 0.6).float()
    acc = DeviceEval(6, dev()); acc.update(p, y)
    st = acc.state.cpu().numpy()
    tp, fp, fn = st[:6], st[6:12], st[12:18]
    assert np.array_equal(tp, ((y > 0) & (p > 0)).sum(0).cpu().numpy().astype(np.float64))
    assert np.array_equal(tp + fn, (y > 0).sum(0).cpu().numpy().astype(np.float64))
    assert np.array_equal(tp + fp, (p > 0).sum(0).cpu().numpy().astype(np.float64)) and st[19] == N


def test_transpose_f32_multi():
    from mmda_amd import ops
    torch.manual_seed(2)
    mats = [torch.randn(12, 768), torch.randn(2048, 128), torch.randn(128, 2048), torch.randn(33, 70), torch.randn(3, 128), torch.randn(1, 1)]
    outs = ops.transpose_f32([m.to(dev()) for m in mats])
    for m, o in zip(mats, outs):
        assert torch.equal(o.cpu(), m.t().contiguous())


def test_gemm_bf16_tall_class_in_a_fresh_process():
    """The 256 x 128 tile class of the LDS-DMA GEMM (K >= 1024, M >= 512 in a call of >= 8192 rows) is off by default since the end of
    round 3 (MMDA_GEMM_DMA_TALL=1 switches it on; read once per process, hence the subprocess): nt input-gradient shapes and a tn
    weight-gradient shape with bias gradient and accumulation through it."""
    import subprocess, sys
    code = r'''
import math, sys, torch
sys.path.insert(0, %r)
from mmda_amd import ops
d = torch.device("cuda:0")
rel = lambda a, b: float((a.cpu() - b).abs().max() / b.abs().max())
torch.manual_seed(4)
for M, N, K in [(8200, 600, 1100), (8200, 300, 2400)]:
    A = torch.randn(M, K); W = torch.randn(N, K) / math.sqrt(K); b = torch.randn(N)
    (Ap, _), (Wp, _) = ops.convert_bf16([(A.to(d), None, True, False), (W.to(d), None, True, False)])
    ref = A.bfloat16().float() @ W.bfloat16().float().t() + b
    out, = ops.gemm_bf16_grouped([dict(A=Ap, B=Wp, K=K, bias=b.to(d))])
    assert rel(out, ref) < 1e-4, (M, N, K, rel(out, ref))
# tn: C (M, N) += A^T B over K = 8320 rows, M = 2400 >= 512
K, M, N = 8320, 2400, 304
A = (torch.randn(K, M) / math.sqrt(K)).bfloat16(); Bm = torch.randn(K, N).bfloat16(); C0 = torch.randn(M, N)
bg = torch.zeros(M)
out, = ops.gemm_bf16_grouped([dict(A=A.to(d), B=Bm.to(d), M=M, N=N, K=K, tn=True, out=C0.clone().to(d), accumulate=True, bias_grad=bg.to(d))])
ref = C0 + A.float().t() @ Bm.float()
assert rel(out, ref) < 1e-4, rel(out, ref)
print("ok")
''' % ROOT
    env = dict(os.environ, MMDA_GEMM_DMA_TALL="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("switches", [{"MMDA_XCD_LOCAL": "0"}, {"MMDA_XCD_LOCAL": "3"}, {"MMDA_LSTM_NO_QUAD": "1"},
                                      {"MMDA_LSTM_NO_QUAD": "1", "MMDA_XCD_LOCAL": "3"}],
                         ids=["write_through", "placement_check_fails", "one_wave_per_tile", "one_wave_per_tile_check_fails"])
def test_recurrence_hand_off_fallbacks_in_a_fresh_process(switches):
    """The XCD-local hand-off is taken only after the waves have verified that their cluster shares an XCD.  MMDA_XCD_LOCAL=0 never
    tries (write-through form throughout); =3 is a test hook that makes the odd hidden tiles announce a wrong XCC id, so every
    cluster's check fails at step 1 and the kernels must carry on in the write-through form.  MMDA_LSTM_NO_QUAD=1 selects the
    one-wave-per-tile kernels (what batches beyond 128 run) at this small batch.  All must reproduce nn.LSTM.
    (The switches are read once per process, hence the subprocess.)"""
    import subprocess, sys
    code = r'''
import math, sys, torch
sys.path.insert(0, %r)
from mmda_amd import ops
torch.manual_seed(5)
T, B, H, D = 12, 32, 300, 40
rnn = torch.nn.LSTM(D, H, bidirectional=True)
x = torch.randn(T, B, D, requires_grad=True)
lengths = torch.sort(torch.randint(1, T + 1, (B,)), descending=True).values; lengths[0] = T
pk = torch.nn.utils.rnn.pack_padded_sequence(x, lengths, enforce_sorted=False)
out, (hn, _) = rnn(pk)
pad, _ = torch.nn.utils.rnn.pad_packed_sequence(out, total_length=T)
d_out = torch.randn(T, B, 2 * H); d_hn = torch.randn(2, B, H)
(pad * d_out).sum().add((hn * d_hn).sum()).backward()
d = torch.device("cuda:0")
wih = torch.cat((rnn.weight_ih_l0, rnn.weight_ih_l0_reverse), 0).detach().to(d)
b1 = torch.cat((rnn.bias_ih_l0, rnn.bias_ih_l0_reverse), 0).detach().to(d); b2 = torch.cat((rnn.bias_hh_l0, rnn.bias_hh_l0_reverse), 0).detach().to(d)
pre = ops.gemm(x.detach().reshape(T * B, D).to(d), wih, mode="bf16", bias=b1, bias2=b2).view(T, B, 2, 4 * H)
fw = ops.lstm_bidir_fwd(pre, rnn.weight_hh_l0.detach().to(d), rnn.weight_hh_l0_reverse.detach().to(d), lengths, mode="bf16", layer=1,
                        resident=True, gate_minor=True)
assert not ops.lstm_aborted(fw)
rel = lambda a, b: float((a.cpu() - b).abs().max() / b.abs().max())
assert rel(fw["hseq"], pad.detach()) < 1e-2, rel(fw["hseq"], pad.detach())
d_utt = torch.zeros(B, 4, H); d_utt[:, 1] = d_hn[0]; d_utt[:, 3] = d_hn[1]
dG = ops.lstm_bidir_bwd(fw, d_utt.view(B, 4 * H).to(d), d_out.to(d), mode="bf16", layer=1).view(T * B, 8 * H)
assert not ops.lstm_aborted(fw)
dx = ops.gemm(dG, wih, mode="bf16", transB=False).view(T, B, D)
assert rel(dx, x.grad) < 3e-2, rel(dx, x.grad)
print("ok")
''' % ROOT
    env = dict(os.environ, **switches)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]


# ------------------------------------------------------------------------------------------------ data-parallel pieces
def _segment_sum_reference(ids, rows, V):
    """The documented order in numpy fp32: stable sort by id; runs = segments cut at multiples of 64 sorted positions; a run is summed
    sequentially, then a segment's runs sequentially."""
    ids = ids.numpy(); rows = rows.numpy()
    order = np.argsort(np.where(ids < 0, 1 << 40, ids), kind="stable")
    sid = ids[order]
    out = {}
    p = 0
    n = len(sid)
    while p < n and sid[p] >= 0:
        e = p
        while e < n and sid[e] == sid[p]:
            e += 1
        acc = np.zeros(rows.shape[1], np.float32)
        q = p
        while q < e:
            lim = min(e, (q // 64 + 1) * 64)
            part = np.zeros(rows.shape[1], np.float32)
            for r in range(q, lim):
                part = (part + rows[order[r]]).astype(np.float32)
            acc = (acc + part).astype(np.float32)
            q = lim
        out[int(sid[p])] = acc
        p = e
    return out


@pytest.mark.parametrize("n,V,D", [(1600, 500, 300), (4000, 37, 300), (300, 64, 12), (5, 3, 7)])
def test_embed_segment_sum_is_exact_and_deterministic(n, V, D):
    """mmda_embed_segment_sum: the dense rows equal the list-order sums BIT FOR BIT (fixed two-level order, no atomics), untouched rows
    stay as they were, ids < 0 are skipped, and a second run gives identical bits (what keeps data-parallel replicas identical)."""
    from mmda_amd import ops
    torch.manual_seed(n + D)
    ids = torch.randint(0, V, (n,))
    if n >= 1000:
        ids[torch.randperm(n)[: n // 3]] = 1           # one long segment (a frequent word)
        ids[torch.randperm(n)[: n // 10]] = -1         # padded positions
    rows = torch.randn(n, D)
    base = torch.randn(V, D)
    ref = _segment_sum_reference(ids, rows, V)
    outs = []
    for _ in range(2):
        dW = base.clone().to(dev())
        ops.embed_segment_sum(dW, ids.to(dev()), rows.to(dev()))
        outs.append(dW.cpu())
    assert torch.equal(outs[0], outs[1])
    for v in range(V):
        if v in ref:
            assert np.array_equal(outs[0][v].numpy(), ref[v]), v
        else:
            assert torch.equal(outs[0][v], base[v]), v


def test_allreduce_entry_on_a_single_rank_rccl_communicator():
    """mmda_allreduce (the C-ABI data-parallel exchange for hosts that own an RCCL communicator): exercised with a one-rank
    communicator created through the same librccl the entry resolves ncclAllReduce from; a sum over one rank leaves the buffer as it
    is, and the call has to go through RCCL's stream-ordered path to say so."""
    import ctypes as C
    from mmda_amd import _lib
    lib = _lib.load()
    rccl = None
    for name in ("librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"):
        try:
            rccl = C.CDLL(name, mode=C.RTLD_GLOBAL)
            break
        except OSError:
            continue
    if rccl is None:
        pytest.skip("librccl.so not found on this box")

    class UniqueId(C.Structure):
        _fields_ = [("internal", C.c_char * 128)]
    uid = UniqueId()
    assert rccl.ncclGetUniqueId(C.byref(uid)) == 0
    comm = C.c_void_p()
    rccl.ncclCommInitRank.argtypes = [C.POINTER(C.c_void_p), C.c_int, UniqueId, C.c_int]
    assert rccl.ncclCommInitRank(C.byref(comm), 1, uid, 0) == 0
    try:
        x = torch.randn(100003, device=dev())
        want = x.clone()
        _lib.check(lib.mmda_allreduce(x.data_ptr(), x.numel(), comm, _lib.stream_ptr()), "mmda_allreduce")
        torch.cuda.synchronize()
        assert torch.equal(x, want)
        assert lib.mmda_allreduce(None, 4, comm, None) == -1 and lib.mmda_allreduce(x.data_ptr(), 4, None, None) == -1
    finally:
        rccl.ncclCommDestroy.argtypes = [C.c_void_p]
        rccl.ncclCommDestroy(comm)


# ------------------------------------------------------------------------------------------------ block-scaled fp8 GEMM (configs[4])
@pytest.mark.parametrize("M,N,K,scale", [(192, 2048, 128, 1.0), (192, 128, 2048, 1.0), (37, 48, 256, 1e-3), (16, 16, 128, 300.0),
                                         (1536, 128, 2048, 1.0)])
def test_gemm_mx8_equals_the_product_of_the_quantised_operands(M, N, K, scale):
    """mmda_gemm_mx8 = exact product (fp32 accumulate) of the OCP-MX e4m3 images of A and B.  The reference computes the image the
    documented way (oracle/fp8_emul.py: shared exponent floor(log2 amax) - 8 per 32 consecutive k, clamp +-448, round to nearest even
    onto torch.float8_e4m3fn's grid); agreement to fp32 summation order means the quantiser, the operand packing of
    v_mfma_scale_f32_16x16x128_f8f6f4 and its scale bytes are all what the header says.  Plus bias / relu epilogue."""
    from mmda_amd import ops
    from oracle import fp8_emul as f8
    torch.manual_seed(M + N + K)
    A = torch.randn(M, K) * scale
    A[:, :32] *= 40.0                                   # blocks of very different magnitude in one row
    A[0, 64:96] = 0.0                                   # an all-zero block
    Bm = torch.randn(N, K) / math.sqrt(K)
    b = torch.randn(N)
    ref = f8.mx_quant(A).double() @ f8.mx_quant(Bm).double().t()
    # (2e-4 of the largest output, not 1e-5: the matrix core aligns the 128 products of a step to a common exponent before it adds
    # them, so with blocks of very different magnitude in one dot product the sum is not the sequential fp32 one; measured 6e-5)
    out = ops.gemm_mx8(A.to(dev()), Bm.to(dev()))
    assert relerr(out, ref.float()) < 2e-4
    out2 = ops.gemm_mx8(A.to(dev()), Bm.to(dev()), bias=b.to(dev()), act="relu")
    assert relerr(out2, torch.relu(ref.float() + b)) < 2e-4
    # and the quantisation itself is what fp8 promises: a few percent per element, well under it per dot product
    exact = A.double() @ Bm.double().t()
    assert float((ref - exact).norm() / exact.norm()) < 6e-2
