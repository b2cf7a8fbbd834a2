"""The edge cases of the bf16 grouped GEMM (mmda_amd/csrc/gemm_bf16.hip, splitk.hip), defined once for the CPU test that proves what
each case reaches (test_gemm_bf16_plan_cpu.py) and the GPU test that checks its numbers (test_gpu_gemm_bf16_edges.py).

A case is one call: a switch set, its problems, and per problem the kernel instance and the k-slices it is meant to get.  The
instances: reg64 / reg128 = gemm_bf16_kernel<T, false>, *_mixed = <T, true>, dmaS_T = gemm_bf16_dma_kernel<S, T>.  A slice length L
counts k-tiles of 64.  Also here: the operand / output buffers of a problem (what surrounds the operands and the output window is part
of the test) and its float64 reference, both plain torch on the CPU.
"""
import zlib

import torch

DEFAULT, STAGES3, TALL = (1, 2, 8192, 0), (1, 3, 8192, 0), (1, 2, 8192, 1)      # (dma_on, dma_stages, dma_min_rows, dma_tall)
ENV = {DEFAULT: {}, STAGES3: {"MMDA_GEMM_DMA_STAGES": "3"}, TALL: {"MMDA_GEMM_DMA_TALL": "1"}}
SWITCH_NAME = {DEFAULT: "default", STAGES3: "stages3", TALL: "tall"}
NS = {"reg64": 4, "reg64_mixed": 4, "reg128": 2, "reg128_mixed": 2, "dma2_128": 2, "dma3_128": 3, "dma3_256": 3}   # prefetch ring depth
# unsplit slice lengths every instance must be run at, with the last k-tile full / ragged: 1 .. 2 NS + 1.  The 256-row class needs
# K >= 1024: 16 k-tiles and up, and 16 k-tiles only with the last one full; one length per residue mod NS either way
REQUIRED_L = {i: {"full": range(1, 2 * ns + 2), "ragged": range(1, 2 * ns + 2)} for i, ns in NS.items()}
REQUIRED_L["dma3_256"] = {"full": range(16, 19), "ragged": range(17, 20)}
FEATURES = ("plain", "alpha_acc", "bias2", "bgrad", "perm_n", "perm_m")
EPILOGUES = ("epi64", "epi128_reg", "epi128_dma", "epi256_dma", "reduce")
H = 35                                              # the gate interleave's unit count: 4H = 140 is off every tile grid


def instance_of(row, switches):
    """The kernel instance pick_kernel() names for a plan row"""
    if row["cls"] == "Dma256":
        return "dma3_256"
    if row["cls"] == "Dma128":
        return "dma%d_128" % (3 if switches[1] == 3 else 2)
    return row["cls"].lower() + ("_mixed" if row["mixed"] else "")


def P(form, M, N, K, inst, sk=1, per=None, last=None, **kw):
    nk = (K + 63) // 64
    per = nk if per is None else per
    return dict(form=form, M=M, N=N, K=K, expect=dict(inst=inst, sk=sk, per=per, last=per if last is None else last), **kw)


def carrier():
    """A trivial problem of 8192 rows: its call is a large-batch call, whose problems may take the LDS-DMA classes"""
    return P("nt", 8192, 8, 8, "reg64")


def _feat(name):
    return {"plain": {}, "alpha_acc": dict(alpha=-0.5, accumulate=True), "bias2": dict(bias=True, bias2=True),
            "bgrad": dict(bias_grad=True, bias_grad2=True, accumulate=True), "perm_n": dict(perm_n_H=H, bias=True, bias2=True),
            "perm_m": dict(perm_m_H=H, bias_grad=True, accumulate=True)}[name]


# output shapes (M, N) per class: one more / one less than a tile on either side, N % 4 != 0 (no 16-byte row store) and N % 4 == 0
SHAPES = {"Reg64": [(65, 63), (63, 68), (129, 65), (64, 124)],
          "Reg128": [(2945, 2815), (2943, 2817), (2900, 2892)],            # >= 512 tiles of 128 x 128
          "Dma128": [(129, 127), (127, 132), (257, 129), (128, 252)],       # >= 96 rows and columns
          # unsplit at 16 k-tiles only where the launch has > 2560 k-tiles of work (split_dma): >= 176 tiles of 256 x 128
          "Dma256": [(2561, 2047), (2815, 2049)]}
INSTANCES = {  # instance -> (class, form that reaches it alone, switches)
    "reg64": ("Reg64", "nt", DEFAULT), "reg64_mixed": ("Reg64", "tn", DEFAULT), "reg128": ("Reg128", "nt", DEFAULT),
    "reg128_mixed": ("Reg128", "tn", DEFAULT), "dma2_128": ("Dma128", None, DEFAULT), "dma3_128": ("Dma128", None, STAGES3),
    "dma3_256": ("Dma256", None, TALL)}


def _window(cls, form, i):
    """tn column windows: every other case off zero -- off the 16-byte grid for the register-staged classes (the reverse direction's
    half of dG for a 35-wide LSTM), on it for the DMA classes (which need it)"""
    if form != "tn" or i % 2 == 0:
        return {}
    return dict(a0=140, b0=40, ld_pad=4) if cls.startswith("Reg") else dict(a0=136, b0=40)


def _cases():
    out = []

    def add(name, switches, problems, epi=None):
        if any(p["expect"]["inst"].startswith("dma") for p in problems):
            problems = problems + [carrier()]
        out.append(dict(name=name, switches=switches, problems=problems, epi=epi))

    for inst, (cls, only_form, sw) in INSTANCES.items():
        forms = (only_form,) if only_form else ("nt", "tn")
        shapes = SHAPES[cls]
        # ---- unsplit slice lengths, last k-tile full and ragged
        for form in forms:
            tails = (("full", 64), ("ragged", 35)) if form == "nt" else (("full", 64), ("k1", 1), ("k63", 63))
            i = 0
            for L in sorted(set(REQUIRED_L[inst]["full"]) | set(REQUIRED_L[inst]["ragged"])):
                for tname, t in tails:
                    if L not in REQUIRED_L[inst]["full" if tname == "full" else "ragged"]:
                        continue
                    M, N = shapes[i % len(shapes)]
                    kw = dict(_window(cls, form, i), poison=tname != "full" or (form == "tn" and i % 2 == 1))
                    if i % 3 == 1:
                        kw["bias_grad"] = True
                    add(f"{inst}-{form}-L{L}-{tname}", sw, [P(form, M, N, 64 * (L - 1) + t, inst, **kw)])
                    i += 1
        # ---- the bias gradient's ones-column alone in a column tile of its own / in the last column of a tile
        big = {"Reg128": [(2945, 2816), (2945, 2815)], "Dma256": [(2561, 2048), (2815, 2047)]}
        tm, tn_ = (256, 128) if cls == "Dma256" else ((64, 64) if cls == "Reg64" else (128, 128))
        for form in forms:
            for k, (M, N) in enumerate(big.get(cls, [(tm + 1, 2 * tn_), (2 * tm - 1, 2 * tn_ - 1)])):
                K = (1024 if cls == "Dma256" else 64) + (35 if form == "nt" else 63)
                add(f"{inst}-{form}-ones-column-N{N}", sw, [P(form, M, N, K, inst, bias_grad=True, bias_grad2=bool(k), poison=True,
                                                             **_window(cls, form, k))])
    # ---- split problems: slices in every residue mod NS, the last one shorter
    # register-staged, one 64 x 64 tile walking >= 128 k-tiles: 8 slices of 17, the last 10 .. 13
    for form, inst in (("nt", "reg64"), ("tn", "reg64_mixed")):
        for K, last in ((8200, 10), (8320, 11), (8330, 12), (8448, 13)):
            add(f"{inst}-{form}-split-sk8-per17-last{last}", DEFAULT,
                [P(form, 63, 61, K, inst, sk=8, per=17, last=last, bias_grad=last % 2 == 0, accumulate=last > 11, poison=True)])
    # DMA classes: from 12 k-tiles with accumulate
    for inst, (cls, _, sw) in INSTANCES.items():
        if not inst.startswith("dma"):
            continue
        plans = ((17, 2, 9, 8), (19, 2, 10, 9), (20, 3, 7, 6)) if cls == "Dma256" else ((13, 2, 7, 6), (15, 2, 8, 7), (20, 3, 7, 6))
        shapes = [(513, 127), (767, 132), (600, 129)] if cls == "Dma256" else SHAPES[cls]
        for form in ("nt", "tn"):
            for k, (nk, sk, per, last) in enumerate(plans):
                M, N = shapes[k]
                K = 64 * (nk - 1) + ((35, 64, 8)[k] if form == "nt" else (1, 64, 63)[k])
                add(f"{inst}-{form}-split-sk{sk}-per{per}-last{last}", sw,
                    [P(form, M, N, K, inst, sk=sk, per=per, last=last, accumulate=True, bias_grad=k != 1, poison=True,
                       **_window(cls, form, k))])
    # ---- grouping: an nt problem on the mixed instance because its launch also holds a tn problem
    add("reg64_mixed-group-nt-beside-tn", DEFAULT, [P("nt", 65, 63, 99, "reg64_mixed", bias=True, poison=True),
                                                    P("tn", 63, 68, 65, "reg64_mixed", bias_grad=True, a0=140, b0=40, ld_pad=4, poison=True)])
    add("reg128_mixed-group-nt-beside-tn", DEFAULT, [P("nt", 2900, 2890, 99, "reg128_mixed", bias=True, poison=True),
                                                     P("tn", 2900, 2892, 65, "reg128_mixed", bias_grad=True, poison=True)])
    # ---- epilogue matrix: every feature set through every implementation of the epilogue
    epi_shapes = {  # implementation -> (instance, switches, K, (M, N) of the plain / perm_n / perm_m forms)
        "epi64": ("reg64", DEFAULT, 99, (129, 68), (96, 8 * H), (8 * H, 40)),
        "epi128_reg": ("reg128", DEFAULT, 99, (2900, 2892), (2945, 80 * H), (80 * H, 2948)),
        "epi128_dma": ("dma2_128", DEFAULT, 99, (129, 132), (129, 8 * H), (8 * H, 100)),
        "epi256_dma": ("dma3_256", TALL, 1059, (2561, 2052), (2561, 60 * H), (80 * H, 2052)),
        "reduce": ("dma2_128", DEFAULT, 1251, (129, 132), (129, 8 * H), (8 * H, 100))}
    for impl, (inst, sw, K, s_plain, s_pn, s_pm) in epi_shapes.items():
        for odd in (False, True):                         # odd: a leading dimension of C that forbids 16-byte stores
            if odd and impl == "epi128_reg":
                continue
            for f in FEATURES:
                M, N = s_pn if f == "perm_n" else s_pm if f == "perm_m" else s_plain
                split = dict(sk=3, per=7, last=6) if impl == "reduce" else {}
                kw = dict(_feat(f), **split)
                if odd:
                    kw["ldc_pad"] = 5
                add(f"epilogue-{impl}-{f}" + ("-odd-ldc" if odd else ""), sw, [P("nt", M, N, K, inst, **kw)], epi=(f, impl))
    return out


CASES = _cases()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def cases_of(switches):
    return [c for c in CASES if c["switches"] == switches]


# ------------------------------------------------------------------------------------------------ buffers
def round_up(x, m):
    return (x + m - 1) // m * m


def layout(p):
    """Leading dimensions and allocation sizes of a problem: operands and output sit inside larger buffers"""
    M, N, K = p["M"], p["N"], p["K"]
    if p["form"] == "nt":
        Kp = round_up(K, 8)
        lay = dict(lda=Kp + 8, ldb=Kp + 8, a_rows=M, b_rows=N, a0=0, b0=0)
    else:
        a0, b0, pad = p.get("a0", 0), p.get("b0", 0), p.get("ld_pad", 8)
        lay = dict(lda=round_up(a0 + M, 8) + pad, ldb=round_up(b0 + N, 8) + pad, a_rows=K + 3, b_rows=K + 3, a0=a0, b0=b0)
    lay.update(ldc=N + p.get("ldc_pad", 4 if N % 4 == 0 else 3), c_rows=M + 2, bg_len=M + 8)
    return lay


def plan_problem(p):
    """The problem by shape alone, as ops.gemm_bf16_plan takes it (addresses: only their alignment matters)"""
    lay = layout(p)
    base = 1 << 20
    d = dict(M=p["M"], N=p["N"], K=p["K"], tn=p["form"] == "tn", lda=lay["lda"], ldb=lay["ldb"], ldc=lay["ldc"],
             A_addr=base + 2 * lay["a0"], B_addr=base + 2 * lay["b0"], C_addr=base)
    for k in ("bias", "bias2", "bias_grad", "bias_grad2", "accumulate", "perm_n_H", "perm_m_H", "alpha"):
        if k in p:
            d[k] = p[k]
    return d


SENTINEL_BITS = 0x7FC5A5A5                          # a quiet NaN with a payload: what surrounds the output window


def sentinel(shape):
    return torch.full(shape, SENTINEL_BITS, dtype=torch.int32).view(torch.float32)


def gate_perm(n):
    j = torch.arange(n)
    return (j // (4 * H)) * 4 * H + (j % 4) * H + (j % (4 * H)) // 4


def make_data(p, family, seed):
    """Host tensors of one problem.  family "a": integer-valued operands in [-8, 8] and small-integer C0 / biases (every partial sum
    is an integer below 2^24: exact in fp32 in any order); "b": randn; "c": as "a" with NaN in every operand element the contract
    says is not read (elsewhere that padding holds 3.0, which nothing may read either)."""
    gen = torch.Generator().manual_seed(seed)
    M, N, K = p["M"], p["N"], p["K"]
    lay = layout(p)
    exact = family in ("a", "c")

    def values(*shape):
        if exact:
            return torch.randint(-8, 9, shape, generator=gen).to(torch.bfloat16)
        return torch.randn(*shape, generator=gen).to(torch.bfloat16)

    def small(*shape):
        return torch.randint(-3, 4, shape, generator=gen).float() if exact else torch.randn(*shape, generator=gen)

    A, B = values(M, K), values(N, K)                 # the logical operands: C = alpha A B^T ...
    fill = float("nan") if family == "c" else 3.0
    if p["form"] == "nt":
        Kp = round_up(K, 8)
        Abuf = torch.full((lay["a_rows"], lay["lda"]), fill, dtype=torch.bfloat16); Bbuf = torch.full((lay["b_rows"], lay["ldb"]), fill, dtype=torch.bfloat16)
        Abuf[:, :K] = A; Abuf[:, K:Kp] = 0; Bbuf[:, :K] = B; Bbuf[:, K:Kp] = 0       # the contract: zero up to the 8-padded depth
    else:
        Abuf = torch.full((lay["a_rows"], lay["lda"]), fill, dtype=torch.bfloat16); Bbuf = torch.full((lay["b_rows"], lay["ldb"]), fill, dtype=torch.bfloat16)
        Abuf[:K, lay["a0"]:lay["a0"] + M] = A.t(); Bbuf[:K, lay["b0"]:lay["b0"] + N] = B.t()
    d = dict(A=A, B=B, Abuf=Abuf, Bbuf=Bbuf, Cbuf=sentinel((lay["c_rows"], lay["ldc"])))
    d["C0"] = small(M, N) if p.get("accumulate") else None
    if d["C0"] is not None:
        d["Cbuf"][:M, :N] = d["C0"]
    for k in ("bias", "bias2"):
        d[k] = small(N) if p.get(k) else None
    for k in ("bias_grad", "bias_grad2"):
        d[k + "0"] = small(M) if p.get(k) else None
        d[k + "buf"] = None
        if p.get(k):
            d[k + "buf"] = sentinel((lay["bg_len"],)); d[k + "buf"][:M] = d[k + "0"]
    return d


def reference(p, d, rows=None):
    """float64 results of the problem and the magnitudes its error bound scales with: (C, mag_C, {bias_grad: (ref, mag)}).  C is
    (M, N) as it lies in the output window.  rows: compute only these logical rows m of the product (then C and mag_C hold only the
    output rows they are written to, in the order given)."""
    M, N = p["M"], p["N"]
    A, B = d["A"].double(), d["B"].double()
    m_idx = torch.arange(M) if rows is None else torch.as_tensor(rows)
    A = A[m_idx]
    alpha = p.get("alpha", 1.0)
    C = alpha * (A @ B.t()); mag = abs(alpha) * (A.abs() @ B.abs().t())
    pn = gate_perm(N) if p.get("perm_n_H") else torch.arange(N)
    for k in ("bias", "bias2"):
        if d[k] is not None:
            C += d[k].double()[pn]; mag += d[k].double().abs()[pn]
    pm = gate_perm(M) if p.get("perm_m_H") else torch.arange(M)
    out_rows = pm[m_idx]                              # logical row m is written to row orig(m)
    if d["C0"] is not None:
        C += d["C0"].double()[out_rows]; mag += d["C0"].double().abs()[out_rows]
    if rows is None:                                  # as it lies in memory
        Cm = torch.empty_like(C); Cm[out_rows] = C; magm = torch.empty_like(mag); magm[out_rows] = mag
        C, mag = Cm, magm
    grads = {}
    for k in ("bias_grad", "bias_grad2"):
        if d[k + "0"] is not None:
            g = d[k + "0"].double().clone(); gm = g.abs()
            g[out_rows] += A.sum(1); gm[out_rows] += A.abs().sum(1)
            grads[k] = (g[out_rows], gm[out_rows]) if rows is not None else (g, gm)
    return C, mag, grads, out_rows


U = 2.0 ** -24
FACTOR = {i: 8.0 for i in NS}                       # working bar of family (b): FACTOR sqrt(n) u mag, n = K + 8


def bars(K, mag, inst):
    """(working bar, hard ceiling) of family (b) per element: the ceiling is the worst case of n fp32 roundings, n u / (1 - n u) mag"""
    n = K + 8
    return FACTOR[inst] * (n ** 0.5) * U * mag, n * U / (1 - n * U) * mag


def seed_of(case, k, family):
    return zlib.crc32(f"{case['name']}/{k}/{'b' if family == 'b' else 'a'}".encode())
