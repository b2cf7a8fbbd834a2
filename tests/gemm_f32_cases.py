"""The edge cases of the fp32-operand GEMMs (mmda_amd/csrc/gemm.hip, gemm_skinny.hip, splitk.hip): mmda_gemm, mmda_gemm_grouped, the
split-K reduce behind them, mmda_gemm_skinny and mmda_colsum.  Defined once for the CPU test that proves what each case reaches
(test_gemm_f32_plan_cpu.py) and the GPU test that checks its numbers (test_gpu_gemm_f32_edges.py).

A case is one call: its problems, and per problem the kernel instance, the k-slices and the reduce form it is meant to get.  Instances:
f32/PF1, f32/PF4, bf16/PF1, bf16/PF4 = gemm_kernel<MODE, PF>; t128/nn .. t128/tt = gemm128_bf16_kernel<TA, TB>; group/f32, group/bf16 =
the two gemm_body instances of gemm_grouped_kernel; skinny/<nn|nt>/<vec|scalar> = skinny_product<TB, VEC>; colsum.  A slice length
counts k-tiles of 32.  Also here: the buffers of a problem (every operand and output sits inside a larger flat buffer; what surrounds
them is part of the test) and its float64 reference, both plain torch on the CPU.  Dropout masks come from oracle/dropout_rng.py, never
from another kernel.
"""
import zlib

import numpy as np
import torch

import gemm_bf16_cases as gb
from gemm_bf16_cases import SENTINEL_BITS, U, sentinel  # noqa: F401  (re-exported for the tests)
from mmda_amd import _lib
from oracle import dropout_rng

FACTOR = gb.FACTOR["reg64"]                         # the project's working bar for fp32-accumulated MFMA sums: 8 sqrt(n) u mag
GEMM_INSTANCES = ("f32/PF1", "f32/PF4", "bf16/PF1", "bf16/PF4", "t128/nn", "t128/nt", "t128/tn", "t128/tt", "group/f32", "group/bf16")
SKINNY_INSTANCES = ("skinny/nn/vec", "skinny/nn/scalar", "skinny/nt/vec", "skinny/nt/scalar")
FORMS = ("nt", "nn", "tn", "tt")
TILE_EDGES = ((1, 1), (63, 65), (65, 63), (64, 64), (129, 64))
DROP_P, DROP_SEED, DROP_SITE = 0.5, 0x5EED1234, 3    # p = 0.5: the kept multiplier is exactly 2
GATE_SCALE = 2.0
FAKE = 1 << 20                                       # a 16-byte aligned address for the plan view
BAD_ID = 1 << 40                                     # the gather array's padding: an index that must never be dereferenced
EPI_FEATURES = ("alpha", "alpha0", "bias", "bias2", "accumulate", "relu", "drop", "gate", "A2", "gather", "all")
SPLIT_FEATURES = ("bias", "bias2", "alpha", "accumulate", "A2", "gather", "all")


def instance_of(row):
    """The kernel instance pick_kernel() / gemm_grouped_kernel names for a plan row"""
    mode = "bf16" if row["mode"] == _lib.BF16 else "f32"
    if row["cls"] == "Tile128":
        return "t128/" + ("t" if row["ta"] else "n") + ("t" if row["tb"] else "n")
    if row["cls"] == "GroupSlot":
        return "group/" + mode
    return mode + ("/PF4" if row["cls"] == "Tile64Tiny" else "/PF1")


def G(mode, form, M, N, K, inst, sk=1, per=None, last=None, reduce=None, **kw):
    """One mmda_gemm problem and what the plan is meant to say about it.  inst: PF1 / PF4 / t128 / group / none (an empty problem)"""
    nk = -(-K // 32)
    per = nk if per is None else per
    name = {"t128": "t128/" + form, "group": "group/" + mode, "none": None}.get(inst, mode + "/" + inst)
    return dict(kind="gemm", mode=mode, form=form, M=M, N=N, K=K, batch=kw.pop("batch", 1),
                expect=dict(inst=name, sk=sk, per=per, last=per if last is None else last, reduce=reduce), **kw)


def feat(name):
    return {"plain": {}, "alpha": dict(alpha=-0.5), "alpha0": dict(alpha=0.0), "bias": dict(bias=True), "bias2": dict(bias=True, bias2=True),
            "accumulate": dict(accumulate=True), "relu": dict(act="relu"), "leakyrelu": dict(act="leakyrelu"), "drop": dict(drop=True),
            "gate": dict(gate=True), "A2": dict(A2=True), "gather": dict(gather=True)}[name]


def _gemm_cases():
    out = []

    def add(name, problems, call="gemm", **tags):
        out.append(dict(name=name, call=call, problems=problems if isinstance(problems, list) else [problems], **tags))

    # ---- generic 64 x 64 x 32 tile: the unsplit k-walk, every layout, last k-tile full and ragged
    i = 0
    for mode in ("f32", "bf16"):
        for form in FORMS:
            for nk in range(1, 7):
                for tail in (32, 1, 3, 31):
                    M, N = TILE_EDGES[i % len(TILE_EDGES)]
                    kw = dict(bias_grad=True) if form == "tn" and i % 3 == 1 else {}
                    add(f"{mode}-{form}-nk{nk}-k{tail}", G(mode, form, M, N, 32 * (nk - 1) + tail, "PF4" if nk <= 4 else "PF1", **kw), walk=True)
                    i += 1
    # PF1 at 1, 2 and 4 k-tiles: more than 1024 blocks (1025 tiny batch entries), A broadcast (strideA = 0) or strided
    for mode in ("f32", "bf16"):
        for k, nk in enumerate((1, 2, 4)):
            for bc in (True, False):
                form = FORMS[(k + bc) % 4]
                add(f"{mode}-{form}-nk{nk}-batch1025" + ("-bcastA" if bc else ""),
                    G(mode, form, 3, 3, 32 * nk - (1 if bc else 0), "PF1", batch=1025, bcastA=bc, bias=not bc), walk=True)
    # ---- tile edges: every (M, N) on every instance (the k-walk cycles through them; here each at a fixed K, all layouts)
    for mode in ("f32", "bf16"):
        for k, (M, N) in enumerate(TILE_EDGES):
            for K, pf in ((45, "PF4"), (170, "PF1")):
                add(f"{mode}-{FORMS[k % 4]}-edge-{M}x{N}-K{K}", G(mode, FORMS[k % 4], M, N, K, pf))
    # ---- the bias gradient's ones-column: alone in a column tile of its own (N = 64, 128), last column inside a tile (N = 63)
    for mode in ("f32", "bf16"):
        for N in (64, 128, 63):
            for K, pf in ((45, "PF4"), (170, "PF1")):
                add(f"{mode}-tn-ones-column-N{N}-K{K}", G(mode, "tn", 65, N, K, pf, bias_grad=True, bias_grad2=K == 45, accumulate=N == 63))
        add(f"{mode}-tn-ones-column-batch3", G(mode, "tn", 65, 64, 45, "PF4", batch=3, bias_grad=True, bias_grad2=True))
    # ---- split-K, plain epilogue, one tile: no split at 7 k-tiles, then the slice arithmetic's corners
    one_tile = ((7, 1, 7, 7, "PF1"), (8, 4, 2, 2, "PF4"), (9, 3, 3, 3, "PF4"), (10, 5, 2, 2, "PF4"), (131, 44, 3, 2, "PF4"))
    for mode in ("f32", "bf16"):
        for k, (nk, sk, per, last, pf) in enumerate(one_tile):
            for vec in (True, False):
                M, N, pad = (61, 64, 4) if vec else (63, 61, 3)
                red = None if sk == 1 else ("vector" if vec else "scalar")
                add(f"{mode}-{FORMS[(k + vec) % 4]}-split-nk{nk}-{'vec' if vec else 'scalar'}",
                    G(mode, FORMS[(k + vec) % 4], M, N, 32 * nk - (0 if vec else 5), pf, sk=sk, per=per, last=last, reduce=red, ldc_pad=pad))
        # PF1 behind a split: 96 tiles of 41 k-tiles -> 7 slices of 6, the last one 5 (K % 4 != 0 keeps the bf16 problem off the 128 tile)
        add(f"{mode}-nt-split-nk41-96tiles", G(mode, "nt", 500, 760, 1309, "PF1", sk=7, per=6, last=5, reduce="vector", ldc_pad=4))
    # SPLIT_MAX_TILES: 256 tiles of 8 k-tiles split, 272 do not
    add("f32-nt-split-256-tiles", G("f32", "nt", 1024, 1024, 256, "PF4", sk=3, per=3, last=2, reduce="vector", ldc_pad=4))
    add("f32-nt-nosplit-272-tiles", G("f32", "nt", 1024, 1088, 256, "PF1", ldc_pad=4))
    # split with each epilogue feature the reduce knows, through both reduce forms; refused by each feature it does not know
    for mode in ("f32", "bf16"):
        for f in SPLIT_FEATURES:
            for vec in (True, False):
                kw = dict(alpha=-0.5, bias=True, bias2=True, accumulate=True, A2=True, gather=True) if f == "all" else feat(f)
                M, N, pad = (61, 64, 4) if vec else (65, 63, 3)
                add(f"{mode}-nt-split-{f}-{'vec' if vec else 'scalar'}",
                    G(mode, "nt", M, N, 250, "PF4", sk=4, per=2, last=2, reduce="vector" if vec else "scalar", ldc_pad=pad, **kw), epi=(f, "reduce"))
        for f in ("relu", "drop", "gate"):
            add(f"{mode}-nt-split-refused-{f}", G(mode, "nt", 61, 64, 250, "PF1", ldc_pad=4, **feat(f)), refused=f)
        # batched problems that split: scalar reduce with bz, strideC, strideBias
        add(f"{mode}-nt-split-batch3-bias", G(mode, "nt", 61, 64, 250, "PF4", sk=4, per=2, last=2, reduce="scalar", batch=3, ldc_pad=4,
                                              bias=True, bias2=True, accumulate=True))
        add(f"{mode}-tn-split-batch3-bias-grad", G(mode, "tn", 61, 63, 250, "PF4", sk=4, per=2, last=2, reduce="scalar", batch=3,
                                                   bias_grad=True, bias_grad2=True, alpha=-0.5))
    # the reduce form: 16-byte, and scalar by each single disqualifier
    base = dict(sk=4, per=2, last=2)
    add("reduce-vector", G("f32", "nt", 61, 64, 256, "PF4", reduce="vector", ldc_pad=4, **base), reduce_why="none")
    add("reduce-scalar-N66", G("f32", "nt", 61, 66, 256, "PF4", reduce="scalar", ldc_pad=2, **base), reduce_why="N")
    add("reduce-scalar-ldc", G("f32", "nt", 61, 64, 256, "PF4", reduce="scalar", ldc_pad=5, **base), reduce_why="ldc")
    add("reduce-scalar-bias-grad", G("f32", "tn", 61, 64, 256, "PF4", reduce="scalar", ldc_pad=4, bias_grad=True, **base), reduce_why="bias_grad")
    add("reduce-scalar-batch2", G("f32", "nt", 61, 64, 256, "PF4", reduce="scalar", ldc_pad=4, batch=2, **base), reduce_why="batch")
    add("reduce-scalar-C-offset", G("f32", "nt", 61, 64, 256, "PF4", reduce="scalar", ldc_pad=4, c_off=1, **base), reduce_why="C")
    # ---- epilogue matrix, unsplit: each feature alone and all together.  M = 65: a row tile that holds one valid row (gather: one id)
    for mode in ("f32", "bf16"):
        for f in EPI_FEATURES:
            kw = dict(alpha=-0.5, bias=True, bias2=True, accumulate=True, act="relu", drop=True, gate=True, A2=True, gather=True) if f == "all" else feat(f)
            for K, pf in ((45, "PF4"), (170, "PF1")):
                add(f"{mode}-nt-epilogue-{f}-K{K}", G(mode, "nt", 65, 63, K, pf, **kw), epi=(f, "direct"))
        add(f"{mode}-nt-epilogue-leakyrelu", G(mode, "nt", 65, 63, 45, "PF4", bias=True, act="leakyrelu"), only="b")
        add(f"{mode}-nn-epilogue-gate-batch2", G(mode, "nn", 65, 63, 45, "PF4", batch=2, gate=True, drop=True, bias=True))
    # ---- 128 x 128 bf16 tile: four instances, one or two k-tiles and a walk with a ragged last tile (K = 300 splits: 5 slices of 2)
    for form in FORMS:
        for M, N in ((128, 128), (132, 252), (260, 132)):
            for K in (4, 28, 32, 36, 64, 300):
                sp = dict(sk=5, per=2, last=2, reduce="vector") if K == 300 else {}
                add(f"t128-{form}-{M}x{N}-K{K}", G("bf16", form, M, N, K, "t128", lda_pad=4, ldb_pad=4, ldc_pad=4, **sp), walk128=True)
        add(f"t128-{form}-split-nk32", G("bf16", form, 132, 252, 1024, "t128", sk=16, per=2, last=2, reduce="vector", lda_pad=4, ldb_pad=4,
                                         ldc_pad=4, accumulate=True, alpha=-0.5))
        add(f"t128-{form}-batch2", G("bf16", form, 128, 128, 300, "t128", sk=5, per=2, last=2, reduce="scalar", batch=2, lda_pad=4, ldb_pad=4,
                                     ldc_pad=4, bias=True))
        # sub-matrix windows: big leading dimensions, bases four floats (16 bytes) into their buffers
        add(f"t128-{form}-window", G("bf16", form, 132, 252, 36, "t128", lda_pad=260, ldb_pad=132, ldc_pad=8, a_off=4, b_off=8, bias=True, bias2=True))
    # the conditional 16-byte loads test their first element only: tn, M = 132 in rows of 136 with poison in columns 132 .. 135
    add("t128-tn-poison-behind-M132", G("bf16", "tn", 132, 128, 36, "t128", lda_pad=4, ldb_pad=4, ldc_pad=4))
    # the fall-through boundaries: each lands on the 64 tile
    t = dict(lda_pad=4, ldb_pad=4, ldc_pad=4)
    for why, p in (("M127", G("bf16", "nt", 127, 128, 36, "PF4", **t)), ("N127", G("bf16", "nt", 128, 127, 36, "PF4", **t)),
                   ("K30", G("bf16", "nt", 128, 128, 30, "PF4", lda_pad=2, ldb_pad=2, ldc_pad=4)),
                   ("lda", G("bf16", "nt", 128, 128, 36, "PF4", lda_pad=2, ldb_pad=4, ldc_pad=4)),
                   ("A-offset", G("bf16", "nt", 128, 128, 36, "PF4", a_off=1, **t)),
                   ("tn-M", G("bf16", "tn", 130, 128, 36, "PF4", lda_pad=2, ldb_pad=4, ldc_pad=4)),
                   ("nn-N", G("bf16", "nn", 128, 130, 36, "PF4", lda_pad=4, ldb_pad=2, ldc_pad=4)),
                   ("bias_grad", G("bf16", "tn", 128, 128, 36, "PF4", bias_grad=True, **t)), ("A2", G("bf16", "nt", 128, 128, 36, "PF4", A2=True, **t)),
                   ("gather", G("bf16", "nt", 128, 128, 36, "PF4", gather=True, **t)), ("act", G("bf16", "nt", 128, 128, 36, "PF4", act="relu", **t))):
        add("t128-refused-" + why, p, refused128=why)
    # ---- grouped kernel: 17 problems = a full launch and a second one of one slot; first and last slot of one block (both ends of the
    # prefix search); an empty problem in the middle; modes, layouts, split and unsplit side by side; a split slot whose slab starts
    # off the 16-byte grid (scalar reduce for a shape that would take the 16-byte one: problem 5 against problem 2)
    s4 = dict(sk=4, per=2, last=2)
    group = [G("f32", "nt", 3, 3, 40, "group"),
             G("bf16", "nt", 65, 63, 45, "group", bias=True),
             G("f32", "nt", 61, 64, 256, "group", reduce="vector", ldc_pad=4, **s4),
             G("f32", "nn", 3, 3, 288, "group", sk=3, per=3, last=3, reduce="scalar"),
             G("f32", "nt", 0, 5, 40, "none"),
             G("f32", "nt", 61, 64, 256, "group", reduce="scalar", ldc_pad=4, accumulate=True, **s4),
             G("bf16", "tn", 65, 63, 300, "group", sk=5, per=2, last=2, reduce="scalar", bias_grad=True, accumulate=True),
             G("bf16", "tn", 65, 64, 45, "group", bias_grad=True, bias_grad2=True, accumulate=True),
             G("f32", "tt", 63, 65, 97, "group", alpha=-0.5),
             G("bf16", "nn", 129, 64, 170, "group", act="relu", bias=True),
             G("f32", "nt", 65, 63, 250, "group", gate=True, drop=True),                      # nk = 8, split refused by its epilogue
             G("bf16", "tt", 64, 64, 64, "group"),
             G("f32", "tn", 1, 1, 1, "group", bias_grad=True),
             G("bf16", "nt", 65, 63, 250, "group", reduce="scalar", gather=True, A2=True, bias=True, bias2=True, **s4),
             G("f32", "nn", 64, 129, 33, "group", accumulate=True),
             G("bf16", "nn", 3, 3, 31, "group"),
             G("f32", "nt", 63, 65, 256, "group", reduce="scalar", **s4)]
    add("grouped-17-problems", group, call="grouped")
    add("grouped-16-problems", [dict(p) for p in group[:16]], call="grouped")
    return out


# ------------------------------------------------------------------------------------------------ skinny
def S(M, N, K, tb, form, second=None, **kw):
    """One mmda_gemm_skinny problem.  form / second: vec or scalar, the form its first / second product is meant to take"""
    return dict(kind="skinny", M=M, N=N, K=K, tb=tb, expect=dict(form=form, second=second), **kw)


SKINNY_CHUNKS = (1, 2, 7, 8, 9, 31, 32, 33, 64, 65)     # fewer chunks than waves; one and two rounds of the prefetch ring, one past each
SKINNY_SHAPES = ((1, 1), (31, 17), (33, 15), (32, 16), (97, 33))


def _skinny_cases():
    out = []

    def add(name, problems, **tags):
        out.append(dict(name=name, call="skinny", problems=problems if isinstance(problems, list) else [problems], **tags))

    i = 0
    for tb in (True, False):
        for nch in SKINNY_CHUNKS:
            for tail in (16, 4, 5):
                M, N = SKINNY_SHAPES[i % len(SKINNY_SHAPES)]
                add(f"skinny-{'nt' if tb else 'nn'}-chunks{nch}-k{tail}", S(M, N, 16 * (nch - 1) + tail, tb, "scalar" if tail == 5 else "vec"), walk=True)
                i += 1
        # every shape in both forms
        for M, N in SKINNY_SHAPES:
            for K, form in ((40, "vec"), (37, "scalar")):
                add(f"skinny-{'nt' if tb else 'nn'}-edge-{M}x{N}-K{K}", S(M, N, K, tb, form))
        # the 16-byte form lost by each cause alone
        tag = "nt" if tb else "nn"
        add(f"skinny-{tag}-novec-A-offset", S(33, 15, 40, tb, "scalar", a_off=1), lost="A")
        add(f"skinny-{tag}-novec-lda", S(33, 15, 40, tb, "scalar", lda_odd=True), lost="lda")
        add(f"skinny-{tag}-novec-K", S(33, 15, 42, tb, "scalar"), lost="K")
        add(f"skinny-{tag}-novec-A2-offset", S(33, 15, 40, tb, "scalar", A2=True, a2_off=1), lost="A2")
        add(f"skinny-{tag}-B-offset", S(33, 15, 40, tb, "scalar" if tb else "vec", b_off=1), lost="B")
        add(f"skinny-{tag}-ldb-odd", S(33, 15, 40, tb, "scalar" if tb else "vec", ldb_odd=True), lost="ldb")
        # two products: K2 != K, one in each form
        add(f"skinny-{tag}-second-vec-vec", S(33, 17, 40, tb, "vec", "vec", K2=20))
        add(f"skinny-{tag}-second-vec-scalar", S(33, 17, 40, tb, "vec", "scalar", K2=21))
        add(f"skinny-{tag}-second-scalar-vec", S(33, 17, 42, tb, "scalar", "vec", K2=148))
        add(f"skinny-{tag}-second-scalar-scalar", S(33, 17, 40, tb, "scalar", "scalar", K2=20, a_off=1, a2nd_off=2, accumulate=True, alpha=-0.5))
        # epilogue: each feature alone in both forms, then together
        feats = dict(alpha=dict(alpha=-0.5), alpha0=dict(alpha=0.0), bias=dict(bias=True), accumulate=dict(accumulate=True), relu=dict(act="relu"),
                     drop=dict(drop=True), gate=dict(gate=True), dsig=dict(dsig=True), A2=dict(A2=True),
                     C2=dict(C2=True), C2full=dict(C2=True, accumulate=True, dsig=True, dsig2=True, alpha=-0.5),
                     all=dict(alpha=-0.5, bias=True, accumulate=True, act="relu", drop=True, gate=True, dsig=True, A2=True))
        for f, kw in feats.items():
            for K, form in ((148, "vec"), (37, "scalar")):
                add(f"skinny-{tag}-epilogue-{f}-K{K}", S(33, 17, K, tb, form, **kw), epi=f)
        add(f"skinny-{tag}-epilogue-leakyrelu", S(33, 17, 40, tb, "vec", bias=True, act="leakyrelu"), only="b")
    # nine problems in one call: two launches (8 + 1), an empty one among them
    nine = [S(31, 17, 40, True, "vec", bias=True), S(1, 1, 5, False, "scalar"), S(97, 33, 148, False, "vec", accumulate=True),
            S(0, 16, 16, True, "vec"), S(33, 15, 37, True, "scalar", act="relu", bias=True), S(32, 16, 520, True, "vec", drop=True),
            S(33, 17, 40, False, "vec", "scalar", K2=21), S(32, 16, 16, False, "vec", C2=True, dsig2=True), S(33, 15, 1029, True, "scalar", alpha=-0.5)]
    add("skinny-nine-problems", nine)
    return out


# ------------------------------------------------------------------------------------------------ column sums
def _colsum_cases():
    out = []
    i = 0
    for M in (1, 255, 256, 257, 513):                   # the 256-row block edge
        for N in (1, 63, 64, 65):
            out.append(dict(name=f"colsum-{M}x{N}", call="colsum", problems=[dict(kind="colsum", M=M, N=N, out2=i % 2 == 0, expect={})]))
            i += 1
    return out


CASES = _gemm_cases() + _skinny_cases() + _colsum_cases()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def families_of(case):
    return (case["only"],) if case.get("only") else ("a", "b", "c")


def seed_of(case, k, family):
    return zlib.crc32(f"{case['name']}/{k}/{'b' if family == 'b' else 'a'}".encode())


# ------------------------------------------------------------------------------------------------ buffers
def round_up(x, m):
    return (x + m - 1) // m * m


class Buf:
    """A flat fp32 buffer that holds `nb` matrices of `rows` x `cols` with leading dimension ld, the first one `off` floats in, `stride`
    floats apart (0: one matrix), with two more rows of the same ld below each; everything but the matrices holds `fill`."""

    def __init__(self, rows, cols, ld, off=0, nb=1, stride=None, fill=3.0, sent=False):
        self.rows, self.cols, self.ld, self.off = rows, cols, ld, off
        self.stride = (rows + 2) * ld if stride is None else stride
        self.nb = 1 if self.stride == 0 else nb
        size = off + (self.nb - 1) * self.stride + (rows + 2) * ld + 4
        self.flat = sentinel((size,)) if sent else torch.full((size,), fill, dtype=torch.float32)

    def window(self, flat=None):
        return torch.as_strided(self.flat if flat is None else flat, (self.nb, self.rows, self.cols), (max(self.stride, 1), self.ld, 1), self.off)

    def outside(self):
        m = torch.ones(self.flat.shape, dtype=torch.bool)
        torch.as_strided(m, (self.nb, self.rows, self.cols), (max(self.stride, 1), self.ld, 1), self.off).fill_(False)
        return m


def gemm_layout(p):
    M, N, K, nb = p["M"], p["N"], p["K"], p["batch"]
    ta, tb = p["form"][0] == "t", p["form"][1] == "t"
    a_rows, a_cols = (K, M) if ta else ((9 if p.get("gather") else M), K)
    b_rows, b_cols = (N, K) if tb else (K, N)
    lay = dict(ta=ta, tb=tb, a_rows=a_rows, a_cols=a_cols, b_rows=b_rows, b_cols=b_cols,
               lda=a_cols + p.get("lda_pad", 3), ldb=b_cols + p.get("ldb_pad", 3), ldc=N + p.get("ldc_pad", 3), ldgate=N + 5,
               a_off=p.get("a_off", 0), b_off=p.get("b_off", 0), c_off=p.get("c_off", 0))
    lay["strideA"] = 0 if p.get("bcastA") or nb == 1 else (a_rows + 2) * lay["lda"]
    lay["strideB"] = 0 if nb == 1 else (b_rows + 2) * lay["ldb"]
    # a batched gate lies as its C does (mmda_hip.h): one batch stride for both
    lay["strideC"] = 0 if nb == 1 else (M + 2) * max(lay["ldc"], lay["ldgate"] if p.get("gate") else 0)
    lay["strideBias"] = 0 if nb == 1 else max(M, N) + 3
    return lay


def _gen(family, seed):
    gen = torch.Generator().manual_seed(seed)
    exact = family in ("a", "c")

    def values(*shape):
        return torch.randint(-8, 9, shape, generator=gen).float() if exact else torch.randn(*shape, generator=gen)

    def small(*shape):
        return torch.randint(-3, 4, shape, generator=gen).float() if exact else torch.randn(*shape, generator=gen)

    def signs(*shape):
        return torch.randint(-1, 2, shape, generator=gen).float()

    return gen, values, small, signs


def _vector(x, tail=8):
    """(nb, n) values with a sentinel tail behind each row"""
    buf = sentinel((x.shape[0], x.shape[1] + tail)) if tail else torch.empty_like(x)
    buf[:, :x.shape[1]] = x
    return buf


def make_gemm(p, family, seed):
    """Host tensors of one mmda_gemm problem.  family "a": integer-valued operands in [-8, 8], small-integer C0 / biases / gradient
    seeds (every partial sum exact in fp32 and in bf16 mode, in any order); "b": randn; "c": as "a" with NaN in every element the
    contract says is never read (elsewhere that padding holds 3.0, which nothing may read either)."""
    gen, values, small, signs = _gen(family, seed)
    M, N, K, nb = p["M"], p["N"], p["K"], p["batch"]
    lay = gemm_layout(p)
    fill = float("nan") if family == "c" else 3.0
    d = dict(lay=lay)
    nbA = 1 if lay["strideA"] == 0 else nb
    nbB = 1 if lay["strideB"] == 0 else nb
    for name in ("A", "A2"):
        if name == "A2" and not p.get("A2"):
            d["A2"] = d["A2buf"] = None
            continue
        phys = values(nbA, lay["a_rows"], lay["a_cols"])                   # as it lies in memory: (K, M), (M, K) or the gather table
        d[name + "buf"] = Buf(lay["a_rows"], lay["a_cols"], lay["lda"], lay["a_off"], nbA, lay["strideA"], fill)
        d[name + "buf"].window()[:] = phys
        d[name + "phys"] = phys
    if p.get("gather"):
        ids = torch.randint(0, lay["a_rows"], (max(M, 1),), generator=gen)[:M]
        d["ids"] = ids
        d["gather"] = torch.cat([ids, torch.full((8,), BAD_ID, dtype=torch.int64)])     # exactly M entries, then poison
    for name in ("A", "A2"):
        if d[name + "buf"] is not None:
            x = d[name + "phys"]
            d[name] = x.transpose(1, 2) if lay["ta"] else (x[:, d["ids"]] if p.get("gather") else x)       # (nbA, M, K)
    Bp = values(nbB, lay["b_rows"], lay["b_cols"])
    d["Bbuf"] = Buf(lay["b_rows"], lay["b_cols"], lay["ldb"], lay["b_off"], nbB, lay["strideB"], fill)
    d["Bbuf"].window()[:] = Bp
    d["B"] = Bp if lay["tb"] else Bp.transpose(1, 2)                           # (nbB, N, K)
    d["Cbuf"] = Buf(M, N, lay["ldc"], lay["c_off"], nb, lay["strideC"] or None, sent=True)
    d["C0"] = small(nb, M, N) if p.get("accumulate") else None
    if d["C0"] is not None:
        d["Cbuf"].window()[:] = d["C0"]
    for k in ("bias", "bias2"):
        d[k] = small(nb, N) if p.get(k) else None
        d[k + "buf"] = None if d[k] is None else _vector(d[k], max(lay["strideBias"] - N, 0) if nb > 1 else 0)
    for k in ("bias_grad", "bias_grad2"):
        d[k + "0"] = small(nb, M) if p.get(k) else None
        d[k + "buf"] = None if d[k + "0"] is None else _vector(d[k + "0"], lay["strideBias"] - M if nb > 1 else 8)
    d["gate"] = d["gatebuf"] = None
    if p.get("gate"):
        d["gate"] = signs(nb, M, N)
        d["gatebuf"] = Buf(M, N, lay["ldgate"], 0, nb, lay["strideC"] or None, fill)
        d["gatebuf"].window()[:] = d["gate"]
    d["mask"] = None
    if p.get("drop"):
        idx = np.arange(nb * M * N, dtype=np.uint64)                          # ((bz M + m) N + n)
        d["mask"] = torch.from_numpy(dropout_rng.drop_mul(DROP_P, DROP_SEED, DROP_SITE, idx).reshape(nb, M, N))
    return d


def _round(x32, mode):
    """The value the MFMA multiplies: bf16 mode rounds the fp32 operand to nearest even"""
    return (x32.bfloat16() if mode == "bf16" else x32).double()


def _act(name, v):
    if name == "relu":
        return v.clamp_min(0)
    if name == "leakyrelu":
        return torch.where(v > 0, v, 0.01 * v)
    assert name in (None, "none")
    return v


def _epilogue(p, d, prod, mag):
    alpha = p.get("alpha", 1.0) or 1.0                  # 0 is read as 1
    C, mag = alpha * prod, abs(alpha) * mag
    for k in ("bias", "bias2"):
        if d.get(k) is not None:
            C = C + d[k].double()[:, None, :]; mag = mag + d[k].double().abs()[:, None, :]
    if d["C0"] is not None:
        C = C + d["C0"].double(); mag = mag + d["C0"].double().abs()
    C = _act(p.get("act"), C)
    if d["mask"] is not None:
        C = C * d["mask"]; mag = mag * d["mask"]
    if d["gate"] is not None:
        f = torch.where(d["gate"] > 0, GATE_SCALE, 0.0).double()
        C = C * f; mag = mag * f
    return C, mag


def ref_gemm(p, d):
    """float64 results and the magnitudes the error bound scales with: (C (nb, M, N), mag, {bias_grad name: (ref (nb, M), mag)})"""
    A32 = d["A"] if d["A2"] is None else d["A"] + d["A2"]                    # summed in fp32, as the kernel does
    A, B = _round(A32, p["mode"]), _round(d["B"], p["mode"])
    prod = torch.matmul(A, B.transpose(1, 2)); mag = torch.matmul(A.abs(), B.abs().transpose(1, 2))
    nb = p["batch"]
    C, mag = _epilogue(p, d, prod.expand(nb, -1, -1), mag.expand(nb, -1, -1))
    grads = {}
    for k in ("bias_grad", "bias_grad2"):
        if d[k + "0"] is not None:
            g0 = d[k + "0"].double()
            grads[k] = (g0 + A.sum(2).expand(nb, -1), g0.abs() + A.abs().sum(2).expand(nb, -1))
    return C, mag, grads


def gemm_args(p, addr=None):
    """The mmda_gemm_args of a problem.  addr: {buffer name: address of its first float}; None: the plan view's stand-ins (only the
    alignment of an address matters there)"""
    lay = gemm_layout(p)
    a = addr or {}

    def at(name, present=True, off=0):
        return (a.get(name, FAKE) + 4 * off) if present else None

    g = _lib.GemmArgs()
    g.mode = _lib.BF16 if p["mode"] == "bf16" else _lib.F32
    g.transA = int(lay["ta"]); g.transB = int(lay["tb"]); g.M = p["M"]; g.N = p["N"]; g.K = p["K"]; g.batch = p["batch"]
    g.A = at("A", off=lay["a_off"]); g.lda = lay["lda"]; g.strideA = lay["strideA"]
    g.A2 = at("A2", p.get("A2"), lay["a_off"]); g.gather = at("gather", p.get("gather"))
    g.B = at("B", off=lay["b_off"]); g.ldb = lay["ldb"]; g.strideB = lay["strideB"]
    g.C = at("C", off=lay["c_off"]); g.ldc = lay["ldc"]; g.strideC = lay["strideC"]
    g.bias = at("bias", p.get("bias")); g.bias2 = at("bias2", p.get("bias2")); g.strideBias = lay["strideBias"]
    g.accumulate = int(bool(p.get("accumulate"))); g.act = _lib.ACT[p.get("act") or "none"]
    if p.get("drop"):
        g.drop_p = DROP_P; g.drop_seed = DROP_SEED; g.drop_site = DROP_SITE
    g.gate = at("gate", p.get("gate")); g.ldgate = lay["ldgate"]; g.gate_scale = GATE_SCALE
    g.alpha = p.get("alpha", 1.0)
    g.bias_grad = at("bias_grad", p.get("bias_grad")); g.bias_grad2 = at("bias_grad2", p.get("bias_grad2"))
    return g


def exact_bound(p):
    """Family a's premise: the largest |value| a partial or final result of the problem can take, in units of its finest binary
    fraction -- below 2^24 every one of them is an fp32 number, whatever the order of the additions"""
    if p["kind"] == "colsum":
        return 8 * p["M"] + 3
    a = 16 if p.get("A2") else 8
    s = a * 8 * p["K"] + 64 * p.get("K2", 0)
    frac = 1
    alpha = p.get("alpha", 1.0) or 1.0
    s *= abs(alpha)
    if alpha != int(alpha):
        frac *= 2
    s += 3 * (bool(p.get("bias")) + bool(p.get("bias2")) + bool(p.get("accumulate")))
    if p.get("act") == "leakyrelu":
        return float("inf")                              # 0.01 v is not exact: family b only
    if p.get("drop"):
        s *= 2
    if p.get("gate"):
        s *= GATE_SCALE
    if p.get("dsig") or p.get("dsig2"):
        s *= 2; frac *= 4                                # s (1 - s) in {0, 1/4, -2}
    return max(s, a * p.get("K", 0) + 3) * frac          # (the bias gradient: K ones times |A + A2|, unscaled)


# ------------------------------------------------------------------------------------------------ skinny buffers
def skinny_layout(p):
    M, N, K, tb, K2 = p["M"], p["N"], p["K"], p["tb"], p.get("K2", 0)

    def ld(cols, odd):
        return round_up(cols, 4) + (5 if odd else 4)

    lay = dict(lda=ld(K, p.get("lda_odd")), ldb=ld(K if tb else N, p.get("ldb_odd")), a_off=p.get("a_off", 0), a2_off=p.get("a2_off", 0),
               b_off=p.get("b_off", 0), lda_2nd=ld(K2, False), ldb_2nd=ld(K2 if tb else N, False), a2nd_off=p.get("a2nd_off", 0),
               ldc=N + 3, ldc2=N + 6, ldgate=N + 5, lddsig=N + 2)
    if K2 and K2 % 4:
        lay["lda_2nd"] = K2 + 3
    return lay


def skinny_forms(p, align=None):
    """(form of the first product, of the second or None) by the kernel's rule: vec_ok(A, lda) && K % 4 == 0 && (!A2 || vec_ok(A2)), and
    for transB also vec_ok(B, ldb); vec_ok = 16-byte aligned base and ld % 4 == 0.  align: {buffer name: address} of the real
    buffers (None: bases taken as 16-byte aligned, the offsets decide)"""
    lay = skinny_layout(p)
    al = align or {}

    def vec_ok(name, off, ld):
        return (al.get(name, 0) + 4 * off) % 16 == 0 and ld % 4 == 0

    first = vec_ok("A", lay["a_off"], lay["lda"]) and p["K"] % 4 == 0 and (not p.get("A2") or vec_ok("A2", lay["a2_off"], lay["lda"]))
    if p["tb"]:
        first = first and vec_ok("B", lay["b_off"], lay["ldb"])
    second = None
    if p.get("K2"):
        second = vec_ok("A_2nd", lay["a2nd_off"], lay["lda_2nd"]) and p["K2"] % 4 == 0
        if p["tb"]:
            second = second and vec_ok("B_2nd", 0, lay["ldb_2nd"])
    name = {True: "vec", False: "scalar", None: None}
    return name[first], name[second]


def make_skinny(p, family, seed):
    gen, values, small, signs = _gen(family, seed)
    M, N, K, tb, K2 = p["M"], p["N"], p["K"], p["tb"], p.get("K2", 0)
    lay = skinny_layout(p)
    fill = float("nan") if family == "c" else 3.0
    d = dict(lay=lay)

    def operand(name, rows, cols, ld, off):
        x = values(1, rows, cols)
        d[name + "buf"] = Buf(rows, cols, ld, off, fill=fill)
        d[name + "buf"].window()[:] = x
        return x[0]

    d["A"] = operand("A", M, K, lay["lda"], lay["a_off"])
    d["A2"] = operand("A2", M, K, lay["lda"], lay["a2_off"]) if p.get("A2") else None
    B = operand("B", *((N, K) if tb else (K, N)), lay["ldb"], lay["b_off"])
    d["B"] = B if tb else B.t()                                               # (N, K)
    d["A_2nd"] = d["B_2nd"] = None
    if K2:
        d["A_2nd"] = operand("A_2nd", M, K2, lay["lda_2nd"], lay["a2nd_off"])
        B2 = operand("B_2nd", *((N, K2) if tb else (K2, N)), lay["ldb_2nd"], 0)
        d["B_2nd"] = B2 if tb else B2.t()
    for name, ld in (("C", lay["ldc"]), ("C2", lay["ldc2"])):
        d[name + "buf"] = d[name + "0"] = None
        if name == "C" or p.get("C2"):
            d[name + "buf"] = Buf(M, N, ld, sent=True)
            if p.get("accumulate"):
                d[name + "0"] = small(1, M, N)
                d[name + "buf"].window()[:] = d[name + "0"]
    d["C0"] = d.pop("C0")
    d["bias"] = small(1, N) if p.get("bias") else None
    d["biasbuf"] = d["bias"]
    d["gate"] = d["gatebuf"] = None
    if p.get("gate"):
        d["gate"] = signs(1, M, N)
        d["gatebuf"] = Buf(M, N, lay["ldgate"], fill=fill); d["gatebuf"].window()[:] = d["gate"]
    for k in ("dsig", "dsig2"):
        d[k] = d[k + "buf"] = None
        if p.get(k):
            if family == "b":
                d[k] = torch.rand(1, M, N, generator=gen)
            else:
                d[k] = torch.tensor([0.5, 2.0, -1.0, 0.0])[torch.randint(0, 4, (1, M, N), generator=gen)]
            d[k + "buf"] = Buf(M, N, lay["lddsig"], fill=fill); d[k + "buf"].window()[:] = d[k]
    d["mask"] = None
    if p.get("drop"):
        d["mask"] = torch.from_numpy(dropout_rng.drop_mul(DROP_P, DROP_SEED, DROP_SITE, np.arange(M * N, dtype=np.uint64)).reshape(1, M, N))
    return d


def ref_skinny(p, d):
    """float64: (C (1, M, N), mag, C2 or None, mag2)"""
    A32 = d["A"] if d["A2"] is None else d["A"] + d["A2"]
    A, B = A32.double(), d["B"].double()
    prod = A @ B.t(); mag = A.abs() @ B.abs().t()
    if d["A_2nd"] is not None:
        prod = prod + d["A_2nd"].double() @ d["B_2nd"].double().t(); mag = mag + d["A_2nd"].double().abs() @ d["B_2nd"].double().abs().t()
    prod, mag = prod[None], mag[None]
    C, mg = _epilogue(p, d, prod, mag)
    if d["dsig"] is not None:
        s = d["dsig"].float(); f = (s * (1 - s)).double()                     # the factor is an fp32 product in the kernel
        C = C * f; mg = mg * f.abs()
    C2 = mg2 = None
    if p.get("C2"):
        alpha = p.get("alpha", 1.0) or 1.0
        C2, mg2 = alpha * prod, abs(alpha) * mag
        if d["C20"] is not None:
            C2 = C2 + d["C20"].double(); mg2 = mg2 + d["C20"].double().abs()
        if d["dsig2"] is not None:
            s = d["dsig2"].float(); f = (s * (1 - s)).double()
            C2 = C2 * f; mg2 = mg2 * f.abs()
    return C, mg, C2, mg2


def skinny_args(p, addr=None):
    lay = skinny_layout(p)
    a = addr or {}

    def at(name, present=True, off=0):
        return (a.get(name, FAKE) + 4 * off) if present else None

    g = _lib.SkinnyArgs()
    g.M = p["M"]; g.N = p["N"]; g.K = p["K"]; g.transB = int(p["tb"])
    g.A = at("A", off=lay["a_off"]); g.A2 = at("A2", p.get("A2"), lay["a2_off"]); g.lda = lay["lda"]
    g.B = at("B", off=lay["b_off"]); g.ldb = lay["ldb"]
    if p.get("K2"):
        g.K2 = p["K2"]; g.A_2nd = at("A_2nd", off=lay["a2nd_off"]); g.lda_2nd = lay["lda_2nd"]; g.B_2nd = at("B_2nd"); g.ldb_2nd = lay["ldb_2nd"]
    g.C = at("C"); g.ldc = lay["ldc"]
    g.C2 = at("C2", p.get("C2")); g.ldc2 = lay["ldc2"]
    g.bias = at("bias", p.get("bias")); g.accumulate = int(bool(p.get("accumulate"))); g.alpha = p.get("alpha", 1.0)
    g.act = _lib.ACT[p.get("act") or "none"]
    if p.get("drop"):
        g.drop_p = DROP_P; g.drop_seed = DROP_SEED; g.drop_site = DROP_SITE
    g.gate = at("gate", p.get("gate")); g.ldgate = lay["ldgate"]; g.gate_scale = GATE_SCALE
    g.dsig = at("dsig", p.get("dsig")); g.dsig2 = at("dsig2", p.get("dsig2")); g.lddsig = lay["lddsig"]
    return g


# ------------------------------------------------------------------------------------------------ column sums
def make_colsum(p, family, seed):
    gen, values, small, signs = _gen(family, seed)
    M, N = p["M"], p["N"]
    d = dict(X=values(1, M, N), Xbuf=Buf(M, N, N + 3, fill=float("nan") if family == "c" else 3.0))
    d["Xbuf"].window()[:] = d["X"]
    for k in ("out", "out2"):
        d[k + "0"] = small(1, N) if (k == "out" or p["out2"]) else None
        d[k + "buf"] = None if d[k + "0"] is None else _vector(d[k + "0"])
    return d


def ref_colsum(p, d):
    X = d["X"].double()[0]
    return {k: (d[k + "0"].double()[0] + X.sum(0), d[k + "0"].double()[0].abs() + X.abs().sum(0)) for k in ("out", "out2") if d[k + "0"] is not None}


def bars(n_terms, mag):
    """(working bar, hard ceiling) of family b per element: FACTOR sqrt(n) u mag and the worst case of n fp32 roundings,
    n u / (1 - n u) mag, with n = n_terms + 8"""
    n = n_terms + 8
    return FACTOR * (n ** 0.5) * U * mag, n * U / (1 - n * U) * mag


def terms_of(p):
    """Additions behind one output element: K (+ K2), or M for a column sum"""
    return p["M"] if p["kind"] == "colsum" else p["K"] + p.get("K2", 0)
