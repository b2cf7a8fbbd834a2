"""CPU: the case table of tests/gemm_f32_cases.py reaches what it says.  Everything about mmda_gemm / mmda_gemm_grouped is read off the
launch plan itself (ops.gemm_plan -> mmda_gemm_plan_describe: host code, no GPU): every case lands on its intended kernel instance with
its intended k-slices and reduce form, and the union of the cases covers every instance, slice length, reduce form, epilogue feature,
128-tile disqualifier and planner threshold that test_gpu_gemm_f32_edges.py claims to check.  mmda_gemm_skinny has no host plan: its
form rule is checked against the buffers the cases build, and its argument checks against the entry point (no launch happens).  Also
the premises of the exact and the poisoned input families."""
import ctypes as C

import pytest
import torch

import gemm_f32_cases as gc
from mmda_amd import _lib, ops

GEMM_CASES = [c for c in gc.CASES if c["call"] in ("gemm", "grouped")]
SKINNY_CASES = [c for c in gc.CASES if c["call"] == "skinny"]


def plan(case):
    return ops.gemm_plan([gc.gemm_args(p) for p in case["problems"]], grouped=case["call"] == "grouped")


@pytest.fixture(scope="module")
def planned():
    """(case, problem, plan row, instance) of every mmda_gemm problem of the table"""
    out = []
    for c in GEMM_CASES:
        rows, _ = plan(c)
        out += [(c, p, r, gc.instance_of(r) if r["cls"] else None) for p, r in zip(c["problems"], rows)]
    return out


@pytest.mark.parametrize("case", GEMM_CASES, ids=[c["name"] for c in GEMM_CASES])
def test_case_lands_on_its_instance_slices_and_reduce_form(case):
    rows, launches = plan(case)
    for p, r in zip(case["problems"], rows):
        e = p["expect"]
        if e["inst"] is None:
            assert r["cls"] is None and r["launch"] == -1
            continue
        got = dict(inst=gc.instance_of(r), sk=r["sk"], per=r["per"], last=r["last"], reduce=r["reduce"])
        assert got == e, (case["name"], p["M"], p["N"], p["K"], got, e)
        assert r["per"] * (r["sk"] - 1) + r["last"] == -(-p["K"] // 32) and 0 < r["last"] <= r["per"]
        assert r["blocks"] == r["tx"] * r["ty"] * p["batch"] * r["sk"] and r["ldn"] == p["N"] + bool(p.get("bias_grad"))
    if case["call"] == "grouped":
        assert launches == -(-len(case["problems"]) // 16)
        assert [r["launch"] for r in rows if r["cls"]] == [k // 16 for k, r in enumerate(rows) if r["cls"]]


def test_every_instance_is_reached_split_and_unsplit(planned):
    assert {i for _, _, _, i in planned if i} == set(gc.GEMM_INSTANCES)
    for inst in gc.GEMM_INSTANCES:
        assert any(i == inst and r["sk"] > 1 for _, _, r, i in planned), inst
        assert any(i == inst and r["sk"] == 1 for _, _, r, i in planned), inst
    forms = {(i, p["form"]) for _, p, _, i in planned if i and i.split("/")[1].startswith("PF")}
    assert forms == {(m + "/" + pf, f) for m in ("f32", "bf16") for pf in ("PF1", "PF4") for f in gc.FORMS}      # transA && transB included


def _tail(K):
    return "full" if K % 32 == 0 else K % 32


def test_unsplit_slice_lengths_full_and_ragged_per_instance(planned):
    want = {"PF4": (1, 2, 3, 4), "PF1": (1, 2, 4, 5, 6, 7)}                   # PF1 below 5 k-tiles: only past 1024 blocks
    for mode in ("f32", "bf16"):
        for pf, lengths in want.items():
            have = {(r["per"], _tail(p["K"])) for _, p, r, i in planned if i == f"{mode}/{pf}" and r["sk"] == 1}
            assert {(L, "full") for L in lengths} <= have, (mode, pf, have)
            assert {(L, "ragged") for L in lengths} <= {(L, "ragged") for L, t in have if t != "full"}, (mode, pf)
        walk = {(r["per"], p["form"], _tail(p["K"])) for c, p, r, i in planned if c.get("walk") and p["mode"] == mode and p["batch"] == 1}
        assert walk == {(L, f, t) for L in range(1, 7) for f in gc.FORMS for t in ("full", 1, 3, 31)}
    for form in gc.FORMS:                                                    # the 128 tile: one and two k-tiles, full and ragged, and a split walk
        have = {(r["per"], r["sk"], _tail(p["K"])) for _, p, r, i in planned if i == "t128/" + form}
        assert {(1, 1, 4), (1, 1, 28), (1, 1, "full"), (2, 1, 4), (2, 1, "full"), (2, 5, 12), (2, 16, "full")} <= have, (form, have)
        shapes = {(p["M"], p["N"]) for c, p, _, i in planned if i == "t128/" + form and c.get("walk128")}
        assert shapes == {(128, 128), (132, 252), (260, 132)}


def test_tile_edges_and_the_ones_column_per_instance(planned):
    for inst in gc.GEMM_INSTANCES[:4]:
        mine = [(p, r) for _, p, r, i in planned if i == inst]
        assert set(gc.TILE_EDGES) <= {(p["M"], p["N"]) for p, _ in mine}, inst
        bg = [(p, r) for p, r in mine if p.get("bias_grad")]
        assert any(p["N"] % 64 == 0 and r["tx"] == p["N"] // 64 + 1 for p, r in bg), inst      # alone in a column tile of its own
        assert any(p["N"] % 64 == 63 and r["tx"] == (p["N"] + 1) // 64 for p, r in bg), inst   # the last column inside a tile
        if inst.endswith("PF4"):
            assert any(p.get("bias_grad2") and p["batch"] == 3 for p, _ in bg), inst


def test_split_slices_and_both_reduce_forms(planned):
    for mode in ("f32", "bf16"):
        one = {(-(-p["K"] // 32), r["sk"], r["per"], r["last"]) for _, p, r, i in planned if p["mode"] == mode and r["cls"] in ("Tile64", "Tile64Tiny")
               and r["tx"] * r["ty"] * p["batch"] == 1}
        assert {(7, 1, 7, 7), (8, 4, 2, 2), (9, 3, 3, 3), (10, 5, 2, 2), (131, 44, 3, 2)} <= one, mode
        assert any(i == mode + "/PF1" and r["sk"] > 1 and r["per"] >= 5 and r["last"] < r["per"] for _, _, r, i in planned), mode
        assert any(i == mode + "/PF4" and r["sk"] > 1 and r["last"] < r["per"] for _, _, r, i in planned), mode
        for form in ("vector", "scalar"):
            assert any(p["mode"] == mode and r["reduce"] == form for _, p, r, _ in planned), (mode, form)
        assert any(p["mode"] == mode and p["batch"] == 3 and r["reduce"] == "scalar" and p.get("bias") for _, p, r, _ in planned)
        assert any(p["mode"] == mode and p["batch"] == 3 and r["reduce"] == "scalar" and p.get("bias_grad") for _, p, r, _ in planned)
    # the 16-byte form, and the scalar one by each single disqualifier: taking the disqualifier away gives the 16-byte form back
    why = {c["reduce_why"]: (p, r) for c, p, r, _ in planned if c.get("reduce_why")}
    assert set(why) == {"none", "N", "ldc", "bias_grad", "batch", "C"}
    assert why["none"][1]["reduce"] == "vector" and all(r["reduce"] == "scalar" for k, (_, r) in why.items() if k != "none")
    undo = {"N": dict(N=64, ldc_pad=4), "ldc": dict(ldc_pad=4), "bias_grad": dict(bias_grad=False), "batch": dict(batch=1), "C": dict(c_off=0)}
    for k, change in undo.items():
        rows, _ = ops.gemm_plan([gc.gemm_args(dict(why[k][0], **change))])
        assert rows[0]["reduce"] == "vector" and rows[0]["sk"] == why[k][1]["sk"], k
    # a grouped slot whose slab starts off the 16-byte grid: scalar for the shape that is vector at offset 0
    g = [(p, r) for c, p, r, _ in planned if c["name"] == "grouped-17-problems"]
    (p2, r2), (p5, r5) = g[2], g[5]
    assert (p2["M"], p2["N"], p2["K"]) == (p5["M"], p5["N"], p5["K"]) and gc.gemm_layout(p2)["ldc"] == gc.gemm_layout(p5)["ldc"]
    assert r2["reduce"] == "vector" and r2["slab_off"] == 0 and r5["reduce"] == "scalar" and r5["slab_off"] % 4 != 0
    # the grouped launch: both ends of the prefix search are slots of one block, an empty problem has no slot
    assert g[0][1]["blocks"] == 1 and g[15][1]["blocks"] == 1 and g[16][1]["launch"] == 1 and g[4][1]["cls"] is None
    assert {gc.instance_of(r) for _, r in g if r["cls"] and r["sk"] > 1} == {"group/f32", "group/bf16"}
    assert any(p.get("bias_grad") and p.get("accumulate") and r["sk"] > 1 for p, r in g)


def test_epilogue_matrix_is_complete(planned):
    direct, reduce = set(), set()
    for c, p, r, inst in planned:
        if not c.get("epi"):
            continue
        f, impl = c["epi"]
        assert (r["sk"] > 1) == (impl == "reduce"), c["name"]
        (reduce if impl == "reduce" else direct).add((inst, f) if impl == "direct" else (p["mode"], r["reduce"], f))
    assert direct == {(m + "/" + pf, f) for m in ("f32", "bf16") for pf in ("PF1", "PF4") for f in gc.EPI_FEATURES}
    assert reduce == {(m, form, f) for m in ("f32", "bf16") for form in ("vector", "scalar") for f in gc.SPLIT_FEATURES}
    # the features the reduce launch does not know keep a problem whole, at the shape that splits without them
    refused = {(p["mode"], c["refused"]): (p, r) for c, p, r, _ in planned if c.get("refused")}
    assert set(refused) == {(m, f) for m in ("f32", "bf16") for f in ("relu", "drop", "gate")}
    for (mode, f), (p, r) in refused.items():
        assert r["sk"] == 1
        bare = {k: v for k, v in p.items() if k not in ("act", "drop", "gate")}
        assert ops.gemm_plan([gc.gemm_args(bare)])[0][0]["sk"] == 4


def test_each_128_tile_disqualifier(planned):
    refused = {c["refused128"]: (p, r) for c, p, r, _ in planned if c.get("refused128")}
    assert set(refused) == {"M127", "N127", "K30", "lda", "A-offset", "tn-M", "nn-N", "bias_grad", "A2", "gather", "act"}
    for why, (p, r) in refused.items():
        assert r["cls"] in ("Tile64", "Tile64Tiny"), why
    # each is the only one: the nearest problem without it takes the 128 tile
    fix = {"M127": dict(M=128), "N127": dict(N=128), "K30": dict(K=32, lda_pad=0, ldb_pad=0),"lda": dict(lda_pad=4), "A-offset": dict(a_off=4), "tn-M": dict(M=128, lda_pad=4),
           "nn-N": dict(N=128, ldb_pad=4), "bias_grad": dict(bias_grad=False), "A2": dict(A2=False), "gather": dict(gather=False), "act": dict(act=None)}
    for why, change in fix.items():
        rows, _ = ops.gemm_plan([gc.gemm_args(dict(refused[why][0], **change))])
        assert rows[0]["cls"] == "Tile128", why
    p = gc.G("bf16", "nt", 128, 128, 36, "t128", lda_pad=4, ldb_pad=4, ldc_pad=4)
    for change in (dict(mode="f32"), dict(drop=True), dict(gate=True), dict(b_off=2), dict(ldb_pad=2)):
        assert ops.gemm_plan([gc.gemm_args(dict(p, **change))])[0][0]["cls"] != "Tile128", change


def test_planner_thresholds_from_both_sides():
    def one(M, N, K, **kw):
        return ops.gemm_plan([gc.gemm_args(gc.G("f32", "nt", M, N, K, "PF1", **kw))])[0][0]
    assert one(3, 3, 224)["sk"] == 1 and one(3, 3, 225)["sk"] == 4                                # nk >= 8
    assert one(3, 3, 256, batch=256)["sk"] == 3 and one(3, 3, 256, batch=257)["sk"] == 1          # SPLIT_MAX_TILES
    assert one(1024, 1024, 256)["sk"] == 3 and one(1024, 1088, 256)["sk"] == 1
    assert one(3, 3, 128)["cls"] == "Tile64Tiny" and one(3, 3, 129)["cls"] == "Tile64"            # <= 4 k-tiles per block
    assert one(3, 3, 32, batch=1024)["cls"] == "Tile64Tiny" and one(3, 3, 32, batch=1025)["cls"] == "Tile64"     # <= 1024 blocks
    r = one(3, 3, 256, batch=256)
    assert (r["blocks"], r["per"], r["cls"]) == (768, 3, "Tile64Tiny")
    r = one(3, 3, 512, batch=256)                                                                  # 16 k-tiles in 3 slices of 6
    assert (r["sk"], r["per"], r["last"], r["cls"]) == (3, 6, 4, "Tile64")
    assert one(0, 3, 32)["cls"] is None and one(3, 3, 32, batch=0)["cls"] is None
    with pytest.raises(Exception):
        one(3, 3, 0)
    with pytest.raises(Exception):
        ops.gemm_plan([gc.gemm_args(gc.G("f32", "nt", 3, 3, 32, "PF4", bias_grad=True))])          # the bias gradient is tn only
    with pytest.raises(Exception):
        ops.gemm_plan([gc.gemm_args(gc.G("f32", "tn", 3, 3, 32, "PF4", gather=True))])


def kernel_slices(nk, sk):
    """[kt0, kt1) of every slice as gemm_body / gemm128_bf16_kernel compute them from (K, splitk)"""
    per = -(-nk // sk)
    return [(sp * per, min(nk, sp * per + per)) for sp in range(sk)]


def test_slice_arithmetic_of_host_and_kernels_agree():
    """The host's slice count (splitk_slices) and the kernels' (per, kt0, nk): for every k-tile count up to 300 and every requested
    slice count up to 64, no slice is empty and the slices tile [0, nk) exactly; where a request is reachable through the planner
    (ceil(768 / tiles) for some tile count, capped by nk / 2 and 64), the plan's sk / per / last are those numbers."""
    for nk in range(1, 301):
        for req in range(1, 65):
            per = -(-nk // req)
            sk = -(-nk // per)                               # splitk_slices(nk, req)
            sl = kernel_slices(nk, sk)
            assert all(a < b for a, b in sl) and sl[0][0] == 0 and sl[-1][1] == nk and all(sl[i][1] == sl[i + 1][0] for i in range(sk - 1))
            assert -(-nk // sk) == per                       # the kernel's slice length is the host's
    batches = sorted({b for b in range(1, 257)}, key=lambda b: -(-768 // b))
    seen = set()
    for nk in range(8, 301):
        probs = [gc.G("f32", "nt", 3, 3, 32 * nk - 7, "PF1", batch=b) for b in batches]
        rows, _ = ops.gemm_plan([gc.gemm_args(p) for p in probs])
        for b, r in zip(batches, rows):
            req = min(-(-768 // b), nk // 2, 64)
            per = -(-nk // req)
            sl = kernel_slices(nk, r["sk"])
            assert (r["sk"], r["per"], r["last"]) == (-(-nk // per), per, sl[-1][1] - sl[-1][0]), (nk, b, r)
            seen.add(req)
    assert set(range(3, 28)) <= seen and 64 in seen


# ------------------------------------------------------------------------------------------------ skinny
def test_skinny_cases_cover_the_prefetch_ring_the_forms_and_the_epilogue():
    walk = [c["problems"][0] for c in SKINNY_CASES if c.get("walk")]
    for tb in (True, False):
        have = {(-(-p["K"] // 16), p["K"] % 16) for p in walk if p["tb"] == tb}
        assert have == {(n, t) for n in gc.SKINNY_CHUNKS for t in (0, 4, 5)}
        forms = {("nt" if tb else "nn", p["expect"]["form"]) for c in SKINNY_CASES for p in c["problems"] if p["tb"] == tb}
        assert forms == {("nt" if tb else "nn", "vec"), ("nt" if tb else "nn", "scalar")}
        pairs = {(p["expect"]["form"], p["expect"]["second"]) for c in SKINNY_CASES for p in c["problems"] if p["tb"] == tb and p.get("K2")}
        assert pairs == {(a, b) for a in ("vec", "scalar") for b in ("vec", "scalar")}
        assert {(p["M"], p["N"], p["expect"]["form"]) for c in SKINNY_CASES for p in c["problems"] if p["tb"] == tb} >= \
            {(M, N, f) for M, N in gc.SKINNY_SHAPES for f in ("vec", "scalar")}
        assert {c["lost"] for c in SKINNY_CASES if c.get("lost") and c["problems"][0]["tb"] == tb} == {"A", "lda", "K", "A2", "B", "ldb"}
        epi = {(c["epi"], c["problems"][0]["expect"]["form"]) for c in SKINNY_CASES if c.get("epi") and c["problems"][0]["tb"] == tb}
        assert epi == {(f, v) for f in ("alpha", "alpha0", "bias", "accumulate", "relu", "drop", "gate", "dsig", "A2", "C2", "C2full", "all")
                       for v in ("vec", "scalar")}
    nine = gc.BY_NAME["skinny-nine-problems"]["problems"]
    assert len(nine) == 9 and any(p["M"] == 0 for p in nine[:8])
    assert {8 * 16 * 4 * r + t for r in (1, 2) for t in (0,)} == {512, 1024}      # one and two rounds of the ring: 32 and 64 chunks of 16


@pytest.mark.parametrize("case", SKINNY_CASES, ids=[c["name"] for c in SKINNY_CASES])
def test_skinny_form_rule_on_the_buffers_the_case_builds(case):
    for k, p in enumerate(case["problems"]):
        d = gc.make_skinny(p, "a", gc.seed_of(case, k, "a"))
        addr = {n: d[n + "buf"].flat.data_ptr() for n in ("A", "A2", "B", "A_2nd", "B_2nd") if d.get(n + "buf") is not None}
        assert all(a % 16 == 0 for a in addr.values())                         # torch's allocations; the offsets decide
        assert gc.skinny_forms(p, addr) == (p["expect"]["form"], p["expect"]["second"]), case["name"]
        assert gc.skinny_forms(p) == gc.skinny_forms(p, addr)
        lay = d["lay"]
        assert lay["lda"] >= p["K"] and lay["ldb"] >= (p["K"] if p["tb"] else p["N"]) and lay["ldc2"] != lay["ldc"] and lay["ldgate"] > p["N"]


def test_skinny_argument_checks_return_einval():
    lib = _lib.load()
    ok = gc.S(33, 17, 40, True, "vec")

    def rc(p, **fields):
        g = gc.skinny_args(p)
        for k, v in fields.items():
            setattr(g, k, v)
        return lib.mmda_gemm_skinny(C.byref(g), 1, None)

    lay = gc.skinny_layout(ok)
    assert lay["lda"] >= 40
    for bad in (dict(lda=39), dict(ldb=39), dict(ldc=16), dict(K=0), dict(K=-1), dict(act=-1), dict(act=_lib.ACT["prelu"]), dict(A=None),
                dict(M=-1), dict(K2=8, A_2nd=None), dict(K2=8, A_2nd=gc.FAKE, B_2nd=gc.FAKE, lda_2nd=7, ldb_2nd=8)):
        assert rc(ok, **bad) == -1, bad
    assert rc(gc.S(33, 17, 40, False, "vec"), ldb=16) == -1                    # transB = 0: ldb counts columns
    c2 = gc.S(33, 17, 40, True, "vec", C2=True)
    for bad in (dict(ldc2=16), dict(bias=gc.FAKE), dict(act=_lib.ACT["relu"]), dict(drop_p=0.5), dict(gate=gc.FAKE)):
        assert rc(c2, **bad) == -1, bad
    assert lib.mmda_gemm_skinny(None, 1, None) == -1


# ------------------------------------------------------------------------------------------------ the input families
def _make(case, k, p, family):
    make = {"gemm": gc.make_gemm, "skinny": gc.make_skinny, "colsum": gc.make_colsum}[p["kind"]]
    return make(p, family, gc.seed_of(case, k, family))


def _ref(p, d):
    if p["kind"] == "gemm":
        C_, _, grads = gc.ref_gemm(p, d)
        return [C_] + [g for g, _ in grads.values()]
    if p["kind"] == "skinny":
        C_, _, C2, _ = gc.ref_skinny(p, d)
        return [C_] + ([C2] if C2 is not None else [])
    return [v for v, _ in gc.ref_colsum(p, d).values()]


def test_exact_family_stays_below_2_to_the_24():
    worst = 0
    for c in gc.CASES:
        if "a" in gc.families_of(c):
            for p in c["problems"]:
                worst = max(worst, gc.exact_bound(p))
    assert worst < 2 ** 24, worst
    assert max(p["K"] for c in gc.CASES for p in c["problems"] if "K" in p) <= 4200


@pytest.mark.parametrize("case", gc.CASES, ids=[c["name"] for c in gc.CASES])
def test_poison_family_is_the_exact_family_inside_the_windows(case):
    if "c" not in gc.families_of(case):
        return
    for k, p in enumerate(case["problems"]):
        a, c = _make(case, k, p, "a"), _make(case, k, p, "c")
        bufs = [n for n, v in c.items() if isinstance(v, gc.Buf) and not n.startswith("C")]
        assert bufs
        for n in bufs:
            w = c[n].window()
            assert not bool(torch.isnan(w).any()) and torch.equal(w, a[n].window()), (case["name"], n)
            assert bool(torch.isnan(c[n].flat[c[n].outside()]).all()), (case["name"], n)
        if p.get("gather"):
            assert c["gather"].numel() == p["M"] + 8 and bool((c["gather"][p["M"]:] == gc.BAD_ID).all()) and int(c["gather"][:p["M"]].max()) < 9
        for x, y in zip(_ref(p, a), _ref(p, c)):
            assert not bool(torch.isnan(y).any()) and torch.equal(x, y) and torch.equal(x, x.float().double()), case["name"]
