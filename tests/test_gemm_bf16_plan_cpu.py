"""CPU: the case table of tests/gemm_bf16_cases.py reaches what it says.  Everything here is read off the launch plan itself
(ops.gemm_bf16_plan -> mmda_gemm_bf16_plan_describe: host code, no GPU): every case lands on its intended kernel instance with its
intended k-slices, and the union of the cases covers, per instance, every slice length, residue, tile edge and epilogue pair that
test_gpu_gemm_bf16_edges.py claims to check.  Also: the error bound of that test's rounding family holds for a plain fp32 product."""
import pytest
import torch

import gemm_bf16_cases as gc
from mmda_amd import ops


def plan(case):
    return ops.gemm_bf16_plan([gc.plan_problem(p) for p in case["problems"]], case["switches"])


@pytest.fixture(scope="module")
def planned():
    """(case, problem, plan row, instance) of every problem of the table"""
    out = []
    for c in gc.CASES:
        rows, _ = plan(c)
        out += [(c, p, r, gc.instance_of(r, c["switches"])) for p, r in zip(c["problems"], rows)]
    return out


@pytest.mark.parametrize("case", gc.CASES, ids=[c["name"] for c in gc.CASES])
def test_case_lands_on_its_instance_and_slices(case):
    rows, launches = plan(case)
    classes = set()
    for p, r in zip(case["problems"], rows):
        e = p["expect"]
        got = dict(inst=gc.instance_of(r, case["switches"]), sk=r["sk"], per=r["per"], last=r["last"])
        assert got == e, (case["name"], p["M"], p["N"], p["K"], got, e)
        classes.add(r["cls"])
    assert launches == len(classes) and sorted({r["launch"] for r in rows}) == list(range(launches))
    env_switches = {k for k, v in gc.ENV.items()}
    assert case["switches"] in env_switches


def test_every_instance_and_the_reduce_launch_are_reached(planned):
    reached = {inst for _, _, _, inst in planned}
    assert reached == set(gc.NS)
    for inst in gc.NS:                                  # a split problem per instance that can have one: the reduce launch behind it
        if not inst.startswith("reg128"):
            assert any(i == inst and r["sk"] > 1 for _, _, r, i in planned), inst


def _tail(p):
    K = p["K"]
    if K % 64 == 0:
        return "full"
    if p["form"] == "nt":
        return "ragged" if K % 8 else None              # ragged: the 8-padded depth is longer than K
    return {1: "k1", 63: "k63"}.get(K % 64)


def test_unsplit_slice_lengths_full_and_ragged_per_instance(planned):
    for inst in gc.NS:
        form_sets = {}
        alone = gc.INSTANCES[inst][1]                   # the form that reaches a register-staged instance without a companion problem
        for c, p, r, i in planned:
            if i == inst and r["sk"] == 1 and c["epi"] is None and p["M"] != 8192 and alone in (None, p["form"]):
                form_sets.setdefault(p["form"], set()).add((r["per"], _tail(p)))
        assert form_sets, inst
        for form, have in form_sets.items():
            tails = ("full", "ragged") if form == "nt" else ("full", "k1", "k63")
            want = {(L, t) for t in tails for L in gc.REQUIRED_L[inst]["full" if t == "full" else "ragged"]}
            assert want <= have, (inst, form, sorted(want - have))
    # a register-staged instance is reached by one form only; the DMA instances by both
    assert all({"nt", "tn"} == {p["form"] for _, p, r, i in planned if i == inst and r["sk"] == 1 and p["M"] != 8192}
               for inst in gc.NS if inst.startswith("dma"))


def test_split_slices_fall_in_every_residue_and_the_last_one_is_shorter(planned):
    for inst, ns in gc.NS.items():
        split = [(p, r) for _, p, r, i in planned if i == inst and r["sk"] > 1]
        if inst.startswith("reg128"):
            assert not split                            # unreachable at any affordable size: see test_reg128_split_is_out_of_reach
            continue
        forms = {p["form"] for p, _ in split}
        assert forms == ({"nt", "tn"} if inst.startswith("dma") else {"nt"} if inst == "reg64" else {"tn"}), inst
        for form in forms:
            mine = [r for p, r in split if p["form"] == form]
            lengths = {r["per"] for r in mine} | {r["last"] for r in mine}
            assert {L % ns for L in lengths} == set(range(ns)), (inst, form, sorted(lengths))
            assert any(r["last"] < r["per"] for r in mine), (inst, form)
            assert all(r["per"] * (r["sk"] - 1) + r["last"] == (p["K"] + 63) // 64 for p, r in split)


def test_reg128_split_is_out_of_reach():
    """A register-staged split needs >= 128 k-tiles and slabs of at most 24 MB: with the >= 512 tiles of 128 x 128 that make a problem
    Reg128 that leaves outputs a few rows high and >= 65 000 wide (an operand of a gigabyte).  An output of the table's size stays whole."""
    for acc in (False, True):
        rows, _ = ops.gemm_bf16_plan([dict(M=2900, N=2890, K=8256, lda=8264, ldb=8264, accumulate=acc)])
        assert rows[0]["cls"] == "Reg128" and rows[0]["sk"] == 1
    rows, _ = ops.gemm_bf16_plan([dict(M=8, N=65409, K=8256, lda=8264, ldb=8264, accumulate=True)])
    assert rows[0]["cls"] == "Reg128" and rows[0]["sk"] == 2


def test_output_tile_edges_per_instance(planned):
    for inst in gc.NS:
        mine = [(p, r) for _, p, r, i in planned if i == inst and p["M"] != 8192]
        tm, tn = (256, 128) if inst == "dma3_256" else (64, 64) if inst.startswith("reg64") else (128, 128)
        assert any(p["M"] % tm == 1 for p, _ in mine) and any(p["M"] % tm == tm - 1 for p, _ in mine), inst
        assert any(p["N"] % tn == 1 for p, _ in mine) and any(p["N"] % tn == tn - 1 for p, _ in mine), inst
        assert any(p["N"] % 4 for p, _ in mine) and any(p["N"] % 4 == 0 and gc.layout(p)["ldc"] % 4 == 0 for p, _ in mine), inst
        # the bias gradient's ones-column alone in an extra column tile, and in the last column of a tile
        assert any(p.get("bias_grad") and p["N"] % tn == 0 and r["tx"] == p["N"] // tn + 1 for p, r in mine), inst
        assert any(p.get("bias_grad") and p["N"] % tn == tn - 1 and r["tx"] == (p["N"] + 1) // tn for p, r in mine), inst
        # tn column windows: off the 16-byte grid (register-staged classes only), on it and off zero (DMA classes)
        tn_off16 = [p for p, _ in mine if p["form"] == "tn" and (2 * p.get("a0", 0)) % 16]
        tn_on16 = [p for p, _ in mine if p["form"] == "tn" and p.get("a0", 0) and (2 * p["a0"]) % 16 == 0 and (2 * p["b0"]) % 16 == 0]
        if inst.endswith("_mixed"):
            assert tn_off16 and any(p["a0"] == 140 and p["b0"] == 40 for p in tn_off16), inst
        if inst.startswith("dma"):
            assert tn_on16 and not tn_off16, inst
    # grouping: an nt problem on the mixed instance
    for inst in ("reg64_mixed", "reg128_mixed"):
        assert any(i == inst and p["form"] == "nt" for _, p, _, i in planned), inst
    # both forms of the reduce launch: 16-byte (N, ldc multiples of 4) and scalar
    split = [p for _, p, r, _ in planned if r["sk"] > 1]
    assert any(p["N"] % 4 == 0 and gc.layout(p)["ldc"] % 4 == 0 for p in split) and any(p["N"] % 4 for p in split)
    assert any(p["N"] % 4 == 0 and gc.layout(p)["ldc"] % 4 for p in split)


def test_epilogue_matrix_is_complete(planned):
    impl_of = {"reg64": "epi64", "reg64_mixed": "epi64", "reg128": "epi128_reg", "reg128_mixed": "epi128_reg", "dma2_128": "epi128_dma",
               "dma3_128": "epi128_dma", "dma3_256": "epi256_dma"}
    pairs = set()
    for c, p, r, inst in planned:
        if c["epi"] is None or p["M"] == 8192:
            continue
        feature, impl = c["epi"]
        assert impl == ("reduce" if r["sk"] > 1 else impl_of[inst]), c["name"]
        want = gc._feat(feature)
        assert all(p.get(k) == v for k, v in want.items()), c["name"]
        assert not any(p.get(k) for k in ("bias", "bias2", "bias_grad", "bias_grad2", "accumulate", "perm_n_H", "perm_m_H") if k not in want)
        if feature.startswith("perm"):
            assert (p["N"] if feature == "perm_n" else p["M"]) % (4 * gc.H) == 0 and (4 * gc.H) % 64
        if gc.layout(p)["ldc"] % 4 == 0:                 # the odd-ldc twins come on top
            pairs.add(c["epi"])
    assert pairs == {(f, i) for f in gc.FEATURES for i in gc.EPILOGUES}


def test_poison_runs_on_every_ragged_and_off_grid_window_case(planned):
    for c, p, r, _ in planned:
        ragged = p["K"] % 64 != 0 and c["epi"] is None and p["M"] != 8192
        window = p["form"] == "tn" and (p.get("a0", 0) or p.get("b0", 0))
        if ragged or window:
            assert p.get("poison"), c["name"]


def test_planner_facts_the_suite_relies_on():
    def one(M, N, K, switches=None, **kw):
        Kp = (K + 7) // 8 * 8
        rows, _ = ops.gemm_bf16_plan([dict(M=M, N=N, K=K, lda=Kp, ldb=Kp, **kw)], switches)
        return rows[0]
    assert one(1600, 2400, 300)["cls"] == "Reg64"
    assert one(8320, 2400, 300)["cls"] == "Dma128"
    assert one(6400, 2400, 300)["cls"] == "Reg128"                       # B = 128, T = 50 of the product
    assert one(3200, 2400, 300)["cls"] == "Reg64" and one(3072, 2400, 300)["cls"] == "Reg64"     # B = 64 / T = 50, B = 128 / T = 24
    for shape in ((8200, 600, 1100), (8200, 300, 2400)):
        assert one(*shape)["cls"] == "Dma128" and one(*shape, switches=gc.TALL)["cls"] == "Dma256"
    assert one(8320, 2400, 300, switches=gc.TALL)["cls"] == "Dma128"     # the tall class: K >= 1024 only
    assert one(8320, 2400, 300, switches=(0, 2, 8192, 0))["cls"] == "Reg128"
    # problems of a DMA call under 96 rows or columns stay register-staged
    assert one(8320, 95, 300)["cls"] == "Reg64" and one(8320, 96, 300)["cls"] == "Dma128" and one(8320, 95, 300, bias_grad=True)["cls"] == "Dma128"
    rows, _ = ops.gemm_bf16_plan([dict(M=8192, N=8, K=8, lda=8, ldb=8), dict(M=95, N=300, K=300, lda=304, ldb=304),
                                  dict(M=96, N=300, K=300, lda=304, ldb=304)])
    assert [r["cls"] for r in rows] == ["Reg64", "Reg64", "Dma128"]
    # tn: a window off the 16-byte grid keeps a problem of a DMA call register-staged
    tn = dict(M=256, N=96, K=8256, tn=True, lda=400, ldb=136, accumulate=True)
    rows, _ = ops.gemm_bf16_plan([dict(tn, A_addr=(1 << 20) + 2 * 140, B_addr=(1 << 20) + 2 * 40), dict(tn)])
    assert [r["cls"] for r in rows] == ["Reg64", "Dma128"]
    # what tests/test_gpu_ops.py says about its split-K shapes
    rows, _ = ops.gemm_bf16_plan([dict(M=2400, N=300, K=1600, tn=True, lda=2400, ldb=304, accumulate=True, bias_grad=True)])
    assert (rows[0]["cls"], rows[0]["sk"]) == ("Reg64", 1)
    rows, _ = ops.gemm_bf16_plan([dict(M=2400, N=300, K=12800, tn=True, lda=2400, ldb=304, accumulate=True, bias_grad=True),
                                  dict(M=1200, N=300, K=12800, tn=True, lda=2400, ldb=600, A_addr=(1 << 20) + 2 * 1200,
                                       B_addr=(1 << 20) + 2 * 300, accumulate=True)])
    assert [(r["cls"], r["mixed"], r["sk"]) for r in rows] == [("Dma128", False, 9), ("Reg64", True, 10)]
    rows, n = ops.gemm_bf16_plan([dict(M=0, N=5, K=8, lda=8, ldb=8)])
    assert rows[0]["cls"] is None and n == 0
    with pytest.raises(Exception):
        ops.gemm_bf16_plan([dict(M=16, N=16, K=30, lda=24, ldb=24)])      # K beyond the padded leading dimension


def _sample_rows(M):
    """<= 48 logical rows of a tall problem, both ends included (the bound is a property of the arithmetic, not of the row)"""
    return None if M <= 300 else sorted(set(torch.linspace(0, M - 1, 48).long().tolist()))


@pytest.mark.parametrize("case", gc.CASES, ids=[c["name"] for c in gc.CASES])
def test_fp32_reference_meets_the_working_bar(case):
    """Family (b)'s working bar 8 sqrt(n) u mag (and the hard ceiling n u / (1 - n u) mag) hold for a plain fp32 evaluation of the
    same bf16-rounded values: the bar asks nothing that fp32 arithmetic itself does not deliver."""
    worst = 0.0
    for k, p in enumerate(case["problems"]):
        if p["M"] == 8192:
            continue
        d = gc.make_data(p, "b", gc.seed_of(case, k, "b"))
        rows = _sample_rows(p["M"])
        C, mag, grads, out_rows = gc.reference(p, d, rows=rows)
        m_idx = torch.arange(p["M"]) if rows is None else torch.as_tensor(rows)
        A32, B32 = d["A"].float()[m_idx], d["B"].float()
        got = torch.tensor(p.get("alpha", 1.0)) * (A32 @ B32.t())
        pn = gc.gate_perm(p["N"]) if p.get("perm_n_H") else torch.arange(p["N"])
        for b in ("bias", "bias2"):
            if d[b] is not None:
                got = got + d[b][pn]
        if d["C0"] is not None:
            got = got + d["C0"][out_rows]
        if rows is None:
            tmp = torch.empty_like(got); tmp[out_rows] = got; got = tmp
        work, ceil = gc.bars(p["K"], mag, p["expect"]["inst"])
        err = (got.double() - C).abs()
        assert bool((err <= work).all()) and bool((err <= ceil).all()), case["name"]
        worst = max(worst, float((err / work.clamp_min(1e-300)).max()))
        for name, (g, gm) in grads.items():
            got_g = A32.sum(1) + d[name + "0"][out_rows]
            if rows is None:
                tmp = torch.empty_like(got_g); tmp[out_rows] = got_g; got_g = tmp
            work, ceil = gc.bars(p["K"], gm, p["expect"]["inst"])
            assert bool(((got_g.double() - g).abs() <= torch.minimum(work, ceil)).all()), (case["name"], name)
    assert worst <= 1.0
