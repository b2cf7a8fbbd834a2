"""CPU: what the cases of tests/lstm_forms_cases.py reach, proven from the resident launch plan itself (ops.lstm_plan ->
mmda_lstm_plan_describe: host code, no GPU, the quad form's block cap given instead of asked of a device): every case lands on the
form, waves per block, launch count and kernel instances it is meant for; together the cases reach every instance pick_kernel() can
return and every (form, waves per block, chunked or not) the plan can produce; their inputs have the rows that make an indexing error
O(1); and the two bf16-emulating oracles a PAIR case is held to can be told apart yet stay within the bound of each other."""
import ctypes as C
import itertools

import pytest
import torch

import lstm_forms_cases as lc
from mmda_amd import _lib, ops

CAPS = (240, 512)                                    # min(512, 240 * blocks per CU) at an occupancy of one and of three or four
# instances no case runs, and why
EXCLUDED = {
    "stamped debug instance": "runs only after mmda_debug_set_lstm_stamps() handed the library a stamp buffer (tools/ diagnostics)",
}


def test_every_case_lands_on_its_expect():
    bad = []
    for c in lc.CASES:
        for p in lc.passes_of(c):
            for cap in CAPS:
                bad += lc.plan_mismatch(c, p, lc.plan_of(c, p, cap))
    assert not bad, "\n".join(bad)


def test_workgroup_counts_of_the_descriptor_sets():
    for Hs, want in ((lc.P3, (108, 54, 30)), (lc.Q4, (188, 94, 50))):
        tiles = [(H + 15) // 16 for H in Hs]
        assert tuple(sum(2 * -(-2 * t // w) for t in tiles) for w in (1, 2, 4)) == want
    for c in lc.CASES:
        plan = lc.plan_of(c, "fwd", 240)
        assert plan["groups"] == -(-c["B"] // 32) and sum(plan["wg_per_desc"]) == plan["wg_per_group"]
        assert plan["launches"] == -(-plan["groups"] // max(1, 240 // plan["wg_per_group"])) or plan["form"] == "quad"
        assert plan["wg_per_group"] * plan["groups_per_launch"] <= (512 if plan["form"] == "quad" else 240)
        if c["gate_minor"] and c["switches"] == lc.DEFAULT and c["expect"]["form"] != "barrier":
            one_wave = sum(4 * t for t in [(H + 15) // 16 for H in c["Hs"]]) * plan["groups"]
            assert one_wave <= 240 or one_wave > 512, f"{c['name']}: quad or not would depend on the device's occupancy"


def test_plan_only_cases():
    assert not ops.lstm_plan([dict(H=336, cell="gru")], 21, 4, quad_cap=240)["ok"]
    assert not ops.lstm_plan([dict(H=300, cell="gru"), dict(H=321, cell="gru")], 21, 4, quad_cap=240)["ok"]
    assert ops.lstm_plan([dict(H=320, cell="gru")], 21, 4, quad_cap=240)["ok"]
    assert not ops.lstm_plan([dict(H=35)] * 5, 21, 4, quad_cap=240)["ok"]
    assert not ops.lstm_plan([dict(H=35, xchg=False)], 21, 4, quad_cap=240)["ok"]
    assert not ops.lstm_plan([dict(H=35, wpack_c=False)], 21, 4, backward=True, quad_cap=240)["ok"]
    gm = [dict(H=H, gate_minor=True) for H in lc.Q4]
    at240, at512 = ops.lstm_plan(gm, 37, 4, quad_cap=240), ops.lstm_plan(gm, 37, 4, quad_cap=512)
    assert (at240["form"], at240["wpb"]) == ("wave", 2) and (at512["form"], at512["wpb"]) == ("quad", 1)
    # ResidentPlan.pair_bwd sizes the LDS of every gate-minor LSTM backward at four waves per block; `pair` is what runs
    rt = ops.lstm_plan([dict(H=H, gate_minor=True, d_hseq=True, dg_bf16=True) for H in lc.Q4], 69, 4, backward=True, quad_cap=240)
    assert (rt["wpb"], rt["pair"], rt["kernel"]) == (4, False, "lstm_bwd_wave_kernel<20,true,LSTM,false>")
    # mixed d_hseq among the descriptors of a dg_bf16_only call: the run-time instance
    mix = [dict(H=H, gate_minor=True, d_hseq=bool(i), dg_bf16=True, dg_bf16_only=True) for i, H in enumerate(lc.P3)]
    assert ops.lstm_plan(mix, 133, 4, backward=True, quad_cap=240)["dhseq"] == "run-time"


# ------------------------------------------------------------------------------------------------ the sweep
_SIZES = (35, 74, 300, 320, 336, 512)
PAIR_INSTANCES = ("lstm_bwd_wave_kernel<20,true,LSTM,false,0,1,1>", "lstm_bwd_wave_kernel<20,true,LSTM,false,1,1,1>")   # PAIR = 1
_VARIANTS = (("fwd", 0), ("fwd_only", 0), ("bwd", 1), ("bwd16", 1), ("bwd16_nodh", 1))


def _sweep():
    """Every plan of: H = 1 .. 512 alone and every mix of up to four sizes of _SIZES, each cell, layout, pass variant, a few B, both
    switch values, both caps.  Yields (no_quad, plan struct)."""
    lib = _lib.load()
    plan = _lib.LstmPlan()
    mixes = [(H,) for H in range(1, 513)]
    mixes += [m for n in (2, 3, 4) for m in itertools.combinations_with_replacement(_SIZES, n)]
    for Hs in mixes:
        arr = (_lib.LstmDesc * len(Hs))()
        for d, H in zip(arr, Hs):
            d.H = H; d.xchg = 4096; d.wpack_c[0] = d.wpack_c[1] = 4096
        for cell, gm, (p, bwd) in itertools.product((0, 1), (0, 1), _VARIANTS):
            only = p in ("bwd16", "bwd16_nodh")
            for d in arr:
                d.cell, d.gate_minor, d.forward_only, d.dg_bf16_only = cell, gm, int(p == "fwd_only"), int(only)
                d.d_hseq = 4096 if p in ("bwd", "bwd16") else None
                d.dg_bf16 = 4096 if (only or (bwd and gm)) else None
            for B in ((21, 385) if len(Hs) == 1 else (21, 69, 133, 385)):
                for no_quad, cap in ((0, 240), (0, 512), (1, 240)):
                    assert lib.mmda_lstm_plan_describe(len(Hs), arr, B, 4, bwd, (C.c_int * 2)(no_quad, cap), C.byref(plan)) == 0
                    if plan.ok:
                        yield no_quad, plan


@pytest.fixture(scope="module")
def swept():
    names = ops.lstm_kernel_names()
    kernels, combos = set(), set()
    for no_quad, plan in _sweep():
        kernels.add(names[plan.kernel])
        if plan.form != 2:
            combos.add((ops.LSTM_FORMS[plan.form], plan.wpb, plan.launches > 1, bool(plan.gate_minor)))
        assert plan.pair == int(names[plan.kernel] in PAIR_INSTANCES)
    return kernels, combos


def test_cases_reach_every_instance_the_plan_can_return(swept):
    names = ops.lstm_kernel_names()
    assert len(names) == len(set(names)) == 26
    reached = {k for c in lc.CASES for k in c["expect"]["kernels"].values()}
    assert reached <= set(names) and set(EXCLUDED) <= set(names)
    assert not reached & set(EXCLUDED)
    left = set(names) - reached - set(EXCLUDED)
    assert not left, f"instances that no case runs and no exclusion explains: {sorted(left)}"
    # the sweep returns every instance but the excluded ones, so "unreachable" is shown, not assumed
    kernels, _ = swept
    assert kernels == set(names) - set(EXCLUDED)


def test_cases_reach_every_form_width_and_chunking_the_plan_can_produce(swept):
    _, combos = swept
    have = {(c["expect"]["form"], c["expect"]["wpb"], c["expect"]["launches"] > 1, c["gate_minor"]) for c in lc.CASES
            if c["expect"]["form"] != "quad"}
    assert combos - have == set(), f"(form, waves per block, chunked, gate_minor) with no case: {sorted(combos - have)}"
    assert {(f, w, ch) for f, w, ch, _ in combos} == {("wave", 1, False), ("wave", 2, False), ("wave", 4, False), ("wave", 4, True),
                                                     ("barrier", 4, False), ("barrier", 4, True)}


def test_input_recipe_of_every_case():
    for c in lc.CASES:
        B, T = c["B"], c["T"]
        lengths = lc.lengths_of(c)
        assert B % 4 != 0 and B % 32 != 0, c["name"]               # the cell stash's rounding to fours; a partial last group
        assert not torch.equal(lengths, torch.sort(lengths, descending=True).values) or B == 1
        for r0 in range(0, B, 32):
            grp = lengths[r0:r0 + 32]
            assert int(grp.max()) == T and int(grp.min()) >= 1, (c["name"], r0)
            assert len(grp) < 2 or int(grp.min()) == 1, (c["name"], r0)
        assert torch.equal(lengths, lc.lengths_of(c))
    assert {c["T"] for c in lc.CASES} == {2, 3, 4}


PAIR_CASES = [c for c in lc.CASES if any(c["expect"]["pair"].values())]


@pytest.mark.parametrize("c", PAIR_CASES, ids=[c["name"] for c in PAIR_CASES])
def test_pair_and_tile_oracles_differ_yet_stay_within_the_bound(c):
    """From the oracle alone: a case held to tile_partials=32 must be able to tell it from tile_partials=True (dX differs), and the
    two must be closer than the 1e-2 relative L2 the GPU test grants, or a correct kernel could not meet the bound."""
    inputs, lengths = lc.inputs_of(c["name"])
    # the largest hidden size of the set: the most tile pairs (the others follow the same code path)
    inp = inputs[max(range(len(inputs)), key=lambda i: inputs[i]["H"])]
    tile, pair = (lc.emul_reference(c, inp, lengths, tp)["grads"] for tp in (True, 32))
    for key in ("dh", "nodh"):
        a, b = tile[key]["dX"].double(), pair[key]["dX"].double()
        dist = float((a - b).norm() / a.norm())
        print(f"lstm-forms-oracle-distance {c['name']} H={inp['H']} {key}: relative L2 of dX, tile_partials 32 against True = {dist:.3e}")
        assert not torch.equal(a, b) and 0.0 < dist < 1e-2
