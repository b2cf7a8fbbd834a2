"""CPU: the plan of a training step (plan_step, csrc/step_plan.hip) seen through mmda_misa_plan_describe / ops.step_plan: host code, no
GPU, no workspace, the switches given as an argument.

tests/golden/step_plan_cases.json was recorded from the commit BEFORE plan_step became a pure function (its plan_step(handle), reached
through a throw-away probe that bound a host buffer as the workspace and set the four request fields the handle then had): `rows` is a
thinned sweep over precision, B, T, cell, losses, sizes, every setting the plan reads and the request; `switch_rows` is a small sweep
per non-default value of each of the thirteen switches, recorded with the variable in the environment of a fresh process each.  Every
row is the inputs and that commit's plan as integers (the booleans as one bit mask in the order of `plan`).

Not in the sweep: the deferred table (mmda_misa_set_embed_deferred clears the caller's device buffer, a device call), so
StepPlan::embed_deferred is 0 in every row; it is a copy of its input.  `fused` did not exist in that commit's plan: it must equal the
request's."""
import ctypes as C
import json
import os

import pytest

from mmda_amd import _lib, ops

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_plan_cases.json")
INPUTS = ("bf16", "B", "T", "gru", "cmd_sim", "confid", "hidden", "wide", "inference", "overlap", "recurrence", "gemm_operands",
          "fusion_fp8", "embed_update", "embed_bg", "trainable", "moments", "fused", "labels", "opt_step", "enc_cached")
PLAN_INTS = ("embed_update", "embed_bg_wgs", "embed_bg_lds")
# trainable: 0 nothing frozen, 1 one fusion tensor frozen, 2 every encoder tensor and the table frozen (the cut), 3 the cut that stashes
ENCODER_TOPS = ("trnn1", "trnn2", "vrnn1", "vrnn2", "arnn1", "arnn2", "tlayer_norm", "vlayer_norm", "alayer_norm", "embed")


def make_handle(lib, r):
    """A model handle set as the row says, through the public entry points only.  Nothing is bound but fake parameter / moment
    addresses (never followed by the plan).  embed_bg: -1 the handle left alone, 0 off, 1 on with 8 workgroups."""
    cfg = _lib.MisaConfig(vocab=64, d_t=336 if r["wide"] else 300, d_v=35, d_a=74, hidden=r["hidden"], ncls=6, act=_lib.ACT["relu"],
                          use_cmd_sim=r["cmd_sim"], use_confidNet=r["confid"], dropout=0.5, fusion_dropout=0.1, threshold=0.5,
                          reverse_grad_weight=1.0, diff_weight=0.3, sim_weight=1.0, recon_weight=1.0, conf_weight=1.0, mode=r["bf16"],
                          rnncell=r["gru"])
    h = C.c_void_p()
    assert lib.mmda_misa_create(C.byref(cfg), C.byref(h)) == 0
    assert lib.mmda_misa_set_inference(h, r["inference"]) == 0 and lib.mmda_misa_set_overlap(h, r["overlap"]) == 0
    assert lib.mmda_misa_set_recurrence(h, r["recurrence"]) == 0 and lib.mmda_misa_set_gemm_operands(h, r["gemm_operands"]) == 0
    assert lib.mmda_misa_set_fusion_fp8(h, r["fusion_fp8"]) == 0 and lib.mmda_misa_set_embed_update(h, r["embed_update"]) == 0
    if r["embed_bg"] >= 0:
        assert lib.mmda_misa_set_embed_background(h, r["embed_bg"], 8 * r["embed_bg"]) == 0
    if r["trainable"]:
        flags = bytearray()
        for i in range(lib.mmda_misa_num_params(h)):
            name = C.c_char_p()
            assert lib.mmda_misa_param_info(h, i, C.byref(name), None, None, None) == 0
            key = name.value.decode()
            flags.append(int(key != "shared.shared_1.weight") if r["trainable"] == 1 else int(key.split(".")[0] not in ENCODER_TOPS))
        assert lib.mmda_misa_set_trainable(h, bytes(flags), len(flags)) == 0
        assert lib.mmda_misa_set_cut_forward(h, int(r["trainable"] == 3)) == 0
    assert lib.mmda_misa_bind(h, 4096, 8192, 12288 if r["moments"] else None, 16384 if r["moments"] else None) == 0
    return h


def plan_of(lib, r, switches=None):
    h = make_handle(lib, r)
    try:
        return ops.step_plan(h, r["B"], r["T"], fused=r["fused"], labels=r["labels"], opt_step=r["opt_step"], enc_cached=r["enc_cached"],
                             switches=switches)
    finally:
        lib.mmda_misa_destroy(h)


def unpack(fx, tail):
    """(bits, embed_update, embed_bg_wgs, embed_bg_lds) -> the recorded plan as a dict in ops.step_plan's types"""
    bits = [k for k in fx["plan"] if k not in PLAN_INTS]
    plan = {k: bool(tail[0] >> i & 1) for i, k in enumerate(bits)}
    plan["gm"] = int(plan["gm"])
    plan.update(zip(PLAN_INTS, tail[1:]))
    return plan


@pytest.fixture(scope="module")
def fx():
    with open(FIXTURE) as f:
        d = json.load(f)
    assert tuple(d["inputs"]) == INPUTS and tuple(d["switches"]) == tuple(_lib.STEP_SWITCHES)
    assert set(d["plan"]) == set(_lib.STEP_PLAN_FIELDS) - {"fused"}
    return d


def test_fixture_makes_every_plan_field_take_every_value(fx):
    """A thinned table must still exercise every rule: each boolean of the plan is recorded both ways, each integer at every value the
    sweep's settings can give it (embed_deferred: see the module docstring)."""
    n_in = len(INPUTS)
    plans = [unpack(fx, r[n_in:]) for r in fx["rows"]] + [unpack(fx, r[len(fx["switches"]) + 1:]) for r in fx["switch_rows"]]
    assert 1000 <= len(fx["rows"]) <= 5000 and len(fx["switch_rows"]) == 15 * 3
    seen = {k: {p[k] for p in plans} for k in fx["plan"]}
    for k in fx["plan"]:
        if k not in PLAN_INTS + ("embed_deferred", "gm"):
            assert seen[k] == {False, True}, k
    assert seen["gm"] == {0, 1} and seen["embed_deferred"] == {False}
    assert seen["embed_update"] == {0, 1, 2} and seen["embed_bg_wgs"] == {32, 8} and seen["embed_bg_lds"] == {1024, 4096}
    # ... and the inputs: every value of the sweep's axes is there
    cols = {k: {r[i] for r in fx["rows"]} for i, k in enumerate(INPUTS)}
    assert cols["B"] == {1, 7, 8, 32, 33, 64, 65, 127, 128, 256, 257} and cols["T"] == {1, 20, 50} and cols["hidden"] == {64, 128}
    assert cols["embed_update"] == {0, 1, 2} and cols["embed_bg"] == {-1, 0, 1} and cols["trainable"] == {0, 1, 2, 3}
    for k in set(INPUTS) - {"B", "T", "hidden", "embed_update", "embed_bg", "trainable"}:
        assert cols[k] == {0, 1}, k
    assert {tuple(r[n_in - 4:n_in]) for r in fx["rows"]} == {(0, 0, 0, 0), (1, 1, 0, 0), (1, 1, 1, 0), (0, 0, 0, 1), (1, 1, 0, 1), (1, 1, 1, 1)}


def test_plan_equals_the_recorded_plan_over_the_sweep(fx):
    lib = _lib.load()
    bad = []
    for row in fx["rows"]:
        r = dict(zip(INPUTS, row))
        want = dict(unpack(fx, row[len(INPUTS):]), fused=bool(r["fused"]))
        got = plan_of(lib, r)
        bad += [f"{r}: {k} = {got[k]}, recorded {want[k]}" for k in _lib.STEP_PLAN_FIELDS if got[k] != want[k]]
    assert not bad, f"{len(bad)} fields differ:\n" + "\n".join(bad[:20])


def _switch_row(fx, row):
    n = len(fx["switches"])
    r = dict(zip(INPUTS, (1, row[n], 50, 0, 1, 0, 128, 0, 0, 1, 1, 1, 0, 0, -1, 0, 1, 1, 1, 1, 0)))
    return r, dict(zip(fx["switches"], row[:n])), dict(unpack(fx, row[n + 1:]), fused=True)


def test_switch_vectors_through_the_argument(fx):
    """What took a fresh process per setting when the switches were read from the environment inside plan_step: one process here."""
    lib = _lib.load()
    moved = set()
    for row in fx["switch_rows"]:
        r, sw, want = _switch_row(fx, row)
        assert sum(v != _lib.STEP_SWITCHES[k] for k, v in sw.items()) == 1 and r["B"] in (32, 64, 256)
        got = plan_of(lib, r, sw)
        assert got == want, (sw, r["B"], {k: (got[k], want[k]) for k in got if got[k] != want[k]})
        moved |= {k for k, v in sw.items() if v != _lib.STEP_SWITCHES[k] and got != plan_of(lib, r)}
    assert moved == set(_lib.STEP_SWITCHES), f"switches that moved no plan field at any B: {sorted(set(_lib.STEP_SWITCHES) - moved)}"


def test_the_plan_follows_the_argument_not_the_environment(fx, monkeypatch):
    lib = _lib.load()
    r, _, _ = _switch_row(fx, fx["switch_rows"][0])
    default = plan_of(lib, r)
    assert default["row_fuse"] and default["tn_wgrad"]
    monkeypatch.setenv("MMDA_ROW_FUSE", "0")
    monkeypatch.setenv("MMDA_GEMM_TN", "0")
    assert plan_of(lib, r) == default                                    # NULL: the defaults, whatever the environment says
    assert plan_of(lib, r, {"MMDA_ROW_FUSE": 1}) == default
    off = plan_of(lib, r, {"MMDA_ROW_FUSE": 0})
    assert not off["row_fuse"] and off["tn_wgrad"] and not off["seed_recon"]
    monkeypatch.setenv("MMDA_ROW_FUSE", "1")
    assert plan_of(lib, r, {"MMDA_ROW_FUSE": 0}) == off and plan_of(lib, r, {"MMDA_GEMM_TN": 0})["row_fuse"]


def test_refusals_leave_out_untouched():
    lib = _lib.load()
    r = dict(zip(INPUTS, (1, 32, 50, 0, 1, 0, 128, 0, 0, 1, 1, 1, 0, 0, -1, 0, 1, 1, 1, 1, 0)))
    h = make_handle(lib, r)
    try:
        n = len(_lib.STEP_SWITCHES)
        req, sw = _lib.MisaStepRequest(1, 1, 1, 0), (C.c_int * n)(*_lib.STEP_SWITCHES.values())
        out = _lib.MisaStepPlan(*[77] * len(_lib.STEP_PLAN_FIELDS))
        for args in ((None, 32, 50, req, None, 0, out), (h, 32, 50, None, None, 0, out), (h, 32, 50, req, None, 0, None),
                     (h, 0, 50, req, None, 0, out), (h, -1, 50, req, None, 0, out), (h, 32, 0, req, None, 0, out),
                     (h, 32, 50, req, sw, n - 1, out), (h, 32, 50, req, sw, n + 1, out), (h, 32, 50, req, sw, 0, out)):
            assert lib.mmda_misa_plan_describe(*args) == -1, args[1:3] + args[5:6]
            assert all(getattr(out, k) == 77 for k in _lib.STEP_PLAN_FIELDS)
        assert lib.mmda_misa_plan_describe(h, 32, 50, req, sw, n, out) == 0 and out.fused == 1 and out.skinny == 1
    finally:
        lib.mmda_misa_destroy(h)
