"""The training-mode (dropout on) model configurations that tests/test_gpu_dropout_parity.py runs on the GPU and that
tests/test_dropout_oracle_cpu.py proves sensitive on the CPU (the power check): one table, so the two files cannot drift apart.

Every case is one training step from ``orc.synth_params(cfg, wseed)`` on ``orc.synth_batch(cfg, B, T, bseed, ragged)`` with the dropout
masks of ``seed``: ``p_tf`` (mmda_amd.models.FUSION_DROPOUT) at the four sites of the fusion layer, ``p_cls`` (config.dropout) at the
classifier logits and in the discriminator.  ``tol_out`` / ``tol_grad`` are the dropout-off bounds of the same path
(tests/test_gpu_model.py): a mask multiplies by 0 or by a constant, so no new rounding enters.  The seeds are constants: each was
checked (test_dropout_oracle_cpu.py) to give masks with dropped and kept elements at every site, a step that every site moves, and no
live unit within fp32 rounding of an activation's kink (where two correct fp32 implementations may disagree about a gradient)."""
from types import SimpleNamespace

from oracle import dropout_rng as drng
from oracle import misa_oracle as orc

SITE_NAMES = ("attn", "drop1", "ffn", "drop2", "cls", "disc")


def _case(name, *, B, T=4, ragged=True, precision="fp32", p_tf=0.25, p_cls=0.5, seed, wseed=31, bseed=17, kink_floor=False, **cfg_kw):
    fp32 = precision == "fp32"
    return SimpleNamespace(name=name, B=B, T=T, ragged=ragged, precision=precision, p_tf=p_tf, p_cls=p_cls, seed=seed, wseed=wseed,
                           bseed=bseed, kink_floor=kink_floor, cfg_kw=dict(vocab_size=80, dropout=p_cls, **cfg_kw),
                           # fp32: outputs and losses 1e-4, gradients 2e-4 of the tensor's max (test_fp32_fused_step_matches_golden);
                           # bf16: outputs 1e-3, losses 1e-4, gradients 1e-2 relative L2, all against the bf16-emulating oracle
                           # (test_bf16_path_within_1e2, part 1)
                           tol_out=1e-4 if fp32 else 1e-3, tol_loss=1e-4, tol_grad=2e-4 if fp32 else 1e-2)


CASES = {c.name: c for c in (
    _case("fused_b5", B=5, seed=0x1D0A5EF0),                                   # (a) the default fused stretches
    _case("fused_b1", B=1, seed=0x1D0A5EF3),                                    # (a) one sample per workgroup
    _case("fused_b5_p01", B=5, p_tf=0.1, seed=0x2B0B0001),                      # the default FUSION_DROPOUT
    _case("adv_confid_b6", B=6, seed=0x3C0C0002, use_cmd_sim=False, use_confidNet=True),      # (b) stand-alone launches, SITE_DISC
    # (c) above SKINNY_MAX_B: the tiled generic GEMM epilogue.  3.2 M hidden units: some sit on the ReLU kink whatever the seed, see
    # grad_bounds()
    _case("generic_b260", B=260, T=3, seed=0x4D0D0003, kink_floor=True),
    # (d) gate-minor resident recurrences.  The bf16 bounds are 50 times wider than the fp32 ones, so only the loss (1e-4) can show a
    # swap at 100 tolerances: this seed is the third of 1500 consecutive ones at which all ten swaps move the total loss by over 1 %
    _case("bf16_b8", B=8, precision="bf16", seed=0x5E0E04F5),
    # (f) the autograd entry draws its own seed: the first draw of a fresh model (MISA._seed = 0x5EED through MISA._next_seed)
    _case("autograd_b5", B=5, seed=(0x5EED * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF),
)}


def config_of(case):
    return orc.default_config(**case.cfg_kw)


def sites_of(case):
    """The sites a case runs: the discriminator (and its dropout) exists in the adversarial configuration only."""
    return tuple(s for s in SITE_NAMES if s != "disc" or not case.cfg_kw.get("use_cmd_sim", True))


def inputs_of(case):
    cfg = config_of(case)
    return cfg, orc.synth_params(cfg, case.wseed), orc.synth_batch(cfg, case.B, case.T, case.bseed, case.ragged)


def masks_of(case, seed=None):
    return drng.site_masks(config_of(case), case.B, case.seed if seed is None else seed, case.p_tf, case.p_cls)


_REF = {}


def reference(case):
    """(cfg, P, batch, masks, (o, L, G)) of the case: the masked oracle's step, computed once per process and never modified.  bf16: the
    bf16-emulating oracle with per-tile partial sums (the resident recurrences)."""
    if case.name not in _REF:
        cfg, P, batch = inputs_of(case)
        masks = masks_of(case)
        if case.precision == "fp32":
            out = orc.loss_and_grads(P, cfg, batch, masks=masks)
        else:
            from oracle import bf16_emul as emu
            out = emu.loss_and_grads(P, cfg, batch, rounding=True, tile_partials=True, masks=masks)
        _REF[case.name] = (cfg, P, batch, masks, out)
    return _REF[case.name]


def _max_rel(g, ref):
    return float((g.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-6))


def float64_grads(case):
    """The masked oracle's gradients from a float64 run of the case (parameters and inputs widened, same masks)."""
    import torch
    cfg, P, batch, masks, _ = reference(case)
    P64 = {k: v.double() for k, v in P.items()}
    b64 = dict(batch, v=batch["v"].double(), a=batch["a"].double(), emo=batch["emo"].double())
    old = torch.get_default_dtype()
    try:
        torch.set_default_dtype(torch.float64)                    # (the encoders' nn.LSTM modules are made inside the oracle)
        return orc.loss_and_grads(P64, cfg, b64, masks=masks)[2]
    finally:
        torch.set_default_dtype(old)


def fp32_oracle_error(case):
    """{parameter: max error, relative to the tensor's max, of the fp32 oracle's gradient against its own float64 run}: the
    measurement behind KINK_FLOOR_B260."""
    G, G64 = reference(case)[4][2], float64_grads(case)
    return {k: _max_rel(g, G64[k]) for k, g in G.items() if g is not None}


# generic_b260: fp32_oracle_error() as measured when the case was written, for every tensor where it exceeds a quarter of tol_grad
TE = "transformer_encoder.layers.0."
KINK_FLOOR_B260 = {
    TE + "linear1.weight": 2.08e-3, TE + "linear1.bias": 1.63e-3,
    "vrnn1.weight_ih_l0_reverse": 4.71e-4, "vrnn1.weight_hh_l0_reverse": 4.05e-4, "vrnn1.weight_hh_l0": 3.54e-4, "vrnn1.weight_ih_l0": 3.37e-4,
    "vrnn2.weight_ih_l0": 2.33e-4, "vrnn2.weight_hh_l0": 2.29e-4, "project_v.project_v.weight": 1.93e-4,
    "vrnn2.weight_ih_l0_reverse": 1.63e-4, "vlayer_norm.weight": 1.27e-4, "vrnn2.weight_hh_l0_reverse": 1.21e-4, "embed.weight": 1.06e-4,
    "shared.shared_1.weight": 7.5e-5, "vrnn2.bias_ih_l0": 6.7e-5, "vrnn2.bias_hh_l0": 6.7e-5, "vrnn1.bias_ih_l0_reverse": 5.9e-5,
    "vrnn1.bias_hh_l0_reverse": 5.9e-5, "arnn2.weight_hh_l0": 5.6e-5, "arnn2.weight_ih_l0": 5.4e-5, "arnn1.weight_ih_l0_reverse": 5.3e-5,
    "trnn1.weight_ih_l0": 5.3e-5, "vrnn1.bias_ih_l0": 5.2e-5, "vrnn1.bias_hh_l0": 5.2e-5, "vlayer_norm.bias": 5.1e-5,
    "project_v.project_v.bias": 5.0e-5}

_BOUNDS = {}


def grad_bounds(case):
    """(G, {parameter: bound}): the gradients a GPU step of the case is compared with, and the bound of each.

    Everywhere but at B = 260 that is the oracle's G at ``tol_grad``.  At B = 260 the step has 6 x 260 x 2048 = 3.2 M ReLU units and
    100 k leaky-ReLU units, and the fp32 rounding of a pre-activation (measured in the oracle, fp32 against float64: mean 1.8e-7, max
    1.7e-6) is larger than the distance of the nearest live unit from zero (7e-8 in the feed-forward block, 1.8e-7 in the visual
    projection; of 600 dropout seeds and 13 batches tried, none keeps every unit 2e-6 away).  Two correct fp32 implementations then
    disagree about a gate or two, and one gate is a whole row's worth of one weight gradient: the fp32 oracle against ITS OWN float64
    run, same masks, differs by 2.1e-3 of the max in linear1.weight, 1.6e-3 in linear1.bias, 3.4e-4 .. 4.7e-4 in vrnn1's weights and
    less elsewhere (KINK_FLOOR_B260; with one site's mask at a time: 8e-7 everywhere -- no unit on the kink, so this is no property of
    a mask).  So there the reference is the float64 run, which no rounding flips, and a tensor's bound is four times that measured error
    of the fp32 oracle where this exceeds ``tol_grad``: 8.3e-3 and 6.5e-3 for linear1, 1.3e-3 .. 1.9e-3 for vrnn1's weights, 4e-4 ..
    9.3e-4 for seven more tensors, 2e-4 .. 3e-4 for thirteen, ``tol_grad`` = 2e-4 for the other 73.  The table is a constant (an fp32
    CPU run may round differently on another host; the float64 run and the kernels do not), made from oracle runs alone, never from
    a kernel's output."""
    if case.name not in _BOUNDS:
        G = reference(case)[4][2]
        bounds = {k: case.tol_grad for k in G}
        if case.kink_floor:
            G = float64_grads(case)
            bounds.update({k: max(case.tol_grad, 4.0 * e) for k, e in KINK_FLOOR_B260.items()})
        _BOUNDS[case.name] = (G, bounds)
    return _BOUNDS[case.name]
