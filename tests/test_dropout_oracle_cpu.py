"""CPU: the host restatement of the dropout masks (oracle/dropout_rng.py) and the masked oracle (misa_oracle ``masks=``) that
tests/test_gpu_dropout_parity.py holds the training-mode step against.

  * the mask function against values worked out from the C expression (mmda_amd/csrc/common.h) with Python integers;
  * ``masks`` of all ones against ``masks=None``: the same bits;
  * where each mask sits, against stock torch modules in ``.train()`` whose ``torch.nn.functional.dropout`` hands out the prepared masks
    in call order (the attention mask, which stock torch applies inside SDPA, against a float64 restatement written here);
  * the power check: at every configuration the GPU tests run, swapping ONE site's mask -- for another seed's, or for "nothing
    dropped, everything scaled" -- moves the loss or a gradient by at least 100 times the GPU test's tolerance.  A kernel that drops
    the wrong elements, or forgets the 1 / (1 - p) factor, at any one site therefore cannot pass there."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dropout_cases import CASES, grad_bounds, inputs_of, masks_of, sites_of
from oracle import dropout_rng as drng
from oracle import misa_oracle as orc

M64 = (1 << 64) - 1


def _u32_int(seed, site, idx):
    """rng_u32 of common.h with Python integers (masked to 64 bits after every sum and product)"""
    z = (seed + 0x9E3779B97F4A7C15 * (site + 1) + idx * 0xD6E8FEB86659FD93) & M64
    z ^= z >> 33; z = (z * 0xFF51AFD7ED558CCD) & M64
    z ^= z >> 33; z = (z * 0xC4CEB9FE1A85EC53) & M64
    z ^= z >> 33
    return (z >> 16) & 0xFFFFFFFF


# (seed, site, idx, rng_u32, u = (r >> 8) / 2^24): worked out once from the C expression, by hand with integer arithmetic
HAND = [(0, 0, 0, 1727112363, 0.40212464332580566),
        (1234567, 1, 0, 1594518639, 0.37125277519226074),
        (1234567, 1, 35, 903301310, 0.21031618118286133),
        (0x5EED, 3, 2047, 3499454981, 0.8147803544998169),
        (0xFFFFFFFFFFFFFFFF, 5, 7, 697285260, 0.16234934329986572),
        (42, 6, 5, 1503963626, 0.35016876459121704),
        (42, 6, (1 << 32) + 5, 4068901352, 0.947364866733551),                  # an index above 2^32: not the draw of index 5
        (987654321987654321, 4, (1 << 40) + 123, 2133411432, 0.4967235326766968)]


def test_mask_values_worked_out_by_hand():
    for seed, site, idx, r, u in HAND:
        assert _u32_int(seed, site, idx) == r
        assert int(drng.rng_u32(seed, site, idx)) == r, (seed, site, idx)
        assert (r >> 8) / 16777216.0 == u
        for p in (0.1, 0.25, 0.5, 0.9):
            keep = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
            want = 0.0 if np.float32(u) < np.float32(p) else keep
            assert float(drng.drop_mul(p, seed, site, idx)) == want, (seed, site, idx, p)
        assert float(drng.drop_mul(0.0, seed, site, idx)) == 1.0
    # a 64-bit index is not truncated: u(2^32 + 5) = 0.947 is kept at p = 0.5, u(5) = 0.350 is dropped
    assert float(drng.drop_mul(0.5, 42, 6, (1 << 32) + 5)) == 2.0 and float(drng.drop_mul(0.5, 42, 6, 5)) == 0.0
    # the kept value is the fp32 quotient widened, not the double one
    assert float(drng.drop_mul(0.1, 0, 0, 0)) == 1.1111111640930176
    # p = 0: all ones; mask() is drop_mul over the flat index, reshaped
    assert np.array_equal(drng.mask(0.0, 7, 2, (3, 4)), np.ones((3, 4)))
    m = drng.mask(0.25, 1234567, 1, (2, 3, 6))
    assert m.dtype == np.float64 and m.shape == (2, 3, 6)
    assert m[1, 2, 5] == float(drng.drop_mul(0.25, 1234567, 1, 35)) == 0.0          # u = 0.2103 < 0.25
    assert m[0, 0, 0] == float(np.float32(1.0) / np.float32(0.75))                  # u = 0.3713
    # the vectorised form against the integer form on indices spread over 64 bits
    rng = np.random.default_rng(5)
    idx = rng.integers(0, 1 << 63, 200, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 200, dtype=np.uint64)
    for seed, site in ((0x5EED, 1), (M64, 6), (1 << 63, 3)):
        assert [int(x) for x in drng.rng_u32(seed, site, idx)] == [_u32_int(seed, site, int(i)) for i in idx]


def test_site_masks_shapes_and_rates():
    cfg = orc.default_config(vocab_size=60, num_classes=6)
    B, seed = 37, 99
    m = drng.site_masks(cfg, B, seed, 0.25, 0.5)
    assert {k: tuple(v.shape) for k, v in m.items()} == {"attn": (B, 2, 6, 6), "drop1": (6, B, 128), "ffn": (6, B, 2048),
                                                          "drop2": (6, B, 128), "cls": (B, 6), "disc": (3, B, 128)}
    for k, v in m.items():
        p = 0.5 if k in ("cls", "disc") else 0.25
        keep = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
        assert v.dtype == torch.float64 and set(v.unique().tolist()) == {0.0, keep}, k
        n = v.numel()
        assert abs(float((v == 0).double().mean()) - p) < 5 * math.sqrt(p * (1 - p) / n), k          # five sigma
        # element (i, j, ...) is the draw of its flat index under the site's id
        flat = int(np.ravel_multi_index(tuple(s - 1 for s in v.shape), tuple(v.shape)))
        assert float(v.flatten()[-1]) == float(drng.drop_mul(p, seed, drng.SITES[k], flat))
    assert not torch.equal(m["drop1"], m["drop2"])                                                    # the site id enters the draw
    assert all(bool((v == 1).all()) for v in drng.ones_masks(cfg, B).values())


# ------------------------------------------------------------------------------------------------ masks of ones == masks=None
@pytest.mark.parametrize("use_cmd_sim", [True, False])
def test_all_ones_masks_give_the_bits_of_masks_none(use_cmd_sim):
    cfg = orc.default_config(vocab_size=70, use_cmd_sim=use_cmd_sim, use_confidNet=True)
    P = orc.synth_params(cfg, 3)
    batch = orc.synth_batch(cfg, 5, 4, 2, ragged=True)
    o0, L0, G0 = orc.loss_and_grads(P, cfg, batch)
    o1, L1, G1 = orc.loss_and_grads(P, cfg, batch, masks=drng.ones_masks(cfg, 5))
    for k, v in vars(o0).items():
        if v is None:
            assert getattr(o1, k) is None
        else:
            assert torch.equal(v, getattr(o1, k)), k
    for k, v in vars(L0).items():
        assert torch.equal(v, getattr(L1, k)), k
    assert G0.keys() == G1.keys()
    for k, g in G0.items():
        assert (g is None) == (G1[k] is None), k
        if g is not None:
            assert torch.equal(g, G1[k]), k


# ------------------------------------------------------------------------------------------------ placement
def _fusion_params(hs, seed, dtype=torch.float64):
    cfg = orc.default_config(vocab_size=10, hidden_size=hs)
    te = "transformer_encoder.layers.0."
    return cfg, {k: v.to(dtype) for k, v in orc.synth_params(cfg, seed).items() if k.startswith(te) or k.startswith("classifier")}


def _hand_out(queue):
    """A stand-in for torch.nn.functional.dropout that multiplies by the prepared masks in call order"""
    def fake(input, p=0.5, training=True, inplace=False):
        assert training and p > 0
        name, m = queue.pop(0)
        assert m.shape == input.shape, (name, m.shape, input.shape)
        return input * m.to(input.dtype)
    return fake


def test_drop1_ffn_drop2_sit_where_the_stock_encoder_layer_drops(monkeypatch):
    """nn.TransformerEncoderLayer in .train() (attention dropout 0): its three F.dropout calls are dropout1 (on sa), the feed-forward
    dropout (on relu(linear1 x)) and dropout2 (on ff), in that order.  Output and every gradient against fusion_layer(masks=...)."""
    hs, B, p = 32, 5, 0.25
    cfg, P = _fusion_params(hs, 11)
    te = "transformer_encoder.layers.0."
    layer = torch.nn.TransformerEncoderLayer(d_model=hs, nhead=orc.NHEAD, dropout=p).double()
    layer.load_state_dict({k[len(te):]: v for k, v in P.items() if k.startswith(te)})
    layer.self_attn.dropout = 0.0
    layer.train()
    masks = drng.site_masks(cfg, B, 2024, p, 0.5)
    masks["attn"] = torch.ones_like(masks["attn"])
    for k in ("drop1", "ffn", "drop2"):
        assert bool((masks[k] == 0).any()) and bool((masks[k] != 0).any())
    x = torch.randn(6, B, hs, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    w = torch.randn(6, B, hs, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    queue = [(k, masks[k]) for k in ("drop1", "ffn", "drop2")]
    monkeypatch.setattr(torch.nn.functional, "dropout", _hand_out(queue))
    xs = x.clone().requires_grad_(True)
    ys = layer(xs)
    assert not queue, "the stock layer called dropout fewer than three times"
    (ys * w).sum().backward()
    monkeypatch.undo()
    leaves = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    xo = x.clone().requires_grad_(True)
    yo = orc.fusion_layer(xo, leaves, masks=masks)
    (yo * w).sum().backward()
    assert float((yo - ys).detach().abs().max()) < 1e-12
    assert float((xo.grad - xs.grad).abs().max()) < 1e-12 * max(1.0, float(xs.grad.abs().max()))
    for k, v in layer.named_parameters():
        g = leaves[te + k].grad
        assert float((g - v.grad).abs().max()) < 1e-12 * max(1.0, float(v.grad.abs().max())), k
    # and the masks matter: without them the output is another one
    assert float((orc.fusion_layer(x, P) - ys).detach().abs().max()) > 1e-2


def test_cls_mask_sits_where_the_stock_classifier_drops(monkeypatch):
    """The reference's classifier is Sequential(Linear, Dropout, Sigmoid) (models.py:150-153): the mask multiplies the logits."""
    hs, B, p = 16, 7, 0.5
    cfg, P = _fusion_params(hs, 12)
    torch.manual_seed(3)
    utt = {m: torch.randn(B, 4 * d, dtype=torch.float64) for m, d in (("t", cfg.embedding_size), ("v", cfg.visual_size), ("a", cfg.acoustic_size))}
    Pfull = {k: v.double() for k, v in orc.synth_params(cfg, 12).items()}
    masks = drng.ones_masks(cfg, B)
    masks["cls"] = drng.site_masks(cfg, B, 77, 0.25, p)["cls"]
    assert bool((masks["cls"] == 0).any()) and bool((masks["cls"] != 0).any())
    o = orc.fusion_from_utterances(Pfull, cfg, utt, masks=masks)
    o_eval = orc.fusion_from_utterances(Pfull, cfg, utt)
    assert torch.equal(o.h, o_eval.h) and torch.equal(o.tcp, o_eval.tcp)                     # the confidence head has no dropout
    head = torch.nn.Sequential(torch.nn.Linear(6 * hs, cfg.num_classes), torch.nn.Dropout(p), torch.nn.Sigmoid()).double()
    head.load_state_dict({"0.weight": Pfull["classifier.classifier_layer.weight"], "0.bias": Pfull["classifier.classifier_layer.bias"]})
    head.train()
    queue = [("cls", masks["cls"])]
    monkeypatch.setattr(torch.nn.functional, "dropout", _hand_out(queue))
    s = head(o.h)
    assert not queue
    monkeypatch.undo()
    assert float((s - o.scores).abs().max()) < 1e-14
    assert bool((o.scores[masks["cls"] == 0] == 0.5).all())                                    # a dropped logit is sigmoid(0)
    assert torch.equal(o.labels, (o.scores > cfg.threshold).to(o.scores.dtype))


def test_attn_mask_multiplies_the_softmax_rows_before_the_value_product():
    """Attention dropout is out of reach of the F.dropout stand-in (stock torch applies it inside SDPA): a float64 restatement, head by
    head and sample by sample, of what multi_head_attention_forward computes -- dropout(softmax(q k' / sqrt(hd))) v."""
    hs, B, p = 32, 4, 0.25
    cfg, P = _fusion_params(hs, 13)
    te = "transformer_encoder.layers.0."
    masks = drng.ones_masks(cfg, B)
    masks["attn"] = drng.site_masks(cfg, B, 31337, p, 0.5)["attn"]
    assert bool((masks["attn"] == 0).any()) and bool((masks["attn"] != 0).any())
    x = torch.randn(6, B, hs, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
    hd = hs // orc.NHEAD
    qkv = F.linear(x, P[te + "self_attn.in_proj_weight"], P[te + "self_attn.in_proj_bias"])
    ctx = torch.zeros(6, B, hs, dtype=torch.float64)
    for b in range(B):
        for h in range(orc.NHEAD):
            q, k, v = (qkv[:, b, i * hs + h * hd:i * hs + (h + 1) * hd] for i in range(3))
            pr = torch.softmax(q @ k.t() / math.sqrt(hd), dim=1) * masks["attn"][b, h]
            ctx[:, b, h * hd:(h + 1) * hd] = pr @ v
    x1 = F.layer_norm(x + F.linear(ctx, P[te + "self_attn.out_proj.weight"], P[te + "self_attn.out_proj.bias"]), (hs,),
                      P[te + "norm1.weight"], P[te + "norm1.bias"])
    ff = F.linear(torch.relu(F.linear(x1, P[te + "linear1.weight"], P[te + "linear1.bias"])), P[te + "linear2.weight"], P[te + "linear2.bias"])
    want = F.layer_norm(x1 + ff, (hs,), P[te + "norm2.weight"], P[te + "norm2.bias"])
    got = orc.fusion_layer(x, P, masks=masks)
    assert float((got - want).abs().max()) < 1e-12
    assert float((orc.fusion_layer(x, P) - want).abs().max()) > 1e-3


def test_disc_mask_multiplies_the_activation_output():
    """models.py:124-127: Linear, activation, Dropout, Linear.  With the discriminator's second layer fed by hand."""
    cfg = orc.default_config(vocab_size=10, hidden_size=16, use_cmd_sim=False, activation="relu")
    P = {k: v.double() for k, v in orc.synth_params(cfg, 14).items()}
    B = 5
    torch.manual_seed(5)
    utt = {m: torch.randn(B, 4 * d, dtype=torch.float64) for m, d in (("t", cfg.embedding_size), ("v", cfg.visual_size), ("a", cfg.acoustic_size))}
    masks = drng.ones_masks(cfg, B)
    masks["disc"] = drng.site_masks(cfg, B, 5150, 0.25, 0.5)["disc"]
    o = orc.fusion_from_utterances(P, cfg, utt, masks=masks)
    for i, m in enumerate("tva"):
        sh = getattr(o, f"utt_shared_{m}")
        hdn = torch.relu(F.linear(sh, P["discriminator.discriminator_layer_1.weight"], P["discriminator.discriminator_layer_1.bias"]))
        want = F.linear(hdn * masks["disc"][i], P["discriminator.discriminator_layer_2.weight"], P["discriminator.discriminator_layer_2.bias"])
        assert float((getattr(o, f"domain_label_{m}") - want).abs().max()) < 1e-13, m


# ------------------------------------------------------------------------------------------------ the GPU cases: masks and power
@pytest.mark.parametrize("name", list(CASES))
def test_every_mask_of_the_gpu_cases_drops_and_keeps(name):
    case = CASES[name]
    masks = masks_of(case)
    for site in sites_of(case):
        m = masks[site]
        assert bool((m == 0).any()) and bool((m != 0).any()), (name, site)
    if case.B == 1:
        assert masks["cls"].numel() == 6


KINK_MARGIN = 2e-6


def _kink_margin(case, seed=None):
    """The smallest |pre-activation| among the units whose derivative jumps at zero and whose gradient is live: the three projections
    and the discriminator's first layer (leaky ReLU and its kin), and the kept hidden units of the feed-forward block (ReLU).  From a
    float64 run of the oracle."""
    cfg, P, batch = inputs_of(case)
    masks = masks_of(case, seed)
    P64 = {k: v.double() for k, v in P.items()}
    seen = {}
    real_ffn, real_linear = orc.ffn_exact, orc._linear

    def ffn(x, P_, mask=None):
        z = real_linear(x, P_, "transformer_encoder.layers.0.linear1")
        seen["ffn"] = float(z[mask != 0].abs().min())
        return real_ffn(x, P_, mask)

    def linear(x, P_, name):
        z = real_linear(x, P_, name)
        if name.startswith("project_"):
            seen[name] = float(z.abs().min())
        elif name == "discriminator.discriminator_layer_1":
            i = sum(k.startswith("disc") for k in seen)
            seen[f"disc{i}"] = float(z[masks["disc"][i] != 0].abs().min())
        return z

    orc.ffn_exact, orc._linear = ffn, linear
    try:
        with torch.no_grad():
            orc.forward(P64, cfg, batch["t"], batch["v"].double(), batch["a"].double(), batch["l"], masks=masks)
    finally:
        orc.ffn_exact, orc._linear = real_ffn, real_linear
    assert "ffn" in seen and len(seen) == (4 if cfg.use_cmd_sim else 7), seen
    return min(seen.values()), seen


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if not c.kink_floor])
def test_no_live_unit_of_the_gpu_cases_sits_on_an_activation_kink(name):
    """ReLU's derivative jumps at zero: a hidden unit whose pre-activation lies within fp32 rounding of zero (1e-7 .. 3e-7 here: 128
    products of magnitude 0.05, an input row that carries 3e-7 of its own) has gradient 0 in one correct fp32 implementation and d_f1
    in the next, and one such unit moves linear1's weight gradient by 5e-4 .. 2e-3 of its max (seen at B = 260: the fp32 oracle
    against its own float64 run, 2.1e-3, with a kept unit at |z| = 7e-8).  That is no error of either side, so the cases are chosen away
    from it: every live unit keeps at least 2e-6 from the kink, ten times the rounding, in the float64 oracle.  (B = 260 cannot be
    chosen away from it: dropout_cases.grad_bounds.)"""
    margin, seen = _kink_margin(CASES[name])
    print(name, {k: f"{v:.2e}" for k, v in seen.items()})
    assert margin >= KINK_MARGIN, (name, seen)


def test_float64_floor_of_the_b260_case_widens_few_tensors_and_none_far():
    """dropout_cases.grad_bounds at B = 260: the case does sit on the kink (float64 run); the widened bounds are those of the
    feed-forward's first layer, whose rows a flipped gate owns, and of the visual branch behind a flipped projection unit, none beyond
    1e-2, and three quarters of the tensors keep 2e-4.  The table stays tied to its measurement: the fp32 oracle's error against its
    float64 run, measured again here, lies within a factor of two of every entry, either way (loose on purpose: an fp32 run on another
    host may sum in another order), and no tensor outside the table exceeds a quarter of tol_grad by more than that."""
    from dropout_cases import KINK_FLOOR_B260, fp32_oracle_error
    case = CASES["generic_b260"]
    margin, _ = _kink_margin(case)
    assert margin < 3e-7                                     # below the mean fp32 rounding of a pre-activation
    G, bounds = grad_bounds(case)
    assert all(g is None or g.dtype == torch.float64 for g in G.values())
    assert set(KINK_FLOOR_B260) <= set(bounds)
    wide = {k: b for k, b in bounds.items() if b > case.tol_grad}
    assert 0 < len(wide) <= 26 and max(wide.values()) < 1e-2 and len(bounds) - len(wide) >= 73, wide
    assert all(b <= 2e-3 for k, b in wide.items() if not k.startswith("transformer_encoder")), wide
    assert all(k.split(".")[0] in ("transformer_encoder", "vrnn1", "vrnn2", "project_v", "vlayer_norm") for k, b in wide.items() if b > 5e-4)
    measured = fp32_oracle_error(case)
    print({k: f"{e:.2e}" for k, e in measured.items() if e > 5e-5})
    for k, e in KINK_FLOOR_B260.items():
        assert 0.5 * e <= measured[k] <= 2.0 * e, f"{k}: table {e:.2e}, measured {measured[k]:.2e}"
    assert all(e <= 2.0 * 0.25 * case.tol_grad for k, e in measured.items() if k not in KINK_FLOOR_B260)


def _moved(case, ref, got):
    """By how many tolerances of the GPU test the step ``got`` lies from ``ref``: the total loss (relative), or the worst parameter
    gradient -- fp32: max error relative to the tensor's max magnitude; bf16: relative L2, as the GPU test measures each, over the
    tensors the GPU test compares (B = 1: those whose gradient is finite in the oracle).  Scores, tcp and the single losses, which the
    GPU test asserts as well, are not counted: the measure is the stricter one."""
    (_, L0, G0), (_, L1, G1) = ref, got
    bounds = grad_bounds(case)[1]
    l0, l1 = float(L0.total.detach()), float(L1.total.detach())
    worst = abs(l1 - l0) / abs(l0) / case.tol_loss
    for k, g0 in G0.items():
        if g0 is None or k.endswith("self_attn.in_proj_bias") or not bool(torch.isfinite(g0).all()):
            continue                                             # (left out by the GPU test's _assert_grads in the same way)
        g0, g1 = g0.double(), G1[k].double()
        if case.precision == "fp32":
            e = float((g1 - g0).abs().max() / g0.abs().max().clamp_min(1e-6))
        else:
            e = float((g1 - g0).norm() / g0.norm().clamp_min(1e-30))
        worst = max(worst, e / bounds[k])
    return worst


@pytest.mark.parametrize("name", list(CASES))
def test_power_every_site_moves_the_step_by_100_tolerances(name):
    """Each site's mask, swapped for the one of seed + 1 and for all-1/(1-p), moves the total loss or a parameter gradient by at least
    100 times the bound the GPU test applies.  (Sensitivity is a property of the function: the exact oracle is used for the bf16 case
    too, against that case's bounds.)"""
    case = CASES[name]
    cfg, P, batch = inputs_of(case)
    masks = masks_of(case)
    other = masks_of(case, case.seed + 1)
    ref = orc.loss_and_grads(P, cfg, batch, masks=masks)
    for site in sites_of(case):
        p = case.p_cls if site in ("cls", "disc") else case.p_tf
        keep = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
        for what, swap in (("seed + 1", other[site]), ("all kept", torch.full_like(masks[site], keep))):
            assert not torch.equal(swap, masks[site])
            got = orc.loss_and_grads(P, cfg, batch, masks=dict(masks, **{site: swap}))
            moved = _moved(case, ref, got)
            print(f"{name} {site} {what}: {moved:.1f} tolerances")
            assert moved >= 100.0, f"{name}: site {site} swapped for '{what}' moves the step by {moved:.1f} tolerances only"
