"""CPU: the host side of MC-dropout uncertainty (mmda_amd/uncertainty.py) and the yardsticks its GPU tests are held against.

  * the numpy restatement of the seven figures (tests/uncertainty_cases.py) on cases worked out by hand;
  * the chunk seeds against ``MISA._next_seed``'s constants, the chunking, and every refusal by the name of its setting;
  * the power check: over rows repeated K = 3 times the draws of one sample differ from each other, and from what a pass that ignored
    the column index would give, by at least 100 times the bound the GPU test applies -- so that test can tell the two apart;
  * the constants the GPU test relies on: ``MC_SEED`` keeps every oracle draw ``VOTE_MARGIN`` from the threshold."""
import math

import numpy as np
import pytest
import torch

import uncertainty_cases as uc
from dropout_cases import CASES, inputs_of
from oracle import dropout_rng as drng
from oracle import misa_oracle as orc

LN2 = math.log(2.0)


# ------------------------------------------------------------------------------------------------ the figures, by hand
def _one(draws, thr=0.35):
    r = uc.mc_reference(np.array(draws, dtype=np.float32).reshape(-1, 1), len(draws), np.float32(thr))
    return {k: float(r[k][0, 0]) for k in uc.STATS}


def test_reference_figures_on_hand_computed_cases():
    # K = 1: the mean is the draw, the variance exactly 0, no disagreement to inform about.  h(1/4) = ln 4 - (3/4) ln 3
    h25 = math.log(4.0) - 0.75 * math.log(3.0)
    r = _one([0.25])
    assert r["mean"] == 0.25 and r["var"] == 0.0 and r["vote"] == 0.0
    assert abs(r["entropy"] - h25) < 1e-15 and abs(r["expected_entropy"] - h25) < 1e-15 and r["mutual_info"] == 0.0
    assert abs(h25 - 0.5623351446188083) < 1e-15
    # all draws equal (1/2, exact in binary): variance 0, entropy ln 2 in both forms, no mutual information, every draw above 0.35
    r = _one([0.5] * 4)
    assert r == dict(mean=0.5, var=0.0, entropy=LN2, expected_entropy=LN2, mutual_info=0.0, vote=1.0)
    # draws 0 and 1: the mean is undecided (ln 2), every single draw is certain (h(0) = h(1) = 0): all of it is mutual information
    r = _one([0.0, 1.0])
    assert r == dict(mean=0.5, var=0.25, entropy=LN2, expected_entropy=0.0, mutual_info=LN2, vote=0.5)
    # three draws 0.2, 0.4, 0.9: mean 0.5, var = (0.09 + 0.01 + 0.16) / 3, two of three above 0.35
    r = _one([0.2, 0.4, 0.9])
    d = [float(np.float32(x)) for x in (0.2, 0.4, 0.9)]
    assert abs(r["mean"] - sum(d) / 3) < 1e-15 and abs(r["var"] - 0.26 / 3) < 1e-7 and r["vote"] == 2.0 / 3.0
    eh = sum(-x * math.log(x) - (1 - x) * math.log(1 - x) for x in d) / 3
    assert abs(r["expected_entropy"] - eh) < 1e-15 and abs(r["mutual_info"] - (r["entropy"] - eh)) < 1e-15 and r["mutual_info"] > 0.05
    # one NaN: every float64 figure of the element is NaN; the vote is a count, and a NaN is not above
    r = _one([0.5, float("nan")])
    assert all(math.isnan(r[k]) for k in ("mean", "var", "entropy", "expected_entropy", "mutual_info")) and r["vote"] == 0.5
    # ... and it touches no other element
    p = np.array([[0.5, 0.25], [np.nan, 0.25]], dtype=np.float32)
    r2 = uc.mc_reference(p, 2, np.float32(0.35))
    assert math.isnan(r2["mean"][0, 0]) and r2["mean"][0, 1] == 0.25 and r2["var"][0, 1] == 0.0 and r2["mutual_info"][0, 1] == 0.0
    # the vote compares in fp32 and strictly; without thresholds it is left out, without `bernoulli` the entropy figures are
    assert _one([0.35], thr=0.35)["vote"] == 0.0
    r3 = uc.mc_reference(p, 2, None, bernoulli=False)
    assert set(r3) == {"draws", "mean", "var"}
    # mutual information is clipped at 0 (rounding can make h(mean) - mean h a hair negative where all draws are equal)
    q = np.full((7, 1), 0.3, dtype=np.float32)
    assert uc.mc_reference(q, 7)["mutual_info"][0, 0] >= 0.0
    assert uc.bernoulli_entropy(np.array([0.0, 1.0, 0.5])).tolist() == [0.0, 0.0, LN2]


def test_reduce_inputs_hold_every_planted_value():
    for B, K, W in uc.REDUCE_SHAPES:
        p, thr = uc.reduce_input(B, K, W)
        assert p.shape == (B * K, W) and p.dtype == np.float32 and thr.shape == (W,)
        flat = p.reshape(-1)
        if flat.size >= len(uc.PLANTED):
            assert (flat == 0.0).any() and (flat == 1.0).any() and (flat == np.float32(uc.ALMOST_ONE)).any()
            assert (flat == np.float32(uc.DENORMAL)).any() and 0.0 < uc.DENORMAL < np.finfo(np.float32).tiny
            assert int(np.isnan(flat).sum()) == 1
        r = uc.mc_reference(p, K, thr)
        assert all(r[k].shape == (B, W) for k in uc.STATS)
        assert int(np.isnan(r["mean"]).sum()) == int(np.isnan(flat).sum()) and not np.isnan(r["vote"]).any()


# ------------------------------------------------------------------------------------------------ seeds, chunks, refusals
def test_chunk_seeds_are_next_seeds_lcg_with_their_own_state():
    from mmda_amd import uncertainty as un
    from mmda_amd.models import MISA

    class Stub:                                              # _next_seed reads and writes `_seed` only
        _seed = 0x5EED
    assert (un.SEED_MUL, un.SEED_ADD, un.SEED_MASK) == (6364136223846793005, 1442695040888963407, (1 << 64) - 1)
    seeds = un.chunk_seeds(0x5EED, 5)
    stub = Stub()
    assert seeds[0] == 0x5EED and seeds[1:] == [MISA._next_seed(stub) for _ in range(4)]
    assert un.chunk_seeds(-1, 2)[0] == (1 << 64) - 1 and all(0 <= s < (1 << 64) for s in un.chunk_seeds(-1, 3))
    assert un.chunk_seeds(7, 0) == []
    # (the autograd case of tests/dropout_cases.py spells the same step out)
    assert un.chunk_seeds(0x5EED, 2)[1] == CASES["autograd_b5"].seed


def test_chunking():
    from mmda_amd.uncertainty import chunk_plan
    assert [c.tolist() for c in chunk_plan(7, 3, 16)] == [[0, 1, 2, 3, 4], [5, 6]]
    assert [c.tolist() for c in chunk_plan(7, 16, 16)] == [[i] for i in range(7)]
    assert [c.tolist() for c in chunk_plan(4, 65, 260)] == [[0, 1, 2, 3]]
    assert [len(c) for c in chunk_plan(4096, 32, 256)] == [8] * 512
    assert chunk_plan(0, 3, 16) == []
    assert all(c.dtype == np.int64 for c in chunk_plan(7, 3, 16))


def test_every_refusal_names_its_setting():
    from mmda_amd import MISA, MCDropoutPass, make_config, mc_statistics
    from mmda_amd._lib import MMDAError
    from mmda_amd.uncertainty import check_settings
    cfg = orc.default_config(vocab_size=40)
    model = MISA(make_config(precision="fp32", device="cpu", **vars(cfg)))
    for bad in (0, 257, -3, 2.5, True, None):
        with pytest.raises(MMDAError, match="passes must be an int in 1 .. 256"):
            MCDropoutPass(model, passes=bad)
    for bad in (7, 0, True, 8.0):
        with pytest.raises(MMDAError, match="columns must be an int >= passes"):
            MCDropoutPass(model, passes=8, columns=bad)
    MCDropoutPass(model, passes=8, columns=8), MCDropoutPass(model, passes=1, columns=1), MCDropoutPass(model, passes=256)
    with pytest.raises(MMDAError, match="task='sentiment'"):
        check_settings(8, 256, "sentiment")
    senti = MISA(make_config(precision="fp32", device="cpu", task="sentiment", **dict(vars(cfg), num_classes=1)))
    with pytest.raises(MMDAError, match="task='sentiment'"):
        MCDropoutPass(senti, passes=8)
    # a model that is not on the device: named before anything is launched (this host has no device to launch on)
    from mmda_amd.encoded import EncoderCache
    flat = torch.zeros(3 * 8)
    cache = EncoderCache(flat, (4, 4, 4), 2, None, torch.tensor([1, 1]), np.array(["a", "b"], dtype=object), 0)
    with pytest.raises(MMDAError, match="MCDropoutPass: the model is on cpu"):
        MCDropoutPass(model, passes=2).run_cache(cache)
    with pytest.raises(MMDAError, match="needs a device tensor"):
        mc_statistics(torch.zeros(4, 2), 2)
    with pytest.raises(MMDAError, match="passes must be"):
        mc_statistics(torch.zeros(4, 2), 0)
    # a cache of other widths is refused by the cache's own rule, by name
    with pytest.raises(MMDAError, match="encoder cache: its rows are"):
        cache._refuse(model)


def test_mc_passes_defaults_to_nothing():
    from mmda_amd.config import DEFAULTS, get_config, make_config
    assert DEFAULTS["mc_passes"] == 0 and make_config().mc_passes == 0
    assert get_config(parse=False).mc_passes == 0 and get_config(parse=False, mc_passes=8).mc_passes == 8


# ------------------------------------------------------------------------------------------------ the power check
def _utterances(case):
    cfg, P, batch = inputs_of(case)
    with torch.no_grad():
        o = orc.forward(P, cfg, batch["t"], batch["v"], batch["a"], batch["l"])
    return cfg, P, {"t": o.utterance_t, "v": o.utterance_v, "a": o.utterance_a}


@pytest.mark.parametrize("name", ["fused_b5", "fused_b5_p01", "adv_confid_b6"])
def test_power_draws_differ_and_the_column_index_matters(name):
    """At the configurations of tests/dropout_cases.py, rows repeated K = 3 times: (a) the three draws of every sample differ pairwise
    by at least 100 x that case's ``tol_out`` -- the K copies do see K masks; (b) replacing the (seed, B K) masks by the masks of
    (seed, B) tiled K times -- what a pass that ignored the column index inside a sample's copies would apply -- moves the draws by at
    least 100 x ``tol_out``.  The error measure is the GPU test's (max error relative to the tensor's max)."""
    case = CASES[name]
    K, B = 3, case.B
    cfg, P, utt = _utterances(case)
    rep = {m: v.repeat_interleave(K, dim=0) for m, v in utt.items()}
    rel = lambda a, b: float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-6))
    with torch.no_grad():
        o = orc.fusion_from_utterances(P, cfg, rep, masks=drng.site_masks(cfg, B * K, case.seed, case.p_tf, case.p_cls))
        tiled = {k: v.repeat_interleave(K, dim=0 if k in ("attn", "cls") else 1)
                 for k, v in drng.site_masks(cfg, B, case.seed, case.p_tf, case.p_cls).items()}
        ot = orc.fusion_from_utterances(P, cfg, rep, masks=tiled)
    for what, got, wrong in (("scores", o.scores, ot.scores), ("tcp", o.tcp, ot.tcp)):
        d = got.reshape(B, K, -1)
        apart = min(rel(d[b, i], d[b, j]) for b in range(B) for i in range(K) for j in range(i + 1, K))
        moved = rel(wrong, got)
        print(f"{name} {what}: draws of one sample differ by {apart / case.tol_out:.0f} tolerances, tiled masks move them by "
              f"{moved / case.tol_out:.0f}")
        assert apart >= 100.0 * case.tol_out, (name, what, apart)
        assert moved >= 100.0 * case.tol_out, (name, what, moved)
        w = wrong.reshape(B, K, -1)
        # tiled masks: K equal copies, up to the fp32 rounding of a batched product (far below one tolerance)
        assert float((w[:, 0] - w[:, 1]).abs().max()) < 0.1 * case.tol_out and float((w[:, 0] - w[:, 2]).abs().max()) < 0.1 * case.tol_out


# ------------------------------------------------------------------------------------------------ the GPU test's constants
def test_the_gpu_case_keeps_its_draws_away_from_the_threshold():
    """tests/test_gpu_uncertainty.py compares the vote at EVERY element: no draw of the fp32 oracle at (MC_SEED, K = 3, columns = 16) may
    lie within VOTE_MARGIN = 2e-2 of the threshold (the GPU test skips within 10 x tol_out = 1e-3 and asserts it skipped nothing).
    Also here: both chunk sizes occur, some logits are dropped (a score of exactly 1/2) and some kept, and the entropy figures' slope."""
    from mmda_amd.uncertainty import chunk_plan, chunk_seeds
    cfg = uc.config()
    samples = uc.make_samples()
    assert len(samples) == uc.N and max(len(s[0][0]) for s in samples) == uc.T and min(len(s[0][0]) for s in samples) == 1
    utt = uc.oracle_utterances(samples)
    chunks = chunk_plan(uc.N, uc.K_SMALL, uc.COLUMNS_SMALL)
    assert [len(c) for c in chunks] == [5, 2]
    S, Q = uc.oracle_draws(utt, chunks, chunk_seeds(uc.MC_SEED, len(chunks)), uc.K_SMALL)
    assert S.shape == (uc.N, uc.K_SMALL, 6) and Q.shape == (uc.N, uc.K_SMALL, 6)
    margin = uc.threshold_margin(S, cfg.threshold)
    L = uc.entropy_slope(S)
    print(f"margin {margin:.4f}, entropy slope {L:.3f}, bounds {uc.stat_bounds(S)}")
    assert margin >= uc.VOTE_MARGIN
    dropped = float((S == 0.5).double().mean())
    assert 0.3 < dropped < 0.7                                # p_cls = 0.5
    assert 1.0 < L < 4.0
    # the second chunk's draws are not the first seed's: chunk c runs under seeds[c]
    other, _ = uc.oracle_chunk(utt, chunks[1], uc.K_SMALL, uc.MC_SEED)
    assert float((other - S[5:]).abs().max()) > 100 * uc.TOL_OUT
