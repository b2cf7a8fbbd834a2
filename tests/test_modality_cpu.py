"""CPU: the host side of modality masking (mmda_amd/modality.py) -- the numpy restatement of the random keep sets
against the oracle's generator, the all-dropped rule, the drop rates, keep-set parsing, the refusal over the encoder cache, the
loader's argument checks -- and the references tests/test_gpu_modality.py compares the device with."""
import numpy as np
import pytest

from mmda_amd import DeviceLoader, modality, step_rules
from mmda_amd._lib import MMDAError
from oracle import dropout_rng

import modality_cases as mc

SEEDS = (0, 1, 2 ** 63 + 5)


def _indices():
    return np.concatenate([np.arange(0, 300), np.array([2 ** 20 + 1, 2 ** 31 - 1, 2 ** 31], dtype=np.int64)])


def _keep_from_oracle(seed, p, s):
    """keep sets from oracle.dropout_rng.rng_u32(seed, 11, 3 s + m), spelled with Python ints and one fp32 compare per draw"""
    out = []
    for i in s.tolist():
        drop = 0
        for m in range(3):
            u = np.float32(int(dropout_rng.rng_u32(seed, 11, 3 * i + m)) >> 8) * np.float32(2.0 ** -24)
            if np.float32(p[m]) > 0 and u < np.float32(p[m]):
                drop |= 1 << m
        out.append(7 if drop == 7 else 7 & ~drop)
    return np.array(out, dtype=np.uint8)


@pytest.mark.parametrize("seed", SEEDS)
def test_keep_bits_agree_with_the_oracle_generator(seed):
    s = _indices()
    assert modality.SITE_MODALITY == 11 and 11 not in dropout_rng.SITES.values()
    assert np.array_equal(modality._rng_u32(seed, 11, s), dropout_rng.rng_u32(seed, 11, s))
    for p in ((0.5, 0.5, 0.5), (0.1, 0.0, 0.9), (0.999, 0.999, 0.999)):
        got = modality.keep_bits(seed, p, s)
        assert got.dtype == np.uint8 and got.shape == s.shape
        assert np.array_equal(got, _keep_from_oracle(seed, p, s)), p
    assert modality.keep_bits(seed, (0.5, 0.5, 0.5), s.reshape(3, 101)).shape == (3, 101)


@pytest.mark.parametrize("seed", SEEDS)
def test_no_rate_keeps_everything(seed):
    assert np.all(modality.keep_bits(seed, (0.0, 0.0, 0.0), _indices()) == 7)


def test_a_sample_is_never_emptied_by_chance():
    k = modality.keep_bits(3, (0.999, 0.999, 0.999), np.arange(20000))
    assert not np.any(k == 0)
    bits = np.array([bin(int(x)).count("1") for x in range(8)])[k]
    assert set(np.unique(bits).tolist()) <= {1, 2, 3} and np.all(k[bits == 3] == 7)
    assert np.mean(k == 7) > 0.99                                     # nearly every draw drops all three, and is undone


def test_drop_rates():
    """seed 0, n = 30 000, p = (0.1, 0.3, 0.5): the dropped share of modality m within 4 sigma of p_m - p_t p_v p_a (an all-dropped draw
    drops nothing), the share of all-dropped draws within 4 sigma of p_t p_v p_a, sigma = sqrt(q (1 - q) / n)."""
    n, p = 30000, (0.1, 0.3, 0.5)
    s = np.arange(n)
    k = modality.keep_bits(0, p, s)
    all3 = float(np.prod(p))
    for m in range(3):
        q = p[m] - all3
        share = float(np.mean((k >> m & 1) == 0))
        z = (share - q) / np.sqrt(q * (1 - q) / n)
        print(f"modality {m}: dropped share {share:.5f}, expected {q:.5f}, {z:+.2f} sigma")
        assert abs(z) <= 4.0, (m, share, q, z)
    raw = np.ones(n, dtype=bool)                                      # the draws that would have dropped all three, from the oracle
    for m in range(3):
        u = (dropout_rng.rng_u32(0, 11, 3 * s + m) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
        raw &= u < np.float32(p[m])
    z = (float(raw.mean()) - all3) / np.sqrt(all3 * (1 - all3) / n)
    print(f"all-dropped draws: {int(raw.sum())}, {z:+.2f} sigma")
    assert abs(z) <= 4.0 and np.all(k[raw] == 7)


def test_keep_set_parsing():
    pk = modality.parse_keep
    assert pk(None) == 7 and [pk(k) for k in range(8)] == list(range(8)) and pk(np.int64(5)) == 5
    assert pk("text") == 1 and pk("visual") == 2 and pk("acoustic") == 4
    assert pk(("text", "acoustic")) == 5 and pk(["visual", "visual", "text"]) == 3 and pk({"text", "visual", "acoustic"}) == 7
    assert pk(()) == 0
    for bad in (8, -1, True, "audio", ("text", "video"), (1, 2), 1.0):
        with pytest.raises((ValueError, TypeError)):
            pk(bad)
    assert modality.keep_names(5) == ("text", "acoustic") and modality.keep_names(0) == ()


def test_the_encoder_cache_refuses_a_keep_set_by_name():
    assert [n for n, _ in step_rules.MODALITY_RULES] == ["modality_encoded"]
    assert step_rules.modality_verdict(None, encoded=True) is None
    assert step_rules.modality_verdict(7, encoded=True) is None
    assert step_rules.modality_verdict(3, encoded=False) is None
    for k in range(7):
        assert step_rules.modality_verdict(k, encoded=True) == ("modality_encoded", dict(keep=k))
    step_rules.modality_check(7, encoded=True)
    with pytest.raises(MMDAError, match="encoder cache") as e:
        step_rules.modality_check(5, encoded=True)
    assert str(e.value) == dict(step_rules.MODALITY_RULES)["modality_encoded"].format(keep=5)


def test_loader_arguments_are_checked_without_a_device():
    class Stub:
        lengths = np.ones(10, dtype=np.int64)

        def __len__(self):
            return 10

    ld = DeviceLoader(Stub(), 4)
    assert ld.modality_dropout is None and ld.keep is None and not ld.masked and ld.epoch == 0 and ld.last_keep is None
    ld = DeviceLoader(Stub(), 4, modality_dropout=(0.1, 0, 0.5), modality_seed=2 ** 64 - 1, keep=("text", "visual"))
    assert ld.modality_dropout == (0.1, 0.0, 0.5) and ld.keep == 3 and ld.masked and len(ld) == 3
    assert DeviceLoader(Stub(), 4, keep=0).masked and DeviceLoader(Stub(), 4, modality_dropout=(0, 0, 0)).masked
    ld.set_epoch(5)
    assert ld.epoch == 5
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError):
            ld.set_epoch(bad)
    for bad in ((0.1, 0.2), (0.1, 0.2, 1.0), (-0.1, 0, 0), (0.1, 0.2, float("nan")), 0.3, ("a", "b", "c")):
        with pytest.raises(ValueError):
            DeviceLoader(Stub(), 4, modality_dropout=bad)
    for bad in (8, "audio"):
        with pytest.raises(ValueError):
            DeviceLoader(Stub(), 4, keep=bad)
    with pytest.raises(ValueError):
        DeviceLoader(Stub(), 4, modality_seed=1.5)


def test_shapley_references_agree_and_are_efficient():
    """The permutation form (tests/modality_cases.py) against the subset form with the kernel's weights (mmda_amd.modality.shapley3),
    both float64; efficiency, the null player and symmetry on constructed games."""
    V = mc.attrib_values(65, 6, 1, -3.0, 3.0)
    phi, loo = modality.shapley3(V)
    assert np.allclose(phi, mc.shapley_ref(V), rtol=0, atol=1e-14) and np.array_equal(loo, mc.loo_ref(V))
    assert np.allclose(phi.sum(0), V[7].astype(np.float64) - V[0], rtol=0, atol=1e-14)
    W = V.copy()
    for S in range(8):
        W[S] = V[S & ~2]                                              # visual changes nothing
    assert np.all(mc.shapley_ref(W)[1] == 0.0)
    add = np.stack([sum(float(w) for m, w in enumerate((0.5, -1.25, 2.0)) if S >> m & 1) * np.ones((3, 2)) for S in range(8)])
    assert np.allclose(mc.shapley_ref(add)[:, 0, 0], (0.5, -1.25, 2.0))   # an additive game gives every player its own weight
    dom, counts = mc.dominant_ref(np.array([[[1.0], [1.0], [0.5]], [[np.nan], [0.0], [0.0]], [[np.nan], [np.nan], [np.nan]]]))
    assert dom[:, 0].tolist() == [0, 1, -1] and counts[:, 0].tolist() == [1, 1, 0]


def test_host_mask_agrees_with_the_length_form():
    from mmda_amd.data import collate_fn
    t, v, a, _, _, l, *_ = collate_fn(mc.make_samples([3, 9, 1, 5], 5, 3))
    keep = np.array([0, 5, 3, 6], dtype=np.uint8)
    for k in (keep, 0, 2, 7):
        got, ref = modality.mask_batch(t.numpy(), v.numpy(), a.numpy(), k), mc.mask_ref(t.numpy(), v.numpy(), a.numpy(), l.numpy(), k)
        assert all(np.array_equal(g, r) for g, r in zip(got, ref))
    ids0 = modality.mask_batch(t.numpy(), v.numpy(), a.numpy(), 6)[0]
    assert np.all(ids0[t.numpy() == mc.PAD] == mc.PAD) and np.all(ids0[t.numpy() != mc.PAD] == mc.UNK)


def test_bench_tool_parent_assembles_and_writes_its_document(tmp_path, monkeypatch, capsys):
    """tools/bench_modality.py, the parent process: one measuring child per worker, each with the time limit, the GPU never opened
    here; one JSON document printed and written; a child that fails or runs out of time ends the run with its name."""
    import importlib.util
    import json
    import os
    import subprocess
    import sys
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "bench_modality.py")
    spec = importlib.util.spec_from_file_location("bench_modality", path)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    seen = []

    def fake_run(cmd, **kw):
        w = cmd[cmd.index("--worker") + 1]
        seen.append((w, kw["timeout"]))
        return subprocess.CompletedProcess(cmd, 3 if w == "fail" else 0, stdout="noise\n" + json.dumps(
            {"worker": w, "device": "stub", "result": [{"w": w}]}) + "\n")

    monkeypatch.setattr(subprocess, "run", fake_run)
    out = tmp_path / "profiles" / "modality.json"
    monkeypatch.setattr(sys, "argv", ["bench_modality.py", "--out", str(out), "--step-timeout", "7"])
    tool.main()
    assert seen == [("gather", 7), ("pass", 7), ("attrib", 7)]
    doc = json.loads(out.read_text())
    assert doc == json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert doc == {"bench": "modality", "device": "stub", "gather": [{"w": "gather"}], "pass": [{"w": "pass"}], "attrib": [{"w": "attrib"}]}
    monkeypatch.setattr(tool, "WORKERS", ("gather", "fail"))
    with pytest.raises(SystemExit, match="fail: exit status 3"):
        tool.main()

    def slow_run(cmd, **kw):
        raise subprocess.TimeoutExpired(cmd, kw["timeout"])

    monkeypatch.setattr(subprocess, "run", slow_run)
    with pytest.raises(SystemExit, match="gather: no result after 7 s"):
        tool.main()
