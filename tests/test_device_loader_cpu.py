"""CPU: the host side of the device-resident dataset (mmda_amd/data.py: batch_plan, DeviceDataset.from_samples' argument checks).
``batch_plan`` is compared with what a real ``torch.utils.data.DataLoader`` hands to ``collate_fn`` for the same sampler seed: per batch the
segment order (ties in length included), the lengths and T.  No tolerance anywhere: the plan is integers."""
import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, RandomSampler

from mmda_amd import DeviceDataset, DeviceLoader, batch_plan
from mmda_amd.data import collate_fn
from mmda_amd._lib import MMDAError

N = 37


def make_samples(lengths, dv=35, da=74, seed=0, label_width=7):
    rng = np.random.default_rng(seed)
    out = []
    for i, L in enumerate(lengths):
        lab = rng.normal(size=(1, label_width)).astype(np.float32)
        out.append(((rng.integers(2, 50, size=L), rng.normal(size=(L, dv)).astype(np.float32),
                     rng.normal(size=(L, da)).astype(np.float32), ["w"] * L), lab, f"seg{i}"))
    return out


@pytest.fixture(scope="module")
def dataset():
    lengths = np.random.default_rng(5).integers(1, 10, size=N)            # 37 samples over 9 lengths: ties in every batch of 8
    return lengths.astype(np.int64), make_samples(lengths, dv=5, da=3)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("drop_last", [False, True])
@pytest.mark.parametrize("batch_size", [1, 4, 8])
def test_batch_plan_matches_dataloader_with_collate_fn(dataset, batch_size, drop_last):
    lengths, samples = dataset
    assert len(np.unique(lengths)) < N
    dl = DataLoader(samples, batch_size=batch_size, sampler=RandomSampler(samples, generator=_gen(3)), collate_fn=collate_fn,
                    drop_last=drop_last)
    ref = list(dl)
    indices = list(RandomSampler(samples, generator=_gen(3)))
    order, bounds = batch_plan(lengths, indices, batch_size, drop_last=drop_last)
    assert order.dtype == np.int64 and bounds.dtype == np.int64
    assert len(bounds) - 1 == len(ref) == len(dl)
    assert len(ref) == (N // batch_size if drop_last else -(-N // batch_size))
    if not drop_last and N % batch_size:
        assert bounds[-1] - bounds[-2] == N % batch_size                    # the short tail is there
    for k, batch in enumerate(ref):
        mine = order[bounds[k]:bounds[k + 1]]
        assert [f"seg{i}" for i in mine] == batch[9], k                      # the order inside the batch, ties included
        assert lengths[mine].tolist() == batch[5].tolist(), k
        assert int(lengths[mine[0]]) == batch[0].shape[0], k                 # T
        assert len(mine) == batch[0].shape[1], k                             # B
    kept = N // batch_size * batch_size if drop_last else N
    assert sorted(order.tolist()) == sorted(indices[:kept])


def test_batch_plan_takes_repeated_indices_and_an_empty_sequence():
    lengths = np.array([3, 1, 2], dtype=np.int64)
    order, bounds = batch_plan(lengths, [1, 1, 0, 2, 1], 2)
    assert order.tolist() == [1, 1, 0, 2, 1] and bounds.tolist() == [0, 2, 4, 5]
    order, bounds = batch_plan(lengths, [], 2)
    assert order.size == 0 and bounds.tolist() == [0]


@pytest.mark.parametrize("drop_last", [False, True])
@pytest.mark.parametrize("world", [2, 3])
def test_shards_are_disjoint_equal_in_count_and_cover_the_truncated_prefix(dataset, world, drop_last):
    lengths, _ = dataset
    bs = 4
    indices = torch.randperm(N, generator=_gen(9)).numpy()
    plans = [batch_plan(lengths, indices, bs, drop_last=drop_last, shard=(r, world)) for r in range(world)]
    counts = {len(b) - 1 for _, b in plans}
    assert len(counts) == 1 and counts.pop() > 0                             # the ranks' collectives line up
    assert all(b.tolist() == plans[0][1].tolist() for _, b in plans)         # batch by batch the same B on every rank
    unit = world * bs if drop_last else world
    prefix = indices[:N // unit * unit]
    sets = [set(o.tolist()) for o, _ in plans]
    for r in range(world):
        assert sets[r] == set(prefix[r::world].tolist())
        for q in range(r):
            assert not sets[r] & sets[q]
    assert sorted(np.concatenate([o for o, _ in plans]).tolist()) == sorted(prefix.tolist())
    if drop_last:
        assert all(np.all(np.diff(b) == bs) for _, b in plans)


def test_shard_arguments_are_checked():
    lengths = np.ones(8, dtype=np.int64)
    for shard in ((2, 2), (-1, 2), (0, 0)):
        with pytest.raises(ValueError):
            batch_plan(lengths, np.arange(8), 2, shard=shard)
    with pytest.raises(ValueError):
        batch_plan(lengths, np.arange(8), 0)


@pytest.mark.parametrize("bad", [[0, 1, 37], [0, -1, 2], [10 ** 12]])
def test_out_of_range_and_negative_indices_raise(dataset, bad):
    lengths, _ = dataset
    with pytest.raises(IndexError):
        batch_plan(lengths, bad, 4)
    with pytest.raises(IndexError):
        batch_plan(lengths, bad, 4, shard=(0, 2))                            # also where the shard would not keep the bad entry


def test_device_dataset_refuses_the_cpu(dataset):
    _, samples = dataset
    with pytest.raises(MMDAError):
        DeviceDataset.from_samples(samples, "cpu")
    with pytest.raises(MMDAError):
        DeviceDataset.from_samples(samples, torch.device("cpu"))


def test_device_dataset_checks_its_samples_before_any_upload():
    good = make_samples([3, 2, 4], dv=5, da=3)
    with pytest.raises(ValueError):
        DeviceDataset.from_samples([], "cuda")
    zero = make_samples([3, 0, 4], dv=5, da=3)
    with pytest.raises(ValueError):
        DeviceDataset.from_samples(zero, "cuda")
    with pytest.raises(ValueError):
        DeviceDataset.from_samples(good + make_samples([2], dv=6, da=3), "cuda")       # visual width differs
    with pytest.raises(ValueError):
        DeviceDataset.from_samples(good + make_samples([2], dv=5, da=4), "cuda")       # acoustic width differs
    (w, v, a, words), lab, seg = good[0]
    with pytest.raises(ValueError):
        DeviceDataset.from_samples([((w, v[:2], a, words), lab, seg)], "cuda")          # features shorter than the word ids


def test_loader_length_follows_the_plan(dataset):
    """__len__ without a device: the loader only reads len(dataset) / len(sampler) for it."""
    lengths, _ = dataset

    class Stub:
        def __len__(self):
            return N

    Stub.lengths = lengths
    for bs in (1, 4, 8):
        for drop_last in (False, True):
            for shard in (None, (0, 2), (2, 3)):
                ld = DeviceLoader(Stub(), bs, drop_last=drop_last, shard=shard)
                _, bounds = batch_plan(lengths, np.arange(N), bs, drop_last=drop_last, shard=shard)
                assert len(ld) == len(bounds) - 1, (bs, drop_last, shard)
    assert len(DeviceLoader(Stub(), 4, sampler=list(range(10)))) == 3
    with pytest.raises(ValueError):
        DeviceLoader(Stub(), 4, shuffle=True, sampler=list(range(10)))


def test_bench_tool_parent_assembles_and_writes_its_document(tmp_path, monkeypatch, capsys):
    """tools/bench_input_pipeline.py, the parent process: it starts the one measuring child with a time limit, never opens the GPU
    itself, and prints and writes one JSON document; a child that fails or runs out of time ends the run with its name."""
    import importlib.util
    import json
    import os
    import subprocess
    import sys
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "bench_input_pipeline.py")
    spec = importlib.util.spec_from_file_location("bench_input_pipeline", path)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    rows = [{"batch": 32, "T": 50, "lengths": "ragged", "us_per_launch": {"min": 1.0, "median": 2.0, "max": 3.0, "rounds": [2.0, 1.0, 3.0]}}]
    seen = {}

    def fake_run(cmd, **kw):
        seen["cmd"], seen["kw"] = cmd, kw
        return subprocess.CompletedProcess(cmd, seen.get("rc", 0), stdout="noise\n" + json.dumps(
            {"worker": "gather", "device": "stub", "result": rows}) + "\n")

    monkeypatch.setattr(subprocess, "run", fake_run)
    out = tmp_path / "profiles" / "input_pipeline.json"
    monkeypatch.setattr(sys, "argv", ["bench_input_pipeline.py", "--out", str(out), "--step-timeout", "7"])
    tool.main()
    assert seen["cmd"][2:4] == ["--worker", "gather"] and seen["kw"]["timeout"] == 7
    assert "stderr" not in seen["kw"]                                # the child's progress lines go straight to the terminal
    doc = json.loads(out.read_text())
    assert doc == json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert doc["gather"] == rows and doc["device"] == "stub" and doc["epoch_rates"] is None
    seen["rc"] = 3
    with pytest.raises(SystemExit, match="gather: exit status 3"):
        tool.main()

    def slow_run(cmd, **kw):
        raise subprocess.TimeoutExpired(cmd, kw["timeout"])

    monkeypatch.setattr(subprocess, "run", slow_run)
    with pytest.raises(SystemExit, match="gather: no result after 7 s"):
        tool.main()
    assert tool._range([3.0, 1.0, 2.0]) == {"min": 1.0, "median": 2.0, "max": 3.0, "rounds": [3.0, 1.0, 2.0]}
    s = tool.synth_samples(5, 0)
    assert [x[0][1].shape[1] for x in s] == [35] * 5 and all(5 <= len(x[0][0]) <= 50 for x in s) and s[0][1].shape == (1, 7)
