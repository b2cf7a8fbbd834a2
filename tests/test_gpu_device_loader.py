"""GPU: the device-resident dataset -- ``mmda_collate_gather`` (one launch per batch), ``DeviceLoader`` and a ``Solver`` fed by it --
against ``mmda_amd.data.collate_fn`` on the same samples in the same order.  The feature only copies, so every comparison is
``torch.equal`` plus dtype and shape: there is no tolerance in this file."""
import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, RandomSampler

pytestmark = pytest.mark.gpu

from oracle import misa_oracle as orc

DEV = "cuda:0"
MOSEI = (35, 74)


def make_samples(lengths, dv, da, seed=0, label_width=7):
    """Reference-style samples; labels in turn: plain normal scores (negative ones among them), one with NaNs, one all zeros."""
    rng = np.random.default_rng(seed)
    out = []
    for i, L in enumerate(lengths):
        lab = rng.normal(size=(1, label_width)).astype(np.float32)
        if i % 4 == 1:
            lab[0, 0] = np.nan
            lab[0, label_width // 2] = np.nan
        if i % 4 == 2:
            lab[:] = 0.0
        if i % 4 == 3:
            lab[:] = -np.abs(lab)
        out.append(((rng.integers(2, 50, size=L), rng.normal(size=(L, dv)).astype(np.float32),
                     rng.normal(size=(L, da)).astype(np.float32), ["w"] * L), lab, f"seg{i}"))
    return out


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _same(got, ref, what):
    assert got.dtype == ref.dtype and tuple(got.shape) == tuple(ref.shape), (what, got.dtype, ref.dtype, tuple(got.shape), tuple(ref.shape))
    assert torch.equal(got.cpu(), ref), what


def _same_batch(got, ref, what):
    """all ten slots of the reference's tuple"""
    assert len(got) == len(ref) == 10
    for i, name in zip(range(4), ("ids", "visual", "acoustic", "labels")):
        assert got[i].is_cuda, name
        _same(got[i], ref[i], (what, name))
    if ref[4] is None:
        assert got[4] is None, what
    else:
        assert got[4].is_cuda
        _same(got[4], ref[4], (what, "emo"))
    assert not got[5].is_cuda and got[5].dtype == torch.int64
    _same(got[5], ref[5], (what, "lengths"))
    for i in (6, 7, 8):
        _same(got[i], ref[i], (what, "bert", i))
    assert got[9] == ref[9], what


# ------------------------------------------------------------------------------------------------ 1: the launch
SHAPES = {
    "B1_T1": [1],
    "B1_T9": [9],
    "B4_T9_ties": [9, 4, 9, 4],
    "B8_T9_ragged": [3, 9, 1, 5, 2, 7, 1, 4],
    "B8_T9_full": [9] * 8,
}


def _gather_with_sentinels(ds, order, T):
    from mmda_amd import ops
    B = len(order)
    out = (torch.full((T, B), -7, dtype=torch.int64, device=DEV), torch.full((T, B, ds.dv), float("nan"), device=DEV),
           torch.full((T, B, ds.da), float("nan"), device=DEV),
           None if ds.emo is None else torch.full((B, 6), float("nan"), device=DEV), torch.full((B,), float("nan"), device=DEV))
    o = torch.from_numpy(order.astype(np.int32)).to(DEV)
    got = ops.collate_gather(ds.words, ds.visual, ds.acoustic, ds.offsets, ds.emo, ds.sentiment, o, T, out=out)
    assert all(g is x for g, x in zip(got, out))
    return got


def _check_op(lengths, dv, da, label_width=7):
    """Every output element was a sentinel (NaN / -7) that no collated batch holds: equality proves the launch wrote them all, the
    padding included."""
    from mmda_amd import DeviceDataset, batch_plan
    from mmda_amd.data import collate_fn
    samples = make_samples(lengths, dv, da, seed=len(lengths), label_width=label_width)
    ds = DeviceDataset.from_samples(samples, DEV)
    ref = collate_fn(list(samples))
    order, bounds = batch_plan(ds.lengths, np.arange(len(samples)), len(samples))
    assert bounds.tolist() == [0, len(samples)]
    T = int(ds.lengths[order[0]])
    ids, v, a, emo, y = _gather_with_sentinels(ds, order, T)
    _same(ids, ref[0], "ids"); _same(v, ref[1], "visual"); _same(a, ref[2], "acoustic"); _same(y, ref[3], "labels")
    if label_width == 7:
        _same(emo, ref[4], "emo")
    else:
        assert emo is None and ref[4] is None and ds.emo is None
    assert [ds.segments[i] for i in order] == ref[9] and ds.lengths[order].tolist() == ref[5].tolist()
    return ds, order, ref


@pytest.mark.parametrize("widths", [MOSEI, (5, 3)])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_gather_equals_collate_fn(shape, widths):
    _check_op(SHAPES[shape], *widths)


@pytest.mark.parametrize("B", [64, 256])
def test_gather_with_more_work_than_the_grid_holds(B):
    """B = 64, T = 50 at MOSEI widths: more elements than the launch has threads.  B = 256, T = 50: the launch is capped at 2048
    workgroups (64 columns of four waves x 32 rows of t), so every wave takes a second trip through its t loop."""
    lengths = np.random.default_rng(B).integers(1, 51, size=B)
    lengths[B // 3] = 50
    _check_op(lengths.tolist(), *MOSEI)


def test_gather_pads_whole_time_steps_and_cuts_at_T():
    """T is the caller's: beyond every length the launch writes padding only; below a length it stops at T."""
    from mmda_amd import DeviceDataset
    from mmda_amd.data import collate_fn
    samples = make_samples([4, 2, 3], 5, 3)
    ds = DeviceDataset.from_samples(samples, DEV)
    ref = collate_fn(list(samples))
    order = np.array([0, 2, 1])
    ids, v, a, emo, y = _gather_with_sentinels(ds, order, 6)
    _same(ids[:4], ref[0], "ids"); _same(v[:4], ref[1], "visual"); _same(a[:4], ref[2], "acoustic")
    assert bool((ids[4:] == 1).all()) and bool((v[4:] == 0).all()) and bool((a[4:] == 0).all())
    ids, v, a, emo, y = _gather_with_sentinels(ds, order, 2)
    _same(ids, ref[0][:2], "ids"); _same(v, ref[1][:2], "visual"); _same(a, ref[2][:2], "acoustic")
    _same(emo, ref[4], "emo"); _same(y, ref[3], "labels")


def test_gather_takes_a_repeated_sample():
    from mmda_amd import DeviceDataset
    from mmda_amd.data import collate_fn
    samples = make_samples([4, 2, 3], 5, 3)
    ds = DeviceDataset.from_samples(samples, DEV)
    ref = collate_fn([samples[0], samples[2], samples[2], samples[1]])
    ids, v, a, emo, y = _gather_with_sentinels(ds, np.array([0, 2, 2, 1]), 4)
    for g, r in zip((ids, v, a, y, emo), ref[:5]):
        _same(g, r, "repeat")


def test_dataset_without_emotion_labels_yields_none():
    from mmda_amd import DeviceLoader
    ds, order, ref = _check_op(SHAPES["B8_T9_ragged"], *MOSEI, label_width=1)
    (batch,) = list(DeviceLoader(ds, 8))
    assert batch[4] is None
    _same_batch(batch, ref, "no emo")


def test_bad_arguments_are_refused_without_a_launch():
    from mmda_amd import DeviceDataset, _lib
    lib = _lib.load()
    ds = DeviceDataset.from_samples(make_samples([3, 2], 5, 3), DEV)
    B, T = 2, 3
    order = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    outs = [torch.full((T, B), -7, dtype=torch.int64, device=DEV), torch.full((T, B, 5), float("nan"), device=DEV),
            torch.full((T, B, 3), float("nan"), device=DEV), torch.full((B, 6), float("nan"), device=DEV),
            torch.full((B,), float("nan"), device=DEV)]
    before = [x.clone() for x in outs]
    good = [_lib.ptr(x) for x in (ds.words, ds.visual, ds.acoustic, ds.offsets, ds.emo, ds.sentiment, order)] + [B, T, 5, 3, 1] + \
           [x.data_ptr() for x in outs] + [_lib.stream_ptr()]
    EINVAL = -1
    for k in (0, 1, 2, 3, 5, 6, 12, 13, 14, 16):                     # every pointer but emo / out_emo
        bad = list(good); bad[k] = None
        assert lib.mmda_collate_gather(*bad) == EINVAL, k
    for k in (7, 8, 9, 10):                                          # B, T, dv, da
        for val in (0, -1):
            bad = list(good); bad[k] = val
            assert lib.mmda_collate_gather(*bad) == EINVAL, (k, val)
    bad = list(good); bad[4] = None                                  # out_emo asked of a dataset without emo
    assert lib.mmda_collate_gather(*bad) == EINVAL
    torch.cuda.synchronize()
    for x, y in zip(outs, before):                                   # nothing ran
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    ok = list(good); ok[15] = None                                   # emo without out_emo is a request for fewer outputs
    assert lib.mmda_collate_gather(*ok) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(outs[3]).all()) and not bool(torch.isnan(outs[4]).any())


# ------------------------------------------------------------------------------------------------ 2: the loader
N = 37


@pytest.fixture(scope="module")
def corpus():
    from mmda_amd import DeviceDataset
    lengths = np.random.default_rng(5).integers(1, 10, size=N)
    samples = make_samples(lengths, *MOSEI, seed=1)
    return samples, DeviceDataset.from_samples(samples, DEV)


@pytest.mark.parametrize("drop_last", [False, True])
def test_epoch_equals_dataloader_with_the_same_sampler(corpus, drop_last):
    from mmda_amd import DeviceLoader
    from mmda_amd.data import collate_fn
    samples, ds = corpus
    ref = list(DataLoader(samples, batch_size=8, sampler=RandomSampler(samples, generator=_gen(3)), collate_fn=collate_fn,
                          drop_last=drop_last))
    ld = DeviceLoader(ds, 8, sampler=RandomSampler(samples, generator=_gen(3)), drop_last=drop_last)
    got = list(ld)
    assert len(got) == len(ref) == len(ld) == (4 if drop_last else 5)
    assert got[-1][0].shape[1] == (8 if drop_last else N % 8)        # the tail batch is there
    for k, (g, r) in enumerate(zip(got, ref)):
        _same_batch(g, r, k)
    assert got[0][6] is got[0][7] is got[0][8]                       # one cached placeholder, as collate_fn shares one


def test_shuffled_epoch_equals_randperm(corpus):
    from mmda_amd import DeviceLoader
    from mmda_amd.data import collate_fn
    samples, ds = corpus
    perm = torch.randperm(N, generator=_gen(11)).tolist()
    got = list(DeviceLoader(ds, 8, shuffle=True, generator=_gen(11)))
    assert len(got) == 5
    for k, g in enumerate(got):
        _same_batch(g, collate_fn([samples[i] for i in perm[8 * k:8 * k + 8]]), k)
    plain = list(DeviceLoader(ds, 8))                                # no shuffle: 0 .. n-1
    for k, g in enumerate(plain):
        _same_batch(g, collate_fn(samples[8 * k:8 * k + 8]), k)


def test_two_epochs_of_one_generator_differ_and_cover_the_same_samples(corpus):
    from mmda_amd import DeviceLoader
    samples, ds = corpus
    ld = DeviceLoader(ds, 8, shuffle=True, generator=_gen(2))
    e1 = [s for b in ld for s in b[9]]
    e2 = [s for b in ld for s in b[9]]
    assert e1 != e2
    assert sorted(e1) == sorted(e2) == sorted(s[2] for s in samples)


def test_a_batch_written_into_leaves_the_later_batches_alone(corpus):
    """Every tensor of a yielded tuple but the BERT placeholder is the batch's own, as collate_fn's are: a consumer that overwrites a
    batch in place (the lengths are a CPU tensor cut from the epoch's plan) changes nothing that comes after it."""
    from mmda_amd import DeviceLoader
    from mmda_amd.data import collate_fn
    samples, ds = corpus
    ref = list(DataLoader(samples, batch_size=8, collate_fn=collate_fn))
    got = []
    for batch in DeviceLoader(ds, 8):
        got.append(tuple(x.clone() if torch.is_tensor(x) else x for x in batch))
        for x in batch[:6]:
            x.fill_(-3)
    torch.cuda.synchronize()
    for k, (g, r) in enumerate(zip(got, ref)):
        _same_batch(g, r, k)


def test_shards_yield_equal_batch_counts_on_the_device(corpus):
    from mmda_amd import DeviceLoader
    samples, ds = corpus
    seen = []
    for r in range(2):
        ld = DeviceLoader(ds, 4, shuffle=True, generator=_gen(4), shard=(r, 2))
        batches = list(ld)
        assert len(batches) == len(ld) == 5
        seen.append({s for b in batches for s in b[9]})
    assert not seen[0] & seen[1] and len(seen[0] | seen[1]) == 36


def test_iterating_does_not_synchronise(corpus):
    """A warmed loader (allocator blocks and placeholders cached) runs a whole epoch, the epoch's upload included, with torch's
    synchronisation check armed."""
    from mmda_amd import DeviceLoader
    samples, ds = corpus
    ld = DeviceLoader(ds, 8, shuffle=True, generator=_gen(6))
    for _ in ld:
        pass
    probe = torch.ones(1, device=DEV)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()                                             # the check is live in this build
        n = 0
        for batch in ld:
            n += 1
        assert n == 5
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 3: under the Solver
class ListLoader:
    def __init__(self, batches):
        self.batches = batches
        self.dataset = self

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


def _solver_corpus():
    """20 samples; every sample has at least one class at a positive score and the batches below hold every class"""
    from mmda_amd import DeviceDataset
    lengths = np.random.default_rng(8).integers(1, 10, size=20)
    samples = make_samples(lengths, *MOSEI, seed=2)
    for i, s in enumerate(samples):
        s[1][0, 1 + i % 6] = 1.0
        s[1][0, 1 + (i + 3) % 6] = 0.5
    return samples, DeviceDataset.from_samples(samples, DEV)


def _solver(train, dev, precision="fp32"):
    from mmda_amd import make_config, models
    from mmda_amd.solver import Solver
    cfg = orc.default_config(vocab_size=120, learning_rate=1e-3, clip=1.0)
    c = make_config(precision=precision, device=DEV, n_epoch=1, name="device_loader", **vars(cfg))
    m = models.MISA(c)
    m.load_state_dict(orc.synth_params(cfg, 21))
    torch.manual_seed(0)                                             # build() draws the orthogonal recurrent weights
    return Solver(c, c, c, train, dev, ListLoader([]), is_train=True, model=m).build()


def _state(m):
    P, _, M, V = m.flat_buckets()
    torch.cuda.synchronize()
    return [x.detach().cpu().clone() for x in (P, M, V)]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_solver_trains_to_the_same_bits_from_either_source(precision):
    """One epoch whose three batches have three different T (and a short tail).  bf16 is the default precision of the product path and
    runs the resident-weights recurrences; every reduction of the step is deterministic in either precision (tests/test_gpu_solver.py),
    so equal batches give equal bits."""
    from mmda_amd import DeviceLoader
    from mmda_amd.data import collate_fn
    samples, ds = _solver_corpus()
    host = list(DataLoader(samples, batch_size=8, sampler=RandomSampler(samples, generator=_gen(7)), collate_fn=collate_fn))
    assert [b[0].shape[1] for b in host] == [8, 8, 4] and len({b[0].shape[0] for b in host}) == 3     # three T: the workspace is re-cut
    assert all(bool((b[4].sum(0) > 0).all()) for b in host)          # every class occurs in every batch: the losses stay finite
    a = _solver(DeviceLoader(ds, 8, sampler=RandomSampler(samples, generator=_gen(7))), ListLoader([]), precision)
    b = _solver(ListLoader(host), ListLoader([]), precision)
    a.model._materialize(torch.device(DEV)); b.model._materialize(torch.device(DEV))
    for x, y in zip(_state(a.model), _state(b.model)):
        assert torch.equal(x, y)                                     # the same start
    start = _state(a.model)[0]
    la, lb = a.train_epoch(), b.train_epoch()
    assert a.model._step == b.model._step == 3 and not a.model.cluster_aborted()
    assert la == lb and all(v == v for v in la.values())
    for name, x, y in zip("PMV", _state(a.model), _state(b.model)):
        assert torch.equal(x, y), (name, int((x != y).sum()))
    assert not torch.equal(start, _state(a.model)[0])                # ... and it did train


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_solver_eval_gives_the_same_results_from_either_source(precision):
    from mmda_amd import DeviceLoader
    from mmda_amd.data import collate_fn
    samples, ds = _solver_corpus()
    host = list(DataLoader(samples, batch_size=8, collate_fn=collate_fn))
    s = _solver(ListLoader([]), DeviceLoader(ds, 8), precision)
    loss_a, acc_a, pred_a, true_a = s.eval("dev")
    s.dev_data_loader = ListLoader(host)
    loss_b, acc_b, pred_b, true_b = s.eval("dev")
    assert loss_a == loss_b and acc_a == acc_b and loss_a == loss_a and not s.model.cluster_aborted()
    assert pred_a.shape == pred_b.shape == (20, 6) and np.array_equal(pred_a, pred_b) and np.array_equal(true_a, true_b)
