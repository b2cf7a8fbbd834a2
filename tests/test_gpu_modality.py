"""GPU: modality masking (mmda_amd/modality.py, csrc/modality.hip) -- the masked gather, the out-of-place mask, the
loader's modality dropout, the Shapley collector and the pass over the eight keep sets.

Where the kernels copy, the checks are ``torch.equal`` plus dtype and shape: no tolerance.  The one computed quantity, ``phi`` / ``loo``
of ``mmda_modality_attrib``, is held to ``2^-19 max(1, max |V|)`` against float64 (tests/modality_cases.py: ``attrib_bound``)."""
import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, RandomSampler

pytestmark = pytest.mark.gpu

import modality_cases as mc
from oracle import misa_oracle as orc

DEV = "cuda:0"
P_HALF = (0.5, 0.5, 0.5)
SEEDS = (0, 2 ** 63 + 5)


def _same(got, ref, what):
    ref = torch.as_tensor(ref)
    assert got.dtype == ref.dtype and tuple(got.shape) == tuple(ref.shape), (what, got.dtype, ref.dtype, tuple(got.shape), tuple(ref.shape))
    assert torch.equal(got.cpu(), ref), what


def _gen(seed):
    return torch.Generator().manual_seed(seed)


class ListLoader:
    def __init__(self, batches):
        self.batches = batches
        self.dataset = self

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


# ------------------------------------------------------------------------------------------------ 1: the masked gather
def _case(shape, widths):
    """A dataset of one extra sample followed by the case's, and an order over the case's samples that is not the identity and names
    the dataset's last index; the collated reference of the ordered samples."""
    from mmda_amd import DeviceDataset
    from mmda_amd.data import collate_fn
    lengths = [4] + mc.LENGTH_LISTS[shape]
    samples = mc.make_samples(lengths, *widths, seed=len(lengths))
    ds = DeviceDataset.from_samples(samples, DEV)
    n = len(samples)
    pick = np.arange(n - 1, 0, -1, dtype=np.int64)                   # reversed, sample 0 left out
    pick = pick[np.argsort(-ds.lengths[pick], kind="stable")]        # the batch order collate_fn gives these samples
    ref = collate_fn([samples[i] for i in pick])
    assert [f"seg{i}" for i in pick] == ref[9] and int(pick.max()) == n - 1 and not np.array_equal(pick, np.arange(len(pick)))
    return ds, pick, ref


def _sentinel_out(ds, B, T):
    return (torch.full((T, B), -7, dtype=torch.int64, device=DEV), torch.full((T, B, ds.dv), float("nan"), device=DEV),
            torch.full((T, B, ds.da), float("nan"), device=DEV), torch.full((B, 6), float("nan"), device=DEV),
            torch.full((B,), float("nan"), device=DEV))


def _masked_gather(ds, pick, T, **kw):
    from mmda_amd import ops
    out = _sentinel_out(ds, len(pick), T)
    kept = torch.full((len(pick),), 255, dtype=torch.uint8, device=DEV)
    o = torch.from_numpy(pick.astype(np.int32)).to(DEV)
    got = ops.collate_gather_masked(ds.words, ds.visual, ds.acoustic, ds.offsets, ds.emo, ds.sentiment, o, T, out=out, out_keep=kept, **kw)
    assert all(g is x for g, x in zip(got, out + (kept,)))
    return got


def _check_gather(got, ref, keep, what):
    """every output element was a sentinel no batch holds: equality proves the launch wrote them all, padding and blanks included"""
    ids, v, a = mc.mask_ref(ref[0].numpy(), ref[1].numpy(), ref[2].numpy(), ref[5].numpy(), keep)
    _same(got[0], ids, (what, "ids")); _same(got[1], v, (what, "visual")); _same(got[2], a, (what, "acoustic"))
    _same(got[3], ref[4], (what, "emo")); _same(got[4], ref[3], (what, "labels"))
    _same(got[5], np.broadcast_to(np.asarray(keep, dtype=np.uint8), (ids.shape[1],)).copy(), (what, "keep"))


@pytest.mark.parametrize("widths", mc.WIDTHS)
@pytest.mark.parametrize("shape", list(mc.LENGTH_LISTS))
def test_masked_gather_equals_collate_fn_and_the_mask(shape, widths):
    from mmda_amd import modality, ops
    ds, pick, ref = _case(shape, widths)
    T = int(ref[0].shape[0])
    for k in range(8):
        _check_gather(_masked_gather(ds, pick, T, keep=k), ref, k, ("const", k))
    for seed in SEEDS:
        bits = modality.keep_bits(seed, P_HALF, pick)
        _check_gather(_masked_gather(ds, pick, T, p=P_HALF, seed=seed), ref, bits, ("random", seed))
        _check_gather(_masked_gather(ds, pick, T, p=P_HALF, seed=seed, keep=5), ref, bits & 5, ("random & 5", seed))
    # keep = 7, p = 0: the bytes of mmda_collate_gather
    plain = ops.collate_gather(ds.words, ds.visual, ds.acoustic, ds.offsets, ds.emo, ds.sentiment,
                               torch.from_numpy(pick.astype(np.int32)).to(DEV), T, out=_sentinel_out(ds, len(pick), T))
    got = _masked_gather(ds, pick, T, keep=7, p=(0.0, 0.0, 0.0))
    for g, r in zip(got[:5], plain):
        assert g.dtype == r.dtype and torch.equal(g.view(torch.int32), r.view(torch.int32))
    assert bool((got[5] == 7).all())


@pytest.mark.parametrize("B", [40, 44, 64, 256])
def test_masked_gather_on_either_side_of_the_launch_forms(B):
    """T = 50 at MOSEI widths.  B = 40 is the last batch the scalar-column form takes (10 x 50 = 500 workgroups of at most 512), B = 44
    the first of the other form (550); B = 64 has more elements than the launch has threads; at B = 256 the launch is capped at 2048
    workgroups and every wave takes a second trip through its t loop."""
    from mmda_amd import DeviceDataset, modality
    from mmda_amd.data import collate_fn
    lengths = np.random.default_rng(B).integers(1, 51, size=B)
    lengths[B // 3] = 50
    samples = mc.make_samples(lengths.tolist(), 35, 74, seed=B)
    ds = DeviceDataset.from_samples(samples, DEV)
    pick = np.argsort(-ds.lengths, kind="stable")
    ref = collate_fn([samples[i] for i in pick])
    assert ref[0].shape == (50, B)
    bits = modality.keep_bits(B, (0.3, 0.4, 0.5), pick)
    assert len(set(bits.tolist())) >= 6
    _check_gather(_masked_gather(ds, pick, 50, p=(0.3, 0.4, 0.5), seed=B), ref, bits, ("random", B))
    _check_gather(_masked_gather(ds, pick, 50, keep=7), ref, 7, ("keep 7", B))


def test_masked_gather_random_sets_vary_and_use_the_sample_index():
    """64 samples at p = 1/2: every keep set but 0 occurs, and a sample's set does not depend on where in the batch it sits."""
    from mmda_amd import DeviceDataset, modality
    lengths = np.random.default_rng(1).integers(1, 8, size=64).tolist()
    ds = DeviceDataset.from_samples(mc.make_samples(lengths, 5, 3), DEV)
    bits = modality.keep_bits(9, P_HALF, np.arange(64))
    assert set(bits.tolist()) == set(range(1, 8))
    a = _masked_gather(ds, np.arange(64), 8, p=P_HALF, seed=9)[5].cpu().numpy()
    perm = np.random.default_rng(2).permutation(64)
    b = _masked_gather(ds, perm, 8, p=P_HALF, seed=9)[5].cpu().numpy()
    assert np.array_equal(a, bits) and np.array_equal(b, bits[perm])


def test_masked_gather_refuses_bad_arguments_without_a_launch():
    from mmda_amd import DeviceDataset, _lib
    lib = _lib.load()
    ds = DeviceDataset.from_samples(mc.make_samples([3, 2], 5, 3), DEV)
    B, T = 2, 3
    order = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    outs = list(_sentinel_out(ds, B, T)) + [torch.full((B,), 255, dtype=torch.uint8, device=DEV)]
    before = [x.clone() for x in outs]
    P = lambda *p: _lib.ModalityP((_lib.C.c_float * 3)(*p))
    good = [_lib.ptr(x) for x in (ds.words, ds.visual, ds.acoustic, ds.offsets, ds.emo, ds.sentiment, order)] + \
           [B, T, 5, 3, 1, 7, P(0.1, 0.2, 0.3), 5, 0] + [x.data_ptr() for x in outs] + [_lib.stream_ptr()]
    EINVAL = -1
    for k in (0, 1, 2, 3, 5, 6, 16, 17, 18, 20):                     # every pointer but emo / out_emo / out_keep
        bad = list(good); bad[k] = None
        assert lib.mmda_collate_gather_masked(*bad) == EINVAL, k
    for k in (7, 8, 9, 10):                                          # B, T, dv, da
        for val in (0, -1):
            bad = list(good); bad[k] = val
            assert lib.mmda_collate_gather_masked(*bad) == EINVAL, (k, val)
    for val in (-1, 8):                                              # keep_const
        bad = list(good); bad[12] = val
        assert lib.mmda_collate_gather_masked(*bad) == EINVAL, val
    for p in ((1.0, 0, 0), (0, -0.5, 0), (0, 0, float("nan")), (0, 0, 1.5)):
        bad = list(good); bad[13] = P(*p)
        assert lib.mmda_collate_gather_masked(*bad) == EINVAL, p
    bad = list(good); bad[4] = None                                  # out_emo asked of a dataset without emo
    assert lib.mmda_collate_gather_masked(*bad) == EINVAL
    torch.cuda.synchronize()
    for x, y in zip(outs, before):                                   # nothing ran
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    ok = list(good); ok[21] = None                                   # no out_keep: fewer outputs
    assert lib.mmda_collate_gather_masked(*ok) == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(outs[4]).any()) and bool((outs[5] == 255).all())


# ------------------------------------------------------------------------------------------------ 2: the out-of-place mask
@pytest.mark.parametrize("widths", mc.WIDTHS)
@pytest.mark.parametrize("shape", list(mc.LENGTH_LISTS))
def test_modality_mask_equals_the_host_mask_and_leaves_its_inputs(shape, widths):
    from mmda_amd import modality, ops
    from mmda_amd.data import collate_fn
    ref = collate_fn(mc.make_samples(mc.LENGTH_LISTS[shape], *widths, seed=3))
    t, v, a = (x.to(DEV) for x in ref[:3])
    clones = [x.clone() for x in (t, v, a)]
    T, B = t.shape
    keeps = list(range(8)) + [modality.keep_bits(s, P_HALF, np.arange(B)) for s in SEEDS]
    for k in keeps:
        out = (torch.full_like(t, -7), torch.full_like(v, float("nan")), torch.full_like(a, float("nan")))
        arg = torch.from_numpy(k).to(DEV) if isinstance(k, np.ndarray) else k
        got = ops.modality_mask(t, v, a, arg, out=out)
        assert all(g is o for g, o in zip(got, out))
        want = mc.mask_ref(ref[0].numpy(), ref[1].numpy(), ref[2].numpy(), ref[5].numpy(), k)
        for g, w, name in zip(got, want, ("ids", "visual", "acoustic")):
            _same(g, w, (name, k if not isinstance(k, np.ndarray) else k.tolist()))
        assert bool((got[0][t == mc.PAD] == mc.PAD).all())           # padding keeps PAD whatever is dropped
    for x, c in zip((t, v, a), clones):
        assert torch.equal(x, c)                                     # the inputs were only read
    fresh = ops.modality_mask(t, v, a, ("visual",))                  # names, fresh outputs
    _same(fresh[1], ref[1], "visual kept"); assert bool((fresh[2] == 0).all()) and fresh[0].data_ptr() != t.data_ptr()


def test_modality_mask_refuses_bad_arguments_without_a_launch():
    from mmda_amd import _lib
    lib = _lib.load()
    T, B, dv, da = 3, 2, 5, 3
    t = torch.full((T, B), 4, dtype=torch.int64, device=DEV); v = torch.ones(T, B, dv, device=DEV); a = torch.ones(T, B, da, device=DEV)
    outs = [torch.full_like(t, -7), torch.full_like(v, float("nan")), torch.full_like(a, float("nan"))]
    keep = torch.full((B,), 7, dtype=torch.uint8, device=DEV)
    good = [t.data_ptr(), v.data_ptr(), a.data_ptr(), T, B, dv, da, keep.data_ptr(), 7, 1, 0] + [x.data_ptr() for x in outs] + \
           [_lib.stream_ptr()]
    for k in (0, 1, 2, 11, 12, 13):
        bad = list(good); bad[k] = None
        assert lib.mmda_modality_mask(*bad) == -1, k
    for k in (3, 4, 5, 6):
        for val in (0, -1):
            bad = list(good); bad[k] = val
            assert lib.mmda_modality_mask(*bad) == -1, (k, val)
    for val in (-1, 8):
        bad = list(good); bad[8] = val
        assert lib.mmda_modality_mask(*bad) == -1, val
    for i in range(3):                                               # an output that is its input
        bad = list(good); bad[11 + i] = good[i]
        assert lib.mmda_modality_mask(*bad) == -1, i
    torch.cuda.synchronize()
    assert bool((outs[0] == -7).all()) and bool(torch.isnan(outs[1]).all()) and bool(torch.isnan(outs[2]).all())
    ok = list(good); ok[7] = None; ok[8] = 2
    assert lib.mmda_modality_mask(*ok) == 0
    torch.cuda.synchronize()
    assert bool((outs[0] == 0).all()) and bool((outs[1] == 1).all()) and bool((outs[2] == 0).all())


# ------------------------------------------------------------------------------------------------ 3: the loader
N = 37


@pytest.fixture(scope="module")
def corpus():
    from mmda_amd import DeviceDataset
    lengths = np.random.default_rng(5).integers(1, 10, size=N)
    samples = mc.make_samples(lengths, 35, 74, seed=1)
    return samples, DeviceDataset.from_samples(samples, DEV)


def _same_batch(got, ref, what):
    assert len(got) == len(ref) == 10
    for i in range(5):
        assert got[i].is_cuda
        _same(got[i], ref[i], (what, i))
    assert not got[5].is_cuda
    _same(got[5], ref[5], (what, "lengths"))
    for i in (6, 7, 8):
        _same(got[i], ref[i], (what, "bert", i))
    assert got[9] == ref[9], what


def _host_masked(samples, batch, seed, p, keep_const=7):
    """a collated host batch under the keep sets of its samples (their dataset indices are in the segment names)"""
    from mmda_amd import modality
    idx = np.array([int(s[3:]) for s in batch[9]])
    bits = (modality.keep_bits(seed, p, idx) if p is not None else np.full(len(idx), 7, np.uint8)) & np.uint8(keep_const)
    ids, v, a = mc.mask_ref(batch[0].numpy(), batch[1].numpy(), batch[2].numpy(), batch[5].numpy(), bits)
    return (torch.from_numpy(ids), torch.from_numpy(v), torch.from_numpy(a)) + tuple(batch[3:]), bits


def test_loader_epochs_follow_seed_plus_epoch(corpus):
    from mmda_amd import DeviceLoader
    from mmda_amd.data import collate_fn
    samples, ds = corpus
    host = list(DataLoader(samples, batch_size=8, collate_fn=collate_fn))
    seed = 2 ** 64 - 1                                               # epoch 1 runs under (seed + 1) mod 2^64 = 0
    ld = DeviceLoader(ds, 8, modality_dropout=P_HALF, modality_seed=seed, keep=("text", "visual"))
    epochs = []
    for e in range(2):
        assert ld.epoch == e
        got = []
        for k, batch in enumerate(ld):
            want, bits = _host_masked(samples, host[k], (seed + e) % 2 ** 64, P_HALF, 3)
            _same_batch(batch, want, (e, k))
            _same(ld.last_keep, bits, (e, k, "last_keep"))
            got.append(batch)
        assert len(got) == len(host) == 5
        epochs.append(got)
    assert any(not torch.equal(x[0], y[0]) or not torch.equal(x[1], y[1]) for x, y in zip(*epochs))      # the two epochs differ
    ld.set_epoch(0)
    for x, y in zip(ld, epochs[0]):
        for i in range(5):
            assert torch.equal(x[i], y[i])
    assert ld.epoch == 1


def test_loader_defaults_are_the_plain_loader(corpus):
    from mmda_amd import DeviceLoader
    from mmda_amd.data import collate_fn
    samples, ds = corpus
    ld = DeviceLoader(ds, 8, sampler=RandomSampler(samples, generator=_gen(3)))
    ref = list(DataLoader(samples, batch_size=8, sampler=RandomSampler(samples, generator=_gen(3)), collate_fn=collate_fn))
    got = list(ld)
    assert len(got) == len(ref) == 5 and not ld.masked and ld.last_keep is None and ld.epoch == 1
    for k, (g, r) in enumerate(zip(got, ref)):
        _same_batch(g, r, k)
    full = list(DeviceLoader(ds, 8, sampler=RandomSampler(samples, generator=_gen(3)), keep=7))          # the masked launch, nothing dropped
    for k, (g, r) in enumerate(zip(full, ref)):
        _same_batch(g, r, ("keep 7", k))


def _solver(train, dev, precision="fp32"):
    from mmda_amd import make_config, models
    from mmda_amd.solver import Solver
    cfg = orc.default_config(vocab_size=120, learning_rate=1e-3, clip=1.0)
    c = make_config(precision=precision, device=DEV, n_epoch=1, name="modality", **vars(cfg))
    m = models.MISA(c)
    m.load_state_dict(orc.synth_params(cfg, 21))
    torch.manual_seed(0)                                             # build() draws the orthogonal recurrent weights
    return Solver(c, c, c, train, dev, ListLoader([]), is_train=True, model=m).build()


def _state(m):
    P, _, M, V = m.flat_buckets()
    torch.cuda.synchronize()
    return [x.detach().cpu().clone() for x in (P, M, V)]


def test_solver_trains_to_the_same_bits_from_masked_batches_of_either_source():
    """One epoch of modality dropout from the loader against the same epoch fed from a list of host-masked batches.  The step is
    untouched and deterministic (tests/test_gpu_solver.py), so equal batches give equal bits: equality is the bound."""
    from mmda_amd import DeviceDataset, DeviceLoader
    from mmda_amd.data import collate_fn
    lengths = np.random.default_rng(8).integers(1, 10, size=20)
    samples = mc.make_samples(lengths, 35, 74, seed=2)
    ds = DeviceDataset.from_samples(samples, DEV)
    p, seed = (0.3, 0.4, 0.5), 11
    plain = list(DataLoader(samples, batch_size=8, sampler=RandomSampler(samples, generator=_gen(7)), collate_fn=collate_fn))
    assert all(bool((b[4].sum(0) > 0).all()) for b in plain)         # every class occurs in every batch: the losses stay finite
    host = [_host_masked(samples, b, seed, p) for b in plain]
    assert len({int(x) for _, bits in host for x in bits}) >= 4      # ... and the epoch does drop modalities
    a = _solver(DeviceLoader(ds, 8, sampler=RandomSampler(samples, generator=_gen(7)), modality_dropout=p, modality_seed=seed),
                ListLoader([]))
    b = _solver(ListLoader([h for h, _ in host]), ListLoader([]))
    a.model._materialize(torch.device(DEV)); b.model._materialize(torch.device(DEV))
    start = _state(a.model)[0]
    la, lb = a.train_epoch(), b.train_epoch()
    assert a.model._step == b.model._step == 3 and not a.model.cluster_aborted()
    assert la == lb and all(v == v for v in la.values())
    for name, x, y in zip("PMV", _state(a.model), _state(b.model)):
        assert torch.equal(x, y), (name, int((x != y).sum()))
    assert not torch.equal(start, _state(a.model)[0])


# ------------------------------------------------------------------------------------------------ 4: the Shapley collector
def _attrib(V):
    from mmda_amd import ops
    out = ops.modality_attrib(torch.from_numpy(V).to(DEV))
    torch.cuda.synchronize()
    return out


def _check_attrib(V, what):
    phi, loo, dom, counts = _attrib(V)
    n, C = V.shape[1:]
    assert tuple(phi.shape) == tuple(loo.shape) == (n, 3, C) and phi.dtype == loo.dtype == torch.float32
    assert tuple(dom.shape) == (n, C) and dom.dtype == torch.int32 and tuple(counts.shape) == (3, C) and counts.dtype == torch.int64
    bound = mc.attrib_bound(V)
    p64, l64 = phi.cpu().numpy().astype(np.float64).transpose(1, 0, 2), loo.cpu().numpy().astype(np.float64).transpose(1, 0, 2)
    r_phi, r_loo = mc.shapley_ref(V), mc.loo_ref(V)
    assert np.array_equal(np.isnan(p64), np.isnan(r_phi)) and np.array_equal(np.isnan(l64), np.isnan(r_loo)), what
    e_phi, e_loo = np.nanmax(np.abs(p64 - r_phi)), np.nanmax(np.abs(l64 - r_loo))
    e_eff = np.nanmax(np.abs(p64.sum(0) - (V[7].astype(np.float64) - V[0])))
    print(f"{what}: phi {e_phi:.3e} loo {e_loo:.3e} efficiency {e_eff:.3e} bound {bound:.3e}")
    assert e_phi <= bound and e_loo <= bound and e_eff <= 3 * bound, (what, e_phi, e_loo, e_eff, bound)
    d_ref, c_ref = mc.dominant_ref(phi.cpu().numpy())
    assert np.array_equal(dom.cpu().numpy(), d_ref) and np.array_equal(counts.cpu().numpy(), c_ref), what
    return phi, loo, dom, counts


@pytest.mark.parametrize("C", mc.ATTRIB_C)
def test_attrib_against_float64(C):
    for n in mc.ATTRIB_N:
        _check_attrib(mc.attrib_values(n, C, 100 * C + n), (n, C))
    _check_attrib(mc.attrib_values(257, C, 7, -3.0, 3.0), ("[-3, 3]", C))


def test_attrib_with_more_classes_than_the_workgroup_counts_in_lds():
    _check_attrib(mc.attrib_values(5, 300, 4), (5, 300))


def test_attrib_null_player_ties_nan_and_determinism():
    V = mc.attrib_values(65, 6, 5)
    for S in range(8):
        V[S] = V[S & ~2]                                             # visual changes no subset's value
    V[:, 3, :] = V[0, 3, :]                                          # row 3: nothing matters, a three-way tie at 0 -> modality 0
    V[:, 4, :] = 0.0
    for S in range(8):
        V[S, 4, :] = 0.25 * bin(S).count("1")                        # row 4: the three are interchangeable -> tie -> modality 0
    V[5, 7, 2] = np.nan                                              # row 7, class 2: a NaN reaches every phi -> -1, counted nowhere
    phi, loo, dom, counts = _check_attrib(V, "constructed")
    null = [i for i in range(65) if i != 4]                          # the rows where visual is a null player: exactly 0.0, not small
    for x in (phi[null, 1, :], loo[null, 1, :]):
        assert bool((x[~torch.isnan(x)] == 0.0).all()) and int(torch.isnan(x).sum()) == 1
    assert bool((phi[4] == phi[4, 0, 0]).all()) and float(phi[4, 0, 0]) > 0.2
    assert bool((phi[3] == 0.0).all()) and dom[3].tolist() == [0] * 6 and dom[4].tolist() == [0] * 6
    assert bool(torch.isnan(phi[7, :, 2]).all()) and int(dom[7, 2]) == -1 and int(counts[:, 2].sum()) == 64
    assert int(counts.sum()) == 65 * 6 - 1
    again = _attrib(V)
    for x, y in zip((phi, loo, dom, counts), again):
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)


def test_attrib_refuses_bad_arguments_without_a_launch():
    from mmda_amd import _lib
    lib = _lib.load()
    V = torch.zeros(8, 4, 6, device=DEV)
    phi = torch.full((4, 3, 6), float("nan"), device=DEV); loo = phi.clone()
    dom = torch.full((4, 6), -7, dtype=torch.int32, device=DEV); counts = torch.full((3, 6), -7, dtype=torch.int64, device=DEV)
    good = [V.data_ptr(), 4, 6, phi.data_ptr(), loo.data_ptr(), dom.data_ptr(), counts.data_ptr(), _lib.stream_ptr()]
    for k in (0, 3, 4, 5, 6):
        bad = list(good); bad[k] = None
        assert lib.mmda_modality_attrib(*bad) == -1, k
    for k in (1, 2):
        for val in (0, -1):
            bad = list(good); bad[k] = val
            assert lib.mmda_modality_attrib(*bad) == -1, (k, val)
    torch.cuda.synchronize()
    assert bool(torch.isnan(phi).all()) and bool((dom == -7).all()) and bool((counts == -7).all())


# ------------------------------------------------------------------------------------------------ 5: the pass
PASS_LENGTHS = [3, 7, 1, 5, 2, 6, 4, 1, 7, 2, 5]


@pytest.fixture(scope="module")
def small():
    from mmda_amd import DeviceDataset
    samples = mc.make_samples(PASS_LENGTHS, 35, 74, seed=4)
    return samples, DeviceDataset.from_samples(samples, DEV)


def _model(precision):
    from mmda_amd import MISA, make_config
    cfg = orc.default_config(vocab_size=120)
    m = MISA(make_config(precision=precision, device=DEV, **vars(cfg)))
    m.load_state_dict(orc.synth_params(cfg, 21))
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def models_by_precision():
    return {p: _model(p) for p in ("fp32", "bf16")}


@pytest.mark.parametrize("batch_size", [4, 11])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_pass_slices_equal_inference_passes_with_that_keep_set(small, models_by_precision, precision, batch_size):
    from mmda_amd import InferencePass, ModalityPass
    from mmda_amd.utils.eval import get_metrics
    samples, ds = small
    m = models_by_precision[precision]
    res = ModalityPass(m).run(ds, batch_size)
    n = len(samples)
    assert tuple(res.scores.shape) == (8, n, 6) and tuple(res.tcp.shape) == (8, n, 6) and res.scores.is_cuda and len(res) == n
    assert not bool(torch.isnan(res.scores).any()) and not bool(torch.isnan(res.tcp).any())
    ip = InferencePass(m, ("scores", "tcp"))
    for k in range(8):
        one = ip.run(ds, batch_size, keep=k)
        assert torch.equal(res.scores[k], one.scores) and torch.equal(res.tcp[k], one.tcp), k
    plain = ip.run(ds, batch_size)
    assert torch.equal(res.scores[7], plain.scores) and torch.equal(res.tcp[7], plain.tcp)
    assert not torch.equal(res.scores[0], res.scores[7])             # blanking everything does change the scores
    assert torch.equal(res.truth, ds.emo) and list(res.segments) == [s[2] for s in samples]
    # the figures per keep set, against get_metrics on read-back copies
    truth = ds.emo.cpu().numpy()
    thr = float(m.config.threshold)
    for k, got in enumerate(res.metrics()):
        want = get_metrics(truth, (res.scores[k].cpu().numpy() > np.float32(thr)).astype(np.float32))
        assert got["keep"] == k and {x: got[x] for x in want} == want, k
    at = res.attribution("scores")
    assert tuple(at["phi"].shape) == (n, 3, 6) and int(at["counts"].sum()) == n * 6
    eff = (at["phi"].sum(1) - (res.scores[7] - res.scores[0])).abs().max()
    assert float(eff) <= 3 * mc.attrib_bound(res.scores.cpu().numpy())
    host = res.cpu()
    assert not host.scores.is_cuda and torch.equal(host.scores, res.scores.cpu())
    d = res.as_dict()
    assert d["scores"].shape == (8, n, 6) and d["phi_tcp"].shape == (n, 3, 6) and d["counts_scores"].shape == (3, 6)


def test_pass_over_a_loader_gives_the_same_tables(small, models_by_precision):
    """the slow road: any loader of the reference's tuples, walked eight times; rows in the loader's order"""
    from mmda_amd import DeviceLoader, InferencePass, ModalityPass
    from mmda_amd.data import collate_fn
    samples, ds = small
    m = models_by_precision["fp32"]
    res = ModalityPass(m).run(ds, 4, order="dataset")
    host = ListLoader(list(DataLoader(samples, batch_size=4, collate_fn=collate_fn)))
    slow = ModalityPass(m).run_loader(host)
    rows = torch.tensor([int(s[3:]) for s in slow.segments], device=DEV)
    assert torch.equal(slow.scores, res.scores[:, rows]) and torch.equal(slow.tcp, res.tcp[:, rows])
    assert torch.equal(slow.truth, ds.emo[rows])
    one = InferencePass(m, ("scores",)).run_loader(DeviceLoader(ds, 4), keep=("acoustic",))
    assert torch.equal(one.scores, slow.scores[4])
    for b, c in zip(host, DataLoader(samples, batch_size=4, collate_fn=collate_fn)):
        assert all(torch.equal(x, y) for x, y in zip(b[:3], c[:3]))  # the list's batches were not written


@pytest.mark.parametrize("keep", [0, 5, ("visual",)])
def test_solver_eval_under_a_keep_set_equals_host_masked_batches(small, keep, capsys):
    from mmda_amd import DeviceLoader, parse_keep
    from mmda_amd.data import collate_fn
    samples, ds = small
    s = _solver(ListLoader([]), DeviceLoader(ds, 4))
    loss_a, acc_a, pred_a, true_a = s.eval("dev", keep=keep)
    if parse_keep(keep) == 5:                                        # the pass and the inference pass through the solver
        res = s.modalities("dev", to_print=True)
        assert res is s.last_modalities and tuple(res.scores.shape) == (8, 11, 6)
        table = capsys.readouterr().out
        assert "text+acoustic" in table and "mean phi" in table and len(table.strip().splitlines()) == 9 + 1 + 6
        inf = s.infer("dev", fields=("scores",), order="length", keep=keep)
        assert torch.equal(inf.scores, res.scores[5])
        assert acc_a == res.metrics()[5]["acc"]
    host = [_host_masked(samples, b, 0, None, parse_keep(keep))[0] for b in DataLoader(samples, batch_size=4, collate_fn=collate_fn)]
    s.dev_data_loader = ListLoader(host)
    loss_b, acc_b, pred_b, true_b = s.eval("dev")
    assert loss_a == loss_b and acc_a == acc_b and loss_a == loss_a and not s.model.cluster_aborted()
    assert pred_a.shape == (11, 6) and np.array_equal(pred_a, pred_b) and np.array_equal(true_a, true_b)


def test_the_encoder_cache_refuses_a_keep_set(small, models_by_precision):
    from mmda_amd import EncodedLoader, InferencePass, step_rules
    from mmda_amd._lib import MMDAError
    m = models_by_precision["fp32"]
    text = dict(step_rules.MODALITY_RULES)["modality_encoded"].format(keep=3)
    with pytest.raises(MMDAError) as e:
        m.forward_encoded(None, keep=("text", "visual"))
    assert str(e.value) == text

    class Cache:
        lengths = torch.ones(4, dtype=torch.int64)

        def __len__(self):
            return 4

    loader = EncodedLoader(Cache(), 2)
    with pytest.raises(MMDAError) as e:
        InferencePass(m, ("scores",)).run_loader(loader, keep=3)
    assert str(e.value) == text
    s = _solver(ListLoader([]), loader)
    for call in (lambda: s.eval("dev", keep=3), lambda: s.infer("dev", keep=3)):
        with pytest.raises(MMDAError) as e:
            call()
        assert str(e.value) == text
    with pytest.raises(MMDAError, match="encoder cache"):
        s.modalities("dev")
