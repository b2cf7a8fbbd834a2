"""CPU: the encoder cache's host side -- the refusals of the five native entry points (all before any launch, so no device is needed),
the ctypes mirror of ``mmda_encoded_batch``, ``EncodedLoader`` against ``batch_plan``, the fingerprint and the staleness check on host
tensors, a save / load round trip, and the Python refusals that need no device."""
import ctypes as C
import os
import subprocess
import textwrap

import numpy as np
import pytest
import torch

from mmda_amd import _lib, make_config, MISA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
FAKE = 256                      # 16-byte aligned, never dereferenced: every call below is refused before a launch
CUT = ("trnn1", "trnn2", "vrnn1", "vrnn2", "arnn1", "arnn2", "tlayer_norm", "vlayer_norm", "alayer_norm", "embed")
WIDTHS = (1200, 140, 296)


def _model(**kw):
    kw.setdefault("vocab_size", 50)
    return MISA(make_config(**kw))


# ------------------------------------------------------------------------------------------------ the two row movers
def test_collect_refuses_bad_arguments_without_a_launch():
    lib = _lib.load()
    call = lambda src=(FAKE,) * 3, w=(8, 8, 8), tab=(FAKE,) * 3, B=4: lib.mmda_encoded_collect(*src, *w, *tab, None, 0, B, None)
    assert call(tab=(None, None, None), src=(None, None, None)) == EINVAL          # every segment NULL
    assert call(tab=(None, None, None)) == EINVAL
    for k in range(3):
        one = lambda v: tuple(v if i == k else FAKE for i in range(3))
        assert call(tab=one(None)) == EINVAL                       # a source without its table
        assert call(src=one(None)) == EINVAL                       # a table without its source
        for w in (0, -4):
            assert call(w=tuple(w if i == k else 8 for i in range(3))) == EINVAL
    for B in (0, -1):
        assert call(B=B) == EINVAL


def test_gather_refuses_bad_arguments_without_a_launch():
    lib = _lib.load()

    def call(tab=(FAKE,) * 3, w=(8, 8, 8), tab_emo=FAKE, ncls=6, rows=FAKE, B=4, out=(FAKE,) * 3, emo=FAKE):
        return lib.mmda_encoded_gather(*tab, *w, tab_emo, ncls, rows, B, *out, emo, None)

    assert call(tab=(None,) * 3, out=(None,) * 3, tab_emo=None, emo=None) == EINVAL     # every segment NULL
    assert call(rows=None) == EINVAL
    assert call(emo=None) == EINVAL and call(tab_emo=None) == EINVAL                     # labels without their table, or the reverse
    assert call(ncls=0) == EINVAL
    for k in range(3):
        one = lambda v: tuple(v if i == k else FAKE for i in range(3))
        assert call(tab=one(None)) == EINVAL and call(out=one(None)) == EINVAL
        assert call(w=tuple(0 if i == k else 8 for i in range(3))) == EINVAL
    for B in (0, -3):
        assert call(B=B) == EINVAL


# ------------------------------------------------------------------------------------------------ the model's entry points
def _batch(**kw):
    eb = _lib.EncodedBatch(tab_t=FAKE, tab_v=FAKE, tab_a=FAKE, tab_emo=FAKE, rows=FAKE, B=4)
    for k, v in kw.items():
        setattr(eb, k, v)
    return eb


def test_model_entry_points_refuse_without_a_launch():
    """No device, so no workspace: what can be reached here is that every way of asking -- with and without the cut, which is sent
    through mmda_misa_set_trainable, with a good and with a bad batch -- is MMDA_EINVAL and launches nothing.  That it is the cut which
    refuses a model with a workspace is tests/test_gpu_encoded.py's."""
    lib = _lib.load()
    step = lambda m, eb, emo=FAKE: lib.mmda_misa_train_step_encoded(m, None if eb is None else C.byref(eb), emo, 1, 7, 1, 1e-3, 1.0, 1, None)
    fwd = lambda m, eb: lib.mmda_misa_forward_encoded(m, None if eb is None else C.byref(eb), 0, 7, None)
    m = _model(precision="fp32")
    assert step(None, _batch()) == EINVAL and fwd(None, _batch()) == EINVAL
    assert lib.mmda_misa_encoded_collect(None, FAKE, FAKE, FAKE, None, 0, None) == EINVAL
    assert lib.mmda_misa_encoded_collect(m._h, FAKE, FAKE, FAKE, None, 0, None) == EINVAL        # no workspace: nothing to collect from
    for cut in (False, True):
        if cut:
            m.freeze(*CUT)
        m._sync_trainable()
        assert m.trainable_info()[2] == cut
        assert step(m._h, _batch()) == EINVAL and fwd(m._h, _batch()) == EINVAL
        assert step(m._h, None) == EINVAL and fwd(m._h, None) == EINVAL
        for bad in (dict(tab_t=None), dict(tab_v=None), dict(tab_a=None), dict(rows=None), dict(B=0), dict(B=-4)):
            assert step(m._h, _batch(**bad)) == EINVAL and fwd(m._h, _batch(**bad)) == EINVAL, bad
        assert step(m._h, _batch(tab_emo=None)) == EINVAL and step(m._h, _batch(), emo=None) == EINVAL
    # the backward pass's extern form still wants its batch
    assert lib.mmda_misa_backward(m._h, None, None, None, None, None) == EINVAL


def test_struct_mirror_has_the_compilers_layout(tmp_path):
    code = textwrap.dedent("""
        #include <stdio.h>
        #include <stddef.h>
        #include "mmda_hip.h"
        int main(){printf("%zu %zu %zu %zu\\n", sizeof(mmda_encoded_batch), offsetof(mmda_encoded_batch, tab_emo),
                          offsetof(mmda_encoded_batch, rows), offsetof(mmda_encoded_batch, B)); return 0;}""")
    (tmp_path / "s.c").write_text(code)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")], check=True)
    out = subprocess.run([str(tmp_path / "s")], check=True, capture_output=True, text=True).stdout.split()
    E = _lib.EncodedBatch
    assert [int(x) for x in out] == [C.sizeof(E), E.tab_emo.offset, E.rows.offset, E.B.offset]


# ------------------------------------------------------------------------------------------------ the loader
def _cache(n=21, model=None, seed=0, widths=WIDTHS):
    from mmda_amd import EncoderCache
    from mmda_amd.encoded import _fingerprint_tensor
    g = torch.Generator().manual_seed(seed)
    flat = torch.randn(sum((n * w + 3) // 4 * 4 for w in widths), generator=g)
    L = torch.from_numpy(np.random.default_rng(seed).integers(1, 13, size=n))
    seg = np.array([f"seg{i}" for i in range(n)], dtype=object)
    fp = 0 if model is None else int(_fingerprint_tensor(model))
    return EncoderCache(flat, widths, n, (torch.rand(n, 6, generator=g) > 0.5).float(), L, seg, fp, model)


def test_cache_views_tile_the_flat_buffer():
    c = _cache(n=7, widths=(20, 12, 7))
    assert c.utt_t.shape == (7, 20) and c.utt_v.shape == (7, 12) and c.utt_a.shape == (7, 7) and len(c) == 7
    base = c.flat.data_ptr()
    assert [(x.data_ptr() - base) // 4 for x in (c.utt_t, c.utt_v, c.utt_a)] == [0, 140, 140 + 84]     # each starts on a 16-byte boundary
    assert c.flat.numel() == 140 + 84 + 52


@pytest.mark.parametrize("drop_last", [False, True])
@pytest.mark.parametrize("batch_size", [1, 8, 21, 32])
def test_loader_batches_are_batch_plans(batch_size, drop_last):
    from mmda_amd import EncodedLoader, batch_plan
    m = _model()
    c = _cache(model=m)
    for kw in (dict(), dict(shuffle=True, generator=torch.Generator().manual_seed(3)), dict(sampler=[5, 3, 3, 20, 0, 7, 11, 2, 9, 1])):
        ld = EncodedLoader(c, batch_size, drop_last=drop_last, **kw)
        if "sampler" in kw:
            seq = np.array(kw["sampler"])
        elif kw:
            seq = torch.randperm(21, generator=torch.Generator().manual_seed(3)).numpy()
        else:
            seq = np.arange(21)
        order, bounds = batch_plan(c.lengths.numpy(), seq, batch_size, drop_last)
        got = list(ld)
        assert len(got) == len(ld) == len(bounds) - 1
        for eb, lo, hi in zip(got, bounds[:-1], bounds[1:]):
            assert eb.cache is c and eb.B == hi - lo and eb.rows.dtype == torch.int32 and eb.rows_ptr == eb.rows.data_ptr()
            assert eb.rows.tolist() == order[lo:hi].tolist()
            assert eb.lengths.tolist() == c.lengths[order[lo:hi]].tolist() and bool((np.diff(eb.lengths.numpy()) <= 0).all())
            assert eb.segments == [f"seg{i}" for i in order[lo:hi]]
            assert torch.equal(eb.emo(), c.emo[order[lo:hi]])
    assert list(EncodedLoader(_cache(n=3, model=m), 8, drop_last=True)) == []


def test_loader_refuses_bad_arguments():
    from mmda_amd import EncodedLoader
    c = _cache()
    with pytest.raises(ValueError, match="mutually exclusive"):
        EncodedLoader(c, 8, shuffle=True, sampler=[0, 1])
    with pytest.raises(ValueError):
        EncodedLoader(c, 0)
    with pytest.raises(IndexError):
        list(EncodedLoader(c, 8, sampler=[0, 21]))
    with pytest.raises(_lib.MMDAError, match=r"cache\.check\(model\)"):
        list(EncodedLoader(c, 8))                                    # a cache that knows no model (loaded from a file)


# ------------------------------------------------------------------------------------------------ fingerprint, staleness, files
def test_fingerprint_covers_exactly_what_the_encoders_read():
    from mmda_amd import EncodedLoader
    from mmda_amd.encoded import ENCODER_PREFIXES, encoder_ranges, _fingerprint_tensor
    m = _model()
    # the ranges: every encoder tensor inside one, no other tensor touched
    ranges = encoder_ranges(m)
    inside = lambda off, n: any(b <= off and off + n <= e for b, e in ranges)
    for name in m._native_names:
        off, shape = m._layout[name]
        assert inside(off, int(np.prod(shape))) == (name.split(".")[0] in ENCODER_PREFIXES), name
    want = sum(int(m._get(n).detach().view(torch.int32).sum(dtype=torch.int64)) for n in m._native_names
               if n.split(".")[0] in ENCODER_PREFIXES)
    c = _cache(model=m)
    assert c.fingerprint == want == int(_fingerprint_tensor(m))
    c.check(m)
    with torch.no_grad():
        m.classifier.classifier_layer.weight[0, 0] += 1.0            # the heads are not the encoders'
        m.project_t.project_t.bias[3] -= 1.0
    c.check(m)
    assert len(list(EncodedLoader(c, 8))) == 3
    for name in ("trnn1.weight_ih_l0", "arnn2.bias_hh_l0_reverse", "vlayer_norm.bias", "embed.weight"):
        p = m._get(name)
        with torch.no_grad():
            keep = p.detach().clone()
            p.view(-1)[1] += 0.25
        with pytest.raises(_lib.MMDAError, match="stale"):
            c.check(m)
        with pytest.raises(_lib.MMDAError, match="stale"):           # an epoch reads the verdict behind its last batch
            list(EncodedLoader(c, 8))
        with torch.no_grad():
            p.copy_(keep)
        c.check(m)


def test_save_and_load_round_trip(tmp_path):
    from mmda_amd import EncoderCache
    m = _model()
    c = _cache(model=m, seed=4)
    path = tmp_path / "cache.pt"
    c.save(path)
    raw = torch.load(path, weights_only=True)                       # plain tensors and scalars
    assert set(raw) == {"flat", "widths", "n", "emo", "lengths", "segments", "fingerprint"}
    d = EncoderCache.load(path, "cpu")
    assert d.n == c.n and d.widths == c.widths and d.fingerprint == c.fingerprint and d.model is None
    for k in "tva":
        assert torch.equal(getattr(d, f"utt_{k}"), getattr(c, f"utt_{k}"))
    assert torch.equal(d.emo, c.emo) and torch.equal(d.lengths, c.lengths) and list(d.segments) == list(c.segments)
    assert d.check(m) is d and d.model is m
    no_emo = _cache(model=m)
    no_emo.emo = None
    no_emo.save(path)
    assert EncoderCache.load(path, "cpu").emo is None


# ------------------------------------------------------------------------------------------------ the Python refusals
def test_steps_from_the_cache_are_refused_by_name_before_any_launch():
    from mmda_amd import EncodedLoader
    m = _model()
    c = _cache(model=m)
    (eb,) = list(EncodedLoader(c, 32))
    step = lambda mm=m, b=eb, **kw: mm.train_step_encoded(b, lr=1e-3, clip=1.0, **kw)
    with pytest.raises(TypeError, match="EncodedBatch"):
        step(b=(1, 2, 3))
    with pytest.raises(_lib.MMDAError, match="gradient exchange"):
        step(grad_sync=lambda g, n: 1.0)
    for kw in (dict(accum_count=2), dict(accum_index=1, accum_count=2)):
        with pytest.raises(_lib.MMDAError, match="not built"):
            step(**kw)
    with pytest.raises(_lib.MMDAError, match="not built"):
        step(mm=_model(accum_steps=2))
    with pytest.raises(_lib.MMDAError, match="wide"):
        step(mm=_model(visual_size=20))
    # the cut is not in force: the trainable encoder tensors are listed
    with pytest.raises(_lib.MMDAError, match="encoder cut") as e:
        step()
    assert "trnn1.weight_ih_l0" in str(e.value) and "embed.weight" in str(e.value) and "classifier" not in str(e.value)
    m.freeze(*CUT)
    m.unfreeze("vlayer_norm.bias")
    with pytest.raises(_lib.MMDAError, match=r"Still trainable: \['vlayer_norm.bias'\]"):
        step()
    with torch.no_grad():
        with pytest.raises(_lib.MMDAError, match="encoder cut"):
            m.forward_encoded(eb)
    sparse = _model(embed_update="sparse")
    sparse.freeze(*CUT[:-1])
    with pytest.raises(_lib.MMDAError, match="embed_update='sparse'"):
        step(mm=sparse)
    # under the cut: autograd, and a cache that is not on the GPU
    m.freeze(*CUT)
    with pytest.raises(_lib.MMDAError, match="autograd"):
        m.forward_encoded(eb)
    with pytest.raises(_lib.MMDAError, match="no CPU path"):
        step()
    assert m._step == 0 and m._seed == 0x5EED and m._ws is None          # nothing ran, no seed was drawn


def test_solver_refusals():
    from mmda_amd import EncodedLoader
    from mmda_amd.solver import Solver
    m = _model()
    cfg = m.config
    s = Solver(cfg, cfg, cfg, EncodedLoader(_cache(model=m), 8), [], [], is_train=True, model=m)
    with pytest.raises(_lib.MMDAError, match="EncodedLoader"):
        s.train_epoch_unfused()
    with pytest.raises(ValueError, match="DeviceLoader"):
        s.encode("dev")
    with pytest.raises(ValueError):
        s.encode("valid")
