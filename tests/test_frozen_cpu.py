"""CPU: frozen parameters (requires_grad = False) down to the C ABI -- what can be checked without a GPU: the table of trainable runs that
``mmda_misa_set_trainable`` builds and ``mmda_misa_trainable_info`` reads back, the encoder-cut decision, ``mmda_runs_build``, the error
codes of the run-table launches (none of which launches anything here), ``MISA.freeze`` / ``unfreeze`` and the refusals that need no
device.  A tensor's range runs up to the next tensor's offset: the alignment padding behind it (at most three floats, always zero) goes
with it."""
import ctypes as C

import pytest

from mmda_amd import _lib, make_config, MISA

EINVAL = -1
RNN = ("trnn1", "trnn2", "vrnn1", "vrnn2", "arnn1", "arnn2")
LNS = ("tlayer_norm", "vlayer_norm", "alayer_norm")
CUT = RNN + LNS + ("embed",)


def _model(**kw):
    kw.setdefault("vocab_size", 50)
    return MISA(make_config(**kw))


def _extents(m):
    """name -> (begin, end) in native order; the end is the next tensor's offset"""
    names = m._native_names
    offs = [m._layout[n][0] for n in names] + [m._flat_floats]
    assert offs == sorted(offs)
    return {n: (offs[i], offs[i + 1]) for i, n in enumerate(names)}


def _send(m):
    m._sync_trainable()
    return m.trainable_info()


def _check_cover(m, runs, floats):
    """sorted, disjoint, not touching (touching runs are merged), and exactly the trainable tensors' floats"""
    ext = _extents(m)
    want = set()
    for n, (b, e) in ext.items():
        if m._get(n).requires_grad:
            want.update(range(b, e))
    got = set()
    end = -1
    for b, l in runs:
        assert l > 0 and b > end                       # b == end would be two runs that touch
        got.update(range(b, b + l))
        end = b + l
    assert end <= m._flat_floats
    assert got == want and floats == len(want)


def test_nothing_frozen_is_one_run_and_no_cut():
    m = _model()
    runs, floats, cut = m.trainable_info()             # the state after create, nothing sent yet
    assert runs == [(0, m._flat_floats)] and floats == m._flat_floats and not cut
    assert _send(m) == (runs, floats, cut) and m._trainable_sends == 0


def test_one_float_tensor_frozen():
    m = _model(activation="prelu")
    b, e = _extents(m)["activation.weight"]
    assert m._layout["activation.weight"][1] == (1,) and e - b == 4       # one float and the padding in front of the recurrent layers
    assert m.freeze("activation") == ["activation.weight"]
    assert not m.project_t.project_t_activation.weight.requires_grad          # (the aliases are the same Parameter)
    runs, floats, cut = _send(m)
    assert runs == [(0, b), (e, m._flat_floats - e)] and not cut
    _check_cover(m, runs, floats)
    assert m._trainable_sends == 1


def test_two_adjacent_tensors_frozen():
    m = _model()
    ext = _extents(m)
    names = m._native_names
    i = names.index("shared.shared_1.weight")
    a, b = names[i], names[i + 1]
    assert ext[a][1] == ext[b][0]
    m.freeze(a, b)
    runs, floats, cut = _send(m)
    assert runs == [(0, ext[a][0]), (ext[b][1], m._flat_floats - ext[b][1])] and not cut
    _check_cover(m, runs, floats)


def test_first_and_last_tensor_frozen():
    m = _model()
    ext = _extents(m)
    first, last = m._native_names[0], m._native_names[-1]
    assert ext[first][0] == 0 and last == "embed.weight" and ext[last][1] == m._flat_floats
    m.freeze(first, last)
    runs, floats, cut = _send(m)
    assert runs == [(ext[first][1], ext[last][0] - ext[first][1])] and not cut
    _check_cover(m, runs, floats)


def test_everything_frozen():
    m = _model()
    for p in m.parameters():
        p.requires_grad_(False)
    runs, floats, cut = _send(m)
    assert runs == [] and floats == 0 and cut


def test_scattered_set_covers_exactly_the_trainable_floats():
    m = _model(activation="prelu", use_cmd_sim=False)
    for k, n in enumerate(m._native_names):
        if k % 3 == 1 or n.endswith("bias"):
            m._get(n).requires_grad_(False)
    runs, floats, cut = _send(m)
    assert len(runs) > 10 and not cut
    _check_cover(m, runs, floats)


def test_cut_is_on_exactly_for_the_cut_sets():
    m = _model()
    assert m.freeze(*CUT)
    runs, floats, cut = _send(m)
    ext = _extents(m)
    assert cut
    _check_cover(m, runs, floats)
    assert all(b + l <= ext["trnn2.weight_ih_l0"][0] for b, l in runs)     # every trainable float lies in front of rnn2_begin
    # one encoder bias, or one inter-layer LayerNorm tensor, trainable: off
    for one in ("arnn1.bias_hh_l0_reverse", "trnn2.bias_ih_l0", "vlayer_norm.bias", "tlayer_norm.weight", "embed.weight"):
        m.unfreeze(one)
        assert not _send(m)[2], one
        m.freeze(one)
        assert _send(m)[2], one
    # tensors in front of the cut do not matter
    m.freeze("project_t", "classifier")
    assert _send(m)[2]
    m.unfreeze("project_t", "classifier")
    # the table frozen by embed_update instead of by its flag
    f = _model(embed_update="frozen")
    assert not f.embed.weight.requires_grad and not _send(f)[2]
    f.freeze(*RNN, *LNS)
    runs, floats, cut = _send(f)
    assert cut
    _check_cover(f, runs, floats)
    # sparse: the table trains through the rows update, which needs the pass down to the embedding rows
    s = _model(embed_update="sparse")
    s.freeze(*RNN, *LNS)
    assert not _send(s)[2]


def test_set_is_sent_only_when_it_changes():
    m = _model()
    _send(m); _send(m)
    assert m._trainable_sends == 0
    m.freeze("trnn1")
    _send(m); _send(m)
    assert m._trainable_sends == 1
    m.unfreeze("trnn1")
    _send(m)
    assert m._trainable_sends == 2 and m.trainable_info()[0] == [(0, m._flat_floats)]


def test_freeze_and_unfreeze_names():
    m = _model()
    got = m.freeze("trnn1")
    assert got == ["trnn1." + k for k in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0", "weight_ih_l0_reverse",
                                          "weight_hh_l0_reverse", "bias_ih_l0_reverse", "bias_hh_l0_reverse")]
    assert m.frozen_names() == got and not any(dict(m.named_parameters())[k].requires_grad for k in got)
    assert m.freeze("embed", "embed.weight") == ["embed.weight"]
    assert m.unfreeze("trnn1.weight_hh") == ["trnn1.weight_hh_l0", "trnn1.weight_hh_l0_reverse"]
    assert m.trnn1.weight_hh_l0.requires_grad and not m.trnn1.weight_ih_l0.requires_grad
    assert len(m.freeze("trnn", "vrnn", "arnn")) == 48
    with pytest.raises(ValueError):
        m.freeze("nothing_like_this")
    with pytest.raises(ValueError):
        m.unfreeze("")
    f = _model(embed_update="frozen")
    assert f.frozen_names() == ["embed.weight"] and f.frozen_names(beyond_embed_update=True) == []
    with pytest.raises(_lib.MMDAError, match="set_embed_update"):
        f.unfreeze("embed")


def test_refusals_without_a_device():
    for mode in ("sparse", "deferred"):
        m = _model(embed_update=mode)
        m.embed.weight.requires_grad_(False)
        with pytest.raises(_lib.MMDAError, match=r'set_embed_update\("frozen"\)'):
            m._sync_trainable()
        m.embed.weight.requires_grad_(True)
        m._sync_trainable()
    m = _model()
    m.freeze("trnn1")
    with pytest.raises(_lib.MMDAError, match="not built yet"):
        m._sync_trainable(exchange=True)
    f = _model(embed_update="frozen")
    f._sync_trainable(exchange=True)                   # embed_update='frozen' with an exchange is what it was
    lib = _lib.load()
    flags = bytes(len(m._native_names))
    assert lib.mmda_misa_set_trainable(m._h, flags, len(flags) - 1) == EINVAL
    assert lib.mmda_misa_set_trainable(m._h, None, len(flags)) == EINVAL
    assert lib.mmda_misa_set_trainable(None, flags, len(flags)) == EINVAL


def _build(ranges, bucket):
    lib = _lib.load()
    k = len(ranges)
    b = (C.c_int64 * max(k, 1))(*[r[0] for r in ranges])
    l = (C.c_int64 * max(k, 1))(*[r[1] for r in ranges])
    out = (_lib.Run * max(k, 1))()
    n = C.c_int(-1)
    items = lib.mmda_runs_build(b, l, k, bucket, out, C.byref(n))
    return items, [(out[i].begin, out[i].len, out[i].first) for i in range(max(n.value, 0))]


def test_runs_build():
    # items: the aligned quads a run touches.  [1, 4): quad 0; [5, 10): quads 1, 2; [10, 11) touches [5, 10) and is merged; [12, 16): quad 3
    items, runs = _build([(1, 3), (5, 5), (10, 1), (11, 0), (12, 4)], 16)
    assert runs == [(1, 3, 0), (5, 6, 1), (12, 4, 3)] and items == 4
    assert _build([], 16) == (0, [])
    assert _build([(0, 16)], 16) == (4, [(0, 16, 0)])
    assert _build([(3, 2)], 16) == (2, [(3, 2, 0)])            # two floats, two quads
    for bad in ([(4, 4), (0, 4)], [(0, 5), (4, 4)], [(0, 17)], [(-1, 2)], [(0, -1)], [(16, 1)]):
        assert _build(bad, 16)[0] == EINVAL, bad


FAKE = C.c_void_p(256)          # 16-byte aligned, never dereferenced: every call below is refused (or empty) before a launch
ODD = C.c_void_p(260)


def test_run_table_launches_reject_bad_arguments_without_a_launch():
    lib = _lib.load()
    adam = lambda p=FAKE, g=FAKE, m=FAKE, v=FAKE, runs=FAKE, n=1, items=1, step=1: lib.mmda_clamp_adam_runs(
        p, g, m, v, runs, n, items, 1e-3, 0.9, 0.999, 1e-8, 1.0, 1.0, step, None)
    assert adam(p=None) == EINVAL and adam(g=None) == EINVAL and adam(m=None) == EINVAL and adam(v=None) == EINVAL
    assert adam(p=ODD) == EINVAL and adam(v=ODD) == EINVAL and adam(step=0) == EINVAL and adam(n=-1) == EINVAL and adam(items=-1) == EINVAL
    assert adam(runs=None) == EINVAL
    assert adam(n=0, runs=None) == 0 and adam(items=0) == 0                  # nothing trains in the range: nothing is launched
    asum = lambda acc=FAKE, runs=FAKE, n=1, items=1, step=1: lib.mmda_clamp_adam_sum_runs(
        FAKE, acc, FAKE, FAKE, FAKE, runs, n, items, 1e-3, 0.9, 0.999, 1e-8, 1.0, 1.0, step, None)
    assert asum(acc=ODD) == EINVAL and asum(step=0) == EINVAL and asum(runs=None) == EINVAL and asum(n=0) == 0
    assert asum(acc=None, n=0) == 0 and asum(acc=None, step=0) == EINVAL
    rms = lambda p=FAKE, sq=FAKE, runs=FAKE, n=1, items=1: lib.mmda_clamp_rmsprop_runs(p, FAKE, sq, runs, n, items, 1e-2, 0.99, 1e-8, 1.0, 1.0, None)
    assert rms(p=None) == EINVAL and rms(sq=None) == EINVAL and rms(runs=None) == EINVAL and rms(n=-1) == EINVAL
    assert rms(n=0) == 0 and rms(items=0) == 0


def test_run_struct_matches_c_layout():
    import os, subprocess, tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write('#include <stdio.h>\n#include "mmda_hip.h"\nint main(){printf("%zu\\n", sizeof(mmda_run));return 0;}\n')
        subprocess.run(["gcc", "-I", os.path.join(root, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")], check=True)
        out = subprocess.run([os.path.join(d, "s")], check=True, capture_output=True, text=True).stdout
    assert int(out) == C.sizeof(_lib.Run) == 24
