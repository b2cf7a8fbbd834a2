"""GPU: a bound workspace answers the pinned layout.  tests/workspace_layout_cases.py holds, for every configuration and shape, the
offset of every name of mmda_misa_tensor_offset as the build in front of carve() gave it; here a real buffer is bound (the binding
enqueues only the clears of the exchange and GRU-gradient regions: no kernel runs) and every name is asked.  Reference: the recorded
numbers, compared exactly."""
import pytest
import torch

import workspace_layout_cases as wl
from mmda_amd import make_config, MISA, _lib

pytestmark = pytest.mark.gpu

EINVAL = -1


@pytest.fixture(scope="module")
def buf():
    """one buffer for the module, as large as the largest case bound here (GRU at B = 33, T = 7: 102 MB)"""
    n = max(wl.TOTALS[(c, B, T)] for c in wl.CONFIGS for (B, T) in wl.GPU_SHAPES)
    return torch.empty(n, dtype=torch.float32, device="cuda:0")


def _bind(lib, m, buf, floats, B, T):
    return lib.mmda_misa_set_workspace_async(m._h, buf.data_ptr(), floats, B, T, _lib.stream_ptr())


def _offsets(lib, m):
    return tuple(lib.mmda_misa_tensor_offset(m._h, n.encode()) for n in wl.NAMES)


@pytest.mark.parametrize("cfg", list(wl.CONFIGS))
def test_every_named_offset_matches_the_pinned_layout(buf, cfg):
    lib = _lib.load()
    m = MISA(make_config(vocab_size=50, **wl.CONFIGS[cfg]))
    for (B, T) in wl.GPU_SHAPES:                       # one handle re-carved: a new B, then a new B again
        assert _bind(lib, m, buf, wl.TOTALS[(cfg, B, T)], B, T) == 0, (cfg, B, T)
        assert _offsets(lib, m) == wl.OFFSETS[(cfg, B, T)], (cfg, B, T)
        assert lib.mmda_misa_tensor_offset(m._h, b"no_such_tensor") == -1
        assert lib.mmda_misa_tensor_offset(m._h, b"") == -1
    torch.cuda.synchronize()


def test_exchange_regions_do_not_move_with_T(buf):
    lib = _lib.load()
    m = MISA(make_config(vocab_size=50))
    x = wl.NAMES.index("xchg_t")
    assert wl.NAMES[x:x + 3] == ("xchg_t", "xchg_v", "xchg_a")
    seen = []
    for T in (3, 7, 3):
        need = lib.mmda_misa_workspace_floats(m._h, 5, T)
        assert _bind(lib, m, buf, need, 5, T) == 0
        seen.append(_offsets(lib, m)[x:x + 3])
    assert seen[0] == seen[1] == seen[2] == wl.OFFSETS[("default", 5, 3)][x:x + 3]
    assert min(seen[0]) >= 0
    torch.cuda.synchronize()


def test_a_buffer_one_float_short_is_refused_and_changes_nothing(buf):
    lib = _lib.load()
    m = MISA(make_config(vocab_size=50))
    assert _bind(lib, m, buf, wl.TOTALS[("default", 5, 3)] - 1, 5, 3) == EINVAL
    assert _offsets(lib, m) == (-1,) * len(wl.NAMES)                  # nothing was bound: nothing has an offset
    assert _bind(lib, m, buf, wl.TOTALS[("default", 5, 3)], 5, 3) == 0
    assert _bind(lib, m, buf, wl.TOTALS[("default", 33, 7)] - 1, 33, 7) == EINVAL
    assert _offsets(lib, m) == wl.OFFSETS[("default", 5, 3)]          # the previous carve still answers
    assert _bind(lib, m, buf, wl.TOTALS[("default", 33, 7)], 33, 7) == 0
    assert _offsets(lib, m) == wl.OFFSETS[("default", 33, 7)]
    torch.cuda.synchronize()
