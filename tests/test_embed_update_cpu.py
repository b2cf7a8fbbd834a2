"""CPU: the `embed_update` configuration field ('dense' / 'sparse' / 'frozen') from config.py down to the C ABI -- what can be
checked without a GPU: the flag and its default, validation where `precision` is validated, requires_grad of a frozen table, the new
entry points and their error codes."""
import ctypes as C

import pytest

from mmda_amd import _lib, make_config, MISA
from mmda_amd.config import get_config


def test_config_field_and_default():
    assert get_config(parse=False).embed_update == "dense"
    assert make_config().embed_update == "dense"
    for mode in ("dense", "sparse", "frozen"):
        m = MISA(make_config(vocab_size=50, embed_update=mode))
        assert m.embed_update == mode
        assert len(m.state_dict()) == 99
        assert m.embed.weight.requires_grad is (mode != "frozen")
        assert m.embed.weight.grad is None


@pytest.mark.parametrize("bad", ["Dense", "lazy", "", None, 1])
def test_unknown_value_raises(bad):
    with pytest.raises(ValueError):
        MISA(make_config(vocab_size=50, embed_update=bad))


def test_frozen_table_is_left_out_of_the_optimizer_filter():
    """reference solver.py:97-99: filter(lambda p: p.requires_grad, model.parameters())"""
    m = MISA(make_config(vocab_size=50, embed_update="frozen"))
    kept = [p for p in m.parameters() if p.requires_grad]
    assert all(p is not m.embed.weight for p in kept)
    assert len(kept) == len(list(m.parameters())) - 1
    assert m.grad_floats == m.dense_floats
    assert MISA(make_config(vocab_size=50)).grad_floats == m.dense_floats + 50 * 300


def _handle(lib):
    m = MISA(make_config(vocab_size=50))
    return m, m._h


def test_setter_error_codes():
    lib = _lib.load()
    assert lib.mmda_misa_set_embed_update(None, 1) == -1                 # MMDA_EINVAL
    keep, h = _handle(lib)
    for mode in (0, 1, 2):
        assert lib.mmda_misa_set_embed_update(h, mode) == 0
    for mode in (-1, 3, 99):
        assert lib.mmda_misa_set_embed_update(h, mode) == -1
    assert lib.mmda_misa_set_embed_update(h, 0) == 0
    del keep


def test_rows_update_rejects_bad_arguments_without_a_launch():
    lib = _lib.load()
    fake = C.c_void_p(256)
    ok = dict(P=fake, M=fake, V=fake, ids=fake, n=4, D=300, rows=fake, lengths=None, B=0, table_rows=10, step=1)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.mmda_embed_rows_sparse_adam(a["P"], a["M"], a["V"], a["ids"], a["n"], a["D"], a["rows"], a["lengths"], a["B"],
                                               a["table_rows"], 1e-3, 0.9, 0.999, 1e-8, 1.0, 1.0, a["step"], None)
    assert call(P=None) == -1 and call(M=None) == -1 and call(V=None) == -1
    assert call(ids=None) == -1 and call(rows=None) == -1
    assert call(n=-1) == -1 and call(D=0) == -1 and call(table_rows=0) == -1 and call(step=0) == -1
    assert call(lengths=fake, B=0) == -1
    assert call(n=0) == 0                                                # an empty list: nothing to do, nothing launched
