"""CPU: config.embed_update = 'deferred' (dense Adam's weights without a pass over the table per step) -- what can be checked without
a GPU: the value is accepted where 'dense' / 'sparse' / 'frozen' are, the others are still rejected, and the new entry points refuse bad
arguments before they launch anything.  Natively the mode is dense plus a switch: mmda_misa_set_embed_update keeps its three values."""
import ctypes as C

import pytest

from mmda_amd import _lib, make_config, MISA
from mmda_amd.config import get_config


def test_value_is_accepted():
    assert make_config(embed_update="deferred").embed_update == "deferred"
    assert get_config(parse=False, embed_update="deferred").embed_update == "deferred"
    assert get_config(parse=False).embed_update == "dense" and make_config().embed_update == "dense"
    m = MISA(make_config(vocab_size=50, embed_update="deferred"))
    assert m.embed_update == "deferred"
    assert len(m.state_dict()) == 99
    assert m.embed.weight.requires_grad is True and m.embed.weight.grad is None
    assert m.grad_floats == m.dense_floats                       # the bucket ends at the table, as in 'sparse' and 'frozen'
    assert m.embed_window == 256
    assert MISA(make_config(vocab_size=50, embed_update="deferred", embed_deferred_window=4)).embed_window == 4
    m.flush_embedding()                                          # no device state yet: nothing to do, nothing launched


@pytest.mark.parametrize("bad", ["lazy", "Dense", "", "Deferred", "defer", None, 1])
def test_other_values_are_still_rejected(bad):
    with pytest.raises(ValueError):
        MISA(make_config(vocab_size=50, embed_update=bad))


def test_window_must_be_positive_in_this_mode_only():
    assert MISA(make_config(vocab_size=50, embed_update="deferred", embed_deferred_window=1)).embed_window == 1
    with pytest.raises(ValueError):
        MISA(make_config(vocab_size=50, embed_update="deferred", embed_deferred_window=0))
    for mode in ("dense", "sparse", "frozen"):               # the other modes never read it
        assert MISA(make_config(vocab_size=50, embed_update=mode, embed_deferred_window=0)).embed_update == mode


def test_model_setter_error_codes():
    lib = _lib.load()
    fake = C.c_void_p(256)
    assert lib.mmda_misa_set_embed_deferred(None, fake, fake, 4, None) == -1             # MMDA_EINVAL
    assert lib.mmda_misa_embed_flush(None, None) == -1
    assert lib.mmda_misa_embed_deferred_step(None, 1e-3, 0.9, 0.999, 1e-8, 1.0, 1.0, 1, None) == -1
    keep = MISA(make_config(vocab_size=50))
    h = keep._h
    assert lib.mmda_misa_set_embed_update(h, 3) == -1            # still no fourth mode number
    assert lib.mmda_misa_set_embed_deferred(h, None, fake, 4, None) == -1
    assert lib.mmda_misa_set_embed_deferred(h, fake, None, 4, None) == -1
    assert lib.mmda_misa_set_embed_deferred(h, fake, fake, 0, None) == -1
    assert lib.mmda_misa_set_embed_deferred(h, fake, fake, -3, None) == -1
    for mode in (1, 2):                                          # binding needs the dense mode
        assert lib.mmda_misa_set_embed_update(h, mode) == 0
        assert lib.mmda_misa_set_embed_deferred(h, fake, fake, 4, None) == -1
    assert lib.mmda_misa_set_embed_update(h, 0) == 0
    assert lib.mmda_misa_set_embed_deferred(h, None, None, 0, None) == 0                 # off: nothing bound, nothing launched
    assert lib.mmda_misa_embed_deferred_step(h, 1e-3, 0.9, 0.999, 1e-8, 1.0, 1.0, 1, None) == -1      # nothing bound, nothing pending
    assert lib.mmda_misa_embed_flush(h, None) == 0                                      # nothing deferred: no launch
    del keep


def test_op_entry_points_reject_bad_arguments_without_a_launch():
    lib = _lib.load()
    fake = C.c_void_p(256)
    assert lib.mmda_embed_deferred_scalar_floats(4) == 8 and lib.mmda_embed_deferred_scalar_floats(0) == -1
    assert lib.mmda_embed_deferred_reset(None, 10, None) == -1
    assert lib.mmda_embed_deferred_reset(fake, 0, None) == -1
    ok = dict(P=fake, M=fake, V=fake, rs=fake, ring=fake, window=4, ids=fake, n=4, D=300, rows=fake, lengths=None, B=0, table_rows=10, step=1,
              seq=1, upto=1)

    def step(**kw):
        a = dict(ok, **kw)
        return lib.mmda_embed_rows_dense_adam(a["P"], a["M"], a["V"], a["rs"], a["ring"], a["window"], a["ids"], a["n"], a["D"], a["rows"],
                                              a["lengths"], a["B"], a["table_rows"], 1e-3, 0.9, 0.999, 1e-8, 1.0, 1.0, a["seq"], a["step"], None)

    def catch_up(**kw):
        a = dict(ok, **kw)
        return lib.mmda_embed_rows_catch_up(a["P"], a["M"], a["V"], a["rs"], a["ring"], a["window"], a["ids"], a["n"], a["D"], a["lengths"],
                                            a["B"], a["table_rows"], 0.9, 0.999, 1e-8, a["upto"], None)

    def flush(**kw):
        a = dict(ok, **kw)
        return lib.mmda_embed_rows_flush(a["P"], a["M"], a["V"], a["rs"], a["ring"], a["window"], a["D"], a["table_rows"], 0.9, 0.999, 1e-8,
                                         a["upto"], None)
    for call in (step, catch_up, flush):
        for k in ("P", "M", "V", "rs", "ring"):
            assert call(**{k: None}) == -1, (call.__name__, k)
        assert call(window=0) == -1 and call(window=-1) == -1
        assert call(D=0) == -1 and call(D=1025) == -1 and call(table_rows=0) == -1
    for call in (step, catch_up):
        assert call(ids=None) == -1 and call(n=-1) == -1 and call(lengths=fake, B=0) == -1
    assert step(rows=None) == -1 and step(step=0) == -1 and step(seq=0) == -1
    assert catch_up(upto=-1) == -1 and flush(upto=-1) == -1
    assert catch_up(n=0) == 0 and catch_up(upto=0) == 0 and flush(upto=0) == 0     # nothing to do: nothing launched
