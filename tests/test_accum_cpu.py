"""CPU: the `accum_steps` configuration field (one optimizer step from N micro-batches) from config.py down to the C ABI -- what can be
checked without a GPU: the flag and its default, its validation in MISA.__init__, and the error codes of the new entry points, none of
which launches anything here (the pattern of test_embed_update_cpu.py::test_rows_update_rejects_bad_arguments_without_a_launch)."""
import ctypes as C

import pytest

from mmda_amd import _lib, make_config, MISA
from mmda_amd.config import get_config

EINVAL = -1


def test_config_field_and_default():
    assert get_config(parse=False).accum_steps == 1
    assert make_config().accum_steps == 1
    assert MISA(make_config(vocab_size=50)).accum_steps == 1
    assert MISA(make_config(vocab_size=50, accum_steps=4)).accum_steps == 4


@pytest.mark.parametrize("bad", [0, -1, 2.0, "2", None, True, False])
def test_bad_value_raises(bad):
    with pytest.raises(ValueError):
        MISA(make_config(vocab_size=50, accum_steps=bad))


def test_train_step_has_the_keywords():
    import inspect
    ps = inspect.signature(MISA.train_step).parameters
    assert ps["accum_index"].default == 0 and ps["accum_count"].default == 1


FAKE = C.c_void_p(256)          # 16-byte aligned, never dereferenced: every call below is refused (or empty) before a launch
ODD = C.c_void_p(260)           # 4-byte aligned only


def test_accumulate_rejects_bad_arguments_without_a_launch():
    lib = _lib.load()
    f = lib.mmda_grad_accumulate
    assert f(None, FAKE, 8, 1, None) == EINVAL and f(FAKE, None, 8, 0, None) == EINVAL
    assert f(ODD, FAKE, 8, 1, None) == EINVAL and f(FAKE, ODD, 8, 0, None) == EINVAL
    assert f(FAKE, FAKE, -1, 1, None) == EINVAL
    assert f(FAKE, FAKE, 0, 1, None) == 0 and f(FAKE, FAKE, 0, 0, None) == 0          # nothing to do, nothing launched


def test_clamp_adam_sum_rejects_bad_arguments_without_a_launch():
    lib = _lib.load()
    ok = dict(p=FAKE, acc=FAKE, g=FAKE, m=FAKE, v=FAKE, n=8, step=1)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.mmda_clamp_adam_sum(a["p"], a["acc"], a["g"], a["m"], a["v"], a["n"], 1e-3, 0.9, 0.999, 1e-8, 1.0, 0.5, a["step"], None)
    for k in ("p", "g", "m", "v"):
        assert call(**{k: None}) == EINVAL, k
        assert call(**{k: None}, acc=None) == EINVAL, k              # acc = NULL is mmda_clamp_adam, which checks the rest
    for k in ("p", "acc", "g", "m", "v"):
        assert call(**{k: ODD}) == EINVAL, k
    assert call(n=-1) == EINVAL and call(n=-1, acc=None) == EINVAL
    assert call(step=0) == EINVAL and call(step=0, acc=None) == EINVAL
    assert call(n=0) == 0 and call(n=0, acc=None) == 0


def test_rows_append_rejects_bad_arguments_without_a_launch():
    lib = _lib.load()
    ok = dict(ids_out=FAKE, rows_out=FAKE, offset=0, capacity=64, ids=FAKE, rows=FAKE, n=8, D=300, lengths=None, B=0)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.mmda_embed_rows_append(a["ids_out"], a["rows_out"], a["offset"], a["capacity"], a["ids"], a["rows"], a["n"], a["D"],
                                          a["lengths"], a["B"], None)
    for k in ("ids_out", "rows_out", "ids", "rows"):
        assert call(**{k: None}) == EINVAL, k
    assert call(ids_out=ODD) == EINVAL and call(ids=ODD) == EINVAL                     # int64 lists: 8-byte alignment
    assert call(rows=C.c_void_p(258)) == EINVAL and call(rows_out=C.c_void_p(258)) == EINVAL
    assert call(n=-1) == EINVAL and call(D=0) == EINVAL and call(offset=-1) == EINVAL
    assert call(lengths=FAKE, B=0) == EINVAL
    assert call(offset=60) == EINVAL and call(offset=65, n=0) == EINVAL and call(capacity=7) == EINVAL      # the list is too short
    assert call(n=0) == 0 and call(n=0, offset=64) == 0


def test_model_level_entries_reject_an_unbound_model():
    lib = _lib.load()
    acc = lib.mmda_misa_grad_accumulate
    step = lib.mmda_misa_adam_step_accumulated
    assert acc(None, FAKE, 1, None, None, 0, 0, None) == EINVAL
    assert step(None, FAKE, None, None, 0, 0, 1e-3, 1.0, 0.5, 1, None) == EINVAL
    m = MISA(make_config(vocab_size=50))                  # no buckets bound (no GPU): refused before anything is read
    assert acc(m._h, FAKE, 1, None, None, 0, 0, None) == EINVAL
    assert step(m._h, FAKE, None, None, 0, 0, 1e-3, 1.0, 0.5, 1, None) == EINVAL
    assert step(m._h, None, None, None, 0, 0, 1e-3, 1.0, 1.0, 1, None) == EINVAL


@pytest.mark.parametrize("n_batches,N,want", [
    (5, 2, [(0, 2), (1, 2), (0, 2), (1, 2), (0, 1)]),          # the leftover micro-batch makes a step of its own, scaled 1/1
    (6, 3, [(0, 3), (1, 3), (2, 3)] * 2),
    (2, 4, [(0, 2), (1, 2)]),                                  # fewer batches than accum_steps: one step of what there is
    (3, 1, [(0, 1)] * 3),
    (0, 2, []),
])
def test_solver_groups_batches_into_steps(n_batches, N, want):
    """the position and the count every micro-batch is issued with: the count is known at the first micro-batch of its step"""
    from mmda_amd.solver import Solver
    c = make_config(vocab_size=50, accum_steps=N)
    s = Solver(c, c, c, [f"b{i}" for i in range(n_batches)], None, None, is_train=True, model=None)
    got = list(s._micro_batches())
    assert [b for b, _, _ in got] == [f"b{i}" for i in range(n_batches)]
    assert [(k, cnt) for _, k, cnt in got] == want
