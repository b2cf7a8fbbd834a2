"""GPU: the embedding-rows calls give the bits that tests/golden/embed_rows_bits.npz recorded from the build before the rows code moved
into embed_rows.hip (nine kernels and nine launchers then, three kernel templates and one launcher now).  The other bitwise tests hold
the list forms of one build to each other (short == sort == presorted) and to torch within a tolerance, so a mistake the forms share
would pass them all; this one holds each form to a recording.  tests/golden/gen_embed_rows_bits.py made the fixture and owns the list of
calls: replay() runs it here on the build under test, once for the whole module; tests/embed_rows_cases.py holds the lists, and
tests/test_embed_rows_cases_cpu.py proves they reach the branches.  Reference: the recorded outputs, compared with torch.equal -- no
tolerance."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("gen_embed_rows_bits", os.path.join(GOLDEN, "gen_embed_rows_bits.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def bits():
    z = np.load(gen.FIXTURE, allow_pickle=False)
    want = {k[5:]: z[k] for k in z.files if k.startswith("out::")}
    assert len(want) == len(z.files) == 54
    got = gen.replay()
    assert set(got) == set(want)
    return want, got


def _assert_equal(bits, prefix, expect):
    want, got = bits
    keys = sorted(k for k in want if k.startswith(prefix))
    assert len(keys) == expect, keys
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert torch.equal(torch.from_numpy(got[k]), torch.from_numpy(want[k])), (k, int((got[k] != want[k]).sum()))


def test_short_form_wide_rows_give_the_recorded_bits(bits):
    """D = 300, n = 200: the scatter-add (rows + bit sum), the sparse optimizer over the ragged list (P, M, V + bit sums)"""
    _assert_equal(bits, "short300::add::", 2)
    _assert_equal(bits, "short300::sparse_ragged::", 4)
    want, _ = bits
    assert want["short300::add::dW"].shape == (13, 300) and want["short300::sparse_ragged::P"].shape == (12, 300)


def test_short_form_narrow_rows_give_the_recorded_bits(bits):
    """D = 7: the scatter-add; the sparse and the deferred optimizer with and without lengths (the deferred one after its update, bit
    sums, and after the flush, rows + bit sums)"""
    _assert_equal(bits, "short7::add::", 2)
    for name in ("ragged", "full"):
        _assert_equal(bits, f"short7::sparse_{name}::", 4)
        _assert_equal(bits, f"short7::dense_{name}::", 1 + 4)
    want, _ = bits
    assert not np.array_equal(want["short7::sparse_ragged::P"], want["short7::sparse_full::P"])        # the lengths matter


def test_deferred_sequence_gives_the_recorded_bits(bits):
    """three updates with window 2 (a flush inside), a catch-up of a second list, the last flush: bit sums of P, M, V after each of the
    five, the rows of both lists and row_step at the end"""
    _assert_equal(bits, "short300::deferred::", 5 + 3 + 1)
    want, _ = bits
    assert want["short300::deferred::flushed::P"].shape == (21, 300)
    assert (want["short300::deferred::row_step"] == 3).all()
    sums = [tuple(want[f"short300::deferred::{k}::bit_sums"]) for k in ("update1", "catch_up", "update2", "update3", "flushed")]
    assert len(set(sums)) == 5                                                                        # every stage wrote something


@pytest.mark.parametrize("name", ["plain", "negatives"])
def test_segment_sum_gives_the_recorded_bits(bits, name):
    """n = 203 through the sort form with the caller's work buffer: the rows it overwrote and the bit sum of the gradient"""
    _assert_equal(bits, f"seg::{name}::", 2)
    want, _ = bits
    assert want[f"seg::{name}::dW"].shape == (24, gen.ec.SEG_D)


def test_sort_form_small_table_gives_the_recorded_bits(bits):
    """n = 3200, 120 rows of 300: the scatter-add, the sparse optimizer, the deferred optimizer after its update and after the flush"""
    _assert_equal(bits, "long120::add::", 2)
    _assert_equal(bits, "long120::sparse::", 4)
    _assert_equal(bits, "long120::dense::", 1 + 4)
    want, _ = bits
    assert want["long120::sparse::P"].shape == (19, 300) and want["long120::add::dW"].shape == (20, 300)


def test_sort_form_large_table_gives_the_recorded_bit_sums(bits):
    """n = 3200, 20 000 rows of 7 (two key passes): wrap-around sums of the bit patterns of the whole arrays"""
    _assert_equal(bits, "long20000::", 1 + 1 + 2)
