"""GPU: the optimizer launches give the bits that tests/golden/optim_bits.npz recorded from the build before the element functors and
walkers of optim.hip replaced the hand-written kernel bodies.  The other bitwise tests hold the forms of one build to each other (run
table == dense, rows == dense, sum == accumulate-then-step), so a mistake the forms share would pass them all; this one holds each form
to a recording.  tests/golden/gen_optim_bits.py made the fixture and owns the list of calls: replay() runs it here on the build under
test, once for the whole module.  Reference: the recorded outputs, compared with torch.equal -- no tolerance."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("gen_optim_bits", os.path.join(GOLDEN, "gen_optim_bits.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def bits():
    z = np.load(gen.FIXTURE, allow_pickle=False)
    inp = {k[4:]: z[k] for k in z.files if k.startswith("in::")}
    want = {k[5:]: z[k] for k in z.files if k.startswith("out::")}
    got = gen.replay(inp)
    assert set(got) == set(want) | set(gen.DERIVED)
    return inp, want, got


def _assert_equal(bits, prefix, expect):
    _, want, got = bits
    keys = sorted(k for k in want if k.startswith(prefix))
    assert len(keys) == expect, keys
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert torch.equal(torch.from_numpy(got[k]), torch.from_numpy(want[k])), (k, int((got[k] != want[k]).sum()))


@pytest.mark.parametrize("n", gen.DENSE_N)
def test_dense_adam_sum_accumulate_and_rmsprop_give_the_recorded_bits(bits, n):
    """P, M, V after three steps (clip 1, scale 0.5) and after a fourth with neither, for g and for acc + g; the accumulator after a copy
    and after two adds; P and square_avg after three RMSprop steps"""
    _assert_equal(bits, f"dense{n}::", 3 * 4 + 2 + 2)
    inp, _, got = bits
    assert np.array_equal(got[f"dense{n}::accumulate1::acc"], inp[f"dense{n}::g1"])          # first: a plain copy
    assert not np.array_equal(got[f"dense{n}::adam3::P"], got[f"dense{n}::sum3::P"])


@pytest.mark.parametrize("D", [d for _, d in gen.ROWS])
def test_masked_rows_give_the_recorded_bits(bits, D):
    """P, M, V after the want = 0 and the want = 1 pass; after the first, rows with mask 1 still hold the inputs"""
    _assert_equal(bits, f"rows{D}::", 3)
    inp, _, got = bits
    mask = inp[f"rows{D}::mask"].astype(bool)
    assert mask.any() and not mask.all()
    for k, name in zip("PMV", "pmv"):
        first, final, start = got[f"rows{D}::want0::{k}"], got[f"rows{D}::want1::{k}"], inp[f"rows{D}::{name}"]
        assert np.array_equal(first[~mask], final[~mask]) and np.array_equal(first[mask], start[mask]), k
        assert not np.array_equal(final[mask], start[mask]) and not np.array_equal(final[~mask], start[~mask]), k


def test_run_table_launches_give_the_recorded_bits(bits):
    """Adam, Adam over acc + g, RMSprop, and Adam over a slice of the table"""
    _assert_equal(bits, "runs::", 3 + 3 + 2 + 3)


def test_grid_stride_loop_gives_the_recorded_bit_sums(bits):
    """more quads than the capped grid has lanes: wrap-around sums of the bit patterns of P, M and V, Adam and Adam over acc + g"""
    assert gen.LARGE_N // 4 > 2048 * 256
    _assert_equal(bits, "large::", 2)
