"""What the single device bodies of csrc/eval_terms.h and csrc/eval_counts.hip guarantee, and separate copies did not: two reports of
the same decisions agree bit for bit.

Decision figures: a sweep over five cut-offs (``bootstrap_cases.THRESHOLD`` among them) of the decision tables of
``bootstrap_cases.case`` -- ``value_case``'s scores with NaN and +-inf, which go through ``s > t`` on both sides -- against the
identity replicate of ``Bootstrap.decisions`` over the labels ``scores > grid[k]``: all ten columns, as 64-bit words.  Row n // 5 is
cleared in the truth and in the scores (``bootstrap_cases.sweep_case``), so it predicts nothing at any cut-off and takes the
``max(union, 1)`` branch of the accuracy on both sides.  Shapes (2, 1), (37, 6) and (300, 16), where the class sums are longest.
tests/test_bootstrap_cpu.py shows with the numpy restatements that the two sides agree to the existing bounds on these inputs and
that the inputs hold what they are meant to.

Evaluation counts: N = 37, C = 6 is one wave, so the Jaccard sum has one order, and the WHOLE state of ``mmda_eval_accumulate`` over
labels equals that of ``mmda_eval_accumulate_thr`` over the scores, word 3 C included."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bootstrap_cases as bc
from mmda_amd import bootstrap as bt

DEV = "cuda:0"


@pytest.mark.parametrize("shape", bc.SWEEP_SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_sweep_row_equals_the_bootstraps_identity_row_bit_for_bit(shape):
    from mmda_amd import ThresholdSweep
    n, C = shape
    scores, truth_d, labels = bc.sweep_case(n, C)
    y = torch.from_numpy(truth_d).to(DEV)
    sweep = ThresholdSweep(C, bc.SWEEP_GRID, DEV)
    sweep.update(torch.from_numpy(scores).to(DEV), y)
    table = sweep.table()
    bs = bt.Bootstrap(n, 1, bc.SEED, DEV)
    for k in range(len(bc.SWEEP_GRID)):
        row = bs.decisions(torch.from_numpy(labels[k]).to(DEV), y).figures[1, :10].cpu().numpy()
        assert np.array_equal(table[k].view(np.int64), row.view(np.int64)), \
            (k, "largest difference in units of 2^-52:", np.abs(table[k] - row).max() / bc.EPS, [x.hex() for x in table[k]], [x.hex() for x in row])


def test_eval_accumulate_over_labels_and_over_scores_give_the_same_state():
    from mmda_amd import _lib
    N, C = 37, 6
    case = bc.case(N, C)
    s, t = (torch.from_numpy(case[k]).to(DEV) for k in ("scores", "truth_d"))
    thr = torch.tensor([0.35, 0.2, 0.01, 0.5, 0.6, 0.99], device=DEV)
    labels = (s > thr).float()
    lib, st = _lib.load(), _lib.stream_ptr()
    a, b = (torch.zeros(3 * C + 2, dtype=torch.float64, device=DEV) for _ in range(2))
    _lib.check(lib.mmda_eval_accumulate(labels.data_ptr(), t.data_ptr(), N, C, a.data_ptr(), st), "mmda_eval_accumulate")
    _lib.check(lib.mmda_eval_accumulate_thr(s.data_ptr(), t.data_ptr(), N, C, thr.data_ptr(), None, b.data_ptr(), st),
               "mmda_eval_accumulate_thr")
    assert float(a[3 * C + 1]) == N and 0.0 < float(a[3 * C]) < N
    assert torch.equal(a.view(torch.int64), b.view(torch.int64)), (a.tolist(), b.tolist())
