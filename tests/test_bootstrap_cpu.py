"""CPU: the bootstrap's definitions (mmda_amd/bootstrap.py) -- the draws, the weighted restatements of the decision and ranking figures
against the MATERIALISED resample through the existing ``get_metrics`` and ``rank_counts_host`` + ``figures_from_counts``, the summary
arithmetic against numpy's nan-functions, what the bootstrap estimates on a case whose exact bootstrap variance is known, the plan
and the refusals.  Bounds: tests/bootstrap_cases.py."""
import numpy as np
import pytest

import bootstrap_cases as bc
from mmda_amd import bootstrap as bt
from mmda_amd import step_rules
from mmda_amd._lib import MMDAError
from mmda_amd.modality import keep_bits

CPU_SHAPES = [(1, 1), (2, 1), (37, 6), (300, 16), (257, 6)]


# ------------------------------------------------------------------------------------------------ draws
def test_draws_are_in_range_deterministic_and_independent_of_R():
    for n in (1, 2, 37, 300, 16385):
        j = bt.resample_indices(bc.SEED, 5, n)
        assert j.shape == (5, n) and j.dtype == np.int64 and j.min() >= 0 and j.max() < n
        assert np.array_equal(j, bt.resample_indices(bc.SEED, 5, n))
        assert np.array_equal(j[:3], bt.resample_indices(bc.SEED, 3, n))           # replicate r does not move when R grows
        w = bt.resample_weights(bc.SEED, 5, n)
        assert w.shape == (6, n) and (w.sum(1) == n).all() and (w[5] == 1).all()
        assert np.array_equal(w[2], np.bincount(j[2], minlength=n))
    assert not np.array_equal(bt.resample_indices(0, 2, 300), bt.resample_indices(1, 2, 300))
    assert not np.array_equal(bt.resample_indices(0, 2, 300)[0], bt.resample_indices(0, 2, 300)[1])


def test_draws_are_uniform_and_a_stream_of_their_own():
    j = bt.resample_indices(0, 64, 37)
    counts = np.bincount(j.reshape(-1), minlength=37)
    chi2 = float(((counts - 64.0) ** 2 / 64.0).sum())
    assert chi2 < 36 + 5 * np.sqrt(72)                                             # 36 degrees of freedom: mean 36, sd sqrt(72)
    # site 12 is not site 11: the uniforms behind the draws differ from those behind modality.keep_bits at the same seed and index
    from mmda_amd.modality import SITE_MODALITY, _rng_u32
    idx = np.arange(64, dtype=np.uint64)
    assert bt.SITE_BOOTSTRAP == 12 == SITE_MODALITY + 1
    assert (_rng_u32(0, bt.SITE_BOOTSTRAP, idx) != _rng_u32(0, SITE_MODALITY, idx)).all()
    # ... so whether sample s keeps its text under modality dropout says nothing about draw k = 3 s of replicate 0 over two rows
    kept = keep_bits(0, (0.5, 0.0, 0.0), np.arange(256)) & 1
    drawn = bt.resample_indices(0, 1, 2 * 3 * 256)[0, 0:3 * 256:3] >= 3 * 256
    assert 64 < int((kept == drawn).sum()) < 192
    never = [int((bt.resample_weights(0, 65, n)[:65, 0] == 0).sum()) for n in (37, 300)]
    assert all(5 <= k <= 45 for k in never)                                        # a given row is absent from about 1/e of the replicates


# ------------------------------------------------------------------------------------------------ weighted == materialised
@pytest.mark.parametrize("shape", CPU_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_weighted_decisions_equal_the_materialised_resample(shape):
    n, C = shape
    case, R = bc.case(n, C), 65
    state, figures = bt.decisions_host(case["labels"], case["truth_d"], bc.SEED, R)
    assert state.shape == (R + 1, 3 * C + 2) and state.dtype == np.int64 and figures.shape == (R + 1, 10 + 3 * C)
    j = bt.resample_indices(bc.SEED, R, n)
    for r in range(R + 1):
        rows = j[r] if r < R else np.arange(n)
        want_state, want = bc.materialised_decisions(case["labels"], case["truth_d"], rows)
        assert np.array_equal(state[r], want_state), r
        bc.check_decision_figures(figures[r], want_state, want, C)
    assert len(bt.decision_names(C)) == 10 + 3 * C


@pytest.mark.parametrize("shape", bc.SWEEP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_a_sweep_row_and_the_identity_replicate_agree_on_the_host(shape):
    """The inputs of tests/test_gpu_eval_terms.py hold what they are meant to, and the numpy restatements of its two sides
    (``table_from_counts``, ``figures_from_states``) agree on them to the bound of the decision figures."""
    from mmda_amd import calibrate as cal
    n, C = shape
    scores, truth_d, labels = bc.sweep_case(n, C)
    assert bc.SWEEP_GRID[2] == np.float32(bc.THRESHOLD) and not truth_d[n // 5].any() and not any(l[n // 5].any() for l in labels)
    if C >= 6:
        assert np.isnan(scores).any() and np.isposinf(scores).any() and np.isneginf(scores).any()
    table = cal.table_from_counts(*cal.sweep_counts(scores, truth_d, bc.SWEEP_GRID), n)
    for k in range(len(bc.SWEEP_GRID)):
        _, figures = bt.decisions_host(labels[k], truth_d, bc.SEED, 1)
        assert bc.same_bits(table[k, 0], figures[1, 0])             # one division of the same two integers
        assert (np.abs(table[k, 1:] - figures[1, 1:10]) <= (C + 2) * bc.EPS).all(), k


@pytest.mark.parametrize("shape", CPU_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_weighted_ranking_equals_the_materialised_resample(shape):
    n, C = shape
    case, R = bc.case(n, C), 65
    got = bt.ranking_host(case["scores"], case["truth"], bc.SEED, R, 0.95)
    assert got.shape == (R + 1, C + 1, 6)
    j = bt.resample_indices(bc.SEED, R, n)
    absent = 0
    for r in range(R + 1):
        rows = j[r] if r < R else np.arange(n)
        want = bc.materialised_ranking(case["scores"], case["truth"], rows)
        bc.check_rank_table(got[r], want, C)
        absent += int(np.isnan(want[:C, 2]).sum())
    if C >= 6:
        assert absent >= 2 * (R + 1)                                               # the no-positive and the no-negative class, every replicate
    assert len(bt.ranking_names(C)) == len(bt.ranking_names(C, failure=True)) == 6 * (C + 1)
    assert bt.ranking_names(C, failure=True)[-1] == "macro_fpr_at_95tpr" and bt.ranking_names(C)[-3] == "map"


# ------------------------------------------------------------------------------------------------ summary
@pytest.mark.parametrize("R", [1, 2, 3, 64, 65, 2000])
def test_summary_against_numpy(R):
    x = bc.summary_table(R, 9)
    alpha = 0.05
    got = bt.summary_host(x, alpha)
    assert got.shape == (9, 6)
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for f in range(9):
                v = x[:R, f]
                m = int((~np.isnan(v)).sum())
                tol = max(m, 1) * 2.0 ** -50 * np.nanmax(np.abs(v), initial=0.0)
                assert got[f, 5] == m and bc.same_bits(got[f, 0], x[R, f])
                if m == 0:
                    assert np.isnan(got[f, 1:5]).all()
                    continue
                assert abs(got[f, 1] - np.nanmean(v)) <= tol
                assert abs(got[f, 3] - np.nanpercentile(v, 2.5)) <= tol and abs(got[f, 4] - np.nanpercentile(v, 97.5)) <= tol
                assert got[f, 3] <= got[f, 4]
                if m < 2:
                    assert np.isnan(got[f, 2])
                else:
                    assert abs(got[f, 2] - np.nanstd(v, ddof=1)) <= tol
    with pytest.raises(ValueError, match="alpha"):
        bt.summary_host(x, 1.0)


@pytest.mark.parametrize("R", [1, 2, 65])
def test_compare_columns_are_exact(R):
    a, b = bc.summary_table(R, 9, seed=1), bc.summary_table(R, 9, seed=2)
    got = bt.summary_host(a, 0.1, other=b)
    assert got.shape == (9, 9)
    assert np.array_equal(got[:, :6], bt.summary_host(a - b, 0.1), equal_nan=True)
    for f in range(9):
        d = [a[r, f] - b[r, f] for r in range(R)]
        d = [v for v in d if v == v]
        m, le, ge = len(d), sum(v <= 0 for v in d), sum(v >= 0 for v in d)
        assert got[f, 6] == (1 + le) / (m + 1) and got[f, 7] == (1 + ge) / (m + 1)
        assert got[f, 8] == min(1.0, 2.0 * min(got[f, 6], got[f, 7]))
    same = bt.summary_host(a, 0.1, other=a)                                        # a table against itself
    defined = ~np.isnan(a[:R]).all(0)
    assert (same[defined, 1] == 0).all() and (same[defined, 3] == 0).all() and (same[defined, 4] == 0).all()
    assert (same[:, 8] == 1).all()


# ------------------------------------------------------------------------------------------------ statistics
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_the_bootstrap_variance_of_a_mean(seed):
    """One class, truth all ones, predictions Bernoulli(0.3), n = 400: recall is the mean of n draws from the table, whose exact
    bootstrap variance is p(1 - p) / n at the table's own p."""
    n, R = 400, 2000
    labels = (np.random.default_rng(100 + seed).random((n, 1)) < 0.3).astype(np.float32)
    truth = np.ones((n, 1), dtype=np.float32)
    _, figures = bt.decisions_host(labels, truth, seed, R)
    recall = bt.decision_names(1).index("recall[0]")
    s = bt.summary_host(figures, 0.05)[recall]
    p = float(labels.sum()) / n
    sd = np.sqrt(p * (1 - p) / n)
    assert s[0] == p and s[5] == R
    print("relative std error", s[2] / sd - 1, "unit", 1 / np.sqrt(2 * (R - 1)))
    assert abs(s[2] / sd - 1) <= 5 / np.sqrt(2 * (R - 1))
    assert abs(s[1] - p) <= 5 * sd / np.sqrt(R)
    assert s[3] < p < s[4]
    same = bt.summary_host(figures[:, :10], 0.05, other=figures[:, :10])
    assert (same[:, 1] == 0).all() and (same[:, 8] == 1).all()


# ------------------------------------------------------------------------------------------------ plan
def test_the_plan_names_the_form_of_every_gpu_shape():
    for n, C in bc.gpu_shapes():
        for R in bc.replicates((n, C)):
            p = bt.boot_plan(n, C, R)
            assert p.form == (1 if n <= 16384 else 2) and p.threads == 256 and p.state_words == 3 * C + 2
            assert p.lds_bytes == (4 * n if p.form == 1 else 0) and p.rank_lds_bytes == (8 * n if n <= 16384 else 0)
            assert p.wgs_per_replicate == min(16, -(-n // 4096)) and p.lds_rows == 16384 and p.max_replicates == 8192
    assert bt.boot_plan(16326, 6, 2000).form == 1 and bt.boot_plan(16326, 6, 2000).wgs_per_replicate == 4
    assert bt.boot_plan(1 << 20, 16, 8192).wgs_per_replicate == 16
    assert {s[0] for s in bc.gpu_shapes()} >= {255, 256, 257, 16384, 16385}
    for bad in ((0, 6, 1), (1, 0, 1), (1, 17, 1), (1, 6, 0), (1, 6, 8193), ((1 << 20) + 1, 6, 1)):
        with pytest.raises(MMDAError, match="mmda_boot_plan_describe"):
            bt.boot_plan(*bad)


# ------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_raises_by_name():
    rules = dict(step_rules.BOOTSTRAP_RULES)
    assert list(rules) == ["boot_sentiment", "boot_sharded", "boot_replicates", "boot_rows", "boot_classes", "boot_rank_rows", "boot_compare"]
    with pytest.raises(MMDAError, match="task='sentiment' with the bootstrap"):
        step_rules.bootstrap_check(task="sentiment", replicates=5)
    with pytest.raises(MMDAError, match="must not be sharded"):
        step_rules.bootstrap_check(sharded=(0, 2), mode="dev")
    for bad in (0, 8193, -1, 2.5, True, None):
        with pytest.raises(MMDAError, match="replicates must be an integer in 1 .. 8192"):
            bt.Bootstrap(10, bad)
    for bad in (0, (1 << 20) + 1):
        with pytest.raises(MMDAError, match="outside 1 .. 2\\^20"):
            bt.Bootstrap(bad, 5)
    with pytest.raises(MMDAError, match="1 .. 16 classes"):
        bt.decisions_host(np.zeros((4, 17)), np.zeros((4, 17)), 0, 2)
    with pytest.raises(MMDAError, match="over the limit of 16384 rows"):
        bt.ranking_host(np.zeros((16385, 1), np.float32), np.zeros((16385, 1)), 0, 1)
    a, b = bt.Bootstrap(10, 5), bt.Bootstrap(10, 5)
    ra = bt.BootstrapResult(a, ("decisions", 2), None, bt.decision_names(2))
    rb = bt.BootstrapResult(b, ("decisions", 2), None, bt.decision_names(2))
    rc = bt.BootstrapResult(a, ("decisions", 3), None, bt.decision_names(3))
    with pytest.raises(MMDAError, match="compare needs two results of the same Bootstrap.*different Bootstrap"):
        a.compare(ra, rb)
    with pytest.raises(MMDAError, match="compare needs two results.*figure sets differ"):
        a.compare(ra, rc)
    with pytest.raises(MMDAError, match="compare needs two results.*BootstrapResults"):
        a.compare(ra, None)
    with pytest.raises(MMDAError, match="GPU only"):
        bt.Bootstrap(10, 5, device="cpu")


def test_the_flag_defaults_to_nothing_and_sentiment_is_refused_at_build():
    from mmda_amd.config import DEFAULTS, get_config, make_config
    from mmda_amd.solver import Solver
    assert DEFAULTS["bootstrap"] == 0 and make_config().bootstrap == 0
    assert get_config(parse=False).bootstrap == 0 and get_config(parse=False, bootstrap=200).bootstrap == 200
    cfg = make_config(task="sentiment", num_classes=1, bootstrap=5, device="cpu", vocab_size=32)
    with pytest.raises(MMDAError, match="task='sentiment' with the bootstrap"):
        Solver(cfg, cfg, cfg, None, None, None, is_train=False).build()
    cfg = make_config(bootstrap=9000, device="cpu", vocab_size=32)
    with pytest.raises(MMDAError, match="replicates must be an integer"):
        Solver(cfg, cfg, cfg, None, None, None, is_train=False).build()
