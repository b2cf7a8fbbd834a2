"""GPU: reliability tables and logit scaling -- ``mmda_reliab_accumulate`` / ``mmda_reliab_finish``, ``mmda_scaling_fit`` and
``mmda_scaling_apply`` against the numpy definitions of mmda_amd/reliability.py (tests/test_reliability_cpu.py checks those against
sklearn, a float64 restatement and scipy), and ``Solver.reliability`` / ``fit_scaling`` / ``calibrate(scaling=)`` / ``eval(scaling=)``
end to end on the tiny model of tests/test_gpu_calibrate.py.

Bounds.  Collector: every integer of the state equals the host's; ECE, MCE and the diagram are functions of those integers and one
division, and ``sum_sq`` is restated in the kernel's own order (``reliability.ordered_sum``): all compared bit for bit.  ``sum_nll``,
``brier`` and ``nll`` are within ``(n + 2) 2^-53`` relative of numpy's: the terms are non-negative, so the recursive-summation bound
holds against the sum in any order, and the 2 covers the device ``log``'s ulp (n is at most 513 x 16 = 8208 here).  Fit: the mean-NLL
gradient recomputed in numpy float64 at the device's parameters is at most 1e-9 (its rounding floor is near 16 x 2^-53 x a few, about
1e-14; the iteration stops at 1e-12); with the smallest Hessian eigenvalue of a case at least 1e-3 the parameters are then within
sqrt(2) 1e-9 / 1e-3 of the optimum and scipy within its own 1e-7: 2e-6.  The NLL at the fit is at most the NLL at (1, 0), which is
feasible.  Apply: 2 fp32 ulp of the float64 definition rounded to fp32; 1 ulp of the clamped input under the identity."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import reliability_cases as rc
from mmda_amd import _lib
from mmda_amd import reliability as rel

DEV = "cuda:0"
GUARD = 8                                                            # sentinel words either side of a buffer
MARK = 0x5A5A5A5A5A5A5A5A


def _guarded(words):
    """an int64 device buffer of ``words`` zeroed words between two runs of sentinels, and the view between them"""
    buf = torch.full((words + 2 * GUARD,), MARK, dtype=torch.int64, device=DEV)
    buf[GUARD:GUARD + words] = 0
    return buf, buf[GUARD:GUARD + words]


def _guards_intact(buf):
    b = buf.cpu()
    return bool((b[:GUARD] == MARK).all() and (b[-GUARD:] == MARK).all())


def _collect(p, t, M, splits):
    """the state words, the figures and the diagram (host arrays) after accumulating the row ranges ``splits`` and finishing; asserts
    the sentinels and the ticket"""
    lib = _lib.load()
    N, C = p.shape
    pd, td = torch.from_numpy(p).to(DEV), torch.from_numpy(t).to(DEV)
    sbuf, state = _guarded(rel.state_words(C, M))
    fbuf, fig = _guarded((C + 2) * 8)
    dbuf, dia = _guarded(C * M * 3)
    for a, b in splits:
        pa, ta = (pd[a:b].contiguous(), td[a:b].contiguous()) if b > a else (pd, td)     # an empty slice has no pointer: N = 0 of the table
        _lib.check(lib.mmda_reliab_accumulate(pa.data_ptr(), ta.data_ptr(), b - a, C, M, state.data_ptr(), _lib.stream_ptr()), "accumulate")
        assert int(state[0]) == 0                                    # the ticket is 0 between launches
    _lib.check(lib.mmda_reliab_finish(state.data_ptr(), C, M, fig.data_ptr(), dia.data_ptr(), _lib.stream_ptr()), "finish")
    torch.cuda.synchronize()
    assert _guards_intact(sbuf) and _guards_intact(fbuf) and _guards_intact(dbuf)
    return (state.cpu().numpy().copy(), fig.cpu().numpy().view(np.float64).reshape(C + 2, 8).copy(),
            dia.cpu().numpy().view(np.float64).reshape(C, M, 3).copy())


def _within(got, want, n):
    """|got - want| <= (n + 2) 2^-53 |want|, elementwise; NaN only where both are"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    return bool((np.abs(got - want)[ok] <= (np.asarray(n, np.float64) + 2.0)[ok] * 2.0 ** -53 * np.abs(want)[ok]).all())


# ------------------------------------------------------------------------------------------------ the collector
@pytest.mark.parametrize("N", rc.COLLECTOR_N)
def test_collector_equals_the_numpy_definition(N):
    for C in rc.COLLECTOR_C:
        for M in rc.COLLECTOR_M:
            p, t = rc.prob_table(N, C, M, seed=1000 * C + M)
            want = rel.state_host(p, t, M)
            sq, _ = rel.elementwise_host(p, t)
            n = want["cnt"].sum(1).astype(np.float64)
            want_fig, want_dia = rel.figures_from_state(want)
            runs = []
            for splits in ([(0, N)], rc.ragged_splits(N, seed=N + C + M)):
                words, fig, dia = _collect(p, t, M, splits)
                got, ticket = rel.unpack_state(words, C, M)
                tag = (N, C, M, splits)
                assert ticket == 0 and int(np.asarray(words).view(np.uint64)[1]) == 0, tag
                for k in ("cnt", "pos", "sum_p", "n_nan"):
                    assert np.array_equal(got[k], want[k]), (k, tag)
                order = None
                for a, b in splits:                                  # an empty batch launches nothing and adds nothing
                    order = rel.ordered_sum(sq[a:b], order)
                assert np.array_equal(got["sum_sq"], order), tag
                assert _within(got["sum_nll"], want["sum_nll"], n), tag
                # the finish launch restates figures_from_state over its own state, bit for bit ...
                own_fig, own_dia = rel.figures_from_state(got)
                np.testing.assert_array_equal(fig, own_fig, err_msg=str(tag))
                np.testing.assert_array_equal(dia, own_dia, err_msg=str(tag))
                # ... and against the host's state everything that follows from the integers is equal, the two means within the bound
                np.testing.assert_array_equal(fig[:, :6], want_fig[:, :6], err_msg=str(tag))
                np.testing.assert_array_equal(dia, want_dia, err_msg=str(tag))
                rows, rows_n = list(range(C)) + [C + 1], np.concatenate([n, [n.sum()]])        # the classes and the pooled row
                assert _within(fig[rows, 6], want_fig[rows, 6], rows_n) and _within(fig[rows, 7], want_fig[rows, 7], rows_n), tag
                runs.append((words, fig, dia))
            # integers do not depend on the split; a second run on fresh buffers gives the same bits
            words2, fig2, dia2 = _collect(p, t, M, [(0, N)])
            assert np.array_equal(words2, runs[0][0])
            np.testing.assert_array_equal(fig2, runs[0][1])
            np.testing.assert_array_equal(runs[0][2], runs[1][2])
            np.testing.assert_array_equal(runs[0][1][:, :6], runs[1][1][:, :6])


def test_python_collector_and_result():
    p, t = rc.prob_table(300, 6, 15, seed=4)
    pd, td = torch.from_numpy(p).to(DEV), torch.from_numpy(t).to(DEV)
    ev = rel.ReliabilityEval(6, device=DEV)
    ev.update(pd[:100], td[:100]).update(pd[100:100], td[100:100]).update(pd[100:], td[100:])
    assert ev.rows == 300
    res = ev.result()
    assert res.figures.is_cuda and res.figures.shape == (8, 8) and res.diagram.shape == (6, 15, 3) and res.C == 6 and res.bins == 15
    want_fig, want_dia = rel.reliability_host(p, t, 15)
    np.testing.assert_array_equal(res.cpu().figures.numpy()[:, :6], want_fig[:, :6])
    np.testing.assert_array_equal(res.cpu().diagram.numpy(), want_dia)
    d = res.as_dict()
    assert d["ece"] == want_fig[:6, 4].tolist() and d["pooled_ece"] == want_fig[7, 4] and d["macro_mce"] == want_fig[6, 5]
    one = rel.reliability_metrics(pd, td)
    np.testing.assert_array_equal(one.cpu().figures.numpy()[:, :6], want_fig[:, :6])
    ev.reset()
    assert ev.rows == 0 and int(ev.state.abs().sum()) == 0
    empty = ev.result().cpu()
    assert empty.figures[:, 0].tolist() == [0.0] * 8 and bool(torch.isnan(empty.figures[:, 2:]).all())
    with pytest.raises(ValueError, match="must both be"):
        ev.update(pd[:, :5], td[:, :5])
    with pytest.raises(_lib.MMDAError, match="no CPU fallback"):
        ev.update(pd.cpu(), td.cpu())
    with pytest.raises(ValueError, match="2\\^20"):
        big = rel.ReliabilityEval(1, device=DEV)
        big.rows = rel.MAX_ROWS
        big.update(pd[:1, :1], td[:1, :1])


# ------------------------------------------------------------------------------------------------ the fit
def _fit_bits(sc):
    c = sc.cpu()
    return c.a.numpy().tobytes() + c.b.numpy().tobytes() + c.status.numpy().tobytes() + c.iterations.numpy().tobytes()


@pytest.mark.parametrize("case", rc.fit_cases(), ids=lambda c: f"{c[0]}x{c[1]}-{c[3]}-{'per_class' if c[4] else 'shared'}-a{c[2][0]}")
def test_fit_reaches_the_optimum(case):
    N, C, true, how, per_class, seed = case
    s, t = rc.fit_table(N, C, true, how, per_class, seed)
    sd, td = torch.from_numpy(s).to(DEV), torch.from_numpy(t).to(DEV)
    sc = rel.fit_scaling(sd, td, how=how, per_class=per_class)
    assert sc.a.is_cuda and sc.how == how and sc.per_class is per_class and len(sc) == C
    got = sc.cpu()
    a, b, status, iters = got.a.numpy(), got.b.numpy(), got.status.numpy(), got.iterations.numpy()
    assert (status == 0).all() and (iters >= 1).all() and (iters <= 64).all(), (status, iters)
    if how == "temperature":
        assert (b == 0).all()
    if not per_class:
        assert (a == a[0]).all() and (b == b[0]).all() and (iters == iters[0]).all()
    at_fit = rel.mean_nll_host(s, t, a, b, per_class)
    for f, g, H in at_fit:
        assert np.abs(g[:1] if how == "temperature" else g).max() <= 1e-9, (g, iters)
    sa, sb = rc.scipy_fit(s, t, how, per_class)
    assert np.abs(a - sa).max() <= 2e-6 and np.abs(b - sb).max() <= 2e-6, (a, sa, b, sb)
    for (f, _, _), (f0, _, _) in zip(at_fit, rel.mean_nll_host(s, t, np.ones(C), np.zeros(C), per_class)):
        assert f <= f0
    # frozen groups keep their bits through further launches; a second run gives the same bits
    assert _fit_bits(rel.fit_scaling(sd, td, how=how, per_class=per_class, max_iter=96)) == _fit_bits(sc)
    assert _fit_bits(rel.fit_scaling(sd, td, how=how, per_class=per_class, max_iter=64)) == _fit_bits(sc)
    assert torch.equal(sd.cpu(), torch.from_numpy(s))


def test_fit_statuses_nan_scores_and_refusals():
    s, t, want = rc.degenerate_table()
    s[3, 0] = np.nan                                                 # a NaN score is left out of the fit
    sd, td = torch.from_numpy(s).to(DEV), torch.from_numpy(t).to(DEV)
    for how in ("temperature", "platt"):
        got = rel.fit_scaling(sd, td, how=how, per_class=True).cpu()
        status = got.status.tolist()
        assert status[0] == 0 and status[1] == 1 and status[2] in (0, 2), status       # the separable class: reported, not compared
        assert float(got.a[1]) == 1.0 and float(got.b[1]) == 0.0 and int(got.iterations[1]) == 0
        a, b = got.a.numpy(), got.b.numpy()
        f, g, H = rel.mean_nll_host(s[:, :1], t[:, :1], a[:1], b[:1], True)[0]
        assert np.abs(g[:1] if how == "temperature" else g).max() <= 1e-9
    short = rel.fit_scaling(sd, td, how="platt", per_class=True, max_iter=3).cpu()
    assert short.status.tolist() == [2, 1, 2] and short.iterations.tolist() == [3, 0, 3]
    ha, hb, _, _ = rel.fit_scaling_host(s, t, "platt", True, 3)     # the last accepted point of the same iteration
    assert np.allclose(short.a.numpy(), ha, rtol=1e-9) and np.allclose(short.b.numpy(), hb, rtol=1e-9, atol=1e-12)
    alone = rel.fit_scaling(sd[:, 1:2], td[:, 1:2], how="platt", per_class=False).cpu()            # every group degenerate
    assert alone.status.tolist() == [1] and alone.a.tolist() == [1.0] and alone.b.tolist() == [0.0]
    none = rel.fit_scaling(sd[:0], td[:0]).cpu()                     # no row: nothing launched, the identity
    assert none.status.tolist() == [1, 1, 1] and none.a.tolist() == [1.0] * 3
    with pytest.raises(ValueError, match="must both be"):
        rel.fit_scaling(sd, td[:, :2])


# ------------------------------------------------------------------------------------------------ apply
def _ulps(got, want32):
    return np.abs(got.astype(np.float64) - want32.astype(np.float64)) / np.spacing(np.abs(want32)).astype(np.float64)


def test_apply_equals_the_float64_definition():
    p, _ = rc.prob_table(700, 6, 15, seed=9)
    pd = torch.from_numpy(p).to(DEV)
    keep = pd.clone()
    rng = np.random.default_rng(2)
    a, b = rng.uniform(0.2, 3.0, 6), rng.uniform(-1.5, 1.5, 6)
    out = rel.Scaling(a, b).to(DEV).apply(pd)
    assert out.dtype == torch.float32 and out.shape == pd.shape and out.data_ptr() != pd.data_ptr()
    got = out.cpu().numpy()
    want = rel.apply_host(p, a, b)
    nan = np.isnan(p)
    assert nan.any() and np.array_equal(np.isnan(got), nan)
    assert _ulps(got[~nan], want[~nan].astype(np.float32)).max() <= 2.0
    ident = rel.Scaling(np.ones(6), np.zeros(6)).to(DEV).apply(pd).cpu().numpy()
    clamped = np.minimum(np.maximum(p, rel.P_LO), rel.P_HI)
    assert np.array_equal(np.isnan(ident), nan) and _ulps(ident[~nan], clamped[~nan]).max() <= 1.0
    assert torch.equal(pd.view(torch.int32), keep.view(torch.int32))                               # the input is never written
    with pytest.raises(ValueError, match="scores must be"):
        rel.Scaling(np.ones(5), np.zeros(5)).to(DEV).apply(pd)


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def solver():
    import test_gpu_calibrate as tc
    from mmda_amd import DeviceDataset, DeviceLoader
    lengths = np.random.default_rng(8).integers(1, 10, size=tc.N_SAMPLES)
    dataset = DeviceDataset.from_samples(tc.make_samples(lengths, *tc.MOSEI, seed=2), DEV)
    return tc._solver(tc.ListLoader([]), DeviceLoader(dataset, 8), tc.ListLoader([]), "fp32", name="reliability")


def _tables(s):
    rows = list(s._eval_batches(s.dev_data_loader, confidence=True))
    cat = lambda k: None if any(r[k] is None for r in rows) else torch.cat([r[k].detach() for r in rows], 0)
    return cat(0), cat(1), cat(2), cat(3)


def test_solver_reliability_equals_the_metrics_of_the_concatenated_tables(solver):
    s = solver
    scores, truth, labels, tcp = _tables(s)
    out = s.reliability("dev")
    assert out is s.last_reliability and set(out) == {"scores", "confidence"}
    want = rel.reliability_metrics(scores, truth)
    assert torch.equal(out["scores"].figures.view(torch.int64), want.figures.view(torch.int64))
    assert torch.equal(out["scores"].diagram.view(torch.int64), want.diagram.view(torch.int64))
    host_fig, _ = rel.reliability_host(scores.cpu().numpy(), truth.cpu().numpy())
    np.testing.assert_array_equal(out["scores"].cpu().figures.numpy()[:, :6], host_fig[:, :6])
    if tcp is not None and tcp.shape == labels.shape:
        correct = ((labels > 0) == (truth > 0)).to(torch.float32)
        conf = rel.reliability_metrics(tcp, correct)
        assert torch.equal(out["confidence"].figures.view(torch.int64), conf.figures.view(torch.int64))
    else:
        assert out["confidence"] is None
    assert s.reliability("dev", bins=4)["scores"].diagram.shape == (scores.shape[1], 4, 3)
    with pytest.raises(ValueError, match="mode must be"):
        s.reliability("train")


def test_solver_scaling_feeds_calibrate_and_eval(solver):
    s = solver
    before = s.eval("dev")
    scores, truth, _, _ = _tables(s)
    sc = s.fit_scaling("dev", how="platt", per_class=True, max_iter=64)
    assert sc is s.scaling and sc.a.is_cuda and sc.how == "platt" and sc.per_class is True
    direct = rel.fit_scaling(scores, truth, how="platt", per_class=True)
    assert _fit_bits(direct) == _fit_bits(sc)
    scaled = sc.apply(scores).cpu().numpy()
    thr = s.calibrate("dev", scaling=sc)
    from mmda_amd.calibrate import ThresholdSweep
    sweep = ThresholdSweep(scores.shape[1], None, DEV)
    sweep.update(torch.from_numpy(scaled).to(DEV), truth)
    want_thr = sweep.select(thr.objective, True)
    assert torch.equal(thr.k, want_thr.k) and torch.equal(thr.values, want_thr.values)
    _, _, y_pred, y_true = s.eval("dev", thresholds=thr, scaling=sc)
    assert np.array_equal(y_pred > 0, scaled > thr.cpu().values.numpy())
    assert np.array_equal(y_true, truth.cpu().numpy())
    # a scaling without cut-offs decides with config.threshold in every class
    _, _, y_pred, _ = s.eval("dev", scaling=sc)
    assert np.array_equal(y_pred > 0, scaled > np.float32(s.train_config.threshold))
    # reliability under the scaling is that of the scaled scores
    rs = s.reliability("dev", scaling=sc)["scores"]
    want = rel.reliability_metrics(torch.from_numpy(scaled).to(DEV), truth)
    assert torch.equal(rs.figures.view(torch.int64), want.figures.view(torch.int64))
    # and eval() without a scaling returns the bits it returned before
    after = s.eval("dev")
    assert after[0] == before[0] and after[1] == before[1] and np.array_equal(after[2], before[2]) and np.array_equal(after[3], before[3])
    again = s.eval("dev", scaling=None, thresholds=None)
    assert again[0] == before[0] and np.array_equal(again[2], before[2])


def test_train_with_scaling_saves_and_uses_it(tmp_path, monkeypatch):
    import test_gpu_calibrate as tc
    from mmda_amd import DeviceDataset, DeviceLoader, Scaling, Thresholds
    monkeypatch.chdir(tmp_path)
    lengths = np.random.default_rng(8).integers(1, 10, size=tc.N_SAMPLES)
    dataset = DeviceDataset.from_samples(tc.make_samples(lengths, *tc.MOSEI, seed=2), DEV)
    gen = torch.Generator().manual_seed(5)
    s = tc._solver(DeviceLoader(dataset, 8, shuffle=True, generator=gen), DeviceLoader(dataset, 8), DeviceLoader(dataset, 8), "fp32",
                   name="scal", scaling="temperature", calibrate="per_class")
    s.train()
    final = dict(s.last_eval_metrics)                                # of train()'s last act: the test pass, scaled and under the cut-offs
    loaded = Scaling.load(tmp_path / "checkpoints" / "scaling_scal.pt", DEV)
    assert _fit_bits(loaded) == _fit_bits(s.scaling) and loaded.how == "temperature" and loaded.per_class is False
    thr = Thresholds.load(tmp_path / "checkpoints" / "thresholds_scal.pt", DEV)
    s.eval("test", thresholds=thr, scaling=loaded)
    assert dict(s.last_eval_metrics) == final
    again = s.calibrate("dev", per_class=True, scaling=loaded)       # the saved cut-offs were chosen on the scaled scores
    assert torch.equal(again.k, thr.k)
