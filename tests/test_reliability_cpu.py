"""CPU: the numpy definitions of mmda_amd/reliability.py (the yardstick of tests/test_gpu_reliability.py) against sklearn, a direct
float64 restatement and scipy; the entry points' refusals without a GPU; the files, the flag, the rule and the argument paths.

Bounds: Brier score and NLL are float64 means of the same terms as sklearn's: 1e-12 relative.  ECE and the diagram carry every
p >= 2^-17 exactly in the 2^40 fixed point, so on inputs at least 1e-3 away from a bin edge (where float64 and fp32 binning agree) they
equal the textbook float64 expression to a few roundings: 1e-12.  The host fit stops at a mean-NLL gradient of 1e-12; with the smallest
Hessian eigenvalue of a case at least 1e-3 its parameters are within sqrt(2) 1e-12 / 1e-3 of the optimum, scipy's within its own 1e-7:
2e-6 bounds both, as in the GPU test."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

import reliability_cases as rc
from mmda_amd import _lib, step_rules
from mmda_amd import reliability as rel

EINVAL, OK = -1, 0


# ------------------------------------------------------------------------------------------------ the report
def _plain_table(N, C, M, seed):
    """probabilities in [0.01, 0.99] at least 1e-3 away from every edge k / M, both labels in every class"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.01, 0.99, (N, C))
    frac = p * M - np.floor(p * M)
    p = np.where((frac < 1e-3 * M) | (frac > 1 - 1e-3 * M), (np.floor(p * M) + 0.5) / M, p).astype(np.float32)
    y = rng.random((N, C)) < p
    y[0], y[1] = True, False
    return p, y.astype(np.float32)


@pytest.mark.parametrize("shape", [(50, 1, 15), (400, 6, 15), (333, 16, 64), (77, 3, 1)], ids=lambda s: "x".join(map(str, s)))
def test_brier_and_nll_equal_sklearn(shape):
    from sklearn.metrics import brier_score_loss, log_loss
    N, C, M = shape
    p, y = _plain_table(N, C, M, 3)
    fig, _ = rel.reliability_host(p, y, M)
    for c in range(C):
        want_b = brier_score_loss(y[:, c] > 0, p[:, c].astype(np.float64))
        want_l = log_loss(y[:, c] > 0, p[:, c].astype(np.float64), labels=[False, True])
        assert abs(fig[c, 6] - want_b) <= 1e-12 * want_b and abs(fig[c, 7] - want_l) <= 1e-12 * want_l
    assert fig[C + 1, 0] == N * C and abs(fig[C + 1, 6] - np.mean((p.astype(np.float64) - y) ** 2)) <= 1e-12
    assert abs(fig[C, 7] - fig[:C, 7].mean()) <= 1e-15 * C


@pytest.mark.parametrize("shape", [(50, 1, 15), (400, 6, 15), (333, 16, 64), (77, 3, 2)], ids=lambda s: "x".join(map(str, s)))
def test_ece_mce_and_diagram_equal_the_float64_restatement(shape):
    N, C, M = shape
    p, y = _plain_table(N, C, M, 5)
    fig, dia = rel.reliability_host(p, y, M)
    pd, yd = p.astype(np.float64), y.astype(np.float64)
    for c in range(C):
        j = np.minimum(M - 1, np.floor(pd[:, c] * M).astype(int))
        ece, mce = 0.0, 0.0
        for b in range(M):
            sel = j == b
            assert dia[c, b, 0] == sel.sum()
            if not sel.any():
                assert np.isnan(dia[c, b, 1]) and np.isnan(dia[c, b, 2])
                continue
            acc, conf = yd[sel, c].mean(), pd[sel, c].mean()
            assert abs(dia[c, b, 1] - acc) <= 1e-12 and abs(dia[c, b, 2] - conf) <= 1e-12
            ece += abs(acc - conf) * sel.sum() / N
            mce = max(mce, abs(acc - conf))
        assert abs(fig[c, 4] - ece) <= 1e-12 and abs(fig[c, 5] - mce) <= 1e-12
        assert abs(fig[c, 2] - yd[:, c].mean()) <= 1e-15 and abs(fig[c, 3] - pd[:, c].mean()) <= 1e-12


def test_cleaning_binning_and_the_empty_state():
    M = 15
    p = np.array([[np.nan], [-0.25], [1.5], [-0.0], [1.0], [0.0], [2.0 ** -41]], dtype=np.float32)
    y = np.array([[1], [1], [1], [0], [0], [1], [0]], dtype=np.float32)
    st = rel.state_host(p, y, M)
    assert st["n_nan"].tolist() == [1] and int(st["cnt"].sum()) == 6
    assert st["cnt"][0, 0] == 4 and st["cnt"][0, M - 1] == 2 and st["pos"][0, 0] == 2 and st["pos"][0, M - 1] == 1
    assert int(st["sum_p"][0, M - 1]) == 2 * rel.FIX and int(st["sum_p"][0, 0]) == 0          # 2^-41 2^40 = 0.5 rounds to even
    # log p = -inf is clamped to -100: (p = 0, y = 1) twice, (p = 1, y = 0) once; (p = 1, y = 1), (p = 0, y = 0) and 2^-41 add (almost) nothing
    assert abs(st["sum_nll"][0] - 300.0) <= 1e-9
    e = rc.edge_values(M)
    j = rel.bin_index(rel.clean(e)[0], M)
    assert j.min() == 0 and j.max() == M - 1
    for m in rc.COLLECTOR_M:
        # the product of two floats is exact in a double: rounding it once to fp32 is the single fp32 multiply the definition names
        v = rel.clean(rc.edge_values(m))[0]
        once = (v.astype(np.float64) * float(m)).astype(np.float32)
        assert np.array_equal(rel.bin_index(v, m), np.minimum(m - 1, np.floor(once).astype(np.int32)))
    fig, dia = rel.reliability_host(np.full((3, 2), np.nan, np.float32), np.ones((3, 2), np.float32), 4)
    assert fig[:, 0].tolist() == [0, 0, 0, 0] and fig[:2, 1].tolist() == [3, 3] and fig[3, 1] == 6 and np.isnan(fig[:, 2:]).all()
    assert (dia[..., 0] == 0).all() and np.isnan(dia[..., 1:]).all()


def test_ordered_sum_is_a_sum_and_chains_over_batches():
    rng = np.random.default_rng(0)
    for N in (1, 15, 16, 17, 511, 512, 513, 1500):
        ints = rng.integers(0, 1000, (N, 3)).astype(np.float64)          # exact in any order
        assert np.array_equal(rel.ordered_sum(ints), ints.sum(0))
        t = rng.random((N, 3))
        got = rel.ordered_sum(t[N // 2:], rel.ordered_sum(t[:N // 2]))
        assert np.allclose(got, t.sum(0), rtol=N * 2.0 ** -52, atol=0)


def test_unpack_state_reads_the_layout_of_the_header():
    C, M = 3, 4
    w = np.zeros(rel.state_words(C, M), dtype=np.int64)
    w[0], w[2 + 1] = 9, 5
    w[2 + C:2 + 3 * C] = np.arange(1.0, 7.0).view(np.int64)
    w[2 + 3 * C + 3 * (2 * M + 3) + 1] = 11
    st, ticket = rel.unpack_state(w, C, M)
    assert ticket == 9 and st["n_nan"].tolist() == [0, 5, 0] and st["pos"][2, 3] == 11 and int(st["pos"].sum()) == 11
    assert st["sum_sq"].tolist() == [1.0, 2.0, 3.0] and st["sum_nll"].tolist() == [4.0, 5.0, 6.0]
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mmda_hip.h")).read()
    assert "#define MMDA_RELIAB_STATE_WORDS(C, M) (2 + 3 * (C) + 3 * (C) * (M))" in src


# ------------------------------------------------------------------------------------------------ the fit
@pytest.mark.parametrize("case", rc.fit_cases(), ids=lambda c: f"{c[0]}x{c[1]}-{c[3]}-{'per_class' if c[4] else 'shared'}-a{c[2][0]}")
def test_host_fit_reaches_the_scipy_optimum(case):
    N, C, true, how, per_class, seed = case
    s, t = rc.fit_table(N, C, true, how, per_class, seed)
    a, b, status, iters = rel.fit_scaling_host(s, t, how, per_class, 64)
    assert (status == 0).all() and (iters >= 1).all() and (iters <= 32).all()
    if how == "temperature":
        assert (b == 0).all()
    if not per_class:
        assert (a == a[0]).all() and (b == b[0]).all()
    for f, g, H in rel.mean_nll_host(s, t, a, b, per_class):
        assert np.abs(g[:1] if how == "temperature" else g).max() <= 1e-9
    sa, sb = rc.scipy_fit(s, t, how, per_class)
    assert np.abs(a - sa).max() <= 2e-6 and np.abs(b - sb).max() <= 2e-6
    at_id = rel.mean_nll_host(s, t, np.ones(C), np.zeros(C), per_class)
    for (f, _, _), (f0, _, _) in zip(rel.mean_nll_host(s, t, a, b, per_class), at_id):
        assert f <= f0
    # a frozen group keeps its bits: more launches change nothing
    a2, b2, _, it2 = rel.fit_scaling_host(s, t, how, per_class, 96)
    assert np.array_equal(a, a2) and np.array_equal(b, b2) and np.array_equal(iters, it2)


def test_host_fit_statuses_of_the_degenerate_table():
    s, t, want = rc.degenerate_table()
    for how in ("temperature", "platt"):
        a, b, status, iters = rel.fit_scaling_host(s, t, how, True, 64)
        assert status[0] == 0 and status[1] == 1 and a[1] == 1.0 and b[1] == 0.0 and iters[1] == 0
        assert status[2] in (0, 2) and a[2] > 20.0                 # separable: drifts; reported, not compared
    a, b, status, iters = rel.fit_scaling_host(s, t, "platt", True, 3)
    assert status.tolist() == [2, 1, 2] and iters.tolist() == [3, 0, 3]


def test_apply_host_identity_and_nan():
    p = np.array([[0.25, np.nan, 0.0, 1.0, 0.9]], dtype=np.float32)
    q = rel.apply_host(p, np.ones(5), np.zeros(5))
    assert np.isnan(q[0, 1]) and abs(q[0, 0] - 0.25) <= 1e-15 and q[0, 2] == pytest.approx(2.0 ** -23, rel=1e-12)
    assert q[0, 3] == pytest.approx(1 - 2.0 ** -23, rel=1e-12)
    z = rel.logit_host(p)
    assert np.nanmax(np.abs(z)) <= 15.95 and np.isnan(z[0, 1])


# ------------------------------------------------------------------------------------------------ refusals without a GPU
def _caller(fn, names, **good):
    """fn called with ``good`` by name, a keyword replacing one argument"""
    return lambda **k: fn(*[dict(good, **k)[x] for x in names])


def test_entry_points_refuse_before_any_launch():
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    good = ctypes.addressof(buf)                                     # 8-byte aligned host memory: never read, every call below is refused
    assert good % 8 == 0
    acc = _caller(lib.mmda_reliab_accumulate, ("prob", "target", "N", "C", "M", "state", "stream"),
                  prob=good, target=good, N=4, C=6, M=15, state=good, stream=None)
    for bad in (dict(prob=None), dict(target=None), dict(state=None), dict(prob=good + 2), dict(target=good + 1), dict(state=good + 4),
                dict(C=0), dict(C=17), dict(M=0), dict(M=65), dict(N=-1), dict(N=(1 << 20) + 1)):
        assert acc(**bad) == EINVAL, bad
    assert acc(N=0) == OK                                            # nothing to add: no launch
    fin = _caller(lib.mmda_reliab_finish, ("state", "C", "M", "figures", "diagram", "stream"),
                  state=good, C=6, M=15, figures=good, diagram=good, stream=None)
    for bad in (dict(state=None), dict(figures=None), dict(diagram=None), dict(state=good + 4), dict(figures=good + 4),
                dict(diagram=good + 4), dict(C=0), dict(C=17), dict(M=0), dict(M=65)):
        assert fin(**bad) == EINVAL, bad
    need = lib.mmda_scaling_work_bytes(4, 6)
    assert need == 8 * (256 + 32 * 16 * 6 + 4 * 6) and lib.mmda_scaling_work_bytes(4, 17) == -1
    assert lib.mmda_scaling_work_bytes((1 << 20) + 1, 6) == -1 and lib.mmda_scaling_work_bytes(-1, 6) == -1
    fit = _caller(lib.mmda_scaling_fit, ("prob", "target", "N", "C", "how", "per_class", "max_iter", "work", "work_bytes", "a", "b", "status",
                                         "iterations", "stream"),
                  prob=good, target=good, N=4, C=6, how=0, per_class=1, max_iter=64, work=good, work_bytes=need, a=good, b=good,
                  status=good, iterations=good, stream=None)
    for bad in (dict(prob=None), dict(target=None), dict(work=None), dict(a=None), dict(b=None), dict(status=None), dict(iterations=None),
                dict(prob=good + 2), dict(work=good + 4), dict(a=good + 4), dict(b=good + 4), dict(status=good + 2), dict(iterations=good + 1),
                dict(C=0), dict(C=17), dict(N=-1), dict(N=(1 << 20) + 1), dict(max_iter=0), dict(max_iter=257), dict(max_iter=-1),
                dict(how=2), dict(how=-1), dict(work_bytes=need - 8)):
        assert fit(**bad) == EINVAL, bad
    assert fit(N=0, work_bytes=lib.mmda_scaling_work_bytes(0, 6)) == OK
    app = _caller(lib.mmda_scaling_apply, ("prob", "a", "b", "N", "C", "out", "stream"), prob=good, a=good, b=good, N=4, C=6, out=good,
                  stream=None)
    for bad in (dict(prob=None), dict(a=None), dict(b=None), dict(out=None), dict(prob=good + 2), dict(a=good + 4), dict(b=good + 4),
                dict(out=good + 1), dict(C=0), dict(C=17), dict(N=-1), dict(N=(1 << 20) + 1)):
        assert app(**bad) == EINVAL, bad
    assert app(N=0) == OK


def test_python_surface_refuses_host_tensors_and_bad_arguments():
    p, t = torch.rand(4, 6), torch.ones(4, 6)
    with pytest.raises(_lib.MMDAError, match="no CPU fallback"):
        rel.ReliabilityEval(6, device="cpu")
    with pytest.raises(_lib.MMDAError, match="no CPU fallback"):
        rel.reliability_metrics(p, t)
    with pytest.raises(_lib.MMDAError, match="no CPU fallback"):
        rel.fit_scaling(p, t)
    with pytest.raises(_lib.MMDAError, match="no CPU fallback"):
        rel.Scaling(np.ones(6), np.zeros(6)).apply(p)
    with pytest.raises(ValueError, match="how must be"):
        rel.fit_scaling(p, t, how="isotonic")
    for bad in (0, 257, True):
        with pytest.raises(ValueError, match="max_iter"):
            rel.fit_scaling(p, t, max_iter=bad)
    with pytest.raises(ValueError, match="classes"):
        rel.ReliabilityEval(17)
    with pytest.raises(ValueError, match="bins"):
        rel.ReliabilityEval(6, bins=65)
    with pytest.raises(ValueError, match="one entry per class"):
        rel.Scaling(np.ones(6), np.zeros(5))


# ------------------------------------------------------------------------------------------------ files, flag, rule, argument paths
def test_scaling_round_trips_through_its_file_and_the_tools(tmp_path, monkeypatch):
    from mmda_amd import Scaling
    from mmda_amd.utils import tools
    sc = Scaling(np.array([0.5, 1.25, 3.0]), np.array([0.1, -0.2, 0.0]), [0, 1, 2], [7, 0, 64], "platt", True)
    sc.save(tmp_path / "s.pt")
    got = Scaling.load(tmp_path / "s.pt")
    for k in ("a", "b", "status", "iterations"):
        assert torch.equal(getattr(got, k), getattr(sc, k)) and getattr(got, k).dtype == getattr(sc, k).dtype
    assert got.how == "platt" and got.per_class is True and len(got) == 3 and got.a.dtype == torch.float64
    assert torch.equal(sc.cpu().a, sc.a) and torch.equal(sc.to("cpu").status, sc.status)
    monkeypatch.chdir(tmp_path)

    class Args:
        use_confidNet = True
    tools.save_scaling(Args, sc, "mosei")
    assert (tmp_path / "scaling" / "MISA_C_mosei.pt").exists()
    back = tools.load_scaling(Args, "mosei")
    assert torch.equal(back.a, sc.a) and torch.equal(back.b, sc.b) and back.how == "platt"


def test_scaling_flag_parses(monkeypatch):
    from mmda_amd import get_config, make_config
    assert make_config(vocab_size=8).scaling == "none"
    for how in ("none", "temperature", "platt"):
        monkeypatch.setattr(sys, "argv", ["x", "--scaling", how])
        assert get_config(vocab_size=8).scaling == how
    monkeypatch.setattr(sys, "argv", ["x"])
    assert get_config(vocab_size=8).scaling == "none"
    monkeypatch.setattr(sys, "argv", ["x", "--scaling", "isotonic"])
    with pytest.raises(SystemExit):
        get_config(vocab_size=8)


def test_sentiment_refusal_names_the_rule():
    assert [n for n, _ in step_rules.SCALING_RULES] == ["senti_scaling"]
    for kw in (dict(scaling="temperature"), dict(scaling="platt"), dict(reliability=True)):
        hit = step_rules.scaling_verdict("sentiment", **kw)
        assert hit is not None and hit[0] == "senti_scaling"
        with pytest.raises(_lib.MMDAError) as e:
            step_rules.scaling_check("sentiment", **kw)
        assert str(e.value) == dict(step_rules.SCALING_RULES)["senti_scaling"].format(**hit[1]) and "sentiment" in str(e.value)
    assert step_rules.scaling_verdict("sentiment") is None and step_rules.scaling_verdict("sentiment", scaling=None) is None
    assert step_rules.scaling_verdict("emotion", scaling="platt", reliability=True) is None
    # Solver.build refuses the configuration before a model exists
    from mmda_amd import make_config
    from mmda_amd.solver import Solver
    c = make_config(vocab_size=8, task="sentiment", num_classes=1, scaling="platt", device="cpu")
    with pytest.raises(_lib.MMDAError, match="logit scaling"):
        Solver(c, c, c, [], [], [], is_train=False).build()
    c = make_config(vocab_size=8, scaling="isotonic", device="cpu")
    with pytest.raises(ValueError, match="config.scaling"):
        Solver(c, c, c, [], [], [], is_train=False).build()


def test_defaults_leave_the_eval_and_calibrate_argument_paths_unchanged():
    from mmda_amd.solver import Solver
    for fn in (Solver.eval, Solver.calibrate, Solver._eval_batches, Solver._eval_emotion, Solver.reliability,
               Solver._calibrate_after_training):
        assert inspect.signature(fn).parameters["scaling"].default is None
    names = list(inspect.signature(Solver.eval).parameters)
    assert names[:5] == ["self", "mode", "to_print", "thresholds", "keep"]          # positional callers of today keep their meaning
    assert list(inspect.signature(Solver.calibrate).parameters)[:5] == ["self", "mode", "grid", "objective", "per_class"]

    calls = []

    class Probe(Solver):
        def __init__(self):
            pass

        def _sentiment(self):
            return False

        def _eval_batches(self, dataloader, confidence=False, keep=None, scaling=None):
            calls.append((keep, scaling))
            return iter(())

    s = Probe()
    s.dev_data_loader = s.test_data_loader = []
    s.device = torch.device("cpu")
    s.train_config = type("C", (), {"num_classes": 2, "threshold": 0.5, "name": "no_such_run"})()
    s._check_cluster = lambda where: None
    thr, sc = type("T", (), {"values": torch.tensor([0.25, 0.75])})(), object()
    # what a caller observes of "the defaults change nothing": every form walks its split exactly once, and exactly the scaling it was
    # given reaches the walk
    for args, kw, want in ((("dev",), {}, None), (("dev",), dict(thresholds=thr), None), (("dev",), dict(scaling=sc), sc),
                           (("test", True, thr, None, sc), {}, sc)):
        out = s.eval(*args, **kw)
        assert calls == [(None, want)], (args, kw)
        calls.clear()
        assert out[0] == 0.0 and out[2].shape == (0,)
