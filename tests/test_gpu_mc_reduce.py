"""GPU: ``mmda_mc_reduce`` alone -- K draws per (sample, column) reduced to float64 tables in one launch -- against the numpy float64
restatement of tests/uncertainty_cases.py (checked by hand in tests/test_uncertainty_cpu.py).

Bound: 1e-12 absolute on every float64 figure, the bound the project's other float64 collectors hold against their numpy definitions:
a sum of at most 256 terms of magnitude at most 1 in float64 (error below 256 x 2^-53 = 3e-14 whatever the order) and a few-ulp ``log``
stay orders of magnitude below it.  ``vote`` and ``draws`` are exact."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import uncertainty_cases as uc

DEV = "cuda:0"
EINVAL = -1                                                   # MMDA_EINVAL (include/mmda_hip.h)
TOL = 1e-12
SENTINEL = -7.25
F64 = ("mean", "var", "entropy", "expected_entropy", "mutual_info", "vote")


def _reduce(p, K, thr, bernoulli=True, dst=None, rows=None, draws=True, base=0):
    """One ``mmda_mc_reduce`` launch into tables of ``rows`` rows filled with SENTINEL; returns them on the host."""
    from mmda_amd import _lib
    lib = _lib.load()
    B, W = p.shape[0] // K, p.shape[1]
    rows = B if rows is None else rows
    pd = torch.from_numpy(p).to(DEV)
    names = [k for k in F64 if (k != "vote" or thr is not None) and (bernoulli or k in ("mean", "var", "vote"))]
    tabs = {k: torch.full((rows, W), SENTINEL, dtype=torch.float64, device=DEV) for k in names}
    dr = torch.full((rows, K, W), SENTINEL, dtype=torch.float32, device=DEV) if draws else None
    out = _lib.McOut(**{k: t.data_ptr() for k, t in tabs.items()}, draws=_lib.ptr(dr))
    td = None if thr is None else torch.from_numpy(thr).to(DEV)
    dd = None if dst is None else torch.from_numpy(np.asarray(dst, dtype=np.int32)).to(DEV)
    rc = lib.mmda_mc_reduce(pd.data_ptr(), B, K, W, _lib.ptr(td), int(bernoulli), C.byref(out), _lib.ptr(dd), base, _lib.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = {k: t.cpu().numpy() for k, t in tabs.items()}
    if draws:
        got["draws"] = dr.cpu().numpy()
    return got


def _bits(x):
    return np.ascontiguousarray(x).view(np.int64 if x.dtype == np.float64 else np.int32)


def _check(got, ref, rows_of):
    """``got`` rows ``rows_of`` against ``ref`` rows 0 .. B-1: the float64 figures within TOL with NaN exactly where the reference has
    one, the vote and the draws exact."""
    worst = 0.0
    for k in got:
        g, r = got[k][rows_of], ref[k]
        if k in ("vote", "draws"):
            assert np.array_equal(_bits(g), _bits(r.astype(g.dtype))), k
            continue
        assert np.array_equal(np.isnan(g), np.isnan(r)), k
        ok = ~np.isnan(r)
        if ok.any():
            e = float(np.abs(g[ok] - r[ok]).max())
            worst = max(worst, e)
            assert e <= TOL, (k, e)
    return worst


@pytest.mark.parametrize("shape", uc.REDUCE_SHAPES, ids=[f"B{b}-K{k}-W{w}" for b, k, w in uc.REDUCE_SHAPES])
def test_reduce_against_the_numpy_restatement(shape):
    B, K, W = shape
    p, thr = uc.reduce_input(B, K, W)
    ref = uc.mc_reference(p, K, thr)
    if shape == (33, 8, 6):
        # rows through a permutation into a 40-row table: the seven rows nobody is sent to keep the sentinel, in every table
        dst = np.random.default_rng(3).permutation(40)[:B].astype(np.int32)
        got = _reduce(p, K, thr, dst=dst, rows=40)
        rest = np.setdiff1d(np.arange(40), dst)
        assert rest.size == 7
        for k, t in got.items():
            assert (t[rest] == SENTINEL).all(), k
        rows_of = dst
    else:
        got = _reduce(p, K, thr)
        rows_of = np.arange(B)
    assert set(got) == set(F64) | {"draws"}
    worst = _check(got, ref, rows_of)
    print(f"{shape}: worst float64 error {worst:.2e} (bound {TOL:.0e})")
    if K == 1:
        v = got["var"][rows_of]
        assert (v[~np.isnan(v)] == 0.0).all()                # exactly 0: the mean of one draw is the draw
        m = got["mutual_info"][rows_of]
        assert (m[~np.isnan(m)] == 0.0).all()
    assert (got["mutual_info"][rows_of][~np.isnan(ref["mutual_info"])] >= 0.0).all()
    # two runs: identical bits
    again = _reduce(p, K, thr, dst=rows_of if shape == (33, 8, 6) else None, rows=got["mean"].shape[0])
    for k in got:
        assert np.array_equal(_bits(got[k]), _bits(again[k])), k


def test_without_thresholds_and_without_bernoulli():
    B, K, W = 5, 3, 6
    p, thr = uc.reduce_input(B, K, W)
    got = _reduce(p, K, None, draws=False)
    assert set(got) == {"mean", "var", "entropy", "expected_entropy", "mutual_info"}
    _check(got, uc.mc_reference(p, K, None), np.arange(B))
    got = _reduce(p, K, thr, bernoulli=False, base=2, rows=B + 3)          # the tcp form, rows base + b
    assert set(got) == {"mean", "var", "vote", "draws"}
    ref = uc.mc_reference(p, K, thr, bernoulli=False)
    _check(got, ref, np.arange(2, 2 + B))
    for k, t in got.items():
        assert (t[:2] == SENTINEL).all() and (t[2 + B:] == SENTINEL).all(), k


@pytest.mark.parametrize("K", [3, 65, 256])
def test_a_samples_bits_depend_on_neither_B_nor_dst(K):
    """The same sample reduced in two launches of different B, at different columns and through different ``dst``: identical bits."""
    W, B = 6, 9
    p, thr = uc.reduce_input(B, K, W, seed=77 + K)
    full = _reduce(p, K, thr)
    pick = [7, 2, 4]                                          # three of its samples, in another order, as a launch of their own
    sub = np.concatenate([p[b * K:(b + 1) * K] for b in pick])
    dst = np.array([5, 0, 3], dtype=np.int32)
    part = _reduce(sub, K, thr, dst=dst, rows=6)
    for k in full:
        for b, r in zip(pick, dst):
            assert np.array_equal(_bits(full[k][b]), _bits(part[k][r])), (k, b)
    one = _reduce(p[4 * K:5 * K], K, thr)                     # B = 1
    for k in full:
        assert np.array_equal(_bits(full[k][4]), _bits(one[k][0])), k


def test_einval_cases_launch_nothing():
    from mmda_amd import _lib
    lib = _lib.load()
    B, K, W = 2, 4, 6
    p = torch.rand(B * K, W, device=DEV)
    thr = torch.full((W,), 0.35, device=DEV)
    tabs = {k: torch.full((B, W), SENTINEL, dtype=torch.float64, device=DEV) for k in F64}
    dr = torch.full((B, K, W), SENTINEL, dtype=torch.float32, device=DEV)
    full = _lib.McOut(**{k: t.data_ptr() for k, t in tabs.items()}, draws=dr.data_ptr())
    s = _lib.stream_ptr()
    call = lambda p_, B_, K_, W_, thr_, bern, out: lib.mmda_mc_reduce(p_, B_, K_, W_, thr_, bern, out, None, 0, s)
    pp, tp = p.data_ptr(), thr.data_ptr()
    assert call(None, B, K, W, tp, 1, C.byref(full)) == EINVAL                       # p NULL
    assert call(pp, B, K, W, tp, 1, None) == EINVAL                                  # out NULL
    assert call(pp, B, K, W, tp, 1, C.byref(_lib.McOut())) == EINVAL                 # every table NULL
    assert call(pp, B, K, W, None, 1, C.byref(_lib.McOut(vote=tabs["vote"].data_ptr()))) == EINVAL      # a vote without thresholds
    for b_, k_, w_ in ((0, K, W), (-1, K, W), (B, 0, W), (B, 257, W), (B, K, 0), (B, K, 65)):
        assert call(pp, b_, k_, w_, tp, 1, C.byref(full)) == EINVAL, (b_, k_, w_)
    for k in ("entropy", "expected_entropy", "mutual_info"):                         # an entropy table without bernoulli
        assert call(pp, B, K, W, tp, 0, C.byref(_lib.McOut(mean=tabs["mean"].data_ptr(), **{k: tabs[k].data_ptr()}))) == EINVAL, k
    torch.cuda.synchronize()
    for k, t in tabs.items():
        assert bool((t == SENTINEL).all()), k
    assert bool((dr == SENTINEL).all())
    # and the edges of the ranges are accepted: K = 256, W = 64
    p2 = torch.rand(256, 64, device=DEV)
    m = torch.empty(1, 64, dtype=torch.float64, device=DEV)
    assert lib.mmda_mc_reduce(p2.data_ptr(), 1, 256, 64, None, 0, C.byref(_lib.McOut(mean=m.data_ptr())), None, 0, s) == 0
    ref = p2.cpu().numpy().astype(np.float64).sum(0) / 256
    assert float(np.abs(m.cpu().numpy()[0] - ref).max()) <= TOL


def test_mc_statistics_is_the_same_launch():
    from mmda_amd import mc_statistics
    B, K, W = 5, 3, 6
    p, thr = uc.reduce_input(B, K, W)
    want = _reduce(p, K, thr)
    got = mc_statistics(torch.from_numpy(p).to(DEV), K, thresholds=torch.from_numpy(thr), keep_draws=True)
    assert set(got) == set(want) and all(v.is_cuda for v in got.values())
    for k in want:
        assert np.array_equal(_bits(want[k]), _bits(got[k].cpu().numpy())), k
    plain = mc_statistics(torch.from_numpy(p).to(DEV), K, bernoulli=False)
    assert set(plain) == {"mean", "var"} and np.array_equal(_bits(plain["mean"].cpu().numpy()), _bits(want["mean"]))
    with pytest.raises(ValueError, match="must be"):
        mc_statistics(torch.from_numpy(p).to(DEV), 4)
