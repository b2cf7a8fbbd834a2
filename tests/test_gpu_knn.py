"""GPU: ``mmda_knn_sets`` (csrc/knn.hip) through ``knn_search`` over the case table of tests/knn_cases.py.

Integer cases: every distance and every partial sum is an integer below 2^24, so dist and index must equal the int64 reference bit for
bit, ties, duplicates and ``exclude_self`` included.  Real-valued cases, by value: every reported distance within the worst-case bound
of a direct-form fp32 sum, 2 (D + 2) 2^-24 d64, of the float64 distance of THAT pair (the dot form misses it by orders of magnitude on
the clustered case); the float64 distance of the j-th returned pair within 4 gamma (|q|^2 + max |b|^2) of the j-th smallest float64
distance of its (query, set) -- twice the worst-case error of the dot form, all a selection by it can move; every list sorted by
(dist, index); padding and the NaN row as defined.  The largest measured errors are printed per case (DESIGN.md 4t records them).
Determinism: a call over Q rows equals Q calls over one row, and two runs agree, bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import knn_cases as kc

DEV = "cuda:0"
INT_CASES = [c.name for c in kc.CASES if c.kind == "int"]
REAL_CASES = [c.name for c in kc.CASES if c.kind != "int"]


def _search(name, rows=None):
    from mmda_amd import knn_search
    case = kc.BY_NAME[name]
    query, base, member = kc.tables(name)
    q = torch.tensor(query).to(DEV)
    b = q if case.q == "self" else torch.tensor(base).to(DEV)
    m = torch.tensor(member).to(DEV)
    if rows is not None:
        q = q[rows].contiguous()
    return knn_search(q, b, case.k, member=m, sets=case.S, exclude_self=case.exclude_self)


@pytest.mark.parametrize("name", INT_CASES)
def test_integer_cases_are_the_reference_bit_for_bit(name):
    _, ref_d, ref_i, _ = kc.reference(name)
    dist, index = _search(name)
    assert dist.dtype == torch.float32 and index.dtype == torch.int32 and tuple(dist.shape) == ref_d.shape
    assert torch.equal(index.cpu(), torch.from_numpy(ref_i.copy())), name
    assert torch.equal(dist.cpu(), torch.from_numpy(ref_d.astype(np.float32))), name


@pytest.mark.parametrize("name", REAL_CASES)
def test_real_cases_by_value(name):
    case = kc.BY_NAME[name]
    query, base, member = kc.tables(name)
    d, ref_d, ref_i, eligible = kc.reference(name)
    dist, index = _search(name)
    dist, index = dist.cpu().numpy(), index.cpu().numpy()
    Q, S, k = index.shape
    valid = index >= 0
    # padding: exactly the entries past the eligible rows, +inf / -1, at the tail
    want_valid = np.arange(k)[None, None, :] < np.minimum(eligible, k)[:, :, None]
    assert np.array_equal(valid, want_valid)
    assert np.all(np.isinf(dist[~valid])) and np.all(dist[~valid] > 0) and np.all(np.isfinite(dist[valid]))
    if case.nan_row:
        bad = np.flatnonzero(np.isnan(base).any(axis=1))
        assert bad.size == 1 and not np.isin(index, bad).any()
    # members only, no row twice, and never the row itself under exclude_self
    qi, si, _ = np.nonzero(valid)
    got = index[valid]
    assert np.all((member[got] >> si) & 1)
    for i in range(Q):
        for s in range(S):
            row = index[i, s][valid[i, s]]
            assert np.unique(row).size == row.size
    if case.exclude_self:
        assert not np.any(got == qi)
    # sorted by (dist, index)
    a_d, b_d, a_i, b_i = dist[:, :, :-1], dist[:, :, 1:], index[:, :, :-1], index[:, :, 1:]
    both = valid[:, :, 1:]
    assert np.all((a_d[both] < b_d[both]) | ((a_d[both] == b_d[both]) & (a_i[both] < b_i[both])))
    # reported distances against the float64 distance of the same pair
    d64 = d[qi, got]
    err = np.abs(dist[valid].astype(np.float64) - d64)
    bound = kc.reported_bound(case.D, d64)
    # selected neighbours against the j-th smallest float64 distance of the (query, set)
    qn = (query.astype(np.float64) ** 2).sum(axis=1)
    bn = (base.astype(np.float64) ** 2).sum(axis=1)
    sel_bound = kc.selection_bound(case.D, qn, np.nanmax(bn))[qi]
    sel_err = np.abs(d64 - ref_d[valid])
    rel = err / np.maximum(d64, 1e-300)
    print(f"{name}: reported error max {err.max() if err.size else 0.0:.3e} (relative {rel.max() if rel.size else 0.0:.3e}, bound "
          f"{2 * (case.D + 2) * kc.U:.3e} relative); selection error max {sel_err.max() if sel_err.size else 0.0:.3e} "
          f"(bound {sel_bound.min() if sel_bound.size else 0.0:.3e}); distances {d64.min() if d64.size else 0.0:.4g} .. "
          f"{d64.max() if d64.size else 0.0:.4g}")
    assert np.all(err <= bound), (name, float(err.max()))
    assert np.all(sel_err <= sel_bound), (name, float(sel_err.max()))


@pytest.mark.parametrize("name", ["normal_d768_nan", "clustered_d768", "scaled_d770_narrow_tile"])
def test_one_call_is_q_calls_and_two_runs_agree(name):
    """(cases without exclude_self: row i of a one-row call is query row 0)"""
    dist, index = _search(name)
    again_d, again_i = _search(name)
    assert torch.equal(dist.view(torch.int32), again_d.view(torch.int32)) and torch.equal(index, again_i)
    for i in range(int(dist.shape[0])):
        d1, i1 = _search(name, rows=slice(i, i + 1))
        assert torch.equal(d1[0].view(torch.int32), dist[i].view(torch.int32)), (name, i)
        assert torch.equal(i1[0], index[i]), (name, i)


def test_member_none_is_one_set_of_every_row():
    from mmda_amd import NeighbourIndex, knn_search
    query, base, _ = kc.tables("normal_d42_k1")
    q, b = torch.tensor(query).to(DEV), torch.tensor(base).to(DEV)
    dist, index = knn_search(q, b, 5)
    d = kc.pair_distances(query, base)
    _, ref_i, _ = kc.ref_knn(d, np.ones(base.shape[0], dtype=np.int32), 1, 5)
    assert torch.equal(index.cpu(), torch.from_numpy(ref_i))
    d2, i2 = NeighbourIndex(b).search(q, 5)
    assert torch.equal(d2, dist[:, 0]) and torch.equal(i2, index[:, 0])
    # a table searched against itself reports exactly 0 for every row, and the row itself first
    self_d, self_i = knn_search(b, b, 1)
    assert torch.equal(self_d.flatten(), torch.zeros(b.shape[0], device=DEV))
    assert torch.equal(self_i.flatten().cpu(), torch.arange(b.shape[0], dtype=torch.int32))


def test_a_work_buffer_that_is_too_small_is_refused():
    from mmda_amd import _lib, ops
    q = torch.zeros(4, 8, device=DEV)
    m = torch.ones(4, dtype=torch.int32, device=DEV)
    small = torch.empty(ops.knn_plan(4, 4, 8, 1, 1)["work_bytes"] - 16, dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.MMDAError, match="mmda_knn_sets"):
        ops.knn_sets(q, q, m, 1, 1, work=small)
