"""CPU: what the nearest-neighbour GPU tests stand on (tests/knn_cases.py), and everything of the feature that needs no GPU.

The case table: every integer case really stays below 2^24 and really has ties; every real-valued case, selected by an fp32 torch
restatement of the dot form on the host, stays inside the by-value selection bound the GPU test asserts.  ``ops.knn_plan`` over the case
table: the one-slab and the merged form, every tile and slab edge, LDS within 160 KB, work bytes that only grow.  The Trust Score
definition on a hand-worked one-dimensional example, the density filter against its stated rule, the refusals by name, the
null-argument MMDA_EINVALs, and the size of ``mmda_knn_plan`` against the C compiler."""
import ctypes
import os
import subprocess
import textwrap

import numpy as np
import pytest
import torch

import knn_cases as kc
from mmda_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_CASES = [c for c in kc.CASES if c.kind == "int"]
REAL_CASES = [c for c in kc.CASES if c.kind != "int"]


# ---------------------------------------------------------------------------------------------- the case table
def test_the_table_reaches_every_shape_named():
    assert {c.q for c in kc.CASES} >= {"1", "tile-1", "tile", "tile+1", "self"}
    assert {c.n for c in kc.CASES} == {"1", "k-1", "slab-1", "slab", "slab+1", "2slab+3"}
    assert {c.D for c in kc.CASES} == {6, 42, 768, 770}
    assert {c.k for c in kc.CASES} == {1, 10, 16} and {c.S for c in kc.CASES} == {1, 12, 16}
    assert {c.kind for c in kc.CASES} == {"int"} | set(kc.KINDS_REAL)
    assert any(c.nan_row for c in REAL_CASES) and any(c.exclude_self for c in INT_CASES)
    assert {c.D for c in INT_CASES} == {6, 42, 768, 770} and {c.D for c in REAL_CASES} == {6, 42, 768, 770}
    assert max(kc.shape(c)[0] * kc.shape(c)[1] for c in kc.CASES) < 100_000 and max(kc.shape(c)[1] for c in kc.CASES) < 4096
    for c in kc.CASES:
        _, _, member = kc.tables(c.name)
        if c.S > 1 and member.size > 20:
            counts = [int(((member >> s) & 1).sum()) for s in range(c.S)]
            assert counts[c.S - 1] == 0 and 0 < counts[c.S - 2] <= 3                        # an empty set, a set of at most 3 rows
            assert min(counts[:c.S - 2]) > 3
            assert (member == 0).any()                                                      # rows in no set


@pytest.mark.parametrize("case", INT_CASES, ids=lambda c: c.name)
def test_integer_cases_are_exact_in_fp32_and_have_ties(case):
    query, base, member = kc.tables(case.name)
    assert np.array_equal(query, np.rint(query)) and np.array_equal(base, np.rint(base))
    d, dist, index, _ = kc.reference(case.name)
    # every partial sum of either form is bounded by the sum of absolute terms: D * (2 span)^2 for the direct form, and
    # |q|^2 + |b|^2 + 2 sum |q_i b_i| <= 4 D span^2 for the dot form, whatever the order
    assert 4 * case.D * case.span ** 2 < 2 ** 24 and int(d.max()) < 2 ** 24
    if d.shape[1] > 8:
        # ties: adjacent ranks of a query's sorted distances that are equal (at D = 6 most of them)
        srt = np.sort(d, axis=1)
        share = float((srt[:, 1:] == srt[:, :-1]).mean())
        assert share > (0.5 if case.D == 6 else 0.01), share
        valid = index[:, :, 1:] >= 0
        assert ((dist[:, :, 1:] == dist[:, :, :-1]) & valid).any() or case.k == 1          # and inside the returned lists
    if case.exclude_self:
        # a planted duplicate of row i stays eligible at distance 0; row i itself does not
        rows = np.arange(d.shape[0])
        assert not (index == rows[:, None, None]).any()
        dup = [i for i in range(3, d.shape[0], 7) if member[i] & member[i - 2]]
        assert dup
        for i in dup[:5]:
            s = int(np.log2(int(member[i] & member[i - 2]) & -int(member[i] & member[i - 2])))
            assert dist[i, s, 0] == 0 and index[i, s, 0] != i and d[i, index[i, s, 0]] == 0


@pytest.mark.parametrize("case", REAL_CASES, ids=lambda c: c.name)
def test_real_cases_stay_inside_the_selection_bound_in_fp32(case):
    """The fp32 dot form selects; the float64 distance of its j-th pick is compared with the j-th smallest float64 distance."""
    query, base, member = kc.tables(case.name)
    d, ref_d, ref_i, _ = kc.reference(case.name)
    approx = kc.dot_form_fp32(query, base).astype(np.float64)
    approx[~np.isfinite(d)] = np.nan
    _, got_i, _ = kc.ref_knn(approx, member, case.S, case.k, case.exclude_self)
    assert np.array_equal(got_i >= 0, ref_i >= 0)
    valid = got_i >= 0
    qi = np.nonzero(valid)[0]
    err = np.abs(d[qi, got_i[valid]] - ref_d[valid])
    qn, bn = (query.astype(np.float64) ** 2).sum(axis=1), (base.astype(np.float64) ** 2).sum(axis=1)
    assert np.all(err <= kc.selection_bound(case.D, qn, np.nanmax(bn))[qi])
    if case.kind == "clustered" and case.D == 768:
        # why the reported distance is recomputed: the dot form misses near distances by far more than the reported bound allows
        near = ref_d[valid] < 1.0
        dot_err = np.abs(approx[qi, got_i[valid]] - d[qi, got_i[valid]])[near]
        assert np.median(dot_err / d[qi, got_i[valid]][near]) > 100 * 2 * (case.D + 2) * kc.U


# ---------------------------------------------------------------------------------------------- the plan
def test_plan_over_the_case_table():
    merged = set()
    for c in kc.CASES:
        Q, N, tile, slab = kc.shape(c)
        p = ops.knn_plan(Q, N, c.D, c.S, c.k)
        assert p["tile_q"] == tile == (64 if c.S * c.k <= 200 else 32) and p["tile_b"] == 128
        assert p["slab_rows"] == slab and p["slab_rows"] % p["tile_b"] == 0
        assert p["slabs"] == -(-N // slab) and p["merge"] == (p["slabs"] > 1) and p["slabs"] <= p["max_slabs"]
        assert (p["grid_x"], p["grid_y"]) == (-(-Q // tile), p["slabs"]) and p["threads"] == 256 and p["launches"] == 3
        assert 0 < p["lds_bytes"] <= 160 * 1024
        assert p["vector_loads"] == (c.D % 4 == 0)
        assert p["work_bytes"] >= 4 * (Q + N) + 8 * p["slabs"] * Q * c.S * c.k
        merged.add(p["merge"])
    assert merged == {False, True}
    assert {c.S * c.k > 200 for c in kc.CASES} == {False, True}              # both query tiles


def test_plan_of_the_sizes_the_feature_is_for():
    dev, test, self_ = (ops.knn_plan(q, 16326, 768, 12, 10) for q in (1871, 4662, 16326))
    assert (dev["grid_x"], dev["slabs"]) == (30, 8) and dev["merge"]          # 15 tiles of 128 would idle the device: slabs fill it
    assert test["slabs"] == 3 and self_["slabs"] == 1 and not self_["merge"]
    for p in (dev, test, self_):
        assert p["grid_x"] * p["grid_y"] <= 256 and p["slabs"] * p["slab_rows"] >= 16326
    for S in range(1, 17):
        for k in range(1, 17):
            assert ops.knn_plan(100, 1000, 1024, S, k)["lds_bytes"] <= 160 * 1024


def test_work_bytes_only_grow():
    base = dict(Q=65, N=300, D=768, S=12, k=10)
    for key, values in (("Q", [1, 63, 64, 65, 500, 1871, 4662, 8192, 8256, 16326, 100000]), ("N", [1, 127, 128, 129, 259, 16326, 10 ** 6]),
                        ("S", range(1, 17)), ("k", range(1, 17))):
        sizes = [ops.knn_plan(**dict(base, **{key: v}))["work_bytes"] for v in values]
        assert sizes == sorted(sizes) and sizes[0] > 0, (key, sizes)
    assert ops.knn_plan(65, 300, 6, 12, 10)["work_bytes"] == ops.knn_plan(65, 300, 1024, 12, 10)["work_bytes"]


def test_plan_refuses_shapes_outside_the_limits():
    for bad in (dict(D=0), dict(D=1025), dict(S=0), dict(S=17), dict(k=0), dict(k=17), dict(N=0), dict(Q=-1), dict(N=2 ** 31)):
        with pytest.raises(_lib.MMDAError, match="mmda_knn_plan_describe"):
            ops.knn_plan(**dict(dict(Q=4, N=4, D=8, S=1, k=1), **bad))
    assert ops.knn_plan(0, 4, 8, 1, 1)["grid_x"] == 1


# ---------------------------------------------------------------------------------------------- the definitions
def test_trust_score_on_a_line():
    """One class on a line: negatives at 0 and 1, positives at 4 and 10.  A query at 3 decided positive: the nearest positive is 1
    away, the nearest negative 2: trust 2.  Decided negative: 1 / 2."""
    base = np.array([[0.0], [1.0], [4.0], [10.0]], dtype=np.float32)
    truth = np.array([[0.0], [0.0], [1.0], [1.0]])
    query = np.array([[3.0], [3.0], [4.0], [-2.0]], dtype=np.float32)
    labels = np.array([[1.0], [0.0], [1.0], [1.0]])
    members = kc.ref_members(truth)
    assert members.tolist() == [1, 1, 2, 2]
    dist, index, _ = kc.ref_knn(kc.pair_distances(query, base), members, 2, 1)
    assert dist[:, :, 0].tolist() == [[4.0, 1.0], [4.0, 1.0], [9.0, 0.0], [4.0, 36.0]]
    assert index[:, :, 0].tolist() == [[1, 2], [1, 2], [1, 2], [0, 2]]
    trust, p, o = kc.ref_trust(dist, labels)
    assert trust[0, 0] == 2.0 / (1.0 + 1e-12) and trust[1, 0] == 1.0 / (2.0 + 1e-12)
    assert trust[2, 0] == 3.0 / 1e-12                      # the query IS a row of its decided label: min_dist keeps the ratio finite
    assert trust[3, 0] == 2.0 / (6.0 + 1e-12)
    assert p[:, 0].tolist() == [1.0, 4.0, 0.0, 36.0] and o[:, 0].tolist() == [4.0, 1.0, 9.0, 4.0]
    empty = np.array([[[np.inf], [4.0]]])                  # no negative row at all
    assert kc.ref_trust(empty, np.array([[1.0]]))[0][0, 0] == np.inf and kc.ref_trust(empty, np.array([[0.0]]))[0][0, 0] == 0.0
    assert kc.ref_trust(np.full((1, 2, 1), np.inf), np.array([[1.0]]))[0][0, 0] == 0.0


def test_density_filter_rule():
    """A set of 8 members with radii 1 .. 8 at alpha = 0.25 keeps the ceil(0.75 * 8) = 6 smallest; ties at the threshold stay; at
    alpha = 0 everything stays; a set smaller than k is kept whole."""
    radius = np.full((10, 3), np.inf)
    inside = np.zeros((10, 3), dtype=bool)
    inside[:8, 0] = True
    radius[:8, 0] = [3, 1, 8, 2, 7, 4, 6, 5]
    inside[2:, 1] = True
    radius[2:, 1] = [1, 2, 2, 2, 2, 2, 9, 9]
    inside[:2, 2] = True                                   # fewer than k = 3 members: radii are +inf, kept whole
    kept = kc.ref_density_filter(radius, inside, 3, 0.25)
    assert kept[:, 0].tolist() == [True, True, False, True, False, True, True, True, False, False]
    assert kept[:, 1].tolist() == [False, False] + [True] * 6 + [False, False]
    assert kept[:, 2].tolist() == [True, True] + [False] * 8
    assert np.array_equal(kc.ref_density_filter(radius, inside, 3, 0.0), inside)
    for alpha in (0.1, 0.5, 0.9):
        k2 = kc.ref_density_filter(radius, inside, 3, alpha)
        assert k2[:, 0].sum() == int(np.ceil((1 - alpha) * 8)) and not (k2 & ~inside).any()


def test_members_and_vote():
    truth = np.array([[1, 0, 1], [0, 0, 0], [1, 1, 1]])
    assert kc.ref_members(truth).tolist() == [0b100110, 0b010101, 0b101010]
    index = np.array([[0, 2, -1], [1, -1, -1]])
    assert np.array_equal(kc.ref_vote(index, truth), np.array([[1.0, 0.5, 1.0], [0.0, 0.0, 0.0]], dtype=np.float32))


# ---------------------------------------------------------------------------------------------- refusals, by name
def test_knn_search_refusals():
    from mmda_amd import knn_search
    host = torch.zeros(4, 8)
    with pytest.raises(_lib.MMDAError, match="knn_search needs device tensors.*query"):
        knn_search(host, host, 1)

    class FakeCuda(torch.Tensor):
        is_cuda = True

    q = torch.zeros(4, 8).as_subclass(FakeCuda)
    for kw, text in ((dict(query=torch.zeros(4).as_subclass(FakeCuda)), "query must be 2-D"),
                     (dict(base=torch.zeros(4, 9).as_subclass(FakeCuda)), "base has 9 columns"),
                     (dict(query=torch.zeros(4, 1025).as_subclass(FakeCuda), base=torch.zeros(4, 1025).as_subclass(FakeCuda)),
                      "query must have D in 1 .. 1024"),
                     (dict(k=0), "k must be an int in 1 .. 16"), (dict(k=17), "k must be an int in 1 .. 16"),
                     (dict(k=2.0), "k must be an int"), (dict(sets=0), "sets must be an int in 1 .. 16"),
                     (dict(sets=17), "sets must be an int in 1 .. 16"),
                     (dict(base=torch.zeros(0, 8).as_subclass(FakeCuda)), "base must have at least one row"),
                     (dict(member=torch.zeros(5, dtype=torch.int32).as_subclass(FakeCuda)), "member must be"),
                     (dict(member=torch.zeros(4).as_subclass(FakeCuda)), "member must be")):
        args = dict(dict(query=q, base=q, k=1), **kw)
        with pytest.raises(ValueError, match=text):
            knn_search(**args)
    with pytest.raises(_lib.MMDAError, match="member is not one"):
        knn_search(q, q, 1, member=torch.zeros(4, dtype=torch.int32))


def test_trust_refusals():
    from mmda_amd import TrustIndex, step_rules
    from mmda_amd.neighbours import check_trust_settings
    with pytest.raises(_lib.MMDAError, match="TrustIndex.fit needs device tensors"):
        TrustIndex.fit(torch.zeros(4, 8), torch.zeros(4, 2))
    check_trust_settings(10, 0.0, 6)
    check_trust_settings(1, 0.999, 8)
    for alpha in (-0.1, 1.0, 2, "0.5", None, True):
        with pytest.raises(ValueError, match="alpha must be a number in \\[0, 1\\)"):
            check_trust_settings(10, alpha, 6)
    for k in (0, 17, 2.5, True):
        with pytest.raises(ValueError, match="k must be an int in 1 .. 16"):
            check_trust_settings(k, 0.0, 6)
    for classes in (0, 9):
        with pytest.raises(ValueError, match="truth must have 1 .. 8 classes"):
            check_trust_settings(10, 0.0, classes)
    assert [n for n, _ in step_rules.TRUST_RULES] == ["trust_sentiment"]
    assert step_rules.trust_verdict("emotion", 10) is None
    assert step_rules.trust_verdict("sentiment", 5) == ("trust_sentiment", dict(k=5))
    with pytest.raises(_lib.MMDAError) as e:
        check_trust_settings(5, 0.0, 1, task="sentiment")
    assert str(e.value) == dict(step_rules.TRUST_RULES)["trust_sentiment"].format(k=5) and "sentiment" in str(e.value)


def test_trust_k_defaults_to_nothing_and_is_refused_under_sentiment_at_build():
    from mmda_amd import step_rules
    from mmda_amd.config import DEFAULTS, get_config, make_config
    from mmda_amd.solver import Solver
    assert DEFAULTS["trust_k"] == 0 and DEFAULTS["trust_alpha"] == 0.0 and make_config().trust_k == 0
    assert get_config(parse=False).trust_k == 0
    c = get_config(parse=False, trust_k=10, trust_alpha=0.25)
    assert (c.trust_k, c.trust_alpha) == (10, 0.25)
    cfg = make_config(task="sentiment", num_classes=1, trust_k=5, vocab_size=16)
    with pytest.raises(_lib.MMDAError) as e:
        Solver(cfg, cfg, cfg, [], [], [], is_train=False).build()
    assert str(e.value) == dict(step_rules.TRUST_RULES)["trust_sentiment"].format(k=5)
    bad = make_config(trust_k=17, vocab_size=16)
    with pytest.raises(ValueError, match="k must be an int in 1 .. 16"):
        Solver(bad, bad, bad, [], [], [], is_train=False).build()


def test_flags_parse(monkeypatch):
    import sys
    from mmda_amd.config import get_config
    monkeypatch.setattr(sys, "argv", ["x", "--trust_k", "7", "--trust_alpha", "0.1"])
    c = get_config(parse=True)
    assert (c.trust_k, c.trust_alpha) == (7, 0.1)


# ---------------------------------------------------------------------------------------------- the C ABI without a GPU
def test_null_arguments_are_einval():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf) // 16 * 16 + 16
    ok = dict(query=p, base=p, member=p, dist=p, index=p, work=p)
    for name in ok:
        a = dict(ok, **{name: None})
        assert lib.mmda_knn_sets(a["query"], a["base"], a["member"], 1, 1, 1, 1, 1, 0, a["dist"], a["index"], a["work"], 1 << 20,
                                 None) == -1, name
    for shape in ((1, 1, 0, 1, 1), (1, 1, 1025, 1, 1), (1, 1, 1, 17, 1), (1, 1, 1, 1, 17), (1, 0, 1, 1, 1), (-1, 1, 1, 1, 1)):
        assert lib.mmda_knn_sets(p, p, p, shape[0], shape[1], shape[2], shape[3], shape[4], 0, p, p, p, 1 << 20, None) == -1, shape
    need = ops.knn_plan(1, 1, 1, 1, 1)["work_bytes"]
    assert lib.mmda_knn_sets(p, p, p, 1, 1, 1, 1, 1, 0, p, p, p, need - 1, None) == -1          # a work buffer that is too small
    assert lib.mmda_knn_sets(p, p, p, 1, 1, 1, 1, 1, 0, p, p, p + 4, need, None) == -1           # or misaligned
    assert lib.mmda_knn_sets(p, p, p, 0, 1, 1, 1, 1, 0, p, p, p, need, None) == 0                # no query rows: nothing to launch
    assert lib.mmda_knn_plan_describe(1, 1, 1, 1, 1, None) == -1
    t = dict(dist=p, labels=p, trust=p)
    for name in t:
        a = dict(t, **{name: None})
        assert lib.mmda_trust_score(a["dist"], None, a["labels"], 1, 1, 1, a["trust"], None, None, None, None, None) == -1, name
    assert lib.mmda_trust_score(p, None, p, 1, 1, 1, p, None, None, p, None, None) == -1         # a nearest table without index
    for n, C, k in ((-1, 1, 1), (1, 0, 1), (1, 9, 1), (1, 1, 0), (1, 1, 17)):
        assert lib.mmda_trust_score(p, p, p, n, C, k, p, None, None, None, None, None) == -1
    assert lib.mmda_trust_score(p, p, p, 0, 1, 1, p, None, None, None, None, None) == 0


def test_knn_plan_struct_size_matches_c_layout(tmp_path):
    code = textwrap.dedent("""
        #include <stdio.h>
        #include <stddef.h>
        #include "mmda_hip.h"
        int main(){printf("%zu %zu %zu\\n", sizeof(mmda_knn_plan), offsetof(mmda_knn_plan, work_bytes), offsetof(mmda_knn_plan, lds_bytes));
                   return 0;}""")
    (tmp_path / "s.c").write_text(code)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")], check=True)
    out = subprocess.run([str(tmp_path / "s")], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out] == [ctypes.sizeof(_lib.KnnPlan), _lib.KnnPlan.work_bytes.offset, _lib.KnnPlan.lds_bytes.offset]
    assert [f for f, _ in _lib.KnnPlan._fields_] == list(ops.KNN_PLAN_FIELDS)
