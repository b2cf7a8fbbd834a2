"""CPU: the ranking metrics' host functions (mmda_amd/ranking.py: rank_counts_host, figures_from_counts, label_ranking_host) against a
brute-force O(N^2) restatement (integers, compared for equality) and against scikit-learn's figures (tests/golden/rank/rank_cases.npz,
written by tests/golden/gen_golden_rank.py; sklearn is not imported here); what mmda_rank_plan_describe gives the shapes of
tests/test_gpu_rank.py; the native entry points' refusals (no launch: no GPU here); config.select_by."""
import ctypes
import os
import subprocess
import sys
import tempfile
import textwrap

import numpy as np
import pytest
import torch

from mmda_amd import _lib, ranking as rk
from rank_cases import gpu_shapes, value_case, value_classes

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def brute_counts(scores, truth):
    """{gp, gn, ep, en} by comparing every pair as the definition reads: fp32 compares, NaN as -inf"""
    s = np.asarray(scores, dtype=np.float32).copy()
    s[np.isnan(s)] = -np.inf
    pos = np.asarray(truth) > 0
    N, C = s.shape
    out = np.zeros((N, C, 4), dtype=np.uint32)
    for c in range(C):
        col = s[:, c]
        gt = col[None, :] > col[:, None]                        # [i, j]: s_j > s_i
        eq = col[None, :] == col[:, None]
        out[:, c, 0] = (gt & pos[None, :, c]).sum(1)
        out[:, c, 1] = (gt & ~pos[None, :, c]).sum(1)
        out[:, c, 2] = (eq & pos[None, :, c]).sum(1)
        out[:, c, 3] = (eq & ~pos[None, :, c]).sum(1)
    return out


def brute_rows(scores, truth):
    s = np.asarray(scores, dtype=np.float32).copy()
    s[np.isnan(s)] = -np.inf
    pos = np.asarray(truth) > 0
    N, C = s.shape
    st = [0] * rk.state_words(C)
    for i in range(N):
        P = int(pos[i].sum())
        st[0] += 1
        st[2 + P] += 1
        cover = 0
        for j in range(C):
            if pos[i, j]:
                rank = int((s[i] >= s[i, j]).sum())
                L = int(((s[i] >= s[i, j]) & pos[i]).sum())
                st[2 + (C + 1) + P] += L * (rk.LCM // rank)
                st[2 + 2 * (C + 1) + P] += rank - L
                cover = max(cover, rank)
        st[1] += cover
    return np.array(st, dtype=np.int64)


@pytest.fixture(scope="module")
def golden():
    d = np.load(os.path.join(HERE, "golden", "rank", "rank_cases.npz"))
    return {k: d[k] for k in d.files}


# ------------------------------------------------------------------------------------------------ the yardstick
def test_keys_order_the_special_values():
    v = np.array([np.nan, -np.inf, -1.0, -0.0, 0.0, 1e-45, 1.0, np.inf, -np.nan], dtype=np.float32)
    k = rk.score_keys(v)
    assert k.dtype == np.uint32
    assert k[0] == k[1] == k[8] and k[3] == k[4]                # NaN (either sign) == -inf; -0 == +0
    assert k[1] < k[2] < k[3] < k[5] < k[6] < k[7]
    assert k[1] == k.min()                                      # nothing is below a NaN's key


@pytest.mark.parametrize("shape", [(1, 1), (2, 1), (37, 6), (127, 3), (300, 16), (257, 5)], ids=lambda s: "x".join(map(str, s)))
def test_sorted_counts_equal_brute_force(shape):
    scores, truth = value_case(*shape)
    got = rk.rank_counts_host(scores, truth)
    assert got.dtype == np.uint32 and got.shape == shape + (4,)
    assert np.array_equal(got, brute_counts(scores, truth))
    assert (got.astype(np.int64).sum(2) <= shape[0]).all() and (got[:, :, 2] + got[:, :, 3] >= 1).all()
    assert np.array_equal(rk.label_ranking_host(scores, truth), brute_rows(scores, truth))


def test_figures_equal_sklearn(golden):
    n = int(golden["n_cases"])
    assert n >= 36 and float(golden["tpr"]) == 0.95
    exact_p = []
    for k in range(n):
        s, t, want, rows = (golden[f"{name}_{k}"] for name in ("scores", "truth", "classes", "rows"))
        N, C = s.shape
        table = rk.figures_from_counts(rk.rank_counts_host(s, t), t, tpr=0.95)
        got = table[:C, 2:]
        assert np.array_equal(np.isnan(got), np.isnan(want)), k
        assert np.nanmax(np.abs(got - want), initial=0.0) <= 1e-12, k
        assert np.array_equal(table[:C, 0], (t > 0).sum(0)) and np.array_equal(table[:C, 1], (t <= 0).sum(0))
        for f in range(2, 6):                                   # the macro row: nan-mean of the class rows
            col = table[:C, f]
            if np.isnan(col).all():
                assert np.isnan(table[C, f])
            else:
                assert abs(table[C, f] - np.nanmean(col)) <= C * 2.0 ** -52
        assert table[C, 0] == (~np.isnan(table[:C, 2])).sum() and table[C, 1] == (~np.isnan(table[:C, 3])).sum()
        if C > 1:
            fig = rk.label_ranking_figures(rk.label_ranking_host(s, t), C)
            got_rows = np.array([fig["lrap"], fig["ranking_loss"], fig["coverage_error"]])
            assert np.abs(got_rows - rows).max() <= 1e-12, k
        if C == 1 and int((t > 0).sum()) in (20, 40):
            exact_p.append(int((t > 0).sum()))
    assert sorted(exact_p) == [20, 20, 40, 40]                  # the cases where 0.95 P is exactly an integer


def test_undefined_figures_are_nan_and_nan_scores_are_lowest():
    s = np.array([[0.2, np.nan, 0.1], [0.9, 0.3, 0.1], [np.nan, 0.5, 0.1], [0.4, -np.inf, 0.1]], dtype=np.float32)
    t = np.array([[1, 0, 1], [0, 0, 1], [1, 0, 1], [0, 0, 1]], dtype=np.float32)
    table = rk.figures_from_counts(rk.rank_counts_host(s, t), t)
    # class 0: positives 0.2 and NaN, negatives 0.9 and 0.4: every negative is above every positive
    assert table[0, 2] == 0.0 and table[0, 5] == 1.0
    # class 1 has no positives, class 2 no negatives
    assert np.isnan(table[1, [2, 3, 5]]).all() and table[1, 4] == 1.0
    assert np.isnan(table[2, [2, 4, 5]]).all() and table[2, 3] == 1.0
    assert table[3, 0] == 1 and table[3, 1] == 2                # one class in the mean AUROC, two in mAP
    assert table[3, 2] == 0.0 and table[3, 3] == (table[0, 3] + 1.0) / 2
    c = rk.rank_counts_host(s, t)
    assert c[0, 1].tolist() == [0, 2, 0, 2]                     # a NaN ties with the real -inf: both below 0.3 and 0.5
    empty = rk.label_ranking_figures(np.zeros(rk.state_words(3), dtype=np.int64), 3)
    assert all(np.isnan(v) for v in empty.values())
    with pytest.raises(ValueError, match="tpr"):
        rk.figures_from_counts(c, t, tpr=0.0)


# ------------------------------------------------------------------------------------------------ the plan
def test_rank_plan_mirror_has_the_c_size():
    code = textwrap.dedent("""
        #include <stdio.h>
        #include "mmda_hip.h"
        int main(){printf("%zu\\n", sizeof(mmda_rank_plan)); return 0;}""")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(code)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")], check=True)
        out = subprocess.run([os.path.join(d, "s")], check=True, capture_output=True, text=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(_lib.RankPlan)


def test_gpu_shapes_reach_every_plan_form():
    shapes = gpu_shapes()
    assert len(set(shapes)) == len(shapes) == 12 and max(n for n, _ in shapes) == 20001
    plans = {s: rk.rank_plan(*s) for s in shapes}
    for (N, C), p in plans.items():
        assert p.rows_per_wg == 128 and p.tile == 512
        assert p.tiles == -(-N // p.tile) and p.grid_x == -(-N // p.rows_per_wg) and p.grid_y == C and p.grid_z == p.splits
        assert p.splits * p.tiles_per_split >= p.tiles > (p.splits - 1) * p.tiles_per_split       # every tile once, no empty split
        assert p.counts_bytes == N * C * 16
    R, T = 128, 512
    form = lambda s: (plans[s].tiles, plans[s].splits, plans[s].tiles_per_split, plans[s].grid_x)
    # one tile, one row block more at R + 1
    assert form((R - 1, 6)) == (1, 1, 1, 1) and form((R, 6)) == (1, 1, 1, 1) and form((R + 1, 6)) == (1, 1, 1, 2)
    # the tile edge: a second tile, of one row, at T + 1 -- and with it the split form (the clear and the integer adds)
    assert form((T - 1, 6))[:2] == (1, 1) and form((T, 6))[:2] == (1, 1) and form((T + 1, 6))[:3] == (2, 2, 1)
    # several tiles walked by ONE split: enough row blocks x classes that the plan stops splitting
    above = shapes[-2]
    assert plans[above].splits == 1 and plans[above].tiles >= 2 and plans[above].tiles_per_split == plans[above].tiles
    assert rk.rank_plan(above[0] - 1 - R, 16).splits > 1       # and that shape sits just above that threshold
    # several splits of several tiles each
    p = plans[(20001, 6)]
    assert p.splits > 1 and p.tiles_per_split > 1
    assert plans[(300, 16)].splits == 1 and plans[(1, 1)].grid_x == 1
    # the plan has no cap on the grid: nothing strides
    assert rk.rank_plan(1 << 20, 1).grid_x == (1 << 20) // R


def test_every_gpu_shape_holds_every_value_class():
    """all of them from six classes on: every shape but the two single-class ones the issue fixes"""
    for N, C in gpu_shapes():
        got = value_classes(*value_case(N, C))
        if C >= 6:
            assert all(got.values()), ((N, C), got)
        else:
            assert (N, C) in ((1, 1), (2, 1)) and got["nan_in_last_row"]


def test_row_chunks_fit_both_limits():
    """RowRanking streams a batch in chunks the native entry accepts: the row cap and the comparison cap it shares with the counts"""
    lib, plan = _lib.load(), _lib.RankPlan()
    for C in range(1, 17):
        n = rk.max_rows(C)
        assert n <= rk.MAX_ROWS and n * n * C <= rk.MAX_PAIRS
        assert lib.mmda_rank_plan_describe(n, C, ctypes.byref(plan)) == 0
        assert lib.mmda_rank_plan_describe(n + 1, C, ctypes.byref(plan)) == -1
        assert lib.mmda_rank_rows_accumulate(4096, 4096, n + 1, C, 4096, None) == -1
    assert rk.max_rows(4) == 1 << 20 and rk.max_rows(16) == 1 << 19


def test_native_refusals_without_gpu():
    """MMDA_EINVAL (-1) before any launch; N == 0 is MMDA_OK with no launch.  Pointers are never dereferenced on the host."""
    lib = _lib.load()
    p = 4096                                                    # a non-NULL, 16-byte aligned stand-in: never read
    plan = _lib.RankPlan()
    for hole in range(3):
        a = [p, p, p]
        a[hole] = None
        assert lib.mmda_rank_counts(a[0], a[1], 4, 6, a[2], None) == -1
        assert lib.mmda_rank_finish(a[0], a[1], 4, 6, 0.95, a[2], None) == -1
        assert lib.mmda_rank_rows_accumulate(a[0], a[1], 4, 6, a[2], None) == -1
    assert lib.mmda_rank_plan_describe(4, 6, None) == -1
    big = 1 << 20
    for N, C in ((4, 0), (4, 17), (-1, 6), (big + 1, 1), (big, 5), (1 << 19, 16 + 1), (2 ** 19 + 1, 16)):
        assert lib.mmda_rank_counts(p, p, N, C, p, None) == -1, (N, C)
        assert lib.mmda_rank_finish(p, p, N, C, 0.95, p, None) == -1, (N, C)
        assert lib.mmda_rank_rows_accumulate(p, p, N, C, p, None) == -1, (N, C)
        assert lib.mmda_rank_plan_describe(N, C, ctypes.byref(plan)) == -1, (N, C)
    for level in (0.0, -0.5, 1.5, float("nan")):
        assert lib.mmda_rank_finish(p, p, 4, 6, level, p, None) == -1
    assert lib.mmda_rank_counts(p, p, 4, 6, p + 4, None) == -1  # counts is read and written sixteen bytes at a time
    # at the cap: accepted by the plan (which launches nothing): 2^20 rows of 4 classes, 2^19 rows of 16
    assert lib.mmda_rank_plan_describe(big, 4, ctypes.byref(plan)) == 0 and plan.counts_bytes == big * 4 * 16
    assert lib.mmda_rank_plan_describe(1 << 19, 16, ctypes.byref(plan)) == 0
    for C in (1, 6, 16):
        assert lib.mmda_rank_counts(p, p, 0, C, p, None) == 0
        assert lib.mmda_rank_finish(p, p, 0, C, 0.95, p, None) == 0
        assert lib.mmda_rank_rows_accumulate(p, p, 0, C, p, None) == 0
    assert lib.mmda_rank_plan_describe(0, 6, ctypes.byref(plan)) == 0 and plan.splits == 0 and plan.counts_bytes == 0


def test_python_refusals_name_the_rule():
    with pytest.raises(_lib.MMDAError, match="ranking_metrics"):
        rk.ranking_metrics(torch.zeros(4, 6), torch.zeros(4, 6))
    with pytest.raises(_lib.MMDAError, match="failure_prediction"):
        rk.failure_prediction(torch.zeros(4, 6), torch.zeros(4, 6))
    with pytest.raises(_lib.MMDAError, match="RowRanking"):
        rk.RowRanking(6, "cpu")
    with pytest.raises(ValueError, match=r"2\^20"):
        rk.check_size((1 << 20) + 1, 1)
    with pytest.raises(ValueError, match=r"2\^42"):
        rk.check_size(1 << 20, 5)
    with pytest.raises(ValueError, match="1 .. 16 classes"):
        rk.check_size(10, 17)
    rk.check_size(1 << 20, 4)


# ------------------------------------------------------------------------------------------------ config.select_by
def test_select_by_parses_and_defaults_to_valid_loss(monkeypatch):
    from mmda_amd import get_config, make_config
    assert make_config().select_by == "valid_loss"
    monkeypatch.setattr(sys, "argv", ["prog"])
    assert get_config().select_by == "valid_loss"
    for value in ("map", "auroc", "valid_loss"):
        monkeypatch.setattr(sys, "argv", ["prog", "--select_by", value])
        assert get_config().select_by == value
    monkeypatch.setattr(sys, "argv", ["prog", "--select_by", "f1"])
    with pytest.raises(SystemExit):
        get_config()


def test_select_by_is_refused_under_a_process_group(monkeypatch):
    from mmda_amd import make_config
    from mmda_amd.solver import Solver
    from mmda_amd.utils import convert
    monkeypatch.setattr(convert, "_DEVICE", convert._DEVICE)    # a Solver sets the process-wide device: put it back afterwards
    assert rk.check_select_by("map") == "map" and rk.check_select_by("valid_loss", process_group=True) == "valid_loss"
    with pytest.raises(ValueError, match="select_by must be one of"):
        rk.check_select_by("f1")
    for value in ("map", "auroc"):
        with pytest.raises(ValueError, match=f"select_by='{value}'.*process group"):
            rk.check_select_by(value, process_group=True)
    # Solver.build() asks before it makes anything: an initialised process group is enough
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    c = make_config(device="cpu", vocab_size=32, select_by="map")
    s = Solver(c, c, c, [], [], [], is_train=True, model=None)
    with pytest.raises(ValueError, match="select_by='map'.*process group"):
        s.build()
    assert s.model is None
    c = make_config(device="cpu", vocab_size=32, select_by="best")
    with pytest.raises(ValueError, match="select_by must be one of"):
        Solver(c, c, c, [], [], [], is_train=True, model=None).build()


def test_train_keeps_the_epoch_with_the_highest_figure(tmp_path, monkeypatch):
    """train()'s choice alone, with the epoch, the evaluation and the ranking scripted: the dev loss falls every epoch, so the loop
    without the option would keep the last one; mAP peaks at epoch 1, ties go to the later epoch as the loss's `<=` does, and an epoch
    whose figure is undefined (NaN) is never kept."""
    from types import SimpleNamespace
    from mmda_amd import make_config
    from mmda_amd.solver import Solver
    from mmda_amd.utils import convert
    monkeypatch.setattr(convert, "_DEVICE", convert._DEVICE)
    monkeypatch.chdir(tmp_path)

    def run(select_by, figures):
        c = make_config(device="cpu", vocab_size=32, name=select_by, n_epoch=len(figures), select_by=select_by)
        s = Solver(c, c, c, [], [], [], is_train=True, model=torch.nn.Linear(1, 1, bias=False))
        s.optimizer = torch.optim.SGD(s.model.parameters(), lr=0.1)
        epoch = iter(range(len(figures)))

        def train_epoch():
            with torch.no_grad():
                s.model.weight.fill_(float(next(epoch)))          # the weights of epoch e hold e
            return dict(total=1.0)

        s.train_epoch = train_epoch
        s.eval = lambda mode=None, **kw: (10.0 - s.model.weight.item(), 0.5, None, None)
        key = {"map": "map", "auroc": "macro_auroc"}.get(select_by)
        ranked = []

        def rank(mode, **kw):
            ranked.append(mode)
            return {"scores": SimpleNamespace(as_dict=lambda: {key: figures[int(s.model.weight.item())]}), "confidence": None}

        s.rank = rank
        history = s.train()
        saved = torch.load(tmp_path / "checkpoints" / f"model_{select_by}.std", weights_only=True)
        return history, float(saved["weight"]), ranked

    nan = float("nan")
    history, kept, ranked = run("map", [0.5, 0.7, 0.6])
    assert kept == 1.0 and ranked == ["dev"] * 3 and [h["valid_map"] for h in history] == [0.5, 0.7, 0.6]
    history, kept, _ = run("auroc", [0.5, nan, 0.5, 0.4])
    assert kept == 2.0 and history[2]["valid_auroc"] == 0.5
    history, kept, ranked = run("valid_loss", [0.5, 0.7, 0.6])
    assert kept == 2.0 and ranked == [] and set(history[0]) == {"epoch", "train", "valid_loss", "valid_acc"}
