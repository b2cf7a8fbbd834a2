"""CPU: the inference pass's host side -- ``inference_plan``, the refusals of the two native entry points and of the Python interface
(all raised before any launch, so no device is needed), the ctypes mirrors of the two new structs, and the ``utils.tools`` files."""
import ctypes
import os
import subprocess
import textwrap
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from mmda_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


# ------------------------------------------------------------------------------------------------ the plan
def _lengths(n=4096, seed=0):
    return np.random.default_rng(seed).integers(5, 51, size=n)          # uniform in [5, 50]


@pytest.mark.parametrize("order", ["length", "dataset"])
@pytest.mark.parametrize("n,B", [(1, 4), (21, 8), (32, 32), (4096, 256)])
def test_plan_holds_every_sample_exactly_once(order, n, B):
    from mmda_amd import inference_plan
    L = _lengths(n, seed=n)
    plan, bounds = inference_plan(L, B, order)
    assert sorted(plan.tolist()) == list(range(n))
    assert bounds[0] == 0 and bounds[-1] == n and bool((np.diff(bounds) > 0).all()) and int(np.diff(bounds).max()) <= B
    for lo, hi in zip(bounds[:-1], bounds[1:]):                         # every batch is sorted as collate_fn sorts it
        assert bool((np.diff(L[plan[lo:hi]]) <= 0).all())


def test_length_order_starts_with_the_longest_batch():
    from mmda_amd import inference_plan
    L = _lengths(1000, seed=3)
    plan, bounds = inference_plan(L, 32, "length")
    T = L[plan[bounds[:-1]]]
    assert T[0] == L.max() and bool((np.diff(T) <= 0).all())           # the workspace is carved once, at its largest


def test_plans_equal_batch_plan_of_their_sequences():
    from mmda_amd import batch_plan, inference_plan
    L = _lengths(777, seed=5)
    for order, seq in (("length", np.argsort(-L, kind="stable")), ("dataset", np.arange(777))):
        got, want = inference_plan(L, 32, order), batch_plan(L, seq, 32)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # ties keep dataset order: the sort is stable
    plan, _ = inference_plan(np.array([3, 7, 3, 7, 3]), 8, "length")
    assert plan.tolist() == [1, 3, 0, 2, 4]


def test_length_order_runs_fewer_recurrent_steps():
    """The seeded corpus of DESIGN.md 4f: n = 4096, lengths uniform in [5, 50], B = 32: the sum of the batches' T drops 6296 -> 3562."""
    from mmda_amd import inference_plan
    L = _lengths()
    steps = {}
    for order in ("dataset", "length"):
        plan, bounds = inference_plan(L, 32, order)
        steps[order] = int(L[plan[bounds[:-1]]].sum())
    assert steps == {"dataset": 6296, "length": 3562}


def test_plan_refuses_an_unknown_order():
    from mmda_amd import inference_plan
    for bad in ("loader", "", None, 3):
        with pytest.raises(ValueError):
            inference_plan([3, 2, 1], 2, bad)


# ------------------------------------------------------------------------------------------------ the two native entry points
def _src(**kw):
    s = _lib.InferSrc(scores=16, labels=16, tcp=16, hfused=16, x6=16, probs=16, ncls=6, hs=128, nhead=2)       # (never dereferenced)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _out(**kw):
    o = _lib.InferOut(scores=16, labels=16, tcp=16, hidden=16, utterance=16, attention=16)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_collect_refuses_bad_arguments_without_a_launch():
    lib = _lib.load()
    call = lambda s, o, B=4: lib.mmda_infer_collect(None if s is None else ctypes.byref(s), None if o is None else ctypes.byref(o), None, 0,
                                                   B, None)
    assert call(None, _out()) == EINVAL
    assert call(_src(), None) == EINVAL
    assert call(_src(), _lib.InferOut()) == EINVAL                      # every table NULL
    for B in (0, -1):
        assert call(_src(), _out(), B) == EINVAL
    for k in ("ncls", "hs", "nhead"):
        for val in (0, -2):
            assert call(_src(**{k: val}), _out()) == EINVAL, (k, val)
    pairs = dict(scores="scores", labels="labels", tcp="tcp", hidden="hfused", utterance="x6", attention="probs")
    for table, source in pairs.items():                                 # a table whose source is missing
        only = _lib.InferOut(**{table: 16})
        assert call(_src(**{source: None}), only) == EINVAL, table
        assert call(_src(**{source: None}), _out()) == EINVAL, table


def test_model_collect_refuses_bad_arguments_without_a_launch():
    from mmda_amd import MISA, make_config
    lib = _lib.load()
    o = _out()
    assert lib.mmda_misa_infer_collect(None, ctypes.byref(o), None, 0, None) == EINVAL
    m = MISA(make_config(vocab_size=32))
    assert lib.mmda_misa_infer_collect(m._h, None, None, 0, None) == EINVAL
    assert lib.mmda_misa_infer_collect(m._h, ctypes.byref(o), None, 0, None) == EINVAL       # no workspace: nothing to collect from


def test_struct_mirrors_have_the_compilers_sizes(tmp_path):
    code = textwrap.dedent("""
        #include <stdio.h>
        #include <stddef.h>
        #include "mmda_hip.h"
        int main(){printf("%zu %zu %zu %zu %zu\\n", sizeof(mmda_infer_src), sizeof(mmda_infer_out), offsetof(mmda_infer_src, ncls),
                          offsetof(mmda_infer_src, nhead), offsetof(mmda_infer_out, attention)); return 0;}""")
    (tmp_path / "s.c").write_text(code)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")], check=True)
    out = subprocess.run([str(tmp_path / "s")], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out] == [ctypes.sizeof(_lib.InferSrc), ctypes.sizeof(_lib.InferOut), _lib.InferSrc.ncls.offset,
                                     _lib.InferSrc.nhead.offset, _lib.InferOut.attention.offset]


# ------------------------------------------------------------------------------------------------ the Python refusals
@pytest.fixture(scope="module")
def cpu_model():
    from mmda_amd import MISA, make_config
    return MISA(make_config(vocab_size=32))


def _cpu_dataset(n=3):
    from mmda_amd import DeviceDataset
    L = np.arange(1, n + 1, dtype=np.int64)
    P = int(L.sum())
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(L)]))
    return DeviceDataset(torch.zeros(P, dtype=torch.int32), torch.zeros(P, 35), torch.zeros(P, 74), off, None, torch.zeros(n), L,
                         np.array([f"s{i}" for i in range(n)], dtype=object))


def test_fields_are_validated(cpu_model):
    from mmda_amd import FIELDS, InferencePass
    assert FIELDS == ("scores", "labels", "tcp", "hidden", "utterance", "attention")
    assert InferencePass(cpu_model).fields == ("scores", "labels", "tcp", "hidden")
    assert InferencePass(cpu_model, ["attention", "scores"]).fields == ("scores", "attention")
    for bad in ((), [], ("scores", "h"), ("Hidden",), (3,)):
        with pytest.raises(ValueError):
            InferencePass(cpu_model, bad)


def test_a_model_or_dataset_off_the_gpu_is_refused(cpu_model):
    from mmda_amd import InferencePass
    p = InferencePass(cpu_model)
    with pytest.raises(_lib.MMDAError, match="model is on cpu"):
        p.run_loader([])
    with pytest.raises(_lib.MMDAError, match="dataset is on cpu"):
        p.run(_cpu_dataset(), 2)
    assert cpu_model._ws is None and cpu_model._seed == 0x5EED          # nothing ran, no seed was drawn


def test_an_unknown_order_is_refused_first(cpu_model):
    from mmda_amd import InferencePass
    with pytest.raises(ValueError):
        InferencePass(cpu_model).run(_cpu_dataset(), 2, order="loader")


def test_solver_infer_refuses_before_touching_the_model(cpu_model):
    from mmda_amd.solver import Solver
    cfg = cpu_model.config
    s = Solver(cfg, cfg, cfg, [], [], [], is_train=False, model=cpu_model)
    for order in ("length", "dataset"):
        with pytest.raises(ValueError, match="DeviceLoader"):
            s.infer("dev", order=order)                                  # a plain list cannot be re-batched
    with pytest.raises(ValueError):
        s.infer("dev", order="random")
    with pytest.raises(ValueError):
        s.infer("valid")
    with pytest.raises(ValueError):
        s.infer("dev", fields=())


# ------------------------------------------------------------------------------------------------ the files
@pytest.mark.parametrize("confid", [False, True])
def test_tools_round_trip_under_the_reference_names(tmp_path, monkeypatch, confid):
    from mmda_amd.utils import tools
    monkeypatch.chdir(tmp_path)
    args = SimpleNamespace(use_confidNet=confid)
    g = torch.Generator().manual_seed(3)
    h, tcp = torch.randn(5, 768, generator=g), torch.rand(5, 6, generator=g)
    tools.save_hidden(args, h, dataset="mosei")
    tools.save_tcp(args, tcp, dataset="mosei")
    name = "MISA_C_mosei.pt" if confid else "MISA_mosei.pt"
    assert sorted(os.listdir(tmp_path)) == ["hidden_vectors", "tcp_vectors"]
    assert os.listdir(tmp_path / "hidden_vectors") == [name] and os.listdir(tmp_path / "tcp_vectors") == [name]
    assert torch.equal(tools.load_hidden(args, dataset="mosei"), h) and torch.equal(tools.load_tcp(args, dataset="mosei"), tcp)
    tools.save_hidden(args, h * 2, dataset="mosei")                     # a second save overwrites, the folder is reused
    assert torch.equal(tools.load_hidden(args, dataset="mosei"), h * 2)
    other = SimpleNamespace(use_confidNet=not confid)                   # the other name is another file
    with pytest.raises(FileNotFoundError):
        tools.load_hidden(other, dataset="mosei")
