"""GPU: every evaluation report of ``Solver`` walks its split exactly once.  One forward per batch is what the model's
forward counter shows (``_fwd_id``), and one seed per forward is what keeps training that continues behind an evaluation bit-identical
(``_seed``: the 64-bit linear congruential recurrence of ``MISA._next_seed``, restated here).  The tiny model and the seven samples of
tests/uncertainty_cases.py at batch size 4 (two batches, the second partial), fp32, built as tests/test_gpu_bootstrap.py builds its
solver; the host-tuple case runs the same samples through ``collate_fn`` (the ``to_gpu`` placement), the sentiment case the MOSEI-width
model of tests/test_gpu_senti.py (``num_classes=1``) over the samples' sentiment column."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import uncertainty_cases as uc
from oracle import misa_oracle as orc

DEV = "cuda:0"
MASK64 = 0xFFFFFFFFFFFFFFFF


def _seed_after(seed, forwards):
    for _ in range(forwards):
        seed = (seed * 6364136223846793005 + 1442695040888963407) & MASK64
    return seed


class ListLoader:
    def __init__(self, batches):
        self.batches, self.dataset = batches, self

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


def _solver(cfg, params, dev, **extra):
    from mmda_amd import make_config, models
    from mmda_amd.solver import Solver
    cfg.learning_rate, cfg.clip = 1e-3, 1.0
    c = make_config(precision="fp32", device=DEV, n_epoch=1, name="walk", **vars(cfg), **extra)
    m = models.MISA(c)
    m.load_state_dict(params)
    torch.manual_seed(0)
    return Solver(c, c, c, ListLoader([]), dev, dev, is_train=True, model=m).build()


def _thresholds():
    from mmda_amd.calibrate import Thresholds
    return Thresholds([0.3, 0.4, 0.5, 0.6, 0.7, 0.45], [0] * 6)


def _scaling():
    from mmda_amd.reliability import Scaling
    return Scaling([1.5] * 6, [0.1] * 6)


REPORTS = {
    "eval": lambda s: s.eval("dev"),
    "eval_keep": lambda s: s.eval("dev", keep=5),
    "eval_thresholds": lambda s: s.eval("dev", thresholds=_thresholds()),
    "eval_scaling": lambda s: s.eval("dev", scaling=_scaling()),
    "eval_thresholds_scaling": lambda s: s.eval("dev", thresholds=_thresholds(), scaling=_scaling()),
    "calibrate": lambda s: s.calibrate("dev"),
    "reliability": lambda s: s.reliability("dev"),
    "fit_scaling": lambda s: s.fit_scaling("dev"),
    "rank": lambda s: s.rank("dev"),
    "rank_without_confidence": lambda s: s.rank("dev", confidence=False),
    "bootstrap": lambda s: s.bootstrap("dev", replicates=8),
    "bootstrap_thresholds": lambda s: s.bootstrap("dev", replicates=8, thresholds=_thresholds()),
}


def _walks_once(s, report):
    m, n = s.model, len(s.dev_data_loader)
    assert n == 2
    fwd, seed = m._fwd_id, m._seed
    out = report(s)
    assert m._fwd_id - fwd == n, f"{m._fwd_id - fwd} forwards over {n} batches"
    assert m._seed == _seed_after(seed, n)
    return out


@pytest.fixture(scope="module")
def solver():
    from mmda_amd import DeviceDataset, DeviceLoader
    return _solver(uc.config(), uc.params(), DeviceLoader(DeviceDataset.from_samples(uc.make_samples(), DEV), 4))


@pytest.mark.parametrize("name", list(REPORTS))
def test_every_report_walks_its_split_once(solver, name):
    _walks_once(solver, REPORTS[name])


def test_host_tuples_are_walked_once():
    from mmda_amd.data import collate_fn
    samples = uc.make_samples()
    batches = [collate_fn(samples[lo:lo + 4]) for lo in range(0, len(samples), 4)]
    assert not batches[0][0].is_cuda
    s = _solver(uc.config(), uc.params(), ListLoader(batches))
    for name in ("eval", "eval_keep", "eval_thresholds", "rank"):
        out = _walks_once(s, REPORTS[name])
    assert out["scores"].table.is_cuda


def test_the_sentiment_eval_walks_its_split_once():
    from mmda_amd import DeviceDataset, DeviceLoader
    cfg = orc.default_config(num_classes=1, vocab_size=80)
    ds = DeviceDataset.from_samples(uc.make_samples(), DEV)
    s = _solver(cfg, orc.synth_params(cfg, 9), DeviceLoader(ds, 4), task="sentiment")
    loss, acc, preds, truths = _walks_once(s, REPORTS["eval"])
    assert preds.shape == truths.shape == (len(ds),) and loss > 0 and s.last_sentiment is not None
    assert sorted(truths.tolist()) == sorted(ds.sentiment.cpu().tolist())
