"""Files of the second stage (reference src/utils/tools.py:52-73): the per-sample fused hidden vectors ``h`` and the ConfidNet confidence
``tcp`` of a split, as ``InferencePass`` produces them, saved in the working directory under the reference's names --
``hidden_vectors/MISA_{dataset}.pt``, or ``MISA_C_{dataset}.pt`` when ``args.use_confidNet``; the tcp files likewise under
``tcp_vectors/`` (the reference leaves them as ``# TODO: Implement tcp saving``).

The reference's ``save_hidden`` works out the ``_C_`` name and then saves under the plain one, so its own ``load_hidden`` cannot find a
ConfidNet run's file; here the save goes where the load reads.  Loading is ``weights_only=True``: these files hold tensors only.
"""
import os

import torch


def _file(args, folder, dataset):
    return os.path.join(folder, f"MISA_C_{dataset}.pt" if getattr(args, "use_confidNet", False) else f"MISA_{dataset}.pt")


def _save(args, tensor, folder, dataset):
    os.makedirs(folder, exist_ok=True)
    torch.save(tensor.detach().cpu(), _file(args, folder, dataset))


def _load(args, folder, dataset):
    return torch.load(_file(args, folder, dataset), weights_only=True)


def save_hidden(args, tensor, dataset=''):
    _save(args, tensor, "hidden_vectors", dataset)


def load_hidden(args, dataset=''):
    return _load(args, "hidden_vectors", dataset)


def save_tcp(args, tensor, dataset=''):
    _save(args, tensor, "tcp_vectors", dataset)


def load_tcp(args, dataset=''):
    return _load(args, "tcp_vectors", dataset)


def save_scaling(args, scaling, dataset=''):
    """A ``Scaling`` (mmda_amd/reliability.py) beside the tcp files, under ``scaling/``: what ``Scaling.save`` writes."""
    os.makedirs("scaling", exist_ok=True)
    scaling.save(_file(args, "scaling", dataset))


def load_scaling(args, dataset='', device="cpu"):
    from ..reliability import Scaling
    return Scaling.load(_file(args, "scaling", dataset), device)
