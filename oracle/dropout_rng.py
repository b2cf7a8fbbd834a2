"""Host restatement of the counter-based dropout masks.  TEST INFRASTRUCTURE ONLY (see oracle/misa_oracle.py).

The kernels never store a mask: every site recomputes its multiplier from (seed, site, element index) with ``rng_u32`` / ``drop_mul``
of ``mmda_amd/csrc/common.h``.  The same two functions in numpy -- uint64 arithmetic modulo 2^64, the fp32 comparison ``u < p``, the
kept value the fp32 quotient ``1 / (1 - p)`` widened to double -- give the masks of a training step on the host, so that step has an
exact reference (``misa_oracle.loss_and_grads(..., masks=site_masks(...))``).

Site ids are ``misa.hip``'s; the element index of each site is read from the kernel that applies it ("Dropout sites").
"""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

SITE_ATTN, SITE_DROP1, SITE_FFN, SITE_DROP2, SITE_CLS, SITE_DISC = 1, 2, 3, 4, 5, 6
SITES = {"attn": SITE_ATTN, "drop1": SITE_DROP1, "ffn": SITE_FFN, "drop2": SITE_DROP2, "cls": SITE_CLS, "disc": SITE_DISC}

_GOLD = np.uint64(0x9E3779B97F4A7C15)
_STRIDE = np.uint64(0xD6E8FEB86659FD93)
_MIX1 = np.uint64(0xFF51AFD7ED558CCD)
_MIX2 = np.uint64(0xC4CEB9FE1A85EC53)
_S33, _S16, _S8 = np.uint64(33), np.uint64(16), np.uint64(8)


def rng_u32(seed: int, site: int, idx) -> np.ndarray:
    """murmur3 fmix64 of seed + GOLD (site + 1) + idx STRIDE; bits 16..47 of the result (common.h: rng_u32)."""
    idx = np.asarray(idx, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed & 0xFFFFFFFFFFFFFFFF) + _GOLD * np.uint64(site + 1) + idx * _STRIDE
        z = z ^ (z >> _S33); z = z * _MIX1
        z = z ^ (z >> _S33); z = z * _MIX2
        z = z ^ (z >> _S33)
    return ((z >> _S16) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def drop_mul(p: float, seed: int, site: int, idx) -> np.ndarray:
    """Inverted-dropout multiplier of element ``idx``: 0 where u < p, else the fp32 1 / (1 - p), as float64 (common.h: drop_mul)."""
    idx = np.asarray(idx, dtype=np.uint64)
    p32 = np.float32(p)
    if p32 <= np.float32(0.0):
        return np.ones(idx.shape, np.float64)
    u = (rng_u32(seed, site, idx) >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    keep = np.float32(1.0) / (np.float32(1.0) - p32)
    return np.where(u < p32, np.float64(0.0), np.float64(keep))


def mask(p: float, seed: int, site: int, shape) -> np.ndarray:
    """The multipliers of elements 0 .. prod(shape) - 1 in flat index order, reshaped to ``shape`` (float64)."""
    n = int(np.prod(shape, dtype=np.int64))
    return drop_mul(p, seed, site, np.arange(n, dtype=np.uint64)).reshape(shape)


def site_shapes(cfg, B: int) -> Dict[str, tuple]:
    """{site name: shape}; the flat index of each shape is the kernels' element index (six tokens, two heads, 2048 hidden units)."""
    from .misa_oracle import FFN_DIM, NHEAD
    hs = cfg.hidden_size
    return {"attn": (B, NHEAD, 6, 6),             # ((b nhead + h) S + i) S + j
            "drop1": (6, B, hs),                  # row n + col, row = s B + b
            "ffn": (6, B, FFN_DIM),               # m F + n, m = s B + b
            "drop2": (6, B, hs),                  # row n + col, row = s B + b BEFORE LayerNorm 2 permutes its output rows
            "cls": (B, cfg.num_classes),          # b ncls + k: the classifier logits only
            "disc": (3, B, hs)}                   # flat over the discriminator's hidden rows of text, visual, acoustic


def site_masks(cfg, B: int, seed: int, p_tf: float, p_cls: float) -> Dict[str, torch.Tensor]:
    """All six masks of one training step: ``p_tf`` (the fusion layer's dropout) at attn / drop1 / ffn / drop2, ``p_cls``
    (config.dropout) at cls / disc.  float64 tensors; the oracle casts them to its working precision."""
    p = {"attn": p_tf, "drop1": p_tf, "ffn": p_tf, "drop2": p_tf, "cls": p_cls, "disc": p_cls}
    return {k: torch.from_numpy(mask(p[k], seed, SITES[k], shp)) for k, shp in site_shapes(cfg, B).items()}


def ones_masks(cfg, B: int) -> Dict[str, torch.Tensor]:
    """Masks that drop nothing and scale nothing."""
    return {k: torch.ones(shp, dtype=torch.float64) for k, shp in site_shapes(cfg, B).items()}
