"""The seven launches of mmda_amd/csrc/fused_rows.hip, each alone: ctypes mirrors of their argument structs, one plain torch
restatement per launch, the case table, the inputs and the bounds.  tests/test_gpu_fused_rows.py runs the cases on the GPU;
tests/test_fused_rows_cases_cpu.py proves the restatement against oracle/misa_oracle.py and the comparison sensitive.  Importing this
file needs neither a GPU nor the library.

Restatements.  ``RESTATE[launch](I, c, dt, given, mut) -> (out, ap)``: ``I`` the launch's input tensors (float32; the pre-fill of an
accumulated output is an input, ``pre_<name>``), ``c`` the case, ``dt`` the working precision.  ``out`` holds every tensor the launch
writes, intermediates included, with the sample axis explicit (``BDIM``); a buffer that is not in ``out`` is not touched.  ``given``
replaces a stored intermediate by another copy of it (the GPU's) as the input of the stages behind it, so that a comparison covers one
stage.  ``mut`` plants one of ``MISTAKES`` (the power check): those made inside a launch here, those made on its buffers in ``written``.

Bounds, per output tensor and per element, never from a GPU result (``bound``):
  * products of depth K: ``ap[name]`` = 2 K 2^-24 (|A| @ |B|) from the float64 operands, plus the bound of every earlier stage of the
    same launch carried through |B| (absent under ``given``: the stage then starts from exact inputs).  The sums of partials are depth-n
    products with ones; an elementwise chain of r roundings is 2 r 2^-24 |value|.
  * LayerNorm, softmax, sigmoid, the attention backward, the classification seed: four times REC[launch][name], the largest distance,
    over all cases, of the same restatement run in float32 on the CPU from its float64 run, in units of |float64 value| + the tensor's
    mean |value| (``dist``).  Four is the margin tests/dropout_cases.py uses for two correct fp32 implementations.  The numbers are
    constants of this file (``measure_rec`` makes them; the CPU test checks that they are current).
  * labels compare exactly; so does every buffer a case leaves untouched, against its pre-fill.

Inputs are independent random buffers (``inputs``), seeded per case and buffer, with a few saturating values planted (x6 of exactly 0
and 1, class scores of exactly 0 and 1, head biases of +-9).  With the seeds of the table, in float64, no class score lies within 1e-6
of the threshold (the nearest: 4.9e-5, B129-nb2) and no feed-forward pre-activation within 2e-6 of zero (the nearest: 9.9e-6,
M102-F64); a seed that is changed has to meet both again (``input_conditions``, asserted by the CPU test)."""
import ctypes as C

import numpy as np
import torch

from mmda_amd import _lib
from oracle import dropout_rng as drng

HS, NHEAD, S6, FFN_S, PG_SLOTS = 128, 2, 6, 32, 5
ACT_NONE, ACT_LEAKY, ACT_TANH = 0, 3, 4
U = 2.0 ** -24
F64, F32 = torch.float64, torch.float32
THRESHOLD = 0.35
RECON_SCALE = float(np.float32(0.7))

# ------------------------------------------------------------------------------------------------ ctypes mirrors (fused_rows.h)
_P, _I, _F, _U64 = C.c_void_p, C.c_int, C.c_float, C.c_uint64


class ClsTerm(C.Structure):
    _fields_ = [("g", _F), ("nw", _I), ("w", _F * 16)]


class FusedBwdC(C.Structure):
    _fields_ = [("B", _I), ("hs", _I), ("ncls", _I), ("nb", _I), ("tcp", _P), ("scores", _P), ("d_tcp", _P), ("d_scores", _P),
                ("d_logits", _P), ("p_cls", _F), ("seed", _U64), ("site_cls", _I), ("head_w", _P), ("d_hfused", _P),
                ("ln2", _lib.LnBwdArgs), ("pg_parts", _P), ("d_recon", _P), ("rec_wT", _P), ("rec_part", _P)]


class FusedBwdA(C.Structure):
    _fields_ = [("B", _I), ("hs", _I), ("nhead", _I), ("nb", _I), ("ln1", _lib.LnBwdArgs), ("ffn_parts", _P), ("n_parts", _I),
                ("d_x1", _P), ("d_attn_out", _P), ("out_wT", _P), ("d_ctx", _P), ("qkv", _P), ("probs", _P), ("d_qkv", _P),
                ("p_tf", _F), ("seed", _U64), ("site_attn", _I), ("in_wT", _P), ("d_recon", _P), ("rec_part", _P), ("rec_wT", _P),
                ("x6", _P), ("d_x6", _P), ("priv_wT", _P), ("sh_wT", _P), ("d_orig", _P), ("lnp", _lib.LnBwdArgs * 3),
                ("pg_parts", _P), ("dbg", _P), ("wait_flag", _P), ("wait_value", C.c_uint), ("wait_err", _P)]


class FusedFwdA(C.Structure):
    _fields_ = [("B", _I), ("hs", _I), ("nhead", _I), ("nb", _I), ("x6", _P), ("rec_w", _P), ("rec_b", _P), ("recon", _P),
                ("in_w", _P), ("in_b", _P), ("qkv", _P), ("ctx", _P), ("probs", _P), ("p_tf", _F), ("seed", _U64), ("site_attn", _I),
                ("out_w", _P), ("out_b", _P), ("attn_out", _P), ("ln1", _lib.LnArgs), ("orig", _P), ("d_recon", _P), ("d_orig", _P),
                ("recon_inv_n", _F), ("recon_scale", _F), ("split_recon", _I)]


class FusedFwdC(C.Structure):
    _fields_ = [("B", _I), ("hs", _I), ("ncls", _I), ("nb", _I), ("ln2", _lib.LnArgs), ("ffn_parts", _P), ("n_parts", _I), ("b2", _P),
                ("f2", _P), ("hfused", _P), ("head_w", _P), ("head_b", _P), ("logits", _P), ("threshold", _F), ("tcp", _P),
                ("scores", _P), ("labels", _P), ("p_cls", _F), ("seed", _U64), ("site_cls", _I), ("emo", _P), ("d_scores", _P),
                ("cls", ClsTerm)]


class FusedFfnFwd(C.Structure):
    _fields_ = [("M", _I), ("hs", _I), ("F", _I), ("S", _I), ("x1", _P), ("w1", _P), ("b1", _P), ("f1", _P), ("p", _F), ("seed", _U64),
                ("site", _I), ("w2", _P), ("parts", _P)]


class FusedFfnBwd(C.Structure):
    _fields_ = [("M", _I), ("hs", _I), ("F", _I), ("S", _I), ("d_f2", _P), ("f1", _P), ("gate_scale", _F), ("l2_wT", _P),
                ("d_f1", _P), ("l1_wT", _P), ("parts", _P)]


# the order of mmda_debug_fused_sizeof(which)
MIRRORS = (FusedFwdA, FusedFwdC, FusedBwdC, FusedBwdA, FusedFfnFwd, FusedFfnBwd, ClsTerm)


def debug_entries(lib):
    """The tests/-only entry points (not in _lib.SIGNATURES, as mmda_debug_set_fused_stamps is not), with their argument types."""
    sig = {"fwd_a": FusedFwdA, "ffn_fwd": FusedFfnFwd, "fwd_c": FusedFwdC, "bwd_c": FusedBwdC, "ffn_bwd": FusedFfnBwd, "bwd_a": FusedBwdA}
    out = {}
    for name, st in sig.items():
        fn = getattr(lib, "mmda_debug_fused_" + name)
        fn.restype, fn.argtypes = _I, [C.POINTER(st), _P]
        out[name] = fn
    fn = lib.mmda_debug_fused_pg_finish
    fn.restype, fn.argtypes = _I, [_P, _I, _I, C.POINTER(_P), C.POINTER(_P), _P]
    out["pg_finish"] = fn
    lib.mmda_debug_fused_sizeof.restype, lib.mmda_debug_fused_sizeof.argtypes = _I, [_I]
    out["sizeof"] = lib.mmda_debug_fused_sizeof
    return out


# ------------------------------------------------------------------------------------------------ the case table (literals only)
FOCAL = dict(g=2.0, w=(0.5, 1.0, 2.0, 3.0, 0.25, 1.5, 1.0, 0.75, 2.5, 1.25, 0.6, 1.8, 1.0, 0.9, 3.5, 0.4))


def _ac(name, B, nb, seed, p_tf=0.0, p_cls=0.0, seeds=False, cls=None, ncls=6, n_parts=64, rec_part=False, null=(), act=ACT_LEAKY,
        flag=False):
    return dict(name=name, B=B, nb=nb, seed=seed, p_tf=p_tf, p_cls=p_cls, seeds=seeds, cls=cls, ncls=ncls, n_parts=n_parts,
                rec_part=rec_part, null=null, act=act, flag=flag)


# Stretches A and C, both directions.  64 | 65 at nb = 1 and 128 | 129 at nb = 2: either side of nblk <= 64 (forward A's split);
# (1, 2), (5, 2), (129, 2) end on a one-sample workgroup, and every option appears at one of those three at least once.
# n_parts 0: ffn_parts absent.  null: arguments passed as NULL.  Bwd C at nb = 3: the one launcher that takes it (without rec_part).
AC_CASES = [
    _ac("B1-nb1", 1, 1, 1101, n_parts=64),
    _ac("B1-nb2", 1, 2, 1202, p_tf=0.1, p_cls=0.5, seeds=True, cls=FOCAL, ncls=3, n_parts=1, rec_part=True),
    _ac("B5-nb1", 5, 1, 1300, p_tf=0.25, p_cls=0.5, seeds=True, ncls=16, n_parts=3, rec_part=True, null=("d_tcp",)),
    _ac("B5-nb2-a", 5, 2, 1400, p_tf=0.1, p_cls=0.5, seeds=True, cls=FOCAL, ncls=1, n_parts=33, rec_part=True, act=ACT_TANH, flag=True),
    _ac("B5-nb2-b", 5, 2, 1500, ncls=3, n_parts=0, rec_part=True, null=("pg_parts",)),      # (rec_part without ffn_parts)
    _ac("B5-nb2-c", 5, 2, 1600, p_tf=0.25, seeds=True, ncls=16, n_parts=64, null=("d_scores",)),
    _ac("B5-nb2-d", 5, 2, 1700, p_cls=0.5, seeds=True, ncls=6, n_parts=3, rec_part=True, null=("d_tcp",)),
    _ac("B64-nb1", 64, 1, 1800, p_tf=0.1, p_cls=0.5, seeds=True, ncls=6, n_parts=3, rec_part=True),
    _ac("B65-nb1", 65, 1, 1900, p_tf=0.1, seeds=True, cls=FOCAL, ncls=3, n_parts=1),
    _ac("B128-nb2", 128, 2, 2000, p_tf=0.1, p_cls=0.5, seeds=True, ncls=6, n_parts=3, rec_part=True),
    _ac("B129-nb2", 129, 2, 2100, p_tf=0.1, p_cls=0.5, seeds=True, cls=FOCAL, ncls=16, n_parts=1, rec_part=True, act=ACT_TANH),
]
BWD_C_NB3 = _ac("B5-nb3", 5, 3, 2200, p_tf=0.1, p_cls=0.5, seeds=True, ncls=6)


def _ffn(M, F, p, scaled, seed):
    return dict(name=f"M{M}-F{F}-p{p}-{'scaled' if scaled else 'unit'}", M=M, F=F, p=p, scaled=scaled, seed=seed)


# 48 rows = one row block; 49 and 102 end on a padded block; 6 = one sample.  scaled: gate_scale = the fp32 1 / (1 - p), else 1.
FFN_CASES = [_ffn(6, 32, 0.0, False, 3100), _ffn(6, 64, 0.1, True, 3200), _ffn(48, 32, 0.1, True, 3300), _ffn(48, 64, 0.0, False, 3400),
             _ffn(49, 32, 0.0, True, 3500), _ffn(49, 64, 0.1, False, 3600), _ffn(102, 32, 0.1, False, 3700), _ffn(102, 64, 0.0, True, 3800),
             _ffn(6, 2048, 0.1, True, 3900)]

# null: (slot whose dgamma is NULL, slot whose dbeta is NULL).  15 | 16 | 17 and 127 | 128 | 129: either side of one pass of the
# sixteen threads of an output and of their 8 x 16 unrolled body; 200: one unrolled round and a tail; 256: two rounds.
def _pg(B, seed, null):
    return dict(name=f"B{B}", B=B, seed=seed, null=null)


PG_CASES = [_pg(1, 4001, (1, 3)), _pg(15, 4015, (0, 2)), _pg(16, 4016, (1, 3)), _pg(17, 4017, (2, 4)), _pg(127, 4127, (2, 4)),
            _pg(128, 4128, (3, 0)), _pg(129, 4129, (4, 1)), _pg(200, 4200, (0, 2)), _pg(256, 4256, (1, 3))]

CASES = {"fwd_a": AC_CASES, "fwd_c": AC_CASES, "bwd_c": AC_CASES + [BWD_C_NB3], "bwd_a": AC_CASES, "ffn_fwd": FFN_CASES,
         "ffn_bwd": FFN_CASES, "pg_finish": PG_CASES}

# REC[launch][tensor]: the float32 restatement's distance from float64 (dist), the largest over the launch's cases (measure_rec).  A
# float32 CPU run rounds differently on another processor (torch's GEMM kernels differ; the thread count changed nothing from 1 to 32):
# each figure is the larger of the measurements on the two kinds of host the suite runs on, which differ by up to 1.8 x (pg2: 1.40e-6
# and 2.48e-6; ln1_mean 8.2e-7 and 1.09e-6; d_scores 3.27e-6 and 1.85e-6).
REC = {
    "fwd_a": {"probs": 2.11e-06, "ctx": 1.85e-06, "x1": 2.95e-06, "ln1_mean": 1.09e-06, "ln1_rstd": 6.44e-07},
    "fwd_c": {"ln2_mean": 2.25e-07, "ln2_rstd": 8.05e-08, "hfused": 2.77e-07, "tcp": 3.27e-07, "scores": 8.81e-07, "d_scores": 3.27e-06},
    "bwd_c": {"d_x1": 8.76e-07, "d_f2": 1.14e-06, "pg0": 1.51e-06},
    "bwd_a": {"d_attn_out": 5.88e-07, "pg1": 8.6e-07, "d_qkv": 3.51e-06, "d_x6": 1.62e-06, "d_z": 1.95e-06, "pg2": 2.48e-06, "pg3": 2.18e-06,
              "pg4": 1.78e-06},
}

# the sample axis of every output (short workgroups, the power check); tensors without one are absent
BDIM = {"recon": 1, "d_recon": 1, "d_orig": 1, "qkv": 1, "probs": 0, "ctx": 1, "attn_out": 1, "x1": 1, "ln1_mean": 1, "ln1_rstd": 1,
        "f2": 1, "hfused": 0, "ln2_mean": 1, "ln2_rstd": 1, "logits": 0, "tcp": 0, "scores": 0, "labels": 0, "d_scores": 0,
        "d_logits": 0, "d_hfused": 0, "d_x1": 1, "d_f2": 1, "rec_part": 1, "pg0": 0, "pg1": 0, "pg2": 0, "pg3": 0, "pg4": 0,
        "d_attn_out": 1, "d_ctx": 1, "d_qkv": 1, "d_x6": 1, "d_z": 1}
# outputs that accumulate into what the buffer holds (everything else is a store); their pre-fill is the input pre_<name>
ACCUMULATED = {"bwd_a": ("d_x1", "d_x6", "d_orig"), "pg_finish": ("dgamma", "dbeta")}


# ------------------------------------------------------------------------------------------------ inputs
def _rnd(seed, k, shape, scale=1.0):
    g = torch.Generator().manual_seed(seed * 64 + k)
    return torch.randn(shape, generator=g) * scale


def _uni(seed, k, shape):
    g = torch.Generator().manual_seed(seed * 64 + k)
    return torch.rand(shape, generator=g)


def _w(seed, k, shape):
    return _rnd(seed, k, shape, 1.0 / float(shape[-1]) ** 0.5)


def _x6(seed, k, B):
    x = torch.sigmoid(_rnd(seed, k, (S6, B, HS)))
    x[0, 0, 3], x[4, B - 1, 77], x[2, B // 2, 127] = 0.0, 1.0, 1.0           # saturated sigmoids
    return x


def _probs(seed, k, B):
    return torch.softmax(_rnd(seed, k, (B, NHEAD, S6, S6), 2.0), -1)


def inv_n(B):
    return float(np.float32(1.0) / np.float32(3 * B * HS))


def inputs(launch, c):
    """name -> float32 tensor: every input buffer of the case, independent of the others, and the pre-fills of accumulated outputs"""
    s = c["seed"]
    if launch == "pg_finish":
        B = c["B"]
        return dict(pg=_rnd(s, 0, (B, PG_SLOTS, 2, HS)), pre_dgamma=_rnd(s, 1, (PG_SLOTS, HS)), pre_dbeta=_rnd(s, 2, (PG_SLOTS, HS)))
    if launch == "ffn_fwd":
        M, F = c["M"], c["F"]
        return dict(x1=_rnd(s, 0, (M, HS)), w1=_w(s, 1, (F, HS)), b1=_rnd(s, 2, (F,), 0.1), w2=_w(s, 3, (HS, F)))
    if launch == "ffn_bwd":
        M, F = c["M"], c["F"]
        f1 = torch.relu(_rnd(s, 5, (M, F)))                   # about half exact zeros, as relu and the dropout leave them
        f1[0, 0], f1[M - 1, F - 1], f1[M // 2, 7] = 0.0, 0.0, 0.0
        return dict(d_f2=_rnd(s, 4, (M, HS)), f1=f1, l2_wT=_w(s, 6, (F, HS)), l1_wT=_w(s, 7, (HS, F)))
    B, ncls = c["B"], c["ncls"]
    NC = 6 + ncls
    if launch == "fwd_a":
        return dict(x6=_x6(s, 0, B), rec_w=_w(s, 1, (3, HS, HS)), rec_b=_rnd(s, 2, (3, HS), 0.1), in_w=_w(s, 3, (3 * HS, HS)) * 3.0,
                    in_b=_rnd(s, 4, (3 * HS,), 0.1), out_w=_w(s, 5, (HS, HS)), out_b=_rnd(s, 6, (HS,), 0.1),
                    ln1_g=1.0 + _rnd(s, 7, (HS,), 0.1), ln1_b=_rnd(s, 8, (HS,), 0.1), orig=_rnd(s, 9, (3, B, HS)))
    if launch == "fwd_c":
        hb = _rnd(s, 15, (NC,), 0.1)
        hb[1], hb[NC - 1] = 9.0, -9.0                          # a confidence and a class score that nearly saturate
        I = dict(x1=_rnd(s, 10, (S6, B, HS)), b2=_rnd(s, 11, (HS,), 0.1), ln2_g=1.0 + _rnd(s, 12, (HS,), 0.1), ln2_b=_rnd(s, 13, (HS,), 0.1),
                 head_w=_w(s, 14, (NC, S6 * HS)), head_b=hb, emo=(_uni(s, 16, (B, ncls)) < 0.4).float())
        if c["n_parts"]:
            I["parts"] = _rnd(s, 17, (c["n_parts"], S6, B, HS), 1.0 / float(c["n_parts"]) ** 0.5)
        else:
            I["f2"] = _rnd(s, 18, (S6, B, HS))
        return I
    if launch == "bwd_c":
        sc = _uni(s, 21, (B, ncls))
        sc[0, 0], sc[B - 1, ncls - 1] = 1.0, 0.0               # saturated class scores (the last wins where both are one element)
        return dict(tcp=_uni(s, 20, (B, 6)), scores=sc, d_tcp=_rnd(s, 22, (B, 6)), d_scores=_rnd(s, 23, (B, ncls)),
                    head_w=_w(s, 24, (NC, S6 * HS)), x1=_rnd(s, 25, (S6, B, HS)), f2=_rnd(s, 26, (S6, B, HS)),
                    ln2_g=1.0 + _rnd(s, 27, (HS,), 0.1), ln2_mean=_rnd(s, 28, (S6, B), 0.1), ln2_rstd=0.5 + _uni(s, 29, (S6, B)),
                    d_recon=_rnd(s, 30, (3, B, HS)), rec_wT=_w(s, 31, (3, HS, HS)))
    if launch == "bwd_a":
        I = dict(pre_d_x1=_rnd(s, 40, (S6, B, HS)), x6=_x6(s, 41, B), attn_out=_rnd(s, 42, (S6, B, HS)), ln1_g=1.0 + _rnd(s, 43, (HS,), 0.1),
                 ln1_mean=_rnd(s, 44, (S6, B), 0.1), ln1_rstd=0.5 + _uni(s, 45, (S6, B)), pre_d_x6=_rnd(s, 46, (S6, B, HS)),
                 out_wT=_w(s, 47, (HS, HS)), qkv=_rnd(s, 48, (S6, B, 3 * HS)), probs=_probs(s, 49, B), in_wT=_w(s, 50, (HS, 3 * HS)),
                 d_recon=_rnd(s, 51, (3, B, HS)), rec_wT=_w(s, 52, (3, HS, HS)), rec_part=_rnd(s, 53, (3, B, HS)),
                 priv_wT=_w(s, 54, (3, HS, HS)), sh_wT=_w(s, 55, (HS, HS)), pre_d_orig=_rnd(s, 56, (3, B, HS)), z=_rnd(s, 57, (3, B, HS)),
                 lnp_g=1.0 + _rnd(s, 58, (3, HS), 0.1), lnp_mean=_rnd(s, 59, (3, B), 0.1), lnp_rstd=0.5 + _uni(s, 60, (3, B)))
        if c["n_parts"]:
            I["parts"] = _rnd(s, 61, (c["n_parts"], S6, B, HS), 1.0 / float(c["n_parts"]) ** 0.5)
        return I
    raise KeyError(launch)


# ------------------------------------------------------------------------------------------------ pieces
def _mask(p, seed, site, shape, dt, shift=0):
    n = int(np.prod(shape))
    return torch.from_numpy(drng.drop_mul(p, seed, site, np.arange(n, dtype=np.uint64) + np.uint64(shift)).reshape(shape)).to(dt)


def _ap(K, A, Bt, bias=None):
    """2 K 2^-24 (|A| @ |Bt|^T + |bias|), Bt (N, K)"""
    t = A.abs() @ Bt.abs().transpose(-1, -2)
    return 2.0 * K * U * (t + bias.abs() if bias is not None else t)


def _thru(bnd, Bt):
    """an operand's bound carried through the product with Bt (N, K)"""
    return bnd @ Bt.abs().transpose(-1, -2)


def _nb(launch, name, ref):
    """the bound of a tensor without a closed form: 4 REC (|value| + the tensor's mean |value|)"""
    r = ref.double()
    return (4.0 * REC[launch].get(name, 0.0) * (r.abs() + r.abs().mean())).to(ref.dtype)


def dist(a, ref):
    """the largest |a - ref| in units of |ref| + mean |ref| (an all-zero reference: 0 where equal, inf otherwise)"""
    a, ref = a.double(), ref.double()
    d = (a - ref).abs()
    den = ref.abs() + ref.abs().mean()
    if d.numel() == 0:
        return 0.0
    q = torch.where(den > 0, d / den.clamp_min(1e-300), torch.where(d == 0, torch.zeros_like(d), torch.full_like(d, float("inf"))))
    return float(q.max())


def _act(act, z):
    if act == ACT_LEAKY:
        return torch.where(z > 0, z, 0.01 * z)
    return torch.tanh(z) if act == ACT_TANH else z


def _dact(act, z):
    if act == ACT_LEAKY:
        return torch.where(z > 0, torch.ones_like(z), torch.full_like(z, 0.01))
    return 1.0 - torch.tanh(z) ** 2 if act == ACT_TANH else torch.ones_like(z)


def _ln_fwd(x, g, b):
    mean = x.mean(-1)
    d = x - mean[..., None]
    rstd = 1.0 / torch.sqrt((d * d).mean(-1) + 1e-5)
    return d * rstd[..., None] * g + b, mean, rstd


def _ln_bwd(dy, x, g, mean, rstd):
    """(d of the normalised row's input, the row's dgamma terms, its dbeta terms)"""
    xh = (x - mean[..., None]) * rstd[..., None]
    gdy = dy * g
    s1, s2 = gdy.mean(-1, keepdim=True), (gdy * xh).mean(-1, keepdim=True)
    return rstd[..., None] * (gdy - s1 - xh * s2), dy * xh, dy


def _pg_rows(dg, db, B, nb):
    """(rows, B, HS) terms -> (B, 2, HS): the sum over a workgroup's rows in the slot of its first sample, zeros in the others"""
    t = torch.stack((dg.sum(0), db.sum(0)), 1)                      # (B, 2, HS) per sample
    out = torch.zeros_like(t)
    for b0 in range(0, B, nb):
        out[b0] = t[b0:b0 + nb].sum(0)
    return out


def _heads(z):                                                      # (6, B, E) -> (B, NHEAD, 6, hd)
    return z.reshape(S6, -1, NHEAD, HS // NHEAD).permute(1, 2, 0, 3)


def _unheads(z):                                                    # (B, NHEAD, 6, hd) -> (6, B, E)
    return z.permute(2, 0, 1, 3).reshape(S6, -1, HS)


def _shift(mut, width):
    return width if mut == "drop_row" else 0


# ------------------------------------------------------------------------------------------------ the seven launches
def fwd_a(I, c, dt=F64, given=None, mut=None):
    g, T = given or {}, {k: v.to(dt) for k, v in I.items()}
    B, seed, x6 = c["B"], c["seed"], T["x6"]
    out, ap = {}, {}
    rec_w = T["rec_w"][[1, 0, 2]] if mut == "swap_rec" else T["rec_w"]
    s = x6[:3] + x6[3:]
    out["recon"] = torch.einsum("ibk,ink->ibn", s, rec_w) + T["rec_b"][:, None, :]
    ap["recon"] = 2.0 * (HS + 1) * U * (torch.einsum("ibk,ink->ibn", s.abs(), rec_w.abs()) + T["rec_b"].abs()[:, None, :])
    if c["seeds"]:
        k = 2.0 * inv_n(B) * RECON_SCALE
        out["d_recon"] = k * (g.get("recon", out["recon"]).to(dt) - T["orig"])
        out["d_orig"] = -out["d_recon"]
        ap["d_recon"] = 8.0 * U * out["d_recon"].abs() + (0.0 if "recon" in g else k * ap["recon"])
        ap["d_orig"] = ap["d_recon"]
    out["qkv"] = x6 @ T["in_w"].t() + T["in_b"]
    ap["qkv"] = _ap(HS, x6, T["in_w"], T["in_b"])
    q, k_, v = (_heads(t) for t in g.get("qkv", out["qkv"]).to(dt).split(HS, -1))
    att = torch.softmax(q @ k_.transpose(-1, -2) / 8.0, -1)
    out["probs"] = att.permute(1, 0, 2, 3).reshape(att.shape) if mut == "probs_sb" else att
    out["ctx"] = _unheads((att * _mask(c["p_tf"], seed, drng.SITE_ATTN, att.shape, dt, _shift(mut, S6))) @ v)
    ctx = g.get("ctx", out["ctx"]).to(dt)
    out["attn_out"] = ctx @ T["out_w"].t() + T["out_b"]
    ap["attn_out"] = _ap(HS, ctx, T["out_w"], T["out_b"]) + (0.0 if "ctx" in g else _thru(_nb("fwd_a", "ctx", out["ctx"]), T["out_w"]))
    ao = g.get("attn_out", out["attn_out"]).to(dt)
    x = x6 + ao * _mask(c["p_tf"], seed, drng.SITE_DROP1, ao.shape, dt, _shift(mut, HS))
    out["x1"], out["ln1_mean"], out["ln1_rstd"] = _ln_fwd(x, T["ln1_g"], T["ln1_b"])
    return out, ap


def ffn_fwd(I, c, dt=F64, given=None, mut=None):
    g, T = given or {}, {k: v.to(dt) for k, v in I.items()}
    M, F = c["M"], c["F"]
    mask = _mask(c["p"], c["seed"], drng.SITE_FFN, (M, F), dt, _shift(mut, F))
    out, ap = {}, {}
    out["f1"] = torch.relu(T["x1"] @ T["w1"].t() + T["b1"]) * mask
    ap["f1"] = _ap(HS + 1, T["x1"], T["w1"], T["b1"]) * mask
    f1 = g.get("f1", out["f1"]).to(dt)
    w2 = T["w2"].reshape(HS, F // FFN_S, FFN_S).permute(1, 0, 2)                            # (slices, HS, S)
    f1s = f1.reshape(M, F // FFN_S, FFN_S).permute(1, 0, 2)                                 # (slices, M, S)
    out["parts"] = f1s @ w2.transpose(-1, -2)
    a1 = ap["f1"].reshape(M, F // FFN_S, FFN_S).permute(1, 0, 2)
    ap["parts"] = _ap(FFN_S, f1s, w2) + (0.0 if "f1" in g else _thru(a1, w2))
    return out, ap


def pre_activation(I, c):
    """float64 x1 W1^T + b1 of a feed-forward case (the kink condition)"""
    return I["x1"].double() @ I["w1"].double().t() + I["b1"].double()


def cls_seed(s, y, cls, B):
    """the classification loss's seed d_scores (loss_terms.h: bce_plain / cls_term, over B)"""
    if cls is None:
        return (s - y) / torch.clamp(s * (1 - s), min=1e-12) / B
    gm, w = cls["g"], torch.tensor(cls["w"][:s.shape[1]], dtype=s.dtype)
    lp, lq = torch.clamp(torch.log(s), min=-100.0), torch.clamp(torch.log1p(-s), min=-100.0)
    q = 1 - s
    d = -w * y * (q ** gm / torch.clamp(s, min=1e-12) - gm * q ** (gm - 1) * lp) \
        + (1 - y) * (s ** gm / torch.clamp(q, min=1e-12) - gm * s ** (gm - 1) * lq)
    return d / B


def fwd_c(I, c, dt=F64, given=None, mut=None):
    g, T = given or {}, {k: v.to(dt) for k, v in I.items()}
    B, seed, ncls = c["B"], c["seed"], c["ncls"]
    out, ap = {}, {}
    if c["n_parts"]:
        n = c["n_parts"] - (1 if mut == "partial_fewer" else 0)
        out["f2"] = T["parts"][:n].sum(0) + (0.0 if mut == "no_b2" else T["b2"])
        ap["f2"] = 2.0 * (c["n_parts"] + 1) * U * (T["parts"].abs().sum(0) + T["b2"].abs())
        f2 = g.get("f2", out["f2"]).to(dt)
    else:
        f2 = T["f2"]
    x = T["x1"] + f2 * _mask(c["p_tf"], seed, drng.SITE_DROP2, f2.shape, dt, _shift(mut, HS))
    y, out["ln2_mean"], out["ln2_rstd"] = _ln_fwd(x, T["ln2_g"], T["ln2_b"])
    out["hfused"] = y.permute(1, 0, 2).reshape(B, S6 * HS)
    h = g.get("hfused", out["hfused"]).to(dt)
    hw, hb = T["head_w"][:6 + ncls], T["head_b"][:6 + ncls]
    out["logits"] = h @ hw.t() + hb
    ap["logits"] = _ap(S6 * HS, h, hw, hb) + (0.0 if "hfused" in g else _thru(_nb("fwd_c", "hfused", out["hfused"]), hw))
    z = g.get("logits", out["logits"]).to(dt)
    out["tcp"] = torch.sigmoid(z[:, :6])
    zc = z[:, 6:]
    out["scores"] = torch.sigmoid(zc * _mask(c["p_cls"], seed, drng.SITE_CLS, zc.shape, dt, _shift(mut, ncls)))
    s = g.get("scores", out["scores"]).to(dt)
    out["labels"] = (s > THRESHOLD).to(dt)
    if c["seeds"]:
        out["d_scores"] = cls_seed(s, T["emo"][:, :ncls], c["cls"], B)
    return out, ap


def bwd_c(I, c, dt=F64, given=None, mut=None):
    g, T = given or {}, {k: v.to(dt) for k, v in I.items()}
    B, seed, nb, ncls = c["B"], c["seed"], c["nb"], c["ncls"]
    out, ap = {}, {}
    t, s = T["tcp"], T["scores"][:, :ncls]
    dt6 = torch.zeros_like(t) if "d_tcp" in c["null"] else T["d_tcp"] * t * (1 - t)
    dsc = torch.zeros_like(s) if "d_scores" in c["null"] else \
        T["d_scores"][:, :ncls] * s * (1 - s) * _mask(c["p_cls"], seed, drng.SITE_CLS, s.shape, dt, _shift(mut, ncls))
    out["d_logits"] = torch.cat((dt6, dsc), 1)
    ap["d_logits"] = 8.0 * U * out["d_logits"].abs()
    dl = g.get("d_logits", out["d_logits"]).to(dt)
    hw = T["head_w"][:6 + ncls]
    out["d_hfused"] = dl @ hw
    ap["d_hfused"] = _ap(6 + ncls, dl, hw.t()) + (0.0 if "d_logits" in g else _thru(ap["d_logits"], hw.t()))
    dy = g.get("d_hfused", out["d_hfused"]).to(dt).reshape(B, S6, HS).permute(1, 0, 2)
    mask = _mask(c["p_tf"], seed, drng.SITE_DROP2, dy.shape, dt, _shift(mut, HS))
    dxp, dg, db = _ln_bwd(dy, T["x1"] + T["f2"] * mask, T["ln2_g"], T["ln2_mean"], T["ln2_rstd"])
    out["d_x1"], out["d_f2"] = dxp, dxp * mask
    if "pg_parts" not in c["null"]:
        out["pg0"] = _pg_rows(dg, db, B, nb)
    if c["rec_part"]:
        wT = T["rec_wT"][[1, 0, 2]] if mut == "swap_rec" else T["rec_wT"]
        out["rec_part"] = torch.einsum("ibk,ink->ibn", T["d_recon"], wT)
        ap["rec_part"] = 2.0 * HS * U * torch.einsum("ibk,ink->ibn", T["d_recon"].abs(), wT.abs())
    return out, ap


def gate_scale(c):
    """the fp32 1 / (1 - p) of a scaled feed-forward case (what the step passes with dropout on), else 1"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(c["p"]))) if c["scaled"] else 1.0


def ffn_bwd(I, c, dt=F64, given=None, mut=None):
    g, T = given or {}, {k: v.to(dt) for k, v in I.items()}
    M, F = c["M"], c["F"]
    gs = gate_scale(c)
    gate = (T["f1"] > 0).to(dt) * gs
    out, ap = {}, {}
    out["d_f1"] = (T["d_f2"] @ T["l2_wT"].t()) * gate
    ap["d_f1"] = _ap(HS + 1, T["d_f2"], T["l2_wT"]) * gate
    d1 = g.get("d_f1", out["d_f1"]).to(dt).reshape(M, F // FFN_S, FFN_S).permute(1, 0, 2)
    w1 = T["l1_wT"].reshape(HS, F // FFN_S, FFN_S).permute(1, 0, 2)
    out["parts"] = d1 @ w1.transpose(-1, -2)
    a1 = ap["d_f1"].reshape(M, F // FFN_S, FFN_S).permute(1, 0, 2)
    ap["parts"] = _ap(FFN_S, d1, w1) + (0.0 if "d_f1" in g else _thru(a1, w1))
    return out, ap


def bwd_a(I, c, dt=F64, given=None, mut=None):
    g, T = given or {}, {k: v.to(dt) for k, v in I.items()}
    B, seed, nb, p = c["B"], c["seed"], c["nb"], c["p_tf"]
    out, ap = {}, {}
    d_x1 = T["pre_d_x1"]
    if c["n_parts"]:
        n = c["n_parts"] - (1 if mut == "partial_fewer" else 0)
        d_x1 = out["d_x1"] = T["pre_d_x1"] + T["parts"][:n].sum(0)
        ap["d_x1"] = 2.0 * (c["n_parts"] + 1) * U * (T["parts"].abs().sum(0) + T["pre_d_x1"].abs())
        d_x1 = g.get("d_x1", d_x1).to(dt)
    x6 = T["x6"]
    mask = _mask(p, seed, drng.SITE_DROP1, x6.shape, dt, _shift(mut, HS))
    dxp, dg, db = _ln_bwd(d_x1, x6 + T["attn_out"] * mask, T["ln1_g"], T["ln1_mean"], T["ln1_rstd"])
    out["d_attn_out"] = dxp * mask
    if "pg_parts" not in c["null"]:
        out["pg1"] = _pg_rows(dg, db, B, nb)
    dao = g.get("d_attn_out", out["d_attn_out"]).to(dt)
    out["d_ctx"] = dao @ T["out_wT"].t()
    ap["d_ctx"] = _ap(HS, dao, T["out_wT"]) + (0.0 if "d_attn_out" in g else _thru(_nb("bwd_a", "d_attn_out", out["d_attn_out"]), T["out_wT"]))
    dc = _heads(g.get("d_ctx", out["d_ctx"]).to(dt))
    q, k_, v = (_heads(t) for t in T["qkv"].split(HS, -1))
    P = T["probs"].permute(1, 0, 2, 3).reshape(T["probs"].shape) if mut == "probs_sb" else T["probs"]
    mul = _mask(p, seed, drng.SITE_ATTN, P.shape, dt, _shift(mut, S6))
    dP = (dc @ v.transpose(-1, -2)) * mul
    dS = P * (dP - (dP * P).sum(-1, keepdim=True))
    out["d_qkv"] = torch.cat((_unheads(dS @ k_ / 8.0), _unheads(dS.transpose(-1, -2) @ q / 8.0), _unheads((P * mul).transpose(-1, -2) @ dc)), -1)
    dq = g.get("d_qkv", out["d_qkv"]).to(dt)
    if c["rec_part"]:
        rec = T["rec_part"]
        rec = rec[[1, 0, 2]] if mut == "swap_rec" else rec
    else:
        rec = torch.einsum("ibk,ink->ibn", T["d_recon"], T["rec_wT"][[1, 0, 2]] if mut == "swap_rec" else T["rec_wT"])
    out["d_x6"] = (T["pre_d_x6"] + dxp + dq @ T["in_wT"].t() + torch.cat((rec, rec), 0)) * (x6 * (1 - x6))
    d6 = g.get("d_x6", out["d_x6"]).to(dt)
    out["d_orig"] = T["pre_d_orig"] + torch.einsum("ibk,ink->ibn", d6[:3], T["priv_wT"]) + d6[3:] @ T["sh_wT"].t()
    ap["d_orig"] = 2.0 * (2 * HS + 1) * U * (torch.einsum("ibk,ink->ibn", d6[:3].abs(), T["priv_wT"].abs()) + d6[3:].abs() @ T["sh_wT"].abs().t()
                                             + T["pre_d_orig"].abs())
    if "d_x6" not in g:
        b6 = _nb("bwd_a", "d_x6", out["d_x6"])
        ap["d_orig"] = ap["d_orig"] + torch.einsum("ibk,ink->ibn", b6[:3], T["priv_wT"].abs()) + b6[3:] @ T["sh_wT"].abs().t()
    do = g.get("d_orig", out["d_orig"]).to(dt)
    dzp, dgp, dbp = _ln_bwd(do, _act(c["act"], T["z"]), T["lnp_g"][:, None, :], T["lnp_mean"], T["lnp_rstd"])
    out["d_z"] = dzp * _dact(c["act"], T["z"])
    if "pg_parts" not in c["null"]:
        for i in range(3):
            out[f"pg{2 + i}"] = torch.stack((dgp[i], dbp[i]), 1)
    return out, ap


def pg_finish(I, c, dt=F64, given=None, mut=None):
    T = {k: v.to(dt) for k, v in I.items()}
    B = c["B"] - (1 if mut == "partial_fewer" else 0)
    s = T["pg"][:B].sum(0)                                                                 # (5, 2, HS)
    a = 2.0 * (c["B"] + 1) * U * T["pg"].abs().sum(0)
    out = {"dgamma": T["pre_dgamma"] + s[:, 0], "dbeta": T["pre_dbeta"] + s[:, 1]}
    ap = {"dgamma": a[:, 0] + 2.0 * (c["B"] + 1) * U * T["pre_dgamma"].abs(), "dbeta": a[:, 1] + 2.0 * (c["B"] + 1) * U * T["pre_dbeta"].abs()}
    return out, ap                                       # (the rows of the case's NULL slots are not written: see written)


RESTATE = {"fwd_a": fwd_a, "ffn_fwd": ffn_fwd, "fwd_c": fwd_c, "bwd_c": bwd_c, "ffn_bwd": ffn_bwd, "bwd_a": bwd_a, "pg_finish": pg_finish}
# the stored intermediates of each launch that outlive it, in stage order (`given`)
INTERMEDIATES = {"fwd_a": ("recon", "qkv", "ctx", "attn_out"), "ffn_fwd": ("f1",), "fwd_c": ("f2", "hfused", "logits", "scores"),
                 "bwd_c": ("d_logits", "d_hfused"), "ffn_bwd": ("d_f1",), "bwd_a": ("d_x1", "d_attn_out", "d_ctx", "d_qkv", "d_x6", "d_orig"),
                 "pg_finish": ()}


def bound(launch, name, ref, ap):
    """per-element bound of output `name` whose float64 value is `ref`"""
    if name == "labels":
        return torch.zeros_like(ref, dtype=F64)
    b = ap[name] if name in ap else _nb(launch, name, ref)
    return b.double().expand_as(ref) if torch.is_tensor(b) else torch.full_like(ref, float(b), dtype=F64)


def excess(launch, got, ref, ap):
    """{name: the largest |got - ref| / bound} (0 / 0 = 0, x / 0 = inf, NaN = inf) over the tensors of `ref`"""
    out = {}
    for name, r in ref.items():
        d = (got[name].double() - r.double()).abs()
        b = bound(launch, name, r, ap)
        q = torch.where(d == 0, torch.zeros_like(d), d / b.clamp_min(1e-300))
        q = torch.where(torch.isnan(d), torch.full_like(q, float("inf")), q)
        out[name] = float(q.max()) if q.numel() else 0.0
    return out


# ------------------------------------------------------------------------------------------------ conditions and recorded distances
def input_conditions(launch, c):
    """{condition: distance}: class scores from the threshold (forward C), feed-forward pre-activations from zero (feed-forward
    forward), both in float64"""
    I = inputs(launch, c)
    if launch == "fwd_c":
        return {"threshold": float((RESTATE[launch](I, c)[0]["scores"] - THRESHOLD).abs().min())}
    if launch == "ffn_fwd":
        return {"kink": float(pre_activation(I, c).abs().min())}
    return {}


CONDITION_FLOOR = {"threshold": 1e-6, "kink": 2e-6}


def measure_rec(launch):
    """{tensor: the largest dist(float32 run, float64 run) over the launch's cases} for the tensors without a closed-form bound"""
    rec = {}
    for c in CASES[launch]:
        I = inputs(launch, c)
        o64, ap = RESTATE[launch](I, c, F64)
        o32, _ = RESTATE[launch](I, c, F32)
        for name, r in o64.items():
            if name not in ap and name != "labels":
                rec[name] = max(rec.get(name, 0.0), dist(o32[name], r))
    return rec


# ------------------------------------------------------------------------------------------------ the power check's mistakes
MISTAKES = ("swap_rec", "short_last", "drop_row", "probs_sb", "no_b2", "partial_fewer", "pg_not_zeroed", "acc_for_store", "store_for_acc",
            "ncls6")


def applies(launch, c, mut):
    """does the planted mistake change anything the launch of this case computes?"""
    ac = launch in ("fwd_a", "fwd_c", "bwd_c", "bwd_a")
    if mut == "swap_rec":
        return launch == "fwd_a" or (launch == "bwd_c" and c["rec_part"]) or launch == "bwd_a"
    if mut == "short_last":
        return ac and c["nb"] == 2 and c["B"] % 2 == 1
    if mut == "drop_row":
        if launch == "ffn_fwd":
            return c["p"] > 0
        if launch in ("fwd_a", "bwd_a"):
            return c["p_tf"] > 0
        if launch == "fwd_c":
            return c["p_tf"] > 0 or (c["p_cls"] > 0 and c["B"] > 1)
        return launch == "bwd_c" and (c["p_tf"] > 0 or (c["p_cls"] > 0 and c["B"] > 1 and "d_scores" not in c["null"]))
    if mut == "probs_sb":
        return launch in ("fwd_a", "bwd_a") and c["B"] > 1
    if mut == "no_b2":
        return launch == "fwd_c" and c["n_parts"] > 0
    if mut == "partial_fewer":
        return launch == "pg_finish" or (launch in ("fwd_c", "bwd_a") and c["n_parts"] > 0)
    if mut == "pg_not_zeroed":
        return launch in ("bwd_c", "bwd_a") and c["nb"] >= 2 and c["B"] >= 2 and "pg_parts" not in c["null"]
    if mut == "acc_for_store":
        return launch != "pg_finish"                     # (every output of pg_finish accumulates)
    if mut == "store_for_acc":
        return launch in ACCUMULATED
    if mut == "ncls6":
        return (launch == "bwd_c" or (launch == "fwd_c" and c["B"] > 1)) and c["ncls"] != 6
    return False


def written(launch, c, I, dt=F64, given=None, mut=None):
    """(bufs, ap): what every buffer the launch writes holds afterwards, the planted mistake `mut` included.  Stores start from a NaN
    pre-fill, accumulated outputs from their pre_<name> input; pg_finish leaves the rows of its NULL slots alone (dropped here)."""
    out, ap = RESTATE[launch](I, c, dt, given, mut if mut in ("swap_rec", "drop_row", "probs_sb", "no_b2", "partial_fewer") else None)
    acc = ACCUMULATED.get(launch, ())
    pre = {k: (I["pre_" + k].to(dt) if k in acc else torch.full_like(v, float("nan"))) for k, v in out.items()}
    if mut == "ncls6":
        # a kernel that takes ncls as 6 walks the class buffers of the case with the rows of six classes: the same memory, re-strided
        # (what lies behind a buffer reads as noise), and what it writes lands at the six-class offsets of the real buffers
        B = c["B"]
        gen = torch.Generator().manual_seed(c["seed"])

        def six(t, lead, width):                                     # (lead, n + width) buffer read as (lead, 6 + width)
            flat = t.flatten()
            need = lead * (6 + width)
            flat = torch.cat((flat, torch.randn(max(0, need - flat.numel()), generator=gen).to(flat.dtype)))[:need]
            return flat.reshape(lead, 6 + width)
        I6 = dict(I)
        for k, lead, width in (("emo", B, 0), ("scores", B, 0), ("d_scores", B, 0), ("head_b", 1, 6)):
            if k in I:
                I6[k] = six(I[k], lead, width).reshape(-1) if k == "head_b" else six(I[k], lead, width)
        hw = I["head_w"]
        I6["head_w"] = torch.cat((hw, torch.randn(max(0, 12 - hw.shape[0]), hw.shape[1], generator=gen) * 0.04))[:12]
        o6, _ = RESTATE[launch](I6, dict(c, ncls=6, cls=None if c["cls"] is None else dict(c["cls"])), dt, given)
        for k, v in out.items():
            if o6[k].shape == v.shape:
                out[k] = o6[k]
            else:
                flat = torch.full((v.numel(),), float("nan"), dtype=v.dtype)
                m = min(v.numel(), o6[k].numel())
                flat[:m] = o6[k].flatten()[:m]
                out[k] = flat.reshape(v.shape)
        return out, ap
    if mut == "short_last":
        for k, v in out.items():
            v.select(BDIM[k], c["B"] - 1).copy_(pre[k].select(BDIM[k], c["B"] - 1))
    if mut == "pg_not_zeroed":
        for k in out:
            if k in ("pg0", "pg1"):
                out[k][1::c["nb"]] = pre[k][1::c["nb"]]
    if mut == "acc_for_store":
        k = next(k for k in out if k not in acc)
        out[k] = out[k] + pre[k]
    if mut == "store_for_acc":
        k = next(k for k in out if k in acc)
        out[k] = out[k] - pre[k]
    if launch == "pg_finish":
        keep_g = [k for k in range(PG_SLOTS) if k != c["null"][0]]
        keep_b = [k for k in range(PG_SLOTS) if k != c["null"][1]]
        out = {"dgamma": out["dgamma"][keep_g], "dbeta": out["dbeta"][keep_b]}
        ap = {"dgamma": ap["dgamma"][keep_g], "dbeta": ap["dbeta"][keep_b]}
    return out, ap
