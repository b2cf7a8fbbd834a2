"""Writes tests/golden/losses_bits.npz: the inputs of a fixed list of head and small-loss launches (cls, conf, recon, the one-launch
mmda_loss_misc, heads forward / backward) and the bits each of them produced.

Run once, on the GPU, at the commit whose bits are to be kept (``python tests/golden/gen_losses_bits.py [--out FILE]``);
tests/test_gpu_losses_bits.py replays the same calls -- replay() below, through ctypes and ``mmda_amd.ops`` only -- on the build under
test and asks for equal bits.  The stored inputs come from numpy's generator once and are read back ever after; the inputs of the two
larger recon cases are an exact integer formula of the element index, and the outputs of the largest are kept as wrap-around sums of
their bit patterns.

Shapes: the smallest that reach every branch of a launch's loop.  cls: 6 elements, 258 (the 256-thread stride loop takes a second
trip), 7 classes.  conf: 1, 65, 257 rows (within a wave, across waves, past the block).  recon: 3 B D = 3, 258 and 16386 (65 blocks
wanted, 64 given), and one strided call (three launches).  misc: every (with_conf, conf_grads, use_conf) at n_recon = 2049 (two recon
workgroups), then n_recon = 1, 2048 and 64 * 2048 + 5 (the capped grid's stride loop takes a second trip).  heads: 1 and 37 samples,
6 and 7 classes, dropout off and on.

The misc launch adds into d_scores from two roles with atomics: from zero the two orders give the same bits, so d_scores / d_tcp start
at zero there; every buffer with one writer starts from non-zero values."""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "losses_bits.npz")

DEV = "cuda:0"
CLS_SHAPES = ((1, 6), (43, 6), (41, 7))
CLS_SCALE, FOCAL_GAMMA = 0.7, 2.0
CONF_B, CONF_SCALE = (1, 65, 257), 0.3
RECON_SHAPES = ((1, 1), (2, 43))                  # (B, D) of the stored contiguous calls: 3 B D = 3, 258
RECON_FORMULA = (2, 2731)                         # 3 B D = 16386, inputs by formula
RECON_STRIDED = (2, 43, 2 * 43 + 8)               # B, D, stride
RECON_SCALE = 0.6
MISC_B, MISC_NCLS = 5, 6
MISC_COMBOS = tuple((w, g, u) for w in (0, 1) for g in (0, 1) for u in (0, 1))
MISC_N = (1, 2048)                                # at the default switches (1, 1, 1); 2049: MISC_COMBOS
MISC_LARGE_N = 64 * 2048 + 5
MISC_W = dict(L1=0.37, L2=1.21, dw=0.3, sw=0.8, rw=0.6, cw=0.9, conf_scale=0.9, recon_scale=0.6)
HEAD_SHAPES = ((1, 6), (37, 6), (37, 7))
HEAD_DROP = ((0.0, 0, 0), (0.5, 20261, 7))        # (p, seed, site)
THRESHOLD = 0.35


def _heads(rng, B, ncls, ntcp=None):
    """scores and tcp in (0, 1), 0/1 labels with a positive in every class column (ConfidNet divides by their count)"""
    f32 = lambda x: np.ascontiguousarray(x, dtype=np.float32)
    sig = lambda x: 1.0 / (1.0 + np.exp(-x))
    s = f32(sig(rng.standard_normal((B, ncls))))
    t = f32(sig(rng.standard_normal((B, ntcp or ncls))))
    y = f32(rng.uniform(size=(B, ncls)) > 0.6)
    y[0] = 1.0
    assert (np.count_nonzero(y, axis=0) > 0).all()
    return s, t, y


def make_inputs(seed=21):
    rng = np.random.default_rng(seed)
    f32 = lambda x: np.ascontiguousarray(x, dtype=np.float32)
    inp = {}
    for B, n in CLS_SHAPES:
        s, _, y = _heads(rng, B, n)
        if B > 2:                                 # both clamps of the logarithm and of the gradient's denominator
            s[1, 0], s[2, 1], y[1, 0], y[2, 1] = 0.0, 1.0, 1.0, 0.0
        k = f"cls{B}x{n}"
        inp[f"{k}::s"], inp[f"{k}::y"] = s, y
        inp[f"{k}::pre"] = f32(rng.standard_normal((B, n)))
        inp[f"{k}::w"] = f32(rng.uniform(0.5, 3.0, n))
    for B in CONF_B:
        k = f"conf{B}"
        inp[f"{k}::s"], inp[f"{k}::t"], inp[f"{k}::y"] = _heads(rng, B, 6)
        inp[f"{k}::pre_s"], inp[f"{k}::pre_t"] = f32(rng.standard_normal((B, 6))), f32(rng.standard_normal((B, 6)))
    for tag, n in [(f"recon{B}x{D}", 3 * B * D) for B, D in RECON_SHAPES] + [("recon_strided", 3 * RECON_STRIDED[2])]:
        for name in ("rec", "org", "pre_rec", "pre_org"):
            inp[f"{tag}::{name}"] = f32(rng.standard_normal(n))
    inp["misc::s"], inp["misc::t"], inp["misc::y"] = _heads(rng, MISC_B, MISC_NCLS)
    inp["misc::w"] = f32(rng.uniform(0.5, 3.0, MISC_NCLS))
    for name in ("rec", "org", "pre_rec", "pre_org"):
        inp[f"misc::{name}"] = f32(rng.standard_normal(2049))      # (the smaller n_recon take a prefix)
    for B, n in HEAD_SHAPES:
        k = f"heads{B}x{n}"
        inp[f"{k}::logits"] = f32(1.5 * rng.standard_normal((B, 6 + n)))
        inp[f"{k}::dtcp"], inp[f"{k}::dscores"] = f32(rng.standard_normal((B, 6))), f32(rng.standard_normal((B, n)))
    return inp


def formula_inputs(n):
    """rec, org, pre_rec, pre_org of a larger recon case on the device: small integers from the element index, times a power of two
    (exact in fp32)"""
    i = torch.arange(n, dtype=torch.int64, device=DEV)
    h = lambda mul, add, mod: ((i * mul + add) % 4294967296 >> 7) % mod
    rec = (h(2654435761, 1, 4097) - 2048).to(torch.float32) / 1024.0
    org = (h(2246822519, 2, 4097) - 2048).to(torch.float32) / 1024.0
    pre_rec = (h(3266489917, 3, 513) - 256).to(torch.float32) / 4096.0
    pre_org = (h(668265263, 4, 513) - 256).to(torch.float32) / 4096.0
    return rec, org, pre_rec, pre_org


def bit_sums(*tensors):
    """the 64-bit wrap-around sum of each tensor's int32 bit patterns"""
    return np.array([int(t.view(torch.int32).to(torch.int64).sum().item()) for t in tensors], dtype=np.int64)


def misc_call(lib, s, t, y, d_scores, d_tcp, with_conf, conf_grads, use_conf, rec, org, d_rec, d_org, L, opts=None, conf_scale=None,
              recon_scale=None):
    """mmda_loss_misc (opts: mmda_loss_misc_opts) over n_recon = rec.numel() elements, with MISC_W's weights"""
    from mmda_amd import _lib
    w = MISC_W
    args = [_lib.ptr(s), _lib.ptr(t), _lib.ptr(y), s.shape[0], s.shape[1], _lib.ptr(d_scores), _lib.ptr(d_tcp), with_conf, conf_grads,
            w["conf_scale"] if conf_scale is None else conf_scale, _lib.ptr(rec), _lib.ptr(org), rec.numel(),
            w["recon_scale"] if recon_scale is None else recon_scale, _lib.ptr(d_rec), _lib.ptr(d_org), _lib.ptr(L), w["dw"], w["sw"],
            w["rw"], w["cw"], use_conf]
    if opts is None:
        _lib.check(lib.mmda_loss_misc(*args, _lib.stream_ptr()), "mmda_loss_misc")
    else:
        _lib.check(lib.mmda_loss_misc_opts(*args, opts, _lib.stream_ptr()), "mmda_loss_misc_opts")


def replay(inp):
    """Every launch of the list on the current build; {name: array} of what it left behind."""
    from mmda_amd import _lib, ops
    lib = _lib.load()
    st = _lib.stream_ptr()
    p = _lib.ptr
    dev = lambda name: torch.from_numpy(np.ascontiguousarray(inp[name])).to(DEV)
    scalar = lambda v: torch.full((1,), v, device=DEV)
    out = {}

    def keep(tag, **tensors):
        torch.cuda.synchronize()
        for k, t in tensors.items():
            out[f"{tag}::{k}"] = t.detach().cpu().numpy().copy()

    # ---- mmda_loss_cls / mmda_loss_cls_opts: value onto 0.25 and gradient onto `pre`; the gradient alone; the value alone
    for B, n in CLS_SHAPES:
        k = f"cls{B}x{n}"
        s, y = dev(f"{k}::s"), dev(f"{k}::y")
        o = _lib.cls_opts(tuple(float(v) for v in inp[f"{k}::w"]), FOCAL_GAMMA)
        for tag, call in (("plain", lambda l, d: lib.mmda_loss_cls(p(s), p(y), B, n, CLS_SCALE, p(l), p(d), st)),
                          ("opts", lambda l, d: lib.mmda_loss_cls_opts(p(s), p(y), B, n, CLS_SCALE, p(l), p(d), o, st))):
            loss, ds = scalar(0.25), dev(f"{k}::pre")
            _lib.check(call(loss, ds), "mmda_loss_cls")
            keep(f"{k}::{tag}", loss=loss, ds=ds)
            ds = dev(f"{k}::pre")
            _lib.check(call(None, ds), "mmda_loss_cls")
            keep(f"{k}::{tag}::no_loss", ds=ds)
            loss = scalar(0.25)
            _lib.check(call(loss, None), "mmda_loss_cls")
            keep(f"{k}::{tag}::no_ds", loss=loss)

    # ---- mmda_loss_conf
    for B in CONF_B:
        k = f"conf{B}"
        s, t, y = dev(f"{k}::s"), dev(f"{k}::t"), dev(f"{k}::y")
        loss, ds, dt = scalar(0.25), dev(f"{k}::pre_s"), dev(f"{k}::pre_t")
        _lib.check(lib.mmda_loss_conf(p(s), p(t), p(y), B, 6, CONF_SCALE, p(loss), p(ds), p(dt), st), "mmda_loss_conf")
        keep(k, loss=loss, ds=ds, dt=dt)
        loss = scalar(0.25)
        _lib.check(lib.mmda_loss_conf(p(s), p(t), p(y), B, 6, CONF_SCALE, p(loss), None, None, st), "mmda_loss_conf")
        keep(f"{k}::no_grads", loss=loss)

    # ---- mmda_loss_recon: contiguous (one launch) and strided (three)
    def recon(tag, B, D, stride, rec, org, d_rec, d_org):
        loss = scalar(0.25)
        _lib.check(lib.mmda_loss_recon(p(rec), p(org), stride, B, D, RECON_SCALE, p(loss), p(d_rec), p(d_org), st), "mmda_loss_recon")
        keep(tag, loss=loss, d_rec=d_rec, d_org=d_org)

    for B, D in RECON_SHAPES:
        k = f"recon{B}x{D}"
        recon(k, B, D, B * D, *(dev(f"{k}::{name}") for name in ("rec", "org", "pre_rec", "pre_org")))
    B, D = RECON_FORMULA
    recon(f"recon{B}x{D}", B, D, B * D, *formula_inputs(3 * B * D))
    B, D, stride = RECON_STRIDED                  # (the gaps between the tensors keep what they held)
    recon("recon_strided", B, D, stride, *(dev(f"recon_strided::{name}") for name in ("rec", "org", "pre_rec", "pre_org")))

    # ---- mmda_loss_misc
    s, t, y = dev("misc::s"), dev("misc::t"), dev("misc::y")

    def misc(tag, n, w, g, u, opts=None, large=False):
        src = formula_inputs(n) if large else [dev(f"misc::{name}")[:n].clone() for name in ("rec", "org", "pre_rec", "pre_org")]
        rec, org, d_rec, d_org = src
        d_scores, d_tcp = torch.zeros_like(s), torch.zeros_like(t)
        L = torch.zeros(8, device=DEV)
        L[1], L[2] = MISC_W["L1"], MISC_W["L2"]
        misc_call(lib, s, t, y, d_scores, d_tcp, w, g, u, rec, org, d_rec, d_org, L, opts)
        keep(tag, d_scores=d_scores, d_tcp=d_tcp, L=L[:6])
        if large:
            out[f"{tag}::recon_bit_sums"] = bit_sums(d_rec, d_org)
        else:
            keep(tag, d_rec=d_rec, d_org=d_org)

    for w, g, u in MISC_COMBOS:
        misc(f"misc2049::w{w}g{g}u{u}", 2049, w, g, u)
    for n in MISC_N:
        misc(f"misc{n}", n, 1, 1, 1)
    misc("misc_large", MISC_LARGE_N, 1, 1, 1, large=True)
    misc("misc2049::opts", 2049, 1, 1, 1, opts=_lib.cls_opts(tuple(float(v) for v in inp["misc::w"]), FOCAL_GAMMA))

    # ---- heads forward and backward
    for B, n in HEAD_SHAPES:
        k = f"heads{B}x{n}"
        logits, dtcp, dscores = dev(f"{k}::logits"), dev(f"{k}::dtcp"), dev(f"{k}::dscores")
        for drop_p, seed, site in HEAD_DROP:
            tag = f"{k}::p{drop_p}"
            tcp, sc, lab = ops.heads_fwd(logits, n, THRESHOLD, drop_p, seed, site)
            keep(f"{tag}::fwd", tcp=tcp, scores=sc, labels=lab)
            keep(f"{tag}::bwd", dlogits=ops.heads_bwd(tcp, sc, dtcp, dscores, n, drop_p, seed, site))
            keep(f"{tag}::bwd_no_dtcp", dlogits=ops.heads_bwd(tcp, sc, None, dscores, n, drop_p, seed, site))
    return out


# what the fixture leaves out, because the test derives it from what it keeps: the recon role does not see the conf switches or the
# classification criterion, so every n_recon = 2049 call leaves the d_recon / d_orig of the first
MISC_FIRST = "misc2049::w0g0u0"
DERIVED = tuple(f"misc2049::{tag}::{k}" for tag in [f"w{w}g{g}u{u}" for w, g, u in MISC_COMBOS[1:]] + ["opts"] for k in ("d_rec", "d_org"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=FIXTURE)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    inp = make_inputs()
    out = replay(inp)
    again = replay(inp)                                   # the launches are deterministic, or nothing could be recorded
    for k, x in out.items():
        assert x.tobytes() == again[k].tobytes(), k
    for k in DERIVED:
        assert out[k].tobytes() == out[MISC_FIRST + k[k.rindex("::"):]].tobytes(), k
    arrays = {"in::" + k: x for k, x in inp.items()}
    arrays.update({"out::" + k: x for k, x in out.items() if k not in DERIVED})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **arrays)
    print(f"{a.out}: {len(arrays)} arrays, {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
