"""Writes tests/golden/optim_bits.npz: the inputs of a fixed list of optimizer launches and the bits each of them produced.

Run once, on the GPU, at the commit whose bits are to be kept (``python tests/golden/gen_optim_bits.py [--out FILE]``);
tests/test_gpu_optim_bits.py replays the same calls -- replay() below, through ``mmda_amd.ops`` only -- on the build under test and
asks for equal bits.  The stored inputs come from numpy's generator once and are read back ever after; the large case's inputs are
an exact integer formula of the element index, and its outputs are kept as wrap-around sums of their bit patterns.

Shapes: the smallest that reach every branch of a launch's loop.  Dense: 1031 floats = 257 quads (two blocks) + a tail of 3, then a
tail alone (3) and a quad alone (4).  Rows: a width of 75 quads (a lane takes two) and a width of 7 (the scalar form).  Runs: the
range list of tests/test_gpu_frozen.py.  Large: more quads than the capped grid has lanes, so the stride loop takes a second trip."""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "optim_bits.npz")

DEV = "cuda:0"
LR, CLIP, SCALE = 1e-3, 1.0, 0.5                 # gradients lie in +-3: scaled by 0.5, the clamp at 1 bites on a third of them
DENSE_N = (1031, 3, 4)
ROWS = ((37, 300), (37, 7))
RUNS_N = 1063
LARGE_N = 2048 * 256 * 4 + 1031


def run_ranges(n):
    """tests/test_gpu_frozen.py::_op_ranges: lengths 1, 3, 4, 5 at begins = 1, 2, 3, 0 mod 4, a whole quad, a long run, a run that
    ends at n; the first float is frozen"""
    r = [(1, 1), (6, 3), (11, 4), (16, 5), (24, 4), (33, 1000), (1037, 2), (1041, n - 1041 - 9), (n - 7, 7)]
    assert r[-2][1] > 0 and r[-1][0] + r[-1][1] == n
    return r


def make_inputs(seed=20):
    rng = np.random.default_rng(seed)
    f32 = lambda x: np.ascontiguousarray(x, dtype=np.float32)
    grad = lambda *s: f32(rng.uniform(-3.0, 3.0, s))
    inp = {}
    for n in DENSE_N:
        inp[f"dense{n}::p"] = f32(rng.standard_normal(n))
        for s in (1, 2, 3):
            inp[f"dense{n}::g{s}"] = grad(n)
        inp[f"dense{n}::acc"] = grad(n)
        inp[f"dense{n}::sq"] = f32(rng.uniform(0.0, 1e-2, n))
    for V, D in ROWS:
        inp[f"rows{D}::p"] = f32(rng.standard_normal((V, D)))
        inp[f"rows{D}::g"] = grad(V, D)
        inp[f"rows{D}::m"] = f32(0.1 * rng.standard_normal((V, D)))
        inp[f"rows{D}::v"] = f32(rng.uniform(0.0, 1e-2, (V, D)))
        mask = (rng.uniform(size=V) < 0.5).astype(np.uint8)
        assert 0 < int(mask.sum()) < V
        inp[f"rows{D}::mask"] = mask
    n = RUNS_N
    inp["runs::p"] = f32(rng.standard_normal(n))
    inp["runs::g"] = grad(n)
    inp["runs::acc"] = grad(n)
    inp["runs::m"] = f32(0.1 * rng.standard_normal(n))
    inp["runs::v"] = f32(rng.uniform(0.0, 1e-2, n))
    return inp


def large_inputs(n):
    """p, acc, g, m, v of the large case on the device: small integers from the element index, times a power of two (exact in fp32)"""
    i = torch.arange(n, dtype=torch.int64, device=DEV)
    h = lambda mul, add, mod: ((i * mul + add) % 4294967296 >> 7) % mod
    p = (h(2654435761, 1, 4097) - 2048).to(torch.float32) / 2048.0
    acc = (h(2246822519, 2, 6145) - 3072).to(torch.float32) / 1024.0
    g = (h(3266489917, 3, 6145) - 3072).to(torch.float32) / 1024.0
    m = (h(668265263, 4, 513) - 256).to(torch.float32) / 4096.0
    v = h(374761393, 5, 1025).to(torch.float32) / 65536.0
    return p, acc, g, m, v


def bit_sums(*tensors):
    """the 64-bit wrap-around sum of each tensor's int32 bit patterns"""
    return np.array([int(t.view(torch.int32).to(torch.int64).sum().item()) for t in tensors], dtype=np.int64)


def replay(inp):
    """Every launch of the list on the current build; {name: array} of what it left behind."""
    from mmda_amd import ops
    dev = lambda name: torch.from_numpy(np.ascontiguousarray(inp[name])).to(DEV)
    out = {}

    def keep(tag, names, tensors):
        torch.cuda.synchronize()
        for k, t in zip(names, tensors):
            out[f"{tag}::{k}"] = t.detach().cpu().numpy().copy()

    for n in DENSE_N:
        p0, acc, sq0 = dev(f"dense{n}::p"), dev(f"dense{n}::acc"), dev(f"dense{n}::sq")
        g = [dev(f"dense{n}::g{s}") for s in (1, 2, 3)]
        # three steps from m = v = 0 (the step number changes the scalars), then one with no clamp and no scale
        p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
        for s in (1, 2, 3):
            ops.clamp_adam(p, g[s - 1], m, v, LR, s, clip=CLIP, grad_scale=SCALE)
        keep(f"dense{n}::adam3", "PMV", (p, m, v))
        ops.clamp_adam(p, g[0], m, v, LR, 4)
        keep(f"dense{n}::adam4_noclip", "PMV", (p, m, v))
        p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
        for s in (1, 2, 3):
            ops.clamp_adam_sum(p, acc, g[s - 1], m, v, LR, s, clip=CLIP, grad_scale=SCALE)
        keep(f"dense{n}::sum3", "PMV", (p, m, v))
        ops.clamp_adam_sum(p, acc, g[0], m, v, LR, 4)
        keep(f"dense{n}::sum4_noclip", "PMV", (p, m, v))
        a = torch.full_like(p0, float("nan"))            # first = a plain copy: nothing of this survives
        ops.grad_accumulate(a, g[0], first=True)
        keep(f"dense{n}::accumulate1", ("acc",), (a,))
        ops.grad_accumulate(a, g[1])
        ops.grad_accumulate(a, g[2])
        keep(f"dense{n}::accumulate3", ("acc",), (a,))
        p, sq = p0.clone(), sq0.clone()
        for s in (1, 2, 3):
            ops.clamp_rmsprop(p, g[s - 1], sq, 1e-2, clip=CLIP, grad_scale=SCALE)
        keep(f"dense{n}::rmsprop3", ("P", "square_avg"), (p, sq))

    for V, D in ROWS:
        p, g, m, v, mask = (dev(f"rows{D}::{k}") for k in ("p", "g", "m", "v", "mask"))
        for want in (0, 1):
            ops.clamp_adam_rows(p, g, m, v, mask, want, LR, 3, clip=CLIP, grad_scale=SCALE)
            keep(f"rows{D}::want{want}", "PMV", (p, m, v))

    n = RUNS_N
    runs = ops.runs_table(run_ranges(n), n, DEV)
    p0, g, acc, m0, v0 = (dev(f"runs::{k}") for k in ("p", "g", "acc", "m", "v"))
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    ops.clamp_adam_runs(p, g, m, v, runs, LR, 3, clip=CLIP, grad_scale=SCALE)
    keep("runs::adam", "PMV", (p, m, v))
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    ops.clamp_adam_sum_runs(p, acc, g, m, v, runs, LR, 2, clip=CLIP, grad_scale=SCALE)
    keep("runs::sum", "PMV", (p, m, v))
    p, sq = p0.clone(), v0.clone()
    ops.clamp_rmsprop_runs(p, g, sq, runs, 1e-2, clip=CLIP, grad_scale=SCALE)
    keep("runs::rmsprop", ("P", "square_avg"), (p, sq))
    table, k, items = runs                                # a slice of the table that starts at its fourth run
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    ops.clamp_adam_runs(p, g, m, v, (table[3:], k - 3, items - int(table[3, 2])), LR, 1, clip=CLIP)
    keep("runs::adam_slice", "PMV", (p, m, v))

    p0, acc, g, m0, v0 = large_inputs(LARGE_N)
    assert 0 < int((g.abs() * SCALE > CLIP).sum()) < LARGE_N
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    ops.clamp_adam(p, g, m, v, LR, 3, clip=CLIP, grad_scale=SCALE)
    torch.cuda.synchronize()
    out["large::adam::bit_sums"] = bit_sums(p, m, v)
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    ops.clamp_adam_sum(p, acc, g, m, v, LR, 3, clip=CLIP, grad_scale=SCALE)
    torch.cuda.synchronize()
    out["large::sum::bit_sums"] = bit_sums(p, m, v)
    return out


# what the fixture leaves out, because the test derives it from what it keeps: after the want = 0 pass the rows with mask 0 hold
# their final bits and the rows with mask 1 still hold the inputs
DERIVED = tuple(f"rows{D}::want0::{k}" for _, D in ROWS for k in "PMV")


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
    arrays = {"in::" + k: x for k, x in inp.items()}
    arrays.update({"out::" + k: x for k, x in out.items() if k not in DERIVED})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **arrays)
    print(f"{a.out}: {len(arrays)} arrays, {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
