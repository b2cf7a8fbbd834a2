"""Writes tests/golden/embed_rows_bits.npz: the bits that a fixed list of embedding-rows calls left behind -- the plain scatter-add, the
segment sum, the sparse and the deferred row optimizer, over the short and the sort form of an id list.

Run once, on the GPU, at the commit whose bits are to be kept (``python tests/golden/gen_embed_rows_bits.py [--out FILE]``; the
fixture was recorded at the commit before the rows code moved into embed_rows.hip);
tests/test_gpu_embed_rows_bits.py replays the same calls -- replay() below, through ``mmda_amd.ops`` only -- on the build under test
and asks for equal bits.  Nothing of the inputs is stored: tests/embed_rows_cases.py makes the lists and the values from literals and
exact integer formulas.  Kept per call: the table rows the list touches (and their moments) in full, and a wrap-around sum of the bit
patterns of each whole array, which is all that is kept of the 20 000-row table."""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
FIXTURE = os.path.join(HERE, "embed_rows_bits.npz")
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)
import embed_rows_cases as ec  # noqa: E402

DEV = "cuda:0"
LR, CLIP, SCALE = 1e-3, 1.0, 0.05
SHORT = ((ec.SMALL_V, ec.WIDE_D), (ec.SMALL_V, ec.NARROW_D))
LONG = ((ec.SMALL_V, ec.WIDE_D), (ec.LARGE_V, ec.NARROW_D))
SEG_V = 64


def bit_sums(*tensors):
    """the 64-bit wrap-around sum of each tensor's int32 bit patterns"""
    return np.array([int(t.view(torch.int32).to(torch.int64).sum().item()) for t in tensors], dtype=np.int64)


def replay():
    """Every call of the list on the current build; {name: array} of what it left behind."""
    from mmda_amd import ops
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    out = {}

    def keep(tag, names, tensors, touched=None):
        """bit sums of the whole arrays and, touched given, those rows in full"""
        torch.cuda.synchronize()
        out[f"{tag}::bit_sums"] = bit_sums(*tensors)
        if touched is not None:
            idx = torch.from_numpy(np.asarray(touched, dtype=np.int64)).to(DEV)
            for k, t in zip(names, tensors):
                out[f"{tag}::{k}"] = t[idx].detach().cpu().numpy().copy()

    def fresh(V, D, salt):
        return tuple(dev(x) for x in ec.table(V, D, salt))

    def dense_once(tag, V, D, ids, rows, lengths, touched):
        """one deferred update of a fresh state (window 2), then the flush: dense Adam over the whole table"""
        p, m, v = fresh(V, D, 40)
        state = ops.embed_deferred_state(V, 2, DEV)
        ops.embed_rows_dense_adam(p, m, v, state, ids, rows, LR, 3, lengths=lengths, clip=CLIP, grad_scale=SCALE)
        keep(f"{tag}::update", "PMV", (p, m, v))
        ops.embed_rows_flush(p, m, v, state)
        keep(f"{tag}::flushed", "PMV", (p, m, v), touched)

    # ---- short form
    lengths_np = np.array(ec.SHORT_LENGTHS, dtype=np.int32)
    lengths = dev(lengths_np)
    for V, D in SHORT:
        tag = f"short{D}"
        ids_np, ids2_np = ec.short_ids(V), ec.short_ids(V, second=True)
        ids, ids2 = dev(ids_np), dev(ids2_np)
        n = ids_np.size
        rows = [dev(ec.grad_rows(n, D, 10 + s)) for s in range(3)]
        # the plain scatter-add into a gradient that already holds something (it accumulates); no lengths at this entry
        dW = dev(ec.values((V, D), 30))
        ops.embed_scatter_add(dW, dev(ec.in_table(ids_np, V)), rows[0])
        keep(f"{tag}::add", ("dW",), (dW,), ec.touched_rows(ec.in_table(ids_np, V)))
        for name, ln, ln_np in (("ragged", lengths, lengths_np), ("full", None, None)):
            if D == ec.WIDE_D and name == "full":
                continue                                               # (the wide table without lengths: the scatter-add above)
            p, m, v = fresh(V, D, 40)
            ops.embed_rows_sparse_adam(p, m, v, ids, rows[0], LR, 3, lengths=ln, clip=CLIP, grad_scale=SCALE)
            keep(f"{tag}::sparse_{name}", "PMV", (p, m, v), ec.touched_rows(ids_np, ln_np, V))
            if D == ec.NARROW_D:
                dense_once(f"{tag}::dense_{name}", V, D, ids, rows[0], ln, ec.touched_rows(ids_np, ln_np, V))
        if D != ec.WIDE_D:
            continue
        # deferred: three updates with window 2 (the second flushes first), a catch-up of the second list, a last flush; the Adam step
        # number skips one
        p, m, v = fresh(V, D, 40)
        state = ops.embed_deferred_state(V, 2, DEV)
        ops.embed_rows_dense_adam(p, m, v, state, ids, rows[0], LR, 1, lengths=lengths, clip=CLIP, grad_scale=SCALE)
        keep(f"{tag}::deferred::update1", "PMV", (p, m, v))
        ops.embed_rows_catch_up(p, m, v, state, ids2, lengths=lengths)
        keep(f"{tag}::deferred::catch_up", "PMV", (p, m, v))
        ops.embed_rows_dense_adam(p, m, v, state, ids2, rows[1], LR, 2, lengths=lengths, clip=CLIP, grad_scale=SCALE)
        assert state.flushed == 1
        keep(f"{tag}::deferred::update2", "PMV", (p, m, v))
        ops.embed_rows_dense_adam(p, m, v, state, ids, rows[2], LR, 4, lengths=lengths, clip=CLIP, grad_scale=SCALE)
        keep(f"{tag}::deferred::update3", "PMV", (p, m, v))
        ops.embed_rows_flush(p, m, v, state)
        both = np.union1d(ec.touched_rows(ids_np, lengths_np, V), ec.touched_rows(ids2_np, lengths_np, V))
        keep(f"{tag}::deferred::flushed", "PMV", (p, m, v), both)
        out[f"{tag}::deferred::row_step"] = state.row_step.cpu().numpy().copy()

    # ---- sort form through the segment sum (overwrites the rows it touches)
    for name, neg in (("plain", False), ("negatives", True)):
        ids_np = ec.segment_ids(neg)
        dW = dev(ec.values((SEG_V, ec.SEG_D), 31))
        ops.embed_segment_sum(dW, dev(ids_np), dev(ec.grad_rows(ids_np.size, ec.SEG_D, 13)))
        keep(f"seg::{name}", ("dW",), (dW,), ec.touched_rows(ids_np))

    # ---- sort form at the length threshold: the scatter-add and both row optimizers
    lengths_np = ec.long_lengths()
    lengths = dev(lengths_np)
    for V, D in LONG:
        tag = f"long{V}"
        ids_np = ec.long_ids(V)
        ids = dev(ids_np)
        rows = dev(ec.grad_rows(ids_np.size, D, 14))
        full = V == ec.SMALL_V                                         # the large table: bit sums only
        dW = dev(ec.values((V, D), 32))
        ops.embed_scatter_add(dW, dev(ec.in_table(ids_np, V)), rows)
        keep(f"{tag}::add", ("dW",), (dW,), ec.touched_rows(ec.in_table(ids_np, V)) if full else None)
        touched = ec.touched_rows(ids_np, lengths_np, V) if full else None
        p, m, v = fresh(V, D, 40)
        ops.embed_rows_sparse_adam(p, m, v, ids, rows, LR, 3, lengths=lengths, clip=CLIP, grad_scale=SCALE)
        keep(f"{tag}::sparse", "PMV", (p, m, v), touched)
        dense_once(f"{tag}::dense", V, D, ids, rows, lengths, touched)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=FIXTURE)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    out = replay()
    again = replay()                                      # the calls are deterministic, or nothing could be recorded
    for k, x in out.items():
        assert x.tobytes() == again[k].tobytes(), k
    arrays = {"out::" + k: x for k, x in out.items()}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **arrays)
    print(f"{a.out}: {len(arrays)} arrays, {os.path.getsize(a.out)} bytes")
    for k in sorted(arrays):
        print(k, arrays[k].shape)


if __name__ == "__main__":
    main()
