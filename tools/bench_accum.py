"""What gradient accumulation (config.accum_steps) costs per micro-batch.

    python tools/bench_accum.py [--modes dense,sparse,frozen] [--accum 4] [--out FILE.json]

Per embed_update mode, one model, B = 32, T = 50, bf16, V = 20 000, dropout on, three variants alternated --rounds times in one process
(drift of the machine lands on all of them alike):
    micro   train_step(do_adam=False): the micro-batch alone -- the step every accumulated micro-batch starts with, unchanged by this
            feature, so it is also the reference point "without accumulation"
    accum   an optimizer step from --accum micro-batches, reported per micro-batch: (accum - 1) accumulate passes and one closing step
    plain   train_step(): today's step, optimizer included
and, with events around the single launches on the model's own buckets, the accumulate pass, the closing step over a sum and the plain
clamp + Adam launch over the same range (median of --rounds, after one untimed call each).

Needs the MI355X: there is no fall-back.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MODES = ("dense", "sparse", "frozen")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="micro-batches per timed round (a multiple of --accum)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--accum", type=int, default=4)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seq-len", type=int, default=50)
    ap.add_argument("--vocab", type=int, default=20000)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--out", help="also write the result to this file")
    args = ap.parse_args()
    if args.accum < 2 or args.steps % args.accum:
        raise SystemExit("--accum must be at least 2 and divide --steps")

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_accum needs the MI355X (no CPU path)")
    from mmda_amd import make_config, ops
    from mmda_amd.data import synth_batch
    from mmda_amd.solver import Solver

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    modes = tuple(args.modes.split(","))
    if any(mo not in MODES for mo in modes):
        raise SystemExit(f"--modes: choose from {MODES}")
    emb = torch.randn(args.vocab, 300, generator=torch.Generator().manual_seed(0))
    N = args.accum
    results = []
    for mode in modes:
        torch.manual_seed(0)
        cfg = make_config(vocab_size=args.vocab, precision=args.precision, device=str(dev), batch_size=args.batch, seq_len=args.seq_len,
                          pretrained_emb=emb.clone(), embed_update=mode, accum_steps=N)
        m = Solver(cfg, cfg, cfg, None, None, None, is_train=True).build().model
        m.train()
        t, v, a, y, emo, lengths, *_ = synth_batch(cfg, args.batch, args.seq_len, seed=0, ragged=False, device=dev)
        kw = dict(lr=cfg.learning_rate, clip=cfg.clip)

        def micro(n):
            for _ in range(n):
                m.train_step(t, v, a, lengths, emo, do_adam=False, **kw)

        def accum(n):
            for i in range(n):
                m.train_step(t, v, a, lengths, emo, accum_index=i % N, accum_count=N, **kw)

        def plain(n):
            for _ in range(n):
                m.train_step(t, v, a, lengths, emo, **kw)

        variants = {"micro": micro, "accum": accum, "plain": plain}

        def run(fn, n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(n)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n * 1e3

        warm = (args.warmup + N - 1) // N * N
        for fn in variants.values():
            run(fn, warm)
        ms = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                ms[k].append(run(fn, args.steps))
        L = m.read_losses()
        if not all(x == x for x in L.values()) or m.cluster_aborted():
            raise SystemExit(f"{mode}: non-finite losses or an aborted recurrence: {L}")

        # the single launches, on the model's own buckets (values are irrelevant: lr = 0 leaves the parameters alone)
        P, G, M, V = m.flat_buckets()
        n = m.grad_floats
        acc = m._acc[:n]
        launches = {
            "accumulate": lambda: ops.grad_accumulate(acc, G[:n]),
            "clamp_adam_sum": lambda: ops.clamp_adam_sum(P[:n], acc, G[:n], M[:n], V[:n], 0.0, 1, clip=cfg.clip, grad_scale=1.0 / N),
            "clamp_adam": lambda: ops.clamp_adam(P[:n], G[:n], M[:n], V[:n], 0.0, 1, clip=cfg.clip),
        }
        us = {k: [] for k in launches}
        for rep in range(args.rounds + 1):
            for k, fn in launches.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record(); fn(); e1.record()
                torch.cuda.synchronize()
                if rep:
                    us[k].append(e0.elapsed_time(e1) * 1e3)
        row = {"embed_update": mode, "batch": args.batch, "seq_len": args.seq_len, "precision": args.precision, "vocab": args.vocab,
               "accum_steps": N, "micro_batches_per_round": args.steps, "rounds": args.rounds, "bucket_floats": int(n),
               "bucket_mb": n * 4 / 1e6}
        for k in variants:
            xs = sorted(ms[k])
            row[k] = {"ms_per_micro_batch_median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "rounds_ms": ms[k]}
        row["accum_minus_micro_us"] = (row["accum"]["ms_per_micro_batch_median"] - row["micro"]["ms_per_micro_batch_median"]) * 1e3
        row["plain_minus_micro_us"] = (row["plain"]["ms_per_micro_batch_median"] - row["micro"]["ms_per_micro_batch_median"]) * 1e3
        for k in launches:
            xs = sorted(us[k])
            row[k + "_us"] = {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}
        results.append(row)
        del m
        torch.cuda.empty_cache()
    line = json.dumps({"bench": "accum", "device": torch.cuda.get_device_name(0), "results": results})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
