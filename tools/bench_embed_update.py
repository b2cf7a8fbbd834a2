"""Step time of the four config.embed_update modes against each other (dense = the reference point, in the same call).

    python tools/bench_embed_update.py [--out FILE.json]          B in {32, 256} x {full, ragged} lengths, T = 50, bf16, dropout on,
                                                                  V = 20 000; every shape warmed, the modes alternated --rounds times
    python tools/bench_embed_update.py --only MODE --batch 32     one mode, one shape, few steps: the program of a kernel-trace run
    python tools/bench_embed_update.py --modes dense,deferred --batches 32,256 --ragged 0
                                                                  a subset of the modes / shapes, still alternated in one call
    python tools/bench_embed_update.py --deferred-costs 64,256,1024
                                                                  what the window of the deferred mode costs (op level): after
                                                                  window - 1 updates on one id list, the catch-up launch of ANOTHER
                                                                  list (every row at the largest gap) and the full flush, timed with
                                                                  events, --rounds times each

Needs the MI355X: there is no fall-back (the model raises on a CPU tensor, and this script checks first).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MODES = ("dense", "sparse", "frozen", "deferred")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seq-len", type=int, default=50)
    ap.add_argument("--vocab", type=int, default=20000)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--only", choices=MODES, help="time this mode alone (with --batch / --ragged)")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--ragged", type=int, default=0)
    ap.add_argument("--modes", help="comma-separated subset of the modes (default: all)")
    ap.add_argument("--batches", help="comma-separated batch sizes (default: 32,256, each with full and ragged lengths)")
    ap.add_argument("--window", type=int, default=0, help="deferred: steps between full flushes (default: the configuration's)")
    ap.add_argument("--deferred-costs", help="comma-separated windows: time the catch-up launch at the largest gap and the flush")
    ap.add_argument("--out", help="also write the result to this file")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_embed_update needs the MI355X (no CPU path)")
    from mmda_amd import make_config
    from mmda_amd.data import synth_batch
    from mmda_amd.solver import Solver

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    modes = (args.only,) if args.only else tuple(args.modes.split(",")) if args.modes else MODES
    if any(mo not in MODES for mo in modes):
        raise SystemExit(f"--modes: choose from {MODES}")
    if args.only:
        shapes = [(args.batch, bool(args.ragged))]
    elif args.batches:
        shapes = [(int(b), bool(args.ragged)) for b in args.batches.split(",")]
    else:
        shapes = [(32, False), (32, True), (256, False), (256, True)]
    emb = torch.randn(args.vocab, 300, generator=torch.Generator().manual_seed(0))

    def build(mode, B, window=0):
        torch.manual_seed(0)
        kw = {"embed_deferred_window": window or args.window} if (window or args.window) else {}
        cfg = make_config(vocab_size=args.vocab, precision=args.precision, device=str(dev), batch_size=B, seq_len=args.seq_len,
                          pretrained_emb=emb.clone(), embed_update=mode, **kw)
        s = Solver(cfg, cfg, cfg, None, None, None, is_train=True).build()
        s.model.train()
        return cfg, s.model

    if args.deferred_costs:
        # the two costs of a window, at the op level on a (vocab, 300) table: window - 1 updates on list A leave every other row
        # window - 1 updates behind; the catch-up launch of list B (other ids: every row at that gap) and the full flush are then timed
        # with events.  The gap is rebuilt and both are timed --rounds times after one untimed pass (first launches); the range is
        # reported, never one sample.
        from mmda_amd import ops
        n, D, V = args.batch * args.seq_len, 300, args.vocab
        g = torch.Generator().manual_seed(0)
        ids_a = torch.randint(2, V, (n,), generator=g).to(dev)
        ids_b = torch.randint(2, V, (n,), generator=g).to(dev)
        rows = (torch.randn(n, D, generator=g) * 1e-2).to(dev)
        out = []
        for w in [int(x) for x in args.deferred_costs.split(",")]:
            P = emb.clone().to(dev); M = torch.zeros_like(P); Vv = torch.zeros_like(P)
            cu, fl, stale = [], [], 0
            for rep in range(args.rounds + 1):
                st = ops.embed_deferred_state(V, w)
                for k in range(1, w):
                    ops.embed_rows_dense_adam(P, M, Vv, st, ids_a, rows, 1e-4, k, clip=1.0)
                stale = int((st.row_step[torch.unique(ids_b)] < w - 1).sum())
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                torch.cuda.synchronize()
                ev[0].record(); ops.embed_rows_catch_up(P, M, Vv, st, ids_b); ev[1].record()
                ev[2].record(); ops.embed_rows_flush(P, M, Vv, st); ev[3].record()
                torch.cuda.synchronize()
                if rep:
                    cu.append(ev[0].elapsed_time(ev[1]) * 1e3); fl.append(ev[2].elapsed_time(ev[3]) * 1e3)
            cu.sort(); fl.sort()
            out.append({"window": w, "positions": n, "vocab": V, "gap_updates": w - 1, "catch_up_rows": stale, "samples": len(cu),
                        "catch_up_us": {"min": cu[0], "median": cu[len(cu) // 2], "max": cu[-1]},
                        "flush_us": {"min": fl[0], "median": fl[len(fl) // 2], "max": fl[-1]},
                        "flush_us_per_update_median": fl[len(fl) // 2] / w})
        line = json.dumps({"bench": "embed_deferred_costs", "device": torch.cuda.get_device_name(0), "results": out})
        print(line)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return

    results = []
    for B, ragged in shapes:
        models = {mo: build(mo, B) for mo in modes}
        cfg0 = models[modes[0]][0]
        t, v, a, y, emo, lengths, *_ = synth_batch(cfg0, B, args.seq_len, seed=0, ragged=ragged, device=dev)

        def run(mode, n):
            cfg, m = models[mode]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                m.train_step(t, v, a, lengths, emo, lr=cfg.learning_rate, clip=cfg.clip)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n * 1e3

        for mo in modes:
            run(mo, args.warmup)
        ms = {mo: [] for mo in modes}
        for _ in range(args.rounds):                     # alternate the variants: drift of the box lands on all of them alike
            for mo in modes:
                ms[mo].append(run(mo, args.steps))
        for mo in modes:
            cfg, m = models[mo]
            L = m.read_losses()
            if not all(x == x for x in L.values()) or m.cluster_aborted():
                raise SystemExit(f"{mo}: non-finite losses or an aborted recurrence: {L}")
        row = {"batch": B, "seq_len": args.seq_len, "ragged": ragged, "precision": args.precision, "vocab": args.vocab,
               "steps_per_round": args.steps, "rounds": args.rounds}
        for mo in modes:
            xs = sorted(ms[mo])
            row[mo] = {"ms_per_step_median": xs[len(xs) // 2], "ms_per_step_min": xs[0], "ms_per_step_max": xs[-1], "rounds_ms": ms[mo]}
        if "dense" in row:
            for mo in modes:
                row[mo]["vs_dense"] = row[mo]["ms_per_step_median"] / row["dense"]["ms_per_step_median"]
        results.append(row)
        del models
        torch.cuda.empty_cache()
    line = json.dumps({"bench": "embed_update", "device": torch.cuda.get_device_name(0), "results": results})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
