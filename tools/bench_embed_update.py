"""Step time of the three config.embed_update modes against each other (dense = the reference point, in the same call).

    python tools/bench_embed_update.py [--out FILE.json]          B in {32, 256} x {full, ragged} lengths, T = 50, bf16, dropout on,
                                                                  V = 20 000; every shape warmed, the modes alternated --rounds times
    python tools/bench_embed_update.py --only MODE --batch 32     one mode, one shape, few steps: the program of a kernel-trace run

Needs the MI355X: there is no fall-back (the model raises on a CPU tensor, and this script checks first).  Prints one JSON line."""
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
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seq-len", type=int, default=50)
    ap.add_argument("--vocab", type=int, default=20000)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--only", choices=MODES, help="time this mode alone (with --batch / --ragged)")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--ragged", type=int, default=0)
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
    modes = (args.only,) if args.only else MODES
    shapes = [(args.batch, bool(args.ragged))] if args.only else [(32, False), (32, True), (256, False), (256, True)]
    emb = torch.randn(args.vocab, 300, generator=torch.Generator().manual_seed(0))

    def build(mode, B):
        torch.manual_seed(0)
        cfg = make_config(vocab_size=args.vocab, precision=args.precision, device=str(dev), batch_size=B, seq_len=args.seq_len,
                          pretrained_emb=emb.clone(), embed_update=mode)
        s = Solver(cfg, cfg, cfg, None, None, None, is_train=True).build()
        s.model.train()
        return cfg, s.model

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
