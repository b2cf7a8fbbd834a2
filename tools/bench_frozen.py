"""What freezing parameters (requires_grad = False) saves per training step.

    python tools/bench_frozen.py [--out profiles/frozen_step.json]

One model, B = 32, T = 50, bf16, V = 20 000, dropout on (the shapes of bench.py's default, this tool's own code), four forms of the fused
step alternated --rounds times in one process (drift of the machine lands on all of them alike):
    unfrozen     nothing frozen: today's step
    trnn1_embed  trnn1.* and the table frozen: every gradient is still computed, the optimizer launches walk the trainable runs
    cut_stash    the encoder cut (all six recurrent layers, the three inter-layer LayerNorms, the table), stashing forward
    cut          the same with the forward that keeps no encoder stash (the default under the cut)
Device events around --steps steps of each form, after --warmup untimed steps of that form (the first of which re-sends the set and
copies the run table).  Reports the per-round times, their median and spread, and whether `cut` beats `unfrozen` by more than the
spread between rounds of one form.

Needs the MI355X: there is no fall-back.  Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ENCODERS = ("trnn", "vrnn", "arnn", "tlayer_norm", "vlayer_norm", "alayer_norm", "embed")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seq-len", type=int, default=50)
    ap.add_argument("--vocab", type=int, default=20000)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--out", help="also write the result to this file")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_frozen needs the MI355X (no CPU path)")
    from mmda_amd import make_config
    from mmda_amd.data import synth_batch
    from mmda_amd.solver import Solver

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(0)
    emb = torch.randn(args.vocab, 300, generator=torch.Generator().manual_seed(0))
    cfg = make_config(vocab_size=args.vocab, precision=args.precision, device=str(dev), batch_size=args.batch, seq_len=args.seq_len,
                      pretrained_emb=emb.clone())
    m = Solver(cfg, cfg, cfg, None, None, None, is_train=True).build().model
    m.train()
    t, v, a, y, emo, lengths, *_ = synth_batch(cfg, args.batch, args.seq_len, seed=0, ragged=False, device=dev)
    kw = dict(lr=cfg.learning_rate, clip=cfg.clip)
    everything = [n.split(".")[0] for n in m._names]

    def form(frozen, stash):
        def enter():
            m.unfreeze(*everything)
            if frozen:
                m.freeze(*frozen)
            m.set_frozen_forward(stash)
        return enter

    forms = {"unfrozen": form((), False), "trnn1_embed": form(("trnn1", "embed"), False), "cut_stash": form(ENCODERS, True),
             "cut": form(ENCODERS, False)}

    def run(n, timed):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            m.train_step(t, v, a, lengths, emo, **kw)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n if timed else 0.0

    ms = {k: [] for k in forms}
    info = {}
    for _ in range(args.rounds):
        for k, enter in forms.items():
            enter()
            run(args.warmup, False)
            ms[k].append(run(args.steps, True))
            runs, floats, cut = m.trainable_info()
            info[k] = {"runs": len(runs), "trainable_floats": floats, "encoder_cut": cut}
    L = m.read_losses()
    if not all(x == x for x in L.values()) or m.cluster_aborted():
        raise SystemExit(f"non-finite losses or an aborted recurrence: {L}")
    out = {"bench": "frozen", "device": torch.cuda.get_device_name(0), "batch": args.batch, "seq_len": args.seq_len,
           "precision": args.precision, "vocab": args.vocab, "steps_per_round": args.steps, "rounds": args.rounds, "forms": {}}
    for k in forms:
        xs = sorted(ms[k])
        out["forms"][k] = dict(info[k], ms_per_step_median=xs[len(xs) // 2], min=xs[0], max=xs[-1], spread_ms=xs[-1] - xs[0], rounds_ms=ms[k])
    f = out["forms"]
    spread = max(f["unfrozen"]["spread_ms"], f["cut"]["spread_ms"])
    out["cut_saves_ms"] = f["unfrozen"]["ms_per_step_median"] - f["cut"]["ms_per_step_median"]
    out["no_stash_saves_ms"] = f["cut_stash"]["ms_per_step_median"] - f["cut"]["ms_per_step_median"]
    out["cut_faster_than_unfrozen_beyond_the_spread"] = bool(out["cut_saves_ms"] > spread)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
