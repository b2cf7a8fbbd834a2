"""What the optimizer's settings cost the fused training step.

    python tools/bench_optim.py [--out profiles/optim_step.json]

B = 32 and B = 256, T = 50, bf16, V = 20 000, dropout on, one model per batch size.  Three forms take turns --rounds times in one process
(drift of the machine lands on all of them alike), each after a warm-up of its own:
    adam        train_step(optimizer=Adam(lr)): the default launches (early optimizer pass beside the layer-1 recurrence, flag join)
    adamw       train_step(optimizer=AdamW(lr, weight_decay=0.1)): the same launches with the decayed functor
    clip_norm   train_step(optimizer=Adam(lr), clip_norm=...): no early pass, event join, the norm's two launches, one launch over the
                whole bucket -- what it costs is the lost overlap plus one reduction
One device-event pair around --steps steps of a form (after --warmup untimed ones), the model's cluster check at the end of each turn.
The norm alone (mmda_grad_norm over the model's gradient bucket, both of its launches): --norm-reps calls queued behind a blocking
matrix product, one event pair around them (the method of tools/bench_infer.py).

Needs the MI355X: there is no fall-back.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _range(xs):
    s = sorted(xs)
    return {"min": s[0], "median": s[len(s) // 2], "max": s[-1], "rounds": list(xs)}


def measure(args, B):
    import torch
    from mmda_amd import make_config, ops, optim
    from mmda_amd.data import synth_batch
    from mmda_amd.solver import Solver
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    emb = torch.randn(args.vocab, 300, generator=torch.Generator().manual_seed(0))
    cfg = make_config(vocab_size=args.vocab, precision="bf16", device=str(dev), batch_size=B, seq_len=args.seq_len, pretrained_emb=emb.clone())
    m = Solver(cfg, cfg, cfg, None, None, None, is_train=True).build().model
    m.train()
    t, v, a, y, emo, lengths, *_ = synth_batch(cfg, B, args.seq_len, seed=B, device=dev)       # bench.py's batch
    params = list(m.parameters())
    adam = optim.Adam(params, lr=cfg.learning_rate).attach(m)
    adamw = optim.AdamW(params, lr=cfg.learning_rate, weight_decay=0.1).attach(m)
    kw = dict(lr=cfg.learning_rate, clip=cfg.clip)
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def timed(fn, n=1):
        e0, e1 = ev(), ev()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    # a max_norm the gradient exceeds, so the coefficient is not 1 (the launches are the same either way)
    m.train_step(t, v, a, lengths, emo, do_adam=False, **kw)
    clip_norm = 0.5 * float(ops.grad_norm(m.flat_buckets()[1], 1.0)[0])
    forms = (("adam", lambda: m.train_step(t, v, a, lengths, emo, optimizer=adam, **kw)),
             ("adamw", lambda: m.train_step(t, v, a, lengths, emo, optimizer=adamw, **kw)),
             ("clip_norm", lambda: m.train_step(t, v, a, lengths, emo, optimizer=adam, clip_norm=clip_norm, **kw)))
    ms = {k: [] for k, _ in forms}
    for _ in range(args.rounds):
        for name, step in forms:
            timed(step, args.warmup)
            ms[name].append(timed(step, args.steps))
            m.check_cluster(f"bench_optim {name}")
    L = m.read_losses()
    if not all(x == x for x in L.values()):
        raise SystemExit(f"non-finite losses: {L}")
    f = {k: _range(x) for k, x in ms.items()}
    out = {"batch": B, "bucket_floats": int(m.grad_floats), "clip_norm": clip_norm, "last_grad_norm": float(m.grad_norm()),
           "forms_ms_per_step": f,
           "adamw_over_adam": f["adamw"]["median"] / f["adam"]["median"],
           "clip_norm_over_adam": f["clip_norm"]["median"] / f["adam"]["median"],
           "clip_norm_minus_adam_us": 1e3 * (f["clip_norm"]["median"] - f["adam"]["median"]),
           "adamw_inside_adam_spread": bool(f["adam"]["min"] <= f["adamw"]["median"] <= f["adam"]["max"]),
           "clip_norm_slower_beyond_spread": bool(f["clip_norm"]["min"] > f["adam"]["max"])}
    print(f"B={B}: " + ", ".join(f"{k} {f[k]['min']:.3f}-{f[k]['max']:.3f}" for k in f) + " ms/step", file=sys.stderr, flush=True)

    # ---- the norm alone (its two launches), queued behind a blocker
    G = m.flat_buckets()[1]
    norm = lambda: ops.grad_norm(G, clip_norm)
    big = torch.randn(8192, 8192, device=dev)
    sink = torch.empty_like(big)
    torch.mm(big, big, out=sink)
    for _ in range(20):
        norm()
    us = []
    for r in range(args.norm_rounds):
        b0, e0, e1 = ev(), ev(), ev()
        torch.cuda.synchronize()
        b0.record()
        for _ in range(args.blockers):
            torch.mm(big, big, out=sink)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(args.norm_reps):
            norm()
        e1.record()
        host_ms = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        if host_ms >= b0.elapsed_time(e0):
            raise SystemExit(f"norm: B={B} round {r}: queueing took the host {host_ms:.2f} ms, longer than the blocker: the launches were "
                             "not all waiting, nothing is reported")
        us.append(e0.elapsed_time(e1) * 1e3 / args.norm_reps)
    out["grad_norm"] = {"bytes_read": int(m.grad_floats) * 4, "launches_per_call": 2, "calls_per_round": args.norm_reps,
                        "us_per_call": _range(us)}
    m.check_cluster("bench_optim norm")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seq-len", type=int, default=50)
    ap.add_argument("--vocab", type=int, default=20000)
    ap.add_argument("--norm-reps", type=int, default=100)
    ap.add_argument("--norm-rounds", type=int, default=3)
    ap.add_argument("--blockers", type=int, default=4, help="8192^2 matrix products the norm calls are queued behind")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_step.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim needs the MI355X (no CPU path)")
    torch.cuda.set_device(0)
    line = json.dumps({"bench": "optim_step", "device": torch.cuda.get_device_name(0), "seq_len": args.seq_len, "precision": "bf16",
                       "vocab": args.vocab, "steps_per_round": args.steps, "rounds": args.rounds,
                       "results": [measure(args, B) for B in (32, 256)]})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
