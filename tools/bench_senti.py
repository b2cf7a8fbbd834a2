"""What the sentiment task costs: the step under the task beside the default step, the collector launch, and a dev
evaluation pass with the collector beside the same pass with a read-back per batch and the numpy definition.

    python tools/bench_senti.py [--out profiles/senti.json]

The forms take turns inside each of --rounds rounds (the spread of a form is its min - max over the rounds):
    step        B = 32 and B = 256, T = 50, bf16, V = 20 000, dropout on: bench.py's batch.  `default` is the six-class emotion step,
                `sentiment` the one-column step under senti_loss = l1 on the same inputs; --steps steps between one device-event pair
                after --warmup untimed ones.  Every measurement is a process of its own (this file with --child TASK: one model per
                batch size), started before this process touches the device, so that no measurement shares its process with
                another model (two models taking turns in one process measured the second one slower at B = 32).  The head shrinks from 12 to 7 columns and no launch is added: the
                expectation is that `sentiment` lies inside `default`'s own range.
    collector   mmda_senti_accumulate over 32, 256 and 4096 rows: --reps launches back to back between one event pair
    eval        a dev pass over --eval-samples samples in batches of --eval-batch (a DeviceLoader): Solver.eval under the task -- one
                collector launch and one loss launch per batch, one read-back at the end -- against the same forwards with
                scores.cpu() per batch (the reference's loop) and eval_mosei_senti's definitions in numpy; host clock around a
                device synchronise

Needs the MI355X: there is no fall-back.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _range(xs):
    s = sorted(xs)
    return {"min": s[0], "median": s[len(s) // 2], "max": s[-1], "rounds": list(xs)}


def numpy_table(p, t):
    """eval_mosei_senti's figures from host arrays (numpy only: the weighted F1 from the 2x2 table)"""
    import numpy as np

    def f1w(y, q):
        out, n = 0.0, y.size
        for lab in (False, True):
            tp = float(((y == lab) & (q == lab)).sum()); den = float((y == lab).sum() + (q == lab).sum())
            out += (2 * tp / den if den else 0.0) * float((y == lab).sum())
        return out / n if n else float("nan")

    nz = t != 0
    ext = np.abs(t) > 2
    r = lambda x, lim: np.round(np.clip(x, -lim, lim))
    with np.errstate(all="ignore"):
        return dict(mae=float(np.abs(p - t).mean()), corr=float(np.corrcoef(p, t)[0][1]), acc7=float((r(p, 3) == r(t, 3)).mean()),
                    acc5=float((r(p, 2) == r(t, 2)).mean()), acc2=float(((p >= 0) == (t >= 0)).mean()), f1=f1w(t >= 0, p >= 0),
                    acc2_non0=float(((p[nz] > 0) == (t[nz] > 0)).mean()), f1_non0=f1w(t[nz] > 0, p[nz] > 0),
                    mae_intensity=float(np.abs(p[ext] - t[ext]).mean()))


def child(args):
    """one task: {"32": ms per step, "256": ms per step, "cls_32": ..., "cls_256": ...}"""
    import torch
    from mmda_amd import make_config
    from mmda_amd.data import synth_batch
    from mmda_amd.solver import Solver
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    out = {}
    for B in (32, 256):
        emb = torch.randn(args.vocab, 300, generator=torch.Generator().manual_seed(0))
        kw = dict(task="sentiment", num_classes=1) if args.child == "sentiment" else {}
        cfg = make_config(vocab_size=args.vocab, precision="bf16", device=str(dev), batch_size=B, seq_len=args.seq_len,
                          pretrained_emb=emb.clone(), **kw)
        torch.manual_seed(0)
        m = Solver(cfg, cfg, cfg, None, None, None, is_train=True).build().model
        m.train()
        t, v, a, y, emo, lengths, *_ = synth_batch(cfg, B, args.seq_len, seed=B, device=dev)
        target = y if args.child == "sentiment" else emo
        step = lambda: m.train_step(t, v, a, lengths, target, lr=cfg.learning_rate, clip=cfg.clip)
        for _ in range(args.warmup):
            step()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.steps):
            step()
        e1.record()
        torch.cuda.synchronize()
        m.check_cluster("bench_senti")
        L = m.read_losses()
        if not all(x == x for x in L.values()):
            raise SystemExit(f"non-finite losses: {L}")
        out[str(B)] = e0.elapsed_time(e1) / args.steps
        out[f"cls_{B}"] = L["cls"]
        del m
    print("CHILD " + json.dumps(out), flush=True)


def run_child(args, task):
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--child", task, "--steps", str(args.steps), "--warmup", str(args.warmup),
           "--seq-len", str(args.seq_len), "--vocab", str(args.vocab)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.child_timeout, cwd=ROOT)
    lines = [x for x in r.stdout.splitlines() if x.startswith("CHILD ")]
    if r.returncode != 0 or not lines:
        # (nothing more is started on the device behind a child that failed)
        raise SystemExit(f"child {task} ended with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads(lines[-1][6:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seq-len", type=int, default=50)
    ap.add_argument("--vocab", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=500)
    ap.add_argument("--eval-samples", type=int, default=1024)
    ap.add_argument("--eval-batch", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "senti.json"))
    ap.add_argument("--child", default=None, choices=("default", "sentiment"))
    ap.add_argument("--child-timeout", type=int, default=120)
    args = ap.parse_args()
    if args.child:
        return child(args)
    # ---- the step: children, before this process opens the device
    ms = {k: {"32": [], "256": []} for k in ("default", "sentiment")}
    last = {}
    for r in range(args.rounds):
        for k in ms:
            got = run_child(args, k)
            for B in ("32", "256"):
                ms[k][B].append(got[B])
                last.setdefault(B, {})[k] = got[f"cls_{B}"]
            print(f"round {r} {k}: B=32 {got['32']:.4f}  B=256 {got['256']:.4f} ms/step", file=sys.stderr, flush=True)
    steps = []
    for B in ("32", "256"):
        f = {k: _range(ms[k][B]) for k in ms}
        steps.append({"batch": int(B), "forms_ms_per_step": f, "last_cls_loss": last[B],
                      "sentiment_minus_default_us": 1e3 * (f["sentiment"]["median"] - f["default"]["median"]),
                      "sentiment_inside_default_range": bool(f["default"]["min"] <= f["sentiment"]["median"] <= f["default"]["max"])})
    import numpy as np
    import torch
    from mmda_amd import DeviceDataset, DeviceLoader, SentimentEval, make_config
    from mmda_amd.solver import Solver
    if not torch.cuda.is_available():
        raise SystemExit("bench_senti needs the MI355X: there is no fall-back")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def timed(fn, n):
        e0, e1 = ev(), ev()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    def solver(B, task):
        emb = torch.randn(args.vocab, 300, generator=torch.Generator().manual_seed(0))
        kw = dict(task="sentiment", num_classes=1) if task == "sentiment" else {}
        cfg = make_config(vocab_size=args.vocab, precision="bf16", device=str(dev), batch_size=B, seq_len=args.seq_len,
                          pretrained_emb=emb.clone(), **kw)
        torch.manual_seed(0)
        return Solver(cfg, cfg, cfg, None, None, None, is_train=True).build()

    # ---- the collector launch
    collector = []
    for n in (32, 256, 4096):
        p, t = torch.randn(n, device=dev), (torch.randint(-9, 10, (n,), device=dev).float() / 3.0)
        e = SentimentEval(dev)
        for _ in range(20):
            e.update(p, t)
        us = [1e3 * timed(lambda: e.update(p, t), args.reps) for _ in range(args.rounds)]
        collector.append({"rows": n, "us_per_launch": _range(us)})
    # ---- a dev evaluation pass
    s = solver(args.eval_batch, "sentiment")
    cfg = s.train_config
    rng = np.random.default_rng(1)
    samples = []
    for i in range(args.eval_samples):
        ln = int(rng.integers(5, args.seq_len + 1))
        lab = np.zeros((1, 7), np.float32)
        lab[0, 0] = rng.integers(-9, 10) / 3.0
        samples.append(((rng.integers(2, args.vocab, ln), rng.standard_normal((ln, cfg.visual_size)).astype(np.float32),
                         rng.standard_normal((ln, cfg.acoustic_size)).astype(np.float32), ["w"] * ln), lab, f"s{i}"))
    ds = DeviceDataset.from_samples(samples, dev)
    s.dev_data_loader = DeviceLoader(ds, args.eval_batch)

    def with_collector():
        s.eval("dev")
        return s.last_sentiment

    def with_readback():
        P, T = [], []
        for scores, y in s._eval_batches(s.dev_data_loader):
            P.append(scores.cpu().numpy().reshape(-1)); T.append(y.cpu().numpy().reshape(-1))       # a read-back per batch
        return numpy_table(np.concatenate(P).astype(np.float64), np.concatenate(T).astype(np.float64))

    passes = {"collector": with_collector, "readback_numpy": with_readback}
    tabs = {k: fn() for k, fn in passes.items()}                                                   # warm-up, and the two tables
    for k in tabs["readback_numpy"]:
        a_, b_ = tabs["collector"][k], tabs["readback_numpy"][k]
        if not (abs(a_ - b_) <= 1e-9 * max(1.0, abs(b_)) or (a_ != a_ and b_ != b_)):
            raise SystemExit(f"the two passes disagree about {k}: {a_} / {b_}")
    ms = {k: [] for k in passes}
    for r in range(args.rounds):
        for k, fn in passes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[k].append(1e3 * (time.perf_counter() - t0))
    evalp = {"samples": args.eval_samples, "batch": args.eval_batch, "batches": len(s.dev_data_loader),
             "ms_per_pass": {k: _range(x) for k, x in ms.items()}, "mae": tabs["collector"]["mae"]}
    line = json.dumps({"bench": "senti", "seq_len": args.seq_len, "precision": "bf16", "vocab": args.vocab, "steps_per_round": args.steps,
                       "rounds": args.rounds, "senti_loss": "l1", "step": steps, "collector": collector,
                       "collector_launches_per_round": args.reps, "eval_pass": evalp})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
