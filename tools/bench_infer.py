"""An inference pass over a device-resident corpus, three ways (GPU box), and its collect launch by itself.

    python tools/bench_infer.py [--out profiles/infer_pass.json]
                                n = 4096 seeded synthetic samples, lengths uniform in [5, 50], MOSEI widths, V = 20 000, bf16; B = 32 and 256
                                  (a) eval_loop      the Solver.eval-style loop over DeviceLoader in dataset order: model(...) under no_grad,
                                                     the labels kept per batch and concatenated -- the only way before the pass existed
                                  (b) run_dataset    InferencePass.run(order="dataset"): the same batches, one collect launch each
                                  (c) run_length     InferencePass.run(order="length"): batches by length, rows put back by index
                                --rounds rounds, the three forms taking turns inside a round; one device-event pair (and the host's wall
                                clock) per pass.  Every pass ends in the model's cluster check (a synchronous read), inside the pair.
                                The collect launch alone: --collect-reps launches queued behind a blocking matrix product, one event pair
                                around them (the method of tools/bench_input_pipeline.py).
    python tools/bench_infer.py --worker pass       the measuring process by itself (prints its JSON line)

The parent process never opens the GPU: the measurement is a child process with a time limit (--step-timeout) that reports each case on
stderr as it goes.  Needs the MI355X: there is no fall-back.  Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DV, DA, VOCAB = 35, 74, 20000


def synth_samples(n, seed, lo=5, hi=50):
    """n reference-style samples, seeded; the lengths are the first draw: default_rng(seed).integers(lo, hi + 1, n)"""
    import numpy as np
    rng = np.random.default_rng(seed)
    lengths = rng.integers(lo, hi + 1, size=n)
    out = []
    for i, L in enumerate(lengths.tolist()):
        out.append(((rng.integers(2, VOCAB, size=L), rng.standard_normal((L, DV), dtype=np.float32),
                     rng.standard_normal((L, DA), dtype=np.float32), None), rng.standard_normal((1, 7)).astype(np.float32), f"seg{i}"))
    return out


def _range(xs):
    s = sorted(xs)
    return {"min": s[0], "median": s[len(s) // 2], "max": s[-1], "rounds": list(xs)}


def worker_pass(args):
    import time
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_infer needs the MI355X (no CPU path)")
    import ctypes
    from mmda_amd import MISA, DeviceDataset, DeviceLoader, InferencePass, _lib, inference_plan, make_config
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ds = DeviceDataset.from_samples(synth_samples(args.n, args.seed), dev)
    torch.manual_seed(args.seed)
    model = MISA(make_config(precision="bf16", device="cuda:0", vocab_size=VOCAB)).to(dev).eval()
    fields = ("scores", "labels", "tcp", "hidden")
    p = InferencePass(model, fields)
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def eval_loop(B):
        preds = []
        with torch.no_grad():
            for batch in DeviceLoader(ds, B):
                _, labels = model(batch[0], batch[1], batch[2], batch[5])
                preds.append(labels)
        out = torch.cat(preds, 0)
        model.check_cluster("bench_infer eval_loop")
        return out

    def timed(fn):
        e0, e1 = ev(), ev()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3

    results = []
    for B in (32, 256):
        forms = {"eval_loop": lambda: eval_loop(B), "run_dataset": lambda: p.run(ds, B, "dataset"), "run_length": lambda: p.run(ds, B, "length")}
        steps = {}
        for order in ("dataset", "length"):
            plan, bounds = inference_plan(ds.lengths, B, order)
            T = ds.lengths[plan[bounds[:-1]]]
            steps[order] = {"batches": int(len(T)), "sum_T": int(T.sum()),
                            "padded_fraction": float(1.0 - ds.lengths.sum() / (T * np.diff(bounds)).sum())}
        for fn in forms.values():                                    # warm-up: workspace, allocator blocks, first-call set-up
            fn()
        dev_ms = {k: [] for k in forms}
        wall_ms = {k: [] for k in forms}
        for r in range(args.rounds):
            for k, fn in forms.items():
                d, w = timed(fn)
                dev_ms[k].append(d); wall_ms[k].append(w)
        med = {k: sorted(v)[len(v) // 2] for k, v in dev_ms.items()}
        print(f"pass: B={B}: " + ", ".join(f"{k} {med[k]:.2f} ms" for k in forms) + f" (device, median of {args.rounds})", file=sys.stderr,
              flush=True)
        results.append({"batch": B, "plan": steps, "step_ratio": steps["dataset"]["sum_T"] / steps["length"]["sum_T"],
                        "device_ms": {k: _range(v) for k, v in dev_ms.items()}, "wall_ms": {k: _range(v) for k, v in wall_ms.items()},
                        "speedup_length_over_eval_loop": med["eval_loop"] / med["run_length"],
                        "speedup_dataset_over_eval_loop": med["eval_loop"] / med["run_dataset"],
                        # the claim: (c) beats (a) by more than the round-to-round spread of either form
                        "length_beats_eval_loop_beyond_spread": min(dev_ms["eval_loop"]) > max(dev_ms["run_length"])})

    # ---- the collect launch alone, queued behind a blocker
    big = torch.randn(8192, 8192, device=dev)
    sink = torch.empty_like(big)
    torch.mm(big, big, out=sink)
    collect = []
    for B in (32, 256):
        batch = next(iter(DeviceLoader(ds, B)))
        flat, layout, out = p._tables(B, dev)
        p._batch(batch[0], batch[1], batch[2], batch[5], out, None, 0)           # a forward's results in the workspace, B columns
        lib, h, s = model._lib, model._h, _lib.stream_ptr()
        launch = lambda: lib.mmda_misa_infer_collect(h, ctypes.byref(out), None, 0, s)
        for _ in range(20):
            _lib.check(launch(), "collect")
        us = []
        for r in range(args.collect_rounds):
            b0, e0, e1 = ev(), ev(), ev()
            torch.cuda.synchronize()
            b0.record()
            torch.mm(big, big, out=sink); torch.mm(big, big, out=sink)
            t0 = time.perf_counter()
            e0.record()
            for _ in range(args.collect_reps):
                launch()
            e1.record()
            host_ms = (time.perf_counter() - t0) * 1e3
            torch.cuda.synchronize()
            blk_ms = b0.elapsed_time(e0)
            if host_ms >= blk_ms:
                raise SystemExit(f"collect: B={B} round {r}: queueing took the host {host_ms:.2f} ms, the blocker {blk_ms:.2f} ms: the "
                                 "launches were not all waiting, nothing is reported")
            us.append(e0.elapsed_time(e1) * 1e3 / args.collect_reps)
        print(f"collect: B={B}: {sorted(us)[len(us) // 2]:.2f} us per queued launch", file=sys.stderr, flush=True)
        collect.append({"batch": B, "fields": list(fields), "bytes_written": int(B * 4 * (6 + 6 + 6 + 768)),
                        "launches_per_round": args.collect_reps, "us_per_launch": _range(us)})
    model.check_cluster("bench_infer")
    print(json.dumps({"worker": "pass", "device": torch.cuda.get_device_name(0), "passes": results, "collect": collect}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--collect-reps", type=int, default=200)
    ap.add_argument("--collect-rounds", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds the GPU step (a child process) may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "infer_pass.json"))
    ap.add_argument("--worker", choices=["pass"])
    args = ap.parse_args()
    if args.worker == "pass":
        return worker_pass(args)

    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "pass", "--n", str(args.n), "--seed", str(args.seed),
           "--rounds", str(args.rounds), "--collect-reps", str(args.collect_reps), "--collect-rounds", str(args.collect_rounds)]
    try:
        q = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.step_timeout)      # the child's stderr is ours: progress lines
    except subprocess.TimeoutExpired:
        raise SystemExit(f"pass: no result after {args.step_timeout} s")
    if q.returncode != 0:
        sys.stderr.write(q.stdout)
        raise SystemExit(f"pass: exit status {q.returncode}")
    res = json.loads(q.stdout.strip().splitlines()[-1])
    line = json.dumps({"bench": "infer_pass", "device": res["device"], "n": args.n, "seed": args.seed, "precision": "bf16",
                       "vocab": VOCAB, "passes": res["passes"], "collect": res["collect"]})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
