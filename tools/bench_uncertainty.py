"""MC-dropout uncertainty over a device-resident corpus, four ways (GPU box), and its reduce launch by itself.

    python tools/bench_uncertainty.py [--out profiles/uncertainty.json]
                                n = 4096 seeded synthetic samples, lengths uniform in [5, 50], MOSEI widths, V = 20 000, bf16; K = 8 and 32
                                  (a) pass            MCDropoutPass(model, K, columns=256).run(dataset, 256): one evaluation forward per
                                                      batch, then ONE training-mode forward of the fusion block per 256 // K samples over
                                                      rows repeated K times, two reduce launches each
                                  (b) model_loop      the loop it replaces: per DeviceLoader batch of 256, K training-mode model(...) calls
                                                      under no_grad (encoders and all), the scores stacked and reduced by torch ops
                                  (c) encoded_chunk   phase A as (a); then, per chunk of 256 // K samples, K separate forwards from the
                                                      cached rows at that many columns, stacked and reduced by torch ops: what the
                                                      repeated-row form buys over calling the block K times on the same samples
                                  (d) encoded_256     the same with 256 samples per chunk: K separate forwards at 256 columns each, the
                                                      same number of columns per launch as (a) and the same number of launches
                                --rounds rounds, the forms taking turns inside a round; one device-event pair (and the host's wall clock) per
                                pass.  Every form ends in the model's cluster check (a synchronous read), inside the pair.
                                The reduce launch alone at (B, K) = (8, 32), (32, 8), (1, 256), W = 6, every table asked for: --reduce-reps
                                launches queued behind a blocking matrix product, one event pair around them (tools/bench_infer.py's method).
    python tools/bench_uncertainty.py --worker pass     the measuring process by itself (prints its JSON line)

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

from bench_infer import VOCAB, _range, synth_samples  # noqa: E402  (tools/ is this script's directory)

COLUMNS, BATCH = 256, 256


def torch_stats(stack, thr):
    """The seven figures of a (K, B, C) stack of score draws by torch ops in float64 (what a user would write)."""
    import torch
    d = stack.double()
    mean = d.mean(0)
    var = d.var(0, unbiased=False)
    h = lambda q: -(torch.xlogy(q, q) + torch.xlogy(1 - q, 1 - q))
    ent, eh = h(mean), h(d).mean(0)
    return mean, var, ent, eh, (ent - eh).clamp_min(0), (stack > thr).double().mean(0)


def worker_pass(args):
    import ctypes
    import time
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_uncertainty needs the MI355X (no CPU path)")
    from mmda_amd import MISA, DeviceDataset, DeviceLoader, EncoderCache, MCDropoutPass, _lib, make_config
    from mmda_amd.uncertainty import chunk_seeds
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ds = DeviceDataset.from_samples(synth_samples(args.n, args.seed), dev)
    torch.manual_seed(args.seed)
    model = MISA(make_config(precision="bf16", device="cuda:0", vocab_size=VOCAB)).to(dev)
    thr = float(model.config.threshold)
    n = len(ds)
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def timed(fn):
        e0, e1 = ev(), ev()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3

    def run_pass(K):
        model.eval()
        res = MCDropoutPass(model, passes=K, seed=1, columns=COLUMNS).run(ds, BATCH)
        model.check_cluster("bench_uncertainty pass")
        return res

    def model_loop(K):
        model.train()                                             # model(...) draws its masks only in training mode
        out = []
        with torch.no_grad():
            for batch in DeviceLoader(ds, BATCH):
                draws = [model(batch[0], batch[1], batch[2], batch[5])[0] for _ in range(K)]
                out.append(torch_stats(torch.stack(draws), thr))
        model.eval()
        model.check_cluster("bench_uncertainty model_loop")
        return [torch.cat(x, 0) for x in zip(*out)]

    def encoded_separate(K, per):
        model.eval()
        cache = EncoderCache.build(model, ds, BATCH)              # (phase A: the evaluation pass; ends in its own fingerprint read-back)
        rows = torch.arange(n, dtype=torch.int32, device=dev)
        nc = int(model.config.num_classes)
        seeds = chunk_seeds(1, K * ((n + per - 1) // per))
        out, s = [], 0
        for lo in range(0, n, per):
            cnt = min(per, n - lo)
            draws = []
            for _ in range(K):
                model._forward_encoded_raw(cache, rows.data_ptr() + 4 * lo, cnt, True, seeds[s])
                s += 1
                draws.append(model._ws_view("scores", (cnt, nc)).clone())
            out.append(torch_stats(torch.stack(draws), thr))
        model.check_cluster("bench_uncertainty encoded")
        return [torch.cat(x, 0) for x in zip(*out)]

    results = []
    for K in (8, 32):
        forms = {"pass": lambda: run_pass(K), "model_loop": lambda: model_loop(K),
                 "encoded_chunk": lambda: encoded_separate(K, COLUMNS // K), "encoded_256": lambda: encoded_separate(K, COLUMNS)}
        for fn in forms.values():                                 # warm-up: workspace, allocator blocks, first-call set-up
            fn()
        dev_ms = {k: [] for k in forms}
        wall_ms = {k: [] for k in forms}
        for r in range(args.rounds):
            for k, fn in forms.items():
                d, w = timed(fn)
                dev_ms[k].append(d); wall_ms[k].append(w)
        med = {k: sorted(v)[len(v) // 2] for k, v in dev_ms.items()}
        print(f"pass: K={K}: " + ", ".join(f"{k} {med[k]:.2f} ms" for k in forms) + f" (device, median of {args.rounds})", file=sys.stderr,
              flush=True)
        # the forms compute the same figures from other masks: their means over the corpus agree to the sampling error
        a, b = run_pass(K), model_loop(K)
        results.append({"passes": K, "columns": COLUMNS, "batch": BATCH, "chunks": (n + COLUMNS // K - 1) // (COLUMNS // K),
                        "device_ms": {k: _range(v) for k, v in dev_ms.items()}, "wall_ms": {k: _range(v) for k, v in wall_ms.items()},
                        "speedup_over_model_loop": med["model_loop"] / med["pass"],
                        "speedup_over_encoded_chunk": med["encoded_chunk"] / med["pass"],
                        "speedup_over_encoded_256": med["encoded_256"] / med["pass"],
                        "pass_beats_model_loop_beyond_spread": min(dev_ms["model_loop"]) > max(dev_ms["pass"]),
                        "pass_beats_encoded_chunk_beyond_spread": min(dev_ms["encoded_chunk"]) > max(dev_ms["pass"]),
                        "pass_beats_encoded_256_beyond_spread": min(dev_ms["encoded_256"]) > max(dev_ms["pass"]),
                        "corpus_mean_of_mean": [float(a.mean.mean()), float(b[0].mean())],
                        "corpus_mean_of_mutual_info": [float(a.mutual_info.mean()), float(b[4].mean())]})

    # ---- the reduce launch alone, queued behind a blocker
    big = torch.randn(8192, 8192, device=dev)
    sink = torch.empty_like(big)
    torch.mm(big, big, out=sink)
    lib, s = _lib.load(), _lib.stream_ptr()
    reduce = []
    for B, K in ((8, 32), (32, 8), (1, 256)):
        W = 6
        p = torch.rand(B * K, W, device=dev)
        t = torch.full((W,), thr, device=dev)
        tabs = torch.empty(6, B, W, dtype=torch.float64, device=dev)
        draws = torch.empty(B, K, W, device=dev)
        out = _lib.McOut(*(tabs[i].data_ptr() for i in range(6)), draws.data_ptr())
        launch = lambda: lib.mmda_mc_reduce(p.data_ptr(), B, K, W, t.data_ptr(), 1, ctypes.byref(out), None, 0, s)
        for _ in range(20):
            _lib.check(launch(), "mc_reduce")
        us = []
        for r in range(args.rounds):
            b0, e0, e1 = ev(), ev(), ev()
            torch.cuda.synchronize()
            b0.record()
            torch.mm(big, big, out=sink); torch.mm(big, big, out=sink)
            t0 = time.perf_counter()
            e0.record()
            for _ in range(args.reduce_reps):
                launch()
            e1.record()
            host_ms = (time.perf_counter() - t0) * 1e3
            torch.cuda.synchronize()
            blk_ms = b0.elapsed_time(e0)
            if host_ms >= blk_ms:
                raise SystemExit(f"reduce: B={B} K={K} round {r}: queueing took the host {host_ms:.2f} ms, the blocker {blk_ms:.2f} ms: the "
                                 "launches were not all waiting, nothing is reported")
            us.append(e0.elapsed_time(e1) * 1e3 / args.reduce_reps)
        print(f"reduce: B={B} K={K}: {sorted(us)[len(us) // 2]:.2f} us per queued launch", file=sys.stderr, flush=True)
        reduce.append({"B": B, "K": K, "W": W, "bytes_read": B * K * W * 4, "bytes_written": B * W * 8 * 6 + B * K * W * 4,
                       "launches_per_round": args.reduce_reps, "us_per_launch": _range(us)})
    print(json.dumps({"worker": "pass", "device": torch.cuda.get_device_name(0), "passes": results, "reduce": reduce}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reduce-reps", type=int, default=200)
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds the GPU step (a child process) may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uncertainty.json"))
    ap.add_argument("--worker", choices=["pass"])
    args = ap.parse_args()
    if args.worker == "pass":
        return worker_pass(args)

    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "pass", "--n", str(args.n), "--seed", str(args.seed),
           "--rounds", str(args.rounds), "--reduce-reps", str(args.reduce_reps)]
    try:
        q = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.step_timeout)      # the child's stderr is ours: progress lines
    except subprocess.TimeoutExpired:
        raise SystemExit(f"pass: no result after {args.step_timeout} s")
    if q.returncode != 0:
        sys.stderr.write(q.stdout)
        raise SystemExit(f"pass: exit status {q.returncode}")
    res = json.loads(q.stdout.strip().splitlines()[-1])
    line = json.dumps({"bench": "uncertainty", "device": res["device"], "n": args.n, "seed": args.seed, "precision": "bf16",
                       "vocab": VOCAB, "passes": res["passes"], "reduce": res["reduce"]})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
