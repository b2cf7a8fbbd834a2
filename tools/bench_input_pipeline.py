"""The batch-collating launch of the device-resident dataset by itself (GPU box): ``mmda_collate_gather`` between HIP events.

    python tools/bench_input_pipeline.py [--out profiles/input_pipeline.json]
                                         n = 16 384 seeded synthetic samples, lengths uniform in [5, 50], MOSEI widths; B = 32 and 256 at
                                         T = 50, a ragged batch and one whose samples all have length 50; --gather-reps launches queued
                                         behind a blocking matrix product, one event pair around them, --rounds rounds; the empty pair beside
    python tools/bench_input_pipeline.py --worker gather       the measuring process by itself (prints its JSON line)

What the input side costs a whole epoch -- ``Solver.train_epoch()`` over DataLoader + collate_fn + DevicePrefetcher, over DeviceLoader and
over prebuilt device batches -- is NOT measured here (DESIGN.md section 5 says why); ``epoch_rates`` in the output is null.

The parent process never opens the GPU: the measurement is a child process with a time limit (--step-timeout) that reports each
measured case on stderr as it goes.  Needs the MI355X: there is no fall-back.  Prints one JSON line and writes it to --out."""
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
    """n reference-style samples ((word_ids, visual (L, 35), acoustic (L, 74), words), label (1, 7), segment), seeded"""
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


def worker_gather(args):
    """The gather launch by itself.  The host issues a launch more slowly than the kernel runs, so an event pair around launches that go
    out one by one times the host.  Here --gather-reps launches are queued BEHIND a blocking piece of device work (two large matrix
    products), the event pair around them: the device finds them all waiting and runs them back to back, and the pair's time over their
    number is the kernel plus the dispatch of one queued launch.  A round whose launches were not all queued before the blocker ended is
    refused, not reported.  The same pair around nothing (``event_pair_floor_us``, the whole pair, not per launch) is reported beside."""
    import time
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_input_pipeline needs the MI355X (no CPU path)")
    from mmda_amd import DeviceDataset, ops
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    samples = synth_samples(args.n, args.seed)
    ds = DeviceDataset.from_samples(samples, dev)
    T = int(ds.lengths.max())
    rng = np.random.default_rng(args.seed + 1)
    longest = np.flatnonzero(ds.lengths == T)
    big = torch.randn(8192, 8192, device=dev)
    sink = torch.empty_like(big)
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def queued_us(launch, reps):
        """(us per launch, blocker ms, host ms spent queueing) of `reps` launches queued behind the blocker"""
        b0, e0, e1 = ev(), ev(), ev()
        torch.cuda.synchronize()
        b0.record()
        torch.mm(big, big, out=sink); torch.mm(big, big, out=sink)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(reps):
            launch()
        e1.record()
        host_ms = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / max(reps, 1), b0.elapsed_time(e0), host_ms

    torch.mm(big, big, out=sink)                                      # (the product's own first-call set-up)
    results = []
    for B in (32, 256):
        for kind in ("ragged", "full"):
            if kind == "full":
                idx = rng.choice(longest, size=B, replace=len(longest) < B)
            else:
                idx = rng.choice(len(ds), size=B, replace=False)
                idx[0] = longest[0]
            idx = idx[np.argsort(-ds.lengths[idx], kind="stable")]
            order = torch.from_numpy(idx.astype(np.int32)).to(dev)
            out = ops.collate_gather(ds.words, ds.visual, ds.acoustic, ds.offsets, ds.emo, ds.sentiment, order, T)
            launch = lambda: ops.collate_gather(ds.words, ds.visual, ds.acoustic, ds.offsets, ds.emo, ds.sentiment, order, T, out=out)
            for _ in range(20):
                launch()
            us, floor, blocker = [], [], []
            for r in range(args.rounds):
                u, blk_ms, host_ms = queued_us(launch, args.gather_reps)
                if host_ms >= blk_ms:
                    raise SystemExit(f"gather: B={B} {kind} round {r}: queueing {args.gather_reps} launches took the host {host_ms:.2f} ms, "
                                     f"the blocker {blk_ms:.2f} ms: the launches were not all waiting, nothing is reported")
                us.append(u); blocker.append(blk_ms)
                floor.append(queued_us(lambda: None, 0)[0])
            print(f"gather: B={B} T={T} {kind}: {sorted(us)[len(us) // 2]:.2f} us per queued launch (median of {args.rounds} rounds of "
                  f"{args.gather_reps}; blocker {min(blocker):.1f} ms)", file=sys.stderr, flush=True)
            results.append({"batch": B, "T": T, "lengths": kind, "positions_copied": int(ds.lengths[idx].sum()),
                            "bytes_written": T * B * (8 + 4 * (DV + DA)), "launches_per_round": args.gather_reps,
                            "us_per_launch": _range(us), "event_pair_floor_us": _range(floor)})
    print(json.dumps({"worker": "gather", "device": torch.cuda.get_device_name(0), "result": results}))


def assemble(result, device):
    """The document the tool prints and writes, from the gather worker's result"""
    return {"bench": "input_pipeline", "device": device, "gather": result,
            "epoch_rates": None,
            "epoch_rates_note": "Solver.train_epoch() over DataLoader + DevicePrefetcher, DeviceLoader and prebuilt batches: not measured"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--gather-reps", type=int, default=200)
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds the GPU step (a child process) may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "input_pipeline.json"))
    ap.add_argument("--worker", choices=["gather"])
    args = ap.parse_args()
    if args.worker == "gather":
        return worker_gather(args)

    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "gather", "--n", str(args.n), "--seed", str(args.seed),
           "--rounds", str(args.rounds), "--gather-reps", str(args.gather_reps)]
    try:
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.step_timeout)      # the child's stderr is ours: progress lines
    except subprocess.TimeoutExpired:
        raise SystemExit(f"gather: no result after {args.step_timeout} s")
    if p.returncode != 0:
        sys.stderr.write(p.stdout)
        raise SystemExit(f"gather: exit status {p.returncode}")
    res = json.loads(p.stdout.strip().splitlines()[-1])
    line = json.dumps(assemble(res["result"], res["device"]))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
