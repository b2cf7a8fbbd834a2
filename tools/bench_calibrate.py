"""Threshold calibration (mmda_amd/calibrate.py) on the GPU box: the sweep launch by itself, a calibration pass against an evaluation
pass, and selecting from a stored table against the loop this took before the sweep existed.

    python tools/bench_calibrate.py [--out profiles/calibrate.json]
                                n = 4096 seeded synthetic samples (tools/bench_infer.py's), MOSEI widths, V = 20 000, bf16, C = 6, K = 99
                                  (a) update     one mmda_calib_accumulate launch (histogram + pair counts) over B = 32 and B = 256 rows
                                                 and over the whole 4096-row table: --reps launches queued behind a blocking matrix
                                                 product, one device-event pair around them (the method of tools/bench_infer.py)
                                  (b) pass       Solver.calibrate("dev") against Solver.eval("dev") over the same DeviceLoader, B = 256:
                                                 the same forwards; the sweep launch + select + one table read-back in the place of
                                                 DeviceEval's launches + label concatenation + read-back
                                  (c) select     ThresholdSweep over the stored (4096, 6) score table: update + select + table(),
                                                 against 99 x (scores > t, DeviceEval.update, result()) -- one read-back per candidate
                                --rounds rounds, the forms of a comparison taking turns inside a round; (b) and (c) are host wall-clock
                                times of whole operations that end in a read-back (the device-event time is reported beside them).
    python tools/bench_calibrate.py --worker run    the measuring process by itself (prints its JSON line)

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

from tools.bench_infer import VOCAB, _range, synth_samples      # noqa: E402


class ListLoader:
    def __init__(self, batches):
        self.batches = batches
        self.dataset = self

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


def worker_run(args):
    import time
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_calibrate needs the MI355X (no CPU path)")
    from mmda_amd import MISA, DeviceDataset, DeviceLoader, ThresholdSweep, _lib, make_config
    from mmda_amd.solver import Solver
    from mmda_amd.utils.eval import DeviceEval
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ds = DeviceDataset.from_samples(synth_samples(args.n, args.seed), dev)
    torch.manual_seed(args.seed)
    cfg = make_config(precision="bf16", device="cuda:0", vocab_size=VOCAB)
    model = MISA(cfg).to(dev).eval()
    solver = Solver(cfg, cfg, cfg, ListLoader([]), DeviceLoader(ds, 256), ListLoader([]), is_train=False, model=model).build()
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

    def rounds(forms):
        for fn in forms.values():                                    # warm-up
            fn()
        dev_ms, wall_ms = {k: [] for k in forms}, {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, fn in forms.items():
                d, w = timed(fn)
                dev_ms[k].append(d); wall_ms[k].append(w)
        return {"device_ms": {k: _range(v) for k, v in dev_ms.items()}, "wall_ms": {k: _range(v) for k, v in wall_ms.items()}}

    # the stored table: the model's own scores of the corpus, and labels with MOSEI-like imbalance
    scores = solver.infer("dev", fields=("scores",)).scores.contiguous()
    rng = np.random.default_rng(args.seed)
    truth = torch.from_numpy((rng.random((args.n, 6)) < np.array([0.5, 0.3, 0.2, 0.15, 0.1, 0.05])).astype(np.float32)).to(dev)

    # ---- (a) the sweep launch alone, queued behind a blocker
    big = torch.randn(8192, 8192, device=dev)
    sink = torch.empty_like(big)
    torch.mm(big, big, out=sink)
    update = []
    for rows in (32, 256, args.n):
        sw = ThresholdSweep(6, None, dev)
        s, t = scores[:rows].contiguous(), truth[:rows].contiguous()
        lib, stream = sw._lib, _lib.stream_ptr()
        launch = lambda: lib.mmda_calib_accumulate(s.data_ptr(), t.data_ptr(), rows, 6, sw.grid_dev.data_ptr(), sw.K, sw._counts.data_ptr(),
                                                   sw._pairs_ptr, stream)
        for _ in range(20):
            _lib.check(launch(), "mmda_calib_accumulate")
        us = []
        for r in range(args.rounds):
            b0, e0, e1 = ev(), ev(), ev()
            torch.cuda.synchronize()
            b0.record()
            torch.mm(big, big, out=sink); torch.mm(big, big, out=sink)
            t0 = time.perf_counter()
            e0.record()
            for _ in range(args.reps):
                launch()
            e1.record()
            host_ms = (time.perf_counter() - t0) * 1e3
            torch.cuda.synchronize()
            blk_ms = b0.elapsed_time(e0)
            if host_ms >= blk_ms:
                raise SystemExit(f"update: rows={rows} round {r}: queueing took the host {host_ms:.2f} ms, the blocker {blk_ms:.2f} ms: the "
                                 "launches were not all waiting, nothing is reported")
            us.append(e0.elapsed_time(e1) * 1e3 / args.reps)
        print(f"update: rows={rows}: {sorted(us)[len(us) // 2]:.2f} us per queued launch", file=sys.stderr, flush=True)
        update.append({"rows": rows, "K": sw.K, "launches_per_round": args.reps, "us_per_launch": _range(us)})

    # ---- (b) a calibration pass against an evaluation pass, the same loader
    passes = rounds({"eval": lambda: solver.eval("dev"), "calibrate": lambda: solver.calibrate("dev")})
    print("pass: " + ", ".join(f"{k} {v['median']:.2f} ms" for k, v in passes["wall_ms"].items()) + " (wall, median)", file=sys.stderr,
          flush=True)

    # ---- (c) selecting from the stored table: sweep + select + table() against one DeviceEval pass per candidate
    grid = ThresholdSweep(6, None, dev).grid

    def sweep_select():
        sw = ThresholdSweep(6, None, dev)
        sw.update(scores, truth)
        thr = sw.select("f1", per_class=True)
        return thr, sw.table()

    def candidate_loop():
        best = None
        for t in grid.tolist():
            acc = DeviceEval(6, dev)
            acc.update((scores > t).float(), truth)
            m = acc.result()[2]
            if best is None or m["f1"] > best[0]:
                best = (m["f1"], t)
        return best

    select = rounds({"sweep_select_table": sweep_select, "candidate_loop": candidate_loop})
    print("select: " + ", ".join(f"{k} {v['median']:.3f} ms" for k, v in select["wall_ms"].items()) + " (wall, median)", file=sys.stderr,
          flush=True)
    model.check_cluster("bench_calibrate")
    print(json.dumps({"worker": "run", "device": torch.cuda.get_device_name(0), "update": update, "pass": passes, "select": select}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds the GPU step (a child process) may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "calibrate.json"))
    ap.add_argument("--worker", choices=["run"])
    args = ap.parse_args()
    if args.worker == "run":
        return worker_run(args)

    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "run", "--n", str(args.n), "--seed", str(args.seed),
           "--rounds", str(args.rounds), "--reps", str(args.reps)]
    try:
        q = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.step_timeout)      # the child's stderr is ours: progress lines
    except subprocess.TimeoutExpired:
        raise SystemExit(f"run: no result after {args.step_timeout} s")
    if q.returncode != 0:
        sys.stderr.write(q.stdout)
        raise SystemExit(f"run: exit status {q.returncode}")
    res = json.loads(q.stdout.strip().splitlines()[-1])
    line = json.dumps({"bench": "calibrate", "device": res["device"], "n": args.n, "seed": args.seed, "precision": "bf16",
                       "vocab": VOCAB, "classes": 6, "K": 99, "update": res["update"], "pass": res["pass"], "select": res["select"]})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
