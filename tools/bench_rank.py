"""Ranking metrics (mmda_amd/ranking.py) on the GPU box: the device path -- mmda_rank_counts + mmda_rank_finish over a table that is
already on the device -- against the loop it replaces: read the table back, then count on the host.

    python tools/bench_rank.py [--out profiles/rank.json]
                                seeded synthetic (N, 6) tables of the dev / test / train split sizes (1871, 4662, 16326 rows; informative
                                scores, MOSEI-like imbalance) and their pooled (6 N, 1) forms.  Per table, --rounds rounds, the forms taking
                                turns inside a round:
                                  device      --reps x (counts + finish) between one device-event pair: microseconds per table, the
                                              launches queued back to back (device time), and the host wall clock of ONE counts +
                                              finish + read-back of the (C + 1, 6) table
                                  host_numpy  scores.cpu(), truth.cpu(), rank_counts_host (a sort per class) + figures_from_counts:
                                              host wall clock ending in the table, starting at the read-back
                                  host_sklearn  the same read-back, then roc_auc_score and average_precision_score (both senses) per
                                              class, where scikit-learn can be imported; "not importable" otherwise
                                The device and numpy tables are compared before anything is timed.
    python tools/bench_rank.py --worker run    the measuring process by itself (prints its JSON line); with --splits dev (test, train)
                                only that size: what a kernel trace of one table size is taken from
    python tools/bench_rank.py --trace-summary dev=DEV_kernel_trace.csv train=TRAIN_kernel_trace.csv [--out profiles/rank_kernel_trace.json]
                                no GPU: the kernel-trace CSVs of
                                  rocprofv3 --kernel-trace --stats -d DIR -o NAME --output-format csv -- \
                                      python tools/bench_rank.py --worker run --rounds 2 --reps 20 --splits dev     (then train)
                                grouped by kernel and launch shape (the per-class and the pooled table differ in their grids):
                                dispatches and min / median / max microseconds of each

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

SPLITS = (("dev", 1871), ("test", 4662), ("train", 16326))
RATES = (0.5, 0.3, 0.2, 0.15, 0.1, 0.05)


def _range(xs):
    s = sorted(xs)
    return {"min": s[0], "median": s[len(s) // 2], "max": s[-1], "rounds": list(xs)}


def synth_table(n, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    truth = (rng.random((n, 6)) < np.array(RATES)).astype(np.float32)
    scores = (1.0 / (1.0 + np.exp(-(1.5 * truth - 1.0 + rng.normal(0.0, 1.0, truth.shape))))).astype(np.float32)
    return scores, truth


def trace_summary(args):
    import csv
    import statistics
    out = {"bench": "rank_kernel_trace", "tables": {}}
    for item in args.trace_summary:
        name, path = item.split("=", 1)
        groups = {}
        for r in csv.DictReader(open(path)):
            kernel = r["Kernel_Name"].split("(anonymous namespace)::")[-1].split("(")[0]
            key = (kernel, tuple(int(r[f"Grid_Size_{a}"]) // int(r[f"Workgroup_Size_{a}"]) for a in "XYZ"), int(r["Workgroup_Size_X"]))
            groups.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        out["tables"][name] = [{"kernel": k, "workgroups": list(g), "threads": t, "dispatches": len(v), "us": {
            "min": min(v), "median": statistics.median(v), "max": max(v)}} for (k, g, t), v in sorted(groups.items())]
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


def worker_run(args):
    import time
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_rank needs the MI355X (no CPU path)")
    from mmda_amd import _lib, ranking as rk
    try:
        from sklearn.metrics import average_precision_score, roc_auc_score
    except ImportError:
        roc_auc_score = None
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lib = _lib.load()
    ev = lambda: torch.cuda.Event(enable_timing=True)
    tables = []
    for name, n in SPLITS:
        if args.splits and name not in args.splits:
            continue
        s, t = synth_table(n, args.seed)
        for form, (a, b) in (("per_class", (s, t)), ("pooled", (s.reshape(-1, 1), t.reshape(-1, 1)))):
            N, C = a.shape
            sd, td = torch.from_numpy(np.ascontiguousarray(a)).to(dev), torch.from_numpy(np.ascontiguousarray(b)).to(dev)
            counts = torch.empty(N, C, 4, dtype=torch.int32, device=dev)
            table = torch.empty(C + 1, 6, dtype=torch.float64, device=dev)
            plan = rk.rank_plan(N, C)

            def launch():
                lib.mmda_rank_counts(sd.data_ptr(), td.data_ptr(), N, C, counts.data_ptr(), _lib.stream_ptr())
                lib.mmda_rank_finish(counts.data_ptr(), td.data_ptr(), N, C, 0.95, table.data_ptr(), _lib.stream_ptr())

            def device_once():
                launch()
                return table.cpu().numpy()

            def host_numpy():
                hs, ht = sd.cpu().numpy(), td.cpu().numpy()
                return rk.figures_from_counts(rk.rank_counts_host(hs, ht), ht, 0.95)

            def host_sklearn():
                hs, ht = sd.cpu().numpy(), td.cpu().numpy()
                out = []
                for c in range(C):
                    y = ht[:, c] > 0
                    out.append((roc_auc_score(y, hs[:, c]), average_precision_score(y, hs[:, c]), average_precision_score(~y, -hs[:, c])))
                return out

            # the two paths agree before either is timed
            got, want = device_once(), host_numpy()
            if not (np.array_equal(got[:, [0, 1, 2, 5]], want[:, [0, 1, 2, 5]], equal_nan=True)
                    and np.nanmax(np.abs(got[:, 3:5] - want[:, 3:5])) <= N * 2.0 ** -52):
                raise SystemExit(f"{name} {form}: the device table differs from the host's, nothing is reported")
            forms = {"device": device_once, "host_numpy": host_numpy}
            if roc_auc_score is not None:
                forms["host_sklearn"] = host_sklearn
            for fn in forms.values():
                fn()
            for _ in range(3):
                launch()
            wall = {k: [] for k in forms}
            dev_us = []
            for _ in range(args.rounds):
                e0, e1 = ev(), ev()
                torch.cuda.synchronize()
                e0.record()
                for _ in range(args.reps):
                    launch()
                e1.record()
                torch.cuda.synchronize()
                dev_us.append(e0.elapsed_time(e1) * 1e3 / args.reps)
                for k, fn in forms.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    wall[k].append((time.perf_counter() - t0) * 1e3)
            row = {"split": name, "form": form, "N": N, "C": C, "comparisons": N * N * C,
                   "plan": {"rows_per_wg": plan.rows_per_wg, "tile": plan.tile, "splits": plan.splits,
                            "tiles_per_split": plan.tiles_per_split, "grid": [plan.grid_x, plan.grid_y, plan.grid_z]},
                   "launches_per_round": args.reps, "device_us_per_table": _range(dev_us),
                   "wall_ms": {k: _range(v) for k, v in wall.items()}}
            if roc_auc_score is None:
                row["host_sklearn"] = "not importable"
            print(f"{name} {form} ({N}, {C}): device {row['device_us_per_table']['median']:.1f} us queued, "
                  + ", ".join(f"{k} {v['median']:.3f} ms" for k, v in row["wall_ms"].items()) + " (wall, median)", file=sys.stderr, flush=True)
            tables.append(row)
    print(json.dumps({"worker": "run", "device": torch.cuda.get_device_name(0), "tables": tables}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--splits", nargs="*", choices=[n for n, _ in SPLITS], help="only these table sizes (a kernel trace of one size)")
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds the GPU step (a child process) may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank.json"))
    ap.add_argument("--worker", choices=["run"])
    ap.add_argument("--trace-summary", nargs="+", metavar="NAME=CSV", help="summarise rocprofv3 kernel-trace CSVs instead of measuring")
    args = ap.parse_args()
    if args.trace_summary:
        return trace_summary(args)
    if args.worker == "run":
        return worker_run(args)

    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "run", "--seed", str(args.seed), "--rounds", str(args.rounds),
           "--reps", str(args.reps)] + (["--splits"] + args.splits if args.splits else [])
    try:
        q = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.step_timeout)      # the child's stderr is ours: progress lines
    except subprocess.TimeoutExpired:
        raise SystemExit(f"run: no result after {args.step_timeout} s")
    if q.returncode != 0:
        sys.stderr.write(q.stdout)
        raise SystemExit(f"run: exit status {q.returncode}")
    res = json.loads(q.stdout.strip().splitlines()[-1])
    line = json.dumps({"bench": "rank", "device": res["device"], "seed": args.seed, "classes": 6, "tpr": 0.95, "rounds": args.rounds,
                       "tables": res["tables"]})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
