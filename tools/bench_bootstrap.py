"""Bootstrap intervals (mmda_amd/bootstrap.py) on the GPU box: the three device passes at R replicates -- decisions (pack + counts +
figures), ranking (the sort, then one workgroup per replicate and class) and the summary -- against the loop they replace.

    python tools/bench_bootstrap.py [--out profiles/bootstrap.json]
                                seeded synthetic (n, 6) tables of the dev / test / train split sizes (1871, 4662, 16326 rows; MOSEI-like
                                imbalance), R = --replicates (2000).  Per size, --rounds rounds:
                                  decisions / ranking / summary   queued: the pass's launches between one device-event pair,
                                              milliseconds (device time); wall: host wall clock of one pass ending in the read-back of
                                              its table
                                  loop        what the passes replace, on the same device tables: per replicate, index the tables with
                                              the replicate's materialised indices (uploaded beforehand: no torch.randint in the
                                              timing), DeviceEval.update + result(), ranking_metrics(...).as_dict().  Timed over
                                              --loop-replicates replicates (20) per round; `ms_per_replicate` is measured,
                                              `ms_at_R` is that times R -- an extrapolation, marked as one.
                                The device tables are compared with the host restatement (three replicates) before anything is timed.
    python tools/bench_bootstrap.py --worker run   the measuring process by itself (prints its JSON line)

The parent process never opens the GPU: the measurement is a child process with a time limit (--step-timeout).  Needs the MI355X:
there is no fall-back.  Prints one JSON line and writes it to --out."""
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


def worker_run(args):
    import time
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_bootstrap needs the MI355X (no CPU path)")
    from mmda_amd import bootstrap as bt
    from mmda_amd import ranking_metrics
    from mmda_amd.utils.eval import DeviceEval
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    R, tables = args.replicates, []
    for name, n in SPLITS:
        s, t = synth_table(n, args.seed)
        lab = (s > np.float32(0.35)).astype(np.float32)
        sd, td, ld = (torch.from_numpy(x).to(dev) for x in (s, t, lab))
        bs = bt.Bootstrap(n, R, args.seed, dev)
        plan = bt.boot_plan(n, 6, R)

        # the device agrees with the host restatement before anything is timed
        small = bt.Bootstrap(n, 3, args.seed, dev)
        st, fig = bt.decisions_host(lab, t, args.seed, 3)
        m3, r3 = small.decisions(ld, td), small.ranking(sd, td)
        want = bt.ranking_host(s, t, args.seed, 3).reshape(4, -1)
        got = r3.figures.cpu().numpy()
        if not (np.array_equal(m3.state.cpu().numpy(), st) and np.nanmax(np.abs(m3.figures.cpu().numpy() - fig)) <= 8 * 2.0 ** -52
                and np.array_equal(np.isnan(got), np.isnan(want)) and np.nanmax(np.abs(got - want)) <= n * 2.0 ** -52):
            raise SystemExit(f"{name}: the device tables differ from the host's, nothing is reported")

        passes = {"decisions": lambda: bs.decisions(ld, td).figures, "ranking": lambda: bs.ranking(sd, td).figures}
        m, r = bs.decisions(ld, td), bs.ranking(sd, td)
        passes["summary"] = lambda: (m.summary().table, r.summary().table)[1]
        idx = torch.from_numpy(bt.resample_indices(args.seed, args.loop_replicates, n)).to(dev)

        def loop():
            for j in idx:
                e = DeviceEval(6, dev)
                e.update(ld[j], td[j])
                e.result()
                ranking_metrics(sd[j], td[j]).as_dict()

        for fn in passes.values():
            fn()
        loop()
        queued, wall, loop_ms = {k: [] for k in passes}, {k: [] for k in passes}, []
        for _ in range(args.rounds):
            for k, fn in passes.items():
                e0, e1 = ev(), ev()
                torch.cuda.synchronize()
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                queued[k].append(e0.elapsed_time(e1))
                t0 = time.perf_counter()
                fn().cpu()
                wall[k].append((time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loop()
            loop_ms.append((time.perf_counter() - t0) * 1e3 / args.loop_replicates)
        row = {"split": name, "n": n, "C": 6, "R": R,
               "plan": {"form": plan.form, "wgs_per_replicate": plan.wgs_per_replicate, "lds_bytes": plan.lds_bytes,
                        "rank_lds_bytes": plan.rank_lds_bytes},
               "queued_ms": {k: _range(v) for k, v in queued.items()}, "wall_ms": {k: _range(v) for k, v in wall.items()},
               "loop": {"replicates_timed": args.loop_replicates, "ms_per_replicate": _range(loop_ms),
                        "ms_at_R_extrapolated": _range([x * R for x in loop_ms])}}
        print(f"{name} n = {n}: " + ", ".join(f"{k} {v['min']:.2f} - {v['max']:.2f} ms queued" for k, v in row["queued_ms"].items())
              + f"; loop {row['loop']['ms_per_replicate']['min']:.2f} - {row['loop']['ms_per_replicate']['max']:.2f} ms per replicate",
              file=sys.stderr, flush=True)
        tables.append(row)
    print(json.dumps({"worker": "run", "device": torch.cuda.get_device_name(0), "tables": tables}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replicates", type=int, default=2000)
    ap.add_argument("--loop-replicates", type=int, default=20, help="replicates of the replaced loop that are timed per round")
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds the GPU step (a child process) may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bootstrap.json"))
    ap.add_argument("--worker", choices=["run"])
    args = ap.parse_args()
    if args.worker == "run":
        return worker_run(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "run", "--seed", str(args.seed), "--rounds", str(args.rounds),
           "--replicates", str(args.replicates), "--loop-replicates", str(args.loop_replicates)]
    try:
        q = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.step_timeout)      # the child's stderr is ours: progress lines
    except subprocess.TimeoutExpired:
        raise SystemExit(f"run: no result after {args.step_timeout} s")
    if q.returncode != 0:
        sys.stderr.write(q.stdout)
        raise SystemExit(f"run: exit status {q.returncode}")
    res = json.loads(q.stdout.strip().splitlines()[-1])
    line = json.dumps({"bench": "bootstrap", "device": res["device"], "seed": args.seed, "classes": 6, "replicates": args.replicates,
                       "rounds": args.rounds, "tables": res["tables"]})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
