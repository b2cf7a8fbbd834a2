"""Nearest neighbours and the Trust Score (mmda_amd/neighbours.py, csrc/knn.hip) on the GPU box, against the torch form they replace.

    python tools/bench_trust.py [--out profiles/trust.json]
                                seeded standard-normal tables of the dev / test x train sizes (1871 / 4662 x 16326 rows, D = 768,
                                C = 6: 12 sets).  Per pair of sizes, --rounds rounds, each between one device-event pair (device time,
                                milliseconds), the work buffer allocated beforehand:
                                  knn_k1 / knn_k10   mmda_knn_sets at k = 1 / k = 10, S = 12
                                  self_k10           the train x train self-search at k = 10 (the density filter's radii)
                                  fit_score          TrustIndex.fit(alpha = 0.25) + .score end to end
                                  torch_*            the torch form on the same device tables: |q|^2 + |b|^2 - 2 q b^T as one matmul,
                                                     then per set a masked topk (the Q x N matrix is written and read 12 times)
                                `floor_fraction`: the f32-MFMA floor 2 Q N D / 155 TF over the kernel's minimum.
                                The kernel's row numbers are compared with the torch form's before anything is timed (where the
                                dot form ties or rounds differently the reported distances must agree to 1e-3 relative instead).
    python tools/bench_trust.py --worker run   the measuring process by itself (prints its JSON line)

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

TRAIN, D, C = 16326, 768, 6
QUERIES = (("dev", 1871), ("test", 4662))
RATES = (0.5, 0.3, 0.2, 0.15, 0.1, 0.05)
MFMA_F32_TFLOPS = 155.0


def _range(xs):
    s = sorted(xs)
    return {"min": s[0], "median": s[len(s) // 2], "max": s[-1], "rounds": list(xs)}


def torch_knn_sets(q, b, member, S, k):
    """The form the kernel replaces: the whole distance matrix, then a masked topk per set"""
    import torch
    d = ((q * q).sum(dim=1, keepdim=True) + (b * b).sum(dim=1).unsqueeze(0)) - 2.0 * (q @ b.t())
    dist, index = [], []
    for s in range(S):
        out = (member >> s) & 1
        v, i = torch.topk(d.masked_fill((out == 0).unsqueeze(0), float("inf")), k, dim=1, largest=False)
        dist.append(v)
        index.append(i)
    return torch.stack(dist, 1), torch.stack(index, 1)


def torch_fit_score(base, truth, q, labels, members, k, alpha):
    import torch
    S = 2 * C
    bits = torch.arange(S, device=base.device).unsqueeze(0)
    inside = ((members.unsqueeze(1) >> bits) & 1).bool()
    radius = torch.where(inside, torch_knn_sets(base, base, members, S, k)[0][:, :, k - 1], torch.full((), float("inf"), device=base.device))
    m = inside.sum(dim=0)
    rank = torch.ceil((1.0 - alpha) * m.double()).long()
    thr = torch.sort(radius, dim=0)[0].gather(0, (rank - 1).clamp(0).unsqueeze(0))
    kept = inside & ((radius <= thr) | (m < k).unsqueeze(0))
    members = (kept.int() << bits.int()).sum(dim=1).int()
    dist = torch_knn_sets(q, base, members, S, 1)[0][:, :, 0].clamp_min(0)
    y = (labels > 0).long()
    cols = 2 * torch.arange(C, device=base.device).unsqueeze(0)
    p, o = dist.gather(1, cols + y), dist.gather(1, cols + 1 - y)
    return o.double().sqrt() / (p.double().sqrt() + 1e-12)


def worker_run(args):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_trust needs the MI355X (no CPU path)")
    from mmda_amd import TrustIndex, ops
    from mmda_amd.neighbours import set_members
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rng = np.random.default_rng(args.seed)
    base = torch.tensor(rng.standard_normal((TRAIN, D)).astype(np.float32)).to(dev)
    truth = torch.tensor((rng.random((TRAIN, C)) < np.array(RATES)).astype(np.float32)).to(dev)
    members = set_members(truth)
    S = 2 * C

    def timed(fn):
        fn()
        out = []
        for _ in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1))
        return _range(out)

    def agree(q, k):
        got_d, got_i = ops.knn_sets(q, base, members, S, k)
        want_d, want_i = torch_knn_sets(q, base, members, S, k)
        same = (got_i.long() == want_i)
        close = ((got_d - want_d).abs() <= 1e-3 * want_d.abs().clamp_min(1e-6))
        if not bool((same | close).all()):
            raise SystemExit("the kernel's neighbours differ from the torch form's, nothing is reported")
        return float(same.float().mean())

    def knn_row(q, k, name, exclude_self=False):
        Q = int(q.shape[0])
        plan = ops.knn_plan(Q, TRAIN, D, S, k)
        work = torch.empty(plan["work_bytes"], dtype=torch.uint8, device=dev)
        ours = timed(lambda: ops.knn_sets(q, base, members, S, k, exclude_self, work=work))
        theirs = timed(lambda: torch_knn_sets(q, base, members, S, k))
        floor_ms = 2.0 * Q * TRAIN * D / (MFMA_F32_TFLOPS * 1e12) * 1e3
        row = {"what": name, "Q": Q, "N": TRAIN, "D": D, "S": S, "k": k,
               "plan": {f: plan[f] for f in ("tile_q", "slab_rows", "slabs", "merge", "grid_x", "grid_y", "lds_bytes", "work_bytes")},
               "kernel_ms": ours, "torch_ms": theirs, "torch_over_kernel": theirs["min"] / ours["min"],
               "mfma_floor_ms": floor_ms, "floor_fraction": floor_ms / ours["min"]}
        print(f"{name} Q = {Q}: kernel {ours['min']:.2f} - {ours['max']:.2f} ms, torch {theirs['min']:.2f} - {theirs['max']:.2f} ms, "
              f"floor {floor_ms:.2f} ms ({row['floor_fraction']:.2f} of the kernel's time)", file=sys.stderr, flush=True)
        return row

    rows = []
    for name, n in QUERIES:
        q = torch.tensor(rng.standard_normal((n, D)).astype(np.float32)).to(dev)
        labels = torch.tensor((rng.random((n, C)) < 0.3).astype(np.float32)).to(dev)
        same = {k: agree(q, k) for k in (1, 10)}
        rows.append(dict(knn_row(q, 1, f"{name}_knn_k1"), same_rows_as_torch=same[1]))
        rows.append(dict(knn_row(q, 10, f"{name}_knn_k10"), same_rows_as_torch=same[10]))
        ours = timed(lambda: TrustIndex.fit(base, truth, k=10, alpha=0.25).score(q, labels).trust)
        theirs = timed(lambda: torch_fit_score(base, truth, q, labels, members, 10, 0.25))
        rows.append({"what": f"{name}_fit_score", "Q": n, "N": TRAIN, "k": 10, "alpha": 0.25, "kernel_ms": ours, "torch_ms": theirs,
                     "torch_over_kernel": theirs["min"] / ours["min"]})
        print(f"{name} fit + score: ours {ours['min']:.2f} - {ours['max']:.2f} ms, torch {theirs['min']:.2f} - {theirs['max']:.2f} ms",
              file=sys.stderr, flush=True)
    rows.append(knn_row(base, 10, "self_k10", exclude_self=False))
    print(json.dumps({"worker": "run", "device": torch.cuda.get_device_name(0), "rows": rows}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds the GPU step (a child process) may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trust.json"))
    ap.add_argument("--worker", choices=["run"])
    args = ap.parse_args()
    if args.worker == "run":
        return worker_run(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "run", "--seed", str(args.seed), "--rounds", str(args.rounds)]
    try:
        q = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.step_timeout)      # the child's stderr is ours: progress lines
    except subprocess.TimeoutExpired:
        raise SystemExit(f"run: no result after {args.step_timeout} s")
    if q.returncode != 0:
        sys.stderr.write(q.stdout)
        raise SystemExit(f"run: exit status {q.returncode}")
    res = json.loads(q.stdout.strip().splitlines()[-1])
    line = json.dumps({"bench": "trust", "device": res["device"], "seed": args.seed, "rounds": args.rounds,
                       "mfma_f32_tflops": MFMA_F32_TFLOPS, "rows": res["rows"]})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
