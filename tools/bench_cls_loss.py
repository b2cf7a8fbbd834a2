"""What the classification criterion costs the fused training step.

    python tools/bench_cls_loss.py [--parent-tree DIR] [--out profiles/cls_loss.json]

B = 32 and B = 256, T = 50, bf16, V = 20 000, dropout on: bench.py's batch.  Every measurement is a process of its own (this file with
--child), so that two builds of the library can take turns: --rounds rounds, and in each round, one after the other,
    parent      the default step of the tree at --parent-tree (a built checkout of the parent commit; left out when not given)
    default     the default step of this tree: no weights, focal_gamma = 0 -- must lie inside the parent's own range
    criterion   this tree with pos_weight = [1, 4, 4, 11, 5, 9] and focal_gamma = 2: the same launches, cls_term in three of them
A child builds one model per batch size and puts one device-event pair around --steps steps after --warmup untimed ones.  The criterion
child also times mmda_label_counts over a 4096-row label table: --count-reps launches back to back between one event pair.

Needs the MI355X: there is no fall-back.  Prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTS = [1.0, 4.0, 4.0, 11.0, 5.0, 9.0]
GAMMA = 2.0


def _range(xs):
    s = sorted(xs)
    return {"min": s[0], "median": s[len(s) // 2], "max": s[-1], "rounds": list(xs)}


def child(args):
    """one tree, one form: {"32": ms per step, "256": ms per step[, "label_counts_us": us per launch]}"""
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    import mmda_amd
    from mmda_amd import _lib, make_config
    from mmda_amd.data import synth_batch
    from mmda_amd.solver import Solver
    assert os.path.abspath(mmda_amd.__file__).startswith(os.path.abspath(args.tree)), mmda_amd.__file__
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    out = {}
    for B in (32, 256):
        torch.manual_seed(0)
        emb = torch.randn(args.vocab, 300, generator=torch.Generator().manual_seed(0))
        cfg = make_config(vocab_size=args.vocab, precision="bf16", device=str(dev), batch_size=B, seq_len=args.seq_len,
                          pretrained_emb=emb.clone())
        m = Solver(cfg, cfg, cfg, None, None, None, is_train=True).build().model
        if args.criterion:
            m.set_cls_loss(WEIGHTS, GAMMA)
        m.train()
        t, v, a, y, emo, lengths, *_ = synth_batch(cfg, B, args.seq_len, seed=B, device=dev)
        step = lambda: m.train_step(t, v, a, lengths, emo, lr=cfg.learning_rate, clip=cfg.clip)
        for _ in range(args.warmup):
            step()
        e0, e1 = ev(), ev()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.steps):
            step()
        e1.record()
        torch.cuda.synchronize()
        m.check_cluster("bench_cls_loss")
        L = m.read_losses()
        if not all(x == x for x in L.values()):
            raise SystemExit(f"non-finite losses: {L}")
        out[str(B)] = e0.elapsed_time(e1) / args.steps
        out[f"cls_{B}"] = L["cls"]
    if args.criterion:
        lib = _lib.load()
        lab = (torch.rand(4096, 6, device=dev) < 0.2).float()
        counts = torch.zeros(6, dtype=torch.int64, device=dev)
        call = lambda: _lib.check(lib.mmda_label_counts(lab.data_ptr(), 4096, 6, counts.data_ptr(), _lib.stream_ptr()), "mmda_label_counts")
        for _ in range(20):
            call()
        e0, e1 = ev(), ev()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.count_reps):
            call()
        e1.record()
        torch.cuda.synchronize()
        out["label_counts_us"] = e0.elapsed_time(e1) * 1e3 / args.count_reps
    print("CHILD " + json.dumps(out), flush=True)


def run_child(args, tree, criterion):
    tree = os.path.abspath(tree)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--steps", str(args.steps), "--warmup", str(args.warmup),
           "--seq-len", str(args.seq_len), "--vocab", str(args.vocab), "--count-reps", str(args.count_reps)]
    if criterion:
        cmd.append("--criterion")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.child_timeout, cwd=tree)
    lines = [x for x in r.stdout.splitlines() if x.startswith("CHILD ")]
    if r.returncode != 0 or not lines:
        # (nothing more is started on the device behind a child that failed)
        raise SystemExit(f"child {tree} criterion={criterion} ended with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads(lines[-1][6:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seq-len", type=int, default=50)
    ap.add_argument("--vocab", type=int, default=20000)
    ap.add_argument("--count-reps", type=int, default=500)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cls_loss.json"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--criterion", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    forms = ([("parent", args.parent_tree, False)] if args.parent_tree else []) + [("default", ROOT, False), ("criterion", ROOT, True)]
    ms = {name: {"32": [], "256": []} for name, _, _ in forms}
    counts_us, cls_values = [], {}
    for r in range(args.rounds):
        for name, tree, criterion in forms:
            got = run_child(args, tree, criterion)
            for B in ("32", "256"):
                ms[name][B].append(got[B])
                cls_values.setdefault(name, {})[B] = got[f"cls_{B}"]
            if "label_counts_us" in got:
                counts_us.append(got["label_counts_us"])
            print(f"round {r} {name}: B=32 {got['32']:.4f}  B=256 {got['256']:.4f} ms/step", file=sys.stderr, flush=True)
    results = []
    for B in ("32", "256"):
        f = {name: _range(ms[name][B]) for name in ms}
        row = {"batch": int(B), "forms_ms_per_step": f, "last_cls_loss": {name: cls_values[name][B] for name in ms},
               "criterion_minus_default_us": 1e3 * (f["criterion"]["median"] - f["default"]["median"])}
        if "parent" in f:
            row["default_overlaps_parent"] = bool(f["default"]["min"] <= f["parent"]["max"] and f["parent"]["min"] <= f["default"]["max"])
            row["default_over_parent"] = f["default"]["median"] / f["parent"]["median"]
        results.append(row)
    line = json.dumps({"bench": "cls_loss", "seq_len": args.seq_len, "precision": "bf16", "vocab": args.vocab, "steps_per_round": args.steps,
                       "rounds": args.rounds, "pos_weight": WEIGHTS, "focal_gamma": GAMMA, "results": results,
                       "label_counts": {"rows": 4096, "classes": 6, "launches_per_round": args.count_reps, "us_per_launch": _range(counts_us)}})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
