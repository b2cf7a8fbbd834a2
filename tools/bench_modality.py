"""Modality masking by itself (GPU box): the masked gather beside the plain one, the pass over the eight keep sets beside what it replaces,
and the Shapley collector.

    python tools/bench_modality.py [--out profiles/modality.json]
    python tools/bench_modality.py --worker gather | pass | attrib      one measuring process by itself (prints its JSON line)

  gather   ``mmda_collate_gather`` and ``mmda_collate_gather_masked`` (p = 0 / keep = 7; p = (0.3, 0.3, 0.3); keep = 1) at B = 32 and 256,
           T = 50, ragged lengths, timed as tools/bench_input_pipeline.py times the gather: --gather-reps launches queued behind a
           blocking matrix product, one event pair around them.  The yardstick of the masked launch is the plain launch of the SAME job.
  pass     ``ModalityPass.run`` over --n-pass synthetic samples of lengths 5 .. 50, bf16, at B = 32 and 256, beside eight
           ``InferencePass.run(keep=k)`` calls and beside the host loop they replace (per batch and keep set: read the batch back, mask it
           in numpy, upload it, evaluate, read the scores back).  Wall time around a synchronised run.
  attrib   the ``mmda_modality_attrib`` launch at n = 1871 and 16 326, C = 6, queued like the gather.

Every figure is min - max (and the median) of --rounds rounds.  The parent process never opens the GPU: each measurement is a child
process with a time limit (--step-timeout).  Needs the MI355X: there is no fall-back.  Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_input_pipeline import _range, synth_samples  # noqa: E402

WORKERS = ("gather", "pass", "attrib")


def _queued(torch, dev):
    """bench_input_pipeline's method: (us per launch, blocker ms, host ms) of `reps` launches queued behind two large matrix products"""
    import time
    big = torch.randn(8192, 8192, device=dev)
    sink = torch.empty_like(big)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    torch.mm(big, big, out=sink)

    def queued_us(launch, reps):
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

    def rounds(name, launch, reps, n_rounds):
        for _ in range(20):
            launch()
        us = []
        for r in range(n_rounds):
            u, blk_ms, host_ms = queued_us(launch, reps)
            if host_ms >= blk_ms:
                raise SystemExit(f"{name}: round {r}: queueing {reps} launches took the host {host_ms:.2f} ms, the blocker "
                                 f"{blk_ms:.2f} ms: the launches were not all waiting, nothing is reported")
            us.append(u)
        print(f"{name}: {sorted(us)[len(us) // 2]:.2f} us per queued launch (median of {n_rounds} rounds of {reps})", file=sys.stderr,
              flush=True)
        return _range(us)

    return rounds


def _device(torch):
    if not torch.cuda.is_available():
        raise SystemExit("bench_modality needs the MI355X (no CPU path)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    return dev


def worker_gather(args):
    import numpy as np
    import torch
    from mmda_amd import DeviceDataset, _lib, ops
    dev = _device(torch)
    lib, stream = _lib.load(), _lib.stream_ptr()
    ds = DeviceDataset.from_samples(synth_samples(args.n, args.seed), dev)
    T = int(ds.lengths.max())
    rng = np.random.default_rng(args.seed + 1)
    longest = np.flatnonzero(ds.lengths == T)
    rounds = _queued(torch, dev)
    src = (ds.words, ds.visual, ds.acoustic, ds.offsets, ds.emo, ds.sentiment)
    results = []
    for B in (32, 256):
        idx = rng.choice(len(ds), size=B, replace=False)
        idx[0] = longest[0]
        idx = idx[np.argsort(-ds.lengths[idx], kind="stable")]
        order = torch.from_numpy(idx.astype(np.int32)).to(dev)
        out = ops.collate_gather(*src, order, T)
        kept = torch.empty(B, dtype=torch.uint8, device=dev)
        # the entry points themselves, arguments made once: the host must queue a round's launches while the blocker still runs
        head = tuple(_lib.ptr(x) for x in src) + (order.data_ptr(), B, T, ds.dv, ds.da, 1)
        tail = tuple(_lib.ptr(x) for x in out)
        P = lambda *p: _lib.ModalityP((_lib.C.c_float * 3)(*p))
        masked = lambda keep, p, seed: (lambda: _lib.check(lib.mmda_collate_gather_masked(*head, keep, p, seed, 0, *tail, kept.data_ptr(),
                                                                                          stream), "mmda_collate_gather_masked"))
        forms = {"plain": lambda: _lib.check(lib.mmda_collate_gather(*head, *tail, stream), "mmda_collate_gather"),
                 "masked_p0_keep7": masked(7, P(0.0, 0.0, 0.0), 0), "masked_p0.3": masked(7, P(0.3, 0.3, 0.3), 1),
                 "masked_keep1": masked(1, P(0.0, 0.0, 0.0), 0)}
        row = {"batch": B, "T": T, "positions": int(ds.lengths[idx].sum()), "launches_per_round": args.gather_reps, "us_per_launch": {}}
        for name, launch in forms.items():
            row["us_per_launch"][name] = rounds(f"gather B={B} {name}", launch, args.gather_reps, args.rounds)
        row["us_per_launch"]["plain_again"] = rounds(f"gather B={B} plain again", forms["plain"], args.gather_reps, args.rounds)
        results.append(row)
    print(json.dumps({"worker": "gather", "device": torch.cuda.get_device_name(0), "result": results}))


def worker_attrib(args):
    import torch
    from mmda_amd import _lib
    dev = _device(torch)
    lib = _lib.load()
    rounds = _queued(torch, dev)
    results = []
    for n in (1871, 16326):
        C = 6
        V = torch.rand(8, n, C, device=dev)
        phi, loo = torch.empty(n, 3, C, device=dev), torch.empty(n, 3, C, device=dev)
        dom = torch.empty(n, C, dtype=torch.int32, device=dev)
        counts = torch.empty(3, C, dtype=torch.int64, device=dev)
        stream = _lib.stream_ptr()
        launch = lambda: _lib.check(lib.mmda_modality_attrib(V.data_ptr(), n, C, phi.data_ptr(), loo.data_ptr(), dom.data_ptr(),
                                                            counts.data_ptr(), stream), "mmda_modality_attrib")
        results.append({"n": n, "C": C, "launches_per_round": args.gather_reps,
                        "us_per_call": rounds(f"attrib n={n}", launch, args.gather_reps, args.rounds),
                        "note": "one call = the 8-byte-per-cell clear of counts on the stream and the launch"})
    print(json.dumps({"worker": "attrib", "device": torch.cuda.get_device_name(0), "result": results}))


def worker_pass(args):
    import time
    import numpy as np
    import torch
    from mmda_amd import DeviceDataset, InferencePass, MISA, ModalityPass, make_config, modality
    from mmda_amd.data import collate_fn
    from mmda_amd.inference import inference_plan
    dev = _device(torch)
    samples = synth_samples(args.n_pass, args.seed)
    ds = DeviceDataset.from_samples(samples, dev)
    cfg = make_config(vocab_size=20000, precision="bf16", device=str(dev))
    torch.manual_seed(0)
    m = MISA(cfg).to(dev).eval()

    def timed(fn):
        ms = []
        fn()
        for _ in range(args.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return _range(ms)

    results = []
    for B in (32, 256):
        mp, ip = ModalityPass(m, ("scores", "tcp")), InferencePass(m, ("scores", "tcp"))
        plan, bounds = inference_plan(ds.lengths, B, "length")
        host_batches = [collate_fn([samples[i] for i in plan[lo:hi]]) for lo, hi in zip(bounds[:-1], bounds[1:])]

        def host_loop():
            """what a user does without the pass: per batch and keep set, read the device batch back, mask it in numpy, copy it up,
            evaluate, read the scores back"""
            out = []
            with torch.no_grad():
                for b in host_batches:
                    t, v, a = (x.to(dev) for x in b[:3])
                    for k in range(8):
                        ids, vv, aa = modality.mask_batch(t.cpu().numpy(), v.cpu().numpy(), a.cpu().numpy(), k)
                        s, _ = m(torch.from_numpy(ids).to(dev), torch.from_numpy(vv).to(dev), torch.from_numpy(aa).to(dev), b[5])
                        out.append((s.cpu(), m.tcp.cpu()))
            return out

        row = {"batch": B, "samples": len(ds), "precision": "bf16",
               "ms": {"modality_pass": timed(lambda: mp.run(ds, B)),
                      "eight_inference_passes": timed(lambda: [ip.run(ds, B, keep=k) for k in range(8)]),
                      "host_loop": timed(host_loop)}}
        print(f"pass B={B}: " + ", ".join(f"{k} {v['median']:.1f} ms" for k, v in row["ms"].items()), file=sys.stderr, flush=True)
        results.append(row)
    m.check_cluster("bench_modality")
    print(json.dumps({"worker": "pass", "device": torch.cuda.get_device_name(0), "result": results}))


def assemble(parts, device):
    """The document the tool prints and writes, from the workers' results"""
    return {"bench": "modality", "device": device, "gather": parts.get("gather"), "pass": parts.get("pass"), "attrib": parts.get("attrib")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384, help="samples of the gather's dataset")
    ap.add_argument("--n-pass", type=int, default=4096, help="samples the passes run over")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--gather-reps", type=int, default=200)
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds each GPU step (a child process) may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "modality.json"))
    ap.add_argument("--worker", choices=WORKERS)
    ap.add_argument("--only", choices=WORKERS, action="append", help="run these workers only (default: all three)")
    args = ap.parse_args()
    if args.worker:
        return {"gather": worker_gather, "pass": worker_pass, "attrib": worker_attrib}[args.worker](args)

    parts, device = {}, None
    for w in args.only or WORKERS:
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", w, "--n", str(args.n), "--n-pass", str(args.n_pass), "--seed",
               str(args.seed), "--rounds", str(args.rounds), "--gather-reps", str(args.gather_reps)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.step_timeout)  # the child's stderr is ours: progress lines
        except subprocess.TimeoutExpired:
            raise SystemExit(f"{w}: no result after {args.step_timeout} s")
        if p.returncode != 0:
            sys.stderr.write(p.stdout)
            raise SystemExit(f"{w}: exit status {p.returncode}")
        res = json.loads(p.stdout.strip().splitlines()[-1])
        parts[w], device = res["result"], res["device"]
    line = json.dumps(assemble(parts, device))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
