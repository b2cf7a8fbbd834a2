"""What reliability and logit scaling cost: the collector launch, a report beside reading the table back for the numpy
definition, and the device fit beside the usual host recipe on the same device table.

    python tools/bench_reliability.py [--out profiles/reliability.json]

The forms of a comparison take turns inside each of --rounds rounds (the spread of a form is its min - max over the rounds):
    collector   mmda_reliab_accumulate over 32, 256, 4096 and 16 326 rows of 6 classes, 15 bins: --reps launches back to back between
                one device-event pair
    report      accumulate + finish over 4096 and 16 326 rows (the figures stay on the device) against table.cpu() and
                reliability.reliability_host, the numpy definition; host clock around a device synchronise
    fit         fit_scaling over 1871 x 6 and 16 326 x 6 in the four (how, per_class) combinations, max_iter = 64, against
                torch.optim.LBFGS(max_iter = 50) over binary_cross_entropy_with_logits of a z + b on the same device table, its result
                read back; host clock around a device synchronise.  The iteration counts reached by both are recorded, and the largest
                difference between their parameters.

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reliability.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from mmda_amd import ReliabilityEval, fit_scaling
    from mmda_amd import reliability as rel
    if not torch.cuda.is_available():
        raise SystemExit("bench_reliability needs the MI355X: there is no fall-back")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    C, M = 6, 15

    def table(n, seed):
        """scores that are too sure of themselves (a0 = 0.5, b0 = 0.7), labels drawn from the true probabilities"""
        rng = np.random.default_rng(seed)
        zs = rng.normal(0.0, 1.5, (n, C))
        y = (rng.random((n, C)) < 1.0 / (1.0 + np.exp(-zs))).astype(np.float32)
        s = (1.0 / (1.0 + np.exp(-(zs - 0.7) / 0.5))).astype(np.float32)
        return torch.from_numpy(s).to(dev), torch.from_numpy(y).to(dev)

    def timed_events(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    def timed_host(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), out

    # ---- the collector launch
    collector = []
    for n in (32, 256, 4096, 16326):
        p, t = table(n, n)
        ev = ReliabilityEval(C, M, dev)

        def launch():
            ev.rows = 0                                              # the row limit of a state is the caller's count: this loop adds the same rows again
            ev.update(p, t)
        for _ in range(20):
            launch()
        us = [1e3 * timed_events(launch, args.reps) for _ in range(args.rounds)]
        collector.append({"rows": n, "us_per_launch": _range(us)})
    # ---- a report: on the device, or read back for the numpy definition
    report = []
    for n in (4096, 16326):
        p, t = table(n, n + 1)
        on_device = lambda: rel.reliability_metrics(p, t, M)
        on_host = lambda: rel.reliability_host(p.cpu().numpy(), t.cpu().numpy(), M)
        forms = {"device": on_device, "readback_numpy": on_host}
        got = on_device().cpu().figures.numpy()
        want, _ = on_host()
        if not (np.array_equal(got[:, :6], want[:, :6], equal_nan=True) and np.allclose(got, want, rtol=1e-12, equal_nan=True)):
            raise SystemExit(f"the two reports of {n} rows disagree")
        ms = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, fn in forms.items():
                ms[k].append(timed_host(fn)[0])
        report.append({"rows": n, "ms": {k: _range(v) for k, v in ms.items()}, "pooled_ece": float(got[C + 1, 4])})
    # ---- the fit
    import torch.nn.functional as F

    def lbfgs(z, y, how, per_class):
        """the usual recipe on the device table: parameters (C,) or (1,), the sum over the groups of their mean NLL"""
        k = C if per_class else 1
        a = torch.ones(k, dtype=torch.float64, device=dev, requires_grad=True)
        b = torch.zeros(k, dtype=torch.float64, device=dev, requires_grad=how == "platt")
        params = [a, b] if how == "platt" else [a]
        opt = torch.optim.LBFGS(params, lr=1.0, max_iter=50, tolerance_grad=1e-12, tolerance_change=1e-15, line_search_fn="strong_wolfe")

        def closure():
            opt.zero_grad()
            loss = F.binary_cross_entropy_with_logits(a * z + b, y, reduction="none").mean(0).sum() if per_class else \
                F.binary_cross_entropy_with_logits(a * z + b, y)
            loss.backward()
            return loss
        opt.step(closure)
        n_iter = opt.state[opt._params[0]]["n_iter"]
        return a.detach().cpu().numpy(), b.detach().cpu().numpy(), int(n_iter)      # the read-back ends the recipe

    fits = []
    for n in (1871, 16326):
        s, y = table(n, n + 2)
        z = torch.from_numpy(rel.logit_host(s.cpu().numpy())).to(dev)
        y64 = y.double()
        for how in ("temperature", "platt"):
            for per_class in (False, True):
                forms = {"device": lambda: fit_scaling(s, y, how=how, per_class=per_class, max_iter=64),
                         "lbfgs": lambda: lbfgs(z, y64, how, per_class)}
                for fn in forms.values():
                    fn()                                             # warm-up
                ms, last = {k: [] for k in forms}, {}
                for _ in range(args.rounds):
                    for k, fn in forms.items():
                        took, last[k] = timed_host(fn)
                        ms[k].append(took)
                sc = last["device"].cpu()
                la, lb, n_iter = last["lbfgs"]
                diff = max(float(np.abs(sc.a.numpy() - la).max()), float(np.abs(sc.b.numpy() - lb).max()))
                fits.append({"rows": n, "how": how, "per_class": per_class, "ms": {k: _range(v) for k, v in ms.items()},
                             "device_iterations": int(sc.iterations.max()), "device_status": sc.status.tolist(),
                             "device_launches": 2 + 64, "lbfgs_iterations": n_iter, "max_parameter_difference": diff,
                             "a": sc.a.tolist(), "b": sc.b.tolist()})
    line = json.dumps({"bench": "reliability", "classes": C, "bins": M, "rounds": args.rounds, "collector_launches_per_round": args.reps,
                       "collector": collector, "report": report, "fit": fits})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
