"""What starting a training step behind the frozen encoders saves (the encoder cache).

    python tools/bench_encoded.py [--out profiles/encoded_step.json]

B = 32 and B = 256, T = 50, bf16, V = 20 000, dropout on, one model per batch size; a corpus of --batches * B seeded samples of length T
on the device.  Four forms take turns --rounds times in one process (drift of the machine lands on all of them alike):
    unfrozen       nothing frozen: the whole step
    cut            the encoder cut (six recurrent layers, three inter-layer LayerNorms, the table frozen): the encoders' forward, the
                   fusion block's forward and backward
    encoded        MISA.train_step_encoded over an EncoderCache of the corpus: one gather, then the projections onwards
    encoded_epoch  `encoded` plus the cache build (one evaluation pass over the corpus, timed in every turn) spread over --epochs
                   epochs of the corpus: ms per step of a run that builds the cache once and trains --epochs epochs from it
One device-event pair around --steps steps of a form (after --warmup untimed ones), the model's cluster check at the end of each turn.
Reports min - max per form and whether `encoded` beats `cut` by more than the round-to-round spread of either.
The gather launch alone: --gather-reps launches queued behind a blocking matrix product, one event pair around them (the method of
tools/bench_infer.py).

Needs the MI355X: there is no fall-back.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ENCODERS = ("trnn", "vrnn", "arnn", "tlayer_norm", "vlayer_norm", "alayer_norm", "embed")
DV, DA = 35, 74


def synth_samples(n, T, vocab, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        lab = rng.standard_normal((1, 7)).astype(np.float32)
        lab[0, 1 + i % 6] = 1.0                                       # every class occurs in any six consecutive samples
        out.append(((rng.integers(2, vocab, size=T), rng.standard_normal((T, DV), dtype=np.float32),
                     rng.standard_normal((T, DA), dtype=np.float32), None), lab, f"seg{i}"))
    return out


def _range(xs):
    s = sorted(xs)
    return {"min": s[0], "median": s[len(s) // 2], "max": s[-1], "rounds": list(xs)}


def measure(args, B):
    import torch
    from mmda_amd import DeviceDataset, DeviceLoader, EncodedLoader, EncoderCache, _lib, make_config
    from mmda_amd.solver import Solver
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    emb = torch.randn(args.vocab, 300, generator=torch.Generator().manual_seed(0))
    cfg = make_config(vocab_size=args.vocab, precision="bf16", device=str(dev), batch_size=B, seq_len=args.seq_len, pretrained_emb=emb.clone())
    m = Solver(cfg, cfg, cfg, None, None, None, is_train=True).build().model
    m.train()
    ds = DeviceDataset.from_samples(synth_samples(args.batches * B, args.seq_len, args.vocab, seed=B), dev)
    t, v, a, y, emo, lengths, *_ = next(iter(DeviceLoader(ds, B)))
    kw = dict(lr=cfg.learning_rate, clip=cfg.clip)
    everything = [n.split(".")[0] for n in m._names]
    state = {}
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def timed(fn, n=1):
        e0, e1 = ev(), ev()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    def enter(frozen):
        m.unfreeze(*everything)
        if frozen:
            m.freeze(*ENCODERS)

    def build():
        state["cache"] = EncoderCache.build(m, ds, B)
        state["eb"] = next(iter(EncodedLoader(state["cache"], B)))

    plain = lambda: m.train_step(t, v, a, lengths, emo, **kw)
    encoded = lambda: m.train_step_encoded(state["eb"], **kw)
    ms = {k: [] for k in ("unfrozen", "cut", "encoded", "build", "encoded_epoch")}
    for _ in range(args.rounds):
        for name, frozen, step in (("unfrozen", False, plain), ("cut", True, plain)):
            enter(frozen)
            timed(step, args.warmup)
            ms[name].append(timed(step, args.steps))
            m.check_cluster(f"bench_encoded {name}")
        enter(True)
        build()                                                       # (warm: workspace at the corpus's shapes)
        ms["build"].append(timed(build))
        timed(encoded, args.warmup)
        ms["encoded"].append(timed(encoded, args.steps))
        ms["encoded_epoch"].append(ms["encoded"][-1] + ms["build"][-1] / (args.epochs * args.batches))
        m.check_cluster("bench_encoded encoded")
    L = m.read_losses()
    if not all(x == x for x in L.values()):
        raise SystemExit(f"non-finite losses: {L}")
    out = {"batch": B, "corpus": args.batches * B, "forms_ms_per_step": {k: _range(v) for k, v in ms.items() if k != "build"},
           "cache_build_ms": _range(ms["build"]), "cache_bytes": int(state["cache"].flat.numel() * 4)}
    f = out["forms_ms_per_step"]
    out["encoded_over_cut"] = f["encoded"]["median"] / f["cut"]["median"]
    out["cut_over_unfrozen"] = f["cut"]["median"] / f["unfrozen"]["median"]
    out["encoded_beats_cut_beyond_spread"] = bool(f["encoded"]["max"] < f["cut"]["min"])
    out["cut_beats_unfrozen_beyond_spread"] = bool(f["cut"]["max"] < f["unfrozen"]["min"])
    print(f"B={B}: " + ", ".join(f"{k} {f[k]['min']:.3f}-{f[k]['max']:.3f}" for k in f) + " ms/step", file=sys.stderr, flush=True)

    # ---- the gather launch alone, queued behind a blocker
    c, eb = state["cache"], state["eb"]
    m._carve(B, 1, dev)
    nb = _lib.EncodedBatch(tab_t=c.utt_t.data_ptr(), tab_v=c.utt_v.data_ptr(), tab_a=c.utt_a.data_ptr(), tab_emo=c.emo.data_ptr(),
                           rows=eb.rows_ptr, B=B)
    outs = [m._ws_view(f"utt_{k}", (B, w)) for k, w in zip("tva", c.widths)]
    emo_out = torch.empty(B, 6, device=dev)
    lib, s = m._lib, _lib.stream_ptr()
    launch = lambda: lib.mmda_encoded_gather(nb.tab_t, nb.tab_v, nb.tab_a, *c.widths, nb.tab_emo, 6, nb.rows, B,
                                             *(o.data_ptr() for o in outs), emo_out.data_ptr(), s)
    big = torch.randn(8192, 8192, device=dev)
    sink = torch.empty_like(big)
    torch.mm(big, big, out=sink)
    for _ in range(20):
        _lib.check(launch(), "gather")
    us = []
    for r in range(args.gather_rounds):
        b0, e0, e1 = ev(), ev(), ev()
        torch.cuda.synchronize()
        b0.record()
        torch.mm(big, big, out=sink); torch.mm(big, big, out=sink)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(args.gather_reps):
            launch()
        e1.record()
        host_ms = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        if host_ms >= b0.elapsed_time(e0):
            raise SystemExit(f"gather: B={B} round {r}: queueing took the host {host_ms:.2f} ms, longer than the blocker: the launches were "
                             "not all waiting, nothing is reported")
        us.append(e0.elapsed_time(e1) * 1e3 / args.gather_reps)
    out["gather"] = {"bytes_moved": int(B * 4 * (sum(c.widths) + 6)), "launches_per_round": args.gather_reps, "us_per_launch": _range(us)}
    m.check_cluster("bench_encoded gather")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", type=int, default=8, help="batches per epoch of the corpus")
    ap.add_argument("--epochs", type=int, default=40, help="epochs the cache build is spread over")
    ap.add_argument("--seq-len", type=int, default=50)
    ap.add_argument("--vocab", type=int, default=20000)
    ap.add_argument("--gather-reps", type=int, default=200)
    ap.add_argument("--gather-rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encoded_step.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_encoded needs the MI355X (no CPU path)")
    torch.cuda.set_device(0)
    line = json.dumps({"bench": "encoded_step", "device": torch.cuda.get_device_name(0), "seq_len": args.seq_len, "precision": "bf16",
                       "vocab": args.vocab, "steps_per_round": args.steps, "rounds": args.rounds, "epochs": args.epochs,
                       "results": [measure(args, B) for B in (32, 256)]})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
