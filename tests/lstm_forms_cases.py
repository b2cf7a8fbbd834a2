"""The launch forms of the resident-weights recurrences (mmda_amd/csrc/lstm_resident.hip and its three kernel files), defined once for the CPU test that proves
from the launch plan what each case reaches (test_lstm_plan_cpu.py) and the GPU test that checks its numbers
(test_gpu_lstm_forms.py).

A case is one set of descriptors (hidden sizes Hs, one cell, one gate layout) at one (B, T) under one switch set, run in up to five
PASSES -- `fwd` (stash) then `bwd` (fp32 dG, d_hseq given), `fwd_only` (forward_only = 1), `bwd16` (dg_bf16_only = 1, d_hseq given:
the model's layer 1) and `bwd16_nodh` (dg_bf16_only = 1, d_hseq NULL: its layer 2) -- as far as the form has instances for them.
`expect` holds what plan_resident() / pick_kernel() are meant to make of it: form, waves per block, launches, and per pass the
kernel instance and whether it is a PAIR = 1 instance.  Also here: the inputs of a case, its float64 and bf16-emulating references
(plain torch on the CPU), and the helper that builds the n descriptors inside guarded buffers and calls mmda_lstm_fwd / mmda_lstm_bwd.

Hidden sizes: P3 = the model's (19, 3 and 5 hidden tiles), Q4 adds 320 (20 tiles: the largest wave-form size, an even count, no ragged
k-step), BAR puts 300 beside a size (336) that sends the whole launch to the barrier form.  Workgroups per 32-sample batch group at
1 / 2 / 4 waves per block: P3 108 / 54 / 30, Q4 188 / 94 / 50; a launch holds 240.  Whether a gate-minor wave-sized plan takes the quad
form depends on a device occupancy query (at most min(512, 240 * blocks per CU) workgroups): every gate-minor case of the default
process has at most 240 one-wave workgroups (quad for any occupancy) or more than 512 (never quad)."""
import functools
import math
import zlib

import torch

P3, Q4, BAR = (300, 35, 74), (320, 300, 74, 35), (336, 300)
DEFAULT, NO_QUAD = "default", "no_quad"
ENV = {DEFAULT: {}, NO_QUAD: {"MMDA_LSTM_NO_QUAD": "1"}}
PASSES = ("fwd", "fwd_only", "bwd", "bwd16", "bwd16_nodh")
GROUP = 32

# (form, cell, gate_minor) -> instance per pass; {P} = ",1" at four waves per block (the pair pre-reduction), "" below
KERNELS = {
    ("wave", "lstm", False): dict(fwd="lstm_fwd_wave_kernel<10,false,LSTM,false>", fwd_only="lstm_fwd_wave_kernel<10,false,LSTM,false>",
                                  bwd="lstm_bwd_wave_kernel<20,false,LSTM,false>"),
    ("wave", "lstm", True): dict(fwd="lstm_fwd_wave_kernel<10,true,LSTM,false,0>", fwd_only="lstm_fwd_wave_kernel<10,true,LSTM,false,1>",
                                 bwd="lstm_bwd_wave_kernel<20,true,LSTM,false>", bwd16="lstm_bwd_wave_kernel<20,true,LSTM,false,1,1{P}>",
                                 bwd16_nodh="lstm_bwd_wave_kernel<20,true,LSTM,false,0,1{P}>"),
    ("quad", "lstm", True): dict(fwd="lstm_fwd_quad_kernel<LSTM,0>", fwd_only="lstm_fwd_quad_kernel<LSTM,1>",
                                 bwd="lstm_bwd_quad_kernel<LSTM,2,2>", bwd16="lstm_bwd_quad_kernel<LSTM,1,1>",
                                 bwd16_nodh="lstm_bwd_quad_kernel<LSTM,0,1>"),
    ("barrier", "lstm", False): dict(fwd="lstm_fwd_cluster_kernel<10,false>", fwd_only="lstm_fwd_cluster_kernel<10,false>",
                                     bwd="lstm_bwd_cluster_kernel<false>"),
    ("barrier", "lstm", True): dict(fwd="lstm_fwd_cluster_kernel<10,true>", fwd_only="lstm_fwd_cluster_kernel<10,true>",
                                    bwd="lstm_bwd_cluster_kernel<true>"),
    ("wave", "gru", False): dict(fwd="lstm_fwd_wave_kernel<10,false,GRU,false>", fwd_only="lstm_fwd_wave_kernel<10,false,GRU,false>",
                                 bwd="lstm_bwd_wave_kernel<20,false,GRU,false>"),
    ("wave", "gru", True): dict(fwd="lstm_fwd_wave_kernel<10,true,GRU,false>", fwd_only="lstm_fwd_wave_kernel<10,true,GRU,false>",
                                bwd="lstm_bwd_wave_kernel<20,true,GRU,false>"),
    ("quad", "gru", True): dict(fwd="lstm_fwd_quad_kernel<GRU,0>", fwd_only="lstm_fwd_quad_kernel<GRU,1>",
                                bwd="lstm_bwd_quad_kernel<GRU,2,2>"),
}


def case(Hs, B, T, form, wpb, launches, gate_minor=False, cell="lstm", switches=DEFAULT):
    pair = form == "wave" and wpb == 4 and gate_minor and cell == "lstm"
    kernels = {p: k.replace("{P}", ",1" if pair else "") for p, k in KERNELS[(form, cell, gate_minor)].items()}
    tag = {P3: "P3", Q4: "Q4", BAR: "BAR"}.get(tuple(Hs), "H" + "_".join(map(str, Hs)))
    name = f"{tag}-B{B}-T{T}-{cell}-{'gm' if gate_minor else 'gmaj'}" + ("-noquad" if switches == NO_QUAD else "")
    return dict(name=name, Hs=tuple(Hs), B=B, T=T, cell=cell, gate_minor=gate_minor, switches=switches,
                expect=dict(form=form, wpb=wpb, launches=launches, kernels=kernels,
                            pair={p: pair and p in ("bwd16", "bwd16_nodh") for p in kernels}))


CASES = [
    # gate-major wave form at 1, 2 and 4 waves per block, then chunked 4 + 1 groups (last group 5 rows: its second m-tile is empty)
    case(Q4, 21, 4, "wave", 1, 1), case(Q4, 37, 4, "wave", 2, 1), case(Q4, 69, 4, "wave", 4, 1), case(Q4, 133, 2, "wave", 4, 2),
    # gate-minor quad: 188 blocks; 216 blocks with a last group of 5 rows
    case(Q4, 21, 4, "quad", 1, 1, gate_minor=True), case(P3, 37, 4, "quad", 1, 1, gate_minor=True),
    # gate-minor wave form of the default process (more than 512 one-wave workgroups: never quad), four waves per block: the pair
    # instances with dg_bf16_only; chunked 4 + 1; the model's B = 256 shape in small
    case(Q4, 69, 4, "wave", 4, 1, gate_minor=True), case(Q4, 133, 4, "wave", 4, 2, gate_minor=True),
    case(P3, 133, 4, "wave", 4, 1, gate_minor=True),
    # one text-sized descriptor, the smallest B at which it chunks: 13 groups at 12 per launch, the last of one row
    case((300,), 385, 3, "wave", 4, 2), case((300,), 385, 3, "wave", 4, 2, gate_minor=True),
    # barrier form with several descriptors (H = 300 then runs the barrier kernels too), one launch and chunked 5 + 1 groups
    case(BAR, 37, 4, "barrier", 4, 1), case(BAR, 37, 4, "barrier", 4, 1, gate_minor=True),
    case(BAR, 165, 4, "barrier", 4, 2), case(BAR, 165, 4, "barrier", 4, 2, gate_minor=True),
    # the GRU cell above one wave per block, chunked, and in the quad form with and without stash
    case(Q4, 37, 4, "wave", 2, 1, cell="gru"), case(Q4, 133, 4, "wave", 4, 2, cell="gru"),
    case(Q4, 21, 4, "quad", 1, 1, gate_minor=True, cell="gru"),
    # MMDA_LSTM_NO_QUAD=1: the gate-minor wave form below four waves per block (the dg_bf16_only instances without pairing)
    case(Q4, 21, 4, "wave", 1, 1, gate_minor=True, switches=NO_QUAD), case(Q4, 37, 4, "wave", 2, 1, gate_minor=True, switches=NO_QUAD),
    case(Q4, 37, 4, "wave", 2, 1, gate_minor=True, cell="gru", switches=NO_QUAD),
]
assert len({c["name"] for c in CASES}) == len(CASES)


def cases_of(switches):
    return [c for c in CASES if c["switches"] == switches]


def passes_of(c):
    return tuple(p for p in PASSES if p in c["expect"]["kernels"])


def emits_dg_bf16(c):
    """mmda_lstm_desc.dg_bf16 is written by the wave and quad forms with the gate-minor layout"""
    return c["gate_minor"] and c["expect"]["form"] != "barrier"


def plan_descs(c, p, Hs=None):
    """The descriptors of pass p by shape alone, as ops.lstm_plan takes them"""
    only = p in ("bwd16", "bwd16_nodh")
    return [dict(H=H, cell=c["cell"], gate_minor=c["gate_minor"], forward_only=p == "fwd_only", d_hseq=p in ("bwd", "bwd16"),
                 dg_bf16=p.startswith("bwd") and (only or emits_dg_bf16(c)), dg_bf16_only=only) for H in (Hs or c["Hs"])]


def plan_of(c, p, quad_cap, Hs=None):
    from mmda_amd import ops
    return ops.lstm_plan(plan_descs(c, p, Hs), c["B"], c["T"], backward=p.startswith("bwd"), no_quad=c["switches"] == NO_QUAD,
                         quad_cap=quad_cap)


def plan_mismatch(c, p, plan):
    """What of the case's `expect` a plan of pass p does not show ([] = lands where intended)"""
    e = c["expect"]
    got = dict(ok=plan["ok"], form=plan["form"], wpb=plan["wpb"], launches=plan["launches"], kernel=plan["kernel"], pair=plan["pair"])
    want = dict(ok=True, form=e["form"], wpb=e["wpb"], launches=e["launches"], kernel=e["kernels"][p], pair=e["pair"][p])
    return [f"{c['name']} {p}: {k} is {got[k]!r}, expected {want[k]!r}" for k in want if got[k] != want[k]]


# ------------------------------------------------------------------------------------------------ inputs and references (CPU)
def seed_of(c, i):
    return zlib.crc32(f"{c['name']}/{i}".encode()) & 0x7FFFFFFF


def lengths_of(c):
    """Ragged, unsorted, drawn per batch group: every group (the last included) holds a row of length T and, where it has two rows, a
    row of length 1 -- an error in the group offset or in the indexing of `lengths` then moves an output by O(1)"""
    g = torch.Generator().manual_seed(seed_of(c, "lengths"))
    B, T = c["B"], c["T"]
    lengths = torch.randint(1, T + 1, (B,), generator=g)
    for r0 in range(0, B, GROUP):
        rows = min(GROUP, B - r0)
        pos = torch.randperm(rows, generator=g)
        lengths[r0 + int(pos[0])] = T
        if rows >= 2:
            lengths[r0 + int(pos[1])] = 1
    return lengths


def in_width(H):
    return H if H < 100 else 40


@functools.lru_cache(maxsize=2)
def inputs_of(name):
    """Per descriptor: the torch module (weights uniform in +-2/sqrt(H), twice torch's default range), x, d_out, d_hn; one `lengths`"""
    c = {k["name"]: k for k in CASES}[name]
    out = []
    for i, H in enumerate(c["Hs"]):
        torch.manual_seed(seed_of(c, i))
        D = in_width(H)
        rnn = (torch.nn.GRU if c["cell"] == "gru" else torch.nn.LSTM)(D, H, bidirectional=True)
        with torch.no_grad():
            k = 2.0 / math.sqrt(H)
            for p in rnn.parameters():
                p.uniform_(-k, k)
        out.append(dict(H=H, D=D, rnn=rnn, x=torch.randn(c["T"], c["B"], D), d_out=torch.randn(c["T"], c["B"], 2 * H),
                        d_hn=torch.randn(2, c["B"], H)))
    return out, lengths_of(c)


GRAD_KEYS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0", "weight_ih_l0_reverse", "weight_hh_l0_reverse",
             "bias_ih_l0_reverse", "bias_hh_l0_reverse")


def exact_reference(c, inp, lengths):
    """torch.nn.LSTM / nn.GRU in float64 on the packed sequence.  Returns hseq, hn and the gradients {"dX", parameter names} of
    sum(hseq d_out) + sum(hn d_hn) ("dh") and of sum(hn d_hn) alone ("nodh": d_hseq = NULL)."""
    import copy
    rnn = copy.deepcopy(inp["rnn"]).double()
    x = inp["x"].double().requires_grad_(True)
    pk = torch.nn.utils.rnn.pack_padded_sequence(x, lengths, enforce_sorted=False)
    out, hn = rnn(pk)
    hn = hn if c["cell"] == "gru" else hn[0]
    pad, _ = torch.nn.utils.rnn.pad_packed_sequence(out, total_length=c["T"])
    leaves = [x] + [dict(rnn.named_parameters())[k] for k in GRAD_KEYS]
    tail = (hn * inp["d_hn"].double()).sum()
    grads = {}
    for key, loss in (("dh", (pad * inp["d_out"].double()).sum() + tail), ("nodh", tail)):
        grads[key] = dict(zip(("dX",) + GRAD_KEYS, torch.autograd.grad(loss, leaves, retain_graph=True)))
    return dict(hseq=pad.detach(), hn=hn.detach(), grads=grads)


def emul_reference(c, inp, lengths, tile_partials):
    """The same layer on oracle.bf16_emul.birnn (rounds to bf16 where the kernels do); tile_partials: True = one bf16 partial dh per
    16-unit tile, 32 = per tile pair (the PAIR = 1 instances).  Same return value as exact_reference, in fp32."""
    from oracle import bf16_emul as emu
    leaves = {"r." + k: p.detach().clone().requires_grad_(True) for k, p in inp["rnn"].named_parameters()}
    x = inp["x"].clone().requires_grad_(True)
    out, hn = emu.birnn(x, lengths, leaves, "r", c["cell"], True, tile_partials)
    wrt = [x] + [leaves["r." + k] for k in GRAD_KEYS]
    tail = (hn * inp["d_hn"]).sum()
    grads = {}
    for key, loss in (("dh", (out * inp["d_out"]).sum() + tail), ("nodh", tail)):
        grads[key] = dict(zip(("dX",) + GRAD_KEYS, torch.autograd.grad(loss, wrt, retain_graph=True)))
    return dict(hseq=out.detach(), hn=hn.detach(), grads=grads)


def _q(t):
    return t.detach().bfloat16().double()


def four_slot(c, inp):
    """The parameters as the kernels take them, (w_ih (8H, D), [w_hh per direction (4H, H)], bias (8H) = b_ih + b_hh), fp32: the LSTM's
    as they are, the GRU's three gate blocks padded into four slots (W_ih / b_ih rows [r; z; n; 0], W_hh / b_hh rows [r; z; 0; n])"""
    P, H = {k: v.detach() for k, v in inp["rnn"].named_parameters()}, inp["H"]
    w_ih, w_hh, bias = [], [], []
    for sfx in ("", "_reverse"):
        wi, wh, bi, bh = (P[k + sfx] for k in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"))
        if c["cell"] == "gru":
            wi = torch.cat((wi, torch.zeros(H, wi.shape[1])), 0)
            wh = torch.cat((wh[:2 * H], torch.zeros(H, H), wh[2 * H:]), 0)
            bi = torch.cat((bi, torch.zeros(H)), 0)
            bh = torch.cat((bh[:2 * H], torch.zeros(H), bh[2 * H:]), 0)
        w_ih.append(wi); w_hh.append(wh.contiguous()); bias.append(bi + bh)
    return torch.cat(w_ih, 0), w_hh, torch.cat(bias, 0)


def host_pre(c, inp):
    """(T, B, 2, 4H) fp32: x W_ih^T + b_ih + b_hh per direction as the bf16 input GEMM forms it (bf16 operands), by a float64 product"""
    w_ih, _, bias = four_slot(c, inp)
    T, B, D = inp["x"].shape
    return (_q(inp["x"]).reshape(T * B, D) @ _q(w_ih).t() + bias.double()).float().view(T, B, 2, 4 * inp["H"])


def host_gradients(c, inp, dG, hseq):
    """The layer's gradients from the kernel's own outputs -- dG (T, B, 2, 4H) in torch's gate order (four slots for the GRU: d[pre_r,
    pre_z, pre_n, q]) and hseq (T, B, 2H) -- by float64 products of the bf16 operands the GEMMs would read (dG itself included: the
    model's GEMMs read dg_bf16 = round(dG)): no GEMM kernel involved"""
    H, (T, B, D) = inp["H"], inp["x"].shape
    P = {k: v.detach() for k, v in inp["rnn"].named_parameters()}
    xq, hq, dG = _q(inp["x"]).reshape(T * B, D), _q(hseq), _q(dG)
    out = {"dX": torch.zeros(T * B, D, dtype=torch.float64)}
    for d, sfx in enumerate(("", "_reverse")):
        G = dG[:, :, d]
        if c["cell"] == "gru":
            g_ih, g_hh = G[..., :3 * H], torch.cat((G[..., :2 * H], G[..., 3 * H:]), -1)
        else:
            g_ih = g_hh = G
        shifted = torch.zeros(T, B, H, dtype=torch.float64)               # h of the step before, in processing order
        if d:
            shifted[:-1] = hq[1:, :, H:]
        else:
            shifted[1:] = hq[:-1, :, :H]
        out["dX"] += g_ih.reshape(T * B, -1) @ _q(P["weight_ih_l0" + sfx])
        out["weight_ih_l0" + sfx] = g_ih.reshape(T * B, -1).t() @ xq
        out["weight_hh_l0" + sfx] = g_hh.reshape(T * B, -1).t() @ shifted.reshape(T * B, H)
        out["bias_ih_l0" + sfx] = g_ih.reshape(T * B, -1).sum(0)
        out["bias_hh_l0" + sfx] = g_hh.reshape(T * B, -1).sum(0)
    out["dX"] = out["dX"].view(T, B, D)
    return out


# ------------------------------------------------------------------------------------------------ the launch helper (GPU)
GUARD = 256                                          # bytes either side of every window
SENTINEL = 0x5A
UTT_FILL = 7.25                                      # what the final-h slots of the other layer must still hold


class Window:
    """`numel` elements inside a larger allocation whose surroundings hold a sentinel byte pattern"""

    def __init__(self, numel, dtype, dev, fill=None, src=None):
        size = torch.empty((), dtype=dtype).element_size()
        self.whole = torch.full((2 * GUARD + numel * size,), SENTINEL, dtype=torch.uint8, device=dev)
        self.t = self.whole[GUARD:GUARD + numel * size].view(dtype)
        if src is not None:
            self.t.copy_(src.reshape(-1))
        else:
            self.t.fill_(fill)

    def intact(self):
        return bool((self.whole[:GUARD] == SENTINEL).all()) and bool((self.whole[self.whole.numel() - GUARD:] == SENTINEL).all())


def prepare(c, inputs, lengths, dev):
    """What every pass of a case shares, on the device: packed W_hh (three packings per direction), the input projection, lengths"""
    from mmda_amd import ops
    prep = []
    for inp in inputs:
        _, w_hh, _ = four_slot(c, inp)
        wd = [w.to(dev) for w in w_hh]
        packs = [ops.lstm_pack(w, "bf16") for w in wd]
        pre = host_pre(c, inp).to(dev)
        prep.append(dict(H=inp["H"], pre=ops._to_gate_minor(pre, inp["H"]) if c["gate_minor"] else pre,
                         fwd=[p[0] for p in packs], bwd=[p[1] for p in packs], clu=[ops.lstm_pack_cluster(w) for w in wd]))
    return prep, lengths.to(device=dev, dtype=torch.int32)


def run_pass(c, p, prep, len_dev, inputs, dev, only=None, no_quad=False):
    """One forward call and, for a backward pass p, one backward call behind it, on fresh guarded buffers; `only` = i runs descriptor i
    alone.  Returns the plans the device reports for the two calls and, per descriptor, the buffers as the calls left them (on the
    CPU, in torch's layouts), whether an exchange timed out and whether every sentinel is intact."""
    import ctypes as C
    from mmda_amd import _lib, ops
    lib = _lib.load()
    T, B, gm = c["T"], c["B"], c["gate_minor"]
    idx = list(range(len(prep))) if only is None else [only]
    n = len(idx)
    arr = (_lib.LstmDesc * n)()
    bufs = []
    for d, i in zip(arr, idx):
        H, q = prep[i]["H"], prep[i]
        w = dict(gates=Window(T * B * 8 * H, torch.float32, dev, src=q["pre"]),
                 cstash=Window(T * ((B + 3) // 4 * 4 if gm else B) * 2 * H, torch.float32, dev, fill=0.0),
                 hseq=Window(T * B * 2 * H, torch.float32, dev, fill=float("nan")),
                 utt=Window(B * 4 * H, torch.float32, dev, fill=UTT_FILL),
                 xchg=Window(lib.mmda_lstm_xchg_bytes(H, B), torch.uint8, dev, fill=0))
        d.H = H; d.gates = w["gates"].t.data_ptr(); d.cstash = w["cstash"].t.data_ptr(); d.hseq = w["hseq"].t.data_ptr()
        d.wpack[0], d.wpack[1] = q["fwd"][0].data_ptr(), q["fwd"][1].data_ptr()
        d.utt = w["utt"].t.data_ptr(); d.layer = i % 2; d.xchg = w["xchg"].t.data_ptr(); d.epoch_base = 0
        d.gate_minor = int(gm); d.cell = _lib.CELL[c["cell"]]; d.forward_only = int(p == "fwd_only")
        bufs.append(w)
    plans = dict(fwd=ops.lstm_plan(arr, B, T, backward=False, no_quad=no_quad))
    _lib.check(lib.mmda_lstm_fwd(_lib.BF16, n, arr, B, T, len_dev.data_ptr(), _lib.stream_ptr()), "mmda_lstm_fwd")
    torch.cuda.synchronize()
    aborted = lambda: any(int(w["xchg"].t[:4].view(torch.int32).item()) != 0 for w in bufs)
    res = dict(plans=plans, aborted_fwd=aborted(), descs=[])
    for w, i in zip(bufs, idx):
        H = prep[i]["H"]
        r = dict(hseq=w["hseq"].t.cpu().view(T, B, 2 * H), utt=w["utt"].t.cpu().view(B, 4, H), cstash=w["cstash"].t.cpu(),
                 stash=w["gates"].t.cpu())
        res["descs"].append(r)
    if p.startswith("bwd"):
        only16, dh = p in ("bwd16", "bwd16_nodh"), p in ("bwd", "bwd16")
        for d, w, i in zip(arr, bufs, idx):
            H, q, inp = prep[i]["H"], prep[i], inputs[i]
            d_utt = torch.zeros(B, 4, H)
            d_utt[:, i % 2], d_utt[:, 2 + i % 2] = inp["d_hn"][0], inp["d_hn"][1]
            w["d_utt"] = Window(B * 4 * H, torch.float32, dev, src=d_utt.to(dev))
            w["d_hseq"] = Window(T * B * 2 * H, torch.float32, dev, src=inp["d_out"].to(dev)) if dh else None
            d.wpack[0], d.wpack[1] = q["bwd"][0].data_ptr(), q["bwd"][1].data_ptr()
            d.wpack_c[0], d.wpack_c[1] = q["clu"][0].data_ptr(), q["clu"][1].data_ptr()
            d.utt = w["d_utt"].t.data_ptr(); d.d_hseq = w["d_hseq"].t.data_ptr() if dh else None; d.epoch_base = T + 2
        if only16 or lib.mmda_lstm_bwd_emits_dg_bf16(_lib.BF16, n, arr, B, T):
            for d, w, i in zip(arr, bufs, idx):
                w["dg16"] = Window(T * B * 8 * prep[i]["H"], torch.bfloat16, dev, fill=float("nan"))
                d.dg_bf16 = w["dg16"].t.data_ptr(); d.dg_bf16_only = int(only16)
        plans["bwd"] = ops.lstm_plan(arr, B, T, backward=True, no_quad=no_quad)
        _lib.check(lib.mmda_lstm_bwd(_lib.BF16, n, arr, B, T, len_dev.data_ptr(), _lib.stream_ptr()), "mmda_lstm_bwd")
        torch.cuda.synchronize()
        res["aborted_bwd"] = aborted()
        for r, w, i in zip(res["descs"], bufs, idx):
            H = prep[i]["H"]
            if "dg16" in w:
                r["dg16_bits"] = w["dg16"].t.view(torch.int16).cpu()
                g16 = w["dg16"].t.float().cpu().view(T, B, 2, 4 * H)                  # the column order of `gates`
                r["dg16"] = ops._from_gate_minor(g16, H) if gm else g16
            if not only16:
                r["dG_raw"] = w["gates"].t.cpu()
                g = r["dG_raw"].view(T, B, 2, 4 * H)
                r["dG"] = ops._from_gate_minor(g, H) if gm else g
    for r, w in zip(res["descs"], bufs):
        r["broken"] = [k for k, v in w.items() if v is not None and not v.intact()]
    return res
