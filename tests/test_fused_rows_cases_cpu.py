"""No GPU: what tests/test_gpu_fused_rows.py relies on (tests/fused_rows_cases.py).

  * the ctypes mirrors have the sizes the library's structs have;
  * the float64 restatements, chained, ARE the fusion block: forward against oracle/misa_oracle.py, backward against torch autograd of
    that oracle, 1e-10 relative, dropout off and on;
  * the case inputs keep class scores off the threshold and feed-forward pre-activations off the kink;
  * the recorded float32-against-float64 distances (REC) are current;
  * the comparison has power: every planted mistake moves some compared tensor at least ten bounds away, at every case it applies to;
  * the launchers refuse what their kernels cannot serve, before any launch."""
import ctypes as C

import pytest
import torch

import fused_rows_cases as fc
from mmda_amd import _lib
from oracle import dropout_rng as drng
from oracle import misa_oracle as orc

EINVAL = -1
LAUNCHES = tuple(fc.CASES)


@pytest.fixture(scope="module")
def entries():
    return fc.debug_entries(_lib.load())


def test_mirrors_have_the_library_struct_sizes(entries):
    for which, st in enumerate(fc.MIRRORS):
        assert C.sizeof(st) == entries["sizeof"](which), st.__name__
    assert entries["sizeof"](len(fc.MIRRORS)) == -1


# ------------------------------------------------------------------------------------------------ the restatement is the fusion block
TE = "transformer_encoder.layers.0."
PRIV = ("private_t.private_t_1", "private_v.private_v_1", "private_a.private_a_3")


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("p_tf,p_cls", [(0.0, 0.0), (0.25, 0.5)], ids=["dropout-off", "dropout-on"])
def test_chained_restatements_equal_the_oracle_and_its_autograd(p_tf, p_cls):
    B, seed = 5, 0x1D0A5EF0
    cfg = orc.default_config(vocab_size=80, dropout=p_cls)
    P = {k: v.double().requires_grad_(True) for k, v in orc.synth_params(cfg, 31).items()}
    g = torch.Generator().manual_seed(7)
    dims = {"t": cfg.embedding_size, "v": cfg.visual_size, "a": cfg.acoustic_size}
    utt = {m: torch.randn(B, 4 * d, generator=g, dtype=torch.float64).requires_grad_(True) for m, d in dims.items()}
    emo = (torch.rand(B, 6, generator=g) < 0.4).double()
    Gt, G6 = torch.randn(B, 6, generator=g, dtype=torch.float64), torch.randn(6, B, 128, generator=g, dtype=torch.float64)
    masks = drng.site_masks(cfg, B, seed, p_tf, p_cls) if p_tf > 0 else None
    o = orc.fusion_from_utterances(P, cfg, utt, masks=masks)
    x6 = torch.stack([getattr(o, f"utt_private_{m}") for m in "tva"] + [getattr(o, f"utt_shared_{m}") for m in "tva"])
    orig = torch.stack([getattr(o, f"utt_{m}_orig") for m in "tva"])
    recon = torch.stack([getattr(o, f"utt_{m}_recon") for m in "tva"])
    loss = (o.tcp * Gt).sum() + orc.cls_loss(o.scores, emo) + fc.RECON_SCALE * fc.inv_n(B) * ((recon - orig) ** 2).sum() + (x6 * G6).sum()
    loss.backward()
    D = lambda t: t.detach()
    W = lambda k: D(P[k])
    c = dict(B=B, nb=1, seed=seed, p_tf=p_tf, p_cls=p_cls, seeds=True, cls=None, ncls=6, n_parts=64, rec_part=False, null=(),
             act=fc.ACT_LEAKY)
    cf = dict(M=6 * B, F=2048, p=p_tf, seed=seed, scaled=p_tf > 0)
    rec_w = torch.stack([W(f"recon_{m}.recon_{m}_1.weight") for m in "tva"])
    head_w = torch.cat((W("confidence.confidence_layer_1.weight"), W("classifier.classifier_layer.weight")))
    # ---- forward
    a, _ = fc.fwd_a(dict(x6=D(x6), rec_w=rec_w, rec_b=torch.stack([W(f"recon_{m}.recon_{m}_1.bias") for m in "tva"]),
                         in_w=W(TE + "self_attn.in_proj_weight"), in_b=W(TE + "self_attn.in_proj_bias"),
                         out_w=W(TE + "self_attn.out_proj.weight"), out_b=W(TE + "self_attn.out_proj.bias"),
                         ln1_g=W(TE + "norm1.weight"), ln1_b=W(TE + "norm1.bias"), orig=D(orig)), c)
    f, _ = fc.ffn_fwd(dict(x1=a["x1"].reshape(6 * B, 128), w1=W(TE + "linear1.weight"), b1=W(TE + "linear1.bias"),
                           w2=W(TE + "linear2.weight")), cf)
    h, _ = fc.fwd_c(dict(parts=f["parts"].reshape(64, 6, B, 128), b2=W(TE + "linear2.bias"), x1=a["x1"], ln2_g=W(TE + "norm2.weight"),
                         ln2_b=W(TE + "norm2.bias"), head_w=head_w,
                         head_b=torch.cat((W("confidence.confidence_layer_1.bias"), W("classifier.classifier_layer.bias"))), emo=emo), c)
    for name, got, want in (("recon", a["recon"], recon), ("hfused", h["hfused"], o.h), ("tcp", h["tcp"], o.tcp),
                            ("scores", h["scores"], o.scores)):
        assert _rel(got, D(want)) <= 1e-10, name
    assert torch.equal(h["labels"], D(o.labels))
    # ---- backward
    bc, _ = fc.bwd_c(dict(tcp=h["tcp"], scores=h["scores"], d_tcp=Gt, d_scores=h["d_scores"], head_w=head_w, x1=a["x1"], f2=h["f2"],
                          ln2_g=W(TE + "norm2.weight"), ln2_mean=h["ln2_mean"], ln2_rstd=h["ln2_rstd"], d_recon=a["d_recon"],
                          rec_wT=rec_w.transpose(1, 2)), c)
    fb, _ = fc.ffn_bwd(dict(d_f2=bc["d_f2"].reshape(6 * B, 128), f1=f["f1"], l2_wT=W(TE + "linear2.weight").t(),
                            l1_wT=W(TE + "linear1.weight").t()), cf)
    z = torch.stack([D(utt[m]) @ W(f"project_{m}.project_{m}.weight").t() + W(f"project_{m}.project_{m}.bias") for m in "tva"])
    az = fc._act(fc.ACT_LEAKY, z)
    _, pmean, prstd = fc._ln_fwd(az, 1.0, 0.0)
    ba, _ = fc.bwd_a(dict(pre_d_x1=bc["d_x1"], parts=fb["parts"].reshape(64, 6, B, 128), x6=D(x6), attn_out=a["attn_out"],
                          ln1_g=W(TE + "norm1.weight"), ln1_mean=a["ln1_mean"], ln1_rstd=a["ln1_rstd"], pre_d_x6=G6,
                          out_wT=W(TE + "self_attn.out_proj.weight").t(), qkv=a["qkv"], probs=a["probs"],
                          in_wT=W(TE + "self_attn.in_proj_weight").t(), d_recon=a["d_recon"], rec_wT=rec_w.transpose(1, 2),
                          rec_part=torch.zeros(3, B, 128, dtype=torch.float64), priv_wT=torch.stack([W(n + ".weight").t() for n in PRIV]),
                          sh_wT=W("shared.shared_1.weight").t(), pre_d_orig=a["d_orig"], z=z,
                          lnp_g=torch.stack([W(f"project_{m}.project_{m}_layer_norm.weight") for m in "tva"]), lnp_mean=pmean,
                          lnp_rstd=prstd), c)
    pg = torch.stack((bc["pg0"], ba["pg1"], ba["pg2"], ba["pg3"], ba["pg4"]), 1)                  # (B, 5, 2, 128)
    zero = torch.zeros(5, 128, dtype=torch.float64)
    fin, _ = fc.pg_finish(dict(pg=pg, pre_dgamma=zero, pre_dbeta=zero), dict(B=B))
    flat = lambda t: t.reshape(-1, t.shape[-1])
    ln_names = [TE + "norm2", TE + "norm1"] + [f"project_{m}.project_{m}_layer_norm" for m in "tva"]
    checks = [(f"d_utt_{m}", ba["d_z"][i] @ W(f"project_{m}.project_{m}.weight"), utt[m].grad) for i, m in enumerate("tva")]
    checks += [("in_proj_weight", flat(ba["d_qkv"]).t() @ flat(D(x6)), P[TE + "self_attn.in_proj_weight"].grad),
               ("in_proj_bias", flat(ba["d_qkv"]).sum(0), P[TE + "self_attn.in_proj_bias"].grad),
               ("out_proj.weight", flat(ba["d_attn_out"]).t() @ flat(a["ctx"]), P[TE + "self_attn.out_proj.weight"].grad),
               ("linear1.weight", fb["d_f1"].t() @ flat(a["x1"]), P[TE + "linear1.weight"].grad),
               ("linear2.weight", flat(bc["d_f2"]).t() @ f["f1"], P[TE + "linear2.weight"].grad),
               ("linear2.bias", flat(bc["d_f2"]).sum(0), P[TE + "linear2.bias"].grad),
               ("head_w", bc["d_logits"].t() @ h["hfused"],
                torch.cat((P["confidence.confidence_layer_1.weight"].grad, P["classifier.classifier_layer.weight"].grad))),
               ("d_hfused -> head_b", bc["d_logits"].sum(0),
                torch.cat((P["confidence.confidence_layer_1.bias"].grad, P["classifier.classifier_layer.bias"].grad))),
               ("shared.weight", sum(ba["d_x6"][3 + i].t() @ D(orig)[i] for i in range(3)), P["shared.shared_1.weight"].grad)]
    for i, m in enumerate("tva"):
        checks.append((f"recon_{m}.weight", a["d_recon"][i].t() @ D(x6[i] + x6[3 + i]), P[f"recon_{m}.recon_{m}_1.weight"].grad))
        checks.append((PRIV[i], ba["d_x6"][i].t() @ D(orig)[i], P[PRIV[i] + ".weight"].grad))
    for k, n in enumerate(ln_names):
        checks.append((n + ".weight", fin["dgamma"][k], P[n + ".weight"].grad))
        checks.append((n + ".bias", fin["dbeta"][k], P[n + ".bias"].grad))
    for name, got, want in checks:
        assert _rel(got, want) <= 1e-10, (name, _rel(got, want))


# ------------------------------------------------------------------------------------------------ inputs, recorded distances
def test_input_conditions_hold_at_every_case():
    for launch in ("fwd_c", "ffn_fwd"):
        for c in fc.CASES[launch]:
            for cond, d in fc.input_conditions(launch, c).items():
                assert d > fc.CONDITION_FLOOR[cond], (launch, c["name"], cond, d)


@pytest.mark.parametrize("launch", sorted(fc.REC))
def test_recorded_distances_are_current(launch):
    """a bound is 4 REC: what is measured now stays under 1.5 REC, and every tensor without a closed-form bound has an entry"""
    now = fc.measure_rec(launch)
    print(launch, {k: f"{v:.3g} (recorded {fc.REC[launch].get(k)})" for k, v in now.items()})
    assert set(now) == set(fc.REC[launch])
    for name, v in now.items():
        assert v <= 1.5 * fc.REC[launch][name], (launch, name, v)


# ------------------------------------------------------------------------------------------------ power
FACTORS = {}


@pytest.mark.parametrize("launch", LAUNCHES)
def test_every_planted_mistake_is_seen_at_ten_bounds(launch):
    tried = set()
    for c in fc.CASES[launch]:
        I = fc.inputs(launch, c)
        ref, ap = fc.written(launch, c, I)
        assert max(fc.excess(launch, ref, ref, ap).values()) == 0.0
        for mut in fc.MISTAKES:
            if not fc.applies(launch, c, mut):
                continue
            got, _ = fc.written(launch, c, I, mut=mut)
            worst = max(fc.excess(launch, got, ref, ap).values())
            FACTORS[(launch, c["name"], mut)] = worst
            tried.add(mut)
            assert worst >= 10.0, (launch, c["name"], mut, worst)
    low = min((v, k) for k, v in FACTORS.items() if k[0] == launch)
    print(f"{launch}: mistakes tried {sorted(tried)}; smallest factor {low[0]:.3g} at {low[1][1]} / {low[1][2]}")
    assert tried


def test_every_mistake_and_option_is_exercised():
    """each mistake applies somewhere, and each option of the A / C table appears at an nb = 2, odd-B shape"""
    for mut in fc.MISTAKES:
        assert any(fc.applies(launch, c, mut) for launch in LAUNCHES for c in fc.CASES[launch]), mut
    odd = [c for c in fc.AC_CASES if c["nb"] == 2 and c["B"] % 2 == 1]
    assert {c["B"] for c in odd} == {1, 5, 129}
    has = lambda f: any(f(c) for c in odd)
    assert {c["ncls"] for c in odd} == {1, 3, 6, 16} and {c["n_parts"] for c in odd} == {0, 1, 3, 33, 64}
    for f in (lambda c: c["p_tf"] == 0, lambda c: c["p_tf"] > 0, lambda c: c["p_cls"] == 0, lambda c: c["p_cls"] > 0, lambda c: c["seeds"],
              lambda c: not c["seeds"], lambda c: c["cls"] is None and c["seeds"], lambda c: c["cls"] is not None and c["seeds"],
              lambda c: c["rec_part"], lambda c: not c["rec_part"], lambda c: "d_tcp" in c["null"], lambda c: "d_scores" in c["null"],
              lambda c: "pg_parts" in c["null"], lambda c: c["act"] == fc.ACT_LEAKY, lambda c: c["act"] != fc.ACT_LEAKY,
              lambda c: c["flag"], lambda c: not c["flag"]):
        assert has(f)
    assert {(c["B"], c["nb"]) for c in fc.AC_CASES} == {(1, 1), (1, 2), (5, 1), (5, 2), (64, 1), (65, 1), (128, 2), (129, 2)}


# ------------------------------------------------------------------------------------------------ refusals
X = 0x1000            # a non-NULL address that is never read: every call below is refused before any launch


def _ln(st, n=128):
    a = st()
    a.rows, a.n = 6, n
    for name, t in st._fields_:
        if t is C.c_void_p and name not in ("res", "dgamma", "dbeta", "y_bf16"):
            setattr(a, name, X)
    return a


def _valid(launch):
    """arguments the launcher would accept (never passed as they are)"""
    st = {"fwd_a": fc.FusedFwdA, "fwd_c": fc.FusedFwdC, "bwd_c": fc.FusedBwdC, "bwd_a": fc.FusedBwdA, "ffn_fwd": fc.FusedFfnFwd,
          "ffn_bwd": fc.FusedFfnBwd}[launch]
    a = st()
    for name, t in st._fields_:
        if t is C.c_void_p and name not in ("dbg", "wait_flag", "wait_err"):
            setattr(a, name, X)
    if launch in ("ffn_fwd", "ffn_bwd"):
        a.M, a.hs, a.F, a.S = 6, 128, 64, 32
        return a
    a.B, a.hs, a.nb = 1, 128, 1
    if launch in ("fwd_a", "bwd_a"):
        a.nhead = 2
    else:
        a.ncls = 6
    if launch == "fwd_a":
        a.ln1 = _ln(_lib.LnArgs)
    if launch == "fwd_c":
        a.ln2 = _ln(_lib.LnArgs)
    if launch == "bwd_c":
        a.ln2 = _ln(_lib.LnBwdArgs)
    if launch == "bwd_a":
        a.ln1 = _ln(_lib.LnBwdArgs)
        for i in range(3):
            a.lnp[i] = _ln(_lib.LnBwdArgs)
    return a


def _set(a, path, value):
    *head, last = path.split(".")
    for h in head:
        a = a.lnp[int(h[3:])] if h.startswith("lnp") and h != "lnp" else getattr(a, h)
    setattr(a, last, value)


REFUSED = {
    "fwd_a": [("B", 0), ("nb", 0), ("nb", 3), ("hs", 64), ("nhead", 4), ("ln1.n", 64), ("orig", None), ("d_orig", None)],
    "fwd_c": [("B", 0), ("nb", 0), ("nb", 3), ("hs", 64), ("ln2.n", 64), ("emo", None)],
    "bwd_c": [("B", 0), ("nb", 0), ("nb", 3), ("hs", 64), ("ln2.n", 64), ("d_recon", None), ("rec_wT", None),
              ("ln2.dgamma+pg_parts", None), ("ln2.dbeta+pg_parts", None)],
    "bwd_a": [("B", 0), ("nb", 0), ("nb", 3), ("hs", 64), ("nhead", 1), ("ln1.n", 64), ("lnp1.n", 64), ("lnp2.n", 256),
              ("ln1.dgamma+pg_parts", None), ("lnp0.dbeta+pg_parts", None)],
    "ffn_fwd": [("M", 0), ("hs", 64), ("F", 0), ("F", 48), ("S", 16), ("S", 64)],
    "ffn_bwd": [("M", 0), ("hs", 64), ("F", 0), ("F", 48), ("S", 16), ("S", 64)],
}


@pytest.mark.parametrize("launch", sorted(REFUSED))
def test_launchers_refuse_before_any_launch(entries, launch):
    """MMDA_EINVAL for a NULL argument block and for each single change of REFUSED to arguments that would be accepted.  With every
    optional pointer given, the valid block of bwd_c carries rec_part, so its nb = 3 row is the refusal of three samples per workgroup
    beside rec_part; WITHOUT rec_part mmda_fused_bwd_c accepts any nb >= 1 (its kernel walks 6 nb rows and zeroes nb - 1 slots), which
    only a real launch can show: tests/test_gpu_fused_rows.py runs that launch at nb = 3 against the restatement."""
    fn = entries[launch]
    assert fn(None, None) == EINVAL
    for path, value in REFUSED[launch]:
        a = _valid(launch)
        if path.endswith("+pg_parts"):                        # a LayerNorm parameter gradient wanted, no partials to put it in
            _set(a, path[:-len("+pg_parts")], X)
            a.pg_parts = None
        else:
            _set(a, path, value)
        assert fn(C.byref(a), None) == EINVAL, (launch, path, value)


def test_pg_finish_refuses_before_any_launch(entries):
    fn = entries["pg_finish"]
    slots = (C.c_void_p * fc.PG_SLOTS)(*([X] * fc.PG_SLOTS))
    assert fn(None, 4, 128, slots, slots, None) == EINVAL
    assert fn(X, 0, 128, slots, slots, None) == EINVAL
    assert fn(X, 4, 64, slots, slots, None) == EINVAL
    assert fn(X, 4, 128, None, slots, None) == EINVAL
    assert fn(X, 4, 128, slots, None, None) == EINVAL
