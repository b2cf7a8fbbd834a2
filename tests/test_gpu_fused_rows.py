"""MI355X: the seven launches of mmda_amd/csrc/fused_rows.hip, each alone, against the float64 restatement of tests/fused_rows_cases.py
(cases, inputs, bounds: there; why they can be trusted: tests/test_fused_rows_cases_cpu.py).

Per case: every buffer sits between two 256-float guards; stored outputs start as NaN, accumulated ones from known random values.  One
launch on the current stream, then (1) every written tensor within its per-element bound of the restatement, (2) every guard and every
buffer the case leaves untouched bit-equal to its pre-fill, no NaN left where a store is promised, (3) each stage again, from the GPU's
own copy of the intermediates it stored, within the bound of that single stage -- a failure there names the stage -- and (4) a second
launch from the same pre-fill gives the same bits.  Every figure is printed before it is asserted.

First run (72 cases, 1.6 s): every launch within its bounds at one and at two samples per workgroup, the short last workgroup included;
the largest error was 0.43 of its bound (pg slot 4 of backward A at B = 128, nb = 2), the feed-forward pair stayed under 0.07."""
import ctypes as C

import pytest
import torch

import fused_rows_cases as fc
from mmda_amd import _lib
from oracle import dropout_rng as drng

pytestmark = pytest.mark.gpu
GUARD, SENTINEL = 256, -7.5
HS = fc.HS


def _ids(launch):
    return [c["name"] for c in fc.CASES[launch]]


@pytest.fixture(scope="module")
def entries():
    return fc.debug_entries(_lib.load())


class Arena:
    """named device buffers between guards, with the pre-fill of each kept on the host"""

    def __init__(self):
        self.full, self.pre = {}, {}

    def put(self, name, t):
        """a buffer holding the float32 tensor t (an input, or an output's pre-fill)"""
        t = t.to(torch.float32).contiguous()
        full = torch.full((t.numel() + 2 * GUARD,), SENTINEL, dtype=torch.float32)
        full[GUARD:GUARD + t.numel()] = t.flatten()
        self.full[name], self.pre[name] = full.cuda(), t.clone()
        return self.ptr(name)

    def nan(self, name, *shape):
        return self.put(name, torch.full(shape, float("nan")))

    def ptr(self, name, offset=0):
        return self.full[name].data_ptr() + 4 * (GUARD + offset)

    def get(self, name):
        return self.full[name][GUARD:-GUARD].cpu().reshape(self.pre[name].shape)

    def refill(self):
        for name, t in self.pre.items():
            self.full[name][GUARD:-GUARD].copy_(t.flatten())

    def guards_intact(self):
        return [n for n, f in self.full.items() if not (bool((f[:GUARD] == SENTINEL).all()) and bool((f[-GUARD:] == SENTINEL).all()))]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _ln_fwd_args(A, rows, x, res, gamma, beta, y, mean, rstd, c, site, permute=False):
    ln = _lib.LnArgs()
    ln.rows, ln.n, ln.x, ln.res, ln.gamma, ln.beta, ln.y, ln.mean, ln.rstd = rows, HS, A.ptr(x), A.ptr(res), A.ptr(gamma), A.ptr(beta), \
        A.ptr(y), A.ptr(mean), A.ptr(rstd)
    ln.drop_p, ln.drop_seed, ln.drop_site, ln.eps = c["p_tf"], c["seed"], site, 1e-5
    if permute:
        ln.permute_S, ln.permute_B = fc.S6, c["B"]
    return ln


def _ln_bwd_args(rows, dy, x, res, gamma, mean, rstd, d_x, d_res, acc=0, act=fc.ACT_NONE, p=0.0, seed=0, site=0, permute_B=0):
    l = _lib.LnBwdArgs()
    l.rows, l.n, l.dy, l.x, l.res, l.gamma, l.mean, l.rstd, l.d_x, l.accumulate_dx, l.d_res = rows, HS, dy, x, res, gamma, mean, rstd, d_x, \
        acc, d_res
    l.act, l.drop_p, l.drop_seed, l.drop_site = act, p, seed, site
    if permute_B:
        l.permute_S, l.permute_B = fc.S6, permute_B
    return l


# ------------------------------------------------------------------------------------------------ one set-up per launch
# each fills the arena and returns (the launch's argument block, {restatement name: how to read it} for outputs that are part of a buffer)
def _setup_fwd_a(A, c, I):
    B = c["B"]
    for k, v in I.items():
        A.put(k, v)
    for name, shape in (("recon", (3, B, HS)), ("qkv", (6, B, 3 * HS)), ("ctx", (6, B, HS)), ("probs", (B, 2, 6, 6)), ("attn_out", (6, B, HS)),
                        ("x1", (6, B, HS)), ("ln1_mean", (6, B)), ("ln1_rstd", (6, B)), ("d_recon", (3, B, HS)), ("d_orig", (3, B, HS))):
        A.nan(name, *shape)
    f = fc.FusedFwdA()
    f.B, f.hs, f.nhead, f.nb = B, HS, 2, c["nb"]
    for k in ("x6", "rec_w", "rec_b", "recon", "in_w", "in_b", "qkv", "ctx", "probs", "out_w", "out_b", "attn_out"):
        setattr(f, k, A.ptr(k))
    f.p_tf, f.seed, f.site_attn = c["p_tf"], c["seed"], drng.SITE_ATTN
    f.ln1 = _ln_fwd_args(A, 6 * B, "x6", "attn_out", "ln1_g", "ln1_b", "x1", "ln1_mean", "ln1_rstd", c, drng.SITE_DROP1)
    if c["seeds"]:
        f.orig, f.d_recon, f.d_orig, f.recon_inv_n, f.recon_scale = A.ptr("orig"), A.ptr("d_recon"), A.ptr("d_orig"), fc.inv_n(B), fc.RECON_SCALE
    return f, {}


def _setup_fwd_c(A, c, I):
    B, ncls = c["B"], c["ncls"]
    for k, v in I.items():
        A.put(k, v)
    if c["n_parts"]:
        A.nan("f2", 6, B, HS)
    for name, shape in (("hfused", (B, 6 * HS)), ("ln2_mean", (6, B)), ("ln2_rstd", (6, B)), ("logits", (B, 6 + ncls)), ("tcp", (B, 6)),
                        ("scores", (B, ncls)), ("labels", (B, ncls)), ("d_scores", (B, ncls))):
        A.nan(name, *shape)
    f = fc.FusedFwdC()
    f.B, f.hs, f.ncls, f.nb = B, HS, ncls, c["nb"]
    f.ln2 = _ln_fwd_args(A, 6 * B, "x1", "f2", "ln2_g", "ln2_b", "hfused", "ln2_mean", "ln2_rstd", c, drng.SITE_DROP2, permute=True)
    if c["n_parts"]:
        f.ffn_parts, f.n_parts, f.b2, f.f2 = A.ptr("parts"), c["n_parts"], A.ptr("b2"), A.ptr("f2")
    for k in ("hfused", "head_w", "head_b", "logits", "tcp", "scores", "labels"):
        setattr(f, k, A.ptr(k))
    f.threshold, f.p_cls, f.seed, f.site_cls = fc.THRESHOLD, c["p_cls"], c["seed"], drng.SITE_CLS
    if c["seeds"]:
        f.emo, f.d_scores = A.ptr("emo"), A.ptr("d_scores")
        if c["cls"]:
            f.cls.g, f.cls.nw = c["cls"]["g"], ncls
            for k in range(ncls):
                f.cls.w[k] = c["cls"]["w"][k]
    return f, {}


def _setup_bwd_c(A, c, I):
    B, ncls = c["B"], c["ncls"]
    for k, v in I.items():
        A.put(k, v)
    for name, shape in (("d_logits", (B, 6 + ncls)), ("d_hfused", (B, 6 * HS)), ("d_x1", (6, B, HS)), ("d_f2", (6, B, HS)),
                        ("pg", (B, fc.PG_SLOTS, 2, HS)), ("rec_part", (3, B, HS))):
        A.nan(name, *shape)
    f = fc.FusedBwdC()
    f.B, f.hs, f.ncls, f.nb = B, HS, ncls, c["nb"]
    f.tcp, f.scores, f.d_logits, f.head_w, f.d_hfused = A.ptr("tcp"), A.ptr("scores"), A.ptr("d_logits"), A.ptr("head_w"), A.ptr("d_hfused")
    f.d_tcp = None if "d_tcp" in c["null"] else A.ptr("d_tcp")
    f.d_scores = None if "d_scores" in c["null"] else A.ptr("d_scores")
    f.p_cls, f.seed, f.site_cls = c["p_cls"], c["seed"], drng.SITE_CLS
    f.ln2 = _ln_bwd_args(6 * B, A.ptr("d_hfused"), A.ptr("x1"), A.ptr("f2"), A.ptr("ln2_g"), A.ptr("ln2_mean"), A.ptr("ln2_rstd"),
                         A.ptr("d_x1"), A.ptr("d_f2"), p=c["p_tf"], seed=c["seed"], site=drng.SITE_DROP2, permute_B=B)
    f.pg_parts = None if "pg_parts" in c["null"] else A.ptr("pg")
    if c["rec_part"]:
        f.d_recon, f.rec_wT, f.rec_part = A.ptr("d_recon"), A.ptr("rec_wT"), A.ptr("rec_part")
    return f, {"pg0": lambda: A.get("pg")[:, 0]}


def _setup_bwd_a(A, c, I):
    B = c["B"]
    for k, v in I.items():
        A.put(k[4:] if k.startswith("pre_") else k, v)
    for name, shape in (("d_attn_out", (6, B, HS)), ("d_ctx", (6, B, HS)), ("d_qkv", (6, B, 3 * HS)), ("d_z", (3, B, HS)),
                        ("pg", (B, fc.PG_SLOTS, 2, HS))):
        A.nan(name, *shape)
    f = fc.FusedBwdA()
    f.B, f.hs, f.nhead, f.nb = B, HS, 2, c["nb"]
    f.ln1 = _ln_bwd_args(6 * B, A.ptr("d_x1"), A.ptr("x6"), A.ptr("attn_out"), A.ptr("ln1_g"), A.ptr("ln1_mean"), A.ptr("ln1_rstd"),
                         A.ptr("d_x6"), A.ptr("d_attn_out"), acc=1, p=c["p_tf"], seed=c["seed"], site=drng.SITE_DROP1)
    if c["n_parts"]:
        f.ffn_parts, f.n_parts, f.d_x1 = A.ptr("parts"), c["n_parts"], A.ptr("d_x1")
    for k in ("d_attn_out", "out_wT", "d_ctx", "qkv", "probs", "d_qkv", "in_wT", "d_recon", "rec_wT", "x6", "d_x6", "priv_wT", "sh_wT", "d_orig"):
        setattr(f, k, A.ptr(k))
    f.p_tf, f.seed, f.site_attn = c["p_tf"], c["seed"], drng.SITE_ATTN
    if c["rec_part"]:
        f.rec_part = A.ptr("rec_part")
    for i in range(3):
        f.lnp[i] = _ln_bwd_args(B, A.ptr("d_orig", i * B * HS), A.ptr("z", i * B * HS), None, A.ptr("lnp_g", i * HS), A.ptr("lnp_mean", i * B),
                                A.ptr("lnp_rstd", i * B), A.ptr("d_z", i * B * HS), None, act=c["act"])
    f.pg_parts = None if "pg_parts" in c["null"] else A.ptr("pg")
    if c["flag"]:                                         # a flag that already holds its value, and the word a timeout would set
        A.flags = torch.tensor([7, 0, 0, 0], dtype=torch.int32).cuda()
        f.wait_flag, f.wait_value, f.wait_err = A.flags.data_ptr(), 7, A.flags.data_ptr() + 8
    return f, {f"pg{k}": (lambda k=k: A.get("pg")[:, k]) for k in range(1, 5)}


def _setup_ffn_fwd(A, c, I):
    M, F = c["M"], c["F"]
    for k, v in I.items():
        A.put(k, v)
    A.nan("f1", M, F)
    A.nan("parts", F // fc.FFN_S, M, HS)
    f = fc.FusedFfnFwd()
    f.M, f.hs, f.F, f.S, f.p, f.seed, f.site = M, HS, F, fc.FFN_S, c["p"], c["seed"], drng.SITE_FFN
    for k in ("x1", "w1", "b1", "f1", "w2", "parts"):
        setattr(f, k, A.ptr(k))
    return f, {}


def _setup_ffn_bwd(A, c, I):
    M, F = c["M"], c["F"]
    for k, v in I.items():
        A.put(k, v)
    A.nan("d_f1", M, F)
    A.nan("parts", F // fc.FFN_S, M, HS)
    f = fc.FusedFfnBwd()
    f.M, f.hs, f.F, f.S = M, HS, F, fc.FFN_S
    f.gate_scale = fc.gate_scale(c)
    for k in ("d_f2", "f1", "l2_wT", "d_f1", "l1_wT", "parts"):
        setattr(f, k, A.ptr(k))
    return f, {}


SETUP = {"fwd_a": _setup_fwd_a, "fwd_c": _setup_fwd_c, "bwd_c": _setup_bwd_c, "bwd_a": _setup_bwd_a, "ffn_fwd": _setup_ffn_fwd,
         "ffn_bwd": _setup_ffn_bwd}


def _compare(tag, launch, got, ref, ap):
    ex = fc.excess(launch, got, ref, ap)
    print(f"{tag}: " + "  ".join(f"{k} {v:.3g}" for k, v in ex.items()))
    bad = {k: v for k, v in ex.items() if not v <= 1.0}
    assert not bad, (tag, bad)


def _check(launch, c, I, A, call, special):
    ref, ap = fc.written(launch, c, I)
    assert call() == 0
    torch.cuda.synchronize()
    assert A.guards_intact() == []
    if hasattr(A, "flags"):
        assert A.flags.cpu().tolist() == [7, 0, 0, 0]                               # no timeout reported, nothing else written
    got = {k: (special[k]() if k in special else A.get(k)).reshape(v.shape) for k, v in ref.items()}
    for k, v in got.items():
        assert not torch.isnan(v).any(), f"{k}: a NaN of the pre-fill is left where a store is promised (or the kernel made one)"
    first = {n: _bits(A.get(n)).clone() for n in A.full}
    _compare(f"{launch} {c['name']} whole launch", launch, got, ref, ap)
    # buffers (and pg slots) that the restatement does not return are not touched
    for n in A.full:
        if n == "pg":
            for k in range(fc.PG_SLOTS):
                if f"pg{k}" not in ref:
                    assert torch.equal(_bits(A.get("pg")[:, k]), _bits(A.pre["pg"][:, k])), f"pg slot {k} touched"
        elif n not in ref:
            assert torch.equal(first[n], _bits(A.pre[n])), f"{n} touched"
    # each stage from the GPU's own copy of what the stage before it stored
    given = {k: got[k] for k in fc.INTERMEDIATES[launch] if k in got}
    if given:
        ref1, ap1 = fc.written(launch, c, I, given=given)
        _compare(f"{launch} {c['name']} stage by stage", launch, got, ref1, ap1)
    # the same bits from the same pre-fill
    A.refill()
    assert call() == 0
    torch.cuda.synchronize()
    for n in A.full:
        assert torch.equal(first[n], _bits(A.get(n))), f"{n}: the second launch gave other bits"
    assert A.guards_intact() == []


def _run(launch, c, entries):
    A, I = Arena(), fc.inputs(launch, c)
    f, special = SETUP[launch](A, c, I)
    _check(launch, c, I, A, lambda: entries[launch](C.byref(f), _lib.stream_ptr()), special)


@pytest.mark.parametrize("c", fc.CASES["fwd_a"], ids=_ids("fwd_a"))
def test_fwd_a(entries, c):
    _run("fwd_a", c, entries)


@pytest.mark.parametrize("c", fc.CASES["ffn_fwd"], ids=_ids("ffn_fwd"))
def test_ffn_fwd(entries, c):
    _run("ffn_fwd", c, entries)


@pytest.mark.parametrize("c", fc.CASES["fwd_c"], ids=_ids("fwd_c"))
def test_fwd_c(entries, c):
    _run("fwd_c", c, entries)


@pytest.mark.parametrize("c", fc.CASES["bwd_c"], ids=_ids("bwd_c"))
def test_bwd_c(entries, c):
    """the last case runs three samples per workgroup: mmda_fused_bwd_c accepts any nb >= 1 without rec_part, and serves it"""
    _run("bwd_c", c, entries)


@pytest.mark.parametrize("c", fc.CASES["ffn_bwd"], ids=_ids("ffn_bwd"))
def test_ffn_bwd(entries, c):
    _run("ffn_bwd", c, entries)


@pytest.mark.parametrize("c", fc.CASES["bwd_a"], ids=_ids("bwd_a"))
def test_bwd_a(entries, c):
    _run("bwd_a", c, entries)


@pytest.mark.parametrize("c", fc.CASES["pg_finish"], ids=_ids("pg_finish"))
def test_pg_finish(entries, c):
    A = Arena()
    I = fc.inputs("pg_finish", c)
    A.put("pg", I["pg"])
    A.put("dgamma", I["pre_dgamma"])
    A.put("dbeta", I["pre_dbeta"])
    ng, nbt = c["null"]
    dg = (C.c_void_p * fc.PG_SLOTS)(*[None if k == ng else A.ptr("dgamma", k * HS) for k in range(fc.PG_SLOTS)])
    db = (C.c_void_p * fc.PG_SLOTS)(*[None if k == nbt else A.ptr("dbeta", k * HS) for k in range(fc.PG_SLOTS)])
    keep_g, keep_b = [k for k in range(fc.PG_SLOTS) if k != ng], [k for k in range(fc.PG_SLOTS) if k != nbt]
    special = {"dgamma": lambda: A.get("dgamma")[keep_g], "dbeta": lambda: A.get("dbeta")[keep_b]}
    _check("pg_finish", c, I, A, lambda: entries["pg_finish"](A.ptr("pg"), c["B"], HS, dg, db, _lib.stream_ptr()), special)
    # the rows of the NULL slots keep their pre-fill
    assert torch.equal(_bits(A.get("dgamma")[ng]), _bits(A.pre["dgamma"][ng]))
    assert torch.equal(_bits(A.get("dbeta")[nbt]), _bits(A.pre["dbeta"][nbt]))
