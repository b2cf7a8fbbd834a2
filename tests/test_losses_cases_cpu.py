"""CPU: what the cases of tests/losses_cases.py reach, proven from the form query itself (ops.loss_forms -> mmda_loss_forms_describe:
host code, the decision the launchers read): every row lands on the form it names; together the rows reach every value the query can
return; every threshold has a row on either side; the generalised float64 reference equals the oracle's own functions on the
production pair lists; every row's inputs keep the reference well-posed; and the float32-against-float64 table a row's bound comes
from is computed (and printed) here as the GPU test computes it."""
from types import SimpleNamespace

import pytest
import torch

import losses_cases as lc
from mmda_amd import ops
from oracle import misa_oracle as orc


def test_every_row_lands_on_the_form_it_names():
    bad = []
    names = [c["name"] for c in lc.ALL_FORM_ROWS + lc.CLS_CASES + lc.CONF_CASES + lc.DOMAIN_CASES + lc.REPRO]
    assert len(names) == len(set(names)), sorted(n for n in names if names.count(n) > 1)
    for c in lc.ALL_FORM_ROWS:
        got = lc.forms_of(c)
        bad += [f"{c['name']}: {k} is {got[k]!r}, the row names {v!r}" for k, v in c["expect"].items() if got[k] != v]
        assert c["expect"] or c["kind"] in ("cls", "conf", "domain"), c["name"]         # (one form each: nothing to name)
    assert not bad, "\n".join(bad)
    for c in lc.MISC_CASES:
        assert c["grid"] == 1 + (c["ncls"] if c["with_conf"] else 0) + c["expect"]["misc_recon_blocks"]


def _reachable():
    """every value the query returns over B = 1 .. 300, D = 1 .. 520, loss / dx given or not, two or three CMD tensors"""
    seen = {k: set() for k in ("diff", "diff_products", "diff_loss_sum", "cmd", "stream_grid")}
    for B in list(range(1, 300)) + [1000]:
        for D in (1, 2, 3, 64, 127, 128, 129, 300, 512, 513, 520):
            for hl in (True, False):
                for hd in (True, False):
                    for nt in (2, 3):
                        f = ops.loss_forms(B, D, have_loss=hl, have_dx=hd, cmd_nt=nt)
                        for k in ("diff", "diff_products", "diff_loss_sum", "cmd"):
                            seen[k].add(f[k])
                        if f["cmd"] == "stream":
                            seen["stream_grid"].add("nt" if f["cmd_grid"] == nt and hd else f["cmd_grid"])
    return seen


def test_rows_reach_every_value_the_query_can_return():
    seen = _reachable()
    assert seen["diff"] == set(ops.LOSS_DIFF_FORMS) and seen["cmd"] == set(ops.LOSS_CMD_FORMS)
    assert seen["diff_products"] == set(ops.LOSS_DIFF_PRODUCTS) and seen["diff_loss_sum"] == set(ops.LOSS_DIFF_SUMS)
    assert seen["stream_grid"] == {"nt", 1}
    have = {k: set() for k in seen}
    for c in lc.ALL_FORM_ROWS:
        for k in ("diff", "diff_products", "diff_loss_sum", "cmd"):
            if k in c["expect"]:
                have[k].add(c["expect"][k])
        if c["expect"].get("cmd") == "stream":
            have["stream_grid"].add("nt" if c.get("have_dx", True) else c["expect"]["cmd_grid"])
    for k in seen:
        assert seen[k] - have[k] == set(), f"{k}: values the query returns and no row names: {sorted(map(str, seen[k] - have[k]))}"
    # the stream form with both tensor counts, so that grid = nt is told from grid = 3
    assert {c["expect"]["cmd_grid"] for c in lc.ALL_FORM_ROWS if c["expect"].get("cmd") == "stream"} == {1, 2, 3}
    # and the GPU test runs every list this proof is about
    assert {c["kind"] for c in lc.SIDE_CASES} == {"diff", "cmd"}


def _sides(kind, key, fixed, var, lo, hi):
    """the values of `key` that rows of `kind` name at var = lo and var = hi (the other dimension held at one value)"""
    out = []
    for v in (lo, hi):
        out.append({(c[fixed], c["expect"][key]) for c in lc.ALL_FORM_ROWS if c["kind"] == kind and c[var] == v and key in c["expect"]
                    and "variant" not in c})
    return out


@pytest.mark.parametrize("kind,key,var,lo,hi", [
    ("diff", "diff", "B", 32, 33), ("diff", "diff", "B", 64, 65), ("diff", "diff", "B", 128, 129), ("diff", "diff", "B", 256, 257),
    ("diff", "diff", "D", 128, 129), ("diff", "diff_products", "B", 256, 257), ("diff", "diff_loss_sum", "B", 256, 257),
    ("cmd", "cmd", "B", 32, 33), ("cmd", "cmd", "B", 64, 65), ("cmd", "cmd", "D", 128, 129), ("cmd", "cmd", "D", 512, 513)])
def test_each_threshold_has_a_row_on_either_side(kind, key, var, lo, hi):
    fixed = "D" if var == "B" else "B"
    below, above = _sides(kind, key, fixed, var, lo, hi)
    pairs = [(f, a, b) for f, a in below for g, b in above if f == g and a != b]
    assert pairs, f"no two rows of {kind} at {var} = {lo} and {hi} (same {fixed}) that name different values of {key}"


def test_recon_and_misc_block_counts_straddle_their_steps():
    assert [rb for _, rb in lc.MISC_RECON] == [1, 1, 1, 2, 17, 64]
    assert {c["expect"]["recon_blocks"] for c in lc.RECON_CASES} >= {1, 7, 64}
    assert ops.loss_forms(1, 1, n_recon=64 * 2048)["misc_recon_blocks"] == 64 and ops.loss_forms(1, 1, n_recon=10 ** 9)["misc_recon_blocks"] == 64
    assert ops.loss_forms(1, 1, n_recon=256)["recon_blocks"] == 1 and ops.loss_forms(1, 1, n_recon=257)["recon_blocks"] == 2


def test_generalised_reference_equals_the_oracle_on_the_production_lists():
    torch.manual_seed(3)
    ts = [torch.sigmoid(torch.randn(9, 65)).double() for _ in range(6)]
    o = SimpleNamespace(utt_private_t=ts[0], utt_private_v=ts[1], utt_private_a=ts[2], utt_shared_t=ts[3], utt_shared_v=ts[4],
                        utt_shared_a=ts[5], utt_t_recon=ts[0], utt_v_recon=ts[1], utt_a_recon=ts[2], utt_t_orig=ts[3], utt_v_orig=ts[4],
                        utt_a_orig=ts[5], domain_label_t=ts[0][:, :3], domain_label_v=ts[1][:, :3], domain_label_a=ts[2][:, :3])
    assert torch.equal(lc.diff_ref(ts, lc.PROD_DIFF), orc.diff_loss(o))
    assert torch.equal(lc.cmd_ref(ts[3:], lc.PROD_CMD, 5, 1.0) / 3.0, orc.cmd_loss(o))
    assert abs(float(lc.cmd_ref(ts[3:], lc.PROD_CMD, 5, 1.0 / 3.0) - orc.cmd_loss(o))) < 1e-15
    assert torch.equal(lc.recon_ref(ts[:3], ts[3:]), orc.recon_loss(o))
    assert torch.equal(lc.domain_ref([t[:, :3] for t in ts[:3]]), orc.domain_loss(o))
    # misc: its three losses are the oracle's, its recon term the mean over the flat buffer
    c = lc.MISC_CASES[7]
    inp = lc.misc_inputs(c)
    L, _ = lc.misc_reference(c, inp, torch.float64)
    s, t, y = (inp[k].double() for k in "sty")
    assert torch.equal(L["cls"], orc.cls_loss(s, y)) and torch.equal(L["conf"], orc.conf_loss(s, t, y))
    # fewer moments and a reversed pair: the value is symmetric, k moments are a prefix of k + 1
    a, b = ts[0], ts[1]
    assert torch.equal(lc.cmd_ref([a, b], [(0, 1)], 3), lc.cmd_ref([a, b], [(1, 0)], 3))
    assert float(lc.cmd_ref([a, b], [(0, 1)], 1)) == float(((a.mean(0) - b.mean(0)) ** 2).sum() ** 0.5)
    assert float(lc.cmd_ref([a, b], [(0, 1)], 4)) < float(lc.cmd_ref([a, b], [(0, 1)], 5))


def test_inputs_keep_the_reference_well_posed():
    for c in lc.SIDE_CASES + [c for c in lc.CONTRACT if c["kind"] == "cmd"]:
        if c["kind"] != "cmd":
            continue
        assert c["B"] >= 3, c["name"]
        ts = [t.double() for t in lc.side_inputs(c)]
        for i, j in c["pairs"]:
            assert i != j, c["name"]
            m = [[t.mean(0)] + [((t - t.mean(0)) ** k).mean(0) for k in range(2, c["n_moments"] + 1)] for t in (ts[i], ts[j])]
            norms = [float((p - q).norm()) for p, q in zip(*m)]
            assert min(norms) >= 1e-6, (c["name"], (i, j), norms)
    for c in lc.DIFF_SHAPES + lc.DIFF_LISTS + lc.DIFF_NAN:
        assert c["D"] >= 3 and c["B"] >= 2, c["name"]
        for t in lc.side_inputs(c):
            x = torch.nan_to_num(t.double())
            assert float((x - x.mean(0)).norm(dim=1).min()) > 1e-3, c["name"]       # the +1e-6 of the row norm stays negligible
    for c in lc.CONF_CASES + lc.MISC_CASES + lc.CLS_CASES:
        s, t, y = lc.head_inputs(c)
        assert bool((y.sum(0) > 0).all()), c["name"]
        assert float(s.min()) > 0 and float(s.max()) < 1
    for c in lc.DIFF_NAN:
        assert sum(int(torch.isnan(t).sum()) for t in lc.side_inputs(c)) == len(c["nan"])
        assert all(t < c["nt"] and r < c["B"] and col < c["D"] for t, r, col in c["nan"])
    unused = [c for c in lc.DIFF_LISTS if "unused" in c["name"]]
    assert len(unused) == 2 and all(2 not in {i for p in c["pairs"] for i in p} and c["nt"] == 4 for c in unused)


def test_inputs_are_reproducible():
    c = lc.DIFF_SHAPES[0]
    assert all(torch.equal(a, b) for a, b in zip(lc.side_inputs(c), lc.side_inputs(c)))
    assert not torch.equal(lc.side_inputs(lc.DIFF_SHAPES[0])[0], lc.side_inputs(lc.CMD_SHAPES[0])[0][:2])


def test_recorded_ratios_name_every_row_and_stay_under_the_factor():
    """tests/golden/losses_error_ratios.json is what one MI355X run of tests/test_gpu_losses.py measured (kernel error / e32 per row and
    metric): a record, kept in step with the table -- a row added without a new run shows up here."""
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "losses_error_ratios.json")
    rec = json.load(open(path))
    rows = lc.SIDE_CASES + lc.DIFF_NAN + lc.CONTRACT + lc.RECON_CASES + lc.MISC_CASES + lc.CLS_CASES + lc.CONF_CASES + lc.DOMAIN_CASES
    assert set(rec) == {c["name"] for c in rows}
    worst = max((v, n, k) for n, d in rec.items() for k, v in d.items())
    print(f"losses-ratio-worst {worst[1]} {worst[2]}: {worst[0]}")
    assert all(d for d in rec.values()) and worst[0] <= lc.FACTOR


def test_float32_against_float64_table():
    """e32 per row and metric: what 8 x of it is the bound.  Printed so that the bound of a row is visible without a GPU; asserted
    only to be a real figure, and the bound never above what the present tests allow."""
    worst = {}
    for c in lc.SIDE_CASES:
        _, _, e32 = lc.side_reference(c)
        for k, e in e32.items():
            assert e == e and e < float("inf"), (c["name"], k)
            b = lc.bound(c["kind"], k, e)
            assert 8 * lc.E32_FLOOR <= b <= lc.PRESENT[(c["kind"], k.split(".")[0])]
            worst[(c["kind"], k)] = max(worst.get((c["kind"], k), 0.0), e)
        print(f"losses-e32 {c['name']}: " + "  ".join(f"{k} {e:.2e}" for k, e in sorted(e32.items())))
    for (kind, k), e in sorted(worst.items()):
        print(f"losses-e32-worst {kind} {k}: {e:.2e}")
        assert e < 1e-4, (kind, k, e)          # float32 itself is a usable oracle at every shape of the table (D = 1 of DiffLoss is not: left out)
