"""What the whole-model GPU tests share when they hold mmda_amd.MISA against the live CPU oracle (oracle/misa_oracle.py): the
reference's statement order for the losses, and the comparison of one step's outputs, losses and gradients."""
import torch


def rel(got, ref):
    got = torch.as_tensor(got).detach().float().cpu(); ref = torch.as_tensor(ref).detach().float().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-6))


def statement_order_losses(solver, cfg, scores, emo):
    """The reference's statement order behind model(...): the getters on the side-channel attributes, then the weighted total
    (solver.py:165-181).  Returns ({name: loss tensor}, total); total.backward() is the caller's."""
    L = dict(cls=solver.get_cls_loss(scores, emo), diff=solver.get_diff_loss(), recon=solver.get_recon_loss(),
             conf=solver.get_conf_loss(scores, emo))
    L["sim"] = solver.get_cmd_loss() if cfg.use_cmd_sim else solver.get_domain_loss()
    total = L["cls"] + cfg.diff_weight * L["diff"] + cfg.sim_weight * L["sim"] + cfg.recon_weight * L["recon"]
    if cfg.use_confidNet:
        total = total + cfg.conf_weight * L["conf"]
    return L, total


def assert_outputs_and_losses_match_oracle(scores, tcp, losses, o, L, tol):
    """scores / tcp against the oracle's forward `o`, the six losses ({name: float}) against its `L`, both to `tol`."""
    assert rel(scores, o.scores.detach()) < tol and rel(tcp, o.tcp.detach()) < tol
    for k in ("cls", "diff", "sim", "recon", "conf", "total"):
        ref = float(getattr(L, k).detach())
        assert abs(losses[k] - ref) <= tol * abs(ref) + 1e-6, (k, losses[k], ref)


def assert_grads_match_oracle(model, G, bound):
    """Relative L2 error of every parameter gradient against the oracle's G within `bound`.  Left out: gradients the oracle leaves None
    and in_proj_bias, whose key part is identically zero in exact arithmetic (softmax shift invariance: DESIGN section 2)."""
    for k, p in model.named_parameters():
        if G[k] is None or k.endswith("self_attn.in_proj_bias"):
            continue
        g = p.grad.cpu().double(); ref = G[k].double()
        if float(ref.norm()) < 1e-12:
            assert float(g.norm()) < 1e-6, k
            continue
        l2 = float((g - ref).norm() / ref.norm())
        assert l2 <= bound, f"{k}: relative L2 error {l2:.3e}"
