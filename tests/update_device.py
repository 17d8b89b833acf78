"""Device side of test_hip_update.py and of its child process update_route_child.py (not a test module): one update of the device
from the state of a case of update_cases.py, results as NumPy arrays."""
import update_cases as cases


def run_round(ctx, case, rnd, reference=False, h_neg=None, g_neg=None):
    """One update of the device from the state of round ``rnd`` -> dict of NumPy arrays: success, means, chols, last_eta, l2,
    num_updates and, for the KL update, kls, probes, packed (the kernel's parameter blocks; not with ``reference``) and
    packed_ref (gmmvi_pack_components of the device's own result)."""
    from gmmvi_amd import hip_ops
    r = case["rounds"][rnd]
    means, chols = ctx.asarray(r["means"]), ctx.asarray(r["chols"])
    h = ctx.asarray(case["H_neg"] if h_neg is None else h_neg)
    g = ctx.asarray(case["g_neg"] if g_neg is None else g_neg)
    steps, l2, nupd = ctx.asarray(case["stepsizes"]), ctx.asarray(r["l2"]), ctx.asarray(r["num_updates"])
    out = {}
    if case["mode"] == "kl":
        last_eta = ctx.asarray(r["last_eta"])
        res = hip_ops.update_components_kl(ctx, means, chols, h, g, steps, case["temperature"], cases.L2_INIT, last_eta, l2, nupd,
                                           want_info=True, reference=reference, want_packed=not reference)
        out.update(success=res[0].numpy().astype(bool), kls=res[1].numpy(), probes=res[2].numpy(), last_eta=last_eta.numpy())
        if not reference:
            out.update(packed=res[3].numpy(), packed_ref=hip_ops.pack_components(ctx, means, chols)[0].numpy())
    else:
        succ = hip_ops.update_components_plain(ctx, case["mode"], means, chols, h, g, steps, cases.L2_INIT, l2, nupd)
        out.update(success=succ.numpy().astype(bool))
    out.update(means=means.numpy(), chols=chols.numpy(), l2=l2.numpy(), num_updates=nupd.numpy())
    return out


def run_slab(ctx, case):
    """gmmvi_stein_update_kl on a case of update_cases.make_slab_case -> dict(success, means, chols, last_eta, l2, num_updates,
    packed, packed_ref, h_scratch, g_scratch, R)."""
    from gmmvi_amd import hip_ops
    sc, r = case["stein"], case["rounds"][0]
    means, chols = ctx.asarray(r["means"]), ctx.asarray(r["chols"])
    packed_old, _ = hip_ops.pack_components(ctx, means, chols)
    last_eta, l2, nupd = ctx.asarray(r["last_eta"]), ctx.asarray(r["l2"]), ctx.asarray(r["num_updates"])
    succ, packed, h, g, parts = hip_ops.stein_update_kl(
        ctx, packed_old, ctx.asarray(sc["x"]), ctx.asarray(sc["ld"]), ctx.asarray(sc["qgrad"]), ctx.asarray(sc["bg"]),
        ctx.asarray(sc["tgrad"]), means, chols, ctx.asarray(case["stepsizes"]), case["temperature"], cases.L2_INIT, last_eta, l2,
        nupd, self_normalized=case["snis"])
    return dict(success=succ.numpy().astype(bool), means=means.numpy(), chols=chols.numpy(), last_eta=last_eta.numpy(),
                l2=l2.numpy(), num_updates=nupd.numpy(), packed=packed.numpy(),
                packed_ref=hip_ops.pack_components(ctx, means, chols)[0].numpy(), h_scratch=h.numpy(), g_scratch=g.numpy(), R=parts)
