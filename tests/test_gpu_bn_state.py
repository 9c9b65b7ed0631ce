"""BN state of the bf16 training engine against float64 on the engine's own stored tensors: the running statistics every training
forward writes (what eval() and every exported checkpoint use), and the eval-mode forward that consumes them.

ResNet-18 and ResNet-50 at P = 64 with B = 2 and B = 3: the layer-4 maps are 2 x 2, so n = 8 / 12 rows and the unbiased factor n / (n - 1)
is 14 % / 9 %; starting running statistics and gains are random (oracle seeded_model(perturb_bn=True), pushed with dh_train2_tensor
kind 2 / 0).  One case runs with DH_T2_FOLD=0, so both writers of the statistics are covered: bn_stat_finalize_onepass_kernel, and row
group 0 of bn2_fold_apply_kernel.

  running statistics   two consecutive training forwards on different batches.  After each, for EVERY BN (stem and downsample BNs
                       included) the engine's stored Z (dh_train2_debug_act, what = 0) gives the float64 mean and unbiased variance over
                       its B Ho Wo rows, and R' = 0.9 R + 0.1 stat is required per channel from the engine's previous R, with
                       num_batches_tracked counted.  Gates and the chain length K of each producing path: oracle/bn_state_ref.py.  All
                       paths sum the bf16-rounded stored values, none takes its sums from accumulators before the rounding.
  eval route           a forward with training = 0 on those statistics: for every non-downsample conv Y (what = 1) against
                       relu(z scale + shift [+ identity]) from the engine's Z and float64 coefficients gamma / sqrt(rv + eps),
                       beta - rm scale; at a downsample join the identity is the branch's BN of its own Z rounded to bf16.  The eval
                       forward leaves the running-statistics arena and the batch counters bit-identical.

Measured on an MI355X, worst |got - want| / gate (file: 5.2 s wall for the six cases): running_mean <= 0.19 (layer-4 maps, n = 8), running_var
<= 0.47; DH_T2_FOLD=0 gives the same figures as the folded writer (the two are bit-identical).  Eval Y: 1.000 in every case -- elements one bf16
unit from the float64 result where the float32 multiply-add landed on the other side of a rounding boundary, which the gate's bf16 unit admits.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import bn_state_ref as br
from oracle import resnet18 as o18
from oracle import resnet50 as o50
from oracle.layer_ref import topology

pytestmark = pytest.mark.gpu

P = 64


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _z(eng, name, what, shape, dev):
    """Stored tensor of conv `name` as float64 [B][H][W][C] (channels last, as the engine keeps it)."""
    from deephisto_amd._lib import check, lib
    b, c, h, w = shape
    buf = torch.empty(b * c * h * w, dtype=torch.float32, device=dev)
    check(lib().dh_train2_debug_act(eng.handle, name.encode(), what, buf.data_ptr(), buf.numel(), None), "dh_train2_debug_act")
    return buf.cpu().numpy().astype(np.float64).reshape(b, h, w, c)


@pytest.mark.parametrize("arch,B,fold", [("resnet18", 2, 1), ("resnet50", 2, 1), ("resnet18", 3, 1), ("resnet50", 3, 1), ("resnet18", 2, 0),
                                         ("resnet50", 2, 0)])
def test_running_statistics_and_eval_route(dev, arch, B, fold, monkeypatch):
    from deephisto_amd.models.patch_cls_simple.model import get_model
    monkeypatch.setenv("DH_T2_FOLD", str(fold))          # read when the engine's handle is created (the first forward)
    onet = o50 if arch == "resnet50" else o18
    ref = onet.seeded_model(7, 5, perturb_bn=True)
    topo = topology(ref)
    convs = {n: mod for n, mod in ref.named_modules() if isinstance(mod, torch.nn.Conv2d)}
    shapes = {}
    hooks = [mod.register_forward_hook(lambda _m, _i, out, n=n: shapes.__setitem__(n, tuple(out.shape))) for n, mod in convs.items()]
    with torch.no_grad():
        ref.eval()(torch.zeros(B, 3, P, P))
    for h in hooks:
        h.remove()
    assert shapes[topo[-1]["name"]][2:] == (2, 2)          # the layer-4 maps: n = 4 B rows
    m = get_model(5, "bf16", arch=arch)
    m.load_state_dict(ref.state_dict())
    m.to(dev).train()
    eng = m._engine
    g = torch.Generator().manual_seed(B)
    worst = {"mean": (0.0, ""), "var": (0.0, "")}
    for step in range(2):
        before = {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items() if "running" in k or "tracked" in k}
        x = torch.rand(B, 3, P, P, generator=g).to(dev)
        eng.forward(x, training=True)
        torch.cuda.synchronize()
        after = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
        for L in topo:
            name, bn = L["name"], L["bn"]
            b, c, h, w = shapes[name]
            z = _z(eng, name, 0, shapes[name], dev).reshape(-1, c)
            K = br.chain_length(br.path_of(name, convs[name].kernel_size[0]), z.shape[0], c)
            want_m, gate_m, want_v, gate_v = br.running_update_ref(z, before[bn + ".running_mean"], before[bn + ".running_var"], K)
            rm = np.abs(after[bn + ".running_mean"].astype(np.float64) - want_m) / gate_m
            rv = np.abs(after[bn + ".running_var"].astype(np.float64) - want_v) / gate_v
            for key, r in (("mean", rm), ("var", rv)):
                if float(r.max()) > worst[key][0]:
                    worst[key] = (float(r.max()), f"{name} (n = {z.shape[0]}, K = {K}, step {step})")
            assert float(rm.max()) <= 1.0, (name, step, "running_mean", float(rm.max()), int(rm.argmax()))
            assert float(rv.max()) <= 1.0, (name, step, "running_var", float(rv.max()), int(rv.argmax()))
            assert int(after[bn + ".num_batches_tracked"]) == int(before[bn + ".num_batches_tracked"]) + 1 == step + 1
    print(f"[bn state] {arch} B={B} fold={fold}: worst |got - want| / gate: running_mean {worst['mean'][0]:.3f} at {worst['mean'][1]}, "
          f"running_var {worst['var'][0]:.3f} at {worst['var'][1]}")

    # ---- eval route on those statistics ----------------------------------------------------------------------------------------------
    sd = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in m.state_dict().items()}
    arena = eng.flat(2, dev).clone()
    eng.forward(x, training=False)
    torch.cuda.synchronize()
    assert torch.equal(eng.flat(2, dev), arena)           # bit-identical running statistics
    for k, v in m.state_dict().items():
        if "tracked" in k:
            assert int(v) == 2, k
    coef = {L["name"]: br.eval_coefficients(sd[L["bn"] + ".weight"], sd[L["bn"] + ".bias"], sd[L["bn"] + ".running_mean"],
                                            sd[L["bn"] + ".running_var"]) for L in topo}
    Y = {}
    worst_y = (0.0, "")
    for L in topo:
        name = L["name"]
        if "downsample" in name:
            continue
        z = _z(eng, name, 0, shapes[name], dev)
        got = _z(eng, name, 1, shapes[name], dev)
        Y[name] = got
        if name == "conv1":      # the block input of layer 1: the engine's own max-pool of this map
            Y["maxpool"] = F.max_pool2d(torch.from_numpy(got).permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).numpy()
        idt, join = None, None
        if L["res"] is not None and "downsample" in L["res"]:
            join = (_z(eng, L["res"], 0, shapes[L["res"]], dev), *coef[L["res"]])
        elif L["res"] is not None:
            idt = Y[L["res"]]
        want, gate = br.eval_y_ref(z, *coef[name], idt, L["relu"], join)
        r = np.abs(got - want) / gate
        if float(r.max()) > worst_y[0]:
            worst_y = (float(r.max()), name)
        assert float(r.max()) <= 1.0, (name, float(r.max()), np.unravel_index(int(r.argmax()), r.shape))
    print(f"[bn state] {arch} B={B} fold={fold}: eval Y worst |got - want| / gate = {worst_y[0]:.3f} at {worst_y[1]}")
    m._release()
