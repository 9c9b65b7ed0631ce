"""CPU checks of the float64 layer reference (oracle/layer_ref.py) that tests/test_gpu_layer_parity.py holds every stored activation of the
inference engines to: composed layer by layer it IS the oracle network, the float64 BN fold is eval BN, and its gate resolves a single
wrong element (one element off by 2 bf16 ulps at a border pixel, two channels of one pixel swapped) while it passes an honest f32
evaluation of the same layer."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import layer_ref as lr
from oracle import resnet18 as o18
from oracle import resnet50 as o50


def _r50(seed):
    m = o50.seeded_model(seed, 5, perturb_bn=True)
    with torch.no_grad():
        for name, mod in m.named_modules():
            if name.endswith("bn3"):
                mod.weight.mul_(0.2)
    return m.eval()


@pytest.mark.parametrize("arch,P", [("r18", 224), ("r18", 96), ("r50", 224), ("r50", 96)])
def test_composed_layers_reproduce_the_oracle_in_float64(arch, P):
    m = o18.seeded_model(321, 5, perturb_bn=True).eval() if arch == "r18" else _r50(5)
    x = torch.rand(2, 3, P, P, generator=torch.Generator().manual_seed(P), dtype=torch.float64)
    acts, logits = lr.compose(m, x.numpy())
    md = m.double()
    with torch.no_grad():
        want = md(x).numpy()
        stem = F.max_pool2d(F.relu(md.bn1(md.conv1(x))), 3, 2, 1).numpy()
        l1 = md.layer1(torch.from_numpy(stem)).numpy()
    assert np.abs(logits - want).max() <= 1e-9 * (1 + np.abs(want).max())
    assert np.abs(acts["maxpool"] - stem).max() <= 1e-12 * np.abs(stem).max()
    last1 = [L["name"] for L in lr.topology(m) if L["name"].startswith("layer1.")][-1]
    assert np.abs(acts[last1] - l1).max() <= 1e-11 * np.abs(l1).max()
    names = [L["name"] for L in lr.topology(m)]
    assert len(names) == (20 if arch == "r18" else 53) and len(set(names)) == len(names)


def test_float64_fold_equals_conv_then_eval_bn():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 64, 9, 9, generator=g, dtype=torch.float64)
    bn = torch.nn.BatchNorm2d(128).double().eval()
    with torch.no_grad():
        bn.weight.copy_(0.5 + torch.rand(128, generator=g))
        bn.bias.copy_(0.1 * torch.randn(128, generator=g))
        bn.running_mean.copy_(0.1 * torch.randn(128, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(128, generator=g))
    w = torch.randn(128, 64, 3, 3, generator=g, dtype=torch.float64) * 0.06
    with torch.no_grad():
        want = bn(F.conv2d(x, w, None, 2, 1)).numpy()
    p = [t.detach().numpy() for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var)]
    wf, b = lr.fold_bn(w.numpy(), *p)
    got, _ = lr.conv_epilogue(x.numpy(), wf, np.ones(128), b, 2, relu=False, exact=True)
    assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()


def test_round_to_is_one_round_to_nearest_even():
    v = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -40, -(1 + 2.0 ** -8), 3.0 * 2.0 ** -130, 0.0])
    assert list(lr.round_to(v, "bf16")) == [1.0, 1 + 2 * 2.0 ** -7, 1 + 2.0 ** -7, -1.0, 3.0 * 2.0 ** -130, 0.0]
    # f64 -> f32 -> bf16 (torch's cast) rounds twice: 1 + 2^-8 + 2^-30 becomes the tie 1 + 2^-8 in f32, then 1.0; once it is 1 + 2^-7
    assert lr.round_to(np.array([1 + 2.0 ** -8 + 2.0 ** -30]), "bf16")[0] == 1 + 2.0 ** -7
    r = np.random.default_rng(0).standard_normal(10000)
    assert np.array_equal(lr.round_to(r, "f32"), r.astype(np.float32).astype(np.float64))


def _layer(seed=7, cin=64, cout=64, hw=14):
    """A bf16 layer with residual: operands bf16-exact, an honest f32 evaluation of it (torch CPU float32 conv, f32 epilogue, one
    rounding to bf16), and the reference's (want, A)."""
    g = torch.Generator().manual_seed(seed)
    bf = lambda t: t.bfloat16().double()  # noqa: E731
    x = bf(F.relu(torch.randn(3, cin, hw, hw, generator=g)))
    w = bf(torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5)
    sc = (0.5 + torch.rand(cout, generator=g)).double()
    sh = (0.1 * torch.randn(cout, generator=g)).double()
    res = bf(torch.randn(3, cout, hw, hw, generator=g))
    want, A = lr.conv_epilogue(x, w, sc, sh, 1, res)
    y = F.conv2d(x.float(), w.float(), None, 1, 1) * sc.float()[None, :, None, None] + sh.float()[None, :, None, None] + res.float()
    got = F.relu(y).bfloat16().double().numpy()
    return got, want, A, lr.rounding_count(cin, 3, "bf16", True)


def test_gate_passes_an_f32_evaluation_and_resolves_one_element():
    got, want, A, K = _layer()
    assert lr.gate_mask(got, want, A, K, "bf16").all()
    assert (got == want).mean() > 0.95
    # one element, 2 bf16 ulps off, on the border (last row) of image 2
    c, px = np.unravel_index(np.argmax(np.abs(want[2, :, -1, :])), want[2, :, -1, :].shape)
    bad = got.copy()
    bad[2, c, -1, px] += 2 * lr.quantum(want[2, c, -1, px], "bf16")
    m = lr.gate_mask(bad, want, A, K, "bf16")
    assert (~m).sum() == 1 and not m[2, c, -1, px]
    # two channels of one pixel (the top-left corner of image 1) swapped
    v = want[1, :, 0, 0]
    c1, c2 = int(np.argmax(v)), int(np.argmin(v))
    bad = got.copy()
    bad[1, [c1, c2], 0, 0] = bad[1, [c2, c1], 0, 0]
    m = lr.gate_mask(bad, want, A, K, "bf16")
    assert (~m).sum() == 2 and not m[1, c1, 0, 0] and not m[1, c2, 0, 0]


def test_gate_of_pooled_stem_and_f32_storage():
    g = torch.Generator().manual_seed(11)
    x = torch.rand(2, 3, 32, 32, generator=g).double()
    w = torch.randn(64, 3, 7, 7, generator=g).double() * 0.1
    sc, sh = torch.ones(64, dtype=torch.float64), 0.1 * torch.randn(64, generator=g).double()
    want, A = lr.conv_epilogue(x, w, sc, sh, 2, pool=True, fmt="f32")
    y = F.relu(F.conv2d(x.float(), w.float(), None, 2, 3) + sh.float()[None, :, None, None])
    got = F.max_pool2d(y, 3, 2, 1).double().numpy()
    K = lr.rounding_count(3, 7, "f32", False)
    assert want.shape == (2, 64, 8, 8) and lr.gate_mask(got, want, A, K, "f32").all()
    bad = got.copy()
    bad[0, 5, 7, 7] += 4 * lr.quantum(want[0, 5, 7, 7], "f32") + 2 * lr.gamma(K) * A[0, 5, 7, 7]
    assert (~lr.gate_mask(bad, want, A, K, "f32")).sum() == 1
