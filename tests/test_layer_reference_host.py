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


# ---- data gradient (oracle/layer_ref.py: conv_dgrad) and the single-convolution cases of the bf16 training engine -----------------------
@pytest.mark.parametrize("ks", [1, 3])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("Hi", [4, 6, 14, 24])
def test_conv_dgrad_is_autograd_of_the_float64_conv(ks, stride, with_res, Hi):
    g = torch.Generator().manual_seed(ks * 100 + stride * 10 + Hi)
    cin, cout, B, Wi = 6, 10, 3, Hi + 2   # (unequal sides: a swapped output padding would show)
    x = torch.zeros(B, cin, Hi, Wi, dtype=torch.float64, requires_grad=True)
    w = torch.randn(cout, cin, ks, ks, generator=g, dtype=torch.float64)
    y = F.conv2d(x, w, None, stride, ks // 2)
    dz = torch.randn(y.shape, generator=g, dtype=torch.float64)
    (want,) = torch.autograd.grad(y, x, dz)
    res = torch.randn(x.shape, generator=g, dtype=torch.float64) if with_res else None
    if with_res:
        want = want + res
    got, A = lr.conv_dgrad(dz, w, stride, Hi, Wi, res, exact=True)
    assert got.shape == tuple(x.shape) and A.shape == got.shape
    assert np.abs(got - want.numpy()).max() <= 1e-12 * np.abs(want.numpy()).max()
    assert (A >= np.abs(got) * (1 - 1e-12)).all()
    rounded, _ = lr.conv_dgrad(dz, w, stride, Hi, Wi, res)
    assert np.array_equal(rounded, lr.round_to(got, "bf16"))


def _dgrad_layer(stride, B=3, c=64, Hi=12, seed=5):
    """A 3x3 data gradient with cin == cout on bf16-exact operands, with res: (dz, w, res, want, A, K)."""
    g = torch.Generator().manual_seed(seed)
    bf = lambda t: t.bfloat16().double()  # noqa: E731
    Ho = (Hi - 1) // stride + 1
    dz = bf(torch.randn(B, c, Ho, Ho, generator=g))
    w = bf(torch.randn(c, c, 3, 3, generator=g) * (2.0 / (9 * c)) ** 0.5)
    res = bf(torch.randn(B, c, Hi, Hi, generator=g))
    want, A = lr.conv_dgrad(dz, w, stride, Hi, Hi, res)
    return dz, w, res, want, A, lr.rounding_count(c, 3, "bf16", True)


def _failing(bad, want, A, K):
    return ~lr.gate_mask(bad, want, A, K, "bf16")


@pytest.mark.parametrize("stride", [1, 2])
def test_dgrad_gate_fails_every_planted_kernel_error(stride):
    """The errors a data-gradient kernel or its host tables would actually make, planted in a copy of `want`: each must fail the gate,
    and where the error is local the failures must sit where it was planted."""
    dz, w, res, want, A, K = _dgrad_layer(stride)
    B, c, Hi = want.shape[0], want.shape[1], want.shape[2]
    assert not _failing(want, want, A, K).any()
    # the operand transposed but not flipped / flipped but not transposed (cin == cout: both are valid operands of the same shape)
    for name, wrong in (("no flip", w.flip(2, 3)), ("no transpose", w.transpose(0, 1).contiguous())):
        bad, _ = lr.conv_dgrad(dz, wrong, stride, Hi, Hi, res)
        assert _failing(bad, want, A, K).mean() > 0.5, name
    # the last input row's contribution dropped: only the output rows it reaches may fail, and they must
    dz0 = dz.clone()
    dz0[:, :, -1, :] = 0
    bad, _ = lr.conv_dgrad(dz0, w, stride, Hi, Hi, res)
    f = _failing(bad, want, A, K)
    reach = stride * (dz.shape[2] - 1) - 1
    assert f.any() and not f[:, :, :reach].any() and f[:, :, reach:].any(axis=(1, 3)).all()
    # one parity class of the output shifted by one pixel
    bad = want.copy()
    bad[:, :, 1::2, 0::2] = np.roll(want[:, :, 1::2, 0::2], 1, axis=3)
    f = _failing(bad, want, A, K)
    assert f[:, :, 1::2, 0::2].mean() > 0.5 and not f[:, :, 0::2].any() and not f[:, :, :, 1::2].any()
    # the res of the last image of an odd batch omitted
    assert B % 2 == 1
    bad, _ = lr.conv_dgrad(dz, w, stride, Hi, Hi, torch.cat([res[:-1], torch.zeros_like(res[-1:])]))
    f = _failing(bad, want, A, K)
    assert f[-1].mean() > 0.5 and not f[:-1].any()
    # a single element moved by two bf16 ulps, in the last row of the last image
    ch, px = np.unravel_index(np.argmax(np.abs(want[-1, :, -1, :])), want[-1, :, -1, :].shape)
    bad = want.copy()
    bad[-1, ch, -1, px] += 2 * lr.quantum(want[-1, ch, -1, px], "bf16")
    f = _failing(bad, want, A, K)
    assert f.sum() == 1 and f[-1, ch, -1, px]


def test_stored_product_gate_holds_the_two_rounding_contract_and_resolves_two_ulps():
    """The strided 1x1 data gradient stores its product before adding it: the derived gate passes both the float64 value of that contract
    and its float32 evaluation, the plain gate does not pass the contract everywhere (which is why it has its own), and an element two
    bf16 ulps off, or the product scattered to the odd pixels, still fails."""
    from oracle import train_conv_cases as tc
    c = tc.BY_NAME["dgrad1_s2_accumulate"]
    ref = tc.reference(c.name)
    assert tc.gate(c, ref, ref.stored).all() and tc.gate(c, ref, tc.float32_evaluation(c.name)).all()
    assert not lr.gate_mask(ref.stored, ref.want, ref.A, ref.K, "bf16").all()
    i = np.unravel_index(np.argmax(np.abs(ref.want)), ref.want.shape)
    bad = ref.stored.copy()
    bad[i] = ref.want[i] + 2 * lr.quantum(ref.want[i], "bf16")
    assert (~tc.gate(c, ref, bad)).sum() == 1
    res = tc.operands(c.name).res.double().numpy()
    shifted = lr.stored_product_sum(np.roll(ref.prod, 1, axis=3), res)
    assert (~tc.gate(c, ref, shifted)).mean() > 0.4


def _case_names():
    from oracle import train_conv_cases as tc
    return [c.name for c in tc.CASES]


@pytest.mark.parametrize("name", _case_names())
def test_float32_evaluation_of_every_gpu_case_meets_the_identical_floor(name):
    """tests/test_gpu_conv_bf16_train.py demands that 0.999 of a kernel's elements equal the float64 value bit for bit (the project's
    IDENTICAL["bf16"]).  That floor is one an independent float32 evaluation of the same operands (torch's CPU convolution, one rounding
    to bf16) already meets on every case, and all of it lies inside the gate."""
    from oracle import train_conv_cases as tc
    c = tc.BY_NAME[name]
    ref = tc.reference(name)
    got = tc.float32_evaluation(name)
    assert got.shape == ref.want.shape == ref.A.shape
    assert tc.gate(c, ref, got).all()
    frac = float((got == ref.stored).mean())
    print(f"\n{name}: {len(ref.sel)} of {c.B} images, float32 evaluation identical fraction {frac:.5f}")
    assert frac >= 0.999, f"{name}: only {frac:.5f} of a float32 evaluation's elements identical"


def test_reference_images_of_a_large_batch_cover_the_group_boundaries():
    from oracle import train_conv_cases as tc
    c = tc.BY_NAME["dgrad3_s2_8x8x4_mt2"]
    sel = set(tc.select(c).tolist())
    assert set(range(8)) <= sel and {55, 56, 59, 60, 63, 64} <= sel and set(range(120, 125)) <= sel and len(sel) <= 24
    c = tc.BY_NAME["dgrad3_s1_64_persistent"]
    sel = set(tc.select(c).tolist())
    assert set(range(8)) <= sel and {15, 16} <= sel and {30, 31} <= sel and len(sel) <= 16
    assert all(len(tc.select(k)) == k.B for k in tc.CASES if k.B <= 16)


@pytest.mark.skipif(__import__("shutil").which("g++") is None, reason="g++ not available")
def test_stride1_cases_land_on_the_intended_tile_variant(tmp_path):
    """The stride-1 3x3 cases against `dh_conv3::pick_stride1` of the engine's own host header: the 32-image 64 x 64 case is the one that
    reaches the persistent 512-pixel variant (variant 0, 256 tiles = one per CU); the small ones the 256- and 128-pixel tiles."""
    import subprocess
    from pathlib import Path
    from oracle import train_conv_cases as tc
    repo = Path(__file__).resolve().parents[1]
    exe = tmp_path / "pick_stride1_probe"
    b = subprocess.run(["g++", "-std=c++17", "-O1", str(repo / "tests" / "host" / "pick_stride1_probe.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    want = {"dgrad3_s1_64": (2, 8), "dgrad3_s1_128": (1, 32), "dgrad3_s1_512_res": (2, 24), "dgrad3_s1_64_persistent": (0, 256),
            "fwd3_s1_64": (2, 8)}
    for name, (variant, tiles) in want.items():
        c = tc.BY_NAME[name]
        ch = c.cin if c.dgrad else c.cout   # the data gradient is a convolution from cout to cin channels over the same map
        r = subprocess.run([str(exe), str(c.B), str(c.H), str(c.H), str(ch), "256"], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        th, tw, imgs, v, n = map(int, r.stdout.split())
        assert (v, n) == (variant, tiles), (name, r.stdout)
        if c.B > 16:
            assert imgs == c.imgs, name


@pytest.mark.skipif(__import__("shutil").which("g++") is None, reason="g++ not available")
def test_range_cases_reach_the_launch_classes_their_table_claims(tmp_path):
    """The ResNet-18 cases of tests/test_gpu_layer_parity_range.py (tests/helpers/layer_parity.py, RANGE_CASES) through the engine's own launch
    plan (tests/host/conv3_plan_probe.cpp): their union reaches every class below, and each class is reached by the patch size the range
    file's table names for it.  The plan is the authority: the table follows it."""
    import subprocess
    import sys
    from pathlib import Path
    repo = Path(__file__).resolve().parents[1]
    sys.path.insert(0, str(repo / "tests" / "helpers"))
    import layer_parity as lp
    exe = tmp_path / "conv3_plan_probe"
    b = subprocess.run(["g++", "-std=c++17", "-O1", str(repo / "tests" / "host" / "conv3_plan_probe.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    reached, seen = {}, {}
    for arch, dtype, P, n in lp.RANGE_CASES:
        if arch != "r18":
            continue
        for args in lp.r18_conv3_launches(dtype, P, n):
            if args not in seen:
                r = subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
                assert r.returncode == 0 and "refused" not in r.stdout, (args, r.stdout, r.stderr)
                f = r.stdout.split()
                assert f[1] == "v" and f[11] == "tile", r.stdout
                seen[args] = ([int(t) for t in f[2:10]], [int(t) for t in f[12:23]])
            (stride, nt, mt, ds, wres, cls, half, m16), (TH, TW, IMGS, ty, tx, HR, HC, HP, HPH, WTAIL, FIT) = seen[args]
            esz, B, Hi, cin, cout, s, blocked, out16, wide, _ = args
            Ho = (Hi - 1) // s + 1
            assert stride == s and half == wide
            hit = []
            if s == 1:
                hit.append(f"stride-1 variant {0 if nt == 2 else 1 if mt == 2 else 2}")
                if (TH, TW, FIT) == (8, 64, 0) and Ho % 8 and Ho % 64:
                    hit.append("8x64 ragged")
                if (TH, TW, FIT) == (16, 32, 0) and Ho % 16 and Ho % 32:
                    hit.append("16x32 ragged")
                if (TH, TW, IMGS) == (16, 16, 2):
                    hit.append("16x16 two-image")
                if FIT and (TH, IMGS) == (7, 10):
                    hit.append(f"fit 7x7 x10 cout {cout}")
                if FIT and (TH, IMGS) == (8, 8):
                    hit.append(f"fit 8x8 x8 cout {cout}")
                if m16 and wres:
                    hit.append("m16 wres")
            elif half:
                if (TH, TW) == (16, 16):
                    hit.append("wide stride-2 16x16")
                if (TH, TW, IMGS) == (8, 8, 4) and Hi % 2:
                    hit.append("wide stride-2 8x8x4 odd input")
            else:
                hit.append(f"128-pixel stride-2 Wo {Ho}")
            for h in hit:
                reached.setdefault(h, set()).add((dtype, P, n))
        # the walk's last launch (layer4.1.conv2) runs the variant the GPU test requires of the engine's own report after the same forward
        assert (0 if nt == 2 else 1 if mt == 2 else 2) == lp.LAST_VARIANT[(dtype, P, n)], (dtype, P, n)
    # class -> a (dtype, P) of the table that must be among the cases reaching it
    want = {"stride-1 variant 0": ("bf16", 200), "stride-1 variant 1": ("bf16", 330), "stride-1 variant 2": ("f32", 32),
            "8x64 ragged": ("bf16", 200), "16x32 ragged": ("bf16", 97), "16x16 two-image": ("bf16", 97),
            "fit 7x7 x10 cout 256": ("bf16", 97), "fit 7x7 x10 cout 512": ("bf16", 200), "fit 8x8 x8 cout 64": ("bf16", 32),
            "m16 wres": ("bf16", 512), "wide stride-2 16x16": ("bf16", 512), "wide stride-2 8x8x4 odd input": ("bf16", 97),
            "128-pixel stride-2 Wo 4": ("bf16", 32), "128-pixel stride-2 Wo 2": ("bf16", 32), "128-pixel stride-2 Wo 1": ("bf16", 32)}
    for name in sorted(reached):
        print(f"{name}: {sorted(reached[name])}")
    for name, (dtype, P) in want.items():
        assert name in reached, f"no case reaches '{name}'"
        assert any((d, p) == (dtype, P) for d, p, _ in reached[name]), (name, sorted(reached[name]))
    # 16x32 ragged BOTH ways (25 and 21), the odd-input wide tiles of both odd chains, and the 128-pixel 7 -> 4 of P = 97 (layer 3 must not write 16-channel planes)
    assert {97, 330} <= {p for _, p, _ in reached["16x32 ragged"]} and {97, 330} <= {p for _, p, _ in reached["16x16 two-image"]}
    assert any(p == 97 for _, p, _ in reached["128-pixel stride-2 Wo 4"])
    # ten 7 x 7 images per tile at cout 512 take 256 tiles = 32 image groups x 8 cout blocks: n >= 311, not the table's first n = 300 (five per tile)
    assert ("bf16", 200, 311) in reached["fit 7x7 x10 cout 512"] and ("bf16", 200, 300) not in reached["fit 7x7 x10 cout 512"]
