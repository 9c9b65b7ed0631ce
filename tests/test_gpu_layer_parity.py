"""GPU: every stored activation of the inference engines, element by element, against the float64 layer reference (oracle/layer_ref.py).

For each conv of the network (ResNet-18: the stem + 19 convs, downsamples included; ResNet-50: the stem + 52) the engine's own stored
input and residual are tapped (dh_debug_*_forward_tap: the launches of forward_tiles for all n tiles, one stored output copied out
right after the launch that writes it) and fed, with the conv's operands as the engine holds them (dh_debug_*_operands), to the float64
reference.  Every element of every selected image must satisfy

    |got - want| <= ulp(want) + gamma_K * A        (want: the exact value rounded once to bf16 / f32; A, K: oracle/layer_ref.py)

and a floor of the elements must be bit-identical to `want`.  The head: logits against float64 fc(avgpool(tapped last activation)).
The launch sizes reach every tile shape `pick_stride1` (conv3_tables_host.h) chooses for these maps:

    P = 224, n >= 300: fit tiles, 7 x 14 half-images (14 x 14) and whole 7 x 7 images (ten per tile at n >= 1021, five at n = 300);
                       8 x 64 (56 x 56) and 16 x 32 (28 x 28) power-of-two tiles; n = 5: 16 x 16 and 8 x 8 x 2 images
    P = 256, n >= 300: 16 x 32, 16 x 16 x 2 images and the 8 x 8 x 8-image fit tile (8 x 8); n = 5: 16 x 16, 8 x 8 x 2
    P = 96:            16 x 32 / 16 x 16 x 2 / 8 x 8 x 4 images; n = 5: 16 x 16, 8 x 8 x 2
n = 4096 is the timed launch, 4093 / 1021 leave a ragged last iteration of the persistent schedule, n = 300 is the launch of the
wide stride-2 aliasing bug (tests/test_gpu_resnet.py).  Selected images: 0..15, n/2-4 .. n/2+3, n-12 .. n-1 and 8 evenly spaced
(ResNet-50: 0..7, n/2-2 .. n/2+1, n-8 .. n-1, 4 spaced, to bound the float64 CPU cost); the first four tiles sit in the slide's corners.

Measured on one MI355X (every element of every case inside the gate; the file takes ~95 s): the lowest per-layer fraction of elements
bit-identical to `want` is 0.9997 for the bf16 engines (ResNet-18 and -50 alike; the rest differ by one bf16 unit where the f32 sum
straddles a rounding boundary) and 0.130 for the float32 engine (layer4.0.downsample.0; mean over its layers 0.458: a float32 result of
a 64..4608-term sum rarely equals the exactly rounded one, the gate's gamma_K * A term carries it).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import layer_ref as lr
from oracle import resnet18 as o18
from oracle import resnet50 as o50
from oracle import synth, tiling

pytestmark = pytest.mark.gpu

# floor of the fraction of elements bit-identical to `want`, per layer (measured minimum of any layer and case: 0.9997 / 0.1303)
IDENTICAL = {"bf16": 0.999, "f32": 0.12}

CASES = ([("r18", "bf16", P, n) for P in (224, 256, 96) for n in (4096, 4093, 300, 5)]
         + [("r18", "f32", P, n) for P in (224, 256) for n in (1024, 1021, 5)]
         + [("r50", "bf16", P, n) for P in (224, 256, 96) for n in (1024, 1021, 5)])


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _oracle(arch):
    if arch == "r18":
        return o18.seeded_model(321, 5, perturb_bn=True).eval()
    ref = o50.seeded_model(5, 5, perturb_bn=True)
    with torch.no_grad():
        for name, mod in ref.named_modules():
            if name.endswith("bn3"):
                mod.weight.mul_(0.2)
    return ref.eval()


def _model(ref, arch, dtype, dev):
    from deephisto_amd.models.patch_cls_simple.model import get_model
    m = get_model(5, compute_dtype=dtype) if arch == "r18" else get_model(5, arch="resnet50")
    m.load_state_dict(ref.state_dict())
    return m.to(dev).eval()


def _origins(h, w, P, n, seed):
    rng = np.random.default_rng(seed)
    o = [(0, 0), (0, w - P), (h - P, 0), (h - P, w - P)]
    o += [(int(rng.integers(0, h - P + 1)), int(rng.integers(0, w - P + 1))) for _ in range(n - 4)]
    return np.asarray(o[:n], np.int32)


def _select(n, arch):
    a, b, c, s = (16, 4, 12, 8) if arch == "r18" else (8, 2, 8, 4)
    idx = np.r_[0:a, n // 2 - b:n // 2 + b, n - c:n, np.linspace(0, n - 1, s).round().astype(int)]
    return np.unique(idx[(idx >= 0) & (idx < n)]).astype(np.int32)


def _operands(m, arch, L):
    from deephisto_amd._lib import check, lib
    cout, cin, ks = L["shape"]
    w = np.empty((cout, cin, ks, ks), np.float32)
    sc, sh = np.empty(cout, np.float32), np.empty(cout, np.float32)
    fn = lib().dh_debug_resnet18_operands if arch == "r18" else lib().dh_debug_resnet50_operands
    check(fn(m._handle, L["name"].encode(), w.ctypes.data, w.size, sc.ctypes.data, sh.ctypes.data, cout), "operands")
    return w, sc, sh


class _Taps:
    """Stored activations of one launch by name, fetched on first use (one tapped forward each) and dropped after their last use."""

    def __init__(self, m, arch, slide, o_dev, P, sel):
        self.m, self.arch, self.slide, self.o_dev, self.P = m, arch, slide, o_dev, P
        self.sel = torch.from_numpy(sel).to(slide.device)
        self.cache, self.logits = {}, []

    def get(self, name, shape):
        if name not in self.cache:
            from deephisto_amd._lib import check, lib
            out = torch.empty((len(self.sel),) + tuple(shape), dtype=torch.float32, device=self.slide.device)
            lg = torch.empty((len(self.o_dev), 5), dtype=torch.float32, device=self.slide.device)
            fn = lib().dh_debug_resnet18_forward_tap if self.arch == "r18" else lib().dh_debug_resnet50_forward_tap
            check(fn(self.m._handle, self.slide.data_ptr(), self.slide.shape[0], self.slide.shape[1], self.o_dev.data_ptr(),
                     len(self.o_dev), self.P, name.encode(), self.sel.data_ptr(), len(self.sel), out.data_ptr(), out.numel(),
                     lg.data_ptr(), None), f"forward tap {name}")
            self.cache[name] = out.cpu().numpy().astype(np.float64)
            self.logits.append(lg.cpu())
        return self.cache[name]


def _shapes(ref, P):
    """Output [C][H][W] of every stored activation of the topology, and each conv's [cout][cin][ks]."""
    shapes, H = {}, {"input": P}
    layers = lr.topology(ref)
    for L in layers:
        conv = ref.get_submodule(L["name"])
        h = (H[L["src"]] - 1) // L["stride"] + 1
        H[L["name"]] = h
        shapes[L["name"]] = (conv.out_channels, h, h)
        L["shape"] = (conv.out_channels, conv.in_channels, conv.kernel_size[0])
        if L["name"] == "conv1":
            H["maxpool"] = (h - 1) // 2 + 1
            shapes["maxpool"] = (64, H["maxpool"], H["maxpool"])
    return layers, shapes


def _fail_report(name, got, want, A, ok, sel):
    bad = np.argwhere(~ok)
    lines = [f"{name}: {len(bad)} of {ok.size} elements outside the gate; first (image, channel, y, x): got / want / A"]
    for i, c, y, x in bad[:8]:
        lines.append(f"  tile {int(sel[i])} c{c} ({y},{x}): {got[i, c, y, x]!r} / {want[i, c, y, x]!r} / {A[i, c, y, x]:.3g}")
    chans = np.unique(bad[:, 1])
    lines.append(f"  tiles {sorted(set(int(sel[i]) for i in bad[:, 0]))[:16]}, channels {chans[:16].tolist()} ({len(chans)}), "
                 f"rows {np.unique(bad[:, 2])[:16].tolist()}, cols {np.unique(bad[:, 3])[:16].tolist()}")
    return "\n".join(lines)


@pytest.mark.parametrize("arch,dtype,P,n", CASES)
def test_every_stored_activation_matches_float64_reference(dev, arch, dtype, P, n):
    ref = _oracle(arch)
    m = _model(ref, arch, dtype, dev)
    h, w = 2 * P + 300, 3 * P + 211
    host = synth.synth_slide(h, w, P + n)
    slide = torch.from_numpy(host).to(dev)
    o = _origins(h, w, P, n, n)
    o_dev = torch.from_numpy(o).to(dev)
    sel = _select(n, arch)
    taps = _Taps(m, arch, slide, o_dev, P, sel)
    layers, shapes = _shapes(ref, P)
    last_use = {}
    for i, L in enumerate(layers):
        for s in (L["src"], L["res"], L["name"]):
            last_use[s] = i
    x = tiling.features_nchw_predictor(host, o[sel], P).astype(np.float64)
    if dtype == "bf16":
        x = torch.from_numpy(x).bfloat16().double().numpy()
    fused_stem = dtype == "bf16"
    fractions = {}
    for i, L in enumerate(layers):
        name = L["name"]
        cout, cin, ks = L["shape"]
        w_, sc, sh = _operands(m, arch, L)
        src = x if L["src"] == "input" else taps.get(L["src"], shapes[L["src"]])
        res = taps.get(L["res"], shapes[L["res"]]) if L["res"] else None
        pool = name == "conv1" and fused_stem
        want, A = lr.conv_epilogue(src, w_, sc, sh, L["stride"], res, L["relu"], pool=pool, fmt=dtype)
        got = taps.get(name, shapes["maxpool"] if pool else shapes[name])
        assert got.shape == want.shape, name
        ok = lr.gate_mask(got, want, A, lr.rounding_count(cin, ks, dtype, res is not None), dtype)
        assert ok.all(), _fail_report(f"{arch} {dtype} P={P} n={n} {name}", got, want, A, ok, sel)
        fractions[name] = float((got == want).mean())
        if name == "conv1":   # the float32 stem also stores its pooled map; the fused bf16 stems store only that, under both names
            pooled = taps.get("maxpool", shapes["maxpool"])
            assert np.array_equal(pooled, got if fused_stem else F.max_pool2d(torch.from_numpy(got), 3, 2, 1).numpy()), "maxpool"
        for s in [k for k, v in last_use.items() if v == i]:
            taps.cache.pop(s, None)
    # head: logits of the same runs (identical in every tapped run and to an untapped forward) vs float64 fc(avgpool(last))
    plain = m.forward_tiles(slide, o_dev, P).cpu()
    assert all(torch.equal(lg, plain) for lg in taps.logits), "a tap changed the logits"
    last = taps.get(layers[-1]["name"], shapes[layers[-1]["name"]])
    sd = ref.state_dict()
    want = lr.head(last, sd["fc.weight"].double().numpy(), sd["fc.bias"].double().numpy())
    got = plain.numpy()[sel].astype(np.float64)
    assert np.all(np.abs(got - want) <= 1e-5 * (1 + np.abs(want))), f"head: max |d| = {np.abs(got - want).max():.3g}"
    worst = min(fractions, key=fractions.get)
    print(f"\n{arch} {dtype} P={P} n={n}: identical fraction min {fractions[worst]:.4f} ({worst}), "
          f"mean {np.mean(list(fractions.values())):.4f}")
    assert fractions[worst] >= IDENTICAL[dtype], f"{worst}: only {fractions[worst]:.4f} of the elements identical"


def test_resnet18_operands_are_the_rounded_weights_and_eval_bn(dev):
    """bf16 engine: every conv weight the kernels read is w.bfloat16(), bit for bit; float32 engine: w itself.  Scale and shift of both:
    float64 eval BN rounded once to float32."""
    ref = _oracle("r18")
    sd = {k: v.double().numpy() for k, v in ref.state_dict().items()}
    for dtype in ("bf16", "f32"):
        m = _model(ref, "r18", dtype, dev)
        layers, _ = _shapes(ref, 64)
        for L in layers:
            w, sc, sh = _operands(m, "r18", L)
            w0 = ref.state_dict()[L["name"] + ".weight"]
            want = (w0.bfloat16() if dtype == "bf16" else w0).float().numpy()
            assert np.array_equal(w, want), (dtype, L["name"])
            s, b = lr.bn_scale_shift(*(sd[L["bn"] + k] for k in (".weight", ".bias", ".running_mean", ".running_var")))
            assert np.array_equal(sc, s.astype(np.float32)) and np.array_equal(sh, b.astype(np.float32)), (dtype, L["name"])


def test_resnet50_folded_operands_within_half_ulp_of_float64_fold(dev):
    """The folded ResNet-50 weight (host fold in double, then float32, then bf16) against the float64 fold rounded ONCE to bf16: within
    half a bf16 ulp (+ half a float32 ulp: the float32 step can land on a bf16 tie) of the exact fold, and identical but for the double
    roundings: FOLD_MISMATCH of the 23.5 M weights (seed 5, bn3 x 0.2; the fold is host arithmetic, the same on every machine).  The bias is the float64 fold rounded once to float32; scale is 1."""
    FOLD_MISMATCH = 229
    ref = _oracle("r50")
    sd = {k: v.double().numpy() for k, v in ref.state_dict().items()}
    m = _model(ref, "r50", "bf16", dev)
    layers, _ = _shapes(ref, 64)
    mismatch = 0
    for L in layers:
        w, sc, sh = _operands(m, "r50", L)
        wf, b = lr.fold_bn(sd[L["name"] + ".weight"], *(sd[L["bn"] + k] for k in (".weight", ".bias", ".running_mean", ".running_var")))
        d = np.abs(w.astype(np.float64) - wf)
        assert np.all(d <= 0.5 * lr.quantum(wf, "bf16") + 0.5 * lr.quantum(wf, "f32")), L["name"]
        mismatch += int((w != lr.round_to(wf, "bf16")).sum())
        assert np.all(sc == 1) and np.array_equal(sh, b.astype(np.float32)), L["name"]
    assert mismatch <= FOLD_MISMATCH, f"{mismatch} folded weights differ from the single rounding"
