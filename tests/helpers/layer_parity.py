"""The layer-parity machinery of tests/test_gpu_layer_parity.py and tests/test_gpu_layer_parity_range.py: the oracle and the engine
built from it, tile origins, the selected images, the engines' operands and tapped activations, and `check_forward`, which holds
every stored activation of one launch element-wise to the float64 layer reference (oracle/layer_ref.py) and the logits to the
float64 head of the tapped last activation.  RANGE_CASES is the case list of the range file; tests/test_layer_reference_host.py
walks it through the launch plan (tests/host/conv3_plan_probe.cpp) without a GPU."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import layer_ref as lr
from oracle import resnet18 as o18
from oracle import resnet50 as o50
from oracle import synth, tiling

# floor of the fraction of elements bit-identical to `want`, per layer (measured minimum of any layer and case of
# tests/test_gpu_layer_parity.py: 0.9997 / 0.1303); tests/test_gpu_layer_parity.py states its own and passes them to check_forward
IDENTICAL = {"bf16": 0.999, "f32": 0.12}

# (arch, dtype, P, n) of tests/test_gpu_layer_parity_range.py; what each P reaches is tabulated in that file's docstring
RANGE_CASES = ([("r18", "bf16", 32, n) for n in (4096, 5)] + [("r18", "f32", 32, n) for n in (1024, 5)]
               + [("r18", dt, P, n) for P, ns in ((97, (1021, 5)), (200, (311, 300, 5)), (330, (300, 3)), (512, (64, 2)))
                  for dt in ("bf16", "f32") for n in ns]
               + [("r18", "f32", 256, 2600), ("r18", "bf16", 320, 3300)]
               + [("r50", "bf16", P, n) for P in (64, 160) for n in (1021, 5)])
# the ONE (case, layer) of RANGE_CASES whose geometry falls under a shared floor with every element inside the gate (a 1 x 1 map: 42 x 512
# elements; measured device fraction 0.1144 against 0.12): its floor is half the identical fraction of the float32 CPU evaluation of the
# same layer (measured 0.1125, floor 0.0562), computed when the case runs.  Every other layer of every case stays at IDENTICAL.
OWN_FLOOR = {("r18", "f32", 32, 1024): {"layer4.0.downsample.0"}}
BAND_CASES = {("r18", "f32", 256, 2600), ("r18", "bf16", 320, 3300)}   # layer-1 maps between 2^31 and 2^32 bytes


def r18_conv3_launches(dtype, P, n):
    """The 3x3 launches of one ResNet-18 forward as forward_impl issues them: (esz, B, Hi, cin, cout, stride, blocked, out16, wide, ds).  bf16:
    channel-blocked; a stride-2 conv whose output is wider than 4 runs on the wide kernel, and the conv before it writes 16-channel planes.
    A restatement of the block loop of forward_impl (deephisto_amd/csrc/resnet_kernels.hip: `x16`, the `launch_conv3x3` / `run_conv` calls) and of
    `s2_wide_eligible` (csrc/conv3_plan_host.h); a change there must be made here.  What ties the two together on a device: LAST_VARIANT."""
    bf = dtype == "bf16"
    esz, H, c = (2 if bf else 4), ((P - 1) // 2 + 1 - 1) // 2 + 1, 64
    out = []
    for stage in range(4):
        if stage:
            Ho = (H - 1) // 2 + 1
            out.append((esz, n, H, c, 2 * c, 2, int(bf), 0, int(bf and Ho > 4), 1))
            H, c = Ho, 2 * c
        next_wide = bf and stage < 3 and ((H - 1) // 2 + 1) > 4
        convs = 4 if stage == 0 else 3
        out += [(esz, n, H, c, c, 1, int(bf), int(next_wide and i == convs - 1), 0, 0) for i in range(convs)]
    return out


# stride-1 tile variant (0 / 1 / 2 = 512 / 256 / 128 pixels) of the LAST 3x3 launch of a ResNet-18 forward, layer4.1.conv2, per case: the host
# test requires it of r18_conv3_launches through the launch plan, the GPU test of the engine's own report (dh_debug_last_conv3)
LAST_VARIANT = {('bf16', 32, 4096): 1, ('bf16', 32, 5): 2, ('f32', 32, 1024): 1, ('f32', 32, 5): 2, ('bf16', 97, 1021): 1, ('bf16', 97, 5): 2, ('f32', 97, 1021): 1,
                ('f32', 97, 5): 2, ('bf16', 200, 311): 0, ('bf16', 200, 300): 1, ('bf16', 200, 5): 2, ('f32', 200, 311): 0, ('f32', 200, 300): 1, ('f32', 200, 5): 2,
                ('bf16', 330, 300): 0, ('bf16', 330, 3): 2, ('f32', 330, 300): 0, ('f32', 330, 3): 2, ('bf16', 512, 64): 0, ('bf16', 512, 2): 2, ('f32', 512, 64): 0,
                ('f32', 512, 2): 2, ('f32', 256, 2600): 0, ('bf16', 320, 3300): 0}


def _oracle(arch, n_classes=5):
    if arch == "r18":
        return o18.seeded_model(321, n_classes, perturb_bn=True).eval()
    ref = o50.seeded_model(5, n_classes, perturb_bn=True)
    with torch.no_grad():
        for name, mod in ref.named_modules():
            if name.endswith("bn3"):
                mod.weight.mul_(0.2)
    return ref.eval()


def _model(ref, arch, dtype, dev):
    from deephisto_amd.models.patch_cls_simple.model import get_model
    n_classes = ref.fc.out_features
    m = get_model(n_classes, compute_dtype=dtype) if arch == "r18" else get_model(n_classes, arch="resnet50")
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


def pooled_side(P):
    return ((P - 1) // 2 + 1 - 1) // 2 + 1


def band_indices(P, n, esz):
    """The first image whose layer-1 map (pooled side^2 x 64 channels x esz bytes) starts past byte 2^31 of its buffer, and the first
    past byte 3 * 2^30: those of them the launch reaches."""
    img = pooled_side(P) ** 2 * 64 * esz
    return [i for i in ((1 << 31) // img + 1, (3 << 30) // img + 1) if i < n]


def range_select(arch, dtype, P, n):
    """Selected images of a RANGE_CASES case.  P <= 256: `_select`.  Larger patches: the float64 reference costs what P = 256 costs --
    the largest set with len(sel) * P^2 <= 16 * 256^2, at least 3 (all of a smaller launch), evenly spaced, always with image 0, the
    middle image n // 2 and image n - 1.  The two band cases: `_select` and eight images straddling each index of `band_indices`."""
    if (arch, dtype, P, n) in BAND_CASES:
        extra = [np.arange(i - 4, i + 4) for i in band_indices(P, n, 2 if dtype == "bf16" else 4)]
        idx = np.concatenate([_select(n, arch)] + extra)
        return np.unique(idx[(idx >= 0) & (idx < n)]).astype(np.int32)
    if P <= 256:
        return _select(n, arch)
    k = max(3, 16 * 256 * 256 // (P * P))
    if n <= k:
        return np.arange(n, dtype=np.int32)
    idx = np.linspace(0, n - 1, k).round().astype(int)
    idx[k // 2] = n // 2
    return np.unique(idx).astype(np.int32)


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
            lg = torch.empty((len(self.o_dev), self.m.n_classes), dtype=torch.float32, device=self.slide.device)
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


def float32_identical_fraction(src, w_, sc, sh, stride, res, relu, pool, fmt, want):
    """The fraction of an independent float32 evaluation of the layer (torch's CPU convolution from the same operands, the epilogue in
    float32, ONE rounding to the storage type -- as tests/test_layer_reference_host.py does for the training cases) that is
    bit-identical to `want`: what a correct float32 engine reaches on this geometry."""
    f = lambda t: torch.as_tensor(np.asarray(t), dtype=torch.float32)  # noqa: E731
    y = F.conv2d(f(src), f(w_), None, stride, w_.shape[-1] // 2) * f(sc)[None, :, None, None] + f(sh)[None, :, None, None]
    if res is not None:
        y = y + f(res)
    if relu:
        y = F.relu(y)
    y = lr.round_to(y.double().numpy(), fmt)
    if pool:
        y = F.max_pool2d(torch.from_numpy(y), 3, 2, 1).numpy()
    return float((y == want).mean())


def launch(dev, arch, dtype, P, n, n_classes=5):
    """The oracle, the engine built from it, the synthetic slide (host and device) and the n tile origins (host and device) of a case."""
    ref = _oracle(arch, n_classes)
    m = _model(ref, arch, dtype, dev)
    h, w = 2 * P + 300, 3 * P + 211
    host = synth.synth_slide(h, w, P + n)
    o = _origins(h, w, P, n, n)
    return ref, m, host, torch.from_numpy(host).to(dev), o, torch.from_numpy(o).to(dev)


def check_head(ref, m, taps, slide, o_dev, P, layers, shapes, sel):
    """The plain forward's logits: bit-equal to those of every tapped run so far, and the selected rows within 1e-5 (1 + |want|) of the
    float64 fc(avgpool) of the tapped last activation.  Returns (identical fraction, worst |got - want| / gate)."""
    last = taps.get(layers[-1]["name"], shapes[layers[-1]["name"]])
    plain = m.forward_tiles(slide, o_dev, P).cpu()
    assert plain.shape == (len(o_dev), m.n_classes)
    assert all(torch.equal(lg, plain) for lg in taps.logits), "a tap changed the logits"
    sd = ref.state_dict()
    want = lr.head(last, sd["fc.weight"].double().numpy(), sd["fc.bias"].double().numpy())
    got = plain.numpy()[sel].astype(np.float64)
    assert got.shape == want.shape == (len(sel), m.n_classes)
    ratio = np.abs(got - want) / (1e-5 * (1 + np.abs(want)))
    assert np.all(np.abs(got - want) <= 1e-5 * (1 + np.abs(want))), f"head: max |d| = {np.abs(got - want).max():.3g}"
    return float((got == want).mean()), float(ratio.max())


def check_forward(dev, arch, dtype, P, n, sel=None, n_classes=5, identical=None, own_floor=()):
    """One launch of n tiles of P x P: every stored activation of the images `sel` (None: `_select`) inside `gate_mask` of the float64
    reference of that layer on the engine's own operands; the pooled map against the stem; the logits of every tapped run bit-equal
    to the plain forward's and within 1e-5 (1 + |want|) of the float64 head of the tapped last activation; per layer at least
    identical[dtype] (None: IDENTICAL) of the elements bit-identical to `want`.  own_floor: the names of the layers of THIS case whose
    floor is instead half the identical fraction of `float32_identical_fraction` (never above the shared one) -- a number of the
    reference, not of the kernel.
    Returns {layer: (identical fraction, worst |got - want| / gate)} with the head under "fc"."""
    identical = IDENTICAL if identical is None else identical
    ref, m, host, slide, o, o_dev = launch(dev, arch, dtype, P, n, n_classes)
    if sel is None:
        sel = _select(n, arch)
    taps = _Taps(m, arch, slide, o_dev, P, sel)
    layers, shapes = _shapes(ref, P)
    assert set(own_floor) <= {L["name"] for L in layers}, own_floor
    last_use = {}
    for i, L in enumerate(layers):
        for s in (L["src"], L["res"], L["name"]):
            last_use[s] = i
    x = tiling.features_nchw_predictor(host, o[sel], P).astype(np.float64)
    if dtype == "bf16":
        x = torch.from_numpy(x).bfloat16().double().numpy()
    fused_stem = dtype == "bf16"
    fractions, ratios, floors = {}, {}, {}
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
        K = lr.rounding_count(cin, ks, dtype, res is not None)
        ok = lr.gate_mask(got, want, A, K, dtype)
        assert ok.all(), _fail_report(f"{arch} {dtype} P={P} n={n} {name}", got, want, A, ok, sel)
        fractions[name] = float((got == want).mean())
        ratios[name] = float((np.abs(got - want) / (lr.quantum(want, dtype) + lr.gamma(K) * A)).max())
        floors[name] = identical[dtype]
        if name in own_floor:
            f32 = float32_identical_fraction(src, w_, sc, sh, L["stride"], res, L["relu"], pool, dtype, want)
            floors[name] = min(identical[dtype], 0.5 * f32)
            print(f"\n{arch} {dtype} P={P} n={n} {name}: device identical fraction {fractions[name]:.4f}, float32 CPU evaluation "
                  f"{f32:.4f}, derived floor {floors[name]:.4f}")
        if name == "conv1":   # the float32 stem also stores its pooled map; the fused bf16 stems store only that, under both names
            pooled = taps.get("maxpool", shapes["maxpool"])
            assert np.array_equal(pooled, got if fused_stem else F.max_pool2d(torch.from_numpy(got), 3, 2, 1).numpy()), "maxpool"
        for s in [k for k, v in last_use.items() if v == i]:
            taps.cache.pop(s, None)
    # head: logits of the same runs (identical in every tapped run and to an untapped forward) vs float64 fc(avgpool(last))
    head = check_head(ref, m, taps, slide, o_dev, P, layers, shapes, sel)
    worst = min(fractions, key=lambda k: fractions[k] - floors[k])
    low = min(fractions, key=fractions.get)
    top = max(ratios, key=ratios.get)
    print(f"\n{arch} {dtype} P={P} n={n}: identical fraction min {fractions[low]:.4f} ({low}), "
          f"mean {np.mean(list(fractions.values())):.4f}; worst |got - want| / gate {ratios[top]:.3f} ({top}), "
          f"head {head[1]:.3f}; {len(sel)} images")
    assert fractions[worst] >= floors[worst], f"{worst}: only {fractions[worst]:.4f} of the elements identical (floor {floors[worst]:.4f})"
    out = {k: (fractions[k], ratios[k]) for k in fractions}
    out["fc"] = head
    return out
