"""GPU: every conv weight gradient of a training step, as the step computes it, element by element against float64 -- and every stored Z of
the training forward (oracle/wgrad_ref.py, oracle/layer_ref.py; the reference and its conditions: tests/test_wgrad_reference_host.py).

The kernels have float64 tests through their debug hooks; this module holds the backward pass AS A STEP RUNS IT (t2_backward / tr_backward):
side-stream weight gradients that read each conv's own dZ long after it was written, one slab buffer shared by all convs, n_slabs == 1
writing straight into the gradient arena, pre-masked blocks, BN-backward sums left by dgrad epilogues, join fusion and fold.  After one
step (m.train(), forward, cross entropy, loss.backward(); no fused Adam) every conv still holds its dZ, its input and its Z
(dh_train2_debug_act / dh_resnet18_train_debug_act, what = 0 Z, 1 Y, 2 dZ, 3 X1), so every weight gradient is recomputed in float64 from
exactly the operands the engine's kernel read: a wrong operand hand-off, a stale dZ or a slab plan that differs in the engine shows here.

  (a) weight gradients  for every conv of oracle.layer_ref.topology (stem and downsamples included): p.grad against wgrad(x, dz) with x the
                        stored tensor the conv reads (Y of its producer, X1, or the image -- rounded to bf16 for the bf16 engine, as its
                        stem kernels read it) and dz the tap.  Every element: |got - want| <= quantum(want) + gamma_K A, K = N - 1 (bf16) /
                        2N - 1 (f32), N = B Ho Wo; per tensor: relative L2 <= 1e-5.  Both derived in oracle/wgrad_ref.py, neither measured.
  (b) training Z        tap 0 against conv_epilogue(src, w, 1, 0) (w = weight.bfloat16() / the float32 weight) under lr.gate_mask with
                        K = rounding_count(cin, ks, fmt, False); bf16 storage also meets the identical-fraction floor 0.999.  This is the
                        only place gemm1x1_f32 runs forward (the f32 engine's downsample conv: stride-2 row gather, master weights in
                        place, clamped rows where M is no multiple of 128); its identical fraction is printed, no floor is known for it.
  (c) read-only taps    the same forward and backward twice from the same state: every p.grad and every dZ bit-identical.  The first run
                        is not tapped before its gradients are read; the second is tapped between forward and backward.
  (d) refusals          what = 2 before a backward and after a new forward, what = 2 on an engine created with DH_T2_SIDE=0 /
                        DH_T1_SIDE=0, what = 3 for another conv, a wrong n_elem, what = 4: -22, dh_last_error() names the argument.

Cases (the smallest shapes that reach these paths):
  bf16 resnet18 B=5  P=96   maps 48 / 24 / 12 / 6 / 3: row pitches that are no multiple of 4 or of the 64-pixel step, an odd 3 x 3 map,
                            45 pixels = one partial step, odd batch
  bf16 resnet50 B=3  P=96   ring / quad 1x1 kernels with M = 27 .. 1728, n_slabs from 1 up, strided 1x1 downsample
  bf16 resnet50 B=6  P=64   2 x 2 maps in layer 4, N = 24
  bf16 resnet18 B=16 P=64   several images per slab, stem N = 16 384
  f32  resnet18 B=5  P=96   gemm1x1_f32 forward with M = 720 / 180 / 45 and stride-2 gather from 24 / 12 / 6-wide maps; wgrad3_kernel,
                            the per-tap fallback, wgrad_kernel
  f32  resnet18 B=2  P=64

Measured on an MI355X (records only, no threshold is derived from them; every element of every case inside both conditions; the file:
9.7 s wall for its 23 tests, the slowest case 2.0 s), in the order of the cases above:
  worst |got - want| / gate of dW   0.082 layer4.1.conv2 (N = 45) | 0.135 layer4.2.conv2 (N = 27) | 0.127 layer4.0.conv2 (N = 24) |
                                    0.056 layer4.1.conv1 (N = 64) | 0.055 layer4.0.conv2 (N = 45) | 0.213 layer4.0.conv1 (N = 8)
  worst relative L2 of dW           7.1e-7 | 4.3e-7 | 4.1e-7 | 8.2e-7 (conv1, the stem, in all four bf16 cases) | 2.8e-7 | 2.6e-7 (layer1.0.conv1)
  lowest identical fraction of Z    0.9997 layer4.0.conv1 | 0.9997 layer4.2.conv1 | 0.9998 layer3.4.conv2 | 0.9998 layer3.0.conv2 |
                                    0.047 layer4.0.conv2 | 0.051 layer4.1.conv2 (float32: mean 0.089 / 0.091 over the layers)
The worst ratios sit on the smallest maps, where gamma_K A is small next to the float32 unit of `want`.

Out of scope here, the next slices: training-mode Y from Z with batch statistics (the coefficient error needs the chain-length bounds of
oracle/bn_state_ref.py carried into scale and shift); the float32 engine's backward chain (dgamma / dbeta and the dZ chain of tr_backward:
the bf16 engine's are held by tests/test_gpu_step_bwd.py, which taps each BN's incoming gradient during the pass).  The fc gradients:
tests/test_gpu_head.py.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import layer_ref as lr
from oracle import resnet18 as o18
from oracle import resnet50 as o50
from oracle import wgrad_ref as wr

pytestmark = pytest.mark.gpu

IDENTICAL = {"bf16": 0.999}   # floor of the fraction of Z bit-identical to `want` (tests/test_gpu_layer_parity.py); f32: printed only

CASES = [("bf16", "resnet18", 5, 96), ("bf16", "resnet50", 3, 96), ("bf16", "resnet50", 6, 64), ("bf16", "resnet18", 16, 64),
         ("f32", "resnet18", 5, 96), ("f32", "resnet18", 2, 64)]
SEED = {"resnet18": 321, "resnet50": 5}


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _tap_fn(fmt):
    from deephisto_amd._lib import lib
    return lib().dh_train2_debug_act if fmt == "bf16" else lib().dh_resnet18_train_debug_act


def _tap(eng, fmt, name, what, shape, dev):
    """Stored tensor of conv `name` as float32 NCHW (the engines keep it channels last)."""
    from deephisto_amd._lib import check
    b, c, h, w = shape
    buf = torch.empty(b * c * h * w, dtype=torch.float32, device=dev)
    check(_tap_fn(fmt)(eng.handle, name.encode(), what, buf.data_ptr(), buf.numel(), None), f"debug_act {name} what={what}")
    return np.ascontiguousarray(buf.cpu().numpy().reshape(b, h, w, c).transpose(0, 3, 1, 2))


def _model(fmt, arch, dev):
    from deephisto_amd.models.patch_cls_simple.model import get_model
    ref = (o50 if arch == "resnet50" else o18).seeded_model(SEED[arch], 5, perturb_bn=True)
    m = get_model(5, fmt, arch=arch)
    m.load_state_dict(ref.state_dict())
    return ref, m.to(dev).train()


def _shapes(ref, B, P):
    """[B][C][H][W] of every conv output and of the pooled stem map."""
    shapes = {}
    convs = {n: mod for n, mod in ref.named_modules() if isinstance(mod, torch.nn.Conv2d)}
    hooks = [mod.register_forward_hook(lambda _m, _i, out, n=n: shapes.__setitem__(n, (B,) + tuple(out.shape[1:]))) for n, mod in convs.items()]
    with torch.no_grad():
        ref.eval()(torch.zeros(1, 3, P, P))
    for h in hooks:
        h.remove()
    h2 = (shapes["conv1"][2] - 1) // 2 + 1
    shapes["maxpool"] = (B, 64, h2, h2)
    return shapes


def _one_step(m, x, labels):
    m.zero_grad(set_to_none=True)
    loss = F.cross_entropy(m(x), labels)
    return loss


@functools.lru_cache(maxsize=None)
def _step(case):
    """One case's two identical steps, as host arrays: the second run's gradients and taps, and what (c) compares them with."""
    fmt, arch, B, P = case
    dev = torch.device("cuda:0")
    ref, m = _model(fmt, arch, dev)
    eng = m._engine
    topo = lr.topology(ref)
    shapes = _shapes(ref, B, P)
    g = torch.Generator().manual_seed(1000 * B + P)
    x = torch.rand(B, 3, P, P, generator=g).to(dev)
    labels = torch.randint(0, 5, (B,), generator=g).to(dev)
    grads = lambda: {n: p.grad.detach().cpu().numpy().copy() for n, p in m.named_parameters()}  # noqa: E731
    dzs = lambda: {L["name"]: _tap(eng, fmt, L["name"], 2, shapes[L["name"]], dev) for L in topo}  # noqa: E731
    # run 1: no tap before its gradients are read
    _one_step(m, x, labels).backward()
    grads1 = grads()
    dz1 = dzs()
    # run 2 from the same state, tapped between forward and backward, and after
    loss = _one_step(m, x, labels)
    Z = {L["name"]: _tap(eng, fmt, L["name"], 0, shapes[L["name"]], dev) for L in topo}
    srcs = {L["src"] for L in topo} - {"input", "maxpool"}
    Y = {n: _tap(eng, fmt, n, 1, shapes[n], dev) for n in srcs}
    Y["maxpool"] = _tap(eng, fmt, "conv1", 3, shapes["maxpool"], dev)
    loss.backward()
    grads2 = grads()
    dz2 = dzs()
    xh = x.cpu()
    Y["input"] = (xh.bfloat16().float() if fmt == "bf16" else xh).numpy()     # the bf16 stem kernels round the image on its way into LDS
    weights = {L["name"]: ref.state_dict()[L["name"] + ".weight"].clone() for L in topo}
    m._release()
    return dict(topo=topo, shapes=shapes, grads1=grads1, dz1=dz1, grads=grads2, dz=dz2, Z=Z, Y=Y, weights=weights)


TAPS3 = (("corner (0,0)", 0, 0), ("corner (0,2)", 0, 2), ("corner (2,0)", 2, 0), ("corner (2,2)", 2, 2), ("centre (1,1)", 1, 1))


def _fail_report(tag, got, want, A, ratio, l2):
    bad = np.argwhere(ratio > 1.0)
    lines = [f"{tag}: {len(bad)} of {ratio.size} elements outside the gate, relative L2 {l2:.3g} (<= {wr.REL_L2:g}); "
             f"first (cout, cin, ky, kx): got / want / A"]
    for co, ci, ky, kx in bad[:8]:
        lines.append(f"  ({co}, {ci}, {ky}, {kx}): {float(got[co, ci, ky, kx])!r} / {float(want[co, ci, ky, kx])!r} / {A[co, ci, ky, kx]:.3g}")
    if len(bad):
        lines.append(f"  couts {np.unique(bad[:, 0])[:16].tolist()} ({len(np.unique(bad[:, 0]))}), cins {np.unique(bad[:, 1])[:16].tolist()} "
                     f"({len(np.unique(bad[:, 1]))}), taps {sorted(set((int(a), int(b)) for a, b in bad[:, 2:]))}")
    if got.shape[-1] == 3:
        for label, ky, kx in TAPS3:
            r = ratio[:, :, ky, kx]
            lines.append(f"  {label}: {int((r > 1.0).sum())} outside, worst |d| / gate {r.max():.3g}, "
                         f"relative L2 {wr.rel_l2(got[:, :, ky, kx], want[:, :, ky, kx]):.3g}")
    return "\n".join(lines)


@pytest.mark.parametrize("fmt,arch,B,P", CASES)
def test_every_conv_weight_gradient_matches_float64(dev, fmt, arch, B, P):
    s = _step((fmt, arch, B, P))
    worst, worst_l2, reports = (0.0, ""), (0.0, ""), []
    for L in s["topo"]:
        name = L["name"]
        got = s["grads"][name + ".weight"].astype(np.float64)
        x, dz = s["Y"][L["src"]], s["dz"][name]
        want, A = wr.wgrad(x, dz, got.shape[-1], L["stride"])
        assert got.shape == want.shape, name
        K = wr.rounding_count(wr.terms(dz.shape), fmt)
        ratio, l2 = wr.gate_ratio(got, want, A, K), wr.rel_l2(got, want)
        if float(ratio.max()) > worst[0]:
            worst = (float(ratio.max()), f"{name} (N = {wr.terms(dz.shape)})")
        if l2 > worst_l2[0]:
            worst_l2 = (l2, name)
        if float(ratio.max()) > 1.0 or l2 > wr.REL_L2:
            reports.append(_fail_report(f"{fmt} {arch} B={B} P={P} {name} dW", got, want, A, ratio, l2))
    print(f"\n[step wgrad] {fmt} {arch} B={B} P={P}: worst |got - want| / gate {worst[0]:.3f} at {worst[1]}; "
          f"worst relative L2 {worst_l2[0]:.2e} at {worst_l2[1]}")
    assert not reports, "\n".join(reports)


@pytest.mark.parametrize("fmt,arch,B,P", CASES)
def test_every_training_forward_z_matches_float64(dev, fmt, arch, B, P):
    s = _step((fmt, arch, B, P))
    fractions, reports = {}, []
    for L in s["topo"]:
        name = L["name"]
        w = s["weights"][name]
        w = (w.bfloat16() if fmt == "bf16" else w).double().numpy()
        cout, cin, ks, _ = w.shape
        want, A = lr.conv_epilogue(s["Y"][L["src"]], w, np.ones(cout), np.zeros(cout), L["stride"], None, relu=False, fmt=fmt)
        got = s["Z"][name].astype(np.float64)
        assert got.shape == want.shape, name
        ok = lr.gate_mask(got, want, A, lr.rounding_count(cin, ks, fmt, False), fmt)
        fractions[name] = float((got == want).mean())
        if not ok.all():
            bad = np.argwhere(~ok)
            lines = [f"{fmt} {arch} B={B} P={P} {name} Z: {len(bad)} of {ok.size} elements outside the gate; first (image, channel, y, x): got / want / A"]
            lines += [f"  ({i}, {c}, {y}, {x_}): {float(got[i, c, y, x_])!r} / {float(want[i, c, y, x_])!r} / {A[i, c, y, x_]:.3g}" for i, c, y, x_ in bad[:8]]
            lines.append(f"  images {np.unique(bad[:, 0])[:16].tolist()}, channels {np.unique(bad[:, 1])[:16].tolist()}, "
                         f"rows {np.unique(bad[:, 2])[:16].tolist()}, cols {np.unique(bad[:, 3])[:16].tolist()}")
            reports.append("\n".join(lines))
    low = min(fractions, key=fractions.get)
    print(f"\n[step wgrad] {fmt} {arch} B={B} P={P}: Z identical fraction min {fractions[low]:.4f} ({low}), mean {np.mean(list(fractions.values())):.4f}")
    assert not reports, "\n".join(reports)
    if fmt in IDENTICAL:
        assert fractions[low] >= IDENTICAL[fmt], f"{low}: only {fractions[low]:.4f} of the elements identical"


@pytest.mark.parametrize("fmt,arch,B,P", CASES)
def test_taps_are_read_only_and_backward_is_bit_reproducible(dev, fmt, arch, B, P):
    s = _step((fmt, arch, B, P))
    assert s["grads1"].keys() == s["grads"].keys() and len(s["grads"]) > 60
    for n, g in s["grads"].items():
        assert np.array_equal(s["grads1"][n].view(np.uint32), g.view(np.uint32)), f"{n}.grad differs between two identical steps"
    for n, d in s["dz"].items():
        assert np.array_equal(s["dz1"][n].view(np.uint32), d.view(np.uint32)), f"dZ of {n} differs between two identical steps"
        assert np.isfinite(d).all() and np.any(d != 0), n


@pytest.mark.parametrize("fmt,arch", [("bf16", "resnet18"), ("bf16", "resnet50"), ("f32", "resnet18")])
def test_refusals_name_the_argument(dev, fmt, arch):
    from deephisto_amd._lib import lib
    B, P = 2, 64
    ref, m = _model(fmt, arch, dev)
    shapes = _shapes(ref, B, P)
    x = torch.rand(B, 3, P, P).to(dev)
    labels = torch.tensor([1, 3], device=dev)
    fn = _tap_fn(fmt)
    other = "layer1.0.conv1"
    n1, n0, nx = int(np.prod(shapes[other])), int(np.prod(shapes["conv1"])), int(np.prod(shapes["maxpool"]))
    buf = torch.empty(max(n0, n1), dtype=torch.float32, device=dev)

    def refused(name, what, n, *words):
        assert fn(m._engine.handle, name.encode(), what, buf.data_ptr(), n, None) == -22, (name, what, n)
        err = lib().dh_last_error()
        assert all(w in err for w in words), err

    with torch.no_grad():
        m(x)                                                   # a training forward, no backward yet
    refused(other, 2, n1, b"what = 2", b"backward")
    refused("conv1", 2, n0, b"what = 2", b"backward")
    refused(other, 3, n1, b"what = 3", b"conv1")
    refused(other, 3, nx, b"what = 3", b"conv1")
    refused(other, 0, n1 - 8, b"n_elem")
    refused("conv1", 3, n0, b"n_elem")
    refused(other, 4, n1, b"what = 4")
    refused(other, -1, n1, b"what = -1")
    refused("layer9.0.conv1", 0, n1, b"conv_name")
    if fmt == "f32":
        refused("conv1", 1, n0, b"what = 1")                   # the float32 stem's Y is never stored, and the taps do not write
    _one_step(m, x, labels).backward()
    for name, what, n in ((other, 2, n1), ("conv1", 2, n0), ("conv1", 3, nx), (other, 0, n1)):
        assert fn(m._engine.handle, name.encode(), what, buf.data_ptr(), n, None) == 0, (name, what)
    with torch.no_grad():
        m(x)                                                   # a new forward: the dZ buffers are last step's
    refused(other, 2, n1, b"what = 2", b"backward")
    refused("conv1", 2, n0, b"what = 2", b"backward")
    torch.cuda.synchronize()
    m._release()


@pytest.mark.parametrize("fmt,arch,knob", [("bf16", "resnet18", "DH_T2_SIDE"), ("f32", "resnet18", "DH_T1_SIDE")])
def test_dz_tap_is_refused_without_the_side_stream(dev, fmt, arch, knob, monkeypatch):
    from deephisto_amd._lib import lib
    monkeypatch.setenv(knob, "0")                              # read when the engine's training state is created (the first forward)
    B, P = 2, 64
    ref, m = _model(fmt, arch, dev)
    shapes = _shapes(ref, B, P)
    x = torch.rand(B, 3, P, P).to(dev)
    _one_step(m, x, torch.tensor([0, 4], device=dev)).backward()
    fn = _tap_fn(fmt)
    for name in ("layer2.0.downsample.0", "conv1"):
        n = int(np.prod(shapes[name]))
        buf = torch.empty(n, dtype=torch.float32, device=dev)
        assert fn(m._engine.handle, name.encode(), 2, buf.data_ptr(), n, None) == -22
        assert knob.encode() in lib().dh_last_error(), lib().dh_last_error()
        assert fn(m._engine.handle, name.encode(), 0, buf.data_ptr(), n, None) == 0      # Z is kept either way
    torch.cuda.synchronize()
    m._release()
