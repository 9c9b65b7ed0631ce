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

The machinery (taps, operands, selection, the body of the parametrised test) is tests/helpers/layer_parity.py, shared with
tests/test_gpu_layer_parity_range.py, which runs it over the rest of the sizes the engines accept.
"""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import layer_ref as lr

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import layer_parity as lp  # noqa: E402
from layer_parity import _model, _operands, _oracle, _shapes  # noqa: E402

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


@pytest.mark.parametrize("arch,dtype,P,n", CASES)
def test_every_stored_activation_matches_float64_reference(dev, arch, dtype, P, n):
    """tests/helpers/layer_parity.py, check_forward: the gate on every element, the pooled map, the logits, the IDENTICAL floors."""
    lp.check_forward(dev, arch, dtype, P, n, identical=IDENTICAL)


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
