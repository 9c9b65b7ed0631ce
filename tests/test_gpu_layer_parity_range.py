"""GPU: the float64 layer parity of tests/test_gpu_layer_parity.py over the rest of the range the inference engines accept.

ResNet-18 takes any patch 32 <= P <= 1024 and up to 4096 tiles, as long as its largest post-pool activation stays under 2^32 bytes; the
sibling file checks values at P in {96, 224, 256}.  Each case here is one call of tests/helpers/layer_parity.py `check_forward`: every stored
activation of every selected image element-wise inside `gate_mask` of the float64 reference, the logits within 1e-5 (1 + |want|) of the
float64 head of the tapped last activation, and the tapped runs' logits bit-equal to the plain forward's.  What the sizes reach (the
launch classes are checked against the engine's own plan, without a GPU, by tests/test_layer_reference_host.py
test_range_cases_reach_the_launch_classes_their_table_claims; its walk of the forward and the engine are tied together here by the tile
variant of the forward's last 3x3 launch, which the engine reports):

  r18 bf16 / f32  P = 32   n = 4096 / 1024, 5   maps 8 / 4 / 2 / 1: the 8 x 8 fit tile at cout 64 (eight images; float32 at n = 1024: the four-image
                                                tile); the 128-pixel stride-2 kernel at Wo = 4, 2, 1; the head averages one pixel
  r18 bf16 / f32  P = 97   n = 1021, 5          odd P: the stem's last column has three padded input columns; 49 -> 25 pool; 25 (16 x 32 ragged both
                                                ways), 13 (two-image 16 x 16), 7 x 7 fit x10 at cout 256 with a ragged last group, 4; odd-input
                                                stride-2 at 25 -> 13 (wide 16 x 16) and 13 -> 7 (wide, four images per 8 x 8 tile); 7 -> 4 on the
                                                128-pixel kernel, so layer 3 does not write 16-channel planes
  r18 bf16 / f32  P = 200  n = 311, 300, 5      50 (8 x 64 tiles ragged in x and y); 50 -> 25 (even in, odd out); 7 x 7 through an odd chain: ten images
                                                per fit tile at cout 512 from n = 311 (32 groups x 8 cout blocks = 256 tiles), five at n = 300
  r18 bf16 / f32  P = 330  n = 300, 3           83 (three 16 x 32 tile columns, the last ragged); 83 -> 42 and 21 -> 11 (odd in); 21 on ragged 16 x 32;
                                                11 on two-image tiles
  r18 bf16 / f32  P = 512  n = 64, 2            128 / 64 / 32 / 16 maps; channel-blocked planes of 1 MiB
  r18 f32         P = 256  n = 2600             layer-1 map of 2.73e9 bytes: window and output byte offsets past 2^31 (workspace ~ 19 GB)
  r18 bf16        P = 320  n = 3300             the same band in the channel-blocked layout: 2.70e9 bytes (~ 19 GB)
  r50 bf16        P = 64, 160  n = 1021, 5      2 x 2 and 5 x 5 last maps; 10 -> 5 stride-2 inside a bottleneck; the 5-wide map ragged in the four-image
                                                8 x 8 wide tile

Selected images (layer_parity.range_select): P <= 256: the sibling's `_select`; larger P: the largest evenly spaced set with
len(sel) * P^2 <= 16 * 256^2 (the float64 CPU cost of a P = 256 case), with images 0, n // 2 and n - 1; the two band cases: `_select` plus
eight images straddling the first index whose layer-1 map starts past byte 2^31 (2049 in float32, 2622 in bf16; neither launch reaches
byte 3 * 2^30: they end at 2.73e9 and 2.70e9 bytes).

Gates: `gate_mask` as derived in oracle/layer_ref.py, and the sibling's IDENTICAL floors (0.999 bf16, 0.12 float32) on the per-layer
fraction of bit-identical elements, on every layer of every case but one.  A layer of a new geometry that falls under the shared floor
with every element inside the gate is listed in layer_parity.OWN_FLOOR, and only there the floor is half the identical fraction of a
float32 CPU evaluation of the same layer from the same operands, rounded once to the storage type
(layer_parity.float32_identical_fraction): a number of the reference, not of the kernel.

Measured on one MI355X: every element of all 28 cases inside the gate -- none of the new geometries found a fault in the engines; the file
takes 78 s (the two band cases 12 s and 16 s, mostly the float64 reference of their 50 images; every other case 0.2 .. 5.3 s).  Per
case group, the worst |got - want| / gate over all layers and images, the lowest per-layer identical fraction, the worst head ratio:

  r18 bf16, P = 32 .. 512 (11 cases)   0.999 (layer2.0.downsample.0)   0.9998   head 0.029
  r18 f32,  P = 32 .. 512 (11 cases)   0.048 (layer2.0.downsample.0)   0.1144   head 0.071
  r18 f32  P = 256 n = 2600 (band)     0.041                           0.1314   head 0.039
  r18 bf16 P = 320 n = 3300 (band)     0.999                           0.9999   head 0.036
  r50 bf16, P = 64, 160 (4 cases)      0.999 (layer1.x.conv3)          0.9998   head 0.007

(bf16: a ratio just under 1 is one bf16 unit where the float32 sum straddles a rounding boundary, as in the sibling file.)  One layer fell
under a shared floor: layer4.0.downsample.0 of r18 f32 P = 32 n = 1024, a 1 x 1 map (42 x 512 elements), device fraction 0.1144; the
float32 CPU evaluation of the same layer is identical in 0.1125, so the derived floor is 0.0562: the one entry of OWN_FLOOR.  The same
layer at n = 5: 0.1203, held to the shared 0.12; every
other float32 case >= 0.1289 (the sibling's minimum: 0.1303).
"""
import ctypes as C
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import layer_parity as lp  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.mark.parametrize("arch,dtype,P,n", lp.RANGE_CASES)
def test_every_stored_activation_matches_float64_reference_over_the_accepted_range(dev, arch, dtype, P, n):
    sel = lp.range_select(arch, dtype, P, n)
    if (arch, dtype, P, n) in lp.BAND_CASES:   # the case exists for the images past byte 2^31: they must be among the checked ones
        first = lp.band_indices(P, n, 2 if dtype == "bf16" else 4)
        assert first and all(i - 1 in sel and i in sel for i in first), (first, sel)
    lp.check_forward(dev, arch, dtype, P, n, sel=sel, identical=lp.IDENTICAL, own_floor=lp.OWN_FLOOR.get((arch, dtype, P, n), ()))
    if arch == "r18":   # the forward's last 3x3 launch ran the tile variant the host walk of the launch plan expects (layer_parity.LAST_VARIANT)
        from deephisto_amd._lib import check, lib
        v, mfma = C.c_int32(-1), C.c_int32(0)
        check(lib().dh_debug_last_conv3(C.byref(v), C.byref(mfma)), "dh_debug_last_conv3")
        assert v.value == lp.LAST_VARIANT[(dtype, P, n)], (v.value, mfma.value)
