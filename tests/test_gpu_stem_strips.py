"""Fused bf16 stem: strips of 16 pooled columns joined by the seam pass against independent strips of 15.

A strip of 16 pooled columns computes the aligned 32-column conv tile; its first pooled column lacks the conv column to its left,
which the neighbouring strip writes to a seam scratch and stem_seam_kernel folds in with an integer max.  Every conv output goes
through the same MFMA sequence, BN and rounding in either width and the pooled maximum is over the same nine values, so the two
widths must agree BIT FOR BIT; the 15-column strips are the ones test_gpu_resnet.py checks against the torch-CPU restatement.

Measured on one MI355X: the file takes 4 s; the comparison is exact, so the worst |got - want| / gate of every case, the odd patches 97 and
255 included, is 0 differing elements."""
import numpy as np
import pytest
import torch

from oracle import resnet18 as oracle_net
from oracle import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _hip_model(oracle, dev):
    from deephisto_amd.models.patch_cls_simple.model import get_model
    m = get_model(5, compute_dtype="bf16")
    m.load_state_dict(oracle.state_dict(), strict=True)
    return m.to(dev).eval()


def _stem(model, slide, o_dev, n, P, width):
    from deephisto_amd._lib import check, lib
    H2 = ((P - 1) // 2 + 1 - 1) // 2 + 1
    got = torch.empty((n, H2, H2, 64), dtype=torch.float32, device=slide.device)
    check(lib().dh_debug_stem_strip_width(width), "dh_debug_stem_strip_width")
    try:
        check(lib().dh_debug_stem_pool_bf16(model._handle, slide.data_ptr(), slide.shape[0], slide.shape[1], o_dev.data_ptr(), n, P,
                                            got.data_ptr(), None), "dh_debug_stem_pool_bf16")
    finally:
        check(lib().dh_debug_stem_strip_width(0), "dh_debug_stem_strip_width")
    return got


@pytest.mark.parametrize("P,side", [(256, 700), (64, 64), (32, 90), (330, 700), (100, 300), (97, 300), (255, 700)])
def test_strip_widths_agree_bit_for_bit(dev, P, side):
    """Width 15 forced, width 16 forced and the width the launcher picks (16 at P = 256 and 64, 15 elsewhere): identical bits for
    every pooled pixel of tiles in all four slide corners (the slide-edge byte path) and of random tiles.  Forcing 16 exercises
    seams on every geometry: one at P = 100 (25 columns: the second strip ragged), five at P = 330, none at P = 32 and 64.  P = 97 and 255
    are odd: the last conv column of the 7x7/2 stem has three padded input columns, not two (49 conv columns pool to 25, 128 to 64)."""
    oracle = oracle_net.seeded_model(77, 5, perturb_bn=True).eval()
    model = _hip_model(oracle, dev)
    host = synth.synth_slide(side, side + 37 if side > P else side, seed=P)
    H, W = host.shape[:2]
    rng = np.random.default_rng(P + 1)
    o = [[0, 0], [H - P, W - P], [0, W - P], [H - P, 0]]
    o += [[int(rng.integers(0, H - P + 1)), int(rng.integers(0, W - P + 1))] for _ in range(17)]
    o = np.array(o, np.int32)
    n = len(o)
    model(torch.zeros(1, 3, P, P, device=dev))                         # finalises the handle
    slide = torch.from_numpy(host).to(dev)
    o_dev = torch.from_numpy(o).to(dev)
    w15 = _stem(model, slide, o_dev, n, P, 15)
    w16 = _stem(model, slide, o_dev, n, P, 16)
    auto = _stem(model, slide, o_dev, n, P, 0)
    assert bool(torch.isfinite(w15).all()) and float(w15.max()) > 0
    assert torch.equal(w16, w15), f"{int((w16 != w15).sum())} elements differ between strips of 16 and of 15 pooled columns"
    assert torch.equal(auto, w15), f"{int((auto != w15).sum())} elements differ between the chosen width and 15"


def test_unknown_strip_width_is_refused(built_lib):
    from deephisto_amd._lib import lib
    assert lib().dh_debug_stem_strip_width(14) != 0
    assert lib().dh_debug_stem_strip_width(0) == 0


def test_seam_scratch_carries_nothing_between_forwards(dev):
    """A stale or uninitialised seam row would show as a dependence on what the handle ran before: two forwards with different slides
    (the second a smaller launch, so rows of the first stay behind it in the scratch) through ONE handle, each against a fresh
    handle that has run nothing else.  Logits of the whole network at P = 256, where the strips are 16 wide: identical bits."""
    from deephisto_amd import tiles
    oracle = oracle_net.seeded_model(31, 5, perturb_bn=True).eval()
    P, side = 256, 2048
    slides = [tiles.synth_slide(side, side, seed, dev) for seed in (3, 4)]
    rng = np.random.default_rng(5)
    origins = [torch.from_numpy(np.stack([rng.integers(0, side - P, n), rng.integers(0, side - P, n)], 1).astype(np.int32)).to(dev)
               for n in (300, 70)]
    used = _hip_model(oracle, dev)
    got = [used.forward_tiles(s, o, P).clone() for s, o in zip(slides, origins)]
    got.append(used.forward_tiles(slides[0], origins[0], P).clone())       # and back again
    for i, (s, o) in enumerate(zip(slides, origins)):
        fresh = _hip_model(oracle, dev)
        want = fresh.forward_tiles(s, o, P)
        assert torch.equal(got[i], want), f"forward {i} of the used handle differs from a fresh handle"
        del fresh
    assert torch.equal(got[2], got[0])
    assert bool(torch.isfinite(got[0]).all()) and float(got[0].abs().max()) > 0
