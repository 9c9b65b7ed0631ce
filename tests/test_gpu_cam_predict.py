"""GPU: predict_fine_patched end to end (deephisto_amd/cam.py) on a 700 x 900 slide, P = 64, stride 32,
d = 16, ResNet-18 bf16 and ResNet-50: the plan's result equals cam_tiles over the sampler's unique tiles plus accumulate_cam over
accumulation_list; filters, probabilities, micro-batches; the CLI's --fine."""
import numpy as np
import pytest
import torch

from deephisto_amd.plan import accumulation_list
from oracle import synth

pytestmark = pytest.mark.gpu

H, W, P, STRIDE, D, B = 700, 900, 64, 32, 16, 16


@pytest.fixture(scope="module", params=["r18", "r50"])
def setup(request, built_lib):
    from deephisto_amd.models.patch_cls_simple.model import get_model
    from deephisto_amd.patch_samplers.full_samplers import FullImageDenseSampler
    dev = torch.device("cuda:0")
    torch.manual_seed(11)
    m = (get_model(5, compute_dtype="bf16") if request.param == "r18" else get_model(5, arch="resnet50")).to(dev).eval()
    host = synth.synth_slide(H, W, 3)
    smp = FullImageDenseSampler(host, layer=1, patch_size=P, batch_size=B, stride=STRIDE, device=dev)
    assert len(smp.origins) > smp.n_tiles, "the batch size leaves padding duplicates of the corner tile"
    unique = torch.from_numpy(smp.origins[:smp.n_tiles]).to(dev)
    cam = m.cam_tiles(smp.data_device, unique, P)     # one launch of all unique tiles
    return dict(dev=dev, m=m, host=host, smp=smp, cam=cam)


@pytest.mark.parametrize("dedupe", [False, True])
def test_fine_prediction_is_cam_tiles_plus_accumulate_cam(setup, dedupe):
    from deephisto_amd import tiles
    from deephisto_amd.cam import predict_fine_patched
    smp, m, cam = setup["smp"], setup["m"], setup["cam"]
    rows, yx = accumulation_list(smp.origins, smp.n_tiles, None, dedupe)
    _, want = tiles.accumulate_cam(cam[torch.from_numpy(rows).to(cam.device)], yx, P, D, H, W)
    got, got_cam = predict_fine_patched(smp, m, 5, downscale=D, dedupe_padding=dedupe, return_cam=True)
    assert got.shape == (H // D, W // D) and got.dtype == torch.int64
    assert torch.equal(got, want)
    assert got_cam.shape == (len(smp.origins), P // 32, P // 32, 5)
    assert torch.equal(got_cam[:smp.n_tiles].view(torch.int32), cam.view(torch.int32))
    assert torch.equal(got_cam[smp.n_tiles:].view(torch.int32), cam[-1:].expand(len(smp.origins) - smp.n_tiles, -1, -1, -1).view(torch.int32))
    # a micro-batch smaller than the tile count changes no bit
    small, small_cam = predict_fine_patched(smp, m, 5, downscale=D, dedupe_padding=dedupe, micro_batch=100, streams=1, return_cam=True)
    assert torch.equal(small, got) and torch.equal(small_cam.view(torch.int32), got_cam.view(torch.int32))


def test_fine_map_has_the_tile_map_s_canvas(setup):
    """Not a parity: the two maps are different functions of the same forward pass.  Both cover the same canvas."""
    from deephisto_amd.cam import predict_fine_patched
    from deephisto_amd.predict import predict_full_patched
    smp, m = setup["smp"], setup["m"]
    fine, coarse = predict_fine_patched(smp, m, 5, downscale=D), predict_full_patched(smp, m, 5, downscale=D)
    assert fine.shape == coarse.shape and fine.dtype == coarse.dtype
    assert int(fine.min()) >= 0 and int(fine.max()) < 5


def test_fine_probabilities(setup):
    from deephisto_amd import tiles
    from deephisto_amd.cam import predict_fine_patched
    smp, m, cam = setup["smp"], setup["m"], setup["cam"]
    cmap, proba = predict_fine_patched(smp, m, 5, downscale=D, return_proba=True)
    assert isinstance(proba, tiles.SlideProbabilities) and proba.finished
    assert proba.class_map.shape == cmap.shape and proba.proba.shape == (*cmap.shape, 5) and proba.count.shape == cmap.shape
    rows, yx = accumulation_list(smp.origins, smp.n_tiles, None, False)
    want = tiles.accumulate_cam_probabilities(cam[torch.from_numpy(rows).to(cam.device)], yx, P, D, H, W)
    for name in ("proba", "count", "class_map", "confidence"):
        assert torch.equal(getattr(proba, name), getattr(want, name)), name
    assert int(proba.count.min()) >= 1
    assert torch.allclose(proba.proba.sum(dim=2), torch.ones_like(proba.confidence), atol=1e-5)


def test_fine_prediction_with_a_tissue_filter(setup):
    from deephisto_amd import tiles
    from deephisto_amd.cam import predict_fine_patched
    from deephisto_amd.patch_samplers.full_samplers import FullImageDenseSampler
    from deephisto_amd.tissue import TissueFilter
    m, dev = setup["m"], setup["dev"]
    host = setup["host"].copy()
    host[:, W // 2:] = 255                       # the right half is glass
    smp = FullImageDenseSampler(host, layer=1, patch_size=P, batch_size=B, stride=STRIDE, device=dev)
    info: dict = {}
    cmap, cam, proba = predict_fine_patched(smp, m, 5, downscale=D, tissue=TissueFilter("otsu", fill_class=3), tissue_info=info,
                                            return_cam=True, return_proba=True)
    kept = info["kept"]
    assert 0 < len(kept) < smp.n_tiles
    rejected = np.setdiff1d(np.arange(smp.n_tiles), kept)
    assert torch.isnan(cam[torch.from_numpy(rejected).to(dev)]).all() and not torch.isnan(cam[torch.from_numpy(kept).to(dev)]).any()
    # the kept tiles alone give the map; cells none of them covers carry the fill class
    unique = torch.from_numpy(smp.origins[:smp.n_tiles][kept]).to(dev)
    rows = m.cam_tiles(smp.data_device, unique, P)
    assert torch.equal(rows.view(torch.int32), cam[torch.from_numpy(kept).to(dev)].view(torch.int32))
    covered, _ = tiles.accumulate_logits(torch.ones((len(kept), 1), device=dev), smp.origins[:smp.n_tiles][kept], P, D, H, W,
                                         want_map=False)
    uncovered = covered[..., 0] == 0
    assert bool(uncovered.any()) and bool((cmap[uncovered] == 3).all())
    assert bool((proba.count[uncovered] == 0).all()) and bool((proba.class_map[uncovered] == 3).all())
    rows_l, yx = accumulation_list(smp.origins, smp.n_tiles, kept, False)
    _, want = tiles.accumulate_cam(rows[torch.from_numpy(rows_l).to(dev)], yx, P, D, H, W)
    assert torch.equal(cmap[~uncovered], want[~uncovered])


def test_cli_fine(built_lib, tmp_path):
    from deephisto_amd.examples.predict_full_patched import main
    from deephisto_amd.models.patch_cls_simple.model import get_model
    torch.manual_seed(11)
    m = get_model(5, compute_dtype="bf16").to(torch.device("cuda:0")).eval()
    base = ["--synthetic", str(H), str(W), "--weights", "", "--patch_size", str(P), "--stride", str(STRIDE), "--batch_size", str(B)]
    plain = main([*base, "--out_dir", str(tmp_path / "plain")], model=m)
    fine = main([*base, "--fine", "--out_dir", str(tmp_path / "fine")], model=m)
    assert fine.shape == plain.shape
    names = lambda d: sorted(p.name for p in (tmp_path / d).iterdir())   # noqa: E731
    assert names("fine") == names("plain") and len(names("fine")) == 3
    main([*base, "--fine", "--proba", "--heat", "TUM", "--out_dir", str(tmp_path / "heat")], model=m)
    assert any("confidence" in n for n in names("heat")) and len(names("heat")) > 3
    main([*base, "--fine", "--regions_json", str(tmp_path / "regions.json"), "--out_dir", str(tmp_path / "reg")], model=m)
    assert (tmp_path / "regions.json").stat().st_size > 0
