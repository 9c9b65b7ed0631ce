"""GPU: extract_embeddings, SlideEmbeddings.class_map and the prototype scorer on real features.

Slide: 700 x 900 synthetic with a band of glass; P = 96, stride 64 (154 unique tiles, 6 padding duplicates at batch 16); ResNet-18 in
bf16 and ResNet-50."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import resnet18 as o18
from oracle import resnet50 as o50
from oracle import synth

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import embed_ref as er  # noqa: E402

pytestmark = pytest.mark.gpu

H, W, P, S, B, DOWN = 700, 900, 96, 64, 16, 16
ANNO_SEED = 36   # as tests/test_embeddings_host.py: four tile centres of class 2 on tissue or glass, four of class 1 on the other


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def slide_host():
    host = synth.synth_slide(H, W, 17).copy()
    host[:, 380:560] = 255     # a band of glass, wider than a tile
    return host


@pytest.fixture(scope="module", params=["r18", "r50"])
def setup(request, dev, slide_host):
    from deephisto_amd.models.patch_cls_simple.model import get_model
    from deephisto_amd.patch_samplers.full_samplers import FullImageDenseSampler
    if request.param == "r18":
        ref, m = o18.seeded_model(321, 5, perturb_bn=True), get_model(5, compute_dtype="bf16")
    else:
        ref, m = o50.seeded_model(5, 5, perturb_bn=True), get_model(5, arch="resnet50")
        with torch.no_grad():   # as tests/test_gpu_layer_parity.py: without it the 16 residual joins swamp the features with one direction
            for name, mod in ref.named_modules():
                if name.endswith("bn3"):
                    mod.weight.mul_(0.2)
    m.load_state_dict(ref.state_dict())
    m = m.to(dev).eval()
    smp = FullImageDenseSampler(slide_host, layer=1, patch_size=P, batch_size=B, stride=S, device=dev)
    assert smp.n_tiles == 154 and len(smp.origins) == 160
    return m, smp


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_one_launch_and_hand_made_launches(setup, dev):
    from deephisto_amd.embeddings import extract_embeddings
    from deephisto_amd.predict import launch_size
    m, smp = setup
    n = smp.n_tiles
    o_dev = torch.from_numpy(smp.origins[:n]).to(dev)
    emb = extract_embeddings(smp, m, micro_batch=256, return_logits=True)
    feat, logits = m.features_tiles(smp.data_device, o_dev, P, return_logits=True)
    assert _same(emb.features, feat) and _same(emb.logits, logits)
    assert np.array_equal(emb.origins, smp.origins[:n]) and np.array_equal(emb.tile_index, np.arange(n))
    assert (emb.patch_size, emb.stride, emb.h, emb.w, emb.layer, emb.n_unique, emb.n_padded) == (P, S, H, W, 1, 154, 160)
    assert emb.width == m.feature_width and emb.compute_dtype == "bf16" and emb.row_range is None
    mb = launch_size(n, 40)
    assert mb == 39
    by_hand = torch.cat([m.features_tiles(smp.data_device, o_dev[s:s + mb], P) for s in range(0, n, mb)])
    small = extract_embeddings(smp, m, micro_batch=40)
    assert small.logits is None and _same(small.features, by_hand)
    alone = extract_embeddings(smp, m, micro_batch=40, gather=False)     # one process: its own rows are all rows
    assert _same(alone.features, by_hand) and alone.row_range is None


def test_kept_list_and_class_map_follow_predict_full_patched(setup, dev, tmp_path):
    from deephisto_amd.embeddings import SlideEmbeddings, extract_embeddings
    from deephisto_amd.predict import predict_full_patched
    from deephisto_amd.tissue import TissueFilter
    m, smp = setup
    # plain, with and without the corner's padding duplicates
    emb = extract_embeddings(smp, m, return_logits=True)
    for dedupe in (False, True):
        want = predict_full_patched(smp, m, 5, downscale=DOWN, dedupe_padding=dedupe)
        assert torch.equal(emb.class_map(DOWN, dedupe_padding=dedupe), want), f"plain, dedupe_padding={dedupe}"
    # filtered
    filt = TissueFilter("otsu", fill_class=3)
    info, einfo = {}, {}
    want = predict_full_patched(smp, m, 5, downscale=DOWN, tissue=filt, tissue_info=info)
    femb = extract_embeddings(smp, m, tissue=filt, tissue_info=einfo, return_logits=True)
    assert 0 < info["n_kept"] < smp.n_tiles, "the band of glass must cost tiles"
    assert np.array_equal(femb.tile_index, info["kept"]) and np.array_equal(einfo["kept"], info["kept"])
    assert np.array_equal(femb.origins, smp.origins[:smp.n_tiles][info["kept"]])
    assert torch.equal(femb.class_map(DOWN, fill_class=3), want)
    assert (want == 3).any()
    want_d = predict_full_patched(smp, m, 5, downscale=DOWN, tissue=filt, dedupe_padding=True)
    assert torch.equal(femb.class_map(DOWN, dedupe_padding=True, fill_class=3), want_d)
    # the kept rows are the plain run's rows of those tiles
    assert _same(femb.features, emb.features[torch.from_numpy(info["kept"]).to(dev)])
    # and the file gives the same map back
    femb.save(tmp_path / "emb.npz")
    back = SlideEmbeddings.load(tmp_path / "emb.npz", device=dev)
    assert _same(back.features, femb.features) and torch.equal(back.class_map(DOWN, fill_class=3), want)


def test_both_filters_at_once_follow_predict_full_patched(setup, dev):
    """The tissue stage and the quality stage together: both routes compose the same lists and finish the same map."""
    from deephisto_amd.embeddings import extract_embeddings
    from deephisto_amd.predict import predict_full_patched
    from deephisto_amd.quality import QualityFilter, sharpness_summary
    from deephisto_amd.tissue import TissueFilter
    m, smp = setup
    tissue, first = TissueFilter("otsu", fill_class=3), {}
    extract_embeddings(smp, m, tissue=tissue, quality=QualityFilter(fill_class=3), quality_info=first)
    q = sharpness_summary(first["stats"])
    min_sharpness = int((q["q1"] + q["q3"]) / 2)
    assert q["q1"] < min_sharpness < q["q3"], q
    quality = QualityFilter(min_sharpness=min_sharpness, fill_class=3)
    tinfo, qinfo, etinfo, eqinfo = {}, {}, {}, {}
    emb = extract_embeddings(smp, m, tissue=tissue, tissue_info=etinfo, quality=quality, quality_info=eqinfo, return_logits=True)
    for dedupe in (False, True):
        want = predict_full_patched(smp, m, 5, downscale=DOWN, dedupe_padding=dedupe, tissue=tissue, tissue_info=tinfo,
                                    quality=quality, quality_info=qinfo)
        assert np.array_equal(eqinfo["kept"], qinfo["kept"]) and np.array_equal(etinfo["kept"], tinfo["kept"])
        assert 0 < len(qinfo["kept"]) < len(tinfo["kept"]) < smp.n_tiles
        assert qinfo["n_kept"] == len(qinfo["kept"]) and tinfo["n_kept"] == len(tinfo["kept"])
        assert torch.equal(emb.class_map(DOWN, dedupe_padding=dedupe, fill_class=3), want), f"dedupe_padding={dedupe}"
    assert np.array_equal(emb.tile_index, qinfo["kept"])


def test_prototype_map_on_real_features(setup, dev):
    """Labels: the two-region synthetic annotation of ANNO_SEED.  predict_map must equal the float64 NumPy pipeline on every cell whose
    float64 top-two accumulated scores differ by more than the scores' bound ((D + 2) u sum |f| |p|) summed over the cell's tiles; the
    other cells may differ and must number at most 1 % of the cells (24 of 2 408).  One region of the annotation lies on the band of
    glass, the other on tissue.  The count of undecided cells is a property of the float64 reference on these inputs, not of the
    kernels: on the CPU, with stand-in features, it is 0 at D = 512 and at D = 2048 (tests/test_embeddings_host.py); measured on one
    MI355X with the real features it is 0 for both models, and no cell differs from the float64 map.  (A ResNet-50 without the
    bn3 x 0.2 of the parity tests has nearly parallel features for glass and tissue: 60 undecided cells, none different.)"""
    from deephisto_amd.anno.utils import AnnoDescription
    from deephisto_amd.embeddings import PrototypeClassifier, extract_embeddings, tile_labels
    from deephisto_amd.scoring import annotation_rings, rasterize_annotation, synthetic_annotation
    from deephisto_amd.visualize import KNOWN_COLORS
    m, smp = setup
    dsc = AnnoDescription.with_known_colors(KNOWN_COLORS)
    records = synthetic_annotation(H, W, 2, 24, list(KNOWN_COLORS), seed=ANNO_SEED)
    truth, _ = rasterize_annotation(records, dsc, 1, H, W, DOWN, device=dev)
    emb = extract_embeddings(smp, m)
    lab = tile_labels(emb, truth, DOWN)
    xy, start, cls, _ = annotation_rings(records, dsc, 1, H, W)
    assert np.array_equal(lab, er.tile_labels_ref(xy, start, cls, emb.origins, P, DOWN, H, W))
    assert np.bincount(lab[lab >= 0], minlength=5).tolist() == [0, 4, 4, 0, 0]
    pc = PrototypeClassifier(5).fit(emb, lab)
    assert pc.empty_classes == [0, 3, 4]
    got = pc.predict_map(emb, DOWN).cpu().numpy()
    want, decided = er.prototype_map_ref(emb.features.cpu().numpy(), lab, 5, emb.origins, P, DOWN, H, W)
    undecided = int((~decided).sum())
    differ = int((got != want).sum())
    print(f"\nD = {emb.width}: {undecided} undecided cells of {want.size}, {differ} cells differ from the float64 map")
    assert np.array_equal(got[decided], want[decided])
    assert undecided <= 0.01 * want.size
    assert (want >= 0).all() and set(np.unique(got)) <= {1, 2}
    # the similarity field of the class-1 tiles: a [0, 1] map on the canvas, highest on those tiles' own cells
    sim = pc.similarity(emb, np.nonzero(lab == 1)[0], DOWN)
    assert sim.shape == (H // DOWN, W // DOWN) and sim.dtype == torch.float32
    assert float(sim.min()) >= 0 and float(sim.max()) <= 1 and float(sim.max()) > 0.5
