"""GPU: test-time augmentation of whole-slide prediction over dihedral views.

The reference of every test is the stated float32 fold  acc = L[0]; acc += L[k]; acc *= float32(1 / V)  in NumPy over
`model.forward_tiles(view_np(slide), map_origins(origins), P)` per view, the views built by NumPy, never by the kernel under
test.  Launch size and a tile's place in a launch do not change its logits in this project, so equality is bit for bit."""
import numpy as np
import pytest
import torch

from oracle import synth

pytestmark = pytest.mark.gpu

H, W, P, S, B, D, NCLS = 600, 700, 256, 256, 4, 16, 5
CONFIGS = [("resnet18", "f32"), ("resnet18", "bf16"), ("resnet50", "bf16")]
VIEWS = ("r0", "r90", "r180", "r270", "r0f", "r90f", "r180f", "r270f")


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def view_np(a, v):
    return np.rot90(np.fliplr(a) if v >> 2 else a, v & 3).copy()      # a fresh C-ordered array


_MODELS: dict = {}


def _model(arch, dtype, dev):
    from deephisto_amd.models.patch_cls_simple.model import get_model
    if (arch, dtype) not in _MODELS:
        torch.manual_seed(0)
        _MODELS[arch, dtype] = get_model(NCLS, dtype, arch=arch).to(dev).eval()
    return _MODELS[arch, dtype]


def _sampler(host, dev, patch=P, stride=S, batch=B):
    from deephisto_amd.patch_samplers.full_samplers import FullImageDenseSampler
    return FullImageDenseSampler(host, layer=1, patch_size=patch, batch_size=batch, stride=stride, device=dev)


def _host(kind="plain"):
    host = synth.synth_slide(H, W, 3)
    if kind == "glass":
        host[:, W // 2:] = 255           # half constant glass
    return host


_PER_VIEW: dict = {}


def per_view_logits(key, model, host, origins, patch, dev):
    """float32[8][n, n_cls] (NumPy, read-only): the plain forward of every view of `host`, built by NumPy, over the mapped
    origins.  Computed once per `key` and shared."""
    from deephisto_amd import tta
    if key not in _PER_VIEW:
        out = []
        for v in range(8):
            slide = torch.from_numpy(view_np(host, v)).to(dev)
            mapped = torch.from_numpy(tta.map_origins(origins, host.shape[0], host.shape[1], patch, v)).to(dev)
            out.append(model.forward_tiles(slide, mapped, patch).cpu().numpy())
            out[-1].setflags(write=False)
        _PER_VIEW[key] = out
    return _PER_VIEW[key]


def fold_np(per_view, names):
    """The contract, restated: float32, in the order of `names`."""
    L = [per_view[VIEWS.index(name)] for name in names]
    acc = L[0].copy()
    for x in L[1:]:
        acc += x
    acc *= np.float32(1 / len(L))
    assert acc.dtype == np.float32
    return acc


@pytest.mark.parametrize("arch,dtype", CONFIGS)
def test_identity_view_changes_no_bit(dev, arch, dtype):
    from deephisto_amd.predict import predict_full_patched
    from deephisto_amd.tta import TestTimeAugmenter
    model, smp = _model(arch, dtype, dev), _sampler(_host(), dev)
    assert len(smp.origins) > smp.n_tiles           # the corner's padding duplicates are in play
    cmap0, logits0 = predict_full_patched(smp, model, NCLS, downscale=D, return_logits=True, tta=None)
    info: dict = {}
    cmap1, logits1 = predict_full_patched(smp, model, NCLS, downscale=D, return_logits=True, tta=TestTimeAugmenter(["r0"]), tta_info=info)
    assert torch.equal(cmap1, cmap0) and torch.equal(logits1, logits0)
    assert info == {"views": ["r0"], "n_forward_tiles": smp.n_tiles}


@pytest.mark.parametrize("arch,dtype", CONFIGS)
def test_d4_equals_the_fold_over_per_view_forwards(dev, arch, dtype):
    from deephisto_amd import tiles
    from deephisto_amd.predict import predict_full_patched
    from deephisto_amd.tta import TestTimeAugmenter
    host = _host()
    model, smp = _model(arch, dtype, dev), _sampler(host, dev)
    assert (smp.h, smp.w) == (H, W) and smp.n_tiles == 9 and len(smp.origins) == 12
    per_view = per_view_logits((arch, dtype, "plain"), model, host, smp.origins, P, dev)
    assert any(not np.array_equal(per_view[0], x) for x in per_view[1:])       # the network is not invariant: the views matter
    for names, kw in ((VIEWS, {}), (VIEWS, dict(micro_batch=4, streams=2)), (VIEWS, dict(micro_batch=2, streams=3)),
                      (("r270f", "r90", "r0", "r180f"), {}), ("flips", {}), ("rot", dict(dedupe_padding=True))):
        aug = TestTimeAugmenter(names)
        want = fold_np(per_view, aug.views)
        info: dict = {}
        cmap, logits = predict_full_patched(smp, model, NCLS, downscale=D, return_logits=True, tta=aug, tta_info=info, **kw)
        assert logits.dtype == torch.float32 and tuple(logits.shape) == (12, NCLS)
        assert np.array_equal(logits.cpu().numpy(), want), (names, kw)
        n_acc = 9 if kw.get("dedupe_padding") else 12
        _, want_map = tiles.accumulate_logits(torch.from_numpy(want[:n_acc]).to(dev), smp.origins[:n_acc], P, D, H, W)
        assert torch.equal(cmap, want_map)
        assert info == {"views": list(aug.views), "n_forward_tiles": 9 * len(aug)}
    # a set of views by name is taken as the augmenter of that name
    assert torch.equal(predict_full_patched(smp, model, NCLS, downscale=D, tta="d4"), predict_full_patched(smp, model, NCLS, downscale=D, tta=TestTimeAugmenter()))
    assert torch.equal(smp.data_device.cpu(), torch.from_numpy(host))          # the resident slide is left alone


def test_tissue_filter_keeps_its_list(dev):
    from deephisto_amd.predict import predict_full_patched
    from deephisto_amd.tissue import TissueFilter
    host = _host("glass")
    model, smp = _model("resnet18", "bf16", dev), _sampler(host, dev)
    per_view = per_view_logits(("resnet18", "bf16", "glass"), model, host, smp.origins, P, dev)
    plain: dict = {}
    predict_full_patched(smp, model, NCLS, downscale=D, tissue=TissueFilter("otsu"), tissue_info=plain)
    info, tinfo = {}, {}
    cmap, logits = predict_full_patched(smp, model, NCLS, downscale=D, return_logits=True, tissue=TissueFilter("otsu"), tissue_info=info,
                                        tta="d4", tta_info=tinfo)
    kept = info["kept"]
    assert np.array_equal(kept, plain["kept"]) and info["threshold"] == plain["threshold"] and 0 < len(kept) < smp.n_tiles
    assert tinfo["n_forward_tiles"] == 8 * len(kept)
    lg = logits.cpu().numpy()
    want = fold_np(per_view, VIEWS)
    rejected = np.setdiff1d(np.arange(smp.n_tiles), kept)
    assert np.array_equal(lg[kept], want[kept]) and np.isnan(lg[rejected]).all()
    # the map is the plain filtered run's finish over the combined rows: cells no kept tile covers hold the fill class
    cover = np.zeros((H // D, W // D), bool)
    for y, x in smp.origins[:smp.n_tiles][kept]:
        cover[y // D:(y + P) // D, x // D:(x + P) // D] = True
    assert np.array_equal(cmap.cpu().numpy() == -1, ~cover)
    assert kept[-1] != smp.n_tiles - 1            # the corner tile is glass: no padding duplicates follow
    from deephisto_amd import tiles
    _, covered = tiles.accumulate_logits(torch.from_numpy(want[kept]).to(dev), smp.origins[kept], P, D, H, W)
    assert np.array_equal(cmap.cpu().numpy()[cover], covered.cpu().numpy()[cover])


def test_probabilities_are_the_softmax_of_the_mean_logits(dev):
    from deephisto_amd import tiles
    from deephisto_amd.predict import predict_full_patched
    host = _host()
    model, smp = _model("resnet18", "bf16", dev), _sampler(host, dev)
    want = fold_np(per_view_logits(("resnet18", "bf16", "plain"), model, host, smp.origins, P, dev), VIEWS)
    cmap, logits, proba = predict_full_patched(smp, model, NCLS, downscale=D, return_logits=True, return_proba=True, tta="d4")
    assert np.array_equal(logits.cpu().numpy(), want)
    ref = tiles.accumulate_probabilities(torch.from_numpy(want).to(dev), smp.origins, P, D, H, W)
    for name in ("proba", "count", "class_map", "confidence"):
        assert torch.equal(getattr(proba, name), getattr(ref, name)), name


def test_stain_composes(dev):
    """`stain=` swaps the normalised slide in before the function runs: the views are those of the normalised slide."""
    from deephisto_amd.predict import predict_full_patched
    from deephisto_amd.stain import StainNormalizer
    host = _host()
    model, smp = _model("resnet18", "bf16", dev), _sampler(host, dev)
    norm = StainNormalizer("macenko")
    got = predict_full_patched(smp, model, NCLS, downscale=D, return_logits=True, stain=norm, tta="flips")
    want = predict_full_patched(_sampler(norm.normalize(smp.data_device).cpu().numpy(), dev), model, NCLS, downscale=D, return_logits=True,
                                tta="flips")
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert torch.equal(smp.data_device.cpu(), torch.from_numpy(host))


def test_equivariance_under_a_quarter_turn(dev):
    """768 x 768, patch and stride 256: a 3 x 3 grid that a quarter turn maps onto itself.  The d4 logits of a tile of the turned
    slide are the mean of the same eight per-view logits x_k as those of its preimage tile, summed in another order.  A float32
    sum of V terms in any order is within (V - 1) 2^-24 sum |x_k| of the exact sum (first order), two orders within twice that,
    and the scaling by 1/8 is exact, so the means differ by at most 2 (V - 1) 2^-24 sum |x_k| / 8 per element: derived, not
    tuned (and tighter than the bound on the sums)."""
    from deephisto_amd import tta
    from deephisto_amd.predict import predict_full_patched
    n, patch = 768, 256
    host = synth.synth_slide(n, n, 5)
    turned = view_np(host, 1)
    model = _model("resnet18", "bf16", dev)
    a, b = _sampler(host, dev, patch, patch), _sampler(turned, dev, patch, patch)
    assert a.n_tiles == 9 == b.n_tiles and np.array_equal(a.origins, b.origins)
    x = np.stack(per_view_logits(("resnet18", "bf16", "square"), model, host, a.origins[:9], patch, dev))     # [8, 9, n_cls]
    _, la = predict_full_patched(a, model, NCLS, downscale=D, return_logits=True, tta="d4")
    _, lb = predict_full_patched(b, model, NCLS, downscale=D, return_logits=True, tta="d4")
    la, lb = la.cpu().numpy()[:9], lb.cpu().numpy()[:9]
    assert np.array_equal(la, fold_np(list(x), VIEWS))
    mapped = tta.map_origins(a.origins[:9], n, n, patch, "r90")
    where = {tuple(o): j for j, o in enumerate(b.origins[:9].tolist())}
    perm = np.array([where[tuple(o)] for o in mapped.tolist()])
    assert sorted(perm) == list(range(9)) and (perm != np.arange(9)).sum() == 8        # only the centre tile stays
    bound = 2 * (8 - 1) * 2.0 ** -24 * np.abs(x.astype(np.float64)).sum(axis=0) / 8
    diff = np.abs(la.astype(np.float64) - lb[perm].astype(np.float64))
    print(f"equivariance: max diff {diff.max():.3e}, min bound {bound.min():.3e}, max diff / bound {(diff / bound).max():.3f}")
    assert (diff <= bound).all()
    # the per-view logits of the turned slide are those of the original, renamed: view u of the turned slide is view
    # compose(r90, u) of the original
    y = per_view_logits(("resnet18", "bf16", "square-turned"), model, turned, b.origins[:9], patch, dev)
    for u in range(8):
        assert np.array_equal(y[u][perm], x[tta.compose(1, u)]), u


def _rnd_sampler(slide, patch, batch, dev):
    from deephisto_amd.patch_samplers.full_samplers import FullImageRndSampler
    return FullImageRndSampler(slide, layer=1, patch_size=patch, batch_size=batch, dense_level=1, speedup=D, device=dev, index_logic="device")


def test_predict_random_patched(dev):
    from deephisto_amd import tiles
    from deephisto_amd.predict import predict_random_patched
    from deephisto_amd.tta import TestTimeAugmenter
    patch, batch = 128, 8
    host = _host()
    slide = torch.from_numpy(host).to(dev)
    model = _model("resnet18", "bf16", dev)
    np.random.seed(17)
    origins = np.concatenate([np.array([(p.pos_y, p.pos_x) for p in patches], np.int32)
                              for patches, _ in _rnd_sampler(slide, patch, batch, dev).generator()])
    assert len(origins) % batch == 0 and len(origins) > 3 * batch
    per_view = per_view_logits(("resnet18", "bf16", "random"), model, host, origins, patch, dev)
    for tta_arg, names, mb in (("flips", TestTimeAugmenter("flips").views, None), (TestTimeAugmenter(["r90f", "r0"]), ("r90f", "r0"), 16),
                               (None, ("r0",), None)):
        want = torch.from_numpy(fold_np(per_view, names)).to(dev)
        want_canvas, want_map = tiles.accumulate_logits(want, origins, patch, D, H, W)
        np.random.seed(17)
        cmap, canvas = predict_random_patched(_rnd_sampler(slide, patch, batch, dev), model, NCLS, D, micro_batch=mb, return_canvas=True,
                                              tta=tta_arg)
        assert torch.equal(canvas, want_canvas) and torch.equal(cmap, want_map), names
    assert torch.equal(slide.cpu(), torch.from_numpy(host))


def test_streamed_sampler_is_refused(dev, tmp_path):
    from deephisto_amd.patch_samplers.full_samplers import FullImageDenseSampler, SamplerExecutionMode
    from deephisto_amd.predict import predict_full_patched
    path = tmp_path / "slide.npy"
    np.save(path, _host())
    disk = FullImageDenseSampler(path, layer=1, patch_size=P, batch_size=B, stride=S, device=dev, mode=SamplerExecutionMode.ONDISK_MULTIPROC)
    with pytest.raises(ValueError, match=r"test-time augmentation needs an HBM-resident slide \(ONDISK_MULTIPROC streams it\)"):
        predict_full_patched(disk, _model("resnet18", "bf16", dev), NCLS, tta="d4")
    with pytest.raises(ValueError, match="unknown view set"):
        predict_full_patched(_sampler(_host(), dev), _model("resnet18", "bf16", dev), NCLS, tta="all")


def test_cli_tta(dev, tmp_path):
    """`--tta flips` on both fused routes equals the in-process calls."""
    from deephisto_amd import tiles
    from deephisto_amd.examples.predict_full_patched import main, predict_full_patched, predict_random_patched
    model = _model("resnet18", "bf16", dev)
    argv = ["--synthetic", str(H), str(W), "--weights", "", "--patch_size", str(P), "--stride", str(S), "--batch_size", str(B),
            "--no_visualizations", "--out_dir", str(tmp_path / "out"), "--tta", "flips"]
    slide = tiles.synth_slide(H, W, 0, dev)
    pred = main(argv, model=model)
    assert torch.equal(pred, predict_full_patched(_sampler(slide, dev), model, NCLS, downscale=D, tta="flips"))
    np.random.seed(5)
    pred = main(argv + ["--random_sampler"], model=model)
    from deephisto_amd.patch_samplers.full_samplers import FullImageRndSampler
    np.random.seed(5)
    smp = FullImageRndSampler(slide, layer=2, patch_size=P, batch_size=B, device=dev)
    np.testing.assert_array_equal(pred, predict_random_patched(smp, model, NCLS, downscale=D, tta="flips").cpu().numpy())
