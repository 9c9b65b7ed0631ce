"""GPU: `--save_embeddings` and `--prototypes` through the CLI of examples/predict_full_patched.py, in process, on a --synthetic slide."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ARGS = ["--synthetic", "700", "900", "--layer", "1", "--weights", "", "--patch_size", "96", "--stride", "64", "--batch_size", "16",
        "--compute_dtype", "bf16"]
STEM = "synthetic_700x900"


def test_save_embeddings_leaves_the_class_map_jpeg_byte_identical(built_lib, tmp_path):
    from deephisto_amd.embeddings import SlideEmbeddings
    from deephisto_amd.examples.predict_full_patched import main
    assert torch.cuda.is_available()
    plain = main(ARGS + ["--out_dir", str(tmp_path / "plain")])
    path = tmp_path / "out" / "emb.npz"
    with_emb = main(ARGS + ["--out_dir", str(tmp_path / "emb"), "--save_embeddings", str(path)])
    assert torch.equal(torch.as_tensor(plain), torch.as_tensor(with_emb))
    for name in (f"{STEM}_mask.jpg", f"{STEM}_overlay.jpg", f"{STEM}.jpg"):
        assert (tmp_path / "plain" / name).read_bytes() == (tmp_path / "emb" / name).read_bytes(), name
    emb = SlideEmbeddings.load(path)
    assert emb.features.shape == (154, 512) and emb.logits.shape == (154, 5) and emb.n_padded == 160
    assert (emb.patch_size, emb.stride, emb.h, emb.w, emb.arch, emb.compute_dtype) == (96, 64, 700, 900, "resnet18", "bf16")
    assert torch.isfinite(emb.features).all() and float(emb.features.min()) >= 0
    back = SlideEmbeddings.load(path, device="cuda:0").class_map(16)
    assert torch.equal(back, torch.as_tensor(plain).to(back.device))


def test_prototypes_fit_with_anno_then_map_without(built_lib, tmp_path):
    from deephisto_amd.embeddings import PrototypeClassifier
    from deephisto_amd.examples.predict_full_patched import main
    from deephisto_amd.scoring import synthetic_annotation
    from deephisto_amd.visualize import KNOWN_COLORS
    anno = tmp_path / "anno.json"
    anno.write_text(json.dumps(synthetic_annotation(700, 900, 2, 24, list(KNOWN_COLORS), seed=36)))
    protos = tmp_path / "protos.npz"
    main(ARGS + ["--out_dir", str(tmp_path / "fit"), "--no_visualizations", "--anno", str(anno), "--prototypes", str(protos)])
    pc = PrototypeClassifier.load(protos)
    assert pc.prototypes.shape == (5, 512) and pc.counts.tolist() == [0, 4, 4, 0, 0] and pc.empty_classes == [0, 3, 4]
    assert np.allclose(pc.prototypes[[1, 2]].square().sum(1).numpy(), 1.0, atol=1e-5) and not pc.prototypes[[0, 3, 4]].any()
    main(ARGS + ["--out_dir", str(tmp_path / "map"), "--prototypes", str(protos)])
    jpg = tmp_path / "map" / f"{STEM}_prototype_map.jpg"
    assert jpg.is_file() and jpg.stat().st_size > 1000
