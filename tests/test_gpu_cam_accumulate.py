"""GPU: the fine accumulations (dh_accumulate_cam / dh_accumulate_cam_mean) against their definition -- the
existing ordered accumulations over the expanded list with patch 32 -- and against tests/helpers/cam_ref.py, bit for bit.  The rows
are random: no network runs.  Origins: the four corners, unaligned ones, exact duplicates, and one origin 300 times over (more than
one 256-entry chunk of a bin's tile list)."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import cam_ref  # noqa: E402

pytestmark = pytest.mark.gpu


def _bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.fixture(scope="module", params=[(P, d) for P in (32, 64, 224) for d in (1, 7, 16, 32, 48, 100)], ids=lambda c: f"P{c[0]}-d{c[1]}")
def geom(request):
    P, d = request.param
    h, w = P + 283, P + 391
    rng = np.random.default_rng(100 * P + d)
    o = [(0, 0), (0, w - P), (h - P, 0), (h - P, w - P), (3, 5), (33, 70), (33, 70), (h - P - 1, 17), (0, 0)]
    o += [(int(rng.integers(0, h - P + 1)), int(rng.integers(0, w - P + 1))) for _ in range(6)]
    o += [(41, 59)] * 300
    return P, d, h, w, np.asarray(o, np.int32)


@pytest.mark.parametrize("K", [1, 5, 64])
def test_accumulate_cam_is_accumulate_logits_over_the_expanded_list(built_lib, geom, K):
    from deephisto_amd import tiles
    P, d, h, w, o = geom
    dev = torch.device("cuda:0")
    S = P // 32
    rng = np.random.default_rng(K)
    cam_h = rng.standard_normal((len(o), S, S, K)).astype(np.float32)
    base_h = rng.standard_normal((h // d, w // d, K)).astype(np.float32)
    cam = torch.from_numpy(cam_h).to(dev)
    expanded = tiles.expand_positions(o, P)
    rows = cam.view(-1, K)
    for base in (None, base_h):
        start = (lambda: None) if base is None else (lambda: torch.from_numpy(base).to(dev))
        got_c, got_m = tiles.accumulate_cam(cam, o, P, d, h, w, canvas=start())
        exp_c, exp_m = tiles.accumulate_logits(rows, expanded, 32, d, h, w, canvas=start())
        ref_c = cam_ref.accumulate(h, w, d, P, o, cam_h, canvas=base)
        assert got_c.shape == (h // d, w // d, K)
        assert np.array_equal(_bits(got_c), _bits(exp_c)), "differs from accumulate_logits over the expanded list"
        assert np.array_equal(_bits(got_c), _bits(ref_c)), "differs from the NumPy loop over the expanded list"
        assert np.array_equal(got_m.cpu().numpy(), exp_m.cpu().numpy())
        assert np.array_equal(got_m.cpu().numpy(), np.argmax(ref_c, axis=2))
    no_map = tiles.accumulate_cam(cam, o, P, d, h, w, want_map=False)
    assert no_map[1] is None and np.array_equal(_bits(no_map[0]), _bits(cam_ref.accumulate(h, w, d, P, o, cam_h)))


@pytest.mark.parametrize("K", [1, 5, 64])
def test_accumulate_cam_probabilities_is_accumulate_probabilities_over_the_expanded_list(built_lib, geom, K):
    from deephisto_amd import tiles
    P, d, h, w, o = geom
    dev = torch.device("cuda:0")
    S = P // 32
    cam = torch.from_numpy(np.random.default_rng(7 + K).standard_normal((len(o), S, S, K)).astype(np.float32) * 3).to(dev)
    fill = K - 1
    got = tiles.accumulate_cam_probabilities(cam, o, P, d, h, w, fill_class=fill)
    exp = tiles.accumulate_probabilities(cam.view(-1, K), tiles.expand_positions(o, P), 32, d, h, w, fill_class=fill)
    assert got.finished and got.fill_class == fill
    for name in ("proba", "count", "class_map", "confidence"):
        assert np.array_equal(_bits(getattr(got, name)), _bits(getattr(exp, name))), name
    ref = cam_ref.mean(h, w, d, P, o, tiles.softmax_rows(cam.view(-1, K)).cpu().numpy(), fill=fill)
    for name in ("proba", "count", "class_map", "confidence"):
        assert np.array_equal(_bits(getattr(got, name)), _bits(ref[name])), f"{name} differs from the NumPy rules"
    count = got.count.cpu().numpy()
    assert d > 16 or (count == 0).any(), "at fine cells the corner tiles leave a cross of the canvas uncovered"
    assert np.all(got.class_map.cpu().numpy()[count == 0] == fill) and np.all(got.proba.cpu().numpy()[count == 0] == 0)
    assert d > 32 or count.max() >= 300, "the repeated origin fills more than one chunk of its bin's tile list"
