"""GPU: the ResNet-50 inference engine (dh_resnet50_*: eval BN folded, one pass per convolution, channel-blocked bf16 activations)
and whole-slide prediction with a ResNet-50 (predict_full_patched, predict_random_patched, the CLI).

Tolerance: the SURVEY's bf16 gate, max|d| <= 2e-2 * max(1, |logit|_inf), against the float32 CPU oracle (oracle/resnet50.py) with
perturbed running statistics (the folding is exercised) and bn3 weights x 0.2 (as test_gpu_train_bf16._pair: keeps the 16-block
residual chain at a realistic scale)."""
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import resnet50 as o50
from oracle import synth, tiling

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parents[1]
GATE = 2e-2


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _oracle(seed=5):
    ref = o50.seeded_model(seed, 5, perturb_bn=True)
    with torch.no_grad():
        for name, mod in ref.named_modules():
            if name.endswith("bn3"):
                mod.weight.mul_(0.2)
    return ref.eval()


def _model(ref, dev):
    from deephisto_amd.models.patch_cls_simple.model import get_model
    m = get_model(5, arch="resnet50")
    m.load_state_dict(ref.state_dict())
    return m.to(dev).eval()


def _origins(h, w, P, n, seed):
    """Arbitrary, non-grid origins, the four corners (border-touching) first."""
    rng = np.random.default_rng(seed)
    o = [(0, 0), (0, w - P), (h - P, 0), (h - P, w - P)]
    o += [(int(rng.integers(0, h - P + 1)), int(rng.integers(0, w - P + 1))) for _ in range(n - 4)]
    return np.asarray(o, np.int32)


def _oracle_logits(ref, host, o, P):
    with torch.no_grad():
        return ref(torch.from_numpy(tiling.features_nchw_predictor(host, o, P))).numpy()


def _gate(got, want, what):
    scale = max(1.0, float(np.abs(want).max()))
    err = float(np.abs(got - want).max())
    assert err <= GATE * scale, f"{what}: logit error {err} at scale {scale}"
    return err


@pytest.mark.parametrize("P", [224, 256, 96])
def test_forward_tiles_matches_oracle_and_eval_route(dev, P):
    """(1) forward_tiles vs the float32 oracle, (2) vs ResNet50HIP.eval() on the gathered tiles (training engine), (3) the float NCHW
    entry on the gathered tiles equals the uint8 entry bit for bit (the same fused stem reads either)."""
    from deephisto_amd import tiles
    h, w = 700, 610
    host = synth.synth_slide(h, w, 3)
    slide = torch.from_numpy(host).to(dev)
    o = _origins(h, w, P, 12, P)
    ref = _oracle()
    m = _model(ref, dev)
    o_dev = torch.from_numpy(o).to(dev)
    got = m.forward_tiles(slide, o_dev, P)
    want = _oracle_logits(ref, host, o, P)
    _gate(got.cpu().numpy(), want, "forward_tiles vs oracle")
    x = tiles.gather_tiles(slide, o_dev, P)
    with torch.no_grad():
        ev = m(x)
    _gate(got.cpu().numpy(), ev.cpu().numpy(), "forward_tiles vs training-engine eval")
    assert torch.equal(m.forward_infer(x), got)


def test_launch_invariance_and_reproducibility(dev):
    """(4) one launch of the maximum size == the same origins in launches of 1, 7 and 128 tiles, bit for bit; two runs are identical;
    n = 1 and n not a multiple of 128 work."""
    from deephisto_amd.models.patch_cls_simple.resnet_bf16 import ResNet50HIP
    h, w, P = 1500, 1300, 224
    slide = torch.from_numpy(synth.synth_slide(h, w, 8)).to(dev)
    n = ResNet50HIP.MAX_TILES
    o_dev = torch.from_numpy(_origins(h, w, P, n, 1)).to(dev)
    m = _model(_oracle(9), dev)
    big = m.forward_tiles(slide, o_dev, P)
    assert torch.equal(big, m.forward_tiles(slide, o_dev, P))
    assert torch.isfinite(big).all()
    for step in (1, 7, 128):
        idx = list(range(0, 300 if step > 1 else 40, step))
        parts = torch.cat([m.forward_tiles(slide, o_dev[s:s + step], P) for s in idx])
        assert torch.equal(parts, big[:len(parts)]), f"launches of {step}"
    assert torch.equal(m.forward_tiles(slide, o_dev[1000:], P), big[1000:])   # n = 24


def test_resync_after_train_steps(dev):
    """(5) after two fused train_steps the inference handle serves the new weights and running statistics."""
    from deephisto_amd import tiles
    h, w, P = 600, 600, 96
    host = synth.synth_slide(h, w, 2)
    slide = torch.from_numpy(host).to(dev)
    ref = _oracle(4)
    m = _model(ref, dev)
    o = _origins(h, w, P, 8, 3)
    o_dev = torch.from_numpy(o).to(dev)
    before = m.forward_tiles(slide, o_dev, P)
    m.train()
    x = tiles.gather_tiles(slide, o_dev, P)
    labels = torch.arange(8, device=dev) % 5
    for _ in range(2):
        m.train_step(x, labels, lr=1e-2)
    m.eval()
    after = m.forward_tiles(slide, o_dev, P)
    assert not torch.equal(before, after)
    ref2 = o50.ResNet50Oracle(5)
    ref2.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})
    _gate(after.cpu().numpy(), _oracle_logits(ref2.eval(), host, o, P), "after train_step")


def test_dense_pipeline_vs_oracle_and_streamed(dev):
    """(6) predict_full_patched with a ResNet-50 at 224 / 112 vs the float32 oracle pipeline (per-tile logits under the gate, class
    map >= 99.9 %); the streamed (ONDISK_MULTIPROC) slide gives the resident result bit for bit."""
    from deephisto_amd.examples.predict_full_patched import predict_full_patched
    from deephisto_amd.patch_samplers.full_samplers import FullImageDenseSampler, SamplerExecutionMode
    h, w, P, S, B, d = 1200, 1000, 224, 112, 16, 16
    host = synth.synth_slide(h, w, 0)
    ref = _oracle(77)
    m = _model(ref, dev)
    o = tiling.batched_origins(h, w, P, S, B)
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    want = np.concatenate([_oracle_logits(ref, host, ob, P) for ob in o])
    want_map = tiling.class_map(tiling.accumulate_logits(h, w, 5, d, P, o.reshape(-1, 2), want))
    smp = FullImageDenseSampler(host, layer=1, patch_size=P, batch_size=B, stride=S, device=dev)
    cmap, logits = predict_full_patched(smp, m, 5, downscale=d, return_logits=True)
    _gate(logits.cpu().numpy(), want, "dense pipeline")
    agree = float((cmap.cpu().numpy() == want_map).mean())
    assert agree >= 0.999, f"class-map agreement {agree}"
    disk = FullImageDenseSampler(host, layer=1, patch_size=P, batch_size=B, stride=S, device=dev,
                                 mode=SamplerExecutionMode.ONDISK_MULTIPROC)
    cm2, lg2 = predict_full_patched(disk, m, 5, downscale=d, return_logits=True, streams=1)
    assert torch.equal(lg2, logits) and torch.equal(cm2, cmap)


def test_random_pipeline_equals_callback(dev):
    """(7) predict_random_patched with a ResNet-50 == ImagePredictorPatched fed by model.forward_tiles, same NumPy seed, bit for bit."""
    from deephisto_amd import tiles
    from deephisto_amd.examples.predict_full_patched import ImagePredictorPatched, predict_random_patched
    from deephisto_amd.patch_samplers.full_samplers import FullImageRndSampler
    h = w = 1536
    P, B, d = 224, 64, 16
    slide = tiles.synth_slide(h, w, 4, dev)
    m = _model(_oracle(6), dev)

    def smp():
        return FullImageRndSampler(slide, layer=1, patch_size=P, batch_size=B, dense_level=1, speedup=d, index_logic="device")

    np.random.seed(17)
    cmap, canvas = predict_random_patched(smp(), m, 5, d, return_canvas=True)

    def cb(patches):
        o = torch.from_numpy(np.array([(p.pos_y, p.pos_x) for p in patches], np.int32)).to(dev)
        return m.forward_tiles(slide, o, P)

    np.random.seed(17)
    origins, logits = [], []
    for patches, _ in smp().generator():
        logits.append(cb(patches))
        origins.append(np.array([(p.pos_y, p.pos_x) for p in patches], np.int32))
    canvas_cb, cmap_cb = tiles.accumulate_logits(torch.cat(logits).contiguous(), np.concatenate(origins), P, d, h, w)
    assert torch.equal(canvas, canvas_cb) and torch.equal(cmap, cmap_cb)
    np.random.seed(17)
    pred = ImagePredictorPatched((h, w), smp().generator(), cb, 5, layer=1, downscale=d).process()
    np.testing.assert_array_equal(cmap.cpu().numpy(), pred)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_cli_resnet50_checkpoint_one_and_two_ranks(built_lib, tmp_path):
    """(8) a ResNet-50 checkpoint through `python -m examples.predict_full_patched` (--arch auto), one rank and two ranks sharing
    cuda:0: bit-equal class maps, JPEGs written."""
    from deephisto_amd.models.patch_cls_simple.model import get_model
    torch.manual_seed(3)
    torch.save(get_model(5, arch="resnet50").state_dict(), tmp_path / "r50.pth")
    (tmp_path / "run.py").write_text(
        "import os, sys, numpy as np\n"
        "from examples import predict_full_patched as pfp\n"
        "from deephisto_amd.models.patch_cls_simple.resnet_bf16 import ResNet50HIP\n"
        "seen = []\n"
        "real = pfp.predict_full_patched\n"
        "pfp_mod = sys.modules['deephisto_amd.examples.predict_full_patched']\n"
        "def spy(smp, model, *a, **k):\n"
        "    seen.append(type(model).__name__)\n"
        "    return real(smp, model, *a, **k)\n"
        "pfp_mod.predict_full_patched = spy\n"
        "pred = pfp.main(sys.argv[1:])\n"
        "assert seen == ['ResNet50HIP'], seen\n"
        "np.save(f'pred_{os.environ.get(\"RANK\", \"0\")}_{os.environ.get(\"WORLD_SIZE\", \"1\")}.npy', pred.cpu().numpy())\n")
    args = ["--synthetic", "1100", "900", "--weights", str(tmp_path / "r50.pth"), "--patch_size", "224", "--stride", "112",
            "--batch_size", "16"]
    env = dict(os.environ, PYTHONPATH=f"{REPO / 'compat'}:{REPO}")
    r = subprocess.run([sys.executable, str(tmp_path / "run.py"), *args, "--out_dir", str(tmp_path / "one")], env=env, cwd=tmp_path,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    env.update(DH_DIST_BACKEND="gloo", DH_SHARE_GPU="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), str(tmp_path / "run.py"), *args, "--out_dir", str(tmp_path / "two")]
    r = subprocess.run(cmd, env=env, cwd=tmp_path, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    one = np.load(tmp_path / "pred_0_1.npy")
    assert one.shape == (1100 // 16, 900 // 16)
    for k in range(2):
        assert np.array_equal(np.load(tmp_path / f"pred_{k}_2.npy"), one), f"rank {k}"
    for d in ("one", "two"):
        for f in ("synthetic_1100x900_mask.jpg", "synthetic_1100x900.jpg", "synthetic_1100x900_overlay.jpg"):
            assert (tmp_path / d / f).stat().st_size > 0


def test_errors_are_python_errors_not_faults(dev):
    """(9) bad P, int64 origins, an origin past the slide edge, a launch above the maximum and a forward before finalize are refused
    with a message naming the problem; the handle keeps working afterwards."""
    import ctypes as C
    from deephisto_amd._lib import lib
    from deephisto_amd.models.patch_cls_simple.resnet_bf16 import ResNet50HIP
    h, w = 700, 700
    slide = torch.from_numpy(synth.synth_slide(h, w, 1)).to(dev)
    m = _model(_oracle(2), dev)
    o_dev = torch.from_numpy(_origins(h, w, 288, 4, 0)).to(dev)
    with pytest.raises(RuntimeError, match="patch 288"):
        m.forward_tiles(slide, o_dev, 288)
    with pytest.raises(RuntimeError, match="patch 100"):
        m.forward_tiles(slide, o_dev, 100)
    with pytest.raises(ValueError, match="int32"):
        m.forward_tiles(slide, o_dev.to(torch.int64), 224)
    bad = torch.tensor([[0, 0], [h - 224 + 1, 5]], dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match="outside"):
        m.forward_tiles(slide, bad, 224)
    many = torch.zeros((ResNet50HIP.MAX_TILES + 1, 2), dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match="launch limit"):
        m.forward_tiles(slide, many, 224)
    h0 = C.c_void_p()
    assert lib().dh_resnet50_create(C.byref(h0), 5) == 0
    try:
        out = torch.empty((1, 5), device=dev)
        rc = lib().dh_resnet50_forward_tiles(h0, slide.data_ptr(), h, w, o_dev.data_ptr(), 1, 224, out.data_ptr(), None)
        assert rc != 0 and b"finalize" in lib().dh_last_error()
    finally:
        lib().dh_resnet50_destroy(h0)
    good = torch.from_numpy(_origins(h, w, 224, 4, 0)).to(dev)
    assert torch.isfinite(m.forward_tiles(slide, good, 224)).all()
