"""GPU: the class activation maps out of both inference engines (dh_resnet18_cam_tiles / dh_resnet50_cam_tiles).

Slide, origins (the first four in the slide's corners) and models are those of tests/test_gpu_embed_features.py.  Per case the
launches run once (module fixture): forward_tiles, the CAM entry with and without logits (each into a buffer with one extra sentinel
row), the same tiles in two launches, and one tapped forward of the last stored activation of all n tiles, from which fc per position
is computed in float64.  HW = 49, 1, 9, 9, 4 and 4; the last case has 64 classes: eight passes of the class chunking."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import layer_ref as lr
from oracle import resnet18 as o18
from oracle import resnet50 as o50
from oracle import synth

pytestmark = pytest.mark.gpu

CASES = [("r18", "bf16", 224, 20, 5), ("r18", "bf16", 32, 5, 5), ("r18", "f32", 96, 5, 5), ("r50", "bf16", 96, 5, 5),
         ("r50", "bf16", 64, 3, 5), ("r50", "bf16", 64, 3, 64)]
SENTINEL = -12345.5
U = 2.0 ** -24


def _oracle(arch, n_cls):
    if arch == "r18":
        return o18.seeded_model(321, n_cls, perturb_bn=True).eval()
    ref = o50.seeded_model(5, n_cls, perturb_bn=True)
    with torch.no_grad():
        for name, mod in ref.named_modules():
            if name.endswith("bn3"):
                mod.weight.mul_(0.2)
    return ref.eval()


def _origins(h, w, P, n, seed):
    rng = np.random.default_rng(seed)
    o = [(0, 0), (0, w - P), (h - P, 0), (h - P, w - P)]
    o += [(int(rng.integers(0, h - P + 1)), int(rng.integers(0, w - P + 1))) for _ in range(n - 4)]
    return np.asarray(o[:n], np.int32)


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "-".join(map(str, c)))
def run(request, built_lib):
    from deephisto_amd._lib import check, lib
    from deephisto_amd.models.patch_cls_simple.model import get_model
    arch, dtype, P, n, K = request.param
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    ref = _oracle(arch, K)
    m = get_model(K, compute_dtype=dtype) if arch == "r18" else get_model(K, arch="resnet50")
    m.load_state_dict(ref.state_dict())
    m = m.to(dev).eval()
    h, w = 2 * P + 300, 3 * P + 211
    slide = torch.from_numpy(synth.synth_slide(h, w, P + n)).to(dev)
    o_dev = torch.from_numpy(_origins(h, w, P, n, n)).to(dev)
    D, S = m.feature_width, P // 32
    HW = S * S
    plain = m.forward_tiles(slide, o_dev, P)
    fwd, name = m.cam_entry()

    def cams(with_logits, lo=0, hi=n):
        cam = torch.full((hi - lo + 1, HW, K), SENTINEL, dtype=torch.float32, device=dev)
        lg = torch.full((hi - lo + 1, K), SENTINEL, dtype=torch.float32, device=dev)
        check(fwd(m._handle, slide.data_ptr(), h, w, o_dev.data_ptr() + 8 * lo, hi - lo, P, cam.data_ptr(),
                  lg.data_ptr() if with_logits else None, None), name)
        return cam.cpu().numpy(), lg.cpu().numpy()

    cam_a, logits_a = cams(True)
    cam_b, logits_b = cams(False)
    k = n // 2
    halves = np.concatenate([cams(False, 0, k)[0][:k], cams(False, k, n)[0][:n - k]])
    # the float64 reference: the last stored activation of every tile, tapped right after the launch that writes it
    last = lr.topology(ref)[-1]["name"]
    sel = torch.arange(n, dtype=torch.int32, device=dev)
    act = torch.empty((n, D, S, S), dtype=torch.float32, device=dev)
    lg = torch.empty((n, K), dtype=torch.float32, device=dev)
    tap = lib().dh_debug_resnet18_forward_tap if arch == "r18" else lib().dh_debug_resnet50_forward_tap
    check(tap(m._handle, slide.data_ptr(), h, w, o_dev.data_ptr(), n, P, last.encode(), sel.data_ptr(), n, act.data_ptr(), act.numel(),
              lg.data_ptr(), None), "forward tap")
    assert act.min().item() >= 0, "the last activation follows a ReLU"
    a = act.cpu().numpy().astype(np.float64).reshape(n, D, HW).transpose(0, 2, 1)   # [n][p][c], p = i * S + j
    c_m, l_m = m.cam_tiles(slide, o_dev, P, return_logits=True)
    c_only = m.cam_tiles(slide, o_dev, P)
    sd = ref.state_dict()
    return dict(n=n, D=D, S=S, HW=HW, K=K, plain=plain.cpu().numpy(), cam_a=cam_a, logits_a=logits_a, cam_b=cam_b, logits_b=logits_b,
                halves=halves, a=a, c_m=c_m.cpu().numpy(), l_m=l_m.cpu().numpy(), c_only=c_only.cpu().numpy(),
                fc_w=sd["fc.weight"].double().numpy(), fc_b=sd["fc.bias"].double().numpy())


def test_cam_against_fc_per_position_in_float64(run):
    """A C-term float32 dot product in any order plus the bias: (C + 2) u (sum |w||a| + |b|) per element."""
    n, D = run["n"], run["D"]
    want = run["a"] @ run["fc_w"].T + run["fc_b"]
    mag = run["a"] @ np.abs(run["fc_w"]).T + np.abs(run["fc_b"])
    err = np.abs(run["cam_a"][:n].astype(np.float64) - want)
    print(f"\nC = {D}, HW = {run['HW']}, n_cls = {run['K']}: max |cam - fc(a_p)| / bound = {np.max(err / ((D + 2) * U * mag)):.4f}")
    assert np.all(err <= (D + 2) * U * mag)


def test_mean_over_positions_gives_the_entry_s_own_logits(run):
    """logits = mean_p cam: the sum of both computations' bounds, (2 C + HW + 8) u (|fc_w| . pooled + |fc_b|); the activations
    follow a ReLU, so the mean of |a| is the pooled vector."""
    n, D, HW = run["n"], run["D"], run["HW"]
    got = run["cam_a"][:n].astype(np.float64).mean(axis=1)
    pooled = run["a"].mean(axis=1)
    mag = pooled @ np.abs(run["fc_w"]).T + np.abs(run["fc_b"])
    err = np.abs(got - run["logits_a"][:n].astype(np.float64))
    print(f"\nC = {D}, HW = {HW}: max |mean_p cam - logits| / bound = {np.max(err / ((2 * D + HW + 8) * U * mag)):.4f}")
    assert np.all(err <= (2 * D + HW + 8) * U * mag)


def test_logits_of_the_cam_entry_are_those_of_forward_tiles(run):
    n = run["n"]
    assert np.array_equal(run["logits_a"][:n].view(np.uint32), run["plain"].view(np.uint32))
    assert np.array_equal(run["l_m"].view(np.uint32), run["plain"].view(np.uint32))


def test_cam_does_not_depend_on_the_logits_pointer(run):
    n, S, K = run["n"], run["S"], run["K"]
    assert np.array_equal(run["cam_b"][:n].view(np.uint32), run["cam_a"][:n].view(np.uint32))
    assert run["c_m"].shape == (n, S, S, K) and run["c_only"].shape == (n, S, S, K)
    assert np.array_equal(run["c_m"].reshape(n, -1, K).view(np.uint32), run["cam_a"][:n].view(np.uint32))
    assert np.array_equal(run["c_only"].reshape(n, -1, K).view(np.uint32), run["cam_a"][:n].view(np.uint32))


def test_nothing_is_written_past_the_last_row(run):
    n = run["n"]
    assert np.all(run["cam_a"][n] == SENTINEL) and np.all(run["cam_b"][n] == SENTINEL)
    assert np.all(run["logits_a"][n] == SENTINEL)
    assert np.all(run["logits_b"] == SENTINEL), "a null logits pointer must skip the head: this buffer was never passed"
    assert not np.any(run["cam_a"][:n] == SENTINEL)


def test_rows_do_not_depend_on_the_launch(run):
    """Tiles [0, n) in one launch and as [0, k) + [k, n): the property the sharded path relies on."""
    assert np.array_equal(run["halves"].view(np.uint32), run["cam_a"][:run["n"]].view(np.uint32))


def test_engine_argument_checks(built_lib):
    from deephisto_amd.models.patch_cls_simple.model import get_model
    dev = torch.device("cuda:0")
    m = get_model(5, compute_dtype="bf16").to(dev)
    slide = torch.zeros((128, 128, 3), dtype=torch.uint8, device=dev)
    o = torch.zeros((1, 2), dtype=torch.int32, device=dev)
    with pytest.raises(NotImplementedError):
        m.train().cam_tiles(slide, o, 64)
    m.eval()
    with pytest.raises(ValueError):
        m.cam_tiles(slide.float(), o, 64)
    with pytest.raises(ValueError):
        m.cam_tiles(slide, o.long(), 64)
    with pytest.raises(RuntimeError):
        m.cam_tiles(slide.cpu(), o, 64)
    with pytest.raises(ValueError, match="multiple of 32"):
        m.cam_tiles(slide, o, 100)
    assert m.forward_tiles(slide, o, 100).shape == (1, 5), "plain prediction keeps taking other patch sizes"
    assert m.cam_entry()[1] == "dh_resnet18_cam_tiles" and isinstance(m.cam_entry()[0], C._CFuncPtr)
