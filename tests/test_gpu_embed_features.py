"""GPU: the pooled features out of both inference engines (dh_resnet18_features_tiles / dh_resnet50_features_tiles).

Slide, origins (the first four in the slide's corners) and models are those of tests/test_gpu_layer_parity.py.  Per case the launches
run once (module fixture): forward_tiles, the features entry with and without logits (each into a buffer with one extra sentinel row)
and one tapped forward of the last stored activation of all n tiles, the float64 reference of the pool.  HW = 49, 9, 9 and 4."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import layer_ref as lr
from oracle import resnet18 as o18
from oracle import resnet50 as o50
from oracle import synth

pytestmark = pytest.mark.gpu

CASES = [("r18", "bf16", 224, 300), ("r18", "f32", 96, 5), ("r50", "bf16", 96, 5), ("r50", "bf16", 64, 3)]
SENTINEL = -12345.5
U = 2.0 ** -24


def _oracle(arch):
    if arch == "r18":
        return o18.seeded_model(321, 5, perturb_bn=True).eval()
    ref = o50.seeded_model(5, 5, perturb_bn=True)
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
    arch, dtype, P, n = request.param
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    ref = _oracle(arch)
    m = get_model(5, compute_dtype=dtype) if arch == "r18" else get_model(5, arch="resnet50")
    m.load_state_dict(ref.state_dict())
    m = m.to(dev).eval()
    h, w = 2 * P + 300, 3 * P + 211
    slide = torch.from_numpy(synth.synth_slide(h, w, P + n)).to(dev)
    o_dev = torch.from_numpy(_origins(h, w, P, n, n)).to(dev)
    D = m.feature_width
    assert D == (512 if arch == "r18" else 2048)
    plain = m.forward_tiles(slide, o_dev, P)
    fwd, name = m.features_entry()

    def features(with_logits):
        feat = torch.full((n + 1, D), SENTINEL, dtype=torch.float32, device=dev)
        lg = torch.full((n + 1, 5), SENTINEL, dtype=torch.float32, device=dev)
        check(fwd(m._handle, slide.data_ptr(), h, w, o_dev.data_ptr(), n, P, feat.data_ptr(), lg.data_ptr() if with_logits else None,
                  None), name)
        return feat.cpu().numpy(), lg.cpu().numpy()

    feat_a, logits_a = features(True)
    feat_b, logits_b = features(False)
    # the float64 reference: the last stored activation of every tile, tapped right after the launch that writes it
    last = lr.topology(ref)[-1]["name"]
    Hl = P // 32
    sel = torch.arange(n, dtype=torch.int32, device=dev)
    act = torch.empty((n, D, Hl, Hl), dtype=torch.float32, device=dev)
    lg = torch.empty((n, 5), dtype=torch.float32, device=dev)
    tap = lib().dh_debug_resnet18_forward_tap if arch == "r18" else lib().dh_debug_resnet50_forward_tap
    check(tap(m._handle, slide.data_ptr(), h, w, o_dev.data_ptr(), n, P, last.encode(), sel.data_ptr(), n, act.data_ptr(), act.numel(),
              lg.data_ptr(), None), "forward tap")
    want = act.cpu().numpy().astype(np.float64).mean(axis=(2, 3))
    assert act.min().item() >= 0, "the last activation follows a ReLU"
    # the method itself gives the same rows
    f_m, l_m = m.features_tiles(slide, o_dev, P, return_logits=True)
    f_only = m.features_tiles(slide, o_dev, P)
    sd = ref.state_dict()
    return dict(n=n, D=D, HW=Hl * Hl, plain=plain.cpu().numpy(), feat_a=feat_a, logits_a=logits_a, feat_b=feat_b, logits_b=logits_b,
                want=want, f_m=f_m.cpu().numpy(), l_m=l_m.cpu().numpy(), f_only=f_only.cpu().numpy(),
                fc_w=sd["fc.weight"].double().numpy(), fc_b=sd["fc.bias"].double().numpy())


def test_logits_of_the_features_entry_are_those_of_forward_tiles(run):
    n = run["n"]
    assert np.array_equal(run["logits_a"][:n].view(np.uint32), run["plain"].view(np.uint32))
    assert np.array_equal(run["l_m"].view(np.uint32), run["plain"].view(np.uint32))


def test_features_do_not_depend_on_the_logits_pointer(run):
    n = run["n"]
    assert np.array_equal(run["feat_b"][:n].view(np.uint32), run["feat_a"][:n].view(np.uint32))
    assert np.array_equal(run["f_m"].view(np.uint32), run["feat_a"][:n].view(np.uint32))
    assert np.array_equal(run["f_only"].view(np.uint32), run["feat_a"][:n].view(np.uint32))


def test_features_against_the_float64_mean_of_the_tapped_activation(run):
    """HW - 1 additions of non-negative terms, the rounding of 1 / HW and one multiply: (HW + 1) u; the gate adds one unit."""
    got, want = run["feat_a"][:run["n"]].astype(np.float64), run["want"]
    err = np.abs(got - want)
    print(f"\nHW = {run['HW']}: max |got - want| / want = {np.max(err[want > 0] / want[want > 0]) / U:.3f} u, "
          f"{int((want == 0).sum())} exact zeros of {want.size}")
    assert np.all(err <= (run["HW"] + 2) * U * want)
    assert np.all(got[want == 0] == 0)


def test_fc_of_the_stored_features_gives_the_logits(run):
    n, D = run["n"], run["D"]
    f = run["feat_a"][:n].astype(np.float64)
    want = f @ run["fc_w"].T + run["fc_b"]
    mag = np.abs(f) @ np.abs(run["fc_w"]).T + np.abs(run["fc_b"])
    err = np.abs(run["logits_a"][:n].astype(np.float64) - want)
    print(f"\nD = {D}: max |logits - fc(features)| / bound = {np.max(err / ((D + 2) * U * mag)):.4f}")
    assert np.all(err <= (D + 2) * U * mag)


def test_nothing_is_written_past_the_last_row(run):
    n = run["n"]
    assert np.all(run["feat_a"][n] == SENTINEL) and np.all(run["feat_b"][n] == SENTINEL)
    assert np.all(run["logits_a"][n] == SENTINEL)
    assert np.all(run["logits_b"] == SENTINEL), "a null logits pointer must skip the fc: this buffer was never passed"
    assert not np.any(run["feat_a"][:n] == SENTINEL)


def test_engine_argument_checks(built_lib):
    from deephisto_amd.models.patch_cls_simple.model import get_model
    dev = torch.device("cuda:0")
    m = get_model(5, compute_dtype="bf16").to(dev)
    slide = torch.zeros((128, 128, 3), dtype=torch.uint8, device=dev)
    o = torch.zeros((1, 2), dtype=torch.int32, device=dev)
    with pytest.raises(NotImplementedError):
        m.train().features_tiles(slide, o, 64)
    m.eval()
    with pytest.raises(ValueError):
        m.features_tiles(slide.float(), o, 64)
    with pytest.raises(ValueError):
        m.features_tiles(slide, o.long(), 64)
    with pytest.raises(RuntimeError):
        m.features_tiles(slide.cpu(), o, 64)
    assert m.feature_width == 512 and m.features_entry()[1] == "dh_resnet18_features_tiles"
    assert isinstance(m.features_entry()[0], C._CFuncPtr)
