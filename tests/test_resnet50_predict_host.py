"""CPU: backbone selection of the prediction entry points (`--arch auto` / `load_model`) from a checkpoint's state_dict keys."""
import pytest
import torch


def _sd(arch):
    from deephisto_amd.models.patch_cls_simple.model import get_model
    return get_model(5, arch=arch).state_dict()


def test_detect_arch_from_keys():
    from deephisto_amd.examples.predict_full_patched import detect_arch, resolve_arch
    r18, r50 = _sd("resnet18"), _sd("resnet50")
    assert detect_arch(r18) == "resnet18" and detect_arch(r50) == "resnet50"
    assert resolve_arch("auto", r50) == "resnet50" and resolve_arch(None, r18) == "resnet18"
    assert resolve_arch("auto") == "resnet18"            # --weights '': the reference's ResNet-18
    assert resolve_arch("resnet50") == "resnet50"
    assert resolve_arch("resnet50", r50) == "resnet50"


def test_mismatched_explicit_arch_is_refused():
    from deephisto_amd.examples.predict_full_patched import resolve_arch
    with pytest.raises(ValueError, match="--arch resnet18 does not match the checkpoint.*resnet50"):
        resolve_arch("resnet18", _sd("resnet50"))
    with pytest.raises(ValueError, match="--arch resnet50 does not match the checkpoint.*resnet18"):
        resolve_arch("resnet50", _sd("resnet18"))
    with pytest.raises(ValueError, match="unknown architecture"):
        resolve_arch("resnet34")


def test_load_model_builds_the_checkpoints_backbone(tmp_path):
    from deephisto_amd.examples.predict_full_patched import load_model
    from deephisto_amd.models.patch_cls_simple.model import ResNet18HIP, ResNet50HIP
    for arch, cls in (("resnet18", ResNet18HIP), ("resnet50", ResNet50HIP)):
        sd = _sd(arch)
        torch.save(sd, tmp_path / f"{arch}.pth")
        m = load_model(tmp_path / f"{arch}.pth", "cpu")
        assert type(m) is cls and not m.training
        assert torch.equal(m.state_dict()["fc.weight"], sd["fc.weight"])
    assert load_model(tmp_path / "resnet50.pth", "cpu", "f32").compute_dtype == "bf16"
    with pytest.raises(ValueError, match="does not match"):
        load_model(tmp_path / "resnet50.pth", "cpu", arch="resnet18")
