"""The parameter entry points of the inference handles (`dh_resnet18_*` in float32 and bf16, `dh_resnet50_*`): set_param, finalize's
checks, the finalized check of the forwards, destroy.  CPU only: no kernel runs and no device memory is touched -- every failure
asserted here has to come before the first upload.  Names and element counts are those of the oracles' CPU state_dicts."""
import ctypes as C

import numpy as np
import pytest

N_CLS = 5
HANDLES = ["resnet18-f32", "resnet18-bf16", "resnet50"]


@pytest.fixture(scope="module")
def state_dicts():
    from oracle import resnet18, resnet50
    out = {}
    for abi, mod in (("resnet18", resnet18), ("resnet50", resnet50)):
        sd = mod.seeded_model(0, N_CLS).state_dict()
        out[abi] = {k: np.ascontiguousarray(v.numpy().astype(np.float32).ravel()) for k, v in sd.items()}
    return out


class Handle:
    def __init__(self, lib, kind):
        self.lib, self.kind, self.abi = lib, kind, kind.split("-")[0]
        self.h = C.c_void_p()
        if self.abi == "resnet18":
            from deephisto_amd import _lib
            rc = lib.dh_resnet18_create(C.byref(self.h), N_CLS, _lib.DH_DTYPE_F32 if kind.endswith("f32") else _lib.DH_DTYPE_BF16)
        else:
            rc = lib.dh_resnet50_create(C.byref(self.h), N_CLS)
        assert rc == 0, lib.dh_last_error()

    def call(self, entry, *args):
        return getattr(self.lib, f"dh_{self.abi}_{entry}")(self.h, *args)

    def set_param(self, name, a, n=None):
        return self.call("set_param", name.encode(), a.ctypes.data_as(C.c_void_p), a.size if n is None else n)

    def error(self):
        return self.lib.dh_last_error().decode()

    def destroy(self):
        self.call("destroy")
        self.h = None


@pytest.fixture(params=HANDLES)
def handle(request, built_lib):
    h = Handle(built_lib, request.param)
    yield h
    if h.h is not None:
        h.destroy()


def test_set_param_takes_every_state_dict_entry_with_its_own_count(handle, state_dicts):
    sd = state_dicts[handle.abi]
    assert sum(k.endswith("num_batches_tracked") for k in sd) > 0
    for name, a in sd.items():
        assert a.size == 1 or not name.endswith("num_batches_tracked")
        assert handle.set_param(name, a) == 0, f"{name}: {handle.error()}"
    for name, a in sd.items():
        longer = np.zeros(a.size + 1, np.float32)
        assert handle.set_param(name, longer) == -22, name
        msg = handle.error()
        assert f"'{name}'" in msg and f"{a.size + 1} elements" in msg and f"expected {a.size}" in msg, msg


def test_names_of_another_architecture_are_refused(handle, state_dicts):
    buf = np.zeros(512 * 512 * 9, np.float32)
    assert handle.set_param("layer5.0.conv1.weight", buf, 64 * 64 * 9) == -22
    assert "unknown parameter 'layer5.0.conv1.weight'" in handle.error()
    for name, n in (("layer1.0.conv3.weight", 256 * 64), ("layer1.0.downsample.0.weight", 256 * 64)):
        assert state_dicts["resnet50"][name].size == n and name not in state_dicts["resnet18"]
        rc = handle.set_param(name, buf, n)
        if handle.abi == "resnet18":
            assert rc == -22 and f"unknown parameter '{name}'" in handle.error()
        else:
            assert rc == 0, handle.error()


def test_finalize_of_a_fresh_handle_names_the_stem(handle):
    assert handle.call("finalize", None) == -22
    msg = handle.error()
    assert handle.abi in msg and "'conv1' / 'bn1'" in msg and "not all set" in msg, msg


def test_finalize_checks_the_fc_before_it_uploads_anything(handle, state_dicts):
    """Everything but fc.bias is set: the refusal must come before the first upload (this test has no device to upload to)."""
    for name, a in state_dicts[handle.abi].items():
        if name != "fc.bias":
            assert handle.set_param(name, a) == 0, handle.error()
    assert handle.call("finalize", None) == -22
    assert f"{handle.abi} finalize: fc.weight / fc.bias are not set" in handle.error()


def test_forward_entries_ask_for_finalize_first(handle, state_dicts):
    n, P = 1, 64
    x = np.zeros((n, 3, P, P), np.float32)
    slide = np.zeros((P, P, 3), np.uint8)
    yx = np.zeros((n, 2), np.int32)
    logits = np.zeros((n, N_CLS), np.float32)
    feat = np.zeros((n, 2048), np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    want = f"call dh_{handle.abi}_finalize"
    for filled in (False, True):   # a fresh handle, and one whose parameters are set but not finalized
        if filled:
            for name, a in state_dicts[handle.abi].items():
                assert handle.set_param(name, a) == 0, handle.error()
        assert handle.call("forward", p(x), n, P, p(logits), None) == -22 and want in handle.error()
        assert handle.call("forward_tiles", p(slide), P, P, p(yx), n, P, p(logits), None) == -22 and want in handle.error()
        assert handle.call("features_tiles", p(slide), P, P, p(yx), n, P, p(feat), p(logits), None) == -22 and want in handle.error()


def test_destroy(handle, state_dicts, built_lib):
    getattr(built_lib, f"dh_{handle.abi}_destroy")(None)   # a no-op
    fresh = Handle(built_lib, handle.kind)
    fresh.destroy()
    for name, a in state_dicts[handle.abi].items():
        assert handle.set_param(name, a) == 0, handle.error()
    handle.destroy()
