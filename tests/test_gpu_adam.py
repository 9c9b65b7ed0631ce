"""Element-wise float64 parity of the engines' Adam step (adam_kernel, reached through dh_resnet18_adam_step and dh_train2_adam_step).

Both engines are driven through their flat arenas: parameters P and gradients G are filled over the WHOLE arena (11.2 M elements, about ten
times what one pass of the capped grid covers, and not a multiple of it), `*_adam_step` runs, and every element of P is compared after every
step with oracle/adam_ref.AdamRef -- the same recurrences in float64 on the same float32 operands, carrying its own m and v, evaluated on
the device.  The gate is AdamRef's E_p (derivation in oracle/adam_ref.py): the float32 roundings of the update counted from the kernel's
expression, the conditioning of the float32 bias corrections, an absolute bound for the first moment, half a unit of p per step.  Nothing in
it comes from what the kernel returns; tests/test_adam_ref_host.py shows on these inputs that a float32 evaluation of the kernel's formula
passes it and that each of seven planted formula errors does not.

Cases (oracle/adam_ref.CASES) x engine: three counted steps (step = 0) with the default hyper-parameters, with eps = 1e-3, with betas
(0.8, 0.99); explicit step = 1000, 1001 and step = 100000, 100001 on fresh handles.  Gradients: log-uniform 1e-12 .. 1e2 of both signs, a band
at |g| ~ eps, exact zeros, elements that flip sign between steps (adam_ref.case_grads).

Measured on an MI355X, worst |got - want| / gate over the arena (11 179 080 elements), both engines alike: 1.000 after the first step of
every case, 0.996 .. 1.000 after the second, 0.972 .. 0.995 after the third.  The worst element is always a parameter of order one whose
update (about lr) is far below its unit: its distance to the reference is the half unit of the final subtraction, which is the gate's
leading term there, so the ratio sits at 1 from below by construction; the update itself is resolved on the parameters near 1e-6 and 0.
File: 24 s wall for the ten cases (1.6 .. 3.4 s each, most of it drawing the inputs on the host).
"""
import ctypes as C

import pytest
import torch

from oracle import adam_ref as ar

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


class _F32Engine:
    """The float32 engine's training state: it lives in an inference handle and exists after one training forward (B = 1, P = 64)."""

    def __init__(self, dev):
        from deephisto_amd.models.patch_cls_simple.model import get_model
        self.model = get_model(5, "f32").to(dev).train()
        self.eng = self.model._engine
        self.eng.forward(torch.rand(1, 3, 64, 64, device=dev))
        self.flat = lambda kind: self.eng.flat(kind, dev)

    def adam(self, lr, betas, eps, step):
        self.eng._call("adam_step", lr, betas[0], betas[1], eps, step, None)

    def close(self):
        self.model._release()


class _Bf16Engine:
    """A dh_train2 handle: its arenas exist from creation on."""

    def __init__(self, dev):
        from deephisto_amd._lib import check, lib
        from deephisto_amd.models.patch_cls_simple.engine import _DevView
        self.h = C.c_void_p()
        check(lib().dh_train2_create(C.byref(self.h), b"resnet18", 5), "dh_train2_create")

        def flat(kind):
            ptr, n = C.c_void_p(), C.c_int64()
            check(lib().dh_train2_flat(self.h, kind, C.byref(ptr), C.byref(n)), "dh_train2_flat")
            return torch.as_tensor(_DevView(ptr.value, n.value), device=dev)
        self.flat = flat

    def adam(self, lr, betas, eps, step):
        from deephisto_amd._lib import check, lib
        check(lib().dh_train2_adam_step(self.h, lr, betas[0], betas[1], eps, step, None), "dh_train2_adam_step")

    def close(self):
        from deephisto_amd._lib import lib
        lib().dh_train2_destroy(self.h)


@pytest.mark.parametrize("engine", ["f32", "bf16"])
@pytest.mark.parametrize("case", list(ar.CASES))
def test_adam_step_every_element(dev, engine, case):
    c = ar.CASES[case]
    seed = list(ar.CASES).index(case) + (10 if engine == "bf16" else 0)
    e = (_F32Engine if engine == "f32" else _Bf16Engine)(dev)
    try:
        P, G = e.flat(0), e.flat(1)
        n = P.numel()
        assert n == G.numel() and n > 10 * 256 * 4096 and n % (256 * 4096) != 0   # grid-stride rounds and a tail
        p0 = ar.case_params(n, seed).to(dev)
        P.copy_(p0)
        ref = ar.AdamRef(p0, ar.LR, c["betas"], c["eps"])
        for s, t in enumerate(c["steps"]):
            g = ar.case_grads(n, seed, s, c["eps"]).to(dev)
            G.copy_(g)
            e.adam(ar.LR, c["betas"], c["eps"], t)
            torch.cuda.synchronize()
            want, gate = ref.step(g, t)
            got = P.double()
            assert bool(torch.isfinite(got).all()), (engine, case, s)
            err = (got - want).abs()
            ratio = err / gate
            worst = int(ratio.argmax())
            print(f"[adam] {engine} {case} step {s} (t = {ref.t}): worst |got - want| / gate = {float(ratio[worst]):.3f} at element {worst} of {n}"
                  f" (got {float(got[worst])!r}, want {float(want[worst])!r}); moved elements {int((got != p0.double()).sum())}")
            bad = err > gate
            assert not bool(bad.any()), (engine, case, s, int(bad.sum()), int(bad.nonzero()[0]), float(ratio[worst]))
            assert torch.equal(G, g)      # the step leaves the gradients alone
    finally:
        e.close()
