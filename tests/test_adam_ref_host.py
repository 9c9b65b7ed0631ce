"""CPU self-check of the Adam reference and gate (oracle/adam_ref.py) on the inputs of tests/test_gpu_adam.py, at a smaller arena.

  * the NumPy float32 restatement of adam_kernel's formula passes the gate on every element, after every step of every case;
  * each planted error (adam_ref.PLANTED) is refused by it: that is a property of the inputs (a band of |g| near eps, zeros, sign flips,
    three counted steps), asserted here so that the GPU test is known to be able to tell these errors from the kernel;
  * the reference agrees with torch.optim.Adam in float64, and the float32 bias corrections stay inside the bound the gate gives them.
"""
import math

import numpy as np
import pytest
import torch

from oracle import adam_ref as ar

N = 3 * 4096 * 8 + 5      # not a multiple of anything the kernel strides by


def _run(case, variant=None, n=N, seed=1):
    c = ar.CASES[case]
    p0 = ar.case_params(n, seed)
    ref = ar.AdamRef(p0, ar.LR, c["betas"], c["eps"])
    f32 = ar.AdamF32(p0.numpy(), ar.LR, c["betas"], c["eps"], variant)
    out = []
    for s, t in enumerate(c["steps"]):
        g = ar.case_grads(n, seed, s, c["eps"])
        want, gate = ref.step(g, t)
        got = torch.from_numpy(f32.step(g.numpy(), t)).double()
        out.append(((got - want).abs(), gate, want))
    return out


@pytest.mark.parametrize("case", list(ar.CASES))
def test_float32_restatement_meets_the_gate(case):
    for s, (err, gate, want) in enumerate(_run(case)):
        ratio = float((err / gate).max())
        print(f"[adam host] {case} step {s}: worst |got - want| / gate = {ratio:.3f}; median gate / lr = {float(gate.median()) / ar.LR:.2e}")
        assert bool((err <= gate).all()), (case, s, ratio)
        assert bool(torch.isfinite(want).all())
        # the gate stays a small fraction of the step it guards: half a unit of p plus <= 1e-3 of lr per step on the bulk
        assert float(gate.median()) <= (s + 1) * (1e-3 * ar.LR + 2.0 ** -24)


@pytest.mark.parametrize("variant", ar.PLANTED)
def test_planted_errors_fail_the_gate(variant):
    steps = _run("default-3-steps", variant)
    bad = [float((err > gate).double().mean()) for err, gate, _ in steps]
    print(f"[adam host] planted {variant}: fraction of elements outside the gate per step = {[f'{b:.3f}' for b in bad]}")
    assert max(bad) >= 0.05, (variant, bad)      # not one unlucky element: a whole class of inputs shows it


def test_no_subnormal_intermediates():
    for case, c in ar.CASES.items():
        for s in range(len(c["steps"])):
            g = ar.case_grads(N, 1, s, c["eps"]).numpy()
            nz = g[g != 0]
            inc = (np.float32(1) - np.float32(c["betas"][1])) * nz * nz
            assert float(np.abs(nz).min()) >= 1e-12 * 0.999 and float(inc.min()) >= 2.0 ** -126, case


def test_reference_is_torch_adam_in_float64():
    """Same recurrences as torch.optim.Adam (no weight decay, no amsgrad) run in float64 with the float32 values of the hyper-parameters."""
    c = ar.CASES["default-3-steps"]
    p0 = ar.case_params(4099, 2)
    ref = ar.AdamRef(p0, ar.LR, c["betas"], c["eps"])
    q = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.Adam([q], lr=ar.f32(ar.LR), betas=(ar.f32(0.9), ar.f32(0.999)), eps=ar.f32(c["eps"]))
    for s in range(3):
        g = ar.case_grads(4099, 2, s, c["eps"])
        want, _ = ref.step(g)
        q.grad = g.double()
        opt.step()
        assert float((q.detach() - want).abs().max()) <= 1e-15


@pytest.mark.parametrize("beta", [0.9, 0.999, 0.8, 0.99])
def test_float32_bias_correction_inside_its_bound(beta):
    b = np.float32(beta)
    for t in (1, 2, 3, 10, 1000, 1001, 100000, 100001):
        bc, rho = ar.bias_correction(float(b), t)
        got = float(np.float32(1) - np.power(b, np.float32(t)))
        assert abs(got - bc) <= rho * bc, (beta, t, got, bc, rho)
        assert rho >= 2.0 ** -24 and (t < 1000 or rho <= 1e-4)
    assert math.isclose(ar.bias_correction(float(np.float32(0.999)), 1)[0], 1 - float(np.float32(0.999)), rel_tol=1e-12)
