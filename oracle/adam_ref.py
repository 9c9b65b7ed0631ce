"""float64 reference of the engines' Adam step (adam_kernel, csrc/train_core_kernels.inc) and the element-wise gate its parameters are held to
(tests/test_gpu_adam.py; the reference and the gate are checked by tests/test_adam_ref_host.py).

The kernel, per element, all in float32 with -ffp-contract=off (a contracted multiply-add would only drop roundings):

    m' = b1 * m + (1 - b1) * g
    v' = b2 * v + (1 - b2) * g * g                       (left to right: ((1 - b2) * g) * g)
    d  = sqrtf(v') / bc2s + eps
    p' = p - (lr / bc1) * (m' / d)

with bc1 = 1 - powf(b1, t) and bc2s = sqrtf(1 - powf(b2, t)) evaluated in float32 on the host (t = (float)step).  `AdamRef` evaluates the same
expressions in float64 on the SAME operands -- lr, b1, b2, eps are taken as the float32 values the entry point receives, p and g as the float32
arena contents -- and carries its own m, v and p across steps (the engines do not expose their moments).  Next to each value it carries a
bound on the distance of the float32 state from it; u = 2^-24, gamma(K) = K u / (1 - K u), hats are the float64 values:

  m   every term of m' passes at most 3 roundings ((1 - b1), its product with g, the addition; b1 * m: product, addition) and m itself is
      off by E_m, so                     E_m' = (1 + gamma(3)) b1 E_m + gamma(3) (|b1 m^| + |(1 - b1) g|).
      m may cancel (a gradient that flips sign), so this bound is ABSOLUTE and is carried as such into the update below.
  v   all terms are non-negative; at most 4 roundings ((1 - b2), two products, the addition):
                                         E_v' = (1 + gamma(4)) b2 E_v + gamma(4) (b2 v^ + (1 - b2) g^2).
  bc  P = powf(b, t) = b^t (1 + dp) with |dp| <= 2^-23 (glibc documents powf to 1 ulp) or, where b^t is subnormal, |P - b^t| <= 2^-149;
      bc = fl(1 - P) = (1 - b^t)(1 + ds)(1 - b^t dp / (1 - b^t)), |ds| <= u.  The subtraction is well conditioned only while b^t is
      small: the relative error of 1 - b^t is amplified by b^t / (1 - b^t).  To that the gate adds the term the bias correction is specified
      with, u (1 + t b^t) / (1 - b^t): the rounding of P itself (absolute error <= u) and the sensitivity t b^t of b^t to the last bit of b.
                                         rho(b, t) = u + (2^-23 b^t + 2^-149 + u (1 + t b^t)) / (1 - b^t)
      What float32 costs here: at t = 1 with b2 = 0.999, rho = 2.4e-4 (4000 u: 1 - b^t = 1e-3 is formed from a number next to 1), so the
      first update is known to 1.2e-4 of lr; with b1 = 0.9, rho = 2e-6.  At t = 1000: rho(0.999) = 3.5e-5 (t b^t = 368), rho(0.9) = u.  At t = 10^5 both
      b^t are below 2^-126, both corrections are exactly 1 and rho = u.
  d   sqrtf and the divisions are correctly rounded (the build keeps hipcc's default, no fast-math).  With rho_v = E_v / v^,
      |sqrt(1 + x) - 1| <= |x| / 2 (1 + |x|), and prod (1 + d_i)^(+-1) = 1 + theta, |theta| <= S / (1 - S) for S = sum |d_i|:
      r = sqrtf(v') / bc2s is off by     S_r = rho_v / 2 (1 + rho_v) + rho_2 / 2 (1 + rho_2) + 3 u   (rho_2 = rho(b2, t); sqrtf, sqrtf, division)
      relative, eps is exact, so d is off by   S_d = w S_r / (1 - S_r) + u,  w = r^ / d^ <= 1 the share of d that carries an error.
  u   q = fl(m' / d): |m'/d - m^/d^| <= E_m / (d^ (1 - S_d)) + |q^| S_d / (1 - S_d); a = fl(lr / bc1) is off by S_a = rho_1 + u; the quotient's
      and the product's roundings add 2 u: T = (S_a + 2 u) / (1 - S_a - 2 u), and for upd = fl(a q) against upd^ = a^ q^
                                         E_u = |upd^| (T + (1 + T) S_d / (1 - S_d)) + a^ (1 + T) E_m / (d^ (1 - S_d)).
  p   the subtraction rounds once: half a unit of float32 at the magnitude the float32 result can have,
                                         E_p' = E_p + E_u + quantum(|p^'| + E_p + E_u) / 2.

E_p after each step is the gate of that step: |p_engine - p^| <= E_p, element by element.  Nothing in it is taken from what an engine returns.
No intermediate may be subnormal ((1 - b2) g^2 >= 2^-126 for every non-zero g: |g| >= 1e-17 suffices for b2 <= 0.9999); `case_grads` keeps
|g| >= 1e-12 on every non-zero element.

Everything here is torch float64 on whatever device the operands live on, so the GPU test evaluates the whole arena (1e7 elements, several
steps) in float64 on the device and the CPU test runs the very same code.
"""
from __future__ import annotations

import math

import numpy as np
import torch

U = 2.0 ** -24
U_POWF = 2.0 ** -23


def gamma(K: int) -> float:
    return K * U / (1 - K * U)


def f32(x: float) -> float:
    """The float32 value an entry point receives for the Python float x, as a Python float (exact in float64)."""
    return float(np.float32(x))


def bias_correction(beta: float, t: int) -> tuple[float, float]:
    """(1 - beta^t in float64, rho: bound on the relative error of the float32 evaluation 1.f - powf(beta, (float)t)).  beta: a float32 value."""
    assert 0 < t < 2 ** 24 and 0.0 < beta < 1.0
    bt = math.exp(t * math.log(beta)) if t * math.log(beta) > -745 else 0.0
    bc = -math.expm1(t * math.log(beta))
    return bc, U + (U_POWF * bt + 2.0 ** -149 + U * (1 + t * bt)) / bc


def quantum32(v: torch.Tensor) -> torch.Tensor:
    """ulp of float64 values in float32 (subnormal spacing below 2^-126), as oracle.layer_ref.quantum(v, "f32")."""
    _, e = torch.frexp(v)
    return torch.ldexp(torch.ones_like(v), e.clamp(min=-125) - 24)


class AdamRef:
    """float64 Adam state (p, m, v) of one arena and the error bounds (E_p, E_m, E_v) of a float32 engine stepping the same operands."""

    def __init__(self, p, lr: float, betas=(0.9, 0.999), eps: float = 1e-8):
        self.p = torch.as_tensor(p).to(torch.float64).clone()
        self.m, self.v = torch.zeros_like(self.p), torch.zeros_like(self.p)
        self.Ep, self.Em, self.Ev = torch.zeros_like(self.p), torch.zeros_like(self.p), torch.zeros_like(self.p)
        self.lr, self.b1, self.b2, self.eps = f32(lr), f32(betas[0]), f32(betas[1]), f32(eps)
        self.t = 0

    def step(self, g, t: int = 0):
        """One step on gradient g (float32 values); t <= 0: the reference's own count, as the engines count.  Returns (p^, E_p)."""
        t = self.t + 1 if t <= 0 else int(t)
        self.t = t
        g = torch.as_tensor(g).to(torch.float64)
        b1, b2, eps = self.b1, self.b2, self.eps
        g3, g4 = gamma(3), gamma(4)
        t1, t2 = b1 * self.m, (1 - b1) * g
        self.Em = (1 + g3) * b1 * self.Em + g3 * (t1.abs() + t2.abs())
        self.m = t1 + t2
        s1, s2 = b2 * self.v, (1 - b2) * g * g
        self.Ev = (1 + g4) * b2 * self.Ev + g4 * (s1 + s2)
        self.v = s1 + s2
        bc1, rho1 = bias_correction(b1, t)
        bc2, rho2 = bias_correction(b2, t)
        r = self.v.sqrt() / math.sqrt(bc2)
        d = r + eps
        a = self.lr / bc1
        q = self.m / d
        upd = a * q
        rho_v = torch.where(self.v > 0, self.Ev / self.v.clamp(min=1e-300), torch.zeros_like(self.v))
        S_r = rho_v / 2 * (1 + rho_v) + rho2 / 2 * (1 + rho2) + 3 * U
        S_d = (r / d) * S_r / (1 - S_r) + U
        S_a = rho1 + U
        T = (S_a + 2 * U) / (1 - S_a - 2 * U)
        Eu = upd.abs() * (T + (1 + T) * S_d / (1 - S_d)) + a * (1 + T) * self.Em / (d * (1 - S_d))
        self.p = self.p - upd
        self.Ep = self.Ep + Eu
        self.Ep = self.Ep + 0.5 * quantum32(self.p.abs() + self.Ep)
        return self.p, self.Ep


# ---- float32 restatement of the kernel, and the errors a test must be able to tell from it ------------------------------------------

PLANTED = ("eps_in_root", "eps_before_bc2", "no_bc1", "bc2_not_rooted", "step_off_by_one", "v_from_g_not_g2", "p_from_old_moments")


class AdamF32:
    """adam_kernel restated in NumPy float32, one rounding per operation as the kernel is compiled.  `variant`: None = the kernel's formula;
    one of PLANTED = that formula with ONE deliberate error (the gate has to refuse each of them)."""

    def __init__(self, p, lr, betas=(0.9, 0.999), eps=1e-8, variant: str | None = None):
        assert variant is None or variant in PLANTED
        F = np.float32
        self.p = np.asarray(p, F).copy()
        self.m, self.v = np.zeros_like(self.p), np.zeros_like(self.p)
        self.lr, self.b1, self.b2, self.eps = F(lr), F(betas[0]), F(betas[1]), F(eps)
        self.t, self.variant = 0, variant

    def step(self, g, t: int = 0):
        F, one = np.float32, np.float32(1)
        t = self.t + 1 if t <= 0 else int(t)
        self.t = t
        var, b1, b2, eps = self.variant, self.b1, self.b2, self.eps
        g = np.asarray(g, F)
        tb = max(t - 1, 1) if var == "step_off_by_one" else t
        bc1 = one - np.power(b1, F(tb))
        bc2 = one - np.power(b2, F(tb))
        bc2s = np.sqrt(bc2)
        m0, v0 = self.m, self.v
        m = b1 * m0 + (one - b1) * g
        v = b2 * v0 + ((one - b2) * g if var == "v_from_g_not_g2" else (one - b2) * g * g)
        if var == "v_from_g_not_g2":
            v = np.abs(v)                     # keep the root real: the planted error is the missing square, not a NaN
        mu, vu = (m0, v0) if var == "p_from_old_moments" else (m, v)
        if var == "eps_in_root":
            d = np.sqrt(vu + eps) / bc2s
        elif var == "eps_before_bc2":
            d = (np.sqrt(vu) + eps) / bc2s
        elif var == "bc2_not_rooted":
            d = np.sqrt(vu) / bc2 + eps
        else:
            d = np.sqrt(vu) / bc2s + eps
        a = self.lr if var == "no_bc1" else self.lr / bc1
        self.p = self.p - a * (mu / d)
        self.m, self.v = m, v
        assert self.p.dtype == F
        return self.p


# ---- the inputs of both tests ---------------------------------------------------------------------------------------------------------

def case_params(n: int, seed: int) -> torch.Tensor:
    """float32 parameters over a whole arena: weights of a few 1e-2, exact zeros, values near 1e-6 (where half a unit of p hides nothing
    of an update of lr) and values of order one, interleaved at random."""
    gen = torch.Generator().manual_seed(1000 + seed)
    cls = torch.randint(0, 4, (n,), generator=gen)
    z = torch.randn(n, generator=gen)
    scale = torch.tensor([5e-2, 0.0, 1e-6, 1.0])[cls]
    return (z * scale).to(torch.float32)


def case_grads(n: int, seed: int, s: int, eps: float) -> torch.Tensor:
    """float32 gradients of step index s = 0, 1, 2 ... of a case.  Every element keeps its class through the steps:
      0-2  magnitude log-uniform over 1e-12 .. 1e2, sign at random, both drawn anew every step;
      3    |g| = eps * 2^[-3, 3): where eps is added decides the result;
      4    exactly zero at every step (m = v = 0: the update is 0 / eps);
      5    zero at every other step (the moments only decay);
      6    a fixed magnitude from 1e-4 .. 1 whose sign flips every step (m cancels);
      7    as 6 with a magnitude that also changes by a factor 2^[-1, 1)."""
    gc = torch.Generator().manual_seed(2000 + seed)          # per case: classes, fixed magnitudes and signs
    cls = torch.randint(0, 8, (n,), generator=gc)
    base = 10.0 ** (torch.rand(n, generator=gc, dtype=torch.float64) * 4 - 4)
    sign0 = torch.randint(0, 2, (n,), generator=gc).double() * 2 - 1
    gs = torch.Generator().manual_seed(3000 + 17 * seed + s)   # per step
    r = torch.rand(n, generator=gs, dtype=torch.float64)
    sign = torch.randint(0, 2, (n,), generator=gs).double() * 2 - 1
    g = 10.0 ** (r * 14 - 12) * sign
    g = torch.where(cls == 3, eps * 2.0 ** (r * 6 - 3) * sign, g)
    g = torch.where(cls == 4, torch.zeros_like(g), g)
    g = torch.where(cls == 5, g * ((s + 1) % 2), g)
    flip = sign0 * (-1.0) ** s
    g = torch.where(cls == 6, base * flip, g)
    g = torch.where(cls == 7, base * 2.0 ** (r * 2 - 1) * flip, g)
    return g.to(torch.float32)


# (engine-independent) cases: betas, eps, the `step` argument of each call (0 = the library's own count)
CASES = {
    "default-3-steps": dict(betas=(0.9, 0.999), eps=1e-8, steps=(0, 0, 0)),
    "eps-1e-3": dict(betas=(0.9, 0.999), eps=1e-3, steps=(0, 0, 0)),
    "betas-0.8-0.99": dict(betas=(0.8, 0.99), eps=1e-8, steps=(0, 0, 0)),
    "step-1000": dict(betas=(0.9, 0.999), eps=1e-8, steps=(1000, 1001)),
    "step-100000": dict(betas=(0.9, 0.999), eps=1e-3, steps=(100000, 100001)),
}
LR = 1e-4
