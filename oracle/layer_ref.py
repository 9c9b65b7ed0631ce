"""float64 reference of ONE convolution + epilogue of the inference engines, and the element-wise gate their stored activations are held to
(tests/test_gpu_layer_parity.py; the reference itself is checked by tests/test_layer_reference_host.py).

A layer is  y = conv(x, w) * scale + shift (+ res) (ReLU)  on operands the caller takes from the engine (bf16- or f32-exact inputs,
weights, scale/shift or folded bias, residual).  `conv_epilogue` evaluates it in float64 (exact up to ~1e-16 relative) and returns

  want = y rounded ONCE, round-to-nearest-even, to the engine's storage type (bf16 or f32);
  A    = conv(|x|, |w|) * |scale| + |shift| + |res|: the magnitude the engine's f32 accumulation error scales with.

The gate (`gate_mask`):  |got - want| <= ulp(want) + gamma_K * A,  gamma_K = K u / (1 - K u), u = 2^-24 (f32 accumulation), where K counts
every f32 rounding between the exact operands and the stored value: cin * ks * ks - 1 additions of the dot product, + 1 per product for
the f32 MFMA (bf16 x bf16 products are exact in f32), + the epilogue's multiply and its one or two additions.  gamma_K * A bounds the
distance between the engine's f32 value y_c and y (Higham, Accuracy and Stability, section 3.1); the final rounding of y_c against that
of y contributes at most one unit of the storage format.  ReLU is 1-Lipschitz, and max-pooling of rounded values equals the pooled
rounding, so the same bound holds after either with A max-pooled alongside.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

MANT = {"bf16": 8, "f32": 24}          # significant bits of the storage format
MIN_EXP = -125                          # frexp exponent of the smallest normal of both formats (2^-126 = 0.5 * 2^-125)


def quantum(v: np.ndarray, fmt: str) -> np.ndarray:
    """ulp of float64 values v in format `fmt` (bf16 / f32): 2^(e - p) for v = m 2^e, 0.5 <= |m| < 1; subnormal spacing below, and at
    0 (frexp gives 0 the exponent 0, which would make the unit of an exact zero -- every ReLU-clamped element -- that of 0.5)."""
    v = np.asarray(v, np.float64)
    _, e = np.frexp(v)
    return np.ldexp(1.0, np.maximum(np.where(v == 0, MIN_EXP, e), MIN_EXP) - MANT[fmt])


def round_to(v: np.ndarray, fmt: str) -> np.ndarray:
    """float64 -> the nearest value of `fmt`, ties to even, in ONE rounding (torch's float64 -> bfloat16 cast goes through float32)."""
    v = np.asarray(v, np.float64)
    q = quantum(v, fmt)
    return np.rint(v / q) * q


def conv_epilogue(x, w, scale, shift, stride: int, res=None, relu: bool = True, pool: bool = False, fmt: str = "bf16",
                  exact: bool = False):
    """x [N][cin][H][W], w [cout][cin][ks][ks], scale / shift [cout], res like the output (or None); all taken as float64.
    pool: the fused stem's max-pool 3x3/2/1 after the ReLU.  Returns (want, A) as float64 numpy arrays; exact=True returns the unrounded
    float64 value instead of `want` (the composition test)."""
    d = lambda t: torch.as_tensor(np.asarray(t), dtype=torch.float64)  # noqa: E731
    x, w, sc, sh = d(x), d(w), d(scale)[None, :, None, None], d(shift)[None, :, None, None]
    ks = w.shape[-1]
    y = F.conv2d(x, w, None, stride, ks // 2) * sc + sh
    a = F.conv2d(x.abs(), w.abs(), None, stride, ks // 2) * sc.abs() + sh.abs()
    if res is not None:
        r = d(res)
        y, a = y + r, a + r.abs()
    if relu:
        y = F.relu(y)
    y = y.numpy()
    if not exact:
        y = round_to(y, fmt)
    if pool:
        y = F.max_pool2d(torch.from_numpy(y), 3, 2, 1).numpy()
        a = F.max_pool2d(a, 3, 2, 1)
    return y, a.numpy()


def conv_dgrad(dz, w, stride: int, Hi: int, Wi: int, res=None, fmt: str = "bf16", exact: bool = False):
    """Data gradient of y = conv(x, w) (pad ks // 2) in float64: dz [N][cout][Ho][Wo], w [cout][cin][ks][ks], res (the gradient joining
    from another branch) [N][cin][Hi][Wi] or None.  Hi x Wi is the convolution's INPUT size: at stride 2 an even map and an odd one
    give the same Ho, and the transposed convolution needs the output padding that tells them apart.  Returns (want, A):

      want = conv_transpose(dz, w) (+ res) rounded ONCE to `fmt` (exact=True: the unrounded float64 value);
      A    = conv_transpose(|dz|, |w|) (+ |res|).

    The contraction runs over cout * ks * ks terms: K of the gate is rounding_count(cout, ks, fmt, res is not None) -- the engine's
    multiply by ones and add of zeros are exact and stay under the two roundings that count keeps for the epilogue."""
    d = lambda t: torch.as_tensor(np.asarray(t), dtype=torch.float64)  # noqa: E731
    dz, w = d(dz), d(w)
    ks, pad = w.shape[-1], w.shape[-1] // 2
    Ho, Wo = (Hi + 2 * pad - ks) // stride + 1, (Wi + 2 * pad - ks) // stride + 1
    assert tuple(dz.shape[2:]) == (Ho, Wo), f"dz is {tuple(dz.shape[2:])}, the conv of a {Hi} x {Wi} map gives {Ho} x {Wo}"
    op = (Hi - ((Ho - 1) * stride - 2 * pad + ks), Wi - ((Wo - 1) * stride - 2 * pad + ks))   # rows / columns no output pixel reaches from
    y = F.conv_transpose2d(dz, w, None, stride, pad, output_padding=op)
    a = F.conv_transpose2d(dz.abs(), w.abs(), None, stride, pad, output_padding=op)
    if res is not None:
        r = d(res)
        y, a = y + r, a + r.abs()
    y = y.numpy()
    return (y if exact else round_to(y, fmt)), a.numpy()


def stored_product_sum(prod, res, fmt: str = "bf16") -> np.ndarray:
    """The value the accumulate contract DEFINES for an exact product: the product is stored in `fmt`, then added to `res` (None: zero)
    and stored again -- round(res + round(prod)), two roundings of exact float64 values."""
    t = round_to(prod, fmt)
    return t if res is None else round_to(np.asarray(res, np.float64) + t, fmt)


def stored_product_gate_mask(got, want, A, K: int, prod, A_prod, fmt: str = "bf16") -> np.ndarray:
    """Gate of a data gradient that reaches memory in TWO stored roundings (the strided 1x1 convolution of a downsample branch: the
    low-resolution product goes to bf16 scratch, then it is added into dX, which already holds the other branch's gradient `res`).

    With p the exact product, p_c the engine's f32 accumulation of it, T = rn(p_c) the stored product, s = fl32(res + T) and
    got = rn(s), against y = res + p and want = rn(y):

      |p_c - p|       <= gamma_{cout - 1} A_prod                               (f32 dot product of exact bf16 x bf16 products)
      |T - p_c|       <= ulp(p_c) / 2 <= quantum(|p| + gamma_K A_prod) / 2     (the extra stored rounding; quantum is monotone)
      |s - (res + T)| <= u (|res| + |T|) <= 2 u (|res| + A_prod)               (|T| <= |p| (1 + 2^-8) + gamma_K A_prod <= 2 A_prod)

    so |s - y| <= gamma_K A + quantum(|p| + gamma_K A_prod) / 2 with A = A_prod + |res| and K = rounding_count(cout, 1, fmt, True) =
    (cout - 1) + 3: the dot product's additions, and three for the one f32 addition (bounded by 2 u above; the GEMM has no other
    epilogue arithmetic).  The final rounding of s against that of y adds at most one unit of the format, as in `gate_mask`:

      |got - want| <= ulp(want) + gamma_K A + quantum(|p| + gamma_K A_prod) / 2.

    `prod`, `A_prod`: conv_dgrad(..., res=None, exact=True) of the same operands; want, A: conv_dgrad with res."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    g = gamma(K)
    extra = 0.5 * quantum(np.abs(np.asarray(prod, np.float64)) + g * np.asarray(A_prod, np.float64), fmt)
    return np.abs(got - want) <= quantum(want, fmt) + g * np.asarray(A, np.float64) + extra


def gamma(K: int) -> float:
    u = 2.0 ** -24
    return K * u / (1 - K * u)


def rounding_count(cin: int, ks: int, fmt: str, res: bool) -> int:
    """K of the gate: the dot product's additions (+ its rounded products in f32), the epilogue's multiply and additions."""
    k = cin * ks * ks
    return (k - 1) + (k if fmt == "f32" else 0) + 2 + (1 if res else 0)


def gate_mask(got, want, A, K: int, fmt: str) -> np.ndarray:
    """True where an element passes |got - want| <= ulp(want) + gamma_K * A."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want) <= quantum(want, fmt) + gamma(K) * np.asarray(A, np.float64)


def fold_bn(w, gamma_, beta, mean, var, eps: float = 1e-5):
    """Eval BN folded in float64: (w * s, beta - mean * s), s = gamma / sqrt(var + eps)."""
    f = lambda t: np.asarray(t, np.float64)  # noqa: E731
    s = f(gamma_) / np.sqrt(f(var) + eps)
    return f(w) * s.reshape(-1, *([1] * (np.ndim(w) - 1))), f(beta) - f(mean) * s


def bn_scale_shift(gamma_, beta, mean, var, eps: float = 1e-5):
    """Eval BN as float64 scale / shift (the unfolded engines' epilogue)."""
    f = lambda t: np.asarray(t, np.float64)  # noqa: E731
    s = f(gamma_) / np.sqrt(f(var) + eps)
    return s, f(beta) - f(mean) * s


def topology(model) -> list[dict]:
    """The convs of oracle.resnet18 / oracle.resnet50 in launch order, each with the stored activation it reads (`src`: "input" for the
    stem, else a conv name or "maxpool") and the one it adds (`res`, or None): {name, bn, src, res, stride, relu}."""
    out = [dict(name="conv1", bn="bn1", src="input", res=None, stride=2, relu=True)]
    prev = "maxpool"
    for li in range(1, 5):
        for bi, blk in enumerate(getattr(model, f"layer{li}")):
            pre = f"layer{li}.{bi}"
            chain = [c for c in ("conv1", "conv2", "conv3") if hasattr(blk, c)]
            idt = prev
            src = prev
            for c in chain[:-1]:
                out.append(dict(name=f"{pre}.{c}", bn=f"{pre}.bn{c[-1]}", src=src, res=None, stride=getattr(blk, c).stride[0], relu=True))
                src = f"{pre}.{c}"
            if blk.downsample is not None:
                idt = f"{pre}.downsample.0"
                out.append(dict(name=idt, bn=f"{pre}.downsample.1", src=prev, res=None, stride=blk.downsample[0].stride[0], relu=False))
            last = chain[-1]
            out.append(dict(name=f"{pre}.{last}", bn=f"{pre}.bn{last[-1]}", src=src, res=idt, stride=getattr(blk, last).stride[0], relu=True))
            prev = f"{pre}.{last}"
    return out


def compose(model, x) -> tuple[dict, np.ndarray]:
    """The whole network layer by layer through conv_epilogue in float64 WITHOUT rounding (unfolded eval BN as scale / shift): the stored
    activations by name and the logits of fc(avgpool(last)).  Equals model.double()(x) up to float64 summation order."""
    sd = {k: v.detach().double().numpy() for k, v in model.state_dict().items()}
    acts = {"input": np.asarray(x, np.float64)}
    for L in topology(model):
        sc, sh = bn_scale_shift(sd[L["bn"] + ".weight"], sd[L["bn"] + ".bias"], sd[L["bn"] + ".running_mean"], sd[L["bn"] + ".running_var"])
        acts[L["name"]], _ = conv_epilogue(acts[L["src"]], sd[L["name"] + ".weight"], sc, sh, L["stride"],
                                           acts[L["res"]] if L["res"] else None, L["relu"], exact=True)
        if L["name"] == "conv1":
            acts["maxpool"] = F.max_pool2d(torch.from_numpy(acts["conv1"]), 3, 2, 1).numpy()
    last = acts[topology(model)[-1]["name"]]
    return acts, head(last, sd["fc.weight"], sd["fc.bias"])


def head(last, fc_w, fc_b) -> np.ndarray:
    """float64 fc(avgpool(last)) of a stored activation [N][C][H][W]."""
    return np.asarray(last, np.float64).mean(axis=(2, 3)) @ np.asarray(fc_w, np.float64).T + np.asarray(fc_b, np.float64)
