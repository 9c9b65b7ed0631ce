"""float64 reference of the bf16 training engine's batch-norm and pooling passes, and the element-wise gates their outputs are held to
(tests/test_gpu_bn_bf16_parity.py; the reference itself, a float32 emulation of the kernels and a set of planted errors are checked on the
CPU by tests/test_bn_reference_host.py).  The gate is layer_ref's:  |got - want| <= ulp(want) + gamma_K * A,  u = 2^-24.

The ELEMENTWISE passes are referenced from the statistics the kernel under test returned: its float32 mean, invstd, dgamma and dbeta are
taken as exact float64 inputs, so a gate holds only the roundings of the pass it judges.  The statistics keep gates of their own against
float64 sums over the whole tensor (`column_stats`, `column_grad_sums`).

Forward (bn2_apply_kernel, bn2_fold_apply_kernel).  pre = z sc + sh (+ res), sc = gamma invstd, sh = beta - mean sc, want = rn_bf16(relu(pre)).
The kernel makes sc_c = fl(gamma invstd) [1 rounding], sh_c = fl(beta - fl(mean sc_c)) [2; 1 if the compiler contracts it into an fma],
v = fma(z, sc_c, sh_c) [1] and v + res [1].  Every term of pre therefore carries a product of at most five factors (1 + d), |d| <= u:
  |v - pre| <= gamma_5 A,   A = |z sc| + |mean sc| + |beta| + |res|,   K_FWD = 5.
A keeps |z sc| and |mean sc| apart, so the cancellation of a channel whose mean is many standard deviations (or whose variance is 0,
invstd = 1 / sqrt(eps)) is in the gate.  ReLU is 1-Lipschitz; the stored rounding of v against that of pre adds one unit of bf16.

Join (bn2_apply_join_kernel).  y = relu(bn(z) + r), r = rn_bf16(bn_ds(z2)) made on the fly.  With p = z2 sc2 + sh2 exact, p_c the kernel's
float32 value (|p_c - p| <= gamma_4 A2 <= gamma_K A2, A2 = |z2 sc2| + |mean2 sc2| + |beta2|), the stored rounding moves r by at most
ulp(p_c) / 2 <= quantum(|p| + gamma_K A2) / 2, exactly the extra term of layer_ref.stored_product_gate_mask:
  |got - want| <= ulp(want) + gamma_5 (A1 + A2) + quantum(|p| + gamma_5 A2) / 2,   want = rn_bf16(relu(bn(z) + p)).
The identical fraction is taken against the value the two stored roundings define, rn_bf16(relu(bn(z) + rn_bf16(p))) (`stored`).

Backward (bn2_bwd_apply_kernel, bn2_fold_bwd_apply_kernel, bn2_pool_bwd_apply_kernel).  With a = gamma invstd and n rows
  dz = a g - (a / n) dbeta - (a invstd / n) dgamma (z - mean)  =  k0 g + k1 z + k2,
  k0 = a,  k1 = -a invstd dgamma / n,  k2 = -a dbeta / n - k1 mean.
The kernels make the coefficients in double from the DOUBLE column sums s1, s2 and round each once to float32 [3 roundings]; the reference
reads dbeta = fl(s1), dgamma = fl(s2) instead [2]; dz_c = fma(k0, g, fma(k1, z, k2)) [2].  No single term meets more than four of them
(k1 z: dgamma, k1, two fmas; the parts of k2 likewise; k0 g: k0 and one fma), so gamma_4 would do; K_BWD = 8 counts every rounding named
above once plus one spare for the double arithmetic, and is what the gate uses:
  |dz_c - dz| <= gamma_8 A,   A = |k0 g| + |k1 z| + |a dbeta / n| + |k1 mean|.
A holds k1 z and k1 mean apart: that is the cancellation of the projection terms.  The stem's fused tail gathers g from up to four
pooled gradients in float32 (three additions): K_POOL_BWD = K_BWD + 3 with |k0| sum|terms| in A.

ReLU masks.  Mode 1 (pattern from the kernel's own stored y > 0) is exact.  Mode 0 takes dy as it comes (pre-masked by the caller).  Mode 2
recomputes fma(z, sc_c, sh_c) > 0: the reference uses pre > 0 and an element with |pre| <= gamma_5 A is UNDECIDED -- either pattern is a
correct float32 answer there -- and is left out of the dz gate (`undecided`); a case may hold at most UNDECIDED_CAP of them.

Pool (bn2_apply_pool_kernel, maxpool2_fwd_idx_kernel).  r = rn_bf16(relu(pre)) per element; pooled value and FIRST-maximum position
(row-major over the in-bounds 3x3/2 window, strict >) are computed here in numpy.  An element is UNSAFE where pre lies within gamma_5 A of
a bf16 rounding midpoint or of zero (there the kernel's stored value may differ by a unit, which can move a maximum or make or break a
tie); a window with an unsafe element is undecided.  Every decided window must match in pooled bits AND position; every window must pass
the value gate with A max-pooled alongside; at most WINDOW_CAP of a case's windows may be undecided (expected: about 9 * 2^-13, nine
elements a window, each near a midpoint with probability 2 gamma_5 A / ulp ~ 2^-13 at |z sc| ~ 8 |pre|).  The backward reference scatters
the pooled gradient to the REFERENCE's positions.

Identical fraction.  got == want bit for bit is asked of at least 0.999 of ALL referenced elements of an output, as for every other
tensor of the engine (a float32 value within gamma_K A of the exact one rounds to another bf16 value with a probability of about
gamma_K A / ulp(want), a few 1e-4 even on the channels whose mean is 8 standard deviations).  Exempt, by name and by construction only:
every output of a map of ONE or TWO rows (variance 0, or xhat = +-1: y is what z sc - mean sc leaves at an invstd of up to 1 / sqrt(eps),
and dz is identically 0 in exact arithmetic, so the stored value is rounding noise), and the FORWARD output of the constant channel
(|z sc| = |gamma z| / sqrt(eps), several hundred times the result beta + res).  Those stay under the gate (bn_cases._exempt).

Channel sums (dgamma = sum g xhat, dbeta = sum g over the rows of a channel).  float32 terms added in some order, partial sums in float32,
then double: any order of the rows - 1 additions satisfies |got - want| <= gamma_{rows - 1} sum|terms| (Higham, section 4.2); a term
fl(g fl(fl(z - mean) invstd)) carries three roundings of its own and the float32 result one more, hence gamma_{rows + 3} (at rows = 1
the sum has no addition at all and gamma_rows alone would not cover the term).  Undecided elements may be in or out of the sum, which adds
their |g xhat| (|g|) to the bound (`channel_sum_ratio`).
"""
from __future__ import annotations

import numpy as np

from oracle.layer_ref import gamma, gate_mask, quantum, round_to

K_FWD = 5
K_BWD = 8
K_POOL_BWD = K_BWD + 3
K_POOL_DX = 3                # stand-alone max-pool backward: at most four bf16 terms added in float32
UNDECIDED_CAP = 1e-4         # mode-2 elements whose ReLU pattern float32 cannot decide, as a share of a case's elements
WINDOW_CAP = 1e-2            # pool windows holding an unsafe element, as a share of a case's windows
EPS = float(np.float32(1e-5))  # BN_EPS of the engine (a float32 constant)

f64 = lambda t: np.asarray(t, np.float64)  # noqa: E731


def column_stats(z, chunk: int = 4096):
    """float64 mean and biased variance of every column of z [rows][C] (two passes, in row chunks)."""
    n = z.shape[0]
    s = np.zeros(z.shape[1])
    for i in range(0, n, chunk):
        s += f64(z[i:i + chunk]).sum(0)
    mu = s / n
    v = np.zeros(z.shape[1])
    for i in range(0, n, chunk):
        v += ((f64(z[i:i + chunk]) - mu) ** 2).sum(0)
    return mu, v / n


def coefficients(gamma_, beta, mean, invstd):
    sc = f64(gamma_) * f64(invstd)
    return sc, f64(beta) - f64(mean) * sc


def forward(z, gamma_, beta, mean, invstd, res=None):
    """(pre, A) of pre = z sc + sh (+ res), before the ReLU and unrounded; z, res [..., C]."""
    sc, sh = coefficients(gamma_, beta, mean, invstd)
    z = f64(z)
    pre = z * sc + sh
    A = np.abs(z * sc) + np.abs(f64(mean) * sc) + np.abs(f64(beta))
    if res is not None:
        pre, A = pre + f64(res), A + np.abs(f64(res))
    return pre, A


def stored(pre, relu: bool = True):
    return round_to(np.maximum(pre, 0.0) if relu else pre, "bf16")


def forward_ok(got, pre, A, relu: bool = True):
    return gate_mask(got, stored(pre, relu), A, K_FWD, "bf16")


def gate_width(want, A, K: int, extra=0.0):
    return quantum(want, "bf16") + gamma(K) * f64(A) + extra


def join(z, p1, z2, p2):
    """The join of a downsample block; p1 / p2 = (gamma, beta, mean, invstd) of the top / branch BN.  Returns want (one rounding of the
    exact value), A, extra (the inner stored rounding's share of the gate) and stored (the value of the two stored roundings)."""
    pre1, A1 = forward(z, *p1)
    p, A2 = forward(z2, *p2)
    extra = 0.5 * quantum(np.abs(p) + gamma(K_FWD) * A2, "bf16")
    return stored(pre1 + p), A1 + A2, extra, stored(pre1 + round_to(p, "bf16"))


def backward(z, g, gamma_, mean, invstd, dgamma, dbeta, n: int, g_terms=None):
    """(dz, A) unrounded of dz = k0 g + k1 z + k2; g = the masked gradient [..., C] (float64), g_terms = sum|terms| of g where g itself is a
    float32 sum (the pool's gather), else |g|."""
    a = f64(gamma_) * f64(invstd)
    k1 = -a * f64(invstd) * f64(dgamma) / n
    kb = -a * f64(dbeta) / n
    z, g = f64(z), f64(g)
    dz = a * g + k1 * z + (kb - k1 * f64(mean))
    A = np.abs(a) * (np.abs(g) if g_terms is None else f64(g_terms)) + np.abs(k1 * z) + np.abs(kb) + np.abs(k1 * f64(mean))
    return dz, A


def undecided(pre, A):
    return np.abs(pre) <= gamma(K_FWD) * A


def unsafe(pre, A):
    """Elements whose stored bf16 value float32 arithmetic cannot decide: pre within gamma_5 A of zero or of a rounding midpoint."""
    tol = gamma(K_FWD) * A
    q = quantum(pre, "bf16")
    t = pre / q
    mid = np.abs(t - np.floor(t) - 0.5) * q
    return (np.abs(pre) <= tol) | ((pre > 0) & (mid <= tol))


def _padded(x, fill):
    B, H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    P = np.full((B, 2 * Ho + 1, 2 * Wo + 1, C), fill, x.dtype)
    P[:, 1:H + 1, 1:W + 1] = x
    return P, Ho, Wo


def pool(r):
    """3x3 / 2 pad 1 max-pool of r [B][H][W][C]: (pooled, pos), pos = dyy * 3 + dxx of the FIRST maximum in row-major window order."""
    P, Ho, Wo = _padded(f64(r), -np.inf)
    best = np.full((r.shape[0], Ho, Wo, r.shape[3]), -np.inf)
    pos = np.zeros(best.shape, np.uint8)
    for k in range(9):
        v = P[:, k // 3:k // 3 + 2 * Ho:2, k % 3:k % 3 + 2 * Wo:2]
        m = v > best
        best = np.where(m, v, best)
        pos[m] = k
    return best, pos


def pool_any(flag):
    P, Ho, Wo = _padded(np.asarray(flag, bool), False)
    out = np.zeros((flag.shape[0], Ho, Wo, flag.shape[3]), bool)
    for k in range(9):
        out |= P[:, k // 3:k // 3 + 2 * Ho:2, k % 3:k % 3 + 2 * Wo:2]
    return out


def pool_max(A):
    return pool(A)[0]


def pool_scatter(dpool, pos, H: int, W: int, absolute: bool = False):
    """The max-pool's gradient: dpool [B][Ho][Wo][C] added at the positions `pos` into a [B][H][W][C] map (absolute: sum of |terms|)."""
    d = np.abs(f64(dpool)) if absolute else f64(dpool)
    B, Ho, Wo, C = d.shape
    P = np.zeros((B, 2 * Ho + 1, 2 * Wo + 1, C))
    for k in range(9):
        P[:, k // 3:k // 3 + 2 * Ho:2, k % 3:k % 3 + 2 * Wo:2] += np.where(pos == k, d, 0.0)
    return P[:, 1:H + 1, 1:W + 1]


def window_cover(win_flag, H: int, W: int):
    """Pixels [B][H][W][C] that lie under a flagged window."""
    B, Ho, Wo, C = win_flag.shape
    P = np.zeros((B, 2 * Ho + 1, 2 * Wo + 1, C), bool)
    for k in range(9):
        P[:, k // 3:k // 3 + 2 * Ho:2, k % 3:k % 3 + 2 * Wo:2] |= win_flag
    return P[:, 1:H + 1, 1:W + 1]


def pack_bits(y_bits):
    """The ReLU pattern bytes of stored bf16 bits y_bits [rows][C] (uint16): bit e of byte [row][c / 8] set where value 8 (c / 8) + e is
    non-zero (either sign of zero counts as zero)."""
    nz = (np.asarray(y_bits, np.uint16) & 0x7FFF) != 0
    return np.packbits(nz.reshape(nz.shape[0], -1, 8), axis=-1, bitorder="little")[..., 0]


def column_grad_sums(z, g, mean, invstd, loose=None, chunk: int = 4096):
    """float64 sums over the rows of g and g xhat (xhat from the given mean / invstd), of their absolute terms, of g z (to re-centre the
    sums on other statistics), and of m, m |xhat| for `loose` = m, the gradient magnitude an undecided element may gain or lose (0 where
    the element is decided).  Row chunks: the largest case is 33 M elements."""
    C = z.shape[1]
    out = {k: np.zeros(C) for k in ("g", "gx", "abs_g", "abs_gx", "gz", "loose_g", "loose_gx")}
    mean, invstd = f64(mean), f64(invstd)
    for i in range(0, z.shape[0], chunk):
        zz, gg = f64(z[i:i + chunk]), f64(g[i:i + chunk])
        xh = (zz - mean) * invstd
        gx = gg * xh
        out["g"] += gg.sum(0); out["gx"] += gx.sum(0); out["gz"] += (gg * zz).sum(0)
        out["abs_g"] += np.abs(gg).sum(0); out["abs_gx"] += np.abs(gx).sum(0)
        if loose is not None:
            lo = f64(loose[i:i + chunk])
            out["loose_g"] += lo.sum(0); out["loose_gx"] += (lo * np.abs(xh)).sum(0)
    return out


def channel_sum_ratio(got, want, abs_terms, loose, rows: int):
    """|got - want| / (gamma_{rows + 3} sum|terms| + the undecided elements' terms), per channel; <= 1 passes."""
    bound = gamma(rows + 3) * f64(abs_terms) + f64(loose)
    return np.abs(f64(got) - f64(want)) / np.maximum(bound, 1e-300)
