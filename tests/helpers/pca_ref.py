"""NumPy restatement of the PCA layer (deephisto_amd/pca.py, dh_embed_scatter, dh_embed_project), in float64.

The error model of the scatter kernel: t = fl(x - mean) is the input (one float32 subtract, done once); an element is a chain of
m = min(n, 1024) fused multiply-adds per chunk and c = ceil(n / 1024) float32 additions of the partials, so to first order
(m + c + 2) u sum |t_a| |t_b|; the gate adds 2 u for the second-order terms, as cluster_ref.gate does.  The projection is one chain of D
fused multiply-adds and one multiply by the scale: (D + 2) u to first order, (D + 4) u the gate."""
import math

import numpy as np

import embed_ref as er

U = 2.0 ** -24      # unit roundoff of float32
CHUNK_ROWS = er.CHUNK_ROWS


def centred(x, mean):
    """float32[n, D]: the one float32 subtract of both kernels."""
    return np.asarray(x, np.float32) - np.asarray(mean, np.float32)[None, :]


def scatter_coeff(n):
    return (min(n, CHUNK_ROWS) + math.ceil(n / CHUNK_ROWS) + 4) * U


def scatter_ref(x, mean):
    """(float64[D, D] scatter of the float32 differences, float64[D, D] gate per element)."""
    t = centred(x, mean).astype(np.float64)
    a = np.abs(t)
    return t.T @ t, scatter_coeff(len(t)) * (a.T @ a)


def project_ref(x, mean, comp, scale=None):
    """(float64[n, K] projection of the float32 differences, float64[n, K] gate per element)."""
    t = centred(x, mean).astype(np.float64)
    c = np.asarray(comp, np.float64)
    s = np.ones(len(c)) if scale is None else np.asarray(scale, np.float64)
    return (t @ c.T) * s[None, :], (t.shape[1] + 4) * U * np.abs(s)[None, :] * (np.abs(t) @ np.abs(c).T)


def mean_ref(x):
    """float32[D]: the mean as PCA.fit forms it: the float32 sums in the order of dh_embed_class_sums (every label 0), divided by n
    in float64, rounded once."""
    sums, _ = er.class_sums_ref(x, np.zeros(len(x), np.int32), 1)
    return (sums[0].astype(np.float64) / len(x)).astype(np.float32)


def fix_signs_ref(v):
    """Rows with their entry of largest magnitude (first index at ties) made positive, written without argmax."""
    out = np.array(v, dtype=np.float64, copy=True)
    for row in out:
        best = 0
        for i in range(1, len(row)):
            if abs(row[i]) > abs(row[best]):
                best = i
        if row[best] < 0:
            row *= -1.0
    return out


STDS = (10.0, 5.0, 2.0)


def planted(n=1030, D=64, seed=11, noise=0.1, offset=20.0):
    """(float32[n, D] rows, float64[3, D] planted orthonormal directions): three directions with standard deviations 10, 5 and 2
    over isotropic noise of 0.1, plus a common offset of +20 per column (the case that matters: a large mean, small detail)."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((D, 3)))
    x = (rng.standard_normal((n, 3)) * np.array(STDS)) @ q.T + noise * rng.standard_normal((n, D)) + offset
    return x.astype(np.float32), q.T.copy()


def pca_ref(x, k):
    """The float64 PCA of the float32 rows `x` and what a float32 fit may differ by.  Returns a dict:
    mean32 (the contract's mean), lam (float64[D] eigenvalues, descending), vec (float64[D, D] rows = eigenvectors under the sign
    rule), trace, E_fro and E_trace (the Frobenius norm and the trace of the covariance error bound E), gap (float64[k]: the
    distance of eigenvalue j to the nearest other eigenvalue).

    E, per element: the scatter gate over (n - 1); plus 2 u |t|^T |t| / (n - 1) for the rounding of the float32 subtract itself
    (the kernel's reference takes t as given, a float64 PCA of the rows does not); plus n / (n - 1) |d| |d|^T for the scatter
    being taken about the float32 mean, d = mean32 - the float64 mean (sum (x - m')(x - m')^T = sum (x - m)(x - m)^T + n d d^T)."""
    x64 = np.asarray(x, np.float64)
    n = len(x64)
    mean32 = mean_ref(x)
    m64 = x64.mean(0)
    t64 = x64 - m64
    cov = t64.T @ t64 / (n - 1)
    lam, vec = np.linalg.eigh(cov)
    lam, vec = lam[::-1].copy(), fix_signs_ref(vec[:, ::-1].T)
    a = np.abs(centred(x, mean32).astype(np.float64))
    d = np.abs(mean32.astype(np.float64) - m64)
    E = (scatter_coeff(n) + 2 * U) * (a.T @ a) / (n - 1) + n / (n - 1) * np.outer(d, d)
    gap = np.array([np.min(np.abs(np.delete(lam, j) - lam[j])) for j in range(k)])
    return dict(mean32=mean32, lam=lam, vec=vec, trace=float(np.trace(cov)), E_fro=float(np.linalg.norm(E)), E_trace=float(np.trace(E)),
                gap=gap)


def footprints(origins, P, d, h, w):
    for y, x in np.asarray(origins, np.int64):
        yield slice(y // d, min((y + P) // d, h // d)), slice(x // d, min((x + P) // d, w // d))


def colour_map_ref(z, origins, P, d, h, w, clip=(1.0, 99.0)):
    """uint8[h // d, w // d, 3] from float64[n, <= 3] per-tile values: per cell the mean over the covering tiles, mapped through
    floor(255 clamp((v - lo) / (hi - lo), 0, 1) + 0.5) with lo, hi the `clip` percentiles of the per-tile values; 128 where hi == lo;
    0 where no tile covers."""
    z = np.asarray(z, np.float64)
    acc = np.zeros((h // d, w // d, z.shape[1]))
    hits = np.zeros((h // d, w // d), np.int64)
    for i, (ys, xs) in enumerate(footprints(origins, P, d, h, w)):
        acc[ys, xs] += z[i]
        hits[ys, xs] += 1
    out = np.zeros((h // d, w // d, 3), np.uint8)
    for ch in range(z.shape[1]):
        lo, hi = np.percentile(z[:, ch], list(clip))
        mean = acc[..., ch] / np.maximum(hits, 1)
        lev = np.full(mean.shape, 128.0) if hi == lo else np.floor(255.0 * np.clip((mean - lo) / (hi - lo), 0.0, 1.0) + 0.5)
        out[..., ch] = np.where(hits > 0, lev, 0).astype(np.uint8)
    return out, hits
