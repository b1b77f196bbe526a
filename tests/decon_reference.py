"""The yardstick of the multi-view deconvolution tests: a NumPy fp64 restatement of the recipe in include/mvsim.h, a float32
restatement of its two elementwise steps, and the cases the tests share.  Nothing here touches the GPU or the library.

    conv(a, P)[i] = sum_k P[k] a_mirror[i - (k - K/2)]          mirror-single extension, centre K/2, no flip
    for iteration, for view v (psi updated after every view):
        b = conv(psi, P_v);  r = phi_v / max(b, eps);  c = conv(r, F_v)  with  c[i] = sum_k P_v[k] r_mirror[i + (k - K/2)]
        n = psi c;  lambda > 0: n = (sqrt(1 + 2 lambda n) - 1) / lambda;  n NaN or < min_value: n = min_value
        psi = n   or   psi + w_v (n - psi)

Arrays are (Nz, Ny, Nx) like everywhere in the package; extents quoted as (x, y, z) in the issue are reversed here."""
import math

import numpy as np
from scipy.signal import fftconvolve

F32 = np.float32
F64 = np.float64


# ------------------------------------------------------------------------------------------------ fp64 recipe
def normalise(psf):
    """Tools.normImage as the library applies it to its copy: fp64 sum, (float)(v / sum)."""
    p = np.ascontiguousarray(psf, dtype=F32)
    s = math.fsum(p.ravel().tolist())
    return (p.astype(F64) / s).astype(F32)


def conv64(a, psf):
    """The convolution by its formula: mirror pad of K-1-K/2 before and K/2 behind the image, then a 'valid' FFT convolution."""
    k = psf.shape
    pad = [(kk - 1 - kk // 2, kk // 2) for kk in k]
    ext = np.pad(np.asarray(a, dtype=F64), pad, mode="reflect")
    return fftconvolve(ext, np.asarray(psf, dtype=F64), mode="valid")


def flip_psf(psf):
    """F[j] = P[K-1-j] per axis; one leading zero tap on every axis of even extent."""
    f = np.asarray(psf)[::-1, ::-1, ::-1]
    return np.pad(f, [((0 if kk & 1 else 1), 0) for kk in f.shape], mode="constant")


def corr_literal(r, psf):
    """c[i] = sum_k P[k] r_mirror[i + (k - K/2)], term by term (small cases only)."""
    r = np.asarray(r, dtype=F64)
    kz, ky, kx = psf.shape
    pad = [(kk // 2, kk - 1 - kk // 2) for kk in psf.shape]
    ext = np.pad(r, pad, mode="reflect")
    out = np.zeros(r.shape, dtype=F64)
    nz, ny, nx = r.shape
    for z in range(kz):
        for y in range(ky):
            for x in range(kx):
                out += float(psf[z, y, x]) * ext[z:z + nz, y:y + ny, x:x + nx]
    return out


def start_value(views, init_value, min_value):
    if init_value > 0:
        v = F32(init_value)
    else:
        v = F32(sum(math.fsum(np.asarray(p, dtype=F64).ravel().tolist()) / p.size for p in views) / len(views))
    return max(v, F32(min_value))


def deconvolve64(views, psfs, weights=None, iterations=3, init_value=0.0, min_value=1e-4, eps=1e-6, lam=0.0, psi0=None,
                 mistake=None, perturb=None):
    """The recipe in fp64 (the PSFs normalised to float first, as the library does).  Returns the estimates [start, after
    iteration 0, ...].  ``mistake``: one of the deliberate errors of the sensitivity test.  ``perturb(x)``: applied to every
    convolution's result (the error-propagation figure of the tolerance's derivation)."""
    min_value, eps = float(F32(min_value)), float(F32(eps))
    ps = [normalise(p).astype(F64) for p in psfs]
    fs = [p if mistake == "no_flip" else flip_psf(p) for p in ps]
    order = list(range(len(views)))
    if mistake == "reversed":
        order.reverse()
    psi = np.full(views[0].shape, float(start_value(views, init_value, min_value)), dtype=F64) if psi0 is None else np.asarray(psi0, dtype=F64).copy()
    out = [psi.copy()]
    cv = (lambda a, p: perturb(conv64(a, p))) if perturb else conv64
    for _ in range(iterations):
        base = psi.copy()
        for v in order:
            src = base if mistake == "simultaneous" else psi
            b = cv(src, ps[v])
            r = np.asarray(views[v], dtype=F64) / np.fmax(b, eps)
            c = cv(r, fs[v])
            n = src * c
            if lam > 0 and mistake != "no_lambda":
                with np.errstate(invalid="ignore"):
                    n = (np.sqrt(1.0 + 2.0 * lam * n) - 1.0) / lam
            if mistake != "no_floor":
                n = np.where(np.isnan(n) | (n < min_value), min_value, n)
            if weights is None or mistake == "no_weights":
                psi = n
            else:
                psi = psi + np.asarray(weights[v], dtype=F64) * (n - psi)
        out.append(psi.copy())
    return out


def nrmse(est, truth):
    """Root mean square error after the least-squares scale of ``est`` onto ``truth``, over the range of ``truth``."""
    e = np.asarray(est, dtype=F64).ravel()
    t = np.asarray(truth, dtype=F64).ravel()
    s = float(e @ t) / float(e @ e)
    return float(np.sqrt(np.mean((s * e - t) ** 2)) / (t.max() - t.min()))


def range_err(a, ref):
    ref = np.asarray(ref, dtype=F64)
    return float(np.max(np.abs(np.asarray(a, dtype=F64) - ref)) / (ref.max() - ref.min()))


# ------------------------------------------------------------------------------------------------ float32 steps
def ratio32(phi, b, eps):
    """Step 2 in float32: one division; fmax drops a NaN b."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        return (np.asarray(phi, F32) / np.fmax(np.asarray(b, F32), F32(eps))).astype(F32)


def update32(psi, c, w, min_value, lam):
    """Step 4 in float32 (the Tikhonov term in fp64), every operation rounded on its own.  Returns (new psi, n_floored,
    max |new - old| as float with NaN differences dropped)."""
    psi = np.asarray(psi, F32)
    mv = F32(min_value)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        n = (psi * np.asarray(c, F32)).astype(F32)
        if lam > 0:
            t = F64(2.0) * F64(lam)
            n = ((np.sqrt(F64(1.0) + t * n.astype(F64)) - F64(1.0)) / F64(lam)).astype(F32)
        fl = ~(n >= mv)
        n = np.where(fl, mv, n).astype(F32)
        if w is not None:
            d = (n - psi).astype(F32)
            t = (np.asarray(w, F32) * d).astype(F32)
            n = (psi + t).astype(F32)
        change = np.abs((n - psi).astype(F32))
        mc = F32(np.fmax.reduce(change, initial=F32(0))) if not np.all(np.isnan(change)) else F32(0)
    return n, int(np.count_nonzero(fl)), mc


def same_bits(a, b):
    """Bit for bit, with every NaN equal to every NaN (a NaN's sign and payload are the hardware's choice)."""
    a = np.ascontiguousarray(a, dtype=F32).ravel()
    b = np.ascontiguousarray(b, dtype=F32).ravel()
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


# ------------------------------------------------------------------------------------------------ the cases
def skewed_psf(shape_zyx, seed=0):
    """An asymmetric PSF: a Gaussian times a ramp along every axis, so that a missing flip shows."""
    ax = []
    for i, k in enumerate(shape_zyx):
        x = np.arange(k, dtype=F64) - k // 2
        g = np.exp(-0.5 * (x / max(0.8, 0.22 * k)) ** 2) * (1.0 + (0.7 - 0.1 * ((i + seed) % 3)) * x / max(1.0, k / 2.0))
        ax.append(np.maximum(g, 0.02))
    return (ax[0][:, None, None] * ax[1][None, :, None] * ax[2][None, None, :]).astype(F32)


def box_phantom(shape_zyx, peak=40.0, background=0.05):
    nz, ny, nx = shape_zyx
    p = np.full(shape_zyx, background, dtype=F64)
    p[nz // 4: nz - nz // 3, ny // 4: ny - ny // 4, nx // 3: nx - nx // 5] = peak
    p[nz // 2:, ny // 2: ny // 2 + max(2, ny // 6), nx // 8: nx // 4] = 0.6 * peak
    return p


STD_SHAPE = (12, 20, 24)                                  # dim (24, 20, 12) as x, y, z
STD_PSF_SHAPES = ((5, 7, 9), (9, 7, 5), (5, 9, 7))        # (9,7,5), (5,7,9), (7,9,5) as x, y, z
STD_MIN_VALUE = 1.0                                       # 2.5 % of the phantom's peak: high enough that omitting the floor shows
STD_EPS = 1e-6
TOL = 1e-4                                                # of the fp64 result's range


def make_case(shape_zyx=STD_SHAPE, psf_shapes=STD_PSF_SHAPES, seed=20260101, ones=False):
    """Views: Poisson counts of the blurred box phantom; weights: random in [0, 1] with 10 % exact zeros and one slab of ones
    (``ones``: all ones).  Deterministic."""
    rng = np.random.default_rng(seed)
    truth = box_phantom(shape_zyx)
    psfs = [skewed_psf(s, i) for i, s in enumerate(psf_shapes)]
    views = [rng.poisson(np.maximum(conv64(truth, normalise(p)), 0.0)).astype(F32) for p in psfs]
    weights = []
    for _ in psfs:
        w = rng.random(shape_zyx).astype(F32)
        w[rng.random(shape_zyx) < 0.1] = 0.0
        w[shape_zyx[0] // 2] = 1.0
        weights.append(np.ones(shape_zyx, F32) if ones else w)
    return {"truth": truth, "psfs": psfs, "views": views, "weights": weights}
