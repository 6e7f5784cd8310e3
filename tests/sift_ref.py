"""NumPy restatement of OpenCV 4.x ``SIFT_create(nfeatures=0, nOctaveLayers=3, contrastThreshold=0.001, edgeThreshold=80,
sigma=1.6).detect(img)`` (utils/common.py:838-857 of the reference), the yardstick of gims_amd/csrc/sift.hip.

Every float operation is float32 in the order gims_amd/csrc/sift.hip performs it (no fused multiply-add), so the pyramid is
bit-identical and keypoints differ only where a transcendental (exp, pow) differs by an ulp.  DESIGN.md 4.8 lists the
constants and the choices this restatement makes where OpenCV's order depends on its SIMD / IPP build.

``detect(img)`` returns a dict of arrays (pt [n, 2], size, angle, response, octave) in OpenCV's output order, plus
``margin``: for each keypoint the smallest relative slack of the decisions that admitted it (contrast, edge ratio, peak
ratio, Newton convergence).  A keypoint that one implementation keeps and the other drops must have a small margin.
"""
from __future__ import annotations

import math

import numpy as np

N_LAYERS = 3
SIGMA = 1.6
CONTRAST = 0.001
EDGE = 80.0
IMG_BORDER = 5
MAX_STEPS = 5
ORI_BINS = 36
ORI_SIG = 1.5
ORI_RADIUS = 4.5
ORI_PEAK = 0.8
F = np.float32


def n_octaves(h, w):
    return int(round_half_even(math.log(min(2 * w, 2 * h)) / math.log(2.0) - 2)) + 1


def round_half_even(x):
    return float(np.rint(x))


def blur_ksize(sig):
    return int(round_half_even(sig * 8 + 1)) | 1


def layer_sigmas():
    """sig[0] = sigma (only the first octave's initial blur uses sig_diff instead), sig[i] the incremental blur of layer i."""
    sig = [SIGMA]
    k = 2.0 ** (1.0 / N_LAYERS)
    for i in range(1, N_LAYERS + 3):
        prev = k ** (i - 1) * SIGMA
        tot = prev * k
        sig.append(math.sqrt(tot * tot - prev * prev))
    return sig


def init_sigma():
    return float(np.sqrt(max(F(SIGMA) * F(SIGMA) - F(0.5) * F(0.5) * F(4), F(0.01))))


def gaussian_kernel(n, sigma):
    """getGaussianKernelBitExact (double, symmetric), cast to float32."""
    scale2x = -0.5 * 0.25 / (sigma * sigma)
    n2 = (n - 1) // 2
    vals, s = [], 0.0
    for i, x in zip(range(n2), range(1 - n, 0, 2)):
        t = math.exp(float(x * x) * scale2x)
        vals.append(t)
        s += t
    s = s * 2 + 1.0
    mul = 1.0 / s
    out = np.empty(n, np.float64)
    for i in range(n2):
        out[i] = out[n - 1 - i] = vals[i] * mul
    out[n2] = mul
    return out.astype(np.float32)


def layout(h, w):
    """What gims_sift_layout reports: per octave (h, w); per level blur sigma and kernel size (level 0 of octave 0: the initial
    blur; level 0 of later octaves: none)."""
    no = n_octaves(h, w)
    sizes, hh, ww = [], 2 * h, 2 * w
    for _ in range(no):
        sizes.append((hh, ww))
        hh, ww = hh // 2, ww // 2
    sig = layer_sigmas()
    sig0 = init_sigma()
    return {"n_octaves": no, "sizes": sizes, "sigmas": [sig0] + sig[1:], "ksizes": [blur_ksize(sig0)] + [blur_ksize(s) for s in sig[1:]]}


def reflect101(i, n):
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i >= n, p - i, i)


def blur(src, sig):
    """GaussianBlur(float32, sigma, BORDER_REFLECT_101): row pass then column pass, each acc = k0 * s[0], then
    acc += k_j * (s[-j] + s[+j]) for j = 1 .. r, float32 without fused multiply-add."""
    n = blur_ksize(sig)
    k = gaussian_kernel(n, sig)
    r = n // 2
    h, w = src.shape
    xs = np.arange(w)
    t = k[r] * src
    for j in range(1, r + 1):
        t = t + k[r + j] * (src[:, reflect101(xs - j, w)] + src[:, reflect101(xs + j, w)])
    ys = np.arange(h)
    o = k[r] * t
    for j in range(1, r + 1):
        o = o + k[r + j] * (t[reflect101(ys - j, h)] + t[reflect101(ys + j, h)])
    return o.astype(F)


def gray(img):
    img = np.asarray(img)
    if img.ndim == 3:
        b, g, r = (img[:, :, i].astype(np.int32) for i in range(3))
        img = ((b * 1868 + g * 9617 + r * 4899 + (1 << 13)) >> 14).astype(np.uint8)
    return img


def upscale2(g):
    """resize(INTER_LINEAR) to 2x on float32: per axis weights (0.25, 0.75) / (0.75, 0.25), clamped to (1, 0) at both ends;
    horizontal pass then vertical, dst = a0 * s0 + a1 * s1."""
    def axis(n):
        d = np.arange(2 * n)
        f = (d + 0.5) * 0.5 - 0.5
        s = np.floor(f).astype(np.int64)
        fr = (f - s).astype(F)
        lo = s < 0
        fr[lo], s[lo] = 0, 0
        hi = s >= n - 1
        fr[hi], s[hi] = 0, n - 1
        return s, np.minimum(s + 1, n - 1), F(1) - fr, fr
    h, w = g.shape
    x0, x1, a0, a1 = axis(w)
    t = g[:, x0] * a0 + g[:, x1] * a1
    y0, y1, b0, b1 = axis(h)
    return (t[y0] * b0[:, None] + t[y1] * b1[:, None]).astype(F)


def pyramid(img):
    """Gaussian levels [octave][6] and DoG levels [octave][5], float32."""
    g = gray(img).astype(F)
    lay = layout(*g.shape)
    sig = layer_sigmas()
    gp, dp = [], []
    for o in range(lay["n_octaves"]):
        if o == 0:
            lv = [blur(upscale2(g), lay["sigmas"][0])]
        else:
            p = gp[o - 1][N_LAYERS]
            hh, ww = lay["sizes"][o]
            lv = [np.ascontiguousarray(p[0:2 * hh:2, 0:2 * ww:2])]
        for i in range(1, N_LAYERS + 3):
            lv.append(blur(lv[-1], sig[i]))
        gp.append(lv)
        dp.append([(lv[i + 1] - lv[i]).astype(F) for i in range(N_LAYERS + 2)])
    return gp, dp


def extrema(dp):
    """(octave, layer, r, c) of every 3 x 3 x 3 extremum (val >= / <= all 26 neighbours, val != 0) inside the border."""
    out = []
    for o, lv in enumerate(dp):
        h, w = lv[0].shape
        if h <= 2 * IMG_BORDER or w <= 2 * IMG_BORDER:
            continue
        for i in range(1, N_LAYERS + 1):
            c = lv[i][IMG_BORDER:h - IMG_BORDER, IMG_BORDER:w - IMG_BORDER]
            ge = c > 0
            le = c < 0
            for d in (-1, 0, 1):
                src = lv[i + d]
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        if d == 0 and dy == 0 and dx == 0:
                            continue
                        nb = src[IMG_BORDER + dy:h - IMG_BORDER + dy, IMG_BORDER + dx:w - IMG_BORDER + dx]
                        ge &= c >= nb
                        le &= c <= nb
            rr, cc = np.nonzero(ge | le)
            out.append(np.stack([np.full_like(rr, o), np.full_like(rr, i), rr + IMG_BORDER, cc + IMG_BORDER], 1))
    return np.concatenate(out) if out else np.zeros((0, 4), np.int64)


_STACK = [None, None, None]      # (dp, octave, stacked DoG levels) of the last lookup


def _stack(dp, o):
    if _STACK[0] is not dp or _STACK[1] != o:
        _STACK[:] = [dp, o, np.stack(dp[o])]
    return _STACK[2]


def _derivs(dp, o, layer, r, c):
    """dD and the Hessian of adjustLocalExtrema at integer positions (arrays), float32 in OpenCV's order."""
    img_scale = F(1.0) / F(255)
    ds, s2, cs = img_scale * F(0.5), img_scale, img_scale * F(0.25)
    st = _stack(dp, o)
    def at(l, dy, dx):
        return st[l, r + dy, c + dx]
    cur = lambda dy, dx: at(layer, dy, dx)
    nxt = lambda dy, dx: at(layer + 1, dy, dx)
    prv = lambda dy, dx: at(layer - 1, dy, dx)
    v = cur(0, 0)
    dD = [(cur(0, 1) - cur(0, -1)) * ds, (cur(1, 0) - cur(-1, 0)) * ds, (nxt(0, 0) - prv(0, 0)) * ds]
    v2 = v * F(2)
    dxx = (cur(0, 1) + cur(0, -1) - v2) * s2
    dyy = (cur(1, 0) + cur(-1, 0) - v2) * s2
    dss = (nxt(0, 0) + prv(0, 0) - v2) * s2
    dxy = (cur(1, 1) - cur(1, -1) - cur(-1, 1) + cur(-1, -1)) * cs
    dxs = (nxt(0, 1) - nxt(0, -1) - prv(0, 1) + prv(0, -1)) * cs
    dys = (nxt(1, 0) - nxt(-1, 0) - prv(1, 0) + prv(-1, 0)) * cs
    return v, dD, (dxx, dyy, dss, dxy, dxs, dys)


def _solve3(H, b):
    """Matx33f::solve(DECOMP_LU) for 3 x 3 x 1: Cramer's rule in float32; zeros when the determinant is 0."""
    dxx, dyy, dss, dxy, dxs, dys = H
    a00, a01, a02, a10, a11, a12, a20, a21, a22 = dxx, dxy, dxs, dxy, dyy, dys, dxs, dys, dss
    b0, b1, b2 = b
    det = a00 * (a11 * a22 - a21 * a12) - a01 * (a10 * a22 - a20 * a12) + a02 * (a10 * a21 - a20 * a11)
    ok = det != 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        d = F(1) / np.where(ok, det, F(1))
        x0 = d * (b0 * (a11 * a22 - a12 * a21) - a01 * (b1 * a22 - a12 * b2) + a02 * (b1 * a21 - a11 * b2))
        x1 = d * (a00 * (b1 * a22 - a12 * b2) - b0 * (a10 * a22 - a12 * a20) + a02 * (a10 * b2 - b1 * a20))
        x2 = d * (a00 * (a11 * b2 - b1 * a21) - a01 * (a10 * b2 - b1 * a20) + b0 * (a10 * a21 - a11 * a20))
    z = F(0)
    return [np.where(ok, x0, z).astype(F), np.where(ok, x1, z).astype(F), np.where(ok, x2, z).astype(F)]


def refine(dp, cand):
    """adjustLocalExtrema for every candidate: returns (keep mask, octave, layer, r, c, xc, xr, xi, contr, margin)."""
    m = len(cand)
    o = cand[:, 0].astype(np.int64)
    layer, r, c = cand[:, 1].astype(np.int64).copy(), cand[:, 2].astype(np.int64).copy(), cand[:, 3].astype(np.int64).copy()
    alive = np.ones(m, bool)
    done = np.zeros(m, bool)
    xi, xr, xc = np.zeros(m, F), np.zeros(m, F), np.zeros(m, F)
    margin = np.full(m, np.inf)
    big = F(2147483647 // 3)
    for _step in range(MAX_STEPS):
        act = np.nonzero(alive & ~done)[0]
        if not len(act):
            break
        for oo in np.unique(o[act]):
            a = act[o[act] == oo]
            _, dD, H = _derivs(dp, oo, layer[a], r[a], c[a])
            X = _solve3(H, dD)
            xi[a], xr[a], xc[a] = -X[2], -X[1], -X[0]
            amax = np.maximum(np.maximum(np.abs(xi[a]), np.abs(xr[a])), np.abs(xc[a]))
            conv = amax < F(0.5)
            done[a[conv]] = True
            margin[a[conv]] = np.minimum(margin[a[conv]], np.abs(amax[conv] - 0.5) / 0.5)
            mv = a[~conv]
            if not len(mv):
                continue
            with np.errstate(invalid="ignore"):
                huge = (np.abs(xi[mv]) > big) | (np.abs(xr[mv]) > big) | (np.abs(xc[mv]) > big) | ~np.isfinite(xi[mv] + xr[mv] + xc[mv])
            alive[mv[huge]] = False
            mv = mv[~huge]
            margin[mv] = np.minimum(margin[mv], np.abs(amax[~conv][~huge] - 0.5) / 0.5)
            c[mv] += np.rint(xc[mv]).astype(np.int64)
            r[mv] += np.rint(xr[mv]).astype(np.int64)
            layer[mv] += np.rint(xi[mv]).astype(np.int64)
            h, w = dp[oo][0].shape
            out = (layer[mv] < 1) | (layer[mv] > N_LAYERS) | (c[mv] < IMG_BORDER) | (c[mv] >= w - IMG_BORDER) | (r[mv] < IMG_BORDER) | (r[mv] >= h - IMG_BORDER)
            alive[mv[out]] = False
    alive &= done
    contr = np.zeros(m, F)
    for oo in np.unique(o[alive]):
        a = np.nonzero(alive & (o == oo))[0]
        v, dD, H = _derivs(dp, oo, layer[a], r[a], c[a])
        t = dD[0] * xc[a] + dD[1] * xr[a] + dD[2] * xi[a]
        ct = v * (F(1) / F(255)) + t * F(0.5)
        contr[a] = ct
        lhs = np.abs(ct) * F(N_LAYERS)
        ok = ~(lhs < F(CONTRAST))
        margin[a] = np.minimum(margin[a], np.abs(lhs.astype(np.float64) - CONTRAST) / CONTRAST)
        dxx, dyy, _, dxy, _, _ = H
        tr = dxx + dyy
        det = dxx * dyy - dxy * dxy
        lhs2 = tr * tr * F(EDGE)
        rhs2 = F((EDGE + 1) * (EDGE + 1)) * det
        ok &= ~((det <= 0) | (lhs2 >= rhs2))
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.abs(lhs2.astype(np.float64) - rhs2) / np.maximum(np.abs(rhs2.astype(np.float64)), 1e-30)
        margin[a] = np.minimum(margin[a], rel)
        alive[a[~ok]] = False
    return alive, o, layer, r, c, xc, xr, xi, contr, margin


def fast_atan2(y, x):
    """cv::hal::fastAtan2 (degrees, [0, 360)): the scalar polynomial of mathfuncs_core, float32, no fused multiply-add."""
    deg = F(180.0 / math.pi)
    p1, p3, p5, p7 = F(0.9997878412794807) * deg, F(-0.3258083974640975) * deg, F(0.1555786518463281) * deg, F(-0.04432655554792128) * deg
    eps = F(2.220446049250313e-16)
    y, x = np.asarray(y, F), np.asarray(x, F)
    ax, ay = np.abs(x), np.abs(y)
    sel = ax >= ay
    with np.errstate(divide="ignore", invalid="ignore"):
        cc = np.where(sel, ay / (ax + eps), ax / (ay + eps)).astype(F)
    c2 = cc * cc
    p = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * cc
    a = np.where(sel, p, F(90) - p)
    a = np.where(x < 0, F(180) - a, a)
    a = np.where(y < 0, F(360) - a, a)
    return a.astype(F)


def orientations(gp, o, layer, r, c, size):
    """calcOrientationHist + the peak loop for keypoints sharing one octave: returns (index into the inputs, angle, peak
    margin) per output keypoint, in bin order per input."""
    n = ORI_BINS
    scl = (size * F(0.5) / F(1 << o)).astype(F)
    radius = np.rint(F(ORI_RADIUS) * scl).astype(np.int64)
    sig = F(ORI_SIG) * scl
    exps = (F(-1) / (F(2) * sig * sig)).astype(F)
    idx_out, ang_out, mar_out = [], [], []
    for rad in np.unique(radius):
        sel = np.nonzero(radius == rad)[0]
        ii, jj = np.meshgrid(np.arange(-rad, rad + 1), np.arange(-rad, rad + 1), indexing="ij")
        ii, jj = ii.reshape(-1), jj.reshape(-1)
        hist = np.zeros((len(sel), n), F)
        for q, kk in enumerate(sel):
            img = gp[o][layer[kk]]
            h, w = img.shape
            y, x = r[kk] + ii, c[kk] + jj
            ok = (y > 0) & (y < h - 1) & (x > 0) & (x < w - 1)
            y, x, i2 = y[ok], x[ok], (ii[ok] * ii[ok] + jj[ok] * jj[ok]).astype(F)
            dx = img[y, x + 1] - img[y, x - 1]
            dy = img[y - 1, x] - img[y + 1, x]
            wgt = np.exp((i2 * exps[kk]).astype(np.float64)).astype(F)
            ori = fast_atan2(dy, dx)
            mag = np.sqrt(dx * dx + dy * dy)
            b = np.rint(F(n / 360.0) * ori).astype(np.int64)
            b = np.where(b >= n, b - n, b)
            b = np.where(b < 0, b + n, b)
            np.add.at(hist[q], b, wgt * mag)
        t = hist
        sm = (np.roll(t, 2, 1) + np.roll(t, -2, 1)) * F(1 / 16) + (np.roll(t, 1, 1) + np.roll(t, -1, 1)) * F(4 / 16) + t * F(6 / 16)
        mx = sm.max(1)
        thr = (mx * F(ORI_PEAK)).astype(F)
        lft, rgt = np.roll(sm, 1, 1), np.roll(sm, -1, 1)
        pk = (sm > lft) & (sm > rgt) & (sm >= thr[:, None])
        # margin: how near the peak test's deciding comparisons came to flipping
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.minimum(np.minimum(np.abs(sm - lft), np.abs(sm - rgt)), np.abs(sm - thr[:, None])) / np.maximum(mx[:, None], 1e-30)
        for q, j in zip(*np.nonzero(pk)):
            lv, cv, rv = sm[q, (j - 1) % n], sm[q, j], sm[q, (j + 1) % n]
            bin_ = F(j) + F(0.5) * (lv - rv) / (lv - F(2) * cv + rv)
            bin_ = bin_ + F(n) if bin_ < 0 else (bin_ - F(n) if bin_ >= n else bin_)
            ang = F(360) - F(F(360.0 / n) * bin_)
            if abs(ang - F(360)) < np.finfo(np.float32).eps:
                ang = F(0)
            idx_out.append(sel[q]); ang_out.append(ang)
            # near-miss neighbours: a bin that nearly qualified also makes the count fragile
            near = np.abs(sm[q] - thr[q]) / max(mx[q], 1e-30)
            mar_out.append(min(rel[q, j], near[~pk[q]].min() if (~pk[q]).any() else np.inf))
    order = np.argsort(np.asarray(idx_out, np.int64), kind="stable")
    return np.asarray(idx_out, np.int64)[order], np.asarray(ang_out, F)[order], np.asarray(mar_out)[order]


def detect(img):
    gp, dp = pyramid(img)
    return detect_from_pyramid(gp, dp)


def detect_from_pyramid(gp, dp):
    cand = extrema(dp)
    alive, o, layer, r, c, xc, xr, xi, contr, margin = refine(dp, cand)
    a = np.nonzero(alive)[0]
    o, layer, r, c, xc, xr, xi, contr, margin = (v[a] for v in (o, layer, r, c, xc, xr, xi, contr, margin))
    scale = np.array([F(1 << int(q)) for q in o], F)
    x = ((c.astype(F) + xc) * scale).astype(F)
    y = ((r.astype(F) + xr) * scale).astype(F)
    e = ((layer.astype(F) + xi) / F(N_LAYERS)).astype(F)
    size = (F(SIGMA) * np.power(2.0, e.astype(np.float64)).astype(F) * scale * F(2)).astype(F)
    octave = o + (layer << 8) + (np.rint((xi.astype(np.float64) + 0.5) * 255).astype(np.int64) << 16)
    resp = np.abs(contr)
    kx, ky, ks, ka, kr, ko, km = [], [], [], [], [], [], []
    for oo in np.unique(o):
        s = np.nonzero(o == oo)[0]
        idx, ang, pm = orientations(gp, int(oo), layer[s], r[s], c[s], size[s])
        g = s[idx]
        kx.append(x[g]); ky.append(y[g]); ks.append(size[g]); ka.append(ang); kr.append(resp[g]); ko.append(octave[g])
        km.append(np.minimum(margin[g], pm))
    cat = lambda v, dt: np.concatenate(v).astype(dt) if v else np.zeros(0, dt)
    kx, ky, ks, ka, kr, ko, km = cat(kx, F), cat(ky, F), cat(ks, F), cat(ka, F), cat(kr, F), cat(ko, np.int64), cat(km, np.float64)
    # removeDuplicatedSorted: x asc, y asc, size desc, angle asc, response desc, octave desc
    order = np.lexsort((-ko, -kr, ka, -ks, ky, kx))
    kx, ky, ks, ka, kr, ko, km = (v[order] for v in (kx, ky, ks, ka, kr, ko, km))
    keep = np.ones(len(kx), bool)
    if len(kx) > 1:
        keep[1:] = (kx[1:] != kx[:-1]) | (ky[1:] != ky[:-1]) | (ks[1:] != ks[:-1]) | (ka[1:] != ka[:-1])
    kx, ky, ks, ka, kr, ko, km = (v[keep] for v in (kx, ky, ks, ka, kr, ko, km))
    # firstOctave = -1
    ko = (ko & ~255) | ((ko - 1) & 255)
    return {"pt": np.stack([kx * F(0.5), ky * F(0.5)], 1).astype(F), "size": (ks * F(0.5)).astype(F), "angle": ka,
            "response": kr, "octave": ko.astype(np.int32), "margin": km}
