"""NumPy restatement of csrc/warp.hip: cv2.warpPerspective (INTER_LINEAR, BORDER_CONSTANT 0) and cv2.resize
(INTER_LINEAR, INTER_AREA) for uint8 images, integer- and float32-exact, operation for operation.  The device is pinned to it bit
for bit; it is itself pinned to known answers (tests/test_warp_cpu.py), not to OpenCV, which is not available here."""
import numpy as np

INT_MAX, INT_MIN = 2147483647.0, -2147483648.0
INTER_LINEAR, INTER_AREA = 1, 3
F32 = np.float32


def invert3(m):
    """cv::invert(M, DECOMP_LU) for 3x3 float64: determinant / cofactor fast path, zeros when singular."""
    s = [[float(v) for v in r] for r in np.asarray(m, dtype=np.float64).reshape(3, 3)]
    d = s[0][0] * (s[1][1] * s[2][2] - s[1][2] * s[2][1]) - s[0][1] * (s[1][0] * s[2][2] - s[1][2] * s[2][0]) + \
        s[0][2] * (s[1][0] * s[2][1] - s[1][1] * s[2][0])
    if d == 0.0:
        return np.zeros((3, 3))
    d = 1.0 / d
    t = [(s[1][1] * s[2][2] - s[1][2] * s[2][1]) * d, (s[0][2] * s[2][1] - s[0][1] * s[2][2]) * d, (s[0][1] * s[1][2] - s[0][2] * s[1][1]) * d,
         (s[1][2] * s[2][0] - s[1][0] * s[2][2]) * d, (s[0][0] * s[2][2] - s[0][2] * s[2][0]) * d, (s[0][2] * s[1][0] - s[0][0] * s[1][2]) * d,
         (s[1][0] * s[2][1] - s[1][1] * s[2][0]) * d, (s[0][1] * s[2][0] - s[0][0] * s[2][1]) * d, (s[0][0] * s[1][1] - s[0][1] * s[1][0]) * d]
    return np.array(t).reshape(3, 3)


def _hwc(img):
    a = np.asarray(img, dtype=np.uint8)
    return (a[:, :, None] if a.ndim == 2 else a), a.ndim == 2


def warp_perspective(img, M, dsize):
    src, gray = _hwc(img)
    sh, sw, c = src.shape
    dw, dh = dsize
    m = invert3(M).reshape(9)
    bh0 = min(16, dh)
    bw0 = min(1024 // bh0, dw)
    xs = np.arange(dw)
    xb = ((xs // bw0) * bw0).astype(np.float64)[None, :]
    x1 = (xs - (xs // bw0) * bw0).astype(np.float64)[None, :]
    y = np.arange(dh, dtype=np.float64)[:, None]
    X0 = m[0] * xb + m[1] * y + m[2]
    Y0 = m[3] * xb + m[4] * y + m[5]
    W0 = m[6] * xb + m[7] * y + m[8]
    W = W0 + m[6] * x1
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        W = np.where(W != 0, 32.0 / np.where(W != 0, W, 1.0), 0.0)
        fX = (X0 + m[0] * x1) * W
        fY = (Y0 + m[3] * x1) * W
    fX = np.where(fX < INT_MAX, fX, INT_MAX)
    fX = np.where(INT_MIN < fX, fX, INT_MIN)
    fY = np.where(fY < INT_MAX, fY, INT_MAX)
    fY = np.where(INT_MIN < fY, fY, INT_MIN)
    X, Y = np.rint(fX).astype(np.int64), np.rint(fY).astype(np.int64)
    sx, sy = np.clip(X >> 5, -32768, 32767), np.clip(Y >> 5, -32768, 32767)
    ax, ay = X & 31, Y & 31
    w = [(32 - ay) * (32 - ax) * 32, (32 - ay) * ax * 32, ay * (32 - ax) * 32, ay * ax * 32]
    corner = (ax == 0) & (ay == 0)
    w[0] = np.where(corner, 32767, w[0])
    w[3] = np.where(corner, 1, w[3])
    acc = np.zeros((dh, dw, c), dtype=np.int64)
    for k, (ox, oy) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
        tx, ty = sx + ox, sy + oy
        inside = (tx >= 0) & (tx < sw) & (ty >= 0) & (ty < sh)
        v = src[np.clip(ty, 0, sh - 1), np.clip(tx, 0, sw - 1)].astype(np.int64) * inside[:, :, None]
        acc += v * w[k][:, :, None]
    out = np.clip((acc + (1 << 14)) >> 15, 0, 255).astype(np.uint8)
    return out[:, :, 0] if gray else out


def _linear_coef(n_dst, n_src, scale, inv_scale, area_mode, clamp):
    d = np.arange(n_dst)
    if not area_mode:
        f = ((d + 0.5) * scale - 0.5).astype(F32)
        s = np.floor(f).astype(np.int64)
        f = (f - s.astype(F32)).astype(F32)
    else:
        s = np.floor(d * scale).astype(np.int64)
        f = ((d + 1).astype(np.float64) - (s + 1).astype(np.float64) * inv_scale).astype(F32)
        f = np.where(f <= 0, F32(0), (f - np.floor(f).astype(np.int64).astype(F32)).astype(F32)).astype(F32)
    if clamp:
        lo, hi = s < 0, s >= n_src - 1
        f = np.where(lo | hi, F32(0), f).astype(F32)
        s = np.where(lo, 0, np.where(hi, n_src - 1, s))
    a0 = np.clip(np.rint((F32(1) - f) * F32(2048)), -32768, 32767).astype(np.int64)
    a1 = np.clip(np.rint(f * F32(2048)), -32768, 32767).astype(np.int64)
    return s, a0, a1


def _resize_linear(src, dw, dh, sx_, sy_, isx, isy, area_mode):
    sh, sw, c = src.shape
    sx, a0, a1 = _linear_coef(dw, sw, sx_, isx, area_mode, True)
    sy, b0, b1 = _linear_coef(dh, sh, sy_, isy, area_mode, False)
    clip = lambda v: np.where(v >= 0, np.where(v < sh, v, sh - 1), 0)   # noqa: E731
    s = src.astype(np.int64)
    x1 = np.minimum(sx + 1, sw - 1)
    hrow = s[:, sx] * a0[None, :, None] + np.where((sx + 1 < sw)[None, :, None], s[:, x1] * a1[None, :, None], 0)   # [sh, dw, c]
    h0, h1 = hrow[clip(sy)], hrow[clip(sy + 1)]
    out = (((b0[:, None, None] * (h0 >> 4)) >> 16) + ((b1[:, None, None] * (h1 >> 4)) >> 16) + 2) >> 2
    return out.astype(np.uint8)


def _resize_area_fast(src, dw, dh, ix, iy):
    sh, sw, c = src.shape
    out = np.zeros((dh, dw, c), dtype=np.uint8)
    s = src.astype(np.int64)
    scale = F32(1) / F32(ix * iy)
    fh, fw = min(dh, sh // iy), min(dw, sw // ix)                       # blocks wholly inside the image
    tot = s[:fh * iy, :fw * ix].reshape(fh, iy, fw, ix, c).sum((1, 3))
    v = (tot + 2) >> 2 if ix == 2 and iy == 2 else np.rint(tot.astype(F32) * scale)
    out[:fh, :fw] = np.clip(v, 0, 255)
    for y in range(dh):
        for x in range(dw):
            y0, x0 = y * iy, x * ix
            if (y < fh and x < fw) or y0 >= sh or x0 >= sw:
                continue
            blk = s[y0:min(y0 + iy, sh), x0:min(x0 + ix, sw)]
            out[y, x] = np.clip(np.rint(blk.reshape(-1, c).sum(0).astype(F32) / F32(blk.shape[0] * blk.shape[1])), 0, 255)
    return out


def area_taps(d, n, scale):
    """computeResizeAreaTab for destination index d: [(source index, float32 weight)] in OpenCV's order."""
    fs1 = d * scale
    fs2 = fs1 + scale
    cell = min(scale, n - fs1)
    s1, s2 = int(np.ceil(fs1)), int(np.floor(fs2))
    s2 = min(s2, n - 1)
    s1 = min(s1, s2)
    taps = []
    if s1 - fs1 > 1e-3:
        taps.append((s1 - 1, F32((s1 - fs1) / cell)))
    for s in range(s1, s2):
        taps.append((s, F32(1.0 / cell)))
    if fs2 - s2 > 1e-3:
        taps.append((s2, F32(min(min(fs2 - s2, 1.0), cell) / cell)))
    return taps


def _resize_area(src, dw, dh, scale_x, scale_y):
    sh, sw, c = src.shape
    xt = [area_taps(x, sw, scale_x) for x in range(dw)]
    yt = [area_taps(y, sh, scale_y) for y in range(dh)]
    nx, ny = max(map(len, xt)), max(map(len, yt))
    xi = np.array([[t[i][0] if i < len(t) else 0 for i in range(nx)] for t in xt])
    xa = np.array([[t[i][1] if i < len(t) else 0 for i in range(nx)] for t in xt], dtype=F32)
    xm = np.array([[i < len(t) for i in range(nx)] for t in xt])
    s = src.astype(F32)
    out = np.zeros((dh, dw, c), dtype=np.uint8)
    for y in range(dh):
        acc = np.zeros((dw, c), dtype=F32)
        for sy, beta in yt[y]:
            row = s[sy]
            buf = np.zeros((dw, c), dtype=F32)
            for i in range(nx):
                buf = np.where(xm[:, i, None], (buf + row[xi[:, i]] * xa[:, i, None]).astype(F32), buf)
            acc = (acc + (F32(beta) * buf).astype(F32)).astype(F32)
        out[y] = np.clip(np.rint(acc), 0, 255)
    return out


def resize(img, dsize, interpolation=INTER_LINEAR):
    src, gray = _hwc(img)
    sh, sw, c = src.shape
    dw, dh = dsize
    if (dw, dh) == (sw, sh):
        out = src.copy()
    else:
        isx, isy = dw / sw, dh / sh
        scx, scy = 1.0 / isx, 1.0 / isy
        ix, iy = int(np.rint(scx)), int(np.rint(scy))
        fast = abs(scx - ix) < np.finfo(np.float64).eps and abs(scy - iy) < np.finfo(np.float64).eps
        interp = interpolation
        if interp == INTER_LINEAR and fast and ix == 2 and iy == 2:
            interp = INTER_AREA
        if interp == INTER_AREA and scx >= 1 and scy >= 1:
            out = _resize_area_fast(src, dw, dh, ix, iy) if fast else _resize_area(src, dw, dh, scx, scy)
        else:
            out = _resize_linear(src, dw, dh, scx, scy, isx, isy, interp == INTER_AREA)
    return out[:, :, 0] if gray else out


def label_rows(kp0s, kp1s, Hs, dist_thresh=3, n_iters=1):
    """The match_indexes rows of train.py:118-125 for a batch of pairs, through the CPU oracle of torch_find_matches
    (oracle/eval_oracle.py): [k, i0, i1] matches, [k, miss0, -1], [k, -1, miss1], pair after pair; int64 [R, 3]."""
    import torch
    from oracle.eval_oracle import find_gt_matches
    out = []
    for k, (a, b, h) in enumerate(zip(kp0s, kp1s, Hs)):
        ma0, ma1, mi0, mi1 = find_gt_matches(torch.as_tensor(np.asarray(a, np.float32)), torch.as_tensor(np.asarray(b, np.float32)),
                                             torch.as_tensor(np.asarray(h, np.float32)), dist_thresh, n_iters)
        c1 = np.concatenate([ma0, mi0, -np.ones(len(mi1), np.int64)])
        c2 = np.concatenate([ma1, -np.ones(len(mi0), np.int64), mi1])
        out.append(np.stack([np.full(len(c1), k, np.int64), c1, c2], 1).astype(np.int64))
    return np.concatenate(out) if out else np.zeros((0, 3), np.int64)
