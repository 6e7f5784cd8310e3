"""NumPy restatement of the colour augmentation specified in include/gims_hip.h (gims_color_aug), written independently of
gims_amd/augment.py and csrc/augment.hip: its own border loop, its own line drawing, its own table, the same integer generator.  The
device is pinned to this bit for bit (tests/test_augment_gpu.py); the known answers of tests/test_augment_cpu.py pin this.

A float32 fmaf(a, b, c) is emulated as float32(float64(a) * float64(b) + float64(c)): with a pixel (8 bits) or a z (20 bits) as one factor
and magnitudes below 2^10 the float64 product and sum are exact, so the one rounding to float32 is the fused one."""
import numpy as np

GAMMA = np.uint64(0x9E3779B97F4A7C15)
M1 = np.uint64(0xBF58476D1CE4E5B9)
M2 = np.uint64(0x94D049BB133111EB)


# ------------------------------------------------------------------------------------------------ (a) the table
def lut(alpha=1.0, beta=0.0):
    """Brightness / contrast table, entry by entry in float32: i * float32(alpha) (if alpha != 1) + float32(beta * 255) (if beta != 0),
    clipped to [0, 255], truncated."""
    out = np.zeros(256, dtype=np.uint8)
    a, b = np.float32(alpha), np.float32(beta * 255)
    for i in range(256):
        v = np.float32(i)
        if alpha != 1:
            v = np.float32(v * a)
        if beta != 0:
            v = np.float32(v + b)
        out[i] = int(min(max(float(v), 0.0), 255.0))        # int() truncates; the value is >= 0
    return out


# ------------------------------------------------------------------------------------------------ (b) motion blur
def reflect101(p, n):
    """cv::borderInterpolate(p, n, BORDER_REFLECT_101)."""
    if n == 1:
        return 0
    while not 0 <= p < n:
        p = -p if p < 0 else 2 * (n - 1) - p
    return p


def line_kernel(ksize, xs, ys, xe, ye):
    """8-connected line from (xs, ys) to (xe, ye): one cell per step along the longer axis, the other coordinate the nearest integer of
    the ideal line, an exact half going towards the end point; float32, divided by its float32 sum."""
    k = np.zeros((ksize, ksize), dtype=np.float32)
    dx, dy = xe - xs, ye - ys
    sx, sy = (dx > 0) - (dx < 0), (dy > 0) - (dy < 0)
    n = max(abs(dx), abs(dy))
    for i in range(n + 1):
        side = (2 * i * min(abs(dx), abs(dy)) + n) // (2 * n) if n else 0
        if abs(dx) >= abs(dy):
            x, y = xs + sx * i, ys + sy * side
        else:
            x, y = xs + sx * side, ys + sy * i
        k[y, x] = 1
    total = np.float32(0)
    for v in k.reshape(-1):
        total = np.float32(total + v)
    return (k / total).astype(np.float32)


def blur(img, kernel):
    """cv2.filter2D(img, -1, kernel) restated for uint8 [h, w, c]: correlation, anchor at the centre, BORDER_REFLECT_101, one fmaf per
    non-zero tap in row-major order from acc = 0, saturate_cast<uchar> (round half to even, clamp)."""
    h, w = img.shape[:2]
    ks = kernel.shape[0]
    r = ks // 2
    ys = np.array([reflect101(p, h) for p in range(-r, h + r)])
    xs = np.array([reflect101(p, w) for p in range(-r, w + r)])
    acc = np.zeros(img.shape, dtype=np.float32)
    for i in range(ks):
        for j in range(ks):
            coef = kernel[i, j]
            if coef == 0:
                continue
            pix = img[ys[i:i + h]][:, xs[j:j + w]].astype(np.float64)
            acc = (np.float64(coef) * pix + acc.astype(np.float64)).astype(np.float32)
    return np.clip(np.rint(acc), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ (c) noise
def splitmix64(x):
    with np.errstate(over="ignore"):
        x = x + GAMMA
        x = (x ^ (x >> np.uint64(30))) * M1
        x = (x ^ (x >> np.uint64(27))) * M2
        return x ^ (x >> np.uint64(31))


def noise_z(key, e):
    """z of the elements e (array of indices) under the 64-bit key: float32, exact."""
    with np.errstate(over="ignore"):
        s = np.uint64(key) ^ (np.asarray(e).astype(np.uint64) * GAMMA)
    total = np.zeros(s.shape, dtype=np.int64)
    for _ in range(3):
        s = splitmix64(s)
        for sh in (0, 16, 32, 48):
            total += ((s >> np.uint64(sh)) & np.uint64(0xFFFF)).astype(np.int64)
    return ((total - 393210).astype(np.float32) / np.float32(65536)).astype(np.float32)


def noise(img, sigma, key):
    z = noise_z(key, np.arange(img.size)).reshape(img.shape)
    v = (np.float64(np.float32(sigma)) * z.astype(np.float64) + img.astype(np.float64)).astype(np.float32)
    return np.trunc(np.clip(v, 0, 255)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ a whole plan
def apply(img, table=None, kernel=None, sigma=0.0, key=0):
    """One image uint8 [h, w] or [h, w, c] under one plan: table, then blur OR noise."""
    assert kernel is None or not sigma > 0
    a = np.asarray(img, dtype=np.uint8)
    x = a.reshape(a.shape[0], a.shape[1], -1)
    if table is not None:
        x = table[x]
    if kernel is not None:
        x = blur(x, kernel)
    elif sigma > 0:
        x = noise(x, sigma, key)
    return x.reshape(a.shape).copy()


def apply_plan(img, plan):
    """The same for the PARAMETERS of a drawn plan (gims_amd.augment.ColorAugPlan): the table and the line are rebuilt here."""
    table = lut(plan.alpha, plan.beta) if plan.lut_kind is not None else None
    kernel = line_kernel(plan.ksize, *plan.line[0], *plan.line[1]) if plan.ksize else None
    return apply(img, table, kernel, float(plan.sigma), plan.key)
