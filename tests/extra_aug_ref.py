"""numpy restatement of the reference's ``ExtraAugmentations`` (transforms.py:292-329) as this project defines it: the
yardstick for csrc/extra_augment.hip and yolo_v3_amd/extra_augment.py.  Deliberately slow and plain.

``extra_ref(images, programs)``: uint8 ``[H,W,3]`` images and one program per image -> uint8 images.  A program is a list of
at most six steps, executed in order, each on the whole output of the one before; every operation works per channel:

    ("GAUSS", sigma)                 scipy.ndimage.gaussian_filter(channel, sigma) on uint8: radius r = int(4 sigma + 0.5), float64
                                     weights exp(-0.5 / sigma^2 * x^2) / sum, border `reflect`, axis 0 then axis 1, each pass
                                     truncated to uint8; a pass sums centre * w[r] first, then (left + right) * w[r + j] for
                                     j = -r .. -1 (the farthest pair first).  Skipped when r == 0.        [pinned: scipy, bit for bit]
    ("MEDIAN", k)                    odd k in 3..11: the middle of the k x k window, border replicated.   [pinned: scipy]
    ("AVERAGE", k)                   k in 2..7, cv2.blur: window anchored at k // 2, border reflect-101, integer sum,
                                     rint(float64(sum) * float64(1.0 / (k k))).                           [unpinned: cv2 is not installed]
    ("SHARPEN", alpha, lightness)    3x3 float32 kernel (1 - alpha) I + alpha [[-1,-1,-1],[-1,8+lightness,-1],[-1,-1,-1]], border
                                     reflect-101, float32 products summed in row-major tap order without fused multiply-add,
                                     rint, clip to 0..255.                                                [unpinned: imgaug, cv2]
    ("NOISE", scale, per_channel, key)   trunc(clip(float64(p) + scale * z, 0, 255)), z a standard normal from Philox4x32-10 and
                                     Box-Muller in float64 (`normal`), one draw per pixel or, with per_channel, per byte.
    ("ADD", v0, v1, v2)              integers: clip(int32(p) + v_c, 0, 255)
    ("MUL", m0, m1, m2)              trunc(clip(float32(p) * float32(m_c), 0, 255))
    ("CONTRAST", a0, a1, a2)         trunc(clip(float32(a_c) * (float32(p) - 128) + 128, 0, 255)), no fused multiply-add

imgaug 0.2.6 and cv2 are not installed where this was written: the four "unpinned" definitions are recalled from their sources,
the two blurs that reach scipy are checked against it (tests/test_extra_aug_host.py).  The sharpen kernel's entries are float32:
centre = float32(1 - alpha) + float32(alpha) * float32(8 + lightness), the others float32(alpha) * -1.
"""
import numpy as np

M32 = 0xFFFFFFFF
PHILOX_M0, PHILOX_M1, PHILOX_W0, PHILOX_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


# ---- borders ---------------------------------------------------------------------------------------------------------------------
def reflect(i, n):
    """scipy `reflect` (d c b a | a b c d | d c b a): half-sample symmetric, period 2n."""
    i = np.asarray(i) % (2 * n)
    return np.where(i >= n, 2 * n - 1 - i, i)


def reflect101(i, n):
    """cv2 BORDER_REFLECT_101 (d c b | a b c d | c b a): period 2n - 2; an axis of length 1 maps to index 0."""
    if n == 1:
        return np.zeros_like(np.asarray(i))
    i = np.asarray(i) % (2 * n - 2)
    return np.where(i >= n, 2 * n - 2 - i, i)


def replicate(i, n):
    return np.clip(np.asarray(i), 0, n - 1)


# ---- the blurs ---------------------------------------------------------------------------------------------------------------------
def gauss_radius(sigma):
    return int(4.0 * float(sigma) + 0.5)


def gauss_weights(sigma):
    """scipy's _gaussian_kernel1d(sigma, 0, r): float64 [2r + 1]."""
    r = gauss_radius(sigma)
    x = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / (float(sigma) * float(sigma)) * x ** 2)
    return phi / phi.sum()


def _gauss_pass(a, w, r, axis):
    """One correlate1d pass (scipy's symmetric branch) along ``axis`` of a uint8 plane, truncated to uint8."""
    n = a.shape[axis]
    idx = np.arange(n)
    f = a.astype(np.float64)
    acc = f * w[r]
    for j in range(-r, 0):
        left = np.take(f, reflect(idx + j, n), axis=axis)
        right = np.take(f, reflect(idx - j, n), axis=axis)
        acc = acc + (left + right) * w[r + j]
    return acc.astype(np.uint8)                       # values are in [0, 255.0...]: the C cast truncates


def gauss(ch, sigma):
    r = gauss_radius(sigma)
    if r == 0:
        return ch.copy()
    w = gauss_weights(sigma)
    return _gauss_pass(_gauss_pass(ch, w, r, 0), w, r, 1)


def _window(ch, offsets_y, offsets_x, border):
    """[len(oy) * len(ox), H, W]: the taps of every pixel, row-major in (dy, dx)."""
    H, W = ch.shape
    ys, xs = np.arange(H), np.arange(W)
    taps = []
    for dy in offsets_y:
        rows = ch[border(ys + dy, H)]
        for dx in offsets_x:
            taps.append(rows[:, border(xs + dx, W)])
    return np.stack(taps)


def median(ch, k):
    o = range(-(k // 2), k // 2 + 1)
    taps = _window(ch, o, o, replicate)
    return np.sort(taps, axis=0)[k * k // 2]


def average(ch, k):
    o = range(-(k // 2), k - k // 2)
    s = _window(ch, o, o, reflect101).astype(np.int64).sum(axis=0)
    return np.rint(s.astype(np.float64) * np.float64(1.0 / (k * k))).astype(np.uint8)


def sharpen_kernel(alpha, lightness):
    a = np.float32(alpha)
    centre = np.float32(1.0 - float(alpha)) + a * np.float32(8.0 + float(lightness))
    off = a * np.float32(-1.0)
    kern = np.full((3, 3), off, dtype=np.float32)
    kern[1, 1] = centre
    return kern


def sharpen(ch, alpha, lightness):
    kern = sharpen_kernel(alpha, lightness).reshape(-1)
    taps = _window(ch, (-1, 0, 1), (-1, 0, 1), reflect101).astype(np.float32)
    acc = np.zeros(ch.shape, dtype=np.float32)
    for t in range(9):
        acc = acc + kern[t] * taps[t]                 # float32 product, then float32 sum
    return np.clip(np.rint(acc), 0, 255).astype(np.uint8)


# ---- the noise ---------------------------------------------------------------------------------------------------------------------
def philox4x32(counter, key, rounds=10):
    """Philox4x32-10 (Salmon et al., Random123): counter [..., 4] and key [..., 2] uint32 arrays -> [..., 4] uint32."""
    c = [np.asarray(counter[..., i], dtype=np.uint64) for i in range(4)]
    k0, k1 = (np.asarray(key[..., i], dtype=np.uint64) for i in range(2))
    for _ in range(rounds):
        p0, p1 = c[0] * np.uint64(PHILOX_M0), c[2] * np.uint64(PHILOX_M1)          # 32 x 32 -> 64 bits: no overflow
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & np.uint64(M32), p1 >> np.uint64(32), p1 & np.uint64(M32)
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0, k1 = (k0 + np.uint64(PHILOX_W0)) & np.uint64(M32), (k1 + np.uint64(PHILOX_W1)) & np.uint64(M32)
    return np.stack(c, axis=-1).astype(np.uint32)


def normal(e, key):
    """The standard normal of element ``e`` (uint64 array) under the 64-bit ``key``: counter (e & 0xffffffff, e >> 32, 0, 0),
    Box-Muller in float64 on the first two words: u1 = (x0 + 1) 2^-32, u2 = x1 2^-32, z = sqrt(-2 ln u1) cos(2 pi u2)."""
    e = np.asarray(e, dtype=np.uint64)
    ctr = np.zeros(e.shape + (4,), dtype=np.uint32)
    ctr[..., 0] = (e & np.uint64(M32)).astype(np.uint32)
    ctr[..., 1] = (e >> np.uint64(32)).astype(np.uint32)
    k = np.zeros(e.shape + (2,), dtype=np.uint32)
    k[..., 0], k[..., 1] = int(key) & M32, (int(key) >> 32) & M32
    x = philox4x32(ctr, k)
    u1 = (x[..., 0].astype(np.float64) + 1.0) * 2.0 ** -32
    u2 = x[..., 1].astype(np.float64) * 2.0 ** -32
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)


def _elements(img, per_channel):
    H, W, _ = img.shape
    pix = np.arange(H * W, dtype=np.uint64).reshape(H, W, 1)
    return pix * np.uint64(3) + np.arange(3, dtype=np.uint64) if per_channel else np.broadcast_to(pix, (H, W, 3))


def noise_float(img, scale, per_channel, key):
    """float64 [H,W,3]: p + scale * z, before the clip and the truncation."""
    return img.astype(np.float64) + float(scale) * normal(_elements(img, per_channel), key)


def noise_mask(img, scale, per_channel, key, eps=1e-9):
    """Bytes whose value before clip and truncation lies within ``eps`` of an integer (the clip bounds 0 and 255 are integers):
    the only places where another float64 log / cos may give a neighbouring byte.  A byte the noise does not move at all
    (scale * z == 0: the same on every implementation) is not one of them."""
    v = noise_float(img, scale, per_channel, key)
    return (np.abs(v - np.rint(v)) <= eps) & (v != img)


# ---- programs ----------------------------------------------------------------------------------------------------------------------
def apply_step(img, step):
    op, a = step[0], step[1:]
    if op == "NOISE":
        return np.clip(noise_float(img, a[0], a[1], a[2]), 0.0, 255.0).astype(np.uint8)
    out = np.empty_like(img)
    for c in range(3):
        ch = img[:, :, c]
        if op == "GAUSS":
            out[:, :, c] = gauss(ch, a[0])
        elif op == "MEDIAN":
            out[:, :, c] = median(ch, a[0])
        elif op == "AVERAGE":
            out[:, :, c] = average(ch, a[0])
        elif op == "SHARPEN":
            out[:, :, c] = sharpen(ch, a[0], a[1])
        elif op == "ADD":
            out[:, :, c] = np.clip(ch.astype(np.int32) + int(a[c]), 0, 255)
        elif op == "MUL":
            out[:, :, c] = np.clip(ch.astype(np.float32) * np.float32(a[c]), 0, 255)
        elif op == "CONTRAST":
            out[:, :, c] = np.clip(np.float32(a[c]) * (ch.astype(np.float32) - np.float32(128)) + np.float32(128), 0, 255)
        else:
            raise ValueError("unknown operation %r" % (op,))
    return out


def extra_ref(images, programs):
    out = []
    for img, prog in zip(images, programs):
        img = np.ascontiguousarray(img, dtype=np.uint8)
        assert len(prog) <= 6
        for step in prog:
            img = apply_step(img, step)
        out.append(img)
    return out


def program_noise_mask(img, prog, eps=1e-9):
    """OR of `noise_mask` over the NOISE steps of a program, each taken at that step's input (restatement values).  A masked
    byte that later steps spread (a blur after the noise) is not followed: such a program's mask must be empty to be usable."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    mask = np.zeros(img.shape, dtype=bool)
    for step in prog:
        if step[0] == "NOISE":
            mask |= noise_mask(img, step[1], step[2], step[3], eps)
        img = apply_step(img, step)
    return mask
