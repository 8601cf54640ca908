"""numpy restatement of the photometric contract ("Photometric augmentation") -- a helper of the photometric tests, not a test.
Written from the contract's text: refl as stated, explicit loops over the taps k, every product and sum one binary64 numpy operation in the
order written, the hash in uint64."""
import numpy as np

MASK64 = (1 << 64) - 1


def refl(i, n):
    if n == 1:
        return 0
    P = 2 * (n - 1)
    m = ((i % P) + P) % P
    return m if m < n else P - m


def splitmix64(z):
    """the finaliser on a uint64 array (numpy wraps modulo 2**64)"""
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def splitmix64_int(z):
    """the same on one Python integer: a second statement of the hash, for the tests of the first"""
    z = (z + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def noise_field(key, H, W):
    """-> float64 [H,W,3]: n of every (pixel, channel) under this key"""
    j = np.arange(H * W * 3, dtype=np.uint64)
    z = splitmix64((np.uint64(int(key)) << np.uint64(32)) | j)
    m = np.uint64(0xffff)
    S = (z & m) + ((z >> np.uint64(16)) & m) + ((z >> np.uint64(32)) & m) + (z >> np.uint64(48))
    n = (S.astype(np.float64) - 131070.0) * (1.7320508075688772 / 65536.0)
    return n.reshape(H, W, 3)


def blur_axis(s, w, r, axis):
    """one pass of the blur over `axis` (0: y, 1: x) of a float64 [H,W,3] array"""
    n = s.shape[axis]
    h = w[0] * s
    for k in range(1, r + 1):
        lo = np.array([refl(i - k, n) for i in range(n)])
        hi = np.array([refl(i + k, n) for i in range(n)])
        h = h + w[k] * (np.take(s, lo, axis=axis) + np.take(s, hi, axis=axis))
    return h


def photometric_image(src, row, max_radius=15):
    """One image.  src float32 [H,W,3], row float64 [32] -> float32 [H,W,3]"""
    H, W = src.shape[:2]
    s = src.astype(np.float64)
    r = min(int(row[14]), int(max_radius))
    w = row[16:32]
    v = blur_axis(blur_axis(s, w, r, axis=1), w, r, axis=0)
    A = row[0:12].reshape(3, 4)
    u = np.empty((H, W, 3), np.float64)
    for c in range(3):
        u[..., c] = ((A[c][0] * v[..., 0] + A[c][1] * v[..., 1]) + A[c][2] * v[..., 2]) + A[c][3]
    u = u + row[12] * noise_field(int(row[13]), H, W)
    u = np.where(u > 0.0, u, 0.0)                # min(max(u, 0), 1), with +0 for a zero of either sign
    u = np.where(u < 1.0, u, 1.0)
    return u.astype(np.float32)


def photometric_batch(images, rows, max_radius=15):
    images = np.asarray(images, np.float32)
    return np.stack([photometric_image(images[b], np.asarray(rows[b], np.float64), max_radius) for b in range(len(images))])
