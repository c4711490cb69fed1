"""numpy emulation of the device half of the baseline JPEG decode (tmrnet_amd/csrc/jpeg.hip):
DCT coefficients in the host decoder's layout -> the RGB frame Pillow (libjpeg-turbo: islow IDCT,
fancy upsampling) returns, bit for bit.  Written from the arithmetic alone, all in int64; it shares
no code with the kernels.  Also the loader of tests/golden/jpeg_cases.npz."""
import hashlib
import io
import os

import numpy as np

GRAY, S444, S420 = 0, 1, 2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_cases.npz")


def load_cases():
    """[(name, kind, (h, w), sha256, bytes)] of the committed fixture file."""
    z = np.load(GOLDEN)
    return [(str(n), str(k), (int(s[0]), int(s[1])), str(sha), z["data_%d" % i].tobytes())
            for i, (n, k, s, sha) in enumerate(zip(z["names"], z["kind"], z["size"], z["sha256"]))]


def pil_rgb(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB"))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _pass(i, sh):
    """The 1-D pass along axis 0 of i (8, ...), int64."""
    i0, i1, i2, i3, i4, i5, i6, i7 = i
    z1 = (i2 + i6) * 4433
    t2 = z1 - i6 * 15137
    t3 = z1 + i2 * 6270
    t0 = (i0 + i4) << 13
    t1 = (i0 - i4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o0, o1, o2, o3 = i7, i5, i3, i1
    z1, z2, z3, z4 = o0 + o3, o1 + o2, o0 + o2, o1 + o3
    z5 = (z3 + z4) * 9633
    o0, o1, o2, o3 = o0 * 2446, o1 * 16819, o2 * 25172, o3 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3 = z3 * -16069 + z5
    z4 = z4 * -3196 + z5
    o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
    out = np.stack([t10 + o3, t11 + o2, t12 + o1, t13 + o0, t13 - o0, t12 - o1, t11 - o2, t10 - o3])
    return (out + (1 << (sh - 1))) >> sh


def idct_plane(coef, q, bh, bw):
    """coef (bh * bw, 64) int16 in block-raster order, q (64,) -> (bh * 8, bw * 8) int64 samples."""
    x = coef.astype(np.int64).reshape(-1, 8, 8) * q.astype(np.int64).reshape(8, 8)
    cols = _pass(np.moveaxis(x, 1, 0), 11)              # along the rows index: columns
    cols = np.moveaxis(cols, 0, 1)                      # (n, 8, 8) again
    rows = _pass(np.moveaxis(cols, 2, 0), 18)           # along each row
    s = np.clip(np.moveaxis(rows, 0, 2) + 128, 0, 255)
    return s.reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def upsample420(c, h, w):
    """Real chroma plane c (ceil(h/2), ceil(w/2)) -> (h, w), the triangle filter."""
    c = c.astype(np.int64)
    up = np.concatenate([c[:1], c[:-1]])    # row r - 1, first row replicated
    dn = np.concatenate([c[1:], c[-1:]])    # row r + 1, last row replicated
    s = np.empty((2 * c.shape[0], c.shape[1]), dtype=np.int64)
    s[0::2] = 3 * c + up
    s[1::2] = 3 * c + dn
    le = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
    ri = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
    out = np.empty((s.shape[0], 2 * s.shape[1]), dtype=np.int64)
    out[:, 0::2] = (3 * s + le + 8) >> 4
    out[:, 1::2] = (3 * s + ri + 7) >> 4
    return out[:h, :w]


def reconstruct(coef, h, w, sampling, blocks_h, blocks_w, qt):
    """coef: flat int16 in the host decoder's layout; qt (3, 64) natural order -> (h, w, 3) uint8."""
    ncomp = 1 if sampling == GRAY else 3
    planes, at = [], 0
    for c in range(ncomp):
        n = blocks_h[c] * blocks_w[c]
        planes.append(idct_plane(np.asarray(coef[at:at + n * 64]).reshape(n, 64), np.asarray(qt[c]),
                                 blocks_h[c], blocks_w[c]))
        at += n * 64
    assert at == len(coef)
    y = planes[0][:h, :w]
    if sampling == GRAY:
        return np.repeat(y[..., None], 3, axis=2).astype(np.uint8)
    if sampling == S444:
        cb, cr = planes[1][:h, :w], planes[2][:h, :w]
    else:
        ch, cw = (h + 1) // 2, (w + 1) // 2
        cb, cr = upsample420(planes[1][:ch, :cw], h, w), upsample420(planes[2][:ch, :cw], h, w)
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)
