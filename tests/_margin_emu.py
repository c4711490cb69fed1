"""numpy emulation of the black-margin cut, written from its description:

1. grey  g = (9798 R + 19235 G + 3735 B + 16384) >> 15   (OpenCV 4's 8-bit RGB -> grey table)
2. mask  m = g > 15
3. 19x19 median with replicated borders = majority vote: set iff >= 181 of the 361 window values
   are set, out-of-range indices clamped to the edge and counted with multiplicity
4. box   over the set pixels with column in [10, w - 10): r0 / r1 min / max row, c0 / c1 min / max
   column; the crop is rows [r0, r1), columns [c0, c1)
5. the full frame [0, h, 0, w] when no pixel qualifies or the crop would be empty

and the synthetic frames the margin tests share (a bright disc on black plus salt noise)."""
import hashlib

import numpy as np

WIN, HALF, VOTES, EDGE, THRESH = 19, 9, 181, 10, 15
SHAPES = [(48, 64), (37, 131), (40, 41), (19, 21), (33, 20), (7, 90), (120, 214)]


def grey(rgb):
    a = rgb.astype(np.int64)
    return ((9798 * a[..., 0] + 19235 * a[..., 1] + 3735 * a[..., 2] + 16384) >> 15).astype(np.uint8)


def grey14(rgb):
    """The older 14-bit table; differs from grey() only where the result lands on 15 or 16."""
    a = rgb.astype(np.int64)
    return ((4899 * a[..., 0] + 9617 * a[..., 1] + 1868 * a[..., 2] + 8192) >> 14).astype(np.uint8)


def majority(m):
    """(h, w) bool -> (h, w) bool: the 19x19 median of a two-valued image, replicated borders."""
    p = np.pad(m.astype(np.int64), HALF, mode="edge")
    c = np.zeros((p.shape[0] + 1, p.shape[1] + 1), dtype=np.int64)
    c[1:, 1:] = p.cumsum(0).cumsum(1)
    h, w = m.shape
    s = c[WIN:WIN + h, WIN:WIN + w] - c[:h, WIN:WIN + w] - c[WIN:WIN + h, :w] + c[:h, :w]
    return s >= VOTES


def mask(rgb):
    """(h, w, 3) uint8 -> (h, w) uint8 0 / 255 after the median."""
    return (majority(grey(rgb) > THRESH) * 255).astype(np.uint8)


def box_of(m):
    """(h, w) mask after the median -> [r0, r1, c0, c1] with the fallbacks."""
    h, w = m.shape
    full = [0, h, 0, w]
    if w <= 2 * EDGE:
        return full
    rows, cols = np.nonzero(m[:, EDGE:w - EDGE])
    if rows.size == 0:
        return full
    r0, r1, c0, c1 = int(rows.min()), int(rows.max()), int(cols.min()) + EDGE, int(cols.max()) + EDGE
    if r1 == r0 or c1 == c0:
        return full
    return [r0, r1, c0, c1]


def box(rgb):
    return box_of(mask(rgb) != 0)


def boxes(frames):
    return np.array([box(f) for f in frames], dtype=np.int32).reshape(-1, 4)


def mask_sha(rgb):
    return hashlib.sha256(mask(rgb).tobytes()).hexdigest()


def disc_frame(h, w, seed, salt=0.03):
    """A bright, textured disc (values 60..255) off-centre on black, plus `salt` of the pixels set
    to a bright value anywhere: the speckle the median has to remove."""
    rng = np.random.default_rng(seed)
    cy = h * (0.45 + 0.1 * rng.random())
    cx = w * (0.45 + 0.1 * rng.random())
    # a frame shorter than the window keeps its disc only if the disc reaches the replicated edges
    ry = 0.42 * h + 0.5 if h >= WIN else 0.8 * h
    rx = max(1.25 * ry, 0.2 * w)
    yy, xx = np.mgrid[0:h, 0:w]
    inside = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
    img = np.zeros((h, w, 3), dtype=np.uint8)
    tex = rng.integers(60, 256, size=(h, w, 3), dtype=np.uint8)
    img[inside] = tex[inside]
    s = rng.random((h, w)) < salt
    img[s] = rng.integers(128, 256, size=(int(s.sum()), 3), dtype=np.uint8)
    return img


def mean_std_f64(frames):
    """meanStd.py in float64: per image mean / population std of v / 255, averaged over images."""
    a = frames.astype(np.float64) / 255.0
    return a.mean(axis=(1, 2)).mean(axis=0), a.std(axis=(1, 2)).mean(axis=0)


def mean_std_f32(frames):
    """meanStd.py as the reference runs it: ToTensor's float32 v / 255 in (3, H, W) layout, numpy
    float32 mean / std over the two contiguous axes (pairwise summation)."""
    a = np.ascontiguousarray(frames.transpose(0, 3, 1, 2)).astype(np.float32) / np.float32(255.0)
    m = np.array([x.mean(axis=(1, 2)) for x in a])
    s = np.array([x.std(axis=(1, 2)) for x in a])
    return m.mean(axis=0), s.mean(axis=0)
