"""Generate tests/golden/jpeg_cases.npz: small JPEG files (and a few files the device decoder must
hand to PIL or refuse) with the sha256 of Pillow's own RGB decode of each, for
tests/test_jpeg_cpu.py (host entropy decoder + the numpy emulation) and tests/test_jpeg_gpu.py
(tmrnet_amd.jpeg.DeviceJpegDecoder).  The bytes are committed, so the encoder that wrote them does
not matter afterwards; the hashes pin Pillow 12.2.0 / libjpeg-turbo's decode.

Arrays: names (U), kind (U: ok / unsupported / malformed), size (n, 2) = (h, w), sha256 (U, empty
where Pillow's decode is not the point), data_<i> (uint8 file bytes)."""
import hashlib
import io
import os

import numpy as np
import PIL
from PIL import Image

# (h, w)
SIZES_A = [(1, 1), (8, 8), (16, 16), (17, 17), (29, 37), (37, 29), (86, 48)]
VARIANTS_A = [
    ("420_q75", "RGB", dict(quality=75)),
    ("444_q90", "RGB", dict(quality=90, subsampling=0)),
    ("gray_q75", "L", dict(quality=75)),
    ("420_opt", "RGB", dict(quality=75, optimize=True)),
    ("420_rst3", "RGB", dict(quality=75, restart_marker_blocks=3)),
    ("420_q100", "RGB", dict(quality=100)),
    ("420_q3", "RGB", dict(quality=3)),
]
SIZES_B = [(70, 50), (214, 120)]
VARIANTS_B = [
    ("420_q75", dict(quality=75)),
    ("420_q100", dict(quality=100)),
    ("420_q3", dict(quality=3)),
    ("444_q95", dict(quality=95, subsampling=0)),
    ("420_rstrow", dict(quality=75, restart_marker_rows=1)),
]
# beyond the list above: the wide orientation of the odd size (width 214 = 13 * 16 + 6, as 854 is)
SIZES_C = [(120, 214)]
VARIANTS_C = [("420_q75", dict(quality=75)), ("420_q3", dict(quality=3))]


def smooth(h, w, seed):
    """A colour field with noise on it: every frequency band sees some energy."""
    rng = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(xx * 3 + yy) % 256, (yy * 5 + 40) % 256, (xx + yy * 2 + 90) % 256], -1)
    return np.clip(base + rng.normal(0, 12, base.shape), 0, 255).astype(np.uint8)


def noise(h, w, seed):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, (h, w, 3), dtype=np.uint8)


def saturated(h, w, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    return (g.integers(0, 2, (h, w, 3), dtype=np.uint8) * 255).astype(np.uint8)


def encode(img, mode, fmt="JPEG", **kw):
    im = Image.fromarray(img, "RGB")
    if mode != "RGB":
        im = im.convert(mode)
    buf = io.BytesIO()
    im.save(buf, fmt, **kw)
    return buf.getvalue()


def hand_built(value, q=1):
    """An 8x8 greyscale baseline file written by hand: DC 0 and AC[1] = value (128 <= |value| <=
    255, so 8 value bits), with an AC table whose only codes are the 1-bit '0' for symbol 0x08
    (run 0, size 8) and the 2-bit '10' for the end of block.  Code and value bits together are 9:
    the longest pair a 9-bit one-lookup table can hold, with the largest values it can meet."""
    assert 128 <= abs(value) <= 255
    seg = lambda m, body: b"\xff" + bytes([m]) + (len(body) + 2).to_bytes(2, "big") + body
    dqt = seg(0xDB, b"\x00" + bytes([q] * 64))
    sof = seg(0xC0, b"\x08" + (8).to_bytes(2, "big") + (8).to_bytes(2, "big") + b"\x01\x01\x11\x00")
    dht_dc = seg(0xC4, b"\x00" + bytes([1] + [0] * 15) + b"\x00")          # '0' -> size 0
    dht_ac = seg(0xC4, b"\x10" + bytes([1, 1] + [0] * 14) + b"\x08\x00")   # '0' -> 0x08, '10' -> EOB
    sos = seg(0xDA, b"\x01\x01\x00\x00\x3f\x00")
    vbits = value if value > 0 else value + 255      # the 8 value bits of a size-8 coefficient
    bits = "0" + "0" + format(vbits, "08b") + "10"   # DC size 0; AC code, value; EOB
    bits += "1" * (-len(bits) % 8)
    scan = bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8))
    assert b"\xff" not in scan
    return b"\xff\xd8" + dqt + sof + dht_dc + dht_ac + sos + scan + b"\xff\xd9"


def pil_sha(data):
    with Image.open(io.BytesIO(data)) as im:
        rgb = np.asarray(im.convert("RGB"))
    return hashlib.sha256(np.ascontiguousarray(rgb).tobytes()).hexdigest()


def main():
    cases = []   # (name, kind, (h, w), bytes)
    seed = 7000
    for h, w in SIZES_A:
        for tag, mode, kw in VARIANTS_A:
            seed += 1
            cases.append(("smooth_%dx%d_%s" % (h, w, tag), "ok", (h, w), encode(smooth(h, w, seed), mode, **kw)))
    for sizes, variants in ((SIZES_B, [(t, k) for t, k in VARIANTS_B]), (SIZES_C, VARIANTS_C)):
        for h, w in sizes:
            for kind, gen in (("noise", noise), ("sat", saturated)):
                for tag, kw in variants:
                    seed += 1
                    cases.append(("%s_%dx%d_%s" % (kind, h, w, tag), "ok", (h, w),
                                  encode(gen(h, w, seed), "RGB", **kw)))
    for value in (200, -200, 255, -128):
        cases.append(("hand_8x8_ac1_%+d" % value, "ok", (8, 8), hand_built(value)))
    h, w = 37, 29
    img = smooth(h, w, 99)
    cases.append(("progressive_37x29", "unsupported", (h, w), encode(img, "RGB", quality=75, progressive=True)))
    cases.append(("422_37x29", "unsupported", (h, w), encode(img, "RGB", quality=75, subsampling=1)))
    cases.append(("cmyk_37x29", "unsupported", (h, w), encode(img, "CMYK", quality=75)))
    cases.append(("png_37x29", "unsupported", (h, w), encode(img, "RGB", fmt="PNG")))
    whole = encode(smooth(h, w, 98), "RGB", quality=75)
    cases.append(("cut60_37x29", "malformed", (h, w), whole[:len(whole) * 6 // 10]))
    # a DHT segment whose length field claims more bytes than the file has
    at = whole.index(b"\xff\xc4")
    cases.append(("dhtlen_37x29", "malformed", (h, w), whole[:at + 2] + b"\xff\xf0" + whole[at + 4:]))

    out = {"pillow": np.array(PIL.__version__),
           "names": np.array([c[0] for c in cases]),
           "kind": np.array([c[1] for c in cases]),
           "size": np.array([c[2] for c in cases], dtype=np.int32),
           "sha256": np.array([pil_sha(c[3]) if c[1] != "malformed" else "" for c in cases])}
    for i, c in enumerate(cases):
        out["data_%d" % i] = np.frombuffer(c[3], dtype=np.uint8)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jpeg_cases.npz")
    np.savez(path, **out)
    print(path, len(cases), "cases", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
