"""The black-margin cut on the device (margin.hip, the boxed passes of resize.hip),
bit for bit: masks and boxes against the numpy emulation (tests/_margin_emu.py) and the committed
cases (tests/golden/margin_cases.npz), the boxed resize against the dense one and Pillow's
crop().resize(), the channel sums against numpy, load_frames(cut_margin=True) end to end."""
import hashlib

import numpy as np
import pytest
import torch
from PIL import Image

from oracle import resize_ref
from tests import _margin_emu as emu
from tests.test_margin_cpu import golden_cases
from tmrnet_amd import frames

pytestmark = pytest.mark.gpu


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _check(x, dev, **kw):
    """masks and boxes of the (F, h, w, 3) uint8 batch x equal the emulation's; returns the boxes."""
    xd = _dev(x, dev)
    want_m = np.stack([emu.mask(f) for f in x])
    want_b = np.array([emu.box_of(m != 0) for m in want_m], dtype=np.int32)
    got_m = frames.margin_mask(xd, **kw)
    got_b = frames.margin_boxes(xd, **kw)
    assert got_m.dtype == torch.uint8 and got_b.dtype == torch.int32 and got_b.is_cuda
    assert torch.equal(got_m.cpu(), torch.from_numpy(want_m)), "the vote differs"
    assert torch.equal(got_b.cpu(), torch.from_numpy(want_b)), "the reduction differs"
    return want_b


@pytest.mark.parametrize("shape", emu.SHAPES)
def test_masks_and_boxes(dev, shape):
    """The committed disc-plus-salt cases of this shape in one batch, then dense noise (votes near
    181 everywhere, so an off-by-one in either count shows)."""
    h, w = shape
    cases = [c for c in golden_cases() if c[1] == shape]
    assert len(cases) == 3
    x = np.stack([emu.disc_frame(h, w, seed) for seed, _, _, _ in cases])
    got = _check(x, dev)
    assert got.tolist() == [b for _, _, b, _ in cases]
    m = frames.margin_mask(_dev(x, dev)).cpu().numpy()
    for i, (_, _, _, sha) in enumerate(cases):
        assert hashlib.sha256(m[i].tobytes()).hexdigest() == sha
    # a batch that starts at any byte (a view from frame 1 on), as every later frame does
    xd = _dev(x, dev)
    assert torch.equal(frames.margin_boxes(xd[1:]).cpu(), torch.from_numpy(got[1:]))
    assert torch.equal(frames.frame_sums(xd[1:]), frames.frame_sums(xd)[1:])
    rng = np.random.default_rng(h * 1000 + w)
    noise = (rng.random((2, h, w, 1)) < 0.5) * np.ones((1, 1, 1, 3)) * 200
    _check(noise.astype(np.uint8), dev)


def test_black_and_bright(dev):
    black = np.zeros((1, 48, 64, 3), np.uint8)
    bright = np.full((1, 48, 64, 3), 200, np.uint8)
    assert _check(black, dev).tolist() == [[0, 48, 0, 64]]
    assert _check(bright, dev).tolist() == [[0, 47, 10, 53]]
    assert _check(np.full((1, 19, 21, 3), 200, np.uint8), dev).tolist() == [[0, 19, 0, 21]]
    assert _check(np.full((1, 33, 20, 3), 200, np.uint8), dev).tolist() == [[0, 33, 0, 20]]
    assert _check(np.full((2, 1, 1, 3), 200, np.uint8), dev).tolist() == [[0, 1, 0, 1]] * 2


def test_grey_15_and_16(dev):
    """Left half grey exactly 15 (below the threshold), right half exactly 16, each from several
    RGB triples: the threshold sits between them."""
    r, g, b = np.meshgrid(np.arange(64), np.arange(40), np.arange(64), indexing="ij")
    tri = np.stack([r, g, b], axis=-1).reshape(-1, 3).astype(np.uint8)
    gr = emu.grey(tri)
    t15, t16 = tri[gr == 15], tri[gr == 16]
    assert len(t15) > 100 and len(t16) > 100
    rng = np.random.default_rng(3)
    x = np.zeros((1, 48, 64, 3), np.uint8)
    x[0, :, :32] = t15[rng.integers(0, len(t15), size=(48, 32))]
    x[0, :, 32:] = t16[rng.integers(0, len(t16), size=(48, 32))]
    assert len(np.unique(x[0, :, :32].reshape(-1, 3), axis=0)) > 20
    assert (emu.grey(x[0, :, :32]) == 15).all() and (emu.grey(x[0, :, 32:]) == 16).all()
    assert _check(x, dev).tolist() == [[0, 47, 32, 53]]


def test_mixed_batch_stream_and_workspace(dev):
    """Frames whose boxes differ in one batch; a non-default stream; one workspace used twice."""
    h, w = 120, 214
    a = np.stack([emu.disc_frame(h, w, 0), np.zeros((h, w, 3), np.uint8), emu.disc_frame(h, w, 1),
                  np.full((h, w, 3), 90, np.uint8), emu.disc_frame(h, w, 2)])
    b = a[::-1].copy()
    want_a = _check(a, dev)
    assert len(set(map(tuple, want_a.tolist()))) == 5
    nb = frames.query("tmr_margin_ws_bytes", 5, h, w)
    ws = torch.empty(nb // 8, dtype=torch.int64, device=dev)
    s = torch.cuda.Stream(device=dev)
    ad, bd = _dev(a, dev), _dev(b, dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(s):
        first = frames.margin_boxes(ad, ws=ws)
        second = frames.margin_boxes(bd, ws=ws)
        third = frames.margin_mask(ad, ws=ws)
    s.synchronize()
    assert torch.equal(first.cpu(), torch.from_numpy(want_a))
    assert torch.equal(second.cpu(), torch.from_numpy(want_a[::-1].copy()))
    assert torch.equal(third.cpu(), torch.from_numpy(np.stack([emu.mask(f) for f in a])))
    with pytest.raises(RuntimeError, match="workspace of"):
        frames.margin_boxes(ad, ws=ws[:-1])


def test_frame_sums_and_mean_std(dev):
    rng = np.random.default_rng(4)
    for shape in ((3, 37, 131), (2, 224, 224), (1, 1, 1)):
        x = rng.integers(0, 256, size=shape + (3,), dtype=np.uint8)
        x[0, ..., 2] = 255                       # the largest sums a channel can have
        a = x.astype(np.int64)
        want = np.stack([a.sum(axis=(1, 2)), (a * a).sum(axis=(1, 2))], axis=-1)
        got = frames.frame_sums(_dev(x, dev))
        assert got.dtype == torch.int64 and torch.equal(got.cpu(), torch.from_numpy(want)), shape
        mean, std = frames.mean_std(_dev(x, dev))
        m64, s64 = emu.mean_std_f64(x)
        assert np.abs(mean - m64).max() <= 1e-12 and np.abs(std - s64).max() <= 1e-12


# ------------------------------------------------------------------ boxed resize
H, W = 270, 520
BOXES = [[10, 260, 20, 270],      # 250 x 250: both passes skipped, the crop's own bytes
         [0, 270, 100, 350],      # 250 wide: the horizontal pass is skipped
         [3, 253, 0, 520],        # 250 high: the vertical pass is skipped
         [5, 6, 7, 8],            # 1 x 1
         [0, 270, 0, 520],        # the full frame: downscaling both ways
         [100, 140, 300, 360],    # upscaling both ways
         [0, 270, 200, 260]]      # down one way, up the other


@pytest.fixture(scope="module")
def boxed(dev):
    rng = np.random.default_rng(5)
    x = rng.integers(0, 256, size=(len(BOXES), H, W, 3), dtype=np.uint8)
    xd = _dev(x, dev)
    out = frames.resize_frames(xd, boxes=np.array(BOXES))
    return x, xd, out


def test_boxed_resize_vs_dense(boxed):
    x, xd, out = boxed
    assert tuple(out.shape) == (len(BOXES), 250, 250, 3)
    for i, (r0, r1, c0, c1) in enumerate(BOXES):
        want = frames.resize_frames(xd[i:i + 1, r0:r1, c0:c1].contiguous())
        assert torch.equal(out[i:i + 1], want), BOXES[i]
    assert torch.equal(out[0], xd[0, 10:260, 20:270])


def test_boxed_resize_vs_pillow(boxed):
    x, xd, out = boxed
    got = out.cpu().numpy()
    for i, (r0, r1, c0, c1) in enumerate(BOXES):
        want = Image.fromarray(x[i], "RGB").crop((c0, r0, c1, r1)).resize((250, 250), Image.BILINEAR)
        assert np.array_equal(got[i], np.asarray(want)), BOXES[i]


def test_boxed_resize_arguments(boxed, dev):
    x, xd, out = boxed
    # device boxes (read to the host once), another output size, a caller's output buffer
    bd = torch.tensor(BOXES, dtype=torch.int32, device=dev)
    assert torch.equal(frames.resize_frames(xd, boxes=bd), out)
    buf = torch.zeros((len(BOXES), 40, 33, 3), dtype=torch.uint8, device=dev)
    small = frames.resize_frames(xd, (40, 33), out=buf, boxes=bd)
    assert small.data_ptr() == buf.data_ptr()
    for i, (r0, r1, c0, c1) in enumerate(BOXES):
        want = frames.resize_frames(xd[i:i + 1, r0:r1, c0:c1].contiguous(), (40, 33))
        assert torch.equal(small[i:i + 1], want), BOXES[i]
    # boxes=None is the dense path
    dense = frames.resize_frames(xd[:2], boxes=None)
    assert torch.equal(dense, frames.resize_frames(xd[:2]))
    assert np.array_equal(dense[0].cpu().numpy(), resize_ref.resize_ref(x[0], 250, 250))
    for bad in ([0, 271, 0, 520], [0, 270, -1, 520], [7, 7, 0, 520]):
        with pytest.raises(RuntimeError, match="outside the 270 x 520 frame"):
            frames.resize_frames(xd[:1], boxes=[bad])
    with pytest.raises(RuntimeError, match=r"boxes must be \(7, 4\)"):
        frames.resize_frames(xd, boxes=BOXES[:3])


def test_load_frames_cut_margin(dev, tmp_path):
    """Files -> decode -> boxes -> boxed resize on the device == decode, the emulated box and
    Pillow's crop().resize() on the host; with the host decoder and with the device one."""
    from tmrnet_amd.jpeg import DeviceJpegDecoder
    paths = []
    for i in range(3):
        p = str(tmp_path / ("%03d.jpg" % i))
        Image.fromarray(emu.disc_frame(120, 214, 10 + i, salt=0.01), "RGB").save(p, quality=92)
        paths.append(p)
    want = []
    for p in paths:
        img = frames.pil_loader(p)
        r0, r1, c0, c1 = emu.box(np.asarray(img))
        assert (r1 - r0, c1 - c0) != (120, 214)
        want.append(np.asarray(img.crop((c0, r0, c1, r1)).resize((250, 250), Image.BILINEAR)))
    want = torch.from_numpy(np.stack(want))
    assert torch.equal(frames.load_frames(paths, device=dev, cut_margin=True).cpu(), want)
    dec = DeviceJpegDecoder(workers=2, device=dev)
    assert torch.equal(frames.load_frames(paths, decoder=dec, cut_margin=True).cpu(), want)
    plain = frames.load_frames(paths, device=dev)
    assert not torch.equal(plain.cpu(), want)
