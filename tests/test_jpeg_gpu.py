"""tmrnet_amd.jpeg.DeviceJpegDecoder on the device: host entropy decode + tmr_jpeg_reconstruct
(jpeg.hip) equal Pillow's decode -- pil_loader, train_only_non-local_pretrained.py:96-99 -- byte
for byte on the fixtures of tests/golden/jpeg_cases.npz (this machine's Pillow and the committed
hashes), alone, in batches with per-frame tables and mixed sampling classes, with PIL fallbacks in
the batch, through load_frames, on a second call and on another stream; bad arguments are refused
by name before any launch."""
import ctypes
import io

import numpy as np
import pytest
import torch
from PIL import Image

from tests import _jpeg_emu as emu
from tmrnet_amd import _lib, frames
from tmrnet_amd.jpeg import DeviceJpegDecoder

pytestmark = pytest.mark.gpu
CASES = emu.load_cases()
OK = [c for c in CASES if c[1] == "ok"]
BY_NAME = {c[0]: c for c in CASES}


@pytest.fixture(scope="module")
def dec(dev):
    with DeviceJpegDecoder(workers=4, device=dev) as d:
        yield d


@pytest.fixture(scope="module")
def pil():
    """Pillow's decode of every fixture it can open, computed once."""
    return {c[0]: torch.from_numpy(emu.pil_rgb(c[4]).copy()) for c in CASES if c[1] != "malformed"}


def _jpeg(img, **kw):
    buf = io.BytesIO()
    Image.fromarray(img, "RGB").save(buf, "JPEG", **kw)
    return buf.getvalue()


def test_every_supported_case_alone(dec, pil):
    before = dict(dec.stats)
    for name, _, (h, w), sha, data in OK:
        out = dec.decode([data]).cpu()
        assert tuple(out.shape) == (1, h, w, 3) and out.dtype == torch.uint8, name
        assert torch.equal(out[0], pil[name]), name
        assert emu.sha(out[0].numpy()) == sha, name
    assert dec.stats["device"] - before["device"] == len(OK)
    assert dec.stats["fallback"] == before["fallback"]


def test_batch_with_per_frame_tables(dec):
    img = np.asarray(Image.open(io.BytesIO(BY_NAME["smooth_37x29_444_q90"][4])).convert("RGB"))
    files = [_jpeg(img, quality=q) for q in (10, 35, 60, 85, 98)]
    out = dec.decode(files).cpu()
    for i, f in enumerate(files):
        assert torch.equal(out[i], torch.from_numpy(emu.pil_rgb(f).copy())), i
    assert not torch.equal(out[0], out[4])


def test_batch_mixing_sampling_classes(dec, pil):
    names = ["smooth_37x29_420_q75", "smooth_37x29_444_q90", "smooth_37x29_gray_q75",
             "smooth_37x29_420_q3", "smooth_37x29_444_q90", "smooth_37x29_420_rst3"]
    out = dec.decode([BY_NAME[n][4] for n in names]).cpu()
    for i, n in enumerate(names):
        assert torch.equal(out[i], pil[n]), n


def test_fallbacks_in_the_batch_equal_decode_frames(dec, tmp_path):
    names = ["progressive_37x29", "smooth_37x29_420_q75", "422_37x29", "png_37x29"]
    paths = []
    for n in names:
        p = str(tmp_path / (n + (".png" if "png" in n else ".jpg")))
        with open(p, "wb") as f:
            f.write(BY_NAME[n][4])
        paths.append(p)
    before = dict(dec.stats)
    out = dec.decode(paths).cpu()
    assert torch.equal(out, frames.decode_frames(paths, workers=2))
    assert dec.stats["device"] - before["device"] == 1
    assert dec.stats["fallback"] - before["fallback"] == 3


def test_load_frames_with_decoder_equals_without(dec, dev, tmp_path):
    paths = []
    for n in ("noise_214x120_420_q75", "sat_214x120_420_q3", "noise_214x120_444_q95",
              "sat_214x120_420_rstrow"):
        p = str(tmp_path / (n + ".jpg"))
        with open(p, "wb") as f:
            f.write(BY_NAME[n][4])
        paths.append(p)
    a = frames.load_frames(paths, device=dev, decoder=dec)
    b = frames.load_frames(paths, device=dev)
    assert tuple(a.shape) == (4, 250, 250, 3)
    assert torch.equal(a, b)


def test_second_call_and_other_stream_give_the_same_bytes(dec, dev, pil):
    names = ["noise_70x50_420_q75", "sat_70x50_420_q100", "noise_70x50_420_q3"]
    files = [BY_NAME[n][4] for n in names]
    first = dec.decode(files)
    second = dec.decode(files)
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        third = dec.decode(files)
    side.synchronize()
    jobs = [dec.submit(files), dec.submit(files[::-1])]   # two batches in flight
    fourth, fifth = jobs[0].result(), jobs[1].result()
    torch.cuda.synchronize()
    for i, n in enumerate(names):
        assert torch.equal(first[i].cpu(), pil[n]), n
    assert torch.equal(first, second) and torch.equal(first, third) and torch.equal(first, fourth)
    assert torch.equal(first, fifth.flip(0))


def test_reconstruct_refuses_bad_arguments(dev):
    h, w = 37, 29
    nb = _lib.query("tmr_jpeg_ws_bytes", 2, h, w, 2)
    assert nb == 2 * 64 * (6 * 4 + 2 * 3 * 2)
    coef = torch.zeros(2 * nb, dtype=torch.uint8, device=dev)
    qt = torch.ones(2 * 3 * 64, dtype=torch.int16, device=dev)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    out = torch.empty((2, h, w, 3), dtype=torch.uint8, device=dev)
    s = _lib.stream_ptr(dev)

    def run(coef=coef, qt=qt, f=2, h=h, w=w, sampling=2, ws=ws, nb=nb, out=out, nout=2):
        _lib.call("tmr_jpeg_reconstruct", coef, qt, f, h, w, sampling, ws, ctypes.c_size_t(nb), out,
                  None, nout, s)

    with pytest.raises(RuntimeError, match="tmr_jpeg_reconstruct: workspace"):
        run(nb=nb - 1)
    for null in ("coef", "qt", "ws", "out"):
        with pytest.raises(RuntimeError, match="tmr_jpeg_reconstruct: null operand"):
            run(**{null: None})
    for f in (0, -3):
        with pytest.raises(RuntimeError, match="tmr_jpeg_reconstruct: bad sizes"):
            run(f=f)
    with pytest.raises(RuntimeError, match="tmr_jpeg_reconstruct: bad sizes"):
        run(sampling=3)
    with pytest.raises(RuntimeError, match="tmr_jpeg_reconstruct: bad sizes"):
        run(w=0)
    with pytest.raises(RuntimeError, match="tmr_jpeg_reconstruct: 2 frames into 1 output"):
        run(nout=1)
    with pytest.raises(RuntimeError, match="tmr_jpeg_ws_bytes"):
        _lib.query("tmr_jpeg_ws_bytes", 0, h, w, 2)
    run()   # and the same call with good arguments goes through: zero coefficients are mid grey
    assert torch.equal(out.cpu(), torch.full((2, h, w, 3), 128, dtype=torch.uint8))


def test_mismatched_frame_size_and_malformed_file_raise(dec):
    with pytest.raises(RuntimeError, match="expected"):
        dec.decode([BY_NAME["smooth_37x29_420_q75"][4], BY_NAME["smooth_29x37_420_q75"][4]])
    with pytest.raises(RuntimeError, match="tmr_jpeg_probe"):
        dec.decode([BY_NAME["smooth_37x29_420_q75"][4], BY_NAME["cut60_37x29"][4]])
    # the decoder is still good afterwards
    out = dec.decode([BY_NAME["smooth_37x29_420_q75"][4]])
    assert tuple(out.shape) == (1, 37, 29, 3)
