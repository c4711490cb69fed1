"""The device entropy decoder (tmrnet_amd/csrc/jpeg_entropy.hip) on the device.  The kernel
against the host decoder, bit for bit with status 0: every restart-free fixture of
tests/golden/jpeg_cases.npz alone at sub_bits 64, 256 and the default, the same-size same-class
fixtures in one call, and generated files that reach the remaining branches (more subsequences
than the workgroup has lanes, DC-only blocks, stuffed bytes, optimised tables, less than one
subsequence, a ragged grid, one component, per-frame tables in one call).  Then
DeviceJpegDecoder(entropy="device") against Pillow, its counters, a second call, a second stream,
two batches in flight, and the refusals.  Corrupted input runs here only in the forms the
sanitized CPU driver (tests/test_jpeg_entropy_cpu.py) runs too."""
import ctypes
import io

import numpy as np
import pytest
import torch
from PIL import Image

from tests import _jpeg_emu as emu
from tmrnet_amd import _lib, jpeg
from tmrnet_amd.jpeg import DeviceJpegDecoder

pytestmark = pytest.mark.gpu
CASES = emu.load_cases()
OK = [c for c in CASES if c[1] == "ok"]
BY_NAME = {c[0]: c for c in CASES}
PACKED = [c for c in OK if not (c[0].endswith("_rst3") or c[0].endswith("_rstrow"))]
SUBS = (64, 256, 0)
HUFF = ctypes.sizeof(_lib.JpegHuff)
DESC = ctypes.sizeof(_lib.JpegScanDesc)


def _host(data):
    """(info, coefficients) of the host decoder."""
    p = jpeg.probe(data)
    assert p.status == 0, p
    info = _lib.JpegInfo()
    coef = np.full(p.coef_bytes // 2, 0x5a5a, dtype=np.int16)
    rc = _lib.lib().tmr_jpeg_entropy_decode(data, len(data), ctypes.byref(info), coef.ctypes.data,
                                            coef.nbytes)
    assert rc == 0, _lib.lib().tmr_last_error()
    return info, torch.from_numpy(coef)


def _pack_batch(files):
    """One buffer: descriptors, then per frame its tables and bits.  -> (buffer, infos, max_bits)"""
    n = len(files)
    at = (n * DESC + 15) // 16 * 16
    offs = []
    for d in files:
        cap = (len(d) + 8 + 15) // 16 * 16
        offs.append((at, at + _lib.JPEG_MAX_TABLES * HUFF, cap))
        at += _lib.JPEG_MAX_TABLES * HUFF + cap
    buf = np.zeros(at, dtype=np.uint8)
    infos, bits = [], []
    for j, (d, (t, b, cap)) in enumerate(zip(files, offs)):
        info = _lib.JpegInfo()
        rc = _lib.lib().tmr_jpeg_scan_pack(d, len(d), ctypes.byref(info), buf.ctypes.data + b, cap, b,
                                           buf.ctypes.data + t, _lib.JPEG_MAX_TABLES * HUFF, t,
                                           buf.ctypes.data + j * DESC)
        assert rc == 0, _lib.lib().tmr_last_error()
        infos.append(info)
        bits.append(_lib.JpegScanDesc.from_buffer_copy(buf[j * DESC:(j + 1) * DESC].tobytes()).nbits)
    return buf, infos, max(bits)


def _kernel(dev, files, sub_bits=0):
    """(status, coefficients (f, n) int16, rounds) of one call on `files`, all of one size and class."""
    buf, infos, max_bits = _pack_batch(files)
    i0 = infos[0]
    f, cb = len(files), int(i0.coef_bytes)
    dbuf = torch.from_numpy(buf).to(dev)
    coef = torch.full((f, cb // 2), 0x5a5a, dtype=torch.int16, device=dev)
    status = torch.full((f,), -7, dtype=torch.int32, device=dev)
    nb = _lib.query("tmr_jpeg_entropy_ws_bytes", f, max_bits, sub_bits)
    ws = torch.zeros(nb, dtype=torch.uint8, device=dev)
    _lib.call("tmr_jpeg_entropy_decode_device", dbuf, dbuf, ctypes.c_size_t(buf.size), f, i0.height,
              i0.width, i0.sampling, max_bits, sub_bits, coef, status, ws, ctypes.c_size_t(nb),
              _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    return status.cpu(), coef.cpu(), ws[:4 * f].view(torch.int32).cpu(), max_bits


def _check(dev, files, sub_bits, what):
    status, coef, rounds, max_bits = _kernel(dev, files, sub_bits)
    assert status.tolist() == [0] * len(files), (what, sub_bits, status.tolist())
    for j, d in enumerate(files):
        assert torch.equal(coef[j], _host(d)[1]), (what, sub_bits, j)
    return rounds, max_bits


@pytest.mark.parametrize("sub_bits", SUBS)
def test_kernel_equals_host_on_each_fixture(dev, sub_bits):
    assert len(PACKED) == 66
    for name, _, _, _, data in PACKED:
        _check(dev, [data], sub_bits, name)


@pytest.mark.parametrize("sub_bits", SUBS)
def test_kernel_equals_host_on_same_class_fixtures_in_one_call(dev, sub_bits):
    groups = {}
    for name, _, size, _, data in PACKED:
        groups.setdefault((size, jpeg.probe(data).sampling), []).append(data)
    many = [v for v in groups.values() if len(v) > 1]
    assert len(many) >= 5 and max(len(v) for v in many) >= 4
    for (size, cls), files in groups.items():
        if len(files) > 1:
            _check(dev, files, sub_bits, (size, cls))


def _jpeg(img, mode="RGB", **kw):
    buf = io.BytesIO()
    Image.fromarray(img, mode).save(buf, "JPEG", **kw)
    return buf.getvalue()


def _noise(h, w, seed, saturated=False):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return np.where(a < 128, 0, 255).astype(np.uint8) if saturated else a


def _generated():
    smooth = np.stack(list(np.meshgrid(np.arange(29), np.arange(37))) + [np.full((37, 29), 90)], -1)
    smooth = (smooth * 5 % 256).astype(np.uint8)
    return {
        "noise_640x480_420_q95": [_jpeg(_noise(480, 640, 1), quality=95, subsampling=2)],
        "flat_320x240": [_jpeg(np.full((240, 320, 3), (200, 30, 90), dtype=np.uint8), quality=90,
                               subsampling=2)],
        "sat_214x120_444_q100": [_jpeg(_noise(120, 214, 2, saturated=True), quality=100, subsampling=0)],
        "optimized_214x120": [_jpeg(_noise(120, 214, 3), quality=80, subsampling=2, optimize=True)],
        "tiny_8x8": [_jpeg(np.full((8, 8, 3), 17, dtype=np.uint8), quality=75, subsampling=0)],
        "ragged_37x29": [_jpeg(smooth, quality=85, subsampling=2)],
        "gray_50x70": [_jpeg(_noise(70, 50, 4)[..., 0], mode="L", quality=85)],
        "two_frames_own_tables": [_jpeg(_noise(50, 70, 5), quality=60, subsampling=2, optimize=True),
                                  _jpeg(smooth.repeat(2, 0).repeat(3, 1)[:50, :70], quality=97,
                                        subsampling=2, optimize=True)],
    }


GENERATED = _generated()


@pytest.mark.parametrize("name", list(GENERATED))
def test_kernel_equals_host_on_generated_cases(dev, name):
    files = GENERATED[name]
    descs = [_lib.JpegScanDesc.from_buffer_copy(_pack_batch([d])[0][:DESC].tobytes()) for d in files]
    if name == "noise_640x480_420_q95":   # more subsequences than the workgroup has lanes
        assert descs[0].nbits > 1024 * 1024, descs[0].nbits
    if name == "tiny_8x8":                # fewer bits than one subsequence
        assert descs[0].nbits < 64, descs[0].nbits
    if name == "sat_214x120_444_q100":    # stuffed bytes were there to remove
        assert b"\xff\x00" in files[0][files[0].index(b"\xff\xda"):]
    if name == "gray_50x70":
        assert descs[0].ncomp == 1 and descs[0].mcu_blocks == 1
    if name == "two_frames_own_tables":
        assert _pack_batch(files[:1])[0][DESC:DESC + 2 * HUFF].tobytes() != \
            _pack_batch(files[1:])[0][DESC:DESC + 2 * HUFF].tobytes()
    for sub_bits in ((256, 0) if name == "noise_640x480_420_q95" else SUBS):
        rounds, _ = _check(dev, files, sub_bits, name)
        print(name, "sub_bits", sub_bits, "rounds", rounds.tolist())
        if name == "noise_640x480_420_q95":
            assert rounds.item() > 1   # speculation had to be corrected over several rounds


# ---- the decoder ----
@pytest.fixture(scope="module")
def dec(dev):
    with DeviceJpegDecoder(workers=4, device=dev, entropy="device") as d:
        yield d


@pytest.fixture(scope="module")
def pil():
    return {c[0]: torch.from_numpy(emu.pil_rgb(c[4]).copy()) for c in CASES if c[1] != "malformed"}


def test_decoder_equals_pillow_on_every_fixture(dec, pil):
    before = dict(dec.stats)
    for name, _, (h, w), sha, data in OK:
        out = dec.decode([data]).cpu()
        assert tuple(out.shape) == (1, h, w, 3) and out.dtype == torch.uint8, name
        assert torch.equal(out[0], pil[name]), name
        assert emu.sha(out[0].numpy()) == sha, name
    assert dec.stats["device"] - before["device"] == len(OK)
    assert dec.stats["entropy_device"] - before["entropy_device"] == len(PACKED)
    assert dec.stats["entropy_host"] - before["entropy_host"] == len(OK) - len(PACKED)
    assert dec.stats["fallback"] == before["fallback"]


def test_decoder_mixed_batch(dec, pil):
    names = ["smooth_37x29_420_q75", "smooth_37x29_444_q90", "smooth_37x29_420_rst3",
             "progressive_37x29", "png_37x29", "smooth_37x29_gray_q75", "smooth_37x29_420_q3"]
    before = dict(dec.stats)
    out = dec.decode([BY_NAME[n][4] for n in names]).cpu()
    for i, n in enumerate(names):
        assert torch.equal(out[i], pil[n]), n
    diff = {k: dec.stats[k] - before[k] for k in before}
    assert diff == {"device": 5, "fallback": 2, "entropy_device": 4, "entropy_host": 1}
    assert diff["entropy_device"] + diff["entropy_host"] == diff["device"]
    assert diff["device"] + diff["fallback"] == len(names)
    # the restart-per-row files are 70x50: the same mix of routes at their size
    names = ["noise_70x50_420_q75", "noise_70x50_420_rstrow", "sat_70x50_420_q100", "sat_70x50_420_rstrow"]
    before = dict(dec.stats)
    out = dec.decode([BY_NAME[n][4] for n in names]).cpu()
    for i, n in enumerate(names):
        assert torch.equal(out[i], pil[n]), n
    diff = {k: dec.stats[k] - before[k] for k in before}
    assert diff == {"device": 4, "fallback": 0, "entropy_device": 2, "entropy_host": 2}


def test_decoder_second_call_other_stream_and_two_in_flight(dec, dev, pil):
    names = ["noise_70x50_420_q75", "sat_70x50_420_q100", "noise_70x50_420_q3"]
    files = [BY_NAME[n][4] for n in names]
    first = dec.decode(files)
    second = dec.decode(files)
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        third = dec.decode(files)
    side.synchronize()
    jobs = [dec.submit(files), dec.submit(files[::-1])]
    fourth, fifth = jobs[0].result(), jobs[1].result()
    torch.cuda.synchronize()
    for i, n in enumerate(names):
        assert torch.equal(first[i].cpu(), pil[n]), n
    assert torch.equal(first, second) and torch.equal(first, third) and torch.equal(first, fourth)
    assert torch.equal(first, fifth.flip(0))
    with DeviceJpegDecoder(workers=2, device=dev) as host:   # and the default route's bytes
        assert host.entropy == "host" and torch.equal(host.decode(files), first)


def test_decoder_load_frames_and_kernel_events(dec, dev, tmp_path):
    from tmrnet_amd import frames
    paths = []
    for n in ("noise_214x120_420_q75", "sat_214x120_420_q3", "noise_214x120_444_q95",
              "sat_214x120_420_rstrow"):
        p = str(tmp_path / (n + ".jpg"))
        with open(p, "wb") as f:
            f.write(BY_NAME[n][4])
        paths.append(p)
    dec.kernel_events, dec.entropy_events, dec.entropy_rounds = [], [], []
    try:
        a = frames.load_frames(paths, device=dev, decoder=dec)
    finally:
        events, dec.kernel_events = dec.kernel_events, None
    assert torch.equal(a, frames.load_frames(paths, device=dev))
    torch.cuda.synchronize()
    assert len(events) == 1 and len(dec.entropy_events) == 1 and len(dec.entropy_rounds) == 3
    assert 0 < dec.entropy_events[0][0].elapsed_time(dec.entropy_events[0][1]) <= \
        events[0][0].elapsed_time(events[0][1])


# ---- refusals ----
def test_bad_arguments_are_refused_before_any_launch(dev):
    calls = []
    real = jpeg.call
    jpeg.call = lambda *a, **k: calls.append(a[0]) or real(*a, **k)
    try:
        with pytest.raises(RuntimeError, match="entropy must be"):
            DeviceJpegDecoder(device=dev, entropy="gpu")
        for sub in (32, 100, -64):
            with pytest.raises(RuntimeError, match="sub_bits"):
                DeviceJpegDecoder(device=dev, entropy="device", sub_bits=sub)
    finally:
        jpeg.call = real
    assert calls == []

    data = BY_NAME["smooth_37x29_420_q75"][4]
    buf, infos, max_bits = _pack_batch([data, data])
    h, w, s = infos[0].height, infos[0].width, infos[0].sampling
    dbuf = torch.from_numpy(buf).to(dev)
    cb = int(infos[0].coef_bytes)
    coef = torch.full((2, cb // 2), 0x5a5a, dtype=torch.int16, device=dev)
    status = torch.full((2,), -7, dtype=torch.int32, device=dev)
    nb = _lib.query("tmr_jpeg_entropy_ws_bytes", 2, max_bits, 0)
    ws = torch.zeros(nb, dtype=torch.uint8, device=dev)

    def run(desc=dbuf, buf=dbuf, f=2, h=h, w=w, s=s, sub=0, coef=coef, status=status, ws=ws, nb=nb):
        _lib.call("tmr_jpeg_entropy_decode_device", desc, buf, ctypes.c_size_t(dbuf.numel()), f, h, w,
                  s, max_bits, sub, coef, status, ws, ctypes.c_size_t(nb), _lib.stream_ptr(dev))

    name = "tmr_jpeg_entropy_decode_device: "
    for null in ("desc", "buf", "coef", "status", "ws"):
        with pytest.raises(RuntimeError, match=name + "null operand"):
            run(**{null: None})
    for bad in (dict(f=0), dict(f=-1), dict(w=0), dict(s=3), dict(h=70000)):
        with pytest.raises(RuntimeError, match=name + "bad sizes"):
            run(**bad)
    for sub in (32, 100, -64):
        with pytest.raises(RuntimeError, match=name + "sub_bits"):
            run(sub=sub)
    with pytest.raises(RuntimeError, match=name + "workspace"):
        run(nb=nb - 1)
    with pytest.raises(RuntimeError, match="aligned"):
        run(coef=coef.view(-1)[4:])
    torch.cuda.synchronize()
    assert status.tolist() == [-7, -7] and bool((coef == 0x5a5a).all())   # nothing ran
    # a descriptor that does not fit the arguments: status 3, the frame left alone
    run(h=h + 16)
    torch.cuda.synchronize()
    assert status.tolist() == [3, 3] and bool((coef == 0x5a5a).all())
    run()
    torch.cuda.synchronize()
    assert status.tolist() == [0, 0] and torch.equal(coef[0].cpu(), _host(data)[1])


def test_malformed_files_raise_what_the_host_route_raises(dev):
    data = BY_NAME["noise_70x50_420_q75"][4]
    cut = data[:len(data) * 9 // 10]   # the cut of tests/test_jpeg_cpu.py: inside the scan
    bad = [cut] + [c[4] for c in CASES if c[1] == "malformed"]
    assert len(bad) == 3
    # and a scan the probe lets through but the entropy decoders run off the end of: the status
    # word sends it to the host pass, whose message it is (an input the sanitized driver runs)
    from tests.test_jpeg_entropy_cpu import cut_scan
    bad.append(cut_scan(data))
    assert jpeg.probe(bad[-1]).status == 0
    with DeviceJpegDecoder(workers=2, device=dev) as host, \
            DeviceJpegDecoder(workers=2, device=dev, entropy="device") as device:
        for d in bad:
            with pytest.raises(RuntimeError) as a:
                host.decode([d])
            with pytest.raises(RuntimeError) as b:
                device.decode([d])
            assert str(a.value) == str(b.value)
        assert "tmr_jpeg_entropy_decode failed (1)" in str(b.value) and "truncated" in str(b.value)
        out = device.decode([data])   # and the decoder is still good afterwards
        assert torch.equal(out[0].cpu(), torch.from_numpy(emu.pil_rgb(data).copy()))


def test_truncated_scan_gets_a_status_not_coefficients(dev):
    """The kernel itself on a scan that ends early: the probe's end-marker check is what stops
    such a file in the decoder, so here the file keeps its end marker and loses the tenth of the
    scan before it -- an input the sanitized CPU driver runs too (test_jpeg_entropy_cpu.CUT)."""
    from tests.test_jpeg_entropy_cpu import cut_scan
    data = BY_NAME["noise_70x50_420_q75"][4]
    cut = cut_scan(data)
    info = _lib.JpegInfo()
    coef = np.zeros(jpeg.probe(data).coef_bytes // 2, dtype=np.int16)
    assert _lib.lib().tmr_jpeg_entropy_decode(cut, len(cut), ctypes.byref(info), coef.ctypes.data,
                                              coef.nbytes) == 1
    for sub_bits in SUBS:
        status = _kernel(dev, [cut], sub_bits)[0]
        assert status.item() != 0, sub_bits
