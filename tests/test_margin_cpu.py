"""Black-margin cut without a GPU: the numpy emulation against scipy's median,
the committed boxes and OpenCV's grey; the host argument checks of the new entry points; the
normalisation statistic from integer sums."""
import ctypes
import os

import numpy as np
import pytest

from tests import _margin_emu as emu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "margin_cases.npz")


def golden_cases():
    g = np.load(GOLDEN)
    return [(int(s), tuple(int(v) for v in hw), [int(v) for v in b], str(sha))
            for s, hw, b, sha in zip(g["seeds"], g["shapes"], g["boxes"], g["mask_sha256"])]


def test_majority_vote_is_scipys_median():
    ndi = pytest.importorskip("scipy.ndimage")
    for h, w in emu.SHAPES:
        for seed in (0, 1):
            m = emu.grey(emu.disc_frame(h, w, seed)) > emu.THRESH
            want = ndi.median_filter(m.astype(np.uint8), size=emu.WIN, mode="nearest")
            assert np.array_equal(emu.majority(m), want.astype(bool)), (h, w, seed)
        rng = np.random.default_rng(h * 1000 + w)      # dense noise: votes near the threshold
        m = rng.random((h, w)) < 0.5
        want = ndi.median_filter(m.astype(np.uint8), size=emu.WIN, mode="nearest")
        assert np.array_equal(emu.majority(m), want.astype(bool)), (h, w)


def test_boxes_equal_the_committed_ones():
    cases = golden_cases()
    assert sorted(set(hw for _, hw, _, _ in cases)) == sorted(emu.SHAPES)
    for seed, (h, w), want, sha in cases:
        f = emu.disc_frame(h, w, seed)
        assert emu.box(f) == want, (h, w, seed)
        assert emu.mask_sha(f) == sha, (h, w, seed)
    # the cases are not degenerate: a proper crop wherever the shape admits one
    proper = [hw for _, hw, b, _ in cases if b != [0, hw[0], 0, hw[1]]]
    assert set(proper) == {(48, 64), (37, 131), (40, 41), (7, 90), (120, 214)}


def test_fallbacks_and_simple_frames():
    assert emu.box(np.zeros((48, 64, 3), np.uint8)) == [0, 48, 0, 64]
    assert emu.box(np.full((48, 64, 3), 200, np.uint8)) == [0, 47, 10, 53]
    assert emu.box(np.full((19, 21, 3), 200, np.uint8)) == [0, 19, 0, 21]    # c0 == c1
    assert emu.box(np.full((33, 20, 3), 200, np.uint8)) == [0, 33, 0, 20]    # no admissible column
    one_row = np.zeros((40, 64, 3), np.uint8)
    one_row[:10] = 200                        # rows 0..9 of 40: the vote keeps rows 0..9
    assert emu.box(one_row) == [0, 9, 10, 53]


def test_grey_tables_differ_only_at_the_threshold():
    """The 15-bit table (OpenCV 4) and the older 14-bit one can disagree about g > 15 only for
    pixels whose grey lands on 15 or 16 (which one the reference ran is unpinned)."""
    rng = np.random.default_rng(0)
    rgb = rng.integers(0, 256, size=(200000, 3), dtype=np.uint8)
    rgb[:50000] = rng.integers(0, 48, size=(50000, 3), dtype=np.uint8)
    a, b = emu.grey(rgb).astype(int), emu.grey14(rgb).astype(int)
    assert np.abs(a - b).max() <= 1
    differ = (a > 15) != (b > 15)
    assert np.isin(a[differ], (15, 16)).all()


def test_grey_is_opencvs():
    cv2 = pytest.importorskip("cv2")
    rng = np.random.default_rng(1)
    rgb = rng.integers(0, 256, size=(64, 4096, 3), dtype=np.uint8)
    rgb[:32] = rng.integers(0, 40, size=(32, 4096, 3), dtype=np.uint8)
    bgr = np.ascontiguousarray(rgb[..., ::-1])
    assert np.array_equal(emu.grey(rgb), cv2.cvtColor(bgr, cv2.COLOR_BGR2GRAY))
    f = emu.disc_frame(120, 214, 0)
    g = cv2.cvtColor(np.ascontiguousarray(f[..., ::-1]), cv2.COLOR_BGR2GRAY)
    _, binary = cv2.threshold(g, 15, 255, cv2.THRESH_BINARY)
    assert np.array_equal(cv2.medianBlur(binary, 19), emu.mask(f))


def test_host_argument_checks():
    """Every check of the new entry points runs on the host before any launch: they fail here,
    with no GPU, on null pointers, n <= 0, a short workspace and a box outside the frame."""
    from tmrnet_amd import _lib
    buf = np.zeros(1 << 16, dtype=np.int64)
    p = buf.ctypes.data
    for entry in ("tmr_margin_boxes", "tmr_margin_mask"):
        with pytest.raises(RuntimeError, match=entry + ": null operand"):
            _lib.call(entry, None, 1, 8, 8, p, ctypes.c_size_t(buf.nbytes), p, None)
        with pytest.raises(RuntimeError, match=entry + ": null operand"):
            _lib.call(entry, p, 1, 8, 8, None, ctypes.c_size_t(buf.nbytes), p, None)
        with pytest.raises(RuntimeError, match=entry + ": null operand"):
            _lib.call(entry, p, 1, 8, 8, p, ctypes.c_size_t(buf.nbytes), None, None)
        with pytest.raises(RuntimeError, match=entry + ": bad shape"):
            _lib.call(entry, p, 0, 8, 8, p, ctypes.c_size_t(buf.nbytes), p, None)
        with pytest.raises(RuntimeError, match=entry + ": bad shape"):
            _lib.call(entry, p, 1, 8, -3, p, ctypes.c_size_t(buf.nbytes), p, None)
        need = _lib.query("tmr_margin_ws_bytes", 2, 37, 131)
        assert need == 2 * 3 * 16 + 2 * 37 * 3 * 8      # a slot per 64 x 64 tile, a word per 64 pixels
        with pytest.raises(RuntimeError, match=entry + ": workspace of"):
            _lib.call(entry, p, 2, 37, 131, p, ctypes.c_size_t(need - 1), p, None)
    with pytest.raises(RuntimeError, match="tmr_margin_ws_bytes"):
        _lib.query("tmr_margin_ws_bytes", 0, 8, 8)
    with pytest.raises(RuntimeError, match="tmr_frame_sums: null operand"):
        _lib.call("tmr_frame_sums", None, 1, 8, 8, p, None)
    with pytest.raises(RuntimeError, match="tmr_frame_sums: bad shape"):
        _lib.call("tmr_frame_sums", p, -1, 8, 8, p, None)

    def boxes(desc, n=1, h=40, w=60, pool_ints=0, tmp=None, tmp_bytes=0, null=None):
        d = np.asarray(desc, dtype=np.int32)
        args = [p, n, h, w, d.ctypes.data, p, p, pool_ints, tmp, ctypes.c_size_t(tmp_bytes), p,
                25, 25, None]
        if null is not None:
            args[null] = None
        _lib.call("tmr_resize_u8_boxes", *args)

    ks = _lib.query("tmr_resize_ksize", 30, 25)
    good = [0, 30, 10, 40, 0, 50, ks, 0, 50, ks]
    with pytest.raises(RuntimeError, match="tmr_resize_u8_boxes: bad arguments"):
        boxes(good, null=0)
    with pytest.raises(RuntimeError, match="tmr_resize_u8_boxes: bad arguments"):
        boxes(good, null=4)
    with pytest.raises(RuntimeError, match="tmr_resize_u8_boxes: bad arguments"):
        boxes(good, n=0)
    for bad in ([0, 41, 10, 40], [-1, 30, 10, 40], [0, 30, 10, 61], [5, 5, 10, 40], [0, 30, 40, 10]):
        with pytest.raises(RuntimeError, match="outside 40 x 60"):
            boxes(bad + good[4:], pool_ints=50 + 25 * ks)
    with pytest.raises(RuntimeError, match="has ksize"):
        boxes(good[:6] + [ks + 2] + good[7:], pool_ints=50 + 25 * ks)
    with pytest.raises(RuntimeError, match="horizontal tables of frame 0 outside the pool"):
        boxes(good, pool_ints=50 + 25 * ks - 1)
    with pytest.raises(RuntimeError, match="tmp missing or smaller"):
        boxes(good, pool_ints=50 + 25 * ks, tmp=p, tmp_bytes=40 * 25 * 3 - 1)


def test_mean_std_from_integer_sums():
    from tmrnet_amd.frames import mean_std_from_sums
    rng = np.random.default_rng(2)
    frames = rng.integers(0, 256, size=(3, 224, 224, 3), dtype=np.uint8)
    frames[1] = (frames[1] // 8)               # a dark frame
    frames[2, :, :, 1] = 77                    # a constant channel: std exactly 0
    a = frames.astype(np.int64)
    sums = np.stack([a.sum(axis=(1, 2)), (a * a).sum(axis=(1, 2))], axis=-1)   # (F, 3, 2)
    mean, std = mean_std_from_sums(sums, 224 * 224)
    m64, s64 = emu.mean_std_f64(frames)
    assert np.abs(mean - m64).max() <= 1e-12 and np.abs(std - s64).max() <= 1e-12
    m32, s32 = emu.mean_std_f32(frames)
    assert np.abs(mean - m32).max() <= 1e-5 and np.abs(std - s32).max() <= 1e-5
    one = mean_std_from_sums(sums[2:], 224 * 224)
    assert one[1][1] == 0.0
