"""Geometries of the conv-engine tests (test_conv_engine_cpu.py, test_conv_engine_gpu.py).

Each row: (name, n, h, w, cin, cout, r, stride, pad, extras, expect).  expect maps a view to the
(engine, cfg, tapv) the fp32 launch is meant to reach (engine 2 = LDS-DMA; the dgrad with the
transposed fp32 weights, TMR_IO_WT_F32); a view that is absent is not run for the row.  The configs
are written from the rules of gemm16_select.h (pick_cfg16 with f32 = true), not recorded from the
query -- test_conv_engine_cpu.py then asks tmr_conv2d_tile whether each launch goes there.

The GEMM of a view (M rows x N columns over K):
  fwd    M = n*ho*wo  N = cout       K = r*r*cin
  dgrad  M = n*h*w    N = cin        K = r*r*cout     (stride 1; stride 2: one GEMM per parity class)
  wgrad  M = cout     N = r*r*cin    K = n*ho*wo      (split over K: extras splits / kchunk)
tiles(c) = ceil(M/bm) * ceil(N/bn) of config c.  The fp32 rules, in the order they apply:
  wgrad  M <= 64: N <= 64 or N >= 512 -> 5, else 4;  N <= 64 -> 5;
         M >= 256, N >= 256, 2*M*N*K >= 100e9 -> 6;  else 7
  dgrad  M >= 256 and N >= 512: 7 if tiles(7) >= 256 else 2 (final)
  fwd    M >= 256 and N == 128: 7 if tiles(7) >= 256 else 2 (final)
  else   N <= 64: 3 if M >= 256 else 5;  fwd with N >= 256 and M >= 256: 6;  else 2;
         then below 256 tiles (224 for config 6) step to the first of 1, 2, 5 with a smaller tile
         and more tiles, going on while that one too has fewer than 256.
TAPV (fwd / dgrad): more than one tap and channels per tap (cin; dgrad: cout) no multiple of 32.

extras: x_ld / y_ld (channel-slice operands), max_frames (frame chunks), classes (the strided
dgrad as one launch per parity class, TMR_IO_CLASSES), nclasses (parity classes with a tap),
splits / kchunk (the wgrad plan), ws (the fused dgrad qualifies for the wave-specialised launch).
"""
import contextlib
from collections import namedtuple

Case = namedtuple("Case", "name n h w cin cout r stride pad extras expect")

L = 2   # the LDS-DMA engine


def _e(fwd=None, dgrad=None, wgrad=None):
    out = {}
    for view, v in (("fwd", fwd), ("dgrad", dgrad), ("wgrad", wgrad)):
        if v is not None:
            cfg, tapv = v if isinstance(v, tuple) else (v, 0)
            out[view] = (L, cfg, tapv)
    return out


CASES = [
    # K of one partial k-tile (16 < 32); every view a single 64x64 tile
    Case("tiny", 1, 7, 7, 16, 16, 1, 1, 0, {}, _e(fwd=5, dgrad=5, wgrad=5)),
    # fwd M 429, N 128: tiles(7) = 4 -> 2.  dgrad N 64 -> 3, 2 tiles -> 5 (7 tiles).  wgrad M 128,
    # N 576 -> 7.  K = 576 = 18 whole k-tiles
    Case("c64_128_3x3", 3, 13, 11, 64, 128, 3, 1, 1, {}, _e(fwd=2, dgrad=5, wgrad=7)),
    # M = 21*57*55 = 65835 = 257*256 + 43: ragged M on 256x64 (258 tiles >= 256); wgrad 64x64
    Case("c64_64_ragM", 21, 57, 55, 64, 64, 1, 1, 0, {}, _e(fwd=3, dgrad=3, wgrad=5)),
    # the same rows with K = 8 (fwd) below one k-tile on 256x64; dgrad N = 8, one ragged column block
    Case("c8_64_k8", 21, 57, 55, 8, 64, 1, 1, 0, {}, _e(fwd=3, dgrad=3, wgrad=5)),
    # fwd M 34496, N 128: tiles(7) = 270 -> 7; 8 channels per tap: TAPV, K = 72 = 2 k-tiles + 8.
    # dgrad N 8 -> 3, 135 tiles -> 5 (539).  wgrad M 128, N 72 -> 7
    Case("c8_128_tapv8", 11, 56, 56, 8, 128, 3, 1, 1, {}, _e(fwd=(7, 1), dgrad=5, wgrad=7)),
    # K = 4 on 128x128 as 8 waves; wgrad N = 4 -> 5.  (dgrad: 4 input channels are not served)
    Case("c4_128_k4", 11, 56, 56, 4, 128, 1, 1, 0, {}, _e(fwd=7, wgrad=5)),
    # fwd N 256 -> 6; tiles(6) = 135 < 224 -> 1 (270 tiles)
    Case("c64_256_cfg1", 11, 56, 56, 64, 256, 1, 1, 0, {}, _e(fwd=1)),
    # M 59584: tiles(6) = 233 >= 224 -> 6
    Case("c64_256_cfg6", 19, 56, 56, 64, 256, 1, 1, 0, {}, _e(fwd=6)),
    # fwd N 128, tiles(7) = 68 -> 2.  dgrad M 8624, N 512: tiles(7) = 68*4 = 272 -> 7.  wgrad -> 7
    Case("c512_128", 11, 28, 28, 512, 128, 1, 1, 0, {}, _e(fwd=2, dgrad=7, wgrad=7)),
    # fwd M 3920, N 2048 -> 6, 128 tiles -> 1 (256).  dgrad N 512: tiles(7) = 31*4 = 124 -> 2.
    # wgrad 2*2048*512*3920 = 8.2e9 -> 7
    Case("c512_2048_l4", 80, 7, 7, 512, 2048, 1, 1, 0, {}, _e(fwd=1, dgrad=2, wgrad=7)),
    # M 11956: fwd tiles(6) = 47*8 = 376 -> 6; dgrad tiles(7) = 94*16 -> 7;
    # wgrad 2*2048*2048*11956 = 100.3e9 -> 6
    Case("c2048_2048_big", 61, 14, 14, 2048, 2048, 1, 1, 0, {}, _e(fwd=6, dgrad=7, wgrad=6)),
    # the wave-specialised fused dgrad (gemm16_ws.h) takes a 1x1 stride-1 dgrad on a 128-row tile
    # with N a multiple of 128, K = 64 or 128 and at least 512 tiles of 128x128 (mask bits, beta 1):
    # M 16464, N 512: tiles(7) = 129*4 = 516 -> 7, K = 128 (four k-tiles);
    # M 34496, N 256 -> 2 (not >= 512 columns), 270*2 = 540 tiles, K = 64 (two k-tiles)
    Case("c512_128_ws", 21, 28, 28, 512, 128, 1, 1, 0, {"ws": True}, _e(dgrad=7)),
    Case("c256_64_ws", 11, 56, 56, 256, 64, 1, 1, 0, {"ws": True}, _e(dgrad=2)),
    # wgrad M 64, N 256 -> 4 (64x256).  fwd N 64 -> 3, 9 tiles -> 5.  dgrad N 256 -> 2, 34 tiles -> 5
    Case("c256_64_w4", 11, 14, 14, 256, 64, 1, 1, 0, {}, _e(fwd=5, dgrad=5, wgrad=4)),
    # N = 200: no multiple of 128 or 64, on 128x128 (fwd tiles(2) = 129*2 = 258); wgrad N 32 -> 5
    Case("c32_200_ragN", 21, 29, 27, 32, 200, 1, 1, 0, {}, _e(fwd=2, wgrad=5)),
    # wgrad M = 200, N = 288: both ragged on 128x128 as 8 waves.  fwd -> 2, 6 tiles -> 5 (20)
    Case("c32_200_3x3", 2, 13, 11, 32, 200, 3, 1, 1, {}, _e(fwd=5, wgrad=7)),
    # dgrad N = 200 on 128x128 (258 tiles), K = 32: one k-tile.  (200 stored channels: dgrad only)
    Case("c200_32_dragN", 21, 29, 27, 200, 32, 1, 1, 0, {}, _e(dgrad=2)),
    # TAPV at 4 and 16 channels per tap on 128x128 (fwd N 128, M 429: tiles(7) = 4 -> 2)
    Case("c4_128_tapv4", 3, 13, 11, 4, 128, 3, 1, 1, {}, _e(fwd=(2, 1), wgrad=5)),
    Case("c16_128_tapv16", 3, 13, 11, 16, 128, 3, 1, 1, {}, _e(fwd=(2, 1), dgrad=5, wgrad=7)),
    # the dgrad's TAPV (cout channels per tap) on 128x128: N 512, M 429, tiles(7) = 16 -> 2
    Case("d512_4_tapv4", 3, 13, 11, 512, 4, 3, 1, 1, {}, _e(dgrad=(2, 1))),
    Case("d512_8_tapv8", 3, 13, 11, 512, 8, 3, 1, 1, {}, _e(dgrad=(2, 1))),
    Case("d512_16_tapv16", 3, 13, 11, 512, 16, 3, 1, 1, {}, _e(dgrad=(2, 1))),
    # 3x3 stride 2 pad 1, odd and even sizes: four parity classes of 280..360 rows, N 512 -> 2
    # each (the one-launch form, and one launch per class).  fwd N 32 -> 3, 2 tiles -> 5.
    # wgrad M 32, N 4608 -> 5
    Case("s2_odd", 5, 17, 15, 512, 32, 3, 2, 1, {"nclasses": 4}, _e(fwd=5, dgrad=2, wgrad=5)),
    Case("s2_even", 5, 16, 16, 512, 32, 3, 2, 1, {"nclasses": 4}, _e(fwd=5, dgrad=2, wgrad=5)),
    Case("s2_odd_classes", 5, 17, 15, 512, 32, 3, 2, 1, {"nclasses": 4, "classes": True},
         _e(dgrad=2)),
    Case("s2_even_classes", 5, 16, 16, 512, 32, 3, 2, 1, {"nclasses": 4, "classes": True},
         _e(dgrad=2)),
    # strided 1x1: one class has the tap (360 rows, N 512 -> 2), three are empty and zero-filled
    Case("s2_1x1", 5, 17, 15, 512, 64, 1, 2, 0, {"nclasses": 1}, _e(fwd=5, dgrad=2, wgrad=5)),
    # channel slices: x / dx of 64 channels in 96, y / dy of 128 in 160
    Case("slices", 3, 13, 11, 64, 128, 3, 1, 1, {"x_ld": 96, "y_ld": 160},
         _e(fwd=2, dgrad=5, wgrad=7)),
    # frame chunks of 3, 3, 1 frames: 429 rows per chunk, the boundary inside a 128-row tile
    Case("chunks", 7, 13, 11, 64, 128, 3, 1, 1, {"max_frames": 3}, _e(fwd=2, dgrad=5, wgrad=7)),
    # wgrad K = 23*35*23 = 18515 rows: at most 18515 / 1024 = 18 splits, ceil(18515 / 18) = 1029
    # -> 1088 rows each (multiples of 64), ceil(18515 / 1088) = 18 splits, the last of
    # 18515 - 17*1088 = 19 rows: shorter than one k-tile.  On 64x256 and on 128x128 as 8 waves
    Case("wsplit_cfg4", 23, 35, 23, 256, 64, 1, 1, 0, {"splits": 18, "kchunk": 1088},
         _e(wgrad=4)),
    Case("wsplit_cfg7", 23, 35, 23, 128, 128, 1, 1, 0, {"splits": 18, "kchunk": 1088},
         _e(fwd=2, dgrad=5, wgrad=7)),
]

# every (view, config) pair pick_cfg16(..., f32 = true) can return (derivation:
# test_conv_engine_cpu.test_fp32_rows_reach_every_config)
FP32_PAIRS = sorted([("fwd", c) for c in (5, 2, 7, 3, 1, 6)] +
                    [("dgrad", c) for c in (5, 2, 3, 7)] +
                    [("wgrad", c) for c in (5, 4, 7, 6)])

VIEW_IO_F32 = {"fwd": 0, "dgrad": 64, "wgrad": 0}             # dgrad: TMR_IO_WT_F32
VIEW_IO_BF16 = {"fwd": 1 | 2, "dgrad": 4 | 8, "wgrad": 1 | 4}  # X|W, DY|WT, X|DY


def out_hw(c):
    return ((c.h + 2 * c.pad - c.r) // c.stride + 1, (c.w + 2 * c.pad - c.r) // c.stride + 1)


def gemm_k(c, view):
    """The longest reduction of the view (the exact pass asserts 9*K < 2^24)."""
    ho, wo = out_hw(c)
    return {"fwd": c.r * c.r * c.cin, "dgrad": c.r * c.r * c.cout, "wgrad": c.n * ho * wo}[view]


def flops(c):
    ho, wo = out_hw(c)
    return 2.0 * c.n * ho * wo * c.cout * c.r * c.r * c.cin


def tile(ops, c, view, math="fp32"):
    """ops.conv_tile of the row's view under fp32 or bf16 (bf16-stored operands) rules."""
    io = (VIEW_IO_F32 if math == "fp32" else VIEW_IO_BF16)[view]
    with run_form(ops, c):
        return ops.conv_tile(c.n, c.h, c.w, c.cin, c.cout, c.r, c.r, c.stride, c.pad, view,
                             math=math, io=io, x_ld=c.extras.get("x_ld", 0),
                             y_ld=c.extras.get("y_ld", 0))


@contextlib.contextmanager
def run_form(ops, c):
    """The launch form the row's extras ask for: frame chunks, one launch per parity class."""
    old = ops.MAX_FRAMES
    ops.MAX_FRAMES = c.extras.get("max_frames", 0)
    try:
        with (ops.dgrad_class_launches() if c.extras.get("classes") else contextlib.nullcontext()):
            yield
    finally:
        ops.MAX_FRAMES = old


def bf16_rows(ops):
    """(case, view, cfg) of the rows that run under bf16 rules (bf16 math on bf16-stored operands):
    every row but those with a 4-channel side (the bf16 engine moves 8-channel pieces).  Each must
    be an LDS-DMA launch; cfg is the config the bf16 rules give it."""
    rows = []
    for c in CASES:
        if min(c.cin, c.cout) % 8 != 0:
            continue
        for v in ("fwd", "dgrad", "wgrad"):
            if v in c.expect:
                t = tile(ops, c, v, math="bf16")
                assert t["engine"] == L, (c.name, v, t)
                rows.append((c, v, t["cfg"]))
    return rows
