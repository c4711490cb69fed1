"""Coverage of the conv engine's tile rules by the case table of the engine tests, checked without
a GPU: tmr_conv2d_tile (host code; the selection functions the launches call) must send every row
of tests/_conv_engine_cases.py to the (engine, config, TAPV form) the row declares, and the fp32
rows together must reach every (view, config) pair the fp32 rules can select."""
import pytest

from tmrnet_amd import ops

from tests import _conv_engine_cases as T

ROWS = [(c, v) for c in T.CASES for v in ("fwd", "dgrad", "wgrad") if v in c.expect]


@pytest.mark.parametrize("case,view", ROWS, ids=["%s-%s" % (c.name, v) for c, v in ROWS])
def test_row_reaches_declared_config(case, view):
    t = T.tile(ops, case, view)
    assert (t["engine"], t["cfg"], t["tapv"]) == case.expect[view], t
    bm, bn, waves = {1: (256, 128, 8), 2: (128, 128, 4), 3: (256, 64, 4), 4: (64, 256, 4),
                     5: (64, 64, 4), 6: (256, 256, 16), 7: (128, 128, 8)}[t["cfg"]]
    assert (t["bm"], t["bn"], t["waves"]) == (bm, bn, waves)
    if view == "dgrad":
        assert t["classes"] == case.extras.get("nclasses", 1)
    if view == "wgrad" and "splits" in case.extras:
        assert (t["splits"], t["kchunk"]) == (case.extras["splits"], case.extras["kchunk"])
        ho, wo = T.out_hw(case)
        last = case.n * ho * wo - t["kchunk"] * (t["splits"] - 1)
        assert 1 <= last <= 31          # the last split: shorter than one fp32 k-tile


def test_fp32_rows_reach_every_config():
    """The (view, config) pairs pick_cfg16(M, N, K, view, f32 = true) can return, read off its
    rules (gemm16_select.h) in order:
      wgrad  returns inside its own block: 5 (M <= 64 with N <= 64 or N >= 512; N <= 64),
             4 (M <= 64, 64 < N < 512), 6 (M, N >= 256 and >= 100 GFLOP), 7 (the rest)  -> {5,4,6,7}
      dgrad  M >= 256 and N >= 512 returns 7 or 2.  Otherwise the shape rule gives 3 or 5 (N <= 64)
             or 2 -- 6 is for the forward only -- and the few-tiles step goes from 3 or 2 to a
             smaller tile among (1, 2, 5): 1 (256x128) is never smaller than 3 (256x64) or 2
             (128x128), 2 is not smaller than either, so only 5 is added                -> {3,5,2,7}
      fwd    M >= 256 and N == 128 returns 7 or 2.  Otherwise 3 / 5 / 6 / 2 by shape; the step
             from 6 reaches 1, then 2, then 5; from 3 and 2 only 5                   -> {3,5,6,2,7,1}
    Configs 0 (256x256 as 8 waves) and 4 outside the wgrad are reachable only through
    TMR_GEMM16_CFG.  14 pairs; the table must reach each with at least one fp32 row."""
    assert len(T.FP32_PAIRS) == 14
    reached = sorted({(v, c.expect[v][1]) for c, v in ROWS})
    assert reached == T.FP32_PAIRS
    # ... and the query agrees that those rows get there
    got = sorted({(v, T.tile(ops, c, v)["cfg"]) for c, v in ROWS})
    assert got == T.FP32_PAIRS


def test_bf16_rows_are_lds_dma_launches():
    """The bf16 exact pass runs every row without a 4-channel side (the five views of c4_128_k4,
    c4_128_tapv4 and d512_4_tapv4 are the only ones left out), each on the LDS-DMA engine."""
    rows = T.bf16_rows(ops)
    assert len(rows) == len(ROWS) - 5
    assert sorted({c.name for c, v in ROWS} - {c.name for c, v, k in rows}) == [
        "c4_128_k4", "c4_128_tapv4", "d512_4_tapv4"]


def test_edges_sit_on_multi_wave_tiles():
    """The edge geometries the table must hold, each on a config other than 64x64 (config 5):
    ragged M, ragged N, K below one k-tile, K = k-tiles + remainder, TAPV at 4 / 8 / 16 channels,
    strided classes."""
    by = {c.name: c for c in T.CASES}

    def cfg(name, view):
        return by[name].expect[view][1]
    assert cfg("c64_64_ragM", "fwd") == 3 and (21 * 57 * 55) % 256 != 0
    assert cfg("c32_200_ragN", "fwd") == 2 and 200 % 64 != 0
    assert cfg("c32_200_3x3", "wgrad") == 7 and cfg("c200_32_dragN", "dgrad") == 2
    assert cfg("c8_64_k8", "fwd") == 3 and cfg("c4_128_k4", "fwd") == 7      # K = 8, 4 < 32
    assert cfg("c8_128_tapv8", "fwd") == 7 and (9 * 8) % 32 == 8             # 2 k-tiles + 8
    for name, view in (("c4_128_tapv4", "fwd"), ("c8_128_tapv8", "fwd"), ("c16_128_tapv16", "fwd"),
                       ("d512_4_tapv4", "dgrad"), ("d512_8_tapv8", "dgrad"),
                       ("d512_16_tapv16", "dgrad")):
        assert by[name].expect[view][2] == 1 and cfg(name, view) != 5
    for name in ("s2_odd", "s2_even", "s2_odd_classes", "s2_even_classes", "s2_1x1"):
        assert cfg(name, "dgrad") == 2
    # the exact pass's condition: every partial sum of products of integers in [-3, 3] stays
    # below 2^24 in magnitude
    assert all(9 * T.gemm_k(c, v) + 6 < 2 ** 24 for c, v in ROWS)
    # the largest case stays under about 110 GFLOP
    assert max(T.flops(c) for c in T.CASES) < 110e9


def test_query_refuses_bad_arguments():
    import ctypes
    from tmrnet_amd import _lib
    t = _lib.ConvTile()
    d = ops.conv_desc(2, 8, 8, 16, 16, 3, 3, 1, 1)
    with pytest.raises(RuntimeError, match="view"):
        _lib.query("tmr_conv2d_tile", ctypes.byref(d), 3, ctypes.byref(t))
    with pytest.raises(RuntimeError, match="null"):
        _lib.query("tmr_conv2d_tile", None, 0, ctypes.byref(t))
    d.c = 12
    with pytest.raises(RuntimeError, match="power of two"):
        _lib.query("tmr_conv2d_tile", ctypes.byref(d), 0, ctypes.byref(t))
    # KRSC weights: the plain dgrad runs the register-staged engine
    assert ops.conv_tile(2, 14, 14, 64, 64, 3, 3, 1, 1, "dgrad")["engine"] == 1
    # the 7x7 stem's wgrad is a direct kernel
    assert ops.conv_tile(2, 224, 224, 4, 64, 7, 7, 2, 3, "wgrad")["engine"] == 0
