"""Conv routing and planning, pinned without a device: the three planning queries of the conv host
layer (tmr_conv2d_fwd_stats_parts, tmr_conv2d_dgrad_bnbwd_parts, tmr_conv2d_wgrad_ws_bytes) are
pure host code, and their values tell a direct kernel family (stem.hip, stem16.hip, direct3.hip:
d3 / d3s) from the implicit-GEMM engine.  A geometry that silently falls through to the engine
passes every parity test (the engine is their reference), so this table is what catches it.

The values below were recorded from a build of the commit before the routing table
(tmrnet_amd/csrc/direct_conv.h) was introduced, not from the code under test: the refactor must
reproduce them.  Each family is covered in every view it serves, with its view's own io flags:
plain, under ops.engine_only(), with ops.MAX_FRAMES = 2 (the 3x3 families then fall back to the
engine; the stems ignore the cap), at a frame count that caps the persistent grid, and at near-miss
geometries that must not route direct (their value equals the engine's)."""
import contextlib
import ctypes

import pytest

from tmrnet_amd import _lib, ops

X, W, DY, WT, Y, BN, G16 = (ops.IO_X, ops.IO_W, ops.IO_DY, ops.IO_WT, ops.IO_Y, ops.IO_BN,
                            ops.IO_G16)
FWD = "tmr_conv2d_fwd_stats_parts"
DGRAD = "tmr_conv2d_dgrad_bnbwd_parts"
WGRAD = "tmr_conv2d_wgrad_ws_bytes"


def _g(n, h, w, c, k, r, stride, pad, math="fp32", groups=1):
    return dict(n=n, h=h, w=w, c=c, k=k, r=r, s=r, stride=stride, pad=pad, math=math,
                groups=groups)


GEOM = {
    # the 7x7/2 stems on the NHWC4 input (fp32: stem.hip, bf16 math: stem16.hip)
    "stem": _g(3, 224, 224, 4, 64, 7, 2, 3),
    "stem_n16": _g(16, 224, 224, 4, 64, 7, 2, 3),
    "stem_w228": _g(3, 224, 228, 4, 64, 7, 2, 3),
    "stem16": _g(3, 224, 224, 4, 64, 7, 2, 3, "bf16"),
    "stem16_n16": _g(16, 224, 224, 4, 64, 7, 2, 3, "bf16"),
    "stem16_w228": _g(3, 224, 228, 4, 64, 7, 2, 3, "bf16"),
    # the narrow stride-1 3x3 convs (d3) and the deep stem's 3x3/2 conv (d3s)
    "d3_32_32": _g(3, 112, 112, 32, 32, 3, 1, 1, "bf16"),
    "d3_32_64": _g(3, 112, 112, 32, 64, 3, 1, 1, "bf16"),
    "d3_32_64_n16": _g(16, 112, 112, 32, 64, 3, 1, 1, "bf16"),
    "d3_64_64_w56": _g(3, 56, 56, 64, 64, 3, 1, 1, "bf16"),
    "d3_64_64_w112": _g(3, 112, 112, 64, 64, 3, 1, 1, "bf16"),
    "d3s": _g(3, 224, 224, 4, 32, 3, 2, 1, "bf16"),
    "d3s_n16": _g(16, 224, 224, 4, 32, 3, 2, 1, "bf16"),
    "d3s_h223": _g(3, 223, 224, 4, 32, 3, 2, 1, "bf16"),
    # engine shapes
    "e1x1": _g(5, 14, 14, 256, 512, 1, 1, 0),
    "e3x3s2": _g(5, 29, 27, 64, 128, 3, 2, 1),
    "grouped": _g(5, 9, 7, 128, 256, 3, 2, 1, groups=2),
}

# (geometry, query, io, variant, value of the build before the routing table)
PLAN = [
    # every family x every view it serves: direct / forced engine / frames capped at 2
    ("stem", FWD, 0, "plain", 1344),
    ("stem", FWD, 0, "engine", 588),
    ("stem", FWD, 0, "mf2", 1344),
    ("stem", WGRAD, 0, "plain", 25690112),
    ("stem", WGRAD, 0, "engine", 1756160),
    ("stem", WGRAD, 0, "mf2", 25690112),
    ("stem16", FWD, W | Y, "plain", 1344),
    ("stem16", FWD, W | Y, "engine", 147),
    ("stem16", FWD, W | Y, "mf2", 1344),
    ("stem16", WGRAD, DY, "plain", 38535168),
    ("stem16", WGRAD, DY, "engine", 1756160),
    ("stem16", WGRAD, DY, "mf2", 38535168),
    ("stem16", WGRAD, 0, "plain", 38535168),
    ("stem16", WGRAD, 0, "engine", 1756160),
    ("stem16", WGRAD, 0, "mf2", 38535168),
    ("d3_32_32", FWD, X | W | Y, "plain", 1344),
    ("d3_32_32", FWD, X | W | Y, "engine", 588),
    ("d3_32_32", FWD, X | W | Y, "mf2", 588),
    ("d3_32_32", DGRAD, DY | WT | BN, "plain", 336),
    ("d3_32_32", DGRAD, DY | WT | BN, "engine", 588),
    ("d3_32_32", DGRAD, DY | WT | BN, "mf2", 588),
    ("d3_32_64", FWD, X | W | Y, "plain", 672),
    ("d3_32_64", FWD, X | W | Y, "engine", 588),
    ("d3_32_64", FWD, X | W | Y, "mf2", 588),
    ("d3_32_64", DGRAD, DY | WT | BN, "plain", 336),
    ("d3_32_64", DGRAD, DY | WT | BN, "engine", 588),
    ("d3_32_64", DGRAD, DY | WT | BN, "mf2", 588),
    ("d3_32_64", WGRAD, X | DY, "plain", 24772608),
    ("d3_32_64", WGRAD, X | DY, "engine", 2580480),
    ("d3_32_64", WGRAD, X | DY, "mf2", 1769472),
    ("d3_64_64_w56", FWD, X | W | Y, "plain", 168),
    ("d3_64_64_w56", FWD, X | W | Y, "engine", 147),
    ("d3_64_64_w56", FWD, X | W | Y, "mf2", 147),
    ("d3_64_64_w56", DGRAD, DY | WT | BN, "plain", 168),
    ("d3_64_64_w56", DGRAD, DY | WT | BN, "engine", 147),
    ("d3_64_64_w56", DGRAD, DY | WT | BN, "mf2", 147),
    ("d3_64_64_w56", DGRAD, DY | WT | BN | G16, "plain", 168),
    ("d3_64_64_w56", DGRAD, DY | WT | BN | G16, "engine", 147),
    ("d3_64_64_w56", DGRAD, DY | WT | BN | G16, "mf2", 147),
    ("d3_64_64_w56", WGRAD, X | DY, "plain", 24772608),
    ("d3_64_64_w56", WGRAD, X | DY, "engine", 1327104),
    ("d3_64_64_w56", WGRAD, X | DY, "mf2", 884736),
    ("d3s", FWD, W | Y, "plain", 1344),
    ("d3s", FWD, W | Y, "engine", 147),
    ("d3s", FWD, W | Y, "mf2", 588),
    ("d3s", WGRAD, DY, "plain", 1548288),
    ("d3s", WGRAD, DY, "engine", 161280),
    ("d3s", WGRAD, DY, "mf2", 110592),
    # more rows than the persistent grids: the partial-row counts and slabs stop growing
    ("stem_n16", FWD, 0, "plain", 2048),
    ("stem16_n16", FWD, W | Y, "plain", 3072),
    ("stem16_n16", WGRAD, DY, "plain", 38535168),
    ("d3_32_64_n16", FWD, X | W | Y, "plain", 1024),
    ("d3_32_64_n16", DGRAD, DY | WT | BN, "plain", 512),
    ("d3_32_64_n16", WGRAD, X | DY, "plain", 37748736),
    ("d3s_n16", FWD, W | Y, "plain", 3072),
    ("d3s_n16", WGRAD, DY, "plain", 2359296),
    # near misses: one step outside what a family serves (width, channels, io, odd height)
    ("stem_w228", FWD, 0, "plain", 599),
    ("stem_w228", FWD, 0, "engine", 599),
    ("stem_w228", WGRAD, 0, "plain", 1806336),
    ("stem_w228", WGRAD, 0, "engine", 1806336),
    ("stem16_w228", FWD, W | Y, "plain", 150),
    ("stem16_w228", FWD, W | Y, "engine", 150),
    ("stem16_w228", WGRAD, DY, "plain", 1806336),
    ("stem16_w228", WGRAD, DY, "engine", 1806336),
    ("stem16", WGRAD, X | DY, "plain", 1756160),
    ("stem16", WGRAD, X | DY, "engine", 1756160),
    ("d3_64_64_w112", FWD, X | W | Y, "plain", 588),
    ("d3_64_64_w112", FWD, X | W | Y, "engine", 588),
    ("d3_64_64_w112", DGRAD, DY | WT | BN, "plain", 588),
    ("d3_64_64_w112", DGRAD, DY | WT | BN, "engine", 588),
    ("d3_64_64_w112", WGRAD, X | DY, "plain", 5160960),
    ("d3_64_64_w112", WGRAD, X | DY, "engine", 5160960),
    ("d3_32_32", DGRAD, DY | WT | BN | G16, "plain", 588),
    ("d3_32_32", DGRAD, DY | WT | BN | G16, "engine", 588),
    ("d3s_h223", FWD, W | Y, "plain", 147),
    ("d3s_h223", FWD, W | Y, "engine", 147),
    ("d3s_h223", WGRAD, DY, "plain", 161280),
    ("d3s_h223", WGRAD, DY, "engine", 161280),
    # the engine's own shapes, ungrouped and grouped, whole and in frame chunks of 2
    ("e1x1", FWD, 0, "plain", 16),
    ("e1x1", FWD, 0, "mf2", 18),
    ("e1x1", DGRAD, 0, "plain", 16),
    ("e1x1", DGRAD, 0, "mf2", 18),
    ("e1x1", WGRAD, 0, "plain", 524288),
    ("e1x1", WGRAD, 0, "mf2", 524288),
    ("e3x3s2", FWD, 0, "plain", 9),
    ("e3x3s2", FWD, 0, "mf2", 12),
    ("e3x3s2", DGRAD, 0, "plain", 64),
    ("e3x3s2", DGRAD, 0, "mf2", 69),
    ("e3x3s2", WGRAD, 0, "plain", 294912),
    ("e3x3s2", WGRAD, 0, "mf2", 294912),
    ("grouped", FWD, 0, "plain", 2),
    ("grouped", FWD, 0, "mf2", 3),
    ("grouped", DGRAD, 0, "plain", 7),
    ("grouped", DGRAD, 0, "mf2", 12),
    ("grouped", WGRAD, 0, "plain", 294912),
    ("grouped", WGRAD, 0, "mf2", 294912),
]


def _value(geom, query, io, variant, monkeypatch):
    monkeypatch.setattr(ops, "MAX_FRAMES", 2 if variant == "mf2" else 0)
    with ops.engine_only() if variant == "engine" else contextlib.nullcontext():
        d = ops.conv_desc(io=io, **GEOM[geom])
    return _lib.query(query, ctypes.byref(d))


@pytest.mark.parametrize("geom,query,io,variant,want", PLAN,
                         ids=["%s-%s-io%d-%s" % (r[0], r[1][11:], r[2], r[3]) for r in PLAN])
def test_plan_value(geom, query, io, variant, want, monkeypatch):
    assert _value(geom, query, io, variant, monkeypatch) == want


def test_table_tells_direct_from_engine():
    """The table itself pins routing: every direct row differs from its forced-engine row, and
    every near-miss row equals it."""
    rows = {r[:4]: r[4] for r in PLAN}
    assert len(rows) == len(PLAN)
    direct = [k for k in rows if k[3] == "engine" and k[:3] + ("mf2",) in rows]
    near = [k for k in rows if k[3] == "engine" and k[:3] + ("mf2",) not in rows]
    assert len(direct) == 16 and len(near) == 11
    for k in direct:
        assert rows[k[:3] + ("plain",)] != rows[k], k
    for k in near:
        assert rows[k[:3] + ("plain",)] == rows[k], k
