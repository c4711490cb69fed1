"""Every BatchNorm entry point of csrc/bn.hip against a plain float64 CPU computation of the same
operation, written here, at the smallest shapes that take each branch of the host launch ladders.

Operands are float64 values that fp32 (bf16 for bf16 operands) holds exactly, so both sides see
the same numbers.  The backward entry points get arbitrary save_mean / save_invstd / scale / shift
(not the statistics of y); their reference is the closed form, with g = mask ? dz : 0:
dbeta = sum g, dgamma = inv * sum g (y - mean), dy = gamma inv (g - dbeta/n - xhat dgamma/n).
Masks agree by construction: mask 1 reads the reference's z rounded to the operand type, mask 2
tests y * scale + shift > 0 in float64 on the fp32 scale / shift (a correctly rounded fmaf keeps
the sign of the exact value).  Outputs handed out by torch.empty* hold NaN (`poison`), outputs
the test allocates sit between sentinels.

Bounds.  rel_err = max |a - b| / max |b|.  fp32: forward z < 3e-6; mean / invstd / scale / shift /
running statistics < 1e-6; dy / dres / dgamma / dbeta < 1e-5 (tests/test_kernels_gpu.py).  bf16
outputs: (a) bitwise the fp32 sibling rounded by torch where the code promises the same arithmetic,
(b) elementwise |out - ref| <= 2^-8 |ref| + E max |ref|, E the fp32 bound of that quantity.
Offset mean (|mean| / std = R ~ 1e3): forward |z - z64| <= 4 u R max |gamma| elementwise (the fp32
shift alone carries u R), backward rel_err <= 1e-5 + 4 u R; tests/test_bn_cpu.py shows both hold
for a float64-statistics, fp32-coefficient emulation.

Shapes (rows, c) and the rungs they reach:
  (3, 8)       one partial block, fewer rows than row threads, ragged bits word
  (77, 12)     c/4 = 3: chan_of's modulo, 3 channel threads (thread 255 idle), 4-wide everywhere
  (101, 24)    c/8 = 3: the 8-wide kernels with the modulo; the stem's per-pixel form
  (1001, 64)   ragged rows, several row blocks
  (530, 2048)  8 channel blocks
  (40037, 256) make_plan's rpb = rows / 1024 branch
  (16400, 1024) / (16400, 2048): the second trip of the grid-stride loops (grid cap 8192 blocks)

Entry point -> kernels / template rungs reached:
  tmr_bn_fwd_stats       bn_stats_partial + bn_finalize_k (tmr_bn_finalize), gamma / beta null too
  tmr_bn_finalize_ws     parts_slab_k<0> + finalize_slabs_k: 1 .. 500 slabs, c = 72's ragged group
  tmr_bn_eval_params     bn_eval_params_k, c = 300's partial block, gamma / beta null
  tmr_bn_apply(_x)       bn_apply_k<RES, RELU> x4, <.., __bf16> x2
  tmr_bn_apply_dual      bn_apply_k<RES, RELU, float, DUAL> x4
  tmr_bn_apply2(_x)      bn_apply2_k<RELU, DUAL> x4
  tmr_bn_apply_a16       bn_apply8_a16_k<RES, RELU, false> x4 (aligned, c % 8), bn_apply_k<.., __bf16,
                         false, __bf16> x4 (else)
  tmr_bn_apply2_a16      bn_apply8_a16_k<false, RELU, true> x2, bn_apply2_k<RELU, false, __bf16, __bf16> x2
  tmr_bn_apply_bits      bn_apply_bits8_k<RES> x2 (aligned, c % 8), bn_apply_bits_k<RES, float> x2
  tmr_bn_apply2_bits     bn_apply_bits8_k<false> with yr, bn_apply_bits_k<false, float> with yr
  tmr_bn_apply(2)_bits_a16  bn_apply_bits_k<RES, __bf16> x2, with yr
  tmr_bn_bwd(_x)         bn_bwd_partial<0 | 1 | 2, WB>, bn_bwd_final, bn_bwd_apply<MASK, DRES, float | __bf16>
  tmr_bn_bwd_a16         bn_bwd_partial<.., __bf16>, bn_bwd_apply<MASK, DRES, __bf16, __bf16>,
                         bn_bwd_apply8_a16<float> (mask 0 left, aligned, c % 8)
  tmr_bn_bwd_g16         bn_bwd_partial<0, false, __bf16, const __bf16>, bn_bwd_apply8_a16<__bf16>
  tmr_bn_bwd_parts(_x)   parts_slab_k<1> + bwd_final_slabs_k, bn_bwd_apply8_k (aligned, c % 8),
                         bn_bwd_apply<0, false, float | __bf16, float>
  tmr_bn_bwd_parts_a16   bn_bwd_apply8_a16<float> / bn_bwd_apply<0, false, __bf16, __bf16>
  tmr_bn_bwd_parts_g16   bn_bwd_apply8_a16<__bf16>
  tmr_bn_bwd_parts_ds    both reductions + bn_bwd_apply_ds8<float | __bf16>
  tmr_bn_bwd_maxpool(_x) stem_bwd_partial_pooled<float>, stem_bwd_apply8q<float, float | __bf16>
                         (c/8 a power of two, aligned), stem_bwd_apply<float | __bf16> (else)
  tmr_bn_bwd_maxpool_a16 stem_bwd_partial_pooled<__bf16>, stem_bwd_apply8q<__bf16, __bf16>,
                         stem_bwd_apply<__bf16, __bf16>
  tmr_bn_frozen_bwd_ds   bn_frozen_bwd8_k<0 | 2, true> (every other frozen rung:
                         tests/test_frozen_bn_gpu.py; all 103: profiles/bn_dispatch/rungs.md)
"""
import ctypes
import functools

import pytest
import torch

from tmrnet_amd import ops
from tmrnet_amd._lib import call, query, stream_ptr
from tests.test_head_gpu import guarded, guards_ok, no_nan, poison, rel_err, rnd  # noqa: F401
from tests.test_kernels_gpu import _pack_bits
from tests.test_stem_pool8_gpu import _off8

gpu = pytest.mark.gpu

f64 = torch.float64
f32 = torch.float32
BF16 = torch.bfloat16
U = 2.0 ** -24          # fp32 unit roundoff
EPS = 1e-5
E_FWD, E_STAT, E_BWD = 3e-6, 1e-6, 1e-5

SMALL = [(3, 8), (77, 12), (101, 24), (1001, 64)]
BIG = [(530, 2048), (40037, 256)]


def rnd16(*shape, g, scale=1.0, shift=0.0):
    """float64 values that bf16 holds exactly"""
    return (torch.randn(*shape, generator=g, dtype=f64) * scale + shift).to(BF16).double()


def pos(c, g):
    """fp32-exact values in [0.5, 1.5)"""
    return (torch.rand(c, generator=g, dtype=f64) + 0.5).float().double()


def up(t, dev, dtype=f32, off=False):
    """the float64 tensor on the device in `dtype` (exact), optionally 8 bytes off a 16-B boundary"""
    v = t.to(dtype).to(dev)
    return _off8(v) if off else v


def bf16_excess(out, ref, E):
    """max over elements of |out - ref| / (2^-8 |ref| + E max |ref|): bound (b) holds when <= 1"""
    out = out.detach().double().cpu()
    bound = 2.0 ** -8 * ref.abs() + E * ref.abs().max() + 1e-300
    return ((out - ref).abs() / bound).max().item()


def same_bits(a16, b32):
    """bf16 tensor a16 is bitwise the fp32 tensor b32 rounded by torch (RNE)"""
    return torch.equal(a16.view(torch.int16), b32.to(BF16).view(torch.int16))


def closed_form(g, y, mean, inv, gamma, S=None, Q=None):
    """-> dy, dgamma, dbeta; S, Q: sum g and sum g (y - mean) when they come from partials"""
    n = y.shape[0]
    if S is None:
        S, Q = g.sum(0), (g * (y - mean)).sum(0)
    dgamma = inv * Q
    dy = gamma * inv * (g - S / n - (y - mean) * inv * dgamma / n)
    return dy, dgamma, S


# ------------------------------------------------------------------ 1. statistics
@functools.lru_cache(maxsize=4)     # the largest case holds 0.6 GB of float64
def _stats_case(rows, c):
    g = torch.Generator().manual_seed(rows * 7 + c)
    # per-channel spread and offset: no two channels share their statistics
    y = (torch.randn(rows, c, generator=g, dtype=f64) * (torch.rand(c, generator=g, dtype=f64) * 3.5 + 0.5)
         + (torch.rand(c, generator=g, dtype=f64) * 6 - 3)).float().double()
    return dict(y=y, gamma=pos(c, g), beta=rnd(c, g=g), rm=rnd(c, g=g), rv=pos(c, g))


def _stats_ref(y, gamma, beta, rm, rv, momentum=0.1):
    n = y.shape[0]
    mean = y.mean(0)
    m2 = ((y - mean) ** 2).sum(0)
    inv = 1.0 / torch.sqrt(m2 / n + EPS)
    gm = gamma if gamma is not None else torch.ones_like(mean)
    bt = beta if beta is not None else torch.zeros_like(mean)
    return dict(mean=mean, inv=inv, scale=gm * inv, shift=bt - mean * gm * inv,
                rm=(1 - momentum) * rm + momentum * mean,
                rv=(1 - momentum) * rv + momentum * m2 / (n - 1))


def _check_stats(got, rmd, rvd, ref):
    for name, t in zip(("mean", "inv", "scale", "shift"), got):
        assert no_nan(t), name
        assert rel_err(t, ref[name]) < E_STAT, name
    assert rel_err(rmd, ref["rm"]) < E_STAT
    assert rel_err(rvd, ref["rv"]) < E_STAT


@gpu
@pytest.mark.parametrize("rows,c", SMALL + BIG)
def test_fwd_stats(dev, poison, rows, c):
    """tmr_bn_fwd_stats (bn_stats_partial + bn_finalize_k) vs float64 mean / biased variance;
    running statistics with momentum 0.1 take the unbiased variance, from non-trivial values."""
    k = _stats_case(rows, c)
    rmd, rvd = up(k["rm"], dev), up(k["rv"], dev)
    got = ops.bn_fwd_train(up(k["y"], dev), up(k["gamma"], dev), up(k["beta"], dev), rmd, rvd,
                           0.1, EPS)
    _check_stats(got, rmd, rvd, _stats_ref(k["y"], k["gamma"], k["beta"], k["rm"], k["rv"]))


@gpu
def test_fwd_stats_no_affine(dev, poison):
    """gamma = beta = null: scale = invstd, shift = -mean invstd"""
    rows, c = 77, 12
    k = _stats_case(rows, c)
    rmd, rvd = up(k["rm"], dev), up(k["rv"], dev)
    got = ops.bn_fwd_train(up(k["y"], dev), None, None, rmd, rvd, 0.1, EPS)
    _check_stats(got, rmd, rvd, _stats_ref(k["y"], None, None, k["rm"], k["rv"]))


OFFSET_CASES = [(4099, 8), (50000, 12)]


@functools.lru_cache(maxsize=None)
def offset_case(rows, c, R=1e3):
    """y = R + randn (|mean| / std = R) with its float64 BatchNorm forward and backward"""
    g = torch.Generator().manual_seed(rows + c)
    y = (torch.randn(rows, c, generator=g, dtype=f64) + R).float().double()
    gamma, beta, dz = pos(c, g), rnd(c, g=g), rnd(rows, c, g=g)
    mean = y.mean(0)
    var = ((y - mean) ** 2).mean(0)
    inv = 1.0 / torch.sqrt(var + EPS)
    z = (y - mean) * inv * gamma + beta
    dy, dgamma, dbeta = closed_form(dz, y, mean, inv, gamma)
    ratio = (mean.abs() / var.sqrt()).max().item()
    return dict(y=y, gamma=gamma, beta=beta, dz=dz, mean=mean, inv=inv, z=z, dy=dy, dgamma=dgamma,
                dbeta=dbeta, fwd_bound=4 * U * ratio * gamma.abs().max().item(),
                bwd_bound=1e-5 + 4 * U * ratio)


@gpu
@pytest.mark.parametrize("rows,c", OFFSET_CASES)
def test_offset_mean(dev, poison, rows, c):
    """stats -> bn_apply -> bn_bwd on y = 1e3 + randn.  Forward |z - z64| <= 4 u R max |gamma|
    elementwise, backward rel_err <= 1e-5 + 4 u R (module docstring; a one-pass fp32 variance
    misses the forward bound by three orders of magnitude)."""
    k = offset_case(rows, c)
    yd, gd = up(k["y"], dev), up(k["gamma"], dev)
    mean, inv, scale, shift = ops.bn_fwd_train(yd, gd, up(k["beta"], dev), None, None, 0.1, EPS)
    z = ops.bn_apply(yd, scale, shift, None, relu=False)
    ferr = (z.double().cpu() - k["z"]).abs().max().item()
    print("offset mean (%d, %d): forward %.3g (bound %.3g)" % (rows, c, ferr, k["fwd_bound"]))
    assert no_nan(z) and ferr <= k["fwd_bound"]
    dy, _, dgm, dbt = ops.bn_bwd(up(k["dz"], dev), yd, None, mean, inv, gd, False)
    errs = rel_err(dy, k["dy"]), rel_err(dgm, k["dgamma"]), rel_err(dbt, k["dbeta"])
    print("offset mean (%d, %d): backward %s (bound %.3g)" % (rows, c, errs, k["bwd_bound"]))
    assert max(errs) <= k["bwd_bound"]


# ------------------------------------------------------------------ 2. finalisers from partials
def _chunks(rows, nparts, g):
    """nparts contiguous chunks of unequal sizes covering rows, the first of one row -> (sizes, ids)"""
    assert 1 <= nparts <= rows
    if nparts == 1:
        sizes = torch.tensor([rows])
    else:
        cuts = torch.randperm(rows - 2, generator=g)[:nparts - 2] + 2 if nparts > 2 else torch.zeros(0, dtype=torch.int64)
        edges = torch.cat([torch.tensor([0, 1]), cuts.sort().values, torch.tensor([rows])])
        sizes = edges[1:] - edges[:-1]
    assert sizes.numel() == nparts and int(sizes.sum()) == rows and int(sizes.min()) >= 1
    return sizes, torch.repeat_interleave(torch.arange(nparts), sizes)


def _seg_sum(v, ids, nparts):
    return torch.zeros(nparts, v.shape[1], dtype=f64).index_add_(0, ids, v)


PARTS_CASES = [(np_, c) for c in (8, 72, 2048) for np_ in (1, 5, 33, 600)] + [(20000, 8)]


def _parts_rows(nparts):
    return 20011 if nparts == 20000 else max(nparts + 11, 40)


@gpu
@pytest.mark.parametrize("nparts,c", PARTS_CASES)
def test_finalize_from_partials(dev, poison, nparts, c):
    """tmr_bn_finalize_ws (parts_slab_k<0> + finalize_slabs_k) on fabricated (count, mean, M2, 0)
    partials of unequal chunks (one-row chunks included), rounded to fp32; the reference combines
    the rounded partials in float64.  (20000, 8): 500 slabs, more than slab_sum's 16 phases;
    c = 72: the second 64-channel group partly empty."""
    rows = _parts_rows(nparts)
    k = _stats_case(rows, c)
    g = torch.Generator().manual_seed(nparts + c)
    sizes, ids = _chunks(rows, nparts, g)
    cnt = sizes.double().view(-1, 1)
    mb = _seg_sum(k["y"], ids, nparts) / cnt
    m2b = _seg_sum((k["y"] - mb[ids]) ** 2, ids, nparts)
    stats = torch.stack([cnt.expand(-1, c), mb, m2b, torch.zeros_like(mb)], 2).float()
    s = stats.double()
    n = s[:, :, 0].sum(0)
    mean = (s[:, :, 0] * s[:, :, 1]).sum(0) / n
    m2 = (s[:, :, 2] + s[:, :, 0] * (s[:, :, 1] - mean) ** 2).sum(0)
    inv = 1.0 / torch.sqrt(m2 / n + EPS)
    ref = dict(mean=mean, inv=inv, scale=k["gamma"] * inv, shift=k["beta"] - mean * k["gamma"] * inv,
               rm=0.9 * k["rm"] + 0.1 * mean, rv=0.9 * k["rv"] + 0.1 * m2 / (n - 1))
    rmd, rvd = up(k["rm"], dev), up(k["rv"], dev)
    got = ops.bn_finalize(stats.to(dev), nparts, up(k["gamma"], dev), up(k["beta"], dev), rmd, rvd,
                          0.1, EPS)
    _check_stats(got, rmd, rvd, ref)


@functools.lru_cache(maxsize=4)     # the largest case holds 0.6 GB of float64
def _bwd_case(rows, c):
    g = torch.Generator().manual_seed(rows * 3 + c)
    k = dict(y=rnd(rows, c, g=g, scale=2.0, shift=1.0), dz=rnd(rows, c, g=g), r=rnd(rows, c, g=g),
             y16=rnd16(rows, c, g=g, scale=2.0, shift=1.0), dz16=rnd16(rows, c, g=g),
             r16=rnd16(rows, c, g=g), yd=rnd(rows, c, g=g, scale=1.5, shift=-0.5),
             yd16=rnd16(rows, c, g=g, scale=1.5, shift=-0.5),
             mean=rnd(c, g=g, scale=0.5, shift=1.0), inv=pos(c, g), gamma=rnd(c, g=g, shift=0.3),
             scale=rnd(c, g=g), shift=rnd(c, g=g),
             mean_d=rnd(c, g=g, scale=0.5, shift=-0.5), inv_d=pos(c, g), gamma_d=rnd(c, g=g, shift=-0.3))
    return k


def _parts_of(gv, y, mean, nparts, seed):
    """(sum g, sum g (y - mean)) per chunk, rounded to fp32 -> parts (nparts, c, 2), S, Q of them"""
    sizes, ids = _chunks(y.shape[0], nparts, torch.Generator().manual_seed(seed))
    parts = torch.stack([_seg_sum(gv, ids, nparts), _seg_sum(gv * (y - mean), ids, nparts)], 2).float()
    return parts, parts[:, :, 0].double().sum(0), parts[:, :, 1].double().sum(0)


@gpu
@pytest.mark.parametrize("nparts,c", PARTS_CASES)
def test_bwd_parts_from_partials(dev, poison, nparts, c):
    """tmr_bn_bwd_parts_x (fp32 and bf16 dy), _a16 and _g16 on fabricated (sum g, sum g (y - mean))
    partials rounded to fp32; reference: float64 sums of the rounded partials, then the closed
    form.  Aligned operands take the 8-wide applies, operands 8 bytes off the 4-wide ones."""
    rows = _parts_rows(nparts)
    k = _bwd_case(rows, c)
    md, iv, gm = (up(k[n], dev) for n in ("mean", "inv", "gamma"))
    # fp32 g and y
    parts, S, Q = _parts_of(k["dz"], k["y"], k["mean"], nparts, nparts + c)
    dy64, dg64, db64 = closed_form(k["dz"], k["y"], k["mean"], k["inv"], k["gamma"], S, Q)
    pd = parts.to(dev)
    for off in (False, True):
        gd, yd = up(k["dz"], dev, off=off), up(k["y"], dev, off=off)
        dy, dgm, dbt = ops.bn_bwd_parts(gd, yd, pd, nparts, md, iv, gm)
        assert no_nan(dy) and rel_err(dy, dy64) < E_BWD
        assert rel_err(dgm, dg64) < E_BWD and rel_err(dbt, db64) < E_BWD
        dy16, dgm16, dbt16 = ops.bn_bwd_parts(gd, yd, pd, nparts, md, iv, gm, bf16=True)
        assert dy16.dtype == BF16 and same_bits(dy16, dy)
        assert bf16_excess(dy16, dy64, E_BWD) <= 1.0
        assert torch.equal(dgm16, dgm) and torch.equal(dbt16, dbt)
    # bf16 y, fp32 g (_a16)
    parts, S, Q = _parts_of(k["dz"], k["y16"], k["mean"], nparts, nparts + c)
    dy64, dg64, db64 = closed_form(k["dz"], k["y16"], k["mean"], k["inv"], k["gamma"], S, Q)
    for off in (False, True):
        dy, dgm, dbt = ops.bn_bwd_parts(up(k["dz"], dev, off=off), up(k["y16"], dev, BF16, off=off),
                                        parts.to(dev), nparts, md, iv, gm)
        assert dy.dtype == BF16 and no_nan(dy) and bf16_excess(dy, dy64, E_BWD) <= 1.0
        assert rel_err(dgm, dg64) < E_BWD and rel_err(dbt, db64) < E_BWD
    # bf16 g and y (_g16)
    parts, S, Q = _parts_of(k["dz16"], k["y16"], k["mean"], nparts, nparts + c)
    dy64, dg64, db64 = closed_form(k["dz16"], k["y16"], k["mean"], k["inv"], k["gamma"], S, Q)
    dy, dgm, dbt = ops.bn_bwd_parts(up(k["dz16"], dev, BF16), up(k["y16"], dev, BF16),
                                    parts.to(dev), nparts, md, iv, gm)
    assert dy.dtype == BF16 and no_nan(dy) and bf16_excess(dy, dy64, E_BWD) <= 1.0
    assert rel_err(dgm, dg64) < E_BWD and rel_err(dbt, db64) < E_BWD


# ------------------------------------------------------------------ 3. forward applies
@functools.lru_cache(maxsize=None)
def _fwd_case(rows, c):
    g = torch.Generator().manual_seed(rows * 5 + c)
    return dict(y=rnd(rows, c, g=g, scale=2.0), r=rnd(rows, c, g=g), yr=rnd(rows, c, g=g, scale=2.0),
                y16=rnd16(rows, c, g=g, scale=2.0), r16=rnd16(rows, c, g=g),
                yr16=rnd16(rows, c, g=g, scale=2.0),
                sc=rnd(c, g=g, shift=0.2), sf=rnd(c, g=g), rs=rnd(c, g=g, shift=-0.2), rf=rnd(c, g=g))


def _fwd_ref(k, sfx, res, relu, branch=False):
    z = k["y" + sfx] * k["sc"] + k["sf"]
    if branch:
        z = z + (k["yr" + sfx] * k["rs"] + k["rf"])
    elif res:
        z = z + k["r" + sfx]
    return torch.relu(z) if relu else z


FORMS = [(res, relu) for res in (False, True) for relu in (False, True)]


@gpu
@pytest.mark.parametrize("off", [False, True], ids=["aligned", "off8"])
@pytest.mark.parametrize("rows,c", SMALL)
def test_apply_fp32(dev, poison, rows, c, off):
    """tmr_bn_apply_x, tmr_bn_apply_dual, tmr_bn_apply2_x on fp32 tensors, every residual / ReLU /
    dual form: z < 3e-6 against float64, between sentinels where the wrapper takes `out`; the bf16
    outputs are bitwise the fp32 ones rounded and within bound (b); a residual with a bf16 output
    and a branch input aliasing z are refused."""
    k = _fwd_case(rows, c)
    y, r, yr = (up(k[n], dev, off=off) for n in ("y", "r", "yr"))
    sc, sf, rs, rf = (up(k[n], dev) for n in ("sc", "sf", "rs", "rf"))
    for res, relu in FORMS:
        ref = _fwd_ref(k, "", res, relu)
        buf, out = guarded((rows, c), dev)
        z = ops.bn_apply(y, sc, sf, r if res else None, relu, out=out)
        assert no_nan(z) and guards_ok(buf) and rel_err(z, ref) < E_FWD, (res, relu)
        zd, z16 = ops.bn_apply_dual(y, sc, sf, r if res else None, relu)
        assert torch.equal(zd, z) and z16.dtype == BF16 and same_bits(z16, z), (res, relu)
        assert bf16_excess(z16, ref, E_FWD) <= 1.0
        if not res:
            zb = ops.bn_apply(y, sc, sf, None, relu, bf16=True)
            assert zb.dtype == BF16 and same_bits(zb, z) and bf16_excess(zb, ref, E_FWD) <= 1.0
    with pytest.raises(RuntimeError, match="no residual"):
        ops.bn_apply(y, sc, sf, r, True, bf16=True)
    for relu in (False, True):
        ref = _fwd_ref(k, "", False, relu, branch=True)
        buf, out = guarded((rows, c), dev)
        z = ops.bn_apply2(y, sc, sf, yr, rs, rf, relu, out=out)
        assert no_nan(z) and guards_ok(buf) and rel_err(z, ref) < E_FWD, relu
        zd, z16 = ops.bn_apply2(y, sc, sf, yr, rs, rf, relu, dual=True)
        assert torch.equal(zd, z) and same_bits(z16, z) and bf16_excess(z16, ref, E_FWD) <= 1.0
    with pytest.raises(RuntimeError, match="must not alias"):
        ops.bn_apply2(y, sc, sf, yr, rs, rf, True, out=yr)


@gpu
@pytest.mark.parametrize("off", [False, True], ids=["aligned", "off8"])
@pytest.mark.parametrize("rows,c", SMALL)
def test_apply_a16(dev, poison, rows, c, off):
    """tmr_bn_apply_a16 / tmr_bn_apply2_a16 (bf16 y, residual / branch input, z): the 8-wide form
    (aligned, c % 8 == 0) and the 4-wide one, every form within bound (b) of float64."""
    k = _fwd_case(rows, c)
    y, r, yr = (up(k[n], dev, BF16, off=off) for n in ("y16", "r16", "yr16"))
    sc, sf, rs, rf = (up(k[n], dev) for n in ("sc", "sf", "rs", "rf"))
    for res, relu in FORMS:
        z = ops.bn_apply(y, sc, sf, r if res else None, relu)
        assert z.dtype == BF16 and no_nan(z)
        assert bf16_excess(z, _fwd_ref(k, "16", res, relu), E_FWD) <= 1.0, (res, relu)
    for relu in (False, True):
        z = ops.bn_apply2(y, sc, sf, yr, rs, rf, relu)
        assert z.dtype == BF16 and no_nan(z)
        assert bf16_excess(z, _fwd_ref(k, "16", False, relu, branch=True), E_FWD) <= 1.0, relu
    with pytest.raises(RuntimeError, match="must not alias"):
        ops.bn_apply2(y, sc, sf, yr, rs, rf, True, out=yr)


@gpu
@pytest.mark.parametrize("off", [False, True], ids=["aligned", "off8"])
@pytest.mark.parametrize("rows,c", SMALL)
def test_apply_bits(dev, poison, rows, c, off):
    """tmr_bn_apply_bits / tmr_bn_apply2_bits and their _a16 forms: z against float64 (fp32 < 3e-6,
    bf16 bound (b)) and the bits exactly (stored z > 0) packed 32 per word, ragged last word
    included; the 8-wide fp32 form (aligned, c % 8 == 0) and the 4-wide ones."""
    k = _fwd_case(rows, c)
    sc, sf, rs, rf = (up(k[n], dev) for n in ("sc", "sf", "rs", "rf"))
    for sfx, dt in (("", f32), ("16", BF16)):
        y, r, yr = (up(k[n + sfx], dev, dt, off=off) for n in ("y", "r", "yr"))
        runs = [(ops.bn_apply_bits(y, sc, sf), _fwd_ref(k, sfx, False, True)),
                (ops.bn_apply_bits(y, sc, sf, r), _fwd_ref(k, sfx, True, True)),
                (ops.bn_apply2_bits(y, sc, sf, yr, rs, rf), _fwd_ref(k, sfx, False, True, branch=True))]
        for (z, bits), ref in runs:
            assert z.dtype == dt and no_nan(z)
            if dt == f32:
                assert rel_err(z, ref) < E_FWD
            else:
                assert bf16_excess(z, ref, E_FWD) <= 1.0
            assert torch.equal(bits.cpu(), _pack_bits(z.float().cpu() > 0))


@gpu
@pytest.mark.parametrize("c", [4, 12, 300, 2048])
def test_eval_params(dev, poison, c):
    """tmr_bn_eval_params: scale = gamma / sqrt(var + eps), shift = beta - mean scale, with and
    without gamma / beta; c = 300 leaves the second block partly empty."""
    g = torch.Generator().manual_seed(c)
    gamma, beta, rm, rv = pos(c, g), rnd(c, g=g), rnd(c, g=g), pos(c, g)
    for affine in (True, False):
        inv = 1.0 / torch.sqrt(rv + EPS)
        gm, bt = (gamma, beta) if affine else (torch.ones(c, dtype=f64), torch.zeros(c, dtype=f64))
        scale, shift = ops.bn_eval_params(up(gamma, dev) if affine else None,
                                          up(beta, dev) if affine else None, up(rm, dev),
                                          up(rv, dev), EPS)
        assert no_nan(scale) and no_nan(shift)
        assert rel_err(scale, gm * inv) < E_STAT and rel_err(shift, bt - rm * gm * inv) < E_STAT


# ------------------------------------------------------------------ 4. backward
def _masked(k, sfx, mask, gname="dz"):
    """-> (float64 masked gradient, float64 z handed to mask 1)"""
    y, g = k["y" + sfx], k[gname]
    z = torch.relu(y * k["scale"] + k["shift"] + k["r" + sfx])
    z = z.to(BF16 if sfx else f32).double()
    if mask == 1:
        return torch.where(z > 0, g, torch.zeros_like(g)), z
    if mask == 2:
        return torch.where(y * k["scale"] + k["shift"] > 0, g, torch.zeros_like(g)), z
    return g, z


def _run_bwd(dev, k, sfx, mask, dres_mode, off=False, bf16=False):
    """one ops.bn_bwd call of the fp32 (sfx "") or bf16-activation (sfx "16") form -> the outputs,
    the gradient buffer afterwards, the sentinel buffer of a separate dres"""
    rows, c = k["y"].shape
    dt = BF16 if sfx else f32
    dz = up(k["dz"], dev, off=off)
    y = up(k["y" + sfx], dev, dt, off=off)
    z = up(_masked(k, sfx, mask)[1], dev, dt, off=off) if mask == 1 else None
    buf, dres_out = None, None
    if dres_mode == "sep":
        buf, dres_out = guarded((rows, c), dev)
    elif dres_mode == "alias":
        dres_out = dz
    dy, dres, dgm, dbt = ops.bn_bwd(dz, y, z, up(k["mean"], dev), up(k["inv"], dev),
                                    up(k["gamma"], dev), mask != 0, want_dres=dres_mode != "none",
                                    dres_out=dres_out, scale=up(k["scale"], dev),
                                    shift=up(k["shift"], dev), bf16=bf16)
    return dy, dres, dgm, dbt, dz, buf


def _check_bwd(k, sfx, mask, dres_mode, out, dy_bf16, ref=None):
    dy, dres, dgm, dbt, dz, buf = out
    g64 = _masked(k, sfx, mask)[0]
    dy64, dg64, db64 = ref or closed_form(g64, k["y" + sfx], k["mean"], k["inv"], k["gamma"])
    tag = (sfx, mask, dres_mode, dy_bf16)
    assert no_nan(dy) and no_nan(dgm) and no_nan(dbt), tag
    if dy_bf16:
        assert dy.dtype == BF16 and bf16_excess(dy, dy64, E_BWD) <= 1.0, tag
    else:
        assert dy.dtype == f32 and rel_err(dy, dy64) < E_BWD, tag
    assert rel_err(dgm, dg64) < E_BWD and rel_err(dbt, db64) < E_BWD, tag
    if dres_mode == "sep":      # the masked gradient, dz untouched, nothing outside dres
        assert guards_ok(buf) and torch.equal(dres.cpu().double(), g64), tag
        assert torch.equal(dz.cpu().double(), k["dz"]), tag
    elif dres_mode == "alias":  # dz holds the masked gradient afterwards
        assert dres.data_ptr() == dz.data_ptr() and torch.equal(dz.cpu().double(), g64), tag
    else:
        assert dres is None and torch.equal(dz.cpu().double(), k["dz"]), tag


@gpu
@pytest.mark.parametrize("rows,c", SMALL)
def test_bwd_fp32(dev, poison, rows, c):
    """tmr_bn_bwd_x: mask 0 / 1 / 2 x dres none / separate / aliasing dz x dy fp32 / bf16.  The
    bf16 dy is bitwise the fp32 one rounded; an aliasing dres leaves the masked gradient in dz, a
    separate one leaves dz untouched."""
    k = _bwd_case(rows, c)
    for mask in (0, 1, 2):
        ref = closed_form(_masked(k, "", mask)[0], k["y"], k["mean"], k["inv"], k["gamma"])
        for dres_mode in ("none", "sep", "alias"):
            o32 = _run_bwd(dev, k, "", mask, dres_mode)
            _check_bwd(k, "", mask, dres_mode, o32, False, ref)
            o16 = _run_bwd(dev, k, "", mask, dres_mode, bf16=True)
            _check_bwd(k, "", mask, dres_mode, o16, True, ref)
            assert same_bits(o16[0], o32[0]), (mask, dres_mode)
            assert torch.equal(o16[2], o32[2]) and torch.equal(o16[3], o32[3])


@gpu
@pytest.mark.parametrize("off", [False, True], ids=["aligned", "off8"])
@pytest.mark.parametrize("rows,c", SMALL)
def test_bwd_a16(dev, poison, rows, c, off):
    """tmr_bn_bwd_a16 (bf16 y / z / dy, fp32 dz / dres): the same masks and dres forms; aligned
    operands with no mask left take bn_bwd_apply8_a16, operands 8 bytes off the 4-wide apply."""
    k = _bwd_case(rows, c)
    for mask in (0, 1, 2):
        ref = closed_form(_masked(k, "16", mask)[0], k["y16"], k["mean"], k["inv"], k["gamma"])
        for dres_mode in ("none", "sep", "alias"):
            _check_bwd(k, "16", mask, dres_mode, _run_bwd(dev, k, "16", mask, dres_mode, off=off),
                       True, ref)


@gpu
@pytest.mark.parametrize("rows,c", BIG)
def test_bwd_big(dev, poison, rows, c):
    """(530, 2048): 8 channel blocks; (40037, 256): make_plan's rpb = rows / 1024 branch.  One
    fp32 form (mask 2, dres aliasing dz: the write-back) and one bf16-activation form (mask 1,
    separate dres)."""
    k = _bwd_case(rows, c)
    _check_bwd(k, "", 2, "alias", _run_bwd(dev, k, "", 2, "alias"), False)
    _check_bwd(k, "16", 1, "sep", _run_bwd(dev, k, "16", 1, "sep"), True)


@gpu
@pytest.mark.parametrize("rows,c", [(3, 8), (101, 24), (1001, 64), (530, 2048)])
def test_bwd_g16(dev, poison, rows, c):
    """tmr_bn_bwd_g16 (bf16 dz, y, dy; no mask): dy within bound (b), dgamma / dbeta < 1e-5."""
    k = _bwd_case(rows, c)
    dy64, dg64, db64 = closed_form(k["dz16"], k["y16"], k["mean"], k["inv"], k["gamma"])
    dy, dres, dgm, dbt = ops.bn_bwd(up(k["dz16"], dev, BF16), up(k["y16"], dev, BF16), None,
                                    up(k["mean"], dev), up(k["inv"], dev), up(k["gamma"], dev), False)
    assert dres is None and dy.dtype == BF16 and no_nan(dy)
    assert bf16_excess(dy, dy64, E_BWD) <= 1.0
    assert rel_err(dgm, dg64) < E_BWD and rel_err(dbt, db64) < E_BWD


@gpu
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows,c", [(3, 8), (101, 24), (1001, 64), (530, 2048)])
def test_bwd_parts_ds(dev, poison, rows, c, bf16):
    """tmr_bn_bwd_parts_ds: bn3 from fabricated partials, the downsample BN from its own reduction
    over (g, y_ds), one apply (bn_bwd_apply_ds8) -- all six outputs against float64."""
    k = _bwd_case(rows, c)
    sfx, dt = ("16", BF16) if bf16 else ("", f32)
    gv, y, yd = k["dz" + sfx], k["y" + sfx], k["yd" + sfx]
    nparts = min(rows, 7)
    parts, S, Q = _parts_of(gv, y, k["mean"], nparts, rows + c)
    ref3 = closed_form(gv, y, k["mean"], k["inv"], k["gamma"], S, Q)
    refd = closed_form(gv, yd, k["mean_d"], k["inv_d"], k["gamma_d"])
    f = lambda n: up(k[n], dev)
    out = ops.bn_bwd_parts_ds(up(gv, dev, dt), up(y, dev, dt), parts.to(dev), nparts, f("mean"),
                              f("inv"), f("gamma"), up(yd, dev, dt), f("mean_d"), f("inv_d"),
                              f("gamma_d"))
    for (dy, dgm, dbt), (dy64, dg64, db64) in ((out[:3], ref3), (out[3:], refd)):
        assert dy.dtype == dt and no_nan(dy)
        if bf16:
            assert bf16_excess(dy, dy64, E_BWD) <= 1.0
        else:
            assert rel_err(dy, dy64) < E_BWD
        assert rel_err(dgm, dg64) < E_BWD and rel_err(dbt, db64) < E_BWD


@gpu
@pytest.mark.parametrize("mask", [0, 2])
def test_frozen_bwd_ds_mask(dev, poison, mask):
    """tmr_bn_frozen_bwd_ds with mask 2 (bn_frozen_bwd8_k<2, true>, the one rung of bn.hip that no
    other test reaches, profiles/bn_dispatch/rungs.md) and mask 0 (<0, true>, elsewhere run but not
    compared): g as it is or masked by y * scale + shift > 0, then dy = g scale, dy_ds = g scale_ds
    and the partial sums of g, g (y - mean), g (y_ds - mean_ds)."""
    rows, c = 3, 8
    k = _bwd_case(rows, c)
    gm, _ = _masked(k, "", mask)
    f = lambda n: up(k[n], dev)
    # (gamma_d serves as the downsample BN's scale: an arbitrary fp32 vector)
    dy, dyd, _, parts, parts_d, nparts = ops.bn_frozen_bwd_ds(
        f("dz"), f("y"), f("scale"), f("shift"), f("mean"), f("yd"), f("gamma_d"), f("mean_d"), mask=mask)
    assert no_nan(dy) and no_nan(dyd)
    assert rel_err(dy, gm * k["scale"]) < E_BWD and rel_err(dyd, gm * k["gamma_d"]) < E_BWD
    for p, y, mean in ((parts, "y", "mean"), (parts_d, "yd", "mean_d")):
        assert p.shape == (nparts, c, 2) and no_nan(p)
        sums = p.double().sum(0)
        assert rel_err(sums[:, 0], gm.sum(0)) < E_BWD
        assert rel_err(sums[:, 1], (gm * (k[y] - k[mean])).sum(0)) < E_BWD


# ------------------------------------------------------------------ 5. stem
STEM_CASES = [(2, 13, 11, 16), (1, 8, 8, 64), (2, 9, 10, 24)]


@functools.lru_cache(maxsize=None)
def _stem_ref(n, h, w, c):
    g = torch.Generator().manual_seed(n + h * 3 + w * 5 + c)
    # quantised to a few levels (as _stem_case of test_stem_pool8_gpu): windows tie; bf16-exact
    y = torch.randint(-6, 7, (n, h, w, c), generator=g).double() / 4
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return dict(y=y, scale=pos(c, g), shift=rnd(c, g=g, scale=0.2), dyp=rnd(n, ho, wo, c, g=g),
                mean=rnd(c, g=g, scale=0.3), inv=pos(c, g), gamma=rnd(c, g=g, shift=0.3))


def _stem_closed(k, am):
    """scatter of dyp through argmax (ids 0..8 in the 3x3 window, padded coordinates), the
    recomputed ReLU mask and the closed form, all float64 on the CPU"""
    n, h, w, c = k["y"].shape
    ids = am.cpu().long()
    _, ho, wo, _ = ids.shape
    dz = torch.zeros(n, h + 2, w + 2, c, dtype=f64)
    oy = torch.arange(ho).view(1, ho, 1, 1) * 2
    ox = torch.arange(wo).view(1, 1, wo, 1) * 2
    nn_ = torch.arange(n).view(n, 1, 1, 1).expand_as(ids)
    cc = torch.arange(c).view(1, 1, 1, c).expand_as(ids)
    dz.index_put_((nn_, oy + ids // 3, ox + ids % 3, cc), k["dyp"], accumulate=True)
    dz = dz[:, 1:h + 1, 1:w + 1]
    g64 = torch.where(k["y"] * k["scale"] + k["shift"] > 0, dz, torch.zeros_like(dz))
    dy, dg, db = closed_form(g64.reshape(-1, c), k["y"].reshape(-1, c), k["mean"], k["inv"], k["gamma"])
    return dy.view(n, h, w, c), dg, db


@gpu
@pytest.mark.parametrize("off", [False, True], ids=["aligned", "off8"])
@pytest.mark.parametrize("shape", STEM_CASES)
def test_bwd_maxpool(dev, poison, shape, off):
    """tmr_bn_bwd_maxpool_x (fp32 and bf16 dy) and tmr_bn_bwd_maxpool_a16 on quantised y: the quad
    form ((2, 13, 11, 16), (1, 8, 8, 64), aligned) and the per-pixel form (c = 24, or operands 8
    bytes off).  dy, dgamma, dbeta against float64; the bf16 dy of fp32 y bitwise the fp32 one."""
    k = _stem_ref(*shape)
    f = lambda n: up(k[n], dev)
    for dt in (f32, BF16):
        ya = up(k["y"], dev, dt)
        _, am = ops.maxpool_fwd_bn(ya, f("scale"), f("shift"))
        dy64, dg64, db64 = _stem_closed(k, am)
        y = _off8(ya) if off else ya
        dyp = up(k["dyp"], dev, off=off)
        args = (dyp, am, y, f("scale"), f("shift"), f("mean"), f("inv"), f("gamma"))
        dy, dgm, dbt = ops.bn_bwd_maxpool(*args)
        assert dy.dtype == dt and no_nan(dy)
        assert rel_err(dgm, dg64) < E_BWD and rel_err(dbt, db64) < E_BWD
        if dt == BF16:
            assert bf16_excess(dy, dy64, E_BWD) <= 1.0
            continue
        assert rel_err(dy, dy64) < E_BWD
        dy16, dgm16, dbt16 = ops.bn_bwd_maxpool(*args, bf16=True)
        assert dy16.dtype == BF16 and same_bits(dy16, dy) and bf16_excess(dy16, dy64, E_BWD) <= 1.0
        assert torch.equal(dgm16, dgm) and torch.equal(dbt16, dbt)


# ------------------------------------------------------------------ the unsuffixed entry points
@gpu
def test_plain_entry_points(dev, poison):
    """tmr_bn_apply, tmr_bn_apply2, tmr_bn_bwd, tmr_bn_bwd_parts and tmr_bn_bwd_maxpool (the
    wrappers call their _x forms) through the binding, against float64."""
    rows, c = 77, 12
    k, b = _fwd_case(rows, c), _bwd_case(rows, c)
    f = lambda t: up(t, dev)
    y, r, yr = f(k["y"]), f(k["r"]), f(k["yr"])
    z = torch.empty_like(y)
    call("tmr_bn_apply", y, f(k["sc"]), f(k["sf"]), r, z, rows, c, 1, stream_ptr())
    assert no_nan(z) and rel_err(z, _fwd_ref(k, "", True, True)) < E_FWD
    z = torch.empty_like(y)
    call("tmr_bn_apply2", y, f(k["sc"]), f(k["sf"]), yr, f(k["rs"]), f(k["rf"]), z, rows, c, 1,
         stream_ptr())
    assert no_nan(z) and rel_err(z, _fwd_ref(k, "", False, True, branch=True)) < E_FWD
    # tmr_bn_bwd, mask 1 with a separate dres
    g64, z64 = _masked(b, "", 1)
    dy64, dg64, db64 = closed_form(g64, b["y"], b["mean"], b["inv"], b["gamma"])
    nb = query("tmr_bn_ws_bytes", rows, c)
    ws = torch.empty((nb + 7) // 8, dtype=f64, device=dev)
    dy, dres = torch.empty_like(y), torch.empty_like(y)
    dgm, dbt = torch.empty(c, device=dev), torch.empty(c, device=dev)
    call("tmr_bn_bwd", f(b["dz"]), f(b["y"]), f(z64), None, None, f(b["mean"]), f(b["inv"]),
         f(b["gamma"]), dy, dres, dgm, dbt, rows, c, 1, ws, ctypes.c_size_t(nb), stream_ptr())
    assert rel_err(dy, dy64) < E_BWD and torch.equal(dres.cpu().double(), g64)
    assert rel_err(dgm, dg64) < E_BWD and rel_err(dbt, db64) < E_BWD
    # tmr_bn_bwd_parts
    parts, S, Q = _parts_of(b["dz"], b["y"], b["mean"], 5, 1)
    dy64, dg64, db64 = closed_form(b["dz"], b["y"], b["mean"], b["inv"], b["gamma"], S, Q)
    nb = query("tmr_bn_parts_ws_bytes", 5, c)
    ws = torch.empty((nb + 7) // 8, dtype=f64, device=dev)
    dy = torch.empty_like(y)
    call("tmr_bn_bwd_parts", f(b["dz"]), f(b["y"]), parts.to(dev), 5, f(b["mean"]), f(b["inv"]),
         f(b["gamma"]), dy, dgm, dbt, rows, c, ws, ctypes.c_size_t(ws.numel() * 8), stream_ptr())
    assert no_nan(dy) and rel_err(dy, dy64) < E_BWD
    assert rel_err(dgm, dg64) < E_BWD and rel_err(dbt, db64) < E_BWD
    # tmr_bn_bwd_maxpool
    shape = STEM_CASES[0]
    n, h, w, cs = shape
    s = _stem_ref(*shape)
    ys = f(s["y"])
    _, am = ops.maxpool_fwd_bn(ys, f(s["scale"]), f(s["shift"]))
    dy64, dg64, db64 = _stem_closed(s, am)
    nb = query("tmr_bn_ws_bytes", n * h * w, cs)
    ws = torch.empty((nb + 7) // 8, dtype=f64, device=dev)
    dy = torch.empty_like(ys)
    dgm, dbt = torch.empty(cs, device=dev), torch.empty(cs, device=dev)
    call("tmr_bn_bwd_maxpool", f(s["dyp"]), am, n, h, w, am.shape[1], am.shape[2], ys, f(s["scale"]),
         f(s["shift"]), f(s["mean"]), f(s["inv"]), f(s["gamma"]), dy, dgm, dbt, cs, ws,
         ctypes.c_size_t(nb), stream_ptr())
    assert no_nan(dy) and rel_err(dy, dy64) < E_BWD
    assert rel_err(dgm, dg64) < E_BWD and rel_err(dbt, db64) < E_BWD


# ------------------------------------------------------------------ grid cap: the second trip
CAP_ROWS = 16400           # x 1024 (4-wide kernels) / x 2048 (8-wide): 16 rows past one trip
HEAD = 4096


def _dev_randn(rows, c, dev, seed, dtype=f32, scale=1.0):
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.randn(rows, c, device=dev, generator=g) * scale).to(dtype)


def _coef(c, seed, n):
    g = torch.Generator().manual_seed(seed)
    return [rnd(c, g=g, shift=0.2) for _ in range(n)]


def _cap_slices(c, per_trip_elems):
    """the first HEAD rows, from the row of the first second-trip element to the end, and 256 rows
    from the middle of the first trip on (the threads' second groups, where a trip has two)"""
    first = per_trip_elems // c
    assert HEAD <= first // 2 and first < CAP_ROWS and per_trip_elems % c == 0
    return slice(0, HEAD), slice(first, CAP_ROWS), slice(first // 2, first // 2 + 256)


def _d(t, sl):
    return t[sl].double().cpu()


TRIP4 = 8192 * 256 * 2 * 4     # elements of one trip: 4-wide kernels, two groups per thread
TRIP8 = 8192 * 256 * 2 * 8
TRIP4_BITS = 8192 * 256 * 4    # bn_apply_bits_k: one group per thread and trip


@gpu
def test_cap_apply_fp32(dev, poison):
    """bn_apply_k<true, true> at (16400, 1024): the loop's second trip (and its `hj` element)."""
    c = 1024
    y, r = _dev_randn(CAP_ROWS, c, dev, 1), _dev_randn(CAP_ROWS, c, dev, 2)
    sc, sf = _coef(c, 3, 2)
    z = ops.bn_apply(y, up(sc, dev), up(sf, dev), r, True)
    assert not bool(torch.isnan(z).any())
    for sl in _cap_slices(c, TRIP4):
        assert rel_err(z[sl], torch.relu(_d(y, sl) * sc + sf + _d(r, sl))) < E_FWD


@gpu
def test_cap_bwd_mask1_dres(dev, poison):
    """bn_bwd_apply<1, true> at (16400, 1024) through tmr_bn_bwd_x: mask 1 and a separate dres."""
    c = 1024
    dz, y = _dev_randn(CAP_ROWS, c, dev, 4), _dev_randn(CAP_ROWS, c, dev, 5, scale=2.0)
    z = torch.relu(_dev_randn(CAP_ROWS, c, dev, 6))
    mean, inv, gamma = _coef(c, 7, 3)
    inv = (inv.abs() + 0.5).float().double()
    dy, dres, dgm, dbt = ops.bn_bwd(dz, y, z, up(mean, dev), up(inv, dev), up(gamma, dev), True,
                                    want_dres=True)
    assert not bool(torch.isnan(dy).any() or torch.isnan(dres).any())
    g64 = torch.where(z.cpu() > 0, dz.cpu().double(), torch.zeros((), dtype=f64))
    y64 = y.cpu().double()
    S, Q = g64.sum(0), (g64 * (y64 - mean)).sum(0)
    assert rel_err(dbt, S) < E_BWD and rel_err(dgm, inv * Q) < E_BWD
    for sl in _cap_slices(c, TRIP4):
        ref = gamma * inv * (g64[sl] - S / CAP_ROWS - (y64[sl] - mean) * inv * inv * Q / CAP_ROWS)
        assert rel_err(dy[sl], ref) < E_BWD
        assert torch.equal(_d(dres, sl), g64[sl])


@gpu
@pytest.mark.parametrize("c,off", [(1024, True), (2048, False)], ids=["bits4_off8", "bits8"])
def test_cap_apply_bits(dev, poison, c, off):
    """bn_apply_bits_k<true, float> from misaligned operands at (16400, 1024) (one group per trip:
    the second trip starts at row 8192) and bn_apply_bits8_k<true> at (16400, 2048)."""
    y, r = _dev_randn(CAP_ROWS, c, dev, 8), _dev_randn(CAP_ROWS, c, dev, 9)
    if off:
        y, r = _off8(y), _off8(r)
    sc, sf = _coef(c, 10, 2)
    z, bits = ops.bn_apply_bits(y, up(sc, dev), up(sf, dev), r)
    assert not bool(torch.isnan(z).any())
    for sl in _cap_slices(c, TRIP4_BITS if off else TRIP8):
        zs = z[sl].cpu()
        assert rel_err(zs, torch.relu(_d(y, sl) * sc + sf + _d(r, sl))) < E_FWD
        words = slice(sl.start * c // 32, sl.stop * c // 32)
        assert torch.equal(bits[words].cpu(), _pack_bits(zs > 0))


@gpu
def test_cap_apply_a16(dev, poison):
    """bn_apply8_a16_k<true, true, false> at (16400, 2048)."""
    c = 2048
    y, r = _dev_randn(CAP_ROWS, c, dev, 11, BF16), _dev_randn(CAP_ROWS, c, dev, 12, BF16)
    sc, sf = _coef(c, 13, 2)
    z = ops.bn_apply(y, up(sc, dev), up(sf, dev), r, True)
    assert z.dtype == BF16 and not bool(torch.isnan(z).any())
    for sl in _cap_slices(c, TRIP8):
        assert bf16_excess(z[sl], torch.relu(_d(y, sl) * sc + sf + _d(r, sl)), E_FWD) <= 1.0


@gpu
@pytest.mark.parametrize("ydt", [f32, BF16], ids=["apply8", "apply8_a16"])
def test_cap_bwd_parts(dev, poison, ydt):
    """bn_bwd_apply8_k (fp32 y) and bn_bwd_apply8_a16<float> (bf16 y) at (16400, 2048) through
    tmr_bn_bwd_parts_x / _a16.  The partials are inputs, so arbitrary ones serve: the reference is
    the closed form on the float64 sums of those partials."""
    c, nparts = 2048, 3
    gd, y = _dev_randn(CAP_ROWS, c, dev, 14), _dev_randn(CAP_ROWS, c, dev, 15, ydt, scale=2.0)
    mean, inv, gamma = _coef(c, 16, 3)
    inv = (inv.abs() + 0.5).float().double()
    parts = (torch.randn(nparts, c, 2, generator=torch.Generator().manual_seed(17)) * 50).float()
    S, Q = parts[:, :, 0].double().sum(0), parts[:, :, 1].double().sum(0)
    dy, dgm, dbt = ops.bn_bwd_parts(gd, y, parts.to(dev), nparts, up(mean, dev), up(inv, dev),
                                    up(gamma, dev))
    assert dy.dtype == ydt and not bool(torch.isnan(dy).any())
    assert rel_err(dbt, S) < E_BWD and rel_err(dgm, inv * Q) < E_BWD
    for sl in _cap_slices(c, TRIP8):
        ref = gamma * inv * (_d(gd, sl) - S / CAP_ROWS - (_d(y, sl) - mean) * inv * inv * Q / CAP_ROWS)
        if ydt == BF16:
            assert bf16_excess(dy[sl], ref, E_BWD) <= 1.0
        else:
            assert rel_err(dy[sl], ref) < E_BWD


@gpu
@pytest.mark.parametrize("dt", [BF16, f32], ids=["bf16", "fp32"])
def test_cap_bwd_parts_ds(dev, poison, dt):
    """bn_bwd_apply_ds8<__bf16 | float> at (16400, 2048) through tmr_bn_bwd_parts_ds: arbitrary
    partials for bn3, the downsample BN's sums taken over the whole tensors in float64."""
    c, nparts = 2048, 3
    gd, y, yd = (_dev_randn(CAP_ROWS, c, dev, 18 + i, dt, scale=s) for i, s in enumerate((1.0, 2.0, 1.5)))
    mean, inv, gamma, mean_d, inv_d, gamma_d = _coef(c, 21, 6)
    inv, inv_d = ((t.abs() + 0.5).float().double() for t in (inv, inv_d))
    parts = (torch.randn(nparts, c, 2, generator=torch.Generator().manual_seed(22)) * 50).float()
    S, Q = parts[:, :, 0].double().sum(0), parts[:, :, 1].double().sum(0)
    g64 = gd.cpu().double()
    Sd = g64.sum(0)
    Qd = (g64 * (yd.cpu().double() - mean_d)).sum(0)
    del g64
    f = lambda t: up(t, dev)
    dy, dgm, dbt, dyd, dgmd, dbtd = ops.bn_bwd_parts_ds(gd, y, parts.to(dev), nparts, f(mean), f(inv),
                                                        f(gamma), yd, f(mean_d), f(inv_d), f(gamma_d))
    assert not bool(torch.isnan(dy).any() or torch.isnan(dyd).any())
    assert rel_err(dbt, S) < E_BWD and rel_err(dgm, inv * Q) < E_BWD
    assert rel_err(dbtd, Sd) < E_BWD and rel_err(dgmd, inv_d * Qd) < E_BWD
    n = CAP_ROWS
    for sl in _cap_slices(c, TRIP8):
        gs = _d(gd, sl)
        ref = gamma * inv * (gs - S / n - (_d(y, sl) - mean) * inv * inv * Q / n)
        refd = gamma_d * inv_d * (gs - Sd / n - (_d(yd, sl) - mean_d) * inv_d * inv_d * Qd / n)
        if dt == BF16:
            assert bf16_excess(dy[sl], ref, E_BWD) <= 1.0 and bf16_excess(dyd[sl], refd, E_BWD) <= 1.0
        else:
            assert rel_err(dy[sl], ref) < E_BWD and rel_err(dyd[sl], refd) < E_BWD
