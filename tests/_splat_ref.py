"""Float64 references and elementwise error bounds for the entry points of csrc/resnest.hip: the
training split attention (unfused fp32 kernels and the forms with bn0 + ReLU applied on load), the
column centring, axpy and the general AvgPool2d.  CPU only; tests/test_splat_direct_cpu.py shows the
bounds are fair and sharp, tests/test_splat_direct_gpu.py holds the kernels to them.

The references are written from the formulas of include/tmr.h and the reference SplAtConv2d /
nn.AvgPool2d, one function per entry point, each returning (ref, bound) pairs.  Layouts:
x, y [n][hw][2C], dout / out [n][hw][C], z / att / dzl [n][2C], gap / dgap [n][C],
sums [4][n][2C], coef [3][2C], scale / shift / mean / invstd / gamma [2C].

Operands are float64 values the operand type holds exactly.  For the `_bn` kernels y, scale and
shift lie on a 2^-6 grid (y in [-4, 4], scale in [0.5, 1.5], shift in [-0.5, 0.5]: bf16-exact), so
y * scale + shift is exact in fp32: the ReLU mask and x_r = relu(.) -- and its bf16 rounding (RNE) --
are the same numbers on both sides.  Every second channel has scale a multiple of 2^-4 and
shift = -y0 * scale for a y0 in {-1/4, 0, 1/4} that an eighth of that channel's y take, so about
1/16 of the pre-activations are exactly 0 and pin the strict `> 0`.  Everything else (att, dout,
dgap, mean, invstd, gamma, coef, sums) is arbitrary fp32, not derived from y: each kernel is held to
its own formula.

Bounds, elementwise, U = 2^-24 (fp32 unit roundoff), derived from the roundings of the documented
arithmetic:
  double accumulation, one rounding to fp32     2U |ref| + 2^-40 sum |terms|   (gap, bwd, dzl, S1,
                                                 coefs, center)
  S3, S4                                        + U sum |m dout (y - mean)|, + U sum m |y - mean|:
                                                 y - mean is an fp32 subtraction
  S2                                            a count: exact
  att                                           (|z0 - z1| + 8) U att + 1e-37: z - max carries
                                                 U |z0 - z1|, which exp turns into a relative error;
                                                 expf, the sum, the reciprocal, the product;
                                                 1e-37 for results below the normal range
  a0 + a1 - 1                                   2U: of s = fl(e0 + e1), inv = fl(1 / s), fl(e0 inv),
                                                 fl(e1 inv) the first two give 2^-24 / s + 2^-25 s
                                                 <= 1.5U for s in [1, 2], the products half an ulp
                                                 each of numbers in [1/2, 1) and below 1/2: 0.75U.
                                                 The four would have to align for 2.25U; the emulation
                                                 stays below 2U on every case of the suite
  combine                                       (|z0 - z1| + 12) U (|a0 x0| + |a1 x1|)
  combine_bn                                    3U (|a0 x0| + |a1 x1|): a product and an fma
  bwd_apply                                     4U (|att dout| + |dgap| / hw): 1/hw, dgap * (1/hw),
                                                 the product, the sum
  bwd_apply_bn                                  6U |k0| (|att dout| + |dgap|/hw + |k1| + |(y-mean) k2|)
  axpy                                          2U |ref| (one fma)
  avgpool2d                                     (T + 2) U sum_window |v| / div, T = k^2 additions
                                                 forward and ceil(k/s)^2 products + additions backward,
                                                 + the reciprocal and the product by it
  bf16 outputs                                  the fp32 bound + 2^-8 |ref|
"""
import functools
import math

import torch
import torch.nn.functional as F

f64 = torch.float64
f32 = torch.float32
BF16 = torch.bfloat16
U = 2.0 ** -24
T40 = 2.0 ** -40
B8 = 2.0 ** -8

# (n, h, w, C) -- what each is for: module docstring of tests/test_splat_direct_gpu.py
SMALL = [(1, 1, 1, 4), (3, 5, 3, 12), (2, 4, 5, 24), (5, 7, 7, 40), (6, 7, 7, 64), (3, 10, 30, 264),
         (4, 7, 7, 512), (2, 3, 1, 2048)]
BIG_SCALAR = (5, 29, 29, 512)
BIG_4WIDE = (5, 29, 29, 2048)
BIG_8WIDE = (10, 29, 29, 2048)
BIG_ATT = (1025, 2048)
AXPY_N = [1, 255, 256, 257, 2 ** 21 + 3]
ROWS = [1, 5, 16, 17, 33]
COLS = [8, 48, 64, 80, 1024]

# (n, h, w, c, k, s, p, count_include_pad, ceil_mode)
POOL_OVERHANG = [(2, 5, 5, 8, 2, 2, 0, True, True), (2, 6, 6, 8, 3, 2, 1, True, True),
                 (2, 15, 13, 12, 2, 2, 0, True, True)]
POOL_SMALL = POOL_OVERHANG + [(2, 7, 7, 4, 1, 1, 0, False, True), (2, 1, 9, 8, 3, 2, 1, True, False),
                              (2, 9, 1, 8, 2, 2, 0, False, True), (2, 7, 7, 12, 3, 1, 1, True, False)]
POOL_BIG_BWD = (33, 32, 32, 256, 2, 2, 0, False, True)
POOL_BIG_FWD = (33, 64, 64, 256, 2, 2, 0, False, True)


# ------------------------------------------------------------------ operands
def rnd(*shape, g, scale=1.0, shift=0.0):
    """float64 values that fp32 holds exactly"""
    return (torch.randn(*shape, generator=g, dtype=f64) * scale + shift).float().double()


def rnd16(*shape, g, scale=1.0, shift=0.0):
    """float64 values that bf16 holds exactly"""
    return (torch.randn(*shape, generator=g, dtype=f64) * scale + shift).to(BF16).double()


def pos(*shape, g):
    """fp32-exact values in [0.5, 1.5)"""
    return (torch.rand(*shape, generator=g, dtype=f64) + 0.5).float().double()


def grid_bn(n, hw, C, g):
    """y [n][hw][2C], scale, shift [2C] on the 2^-6 grid, with the planted zeros (module docstring)"""
    c2 = 2 * C
    y = torch.randint(-256, 257, (n, hw, c2), generator=g).double() / 64
    scale = torch.randint(32, 97, (c2,), generator=g).double() / 64
    shift = torch.randint(-32, 33, (c2,), generator=g).double() / 64
    even = torch.arange(c2) % 2 == 0
    scale4 = torch.randint(8, 25, (c2,), generator=g).double() / 16
    y0 = torch.randint(-1, 2, (c2,), generator=g).double() / 4
    scale = torch.where(even, scale4, scale)
    shift = torch.where(even, -y0 * scale4, shift)
    plant = (torch.rand(n, hw, c2, generator=g) < 0.125) & even
    y = torch.where(plant, y0.expand(n, hw, c2), y)
    assert torch.equal(y, y.to(BF16).double()) and torch.equal(scale, scale.to(BF16).double())
    assert torch.equal(shift, shift.to(BF16).double())
    v = y * scale + shift
    assert torch.equal(v, v.float().double())
    return y, scale, shift


def logits(n, C, g):
    """fc2 logits [n][2C]: N(0, 3) with planted pairs -- equal, +-30 and +-100 apart"""
    z = rnd(n, 2 * C, g=g, scale=3.0)
    m = n * C
    if m >= 36:
        for i, d in enumerate((0.0, 30.0, -30.0, 100.0, -100.0)):
            j = m - 1 - 7 * i                   # the last pair and four more near the end
            z0 = torch.round(z[j // C, j % C] * 1024) / 1024     # z0 - d stays fp32-exact
            z[j // C, j % C], z[j // C, C + j % C] = z0, z0 - d
    assert torch.equal(z, z.float().double())
    return z


@functools.lru_cache(maxsize=2)
def splat_case(n, h, w, C, need="xy"):
    """every operand of the split-attention entry points at one shape (float64, exact in the
    operand type); computed once, shared, never written.  need: which of the two [n][hw][2C]
    tensors to build (the BIG shapes take one: 34 M float64 each)"""
    g = torch.Generator().manual_seed(((n * 31 + h) * 31 + w) * 31 + C)
    hw, c2 = h * w, 2 * C
    y, scale, shift = grid_bn(n, hw if "y" in need else 0, C, g)
    return dict(n=n, hw=hw, C=C, y=y, scale=scale, shift=shift,
                x=rnd(n, hw if "x" in need else 0, c2, g=g, shift=0.3), z=logits(n, C, g),
                att=rnd(n, c2, g=g, scale=0.3, shift=0.5), dout=rnd(n, hw, C, g=g),
                dgap=rnd(n, C, g=g, scale=2.0), mean=rnd(c2, g=g, scale=0.5, shift=0.2),
                invstd=pos(c2, g=g), gamma=rnd(c2, g=g, shift=0.3),
                coef=rnd(3, c2, g=g, scale=0.5, shift=0.2), sums=rnd(4, n, c2, g=g, scale=float(hw)))


def center_case(rows, cols):
    """GAP rows as tmr_center_cols meets them: a per-column base plus 1 % spread"""
    g = torch.Generator().manual_seed(rows * 1000 + cols)
    base = rnd(cols, g=g, shift=1.0)
    return (base * (1 + 0.01 * torch.randn(rows, cols, generator=g, dtype=f64))).float().double()


def pool_case(case):
    """-> fp32-exact x, bf16-exact x (NHWC float64) and the generator, for dy"""
    n, h, w, c = case[:4]
    g = torch.Generator().manual_seed(sum(case[:7]))
    return rnd(n, h, w, c, g=g), rnd16(n, h, w, c, g=g), g


def halves(t, C):
    return t[..., :C], t[..., C:]


def bnrelu(y, scale, shift, bf16):
    """-> x_r (rounded to bf16 under act16), ReLU mask; y * scale + shift is exact (grid)"""
    v = y * scale + shift
    x = torch.relu(v)
    return (x.to(BF16).double() if bf16 else x), v > 0


# ------------------------------------------------------------------ references
def ref_gap(x, C):
    x0, x1 = halves(x, C)
    ref = (x0 + x1).mean(1)
    return ref, 2 * U * ref.abs() + T40 * (x0.abs() + x1.abs()).mean(1)


def ref_gap_bn(y, scale, shift, C, bf16):
    return ref_gap(bnrelu(y, scale, shift, bf16)[0], C)


def ref_att(z, C):
    z0, z1 = halves(z, C)
    a = torch.softmax(torch.stack([z0, z1]), 0)
    att = torch.cat([a[0], a[1]], -1)
    d = (z0 - z1).abs()
    return att, (torch.cat([d, d], -1) + 8) * U * att + 1e-37


def ref_combine(x, z, C):
    """-> (att, bound), (out, bound)"""
    att, batt = ref_att(z, C)
    (a0, a1), (x0, x1) = halves(att, C), halves(x, C)
    a0, a1 = a0.unsqueeze(1), a1.unsqueeze(1)
    d = (z[:, :C] - z[:, C:]).abs().unsqueeze(1)
    return (att, batt), (a0 * x0 + a1 * x1, (d + 12) * U * ((a0 * x0).abs() + (a1 * x1).abs()))


def ref_combine_bn(y, scale, shift, att, C, bf16):
    x, _ = bnrelu(y, scale, shift, bf16)
    (a0, a1), (x0, x1) = halves(att, C), halves(x, C)
    a0, a1 = a0.unsqueeze(1), a1.unsqueeze(1)
    ref = a0 * x0 + a1 * x1
    bound = 3 * U * ((a0 * x0).abs() + (a1 * x1).abs())
    return ref, (bound + B8 * ref.abs() if bf16 else bound)


def _softmax_bwd(dout, x, att, C):
    """dz [n][2C] of da_r = sum_hw dout x_r through the radix softmax, with its bound"""
    x0, x1 = halves(x, C)
    a0, a1 = halves(att, C)
    p0, p1 = (dout * x0).sum(1), (dout * x1).sum(1)
    dot = a0 * p0 + a1 * p1
    ref = torch.cat([a0 * (p0 - dot), a1 * (p1 - dot)], -1)
    mag = ((dout * x0).abs() + (dout * x1).abs()).sum(1)
    return ref, 2 * U * ref.abs() + T40 * torch.cat([mag, mag], -1)


def ref_bwd(dout, x, att, C):
    return _softmax_bwd(dout, x, att, C)


def ref_bwd_reduce_bn(dout, y, scale, shift, mean, att, C, bf16):
    """-> (dzl, bound), (sums [4][n][2C], bound [4][n][2C]); the S2 bound is 0"""
    x, m = bnrelu(y, scale, shift, bf16)
    g2 = torch.cat([dout, dout], -1)
    m = m.double()
    d = y - mean
    sums = torch.stack([(m * g2).sum(1), m.sum(1), (m * g2 * d).sum(1), (m * d).sum(1)])
    a1, a3, a4 = (m * g2).abs().sum(1), (m * g2 * d).abs().sum(1), (m * d).abs().sum(1)
    b = torch.stack([2 * U * sums[0].abs() + T40 * a1, torch.zeros_like(a1),
                     2 * U * sums[2].abs() + (T40 + U) * a3, 2 * U * sums[3].abs() + (T40 + U) * a4])
    return _softmax_bwd(dout, x, att, C), (sums, b)


def ref_bn0_coefs(att, dgap, sums, invstd, gamma, n, hw, C):
    """-> dict name -> (ref, bound) for dgamma, dbeta and the three coef rows"""
    dg = torch.cat([dgap, dgap], -1) / hw
    t = [att * sums[0], dg * sums[1], att * sums[2], dg * sums[3]]
    sg, sgx = (t[0] + t[1]).sum(0), (t[2] + t[3]).sum(0)
    mg, mgx = (t[0].abs() + t[1].abs()).sum(0), (t[2].abs() + t[3].abs()).sum(0)
    N = float(n * hw)
    out = {"dbeta": (sg, mg), "dgamma": (sgx * invstd, mgx * invstd),
           "coef0": (gamma * invstd, torch.zeros_like(sg)), "coef1": (sg / N, mg / N),
           "coef2": (invstd * invstd * sgx / N, invstd * invstd * mgx / N)}
    return {k: (r, 2 * U * r.abs() + T40 * m) for k, (r, m) in out.items()}


def ref_bwd_apply(dout, att, dgap, hw):
    ad = att.unsqueeze(1) * torch.cat([dout, dout], -1)
    dg = torch.cat([dgap, dgap], -1).unsqueeze(1) / hw
    return ad + dg, 4 * U * (ad.abs() + dg.abs())


def ref_bwd_apply_bn(dout, y, scale, shift, mean, att, dgap, coef, hw, bf16):
    _, m = bnrelu(y, scale, shift, bf16)
    m = m.double()
    ad = att.unsqueeze(1) * torch.cat([dout, dout], -1)
    dg = torch.cat([dgap, dgap], -1).unsqueeze(1) / hw
    k0, k1, k2 = coef[0], coef[1], coef[2]
    ref = k0 * (m * (ad + dg) - k1 - (y - mean) * k2)
    bound = 6 * U * k0.abs() * (ad.abs() + dg.abs() + k1.abs() + ((y - mean) * k2).abs())
    return ref, (bound + B8 * ref.abs() if bf16 else bound)


def ref_center_cols(x):
    ref = x.mean(0)
    return ref, 2 * U * ref.abs() + T40 * x.abs().mean(0)


def ref_axpy(alpha, x, y):
    ref = y + alpha * x
    return ref, 2 * U * ref.abs()


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def ref_avgpool2d_fwd(x, k, s, p, incl, ceil, bf16=False):
    """x NHWC float64 -> (y NHWC, bound): F.avg_pool2d, and the same pool of |x| for the bound"""
    pool = lambda t: _nhwc(F.avg_pool2d(_nchw(t), k, s, p, ceil_mode=ceil, count_include_pad=incl))
    ref = pool(x)
    bound = (k * k + 2) * U * pool(x.abs())
    return ref, (bound + B8 * ref.abs() if bf16 else bound)


def ref_avgpool2d_bwd(dy, hw_in, k, s, p, incl, ceil):
    """dy NHWC float64 -> (dx NHWC, bound): autograd of F.avg_pool2d; the pool is linear, so its
    gradient at |dy| is sum |dy| / div over the windows that hold the input cell"""
    n, _, _, c = dy.shape

    def grad(gy):
        x = torch.zeros(n, c, *hw_in, dtype=f64, requires_grad=True)
        F.avg_pool2d(x, k, s, p, ceil_mode=ceil, count_include_pad=incl).backward(_nchw(gy))
        return _nhwc(x.grad)

    T = math.ceil(k / s) ** 2
    return grad(dy), (T + 2) * U * grad(dy.abs())


# ------------------------------------------------------------------ judging
def ratio(out, ref, bound):
    """max over elements of |out - ref| / bound (0 / 0 = 0: an exact result with bound 0 passes,
    any error with bound 0 is inf)"""
    out = out.detach().double().cpu()
    assert out.shape == ref.shape, (tuple(out.shape), tuple(ref.shape))
    err = (out - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    r = torch.where(torch.isnan(out), torch.full_like(r, float("inf")), r)
    return r.max().item() if r.numel() else 0.0
