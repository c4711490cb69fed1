// BatchNorm2d (train-mode batch statistics) + ReLU + residual for NHWC fp32.
//
// Replaces nn.BatchNorm2d / ReLU / the residual add inside torchvision's
// resnet50 Bottleneck (the `share` trunk of
// code/Training TMRNet/train_only_non-local_pretrained.py:204-214).
// Statistics: per-thread fp32 sums of (y - shift_c) (shift = first row, removes
// the mean bias), per-block double partials, fixed-order double reduction ->
// deterministic and accurate for rows up to millions.  HBM-bound kernels:
// float4 loads/stores along channels, grid sized to fill 256 CUs.
#include "common.h"
#include "tmr.h"
#include <type_traits>

namespace {

constexpr int NT = 256;

struct Plan {
  int cthreads;  // threads across channels (each 4 channels)
  int rthreads;  // threads across rows
  int cblocks;   // gridDim.y
  int rpb;       // rows per block
  int nrb;       // row blocks (gridDim.x)
};

Plan make_plan(int rows, int c) {
  Plan p;
  int c4 = c / 4;
  p.cthreads = c4 < 64 ? c4 : 64;
  p.rthreads = NT / p.cthreads;
  p.cblocks = c4 / p.cthreads;
  // ~1024 row blocks for large inputs, >= 8 rows per thread
  int rpb = rows / 1024;
  int minr = p.rthreads * 8;
  if (rpb < minr) rpb = minr;
  rpb = (rpb + p.rthreads - 1) / p.rthreads * p.rthreads;
  p.rpb = rpb;
  p.nrb = (rows + rpb - 1) / rpb;
  return p;
}

// make_plan's grid covers cblocks * cthreads channel groups: every c / 4 up to 64 and every
// multiple of 64 above.  Any other count (c = 320) would leave channels without partials, so the
// entry points that reduce with a Plan refuse it.
bool plan_covers(int c) {
  const int c4 = c / 4;
  return c4 > 0 && c4 % (c4 < 64 ? c4 : 64) == 0;
}

// layout of the double workspace: [nrb][c][2] partials, then float coeffs [3][c]
size_t ws_need(int rows, int c) {
  Plan p = make_plan(rows, c);
  return (size_t)p.nrb * c * 2 * sizeof(double) + (size_t)3 * c * sizeof(float) + 64;
}

__global__ __launch_bounds__(NT) void bn_stats_partial(const float* __restrict__ y, int rows, int c,
                                                       int rpb, int cthreads,
                                                       float4* __restrict__ part) {
  const int tc = threadIdx.x % cthreads, tr = threadIdx.x / cthreads;
  const int rthreads = NT / cthreads;
  const int ch = (blockIdx.y * cthreads + tc) * 4;
  const int r0 = blockIdx.x * rpb;
  const int r1 = min(rows, r0 + rpb);
  // shift by the block's first row: removes the mean from the fp32 sums
  const float4 sh = *reinterpret_cast<const float4*>(y + (long)r0 * c + ch);
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f), q = s;
  for (int r = r0 + tr; r < r1; r += rthreads) {
    float4 v = *reinterpret_cast<const float4*>(y + (long)r * c + ch);
    float a = v.x - sh.x, b = v.y - sh.y, cc = v.z - sh.z, d = v.w - sh.w;
    s.x += a; s.y += b; s.z += cc; s.w += d;
    q.x += a * a; q.y += b * b; q.z += cc * cc; q.w += d * d;
  }
  __shared__ double red[NT][8];
  red[threadIdx.x][0] = s.x; red[threadIdx.x][1] = s.y; red[threadIdx.x][2] = s.z;
  red[threadIdx.x][3] = s.w; red[threadIdx.x][4] = q.x; red[threadIdx.x][5] = q.y;
  red[threadIdx.x][6] = q.z; red[threadIdx.x][7] = q.w;
  __syncthreads();
  if (tr == 0) {
    double acc[8];
    for (int e = 0; e < 8; ++e) acc[e] = 0.0;
    for (int k = 0; k < rthreads; ++k)
      for (int e = 0; e < 8; ++e) acc[e] += red[k * cthreads + tc][e];
    const double n = (double)(r1 - r0);
    const float shv[4] = {sh.x, sh.y, sh.z, sh.w};
    for (int e = 0; e < 4; ++e) {
      const double ms = acc[e] / n;
      double m2 = acc[4 + e] - acc[e] * ms;
      if (m2 < 0) m2 = 0;
      part[(long)blockIdx.x * c + ch + e] = make_float4((float)n, (float)(shv[e] + ms), (float)m2, 0.f);
    }
  }
}

// Combine of (n, mean, M2) partials in double, fixed order -> deterministic.  One
// workgroup per channel (the conv epilogue emits ~8k partials per channel for layer1-sized
// outputs, so the combine needs the whole chip).  Division-free shifted sums about
// K = the first partial's mean: N = sum n_b, S1 = sum n_b d_b, S2 = sum (M2_b + n_b d_b^2),
// d_b = mean_b - K; then mean = K + S1/N and M2 = S2 - S1^2/N (exact in exact arithmetic;
// the shift keeps the cancellation at the size of the spread of the partial means).
__global__ __launch_bounds__(NT) void bn_finalize_k(const float4* __restrict__ part, int nparts,
                                                    int c, const float* gamma, const float* beta,
                                                    float* rmean, float* rvar, float momentum,
                                                    float eps, float* smean, float* sinv,
                                                    float* scale, float* shift) {
  const int ch = blockIdx.x;
  const double K = part[ch].y;
  double n = 0, s1 = 0, s2 = 0;
  for (int b = threadIdx.x; b < nparts; b += NT) {
    const float4 p = part[(long)b * c + ch];
    const double nb = p.x, d = (double)p.y - K;
    n += nb;
    s1 = fma(nb, d, s1);
    s2 += (double)p.z + nb * d * d;
  }
  __shared__ double red[3][NT];
  red[0][threadIdx.x] = n; red[1][threadIdx.x] = s1; red[2][threadIdx.x] = s2;
  __syncthreads();
  for (int h = NT / 2; h > 0; h >>= 1) {
    if (threadIdx.x < h) {
      red[0][threadIdx.x] += red[0][threadIdx.x + h];
      red[1][threadIdx.x] += red[1][threadIdx.x + h];
      red[2][threadIdx.x] += red[2][threadIdx.x + h];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    n = red[0][0]; s1 = red[1][0]; s2 = red[2][0];
    const double mean = n > 0 ? K + s1 / n : 0.0;
    double m2 = n > 0 ? s2 - s1 * (s1 / n) : 0.0;
    if (m2 < 0) m2 = 0;
    const double var = n > 0 ? m2 / n : 0.0;
    const double inv = 1.0 / sqrt(var + (double)eps);
    smean[ch] = (float)mean;
    sinv[ch] = (float)inv;
    const double gm = gamma ? gamma[ch] : 1.0;
    const double bt = beta ? beta[ch] : 0.0;
    scale[ch] = (float)(gm * inv);
    shift[ch] = (float)(bt - mean * gm * inv);
    if (rmean) {
      const double unb = n > 1 ? m2 / (n - 1.0) : var;
      rmean[ch] = (float)((1.0 - momentum) * rmean[ch] + momentum * mean);
      rvar[ch] = (float)((1.0 - momentum) * rvar[ch] + momentum * unb);
    }
  }
}

__global__ void bn_eval_params_k(const float* gamma, const float* beta, const float* rm,
                                 const float* rv, float eps, int c, float* scale, float* shift) {
  int ch = blockIdx.x * blockDim.x + threadIdx.x;
  if (ch >= c) return;
  float inv = 1.0f / sqrtf(rv[ch] + eps);
  float g = gamma ? gamma[ch] : 1.f;
  float b = beta ? beta[ch] : 0.f;
  scale[ch] = g * inv;
  shift[ch] = b - rm[ch] * g * inv;
}

// 4 values to 4 consecutive elements of an fp32 or bf16 (RNE, the conv loaders' rounding) tensor
__device__ __forceinline__ void st4(float* p, long i4, float4 v) {
  reinterpret_cast<float4*>(p)[i4] = v;
}
__device__ __forceinline__ void st4(__bf16* p, long i4, float4 v) {
  typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
  const bf16x2_t a = {(__bf16)v.x, (__bf16)v.y}, b = {(__bf16)v.z, (__bf16)v.w};
  reinterpret_cast<uint2*>(p)[i4] =
      make_uint2(__builtin_bit_cast(uint32_t, a), __builtin_bit_cast(uint32_t, b));
}

// channel group of element group i in rows of c groups: a mask when c is a power of two (every
// conv channel count of the trunks), else a 64-bit remainder
__device__ __forceinline__ int chan_of(long i, int c) {
  return (c & (c - 1)) == 0 ? (int)(i & (long)(c - 1)) : (int)(i % c);
}

// DUAL: z (fp32) and a bf16 (RNE) copy z16 -- a block output is both the next block's identity
// residual (fp32) and the operand of its bf16-math convs (bf16, read by the LDS-DMA engine)
// 4 consecutive elements of an fp32 or bf16 tensor as float4 (bf16 -> fp32 is exact)
__device__ __forceinline__ float4 ld4(const float* p, long i4) {
  return reinterpret_cast<const float4*>(p)[i4];
}
__device__ __forceinline__ float4 ld4(const __bf16* p, long i4) {
  const uint2 u = reinterpret_cast<const uint2*>(p)[i4];
  return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u),
                     __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u));
}
__device__ __forceinline__ float ld1(const float* p, long i) { return p[i]; }
__device__ __forceinline__ float ld1(const __bf16* p, long i) {
  return __uint_as_float((uint32_t)reinterpret_cast<const unsigned short*>(p)[i] << 16);
}

// TY: element type of y and the residual (bf16 under the bf16-activation contract).  Two elements
// per thread and iteration, both loaded before either is used (as bn_bwd_apply).
template <bool RES, bool RELU, typename TZ = float, bool DUAL = false, typename TY = float>
__global__ __launch_bounds__(NT) void bn_apply_k(const TY* __restrict__ y, const float* __restrict__ scale,
                                                 const float* __restrict__ shift,
                                                 const TY* __restrict__ res, TZ* __restrict__ z,
                                                 long n4, int c4, __bf16* __restrict__ z16 = nullptr) {
  const long stride = (long)gridDim.x * NT;
  auto apply = [&](long i, float4 v, const float4 r) {
    const int cc = chan_of(i, c4) * 4;
    const float4 sc = *reinterpret_cast<const float4*>(scale + cc);
    const float4 sf = *reinterpret_cast<const float4*>(shift + cc);
    v.x = fmaf(v.x, sc.x, sf.x);
    v.y = fmaf(v.y, sc.y, sf.y);
    v.z = fmaf(v.z, sc.z, sf.z);
    v.w = fmaf(v.w, sc.w, sf.w);
    if (RES) {
      v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
    }
    if (RELU) {
      v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
    }
    st4(z, i, v);
    if (DUAL) st4(z16, i, v);
  };
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < n4; i += 2 * stride) {
    const long j = i + stride;
    const bool hj = j < n4;
    const float4 v0 = ld4(y, i);
    const float4 r0 = RES ? ld4(res, i) : v0;
    float4 v1 = v0, r1 = r0;
    if (hj) {
      v1 = ld4(y, j);
      if (RES) r1 = ld4(res, j);
    }
    apply(i, v0, r0);
    if (hj) apply(j, v1, r1);
  }
}

// z = act(y*scale + shift + (yr*rscale + rshift)): the Bottleneck's BN3 + residual + ReLU with the
// downsample branch's BatchNorm applied on the fly (its output is never materialised).  Same
// fmaf/add/max sequence as bn_apply of the branch followed by bn_apply with that residual.
template <bool RELU, bool DUAL = false, typename TY = float, typename TZ = float>
__global__ __launch_bounds__(NT) void bn_apply2_k(const TY* __restrict__ y, const float* __restrict__ scale,
                                                  const float* __restrict__ shift,
                                                  const TY* __restrict__ yr,
                                                  const float* __restrict__ rscale,
                                                  const float* __restrict__ rshift,
                                                  TZ* __restrict__ z, long n4, int c4,
                                                  __bf16* __restrict__ z16) {
  const long stride = (long)gridDim.x * NT;
  auto apply = [&](long i, float4 v, const float4 r) {
    const int cc = chan_of(i, c4) * 4;
    const float4 sc = *reinterpret_cast<const float4*>(scale + cc);
    const float4 sf = *reinterpret_cast<const float4*>(shift + cc);
    const float4 rs = *reinterpret_cast<const float4*>(rscale + cc);
    const float4 rf = *reinterpret_cast<const float4*>(rshift + cc);
    v.x = fmaf(v.x, sc.x, sf.x) + fmaf(r.x, rs.x, rf.x);
    v.y = fmaf(v.y, sc.y, sf.y) + fmaf(r.y, rs.y, rf.y);
    v.z = fmaf(v.z, sc.z, sf.z) + fmaf(r.z, rs.z, rf.z);
    v.w = fmaf(v.w, sc.w, sf.w) + fmaf(r.w, rs.w, rf.w);
    if (RELU) {
      v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
    }
    st4(z, i, v);
    if (DUAL) st4(z16, i, v);
  };
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < n4; i += 2 * stride) {
    const long j = i + stride;
    const bool hj = j < n4;
    const float4 v0 = ld4(y, i), r0 = ld4(yr, i);
    float4 v1 = v0, r1 = r0;
    if (hj) {
      v1 = ld4(y, j);
      r1 = ld4(yr, j);
    }
    apply(i, v0, r0);
    if (hj) apply(j, v1, r1);
  }
}

// The bf16-activation forms of bn_apply_k / bn_apply2_k (bf16 y, residual or branch input, and z),
// 8 elements per thread: every access a 16-B lane piece (the 4-wide forms move bf16 in 8-B
// pieces), two pieces per thread in flight.  Same fmaf / add / max sequence per element:
// identical outputs.  BR: the residual is the downsample branch's pre-BN y (bn_apply2_k).
__device__ __forceinline__ void unpack8(const uint4 w, float (&v)[8]) {
  const uint32_t u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    v[2 * e] = __uint_as_float(u[e] << 16);
    v[2 * e + 1] = __uint_as_float(u[e] & 0xffff0000u);
  }
}
__device__ __forceinline__ uint4 pack8(const float (&v)[8]) {
  typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
  uint32_t o[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const bf16x2_t p = {(__bf16)v[2 * e], (__bf16)v[2 * e + 1]};
    o[e] = __builtin_bit_cast(uint32_t, p);
  }
  return make_uint4(o[0], o[1], o[2], o[3]);
}
template <bool RES, bool RELU, bool BR>
__global__ __launch_bounds__(NT) void bn_apply8_a16_k(const __bf16* __restrict__ y,
                                                      const float* __restrict__ scale,
                                                      const float* __restrict__ shift,
                                                      const __bf16* __restrict__ res,
                                                      const float* __restrict__ rscale,
                                                      const float* __restrict__ rshift,
                                                      __bf16* __restrict__ z, long n8, int c8) {
  const long stride = (long)gridDim.x * NT;
  auto apply = [&](long i, const uint4 yw, const uint4 rw) {
    const int cc = chan_of(i, c8) * 8;
    float v[8], r[8];
    unpack8(yw, v);
    unpack8(rw, r);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float4 sc = *reinterpret_cast<const float4*>(scale + cc + 4 * h);
      const float4 sf = *reinterpret_cast<const float4*>(shift + cc + 4 * h);
      const float a[4] = {sc.x, sc.y, sc.z, sc.w}, b[4] = {sf.x, sf.y, sf.z, sf.w};
      float ra[4] = {0.f, 0.f, 0.f, 0.f}, rb[4] = {0.f, 0.f, 0.f, 0.f};
      if (BR) {
        const float4 rs = *reinterpret_cast<const float4*>(rscale + cc + 4 * h);
        const float4 rf = *reinterpret_cast<const float4*>(rshift + cc + 4 * h);
        ra[0] = rs.x; ra[1] = rs.y; ra[2] = rs.z; ra[3] = rs.w;
        rb[0] = rf.x; rb[1] = rf.y; rb[2] = rf.z; rb[3] = rf.w;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float t;
        if (BR) {
          t = fmaf(v[4 * h + e], a[e], b[e]) + fmaf(r[4 * h + e], ra[e], rb[e]);
        } else {
          t = fmaf(v[4 * h + e], a[e], b[e]);
          if (RES) t += r[4 * h + e];
        }
        if (RELU) t = fmaxf(t, 0.f);
        v[4 * h + e] = t;
      }
    }
    reinterpret_cast<uint4*>(z)[i] = pack8(v);
  };
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < n8; i += 2 * stride) {
    const long j = i + stride;
    const bool hj = j < n8;
    const uint4 y0 = reinterpret_cast<const uint4*>(y)[i];
    const uint4 r0 = (RES || BR) ? reinterpret_cast<const uint4*>(res)[i] : y0;
    uint4 y1 = y0, r1 = r0;
    if (hj) {
      y1 = reinterpret_cast<const uint4*>(y)[j];
      if (RES || BR) r1 = reinterpret_cast<const uint4*>(res)[j];
    }
    apply(i, y0, r0);
    if (hj) apply(j, y1, r1);
  }
}

// The ReLU mask of a block output as bits (tmr_bn_apply_bits / tmr_bn_apply2_bits): element e is
// bit e % 32 of word e / 32.  The fp32 residual-gradient dgrads read it (mask 3) instead of
// re-reading the 4-byte z.  Each lane holds 4 consecutive elements (one float4 index i); the 8
// lanes of a word OR their nibbles.  Wave-uniform loop: the waves' lanes stay converged for the
// shuffles.
// T: element type of y, the residual / branch input and z (bf16 under the bf16-activation contract:
// the bit is taken from the stored, rounded value, so it equals the mask-1 test z > 0 exactly)
__device__ __forceinline__ float stored(float v, const float*) { return v; }
__device__ __forceinline__ float stored(float v, const __bf16*) { return (float)(__bf16)v; }
template <bool RES, typename T = float>
__global__ __launch_bounds__(NT) void bn_apply_bits_k(const T* __restrict__ y,
                                                      const float* __restrict__ scale,
                                                      const float* __restrict__ shift,
                                                      const T* __restrict__ res,
                                                      const T* __restrict__ yr,
                                                      const float* __restrict__ rscale,
                                                      const float* __restrict__ rshift,
                                                      T* __restrict__ z,
                                                      uint32_t* __restrict__ bits, long n4, int c4) {
  const int lane = threadIdx.x & 63;
  const long stride = (long)gridDim.x * NT;
  for (long base = blockIdx.x * (long)NT + (threadIdx.x & ~63); base < n4; base += stride) {
    const long i = base + lane;
    uint32_t nib = 0;
    if (i < n4) {
      const int cc = chan_of(i, c4) * 4;
      float4 v = ld4(y, i);
      const float4 sc = *reinterpret_cast<const float4*>(scale + cc);
      const float4 sf = *reinterpret_cast<const float4*>(shift + cc);
      if (yr) {   // bn_apply2: the downsample branch's BatchNorm on the fly
        const float4 r = ld4(yr, i);
        const float4 rs = *reinterpret_cast<const float4*>(rscale + cc);
        const float4 rf = *reinterpret_cast<const float4*>(rshift + cc);
        v.x = fmaf(v.x, sc.x, sf.x) + fmaf(r.x, rs.x, rf.x);
        v.y = fmaf(v.y, sc.y, sf.y) + fmaf(r.y, rs.y, rf.y);
        v.z = fmaf(v.z, sc.z, sf.z) + fmaf(r.z, rs.z, rf.z);
        v.w = fmaf(v.w, sc.w, sf.w) + fmaf(r.w, rs.w, rf.w);
      } else {
        v.x = fmaf(v.x, sc.x, sf.x); v.y = fmaf(v.y, sc.y, sf.y);
        v.z = fmaf(v.z, sc.z, sf.z); v.w = fmaf(v.w, sc.w, sf.w);
        if (RES) {
          const float4 r = ld4(res, i);
          v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
        }
      }
      v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
      st4(z, i, v);
      const T* tag = nullptr;
      nib = (uint32_t)(stored(v.x, tag) > 0.f) | ((uint32_t)(stored(v.y, tag) > 0.f) << 1) |
            ((uint32_t)(stored(v.z, tag) > 0.f) << 2) | ((uint32_t)(stored(v.w, tag) > 0.f) << 3);
    }
    uint32_t w = nib << (4 * (lane & 7));
    w |= (uint32_t)__shfl_xor((int)w, 1, 64);
    w |= (uint32_t)__shfl_xor((int)w, 2, 64);
    w |= (uint32_t)__shfl_xor((int)w, 4, 64);
    if ((lane & 7) == 0 && i < n4) bits[i >> 3] = w;
  }
}

// ReLU mask of the backward: MASK 0 = none, 1 = saved output z > 0, 2 = recomputed
// fmaf(y, scale, shift) > 0 (bit-identical to the forward's z > 0 when there is no residual,
// and saves reading z)
__device__ __forceinline__ float4 relu_mask4(float4 g, float4 m) {
  g.x = m.x > 0.f ? g.x : 0.f; g.y = m.y > 0.f ? g.y : 0.f;
  g.z = m.z > 0.f ? g.z : 0.f; g.w = m.w > 0.f ? g.w : 0.f;
  return g;
}
__device__ __forceinline__ float4 affine4(float4 v, float4 sc, float4 sf) {
  return make_float4(fmaf(v.x, sc.x, sf.x), fmaf(v.y, sc.y, sf.y), fmaf(v.z, sc.z, sf.z),
                     fmaf(v.w, sc.w, sf.w));
}

// WB: write the masked gradient back over dz (dres aliasing dz: the identity branch of a
// residual block takes the masked gradient in place, and the apply pass needs no mask)
// TG: element type of dz (bf16: the bf16 residual-stream gradient of the bf16-activation step,
// tmr_bn_bwd_g16; no write-back)
template <int MASK, bool WB = false, typename TY = float, typename TG = float>
__global__ __launch_bounds__(NT) void bn_bwd_partial(TG* dz, const TY* __restrict__ y,
                                                     const TY* __restrict__ z,
                                                     const float* __restrict__ scale,
                                                     const float* __restrict__ shift,
                                                     const float* __restrict__ mean, int rows, int c,
                                                     int rpb, int cthreads, double* __restrict__ part) {
  const int tc = threadIdx.x % cthreads, tr = threadIdx.x / cthreads;
  const int rthreads = NT / cthreads;
  const int ch = (blockIdx.y * cthreads + tc) * 4;
  const float4 mu = *reinterpret_cast<const float4*>(mean + ch);
  float4 sc = make_float4(0.f, 0.f, 0.f, 0.f), sf = sc;
  if (MASK == 2) {
    sc = *reinterpret_cast<const float4*>(scale + ch);
    sf = *reinterpret_cast<const float4*>(shift + ch);
  }
  const int r0 = blockIdx.x * rpb;
  const int r1 = min(rows, r0 + rpb);
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f), q = s;
  for (int r = r0 + tr; r < r1; r += rthreads) {
    const long o = (long)r * c + ch;
    float4 g = ld4(dz, o >> 2);
    const float4 v = ld4(y, o >> 2);
    if (MASK == 1) g = relu_mask4(g, ld4(z, o >> 2));
    if (MASK == 2) g = relu_mask4(g, affine4(v, sc, sf));
    if constexpr (WB) {
      static_assert(std::is_same<TG, float>::value, "bn_bwd_partial: write-back of an fp32 dz only");
      *reinterpret_cast<float4*>(dz + o) = g;
    }
    s.x += g.x; s.y += g.y; s.z += g.z; s.w += g.w;
    q.x = fmaf(g.x, v.x - mu.x, q.x); q.y = fmaf(g.y, v.y - mu.y, q.y);
    q.z = fmaf(g.z, v.z - mu.z, q.z); q.w = fmaf(g.w, v.w - mu.w, q.w);
  }
  __shared__ double red[NT][8];
  red[threadIdx.x][0] = s.x; red[threadIdx.x][1] = s.y; red[threadIdx.x][2] = s.z;
  red[threadIdx.x][3] = s.w; red[threadIdx.x][4] = q.x; red[threadIdx.x][5] = q.y;
  red[threadIdx.x][6] = q.z; red[threadIdx.x][7] = q.w;
  __syncthreads();
  if (tr == 0) {
    double acc[8];
    for (int e = 0; e < 8; ++e) acc[e] = 0.0;
    for (int k = 0; k < rthreads; ++k)
      for (int e = 0; e < 8; ++e) acc[e] += red[k * cthreads + tc][e];
    double* o = part + ((long)blockIdx.x * c + ch) * 2;
    for (int e = 0; e < 4; ++e) {
      o[2 * e] = acc[e];
      o[2 * e + 1] = acc[4 + e];
    }
  }
}

__global__ __launch_bounds__(NT) void bn_bwd_final(const double* __restrict__ part, int nrb, int rows, int c,
                                                   const float* mean, const float* inv,
                                                   const float* gamma, float* dgamma,
                                                   float* dbeta, float* coef) {
  const int ch = blockIdx.x;  // one workgroup per channel, fixed-order tree reduction
  double s = 0.0, q = 0.0;
  for (int b = threadIdx.x; b < nrb; b += NT) {
    s += part[((long)b * c + ch) * 2];
    q += part[((long)b * c + ch) * 2 + 1];
  }
  __shared__ double red[2][NT];
  red[0][threadIdx.x] = s;
  red[1][threadIdx.x] = q;
  __syncthreads();
  for (int h = NT / 2; h > 0; h >>= 1) {
    if (threadIdx.x < h) {
      red[0][threadIdx.x] += red[0][threadIdx.x + h];
      red[1][threadIdx.x] += red[1][threadIdx.x + h];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    s = red[0][0];
    q = red[1][0];
    const double iv = inv[ch];
    const double dbt = s;
    const double dgm = q * iv;  // sum dzh * xhat
    if (dgamma) dgamma[ch] = (float)dgm;
    if (dbeta) dbeta[ch] = (float)dbt;
    const double n = (double)rows;
    const double gm = gamma ? gamma[ch] : 1.0;
    const double A = gm * iv;
    const double mdz = dbt / n, mdx = dgm / n;
    const double B = -gm * iv * iv * mdx;
    const double C = -A * mdz - B * (double)mean[ch];
    coef[ch] = (float)A;
    coef[c + ch] = (float)B;
    coef[2 * c + ch] = (float)C;
  }
}

// Two elements per thread and iteration (i and i + the grid's stride), both elements' loads issued
// before either is consumed: one element at a time kept 32 B in flight per thread and ran at
// 5.2 TB/s (`profiles/r3/rocprof_r4g/`, the fp32 step's largest non-conv kernel).
template <int MASK, bool DRES, typename TD = float, typename TY = float>
__global__ __launch_bounds__(NT) void bn_bwd_apply(const float* __restrict__ dz, const TY* __restrict__ y,
                                                   const TY* __restrict__ z,
                                                   const float* __restrict__ scale,
                                                   const float* __restrict__ shift,
                                                   const float* __restrict__ coef, TD* __restrict__ dy,
                                                   float* __restrict__ dres, long n4, int c4) {
  const int c = c4 * 4;
  const long stride = (long)gridDim.x * NT;
  auto apply = [&](long i, float4 g, const float4 v, const float4 zv) {
    const int cc = chan_of(i, c4) * 4;
    if (MASK == 1) g = relu_mask4(g, zv);
    if (MASK == 2)
      g = relu_mask4(g, affine4(v, *reinterpret_cast<const float4*>(scale + cc),
                                *reinterpret_cast<const float4*>(shift + cc)));
    if (DRES) reinterpret_cast<float4*>(dres)[i] = g;
    const float4 A = *reinterpret_cast<const float4*>(coef + cc);
    const float4 B = *reinterpret_cast<const float4*>(coef + c + cc);
    const float4 C = *reinterpret_cast<const float4*>(coef + 2 * c + cc);
    float4 o;
    o.x = fmaf(A.x, g.x, fmaf(B.x, v.x, C.x));
    o.y = fmaf(A.y, g.y, fmaf(B.y, v.y, C.y));
    o.z = fmaf(A.z, g.z, fmaf(B.z, v.z, C.z));
    o.w = fmaf(A.w, g.w, fmaf(B.w, v.w, C.w));
    st4(dy, i, o);
  };
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < n4; i += 2 * stride) {
    const long j = i + stride;
    const bool hj = j < n4;
    const float4 g0 = reinterpret_cast<const float4*>(dz)[i];
    const float4 v0 = ld4(y, i);
    const float4 z0 = MASK == 1 ? ld4(z, i) : g0;
    float4 g1 = g0, v1 = v0, z1 = z0;
    if (hj) {
      g1 = reinterpret_cast<const float4*>(dz)[j];
      v1 = ld4(y, j);
      if (MASK == 1) z1 = ld4(z, j);
    }
    apply(i, g0, v0, z0);
    if (hj) apply(j, g1, v1, z1);
  }
}

// The BatchNorm-backward apply of the bf16-activation step, 8 elements per thread: g (fp32, already
// ReLU-masked by the fused dgrad epilogue) 32 B, y (bf16) 16 B, dy (bf16) 16 B -- every access a
// 16-B lane piece (the 4-wide form moved bf16 in 8-B pieces).  Same fmaf sequence as bn_bwd_apply.
// TG: float, or __bf16 when g was stored bf16 by a TMR_IO_G16 dgrad (16 B of g per thread)
__device__ __forceinline__ void ld_g8(const float* g, long i, float4& a, float4& b) {
  a = reinterpret_cast<const float4*>(g)[2 * i];
  b = reinterpret_cast<const float4*>(g)[2 * i + 1];
}
__device__ __forceinline__ void ld_g8(const __bf16* g, long i, float4& a, float4& b) {
  const uint4 w = reinterpret_cast<const uint4*>(g)[i];
  a = make_float4(__uint_as_float(w.x << 16), __uint_as_float(w.x & 0xffff0000u),
                  __uint_as_float(w.y << 16), __uint_as_float(w.y & 0xffff0000u));
  b = make_float4(__uint_as_float(w.z << 16), __uint_as_float(w.z & 0xffff0000u),
                  __uint_as_float(w.w << 16), __uint_as_float(w.w & 0xffff0000u));
}
template <typename TG = float>
__global__ __launch_bounds__(NT) void bn_bwd_apply8_a16(const TG* __restrict__ g,
                                                        const __bf16* __restrict__ y,
                                                        const float* __restrict__ coef,
                                                        __bf16* __restrict__ dy, long n8, int c8) {
  const int c = c8 * 8;
  const long stride = (long)gridDim.x * NT;
  auto apply = [&](long i, const float4 g0, const float4 g1, const uint4 yw) {
    const int cc = chan_of(i, c8) * 8;
    const float gv[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
    const uint32_t yu[4] = {yw.x, yw.y, yw.z, yw.w};
    float yv[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      yv[2 * e] = __uint_as_float(yu[e] << 16);
      yv[2 * e + 1] = __uint_as_float(yu[e] & 0xffff0000u);
    }
    uint32_t ow[4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float4 A = *reinterpret_cast<const float4*>(coef + cc + 4 * h);
      const float4 B = *reinterpret_cast<const float4*>(coef + c + cc + 4 * h);
      const float4 C = *reinterpret_cast<const float4*>(coef + 2 * c + cc + 4 * h);
      const float o0 = fmaf(A.x, gv[4 * h], fmaf(B.x, yv[4 * h], C.x));
      const float o1 = fmaf(A.y, gv[4 * h + 1], fmaf(B.y, yv[4 * h + 1], C.y));
      const float o2 = fmaf(A.z, gv[4 * h + 2], fmaf(B.z, yv[4 * h + 2], C.z));
      const float o3 = fmaf(A.w, gv[4 * h + 3], fmaf(B.w, yv[4 * h + 3], C.w));
      typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
      const bf16x2_t p = {(__bf16)o0, (__bf16)o1}, q = {(__bf16)o2, (__bf16)o3};
      ow[2 * h] = __builtin_bit_cast(uint32_t, p);
      ow[2 * h + 1] = __builtin_bit_cast(uint32_t, q);
    }
    reinterpret_cast<uint4*>(dy)[i] = make_uint4(ow[0], ow[1], ow[2], ow[3]);
  };
  // two elements in flight per thread (bn_bwd_apply)
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < n8; i += 2 * stride) {
    const long j = i + stride;
    const bool hj = j < n8;
    float4 a0, a1;
    ld_g8(g, i, a0, a1);
    const uint4 ya = reinterpret_cast<const uint4*>(y)[i];
    float4 b0 = a0, b1 = a1;
    uint4 yb = ya;
    if (hj) {
      ld_g8(g, j, b0, b1);
      yb = reinterpret_cast<const uint4*>(y)[j];
    }
    apply(i, a0, a1, ya);
    if (hj) apply(j, b0, b1, yb);
  }
}

// ---- per-channel reductions of the GEMM-epilogue partials, two levels ----------------------
// The conv epilogues leave one partial row per m-tile ([nparts][c]; up to ~31k rows for the
// 64x64-tile dgrads of layer1).  Level 1: a (channel-group x row-slab) grid, 64 channels x 4
// row phases per block, coalesced 1-KB rows, double accumulators -> slab sums in ws.  Level 2:
// one block per channel group, 4 slab phases per channel combined in a fixed order
// (deterministic), then the BN math.
constexpr int SLAB_CH = 64;

struct SlabPlan {
  int groups, nslabs, rows;
};

SlabPlan slab_plan(int nparts, int c) {
  SlabPlan p;
  p.groups = cdiv(c, SLAB_CH);
  int target = 512 / p.groups;
  if (target < 1) target = 1;
  int r = cdiv(nparts, 32);
  if (r > target) r = target;
  if (r < 1) r = 1;
  p.rows = cdiv(nparts, r);
  p.nslabs = cdiv(nparts, p.rows);
  return p;
}

size_t slab_ws_bytes(int nparts, int c) {
  const SlabPlan p = slab_plan(nparts, c);
  return (size_t)p.nslabs * 3 * c * sizeof(double);
}

// KIND 0: float4 (count, mean, M2, -) partials -> (N, S1, S2) about K = the first partial's mean
// KIND 1: float2 (sum g, sum g*(y-mean)) partials -> (S, Q, -)
template <int KIND>
__global__ __launch_bounds__(256) void parts_slab_k(const void* __restrict__ part, int nparts, int c,
                                                    int rows, double* __restrict__ ws) {
  const int ch = blockIdx.x * SLAB_CH + (threadIdx.x & (SLAB_CH - 1));
  const int ph = threadIdx.x / SLAB_CH;
  const int b0 = blockIdx.y * rows;
  const int b1 = min(nparts, b0 + rows);
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  if (ch < c) {
    if (KIND == 0) {
      const float4* p = (const float4*)part;
      const double K = p[ch].y;
      for (int b = b0 + ph; b < b1; b += 4) {
        const float4 v = p[(long)b * c + ch];
        const double nb = v.x, d = (double)v.y - K;
        a0 += nb;
        a1 = fma(nb, d, a1);
        a2 += (double)v.z + nb * d * d;
      }
    } else {
      const float2* p = (const float2*)part;
      for (int b = b0 + ph; b < b1; b += 4) {
        const float2 v = p[(long)b * c + ch];
        a0 += v.x;
        a1 += v.y;
      }
    }
  }
  __shared__ double red[3][256];
  red[0][threadIdx.x] = a0; red[1][threadIdx.x] = a1; red[2][threadIdx.x] = a2;
  __syncthreads();
  if (ph == 0 && ch < c) {
    double t0 = 0.0, t1 = 0.0, t2 = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      t0 += red[0][q * SLAB_CH + threadIdx.x];
      t1 += red[1][q * SLAB_CH + threadIdx.x];
      t2 += red[2][q * SLAB_CH + threadIdx.x];
    }
    double* w = ws + (long)blockIdx.y * 3 * c;
    w[ch] = t0; w[c + ch] = t1; w[2 * c + ch] = t2;
  }
}

// sum of the slab partials of channel group blockIdx.x: SLAB_PH slab phases per channel (a
// 64 x SLAB_PH block), combined in phase order; true on the one thread per channel holding the totals
constexpr int SLAB_PH = 16;
template <int NV>
__device__ __forceinline__ bool slab_sum(const double* __restrict__ ws, int nslabs, int c, int& ch,
                                         double (&t)[3]) {
  ch = blockIdx.x * SLAB_CH + (threadIdx.x & (SLAB_CH - 1));
  const int ph = threadIdx.x / SLAB_CH;
  double a[3] = {0.0, 0.0, 0.0};
  if (ch < c)
    for (int r = ph; r < nslabs; r += SLAB_PH) {
      const double* w = ws + (long)r * 3 * c;
#pragma unroll
      for (int j = 0; j < NV; ++j) a[j] += w[j * c + ch];
    }
  __shared__ double red[3][SLAB_CH * SLAB_PH];
#pragma unroll
  for (int j = 0; j < 3; ++j) red[j][threadIdx.x] = a[j];
  __syncthreads();
  if (ph != 0 || ch >= c) return false;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    t[j] = 0.0;
#pragma unroll
    for (int q = 0; q < SLAB_PH; ++q) t[j] += red[j][q * SLAB_CH + threadIdx.x];
  }
  return true;
}

__global__ __launch_bounds__(SLAB_CH * SLAB_PH) void finalize_slabs_k(const double* __restrict__ ws, int nslabs,
                                                        const float4* __restrict__ part, int c,
                                                        const float* gamma, const float* beta,
                                                        float* rmean, float* rvar, float momentum,
                                                        float eps, float* smean, float* sinv,
                                                        float* scale, float* shift) {
  int ch;
  double t[3];
  if (!slab_sum<3>(ws, nslabs, c, ch, t)) return;
  const double n = t[0], s1 = t[1], s2 = t[2];
  const double K = part[ch].y;
  const double mean = n > 0 ? K + s1 / n : 0.0;
  double m2 = n > 0 ? s2 - s1 * (s1 / n) : 0.0;
  if (m2 < 0) m2 = 0;
  const double var = n > 0 ? m2 / n : 0.0;
  const double inv = 1.0 / sqrt(var + (double)eps);
  smean[ch] = (float)mean;
  sinv[ch] = (float)inv;
  const double gm = gamma ? gamma[ch] : 1.0;
  const double bt = beta ? beta[ch] : 0.0;
  scale[ch] = (float)(gm * inv);
  shift[ch] = (float)(bt - mean * gm * inv);
  if (rmean) {
    const double unb = n > 1 ? m2 / (n - 1.0) : var;
    rmean[ch] = (float)((1.0 - momentum) * rmean[ch] + momentum * mean);
    rvar[ch] = (float)((1.0 - momentum) * rvar[ch] + momentum * unb);
  }
}

__global__ __launch_bounds__(SLAB_CH * SLAB_PH) void bwd_final_slabs_k(const double* __restrict__ ws, int nslabs,
                                                         int rows, int c, const float* mean,
                                                         const float* inv, const float* gamma,
                                                         float* dgamma, float* dbeta, float* coef) {
  int ch;
  double t[3];
  if (!slab_sum<2>(ws, nslabs, c, ch, t)) return;
  const double s = t[0], q = t[1];
  const double iv = inv[ch];
  const double dbt = s;
  const double dgm = q * iv;  // sum dzh * xhat
  if (dgamma) dgamma[ch] = (float)dgm;
  if (dbeta) dbeta[ch] = (float)dbt;
  const double n = (double)rows;
  const double gm = gamma ? gamma[ch] : 1.0;
  const double A = gm * iv;
  const double mdz = dbt / n, mdx = dgm / n;
  const double B = -gm * iv * iv * mdx;
  const double C = -A * mdz - B * (double)mean[ch];
  coef[ch] = (float)A;
  coef[c + ch] = (float)B;
  coef[2 * c + ch] = (float)C;
}

// share.maxpool -> share.relu -> share.bn1 backward in two passes (the stem: pre-BN output y
// (rows = n*h*w pixels), ReLU mask recomputed from y*scale+shift, dz gathered from the pooled
// gradient -- neither dz nor the maxpool's input gradient is ever written)
struct PoolGeo {
  const float* dyp;
  const uchar4* am;
  FastDiv dHW, dW;
  int ho, wo;
};

__device__ __forceinline__ float4 stem_dz(const PoolGeo& pg, uint32_t r, int cq, int c4) {
  const uint32_t nn = fdiv(r, pg.dHW);
  const uint32_t rem = r - nn * pg.dHW.d;
  const uint32_t iy = fdiv(rem, pg.dW);
  const uint32_t ix = rem - iy * pg.dW.d;
  return maxpool_grad4(pg.dyp, pg.am, (int)nn, (int)iy, (int)ix, cq, c4, pg.ho, pg.wo);
}

// Partial sums from the pooled side: every pooled output passes its gradient to exactly one
// input pixel per channel (its argmax), so sum g and sum g*(y - mean) over the input pixels equal
// the sums over pooled outputs of dyp * mask(y[argmax]) and that times (y[argmax] - mean): one
// read of the pooled gradient and argmax plus one y element per channel, no gather of windows.
template <typename TY = float>
__global__ __launch_bounds__(NT) void stem_bwd_partial_pooled(
    const PoolGeo pg, int h, int w, const TY* __restrict__ y, const float* __restrict__ scale,
    const float* __restrict__ shift, const float* __restrict__ mean, int prows, int c, int rpb,
    int cthreads, FastDiv dPHW, FastDiv dPW, double* __restrict__ part) {
  const int tc = threadIdx.x % cthreads, tr = threadIdx.x / cthreads;
  const int rthreads = NT / cthreads;
  const int ch = (blockIdx.y * cthreads + tc) * 4;
  const float mu[4] = {mean[ch], mean[ch + 1], mean[ch + 2], mean[ch + 3]};
  const float sc[4] = {scale[ch], scale[ch + 1], scale[ch + 2], scale[ch + 3]};
  const float sf[4] = {shift[ch], shift[ch + 1], shift[ch + 2], shift[ch + 3]};
  const int c4 = c / 4;
  const int r0 = blockIdx.x * rpb;
  const int r1 = min(prows, r0 + rpb);
  float s[4] = {0.f, 0.f, 0.f, 0.f}, q[4] = {0.f, 0.f, 0.f, 0.f};
  for (int r = r0 + tr; r < r1; r += rthreads) {
    const uint32_t nn = fdiv((uint32_t)r, dPHW);
    const uint32_t rem = r - nn * dPHW.d;
    const uint32_t oy = fdiv(rem, dPW);
    const uint32_t ox = rem - oy * dPW.d;
    const long o = (long)r * c4 + ch / 4;
    const uchar4 a = pg.am[o];
    const float4 d = reinterpret_cast<const float4*>(pg.dyp)[o];
    const unsigned char ids[4] = {a.x, a.y, a.z, a.w};
    const float ds[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int iy = (int)oy * 2 - 1 + ids[e] / 3, ix = (int)ox * 2 - 1 + ids[e] % 3;
      const float v = ld1(y, (((long)nn * h + iy) * w + ix) * c + ch + e);
      const float g = fmaf(v, sc[e], sf[e]) > 0.f ? ds[e] : 0.f;
      s[e] += g;
      q[e] = fmaf(g, v - mu[e], q[e]);
    }
  }
  __shared__ double red[NT][8];
  for (int e = 0; e < 4; ++e) {
    red[threadIdx.x][e] = s[e];
    red[threadIdx.x][4 + e] = q[e];
  }
  __syncthreads();
  if (tr == 0) {
    double acc[8];
    for (int e = 0; e < 8; ++e) acc[e] = 0.0;
    for (int k = 0; k < rthreads; ++k)
      for (int e = 0; e < 8; ++e) acc[e] += red[k * cthreads + tc][e];
    double* op = part + ((long)blockIdx.x * c + ch) * 2;
    for (int e = 0; e < 4; ++e) {
      op[2 * e] = acc[e];
      op[2 * e + 1] = acc[4 + e];
    }
  }
}

template <typename TD, typename TY = float>
__global__ __launch_bounds__(NT) void stem_bwd_apply(const PoolGeo pg, const TY* __restrict__ y,
                                                     const float* __restrict__ scale,
                                                     const float* __restrict__ shift,
                                                     const float* __restrict__ coef,
                                                     TD* __restrict__ dy, long n4, int c4) {
  const int c = c4 * 4;
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < n4; i += (long)gridDim.x * NT) {
    const int cq = chan_of(i, c4);
    const int cc = cq * 4;
    const float4 v = ld4(y, i);
    // (c4 a power of two -- the stem's 64 channels -- divides by a shift, not a 64-bit division)
    const uint32_t row = (c4 & (c4 - 1)) == 0 ? (uint32_t)(i >> __builtin_ctz(c4)) : (uint32_t)(i / c4);
    const float4 g = relu_mask4(stem_dz(pg, row, cq, c4),
                                affine4(v, *reinterpret_cast<const float4*>(scale + cc),
                                        *reinterpret_cast<const float4*>(shift + cc)));
    const float4 A = *reinterpret_cast<const float4*>(coef + cc);
    const float4 B = *reinterpret_cast<const float4*>(coef + c + cc);
    const float4 C = *reinterpret_cast<const float4*>(coef + 2 * c + cc);
    float4 o;
    o.x = fmaf(A.x, g.x, fmaf(B.x, v.x, C.x));
    o.y = fmaf(A.y, g.y, fmaf(B.y, v.y, C.y));
    o.z = fmaf(A.z, g.z, fmaf(B.z, v.z, C.z));
    o.w = fmaf(A.w, g.w, fmaf(B.w, v.w, C.w));
    st4(dy, i, o);
  }
}


// 8 consecutive elements (index i in units of 8) of an fp32 or bf16 tensor, as fp32 values
template <typename T>
__device__ __forceinline__ void ld8(const T* p, long i, float (&v)[8]);
template <>
__device__ __forceinline__ void ld8<float>(const float* p, long i, float (&v)[8]) {
  const float4 a = reinterpret_cast<const float4*>(p)[2 * i], b = reinterpret_cast<const float4*>(p)[2 * i + 1];
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
template <>
__device__ __forceinline__ void ld8<__bf16>(const __bf16* p, long i, float (&v)[8]) {
  const uint4 w = reinterpret_cast<const uint4*>(p)[i];
  const uint32_t u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    v[2 * e] = __uint_as_float(u[e] << 16);
    v[2 * e + 1] = __uint_as_float(u[e] & 0xffff0000u);
  }
}
template <typename T>
__device__ __forceinline__ void st8(T* p, long i, const float (&v)[8]);
template <>
__device__ __forceinline__ void st8<float>(float* p, long i, const float (&v)[8]) {
  reinterpret_cast<float4*>(p)[2 * i] = make_float4(v[0], v[1], v[2], v[3]);
  reinterpret_cast<float4*>(p)[2 * i + 1] = make_float4(v[4], v[5], v[6], v[7]);
}
template <>
__device__ __forceinline__ void st8<__bf16>(__bf16* p, long i, const float (&v)[8]) {
  typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
  uint32_t w[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const bf16x2_t q = {(__bf16)v[2 * e], (__bf16)v[2 * e + 1]};
    w[e] = __builtin_bit_cast(uint32_t, q);
  }
  reinterpret_cast<uint4*>(p)[i] = make_uint4(w[0], w[1], w[2], w[3]);
}
// The BatchNorm-backward apply with g already masked (MASK 0; tmr_bn_bwd_parts), 8 elements per
// thread, two groups in flight: the fp32 step's form of bn_bwd_apply8_a16 (64 B of g and y per
// group instead of 32; round 6).  Same fmaf sequence per element as bn_bwd_apply: identical dy.
template <typename TG, typename TY, typename TD>
__global__ __launch_bounds__(NT) void bn_bwd_apply8_k(const TG* __restrict__ g,
                                                      const TY* __restrict__ y,
                                                      const float* __restrict__ coef,
                                                      TD* __restrict__ dy, long n8, int c8) {
  const int c = c8 * 8;
  const long stride = (long)gridDim.x * NT;
  auto apply = [&](long i, const float (&gv)[8], const float (&yv)[8]) {
    const int cc = chan_of(i, c8) * 8;
    float o[8];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float4 A = *reinterpret_cast<const float4*>(coef + cc + 4 * h);
      const float4 B = *reinterpret_cast<const float4*>(coef + c + cc + 4 * h);
      const float4 C = *reinterpret_cast<const float4*>(coef + 2 * c + cc + 4 * h);
      o[4 * h] = fmaf(A.x, gv[4 * h], fmaf(B.x, yv[4 * h], C.x));
      o[4 * h + 1] = fmaf(A.y, gv[4 * h + 1], fmaf(B.y, yv[4 * h + 1], C.y));
      o[4 * h + 2] = fmaf(A.z, gv[4 * h + 2], fmaf(B.z, yv[4 * h + 2], C.z));
      o[4 * h + 3] = fmaf(A.w, gv[4 * h + 3], fmaf(B.w, yv[4 * h + 3], C.w));
    }
    st8(dy, i, o);
  };
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < n8; i += 2 * stride) {
    const long j = i + stride;
    const bool hj = j < n8;
    float ga[8], ya[8], gb[8], yb[8];
    ld8(g, i, ga);
    ld8(y, i, ya);
    if (hj) {
      ld8(g, j, gb);
      ld8(y, j, yb);
    }
    apply(i, ga, ya);
    if (hj) apply(j, gb, yb);
  }
}

// The same per 2x2 quad of input pixels (rows 2k, 2k+1, columns 2l, 2l+1): the pooled outputs
// (k .. k+1) x (l .. l+1) are the candidates of all four pixels, so each is loaded once per quad
// -- one pooled load per pixel instead of 2.25 (the launch is bound by those gathered bytes).
// Pixel (py, px) of the quad sums candidate (dy, dx) when (dy <= py, dx <= px, in range) with
// id = (py + 1 - 2dy) * 3 + (px + 1 - 2dx), in the order (0,0), (0,1), (1,0), (1,1): the
// per-pixel kernels' order, so bit-identical.  nq = n * ceil(h/2) * ceil(w/2) * c/8 < 2^31.
// TY / TD: y and dy fp32 or bf16 (round 5: the fp32 step's stem too).
template <typename TY, typename TD>
__global__ __launch_bounds__(NT) void stem_bwd_apply8q(const PoolGeo pg, int h, int w, FastDiv dQHW,
                                                       FastDiv dQW, const TY* __restrict__ y,
                                                       const float* __restrict__ scale,
                                                       const float* __restrict__ shift,
                                                       const float* __restrict__ coef,
                                                       TD* __restrict__ dy, int nq, int lc8) {
  const int c8 = 1 << lc8, c = c8 * 8;
  const uint2* am = reinterpret_cast<const uint2*>(pg.am);
  const float4* dp = reinterpret_cast<const float4*>(pg.dyp);
  for (int i = blockIdx.x * NT + threadIdx.x; i < nq; i += gridDim.x * NT) {
    const int cq = i & (c8 - 1);
    const uint32_t q = (uint32_t)i >> lc8;
    const uint32_t nn = fdiv(q, dQHW);
    const uint32_t rem = q - nn * dQHW.d;
    const int k = (int)fdiv(rem, dQW), l = (int)(rem - (uint32_t)k * dQW.d);
    const bool pin[2][2] = {{true, l + 1 < pg.wo}, {k + 1 < pg.ho, k + 1 < pg.ho && l + 1 < pg.wo}};
    uint2 a[2][2];
    float4 d0[2][2], d1[2][2];
#pragma unroll
    for (int ddy = 0; ddy < 2; ++ddy)
#pragma unroll
      for (int ddx = 0; ddx < 2; ++ddx) {
        const int o = (((int)nn * pg.ho + k + ddy) * pg.wo + l + ddx) * c8 + cq;
        if (pin[ddy][ddx]) {
          a[ddy][ddx] = am[o];
          d0[ddy][ddx] = dp[2 * (long)o];       // 64-bit: o < 2^31 is checked, 2 o is not
          d1[ddy][ddx] = dp[2 * (long)o + 1];
        } else {
          a[ddy][ddx] = make_uint2(0xffffffffu, 0xffffffffu);
          d0[ddy][ddx] = d1[ddy][ddx] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
      }
    float sc[8], sf[8], A[8], B[8], C[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      sc[e] = scale[cq * 8 + e];
      sf[e] = shift[cq * 8 + e];
      A[e] = coef[cq * 8 + e];
      B[e] = coef[c + cq * 8 + e];
      C[e] = coef[2 * c + cq * 8 + e];
    }
#pragma unroll
    for (int py = 0; py < 2; ++py)
#pragma unroll
      for (int px = 0; px < 2; ++px) {
        const int iy = 2 * k + py, ix = 2 * l + px;
        if (iy >= h || ix >= w) continue;
        const long pix = ((long)nn * h + iy) * w + ix;
        float v[8], g[8];
        ld8(y, pix * c8 + cq, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) g[e] = 0.f;
#pragma unroll
        for (int ddy = 0; ddy < 2; ++ddy)
#pragma unroll
          for (int ddx = 0; ddx < 2; ++ddx) {
            if (ddy > py || ddx > px || !pin[ddy][ddx]) continue;
            const uint32_t id = (uint32_t)((py + 1 - 2 * ddy) * 3 + (px + 1 - 2 * ddx));
            const float dv[8] = {d0[ddy][ddx].x, d0[ddy][ddx].y, d0[ddy][ddx].z, d0[ddy][ddx].w,
                                 d1[ddy][ddx].x, d1[ddy][ddx].y, d1[ddy][ddx].z, d1[ddy][ddx].w};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const uint32_t ab = ((e < 4 ? a[ddy][ddx].x : a[ddy][ddx].y) >> (8 * (e & 3))) & 0xffu;
              if (ab == id) g[e] += dv[e];
            }
          }
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float gm = fmaf(v[e], sc[e], sf[e]) > 0.f ? g[e] : 0.f;
          o[e] = fmaf(A[e], gm, fmaf(B[e], v[e], C[e]));
        }
        st8(dy, pix * c8 + cq, o);
      }
  }
}

// The forward BN + ReLU with the ReLU mask as bits (bn_apply_bits_k's fp32 forms: RES the residual
// add, yr the downsample branch's BN on the fly), 8 elements per thread and two groups in flight
// per thread, each group's 8 mask bits one byte of its word (round 6: the 4-wide form moved its
// 12 B per element at 4.8 TB/s, the 8-wide BN passes at 5.6-5.9).  Same arithmetic per element:
// z and the bits identical to bn_apply_bits_k's.  The loop runs whole waves (the bit words are
// gathered across 4 lanes).
// DUAL (the fp32-forward / bf16-backward step, tmr_bn_apply_bits_dual): also a bf16 (RNE) copy z16
// of z, one 16-B store per group -- the block output as the next convs' wgrad operand.
template <bool RES, bool DUAL = false>
__global__ __launch_bounds__(NT) void bn_apply_bits8_k(const float* __restrict__ y,
                                                       const float* __restrict__ scale,
                                                       const float* __restrict__ shift,
                                                       const float* __restrict__ res,
                                                       const float* __restrict__ yr,
                                                       const float* __restrict__ rscale,
                                                       const float* __restrict__ rshift,
                                                       float* __restrict__ z,
                                                       uint32_t* __restrict__ bits, long n8, int c8,
                                                       __bf16* __restrict__ z16 = nullptr) {
  const int lane = threadIdx.x & 63;
  const long stride = (long)gridDim.x * NT;
  // one group: z of elements 8i .. 8i + 7 and their mask byte
  auto apply = [&](long i, const float (&yv)[8], const float (&rv)[8]) -> uint32_t {
    const int cc = chan_of(i, c8) * 8;
    float v[8];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float4 sc = *reinterpret_cast<const float4*>(scale + cc + 4 * h);
      const float4 sf = *reinterpret_cast<const float4*>(shift + cc + 4 * h);
      const float s4[4] = {sc.x, sc.y, sc.z, sc.w}, f4[4] = {sf.x, sf.y, sf.z, sf.w};
      if (yr) {
        const float4 rs = *reinterpret_cast<const float4*>(rscale + cc + 4 * h);
        const float4 rf = *reinterpret_cast<const float4*>(rshift + cc + 4 * h);
        const float r4[4] = {rs.x, rs.y, rs.z, rs.w}, q4[4] = {rf.x, rf.y, rf.z, rf.w};
#pragma unroll
        for (int e = 0; e < 4; ++e)
          v[4 * h + e] = fmaf(yv[4 * h + e], s4[e], f4[e]) + fmaf(rv[4 * h + e], r4[e], q4[e]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[4 * h + e] = fmaf(yv[4 * h + e], s4[e], f4[e]);
          if (RES) v[4 * h + e] += rv[4 * h + e];
        }
      }
    }
    uint32_t b = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      v[e] = fmaxf(v[e], 0.f);
      b |= (uint32_t)(v[e] > 0.f) << e;
    }
    st8(z, i, v);
    if (DUAL) st8(z16, i, v);
    return b;
  };
  // the word of 4 lanes' bytes (group indices 4k .. 4k + 3: base is a multiple of 64)
  auto put = [&](uint32_t byte, long i, bool ok) {
    uint32_t w = byte << (8 * (lane & 3));
    w |= (uint32_t)__shfl_xor((int)w, 1, 64);
    w |= (uint32_t)__shfl_xor((int)w, 2, 64);
    if ((lane & 3) == 0 && ok) bits[i >> 2] = w;
  };
  const float* rsrc = RES ? res : yr;
  for (long base = blockIdx.x * (long)NT + (threadIdx.x & ~63); base < n8; base += 2 * stride) {
    const long i = base + lane, j = i + stride;
    const bool oi = i < n8, oj = j < n8;
    float ya[8], ra[8], yb[8], rb[8];
    if (oi) {
      ld8(y, i, ya);
      if (rsrc) ld8(rsrc, i, ra);
    }
    if (oj) {
      ld8(y, j, yb);
      if (rsrc) ld8(rsrc, j, rb);
    }
    const uint32_t bi = oi ? apply(i, ya, ra) : 0u;
    const uint32_t bj = oj ? apply(j, yb, rb) : 0u;
    put(bi, i, oi);
    put(bj, j, oj);
  }
}

// bn_apply_k's DUAL form (z fp32 and its bf16 copy z16), 8 elements per thread and two groups in
// flight: 16-B pieces of y, the residual, z and z16 (the 4-wide form stores z16 in 8-B pieces).
// Same fmaf / add / max sequence per element: identical z and z16.
template <bool RES, bool RELU>
__global__ __launch_bounds__(NT) void bn_apply_dual8_k(const float* __restrict__ y,
                                                       const float* __restrict__ scale,
                                                       const float* __restrict__ shift,
                                                       const float* __restrict__ res,
                                                       float* __restrict__ z,
                                                       __bf16* __restrict__ z16, long n8, int c8) {
  const long stride = (long)gridDim.x * NT;
  auto apply = [&](long i, const float (&yv)[8], const float (&rv)[8]) {
    const int cc = chan_of(i, c8) * 8;
    float v[8];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float4 sc = *reinterpret_cast<const float4*>(scale + cc + 4 * h);
      const float4 sf = *reinterpret_cast<const float4*>(shift + cc + 4 * h);
      const float s4[4] = {sc.x, sc.y, sc.z, sc.w}, f4[4] = {sf.x, sf.y, sf.z, sf.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float t = fmaf(yv[4 * h + e], s4[e], f4[e]);
        if (RES) t += rv[4 * h + e];
        if (RELU) t = fmaxf(t, 0.f);
        v[4 * h + e] = t;
      }
    }
    st8(z, i, v);
    st8(z16, i, v);
  };
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < n8; i += 2 * stride) {
    const long j = i + stride;
    const bool hj = j < n8;
    float ya[8], ra[8], yb[8], rb[8];
    ld8(y, i, ya);
    if (RES) ld8(res, i, ra);
    if (hj) {
      ld8(y, j, yb);
      if (RES) ld8(res, j, rb);
    }
    apply(i, ya, ra);
    if (hj) apply(j, yb, rb);
  }
}

int ew_blocks(long n4) {
  long b = (n4 + NT - 1) / NT;
  if (b > 2048 * 4) b = 2048 * 4;
  return (int)(b > 0 ? b : 1);
}

// ---- host dispatch layer ------------------------------------------------------
// A run-time flag becomes a template argument by reaching a generic lambda as a
// std::integral_constant: with_bool(relu, [&](auto RELU) { ... kernel<RELU> ... }).  Only the tags
// a call site hands on are instantiated, so a site that collapses a combination (write-back only
// where there is a mask) says so in its template argument.  Everything inlines.
template <bool B> using Bool = std::bool_constant<B>;
template <int I> using Int = std::integral_constant<int, I>;

template <typename F>
auto with_bool(bool b, F&& f) {
  return b ? f(Bool<true>{}) : f(Bool<false>{});
}
template <typename F>
auto with_bools(bool a, bool b, F&& f) {
  return with_bool(a, [&](auto A) { return with_bool(b, [&](auto B) { return f(A, B); }); });
}
// v in [0, N)
template <int N, typename F>
auto with_int(int v, F&& f) {
  if constexpr (N == 1) return f(Int<0>{});
  else return v == N - 1 ? f(Int<N - 1>{}) : with_int<N - 1>(v, f);
}
template <int N, typename F>
auto with_int_bool(int v, bool b, F&& f) {
  return with_int<N>(v, [&](auto I) { return with_bool(b, [&](auto B) { return f(I, B); }); });
}

template <typename T> struct arg_of { using type = T; };
// One launch and TMR_CHECK_LAUNCH's test: 0, or 2 with "<name>: launch failed: ..." set.  The
// arguments convert implicitly to the kernel's parameter types (nullptr, an int for a long); a
// kernel's default arguments do not reach a function pointer and are passed.
template <typename... KA>
int launch(const char* name, void (*k)(KA...), dim3 grid, dim3 block, hipStream_t stream,
           typename arg_of<KA>::type... a) {
  hipLaunchKernelGGL(k, grid, block, 0, stream, a...);
  TMR_CHECK_LAUNCH(name);
  return 0;
}

// every pointer 16-B aligned (null counts as aligned)
template <typename... P>
bool aligned16(const P*... p) {
  return ((uintptr_t(0) | ... | (uintptr_t)p) & 15) == 0;
}
// the 8-wide forms' condition: 8 channels per thread in 16-B pieces (else the 4-wide forms)
template <typename... P>
bool wide8(int c, const P*... p) {
  return c % 8 == 0 && aligned16(p...);
}

// the element-wise grid over rows x c in groups of w = 4 or 8 channels
struct Ew {
  long n;   // groups (n4 / n8)
  int nb;   // blocks
  int cw;   // groups per row (c / 4, c / 8)
};
Ew ew_grid(long rows, int c, int w) {
  const long n = rows * c / w;
  return {n, ew_blocks(n), c / w};
}

// ---- shared stages --------------------------------------------------------------------------
// level 1 of the slab reduction of per-block partials into ws (KIND as parts_slab_k)
template <int KIND>
int parts_slabs(const SlabPlan& sp, const void* parts, int nparts, int c, void* ws,
                hipStream_t stream) {
  return launch("bn_parts_slab", parts_slab_k<KIND>, dim3(sp.groups, sp.nslabs), 256, stream,
                parts, nparts, c, sp.rows, (double*)ws);
}

// The BatchNorm backward's reduction from a fused dgrad's partials: dgamma, dbeta and the
// coefficients of dy = A*g + B*y + C, 3 * c floats [A | B | C] in ws at
// tmr_bn_parts_coef_offset(nparts, c).  -> the coefficients, nullptr after a failed launch.
float* parts_coef(const void* parts, int nparts, int rows, int c, const float* mean,
                  const float* inv, const float* gamma, float* dgamma, float* dbeta, void* ws,
                  hipStream_t stream) {
  const SlabPlan sp = slab_plan(nparts, c);
  float* coef = (float*)((char*)ws + slab_ws_bytes(nparts, c));
  if (parts_slabs<1>(sp, parts, nparts, c, ws, stream)) return nullptr;
  if (launch("bn_bwd_final_slabs", bwd_final_slabs_k, sp.groups, SLAB_CH * SLAB_PH, stream,
             (const double*)ws, sp.nslabs, rows, c, mean, inv, gamma, dgamma, dbeta, coef))
    return nullptr;
  return coef;
}

// the workspace of a reduction over rows (ws_need): [nrb][c][2] double partials, then [A | B | C]
struct RowWs {
  Plan p;
  double* part;
  float* coef;
};
RowWs row_ws(int rows, int c, void* ws) {
  const Plan p = make_plan(rows, c);
  return {p, (double*)ws, (float*)((char*)ws + (size_t)p.nrb * c * 2 * sizeof(double))};
}
int bwd_final(const RowWs& r, int rows, int c, const float* mean, const float* inv,
              const float* gamma, float* dgamma, float* dbeta, hipStream_t stream) {
  return launch("bn_bwd_final", bn_bwd_final, c, NT, stream, r.part, r.p.nrb, rows, c, mean, inv,
                gamma, dgamma, dbeta, r.coef);
}

// The BatchNorm backward's reduction over the rows of (g, y): bn_bwd_partial<MASK, WB> (MASK: the
// ReLU mask applied to g on the way, WB: the masked g written back), then bn_bwd_final: dgamma,
// dbeta and [A | B | C] behind the partials in ws.  -> the coefficients, nullptr after a failed
// launch.
template <int MASK, bool WB, typename TG, typename TY>
float* rows_coef(const char* name, TG* g, const TY* y, typename arg_of<const TY*>::type z,
                 const float* scale,
                 const float* shift, const float* mean, const float* inv, const float* gamma,
                 float* dgamma, float* dbeta, int rows, int c, void* ws, hipStream_t stream) {
  const RowWs r = row_ws(rows, c, ws);
  if (launch(name, bn_bwd_partial<MASK, WB, TY, TG>, dim3(r.p.nrb, r.p.cblocks), NT, stream, g, y, z,
             scale, shift, mean, rows, c, r.p.rpb, r.p.cthreads, r.part))
    return nullptr;
  if (bwd_final(r, rows, c, mean, inv, gamma, dgamma, dbeta, stream)) return nullptr;
  return r.coef;
}

// dy = A*g + B*y + C of an fp32 g that needs no mask: 8 channels per thread where wide8 holds
// (bf16 y: bn_bwd_apply8_a16), else bn_bwd_apply<0, false> (the same fmaf sequence)
template <typename TY, typename TD>
int apply_coef(const float* g, const TY* y, const float* coef, TD* dy, int rows, int c,
               hipStream_t stream) {
  if (wide8(c, g, y, dy)) {
    const Ew e = ew_grid(rows, c, 8);
    if constexpr (std::is_same_v<TY, __bf16>)
      return launch("bn_bwd_apply", bn_bwd_apply8_a16<float>, e.nb, NT, stream, g, y, coef, dy,
                    e.n, e.cw);
    else
      return launch("bn_bwd_apply", bn_bwd_apply8_k<float, TY, TD>, e.nb, NT, stream, g, y, coef,
                    dy, e.n, e.cw);
  }
  const Ew e = ew_grid(rows, c, 4);
  return launch("bn_bwd_apply", bn_bwd_apply<0, false, TD, TY>, e.nb, NT, stream, g, y, nullptr,
                nullptr, nullptr, coef, dy, nullptr, e.n, e.cw);
}

PoolGeo pool_geo(const float* dyp, const uint8_t* argmax, int h, int w, int ho, int wo) {
  PoolGeo pg;
  pg.dyp = dyp; pg.am = (const uchar4*)argmax;
  pg.dHW = make_fastdiv((uint32_t)(h * w)); pg.dW = make_fastdiv((uint32_t)w);
  pg.ho = ho; pg.wo = wo;
  return pg;
}

// tmr_bn_bwd(_x) (TY float) and tmr_bn_bwd_a16 (TY, TD __bf16): the row reduction, then the apply
template <typename TY, typename TD>
int bn_bwd_impl(const char* name, const float* dz, const TY* y, const TY* z, const float* scale,
                const float* shift, const float* save_mean, const float* save_invstd,
                const float* gamma, TD* dy, float* dres, float* dgamma, float* dbeta, int rows,
                int c, int relu, void* ws, size_t ws_bytes, hipStream_t stream) {
  TMR_CHECK_ARG(c % 4 == 0 && c >= 4, "%s: channels %d must be a multiple of 4", name, c);
  TMR_CHECK_ARG(rows > 0, "%s: empty input", name);
  TMR_CHECK_ARG(plan_covers(c), "%s: unsupported channel count %d", name, c);
  TMR_CHECK_ARG(ws && ws_bytes >= ws_need(rows, c), "%s: workspace too small", name);
  TMR_CHECK_ARG(!relu || z || (scale && shift),
                "%s: relu backward needs the saved output z or the forward scale/shift", name);
  int mask = relu ? (z ? 1 : 2) : 0;
  // in-place identity-branch gradient (dres == dz): pass 1 masks dz itself -- a write-back only
  // where there is a mask -- and pass 2 reads it unmasked
  const bool inplace = dres == dz;
  const float* coef = with_int_bool<3>(mask, inplace, [&](auto M, auto WB) {
    return rows_coef<M, (M != 0 && WB)>("bn_bwd_partial", const_cast<float*>(dz), y, z, scale,
                                        shift, save_mean, save_invstd, gamma, dgamma, dbeta, rows,
                                        c, ws, stream);
  });
  if (!coef) return 2;
  if (inplace) {
    mask = 0;
    dres = nullptr;
  }
  if constexpr (std::is_same_v<TY, __bf16>) {
    // no mask left to apply (the downsample branch's BN, or a mask already written back): the
    // 8-wide apply of the parts path (same coefficients, same fmaf sequence)
    if (!dres && mask == 0 && wide8(c, dz, y, dy)) return apply_coef(dz, y, coef, dy, rows, c, stream);
  }
  const Ew e = ew_grid(rows, c, 4);
  return with_int_bool<3>(mask, dres != nullptr, [&](auto M, auto DRES) {
    return launch("bn_bwd_apply", bn_bwd_apply<M, DRES, TD, TY>, e.nb, NT, stream, dz, y, z, scale,
                  shift, coef, dy, dres, e.n, e.cw);
  });
}

// tmr_bn_bwd_maxpool(_x) (TY float) and tmr_bn_bwd_maxpool_a16 (TY, TD __bf16)
template <typename TY, typename TD>
int bn_bwd_maxpool_impl(const char* name, const float* dyp, const uint8_t* argmax, int n, int h,
                        int w, int ho, int wo, const TY* y, const float* scale, const float* shift,
                        const float* save_mean, const float* save_invstd, const float* gamma,
                        TD* dy, float* dgamma, float* dbeta, int c, void* ws, size_t ws_bytes,
                        hipStream_t stream) {
  const long rows_l = (long)n * h * w;
  TMR_CHECK_ARG(c % 4 == 0 && c >= 4 && rows_l > 0 && rows_l < 0x7fffffffL,
                "%s: bad shape n=%d h=%d w=%d c=%d", name, n, h, w, c);
  TMR_CHECK_ARG(ho == (h + 2 - 3) / 2 + 1 && wo == (w + 2 - 3) / 2 + 1,
                "%s: pooled %dx%d is not MaxPool2d(3,2,1) of %dx%d", name, ho, wo, h, w);
  const int rows = (int)rows_l;
  TMR_CHECK_ARG(plan_covers(c), "%s: unsupported channel count %d", name, c);
  TMR_CHECK_ARG(ws && ws_bytes >= ws_need(rows, c), "%s: workspace too small", name);
  const PoolGeo pg = pool_geo(dyp, argmax, h, w, ho, wo);
  // partials over the pooled rows (fewer than the input rows: the workspace of `rows` suffices)
  const int prows = n * ho * wo;
  const RowWs r = row_ws(prows, c, ws);
  if (const int rc = launch("stem_bwd_partial_pooled", stem_bwd_partial_pooled<TY>,
                            dim3(r.p.nrb, r.p.cblocks), NT, stream, pg, h, w, y, scale, shift,
                            save_mean, prows, c, r.p.rpb, r.p.cthreads,
                            make_fastdiv((uint32_t)(ho * wo)), make_fastdiv((uint32_t)wo), r.part))
    return rc;
  if (const int rc = bwd_final(r, rows, c, save_mean, save_invstd, gamma, dgamma, dbeta, stream))
    return rc;
  const Ew e = ew_grid(rows_l, c, 4);
  const int c8 = c / 8;
  // 8 channels per thread, per 2x2 input quad (its candidate pooled outputs gathered once; the
  // per-pixel form it replaced was bound by 2.25 gathers per pixel), else one pixel and 4 channels
  if (wide8(c, dyp, y, dy) && (c8 & (c8 - 1)) == 0 && e.n / 2 < 0x7fffffffL &&
      ((uintptr_t)argmax & 7) == 0) {
    const int qh = (h + 1) / 2, qw = (w + 1) / 2;
    const int nq = n * qh * qw * c8;
    return launch("stem_bwd_apply", stem_bwd_apply8q<TY, TD>, ew_blocks(nq), NT, stream, pg, h, w,
                  make_fastdiv((uint32_t)(qh * qw)), make_fastdiv((uint32_t)qw), y, scale, shift,
                  r.coef, dy, nq, __builtin_ctz(c8));
  }
  return launch("stem_bwd_apply", stem_bwd_apply<TD, TY>, e.nb, NT, stream, pg, y, scale, shift,
                r.coef, dy, e.n, e.cw);
}

}  // namespace

TMR_API size_t tmr_bn_ws_bytes(int rows, int c) {
  if (rows <= 0 || c < 4 || c % 4) {
    tmr_set_error("tmr_bn_ws_bytes: bad size (rows %d, channels %d)", rows, c);
    return 0;
  }
  return ws_need(rows, c);
}

TMR_API int tmr_bn_fwd_stats(const float* y, int rows, int c, const float* gamma,
                             const float* beta, float* running_mean, float* running_var,
                             float momentum, float eps, float* save_mean, float* save_invstd,
                             float* scale, float* shift, void* ws, size_t ws_bytes,
                             hipStream_t stream) {
  TMR_CHECK_ARG(c % 4 == 0 && c >= 4, "tmr_bn_fwd_stats: channels %d must be a multiple of 4", c);
  TMR_CHECK_ARG(rows > 0, "tmr_bn_fwd_stats: empty input");
  TMR_CHECK_ARG(plan_covers(c), "tmr_bn_fwd_stats: unsupported channel count %d", c);
  TMR_CHECK_ARG(ws && ws_bytes >= ws_need(rows, c), "tmr_bn_fwd_stats: workspace too small");
  const Plan p = make_plan(rows, c);
  float4* part = (float4*)ws;
  if (const int rc = launch("bn_stats_partial", bn_stats_partial, dim3(p.nrb, p.cblocks), NT,
                            stream, y, rows, c, p.rpb, p.cthreads, part))
    return rc;
  return tmr_bn_finalize(part, p.nrb, c, gamma, beta, running_mean, running_var, momentum, eps,
                         save_mean, save_invstd, scale, shift, stream);
}

TMR_API int tmr_bn_finalize(const void* partials, int nparts, int c, const float* gamma,
                            const float* beta, float* running_mean, float* running_var,
                            float momentum, float eps, float* save_mean, float* save_invstd,
                            float* scale, float* shift, hipStream_t stream) {
  TMR_CHECK_ARG(nparts > 0 && c > 0, "tmr_bn_finalize: empty partials");
  return launch("bn_finalize", bn_finalize_k, c, NT, stream, (const float4*)partials, nparts, c,
                gamma, beta, running_mean, running_var, momentum, eps, save_mean, save_invstd,
                scale, shift);
}

TMR_API size_t tmr_bn_parts_ws_bytes(int nparts, int c) {
  if (nparts <= 0 || c <= 0) {
    tmr_set_error("tmr_bn_parts_ws_bytes: bad size (parts %d, channels %d)", nparts, c);
    return 0;
  }
  return slab_ws_bytes(nparts, c) + (size_t)3 * c * sizeof(float) + 64;
}

TMR_API size_t tmr_bn_parts_coef_offset(int nparts, int c) {
  if (nparts <= 0 || c <= 0) {
    tmr_set_error("tmr_bn_parts_coef_offset: bad size (parts %d, channels %d)", nparts, c);
    return 0;
  }
  return slab_ws_bytes(nparts, c);
}

TMR_API int tmr_bn_finalize_ws(const void* partials, int nparts, int c, const float* gamma,
                               const float* beta, float* running_mean, float* running_var,
                               float momentum, float eps, float* save_mean, float* save_invstd,
                               float* scale, float* shift, void* ws, size_t ws_bytes,
                               hipStream_t stream) {
  TMR_CHECK_ARG(nparts > 0 && c > 0, "tmr_bn_finalize_ws: empty partials");
  TMR_CHECK_ARG(ws && ws_bytes >= slab_ws_bytes(nparts, c), "tmr_bn_finalize_ws: workspace too small");
  const SlabPlan p = slab_plan(nparts, c);
  if (const int rc = parts_slabs<0>(p, partials, nparts, c, ws, stream)) return rc;
  return launch("bn_finalize_slabs", finalize_slabs_k, p.groups, SLAB_CH * SLAB_PH, stream,
                (const double*)ws, p.nslabs, (const float4*)partials, c, gamma, beta, running_mean,
                running_var, momentum, eps, save_mean, save_invstd, scale, shift);
}

TMR_API int tmr_bn_eval_params(const float* gamma, const float* beta, const float* running_mean,
                               const float* running_var, float eps, int c, float* scale,
                               float* shift, hipStream_t stream) {
  return launch("bn_eval_params", bn_eval_params_k, cdiv(c, 256), 256, stream, gamma, beta,
                running_mean, running_var, eps, c, scale, shift);
}

TMR_API int tmr_bn_apply(const float* y, const float* scale, const float* shift,
                         const float* residual, float* z, int rows, int c, int relu,
                         hipStream_t stream) {
  return tmr_bn_apply_x(y, scale, shift, residual, z, rows, c, relu, 0, stream);
}

TMR_API int tmr_bn_apply_x(const float* y, const float* scale, const float* shift,
                           const float* residual, void* zv, int rows, int c, int relu,
                           int out_bf16, hipStream_t stream) {
  TMR_CHECK_ARG(c % 4 == 0, "tmr_bn_apply: channels %d must be a multiple of 4", c);
  TMR_CHECK_ARG(!out_bf16 || !residual,
                "tmr_bn_apply_x: a bf16 output is for conv-operand-only tensors (no residual)");
  const Ew e = ew_grid(rows, c, 4);
  return with_bools(residual, relu, [&](auto RES, auto RELU) {
    if (out_bf16)   // (no residual: RES is false here)
      return launch("bn_apply", bn_apply_k<false, RELU, __bf16>, e.nb, NT, stream, y, scale, shift,
                    residual, (__bf16*)zv, e.n, e.cw, nullptr);
    return launch("bn_apply", bn_apply_k<RES, RELU>, e.nb, NT, stream, y, scale, shift, residual,
                  (float*)zv, e.n, e.cw, nullptr);
  });
}

TMR_API int tmr_bn_apply2(const float* y, const float* scale, const float* shift, const float* yr,
                          const float* rscale, const float* rshift, float* z, int rows, int c,
                          int relu, hipStream_t stream) {
  return tmr_bn_apply2_x(y, scale, shift, yr, rscale, rshift, z, nullptr, rows, c, relu, stream);
}

TMR_API int tmr_bn_apply2_x(const float* y, const float* scale, const float* shift, const float* yr,
                            const float* rscale, const float* rshift, float* z, void* z16,
                            int rows, int c, int relu, hipStream_t stream) {
  TMR_CHECK_ARG(c % 4 == 0, "tmr_bn_apply2: channels %d must be a multiple of 4", c);
  TMR_CHECK_ARG(y && scale && shift && yr && rscale && rshift && z, "tmr_bn_apply2: null operand");
  TMR_CHECK_ARG(yr != z, "tmr_bn_apply2: the branch input must not alias z");
  const Ew e = ew_grid(rows, c, 4);
  return with_bools(relu, z16, [&](auto RELU, auto DUAL) {
    return launch("bn_apply2", bn_apply2_k<RELU, DUAL>, e.nb, NT, stream, y, scale, shift, yr,
                  rscale, rshift, z, e.n, e.cw, (__bf16*)z16);
  });
}

// The forward BN + ReLU with the ReLU mask as bits, fp32: a residual or (yr, rscale, rshift), the
// downsample branch's BN on the fly, or neither.  8-wide where wide8 holds, else 4-wide: the same
// z and bits.
static int bn_apply_bits(const char* name, const float* y, const float* scale, const float* shift,
                         const float* residual, const float* yr, const float* rscale,
                         const float* rshift, float* z, uint32_t* bits, int rows, int c,
                         hipStream_t stream) {
  const bool w8 = wide8(c, y, residual, yr, z);
  const Ew e = ew_grid(rows, c, w8 ? 8 : 4);
  if (e.n == 0) return 0;
  return with_bools(w8, residual, [&](auto W8, auto RES) {
    if constexpr (W8)
      return launch(name, bn_apply_bits8_k<RES>, e.nb, NT, stream, y, scale, shift, residual, yr,
                    rscale, rshift, z, bits, e.n, e.cw, nullptr);
    else
      return launch(name, bn_apply_bits_k<RES, float>, e.nb, NT, stream, y, scale, shift, residual,
                    yr, rscale, rshift, z, bits, e.n, e.cw);
  });
}

TMR_API int tmr_bn_apply_bits(const float* y, const float* scale, const float* shift,
                              const float* residual, float* z, uint32_t* bits, int rows, int c,
                              hipStream_t stream) {
  TMR_CHECK_ARG(c % 4 == 0 && y && scale && shift && z && bits,
                "tmr_bn_apply_bits: null operand or channels %d not a multiple of 4", c);
  return bn_apply_bits("bn_apply_bits", y, scale, shift, residual, nullptr, nullptr, nullptr, z,
                       bits, rows, c, stream);
}

TMR_API int tmr_bn_apply2_bits(const float* y, const float* scale, const float* shift,
                               const float* yr, const float* rscale, const float* rshift, float* z,
                               uint32_t* bits, int rows, int c, hipStream_t stream) {
  TMR_CHECK_ARG(c % 4 == 0 && y && scale && shift && yr && rscale && rshift && z && bits,
                "tmr_bn_apply2_bits: null operand or channels %d not a multiple of 4", c);
  TMR_CHECK_ARG(yr != z, "tmr_bn_apply2_bits: the branch input must not alias z");
  return bn_apply_bits("bn_apply2_bits", y, scale, shift, nullptr, yr, rscale, rshift, z, bits,
                       rows, c, stream);
}

// The block outputs of the fp32-forward / bf16-backward step: tmr_bn_apply_bits / _apply2_bits
// plus the bf16 copy of z in the same pass (the 8-wide kernel only: channel counts and alignments
// it does not serve are refused -- the step's block outputs are all 8-channel multiples).
static int bn_apply_bits_dual(const char* name, const float* y, const float* scale,
                              const float* shift, const float* residual, const float* yr,
                              const float* rscale, const float* rshift, float* z, void* z16,
                              uint32_t* bits, int rows, int c, hipStream_t stream) {
  TMR_CHECK_ARG(rows >= 0, "tmr_%s: negative rows", name);
  TMR_CHECK_ARG(!yr || yr != z, "tmr_%s: the branch input must not alias z", name);
  TMR_CHECK_ARG(c % 8 == 0 && c >= 8, "tmr_%s: channels %d must be a multiple of 8", name, c);
  TMR_CHECK_ARG(aligned16(y, residual, yr, z, z16),
                "tmr_%s: y / residual / z / z16 must be 16-B aligned", name);
  const Ew e = ew_grid(rows, c, 8);
  if (e.n == 0) return 0;
  return with_bool(residual, [&](auto RES) {
    return launch(name, bn_apply_bits8_k<RES, true>, e.nb, NT, stream, y, scale, shift, residual,
                  yr, rscale, rshift, z, bits, e.n, e.cw, (__bf16*)z16);
  });
}

TMR_API int tmr_bn_apply_bits_dual(const float* y, const float* scale, const float* shift,
                                   const float* residual, float* z, void* z16, uint32_t* bits,
                                   int rows, int c, hipStream_t stream) {
  TMR_CHECK_ARG(y && scale && shift && z && z16 && bits, "tmr_bn_apply_bits_dual: null operand");
  return bn_apply_bits_dual("bn_apply_bits_dual", y, scale, shift, residual, nullptr, nullptr,
                            nullptr, z, z16, bits, rows, c, stream);
}

TMR_API int tmr_bn_apply2_bits_dual(const float* y, const float* scale, const float* shift,
                                    const float* yr, const float* rscale, const float* rshift,
                                    float* z, void* z16, uint32_t* bits, int rows, int c,
                                    hipStream_t stream) {
  TMR_CHECK_ARG(y && scale && shift && yr && rscale && rshift && z && z16 && bits,
                "tmr_bn_apply2_bits_dual: null operand");
  return bn_apply_bits_dual("bn_apply2_bits_dual", y, scale, shift, nullptr, yr, rscale, rshift, z,
                            z16, bits, rows, c, stream);
}

// bf16 y, residual / yr and z (4-wide only)
static int bn_apply_bits_a16(const char* name, const void* y, const float* scale,
                             const float* shift, const void* residual, const void* yr,
                             const float* rscale, const float* rshift, void* z, uint32_t* bits,
                             int rows, int c, hipStream_t stream) {
  const Ew e = ew_grid(rows, c, 4);
  if (e.n == 0) return 0;
  return with_bool(residual, [&](auto RES) {
    return launch(name, bn_apply_bits_k<RES, __bf16>, e.nb, NT, stream, (const __bf16*)y, scale,
                  shift, (const __bf16*)residual, (const __bf16*)yr, rscale, rshift, (__bf16*)z,
                  bits, e.n, e.cw);
  });
}

TMR_API int tmr_bn_apply_bits_a16(const void* y, const float* scale, const float* shift,
                                  const void* residual, void* z, uint32_t* bits, int rows, int c,
                                  hipStream_t stream) {
  TMR_CHECK_ARG(c % 4 == 0 && y && scale && shift && z && bits,
                "tmr_bn_apply_bits_a16: null operand or channels %d not a multiple of 4", c);
  return bn_apply_bits_a16("bn_apply_bits_a16", y, scale, shift, residual, nullptr, nullptr,
                           nullptr, z, bits, rows, c, stream);
}

TMR_API int tmr_bn_apply2_bits_a16(const void* y, const float* scale, const float* shift,
                                   const void* yr, const float* rscale, const float* rshift,
                                   void* z, uint32_t* bits, int rows, int c, hipStream_t stream) {
  TMR_CHECK_ARG(c % 4 == 0 && y && scale && shift && yr && rscale && rshift && z && bits,
                "tmr_bn_apply2_bits_a16: null operand or channels %d not a multiple of 4", c);
  TMR_CHECK_ARG(yr != z, "tmr_bn_apply2_bits_a16: the branch input must not alias z");
  return bn_apply_bits_a16("bn_apply2_bits_a16", y, scale, shift, nullptr, yr, rscale, rshift, z,
                           bits, rows, c, stream);
}

TMR_API int tmr_bn_apply_dual(const float* y, const float* scale, const float* shift,
                              const float* residual, float* z, void* z16, int rows, int c, int relu,
                              hipStream_t stream) {
  TMR_CHECK_ARG(c % 4 == 0, "tmr_bn_apply_dual: channels %d must be a multiple of 4", c);
  TMR_CHECK_ARG(y && scale && shift && z && z16, "tmr_bn_apply_dual: null operand");
  __bf16* h = (__bf16*)z16;
  // 8 channels per thread (16-B pieces of z16 too), else the 4-wide form: the same values
  const bool w8 = wide8(c, y, residual, z, z16);
  const Ew e = ew_grid(rows, c, w8 ? 8 : 4);
  return with_bools(residual, relu, [&](auto RES, auto RELU) {
    if (w8)
      return launch("bn_apply_dual", bn_apply_dual8_k<RES, RELU>, e.nb, NT, stream, y, scale,
                    shift, residual, z, h, e.n, e.cw);
    return launch("bn_apply_dual", bn_apply_k<RES, RELU, float, true>, e.nb, NT, stream, y, scale,
                  shift, residual, z, e.n, e.cw, h);
  });
}

TMR_API int tmr_bn_bwd(const float* dz, const float* y, const float* z, const float* scale,
                       const float* shift, const float* save_mean, const float* save_invstd,
                       const float* gamma, float* dy, float* dres, float* dgamma, float* dbeta,
                       int rows, int c, int relu, void* ws, size_t ws_bytes, hipStream_t stream) {
  return tmr_bn_bwd_x(dz, y, z, scale, shift, save_mean, save_invstd, gamma, dy, dres, dgamma,
                      dbeta, rows, c, relu, ws, ws_bytes, 0, stream);
}

TMR_API int tmr_bn_bwd_x(const float* dz, const float* y, const float* z, const float* scale,
                         const float* shift, const float* save_mean, const float* save_invstd,
                         const float* gamma, void* dyv, float* dres, float* dgamma, float* dbeta,
                         int rows, int c, int relu, void* ws, size_t ws_bytes, int out_bf16,
                         hipStream_t stream) {
  if (out_bf16)
    return bn_bwd_impl("tmr_bn_bwd", dz, y, z, scale, shift, save_mean, save_invstd, gamma,
                       (__bf16*)dyv, dres, dgamma, dbeta, rows, c, relu, ws, ws_bytes, stream);
  return bn_bwd_impl("tmr_bn_bwd", dz, y, z, scale, shift, save_mean, save_invstd, gamma,
                     (float*)dyv, dres, dgamma, dbeta, rows, c, relu, ws, ws_bytes, stream);
}

TMR_API int tmr_bn_bwd_maxpool(const float* dyp, const uint8_t* argmax, int n, int h, int w,
                               int ho, int wo, const float* y, const float* scale,
                               const float* shift, const float* save_mean,
                               const float* save_invstd, const float* gamma, float* dy,
                               float* dgamma, float* dbeta, int c, void* ws, size_t ws_bytes,
                               hipStream_t stream) {
  return tmr_bn_bwd_maxpool_x(dyp, argmax, n, h, w, ho, wo, y, scale, shift, save_mean,
                              save_invstd, gamma, dy, dgamma, dbeta, c, ws, ws_bytes, 0, stream);
}

TMR_API int tmr_bn_bwd_maxpool_x(const float* dyp, const uint8_t* argmax, int n, int h, int w,
                                 int ho, int wo, const float* y, const float* scale,
                                 const float* shift, const float* save_mean,
                                 const float* save_invstd, const float* gamma, void* dyv,
                                 float* dgamma, float* dbeta, int c, void* ws, size_t ws_bytes,
                                 int out_bf16, hipStream_t stream) {
  TMR_CHECK_ARG(c >= 4 && plan_covers(c), "tmr_bn_bwd_maxpool: unsupported channel count %d", c);
  TMR_CHECK_ARG(dyv, "tmr_bn_bwd_maxpool: null dy");
  if (out_bf16)
    return bn_bwd_maxpool_impl("tmr_bn_bwd_maxpool", dyp, argmax, n, h, w, ho, wo, y, scale, shift,
                               save_mean, save_invstd, gamma, (__bf16*)dyv, dgamma, dbeta, c, ws,
                               ws_bytes, stream);
  return bn_bwd_maxpool_impl("tmr_bn_bwd_maxpool", dyp, argmax, n, h, w, ho, wo, y, scale, shift,
                             save_mean, save_invstd, gamma, (float*)dyv, dgamma, dbeta, c, ws,
                             ws_bytes, stream);
}

TMR_API int tmr_bn_bwd_parts(const float* g, const float* y, const void* parts, int nparts,
                             const float* save_mean, const float* save_invstd, const float* gamma,
                             float* dy, float* dgamma, float* dbeta, int rows, int c, void* ws,
                             size_t ws_bytes, hipStream_t stream) {
  return tmr_bn_bwd_parts_x(g, y, parts, nparts, save_mean, save_invstd, gamma, dy, dgamma, dbeta,
                            rows, c, ws, ws_bytes, 0, stream);
}

TMR_API int tmr_bn_bwd_parts_x(const float* g, const float* y, const void* parts, int nparts,
                               const float* save_mean, const float* save_invstd,
                               const float* gamma, void* dyv, float* dgamma, float* dbeta,
                               int rows, int c, void* ws, size_t ws_bytes, int out_bf16,
                               hipStream_t stream) {
  TMR_CHECK_ARG(c % 4 == 0 && c >= 4 && rows > 0 && nparts > 0,
                "tmr_bn_bwd_parts: bad shape rows=%d c=%d parts=%d", rows, c, nparts);
  TMR_CHECK_ARG(ws && ws_bytes >= tmr_bn_parts_ws_bytes(nparts, c),
                "tmr_bn_bwd_parts: workspace too small (need tmr_bn_parts_ws_bytes)");
  const float* coef = parts_coef(parts, nparts, rows, c, save_mean, save_invstd, gamma, dgamma,
                                 dbeta, ws, stream);
  if (!coef) return 2;
  // coefficients only (tmr_bn_bwd_maxpool's convention): the caller applies them -- the fused
  // wgrad, tmr_conv2d_wgrad_bnbwd, reads them at ws + tmr_bn_parts_coef_offset(nparts, c)
  if (!dyv) return 0;
  // (a bf16 dy of fp32 g and y -- every non-downsample unit of the fp32-forward / bf16-backward
  // step -- takes the 8-wide form too: the 4-wide one stores dy in 8-B pieces)
  if (out_bf16) return apply_coef(g, y, coef, (__bf16*)dyv, rows, c, stream);
  return apply_coef(g, y, coef, (float*)dyv, rows, c, stream);
}

// ---- bf16-activation forms (TMR_MATH_BF16 train step, include/tmr.h "_a16"): y, z and the
// residual are bf16 tensors (the conv outputs rounded by their epilogue, the BN outputs rounded
// here), the gradients dz / dres stay fp32, dy (a conv operand) is written bf16.  Same arithmetic
// as the fp32 forms on the bf16 values.

TMR_API int tmr_bn_apply_a16(const void* y, const float* scale, const float* shift,
                             const void* residual, void* z, int rows, int c, int relu,
                             hipStream_t stream) {
  TMR_CHECK_ARG(c % 4 == 0 && y && scale && shift && z, "tmr_bn_apply_a16: bad arguments (c %d)", c);
  const __bf16 *yb = (const __bf16*)y, *rb = (const __bf16*)residual;
  __bf16* zb = (__bf16*)z;
  const bool w8 = wide8(c, y, residual, z);   // 8 per thread (bn_apply8_a16_k)
  const Ew e = ew_grid(rows, c, w8 ? 8 : 4);
  return with_bools(residual, relu, [&](auto RES, auto RELU) {
    if (w8)
      return launch("bn_apply_a16", bn_apply8_a16_k<RES, RELU, false>, e.nb, NT, stream, yb, scale,
                    shift, rb, nullptr, nullptr, zb, e.n, e.cw);
    return launch("bn_apply_a16", bn_apply_k<RES, RELU, __bf16, false, __bf16>, e.nb, NT, stream,
                  yb, scale, shift, rb, zb, e.n, e.cw, nullptr);
  });
}

TMR_API int tmr_bn_apply2_a16(const void* y, const float* scale, const float* shift, const void* yr,
                              const float* rscale, const float* rshift, void* z, int rows, int c,
                              int relu, hipStream_t stream) {
  TMR_CHECK_ARG(c % 4 == 0, "tmr_bn_apply2_a16: channels %d must be a multiple of 4", c);
  TMR_CHECK_ARG(y && scale && shift && yr && rscale && rshift && z, "tmr_bn_apply2_a16: null operand");
  TMR_CHECK_ARG(yr != z, "tmr_bn_apply2_a16: the branch input must not alias z");
  const __bf16 *yb = (const __bf16*)y, *rb = (const __bf16*)yr;
  __bf16* zb = (__bf16*)z;
  const bool w8 = wide8(c, y, yr, z);   // 8 per thread (bn_apply8_a16_k)
  const Ew e = ew_grid(rows, c, w8 ? 8 : 4);
  return with_bool(relu, [&](auto RELU) {
    if (w8)
      return launch("bn_apply2_a16", bn_apply8_a16_k<false, RELU, true>, e.nb, NT, stream, yb,
                    scale, shift, rb, rscale, rshift, zb, e.n, e.cw);
    return launch("bn_apply2_a16", bn_apply2_k<RELU, false, __bf16, __bf16>, e.nb, NT, stream, yb,
                  scale, shift, rb, rscale, rshift, zb, e.n, e.cw, nullptr);
  });
}

TMR_API int tmr_bn_bwd_a16(const float* dz, const void* y, const void* z, const float* scale,
                           const float* shift, const float* save_mean, const float* save_invstd,
                           const float* gamma, void* dy, float* dres, float* dgamma, float* dbeta,
                           int rows, int c, int relu, void* ws, size_t ws_bytes,
                           hipStream_t stream) {
  return bn_bwd_impl("tmr_bn_bwd_a16", dz, (const __bf16*)y, (const __bf16*)z, scale, shift,
                     save_mean, save_invstd, gamma, (__bf16*)dy, dres, dgamma, dbeta, rows, c,
                     relu, ws, ws_bytes, stream);
}

// BatchNorm backward of a unit without ReLU (the downsample branch's BN) whose output gradient is
// the bf16 residual-stream gradient of the bf16-activation step (trunk.R16): dz, y, dy bf16
TMR_API int tmr_bn_bwd_g16(const void* dz, const void* y, const float* save_mean,
                           const float* save_invstd, const float* gamma, void* dy, float* dgamma,
                           float* dbeta, int rows, int c, void* ws, size_t ws_bytes,
                           hipStream_t stream) {
  TMR_CHECK_ARG(c % 8 == 0 && c >= 8 && rows > 0, "tmr_bn_bwd_g16: bad shape rows=%d c=%d", rows, c);
  TMR_CHECK_ARG(aligned16(dz, y, dy), "tmr_bn_bwd_g16: dz / y / dy must be 16-B aligned");
  TMR_CHECK_ARG(plan_covers(c), "tmr_bn_bwd_g16: unsupported channel count %d", c);
  TMR_CHECK_ARG(ws && ws_bytes >= ws_need(rows, c), "tmr_bn_bwd_g16: workspace too small");
  const __bf16 *gb = (const __bf16*)dz, *yb = (const __bf16*)y;
  const float* coef = rows_coef<0, false>("bn_bwd_partial_g16", gb, yb, nullptr, nullptr, nullptr,
                                          save_mean, save_invstd, gamma, dgamma, dbeta, rows, c,
                                          ws, stream);
  if (!coef) return 2;
  const Ew e = ew_grid(rows, c, 8);
  return launch("bn_bwd_apply_g16", bn_bwd_apply8_a16<__bf16>, e.nb, NT, stream, gb, yb, coef,
                (__bf16*)dy, e.n, e.cw);
}

TMR_API int tmr_bn_bwd_parts_a16(const float* g, const void* y, const void* parts, int nparts,
                                 const float* save_mean, const float* save_invstd,
                                 const float* gamma, void* dy, float* dgamma, float* dbeta,
                                 int rows, int c, void* ws, size_t ws_bytes, hipStream_t stream) {
  TMR_CHECK_ARG(c % 4 == 0 && c >= 4 && rows > 0 && nparts > 0,
                "tmr_bn_bwd_parts_a16: bad shape rows=%d c=%d parts=%d", rows, c, nparts);
  TMR_CHECK_ARG(ws && ws_bytes >= tmr_bn_parts_ws_bytes(nparts, c),
                "tmr_bn_bwd_parts_a16: workspace too small (need tmr_bn_parts_ws_bytes)");
  const float* coef = parts_coef(parts, nparts, rows, c, save_mean, save_invstd, gamma, dgamma,
                                 dbeta, ws, stream);
  if (!coef) return 2;
  return apply_coef(g, (const __bf16*)y, coef, (__bf16*)dy, rows, c, stream);
}

TMR_API int tmr_bn_bwd_parts_g16(const void* g, const void* y, const void* parts, int nparts,
                                 const float* save_mean, const float* save_invstd,
                                 const float* gamma, void* dy, float* dgamma, float* dbeta,
                                 int rows, int c, void* ws, size_t ws_bytes, hipStream_t stream) {
  TMR_CHECK_ARG(c % 8 == 0 && c >= 8 && rows > 0 && nparts > 0,
                "tmr_bn_bwd_parts_g16: bad shape rows=%d c=%d parts=%d", rows, c, nparts);
  TMR_CHECK_ARG(aligned16(g, y, dy), "tmr_bn_bwd_parts_g16: g / y / dy must be 16-B aligned");
  TMR_CHECK_ARG(ws && ws_bytes >= tmr_bn_parts_ws_bytes(nparts, c),
                "tmr_bn_bwd_parts_g16: workspace too small (need tmr_bn_parts_ws_bytes)");
  const float* coef = parts_coef(parts, nparts, rows, c, save_mean, save_invstd, gamma, dgamma,
                                 dbeta, ws, stream);
  if (!coef) return 2;
  const Ew e = ew_grid(rows, c, 8);
  return launch("bn_bwd_apply_g16", bn_bwd_apply8_a16<__bf16>, e.nb, NT, stream, (const __bf16*)g,
                (const __bf16*)y, coef, (__bf16*)dy, e.n, e.cw);
}

// The BatchNorm backward of a downsample block's two units that share one output gradient g (the
// masked gradient of bn3(y3) + bn_ds(y_ds)): bn3's coefficients from the fused dgrad's partials,
// the downsample BN's from one reduction pass over (g, y_ds), then one apply pass that reads g once
// for both -- dy3 = fmaf(A3, g, fmaf(B3, y3, C3)), dyd = fmaf(Ad, g, fmaf(Bd, yd, Cd)), the fmaf
// sequence of bn_bwd_apply / bn_bwd_apply8_a16 -- instead of two apply passes that each read g.
// T: float (fp32 step: g, y, dy fp32) or __bf16 (bf16-activation step under R16: all bf16, dy
// rounded RNE).  8 elements per thread, 16-B accesses.
// TD: the dy's element type (fp32 g / y / y_ds in, bf16 dy's out: the fp32-forward / bf16-backward
// step, tmr_bn_bwd_parts_ds_d16 -- the RNE of the fp32 form's values).
template <typename T, typename TD = T>
__global__ __launch_bounds__(NT) void bn_bwd_apply_ds8(const T* __restrict__ g, const T* __restrict__ y,
                                                       const T* __restrict__ yd,
                                                       const float* __restrict__ coef,
                                                       const float* __restrict__ coefd,
                                                       TD* __restrict__ dy, TD* __restrict__ dyd, long n8,
                                                       int c8) {
  const int c = c8 * 8;
  auto apply = [&](long i, const float (&gv)[8], const float (&yv)[8], const float (&dv)[8]) {
    const int cc = chan_of(i, c8) * 8;
    float o[8], od[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      o[e] = fmaf(coef[cc + e], gv[e], fmaf(coef[c + cc + e], yv[e], coef[2 * c + cc + e]));
      od[e] = fmaf(coefd[cc + e], gv[e], fmaf(coefd[c + cc + e], dv[e], coefd[2 * c + cc + e]));
    }
    st8(dy, i, o);
    st8(dyd, i, od);
  };
  // two groups in flight per thread (round 6: one group moved its 5 tensors at 4.8 TB/s)
  const long stride = (long)gridDim.x * NT;
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < n8; i += 2 * stride) {
    const long j = i + stride;
    const bool hj = j < n8;
    float ga[8], ya[8], da[8], gb[8], yb[8], db[8];
    ld8(g, i, ga);
    ld8(y, i, ya);
    ld8(yd, i, da);
    if (hj) {
      ld8(g, j, gb);
      ld8(y, j, yb);
      ld8(yd, j, db);
    }
    apply(i, ga, ya, da);
    if (hj) apply(j, gb, yb, db);
  }
}

template <typename T, typename TD>
static int apply_ds(const void* g, const void* y, const void* yd, const float* coef,
                    const float* coefd, void* dy, void* dyd, int rows, int c, hipStream_t stream) {
  const Ew e = ew_grid(rows, c, 8);
  return launch("bn_bwd_apply_ds", bn_bwd_apply_ds8<T, TD>, ew_blocks(e.n / 2), NT, stream,
                (const T*)g, (const T*)y, (const T*)yd, coef, coefd, (TD*)dy, (TD*)dyd, e.n, e.cw);
}

TMR_API size_t tmr_bn_bwd_parts_ds_ws_bytes(int nparts, int rows, int c) {
  if (nparts <= 0 || rows <= 0 || c < 8 || c % 8) {
    tmr_set_error("tmr_bn_bwd_parts_ds_ws_bytes: bad size (parts %d, rows %d, channels %d)", nparts,
                  rows, c);
    return 0;
  }
  return (tmr_bn_parts_ws_bytes(nparts, c) + 255) / 256 * 256 + ws_need(rows, c);
}

// where tmr_bn_bwd_parts_ds leaves its coefficient blocks (3 * c floats [A | B | C] each) in the
// caller's workspace: which 0 = bn3's, 1 = the downsample BN's (tmr_bn_parts_coef_offset's twin)
TMR_API size_t tmr_bn_bwd_parts_ds_coef_offset(int nparts, int rows, int c, int which) {
  if (nparts <= 0 || rows <= 0 || c < 8 || c % 8 || !plan_covers(c) || (which != 0 && which != 1)) {
    tmr_set_error("tmr_bn_bwd_parts_ds_coef_offset: bad size (parts %d, rows %d, channels %d, "
                  "which %d)", nparts, rows, c, which);
    return 0;
  }
  if (which == 0) return slab_ws_bytes(nparts, c);
  const Plan p = make_plan(rows, c);
  return (tmr_bn_parts_ws_bytes(nparts, c) + 255) / 256 * 256 + (size_t)p.nrb * c * 2 * sizeof(double);
}

// out16 (bf16 == 0 only): fp32 operands in, both dy's stored bf16 (tmr_bn_bwd_parts_ds_d16)
static int bn_bwd_parts_ds_impl(const void* g, const void* y, const void* parts, int nparts,
                                const float* mean, const float* invstd, const float* gamma,
                                void* dy, float* dgamma, float* dbeta, const void* yd,
                                const float* mean_d, const float* invstd_d, const float* gamma_d,
                                void* dyd, float* dgamma_d, float* dbeta_d, int rows, int c,
                                int bf16, int out16, void* ws, size_t ws_bytes,
                                hipStream_t stream) {
  TMR_CHECK_ARG(c % 8 == 0 && c >= 8 && rows > 0 && nparts > 0,
                "tmr_bn_bwd_parts_ds: bad shape rows=%d c=%d parts=%d", rows, c, nparts);
  TMR_CHECK_ARG(plan_covers(c), "tmr_bn_bwd_parts_ds: unsupported channel count %d", c);
  // dy / dy_ds may be NULL (fp32 only): that output's apply is the caller's -- the wgrad that
  // produces its dy operand (tmr_conv2d_wgrad_bnbwd) from the coefficient block this call leaves
  // at tmr_bn_bwd_parts_ds_coef_offset.  y is read by bn3's apply alone: NULL with dy.
  TMR_CHECK_ARG(g && parts && yd && (y || !dy) && mean && invstd && gamma && mean_d && invstd_d &&
                    gamma_d, "tmr_bn_bwd_parts_ds: null operand");
  TMR_CHECK_ARG((dy && dyd) || !bf16,
                "tmr_bn_bwd_parts_ds: the coefficient-only and single-output forms are fp32 only");
  TMR_CHECK_ARG(aligned16(g, y, yd, dy, dyd),
                "tmr_bn_bwd_parts_ds: g / y / y_ds / dy / dy_ds must be 16-B aligned");
  const size_t a_bytes = (tmr_bn_parts_ws_bytes(nparts, c) + 255) / 256 * 256;
  TMR_CHECK_ARG(ws && ws_bytes >= a_bytes + ws_need(rows, c),
                "tmr_bn_bwd_parts_ds: workspace too small (need tmr_bn_bwd_parts_ds_ws_bytes)");
  // bn3: the fused dgrad's partials
  const float* coef = parts_coef(parts, nparts, rows, c, mean, invstd, gamma, dgamma, dbeta, ws,
                                 stream);
  if (!coef) return 2;
  // the downsample BN: one reduction pass over (g, y_ds), behind bn3's workspace
  void* wsd = (char*)ws + a_bytes;
  const float* coefd =
      bf16 ? rows_coef<0, false>("bn_bwd_partial", (const __bf16*)g, (const __bf16*)yd, nullptr,
                                 nullptr, nullptr, mean_d, invstd_d, gamma_d, dgamma_d, dbeta_d,
                                 rows, c, wsd, stream)
           : rows_coef<0, false>("bn_bwd_partial", (float*)g, (const float*)yd, nullptr, nullptr,
                                 nullptr, mean_d, invstd_d, gamma_d, dgamma_d, dbeta_d, rows, c,
                                 wsd, stream);
  if (!coefd) return 2;
  if (!dy || !dyd) {
    // one output: the single-output apply on that unit's coefficient block (12 B per element;
    // bn_bwd_apply_ds8's fmaf sequence, so the values of the dual pass); none: coefficients only
    const Ew e = ew_grid(rows, c, 8);
    if (dy)
      return launch("bn_bwd_apply", bn_bwd_apply8_k<float, float, float>, e.nb, NT, stream,
                    (const float*)g, (const float*)y, coef, (float*)dy, e.n, e.cw);
    if (dyd)
      return launch("bn_bwd_apply", bn_bwd_apply8_k<float, float, float>, e.nb, NT, stream,
                    (const float*)g, (const float*)yd, coefd, (float*)dyd, e.n, e.cw);
    return 0;
  }
  if (bf16) return apply_ds<__bf16, __bf16>(g, y, yd, coef, coefd, dy, dyd, rows, c, stream);
  if (out16) return apply_ds<float, __bf16>(g, y, yd, coef, coefd, dy, dyd, rows, c, stream);
  return apply_ds<float, float>(g, y, yd, coef, coefd, dy, dyd, rows, c, stream);
}

TMR_API int tmr_bn_bwd_parts_ds(const void* g, const void* y, const void* parts, int nparts,
                                const float* mean, const float* invstd, const float* gamma,
                                void* dy, float* dgamma, float* dbeta, const void* yd,
                                const float* mean_d, const float* invstd_d, const float* gamma_d,
                                void* dyd, float* dgamma_d, float* dbeta_d, int rows, int c,
                                int bf16, void* ws, size_t ws_bytes, hipStream_t stream) {
  return bn_bwd_parts_ds_impl(g, y, parts, nparts, mean, invstd, gamma, dy, dgamma, dbeta, yd,
                              mean_d, invstd_d, gamma_d, dyd, dgamma_d, dbeta_d, rows, c, bf16, 0,
                              ws, ws_bytes, stream);
}

TMR_API int tmr_bn_bwd_parts_ds_d16(const float* g, const float* y, const void* parts, int nparts,
                                    const float* mean, const float* invstd, const float* gamma,
                                    void* dy, float* dgamma, float* dbeta, const float* yd,
                                    const float* mean_d, const float* invstd_d,
                                    const float* gamma_d, void* dyd, float* dgamma_d,
                                    float* dbeta_d, int rows, int c, void* ws, size_t ws_bytes,
                                    hipStream_t stream) {
  TMR_CHECK_ARG(dy && dyd, "tmr_bn_bwd_parts_ds_d16: null dy / dy_ds (both outputs are written)");
  return bn_bwd_parts_ds_impl(g, y, parts, nparts, mean, invstd, gamma, dy, dgamma, dbeta, yd,
                              mean_d, invstd_d, gamma_d, dyd, dgamma_d, dbeta_d, rows, c, 0, 1, ws,
                              ws_bytes, stream);
}

TMR_API int tmr_bn_bwd_maxpool_a16(const float* dyp, const uint8_t* argmax, int n, int h, int w,
                                   int ho, int wo, const void* y, const float* scale,
                                   const float* shift, const float* save_mean,
                                   const float* save_invstd, const float* gamma, void* dy,
                                   float* dgamma, float* dbeta, int c, void* ws, size_t ws_bytes,
                                   hipStream_t stream) {
  return bn_bwd_maxpool_impl("tmr_bn_bwd_maxpool_a16", dyp, argmax, n, h, w, ho, wo,
                             (const __bf16*)y, scale, shift, save_mean, save_invstd, gamma,
                             (__bf16*)dy, dgamma, dbeta, c, ws, ws_bytes, stream);
}


// ---- frozen BatchNorm: a train-mode step on the running statistics (include/tmr.h
// "tmr_bn_frozen_*") ----------------------------------------------------------------------------
// The forward is the eval-mode BN (y*scale + shift, scale = gamma / sqrt(running_var + eps),
// shift = beta - running_mean*scale) through the existing apply forms.  The backward has no
// projection: with g the ReLU-masked gradient at the BN output, dy = g*scale, dbeta = sum g,
// dgamma = inv * sum g*(y - running_mean) -- one read of g and y where the batch-statistics
// backward reduces and then applies.  These kernels serve the units whose g arrives unmasked (the
// last block's bn3, the stem through the maxpool) or that share g (a downsample block's two BNs);
// the other units take g masked from a fused dgrad, whose partials tmr_bn_frozen_finalize reads.
namespace {

// The coefficients of every BN of a trunk in one launch: one workgroup per table entry,
// bn_eval_params_k's arithmetic per channel (so the frozen step and eval mode apply the same
// scale / shift), plus inv for dgamma.
__global__ __launch_bounds__(NT) void bn_frozen_params_k(const tmr_bn_frozen_entry* __restrict__ tab) {
  const tmr_bn_frozen_entry e = tab[blockIdx.x];
  for (int ch = threadIdx.x; ch < e.c; ch += NT) {
    float inv = 1.0f / sqrtf(e.var[ch] + e.eps);
    float g = e.gamma ? e.gamma[ch] : 1.f;
    float b = e.beta ? e.beta[ch] : 0.f;
    e.scale[ch] = g * inv;
    e.shift[ch] = b - e.mean[ch] * g * inv;
    e.inv[ch] = inv;
  }
}

// A thread keeps 8 channels and walks rows (its sums stay in registers); cthreads threads side by
// side cover 32 B each of a row, the block's other threads take other rows.
struct FPlan {
  int cthreads, rthreads, cblocks, rpb, nrb;
};

// c / 8 channel groups in blocks of cthreads: every c / 8 up to 32 and every multiple of 32 above
bool fplan_covers(int c) {
  const int c8 = c / 8;
  return c % 8 == 0 && c8 > 0 && c8 % (c8 < 32 ? c8 : 32) == 0;
}

FPlan make_fplan(int rows, int c) {
  FPlan p;
  const int c8 = c / 8;
  p.cthreads = c8 < 32 ? c8 : 32;
  p.rthreads = NT / p.cthreads;
  p.cblocks = c8 / p.cthreads;
  // ~4096 workgroups for large inputs, >= 4 rows per thread
  int target = 4096 / p.cblocks;
  if (target < 1) target = 1;
  int rpb = cdiv(rows, target);
  if (rpb < p.rthreads * 4) rpb = p.rthreads * 4;
  rpb = (rpb + p.rthreads - 1) / p.rthreads * p.rthreads;
  p.rpb = rpb;
  p.nrb = cdiv(rows, rpb);
  return p;
}

// MASK 0: g is already masked (or the BN has no ReLU); 1: z > 0 from the saved output z; 2: from
// the forward's own fmaf(y, scale, shift) (no residual); 3: from the ReLU-mask bits of
// tmr_bn_apply_bits (8 elements = one byte).  DUAL: a downsample block's second BN (y_ds, its
// scale and mean) on the same masked g.  Outputs that are NULL are skipped: dres (may alias g: the
// identity branch's gradient in place), dy / dy_ds (the caller folds the scale into its conv
// operands), parts / parts_d (want_sums = 0).  Partials: float2 (sum g, sum g*(y - mean)) per row
// block and channel, the layout of the fused dgrad's (tmr_conv2d_dgrad_bnbwd).
// TD: the type dy / dy_ds are stored in (float, or __bf16: RNE, 8 channels as one 16-B piece);
// g16 (NULL: skipped): the masked g rounded to bf16.  The sums are of the fp32 masked g whatever is
// stored (the tmr_bn_frozen_bwd*_x forms).
template <int MASK, bool DUAL, typename TD>
__global__ __launch_bounds__(NT) void bn_frozen_bwd8_k(
    const float* g, const void* __restrict__ zm, const float* __restrict__ y,
    const float* __restrict__ scale, const float* __restrict__ shift,
    const float* __restrict__ mean, TD* __restrict__ dy, float* dres,
    const float* __restrict__ yd, const float* __restrict__ scale_d,
    const float* __restrict__ mean_d, TD* __restrict__ dyd, __bf16* __restrict__ g16,
    float2* __restrict__ parts, float2* __restrict__ parts_d, int rows, int c, int rpb,
    int cthreads) {
  constexpr int NV = DUAL ? 24 : 16;
  const int rthreads = NT / cthreads;
  const int tc = threadIdx.x % cthreads, tr = threadIdx.x / cthreads;
  const bool live = tr < rthreads;   // NT is no multiple of cthreads = 3 (c = 24): one thread idles
  const int c8 = c >> 3;
  const int cg = blockIdx.y * cthreads + tc;
  const bool sums = parts != nullptr;
  const bool need_y = sums || MASK == 2;
  float sc[8], sf[8], mu[8], sd[8], md[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    sc[e] = scale[cg * 8 + e];
    sf[e] = MASK == 2 ? shift[cg * 8 + e] : 0.f;
    mu[e] = mean[cg * 8 + e];
    sd[e] = DUAL ? scale_d[cg * 8 + e] : 0.f;
    md[e] = DUAL ? mean_d[cg * 8 + e] : 0.f;
  }
  float s[8], q[8], qd[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) s[e] = q[e] = qd[e] = 0.f;
  const int r0 = blockIdx.x * rpb;
  const int r1 = min(rows, r0 + rpb);
  auto step = [&](long i, const float (&gv)[8], const float (&yv)[8], const float (&dv)[8],
                  const float (&zv)[8], uint32_t mb) {
    float gm[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      bool on = true;
      if (MASK == 1) on = zv[e] > 0.f;
      if (MASK == 2) on = fmaf(yv[e], sc[e], sf[e]) > 0.f;
      if (MASK == 3) on = (mb >> e) & 1u;
      gm[e] = on ? gv[e] : 0.f;
    }
    if (dres) st8(dres, i, gm);
    if (g16) st8(g16, i, gm);
    if (dy) {
      float o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = gm[e] * sc[e];
      st8(dy, i, o);
    }
    if (DUAL && dyd) {
      float o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = gm[e] * sd[e];
      st8(dyd, i, o);
    }
    if (sums) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        s[e] += gm[e];
        q[e] = fmaf(gm[e], yv[e] - mu[e], q[e]);
        if (DUAL) qd[e] = fmaf(gm[e], dv[e] - md[e], qd[e]);
      }
    }
  };
  auto load = [&](long i, float (&gv)[8], float (&yv)[8], float (&dv)[8], float (&zv)[8],
                  uint32_t& mb) {
    ld8(g, i, gv);
    if (need_y) ld8(y, i, yv);
    if (DUAL && sums) ld8(yd, i, dv);
    if (MASK == 1) ld8(reinterpret_cast<const float*>(zm), i, zv);
    if (MASK == 3) mb = (reinterpret_cast<const uint32_t*>(zm)[i >> 2] >> (8 * (int)(i & 3))) & 0xffu;
  };
  // two row groups in flight per thread, both loaded before either is used (as bn_bwd_apply8_k)
  if (live) {
    for (int r = r0 + tr; r < r1; r += 2 * rthreads) {
      const int rb = r + rthreads;
      const bool hb = rb < r1;
      const long i = (long)r * c8 + cg, j = (long)rb * c8 + cg;
      float ga[8], ya[8], da[8], za[8], gb[8], yb[8], db[8], zb[8];
      uint32_t ma = 0, mbb = 0;
#pragma unroll
      for (int e = 0; e < 8; ++e) ya[e] = da[e] = za[e] = yb[e] = db[e] = zb[e] = 0.f;
      load(i, ga, ya, da, za, ma);
      if (hb) load(j, gb, yb, db, zb, mbb);
      step(i, ga, ya, da, za, ma);
      if (hb) step(j, gb, yb, db, zb, mbb);
    }
  }
  if (!sums) return;   // (uniform: a kernel argument)
  __shared__ float red[NV][NT];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    red[e][threadIdx.x] = s[e];
    red[8 + e][threadIdx.x] = q[e];
    if (DUAL) red[NV - 8 + e][threadIdx.x] = qd[e];
  }
  __syncthreads();
  if (tr == 0) {
    float a[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) a[v] = 0.f;
    for (int k = 0; k < rthreads; ++k)
#pragma unroll
      for (int v = 0; v < NV; ++v) a[v] += red[v][k * cthreads + tc];
    const long o = (long)blockIdx.x * c + cg * 8;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      parts[o + e] = make_float2(a[e], a[8 + e]);
      if (DUAL) parts_d[o + e] = make_float2(a[e], a[NV - 8 + e]);
    }
  }
}

// The stem: the gradient through MaxPool2d(3,2,1) gathered per 2x2 input quad (stem_bwd_apply8q's
// gather and summation order), masked by the forward's fmaf(y, scale, shift) > 0, dy = g*scale and
// the per-channel partial sums in the same pass.  c / 8 is a power of two that divides NT, so a
// thread's channel group is the same on every grid-stride trip and its sums stay in registers.
// TD: dy's stored type (float, or __bf16 rounded once: tmr_bn_frozen_bwd_maxpool_x).
template <typename TD>
__global__ __launch_bounds__(NT) void bn_frozen_bwd_maxpool8q_k(
    const PoolGeo pg, int h, int w, FastDiv dQHW, FastDiv dQW, const float* __restrict__ y,
    const float* __restrict__ scale, const float* __restrict__ shift,
    const float* __restrict__ mean, TD* __restrict__ dy, float2* __restrict__ parts, int nq,
    int lc8) {
  const int c8 = 1 << lc8, c = c8 * 8;
  const uint2* am = reinterpret_cast<const uint2*>(pg.am);
  const float4* dp = reinterpret_cast<const float4*>(pg.dyp);
  const int cq = threadIdx.x & (c8 - 1);
  const bool sums = parts != nullptr;
  float sc[8], sf[8], mu[8], s[8], q[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    sc[e] = scale[cq * 8 + e];
    sf[e] = shift[cq * 8 + e];
    mu[e] = mean[cq * 8 + e];
    s[e] = q[e] = 0.f;
  }
  for (int i = blockIdx.x * NT + threadIdx.x; i < nq; i += gridDim.x * NT) {
    const uint32_t qi = (uint32_t)i >> lc8;
    const uint32_t nn = fdiv(qi, dQHW);
    const uint32_t rem = qi - nn * dQHW.d;
    const int k = (int)fdiv(rem, dQW), l = (int)(rem - (uint32_t)k * dQW.d);
    const bool pin[2][2] = {{true, l + 1 < pg.wo}, {k + 1 < pg.ho, k + 1 < pg.ho && l + 1 < pg.wo}};
    uint2 a[2][2];
    float4 d0[2][2], d1[2][2];
#pragma unroll
    for (int ddy = 0; ddy < 2; ++ddy)
#pragma unroll
      for (int ddx = 0; ddx < 2; ++ddx) {
        const int o = (((int)nn * pg.ho + k + ddy) * pg.wo + l + ddx) * c8 + cq;
        if (pin[ddy][ddx]) {
          a[ddy][ddx] = am[o];
          d0[ddy][ddx] = dp[2 * (long)o];
          d1[ddy][ddx] = dp[2 * (long)o + 1];
        } else {
          a[ddy][ddx] = make_uint2(0xffffffffu, 0xffffffffu);
          d0[ddy][ddx] = d1[ddy][ddx] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
      }
#pragma unroll
    for (int py = 0; py < 2; ++py)
#pragma unroll
      for (int px = 0; px < 2; ++px) {
        const int iy = 2 * k + py, ix = 2 * l + px;
        if (iy >= h || ix >= w) continue;
        const long pix = ((long)nn * h + iy) * w + ix;
        float v[8], gq[8];
        ld8(y, pix * c8 + cq, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) gq[e] = 0.f;
#pragma unroll
        for (int ddy = 0; ddy < 2; ++ddy)
#pragma unroll
          for (int ddx = 0; ddx < 2; ++ddx) {
            if (ddy > py || ddx > px || !pin[ddy][ddx]) continue;
            const uint32_t id = (uint32_t)((py + 1 - 2 * ddy) * 3 + (px + 1 - 2 * ddx));
            const float dv[8] = {d0[ddy][ddx].x, d0[ddy][ddx].y, d0[ddy][ddx].z, d0[ddy][ddx].w,
                                 d1[ddy][ddx].x, d1[ddy][ddx].y, d1[ddy][ddx].z, d1[ddy][ddx].w};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const uint32_t ab = ((e < 4 ? a[ddy][ddx].x : a[ddy][ddx].y) >> (8 * (e & 3))) & 0xffu;
              if (ab == id) gq[e] += dv[e];
            }
          }
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float gm = fmaf(v[e], sc[e], sf[e]) > 0.f ? gq[e] : 0.f;
          o[e] = gm * sc[e];
          s[e] += gm;
          q[e] = fmaf(gm, v[e] - mu[e], q[e]);
        }
        st8(dy, pix * c8 + cq, o);
      }
  }
  if (!sums) return;   // (uniform: a kernel argument)
  __shared__ float red[16][NT];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    red[e][threadIdx.x] = s[e];
    red[8 + e][threadIdx.x] = q[e];
  }
  __syncthreads();
  if ((int)threadIdx.x < c8) {
    float t[16];
#pragma unroll
    for (int v = 0; v < 16; ++v) t[v] = 0.f;
    for (int k = 0; k < NT / c8; ++k)
#pragma unroll
      for (int v = 0; v < 16; ++v) t[v] += red[v][k * c8 + threadIdx.x];
    const long o = (long)blockIdx.x * c + threadIdx.x * 8;
#pragma unroll
    for (int e = 0; e < 8; ++e) parts[o + e] = make_float2(t[e], t[8 + e]);
  }
}

// level 2 of the partials' reduction (parts_slab_k<1> is level 1): dbeta = sum g,
// dgamma = inv * sum g*(y - mean)
__global__ __launch_bounds__(SLAB_CH * SLAB_PH) void frozen_final_slabs_k(
    const double* __restrict__ ws, int nslabs, int c, const float* __restrict__ inv,
    float* __restrict__ dgamma, float* __restrict__ dbeta) {
  int ch;
  double t[3];
  if (!slab_sum<2>(ws, nslabs, c, ch, t)) return;
  if (dgamma) dgamma[ch] = (float)(t[1] * (double)inv[ch]);
  if (dbeta) dbeta[ch] = (float)t[0];
}

// dW rows scaled per output channel: the wgrad of a unit whose dy = g*scale was folded away ran
// on g, so dW[k] = scale[k] * (x^T g)[k]
__global__ __launch_bounds__(NT) void scale_rows_k(float* __restrict__ w,
                                                   const float* __restrict__ scale, long n,
                                                   int row) {
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < n; i += (long)gridDim.x * NT)
    w[i] *= scale[i / row];
}
__global__ __launch_bounds__(NT) void scale_rows4_k(float4* __restrict__ w,
                                                    const float* __restrict__ scale, long n4,
                                                    int row4) {
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < n4; i += (long)gridDim.x * NT) {
    const float sv = scale[i / row4];
    float4 v = w[i];
    v.x *= sv; v.y *= sv; v.z *= sv; v.w *= sv;
    w[i] = v;
  }
}

// tmr_bn_frozen_bwd(_x) (dual false: yd .. dyd, parts_d NULL) and tmr_bn_frozen_bwd_ds(_x); the
// fp32 entry points are out_bf16 = 0, g16 = NULL
int bn_frozen_bwd_impl(const char* name, bool dual, const float* g, const void* zmask, int mask,
                       const float* y, const float* scale, const float* shift, const float* mean,
                       void* dy, const float* yd, const float* scale_d, const float* mean_d,
                       void* dyd, float* dres, void* g16, void* parts, void* parts_d,
                       size_t parts_bytes, int rows, int c, int want_sums, int out_bf16,
                       hipStream_t stream) {
  TMR_CHECK_ARG(rows > 0 && c >= 8 && c % 8 == 0,
                "%s: bad shape rows=%d c=%d (channels must be a multiple of 8)", name, rows, c);
  TMR_CHECK_ARG(fplan_covers(c), "%s: unsupported channel count %d", name, c);
  TMR_CHECK_ARG(aligned16(g, mask == 1 ? zmask : nullptr, y, yd, dy, dyd),
                "%s: g / z / y / y_ds / dy / dy_ds / dres must be 16-B aligned", name);
  TMR_CHECK_ARG(aligned16(dres), "%s: dres must be 16-B aligned", name);
  TMR_CHECK_ARG(aligned16(g16), "%s: g16 must be 16-B aligned", name);
  TMR_CHECK_ARG(mask >= 0 && mask <= 3, "%s: bad mask %d", name, mask);
  TMR_CHECK_ARG(g && scale && mean, "%s: null operand", name);
  TMR_CHECK_ARG(mask == 0 || mask == 2 || zmask, "%s: mask %d needs z (1) or the mask bits (3)", name, mask);
  TMR_CHECK_ARG(mask != 3 || ((uintptr_t)zmask & 3) == 0, "%s: misaligned mask bits", name);
  TMR_CHECK_ARG(mask != 2 || (y && shift), "%s: mask 2 needs y and shift", name);
  TMR_CHECK_ARG(!dual || (scale_d && mean_d && (!want_sums || yd)), "%s: null downsample operand", name);
  const FPlan p = make_fplan(rows, c);
  float2 *pp = nullptr, *pd = nullptr;
  if (want_sums) {
    TMR_CHECK_ARG(y && parts && (!dual || parts_d), "%s: the sums need y and the partials buffer", name);
    TMR_CHECK_ARG(parts_bytes >= (size_t)p.nrb * c * sizeof(float2),
                  "%s: partials buffer too small (tmr_bn_frozen_bwd_parts rows of c float2)", name);
    pp = (float2*)parts;
    pd = (float2*)parts_d;
  }
  return with_bool(out_bf16 != 0, [&](auto B16) {
    using TD = std::conditional_t<B16.value, __bf16, float>;
    return with_int_bool<4>(mask, dual, [&](auto M, auto DUAL) {
      return launch("bn_frozen_bwd", bn_frozen_bwd8_k<M, DUAL, TD>, dim3(p.nrb, p.cblocks), NT,
                    stream, g, zmask, y, scale, shift, mean, (TD*)dy, dres, yd, scale_d, mean_d,
                    (TD*)dyd, (__bf16*)g16, pp, pd, rows, c, p.rpb, p.cthreads);
    });
  });
}

// tmr_bn_frozen_bwd_maxpool(_x)
int bn_frozen_bwd_maxpool_impl(const char* name, const float* dyp, const uint8_t* argmax, int n,
                               int h, int w, int ho, int wo, const float* y, const float* scale,
                               const float* shift, const float* mean, void* dy, void* parts,
                               size_t parts_bytes, int c, int want_sums, int out_bf16,
                               hipStream_t stream) {
  const long rows_l = (long)n * h * w;
  TMR_CHECK_ARG(n > 0 && h > 0 && w > 0 && c >= 8 && c % 8 == 0 && rows_l < 0x7fffffffL,
                "%s: bad shape n=%d h=%d w=%d c=%d (channels must be a multiple of 8)", name, n, h,
                w, c);
  const int c8 = c / 8;
  TMR_CHECK_ARG((c8 & (c8 - 1)) == 0 && c8 <= NT,
                "%s: unsupported channel count %d (c / 8 must be a power of two up to %d)", name, c,
                NT);
  TMR_CHECK_ARG(ho == (h + 2 - 3) / 2 + 1 && wo == (w + 2 - 3) / 2 + 1,
                "%s: pooled %dx%d is not MaxPool2d(3,2,1) of %dx%d", name, ho, wo, h, w);
  TMR_CHECK_ARG(dyp && argmax && y && scale && shift && mean && dy, "%s: null operand", name);
  TMR_CHECK_ARG(aligned16(dyp, y, dy) && ((uintptr_t)argmax & 7) == 0,
                "%s: dyp / y / dy must be 16-B aligned, argmax 8-B", name);
  const int qh = (h + 1) / 2, qw = (w + 1) / 2;
  const long nq_l = (long)n * qh * qw * c8;
  TMR_CHECK_ARG(nq_l < 0x7fffffffL && (long)n * ho * wo * c8 < 0x7fffffffL, "%s: input too large",
                name);
  const int nq = (int)nq_l, nb = ew_blocks(nq);
  float2* pp = nullptr;
  if (want_sums) {
    TMR_CHECK_ARG(parts && parts_bytes >= (size_t)nb * c * sizeof(float2),
                  "%s: partials buffer too small (tmr_bn_frozen_bwd_maxpool_parts rows of c float2)",
                  name);
    pp = (float2*)parts;
  }
  return with_bool(out_bf16 != 0, [&](auto B16) {
    using TD = std::conditional_t<B16.value, __bf16, float>;
    return launch("bn_frozen_bwd_maxpool", bn_frozen_bwd_maxpool8q_k<TD>, nb, NT, stream,
                  pool_geo(dyp, argmax, h, w, ho, wo), h, w, make_fastdiv((uint32_t)(qh * qw)),
                  make_fastdiv((uint32_t)qw), y, scale, shift, mean, (TD*)dy, pp, nq,
                  __builtin_ctz(c8));
  });
}

}  // namespace

TMR_API int tmr_bn_frozen_params(const tmr_bn_frozen_entry* table_dev, int n, hipStream_t stream) {
  TMR_CHECK_ARG(table_dev && n > 0, "tmr_bn_frozen_params: empty table");
  return launch("bn_frozen_params", bn_frozen_params_k, n, NT, stream, table_dev);
}

TMR_API int tmr_bn_frozen_bwd_parts(int rows, int c) {
  if (rows <= 0 || c < 8 || c % 8 || !fplan_covers(c)) {
    tmr_set_error("tmr_bn_frozen_bwd_parts: bad size (rows %d, channels %d)", rows, c);
    return -1;
  }
  return make_fplan(rows, c).nrb;
}

TMR_API int tmr_bn_frozen_bwd(const float* g, const void* zmask, int mask, const float* y,
                              const float* scale, const float* shift, const float* mean,
                              float* dy, float* dres, void* parts, size_t parts_bytes, int rows,
                              int c, int want_sums, hipStream_t stream) {
  return bn_frozen_bwd_impl("tmr_bn_frozen_bwd", false, g, zmask, mask, y, scale, shift, mean, dy,
                            nullptr, nullptr, nullptr, nullptr, dres, nullptr, parts, nullptr,
                            parts_bytes, rows, c, want_sums, 0, stream);
}

TMR_API int tmr_bn_frozen_bwd_x(const float* g, const void* zmask, int mask, const float* y,
                                const float* scale, const float* shift, const float* mean,
                                void* dy, float* dres, void* g16, void* parts, size_t parts_bytes,
                                int rows, int c, int want_sums, int out_bf16, hipStream_t stream) {
  return bn_frozen_bwd_impl("tmr_bn_frozen_bwd_x", false, g, zmask, mask, y, scale, shift, mean, dy,
                            nullptr, nullptr, nullptr, nullptr, dres, g16, parts, nullptr,
                            parts_bytes, rows, c, want_sums, out_bf16, stream);
}

TMR_API int tmr_bn_frozen_bwd_ds(const float* g, const void* zmask, int mask, const float* y,
                                 const float* scale, const float* shift, const float* mean,
                                 float* dy, const float* yd, const float* scale_d,
                                 const float* mean_d, float* dyd, float* dres, void* parts,
                                 void* parts_d, size_t parts_bytes, int rows, int c, int want_sums,
                                 hipStream_t stream) {
  return bn_frozen_bwd_impl("tmr_bn_frozen_bwd_ds", true, g, zmask, mask, y, scale, shift, mean, dy,
                            yd, scale_d, mean_d, dyd, dres, nullptr, parts, parts_d, parts_bytes,
                            rows, c, want_sums, 0, stream);
}

TMR_API int tmr_bn_frozen_bwd_ds_x(const float* g, const void* zmask, int mask, const float* y,
                                   const float* scale, const float* shift, const float* mean,
                                   void* dy, const float* yd, const float* scale_d,
                                   const float* mean_d, void* dyd, float* dres, void* g16,
                                   void* parts, void* parts_d, size_t parts_bytes, int rows, int c,
                                   int want_sums, int out_bf16, hipStream_t stream) {
  return bn_frozen_bwd_impl("tmr_bn_frozen_bwd_ds_x", true, g, zmask, mask, y, scale, shift, mean,
                            dy, yd, scale_d, mean_d, dyd, dres, g16, parts, parts_d, parts_bytes,
                            rows, c, want_sums, out_bf16, stream);
}

TMR_API int tmr_bn_frozen_bwd_maxpool_parts(int n, int h, int w, int c) {
  const long nq = (long)n * ((h + 1) / 2) * ((w + 1) / 2) * (c / 8);
  if (n <= 0 || h <= 0 || w <= 0 || c < 8 || c % 8 || nq >= 0x7fffffffL) {
    tmr_set_error("tmr_bn_frozen_bwd_maxpool_parts: bad size (n %d, h %d, w %d, channels %d)", n,
                  h, w, c);
    return -1;
  }
  return ew_blocks(nq);
}

TMR_API int tmr_bn_frozen_bwd_maxpool(const float* dyp, const uint8_t* argmax, int n, int h, int w,
                                      int ho, int wo, const float* y, const float* scale,
                                      const float* shift, const float* mean, float* dy,
                                      void* parts, size_t parts_bytes, int c, int want_sums,
                                      hipStream_t stream) {
  return bn_frozen_bwd_maxpool_impl("tmr_bn_frozen_bwd_maxpool", dyp, argmax, n, h, w, ho, wo, y,
                                    scale, shift, mean, dy, parts, parts_bytes, c, want_sums, 0,
                                    stream);
}

TMR_API int tmr_bn_frozen_bwd_maxpool_x(const float* dyp, const uint8_t* argmax, int n, int h,
                                        int w, int ho, int wo, const float* y, const float* scale,
                                        const float* shift, const float* mean, void* dy,
                                        void* parts, size_t parts_bytes, int c, int want_sums,
                                        int out_bf16, hipStream_t stream) {
  return bn_frozen_bwd_maxpool_impl("tmr_bn_frozen_bwd_maxpool_x", dyp, argmax, n, h, w, ho, wo, y,
                                    scale, shift, mean, dy, parts, parts_bytes, c, want_sums,
                                    out_bf16, stream);
}

TMR_API int tmr_bn_frozen_finalize(const void* parts, int nparts, int c, const float* inv,
                                   float* dgamma, float* dbeta, void* ws, size_t ws_bytes,
                                   hipStream_t stream) {
  TMR_CHECK_ARG(parts && inv && nparts > 0 && c > 0,
                "tmr_bn_frozen_finalize: bad arguments (parts %d, channels %d)", nparts, c);
  TMR_CHECK_ARG(ws && ws_bytes >= slab_ws_bytes(nparts, c),
                "tmr_bn_frozen_finalize: workspace too small (need tmr_bn_parts_ws_bytes)");
  const SlabPlan sp = slab_plan(nparts, c);
  if (const int rc = parts_slabs<1>(sp, parts, nparts, c, ws, stream)) return rc;
  return launch("bn_frozen_final_slabs", frozen_final_slabs_k, sp.groups, SLAB_CH * SLAB_PH, stream,
                (const double*)ws, sp.nslabs, c, inv, dgamma, dbeta);
}

TMR_API int tmr_scale_rows(float* w, const float* scale, int k, long row, hipStream_t stream) {
  TMR_CHECK_ARG(w && scale && k > 0 && row > 0 && row < 0x7fffffffL,
                "tmr_scale_rows: bad arguments (k %d, row %ld)", k, row);
  const long n = (long)k * row;
  if (row % 4 == 0 && aligned16(w))
    return launch("scale_rows", scale_rows4_k, ew_blocks(n / 4), NT, stream, (float4*)w, scale,
                  n / 4, (int)(row / 4));
  return launch("scale_rows", scale_rows_k, ew_blocks(n), NT, stream, w, scale, n, (int)row);
}

