// ResNeSt-50 split attention of the bf16-activation inference trunk (resnest.py
// ResNeSt50Share.infer_act16).  The grouped conv's fused unit stores x2 = relu(bn0(conv)) as bf16
// [n][h][w][2C]; between it and conv3 run
//  * tmr_splat_gap_bn (resnest.hip) with an identity scale/shift: the radix-summed GAP, fp32
//  * tmr_splat_attn_inf: fc1 + bias -> eval BatchNorm -> ReLU -> fc2 + bias -> r-softmax, one launch
//  * tmr_splat_combine_a16: the weighted sum of the two radix halves in fp32, in avd blocks the
//    AvgPool2d(3, stride, 1) over it in the same pass, rounded once to bf16.
// A translation unit of its own: the train step's kernels (resnest.hip) keep their code.
#include "common.h"
#include "tmr.h"

namespace {
constexpr int NT = 256;
// frames per workgroup of the attention MLP: each weight row read once serves AF frames
constexpr int AF = 8;

int blocks_for(long n) {
  long b = (n + NT - 1) / NT;
  return (int)(b > 0 ? b : 1);
}

// softmax over the radix pair (splat_att_k's definition, resnest.hip)
__device__ __forceinline__ void rsoft2(float z0, float z1, float& a0, float& a1) {
  const float m = fmaxf(z0, z1);
  const float e0 = expf(z0 - m), e1 = expf(z1 - m);
  const float inv = 1.0f / (e0 + e1);
  a0 = e0 * inv;
  a1 = e1 * inv;
}

// Sum over the LPR lanes of a row group of AF = 8 values per lane: three exchange steps that halve
// the values a lane carries, then plain butterflies.  Returns, in every lane of the group, the sum
// for frame (sub * 8) / LPR (sub = the lane's index in its group): 7 + log2(LPR / 8) shuffles
// instead of 8 * log2(LPR).
template <int LPR>
__device__ __forceinline__ float group_sum8(float (&v)[AF], int sub) {
  static_assert(AF == 8 && LPR >= 8 && LPR <= 64 && (LPR & (LPR - 1)) == 0, "row group shape");
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const int m = LPR >> (s + 1), half = 4 >> s;
    const bool hi = (sub & m) != 0;
#pragma unroll
    for (int k = 0; k < half; ++k) {
      const float send = hi ? v[k] : v[k + half];
      const float keep = hi ? v[k + half] : v[k];
      v[k] = keep + __shfl_xor(send, m, 64);
    }
  }
#pragma unroll
  for (int m = LPR >> 4; m > 0; m >>= 1) v[0] += __shfl_xor(v[0], m, 64);
  return v[0];
}

// acc[f] = sum_k w[k] * in[f][k] over this lane's float4 columns (sub, sub + LPR, ...) of a row of
// k4 float4s; in: LDS [AF][4 * k4]
template <int LPR>
__device__ __forceinline__ void row_dot(const float* __restrict__ wrow, const float* in, int k4, int sub,
                                        float (&acc)[AF]) {
#pragma unroll
  for (int f = 0; f < AF; ++f) acc[f] = 0.f;
  for (int q = sub; q < k4; q += LPR) {
    const float4 wv = reinterpret_cast<const float4*>(wrow)[q];
#pragma unroll
    for (int f = 0; f < AF; ++f) {
      const float4 g = reinterpret_cast<const float4*>(in + (long)f * 4 * k4)[q];
      acc[f] = fmaf(wv.x, g.x, fmaf(wv.y, g.y, fmaf(wv.z, g.z, fmaf(wv.w, g.w, acc[f]))));
    }
  }
}

// att[n][r*C + c] = softmax_r(fc2(relu(bn1(fc1(gap)))))[n][r*C + c].  Workgroup (x, y): frames
// [AF*x, AF*x + AF), channel pairs [y*cper, (y+1)*cper); every workgroup computes the hidden rows
// of its frames itself (LDS), so no workgroup waits for another.  A row of w1 / w2 is read by a
// group of L1 / L2 lanes as float4s and serves all AF frames.
template <int L1, int L2>
__global__ __launch_bounds__(NT) void splat_attn_inf_k(
    const float* __restrict__ gap, const float* __restrict__ w1, const float* __restrict__ b1,
    const float* __restrict__ sc1, const float* __restrict__ sh1, const float* __restrict__ w2,
    const float* __restrict__ b2, float* __restrict__ att, int n, int C, int inter, int cper) {
  extern __shared__ __align__(16) float lds[];   // read and written as float4
  float* sg = lds;             // [AF][C]     the frames' GAP rows (zeros past n)
  float* hs = lds + AF * C;    // [AF][inter] the hidden rows
  const int f0 = blockIdx.x * AF;
  const int tid = threadIdx.x;
  for (int i = tid; i < AF * C / 4; i += NT) {
    const int f = i / (C / 4), q = i - f * (C / 4);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (f0 + f < n) v = reinterpret_cast<const float4*>(gap + (long)(f0 + f) * C)[q];
    reinterpret_cast<float4*>(sg)[i] = v;
  }
  __syncthreads();
  float acc[AF];
  {   // hidden rows: h[f][j] = relu((w1[j] . gap[f] + b1[j]) * sc1[j] + sh1[j])
    const int sub = tid % L1, grp = tid / L1;
    for (int j = grp; j < inter; j += NT / L1) {
      row_dot<L1>(w1 + (long)j * C, sg, C / 4, sub, acc);
      const float t = group_sum8<L1>(acc, sub);
      if (sub % (L1 / 8) == 0) {
        const int f = sub / (L1 / 8);
        hs[f * inter + j] = fmaxf(fmaf(t + b1[j], sc1[j], sh1[j]), 0.f);
      }
    }
  }
  __syncthreads();
  {   // logits of the channel pair (c, C + c) and their softmax
    const int sub = tid % L2, grp = tid / L2;
    const int c_end = min(C, (int)(blockIdx.y + 1) * cper);
    for (int c = blockIdx.y * cper + grp; c < c_end; c += NT / L2) {
      row_dot<L2>(w2 + (long)c * inter, hs, inter / 4, sub, acc);
      const float z0 = group_sum8<L2>(acc, sub) + b2[c];
      row_dot<L2>(w2 + (long)(C + c) * inter, hs, inter / 4, sub, acc);
      const float z1 = group_sum8<L2>(acc, sub) + b2[C + c];
      const int f = f0 + sub / (L2 / 8);
      if (sub % (L2 / 8) == 0 && f < n) {
        float a0, a1;
        rsoft2(z0, z1, a0, a1);
        att[(long)f * 2 * C + c] = a0;
        att[(long)f * 2 * C + C + c] = a1;
      }
    }
  }
}

__device__ __forceinline__ float bf_lo(uint32_t w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf_hi(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }

// out[n,ho,wo,c] = rnd(pool(att0 * x2[.., c] + att1 * x2[.., C + c])), 8 channels per lane (16-B
// loads, splat_combine_bn8_k's layout).  POOL: AvgPool2d(3, stride, 1, count_include_pad=True);
// the attention weights are constant over a frame, so the window sums of the two halves are taken
// first (fp32 sums of bf16 values) and weighted once: (att0 * S0 + att1 * S1) / 9.
template <bool POOL>
__global__ __launch_bounds__(NT) void splat_combine_a16_k(const __bf16* __restrict__ x2,
                                                          const float* __restrict__ att,
                                                          __bf16* __restrict__ out, uint32_t total,
                                                          int C, int h, int w, FastDiv dc8, FastDiv dwo,
                                                          FastDiv dho, int stride) {
  const uint32_t i = blockIdx.x * NT + threadIdx.x;
  if (i >= total) return;
  const uint32_t p = fdiv(i, dc8);            // output pixel
  const int q = (int)(i - p * dc8.d);         // channel octet
  const uint32_t row = fdiv(p, dwo);
  const int ox = (int)(p - row * dwo.d);
  const uint32_t nn = fdiv(row, dho);
  const int oy = (int)(row - nn * dho.d);
  float s0[8], s1[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) s0[e] = s1[e] = 0.f;
  auto add = [&](int y, int x) {
    const __bf16* px = x2 + (((long)nn * h + y) * w + x) * 2 * C + 8 * q;
    const uint4 w0 = *reinterpret_cast<const uint4*>(px);
    const uint4 w1 = *reinterpret_cast<const uint4*>(px + C);
    const uint32_t u0[4] = {w0.x, w0.y, w0.z, w0.w}, u1[4] = {w1.x, w1.y, w1.z, w1.w};
#pragma unroll
    for (int e2 = 0; e2 < 4; ++e2) {
      s0[2 * e2] += bf_lo(u0[e2]);
      s0[2 * e2 + 1] += bf_hi(u0[e2]);
      s1[2 * e2] += bf_lo(u1[e2]);
      s1[2 * e2 + 1] += bf_hi(u1[e2]);
    }
  };
  if (POOL) {
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        const int y = oy * stride + dy, x = ox * stride + dx;
        if (y >= 0 && y < h && x >= 0 && x < w) add(y, x);
      }
  } else {
    add(oy, ox);
  }
  const float* a = att + (long)nn * 2 * C + 8 * q;
  const float4 a00 = reinterpret_cast<const float4*>(a)[0], a01 = reinterpret_cast<const float4*>(a)[1];
  const float4 a10 = reinterpret_cast<const float4*>(a + C)[0], a11 = reinterpret_cast<const float4*>(a + C)[1];
  const float a0[8] = {a00.x, a00.y, a00.z, a00.w, a01.x, a01.y, a01.z, a01.w};
  const float a1[8] = {a10.x, a10.y, a10.z, a10.w, a11.x, a11.y, a11.z, a11.w};
  uint32_t o[4];
#pragma unroll
  for (int e2 = 0; e2 < 4; ++e2) {
    float v[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int e = 2 * e2 + b;
      v[b] = fmaf(a1[e], s1[e], a0[e] * s0[e]);
      if (POOL) v[b] = v[b] / 9.0f;
    }
    typedef __bf16 b2 __attribute__((ext_vector_type(2)));
    const b2 pr = {(__bf16)v[0], (__bf16)v[1]};
    o[e2] = __builtin_bit_cast(uint32_t, pr);
  }
  *reinterpret_cast<uint4*>(out + (long)p * C + 8 * q) = make_uint4(o[0], o[1], o[2], o[3]);
}

template <int L1, int L2>
void launch_attn(dim3 grid, size_t lds, hipStream_t stream, const float* gap, const float* w1,
                 const float* b1, const float* sc1, const float* sh1, const float* w2, const float* b2,
                 float* att, int n, int C, int inter, int cper) {
  hipLaunchKernelGGL((splat_attn_inf_k<L1, L2>), grid, dim3(NT), lds, stream, gap, w1, b1, sc1, sh1, w2,
                     b2, att, n, C, inter, cper);
}
}  // namespace

TMR_API int tmr_splat_attn_inf(const float* gap, const float* w1, const float* b1, const float* scale1,
                               const float* shift1, const float* w2, const float* b2, float* att,
                               int n, int c, int inter, hipStream_t stream) {
  TMR_CHECK_ARG(n > 0 && (c == 64 || c == 128 || c == 256 || c == 512) && inter == c / 2,
                "tmr_splat_attn_inf: bad shape n %d c %d inter %d (c 64 / 128 / 256 / 512, inter = c/2)",
                n, c, inter);
  TMR_CHECK_ARG(gap && w1 && b1 && scale1 && shift1 && w2 && b2 && att, "tmr_splat_attn_inf: null operand");
  TMR_CHECK_ARG(((((uintptr_t)gap) | ((uintptr_t)w1) | ((uintptr_t)w2)) & 15) == 0,
                "tmr_splat_attn_inf: gap, w1 and w2 must be 16-B aligned");
  // fewer frame groups than CUs (256): split the channel pairs over up to 8 workgroups per frame
  // group (each computes the hidden rows again: a third of the weight bytes, from L2), every row
  // group (c/8 lanes) keeping a pair.  640 frames: 80 frame groups x 4.
  const int fgroups = (n + AF - 1) / AF;
  int split = 1;
  while (split < 8 && fgroups * split < 256 && (c / (split * 2)) * (c / 8) >= NT) split *= 2;
  const dim3 grid(fgroups, split);
  const size_t lds = (size_t)AF * (c + inter) * sizeof(float);
  const int cper = c / split;
  switch (c) {
    case 64:  launch_attn<16, 8>(grid, lds, stream, gap, w1, b1, scale1, shift1, w2, b2, att, n, c, inter, cper); break;
    case 128: launch_attn<32, 16>(grid, lds, stream, gap, w1, b1, scale1, shift1, w2, b2, att, n, c, inter, cper); break;
    case 256: launch_attn<64, 32>(grid, lds, stream, gap, w1, b1, scale1, shift1, w2, b2, att, n, c, inter, cper); break;
    default:  launch_attn<64, 64>(grid, lds, stream, gap, w1, b1, scale1, shift1, w2, b2, att, n, c, inter, cper); break;
  }
  TMR_CHECK_LAUNCH("splat_attn_inf");
  return 0;
}

TMR_API int tmr_splat_combine_a16(const void* x2, const float* att, void* out, int n, int h, int w,
                                  int c, int pool_stride, hipStream_t stream) {
  TMR_CHECK_ARG(n > 0 && h > 0 && w > 0 && c > 0 && c % 8 == 0,
                "tmr_splat_combine_a16: bad shape n %d h %d w %d c %d (channels a multiple of 8)", n, h, w, c);
  TMR_CHECK_ARG(pool_stride >= 0 && pool_stride <= 2,
                "tmr_splat_combine_a16: pool stride %d (0 = no pool, 1 or 2)", pool_stride);
  TMR_CHECK_ARG(x2 && att && out, "tmr_splat_combine_a16: null operand");
  TMR_CHECK_ARG(((((uintptr_t)x2) | ((uintptr_t)att) | ((uintptr_t)out)) & 15) == 0,
                "tmr_splat_combine_a16: x2, att and out must be 16-B aligned");
  const int ho = pool_stride ? (h - 1) / pool_stride + 1 : h;   // (h + 2 - 3) / s + 1
  const int wo = pool_stride ? (w - 1) / pool_stride + 1 : w;
  const long total = (long)n * ho * wo * (c / 8);
  TMR_CHECK_ARG(total < (1L << 31) - NT, "tmr_splat_combine_a16: %ld channel octets exceed 2^31", total);
  const FastDiv dc8 = make_fastdiv((uint32_t)(c / 8)), dwo = make_fastdiv((uint32_t)wo),
                dho = make_fastdiv((uint32_t)ho);
  if (pool_stride)
    hipLaunchKernelGGL(splat_combine_a16_k<true>, dim3(blocks_for(total)), dim3(NT), 0, stream,
                       (const __bf16*)x2, att, (__bf16*)out, (uint32_t)total, c, h, w, dc8, dwo, dho,
                       pool_stride);
  else
    hipLaunchKernelGGL(splat_combine_a16_k<false>, dim3(blocks_for(total)), dim3(NT), 0, stream,
                       (const __bf16*)x2, att, (__bf16*)out, (uint32_t)total, c, h, w, dc8, dwo, dho, 1);
  TMR_CHECK_LAUNCH("splat_combine_a16");
  return 0;
}
