// nn.LSTM(2048, 512, batch_first=True) forward and backward as C entry points
// (code/Training TMRNet/train_only_non-local_pretrained.py:215, :230-233; gate order i, f, g, o).
//
//   forward : gx = x W_ih^T + (b_ih + b_hh) for all b*t frames (one MFMA GEMM), then the t-step
//             recurrence in ONE persistent launch: every step computes the gate GEMM
//             h_{t-1} W_hh^T, sigma/tanh and the cell update without leaving the kernel.
//   backward: BPTT in one persistent launch (dh = dy_t + dg_{t+1} W_hh, gate backward, dc), then
//             one GEMM each for dW_ih, dW_hh, dx and a column sum for the biases.
//   window  : tmr_lstm_window_fwd, the online path -- the forward recurrence alone over gate rows
//             that already lie in a resident table, addressed through a row table (a sliding
//             window of a ring); a second instantiation of the forward kernels, nothing saved.
//
// Persistent geometry (hidden size 512): workgroup (jx, by) owns hidden units 8*jx..8*jx+7 -- the
// 32 rows of W_hh (forward) / 8 columns of W_hh (backward) that feed them stay on the CU for all
// steps, in registers -- and clips 16*by..16*by+15; 64 x ceil(b/16) workgroups, one per CU.  Consecutive steps
// hand h_t (forward) / dgates_t (backward) between workgroups behind a grid barrier: write-through
// (sc1) stores, one monotonic counter, sc1 loads (every spin bounded; a give-up sets the timeout
// word).  The launch happens only when the whole grid fits the device at once (occupancy query x
// compute units, resident()); otherwise, or if the launch fails, the per-step path runs (one gate
// GEMM + one cell kernel per step).  A plain launch, not hipLaunchCooperativeKernel: the same
// residency rule, and a process that made a cooperative launch faulted in an exit handler under
// rocprofv3 (profiles/r3/exit_probe/), which kept the profiled step off this kernel.
#include "common.h"
#include "tmr.h"

namespace {

constexpr int LH = 512;        // hidden size served by the persistent kernels
constexpr int HU = 8;          // hidden units per workgroup
constexpr int NGC = 4 * HU;    // gate columns per workgroup
constexpr int BBC = 16;        // clips per workgroup
constexpr unsigned SPIN_LIMIT = 1u << 24;   // x s_sleep(1): ~0.5 s, then give up
// TMR_LSTM_SPIN_LIMIT overrides it (tests force a give-up to check that it is reported)
unsigned spin_limit() {
  const char* v = getenv("TMR_LSTM_SPIN_LIMIT");
  return v && v[0] ? (unsigned)strtoul(v, nullptr, 10) : SPIN_LIMIT;
}

typedef __attribute__((address_space(1))) unsigned gu32;

__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }

// Cell arithmetic of one (clip, unit), shared by the persistent kernels and their solo
// re-computation (below), so both produce the same bits.  No implicit FMA contraction: whether
// the compiler fuses a product into an add depended on how it vectorised the surrounding code
// (measured: 1 - g*g fused in one kernel, not in the other), so every product is rounded.
__device__ __forceinline__ float cell_fwd(const float gi, const float gf, const float gc,
                                          const float go, float& c, float& ig, float& fg,
                                          float& gg, float& og) {
#pragma clang fp contract(off)
  ig = sigm(gi); fg = sigm(gf);
  gg = tanhf(gc); og = sigm(go);
  c = fg * c + ig * gg;
  return og * tanhf(c);
}
__device__ __forceinline__ void cell_bwd(const float dh, const float ig, const float fg,
                                         const float gg, const float og, const float cv,
                                         const float cp, float& dc, float d[4]) {
#pragma clang fp contract(off)
  const float tc = tanhf(cv);
  const float dct = dh * og * (1.f - tc * tc) + dc;
  d[0] = dct * gg * ig * (1.f - ig);
  d[1] = dct * cp * fg * (1.f - fg);
  d[2] = dct * ig * (1.f - gg * gg);
  d[3] = dh * tc * og * (1.f - og);
  dc = dct * fg;
}

// Hand-off between steps (MI355X_MICROARCH.md, visibility: the counter row of the sc1 table).
// The handed-off bytes (h_t forward, dgates_t backward) are stored write-through (sc1) and every
// load of them in the kernel is an sc1 load, so no release / acquire fence is needed: each
// storing wave drains its stores, the workgroup barrier joins them, ONE lane adds to the counter
// and polls it (sc1 loads, bounded), the workgroup barrier releases the other waves.
// sync[0] = arrival counter, sync[1] = timeout word; both zeroed by the host before every
// launch.  Returns false after a give-up (every workgroup then leaves its loop: the results are
// garbage and the timeout word says so).
__device__ __forceinline__ void st_sc1(float* p, float v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // global_store sc1
}
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ld_sc1(__amdgpu_buffer_rsrc_t r, uint32_t off) {
  const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 16);   // aux 16 = sc1
  return __builtin_bit_cast(float4, v);
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const float* p, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc((void*)p, (short)0, (int)bytes, 0x00020000);
}

__device__ bool grid_barrier(unsigned* sync, unsigned target, unsigned limit) {
  gu32* cnt = (gu32*)sync;
  gu32* tmo = (gu32*)(sync + 1);
  __shared__ int ok_s;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every wave drains its own sc1 stores
  __syncthreads();
  if (threadIdx.x == 0) {
    __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int ok = 1;
    unsigned spins = 0;
    while (__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
      __builtin_amdgcn_s_sleep(1);
      if (++spins > limit ||
          __hip_atomic_load(tmo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) {
        __hip_atomic_store(tmo, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ok = 0;
        break;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   // compiler ordering only
    ok_s = ok;
  }
  __syncthreads();
  return ok_s != 0;
}

// ---------------------------------------------------------------- forward recurrence
// gx (b,t,4H): x W_ih^T + b_ih + b_hh.  Writes y (b,t,H) = h_t, and when given: cs (t,b,H) cell
// states, acts (t,b,4H) gate activations (i,f,g,o) for the backward, hn / cn (b,H).
// Thread (kg = tid / 32, c = tid % 32) keeps W_hh[row(c)][64 kg .. 64 kg + 63] in registers for
// all steps (the slice never leaves the CU); h_{t-1} of the 16 clips is staged in LDS with one
// batch of loads per thread; the 8 k-group partial dot products are added in a fixed order.
//
// WIN (tmr_lstm_window_fwd): the gate row of (clip, step) is gx + rows[clip * T + step] * 4H, a
// row of a resident gate table of nrows rows (an index outside it reads as zeros); nothing is
// saved, and only h_{T-1} leaves the hand-off sequence: hn + (out_rows ? out_rows[clip] : clip) * H.
template <bool WIN>
__device__ __forceinline__ void lstm_rec_fwd_body(const float* __restrict__ gx,
                                                  const float* __restrict__ whh,
                                                  float* __restrict__ y, float* __restrict__ cs,
                                                  float* __restrict__ acts,
                                                  float* __restrict__ hn, float* __restrict__ cn,
                                                  int B, int T, unsigned* sync, unsigned limit,
                                                  const int32_t* __restrict__ rows, long nrows,
                                                  const int32_t* __restrict__ out_rows) {
  constexpr int KG = 64;                 // k per register slice
  constexpr int HLD = LH + 4 * (LH / KG);  // padded h row: +4 floats per 64 (bank spread)
  __shared__ __attribute__((aligned(16))) float hs[BBC * HLD];
  __shared__ float red[BBC][NGC][LH / KG + 1];   // partial dot products per k-group
  __shared__ float gs[BBC][NGC + 1];              // gate pre-activations
  const int tid = threadIdx.x;
  const int j0 = blockIdx.x * HU;
  const int b0 = blockIdx.y * BBC;
  const int nwg = gridDim.x * gridDim.y;
  const int c = tid & (NGC - 1), kg = tid / NGC;            // 32 columns x 8 k-groups
  const int wrow = (c / HU) * LH + j0 + (c % HU);           // W_hh row of gate column c
  float wreg[KG];
#pragma unroll
  for (int i = 0; i < KG; i += 4) {
    const float4 v = *reinterpret_cast<const float4*>(&whh[(long)wrow * LH + kg * KG + i]);
    wreg[i] = v.x; wreg[i + 1] = v.y; wreg[i + 2] = v.z; wreg[i + 3] = v.w;
  }
  // cell role (tid < 128): clip cb, unit cu; the cell state lives in a register for all steps
  const int cb = tid / HU, cu = tid % HU;
  const int cgb = b0 + cb, cj = j0 + cu;
  const bool cell = tid < BBC * HU && cgb < B;
  float creg = 0.f;
  const __amdgpu_buffer_rsrc_t ry = rsrc(y, (uint32_t)((long)B * T * LH * 4));
  for (int t = 0; t < T; ++t) {
    // this step's input projections, issued before the h_{t-1} hand-off loads
    float gxv[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int o = tid + 256 * e;
      const int bl = o / NGC, cc = o % NGC;
      if (WIN) {
        const long r = b0 + bl < B ? (long)rows[(long)(b0 + bl) * T + t] : -1;
        gxv[e] = r >= 0 && r < nrows ? gx[r * (4 * LH) + (cc / HU) * LH + j0 + (cc % HU)] : 0.f;
      } else {
        gxv[e] = b0 + bl < B
                     ? gx[((long)(b0 + bl) * T + t) * (4 * LH) + (cc / HU) * LH + j0 + (cc % HU)]
                     : 0.f;
      }
    }
    if (t > 0) {
      constexpr int NL = BBC * (LH / 4) / 256;   // float4 loads per thread (8)
      float4 v[NL];
#pragma unroll
      for (int q = 0; q < NL; ++q) {
        const int idx = tid + 256 * q;
        const int bl = idx / (LH / 4), k4 = idx % (LH / 4);
        const uint32_t off = (uint32_t)((((long)(b0 + bl) * T + (t - 1)) * LH + 4 * k4) * 4);
        v[q] = ld_sc1(ry, b0 + bl < B ? off : 0x80000000u);   // out of range -> 0
      }
#pragma unroll
      for (int q = 0; q < NL; ++q) {
        const int idx = tid + 256 * q;
        const int bl = idx / (LH / 4), k = 4 * (idx % (LH / 4));
        *reinterpret_cast<float4*>(&hs[bl * HLD + k + 4 * (k / KG)]) = v[q];
      }
      __syncthreads();
#pragma unroll 4
      for (int bl = 0; bl < BBC; ++bl) {
        const float* hr = &hs[bl * HLD + kg * (KG + 4)];
        float a = 0.f;
#pragma unroll
        for (int i = 0; i < KG; i += 4) {
          const float4 h4 = *reinterpret_cast<const float4*>(hr + i);
          a = fmaf(h4.x, wreg[i], a); a = fmaf(h4.y, wreg[i + 1], a);
          a = fmaf(h4.z, wreg[i + 2], a); a = fmaf(h4.w, wreg[i + 3], a);
        }
        red[bl][c][kg] = a;
      }
      __syncthreads();
    }
    // gate pre-activations: thread -> (clip, 2 columns), k-groups added in order
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int o = tid + 256 * e;
      const int bl = o / NGC, cc = o % NGC;
      float a = 0.f;
      if (t > 0) {
#pragma unroll
        for (int g = 0; g < LH / KG; ++g) a += red[bl][cc][g];
      }
      gs[bl][cc] = gxv[e] + a;
    }
    __syncthreads();
    if (cell) {
      float ig, fg, gg, og;
      const float h = cell_fwd(gs[cb][cu], gs[cb][HU + cu], gs[cb][2 * HU + cu],
                               gs[cb][3 * HU + cu], creg, ig, fg, gg, og);
      st_sc1(&y[((long)cgb * T + t) * LH + cj], h);   // handed to every workgroup
      if (WIN) {
        if (t + 1 == T) hn[(long)(out_rows ? out_rows[cgb] : cgb) * LH + cj] = h;
      } else {
        if (cs) cs[((long)t * B + cgb) * LH + cj] = creg;
        if (acts) {
          float* a = acts + ((long)t * B + cgb) * (4 * LH);
          a[cj] = ig; a[LH + cj] = fg; a[2 * LH + cj] = gg; a[3 * LH + cj] = og;
        }
        if (t + 1 == T) {
          if (hn) hn[(long)cgb * LH + cj] = h;
          if (cn) cn[(long)cgb * LH + cj] = creg;
        }
      }
    }
    if (t + 1 < T && !grid_barrier(sync, (unsigned)((t + 1) * nwg), limit)) return;
  }
}

__global__ __launch_bounds__(256) void lstm_rec_fwd_k(const float* __restrict__ gx,
                                                      const float* __restrict__ whh,
                                                      float* __restrict__ y, float* __restrict__ cs,
                                                      float* __restrict__ acts,
                                                      float* __restrict__ hn,
                                                      float* __restrict__ cn, int B, int T,
                                                      unsigned* sync, unsigned limit) {
  lstm_rec_fwd_body<false>(gx, whh, y, cs, acts, hn, cn, B, T, sync, limit, nullptr, 0, nullptr);
}

// The window instantiation: y is the hand-off sequence in the workspace, out the caller's rows.
__global__ __launch_bounds__(256) void lstm_win_fwd_k(const float* __restrict__ gates,
                                                      const float* __restrict__ whh,
                                                      float* __restrict__ y,
                                                      float* __restrict__ out, int B, int T,
                                                      unsigned* sync, unsigned limit,
                                                      const int32_t* __restrict__ rows, long nrows,
                                                      const int32_t* __restrict__ out_rows) {
  lstm_rec_fwd_body<true>(gates, whh, y, nullptr, nullptr, out, nullptr, B, T, sync, limit, rows,
                          nrows, out_rows);
}

// ---------------------------------------------------------------- backward recurrence
// dy (b,t,H): dL/dh_t from the output sequence.  Writes dg (b,t,4H) = dL/d(gate pre-activations)
// and hprev (b,t,H) = h_{t-1} (0 at t = 0), the operand of dW_hh.
// Thread (g = tid / 8, u = tid % 8) keeps W_hh[64 g .. 64 g + 63][j0 + u] in registers; the whole
// dg_{t+1} row block of the 16 clips (16 x 2048) is staged in LDS with one batch of loads per
// thread; the 32 partial sums per (clip, unit) are added in a fixed order.
__global__ __launch_bounds__(256) void lstm_rec_bwd_k(const float* __restrict__ dy,
                                                      const float* __restrict__ whh,
                                                      const float* __restrict__ y,
                                                      const float* __restrict__ cs,
                                                      const float* __restrict__ acts,
                                                      float* __restrict__ dg,
                                                      float* __restrict__ hprev, int B, int T,
                                                      unsigned* sync, unsigned limit) {
  constexpr int G4 = 4 * LH;               // gate columns (2048)
  constexpr int KG = 64;                   // gate columns per register slice
  constexpr int NG = G4 / KG;              // 32 slices
  constexpr int DLDP = G4 + 4 * NG;        // padded dg row (+4 floats per 64: bank spread)
  __shared__ __attribute__((aligned(16))) float ds[BBC * DLDP];
  __shared__ float red[BBC * HU][NG + 1];
  const int tid = threadIdx.x;
  const int j0 = blockIdx.x * HU;
  const int b0 = blockIdx.y * BBC;
  const int nwg = gridDim.x * gridDim.y;
  const int u = tid % HU, g = tid / HU;
  float wreg[KG];
#pragma unroll
  for (int i = 0; i < KG; ++i) wreg[i] = whh[(long)(g * KG + i) * LH + j0 + u];
  // cell role (tid < 128)
  const int cb = tid / HU, cu = tid % HU;
  const int cgb = b0 + cb, cj = j0 + cu;
  const bool cell = tid < BBC * HU && cgb < B;
  float dc = 0.f;
  const __amdgpu_buffer_rsrc_t rdg = rsrc(dg, (uint32_t)((long)B * T * G4 * 4));
  for (int t = T - 1; t >= 0; --t) {
    // this step's cell operands (written by the forward launch), issued before the hand-off loads
    float dyv = 0.f, ig = 0.f, fg = 0.f, gg = 0.f, og = 0.f, cv = 0.f, cp = 0.f, hp = 0.f;
    if (cell) {
      dyv = dy[((long)cgb * T + t) * LH + cj];
      const float* a = acts + ((long)t * B + cgb) * G4;
      ig = a[cj]; fg = a[LH + cj]; gg = a[2 * LH + cj]; og = a[3 * LH + cj];
      cv = cs[((long)t * B + cgb) * LH + cj];
      if (t > 0) {
        cp = cs[((long)(t - 1) * B + cgb) * LH + cj];
        hp = y[((long)cgb * T + (t - 1)) * LH + cj];
      }
    }
    if (t + 1 < T) {
      constexpr int NL = BBC * (G4 / 4) / 256;   // float4 loads per thread (32)
      float4 v[NL];
#pragma unroll
      for (int q = 0; q < NL; ++q) {
        const int idx = tid + 256 * q;
        const int bl = idx / (G4 / 4), k4 = idx % (G4 / 4);
        const uint32_t off = (uint32_t)((((long)(b0 + bl) * T + (t + 1)) * G4 + 4 * k4) * 4);
        v[q] = ld_sc1(rdg, b0 + bl < B ? off : 0x80000000u);
      }
#pragma unroll
      for (int q = 0; q < NL; ++q) {
        const int idx = tid + 256 * q;
        const int bl = idx / (G4 / 4), k = 4 * (idx % (G4 / 4));
        *reinterpret_cast<float4*>(&ds[bl * DLDP + k + 4 * (k / KG)]) = v[q];
      }
      __syncthreads();
#pragma unroll 4
      for (int bl = 0; bl < BBC; ++bl) {
        const float* dr = &ds[bl * DLDP + g * (KG + 4)];
        float a = 0.f;
#pragma unroll
        for (int i = 0; i < KG; i += 4) {
          const float4 d4 = *reinterpret_cast<const float4*>(dr + i);
          a = fmaf(d4.x, wreg[i], a); a = fmaf(d4.y, wreg[i + 1], a);
          a = fmaf(d4.z, wreg[i + 2], a); a = fmaf(d4.w, wreg[i + 3], a);
        }
        red[bl * HU + u][g] = a;
      }
      __syncthreads();
    }
    if (cell) {
      float rec = 0.f;
      if (t + 1 < T) {
#pragma unroll
        for (int q = 0; q < NG; ++q) rec += red[tid][q];
      }
      const float dh = dyv + rec;
      float dv[4];
      cell_bwd(dh, ig, fg, gg, og, cv, cp, dc, dv);
      float* d = dg + ((long)cgb * T + t) * G4;
      st_sc1(&d[cj], dv[0]);                                 // handed to every workgroup
      st_sc1(&d[LH + cj], dv[1]);
      st_sc1(&d[2 * LH + cj], dv[2]);
      st_sc1(&d[3 * LH + cj], dv[3]);
      hprev[((long)cgb * T + t) * LH + cj] = hp;
    }
    if (t > 0 && !grid_barrier(sync, (unsigned)((T - t) * nwg), limit)) return;
  }
}

// ---------------------------------------------------------------- solo re-computation
// After a persistent launch that gave up a grid barrier (another stream or process held CUs, so
// not every workgroup became resident in time), the same stream runs the recurrence again in
// workgroups that need no barrier: each owns SPC clips and ALL hidden units (clips are
// independent; W_hh is streamed from L2 every step instead of held in registers).  The arithmetic
// is the persistent kernels' -- per 64-wide k-slice fmaf chains, slices added in order, the
// shared cell helpers -- so the outputs are the same bits.  A launch whose timeout word is 0 (the
// persistent kernel completed: every normal step) exits at once.  The word is set to 2
// ("recovered") so tmr_lstm_status_or does not report the step as failed.
constexpr int SPC = 4;   // clips per workgroup of the solo kernels

template <bool WIN>
__device__ __forceinline__ void lstm_rec_fwd_solo_body(const float* __restrict__ gx,
                                                       const float* __restrict__ whh,
                                                       float* __restrict__ y,
                                                       float* __restrict__ cs,
                                                       float* __restrict__ acts,
                                                       float* __restrict__ hn,
                                                       float* __restrict__ cn, int B, int T,
                                                       unsigned* sync,
                                                       const int32_t* __restrict__ rows,
                                                       long nrows,
                                                       const int32_t* __restrict__ out_rows) {
  if (sync[1] == 0u) return;
  if (blockIdx.x == 0 && threadIdx.x == 0) sync[1] = 2u;
  constexpr int G4 = 4 * LH, KG = 64;
  __shared__ __attribute__((aligned(16))) float hs[SPC][LH];
  __shared__ float gs[SPC][G4];
  const int tid = threadIdx.x, b0 = blockIdx.x * SPC;
  float creg[2][SPC];
#pragma unroll
  for (int e = 0; e < 2; ++e)
#pragma unroll
    for (int bl = 0; bl < SPC; ++bl) creg[e][bl] = 0.f;
  for (int t = 0; t < T; ++t) {
    for (int r = 0; r < G4 / 256; ++r) {      // gate column (row of W_hh) col, all SPC clips
      const int col = tid + 256 * r;
      float a[SPC];
#pragma unroll
      for (int bl = 0; bl < SPC; ++bl) a[bl] = 0.f;
      if (t > 0) {
        const float* wr = whh + (long)col * LH;
        for (int kg = 0; kg < LH / KG; ++kg) {
          float pa[SPC];
#pragma unroll
          for (int bl = 0; bl < SPC; ++bl) pa[bl] = 0.f;
#pragma unroll 4
          for (int i = 0; i < KG; i += 4) {
            const float4 w4 = *reinterpret_cast<const float4*>(wr + kg * KG + i);
#pragma unroll
            for (int bl = 0; bl < SPC; ++bl) {
              const float4 h4 = *reinterpret_cast<const float4*>(&hs[bl][kg * KG + i]);
              pa[bl] = fmaf(h4.x, w4.x, pa[bl]); pa[bl] = fmaf(h4.y, w4.y, pa[bl]);
              pa[bl] = fmaf(h4.z, w4.z, pa[bl]); pa[bl] = fmaf(h4.w, w4.w, pa[bl]);
            }
          }
#pragma unroll
          for (int bl = 0; bl < SPC; ++bl) a[bl] += pa[bl];
        }
      }
#pragma unroll
      for (int bl = 0; bl < SPC; ++bl) {
        if (b0 + bl >= B) continue;
        if (WIN) {
          const long r = rows[(long)(b0 + bl) * T + t];
          gs[bl][col] = (r >= 0 && r < nrows ? gx[r * G4 + col] : 0.f) + a[bl];
        } else {
          gs[bl][col] = gx[((long)(b0 + bl) * T + t) * G4 + col] + a[bl];
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int j = tid + 256 * e;
#pragma unroll
      for (int bl = 0; bl < SPC; ++bl) {
        const int cgb = b0 + bl;
        if (cgb >= B) continue;
        float ig, fg, gg, og;
        const float h = cell_fwd(gs[bl][j], gs[bl][LH + j], gs[bl][2 * LH + j],
                                 gs[bl][3 * LH + j], creg[e][bl], ig, fg, gg, og);
        y[((long)cgb * T + t) * LH + j] = h;
        hs[bl][j] = h;
        if (WIN) {
          if (t + 1 == T) hn[(long)(out_rows ? out_rows[cgb] : cgb) * LH + j] = h;
        } else {
          if (cs) cs[((long)t * B + cgb) * LH + j] = creg[e][bl];
          if (acts) {
            float* ap = acts + ((long)t * B + cgb) * G4;
            ap[j] = ig; ap[LH + j] = fg; ap[2 * LH + j] = gg; ap[3 * LH + j] = og;
          }
          if (t + 1 == T) {
            if (hn) hn[(long)cgb * LH + j] = h;
            if (cn) cn[(long)cgb * LH + j] = creg[e][bl];
          }
        }
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void lstm_rec_fwd_solo_k(const float* __restrict__ gx,
                                                           const float* __restrict__ whh,
                                                           float* __restrict__ y,
                                                           float* __restrict__ cs,
                                                           float* __restrict__ acts,
                                                           float* __restrict__ hn,
                                                           float* __restrict__ cn, int B, int T,
                                                           unsigned* sync) {
  lstm_rec_fwd_solo_body<false>(gx, whh, y, cs, acts, hn, cn, B, T, sync, nullptr, 0, nullptr);
}

__global__ __launch_bounds__(256) void lstm_win_fwd_solo_k(const float* __restrict__ gates,
                                                           const float* __restrict__ whh,
                                                           float* __restrict__ y,
                                                           float* __restrict__ out, int B, int T,
                                                           unsigned* sync,
                                                           const int32_t* __restrict__ rows,
                                                           long nrows,
                                                           const int32_t* __restrict__ out_rows) {
  lstm_rec_fwd_solo_body<true>(gates, whh, y, nullptr, nullptr, out, nullptr, B, T, sync, rows,
                               nrows, out_rows);
}

__global__ __launch_bounds__(256) void lstm_rec_bwd_solo_k(const float* __restrict__ dy,
                                                           const float* __restrict__ whh,
                                                           const float* __restrict__ y,
                                                           const float* __restrict__ cs,
                                                           const float* __restrict__ acts,
                                                           float* __restrict__ dg,
                                                           float* __restrict__ hprev, int B,
                                                           int T, unsigned* sync) {
  if (sync[1] == 0u) return;
  if (blockIdx.x == 0 && threadIdx.x == 0) sync[1] = 2u;
  constexpr int G4 = 4 * LH, KG = 64;
  __shared__ float ds[2][SPC][G4];   // dg of step t + 1 (read) and t (written), per clip
  const int tid = threadIdx.x, b0 = blockIdx.x * SPC;
  float dc[2][SPC];
#pragma unroll
  for (int e = 0; e < 2; ++e)
#pragma unroll
    for (int bl = 0; bl < SPC; ++bl) dc[e][bl] = 0.f;
  for (int t = T - 1; t >= 0; --t) {
    const int cur = t & 1, nxt = cur ^ 1;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int j = tid + 256 * e;
      float rec[SPC];
#pragma unroll
      for (int bl = 0; bl < SPC; ++bl) rec[bl] = 0.f;
      if (t + 1 < T) {
        for (int q = 0; q < G4 / KG; ++q) {
          float pa[SPC];
#pragma unroll
          for (int bl = 0; bl < SPC; ++bl) pa[bl] = 0.f;
#pragma unroll 8
          for (int i = 0; i < KG; ++i) {
            const float w = whh[(long)(q * KG + i) * LH + j];
#pragma unroll
            for (int bl = 0; bl < SPC; ++bl) pa[bl] = fmaf(ds[nxt][bl][q * KG + i], w, pa[bl]);
          }
#pragma unroll
          for (int bl = 0; bl < SPC; ++bl) rec[bl] += pa[bl];
        }
      }
#pragma unroll
      for (int bl = 0; bl < SPC; ++bl) {
        const int cgb = b0 + bl;
        if (cgb >= B) continue;
        const float dyv = dy[((long)cgb * T + t) * LH + j];
        const float* ap = acts + ((long)t * B + cgb) * G4;
        const float cv = cs[((long)t * B + cgb) * LH + j];
        const float cp = t > 0 ? cs[((long)(t - 1) * B + cgb) * LH + j] : 0.f;
        const float hp = t > 0 ? y[((long)cgb * T + (t - 1)) * LH + j] : 0.f;
        float dv[4];
        cell_bwd(dyv + rec[bl], ap[j], ap[LH + j], ap[2 * LH + j], ap[3 * LH + j], cv, cp,
                 dc[e][bl], dv);
        float* d = dg + ((long)cgb * T + t) * G4;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          d[q * LH + j] = dv[q];
          ds[cur][bl][q * LH + j] = dv[q];
        }
        hprev[((long)cgb * T + t) * LH + j] = hp;
      }
    }
    __syncthreads();
  }
}

// Test instrumentation (tmr_test_hold_cus): workgroups that occupy wave slots for a bounded
// number of s_sleep periods, so a test can make part of the device unavailable to another
// stream's launch.  Every wave leaves after `periods` sleeps.
__global__ __launch_bounds__(1024) void hold_cus_k(unsigned periods) {
  for (unsigned i = 0; i < periods; ++i) __builtin_amdgcn_s_sleep(127);
}

// ---------------------------------------------------------------- per-step fallback pieces
__global__ void add2_k(const float* __restrict__ a, const float* __restrict__ b,
                       float* __restrict__ o, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) o[i] = a[i] + b[i];
}

__global__ void copy_hprev_k(const float* __restrict__ y, float* __restrict__ hp, int B, int T,
                             int H) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= (long)B * T * H) return;
  const int j = (int)(i % H);
  const long bt = i / H;
  const int t = (int)(bt % T);
  hp[i] = t > 0 ? y[(bt - 1) * H + j] : 0.f;
}

// status |= timeout word of the last persistent launch on a workspace (stream-ordered, no sync)
__global__ void status_or_k(const unsigned* __restrict__ sync, int* __restrict__ status) {
  if (threadIdx.x == 0 && sync[1] == 1u) status[0] |= 1;   // 2 = recovered by the solo kernel
}

__global__ void copy_k(const float* __restrict__ a, float* __restrict__ o, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) o[i] = a[i];
}

// every workgroup of `grid` resident at once on this device (no other work assumed): the
// condition of a grid barrier that cannot deadlock
bool resident(const void* kernel, dim3 grid, int threads) {
  int dev = 0, cus = 0, per = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, kernel, threads, 0) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return (long)per * cus >= (long)grid.x * grid.y;
}

// TMR_LSTM_PERSIST=0 forces the per-step path (tests exercise both; read per call, no state)
bool persist_allowed() {
  const char* v = getenv("TMR_LSTM_PERSIST");
  return !(v && v[0] == '0');
}
// TMR_LSTM_RECOVER=0 leaves a give-up unrecovered (test hook: the health word's loud path)
bool recover_allowed() {
  const char* v = getenv("TMR_LSTM_RECOVER");
  return !(v && v[0] == '0');
}

// workspace layout (bytes, 256-aligned pieces)
struct LstmWs {
  size_t sync, bias, gx, ghh, dg, hprev, dcp, dhb, total;
};
size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
LstmWs lstm_ws(int b, int t, int i, int h) {
  (void)i;
  LstmWs w;
  size_t o = 0;
  w.sync = o; o += 256;
  w.bias = o; o += al256((size_t)4 * h * 4);
  w.gx = o; o += al256((size_t)b * t * 4 * h * 4);   // forward gx; backward dg (same size)
  w.dg = w.gx;
  w.ghh = o; o += al256((size_t)b * 4 * h * 4);       // per-step path: h W_hh^T
  w.hprev = o; o += al256((size_t)b * t * h * 4);
  w.dcp = o; o += al256((size_t)2 * b * h * 4);
  w.dhb = o; o += al256((size_t)b * h * 4);
  w.total = o;
  return w;
}

}  // namespace

TMR_API size_t tmr_lstm_saved_bytes(int b, int t, int h) {
  if (b < 0 || t < 0 || h <= 0) {
    tmr_set_error("tmr_lstm_saved_bytes: bad sizes b=%d t=%d h=%d", b, t, h);
    return 0;
  }
  return al256((size_t)t * b * h * 4) + al256((size_t)t * b * 4 * h * 4);
}

TMR_API size_t tmr_lstm_ws_bytes(int b, int t, int i, int h) {
  if (b < 0 || t < 0 || i <= 0 || h <= 0) {
    tmr_set_error("tmr_lstm_ws_bytes: bad sizes b=%d t=%d i=%d h=%d", b, t, i, h);
    return 0;
  }
  return lstm_ws(b, t, i, h).total;
}

// 32-bit buffer offsets in the persistent kernels' hand-off loads
static bool lstm_persistent_shape(int b, int t, int h) {
  return h == LH && b > 0 && (long)b * t * 4 * h * 4 < 0x80000000L;
}

TMR_API int tmr_lstm_fwd(const float* x, int b, int t, int i, int h, const float* w_ih,
                         const float* w_hh, const float* b_ih, const float* b_hh, float* y,
                         float* hn, float* cn, void* saved, size_t saved_bytes, void* ws,
                         size_t ws_bytes, hipStream_t stream) {
  TMR_CHECK_ARG(b >= 0 && t >= 0 && i > 0 && h > 0, "tmr_lstm_fwd: bad sizes b=%d t=%d i=%d h=%d",
                b, t, i, h);
  TMR_CHECK_ARG(x && w_ih && w_hh && b_ih && b_hh && y, "tmr_lstm_fwd: null operand");
  const LstmWs L = lstm_ws(b, t, i, h);
  TMR_CHECK_ARG(ws && ws_bytes >= L.total, "tmr_lstm_fwd: workspace %zu < %zu bytes", ws_bytes,
                L.total);
  // the barrier words (arrival counter, timeout) start at 0 on every call, also on the per-step
  // path and for empty inputs, so tmr_lstm_status_or never reads a stale or uninitialised word
  TMR_CHECK_ARG(hipMemsetAsync((char*)ws + L.sync, 0, 16, stream) == hipSuccess,
                "tmr_lstm_fwd: memset failed");
  float* cs = nullptr;
  float* acts = nullptr;
  if (saved) {
    TMR_CHECK_ARG(saved_bytes >= tmr_lstm_saved_bytes(b, t, h),
                  "tmr_lstm_fwd: saved buffer %zu < %zu bytes", saved_bytes,
                  tmr_lstm_saved_bytes(b, t, h));
    cs = (float*)saved;
    acts = (float*)((char*)saved + al256((size_t)t * b * h * 4));
  }
  if (b == 0 || t == 0) return 0;
  char* w = (char*)ws;
  float* bias = (float*)(w + L.bias);
  float* gx = (float*)(w + L.gx);
  hipLaunchKernelGGL(add2_k, dim3(cdiv(4 * h, 256)), dim3(256), 0, stream, b_ih, b_hh, bias, 4 * h);
  TMR_CHECK_LAUNCH("lstm bias");
  int rc = tmr_gemm_nt(b * t, 4 * h, i, x, i, w_ih, i, bias, gx, 4 * h, 0.f, stream);
  if (rc) return rc;
  unsigned* sync = (unsigned*)(w + L.sync);
  if (persist_allowed() && lstm_persistent_shape(b, t, h)) {
    dim3 grid(LH / HU, cdiv(b, BBC));
    const float* gxc = gx;
    unsigned lim = spin_limit();
    if (resident((const void*)lstm_rec_fwd_k, grid, 256)) {
      hipLaunchKernelGGL(lstm_rec_fwd_k, grid, dim3(256), 0, stream, gxc, w_hh, y, cs, acts, hn, cn,
                         b, t, sync, lim);
      if (hipGetLastError() == hipSuccess) {
        if (recover_allowed()) {   // exits at once unless the launch above gave up
          hipLaunchKernelGGL(lstm_rec_fwd_solo_k, dim3(cdiv(b, SPC)), dim3(256), 0, stream, gxc,
                             w_hh, y, cs, acts, hn, cn, b, t, sync);
          TMR_CHECK_LAUNCH("lstm_rec_fwd_solo_k");
        }
        return 0;
      }
    }
    // not resident: per-step path below
  }
  // per-step path: gate GEMM + fused cell kernel per step
  float* ghh = (float*)(w + L.ghh);
  float* cbuf[2] = {(float*)(w + L.dcp), (float*)(w + L.dcp) + (size_t)b * h};
  for (int s = 0; s < t; ++s) {
    if (s > 0) {
      rc = tmr_gemm_nt(b, 4 * h, h, y + (size_t)(s - 1) * h, t * h, w_hh, h, nullptr, ghh, 4 * h,
                       0.f, stream);
      if (rc) return rc;
    }
    float* c_out = cs ? cs + (size_t)s * b * h : cbuf[s & 1];
    const float* c_prev = s == 0 ? nullptr : (cs ? cs + (size_t)(s - 1) * b * h : cbuf[(s - 1) & 1]);
    rc = tmr_lstm_cell_fwd(gx + (size_t)s * 4 * h, t * 4 * h, s > 0 ? ghh : nullptr, c_prev,
                           y + (size_t)s * h, t * h, c_out, acts ? acts + (size_t)s * b * 4 * h : nullptr,
                           b, h, stream);
    if (rc) return rc;
    if (s == t - 1 && cn) {
      hipLaunchKernelGGL(copy_k, dim3(cdiv((long)b * h, 256)), dim3(256), 0, stream, c_out, cn, b * h);
      TMR_CHECK_LAUNCH("lstm c_n");
    }
  }
  if (hn) {
    TMR_CHECK_ARG(hipMemcpy2DAsync(hn, (size_t)h * 4, y + (size_t)(t - 1) * h, (size_t)t * h * 4,
                                   (size_t)h * 4, b, hipMemcpyDeviceToDevice, stream) == hipSuccess,
                  "tmr_lstm_fwd: h_n copy failed");
  }
  return 0;
}

// ---------------------------------------------------------------- sliding-window forward
namespace {

// per-step path of tmr_lstm_window_fwd: out row of clip b = its last hidden state
__global__ void win_out_k(const float* __restrict__ y, float* __restrict__ out,
                          const int32_t* __restrict__ out_rows, int B, int T, int H) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= (long)B * H) return;
  const int j = (int)(i % H);
  const long b = i / H;
  out[(long)(out_rows ? out_rows[b] : b) * H + j] = y[(b * T + (T - 1)) * H + j];
}

// workspace of tmr_lstm_window_fwd (bytes, 256-aligned pieces); the barrier words come first, as
// in LstmWs, so tmr_lstm_sync_status / tmr_lstm_status_or read them
struct WinWs {
  size_t sync, gx, ghh, y, c, total;
};
WinWs win_ws(int b, int t, int h) {
  WinWs w;
  size_t o = 0;
  w.sync = o; o += 256;
  w.gx = o; o += al256((size_t)b * t * 4 * h * 4);    // per-step path: the gathered gate rows
  w.ghh = o; o += al256((size_t)b * 4 * h * 4);       // per-step path: h W_hh^T
  w.y = o; o += al256((size_t)b * t * h * 4);         // hand-off sequence h_t
  w.c = o; o += al256((size_t)2 * b * h * 4);         // per-step path: cell states
  w.total = o;
  return w;
}

}  // namespace

TMR_API size_t tmr_lstm_window_ws_bytes(int b, int t, int h) {
  if (b < 0 || t < 0 || h <= 0) {
    tmr_set_error("tmr_lstm_window_ws_bytes: bad sizes b=%d t=%d h=%d", b, t, h);
    return 0;
  }
  return win_ws(b, t, h).total;
}

TMR_API int tmr_lstm_window_fwd(const float* gates, long nrows, const int32_t* rows, int b, int t,
                                int h, const float* w_hh, float* out, const int32_t* out_rows,
                                void* ws, size_t ws_bytes, hipStream_t stream) {
  TMR_CHECK_ARG(b >= 0 && t >= 0 && h > 0 && h % 4 == 0 && nrows >= 0,
                "tmr_lstm_window_fwd: bad sizes b=%d t=%d h=%d nrows=%ld", b, t, h, nrows);
  TMR_CHECK_ARG(gates && rows && w_hh && out, "tmr_lstm_window_fwd: null operand");
  const WinWs L = win_ws(b, t, h);
  TMR_CHECK_ARG(ws && ws_bytes >= L.total, "tmr_lstm_window_fwd: workspace %zu < %zu bytes",
                ws_bytes, L.total);
  // as tmr_lstm_fwd: the barrier words start at 0 on every call, on every path
  TMR_CHECK_ARG(hipMemsetAsync((char*)ws + L.sync, 0, 16, stream) == hipSuccess,
                "tmr_lstm_window_fwd: memset failed");
  if (b == 0 || t == 0) return 0;
  char* w = (char*)ws;
  unsigned* sync = (unsigned*)(w + L.sync);
  float* y = (float*)(w + L.y);
  if (persist_allowed() && lstm_persistent_shape(b, t, h) && b <= 4 * BBC) {
    dim3 grid(LH / HU, cdiv(b, BBC));
    unsigned lim = spin_limit();
    if (resident((const void*)lstm_win_fwd_k, grid, 256)) {
      hipLaunchKernelGGL(lstm_win_fwd_k, grid, dim3(256), 0, stream, gates, w_hh, y, out, b, t,
                         sync, lim, rows, nrows, out_rows);
      if (hipGetLastError() == hipSuccess) {
        if (recover_allowed()) {   // exits at once unless the launch above gave up
          hipLaunchKernelGGL(lstm_win_fwd_solo_k, dim3(cdiv(b, SPC)), dim3(256), 0, stream, gates,
                             w_hh, y, out, b, t, sync, rows, nrows, out_rows);
          TMR_CHECK_LAUNCH("lstm_win_fwd_solo_k");
        }
        return 0;
      }
    }
    // not resident: per-step path below
  }
  // per-step path: gather the window's gate rows, then gate GEMM + fused cell kernel per step
  float* gx = (float*)(w + L.gx);
  float* ghh = (float*)(w + L.ghh);
  float* cbuf[2] = {(float*)(w + L.c), (float*)(w + L.c) + (size_t)b * h};
  int rc = tmr_lfb_gather(gates, rows, gx, (long)b * t, 4 * h, stream);
  if (rc) return rc;
  for (int s = 0; s < t; ++s) {
    if (s > 0) {
      rc = tmr_gemm_nt(b, 4 * h, h, y + (size_t)(s - 1) * h, t * h, w_hh, h, nullptr, ghh, 4 * h,
                       0.f, stream);
      if (rc) return rc;
    }
    rc = tmr_lstm_cell_fwd(gx + (size_t)s * 4 * h, t * 4 * h, s > 0 ? ghh : nullptr,
                           s > 0 ? cbuf[(s - 1) & 1] : nullptr, y + (size_t)s * h, t * h,
                           cbuf[s & 1], nullptr, b, h, stream);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(win_out_k, dim3(cdiv((long)b * h, 256)), dim3(256), 0, stream, y, out,
                     out_rows, b, t, h);
  TMR_CHECK_LAUNCH("lstm window out");
  return 0;
}

TMR_API int tmr_lstm_bwd(const float* dy, const float* x, int b, int t, int i, int h,
                         const float* w_ih, const float* w_hh, const float* y, const void* saved,
                         size_t saved_bytes, float* dx, float* dw_ih, float* dw_hh, float* db_ih,
                         float* db_hh, void* ws, size_t ws_bytes, hipStream_t stream) {
  TMR_CHECK_ARG(b >= 0 && t >= 0 && i > 0 && h > 0, "tmr_lstm_bwd: bad sizes b=%d t=%d i=%d h=%d",
                b, t, i, h);
  TMR_CHECK_ARG(dy && x && w_ih && w_hh && y && saved && dw_ih && dw_hh && db_ih && db_hh,
                "tmr_lstm_bwd: null operand");
  const LstmWs L = lstm_ws(b, t, i, h);
  TMR_CHECK_ARG(ws && ws_bytes >= L.total, "tmr_lstm_bwd: workspace %zu < %zu bytes", ws_bytes,
                L.total);
  TMR_CHECK_ARG(hipMemsetAsync((char*)ws + L.sync, 0, 16, stream) == hipSuccess,
                "tmr_lstm_bwd: memset failed");
  TMR_CHECK_ARG(saved_bytes >= tmr_lstm_saved_bytes(b, t, h),
                "tmr_lstm_bwd: saved buffer %zu < %zu bytes", saved_bytes,
                tmr_lstm_saved_bytes(b, t, h));
  const float* cs = (const float*)saved;
  const float* acts = (const float*)((const char*)saved + al256((size_t)t * b * h * 4));
  char* w = (char*)ws;
  float* dg = (float*)(w + L.dg);
  float* hprev = (float*)(w + L.hprev);
  int rc;
  if (b == 0 || t == 0) {
    (void)hipMemsetAsync(dw_ih, 0, (size_t)4 * h * i * 4, stream);
    (void)hipMemsetAsync(dw_hh, 0, (size_t)4 * h * h * 4, stream);
    (void)hipMemsetAsync(db_ih, 0, (size_t)4 * h * 4, stream);
    (void)hipMemsetAsync(db_hh, 0, (size_t)4 * h * 4, stream);
    return 0;
  }
  bool done = false;
  unsigned* sync = (unsigned*)(w + L.sync);   // zeroed above (see tmr_lstm_fwd)
  if (persist_allowed() && lstm_persistent_shape(b, t, h)) {
    dim3 grid(LH / HU, cdiv(b, BBC));
    unsigned lim = spin_limit();
    if (resident((const void*)lstm_rec_bwd_k, grid, 256)) {
      hipLaunchKernelGGL(lstm_rec_bwd_k, grid, dim3(256), 0, stream, dy, w_hh, y, cs, acts, dg,
                         hprev, b, t, sync, lim);
      done = hipGetLastError() == hipSuccess;
      if (done && recover_allowed()) {   // exits at once unless the launch above gave up
        hipLaunchKernelGGL(lstm_rec_bwd_solo_k, dim3(cdiv(b, SPC)), dim3(256), 0, stream, dy, w_hh,
                           y, cs, acts, dg, hprev, b, t, sync);
        TMR_CHECK_LAUNCH("lstm_rec_bwd_solo_k");
      }
    }
  }
  if (!done) {
    float* dcp[2] = {(float*)(w + L.dcp), (float*)(w + L.dcp) + (size_t)b * h};
    float* dhb = (float*)(w + L.dhb);
    const float* dh_rec = nullptr;
    const float* dc_next = nullptr;
    for (int s = t - 1; s >= 0; --s) {
      rc = tmr_lstm_cell_bwd(dy + (size_t)s * h, t * h, dh_rec, dc_next, acts + (size_t)s * b * 4 * h,
                             cs + (size_t)s * b * h, s > 0 ? cs + (size_t)(s - 1) * b * h : nullptr,
                             dg + (size_t)s * 4 * h, t * 4 * h, dcp[s & 1], b, h, stream);
      if (rc) return rc;
      dc_next = dcp[s & 1];
      if (s > 0) {
        rc = tmr_gemm_nn(b, h, 4 * h, dg + (size_t)s * 4 * h, t * 4 * h, w_hh, h, dhb, h, 0.f, stream);
        if (rc) return rc;
        dh_rec = dhb;
      }
    }
    hipLaunchKernelGGL(copy_hprev_k, dim3(cdiv((long)b * t * h, 256)), dim3(256), 0, stream, y,
                       hprev, b, t, h);
    TMR_CHECK_LAUNCH("lstm hprev");
  }
  const int rows = b * t;
  rc = tmr_gemm_tn(4 * h, i, rows, dg, 4 * h, x, i, dw_ih, i, 0.f, stream);
  if (rc) return rc;
  rc = tmr_gemm_tn(4 * h, h, rows, dg, 4 * h, hprev, h, dw_hh, h, 0.f, stream);
  if (rc) return rc;
  rc = tmr_col_sum(dg, rows, 4 * h, 4 * h, db_ih, 0.f, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(copy_k, dim3(cdiv(4 * h, 256)), dim3(256), 0, stream, db_ih, db_hh, 4 * h);
  TMR_CHECK_LAUNCH("lstm db_hh");
  if (dx) {
    rc = tmr_gemm_nn(rows, i, 4 * h, dg, 4 * h, w_ih, i, dx, i, 0.f, stream);
    if (rc) return rc;
  }
  return 0;
}

// Timeout word of the last persistent launch on this workspace (0 = every grid barrier
// completed, 1 = a barrier gave up and the results are invalid, 2 = a barrier gave up and the
// solo kernel recomputed the recurrence).  Read it after the stream has drained; for tests and
// diagnostics.
TMR_API int tmr_lstm_sync_status(const void* ws, unsigned* timeout_out, hipStream_t stream) {
  TMR_CHECK_ARG(ws && timeout_out, "tmr_lstm_sync_status: null pointer");
  unsigned v[2] = {0, 0};
  if (hipMemcpyAsync(v, ws, 8, hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipStreamSynchronize(stream) != hipSuccess) {
    tmr_set_error("tmr_lstm_sync_status: copy failed");
    return 2;
  }
  *timeout_out = v[1];
  return 0;
}

// Fold the timeout word of the last persistent launch on ws into a caller-owned device status
// word (*status |= 1 after a give-up), enqueued on the stream: the caller checks the status at a
// point where it synchronises anyway (tmrnet_amd/health.py: once per optimizer step), so a
// give-up surfaces as an error instead of a silently wrong recurrence.
TMR_API int tmr_lstm_status_or(const void* ws, int32_t* status, hipStream_t stream) {
  TMR_CHECK_ARG(ws && status, "tmr_lstm_status_or: null pointer");
  hipLaunchKernelGGL(status_or_k, dim3(1), dim3(64), 0, stream, (const unsigned*)ws, (int*)status);
  TMR_CHECK_LAUNCH("lstm status_or");
  return 0;
}

// Test instrumentation: `wgs` workgroups of 1024 threads that sleep `ms` milliseconds on `stream`
// (bounded: every wave leaves after its sleep count), to hold wave slots while another stream
// launches work (tests/test_modules_gpu.py: the persistent LSTM next to a resident kernel).
TMR_API int tmr_test_hold_cus(int wgs, float ms, hipStream_t stream) {
  TMR_CHECK_ARG(wgs > 0 && wgs <= 65536 && ms >= 0.f && ms <= 10000.f,
                "tmr_test_hold_cus: wgs=%d ms=%g out of range", wgs, (double)ms);
  // s_sleep 127 = 127 x 64 clocks; at the 2.4 GHz shader clock about 3.4 us
  const unsigned periods = (unsigned)(ms * 1000.f / 3.4f) + 1u;
  hipLaunchKernelGGL(hold_cus_k, dim3(wgs), dim3(1024), 0, stream, periods);
  TMR_CHECK_LAUNCH("hold_cus_k");
  return 0;
}
