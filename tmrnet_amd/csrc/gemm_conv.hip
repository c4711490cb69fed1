// Implicit-GEMM convolution / GEMM engine: host side and C ABI (kernel template: gemm_kernel.h).
#include "direct_conv.h"
#include "gemm16_select.h"

#include <type_traits>

using namespace tmrg;

namespace {

// sum over the split slabs in split order, loads issued 8 at a time (the adds stay in order, so
// the result is bit-identical to a plain loop; only the load latency is overlapped)
__device__ __forceinline__ float split_sum(const float* __restrict__ slabs, int nsplit, long slab,
                                           long src) {
  float s = 0.f;
  int p = 0;
  for (; p + 8 <= nsplit; p += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = slabs[(p + u) * slab + src];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u];
  }
  for (; p < nsplit; ++p) s += slabs[p * slab + src];
  return s;
}

// WGRAD split reduction: dW[co][tap][c] (KRSC with c < creal) summed over splits in
// split order, written to OIHW (co, c, r, s) of the real weight.
__global__ void wgrad_reduce_kernel(const float* __restrict__ slabs, int nsplit, long slab,
                                    float* __restrict__ out, int Cout, int ntaps, int Cpad,
                                    int creal, float beta) {
  long total = (long)Cout * ntaps * creal;
  for (long o = blockIdx.x * (long)blockDim.x + threadIdx.x; o < total;
       o += (long)gridDim.x * blockDim.x) {
    // o indexes OIHW: co, c, tap
    int tap = (int)(o % ntaps);
    long t2 = o / ntaps;
    int c = (int)(t2 % creal);
    int co = (int)(t2 / creal);
    long src = ((long)co * ntaps + tap) * Cpad + c;
    const float s = split_sum(slabs, nsplit, slab, src);
    out[o] = beta != 0.f ? s + beta * out[o] : s;
  }
}

// The same reduction for multi-tap weights: one block per (co, 64-channel group) sums the splits
// with reads along c (coalesced), transposes (tap, c) -> (c, tap) through LDS and writes OIHW rows
// contiguously.  Per element the split order is the same as wgrad_reduce_kernel's.
constexpr int kReduceTaps = 7 * 7;   // the most taps it takes (its LDS tile)
__global__ __launch_bounds__(256) void wgrad_reduce_taps_kernel(const float* __restrict__ slabs,
                                                                int nsplit, long slab,
                                                                float* __restrict__ out, int ntaps,
                                                                int Cpad, int creal, float beta) {
  __shared__ float tile[kReduceTaps * 64];   // ntaps <= kReduceTaps, checked on the host
  const int co = blockIdx.x;
  const int c0 = blockIdx.y * 64;
  const int nc = min(64, creal - c0);
  for (int idx = threadIdx.x; idx < ntaps * 64; idx += 256) {
    const int tap = idx >> 6, cl = idx & 63;
    float sum = 0.f;
    if (cl < nc) sum = split_sum(slabs, nsplit, slab, ((long)co * ntaps + tap) * Cpad + c0 + cl);
    tile[tap * 64 + cl] = sum;
  }
  __syncthreads();
  float* o = out + ((long)co * creal + c0) * ntaps;
  for (int idx = threadIdx.x; idx < nc * ntaps; idx += 256) {
    const int cl = idx / ntaps, tap = idx - cl * ntaps;
    const float v = tile[tap * 64 + cl];
    o[idx] = beta != 0.f ? v + beta * o[idx] : v;
  }
}

template <int MODE>
int launch_gemm(const GemmArgs& a, bool al, int splits, hipStream_t st) {
  if (MODE == MODE_FWD) return launch_gemm_fwd(a, al, splits, st);
  if (MODE == MODE_DGRAD) return launch_gemm_dgrad(a, al, splits, st);
  return launch_gemm_wgrad(a, al, splits, st);
}

static inline long span(long pixels, int ld, int width) { return pixels > 0 ? (pixels - 1) * ld + width : 0; }

// element bytes of the conv operands (tmr_conv_desc.io: bf16-stored x / w / dy)
static inline int esz_x(const tmr_conv_desc* d) { return (d->io & TMR_IO_X_BF16) ? 2 : 4; }
static inline int esz_w(const tmr_conv_desc* d) { return (d->io & (TMR_IO_W_BF16 | TMR_IO_WT_BF16)) ? 2 : 4; }
static inline int esz_dy(const tmr_conv_desc* d) { return (d->io & TMR_IO_DY_BF16) ? 2 : 4; }
static inline int esz_y(const tmr_conv_desc* d) { return (d->io & TMR_IO_Y_BF16) ? 2 : 4; }
static inline int esz_bn(const tmr_conv_desc* d) { return (d->io & TMR_IO_BN_BF16) ? 2 : 4; }
static inline int esz_dx(const tmr_conv_desc* d) { return (d->io & TMR_IO_G16) ? 2 : 4; }
template <typename T>
static inline T* adv(T* p, long elems, int esz) {   // p + elems elements of esz bytes
  return p ? (T*)((typename std::conditional<std::is_const<T>::value, const char*, char*>::type)p +
                  elems * esz)
           : p;
}
static uint32_t clamp_bytes_e(long elems, int esz) {
  long b = elems * esz;
  return b >= 0x80000000L ? 0x80000000u : (uint32_t)b;
}

static uint32_t clamp_bytes(long elems) {
  long b = elems * 4;
  return b >= 0x80000000L ? 0x80000000u : (uint32_t)b;
}

int ilog2_exact(int v) {
  if (v <= 0 || (v & (v - 1))) return -1;
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}

bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

void set_taps(GemmArgs& a, int nR, int nS) {
  a.ntaps = nR * nS;
  a.tapS = nS > 0 ? nS : 1;
  a.tapSinv = (65536 + a.tapS - 1) / a.tapS;
}

void set_grid(GemmArgs& a, int n, int hg, int wg) {
  (void)n;
  a.dHW = make_fastdiv((uint32_t)(hg * wg));
  a.dW = make_fastdiv((uint32_t)wg);
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
static int conv_fwd_args(const tmr_conv_desc* d, const float* x, const float* w_krsc,
                         const float* bias, float* y, float beta, GemmArgs& a, bool& al) {
  TMR_CHECK_ARG(d, "tmr_conv2d_fwd: null descriptor");
  TMR_CHECK_ARG(d->math == TMR_MATH_F32 || d->math == TMR_MATH_BF16, "tmr_conv2d: bad math mode %d", d->math);
  TMR_CHECK_ARG((d->io & ~(TMR_IO_ENGINE | TMR_IO_CLASSES | TMR_IO_TILES)) == 0 || d->math == TMR_MATH_BF16, "tmr_conv2d: bf16-stored operands (io %d) need TMR_MATH_BF16", d->io);
  const int lc = ilog2_exact(d->c);
  TMR_CHECK_ARG(lc >= 2, "tmr_conv2d_fwd: stored input channels %d must be a power of two >= 4", d->c);
  a = GemmArgs{};
  a.A = x; a.B = w_krsc; a.C = y; a.bias = bias;
  a.M = d->n * d->ho * d->wo; a.N = d->k; a.K = d->r * d->s * d->c;
  a.log2C = lc;
  set_taps(a, d->r, d->s);
  a.oy0 = -d->pad; a.ox0 = -d->pad_w; a.dyr = 1; a.dxs = 1;
  set_grid(a, d->n, d->ho, d->wo);
  a.Hs = d->h; a.Ws = d->w; a.sy = d->stride; a.sx = d->stride;
  a.lds = xld_of(d); a.ldb = a.K; a.ldc = yld_of(d); a.beta = beta;
  a.Abytes = clamp_bytes_e(span((long)d->n * d->h * d->w, a.lds, d->c), esz_x(d));
  a.prec = d->math;
  a.Bbytes = clamp_bytes_e((long)d->k * a.K, esz_w(d));
  a.sab = ((d->io & TMR_IO_X_BF16) ? 1 : 0) | ((d->io & TMR_IO_W_BF16) ? 2 : 0);
  a.Cbytes = clamp_bytes(span((long)d->n * d->ho * d->wo, a.ldc, d->k));
  // (2: the whole-line store form of epilogue_batched, where the tile allows it)
  a.c16 = (d->io & TMR_IO_Y_BF16) ? 2 : 0;
  a.dma32 = d->math == TMR_MATH_F32;
  al = aligned16(x) && aligned16(w_krsc) && (d->k % 4 == 0) && (a.lds % 4 == 0);
  return 0;
}

// Frames per launch: the buffer descriptors take 32-bit byte offsets, so every operand of one
// launch must stay below 2 GiB; larger batches (e.g. C5's 1920 frames) run as several launches
// over consecutive frame ranges (d->max_frames caps it further, for tests).
static int frames_per_launch(const tmr_conv_desc* d) {
  const long xf = (long)d->h * d->w * xld_of(d) * 4;
  const long yf = (long)d->ho * d->wo * yld_of(d) * 4;
  const long mx = xf > yf ? xf : yf;
  long f = mx > 0 ? 0x7fffffffL / mx : d->n;
  if (d->max_frames > 0 && d->max_frames < f) f = d->max_frames;
  if (f > d->n) f = d->n;
  return (int)(f > 0 ? f : 1);
}

static tmr_conv_desc chunk_desc(const tmr_conv_desc* d, int nc) {
  tmr_conv_desc c = *d;
  c.n = nc;
  return c;
}

static int stats_parts_of(const tmr_conv_desc* d) {
  GemmArgs a;
  bool al;
  if (conv_fwd_args(d, nullptr, nullptr, nullptr, nullptr, 0.f, a, al)) return 0;
  return cdiv(a.M, gemm_tile_bm(a, MODE_FWD));
}

static long x_frame(const tmr_conv_desc* d) { return (long)d->h * d->w * xld_of(d); }
static long y_frame(const tmr_conv_desc* d) { return (long)d->ho * d->wo * yld_of(d); }

// Grouped convolutions (tmr_conv_desc.groups = G > 1): group g reads input channels
// [g*c/G, (g+1)*c/G) and writes output channels [g*k/G, (g+1)*k/G); each group is one launch on
// channel slices (pixel strides = the whole tensors').  Weights per group are consecutive blocks
// of (k/G)*(c/G)*r*s elements: KRSC (k, r, s, c/G), the transposed copy (G, c/G, r, s, k/G), and
// OIHW gradients (k, c/G, r, s), i.e. torch's grouped Conv2d weight layout.
static int group_split(const tmr_conv_desc* d, tmr_conv_desc& g) {
  const int G = ngroups(d);
  TMR_CHECK_ARG(d->c % G == 0 && d->k % G == 0, "tmr_conv2d: channels %d / %d not divisible by %d groups",
                d->c, d->k, G);
  g = *d;
  g.x_ld = xld_of(d);
  g.y_ld = yld_of(d);
  g.c = d->c / G;
  g.k = d->k / G;
  g.groups = 0;
  return 0;
}
static long group_wsize(const tmr_conv_desc* g) { return (long)g->k * g->r * g->s * g->c; }

// One visit per (group, frame chunk) of a conv, groups outermost: body(slice, group, first frame),
// slice = the group's channel-slice descriptor cut to the chunk's frames.  one_group: group 0
// only (the planning queries: every group has the same tiling).
template <typename F>
static int for_slices(const tmr_conv_desc* d, F&& body, bool one_group = false) {
  tmr_conv_desc g = *d;
  if (ngroups(d) > 1 && group_split(d, g)) return 1;
  const int fc = frames_per_launch(&g), G = one_group ? 1 : ngroups(d);
  for (int i = 0; i < G; ++i)
    for (int f0 = 0; f0 < g.n; f0 += fc) {
      const int rc = body(chunk_desc(&g, g.n - f0 < fc ? g.n - f0 : fc), i, f0);
      if (rc) return rc;
    }
  return 0;
}
// element offsets of a slice in the whole operands: x / dx, y / dy, the weights
static long x_off(const tmr_conv_desc& c, int g, int f0) { return (long)g * c.c + f0 * x_frame(&c); }
static long y_off(const tmr_conv_desc& c, int g, int f0) { return (long)g * c.k + f0 * y_frame(&c); }
static long w_off(const tmr_conv_desc& c, int g) { return g * group_wsize(&c); }

// The direct kernel families (direct_conv.h), in lookup order.  A geometry one of them serves
// skips the engine; TMR_IO_ENGINE (tests) keeps every conv on the engine.
static const DirectConv* const kDirect[] = {&tmr_direct_stem(), &tmr_direct_stem16(),
                                            &tmr_direct_d3(), &tmr_direct_d3s()};
template <typename V>
static const V* direct_view(const tmr_conv_desc* d, V DirectConv::*view) {
  if (d->io & TMR_IO_ENGINE) return nullptr;
  for (const DirectConv* f : kDirect)
    if ((f->*view).serves && (f->*view).serves(d)) return &(f->*view);
  return nullptr;
}

TMR_API int tmr_conv2d_fwd(const tmr_conv_desc* d, const float* x, const float* w_krsc,
                           const float* bias, float* y, float beta, hipStream_t stream) {
  TMR_CHECK_ARG(d, "tmr_conv2d_fwd: null descriptor");
  return for_slices(d, [&](const tmr_conv_desc& c, int g, int f0) -> int {
    GemmArgs a;
    bool al;
    const int rc = conv_fwd_args(&c, adv(x, x_off(c, g, f0), esz_x(d)), adv(w_krsc, w_off(c, g), esz_w(d)),
                                 bias ? bias + (long)g * c.k : nullptr,
                                 adv(y, y_off(c, g, f0), esz_y(d)), beta, a, al);
    if (rc) return rc;
    TMR_CHECK_ARG(!(a.c16 && (beta != 0.f || bias)),
                  "tmr_conv2d_fwd: a bf16 output (TMR_IO_Y_BF16) takes no beta / bias");
    return launch_gemm<MODE_FWD>(a, al, 1, stream);
  });
}

TMR_API int tmr_conv2d_fwd_fused(const tmr_conv_desc* d, const float* x, const float* w_krsc,
                                 const float* scale, const float* shift, const float* residual,
                                 float* y, int relu, hipStream_t stream) {
  TMR_CHECK_ARG(d, "tmr_conv2d_fwd_fused: null descriptor");
  TMR_CHECK_ARG(scale && shift, "tmr_conv2d_fwd_fused: null BatchNorm scale/shift");
  TMR_CHECK_ARG(!residual || residual != y, "tmr_conv2d_fwd_fused: residual must not alias y");
  // (a grouped conv with a bf16 output: each group's slice passes the bf16-output checks below on
  // its own base and the whole tensor's y_ld -- the INF16 stores address dwords of two columns
  // from the slice base with the row stride ldc, and bound the columns by the slice's N)
  return for_slices(d, [&](const tmr_conv_desc& c, int g, int f0) -> int {
    const long o = (long)g * c.k;
    GemmArgs a;
    bool al;
    const int rc = conv_fwd_args(&c, adv(x, x_off(c, g, f0), esz_x(d)), adv(w_krsc, w_off(c, g), esz_w(d)),
                                 shift + o, adv(y, y_off(c, g, f0), esz_y(d)), 0.f, a, al);
    if (rc) return rc;
    a.scale = scale + o;
    a.res = adv(residual, y_off(c, g, f0), esz_y(d));
    a.relu = relu;
    if (a.c16) {
      // bf16 activations (TMR_IO_Y_BF16): y and the residual are bf16, moved as dwords of two
      // columns; the LDS-DMA engine's forwards carry this epilogue (gemm16_fwd_inf16.hip)
      TMR_CHECK_ARG(use16(a, MODE_FWD),
                    "tmr_conv2d_fwd_fused: a bf16 output (TMR_IO_Y_BF16) needs bf16 x and w "
                    "(TMR_IO_X_BF16 | TMR_IO_W_BF16), channels and row strides multiples of 8");
      TMR_CHECK_ARG(a.N % 2 == 0 && a.ldc % 2 == 0 && (((uintptr_t)a.C | (uintptr_t)a.res) & 3) == 0,
                    "tmr_conv2d_fwd_fused: a bf16 output needs even channels / y_ld and 4-B "
                    "aligned y and residual");
      a.Cbytes = clamp_bytes_e(span((long)c.n * c.ho * c.wo, a.ldc, c.k), 2);
    }
    return launch_gemm<MODE_FWD>(a, al, 1, stream);
  });
}

// The fp32 fused forward that also writes the bf16 copy z16 of its output (GemmArgs::Cbf; the
// LDS-DMA engine's kernels of gemm16_fwd_dual32.hip).  Every slice is checked before the first one
// is launched: a refusal launches nothing, and there is no two-pass fall-back.
TMR_API int tmr_conv2d_fwd_fused_dual(const tmr_conv_desc* d, const float* x, const float* w_krsc,
                                      const float* scale, const float* shift,
                                      const float* residual, float* z, void* z16, int relu,
                                      hipStream_t stream) {
  TMR_CHECK_ARG(d, "tmr_conv2d_fwd_fused_dual: null descriptor");
  TMR_CHECK_ARG(x && w_krsc && z, "tmr_conv2d_fwd_fused_dual: null x / w / z");
  TMR_CHECK_ARG(scale && shift, "tmr_conv2d_fwd_fused_dual: null BatchNorm scale/shift");
  TMR_CHECK_ARG(d->math == TMR_MATH_F32 && (d->io & ~(TMR_IO_ENGINE | TMR_IO_CLASSES | TMR_IO_TILES)) == 0,
                "tmr_conv2d_fwd_fused_dual: fp32 operands in fp32 math only (math %d, io %d)",
                d->math, d->io);
  TMR_CHECK_ARG(ngroups(d) == 1, "tmr_conv2d_fwd_fused_dual: no grouped conv (groups %d)", d->groups);
  TMR_CHECK_ARG(d->n > 0 && d->k > 0 && d->ho > 0 && d->wo > 0, "tmr_conv2d_fwd_fused_dual: empty output");
  TMR_CHECK_ARG(yld_of(d) == d->k, "tmr_conv2d_fwd_fused_dual: z and z16 must be dense (y_ld == k)");
  TMR_CHECK_ARG(d->k % 2 == 0, "tmr_conv2d_fwd_fused_dual: output channels %d must be even "
                "(z16 is stored as dwords of two columns)", d->k);
  TMR_CHECK_ARG(z16, "tmr_conv2d_fwd_fused_dual: null z16");
  TMR_CHECK_ARG(!residual || residual != z, "tmr_conv2d_fwd_fused_dual: residual must not alias z");
  const size_t elems = (size_t)d->n * d->ho * d->wo * d->k;
  const auto apart = [&](const void* p) {   // the fp32 tensor at p against z16's bytes
    return !p || (const char*)p + elems * 4 <= (const char*)z16 ||
           (const char*)z16 + elems * 2 <= (const char*)p;
  };
  TMR_CHECK_ARG(apart(z) && apart(residual), "tmr_conv2d_fwd_fused_dual: z16 overlaps z or the residual");
  TMR_CHECK_ARG(aligned16(z16) && aligned16(z),
                "tmr_conv2d_fwd_fused_dual: z and z16 must be 16-B aligned (whole-line stores)");
  for (int pass = 0; pass < 2; ++pass) {   // 0: check every slice, 1: launch
    const int rc = for_slices(d, [&](const tmr_conv_desc& c, int g, int f0) -> int {
      GemmArgs a;
      bool al;
      const int rc = conv_fwd_args(&c, adv(x, x_off(c, g, f0), 4), w_krsc, shift,
                                   adv(z, y_off(c, g, f0), 4), 0.f, a, al);
      if (rc) return rc;
      a.scale = scale;
      a.res = adv(residual, y_off(c, g, f0), 4);
      a.relu = relu;
      a.Cbf = adv(z16, y_off(c, g, f0), 2);
      TMR_CHECK_ARG(use16(a, MODE_FWD),
                    "tmr_conv2d_fwd_fused_dual: not a shape of the fp32 LDS-DMA forward (16-B "
                    "aligned x / w, stored channels and row strides multiples of 4; c %d, x_ld %d, "
                    "r %d, s %d) -- run tmr_conv2d_fwd_fused and a cast instead",
                    c.c, xld_of(&c), c.r, c.s);
      TMR_CHECK_ARG(((uintptr_t)a.Cbf & 3) == 0, "tmr_conv2d_fwd_fused_dual: z16 chunk not 4-B aligned");
      return pass == 0 ? 0 : launch_gemm<MODE_FWD>(a, al, 1, stream);
    });
    if (rc) return rc;
  }
  return 0;
}

TMR_API int tmr_conv2d_fwd_stats_parts(const tmr_conv_desc* d) {
  if (!d || d->n <= 0) {
    tmr_set_error("tmr_conv2d_fwd_stats_parts: null or empty descriptor");
    return -1;
  }
  if (const auto* f = direct_view(d, &DirectConv::fwd)) return f->parts(d);
  int parts = 0;
  const auto count = [&](const tmr_conv_desc& c, int, int) {
    parts += stats_parts_of(&c);
    return 0;
  };
  return for_slices(d, count, true) ? -1 : parts;
}

// stats: partial rows of d->k columns, a group's k columns at its offset; the rows of a group's
// frame chunks follow each other
TMR_API int tmr_conv2d_fwd_bnstats(const tmr_conv_desc* d, const float* x, const float* w_krsc,
                                   float* y, void* stats, size_t stats_bytes, hipStream_t stream) {
  TMR_CHECK_ARG(d, "tmr_conv2d_fwd_bnstats: null descriptor");
  TMR_CHECK_ARG(yld_of(d) == d->k, "tmr_conv2d_fwd_bnstats: output must be dense (y_ld == k)");
  const int np = tmr_conv2d_fwd_stats_parts(d);
  TMR_CHECK_ARG(np >= 0, "tmr_conv2d_fwd_bnstats: bad descriptor");
  const size_t need = (size_t)np * d->k * sizeof(float4);
  TMR_CHECK_ARG(stats && stats_bytes >= need, "tmr_conv2d_fwd_bnstats: stats buffer too small (%zu < %zu)",
                stats_bytes, need);
  if (const auto* f = direct_view(d, &DirectConv::fwd)) return f->run(d, x, w_krsc, y, stats, stream);
  float4* st = nullptr;
  return for_slices(d, [&](const tmr_conv_desc& c, int g, int f0) -> int {
    if (f0 == 0) st = (float4*)stats + (long)g * c.k;
    GemmArgs a;
    bool al;
    const int rc = conv_fwd_args(&c, adv(x, x_off(c, g, f0), esz_x(d)), adv(w_krsc, w_off(c, g), esz_w(d)),
                                 nullptr, adv(y, y_off(c, g, f0), esz_y(d)), 0.f, a, al);
    if (rc) return rc;
    a.stats = st;
    a.part_ld = d->k;
    st += (long)stats_parts_of(&c) * d->k;
    return launch_gemm<MODE_FWD>(a, al, 1, stream);
  });
}

// Fused BatchNorm-backward epilogue state of one dgrad call (nullptr: plain dgrad).  part
// advances over the launches; count_only tallies the partial rows without launching.
struct BnBwdFuse {
  const float *y, *z, *sc, *sh, *mean;
  int mask;
  float2* part;
  long nparts;
  bool count_only;
  int part_ld;   // columns per partial row (the total channels of a grouped dgrad)
  const void* old;   // the beta operand when it is not dx itself (nullptr: dx)
  int old16;         // the beta operand is bf16
};

// The launch plan of one GEMM view (tmr_conv2d_tile): the engine and tile config launch_gemm<MODE>
// takes for `a`, from the functions it calls.
static void tile_of(const GemmArgs& a, int mode, tmr_conv_tile* t) {
  const bool f32 = a.prec == TMR_MATH_F32;
  if (use16(a, mode)) {
    t->engine = 2;
    t->cfg = pick_cfg16(a.M, a.N, a.K, mode, f32);
    const Cfg16 c = kCfgs16[t->cfg];
    t->bm = c.bm; t->bn = c.bn; t->waves = c.waves;
    t->tapv = tapv16(a, mode, f32) ? 1 : 0;
  } else {
    t->engine = 1;
    t->cfg = pick_cfg(a.M, a.N, a.K, mode);
    const TileCfg c = kCfgs[t->cfg];
    t->bm = c.bm; t->bn = c.bn; t->waves = c.waves;
    t->tapv = 0;
  }
}

// plan: launches nothing and describes the stride-parity classes in *plan (tmr_conv2d_tile)
static int conv_dgrad_impl(const tmr_conv_desc* d, const float* dy, const float* w_krsc,
                           float* dx, float beta, hipStream_t stream, BnBwdFuse* fz = nullptr,
                           tmr_conv_tile* plan = nullptr) {
  TMR_CHECK_ARG(d->math == TMR_MATH_F32 || d->math == TMR_MATH_BF16, "tmr_conv2d: bad math mode %d", d->math);
  const int lk = ilog2_exact(d->k);
  TMR_CHECK_ARG(lk >= 2, "tmr_conv2d_dgrad: output channels %d must be a power of two >= 4", d->k);
  TMR_CHECK_ARG(d->c % 4 == 0, "tmr_conv2d_dgrad: input channels %d must be a multiple of 4", d->c);
  TMR_CHECK_ARG(!(d->io & TMR_IO_WT_BF16) || !(d->io & TMR_IO_W_BF16),
                "tmr_conv2d_dgrad: TMR_IO_WT_BF16 and TMR_IO_W_BF16 are exclusive weight layouts");
  TMR_CHECK_ARG(!(d->io & TMR_IO_WT_F32) ||
                    (d->math == TMR_MATH_F32 && (d->io & ~(TMR_IO_ENGINE | TMR_IO_CLASSES | TMR_IO_TILES)) == TMR_IO_WT_F32),
                "tmr_conv2d_dgrad: TMR_IO_WT_F32 (fp32 transposed weights) needs TMR_MATH_F32 and "
                "no bf16-stored operand");
  TMR_CHECK_ARG((d->io & ~(TMR_IO_WT_F32 | TMR_IO_ENGINE | TMR_IO_CLASSES | TMR_IO_TILES)) == 0 ||
                    d->math == TMR_MATH_BF16,
                "tmr_conv2d: bf16-stored operands (io %d) need TMR_MATH_BF16", d->io);
  const int st = d->stride;
  // one GEMM per stride-parity class (ph,pw): rows h = st*y + ph.  Stride 2 on the LDS-DMA
  // engine: the classes go out as one launch (launch_gemm_dgrad_par; TMR_IO_CLASSES: one each)
  const bool par = st == 2 && !(d->io & TMR_IO_CLASSES);
  GemmArgs pend[PAR_MAX];
  bool pend_al[PAR_MAX];
  int npend = 0;
  long best_m = -1;
  for (int ph = 0; ph < st; ++ph) {
    for (int pw = 0; pw < st; ++pw) {
      // valid kernel rows r with (ph + pad - r) % st == 0
      int r0 = -1, nR = 0, s0 = -1, nS = 0;
      for (int r = 0; r < d->r; ++r)
        if (((ph + d->pad - r) % st + st) % st == 0) { if (r0 < 0) r0 = r; ++nR; }
      for (int s = 0; s < d->s; ++s)
        if (((pw + d->pad_w - s) % st + st) % st == 0) { if (s0 < 0) s0 = s; ++nS; }
      const int hg = (d->h - ph + st - 1) / st, wg = (d->w - pw + st - 1) / st;
      if (hg <= 0 || wg <= 0) continue;
      GemmArgs a{};
      a.A = dy; a.B = w_krsc; a.C = dx; a.bias = nullptr;
      a.M = d->n * hg * wg; a.N = d->c; a.K = nR * nS * d->k;
      a.log2C = lk;
      set_taps(a, nR, nS);
      if (nR == 0 || nS == 0) { a.K = 0; a.ntaps = 0; }
      // ho = (h + pad - r)/st = y + (ph + pad - r0)/st - ri
      a.oy0 = nR ? (ph + d->pad - r0) / st : 0;
      a.ox0 = nS ? (pw + d->pad_w - s0) / st : 0;
      a.dyr = -1; a.dxs = -1;
      a.wr0 = r0 < 0 ? 0 : r0; a.ws0 = s0 < 0 ? 0 : s0; a.wst = st; a.wS = d->s;
      set_grid(a, d->n, hg, wg);
      a.Hs = d->ho; a.Ws = d->wo; a.sy = 1; a.sx = 1;
      a.lds = yld_of(d); a.ldb = d->r * d->s * d->c; a.ldc = xld_of(d); a.beta = beta;
      a.Abytes = clamp_bytes_e(span((long)d->n * d->ho * d->wo, a.lds, d->k), esz_dy(d));
      a.prec = d->math;
      a.Bbytes = clamp_bytes_e((long)d->k * d->r * d->s * d->c, esz_w(d));
      a.sab = ((d->io & TMR_IO_DY_BF16) ? 1 : 0) | ((d->io & (TMR_IO_W_BF16 | TMR_IO_WT_BF16)) ? 2 : 0);
      if (d->io & (TMR_IO_WT_BF16 | TMR_IO_WT_F32)) {   // w = Wt[ci][r][s][co] (bf16 / fp32)
        a.wt = 1;
        a.ldbt = d->r * d->s * d->k;
      }
      a.Cbytes = clamp_bytes(span((long)d->n * d->h * d->w, a.ldc, d->c));
      a.oH = d->h; a.oW = d->w; a.osy = st; a.osx = st; a.oyc = ph; a.oxc = pw;
      if (plan) {   // the non-empty classes; the tile of the largest (the first of equals)
        if (a.K > 0) {
          ++plan->classes;
          if (a.M > best_m) {
            best_m = a.M;
            tile_of(a, MODE_DGRAD, plan);
          }
        }
        continue;
      }
      // nothing to add -- unless the fused BN backward must still see (mask, sum) these pixels
      if (a.K == 0 && beta == 1.f && !fz) continue;
      if (fz) {
        const long nmt = cdiv(a.M, gemm_tile_bm(a, MODE_DGRAD));
        if (fz->count_only) { fz->nparts += nmt; continue; }
        a.bn_y = fz->y; a.bn_z = fz->z; a.bn_sc = fz->sc; a.bn_sh = fz->sh; a.bn_mean = fz->mean;
        a.bn_mask = fz->mask;
        a.bn16 = (d->io & TMR_IO_BN_BF16) ? 1 : 0;
        if (d->io & TMR_IO_G16) {   // dx (g) stored bf16: C's extent in bytes of bf16
          a.g16 = 1;
          a.Cbytes = clamp_bytes_e(span((long)d->n * d->h * d->w, a.ldc, d->c), 2);
        }
        a.bn_part = fz->part;
        a.part_ld = fz->part_ld;
        a.Cold = fz->old;
        a.cold16 = fz->old16;
        a.io_tiles = (d->io & TMR_IO_TILES) ? 1 : 0;
        fz->part += nmt * fz->part_ld;
        fz->nparts += nmt;
      }
      bool al = aligned16(dy) && aligned16(w_krsc) && aligned16(dx) && a.lds % 4 == 0;
      if (par) {
        pend[npend] = a;
        pend_al[npend++] = al;
        continue;
      }
      const int rc = launch_gemm<MODE_DGRAD>(a, al, 1, stream);
      if (rc) return rc;
    }
  }
  if (npend > 0) {
    int rc = launch_gemm_dgrad_par(pend, npend, stream);
    if (rc < 0) {   // not eligible: one launch per class
      rc = 0;
      for (int i = 0; i < npend && rc == 0; ++i)
        rc = launch_gemm<MODE_DGRAD>(pend[i], pend_al[i], 1, stream);
    }
    if (rc) return rc;
  }
  return 0;
}

// The fused dgrad over every slice of d; fz holds the whole operands (group 0, frame 0): y / z /
// the old dx are laid out like dx, a group's scale / shift / mean and partial columns start at its
// channels.  count_only: launches nothing and adds one group's partial rows to *nparts.
static int dgrad_bnbwd_run(const tmr_conv_desc* d, const float* dy, const float* w_krsc, float* dx,
                           float beta, const BnBwdFuse& fz, long* nparts, hipStream_t stream) {
  float2* part = nullptr;
  const auto slice = [&](const tmr_conv_desc& c, int g, int f0) -> int {
    const long o = (long)g * c.c, px = x_off(c, g, f0);
    if (f0 == 0) part = adv(fz.part, o, sizeof(float2));
    BnBwdFuse s = fz;
    s.y = adv(fz.y, px, esz_bn(d));
    // mask 3: z is bits, 32 elements per word (ungrouped, h*w*c % 32 == 0: checked by the caller)
    s.z = fz.mask == 3 ? (const float*)((const uint32_t*)fz.z + px / 32) : adv(fz.z, px, esz_bn(d));
    s.sc = adv(fz.sc, o, 4); s.sh = adv(fz.sh, o, 4); s.mean = adv(fz.mean, o, 4);
    s.old = adv(fz.old, px, fz.old16 ? 2 : 4);
    s.part = part;
    s.nparts = 0;
    const int rc = conv_dgrad_impl(&c, adv(dy, y_off(c, g, f0), esz_dy(d)), adv(w_krsc, w_off(c, g), esz_w(d)),
                                   adv(dx, px, esz_dx(d)), beta, stream, &s);
    part = s.part;
    if (nparts) *nparts += s.nparts;
    return rc;
  };
  return for_slices(d, slice, fz.count_only);
}

long tmrg::g_dgrad_ws_launches = 0;
TMR_API long tmr_dgrad_ws_launches(void) { return __atomic_load_n(&g_dgrad_ws_launches, __ATOMIC_RELAXED); }

TMR_API int tmr_conv2d_dgrad_bnbwd_parts(const tmr_conv_desc* d) {
  if (!d || d->n <= 0) {
    tmr_set_error("tmr_conv2d_dgrad_bnbwd_parts: null or empty descriptor");
    return -1;
  }
  if (const auto* f = direct_view(d, &DirectConv::dgrad)) return f->parts(d);
  BnBwdFuse fz{};
  fz.count_only = true;
  long np = 0;
  if (dgrad_bnbwd_run(d, nullptr, nullptr, nullptr, 1.f, fz, &np, nullptr)) return -1;
  return (int)np;
}

static int dgrad_bnbwd_entry(const tmr_conv_desc* d, const float* dy, const float* w_krsc,
                             float* dx, float beta, const void* dx_old, int old_bf16,
                             const float* y, const float* z, const float* scale,
                             const float* shift, const float* mean, int mask, void* parts,
                             size_t parts_bytes, hipStream_t stream) {
  TMR_CHECK_ARG(xld_of(d) == d->c, "tmr_conv2d_dgrad_bnbwd: dx must be dense (x_ld == c)");
  TMR_CHECK_ARG(ngroups(d) == 1 || mask != 3,
                "tmr_conv2d_dgrad_bnbwd: a grouped dgrad takes no ReLU-mask bits");
  TMR_CHECK_ARG(y && mean && parts, "tmr_conv2d_dgrad_bnbwd: null y / mean / parts");
  TMR_CHECK_ARG(!(d->io & TMR_IO_G16) ||
                    (d->math == TMR_MATH_BF16 && (d->io & TMR_IO_WT_BF16) &&
                     (d->c / ngroups(d)) % 8 == 0),
                "tmr_conv2d_dgrad_bnbwd: a bf16 gradient (TMR_IO_G16) needs bf16 math on the LDS-DMA "
                "engine (TMR_IO_WT_BF16), channels per group a multiple of 8");
  TMR_CHECK_ARG(!dx_old || ngroups(d) == 1, "tmr_conv2d_dgrad_bnbwd: a separate old dx takes no groups");
  // a grouped dgrad writes each group's channel slice of a bf16 gradient with beta == 0 only (the
  // trunk's G16 on ResNeSt's radix-2 conv); accumulating into a bf16 dx runs ungrouped
  TMR_CHECK_ARG(ngroups(d) == 1 || beta == 0.f || !(d->io & TMR_IO_G16),
                "tmr_conv2d_dgrad_bnbwd: a grouped dgrad accumulates (beta != 0) into fp32 dx only");
  TMR_CHECK_ARG(mask == 0 || (mask == 1 && z) || (mask == 2 && scale && shift) || (mask == 3 && z),
                "tmr_conv2d_dgrad_bnbwd: mask %d needs z (1, 3: bits) or scale/shift (2)", mask);
  TMR_CHECK_ARG(mask != 3 || ((d->io & (TMR_IO_WT_F32 | TMR_IO_WT_BF16)) &&
                              ((long)d->h * d->w * d->c) % 32 == 0),
                "tmr_conv2d_dgrad_bnbwd: ReLU-mask bits (mask 3) need the LDS-DMA dgrad "
                "(TMR_IO_WT_F32 / TMR_IO_WT_BF16) and h*w*c a multiple of 32");
  const int np = tmr_conv2d_dgrad_bnbwd_parts(d);
  TMR_CHECK_ARG(np >= 0 && parts_bytes >= (size_t)np * d->c * sizeof(float2),
                "tmr_conv2d_dgrad_bnbwd: parts buffer too small");
  if (const auto* f = direct_view(d, &DirectConv::dgrad)) {   // (np counted the direct kernel's rows)
    TMR_CHECK_ARG(!dx_old && !((d->io & TMR_IO_G16) && beta != 0.f),
                  "tmr_conv2d_dgrad_bnbwd: the direct 3x3 dgrad takes no old dx / "
                  "accumulating bf16 gradient");
    return f->run(d, dy, w_krsc, dx, beta, y, z, scale, shift, mean, mask, parts, stream);
  }
  BnBwdFuse fz{};
  fz.y = y; fz.z = z; fz.sc = scale; fz.sh = shift; fz.mean = mean; fz.mask = mask;
  fz.part = (float2*)parts;
  fz.part_ld = d->c;   // (the total channels of a grouped dgrad)
  fz.old = dx_old;
  // (a grouped dgrad has no old dx, and beta != 0 with a bf16 dx is rejected above)
  fz.old16 = beta != 0.f ? old_bf16 : 0;
  return dgrad_bnbwd_run(d, dy, w_krsc, dx, beta, fz, nullptr, stream);
}

TMR_API int tmr_conv2d_dgrad_bnbwd(const tmr_conv_desc* d, const float* dy, const float* w_krsc,
                                   float* dx, float beta, const float* y, const float* z,
                                   const float* scale, const float* shift, const float* mean,
                                   int mask, void* parts, size_t parts_bytes, hipStream_t stream) {
  TMR_CHECK_ARG(d, "tmr_conv2d_dgrad_bnbwd: null descriptor");
  // in place: a bf16 gradient (TMR_IO_G16) accumulates into its own bf16 values
  return dgrad_bnbwd_entry(d, dy, w_krsc, dx, beta, nullptr, (d->io & TMR_IO_G16) ? 1 : 0, y, z,
                           scale, shift, mean, mask, parts, parts_bytes, stream);
}

TMR_API int tmr_conv2d_dgrad_bnbwd_acc(const tmr_conv_desc* d, const float* dy,
                                       const float* w_krsc, void* dx, float beta,
                                       const void* dx_old, int old_bf16, const float* y,
                                       const float* z, const float* scale, const float* shift,
                                       const float* mean, int mask, void* parts,
                                       size_t parts_bytes, hipStream_t stream) {
  TMR_CHECK_ARG(d, "tmr_conv2d_dgrad_bnbwd_acc: null descriptor");
  TMR_CHECK_ARG(beta != 0.f && dx_old && ((uintptr_t)dx_old & 15) == 0 &&
                    (d->io & TMR_IO_G16) && (d->io & TMR_IO_WT_BF16),
                "tmr_conv2d_dgrad_bnbwd_acc: needs beta != 0, a 16-B aligned old dx and a bf16 "
                "output (TMR_IO_G16) on the bf16 LDS-DMA engine (TMR_IO_WT_BF16)");
  return dgrad_bnbwd_entry(d, dy, w_krsc, (float*)dx, beta, dx_old, old_bf16 ? 1 : 0, y, z, scale,
                           shift, mean, mask, parts, parts_bytes, stream);
}

TMR_API int tmr_conv2d_dgrad(const tmr_conv_desc* d, const float* dy, const float* w_krsc,
                             float* dx, float beta, hipStream_t stream) {
  TMR_CHECK_ARG(d, "tmr_conv2d_dgrad: null descriptor");
  return for_slices(d, [&](const tmr_conv_desc& c, int g, int f0) {
    return conv_dgrad_impl(&c, adv(dy, y_off(c, g, f0), esz_dy(d)), adv(w_krsc, w_off(c, g), esz_w(d)),
                           dx + x_off(c, g, f0), beta, stream);
  });
}

// the WGRAD view of a conv (no pointers, no split plan)
static void wgrad_fill(const tmr_conv_desc* d, GemmArgs& a) {
  a = GemmArgs{};
  a.M = d->k; a.N = d->r * d->s * d->c; a.K = d->n * d->ho * d->wo;
  a.log2C = ilog2_exact(d->c);
  set_taps(a, d->r, d->s);
  a.oy0 = -d->pad; a.ox0 = -d->pad_w; a.dyr = 1; a.dxs = 1;
  set_grid(a, d->n, d->ho, d->wo);
  a.Hs = d->h; a.Ws = d->w; a.sy = d->stride; a.sx = d->stride;
  a.lds = xld_of(d); a.ldb = yld_of(d); a.ldc = a.N; a.beta = 0.f;
  a.Abytes = clamp_bytes_e(span((long)d->n * d->ho * d->wo, a.ldb, d->k), esz_dy(d));
  a.prec = d->math;
  a.Bbytes = clamp_bytes_e(span((long)d->n * d->h * d->w, a.lds, d->c), esz_x(d));
  a.sab = ((d->io & TMR_IO_DY_BF16) ? 1 : 0) | ((d->io & TMR_IO_X_BF16) ? 2 : 0);
  a.dma32 = d->math == TMR_MATH_F32;
}

static int wgrad_plan(const tmr_conv_desc* d, int* splits, int* kchunk, long* slab) {
  const long Mred = (long)d->n * d->ho * d->wo;
  const long Mo = d->k, No = (long)d->r * d->s * d->c;
  GemmArgs a;
  wgrad_fill(d, a);
  const long tiles = gemm_tiles(a, MODE_WGRAD);
  // aim for ~target workgroups; at least minrows reduction rows per split
  static const long target = env_int("TMR_WGRAD_TARGET", 512);
  static const long minrows = env_int("TMR_WGRAD_MINROWS", 1024);
  long sp = target / (tiles > 0 ? tiles : 1);
  if (sp < 1) sp = 1;
  long maxsp = Mred / minrows;
  if (maxsp < 1) maxsp = 1;
  if (sp > maxsp) sp = maxsp;
  long kc = (Mred + sp - 1) / sp;
  kc = (kc + 63) / 64 * 64;  // multiple of every BK (16, 32, 64)
  sp = (Mred + kc - 1) / kc;
  *splits = (int)sp;
  *kchunk = (int)kc;
  *slab = Mo * No;
  return 0;
}

// the direct wgrad of a conv with c_real real input channels (0: any, the workspace query)
static const DirectConv::Wgrad* direct_wgrad(const tmr_conv_desc* d, int c_real) {
  const DirectConv::Wgrad* f = direct_view(d, &DirectConv::wgrad);
  return f && (c_real == 0 || f->c_real == 0 || f->c_real == c_real) ? f : nullptr;
}

TMR_API size_t tmr_conv2d_wgrad_ws_bytes(const tmr_conv_desc* d) {
  if (!d || d->n <= 0 || d->k <= 0 || d->c <= 0 || d->r <= 0 || d->s <= 0) {
    tmr_set_error("tmr_conv2d_wgrad_ws_bytes: null or empty descriptor");
    return 0;
  }
  // one group's workspace, reused in turn: the largest plan of its frame chunks (a smaller chunk
  // can keep more splits: its chunk length rounds up less)
  size_t bytes = 0;
  const auto plan = [&](const tmr_conv_desc& c, int, int) {
    int sp, kc;
    long slab;
    wgrad_plan(&c, &sp, &kc, &slab);
    if ((size_t)sp * slab * sizeof(float) > bytes) bytes = (size_t)sp * slab * sizeof(float);
    return 0;
  };
  if (for_slices(d, plan, true)) return 0;
  if (const auto* f = direct_wgrad(d, 0))
    if (bytes < f->ws_bytes(d)) bytes = f->ws_bytes(d);
  return bytes;
}

// the engine's split slabs (wgrad_plan) summed in split order into the OIHW gradient
static int wgrad_reduce(const tmr_conv_desc* d, const float* ws, int sp, long slab, float* dw_oihw,
                        int c_real, float beta, hipStream_t stream) {
  const int ntaps = d->r * d->s;
  if (ntaps > 1 && ntaps <= kReduceTaps) {
    hipLaunchKernelGGL(wgrad_reduce_taps_kernel, dim3(d->k, cdiv(c_real, 64)), dim3(256), 0,
                       stream, ws, sp, slab, dw_oihw, ntaps, d->c, c_real, beta);
    TMR_CHECK_LAUNCH("wgrad_reduce_taps_kernel");
    return 0;
  }
  long total = (long)d->k * ntaps * c_real;
  int blocks = (int)((total + 255) / 256);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(blocks), dim3(256), 0, stream, ws, sp, slab,
                     dw_oihw, d->k, ntaps, d->c, c_real, beta);
  TMR_CHECK_LAUNCH("wgrad_reduce_kernel");
  return 0;
}

static int conv_wgrad_impl(const tmr_conv_desc* d, const float* x, const float* dy,
                           float* dw_oihw, int c_real, float beta, float* ws, size_t ws_bytes,
                           hipStream_t stream) {
  TMR_CHECK_ARG(d->math == TMR_MATH_F32 || d->math == TMR_MATH_BF16, "tmr_conv2d: bad math mode %d", d->math);
  const int lc = ilog2_exact(d->c);
  TMR_CHECK_ARG(lc >= 2, "tmr_conv2d_wgrad: stored input channels %d must be a power of two >= 4", d->c);
  TMR_CHECK_ARG(c_real >= 1 && c_real <= d->c, "tmr_conv2d_wgrad: bad c_real %d", c_real);
  if (const auto* f = direct_wgrad(d, c_real)) {   // the family's partial slabs, reduced here
    DirectSlabs sl{};
    const int rc = f->run(d, x, dy, ws, ws_bytes, &sl, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(wgrad_reduce_taps_kernel, dim3(d->k, cdiv(c_real, 64)), dim3(256), 0, stream,
                       ws, sl.n, sl.elems, dw_oihw, sl.taps, sl.cstored, c_real, beta);
    TMR_CHECK_LAUNCH("wgrad_reduce_taps_kernel");
    return 0;
  }
  int sp, kc;
  long slab;
  wgrad_plan(d, &sp, &kc, &slab);
  TMR_CHECK_ARG(ws && ws_bytes >= (size_t)sp * slab * sizeof(float),
                "tmr_conv2d_wgrad: workspace too small (%zu < %zu)", ws_bytes,
                (size_t)sp * slab * sizeof(float));
  GemmArgs a;
  wgrad_fill(d, a);
  a.A = dy; a.B = x; a.C = ws; a.bias = nullptr;
  a.kchunk = kc; a.slab = slab;
  a.Cbytes = clamp_bytes(slab);
  bool al = aligned16(x) && aligned16(dy) && (d->k % 4 == 0) && a.lds % 4 == 0 && a.ldb % 4 == 0;
  const int rc = launch_gemm<MODE_WGRAD>(a, al, sp, stream);
  if (rc) return rc;
  return wgrad_reduce(d, ws, sp, slab, dw_oihw, c_real, beta, stream);
}

// frame chunks accumulate into dw in chunk order (beta = 1 after the first): deterministic; the
// groups reuse the workspace in turn (c_real = real input channels per group; dw (k, c_real, r, s))
TMR_API int tmr_conv2d_wgrad(const tmr_conv_desc* d, const float* x, const float* dy,
                             float* dw_oihw, int c_real, float beta, float* ws, size_t ws_bytes,
                             hipStream_t stream) {
  TMR_CHECK_ARG(d, "tmr_conv2d_wgrad: null descriptor");
  return for_slices(d, [&](const tmr_conv_desc& c, int g, int f0) {
    return conv_wgrad_impl(&c, adv(x, x_off(c, g, f0), esz_x(d)), adv(dy, y_off(c, g, f0), esz_dy(d)),
                           dw_oihw + (long)g * c.k * c_real * c.r * c.s, c_real,
                           f0 == 0 ? beta : 1.f, ws, ws_bytes, stream);
  });
}

// The wgrad that produces its dy operand itself (gemm16_kernel.h, BNW): dy = A*g + B*y + C per
// channel, the BatchNorm-backward apply of tmr_bn_bwd_parts folded into the load of the A operand;
// dy_out is written once (from the n-tile 0 workgroups) for the dgrad that follows.
// Why the fused form does not serve (d, operands), or nullptr when it does.  Null pointers are not
// judged (the query before the tensors exist).
static const char* wgrad_bnbwd_why(const tmr_conv_desc* d, int c_real, const void* x, const void* g,
                                   const void* y, const void* dy_out) {
  if (d->n <= 0 || d->k <= 0 || d->c <= 0 || d->r <= 0 || d->s <= 0) return "empty descriptor";
  if (d->math != TMR_MATH_F32) return "fp32 math only";
  if (d->io & (TMR_IO_X_BF16 | TMR_IO_DY_BF16)) return "a bf16 operand";
  if (ngroups(d) > 1) return "grouped conv";
  if (frames_per_launch(d) < d->n) return "frame-chunked tensors";
  if (d->k % 8 != 0) return "output channels not a multiple of 8 (the 8-wide apply's domain)";
  if (yld_of(d) != d->k) return "g / y / dy must be dense";
  if (ilog2_exact(d->c) < 2) return "stored input channels must be a power of two >= 4";
  if (direct_wgrad(d, c_real)) return "the wgrad runs on a direct kernel";
  if ((((uintptr_t)x | (uintptr_t)g | (uintptr_t)y | (uintptr_t)dy_out) & 15) != 0)
    return "operands must be 16-B aligned";
  GemmArgs a;
  wgrad_fill(d, a);
  if (!use16(a, MODE_WGRAD)) return "not an LDS-DMA engine wgrad";
  if (!wgrad_bnbwd_cfg(pick_cfg16(a.M, a.N, a.K, MODE_WGRAD, true)))
    return "tile config without the fused form";
  return nullptr;
}

TMR_API int tmr_conv2d_wgrad_bnbwd_ok(const tmr_conv_desc* d, const void* x, const void* g,
                                      const void* y, const void* dy_out) {
  return d && !wgrad_bnbwd_why(d, 0, x, g, y, dy_out) ? 1 : 0;
}

long tmrg::g_wgrad_bnbwd_launches = 0;
TMR_API long tmr_wgrad_bnbwd_launches(void) {
  return __atomic_load_n(&g_wgrad_bnbwd_launches, __ATOMIC_RELAXED);
}

TMR_API int tmr_conv2d_wgrad_bnbwd(const tmr_conv_desc* d, const float* x, const float* g,
                                   const float* y, const float* coef, float* dy_out,
                                   float* dw_oihw, int c_real, float beta, float* ws,
                                   size_t ws_bytes, hipStream_t stream) {
  TMR_CHECK_ARG(d && x && g && y && coef && dy_out && dw_oihw, "tmr_conv2d_wgrad_bnbwd: null operand");
  TMR_CHECK_ARG(c_real >= 1 && c_real <= d->c, "tmr_conv2d_wgrad_bnbwd: bad c_real %d", c_real);
  const char* why = wgrad_bnbwd_why(d, c_real, x, g, y, dy_out);
  TMR_CHECK_ARG(!why, "tmr_conv2d_wgrad_bnbwd: no fused form (%s); ask tmr_conv2d_wgrad_bnbwd_ok "
                "and keep tmr_bn_bwd_parts + tmr_conv2d_wgrad", why);
  TMR_CHECK_ARG(((uintptr_t)coef & 15) == 0, "tmr_conv2d_wgrad_bnbwd: coef must be 16-B aligned");
  // n-tiles other than 0 read g after n-tile 0 may have written dy: no overlap
  const size_t ybytes = (size_t)d->n * d->ho * d->wo * d->k * sizeof(float);
  const auto apart = [&](const void* p) {
    return (const char*)p + ybytes <= (const char*)dy_out || (const char*)dy_out + ybytes <= (const char*)p;
  };
  TMR_CHECK_ARG(apart(g) && apart(y), "tmr_conv2d_wgrad_bnbwd: dy_out overlaps g or y");
  int sp, kc;
  long slab;
  wgrad_plan(d, &sp, &kc, &slab);
  TMR_CHECK_ARG(ws && ws_bytes >= (size_t)sp * slab * sizeof(float),
                "tmr_conv2d_wgrad_bnbwd: workspace too small (%zu < %zu)", ws_bytes,
                (size_t)sp * slab * sizeof(float));
  GemmArgs a;
  wgrad_fill(d, a);
  a.A = g; a.B = x; a.C = ws; a.bias = nullptr;
  a.bn_y = y; a.bn_sc = coef; a.Cold = dy_out;
  a.kchunk = kc; a.slab = slab;
  a.Cbytes = clamp_bytes(slab);
  const int rc = launch_gemm16_wgrad_bnbwd(a, sp, stream);
  if (rc) return rc;
  __atomic_fetch_add(&g_wgrad_bnbwd_launches, 1L, __ATOMIC_RELAXED);
  return wgrad_reduce(d, ws, sp, slab, dw_oihw, c_real, beta, stream);
}

// The launch plan of one view of a conv: host code only, nothing is launched.  Each answer comes
// from the function the launch itself calls (tile_of; conv_dgrad_impl's class walk; wgrad_plan), on
// the first (group, frame chunk) slice.  Without operands the pointers count as 16-B aligned.
TMR_API int tmr_conv2d_tile(const tmr_conv_desc* d, int view, tmr_conv_tile* out) {
  TMR_CHECK_ARG(d && out, "tmr_conv2d_tile: null descriptor / result");
  TMR_CHECK_ARG(view >= 0 && view <= 2, "tmr_conv2d_tile: view %d is not 0 (fwd), 1 (dgrad), 2 (wgrad)", view);
  TMR_CHECK_ARG(d->n > 0 && d->k > 0 && d->c > 0 && d->r > 0 && d->s > 0 && d->stride > 0,
                "tmr_conv2d_tile: empty descriptor");
  *out = tmr_conv_tile{};
  out->cfg = -1;
  const bool direct = view == 0   ? direct_view(d, &DirectConv::fwd) != nullptr
                      : view == 1 ? direct_view(d, &DirectConv::dgrad) != nullptr
                                  : direct_wgrad(d, 0) != nullptr;
  if (direct) return 0;   // engine 0
  bool first = true;
  return for_slices(d, [&](const tmr_conv_desc& c, int, int) -> int {
    if (!first) return 0;
    first = false;
    GemmArgs a;
    if (view == 0) {
      bool al;
      if (const int rc = conv_fwd_args(&c, nullptr, nullptr, nullptr, nullptr, 0.f, a, al)) return rc;
      tile_of(a, MODE_FWD, out);
    } else if (view == 1) {
      if (const int rc = conv_dgrad_impl(&c, nullptr, nullptr, nullptr, 0.f, nullptr, nullptr, out))
        return rc;
    } else {
      TMR_CHECK_ARG(c.math == TMR_MATH_F32 || c.math == TMR_MATH_BF16, "tmr_conv2d: bad math mode %d", c.math);
      TMR_CHECK_ARG(ilog2_exact(c.c) >= 2, "tmr_conv2d_wgrad: stored input channels %d must be a power of two >= 4", c.c);
      long slab;
      wgrad_plan(&c, &out->splits, &out->kchunk, &slab);
      wgrad_fill(&c, a);
      tile_of(a, MODE_WGRAD, out);
    }
    return 0;
  }, true);
}

// Plain GEMMs on the same engine ---------------------------------------------
// C[M][N] (row stride ldc) = beta*C + A[M][K] (row stride lda) * B^T, B = [N][K] (ldb) (+bias[N])
TMR_API int tmr_gemm_nt(int M, int N, int K, const float* A, int lda, const float* B, int ldb,
                        const float* bias, float* C, int ldc, float beta, hipStream_t stream) {
  TMR_CHECK_ARG(M >= 0 && N >= 0 && K >= 0, "tmr_gemm_nt: negative size");
  GemmArgs a{};
  a.A = A; a.B = B; a.C = C; a.bias = bias;
  a.M = M; a.N = N; a.K = K; a.log2C = 0;
  set_taps(a, 1, 1);
  a.dyr = 1; a.dxs = 1;
  set_grid(a, M, 1, 1);
  a.Hs = 1; a.Ws = 1; a.sy = 1; a.sx = 1;
  a.lds = lda; a.ldb = ldb; a.ldc = ldc; a.beta = beta;
  a.Abytes = clamp_bytes(M > 0 ? (long)(M - 1) * lda + K : 0);
  a.Bbytes = clamp_bytes(N > 0 ? (long)(N - 1) * ldb + K : 0);
  a.Cbytes = clamp_bytes(M > 0 ? (long)(M - 1) * ldc + N : 0);
  bool al = aligned16(A) && aligned16(B) && lda % 4 == 0 && ldb % 4 == 0 && K % 4 == 0;
  return launch_gemm<MODE_FWD>(a, al, 1, stream);
}

// C[M][N] = beta*C + A[M][K] (lda) * B[K][N] (ldb)
TMR_API int tmr_gemm_nn(int M, int N, int K, const float* A, int lda, const float* B, int ldb,
                        float* C, int ldc, float beta, hipStream_t stream) {
  TMR_CHECK_ARG(M >= 0 && N >= 0 && K >= 0, "tmr_gemm_nn: negative size");
  GemmArgs a{};
  a.A = A; a.B = B; a.C = C; a.bias = nullptr;
  a.M = M; a.N = N; a.K = K; a.log2C = 0;
  set_taps(a, 1, 1);
  a.oy0 = 0; a.ox0 = 0; a.dyr = -1; a.dxs = -1;
  a.wr0 = 0; a.ws0 = 0; a.wst = 1; a.wS = 1;
  set_grid(a, M, 1, 1);
  a.Hs = 1; a.Ws = 1; a.sy = 1; a.sx = 1;
  a.lds = lda; a.ldb = ldb; a.ldc = ldc; a.beta = beta;
  a.oH = 1; a.oW = 1; a.osy = 1; a.osx = 1; a.oyc = 0; a.oxc = 0;   // identity row map
  a.Abytes = clamp_bytes(M > 0 ? (long)(M - 1) * lda + K : 0);
  a.Bbytes = clamp_bytes(K > 0 ? (long)(K - 1) * ldb + N : 0);
  a.Cbytes = clamp_bytes(M > 0 ? (long)(M - 1) * ldc + N : 0);
  bool al = aligned16(A) && aligned16(B) && lda % 4 == 0 && ldb % 4 == 0 && K % 4 == 0 &&
            N % 4 == 0;
  return launch_gemm<MODE_DGRAD>(a, al, 1, stream);
}

// C[M][N] = beta*C + A^T B, A = [K][M] (lda), B = [K][N] (ldb)   (no split: small K)
TMR_API int tmr_gemm_tn(int M, int N, int K, const float* A, int lda, const float* B, int ldb,
                        float* C, int ldc, float beta, hipStream_t stream) {
  TMR_CHECK_ARG(M >= 0 && N >= 0 && K >= 0, "tmr_gemm_tn: negative size");
  GemmArgs a{};
  a.A = A; a.B = B; a.C = C; a.bias = nullptr;
  a.M = M; a.N = N; a.K = K; a.log2C = 0;
  set_taps(a, 1, 1);
  a.dyr = 1; a.dxs = 1;
  set_grid(a, K, 1, 1);
  a.Hs = 1; a.Ws = 1; a.sy = 1; a.sx = 1;
  a.lds = ldb; a.ldb = lda; a.ldc = ldc; a.beta = beta;
  a.kchunk = K > 0 ? K : 1; a.slab = 0;
  a.Abytes = clamp_bytes(K > 0 ? (long)(K - 1) * lda + M : 0);
  a.Bbytes = clamp_bytes(K > 0 ? (long)(K - 1) * ldb + N : 0);
  a.Cbytes = clamp_bytes(M > 0 ? (long)(M - 1) * ldc + N : 0);
  bool al = aligned16(A) && aligned16(B) && lda % 4 == 0 && ldb % 4 == 0 && M % 4 == 0 &&
            N % 4 == 0;
  return launch_gemm<MODE_WGRAD>(a, al, 1, stream);
}

