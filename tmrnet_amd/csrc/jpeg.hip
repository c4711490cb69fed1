// Device half of the baseline JPEG decode (include/tmr.h, "baseline JPEG decode"): from the DCT
// coefficients that jpeg_host.cpp entropy-decodes to the packed RGB frame that pil_loader
// (train_only_non-local_pretrained.py:96-99) returns, bit for bit -- libjpeg-turbo's default
// decode as Pillow runs it: the "islow" integer IDCT, "fancy" (triangle) 4:2:0 upsampling and
// the 16-bit fixed-point YCbCr -> RGB tables.
//
// Stage A, idct_k: 8 lanes per block, lane r loads coefficient row r and quantiser row r as one
// 16-byte vector each; the column pass, the row pass and the transposes between them go through
// a padded LDS tile (row stride 9 words, block stride 72: by the index arithmetic a wave's 64
// lanes fall on 64 distinct words modulo 64 in every phase -- derived for 64 banks of 4 bytes,
// not measured with counters);
// lane r stores sample row r as 8 bytes into the component's uint8 plane (MCU-padded size).
// Stage B, rgb_k: 4 consecutive pixels of the flat (frame, y, x) order per lane -> three aligned
// 4-byte stores; chroma is upsampled on the fly from the real ceil(h/2) x ceil(w/2) plane with the
// edge rows / columns replicated.
//
// Arithmetic width.  |coef * q| <= 2^15 * 255 < 2^23 (q is held to its 8 bits).  A 1-D pass
// output is sum_k x_k * m_k with |m_k| < 2^14 (8192 * sqrt 2 * cos, the constants below), so the
// first pass is below 2^40 before its shift and below 2^29 after it: the passes run in 64 bit,
// the tile between them holds 32 bit.  The second pass is below 8 * 2^29 * 2^14 = 2^46.  Stage B
// sees bytes only: s <= 1020, upsampled <= 255, |116130 * 128| < 2^24: 32 bit.  A hostile stream
// therefore cannot overflow anything; it gets clamped samples where libjpeg's range table would
// wrap.
#include "common.h"
#include "tmr.h"

#include <limits.h>

namespace {

constexpr int NT = 256;
constexpr int kBlocksPerGroup = NT / 8;
constexpr int kTile = 72;   // words per block in LDS: 8 rows of stride 9

struct Geom {
  int bw[3], bh[3];     // block grid per component
  long plane_off[3];    // byte offset of a component's plane within a frame's workspace
  long blocks;          // blocks per frame
  long plane_bytes;     // workspace bytes per frame
  int ncomp;
};

bool make_geom(int h, int w, int sampling, Geom* g) {
  if (h <= 0 || w <= 0 || h > 65535 || w > 65535) return false;
  if (sampling != TMR_JPEG_GRAY && sampling != TMR_JPEG_444 && sampling != TMR_JPEG_420) return false;
  const int mcu = sampling == TMR_JPEG_420 ? 16 : 8;
  const int mw = (w + mcu - 1) / mcu, mh = (h + mcu - 1) / mcu;
  g->ncomp = sampling == TMR_JPEG_GRAY ? 1 : 3;
  g->blocks = 0;
  for (int c = 0; c < 3; ++c) {
    const int s = (c == 0 && sampling == TMR_JPEG_420) ? 2 : 1;
    g->bw[c] = c < g->ncomp ? mw * s : 0;
    g->bh[c] = c < g->ncomp ? mh * s : 0;
    g->plane_off[c] = g->blocks * 64;
    g->blocks += (long)g->bw[c] * g->bh[c];
  }
  g->plane_bytes = g->blocks * 64;
  return true;
}

// The 1-D "islow" pass (jidctint's 13-bit constants) on v[0..7] in place, outputs rounded by sh.
__device__ __forceinline__ void idct8(long long* v, int sh) {
  const long long i0 = v[0], i1 = v[1], i2 = v[2], i3 = v[3], i4 = v[4], i5 = v[5], i6 = v[6], i7 = v[7];
  long long z1 = (i2 + i6) * 4433;
  const long long t2 = z1 - i6 * 15137;
  const long long t3 = z1 + i2 * 6270;
  const long long t0 = (i0 + i4) * 8192;
  const long long t1 = (i0 - i4) * 8192;
  const long long t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  long long o0 = i7, o1 = i5, o2 = i3, o3 = i1;
  z1 = o0 + o3;
  long long z2 = o1 + o2, z3 = o0 + o2, z4 = o1 + o3;
  const long long z5 = (z3 + z4) * 9633;
  o0 *= 2446;
  o1 *= 16819;
  o2 *= 25172;
  o3 *= 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  o0 += z1 + z3;
  o1 += z2 + z4;
  o2 += z2 + z3;
  o3 += z1 + z4;
  const long long rnd = 1ll << (sh - 1);
  v[0] = (t10 + o3 + rnd) >> sh;
  v[1] = (t11 + o2 + rnd) >> sh;
  v[2] = (t12 + o1 + rnd) >> sh;
  v[3] = (t13 + o0 + rnd) >> sh;
  v[4] = (t13 - o0 + rnd) >> sh;
  v[5] = (t12 - o1 + rnd) >> sh;
  v[6] = (t11 - o2 + rnd) >> sh;
  v[7] = (t10 - o3 + rnd) >> sh;
}

typedef short shortx8 __attribute__((ext_vector_type(8)));
typedef unsigned short ushortx8 __attribute__((ext_vector_type(8)));

// coef (f, blocks, 64) int16, qt (f, 3, 64) uint16 -> ws (f, plane_bytes) uint8 planes
__global__ __launch_bounds__(NT) void idct_k(const int16_t* __restrict__ coef,
                                             const uint16_t* __restrict__ qt,
                                             uint8_t* __restrict__ ws, Geom g, long total_blocks) {
  __shared__ int tile[kBlocksPerGroup * kTile];
  const int lb = threadIdx.x >> 3, r = threadIdx.x & 7;
  const long gb = (long)blockIdx.x * kBlocksPerGroup + lb;
  const bool live = gb < total_blocks;   // the last group's spare lanes keep the barriers company
  int* t = tile + lb * kTile;
  long fr = 0;
  int comp = 0, by = 0, bx = 0;
  if (live) {
    fr = gb / g.blocks;
    long b = gb - fr * g.blocks;
    const long n0 = (long)g.bw[0] * g.bh[0], n1 = (long)g.bw[1] * g.bh[1];
    if (b >= n0 + n1) {
      comp = 2;
      b -= n0 + n1;
    } else if (b >= n0) {
      comp = 1;
      b -= n0;
    }
    by = (int)(b / g.bw[comp]);
    bx = (int)(b - (long)by * g.bw[comp]);
    const shortx8 c = *reinterpret_cast<const shortx8*>(coef + gb * 64 + r * 8);
    const ushortx8 q = *reinterpret_cast<const ushortx8*>(qt + (fr * 3 + comp) * 64 + r * 8);
#pragma unroll
    for (int k = 0; k < 8; ++k) t[r * 9 + k] = (int)c[k] * min((int)q[k], 255);   // 8-bit tables
  }
  __syncthreads();
  long long v[8];
  if (live) {   // columns: lane r owns column r
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = t[k * 9 + r];
    idct8(v, 11);
#pragma unroll
    for (int k = 0; k < 8; ++k) t[k * 9 + r] = (int)v[k];
  }
  __syncthreads();
  if (live) {   // rows: lane r owns row r
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = t[r * 9 + k];
    idct8(v, 18);
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      long long s = v[k] + 128;
      s = s < 0 ? 0 : (s > 255 ? 255 : s);
      if (k < 4) lo |= (uint32_t)s << (8 * k);
      else hi |= (uint32_t)s << (8 * (k - 4));
    }
    uint8_t* dst = ws + fr * g.plane_bytes + g.plane_off[comp] +
                   ((long)by * 8 + r) * ((long)g.bw[comp] * 8) + (long)bx * 8;
    *reinterpret_cast<uint2*>(dst) = make_uint2(lo, hi);
  }
}

__device__ __forceinline__ int clamp8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// "fancy" h2v2 upsample of one chroma plane at output pixel (y, x); ch x cw is the real plane
__device__ __forceinline__ int upsample420(const uint8_t* __restrict__ c, int pw, int ch, int cw,
                                           int y, int x) {
  const int r = y >> 1, cx = x >> 1;
  const int rn = (y & 1) ? min(r + 1, ch - 1) : max(r - 1, 0);
  const int xn = (x & 1) ? min(cx + 1, cw - 1) : max(cx - 1, 0);
  const uint8_t* a = c + (long)r * pw;
  const uint8_t* b = c + (long)rn * pw;
  const int s = 3 * a[cx] + b[cx], sn = 3 * a[xn] + b[xn];
  return (3 * s + sn + ((x & 1) ? 7 : 8)) >> 4;
}

// ws planes -> out (out_frames, h, w, 3); lane = 4 consecutive pixels of the flat frame order
template <int SAMPLING>
__global__ __launch_bounds__(NT) void rgb_k(const uint8_t* __restrict__ ws, uint8_t* __restrict__ out,
                                            const int32_t* __restrict__ out_index, int out_frames,
                                            int h, int w, Geom g, long total_px, bool aligned) {
  const long p0 = ((long)blockIdx.x * NT + threadIdx.x) * 4;
  if (p0 >= total_px) return;
  const long hw = (long)h * w;
  uint8_t rgb[12];
  long dst[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long p = p0 + j;
    dst[j] = -1;
    rgb[3 * j] = rgb[3 * j + 1] = rgb[3 * j + 2] = 0;
    if (p >= total_px) continue;
    const long fr = p / hw;
    const long q = p - fr * hw;
    const int y = (int)(q / w), x = (int)(q - (long)y * w);
    const int of = out_index ? out_index[fr] : (int)fr;
    if (of < 0 || of >= out_frames) continue;
    const uint8_t* base = ws + fr * g.plane_bytes;
    const int yy = base[(long)y * (g.bw[0] * 8) + x];
    int R = yy, G = yy, B = yy;
    if (SAMPLING != TMR_JPEG_GRAY) {
      const int pw = g.bw[1] * 8;
      int cb, cr;
      if (SAMPLING == TMR_JPEG_444) {
        cb = base[g.plane_off[1] + (long)y * pw + x];
        cr = base[g.plane_off[2] + (long)y * pw + x];
      } else {
        const int ch = (h + 1) >> 1, cw = (w + 1) >> 1;
        cb = upsample420(base + g.plane_off[1], pw, ch, cw, y, x);
        cr = upsample420(base + g.plane_off[2], pw, ch, cw, y, x);
      }
      cb -= 128;
      cr -= 128;
      R = clamp8(yy + ((91881 * cr + 32768) >> 16));
      G = clamp8(yy + ((-22554 * cb - 46802 * cr + 32768) >> 16));
      B = clamp8(yy + ((116130 * cb + 32768) >> 16));
    }
    rgb[3 * j] = (uint8_t)R;
    rgb[3 * j + 1] = (uint8_t)G;
    rgb[3 * j + 2] = (uint8_t)B;
    dst[j] = ((long)of * hw + q) * 3;
  }
  // four pixels of one frame, all present, on a 4-byte boundary: three word stores
  if (aligned && dst[0] >= 0 && dst[3] == dst[0] + 9 && dst[1] == dst[0] + 3 && dst[2] == dst[0] + 6 &&
      (dst[0] & 3) == 0) {
    uint32_t* d = reinterpret_cast<uint32_t*>(out + dst[0]);
#pragma unroll
    for (int k = 0; k < 3; ++k)
      d[k] = (uint32_t)rgb[4 * k] | ((uint32_t)rgb[4 * k + 1] << 8) | ((uint32_t)rgb[4 * k + 2] << 16) |
             ((uint32_t)rgb[4 * k + 3] << 24);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (dst[j] < 0) continue;
      out[dst[j]] = rgb[3 * j];
      out[dst[j] + 1] = rgb[3 * j + 1];
      out[dst[j] + 2] = rgb[3 * j + 2];
    }
  }
}

}  // namespace

TMR_API size_t tmr_jpeg_ws_bytes(int f, int h, int w, int sampling) {
  Geom g;
  if (f <= 0 || !make_geom(h, w, sampling, &g)) {
    tmr_set_error("tmr_jpeg_ws_bytes: bad shape f=%d h=%d w=%d sampling=%d", f, h, w, sampling);
    return 0;
  }
  return (size_t)f * (size_t)g.plane_bytes;
}

TMR_API int tmr_jpeg_reconstruct(const int16_t* coef, const uint16_t* qt, int f, int h, int w,
                                 int sampling, uint8_t* ws, size_t ws_bytes, uint8_t* out,
                                 const int32_t* out_index, int out_frames, hipStream_t stream) {
  Geom g;
  TMR_CHECK_ARG(f > 0 && out_frames > 0 && make_geom(h, w, sampling, &g),
                "tmr_jpeg_reconstruct: bad sizes f=%d h=%d w=%d sampling=%d out_frames=%d", f, h, w,
                sampling, out_frames);
  TMR_CHECK_ARG(coef && qt && ws && out, "tmr_jpeg_reconstruct: null operand");
  TMR_CHECK_ARG(out_index || f <= out_frames,
                "tmr_jpeg_reconstruct: %d frames into %d output frames without an index", f, out_frames);
  TMR_CHECK_ARG(ws_bytes >= (size_t)f * (size_t)g.plane_bytes,
                "tmr_jpeg_reconstruct: workspace of %zu bytes, %zu needed", ws_bytes,
                (size_t)f * (size_t)g.plane_bytes);
  TMR_CHECK_ARG(((uintptr_t)coef & 15) == 0 && ((uintptr_t)qt & 15) == 0 && ((uintptr_t)ws & 7) == 0,
                "tmr_jpeg_reconstruct: coef / qt must be 16-byte aligned, ws 8-byte aligned");
  const long total_blocks = (long)f * g.blocks;
  const long groups = (total_blocks + kBlocksPerGroup - 1) / kBlocksPerGroup;
  const long total_px = (long)f * h * w;
  const long px_groups = (total_px + 4L * NT - 1) / (4L * NT);
  TMR_CHECK_ARG(groups <= INT_MAX && px_groups <= INT_MAX, "tmr_jpeg_reconstruct: batch too large");
  hipLaunchKernelGGL(idct_k, dim3((unsigned)groups), dim3(NT), 0, stream, coef, qt, ws, g, total_blocks);
  TMR_CHECK_LAUNCH("tmr_jpeg_reconstruct (idct)");
  const bool aligned = ((uintptr_t)out & 3) == 0;
  const dim3 grid((unsigned)px_groups), block(NT);
  if (sampling == TMR_JPEG_GRAY)
    hipLaunchKernelGGL(rgb_k<TMR_JPEG_GRAY>, grid, block, 0, stream, ws, out, out_index, out_frames, h,
                       w, g, total_px, aligned);
  else if (sampling == TMR_JPEG_444)
    hipLaunchKernelGGL(rgb_k<TMR_JPEG_444>, grid, block, 0, stream, ws, out, out_index, out_frames, h,
                       w, g, total_px, aligned);
  else
    hipLaunchKernelGGL(rgb_k<TMR_JPEG_420>, grid, block, 0, stream, ws, out, out_index, out_frames, h,
                       w, g, total_px, aligned);
  TMR_CHECK_LAUNCH("tmr_jpeg_reconstruct (rgb)");
  return 0;
}
