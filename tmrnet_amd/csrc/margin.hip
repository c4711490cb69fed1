// Black-margin cut of the reference's frame preparation (code/video2frame_cutmargin.py:20-48,
// change_size): grey -> threshold 15 -> 19x19 median -> bounding box of what is left in columns
// [10, w - 10), and the small job of "Training memory bank model/meanStd.py": exact per-frame
// channel sums.  All integer arithmetic on 8-bit pixels, so the contract is bit-exact
// (numpy emulation: tests/_margin_emu.py).
//
//   margin_pack_k    a wave packs 64 pixels of each of 4 rows (aligned dword loads, cross-lane reads):
//                    g = (9798 R + 19235 G + 3735 B + 16384) >> 15 (OpenCV 4's 8-bit RGB -> grey),
//                    m = g > 15, wave ballot -> one 64-bit word a row.  Bits at columns >= w are
//                    0.
//   margin_vote_k    one block per (frame, 64-row tile, 64-column word).  The median of a two-valued
//                    image is a majority vote: set iff >= 181 of the 361 window values are set,
//                    out-of-range indices clamped to the edge and counted with multiplicity.
//                    Separable: the words of the tile's 82 (clamped) rows go to LDS in one round
//                    of loads, the clamped 19-wide horizontal count of each row follows from three
//                    popcounts, then a sliding 19-row vertical sum.  Set pixels with
//                    10 <= column < w - 10 go into the block's row / column min / max (LDS
//                    atomicMin / atomicMax), stored in the block's own slot of the workspace.
//   margin_finish_k  one block per frame: min / max over the frame's slots and the fallbacks
//                    (nothing qualified, or an empty crop -> the full frame).
//   frame_sums_k     sum v and sum v^2 per frame and channel in 64-bit integers.
#include "common.h"
#include "tmr.h"

#include <limits.h>

namespace {

constexpr int NT = 256;
constexpr int kWin = 19, kHalf = 9;          // the median's window
constexpr int kVotes = (kWin * kWin + 1) / 2;   // 181 of 361
constexpr int kEdge = 10;                    // the reference scans columns [10, w - 10)
constexpr int kTileRows = 64;                // output rows per block of margin_vote_k
constexpr int kLdsRows = kTileRows + 2 * kHalf;
constexpr int kPackRows = 4;                 // rows a wave of margin_pack_k packs
static_assert(kLdsRows * 3 <= NT && kTileRows % (NT / 64) == 0, "margin_vote_k's tile");

__host__ __device__ inline int words_per_row(int w) { return (w + 63) >> 6; }

// grid (cdiv(wq, 4), min(cdiv(h, 4), 65535), n): wave k of a block takes word 4 * blockIdx.x + k.
// The 192 bytes of a wave's 64 pixels are read as the 48 or 49 aligned dwords that hold them (a
// row starts at any byte): lane i loads dword i, pixel lane j takes the two dwords around byte
// 3 j by cross-lane reads and shifts its 3 bytes out of the pair.  An aligned dword that holds a
// byte of the batch lies in that byte's page, so the first and the last dword may reach up to 3
// bytes outside the batch without touching memory the batch does not share a page with.
__global__ __launch_bounds__(NT) void margin_pack_k(const uint8_t* __restrict__ in, int h, int w,
                                                    long bytes,
                                                    unsigned long long* __restrict__ bits) {
  const int lane = threadIdx.x & 63;
  const int f = blockIdx.z;
  const int wq = words_per_row(w);
  const int q = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
  if (q >= wq) return;                       // wave-uniform
  const int x = q * 64 + lane;
  const uintptr_t end = (uintptr_t)in + (uintptr_t)bytes;
  for (int y0 = blockIdx.y * kPackRows; y0 < h; y0 += gridDim.y * kPackRows) {
    uint32_t dw[kPackRows];
    int sh[kPackRows];
#pragma unroll
    for (int r = 0; r < kPackRows; ++r) {
      const uintptr_t first = (uintptr_t)in + (uintptr_t)((((long)f * h + y0 + r) * w + q * 64) * 3);
      sh[r] = (int)(first & 3);
      const uintptr_t mine = (first & ~(uintptr_t)3) + 4 * (uintptr_t)lane;
      const bool ok = y0 + r < h && 4 * lane < sh[r] + 192 && mine < end;
      dw[r] = ok ? *reinterpret_cast<const uint32_t*>(mine) : 0u;
    }
    unsigned long long word = 0;
#pragma unroll
    for (int r = 0; r < kPackRows; ++r) {
      const int o = sh[r] + 3 * lane;        // first byte of this lane's pixel in the dword run
      const uint32_t d0 = (uint32_t)__shfl((int)dw[r], o >> 2, 64);
      const uint32_t d1 = (uint32_t)__shfl((int)dw[r], ((o >> 2) + 1) & 63, 64);
      const uint32_t p = (uint32_t)((((unsigned long long)d1 << 32) | d0) >> (8 * (o & 3)));
      const int g = (9798 * (int)(p & 255u) + 19235 * (int)((p >> 8) & 255u) +
                     3735 * (int)((p >> 16) & 255u) + 16384) >> 15;
      const unsigned long long b = __ballot(x < w && g > 15);
      if (lane == r) word = b;
    }
    if (lane < kPackRows && y0 + lane < h) bits[((long)f * h + y0 + lane) * wq + q] = word;
  }
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

// grid (wq, row tiles, n)
__global__ __launch_bounds__(NT) void margin_vote_k(const unsigned long long* __restrict__ bits,
                                                    int h, int w, int* __restrict__ mm,
                                                    uint8_t* __restrict__ mask) {
  __shared__ unsigned long long wd[kLdsRows][3];   // previous, own, next word of each row
  __shared__ uint8_t eb[kLdsRows][2];              // the row's first and last pixel
  __shared__ uint8_t hs[kLdsRows][64];             // horizontal counts
  __shared__ int red[4];                           // the block's [r0, r1, c0, c1]
  if (threadIdx.x < 4) red[threadIdx.x] = (threadIdx.x & 1) ? -1 : INT_MAX;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wq = words_per_row(w);
  const int q = blockIdx.x, f = blockIdx.z;
  const int y0 = blockIdx.y * kTileRows;
  const int x = q * 64 + lane;
  const unsigned long long* fb = bits + (long)f * h * wq;
  const int last = (w - 1) & 63;

  // rows y0 - 9 .. y0 + 72, clamped into the frame: the replicated border of the vertical pass
  if (threadIdx.x < kLdsRows * 3) {
    const int r = threadIdx.x / 3, k = threadIdx.x - 3 * r;
    const int y = min(max(y0 - kHalf + r, 0), h - 1);
    const int qi = q - 1 + k;
    wd[r][k] = (qi >= 0 && qi < wq) ? fb[(long)y * wq + qi] : 0ull;
  }
  if (threadIdx.x < kLdsRows * 2) {
    const int r = threadIdx.x >> 1, k = threadIdx.x & 1;
    const int y = min(max(y0 - kHalf + r, 0), h - 1);
    const unsigned long long v = fb[(long)y * wq + (k ? wq - 1 : 0)];
    eb[r][k] = (uint8_t)((v >> (k ? last : 0)) & 1ull);
  }

  // which bits of the previous / own / next word lie in [x - 9, x + 9]
  const int lo = max(lane - kHalf, 0), hi = min(lane + kHalf, 63);
  const unsigned long long mcur = (~0ull >> (63 - hi)) & (~0ull << lo);
  const unsigned long long mprev = lane < kHalf ? ~0ull << (64 - (kHalf - lane)) : 0ull;
  const unsigned long long mnext = lane > 63 - kHalf ? ~0ull >> (63 - (lane + kHalf - 64)) : 0ull;
  // replicated border: column 0 stands for x - 9 .. -1, column w - 1 for w .. x + 9
  const int nleft = max(kHalf - x, 0), nright = max(x + kHalf - (w - 1), 0);
  __syncthreads();

  for (int r = wave; r < kLdsRows; r += NT / 64) {
    const int c = __popcll(wd[r][1] & mcur) + __popcll(wd[r][0] & mprev) +
                  __popcll(wd[r][2] & mnext) + nleft * (int)eb[r][0] + nright * (int)eb[r][1];
    hs[r][lane] = (uint8_t)c;                // at most 19
  }
  __syncthreads();

  // wave v takes output rows y0 + 16 v .. y0 + 16 v + 15 of column x
  constexpr int kPer = kTileRows / (NT / 64);
  const int rbeg = wave * kPer;
  int s = 0;
#pragma unroll
  for (int k = 0; k < kWin; ++k) s += hs[rbeg + k][lane];
  int rmin = INT_MAX, rmax = -1;
  bool any = false;
  const bool admissible = x >= kEdge && x < w - kEdge;
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const int y = y0 + rbeg + k;
    if (y < h && x < w) {
      const bool v = s >= kVotes;
      if (mask) mask[((long)f * h + y) * w + x] = v ? 255 : 0;
      if (v && admissible) {
        rmin = min(rmin, y);
        rmax = y;
        any = true;
      }
    }
    if (k + 1 < kPer) s += (int)hs[rbeg + k + kWin][lane] - (int)hs[rbeg + k][lane];
  }
  if (mm == nullptr) return;                 // the debug entry: the mask alone
  // the block's min / max through LDS into the block's own slot: no address is shared between
  // blocks (every block of a frame hitting the frame's four cells kept one L2 channel busy for
  // longer than the rest of the kernel took)
  if (__any(any)) {                          // wave-uniform
    const int r0 = wave_min(rmin), r1 = wave_max(rmax);
    const int c0 = wave_min(any ? x : INT_MAX), c1 = wave_max(any ? x : -1);
    if (lane == 0) {
      atomicMin(&red[0], r0);
      atomicMax(&red[1], r1);
      atomicMin(&red[2], c0);
      atomicMax(&red[3], c1);
    }
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const long tile = ((long)f * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    mm[4 * tile + threadIdx.x] = red[threadIdx.x];
  }
}

// one block per frame: min / max over the frame's tiles, then the fallbacks
__global__ __launch_bounds__(NT) void margin_finish_k(const int* __restrict__ mm, int tiles, int h,
                                                      int w, int* __restrict__ boxes) {
  __shared__ int red[4];
  const int f = blockIdx.x;
  if (threadIdx.x < 4) red[threadIdx.x] = (threadIdx.x & 1) ? -1 : INT_MAX;
  __syncthreads();
  const int4* t = reinterpret_cast<const int4*>(mm) + (long)f * tiles;
  int r0 = INT_MAX, r1 = -1, c0 = INT_MAX, c1 = -1;
  for (int i = threadIdx.x; i < tiles; i += NT) {
    const int4 v = t[i];
    r0 = min(r0, v.x);
    r1 = max(r1, v.y);
    c0 = min(c0, v.z);
    c1 = max(c1, v.w);
  }
  r0 = wave_min(r0);
  r1 = wave_max(r1);
  c0 = wave_min(c0);
  c1 = wave_max(c1);
  if ((threadIdx.x & 63) == 0) {
    atomicMin(&red[0], r0);
    atomicMax(&red[1], r1);
    atomicMin(&red[2], c0);
    atomicMax(&red[3], c1);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    r0 = red[0]; r1 = red[1]; c0 = red[2]; c1 = red[3];
    if (r1 < 0 || r1 == r0 || c1 == c0) {    // nothing qualified, or the crop would be empty
      r0 = 0; r1 = h; c0 = 0; c1 = w;
    }
    boxes[4 * f] = r0;
    boxes[4 * f + 1] = r1;
    boxes[4 * f + 2] = c0;
    boxes[4 * f + 3] = c1;
  }
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// grid (blocks per frame, n); sums (n, 3, 2) zeroed by the launcher.  A frame's bytes are read as
// the aligned dwords that hold them (as margin_pack_k), 3 dwords = 4 pixel periods a thread and
// iteration: byte slot j of the 12 always carries the same channel for a thread, because its
// stride is a multiple of 3.
__global__ __launch_bounds__(NT) void frame_sums_k(const uint8_t* __restrict__ in, long pixels,
                                                   unsigned long long* __restrict__ sums) {
  __shared__ unsigned long long part[NT / 64][6];
  const uintptr_t lo = (uintptr_t)in + (uintptr_t)(blockIdx.y * pixels * 3);
  const uintptr_t hi = lo + (uintptr_t)(pixels * 3);
  const uintptr_t base = lo & ~(uintptr_t)3;
  const long t0 = blockIdx.x * (long)NT + threadIdx.x;
  const long ndw = (long)((hi - base + 3) >> 2);
  unsigned long long s[3] = {0, 0, 0}, sq[3] = {0, 0, 0};   // by byte slot mod 3
  for (long d = t0 * 3; d < ndw; d += (long)gridDim.x * NT * 3) {
    uint32_t v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
      v[k] = d + k < ndw ? *reinterpret_cast<const uint32_t*>(base + 4 * (uintptr_t)(d + k)) : 0u;
    unsigned ps[3] = {0, 0, 0}, pq[3] = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      const uintptr_t at = base + 4 * (uintptr_t)d + k;
      const unsigned b = (at >= lo && at < hi) ? (v[k >> 2] >> (8 * (k & 3))) & 255u : 0u;
      ps[k % 3] += b;
      pq[k % 3] += b * b;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      s[j] += ps[j];
      sq[j] += pq[j];
    }
  }
  // slot j holds channel (first byte's position in the frame + j) mod 3
  const long pos = (long)(base + 12 * (uintptr_t)t0) - (long)lo;   // >= -3
  const int rot = (int)((pos + 3) % 3);
  unsigned long long a[6];
#pragma unroll
  for (int c = 0; c < 3; ++c) {              // channel c sits in slot (c - rot) mod 3
    const int j0 = c, j1 = (c + 2) % 3, j2 = (c + 1) % 3;   // rot = 0, 1, 2
    a[2 * c] = rot == 0 ? s[j0] : (rot == 1 ? s[j1] : s[j2]);
    a[2 * c + 1] = rot == 0 ? sq[j0] : (rot == 1 ? sq[j1] : sq[j2]);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const unsigned long long t = wave_sum_u64(a[k]);
    if (lane == 0) part[wave][k] = t;
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    unsigned long long t = 0;
    for (int v = 0; v < NT / 64; ++v) t += part[v][threadIdx.x];
    atomicAdd(sums + blockIdx.y * 6 + threadIdx.x, t);
  }
}

// every host check of the margin entries; 0 when the launch may go ahead
int margin_check(const char* who, const void* in, int n, int h, int w, const void* ws,
                 size_t ws_bytes, const void* out) {
  TMR_CHECK_ARG(in && ws && out, "%s: null operand", who);
  TMR_CHECK_ARG(n > 0 && h > 0 && w > 0, "%s: bad shape n %d, h %d, w %d", who, n, h, w);
  TMR_CHECK_ARG((long)h * w <= INT_MAX / 4 && n <= 65535 && cdiv(h, kTileRows) <= 65535,
                "%s: %d frames of %d x %d exceed 32-bit indexing / the grid", who, n, h, w);
  const size_t need = tmr_margin_ws_bytes(n, h, w);
  TMR_CHECK_ARG(need > 0 && ws_bytes >= need, "%s: workspace of %zu bytes, %zu needed", who,
                ws_bytes, need);
  TMR_CHECK_ARG(((uintptr_t)ws & 15) == 0, "%s: workspace not 16-byte aligned", who);
  return 0;
}

int margin_run(const char* who, const uint8_t* in, int n, int h, int w, void* ws, int32_t* boxes,
               uint8_t* mask, hipStream_t stream) {
  const int wq = words_per_row(w);
  const int tiles = wq * cdiv(h, kTileRows);
  int* mm = (int*)ws;                                                 // (n, tiles, 4)
  unsigned long long* bits = (unsigned long long*)((char*)ws + (size_t)n * tiles * 16);   // (n, h, wq)
  int rows = cdiv(h, kPackRows);
  if (rows > 65535) rows = 65535;
  hipLaunchKernelGGL(margin_pack_k, dim3(cdiv(wq, NT / 64), rows, n), dim3(NT), 0, stream, in, h, w,
                     (long)n * h * w * 3, bits);
  TMR_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(margin_vote_k, dim3(wq, cdiv(h, kTileRows), n), dim3(NT), 0, stream, bits, h,
                     w, boxes ? mm : (int*)nullptr, mask);
  TMR_CHECK_LAUNCH(who);
  if (boxes) {
    hipLaunchKernelGGL(margin_finish_k, dim3(n), dim3(NT), 0, stream, mm, tiles, h, w,
                       (int*)boxes);
    TMR_CHECK_LAUNCH(who);
  }
  return 0;
}

}  // namespace

TMR_API size_t tmr_margin_ws_bytes(int n, int h, int w) {
  if (n <= 0 || h <= 0 || w <= 0) {
    tmr_set_error("tmr_margin_ws_bytes: bad shape n %d, h %d, w %d", n, h, w);
    return 0;
  }
  const size_t wq = words_per_row(w), tiles = wq * cdiv(h, kTileRows);
  return (size_t)n * tiles * 16 + (size_t)n * h * wq * 8;
}

TMR_API int tmr_margin_boxes(const uint8_t* in, int n, int h, int w, void* ws, size_t ws_bytes,
                             int32_t* boxes, hipStream_t stream) {
  if (int rc = margin_check("tmr_margin_boxes", in, n, h, w, ws, ws_bytes, boxes)) return rc;
  return margin_run("tmr_margin_boxes", in, n, h, w, ws, boxes, nullptr, stream);
}

TMR_API int tmr_margin_mask(const uint8_t* in, int n, int h, int w, void* ws, size_t ws_bytes,
                            uint8_t* mask, hipStream_t stream) {
  if (int rc = margin_check("tmr_margin_mask", in, n, h, w, ws, ws_bytes, mask)) return rc;
  return margin_run("tmr_margin_mask", in, n, h, w, ws, nullptr, mask, stream);
}

TMR_API int tmr_frame_sums(const uint8_t* in, int n, int h, int w, int64_t* sums,
                           hipStream_t stream) {
  TMR_CHECK_ARG(in && sums, "tmr_frame_sums: null operand");
  TMR_CHECK_ARG(n > 0 && h > 0 && w > 0 && n <= 65535, "tmr_frame_sums: bad shape n %d, h %d, w %d",
                n, h, w);
  const hipError_t e = hipMemsetAsync(sums, 0, (size_t)n * 6 * sizeof(int64_t), stream);
  TMR_CHECK_ARG(e == hipSuccess, "tmr_frame_sums: clearing the sums failed (%s)",
                hipGetErrorString(e));
  const long pixels = (long)h * w;
  // few blocks a frame: each ends in six atomic adds on the frame's sums
  long b = (pixels + NT * 64 - 1) / (NT * 64);
  if (b > 64) b = 64;
  hipLaunchKernelGGL(frame_sums_k, dim3((unsigned)b, n), dim3(NT), 0, stream, in, pixels,
                     (unsigned long long*)sums);
  TMR_CHECK_LAUNCH("tmr_frame_sums");
  return 0;
}
