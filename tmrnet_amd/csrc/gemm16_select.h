// Host-side launch selection of the LDS-DMA implicit-GEMM engine (gemm16_kernel.h): eligibility
// per view, tile rules, and the per-(view, precision) launchers instantiated in
// gemm16_<view>_<prec>.hip.  The register-staged translation units include only this header, so
// an edit of the engine rebuilds the six small engine units and nothing else.
#pragma once
#include "gemm_kernel.h"

namespace tmrg {

// ---------------------------------------------------------------- launch selection
struct Cfg16 { int bm, bn, waves; };   // (waves: checked against launch16_switch's instantiations)
constexpr Cfg16 kCfgs16[] = {{256, 256, 8}, {256, 128, 8}, {128, 128, 4}, {256, 64, 4},
                              {64, 256, 4}, {64, 64, 4},
                              {256, 256, 16},    // 6: 256x256 as 16 waves (4x4, 64x64 per wave)
                              {128, 128, 8}};    // 7: 128x128 as 8 waves (4x2, 32x64 per wave)

// Eligibility: bf16 math, every operand bf16 in HBM (sab 3; DGRAD with the transposed weights),
// 16-B pieces of 8 channels (channels per tap, row strides multiples of 8).
// fp32 form (GemmArgs::dma32, set by the conv entry points): FWD with every operand fp32 and
// 16-B aligned, 4-channel pieces; DGRAD whenever the weights come transposed (wt: the engine is
// the only reader of that layout, so eligibility is checked again by launch_gemm16_t).
inline bool use32(const GemmArgs& a, int mode) {
  if (a.prec != TMR_MATH_F32 || a.sab) return false;
  if (mode == MODE_DGRAD) return a.wt != 0;
  if (!a.dma32) return false;
  if ((((uintptr_t)a.A | (uintptr_t)a.B) & 15) != 0) return false;
  if (mode == MODE_WGRAD)
    return a.M % 4 == 0 && a.log2C >= 2 && a.ldb % 4 == 0 && a.lds % 4 == 0 && a.N % 4 == 0;
  return a.lds % 4 == 0 && a.ldb % 4 == 0 && a.log2C >= 2 && (a.ntaps != 1 || a.K % 4 == 0);
}

inline bool use16(const GemmArgs& a, int mode) {
  if (a.prec == TMR_MATH_F32) return use32(a, mode);
  if (a.prec != TMR_MATH_BF16 || a.sab != 3) return false;
  if (mode == MODE_DGRAD && !a.wt) return false;
  if (a.lds % 8) return false;
  if (mode == MODE_WGRAD) return a.M % 8 == 0 && a.log2C >= 3 && a.ldb % 8 == 0 && a.N % 8 == 0;
  if (mode == MODE_FWD && a.ldb % 8) return false;
  if (mode == MODE_DGRAD && a.ldbt % 8) return false;
  return a.ntaps == 1 ? (a.K % 8 == 0 && (mode == MODE_FWD || a.log2C >= 3)) : a.log2C >= 3;
}

inline long cfg16_tiles(long M, long N, int c) {
  return ((M + kCfgs16[c].bm - 1) / kCfgs16[c].bm) * ((N + kCfgs16[c].bn - 1) / kCfgs16[c].bn);
}

// Tile choice per view, from scripts/convbench.py --io16 --stats --bnbwd with each config forced
// over the 23 ResNet-50 conv shapes x 3 views (profiles/r2/convbench16_cfgs/, cb16c/): 256x256
// pays for the forwards and the wgrads with 256-512 output channels, as 16 waves (four per SIMD:
// 5-20% over 8 waves, whose two waves per SIMD stall on the same barrier); the dgrads, whose
// fused BatchNorm-backward epilogue moves 12-16 B per output element, want the occupancy of
// 128x128 / 256x64 tiles.
// fp32 (f32): measured separately (profiles/r2/convbench32_dma_cfgs/, wgrad32_cfgs/): the
// wgrads with 64 output channels want 64-wide tiles, the big-FLOP wgrads (>= 100 GFLOP: 3x3,
// strided downsample) 256x256 as 16 waves, the rest 128x128 as 8 waves; the N = 128 forwards and
// the >= 512-column dgrads 128x128 as 8 waves.
inline int pick_cfg16(long M, long N, long K, int mode, bool f32 = false) {
  static const int forced = env_int("TMR_GEMM16_CFG", -1);   // experiments only
  if (forced >= 0 && forced < (int)(sizeof(kCfgs16) / sizeof(kCfgs16[0]))) return forced;
  int cfg;
  if (f32 && mode == MODE_WGRAD) {
    if (M <= 64) return (N <= 64 || N >= 512) ? 5 : 4;
    if (N <= 64) return 5;
    if (M >= 256 && N >= 256 && 2.0 * M * N * K >= 100e9) return 6;
    return 7;
  }
  if (f32 && M >= 256 && mode == MODE_DGRAD && N >= 512) {
    static const int wide = env_int("TMR_DGRAD32_WIDE_CFG", 7);   // A/B of this rule
    return cfg16_tiles(M, N, wide) >= 256 ? wide : 2;
  }
  if (f32 && M >= 256 && mode == MODE_FWD && N == 128)
    return cfg16_tiles(M, N, 7) >= 256 ? 7 : 2;
  if (mode == MODE_WGRAD) {
    if (M <= 64) cfg = N <= 64 ? 5 : (N >= 512 ? 4 : 2);
    else if (N <= 64) cfg = 3;
    // round 5 (profiles/r5/tile_rules/): 128x128 as 8 waves, or 256x256 as 16 waves for the wide
    // wgrads (N >= 1024: 3x3, 1024-channel inputs) while each of the ~512 / tiles split-K slices
    // still reduces >= 4096 rows; shorter slices (layer3/4 spatial at 640 frames, the grouped
    // split-attention convs one group at a time) spend the 256x256 tile's time on its prologue and
    // its 256 KB slab.  Replaced the round-2 rule (128x128 4-wave / 256x256 by M and K): C5 wgrads
    // -1.1 ms, C4 -0.4 ms per step.
    else cfg = (M >= 256 && N >= 1024 && K * cfg16_tiles(M, N, 6) >= (1L << 21)) ? 6 : 7;
  } else if (N <= 64) {
    cfg = M >= 256 ? 3 : 5;
  } else if (mode == MODE_FWD && N >= 256 && M >= 256) {
    cfg = 6;   // 256x256 as 16 waves: four waves per SIMD hide the barrier / load waits
  } else {
    cfg = 2;
  }
  // too few tiles to fill the 256 CUs: smaller tiles -- except the fp32 256x256 forwards at >= 224
  // tiles (layer4 at 640 frames: 246), which measured 4-6% faster than 492 256x128 tiles (round 5)
  if (mode != MODE_WGRAD && cfg16_tiles(M, N, cfg) < (f32 && cfg == 6 ? 224 : 256)) {
    for (const int c2 : {1, 2, 5}) {
      if ((long)kCfgs16[c2].bm * kCfgs16[c2].bn >= (long)kCfgs16[cfg].bm * kCfgs16[cfg].bn ||
          cfg16_tiles(M, N, c2) <= cfg16_tiles(M, N, cfg))
        continue;
      cfg = c2;
      if (cfg16_tiles(M, N, cfg) >= 256) break;
    }
  }
  return cfg;
}

// a k-tile (64 bf16 / 32 fp32) spans several taps when the channels per tap are fewer (or not a
// multiple): the TAPV kernel form of launch_gemm16_t
inline bool tapv16(const GemmArgs& a, int mode, bool f32) {
  const int bk = f32 ? 32 : 64;
  return mode != MODE_WGRAD && a.ntaps > 1 && ((1 << a.log2C) % bk) != 0;
}

// rows / columns of the output tile the launch for `a` will use (host planning: BN-partial rows,
// wgrad split counts)
inline int gemm_tile_bm(const GemmArgs& a, int mode) {
  return use16(a, mode) ? kCfgs16[pick_cfg16(a.M, a.N, a.K, mode, a.prec == TMR_MATH_F32)].bm
                        : kCfgs[pick_cfg(a.M, a.N, a.K, mode)].bm;
}
inline long gemm_tiles(const GemmArgs& a, int mode) {
  return use16(a, mode) ? cfg16_tiles(a.M, a.N, pick_cfg16(a.M, a.N, a.K, mode, a.prec == TMR_MATH_F32))
                        : cfg_tiles(a.M, a.N, pick_cfg(a.M, a.N, a.K, mode));
}

// the stride-parity classes of one strided dgrad as one launch (launch_gemm16_par): the
// arguments every class shares once, the few that differ per class in a table
constexpr int PAR_MAX = 4;
struct ParClass {
  int M, K, ntaps, tapS, tapSinv, oy0, ox0, wr0, ws0, oyc, oxc, tiles;
  FastDiv dHW, dW;
  float2* bn_part;
};
struct GemmPar {
  GemmArgs a;               // the first class's arguments
  ParClass c[PAR_MAX];      // by tile count, largest first
  int n;
};
// tiles of one class in a row (par_tile): a round of one XCD's workgroup slots (32 CUs x 2)
constexpr int PAR_G = 64;

// wave-specialised dgrad launches so far (gemm16_ws.h; tmr_dgrad_ws_launches)
extern long g_dgrad_ws_launches;

// one view x precision per translation unit (gemm16_<view>_<prec>.hip, explicit instantiations:
// they compile in parallel)
template <int F32>
int launch_gemm16_par(const GemmArgs* as, int n, hipStream_t st);
extern template int launch_gemm16_par<0>(const GemmArgs*, int, hipStream_t);
extern template int launch_gemm16_par<1>(const GemmArgs*, int, hipStream_t);
template <int MODE, int F32>
int launch_gemm16(const GemmArgs& a, int splits, hipStream_t st);
extern template int launch_gemm16<MODE_FWD, 0>(const GemmArgs&, int, hipStream_t);
extern template int launch_gemm16<MODE_FWD, 1>(const GemmArgs&, int, hipStream_t);
extern template int launch_gemm16<MODE_DGRAD, 0>(const GemmArgs&, int, hipStream_t);
extern template int launch_gemm16<MODE_DGRAD, 1>(const GemmArgs&, int, hipStream_t);
extern template int launch_gemm16<MODE_WGRAD, 0>(const GemmArgs&, int, hipStream_t);
extern template int launch_gemm16<MODE_WGRAD, 1>(const GemmArgs&, int, hipStream_t);

// The fp32 wgrad that produces its dY operand from (g, y, BN-backward coefficients) while loading
// it (tmr_conv2d_wgrad_bnbwd; gemm16_kernel.h BNW, gemm16_wgrad_f32.hip): the tile configs that
// have the form -- 64x64, 64x256, 128x128 as 8 waves, and 256x256 as 16 waves in a form of its own
// (118 of 128 VGPRs as a plain wgrad: coefficients in LDS, nothing held across the barrier;
// profiles/wgrad_bnbwd_ds/).
inline bool wgrad_bnbwd_cfg(int cfg) { return cfg == 4 || cfg == 5 || cfg == 6 || cfg == 7; }
int launch_gemm16_wgrad_bnbwd(const GemmArgs& a, int splits, hipStream_t st);
// fused launches so far (tmr_wgrad_bnbwd_launches)
extern long g_wgrad_bnbwd_launches;

// the bf16-activation inference forwards (tmr_conv2d_fwd_fused with TMR_IO_Y_BF16: bf16 residual
// and y, epilogue_batched's INF16 form) of one tile config, in the launch form (one-stage, TAPV)
// the same tile's other bf16 forwards take -- their accumulators are bit-identical.  Kernels of
// their own (gemm16_fwd_inf16.hip): the train step's instantiations are not touched.
template <int BM, int BN, int WM, int WN>
int launch16_inf16(const GemmArgs& a, bool tapv, dim3 grid, hipStream_t st);
extern template int launch16_inf16<256, 128, 4, 2>(const GemmArgs&, bool, dim3, hipStream_t);
extern template int launch16_inf16<128, 128, 2, 2>(const GemmArgs&, bool, dim3, hipStream_t);
extern template int launch16_inf16<256, 64, 4, 1>(const GemmArgs&, bool, dim3, hipStream_t);
extern template int launch16_inf16<64, 256, 1, 4>(const GemmArgs&, bool, dim3, hipStream_t);
extern template int launch16_inf16<128, 128, 4, 2>(const GemmArgs&, bool, dim3, hipStream_t);
extern template int launch16_inf16<64, 64, 2, 2>(const GemmArgs&, bool, dim3, hipStream_t);
extern template int launch16_inf16<256, 256, 2, 4>(const GemmArgs&, bool, dim3, hipStream_t);
extern template int launch16_inf16<256, 256, 4, 4>(const GemmArgs&, bool, dim3, hipStream_t);

// the fp32 inference forwards that also write a bf16 copy of their output
// (tmr_conv2d_fwd_fused_dual: GemmArgs::Cbf, epilogue_batched's INF16 = 2 form), in the launch
// form (two-stage, TAPV) the same tile's other fp32 forwards take.  Kernels of their own
// (gemm16_fwd_dual32.hip), for the tile configs pick_cfg16 gives an fp32 forward; a forced config
// outside them (TMR_GEMM16_CFG 0 / 4) is refused.
template <int BM, int BN, int WM, int WN>
constexpr bool dual32_cfg() {
  return !((BM == 256 && BN == 256 && WM * WN == 8) || (BM == 64 && BN == 256));
}
template <int BM, int BN, int WM, int WN>
int launch16_dual32(const GemmArgs& a, bool tapv, dim3 grid, hipStream_t st);
extern template int launch16_dual32<256, 128, 4, 2>(const GemmArgs&, bool, dim3, hipStream_t);
extern template int launch16_dual32<128, 128, 2, 2>(const GemmArgs&, bool, dim3, hipStream_t);
extern template int launch16_dual32<256, 64, 4, 1>(const GemmArgs&, bool, dim3, hipStream_t);
extern template int launch16_dual32<128, 128, 4, 2>(const GemmArgs&, bool, dim3, hipStream_t);
extern template int launch16_dual32<64, 64, 2, 2>(const GemmArgs&, bool, dim3, hipStream_t);
extern template int launch16_dual32<256, 256, 4, 4>(const GemmArgs&, bool, dim3, hipStream_t);

}  // namespace tmrg
