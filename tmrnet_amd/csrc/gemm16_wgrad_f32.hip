// LDS-DMA engine (gemm16_kernel.h), WGRAD view, f32 form: one view x precision per translation unit.
#include "gemm16_kernel.h"

namespace tmrg {
template int launch_gemm16<MODE_WGRAD, 1>(const GemmArgs& a, int splits, hipStream_t st);

// The dY-producing form (gemm16_body's BNW; tmr_conv2d_wgrad_bnbwd): A = g, bn_y = y, bn_sc = the
// coefficients, Cold = the dY tensor to write.  The tile config is the plain wgrad's
// (pick_cfg16), so the caller's split plan holds; configs without the form are refused
// (wgrad_bnbwd_cfg: the caller asks first).
int launch_gemm16_wgrad_bnbwd(const GemmArgs& a, int splits, hipStream_t st) {
  TMR_CHECK_ARG(use16(a, MODE_WGRAD) && a.prec == TMR_MATH_F32,
                "wgrad_bnbwd: not an fp32 LDS-DMA wgrad");
  const int cfg = pick_cfg16(a.M, a.N, a.K, MODE_WGRAD, true);
  TMR_CHECK_ARG(wgrad_bnbwd_cfg(cfg), "wgrad_bnbwd: tile config %d has no dY-producing form", cfg);
  GemmArgs plain = a;   // the plain wgrad's checks (Cold is the dgrad epilogue's field there)
  plain.Cold = nullptr;
  if (const int rc = check16<MODE_WGRAD, 1>(plain, cfg)) return rc;
  TMR_CHECK_ARG(a.bn_y && a.bn_sc && a.Cold &&
                    ((((uintptr_t)a.bn_y | (uintptr_t)a.bn_sc | (uintptr_t)a.Cold)) & 15) == 0,
                "wgrad_bnbwd: y, coefficients and dy must be 16-B aligned");
  const Cfg16 c = kCfgs16[cfg];
  const dim3 grid(cdiv(a.M, c.bm) * cdiv(a.N, c.bn), splits, 1);
  if (grid.x == 0) return 0;
  switch (cfg) {
    case 4: hipLaunchKernelGGL((gemm16_wgrad_bnbwd_kernel<64, 256, 1, 4>), grid, dim3(256), 0, st, a); break;
    case 5: hipLaunchKernelGGL((gemm16_wgrad_bnbwd_kernel<64, 64, 2, 2>), grid, dim3(256), 0, st, a); break;
    case 6: hipLaunchKernelGGL((gemm16_wgrad_bnbwd16_kernel<256, 256, 4, 4>), grid, dim3(1024), 0, st, a); break;
    case 7: hipLaunchKernelGGL((gemm16_wgrad_bnbwd_kernel<128, 128, 4, 2>), grid, dim3(512), 0, st, a); break;
    default: break;
  }
  TMR_CHECK_LAUNCH("gemm16_wgrad_bnbwd_kernel");
  return 0;
}
}  // namespace tmrg
