// LDS-DMA engine (gemm16_kernel.h), FWD view, bf16 form with the bf16-activation inference
// epilogue (epilogue_batched INF16: bf16 residual in, one RNE rounding, bf16 y out).  A translation
// unit of its own: the train step's kernels (gemm16_fwd_bf16.hip) keep their instantiations.
#include "gemm16_kernel.h"

namespace tmrg {

template <int BM, int BN, int WM, int WN, int TAPV, int NST>
__global__ __launch_bounds__(64 * WM * WN, (occ16<BM, BN, WM, WN, NST>()))
void gemm16_inf16_kernel(const GemmArgs a) {
  int bid, split;
  xcd_work(bid, split);   // XCD-aware tile order (gemm_kernel.h)
  gemm16_body<MODE_FWD, BM, BN, WM, WN, TAPV, 1, 0, NST, 0, 1>(a, bid, split);
}

// The launch forms are launch16_cfg's for a bf16 forward, in the same order: the
// one-stage form of the 4-wave 128x128 / 256x64 tiles and of 256x256 (as 256x128, 8 waves) for one
// k-tile, the TAPV form for k-tiles spanning taps, else the two-stage form.
template <int BM, int BN, int WM, int WN>
int launch16_inf16(const GemmArgs& a, bool tapv, dim3 grid, hipStream_t st) {
  const dim3 blk(64 * WM * WN);
  constexpr int kmax = 64;
  if constexpr (WM * WN == 4 && ((BM == 128 && BN == 128) || (BM == 256 && BN == 64))) {
    if (!tapv && a.K > 0 && a.K <= kmax) {
      hipLaunchKernelGGL((gemm16_inf16_kernel<BM, BN, WM, WN, 0, 1>), grid, blk, 0, st, a);
      TMR_CHECK_LAUNCH("gemm16_inf16_kernel (one stage)");
      return 0;
    }
  }
  if constexpr (BM == 256 && BN == 256) {
    if (!tapv && a.K > 0 && a.K <= kmax) {
      const dim3 g2((unsigned)(cdiv(a.M, 256) * cdiv(a.N, 128)), grid.y, 1);
      hipLaunchKernelGGL((gemm16_inf16_kernel<256, 128, 4, 2, 0, 1>), g2, dim3(512), 0, st, a);
      TMR_CHECK_LAUNCH("gemm16_inf16_kernel (one stage, 256x128)");
      return 0;
    }
  }
  if (tapv)
    hipLaunchKernelGGL((gemm16_inf16_kernel<BM, BN, WM, WN, 1, 2>), grid, blk, 0, st, a);
  else
    hipLaunchKernelGGL((gemm16_inf16_kernel<BM, BN, WM, WN, 0, 2>), grid, blk, 0, st, a);
  TMR_CHECK_LAUNCH("gemm16_inf16_kernel");
  return 0;
}

template int launch16_inf16<256, 128, 4, 2>(const GemmArgs&, bool, dim3, hipStream_t);
template int launch16_inf16<128, 128, 2, 2>(const GemmArgs&, bool, dim3, hipStream_t);
template int launch16_inf16<256, 64, 4, 1>(const GemmArgs&, bool, dim3, hipStream_t);
template int launch16_inf16<64, 256, 1, 4>(const GemmArgs&, bool, dim3, hipStream_t);
template int launch16_inf16<128, 128, 4, 2>(const GemmArgs&, bool, dim3, hipStream_t);
template int launch16_inf16<64, 64, 2, 2>(const GemmArgs&, bool, dim3, hipStream_t);
template int launch16_inf16<256, 256, 2, 4>(const GemmArgs&, bool, dim3, hipStream_t);
template int launch16_inf16<256, 256, 4, 4>(const GemmArgs&, bool, dim3, hipStream_t);

}  // namespace tmrg
