// LDS-DMA engine (gemm16_kernel.h), FWD view, fp32 form with the inference epilogue that also
// writes a bf16 copy of its output (epilogue_batched INF16 = 2: fp32 residual in, fp32 z out, and
// bf16(z), rounded once, into GemmArgs::Cbf; tmr_conv2d_fwd_fused_dual).  A translation unit of
// its own: the fp32 forwards of gemm16_fwd_f32.hip keep their instantiations.
#include "gemm16_kernel.h"

namespace tmrg {

template <int BM, int BN, int WM, int WN, int TAPV>
__global__ __launch_bounds__(64 * WM * WN, (occ16<BM, BN, WM, WN, 2>()))
void gemm16_dual32_kernel(const GemmArgs a) {
  int bid, split;
  xcd_work(bid, split);   // XCD-aware tile order (gemm_kernel.h)
  gemm16_body<MODE_FWD, BM, BN, WM, WN, TAPV, 1, 1, 2, 0, 2>(a, bid, split);
}

// The launch forms are launch16_cfg's for an fp32 forward: the TAPV form for k-tiles spanning
// taps, else the two-stage form (the fp32 forwards have no one-stage form) -- the accumulators
// are those of the same tile's plain fp32 forward, bit for bit.
template <int BM, int BN, int WM, int WN>
int launch16_dual32(const GemmArgs& a, bool tapv, dim3 grid, hipStream_t st) {
  const dim3 blk(64 * WM * WN);
  if (tapv)
    hipLaunchKernelGGL((gemm16_dual32_kernel<BM, BN, WM, WN, 1>), grid, blk, 0, st, a);
  else
    hipLaunchKernelGGL((gemm16_dual32_kernel<BM, BN, WM, WN, 0>), grid, blk, 0, st, a);
  TMR_CHECK_LAUNCH("gemm16_dual32_kernel");
  return 0;
}

// the tile configs pick_cfg16 gives an fp32 forward: 1, 2, 3, 7, 5, 6 (dual32_cfg)
template int launch16_dual32<256, 128, 4, 2>(const GemmArgs&, bool, dim3, hipStream_t);
template int launch16_dual32<128, 128, 2, 2>(const GemmArgs&, bool, dim3, hipStream_t);
template int launch16_dual32<256, 64, 4, 1>(const GemmArgs&, bool, dim3, hipStream_t);
template int launch16_dual32<128, 128, 4, 2>(const GemmArgs&, bool, dim3, hipStream_t);
template int launch16_dual32<64, 64, 2, 2>(const GemmArgs&, bool, dim3, hipStream_t);
template int launch16_dual32<256, 256, 4, 4>(const GemmArgs&, bool, dim3, hipStream_t);

}  // namespace tmrg
