// What the conv host layer (gemm_conv.hip) needs from a family of direct convolution kernels, in
// terms of tmr_conv_desc.  A family serves up to three views of a conv; per view it says whether it
// serves a descriptor, how much the caller must provide (partial rows, workspace), and runs it.
//
// To add a family: in the kernels' translation unit write the view's `serves` predicate next to
// the constants it depends on (grid, LDS row widths, shape lists), the size query and `run` on the
// descriptor, and define one `const DirectConv& tmr_direct_<name>()`; declare it at the bottom of
// this file and append it to kDirect in gemm_conv.hip.  A view left {} is not served.  Nothing
// else in gemm_conv.hip changes: TMR_IO_ENGINE (tests: the engine everywhere) is handled at its
// lookup, so a predicate never sees that bit, and no number of a kernel is named outside its own
// file.  Add the family's rows to tests/test_conv_plan_cpu.py: a routing slip is silent elsewhere.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "tmr.h"

static inline int xld_of(const tmr_conv_desc* d) { return d->x_ld ? d->x_ld : d->c; }
static inline int yld_of(const tmr_conv_desc* d) { return d->y_ld ? d->y_ld : d->k; }
static inline int ngroups(const tmr_conv_desc* d) { return d->groups > 1 ? d->groups : 1; }

// The 7x7/2 stem conv on the NHWC4 input, 3 (4 stored) -> 64 channels, dense, ungrouped: the shape
// of both stem families (stem.hip, stem16.hip); they differ in math, io and the widest input row.
static inline bool stem7_shape(const tmr_conv_desc* d) {
  return ngroups(d) == 1 && d->c == 4 && d->k == 64 && d->r == 7 && d->s == 7 && d->stride == 2 &&
         d->pad == 3 && d->pad_w == 3 && xld_of(d) == 4 && yld_of(d) == 64 &&
         d->ho == (d->h + 6 - 7) / 2 + 1 && d->wo == (d->w + 6 - 7) / 2 + 1;
}

// The partial slabs a direct wgrad left in the workspace: n slabs of elems floats, each
// (k, taps, cstored) -- what wgrad_reduce_taps_kernel sums into the OIHW gradient.
struct DirectSlabs {
  int n;
  long elems;
  int taps, cstored;
};

struct DirectConv {
  // forward + BatchNorm statistics (tmr_conv2d_fwd_bnstats): parts = partial statistics rows
  struct Fwd {
    bool (*serves)(const tmr_conv_desc* d);
    int (*parts)(const tmr_conv_desc* d);
    int (*run)(const tmr_conv_desc* d, const void* x, const void* w_krsc, void* y, void* stats,
               hipStream_t stream);
  } fwd;
  // dgrad + fused BatchNorm backward (tmr_conv2d_dgrad_bnbwd): parts = partial (sum, dot) rows
  struct Dgrad {
    bool (*serves)(const tmr_conv_desc* d);
    int (*parts)(const tmr_conv_desc* d);
    int (*run)(const tmr_conv_desc* d, const void* dy, const void* w_crsk, void* dx, float beta,
               const void* y, const void* z, const float* scale, const float* shift,
               const float* mean, int mask, void* parts, hipStream_t stream);
  } dgrad;
  // wgrad: partial slabs into the workspace (the caller reduces them); c_real = the real input
  // channels the kernel computes (0: any number up to c)
  struct Wgrad {
    bool (*serves)(const tmr_conv_desc* d);
    int c_real;
    size_t (*ws_bytes)(const tmr_conv_desc* d);
    int (*run)(const tmr_conv_desc* d, const void* x, const void* dy, float* ws, size_t ws_bytes,
               DirectSlabs* slabs, hipStream_t stream);
  } wgrad;
};

// (functions, not objects: a const object would be emitted into the device code as well)
const DirectConv& tmr_direct_stem();     // stem.hip: the fp32 7x7/2 stem
const DirectConv& tmr_direct_stem16();   // stem16.hip: the bf16 7x7/2 stem
const DirectConv& tmr_direct_d3();       // direct3.hip: the narrow stride-1 3x3 convs
const DirectConv& tmr_direct_d3s();      // direct3.hip: the deep stem's 3x3/2 conv
