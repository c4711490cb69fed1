// Entropy decode of baseline JPEG scans on the device (include/tmr.h, "Entropy decode on the
// device"): from the packed scans of tmr_jpeg_scan_pack (jpeg_host.cpp) to DCT coefficients in
// exactly the layout tmr_jpeg_entropy_decode writes, so tmr_jpeg_reconstruct (jpeg.hip) takes
// them unchanged.  The per-symbol step and the per-subsequence passes are jpeg_entropy.h, which
// tests/jpeg_entropy_main.cpp runs serially on the host.
//
// Huffman decoding is serial, but self-synchronising: a decoder started at a wrong bit soon falls
// into step with the true symbol sequence.  One workgroup decodes one frame; its lanes stride
// over the frame's subsequences of sub_bits bits.
//   1. Every lane decodes its subsequences from their first bit as "start of a block, slot 0" and
//      records the state (bit, slot, k) with which it crosses into the next one.
//   2. Rounds: a subsequence whose predecessor's end state differs from the start state it last
//      used decodes again from that state.  Subsequence 0 starts from the true state, so after
//      round r subsequences 0..r are exact; the loop runs until a round changes nothing, at most
//      as many rounds as the frame has subsequences -- it always ends exact.
//   3. An exclusive sum of the blocks begun per subsequence gives each its block ordinal in scan
//      order.
//   4. Write pass from the (now true) start states into the zero-filled frame, the DC entry
//      holding the difference; errors in blocks the frame has set the status.
//   5. Per component, an inclusive sum of the DC differences in scan order, modulo 2^16 as the
//      host's predictor wraps.
// All synchronisation is __syncthreads in loops whose trip counts are uniform over the workgroup;
// there is no inter-workgroup protocol.  The tables sit in LDS; the per-subsequence states sit in
// the workspace for every frame (five words per subsequence, touched once per round next to a
// decode of sub_bits bits -- one code path whatever the frame's size).
//
// Bounds.  The geometry comes from the host-checked arguments, never from the descriptor; a
// descriptor that disagrees with it, or whose offsets, sizes or table indices leave the batch
// buffer or the workspace, gets status 3 and nothing of it is read further.  Bit fetches are
// checked against nbits (je::peek32), coefficient stores against the frame's block count
// (je::write_sub), loop counts derive from nbits <= max_bits.
#include "common.h"
#include "jpeg_entropy.h"

#include <limits.h>

namespace {

constexpr int NT = 1024;
constexpr int kStateWords = 5;   // per subsequence: start p, start sk, end p, end sk, count / ordinal

__constant__ uint8_t kZigzagDev[64] = JE_ZIGZAG;

// Inclusive sum of v over the workgroup's threads (by thread index); scratch holds NT words.
__device__ inline uint32_t block_scan(uint32_t v, uint32_t* scratch) {
  const int t = threadIdx.x;
  scratch[t] = v;
  __syncthreads();
  for (int d = 1; d < NT; d <<= 1) {
    const uint32_t add = t >= d ? scratch[t - d] : 0;
    __syncthreads();
    scratch[t] += add;
    __syncthreads();
  }
  const uint32_t r = scratch[t];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(NT) void entropy_k(const tmr_jpeg_scan_desc* __restrict__ desc,
                                                 const uint8_t* __restrict__ buf, size_t buf_bytes,
                                                 je::Geom g, int h, int w, int sampling,
                                                 uint32_t max_bits, uint32_t sub, uint32_t nsub_max,
                                                 int16_t* coef, int32_t* status, uint32_t* rounds,
                                                 uint32_t* states) {
  __shared__ tmr_jpeg_huff tabs[TMR_JPEG_MAX_TABLES];
  __shared__ uint32_t scratch[NT];
  __shared__ uint8_t zigzag[64];
  __shared__ int s_err, s_done;

  const int t = threadIdx.x;
  const uint32_t frame = blockIdx.x;
  const tmr_jpeg_scan_desc d = desc[frame];

  // the descriptor against the host-checked arguments; uniform, before any barrier
  bool ok = d.nbits <= max_bits && (d.nbits & 7) == 0 && d.ntables >= 1 &&
            d.ntables <= TMR_JPEG_MAX_TABLES && (d.bits_off & 15) == 0 && (d.tables_off & 15) == 0 &&
            d.bits_bytes >= TMR_JPEG_SCAN_CAP(d.nbits / 8) && d.bits_off <= buf_bytes &&
            d.bits_bytes <= buf_bytes - d.bits_off && d.tables_off <= buf_bytes &&
            (size_t)d.ntables * sizeof(tmr_jpeg_huff) <= buf_bytes - d.tables_off;
  ok = ok && d.height == h && d.width == w && d.sampling == sampling && d.ncomp == g.ncomp &&
       d.mcu_blocks == g.nslots && d.blocks_w[0] == g.bw0 && d.blocks_h[0] == g.bh0;
  uint32_t dcsel = 0, acsel = 0;
  for (int c = 0; c < 3; ++c) {
    if (c >= g.ncomp) continue;
    ok = ok && d.dc_table[c] < d.ntables && d.ac_table[c] < d.ntables;
    if (c) ok = ok && d.blocks_w[c] == g.bw1 && d.blocks_h[c] == g.bh1;
    dcsel |= (uint32_t)d.dc_table[c] << (8 * c);
    acsel |= (uint32_t)d.ac_table[c] << (8 * c);
  }
  if (!ok) {
    if (t == 0) status[frame] = 3;
    return;
  }

  const uint32_t nbits = d.nbits;
  const uint32_t nsub = nbits ? (nbits + sub - 1) / sub : 1;   // <= nsub_max: nbits <= max_bits
  uint32_t* sp = states + (size_t)frame * nsub_max * kStateWords;
  uint32_t* ssk = sp + nsub_max;
  uint32_t* ep = ssk + nsub_max;
  uint32_t* esk = ep + nsub_max;
  uint32_t* cnt = esk + nsub_max;

  // tables to LDS, the frame to zero
  {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(buf + d.tables_off);
    uint32_t* dst = reinterpret_cast<uint32_t*>(tabs);
    const int nw = d.ntables * (int)(sizeof(tmr_jpeg_huff) / 4);
    for (int i = t; i < nw; i += NT) dst[i] = src[i];
    if (t < 64) zigzag[t] = kZigzagDev[t];
    if (t == 0) s_err = s_done = 0;
    uint4* z = reinterpret_cast<uint4*>(coef + (size_t)frame * g.total * 64);   // 128 B per block
    const uint4 zero = make_uint4(0, 0, 0, 0);
    for (uint32_t i = t; i < g.total * 8; i += NT) z[i] = zero;
  }
  je::Scan sc;
  sc.words = reinterpret_cast<const uint32_t*>(buf + d.bits_off);
  sc.nbits = nbits;
  sc.tabs = tabs;
  sc.dcsel = dcsel;
  sc.acsel = acsel;

  for (uint32_t i = t; i < nsub; i += NT) {
    sp[i] = i * sub;   // < nbits <= 2^32 - 1
    ssk[i] = je::kDirty;
  }
  __syncthreads();

  // 1 and 2: decode what is dirty, then compare each start with its predecessor's end
  uint32_t r = 0;
  for (; r < nsub; ++r) {
    for (uint32_t i = t; i < nsub; i += NT) {
      const uint32_t sk = ssk[i];
      if (!(sk & je::kDirty)) continue;
      uint32_t e0, e1, n;
      je::sync_sub(sc, g, sp[i], sk & ~je::kDirty, je::sub_limit(nbits, sub, i), &e0, &e1, &n);
      ssk[i] = sk & ~je::kDirty;
      ep[i] = e0;
      esk[i] = e1;
      cnt[i] = n;
    }
    __syncthreads();
    int changed = 0;
    for (uint32_t i = t; i < nsub; i += NT) {
      if (i == 0) continue;
      const uint32_t p = ep[i - 1], sk = esk[i - 1];
      if (p != sp[i] || sk != ssk[i]) {
        sp[i] = p;
        ssk[i] = sk | je::kDirty;
        changed = 1;
      }
    }
    if (!__syncthreads_or(changed)) break;
  }
  if (t == 0) rounds[frame] = r;

  // 3: cnt[i] becomes the number of blocks begun before subsequence i
  {
    const uint32_t per = (nsub + NT - 1) / NT;
    const uint32_t lo = min((uint32_t)t * per, nsub), hi = min(lo + per, nsub);
    uint32_t sum = 0;
    for (uint32_t i = lo; i < hi; ++i) sum += cnt[i];
    uint32_t run = block_scan(sum, scratch) - sum;
    for (uint32_t i = lo; i < hi; ++i) {
      const uint32_t n = cnt[i];
      cnt[i] = run;
      run += n;
    }
  }
  __syncthreads();

  // 4: write pass
  int16_t* out = coef + (size_t)frame * g.total * 64;
  {
    int err = 0, done = 0;
    for (uint32_t i = t; i < nsub; i += NT)
      je::write_sub(sc, g, sp[i], ssk[i], je::sub_limit(nbits, sub, i), cnt[i], out, zigzag, &err, &done);
    if (err) s_err = 1;
    if (done) s_done = 1;
  }
  __syncthreads();

  // 5: DC differences to DC values, per component in scan order
  for (int c = 0; c < g.ncomp; ++c) {
    const uint32_t n = je::comp_blocks(g, c);
    const uint32_t per = (n + NT - 1) / NT;
    const uint32_t lo = min((uint32_t)t * per, n), hi = min(lo + per, n);
    uint32_t sum = 0;
    for (uint32_t j = lo; j < hi; ++j) sum += (uint32_t)(int)out[je::dc_index(g, c, j)];
    uint32_t run = block_scan(sum, scratch) - sum;
    for (uint32_t j = lo; j < hi; ++j) {
      const uint32_t at = je::dc_index(g, c, j);
      run += (uint32_t)(int)out[at];
      out[at] = (int16_t)(uint16_t)run;
    }
  }
  if (t == 0) status[frame] = s_err ? 2 : (s_done ? 0 : 1);
}

bool sub_ok(int sub_bits) { return sub_bits == 0 || (sub_bits >= 64 && sub_bits % 32 == 0); }

uint32_t sub_of(int sub_bits) { return sub_bits ? (uint32_t)sub_bits : je::kDefaultSubBits; }

size_t rounds_bytes(int f) { return ((size_t)f * 4 + 15) & ~(size_t)15; }

uint32_t nsub_of(uint32_t max_bits, uint32_t sub) {
  const uint64_t n = ((uint64_t)max_bits + sub - 1) / sub;
  return n ? (uint32_t)n : 1;
}

}  // namespace

TMR_API size_t tmr_jpeg_entropy_ws_bytes(int f, uint32_t max_bits, int sub_bits) {
  if (f <= 0 || !sub_ok(sub_bits)) {
    tmr_set_error("tmr_jpeg_entropy_ws_bytes: bad arguments f=%d sub_bits=%d", f, sub_bits);
    return 0;
  }
  return rounds_bytes(f) + (size_t)f * nsub_of(max_bits, sub_of(sub_bits)) * kStateWords * 4;
}

TMR_API int tmr_jpeg_entropy_decode_device(const tmr_jpeg_scan_desc* desc, const uint8_t* buf,
                                           size_t buf_bytes, int f, int h, int w, int sampling,
                                           uint32_t max_bits, int sub_bits, int16_t* coef,
                                           int32_t* status, void* ws, size_t ws_bytes,
                                           hipStream_t stream) {
  je::Geom g;
  TMR_CHECK_ARG(f > 0 && je::make_geom(h, w, sampling, &g),
                "tmr_jpeg_entropy_decode_device: bad sizes f=%d h=%d w=%d sampling=%d", f, h, w, sampling);
  TMR_CHECK_ARG(sub_ok(sub_bits),
                "tmr_jpeg_entropy_decode_device: sub_bits=%d is neither 0 nor a multiple of 32 >= 64", sub_bits);
  TMR_CHECK_ARG(desc && buf && coef && status && ws, "tmr_jpeg_entropy_decode_device: null operand");
  TMR_CHECK_ARG(((uintptr_t)desc & 7) == 0 && ((uintptr_t)buf & 15) == 0 && ((uintptr_t)coef & 15) == 0 &&
                    ((uintptr_t)status & 3) == 0 && ((uintptr_t)ws & 15) == 0,
                "tmr_jpeg_entropy_decode_device: desc must be 8-byte aligned, buf / coef / ws 16-byte aligned");
  const size_t need = tmr_jpeg_entropy_ws_bytes(f, max_bits, sub_bits);
  TMR_CHECK_ARG(ws_bytes >= need, "tmr_jpeg_entropy_decode_device: workspace of %zu bytes, %zu needed",
                ws_bytes, need);
  const uint32_t sub = sub_of(sub_bits);
  uint32_t* rounds = static_cast<uint32_t*>(ws);
  uint32_t* states = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(ws) + rounds_bytes(f));
  hipLaunchKernelGGL(entropy_k, dim3((unsigned)f), dim3(NT), 0, stream, desc, buf, buf_bytes, g, h, w,
                     sampling, max_bits, sub, nsub_of(max_bits, sub), coef, status, rounds, states);
  TMR_CHECK_LAUNCH("tmr_jpeg_entropy_decode_device");
  return 0;
}
