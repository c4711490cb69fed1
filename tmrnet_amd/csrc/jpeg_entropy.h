// The Huffman decode core shared by the device entropy decoder (jpeg_entropy.hip) and the host
// (tests/jpeg_entropy_main.cpp runs the device scheme serially under the host sanitizers): one
// symbol step over a packed scan (tmr_jpeg_scan_pack), and the three passes a lane runs over one
// subsequence of the bit stream.  Plain C++; with TMR_HOST_ONLY it has no HIP in it.
//
// The step has the semantics of decode_block / decode_sym in jpeg_host.cpp: 9-bit first-level
// lookup, the one-lookup `fast` entry for an AC code with its value bits, the canonical slow path
// up to 16 bits, extend, ZRL / EOB; a run past 63, a DC size > 11 and "no such code" are errors.
// A state is (bit position p, slot in the MCU, zigzag index k); k == 0 means "the next symbol is
// a block's DC code".  Past the frame's bit count the stream reads as zero bits.
//
// On an error the step skips one bit and goes to the next block: a speculative lane, which
// starts in the middle of a symbol, never stops, and every step consumes at least one bit, so a
// pass over a subsequence of n bits takes at most n steps.
#pragma once
#include "tmr.h"

#if defined(__HIPCC__) && !defined(TMR_HOST_ONLY)
#define JE_HD __host__ __device__ inline
#else
#define JE_HD inline
#endif

namespace je {

enum { kCoef = 1, kBegin = 2, kEnd = 4, kError = 8 };
constexpr uint32_t kDefaultSubBits = 1024;
constexpr uint32_t kDirty = 0x80000000u;   // in a start state's sk word: decode it again

// natural index of zigzag position k
#define JE_ZIGZAG                                                                                  \
  {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,         \
   41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,         \
   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}

// Block grids of one (h, w, sampling), as jpeg_host.cpp's classify() and jpeg.hip's make_geom()
// derive them; chroma is always 1x1, so components 1 and 2 share a grid.
struct Geom {
  int ncomp, nslots;   // components; blocks per MCU
  int hv, hs;          // component 0's blocks per MCU, and per MCU row of them
  int mcu_w, mcu_h;
  int bw0, bh0, bw1, bh1;
  uint32_t off1, off2;   // first coefficient of components 1 and 2
  uint32_t total;        // blocks per frame
};

inline bool make_geom(int h, int w, int sampling, Geom* g) {
  if (h <= 0 || w <= 0 || h > 65535 || w > 65535) return false;
  if (sampling != TMR_JPEG_GRAY && sampling != TMR_JPEG_444 && sampling != TMR_JPEG_420) return false;
  const int mcu = sampling == TMR_JPEG_420 ? 16 : 8;
  g->mcu_w = (w + mcu - 1) / mcu;
  g->mcu_h = (h + mcu - 1) / mcu;
  g->ncomp = sampling == TMR_JPEG_GRAY ? 1 : 3;
  g->hs = sampling == TMR_JPEG_420 ? 2 : 1;
  g->hv = g->hs * g->hs;
  g->nslots = g->hv + g->ncomp - 1;
  g->bw0 = g->mcu_w * g->hs;
  g->bh0 = g->mcu_h * g->hs;
  g->bw1 = g->ncomp == 3 ? g->mcu_w : 0;
  g->bh1 = g->ncomp == 3 ? g->mcu_h : 0;
  const uint64_t n0 = (uint64_t)g->bw0 * g->bh0, n1 = (uint64_t)g->bw1 * g->bh1;
  if ((n0 + 2 * n1) * 64 > 0x7fffffffu) return false;
  g->off1 = (uint32_t)(n0 * 64);
  g->off2 = (uint32_t)((n0 + n1) * 64);
  g->total = (uint32_t)(n0 + 2 * n1);
  return true;
}

JE_HD int slot_comp(const Geom& g, int slot) { return slot < g.hv ? 0 : slot - g.hv + 1; }

// First coefficient of the block with ordinal `ord` in scan (MCU) order; ord < g.total.
JE_HD uint32_t coef_index(const Geom& g, uint32_t ord) {
  const uint32_t m = ord / (uint32_t)g.nslots, s = ord - m * (uint32_t)g.nslots;
  const uint32_t my = m / (uint32_t)g.mcu_w, mx = m - my * (uint32_t)g.mcu_w;
  if (s < (uint32_t)g.hv) {
    const uint32_t v = s / (uint32_t)g.hs, h = s - v * (uint32_t)g.hs;
    return ((my * g.hs + v) * (uint32_t)g.bw0 + mx * g.hs + h) * 64;
  }
  return (s - g.hv == 0 ? g.off1 : g.off2) + (my * (uint32_t)g.bw1 + mx) * 64;
}

// First coefficient of component c's j-th block in scan order; j < the component's block count.
JE_HD uint32_t dc_index(const Geom& g, int c, uint32_t j) {
  if (c == 0) {
    const uint32_t m = j / (uint32_t)g.hv, s = j - m * (uint32_t)g.hv;
    return coef_index(g, m * (uint32_t)g.nslots + s);
  }
  return (c == 1 ? g.off1 : g.off2) + j * 64;   // chroma: block raster order is MCU order
}

JE_HD uint32_t comp_blocks(const Geom& g, int c) {
  return c == 0 ? (uint32_t)g.bw0 * g.bh0 : (uint32_t)g.bw1 * g.bh1;
}

// One frame's packed scan as a lane sees it.
struct Scan {
  const uint32_t* words;       // the bits, 4-byte aligned, (nbits / 8 + 8) rounded up to 16 bytes
  uint32_t nbits;
  const tmr_jpeg_huff* tabs;   // the frame's tables
  uint32_t dcsel, acsel;       // byte c: the table of component c
};

// The 32 bits at bit position p, MSB first; bits at and past nbits read as zero.  Reads words
// p / 32 and p / 32 + 1 only for p < nbits: inside the padded buffer.
JE_HD uint32_t peek32(const Scan& sc, uint32_t p) {
  if (p >= sc.nbits) return 0;
  const uint32_t i = p >> 5, sh = p & 31;
  const uint32_t hi = __builtin_bswap32(sc.words[i]), lo = __builtin_bswap32(sc.words[i + 1]);
  uint32_t v = sh ? (hi << sh) | (lo >> (32 - sh)) : hi;
  const uint32_t rem = sc.nbits - p;
  if (rem < 32) v &= ~(0xffffffffu >> rem);
  return v;
}

// One Huffman symbol from the top of v; *len = its code length.  -1: no such code.
JE_HD int decode_sym(const tmr_jpeg_huff* t, uint32_t v, int* len) {
  const uint32_t e = t->lut[v >> 23];
  if (e) {
    *len = (int)(e >> 8);
    return (int)(e & 0xff);
  }
  const int32_t c16 = (int32_t)(v >> 16);
  for (int l = 10; l <= 16; ++l) {
    const int32_t code = c16 >> (16 - l);
    if (code <= t->maxcode[l]) {
      const int i = t->valoff[l] + code;
      if (i < 0 || i >= t->nsym) return -1;
      *len = l;
      return t->sym[i];
    }
  }
  return -1;
}

JE_HD int extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// One step from (*p, slot, *k).  Returns flags: kBegin = this was a block's DC symbol; kCoef =
// *val belongs at zigzag position *zz of the current block (for the DC it is the difference to
// the predictor); kEnd = the block ended, the next state is (slot + 1, k = 0) -- the caller
// advances the slot; kError = invalid, recovered from.  *p grows by 1..31.
JE_HD int step(const Scan& sc, const Geom& g, uint32_t* p, int slot, int* k, int* zz, int* val) {
  const uint32_t v = peek32(sc, *p);
  const int c = slot_comp(g, slot);
  int len = 0;
  if (*k == 0) {
    const int s = decode_sym(sc.tabs + ((sc.dcsel >> (8 * c)) & 0xff), v, &len);
    if (s < 0 || s > 11) {
      *p += 1;
      return kBegin | kEnd | kError;
    }
    *val = s ? extend((int)((v << len) >> (32 - s)), s) : 0;   // len <= 16, s <= 11
    *zz = 0;
    *p += (uint32_t)(len + s);
    *k = 1;
    return kBegin | kCoef;
  }
  const tmr_jpeg_huff* ac = sc.tabs + ((sc.acsel >> (8 * c)) & 0xff);
  int flags = 0;
  const int f = ac->fast[v >> 23];
  if (f) {   // run, size and value in one lookup
    const int kk = *k + ((f >> 4) & 15);
    if (kk > 63) {
      *p += 1;
      *k = 0;
      return kEnd | kError;
    }
    *zz = kk;
    *val = f >> 8;
    *k = kk + 1;
    *p += (uint32_t)(f & 15);
    flags = kCoef;
  } else {
    const int rs = decode_sym(ac, v, &len);
    if (rs < 0) {
      *p += 1;
      *k = 0;
      return kEnd | kError;
    }
    const int r = rs >> 4, s = rs & 15;
    if (s == 0) {
      *p += (uint32_t)len;
      if (r != 15) {   // end of block
        *k = 0;
        return kEnd;
      }
      *k += 16;
    } else {
      const int kk = *k + r;
      if (kk > 63) {
        *p += 1;
        *k = 0;
        return kEnd | kError;
      }
      *zz = kk;
      *val = extend((int)((v << len) >> (32 - s)), s);   // len <= 16, s <= 15
      *k = kk + 1;
      *p += (uint32_t)(len + s);
      flags = kCoef;
    }
  }
  if (*k > 63) {
    *k = 0;
    flags |= kEnd;
  }
  return flags;
}

JE_HD uint32_t pack_sk(int slot, int k) { return ((uint32_t)slot << 8) | (uint32_t)k; }

// Where subsequence i of `sub` bits ends: its lanes decode symbols that start before this.
JE_HD uint32_t sub_limit(uint32_t nbits, uint32_t sub, uint32_t i) {
  const uint64_t e = (uint64_t)(i + 1) * sub;
  return e < nbits ? (uint32_t)e : nbits;
}

// Synchronisation pass over one subsequence: from state (p, sk) decode every symbol that starts
// before `lim`; the state after the last one goes to *ep / *esk, the blocks begun to *count.
JE_HD void sync_sub(const Scan& sc, const Geom& g, uint32_t p, uint32_t sk, uint32_t lim,
                    uint32_t* ep, uint32_t* esk, uint32_t* count) {
  int slot = (int)((sk >> 8) & 0xff), k = (int)(sk & 0xff), zz = 0, val = 0;
  uint32_t n = 0;
  const uint32_t steps = lim > p ? lim - p : 0;   // a step consumes at least one bit
  for (uint32_t it = 0; it < steps && p < lim; ++it) {
    const int fl = step(sc, g, &p, slot, &k, &zz, &val);
    if (fl & kBegin) ++n;
    if (fl & kEnd) slot = slot + 1 == g.nslots ? 0 : slot + 1;
  }
  *ep = p;
  *esk = pack_sk(slot, k);
  *count = n;
}

// Write pass over one subsequence, from its true start state; `ord` blocks began before it.
// Coefficients go to the zero-filled coef (the frame's g.total * 64 entries; the DC entry gets
// the difference); blocks past g.total are not stored.  *err is set on an error in a block the
// frame has, *done when the frame's last block ends inside the data.
JE_HD void write_sub(const Scan& sc, const Geom& g, uint32_t p, uint32_t sk, uint32_t lim,
                     uint32_t ord, int16_t* coef, const uint8_t* zigzag, int* err, int* done) {
  int slot = (int)((sk >> 8) & 0xff), k = (int)(sk & 0xff), zz = 0, val = 0;
  uint32_t cur = ord - 1;   // the block in progress; none (0xffffffff) before the first
  uint32_t base = cur < g.total ? coef_index(g, cur) : 0;
  const uint32_t steps = lim > p ? lim - p : 0;
  for (uint32_t it = 0; it < steps && p < lim; ++it) {
    const int fl = step(sc, g, &p, slot, &k, &zz, &val);
    if (fl & kBegin) {
      cur = ord++;
      base = cur < g.total ? coef_index(g, cur) : 0;
    }
    if (cur < g.total) {
      if (fl & kError) *err = 1;
      if (fl & kCoef) coef[base + zigzag[zz & 63]] = (int16_t)val;   // base + 63 < g.total * 64
      if ((fl & kEnd) && cur == g.total - 1 && p <= sc.nbits) *done = 1;
    }
    if (fl & kEnd) slot = slot + 1 == g.nslots ? 0 : slot + 1;
  }
}

}  // namespace je
