// Host half of the baseline JPEG decode (include/tmr.h, "baseline JPEG decode"): the marker
// parse and the Huffman decode into DCT coefficients -- the serial part of pil_loader
// (train_only_non-local_pretrained.py:96-99); jpeg.hip does the rest on the device.
//
// Plain C++ with no HIP in it and no state outside the call: threads decode side by side.
// Every read goes through a position checked against the input length; a stream that ends early,
// or whose codes, run lengths or markers are wrong, returns 1 and is never read past its end.
#define TMR_HOST_ONLY
#include "tmr.h"

#include <string.h>

void tmr_set_error(const char* fmt, ...);
#define TMR_JPEG_API extern "C" __attribute__((visibility("default")))

namespace {

enum { kOk = 0, kBad = 1, kUnsupported = 2, kArgs = 3 };

const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                             12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                             35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                             58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr int kLutBits = 9;

struct Huff {
  bool defined;
  uint16_t lut[1 << kLutBits];   // (length << 8) | symbol for codes of <= kLutBits bits, else 0
  int32_t maxcode[18];           // largest code of each length, -1 where there is none
  int32_t valoff[17];            // index of a length's first symbol minus its first code
  int nsym;
  uint8_t sym[256];
  // AC tables: where a code and its value bits fit in kLutBits, value * 256 + (run << 4) +
  // (code length + value bits); else 0.  32 bit: a 1-bit code leaves room for 8 value bits,
  // |value| <= 255, and value * 256 does not fit 16.
  int32_t fast[1 << kLutBits];
};

struct Comp {
  int id, h, v, tq, td, ta;
};

struct Header {
  int width, height, ncomp;
  Comp comp[3];
  bool have_sof, have_qt[4];
  uint16_t qt[4][64];
  Huff dc[4], ac[4];
  int restart;
  int adobe_transform;   // -1: no Adobe APP14 segment
  bool jfif;
  size_t scan;           // first byte of the entropy-coded data
};

inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// DHT payload for one table: 16 counts, then the symbols.  Returns bytes used, 0 on error.
size_t build_huff(const uint8_t* p, size_t avail, Huff* t) {
  if (avail < 16) return 0;
  int total = 0;
  for (int l = 0; l < 16; ++l) total += p[l];
  if (total > 256 || avail < 16 + (size_t)total) return 0;
  memset(t->lut, 0, sizeof(t->lut));
  t->nsym = total;
  memcpy(t->sym, p + 16, total);
  int code = 0, k = 0;
  for (int l = 1; l <= 16; ++l) {
    const int n = p[l - 1];
    t->valoff[l] = k - code;
    if (code + n > (1 << l)) return 0;   // more codes than l bits hold
    if (l <= kLutBits) {
      for (int i = 0; i < n; ++i) {
        const int first = (code + i) << (kLutBits - l);
        for (int f = 0; f < (1 << (kLutBits - l)); ++f)
          t->lut[first + f] = (uint16_t)((l << 8) | t->sym[k + i]);
      }
    }
    code += n;
    k += n;
    t->maxcode[l] = n ? code - 1 : -1;
    code <<= 1;
  }
  t->maxcode[17] = 0x7fffffff;
  for (int i = 0; i < (1 << kLutBits); ++i) {
    const int e = t->lut[i], len = e >> 8, run = (e >> 4) & 15, sz = e & 15;
    t->fast[i] = 0;
    if (e && sz && len + sz <= kLutBits) {
      int v = (i >> (kLutBits - len - sz)) & ((1 << sz) - 1);
      if (v < (1 << (sz - 1))) v -= (1 << sz) - 1;
      t->fast[i] = v * 256 + run * 16 + len + sz;   // |v| <= 255 (sz <= 8); the rest is < 256
    }
  }
  t->defined = true;
  return 16 + (size_t)total;
}

// MSB-first bit reader over the entropy-coded segment: removes the stuffed zero after 0xFF and
// stops at a marker or at the end of the input, after which it feeds zero bits and counts them
// (pad); a caller that has consumed any of those has run off the data (overrun()).
struct Bits {
  const uint8_t* p;
  size_t pos, end;
  uint64_t acc;   // the top nbits bits are valid
  int nbits;
  int pad;        // zero bits fed since the data ran out; always the lowest valid bits
  bool stopped;   // at a marker (pos is on its 0xFF) or at the end of the input

  // Afterwards at least 32 bits are valid: a code (<= 16) and its value bits (<= 15).
  inline void refill() {
    if (nbits >= 32) return;
    if (!stopped && pos + 4 <= end) {
      const uint32_t v = ((uint32_t)p[pos] << 24) | ((uint32_t)p[pos + 1] << 16) |
                         ((uint32_t)p[pos + 2] << 8) | p[pos + 3];
      const uint32_t m = ~v;   // a zero byte of m is a 0xFF byte of v
      if (((m - 0x01010101u) & ~m & 0x80808080u) == 0) {
        acc |= (uint64_t)v << (32 - nbits);
        nbits += 32;
        pos += 4;
        return;
      }
    }
    while (nbits <= 56) {
      uint8_t b = 0;
      if (!stopped && pos < end) {
        b = p[pos];
        if (b != 0xFF) {
          ++pos;
        } else if (pos + 1 < end && p[pos + 1] == 0) {
          pos += 2;
        } else {
          stopped = true;
          b = 0;
        }
      } else {
        stopped = true;
      }
      if (stopped) pad += 8;
      acc |= (uint64_t)b << (56 - nbits);
      nbits += 8;
    }
  }
  inline uint32_t peek(int n) const { return (uint32_t)(acc >> (64 - n)); }   // 1 <= n <= 32
  inline void skip(int n) {
    acc <<= n;
    nbits -= n;
  }
  inline bool overrun() const { return pad > nbits; }
};

// One Huffman symbol; needs >= 16 valid bits.  -1: no such code.
inline int decode_sym(Bits& b, const Huff& t) {
  const uint16_t e = t.lut[b.peek(kLutBits)];
  if (e) {
    b.skip(e >> 8);
    return e & 0xff;
  }
  const int32_t c16 = (int32_t)b.peek(16);
  for (int l = kLutBits + 1; l <= 16; ++l) {
    const int32_t code = c16 >> (16 - l);
    if (code <= t.maxcode[l]) {
      const int i = t.valoff[l] + code;
      if (i < 0 || i >= t.nsym) return -1;
      b.skip(l);
      return t.sym[i];
    }
  }
  return -1;
}

inline int extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// One 8x8 block into blk (natural order, all 64 written).  false: bad code or run length.
inline bool decode_block(Bits& b, const Huff& dc, const Huff& ac, int* pred, int16_t* blk) {
  memset(blk, 0, 64 * sizeof(int16_t));
  b.refill();
  int s = decode_sym(b, dc);
  if (s < 0 || s > 11) return false;
  int diff = 0;
  if (s) {
    diff = extend((int)b.peek(s), s);
    b.skip(s);
  }
  // the predictor wraps like the int16 it is stored as, so no stream can overflow it
  *pred = (int16_t)(uint16_t)(*pred + diff);
  blk[0] = (int16_t)*pred;
  for (int k = 1; k < 64;) {
    b.refill();
    const int f = ac.fast[b.peek(kLutBits)];
    if (f) {   // run, size and value in one lookup
      k += (f >> 4) & 15;
      if (k > 63) return false;
      blk[kZigzag[k++]] = (int16_t)(f >> 8);
      b.skip(f & 15);
      continue;
    }
    const int rs = decode_sym(b, ac);
    if (rs < 0) return false;
    const int r = rs >> 4;
    s = rs & 15;
    if (s == 0) {
      if (r != 15) break;   // end of block
      k += 16;
      continue;
    }
    k += r;
    if (k > 63) return false;
    blk[kZigzag[k]] = (int16_t)extend((int)b.peek(s), s);
    b.skip(s);
    ++k;
  }
  return true;
}

int fail(int rc, const char* what, const char* msg) {
  tmr_set_error("%s: %s", what, msg);
  return rc;
}

// Markers up to and including SOS.  Fills hd; 0 / 1 / 2.
int parse_headers(const uint8_t* d, size_t len, const char* who, Header* hd) {
  memset(hd, 0, sizeof(*hd));
  hd->adobe_transform = -1;
  if (len < 4) return fail(kBad, who, "shorter than any JPEG");
  if (d[0] != 0xFF || d[1] != 0xD8) return fail(kUnsupported, who, "not a JPEG file (no SOI)");
  size_t pos = 2;
  for (;;) {
    if (pos + 2 > len) return fail(kBad, who, "truncated before the scan");
    if (d[pos] != 0xFF) return fail(kBad, who, "marker expected");
    while (pos < len && d[pos] == 0xFF) ++pos;   // fill bytes
    if (pos >= len) return fail(kBad, who, "truncated before the scan");
    const int m = d[pos++];
    if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;   // no payload
    if (m == 0xD9) return fail(kBad, who, "end of image before any scan");
    if (m == 0xD8 || m == 0x00) return fail(kBad, who, "misplaced marker");
    if (pos + 2 > len) return fail(kBad, who, "truncated segment length");
    const size_t seg = (size_t)be16(d + pos);
    if (seg < 2 || seg > len - pos) return fail(kBad, who, "segment runs past the end of the file");
    const uint8_t* p = d + pos + 2;
    const size_t n = seg - 2;
    pos += seg;
    if (m == 0xC0) {
      if (hd->have_sof) return fail(kBad, who, "second frame header");
      if (n < 6) return fail(kBad, who, "short SOF0");
      if (p[0] != 8) return fail(kUnsupported, who, "sample precision is not 8 bit");
      hd->height = be16(p + 1);
      hd->width = be16(p + 3);
      const int nc = p[5];
      if (n != 6 + 3 * (size_t)nc) return fail(kBad, who, "SOF0 length does not match its components");
      if (hd->width == 0) return fail(kBad, who, "zero width");
      if (hd->height == 0) return fail(kUnsupported, who, "height given by a DNL marker");
      if (nc != 1 && nc != 3) return fail(kUnsupported, who, "neither one nor three components");
      hd->ncomp = nc;
      for (int c = 0; c < nc; ++c) {
        Comp& k = hd->comp[c];
        k.id = p[6 + 3 * c];
        k.h = p[7 + 3 * c] >> 4;
        k.v = p[7 + 3 * c] & 15;
        k.tq = p[8 + 3 * c];
        if (k.h < 1 || k.h > 4 || k.v < 1 || k.v > 4 || k.tq > 3)
          return fail(kBad, who, "bad component in SOF0");
      }
      hd->have_sof = true;
    } else if ((m >= 0xC1 && m <= 0xCF) && m != 0xC4 && m != 0xC8) {
      return fail(kUnsupported, who, m == 0xC2 ? "progressive JPEG (SOF2)"
                                     : m == 0xCC ? "arithmetic coding"
                                                 : "frame type other than baseline SOF0");
    } else if (m == 0xC4) {
      size_t o = 0;
      while (o < n) {
        const int tc = p[o] >> 4, th = p[o] & 15;
        if (tc > 1 || th > 3) return fail(kBad, who, "bad Huffman table id");
        const size_t used = build_huff(p + o + 1, n - o - 1, tc ? &hd->ac[th] : &hd->dc[th]);
        if (!used) return fail(kBad, who, "bad or truncated Huffman table");
        o += 1 + used;
      }
    } else if (m == 0xDB) {
      size_t o = 0;
      while (o < n) {
        const int pq = p[o] >> 4, tq = p[o] & 15;
        if (pq > 1 || tq > 3) return fail(kBad, who, "bad quantisation table id");
        if (pq == 1) return fail(kUnsupported, who, "16-bit quantisation table");
        if (n - o < 65) return fail(kBad, who, "truncated quantisation table");
        for (int i = 0; i < 64; ++i) hd->qt[tq][kZigzag[i]] = p[o + 1 + i];
        hd->have_qt[tq] = true;
        o += 65;
      }
    } else if (m == 0xDD) {
      if (n != 2) return fail(kBad, who, "bad DRI length");
      hd->restart = be16(p);
    } else if (m == 0xE0) {
      if (n >= 5 && !memcmp(p, "JFIF", 5)) hd->jfif = true;
    } else if (m == 0xEE) {
      if (n >= 12 && !memcmp(p, "Adobe", 5)) hd->adobe_transform = p[11];
    } else if (m == 0xDA) {
      if (!hd->have_sof) return fail(kBad, who, "scan before the frame header");
      if (n < 1) return fail(kBad, who, "short SOS");
      const int ns = p[0];
      if (ns < 1 || ns > 4 || n != 4 + 2 * (size_t)ns) return fail(kBad, who, "bad SOS length");
      if (ns != hd->ncomp) return fail(kUnsupported, who, "more than one scan");
      for (int c = 0; c < ns; ++c) {
        Comp& k = hd->comp[c];
        if (p[1 + 2 * c] != k.id) return fail(kUnsupported, who, "scan components out of frame order");
        k.td = p[2 + 2 * c] >> 4;
        k.ta = p[2 + 2 * c] & 15;
        if (k.td > 3 || k.ta > 3 || !hd->dc[k.td].defined || !hd->ac[k.ta].defined)
          return fail(kBad, who, "scan names a Huffman table that is not defined");
        if (!hd->have_qt[k.tq]) return fail(kBad, who, "component names a quantisation table that is not defined");
      }
      if (p[1 + 2 * ns] != 0 || p[2 + 2 * ns] != 63 || p[3 + 2 * ns] != 0)
        return fail(kBad, who, "spectral selection of a baseline scan is not 0..63");
      hd->scan = pos;
      return kOk;
    }
    // APPn, COM, DNL and the rest: skipped
  }
}

// Sampling class and block grids from the parsed header into info.  0 / 2.
int classify(const Header& hd, const char* who, tmr_jpeg_info* info) {
  memset(info, 0, sizeof(*info));
  info->width = hd.width;
  info->height = hd.height;
  info->ncomp = hd.ncomp;
  int mcu = 8;
  if (hd.ncomp == 1) {
    if (hd.comp[0].h != 1 || hd.comp[0].v != 1)
      return fail(kUnsupported, who, "greyscale with sampling factors other than 1x1");
    info->sampling = TMR_JPEG_GRAY;
  } else {
    const Comp* k = hd.comp;
    if (hd.adobe_transform >= 0 && hd.adobe_transform != 1)
      return fail(kUnsupported, who, "Adobe transform flag says the components are not YCbCr");
    if (hd.adobe_transform < 0 && !hd.jfif && k[0].id == 'R' && k[1].id == 'G' && k[2].id == 'B')
      return fail(kUnsupported, who, "components are marked RGB");
    if (k[1].h != 1 || k[1].v != 1 || k[2].h != 1 || k[2].v != 1)
      return fail(kUnsupported, who, "chroma sampling factors other than 1x1");
    if (k[0].h == 1 && k[0].v == 1) {
      info->sampling = TMR_JPEG_444;
    } else if (k[0].h == 2 && k[0].v == 2) {
      info->sampling = TMR_JPEG_420;
      mcu = 16;
    } else {
      return fail(kUnsupported, who, "chroma subsampling other than 4:4:4 and 4:2:0");
    }
  }
  const int mw = (hd.width + mcu - 1) / mcu, mh = (hd.height + mcu - 1) / mcu;
  uint64_t blocks = 0;
  for (int c = 0; c < hd.ncomp; ++c) {
    info->blocks_w[c] = mw * hd.comp[c].h;
    info->blocks_h[c] = mh * hd.comp[c].v;
    blocks += (uint64_t)info->blocks_w[c] * info->blocks_h[c];
    memcpy(info->qt[c], hd.qt[hd.comp[c].tq], sizeof(info->qt[c]));
  }
  info->coef_bytes = blocks * 64 * sizeof(int16_t);
  return kOk;
}

int probe(const uint8_t* data, size_t len, const char* who, Header* hd, tmr_jpeg_info* info) {
  if (!data || !info) return fail(kArgs, who, "null argument");
  int rc = parse_headers(data, len, who, hd);
  if (rc) return rc;
  rc = classify(*hd, who, info);
  if (rc) return rc;
  // a block costs at least two bits (a DC code and an end of block): a header whose size the
  // scan data cannot fill is refused before anyone sizes a buffer by it
  const uint64_t blocks = info->coef_bytes / 128;
  if ((uint64_t)(len - hd->scan) * 8 < blocks * 2)
    return fail(kBad, who, "scan data too short for the image size");
  return kOk;
}

}  // namespace

TMR_JPEG_API int tmr_jpeg_probe(const uint8_t* data, size_t len, tmr_jpeg_info* info) {
  static const char who[] = "tmr_jpeg_probe";
  Header hd;
  const int rc = probe(data, len, who, &hd, info);
  if (rc) return rc;
  // the scan must end in a marker that is not a restart (EOI in practice)
  // (searched from the end, where a whole file has its EOI)
  for (size_t i = len - 1; i > hd.scan; --i) {
    const uint8_t m = data[i];
    if (data[i - 1] == 0xFF && m != 0x00 && m != 0xFF && !(m >= 0xD0 && m <= 0xD7)) return kOk;
  }
  return fail(kBad, who, "truncated: no marker ends the scan data");
}

// The scan packed for the device entropy decoder (jpeg_entropy.hip): the same header parse, then
// a byte copy that drops the stuffed zeros and stops where Bits::refill stops -- at a marker, at
// a lone 0xFF in the last byte, or at the end of the input.
TMR_JPEG_API int tmr_jpeg_scan_pack(const uint8_t* data, size_t len, tmr_jpeg_info* info,
                                    uint8_t* bits, size_t bits_cap, uint64_t bits_off,
                                    tmr_jpeg_huff* tables, size_t tables_cap, uint64_t tables_off,
                                    tmr_jpeg_scan_desc* desc) {
  static const char who[] = "tmr_jpeg_scan_pack";
  Header hd;
  int rc = probe(data, len, who, &hd, info);
  if (rc) return rc;
  if (hd.restart)
    return fail(TMR_JPEG_HOST_PASS, who, "restart interval: this file keeps the host entropy pass");
  if (!bits && !tables && !desc) return kOk;   // a query: the status alone, nothing packed
  if (!bits || !tables || !desc) return fail(kArgs, who, "null output");
  if ((bits_off & 15) || (tables_off & 15)) return fail(kArgs, who, "offsets must be multiples of 16");

  // the distinct tables the scan names, in order of first use
  const Huff* used[TMR_JPEG_MAX_TABLES];
  int ntab = 0;
  uint8_t dc_ix[4] = {0, 0, 0, 0}, ac_ix[4] = {0, 0, 0, 0};
  for (int c = 0; c < hd.ncomp; ++c) {
    for (int kind = 0; kind < 2; ++kind) {
      const Huff* t = kind ? &hd.ac[hd.comp[c].ta] : &hd.dc[hd.comp[c].td];
      int at = 0;
      while (at < ntab && used[at] != t) ++at;
      if (at == ntab) used[ntab++] = t;   // <= 2 per component, <= 3 components
      (kind ? ac_ix : dc_ix)[c] = (uint8_t)at;
    }
  }
  // unstuffing only shrinks: the raw length bounds the packed one before anything is written
  size_t n = 0;
  for (size_t pos = hd.scan; pos < len; ++pos, ++n) {
    if (data[pos] != 0xFF) continue;
    if (pos + 1 < len && data[pos + 1] == 0) {
      ++pos;
      continue;
    }
    break;
  }
  const size_t padded = TMR_JPEG_SCAN_CAP(n);
  if ((uint64_t)n * 8 > 0xffffffffu) return fail(kUnsupported, who, "scan longer than 2^32 bits");
  if (bits_cap < padded) return fail(kArgs, who, "bit buffer too small");
  if (tables_cap < (size_t)ntab * sizeof(tmr_jpeg_huff)) return fail(kArgs, who, "table buffer too small");

  size_t o = 0;
  for (size_t pos = hd.scan; o < n; ++pos) {
    const uint8_t b = data[pos];   // pos < len: the count above walked the same bytes
    bits[o++] = b;
    if (b == 0xFF) ++pos;
  }
  memset(bits + n, 0, padded - n);

  for (int t = 0; t < ntab; ++t) {
    const Huff& h = *used[t];
    tmr_jpeg_huff* d = tables + t;
    memset(d, 0, sizeof(*d));
    memcpy(d->lut, h.lut, sizeof(d->lut));
    memcpy(d->fast, h.fast, sizeof(d->fast));
    memcpy(d->maxcode, h.maxcode, sizeof(d->maxcode));
    memcpy(d->valoff + 1, h.valoff + 1, 16 * sizeof(int32_t));
    d->nsym = h.nsym;
    memcpy(d->sym, h.sym, (size_t)h.nsym);
  }

  memset(desc, 0, sizeof(*desc));
  desc->bits_off = bits_off;
  desc->tables_off = tables_off;
  desc->nbits = (uint32_t)(n * 8);
  desc->bits_bytes = (uint32_t)padded;
  desc->ntables = ntab;
  desc->ncomp = info->ncomp;
  desc->sampling = info->sampling;
  desc->width = info->width;
  desc->height = info->height;
  int slots = 0;
  for (int c = 0; c < hd.ncomp; ++c) {
    desc->blocks_w[c] = info->blocks_w[c];
    desc->blocks_h[c] = info->blocks_h[c];
    desc->dc_table[c] = dc_ix[c];
    desc->ac_table[c] = ac_ix[c];
    for (int i = 0; i < hd.comp[c].h * hd.comp[c].v; ++i) desc->slot_comp[slots++] = (uint8_t)c;
  }
  desc->mcu_blocks = slots;   // 1, 3 or 6: classify() admits no other sampling
  return kOk;
}

TMR_JPEG_API int tmr_jpeg_entropy_decode(const uint8_t* data, size_t len, tmr_jpeg_info* info,
                                         int16_t* coef, size_t coef_bytes) {
  static const char who[] = "tmr_jpeg_entropy_decode";
  Header hd;
  int rc = probe(data, len, who, &hd, info);
  if (rc) return rc;
  if (!coef) return fail(kArgs, who, "null coefficient buffer");
  if ((uint64_t)coef_bytes < info->coef_bytes) return fail(kArgs, who, "coefficient buffer too small");

  Bits b;
  b.p = data;
  b.pos = hd.scan;
  b.end = len;
  b.acc = 0;
  b.nbits = 0;
  b.pad = 0;
  b.stopped = false;

  const int nc = hd.ncomp;
  const int mcu_w = info->blocks_w[0] / hd.comp[0].h, mcu_h = info->blocks_h[0] / hd.comp[0].v;
  int16_t* plane[3];
  int16_t* at = coef;
  for (int c = 0; c < nc; ++c) {
    plane[c] = at;
    at += (size_t)info->blocks_w[c] * info->blocks_h[c] * 64;
  }
  int pred[3] = {0, 0, 0};
  int until_restart = hd.restart, next_rst = 0;
  for (int my = 0; my < mcu_h; ++my) {
    for (int mx = 0; mx < mcu_w; ++mx) {
      if (hd.restart && until_restart == 0) {
        // the interval ends on a byte boundary (under 8 bits of fill), then RSTn
        if (b.overrun()) return fail(kBad, who, "truncated scan data");
        if (b.nbits - b.pad >= 8) return fail(kBad, who, "bytes between the interval and its restart marker");
        size_t p = b.pos;
        if (p >= len || data[p] != 0xFF) return fail(kBad, who, "restart marker expected");
        while (p < len && data[p] == 0xFF) ++p;
        if (p >= len || data[p] != 0xD0 + next_rst) return fail(kBad, who, "restart marker expected");
        b.pos = p + 1;
        b.acc = 0;
        b.nbits = 0;
        b.pad = 0;
        b.stopped = false;
        next_rst = (next_rst + 1) & 7;
        until_restart = hd.restart;
        pred[0] = pred[1] = pred[2] = 0;
      }
      for (int c = 0; c < nc; ++c) {
        const Comp& k = hd.comp[c];
        for (int v = 0; v < k.v; ++v) {
          for (int h = 0; h < k.h; ++h) {
            const size_t by = (size_t)my * k.v + v, bx = (size_t)mx * k.h + h;
            int16_t* blk = plane[c] + (by * info->blocks_w[c] + bx) * 64;
            if (!decode_block(b, hd.dc[k.td], hd.ac[k.ta], &pred[c], blk))
              return fail(kBad, who, b.overrun() ? "truncated scan data" : "bad Huffman code or run length");
          }
        }
      }
      if (b.overrun()) return fail(kBad, who, "truncated scan data");
      --until_restart;
    }
  }
  return kOk;
}
