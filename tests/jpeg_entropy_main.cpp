// Stand-alone driver of the device entropy decoder's logic on the host: the shared decode core
// (tmrnet_amd/csrc/jpeg_entropy.h) run through the phases of jpeg_entropy.hip serially, with the
// workgroup's lanes as a loop, against tmr_jpeg_entropy_decode (jpeg_host.cpp).
// tests/test_jpeg_entropy_cpu.py builds it plain and with -fsanitize=address,undefined.
//
//   jpeg_entropy_main SEED MUTATE FILE...
//
// Every FILE is decoded by the host decoder and packed by tmr_jpeg_scan_pack; a packed scan then
// goes through the scheme at sub_bits 64, 256 and the default.  With MUTATE = 1 the first FILE
// also goes through all that as every prefix of itself and with each single byte replaced by
// 0x00, 0xFF and a value from a generator seeded with SEED.  Inputs, bits, tables, states and
// coefficients sit in heap blocks of exactly their sizes, so a read or write past any is reported.
// For every input: the pack status is the probe's, or "host pass"; the scheme's status is
// non-zero exactly when the host decoder's is; and where both are 0 the coefficients are equal.
// Exit 0 when all of that held; the last line counts what was seen.
#define TMR_HOST_ONLY
#include "../tmrnet_amd/csrc/jpeg_entropy.h"

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

void tmr_set_error(const char* fmt, ...) {   // the library's is in api.cpp, which needs HIP
  static thread_local char msg[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(msg, sizeof(msg), fmt, ap);
  va_end(ap);
}

static const uint8_t kZigzag[64] = JE_ZIGZAG;
static long g_inputs = 0, g_device_ok = 0, g_device_refused = 0, g_host_pass = 0, g_not_packed = 0;
static long g_max_rounds = 0;

// jpeg_entropy.hip's entropy_k for one frame, lanes in a loop.  Returns the status word.
static int scheme(const tmr_jpeg_scan_desc& d, const uint32_t* words, const tmr_jpeg_huff* tabs,
                  const je::Geom& g, uint32_t sub, int16_t* coef) {
  je::Scan sc;
  sc.words = words;
  sc.nbits = d.nbits;
  sc.tabs = tabs;
  sc.dcsel = sc.acsel = 0;
  for (int c = 0; c < g.ncomp; ++c) {
    if (d.dc_table[c] >= d.ntables || d.ac_table[c] >= d.ntables) return 3;
    sc.dcsel |= (uint32_t)d.dc_table[c] << (8 * c);
    sc.acsel |= (uint32_t)d.ac_table[c] << (8 * c);
  }
  const uint32_t nbits = d.nbits, nsub = nbits ? (nbits + sub - 1) / sub : 1;
  uint32_t* st = (uint32_t*)malloc((size_t)nsub * 5 * sizeof(uint32_t));
  uint32_t *sp = st, *ssk = sp + nsub, *ep = ssk + nsub, *esk = ep + nsub, *cnt = esk + nsub;
  memset(coef, 0, (size_t)g.total * 128);
  for (uint32_t i = 0; i < nsub; ++i) {
    sp[i] = i * sub;
    ssk[i] = je::kDirty;
  }
  uint32_t r = 0;
  for (; r < nsub; ++r) {
    for (uint32_t i = 0; i < nsub; ++i) {
      const uint32_t sk = ssk[i];
      if (!(sk & je::kDirty)) continue;
      je::sync_sub(sc, g, sp[i], sk & ~je::kDirty, je::sub_limit(nbits, sub, i), &ep[i], &esk[i], &cnt[i]);
      ssk[i] = sk & ~je::kDirty;
    }
    int changed = 0;
    for (uint32_t i = 1; i < nsub; ++i) {
      if (ep[i - 1] != sp[i] || esk[i - 1] != ssk[i]) {
        sp[i] = ep[i - 1];
        ssk[i] = esk[i - 1] | je::kDirty;
        changed = 1;
      }
    }
    if (!changed) break;
  }
  if ((long)r > g_max_rounds) g_max_rounds = r;
  uint32_t run = 0;
  for (uint32_t i = 0; i < nsub; ++i) {
    const uint32_t n = cnt[i];
    cnt[i] = run;
    run += n;
  }
  int err = 0, done = 0;
  for (uint32_t i = 0; i < nsub; ++i)
    je::write_sub(sc, g, sp[i], ssk[i], je::sub_limit(nbits, sub, i), cnt[i], coef, kZigzag, &err, &done);
  for (int c = 0; c < g.ncomp; ++c) {
    uint32_t pred = 0;
    for (uint32_t j = 0; j < je::comp_blocks(g, c); ++j) {
      const uint32_t at = je::dc_index(g, c, j);
      pred += (uint32_t)(int)coef[at];
      coef[at] = (int16_t)(uint16_t)pred;
    }
  }
  free(st);
  return err ? 2 : (done ? 0 : 1);
}

static bool one(const uint8_t* src, size_t len) {
  ++g_inputs;
  uint8_t* data = (uint8_t*)malloc(len ? len : 1);
  if (len) memcpy(data, src, len);
  tmr_jpeg_info info, pinfo;
  memset(&info, 0, sizeof(info));
  bool ok = true;

  // pack into buffers of the documented capacity, then move to blocks of the exact sizes
  const size_t cap = TMR_JPEG_SCAN_CAP(len);
  uint8_t* bits_cap = (uint8_t*)malloc(cap);
  tmr_jpeg_huff* tabs_cap = (tmr_jpeg_huff*)malloc(TMR_JPEG_MAX_TABLES * sizeof(tmr_jpeg_huff));
  tmr_jpeg_scan_desc d;
  const int rp = tmr_jpeg_scan_pack(data, len, &pinfo, bits_cap, cap, 0, tabs_cap,
                                    TMR_JPEG_MAX_TABLES * sizeof(tmr_jpeg_huff), 0, &d);
  const int rprobe_stage = rp;
  if (rp != 0 && rp != 1 && rp != 2 && rp != TMR_JPEG_HOST_PASS) {
    fprintf(stderr, "pack status %d\n", rp);
    ok = false;
  }
  if (rp == TMR_JPEG_HOST_PASS) ++g_host_pass;
  if (rp == 1 || rp == 2) ++g_not_packed;

  if (ok && rp == 0 && pinfo.coef_bytes > 0 && pinfo.coef_bytes <= (64u << 20)) {
    const size_t nb = (size_t)pinfo.coef_bytes;
    int16_t* want = (int16_t*)malloc(nb);
    const int rh = tmr_jpeg_entropy_decode(data, len, &info, want, nb);
    if (rh != 0 && rh != 1) {
      fprintf(stderr, "host status %d after pack status 0\n", rh);
      ok = false;
    }
    je::Geom g;
    if (!je::make_geom(d.height, d.width, d.sampling, &g) || (size_t)g.total * 128 != nb ||
        d.mcu_blocks != g.nslots || d.ntables < 1 || d.ntables > TMR_JPEG_MAX_TABLES ||
        d.bits_bytes != TMR_JPEG_SCAN_CAP(d.nbits / 8) || d.bits_bytes > cap) {
      fprintf(stderr, "descriptor does not fit the probe\n");
      ok = false;
    }
    if (ok) {
      uint32_t* words = (uint32_t*)malloc(d.bits_bytes);
      memcpy(words, bits_cap, d.bits_bytes);
      tmr_jpeg_huff* tabs = (tmr_jpeg_huff*)malloc((size_t)d.ntables * sizeof(tmr_jpeg_huff));
      memcpy(tabs, tabs_cap, (size_t)d.ntables * sizeof(tmr_jpeg_huff));
      const uint32_t subs[3] = {64, 256, je::kDefaultSubBits};
      for (int s = 0; s < 3 && ok; ++s) {
        int16_t* coef = (int16_t*)malloc(nb);
        memset(coef, 0x5a, nb);
        const int rd = scheme(d, words, tabs, g, subs[s], coef);
        if ((rd != 0) != (rh != 0)) {
          fprintf(stderr, "sub_bits %u: scheme status %d, host status %d\n", subs[s], rd, rh);
          ok = false;
        } else if (rd == 0 && memcmp(coef, want, nb) != 0) {
          fprintf(stderr, "sub_bits %u: coefficients differ from the host decoder's\n", subs[s]);
          ok = false;
        }
        if (ok && s == 0) ++(rd == 0 ? g_device_ok : g_device_refused);
        free(coef);
      }
      free(tabs);
      free(words);
    }
    free(want);
  } else if (ok) {
    // what the probe stage refuses, the host decoder refuses with the same status
    tmr_jpeg_info again;
    int16_t dummy[64];
    const int rh = tmr_jpeg_entropy_decode(data, len, &again, dummy, 0);
    if ((rprobe_stage == 1 || rprobe_stage == 2) && rh != rprobe_stage) {
      fprintf(stderr, "pack status %d, host status %d\n", rprobe_stage, rh);
      ok = false;
    }
  }
  free(tabs_cap);
  free(bits_cap);
  free(data);
  return ok;
}

static bool read_file(const char* path, std::vector<uint8_t>* out) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  uint8_t buf[4096];
  size_t n;
  out->clear();
  while ((n = fread(buf, 1, sizeof(buf), f)) > 0) out->insert(out->end(), buf, buf + n);
  fclose(f);
  return true;
}

int main(int argc, char** argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: %s SEED MUTATE FILE...\n", argv[0]);
    return 2;
  }
  uint64_t rng = strtoull(argv[1], 0, 10) * 2 + 1;
  const bool mutate = atoi(argv[2]) != 0;
  std::vector<uint8_t> d;
  for (int i = 3; i < argc; ++i) {
    if (!read_file(argv[i], &d)) {
      fprintf(stderr, "cannot read %s\n", argv[i]);
      return 2;
    }
    if (!one(d.data(), d.size())) {
      fprintf(stderr, "failed on %s\n", argv[i]);
      return 1;
    }
    if (i != 3 || !mutate) continue;
    for (size_t n = 0; n < d.size(); ++n)
      if (!one(d.data(), n)) {
        fprintf(stderr, "failed on the %zu-byte prefix of %s\n", n, argv[i]);
        return 1;
      }
    std::vector<uint8_t> m(d);
    for (size_t k = 0; k < d.size(); ++k) {
      rng = rng * 6364136223846793005ull + 1442695040888963407ull;
      const uint8_t vals[3] = {0x00, 0xFF, (uint8_t)(rng >> 56)};
      for (int v = 0; v < 3; ++v) {
        m[k] = vals[v];
        if (!one(m.data(), m.size())) {
          fprintf(stderr, "failed with byte %zu of %s set to %d\n", k, argv[i], vals[v]);
          return 1;
        }
      }
      m[k] = d[k];
    }
  }
  printf("inputs %ld: device ok %ld, device refused %ld, host pass %ld, not packed %ld, max rounds %ld\n",
         g_inputs, g_device_ok, g_device_refused, g_host_pass, g_not_packed, g_max_rounds);
  return 0;
}
