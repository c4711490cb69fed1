// Stand-alone driver of the host JPEG entropy decoder (tmrnet_amd/csrc/jpeg_host.cpp) for the
// host sanitizers: tests/test_jpeg_cpu.py builds it with -fsanitize=address,undefined, linked
// with jpeg_host.cpp alone, and runs it on the fixture files.
//
//   jpeg_host_main SEED MUTATE_FILE FILE...
//
// Every FILE goes through tmr_jpeg_probe and tmr_jpeg_entropy_decode once.  MUTATE_FILE also goes
// through them as every prefix of itself and with each single byte replaced by 0x00, 0xFF and a
// value from a generator seeded with SEED.  Each input sits in a heap block of exactly its size
// and the coefficients in one of exactly coef_bytes, so a read or write past either is reported.
// Exit 0 when every call returned 0, 1 or 2.
#define TMR_HOST_ONLY
#include "tmr.h"

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

static long g_calls = 0, g_status[3] = {0, 0, 0};

static bool one(const uint8_t* src, size_t len) {
  uint8_t* data = (uint8_t*)malloc(len ? len : 1);
  if (len) memcpy(data, src, len);
  tmr_jpeg_info info;
  memset(&info, 0, sizeof(info));
  const int rc = tmr_jpeg_probe(data, len, &info);
  bool ok = rc >= 0 && rc <= 2;
  ++g_calls;
  if (ok) ++g_status[rc];
  // decode also what the probe refused for its missing end marker; skip absurd header sizes
  if (ok && info.coef_bytes > 0 && info.coef_bytes <= (64u << 20)) {
    const size_t nb = (size_t)info.coef_bytes;
    int16_t* coef = (int16_t*)malloc(nb);
    tmr_jpeg_info again;
    memset(&again, 0, sizeof(again));
    const int rd = tmr_jpeg_entropy_decode(data, len, &again, coef, nb);
    ++g_calls;
    ok = rd >= 0 && rd <= 2;
    if (ok) ++g_status[rd];
    if (rd == 0) {   // every coefficient written: reading them all trips nothing
      long sum = 0;
      for (size_t i = 0; i < nb / 2; ++i) sum += coef[i];
      if (sum == 0x7fffffffffffffffL) printf("\n");
    }
    free(coef);
  }
  free(data);
  if (!ok) fprintf(stderr, "status outside 0..2 (probe %d)\n", rc);
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
  if (argc < 3) {
    fprintf(stderr, "usage: %s SEED MUTATE_FILE FILE...\n", argv[0]);
    return 2;
  }
  uint64_t rng = strtoull(argv[1], 0, 10) * 2 + 1;
  std::vector<uint8_t> d;
  for (int i = 2; i < argc; ++i) {
    if (!read_file(argv[i], &d)) {
      fprintf(stderr, "cannot read %s\n", argv[i]);
      return 2;
    }
    if (!one(d.data(), d.size())) return 1;
    if (i != 2) continue;
    for (size_t n = 0; n < d.size(); ++n)
      if (!one(d.data(), n)) return 1;
    std::vector<uint8_t> m(d);
    for (size_t k = 0; k < d.size(); ++k) {
      rng = rng * 6364136223846793005ull + 1442695040888963407ull;
      const uint8_t vals[3] = {0x00, 0xFF, (uint8_t)(rng >> 56)};
      for (int v = 0; v < 3; ++v) {
        m[k] = vals[v];
        if (!one(m.data(), m.size())) return 1;
      }
      m[k] = d[k];
    }
  }
  printf("calls %ld: ok %ld, malformed %ld, unsupported %ld\n", g_calls, g_status[0], g_status[1],
         g_status[2]);
  return 0;
}
