// pool_bytes_host.cpp -- the context's OSFM_POOL_BYTES parsing (opensfm_amd/csrc/osfm_internal.h) compiled for the host against
// tests/native/hipemu (test infrastructure only: tests/test_pool_bytes.py)
#include "osfm_internal.h"

extern "C" int host_parse_pool_bytes(const char *s, unsigned long long *out) {
  size_t v = 0;
  if (!osfm_parse_pool_bytes(s, &v)) return 0;
  *out = v;
  return 1;
}
extern "C" unsigned long long host_pool_limit_from_env() { return osfm_ctx::pool_limit_from_env(); }
extern "C" unsigned long long host_default_pool_bytes() { return osfm_ctx::kPoolBytes; }
