// arena_main.cpp -- OsfmArena (opensfm_amd/csrc/osfm_internal.h) against tests/native/hipemu, as a stand-alone program under
// AddressSanitizer and UndefinedBehaviorSanitizer (test infrastructure only: tests/test_arena.py builds and runs it with emu_ctx.cpp).
// For every size list: the total is the sum of the 256-rounded sizes, and every non-empty buffer is 256-aligned, lies inside the block
// and is disjoint from every other; an arena of the same shape made after the first is released gets the cached block back.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "osfm_internal.h"

static int g_failed = 0;
#define CHECK(cond, ...)                        \
  do {                                          \
    if (!(cond)) {                              \
      printf("FAILED %s: ", #cond);             \
      printf(__VA_ARGS__);                      \
      printf("\n");                             \
      g_failed++;                               \
    }                                           \
  } while (0)

struct Made {
  void *base;
  size_t block_bytes;
};

// one arena over `sizes` (bytes, declared as char buffers); every buffer is written in full, so that the sanitizer sees a slot that
// leaves the block
static Made check_list(osfm_ctx *ctx, const std::vector<size_t> &sizes, int list) {
  OsfmArena A;
  std::vector<OsfmArena::Slot<char>> slots;
  size_t want = 0;
  for (size_t bytes : sizes) {
    slots.push_back(A.add<char>(bytes));
    want += (bytes + 255) / 256 * 256;
  }
  CHECK(A.total == want, "list %d: total %zu, the rounded sizes sum to %zu", list, A.total, want);
  CHECK(slots[0].get() == nullptr, "list %d: a pointer before the allocation", list);
  CHECK(A.alloc(ctx) == hipSuccess, "list %d: alloc", list);
  const uintptr_t base = (uintptr_t)A.block.p;
  CHECK(A.block.bytes >= want, "list %d: block of %zu bytes for %zu", list, A.block.bytes, want);
  for (size_t i = 0; i < sizes.size(); i++) {
    CHECK(slots[i].bytes == sizes[i], "list %d slot %zu: %zu bytes, asked for %zu", list, i, slots[i].bytes, sizes[i]);
    if (!sizes[i]) continue;
    const uintptr_t at = (uintptr_t)slots[i].get();
    CHECK(at % 256 == 0, "list %d slot %zu: not 256-aligned", list, i);
    CHECK(at >= base && at + sizes[i] <= base + want, "list %d slot %zu: outside the block", list, i);
    for (size_t j = 0; j < i; j++) {
      if (!sizes[j]) continue;
      const uintptr_t other = (uintptr_t)slots[j].get();
      CHECK(at + sizes[i] <= other || other + sizes[j] <= at, "list %d: slots %zu and %zu overlap", list, j, i);
    }
    memset(slots[i].get(), (int)i, sizes[i]);
  }
  // typed buffers: the handle carries the element type and the bytes
  OsfmArena T;
  const auto d_off = T.add<int64_t>(3);
  const auto d_flag = T.add<int>(4);
  CHECK(d_off.bytes == 24 && d_flag.offset == 256 && d_flag.bytes == 16 && T.total == 512, "list %d: typed handles", list);
  return Made{A.block.p, A.block.bytes};
}

int main() {
  osfm_ctx *ctx = nullptr;
  if (osfm_ctx_create(0, &ctx) != OSFM_OK) return 2;
  const std::vector<std::vector<size_t>> lists = {
      {0, 1, 255, 256, 257},        // a zero first
      {1, 255, 0, 256, 257},        // in the middle
      {257, 256, 255, 1, 0},        // last
      {0, 0, 300, 0, 0, 1, 0},      // runs of zeros
      {256},
      {0},                          // nothing at all: the pooled buffer's 16-byte minimum
      {1000003, 0, 4096, 1, 0, 77}  // a larger block
  };
  for (size_t l = 0; l < lists.size(); l++) {
    for (auto &b : ctx->pool) (void)hipFree(b.p);  // an empty cache for every list
    ctx->pool.clear();
    ctx->pool_bytes = 0;
    const Made first = check_list(ctx, lists[l], (int)l);
    // the first arena has gone back to the context's cache: the same shape takes that block, not a new one
    const size_t cached = ctx->pool.size();
    CHECK(cached == 1 && ctx->pool_bytes == first.block_bytes, "list %zu: %zu blocks cached", l, cached);
    const Made second = check_list(ctx, lists[l], (int)l);
    CHECK(second.base == first.base && second.block_bytes == first.block_bytes, "list %zu: the cached block did not come back", l);
    CHECK(ctx->pool.size() == cached, "list %zu: %zu cached blocks, %zu before", l, ctx->pool.size(), cached);
  }
  osfm_ctx_destroy(ctx);
  if (g_failed) return 1;
  printf("OK %zu lists\n", lists.size());
  return 0;
}
