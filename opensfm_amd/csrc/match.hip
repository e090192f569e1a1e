// match.hip -- fused descriptor distance + top-2 + Lowe ratio + mutual check for gfx950 (MI355X).
//
// Replaces, per image pair, the cv2 calls under opensfm/matching.py:723-777
// (match_brute_force / match_brute_force_symmetric): an n1 x n2 x 128 distance computation, the
// two nearest neighbours of every feature in BOTH directions, the ratio test and the set
// intersection -- in ONE kernel, one workgroup at a time per pair (the fused kernels: a resident grid of
// workgroups that draw their pairs by ticket).  The n1 x n2 distance matrix never leaves the register file.
//
// Arithmetic (exact, integer): descriptors are integer-valued in [0,255] (features.py:526-534);
// stored as int8 a' = a - 128.  d^2(a,b) = |a'|^2 + |b'|^2 - 2 a'.b'  with a'.b' from
// v_mfma_i32_32x32x32_i8.  All quantities are exact int32, so the result is bit-identical to the
// fp32 computation cv2 performs (every partial sum < 2^24).
//
// Reduction: "best-only + lazy exact second" (see query_pass below).  The second-nearest neighbour is only needed for the
// ratio test, and only its VALUE; per query and class of 32 targets only the best accumulator value is kept, the norm of the
// target riding in the accumulator seed.  Classes are merged into (best, second-largest class best =: s_c); the true second s
// satisfies s >= s_c and the ratio test is monotone in d2: fails with s_c => fails (final, the vast majority); passes with
// s_c => the winner's own class is re-examined exactly with v_dot4 dot products.
// (Earlier generations -- exact top-2 in both directions 0.16, both directions per pass 0.24, one direction per pass with packed
// keys 0.39 of the int8 peak, profiles/r01_*, r02_bench_mid.json -- were removed; the exact VALU kernel below remains as the
// on-GPU cross-check.)
#include "osfm_internal.h"

#ifdef OSFM_DBG_PHASES
// instrumented builds only (tools/match_phases.py): 100 MHz ticks of workgroup thread 0, summed over the workgroups
__device__ unsigned long long g_phase[22];
#define OSFM_TICK(var) const unsigned long long var = wall_clock64();
#define OSFM_PHASE(i, t0, t1) if (threadIdx.x == 0) atomicAdd(&g_phase[i], (t1) - (t0));
extern "C" int osfm_dbg_phases(unsigned long long *out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phase), sizeof(g_phase)) != hipSuccess) return 1;
  if (reset) {
    unsigned long long z[22] = {};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_phase), z, sizeof(z)) != hipSuccess) return 1;
  }
  return 0;
}
#else
#define OSFM_TICK(var)
#define OSFM_PHASE(i, t0, t1)
#endif

#include "match_sweep.h"

namespace {

template <bool FQ>
__global__ void __launch_bounds__(kThreads, 2) match_fused_kernel(MatchArgs a) {
  constexpr int SHAPE = 32;
#include "match_pair_loop.inc"
}

// ---------------------------------------------------------------------------------------------
// Exact kernel: float-key semantics of cv2 (top-2 selected on sqrtf(d^2) with lowest-index
// ties), VALU only.  Used (a) for the rare pairs whose second-nearest d^2 >= 2^22, where distinct
// integers may round to the same float distance, and (b) as an on-GPU cross-check of the fused
// kernel.  One workgroup per pair, one thread per query feature.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void load_row(const int8_t *tiles, int row, v4i out[8]) {
  const int8_t *t = tiles + (long)(row >> 5) * OSFM_TILE_BYTES + (row & 31) * 16;
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    out[2 * ks] = *(const v4i *)(t + ks * 1024);
    out[2 * ks + 1] = *(const v4i *)(t + ks * 1024 + 512);
  }
}

__device__ void exact_direction(const int8_t *tilesQ, const int32_t *normQ, int nQ, const int8_t *tilesT,
                                const int32_t *normT, int nT, double ratio, int tid, int *res_int,
                                unsigned short *res_u16, const float *segQ, const float *segT) {
  for (int q = tid; q < nQ; q += kThreads) {
    v4i qa[8];
    load_row(tilesQ, q, qa);
    const int nq = normQ[q];
    const float sq = segQ ? segQ[q] : 0.f;
    float bd0 = INFINITY, bd1 = INFINITY;
    int bi0 = kNone;
    for (int t = 0; t < nT; ++t) {
      v4i ta[8];
      load_row(tilesT, t, ta);
      int sdot = 0;
#pragma unroll
      for (int k = 0; k < 8; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) sdot = __builtin_amdgcn_sdot4(qa[k][e], ta[k][e], sdot, false);
      const int d2i = nq + normT[t] - 2 * sdot;
      float d2f = (float)d2i;  // exact: < 2^24
      if (segQ) {  // the 129th dimension as cv2's normL2Sqr_ adds it: the scalar tail after the vector blocks, d += t * t (no contraction)
        const float ts = sq - segT[t];
        const float tt = ts * ts;
        d2f = d2f + tt;
      }
      const float d = ratio < 0.0 ? d2f : sqrtf(d2f);  // squared mode: FLANN reports and compares squared distances
      if (d < bd1) {  // cv2 batchDistance K=2 insertion
        if (bd0 > d) {
          bd1 = bd0;
          bd0 = d;
          bi0 = t;
        } else {
          bd1 = d;
        }
      }
    }
    const bool ok = ratio < 0.0 ? (bd0 < (float)(-ratio) * bd1) : ((double)bd0 < ratio * (double)bd1);
    const int v = ok ? bi0 : kNone;
    if (res_int) res_int[q] = v;
    if (res_u16) res_u16[q] = (unsigned short)v;
  }
}

__global__ void __launch_bounds__(kThreads) match_exact_kernel(MatchArgs a, int only_flagged) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int *colBI = (int *)smem;
  unsigned short *rowres = (unsigned short *)(colBI + a.ncap);
  int *misc = (int *)(rowres + a.ncap);
  const int tid = threadIdx.x;
  const long p = blockIdx.x;
  if (only_flagged && a.out_flags[p] == 0) return;
  const bool qs = !a.symmetric && a.query_second;  // queries = the pair's second image (match_flann)
  const int imgC = a.pairs[2 * p + (qs ? 1 : 0)], imgR = a.pairs[2 * p + (qs ? 0 : 1)];
  const int nC = a.counts[imgC], nR = a.counts[imgR];
  if (nC < 2 || nR < 2) {
    if (tid == 0) a.out_counts[p] = 0;
    return;
  }
  const int8_t *tilesC = a.tiles + a.tile_off[imgC] * OSFM_TILE_BYTES;
  const int8_t *tilesR = a.tiles + a.tile_off[imgR] * OSFM_TILE_BYTES;
  const int32_t *normC = a.norms + a.tile_off[imgC] * 32;
  const int32_t *normR = a.norms + a.tile_off[imgR] * 32;
  const float *segC = a.seg ? a.seg + a.tile_off[imgC] * 32 : nullptr, *segR = a.seg ? a.seg + a.tile_off[imgR] * 32 : nullptr;
  exact_direction(tilesC, normC, nC, tilesR, normR, nR, a.ratio, tid, colBI, nullptr, segC, segR);
  if (a.symmetric) exact_direction(tilesR, normR, nR, tilesC, normC, nC, a.ratio, tid, nullptr, rowres, segR, segC);
  __syncthreads();
  emit_matches(a, p, nC, colBI, rowres, misc, tid, qs);
}

// ---------------------------------------------------------------------------------------------
// Float kernel: descriptors that are not integers in [0, 255] (root-SIFT ...; opensfm/features.py:292-298 with feature_root).
// cv2's float semantics as the oracle restates them (oracle/match_oracle.c): squared distance accumulated in four
// 8-lane float vectors over blocks of 32 dimensions (normL2Sqr_ on an AVX2 build), reduced (d0 + d1) + (d2 + d3) and then
// ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7)); sqrtf; K = 2 insertion with the lowest index first among equals; Lowe's
// test in doubles (squared mode: in float on the squared distances).  Every float operation is the oracle's, in its order
// (-ffp-contract=off), so the result is bit-identical -- on the VALU: one thread per query with its descriptor in registers,
// the targets staged through LDS 32 at a time and read as broadcasts.  ~13 k pairs/s at 2000 x 2000: the functional path for
// float descriptors; a half-precision MFMA candidate pass with an exact re-examination is the planned fast one.
// ---------------------------------------------------------------------------------------------
constexpr int kFloatTileFloats = 32 * OSFM_DESC_DIM;

__device__ void float_direction(const float *descQ, int nQ, const float *descT, int nT, double ratio, int tid, float *stage, int *res_int,
                                unsigned short *res_u16) {
  const int tT = (nT + 31) >> 5;
  for (int q0 = 0; q0 < nQ; q0 += kThreads) {
    const int q = q0 + tid;
    const bool live = q < nQ;
    float qa[OSFM_DESC_DIM];
#pragma unroll
    for (int k4 = 0; k4 < OSFM_DESC_DIM; k4 += 4) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (live) v = *(const float4 *)(descQ + (size_t)q * OSFM_DESC_DIM + k4);
      qa[k4] = v.x;
      qa[k4 + 1] = v.y;
      qa[k4 + 2] = v.z;
      qa[k4 + 3] = v.w;
    }
    float bd0 = INFINITY, bd1 = INFINITY;
    int bi0 = kNone;
    for (int tt = 0; tt < tT; ++tt) {
      __syncthreads();
      for (int k = tid * 4; k < kFloatTileFloats; k += kThreads * 4) *(float4 *)(stage + k) = *(const float4 *)(descT + (size_t)tt * kFloatTileFloats + k);
      __syncthreads();
      const int nt = min(32, nT - tt * 32);
      for (int t = 0; t < nt; ++t) {
        const float *b = stage + t * OSFM_DESC_DIM;
        float acc[4][8];
#pragma unroll
        for (int v = 0; v < 4; ++v)
#pragma unroll
          for (int l = 0; l < 8; ++l) acc[v][l] = 0.f;
#pragma unroll
        for (int jb = 0; jb < OSFM_DESC_DIM; jb += 32)
#pragma unroll
          for (int v = 0; v < 4; ++v)
#pragma unroll
            for (int l4 = 0; l4 < 8; l4 += 4) {
              const float4 c = *(const float4 *)(b + jb + 8 * v + l4);
              const float cc[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const float d = qa[jb + 8 * v + l4 + e] - cc[e];
                const float sq = d * d;
                acc[v][l4 + e] = acc[v][l4 + e] + sq;
              }
            }
        float sv[8];
#pragma unroll
        for (int l = 0; l < 8; ++l) sv[l] = (acc[0][l] + acc[1][l]) + (acc[2][l] + acc[3][l]);
        const float sqd = ((sv[0] + sv[1]) + (sv[2] + sv[3])) + ((sv[4] + sv[5]) + (sv[6] + sv[7]));
        const float d = ratio < 0.0 ? sqd : sqrtf(sqd);
        if (d < bd1) {  // cv2 batchDistance K = 2 insertion
          if (bd0 > d) {
            bd1 = bd0;
            bd0 = d;
            bi0 = tt * 32 + t;
          } else {
            bd1 = d;
          }
        }
      }
    }
    if (live) {
      const bool ok = ratio < 0.0 ? (bd0 < (float)(-ratio) * bd1) : ((double)bd0 < ratio * (double)bd1);
      const int v = ok ? bi0 : kNone;
      if (res_int) res_int[q] = v;
      if (res_u16) res_u16[q] = (unsigned short)v;
    }
  }
}

__global__ void __launch_bounds__(kThreads) match_float_kernel(MatchArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float *stage = (float *)smem;  // 32 target descriptors
  int *colBI = (int *)(stage + kFloatTileFloats);
  unsigned short *rowres = (unsigned short *)(colBI + a.ncap);
  int *misc = (int *)(rowres + a.ncap);
  const int tid = threadIdx.x;
  const long p = blockIdx.x;
  if (tid == 0 && a.out_flags) a.out_flags[p] = 0;
  const bool qs = !a.symmetric && a.query_second;  // queries = the pair's second image (match_flann)
  const int imgC = a.pairs[2 * p + (qs ? 1 : 0)], imgR = a.pairs[2 * p + (qs ? 0 : 1)];
  const int nC = a.counts[imgC], nR = a.counts[imgR];
  if (nC < 2 || nR < 2) {
    if (tid == 0) a.out_counts[p] = 0;
    return;
  }
  const float *descC = a.descf + a.tile_off[imgC] * kFloatTileFloats;
  const float *descR = a.descf + a.tile_off[imgR] * kFloatTileFloats;
  float_direction(descC, nC, descR, nR, a.ratio, tid, stage, colBI, nullptr);
  if (a.symmetric) float_direction(descR, nR, descC, nC, a.ratio, tid, stage, nullptr, rowres);
  __syncthreads();
  emit_matches(a, p, nC, colBI, rowres, misc, tid, qs);
}

// ---------------------------------------------------------------------------------------------
// Hamming kernel: binary descriptors (uint8 bit strings; matching.py:737-740 switches cv2 to BruteForce-Hamming).  cv2's batchDistance
// with NORM_HAMMING gives int distances, the same K = 2 insertion (strict <, lowest index first among equals) and DMatch.distance =
// float(int); Lowe's test in doubles (matching.py:752).  Integer work, no matrix cores: one thread per query with its 512 bits in 16
// registers, the targets staged through LDS 256 rows at a time and read as broadcasts, v_bcnt_u32_b32 (popcount + add) per dword.
// ---------------------------------------------------------------------------------------------
constexpr int kHamStageRows = 256;

__device__ void hamming_direction(const uint32_t *binQ, int nQ, const uint32_t *binT, int nT, double ratio, int tid, uint32_t *stage, int *res_int,
                                  unsigned short *res_u16) {
  for (int q0 = 0; q0 < nQ; q0 += kThreads) {
    const int q = q0 + tid;
    const bool live = q < nQ;
    uint4 qa[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) qa[k] = live ? *(const uint4 *)(binQ + (size_t)q * 16 + 4 * k) : make_uint4(0u, 0u, 0u, 0u);
    int bd0 = 0x7fffffff, bd1 = 0x7fffffff, bi0 = kNone;
    for (int t0 = 0; t0 < nT; t0 += kHamStageRows) {
      const int nt = min(kHamStageRows, nT - t0);
      __syncthreads();
      for (int k = tid; k < nt * 4; k += kThreads) *(uint4 *)(stage + 4 * k) = *(const uint4 *)(binT + (size_t)t0 * 16 + 4 * k);
      __syncthreads();
      for (int t = 0; t < nt; ++t) {
        const uint4 *b = (const uint4 *)(stage + t * 16);
        int d = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint4 c = b[k];
          d += __popc(qa[k].x ^ c.x) + __popc(qa[k].y ^ c.y) + __popc(qa[k].z ^ c.z) + __popc(qa[k].w ^ c.w);
        }
        if (d < bd1) {  // cv2 batchDistance K = 2 insertion
          if (bd0 > d) {
            bd1 = bd0;
            bd0 = d;
            bi0 = t0 + t;
          } else {
            bd1 = d;
          }
        }
      }
    }
    if (live) {
      const bool ok = (double)(float)bd0 < ratio * (double)(float)bd1;  // DMatch.distance is float32 of the int; nT >= 2: both are set
      const int v = ok ? bi0 : kNone;
      if (res_int) res_int[q] = v;
      if (res_u16) res_u16[q] = (unsigned short)v;
    }
  }
}

__global__ void __launch_bounds__(kThreads) match_hamming_kernel(MatchArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint32_t *stage = (uint32_t *)smem;  // kHamStageRows target rows
  int *colBI = (int *)(stage + kHamStageRows * 16);
  unsigned short *rowres = (unsigned short *)(colBI + a.ncap);
  int *misc = (int *)(rowres + a.ncap);
  const int tid = threadIdx.x;
  const long p = blockIdx.x;
  if (tid == 0 && a.out_flags) a.out_flags[p] = 0;
  const bool qs = !a.symmetric && a.query_second;  // queries = the pair's second image (match_flann on bit strings, round 6)
  const int imgC = a.pairs[2 * p + (qs ? 1 : 0)], imgR = a.pairs[2 * p + (qs ? 0 : 1)];
  const int nC = a.counts[imgC], nR = a.counts[imgR];
  if (nC < 2 || nR < 2) {
    if (tid == 0) a.out_counts[p] = 0;
    return;
  }
  const uint32_t *binC = a.bin + a.tile_off[imgC] * (32 * 16);
  const uint32_t *binR = a.bin + a.tile_off[imgR] * (32 * 16);
  hamming_direction(binC, nC, binR, nR, a.ratio, tid, stage, colBI, nullptr);
  if (a.symmetric) hamming_direction(binR, nR, binC, nC, a.ratio, tid, stage, nullptr, rowres);
  __syncthreads();
  emit_matches(a, p, nC, colBI, rowres, misc, tid, qs);
}

}  // namespace

size_t osfm_match_lds_bytes(int ncap) { return (size_t)2 * kChunkBytes4 + 2 * kChunkCols4 * 4 + 128 + (size_t)ncap * 6; }

static int ensure_kernel_attributes(int device) {
  static OsfmPerDeviceOnce once;
  return once.run(device, []() -> int {
    OSFM_HIP(hipFuncSetAttribute((const void *)match_fused_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    OSFM_HIP(hipFuncSetAttribute((const void *)match_fused_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    OSFM_HIP(hipFuncSetAttribute((const void *)match_exact_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    OSFM_HIP(hipFuncSetAttribute((const void *)match_float_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    OSFM_HIP(hipFuncSetAttribute((const void *)match_hamming_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    return OSFM_OK;
  });
}

int osfm_launch_match(osfm_ctx *ctx, const osfm_store *store, const int32_t *d_pairs, int64_t n_pairs,
                      double ratio, int symmetric, int flags, int cap, int32_t *d_counts, uint32_t *d_matches,
                      int32_t *d_flags, bool exact_kernel, hipStream_t stream) {
  if (n_pairs == 0) return OSFM_OK;
  const int squared_ratio = (flags & OSFM_MATCH_SQUARED_RATIO) ? 1 : 0;
  MatchArgs a;
  a.tiles = store->d_tiles;
  a.norms = store->d_norms;
  a.hneg = store->d_hneg;
  a.descf = store->d_descf;
  a.qerr = store->d_qerr;
  a.seg = store->d_seg;
  a.bin = store->d_bin;
  a.tile_off = store->d_tile_off;
  a.counts = store->d_counts;
  a.pairs = d_pairs;
  a.n_pairs = n_pairs;
  // squared mode (FLANN semantics, matching.py:683-720): the kernels see -float32(ratio^2); one-way matching then queries
  // with the pair's second image, as match_flann(index1, f2) does
  a.ratio = squared_ratio ? -(double)(float)(ratio * ratio) : ratio;
  a.symmetric = symmetric;
  a.query_second = squared_ratio && !symmetric;
  a.cap = cap;
  a.ncap = ((store->max_count + 127) / 128) * 128;
  if (a.ncap < 128) a.ncap = 128;
  a.out_counts = d_counts;
  a.out_matches = d_matches;
  a.out_flags = d_flags;
  a.pad_tile = store->tile_off[store->n_images];
  a.tickets = nullptr;
  OSFM_REQUIRE(a.ncap <= OSFM_MAX_FEATURES, OSFM_E_UNSUPPORTED, "more than %d features in an image", OSFM_MAX_FEATURES);
  OSFM_REQUIRE(n_pairs < (1ll << 31), OSFM_E_INVALID, "too many pairs in one launch");
  OSFM_TRY(ensure_kernel_attributes(ctx->device));
  // the fused kernels run as a resident grid, two workgroups per CU, that hands the pairs out by ticket
  const bool fused = !store->is_binary && !store->d_seg && !exact_kernel && (!store->is_float || store->quantised);
  unsigned resident = 0;
  if (fused) {
    OSFM_REQUIRE(a.pad_tile < (1ll << 31), OSFM_E_UNSUPPORTED, "too many tiles in the store");
    OSFM_REQUIRE(ctx->num_cus > 0, OSFM_E_INVALID, "the context knows no compute units");
    // One ticket buffer per context, made on first use without a lock: every matcher launch of a context is enqueued by its
    // caller on ctx->stream (osfm_match_pairs' stream A), so this memset and the kernel that counts in the buffer are ordered
    // behind the previous launch's.  A second stream launching the fused matcher on the same context would need tickets of its own.
    if (!ctx->d_match_tickets) OSFM_HIP(hipMalloc(&ctx->d_match_tickets, 8 * kTicketStride * sizeof(int32_t)));
    OSFM_HIP(hipMemsetAsync(ctx->d_match_tickets, 0, 8 * kTicketStride * sizeof(int32_t), stream));
    a.tickets = (int32_t *)ctx->d_match_tickets;
    resident = (unsigned)std::min<int64_t>(n_pairs, 2 * (int64_t)ctx->num_cus);
  }
  if (store->is_binary) {
    // bit strings: Hamming distance on the VALU, every pair in one launch; nothing is ever flagged for a second run.
    // matcher_type FLANN on bit strings (round 6; cv2's LSH index searched EXACTLY, as the kd-forest is for floats): knnSearch returns int32
    // Hamming distances, so `dists[:, 0] < lowes_ratio ** 2 * dists[:, 1]` (matching.py:695-696) is a test in DOUBLES with the squared ratio --
    // the kernel's own test with that ratio (positive: nothing here takes a square root); one-way matching queries with the second image
    if (squared_ratio) a.ratio = ratio * ratio;
    if (exact_kernel && d_flags != nullptr) return OSFM_OK;
    const size_t lds = (size_t)kHamStageRows * 64 + (size_t)a.ncap * 6 + 64;
    hipLaunchKernelGGL(match_hamming_kernel, dim3((unsigned)n_pairs), dim3(kThreads), lds, stream, a);
  } else if (store->d_seg) {
    // segmentation column: every pair on the exact kernel with the label term (the int8 matrix path has no 129th dimension)
    if (exact_kernel && d_flags != nullptr) return OSFM_OK;  // "re-run the flagged pairs": none, the first launch was exact
    if (d_flags) OSFM_HIP(hipMemsetAsync(d_flags, 0, (size_t)n_pairs * sizeof(int32_t), stream));
    const size_t lds = (size_t)a.ncap * 6 + 64;
    hipLaunchKernelGGL(match_exact_kernel, dim3((unsigned)n_pairs), dim3(kThreads), lds, stream, a, 0);
  } else if (store->is_float) {
    // float store: the fused kernel on the 8-bit quantisation with rigorous bounds and float evaluation of what they leave open
    // (FQ mode); the exact float kernel for every pair when asked for (cross-check) or when the store could not be quantised.
    // Nothing is ever flagged for a second run: out_flags then counts the queries that went through the float evaluation.
    if (exact_kernel && d_flags != nullptr) return OSFM_OK;  // "re-run the flagged pairs": none
    if (!exact_kernel && store->quantised) {
      hipLaunchKernelGGL(match_fused_kernel<true>, dim3(resident), dim3(kThreads), osfm_match_lds_bytes(a.ncap), stream, a);
    } else {
      if (d_flags) OSFM_HIP(hipMemsetAsync(d_flags, 0, (size_t)n_pairs * sizeof(int32_t), stream));
      const size_t lds = (size_t)kFloatTileFloats * sizeof(float) + (size_t)a.ncap * 6 + 64;
      hipLaunchKernelGGL(match_float_kernel, dim3((unsigned)n_pairs), dim3(kThreads), lds, stream, a);
    }
  } else if (!exact_kernel) {
    // integer store: the sweep on v_mfma_i32_16x16x64_i8 (match16.hip), on which the chip holds a higher clock; the 32x32x32 kernel
    // (the one the float store runs) on request, as its cross-check
    if (flags & OSFM_MATCH_SWEEP_32X32)
      hipLaunchKernelGGL(match_fused_kernel<false>, dim3(resident), dim3(kThreads), osfm_match_lds_bytes(a.ncap), stream, a);
    else
      OSFM_TRY(osfm_launch_match_sweep16(ctx->device, a, resident, osfm_match_lds_bytes(a.ncap), stream));
  } else {
    const size_t lds = (size_t)a.ncap * 6 + 64;
    hipLaunchKernelGGL(match_exact_kernel, dim3((unsigned)n_pairs), dim3(kThreads), lds, stream, a, d_flags != nullptr ? 1 : 0);
  }
  OSFM_HIP(hipGetLastError());
  return OSFM_OK;
}
