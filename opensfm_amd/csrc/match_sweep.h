// match_sweep.h -- the shape-independent device code of the fused matcher: arguments, ratio test, the query pass ("targets in
// registers, queries in LDS") and the resident grid's tickets and pair headers; the kernel body that uses them (the loop over pairs) is
// match_pair_loop.inc.  Included by match.hip
// (v_mfma_i32_32x32x32_i8 sweep, SHAPE 32) and match16.hip (v_mfma_i32_16x16x64_i8 sweep, SHAPE 16); the includer defines
// OSFM_TICK / OSFM_PHASE first if it wants the instrumented phases.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "match16_maps.h"
#include "osfm_internal.h"

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

#ifndef OSFM_TICK
#define OSFM_TICK(var)
#define OSFM_PHASE(i, t0, t1)
#endif

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = 4;
constexpr int kRT = 2;                         // 32-row tiles per wave
constexpr int kNone = 0xFFFF;
constexpr int kCollisionD2 = 1 << 22;  // above this sqrtf() is no longer injective on integers

// Lowe ratio exactly as the reference evaluates it: float32 distances (cv2), compared in Python
// doubles: m.distance < ratio * n.distance (matching.py:752).  d^2 are exact ints < 2^24.
// Squared mode (ratio < 0 encodes it: -ratio is then float32(lowes_ratio^2)) is match_flann's test on SQUARED
// distances (matching.py:695-696): a numpy float32 array times a Python float stays float32, so
//     d0 < float32(ratio^2) * d1     with one float32 rounding of the product.
__device__ __forceinline__ bool ratio_ok(int d1sq, int d2sq, double ratio) {
  if (ratio < 0.0) return (float)d1sq < (float)(-ratio) * (float)d2sq;
  const float f1 = sqrtf((float)d1sq), f2 = sqrtf((float)d2sq);
  return (double)f1 < ratio * (double)f2;
}

__device__ __forceinline__ long xcd_remap(long b, long n) {
  // blocks are dealt round-robin to the 8 XCDs; give every XCD a contiguous range of pairs so
  // that the pairs in flight on one L2 share their first image (bijective for any n).
  const long q = n >> 3, r = n & 7;
  const long xcd = b & 7, within = b >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + within;
}

}  // namespace

// (a named type: match.hip fills it and hands it to match16.hip's launcher)
struct MatchArgs {
  const int8_t *tiles;
  const int32_t *norms;
  const int32_t *hneg;  // -ceil(norm / 2): accumulator seeds
  const float *descf;   // float store: row (tile * 32 + r) x 128
  const float *qerr;    // float store: per image, max residual norm of the 8-bit quantisation (quantised units)
  const int64_t *tile_off;
  const int32_t *counts;
  const int32_t *pairs;
  long n_pairs;
  double ratio;      // Lowe ratio; NEGATIVE = squared mode: -ratio is float32(lowes_ratio^2) (see ratio_ok)
  int symmetric;
  int query_second;  // one-way matching with the SECOND image as the query set (match_flann(index1, f2), matching.py:683-697)
  int cap;
  int ncap;  // LDS capacity (features), multiple of 128
  int32_t *out_counts;
  uint32_t *out_matches;
  int32_t *out_flags;
  long pad_tile;            // index of the store's first slack tile
  // read by the exact / Hamming kernels only; kept behind the fused kernel's arguments so that its kernarg layout (and with it the
  // register allocation tests/test_kernel_budgets.py pins) does not move
  const uint32_t *bin;  // binary store: 16 dwords per row (tile * 32 + r)
  const float *seg;     // segmentation column (129th descriptor dimension, label x 35) per row, or null
  // fused kernels only (behind the rest for the same reason): the ticket counters of the resident grid, one per XCD range of the
  // pair list, kTicketStride ints apart (a 128-byte line each); zeroed on the stream ahead of every launch
  int32_t *tickets;
};
// match16.hip: the fused kernel on the 16x16x64 sweep (integer store), as a resident grid of `grid` workgroups
int osfm_launch_match_sweep16(int device, const MatchArgs &a, unsigned grid, size_t lds_bytes, hipStream_t stream);

namespace {

constexpr int kTicketStride = 32;

// ---------------------------------------------------------------------------------------------
// Shared tail: ratio test on the column side, mutual check, ordered compaction.
// colBI[c] = row index of the best row for column c (or kNone), rowres[r] = best column for row r
// after the ratio test (or kNone).  Emits (c, r) sorted by c.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void emit_matches(const MatchArgs &a, long p, int nC, const int *colBI,
                                             const unsigned short *rowres, int *misc, int tid, bool swap_halves) {
  const int lane = tid & 63, w = tid >> 6;
  int base = 0;
  for (int j0 = 0; j0 < nC; j0 += kThreads) {
    const int j = j0 + tid;
    bool m = false;
    int r = kNone;
    if (j < nC) {
      r = colBI[j];
      m = (r != kNone) && (!a.symmetric || rowres[r] == j);
    }
    const unsigned long long bal = __ballot(m);
    const int prefix = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) misc[w] = __popcll(bal);
    __syncthreads();
    int woff = 0, total = 0;
#pragma unroll
    for (int w2 = 0; w2 < kWaves; ++w2) {
      const int cnt = misc[w2];
      woff += (w2 < w) ? cnt : 0;
      total += cnt;
    }
    if (m) {
      const int k = base + woff + prefix;
      // low half = feature of image 1, high half = feature of image 2
      if (k < a.cap) a.out_matches[p * a.cap + k] = swap_halves ? ((uint32_t)r | ((uint32_t)j << 16)) : ((uint32_t)j | ((uint32_t)r << 16));
    }
    base += total;
    __syncthreads();
  }
  if (tid == 0) a.out_counts[p] = base;
}

// a'.b' of two stored descriptors (tile layout): all 16 loads issued before the first use, one memory latency per candidate
__device__ __forceinline__ int dot_rows8(const int8_t *tilesA, int rowA, const int8_t *tilesB, int rowB) {
  const int8_t *pa = tilesA + (long)(rowA >> 5) * OSFM_TILE_BYTES + (rowA & 31) * 16;
  const int8_t *pb = tilesB + (long)(rowB >> 5) * OSFM_TILE_BYTES + (rowB & 31) * 16;
  v4i av[8], bv[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    av[q] = *(const v4i *)(pa + q * 512);
    bv[q] = *(const v4i *)(pb + q * 512);
  }
  int s0 = 0, s1 = 0;
#pragma unroll
  for (int q = 0; q < 8; q += 2)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      s0 = __builtin_amdgcn_sdot4(av[q][e], bv[q][e], s0, false);
      s1 = __builtin_amdgcn_sdot4(av[q + 1][e], bv[q + 1][e], s1, false);
    }
  return s0 + s1;
}

// a wave-uniform pointer, as the scalar registers the compiler does not always grant it: loads through it take the
// scalar-base + 32-bit lane offset form (no 64-bit address per lane to build, keep or spill)
template <class P>
__device__ __forceinline__ P *uniform_ptr(P *p) {
  const unsigned long long v = (unsigned long long)p;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  return (P *)(((unsigned long long)hi << 32) | lo);
}

__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = max(v, __shfl_xor(v, m));
  return v;
}

// max over the 16 lanes of a DPP row, in every lane of the row (no LDS traffic): quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror
__device__ __forceinline__ int row16_max(int x) {
  x = max(x, __builtin_amdgcn_update_dpp(x, x, 0xB1, 0xF, 0xF, false));
  x = max(x, __builtin_amdgcn_update_dpp(x, x, 0x4E, 0xF, 0xF, false));
  x = max(x, __builtin_amdgcn_update_dpp(x, x, 0x141, 0xF, 0xF, false));
  x = max(x, __builtin_amdgcn_update_dpp(x, x, 0x140, 0xF, 0xF, false));
  return x;
}

// ---------------------------------------------------------------------------------------------
// FQ mode of the fused kernel: float descriptors (root-SIFT ...) through the int8 matrix pipe with rigorous bounds.
// The store holds x^ = round(x) of x = (v - lo) * 255 / (hi - lo) - 128 next to the float rows, and per image E = max ||x - x^||.
// With D^ = ||x^_q - x^_t|| (an exact integer square root away) and D = scale * (the float32 distance cv2 computes),
//     | D - D^ |  <=  eps + kappa * D,      eps = E_Q + E_T   (triangle inequality; kappa covers the float32 roundings of the
//                                                               reference's accumulation: < 11 ulp on the squared sum)
// so the sweep's (best, class-level second) bounds decide most queries outright:
//     surely fails:   lower bound of the best   >= ratio * upper bound of the second     (the vast majority)
//     surely passes:  upper bound of the best   <  ratio * lower bound of the second, which also makes the integer winner the
//                     float winner (every other target is farther than the winner's upper bound)
// and whatever is left is evaluated in float32, operation for operation as the oracle / cv2 does (l2sqr_rows_f32), against every
// target whose quantised distance does not exclude it from the top two.  Results are bit-identical to the exact float kernel.
// ---------------------------------------------------------------------------------------------
constexpr double kFqSlack = 8e-6;
__device__ __forceinline__ double fq_ratio(double ratio) { return ratio < 0.0 ? sqrt(-ratio) : ratio; }  // squared mode compares d^2
__device__ __forceinline__ bool fq_surely_fails(int d0lo_sq, int d1hi_sq, double eps, double r) {
  const double D0lo = fmax(sqrt((double)max(d0lo_sq, 0)) - eps, 0.0) * (1.0 - kFqSlack);
  const double D1hi = (sqrt((double)max(d1hi_sq, 0)) + eps) * (1.0 + kFqSlack);
  return D0lo >= r * D1hi;
}
__device__ __forceinline__ bool fq_surely_passes(int d0hi_sq, int d1lo_sq, double eps, double r) {
  const double D0hi = (sqrt((double)max(d0hi_sq, 0)) + eps) * (1.0 + kFqSlack);
  const double D1lo = fmax(sqrt((double)max(d1lo_sq, 0)) - eps, 0.0) * (1.0 - kFqSlack);
  return D0hi < r * D1lo && D0hi < D1lo;
}
__device__ __forceinline__ float wave_minf(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fminf(v, __shfl_xor(v, m));
  return v;
}

// ---------------------------------------------------------------------------------------------
// Fused MFMA kernel: "one direction at a time".
//   pass A: the queries are the features of image A, the targets those of image B; resA[a] = best b if it passes the ratio test;
//   pass B: (symmetric matching only) the mutual check needs "best a for b" only for the b that some a chose: those candidates
//           (typically a small subset of image B) become the gathered queries of a second, much smaller pass against image A;
//   a pair (a, b) is emitted iff resA[a] == b and resB[b] == a.
// For symmetric matching A is the pair's SECOND image, so that the image whose row blocks every step re-reads is the first one,
// which the ~64 pairs in flight on an XCD share in L2 (xcd_remap).
// ---------------------------------------------------------------------------------------------
constexpr int kCT4 = 8;                              // a chunk stages 256 queries
constexpr int kChunkCols4 = kCT4 * 32;
constexpr int kChunkBytes4 = kCT4 * OSFM_TILE_BYTES;  // 32 KiB, double buffered

// ---------------------------------------------------------------------------------------------
// Version 5 of the pass: "targets in registers, queries in LDS, the norm in the accumulator".
//
// v4's pass is bounded by its integer epilogue (6.6 VALU per MFMA, profiles/r01_final_match_pmc.txt: VALU port 48 %, matrix pipe
// 45 %, and on gfx950 one integer VALU instruction of a 64-wide wave costs 5-6 cycles of a SIMD, profiles/r01_ubench_valu_issue.txt --
// more than the 32 cycles of the MFMA they follow).  Every one of those instructions builds or compares a key
// (2 a.b - |b|^2) * 2^k + tag.  v5 removes the key arithmetic:
//   * the QUERIES are the streamed operand (columns, one per lane), the TARGETS the register operand (rows, one per accumulator
//     register).  The quantity to maximise over the targets i of a query j is v = 2 a_i.b_j - |a_i|^2; the per-target constant now
//     belongs to a REGISTER, so it rides in the accumulator seed: the first MFMA of a K chain takes C = -ceil(|a_i|^2 / 2) (a
//     16-register tuple per row tile that stays put while the queries stream by), and the chain ends with
//     u = a_i.b_j - ceil(|a_i|^2 / 2), v = 2u + (|a_i|^2 & 1).  No shift, no add.
//   * per query and class (the 32 targets a lane sees in one step) only max u is kept: a v_max3 tree over the 32 accumulators,
//     then second = med3(best, m, second), class = m > best ? step : class, best = max(best, m): 20 VALU per 8 MFMAs.
//   * u orders v up to the parity bit, which is all the lazy scheme needs: the winner has u = max u; the other classes bound the
//     second neighbour between 2 s and 2 s + 1.  A query is final when the ratio test fails even with the most favourable of those
//     bounds (the vast majority); otherwise the winner's class (32 targets) is re-examined exactly with v_dot4, and if the answer
//     still depends on the unknown parity bit, or two classes tie, the query is re-done exactly against all targets.
//   * the chunk of 256 queries stays in LDS for the whole sweep over the targets, so there is no barrier, no DMA wait and no
//     merge inside the sweep: each wave streams its own target rows global -> VGPR one step ahead.
// Results are bit-identical to v4 / the exact kernel / the oracle (tests/test_gpu_matching.py).
// ---------------------------------------------------------------------------------------------
struct QueryPassShared {
  unsigned char *bbuf;  // [2][32 KiB] query chunks (tile layout); the drained one doubles as the merge scratch
  int *hbuf;            // [2][256] accumulator seeds of the row block in flight / the next one
};

// queries: slot q in [0, nslots) is feature qsel[q] of image Q (qsel == nullptr: identity); targets: all nT features of image T.
// out[query feature] = its nearest target if the ratio test passes, else kNone.  Returns the collision flag; any_hit = whether any
// query of the pass got a target (workgroup-uniform: the OR goes through *hit_word, an LDS word that is zero on entry, across the
// pass's closing barrier.  Not __syncthreads_or: the library's workgroup reduction brings static LDS of its own, and the kernel
// already asks for the whole 160 KiB as dynamic LDS).
// hooks: what the caller wants done under the pass, where a round trip to memory costs the pass nothing (the fused kernel fetches its
// next pair there): cold_issue() between the issue of the pass's first (cold) loads and the wait for them, cold_done() after that
// wait, chunk(c) behind the barrier that opens chunk c and ahead of every load of its sweep.
// SHAPE: 32 = v_mfma_i32_32x32x32_i8 (step), 16 = v_mfma_i32_16x16x64_i8 (step16, match16_maps.h); the pass around the step is the
// same but for the lane maps of the operand fragments, of the seeds and of the class re-examination.
template <bool GATHER, bool FQ, int SHAPE, class Hooks>
__device__ __forceinline__ int query_pass(const QueryPassShared &sh, const int8_t *tilesQ, const int32_t *normQ, int nQ, int nslots,
                                          const unsigned short *qsel, const int8_t *tilesT, const int32_t *normT, const int32_t *hnegT,
                                          int nT, const int8_t *tiles_pad, const int32_t *hneg_pad, unsigned short *out, double ratio,
                                          int tid, const float *descQ, const float *descT, double eps, int *hit_word, int &any_hit,
                                          Hooks &&hooks) {
  static_assert(SHAPE == 16 || SHAPE == 32, "the sweep knows v_mfma_i32_16x16x64_i8 (step16) and v_mfma_i32_32x32x32_i8 (step)");
  // the pass runs inside the fused kernel's loop over pairs: what it derives from the thread index is made per call, so that nothing
  // of it is hoisted out of that loop and kept in vector registers through the other pass's sweep
  asm volatile("" : "+v"(tid));
  asm volatile("" : "+s"(ratio));  // (likewise what the float store derives from the ratio in double precision)
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tT = (nT + 31) >> 5;
  const int tS = (nslots + 31) >> 5;
  const int nchunks = (tS + kCT4 - 1) / kCT4;
  const int nrb = (tT + kWaves * kRT - 1) / (kWaves * kRT);
  int flag = 0, hit = 0;

  // one chunk = 8 query tiles, global -> LDS by DMA; thread (w, lane) moves bytes [w*1024 + lane*16, +16) of every tile, i.e. the
  // K slice w of feature (lane & 31), half (lane >> 5) -- which is also how a gathered query is addressed
  auto dma_chunk = [&](int c) {
    unsigned char *dst = sh.bbuf + (c & 1) * kChunkBytes4;
#pragma unroll
    for (int q = 0; q < kCT4; ++q) {
      const int gt = c * kCT4 + q;
      const int8_t *src;
      if (GATHER) {
        const int slot = gt * 32 + (lane & 31);
        const int f = slot < nslots ? (int)qsel[slot] : 0;
        src = tilesQ + (long)(f >> 5) * OSFM_TILE_BYTES + w * 1024 + (lane >> 5) * 512 + (f & 31) * 16;
      } else {
        src = tilesQ + (long)(gt < tS ? gt : 0) * OSFM_TILE_BYTES + tid * 16;
      }
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                       (__attribute__((address_space(3))) void *)(dst + q * OSFM_TILE_BYTES + w * 1024), 16, 0, 0);
    }
  };

  // the wave's two target row tiles of row block rb.  Branch-free: a row tile beyond the image reads the store's slack tile (zero
  // descriptors, padding norms), whose seed -2^22 can never be a maximum.
  //   A operands: global -> VGPR, one step ahead, into the register set the running step does not use;
  //   accumulator seeds: global -> LDS by DMA (each wave stages the 64 seeds of its own two row tiles, so only its own vmcnt
  //   orders them), read into the seed tuples as soon as the running step has issued its last seeded MFMA.
  // A full step issues the three parts in the gaps of its own first tile, a partial one ahead of itself.
  auto load_seeds = [&](int rb, int slot) {
    const int t = rb * (kWaves * kRT) + w * kRT;  // wave-uniform: the halves of the wave stage one row tile each
    const int32_t *h0 = uniform_ptr((t < tT) ? hnegT + (long)t * 32 : hneg_pad);
    const int32_t *h1 = uniform_ptr((t + 1 < tT) ? hnegT + (long)(t + 1) * 32 : hneg_pad);
    const int32_t *hp = ((lane >> 5) ? h1 : h0) + (lane & 31);
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)hp,
                                     (__attribute__((address_space(3))) void *)(sh.hbuf + slot * 256 + w * 64), 4, 0, 0);
  };
  auto load_rows = [&](int rb, v4i (&af)[kRT][4], int rt) {
    const int t = rb * (kWaves * kRT) + w * kRT + rt;  // wave-uniform
    const auto *tp = (const __attribute__((address_space(1))) int8_t *)uniform_ptr((t < tT) ? tilesT + (long)t * OSFM_TILE_BYTES : tiles_pad);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)  // SHAPE 16: fragment ks = (sub-tile ks >> 1 of the row tile, K half ks & 1)
      af[rt][ks] = *(const __attribute__((address_space(1))) v4i *)(tp + (SHAPE == 16 ? osfm16_frag_offset(ks >> 1, ks & 1, lane) : ks * 1024 + lane * 16));
  };
  auto load_targets = [&](int rb, v4i (&af)[kRT][4], int slot) {
    load_seeds(rb, slot);  // the issue order (seeds, row tile 0, row tile 1) is what the vmcnt in the step's last tile counts on
    load_rows(rb, af, 0);
    load_rows(rb, af, 1);
  };
  v16i hn[kRT];
  // accumulator register r of half h belongs to row (r & 3) + 8 (r >> 2) + 4 h of the tile
  // (SHAPE 16: register r of lane group g belongs to row 4 g + r of a 16-row sub-tile: 16 seeds per lane, all in hn[0])
  auto read_seeds_rt = [&](int slot, int rt) {
    if constexpr (SHAPE == 16) {
      int g4 = (lane >> 4) * 4;  // made here every time: kept across the sweep it is one more register to spill
      asm volatile("" : "+v"(g4));
#pragma unroll
      for (int s = 2 * rt; s < 2 * rt + 2; ++s) {
        const v4i hv = *(const v4i *)(sh.hbuf + slot * 256 + w * 64 + 16 * s + g4);
        hn[0][4 * s + 0] = hv[0];
        hn[0][4 * s + 1] = hv[1];
        hn[0][4 * s + 2] = hv[2];
        hn[0][4 * s + 3] = hv[3];
      }
      return;
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const v4i hv = *(const v4i *)(sh.hbuf + slot * 256 + w * 64 + rt * 32 + 8 * g + 4 * (lane >> 5));
      hn[rt][4 * g + 0] = hv[0];
      hn[rt][4 * g + 1] = hv[1];
      hn[rt][4 * g + 2] = hv[2];
      hn[rt][4 * g + 3] = hv[3];
    }
  };
  auto read_seeds = [&](int slot) {
    read_seeds_rt(slot, 0);
    read_seeds_rt(slot, 1);
  };

  int cb[kCT4], cs[kCT4], ci[kCT4];
  const unsigned char *bb = sh.bbuf;
  v4i bf[4];  // B operands of the tile in flight; slice ks is refilled for the next tile as soon as both chains have consumed it

  // max over the 16 accumulators of one chain: two interleaved v_max3 chains
#define OSFM_TREE_A(X, A, B)             \
  A = max(max(X[0], X[1]), X[2]);        \
  B = max(max(X[8], X[9]), X[10]);
#define OSFM_TREE_B(X, A, B)             \
  A = max(max(A, X[3]), X[4]);           \
  B = max(max(B, X[11]), X[12]);
#define OSFM_TREE_C(X, A, B)             \
  A = max(max(A, X[5]), X[6]);           \
  B = max(max(B, X[13]), X[14]);
#define OSFM_TREE_D(X, A, B, M)          \
  M = max(max(A, B), X[7]);              \
  M = max(M, X[15]);
#define OSFM_PIN __builtin_amdgcn_sched_barrier(0);

  // One step = this wave's 64 targets (af, hn) against the 8 query tiles of the chunk: 64 MFMAs.  Per tile two K chains (one per row
  // tile) run interleaved on two of THREE accumulator tuples; the tuples of the previous tile are reduced in the issue gaps of the
  // current one (an in-order wavefront hides about five plain VALU instructions behind a 32-cycle MFMA, MI355X_MICROARCH.md), and the
  // first chain's tuple of tile t-1 becomes the second chain's tuple of tile t.  The class update of tile t-1 rides in the later gaps.
  //
  // Partial steps run only the tiles that exist, in the same pipeline:
  //   * a chunk with nt < 8 query tiles (the last one of an image or of the candidate list) ENTERS the unrolled tile sequence at
  //     t0 = 8 - nt: stage t works on query tile t - t0 (bq = the chunk's base moved back by t0 tiles), so the seed fetch in tile 7
  //     and the drain are the full step's.  The entry stage reduces whatever the tuples held into cb/cs/ci[t0 - 1], which the merge
  //     files under query tile 7 of the chunk -- one that does not exist when nt < 8, and whose slots nobody decides;
  auto step = [&](const v4i (&af)[kRT][4], v4i (&nxt)[kRT][4], int rb, int rbn, int next_slot, int t0, const unsigned char *bq) {
    const int vrb = rb;  // the class index of this step, in a vector register for the selects below
    v16i T[3];
    int mp = 0;
    asm volatile("; osfm-step: a step of the sweep begins (tests/test_kernel_budgets_sweep.py)");
#pragma unroll
    for (int t = 0; t < kCT4; ++t) {
      if (t == 0 && t0 > 0) {  // a partial step has no first tile to hide the fetch of the next step's targets in
        load_targets(rbn, nxt, next_slot);
        continue;
      }
      if (t < kCT4 - 1 && t < t0) continue;  // (t0 <= 7: the last stage always runs)
      // tile 7 prefetches the first tile of the next step
      const unsigned char *nb = (t == kCT4 - 1 ? bq + t0 * OSFM_TILE_BYTES : bq + (t + 1) * OSFM_TILE_BYTES) + lane * 16;
      v16i &C1 = T[(2 * t) % 3];
      v16i &C2 = T[(2 * t + 1) % 3];      // = chain 1 of tile t-1: reduced in the first gap
      v16i &P2 = T[(2 * t + 2) % 3];      // = chain 2 of tile t-1
      int a0 = 0, b0 = 0, a1 = 0, b1 = 0, m2 = 0;
      C1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[0][0], bf[0], hn[0], 0, 0, 0);
      OSFM_PIN
      if (t > 0) {
        OSFM_TREE_A(C2, a0, b0)
        OSFM_TREE_B(C2, a0, b0)
        OSFM_TREE_C(C2, a0, b0)
        OSFM_TREE_D(C2, a0, b0, mp)
      } else {
        load_seeds(rbn, next_slot);  // the next step's targets, in the gaps that have no previous tile to reduce
      }
      OSFM_PIN
      C2 = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[1][0], bf[0], hn[1], 0, 0, 0);
      OSFM_PIN
      if (t == kCT4 - 1) {
        // the step's last seeded MFMAs are out: fetch the next step's seeds.  Their DMA is older than the 8 A-operand loads this step
        // issued (and the 8 DMAs of the next chunk, issued ahead of the chunk's first step, are older still)
        __builtin_amdgcn_s_waitcnt(0x0F70 | (2 * kRT * 4));  // vmcnt(8)
        read_seeds_rt(next_slot, 0);
      }
      bf[0] = *(const v4i *)(nb);
      if (t > 0) { OSFM_TREE_A(P2, a1, b1) }
      OSFM_PIN
      C1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[0][1], bf[1], C1, 0, 0, 0);
      OSFM_PIN
      if (t > 0) { OSFM_TREE_B(P2, a1, b1) } else { load_rows(rbn, nxt, 0); }
      if (t == kCT4 - 1) read_seeds_rt(next_slot, 1);
      OSFM_PIN
      C2 = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[1][1], bf[1], C2, 0, 0, 0);
      OSFM_PIN
      bf[1] = *(const v4i *)(nb + 1024);
      if (t > 0) { OSFM_TREE_C(P2, a1, b1) }
      OSFM_PIN
      C1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[0][2], bf[2], C1, 0, 0, 0);
      OSFM_PIN
      if (t > 0) { OSFM_TREE_D(P2, a1, b1, m2) } else { load_rows(rbn, nxt, 1); }
      OSFM_PIN
      C2 = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[1][2], bf[2], C2, 0, 0, 0);
      OSFM_PIN
      bf[2] = *(const v4i *)(nb + 2048);
      if (t > 0) {
        m2 = max(m2, mp);
        asm("v_med3_i32 %0, %1, %2, %3" : "=v"(cs[t - 1]) : "v"(cb[t - 1]), "v"(m2), "v"(cs[t - 1]));  // cs <= cb: the second-largest of {cb, m, cs}
      }
      OSFM_PIN
      C1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[0][3], bf[3], C1, 0, 0, 0);
      OSFM_PIN
      // (as volatile assembly: left to the compiler, the eight selects of a step all sink into its last tile)
      if (t > 0)
        asm volatile("v_cmp_gt_i32 vcc, %1, %2\n\ts_nop 1\n\tv_cndmask_b32 %0, %0, %3, vcc" : "+v"(ci[t - 1]) : "v"(m2), "v"(cb[t - 1]), "v"(vrb) : "vcc");
      OSFM_PIN
      C2 = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[1][3], bf[3], C2, 0, 0, 0);
      OSFM_PIN
      bf[3] = *(const v4i *)(nb + 3072);
      if (t > 0) cb[t - 1] = max(cb[t - 1], m2);
      OSFM_PIN
    }
    {  // drain: the last tile's tuples
      v16i &Q1 = T[(2 * (kCT4 - 1)) % 3];
      v16i &Q2 = T[(2 * (kCT4 - 1) + 1) % 3];
      int a0, b0, a1, b1, m1, m2;
      OSFM_TREE_A(Q1, a0, b0)
      OSFM_TREE_B(Q1, a0, b0)
      OSFM_TREE_C(Q1, a0, b0)
      OSFM_TREE_D(Q1, a0, b0, m1)
      OSFM_TREE_A(Q2, a1, b1)
      OSFM_TREE_B(Q2, a1, b1)
      OSFM_TREE_C(Q2, a1, b1)
      OSFM_TREE_D(Q2, a1, b1, m2)
      m2 = max(m2, m1);
      asm("v_med3_i32 %0, %1, %2, %3" : "=v"(cs[kCT4 - 1]) : "v"(cb[kCT4 - 1]), "v"(m2), "v"(cs[kCT4 - 1]));
      ci[kCT4 - 1] = m2 > cb[kCT4 - 1] ? rb : ci[kCT4 - 1];
      cb[kCT4 - 1] = max(cb[kCT4 - 1], m2);
    }
  };

  // The same step on v_mfma_i32_16x16x64_i8: per query tile 16 MFMAs = 2 column sub-tiles c x 2 K halves h x 4 row sub-tiles s, issued
  // in the order (c, h, s), so that a chain's second MFMA follows its first at a distance of four.  THREE sets of four 4-register
  // accumulators (one column sub-tile each) rotate as the three tuples of the 32x32 step do: the sets of tile t-1 are reduced in the
  // gaps of tile t, and column sub-tile 0 of tile t-1, reduced first, is the set column sub-tile 1 of tile t accumulates into.  One or
  // two vector instructions per gap (an MFMA of this shape holds the vector issue for 8 of its 16 cycles):
  //   gaps 0-3 / 4-7: the v_max3 tree over the 16 accumulators of column sub-tile 0 / 1;
  //   gap 8: v_permlane16_swap of the two maxima, gap 9: one max.  Lane rows 0 and 2 then hold column sub-tile 0 with the targets of
  //          lane groups {0, 1} / {2, 3} merged, rows 1 and 3 column sub-tile 1: lane l holds query (l & 31) of the tile and class half
  //          (l >> 5), 32 targets per class -- the layout of cb / cs / ci, and of the chunk-end merge, of the 32x32 form;
  //   gaps 10-12: med3, compare + select, max.
  // The B fragment (c, h) is re-read for the next tile behind its fourth MFMA.  Partial steps enter at stage t0 as above.
  auto step16 = [&](const v4i (&af)[kRT][4], v4i (&nxt)[kRT][4], int rb, int rbn, int next_slot, int t0, const unsigned char *bq) {
    int vrb = rb;  // the class index of this step, put into a vector register once
    asm volatile("" : "+v"(vrb));
    v4i H[3][4];
    auto reduce_piece = [&](v4i (&P0)[4], v4i (&P1)[4], int t, int i, int &x, int &y, int &m0, int &m1) {
      const int c = (i >> 2) & 1;
      int &m = c ? m1 : m0;
      v4i(&P)[4] = c ? P1 : P0;
      switch (i) {
        case 0:
        case 4:
          x = max(max(P[0][0], P[0][1]), P[0][2]);
          y = max(max(P[2][0], P[2][1]), P[2][2]);
          break;
        case 1:
        case 5:
          x = max(max(x, P[0][3]), P[1][0]);
          y = max(max(y, P[2][3]), P[3][0]);
          break;
        case 2:
        case 6:
          x = max(max(x, P[1][1]), P[1][2]);
          y = max(max(y, P[3][1]), P[3][2]);
          break;
        case 3:
        case 7:
          m = max(max(x, y), P[1][3]);
          m = max(m, P[3][3]);
          break;
        case 8: {
          const auto r = __builtin_amdgcn_permlane16_swap((unsigned)m0, (unsigned)m1, false, false);
          m0 = (int)r[0];
          m1 = (int)r[1];
        } break;
        case 9:
          m0 = max(m0, m1);
          break;
        case 10:
          asm("v_med3_i32 %0, %1, %2, %3" : "=v"(cs[t]) : "v"(cb[t]), "v"(m0), "v"(cs[t]));  // cs <= cb: the second-largest of {cb, m, cs}
          break;
        case 11:
          asm volatile("v_cmp_gt_i32 vcc, %1, %2\n\ts_nop 1\n\tv_cndmask_b32 %0, %0, %3, vcc" : "+v"(ci[t]) : "v"(m0), "v"(cb[t]), "v"(vrb) : "vcc");
          break;
        case 12:
          cb[t] = max(cb[t], m0);
          break;
        default:
          break;
      }
    };
    asm volatile("; osfm-step16: a step of the 16x16x64 sweep begins (tests/test_kernel_budgets_shape16.py)");
#pragma unroll
    for (int t = 0; t < kCT4; ++t) {
      if (t == 0 && t0 > 0) {  // a partial step has no first tile to hide the fetch of the next step's targets in
        load_targets(rbn, nxt, next_slot);
        continue;
      }
      if (t < kCT4 - 1 && t < t0) continue;  // (t0 <= 7: the last stage always runs)
      // tile 7 prefetches the first tile of the next step
      const unsigned char *nb = (t == kCT4 - 1 ? bq + t0 * OSFM_TILE_BYTES : bq + (t + 1) * OSFM_TILE_BYTES);
      v4i(&C0)[4] = H[(2 * t) % 3];
      v4i(&C1)[4] = H[(2 * t + 1) % 3];  // = column sub-tile 0 of tile t-1: reduced in gaps 0-3, written from MFMA 8 on
      v4i(&P1)[4] = H[(2 * t + 2) % 3];  // = column sub-tile 1 of tile t-1
      int x = 0, y = 0, m0 = 0, m1 = 0;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int c = i >> 3, h = (i >> 2) & 1, s = i & 3;
        const v4i seed = {hn[0][4 * s], hn[0][4 * s + 1], hn[0][4 * s + 2], hn[0][4 * s + 3]};
        v4i &acc = c ? C1[s] : C0[s];
        acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[s >> 1][(s & 1) * 2 + h], bf[c * 2 + h], h == 0 ? seed : acc, 0, 0, 0);
        OSFM_PIN
        if (t > 0) {
          reduce_piece(C1, P1, t - 1, i, x, y, m0, m1);
        } else {  // the next step's targets, in the gaps that have no previous tile to reduce
          if (i == 0) load_seeds(rbn, next_slot);
          if (i == 4) load_rows(rbn, nxt, 0);
          if (i == 8) load_rows(rbn, nxt, 1);
        }
        if (t == kCT4 - 1 && i == 11) {
          // the step's last seeded MFMA is out: fetch the next step's seeds.  Their DMA is older than the 8 A-operand loads this step
          // issued (and the 8 DMAs of the next chunk, issued ahead of the chunk's first step, are older still)
          __builtin_amdgcn_s_waitcnt(0x0F70 | (2 * kRT * 4));  // vmcnt(8)
          read_seeds_rt(next_slot, 0);
        }
        if (t == kCT4 - 1 && i == 13) read_seeds_rt(next_slot, 1);
        if ((i & 3) == 3) bf[i >> 2] = *(const v4i *)(nb + osfm16_frag_offset(i >> 3, (i >> 2) & 1, lane));
        OSFM_PIN
      }
    }
    {  // drain: the last tile's accumulators
      v4i(&Q0)[4] = H[(2 * (kCT4 - 1)) % 3];
      v4i(&Q1)[4] = H[(2 * (kCT4 - 1) + 1) % 3];
      int x = 0, y = 0, m0 = 0, m1 = 0;
#pragma unroll
      for (int i = 0; i < 13; ++i) reduce_piece(Q0, Q1, kCT4 - 1, i, x, y, m0, m1);
    }
  };

  // the norm of the query a thread decides at the end of chunk c: requested one chunk ahead, so that no chunk waits for it alone
  auto load_norm = [&](int c) {
    const int slot = c * kChunkCols4 + tid;
    const int f = slot < nslots ? (GATHER ? (int)qsel[slot] : slot) : -1;
    return (f >= 0 && f < nQ) ? normQ[f] : OSFM_PAD_NORM;
  };
  dma_chunk(0);
  // two register sets for the A operands: the step that computes on one set fetches the next step's targets into the other
  v4i afA[kRT][4], afB[kRT][4];
  load_targets(0, afA, 0);
  int myna_next = load_norm(0);
  hooks.cold_issue();
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): chunk 0, the first targets and their seeds
  hooks.cold_done();
  read_seeds(0);
  int sidx = 0;  // global step counter: the seeds of step s are staged in slot s & 1

  for (int c = 0; c < nchunks; ++c) {
    // the query this thread decides at the end of the chunk (slot c*256 + tid); its norm was requested a chunk ahead
    const int myslot = c * kChunkCols4 + tid;
    const int myf = myslot < nslots ? (GATHER ? (int)qsel[myslot] : myslot) : -1;
    const int myna = myna_next;  // fetched during the previous chunk's merge (chunk 0: with the prologue's loads)
    // chunk c was requested at the top of the sweep of chunk c - 1 (chunk 0: above); everything this thread has in flight is older
    // than what the coming step will issue
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    __syncthreads();
    bb = sh.bbuf + (c & 1) * kChunkBytes4;
    const int t0 = kCT4 - min(kCT4, tS - c * kCT4);  // the chunk has 8 - t0 query tiles: its steps enter the tile sequence at stage t0
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)  // SHAPE 16: fragment ks = (column sub-tile ks >> 1, K half ks & 1)
      bf[ks] = *(const v4i *)(bb + (SHAPE == 16 ? osfm16_frag_offset(ks >> 1, ks & 1, lane) : ks * 1024 + lane * 16));
#pragma unroll
    for (int t = 0; t < kCT4; ++t) {
      cb[t] = INT_MIN;
      cs[t] = INT_MIN;
      ci[t] = 0;
    }

    // steps come in pairs: the first computes on set A and fetches into set B, the second the other way round; an odd last step
    // computes on A and then moves B (the next chunk's first targets) to A, so that every chunk starts on set A
    auto one_step = [&](const v4i (&cur)[kRT][4], v4i (&nxt)[kRT][4], int rb) {
      const int rbn = (rb + 1 < nrb) ? rb + 1 : 0;  // the next chunk starts over at row block 0 (the very last prefetch is unused)
      const bool live = rb * (kWaves * kRT) + w * kRT < tT;
      const int nslot = (sidx + 1) & 1;
      if (live) {  // (a live step fetches the next step's targets itself: a full one in the gaps of its first tile)
        if constexpr (SHAPE == 16)
          step16(cur, nxt, rb, rbn, nslot, t0, bb - t0 * OSFM_TILE_BYTES);
        else
          step(cur, nxt, rb, rbn, nslot, t0, bb - t0 * OSFM_TILE_BYTES);
      } else {  // a wave without targets in this row block still has to fetch the next step's, and pick up their seeds
        load_targets(rbn, nxt, nslot);
        __builtin_amdgcn_s_waitcnt(0x0F70);
        read_seeds(nslot);
      }
      ++sidx;
    };
    OSFM_TICK(tk0)
    hooks.chunk(c);
    if (c + 1 < nchunks) dma_chunk(c + 1);  // its buffer was released by the merge of chunk c - 1; older than every load of the sweep
    int rb = 0;
    for (; rb + 1 < nrb; rb += 2) {
      one_step(afA, afB, rb);
      one_step(afB, afA, rb + 1);
    }
    if (rb < nrb) {
      one_step(afA, afB, rb);
#pragma unroll
      for (int rt = 0; rt < kRT; ++rt)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) afA[rt][ks] = afB[rt][ks];
    }

    // ---- end of the chunk: merge the 8 partial classes (4 waves x 2 halves) of every query, decide, re-examine ----
    OSFM_TICK(tk1)
    if (c + 1 < nchunks) myna_next = load_norm(c + 1);  // in flight during the merge; the next chunk's vmcnt(0) covers it
    __syncthreads();  // everyone is done reading the chunk: its buffer becomes the scratch
    OSFM_TICK(tk2)
    int *scr = (int *)(sh.bbuf + (c & 1) * kChunkBytes4);  // [8 parts][3][256]
    {
      const int part = w * 2 + (lane >> 5);
#pragma unroll
      for (int t = 0; t < kCT4; ++t) {
        const int qt = (t - t0) & (kCT4 - 1);  // stage t held query tile t - t0 (the stages before t0 did not run: tiles that do not exist)
        scr[(part * 3 + 0) * kChunkCols4 + qt * 32 + (lane & 31)] = cb[t];
        scr[(part * 3 + 1) * kChunkCols4 + qt * 32 + (lane & 31)] = cs[t];
        scr[(part * 3 + 2) * kChunkCols4 + qt * 32 + (lane & 31)] = ci[t];
      }
    }
    __syncthreads();
    int b = INT_MIN, s2 = INT_MIN, id = 0;
#pragma unroll
    for (int part = 0; part < 2 * kWaves; ++part) {
      const int pb = scr[(part * 3 + 0) * kChunkCols4 + tid], ps = scr[(part * 3 + 1) * kChunkCols4 + tid];
      const int pi = scr[(part * 3 + 2) * kChunkCols4 + tid];
      s2 = max(max(s2, ps), min(b, pb));
      id = pb > b ? (pi * 8 + part) : id;
      b = max(b, pb);
    }
    __syncthreads();  // scratch read: the buffer may be refilled by the next chunk's prefetch (issued at the top of the loop)
    bool want = false;
    if (myf >= 0 && myf < nQ) {
      // v_best in {2b, 2b+1}; the best of the other classes in {2 s2, 2 s2 + 1}, the true second is at least that
      const int d1lo = max(myna - (2 * b + 1), 0), d2hi = myna - 2 * s2;
      if (FQ) {
        want = !fq_surely_fails(d1lo, d2hi, eps, fq_ratio(ratio));
      } else {
        if (d2hi >= kCollisionD2 && ratio >= 0.0) flag = 1;  // squared mode never takes a square root
        want = ratio_ok(d1lo, d2hi, ratio);
      }
#ifdef OSFM_DBG_NORECHECK
      want = false;
#endif
      if (!want) out[myf] = kNone;
    }
    // ---- re-examination, four queries at a time: one query per 16-lane row, two of the winner class's 32 targets per lane.  The
    //      candidates travel as packed keys v * 32 + (31 - ordinal) (ordinal = position in ascending target order), so one max
    //      gives the winner with cv2's lowest-index rule and a second max the runner-up; both are DPP reductions inside the row.
    unsigned long long pending = __ballot(want);
    unsigned long long redo = 0;  // queries that have to be re-done against all targets
    OSFM_TICK(tk3)
#ifdef OSFM_DBG_PHASES
    if (tid == 0) atomicAdd(&g_phase[(GATHER ? 5 : 0) + 4], (unsigned long long)__popcll(pending));
#endif
    while (pending) {
      int srcs[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        srcs[g] = pending ? (int)__builtin_ctzll(pending) : -1;
        pending &= pending - 1;  // 0 stays 0
      }
      const int g = lane >> 4, sl = lane & 15;
      const int src = g == 0 ? srcs[0] : g == 1 ? srcs[1] : g == 2 ? srcs[2] : srcs[3];
      const int ssrc = src < 0 ? 0 : src;
      const int qf = __shfl(myf, ssrc), qna = __shfl(myna, ssrc), qb = __shfl(b, ssrc), qs = __shfl(s2, ssrc), qid = __shfl(id, ssrc);
      const bool tie = (qs == qb);  // two classes tie on u: the winner may sit in either
      const int qrb = qid >> 3, qw = (qid >> 1) & 3, qh = qid & 1;
      // lane sl takes the class's targets of ordinal sl and 16 + sl (SHAPE 16: qid is the class id of match16_maps.h)
      const int row0 = SHAPE == 16 ? osfm16_class_target(qid, sl) : (qrb * (kWaves * kRT) + qw * kRT) * 32 + (sl & 3) + 8 * (sl >> 2) + 4 * qh;
      const int row1 = row0 + 32;
      int k0 = INT_MIN, k1 = INT_MIN;
      if (src >= 0 && !tie) {
        // a row beyond the image reads row 0 instead (its key is dropped below): the ADDRESS is selected, never the loaded value, so
        // that all 26 loads are in flight before the first wait (a value select made the compiler wait after every query slice:
        // ten memory round trips per step, profiles/r03_match_phases.txt)
        const bool ok0 = row0 < nT, ok1 = row1 < nT;
        const int r0 = ok0 ? row0 : 0, r1 = ok1 ? row1 : 0;
        const int8_t *pa = tilesQ + (long)(qf >> 5) * OSFM_TILE_BYTES + (qf & 31) * 16;
        const int8_t *p0 = tilesT + (long)(r0 >> 5) * OSFM_TILE_BYTES + (r0 & 31) * 16;
        const int8_t *p1 = tilesT + (long)(r1 >> 5) * OSFM_TILE_BYTES + (r1 & 31) * 16;
        v4i av[8], bv0[8], bv1[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          av[q] = *(const v4i *)(pa + q * 512);
          bv0[q] = *(const v4i *)(p0 + q * 512);
          bv1[q] = *(const v4i *)(p1 + q * 512);
        }
        const int n0 = normT[r0], n1 = normT[r1];
        int s0 = 0, s1 = 0;
#pragma unroll
        for (int q = 0; q < 8; ++q)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            s0 = __builtin_amdgcn_sdot4(av[q][e], bv0[q][e], s0, false);
            s1 = __builtin_amdgcn_sdot4(av[q][e], bv1[q][e], s1, false);
          }
        if (ok0) k0 = (2 * s0 - n0) * 32 + (31 - sl);
        if (ok1) k1 = (2 * s1 - n1) * 32 + (15 - sl);
      }
      const int kmax = row16_max(max(k0, k1));
      const int ksec = row16_max(k0 == kmax ? k1 : (k1 == kmax ? k0 : max(k0, k1)));
      if (src >= 0) {
        bool full = tie;
        int win = kNone;
        if (!tie) {
          const int m1 = kmax >> 5, ord = 31 - (kmax & 31);
          const int jwin = SHAPE == 16 ? osfm16_class_target(qid, ord) : (qrb * (kWaves * kRT) + qw * kRT + (ord >> 4)) * 32 + (ord & 3) + 8 * ((ord & 15) >> 2) + 4 * qh;
          const int m2 = ksec >> 5;  // INT_MIN >> 5 when the class has a single target: far below any bound
          const int sa = max(m2, 2 * qs), sb = max(m2, 2 * qs + 1);
          if (FQ) {
            // m1 is the exact quantised best; the quantised second lies in [sa, sb]
            const double r = fq_ratio(ratio);
            if (fq_surely_passes(qna - m1, qna - sb, eps, r))
              win = jwin;
            else if (!fq_surely_fails(qna - m1, qna - sa, eps, r))
              full = true;  // the bounds do not decide: float evaluation
          } else {
            const bool ra = ratio_ok(qna - m1, qna - sa, ratio), rbb = ratio_ok(qna - m1, qna - sb, ratio);
            if (ra == rbb)
              win = ra ? jwin : kNone;
            else
              full = true;  // the decision hangs on the parity bit of a norm in another class
          }
        }
        if (sl == 0 && !full) out[qf] = (unsigned short)win;
        hit |= (!full && win != kNone);
        redo |= (full && sl == 0) ? (1ull << src) : 0ull;
      }
    }
    OSFM_TICK(tk4)
    OSFM_PHASE((GATHER ? 5 : 0) + 0, tk0, tk1)  // sweep
    OSFM_PHASE((GATHER ? 5 : 0) + 1, tk1, tk2)  // wait for the other waves
    OSFM_PHASE((GATHER ? 5 : 0) + 2, tk2, tk3)  // merge + decide
    OSFM_PHASE((GATHER ? 5 : 0) + 3, tk3, tk4)  // class re-examination
    // the rare queries whose decision needs every target: exact best (lowest index among equals) and exact second, by the whole wave
    {
      unsigned lo = (unsigned)redo, hi = (unsigned)(redo >> 32);
#pragma unroll
      for (int m = 32; m >= 16; m >>= 1) {  // lanes 0, 16, 32, 48 hold the bits of their rows
        lo |= (unsigned)__shfl_xor((int)lo, m);
        hi |= (unsigned)__shfl_xor((int)hi, m);
      }
      redo = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)hi) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)lo);
    }
    if (FQ) flag += __popcll(redo);  // diagnostic: queries that needed the float evaluation (per wave, summed by the caller)
    while (FQ && redo) {
      // float evaluation of one query by the whole wave: every target whose quantised distance does not exclude it from the float
      // top two (D^ <= upper bound of the quantised second + 2 eps) is evaluated exactly as the oracle does; cv2's K = 2 insertion
      // (lowest index first among equals) per lane in ascending index order, then across the lanes
      const int src = __builtin_ctzll(redo);
      redo &= redo - 1;
      const int qf = __shfl(myf, src), qna = __shfl(myna, src), qs2 = __shfl(s2, src);
      const double T = (sqrt((double)max(qna - 2 * qs2, 0)) + 2.0 * eps) * (1.0 + 4.0 * kFqSlack) + 1e-6;
      const double T2 = T * T;
      const int vthr = T2 >= 2.0e9 ? INT_MIN : qna - (int)T2 - 1;
      const float *qrow = descQ + (long)qf * OSFM_DESC_DIM;
      float bd0 = INFINITY, bd1 = INFINITY;
      int bi0 = INT_MAX;
      for (int i = lane; i < nT; i += 64) {
        const int v = 2 * dot_rows8(tilesQ, qf, tilesT, i) - normT[i];
        if (v >= vthr) {
          const float sq = l2sqr_rows_f32(qrow, descT + (long)i * OSFM_DESC_DIM);
          const float d = ratio < 0.0 ? sq : sqrtf(sq);
          if (d < bd1) {
            if (bd0 > d) {
              bd1 = bd0;
              bd0 = d;
              bi0 = i;
            } else {
              bd1 = d;
            }
          }
        }
      }
      const float m = wave_minf(bd0);
      const int jwin = -wave_max(bd0 == m ? -bi0 : INT_MIN);
      const float sec = wave_minf(bi0 == jwin ? bd1 : bd0);
      const bool ok = ratio < 0.0 ? (m < (float)(-ratio) * sec) : ((double)m < ratio * (double)sec);
      if (lane == 0) out[qf] = (unsigned short)(ok ? jwin : kNone);
      hit |= ok;
    }
    while (!FQ && redo) {
      const int src = __builtin_ctzll(redo);
      redo &= redo - 1;
      const int qf = __shfl(myf, src), qna = __shfl(myna, src);
      int lv = INT_MIN, lj = INT_MAX, ls = INT_MIN;
      for (int i = lane; i < nT; i += 64) {
        const int v = 2 * dot_rows8(tilesQ, qf, tilesT, i) - normT[i];
        ls = max(ls, min(lv, v));
        if (v > lv) {  // ascending i within a lane: the first maximum is the lowest index
          lv = v;
          lj = i;
        }
      }
      const int m1 = wave_max(lv);
      const int jwin = -wave_max(lv == m1 ? -lj : INT_MIN);
      const int m2 = wave_max(lj == jwin ? ls : lv);
      const bool ok = ratio_ok(qna - m1, qna - m2, ratio);
      if (lane == 0) out[qf] = (unsigned short)(ok ? jwin : kNone);
      hit |= ok;
    }
  }  // chunks
  if (hit) *hit_word = 1;  // (every writer stores the same value)
  __syncthreads();
  any_hit = *hit_word;
  return flag;
}

// The grid is resident: min(n_pairs, 2 x CUs) workgroups, each of which draws pairs by ticket until the list is used up.  Blocks are
// dealt round-robin to the 8 XCDs, and the blocks with the same (blockIdx & 7) share one ticket counter and one contiguous eighth of
// the pair list, so that the pairs in flight on one L2 share their first image (what xcd_remap gave the one-workgroup-per-pair
// grid); where a block really runs decides locality only.  A block whose own eighth is used up goes on with the eighths behind it
// (the XCDs do not finish together; without that the slots of the fast ones idle through the tail of the launch).  The NEXT pair is
// drawn, and its header (image indices, counts, tile offsets) loaded, under pass A of the current pair; it reaches the waves through
// hdr[] in LDS:
//   hdr[0] pair index or -1 (the list is used up), hdr[1..6] img1, img2, n1, n2, tile offsets of img1 and img2 (tiles: < 2^31,
//   osfm_launch_match checks), hdr[7] whether hdr[3..6] are there (or on their way), hdr[8] how many eighths this block has seen empty.
struct PairRange {
  long first;
  int len;
};
__device__ __forceinline__ PairRange pair_range(long n_pairs, int x) {  // the ranges of xcd_remap
  const long q = n_pairs >> 3, r = n_pairs & 7;
  return PairRange{x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q, (int)(q + (x < r ? 1 : 0))};
}
// one thread: the next pair of the block, from the eighth it is in or the next one that has pairs left.  have: ticket t is already
// drawn from the eighth the block is in.
__device__ __forceinline__ int draw_pair(const MatchArgs &a, int xcd, int *hdr, bool have, int t) {
  for (int k = hdr[8]; k < 8; ++k) {
    const int x = (xcd + k) & 7;
    const PairRange r = pair_range(a.n_pairs, x);
    if (!have) t = atomicAdd(a.tickets + x * kTicketStride, 1);
    have = false;
    if (t < r.len) {
      hdr[8] = k;
      return (int)(r.first + t);
    }
  }
  hdr[8] = 8;
  return -1;
}
// the last of the three dependent round trips of a header: counts and tile offsets of the two images
__device__ __forceinline__ void finish_pair_header(const MatchArgs &a, int *hdr) {
  const int img1 = hdr[1], img2 = hdr[2];
  const int n1 = a.counts[img1], n2 = a.counts[img2];
  const int o1 = (int)a.tile_off[img1], o2 = (int)a.tile_off[img2];
  hdr[3] = n1;
  hdr[4] = n2;
  hdr[5] = o1;
  hdr[6] = o2;
  hdr[7] = 1;
}
// All of the header at once, by one thread that waits for each of the three round trips: for a workgroup's first pair and behind a
// pair that is over before it began (an image with fewer than two features).
__device__ __forceinline__ void fetch_pair_header(const MatchArgs &a, int xcd, int *hdr) {
  const int p = draw_pair(a, xcd, hdr, false, 0);
  hdr[0] = p;
  hdr[7] = 1;
  if (p >= 0) {
    const int img1 = a.pairs[2 * (long)p], img2 = a.pairs[2 * (long)p + 1];
    hdr[1] = img1;
    hdr[2] = img2;
    finish_pair_header(a, hdr);
  }
}
// The same under pass A of the current pair, one round trip at a time and none of them waited for: the ticket's atomic goes out with
// the pass's cold loads and comes back with them; the image indices (behind the barrier that opens chunk 0) and the counts and tile
// offsets (chunk 1; a pass of one chunk leaves them to the top of the next pair, finish_pair_header) travel global -> LDS by DMA, so
// that no vector register holds them through a sweep.  Wave 0 issues them; its vmcnt(0) ahead of the next chunk's barrier, or of the
// pair's last barrier, lands them for everyone.
struct NextPairFetch {
  const MatchArgs &a;
  int xcd;
  int *hdr;
  int tid;
  int t;
  __device__ __forceinline__ void cold_issue() {
    if (tid == 0) {
      const int k = hdr[8];
      t = k < 8 ? atomicAdd(a.tickets + ((xcd + k) & 7) * kTicketStride, 1) : 0;
    }
  }
  __device__ __forceinline__ void cold_done() {
    if (tid == 0) {
      hdr[0] = draw_pair(a, xcd, hdr, hdr[8] < 8, t);  // (draws again only where the eighth has just run out)
      hdr[7] = 0;
    }
  }
  __device__ __forceinline__ void chunk(int c) {
    if (c > 1 || __builtin_amdgcn_readfirstlane(tid >> 6) != 0) return;
    const int pn = __builtin_amdgcn_readfirstlane(hdr[0]);
    if (pn < 0) return;
    if (c == 0) {
      if (tid < 2)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(a.pairs + 2 * (long)pn + tid),
                                         (__attribute__((address_space(3))) void *)(hdr + 1), 4, 0, 0);
    } else if (tid < 4) {
      const int img = hdr[1 + (tid & 1)];
      const int32_t *src = tid < 2 ? a.counts + img : (const int32_t *)(a.tile_off + img);  // (little endian: the low word)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                       (__attribute__((address_space(3))) void *)(hdr + 3), 4, 0, 0);
      if (tid == 0) hdr[7] = 1;
    }
  }
};
struct NoFetch {
  __device__ __forceinline__ void cold_issue() {}
  __device__ __forceinline__ void cold_done() {}
  __device__ __forceinline__ void chunk(int) {}
};

// The thread index as a value of its own for one phase of a pair, made from the wave's index (a scalar register) and the lane
// count: what a phase derives from it (lane, wave, masks, LDS addresses) is then made in that phase, not hoisted out of the loop over
// pairs and held, or spilled, through both sweeps -- and neither is the thread index itself.
__device__ __forceinline__ int fresh_tid(int wave) {
  int t = wave * 64 + (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  asm volatile("" : "+v"(t));
  return t;
}

}  // namespace
