// Microbenchmark: the matcher's sweep on the two int8 MFMA shapes of gfx950, v_mfma_i32_32x32x32_i8 against
// v_mfma_i32_16x16x64_i8, at the same output tile per wave (64 targets x 256 queries per step) and on the bench scene's own
// descriptor bytes.  The question is which shape is faster by WALL time: in an MFMA-dense loop on random data the chip lowers
// its clock, and the clock it holds can depend on the shape, so cycles per FLOP do not decide.
//
// Both kernels share one skeleton, the one of query_pass (match.hip):
//   * resident grid of 2 x CUs workgroups of 256 threads, occupancy 2 (80 KiB of dynamic LDS per workgroup);
//   * a chunk of 256 queries (8 tiles of the store's layout) stays in LDS and is streamed with ds_read_b128;
//   * each wave holds 64 targets in registers and fetches the next step's 64 from global memory (L2) one step ahead;
//   * -ceil(|a|^2 / 2) of the targets seeds the accumulators (through LDS, as in the product);
//   * the accumulators of query tile t-1 are reduced in the issue gaps of tile t: a v_max3 tree over all of them, then
//     max / med3 / compare-select per query and class (cb / cs / ci, one register each per query tile, for both shapes:
//     the 16x16 form merges its four lane groups pairwise with v_permlane16_swap + max before the class update).
// The class maxima are written out at the end; the host folds them to the per-query maximum over all targets, which must be
// the same number from both kernels (a check of the 16x16 operand and result maps on real data).
//
// build:  hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/ubench_mfma_shape.hip -o tools/ubench_mfma_shape
//         (... -DUBENCH_STAMPS -o tools/ubench_mfma_shape_stamps: the diagnostic build that reads the in-kernel clock)
// data:   python tools/ubench_mfma_shape_data.py OUT.bin    (two images of synthetic.make_matching_scene(1000, 2000, seed=42))
// run:    tools/ubench_mfma_shape OUT.bin [rounds=4] [seconds=2.0] [steps=4096]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

constexpr int kTile = 4096;          // 32 rows x 128 bytes: piece q (16 dimensions) of row r at q * 512 + r * 16
constexpr int kCT = 8;               // query tiles per chunk
constexpr int kLdsBytes = 80 * 1024;  // half a CU's LDS: two workgroups per CU
constexpr int kPadSeed = -(1 << 22);

#define CK(x)                                                                                  \
  do {                                                                                         \
    hipError_t e_ = (x);                                                                       \
    if (e_ != hipSuccess) {                                                                    \
      fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));      \
      exit(2);                                                                                 \
    }                                                                                          \
  } while (0)
#define PIN __builtin_amdgcn_sched_barrier(0);

struct Args {
  const int8_t *tilesQ;  // tQ tiles
  const int8_t *tilesT;  // tT tiles, tT a multiple of 8 (the tail is the zero slack tile)
  const int *hnegT;      // tT * 32 seeds
  int tQ, tT, steps;
  int *out;                      // [3: cb, cs, ci][grid][4 waves][8 tiles][64 lanes]
  unsigned long long *stamps;    // [grid][4]: memtime, memrealtime at the start and at the end (diagnostic build only)
};

__device__ __forceinline__ int max3(int a, int b, int c) { return max(max(a, b), c); }

// SHAPE 32: v_mfma_i32_32x32x32_i8, 64 per step.  SHAPE 16: v_mfma_i32_16x16x64_i8, 128 per step.
template <int SHAPE>
__global__ void __launch_bounds__(256, 2) sweep_kernel(Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  unsigned char *bb = lds;                 // the chunk: 8 query tiles
  int *hbuf = (int *)(lds + kCT * kTile);  // [2 slots][4 waves][64] seeds
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int q = 0; q < kCT; ++q)
    *(v4i *)(bb + q * kTile + tid * 16) = *(const v4i *)(a.tilesQ + (long)((blockIdx.x * kCT + q) % a.tQ) * kTile + tid * 16);
  __syncthreads();

  const int nrb = a.tT / 8;
  // lane offset of an operand fragment inside a tile
  //   32x32x32: K slice ks (32 dimensions) of row (lane & 31), half (lane >> 5): ks * 1024 + lane * 16
  //   16x16x64: K half h of row 16 s + (lane & 15), piece 4 h + (lane >> 4): (4 h + (lane >> 4)) * 512 + (16 s + (lane & 15)) * 16
  const int off16 = (lane >> 4) * 512 + (lane & 15) * 16;
  auto load_targets = [&](int rb, v4i (&af)[8], int &seed) {
    const int t = rb * 8 + w * 2;
    const int8_t *tp = a.tilesT + (long)t * kTile;
    seed = a.hnegT[t * 32 + lane];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (SHAPE == 32)  // af[rt * 4 + ks]
        af[i] = *(const v4i *)(tp + (i >> 2) * kTile + (i & 3) * 1024 + lane * 16);
      else  // af[s * 2 + h], sub-tile s = 0..3 of the wave's 64 rows
        af[i] = *(const v4i *)(tp + (i >> 2) * kTile + (i & 1) * 2048 + ((i >> 1) & 1) * 256 + off16);
    }
  };
  // seeds of the lane's own rows.  32x32: register r of half h is row (r & 3) + 8 (r >> 2) + 4 h of a row tile, 32 registers;
  // 16x16: register r of lane group g is row 4 g + r of a 16-row sub-tile, 16 registers
  v16i hn[2];
  auto read_seeds = [&](int slot) {
    const int *hb = hbuf + slot * 256 + w * 64;
    if (SHAPE == 32) {
#pragma unroll
      for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const v4i hv = *(const v4i *)(hb + rt * 32 + 8 * g + 4 * (lane >> 5));
#pragma unroll
          for (int e = 0; e < 4; ++e) hn[rt][4 * g + e] = hv[e];
        }
    } else {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const v4i hv = *(const v4i *)(hb + 16 * s + 4 * (lane >> 4));
#pragma unroll
        for (int e = 0; e < 4; ++e) hn[0][4 * s + e] = hv[e];
      }
    }
  };

  int cb[kCT], cs[kCT], ci[kCT];
#pragma unroll
  for (int t = 0; t < kCT; ++t) {
    cb[t] = INT_MIN;
    cs[t] = INT_MIN;
    ci[t] = 0;
  }
  v4i bf[4];

  auto class_update_a = [&](int t, int m) { asm("v_med3_i32 %0, %1, %2, %3" : "=v"(cs[t]) : "v"(cb[t]), "v"(m), "v"(cs[t])); };
  auto class_update_b = [&](int t, int m, int vrb) {
    asm volatile("v_cmp_gt_i32 vcc, %1, %2\n\ts_nop 1\n\tv_cndmask_b32 %0, %0, %3, vcc" : "+v"(ci[t]) : "v"(m), "v"(cb[t]), "v"(vrb) : "vcc");
  };

  // ---------------------------------------------------------------------------------------------------------------------------
  // 32x32x32: the step of query_pass.  Per query tile two K chains (one per row tile) on two of three accumulator tuples.
  // ---------------------------------------------------------------------------------------------------------------------------
  auto step32 = [&](const v4i (&af)[8], v4i (&nxt)[8], int rb, int rbn, int nslot) {
    const int vrb = rb;
    v16i T[3];
    int mp = 0, seed_next = 0;
#pragma unroll
    for (int t = 0; t < kCT; ++t) {
      const unsigned char *nb = (t == kCT - 1 ? bb : bb + (t + 1) * kTile) + lane * 16;
      v16i &C1 = T[(2 * t) % 3];
      v16i &C2 = T[(2 * t + 1) % 3];
      v16i &P2 = T[(2 * t + 2) % 3];
      int a0 = 0, b0 = 0, a1 = 0, b1 = 0, m2 = 0;
      C1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[0], bf[0], hn[0], 0, 0, 0);
      PIN
      if (t > 0) {
        a0 = max3(C2[0], C2[1], C2[2]);
        b0 = max3(C2[8], C2[9], C2[10]);
        a0 = max3(a0, C2[3], C2[4]);
        b0 = max3(b0, C2[11], C2[12]);
        a0 = max3(a0, C2[5], C2[6]);
        b0 = max3(b0, C2[13], C2[14]);
        mp = max3(a0, b0, C2[7]);
        mp = max(mp, C2[15]);
      }
      PIN
      C2 = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[4], bf[0], hn[1], 0, 0, 0);
      PIN
      if (t == 0) load_targets(rbn, nxt, seed_next);
      if (t == kCT - 2) hbuf[nslot * 256 + w * 64 + lane] = seed_next;
      if (t == kCT - 1) read_seeds(nslot);
      bf[0] = *(const v4i *)(nb);
      if (t > 0) {
        a1 = max3(P2[0], P2[1], P2[2]);
        b1 = max3(P2[8], P2[9], P2[10]);
      }
      PIN
      C1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[1], bf[1], C1, 0, 0, 0);
      PIN
      if (t > 0) {
        a1 = max3(a1, P2[3], P2[4]);
        b1 = max3(b1, P2[11], P2[12]);
      }
      PIN
      C2 = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[5], bf[1], C2, 0, 0, 0);
      PIN
      bf[1] = *(const v4i *)(nb + 1024);
      if (t > 0) {
        a1 = max3(a1, P2[5], P2[6]);
        b1 = max3(b1, P2[13], P2[14]);
      }
      PIN
      C1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[2], bf[2], C1, 0, 0, 0);
      PIN
      if (t > 0) {
        m2 = max3(a1, b1, P2[7]);
        m2 = max(m2, P2[15]);
      }
      PIN
      C2 = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[6], bf[2], C2, 0, 0, 0);
      PIN
      bf[2] = *(const v4i *)(nb + 2048);
      if (t > 0) {
        m2 = max(m2, mp);
        class_update_a(t - 1, m2);
      }
      PIN
      C1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[3], bf[3], C1, 0, 0, 0);
      PIN
      if (t > 0) class_update_b(t - 1, m2, vrb);
      PIN
      C2 = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[7], bf[3], C2, 0, 0, 0);
      PIN
      bf[3] = *(const v4i *)(nb + 3072);
      if (t > 0) cb[t - 1] = max(cb[t - 1], m2);
      PIN
    }
    {  // drain
      v16i &Q1 = T[(2 * (kCT - 1)) % 3];
      v16i &Q2 = T[(2 * (kCT - 1) + 1) % 3];
      int m = INT_MIN;
#pragma unroll
      for (int r = 0; r < 16; r += 2) m = max3(m, Q1[r], Q1[r + 1]);
#pragma unroll
      for (int r = 0; r < 16; r += 2) m = max3(m, Q2[r], Q2[r + 1]);
      class_update_a(kCT - 1, m);
      class_update_b(kCT - 1, m, vrb);
      cb[kCT - 1] = max(cb[kCT - 1], m);
    }
  };

  // ---------------------------------------------------------------------------------------------------------------------------
  // 16x16x64: per query tile 16 MFMAs = 2 column sub-tiles c x 2 K halves h x 4 row sub-tiles s, in the order (c, h, s), so a
  // chain's second MFMA follows its first at a distance of four.  Two sets of eight 4-register accumulators: the set of tile
  // t-1 is reduced in the gaps of tile t, one or two vector instructions per gap:
  //   gaps 0-3 / 4-7: the v_max3 tree over the 16 accumulators of column sub-tile 0 / 1 (8 instructions each);
  //   gap 8: v_permlane16_swap of the two maxima, gap 9: one max -> lane rows 0, 2 hold column sub-tile 0 with the targets of
  //          lane groups {0, 1} and {2, 3} merged (32-target classes, as in the 32x32 form), rows 1, 3 column sub-tile 1;
  //   gaps 10-12: med3, compare + select, max.
  // The B fragment (c, h) is re-read for the next tile behind its fourth MFMA.
  // ---------------------------------------------------------------------------------------------------------------------------
  auto step16 = [&](const v4i (&af)[8], v4i (&nxt)[8], int rb, int rbn, int nslot) {
    const int vrb = rb;
    v4i A[2][2][4];
    int seed_next = 0;
    auto reduce_piece = [&](v4i (&P)[2][4], int t, int i, int &x, int &y, int &m0, int &m1) {
      const int c = i >> 2;
      int &m = c ? m1 : m0;
      switch (i) {
        case 0:
        case 4:
          x = max3(P[c][0][0], P[c][0][1], P[c][0][2]);
          y = max3(P[c][2][0], P[c][2][1], P[c][2][2]);
          break;
        case 1:
        case 5:
          x = max3(x, P[c][0][3], P[c][1][0]);
          y = max3(y, P[c][2][3], P[c][3][0]);
          break;
        case 2:
        case 6:
          x = max3(x, P[c][1][1], P[c][1][2]);
          y = max3(y, P[c][3][1], P[c][3][2]);
          break;
        case 3:
        case 7:
          m = max3(x, y, P[c][1][3]);
          m = max(m, P[c][3][3]);
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
          class_update_a(t, m0);
          break;
        case 11:
          class_update_b(t, m0, vrb);
          break;
        case 12:
          cb[t] = max(cb[t], m0);
          break;
        default:
          break;
      }
    };
#pragma unroll
    for (int t = 0; t < kCT; ++t) {
      const unsigned char *nb = (t == kCT - 1 ? bb : bb + (t + 1) * kTile) + off16;
      v4i(&C)[2][4] = A[t & 1];
      v4i(&P)[2][4] = A[(t & 1) ^ 1];
      int x = 0, y = 0, m0 = 0, m1 = 0;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int c = i >> 3, h = (i >> 2) & 1, s = i & 3;
        const v4i seed = {hn[0][4 * s], hn[0][4 * s + 1], hn[0][4 * s + 2], hn[0][4 * s + 3]};
        C[c][s] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[s * 2 + h], bf[c * 2 + h], h == 0 ? seed : C[c][s], 0, 0, 0);
        PIN
        if (t > 0) reduce_piece(P, t - 1, i, x, y, m0, m1);
        if (t == 0 && i == 1) load_targets(rbn, nxt, seed_next);
        if (t == kCT - 2 && i == 13) hbuf[nslot * 256 + w * 64 + lane] = seed_next;
        if (t == kCT - 1 && i == 11) read_seeds(nslot);  // the step's last seeded MFMA is out
        if ((i & 3) == 3) bf[i >> 2] = *(const v4i *)(nb + ((i >> 2) & 1) * 2048 + (i >> 3) * 256);
        PIN
      }
    }
    {  // drain
      v4i(&Q)[2][4] = A[(kCT - 1) & 1];
      int x = 0, y = 0, m0 = 0, m1 = 0;
#pragma unroll
      for (int i = 0; i < 13; ++i) reduce_piece(Q, kCT - 1, i, x, y, m0, m1);
    }
  };

  v4i afA[8], afB[8];
  int seed0;
  load_targets(0, afA, seed0);
  hbuf[w * 64 + lane] = seed0;
  read_seeds(0);
  if (SHAPE == 32) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) bf[ks] = *(const v4i *)(bb + ks * 1024 + lane * 16);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) bf[i] = *(const v4i *)(bb + (i & 1) * 2048 + (i >> 1) * 256 + off16);
  }
#ifdef UBENCH_STAMPS
  const unsigned long long st0 = __builtin_amdgcn_s_memtime(), sr0 = __builtin_amdgcn_s_memrealtime();
#endif
  int rb = 0;
  for (int s = 0; s < a.steps; s += 2) {
    const int rb1 = rb + 1 < nrb ? rb + 1 : 0, rb2 = rb1 + 1 < nrb ? rb1 + 1 : 0;
    if (SHAPE == 32) {
      step32(afA, afB, rb, rb1, 1);
      step32(afB, afA, rb1, rb2, 0);
    } else {
      step16(afA, afB, rb, rb1, 1);
      step16(afB, afA, rb1, rb2, 0);
    }
    rb = rb2;
  }
#ifdef UBENCH_STAMPS
  const unsigned long long st1 = __builtin_amdgcn_s_memtime(), sr1 = __builtin_amdgcn_s_memrealtime();
  if (tid == 0) {
    unsigned long long *sp = a.stamps + (long)blockIdx.x * 4;
    sp[0] = st0;
    sp[1] = sr0;
    sp[2] = st1;
    sp[3] = sr1;
  }
#endif
#pragma unroll
  for (int t = 0; t < kCT; ++t) {
    const long o = (((long)blockIdx.x * 4 + w) * kCT + t) * 64 + lane, plane = (long)gridDim.x * 4 * kCT * 64;
    a.out[o] = cb[t];
    a.out[plane + o] = cs[t];
    a.out[2 * plane + o] = ci[t];
  }
}

static double median(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}

int main(int argc, char **argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s DATA.bin [rounds=4] [seconds=2.0] [steps=4096]\n", argv[0]);
    return 2;
  }
  const int rounds = argc > 2 ? atoi(argv[2]) : 4;
  const double seconds = argc > 3 ? atof(argv[3]) : 2.0;
  const int steps = argc > 4 ? atoi(argv[4]) & ~1 : 4096;
  FILE *f = fopen(argv[1], "rb");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  int hdr[2];
  if (fread(hdr, 4, 2, f) != 2) return 2;
  const int nQ = hdr[0], nT = hdr[1];
  const int tQ = (nQ + 31) / 32, tT = ((nT + 31) / 32 + 1 + 7) / 8 * 8;  // at least one slack tile, a multiple of 8
  std::vector<int8_t> hQ((size_t)tQ * kTile, 0), hT((size_t)tT * kTile, 0);
  if (fread(hQ.data(), kTile, tQ, f) != (size_t)tQ) return 2;
  if (fread(hT.data(), kTile, (nT + 31) / 32, f) != (size_t)((nT + 31) / 32)) return 2;
  fclose(f);
  std::vector<int> hneg((size_t)tT * 32, kPadSeed);
  long nonzero = 0;
  for (int r = 0; r < nT; ++r) {
    int n = 0;
    for (int d = 0; d < 128; ++d) {
      const int v = hT[(size_t)(r >> 5) * kTile + (d >> 4) * 512 + (r & 31) * 16 + (d & 15)];
      n += v * v;
      nonzero += v != 0;
    }
    hneg[r] = -((n + 1) / 2);
  }
  if (nonzero < (long)nT * 64) {
    fprintf(stderr, "the data file holds mostly zeros: this benchmark is meaningless on such operands\n");
    return 2;
  }

  hipDeviceProp_t prop;
  CK(hipGetDeviceProperties(&prop, 0));
  const int grid = 2 * prop.multiProcessorCount;
  int8_t *dQ, *dT;
  int *dH, *dOut;
  unsigned long long *dStamps;
  CK(hipMalloc(&dQ, hQ.size()));
  CK(hipMalloc(&dT, hT.size()));
  CK(hipMalloc(&dH, hneg.size() * 4));
  const size_t out_n = (size_t)grid * 4 * kCT * 64;
  CK(hipMalloc(&dOut, out_n * 4 * 3));
  CK(hipMalloc(&dStamps, (size_t)grid * 4 * 8));
  CK(hipMemcpy(dQ, hQ.data(), hQ.size(), hipMemcpyHostToDevice));
  CK(hipMemcpy(dT, hT.data(), hT.size(), hipMemcpyHostToDevice));
  CK(hipMemcpy(dH, hneg.data(), hneg.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemset(dStamps, 0, (size_t)grid * 4 * 8));
  CK(hipFuncSetAttribute((const void *)sweep_kernel<32>, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes));
  CK(hipFuncSetAttribute((const void *)sweep_kernel<16>, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes));
  int occ32 = 0, occ16 = 0;
  CK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ32, sweep_kernel<32>, 256, kLdsBytes));
  CK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ16, sweep_kernel<16>, 256, kLdsBytes));
  printf("device %s, %d CUs, grid %d x 256, workgroups per CU: 32x32x32 %d, 16x16x64 %d\n", prop.name, prop.multiProcessorCount, grid,
         occ32, occ16);
  printf("operands: %d queries, %d targets of the bench scene; %d steps per launch\n", nQ, nT, steps);
  Args a{dQ, dT, dH, tQ, tT, steps, dOut, dStamps};
  auto launch = [&](int shape) {
    if (shape == 32)
      hipLaunchKernelGGL(sweep_kernel<32>, dim3(grid), dim3(256), kLdsBytes, 0, a);
    else
      hipLaunchKernelGGL(sweep_kernel<16>, dim3(grid), dim3(256), kLdsBytes, 0, a);
  };

  // the two kernels must agree on every query's maximum over all targets (steps >= tT / 8 so that every target was seen)
  {
    Args c = a;
    c.steps = std::max(2, tT / 8);
    std::vector<int> o32(out_n), o16(out_n);
    hipLaunchKernelGGL(sweep_kernel<32>, dim3(grid), dim3(256), kLdsBytes, 0, c);
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(o32.data(), dOut, out_n * 4, hipMemcpyDeviceToHost));
    hipLaunchKernelGGL(sweep_kernel<16>, dim3(grid), dim3(256), kLdsBytes, 0, c);
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(o16.data(), dOut, out_n * 4, hipMemcpyDeviceToHost));
    long bad = 0, checked = 0;
    for (int b = 0; b < grid; ++b)
      for (int q = 0; q < 256; ++q) {
        int m32 = INT_MIN, m16 = INT_MIN;
        const int t = q >> 5, j = q & 31;
        for (int w = 0; w < 4; ++w) {
          const size_t base = (((size_t)b * 4 + w) * kCT + t) * 64;
          for (int hh = 0; hh < 2; ++hh) {
            m32 = std::max(m32, o32[base + hh * 32 + j]);
            m16 = std::max(m16, o16[base + (2 * hh + (j >> 4)) * 16 + (j & 15)]);
          }
        }
        // host reference for the first workgroup's queries
        if (b == 0) {
          int ref = INT_MIN;
          const int qt = (b * kCT + t) % tQ;
          for (int r = 0; r < tT * 32; ++r) {
            int dot = 0;
            for (int d = 0; d < 128; ++d)
              dot += (int)hQ[(size_t)qt * kTile + (d >> 4) * 512 + j * 16 + (d & 15)] * (int)hT[(size_t)(r >> 5) * kTile + (d >> 4) * 512 + (r & 31) * 16 + (d & 15)];
            ref = std::max(ref, dot + hneg[r]);
          }
          bad += (ref != m32);
        }
        bad += (m32 != m16);
        ++checked;
      }
    printf("cross-check: %ld queries, %ld mismatches between the shapes and against the host\n", checked, bad);
    if (bad) return 1;
  }

  const double flop_per_launch = (double)grid * 4 * steps * (64.0 * 256 * 128 * 2);
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  for (int shape : {32, 16}) {  // warm-up
    for (int i = 0; i < 3; ++i) launch(shape);
    CK(hipDeviceSynchronize());
  }
  std::vector<double> ps[2], cyc[2], ghz[2];
  for (int r = 0; r < rounds; ++r)
    for (int k = 0; k < 2; ++k) {
      const int shape = k == 0 ? 32 : 16;
      // calibrate the launch count of a round on one launch, then time the whole round with one pair of events
      CK(hipEventRecord(e0));
      launch(shape);
      CK(hipEventRecord(e1));
      CK(hipEventSynchronize(e1));
      float ms1 = 0;
      CK(hipEventElapsedTime(&ms1, e0, e1));
      const int n = std::max(2, (int)(seconds * 1e3 / ms1) + 1);
      CK(hipEventRecord(e0));
      for (int i = 0; i < n; ++i) launch(shape);
      CK(hipEventRecord(e1));
      CK(hipEventSynchronize(e1));
      float ms = 0;
      CK(hipEventElapsedTime(&ms, e0, e1));
      const double p = ms * 1e-3 / (n * flop_per_launch) * 1e12 * 1e3;  // picoseconds per 1000 MFMA-FLOP
      ps[k].push_back(p);
      printf("round %d  %s  %4d launches  %8.2f ms  %.4f ps per kFLOP  %.1f TOP/s", r, shape == 32 ? "32x32x32" : "16x16x64", n, ms, p,
             n * flop_per_launch / (ms * 1e-3) * 1e-12);
#ifdef UBENCH_STAMPS
      std::vector<unsigned long long> st((size_t)grid * 4);
      CK(hipMemcpy(st.data(), dStamps, st.size() * 8, hipMemcpyDeviceToHost));
      std::vector<double> cs_, gs_;
      for (int b = 0; b < grid; ++b) {
        const double dc = (double)(st[b * 4 + 2] - st[b * 4 + 0]), dr = (double)(st[b * 4 + 3] - st[b * 4 + 1]);
        // one SIMD serves two waves: cycles of the SIMD per 64 Ki MFMA-FLOP = 32 Ki multiply-adds (one 32x32x32, or two 16x16x64)
        cs_.push_back(dc / ((double)steps * 64 * 2));
        gs_.push_back(dc / dr * 0.1);
      }
      cyc[k].push_back(median(cs_));
      ghz[k].push_back(median(gs_));
      printf("  %.2f SIMD cycles per 64 Ki FLOP  %.3f GHz", median(cs_), median(gs_));
#endif
      printf("\n");
      fflush(stdout);
    }
  for (int k = 0; k < 2; ++k) {
    const double lo = *std::min_element(ps[k].begin(), ps[k].end()), hi = *std::max_element(ps[k].begin(), ps[k].end());
    printf("%s  wall: median %.4f ps per kFLOP (min %.4f, max %.4f, spread %.2f %%)", k == 0 ? "32x32x32" : "16x16x64", median(ps[k]), lo, hi,
           (hi - lo) / median(ps[k]) * 100);
#ifdef UBENCH_STAMPS
    printf("  cycles per 64 Ki FLOP per SIMD: median %.2f = %.5f cycles per kFLOP per SIMD; clock: median %.3f GHz (min %.3f, max %.3f)",
           median(cyc[k]), median(cyc[k]) / 65.536, median(ghz[k]), *std::min_element(ghz[k].begin(), ghz[k].end()),
           *std::max_element(ghz[k].begin(), ghz[k].end()));
#endif
    printf("\n");
  }
  printf("ratio 16x16x64 / 32x32x32 by wall (median): %.4f  (below 1: the 16x16x64 loop is faster)\n", median(ps[1]) / median(ps[0]));
  return 0;
}
