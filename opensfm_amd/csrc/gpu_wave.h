// gpu_wave.h -- the GPU side of the wave policy that the walks of relpose_rounds.h and loransac_walk.h are written against (one
// wavefront = one workgroup; the host tests run the same walks with tests/native/loop_wave.h's loops in place of lanes), and a scoped
// device buffer.
#pragma once
#include <hip/hip_runtime.h>

#include "relpose_rounds.h"

namespace osfm_rp {

struct GpuWave {  // one wavefront = one workgroup
  int lane;
  template <class F>
  __device__ void single(F f) {
    __syncthreads();
    if (lane == 0) f();
    __syncthreads();
  }
  template <class F>
  __device__ void parallel_for(int n, F f) {
    __syncthreads();
    for (int i = lane; i < n; i += kWave) f(i);
    __syncthreads();
  }
  template <class P>
  __device__ int count_if(int n, P p) {
    int c = 0;
    for (int base = 0; base < n; base += kWave) {
      const int i = base + lane;
      const bool b = i < n && p(i);
      c += __popcll(__ballot(b));
    }
    return c;
  }
  template <class P>
  __device__ int compact(int n, P p, int *out) {  // ascending indices, as a sequential scan would write them
    int c = 0;
    for (int base = 0; base < n; base += kWave) {
      const int i = base + lane;
      const bool b = i < n && p(i);
      const unsigned long long m = __ballot(b);
      if (b) out[c + __popcll(m & ((1ull << lane) - 1ull))] = i;
      c += __popcll(m);
    }
    __syncthreads();
    return c;
  }
  template <class P>
  __device__ int compact_changed(int n, P p, int *out, int *changed) {  // compact + "did any entry change"
    int c = 0;
    bool diff = false;
    for (int base = 0; base < n; base += kWave) {
      const int i = base + lane;
      const bool b = i < n && p(i);
      const unsigned long long m = __ballot(b);
      if (b) {
        const int k = c + __popcll(m & ((1ull << lane) - 1ull));
        diff |= out[k] != i;
        out[k] = i;
      }
      c += __popcll(m);
    }
    if (__ballot(diff)) *changed = 1;
    __syncthreads();
    return c;
  }
  __device__ int atomic_add(int *p, int v) { return atomicAdd(p, v); }
  // a window of the generator stream next to the wavefront: the draws of lane 0 then cost an LDS read each, not a trip to L2
  __device__ RngView stage_rng(const RngTable &T, uint32_t *buf, int pos, bool want) {
    int n = 0;
    if (want) {
      n = T.size - pos < kRngCache ? T.size - pos : kRngCache;
      if (n < 0) n = 0;
      for (int i = lane; i < n; i += kWave) buf[i] = T.tab[pos + i];
    }
    __syncthreads();
    return RngView{T, buf, pos, n};
  }
};

}  // namespace osfm_rp
