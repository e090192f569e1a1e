// match16.hip -- the fused matcher kernel of the integer store on v_mfma_i32_16x16x64_i8.
//
// The same kernel as match_fused_kernel<false> (match.hip) -- resident grid, tickets, pass A, candidate list, pass B, emission, the
// collision flag -- with the sweep's step on the 16 x 16 x 64 shape (step16 in match_sweep.h, lane maps in match16_maps.h).  The
// matcher's sweep is a dense MFMA loop on random bytes, under which the chip lowers its clock; on this shape it holds a higher one
// (profiles/r08_mfma_shape_ubench.txt: about the same cycles per FLOP, 1.92 against 1.72 GHz).  Results are bit-identical.
// A translation unit of its own, so that the 32x32x32 kernel's code does not depend on this one's.
// (the phase ticks of OSFM_DBG_PHASES builds live in match.hip, with the counters they add to: tools/match_phases.py runs that kernel)
#undef OSFM_DBG_PHASES
#include "match_sweep.h"

namespace {

__global__ void __launch_bounds__(kThreads, 2) match_sweep16_kernel(MatchArgs a) {
  constexpr bool FQ = false;
  constexpr int SHAPE = 16;
#include "match_pair_loop.inc"
}

}  // namespace

int osfm_launch_match_sweep16(int device, const MatchArgs &a, unsigned grid, size_t lds_bytes, hipStream_t stream) {
  static OsfmPerDeviceOnce once;
  OSFM_TRY(once.run(device, []() -> int {
    OSFM_HIP(hipFuncSetAttribute((const void *)match_sweep16_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    return OSFM_OK;
  }));
  hipLaunchKernelGGL(match_sweep16_kernel, dim3(grid), dim3(kThreads), lds_bytes, stream, a);
  return OSFM_OK;
}
