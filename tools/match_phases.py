"""Where match_fused_kernel spends its time per pair, on the neighbour list and on a slice of the exhaustive list; and, for the
resident grid, what lies between two pairs of a workgroup and how long a workgroup lives (a build from before the resident grid
reports neither: there a workgroup was a pair, and what it spent outside its buckets -- launch, header loads, LDS clear -- is the
kernel time times the workgroup slots over the pairs, minus "whole pair").
The ticks are in match.hip only: the tool runs the integer store on match_fused_kernel<false> (OSFM_MATCH_SWEEP_32X32), not on the default
16x16x64 kernel of match16.hip, whose code around the step is the same.
Needs the instrumented build (tools/libosfm_dbg_phases.so: match.hip compiled with -DOSFM_DBG_PHASES, linked with the product's
other objects);  OSFM_MI355_LIB=tools/libosfm_dbg_phases.so python tools/match_phases.py"""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import neighbour_pairs  # noqa: E402
from opensfm_amd import _lib, matching, synthetic  # noqa: E402
from opensfm_amd._lib import MatchTimings, default_context  # noqa: E402

NAMES = ["A sweep", "A wait", "A merge+decide", "A class re-exam", "A queries re-examined",
         "B sweep", "B wait", "B merge+decide", "B class re-exam", "B queries re-examined",
         "pass A", "candidate list", "candidates + pass B", "emission", "whole pair", "pairs",
         "boundary (last write -> pass A)", "workgroup life", "resident workgroups"]


def phases(lib, reset=True):
    out = (C.c_ulonglong * 24)()  # (an older build fills 16)
    assert lib.osfm_dbg_phases(out, int(reset)) == 0
    return np.array(out[:], np.float64)


def _sweep32_params(config=None, robust=True, _make=matching.make_params):
    p = _make(config, robust)
    p.flags |= _lib.MATCH_SWEEP_32X32  # the instrumented kernel
    return p


def main():
    matching.make_params = _sweep32_params
    ctx = default_context(0)
    lib = _lib.load()
    scene = synthetic.make_matching_scene(1000, 2000, seed=0)
    store = matching.DescriptorStore.from_packed(scene.desc, scene.pts, scene.offsets, ctx)
    lists = {"neighbour (j - i <= 16)": neighbour_pairs(1000, 16), "exhaustive, first 60000": synthetic.all_pairs(1000)[:60000]}
    for name, pairs in lists.items():
        matching.match_pairs(store, pairs[:512], robust=False)
        phases(lib)
        tm = MatchTimings()
        matching.match_pairs(store, pairs, robust=False, timings=tm)
        ph = phases(lib)
        n = ph[15]
        print(f"== {name}: {len(pairs)} pairs, match kernel {tm.ms_match_kernel:.3f} ms in {int(tm.match_launches)} launches, {int(n)} pairs ticked")
        for i, nm in list(enumerate(NAMES[:15])) + [(16, NAMES[16])]:
            if i in (4, 9):
                print(f"  {nm:32s} {ph[i] / n:9.1f} per pair")
            else:
                print(f"  {nm:32s} {ph[i] / n / 100.0:9.2f} us per pair   ({100.0 * ph[i] / max(ph[14], 1):5.1f} %)")
        slots = 2 * ctx.num_cus
        print(f"  kernel time x {slots} slots / pairs  {tm.ms_match_kernel * 1e3 * slots / max(n, 1):9.2f} us per pair")
        if ph[18] > 0:
            print(f"  {NAMES[17]:32s} {ph[17] / ph[18] / 100.0:9.2f} us per workgroup, {int(ph[18])} workgroups, {n / ph[18]:.1f} pairs each;"
                  f" {(ph[17] - ph[14]) / n / 100.0:.2f} us per pair outside 'whole pair'")
        if ph[20] > 0:
            print(f"  pairs over before they began (an image of < 2 features): {int(ph[20])}, {ph[19] / ph[20] / 100.0:.2f} us each, in no other bucket")


if __name__ == "__main__":
    main()
