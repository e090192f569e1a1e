// match16_maps.h -- index maps of the matcher's sweep on v_mfma_i32_16x16x64_i8, as plain functions so that the host can test
// them (tests/test_match_shape16_maps.py).
//
// Store layout: a tile holds 32 rows (features) of 128 int8; piece q (16 dimensions) of row r sits at q * 512 + r * 16.
// The MFMA takes a 16 x 64 operand: lane l holds row (l & 15), dimensions 16 (l >> 4) .. +15 of a K half h (64 dimensions), and
// returns a 16 x 16 tile: lane l holds column (l & 15), rows 4 (l >> 4) .. +3 in its four registers.
// A wave's step covers 64 targets = two row tiles = four 16-row sub-tiles s; lane group g = l >> 4.
// The kernel itself calls osfm16_frag_offset (operand addresses) and osfm16_class_target (class id, ordinal -> row, in the
// re-examination).  Which target an accumulator register holds is fixed by the hardware's result layout and by the
// v_permlane16_swap merge, not by a function call: osfm16_target, osfm16_class_id, osfm16_class_of_target and osfm16_ordinal write that
// layout down, the host test checks them against osfm16_class_target, and the check of the kernel against them is the GPU parity
// test (tests/test_gpu_matching_shape16.py: a wrong map picks wrong rows).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define OSFM16_HD __host__ __device__ constexpr
#else
#define OSFM16_HD constexpr
#endif

// ---- lane -> (row, K block) of an operand fragment: sub-tile `sub` (0 or 1) of a 32-row tile, K half h ----
OSFM16_HD int osfm16_frag_row(int sub, int lane) { return 16 * sub + (lane & 15); }
OSFM16_HD int osfm16_frag_piece(int h, int lane) { return 4 * h + (lane >> 4); }
OSFM16_HD int osfm16_frag_offset(int sub, int h, int lane) { return osfm16_frag_piece(h, lane) * 512 + osfm16_frag_row(sub, lane) * 16; }

// ---- (step = row block rb, wave w, lane group g, register = sub-tile s of the step and r) -> target ----
// a row block is what the four waves cover in one step: 8 row tiles, wave w takes tiles 2 w and 2 w + 1 of it
OSFM16_HD int osfm16_target(int rb, int w, int g, int s, int r) { return (rb * 8 + w * 2) * 32 + 16 * s + 4 * g + r; }

// ---- classes: the 32 targets whose maxima end up in one register bit of a lane after the pairwise merge of the lane groups
// (v_permlane16_swap + max): lane groups {0, 1} (half 0) or {2, 3} (half 1) of one wave in one step.  id = rb * 8 + w * 2 + half.
OSFM16_HD int osfm16_class_id(int rb, int w, int g) { return rb * 8 + w * 2 + (g >> 1); }
OSFM16_HD int osfm16_class_of_target(int target) { return (target >> 6) * 2 + ((target >> 3) & 1); }
// ordinal = position of a target among its class's targets in ascending index order (the packed key of the re-examination carries
// 31 - ordinal, which gives cv2's lowest-index rule among equal distances)
OSFM16_HD int osfm16_class_target(int id, int ordinal) { return (id >> 1) * 64 + 16 * (ordinal >> 3) + 8 * (id & 1) + (ordinal & 7); }
OSFM16_HD int osfm16_ordinal(int target) { return ((target >> 4) & 3) * 8 + (target & 7); }
