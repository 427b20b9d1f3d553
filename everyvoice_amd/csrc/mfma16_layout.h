// Lane maps of v_mfma_f32_16x16x32_bf16 as the inference convolution kernels use it, in one place: the kernels call these, and
// tests/test_mfma16_layout.py restates each function in numpy under the same name (change both together).
//
//   operands: lane l holds A[row l & 15][k = 8 (l >> 4) + j] and B[k = 8 (l >> 4) + j][col l & 15], j = 0 .. 7: one 16-byte
//             channel vector of one LDS row per operand.  A 64-channel image is two 32-deep k-steps s = 0, 1; lane l reads channel
//             vector (l >> 4) + 4 s of row (l & 15) (+ 16 per tile).
//   result:   register i of lane l is D[row 4 (l >> 4) + i][col l & 15]: with weights as A, four consecutive channels of one row.
//
// LDS rows are 128 bytes (eight 16-byte slots), unpadded; slot p of row r holds channel vector p ^ swizzle(r).  ds_read_b128 is
// served in four groups of 16 lanes ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32); a group is conflict-free when its
// 16 addresses are 16 distinct 16-byte slots of the 256-byte bank row.  A group of the 16-row read is 8 rows of one channel vector
// and 8 rows of its neighbour.  The activation tile is read at ANY first row (the taps shift it by tap * dilation), and there
// row & 6 is conflict-free at every offset while the swizzle of the 32 x 32 kernels, (row >> 1) & 7, is 2-way wherever the first
// row is not a multiple of 4 (and row & 6 is 2-way under the 32-row read: the swizzle belongs to the shape).  The weight images
// are only read at rows that are multiples of 16, where (row >> 1) & 7 is conflict-free under both reads: they stay in that layout
// (wlayout 1, no host change).  tests/test_mfma16_layout.py derives all of this from the addresses.
#pragma once

namespace evmi {
namespace mfma16 {

#if defined(__HIPCC__)
#define EVMI_HD __host__ __device__ __forceinline__
#else
#define EVMI_HD inline
#endif

EVMI_HD constexpr int x_swizzle(int row) { return row & 6; }         // activation tile (written by issue_x, read by the B fragments)
EVMI_HD constexpr int w_swizzle(int row) { return (row >> 1) & 7; }  // weight image (relayout_conv, layout 1)
// channel vector (0 .. 7) of a 64-channel row that `lane` feeds to k-step s (0, 1)
EVMI_HD constexpr int frag_vec(int lane, int s) { return (lane >> 4) + 4 * s; }
// byte offset of channel vector `vec` of row `row` in an image with the given swizzle value
EVMI_HD constexpr int frag_offset(int row, int vec, int swz) { return row * 128 + ((vec ^ swz) << 4); }
// accumulator register i (0 .. 3) of `lane`: row of the 16-row tile, channel of the 16-channel tile
EVMI_HD constexpr int acc_row(int lane) { return lane & 15; }
EVMI_HD constexpr int acc_channel(int lane, int i) { return 4 * (lane >> 4) + i; }
// v_permlane16_swap(a, b) with a = a register of tile (mt, 2 np), b = the same register of tile (mt, 2 np + 1): the odd 16-lane
// rows of a change places with the even ones of b.  Afterwards (a, b) of a lane are channels 8 (g >> 1) .. + 3 and .. + 4 .. + 7,
// g = lane >> 4, of row (lane & 15) of tile 2 np + (g & 1): as packed bf16, 16 contiguous bytes per lane.  Its own inverse.
EVMI_HD constexpr int swapped_tile(int lane) { return (lane >> 4) & 1; }     // which of the two row tiles the lane ends up with
EVMI_HD constexpr int swapped_channel(int lane) { return 8 * (lane >> 5); }  // first of its 8 channels within the 16-channel tile

#undef EVMI_HD

}  // namespace mfma16
}  // namespace evmi
