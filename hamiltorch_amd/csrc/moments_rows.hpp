// The row segments of the running-statistics kernels (moments.hip, covariance.hip): a chunk x[S, C, D] is cut into segments of
// R = moments_segment_rows(S, C, D) rows, one per blockIdx.y; diagnostics.moments_segment_rows restates it in Python.
#pragma once
#include <cstdint>

namespace hta {

constexpr int MOM_THREADS = 256;
constexpr int MOM_SEGMENT_ROWS = 256;     // rows of S per segment when C D fills the machine
constexpr int MOM_MIN_SEGMENT_ROWS = 32;
constexpr int MOM_TARGET_BLOCKS = 512;    // shorter segments while the grid has fewer blocks than this

static inline int64_t moments_segment_rows(int64_t S, int64_t C, int64_t D) {
  const int64_t bx = (C * D + MOM_THREADS - 1) / MOM_THREADS;
  int64_t R = MOM_SEGMENT_ROWS;
  while (R > MOM_MIN_SEGMENT_ROWS && bx * ((S + R - 1) / R) < MOM_TARGET_BLOCKS) R /= 2;
  return R;
}

}  // namespace hta
