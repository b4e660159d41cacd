// Integer plumbing of the kernels that work on the first *d_num_valid of M padded rows (the mask and keypoint tails, their losses
// and backward passes).  No float expression lives here.
#pragma once

// The rows a kernel works on: *d_num_valid clamped to [0, M] (M without the operand).  Wave-uniform: one scalar load.
__device__ __forceinline__ int lvc_valid_rows(const int* d_num_valid, int M) {
  if (!d_num_valid) return M;
  const int nv = *d_num_valid;
  return nv < 0 ? 0 : (nv < M ? nv : M);
}

// The ordered-slice cut of a weight-gradient sum over `rows` rows: slices of `slice_rows` rows (a multiple of `chunk`, the rows per
// LDS chunk), unless that would make more than `max_slices` -- then `max_slices` equal slices, rounded up to a multiple of `chunk`.
struct LvcSliceCut {
  long long rows;   // rows per slice
  int slices;       // their number, at least 1
};

static inline LvcSliceCut lvc_slice_cut(long long rows, long long slice_rows, int max_slices, int chunk) {
  long long per = slice_rows;
  if ((rows + per - 1) / per > max_slices) per = ((rows + max_slices - 1) / max_slices + chunk - 1) / chunk * chunk;
  const long long n = (rows + per - 1) / per;
  return LvcSliceCut{per, n < 1 ? 1 : (int)n};
}
