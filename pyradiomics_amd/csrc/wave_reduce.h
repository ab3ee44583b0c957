// wave_reduce.h -- butterfly reductions over one wave of 64 lanes: every lane gets the result, the order of the operations is
// fixed (kernels_voxel.h, kernels_mcc.h, kernels_batch_features.h)
#pragma once
#include "prad_runtime.h"

namespace prad {

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

}  // namespace prad
