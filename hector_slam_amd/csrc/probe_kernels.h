// probe_kernels.h -- the kernels that only the probes and test hooks launch (probes.hip).  They are not templates, so exactly one
// translation unit may include this header.
#pragma once
#include <hip/hip_runtime.h>

#include "gn_match.h"
#include "map_cells.h"

namespace hsm {

// test hook (hsm_debug_marks_nonzero): the dense update's byte map and the keyed update's end-cell bitmap must be ALL ZERO
// between updates (each apply pass clears what its mark passes set; map_update.h "dense scans"): count the non-zero words
__global__ void __launch_bounds__(256) count_nonzero_words_kernel(const unsigned int* __restrict__ words, size_t n,
                                                                  unsigned long long* __restrict__ out) {
  unsigned int local = 0;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    local += words[i] != 0u ? 1u : 0u;
  const unsigned long long m = __ballot(local != 0u);
  if (m == 0ull) return;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) local += (unsigned int)__shfl_down((int)local, d);
  if ((threadIdx.x & 63) == 0) atomicAdd(out, (unsigned long long)local);
}

// rectangle (x0,y0,w,h) of the two SoA planes -> the reference's AoS LogOddsCell {float, int}
__global__ void pack_cells_kernel(LevelRW L, int x0, int y0, int w, int h, int2* __restrict__ out) {
  const size_t n = (size_t)w * h;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int x = x0 + (int)(i % (size_t)w), y = y0 + (int)(i / (size_t)w);
    const size_t c = (size_t)y * L.sx + x;
    out[i] = make_int2(__float_as_int(L.logodds[c]), L.update_index[c]);
  }
}

// device expf / getGridProbability sweep for the parity tests
__global__ void expf_debug_kernel(const float* __restrict__ x, int n, float* __restrict__ e, float* __restrict__ p) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  e[i] = libm::expf_glibc(x[i]);
  p[i] = grid_probability(x[i]);
}

// device sin/cos sweep for the parity tests
__global__ void sincos_debug_kernel(const float* __restrict__ x, int n, float* __restrict__ s,
                                    float* __restrict__ c) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  sincos_f32(x[i], s[i], c[i]);
}

}  // namespace hsm
