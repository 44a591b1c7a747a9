// deskew.hip — constant-velocity motion compensation of one organized R x C sweep
// (DESIGN.md §Scan deskewing).  Column c was sampled at sweep fraction s_c; its points
// move to the sensor frame at mid-sweep: p' = Exp((s_c - 0.5) xi) p, xi = [w; v] the
// body-frame twist per scan period (GTSAM Pose3 tangent order, pose.hpp expmap).
//
// A wave owns 64 consecutive columns: each lane builds its column's transform once (12
// doubles in registers, one fp64 sincos per column instead of one per point), then the
// block's waves interleave over its rows, so every row access of a wave is one contiguous
// 1 KB float4 load and store.  Points are widened to fp64, transformed in d_xform's
// expression order ((R0 x + R1 y) + R2 z) + t (no contraction: -ffp-contract=off) and
// rounded once to fp32.  Dropouts (x = y = z = 0) stay exactly 0, the pad is copied, and
// a column whose scaled twist is exactly 0 is copied bit for bit.
//
// k_deskew_cells is the same with one sweep fraction per cell (an organized cloud whose
// points carry their own times, organize.hip): one lane per cell, one transform per lane.
// Both kernels build the transform in deskew_transform, so equal fractions give equal bits.
#include <cfloat>

#include "fmx_internal.hpp"

namespace fmx {

struct DeskewTwist {
  double xi[6];
};

constexpr int kDeskewThreads = 256;   // 4 waves on one group of 64 columns, interleaved over the rows
constexpr int kDeskewRowsPerWave = 4;  // rows each wave transforms with its column transforms (C4: 256 blocks)

// The transform of one sweep fraction: T (3 x 4 row-major) = Exp(s xi), s = s_c - 0.5.
// Returns true when the scaled twist is exactly 0 (the point is then copied).  One
// expression order for every caller (k_deskew per column, k_deskew_cells per point), so
// equal fractions give equal bits.
__device__ __forceinline__ bool deskew_transform(double s, const DeskewTwist& tw, double T[12]) {
  double w[3], v[3];
  bool ident = true;
  for (int k = 0; k < 3; ++k) {
    w[k] = s * tw.xi[k];
    v[k] = s * tw.xi[3 + k];
    ident = ident && w[k] == 0.0 && v[k] == 0.0;
  }
  // pose.hpp expmap (gtsam Pose3::Expmap)
  const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  double A, B, a, b;
  if (th2 <= DBL_EPSILON) {
    A = 1.0;
    B = 0.5;
    a = 0.5;
    b = 1.0 / 6.0;
  } else {
    const double th = sqrt(th2);
    double sn, cs;
    sincos(th, &sn, &cs);  // one argument reduction for both
    A = sn / th;
    B = (1.0 - cs) / th2;
    a = B;
    b = (th - sn) / (th2 * th);
  }
  const double W[3][3] = {{0, -w[2], w[1]}, {w[2], 0, -w[0]}, {-w[1], w[0], 0}};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double w2 = W[i][0] * W[0][j] + W[i][1] * W[1][j] + W[i][2] * W[2][j];
      T[4 * i + j] = (i == j ? 1.0 : 0.0) + A * W[i][j] + B * w2;
    }
  const double wxv[3] = {w[1] * v[2] - w[2] * v[1], w[2] * v[0] - w[0] * v[2], w[0] * v[1] - w[1] * v[0]};
  const double wxwxv[3] = {w[1] * wxv[2] - w[2] * wxv[1], w[2] * wxv[0] - w[0] * wxv[2],
                           w[0] * wxv[1] - w[1] * wxv[0]};
  for (int i = 0; i < 3; ++i) T[4 * i + 3] = v[i] + a * wxv[i] + b * wxwxv[i];
  return ident;
}

// p' = T p in fp64, rounded once; a dropout (x = y = z = 0) stays exactly 0, the pad is copied
__device__ __forceinline__ float4 deskew_apply(float4 q, bool ident, const double T[12]) {
  if (!ident && !(q.x == 0.0f && q.y == 0.0f && q.z == 0.0f)) {
    const double x = q.x, y = q.y, z = q.z;
    q.x = (float)(((T[0] * x + T[1] * y) + T[2] * z) + T[3]);
    q.y = (float)(((T[4] * x + T[5] * y) + T[6] * z) + T[7]);
    q.z = (float)(((T[8] * x + T[9] * y) + T[10] * z) + T[11]);
  }
  return q;
}

__global__ __launch_bounds__(kDeskewThreads) void k_deskew(const float4* __restrict__ in, float4* __restrict__ out,
                                                          const float* __restrict__ frac, int R, int C,
                                                          DeskewTwist tw) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + lane;
  if (col >= C) return;
  // the wave's rows: r0, r0 + 4, ... (the block's 4 waves interleave), all loaded up
  // front: the loads are in flight together while the column's transform is built
  const int r0 = (int)blockIdx.y * (kDeskewThreads / 64) * kDeskewRowsPerWave + wave;
  float4 p[kDeskewRowsPerWave];
#pragma unroll
  for (int k = 0; k < kDeskewRowsPerWave; ++k) {
    const int r = r0 + k * (kDeskewThreads / 64);
    if (r < R) p[k] = in[(size_t)r * (size_t)C + (size_t)col];
  }
  double T[12];
  const bool ident = deskew_transform((frac ? (double)frac[col] : (double)col / (double)C) - 0.5, tw, T);

#pragma unroll
  for (int k = 0; k < kDeskewRowsPerWave; ++k) {
    const int r = r0 + k * (kDeskewThreads / 64);
    if (r >= R) break;
    out[(size_t)r * (size_t)C + (size_t)col] = deskew_apply(p[k], ident, T);
  }
}

// Per-point sweep fractions (an organized cloud, organize.hip): one lane per cell, its
// fraction from the per-cell plane, so every lane builds its own transform (one fp64
// sincos per point).  Same contract as k_deskew otherwise; an empty cell is a dropout.
__global__ __launch_bounds__(kDeskewThreads) void k_deskew_cells(const float4* __restrict__ in,
                                                                float4* __restrict__ out,
                                                                const float* __restrict__ frac, uint32_t n,
                                                                DeskewTwist tw) {
  const uint32_t i = blockIdx.x * (uint32_t)kDeskewThreads + threadIdx.x;
  if (i >= n) return;
  const float4 p = in[i];
  double T[12];
  const bool ident = deskew_transform((double)frac[i] - 0.5, tw, T);
  out[i] = deskew_apply(p, ident, T);
}

// d_in -> d_out (both R * C float4 on the device, not aliased) on stream st; frac: C
// device floats or null (s_c = c / C)
void run_deskew(fmx_ctx* c, const float4* d_in, float4* d_out, const float* d_frac, int R, int C,
                const double xi[6], hipStream_t st) {
  if (R <= 0 || C <= 0) return;
  DeskewTwist tw;
  for (int k = 0; k < 6; ++k) tw.xi[k] = xi[k];
  const int rows_per_block = (kDeskewThreads / 64) * kDeskewRowsPerWave;
  const dim3 grid((uint32_t)((C + 63) / 64), (uint32_t)((R + rows_per_block - 1) / rows_per_block));
  ProfScope ps(c->prof, PROF_DESKEW, 32.0 * (double)R * (double)C, st);
  hipLaunchKernelGGL(k_deskew, grid, dim3(kDeskewThreads), 0, st, d_in, d_out, d_frac, R, C, tw);
  FMX_HIP(hipGetLastError());
}

// the same with one fraction per cell (n = R * C device floats)
void run_deskew_cells(fmx_ctx* c, const float4* d_in, float4* d_out, const float* d_cell_frac, size_t n,
                      const double xi[6], hipStream_t st) {
  if (n == 0) return;
  DeskewTwist tw;
  for (int k = 0; k < 6; ++k) tw.xi[k] = xi[k];
  const uint32_t blocks = (uint32_t)((n + kDeskewThreads - 1) / kDeskewThreads);
  ProfScope ps(c->prof, PROF_DESKEW, 36.0 * (double)n, st);
  hipLaunchKernelGGL(k_deskew_cells, dim3(blocks), dim3(kDeskewThreads), 0, st, d_in, d_out, d_cell_frac,
                     (uint32_t)n, tw);
  FMX_HIP(hipGetLastError());
}

}  // namespace fmx
