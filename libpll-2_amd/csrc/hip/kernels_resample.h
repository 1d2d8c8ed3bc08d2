// kernels_resample.h - sums of per-site values under resampled site weights:
//
//   C[v][b] = sum over n < sites of U[v][n] * (double)W[b][n]
//
// U: V rows of per-site log-likelihoods (binary64), W: B rows of site weights as a caller gives them (unsigned, converted
// here). This file knows nothing about where the rows of U come from: the quartet call is its first user
// (kernels_quartet.h leaves three rows per quartet), the insertion and placement calls can follow.
//
// The contraction runs on the fp64 matrix pipe: v_mfma_f64_16x16x4_f64, D(16 x 16) += A(16 x 4) B(4 x 16); lane l holds
// A[l & 15][l >> 4] and B[l >> 4][l & 15] - here row (l & 15) of the wave's 16 rows of U, and of W, at site k = l >> 4 of
// the step - and register t of the result is D[(l >> 4) + 4 t][l & 15]. The order of the four sites inside a step is
// free as long as both operands agree, so a lane reads FOUR CONSECUTIVE sites of its row at once (32 bytes of U, 16 of
// W: sixteen rows x 128 / 64 contiguous bytes per load instruction) and step t of a 16-site block contracts the sites
// {n0 + 4 q + t : q = 0..3}. A wave owns 32 x 32 results (2 x 2 tiles, 16 independent accumulator registers), the four
// waves of a workgroup four neighbouring column blocks over the same rows of U; nothing goes through LDS.
//
// The sites are split over the grid's z axis: resample_splits(sites) ranges of resample_split_len(sites) sites, both a
// function of the site count alone. Split s leaves its partial at part[s][v][b] with an ordinary store, and
// k_resample_reduce - the next launch on the stream - adds the partials of an element in split order. So the bits of
// C[v][b] follow from the site count, row v of U and row b of W and nothing else: not from V, B, the position of either
// row in its array, what the other rows hold (an MFMA result element is the sum of its own products only), or the run.
// No floating-point atomics.
//
// Bounds. U rows are `ustride` doubles long, a multiple of 64, and hold 0.0 from `sites` on (the producer writes the
// padding): they are read up to ustride. W rows are `wstride` words apart, a multiple of 4 (16-byte rows), and are read
// for n < sites ONLY: a lane whose four sites reach past the end reads them one by one under a mask. Rows past V or B are
// never read (the lane's operand is 0.0) and never stored.
#pragma once
#include "kernels_common.h"

constexpr unsigned kResampleSplitSites = 2048; // sites per split, at least
constexpr unsigned kResampleMaxSplits = 64;    // ... and splits at most: part[] stays a fraction of U and W

// the split of the sites: a function of the site count alone (host and device agree through ResampleGeo)
static inline unsigned resample_splits(unsigned sites)
{
  const unsigned s = (sites + kResampleSplitSites - 1) / kResampleSplitSites;
  return s < 1u ? 1u : (s > kResampleMaxSplits ? kResampleMaxSplits : s);
}
static inline unsigned resample_split_len(unsigned sites)
{
  const unsigned s = resample_splits(sites);
  return (((sites + s - 1) / s) + 63u) / 64u * 64u;
}

struct ResampleGeo
{
  unsigned V, B;      // rows of U and of W in this launch
  unsigned sites;     // W is read for n < sites
  unsigned ustride;   // doubles per row of U: a multiple of 64, zero from `sites` on
  unsigned wstride;   // words per row of W: a multiple of 4
  unsigned split_len; // sites per split: a multiple of 64
};

typedef double __attribute__((ext_vector_type(4))) rs_double4;
typedef unsigned __attribute__((ext_vector_type(4))) rs_uint4;

// grid (ceil(B / 128), ceil(V / 32), splits), 256 threads
__global__ __launch_bounds__(256) void k_resample_mfma(const double *__restrict__ U, const unsigned *__restrict__ W, double *__restrict__ part,
                                                       const ResampleGeo g)
{
  const unsigned lane = threadIdx.x & 63u;
  const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const unsigned r = lane & 15u, q = lane >> 4;
  const unsigned v0 = blockIdx.y * 32u, b0 = (blockIdx.x * 4u + wave) * 32u;
  if (b0 >= g.B) return; // wave-uniform; the kernel has no barrier
  const unsigned n_begin = blockIdx.z * g.split_len;
  const unsigned n_end = min(n_begin + g.split_len, g.ustride);

  const bool uok[2] = {v0 + r < g.V, v0 + 16u + r < g.V};
  const bool wok[2] = {b0 + r < g.B, b0 + 16u + r < g.B};
  const double *urow[2] = {U + (size_t)(uok[0] ? v0 + r : 0u) * g.ustride, U + (size_t)(uok[1] ? v0 + 16u + r : 0u) * g.ustride};
  const unsigned *wrow[2] = {W + (size_t)(wok[0] ? b0 + r : 0u) * g.wstride, W + (size_t)(wok[1] ? b0 + 16u + r : 0u) * g.wstride};

  rs_double4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = rs_double4{0.0, 0.0, 0.0, 0.0};

  for (unsigned n0 = n_begin; n0 < n_end; n0 += 16u)
  {
    const unsigned n = n0 + 4u * q; // the lane's four sites: n .. n + 3 (n + 3 < ustride)
    rs_double4 a[2];
    double w[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
      a[i] = uok[i] ? *reinterpret_cast<const rs_double4 *>(urow[i] + n) : rs_double4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 2; ++j)
    {
      rs_uint4 x = rs_uint4{0u, 0u, 0u, 0u};
      if (wok[j])
      {
        if (n + 4u <= g.sites)
          x = *reinterpret_cast<const rs_uint4 *>(wrow[j] + n);
        else // the tail: only what lies below `sites` is read
        {
          if (n < g.sites) x.x = wrow[j][n];
          if (n + 1u < g.sites) x.y = wrow[j][n + 1u];
          if (n + 2u < g.sites) x.z = wrow[j][n + 2u];
        }
      }
      w[j][0] = (double)x.x;
      w[j][1] = (double)x.y;
      w[j][2] = (double)x.z;
      w[j][3] = (double)x.w;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i][t], w[j][t], acc[i][j], 0, 0, 0);
  }

  double *out = part + (size_t)blockIdx.z * g.V * g.B;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int t = 0; t < 4; ++t)
      {
        const unsigned v = v0 + 16u * i + q + 4u * t, b = b0 + 16u * j + r;
        if (v < g.V && b < g.B) out[(size_t)v * g.B + b] = acc[i][j][t];
      }
}

// C[v][b] = part[0][v][b] + part[1][v][b] + ... in split order; one thread per element
__global__ __launch_bounds__(256) void k_resample_reduce(const double *__restrict__ part, double *__restrict__ C, unsigned V, unsigned B, unsigned splits)
{
  const size_t idx = (size_t)blockIdx.x * 256u + threadIdx.x, total = (size_t)V * B;
  if (idx >= total) return;
  double s = part[idx];
  for (unsigned k = 1; k < splits; ++k) s += part[(size_t)k * total + idx];
  C[idx] = s;
}
