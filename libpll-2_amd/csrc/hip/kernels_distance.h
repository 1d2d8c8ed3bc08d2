// kernels_distance.h - maximum-likelihood distances between tips (pll_gpu_pairwise_distances).
//
// Both ends of a pair are tips given by codes, so a site's sumtable row
//     sum[k][j] = (sum_{i in a} pi_i Vinv[i][j]) * (sum_{i in b} V[j][i]) = U[a][k][j] * W[b][k][j]
// depends on the pair of codes (a, b) alone: at most ncodes^2 distinct rows, and the alignment enters only through how
// often each code pair occurs. k_distance_code_vectors forms U and W once per call. k_pairwise_distances gives a pair of
// tips to one workgroup from start to end: one pass over the two code rows (a byte per site and tip) and the pattern
// weights into a table of counts in LDS, then the whole safeguarded Newton iteration (kernels_deriv.h: newton_step) on
// that table - an evaluation costs one row per code pair that occurs, not one per site. Nothing is written to HBM but the
// pair's six answers; no workgroup waits for another, and the loop is bounded by max_iters.
//
// The alignment is read through one row of weights, so a pair can be served under many rows (pll_gpu_bootstrap_distance_trees,
// DESIGN.md section 5.17): distance_pair is the one body over (weight row, result block); k_pairwise_distances calls it with
// the partition's row, k_pairwise_distances_rows with row rep0 + blockIdx.z of a table of rows `wstride` words apart (the
// layout k_rell_draw writes; a multiple of 4, so the uint4 loads stay aligned) and result block 6 count^2 doubles times that
// row further on.
#pragma once
#include "kernels_common.h"
#include "kernels_deriv.h"
#include "kernels_gradient.h" // branch_diag

struct DevDistance
{
  const unsigned char *const *rows;    // [count] the code row of every tip of the list
  const unsigned *pattern_weights;     // [sites]; k_pairwise_distances_rows: [rows][wstride]
  const double *uw;                    // U [ncodes][R][S], then W [R][S][ncodes]
  const unsigned long long *tipmap;    // code -> state mask, or null: the code is the mask (4 states)
  const double *freqs, *rate_weights;  // the model as deriv_rate_add_share reads it (no prop_invar: refused)
  double *results;                     // [6][count][count]: distance, p_distance, d_f, dd_f, status, iterations
  double t_first, t_min, t_max, tolerance;
  unsigned max_iters;
  unsigned sites, count, row0;         // the launch holds rows row0 .. row0 + gridDim.y of the pair matrix
  unsigned rep0, wstride;              // k_pairwise_distances_rows: the launch holds the weight rows rep0 .. rep0 + gridDim.z
  unsigned ncodes;
  unsigned copies, copy_stride;        // private count tables in LDS: thread % copies owns one, copy_stride words apart
  unsigned char fidx[kMaxRates];
};

// U[c][k][j] = sum_{i in c} m1[k][i][j], W likewise from m2 (the PT layout: the state is the slow index), the states in
// increasing order. One thread per (code, rate, eigen index) and side. W is stored with the code as the fast index: the
// threads of k_pairwise_distances that evaluate neighbouring code pairs (a, b), (a, b + 1), ... read one U value between them
// and neighbouring W values.
__global__ __launch_bounds__(256) void k_distance_code_vectors(const double *__restrict__ m1, const double *__restrict__ m2,
                                                               const unsigned long long *__restrict__ tipmap, unsigned ncodes, unsigned S,
                                                               unsigned SPT, unsigned R, double *__restrict__ uw)
{
  const unsigned per_side = ncodes * R * S;
  const unsigned idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= 2u * per_side) return;
  const unsigned side = idx / per_side, e = idx % per_side;
  const unsigned c = e / (R * S), k = (e / S) % R, j = e % S;
  const unsigned long long mask = tip_mask(tipmap, c);
  const double *m = (side ? m2 : m1) + (size_t)k * S * SPT + j;
  double s = 0.0;
  for (unsigned i = 0; i < S; ++i)
    if ((mask >> i) & 1ull) s += m[(size_t)i * SPT];
  uw[side ? per_side + (size_t)(k * S + j) * ncodes + c : idx] = s;
}

__device__ __forceinline__ void distance_count(unsigned *mine, unsigned ncodes, unsigned a, unsigned b, unsigned w)
{
  // (a code beyond the table cannot come from the host layer; it is dropped, never an address)
  if (w && a < ncodes && b < ncodes) atomicAdd(&mine[a * ncodes + b], w);
}

// the pair (x, y) of list positions, x < y, under one row of weights: every thread of the workgroup calls
__device__ __forceinline__ void distance_pair(const DevDistance &d, const DevDiag &dg, const unsigned *__restrict__ weights,
                                              double *__restrict__ results)
{
  const unsigned x = d.row0 + blockIdx.y, y = blockIdx.x;
  if (y <= x) return;
  __shared__ double ws[2][4];
  __shared__ unsigned psum[2];
  __shared__ NewtonState st;
  extern __shared__ double dyn[]; // the diag table [R][S][4], then the counts
  double *const ldiag = dyn;
  unsigned *const counts = reinterpret_cast<unsigned *>(dyn + (size_t)dg.R * dg.S * 4);
  const unsigned nc = d.ncodes, cells = nc * nc;
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;

  for (unsigned i = threadIdx.x; i < d.copies * d.copy_stride; i += blockDim.x) counts[i] = 0u;
  if (threadIdx.x < 2u) psum[threadIdx.x] = 0u;
  __syncthreads();

  // ---- the histogram: n_ab = the summed pattern weight of the sites that show (a, b). Four sites per thread and step;
  // equal keys of a wave meet in different tables (a thread's own, an odd number of words apart: different banks)
  {
    const unsigned char *ra = d.rows[x], *rb = d.rows[y];
    unsigned *mine = counts + (threadIdx.x & (d.copies - 1u)) * d.copy_stride;
    const unsigned quads = d.sites / 4u;
    const unsigned *ra4 = reinterpret_cast<const unsigned *>(ra), *rb4 = reinterpret_cast<const unsigned *>(rb);
    const uint4 *w4 = reinterpret_cast<const uint4 *>(weights);
    for (unsigned q = threadIdx.x; q < quads; q += blockDim.x)
    {
      const unsigned a = ra4[q], b = rb4[q];
      const uint4 w = w4[q];
      distance_count(mine, nc, a & 255u, b & 255u, w.x);
      distance_count(mine, nc, (a >> 8) & 255u, (b >> 8) & 255u, w.y);
      distance_count(mine, nc, (a >> 16) & 255u, (b >> 16) & 255u, w.z);
      distance_count(mine, nc, a >> 24, b >> 24, w.w);
    }
    for (unsigned n = quads * 4u + threadIdx.x; n < d.sites; n += blockDim.x) distance_count(mine, nc, ra[n], rb[n], weights[n]);
  }
  __syncthreads();

  // ---- the tables added into the first (integers: any order gives the same counts), and the two sums of the p-distance
  {
    const unsigned long long full = full_mask(dg.S);
    unsigned differ = 0u, compared = 0u;
    for (unsigned e = threadIdx.x; e < cells; e += blockDim.x)
    {
      unsigned n = 0u;
      for (unsigned c = 0; c < d.copies; ++c) n += counts[c * d.copy_stride + e];
      counts[e] = n; // (column e of every table is this thread's alone)
      if (!n) continue;
      const unsigned long long ma = tip_mask(d.tipmap, e / nc), mb = tip_mask(d.tipmap, e % nc);
      if (!(ma & mb)) differ += n;
      if (ma != full && mb != full) compared += n;
    }
    if (differ) atomicAdd(&psum[0], differ);
    if (compared) atomicAdd(&psum[1], compared);
  }
  if (threadIdx.x == 0)
  {
    newton_open(st, d.t_min, d.t_max);
    st.t = d.t_first;
    st.status = kNewtonRunning;
  }
  __syncthreads();

  // ---- the iteration: at most max_iters evaluations, each over the code pairs that occur
  const double *U = d.uw, *W = d.uw + (size_t)nc * dg.R * dg.S; // W [R][S][nc]
  for (unsigned it = 0; it < d.max_iters; ++it)
  {
    const double t = st.t;
    branch_diag(dg, t, ldiag); // (ends with a barrier)
    double a1 = 0.0, a2 = 0.0;
    for (unsigned e = threadIdx.x; e < cells; e += blockDim.x)
    {
      const unsigned n = counts[e];
      if (!n) continue;
      const double *ua = U + (size_t)(e / nc) * dg.R * dg.S, *wb = W + e % nc;
      double lk0 = 0.0, lk1 = 0.0, lk2 = 0.0;
      for (unsigned k = 0; k < dg.R; ++k)
      {
        double c0 = 0.0, c1 = 0.0, c2 = 0.0;
        const double *dk = ldiag + (size_t)k * dg.S * 4;
        // (four steps' loads of U and W issued together)
#pragma unroll 4
        for (unsigned j = 0; j < dg.S; ++j)
        {
          const double s = ua[k * dg.S + j] * wb[(size_t)(k * dg.S + j) * nc];
          c0 = fma(s, dk[j * 4 + 0], c0);
          c1 = fma(s, dk[j * 4 + 1], c1);
          c2 = fma(s, dk[j * 4 + 2], c2);
        }
        double unused;
        deriv_rate_add_share<false>(d.freqs, nullptr, d.rate_weights, d.fidx[k], dg.SP, k, -1, c0, c1, c2, lk0, lk1, lk2, unused);
      }
      deriv_site_add(lk0, lk1, lk2, (double)n, a1, a2);
    }
    a1 = wave_sum(a1);
    a2 = wave_sum(a2);
    if (lane == 0)
    {
      ws[0][wave] = a1;
      ws[1][wave] = a2;
    }
    __syncthreads();
    if (threadIdx.x == 0)
      newton_step(st, t, (ws[0][0] + ws[0][1]) + (ws[0][2] + ws[0][3]), (ws[1][0] + ws[1][1]) + (ws[1][2] + ws[1][3]), d.t_min, d.t_max,
                  d.tolerance, d.max_iters);
    __syncthreads();
    if (st.status != kNewtonRunning) break; // the same word in every thread
  }

  if (threadIdx.x < 6u)
  {
    const unsigned v = threadIdx.x;
    const double value = v == 0u   ? st.t
                         : v == 1u ? (psum[1] ? (double)psum[0] / (double)psum[1] : 0.0)
                         : v == 2u ? st.d_f
                         : v == 3u ? st.dd_f
                         : v == 4u ? (double)st.status
                                   : (double)st.iterations;
    double *block = results + (size_t)v * d.count * d.count;
    block[(size_t)x * d.count + y] = value;
    block[(size_t)y * d.count + x] = value;
  }
}

__global__ __launch_bounds__(256) void k_pairwise_distances(const DevDistance d, const DevDiag dg)
{
  distance_pair(d, dg, d.pattern_weights, d.results);
}

__global__ __launch_bounds__(256) void k_pairwise_distances_rows(const DevDistance d, const DevDiag dg)
{
  const size_t z = d.rep0 + blockIdx.z;
  distance_pair(d, dg, d.pattern_weights + z * d.wstride, d.results + z * 6u * d.count * d.count);
}
