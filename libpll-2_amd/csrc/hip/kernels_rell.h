// kernels_rell.h - replicate site weights drawn on the device (pllamd/rell.py restates the
// definition in integer arithmetic and is what these kernels are held to, bit for bit).
//
// The partition has pattern weights p[0..sites), total = sum p, cdf[n] = p[0] + ... + p[n]. Replicate b is `total` draws;
// draw j takes a 64-bit word x(seed, b, j) from Philox-4x32-10 - key = the two halves of the seed, counter =
// (j >> 1, 0, b, kRellTag), even j words 0-1 (word 1 the high half), odd j words 2-3 - forms r = floor(x total / 2^64) and
// increments w_b[n] for the first n with cdf[n] > r. Nothing is carried from draw to draw, so a row is a function of
// (seed, b, p) alone and any thread can regenerate any draw.
//
// k_rell_cdf: one workgroup, the inclusive 64-bit prefix sum of p in blocks of 1024 sites, and a two-word summary
// {total, number of sites whose weight is not 1}. Once per change of the weights.
//
// k_rell_draw: grid (rows, ranges), 1024 threads. A workgroup owns (row, sites [n0, n0 + H)) and keeps the range's
// counters in LDS. It walks ALL draws of its replicate - thread t the Philox blocks t, t + 1024, ... of two draws each -
// keeps those with cdf_lo <= r < cdf_hi (the range's two bounds: wave-uniform, read once), finds the site by binary search
// over the range's slice of the cdf (or takes n = r when every weight is 1: cdf[n] = n + 1, the same function without a
// load), and counts with an LDS atomic add. No global atomics: after a barrier the range goes out once, with plain
// 16-byte stores, the row's padding up to wstride as 0. Every word of a row is written exactly once per launch.
//
// Bounds. cdf is read at n0 - 1 (n0 > 0), n1 - 1 and inside [n0, n1) only, n1 = min(n0 + H, sites) <= sites. LDS holds
// hw = min(H, wstride - n0) words (a multiple of 4; the launch gives min(H, wstride) words); a kept draw's site lies in
// [n0, n1), n1 - n0 <= hw. The stores cover words [n0, n0 + hw) of the row, n0 + hw <= wstride. total < 2^32 (the caller
// checks), so j and the Philox block number fit 32 bits.
#pragma once
#include "kernels_common.h"

// H and the workgroup size, by measurement (61 quartets x 100k sites x 1000 rows on one MI355X, the draw launch alone,
// profiles/quartet_rell.json): H = 16384 (64 KB of LDS, two workgroups per CU, 7 ranges per row) 0.99 ms with 256 threads and
// 0.87 ms with 1024; H = 32768 (128 KB, one workgroup per CU, 4 ranges per row) 0.81 ms with 256 and 0.60 ms with 1024. A
// workgroup regenerates every draw of its row whatever its range holds, so the work is ranges x total per row and fewer,
// larger ranges win; sixteen waves hide the latency of the dependent 32-bit multiplies and of the LDS atomics that four do not.
constexpr unsigned kRellThreads = 1024;
constexpr unsigned kRellRange = 32768;       // H: sites per workgroup at most (128 KB of LDS: one workgroup per CU)
constexpr unsigned kRellTag = 0x52454C4Cu;   // "RELL": the counter's domain word
constexpr unsigned kRellCdfBlock = 4u * 256; // sites per step of k_rell_cdf

typedef unsigned __attribute__((ext_vector_type(4))) rell_uint4;

// Philox-4x32-10 (Salmon et al., SC'11): ten rounds, the key bumped by the Weyl constants between them
__device__ __forceinline__ rell_uint4 rell_philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1)
{
#pragma unroll
  for (int round = 0; round < 10; ++round)
  {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return rell_uint4{c0, c1, c2, c3};
}

// floor((high 2^32 + low) total / 2^64) for total < 2^32: no intermediate leaves 64 bits
__device__ __forceinline__ unsigned rell_scaled(unsigned high, unsigned low, unsigned total)
{
  return (unsigned)(((unsigned long long)high * total + (((unsigned long long)low * total) >> 32)) >> 32);
}

struct RellGeo
{
  unsigned long long seed;
  unsigned first;   // absolute number of the launch's row 0
  unsigned total;   // draws per row
  unsigned sites;
  unsigned wstride; // words per row: a multiple of 4
  unsigned range;   // H of this launch: a multiple of 4
};

template <bool UNIT>
__device__ __forceinline__ void rell_count(unsigned *counts, const unsigned long long *__restrict__ cdf, unsigned r, unsigned n0, unsigned n1,
                                           unsigned long long lo, unsigned long long hi)
{
  if (UNIT)
  {
    if (r >= n0 && r < n1) atomicAdd(&counts[r - n0], 1u);
    return;
  }
  if (r < lo || r >= hi) return;
  // the first n in [n0, n1) with cdf[n] > r: cdf[n0 - 1] = lo <= r < hi = cdf[n1 - 1]
  unsigned a = n0, b = n1 - 1u;
  while (a < b)
  {
    const unsigned m = a + (b - a) / 2u;
    if (cdf[m] > r) b = m;
    else a = m + 1u;
  }
  atomicAdd(&counts[a - n0], 1u);
}

template <bool UNIT>
__global__ __launch_bounds__(kRellThreads) void k_rell_draw(const unsigned long long *__restrict__ cdf, unsigned *__restrict__ W, const RellGeo g)
{
  extern __shared__ unsigned rell_counts[];
  const unsigned n0 = blockIdx.y * g.range;
  const unsigned n1 = min(n0 + g.range, g.sites);
  const unsigned hw = min(g.range, g.wstride - n0);
  for (unsigned i = threadIdx.x; i < hw; i += blockDim.x) rell_counts[i] = 0u;
  __syncthreads();

  unsigned long long lo = 0, hi = 0;
  if (!UNIT)
  {
    lo = n0 ? cdf[n0 - 1u] : 0ull;
    hi = cdf[n1 - 1u];
  }
  const unsigned k0 = (unsigned)g.seed, k1 = (unsigned)(g.seed >> 32);
  const unsigned b = g.first + blockIdx.x;
  const unsigned blocks = g.total / 2u + (g.total & 1u);
  if (UNIT || hi > lo) // (a range of weight 0 keeps no draw)
    for (unsigned k = threadIdx.x; k < blocks; k += blockDim.x)
    {
      const rell_uint4 o = rell_philox(k, 0u, b, kRellTag, k0, k1);
      rell_count<UNIT>(rell_counts, cdf, rell_scaled(o.y, o.x, g.total), n0, n1, lo, hi);
      if (2u * k + 1u < g.total) rell_count<UNIT>(rell_counts, cdf, rell_scaled(o.w, o.z, g.total), n0, n1, lo, hi);
    }
  __syncthreads();

  unsigned *row = W + (size_t)blockIdx.x * g.wstride + n0;
  for (unsigned i = 4u * threadIdx.x; i < hw; i += 4u * blockDim.x)
    *reinterpret_cast<rell_uint4 *>(row + i) = rell_uint4{rell_counts[i], rell_counts[i + 1u], rell_counts[i + 2u], rell_counts[i + 3u]};
}

// one workgroup of 256 threads: cdf[n] = p[0] + ... + p[n]; summary[0] = total, summary[1] = the sites with p[n] != 1
__global__ __launch_bounds__(256) void k_rell_cdf(const unsigned *__restrict__ p, unsigned long long *__restrict__ cdf,
                                                  unsigned long long *__restrict__ summary, unsigned sites)
{
  __shared__ unsigned long long part[256];
  __shared__ unsigned odd[256];
  const unsigned t = threadIdx.x;
  unsigned long long carry = 0;
  unsigned not_one = 0;
  for (unsigned base = 0; base < sites; base += kRellCdfBlock)
  {
    // four consecutive sites per thread, an inclusive scan of the threads' sums (Hillis-Steele over LDS), the carry of the blocks before
    const unsigned n = base + 4u * t;
    unsigned v[4];
#pragma unroll
    for (unsigned i = 0; i < 4; ++i)
    {
      v[i] = n + i < sites ? p[n + i] : 0u;
      not_one += (n + i < sites && v[i] != 1u) ? 1u : 0u;
    }
    const unsigned long long own = (unsigned long long)v[0] + v[1] + v[2] + v[3];
    part[t] = own;
    __syncthreads();
    for (unsigned d = 1; d < 256u; d *= 2u)
    {
      const unsigned long long add = t >= d ? part[t - d] : 0ull;
      __syncthreads();
      part[t] += add;
      __syncthreads();
    }
    unsigned long long run = carry + part[t] - own;
#pragma unroll
    for (unsigned i = 0; i < 4; ++i)
    {
      run += v[i];
      if (n + i < sites) cdf[n + i] = run;
    }
    carry += part[255];
    __syncthreads(); // part[] is rewritten by the next block
  }
  odd[t] = not_one;
  __syncthreads();
  for (unsigned d = 128; d > 0; d /= 2u)
  {
    if (t < d) odd[t] += odd[t + d];
    __syncthreads();
  }
  if (t == 0)
  {
    summary[0] = carry;
    summary[1] = odd[0];
  }
}
