// kernels_gradient.h - the branch-length gradient (pll_gpu_branch_derivatives).
//
// "What are the first and second derivatives of -lnL with respect to this branch?" - asked for every branch of a list in
// ONE launch. Per branch the reference runs pll_update_sumtable (src/derivatives.c:239-324), which writes a CLV-sized
// table, and pll_compute_likelihood_derivatives (:333-418, src/core_derivatives.c:643-849), which reads it back. For one
// evaluation per branch the table is pure overhead: its row of a (site, rate),
//     sum[j] = (sum_i p_i pi_i Vinv[i][j]) * (sum_i V[j][i] c_i),
// is two small matrix-vector products and their element-wise product, contracted at once with the branch's own
// diag[k][j] = (e, l e, l^2 e). Here a row exists in registers only: a branch costs one read of its two ends, no table, no
// write to HBM and no launch of its own. Nothing is written but two partial sums per workgroup, handed off side by side
// through plc_publish_chunk<2> (kernels_placement.h): value (d_f | dd_f, branch) owns gridDim.x slots and a ticket, so its
// bits depend on its own workgroups alone.
//
// Grid: x = the site tiles exactly as launch_insertions cuts them (a function of the site count alone), y = the branch.
// The model travels in a DevEdge (parent, child, mat and the scalers unused; block_sums / counter / result = the slots
// [value][branch of the launch][workgroup], a ticket per value, the results [value][branch of the call]) and a DevDiag
// (eigenvalues, rates, prop_invar; diag unused: no table of a branch stands in HBM); m1 / m2 are the two contraction
// matrices in the PT layout (matrix slots prob_matrices and prob_matrices + 1). The ends and the length of branch y are
// branches[y], read through the scalar path. As in pll_update_sumtable an end given by codes takes the `left` role (m1);
// otherwise the parent is left and the child right. Whether an end is a tip is a wave-uniform branch.
//
// Per-site scaling cancels in L'/L: no scaler is read. Per-rate scalers: column k of a site is multiplied by
// 2^(-256 min(s_k - min_k s_k, 4)), s_k = the two ends' counts added (src/core_derivatives.c:420-460) - what
// k_sumtable_excess does to a table, here applied to the row before it is contracted, as the reference's table holds it.
//
// CAT (pll_gpu_branch_category_derivatives / pll_gpu_rate_gradient): the same two kernels keep what
// they otherwise drop - category k's share c1_k w_k of the site's L' - and sum pw * (-(c1_k w_k) / L) per category beside
// the two sums. A workgroup then publishes R + 2 values per branch (d_f, dd_f, d_cat[0..R)) through the same hand-off,
// in chunks of at most 32; value v of branch y owns its slots and its ticket, and the sums that exist are formed in the
// order they have without CAT. k_rate_gradient contracts the results with the branch lengths and the rates.
#pragma once
#include "kernels_common.h"
#include "kernels_dna.h"
#include "kernels_generic.h"
#include "kernels_deriv.h" // (after kernels_generic.h: it uses tiled_base)
#include "kernels_placement.h"

struct BranchDesc // 64 bytes
{
  const double *left, *right;        // CLV of the end, or null: a tip given by codes
  const unsigned char *ltip, *rtip;  // tip codes or null
  const unsigned *lscaler, *rscaler; // per-rate scalers only; null: the end carries no scaler (or the mode reads none)
  double t;                          // the branch length
  double pad_;
};
typedef const BranchDesc __attribute__((address_space(4))) *cbranch_p;

__device__ __forceinline__ BranchDesc branch_get(const BranchDesc *branches, unsigned y)
{
  cbranch_p p = (cbranch_p)(uintptr_t)branches + y;
  BranchDesc r;
  r.left = p->left;
  r.right = p->right;
  r.ltip = p->ltip;
  r.rtip = p->rtip;
  r.lscaler = p->lscaler;
  r.rscaler = p->rscaler;
  r.t = p->t;
  r.pad_ = 0.0;
  return r;
}

// the branch's diag table, [R][S][4] = (e, l e, l^2 e, 0), formed by the workgroup itself from the branch's own length:
// derivative_sums' local_diag way, with no copy left in HBM
__device__ __forceinline__ void branch_diag(const DevDiag &dg, double t, double *ldiag)
{
  for (unsigned idx = threadIdx.x; idx < dg.R * dg.S; idx += blockDim.x) diag_entry(dg, t, idx, ldiag + (size_t)idx * 4);
  __syncthreads();
}

// 2^(-256 excess) of rate k, or 1
__device__ __forceinline__ double excess_factor(unsigned rs, unsigned mn)
{
  const unsigned ex = rate_excess(rs, mn);
  return ex ? minlh(ex) : 1.0;
}

// The workgroup's V values of its branch through plc_publish_chunk, QCH at a time: value(v) is the wave's share of value v
// (anything for v >= V). The hand-off's words in LDS are last read before a barrier that every wave has passed when a
// round ends, so the next round may write them.
template <int QCH, class Value>
__device__ __forceinline__ void publish_values(const DevEdge &e, unsigned V, unsigned res_stride, unsigned nsum_waves, Value value)
{
  for (unsigned q0 = 0; q0 < V; q0 += QCH)
  {
    double vals[QCH];
#pragma unroll
    for (int j = 0; j < QCH; ++j) vals[j] = value(q0 + (unsigned)j);
    plc_publish_chunk<QCH>(e, q0, min((unsigned)QCH, V - q0), res_stride, vals, nsum_waves);
  }
}

// ------------------------------------------------------------------------------------------------
// 4 states x 4 rates: one wave per 64-site tile, the lane owns its site. Per rate the two ends (8 doubles, or decoded
// codes), the two 4 x 4 products with the contraction-matrix coefficients through the scalar path, the row, its excess
// factor and the three contractions with the branch's diag row (16 x 4 doubles in LDS, wave-uniform addresses). No node
// is kept: register use is small (report in DESIGN.md section 5.9). CAT: the lane owns all four rates, so the four shares
// and their four sums live in registers.
template <bool CAT>
__global__ __launch_bounds__(256) void k_gradient_dna(const DevEdge e, const DevDiag dg, const BranchDesc *branches, const double *m1,
                                                      const double *m2, unsigned res_stride, unsigned tiles_per_wave)
{
  __shared__ double ldiag[16 * 4];
  const BranchDesc b = branch_get(branches, blockIdx.y);
  branch_diag(dg, b.t, ldiag);
  cdouble_p lm = as_const(m1), rm = as_const(m2);
  const int smode = e.per_rate ? 2 : 0; // per-site counts cancel: not read
  double a1 = 0.0, a2 = 0.0;
  double acat[4] = {0.0, 0.0, 0.0, 0.0}; // CAT

  for (unsigned t = 0; t < tiles_per_wave; ++t)
  {
    DnaTile w;
    if (!dna_tile(w, blockIdx.x, tiles_per_wave, t, e.sites)) break;
    const unsigned n = w.n;
    const uint4 ls = dna_load_scaler(b.lscaler, n, smode), rs = dna_load_scaler(b.rscaler, n, smode);
    const unsigned sk[4] = {ls.x + rs.x, ls.y + rs.y, ls.z + rs.z, ls.w + rs.w};
    const unsigned mn = min(min(sk[0], sk[1]), min(sk[2], sk[3]));
    const int inv = e.invariant ? e.invariant[n] : -1;
    const unsigned lcode = b.ltip ? b.ltip[n] : 0u, rcode = b.rtip ? b.rtip[n] : 0u; // wave-uniform choices
    double lk0 = 0.0, lk1 = 0.0, lk2 = 0.0;
    double share[4]; // CAT
#pragma unroll
    for (int k = 0; k < 4; ++k)
    {
      double xl[4], xr[4], pa[4], pb[4];
      if (b.ltip)
        dna_fetch<true>(xl, nullptr, k, lcode);
      else
        dna_fetch<false>(xl, b.left + w.off, k, 0u);
      if (b.rtip)
        dna_fetch<true>(xr, nullptr, k, rcode);
      else
        dna_fetch<false>(xr, b.right + w.off, k, 0u);
      dna_matvec(pa, lm + k * 16, xl);
      dna_matvec(pb, rm + k * 16, xr);
      const double f = excess_factor(sk[k], mn);
      // the rate's diag row, read where it is used: an offset the compiler takes as new keeps it from holding all 48
      // values in vector registers from the top of the kernel to its end (96 registers, two waves per SIMD)
      unsigned row = k * 16u;
      asm volatile("" : "+v"(row));
      double c0 = 0.0, c1 = 0.0, c2 = 0.0;
#pragma unroll
      for (int j = 0; j < 4; ++j)
      {
        const double s = pa[j] * pb[j] * f;
        const double *dk = ldiag + row + j * 4;
        c0 = fma(s, dk[0], c0);
        c1 = fma(s, dk[1], c1);
        c2 = fma(s, dk[2], c2);
      }
      deriv_rate_add_share<CAT>(e.freqs, e.prop_invar, e.rate_weights, e.fidx[k], 4u, k, inv, c0, c1, c2, lk0, lk1, lk2, share[k]);
    }
    if (w.valid)
    {
      const double pw = (double)e.pattern_weights[n];
      deriv_site_add(lk0, lk1, lk2, pw, a1, a2);
      if (CAT)
      {
#pragma unroll
        for (int k = 0; k < 4; ++k) acat[k] += pw * (-share[k] / lk0);
      }
    }
  }
  if (CAT)
  {
    const double sums[6] = {wave_sum(a1), wave_sum(a2), wave_sum(acat[0]), wave_sum(acat[1]), wave_sum(acat[2]), wave_sum(acat[3])};
    plc_publish_chunk<6>(e, 0u, 6u, res_stride, sums, 4u);
  }
  else
  {
    const double sums[2] = {wave_sum(a1), wave_sum(a2)};
    plc_publish_chunk<2>(e, 0u, 2u, res_stride, sums, 4u);
  }
}

// ------------------------------------------------------------------------------------------------
// Every other shape (up to 64 states, any rate count): the tiled kernels' walk (kernels_generic.h: gen_tile) - workgroup =
// one tile of one branch at a time, wave w of min(R, 4) owns the rate categories w, w + nw, ... - and their end_product:
// a tip is decoded through the tipmap. The branch's diag table stands in LDS ([R][S][4]: 7.8 KB at 61 x 4). A wave leaves its
// rates' share of the site's (L, L', L'') in LDS; wave 0 adds the shares in wave order and forms the site's two terms.
// CAT: L of a site exists only once the waves' shares are added, so a wave parks the c1 w of its categories in LDS
// (cshare, [R][64]) and, after the barrier, adds the shares of L in wave 0's order and sums pw * (-(c1 w) / L) per category
// into acat ([R][64], LDS as well: a wave owns any number of categories and indexes them at run time). Both rows of a
// category are written and read by the wave that owns it; wave 0 reads every acat row once, after a barrier, to publish.
template <int ICH, bool CAT>
__global__ __launch_bounds__(256) void k_gradient_tiled(const DevEdge e, const DevDiag dg, const BranchDesc *branches, const double *m1,
                                                        const double *m2, const GenGeo g, const unsigned long long *__restrict__ tipmap,
                                                        unsigned res_stride, unsigned tiles_per_block)
{
  __shared__ double part[3][4][64];
  extern __shared__ double ldiag[]; // [R][S][4]; CAT: then cshare [R][64] and acat [R][64]
  const BranchDesc b = branch_get(branches, blockIdx.y);
  branch_diag(dg, b.t, ldiag);
  const unsigned lane = gen_lane(), wave = gen_wave();
  double *const cshare = ldiag + (size_t)g.R * g.S * 4, *const acat = cshare + (size_t)g.R * 64;
  // (through the scalar path by hand: branch_diag's per-lane stride has the workgroup size in a vector register, and a rate
  // loop stepping by a vector register reads its matrix coefficients with vector loads)
  const unsigned nw = __builtin_amdgcn_readfirstlane(blockDim.x >> 6);
  const bool ltip = b.ltip != nullptr, rtip = b.rtip != nullptr; // wave-uniform
  const unsigned *lsc = e.per_rate ? b.lscaler : nullptr, *rsc = e.per_rate ? b.rscaler : nullptr;
  double a1 = 0.0, a2 = 0.0;
  if (CAT)
    for (unsigned k = wave; k < g.R; k += nw) acat[k * 64u + lane] = 0.0;

  for (unsigned t = 0; t < tiles_per_block; ++t)
  {
    if (!gen_has_tile(tiles_per_block, t, e.sites)) break;
    const GenTile w = gen_tile(tiles_per_block, t, e.sites);
    const unsigned n = w.n, nn = w.nn;
    const bool valid = w.valid;
    const unsigned long long lmask = ltip ? tip_mask(tipmap, b.ltip[nn]) : 0ull;
    const unsigned long long rmask = rtip ? tip_mask(tipmap, b.rtip[nn]) : 0ull;
    const GenEnd le = gen_end(m1, ltip, b.left, nn, g, lmask), re = gen_end(m2, rtip, b.right, nn, g, rmask);
    const unsigned mn = e.per_rate ? scaler_min(lsc, nn, rsc, nn, g.R) : 0u;
    const int inv = e.invariant ? e.invariant[nn] : -1;

    double lk0 = 0.0, lk1 = 0.0, lk2 = 0.0;
    for (unsigned k = wave; k < g.R; k += nw)
    {
      const double f = e.per_rate ? excess_factor(scaler_sum_rate(lsc, nn, rsc, nn, g.R, k), mn) : 1.0;
      double c0 = 0.0, c1 = 0.0, c2 = 0.0;
      for (unsigned ch = 0; ch < g.nchunks; ++ch)
      {
        double v[ICH];
        end_product<ICH>(v, le, re, k, ch, g);
        const double *dk = ldiag + ((size_t)k * g.S + ch * ICH) * 4; // wave-uniform addresses: LDS broadcast
#pragma unroll
        for (int i = 0; i < ICH; ++i)
          if (ch * ICH + i < g.S)
          {
            const double s = v[i] * f;
            c0 = fma(s, dk[i * 4 + 0], c0);
            c1 = fma(s, dk[i * 4 + 1], c1);
            c2 = fma(s, dk[i * 4 + 2], c2);
          }
      }
      double share;
      deriv_rate_add_share<CAT>(e.freqs, e.prop_invar, e.rate_weights, e.fidx[k], g.SP, k, inv, c0, c1, c2, lk0, lk1, lk2, share);
      if (CAT) cshare[k * 64u + lane] = share;
    }
    part[0][wave][lane] = lk0;
    part[1][wave][lane] = lk1;
    part[2][wave][lane] = lk2;
    __syncthreads();
    if (wave == 0 && valid)
    {
      double s[3];
      wave_order_sums(s, &part[0][0][lane], nw);
      deriv_site_add(s[0], s[1], s[2], (double)e.pattern_weights[n], a1, a2);
    }
    if (CAT && valid)
    {
      double s[1]; // the site's L, as wave 0 adds it
      wave_order_sums(s, &part[0][0][lane], nw);
      const double pw = (double)e.pattern_weights[n];
      for (unsigned k = wave; k < g.R; k += nw) acat[k * 64u + lane] += pw * (-cshare[k * 64u + lane] / s[0]);
    }
    __syncthreads(); // part[] is reused by the next tile
  }
  // only wave 0 holds sums
  if (CAT)
  {
    // (the barrier that ends the last tile stands between the waves' last acat and wave 0's reads)
    const unsigned V = g.R + 2u;
    auto value = [&](unsigned v) {
      if (wave != 0 || v >= V) return 0.0;
      return wave_sum(v == 0 ? a1 : v == 1 ? a2 : acat[(v - 2u) * 64u + lane]);
    };
    if (V <= 8u)
      publish_values<8>(e, V, res_stride, 1u, value);
    else
      publish_values<32>(e, V, res_stride, 1u, value);
  }
  else
  {
    const double sums[2] = {wave == 0 ? wave_sum(a1) : 0.0, wave == 0 ? wave_sum(a2) : 0.0};
    plc_publish_chunk<2>(e, 0u, 2u, res_stride, sums, 1u);
  }
}

// ------------------------------------------------------------------------------------------------
// The contraction of a call's results with the branch lengths and the rates: one workgroup, after the last cut on the same
// stream. results = [R + 2][count] as the kernels above leave them (d_f, dd_f, d_cat[0..R)), lengths = [count].
//   out[k] = sum_i (t_i / r_k) d_cat[i][k]  (k < R)        out[R] = sum_i t_i d_f[i]
// each added in list order by one thread, so the bits are those of the same loop on the host. A thread that walked its row
// in HBM would wait for one dependent load per branch; the rows come through LDS instead, kRateRows branches at a time with
// coalesced loads (rows kRateRows + 1 apart: the R + 1 walkers read different banks).
constexpr unsigned kRateRows = 64;

__global__ __launch_bounds__(256) void k_rate_gradient(const double *__restrict__ results, const double *__restrict__ lengths,
                                                       const double *__restrict__ rates, unsigned count, unsigned R, double *__restrict__ out)
{
#pragma clang fp contract(off) // a product is rounded before it is added: what the definition's sum says
  extern __shared__ double rows[]; // [R + 2][kRateRows + 1]: d_cat[0..R), d_f, the lengths
  const unsigned stride = kRateRows + 1u;
  const unsigned me = threadIdx.x;
  const double r = me < R ? rates[me] : 1.0;
  double acc = 0.0;
  for (unsigned i0 = 0; i0 < count; i0 += kRateRows)
  {
    const unsigned n = min(kRateRows, count - i0);
    for (unsigned idx = threadIdx.x; idx < (R + 2u) * kRateRows; idx += blockDim.x)
    {
      const unsigned row = idx / kRateRows, i = idx % kRateRows;
      if (i < n) rows[row * stride + i] = row < R ? results[(size_t)(row + 2u) * count + i0 + i] : row == R ? results[i0 + i] : lengths[i0 + i];
    }
    __syncthreads();
    if (me <= R)
      for (unsigned i = 0; i < n; ++i)
      {
        const double t = rows[(R + 1u) * stride + i], v = rows[me * stride + i];
        const double f = me < R ? t / r : t;
        const double term = f * v;
        acc = acc + term;
      }
    __syncthreads(); // rows[] is reused by the next piece
  }
  if (me <= R) out[me] = acc;
}
