// kernels_ancestral.h - marginal ancestral state probabilities of one node (pll_compute_node_ancestral,
// src/likelihood.c:639-823), one launch per node.
//
// For site n and state j, with x the node's CLV, y the CLV (or tip codes) at the other end of the branch, P the
// branch's transition matrix, pi_f(k) the frequency set of rate category k and w the rate weights:
//
//     a[n][j] = sum_k  w_k * pi_f(k)[j] * x_k[n][j] * (P_k y_k[n])[j]          out[n][j] = a[n][j] / sum_j a[n][j]
//
// This is src/likelihood.c:691-753 with the identity matrix on the node's side folded away. The reference writes the
// product CLV x * (P y) to a temporary of sites x rates x states_padded doubles and reads it back; here it never
// leaves registers: two CLVs (or one CLV and one byte of tip code per site) come in, sites x states doubles go out
// in the reference's layout out[n * states + j], unpadded and site-major.
//
// Scaling. The result is a ratio per site, so every factor common to a site cancels:
//   * per-site scalers: the counts of the two ends are not read at all;
//   * the reference's fresh 2^256 rescale of the product (src/core_partials.c:729-763) cancels as well. What it
//     protects - the mix with w_k * pi[j] pushing a small product into the subnormal range - is protected here by
//     carrying the constant 2^256 in the mix weight: (w_k * 2^256) * pi[j] is exact, is applied to every term of
//     every site, and cancels in the division. A term is subnormal only if x * (P y) itself already was;
//   * PLL_ATTRIB_RATE_SCALERS - DELIBERATELY DIFFERENT FROM THE REFERENCE. The reference ignores the per-rate counts
//     of both ends, rescales each rate of the product on its own and then mixes the rates as if nothing had happened
//     (src/likelihood.c:711-722, :730-743): where the categories of a site carry different counts its result is not
//     the posterior. Here the counts are honoured as they are for the edge log-likelihood and the ascertainment
//     terms (dna_site_add, k_edge_tiled): the site's smallest summed count is taken out, and rate k enters with
//     2^(-256 min(count_k - smallest, 4)) (minlh). Where all counts of a site are equal both agree.
// prop_invar is ignored, as in the reference. Only the `sites` real sites are written (no ascertainment entries).
//
// Two forms:
//   k_ancestral_dna<CTIP>          4 states x 4 rates, lane = site, one wave per 64-site tile as in k_edge_dna: all 32
//                                  (16 with tip codes) loads of the tile are issued before the arithmetic, the lane's
//                                  four results are 32 contiguous bytes and leave as two 16-byte stores (a wave writes
//                                  2 KB contiguous).
//   k_ancestral_tiled<ICH, CTIP>   any other shape, k_edge_tiled's walk (gen_tile): one workgroup per tile, wave w owns the rate
//                                  categories w, w + nw, ...; instead of one scalar per wave the per-state partial
//                                  sums sit in LDS ([wave][state][lane]), are added in wave order (deterministic),
//                                  normalised, and the tile's 64 x S results leave as one contiguous block.
#pragma once
#include "kernels_common.h"
#include "kernels_dna.h"
#include "kernels_generic.h"

// The edge as the log-likelihood kernels read it (parent = the node, child = the other end, mat on the child's
// side) and where the table goes. Of `e` the kernels use parent, child / ctip, pscaler, cscaler (per-rate mode only),
// mat, freqs, rate_weights, fidx, sites and per_rate.
struct DevAncestral
{
  DevEdge e;
  double *out; // [sites][S]
};

// 2^256 rides on every mix weight (see above)
#define PLLGPU_ANCESTRAL_LIFT 0x1p256

template <bool CTIP>
__global__ __launch_bounds__(256) void k_ancestral_dna(const DevAncestral a, unsigned tiles_per_wave)
{
  const DevEdge &e = a.e;
  cdouble_p pm = as_const(e.mat);
  const double none[4][4] = {};

  for (unsigned t = 0; t < tiles_per_wave; ++t)
  {
    DnaTile w;
    if (!dna_tile(w, blockIdx.x, tiles_per_wave, t, e.sites)) break;
    const unsigned nn = w.n;
    const unsigned ccode = CTIP ? e.ctip[nn] : 0u;
    const double *__restrict__ px = e.parent + w.off;
    const double *__restrict__ cx = CTIP ? nullptr : e.child + w.off;

    // every load of the tile first
    double xp[4][4], xc[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) dna_child_row<false>(xp[k], false, none, px, k, 0u);
#pragma unroll
    for (int k = 0; k < 4; ++k) dna_child_row<CTIP>(xc[k], false, none, cx, k, ccode);
    unsigned rs[4];
    unsigned scal = 0;
    if (e.per_rate) scal = dna_site_scalers(e, dna_load_scaler(e.pscaler, nn, 2), dna_load_scaler(e.cscaler, nn, 2), rs);

    double s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 4; ++k)
    {
      double tb[4];
      dna_matvec(tb, pm + k * 16, xc[k]);
      cdouble_p pi = as_const(e.freqs) + (size_t)e.fidx[k] * 4;
      double wk = e.rate_weights[k] * PLLGPU_ANCESTRAL_LIFT;
      if (e.per_rate) wk = rate_scaled(wk, rs[k], scal);
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] = fma(pi[j] * wk, xp[k][j] * tb[j], s[j]);
    }
    const double sum = ((s[0] + s[1]) + s[2]) + s[3];
    if (w.valid)
    {
      dbl2 lo, hi;
      lo.x = s[0] / sum;
      lo.y = s[1] / sum;
      hi.x = s[2] / sum;
      hi.y = s[3] / sum;
      dbl2 *o = reinterpret_cast<dbl2 *>(a.out + (size_t)nn * 4);
      o[0] = lo;
      o[1] = hi;
    }
  }
}

// dynamic LDS: [nw][S][64] partial sums, then [nw][64] partial row sums
template <int ICH, bool CTIP>
__global__ __launch_bounds__(256) void k_ancestral_tiled(const DevAncestral a, const GenGeo g, const unsigned long long *__restrict__ tipmap,
                                                         unsigned tiles_per_block)
{
  extern __shared__ double anc_lds[];
  const DevEdge &e = a.e;
  const unsigned lane = gen_lane(), wave = gen_wave();
  const unsigned nw = blockDim.x >> 6;
  double *mine = anc_lds + (size_t)wave * g.S * 64u + lane; // [state] at stride 64
  double *rowsum = anc_lds + (size_t)nw * g.S * 64u;        // [wave][lane]

  for (unsigned t = 0; t < tiles_per_block; ++t)
  {
    if (!gen_has_tile(tiles_per_block, t, e.sites)) break;
    const GenTile w = gen_tile(tiles_per_block, t, e.sites);
    const unsigned tile = w.tile, nn = w.nn; // tail lanes redo the last site, store nothing
    const unsigned long long cmask = CTIP ? tip_mask(tipmap, e.ctip[nn]) : 0ull;
    const double *__restrict__ px = e.parent + tiled_base(nn, g.tile_sz);
    const GenEnd ce = gen_end(e.mat, CTIP, e.child, nn, g, cmask);

    const unsigned scal = e.per_rate ? scaler_min(e.pscaler, nn, e.cscaler, nn, g.R) : 0u;

    // this wave's rate categories into its own slot
    bool first = true;
    for (unsigned k = wave; k < g.R; k += nw)
    {
      double wk = e.rate_weights[k] * PLLGPU_ANCESTRAL_LIFT;
      if (e.per_rate) wk = rate_scaled(wk, scaler_sum_rate(e.pscaler, nn, e.cscaler, nn, g.R, k), scal);
      for (unsigned c = 0; c < g.nchunks; ++c)
      {
        double B[ICH];
        end_contract<ICH>(B, ce, k, c, g);
        cdouble_p pi = as_const(e.freqs) + (size_t)e.fidx[k] * g.SP + c * ICH;
        const double *pk = px + ((size_t)k * g.S + c * ICH) * 64;
        double *dst = mine + (size_t)(c * ICH) * 64u;
#pragma unroll
        for (int i = 0; i < ICH; ++i)
          if (c * ICH + i < g.S)
          {
            const double v = __builtin_nontemporal_load(pk + (size_t)i * 64) * B[i];
            dst[i * 64] = first ? (pi[i] * wk) * v : fma(pi[i] * wk, v, dst[i * 64]);
          }
      }
      first = false;
    }
    if (first) // more waves than rate categories cannot happen (nw = min(R, 4)); keep the slot defined all the same
      for (unsigned j = 0; j < g.S; ++j) mine[j * 64u] = 0.0;
    lds_barrier();

    // the waves' partial sums in wave order: thread (wave, lane) takes states wave, wave + nw, ... of site `lane`
    double part = 0.0;
    for (unsigned j = wave; j < g.S; j += nw)
    {
      double *col = anc_lds + (size_t)j * 64u + lane;
      double v[1];
      wave_order_sums(v, col, nw, (size_t)g.S * 64u);
      col[0] = v[0];
      part += v[0];
    }
    rowsum[wave * 64u + lane] = part;
    lds_barrier();

    // normalise and write the tile's block of (up to) 64 x S results, contiguous in the output
    const unsigned first_site = tile * 64u;
    const unsigned count = (min(e.sites - first_site, 64u)) * g.S;
    double *o = a.out + (size_t)first_site * g.S;
    for (unsigned idx = threadIdx.x; idx < count; idx += blockDim.x)
    {
      const unsigned site = idx / g.S, j = idx - site * g.S;
      double sum[1];
      wave_order_sums(sum, rowsum + site, nw);
      o[idx] = anc_lds[(size_t)j * 64u + site] / sum[0];
    }
    lds_barrier(); // the slots are rewritten by the next tile
  }
}
