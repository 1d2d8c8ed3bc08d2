// kernels_category.h - the per-category site likelihoods of one edge, and what model optimisation makes of them:
// rate-category posteriors, empirical-Bayes site rates, the EM numerators of the category weights and EM steps on
// those weights (pll_gpu_edge_category_posteriors, pll_gpu_category_weights_em).
//
// For site n and rate category k, with x the parent end's CLV, y the other end (a CLV or tip codes), P the branch's
// transition matrix, pi_f(k) / p_f(k) the frequency set and prop_invar of category k, w the category weights, r the
// category rates and pw the pattern weights:
//
//     l[n][k] = sum_j pi_f(k)[j] x_k[n][j] (P_k y_k[n])[j]
//     s[n][k] = the scaling counts of both ends added: per site (the same for every k) or per rate
//     c[n]    = min_k s[n][k]
//     u[n][k] = l[n][k] * 2^(-256 min(s[n][k] - c[n], 4))            what the edge kernels mix (rate_scaled)
//     A[n][k] = w_k (1 - p_f(k)) u[n][k]
//     I[n][k] = w_k p_f(k) pi_f(k)[inv_n]   where p_f(k) > 0 and site n is invariant, else 0
//     site lnL = finish_site(sum_k A, sum_k I, c[n])                 (src/core_likelihood.c:1462-1481)
//     A *= 2^(-256 min(c[n], 4))   where c[n] > 0 and sum_k I > 0    (src/core_likelihood.c:1156-1174: finish_site's rule)
//     L[n]    = sum_k (A[n][k] + I[n][k])
//
//     cat_lnl[n][k]   = log(l[n][k]) - 256 ln2 * s[n][k]             exact: no cap, no weight, no pinv, no pattern weight
//     posterior[n][k] = (A[n][k] + I[n][k]) / L[n]
//     site_rates[n]   = sum_k (A[n][k] / L[n]) * r_k                 the invariant share has rate 0
//     weight_sums[k]  = sum_n pw[n] * posterior[n][k]                the EM numerator
//     lnl             = sum_n pw[n] * site lnL
//
// A site with L = 0 gets a zero posterior row and rate and adds nothing to weight_sums; lnl is then -inf.
//
// Three stages, ordered by the stream alone - no tickets, no hand-off between workgroups, no loop on the device:
//   A  k_category_dna<CTIP> / k_category_tiled<ICH, CTIP>   one launch: the table u as [k][sites rounded up to 64] and
//      one count word c[n] per site into scratch; cat_lnl, when asked, into its staging buffer in the host's layout
//      [n][k]. The 4 x 4 form is k_ancestral_dna's walk (lane = site, every load of the tile before the arithmetic);
//      the tiled form is gen_tile's walk and k_edge_tiled's rate term (one workgroup per tile, wave w owns the categories w, w + nw, ...) - but
//      the sum over the states is lane-local here: no LDS, no barrier.
//   B  k_category_mix   lane = site, min(ceil(sites / 256), 1024) workgroups of 256 walking the 256-site tiles at that
//      stride: reads the table (whole-wave contiguous per category), mixes it under ONE ROW of weights read from device
//      memory, stores posterior rows and site rates in the host's layout, and leaves R + 1 partial sums per workgroup
//      (wave_sum, then the four waves added in wave order through LDS) in partials[R + 1][B].
//   C  k_category_reduce   one workgroup: value v = its B partials added in ascending index order; one thread then
//      forms the next weight row S_k / (S_0 + ... + S_{R-1}) (added in that order) and writes {S, lnl} to the results.
// An EM step is B + C again under the row C has just written: the CLVs are read once per call, whatever the step count.
// The bits of every sum depend on the site count, the edge and the weight row alone.
#pragma once
#include "kernels_common.h"
#include "kernels_dna.h"
#include "kernels_generic.h"

// Stage A: the edge as the log-likelihood kernels read it (of `e`: parent, child / ctip, pscaler, cscaler, mat, freqs,
// fidx, sites, per_rate) and where its by-products go
struct DevCategory
{
  DevEdge e;
  double *table;    // [R][pad] u
  unsigned *count;  // [sites] c
  double *cat_lnl;  // [sites][R] or null
  unsigned pad;     // sites rounded up to 64
};

// log(l) with the (site, category)'s whole scaling count undone
__device__ __forceinline__ double category_lnl(double l, unsigned s)
{
  const double v = log(l);
  return s ? v + s * PLLGPU_LOG_THRESHOLD : v;
}

template <bool CTIP>
__global__ __launch_bounds__(256) void k_category_dna(const DevCategory a, unsigned tiles_per_wave)
{
  const DevEdge &e = a.e;
  cdouble_p pm = as_const(e.mat);
  const double none[4][4] = {};
  const int smode = e.per_rate ? 2 : 1;

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
    const unsigned scal = dna_site_scalers(e, dna_load_scaler(e.pscaler, nn, smode), dna_load_scaler(e.cscaler, nn, smode), rs);

    double l[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
    {
      double tb[4];
      dna_matvec(tb, pm + k * 16, xc[k]);
      l[k] = dna_rate_term(xp[k], as_const(e.freqs) + (size_t)e.fidx[k] * 4, tb);
    }
    if (!w.valid) continue;
#pragma unroll
    for (int k = 0; k < 4; ++k) a.table[(size_t)k * a.pad + nn] = e.per_rate ? rate_scaled(l[k], rs[k], scal) : l[k];
    a.count[nn] = scal;
    if (a.cat_lnl)
    {
      dbl2 lo, hi;
      lo.x = category_lnl(l[0], e.per_rate ? rs[0] : scal);
      lo.y = category_lnl(l[1], e.per_rate ? rs[1] : scal);
      hi.x = category_lnl(l[2], e.per_rate ? rs[2] : scal);
      hi.y = category_lnl(l[3], e.per_rate ? rs[3] : scal);
      dbl2 *o = reinterpret_cast<dbl2 *>(a.cat_lnl + (size_t)nn * 4);
      o[0] = lo;
      o[1] = hi;
    }
  }
}

template <int ICH, bool CTIP>
__global__ __launch_bounds__(256) void k_category_tiled(const DevCategory a, const GenGeo g, const unsigned long long *__restrict__ tipmap,
                                                        unsigned tiles_per_block)
{
  const DevEdge &e = a.e;
  const unsigned wave = gen_wave();
  const unsigned nw = blockDim.x >> 6;

  for (unsigned t = 0; t < tiles_per_block; ++t)
  {
    if (!gen_has_tile(tiles_per_block, t, e.sites)) break;
    const GenTile w = gen_tile(tiles_per_block, t, e.sites);
    const unsigned nn = w.nn; // tail lanes redo the last site, store nothing
    const bool valid = w.valid;
    const unsigned long long cmask = CTIP ? tip_mask(tipmap, e.ctip[nn]) : 0ull;
    const double *__restrict__ px = e.parent + tiled_base(nn, g.tile_sz);
    const GenEnd ce = gen_end(e.mat, CTIP, e.child, nn, g, cmask);

    const unsigned scal = site_scalings(e.pscaler, nn, e.cscaler, nn, g.R, e.per_rate);
    if (wave == 0 && valid) a.count[nn] = scal;

    for (unsigned k = wave; k < g.R; k += nw)
    {
      double tr = 0.0;
      for (unsigned c = 0; c < g.nchunks; ++c)
      {
        double B[ICH];
        end_contract<ICH>(B, ce, k, c, g);
        cdouble_p pi = as_const(e.freqs) + (size_t)e.fidx[k] * g.SP + c * ICH;
        tr = rate_term_add<ICH>(tr, px + ((size_t)k * g.S + c * ICH) * 64, 64u, pi, B, c, g);
      }
      if (!valid) continue;
      const unsigned sk = e.per_rate ? scaler_sum_rate(e.pscaler, nn, e.cscaler, nn, g.R, k) : scal;
      a.table[(size_t)k * a.pad + nn] = e.per_rate ? rate_scaled(tr, sk, scal) : tr;
      if (a.cat_lnl) a.cat_lnl[(size_t)nn * g.R + k] = category_lnl(tr, sk);
    }
  }
}

// Stage B: what the mix reads and writes. weights is ONE row of R category weights in device memory: the context's
// rate_weights, or row i of the EM call's array.
struct DevCategoryMix
{
  const double *table;     // [R][pad]
  const unsigned *count;   // [sites]
  const double *weights;   // [R]
  const double *freqs;     // [rate_matrices][SP]
  const double *prop_invar; // [rate_matrices] or null
  const double *rates;     // [R] (site_rates only)
  const int *invariant;    // [sites] or null
  const unsigned *pattern_weights;
  double *posterior;       // [sites][R] or null
  double *site_rates;      // [sites] or null
  double *partials;        // [R + 1][gridDim.x] or null: no sums asked
  unsigned sites, pad, R, SP;
  unsigned char fidx[kMaxRates];
};

// rides on every u of the ratios (k_category_mix)
#define PLLGPU_CATEGORY_LIFT 0x1p256

// A and I of (site, category) as the edge kernels form them (edge_rate_add, dna_site_add)
__device__ __forceinline__ void category_terms(const DevCategoryMix &m, unsigned k, double u, int inv, double &A, double &I)
{
  const unsigned fi = m.fidx[k];
  const double pinv = m.prop_invar ? m.prop_invar[fi] : 0.0;
  const double w = m.weights[k];
  I = 0.0;
  if (pinv > 0.0)
  {
    A = w * u * (1.0 - pinv);
    if (inv >= 0) I = w * m.freqs[(size_t)fi * m.SP + inv] * pinv;
  }
  else
    A = u * w;
}

// 2^256 A for the ratios. u (1 - p) is formed before the lift, as the reference forms it under a unit weight row: where
// u is subnormal that product is rounded to the subnormal grid once, there and here, and nothing else is.
__device__ __forceinline__ double category_lifted(const DevCategoryMix &m, unsigned k, double u)
{
  const double pinv = m.prop_invar ? m.prop_invar[m.fidx[k]] : 0.0;
  if (pinv > 0.0) u *= 1.0 - pinv;
  return (u * PLLGPU_CATEGORY_LIFT) * m.weights[k];
}

__global__ __launch_bounds__(256) void k_category_mix(const DevCategoryMix m)
{
  __shared__ double ws[kMaxRates + 1][4];
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const unsigned ntiles = (m.sites + 255u) / 256u;
  if (m.partials)
  {
    for (unsigned v = threadIdx.x; v < (m.R + 1u) * 4u; v += 256u) ws[v >> 2][v & 3u] = 0.0;
    __syncthreads();
  }

  for (unsigned tile = blockIdx.x; tile < ntiles; tile += gridDim.x)
  {
    const unsigned n = tile * 256u + threadIdx.x;
    const bool valid = n < m.sites;
    const unsigned nn = valid ? n : m.sites - 1;
    const unsigned c = m.count[nn];
    const int inv = m.invariant ? m.invariant[nn] : -1;
    const double *__restrict__ u = m.table + nn;

    // The site's sums twice: as the edge kernels form them, for the site lnL - and with 2^256 on every u, for the
    // ratios. A category 4 or more counts above the site's smallest enters as l 2^-1024, a subnormal number: its
    // product with the weight would be rounded to the subnormal grid once more (a relative error of 1e-6 and worse on
    // a posterior of about 2^-1024, which the reference's own per-category values do not carry). u <= 1 (a CLV entry
    // is a probability, or below 1 after its rescaling), so the lifted terms stay far from overflow; the factor
    // cancels in every ratio.
    double terma = 0.0, terminv = 0.0, lifted = 0.0;
    for (unsigned k = 0; k < m.R; ++k)
    {
      const double uk = u[(size_t)k * m.pad];
      double A, I;
      category_terms(m, k, uk, inv, A, I);
      terma += A;
      terminv += I;
      lifted += category_lifted(m, k, uk);
    }
    const double pw = valid ? (double)m.pattern_weights[nn] : 0.0;
    const double site = finish_site(terma, terminv, c, 0) * pw;
    // finish_site's rule for a scaled site with an invariant share: the variable share comes down to its true size
    const double adj = (c && terminv > 0.0) ? minlh(min(c, PLLGPU_RATE_MAXDIFF)) : 1.0;
    const double L = lifted * adj + terminv * PLLGPU_CATEGORY_LIFT;
    const double inv_ok = (terma * adj + terminv) > 0.0 ? 1.0 : 0.0; // L[n] > 0 as defined, without the lift

    double rate = 0.0;
    for (unsigned k = 0; k < m.R; ++k) // (the table's second reading comes from the cache)
    {
      double A, I;
      const double uk = u[(size_t)k * m.pad];
      category_terms(m, k, uk, inv, A, I);
      A = category_lifted(m, k, uk) * adj;
      I *= PLLGPU_CATEGORY_LIFT;
      const double post = inv_ok != 0.0 ? (A + I) / L : 0.0;
      if (m.site_rates && inv_ok != 0.0) rate += (A / L) * m.rates[k];
      if (m.posterior && valid) m.posterior[(size_t)nn * m.R + k] = post;
      if (m.partials)
      {
        const double s = wave_sum(valid ? pw * post : 0.0);
        if (lane == 0) ws[k][wave] += s;
      }
    }
    if (m.site_rates && valid) m.site_rates[nn] = rate;
    if (m.partials)
    {
      const double s = wave_sum(valid ? site : 0.0);
      if (lane == 0) ws[m.R][wave] += s;
    }
  }

  if (!m.partials) return;
  __syncthreads();
  if (threadIdx.x <= m.R) // the four waves in wave order
    m.partials[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = ((ws[threadIdx.x][0] + ws[threadIdx.x][1]) + ws[threadIdx.x][2]) + ws[threadIdx.x][3];
}

// Stage C. result: [R + 1] = {weight_sums, lnl} of this evaluation; next: the following weight row, or null.
// nparts <= 1024 (stage B's grid).
constexpr unsigned kCategoryReduceDoubles = 7u * 1025u; // 56 KB of LDS
__global__ __launch_bounds__(256) void k_category_reduce(const double *__restrict__ partials, unsigned nparts, unsigned R, double *__restrict__ result,
                                                         double *__restrict__ next)
{
  __shared__ double sums[kMaxRates + 1];
  __shared__ double rows[kCategoryReduceDoubles];
  // The partials of as many values as fit come into LDS with coalesced loads, a row per value at an odd stride (the
  // rows' walkers then sit on different banks); thread v adds row v one by one in ascending index order. All rate_cats + 1
  // values at once for up to 7 values of 1024 partials, round after round beyond. (One wave per value taking its partials
  // lane by lane through a cross-lane read measured 40 us at 391 partials: every read waited for the one before.)
  const unsigned stride = nparts | 1u;
  if (stride > kCategoryReduceDoubles) return; // (cannot happen: the grid of stage B ends at 1024)
  const unsigned per = min(R + 1u, kCategoryReduceDoubles / stride); // >= 7: nparts <= 1024
  for (unsigned v0 = 0; v0 <= R; v0 += per)
  {
    const unsigned nv = min(per, R + 1u - v0);
    for (unsigned idx = threadIdx.x; idx < nv * nparts; idx += blockDim.x)
    {
      const unsigned v = idx / nparts, i = idx - v * nparts;
      rows[v * stride + i] = partials[(size_t)(v0 + v) * nparts + i];
    }
    __syncthreads();
    if (threadIdx.x < nv)
    {
      const double *p = rows + threadIdx.x * stride;
      double s = 0.0;
#pragma unroll 8
      for (unsigned i = 0; i < nparts; ++i) s += p[i];
      sums[v0 + threadIdx.x] = s;
    }
    __syncthreads(); // rows[] is rewritten by the next round
  }
  if (threadIdx.x <= R) result[threadIdx.x] = sums[threadIdx.x];
  if (threadIdx.x == 0 && next)
  {
    double tot = 0.0;
    for (unsigned k = 0; k < R; ++k) tot += sums[k];
    for (unsigned k = 0; k < R; ++k) next[k] = sums[k] / tot;
  }
}
